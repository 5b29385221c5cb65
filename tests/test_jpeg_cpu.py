"""The device JPEG encoder without a GPU: the numpy oracle (tests/jpeg_oracle.py) against Pillow byte for byte, the host-only entries
wct_jpeg_header and wct_jpeg_bound against both, the refusals that need no device, the edge cases' claims, and the command line's
defaults."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import jpeg_cases as jc
from tests import jpeg_oracle as jo
from wct_hip import lib as _lib


def case_id(c):
    return "%dx%d-q%d-%s" % c


@pytest.mark.parametrize("case", jo.CASES, ids=case_id)
def test_oracle_equals_pillow(case):
    H, W, q, kind = case
    a = jo.make_image(H, W, kind)
    coef, data = jo.encode(a, q)
    assert coef.shape == (jc.num_blocks(H, W), 64) and coef.dtype == np.int16
    assert data == jo.pillow_bytes(a, q)


def test_default_quality_is_75():
    a = jo.make_image(18, 34, "noise")
    assert jo.pillow_bytes(a) == jo.pillow_bytes(a, 75) == jo.encode(a)[1]


@pytest.mark.parametrize("H,W", [(1, 1), (37, 29), (2160, 3840)])
@pytest.mark.parametrize("q", [1, 75, 100])
def test_header_equals_pillow(H, W, q):
    from wct_hip import WCT
    hdr, qy, qc = WCT.jpeg_header(H, W, q)
    a = np.zeros((H, W, 3), np.uint8)
    a[::2, ::2] = 255
    ref = jo.pillow_bytes(a, q)
    assert len(hdr) == _lib.JPEG_HEADER_BYTES == 623
    assert hdr == ref[:623] == jo.header(H, W, q)
    oy, oc = jo.quant_tables(q)
    assert np.array_equal(qy.ravel(), oy) and np.array_equal(qc.ravel(), oc)


def test_bound_covers_the_noise_cases_and_follows_its_formula():
    from wct_hip import WCT
    for H, W, q, kind in jo.CASES:
        bound = WCT.jpeg_bound(H, W)
        assert bound == 623 + 2 * jc.num_blocks(H, W) * (_lib.JPEG_BLOCK_MAX_BITS // 8) + 2
        if kind == "noise":
            assert bound >= len(jo.encode(jo.make_image(H, W, kind), q)[1])
    # the longest codes: 16 bits (the Annex K.3 tables have codes of every length up to 16) and 11 value bits (the largest DC category)
    assert _lib.JPEG_BLOCK_MAX_BITS == 64 * (16 + 11)
    assert max(l for t in jo.AC_CODES + jo.DC_CODES for _, l in t.values()) == 16


def test_host_entries_refuse_bad_arguments():
    L = _lib.load()
    hdr = (ctypes.c_uint8 * 623)()
    n = ctypes.c_uint64()
    for H, W, q in ((0, 8, 75), (8, 0, 75), (65501, 8, 75), (8, 65501, 75), (8, 8, 0), (8, 8, 101), (-1, 8, 75)):
        assert L.wct_jpeg_header(H, W, q, hdr, None, None) == _lib.WCT_ERR_INVALID
    assert L.wct_jpeg_header(8, 8, 75, None, None, None) == _lib.WCT_ERR_INVALID
    assert L.wct_jpeg_header(65500, 65500, 100, hdr, None, None) == _lib.WCT_OK
    for H, W in ((0, 8), (8, 0), (65501, 8), (8, 65501)):
        assert L.wct_jpeg_bound(H, W, ctypes.byref(n)) == _lib.WCT_ERR_INVALID
    assert L.wct_jpeg_bound(8, 8, None) == _lib.WCT_ERR_INVALID
    assert L.wct_jpeg_bound(65500, 65500, ctypes.byref(n)) == _lib.WCT_OK
    # no context: the device entries refuse before they touch anything
    assert L.wct_jpeg_blocks(None, 1, 8, 8, 75, 1) == _lib.WCT_ERR_INVALID
    assert L.wct_jpeg_pack(None, 1, 8, 8, 1, 16, 8) == _lib.WCT_ERR_INVALID
    assert L.wct_jpeg_encode(None, 1, 8, 8, 75, 1, 16, 8) == _lib.WCT_ERR_INVALID
    from wct_hip import WCT
    for bad in (0, 101, 75.0, True, "75"):
        with pytest.raises(ValueError):
            WCT.jpeg_header(8, 8, bad)
    with pytest.raises(ValueError):
        WCT.jpeg_bound(0, 8)


def test_header_symbol_list_and_library_agree():
    from tests.conftest import REPO
    text = open(os.path.join(REPO, "include", "wct_hip_jpeg.h")).read()
    declared = sorted(set(re.findall(r"\b(wct_[a-z_0-9]+)\s*\(", text)) - {"wct_ctx"})
    assert declared == sorted(_lib.SYMBOLS_JPEG) and len(declared) == 5
    assert not set(_lib.SYMBOLS_JPEG) & set(_lib.SYMBOLS)
    L = _lib.load()
    assert all(hasattr(L, s) for s in _lib.SYMBOLS_JPEG)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert set(_lib.SYMBOLS_JPEG) <= exported
    assert not [s for s in exported if "jpeg" in s.lower() and s not in _lib.SYMBOLS_JPEG], "the launchers and kernels stay inside the library"
    # the launchers' units, mirrored for the tests, are the header's
    for name in ("HEADER_BYTES", "MAX_DIM", "BLOCK_MAX_BITS", "SEG_MCUS", "SCAN_TILE", "SCAN_CHUNK", "PACK_SPAN", "STUFF_CHUNK"):
        m = re.search(r"#define WCT_JPEG_%s (\d+)" % name, text)
        assert m and int(m.group(1)) == getattr(_lib, "JPEG_" + name), name


def test_ff_tail_seed():
    a = jo.make_image(16, 16, "noise", jc.FF_TAIL_SEED)
    coef, data = jo.encode(a, 75)
    assert len(jo.bitstring(coef)) % 8 != 0, "the last byte must be a padded one"
    assert data[-4:] == b"\xff\x00\xff\xd9"
    assert data == jo.pillow_bytes(a, 75)


@pytest.mark.parametrize("edge", [e for e in jc.EDGES if e[1] * e[2] < 200000], ids=lambda e: e[0])
def test_edge_cases_are_where_they_claim(edge):
    name, H, W, quantity, relation, constant = edge
    assert H % 16 and W % 16, "ragged right and bottom MCUs"
    if quantity == "mcus_per_row":
        value = (W + 15) // 16
    elif quantity == "blocks":
        value = jc.num_blocks(H, W)
    else:
        value = (len(jo.bitstring(jo.coefficients(jo.make_image(H, W, "noise"), 75))) + 7) // 8
    assert jc.holds(value, relation, constant), (name, value, relation, constant)


def test_the_large_edge_case_has_two_steps_of_both_scans():
    name, H, W, quantity, relation, constant = jc.EDGES[-1]
    assert name == "two_scan_steps" and jc.holds(jc.num_blocks(H, W), relation, constant)
    # its stream: noise at quality 75 costs over a bit a pixel, and Pillow's file is the stream plus its stuffing, header and EOI
    stream_at_least = (len(jo.pillow_bytes(jo.make_image(H, W, "noise"), 75)) - 625) * 255 // 256 - 4096
    assert stream_at_least > _lib.JPEG_STUFF_CHUNK * _lib.JPEG_SCAN_CHUNK


def test_cli_defaults_and_refusals(tmp_path):
    from PIL import Image
    from wct_hip import cli
    args = cli.build_parser().parse_args([])
    assert args.device_jpeg is False and args.jpeg_quality == 75
    cli.check_jpeg_args(args)
    for q in ("0", "101"):
        with pytest.raises(ValueError):
            cli.check_jpeg_args(cli.build_parser().parse_args(["--jpeg_quality", q]))
    args = cli.build_parser().parse_args(["--device_jpeg", "--jpeg_quality", "90"])
    assert args.device_jpeg is True and args.jpeg_quality == 90
    cli.check_jpeg_args(args)
    # without the flags the host path writes the file it always wrote, and only .jpg / .jpeg outputs are the device's
    a = jo.make_image(41, 70, "noise")
    plain = cli.build_parser().parse_args([])
    for name in ("a.jpg", "a.jpeg", "a.png"):
        cli.save_host_u8(plain, a, str(tmp_path / name))
        Image.fromarray(a).save(tmp_path / ("ref_" + name))
        assert (tmp_path / name).read_bytes() == (tmp_path / ("ref_" + name)).read_bytes()
        assert cli.device_jpeg_wanted(plain, name) is False
        assert cli.device_jpeg_wanted(args, name) is (name != "a.png")
    cli.save_host_u8(args, a, str(tmp_path / "q90.jpg"))
    assert (tmp_path / "q90.jpg").read_bytes() == jo.pillow_bytes(a, 90)
