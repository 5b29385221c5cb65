"""Video mode without a GPU: the new public header and its bindings, wct_clip_bytes (host only), the identities of the numpy reference
(tests/video_oracle.py), and the command line's --video checks and frame order."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import video_oracle as O
from tests.conftest import PKG, REPO
from wct_hip import cli, lib

HEADER = os.path.join(REPO, "include", "wct_hip_video.h")
OTHER_LISTS = ("SYMBOLS", "SYMBOLS_COLOR", "SYMBOLS_SMOOTH", "SYMBOLS_TRANSFORM", "SYMBOLS_SWAP", "SYMBOLS_SCALE", "SYMBOLS_GUIDED")


# ---------------------------------------------------------------------------------------------------------------- header and bindings
def declared():
    return sorted(set(re.findall(r"\b(wct_[a-z_0-9]+)\s*\(", open(HEADER).read())) - {"wct_ctx"})


def test_header_and_symbol_list_agree():
    assert declared() and declared() == sorted(lib.SYMBOLS_VIDEO)
    assert len(set(lib.SYMBOLS_VIDEO)) == len(lib.SYMBOLS_VIDEO)
    for other in OTHER_LISTS:
        assert not set(lib.SYMBOLS_VIDEO) & set(getattr(lib, other)), other
    inc = os.path.join(REPO, "include")
    for name in os.listdir(inc):
        if name != "wct_hip_video.h":
            text = open(os.path.join(inc, name)).read()
            assert not set(lib.SYMBOLS_VIDEO) & set(re.findall(r"\b(wct_[a-z_0-9]+)\s*\(", text)), name
    text = open(HEADER).read()
    for name, value in (("WCT_CLIP_MAX_RADIUS", lib.CLIP_MAX_RADIUS), ("WCT_CLIP_RATE", lib.CLIP_RATE), ("WCT_CLIP_CUT", lib.CLIP_CUT),
                        ("WCT_CLIP_BLEND", lib.CLIP_BLEND), ("WCT_CLIP_SIGMA", lib.CLIP_SIGMA), ("WCT_CLIP_RADIUS", lib.CLIP_RADIUS)):
        m = re.search(r"#define %s\s+(\S+)" % name, text)
        assert m and float(m.group(1)) == float(value), name
    assert "a look, not a measurement" in text
    assert O.MAX_RADIUS == lib.CLIP_MAX_RADIUS
    fields = [f[0] for f in lib.WctClipParams._fields_]
    assert fields == ["rate", "cut", "blend", "sigma", "radius"] and ctypes.sizeof(lib.WctClipParams) == 32


def test_built_library_exports_the_video_entries_and_nothing_else_new():
    import __graft_entry__ as g
    g.build()
    L = lib.load()
    for s in lib.SYMBOLS_VIDEO:
        assert hasattr(L, s), s
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert set(lib.SYMBOLS_VIDEO) <= exported
    assert not [s for s in exported if re.search(r"clip_|temporal_blend|blend_tile", s) and s not in lib.SYMBOLS_VIDEO]     # the helpers stay hidden


def test_header_is_c99_clean_on_its_own(tmp_path):
    src = tmp_path / "only_video.c"
    src.write_text('#include "wct_hip_video.h"\n'
                   "int main(void) { wct_clip_params p = { WCT_CLIP_RATE, WCT_CLIP_CUT, (float)WCT_CLIP_BLEND, (float)WCT_CLIP_SIGMA, WCT_CLIP_RADIUS };\n"
                   "  return (p.radius <= WCT_CLIP_MAX_RADIUS && sizeof(wct_clip_params) == 32) ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"), "-c", str(src), "-o",
                    str(tmp_path / "only_video.o")], check=True)


def test_the_tile_the_gpu_test_names_is_the_kernels():
    text = open(os.path.join(PKG, "csrc", "video.hip")).read()
    m = re.search(r"TB_W = (\d+), TB_H = (\d+);", text)
    assert m and (int(m.group(1)), int(m.group(2))) == (O.TILE_W, O.TILE_H)
    assert "sat_raise(" not in text                                        # nothing here clamps: the range flag is the cascade's
    build = open(os.path.join(PKG, "build.sh")).read()
    assert re.search(r'^SRC=".*\bvideo\b.*\bapi_video\b.*"', build, re.M) and "../include/wct_hip_video.h" in build


# ---------------------------------------------------------------------------------------------------------------- wct_clip_bytes
def test_clip_bytes_values_and_refusals():
    L = lib.load()
    n = ctypes.c_size_t(7)

    def call(H, W, C, out=n):
        arr = (ctypes.c_int * 5)(*C) if C is not None else None
        return L.wct_clip_bytes(H, W, arr, ctypes.byref(out) if out is not None else None)

    c16 = (128, 128, 64, 32, 24)
    for H, W, C in ((96, 128, c16), (100, 135, c16), (2160, 3840, c16), (32, 32, (1, 1, 1, 1, 1)), (47, 500, (512, 512, 256, 128, 64)), (96, 128, (17,) * 5)):
        assert call(H, W, C) == lib.WCT_OK and n.value == O.clip_bytes(H, W, C), (H, W, C)
    # by hand: 96 x 128, five levels of one channel: sums 2 doubles each = 80 bytes -> 256; flags 256; an image 3 * 96 * 128 * 4
    assert call(96, 128, (1,) * 5) == lib.WCT_OK and n.value == 2 * 256 + 256 + 3 * 147456
    assert call(100, 135, (1,) * 5) == lib.WCT_OK and n.value == 2 * 256 + 256 + 3 * 147456      # floored to multiples of 16
    n.value = 7
    for H, W, C, out in ((31, 128, c16, n), (96, 31, c16, n), (0, 0, c16, n), (96, 128, None, n), (96, 128, c16, None), (96, 128, (0, 128, 64, 32, 24), n),
                         (96, 128, (513, 128, 64, 32, 24), n), (96, 128, (128, 128, 64, 32, -4), n)):
        assert call(H, W, C, out) == lib.WCT_ERR_INVALID, (H, W, C)
    assert n.value == 7                                                     # untouched by every refusal


def test_a_null_context_is_refused_by_every_entry():
    L = lib.load()
    p = lib.WctClipParams(0.25, 0.5, 0.6, 0.05, 2)
    h = ctypes.c_void_p()
    assert L.wct_clip_create(None, 96, 128, ctypes.byref(p), ctypes.byref(h)) == lib.WCT_ERR_INVALID and not h.value
    assert L.wct_clip_reset(None, None) == lib.WCT_ERR_INVALID
    assert L.wct_clip_export(None, None, 5, None, None, None) == lib.WCT_ERR_INVALID
    assert L.wct_moments_track(None, None, 5, 1, None, None) == lib.WCT_ERR_INVALID
    assert L.wct_temporal_blend(None, None, 1, 1, None, None, None, 1, 1, 0.5, 0.05, 2, None, None, None, 0) == lib.WCT_ERR_INVALID
    assert L.wct_stylize_clip(None, None, None, 96, 128, 1.0, None, None, 0, None, None) == lib.WCT_ERR_INVALID
    L.wct_clip_destroy(None, None)                                          # ignored


# ---------------------------------------------------------------------------------------------------------------- oracle identities
def test_track_identities():
    rng = np.random.default_rng(3)
    r, c = rng.random(300) * 1e3, rng.random(300) * 1e3
    for rate in (1.0, 0.25, 0.7, 1e-3):
        assert np.array_equal(O.track(r, r.copy(), rate, False), r)                  # c == r gives r
        assert np.array_equal(O.track(r, c, rate, True), c)                          # a cut gives c
    assert np.array_equal(O.track(r, c, 1.0, False), c)                              # rate == 1 gives c
    assert np.array_equal(O.track(np.array([1e16]), np.array([1.0]), 1.0, False), [1.0])     # ... exactly, where (c - r) + r would round
    mid = O.track(r, c, 0.25, False)
    assert np.all((mid >= np.minimum(r, c)) & (mid <= np.maximum(r, c))) and np.abs(mid - (0.75 * r + 0.25 * c)).max() < 1e-12 * 1e3
    assert np.array_equal(mid, r + 0.25 * (c - r))


def test_decision():
    rng = np.random.default_rng(4)
    X = rng.random((8, 48))
    s, ss = X.sum(1), X @ X.T
    assert O.decision(48.0, s, s, ss, 0, np.inf) == (True, 0.0)                      # the first frame: a cut whatever D is
    assert O.decision(48.0, s, s, ss, 3, 0.5) == (False, 0.0)
    assert O.decision(48.0, s, s, ss, 3, 0.0) == (False, 0.0)                        # D == 0 <= 0: the same frame is no cut even at cut = 0
    Y = X + 1.0
    cut, D = O.decision(48.0, Y.sum(1), s, ss, 3, 0.5)
    var = (X.var(1)).sum()
    assert cut and abs(D - 8.0 / var) < 1e-9 * D                                     # every mean moved by 1
    assert not O.decision(48.0, Y.sum(1), s, ss, 3, np.inf)[0]
    bad = s.copy()
    bad[2] = np.nan
    assert O.decision(48.0, bad, s, ss, 3, np.inf)[0]                                # NaN counts as a cut
    assert O.decision(48.0, s, np.zeros(8), np.zeros((8, 8)), 3, 1e300)[0]           # no running variance: D = |mu|^2 / DBL_MIN = inf


def test_blend_identities_and_bound():
    cur, s, p = O.image((20, 30), 1), O.image((17, 25), 2), O.image((17, 25), 3)
    prev = cur[:, :17, :25].copy()
    assert np.array_equal(O.blend(cur, prev, s, s, 0.6, 0.05, 2), s.astype(np.float64))          # p == s gives s
    assert np.array_equal(O.blend(cur, prev, s, p, 0.6, 0.05, 2, cut=True), s.astype(np.float64))
    assert np.array_equal(O.blend(cur, prev, s, p, 0.0, 0.05, 2), s.astype(np.float64))          # blend 0: off
    still = O.blend(cur, prev, s, p, 0.6, 0.05, 8)                                               # the content did not move: w = blend everywhere
    assert np.abs(still - (s + float(np.float32(0.6)) * (p.astype(np.float64) - s))).max() < 1e-15
    moved = O.blend(cur, prev + 1.0, s, p, 0.6, 0.05, 0)                                         # it moved a lot: w = 0.6 exp(-3 / 0.005) = 0
    assert np.abs(moved - s).max() < 1e-300
    e = np.arange(12.0).reshape(3, 4)
    assert np.array_equal(O.window_mean(e, 0), e)
    assert np.allclose(O.window_mean(e, 8), e.mean())                                            # a radius larger than the image: the whole image
    assert O.window_mean(e, 1)[0, 0] == (0 + 1 + 4 + 5) / 4.0                                    # divided by the CLIPPED count
    assert O.blend_bound(2, 0.6, p, s) == 2 * 2.0 ** -24 * ((0.368 * 30 + 3) * 0.6 * float(np.abs(p.astype(np.float64) - s).max())
                                                             + 4 * max(float(np.abs(s).max()), float(np.abs(p).max())))


# ---------------------------------------------------------------------------------------------------------------- command line
def parse(*argv):
    args = cli.build_parser().parse_args(list(argv))
    cli.checkpoint_args(args)
    return args


def test_video_defaults_and_refusals():
    args = parse("--video", "--mode", "16x")
    cli.check_video_args(args)
    assert (args.temporal_rate, args.scene_cut, args.temporal_blend, args.temporal_sigma, args.temporal_radius) == \
        (lib.CLIP_RATE, lib.CLIP_CUT, lib.CLIP_BLEND, lib.CLIP_SIGMA, lib.CLIP_RADIUS)
    cli.check_video_args(parse("--video", "--mode", "16x_kd2sd", "--transform", "ot", "--alpha", "0.6", "--scene_cut", "inf", "--temporal_blend", "0"))
    cli.check_video_args(parse("--mode", "16x"))                                                  # without --video: nothing to check
    for flag, value in (("--temporal_rate", "0.5"), ("--scene_cut", "1"), ("--temporal_blend", "0.5"), ("--temporal_sigma", "0.1"),
                        ("--temporal_radius", "1")):
        with pytest.raises(ValueError, match="%s does nothing without --video" % flag):
            cli.check_video_args(parse("--mode", "16x", flag, value))
    for extra, name in ((["--maskPath", "m", "--region_styles", "a.jpg"], "--maskPath"), (["--interp_styles", "a.jpg,b.jpg"], "--interp_styles"),
                        (["--swap_level", "4"], "--swap_level"), (["--level_scale", "4,4,2,1,1"], "--level_scale"), (["--auto_regions", "3"], "--auto_regions"),
                        (["--synthesis"], "--synthesis"), (["--preserve_color", "luma"], "--preserve_color"), (["--smooth_radius", "4"], "--smooth_radius")):
        with pytest.raises(ValueError, match="--video does not mix with .*%s" % name):
            cli.check_video_args(parse("--video", "--mode", "16x", *extra))
    for mode in (["--mode", "original"], []):
        with pytest.raises(ValueError, match="--mode original"):
            cli.check_video_args(parse("--video", *mode))
    with pytest.raises(ValueError, match="--num_run"):
        cli.check_video_args(parse("--video", "--mode", "16x", "--num_run", "2"))
    for flag, value in (("--temporal_rate", "0"), ("--temporal_rate", "1.5"), ("--temporal_rate", "nan"), ("--scene_cut", "-1"), ("--scene_cut", "nan"),
                        ("--temporal_blend", "1"), ("--temporal_blend", "-0.1"), ("--temporal_sigma", "0"), ("--temporal_sigma", "inf"),
                        ("--temporal_radius", "9"), ("--temporal_radius", "-1")):
        with pytest.raises(ValueError, match=flag):
            cli.check_video_args(parse("--video", "--mode", "16x", flag, value))


def test_frames_of_differing_size_are_refused_by_name():
    args = parse("--video", "--mode", "16x")
    cli.check_video_args(args, [("f000.png", (96, 128)), ("f001.png", (96, 128))])
    with pytest.raises(ValueError, match=r"frame f002\.png is 130x96.*f000\.png is 128x96"):
        cli.check_video_args(args, [("f000.png", (96, 128)), ("f001.png", (96, 128)), ("f002.png", (96, 130))])


def test_frames_are_the_picked_content_files_sorted_by_name(tmp_path):
    for name in ("f010.png", "f002.png", "g001.png", "f001.jpg", "notes.txt", "f003.png"):
        (tmp_path / name).write_bytes(b"")
    assert cli.video_frames(str(tmp_path)) == ["f001.jpg", "f002.png", "f003.png", "f010.png", "g001.png"]
    assert cli.video_frames(str(tmp_path), "f0") == ["f001.jpg", "f002.png", "f003.png", "f010.png"]
