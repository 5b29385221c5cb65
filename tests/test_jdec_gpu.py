"""The device JPEG decoder on the GPU (include/wct_hip_jdec.h): the pixels against Pillow and the coefficients against the oracle
(tests/jdec_oracle.py) on every case of tests/jdec_cases.py and at the edges of the schedule; the round trips with the device encoder;
the status word; and what the entries promise about composition, views, call history and bad arguments."""
import ctypes
import types

import numpy as np
import pytest

from tests import jdec_cases as jc
from tests import jdec_oracle as jd
from tests import jpeg_oracle as jo
from wct_hip import lib as _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "-m gpu tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def eng(torch):
    from wct_hip import WCT
    return WCT(types.SimpleNamespace(mode="16x", alpha=1.0))


def scan_of(torch, data, info):
    seg = np.frombuffer(data, np.uint8, int(info.scan_length), int(info.scan_offset)).copy()
    return torch.from_numpy(seg).cuda()


def check_pixels(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d values differ, the first at (y, x, channel) %s" % (what, len(bad), tuple(bad[0]))


def check_file(torch, eng, data, what, coefficients=True):
    """Pixels = Pillow's, coefficients = the oracle's, status OK, and wct_jdec_decode = its composition."""
    info = eng.jdec_parse(data)
    assert info is not None, what
    scan = scan_of(torch, data, info)
    px, status = eng.jdec_decode_async(scan, info)
    assert int(status.item()) == _lib.JDEC_STATUS_OK, what
    check_pixels(px, jd.pillow_pixels(data), what)
    coef, status = eng.jdec_coefficients(scan, info)
    assert int(status.item()) == _lib.JDEC_STATUS_OK, what
    assert torch.equal(eng.jdec_pixels(coef, info), px), "%s: wct_jdec_decode is not its composition" % what
    if coefficients:
        want, st = jd.decoder(data).coefficients()
        assert st == jd.OK
        got = coef.cpu().numpy()
        bad = np.argwhere(got != want)
        assert bad.size == 0, "%s: %d coefficients differ, the first at (block, zig-zag position) %s" % (what, len(bad), tuple(bad[0]))
    return info, scan, px


@pytest.mark.parametrize("case", jc.CASES, ids=jc.case_id)
def test_pixels_equal_pillow_and_coefficients_the_oracle(torch, eng, case):
    check_file(torch, eng, jc.case_bytes(case), jc.case_id(case))


@pytest.mark.parametrize("name", sorted(jc.EDGES))
def test_schedule_edges(torch, eng, name):
    check_file(torch, eng, jc.EDGES[name](), name)


def test_large_photograph_takes_two_steps_of_every_scan(torch, eng):
    """Pixels only: the oracle's Python decoder is not for 4 megapixels."""
    data = jc.large()
    info, _, _ = check_file(torch, eng, data, "large", coefficients=False)
    assert eng.jdec_num_blocks(info) // 3 > _lib.JDEC_DC_TILE * _lib.JDEC_SCAN_CHUNK
    assert int(info.scan_length) > _lib.JDEC_CHUNK * _lib.JDEC_SCAN_CHUNK


def test_round_trip_with_the_device_encoder(torch, eng):
    """wct_jdec_coefficients(wct_jpeg_encode(img)) = wct_jpeg_blocks(img), and wct_jpeg_pack of the decoded coefficients is the
    file's segment byte for byte (standard tables, 4:2:0)."""
    for H, W, q, kind in ((41, 70, 90, "noise"), (130, 15, 85, "smooth"), (89, 101, 75, "smooth")):
        x = torch.from_numpy(jo.make_image(H, W, kind)).cuda()
        data = eng.jpeg_encode(x, q)
        info = eng.jdec_parse(data)
        coef, status = eng.jdec_coefficients(scan_of(torch, data, info), info)
        assert int(status.item()) == _lib.JDEC_STATUS_OK
        assert torch.equal(coef, eng.jpeg_blocks(x, q)), (H, W, q, kind)
        buf, length = eng.jpeg_pack(coef, H, W)
        n = int(length.item())
        assert buf[:n].cpu().numpy().tobytes() == data[int(info.scan_offset):], (H, W, q, kind)


def test_status_unsync_and_ok_on_the_photo_crop(torch, eng):
    data = jc.photo_crop()
    info = eng.jdec_parse(data)
    scan = scan_of(torch, data, info)
    px, status = eng.jdec_decode_async(scan, info, rounds=1)
    assert int(status.item()) == _lib.JDEC_STATUS_UNSYNC
    px, status = eng.jdec_decode_async(scan, info, rounds=0)
    assert int(status.item()) == _lib.JDEC_STATUS_OK
    check_pixels(px, jd.pillow_pixels(data), "photo crop")


def test_status_follows_the_oracle_on_every_rounds_value(torch, eng):
    """The status is a function of the file and `rounds`: the oracle's restatement of the schedule predicts it."""
    data = jc.saturated()
    d = jd.decoder(data)
    info = eng.jdec_parse(data)
    scan = scan_of(torch, data, info)
    seen = set()
    for rounds in (1, 2, 4, 8, 16, 32, 64):
        want = d.status(rounds)
        seen.add(want)
        assert int(eng.jdec_coefficients(scan, info, rounds)[1].item()) == want, rounds
    assert seen == {jd.OK, jd.UNSYNC}, "the case no longer has both outcomes"


def test_flipped_bits_never_give_wrong_pixels_under_ok(torch, eng):
    case = (41, 70, "noise", "420", 75)
    data = jc.case_bytes(case)
    base = eng.jdec_parse(data)
    outcomes = set()
    for k, at in enumerate(range(int(base.scan_offset) + 3, int(base.scan_offset + base.scan_length) - 3, 97)):
        bad = bytearray(data)
        bad[at] ^= 1 << (k % 8)
        bad = bytes(bad)
        info = eng.jdec_parse(bad)
        if info is None:
            continue
        px, status = eng.jdec_decode_async(scan_of(torch, bad, info), info, rounds=4096)
        status = int(status.item())
        d = jd.decoder(bad)
        coef, want = d.coefficients()
        assert status == want, "flip at byte %d" % at
        outcomes.add(status)
        if status == _lib.JDEC_STATUS_OK:
            check_pixels(px, jd.pixels(coef, d.f), "flip at byte %d" % at)
    assert _lib.JDEC_STATUS_CORRUPT in outcomes


def test_views_and_odd_alignments_of_the_segment(torch, eng):
    data = jc.case_bytes((37, 29, "smooth", "420rb3", 85))
    info = eng.jdec_parse(data)
    want = jd.pillow_pixels(data)
    seg = np.frombuffer(data, np.uint8, int(info.scan_length), int(info.scan_offset)).copy()
    for offset in (1, 3, 4, 13):
        big = torch.full((offset + len(seg) + 7,), 0xFF, dtype=torch.uint8, device="cuda")
        big[offset:offset + len(seg)] = torch.from_numpy(seg).cuda()
        out = torch.zeros(offset + want.size + 3, dtype=torch.uint8, device="cuda")
        view = out[offset:offset + want.size].view(*want.shape)
        _, status = eng.jdec_decode_async(big[offset:offset + len(seg)], info, out=view)
        assert int(status.item()) == _lib.JDEC_STATUS_OK
        check_pixels(view, want, "segment and image at byte offset %d" % offset)
        assert int(out[:offset].sum().item()) == 0 and int(out[offset + want.size:].sum().item()) == 0


def test_history_and_poisoned_scratch(torch, eng):
    cases = [(41, 70, "noise", "420", 75), (9, 7, "noise", "grey", 10), (48, 80, "smooth", "422opt-rb1", 95)]
    files = [jc.case_bytes(c) for c in cases]
    want = [jd.pillow_pixels(f) for f in files]

    def run(e, i):
        out, status = e.jdec_decode(files[i])
        assert status == _lib.JDEC_STATUS_OK
        check_pixels(out, want[i], "case %d" % i)

    for byte in (0xFF, 0x00, 0x5A):
        for i in (0, 1, 2, 1, 0):
            eng.debug_set("poison", byte)
            run(eng, i)
    eng.debug_set("poison", -1)
    from wct_hip import WCT
    fresh = WCT(types.SimpleNamespace(mode="16x", alpha=1.0))
    fresh.debug_set("poison", 0xFF)
    run(fresh, 0)
    fresh.debug_set("poison", -1)
    allocs = eng.debug_get("ws_allocs")
    run(eng, 0)
    run(eng, 1)
    assert eng.debug_get("ws_allocs") == allocs, "no allocation after the first call of a size"


def test_device_entries_refuse_bad_arguments(torch, eng):
    L, ctx = eng._lib, eng._ctx
    data = jc.case_bytes((16, 16, "noise", "420", 75))
    info = eng.jdec_parse(data)
    scan = scan_of(torch, data, info)
    coef = torch.full((6, 64), 7, dtype=torch.int16, device="cuda")
    img = torch.full((16, 16, 3), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((2,), 5, dtype=torch.int32, device="cuda")
    p = lambda t: t.data_ptr()
    ref = ctypes.byref
    broken = _lib.WctJdecInfo.from_buffer_copy(info)
    broken.ncomp = 2
    zero_q = _lib.WctJdecInfo.from_buffer_copy(info)
    zero_q.qt[0][5] = 0
    bad = [L.wct_jdec_coefficients(ctx, None, ref(info), 0, p(coef), p(status)), L.wct_jdec_coefficients(ctx, p(scan), None, 0, p(coef), p(status)),
           L.wct_jdec_coefficients(ctx, p(scan), ref(info), 0, None, p(status)), L.wct_jdec_coefficients(ctx, p(scan), ref(info), 0, p(coef), None),
           L.wct_jdec_coefficients(ctx, p(scan), ref(info), -1, p(coef), p(status)), L.wct_jdec_coefficients(ctx, p(scan), ref(info), 4097, p(coef), p(status)),
           L.wct_jdec_coefficients(ctx, p(scan), ref(info), 0, p(coef) + 2, p(status)), L.wct_jdec_coefficients(ctx, p(scan), ref(info), 0, p(coef), p(status) + 2),
           L.wct_jdec_coefficients(ctx, p(scan), ref(broken), 0, p(coef), p(status)), L.wct_jdec_coefficients(ctx, p(scan), ref(zero_q), 0, p(coef), p(status)),
           L.wct_jdec_pixels(ctx, None, ref(info), p(img)), L.wct_jdec_pixels(ctx, p(coef), ref(info), None), L.wct_jdec_pixels(ctx, p(coef), ref(broken), p(img)),
           L.wct_jdec_pixels(ctx, p(coef) + 2, ref(info), p(img)),
           L.wct_jdec_decode(ctx, None, ref(info), 0, p(img), p(status)), L.wct_jdec_decode(ctx, p(scan), None, 0, p(img), p(status)),
           L.wct_jdec_decode(ctx, p(scan), ref(info), 0, None, p(status)), L.wct_jdec_decode(ctx, p(scan), ref(info), 0, p(img), None),
           L.wct_jdec_decode(ctx, p(scan), ref(info), 5000, p(img), p(status)), L.wct_jdec_decode(ctx, p(scan), ref(broken), 0, p(img), p(status))]
    assert bad == [_lib.WCT_ERR_INVALID] * len(bad)
    assert "wct_jdec_decode" in L.wct_last_error(ctx).decode()
    torch.cuda.synchronize()
    # ... before anything was written
    assert (img == 0xA5).all() and (status == 5).all() and (coef == 7).all()
    with pytest.raises(ValueError):
        eng.jdec_decode_async(scan, info, rounds=-1)
    with pytest.raises(ValueError):
        eng.jdec_decode_async(scan[:-1], info)


# ---- the command line -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    """content/: 96 x 128 images as baseline, optimised 4:4:4, restart-marker, progressive (falls back), PNG (untouched) and a baseline
    file with one flipped bit that the device finds CORRUPT and Pillow still opens (redone from Pillow's decode); style/: one 80 x 96."""
    import io
    from PIL import Image
    root = tmp_path_factory.mktemp("cli_jdec")
    rng = np.random.default_rng(29)
    d = {k: root / k for k in ("content", "style")}
    for p in d.values():
        p.mkdir()

    def blocky(h, w):
        img = rng.random(((h + 3) // 4, (w + 3) // 4, 3)).repeat(4, 0).repeat(4, 1)[:h, :w] * 0.8 + rng.random((h, w, 3)) * 0.2
        return (img * 255).astype(np.uint8)

    Image.fromarray(blocky(96, 128)).save(d["content"] / "c1.jpg", quality=90)
    Image.fromarray(blocky(96, 128)).save(d["content"] / "c2.jpg", quality=85, optimize=True, subsampling=0)
    Image.fromarray(blocky(96, 128)).save(d["content"] / "c3.jpeg", quality=75, restart_marker_blocks=2)
    Image.fromarray(blocky(96, 128)).save(d["content"] / "c4.jpg", quality=75, progressive=True)
    Image.fromarray(blocky(96, 128)).save(d["content"] / "c5.png")
    good = jc.save(blocky(96, 128), 80, subsampling=2)
    f = jd.parse(good)
    for at in range(f["scan_offset"] + f["scan_length"] // 2, f["scan_offset"] + f["scan_length"] - 2):
        bad = bytearray(good)
        bad[at] ^= 0x10
        bad = bytes(bad)
        try:
            if jd.decoder(bad).coefficients()[1] == jd.CORRUPT:
                Image.open(io.BytesIO(bad)).convert("RGB")
                break
        except (jd.Unsupported, OSError):
            continue
    else:
        raise AssertionError("no flipped bit gives a CORRUPT file that Pillow opens")
    (d["content"] / "c6.jpg").write_bytes(bad)
    Image.fromarray(blocky(80, 96)).save(d["style"] / "s1.jpg", quality=95)
    return d


def run_cli(folders, out, extra):
    import os
    from wct_hip import cli
    assert cli.main(["--mode", "16x", "--contentPath", str(folders["content"]), "--stylePath", str(folders["style"]), "--outf", str(out),
                     "--log_mark", "D"] + list(extra)) == 0
    log = "".join(open(out / f).read() for f in os.listdir(out) if f.startswith("log_"))
    return {f: (out / f).read_bytes() for f in sorted(os.listdir(out)) if f.endswith(".jpg")}, log


@pytest.fixture(scope="module")
def host_files(folders, tmp_path_factory):
    return run_cli(folders, tmp_path_factory.mktemp("host"), ["--pipeline", "0"])[0]


@pytest.mark.parametrize("pipeline", [0, 3], ids=["serial", "pipeline3"])
def test_cli_folder_is_byte_identical_with_the_flag(folders, host_files, tmp_path, pipeline):
    assert len(host_files) == 6
    got, log = run_cli(folders, tmp_path, ["--pipeline", str(pipeline), "--device_decode"])
    assert sorted(got) == sorted(host_files)
    for name in host_files:
        assert got[name] == host_files[name], name
    notes = [l for l in log.splitlines() if "--device_decode:" in l]
    assert len(notes) == 2 and any("c4.jpg" in l and "not a baseline file" in l for l in notes) and any("c6.jpg" in l and "CORRUPT" in l for l in notes), notes
    # and with the device encoder beside it
    (tmp_path / "both").mkdir()
    assert run_cli(folders, tmp_path / "both", ["--pipeline", str(pipeline), "--device_decode", "--device_jpeg"])[0] == host_files


def test_cli_without_the_flag_decodes_nothing_on_the_device(folders, host_files, tmp_path):
    from wct_hip import cli
    got, log = run_cli(folders, tmp_path, ["--pipeline", "3"])
    assert got == host_files and "--device_decode:" not in log and cli._DEVICE_DECODER is None
