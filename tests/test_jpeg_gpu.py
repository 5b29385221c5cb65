"""The device JPEG encoder on the GPU (include/wct_hip_jpeg.h): the coefficients against the numpy oracle and the file against Pillow,
byte for byte -- on the cases the definition was checked on, on inputs that reach the coder's other branches, and at every edge of
the launchers; then what the entries promise about composition, overflow, views, graph replay and call history, and the command line."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from tests import jpeg_cases as jc
from tests import jpeg_oracle as jo
from tests.conftest import PKG, REPO
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


def case_id(c):
    return "%dx%d-q%d-%s" % c


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def first_difference(got, want):
    n = min(len(got), len(want))
    at = next((i for i in range(n) if got[i] != want[i]), n)
    return "lengths %d / %d, first difference at byte %d" % (len(got), len(want), at)


def check_file(torch, eng, a, q):
    got = eng.jpeg_encode(dev(torch, a), q)
    want = jo.pillow_bytes(a, q)
    assert got == want, first_difference(got, want)
    return got


@pytest.mark.parametrize("case", jo.CASES, ids=case_id)
def test_coefficients_equal_the_oracle(torch, eng, case):
    H, W, q, kind = case
    a = jo.make_image(H, W, kind)
    got = eng.jpeg_blocks(dev(torch, a), q).cpu().numpy()
    want = jo.coefficients(a, q)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%d coefficients differ, the first at (block, zig-zag position) %s" % (len(bad), tuple(bad[0]))


@pytest.mark.parametrize("case", jo.CASES, ids=case_id)
def test_bytes_equal_pillow(torch, eng, case):
    H, W, q, kind = case
    check_file(torch, eng, jo.make_image(H, W, kind), q)


def test_constant_image(torch, eng):
    """All EOB, every DC difference but the first zero."""
    a = np.full((40, 56, 3), 93, np.uint8)
    coef = eng.jpeg_blocks(dev(torch, a), 75).cpu().numpy()
    assert not coef[:, 1:].any()
    check_file(torch, eng, a, 75)


def test_checkerboard_has_zrl_runs(torch, eng):
    """A one-pixel checkerboard at quality 10: what survives the quantiser sits behind runs of more than 15 zeros."""
    yy, xx = np.mgrid[0:35, 0:52]
    a = (((yy + xx) & 1) * 255).astype(np.uint8)[..., None].repeat(3, 2)
    coef = jo.coefficients(a, 10)
    nz = [np.flatnonzero(b[1:]) for b in coef]
    assert any(len(i) and (i[0] > 15 or (np.diff(i) > 16).any()) for i in nz), "the input no longer produces a ZRL"
    assert np.array_equal(eng.jpeg_blocks(dev(torch, a), 10).cpu().numpy(), coef)
    check_file(torch, eng, a, 10)


def test_padded_last_byte_ff_is_stuffed(torch, eng):
    a = jo.make_image(16, 16, "noise", jc.FF_TAIL_SEED)
    got = check_file(torch, eng, a, 75)
    assert got[-4:] == b"\xff\x00\xff\xd9"


@pytest.mark.parametrize("edge", jc.EDGES, ids=lambda e: e[0])
def test_launcher_edges_equal_pillow(torch, eng, edge):
    name, H, W = edge[:3]
    check_file(torch, eng, jo.make_image(H, W, "noise"), 75)


def test_encode_is_the_composition_of_its_parts(torch, eng):
    for H, W, q, kind in ((41, 70, 90, "noise"), (130, 15, 85, "smooth"), (89, 101, 75, "noise")):
        a = jo.make_image(H, W, kind)
        x = dev(torch, a)
        whole = eng.jpeg_encode(x, q)
        hdr, _, _ = eng.jpeg_header(H, W, q)
        buf, length = eng.jpeg_pack(eng.jpeg_blocks(x, q), H, W)
        n = int(length.item())
        parts = hdr + buf[:n].cpu().numpy().tobytes()
        assert whole == parts, first_difference(whole, parts)
        assert buf[:n].cpu().numpy().tobytes() == jo.entropy(jo.coefficients(a, q))


def test_overflow_writes_nothing_beyond_the_capacity(torch, eng):
    a = jo.make_image(41, 70, "noise")
    x = dev(torch, a)
    want = jo.pillow_bytes(a, 90)
    n = len(want)
    for entry in ("encode", "pack"):
        exact = want if entry == "encode" else want[623:]
        m = len(exact)
        coef = eng.jpeg_blocks(x, 90)
        for cap, fits in ((m, True), (m - 1, False), (m - 2, False), (700 if entry == "encode" else 77, False), (0, False)):
            buf = torch.full((m + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            length = torch.zeros(1, dtype=torch.int64, device="cuda")
            if entry == "encode":
                eng.jpeg_encode_async(x, 90, capacity=cap, out=buf, length=length)
            else:
                eng.jpeg_pack(coef, 41, 70, capacity=cap, out=buf, length=length)
            host = buf.cpu().numpy()
            assert (host[cap:] == 0xA5).all(), "%s at capacity %d of %d wrote beyond it" % (entry, cap, m)
            if fits:
                assert int(length.item()) == m and host[:m].tobytes() == exact
            else:
                assert int(length.item()) == -1, "%s at capacity %d of %d: the length slot must be UINT64_MAX" % (entry, cap, m)
                assert ctypes.c_uint64(int(length.item())).value == _lib.JPEG_OVERFLOW
                assert host[:cap].tobytes() == exact[:cap], "what fits below the capacity is the file's start"
    assert eng.jpeg_encode(x, 90) == want      # the context is none the worse for it


def test_views_give_the_same_bytes(torch, eng):
    H, W = 37, 29
    a = jo.make_image(H, W, "smooth")
    want = jo.pillow_bytes(a, 75)
    for offset in (4, 12, 1, 3):
        big = torch.zeros(offset + H * W * 3 + 5, dtype=torch.uint8, device="cuda")
        view = big[offset:offset + H * W * 3].view(H, W, 3)
        view.copy_(dev(torch, a))
        assert eng.jpeg_encode(view, 75) == want, "image at byte offset %d" % offset
        # the output at that offset too
        out = torch.zeros(offset + len(want) + 3, dtype=torch.uint8, device="cuda")
        _, length = eng.jpeg_encode_async(view, 75, out=out[offset:])
        assert int(length.item()) == len(want) and out[offset:offset + len(want)].cpu().numpy().tobytes() == want


def test_history_and_poisoned_scratch(torch, eng):
    cases = [(41, 70, 90, "noise"), (17, 17, 75, "sat"), (130, 15, 85, "smooth")]
    want = [jo.pillow_bytes(jo.make_image(H, W, k), q) for H, W, q, k in cases]
    imgs = [dev(torch, jo.make_image(H, W, k)) for H, W, q, k in cases]
    for byte in (0xFF, 0x00, 0x5A):
        for i in (0, 1, 2, 1, 0):
            eng.debug_set("poison", byte)
            assert eng.jpeg_encode(imgs[i], cases[i][2]) == want[i], "case %d after poison 0x%02X" % (i, byte)
    eng.debug_set("poison", -1)
    from wct_hip import WCT
    fresh = WCT(types.SimpleNamespace(mode="16x", alpha=1.0))
    fresh.debug_set("poison", 0xFF)
    assert fresh.jpeg_encode(imgs[0], 90) == want[0], "a fresh context whose allocations are poisoned"
    fresh.debug_set("poison", -1)
    allocs = eng.debug_get("ws_allocs")
    eng.jpeg_encode(imgs[0], 90)
    eng.jpeg_encode(imgs[1], 75)
    assert eng.debug_get("ws_allocs") == allocs, "no allocation after the first call of a size"
    assert eng.saturation_count() == 0


def test_device_entries_refuse_bad_arguments(torch, eng):
    L, ctx = eng._lib, eng._ctx
    x = dev(torch, jo.make_image(16, 16, "noise"))
    coef = torch.full((6, 64), 7, dtype=torch.int16, device="cuda")
    buf = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
    length = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    p = lambda t: t.data_ptr()
    bad = [L.wct_jpeg_blocks(ctx, None, 16, 16, 75, p(coef)), L.wct_jpeg_blocks(ctx, p(x), 16, 16, 75, None),
           L.wct_jpeg_blocks(ctx, p(x), 0, 16, 75, p(coef)), L.wct_jpeg_blocks(ctx, p(x), 16, 65501, 75, p(coef)),
           L.wct_jpeg_blocks(ctx, p(x), 16, 16, 0, p(coef)), L.wct_jpeg_blocks(ctx, p(x), 16, 16, 101, p(coef)),
           L.wct_jpeg_blocks(ctx, p(x), 16, 16, 75, p(coef) + 2),
           L.wct_jpeg_pack(ctx, None, 16, 16, p(buf), 4096, p(length)), L.wct_jpeg_pack(ctx, p(coef), 16, 16, None, 4096, p(length)),
           L.wct_jpeg_pack(ctx, p(coef), 16, 16, p(buf), 4096, None), L.wct_jpeg_pack(ctx, p(coef), 16, 0, p(buf), 4096, p(length)),
           L.wct_jpeg_pack(ctx, p(coef), 65501, 16, p(buf), 4096, p(length)),
           L.wct_jpeg_encode(ctx, None, 16, 16, 75, p(buf), 4096, p(length)), L.wct_jpeg_encode(ctx, p(x), 16, 16, 75, None, 4096, p(length)),
           L.wct_jpeg_encode(ctx, p(x), 16, 16, 75, p(buf), 4096, None), L.wct_jpeg_encode(ctx, p(x), 16, 16, 0, p(buf), 4096, p(length)),
           L.wct_jpeg_encode(ctx, p(x), 16, 16, 101, p(buf), 4096, p(length)), L.wct_jpeg_encode(ctx, p(x), 0, 16, 75, p(buf), 4096, p(length)),
           L.wct_jpeg_encode(ctx, p(x), 16, 65501, 75, p(buf), 4096, p(length))]
    assert bad == [_lib.WCT_ERR_INVALID] * len(bad)
    assert "wct_jpeg_encode" in L.wct_last_error(ctx).decode()
    torch.cuda.synchronize()
    # ... before anything was written
    assert (buf == 0xA5).all() and int(length.item()) == 5 and (coef == 7).all()
    with pytest.raises(ValueError):
        eng.jpeg_encode(x, 0)
    with pytest.raises(ValueError):
        eng.jpeg_encode(x[:, :, :2], 75)


def test_encode_is_capturable_and_replays_on_other_pixels():
    """wct_jpeg_encode never synchronises, and its launches are a function of (H, W, capacity) alone: captured after a warm-up, the graph
    gives the bytes of whatever image its input buffer holds.  In a fresh process: a failed capture can leave the runtime in capture mode."""
    code = r"""
import sys, types
sys.path[:0] = [%r, %r]
import torch
from tests import jpeg_oracle as jo
from wct_hip import WCT
wct = WCT(types.SimpleNamespace(mode="16x", alpha=1.0))
H, W = 89, 101
a1, a2 = jo.make_image(H, W, "noise"), jo.make_image(H, W, "smooth")
x = torch.from_numpy(a1).cuda()
out = torch.zeros(wct.jpeg_bound(H, W), dtype=torch.uint8, device="cuda")
length = torch.zeros(1, dtype=torch.int64, device="cuda")
wct.jpeg_encode_async(x, 85, out=out, length=length)      # warm-up on the buffers the graph will use
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph):
    wct.jpeg_encode_async(x, 85, out=out, length=length)
for a in (a1, a2, a1):
    x.copy_(torch.from_numpy(a).cuda())
    out.zero_(); length.zero_()
    graph.replay()
    torch.cuda.synchronize()
    want = jo.pillow_bytes(a, 85)
    assert int(length.item()) == len(want) and out[:len(want)].cpu().numpy().tobytes() == want
print("GRAPH_OK")
""" % (REPO, PKG)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "GRAPH_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    """content/: three 96 x 128 images; style/: one 80 x 96."""
    from PIL import Image
    root = tmp_path_factory.mktemp("cli_jpeg")
    rng = np.random.default_rng(23)
    d = {k: root / k for k in ("content", "style")}
    for p in d.values():
        p.mkdir()

    def blocky(h, w):
        img = rng.random(((h + 3) // 4, (w + 3) // 4, 3)).repeat(4, 0).repeat(4, 1)[:h, :w] * 0.8 + rng.random((h, w, 3)) * 0.2
        return (img * 255).astype(np.uint8)

    for name in ("c1.png", "c2.png", "c3.png"):
        Image.fromarray(blocky(96, 128)).save(d["content"] / name)
    Image.fromarray(blocky(80, 96)).save(d["style"] / "s1.png")
    return d


def run_cli(folders, out, extra):
    from wct_hip import cli
    assert cli.main(["--mode", "16x", "--contentPath", str(folders["content"]), "--stylePath", str(folders["style"]), "--outf", str(out),
                     "--log_mark", "J"] + list(extra)) == 0
    return {f: (out / f).read_bytes() for f in sorted(os.listdir(out)) if f.endswith(".jpg")}


@pytest.fixture(scope="module")
def host_files(folders, tmp_path_factory):
    """What Pillow writes for the folder, per quality: the serial loop without --device_jpeg."""
    made = {}

    def get(quality):
        if quality not in made:
            out = tmp_path_factory.mktemp("host_q%s" % quality)
            made[quality] = run_cli(folders, out, ["--pipeline", "0"] + ([] if quality is None else ["--jpeg_quality", str(quality)]))
        return made[quality]
    return get


@pytest.mark.parametrize("quality", [None, 90], ids=["q-default", "q90"])
@pytest.mark.parametrize("pipeline", [0, 3], ids=["serial", "pipeline3"])
def test_cli_folder_is_byte_identical_with_the_flag(folders, host_files, tmp_path, pipeline, quality):
    want = host_files(quality)
    assert len(want) == 3
    q = [] if quality is None else ["--jpeg_quality", str(quality)]
    got = run_cli(folders, tmp_path, ["--pipeline", str(pipeline), "--device_jpeg"] + q)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], "%s: %s" % (name, first_difference(got[name], want[name]))
    if pipeline:      # and the pipelined loop without the flag still writes Pillow's files
        out = tmp_path / "host"
        out.mkdir()
        assert run_cli(folders, out, ["--pipeline", str(pipeline)] + q) == want
    if quality is not None:
        assert want != host_files(None), "--jpeg_quality must reach the host encoder too"


@pytest.mark.parametrize("mode", [["--video"], ["--proxy_scale", "2"]], ids=["video", "one-job-loop"])
def test_cli_other_loops_are_byte_identical_with_the_flag(folders, tmp_path, mode):
    """The video loop and the loop of the one-job-at-a-time modes save through the same helper."""
    out = {}
    for arm, extra in (("host", []), ("device", ["--device_jpeg"])):
        (tmp_path / arm).mkdir()
        out[arm] = run_cli(folders, tmp_path / arm, mode + ["--pipeline", "0", "--jpeg_quality", "60"] + extra)
    assert len(out["host"]) == 3 and sorted(out["host"]) == sorted(out["device"])
    for name in out["host"]:
        assert out["device"][name] == out["host"][name], "%s: %s" % (name, first_difference(out["device"][name], out["host"][name]))
