"""Texture synthesis on the device: the noise kernel against its definition (bit for bit), wct_synthesize against the calls it is
made of (bit for bit -- which puts it under every parity gate wct_stylize is under), its levels against the CPU checker, graph
capture, the bicubic device resize against the checker, and the command line's --synthesis."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from oracle import resize_oracle as R
from tests import synth_oracle as S
from tests.conftest import GOLD, PKG, REPO, rel_err
from wct_hip import cli

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def wct(torch_cuda, weights16x):
    from wct_hip import WCT
    return WCT(types.SimpleNamespace(mode="16x", alpha=1.0), weights=weights16x)


def cu(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


# ---------------------------------------------------------------------------------------------------------------- noise
@pytest.mark.parametrize("H,W", [(1, 1), (1, 2), (5, 7), (33, 65), (272, 400), (2160, 3840)])
def test_noise_is_the_oracle_bit_for_bit(torch_cuda, wct, H, W):
    torch = torch_cuda
    for seed, sid in ((0, 0), (0xDEADBEEF12345678, 0), (3, 41), (2 ** 64 - 1, 2 ** 32 - 1)):
        if H * W > 10 ** 6 and (seed, sid) not in ((0, 0), (0xDEADBEEF12345678, 0)):
            continue                                  # a 4K oracle image takes seconds of numpy: two of them
        want = S.noise(seed, H, W, sid)
        got = wct.noise(H, W, seed=seed, stream_id=sid)
        assert tuple(got.shape) == (1, 3, H, W) and got.dtype == torch.float32
        g = got.cpu().numpy()[0]
        assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), (H, W, seed, sid, int((g != want).sum()))
        assert torch.equal(wct.noise(H, W, seed=seed, stream_id=sid), got)          # two calls are identical
    assert float(got.max()) < 1.0 and float(got.min()) >= 0.0


@pytest.mark.parametrize("H,W", [(1, 1), (1, 2), (5, 7), (33, 65), (272, 400)])
def test_noise_into_caller_buffers_and_misaligned_views(torch_cuda, wct, H, W):
    """out= buffers: one 16-byte aligned, and views that start 4, 8 and 12 bytes off a 16-byte boundary (single-float stores); the
    floats around the view stay untouched."""
    torch = torch_cuda
    n = 3 * H * W
    want = S.noise(11, H, W, 2).reshape(-1)
    out = torch.empty((3, H, W), device="cuda")
    assert out.data_ptr() % 16 == 0
    r = wct.noise(H, W, seed=11, stream_id=2, out=out)
    assert r.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy().reshape(-1), want)
    for off in (1, 2, 3):
        buf = torch.full((n + 8,), -7.0, device="cuda")
        assert buf.data_ptr() % 16 == 0
        view = buf[off:off + n]
        assert view.data_ptr() % 16 == 4 * off
        wct.noise(H, W, seed=11, stream_id=2, out=view)
        host = buf.cpu().numpy()
        assert np.array_equal(host[off:off + n], want), (H, W, off)
        assert (host[:off] == -7.0).all() and (host[off + n:] == -7.0).all(), (H, W, off)


def test_noise_argument_errors(torch_cuda, wct):
    torch = torch_cuda
    for bad in (dict(H=0, W=4), dict(H=4, W=-1), dict(H=4, W=4, seed=-1), dict(H=4, W=4, seed=2 ** 64), dict(H=4, W=4, stream_id=2 ** 32)):
        with pytest.raises(ValueError):
            wct.noise(**bad)
    with pytest.raises(ValueError):
        wct.noise(4, 4, out=torch.empty(47, device="cuda"))
    with pytest.raises(ValueError):
        wct.noise(4, 4, out=torch.empty(48, device="cuda", dtype=torch.float64))
    # the C entry itself: NULL pointer and empty shapes are WCT_ERR_INVALID with a text
    from wct_hip import lib
    assert wct._lib.wct_noise_uniform(wct._ctx, 0, 0, 4, 4, None) == lib.WCT_ERR_INVALID
    assert b"noise_uniform" in wct._lib.wct_last_error(wct._ctx)
    assert wct._lib.wct_noise_uniform(wct._ctx, 0, 0, 0, 4, torch.empty(48, device="cuda").data_ptr()) == lib.WCT_ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------- synthesize
@pytest.mark.parametrize("alpha,H,W,transform", [
    pytest.param(1.0, 250, 333, "wct", id="1.0-250-333"), pytest.param(1.0, 512, 768, "wct", id="1.0-512-768"),
    pytest.param(0.6, 250, 333, "wct", id="0.6-250-333"), pytest.param(0.6, 512, 768, "wct", id="0.6-512-768"),
    pytest.param(0.6, 250, 333, "ot", id="0.6-250-333-ot"), pytest.param(0.6, 250, 333, "adain", id="0.6-250-333-adain")])
def test_synthesize_equals_stylize_of_the_oracle_noise(torch_cuda, wct, H, W, alpha, transform):
    """Under ot and adain (include/wct_hip_transform.h: the composed entries follow the context's mode) the same identity, on an
    engine of that mode, and against the prepared cascade."""
    torch = torch_cuda
    g = torch.Generator(device="cuda").manual_seed(H)
    texture = torch.rand((1, 3, 200, 160), device="cuda", generator=g)
    seed = 0x1_0000_0007
    if transform != "wct":
        from tests import state_cases as sc
        under_wct = wct.synthesize(texture, H, W, seed=seed, stream_id=3, alpha=alpha).clone()
        wct = sc.make_engine("16x")
        wct.set_transform(transform)
        assert not torch.equal(wct.synthesize(texture, H, W, seed=seed, stream_id=3, alpha=alpha), under_wct)          # the mode took effect
        wct.style_prepare(texture)
        prepared = wct.stylize_prepared(wct.noise(H, W, seed=seed, stream_id=3), alpha=alpha).clone()
        assert torch.equal(wct.synthesize(None, H, W, seed=seed, stream_id=3, alpha=alpha), prepared)
        assert torch.equal(wct.synthesize(texture, H, W, seed=seed, stream_id=3, alpha=alpha), prepared)
    direct = wct.stylize(cu(torch, S.noise(seed, H, W, 3))[None], texture, alpha=alpha).clone()
    got = wct.synthesize(texture, H, W, seed=seed, stream_id=3, alpha=alpha)
    assert got.shape == direct.shape == (1, 3, H // 16 * 16, W // 16 * 16)
    assert torch.equal(got, direct)
    out = torch.empty((3, H, W), device="cuda")
    again = wct.synthesize(texture, H, W, seed=seed, stream_id=3, alpha=alpha, out=out)
    assert again.data_ptr() == out.data_ptr() and torch.equal(again, direct)
    assert wct.saturation_count() == 0


def test_synthesize_other_equalities(torch_cuda, wct):
    torch = torch_cuda
    g = torch.Generator(device="cuda").manual_seed(4)
    texture = torch.rand((1, 3, 176, 208), device="cuda", generator=g)
    # the default size is the texture's
    a = wct.synthesize(texture, seed=5).clone()
    assert a.shape == (1, 3, 176, 208) and torch.equal(a, wct.stylize(wct.noise(176, 208, seed=5), texture))
    # num_run = 3 is three chained cascades
    x = wct.noise(160, 240, seed=9, stream_id=1)
    for _ in range(3):
        x = wct.stylize(x, texture)
    assert torch.equal(wct.synthesize(texture, 160, 240, seed=9, stream_id=1, num_run=3), x)
    # an output size different from the texture's, larger and smaller
    for (H, W) in ((320, 400), (64, 48)):
        y = wct.synthesize(texture, H, W, seed=2).clone()
        assert y.shape == (1, 3, H, W) and bool(torch.isfinite(y).all())
        assert torch.equal(y, wct.stylize(wct.noise(H, W, seed=2), texture))
    # texture=None: the statistics already in the context
    direct = wct.synthesize(texture, 192, 256, seed=21, alpha=0.6).clone()
    wct.style_prepare(texture)
    assert torch.equal(wct.synthesize(None, 192, 256, seed=21, alpha=0.6), direct)
    assert torch.equal(wct.stylize_prepared(wct.noise(192, 256, seed=21), alpha=0.6), direct)
    with pytest.raises(ValueError, match="needs H and W"):
        wct.synthesize(None)
    # seeds and stream ids matter
    other_seed, other_stream = wct.synthesize(texture, 192, 256, seed=22, alpha=0.6).clone(), wct.synthesize(texture, 192, 256, seed=21, stream_id=1, alpha=0.6).clone()
    assert not torch.equal(other_seed, direct) and not torch.equal(other_stream, direct) and not torch.equal(other_seed, other_stream)
    assert wct.saturation_count() == 0


def test_synthesize_argument_errors_write_nothing(torch_cuda, wct, weights16x):
    torch = torch_cuda
    from wct_hip import WCT, lib
    texture = torch.rand((1, 3, 64, 64), device="cuda")
    out = torch.full((3, 64, 64), -3.0, device="cuda")
    for kw in (dict(H=16, W=64), dict(H=64, W=31), dict(H=64, W=64, num_run=0), dict(H=64, W=64, seed=-1), dict(H=64, W=64, stream_id=-1)):
        with pytest.raises(ValueError):
            wct.synthesize(texture, out=out, **kw)
    with pytest.raises(ValueError, match="texture"):
        wct.synthesize(torch.rand((1, 3, 20, 64), device="cuda"), 64, 64, out=out)
    torch.cuda.synchronize()
    assert bool((out == -3.0).all())
    fresh = WCT(types.SimpleNamespace(mode="16x", alpha=1.0), weights=weights16x)      # no style statistics yet
    with pytest.raises(lib.WctError, match="no style statistics"):
        fresh.synthesize(None, 64, 64, out=out)
    torch.cuda.synchronize()
    assert bool((out == -3.0).all())


def test_synthesis_levels_vs_oracle(torch_cuda, wct, oracle, weights16x):
    """250 x 333 from a 200 x 160 texture against the CPU checker, level by level as test_hip_parity.py::test_levels_vs_oracle does:
    level 5 takes the oracle's noise image on both sides, every later level the checker's previous output on both sides; the limit
    per level is that test's 2e-4."""
    torch = torch_cuda
    H, W, Hs, Ws = 250, 333, 200, 160
    rng = np.random.default_rng(H * 7 + W)
    s = rng.random((3, Hs, Ws), dtype=np.float32)
    mods = oracle.Modules("16x", weights16x)
    img = S.noise(17, H, W, 0)
    assert torch.equal(wct.noise(H, W, seed=17)[0], cu(torch, img))
    errs = {}
    for k in (5, 4, 3, 2, 1):
        ref = oracle.style_transfer(mods, k, img, s, 1.0)
        got = wct.style_transfer_level(k, cu(torch, img)[None], cu(torch, s)[None]).cpu().numpy()[0]
        assert got.shape == ref.shape
        errs[k] = rel_err(got, ref)
        print("synthesis level %d: rel err %.3e" % (k, errs[k]))
        img = ref
    for k, e in errs.items():
        assert e < 2e-4, (k, errs)
    assert wct.saturation_count() == 0


def test_synthesize_is_capturable_into_a_hip_graph(torch_cuda):
    """Like wct_stylize on the 16x path, wct_synthesize never synchronises and allocates nothing after the first call of a size: captured
    once after a warm-up, the graph replays the direct call's bits, also with another texture in the same buffer -- the seed is a
    baked kernel argument, so the noise is the same.  In a fresh process: a failed capture can leave the runtime in capture mode."""
    code = r"""
import sys, types
sys.path[:0] = [%r, %r]
import torch
from wct_hip import WCT, model_zoo
import os
w = model_zoo.load_npz_weights(os.path.join(%r, "weights", "16x.npz"))
wct = WCT(types.SimpleNamespace(mode="16x", alpha=1.0), weights=w)
g = torch.Generator(device="cuda").manual_seed(5)
t1 = torch.rand((3, 200, 240), device="cuda", generator=g)
t2 = torch.rand((3, 200, 240), device="cuda", generator=g)
want1 = wct.synthesize(t1, 272, 400, seed=77, stream_id=2).clone()
want2 = wct.synthesize(t2, 272, 400, seed=77, stream_id=2).clone()
assert torch.equal(want1, wct.stylize(wct.noise(272, 400, seed=77, stream_id=2), t1))
t = t1.clone()
out = torch.empty((3, 272, 400), device="cuda")
wct.synthesize(t, 272, 400, seed=77, stream_id=2, out=out)      # warm-up on the buffers the graph will use
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph):
    wct.synthesize(t, 272, 400, seed=77, stream_id=2, out=out)
out.zero_()
graph.replay()
torch.cuda.synchronize()
assert torch.equal(out.view(1, 3, 272, 400), want1), "replay 1 differs"
t.copy_(t2)
graph.replay()
torch.cuda.synchronize()
assert torch.equal(out.view(1, 3, 272, 400), want2), "replay 2 (new texture, same graph) differs"
assert wct.saturation_count() == 0
print("GRAPH_OK")
""" % (REPO, PKG, PKG)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "GRAPH_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------------------- bicubic resize
def test_device_bicubic_resize_vs_checker(torch_cuda, wct):
    torch = torch_cuda
    rng = np.random.default_rng(3)
    shapes = [(1, 1, 5, 7), (1, 37, 1, 11), (41, 1, 9, 1), (5, 7, 1, 1), (33, 65, 33, 65), (2, 3, 200, 300), (2048, 2048, 512, 512)]
    for (h, w, oh, ow) in shapes:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        x = torch.from_numpy(img).cuda()
        got = wct.resize_u8(x, (oh, ow), filter="bicubic")
        assert np.array_equal(got.cpu().numpy(), S.resize_bicubic_u8(img, oh, ow)), (h, w, oh, ow)
        assert torch.equal(wct.resize_u8(x, (oh, ow), to_tensor=True, filter="bicubic"), wct.to_tensor_u8(got)), (h, w, oh, ow)
        # the bilinear entries are what they were, also with bicubic tables of the same sizes in the context's cache
        assert np.array_equal(wct.resize_u8(x, (oh, ow)).cpu().numpy(), R.resize_bilinear_u8(img, oh, ow)), (h, w, oh, ow)
        assert np.array_equal(wct.resize_u8(x, (oh, ow), filter="bilinear").cpu().numpy(), R.resize_bilinear_u8(img, oh, ow)), (h, w, oh, ow)
    img = rng.integers(0, 256, (50, 60, 3), dtype=np.uint8)
    x = torch.from_numpy(img).cuda()
    for k in range(1, 24):      # alternating filters through the bounded table cache
        assert np.array_equal(wct.resize_u8(x, (k, 2 * k), filter="bicubic").cpu().numpy(), S.resize_bicubic_u8(img, k, 2 * k)), k
        assert np.array_equal(wct.resize_u8(x, (k, 2 * k)).cpu().numpy(), R.resize_bilinear_u8(img, k, 2 * k)), k
    try:
        from PIL import Image
        assert np.array_equal(wct.resize_u8(x, (77, 123), filter="bicubic").cpu().numpy(), np.asarray(Image.fromarray(img).resize((123, 77), Image.BICUBIC)))
    except ImportError:
        pass
    with pytest.raises(ValueError, match="explicit"):
        wct.resize_u8(x, 32, filter="bicubic")
    with pytest.raises(ValueError, match="filter"):
        wct.resize_u8(x, (8, 8), filter="lanczos")
    from wct_hip import lib
    o = torch.empty((8, 8, 3), dtype=torch.uint8, device="cuda")
    f = torch.empty((3, 8, 8), device="cuda")
    L = wct._lib
    assert L.wct_resize_u8_filter(wct._ctx, x.data_ptr(), 50, 60, o.data_ptr(), None, 8, 8, 2) == lib.WCT_ERR_INVALID
    assert L.wct_resize_u8_filter(wct._ctx, x.data_ptr(), 50, 60, o.data_ptr(), f.data_ptr(), 8, 8, 1) == lib.WCT_ERR_INVALID
    assert L.wct_resize_u8_filter(wct._ctx, x.data_ptr(), 50, 60, None, None, 8, 8, 1) == lib.WCT_ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------- command line
def test_cli_synthesis(torch_cuda, tmp_path):
    """--synthesis over a folder of two textures (the G11 style and a non-square crop of it) at --style_size 256: names, shapes by the
    size rule, reproducible by seed, --synthesis_size, and every file byte-identical to to_u8(synthesize(...)) of the test's own calls
    saved through the same Pillow call (JPEG is lossy: the BYTES are compared, never decoded pixels)."""
    torch = torch_cuda
    Image = pytest.importorskip("PIL.Image")
    from wct_hip import WCT
    tex = tmp_path / "textures"
    tex.mkdir()
    full = Image.open(os.path.join(GOLD, "g11_style_2048x2048.jpg")).convert("RGB")
    full.save(tex / "full.png")
    full.crop((100, 300, 100 + 1500, 300 + 1000)).save(tex / "crop.v1.png")      # 1500 wide, 1000 high
    (tex / "notes.txt").write_text("not an image")
    jobs = cli.texture_jobs(str(tex))
    assert sorted(jobs) == ["crop.v1.png", "full.png"]

    def run(tag, *extra):
        o = tmp_path / tag
        assert cli.main(["--mode", "16x", "--synthesis", "--texturePath", str(tex), "--style_size", "256", "--outf", str(o), "--log_mark", "S",
                         "--alpha", "0.6", "--num_run", "2"] + list(extra)) == 0
        return o, {f: (o / f).read_bytes() for f in sorted(os.listdir(o)) if f.endswith(".jpg")}

    o, a = run("a", "--seed", "7")
    assert sorted(a) == ["S_mode=16x_alpha=0.6_crop.jpg", "S_mode=16x_alpha=0.6_full.jpg"]
    w = WCT(types.SimpleNamespace(mode="16x", alpha=0.6))
    for i, tfile in enumerate(jobs):
        u8 = cli.load_rgb_u8(str(tex / tfile))
        th, tw = cli.synthesis_shape(u8.shape[0], u8.shape[1], 256)
        assert (th, tw) == ((256, 256) if tfile == "full.png" else (170, 256))
        path = cli.synthesis_out_name(types.SimpleNamespace(outf=str(o), log_mark="S", mode="16x", alpha=0.6), tfile)
        with Image.open(path) as im:
            assert im.size == (tw // 16 * 16, th // 16 * 16) and im.mode == "RGB"      # the cascade floors each edge to a multiple of 16
        t = w.resize_u8(torch.from_numpy(u8).cuda(), (th, tw), to_tensor=True, filter="bicubic")
        if tfile != "full.png":          # (the 2048^2 case is in test_device_bicubic_resize_vs_checker)
            assert np.array_equal(w.resize_u8(torch.from_numpy(u8).cuda(), (th, tw), filter="bicubic").cpu().numpy(), S.resize_bicubic_u8(u8, th, tw))
        ref = w.to_u8(w.synthesize(t, seed=7, stream_id=i, alpha=0.6, num_run=2), 0).cpu().numpy()
        Image.fromarray(ref).save(tmp_path / "ref.jpg")
        assert (tmp_path / "ref.jpg").read_bytes() == a[os.path.basename(path)], tfile
    log = (o / "log_S_16x.txt").read_text()
    assert "Number of content-style pairs: 2" in log and "Processed 2 images." in log and "--pipeline is ignored with --synthesis" in log
    assert log.count("Elapsed time is:") == 2 and ' #1: Transferring "%s.jpg"' % jobs[1].split(".")[0] in log
    # reproducible by seed; another seed differs
    _, b = run("b", "--seed", "7")
    _, c = run("c", "--seed", "8")
    assert b == a and all(c[k] != a[k] for k in a)
    # --synthesis_size: files of exactly that size, made from noise at the next multiples of 16
    o, d = run("d", "--seed", "7", "--synthesis_size", "320x200")
    assert sorted(d) == sorted(a)
    for i, tfile in enumerate(jobs):
        name = "S_mode=16x_alpha=0.6_%s.jpg" % tfile.split(".")[0]
        with Image.open(o / name) as im:
            assert im.size == (320, 200)          # 200 rows x 320 columns
        u8 = cli.load_rgb_u8(str(tex / tfile))
        t = w.resize_u8(torch.from_numpy(u8).cuda(), cli.synthesis_shape(u8.shape[0], u8.shape[1], 256), to_tensor=True, filter="bicubic")
        res = w.synthesize(t, 208, 320, seed=7, stream_id=i, alpha=0.6, num_run=2)
        assert res.shape == (1, 3, 208, 320)
        Image.fromarray(w.to_u8(res[:, :, :200, :320], 0).cpu().numpy()).save(tmp_path / "ref.jpg")
        assert (tmp_path / "ref.jpg").read_bytes() == d[name], tfile
    # a texture folder without images is an empty run, not an error
    empty = tmp_path / "empty"
    empty.mkdir()
    assert cli.main(["--mode", "16x", "--synthesis", "--texturePath", str(empty), "--outf", str(tmp_path / "e"), "--log_mark", "S"]) == 0
