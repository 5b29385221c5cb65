"""Style interpolation and per-pixel style weights on the MI355X: wct_moments_weighted and wct_apply_mixed against numpy,
wct_stylize_interp / wct_style_blend against the tier-1 definition, wct_stylize_blend against the blend oracle (tests/blend_oracle.py)
and against the other cascades it generalises."""
import os
import types

import numpy as np
import pytest

from tests import blend_oracle
from tests.conftest import GOLD, rel_err
from wct_hip import model_zoo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def wct16(torch_cuda, weights16x):
    from wct_hip import WCT
    return WCT(types.SimpleNamespace(mode="16x", alpha=1.0), weights=weights16x)


def cu(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _smooth(rng, shape, passes=2):
    x = rng.random(shape, dtype=np.float32)
    for _ in range(passes):
        x = (x + np.roll(x, 1, -1) + np.roll(x, 1, -2) + np.roll(x, -1, -1) + np.roll(x, -1, -2)) / 5
    return np.ascontiguousarray(x, np.float32)


def _jpg(name, H, W, y0=0, x0=0):
    from PIL import Image
    a = np.asarray(Image.open(os.path.join(GOLD, name)).convert("RGB"), np.float32)[y0:y0 + H, x0:x0 + W] / 255
    return np.ascontiguousarray(a.transpose(2, 0, 1))


def _maps(kind, H, W, rng):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    if kind == "gradient":                               # left to right, style 0 -> style 1
        g = xx / np.float32(W - 1)
        return np.stack([1 - g, g]).astype(np.float32)
    if kind == "disc":                                   # a feathered disc of style 0, the rest unstyled
        r = np.sqrt((yy - H / 2) ** 2 + (xx - W / 2) ** 2) / (min(H, W) / 3)
        return np.clip((1.3 - r) / 0.6, 0, 1)[None].astype(np.float32)
    if kind == "partition3":                             # three styles on a smooth random partition of unity
        n = np.stack([_smooth(rng, (H, W), passes=30) for _ in range(3)]) ** 4
        return (n / n.sum(0, keepdims=True)).astype(np.float32)
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------------- 1. kernels
@pytest.mark.parametrize("C", [24, 32, 64, 128, 512, 4, 20, 36, 132, 260])
@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("mom32", [0, 1])
def test_moments_weighted_vs_numpy(torch_cuda, wct16, C, K, mom32):
    torch = torch_cuda
    rng = np.random.default_rng(C * 100 + K * 10 + mom32)
    shapes = ((37, 53), (260, 256)) if C <= 128 else ((37, 53), (160, 160))
    for h, w in shapes:
        f = np.maximum(rng.standard_normal((h, w, C)).astype(np.float32) + 0.3, 0)
        f[..., 1] = 0
        wts = rng.random((K, h, w)).astype(np.float32)
        wts[:, : h // 3] = 0                                    # tiles without weight: skipped
        wts[0, h // 2:] = 1.0
        wct16.debug_set("mom32", mom32)
        try:
            s, ss = wct16.moments_weighted(cu(torch, f)[None], cu(torch, wts))
            s2, ss2 = wct16.moments_weighted(cu(torch, f)[None], cu(torch, wts))
        finally:
            wct16.debug_set("mom32", 1)
        assert torch.equal(s, s2) and torch.equal(ss, ss2)      # bitwise reproducible
        fp32_form = mom32 == 1 and h * w >= 65536
        bound = 1e-7 if fp32_form else 1e-13
        X = f.reshape(-1, C).astype(np.float64)
        for k in range(K):
            wk = wts[k].reshape(-1).astype(np.float64)
            assert rel_err(s[k].cpu().numpy(), (X * wk[:, None]).sum(0)) < bound
            q = ss[k].cpu().numpy()
            assert rel_err(q, (X * wk[:, None]).T @ X) < bound
            assert np.array_equal(q, q.T)


@pytest.mark.parametrize("C", [24, 64, 128, 512, 4, 20, 36, 132, 260])
@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
def test_apply_mixed_vs_numpy(torch_cuda, wct16, C, layout):
    torch = torch_cuda
    rng = np.random.default_rng(C)
    K, h, w = 3, 29, 41
    f = rng.standard_normal((h, w, C)).astype(np.float32)
    wts = rng.random((K, h, w)).astype(np.float32)
    wts /= np.maximum(wts.sum(0, keepdims=True), 1)
    wts[:, :5] = 0                                              # all-zero weights: x copied through
    wts[:, 5:9] = 0
    wts[1, 5:9] = 1                                             # unit weight on one style
    wts[:, 9:12] = np.float32(1 / 3)                            # unit sum over three
    M = rng.standard_normal((K, C, C)) / np.sqrt(C)
    b = rng.standard_normal((K, C))
    X = f.reshape(-1, C).astype(np.float64)
    ref = X.copy()
    for k in range(K):
        ref += wts[k].reshape(-1, 1) * ((X @ M[k].T + b[k]) - X)
    ref = ref.reshape(h, w, C)
    x = f if layout == "nhwc" else f.transpose(2, 0, 1)
    got = wct16.apply_mixed(cu(torch, x)[None], cu(torch, wts), cu(torch, M), cu(torch, b), layout=layout).cpu().numpy()[0]
    if layout == "nchw":
        got = got.transpose(1, 2, 0)
    assert rel_err(got, ref) <= 1e-6
    assert np.array_equal(got[:5], f[:5])
    assert rel_err(got[5:9], (X.reshape(h, w, C)[5:9] @ M[1].T + b[1])) <= 1e-6


# ---------------------------------------------------------------------------------------------------- 2. tier 1
@pytest.mark.parametrize("K,alpha", [(2, 1.0), (3, 0.6)])
def test_stylize_interp_vs_definition(torch_cuda, oracle, weights16x, wct16, K, alpha):
    torch = torch_cuda
    rng = np.random.default_rng(K)
    content = _jpg("g11_uhd_content_3840x2160.jpg", 512, 512, 800, 1600)
    styles = [_jpg("g11_style_2048x2048.jpg", 256, 256, 900, 900), _smooth(rng, (3, 200, 240)),
              _jpg("g11_style_2048x2048.jpg", 192, 224, 100, 1500)][:K]
    lam = [0.3, 0.7, 0.5][:K]
    mods = oracle.Modules("16x", weights16x)
    ref = blend_oracle.stylize_interp(mods, content, styles, lam, alpha)
    got = wct16.stylize_interp(cu(torch, content), [cu(torch, s) for s in styles], lam, alpha).cpu().numpy()[0]
    assert got.shape == ref.shape and rel_err(got, ref) < 1e-3


def test_interp_levels_original_mode(torch_cuda, oracle):
    """--mode original, each level isolated (the oracle's previous output feeds both sides): style_blend of exported statistics, then the
    split content path against the per-style sum of the reference's transforms."""
    from wct_hip import WCT
    torch = torch_cuda
    w = model_zoo.synth_weights("original", 7)
    wct = WCT(types.SimpleNamespace(mode="original", alpha=1.0), weights=w)
    mods = oracle.Modules("original", w)
    rng = np.random.default_rng(17)
    H, W = 192, 256
    img = _smooth(rng, (3, H, W))
    styles = [_smooth(rng, (3, 96, 112)), rng.random((3, 80, 72), dtype=np.float32)]
    lam, alpha = [1.0, 2.0], 0.8
    stats = []
    for s in styles:
        wct.style_prepare(cu(torch, s))
        stats.append({L: wct.style_export(L).clone() for L in (1, 2, 3, 4, 5)})
    for level in (5, 4, 3, 2, 1):
        ref = blend_oracle.interp_transfer(mods, level, img, styles, lam, alpha)
        wct.style_blend(stats, lam, levels=(level,))
        h, w_, s, ss = wct.content_encode(level, cu(torch, img))
        M, b = wct.content_solve(level, h * w_, s, ss, alpha)
        got = wct.content_decode(level, M, b, img.shape[1], img.shape[2]).cpu().numpy()[0]
        assert got.shape == ref.shape
        assert rel_err(got, ref) < 2e-4, level
        img = ref


def test_interp_degenerate_weights_match_stylize(torch_cuda, wct16):
    torch = torch_cuda
    rng = np.random.default_rng(19)
    c = cu(torch, _jpg("g11_uhd_content_3840x2160.jpg", 384, 448, 300, 700))
    s0 = cu(torch, _jpg("g11_style_2048x2048.jpg", 256, 256, 400, 400))
    s1 = cu(torch, _smooth(rng, (3, 200, 240)))
    ref = wct16.stylize(c, s0, 0.8).clone()
    for styles, lam in (([s0, s1], [1.0, 0.0]), ([s0, s0], [0.5, 0.5])):
        got = wct16.stylize_interp(c, styles, lam, 0.8)
        print("interp %s bitwise equal to stylize: %s" % (lam, bool(torch.equal(got, ref))))
        assert rel_err(got.cpu().numpy(), ref.cpu().numpy()) <= 1e-6


def test_style_blend_prepared_matches_stylize_interp(torch_cuda, wct16):
    torch = torch_cuda
    rng = np.random.default_rng(23)
    c = cu(torch, _jpg("g11_uhd_content_3840x2160.jpg", 320, 384, 1000, 200))
    styles = [cu(torch, _jpg("g11_style_2048x2048.jpg", 256, 256, 1200, 300)), cu(torch, _smooth(rng, (3, 200, 240)))]
    lam = [0.25, 0.75]
    ref = wct16.stylize_interp(c, styles, lam, 1.0).clone()
    stats = []
    for s in styles:
        wct16.style_prepare(s)
        stats.append({L: wct16.style_export(L).clone() for L in (1, 2, 3, 4, 5)})
    wct16.style_blend(stats, lam)
    got = wct16.stylize_prepared(c, 1.0)
    assert rel_err(got.cpu().numpy(), ref.cpu().numpy()) <= 1e-6
    with pytest.raises(ValueError):
        wct16.style_blend(stats, [0.0, 0.0])
    with pytest.raises(ValueError):
        wct16.stylize_interp(c, styles, [1.0, -1.0], 1.0)


# ---------------------------------------------------------------------------------------------------- 3. tier 2
@pytest.mark.parametrize("H,W,kind", [(512, 512, "gradient"), (512, 512, "disc"), (376, 632, "partition3")])
def test_stylize_blend_vs_blend_oracle(torch_cuda, oracle, weights16x, wct16, H, W, kind):
    torch = torch_cuda
    rng = np.random.default_rng(H * 7 + len(kind))
    content = _jpg("g11_uhd_content_3840x2160.jpg", H, W, 800, 1600)
    wts = _maps(kind, H, W, rng)
    styles = [_jpg("g11_style_2048x2048.jpg", 256, 256, 900, 900), _smooth(rng, (3, 200, 240)),
              _jpg("g11_style_2048x2048.jpg", 192, 224, 100, 1500)][: wts.shape[0]]
    alpha = [1.0, 0.6, 0.8][: wts.shape[0]]
    ref = blend_oracle.stylize_blend(oracle.Modules("16x", weights16x), content, styles, wts, alpha)
    got = wct16.stylize_blend(cu(torch, content), [cu(torch, s) for s in styles], cu(torch, wts), alpha).cpu().numpy()[0]
    assert got.shape == ref.shape and rel_err(got, ref) < 1e-3


def test_stylize_blend_reduces_to_the_other_cascades(torch_cuda, wct16):
    torch = torch_cuda
    rng = np.random.default_rng(29)
    H, W = 384, 448
    c = cu(torch, _jpg("g11_uhd_content_3840x2160.jpg", H, W, 500, 2000))
    styles = [cu(torch, _jpg("g11_style_2048x2048.jpg", 256, 256, 700, 1100)), cu(torch, _smooth(rng, (3, 200, 240)))]
    # constant maps = interpolation
    lam = np.array([0.3, 0.7], np.float32)
    wts = torch.from_numpy(np.broadcast_to(lam[:, None, None], (2, H, W)).copy()).cuda()
    got = wct16.stylize_blend(c, styles, wts, 0.9).cpu().numpy()
    ref = wct16.stylize_interp(c, styles, [0.3, 0.7], 0.9).cpu().numpy()
    assert rel_err(got, ref) <= 1e-4
    # 0/1 maps constant on aligned 16 x 16 blocks = regions
    blocks = np.zeros((H // 16, W // 16), np.int64)
    blocks[:, 10:20] = 1
    blocks[:, 20:] = 2
    blocks[rng.random(blocks.shape) < 0.1] = 1
    lab16 = np.kron(blocks, np.ones((16, 16), np.int64))
    labels = np.where(lab16 == 2, 255, lab16).astype(np.uint8)
    wts = np.stack([(lab16 == k).astype(np.float32) for k in range(2)])
    got = wct16.stylize_blend(c, styles, cu(torch, wts), [1.0, 0.7]).cpu().numpy()
    ref = wct16.stylize_regions(c, styles, cu(torch, labels), [1.0, 0.7]).cpu().numpy()
    assert rel_err(got, ref) <= 1e-4
    # a single all-ones map = the single-style cascade
    got = wct16.stylize_blend(c, styles[:1], torch.ones((1, H, W), device="cuda"), 0.7).cpu().numpy()
    ref = wct16.stylize(c, styles[0], 0.7).cpu().numpy()
    assert rel_err(got, ref) <= 1e-4


def test_bad_weights_raise_before_writing_and_repeats_are_bitwise(torch_cuda, wct16):
    torch = torch_cuda
    rng = np.random.default_rng(31)
    H, W = 128, 160
    c = cu(torch, _smooth(rng, (3, H, W)))
    styles = [cu(torch, _smooth(rng, (3, 96, 96))), cu(torch, rng.random((3, 64, 80), dtype=np.float32))]
    good = _maps("gradient", H, W, rng)
    a = wct16.stylize_blend(c, styles, cu(torch, good), [1.0, 0.8])
    b = wct16.stylize_blend(c, styles, cu(torch, good), [1.0, 0.8])
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    cases = {"negative": (0, 5, 7, -0.1, "outside"), "above one": (1, 9, 9, 1.5, "outside"),
             "sum above one": (1, 3, 3, 0.9, "sum to more than 1"), "nan": (0, 100, 2, np.nan, "not finite")}
    for name, (k, i, j, v, msg) in cases.items():
        bad = good.copy()
        bad[k, i, j] = v
        if name == "sum above one":
            bad[0, i, j] = 0.5
        out = torch.full((3, H, W), -3.0, device="cuda")
        with pytest.raises(ValueError, match=msg):
            wct16.stylize_blend(c, styles, cu(torch, bad), 1.0, out=out)
        torch.cuda.synchronize()
        assert bool((out == -3.0).all()), name
    with pytest.raises(ValueError):
        wct16.stylize_blend(c, styles * 5, cu(torch, np.zeros((10, H, W), np.float32)), 1.0)     # K = 10


@pytest.mark.parametrize("H,W", [(64, 80), (70, 90)])
def test_interp_and_blend_num_run_equal_chained_runs(torch_cuda, wct16, H, W):
    """num_run = 2 and 3 of wct_stylize_interp / wct_stylize_blend against chained single-run calls, bit for bit: the two run counts
    take both parities of the ping-pong between the caller's `out` and the context's buffer (`which = (5 * num_run) & 1`).  64 x 80
    carries over unchanged; 70 x 90 is cropped to 64 x 80 by the first run, and the chained runs get the weight maps cropped top-left
    to that size (the level maps are pooled from the top-left, so they are the same maps).  With a caller's `out` an even number
    of levels must still end in that buffer."""
    torch = torch_cuda
    rng = np.random.default_rng(37)
    Hc, Wc = H // 16 * 16, W // 16 * 16
    c = cu(torch, _smooth(rng, (3, H, W)))
    styles = [cu(torch, _smooth(rng, (3, 48, 64))), cu(torch, rng.random((3, 48, 64), dtype=np.float32))]
    wts = cu(torch, _maps("gradient", H, W, rng))
    calls = {"interp": lambda img, n, out=None: wct16.stylize_interp(img, styles, [0.3, 0.7], 0.8, num_run=n, out=out),
             "blend": lambda img, n, out=None: wct16.stylize_blend(img, styles, wts[:, :img.shape[-2], :img.shape[-1]], [1.0, 0.7], num_run=n, out=out)}
    for name, run in calls.items():
        one = run(c, 1).clone()
        assert tuple(one.shape) == (1, 3, Hc, Wc), name
        two, three = run(c, 2).clone(), run(c, 3).clone()
        chained2 = run(one, 1).clone()
        chained3 = run(chained2, 1).clone()
        assert torch.equal(two, chained2), name
        assert torch.equal(three, chained3), name
        out = torch.full((3, H, W), -3.0, device="cuda")
        got = run(c, 2, out)
        assert got.data_ptr() == out.data_ptr() and torch.equal(got, chained2), name


def test_uhd_frame_gradient_vs_blend_oracle(torch_cuda, oracle, weights16x, wct16):
    torch = torch_cuda
    H, W = 2160, 3840
    content = _jpg("g11_uhd_content_3840x2160.jpg", H, W)
    rng = np.random.default_rng(37)
    styles = [_jpg("g11_style_2048x2048.jpg", 2048, 2048), _smooth(rng, (3, 512, 512))]
    wts = _maps("gradient", H, W, rng)
    wct16.saturation_count(reset=True)
    out = wct16.stylize_blend(cu(torch, content), [cu(torch, s) for s in styles], cu(torch, wts), [1.0, 0.6])
    torch.cuda.synchronize()
    assert tuple(out.shape) == (1, 3, H, W) and bool(torch.isfinite(out).all())
    assert wct16.saturation_count() == 0
    ref = blend_oracle.stylize_blend(oracle.Modules("16x", weights16x), content, styles, wts, [1.0, 0.6])
    assert rel_err(out.cpu().numpy()[0], ref) < 1e-3
