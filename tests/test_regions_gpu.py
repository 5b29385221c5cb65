"""Spatial control on the MI355X: wct_moments_labeled, wct_apply_labeled and wct_stylize_regions against numpy and the region oracle
(tests/region_oracle.py)."""
import os
import types

import numpy as np
import pytest

from tests import region_oracle
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


def _masks(kind, H, W, rng):
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "split":
        return (xx >= W // 2).astype(np.uint8)
    if kind == "disc":
        return ((yy - H / 2) ** 2 + (xx - W / 2) ** 2 < (min(H, W) / 3) ** 2).astype(np.uint8)
    if kind == "blobs":
        n = _smooth(rng, (H, W), passes=40)
        return (n > np.median(n)).astype(np.uint8)
    if kind == "three+255":
        lab = np.zeros((H, W), np.uint8)
        lab[:, W // 3:] = 1
        lab[H // 2:, 2 * W // 3:] = 2
        lab[: H // 4, : W // 4] = 255
        return lab
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------------- 1. per-label moments
@pytest.mark.parametrize("C", [24, 32, 64, 128, 4, 20, 36, 132, 260])
@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("mom32", [0, 1])
def test_moments_labeled_vs_numpy(torch_cuda, wct16, C, K, mom32):
    torch = torch_cuda
    rng = np.random.default_rng(C * 100 + K * 10 + mom32)
    # >= 65 536 pixels: the fp32 64-pixel-block form under the default; a small map: fp64 products either way
    for h, w in ((37, 53), (260, 256)):
        f = np.maximum(rng.standard_normal((h, w, C)).astype(np.float32) + 0.3, 0)
        f[..., 1] = 0
        lab = rng.integers(0, K, size=(h, w)).astype(np.uint8)       # random per pixel: every block mixed
        lab[rng.random((h, w)) < 0.1] = 255
        wct16.debug_set("mom32", mom32)
        try:
            n, s, ss = wct16.moments_labeled(cu(torch, f)[None], cu(torch, lab), K)
            n2, s2, ss2 = wct16.moments_labeled(cu(torch, f)[None], cu(torch, lab), K)
        finally:
            wct16.debug_set("mom32", 1)
        assert torch.equal(n, n2) and torch.equal(s, s2) and torch.equal(ss, ss2)      # bitwise reproducible
        fp32_form = mom32 == 1 and h * w >= 65536
        bound = 1e-7 if fp32_form else 1e-13
        X = f.reshape(-1, C).astype(np.float64)
        L = lab.reshape(-1)
        for k in range(K):
            Xk = X[L == k]
            assert n[k].item() == Xk.shape[0]
            assert rel_err(s[k].cpu().numpy(), Xk.sum(0)) < bound
            q = ss[k].cpu().numpy()
            assert rel_err(q, Xk.T @ Xk) < bound
            assert np.array_equal(q, q.T)


# ---------------------------------------------------------------------------------------------------- 2. labeled apply
@pytest.mark.parametrize("C", [24, 64, 128, 512, 4, 20, 36, 132, 260])
@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
def test_apply_labeled_vs_numpy(torch_cuda, wct16, C, layout):
    torch = torch_cuda
    rng = np.random.default_rng(C)
    K, h, w = 3, 29, 41
    f = rng.standard_normal((h, w, C)).astype(np.float32)
    lab = rng.integers(0, K, size=(h, w)).astype(np.uint8)
    lab[rng.random((h, w)) < 0.2] = 255
    M = rng.standard_normal((K, C, C)) / np.sqrt(C)
    b = rng.standard_normal((K, C))
    ref = f.astype(np.float64).copy()
    for k in range(K):
        sel = lab == k
        ref[sel] = ref[sel] @ M[k].T + b[k]
    x = f if layout == "nhwc" else f.transpose(2, 0, 1)
    got = wct16.apply_labeled(cu(torch, x)[None], cu(torch, lab), cu(torch, M), cu(torch, b), layout=layout).cpu().numpy()[0]
    if layout == "nchw":
        got = got.transpose(1, 2, 0)
    assert rel_err(got, ref) <= 1e-6
    assert np.array_equal(got[lab == 255], f[lab == 255])                  # unstyled: copied through


# ---------------------------------------------------------------------------------------------------- 3. one level from the split entries
def _level_from_entries(torch, wct, level, img, lab_full, styles, alpha):
    cF = wct.encode(level, cu(torch, img)[None], layout="nhwc")
    _, h, w, C = cF.shape
    lab = cu(torch, region_oracle.level_labels(lab_full, level, h, w))
    K = len(styles)
    n, s, ss = wct.moments_labeled(cF, lab, K)
    M = torch.zeros((K, C, C), dtype=torch.float64, device="cuda")
    b = torch.zeros((K, C), dtype=torch.float64, device="cuda")
    for k in range(K):
        if n[k].item() < 2:
            M[k] = torch.eye(C, dtype=torch.float64, device="cuda")
            continue
        sF = wct.encode(level, cu(torch, styles[k])[None], layout="nhwc")
        ns, sm, ssq = wct.moments(sF)
        M[k], b[k] = wct.solve(n[k].item(), s[k], ss[k], ns, sm, ssq, alpha=alpha[k])
    csF = wct.apply_labeled(cF, lab, M, b)
    return wct.decode(level, csF, layout="nhwc").cpu().numpy()[0]


@pytest.mark.parametrize("mode,H,W", [("16x", 160, 224), ("original", 192, 256)])
def test_one_level_from_split_entries_vs_region_oracle(torch_cuda, oracle, weights16x, mode, H, W):
    from wct_hip import WCT
    w = weights16x if mode == "16x" else model_zoo.synth_weights("original", 7)
    wct = WCT(types.SimpleNamespace(mode=mode, alpha=1.0), weights=w)
    mods = oracle.Modules(mode, w)
    rng = np.random.default_rng(H + W)
    img = _smooth(rng, (3, H, W))
    styles = [_smooth(rng, (3, 96, 112)), rng.random((3, 80, 72), dtype=np.float32)]
    lab = _masks("split", H, W, rng)
    lab[: H // 5] = 255
    alpha = [1.0, 0.6]
    for level in (5, 4, 3, 2, 1):
        ref = region_oracle.region_transfer(mods, level, img, lab, styles, alpha)
        got = _level_from_entries(torch_cuda, wct, level, img, lab, styles, alpha)
        assert got.shape == ref.shape
        assert rel_err(got, ref) < 2e-4, level
        img = ref


# ---------------------------------------------------------------------------------------------------- 4. the cascade
@pytest.mark.parametrize("H,W,mask", [(512, 512, "split"), (512, 512, "disc"), (376, 632, "blobs"), (376, 632, "three+255")])
def test_stylize_regions_vs_region_oracle(torch_cuda, oracle, weights16x, wct16, H, W, mask):
    rng = np.random.default_rng(H * 7 + len(mask))
    content = _jpg("g11_uhd_content_3840x2160.jpg", H, W, 800, 1600)
    styles = [_jpg("g11_style_2048x2048.jpg", 256, 256, 900, 900), _smooth(rng, (3, 200, 240))]
    alpha = [1.0, 0.6]
    if mask == "three+255":
        styles.append(_jpg("g11_style_2048x2048.jpg", 192, 224, 100, 1500))
        alpha.append(0.8)
    lab = _masks(mask, H, W, rng)
    mods = oracle.Modules("16x", weights16x)
    ref = region_oracle.stylize_regions(mods, content, styles, lab, alpha)
    got = wct16.stylize_regions(cu(torch_cuda, content), [cu(torch_cuda, s) for s in styles], cu(torch_cuda, lab), alpha).cpu().numpy()[0]
    assert got.shape == ref.shape
    assert rel_err(got, ref) < 1e-3


# ---------------------------------------------------------------------------------------------------- 5. K = 1 is the single-style path
def test_single_uniform_region_matches_stylize(torch_cuda, wct16):
    torch = torch_cuda
    rng = np.random.default_rng(11)
    H, W = 208, 272
    c, s = _smooth(rng, (3, H, W)), _smooth(rng, (3, 160, 176))
    lab = np.zeros((H, W), np.uint8)
    got = wct16.stylize_regions(cu(torch, c), [cu(torch, s)], cu(torch, lab), 0.7).cpu().numpy()
    ref = wct16.stylize(cu(torch, c), cu(torch, s), 0.7).cpu().numpy()
    assert got.shape == ref.shape and rel_err(got, ref) <= 1e-4
    img = c
    for level in (5, 4, 3, 2, 1):
        lv = _level_from_entries(torch, wct16, level, img, lab, [s], [0.7])
        st = wct16.style_transfer_level(level, cu(torch, img)[None], cu(torch, s)[None], 0.7).cpu().numpy()[0]
        assert lv.shape == st.shape and rel_err(lv, st) <= 2e-5, level
        img = st


# ---------------------------------------------------------------------------------------------------- 6. edges: tiny regions, bad labels, repeats
def test_tiny_regions_bad_labels_and_repeatability(torch_cuda, wct16, oracle, weights16x):
    torch = torch_cuda
    rng = np.random.default_rng(13)
    H, W = 128, 160
    c = _smooth(rng, (3, H, W))
    styles = [_smooth(rng, (3, 96, 96)), rng.random((3, 64, 80), dtype=np.float32), _smooth(rng, (3, 72, 64))]
    lab = np.zeros((H, W), np.uint8)
    lab[:, W // 2:] = 255
    lab[8, 8] = 1                         # region 1: one pixel at level 5 (the centre of its first pooling window), a few below
    # region 2: no pixel at all
    lab_d = cu(torch, lab)
    cs = [cu(torch, s) for s in styles]
    a = wct16.stylize_regions(cu(torch, c), cs, lab_d, [1.0, 1.0, 1.0])
    b = wct16.stylize_regions(cu(torch, c), cs, lab_d, [1.0, 1.0, 1.0])
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    mods = oracle.Modules("16x", weights16x)
    ref = region_oracle.stylize_regions(mods, c, styles, lab, [1.0, 1.0, 1.0])
    assert rel_err(a.cpu().numpy()[0], ref) < 1e-3
    # a label that is neither < K nor 255: refused before anything is written
    bad = lab.copy()
    bad[3, 5] = 7
    bad[100, 2] = 4
    out = torch.full((3, H, W), -3.0, device="cuda")
    with pytest.raises(ValueError, match="label value 4"):
        wct16.stylize_regions(cu(torch, c), cs, cu(torch, bad), 1.0, out=out)
    torch.cuda.synchronize()
    assert bool((out == -3.0).all())
    with pytest.raises(ValueError):
        wct16.stylize_regions(cu(torch, c), cs * 3, lab_d, 1.0)            # K = 9


@pytest.mark.parametrize("H,W", [(64, 80), (70, 90)])
def test_regions_num_run_equals_chained_runs(torch_cuda, wct16, H, W):
    """num_run = 2 and 3 of wct_stylize_regions against chained single-run calls, bit for bit: the two run counts take both parities
    of the ping-pong between the caller's `out` and the context's buffer (`which = (5 * num_run) & 1`).  64 x 80 carries over
    unchanged; 70 x 90 is cropped to 64 x 80 by the first run, and the chained runs get the label map cropped top-left to that size
    (the level maps are sampled from the top-left, so they are the same maps).  With a caller's `out` an even number of levels must
    still end in that buffer."""
    torch = torch_cuda
    rng = np.random.default_rng(17)
    Hc, Wc = H // 16 * 16, W // 16 * 16
    c = cu(torch, _smooth(rng, (3, H, W)))
    styles = [cu(torch, _smooth(rng, (3, 48, 64))), cu(torch, rng.random((3, 48, 64), dtype=np.float32))]
    lab = np.zeros((H, W), np.uint8)
    lab[:, W // 2:] = 1
    lab[:8] = 255
    lab = cu(torch, lab)

    def run(img, n, out=None):
        return wct16.stylize_regions(img, styles, lab[:img.shape[-2], :img.shape[-1]], [1.0, 0.7], num_run=n, out=out)

    one = run(c, 1).clone()
    assert tuple(one.shape) == (1, 3, Hc, Wc)
    two, three = run(c, 2).clone(), run(c, 3).clone()
    chained2 = run(one, 1).clone()
    chained3 = run(chained2, 1).clone()
    assert torch.equal(two, chained2)
    assert torch.equal(three, chained3)
    out = torch.full((3, H, W), -3.0, device="cuda")
    got = run(c, 2, out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(got, chained2)


# ---------------------------------------------------------------------------------------------------- 7. a 4K frame
def test_uhd_frame_two_regions(torch_cuda, wct16):
    torch = torch_cuda
    g = torch.Generator(device="cuda").manual_seed(3)
    c = torch.rand((3, 2160, 3840), device="cuda", generator=g)
    s0 = cu(torch, _jpg("g11_style_2048x2048.jpg", 2048, 2048))
    s1 = torch.rand((3, 1024, 1024), device="cuda", generator=g)
    lab = torch.zeros((2160, 3840), dtype=torch.uint8, device="cuda")
    lab[:, 1920:] = 1
    wct16.saturation_count(reset=True)
    out = wct16.stylize_regions(c, [s0, s1], lab, [1.0, 0.6])
    torch.cuda.synchronize()
    assert tuple(out.shape) == (1, 3, 2160, 3840) and bool(torch.isfinite(out).all())
    assert wct16.saturation_count() == 0
