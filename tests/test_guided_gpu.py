"""Region-to-region transfer on the MI355X: wct_kmeans_assign, wct_kmeans_seed, wct_feature_regions and wct_stylize_guided against the
numpy definitions of tests/guided_oracle.py (fp64 behind the fp32 z the header specifies)."""
import os
import types

import numpy as np
import pytest

from tests import guided_oracle as G
from tests import region_oracle
from tests.conftest import GOLD, rel_err
from wct_hip import lib as wlib

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


def _masks(kind, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "split":
        return (xx >= W // 2).astype(np.uint8)
    if kind == "disc":
        return ((yy - H / 2) ** 2 + (xx - W / 2) ** 2 < (min(H, W) / 3) ** 2).astype(np.uint8)
    if kind == "three+255":
        lab = np.zeros((H, W), np.uint8)
        lab[:, W // 3:] = 1
        lab[H // 2:, 2 * W // 3:] = 2
        lab[: H // 4, : W // 4] = 255
        return lab
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------------- k-means fixtures
KM_C = [4, 20, 24, 64, 132, 260, 512]
KM_K = [1, 2, 8]
KM_MAPS = [(37, 53), (1, 1), (260, 256)]     # ragged; one pixel; several workgroups per label (the multi-partial reduction)


def km_case(C, K, h, w):
    """Features, their standardisation, z, and centroids two Lloyd steps behind the farthest-first start -- all from the oracle.  The
    one-pixel map is a pixel of the ragged one, under that map's standardisation and centroids."""
    if (h, w) == (1, 1):
        base = km_case(C, K, 37, 53)
        f = np.ascontiguousarray(base.f[5:6, 7:8])
        return types.SimpleNamespace(f=f, sh=base.sh, sc=base.sc, z=G.zmap(f, base.sh, base.sc), cent=base.cent)
    f = G.cluster_features(K, h, w, C, 1000 * C + 10 * K + h)
    sh, sc = G.standardisation_of(f)
    z = G.zmap(f, sh, sc)
    cent = G.lloyd(z, K, 2)[0]
    return types.SimpleNamespace(f=f, sh=sh, sc=sc, z=z, cent=cent)


def check_labels(lab_dev, z, cent, cap):
    """The clear-pixel rule: every clear pixel carries the oracle's label, an unclear pixel's distance is within the margin of the best,
    and at most `cap` of the map is unclear.  Returns (fp64 distances, unclear share)."""
    d = G.distances(z, cent)
    clear, margin = G.clear_pixels(d, z)
    lab = lab_dev.reshape(-1).astype(np.int64)
    assert lab.max() < d.shape[1]
    want = d.argmin(1)
    assert np.array_equal(lab[clear], want[clear]), "clear pixels with another label: %d" % int((lab[clear] != want[clear]).sum())
    chosen = d[np.arange(d.shape[0]), lab]
    assert (chosen - d.min(1) <= margin).all()
    share = 1.0 - clear.mean()
    print("unclear share %.3g (cap %.3g)" % (share, cap))
    assert share <= cap
    return d, share


@pytest.fixture(scope="module", params=[(C, K) for C in KM_C for K in KM_K], ids=lambda p: "C%d-K%d" % p)
def km(request):
    C, K = request.param
    return C, K, {m: km_case(C, K, *m) for m in KM_MAPS}


# ---------------------------------------------------------------------------------------------------- 1. kmeans_assign
def test_kmeans_assign_vs_fp64(torch_cuda, wct16, km):
    torch = torch_cuda
    C, K, cases = km
    for (h, w), c in cases.items():
        args = (cu(torch, c.f)[None], cu(torch, c.sh), cu(torch, c.sc), cu(torch, c.cent))
        lab, n, s, cost, nxt = wct16.kmeans_assign(*args)
        again = wct16.kmeans_assign(*args)
        for a, b in zip((lab, n, s, cost, nxt), again):
            assert torch.equal(a, b)                                              # bitwise reproducible
        lab_h = lab.cpu().numpy().reshape(-1)
        d, _ = check_labels(lab_h, c.z, c.cent, 0.01)
        z64 = c.z.astype(np.float64)
        onehot = (lab_h[None, :] == np.arange(K)[:, None]).astype(np.float64)
        n_h, s_h = n.cpu().numpy(), s.cpu().numpy()
        assert np.array_equal(n_h, onehot.sum(1))                                 # exact
        err = np.abs(s_h - onehot @ z64).max()
        print("%dx%d C=%d K=%d: sum err %.3g of %.3g" % (h, w, C, K, err, np.abs(z64).sum()))
        assert err <= 1e-12 * max(np.abs(z64).sum(), 1e-300)
        want_cost = d[np.arange(d.shape[0]), lab_h].sum()
        assert abs(cost.item() - want_cost) <= 1e-5 * want_cost + 1e-30
        want_next = np.where(n_h[:, None] > 0, s_h / np.maximum(n_h, 1)[:, None], c.cent)
        assert np.array_equal(nxt.cpu().numpy(), want_next)                       # one fp64 division per element
        none = wct16.kmeans_assign(*args, want_labels=False, want_next=False)
        assert none[0] is None and none[4] is None and torch.equal(none[2], s) and torch.equal(none[3], cost)


def test_kmeans_assign_empty_and_duplicate_clusters(torch_cuda, wct16):
    torch = torch_cuda
    for C, h, w in ((20, 37, 53), (260, 64, 70)):
        c = km_case(C, 3, h, w)
        dev = (cu(torch, c.f)[None], cu(torch, c.sh), cu(torch, c.sc))
        far = np.vstack([c.cent[:2], np.full((1, C), 1e3), c.cent[2:]])           # a centroid far outside the data, in the middle
        lab, n, s, cost, nxt = wct16.kmeans_assign(*dev, cu(torch, far))
        assert n[2].item() == 0 and not bool((lab == 2).any()) and bool((s[2] == 0).all())
        assert torch.equal(nxt[2], cu(torch, far)[2])                             # an empty cluster stays where it was, bit for bit
        dup = np.vstack([c.cent[:2], c.cent[1:2], c.cent[2:]])
        lab_d, n_d, *_ = wct16.kmeans_assign(*dev, cu(torch, dup))
        assert n_d[2].item() == 0 and n_d[1].item() > 0                           # equal distances: the lowest k
        lab_o = wct16.kmeans_assign(*dev, cu(torch, c.cent))[0]
        assert torch.equal(torch.where(lab_d == 3, torch.full_like(lab_d, 2), lab_d), lab_o)
    with pytest.raises(ValueError):
        wct16.kmeans_assign(*dev, cu(torch, np.zeros((9, C))))                    # K = 9
    with pytest.raises(ValueError):
        wct16.kmeans_assign(cu(torch, c.f[..., :6])[None], cu(torch, c.sh[:6]), cu(torch, c.sc[:6]), cu(torch, c.cent[:, :6]))   # C % 4


# ---------------------------------------------------------------------------------------------------- 2. kmeans_seed
def test_kmeans_seed_vs_fp64(torch_cuda, wct16, km):
    torch = torch_cuda
    C, K, cases = km
    for (h, w), c in cases.items():
        cent, idx, margins = G.seed(c.z, K)
        assert min(margins) >= 1e-4, "fixture: an arg-max decision of the oracle is too close (%r); change its seed" % (margins,)
        cen_d, idx_d = wct16.kmeans_seed(cu(torch, c.f)[None], cu(torch, c.sh), cu(torch, c.sc), K)
        assert np.array_equal(idx_d.cpu().numpy(), idx), (h, w)
        assert np.array_equal(cen_d.cpu().numpy(), cent)                          # the chosen pixels' fp32 z, exactly
        cen_2, idx_2 = wct16.kmeans_seed(cu(torch, c.f)[None], cu(torch, c.sh), cu(torch, c.sc), K)
        assert torch.equal(cen_d, cen_2) and torch.equal(idx_d, idx_2)


def test_kmeans_seed_duplicate_pixels_take_the_lowest_index(torch_cuda, wct16):
    torch = torch_cuda
    c = km_case(24, 3, 37, 53)
    f = c.f.copy()
    _, idx, _ = G.seed(c.z, 3)
    flat = f.reshape(-1, 24)
    for j, i in enumerate(idx):                                                   # an exact copy of every chosen pixel, further down the map
        flat[1900 + j] = flat[i]
    assert (idx < 1900).all()
    z = G.zmap(f, c.sh, c.sc)
    cent2, idx2, _ = G.seed(z, 3)
    assert np.array_equal(idx2, idx)                                              # the oracle: first maximum
    cen_d, idx_d = wct16.kmeans_seed(cu(torch, f)[None], cu(torch, c.sh), cu(torch, c.sc), 3)
    assert np.array_equal(idx_d.cpu().numpy(), idx) and np.array_equal(cen_d.cpu().numpy(), cent2)
    same = np.ascontiguousarray(np.broadcast_to(f[3, 4], (9, 11, 24)))            # every pixel equal: all K centres are pixel 0
    _, idx_s = wct16.kmeans_seed(cu(torch, same)[None], cu(torch, c.sh), cu(torch, c.sc), 3)
    assert idx_s.cpu().tolist() == [0, 0, 0]


# ---------------------------------------------------------------------------------------------------- 3. feature_regions
def _flat_regions(rng, H, W, colours, noise=0.03):
    """K flat colours plus noise: vertical thirds with a horizontal cut in the last one."""
    lab = np.zeros((H, W), np.int64)
    lab[:, W // 3:] = 1
    lab[H // 2:, 2 * W // 3:] = 2
    img = np.asarray(colours, np.float32)[lab].transpose(2, 0, 1) + noise * rng.standard_normal((3, H, W)).astype(np.float32)
    return np.ascontiguousarray(np.clip(img, 0, 1), np.float32)


COLOURS = [(0.9, 0.15, 0.1), (0.1, 0.8, 0.2), (0.15, 0.2, 0.9)]


def _device_standardisation(wct, torch, level, img):
    f = wct.encode(level, cu(torch, img)[None], layout="nhwc")
    n, s, ss = wct.moments(f)
    sh, sc = G.standardisation(n, s.cpu().numpy(), np.diagonal(ss.cpu().numpy()))
    return f, sh, sc


@pytest.mark.parametrize("level", [2, 4])
def test_feature_regions_synthetic_vs_fp64(torch_cuda, wct16, level):
    torch = torch_cuda
    rng = np.random.default_rng(4)          # a seed at which the oracle's decisions all win by >= 3e-4 (seed and every Lloyd step, both levels)
    K, iters = 3, 10
    content, style = _flat_regions(rng, 96, 128, COLOURS), _flat_regions(rng, 80, 112, COLOURS[::-1])
    lc, ls, cen = wct16.feature_regions(cu(torch, content), cu(torch, style), K, level, iters, want_centroids=True)
    lc2, ls2, cen2 = wct16.feature_regions(cu(torch, content), cu(torch, style), K, level, iters, want_centroids=True)
    assert torch.equal(lc, lc2) and torch.equal(ls, ls2) and torch.equal(cen, cen2)          # bitwise reproducible
    cen_h = cen.cpu().numpy()
    s = 1 << (level - 1)
    for img, lab in ((style, ls), (content, lc)):
        f, sh, sc = _device_standardisation(wct16, torch, level, img)
        fh = f.cpu().numpy()[0]
        z = G.zmap(fh, sh, sc)
        lab_h = lab.cpu().numpy()
        assert lab_h.shape == img.shape[1:] and lab_h.max() < K
        small = lab_h[::s, ::s][: fh.shape[0], : fh.shape[1]]
        assert np.array_equal(lab_h, G.expand(small, level, *img.shape[1:]))                    # the expansion, exactly
        check_labels(small, z, cen_h, 0.01)
        if img is style:                                                                        # the oracle's own loop on the same features
            want, idx, costs, unclear, margins = G.lloyd(z, K, iters)
            assert min(margins) >= 1e-4 and max(unclear) == 0, (margins, unclear)               # the input is chosen so
            assert rel_err(cen_h, want) <= 1e-5
            # the same loop from the public calls: the same bits, and a cost that never rises
            dev = (f, cu(torch, sh), cu(torch, sc))
            c_d = wct16.kmeans_seed(*dev, K)[0]
            got_costs = []
            for _ in range(iters):
                _, _, _, cost, c_d = wct16.kmeans_assign(*dev, c_d, want_labels=False)
                got_costs.append(cost.item())
            assert rel_err(c_d.cpu().numpy(), cen_h) <= 1e-6
            assert all(b <= a * (1 + 1e-6) for a, b in zip(got_costs, got_costs[1:])), got_costs
            assert rel_err(np.array(got_costs), np.array(costs)) <= 1e-5


def test_feature_regions_expansion_off_the_grid(torch_cuda, wct16):
    """100 x 130 at level 4 (s = 8): 12 x 16 feature pixels, the last 4 rows and 2 columns repeat the last cell."""
    torch = torch_cuda
    rng = np.random.default_rng(8)
    content, style = _flat_regions(rng, 100, 130, COLOURS), _flat_regions(rng, 83, 117, COLOURS)
    lc, ls = wct16.feature_regions(cu(torch, content), cu(torch, style), 3, 4, 5)
    for lab, (H, W) in ((lc, (100, 130)), (ls, (83, 117))):
        lab_h = lab.cpu().numpy()
        small = lab_h[::8, ::8][: H // 8, : W // 8]
        assert lab_h.shape == (H, W) and np.array_equal(lab_h, G.expand(small, 4, H, W))
    for bad in (dict(level=1), dict(level=6), dict(iters=0), dict(iters=65), dict(K=0), dict(K=9)):
        kw = dict(K=3, level=4, iters=5)
        kw.update(bad)
        with pytest.raises(ValueError):
            wct16.feature_regions(cu(torch, content), cu(torch, style), kw["K"], kw["level"], kw["iters"])


@pytest.mark.parametrize("level", [2, 4])
def test_feature_regions_natural_frame(torch_cuda, wct16, level):
    torch = torch_cuda
    K, iters = 4, 10
    content = _jpg("g11_uhd_content_3840x2160.jpg", 192, 256, 800, 1600)
    style = _jpg("g11_style_2048x2048.jpg", 160, 208, 900, 900)
    lc, ls, cen = wct16.feature_regions(cu(torch, content), cu(torch, style), K, level, iters, want_centroids=True)
    cen_h = cen.cpu().numpy()
    s = 1 << (level - 1)
    for img, lab in ((style, ls), (content, lc)):
        f, sh, sc = _device_standardisation(wct16, torch, level, img)
        fh = f.cpu().numpy()[0]
        z = G.zmap(fh, sh, sc)
        if img is style:
            own_cent = G.lloyd(z, K, iters)[0]
        own = 1.0 - G.clear_pixels(G.distances(z, own_cent), z)[0].mean()          # the fp64 oracle's own share on this crop
        assert own <= 0.025, "choose another crop: the oracle alone leaves %.3g unclear" % own
        small = lab.cpu().numpy()[::s, ::s][: fh.shape[0], : fh.shape[1]]
        check_labels(small, z, cen_h, min(0.05, 2 * own))


# ---------------------------------------------------------------------------------------------------- 4. guided level and cascade
def _guided_level_from_entries(torch, wct, level, img, lab_full, styles, style_labs, region_style, alpha):
    cF = wct.encode(level, cu(torch, img)[None], layout="nhwc")
    _, h, w, C = cF.shape
    lab = cu(torch, region_oracle.level_labels(lab_full, level, h, w))
    K = len(region_style)
    n, s, ss = wct.moments_labeled(cF, lab, K)
    M = torch.zeros((K, C, C), dtype=torch.float64, device="cuda")
    b = torch.zeros((K, C), dtype=torch.float64, device="cuda")
    for k in range(K):
        M[k] = torch.eye(C, dtype=torch.float64, device="cuda")
        if n[k].item() < 2:
            continue
        sF = wct.encode(level, cu(torch, styles[region_style[k]])[None], layout="nhwc")
        if style_labs[region_style[k]] is None:
            ns, sm, ssq = wct.moments(sF)
        else:
            slab = cu(torch, region_oracle.level_labels(style_labs[region_style[k]], level, sF.shape[1], sF.shape[2]))
            nn, smm, ssqq = wct.moments_labeled(sF, slab, K)
            ns, sm, ssq = nn[k].item(), smm[k], ssqq[k]
            if ns < 2:
                continue
        M[k], b[k] = wct.solve(n[k].item(), s[k], ss[k], ns, sm, ssq, alpha=alpha[k])
    csF = wct.apply_labeled(cF, lab, M, b)
    return wct.decode(level, csF, layout="nhwc").cpu().numpy()[0]


def test_one_guided_level_from_split_entries_vs_oracle(torch_cuda, oracle, weights16x, wct16):
    H, W = 160, 224
    rng = np.random.default_rng(H + W)
    img = _smooth(rng, (3, H, W))
    styles = [_smooth(rng, (3, 96, 112)), rng.random((3, 80, 96), dtype=np.float32)]
    slabs = [_masks("split", 96, 112), _masks("disc", 80, 96)]
    lab = _masks("split", H, W)
    lab[: H // 5] = 255
    alpha, rs = [1.0, 0.6], [0, 1]
    mods, mods64 = oracle.Modules("16x", weights16x), oracle.Modules("16x", weights16x, precision="fp64")
    for level in (5, 4, 3, 2, 1):
        ref = G.region_transfer(mods, level, img, lab, styles, slabs, rs, alpha)
        ref64 = G.region_transfer(mods64, level, img, lab, styles, slabs, rs, alpha)
        assert rel_err(ref, ref64) < 2e-4 / 4, level                       # the two oracles agree: no covariance cut at the eigenvalue threshold
        got = _guided_level_from_entries(torch_cuda, wct16, level, img, lab, styles, slabs, rs, alpha)
        assert got.shape == ref.shape
        assert rel_err(got, ref) < 2e-4, level
        img = ref


GUIDED_CASES = {
    # content frame, content mask kind, styles (crop or None = smooth noise), style mask kinds (None = unmapped), region_style, alpha
    "split": ((512, 512), "split", [(256, 256, 900, 900)], ["split"], [0, 0], [1.0, 0.6]),
    "disc": ((512, 512), "disc", [(256, 256, 900, 900), None], ["disc", None], [0, 1], [1.0, 0.6]),
    "three+255": ((376, 632), "three+255", [(192, 224, 100, 1500), (256, 256, 900, 900)], ["split", "disc"], [0, 1, 0], [1.0, 0.6, 0.8]),
}


@pytest.mark.parametrize("name", list(GUIDED_CASES))
def test_stylize_guided_vs_oracle(torch_cuda, oracle, weights16x, wct16, name):
    (H, W), mask, crops, skinds, rs, alpha = GUIDED_CASES[name]
    rng = np.random.default_rng(H * 7 + len(mask))
    content = _jpg("g11_uhd_content_3840x2160.jpg", H, W, 800, 1600)
    styles = [_jpg("g11_style_2048x2048.jpg", *c) if c else _smooth(rng, (3, 200, 240)) for c in crops]
    slabs = [None if k is None else _masks(k, *s.shape[1:]) for k, s in zip(skinds, styles)]
    if name == "three+255":
        slabs[0] = np.where(slabs[0] == 1, 2, 0).astype(np.uint8)           # style 0 serves regions 0 (its left half) and 2 (its right half)
    lab = _masks(mask, H, W)
    mods, mods64 = oracle.Modules("16x", weights16x), oracle.Modules("16x", weights16x, precision="fp64")
    ref = G.stylize_guided(mods, content, styles, lab, slabs, rs, alpha)
    ref64 = G.stylize_guided(mods64, content, styles, lab, slabs, rs, alpha)
    assert rel_err(ref, ref64) < 1e-3 / 4
    got = wct16.stylize_guided(cu(torch_cuda, content), [cu(torch_cuda, s) for s in styles], cu(torch_cuda, lab),
                               [None if m is None else cu(torch_cuda, m) for m in slabs], rs, alpha).cpu().numpy()[0]
    assert got.shape == ref.shape
    assert rel_err(got, ref) < 1e-3


# ---------------------------------------------------------------------------------------------------- 5. identities and refusals
def _small_case(torch, rng, H=128, W=160):
    c = _smooth(rng, (3, H, W))
    styles = [_smooth(rng, (3, 96, 96)), rng.random((3, 64, 80), dtype=np.float32)]
    lab = _masks("split", H, W)
    lab[:16] = 255
    return c, styles, lab


def test_guided_without_maps_is_stylize_regions(torch_cuda, wct16):
    torch = torch_cuda
    c, styles, lab = _small_case(torch, np.random.default_rng(21))
    cs = [cu(torch, s) for s in styles]
    ref = wct16.stylize_regions(cu(torch, c), cs, cu(torch, lab), [1.0, 0.7]).clone()
    assert torch.equal(wct16.stylize_guided(cu(torch, c), cs, cu(torch, lab), None, None, [1.0, 0.7]), ref)
    assert torch.equal(wct16.stylize_guided(cu(torch, c), cs, cu(torch, lab), [None, None], [0, 1], [1.0, 0.7]), ref)
    assert torch.equal(wct16.stylize_regions(cu(torch, c), cs, cu(torch, lab), [1.0, 0.7]), ref)


def test_guided_shared_style_and_region_order(torch_cuda, wct16):
    torch = torch_cuda
    c, styles, lab = _small_case(torch, np.random.default_rng(22))
    smap = _masks("split", 96, 96)
    args = (cu(torch, c), [cu(torch, styles[0])], cu(torch, lab), [cu(torch, smap)])
    a = wct16.stylize_guided(*args, [0, 0], [1.0, 0.7]).clone()
    # the regions in the other order, content and style labels renumbered with them
    swap = np.concatenate([np.array([1, 0], np.uint8), np.arange(2, 256, dtype=np.uint8)])
    b = wct16.stylize_guided(cu(torch, c), [cu(torch, styles[0])], cu(torch, swap[lab]), [cu(torch, swap[smap])], [0, 0], [0.7, 1.0])
    assert rel_err(b.cpu().numpy(), a.cpu().numpy()) <= 1e-6
    # the same style passed twice, each region naming its own copy
    two = wct16.stylize_guided(cu(torch, c), [cu(torch, styles[0])] * 2, cu(torch, lab), [cu(torch, smap)] * 2, [0, 1], [1.0, 0.7])
    assert rel_err(two.cpu().numpy(), a.cpu().numpy()) <= 1e-6


def test_guided_style_label_absent_at_the_deep_level(torch_cuda, oracle, weights16x, wct16):
    """Style label 1 is a 15 x 15 block between the level-5 sampling points (rows and columns 8, 24, ...: the block is 9..23) that holds
    4 pixels at level 4 and more below: region 1 keeps its features at level 5 and is styled at the shallower levels."""
    torch = torch_cuda
    c, styles, lab = _small_case(torch, np.random.default_rng(23))
    smap = np.zeros((96, 96), np.uint8)
    smap[9:24, 9:24] = 1
    counts = [int((region_oracle.level_labels(smap, L, 96 >> (L - 1), 96 >> (L - 1)) == 1).sum()) for L in (5, 4, 3, 2, 1)]
    assert counts[0] == 0 and min(counts[1:]) >= 2, counts
    mods = oracle.Modules("16x", weights16x)
    ref = G.stylize_guided(mods, c, [styles[0]], lab, [smap], [0, 0], [1.0, 1.0])
    got = wct16.stylize_guided(cu(torch, c), [cu(torch, styles[0])], cu(torch, lab), [cu(torch, smap)], [0, 0], [1.0, 1.0])
    assert bool(torch.isfinite(got).all()) and rel_err(got.cpu().numpy()[0], ref) < 1e-3
    # level 5 alone: region 1's features pass through unchanged, region 0's do not
    lvl = _guided_level_from_entries(torch, wct16, 5, c, lab, [styles[0]], [smap], [0, 0], [1.0, 1.0])
    assert rel_err(lvl, G.region_transfer(mods, 5, c, lab, [styles[0]], [smap], [0, 0], [1.0, 1.0])) < 2e-4


def test_guided_refusals_leave_out_untouched(torch_cuda, wct16):
    torch = torch_cuda
    c, styles, lab = _small_case(torch, np.random.default_rng(24))
    H, W = lab.shape
    cs = [cu(torch, s) for s in styles]
    good = cu(torch, _masks("split", 96, 96))
    bad = _masks("split", 96, 96)
    bad[3, 5] = 7
    out = torch.full((3, H, W), -3.0, device="cuda")

    def refused(match, *a, **kw):
        with pytest.raises(ValueError, match=match):
            wct16.stylize_guided(cu(torch, c), *a, out=out, **kw)
        torch.cuda.synchronize()
        assert bool((out == -3.0).all())

    refused("style 0 label value 7", cs, cu(torch, lab), [cu(torch, bad), None], [0, 1], 1.0)
    badc = lab.copy()
    badc[100, 2] = 4
    refused("label value 4", cs, cu(torch, badc), [good, None], [0, 1], 1.0)
    refused("region_style", cs, cu(torch, lab), [good, None], [0, 2], 1.0)
    refused("region_style", cs, cu(torch, lab), [good, None], [-1, 0], 1.0)
    refused("K=9", cs, cu(torch, lab), [good, None], [0] * 9, 1.0)
    refused("S=9", [cs[0]] * 9, cu(torch, lab), [None] * 9, [0, 1], 1.0)
    with pytest.raises(ValueError, match="S=0"):
        wct16.stylize_guided(cu(torch, c), [], cu(torch, lab), [], [0], 1.0, out=out)
    wct16.set_transform("ot")
    try:
        refused("wct transform only", cs, cu(torch, lab), [good, None], [0, 1], 1.0)
    finally:
        wct16.set_transform("wct")
    assert bool(torch.isfinite(wct16.stylize_guided(cu(torch, c), cs, cu(torch, lab), [good, None], [0, 1], 1.0, out=out)).all())


@pytest.mark.parametrize("H,W", [(64, 80), (70, 90)])
def test_guided_num_run_equals_chained_runs(torch_cuda, wct16, H, W):
    """As test_regions_num_run_equals_chained_runs: bit for bit, both parities of the ping-pong, the cropping first run."""
    torch = torch_cuda
    rng = np.random.default_rng(17)
    Hc, Wc = H // 16 * 16, W // 16 * 16
    c = cu(torch, _smooth(rng, (3, H, W)))
    styles = [cu(torch, _smooth(rng, (3, 48, 64)))]
    smap = [cu(torch, _masks("split", 48, 64))]
    lab = np.zeros((H, W), np.uint8)
    lab[:, W // 2:] = 1
    lab[:8] = 255
    lab = cu(torch, lab)

    def run(img, n, out=None):
        return wct16.stylize_guided(img, styles, lab[:img.shape[-2], :img.shape[-1]], smap, [0, 0], [1.0, 0.7], num_run=n, out=out)

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


# ---------------------------------------------------------------------------------------------------- 6. call-history independence
def test_guided_calls_leave_no_trace(torch_cuda, weights16x, wct16):
    torch = torch_cuda
    from wct_hip import WCT
    rng = np.random.default_rng(31)
    c, styles, lab = _small_case(torch, rng)
    cd, cs, ld = cu(torch, c), [cu(torch, s) for s in styles], cu(torch, lab)
    prepared = cu(torch, _smooth(rng, (3, 72, 88)))
    used = WCT(types.SimpleNamespace(mode="16x", alpha=1.0), weights=weights16x)
    used.style_prepare(prepared)
    used.stylize_guided(cd, cs, ld, [cu(torch, _masks("disc", 96, 96)), None], [0, 1], [1.0, 0.5], num_run=2)
    used.feature_regions(cd, cs[0], 5, 3, 4)
    via_slot = used.stylize_prepared(cd, 0.8).clone()                             # the prepared slot survived both calls
    fresh = WCT(types.SimpleNamespace(mode="16x", alpha=1.0), weights=weights16x)
    fresh.style_prepare(prepared)
    assert torch.equal(via_slot, fresh.stylize_prepared(cd, 0.8))
    assert torch.equal(used.stylize(cd, cs[1], 0.9), fresh.stylize(cd, cs[1], 0.9))
    assert torch.equal(used.stylize_regions(cd, cs, ld, [1.0, 0.6]), fresh.stylize_regions(cd, cs, ld, [1.0, 0.6]))
    assert wlib.SYMBOLS_GUIDED
