"""A catalogue of calls: every compute entry point of include/wct_hip.h, once, as a *case*.

    CASES[name] = Case(fn, covers, size, family, wide)
    fn(engine, seed) -> {output name: torch tensor}

A case builds its inputs from a seeded CPU `torch.Generator` / numpy `default_rng`, so it is a pure function of the engine's
weights and its own seed: whatever the engine did before, the outputs must be the same bits (tests/test_state_gpu.py).  A case
never synchronises on its own account (the streams arm relies on it) and returns freshly allocated device tensors.

Every family exists at two sizes that differ in every tile count: "small" around 100 x 130 (not a multiple of 16) and "large" around
600 x 900 (not a multiple of 32).  `wide` marks the small cases that also run on the un-pruned engine (model_zoo.synth_weights("original", 7)):
there the C > 128 solves are deferred to the end of the call (ok_log, defer_big, the deflated iteration's workspaces).

The module imports without a GPU (tests/test_state_cpu.py checks that the catalogue covers wct_hip.lib.SYMBOLS)."""
import collections
import os
import types

import numpy as np

Case = collections.namedtuple("Case", "fn covers size family wide")
CASES = collections.OrderedDict()

SIZES = {"small": (100, 130, 84, 108), "large": (600, 900, 520, 700)}     # content H, W; style Hs, Ws
SEED = 20240


def case(family, covers, sizes=("small", "large"), wide=False):
    def deco(f):
        for size in sizes:
            CASES["%s/%s" % (family, size)] = Case((lambda eng, seed, _f=f, _s=size: _f(eng, seed, _s)), tuple(covers), size, family,
                                                  wide and size == "small")
        return f
    return deco


# ------------------------------------------------------------------------------------------------ engines
_WEIGHTS = {}


def weights(kind):
    from wct_hip import model_zoo
    from tests.conftest import PKG
    if kind not in _WEIGHTS:
        _WEIGHTS[kind] = model_zoo.load_npz_weights(os.path.join(PKG, "weights", "16x.npz")) if kind == "16x" else \
            model_zoo.synth_weights("original", 7)
    return _WEIGHTS[kind]


def make_engine(kind="16x", w=None):
    """A fresh engine (a new wct_ctx): kind "16x" = --mode 16x on the shipped weights, "wide" = --mode original on synthetic ones."""
    from wct_hip import WCT
    eng = WCT(types.SimpleNamespace(mode="16x" if kind == "16x" else "original", alpha=1.0), weights=weights(kind) if w is None else w)
    eng.state_kind = kind
    return eng


def names(kind="16x", size=None):
    return [n for n, c in CASES.items() if (kind == "16x" or c.wide) and (size is None or c.size == size)]


# ------------------------------------------------------------------------------------------------ inputs
def _torch():
    import torch
    return torch


def _gen(seed):
    g = _torch().Generator()
    g.manual_seed(int(seed))
    return g


def rand(seed, *shape):
    t = _torch()
    return t.rand(shape, generator=_gen(seed)).cuda()


def image(seed, H, W):
    return rand(seed, 1, 3, H, W)


def image_u8(seed, H, W):
    t = _torch()
    return t.randint(0, 256, (H, W, 3), generator=_gen(seed), dtype=t.uint8).cuda()


def feature(seed, h, w, C):
    """An NHWC feature map with correlated, non-negative channels (what a ReLU leaves)."""
    t = _torch()
    g = _gen(seed)
    base = t.rand((h, w, C), generator=g)
    mix = t.rand((C, C), generator=g) * (0.5 / C) + t.eye(C)
    return (base @ mix).reshape(1, h, w, C).contiguous().cuda()


def label_map(H, W, K, block=16):
    """Blocky labels 0..K-1 and 255 (unstyled): every value owns many pixels at every level of the cascade."""
    t = _torch()
    y = t.arange(H).reshape(H, 1) // block
    x = t.arange(W).reshape(1, W) // block
    lab = (y + x) % (K + 1)
    lab[lab == K] = 255
    return lab.to(t.uint8).cuda()


def weight_maps(seed, K, H, W):
    """K per-pixel weights in [0, 1] that sum to less than 1 everywhere."""
    w = _torch().rand((K, H, W), generator=_gen(seed))
    return (w / (w.sum(0, keepdim=True) + 0.25)).contiguous().cuda()


def affine(seed, K, C):
    """K maps (M, b) near the identity, fp64."""
    rng = np.random.default_rng(seed)
    M = np.eye(C)[None] + 0.05 * rng.standard_normal((K, C, C))
    b = 0.1 * rng.standard_normal((K, C))
    t = _torch()
    return t.from_numpy(M).cuda(), t.from_numpy(b).cuda()


def raw_moments(seed, C, n, lo):
    """(n, n mu, (n - 1) cov + n mu mu^T) of a covariance with eigenvalues from 1 down to `lo`."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((C, C)))
    cov = (Q * np.exp(np.linspace(0.0, np.log(lo), C))) @ Q.T
    cov = (cov + cov.T) / 2
    mu = rng.random(C)
    t = _torch()
    return float(n), t.from_numpy(n * mu).cuda(), t.from_numpy((n - 1) * cov + n * np.outer(mu, mu)).cuda()


def channels(eng, level):
    from wct_hip import model_zoo
    return model_zoo.feature_channels(eng.mode, level)


def styles(seed, K, size):
    """K style images of different sizes: the first at the size class's style size, the others smaller."""
    Hs, Ws = SIZES[size][2:]
    return [image(seed + 10 * k, max(40, Hs - 13 * k), max(48, Ws - 9 * k)) for k in range(K)]


# ------------------------------------------------------------------------------------------------ the cascade
@case("stylize", ["wct_stylize"], wide=True)
def _stylize(eng, seed, size):
    H, W, Hs, Ws = SIZES[size]
    c, s = image(seed, H, W), image(seed + 1, Hs, Ws)
    return {"alpha1": eng.stylize(c, s, alpha=1.0, num_run=1), "alpha06_run2": eng.stylize(c, s, alpha=0.6, num_run=2)}


@case("prepared", ["wct_style_prepare", "wct_style_prepare_levels", "wct_stylize_prepared"], wide=True)
def _prepared(eng, seed, size):
    H, W, Hs, Ws = SIZES[size]
    c, s, s2 = image(seed, H, W), image(seed + 1, Hs, Ws), image(seed + 2, Hs - 7, Ws - 5)
    eng.style_prepare(s)
    out = {"levels": eng.stylize_prepared(c, alpha=0.8)}
    eng._style_keep = s2
    eng._stream()
    eng._chk(eng._lib.wct_style_prepare(eng._ctx, s2.data_ptr(), int(s2.shape[2]), int(s2.shape[3])))
    out["all"] = eng.stylize_prepared(c, num_run=2)
    return out


@case("export_import", ["wct_style_export", "wct_style_import", "wct_stylize_prepared"])
def _export_import(eng, seed, size):
    H, W, Hs, Ws = SIZES[size]
    c, s = image(seed, H, W), image(seed + 1, Hs, Ws)
    peer = make_engine(eng.state_kind)
    peer.style_prepare(s)
    out = {}
    for L in (5, 4, 3, 2, 1):
        eng.style_import(L, peer.style_export(L))
    out["out"] = eng.stylize_prepared(c)
    for L in (5, 4, 3, 2, 1):
        out["stats%d" % L] = eng.style_export(L)
    return out


@case("stylize_u8", ["wct_stylize_u8"])
def _stylize_u8(eng, seed, size):
    H, W, Hs, Ws = SIZES[size]
    c, s = image_u8(seed, H, W), image_u8(seed + 1, Hs, Ws)
    return {"floor": eng.stylize_u8(c, s), "round_a07": eng.stylize_u8(c, s, alpha=0.7, round_mode=1)}


@case("level", ["wct_style_transfer_level"], wide=True)
def _level(eng, seed, size):
    H, W, Hs, Ws = SIZES[size]
    c, s = image(seed, H, W), image(seed + 1, Hs, Ws)
    return {"level%d" % L: eng.style_transfer_level(L, c, s, alpha=0.9) for L in (5, 4, 3, 2, 1)}


@case("encode_decode", ["wct_encode", "wct_decode"])
def _encode_decode(eng, seed, size):
    H, W = SIZES[size][:2]
    c = image(seed, H, W)
    out = {}
    for L in (1, 2, 3, 4, 5):
        f = eng.encode(L, c)
        g = eng.encode(L, c, layout="nhwc")
        out["enc%d_nchw" % L], out["enc%d_nhwc" % L] = f, g
        out["dec%d_nchw" % L] = eng.decode(L, f)
        out["dec%d_nhwc" % L] = eng.decode(L, g, layout="nhwc")
    return out


# ------------------------------------------------------------------------------------------------ the split form
@case("moments", ["wct_moments"])
def _moments(eng, seed, size):
    h, w, C = (25, 32, 64) if size == "small" else (260, 300, 32)      # large: 78 000 pixels >= 65 536 -> the fp32-block form
    f = feature(seed, h, w, C)
    _, s, ss = eng.moments(f)
    _, sw, ssw = eng.moments(f, 3, w - 5)
    return {"sum": s, "sumsq": ss, "sum_window": sw, "sumsq_window": ssw}


@case("solve", ["wct_solve"], wide=True)
def _solve(eng, seed, size):
    C = (512 if eng.state_kind == "wide" else 64) if size == "small" else 128
    M, b = eng.solve(*raw_moments(seed, C, 50000, 1e-3), *raw_moments(seed + 1, C, 20000, 1e-2), alpha=1.0)
    M2, b2 = eng.solve(*raw_moments(seed + 2, C, 9000, 1e-5), *raw_moments(seed + 3, C, 30000, 1e-4), alpha=0.6)
    return {"M": M, "b": b, "M_ill": M2, "b_ill": b2}


@case("apply", ["wct_apply"])
def _apply(eng, seed, size):
    t = _torch()
    h, w, C = (25, 33, 64) if size == "small" else (150, 225, 32)
    f = feature(seed, h, w, C)
    M, b = affine(seed + 1, 1, C)
    out = {}
    for name, layout, x in (("nhwc", 0, f), ("nchw", 1, f.permute(0, 3, 1, 2).contiguous())):
        o = t.empty_like(x)
        eng._stream()
        eng._chk(eng._lib.wct_apply(eng._ctx, x.data_ptr(), C, h, w, layout, M.data_ptr(), b.data_ptr(), o.data_ptr()))
        out[name] = o
    return out


@case("transform", ["wct_transform"], wide=True)
def _transform(eng, seed, size):
    C, h, w, hs, ws = (128, 12, 16, 10, 13) if size == "small" else (32, 150, 225, 130, 175)
    if eng.state_kind == "wide":
        C, h, w, hs, ws = 256, 24, 32, 20, 26
    cF = feature(seed, h, w, C)[0].permute(2, 0, 1).contiguous()
    sF = feature(seed + 1, hs, ws, C)[0].permute(2, 0, 1).contiguous()
    return {"a1": eng.transform(cF, sF, alpha=1.0), "a05": eng.transform(cF, sF, alpha=0.5)}


@case("decode_affine", ["wct_decode_affine"])
def _decode_affine(eng, seed, size):
    H, W = SIZES[size][:2]
    out = {}
    for L in (3, 1):
        C = channels(eng, L)
        h, w = H >> (L - 1), W >> (L - 1)
        M, b = affine(seed + L, 1, C)
        out["level%d" % L] = eng.decode_affine(L, feature(seed, h, w, C), M[0], b[0])
    return out


@case("split_level", ["wct_content_encode", "wct_content_solve", "wct_content_decode", "wct_style_prepare_levels"], wide=True)
def _split_level(eng, seed, size):
    H, W, Hs, Ws = SIZES[size]
    c, s = image(seed, H, W), image(seed + 1, Hs, Ws)
    eng.style_prepare(s, levels=(4, 1))
    out = {}
    for L in (4, 1):
        h, w, sm, ss = eng.content_encode(L, c)
        M, b = eng.content_solve(L, float(h * w), sm, ss, alpha=0.9)
        out["sum%d" % L], out["sumsq%d" % L], out["M%d" % L], out["b%d" % L] = sm, ss, M, b
        out["img%d" % L] = eng.content_decode(L, M, b, H, W)
    return out


@case("style_split", ["wct_style_moments", "wct_style_solve", "wct_style_export"])
def _style_split(eng, seed, size):
    Hs, Ws = SIZES[size][2:]
    s = image(seed, Hs, Ws)
    out = {}
    for L in (3, 5):
        sm, ss = eng.style_moments(L, s)
        _, h, w = eng.feature_shape(L, Hs, Ws)
        eng.style_solve(L, float(h * w), sm, ss)
        out["sum%d" % L], out["sumsq%d" % L], out["stats%d" % L] = sm, ss, eng.style_export(L)
    return out


# ------------------------------------------------------------------------------------------------ spatial control
def _feat_labels(seed, size, K):
    t = _torch()
    h, w, C = (25, 33, 64) if size == "small" else (150, 225, 32)
    lab = t.randint(0, K + 1, (h, w), generator=_gen(seed + 5))
    lab[lab == K] = 255
    return feature(seed, h, w, C), lab.to(t.uint8).cuda(), h, w, C


@case("moments_labeled", ["wct_moments_labeled"])
def _moments_labeled(eng, seed, size):
    out = {}
    for K in (1, 5):
        f, lab, h, w, C = _feat_labels(seed, size, K)
        out["n%d" % K], out["sum%d" % K], out["sumsq%d" % K] = eng.moments_labeled(f, lab, K)
    return out


@case("apply_labeled", ["wct_apply_labeled"])
def _apply_labeled(eng, seed, size):
    K = 3
    f, lab, h, w, C = _feat_labels(seed, size, K)
    M, b = affine(seed + 1, K, C)
    return {"nhwc": eng.apply_labeled(f, lab, M, b), "nchw": eng.apply_labeled(f.permute(0, 3, 1, 2).contiguous(), lab, M, b, layout="nchw")}


@case("regions", ["wct_stylize_regions"], wide=True)
def _regions(eng, seed, size):
    H, W = SIZES[size][:2]
    c = image(seed, H, W)
    out = {}
    for K in ((3,) if eng.state_kind == "wide" else (8, 1, 3)):
        out["K%d" % K] = eng.stylize_regions(c, styles(seed + 1, K, size), label_map(H, W, K), alpha=[1.0 - 0.05 * k for k in range(K)])
    return out


# ------------------------------------------------------------------------------------------------ interpolation and weights
@case("moments_weighted", ["wct_moments_weighted"])
def _moments_weighted(eng, seed, size):
    K = 3
    f, _, h, w, C = _feat_labels(seed, size, K)
    s, ss = eng.moments_weighted(f, weight_maps(seed + 2, K, h, w))
    return {"sum": s, "sumsq": ss}


@case("apply_mixed", ["wct_apply_mixed"])
def _apply_mixed(eng, seed, size):
    K = 3
    f, _, h, w, C = _feat_labels(seed, size, K)
    wt = weight_maps(seed + 2, K, h, w)
    M, b = affine(seed + 1, K, C)
    return {"nhwc": eng.apply_mixed(f, wt, M, b), "nchw": eng.apply_mixed(f.permute(0, 3, 1, 2).contiguous(), wt, M, b, layout="nchw")}


@case("interp", ["wct_stylize_interp"], wide=True)
def _interp(eng, seed, size):
    H, W = SIZES[size][:2]
    c = image(seed, H, W)
    out = {}
    for K in ((2,) if eng.state_kind == "wide" else (5, 2)):
        out["K%d" % K] = eng.stylize_interp(c, styles(seed + 1, K, size), [1.0 + k for k in range(K)], alpha=0.8)
    return out


@case("style_blend", ["wct_style_blend", "wct_style_export", "wct_style_prepare_levels", "wct_stylize_prepared"])
def _style_blend(eng, seed, size):
    H, W = SIZES[size][:2]
    c = image(seed, H, W)
    stats = []
    for s in styles(seed + 1, 3, size):
        eng.style_prepare(s)
        stats.append({L: eng.style_export(L) for L in (5, 4, 3, 2, 1)})
    eng.style_blend(stats, [0.5, 0.3, 0.2])
    return {"out": eng.stylize_prepared(c), "stats5": eng.style_export(5), "stats1": eng.style_export(1)}


@case("blend", ["wct_stylize_blend"])
def _blend(eng, seed, size):
    H, W = SIZES[size][:2]
    c = image(seed, H, W)
    return {"K%d" % K: eng.stylize_blend(c, styles(seed + 1, K, size), weight_maps(seed + 3, K, H, W), alpha=[1.0 - 0.1 * k for k in range(K)])
            for K in (4, 2)}


# ------------------------------------------------------------------------------------------------ synthesis
@case("noise", ["wct_noise_uniform"])
def _noise(eng, seed, size):
    H, W = SIZES[size][:2]
    return {"a": eng.noise(H, W, seed=seed), "b": eng.noise(H - 1, W + 3, seed=seed + (1 << 40), stream_id=7)}


@case("synthesize", ["wct_synthesize", "wct_style_prepare_levels"], wide=True)
def _synthesize(eng, seed, size):
    H, W, Hs, Ws = SIZES[size]
    tex = image(seed, Hs, Ws)
    out = {"texture": eng.synthesize(tex, H, W, seed=seed, stream_id=2, alpha=0.9)}
    eng.style_prepare(image(seed + 1, Hs - 3, Ws - 6))
    out["prepared"] = eng.synthesize(None, H, W, seed=seed + 1)
    return out


# ------------------------------------------------------------------------------------------------ the image edge
@case("image_edge", ["wct_u8_to_planar", "wct_planar_to_u8"])
def _image_edge(eng, seed, size):
    H, W = SIZES[size][:2]
    x = (image(seed, H, W) * 1.2 - 0.1)
    return {"to_tensor": eng.to_tensor_u8(image_u8(seed + 1, H, W)), "to_u8_floor": eng.to_u8(x, 0), "to_u8_round": eng.to_u8(x, 1)}


@case("resize", ["wct_resize_u8", "wct_resize_u8_to_planar", "wct_resize_u8_filter"])
def _resize(eng, seed, size):
    H, W = SIZES[size][:2]
    x = image_u8(seed, H, W)
    oH, oW = (H * 3 // 5 + 1, W * 3 // 5 + 2)
    return {"bilinear_edge": eng.resize_u8(x, 64), "bilinear": eng.resize_u8(x, (oH, oW)), "bilinear_planar": eng.resize_u8(x, (oH, oW), to_tensor=True),
            "bicubic": eng.resize_u8(x, (oH + 40, oW + 9), filter="bicubic"),
            "bicubic_planar": eng.resize_u8(x, (oH + 40, oW + 9), to_tensor=True, filter="bicubic")}


# ------------------------------------------------------------------------------------------------ workspace
def workspace_bytes(eng, H, W, Hs, Ws):
    return int(eng._lib.wct_workspace_bytes(eng._ctx, H, W, Hs, Ws))


@case("reserve", ["wct_reserve", "wct_workspace_bytes", "wct_stylize"])
def _reserve(eng, seed, size):
    t = _torch()
    H, W, Hs, Ws = SIZES[size]
    eng.reserve(H, W, Hs, Ws)
    c, s = image(seed, H, W), image(seed + 1, Hs, Ws)
    return {"out": eng.stylize(c, s), "bytes": t.tensor([workspace_bytes(eng, H, W, Hs, Ws)], dtype=t.int64).cuda()}


def covered():
    return set(sym for c in CASES.values() for sym in c.covers)


def run(eng, name, seed=SEED):
    return CASES[name].fn(eng, seed)
