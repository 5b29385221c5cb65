"""Custom model widths on the MI355X against fp64 (tests/width_models.py): the kernel variants behind `wct_load_module`'s width rules.

Modules are loaded through the C ABI on a context of this file's own (the WCT class hard-codes model_zoo's widths).  Every case
turns profiling on and asserts the kernel families it claims to cover really ran, and that no f16x3 operand saturated."""
import numpy as np
import pytest

from tests import width_models as wm
from tests.conftest import rel_err
from tests.gpu_ctx import Ctx
from wct_hip import lib as _lib

pytestmark = pytest.mark.gpu

ENC_DEC_GATE = wm.ENC_DEC_GATE
MOM_GATE = wm.MOM_GATE
FP32_FORM_GATE = 1e-7    # wct_moments with fp32 products (mom32 on a >= 65 536-pixel map) against numpy fp64


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need the MI355X"
    return t


@pytest.fixture
def ctx(torch):
    c = Ctx(torch)
    yield c
    c.close()


def _families(names, want, banned=()):
    missing = [f for f in want if f not in names]
    bad = [n for n in names for b in banned if b in n]
    assert not missing and not bad, "kernel families: missing %s, unexpected %s; ran %s" % (missing, bad, sorted(names))


# ---------------------------------------------------------------------------------------------------- a. conv families per model
# (H, W) per model: ragged 32 x 8 / 32 x 16 tiles at full resolution, odd sizes at every pooling, 2-3 pixel maps at level 5
SIZES = {"A": (37, 53), "B": (45, 83), "C": (41, 36)}


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("model", sorted(wm.MODELS))
def test_model_encode_decode_vs_fp64(ctx, model, mode):
    widths = wm.MODELS[model]
    w = wm.synth(widths, seed=ord(model))
    ctx.load(widths, w)
    ctx.conv_mode(mode)
    rng = np.random.default_rng(ord(model) + 10 * mode)
    H, W = SIZES[model]
    img = wm.smooth_image(rng, H, W)
    ctx.profile_start()
    feats = {}
    for level in (5, 4, 3, 2, 1):
        ref = wm.encode(widths, w, level, img)
        got = ctx.encode(level, img)
        assert got.shape == ref.shape
        # gate: the oracle gate, or the reference's own fp32 distance from fp64 where a deep random stack makes that the larger
        e32 = rel_err(wm.encode(widths, w, level, img, f64=False), ref)
        err = rel_err(got, ref)
        assert err < max(ENC_DEC_GATE, 4 * e32), "encoder %d: %.3e (fp32 arm %.3e)" % (level, err, e32)
        # decode a well-spread feature of the level's shape: the encoded one plus a positive perturbation
        f = np.maximum(ref + 0.3 * np.abs(ref).max() * rng.standard_normal(ref.shape), 0).astype(np.float32)
        refd = wm.decode(widths, w, level, f)
        e32d = rel_err(wm.decode(widths, w, level, f, f64=False), refd)
        gotd = ctx.decode(level, f)
        errd = rel_err(gotd, refd)
        assert errd < max(ENC_DEC_GATE, 4 * e32d), "decoder %d: %.3e (fp32 arm %.3e)" % (level, errd, e32d)
        feats[level] = (ref, refd, f, max(ENC_DEC_GATE, 4 * e32), max(ENC_DEC_GATE, 4 * e32d))
        print("widths %s mode %d level %d: encode %.2e (fp32 %.2e) decode %.2e (fp32 %.2e)" % (model, mode, level, err, e32, errd, e32d))
    names = ctx.profile_names()
    if mode == 1:
        _families(names, *wm.FAMILIES[model])
    else:
        _families(names, ("conv3x3_f32<co=%d,in3>" % min(wm.pad_cout(widths[1]), 128),), ("f16x3", "l1_"))
    assert ctx.saturation() == 0
    # the SP16 hand-over, the upsample form and the fused ends are rewrites of the same layers: with each switched off the stacks meet the
    # same fp64 gates (a different kernel, a different summation order: not bitwise)
    if mode == 1:
        for key in ("sp", "upconv", "fuse"):
            ctx.set(key, 0)
            try:
                for level in (5, 4, 3, 2, 1):
                    ref, refd, f, ge, gd = feats[level]
                    assert rel_err(ctx.encode(level, img), ref) < ge, (key, level)
                    assert rel_err(ctx.decode(level, f), refd) < gd, (key, level)
            finally:
                ctx.set(key, 1)


# ---------------------------------------------------------------------------------------------------- b. level 1 at every width
@pytest.mark.parametrize("size", [(29, 45), (272, 1100)])
@pytest.mark.parametrize("C", wm.L1_WIDTHS)
def test_level1_width_vs_fp64(ctx, C, size):
    widths = wm.level1_widths(C)
    w = wm.synth(widths, seed=100 + C, levels=(1,))
    ctx.load(widths, w, levels=(1,))
    rng = np.random.default_rng(C)
    H, W = size
    img = wm.smooth_image(rng, H, W)
    F = wm.encode(widths, w, 1, img)
    x0, x1 = W // 3, W // 3 + 17                      # an interior column window (not 32-aligned)
    M = np.eye(C) + 0.1 * rng.standard_normal((C, C)) / np.sqrt(C)
    b = rng.standard_normal(C) * 0.1 * np.abs(F).max()
    refd = wm.decode_affine(widths, w, 1, F, M, b)
    fused = 17 <= C <= 24
    outs = {}
    for l1fuse in (1, 0):
        ctx.set("l1fuse", l1fuse)
        try:
            ctx.profile_start()
            got = ctx.encode(1, img)
            assert rel_err(got, F) < ENC_DEC_GATE
            for win in ((0, -1), (x0, x1)):
                s, ss = ctx.content_encode(1, img, *win)
                rs, rss = wm.raw_moments(F, win[0], None if win[1] < 0 else win[1])
                es, ess = rel_err(s, rs), rel_err(ss, rss)
                assert es < MOM_GATE and ess < MOM_GATE, "C=%d window %s: sum %.3e sumsq %.3e" % (C, win, es, ess)
            d = ctx.content_decode(1, M, b, H, W)
            ed = rel_err(d, refd)
            assert ed < ENC_DEC_GATE, "C=%d decode: %.3e" % (C, ed)
            names = ctx.profile_names()
        finally:
            ctx.set("l1fuse", 1)
        outs[l1fuse] = d
        fam = ("l1_moments_fused<3-24>", "l1_decode_fused<3-24-3>")
        if l1fuse and fused:
            _families(names, fam + ("l1_encode<3-24>",))
        elif l1fuse:
            _families(names, ("l1_encode<3-24>", "moments", "fold_affine"), fam)
        else:
            _families(names, ("conv3x3_f32<co=%d,in3>" % wm.pad_cout(C), "moments"), ("l1_",))
        print("widths level1 C=%d %dx%d l1fuse %d: decode %.2e" % (C, H, W, l1fuse, ed))
    assert rel_err(outs[1], outs[0]) < 2e-6
    assert ctx.saturation() == 0


# ---------------------------------------------------------------------------------------------------- c. moments and solve
@pytest.mark.parametrize("C", wm.MOMENT_WIDTHS)
def test_moments_and_solve_width(ctx, C):
    rng = np.random.default_rng(C)
    # a small map (fp64 products either way) and one of >= 65 536 pixels (fp32 products under mom32 = 1)
    for h, w in ((23, 37), (256, 260)):
        f = np.maximum(rng.standard_normal((h, w, C)).astype(np.float32) + 0.3, 0)
        X = f.astype(np.float64)
        for x0, x1 in ((0, w), (w // 5, w // 5 + 11)):
            Xw = X[:, x0:x1].reshape(-1, C)
            rs, rss = Xw.sum(0), Xw.T @ Xw
            for mom32 in (0, 1):
                ctx.set("mom32", mom32)
                try:
                    s, ss = ctx.moments(f, x0, x1)
                finally:
                    ctx.set("mom32", 1)
                bound = FP32_FORM_GATE if (mom32 and h * w >= 65536) else 1e-13
                assert rel_err(s, rs) < bound and rel_err(ss, rss) < bound, (C, h, w, mom32, x0, x1, rel_err(s, rs), rel_err(ss, rss))
                assert np.array_equal(ss, ss.T)
    # the matrix functions on well-conditioned statistics (n >= 4 C): ns_pad 192 / 320 / 448 among them
    from oracle import wct_oracle
    n = 4 * C + 64
    A = rng.standard_normal((C, C)) / np.sqrt(C) + np.eye(C)
    Xc = rng.standard_normal((n, C)) @ A.T + 1.0
    Xs = rng.standard_normal((n + 17, C)) @ (A.T + 0.2) - 0.5
    st = [(x.shape[0], x.sum(0), x.T @ x) for x in (Xc, Xs)]
    M, b = ctx.solve(C, *st[0], *st[1], 0.6)
    mu = [s / k for k, s, _ in st]
    cov = [(q - k * np.outer(m, m)) / (k - 1) for (k, _, q), m in zip(st, mu)]
    Mr, br = wct_oracle.affine_from_moments(mu[0], cov[0], mu[1], cov[1], 0.6)
    assert rel_err(M, Mr) < 1e-8 and rel_err(b, br) < 1e-8, (C, rel_err(M, Mr), rel_err(b, br))


# ---------------------------------------------------------------------------------------------------- refusals at load time
@pytest.mark.parametrize("case", wm.REFUSED, ids=[c[0] for c in wm.REFUSED])
def test_unsupported_shapes_refused_at_load(ctx, case):
    name, kind, level, spec = case
    rng = np.random.default_rng(0)
    layers = [wm.Layer("L%d" % i, cin, cout, pool_after=bool(p), up_after=bool(u)) for i, (cin, cout, p, u) in enumerate(spec)]
    w = {}
    key = ("e" if kind == "enc" else "d") + str(level)
    for l in layers:
        w["%s.%s.weight" % (key, l.name)] = (rng.random((l.cout, l.cin, 3, 3)).astype(np.float32) - 0.5) * 0.1
        w["%s.%s.bias" % (key, l.name)] = np.zeros(l.cout, np.float32)
    w[key + ".conv0.weight"], w[key + ".conv0.bias"] = wm.model_zoo.ORIGINAL_CONV0_W, wm.model_zoo.ORIGINAL_CONV0_B
    rc, msg = ctx.rc_msg(ctx.load_layers(kind, level, layers, w, key))
    assert rc == _lib.WCT_ERR_INVALID and "load_module" in msg, (name, rc, msg)


# ---------------------------------------------------------------------------------------------------- e. one full model
def test_model_a_levels_and_cascade(ctx):
    widths = wm.MODELS["A"]
    w = wm.synth(widths, seed=ord("A"))
    ctx.load(widths, w)
    rng = np.random.default_rng(5)
    c, s = wm.smooth_image(rng, 256, 256), wm.smooth_image(rng, 240, 256)
    alpha = 0.6
    img = c
    for level in (5, 4, 3, 2, 1):
        r64 = wm.style_transfer(widths, w, level, img, s, alpha, f64=True)
        r32 = wm.style_transfer(widths, w, level, img, s, alpha, f64=False)
        got = ctx.style_transfer_level(level, img, s, alpha)
        e_gpu, e32 = rel_err(got, r64), rel_err(r32, r64)
        print("widths A level %d: gpu %.2e fp32 arm %.2e (vs fp64)" % (level, e_gpu, e32))
        assert e_gpu <= 4 * e32 + 1e-4, (level, e_gpu, e32)
        img = r64.astype(np.float32)           # level-isolated: fp64's output feeds the next level of both sides
    chain = c
    for level in (5, 4, 3, 2, 1):
        chain = ctx.style_transfer_level(level, chain, s, alpha)
    full = ctx.stylize(c, s, alpha)
    assert np.array_equal(full, chain)
    assert np.array_equal(ctx.stylize(c, s, alpha, prepared=True), full)
    assert ctx.saturation() == 0
