"""All 128 loadable widths through the feature-space kernels on the MI355X against fp64 (tests/sweep_cases.py).

Parametrised by band (16 bands of 8 widths, small and large mixed, in a fixed non-monotonic order); one context per band and section,
its scratch poisoned with 0xFF (a kernel that reads scratch it did not write meets NaNs) and "prof_forms" on: sections a, b and e
assert per case that the launcher reports the form the restated plan predicts.

  a  wct_moments                    at plan-derived boundary pixel counts, fp64 products (1e-13) and fp32-block products (derived bound)
  b  wct_moments_labeled / _weighted the same counts from their plan; absent label, single-pixel label, a zero-weight tile; bitwise repeatable
  c  wct_apply                      against fp64 M x + b, both layouts and conv modes
  d  wct_apply_labeled / _mixed     at the PT boundary counts, 1e-6; unstyled pixels bit for bit
  e  wct_decode_affine              a thin (C -> 3) and a square (C -> C -> 3) decoder per width: every fold form
  f  wct_solve, wct_transform_solve every front end of launch_eig; widths 100..128 again on a wide-model context (deflated iteration)
  g  one whole level at the fast-fold widths no shipped model has, fastfold 1 and 0

Every section prints its largest error against the gate ("sweep <section> ..." lines)."""
import numpy as np
import pytest

from oracle import wct_oracle
from tests import sweep_cases as S
from tests import transform_oracle as O
from tests import width_models as wm
from tests.conftest import rel_err
from tests.gpu_ctx import Ctx
from tests.test_transform_gpu import GATE_WELL, cond_live, gate_for
from wct_hip import model_zoo
from wct_hip.model_zoo import Layer

pytestmark = pytest.mark.gpu

ENC_DEC_GATE = wm.ENC_DEC_GATE
APPLY_GATE = 1e-6          # tests/test_regions_gpu.py, tests/test_blend_gpu.py
SOLVE_GATE = 1e-8          # tests/test_widths_gpu.py test_moments_and_solve_width
BANDS = list(range(S.N_BANDS))


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need the MI355X"
    return t


def _new_ctx(torch):
    c = Ctx(torch)
    c.set("poison", 0xFF)
    c.set("prof_forms", 1)
    return c


@pytest.fixture
def ctx(torch):
    c = _new_ctx(torch)
    yield c
    c.close()


def _profiled(ctx, fn):
    ctx.profile_start()
    out = fn()
    return out, ctx.profile_names()


def _one(names, family):
    """the one profile name of `family` ("moments" must not match "moments_labeled")"""
    hit = [n for n in names if n.split(":")[0] == family]
    assert len(hit) == 1, (family, sorted(names))
    return hit[0]


class Worst:
    """largest error / gate of a section, printed at its end"""

    def __init__(self):
        self.r, self.what = 0.0, ""

    def add(self, err, gate, what):
        r = float(err) / gate
        if r > self.r:
            self.r, self.what = r, "%s: %.2e of %.1e" % (what, err, gate)

    def __str__(self):
        return "%.3f of the gate (%s)" % (self.r, self.what)


def _entrywise(got, ref, bound, what):
    """|got - ref| <= bound entry by entry; returns the largest ratio"""
    d = np.abs(np.asarray(got, np.float64) - ref)
    bad = d > bound
    assert not bad.any(), "%s: %d entries beyond the fp32-form bound, worst %.3e against %.3e" % (
        what, int(bad.sum()), float(d[bad].max()), float(np.asarray(bound)[bad].min()))
    nz = bound > 0
    return float((d[nz] / bound[nz]).max()) if nz.any() else 0.0


# ---------------------------------------------------------------------------------------------------- a. wct_moments
@pytest.mark.parametrize("b", BANDS)
def test_a_moments(ctx, b):
    w64, w32 = Worst(), Worst()
    for C in S.BANDS[b]:
        tile = S.geometry(C)["MP"]
        for case in S.moments_cases(C):
            f = S.feature(C, case, tile, seed=1000 * C + len(case.name))
            rs, rss, asum, asq = S.raw_moments(S.window_pixels(f, case))
            npix = S.npix_of(case)
            for mom32 in (0, 2):
                what = "C=%d %s (%d px) mom32=%d" % (C, case.name, npix, mom32)
                ctx.set("mom32", mom32)
                (s, ss), names = _profiled(ctx, lambda: ctx.moments(f, case.x0, case.x1))
                assert _one(names, "moments") == "moments:" + S.moments_launch(C, npix, mom32 == 2)["suffix"], (what, sorted(names))
                assert np.isfinite(s).all() and np.isfinite(ss).all(), what
                if mom32 == 0:
                    es, ess = rel_err(s, rs), rel_err(ss, rss)
                    w64.add(max(es, ess), S.GATE64, what)
                    assert es < S.GATE64 and ess < S.GATE64, (what, es, ess)
                    assert np.array_equal(ss, ss.T), what
                else:
                    bs, bq = S.bound_f32(asum, asq, rss)
                    w32.add(max(_entrywise(s, rs, bs, what + " sum"), _entrywise(ss, rss, bq, what + " sumsq")), 1.0, what)
    print("sweep a band %d: fp64 form %s; fp32 form %s" % (b, w64, w32))


# ---------------------------------------------------------------------------------------------------- b. labeled / weighted moments
def _labels(rng, n, tile):
    """K = 3: label 0 on random pixels among 255s, label 1 absent, label 2 on the last pixel alone; the sentinel pixel `tile` is styled"""
    lab = np.where(rng.random(n) < 0.3, 255, 0).astype(np.uint8)
    if tile < n:
        lab[tile] = 0
    lab[n - 1] = 2
    return lab


def _weights(rng, n, tile):
    """K = 2: weight 0 vanishes on the whole second tile, weight 1 on the whole first one (the skip path); the last pixel counts fully"""
    w = rng.random((2, n), dtype=np.float32)
    w[0, tile:2 * tile] = 0
    w[1, :tile] = 0
    w[0, n - 1] = 1
    return w


@pytest.mark.parametrize("b", BANDS)
def test_b_moments_labeled_and_weighted(ctx, b):
    worst = {k: Worst() for k in ("labeled fp64", "labeled fp32", "weighted fp64", "weighted fp32")}
    for C in S.BANDS[b]:
        tile = S.apply_pt(C)
        for case in S.kw_cases(C):
            n = S.npix_of(case)
            rng = np.random.default_rng(2000 * C + n)
            f = S.feature(C, case, tile, seed=3000 * C + len(case.name))
            X = S.window_pixels(f, case)
            lab, wts = _labels(rng, n, tile), _weights(rng, n, tile)
            ref_l = [S.raw_moments(X[lab == k]) for k in range(3)]
            ref_w = [S.raw_moments(X, wts[k]) for k in range(2)]
            for mom32 in (0, 2):
                ctx.set("mom32", mom32)
                what = "C=%d %s (%d px) mom32=%d" % (C, case.name, n, mom32)
                (cnt, s, ss), names = _profiled(ctx, lambda: ctx.moments_labeled(f, lab.reshape(case.h, -1), 3))
                assert _one(names, "moments_labeled") == "moments_labeled:" + S.kw_suffix(C, mom32 == 2), (what, sorted(names))
                again = ctx.moments_labeled(f, lab.reshape(case.h, -1), 3)
                assert all(np.array_equal(x, y) for x, y in zip((cnt, s, ss), again)), what + ": labeled moments differ between two calls"
                (sw, ssw), names = _profiled(ctx, lambda: ctx.moments_weighted(f, wts.reshape(2, case.h, -1)))
                assert _one(names, "moments_weighted") == "moments_weighted:" + S.kw_suffix(C, mom32 == 2), (what, sorted(names))
                again = ctx.moments_weighted(f, wts.reshape(2, case.h, -1))
                assert np.array_equal(sw, again[0]) and np.array_equal(ssw, again[1]), what + ": weighted moments differ between two calls"
                assert [int(v) for v in cnt] == [int((lab == k).sum()) for k in range(3)], what
                for kind, refs, got_s, got_ss in (("labeled", ref_l, s, ss), ("weighted", ref_w, sw, ssw)):
                    for k, (rs, rss, asum, asq) in enumerate(refs):
                        wk = "%s %s k=%d" % (what, kind, k)
                        assert np.isfinite(got_s[k]).all() and np.isfinite(got_ss[k]).all(), wk
                        if mom32 == 0:
                            es, ess = rel_err(got_s[k], rs), rel_err(got_ss[k], rss)
                            worst[kind + " fp64"].add(max(es, ess), S.GATE64, wk)
                            assert es < S.GATE64 and ess < S.GATE64, (wk, es, ess)
                            assert np.array_equal(got_ss[k], got_ss[k].T), wk
                        else:
                            bs, bq = S.bound_f32(asum, asq, rss)
                            worst[kind + " fp32"].add(max(_entrywise(got_s[k], rs, bs, wk + " sum"), _entrywise(got_ss[k], rss, bq, wk + " sumsq")), 1.0, wk)
    print("sweep b band %d: %s" % (b, "; ".join("%s %s" % kv for kv in worst.items())))


# ---------------------------------------------------------------------------------------------------- c. wct_apply
@pytest.mark.parametrize("b", BANDS)
def test_c_apply(ctx, b):
    worst = Worst()
    for C in S.BANDS[b]:
        rng = np.random.default_rng(4000 + C)
        M = np.eye(C) + 0.1 * rng.standard_normal((C, C)) / np.sqrt(C)
        for h, w in ((2, 2), (5, 7), (33, 17)):
            f = rng.standard_normal((h, w, C)).astype(np.float32)
            bb = rng.standard_normal(C) * 0.1 * np.abs(f).max()
            X = f.reshape(-1, C)
            ref = (X.astype(np.float64) @ M.T + bb).reshape(h, w, C)
            arm32 = (X @ M.astype(np.float32).T + bb.astype(np.float32)).reshape(h, w, C)
            gate = max(ENC_DEC_GATE, 4 * rel_err(arm32, ref))
            for mode in (1, 0):
                ctx.conv_mode(mode)
                for nchw in (False, True):
                    got = ctx.apply(f.transpose(2, 0, 1) if nchw else f, M, bb, nchw=nchw)
                    got = got.transpose(1, 2, 0) if nchw else got
                    err = rel_err(got, ref)
                    what = "C=%d %dx%d conv mode %d %s" % (C, h, w, mode, "nchw" if nchw else "nhwc")
                    worst.add(err, gate, what)
                    assert err < gate, (what, err, gate)
    assert ctx.saturation() == 0
    print("sweep c band %d: %s" % (b, worst))


# ---------------------------------------------------------------------------------------------------- d. labeled / mixed apply
@pytest.mark.parametrize("b", BANDS)
def test_d_apply_labeled_and_mixed(ctx, b):
    wl, wx = Worst(), Worst()
    for C in S.BANDS[b]:
        rng = np.random.default_rng(5000 + C)
        M = rng.standard_normal((3, C, C)) / np.sqrt(C)
        bb = rng.standard_normal((3, C))
        for case in S.apply_cases(C):
            h, w, n = case.h, case.wfull, S.npix_of(case)
            f = rng.standard_normal((h, w, C)).astype(np.float32)
            X = f.reshape(n, C).astype(np.float64)
            # labels 0..2, 255, and 7 (>= K, not 255); the last pixel is styled
            lab = rng.choice(np.array([0, 1, 2, 255, 7], np.uint8), size=n, p=[0.3, 0.25, 0.2, 0.15, 0.1])
            lab[n - 1] = 2
            ref = X.copy()
            for k in range(3):
                ref[lab == k] = X[lab == k] @ M[k].T + bb[k]
            wts = rng.random((2, n), dtype=np.float32) * 0.5
            wts[:, rng.random(n) < 0.2] = 0
            wts[0, n - 1] = 0.5
            refx = X + sum(wts[k].astype(np.float64)[:, None] * ((X @ M[k].T + bb[k]) - X) for k in range(2))
            for nchw in ((False, True) if case.name == "two+1" else (False,)):
                what = "C=%d %s (%d px) %s" % (C, case.name, n, "nchw" if nchw else "nhwc")
                fin = f.transpose(2, 0, 1) if nchw else f
                back = (lambda a: a.transpose(1, 2, 0)) if nchw else (lambda a: a)
                got = back(ctx.apply_labeled(fin, lab.reshape(h, w), M, bb, nchw=nchw)).reshape(n, C)
                err = rel_err(got, ref)
                wl.add(err, APPLY_GATE, what)
                assert err <= APPLY_GATE, (what, "labeled", err)
                keep = lab >= 3
                assert np.array_equal(got[keep], f.reshape(n, C)[keep]), what + ": an unstyled pixel was not copied through"
                gotx = back(ctx.apply_mixed(fin, wts.reshape(2, h, w), M[:2], bb[:2], nchw=nchw)).reshape(n, C)
                errx = rel_err(gotx, refx)
                wx.add(errx, APPLY_GATE, what)
                assert errx <= APPLY_GATE, (what, "mixed", errx)
    print("sweep d band %d: labeled %s; mixed %s" % (b, wl, wx))


# ---------------------------------------------------------------------------------------------------- e. wct_decode_affine
def _layer_weights(rng, key, layers):
    """He-uniform stand-ins as tests/width_models.synth builds them (the last decoder conv scaled by 1/128)"""
    w = {}
    for l in layers:
        wt = (rng.random((l.cout, l.cin, 3, 3)) * 2.0 - 1.0) * np.sqrt(6.0 / (9 * l.cin))
        last = key[0] == "d" and l.cout == 3
        w["%s.%s.weight" % (key, l.name)] = (wt / 128.0 if last else wt).astype(np.float32)
        w["%s.%s.bias" % (key, l.name)] = (rng.random(l.cout) * 0.1 + (0.2 if last else 0.0)).astype(np.float32)
    if key[0] == "e":
        w[key + ".conv0.weight"], w[key + ".conv0.bias"] = model_zoo.ORIGINAL_CONV0_W.copy(), model_zoo.ORIGINAL_CONV0_B.copy()
    return w


def _walk(layers, w, key, y, f64):
    conv = wct_oracle.conv3x3_reflect_f64 if f64 else wct_oracle.conv3x3_reflect
    y = np.ascontiguousarray(y, np.float64 if f64 else np.float32)
    for l in layers:
        y = conv(y, w["%s.%s.weight" % (key, l.name)], w["%s.%s.bias" % (key, l.name)], True)
    return y


@pytest.mark.parametrize("b", BANDS)
def test_e_decode_affine(ctx, b):
    worst = Worst()
    for C in S.BANDS[b]:
        rng = np.random.default_rng(6000 + C)
        feat = np.maximum(rng.standard_normal((C, 5, 7)) + 0.3, 0).astype(np.float32)
        M = np.eye(C) + 0.1 * rng.standard_normal((C, C)) / np.sqrt(C)
        bb = rng.standard_normal(C) * 0.1 * np.abs(feat).max()
        y = (M @ feat.reshape(C, -1).astype(np.float64) + bb[:, None]).reshape(feat.shape)
        for shape, layers in (("thin", [Layer("a", C, 3)]), ("square", [Layer("a", C, C), Layer("b", C, 3)])):
            w = _layer_weights(rng, "d1", layers)
            ctx.chk(ctx.load_layers("dec", 1, layers, w, "d1"))
            ref = _walk(layers, w, "d1", y, True)
            gate = max(ENC_DEC_GATE, 4 * rel_err(_walk(layers, w, "d1", y.astype(np.float32), False), ref))
            gemm = S.fold_gemm_capable(layers[0].cout, C, S.pad_cout(layers[0].cout))
            for foldgemm in ((1, 0) if gemm else (1,)):
                ctx.set("foldgemm", foldgemm)
                try:
                    got, names = _profiled(ctx, lambda: ctx.decode_affine(1, feat, M, bb))
                finally:
                    ctx.set("foldgemm", 1)
                what = "C=%d %s foldgemm %d" % (C, shape, foldgemm)
                assert _one(names, "fold_affine") == "fold_affine:" + S.fold_form(C, layers[0].cout, foldgemm=bool(foldgemm)), (what, sorted(names))
                err = rel_err(got, ref)
                worst.add(err, gate, what)
                assert err < gate, (what, err, gate)
    assert ctx.saturation() == 0
    print("sweep e band %d: %s" % (b, worst))


# ---------------------------------------------------------------------------------------------------- f. solves
#: one ulp on the raw moments moves cov_c^(-1/2) by about 2^-53 cond(cov_c) of its largest entries: where that passes a tenth of the 1e-8
#: gate, fp64 inputs do not determine (M, b) to the gate (numpy's own reference moves by 6e-9 at cond 6e8 when the covariance is formed
#: from centred instead of raw sums), and the width's statistics are drawn again
SOLVE_MAX_COND = 1e-9 / 2.0 ** -53


def _stats(C, well=False):
    """test_moments_and_solve_width's statistics: n = 4 C + 64 samples through the mixing matrix I + randn / sqrt(C), redrawn (next
    seed) while cond(cov_c) > SOLVE_MAX_COND = 9e6 -- six of the 128 widths on their first seed.
    well: a quarter of the random part and an independent draw on the style side -- see _solve_width."""
    for k in range(8):
        rng = np.random.default_rng((7500 if well else 7000) + C + 1000 * k)
        n = 4 * C + 64
        g = 0.25 if well else 1.0
        A = g * rng.standard_normal((C, C)) / np.sqrt(C) + np.eye(C)
        As = g * rng.standard_normal((C, C)) / np.sqrt(C) + np.eye(C) if well else A + 0.2
        Xc = rng.standard_normal((n, C)) @ A.T + 1.0
        Xs = rng.standard_normal((n + 17, C)) @ As.T - 0.5
        lam = np.linalg.eigvalsh(np.cov(Xc.T))
        if lam[-1] <= SOLVE_MAX_COND * lam[0]:
            return [(x.shape[0], x.sum(0), x.T @ x) for x in (Xc, Xs)]
    raise AssertionError("C=%d: no well-determined statistics in 8 draws" % C)


def _transform_side(st):
    """what the transform_solve checks need of a statistics pair: content moments, style export, R = cov_c^(1/2), mu_c, cond(B)"""
    (nc, sc, ssc), (ns, ssum, sss) = st
    mu_c, cov_c = O.mean_cov(nc, sc, ssc)
    mu_s, cov_s = O.mean_cov(ns, ssum, sss)
    Sroot = O.sym_pow(cov_s, 0.5)
    cond, rank = cond_live(O.ot_B(cov_c, Sroot))
    return dict(n=nc, s=sc, ss=ssc, st=O.stats(Sroot, mu_s), R=O.sym_pow(cov_c, 0.5), mu_c=mu_c, cond=cond, rank=rank)


def _check_transform(ctx, mode, C, t, gate, tag, worst, want_ns=False):
    Mt, bt, it = ctx.transform_solve(mode, C, t["n"], t["s"], t["ss"], t["st"], 0.6)
    Mo, bo = O.solve(mode, t["n"], t["s"], t["ss"], t["st"], 0.6)
    e_map, e_mean = rel_err(Mt @ t["R"], Mo @ t["R"]), rel_err(Mt @ t["mu_c"] + bt, Mo @ t["mu_c"] + bo)
    worst.add(max(e_map, e_mean), gate, tag)
    assert e_map < gate and e_mean < gate, (tag, mode, e_map, e_mean, gate, it)
    if mode == "adain":
        assert it[0] == 0, (tag, it)
    elif want_ns:
        assert 0 < it[0] < 100, (tag, mode, it)      # the matrix-core iteration, not the Jacobi net (100 + sweeps)


def _solve_width(ctx, C, wide, worst):
    """wct_solve and wct_transform_solve (wct, ot, adain) of one width against fp64; returns wct_solve's info.

    wct_solve, and the wct and adain modes of wct_transform_solve, run on test_moments_and_solve_width's statistics at 1e-8.  Those
    statistics are NOT well-conditioned for ot: B = S cov_c S multiplies two covariances' spectra, and the style side's mixing matrix
    (A + 0.2) makes cond(B) 1e9 at C = 100, 4e12 at C = 64, 1e15 and more from C = 452 -- numpy's own fp64 T_ot then disagrees with the
    SVD form of the same map by 1e-4 (C = 64, 452), so no 1e-8 gate can be read off it.  The ot mode is therefore held to the
    well-conditioned gate, at every width, on statistics of the same construction that ARE well-conditioned (a quarter of the random part,
    cond(B) < 100, asserted <= 1e6), and on the original statistics wherever tests/test_transform_gpu.py gate_for defines a gate
    (cond(B) <= 1e10: 1e-8 up to 1e6, 1e-6 above)."""
    lit = _stats(C)
    (nc, sc, ssc), (ns, ssum, sss) = lit
    mu_c, cov_c = O.mean_cov(nc, sc, ssc)
    mu_s, cov_s = O.mean_cov(ns, ssum, sss)
    tag = "C=%d [%s]" % (C, S.eig_front_end(C, wide))
    M, bvec, info = ctx.solve_info(C, nc, sc, ssc, ns, ssum, sss, 0.6)
    Mr, br = wct_oracle.affine_from_moments(mu_c, cov_c, mu_s, cov_s, 0.6)
    eM, eb = rel_err(M, Mr), rel_err(bvec, br)
    worst["wct_solve"].add(max(eM, eb), SOLVE_GATE, tag)
    assert eM < SOLVE_GATE and eb < SOLVE_GATE, (tag, eM, eb, info)
    # (info is the caller's to judge: as built, the style covariance of some widths is ill-conditioned enough for the Jacobi net, 100 + sweeps)
    t = _transform_side(lit)
    _check_transform(ctx, "wct", C, t, GATE_WELL, tag, worst["wct"])
    _check_transform(ctx, "adain", C, t, GATE_WELL, tag, worst["adain"])
    if t["rank"] == C and t["cond"] <= 1e10:
        _check_transform(ctx, "ot", C, t, gate_for(t["cond"], True), tag + " cond(B) %.1e" % t["cond"], worst["ot as built"])
    tw = _transform_side(_stats(C, well=True))
    assert tw["rank"] == C and tw["cond"] <= 1e6, (tag, tw["cond"])
    _check_transform(ctx, "ot", C, tw, GATE_WELL, tag, worst["ot"], want_ns=True)
    return info


@pytest.mark.parametrize("b", BANDS)
def test_f_solves(torch, ctx, b):
    worst = {k: Worst() for k in ("wct_solve", "wct", "adain", "ot", "ot as built")}
    seen = set()
    for C in S.BANDS[b]:
        _solve_width(ctx, C, False, worst)
        seen.add(S.eig_front_end(C, False))
    print("sweep f band %d [%s]: %s" % (b, " ".join(sorted(seen)), "; ".join("%s %s" % kv for kv in worst.items())))
    again = [C for C in S.BANDS[b] if 100 <= C <= 128]
    if again:
        # a context with an encoder wider than 128 channels loaded: wide_model routes ns_pad = 128 to the deflated iteration
        wide = _new_ctx(torch)
        try:
            layers = [Layer("a", 3, 64), Layer("b", 64, 132)]
            wide.chk(wide.load_layers("enc", 2, layers, _layer_weights(np.random.default_rng(1), "e2", layers), "e2"))
            worst = {k: Worst() for k in worst}
            for C in again:
                assert S.eig_front_end(C, True) == "deflated4"
                info = _solve_width(wide, C, True, worst)
                # without deflation ns_pad = 128 runs a 16-step schedule: a converged count above 16 is the deflated iteration's (19-20)
                assert all(16 < i < 100 for i in info), (C, info)
            print("sweep f band %d wide model %s: %s" % (b, again, "; ".join("%s %s" % kv for kv in worst.items())))
        finally:
            wide.close()


# ---------------------------------------------------------------------------------------------------- g. one whole level
FAST_FOLD_WIDTHS = (8, 12, 16, 52, 60, 116, 120, 124)


def _encode_walk(layers, w, img, f64):
    if f64:
        w0 = np.asarray(w["e1.conv0.weight"], np.float64).reshape(3, 3)
        y = np.einsum("kc,chw->khw", w0, np.asarray(img, np.float64)) + np.asarray(w["e1.conv0.bias"], np.float64)[:, None, None]
    else:
        y = wct_oracle.conv1x1(img, w["e1.conv0.weight"], w["e1.conv0.bias"])
    return _walk(layers, w, "e1", y, f64)


@pytest.mark.parametrize("C", FAST_FOLD_WIDTHS)
def test_g_level_at_fast_fold_width(ctx, C):
    assert S.fold_fast_capable(C)
    enc = [Layer("a", 3, C)] if C <= 64 else [Layer("a", 3, 64), Layer("b", 64, C)]
    dec = [Layer(l.name, l.cout, l.cin) for l in reversed(enc)]
    rng = np.random.default_rng(8000 + C)
    w = dict(_layer_weights(rng, "e1", enc), **_layer_weights(rng, "d1", dec))
    ctx.chk(ctx.load_layers("enc", 1, enc, w, "e1"))
    ctx.chk(ctx.load_layers("dec", 1, dec, w, "d1"))
    ctx.widths = {"l1": C}
    c, s = wm.smooth_image(rng, 40, 52), wm.smooth_image(rng, 36, 44)
    ref = {}
    for f64 in (True, False):
        cF, sF = _encode_walk(enc, w, c, f64), _encode_walk(enc, w, s, f64)
        csF = wct_oracle.transform(cF, sF, 0.6, out_dtype=np.float64 if f64 else np.float32)[0]
        ref[f64] = _walk(dec, w, "d1", csF, f64)
    e32 = rel_err(ref[False], ref[True])
    for fastfold in (1, 0):
        ctx.set("fastfold", fastfold)
        try:
            got, names = _profiled(ctx, lambda: ctx.style_transfer_level(1, c, s, 0.6))
        finally:
            ctx.set("fastfold", 1)
        assert _one(names, "fold_affine") == "fold_affine:" + S.fold_form(C, dec[0].cout, fast=bool(fastfold)), (C, fastfold, sorted(names))
        e_gpu = rel_err(got, ref[True])
        print("sweep g C=%d fastfold %d: gpu %.2e fp32 arm %.2e (vs fp64), gate %.2e" % (C, fastfold, e_gpu, e32, 4 * e32 + 1e-4))
        assert e_gpu <= 4 * e32 + 1e-4, (C, fastfold, e_gpu, e32)
    assert ctx.saturation() == 0


# ---------------------------------------------------------------------------------------------------- what the sweep found
@pytest.mark.parametrize("size", [(5, 7), (9, 35)])
def test_eight_channel_intermediate_layer(ctx, size):
    """Section e at C = 8, square decoder, 5 x 7: the smallest case of the sweep's one finding.  An 8 -> 8 layer in front of another
    f16x3 layer hands its output over in SP16, and conv3x3_f16_c16_kernel placed the pixel records cout * 4 = 32 bytes apart where the
    format (and every consumer) has 64-byte records: every pixel but the first was read from the wrong place (8.5e-2 against a gate
    of 2e-5; 16 channels, the only width below 32 any shipped model has, made both strides equal)."""
    h, w = size
    rng = np.random.default_rng(8)
    dec = [Layer("a", 8, 8), Layer("b", 8, 3)]
    enc = [Layer("a", 3, 8), Layer("b", 8, 8), Layer("c", 8, 8)]
    wts = dict(_layer_weights(rng, "d1", dec), **_layer_weights(rng, "e1", enc))
    ctx.chk(ctx.load_layers("dec", 1, dec, wts, "d1"))
    ctx.chk(ctx.load_layers("enc", 1, enc, wts, "e1"))
    feat = np.maximum(rng.standard_normal((8, h, w)) + 0.3, 0).astype(np.float32)
    ref = _walk(dec, wts, "d1", feat, True)
    gate = max(ENC_DEC_GATE, 4 * rel_err(_walk(dec, wts, "d1", feat, False), ref))
    img = wm.smooth_image(rng, h, w)
    refe = _encode_walk(enc, wts, img, True)
    gatee = max(ENC_DEC_GATE, 4 * rel_err(_encode_walk(enc, wts, img, False), refe))
    for sp in (1, 0):
        ctx.set("sp", sp)
        try:
            err, erre = rel_err(ctx.decode(1, feat), ref), rel_err(ctx.encode(1, img), refe)
        finally:
            ctx.set("sp", 1)
        print("sweep finding 8 -> 8 at %dx%d sp %d: decoder %.2e (gate %.1e) encoder %.2e (gate %.1e)" % (h, w, sp, err, gate, erre, gatee))
        assert err < gate and erre < gatee, (size, sp, err, erre)
    assert ctx.saturation() == 0
