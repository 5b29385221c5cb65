"""The ot and adain transforms off the shipped widths and paths, on the MI355X against fp64.

1. wct_transform_solve at every width of tests/transform_cases.py (ragged 16-tiles, k-tails, every front end of launch_eig under the ot
   schedule) against tests/transform_oracle.py, through the quantities and gates of tests/test_transform_gpu.py check_solve: M R with
   R = cov_c^(1/2) and M mu_c + b; 1e-8 where cond(B) <= 1e6 or B is singular by rank, 1e-6 up to 1e10, adain 1e-8.  In the same test:
   nothing past C is written (M and b sit inside canary-filled buffers), nothing past C is read (a fresh context whose scratch is
   poisoned with 0xA5 gives the same bits), and the result is a function of the inputs (second call, fresh context: same bits).
2. --mode original under ot / adain: level-isolated against an fp64 arm, the call equivalences bit for bit, the forced fallback of
   the deferred solves.
3. Custom-width models (tests/width_models.py) under ot / adain against the fp64 restatement; wct_reserve under ot at cmax = 384.

Cascade gate: e_gpu <= 4 e32 + 1e-4 against the fp64 arm (tests/test_widths_gpu.py).  Iteration counts are printed, not asserted."""
import ctypes
import os
import subprocess
import sys
from ctypes import byref, c_int, c_void_p

import numpy as np
import pytest

from tests import state_cases as sc
from tests import transform_cases as TC
from tests import transform_oracle as O
from tests import width_models as wm
from tests.conftest import PKG, REPO, rel_err
from tests.test_transform_gpu import GATE_WELL, gate_for
from tests.test_widths_gpu import Ctx
from wct_hip import lib as _lib

pytestmark = pytest.mark.gpu

CANARY = 0x7FF8C0DEC0DE0001          # a quiet NaN with a payload: whoever reads it shows it, whoever overwrites it loses the payload
MODES = {"ot": _lib.TRANSFORM_OT, "adain": _lib.TRANSFORM_ADAIN}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need the MI355X"
    return t


# ------------------------------------------------------------------------------------------------ 1. raw moments at every width
class Solver(Ctx):
    """A bare wct_ctx (no modules: wct_transform_solve needs none) that solves into the middle of canary-filled buffers."""

    def __init__(self, torch, **debug):
        super().__init__(torch)
        for k, v in debug.items():
            self.set(k, v)

    def get(self, key):
        v = ctypes.c_double()
        self.chk(self.L.wct_debug_get(self.ctx, key.encode(), byref(v)))
        return v.value

    def solve(self, mode, C, n, dev, alpha):
        """-> (M bits [C*C], b bits [C], info): int64 views, so that comparisons are of bits."""
        t = self.t
        pad = 32 * C + 64                      # a store guard of 16 nt instead of C lands within 16 C doubles of the end
        Mb = t.full((pad + C * C + pad,), CANARY, dtype=t.int64, device="cuda")
        bb = t.full((pad + C + pad,), CANARY, dtype=t.int64, device="cuda")
        info = (c_int * 2)(-1, -1)
        t.cuda.synchronize()
        self.chk(self.L.wct_transform_solve(self.ctx, MODES[mode], C, float(n), dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), float(alpha),
                                            Mb.data_ptr() + 8 * pad, bb.data_ptr() + 8 * pad, info))
        self.sync()
        for buf, m, what in ((Mb, C * C, "M"), (bb, C, "b")):
            out = t.cat([buf[:pad], buf[pad + m:]])
            assert bool((out == CANARY).all()), "%s: %d elements outside [0, %d) written (C=%d, %s)" % (what, int((out != CANARY).sum()), m, C, mode)
        return Mb[pad:pad + C * C].clone(), bb[pad:pad + C].clone(), (info[0], info[1])


_REF = {}


def reference(name):
    """The fp64 side of a case, computed once: the inputs, what describe() says of them, R = cov_c^(1/2), mu_c."""
    if name not in _REF:
        n, s, ss, st = TC.build(name)
        d = TC.describe(n, s, ss, st)
        mu_c, cov_c = O.mean_cov(n, s, ss)
        _REF[name] = dict(n=n, s=s, ss=ss, st=st, d=d, R=O.sym_pow(cov_c, 0.5), mu_c=mu_c, mb={})
    return _REF[name]


def reference_mb(name, mode, alpha):
    r = reference(name)
    if (mode, alpha) not in r["mb"]:
        r["mb"][mode, alpha] = O.solve(mode, r["n"], r["s"], r["ss"], r["st"], alpha)
    return r["mb"][mode, alpha]


def f64(t, bits):
    return bits.view(t.float64).cpu().numpy()


@pytest.fixture(scope="module")
def shared(torch):
    """One context per solver setting that every width goes through, in the table's order: a used engine."""
    made = {}

    def get(**debug):
        key = tuple(sorted(debug.items()))
        if key not in made:
            made[key] = Solver(torch, **debug)
        return made[key]
    yield get
    for s in made.values():
        s.close()


@pytest.mark.parametrize("C", list(TC.WIDTHS))
def test_transform_solve_width(torch, shared, C):
    fe = TC.WIDTHS[C]
    # both solver settings that reach Cp = 128: the single-launch kernel, and the split-k multi-launch iteration with it switched off
    settings = ({}, {"nscoop": 0}) if fe == "single128" else ({},)
    for debug in settings:
        used = shared(**debug)
        for name in TC.names(C):
            r = reference(name)
            d, n = r["d"], r["n"]
            dev = [torch.from_numpy(np.ascontiguousarray(r[k], np.float64)).cuda() for k in ("s", "ss", "st")]
            for mode in ("ot", "adain"):
                fresh = Solver(torch, **debug)
                try:
                    for alpha in (1.0, 0.6):
                        coop0 = used.get("nscoop_solves")
                        M1, b1, info = used.solve(mode, C, n, dev, alpha)
                        coop = used.get("nscoop_solves") - coop0
                        M, b = f64(torch, M1).reshape(C, C), f64(torch, b1)
                        what = "%s %s alpha %.1f%s" % (name, mode, alpha, " nscoop=0" if debug else "")
                        assert np.isfinite(M).all() and np.isfinite(b).all(), what
                        # against the reference, on the content's support
                        Mr, br = reference_mb(name, mode, alpha)
                        full = d["rank"] == d["live"]
                        gate = gate_for(d["cond"], full) if mode == "ot" else GATE_WELL
                        e_map, e_mean = rel_err(M @ r["R"], Mr @ r["R"]), rel_err(M @ r["mu_c"] + b, Mr @ r["mu_c"] + br)
                        print("width %s [%s Cp %d nt %d]: cond(B) %.1e rank %d of %d live, info %s, coop %d, M R %.2e, M mu + b %.2e (gate %.0e)"
                              % (what, fe, TC.ns_pad(C), TC.tiles(C), d["cond"], d["rank"], d["live"], info, coop, e_map, e_mean, gate))
                        assert e_map < gate and e_mean < gate, (what, e_map, e_mean, gate)
                        assert info[1] == 0, what
                        if mode == "adain":
                            assert info[0] == 0, what
                            assert np.count_nonzero(M - np.diag(np.diag(M))) == 0, what
                        elif full and d["cond"] <= 1e9:
                            assert 0 < info[0] < 100, "%s: the matrix-core path did not handle B (info %d, cond %.1e)" % (what, info[0], d["cond"])
                        if mode == "ot" and name == "C88_rank":
                            assert info[0] >= 100, "%s: singular by rank under Cp = 96 must come back through the LDS Jacobi net (info %d)" % (what, info[0])
                        if mode == "ot" and fe == "single128":
                            assert coop == (0 if debug else 1), (what, coop)          # the setting reached the front end it names
                        # a function of the inputs: the second call, and a fresh context whose scratch holds 0xA5 wherever nothing was written
                        M2, b2, info2 = used.solve(mode, C, n, dev, alpha)
                        assert torch.equal(M2, M1) and torch.equal(b2, b1) and info2 == info, what + ": the second call differs"
                        fresh.set("poison", 0xA5)
                        M3, b3, info3 = fresh.solve(mode, C, n, dev, alpha)
                        assert torch.equal(M3, M1) and torch.equal(b3, b1) and info3 == info, what + ": a fresh, poisoned context differs"
                finally:
                    fresh.close()


# ------------------------------------------------------------------------------------------------ 2. --mode original
WIDE = (64, 80, 48, 64)          # content H, W; style Hs, Ws: the shapes of test_hip_parity.py test_wide_model_deferred_solves_fall_back
_WIDE_FEATS = {}


def _wide_inputs():
    H, W, Hs, Ws = WIDE
    return sc.image(61, H, W), sc.image(62, Hs, Ws)


def _wide_features(oracle, precision, level, c, s):
    """(modules, content feature, style feature) of an arm, encoded once for both transforms."""
    key = (precision, level)
    if key not in _WIDE_FEATS:
        if precision not in _WIDE_FEATS:
            _WIDE_FEATS[precision] = oracle.Modules("original", sc.weights("wide"), precision=precision)
        mods = _WIDE_FEATS[precision]
        dt = np.float64 if precision == "fp64" else np.float32
        _WIDE_FEATS[key] = (mods, mods.encode(level, np.asarray(c, dt)), mods.encode(level, np.asarray(s, dt)))
    return _WIDE_FEATS[key]


@pytest.mark.parametrize("mode", ["ot", "adain"])
def test_wide_model_levels_against_the_fp64_arm_and_call_equivalences(torch, oracle, mode):
    """Level 5 has n = 20 pixels for 512 channels (B singular by rank, in a deferred solve), level 3 the deflated iteration fed by
    ot_sandwich, level 2 the 128-channel level that a wide model makes "big"."""
    C, S = _wide_inputs()
    c, s = C.cpu().numpy()[0], S.cpu().numpy()[0]
    e = sc.make_engine("wide")
    e.set_transform(mode)
    for L in (5, 3, 2, 1):
        ref = {}
        for p in ("fp64", "fp32"):
            mods, cF, sF = _wide_features(oracle, p, L, c, s)
            ref[p] = mods.decode(L, O.transform_features(mode, cF, sF, 1.0).astype(cF.dtype))      # fp64 statistics in both arms
        got = e.style_transfer_level(L, C, S).cpu().numpy()[0]
        e_gpu, e32 = rel_err(got, ref["fp64"]), rel_err(ref["fp32"], ref["fp64"])
        print("wide %s level %d: gpu %.2e fp32 arm %.2e (vs fp64)" % (mode, L, e_gpu, e32))
        assert got.shape == ref["fp64"].shape and e_gpu <= 4 * e32 + 1e-4, (mode, L, e_gpu, e32)
    full = e.stylize(C, S).clone()
    e.style_prepare(S)
    assert torch.equal(e.stylize_prepared(C), full), "stylize != style_prepare + stylize_prepared"
    chain = C
    for L in (5, 4, 3, 2, 1):
        chain = e.style_transfer_level(L, chain, S)
    assert torch.equal(chain, full), "stylize != its levels chained"
    assert bool(torch.isfinite(full).all()) and e.saturation_count() == 0
    assert not torch.equal(sc.make_engine("wide").stylize(C, S), full)          # the mode took effect


def test_wide_model_deferred_solves_fall_back_under_ot_and_adain(torch, tmp_path):
    """test_hip_parity.py test_wide_model_deferred_solves_fall_back under the other transforms: with an iteration budget of 3 every
    C > 128 solve of the optimistic pass fails (under ot the content side's B^(-1/2) between the deferred outcome slots too), the call is
    repeated the synchronous way, and the saturation counter is rolled back to where the call began.  One fresh child per setting."""
    code = (
        "import sys, types, numpy as np, torch\n"
        "sys.path[:0] = [%r, %r]\n"
        "from wct_hip import WCT, model_zoo\n"
        "weights = model_zoo.synth_weights('original', 2024)\n"
        "g = torch.Generator(device='cuda').manual_seed(5)\n"
        "c, s = torch.rand((1, 3, 64, 80), device='cuda', generator=g), torch.rand((1, 3, 48, 64), device='cuda', generator=g)\n"
        "outs, sat = [], []\n"
        "for mode in ('ot', 'adain'):\n"
        "    w = WCT(types.SimpleNamespace(mode='original', alpha=1.0), weights=weights)\n"
        "    w.set_transform(mode)\n"
        "    outs += [w.style_transfer_level(k, c, s).cpu().numpy() for k in (5, 3, 2)] + [w.stylize(c, s).cpu().numpy()]\n"
        "    w.style_prepare(s); outs.append(w.stylize_prepared(c).cpu().numpy())\n"
        "    img = c\n"
        "    for k in (5, 4, 3, 2, 1): img = w.style_transfer_level(k, img, s)\n"
        "    outs.append(img.cpu().numpy())\n"
        "    sat.append(w.saturation_count())\n"
        "assert all(np.isfinite(o).all() for o in outs), 'not finite'\n"
        "assert sat == [0, 0], sat\n"
        "np.savez(sys.argv[1], *outs, sat=np.array(sat))\n" % (REPO, PKG))
    res, sat = {}, {}
    for tag, env in (("normal", {}), ("forced", {"WCT_DEBUG": "1", "WCT_NS_MAXIT": "3"})):
        out = str(tmp_path / (tag + ".npz"))
        r = subprocess.run([sys.executable, "-c", code, out], env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        with np.load(out) as z:
            res[tag] = [z["arr_%d" % i] for i in range(12)]
            sat[tag] = z["sat"].tolist()
    assert sat["forced"] == sat["normal"] == [0, 0]
    for m, mode in enumerate(("ot", "adain")):
        for i, k in enumerate((5, 3, 2)):
            a, b = res["forced"][6 * m + i], res["normal"][6 * m + i]
            err = rel_err(a, b)
            print("forced fallback %s level %d: %.2e of the output range" % (mode, k, err))
            assert a.shape == b.shape and err < 1e-5, (mode, k, err)
        # the forced child did take the other path: the Jacobi net and the deflated iteration agree to 1e-5, not to the bit (under adain
        # only the style side has matrix functions, and level 5's 512 channels are one of them)
        assert not np.array_equal(res["forced"][6 * m], res["normal"][6 * m]), mode
        for tag in ("normal", "forced"):
            full, prepared, chain = res[tag][6 * m + 3: 6 * m + 6]
            assert np.array_equal(full, prepared) and np.array_equal(full, chain), (mode, tag)
    assert not np.array_equal(res["normal"][3], res["normal"][9])          # ot and adain are different pictures


# ------------------------------------------------------------------------------------------------ 3. custom-width models
class ModelCtx(Ctx):
    def set_transform(self, mode):
        self.chk(self.L.wct_set_transform(self.ctx, _lib.TRANSFORMS[mode]))

    def get(self, key):
        v = ctypes.c_double()
        self.chk(self.L.wct_debug_get(self.ctx, key.encode(), byref(v)))
        return v.value

    def plan(self, H, W, Hs, Ws):
        return int(self.L.wct_workspace_bytes(self.ctx, H, W, Hs, Ws))

    def reserve(self, H, W, Hs, Ws):
        self.chk(self.L.wct_reserve(self.ctx, H, W, Hs, Ws))


@pytest.fixture
def mctx(torch):
    c = ModelCtx(torch)
    yield c
    c.close()


# A: the shapes of test_widths_gpu.py test_model_a_levels_and_cascade.  B: the smallest pair at which level 4 (88 channels on a 12 x 16
# map) still has full rank, so that Cp = 96 iterates; level 5 (136 channels on 6 x 8) is singular by rank.  C: level 4 (256 channels on
# 17 x 20 content and 16 x 18 style pixels) has full rank, so a full-rank C > 128 matrix goes through ot_sandwich and the deflated
# iteration; level 5 (384 channels on 8 x 10) is singular by rank
MODEL_SHAPES = {"A": (256, 256, 240, 256), "B": (96, 128, 80, 96), "C": (136, 160, 128, 144)}


def _level_reference(widths, w, mode, level, img, style, alpha, f64):
    """The fp64 (or fp32-arithmetic) restatement of a level of tests/width_models.py with (M, b) from tests/transform_oracle.py."""
    cF, sF = wm.encode(widths, w, level, img, f64), wm.encode(widths, w, level, style, f64)
    sm, ssq = wm.raw_moments(cF)
    mu_s, cov_s = O.mean_cov(sF.shape[1] * sF.shape[2], *wm.raw_moments(sF))
    M, b = O.solve(mode, cF.shape[1] * cF.shape[2], sm, ssq, O.stats(O.sym_pow(cov_s, 0.5), mu_s), alpha)
    return wm.decode_affine(widths, w, level, cF, M, b, f64)


@pytest.mark.parametrize("mode", ["ot", "adain"])
@pytest.mark.parametrize("model", sorted(wm.MODELS))
def test_custom_width_model_levels_against_fp64(mctx, model, mode):
    """A: Cp = 96 at level 4 (68) and the ragged Cp = 128 at level 5 (100); B: Cp = 96 at level 4 (88), deflated at 136; C: 256 and 384.

    Open: [B-ot] has failed once at level 3 (C = 56: e_gpu 0.75 against e32 3.5e-6; levels 5 and 4 of the same run were right) late in a
    long test process.  It has not recurred and its cause is not known; the gate stays as it is."""
    widths = wm.MODELS[model]
    w = wm.synth(widths, seed=ord(model))
    mctx.load(widths, w)
    mctx.set_transform(mode)
    H, W, Hs, Ws = MODEL_SHAPES[model]
    rng = np.random.default_rng(5)
    c, s = wm.smooth_image(rng, H, W), wm.smooth_image(rng, Hs, Ws)
    alpha = 0.6
    img = c
    for level in (5, 4, 3, 2, 1):
        r64 = _level_reference(widths, w, mode, level, img, s, alpha, True)
        r32 = _level_reference(widths, w, mode, level, img, s, alpha, False)
        got = mctx.style_transfer_level(level, img, s, alpha)
        e_gpu, e32 = rel_err(got, r64), rel_err(r32, r64)
        print("widths %s %s level %d (C = %d): gpu %.2e fp32 arm %.2e (vs fp64)" % (model, mode, level, wm.feature_channels(widths, level), e_gpu, e32))
        assert got.shape == r64.shape and e_gpu <= 4 * e32 + 1e-4, (model, mode, level, e_gpu, e32)
        img = r64.astype(np.float32)           # level-isolated: fp64's output feeds the next level of both sides
    chain = c
    for level in (5, 4, 3, 2, 1):
        chain = mctx.style_transfer_level(level, chain, s, alpha)
    full = mctx.stylize(c, s, alpha)
    assert np.array_equal(full, chain)
    assert np.array_equal(mctx.stylize(c, s, alpha, prepared=True), full)
    assert mctx.saturation() == 0
    mctx.set_transform("wct")
    assert not np.array_equal(mctx.stylize(c, s, alpha), full)


def test_reserve_is_exact_under_ot_at_384_channels(mctx):
    """wct_reserve sizes the ot buffer from the widest loaded level: model C's 384, not the shipped 128."""
    widths = wm.MODELS["C"]
    mctx.load(widths, wm.synth(widths, seed=ord("C")))
    shape = MODEL_SHAPES["C"]
    rng = np.random.default_rng(6)
    c, s = wm.smooth_image(rng, *shape[:2]), wm.smooth_image(rng, *shape[2:])
    plan_wct = mctx.plan(*shape)
    mctx.set_transform("ot")
    plan_ot = mctx.plan(*shape)
    assert plan_ot == plan_wct + ((2 * 384 * 384 + 384) * 8 + 255) // 256 * 256          # ot_workspace_bytes(384), as ensure() rounds
    mctx.reserve(*shape)
    assert mctx.get("ws_bytes") == plan_ot
    allocs = mctx.get("ws_allocs")
    mctx.stylize(c, s, 0.7)
    mctx.style_transfer_level(5, c, s, 1.0)
    mctx.style_transfer_level(3, c, s, 1.0)
    assert mctx.get("ws_allocs") == allocs, "the reserve was not exact under ot"
    mctx.set_transform("adain")
    assert mctx.plan(*shape) == plan_wct
    mctx.set_transform("wct")
    assert mctx.plan(*shape) == plan_wct


# ------------------------------------------------------------------------------------------------ 4. wct_stylize_interp under the modes
# (wct_synthesize, wct_stylize_color and wct_stylize_smooth: the composition tests of test_synthesis_gpu.py, test_color_gpu.py and
# test_smooth_gpu.py are parametrised over the transform.)
# include/wct_hip.h specifies the blend of the K slots to the bit: one launch, fixed k order, lambda = (1, 0, ..) gives style 0's
# statistics bit for bit.  With weights that are powers of two every product is exact, so numpy's sum in the same order is the same bits.


def _engine(mode):
    e = sc.make_engine("16x")
    e.set_transform(mode)
    return e


@pytest.mark.parametrize("mode", ["wct", "ot", "adain"])
def test_interp_of_one_style_is_stylize(torch, mode):
    H, W, Hs, Ws = sc.SIZES["small"]
    c, s = sc.image(71, H, W), sc.image(72, Hs, Ws)
    e = _engine(mode)
    ref = e.stylize(c, s, alpha=0.8).clone()
    for weights in ([1.0], [3.0]):
        got = e.stylize_interp(c, [s], weights, alpha=0.8)
        assert got.shape == ref.shape and torch.equal(got, ref), (mode, weights, rel_err(got.cpu().numpy(), ref.cpu().numpy()))
    if mode != "wct":
        assert not torch.equal(_engine("wct").stylize(c, s, alpha=0.8), ref)
    assert e.saturation_count() == 0


@pytest.mark.parametrize("mode", ["ot", "adain"])
def test_interp_of_several_styles_targets_the_blended_slot(torch, mode):
    """under ot / adain the target of wct_stylize_interp is the slot SUM_k l_k (S_k, mu_k), not the linear mix of the K
    results.  The blend is made here in numpy fp64 from the exported slots and imported."""
    H, W = sc.SIZES["small"][:2]
    c = sc.image(73, H, W)
    styles = sc.styles(74, 3, "small")
    weights = [2.0, 1.0, 1.0]                    # l = 1/2, 1/4, 1/4: powers of two
    e = _engine(mode)
    ref = e.stylize_interp(c, styles, weights, alpha=0.8).clone()
    slots = []
    for s in styles:
        e.style_prepare(s)
        slots.append({L: e.style_export(L).cpu().numpy() for L in (5, 4, 3, 2, 1)})
    for L in (5, 4, 3, 2, 1):
        blend = 0.5 * slots[0][L] + 0.25 * slots[1][L] + 0.25 * slots[2][L]
        e.style_import(L, torch.from_numpy(blend).cuda())
    got = e.stylize_prepared(c, alpha=0.8)
    assert got.shape == ref.shape and torch.equal(got, ref), (mode, rel_err(got.cpu().numpy(), ref.cpu().numpy()))
    mix = sum(l * e.stylize(c, s, alpha=0.8) for l, s in zip((0.5, 0.25, 0.25), styles))
    assert rel_err(mix.cpu().numpy(), ref.cpu().numpy()) > 1e-4          # ... and it is not the linear mix of the three results
    assert e.saturation_count() == 0
