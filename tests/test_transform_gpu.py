"""The choice of feature transform on the device (include/wct_hip_transform.h): wct_transform_solve against the numpy fp64 reference
(tests/transform_oracle.py) on raw moments and on real features, the cascade under ot / adain against an fp64 arm, what must not move
(wct mode, bit for bit), the context's state under ot, the split and sharded level, the refusals and the command line.

Gates.  The solver's own (tests/test_hip_parity.py): 1e-8 where cond(B) <= 1e6 and for singular-by-rank matrices (the Jacobi net),
1e-6 ("~10 cond eps") up to cond(B) = 1e10; cond(B) is measured on B's live block by the reference.  What is compared is the action on
the content's support, M R with R = cov_c^(1/2), and the image of the content mean M mu_c + b: where B is singular T is unique only
there (the header's null-space argument).  The cascade: e_gpu <= 4 e32 + 1e-4 against the fp64 arm (tests/test_widths_gpu.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import state_cases as sc
from tests import transform_oracle as O
from tests.transform_cases import make_case as _case
from tests.conftest import PKG, REPO, rel_err
from wct_hip import lib as _lib

pytestmark = pytest.mark.gpu

GATE_WELL, GATE_ILL = 1e-8, 1e-6          # test_hip_parity.py:115 / :248-249


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def eng(torch):
    return sc.make_engine("16x")


def t64(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float64)).cuda()


def npy(x):
    return x.detach().cpu().numpy()


def cond_live(B):
    lam = np.linalg.eigvalsh(O.sym(B))
    keep = lam[lam > O.REL * lam.max()]
    return float(keep.max() / keep.min()), int(keep.size)


def gate_for(cond, full_rank):
    if not full_rank:
        return GATE_WELL              # singular by rank: the Jacobi net, which drops the null directions exactly
    assert cond <= 1e10, cond
    return GATE_WELL if cond <= 1e6 else GATE_ILL


def check_solve(torch, eng, mode, n, s, ss, st, alpha, what, want_ns=None):
    """transform_solve against the oracle on the support; returns info[0]."""
    M, b, info = eng.transform_solve(mode, n, t64(torch, s), t64(torch, ss), t64(torch, st), alpha=alpha, want_info=True)
    M, b = npy(M), npy(b)
    assert np.isfinite(M).all() and np.isfinite(b).all(), what
    Mr, br = O.solve(mode, n, s, ss, st, alpha)
    mu_c, cov_c = O.mean_cov(n, s, ss)
    S, _ = O.split_stats(st)
    cond, rank = cond_live(O.ot_B(cov_c, S)) if mode == "ot" else (1.0, 0)
    dB = np.diag(O.ot_B(cov_c, S))
    live = int((dB > 1e-13 * dB.max()).sum()) if mode == "ot" else 0      # the solver's dead-channel identity block: axis-aligned zeros of B
    full = rank == live
    gate = gate_for(cond, full) if mode == "ot" else GATE_WELL
    R = O.sym_pow(cov_c, 0.5)
    e_map, e_mean = rel_err(M @ R, Mr @ R), rel_err(M @ mu_c + b, Mr @ mu_c + br)
    print("transform_solve %s %s alpha %.1f: cond(B) %.1e rank %d of %d live, info %s, M R %.2e, M mu + b %.2e (gate %.0e)"
          % (mode, what, alpha, cond, rank, live, tuple(info), e_map, e_mean, gate))
    assert e_map < gate and e_mean < gate, (what, mode, alpha, e_map, e_mean, gate)
    assert info[1] == 0
    if mode == "adain":
        assert info[0] == 0
    if want_ns is None:
        want_ns = mode == "ot" and full and cond <= 1e9
    if want_ns:
        assert 0 < info[0] < 100, "%s: the matrix-core path did not handle B (info %d, cond %.1e)" % (what, info[0], cond)
    return info[0]


# ------------------------------------------------------------------------------------------------ 1. raw moments
DEAD29 = tuple(range(3, 128, 4))[:29]
RAW_CASES = {
    "C24": dict(C=24, lo_c=1e-2, lo_s=1e-2),
    "C32": dict(C=32, lo_c=1e-2, lo_s=1e-3),
    "C64": dict(C=64, lo_c=1e-3, lo_s=1e-2),
    "C128": dict(C=128, lo_c=1e-2, lo_s=1e-2),
    "C128_dead29": dict(C=128, lo_c=1e-4, lo_s=1e-4, dead_c=DEAD29, dead_s=DEAD29),
    "C32_cond1e9": dict(C=32, lo_c=3e-6, lo_s=1e-5),
    "C64_content_dead1": dict(C=64, lo_c=1e-2, lo_s=1e-2, dead_c=(17,)),
    "C128_content_rank76": dict(C=128, lo_c=1e-2, lo_s=1e-2, n=77, rank_c=76),
    "C64_style_rank40": dict(C=64, lo_c=1e-2, lo_s=1e-2, rank_s=40),
    "C256": dict(C=256, lo_c=3e-4, lo_s=3e-4),
    "C512": dict(C=512, lo_c=3e-4, lo_s=3e-4),
}


@pytest.mark.parametrize("name", list(RAW_CASES))
def test_ot_solve_against_the_oracle_on_raw_moments(torch, eng, name):
    n, s, ss, st = _case(len(name) * 131 + RAW_CASES[name]["C"], **RAW_CASES[name])
    for alpha in (1.0, 0.6):
        check_solve(torch, eng, "ot", n, s, ss, st, alpha, name)
    assert eng.transform_mode == "wct"          # mode-explicit: the context's mode is left alone


# ------------------------------------------------------------------------------------------------ 2. real features
def test_ot_solve_on_real_features(torch, eng, golden):
    g = golden("g4_cascade.npz")
    style = t64(torch, g["a.style"]).float()[None]
    eng.style_prepare(style)
    img = g["a.content"]
    for L in (5, 4, 3, 2, 1):
        f = eng.encode(L, t64(torch, img).float()[None], layout="nhwc")
        n, s, ss = eng.moments(f)
        st = eng.style_export(L)
        info = check_solve(torch, eng, "ot", n, npy(s), npy(ss), npy(st), 1.0, "g4 a level %d" % L, want_ns=L <= 4)
        check_solve(torch, eng, "ot", n, npy(s), npy(ss), npy(st), 0.6, "g4 a level %d" % L, want_ns=L <= 4)
        print("real features level %d: n %d, info[0] %d" % (L, n, info))
        img = g["a.L%d.out" % L]


# ------------------------------------------------------------------------------------------------ 3. adain
@pytest.mark.parametrize("C,dead", [(24, ()), (64, (1, 9, 30, 31, 63)), (128, DEAD29), (512, (0, 511))])
def test_adain_solve_against_the_oracle(torch, eng, C, dead):
    n, s, ss, st = _case(C + 1, C, 1e-3, 1e-2, dead_c=dead, dead_s=dead)
    for alpha in (1.0, 0.6):
        M, b, info = eng.transform_solve("adain", n, t64(torch, s), t64(torch, ss), t64(torch, st), alpha=alpha, want_info=True)
        Mr, br = O.solve("adain", n, s, ss, st, alpha)
        e_m, e_b = rel_err(npy(M), Mr), rel_err(npy(b), br)
        print("adain C=%d alpha %.1f: M %.2e b %.2e" % (C, alpha, e_m, e_b))
        assert e_m < GATE_WELL and e_b < GATE_WELL and tuple(info) == (0, 0)
        assert np.count_nonzero(npy(M) - np.diag(np.diag(npy(M)))) == 0
        if alpha == 1.0 and dead:
            assert np.array_equal(np.diag(npy(M))[list(dead)], np.ones(len(dead)))      # sqrt(eps / eps)


def test_wct_mode_of_transform_solve_is_wct_solve(torch, eng):
    """Mode 0 of the mode-explicit entry: the (M, b) wct_solve makes of the same statistics.  The slot handed in is the reference's
    cov_s^(1/2), which differs from the library's own in the last bits: compared through the solver's gate."""
    C = 64
    nc, sc_, ssc = sc.raw_moments(5, C, 40000, 1e-3)
    ns, ss_, sss = sc.raw_moments(6, C, 30000, 1e-2)
    M0, b0, info0 = eng.solve(nc, sc_, ssc, ns, ss_, sss, alpha=0.7, want_info=True)
    mu_s, cov_s = O.mean_cov(ns, npy(ss_), npy(sss))
    M1, b1, info1 = eng.transform_solve("wct", nc, sc_, ssc, t64(torch, O.stats(O.sym_pow(cov_s, 0.5), mu_s)), alpha=0.7, want_info=True)
    assert rel_err(npy(M1), npy(M0)) < GATE_WELL and rel_err(npy(b1), npy(b0)) < GATE_WELL
    assert info1[0] == info0[0] and info1[1] == 0


# ------------------------------------------------------------------------------------------------ 4. the cascade
@pytest.mark.parametrize("mode", ["ot", "adain"])
def test_level_isolated_cascade_against_the_fp64_arm(torch, oracle, weights16x, golden, mode):
    g = golden("g4_cascade.npz")
    c, s = g["b.content"], g["b.style"]
    alpha = 0.6
    arms = {p: oracle.Modules("16x", weights16x, precision=p) for p in ("fp64", "fp32")}

    def level(mods, L, img):
        f64 = mods.precision == "fp64"
        dt = np.float64 if f64 else np.float32
        cF, sF = mods.encode(L, np.asarray(img, dt)), mods.encode(L, np.asarray(s, dt))
        return mods.decode(L, O.transform_features(mode, cF, sF, alpha).astype(dt))      # fp64 statistics in both arms, like the reference

    e = sc.make_engine("16x")
    e.set_transform(mode)
    assert e.transform_mode == mode
    S = t64(torch, s).float()[None]
    img = c
    for L in (5, 4, 3, 2, 1):
        r64, r32 = level(arms["fp64"], L, img), level(arms["fp32"], L, img)
        got = npy(e.style_transfer_level(L, t64(torch, img).float()[None], S, alpha))[0]
        e_gpu, e32 = rel_err(got, r64), rel_err(r32, r64)
        print("cascade %s level %d: gpu %.2e fp32 arm %.2e (vs fp64)" % (mode, L, e_gpu, e32))
        assert e_gpu <= 4 * e32 + 1e-4, (mode, L, e_gpu, e32)
        img = r64.astype(np.float32)           # level-isolated: fp64's output feeds the next level of both sides
    C = t64(torch, c).float()[None]
    chain = C
    for L in (5, 4, 3, 2, 1):
        chain = e.style_transfer_level(L, chain, S, alpha)
    full = e.stylize(C, S, alpha=alpha).clone()
    assert torch.equal(full, chain)
    e.style_prepare(S)
    assert torch.equal(e.stylize_prepared(C, alpha=alpha), full)
    assert e.saturation_count() == 0
    wct = sc.make_engine("16x").stylize(C, S, alpha=alpha)
    assert not torch.equal(wct, full)


# ------------------------------------------------------------------------------------------------ 5. nothing moved
def _wct_outputs(e):
    H, W, Hs, Ws = sc.SIZES["small"]
    c, s = sc.image(31, H, W), sc.image(32, Hs, Ws)
    out = {"stylize": e.stylize(c, s, alpha=0.8).clone()}
    out["M"], out["b"] = e.solve(*sc.raw_moments(33, 64, 50000, 1e-3), *sc.raw_moments(34, 64, 20000, 1e-2), alpha=0.6)
    for L in (5, 3, 1):
        out["level%d" % L] = e.style_transfer_level(L, c, s, alpha=0.9)
    return out


def test_wct_mode_is_untouched_by_a_detour_through_the_other_modes(torch):
    H, W, Hs, Ws = sc.SIZES["small"]
    fresh = sc.make_engine("16x")
    want = _wct_outputs(fresh)
    torch.cuda.synchronize()
    e = sc.make_engine("16x")
    e.reserve(H, W, Hs, Ws)
    plan_wct = sc.workspace_bytes(e, H, W, Hs, Ws)
    assert e.debug_get("ws_bytes") == plan_wct
    assert plan_wct == sc.workspace_bytes(fresh, H, W, Hs, Ws)
    c, s = sc.image(41, H, W), sc.image(42, Hs, Ws)
    e.stylize(c, s)
    e.set_transform("ot")
    plan_ot = sc.workspace_bytes(e, H, W, Hs, Ws)
    assert plan_ot == plan_wct + ((2 * 128 * 128 + 128) * 8 + 255) // 256 * 256      # one buffer more, for the widest level
    e.reserve(H, W, Hs, Ws)
    assert e.debug_get("ws_bytes") == plan_ot
    allocs = e.debug_get("ws_allocs")
    e.stylize(c, s, alpha=0.7)
    e.style_transfer_level(3, c, s)
    assert e.debug_get("ws_allocs") == allocs                                        # the reserve was exact under ot
    e.set_transform("adain")
    assert sc.workspace_bytes(e, H, W, Hs, Ws) == plan_wct
    e.stylize(c, s)
    e.solve(*sc.raw_moments(43, 64, 50000, 1e-3), *sc.raw_moments(44, 64, 20000, 1e-2), alpha=0.5)
    e.set_transform("wct")
    assert e.transform_mode == "wct" and sc.workspace_bytes(e, H, W, Hs, Ws) == plan_wct
    allocs = e.debug_get("ws_allocs")
    e.reserve(H, W, Hs, Ws)
    assert e.debug_get("ws_allocs") == allocs                                        # nothing the wct-mode reserve had not already
    got = _wct_outputs(e)
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(got[k], want[k]), k


# ------------------------------------------------------------------------------------------------ 6. state under ot
STATE_CASES = ("stylize/small", "prepared/small", "solve/small", "level/small", "transform/small", "split_level/small", "interp/small", "synthesize/small")


def _ot_engine(kind="16x"):
    e = sc.make_engine(kind)
    e.set_transform("ot")
    return e


def _equal(torch, got, want, what):
    torch.cuda.synchronize()
    assert sorted(got) == sorted(want)
    for k in want:
        assert torch.equal(got[k], want[k]), "%s: %s differs" % (what, k)


def _state_under_ot(torch, kind):
    assert all(sc.CASES[name].wide for name in STATE_CASES)
    want = {name: sc.run(_ot_engine(kind), name) for name in STATE_CASES}
    torch.cuda.synchronize()
    differs = sc.run(sc.make_engine(kind), "stylize/small")
    assert not torch.equal(differs["alpha1"], want["stylize/small"]["alpha1"])          # the cases do run under ot
    used = _ot_engine(kind)
    used.stylize(sc.image(7, 72, 88), sc.image(8, 66, 70))
    used.transform_solve("adain", *sc.raw_moments(9, 32, 5000, 1e-2), torch.rand(32 * 33, dtype=torch.float64))
    for name in reversed(STATE_CASES):
        _equal(torch, sc.run(used, name), want[name], "used engine, " + name)
    for name in STATE_CASES:                      # second call of every size: nothing is allocated
        allocs = used.debug_get("ws_allocs")
        _equal(torch, sc.run(used, name), want[name], "second call, " + name)
        assert used.debug_get("ws_allocs") == allocs, name
    poisoned = _ot_engine(kind)
    poisoned.debug_set("poison", 0xA5)
    for name in STATE_CASES:
        _equal(torch, sc.run(poisoned, name), want[name], "poison 0xA5, " + name)
        poisoned.debug_set("poison", 0xA5)
        _equal(torch, sc.run(poisoned, name), want[name], "poison 0xA5 again, " + name)
    poisoned.debug_set("poison", -1)
    assert used.saturation_count() == 0 and poisoned.saturation_count() == 0


def test_state_under_ot(torch):
    _state_under_ot(torch, "16x")


@pytest.fixture(scope="module")
def wide_state(torch):
    """(an un-pruned ot engine with a past, one whose scratch is poisoned between calls), shared by the cases below."""
    used, poisoned = _ot_engine("wide"), _ot_engine("wide")
    used.stylize(sc.image(7, 72, 88), sc.image(8, 66, 70))
    used.transform_solve("adain", *sc.raw_moments(9, 32, 5000, 1e-2), torch.rand(32 * 33, dtype=torch.float64))
    return used, poisoned


@pytest.mark.parametrize("name", STATE_CASES)
def test_state_under_ot_wide_model(torch, wide_state, name):
    """The same legs on the un-pruned engine, one case at a time: the C > 128 solves of a call are deferred to its end (ok_log), and
    under ot the content side runs ot_sandwich -> B^(-1/2) -> ot_assemble between the deferred outcome slots."""
    used, poisoned = wide_state
    want = sc.run(_ot_engine("wide"), name)
    torch.cuda.synchronize()
    if name == "stylize/small":
        assert not torch.equal(sc.run(sc.make_engine("wide"), name)["alpha1"], want["alpha1"])          # the cases do run under ot
    _equal(torch, sc.run(used, name), want, "used engine, " + name)
    allocs = used.debug_get("ws_allocs")
    _equal(torch, sc.run(used, name), want, "second call, " + name)
    assert used.debug_get("ws_allocs") == allocs, name                      # second call of a size: nothing is allocated
    for leg in ("poison 0xA5, ", "poison 0xA5 again, "):
        poisoned.debug_set("poison", 0xA5)
        _equal(torch, sc.run(poisoned, name), want, leg + name)
    poisoned.debug_set("poison", -1)
    assert used.saturation_count() == 0 and poisoned.saturation_count() == 0


def test_graph_capture_under_ot(torch):
    e = _ot_engine()
    c1, c2, s = sc.image(1, 112, 144), sc.image(2, 112, 144), sc.image(3, 96, 128)
    e.style_prepare(s)
    want1, want2 = e.stylize_prepared(c1, alpha=0.6).clone(), e.stylize_prepared(c2, alpha=0.6).clone()
    c = c1.clone()
    out = torch.empty((3, 112, 144), device="cuda")
    e.stylize_prepared(c, alpha=0.6, out=out)      # warm-up on the buffers the graph will use
    torch.cuda.synchronize()
    allocs = e.debug_get("ws_allocs")
    cap = torch.cuda.Stream()
    with torch.cuda.stream(cap):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=cap):
            e.stylize_prepared(c, alpha=0.6, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(1, 3, 112, 144), want1), "replay 1 differs"
    c.copy_(c2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(1, 3, 112, 144), want2), "replay 2 differs"
    assert e.debug_get("ws_allocs") == allocs


# ------------------------------------------------------------------------------------------------ 7. split and sharded level
def test_split_level_under_ot(torch):
    e = _ot_engine()
    H, W = 144, 176
    c, s = sc.image(51, H, W), sc.image(52, 120, 136)
    e.style_prepare(s, levels=(5, 2))
    for L in (5, 2):
        h, w, sm, ssq = e.content_encode(L, c)
        M, b = e.content_solve(L, float(h * w), sm, ssq, alpha=0.8)
        got = e.content_decode(L, M, b, H, W)
        want = e.style_transfer_level(L, c, s, alpha=0.8)
        err = float((got - want).abs().max())
        print("split level %d under ot: max |diff| %.2e" % (L, err))
        assert got.shape == want.shape and err < 2e-5, (L, err)
        # the context's mode and the explicit one: the same launches.  wct_content_solve takes alpha as a float, wct_transform_solve as
        # a double: the same number for both is the float's value
        Mo, bo = e.transform_solve("ot", float(h * w), sm, ssq, e.style_export(L), alpha=float(np.float32(0.8)))
        assert torch.equal(Mo, M) and torch.equal(bo, b), (L, float((Mo - M).abs().max()), float((bo - b).abs().max()))


def test_level_sharded_single_rank_equals_the_split_sequence_under_ot():
    """wct_level_sharded on a one-rank communicator (RCCL refuses two ranks on one device) under ot: the header's contract -- the same
    arithmetic in the same order as wct_content_encode / all-reduce / wct_content_solve / wct_content_decode, bit for bit.  A fresh
    process: torch.distributed is initialised once per process."""
    code = r"""
import os, sys
sys.path[:0] = [%r, %r]
import torch, torch.distributed as dist
os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT='%d', RANK='0', WORLD_SIZE='1')
torch.cuda.set_device(0)
dist.init_process_group('nccl', device_id=torch.device('cuda', 0))
from tests import state_cases as sc
H, W = 144, 176
c, s = sc.image(51, H, W)[0], sc.image(52, 120, 136)
ref = sc.make_engine('16x'); ref.set_transform('ot'); ref.style_prepare(s, levels=(5, 2))
eng = sc.make_engine('16x'); eng.set_transform('ot'); eng.comm_init(dist); eng.style_prepare(s, levels=(5, 2))
wct = sc.make_engine('16x'); wct.comm_init(dist); wct.style_prepare(s, levels=(5, 2))
for L in (5, 2):
    h, w, sm, ssq = ref.content_encode(L, c)
    M, b = ref.content_solve(L, float(h * w), sm, ssq, alpha=0.8)
    want = ref.content_decode(L, M, b, H, W)
    got = eng.level_sharded(L, c, 0, -1, float(h * w), 0.8)
    eng.sync()
    assert torch.equal(got, want), (L, float((got - want).abs().max()))
    assert not torch.equal(wct.level_sharded(L, c, 0, -1, float(h * w), 0.8), got), L
dist.destroy_process_group()
print('OK')
""" % (REPO, PKG, 29500 + os.getpid() % 2000)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_output_untouched(torch):
    e = sc.make_engine("16x")
    H, W = 70, 90
    c, s = sc.image(1, H, W), sc.image(2, 64, 80)
    out = torch.full((3, H, W), 7.25, device="cuda")
    e.set_transform("ot")
    with pytest.raises(ValueError, match="stylize_regions"):
        e.stylize_regions(c, [s, s], sc.label_map(H, W, 2), out=out)
    with pytest.raises(ValueError, match="stylize_blend"):
        e.stylize_blend(c, [s, s], sc.weight_maps(4, 2, H, W), out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.25).all())
    L, ctx = e._lib, e._ctx
    assert L.wct_set_numpy_variant(ctx, 1) == _lib.WCT_ERR_INVALID and b"wct transform only" in L.wct_last_error(ctx)
    assert L.wct_set_numpy_variant(ctx, 0) == _lib.WCT_OK
    e.set_transform("wct")
    assert L.wct_set_numpy_variant(ctx, 1) == _lib.WCT_OK
    for mode in (_lib.TRANSFORM_OT, _lib.TRANSFORM_ADAIN):
        assert L.wct_set_transform(ctx, mode) == _lib.WCT_ERR_INVALID and b"numpy" in L.wct_last_error(ctx)
    assert e.transform_mode == "wct"
    assert L.wct_set_numpy_variant(ctx, 0) == _lib.WCT_OK
    for mode in (-1, 3):
        assert L.wct_set_transform(ctx, mode) == _lib.WCT_ERR_INVALID
    with pytest.raises(ValueError):
        e.set_transform("monge")
    assert e.transform_mode == "wct"
    # wct_transform_solve: a bad mode, C odd, C > 512, n < 2, a NULL pointer -- M and b stay as they were
    C = 32
    n, sm, ssq = sc.raw_moments(3, C, 5000, 1e-2)
    st = torch.rand(C * C + C, dtype=torch.float64, device="cuda")
    big = torch.zeros(514 * 514 + 514, dtype=torch.float64, device="cuda")
    M, b = torch.full((514 * 514,), 7.25, dtype=torch.float64, device="cuda"), torch.full((514,), 7.25, dtype=torch.float64, device="cuda")
    e._stream()
    call = lambda mode, C_, n_, s_=sm, q_=ssq, st_=st: L.wct_transform_solve(ctx, mode, C_, float(n_), s_.data_ptr() if s_ is not None else None, q_.data_ptr(),
                                                                               st_.data_ptr(), 1.0, M.data_ptr(), b.data_ptr(), None)
    assert call(3, C, n) == _lib.WCT_ERR_INVALID and call(-1, C, n) == _lib.WCT_ERR_INVALID
    for mode in (0, 1, 2):
        assert call(mode, 31, n, big, big, big) == _lib.WCT_ERR_INVALID
        assert call(mode, 514, n, big, big, big) == _lib.WCT_ERR_INVALID
        assert call(mode, 0, n) == _lib.WCT_ERR_INVALID
        assert call(mode, C, 1.0) == _lib.WCT_ERR_INVALID
        assert call(mode, C, n, None) == _lib.WCT_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((M == 7.25).all()) and bool((b == 7.25).all())
    for mode in (0, 1, 2):
        assert call(mode, C, n) == _lib.WCT_OK
    torch.cuda.synchronize()
    assert bool(torch.isfinite(M[:C * C]).all()) and bool((M[C * C:] == 7.25).all()) and bool((b[C:] == 7.25).all())


# ------------------------------------------------------------------------------------------------ 9. the command line
def test_cli_transform_ot_serial_and_pipelined(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from wct_hip import cli
    rng = np.random.default_rng(1)
    c, s = tmp_path / "content", tmp_path / "style"
    c.mkdir(); s.mkdir()
    Image.fromarray(rng.integers(0, 256, size=(64, 80, 3), dtype=np.uint8)).save(c / "c1.png")
    Image.fromarray(rng.integers(0, 256, size=(56, 40, 3), dtype=np.uint8)).save(s / "st.png")
    data = {}
    for tag, extra in (("ot0", ["--transform", "ot", "--pipeline", "0"]), ("ot2", ["--transform", "ot", "--pipeline", "2"]), ("wct", ["--pipeline", "0"])):
        o = tmp_path / tag
        assert cli.main(["--mode", "16x", "--contentPath", str(c), "--stylePath", str(s), "--outf", str(o), "--log_mark", "T", "--alpha", "0.6"] + extra) == 0
        mark = "" if tag == "wct" else "_transform=ot"
        path = o / ("T_mode=16x_alpha=0.6%s_c1+st.jpg" % mark)
        assert path.exists(), sorted(os.listdir(o))
        data[tag] = path.read_bytes()
    assert data["ot0"] == data["ot2"]
    assert data["ot0"] != data["wct"]
