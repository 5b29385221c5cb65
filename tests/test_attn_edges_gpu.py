"""The attention statistics at every width and at the edges of their launcher (tests/attn_cases.py), on the MI355X against the numpy fp64
reference (tests/attn_oracle.py):

  E1  wct_attn_stats at all 128 widths (16 bands of 8, non-monotonic), Nq = 65, Nk = 33, every tau of the first test
  E2  the channel tail decides: four planted channels carry the scores -- the last 4, the upper half of the last complete 8-channel
      group, the first 4 of the last 128-channel chunk -- at 30 widths that cover every (nct, nks, half-live group) the plan can produce
  E3  rolling the columns of V rolls the columns of (mean, var), bit for bit, across value slabs
  E4  Nk and Nq at the tile borders; the header's tau = 0 statement
  E5  the running maximum: key orders in which every tile raises it, none does, and all weights but one round to 0 in f16
  E6  the default launch split (no debug key): two launches
  E7  wct_attn_project and wct_attn_apply at every width; the whitened projection either side of attn_whiten_kernel's two forms
  E8  wct_attn_level at level 3 with 256 and with 132 channels

The gate of wct_attn_stats is that of tests/test_attn_gpu.py, imported: 4 e32 + FLOOR_MEAN / FLOOR_VAR, e32 the plain-fp32 numpy arm's
error on the very case.  Every wct_attn_stats call runs on a profiled engine with "prof_forms" on and its reported launch form is held
against attn_cases.plan (gpu_stats below).  The engine's scratch is poisoned with 0xFF.  tests/test_attn_cpu.py shows on the CPU that the
planted cases separate a wrong kernel from a right one.  Every test prints "edges E<n> ..." lines with its figures.

Measured on the MI355X: see DESIGN.md, "Attention statistics", "Off the first test's shapes".

The module imports without a GPU."""
import numpy as np
import pytest

from tests import attn_cases as AC
from tests import attn_oracle as A
from tests import state_cases as sc
from tests import sweep_cases
from tests.test_attn_gpu import FLOOR_MEAN, FLOOR_VAR, LEVEL_FLOOR, cu
from wct_hip import lib as _lib

pytestmark = pytest.mark.gpu

PROJECT_GATE = 1e-6         # tests/test_attn_gpu.py test_project_against_fp64
BANDS = list(range(sweep_cases.N_BANDS))


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "-m gpu tests need the MI355X"
    return t


def reporting_engine():
    eng = sc.make_engine("16x")
    eng.debug_set("poison", 0xFF)
    eng.profile(True)
    eng.debug_set("prof_forms", 1)
    return eng


@pytest.fixture(scope="module")
def wct(torch):
    """One engine for the module: a buffer grown for a wide call is reused by a narrow one."""
    return reporting_engine()


def gpu_stats(torch, eng, q, k, v, tau):
    """(mean, var) on the host; the launch form the library reports is the plan's."""
    eng.profile_reset()
    m, var = eng.attn_stats(*(cu(torch, np.array(a)) for a in (q, k, v)), tau)          # copies: the shared cases are read-only
    torch.cuda.synchronize()
    names = [e["name"] for e in eng.profile_read()]
    want = AC.profile_name(q.shape[0], k.shape[0], q.shape[1])
    assert names == [want], (names, want)
    return m.cpu().numpy(), var.cpu().numpy()


def errors(m, var, ref):
    (m64, v64), _, vmax = ref
    return float(np.abs(m - m64).max()) / vmax, float(np.abs(var - v64).max()) / vmax ** 2


def held(m, var, ref, what, failures=None):
    """The gate of tests/test_attn_gpu.py on one case; prints the figures.  With `failures` a miss is collected instead of raised."""
    _, (e32m, e32v), _ = ref
    em, ev = errors(m, var, ref)
    gm, gv = 4 * e32m + FLOOR_MEAN, 4 * e32v + FLOOR_VAR
    print("edges %s: mean %.3e (fp32 arm %.3e, gate %.3e) var %.3e (fp32 arm %.3e, gate %.3e)" % (what, em, e32m, gm, ev, e32v, gv))
    bad = []
    if not (np.isfinite(m).all() and np.isfinite(var).all() and (var >= 0).all()):
        bad.append("%s: a non-finite output or a negative variance" % what)
    if not em <= gm:
        bad.append("%s: mean %.3e against 4 x %.3e + %.1e" % (what, em, e32m, FLOOR_MEAN))
    if not ev <= gv:
        bad.append("%s: var %.3e against 4 x %.3e + %.1e" % (what, ev, e32v, FLOOR_VAR))
    if failures is None:
        assert not bad, "; ".join(bad)
    else:
        failures += bad
    return em, ev, e32m, e32v


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------- E1. every width
@pytest.mark.parametrize("b", BANDS)
def test_e1_every_width(torch, wct, b):
    """The 8 widths of a band x TAUS at Nq = 65, Nk = 33: a full and a ragged tile on each axis.  Failures are collected and listed
    together, so that structure by width shows in one run.  Measured on the MI355X: per band the largest mean error is 5.8e-7 .. 1.2e-6 and
    the largest var error 3.8e-7 .. 6.9e-7, all at tau = 32, where the fp32 arm is at 2.2e-7 .. 1.3e-6 (the table is in DESIGN.md); the case
    nearest its gate is at 0.78 of it (C = 4, tau = 32).  No structure by width."""
    failures, worst = [], [0.0, 0.0, 0.0, 0.0]
    for C in sweep_cases.BANDS[b]:
        q, k, v = AC.edge_inputs(C)
        for tau in AC.TAUS:
            ref = AC.reference(q, k, v, tau)
            m, var = gpu_stats(torch, wct, q, k, v, tau)
            em, ev, e32m, e32v = held(m, var, ref, "E1 band %d C=%d tau=%g" % (b, C, tau), failures)
            if em > worst[0]:
                worst[:2] = [em, e32m]
            if ev > worst[2]:
                worst[2:] = [ev, e32v]
    print("edges E1 band %d worst: mean %.3e (fp32 arm %.3e) var %.3e (fp32 arm %.3e)" % (b, *worst))
    assert not failures, "%d of %d cases: %s" % (len(failures), 8 * len(AC.TAUS), "; ".join(failures))
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- E2. the channel tail
@pytest.mark.parametrize("C", AC.PLANT_WIDTHS)
def test_e2_the_channel_tail_decides(torch, wct, C):
    """tau = 32 with the scores carried by four channels: zeroing them moves the fp64 mean by 0.78 max |V| and more
    (tests/test_attn_cpu.py), the gate is below 2e-5.  Measured on the MI355X over the 67 cases: mean at most 3.0e-6 (fp32 arm 2.9e-6), var at
    most 1.2e-6 (2.1e-6); nearest the gate 0.78 and 0.74 of it."""
    for name, c0 in AC.plants(C).items():
        q, k, v = AC.planted_inputs(C, c0)
        m, var = gpu_stats(torch, wct, q, k, v, AC.PLANT_TAU)
        held(m, var, AC.reference(q, k, v, AC.PLANT_TAU), "E2 C=%d %s (channels %d..%d)" % (C, name, c0, c0 + 3))
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- E3. slabs and position
@pytest.mark.parametrize("C", AC.ROLL_WIDTHS)
def test_e3_rolling_the_value_columns_rolls_the_outputs_bit_for_bit(torch, wct, C):
    """The header: a query's row does not depend on the slab split.  V's columns rolled by 4, 16 and 128 (mod C) move channels between
    value tiles, lanes and slabs (and into and out of the ragged last slab); q^, k^ and max |V| stay, so every output column must be the
    un-rolled one, moved.  Measured on the MI355X: no value differs in any of the 12 cases."""
    q, k, v = AC.edge_inputs(C)
    m0, var0 = gpu_stats(torch, wct, q, k, v, AC.ROLL_TAU)
    held(m0, var0, AC.reference(q, k, v, AC.ROLL_TAU), "E3 C=%d" % C)
    for r in AC.ROLLS:
        m, var = gpu_stats(torch, wct, q, k, np.roll(v, r, axis=1), AC.ROLL_TAU)
        dm, dv = bits(m) != bits(np.roll(m0, r, axis=1)), bits(var) != bits(np.roll(var0, r, axis=1))
        print("edges E3 C=%d roll %d: %d mean and %d var values differ" % (C, r, int(dm.sum()), int(dv.sum())))
        assert not dm.any() and not dv.any(), "C=%d roll %d: columns %s differ" % (C, r, sorted(set(np.nonzero(dm | dv)[1]))[:16])
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- E4. tile borders
@pytest.mark.parametrize("tau", AC.BORDER_TAUS)
@pytest.mark.parametrize("C", AC.BORDER_WIDTHS)
def test_e4_tile_borders_on_both_axes(torch, wct, C, tau):
    """Nk in 2, 31 .. 33, 63 .. 65 x Nq in 2, 63 .. 65, rows of one draw.  At tau = 0 also the header's statement, on the standardised map
    of the Nk keys themselves: |mean| within the gate of 0 and var within the gate of (Nk - 1) / Nk  v / (v + eps).  Measured on the MI355X:
    mean 8.7e-7 (fp32 arm 7.2e-7) and var 6.7e-7 (1.6e-7) at most at tau = 32, 5.0e-8 and 8.4e-8 at tau = 0; the statement: |mean| at most
    1.8e-8, var within 1.2e-7."""
    failures, worst = [], [0.0, 0.0]
    for Nk in AC.BORDER_NK:
        for Nq in AC.BORDER_NQ:
            q, k, v = AC.border_inputs(C, Nq, Nk)
            m, var = gpu_stats(torch, wct, q, k, v, tau)
            em, ev, _, _ = held(m, var, AC.reference(q, k, v, tau), "E4 C=%d tau=%g Nq=%d Nk=%d" % (C, tau, Nq, Nk), failures)
            worst = [max(worst[0], em), max(worst[1], ev)]
            if tau == 0:
                vs, want = AC.border_standardised(C, Nk)
                _, (e32m, e32v), vmax = AC.reference(q, k, vs, 0.0)
                m, var = gpu_stats(torch, wct, q, k, vs, 0.0)
                zm, zv = float(np.abs(m).max()) / vmax, float(np.abs(var - want).max()) / vmax ** 2
                print("edges E4 C=%d tau=0 Nq=%d Nk=%d, the header's statement: |mean| %.3e, var off by %.3e" % (C, Nq, Nk, zm, zv))
                if not (zm <= 4 * e32m + FLOOR_MEAN and zv <= 4 * e32v + FLOOR_VAR):
                    failures.append("Nq=%d Nk=%d: tau = 0 is not AdaIN with the population variance: %.3e / %.3e" % (Nq, Nk, zm, zv))
    print("edges E4 C=%d tau=%g worst: mean %.3e var %.3e" % (C, tau, *worst))
    assert not failures, "; ".join(failures)
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- E5. the running maximum
@pytest.mark.parametrize("order", AC.RUN_ORDERS)
@pytest.mark.parametrize("C", AC.RUN_WIDTHS)
def test_e5_the_running_maximum(torch, wct, C, order):
    """Five key tiles, tau = 32.  "up" / "spread_up": every tile raises every row's maximum (by 2 .. 54 and by 0.08 .. 2.6 in the logit), so
    the rescale runs at every tile; "down" / "spread_down": at none after the first; "own": key 0 is the query direction and every other
    P' rounds to 0 in f16 -- mean = V[0], var = 0 (the header bounds the dropped weight mass by Nk 2^-40 = 1.2e-10).  A walk that never
    rescales is 7e-2 and more off on the ascending orders (tests/test_attn_cpu.py).  Measured on the MI355X (C = 36 / 132): up, down and own
    alike 5.0e-8 / 7.9e-8 (mean) and 1.1e-8 / 1.3e-8 (var), the fp32 arm being exact there; the spread orders 4.8e-7 / 6.5e-7 and 2.5e-7 / 4.6e-7
    (fp32 arm 6.1e-7 .. 7.6e-7 and 3.6e-7 .. 5.4e-7)."""
    q, k, v = AC.running_inputs(C, order)
    ref = AC.reference(q, k, v, AC.RUN_TAU)
    m, var = gpu_stats(torch, wct, q, k, v, AC.RUN_TAU)
    held(m, var, ref, "E5 C=%d %s" % (C, order))
    if order == "own":
        vmax = ref[2]
        dm, dv = float(np.abs(m - v[0]).max()) / vmax, float(var.max()) / vmax ** 2
        print("edges E5 C=%d own: |mean - V[0]| %.3e, var %.3e" % (C, dm, dv))
        assert dm <= FLOOR_MEAN and dv <= FLOOR_VAR
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- E6. the default split
@pytest.mark.parametrize("C", AC.SPLIT_WIDTHS)
def test_e6_the_default_launch_split(torch, wct, C):
    """32768 + 65 queries, no debug key: launches of 512 and 2 query tiles (the form is l2.s1 at C = 4, l2.s2 at C = 132), held against
    fp64; rows 32768 .. are bit for bit those of a call on these 65 queries alone.  Measured on the MI355X: 3.5e-7 / 4.0e-7 at C = 4 (fp32 arm
    3.6e-7 / 4.5e-7), 2.3e-7 / 2.0e-7 at C = 132 (3.4e-7 / 1.5e-7)."""
    q, k, v = AC.split_inputs(C)
    p = AC.plan(q.shape[0], k.shape[0], C)
    assert (p.launches, p.query_tiles, p.form) == (2, (512, 2), "l2.s%d" % (1 if C == 4 else 2))
    m, var = gpu_stats(torch, wct, q, k, v, AC.SPLIT_TAU)
    held(m, var, AC.reference(q, k, v, AC.SPLIT_TAU), "E6 C=%d, %d queries" % (C, q.shape[0]))
    tm, tvar = gpu_stats(torch, wct, q[AC.QUERY_CHUNK:], k, v, AC.SPLIT_TAU)
    assert tm.shape == (AC.QUERY_TILE + 1, C)
    assert np.array_equal(bits(m[AC.QUERY_CHUNK:]), bits(tm)) and np.array_equal(bits(var[AC.QUERY_CHUNK:]), bits(tvar))
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- E7. projection, apply
@pytest.mark.parametrize("b", BANDS)
def test_e7_project_and_apply_at_every_width(torch, wct, b):
    """wct_attn_project, standard domain, on 1 x 17 maps (one full 16-row group of attn_unit_kernel and one row): unit rows and the
    standardised map within 1e-6 of the largest value.  wct_attn_apply at n = 65 against its fp32 emulation, bit for bit.  Measured on the
    MI355X: unit rows at most 1.7e-7, standardised map 1.4e-7."""
    failures, worst = [], [0.0, 0.0]
    for C in sweep_cases.BANDS[b]:
        f = AC.project_map(C)
        unit, std = wct.attn_project(cu(torch, f)[None], "attention")
        u64, s64 = A.project(f, A.STANDARD)
        eu = np.abs(unit[0].cpu().numpy() - u64).max() / np.abs(u64).max()
        es = np.abs(std[0].cpu().numpy() - s64).max() / np.abs(s64).max()
        worst = [max(worst[0], eu), max(worst[1], es)]
        if not (eu <= PROJECT_GATE and es <= PROJECT_GATE):
            failures.append("C=%d: unit %.3e std %.3e" % (C, eu, es))
        m, v, z, x, mu, sg = AC.apply_inputs(C)
        got = wct.attn_apply(cu(torch, m), cu(torch, v), cu(torch, z), cu(torch, x), cu(torch, mu, np.float64), cu(torch, sg, np.float64), 0.6)
        diff = bits(got.cpu().numpy()) != bits(A.apply_f32_emulation(m, v, z, x, mu, sg, 0.6))
        if tuple(got.shape) != x.shape or diff.any():
            failures.append("C=%d: wct_attn_apply differs from its emulation in %d values, columns %s" % (C, int(diff.sum()), sorted(set(np.nonzero(diff)[1]))[:8]))
    print("edges E7 band %d worst: unit %.3e std %.3e" % (b, *worst))
    assert not failures, "; ".join(failures)
    assert wct.saturation_count() == 0


@pytest.mark.parametrize("C", AC.WHITEN_WIDTHS)
def test_e7_whitened_projection(torch, wct, C):
    """Maps of 2 C + 3 positions (ragged against the 8 pixels of an attn_whiten_kernel workgroup; cond(cov) 23 .. 104, tests/test_attn_cpu.py),
    C either side of the kernel's one and two output channels per thread: the ordinary 1e-6.  The eigen-solve has its own width sweep
    (tests/test_sweep_gpu.py), so a miss here points at the transpose, whiten or unit kernels.  Measured on the MI355X: unit rows
    6.3e-8 .. 1.1e-7, standardised map 5.2e-8 .. 1.2e-7."""
    f = AC.whiten_map(C)
    unit, std = wct.attn_project(cu(torch, f)[None], "attention_whitened")
    u64, s64 = A.project(f, _lib.ATTN_MATCHES["attention_whitened"])
    eu = np.abs(unit[0].cpu().numpy() - u64).max() / np.abs(u64).max()
    es = np.abs(std[0].cpu().numpy() - s64).max() / np.abs(s64).max()
    print("edges E7 whitened C=%d, %d positions: unit %.3e std %.3e" % (C, f.shape[1], eu, es))
    assert eu <= PROJECT_GATE and es <= PROJECT_GATE
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- E8. one level
@pytest.fixture(scope="module")
def level_engines(torch):
    cache = {}

    def get(model):
        if model not in cache:
            if model == "wide":
                cache[model] = sc.make_engine("wide", w=AC.model_weights(model))
            else:
                from tests.shard_engine import WidthWCT
                cache[model] = WidthWCT(AC.ALL_LEVEL_MODELS[model][0], AC.model_weights(model))
        return cache[model]
    return get


@pytest.mark.parametrize("model,level,domain", AC.EDGE_LEVEL_CASES)
def test_e8_one_level_at_the_missing_widths(torch, level_engines, model, level, domain):
    """test_one_level_against_the_fp64_composition of tests/test_attn_gpu.py at level 3 of the un-pruned widths (C = 256, two full slabs)
    and of a stand-in with 132 channels there (a second slab of 4): the same images, tau, alpha and gate, 4 e32 + 1e-4.  The input
    condition of these cases is asserted by tests/test_attn_cpu.py.  Measured on the MI355X (standard / whitened): 2.5e-6 / 2.8e-6 at C = 256
    (fp32 pipeline 4.3e-6 / 3.6e-6), 1.8e-6 / 2.1e-6 at C = 132 (3.3e-6 / 3.4e-6)."""
    eng = level_engines(model)
    c, s = AC.level_images()
    match = "attention" if domain == A.STANDARD else "attention_whitened"
    got = eng.attn_level(level, cu(torch, c)[None], cu(torch, s)[None], match, AC.LEVEL_TAU, AC.LEVEL_ALPHA)
    torch.cuda.synchronize()
    ref, _, var = AC.level_reference(model, level, domain)
    assert var[:, A.live_channels(AC.level_features(model, level)[1])].min() >= AC.MIN_VAR
    ref32 = AC.level_reference(model, level, domain, False)[0]
    scale = np.abs(ref).max()
    e32 = np.abs(ref32 - ref).max() / scale
    err = np.abs(got[0].cpu().numpy() - ref).max() / scale
    print("edges E8 level %s %d domain %d: %.3e (fp32 arm %.3e)" % (model, level, domain, err, e32))
    assert tuple(got.shape) == (1,) + ref.shape
    assert err <= 4 * e32 + LEVEL_FLOOR
    assert eng.saturation_count() == 0
