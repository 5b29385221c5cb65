"""tests/shard_cases.py against the two implementations of the sharded geometry (wct_shard_geometry: host arithmetic of the C ABI, no
device call; wct_hip/sharded.py ShardedStylizer without an engine), the partition property of the owned windows, and the preconditions of
the fp64-compared cases of tests/test_shard_widths_gpu.py from the fp64 reference alone.  No GPU."""
import ctypes
import sys

import numpy as np
import pytest

from tests import shard_cases as SC
from tests import width_models as wm
from tests.test_sweep_gpu import SOLVE_MAX_COND

MODE_IDS = {"auto": 0, "recompute": 1, "exchange": 2}
NAMES = {v: k for k, v in MODE_IDS.items()}
RANKS = range(1, 9)
OT_MAX_COND = 1e10          # tests/test_transform_gpu.py gate_for: the solver's 1e-6 class ends here


def test_helper_imports_without_torch():
    import subprocess
    code = "import sys; sys.path[:0] = %r; from tests import shard_cases; assert 'torch' not in sys.modules, 'torch imported'" % (sys.path[:3],)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


def test_constants_are_those_of_sharded_py_and_the_library_modes():
    from wct_hip import lib, sharded
    assert SC.LEVEL_HALO == sharded.LEVEL_HALO and SC.CUM_HALO == sharded.CUM_HALO and SC.STYLE_HALO == sharded.STYLE_HALO
    assert SC.AUTO_EXCHANGE_BELOW == sharded.AUTO_EXCHANGE_BELOW
    assert lib.HALO_MODES == MODE_IDS
    # what the halos promise each other: on the level's pooling grid, and the cumulative margin covers the next level's after this level's field
    for L in SC.LEVELS:
        for halo in (SC.LEVEL_HALO, SC.CUM_HALO, SC.STYLE_HALO):
            assert halo[L] % (1 << (L - 1)) == 0
        if L > 1:
            assert SC.CUM_HALO[L] - SC.LEVEL_HALO[L] >= SC.CUM_HALO[L - 1]


# ---------------------------------------------------------------------------------------------------- a. geometry sweep
def test_geometry_sweep_library_and_python_agree():
    """Every W of the sweep, 1..8 ranks, every rank, all three halo modes: wct_shard_geometry, ShardedStylizer and shard_cases.geometry give
    the same own, input columns and resolved mode, or all three refuse."""
    from wct_hip import lib
    from wct_hip.sharded import ShardedStylizer
    L = lib.load()
    v = [ctypes.c_int() for _ in range(5)]
    refs = [ctypes.byref(x) for x in v]
    refused = agreed = 0
    for W in SC.sweep_widths():
        for n in RANKS:
            for mode in SC.HALO_MODES:
                for r in range(n):
                    want = SC.geometry(W, n, r, mode)
                    rc = L.wct_shard_geometry(W, n, r, MODE_IDS[mode], *refs)
                    try:
                        sh = ShardedStylizer(None, None, 64, W, 64, 64, rank=r, world=n, halo_mode=mode)
                        py = sh.own + sh.input_columns() + (sh.halo_mode,)
                    except ValueError:
                        py = None
                    got = None if rc != 0 else tuple(x.value for x in v[:4]) + (NAMES[v[4].value],)
                    assert got == want and py == want, (W, n, r, mode, got, py, want)
                    refused += want is None
                    agreed += want is not None
    assert refused > 1000 and agreed > 10000, (refused, agreed)
    # arguments outside the domain
    for bad in ((0, 1, 0, 0), (64, 0, 0, 0), (64, 2, 2, 0), (64, 2, -1, 0), (640, 2, 0, 3), (640, 2, 0, -1)):
        assert L.wct_shard_geometry(*bad, *refs) != 0, bad


# ---------------------------------------------------------------------------------------------------- b. windows partition the map
def test_owned_windows_partition_every_level():
    """Per level the ranks' owned feature windows -- from own, the level's lo and the floor-shrunk running width, as wct_stylize_sharded and
    sharded.py derive them -- cover feature columns 0 .. (Wc >> sh) - 1 exactly once, so the per-rank n add up to n_total / h."""
    checked = 0
    for W in SC.sweep_widths():
        for n in RANKS:
            for mode in SC.HALO_MODES:
                wins = SC.content_windows(W, n, mode)
                assert (wins is None) == (SC.geometry(W, n, 0, mode) is None)
                if wins is None:
                    continue
                Wc = W
                for L in SC.LEVELS:
                    row = wins[L]
                    assert row[0].Wc == Wc and row[0].wf == Wc >> (L - 1)
                    err = SC.partition_error(row)
                    assert err is None, (W, n, mode, L, err)
                    assert sum(p.n for p in row) == row[0].wf
                    for p in row:
                        # the strip is inside the running image, holds its owned columns, and f1 marks the last strip alone
                        assert 0 <= p.lo <= p.own[0] < p.own[1] <= p.hi <= Wc, (W, n, mode, L, vars(p))
                        assert (p.f1 < 0) == (p.rank == n - 1)
                        assert p.f1 < 0 or p.f1 <= (p.hi - p.lo) >> (L - 1)
                    Wc = (Wc >> (L - 1)) << (L - 1)
                    checked += 1
    assert checked > 50000


def test_style_strip_windows_partition_every_level():
    for Ws in SC.sweep_widths(seed=8, count=100, top=8192):
        for n in RANKS:
            wins = SC.style_windows(Ws, n)
            assert (wins is None) == (SC.strip_bounds(Ws, n) is None)
            if wins is None:
                continue
            for L in SC.LEVELS:
                err = SC.partition_error(wins[L])
                assert err is None, (Ws, n, L, err)
                assert sum(p.n for p in wins[L]) == Ws >> (L - 1)


def test_windows_are_those_of_the_python_orchestration():
    """shard_cases.content_windows against the arithmetic inside sharded.py's loop, replayed with its own helpers (ext_bounds, strip_bounds)."""
    from wct_hip import sharded
    for W, n, mode in ((541, 3, "exchange"), (541, 2, "recompute"), (1525, 2, "exchange"), (2005, 3, "recompute"), (4099, 8, "auto"), (333, 2, "auto")):
        wins = SC.content_windows(W, n, mode)
        for r in range(n):
            sh = sharded.ShardedStylizer(None, None, 64, W, 64, 64, rank=r, world=n, halo_mode=mode)
            own, W_cur = sh.own, W
            for L in SC.LEVELS:
                s = L - 1
                lo, hi = sharded.ext_bounds(own, W_cur, sh.halo[L])
                f0 = (own[0] - lo) >> s
                f1 = -1 if own[1] >= W_cur else (own[1] - lo) >> s
                p = wins[L][r]
                assert (p.lo, p.hi, p.f0, p.f1, p.own, p.Wc) == (lo, hi, f0, f1, own, W_cur), (W, n, mode, r, L)
                W_cur = (W_cur >> s) << s
                own = (own[0], min(own[1], W_cur))


# ---------------------------------------------------------------------------------------------------- c. the plan and its preconditions
def test_case_geometry_preconditions():
    for model in ("A", "B", "C"):
        c = SC.case_of(model)
        assert c["H"] % 16 != 0                                              # floor pooling takes rows as well
        assert c["W"] - (c["W"] >> 4 << 4) > 0                               # ... and columns from the last strip
        both = {L: False for L in SC.LEVELS}
        for world in SC.WORLDS:
            wins = SC.content_windows(c["W"], world, "exchange")             # LEVEL_HALO margins
            assert wins is not None and SC.style_windows(c["Ws"], world) is not None
            for L in SC.LEVELS:
                for p in wins[L]:
                    assert p.hi - p.lo < p.Wc                                # every strip is a crop ...
                    both[L] |= p.lo > 0 and p.hi < p.Wc                      # ... some rank's on both sides
            last = wins[5][-1]
            assert last.own[1] - (last.Wc >> 4 << 4) == 13 and last.f1 == -1
        assert all(both.values()), both
    assert [b[1] - b[0] for b in SC.strip_bounds(541, 3)] == [176, 176, 189]


def test_fold_forms_mix_in_models_a_and_b():
    assert SC.fast_fold_levels(wm.MODELS["A"]) == [2, 1] and SC.fast_fold_levels(wm.MODELS["B"]) == [3, 1]
    assert SC.fast_fold_levels(wm.MODELS["C"]) == [] and SC.fast_fold_levels(wm.W16X) == [5, 4, 3, 2, 1]
    # five different feature widths per model: a packed-buffer offset taken from another level's C lands inside a neighbour
    for model in ("A", "B", "C"):
        assert len({wm.feature_channels(wm.MODELS[model], L) for L in SC.LEVELS}) == 5


@pytest.mark.parametrize("mode", SC.TRANSFORMS)
@pytest.mark.parametrize("model", sorted(SC.CASES))
def test_fp64_compared_levels_are_well_posed(model, mode):
    """From the fp64 arm alone: at every level content and style have at least 2 C feature pixels and full rank on their live channels
    (shard_cases.conditioning), and cond(cov_c) stays under SOLVE_MAX_COND (tests/test_sweep_gpu.py: beyond it fp64 moments do not
    determine (M, b) to the solver's gate).

    Under ot cond(B) is held to OT_MAX_COND = 1e10, the end of the range tests/test_transform_gpu.py gate_for covers (1e-6 on the map there:
    a hundredth of the level gate's 1e-4 floor), NOT to the 1e6 of its well-conditioned class: B = S cov_c S multiplies the two spectra, and
    with these stand-in weights levels 5, 4 and 3 of both models sat between 7e6 and 8e11 on wm.smooth_image inputs of 120, 248 and 504
    rows with 0, 2 and 6 smoothing passes, and over fifteen seeds at the case's own size: no shape brings them under 1e6."""
    ref = SC.reference(model, mode)
    for L in SC.LEVELS:
        d = SC.conditioning(ref, L)
        print("shard case %s %s level %d: C %d (live %d / %d), n_c %d n_s %d, cond(cov_c) %.2e cond(cov_s) %.2e cond(B) %.2e, fp32 arm %.2e"
              % (model, mode, L, d["C"], d["live_c"], d["live_s"], d["n_c"], d["n_s"], d["cond_c"], d["cond_s"], d["cond_B"], ref.e32[L]))
        assert d["n_c"] >= 2 * d["C"] and d["n_s"] >= 2 * d["C"], (model, L, d)
        # full rank on the live channels (shard_cases.conditioning: channels the stand-in weights leave exactly zero are set aside)
        assert d["rank_c"] == d["live_c"] and d["rank_s"] == d["live_s"], (model, L, d)
        assert d["cond_c"] <= SOLVE_MAX_COND, (model, mode, L, d)
        if mode == "ot":
            assert d["cond_B"] <= OT_MAX_COND, (model, L, d)
        assert np.isfinite(ref.r64[L].out).all() and ref.r64[L].out.shape[1:] == (ref.inputs[L].shape[1] >> (L - 1) << (L - 1),
                                                                                   ref.inputs[L].shape[2] >> (L - 1) << (L - 1))


def test_level_reference_is_wm_style_transfer_under_wct():
    """The wct arm of shard_cases.level_reference against wm.style_transfer (the oracle's whiten_and_color): two statements of one level."""
    widths, w = wm.MODELS["A"], SC.weights("A")
    rng = np.random.default_rng(3)
    c, s = wm.smooth_image(rng, 40, 56), wm.smooth_image(rng, 36, 48)
    for L in (3, 1):
        got = SC.level_reference(widths, w, "wct", L, c, wm.encode(widths, w, L, s), 0.6).out
        want = wm.style_transfer(widths, w, L, c, s, 0.6)
        # an SVD with a 1e-5 floor against eigh with a relative one: cond(cov_c) eps apart on the map, far below the GPU gate's 1e-4 floor
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-7 * np.abs(want).max(), L
