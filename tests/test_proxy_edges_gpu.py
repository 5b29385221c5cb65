"""The bilateral grid's fit and slice (include/wct_hip_bgrid.h, csrc/bgrid.hip) at every edge of their launchers against the numpy fp64
reference (tests/proxy_oracle.py), on the cases of tests/proxy_edge_cases.py, whose counts tests/test_proxy_cpu.py asserts.

Fit: column supports either side of the 256-column weight table, lane strides against supports 1, 63, 64, 65 and 128 columns wide, row
chunks past a vertex's support (also under poisoned scratch), 64, 65 and 67 slabs of totals -- with weight in the slabs past the 64th --
the largest axes, and a guide that leaves [0, 1]: all at the shipped gate of one fp32 ulp.
Slice: seeded random grids (not fitted: neighbouring vertices are unrelated) with one vertex on each axis, the largest axes, launches whose
tiles take both the LDS and the global-memory path, footprints at the cap and one over, one row and one column over many tiles, W < 4 and
W % 4 == 2, wide-range images -- at a single-rounding gate, bit-identical between the paths, with the bitwise properties of
tests/test_proxy_gpu.py at the ragged shapes, and a NaN or Inf pixel that stays local.

Measured on the MI355X (the figures the tests print): see DESIGN section 4.14."""
import numpy as np
import pytest

from tests import proxy_edge_cases as E
from tests import proxy_oracle as O
from tests import state_cases as sc
from tests.test_proxy_gpu import ULP, slice_bitwise_properties, torch, wct      # noqa: F401  (torch, wct: the shipped module fixtures)
from tests.test_proxy_gpu import cu as _cu

pytestmark = pytest.mark.gpu


def cu(torch, a):
    """The shipped helper on a copy: the shared cases are read-only, and torch warns when it wraps such an array."""
    return _cu(torch, np.array(a))


def fit_error(got, ref):
    g = got.cpu().numpy().astype(np.float64)
    return g, float((np.abs(g - ref) / np.maximum(1.0, np.abs(ref))).max())


def bits(t):
    return t.cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- 1. the fit
@pytest.mark.parametrize("case", E.EDGE_FIT_CASES, ids=[E.fit_id(c) for c in E.EDGE_FIT_CASES])
def test_fit_edges_against_the_oracle(torch, wct, case):
    """The gate of test_fit_against_the_oracle: one fp32 ulp of max(1, |A|); cond <= 1e6 (asserted in tests/test_proxy_cpu.py) keeps the
    fp64 solve error far below the single rounding."""
    h, w, gz, gh, gw, kind, eps, smooth = case
    cl, sl, ref, _, _ = E.fit_reference(*case)
    got = wct.bgrid_fit(cu(torch, cl), cu(torch, sl), gz, gh, gw, eps, smooth)
    assert tuple(got.shape) == (gz, gh, gw, 3, 4) and got.dtype == torch.float32
    g, rel = fit_error(got, ref)
    print("bgrid_fit %dx%d grid %dx%dx%d eps=%g smooth=%d: max |d| / max(1, |A|) = %.3e (%.2f ulp), max |A| = %.3f"
          % (h, w, gz, gh, gw, eps, smooth, rel, rel / ULP, np.abs(ref).max()))
    assert np.isfinite(g).all()
    assert rel <= ULP, (case, rel)


@pytest.mark.parametrize("case", E.POISON_CASES, ids=[E.fit_id(c) for c in E.POISON_CASES])
def test_fit_edges_under_poisoned_scratch(torch, wct, case):
    """Every partial is written, those of a chunk past its vertex's support too: with the context's scratch filled with 0xFF (NaN) before
    the call the bits are those of the unpoisoned engine, and they meet the oracle gate."""
    h, w, gz, gh, gw, kind, eps, smooth = case
    cl, sl, ref, _, _ = E.fit_reference(*case)
    a, b = cu(torch, cl), cu(torch, sl)
    want = wct.bgrid_fit(a, b, gz, gh, gw, eps, smooth)
    eng = sc.make_engine("16x")
    eng.debug_set("poison", 0xFF)
    got = eng.bgrid_fit(a, b, gz, gh, gw, eps, smooth)
    eng.debug_set("poison", 0xFF)
    again = eng.bgrid_fit(a, b, gz, gh, gw, eps, smooth)      # the buffers exist now: poisoned at their final size
    eng.debug_set("poison", -1)
    assert torch.equal(got, want) and torch.equal(again, want), "poisoned scratch changes the fit"
    g, rel = fit_error(got, ref)
    assert np.isfinite(g).all() and rel <= ULP, (case, rel)


@pytest.mark.parametrize("case", E.UNREACHED, ids=[E.fit_id(c) for c in E.UNREACHED])
def test_fit_edges_unreached_vertices_hold_the_global_map_of_more_than_64_slabs(torch, wct, case):
    """Some 16000 vertices under 576 pixels: most have an oracle weight sum of exactly 0, and each of them holds Ag -- the totals of 65
    slabs (the last of one vertex) and of 67 (2.5 % of the weight past the 64th) -- to the rounding."""
    h, w, gz, gh, gw, kind, eps, smooth = case
    assert smooth == 0 and E.slabs(gz, gh, gw) > 64
    cl, sl, ref, Ag, _ = E.fit_reference(*case)
    reached = O.sums(cl, sl, gz, gh, gw)[0][..., 3, 3] != 0.0
    assert 0 < reached.sum() < reached.size
    got = wct.bgrid_fit(cu(torch, cl), cu(torch, sl), gz, gh, gw, eps, smooth).cpu().numpy()
    empty = got[~reached]
    assert np.array_equal(empty.view(np.uint32), np.broadcast_to(empty[0].view(np.uint32), empty.shape)), "unreached vertices differ among themselves"
    err = float(np.abs(empty[0].astype(np.float64) - Ag).max())
    print("bgrid_fit %d slabs: %d of %d vertices unreached, |Ag - oracle| = %.3e (%.2f ulp of max(1, |Ag|))"
          % (E.slabs(gz, gh, gw), (~reached).sum(), reached.size, err, err / (ULP * max(1.0, np.abs(Ag).max()))))
    assert err <= ULP * max(1.0, np.abs(Ag).max())
    assert (got[reached].view(np.uint32) != empty[0].view(np.uint32)).any(), "no reached vertex differs from the global map"


# ---------------------------------------------------------------------------------------------------------------- 2. the slice
SLICE = [c[:6] for c in E.EDGE_SLICE_CASES]


@pytest.mark.parametrize("case", SLICE, ids=[E.slice_id(c) for c in SLICE])
def test_slice_edges_against_the_oracle_and_between_the_two_paths(torch, wct, case):
    """The gate is the header's promise, fp64 throughout and ONE rounding: half an fp32 ulp of the result, at most 2^-24 max(1, |ref|)
    relative to 2^-23 max(1, |ref|) asked here.  The fp64 terms add about 1e-15; a guide that differs from the oracle's in its last bit
    moves the weights continuously, by at most (gz - 1) 2^-52 |A|."""
    gz, gh, gw, H, W, kind = case
    grid, c, ref = E.slice_reference(*case)
    dg, x = cu(torch, grid), cu(torch, c)
    got = wct.bgrid_slice(dg, x)
    assert tuple(got.shape) == (1, 3, H, W) and got.dtype == torch.float32
    g = got.cpu().numpy()[0].astype(np.float64)
    ratio = float((np.abs(g - ref) / (ULP * np.maximum(1.0, np.abs(ref)))).max())
    print("bgrid_slice %dx%d (%s) of a random grid %dx%dx%d: max |d| / (2^-23 max(1, |ref|)) = %.3f, max |ref| = %.3f"
          % (H, W, kind, gz, gh, gw, ratio, np.abs(ref).max()))
    assert np.isfinite(g).all()
    assert ratio <= 1.0, (case, ratio)
    # which path the default launch took, where the case is about that
    foot = E.tile_footprints(gz, gh, gw, H, W)
    if case in E.MIXED:
        assert min(foot) <= E.CAP < max(foot)
    elif case in E.AT_CAP:
        assert foot == [E.CAP]
    elif case in E.OVER_CAP:
        assert len(foot) == 1 and foot[0] > E.CAP
    wct.debug_set("bgrid_lds", 0)
    try:
        forced = wct.bgrid_slice(dg, x)
    finally:
        wct.debug_set("bgrid_lds", 1)
    assert np.array_equal(bits(forced), bits(got)), "the global-memory path and the LDS path give different bits"


@pytest.mark.parametrize("case", E.BITWISE, ids=[E.slice_id(c) for c in E.BITWISE])
def test_slice_edges_bitwise_properties(torch, wct, case):
    """The set of test_slice_bitwise_properties -- views off a 16-byte boundary, in place, fused uint8 in both round modes at two byte
    bases, guards intact -- where every store is scalar (W < 4, one column), where a row ends on two pixels, and over mixed paths."""
    grid, c, _ = E.slice_reference(*case)
    slice_bitwise_properties(torch, wct, cu(torch, grid), cu(torch, c))


def test_slice_edges_a_non_finite_pixel_stays_local(torch, wct):
    """A NaN in one channel of one pixel and +Inf in another pixel (two threads' quads, neither at a row's end) change no other pixel."""
    gz, gh, gw, H, W, kind = E.NONFINITE
    grid, c, _ = E.slice_reference(*E.NONFINITE)
    clean, dirty = c.copy(), c.copy()
    spots = [(4, 57), (7, 101)]
    for y, x in spots:
        clean[:, y, x] = 0.0
    dirty[:, 4, 57] = 0.0
    dirty[1, 4, 57] = np.nan
    dirty[:, 7, 101] = 0.0
    dirty[2, 7, 101] = np.inf
    dg = cu(torch, grid)
    want = bits(wct.bgrid_slice(dg, cu(torch, clean)))
    for lds in (1, 0):
        wct.debug_set("bgrid_lds", lds)
        try:
            got = bits(wct.bgrid_slice(dg, cu(torch, dirty)))
        finally:
            wct.debug_set("bgrid_lds", 1)
        keep = np.ones((H, W), bool)
        for y, x in spots:
            keep[y, x] = False
        assert np.array_equal(got[0][:, keep], want[0][:, keep]), "a non-finite pixel changed another pixel (bgrid_lds %d)" % lds      # their own: not asserted
