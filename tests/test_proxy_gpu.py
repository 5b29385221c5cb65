"""Proxy mode on the device (include/wct_hip_bgrid.h): wct_bgrid_fit within one fp32 ulp of the numpy fp64 reference
(tests/proxy_oracle.py), wct_bgrid_slice of the device's own grid under the project's fp64 gate, their bitwise properties (both paths of
the slice, views, repeats, contexts, fused uint8), wct_stylize_proxy against the public calls it is made of (bit for bit), allocation and
graph capture, history independence of the three device entries with the helpers of tests/state_cases.py, the refusals, and the command
line's --proxy_scale.

The module imports without a GPU: tests/test_proxy_cpu.py reads FIT_CASES, fit_pair and CASES.

Measured on the MI355X (the figures the tests print): see DESIGN section 4.14."""
import collections
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from tests import color_oracle as CO
from tests import proxy_oracle as O
from tests import state_cases as sc
from tests.conftest import PKG, REPO
from wct_hip import lib as _lib

pytestmark = pytest.mark.gpu

GATE = 2e-5          # the project's fp64 gate (GATE of tests/test_smooth_gpu.py), absolute
ULP = 2.0 ** -23     # one fp32 ulp at 1: the fit's gate is ULP * max(1, |A|)
ROWS, TW, TH, CAP = _lib.BGRID_FIT_ROWS, _lib.BGRID_TILE_W, _lib.BGRID_TILE_H, _lib.BGRID_LDS_VERTICES


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "-m gpu tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def wct(torch):
    return sc.make_engine("16x")


def cu(torch, a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def offset_view(torch, x, off):
    """A copy of the fp32 tensor x that starts `off` floats behind a 16-byte boundary."""
    buf = torch.empty(x.numel() + 8, device="cuda", dtype=torch.float32)
    base = (-(buf.data_ptr() // 4)) % 4
    v = buf[base + off: base + off + x.numel()]
    assert v.data_ptr() % 16 == 4 * off
    v.copy_(x.reshape(-1))
    return v.view(x.shape)


def q8(x):
    """8-bit quantisation: multiples of 1/255, as every decoded photograph is."""
    return (np.round(np.asarray(x, np.float64) * 255) / 255).astype(np.float32)


def fit_pair(h, w, narrow=False):
    """(reduced content, its "stylisation"), 3 x h x w fp32, seeded by the shape: a natural-like 8-bit content and a result that is a
    tone curve and colour mix of it plus texture of its own, unquantised, in about [-0.1, 1.2] -- what a cascade returns.
    narrow: the content's luminance stays in [0.4, 0.6], so the outer luminance vertices of an 8-bin grid see no pixel."""
    c = q8(CO.natural(h * 7 + w, h, w))
    if narrow:
        c = q8(0.4 + 0.2 * c.astype(np.float64))
    return c, tone_curve(c)


def tone_curve(c):
    """fit_pair's "stylisation" of a 3 x h x w content with values >= 0 (tests/proxy_edge_cases.py feeds it a clipped wide-range one)."""
    h, w = c.shape[1:]
    x = c.astype(np.float64)
    mix = np.array([[0.7, 0.3, -0.1], [0.1, 0.8, 0.2], [-0.2, 0.3, 0.9]])
    s = np.einsum("ci,ihw->chw", mix, np.sqrt(x)) * 1.1 - 0.1 + 0.15 * CO.natural(h * 13 + w + 1, h, w, cast=(0.6, 1.0, 0.9), shift=(0.2, 0.0, 0.1))
    return s.astype(np.float32)


# (h, w, gz, gh, gw, narrow, why): the issue's seven, the fit's row-chunk edges (a support is the whole image with gh <= 2), the empty bins
FIT_SHAPES = [
    (1, 1, 1, 1, 1, False, "a single pixel, a single vertex"),
    (32, 32, 1, 1, 1, False, "the global fit"),
    (3, 5, 3, 4, 6, False, "more vertices than pixels"),
    (32, 48, 2, 2, 2, False, "the smallest grid with two vertices per axis"),
    (40, 56, 8, 3, 4, False, "eight bins"),
    (64, 96, 16, 5, 7, False, "sixteen bins, four waves of four"),
    (70, 90, 32, 6, 7, False, "the largest z axis"),
    (ROWS - 1, 24, 4, 1, 3, False, "one row below the fit's row chunk"),
    (ROWS, 24, 4, 2, 3, False, "exactly one row chunk"),
    (ROWS + 1, 24, 4, 1, 3, False, "one row into a second chunk"),
    (2 * ROWS + 1, 10, 2, 2, 2, False, "three chunks, the last of one row"),
    (40, 56, 8, 3, 4, True, "luminance in [0.4, 0.6]: bins no pixel reaches"),
]
FIT_CASES = [s[:6] + (eps, smooth) for s in FIT_SHAPES for eps in (1e-2, 1e-4) for smooth in (0, 1, 4)]
EMPTY_BINS = (40, 56, 8, 3, 4, True, 1e-2, 0)

_FIT = {}


def fit_reference(h, w, gz, gh, gw, narrow, eps, smooth):
    """(cl, sl, the oracle's grid) of a FIT_CASES case, computed once and shared (read-only)."""
    key = (h, w, gz, gh, gw, narrow, eps, smooth)
    if key not in _FIT:
        cl, sl = fit_pair(h, w, narrow)
        ref = O.fit(cl, sl, gz, gh, gw, eps, smooth)
        ref.setflags(write=False)
        _FIT[key] = (cl, sl, ref)
    return _FIT[key]


# ---------------------------------------------------------------------------------------------------------------- 1. the fit
@pytest.mark.parametrize("h,w,gz,gh,gw,narrow,eps,smooth", FIT_CASES,
                         ids=["%dx%d-g%dx%dx%d%s-eps%g-s%d" % (c[:5] + ("-narrow" if c[5] else "",) + c[6:]) for c in FIT_CASES])
def test_fit_against_the_oracle(torch, wct, h, w, gz, gh, gw, narrow, eps, smooth):
    """Within one fp32 ulp: the fp64 solve error is about cond * 2^-53 (cond <= 1e6, asserted in tests/test_proxy_cpu.py), far
    below 2^-24, so only the single rounding to fp32 can differ."""
    cl, sl, ref = fit_reference(h, w, gz, gh, gw, narrow, eps, smooth)
    got = wct.bgrid_fit(cu(torch, cl), cu(torch, sl), gz, gh, gw, eps, smooth)
    assert tuple(got.shape) == (gz, gh, gw, 3, 4) and got.dtype == torch.float32
    g = got.cpu().numpy().astype(np.float64)
    rel = float((np.abs(g - ref) / np.maximum(1.0, np.abs(ref))).max())
    print("bgrid_fit %dx%d grid %dx%dx%d eps=%g smooth=%d: max |d| / max(1, |A|) = %.3e (%.2f ulp), max |A| = %.3f"
          % (h, w, gz, gh, gw, eps, smooth, rel, rel / ULP, np.abs(ref).max()))
    assert np.isfinite(g).all()
    assert rel <= ULP, (h, w, gz, gh, gw, eps, smooth, rel)


def test_fit_gives_unreached_vertices_the_global_map(torch, wct):
    h, w, gz, gh, gw, narrow, eps, smooth = EMPTY_BINS
    cl, sl, _ = fit_reference(*EMPTY_BINS)
    _, Ag, _, _ = O.fit(cl, sl, gz, gh, gw, eps, smooth, details=True)
    got = wct.bgrid_fit(cu(torch, cl), cu(torch, sl), gz, gh, gw, eps, smooth).cpu().numpy()
    for k in (0, 1, 6, 7):      # g (gz - 1) in [2.8, 4.2]: only the vertices 2 .. 5 are reached
        assert np.array_equal(got[k], np.broadcast_to(got[k, 0, 0], got[k].shape)), k
        assert np.abs(got[k, 0, 0].astype(np.float64) - Ag).max() <= ULP * max(1.0, np.abs(Ag).max()), k
    assert not np.array_equal(got[3], np.broadcast_to(got[3, 0, 0], got[3].shape))


def test_fit_bitwise_properties(torch, wct):
    cl, sl = fit_pair(70, 90)
    a, b = cu(torch, cl), cu(torch, sl)
    got = wct.bgrid_fit(a, b, 8, 6, 7, 1e-2, 1)
    assert torch.equal(wct.bgrid_fit(a, b, 8, 6, 7, 1e-2, 1), got), "two calls differ"
    for off in (1, 2, 3):
        out = offset_view(torch, torch.zeros(8 * 6 * 7 * 12, device="cuda"), off)
        back = wct.bgrid_fit(offset_view(torch, a, off), offset_view(torch, b, (off + 1) % 4), 8, 6, 7, 1e-2, 1, out=out)
        assert back.data_ptr() == out.data_ptr() and torch.equal(back, got), "views %d floats off a 16-byte boundary fit differently" % off
    assert torch.equal(sc.make_engine("16x").bgrid_fit(a, b, 8, 6, 7, 1e-2, 1), got), "two contexts differ"
    assert torch.equal(a, cu(torch, cl)) and torch.equal(b, cu(torch, sl)), "an input was written"
    assert torch.equal(wct.bgrid_fit(a, b, 8, 6, 7), got), "the defaults are WCT_BGRID_EPS and WCT_BGRID_SMOOTH"


# ---------------------------------------------------------------------------------------------------------------- 2. the slice
# (name) -> (h, w, gz, gh, gw): the pair a grid is fitted to ON THE DEVICE, with the command line's defaults otherwise
GRIDS = {"16x16": (16, 16, 4, 3, 3), "40x56": (40, 56, 8, 4, 5), "fine": (16, 16, 4, 9, 9), "fine-lds": (16, 16, 4, 8, 9)}
SLICE_CASES = [(g, H, W) for g in ("16x16", "40x56") for (H, W) in
               [(1, 1), (37, 53), (130, 257), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (TH, TW + 1), (TH + 1, TW)]] + \
              [("fine", 8, 8), ("fine-lds", 8, 8)]

_GRID = {}


def device_grid(torch, wct, name):
    if name not in _GRID:
        h, w, gz, gh, gw = GRIDS[name]
        cl, sl = fit_pair(h, w)
        _GRID[name] = wct.bgrid_fit(cu(torch, cl), cu(torch, sl), gz, gh, gw)
        torch.cuda.synchronize()
    return _GRID[name]


def full_image(H, W):
    return q8(CO.natural(H * 11 + W + 3, H, W, cast=(0.9, 1.0, 0.8), shift=(0.0, 0.05, 0.1)))


@pytest.mark.parametrize("name,H,W", SLICE_CASES, ids=["%s-%dx%d" % c for c in SLICE_CASES])
def test_slice_against_the_oracle_and_between_its_two_paths(torch, wct, name, H, W):
    grid = device_grid(torch, wct, name)
    gz, gh, gw = GRIDS[name][2:]
    c = full_image(H, W)
    ref = O.slice_(grid.cpu().numpy(), c)
    x = cu(torch, c)
    got = wct.bgrid_slice(grid, x)
    assert tuple(got.shape) == (1, 3, H, W)
    err = float(np.abs(got.cpu().numpy()[0].astype(np.float64) - ref).max())
    print("bgrid_slice %dx%d of grid %s (%dx%dx%d): max abs err vs fp64 %.3e" % (H, W, name, gz, gh, gw, err))
    assert err <= GATE, (name, H, W, err)
    # a tile of at most TW x TH pixels can touch every vertex: the grid alone decides which path such an image takes
    if name == "fine":
        assert gz * gh * gw > CAP, "this grid is meant to lie beyond the LDS cap"
    elif H <= TH and W <= TW:
        assert gz * gh * gw <= CAP
    wct.debug_set("bgrid_lds", 0)
    try:
        forced = wct.bgrid_slice(grid, x)
    finally:
        wct.debug_set("bgrid_lds", 1)
    assert torch.equal(forced, got), "the global-memory path and the LDS path give different bits"


@pytest.mark.parametrize("name,H,W", [("40x56", 37, 53), ("40x56", 130, 257), ("16x16", TH + 1, TW + 1), ("fine", 8, 8)])
def test_slice_bitwise_properties(torch, wct, name, H, W):
    slice_bitwise_properties(torch, wct, device_grid(torch, wct, name), cu(torch, full_image(H, W)))


def slice_bitwise_properties(torch, wct, grid, x):
    """The bitwise properties of one slice of the device image x [3, H, W] (tests/test_proxy_edges_gpu.py runs them at its own shapes)."""
    H, W = int(x.shape[1]), int(x.shape[2])
    got = wct.bgrid_slice(grid, x)
    assert torch.equal(wct.bgrid_slice(grid, x), got), "two calls differ"
    for off in (1, 2, 3):
        out = offset_view(torch, torch.zeros_like(x), off)
        back = wct.bgrid_slice(offset_view(torch, grid, (off + 2) % 4), offset_view(torch, x, off), out=out.view(-1))
        assert back.data_ptr() == out.data_ptr() and torch.equal(back[0], got[0]), "views %d floats off a 16-byte boundary slice differently" % off
        back = wct.bgrid_slice(grid, offset_view(torch, x, off))              # an aligned output of an unaligned content
        assert torch.equal(back, got)
    assert torch.equal(sc.make_engine("16x").bgrid_slice(grid, x), got), "two contexts differ"
    y = x.clone()
    back = wct.bgrid_slice(grid, y, out=y.view(-1))
    assert back.data_ptr() == y.data_ptr() and torch.equal(y, got[0]), "in place over the content differs from out of place"
    for mode in (0, 1):
        bigb = torch.full((3 * H * W + 8,), 201, device="cuda", dtype=torch.uint8)
        for base in (1, 4):                                                                   # an odd base address, and a 4-byte aligned one
            u8 = wct.bgrid_slice(grid, x, out=bigb[base: base + 3 * H * W], u8=True, round_mode=mode)
            assert u8.dtype == torch.uint8 and tuple(u8.shape) == (H, W, 3)
            assert torch.equal(u8, wct.to_u8(got, mode)), "fused uint8 output differs from to_u8 of the planar output (round_mode %d)" % mode
            assert np.array_equal(u8.cpu().numpy(), CO.to_u8(got.cpu().numpy()[0], mode))
            assert bool((bigb[:base] == 201).all()) and bool((bigb[base + 3 * H * W:] == 201).all())
            bigb.fill_(201)
    big = torch.full((3 * H * W + 8,), -7.0, device="cuda")
    wct.bgrid_slice(grid, x, out=big[4: 4 + 3 * H * W])
    assert torch.equal(big[4: 4 + 3 * H * W].view(1, 3, H, W), got) and bool((big[:4] == -7.0).all()) and bool((big[-4:] == -7.0).all())


def test_slice_of_an_exact_affine_grid_is_that_map(torch, wct):
    """Every vertex the same map: whatever the weights, the result is that map of the content, to one rounding."""
    M = np.array([[0.9, 0.2, -0.1, 0.05], [0.1, 0.7, 0.3, -0.1], [-0.2, 0.1, 1.1, 0.2]], np.float32)
    grid = cu(torch, np.broadcast_to(M, (4, 5, 6, 3, 4)))
    c = full_image(37, 53)
    got = wct.bgrid_slice(grid, cu(torch, c)).cpu().numpy()[0].astype(np.float64)
    want = np.einsum("ca,ahw->chw", M[:, :3].astype(np.float64), c.astype(np.float64)) + M[:, 3].astype(np.float64)[:, None, None]
    assert np.abs(got - want).max() <= 4 * ULP      # |result| < 2: half an ulp of the rounding, the rest for weights that sum to 1 +- 1e-16


# ---------------------------------------------------------------------------------------------------------------- 3. the composition
def compose(w, c, s, D, cell, bins, eps, smooth, alpha, runs, u8=False, round_mode=0):
    """wct_stylize_proxy spelled out in its six public calls; s None: against prepared statistics."""
    H, W = int(c.shape[-2]), int(c.shape[-1])
    h, ww = w.scale_shape(H, W, D)
    cl = w.resample(c, (h, ww), "bicubic")
    sl = (w.stylize(cl, s, alpha=alpha, num_run=runs) if s is not None else w.stylize_prepared(cl, alpha=alpha, num_run=runs)).clone()
    gh, gw = w.bgrid_shape(h, ww, cell)
    grid = w.bgrid_fit(cl, sl, bins, gh, gw, eps, smooth)
    return w.bgrid_slice(grid, c, u8=u8, round_mode=round_mode)


@pytest.mark.parametrize("H,W,D,transform", [
    pytest.param(128, 192, 2, "wct", id="128-192-D2"), pytest.param(256, 272, 4, "wct", id="256-272-D4"),
    pytest.param(128, 192, 2, "ot", id="128-192-D2-ot"), pytest.param(131, 197, 2, "wct", id="131-197-D2")])
def test_stylize_proxy_is_the_composition_of_the_public_calls(torch, wct, H, W, D, transform):
    c = cu(torch, CO.natural(H, H, W))[None]
    s = cu(torch, CO.natural(W, 64, 64, cast=(0.5, 1.0, 0.9), shift=(0.3, 0.0, 0.1)))[None]
    if transform != "wct":
        under_wct = wct.stylize_proxy(c, s, D).clone()
        wct = sc.make_engine("16x")
        wct.set_transform(transform)
        assert not torch.equal(wct.stylize_proxy(c, s, D), under_wct)          # the mode took effect
    for alpha, runs, cell, bins, eps, smooth in ((1.0, 1, 16, 8, 1e-2, 1), (0.6, 2, 8, 4, 1e-3, 0)):
        want = compose(wct, c, s, D, cell, bins, eps, smooth, alpha, runs)
        got = wct.stylize_proxy(c, s, D, cell, bins, eps, smooth, alpha=alpha, num_run=runs)
        assert tuple(got.shape) == (1, 3, H, W), "the result has the content's exact size"
        assert torch.equal(got, want), (alpha, runs)
        assert bool(torch.isfinite(got).all()) and not torch.equal(got, c)
        wct.style_prepare(s)
        assert torch.equal(wct.stylize_proxy(c, None, D, cell, bins, eps, smooth, alpha=alpha, num_run=runs),
                           compose(wct, c, None, D, cell, bins, eps, smooth, alpha, runs)), "against prepared statistics"
        for mode in (0, 1):
            u8 = wct.stylize_proxy(c, s, D, cell, bins, eps, smooth, alpha=alpha, num_run=runs, u8=True, round_mode=mode)
            assert torch.equal(u8, wct.to_u8(got, mode)) and tuple(u8.shape) == (H, W, 3)
    out = torch.empty(3 * H * W, device="cuda")
    r = wct.stylize_proxy(c, s, D, 8, 4, 1e-3, 0, alpha=0.6, num_run=2, out=out)
    assert r.data_ptr() == out.data_ptr() and torch.equal(r, want)
    y = c.clone()
    assert torch.equal(wct.stylize_proxy(y, s, D, 8, 4, 1e-3, 0, alpha=0.6, num_run=2, out=y.view(-1)), want), "in place over the content"
    assert torch.equal(wct.stylize_proxy(c, s, D), wct.stylize_proxy(c, s, D, _lib.BGRID_CELL, _lib.BGRID_BINS, _lib.BGRID_EPS, _lib.BGRID_SMOOTH))
    assert wct.saturation_count() == 0


def test_second_call_of_a_size_allocates_nothing(torch):
    eng = sc.make_engine("16x")
    c, s = sc.image(1, 256, 272), sc.image(2, 64, 64)
    eng.stylize_proxy(c, s, 2, smooth=4)
    eng.stylize_proxy(c, s, 2, u8=True)
    allocs = eng.debug_get("ws_allocs")
    eng.stylize_proxy(c, s, 2, smooth=4, alpha=0.6, num_run=2)
    eng.stylize_proxy(c, s, 4, bins=4, u8=True, round_mode=1)             # a smaller working size and grid: nothing either
    eng.stylize_proxy(sc.image(3, 128, 192), sc.image(4, 50, 60), 2)
    assert eng.debug_get("ws_allocs") == allocs
    assert eng.saturation_count() == 0


def test_stylize_proxy_is_capturable_into_a_hip_graph():
    """wct_stylize_proxy never synchronises and allocates nothing after the first call of a size: captured after a warm-up, the graph
    replays the eager bits, also with other content bytes in the same buffers.  In a fresh process: a failed capture can leave the
    runtime in capture mode."""
    code = r"""
import sys
sys.path[:0] = [%r, %r]
import torch
from tests import state_cases as sc
wct = sc.make_engine("16x")
c1, c2, s1 = sc.image(1, 128, 192), sc.image(2, 128, 192), sc.image(3, 64, 64)
for u8 in (False, True):
    want1 = wct.stylize_proxy(c1, s1, 2, alpha=0.6, u8=u8).clone()
    want2 = wct.stylize_proxy(c2, s1, 2, alpha=0.6, u8=u8).clone()
    c, s = c1.clone(), s1.clone()
    out = torch.empty(3 * 128 * 192, device="cuda", dtype=torch.uint8 if u8 else torch.float32)
    wct.stylize_proxy(c, s, 2, alpha=0.6, out=out, u8=u8)      # warm-up on the buffers the graph will use
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        wct.stylize_proxy(c, s, 2, alpha=0.6, out=out, u8=u8)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(want1.shape), want1), "u8=%%s: replay 1 differs" %% u8
    c.copy_(c2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(want2.shape), want2), "u8=%%s: replay 2 (new content bytes, same graph) differs" %% u8
assert wct.saturation_count() == 0
print("GRAPH_OK")
""" % (REPO, PKG)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "GRAPH_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------------------- 4. history independence
Case = collections.namedtuple("Case", "fn covers size family")
CASES = collections.OrderedDict()


def case(family, covers):
    def deco(f):
        for size in ("small", "large"):
            CASES["%s/%s" % (family, size)] = Case((lambda eng, seed, _f=f, _s=size: _f(eng, seed, _s)), tuple(covers), size, family)
        return f
    return deco


@case("bgrid_fit", ["wct_bgrid_fit", "wct_bgrid_shape"])
def _bgrid_fit(eng, seed, size):
    H, W = sc.SIZES[size][:2]
    a, b = sc.image(seed, H, W), sc.image(seed + 1, H, W) * 1.3 - 0.1
    gh, gw = eng.bgrid_shape(H, W, 16 if size == "small" else 8)
    return {"default": eng.bgrid_fit(a, b, 8, gh, gw), "global_rows": eng.bgrid_fit(a, b, 3, 1, 2, 1e-4, 0),
            "smooth4": eng.bgrid_fit(a, b, 16, gh, gw, 1e-3, 4)}


@case("bgrid_slice", ["wct_bgrid_slice"])
def _bgrid_slice(eng, seed, size):
    H, W = sc.SIZES[size][:2]
    grid = sc.rand(seed + 2, 8, 5, 7, 3, 4) - 0.3
    fine = sc.rand(seed + 3, 4, 40, 60, 3, 4) - 0.3        # finer than the tiles of the small size: the global-memory path
    c = sc.image(seed, H, W)
    return {"planar": eng.bgrid_slice(grid, c), "u8_floor": eng.bgrid_slice(grid, c, u8=True), "u8_round": eng.bgrid_slice(grid, c, u8=True, round_mode=1),
            "fine": eng.bgrid_slice(fine, c)}


@case("stylize_proxy", ["wct_stylize_proxy"])
def _stylize_proxy(eng, seed, size):
    H, W, Hs, Ws = sc.SIZES[size]
    c, s = sc.image(seed, H, W), sc.image(seed + 1, Hs, Ws)
    return {"plain": eng.stylize_proxy(c, s, 1 if size == "small" else 4), "a06_run2_u8": eng.stylize_proxy(c, s, 2, 8, 4, 1e-3, 2, alpha=0.6, num_run=2, u8=True)}


def run(eng, name, seed=sc.SEED):
    return CASES[name].fn(eng, seed)


PAST = ("stylize/large", "regions/small", "synthesize/small")      # three other families of tests/state_cases.py


def same(torch, got, want, what):
    torch.cuda.synchronize()
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    bad = ["%s: %d of %d values differ" % (k, int((got[k] != want[k]).sum()), want[k].numel()) for k in sorted(want)
           if got[k].shape != want[k].shape or got[k].dtype != want[k].dtype or not torch.equal(got[k], want[k])]
    assert not bad, "%s differs from its control on a fresh engine: %s" % (what, "; ".join(bad))


@pytest.fixture(scope="module")
def controls(torch):
    cache = {}

    def get(name):
        if name not in cache:
            eng = sc.make_engine("16x")
            cache[name] = run(eng, name)
            torch.cuda.synchronize()
            assert eng.saturation_count() == 0
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_history_fresh_engine_against_an_engine_with_a_past(torch, controls, name):
    eng = sc.make_engine("16x")
    for past in PAST:
        sc.run(eng, past)
    same(torch, run(eng, name), controls(name), "%s after %s" % (name, ", ".join(PAST)))
    same(torch, run(eng, name), controls(name), "%s a second time" % name)
    assert eng.saturation_count() == 0


@pytest.mark.parametrize("byte", [0xFF, 0x3C], ids=["ff", "3c"])
@pytest.mark.parametrize("name", list(CASES))
def test_history_poisoned_scratch(torch, controls, name, byte):
    eng = sc.make_engine("16x")
    eng.debug_set("poison", byte)
    same(torch, run(eng, name), controls(name), "%s, poison 0x%02X on a fresh engine" % (name, byte))
    sc.run(eng, "stylize/small")
    eng.debug_set("poison", byte)
    same(torch, run(eng, name), controls(name), "%s, poison 0x%02X again after stylize/small" % (name, byte))
    eng.debug_set("poison", -1)
    assert eng.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 5. errors
def test_refusals_name_the_entry_and_write_nothing(torch, wct):
    L, ctx = wct._lib, wct._ctx
    wct._stream()
    img = torch.rand((3, 64, 80), device="cuda")
    red = torch.rand((3, 32, 40), device="cuda")
    sty = torch.rand((3, 32, 40), device="cuda")
    keep = img.clone()
    G = (4, 3, 4)
    grid = torch.rand((4 * 3 * 4 * 12,), device="cuda")
    gout = torch.full((4 * 3 * 4 * 12,), -3.0, device="cuda")
    outf = torch.full((3 * 64 * 80,), -3.0, device="cuda")
    outb = torch.full((3 * 64 * 80,), 77, device="cuda", dtype=torch.uint8)
    p = lambda x: x.data_ptr()
    inf, nan = float("inf"), float("nan")
    fit = lambda *a: L.wct_bgrid_fit(ctx, *a)
    sl = lambda *a: L.wct_bgrid_slice(ctx, *a)
    px = lambda *a: L.wct_stylize_proxy(ctx, *a)
    MXY, MZ = _lib.BGRID_MAX_XY, _lib.BGRID_MAX_Z
    refusals = [
        ("wct_bgrid_fit", lambda: fit(None, p(sty), 32, 40, *G, 1e-2, 1, p(gout))),
        ("wct_bgrid_fit", lambda: fit(p(red), None, 32, 40, *G, 1e-2, 1, p(gout))),
        ("wct_bgrid_fit", lambda: fit(p(red), p(sty), 32, 40, *G, 1e-2, 1, None)),
        ("wct_bgrid_fit", lambda: fit(p(red), p(sty), 0, 40, *G, 1e-2, 1, p(gout))),
        ("wct_bgrid_fit", lambda: fit(p(red), p(sty), 32, -1, *G, 1e-2, 1, p(gout))),
        ("wct_bgrid_fit", lambda: fit(p(red), p(sty), 32, 40, 0, 3, 4, 1e-2, 1, p(gout))),
        ("wct_bgrid_fit", lambda: fit(p(red), p(sty), 32, 40, 4, 0, 4, 1e-2, 1, p(gout))),
        ("wct_bgrid_fit", lambda: fit(p(red), p(sty), 32, 40, 4, 3, 0, 1e-2, 1, p(gout))),
        ("wct_bgrid_fit", lambda: fit(p(red), p(sty), 32, 40, MZ + 1, 3, 4, 1e-2, 1, p(gout))),
        ("wct_bgrid_fit", lambda: fit(p(red), p(sty), 32, 40, 4, MXY + 1, 4, 1e-2, 1, p(gout))),
        ("wct_bgrid_fit", lambda: fit(p(red), p(sty), 32, 40, 4, 3, MXY + 1, 1e-2, 1, p(gout))),
        ("wct_bgrid_fit", lambda: fit(p(red), p(sty), 32, 40, *G, 0.0, 1, p(gout))),
        ("wct_bgrid_fit", lambda: fit(p(red), p(sty), 32, 40, *G, -1e-2, 1, p(gout))),
        ("wct_bgrid_fit", lambda: fit(p(red), p(sty), 32, 40, *G, inf, 1, p(gout))),
        ("wct_bgrid_fit", lambda: fit(p(red), p(sty), 32, 40, *G, nan, 1, p(gout))),
        ("wct_bgrid_fit", lambda: fit(p(red), p(sty), 32, 40, *G, 1e-2, -1, p(gout))),
        ("wct_bgrid_fit", lambda: fit(p(red), p(sty), 32, 40, *G, 1e-2, _lib.BGRID_MAX_SMOOTH + 1, p(gout))),
        ("wct_bgrid_fit", lambda: fit(p(img), p(sty), 32, 40, *G, 1e-2, 1, p(img) + 4 * 100)),             # the grid lies inside an image
        ("wct_bgrid_slice", lambda: sl(None, *G, p(img), 64, 80, p(outf), None, 0)),
        ("wct_bgrid_slice", lambda: sl(p(grid), *G, None, 64, 80, p(outf), None, 0)),
        ("wct_bgrid_slice", lambda: sl(p(grid), *G, p(img), 64, 80, None, None, 0)),
        ("wct_bgrid_slice", lambda: sl(p(grid), *G, p(img), 64, 80, p(outf), p(outb), 0)),
        ("wct_bgrid_slice", lambda: sl(p(grid), *G, p(img), 0, 80, p(outf), None, 0)),
        ("wct_bgrid_slice", lambda: sl(p(grid), *G, p(img), 64, -2, p(outf), None, 0)),
        ("wct_bgrid_slice", lambda: sl(p(grid), 0, 3, 4, p(img), 64, 80, p(outf), None, 0)),
        ("wct_bgrid_slice", lambda: sl(p(grid), MZ + 1, 3, 4, p(img), 64, 80, p(outf), None, 0)),
        ("wct_bgrid_slice", lambda: sl(p(grid), 4, MXY + 1, 4, p(img), 64, 80, p(outf), None, 0)),
        ("wct_bgrid_slice", lambda: sl(p(grid), 4, 3, -1, p(img), 64, 80, p(outf), None, 0)),
        ("wct_bgrid_slice", lambda: sl(p(grid), *G, p(img), 64, 80, None, p(outb), 2)),
        ("wct_bgrid_slice", lambda: sl(p(grid), *G, p(img), 64, 80, None, p(outb), -1)),
        ("wct_bgrid_slice", lambda: sl(p(grid), *G, p(img), 64, 80, p(img) + 4 * 16, None, 0)),             # shifted over the content it still reads
        ("wct_bgrid_slice", lambda: sl(p(grid), *G, p(img), 64, 80, None, p(img), 0)),                       # bytes over the content
        ("wct_bgrid_slice", lambda: sl(p(outf), *G, p(img), 64, 80, p(outf), None, 0)),                      # the output over the grid
        ("wct_stylize_proxy", lambda: px(None, 64, 80, p(sty), 32, 40, 1.0, 1, 2, 16, 8, 1e-2, 1, p(outf), None, 0)),
        ("wct_stylize_proxy", lambda: px(p(img), 64, 80, p(sty), 32, 40, 1.0, 0, 2, 16, 8, 1e-2, 1, p(outf), None, 0)),
        ("wct_stylize_proxy", lambda: px(p(img), 64, 80, p(sty), 32, 40, 1.0, 1, 2, 16, 8, 1e-2, 1, None, None, 0)),
        ("wct_stylize_proxy", lambda: px(p(img), 64, 80, p(sty), 32, 40, 1.0, 1, 2, 16, 8, 1e-2, 1, p(outf), p(outb), 0)),
        ("wct_stylize_proxy", lambda: px(p(img), 0, 80, p(sty), 32, 40, 1.0, 1, 2, 16, 8, 1e-2, 1, p(outf), None, 0)),
        ("wct_stylize_proxy", lambda: px(p(img), 64, 80, p(sty), 32, 0, 1.0, 1, 2, 16, 8, 1e-2, 1, p(outf), None, 0)),
        ("wct_stylize_proxy", lambda: px(p(img), 64, 80, p(sty), 32, 40, 1.0, 1, 0, 16, 8, 1e-2, 1, p(outf), None, 0)),
        ("wct_stylize_proxy", lambda: px(p(img), 64, 80, p(sty), 32, 40, 1.0, 1, _lib.SCALE_MAX_DIVISOR + 1, 16, 8, 1e-2, 1, p(outf), None, 0)),
        ("wct_stylize_proxy", lambda: px(p(img), 64, 80, p(sty), 32, 40, 1.0, 1, 4, 16, 8, 1e-2, 1, p(outf), None, 0)),        # 64 / 4: under 32
        ("wct_stylize_proxy", lambda: px(p(img), 64, 80, p(sty), 32, 40, 1.0, 1, 2, 0, 8, 1e-2, 1, p(outf), None, 0)),
        ("wct_stylize_proxy", lambda: px(p(img), 64, 80, p(sty), 32, 40, 1.0, 1, 2, 16, 0, 1e-2, 1, p(outf), None, 0)),
        ("wct_stylize_proxy", lambda: px(p(img), 64, 80, p(sty), 32, 40, 1.0, 1, 2, 16, MZ + 1, 1e-2, 1, p(outf), None, 0)),
        ("wct_stylize_proxy", lambda: px(p(img), 64, 80, p(sty), 32, 40, 1.0, 1, 2, 16, 8, 0.0, 1, p(outf), None, 0)),
        ("wct_stylize_proxy", lambda: px(p(img), 64, 80, p(sty), 32, 40, 1.0, 1, 2, 16, 8, nan, 1, p(outf), None, 0)),
        ("wct_stylize_proxy", lambda: px(p(img), 64, 80, p(sty), 32, 40, 1.0, 1, 2, 16, 8, 1e-2, 5, p(outf), None, 0)),
        ("wct_stylize_proxy", lambda: px(p(img), 64, 80, p(sty), 32, 40, 1.0, 1, 2, 16, 8, 1e-2, 1, None, p(outb), 3)),
        ("wct_stylize_proxy", lambda: px(p(img), 64, 80, p(sty), 32, 40, 1.0, 1, 2, 16, 8, 1e-2, 1, p(img) + 4 * 16, None, 0)),
    ]
    for i, (name, call) in enumerate(refusals):
        assert call() == _lib.WCT_ERR_INVALID, (i, name)
        msg = L.wct_last_error(ctx).decode()
        assert name in msg, (i, name, msg)
    torch.cuda.synchronize()
    assert bool((outf == -3.0).all()) and bool((outb == 77).all()) and bool((gout == -3.0).all()) and torch.equal(img, keep)
    gh, gw = ctypes.c_int(-1), ctypes.c_int(-1)
    for h, w, cell in ((0, 40, 16), (32, 0, 16), (32, 40, 0), (256 * 16, 40, 16), (32, 255 * 16 + 1, 16)):
        assert L.wct_bgrid_shape(h, w, cell, ctypes.byref(gh), ctypes.byref(gw)) == _lib.WCT_ERR_INVALID and (gh.value, gw.value) == (-1, -1)
    assert L.wct_bgrid_shape(255 * 16, 1, 16, ctypes.byref(gh), ctypes.byref(gw)) == _lib.WCT_OK and (gh.value, gw.value) == (256, 2)
    # a 1024-wide image of cells of 4 would need 257 vertices: refused by name, through the grid's shape
    wide = torch.rand((3, 32, 1024), device="cuda")
    assert px(p(wide), 32, 1024, p(sty), 32, 40, 1.0, 1, 1, 4, 8, 1e-2, 1, p(outf), None, 0) == _lib.WCT_ERR_INVALID
    assert "wct_stylize_proxy" in L.wct_last_error(ctx).decode()
    # the Python surface refuses the same way
    g5 = grid.view(4, 3, 4, 3, 4)
    with pytest.raises(ValueError, match="gz"):
        wct.bgrid_fit(red, sty, 0, 3, 4)
    with pytest.raises(ValueError, match="eps"):
        wct.bgrid_fit(red, sty, 4, 3, 4, eps=nan)
    with pytest.raises(ValueError, match="smooth"):
        wct.bgrid_fit(red, sty, 4, 3, 4, smooth=5)
    with pytest.raises(ValueError, match="one shape"):
        wct.bgrid_fit(red, img, 4, 3, 4)
    with pytest.raises(ValueError, match="grid"):
        wct.bgrid_slice(grid, img)
    with pytest.raises(ValueError):
        wct.bgrid_slice(g5, img, out=torch.empty(5, device="cuda"))
    with pytest.raises(ValueError, match="divisor"):
        wct.stylize_proxy(img, sty, 17)
    with pytest.raises(ValueError, match="scale_shape"):
        wct.stylize_proxy(img, sty, 4)
    with pytest.raises(ValueError, match="gz"):
        wct.stylize_proxy(img, sty, 2, bins=33)
    fresh = sc.make_engine("16x")
    with pytest.raises(_lib.WctError, match="wct_stylize_proxy: no style statistics"):
        fresh.stylize_proxy(img, None, 2)
    # the largest grid axes are served
    big = wct.bgrid_fit(red, sty, MZ, 2, MXY)
    assert bool(torch.isfinite(big).all()) and bool(torch.isfinite(wct.bgrid_slice(big, img)).all())
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 6. command line
def test_cli_proxy_scale(torch, tmp_path):
    """Two contents x one style: --proxy_scale 2 writes files of the contents' exact sizes under the _proxy=2 names, byte-identical
    to the engine call saved through the same Pillow call."""
    Image = pytest.importorskip("PIL.Image")
    from wct_hip import WCT, cli
    c, s = tmp_path / "content", tmp_path / "style"
    c.mkdir(); s.mkdir()
    shapes = {"c1.png": (131, 197), "c2.png": (160, 138), "s1.png": (90, 100)}
    for i, (n, (h, w)) in enumerate(shapes.items()):
        img = (CO.natural(70 + i, h, w, cast=(1.0, 0.7, 0.5) if i % 2 else (0.5, 0.9, 1.0)) * 255).astype(np.uint8).transpose(1, 2, 0)
        Image.fromarray(np.ascontiguousarray(img)).save((c if n[0] == "c" else s) / n)

    def run_cli(tag, *extra):
        o = tmp_path / tag
        assert cli.main(["--mode", "16x", "--contentPath", str(c), "--stylePath", str(s), "--outf", str(o), "--log_mark", "C", "--alpha", "0.8"]
                        + list(extra)) == 0
        return {f: (o / f).read_bytes() for f in sorted(os.listdir(o)) if f.endswith(".jpg")}

    w = WCT(types.SimpleNamespace(mode="16x", alpha=0.8))
    sf = w.to_tensor_u8(torch.from_numpy(cli.load_rgb_u8(str(s / "s1.png"))).cuda())

    def refs(mark, **kw):
        out = {}
        for a in ("c1", "c2"):
            cf = w.to_tensor_u8(torch.from_numpy(cli.load_rgb_u8(str(c / (a + ".png")))).cuda())
            u8 = w.stylize_proxy(cf, sf, 2, alpha=0.8, u8=True, **kw)
            assert tuple(u8.shape) == shapes[a + ".png"] + (3,)
            Image.fromarray(u8.cpu().numpy()).save(tmp_path / "ref.jpg")
            out["C_mode=16x_alpha=0.8%s_%s+s1.jpg" % (mark, a)] = (tmp_path / "ref.jpg").read_bytes()
        return out

    got = run_cli("proxy", "--proxy_scale", "2")
    assert got == refs("_proxy=2")
    for f in got:
        with Image.open(tmp_path / "proxy" / f) as im:
            assert im.size[::-1] == shapes[f.split("_")[-1].split("+")[0] + ".png"], "the saved image has the content's H x W"
    got = run_cli("params", "--proxy_scale", "2", "--proxy_cell", "8", "--proxy_bins", "4", "--proxy_eps", "1e-3", "--proxy_smooth", "0", "--round", "1",
                  "--pipeline", "3")
    assert got == refs("_proxy=2", cell=8, bins=4, eps=1e-3, smooth=0, round_mode=1)
    with pytest.raises(ValueError, match="--proxy_scale does not mix with --smooth_radius"):
        run_cli("refused", "--proxy_scale", "2", "--smooth_radius", "8")
    assert not (tmp_path / "refused").exists()
