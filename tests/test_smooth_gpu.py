"""Guided-filter smoothing on the device (include/wct_hip_smooth.h): wct_guided_filter against the numpy fp64 reference
(tests/smooth_oracle.py) under the project's fp64 gate, its bitwise properties, wct_stylize_smooth against the public calls it is made
of (bit for bit), allocation and graph capture, history independence of both entries with the helpers of tests/state_cases.py, the
refusals, and the command line's --smooth_radius.

The module imports without a GPU: tests/test_smooth_cpu.py reads CASES and SHAPES."""
import collections
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from tests import color_oracle as CO
from tests import smooth_oracle as O
from tests import state_cases as sc
from tests.conftest import PKG, REPO
from wct_hip import lib as _lib

pytestmark = pytest.mark.gpu

GATE = 2e-5          # the project's fp64 gate (decision record G.1, tests/test_geometry_gpu.py), absolute


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


def pair(Ho, Wo, Hg=None, Wg=None):
    """(source 3 x Ho x Wo in about [-0.2, 1.3], guide 3 x Hg x Wg in [0, 1]): natural-like, 8-bit-quantised, seeded by the shape."""
    Hg, Wg = Hg or Ho, Wg or Wo
    guide = q8(CO.natural(Hg * 7 + Wg, Hg, Wg))
    src = q8(CO.natural(Ho * 13 + Wo + 1, Ho, Wo, cast=(0.6, 1.0, 0.9), shift=(0.2, 0.0, 0.1)).astype(np.float64) * 1.5 - 0.2)
    return src, guide


# (Ho, Wo, r, eps, guide shape or None, why).  The first eleven are the base set; the rest sit one below, at and one above every
# restart or tile edge of the launchers (smooth.hip).
SHAPES = [
    (1, 1, 1, 1e-4, None, "a single pixel"),
    (1, 2, 1, 1e-4, None, "a single row"),
    (5, 7, 9, 1e-4, None, "radius larger than the image"),
    (33, 65, 4, 1e-4, None, "odd sizes, one column past a 64-column chunk"),
    (64, 64, 1, 1e-4, None, "the smallest radius"),
    (250, 333, 35, 1e-4, None, "a photograph's size"),
    (272, 400, 16, 1e-4, (277, 410), "cut from a larger guide"),
    (600, 900, 60, 1e-4, None, "large radius"),
    (600, 900, 8, 1e-6, None, "small radius, tiny eps: the cancellation case"),
    (1100, 70, 200, 1e-4, None, "tall and narrow"),
    (70, 1100, 200, 1e-4, None, "wide and flat"),
    (127, 70, 8, 1e-4, None, "one row below the 128-row vertical restart"),
    (128, 70, 8, 1e-4, None, "exactly one vertical segment of 128 rows"),
    (129, 70, 8, 1e-4, None, "one row into a second vertical segment"),
    (131, 40, 33, 1e-4, None, "r = 33: segments of 4 r = 132 rows, one row below"),
    (132, 40, 33, 1e-4, None, "r = 33: exactly one segment of 132 rows"),
    (133, 40, 33, 1e-4, None, "r = 33: one row into a second segment of 132"),
    (2047, 8, 600, 1e-4, None, "r = 600: segments capped at 2048 rows, one row below"),
    (2048, 8, 600, 1e-4, None, "r = 600: exactly one capped segment"),
    (2049, 8, 600, 1e-4, None, "r = 600: one row into a second capped segment"),
    (9, 63, 4, 1e-4, None, "one column below the 64-column chunk / vertical workgroup"),
    (9, 64, 4, 1e-4, None, "exactly one 64-column chunk"),
    (9, 65, 4, 1e-4, None, "one column into a second chunk"),
    (3, 4095, 5, 1e-4, None, "one column below the 4096-column horizontal restart"),
    (3, 4096, 5, 1e-4, None, "exactly one horizontal segment"),
    (3, 4097, 5, 1e-4, None, "one column into a second horizontal segment"),
    (6, 4200, 300, 1e-4, None, "a horizontal restart whose first window spans ten chunks"),
    (5, 7, 2048, 1e-4, None, "the largest radius the header allows"),
    (128, 100, 1, 1e-4, None, "ragged last chunk, r < 62, and 168 Ho Wo a multiple of 4096: nothing behind the window sums to read"),
]
RAGGED = SHAPES[-1]

_REF = {}


def reference(Ho, Wo, r, eps, gshape):
    """The oracle's result of a SHAPES case, computed once and shared (read-only)."""
    key = (Ho, Wo, r, eps, gshape)
    if key not in _REF:
        src, guide = pair(Ho, Wo, *(gshape or (None, None)))
        ref = O.guided_filter(src, guide, r, eps)
        ref.setflags(write=False)
        _REF[key] = (src, guide, ref)
    return _REF[key]


# ---------------------------------------------------------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("Ho,Wo,r,eps,gshape,why", SHAPES, ids=["%dx%d-r%d-eps%g" % s[:4] for s in SHAPES])
def test_guided_filter_against_the_oracle(torch, wct, Ho, Wo, r, eps, gshape, why):
    src, guide, ref = reference(Ho, Wo, r, eps, gshape)
    got = wct.guided_filter(cu(torch, src), cu(torch, guide), r, eps)
    assert tuple(got.shape) == (1, 3, Ho, Wo)
    g = got.cpu().numpy()[0].astype(np.float64)
    err = float(np.abs(g - ref).max())
    print("guided_filter %dx%d r=%d eps=%g (%s): max abs err vs fp64 %.3e" % (Ho, Wo, r, eps, why, err))
    assert np.isfinite(g).all()
    assert err <= GATE, (Ho, Wo, r, eps, err)


def test_ragged_last_chunk_on_a_fresh_context(torch):
    """The lanes of a row's last 64-column chunk that lie past the row's end must load nothing: with 168 Ho Wo a multiple of 4096 the
    21 planes of window sums of a fresh context end on a page boundary, so a load behind them would leave the allocation.  Both
    outputs, first call of the context, against the oracle and the warm context's bits."""
    Ho, Wo, r, eps, gshape, _ = RAGGED
    assert (168 * Ho * Wo) % 4096 == 0 and Wo % 64 and r < 62
    src, guide, ref = reference(Ho, Wo, r, eps, gshape)
    got = sc.make_engine("16x").guided_filter(cu(torch, src), cu(torch, guide), r, eps)
    u8 = sc.make_engine("16x").guided_filter(cu(torch, src), cu(torch, guide), r, eps, u8=True)
    torch.cuda.synchronize()
    err = float(np.abs(got.cpu().numpy()[0].astype(np.float64) - ref).max())
    print("guided_filter %dx%d r=%d on a fresh context: max abs err vs fp64 %.3e" % (Ho, Wo, r, err))
    assert err <= GATE
    assert np.array_equal(u8.cpu().numpy(), CO.to_u8(got.cpu().numpy()[0], 0))


# ---------------------------------------------------------------------------------------------------------------- 2. bitwise properties
@pytest.mark.parametrize("Ho,Wo,r,gshape", [(33, 65, 4, None), (250, 333, 35, None), (272, 400, 16, (277, 410)), (3, 4097, 5, None)])
def test_bitwise_properties(torch, wct, Ho, Wo, r, gshape):
    src, guide = pair(Ho, Wo, *(gshape or (None, None)))
    xs, xg = cu(torch, src), cu(torch, guide)
    got = wct.guided_filter(xs, xg, r, 1e-4)
    assert torch.equal(wct.guided_filter(xs, xg, r, 1e-4), got), "two calls differ"
    for off in (0, 1, 2, 3):
        out = offset_view(torch, torch.zeros_like(xs), off)
        back = wct.guided_filter(offset_view(torch, xs, off), offset_view(torch, xg, (off + 1) % 4 if off else 0), r, 1e-4, out=out.view(-1))
        assert back.data_ptr() == out.data_ptr() and torch.equal(back, got), "views %d floats off a 16-byte boundary filter differently" % off
    assert torch.equal(sc.make_engine("16x").guided_filter(xs, xg, r, 1e-4), got), "two contexts differ"
    y = xs.clone()
    back = wct.guided_filter(y, xg, r, 1e-4, out=y)
    assert back.data_ptr() == y.data_ptr() and torch.equal(y, got[0]), "in place over the source differs from out of place"
    assert torch.equal(xg, cu(torch, guide)), "the guide was written"
    for mode in (0, 1):
        bigb = torch.full((3 * Ho * Wo + 8,), 201, device="cuda", dtype=torch.uint8)
        u8 = wct.guided_filter(xs, xg, r, 1e-4, out=bigb[1: 1 + 3 * Ho * Wo], u8=True, round_mode=mode)      # an odd base address
        assert u8.data_ptr() % 2 == 1 and u8.dtype == torch.uint8 and tuple(u8.shape) == (Ho, Wo, 3)
        assert torch.equal(u8, wct.to_u8(got, mode)), "fused uint8 output differs from to_u8 of the planar output (round_mode %d)" % mode
        assert np.array_equal(u8.cpu().numpy(), CO.to_u8(got.cpu().numpy()[0], mode))
        assert bool((bigb[:1] == 201).all()) and bool((bigb[1 + 3 * Ho * Wo:] == 201).all())
        assert torch.equal(wct.guided_filter(xs, xg, r, 1e-4, u8=True, round_mode=mode), u8)
    big = torch.full((3 * Ho * Wo + 8,), -7.0, device="cuda")
    wct.guided_filter(xs, xg, r, 1e-4, out=big[4: 4 + 3 * Ho * Wo])
    assert torch.equal(big[4: 4 + 3 * Ho * Wo].view(1, 3, Ho, Wo), got) and bool((big[:4] == -7.0).all()) and bool((big[-4:] == -7.0).all())


@pytest.mark.parametrize("Ho,Wo,r", [(33, 65, 4), (250, 333, 35)])
def test_constant_source_comes_back(torch, wct, Ho, Wo, r):
    _, guide = pair(Ho, Wo)
    const = np.broadcast_to(np.array([0.25, -0.125, 1.25], np.float32)[:, None, None], (3, Ho, Wo)).copy()
    got = wct.guided_filter(cu(torch, const), cu(torch, guide), r, 1e-4).cpu().numpy()[0]
    err = float(np.abs(got.astype(np.float64) - const).max())
    print("guided_filter of a constant source %dx%d r=%d: max deviation %.3e" % (Ho, Wo, r, err))
    assert err <= 1e-6


# ---------------------------------------------------------------------------------------------------------------- 3. the cascade
COLORS = (None, "luma", "match+luma")


def compose(w, c, s, radius, eps, color, alpha, runs):
    """wct_stylize_smooth spelled out in public calls."""
    st = w.color_match(s, c) if color and "match" in color else s
    res = w.stylize(c, st, alpha=alpha, num_run=runs).clone()
    res = w.guided_filter(res, c, radius, eps)
    return w.luma_merge(res, c) if color and "luma" in color else res


@pytest.mark.parametrize("H,W,Hs,Ws,transform", [
    pytest.param(250, 333, 200, 160, "wct", id="250-333-200-160"), pytest.param(272, 400, 210, 300, "wct", id="272-400-210-300"),
    pytest.param(250, 333, 200, 160, "ot", id="250-333-200-160-ot"), pytest.param(250, 333, 200, 160, "adain", id="250-333-200-160-adain")])
def test_stylize_smooth_is_the_composition_of_the_public_calls(torch, wct, H, W, Hs, Ws, transform):
    """Under ot and adain (include/wct_hip_transform.h: the composed entries follow the context's mode) the same identities, on an
    engine of that mode."""
    c = cu(torch, CO.natural(H, H, W))[None]
    s = cu(torch, CO.natural(W, Hs, Ws, cast=(0.5, 1.0, 0.9), shift=(0.3, 0.0, 0.1)))[None]
    if transform != "wct":
        under_wct = wct.stylize(c, s, alpha=0.6).clone()
        wct = sc.make_engine("16x")
        wct.set_transform(transform)
        assert not torch.equal(wct.stylize(c, s, alpha=0.6), under_wct)          # the mode took effect
    for alpha, runs in ((1.0, 1), (0.6, 1), (0.6, 2)):
        plain = wct.stylize(c, s, alpha=alpha, num_run=runs).clone()
        for color in COLORS:
            want = compose(wct, c, s, 8, 1e-3, color, alpha, runs)
            got = wct.stylize_smooth(c, s, 8, 1e-3, color=color, alpha=alpha, num_run=runs)
            assert tuple(got.shape) == (1, 3, H // 16 * 16, W // 16 * 16)
            assert torch.equal(got, want), (color, alpha, runs)
            assert not torch.equal(got, plain)
    out = torch.empty((3, H, W), device="cuda")
    r = wct.stylize_smooth(c, s, 8, 1e-3, color="match+luma", alpha=0.6, num_run=2, out=out)
    assert r.data_ptr() == out.data_ptr() and torch.equal(r, want)
    assert torch.equal(wct.stylize_smooth(c, s, 8), wct.stylize_smooth(c, s, 8, _lib.SMOOTH_EPS)), "the default eps is WCT_SMOOTH_EPS"
    with pytest.raises(ValueError, match="color"):
        wct.stylize_smooth(c, s, 8, color="chroma")
    assert wct.saturation_count() == 0


def test_second_call_of_a_size_allocates_nothing(torch):
    eng = sc.make_engine("16x")
    c, s = sc.image(1, 250, 333), sc.image(2, 200, 160)
    for color in COLORS + ("match",):
        eng.stylize_smooth(c, s, 8, color=color)
    eng.guided_filter(c[:, :, :240, :320], c, 8, u8=True)
    allocs = eng.debug_get("ws_allocs")
    for color in COLORS + ("match",):
        eng.stylize_smooth(c, s, 30, 1e-4, color=color, alpha=0.6, num_run=2)
    eng.stylize_smooth(sc.image(3, 120, 200), sc.image(4, 90, 100), 8, color="match+luma")          # smaller: nothing either
    eng.guided_filter(c[:, :, :240, :320], c, 8, u8=True), eng.guided_filter(c, c, 3)
    assert eng.debug_get("ws_allocs") == allocs
    assert eng.saturation_count() == 0


def test_stylize_smooth_is_capturable_into_a_hip_graph():
    """wct_stylize_smooth never synchronises and allocates nothing after the first call of a size: captured after a warm-up, the graph
    replays the eager bits, also with other images in the same buffers.  In a fresh process: a failed capture can leave the runtime in
    capture mode."""
    code = r"""
import sys
sys.path[:0] = [%r, %r]
import torch
from tests import state_cases as sc
wct = sc.make_engine("16x")
c1, c2, s1, s2 = sc.image(1, 272, 400), sc.image(2, 272, 400), sc.image(3, 200, 240), sc.image(4, 200, 240)
for color in (None, "luma", "match+luma"):
    want1 = wct.stylize_smooth(c1, s1, 8, 1e-3, color=color, alpha=0.6).clone()
    want2 = wct.stylize_smooth(c2, s2, 8, 1e-3, color=color, alpha=0.6).clone()
    c, s = c1.clone(), s1.clone()
    out = torch.empty((3, 272, 400), device="cuda")
    wct.stylize_smooth(c, s, 8, 1e-3, color=color, alpha=0.6, out=out)      # warm-up on the buffers the graph will use
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        wct.stylize_smooth(c, s, 8, 1e-3, color=color, alpha=0.6, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(1, 3, 272, 400), want1), str(color) + ": replay 1 differs"
    c.copy_(c2); s.copy_(s2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(1, 3, 272, 400), want2), str(color) + ": replay 2 (new images, same graph) differs"
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


@case("guided_filter", ["wct_guided_filter"])
def _guided_filter(eng, seed, size):
    H, W = sc.SIZES[size][:2]
    g, s = sc.image(seed, H, W), sc.image(seed + 1, H // 16 * 16, W // 16 * 16) * 1.4 - 0.2
    r = 6 if size == "small" else 40
    return {"planar": eng.guided_filter(s, g, r, 1e-4), "u8_floor": eng.guided_filter(s, g, r, 1e-4, u8=True),
            "u8_round": eng.guided_filter(s, g, r, 1e-2, u8=True, round_mode=1)}


@case("stylize_smooth", ["wct_stylize_smooth"])
def _stylize_smooth(eng, seed, size):
    H, W, Hs, Ws = sc.SIZES[size]
    c, s = sc.image(seed, H, W), sc.image(seed + 1, Hs, Ws)
    return {"plain": eng.stylize_smooth(c, s, 8), "luma_a06_run2": eng.stylize_smooth(c, s, 12, 1e-4, color="luma", alpha=0.6, num_run=2),
            "both": eng.stylize_smooth(c, s, 5, color="match+luma", alpha=0.8)}


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
    img = torch.rand((3, 40, 48), device="cuda")
    src = torch.rand((3, 32, 32), device="cuda")
    keep_img = img.clone()
    outf = torch.full((3 * 40 * 48,), -3.0, device="cuda")
    outb = torch.full((3 * 40 * 48,), 77, device="cuda", dtype=torch.uint8)
    p = lambda x: x.data_ptr()
    ho, wo = ctypes.c_int(-1), ctypes.c_int(-1)
    inf, nan = float("inf"), float("nan")
    gf = lambda *a: L.wct_guided_filter(ctx, *a)
    ss = lambda *a: L.wct_stylize_smooth(ctx, *a, ctypes.byref(ho), ctypes.byref(wo))
    refusals = [
        ("wct_guided_filter", lambda: gf(None, 32, 32, p(img), 40, 48, 4, 1e-3, p(outf), None, 0)),
        ("wct_guided_filter", lambda: gf(p(src), 32, 32, None, 40, 48, 4, 1e-3, p(outf), None, 0)),
        ("wct_guided_filter", lambda: gf(p(src), 32, 32, p(img), 40, 48, 4, 1e-3, None, None, 0)),
        ("wct_guided_filter", lambda: gf(p(src), 32, 32, p(img), 40, 48, 4, 1e-3, p(outf), p(outb), 0)),
        ("wct_guided_filter", lambda: gf(p(src), 0, 32, p(img), 40, 48, 4, 1e-3, p(outf), None, 0)),
        ("wct_guided_filter", lambda: gf(p(src), 32, -1, p(img), 40, 48, 4, 1e-3, p(outf), None, 0)),
        ("wct_guided_filter", lambda: gf(p(img), 40, 48, p(src), 32, 32, 4, 1e-3, p(outf), None, 0)),        # Ho > Hg
        ("wct_guided_filter", lambda: gf(p(img), 32, 48, p(img), 40, 32, 4, 1e-3, p(outf), None, 0)),        # Wo > Wg
        ("wct_guided_filter", lambda: gf(p(src), 32, 32, p(img), 40, 48, 0, 1e-3, p(outf), None, 0)),
        ("wct_guided_filter", lambda: gf(p(src), 32, 32, p(img), 40, 48, -3, 1e-3, p(outf), None, 0)),
        ("wct_guided_filter", lambda: gf(p(src), 32, 32, p(img), 40, 48, _lib.SMOOTH_MAX_RADIUS + 1, 1e-3, p(outf), None, 0)),
        ("wct_guided_filter", lambda: gf(p(src), 32, 32, p(img), 40, 48, 4, 0.0, p(outf), None, 0)),
        ("wct_guided_filter", lambda: gf(p(src), 32, 32, p(img), 40, 48, 4, -1e-3, p(outf), None, 0)),
        ("wct_guided_filter", lambda: gf(p(src), 32, 32, p(img), 40, 48, 4, inf, p(outf), None, 0)),
        ("wct_guided_filter", lambda: gf(p(src), 32, 32, p(img), 40, 48, 4, nan, p(outf), None, 0)),
        ("wct_guided_filter", lambda: gf(p(src), 32, 32, p(img), 40, 48, 4, 1e-3, None, p(outb), 2)),
        ("wct_guided_filter", lambda: gf(p(src), 32, 32, p(img), 40, 48, 4, 1e-3, p(img), None, 0)),         # the output is the guide
        ("wct_guided_filter", lambda: gf(p(src), 32, 32, p(img), 40, 48, 4, 1e-3, p(img) + 4 * 3000, None, 0)),   # ... or lies inside it
        ("wct_stylize_smooth", lambda: ss(None, 40, 48, p(src), 32, 32, 1.0, 1, 0, 4, 1e-3, p(outf))),
        ("wct_stylize_smooth", lambda: ss(p(img), 40, 48, None, 32, 32, 1.0, 1, 0, 4, 1e-3, p(outf))),
        ("wct_stylize_smooth", lambda: ss(p(img), 40, 48, p(src), 32, 32, 1.0, 1, 0, 4, 1e-3, None)),
        ("wct_stylize_smooth", lambda: ss(p(img), 40, 48, p(src), 32, 32, 1.0, 0, 0, 4, 1e-3, p(outf))),
        ("wct_stylize_smooth", lambda: ss(p(img), 40, 48, p(src), 32, 32, 1.0, 1, 4, 4, 1e-3, p(outf))),
        ("wct_stylize_smooth", lambda: ss(p(img), 40, 48, p(src), 32, 32, 1.0, 1, -1, 4, 1e-3, p(outf))),
        ("wct_stylize_smooth", lambda: ss(p(img), 0, 48, p(src), 32, 32, 1.0, 1, 0, 4, 1e-3, p(outf))),
        ("wct_stylize_smooth", lambda: ss(p(img), 40, 48, p(src), 32, 0, 1.0, 1, 2, 4, 1e-3, p(outf))),
        ("wct_stylize_smooth", lambda: ss(p(img), 40, 48, p(src), 1, 1, 1.0, 1, 1, 4, 1e-3, p(outf))),      # MATCH needs two style pixels
        ("wct_stylize_smooth", lambda: ss(p(img), 40, 48, p(src), 32, 32, 1.0, 1, 0, 0, 1e-3, p(outf))),
        ("wct_stylize_smooth", lambda: ss(p(img), 40, 48, p(src), 32, 32, 1.0, 1, 3, _lib.SMOOTH_MAX_RADIUS + 1, 1e-3, p(outf))),
        ("wct_stylize_smooth", lambda: ss(p(img), 40, 48, p(src), 32, 32, 1.0, 1, 0, 4, 0.0, p(outf))),
        ("wct_stylize_smooth", lambda: ss(p(img), 40, 48, p(src), 32, 32, 1.0, 1, 2, 4, nan, p(outf))),
        ("wct_stylize_smooth", lambda: ss(p(img), 40, 48, p(src), 32, 32, 1.0, 1, 0, 4, 1e-3, p(img))),       # out is the guide
    ]
    for i, (name, call) in enumerate(refusals):
        assert call() == _lib.WCT_ERR_INVALID, (i, name)
        msg = L.wct_last_error(ctx).decode()
        assert name in msg, (i, name, msg)
    torch.cuda.synchronize()
    assert bool((outf == -3.0).all()) and bool((outb == 77).all()) and (ho.value, wo.value) == (-1, -1) and torch.equal(img, keep_img)
    # the Python surface refuses the same way
    with pytest.raises(ValueError):
        wct.guided_filter(img, src, 4)
    with pytest.raises(ValueError, match="radius"):
        wct.guided_filter(src, img, 0)
    with pytest.raises(ValueError, match="radius"):
        wct.guided_filter(src, img, 2.5)
    with pytest.raises(ValueError, match="eps"):
        wct.guided_filter(src, img, 4, eps=0.0)
    with pytest.raises(ValueError, match="eps"):
        wct.stylize_smooth(img, src, 4, eps=nan)
    with pytest.raises(ValueError):
        wct.guided_filter(src, img, 4, out=torch.empty(5, device="cuda"))
    # the largest radius is served
    assert bool(torch.isfinite(wct.guided_filter(src, img, _lib.SMOOTH_MAX_RADIUS)).all())
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 6. command line
def test_cli_smooth_radius(torch, tmp_path):
    """Two contents x one style of ~300 x 400: --smooth_radius 8 writes the same bytes with --pipeline 0 and --pipeline 3 under names
    that carry _smooth=8, alone and with --preserve_color luma; the files are those of the test's own library calls saved through the
    same Pillow call; without the flag names and bytes are the plain run's; --synthesis refuses the flag."""
    Image = pytest.importorskip("PIL.Image")
    from wct_hip import WCT, cli
    c, s = tmp_path / "content", tmp_path / "style"
    c.mkdir(); s.mkdir()
    shapes = {"c1.png": (300, 400), "c2.png": (288, 410), "s1.png": (310, 390)}
    for i, (n, (h, w)) in enumerate(shapes.items()):
        img = (CO.natural(70 + i, h, w, cast=(1.0, 0.7, 0.5) if i % 2 else (0.5, 0.9, 1.0)) * 255).astype(np.uint8).transpose(1, 2, 0)
        Image.fromarray(np.ascontiguousarray(img)).save((c if n[0] == "c" else s) / n)

    def run_cli(tag, *extra):
        o = tmp_path / tag
        assert cli.main(["--mode", "16x", "--contentPath", str(c), "--stylePath", str(s), "--outf", str(o), "--log_mark", "C", "--alpha", "0.8",
                         "--io_threads", "3"] + list(extra)) == 0
        return {f: (o / f).read_bytes() for f in sorted(os.listdir(o)) if f.endswith(".jpg")}

    w = WCT(types.SimpleNamespace(mode="16x", alpha=0.8))
    sf = w.to_tensor_u8(torch.from_numpy(cli.load_rgb_u8(str(s / "s1.png"))).cuda())

    def saved(u8):
        Image.fromarray(u8.cpu().numpy()).save(tmp_path / "ref.jpg")
        return (tmp_path / "ref.jpg").read_bytes()

    def refs(mark, finish):
        out = {}
        for a in ("c1", "c2"):
            cf = w.to_tensor_u8(torch.from_numpy(cli.load_rgb_u8(str(c / (a + ".png")))).cuda())
            w.style_prepare(sf)
            out["C_mode=16x_alpha=0.8%s_%s+s1.jpg" % (mark, a)] = saved(finish(w.stylize_prepared(cf, alpha=0.8).clone(), cf))
        return out

    plain = run_cli("plain", "--pipeline", "0")
    assert plain == refs("", lambda res, cf: w.to_u8(res, 0)), "without the flag: the plain run's names and bytes"
    smooth = run_cli("smooth_serial", "--pipeline", "0", "--smooth_radius", "8")
    assert smooth == run_cli("smooth_pipe", "--pipeline", "3", "--smooth_radius", "8")
    assert smooth == refs("_smooth=8", lambda res, cf: w.to_u8(w.guided_filter(res, cf, 8, 1e-3), 0))
    assert all(smooth[k] != plain[k.replace("_smooth=8", "")] for k in smooth)
    luma = run_cli("luma_serial", "--pipeline", "0", "--smooth_radius", "8", "--preserve_color", "luma", "--smooth_eps", "1e-2")
    assert luma == run_cli("luma_pipe", "--pipeline", "3", "--smooth_radius", "8", "--preserve_color", "luma", "--smooth_eps", "1e-2")
    assert luma == refs("_color=luma_smooth=8", lambda res, cf: w.to_u8(w.luma_merge(w.guided_filter(res, cf, 8, 1e-2), cf), 0))
    with pytest.raises(ValueError, match="--smooth_radius does not mix with --synthesis"):
        run_cli("refused", "--synthesis", "--smooth_radius", "8")
    assert not (tmp_path / "refused").exists()
