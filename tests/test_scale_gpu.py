"""Scale control on the device (include/wct_hip_scale.h): wct_resample_planar and wct_pyramid_merge against the numpy fp64 reference
(tests/scale_oracle.py) inside the first-order bounds of their fp32 sums, their bitwise properties, and wct_stylize_scaled against the
composition of public calls written out here -- bit for bit -- with its allocation, poison, range, graph and refusal behaviour."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from tests import scale_oracle as O
from tests import state_cases as sc
from tests.conftest import PKG, REPO
from wct_hip import lib as _lib

pytestmark = pytest.mark.gpu
FILTERS = [O.BILINEAR, O.BICUBIC]
STYLE = (84, 108)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "-m gpu tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def wct(torch):
    return sc.make_engine("16x")


def cu(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def shape_id(v):
    return "x".join(str(t) for t in v) if isinstance(v, tuple) else str(v)


# ---------------------------------------------------------------------------------------------------------------- 1. R against fp64
@pytest.mark.parametrize("name", FILTERS)
@pytest.mark.parametrize("src,dst", O.RESAMPLE_SHAPES, ids=shape_id)
def test_resample_against_fp64(torch, wct, src, dst, name):
    """(n_h + n_v + 4) u A_h A_v max|x|.  The shapes: tests/scale_oracle.py RESAMPLE_SHAPES -- the issue's six, output sizes one below, at
    and one above the kernel's 64 x 16 tile (and its 32-column tile for widths shrinking by more than 8), and a height whose tile halves."""
    x = O.image(src, 5)
    got = wct.resample(cu(torch, x)[None], dst, name)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (1, 3) + tuple(dst)
    want = O.resample(x, dst[0], dst[1], name)
    bound = O.resample_bound(src, dst[0], dst[1], name, float(np.abs(x).max()))
    dist = float(np.abs(got[0].cpu().numpy().astype(np.float64) - want).max())
    print("resample %s %s->%s: distance %.3g, bound %.3g" % (name, src, dst, dist, bound))
    assert dist <= bound
    assert wct.saturation_count() == 0


@pytest.mark.parametrize("name", FILTERS)
def test_equal_sizes_are_a_copy_and_results_do_not_depend_on_call_context_or_alignment(torch, wct, name):
    x = cu(torch, O.image((37, 53), 8))
    x[1, 4, 7], x[2, 0, 0] = -0.0, 3e38
    same = wct.resample(x[None], (37, 53), name)
    assert torch.equal(same[0], x) and torch.equal(same[0].view(torch.int32), x.view(torch.int32))
    other = sc.make_engine("16x")
    for src, dst in (((131, 257), (16, 32)), ((16, 32), (131, 257)), ((40, 150), (O.TILE_H + 1, O.TILE_W + 1))):
        img = cu(torch, O.image(src, 9))[None]
        first = wct.resample(img, dst, name).clone()
        wct.resample(cu(torch, O.image((50, 70), 1))[None], (20, 90), name)                     # something else in between
        assert torch.equal(wct.resample(img, dst, name), first), (src, dst, "second call")
        assert torch.equal(other.resample(img, dst, name), first), (src, dst, "second context")
        # source and destination at a 4-byte-only alignment: views one, two and three floats into a buffer
        for shift in (1, 2, 3):
            n_in, n_out = 3 * src[0] * src[1], 3 * dst[0] * dst[1]
            big_in = torch.zeros(n_in + 4, device="cuda")
            big_in[shift:shift + n_in] = img.reshape(-1)
            big_out = torch.full((n_out + 8,), -7.0, device="cuda")
            view = big_out[shift:shift + n_out]
            assert view.data_ptr() % 16 == 4 * shift
            r = wct.resample(big_in[shift:shift + n_in].view(1, 3, *src), dst, name, out=view)
            assert r.data_ptr() == view.data_ptr() and torch.equal(r, first), (src, dst, shift)
            assert bool((big_out[:shift] == -7.0).all()) and bool((big_out[shift + n_out:] == -7.0).all())     # nothing past either end
    torch.cuda.synchronize()
    assert wct.saturation_count() == 0 and other.saturation_count() == 0


def test_profile_families(torch, wct):
    img = cu(torch, O.image((96, 128), 2))[None]
    small = cu(torch, O.image((48, 64), 3))[None]
    wct.profile(True)
    wct.profile_reset()
    wct.resample(img, (48, 64), "bicubic")
    wct.resample(small, (96, 128), "bicubic")
    wct.resample(img, (40, 60), "bilinear")
    wct.pyramid_merge(small, small, img, 1.0)
    recs = {r["name"]: r for r in wct.profile_read()}
    wct.profile(False)
    assert set(recs) == {"resample<bicubic,down>", "resample<bicubic,up>", "resample<bilinear,down>", "pyramid_merge"}
    assert recs["resample<bicubic,down>"]["bytes"] == 12.0 * (96 * 128 + 48 * 64) and recs["resample<bicubic,down>"]["launches"] == 1
    assert recs["pyramid_merge"]["bytes"] == 12.0 * (2 * 48 * 64 + 2 * 96 * 128)


# ---------------------------------------------------------------------------------------------------------------- 2. M against fp64
@pytest.mark.parametrize("gain", [0.75, 1.0])
@pytest.mark.parametrize("coarse,fine", O.MERGE_SHAPES, ids=shape_id)
def test_merge_against_fp64(torch, wct, coarse, fine, gain):
    """(n_h + n_v + 6) u A_h A_v (max|a| + g max|b|) + 2 u g max|c|"""
    a, b, c = O.image(coarse, 21), O.image(coarse, 22), O.image(fine, 23)
    got = wct.pyramid_merge(cu(torch, a)[None], cu(torch, b)[None], cu(torch, c)[None], gain)
    torch.cuda.synchronize()
    want = O.merge(a, b, c, gain)
    bound = O.merge_bound(coarse, fine[0], fine[1], gain, float(np.abs(a).max()), float(np.abs(b).max()), float(np.abs(c).max()))
    dist = float(np.abs(got[0].cpu().numpy().astype(np.float64) - want).max())
    print("merge %s->%s gain %g: distance %.3g, bound %.3g" % (coarse, fine, gain, dist, bound))
    assert dist <= bound
    assert wct.saturation_count() == 0


@pytest.mark.parametrize("coarse,fine", O.MERGE_SHAPES, ids=shape_id)
def test_merge_with_gain_zero_is_the_resampler_bit_for_bit(torch, wct, coarse, fine):
    a, b, c = (cu(torch, O.image(s, seed))[None] for s, seed in ((coarse, 31), (coarse, 32), (fine, 33)))
    want = wct.resample(a, fine, "bicubic").clone()
    assert torch.equal(wct.pyramid_merge(a, None, None, 0.0, size=fine), want)
    assert torch.equal(wct.pyramid_merge(a, b, c, 0.0), want)
    twice = wct.pyramid_merge(a, b, c, 0.75).clone()
    assert torch.equal(wct.pyramid_merge(a, b, c, 0.75), twice) and not torch.equal(twice, want)


# ---------------------------------------------------------------------------------------------------------------- 3. the cascade
def compose(eng, c, style_of, div, gain, alpha, runs):
    """The definition of include/wct_hip_scale.h, one public call per step; style_of(level) is that level's style image."""
    H, W = int(c.shape[2]), int(c.shape[3])
    F = {}
    for d in sorted(set(div)):
        size = eng.scale_shape(H, W, d)
        F[d] = c if size == (H, W) else eng.resample(c, size, "bicubic")
    cur = c if div[0] == 1 else F[div[0]]
    for run in range(runs):
        if run > 0 and div[0] > 1:
            cur = eng.resample(cur, tuple(F[div[0]].shape[2:]), "bicubic")
        for i, d in enumerate(div):
            if i > 0 and div[i - 1] != d:
                cur = eng.pyramid_merge(cur, F[div[i - 1]], F[d], gain)
            cur = eng.style_transfer_level(5 - i, cur, style_of(5 - i), alpha)
    return cur


CASCADES = [((208, 280), (4, 4, 2, 1, 1)), ((272, 300), (8, 4, 2, 1, 1))]


@pytest.mark.parametrize("size,div", CASCADES, ids=shape_id)
def test_stylize_scaled_is_the_composition_of_the_public_calls(torch, size, div):
    eng = sc.make_engine("16x")
    c, s = sc.image(41, *size), sc.image(42, *STYLE)
    out_size = eng.scale_shape(size[0], size[1], 1)
    plain = eng.stylize(c, s).clone()
    for alpha in (1.0, 0.6):
        for gain in (1.0, 0.0):
            want = compose(eng, c, lambda level: s, div, gain, alpha, 1).clone()
            got = eng.stylize_scaled(c, s, div, gain, alpha=alpha)
            assert tuple(got.shape) == (1, 3) + out_size
            assert torch.equal(got, want), (div, alpha, gain)
            assert bool(torch.isfinite(got).all()) and not torch.equal(got, plain)
    want = compose(eng, c, lambda level: s, div, 1.0, 0.6, 2).clone()
    out = torch.empty((3,) + size, device="cuda")
    r = eng.stylize_scaled(c, s, div, 1.0, alpha=0.6, num_run=2, out=out)
    assert r.data_ptr() == out.data_ptr() and torch.equal(r, want), (div, "num_run 2")
    assert eng.saturation_count() == 0


@pytest.mark.parametrize("size", [(208, 280), (100, 130)], ids=shape_id)
def test_all_divisors_one_is_stylize(torch, wct, size):
    c, s = sc.image(43, *size), sc.image(44, *STYLE)
    for alpha, runs in ((1.0, 1), (0.6, 2)):
        want = wct.stylize(c, s, alpha=alpha, num_run=runs).clone()
        assert torch.equal(wct.stylize_scaled(c, s, (1, 1, 1, 1, 1), 1.0, alpha=alpha, num_run=runs), want)
        wct.style_prepare(s)
        assert torch.equal(wct.stylize_scaled(c, None, (1, 1, 1, 1, 1), 0.0, alpha=alpha, num_run=runs), want)
    assert wct.saturation_count() == 0


def test_prepared_statistics_and_scale_mixing(torch):
    eng = sc.make_engine("16x")
    size, div = CASCADES[0]
    c, a, b = sc.image(45, *size), sc.image(46, *STYLE), sc.image(47, 96, 80)
    with_style = eng.stylize_scaled(c, a, div, 1.0, alpha=0.6).clone()
    eng.style_prepare(a)
    assert torch.equal(eng.stylize_scaled(c, None, div, 1.0, alpha=0.6), with_style)
    # style B on the levels 5 and 4, style A on the rest
    want = compose(eng, c, lambda level: b if level >= 4 else a, div, 1.0, 0.6, 1).clone()
    eng.style_prepare(b, levels=(5, 4))
    eng.style_prepare(a, levels=(3, 2, 1))
    before = [eng.style_export(level).clone() for level in (5, 4, 3, 2, 1)]
    got = eng.stylize_scaled(c, None, div, 1.0, alpha=0.6)
    assert torch.equal(got, want) and not torch.equal(got, with_style)
    after = [eng.style_export(level) for level in (5, 4, 3, 2, 1)]
    assert all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(before, after))
    assert torch.equal(eng.stylize_scaled(c, None, div, 1.0, alpha=0.6), want)                   # and serve the next call
    # a level without statistics is a state error, not a crash
    fresh = sc.make_engine("16x")
    fresh.style_prepare(a, levels=(5, 4, 3))
    with pytest.raises(_lib.WctError) as e:
        fresh.stylize_scaled(c, None, div, 1.0)
    assert e.value.code == _lib.WCT_ERR_STATE and "wct_stylize_scaled" in str(e.value)
    assert eng.saturation_count() == 0


def test_second_call_of_a_size_allocates_nothing_and_poison_changes_nothing(torch):
    eng = sc.make_engine("16x")
    runs = [(sc.image(51, *size), sc.image(52, *STYLE), div) for size, div in CASCADES]
    wants = [eng.stylize_scaled(c, s, div, 1.0, alpha=0.6, num_run=2).clone() for c, s, div in runs]
    allocs = eng.debug_get("ws_allocs")
    for (c, s, div), want in zip(runs, wants):
        assert torch.equal(eng.stylize_scaled(c, s, div, 1.0, alpha=0.6, num_run=2), want)
    eng.stylize_scaled(sc.image(53, 160, 200), sc.image(54, 64, 64), (4, 2, 2, 1, 1), 0.5)      # smaller: nothing either
    torch.cuda.synchronize()
    assert eng.debug_get("ws_allocs") == allocs
    for byte in (0x00, 0xFF):
        for (c, s, div), want in zip(runs, wants):
            eng.debug_set("poison", byte)
            assert torch.equal(eng.stylize_scaled(c, s, div, 1.0, alpha=0.6, num_run=2), want), (div, byte)
    eng.debug_set("poison", -1)
    fresh = sc.make_engine("16x")
    fresh.debug_set("poison", 0xFF)                                                              # first-use allocations filled too
    assert torch.equal(fresh.stylize_scaled(*runs[0][:2], runs[0][2], 1.0, alpha=0.6, num_run=2), wants[0])
    fresh.debug_set("poison", -1)
    assert eng.saturation_count() == 0 and fresh.saturation_count() == 0


@pytest.mark.parametrize("side", ["content", "style"])
def test_a_value_beyond_the_f16_range_reaches_range_poll(torch, side):
    eng = sc.make_engine("16x")
    eng.strict_range = False
    size, div = CASCADES[0]
    c, s = sc.image(61, *size), sc.image(62, *STYLE)
    eng.stylize_scaled(c, s, div, 1.0)
    torch.cuda.synchronize()
    n = ctypes.c_ulonglong()
    eng._chk(eng._lib.wct_range_poll(eng._ctx, ctypes.byref(n)))
    assert n.value == 0
    bad = c if side == "content" else s
    bad[0, 1, bad.shape[2] // 2, bad.shape[3] // 3] = 1e6
    eng.stylize_scaled(c, s, div, 1.0)
    torch.cuda.synchronize()
    eng._chk(eng._lib.wct_range_poll(eng._ctx, ctypes.byref(n)))
    assert n.value > 0, "%s: wct_range_poll shows nothing after the device has drained" % side
    eng.strict_range = True
    with pytest.raises(OverflowError):
        eng.noise(32, 32, seed=1)
    assert eng.saturation_count(reset=True) > 0
    eng.noise(32, 32, seed=1)


def test_stylize_scaled_is_capturable_into_a_hip_graph():
    """wct_stylize_scaled never synchronises and allocates nothing after the first call of a size: captured after a warm-up, the graph
    replays the eager bits, also with other images in the same buffers.  In a fresh process: a failed capture can leave the runtime in
    capture mode."""
    code = r"""
import sys
sys.path[:0] = [%r, %r]
import torch
from tests import state_cases as sc
wct = sc.make_engine("16x")
div = (4, 4, 2, 1, 1)
c1, c2, s1, s2 = sc.image(1, 208, 280), sc.image(2, 208, 280), sc.image(3, 84, 108), sc.image(4, 84, 108)
want1 = wct.stylize_scaled(c1, s1, div, 1.0, alpha=0.6).clone()
want2 = wct.stylize_scaled(c2, s2, div, 1.0, alpha=0.6).clone()
c, s = c1.clone(), s1.clone()
out = torch.empty((3, 208, 280), device="cuda")
wct.stylize_scaled(c, s, div, 1.0, alpha=0.6, out=out)      # warm-up on the buffers the graph will use
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph):
    wct.stylize_scaled(c, s, div, 1.0, alpha=0.6, out=out)
out.zero_()
graph.replay()
torch.cuda.synchronize()
assert torch.equal(out.view(-1)[: 3 * 208 * 272].view(1, 3, 208, 272), want1), "replay 1 differs"
c.copy_(c2); s.copy_(s2)
graph.replay()
torch.cuda.synchronize()
assert torch.equal(out.view(-1)[: 3 * 208 * 272].view(1, 3, 208, 272), want2), "replay 2 (new images, same graph) differs"
assert wct.saturation_count() == 0
print("GRAPH_OK")
""" % (REPO, PKG)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "GRAPH_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------------------- 4. refusals, command line
def test_refusals_name_the_entry_and_write_nothing(torch, wct):
    L, ctx = wct._lib, wct._ctx
    wct._stream()
    img = torch.rand((3, 208, 280), device="cuda")
    sty = torch.rand((3, 84, 108), device="cuda")
    small = torch.rand((3, 48, 64), device="cuda")
    keep = img.clone()
    outf = torch.full((3 * 208 * 280,), -3.0, device="cuda")
    p = lambda x: x.data_ptr()
    ho, wo = ctypes.c_int(-1), ctypes.c_int(-1)
    inf, nan = float("inf"), float("nan")
    div = lambda *d: (ctypes.c_int * 5)(*d)
    rs = lambda *a: L.wct_resample_planar(ctx, *a)
    pm = lambda *a: L.wct_pyramid_merge(ctx, *a)
    st = lambda *a: L.wct_stylize_scaled(ctx, *a, ctypes.byref(ho), ctypes.byref(wo))
    good = div(4, 4, 2, 1, 1)
    refusals = [
        ("wct_resample_planar", lambda: rs(None, 48, 64, p(outf), 96, 128, 1)),
        ("wct_resample_planar", lambda: rs(p(small), 48, 64, None, 96, 128, 1)),
        ("wct_resample_planar", lambda: rs(p(small), 0, 64, p(outf), 96, 128, 1)),
        ("wct_resample_planar", lambda: rs(p(small), 48, 64, p(outf), 96, 0, 1)),
        ("wct_resample_planar", lambda: rs(p(small), 48, 64, p(outf), -1, 128, 0)),
        ("wct_resample_planar", lambda: rs(p(small), 48, 64, p(outf), 96, 128, 2)),            # unknown filter ids
        ("wct_resample_planar", lambda: rs(p(small), 48, 64, p(outf), 96, 128, -1)),
        ("wct_resample_planar", lambda: rs(p(small), 48, 64, p(outf), 1, 128, 1)),             # 48 -> 1: more than 32-fold
        ("wct_resample_planar", lambda: rs(p(outf), 48, 64, p(outf) + 4 * 3 * 48 * 64 - 16, 96, 128, 1)),     # dst starts inside src
        ("wct_resample_planar", lambda: rs(p(outf), 48, 64, p(outf), 48, 64, 1)),              # a copy onto itself
        ("wct_pyramid_merge", lambda: pm(None, p(small), 48, 64, p(img), 208, 272, 1.0, p(outf))),
        ("wct_pyramid_merge", lambda: pm(p(small), p(small), 48, 64, p(img), 208, 272, 1.0, None)),
        ("wct_pyramid_merge", lambda: pm(p(small), None, 48, 64, p(img), 208, 272, 1.0, p(outf))),          # NULL b needs gain == 0
        ("wct_pyramid_merge", lambda: pm(p(small), p(small), 48, 64, None, 208, 272, 0.5, p(outf))),
        ("wct_pyramid_merge", lambda: pm(p(small), p(small), 48, 64, p(img), 208, 272, -0.5, p(outf))),
        ("wct_pyramid_merge", lambda: pm(p(small), p(small), 48, 64, p(img), 208, 272, nan, p(outf))),
        ("wct_pyramid_merge", lambda: pm(p(small), p(small), 48, 64, p(img), 208, 272, inf, p(outf))),
        ("wct_pyramid_merge", lambda: pm(p(small), p(small), 48, 0, p(img), 208, 272, 1.0, p(outf))),
        ("wct_pyramid_merge", lambda: pm(p(small), p(small), 48, 64, p(img), 1, 272, 1.0, p(outf))),
        ("wct_pyramid_merge", lambda: pm(p(small), p(small), 48, 64, p(img), 208, 272, 1.0, p(img))),       # out is c
        ("wct_pyramid_merge", lambda: pm(p(outf), p(small), 48, 64, p(img), 208, 272, 1.0, p(outf) + 64)),  # out inside a
        ("wct_stylize_scaled", lambda: st(None, 208, 280, p(sty), 84, 108, 1.0, 1, good, 1.0, p(outf))),
        ("wct_stylize_scaled", lambda: st(p(img), 208, 280, p(sty), 84, 108, 1.0, 1, good, 1.0, None)),
        ("wct_stylize_scaled", lambda: st(p(img), 208, 280, p(sty), 84, 108, 1.0, 1, None, 1.0, p(outf))),
        ("wct_stylize_scaled", lambda: st(p(img), 208, 280, p(sty), 84, 108, 1.0, 0, good, 1.0, p(outf))),
        ("wct_stylize_scaled", lambda: st(p(img), 208, 280, p(sty), 84, 108, 1.0, 1, div(0, 0, 0, 0, 0), 1.0, p(outf))),
        ("wct_stylize_scaled", lambda: st(p(img), 208, 280, p(sty), 84, 108, 1.0, 1, div(17, 4, 2, 1, 1), 1.0, p(outf))),
        ("wct_stylize_scaled", lambda: st(p(img), 208, 280, p(sty), 84, 108, 1.0, 1, div(2, 4, 2, 1, 1), 1.0, p(outf))),    # increasing towards level 1
        ("wct_stylize_scaled", lambda: st(p(img), 208, 280, p(sty), 84, 108, 1.0, 1, div(4, 4, 2, 1, 2), 1.0, p(outf))),
        ("wct_stylize_scaled", lambda: st(p(img), 208, 280, p(sty), 84, 108, 1.0, 1, div(4, 4, 2, 2, 2), 1.0, p(outf))),    # last divisor != 1
        ("wct_stylize_scaled", lambda: st(p(img), 208, 280, p(sty), 84, 108, 1.0, 1, div(8, 4, 2, 1, 1), 1.0, p(outf))),    # 16 x 32 at divisor 8
        ("wct_stylize_scaled", lambda: st(p(img), 24, 280, p(sty), 84, 108, 1.0, 1, div(1, 1, 1, 1, 1), 1.0, p(outf))),     # 16 x 272 at divisor 1
        ("wct_stylize_scaled", lambda: st(p(img), 208, 280, p(sty), 84, 108, 1.0, 1, good, -1.0, p(outf))),
        ("wct_stylize_scaled", lambda: st(p(img), 208, 280, p(sty), 84, 108, 1.0, 1, good, nan, p(outf))),
        ("wct_stylize_scaled", lambda: st(p(img), 208, 280, p(sty), 84, 108, 1.0, 1, good, inf, p(outf))),
        ("wct_stylize_scaled", lambda: st(p(outf), 208, 280, p(sty), 84, 108, 1.0, 1, good, 1.0, p(outf) + 4 * 3 * 208 * 280 - 64)),   # out overlaps the content
        ("wct_stylize_scaled", lambda: st(p(outf), 208, 280, p(sty), 84, 108, 1.0, 1, div(1, 1, 1, 1, 1), 1.0, p(outf))),
    ]
    for i, (name, call) in enumerate(refusals):
        assert call() == _lib.WCT_ERR_INVALID, (i, name)
        msg = L.wct_last_error(ctx).decode()
        assert name in msg, (i, name, msg)
    torch.cuda.synchronize()
    assert torch.equal(img, keep) and bool((outf == -3.0).all()) and (ho.value, wo.value) == (-1, -1)
    # the Python surface refuses the same way, before the C call
    for bad in ((4, 4, 2, 1), (4, 4, 2, 1, 2), (2, 4, 2, 1, 1), (17, 4, 2, 1, 1), (4, 4, 2.5, 1, 1), (8, 4, 2, 1, 1)):
        with pytest.raises(ValueError):
            wct.stylize_scaled(img[None], sty[None], bad)
    with pytest.raises(ValueError, match="detail_gain"):
        wct.stylize_scaled(img[None], sty[None], (4, 4, 2, 1, 1), detail_gain=-1.0)
    with pytest.raises(ValueError, match="filter"):
        wct.resample(small[None], (96, 128), "lanczos")
    with pytest.raises(ValueError, match="shrinks"):
        wct.resample(small[None], (1, 64))
    with pytest.raises(ValueError, match="gain"):
        wct.pyramid_merge(small[None], None, None, 0.5, size=(96, 128))
    with pytest.raises(ValueError, match="one shape"):
        wct.pyramid_merge(small[None], img[None], img[None], 0.5)
    assert wct.saturation_count() == 0


def test_cli_level_scale(torch, tmp_path):
    """One content x one style: --level_scale 4,4,2,1,1 writes a file with _scale=4-4-2-1-1 in its name whose pixels are those of
    stylize_scaled + to_u8 saved through the same Pillow call; with --coarse_style the reduced levels take the second style."""
    Image = pytest.importorskip("PIL.Image")
    from wct_hip import WCT, cli
    c, s, k = tmp_path / "content", tmp_path / "style", tmp_path / "coarse"
    for d in (c, s, k):
        d.mkdir()
    rng = np.random.default_rng(9)
    for path, (h, w) in ((c / "c1.png", (208, 280)), (s / "s1.png", (90, 84)), (k / "k1.png", (70, 96))):
        img = rng.random(((h + 3) // 4, (w + 3) // 4, 3)).repeat(4, 0).repeat(4, 1)[:h, :w] * 0.8 + rng.random((h, w, 3)) * 0.2
        Image.fromarray((img * 255).astype(np.uint8)).save(path)
    o = tmp_path / "out"
    base = ["--mode", "16x", "--contentPath", str(c), "--stylePath", str(s), "--outf", str(o), "--alpha", "0.8", "--level_scale", "4,4,2,1,1"]
    assert cli.main(base + ["--log_mark", "C", "--pipeline", "3"]) == 0
    assert cli.main(base + ["--log_mark", "K", "--coarse_style", str(k / "k1.png"), "--scale_detail", "0.5"]) == 0
    files = sorted(f for f in os.listdir(o) if f.endswith(".jpg"))
    assert files == ["C_mode=16x_alpha=0.8_scale=4-4-2-1-1_c1+s1.jpg", "K_mode=16x_alpha=0.8_scale=4-4-2-1-1_c1+s1.jpg"]
    w = WCT(types.SimpleNamespace(mode="16x", alpha=0.8))
    cf, sf, kf = (w.to_tensor_u8(torch.from_numpy(cli.load_rgb_u8(str(f))).cuda()) for f in (c / "c1.png", s / "s1.png", k / "k1.png"))
    want = w.to_u8(w.stylize_scaled(cf, sf, (4, 4, 2, 1, 1), 1.0, alpha=0.8), 0).cpu().numpy()
    Image.fromarray(want).save(tmp_path / "ref.jpg")
    assert (o / files[0]).read_bytes() == (tmp_path / "ref.jpg").read_bytes()
    mixed = compose(w, cf, lambda level: kf if level >= 3 else sf, (4, 4, 2, 1, 1), 0.5, 0.8, 1)
    Image.fromarray(w.to_u8(mixed, 0).cpu().numpy()).save(tmp_path / "mix.jpg")
    assert (o / files[1]).read_bytes() == (tmp_path / "mix.jpg").read_bytes()
    assert "--pipeline is ignored with --level_scale" in open(o / "log_C_16x.txt").read()
