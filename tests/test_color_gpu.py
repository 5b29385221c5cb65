"""Colour preservation on the device (include/wct_hip_color.h): the four kernels against the numpy reference (tests/color_oracle.py),
wct_color_match and wct_stylize_color against the public calls they are made of (bit for bit -- which puts them under every parity
gate wct_stylize is under), the levels against the CPU checker, allocation and graph capture, history independence of every new entry
with the helpers of tests/state_cases.py, the refusals, and the command line's --preserve_color.

The module imports without a GPU: tests/test_color_cpu.py reads CASES."""
import collections
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from tests import color_oracle as O
from tests import state_cases as sc
from tests.conftest import PKG, REPO, rel_err
from wct_hip import lib as _lib

pytestmark = pytest.mark.gpu
natural = O.natural


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
    """A copy of the flat fp32 tensor x that starts `off` floats behind a 16-byte boundary."""
    buf = torch.empty(x.numel() + 8, device="cuda", dtype=torch.float32)
    base = (-(buf.data_ptr() // 4)) % 4                # floats to the next 16-byte boundary
    v = buf[base + off: base + off + x.numel()]
    assert v.data_ptr() % 16 == 4 * off
    v.copy_(x.reshape(-1))
    return v.view(x.shape)


# ---------------------------------------------------------------------------------------------------------------- 1. moments
@pytest.mark.parametrize("H,W", [(1, 2), (5, 7), (33, 65), (600, 900), (2160, 3840)])
def test_moments_against_the_oracle_and_bitwise_reproducible(torch, wct, H, W):
    rng = np.random.default_rng(H * 31 + W)
    img = rng.random((3, H, W), dtype=np.float32)
    img[1] = 0.5 * img[1] + 0.5 * img[0]
    x = cu(torch, img)
    n, s, ss = wct.color_moments(x)
    n0, s0, ss0 = O.moments(img)
    assert n == n0 == H * W
    es = float(np.abs(s.cpu().numpy() - s0).max() / np.abs(s0).min())
    ess = float((np.abs(ss.cpu().numpy() - ss0) / np.abs(ss0)).max())
    print("color_moments %dx%d: rel err sum %.2e, sumsq %.2e" % (H, W, es, ess))
    assert (np.abs(s.cpu().numpy() - s0) <= 1e-12 * np.abs(s0)).all() and (np.abs(ss.cpu().numpy() - ss0) <= 1e-12 * np.abs(ss0)).all()
    assert torch.equal(ss, ss.T)
    _, s2, ss2 = wct.color_moments(x)
    assert torch.equal(s, s2) and torch.equal(ss, ss2), "two calls differ"
    for off in (0, 1, 2, 3):
        v = offset_view(torch, x, off)
        _, sv, ssv = wct.color_moments(v)
        assert torch.equal(s, sv) and torch.equal(ss, ssv), "a view %d bytes off a 16-byte boundary sums differently" % (4 * off)
    other = sc.make_engine("16x")
    _, so, sso = other.color_moments(x)
    assert torch.equal(s, so) and torch.equal(ss, sso), "two contexts differ"


# ---------------------------------------------------------------------------------------------------------------- 2. solve
def solve_cases():
    c = natural(11, 120, 160)
    grey = np.repeat(natural(12, 90, 110).mean(0, keepdims=True), 3, 0).astype(np.float32)
    const = np.broadcast_to(np.array([0.25, 0.5, 0.75], np.float32)[:, None, None], (3, 64, 80)).copy()
    return {"natural": (c, natural(13, 100, 140, cast=(0.5, 1.0, 0.9), shift=(0.3, 0.0, 0.1))), "grey style": (c, grey),
            "constant style": (c, const), "style == content": (c, c)}


@pytest.mark.parametrize("name", ["natural", "grey style", "constant style", "style == content"])
def test_solve_against_the_oracle(torch, wct, name):
    c, s = solve_cases()[name]
    mc, ms = O.moments(c), O.moments(s)
    A0, t0 = O.solve(*mc, *ms)
    A, t = wct.color_solve(mc[0], cu(torch, mc[1], np.float64), cu(torch, mc[2], np.float64), ms[0], cu(torch, ms[1], np.float64),
                           cu(torch, ms[2], np.float64))
    A, t = A.cpu().numpy(), t.cpu().numpy()
    scale = np.abs(A0).max()
    eA, et = float(np.abs(A - A0).max() / scale), float(np.abs(t - t0).max() / scale)
    print("color_solve %s: max|A| %.4g, err A %.2e, err t %.2e (relative to max|A|)" % (name, scale, eA, et))
    assert np.isfinite(A).all() and np.isfinite(t).all()
    assert eA <= 1e-8 and et <= 1e-8
    if name == "style == content":
        assert np.abs(A - np.eye(3)).max() <= 1e-8 and np.abs(t).max() <= 1e-8
    # another eps is honoured
    A1, t1 = O.solve(*mc, *ms, eps=1e-3)
    A2, t2 = wct.color_solve(mc[0], cu(torch, mc[1], np.float64), cu(torch, mc[2], np.float64), ms[0], cu(torch, ms[1], np.float64),
                             cu(torch, ms[2], np.float64), eps=1e-3)
    assert np.abs(A2.cpu().numpy() - A1).max() <= 1e-8 * np.abs(A1).max() and np.abs(t2.cpu().numpy() - t1).max() <= 1e-8 * np.abs(A1).max()


# ---------------------------------------------------------------------------------------------------------------- 3. apply and match
def one_rounding(got, ref):
    """2^-23 max(1, |out|) + 1e-10 per element: one fp32 rounding of an fp64 result."""
    return np.abs(got.astype(np.float64) - ref) <= 2.0 ** -23 * np.maximum(1.0, np.abs(ref)) + 1e-10


@pytest.mark.parametrize("H,W", [(1, 2), (33, 65), (250, 333), (512, 768)])
def test_apply_against_the_oracle_and_in_place(torch, wct, H, W):
    rng = np.random.default_rng(H + W)
    img = rng.random((3, H, W), dtype=np.float32) * 2 - 0.5
    A = np.eye(3) + 0.3 * rng.standard_normal((3, 3))
    t = 0.2 * rng.standard_normal(3)
    x = cu(torch, img)
    got = wct.color_apply(x, cu(torch, A, np.float64), cu(torch, t, np.float64))
    assert tuple(got.shape) == (1, 3, H, W)
    assert one_rounding(got.cpu().numpy()[0], O.apply(img, A, t)).all()
    for off in (1, 3):
        v = offset_view(torch, x, off)
        assert torch.equal(wct.color_apply(v, cu(torch, A, np.float64), cu(torch, t, np.float64))[0], got[0])
    y = x.clone()
    back = wct.color_apply(y, cu(torch, A, np.float64), cu(torch, t, np.float64), out=y)
    assert back.data_ptr() == y.data_ptr() and torch.equal(y, got[0]), "in place differs from out of place"
    with pytest.raises(ValueError):
        wct.color_apply(x, cu(torch, A, np.float64), cu(torch, t, np.float64), out=torch.empty(3 * H * W + 1, device="cuda"))


@pytest.mark.parametrize("name", ["natural", "grey style", "constant style", "style == content"])
def test_match_against_the_oracle_and_the_chain(torch, wct, name):
    c, s = solve_cases()[name]
    xc, xs = cu(torch, c), cu(torch, s)
    got = wct.color_match(xs, xc)
    ref = O.match(s, c)
    A0, _ = O.solve(*O.moments(c), *O.moments(s))
    err = np.abs(got.cpu().numpy()[0].astype(np.float64) - ref)
    print("color_match %s: max err %.3e (max|A| %.4g)" % (name, float(err.max()), np.abs(A0).max()))
    assert one_rounding(got.cpu().numpy()[0], ref).all()
    # bit for bit the four-call chain
    nc, sc_, ssc = wct.color_moments(xc)
    ns, ss_, sss = wct.color_moments(xs)
    A, t = wct.color_solve(nc, sc_, ssc, ns, ss_, sss, eps=_lib.COLOR_EPS)
    chain = wct.color_apply(xs, A, t)
    assert torch.equal(got, chain), "wct_color_match differs from moments + moments + solve + apply"
    # apply against the oracle with the DEVICE's map: the one-rounding bound alone
    assert one_rounding(chain.cpu().numpy()[0], O.apply(s, A.cpu().numpy(), t.cpu().numpy())).all()
    y = xs.clone()
    wct.color_match(y, xc, out=y)
    assert torch.equal(y, got[0]), "in place differs from out of place"
    if name == "natural":      # the matched style has the content's colour statistics: A (S_s + eps I) A^T = S_c + eps I, mean mu_c
        mu_m, Sm = O.cov(*O.moments(got.cpu().numpy()[0]), eps=0.0)
        mu_c, Sc = O.cov(*O.moments(c), eps=0.0)
        # (the pixels were rounded to fp32: ~6e-8 relative each)
        assert np.abs(mu_m - mu_c).max() <= 1e-6 and np.abs(Sm + O.EPS * A0 @ A0.T - Sc - O.EPS * np.eye(3)).max() <= 1e-5 * np.abs(Sc).max()


# ---------------------------------------------------------------------------------------------------------------- 4. luma merge
@pytest.mark.parametrize("Hc,Wc,Ho,Wo", [(250, 333, 240, 320), (33, 65, 33, 65), (40, 50, 37, 47), (1, 2, 1, 1), (600, 900, 592, 896)])
def test_luma_merge_against_the_oracle(torch, wct, Hc, Wc, Ho, Wo):
    rng = np.random.default_rng(Hc * 3 + Wo)
    c = rng.random((3, Hc, Wc), dtype=np.float32)
    s = (rng.random((3, Ho, Wo), dtype=np.float32) * 3 - 1).astype(np.float32)       # [-1, 2]
    xc, xs = cu(torch, c), cu(torch, s)
    got = wct.luma_merge(xs, xc)
    assert tuple(got.shape) == (1, 3, Ho, Wo)
    err = float(np.abs(got.cpu().numpy()[0] - O.luma_merge(s, c)).max())
    print("luma_merge %dx%d in %dx%d: max abs err %.3e" % (Ho, Wo, Hc, Wc, err))
    assert err <= 1e-6
    for mode in (0, 1):
        u8 = wct.luma_merge(xs, xc, u8=True, round_mode=mode)
        assert u8.dtype == torch.uint8 and tuple(u8.shape) == (Ho, Wo, 3)
        assert torch.equal(u8, wct.to_u8(got, mode)), "fused uint8 output differs from to_u8 of the planar output (round_mode %d)" % mode
        assert np.array_equal(u8.cpu().numpy(), O.to_u8(got.cpu().numpy()[0], mode))
    # out= buffers inside larger ones: what surrounds the result stays untouched
    big = torch.full((3 * Ho * Wo + 8,), -7.0, device="cuda")
    wct.luma_merge(xs, xc, out=big[4: 4 + 3 * Ho * Wo])
    assert torch.equal(big[4: 4 + 3 * Ho * Wo].view(1, 3, Ho, Wo), got) and bool((big[:4] == -7.0).all()) and bool((big[-4:] == -7.0).all())
    bigb = torch.full((3 * Ho * Wo + 8,), 201, device="cuda", dtype=torch.uint8)
    wct.luma_merge(xs, xc, out=bigb[4: 4 + 3 * Ho * Wo], u8=True)
    assert torch.equal(bigb[4: 4 + 3 * Ho * Wo].view(Ho, Wo, 3), wct.to_u8(got, 0)) and bool((bigb[:4] == 201).all()) and bool((bigb[-4:] == 201).all())
    for off in (1, 2, 3):      # a uint8 base that is not 4-byte aligned: single-byte stores, the same bytes
        bigb.fill_(201)
        wct.luma_merge(xs, xc, out=bigb[off: off + 3 * Ho * Wo], u8=True, round_mode=1)
        assert torch.equal(bigb[off: off + 3 * Ho * Wo].view(Ho, Wo, 3), wct.to_u8(got, 1)), off
        assert bool((bigb[:off] == 201).all()) and bool((bigb[off + 3 * Ho * Wo:] == 201).all()), off
    # misaligned planes give the same bits; in place over the stylised image too
    assert torch.equal(wct.luma_merge(offset_view(torch, xs, 1), offset_view(torch, xc, 3)), got)
    y = xs.clone()
    wct.luma_merge(y, xc, out=y)
    assert torch.equal(y, got[0])
    assert torch.equal(xc, cu(torch, c)), "the content was written"


# ---------------------------------------------------------------------------------------------------------------- 5. the cascade
@pytest.mark.parametrize("H,W,Hs,Ws,transform", [
    pytest.param(250, 333, 200, 160, "wct", id="250-333-200-160"), pytest.param(512, 768, 300, 420, "wct", id="512-768-300-420"),
    pytest.param(250, 333, 200, 160, "ot", id="250-333-200-160-ot"), pytest.param(250, 333, 200, 160, "adain", id="250-333-200-160-adain")])
def test_stylize_color_is_the_composition_of_the_public_calls(torch, wct, H, W, Hs, Ws, transform):
    """Under ot and adain (include/wct_hip_transform.h: the composed entries follow the context's mode) the same identities, on an
    engine of that mode; the style lane is then waited for BEFORE the content solve."""
    c, s = cu(torch, natural(H, H, W))[None], cu(torch, natural(W, Hs, Ws, cast=(0.5, 1.0, 0.9), shift=(0.3, 0.0, 0.1)))[None]
    if transform != "wct":
        under_wct = wct.stylize(c, s, alpha=0.6).clone()
        wct = sc.make_engine("16x")
        wct.set_transform(transform)
        assert not torch.equal(wct.stylize(c, s, alpha=0.6), under_wct)          # the mode took effect
    for alpha, runs in ((1.0, 1), (0.6, 1), (0.6, 2)):
        matched = wct.color_match(s, c)
        plain = wct.stylize(c, s, alpha=alpha, num_run=runs).clone()
        on_matched = wct.stylize(c, matched, alpha=alpha, num_run=runs).clone()
        got = wct.stylize_color(c, s, "match", alpha=alpha, num_run=runs)
        assert tuple(got.shape) == (1, 3, H // 16 * 16, W // 16 * 16)
        assert torch.equal(got, on_matched), ("match", alpha, runs)
        assert torch.equal(wct.stylize_color(c, s, "luma", alpha=alpha, num_run=runs), wct.luma_merge(plain, c)), ("luma", alpha, runs)
        assert torch.equal(wct.stylize_color(c, s, "match+luma", alpha=alpha, num_run=runs), wct.luma_merge(on_matched, c)), ("match+luma", alpha, runs)
        assert not torch.equal(plain, on_matched)
    out = torch.empty((3, H, W), device="cuda")
    r = wct.stylize_color(c, s, "match+luma", alpha=0.6, num_run=2, out=out)
    assert r.data_ptr() == out.data_ptr() and torch.equal(r, wct.luma_merge(on_matched, c))
    with pytest.raises(ValueError, match="mode"):
        wct.stylize_color(c, s, "chroma")
    assert wct.saturation_count() == 0


def test_match_levels_against_the_cpu_checker(torch, wct, oracle, weights16x):
    """One small case per level: the checker's style_transfer is fed the ORACLE-matched style, level-isolated as
    __graft_entry__.smoke() does (the checker's previous output feeds both sides); the device gets the device-matched style.
    Level isolation means the match is REDONE at every level, against that level's input (the checker's previous output): this
    exercises wct_color_match + wct_style_transfer_level, not wct_stylize_color's match-once-against-the-original -- that one is
    covered by the bit-for-bit composition test above.
    Limit: rel_err < 1e-3, the gate of BASELINE.md section 3.5."""
    c, s = natural(21, 96, 128), natural(22, 80, 96, cast=(0.5, 1.0, 0.9), shift=(0.3, 0.0, 0.1))
    mods = oracle.Modules("16x", weights16x)
    img = c
    for level in (5, 4, 3, 2, 1):
        s_ref = O.match(s, img).astype(np.float32)
        s_dev = wct.color_match(cu(torch, s), cu(torch, img))
        ref = oracle.style_transfer(mods, level, img, s_ref, 1.0)
        got = wct.style_transfer_level(level, cu(torch, img)[None], s_dev).cpu().numpy()[0]
        err = rel_err(got, ref)
        print("colour-matched level %d: rel err %.3e" % (level, err))
        assert got.shape == ref.shape and err < 1e-3, (level, err)
        img = ref
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 6. no hidden host work
def test_second_call_of_a_size_allocates_nothing(torch):
    eng = sc.make_engine("16x")
    c, s = sc.image(1, 250, 333), sc.image(2, 200, 160)
    for mode in ("match", "luma", "match+luma"):
        eng.stylize_color(c, s, mode)
    eng.color_match(s, c), eng.luma_merge(c[:, :, :240, :320], c, u8=True), eng.color_moments(c)
    allocs = eng.debug_get("ws_allocs")
    for mode in ("match", "luma", "match+luma"):
        eng.stylize_color(c, s, mode, alpha=0.6, num_run=2)
    eng.stylize_color(sc.image(3, 120, 200), sc.image(4, 90, 100), "match+luma")          # smaller: nothing either
    eng.color_match(s, c), eng.luma_merge(c[:, :, :240, :320], c, u8=True), eng.color_moments(c)
    assert eng.debug_get("ws_allocs") == allocs
    assert eng.saturation_count() == 0


def test_colour_calls_are_capturable_into_a_hip_graph():
    """wct_stylize_color and wct_color_solve never synchronise and allocate nothing after the first call of a size: captured after a
    warm-up (as tests/test_hip_parity.py does for wct_stylize), the graph replays the eager bits, also with other images in the same
    buffers.  In a fresh process: a failed capture can leave the runtime in capture mode."""
    code = r"""
import sys, types
sys.path[:0] = [%r, %r]
import torch
from tests import state_cases as sc
wct = sc.make_engine("16x")
c1, c2, s1, s2 = sc.image(1, 272, 400), sc.image(2, 272, 400), sc.image(3, 200, 240), sc.image(4, 200, 240)
for mode in ("match", "luma", "match+luma"):
    want1 = wct.stylize_color(c1, s1, mode, alpha=0.6).clone()
    want2 = wct.stylize_color(c2, s2, mode, alpha=0.6).clone()
    c, s = c1.clone(), s1.clone()
    out = torch.empty((3, 272, 400), device="cuda")
    wct.stylize_color(c, s, mode, alpha=0.6, out=out)      # warm-up on the buffers the graph will use
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        wct.stylize_color(c, s, mode, alpha=0.6, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(1, 3, 272, 400), want1), mode + ": replay 1 differs"
    c.copy_(c2); s.copy_(s2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(1, 3, 272, 400), want2), mode + ": replay 2 (new images, same graph) differs"
# the split entries: moments of both sides, solve and apply in one graph (no `info`, no synchronisation)
nc, sc_, ssc = wct.color_moments(c1)
ns, ss_, sss = wct.color_moments(s1)
A, t = wct.color_solve(nc, sc_, ssc, ns, ss_, sss)
want = wct.color_apply(s1, A, t).clone()
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph):
    _, a1, a2 = wct.color_moments(c1)
    _, b1, b2 = wct.color_moments(s1)
    A, t = wct.color_solve(nc, a1, a2, ns, b1, b2)
    got = wct.color_apply(s1, A, t)
graph.replay()
torch.cuda.synchronize()
assert torch.equal(got, want), "split chain: replay differs"
assert wct.saturation_count() == 0
print("GRAPH_OK")
""" % (REPO, PKG)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "GRAPH_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------------------- 7. history independence
Case = collections.namedtuple("Case", "fn covers size family")
CASES = collections.OrderedDict()


def case(family, covers):
    def deco(f):
        for size in ("small", "large"):
            CASES["%s/%s" % (family, size)] = Case((lambda eng, seed, _f=f, _s=size: _f(eng, seed, _s)), tuple(covers), size, family)
        return f
    return deco


@case("color_moments", ["wct_color_moments"])
def _color_moments(eng, seed, size):
    H, W, Hs, Ws = sc.SIZES[size]
    _, s, ss = eng.color_moments(sc.image(seed, H, W))
    _, s2, ss2 = eng.color_moments(sc.image(seed + 1, Hs, Ws))
    return {"sum": s, "sumsq": ss, "sum_style": s2, "sumsq_style": ss2}


def _raw_colour_moments(seed, n):
    rng = np.random.default_rng(seed)
    x = rng.random((3, 4096)) * rng.random((3, 1)) + 0.3 * rng.random((1, 4096))
    import torch
    return float(n), torch.from_numpy(x.sum(1) * (n / 4096)).cuda(), torch.from_numpy((x @ x.T) * (n / 4096)).cuda()


@case("color_solve", ["wct_color_solve"])
def _color_solve(eng, seed, size):
    n = 13000 if size == "small" else 540000
    A, t = eng.color_solve(*_raw_colour_moments(seed, n), *_raw_colour_moments(seed + 1, n // 2))
    A2, t2 = eng.color_solve(*_raw_colour_moments(seed + 2, n), *_raw_colour_moments(seed + 3, n // 3), eps=1e-3)
    return {"A": A, "t": t, "A_eps": A2, "t_eps": t2}


@case("color_apply", ["wct_color_apply"])
def _color_apply(eng, seed, size):
    H, W = sc.SIZES[size][:2]
    M, b = sc.affine(seed + 1, 1, 3)
    return {"out": eng.color_apply(sc.image(seed, H, W), M[0], b[0])}


@case("color_match", ["wct_color_match"])
def _color_match(eng, seed, size):
    H, W, Hs, Ws = sc.SIZES[size]
    return {"out": eng.color_match(sc.image(seed + 1, Hs, Ws), sc.image(seed, H, W))}


@case("luma_merge", ["wct_luma_merge"])
def _luma_merge(eng, seed, size):
    H, W = sc.SIZES[size][:2]
    c, s = sc.image(seed, H, W), sc.image(seed + 1, H // 16 * 16, W // 16 * 16) * 1.4 - 0.2
    return {"planar": eng.luma_merge(s, c), "u8_floor": eng.luma_merge(s, c, u8=True), "u8_round": eng.luma_merge(s, c, u8=True, round_mode=1)}


@case("stylize_color", ["wct_stylize_color"])
def _stylize_color(eng, seed, size):
    H, W, Hs, Ws = sc.SIZES[size]
    c, s = sc.image(seed, H, W), sc.image(seed + 1, Hs, Ws)
    return {"match": eng.stylize_color(c, s, "match"), "luma_a06_run2": eng.stylize_color(c, s, "luma", alpha=0.6, num_run=2),
            "both": eng.stylize_color(c, s, "match+luma", alpha=0.8)}


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


def test_stylisation_after_stylize_color_and_the_slot_lifetime(torch, controls):
    """A stylisation after wct_stylize_color equals the same stylisation on a fresh engine, and the prepared slot then holds the
    MATCHED style's statistics (include/wct_hip_color.h)."""
    H, W, Hs, Ws = sc.SIZES["small"]
    c, s, c2 = sc.image(50, H, W), sc.image(51, Hs, Ws), sc.image(52, H + 12, W - 20)
    fresh = sc.make_engine("16x")
    want_plain = fresh.stylize(c, s, alpha=0.9).clone()
    matched = fresh.color_match(s, c)
    fresh.style_prepare(matched)
    want_on_matched = fresh.stylize_prepared(c2, alpha=0.9).clone()
    fresh.style_prepare(s)
    want_on_given = fresh.stylize_prepared(c2, alpha=0.9).clone()
    eng = sc.make_engine("16x")
    for name in ("stylize_color/small", "stylize_color/large"):
        run(eng, name)
    assert torch.equal(eng.stylize(c, s, alpha=0.9), want_plain), "wct_stylize after wct_stylize_color"
    same(torch, sc.run(eng, "stylize/small"), sc.run(fresh, "stylize/small"), "stylize/small after wct_stylize_color")
    eng.stylize_color(c, s, "match")
    assert torch.equal(eng.stylize_prepared(c2, alpha=0.9), want_on_matched), "the slot does not hold the matched style's statistics"
    eng.stylize_color(c, s, "match+luma")
    assert torch.equal(eng.stylize_prepared(c2, alpha=0.9), want_on_matched)
    eng.stylize_color(c, s, "luma")
    assert torch.equal(eng.stylize_prepared(c2, alpha=0.9), want_on_given), "luma alone leaves the given style's statistics"
    assert not torch.equal(want_on_matched, want_on_given)
    assert eng.saturation_count() == 0 and fresh.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 8. errors
def test_refusals_name_the_entry_and_write_nothing(torch, wct):
    L, ctx = wct._lib, wct._ctx
    wct._stream()
    img = torch.rand((3, 40, 48), device="cuda")
    small = torch.rand((3, 1, 1), device="cuda")
    sty = torch.rand((3, 32, 32), device="cuda")
    f64 = torch.full((64,), -3.0, device="cuda", dtype=torch.float64)
    s, ss, A, t = (f64[0:3], f64[8:17], f64[24:33], f64[40:43])
    outf = torch.full((3 * 40 * 48,), -3.0, device="cuda")
    outb = torch.full((3 * 40 * 48,), 77, device="cuda", dtype=torch.uint8)
    p = lambda x: x.data_ptr()
    ho, wo = ctypes.c_int(-1), ctypes.c_int(-1)
    refusals = [
        ("wct_color_moments", lambda: L.wct_color_moments(ctx, None, 40, 48, p(s), p(ss))),
        ("wct_color_moments", lambda: L.wct_color_moments(ctx, p(img), 40, 48, None, p(ss))),
        ("wct_color_moments", lambda: L.wct_color_moments(ctx, p(img), 40, 48, p(s), None)),
        ("wct_color_moments", lambda: L.wct_color_moments(ctx, p(img), 0, 48, p(s), p(ss))),
        ("wct_color_moments", lambda: L.wct_color_moments(ctx, p(img), 40, -1, p(s), p(ss))),
        # more than 2^33 pixels: the second stage would add more than 4096 partials in sequence (nothing is read)
        ("wct_color_moments", lambda: L.wct_color_moments(ctx, p(img), 100000, 100000, p(s), p(ss))),
        ("wct_color_match", lambda: L.wct_color_match(ctx, p(sty), 32, 32, p(img), 100000, 100000, p(outf))),
        ("wct_stylize_color", lambda: L.wct_stylize_color(ctx, p(img), 100000, 100000, p(sty), 32, 32, 1.0, 1, 1, p(outf), ctypes.byref(ho), ctypes.byref(wo))),
        ("wct_color_solve", lambda: L.wct_color_solve(ctx, 1.0, p(s), p(ss), 100.0, p(s), p(ss), 1e-5, p(A), p(t))),
        ("wct_color_solve", lambda: L.wct_color_solve(ctx, 100.0, p(s), p(ss), 1.5, p(s), p(ss), 1e-5, p(A), p(t))),
        ("wct_color_solve", lambda: L.wct_color_solve(ctx, 100.0, p(s), p(ss), 100.0, p(s), p(ss), 0.0, p(A), p(t))),
        ("wct_color_solve", lambda: L.wct_color_solve(ctx, 100.0, p(s), p(ss), 100.0, p(s), p(ss), -1e-5, p(A), p(t))),
        ("wct_color_solve", lambda: L.wct_color_solve(ctx, 100.0, p(s), p(ss), 100.0, p(s), p(ss), float("inf"), p(A), p(t))),
        ("wct_color_solve", lambda: L.wct_color_solve(ctx, 100.0, p(s), p(ss), 100.0, p(s), p(ss), float("nan"), p(A), p(t))),
        ("wct_color_solve", lambda: L.wct_color_solve(ctx, 100.0, p(s), None, 100.0, p(s), p(ss), 1e-5, p(A), p(t))),
        ("wct_color_solve", lambda: L.wct_color_solve(ctx, 100.0, p(s), p(ss), 100.0, p(s), p(ss), 1e-5, None, p(t))),
        ("wct_color_apply", lambda: L.wct_color_apply(ctx, None, 40, 48, p(A), p(t), p(outf))),
        ("wct_color_apply", lambda: L.wct_color_apply(ctx, p(img), 40, 48, None, p(t), p(outf))),
        ("wct_color_apply", lambda: L.wct_color_apply(ctx, p(img), 40, 48, p(A), p(t), None)),
        ("wct_color_apply", lambda: L.wct_color_apply(ctx, p(img), 40, 0, p(A), p(t), p(outf))),
        ("wct_color_match", lambda: L.wct_color_match(ctx, None, 32, 32, p(img), 40, 48, p(outf))),
        ("wct_color_match", lambda: L.wct_color_match(ctx, p(sty), 32, 32, None, 40, 48, p(outf))),
        ("wct_color_match", lambda: L.wct_color_match(ctx, p(sty), 32, 32, p(img), 40, 48, None)),
        ("wct_color_match", lambda: L.wct_color_match(ctx, p(sty), 32, 32, p(small), 1, 1, p(outf))),
        ("wct_color_match", lambda: L.wct_color_match(ctx, p(small), 1, 1, p(img), 40, 48, p(outf))),
        ("wct_color_match", lambda: L.wct_color_match(ctx, p(sty), 0, 32, p(img), 40, 48, p(outf))),
        ("wct_luma_merge", lambda: L.wct_luma_merge(ctx, None, 32, 32, p(img), 40, 48, p(outf), None, 0)),
        ("wct_luma_merge", lambda: L.wct_luma_merge(ctx, p(sty), 32, 32, None, 40, 48, p(outf), None, 0)),
        ("wct_luma_merge", lambda: L.wct_luma_merge(ctx, p(sty), 32, 32, p(img), 40, 48, p(outf), p(outb), 0)),
        ("wct_luma_merge", lambda: L.wct_luma_merge(ctx, p(sty), 32, 32, p(img), 40, 48, None, None, 0)),
        ("wct_luma_merge", lambda: L.wct_luma_merge(ctx, p(img), 40, 48, p(sty), 32, 32, p(outf), None, 0)),      # Ho > Hc
        ("wct_luma_merge", lambda: L.wct_luma_merge(ctx, p(img), 32, 48, p(img), 40, 32, p(outf), None, 0)),      # Wo > Wc
        ("wct_luma_merge", lambda: L.wct_luma_merge(ctx, p(sty), 0, 32, p(img), 40, 48, p(outf), None, 0)),
        ("wct_luma_merge", lambda: L.wct_luma_merge(ctx, p(sty), 32, 32, p(img), 40, 48, None, p(outb), 2)),
        ("wct_stylize_color", lambda: L.wct_stylize_color(ctx, None, 40, 48, p(sty), 32, 32, 1.0, 1, 1, p(outf), ctypes.byref(ho), ctypes.byref(wo))),
        ("wct_stylize_color", lambda: L.wct_stylize_color(ctx, p(img), 40, 48, None, 32, 32, 1.0, 1, 1, p(outf), ctypes.byref(ho), ctypes.byref(wo))),
        ("wct_stylize_color", lambda: L.wct_stylize_color(ctx, p(img), 40, 48, p(sty), 32, 32, 1.0, 1, 1, None, ctypes.byref(ho), ctypes.byref(wo))),
        ("wct_stylize_color", lambda: L.wct_stylize_color(ctx, p(img), 40, 48, p(sty), 32, 32, 1.0, 0, 1, p(outf), ctypes.byref(ho), ctypes.byref(wo))),
        ("wct_stylize_color", lambda: L.wct_stylize_color(ctx, p(img), 40, 48, p(sty), 32, 32, 1.0, 1, 0, p(outf), ctypes.byref(ho), ctypes.byref(wo))),
        ("wct_stylize_color", lambda: L.wct_stylize_color(ctx, p(img), 40, 48, p(sty), 32, 32, 1.0, 1, 4, p(outf), ctypes.byref(ho), ctypes.byref(wo))),
        ("wct_stylize_color", lambda: L.wct_stylize_color(ctx, p(img), 40, 48, p(sty), 32, 32, 1.0, 1, -1, p(outf), ctypes.byref(ho), ctypes.byref(wo))),
        ("wct_stylize_color", lambda: L.wct_stylize_color(ctx, p(img), 0, 48, p(sty), 32, 32, 1.0, 1, 3, p(outf), ctypes.byref(ho), ctypes.byref(wo))),
        ("wct_stylize_color", lambda: L.wct_stylize_color(ctx, p(img), 40, 48, p(small), 1, 1, 1.0, 1, 1, p(outf), ctypes.byref(ho), ctypes.byref(wo))),
    ]
    for i, (name, call) in enumerate(refusals):
        assert call() == _lib.WCT_ERR_INVALID, (i, name)
        msg = L.wct_last_error(ctx).decode()
        assert name in msg, (i, name, msg)
    torch.cuda.synchronize()
    assert bool((f64 == -3.0).all()) and bool((outf == -3.0).all()) and bool((outb == 77).all()) and (ho.value, wo.value) == (-1, -1)
    # the Python surface refuses the same way
    with pytest.raises(ValueError):
        wct.luma_merge(img, sty)
    with pytest.raises(ValueError):
        wct.color_match(small, img)
    with pytest.raises(ValueError, match="eps"):
        wct.color_solve(100.0, s, ss, 100.0, s, ss, eps=0.0)
    with pytest.raises(ValueError):
        wct.luma_merge(sty, img, out=torch.empty(5, device="cuda"))
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 9. command line
def test_cli_preserve_color(torch, tmp_path):
    """Two contents x two styles of ~300 x 400: --preserve_color match and luma each write the same bytes with --pipeline 0 and
    --pipeline 3, under the new name; the files are those of the test's own library calls saved through the same Pillow call; the luma
    files differ from a run without the flag; --maskPath with --preserve_color luma runs."""
    Image = pytest.importorskip("PIL.Image")
    from wct_hip import WCT, cli
    c, s, m = tmp_path / "content", tmp_path / "style", tmp_path / "masks"
    c.mkdir(); s.mkdir(); m.mkdir()
    shapes = {"c1.png": (300, 400), "c2.png": (288, 410), "s1.png": (310, 390), "s2.png": (280, 420)}
    for i, (n, (h, w)) in enumerate(shapes.items()):
        img = (natural(90 + i, h, w, cast=(1.0, 0.7, 0.5) if i % 2 else (0.5, 0.9, 1.0)) * 255).astype(np.uint8).transpose(1, 2, 0)
        Image.fromarray(np.ascontiguousarray(img)).save((c if n[0] == "c" else s) / n)
    for n in ("c1", "c2"):
        h, w = shapes[n + ".png"]
        lab = (np.arange(h)[:, None] // 32 + np.arange(w)[None, :] // 32) % 3
        lab[lab == 2] = 255
        Image.fromarray(lab.astype(np.uint8), mode="L").save(m / (n + ".png"))

    def run_cli(tag, *extra):
        o = tmp_path / tag
        assert cli.main(["--mode", "16x", "--contentPath", str(c), "--stylePath", str(s), "--outf", str(o), "--log_mark", "C", "--alpha", "0.8",
                         "--io_threads", "3"] + list(extra)) == 0
        return o, {f: (o / f).read_bytes() for f in sorted(os.listdir(o)) if f.endswith(".jpg")}

    _, plain = run_cli("plain", "--pipeline", "0")
    w = WCT(types.SimpleNamespace(mode="16x", alpha=0.8))
    for mode in ("match", "luma"):
        _, serial = run_cli(mode + "_serial", "--pipeline", "0", "--preserve_color", mode)
        _, piped = run_cli(mode + "_pipe", "--pipeline", "3", "--preserve_color", mode)
        names = sorted("C_mode=16x_alpha=0.8_color=%s_%s+%s.jpg" % (mode, a, b) for a in ("c1", "c2") for b in ("s1", "s2"))
        assert sorted(serial) == names and serial == piped, mode
        for a in ("c1", "c2"):
            for b in ("s1", "s2"):
                cf = w.to_tensor_u8(torch.from_numpy(cli.load_rgb_u8(str(c / (a + ".png")))).cuda())
                sf = w.to_tensor_u8(torch.from_numpy(cli.load_rgb_u8(str(s / (b + ".png")))).cuda())
                if mode == "match":
                    ref = w.to_u8(w.stylize(cf, w.color_match(sf, cf), alpha=0.8), 0)
                else:
                    w.style_prepare(sf)
                    ref = w.to_u8(w.luma_merge(w.stylize_prepared(cf, alpha=0.8), cf), 0)
                Image.fromarray(ref.cpu().numpy()).save(tmp_path / "ref.jpg")
                name = "C_mode=16x_alpha=0.8_color=%s_%s+%s.jpg" % (mode, a, b)
                assert (tmp_path / "ref.jpg").read_bytes() == serial[name], name
                assert serial[name] != plain["C_mode=16x_alpha=0.8_%s+%s.jpg" % (a, b)], name
    styles = "%s,%s" % (s / "s1.png", s / "s2.png")
    _, reg_plain = run_cli("regions_plain", "--maskPath", str(m), "--region_styles", styles)
    _, reg = run_cli("regions", "--maskPath", str(m), "--region_styles", styles, "--preserve_color", "luma")
    assert sorted(reg) == ["C_mode=16x_alpha=0.8_color=luma_c1+regions.jpg", "C_mode=16x_alpha=0.8_color=luma_c2+regions.jpg"]
    assert all(reg[k] != reg_plain[k.replace("color=luma_", "")] for k in reg)
    _, itp = run_cli("interp", "--interp_styles", styles, "--interp_weights", "2,1", "--preserve_color", "luma")
    assert sorted(itp) == ["C_mode=16x_alpha=0.8_color=luma_c1+interp.jpg", "C_mode=16x_alpha=0.8_color=luma_c2+interp.jpg"]
    with pytest.raises(ValueError, match="--maskPath"):
        run_cli("refused", "--maskPath", str(m), "--region_styles", styles, "--preserve_color", "match")
