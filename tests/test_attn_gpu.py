"""Attention statistics on the device (include/wct_hip_attn.h): wct_attn_stats against the numpy fp64 reference (tests/attn_oracle.py) under a
gate made of the reference's own fp32 error, position / chunk independence bit for bit, NaN propagation, wct_attn_apply bit for bit,
wct_attn_project and wct_attn_level against fp64, wct_stylize_attn against the public calls it is made of (bit for bit), allocation and graph
capture, history independence, the refusals, and the command line's --swap_match attention.

The module imports without a GPU."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from tests import attn_cases as AC
from tests import attn_oracle as A
from tests import state_cases as sc
from tests.conftest import PKG, REPO
from wct_hip import lib as _lib

pytestmark = pytest.mark.gpu

# Gate of wct_attn_stats: 4 x (the plain-fp32 arm's error against fp64, same measure, computed in the test) + a floor.
# Measured on the MI355X over STATS_SHAPES x TAUS (the full table is in DESIGN.md, "Attention statistics"): the kernel's error is between
# 0.2 x and 2.2 x the fp32 arm's and nowhere above 4 e32, so the excess the floor is made of is the kernel's error beyond the fp32 arm's
# OWN error (err - e32 where positive).  Largest: mean 6.527e-7 against 4.483e-7 at 7x9 / 5x6 / C = 8, tau = 32 (2.04e-7); var 3.713e-7
# against 1.824e-7 at 3x3 / 1x2 / C = 4, tau = 4 (1.89e-7).  Floor = 2 x that; the project's cascade floor 1e-4 is 250 times further out.
FLOOR_MEAN = 4.1e-7
FLOOR_VAR = 3.8e-7
assert max(FLOOR_MEAN, FLOOR_VAR) <= 1e-4
LEVEL_FLOOR = 1e-4          # the cascade gate the project already uses


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


def gpu_stats(torch, eng, q, k, v, tau):
    m, var = eng.attn_stats(cu(torch, q), cu(torch, k), cu(torch, v), tau)
    torch.cuda.synchronize()
    return m.cpu().numpy(), var.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- 1. statistics against fp64
_REF = {}


def stats_reference(shape, tau):
    """(q, k, v, (mean64, var64), (e32 of the mean, e32 of the var)) -- computed once per case and left unchanged."""
    key = (shape, tau)
    if key not in _REF:
        q, k, v = AC.stats_inputs(*shape)
        m64, v64 = A.stats(q, k, v, tau)
        m32, v32 = A.stats(q, k, v, tau, np.float32)
        vmax = float(np.abs(v).max())
        _REF[key] = (q, k, v, (m64, v64), (np.abs(m32 - m64).max() / vmax, np.abs(v32 - v64).max() / vmax ** 2))
    return _REF[key]


@pytest.mark.parametrize("tau", AC.TAUS)
@pytest.mark.parametrize("shape", AC.STATS_SHAPES, ids=lambda s: "%dx%d_%dx%d_C%d" % s)
def test_stats_against_fp64(torch, wct, shape, tau):
    """max |mean - mean64| / max |V| and max |var - var64| / max |V|^2 within 4 e32 + floor.  A padded key that is counted moves the mean by
    1 / Nk at tau = 0; a single-f16 P or V is 1e-3 off.  Measured on the MI355X: see FLOOR_MEAN / FLOOR_VAR above."""
    q, k, v, (m64, v64), (e32m, e32v) = stats_reference(shape, tau)
    m, var = gpu_stats(torch, wct, q, k, v, tau)
    vmax = float(np.abs(v).max())
    em, ev = np.abs(m - m64).max() / vmax, np.abs(var - v64).max() / vmax ** 2
    print("stats %s tau=%g: mean %.3e (fp32 arm %.3e) var %.3e (fp32 arm %.3e)" % (shape, tau, em, e32m, ev, e32v))
    assert np.isfinite(m).all() and np.isfinite(var).all() and (var >= 0).all()
    assert em <= 4 * e32m + FLOOR_MEAN, "mean: %.3e against 4 x %.3e + %.1e" % (em, e32m, FLOOR_MEAN)
    assert ev <= 4 * e32v + FLOOR_VAR, "var: %.3e against 4 x %.3e + %.1e" % (ev, e32v, FLOOR_VAR)
    assert wct.saturation_count() == 0


def test_large_values_keep_their_relative_accuracy(torch, wct):
    """V scaled by 2^12 (|V| up to ~3e4, V^2 up to ~8e8: past every fixed f16 scale): the scale of V^2 follows the map, so the statistics
    of the scaled map meet the same gate against fp64, relative to the scaled maxima."""
    shape, tau, s = AC.STATS_SHAPES[1], 4.0, np.float32(4096)
    q, k, v, (m64, v64), (e32m, e32v) = stats_reference(shape, tau)
    assert np.abs(v).max() * s < 65504
    m, var = gpu_stats(torch, wct, q, k, v * s, tau)
    vmax = float(np.abs(v).max()) * float(s)
    em, ev = np.abs(m - m64 * float(s)).max() / vmax, np.abs(var - v64 * float(s) ** 2).max() / vmax ** 2
    print("stats of 4096 V: mean %.3e var %.3e" % (em, ev))
    assert em <= 4 * e32m + FLOOR_MEAN and ev <= 4 * e32v + FLOOR_VAR
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 2. position and chunking
def duplicate_case():
    """203 queries of which rows 3, 77, 150 and 202 are one row and rows 64 and 65 another; 21 x 18 keys, C = 36."""
    q, k, v = AC.stats_inputs(29, 7, 21, 18, 36)
    q = np.ascontiguousarray(q[:203])
    q[[77, 150, 202]] = q[3]
    q[65] = q[64]
    return q, k, v


def test_duplicate_query_rows_give_bitwise_equal_rows(torch, wct):
    q, k, v = duplicate_case()
    for tau in (4.0, 32.0):
        m, var = gpu_stats(torch, wct, q, k, v, tau)
        for rows in ([3, 77, 150, 202], [64, 65]):
            for r in rows[1:]:
                assert np.array_equal(m[r].view(np.int32), m[rows[0]].view(np.int32)), (tau, r)
                assert np.array_equal(var[r].view(np.int32), var[rows[0]].view(np.int32)), (tau, r)
        assert not np.array_equal(m[3], m[4])


def test_query_chunking_does_not_change_a_bit(torch):
    """attn_query_chunk = 64 (four launches, borders on tile borders), = 50 and = 7 (borders inside tiles: the tiling shifts) against
    the single launch, on the duplicate case and on the C = 512 case (value slabs).  In a child process: the key needs WCT_DEBUG."""
    code = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
from tests import attn_cases as AC, state_cases as sc
from tests import test_attn_gpu as T
eng = sc.make_engine("16x")
cases = [T.duplicate_case(), AC.stats_inputs(*AC.STATS_SHAPES[3])]
run = lambda q, k, v: eng.attn_stats(T.cu(torch, q), T.cu(torch, k), T.cu(torch, v), 8.0)
want = [run(*c) for c in cases]
for chunk in (64, 50, 7):
    eng.debug_set("attn_query_chunk", chunk)
    for c, (wm, wv) in zip(cases, want):
        gm, gv = run(*c)
        assert torch.equal(gm.view(torch.int32), wm.view(torch.int32)) and torch.equal(gv.view(torch.int32), wv.view(torch.int32)), chunk
eng.debug_set("attn_query_chunk", 0)
assert eng.saturation_count() == 0
print("CHUNK_OK")
""" % (REPO, PKG)
    env = dict(os.environ, WCT_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "CHUNK_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def test_query_chunk_override_needs_the_debug_switch(wct, monkeypatch):
    monkeypatch.delenv("WCT_DEBUG", raising=False)
    with pytest.raises(ValueError, match="attn_query_chunk"):
        wct.debug_set("attn_query_chunk", 64)


# ---------------------------------------------------------------------------------------------------------------- 3. NaN, 4. apply
def test_a_nan_value_makes_nan_where_the_header_says_and_raises_no_flag(torch, wct):
    """NaN in V[k, c] -> mean[:, c] and var[:, c] of every query are NaN; every other output keeps its bits; the range flag stays 0."""
    q, k, v = AC.stats_inputs(*AC.STATS_SHAPES[1])
    clean_m, clean_v = gpu_stats(torch, wct, q, k, v, 4.0)
    bad = v.copy()
    kk, c = 100, 17
    bad[kk, c] = np.nan
    m, var = gpu_stats(torch, wct, q, k, bad, 4.0)
    assert np.isnan(m[:, c]).all() and np.isnan(var[:, c]).all()
    others = np.arange(v.shape[1]) != c
    assert np.array_equal(m[:, others].view(np.int32), clean_m[:, others].view(np.int32))
    assert np.array_equal(var[:, others].view(np.int32), clean_v[:, others].view(np.int32))
    badq = q.copy()
    badq[5, 2] = np.nan                           # a query row: its own outputs, nothing else
    m, var = gpu_stats(torch, wct, badq, k, v, 4.0)
    assert np.isnan(m[5]).all() and np.isnan(var[5]).all()
    rest = np.arange(q.shape[0]) != 5
    assert np.array_equal(m[rest].view(np.int32), clean_m[rest].view(np.int32)) and np.array_equal(var[rest].view(np.int32), clean_v[rest].view(np.int32))
    assert wct.saturation_count() == 0


@pytest.mark.parametrize("alpha", [1.0, 0.6])
@pytest.mark.parametrize("n,C", [(63, 8), (19 * 23, 36)])
def test_apply_is_the_fp32_emulation_bit_for_bit(torch, wct, n, C, alpha):
    rng = np.random.default_rng(n + C)
    m, z = (rng.standard_normal((n, C)).astype(np.float32) for _ in range(2))
    x = np.maximum(rng.standard_normal((n, C)), 0).astype(np.float32)
    v = (rng.random((n, C)) ** 4).astype(np.float32)
    v[::7, 1] = 0.0
    mu, sg = rng.standard_normal(C) * 3, rng.random(C) * 2 + 1e-3
    got = wct.attn_apply(cu(torch, m), cu(torch, v), cu(torch, z), cu(torch, x), cu(torch, mu, np.float64), cu(torch, sg, np.float64), alpha)
    want = A.apply_f32_emulation(m, v, z, x, mu, sg, alpha)
    assert tuple(got.shape) == (n, C)
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))


# ---------------------------------------------------------------------------------------------------------------- 5. projection
def swap_test_map(wct, side):
    """The maps the patch swap's level test whitens (tests/test_swap_gpu.py): relu3_1 of the packaged model for its two images."""
    img = sc.image(31, 64, 80) if side == "content" else sc.image(32, 72, 56)
    return wct.encode(3, img, layout="nhwc")[0].cpu().numpy()


@pytest.mark.parametrize("match,h,w,C", [("attention", 19, 23, 36), ("attention", 9, 11, 512), ("attention", 1, 2, 4),
                                          ("attention_whitened", "content", 0, 0), ("attention_whitened", "style", 0, 0)])
def test_project_against_fp64(torch, wct, match, h, w, C):
    """Unit rows and the standardised map against fp64 at 1e-6 of the largest value.  Standard domain: ReLU-like random maps; whitened: the
    patch swap's own test maps.  Measured on the MI355X: standard 1.5e-7 / 1.3e-7 / 1.8e-7 (unit) and 9.7e-8 / 1.2e-7 / 1.6e-7 (std);
    whitened, content map (16 x 20 x 64) 4.7e-8 (unit) / 7.6e-8 (std), style map (18 x 14 x 64) 5.9e-8 (unit) / 1.1e-7 (std).  The whitened
    map is W (x - mu) with the patch swap's W, centred and multiplied in fp64 (attn_whiten_kernel): the swap's own fp32 application of
    (W, -W mu) to the un-centred map measured 8.3e-7 and 1.09e-6 here, and a numpy fp32 evaluation of it 1.12e-6 and 1.10e-6."""
    if match == "attention":
        f = A.relu_map(h * w + C, h, w, C)
    else:
        f = swap_test_map(wct, h)
        h, w, C = f.shape
    unit, std = wct.attn_project(cu(torch, f)[None], match)
    only = wct.attn_project(cu(torch, f)[None], match, want_std=False)
    assert torch.equal(only, unit)
    u64, s64 = A.project(f, _lib.ATTN_MATCHES[match])
    eu = np.abs(unit[0].cpu().numpy() - u64).max() / np.abs(u64).max()
    es = np.abs(std[0].cpu().numpy() - s64).max() / np.abs(s64).max()
    print("project %s %dx%d C=%d: unit %.3e std %.3e" % (match, h, w, C, eu, es))
    assert eu <= 1e-6 and es <= 1e-6
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 6. one level
@pytest.fixture(scope="module")
def level_engines():
    cache = {}

    def get(model):
        if model not in cache:
            cache[model] = sc.make_engine("16x" if model == "16x" else "wide", w=AC.model_weights(model))
        return cache[model]
    return get


@pytest.mark.parametrize("model,level,domain", AC.LEVEL_CASES)
def test_one_level_against_the_fp64_composition(torch, level_engines, model, level, domain):
    """wct_attn_level on stand-in models (the shipped 16x widths; the un-pruned widths, C = 128 / 512) against encoder -> statistics -> apply
    -> decoder in fp64: max |image - ref| / max |ref| within 4 e32 + 1e-4, e32 the same pipeline in fp32.  The cases' input condition
    (min var >= 1e-4) is asserted by tests/test_attn_cpu.py on exactly these cases."""
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
    print("level %s %d domain %d: %.3e (fp32 arm %.3e)" % (model, level, domain, err, e32))
    assert tuple(got.shape) == (1,) + ref.shape
    assert err <= 4 * e32 + LEVEL_FLOOR
    assert eng.saturation_count() == 0


def test_level_is_the_composition_of_the_public_calls(torch, wct):
    """encode, wct_attn_project x 2, wct_moments, wct_attn_stats, wct_attn_apply, decode: the statistics bit for bit, the image within the
    rounding of (mu_s, sigma_s) made on the host side of this test."""
    c, s = sc.image(31, 64, 80), sc.image(32, 72, 56)
    cF, sF = wct.encode(3, c, layout="nhwc"), wct.encode(3, s, layout="nhwc")
    qhat, cstd = wct.attn_project(cF, "attention")
    khat, sstd = wct.attn_project(sF, "attention")
    m, var = wct.attn_stats(qhat, khat, sstd, 4.0)
    n, sm, ss = wct.moments(sF)
    mu = sm / n
    sigma = torch.sqrt(torch.clamp((torch.diagonal(ss) - n * mu * mu) / (n - 1.0), min=0.0) + _lib.ADAIN_EPS)
    csF = wct.attn_apply(m, var, cstd, cF, mu, sigma, 0.6)
    img = wct.decode(3, csF, layout="nhwc")
    got = wct.attn_level(3, c, s, "attention", 4.0, 0.6)
    assert tuple(got.shape) == (1, 3, 64, 80)
    assert float((got - img).abs().max()) <= 1e-5 * float(img.abs().max())


# ---------------------------------------------------------------------------------------------------------------- 7. bitwise composition
def compose_cascade(eng, c, s, attn_level, match, tau, alpha, runs):
    img = c
    for _ in range(runs):
        for level in (5, 4, 3, 2, 1):
            img = eng.attn_level(level, img, s, match, tau, alpha) if level == attn_level else eng.style_transfer_level(level, img, s, alpha)
    return img


@pytest.mark.parametrize("transform", ["wct", "adain"])
def test_stylize_attn_is_the_composition_of_the_public_calls(torch, transform):
    eng = sc.make_engine("16x")
    eng.set_transform(transform)
    c, s = sc.image(41, 80, 96), sc.image(42, 64, 72)
    plain = eng.stylize(c, s, alpha=0.6).clone()
    for level, match, tau in ((3, "attention", 8.0), (4, "attention_whitened", 4.0), (5, "attention", 0.0)):
        for runs in (1, 2):
            want = compose_cascade(eng, c, s, level, match, tau, 0.6, runs).clone()
            got = eng.stylize_attn(c, s, level, match, tau, alpha=0.6, num_run=runs)
            assert tuple(got.shape) == (1, 3, 80, 96)
            assert torch.equal(got, want), (transform, level, match, runs)
            assert bool(torch.isfinite(got).all()) and not torch.equal(got, plain)
    out = torch.empty((3, 80, 96), device="cuda")
    r = eng.stylize_attn(c, s, 5, "attention", 0.0, alpha=0.6, num_run=2, out=out)
    assert r.data_ptr() == out.data_ptr() and torch.equal(r, want)
    assert eng.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 8. allocation, 9. graph capture
def test_second_call_of_a_size_allocates_nothing(torch):
    eng = sc.make_engine("16x")
    c, s = sc.image(1, 250, 333), sc.image(2, 200, 160)
    q, k, v = (cu(torch, a) for a in AC.stats_inputs(*AC.STATS_SHAPES[1]))
    f = sc.feature(3, 40, 50, 64)
    combos = [(5, "attention_whitened"), (4, "attention"), (3, "attention_whitened"), (2, "attention")]
    for level, match in combos:
        eng.stylize_attn(c, s, level, match)
        eng.attn_level(level, c, s, match)
    eng.attn_stats(q, k, v, 4.0)
    eng.attn_project(f, "attention_whitened")
    eng.attn_project(f, "attention", want_std=False)
    allocs = eng.debug_get("ws_allocs")
    for level, match in combos:
        eng.stylize_attn(c, s, level, match, tau=2.0, alpha=0.6, num_run=2)
        eng.attn_level(level, c, s, match, alpha=0.3)
    eng.stylize_attn(sc.image(5, 120, 200), sc.image(6, 90, 100), 3, "attention_whitened")          # smaller: nothing either
    eng.attn_stats(q, k, v, 32.0)
    eng.attn_project(f, "attention_whitened")
    eng.attn_project(f, "attention", want_std=False)
    torch.cuda.synchronize()
    assert eng.debug_get("ws_allocs") == allocs
    assert eng.saturation_count() == 0


def test_stylize_attn_is_capturable_into_a_hip_graph():
    """wct_stylize_attn never synchronises and allocates nothing after the first call of a size: captured after a warm-up, one replay gives
    the eager bytes.  In a fresh process: a failed capture can leave the runtime in capture mode."""
    code = r"""
import sys
sys.path[:0] = [%r, %r]
import torch
from tests import state_cases as sc
wct = sc.make_engine("16x")
c1, s1 = sc.image(1, 144, 176), sc.image(3, 112, 128)
for level, match in ((3, "attention_whitened"), (4, "attention")):
    want = wct.stylize_attn(c1, s1, level, match, 4.0, alpha=0.6).clone()
    c, s = c1.clone(), s1.clone()
    out = torch.empty((3, 144, 176), device="cuda")
    wct.stylize_attn(c, s, level, match, 4.0, alpha=0.6, out=out)      # warm-up on the buffers the graph will use
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        wct.stylize_attn(c, s, level, match, 4.0, alpha=0.6, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(1, 3, 144, 176), want), match + ": the replay differs"
assert wct.saturation_count() == 0
print("GRAPH_OK")
""" % (REPO, PKG)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "GRAPH_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------------------- 10. history independence
def _h_stats(eng, seed):
    import torch as t
    q, k, v = (cu(t, a) for a in AC.stats_inputs(19, 23, 21, 18, 36))
    m, var = eng.attn_stats(q, k, v, 8.0)
    u, sd = eng.attn_project(sc.feature(seed, 19, 23, 36), "attention_whitened")
    return {"mean": m, "var": var, "unit": u, "std": sd}


def _h_level(eng, seed):
    H, W, Hs, Ws = sc.SIZES["small"]
    c, s = sc.image(seed, H, W), sc.image(seed + 1, Hs, Ws)
    return {"l3_whitened": eng.attn_level(3, c, s, "attention_whitened", 8.0), "l4_a06": eng.attn_level(4, c, s, "attention", 4.0, alpha=0.6)}


def _h_stylize(eng, seed):
    H, W, Hs, Ws = sc.SIZES["small"]
    c, s = sc.image(seed, H, W), sc.image(seed + 1, Hs, Ws)
    return {"l4": eng.stylize_attn(c, s, 4), "l3_whitened_a06_run2": eng.stylize_attn(c, s, 3, "attention_whitened", 4.0, alpha=0.6, num_run=2)}


CASES = {"attn_stats": _h_stats, "attn_level": _h_level, "stylize_attn": _h_stylize}
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
            cache[name] = CASES[name](eng, sc.SEED)
            torch.cuda.synchronize()
            assert eng.saturation_count() == 0
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_history_fresh_engine_against_an_engine_with_a_past(torch, controls, name):
    eng = sc.make_engine("16x")
    for past in PAST:
        sc.run(eng, past)
    for other in CASES:                      # ... and the other attention entries, with other inputs
        if other != name:
            CASES[other](eng, sc.SEED + 7)
    eng.stylize_swap(sc.image(3, 120, 200), sc.image(4, 90, 100), 3, "whitened")      # the patch swap shares the whitening's buffers
    same(torch, CASES[name](eng, sc.SEED), controls(name), "%s after %s" % (name, ", ".join(PAST)))
    same(torch, CASES[name](eng, sc.SEED), controls(name), "%s a second time" % name)
    assert eng.saturation_count() == 0


@pytest.mark.parametrize("byte", [0xFF, 0x3C], ids=["ff", "3c"])
@pytest.mark.parametrize("name", list(CASES))
def test_history_poisoned_scratch(torch, controls, name, byte):
    eng = sc.make_engine("16x")
    eng.debug_set("poison", byte)
    same(torch, CASES[name](eng, sc.SEED), controls(name), "%s, poison 0x%02X on a fresh engine" % (name, byte))
    sc.run(eng, "stylize/small")
    eng.debug_set("poison", byte)
    same(torch, CASES[name](eng, sc.SEED), controls(name), "%s, poison 0x%02X again after stylize/small" % (name, byte))
    eng.debug_set("poison", -1)
    assert eng.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 11. refusals, command line
def test_refusals_name_the_entry_and_write_nothing(torch, wct):
    L, ctx = wct._lib, wct._ctx
    wct._stream()
    C, nq, nk = 8, 42, 45
    q = torch.rand((nq, C), device="cuda")
    k = torch.rand((nk, C), device="cuda")
    v = torch.rand((nk, C), device="cuda")
    keep = [t.clone() for t in (q, k, v)]
    o1 = torch.full((nq, C), -3.0, device="cuda")
    o2 = torch.full((nq, C), -3.0, device="cuda")
    o3 = torch.full((nq, C), -3.0, device="cuda")
    mu = torch.zeros(C, device="cuda", dtype=torch.float64)
    sg = torch.ones(C, device="cuda", dtype=torch.float64)
    img = torch.rand((3, 48, 64), device="cuda")
    sty = torch.rand((3, 40, 48), device="cuda")
    outf = torch.full((3 * 48 * 64,), -3.0, device="cuda")
    p = lambda x: x.data_ptr()
    ho, wo = ctypes.c_int(-1), ctypes.c_int(-1)
    inf, nan = float("inf"), float("nan")
    pr = lambda *a: L.wct_attn_project(ctx, *a)
    st = lambda *a: L.wct_attn_stats(ctx, *a)
    ap = lambda *a: L.wct_attn_apply(ctx, *a)
    lv = lambda *a: L.wct_attn_level(ctx, *a, ctypes.byref(ho), ctypes.byref(wo))
    sa = lambda *a: L.wct_stylize_attn(ctx, *a, ctypes.byref(ho), ctypes.byref(wo))
    refusals = [
        ("wct_attn_project", lambda: pr(None, 6, 7, C, 0, p(o1), p(o2))),
        ("wct_attn_project", lambda: pr(p(q), 6, 7, C, 0, None, p(o2))),
        ("wct_attn_project", lambda: pr(p(q), 1, 1, C, 0, p(o1), p(o2))),               # one position: no unbiased variance
        ("wct_attn_project", lambda: pr(p(q), 6, 0, C, 0, p(o1), p(o2))),
        ("wct_attn_project", lambda: pr(p(q), 6, 7, 6, 0, p(o1), p(o2))),               # C not a multiple of 4
        ("wct_attn_project", lambda: pr(p(q), 6, 7, 516, 0, p(o1), p(o2))),
        ("wct_attn_project", lambda: pr(p(q), 6, 7, C, 2, p(o1), p(o2))),
        ("wct_attn_project", lambda: pr(p(q), 6, 7, C, -1, p(o1), p(o2))),
        ("wct_attn_project", lambda: pr(p(q) + 4, 6, 7, C, 0, p(o1), p(o2))),           # not 16-byte aligned
        ("wct_attn_project", lambda: pr(p(q), 6, 7, C, 0, p(q) + 64, p(o2))),           # unit_out inside feat
        ("wct_attn_project", lambda: pr(p(q), 6, 7, C, 0, p(o1), p(o1))),               # std_out is unit_out
        ("wct_attn_stats", lambda: st(None, nq, p(k), p(v), nk, C, 4.0, p(o1), p(o2))),
        ("wct_attn_stats", lambda: st(p(q), nq, None, p(v), nk, C, 4.0, p(o1), p(o2))),
        ("wct_attn_stats", lambda: st(p(q), nq, p(k), None, nk, C, 4.0, p(o1), p(o2))),
        ("wct_attn_stats", lambda: st(p(q), nq, p(k), p(v), nk, C, 4.0, None, p(o2))),
        ("wct_attn_stats", lambda: st(p(q), nq, p(k), p(v), nk, C, 4.0, p(o1), None)),
        ("wct_attn_stats", lambda: st(p(q), 1, p(k), p(v), nk, C, 4.0, p(o1), p(o2))),
        ("wct_attn_stats", lambda: st(p(q), nq, p(k), p(v), 1, C, 4.0, p(o1), p(o2))),
        ("wct_attn_stats", lambda: st(p(q), nq, p(k), p(v), -5, C, 4.0, p(o1), p(o2))),
        ("wct_attn_stats", lambda: st(p(q), nq, p(k), p(v), nk, 10, 4.0, p(o1), p(o2))),
        ("wct_attn_stats", lambda: st(p(q), nq, p(k), p(v), nk, C, -0.5, p(o1), p(o2))),
        ("wct_attn_stats", lambda: st(p(q), nq, p(k), p(v), nk, C, 32.5, p(o1), p(o2))),
        ("wct_attn_stats", lambda: st(p(q), nq, p(k), p(v), nk, C, nan, p(o1), p(o2))),
        ("wct_attn_stats", lambda: st(p(q), nq, p(k), p(v), nk, C, inf, p(o1), p(o2))),
        ("wct_attn_stats", lambda: st(p(q), nq, p(k) + 8, p(v), nk, C, 4.0, p(o1), p(o2))),
        ("wct_attn_stats", lambda: st(p(q), nq, p(k), p(v), nk, C, 4.0, p(q), p(o2))),         # mean is the query map
        ("wct_attn_stats", lambda: st(p(q), nq, p(k), p(v), nk, C, 4.0, p(o1), p(v) + 32)),    # var inside the values
        ("wct_attn_stats", lambda: st(p(q), nq, p(k), p(v), nk, C, 4.0, p(o1), p(o1))),        # var is mean
        ("wct_attn_apply", lambda: ap(None, p(o2), p(q), p(q), nq, C, p(mu), p(sg), 0.5, p(o3))),
        ("wct_attn_apply", lambda: ap(p(o1), p(o2), p(q), p(q), nq, C, None, p(sg), 0.5, p(o3))),
        ("wct_attn_apply", lambda: ap(p(o1), p(o2), p(q), p(q), nq, C, p(mu), p(sg), 0.5, None)),
        ("wct_attn_apply", lambda: ap(p(o1), p(o2), p(q), p(q), 0, C, p(mu), p(sg), 0.5, p(o3))),
        ("wct_attn_apply", lambda: ap(p(o1), p(o2), p(q), p(q), nq, 2, p(mu), p(sg), 0.5, p(o3))),
        ("wct_attn_apply", lambda: ap(p(o1), p(o2), p(q), p(q), nq, C, p(mu), p(sg), nan, p(o3))),
        ("wct_attn_apply", lambda: ap(p(o1), p(o2), p(q), p(q), nq, C, p(mu), p(sg), inf, p(o3))),
        ("wct_attn_apply", lambda: ap(p(o1), p(o2), p(q), p(q), nq, C, p(mu), p(sg), 0.5, p(o3) + 4)),
        ("wct_attn_apply", lambda: ap(p(o1), p(o2), p(q), p(q), nq, C, p(mu), p(sg), 0.5, p(o1))),   # out is the mean
        ("wct_attn_apply", lambda: ap(p(o1), p(o2), p(q), p(q), nq, C, p(mu), p(sg), 0.5, p(q))),    # out is the content
        ("wct_attn_level", lambda: lv(3, None, 48, 64, p(sty), 40, 48, 0, 4.0, 1.0, p(outf))),
        ("wct_attn_level", lambda: lv(3, p(img), 48, 64, None, 40, 48, 0, 4.0, 1.0, p(outf))),
        ("wct_attn_level", lambda: lv(3, p(img), 48, 64, p(sty), 40, 48, 0, 4.0, 1.0, None)),
        ("wct_attn_level", lambda: lv(1, p(img), 48, 64, p(sty), 40, 48, 0, 4.0, 1.0, p(outf))),
        ("wct_attn_level", lambda: lv(6, p(img), 48, 64, p(sty), 40, 48, 0, 4.0, 1.0, p(outf))),
        ("wct_attn_level", lambda: lv(3, p(img), 48, 64, p(sty), 40, 48, 2, 4.0, 1.0, p(outf))),
        ("wct_attn_level", lambda: lv(3, p(img), 48, 64, p(sty), 40, 48, 0, 33.0, 1.0, p(outf))),
        ("wct_attn_level", lambda: lv(3, p(img), 48, 64, p(sty), 40, 48, 0, nan, 1.0, p(outf))),
        ("wct_attn_level", lambda: lv(3, p(img), 48, 64, p(sty), 40, 48, 0, 4.0, nan, p(outf))),
        ("wct_attn_level", lambda: lv(3, p(img), 0, 64, p(sty), 40, 48, 0, 4.0, 1.0, p(outf))),
        ("wct_attn_level", lambda: lv(5, p(img), 48, 64, p(sty), 16, 16, 0, 4.0, 1.0, p(outf))),    # a 1 x 1 style map at level 5
        ("wct_stylize_attn", lambda: sa(None, 48, 64, p(sty), 40, 48, 3, 0, 4.0, 1.0, 1, p(outf))),
        ("wct_stylize_attn", lambda: sa(p(img), 48, 64, None, 40, 48, 3, 0, 4.0, 1.0, 1, p(outf))),
        ("wct_stylize_attn", lambda: sa(p(img), 48, 64, p(sty), 40, 48, 3, 0, 4.0, 1.0, 1, None)),
        ("wct_stylize_attn", lambda: sa(p(img), 48, 64, p(sty), 40, 48, 3, 0, 4.0, 1.0, 0, p(outf))),
        ("wct_stylize_attn", lambda: sa(p(img), 48, 64, p(sty), 40, 48, 1, 0, 4.0, 1.0, 1, p(outf))),
        ("wct_stylize_attn", lambda: sa(p(img), 48, 64, p(sty), 40, 48, 3, -1, 4.0, 1.0, 1, p(outf))),
        ("wct_stylize_attn", lambda: sa(p(img), 48, 64, p(sty), 40, 48, 3, 0, -1.0, 1.0, 1, p(outf))),
        ("wct_stylize_attn", lambda: sa(p(img), 48, 64, p(sty), 40, 48, 3, 0, 4.0, inf, 1, p(outf))),
        ("wct_stylize_attn", lambda: sa(p(img), 8, 64, p(sty), 40, 48, 3, 0, 4.0, 1.0, 1, p(outf))),
    ]
    for i, (name, call) in enumerate(refusals):
        assert call() == _lib.WCT_ERR_INVALID, (i, name)
        msg = L.wct_last_error(ctx).decode()
        assert name in msg, (i, name, msg)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((q, k, v), keep))
    assert all(bool((t == -3.0).all()) for t in (o1, o2, o3, outf)) and (ho.value, wo.value) == (-1, -1)
    # the Python surface refuses the same way
    with pytest.raises(ValueError, match="match"):
        wct.attn_level(3, img[None], sty[None], "whitened")
    with pytest.raises(ValueError, match="match"):
        wct.stylize_attn(img[None], sty[None], 3, "cosine")
    with pytest.raises(ValueError):
        wct.stylize_attn(img[None], sty[None], 1)
    with pytest.raises(ValueError):
        wct.attn_stats(q, k, torch.rand((nk, 12), device="cuda"), 4.0)
    assert wct.saturation_count() == 0


def test_cli_swap_match_attention(torch, tmp_path):
    """One content x one style: --swap_level 4 --swap_match attention --swap_temp 6 writes a file whose bytes are those of stylize_attn + to_u8
    saved through the same Pillow call."""
    Image = pytest.importorskip("PIL.Image")
    from wct_hip import WCT, cli
    c, s = tmp_path / "content", tmp_path / "style"
    c.mkdir(); s.mkdir()
    rng = np.random.default_rng(9)
    for path, (h, w) in ((c / "c1.png", (100, 132)), (s / "s1.png", (90, 84))):
        img = rng.random(((h + 3) // 4, (w + 3) // 4, 3)).repeat(4, 0).repeat(4, 1)[:h, :w] * 0.8 + rng.random((h, w, 3)) * 0.2
        Image.fromarray((img * 255).astype(np.uint8)).save(path)
    o = tmp_path / "out"
    assert cli.main(["--mode", "16x", "--contentPath", str(c), "--stylePath", str(s), "--outf", str(o), "--log_mark", "C", "--alpha", "0.8",
                     "--swap_level", "4", "--swap_match", "attention", "--swap_temp", "6"]) == 0
    files = sorted(f for f in os.listdir(o) if f.endswith(".jpg"))
    assert files == ["C_mode=16x_alpha=0.8_swap=4_attention=6_c1+s1.jpg"]
    w = WCT(types.SimpleNamespace(mode="16x", alpha=0.8))
    cf = w.to_tensor_u8(torch.from_numpy(cli.load_rgb_u8(str(c / "c1.png"))).cuda())
    sf = w.to_tensor_u8(torch.from_numpy(cli.load_rgb_u8(str(s / "s1.png"))).cuda())
    want = w.to_u8(w.stylize_attn(cf, sf, 4, "attention", 6.0, alpha=0.8), 0).cpu().numpy()
    Image.fromarray(want).save(tmp_path / "ref.jpg")
    assert (o / files[0]).read_bytes() == (tmp_path / "ref.jpg").read_bytes()
    log = open(o / "log_C_16x.txt").read()
    assert "attention statistics at level 4, attention, temperature 6" in log
