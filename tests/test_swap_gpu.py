"""Patch swap on the device (include/wct_hip_swap.h): wct_patch_match against planted matches and against the numpy fp64 reference
(tests/swap_oracle.py) under the gate of the f16x3 arithmetic, the tie rule and the independence of the key chunking, wct_patch_assemble
bit for bit against the fp32 emulation of its stated summation order, wct_swap_level against the fp64 decorator, wct_stylize_swap against
the public calls it is made of (bit for bit), allocation and graph capture, history independence with the helpers of
tests/state_cases.py, the refusals, and the command line's --swap_level.

The module imports without a GPU."""
import collections
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from tests import state_cases as sc
from tests import swap_oracle as O
from tests.conftest import PKG, REPO
from wct_hip import lib as _lib

pytestmark = pytest.mark.gpu


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


def normal(seed, h, w, C):
    return np.random.default_rng(seed).standard_normal((h, w, C)).astype(np.float32)


def gpu_match(torch, wct, Q, K):
    idx, best = wct.patch_match(cu(torch, Q)[None], cu(torch, K)[None], want_best=True)
    torch.cuda.synchronize()
    return idx.cpu().numpy().astype(np.int64), best.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- 1. planted matches
# (key map hs x ws, C, crop offset, query map h x w): the issue's key maps 21x18, 12x14 and one-query crops of them, whole-map crops over
# more than one tile, and two long thin key maps for the 3x40 / 40x3 query maps (a crop needs a key map that holds it)
PLANTED = [
    (21, 18, 24, (7, 9), 3, 3), (12, 14, 512, (5, 2), 3, 3), (21, 18, 36, (2, 2), 19, 16), (12, 14, 128, (1, 3), 10, 11),
    (5, 43, 36, (1, 2), 3, 40), (44, 6, 24, (3, 2), 40, 3), (24, 27, 128, (4, 3), 19, 23), (3, 3, 24, (0, 0), 3, 3),
]


@pytest.mark.parametrize("hs,ws,C,off,h,w", PLANTED, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_planted_matches_are_found_exactly(torch, wct, hs, ws, C, off, h, w):
    """Q is a crop of a standard-normal key map (at a non-zero offset wherever the key map is larger than one patch): idx is the planted
    index for every query and best = |patch| to 1e-5 relative."""
    K = normal(hs * 1000 + ws + C, hs, ws, C)
    Q = np.ascontiguousarray(K[off[0]:off[0] + h, off[1]:off[1] + w])
    m = O.match(Q, K)
    assert (m.gap > 1e-2 * m.qnorm).all(), "the oracle's own top-2 gap"
    qy, qx = np.divmod(np.arange((h - 2) * (w - 2)), w - 2)
    planted = (qy + off[0]) * (ws - 2) + qx + off[1]
    assert np.array_equal(m.idx, planted)
    idx, best = gpu_match(torch, wct, Q, K)
    print("planted %dx%d in %dx%d C=%d: max rel |best - |patch|| = %.3e" % (h, w, hs, ws, C, np.abs(best / m.qnorm - 1).max()))
    assert np.array_equal(idx, planted)
    assert np.abs(best / m.qnorm - 1).max() <= 1e-5
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 2. random maps against fp64
# (query h x w, key hs x ws, C); maps are standard_normal from default_rng(C) (queries) and default_rng(C + 1) (keys)
RANDOM = [
    (19, 23, 21, 18, 24), (19, 23, 21, 18, 36), (19, 23, 21, 18, 128), (11, 13, 12, 14, 512),
    (3, 40, 12, 14, 36), (40, 3, 21, 18, 24), (3, 3, 3, 3, 128), (3, 3, 21, 18, 36), (19, 23, 3, 3, 24), (3, 40, 21, 18, 512),
]


def random_pair(h, w, hs, ws, C):
    return normal(C, h, w, C), normal(C + 1, hs, ws, C)


def check_against_fp64(m, idx, best, C, what):
    """The index criterion: where the fp64 top-2 gap is at least tau |patch_Q| the index is the oracle's; elsewhere the fp64 score of the
    chosen key is within tau |patch_Q| of the best, and those queries are at most 5 % (20 % at C = 512) of all."""
    t = O.tau(C) * m.qnorm
    clear = m.gap >= t
    n = len(idx)
    chosen = m.S[np.arange(n), idx]
    err = np.abs(best - chosen).max()
    print("%s: %d queries, %d keys, %.1f %% inside the gate's gap, max |best - fp64 score| = %.3e (tau |patch_Q| >= %.3e)"
          % (what, n, m.S.shape[1], 100.0 * (~clear).mean(), err, t.min()))
    assert ((idx >= 0) & (idx < m.S.shape[1])).all()
    assert np.array_equal(idx[clear], m.idx[clear]), "%s: %d clear queries differ" % (what, int((idx[clear] != m.idx[clear]).sum()))
    assert (m.best[~clear] - chosen[~clear] <= t[~clear]).all()
    assert (~clear).mean() <= (0.20 if C >= 512 else 0.05)
    assert (np.abs(best - chosen) <= t).all()
    return err


@pytest.mark.parametrize("h,w,hs,ws,C", RANDOM)
def test_random_maps_against_fp64(torch, wct, h, w, hs, ws, C):
    """Measured on the MI355X, max |best - fp64 score| per case in the order of RANDOM (scores are O(sqrt(9C)) here): 1.6e-6, 2.3e-6,
    3.5e-6, 4.7e-6, 7.1e-7, 1.0e-6, 3.6e-7, 6.5e-7, 8.6e-7, 6.0e-6 -- against tau |patch_Q| of 3.4e-4 (C = 24) to 3.7e-2 (C = 512); the
    share of queries inside the gate's gap is 0, 0, 1.7, 4.0, 0, 0, 0, 0, 0, 10.5 %; no clear query differs from fp64."""
    Q, K = random_pair(h, w, hs, ws, C)
    idx, best = gpu_match(torch, wct, Q, K)
    check_against_fp64(O.match(Q, K), idx, best, C, "random %dx%d vs %dx%d C=%d" % (h, w, hs, ws, C))
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 3. ties and chunking
def periodic_keys(C=36):
    return np.ascontiguousarray(np.tile(normal(77, 5, 6, C), (5, 3, 1))[:21, :18])


def test_lowest_index_wins_among_equal_patches(torch, wct):
    """A 5x6 block tiled to 21x18 holds every patch up to 12 times: a crop's queries get the lowest copy, and so does any query."""
    K = periodic_keys()
    rep = O.lowest_duplicate(K)
    Q = np.ascontiguousarray(K[6:6 + 13, 7:7 + 11])          # planted at (6, 7): copies at lower indices exist for every query
    idx, best = gpu_match(torch, wct, Q, K)
    qy, qx = np.divmod(np.arange(11 * 9), 9)
    assert np.array_equal(idx, ((qy + 6) % 5) * 16 + (qx + 7) % 6)
    Qr = normal(5, 19, 23, 36)
    m = O.match(Qr, K)
    idx, best = gpu_match(torch, wct, Qr, K)
    assert np.array_equal(idx, rep[idx]), "a chosen key has an equal patch at a lower index"
    # against fp64 on the distinct patches: the gap to the best OTHER patch, not to the winner's own copies
    S = m.S.copy()
    S[rep[None, :] == rep[m.idx][:, None]] = -np.inf
    gap = m.best - S.max(1)
    clear = gap >= O.tau(36) * m.qnorm
    assert clear.mean() >= 0.95 and np.array_equal(idx[clear], rep[m.idx][clear])


def test_key_chunking_does_not_change_a_bit(torch, tmp_path):
    """swap_key_chunk = 64 (5 launches over 304 keys, chunk borders inside key rows and inside tiles) and = 7 against the single-chunk
    run, on the periodic map (ties across chunks) and on a random case of test 2.  In a child process: the key needs WCT_DEBUG."""
    code = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
from tests import state_cases as sc
from tests import test_swap_gpu as T
eng = sc.make_engine("16x")
cases = [(T.normal(5, 19, 23, 36), T.periodic_keys()), T.random_pair(19, 23, 21, 18, 24), T.random_pair(3, 40, 21, 18, 512)]
want = [eng.patch_match(T.cu(torch, q)[None], T.cu(torch, k)[None], want_best=True) for q, k in cases]
for chunk in (64, 7):
    eng.debug_set("swap_key_chunk", chunk)
    for (q, k), (wi, wb) in zip(cases, want):
        gi, gb = eng.patch_match(T.cu(torch, q)[None], T.cu(torch, k)[None], want_best=True)
        assert torch.equal(gi, wi) and torch.equal(gb.view(torch.int32), wb.view(torch.int32)), chunk
eng.debug_set("swap_key_chunk", 0)
assert eng.saturation_count() == 0
print("CHUNK_OK")
""" % (REPO, PKG)
    env = dict(os.environ, WCT_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "CHUNK_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def test_key_chunk_override_needs_the_debug_switch(wct, monkeypatch):
    monkeypatch.delenv("WCT_DEBUG", raising=False)
    with pytest.raises(ValueError, match="swap_key_chunk"):
        wct.debug_set("swap_key_chunk", 64)


# ---------------------------------------------------------------------------------------------------------------- 4. assemble
@pytest.mark.parametrize("C", [24, 512])
@pytest.mark.parametrize("h,w,hs,ws", [(3, 3, 3, 3), (3, 3, 12, 14), (3, 40, 12, 14), (19, 23, 21, 18)])
def test_assemble_is_the_fp32_emulation_bit_for_bit(torch, wct, h, w, hs, ws, C):
    rng = np.random.default_rng(h * w + C)
    V, base = normal(1 + C, hs, ws, C), normal(2 + C, h, w, C)
    nq, nk = (h - 2) * (w - 2), (hs - 2) * (ws - 2)
    idx = rng.integers(0, nk, nq).astype(np.int32)
    idx[::3] = nk - 1                      # the last row and column of the key map, repeated
    if nq > 4:
        idx[1], idx[4] = 0, idx[2]
    for alpha, b in ((1.0, None), (0.6, base), (1.0, base), (0.0, base)):
        got = wct.patch_assemble(cu(torch, idx, np.int32), h, w, cu(torch, V)[None], None if b is None else cu(torch, b)[None], alpha)
        want = O.assemble(idx, h, w, V, b, alpha, dtype=np.float32)
        assert tuple(got.shape) == (1, h, w, C)
        assert np.array_equal(got[0].cpu().numpy().view(np.int32), want.view(np.int32)), (alpha, b is None)


# ---------------------------------------------------------------------------------------------------------------- 5. one level
def compose_level(torch, eng, level, c, s, match, alpha):
    """wct_swap_level as the public calls it is made of; returns (image, idx, best, csF, cF, sF)."""
    cF, sF = eng.encode(level, c, layout="nhwc"), eng.encode(level, s, layout="nhwc")
    C = int(cF.shape[3])
    q, k = cF, sF
    if match == "whitened":
        ident = torch.cat([torch.eye(C, dtype=torch.float64).reshape(-1), torch.zeros(C, dtype=torch.float64)]).cuda()
        proj = []
        for f in (cF, sF):
            n, sm, ss = eng.moments(f)
            M, b = eng.transform_solve("wct", n, sm, ss, ident, alpha=1.0)
            lab = torch.zeros((int(f.shape[1]), int(f.shape[2])), dtype=torch.uint8, device="cuda")
            proj.append(eng.apply_labeled(f, lab, M.reshape(1, C, C), b.reshape(1, C)))
        q, k = proj
    idx, best = eng.patch_match(q, k, want_best=True)
    csF = eng.patch_assemble(idx, int(cF.shape[1]), int(cF.shape[2]), sF, cF, alpha)
    return eng.decode(level, csF, layout="nhwc"), idx, best, csF, cF, sF


@pytest.mark.parametrize("match", ["whitened", "raw"])
def test_one_level_against_the_fp64_decorator(torch, wct, match):
    """Content 64x80, style 72x56, level 3 of the packaged model (16x20 and 18x14 maps of 64 channels).  wct_swap_level is bit for bit
    the composition of public calls, whose indices and blended feature are checked against the fp64 decorator fed with the GPU's own
    encoder features: the index criterion of the random-map test on the oracle's projected maps, and the blended feature within 1e-5
    relative wherever the indices agree.  The share of queries inside the gate's gap is capped as in the random-map test, so that the
    test cannot hide a failure: 5 % for whitened (measured 0 %).  For raw the cap is 20 %, NOT the 5 % the random-map test has for
    C <= 128: ReLU features are far from centred, so all scores of a query are close, and the fp64 oracle's OWN gaps -- evaluated on the
    CPU with the fp32 reference encoder, nothing of the library involved -- put 8.7 % of the 252 queries inside the gate's gap.  5 % is
    therefore unreachable whatever the kernel does; 20 % is the cap the random-map test uses for the one case whose oracle share is of
    that size (12 % at C = 512), i.e. about twice the oracle's own share."""
    c, s = sc.image(31, 64, 80), sc.image(32, 72, 56)
    alpha = 0.6
    got = wct.swap_level(3, c, s, match, alpha)
    img, idx, best, csF, cF, sF = compose_level(torch, wct, 3, c, s, match, alpha)
    assert tuple(got.shape) == (1, 3, 64, 80) and torch.equal(got, img), "wct_swap_level is not the composition of the public calls"
    cFn, sFn = cF[0].cpu().numpy(), sF[0].cpu().numpy()
    m, want, Q, K = O.decorate(cFn, sFn, match, alpha)
    idx, best = idx.cpu().numpy().astype(np.int64), best.cpu().numpy()
    C = cFn.shape[2]
    t = O.tau(C) * m.qnorm
    clear = m.gap >= t
    chosen = m.S[np.arange(len(idx)), idx]
    print("level 3 %s: %d queries, %d keys, %.1f %% inside the gate's gap, %d indices differ from fp64, max (best_fp64 - chosen) / (tau |q|) = %.3e"
          % (match, len(idx), m.S.shape[1], 100.0 * (~clear).mean(), int((idx != m.idx).sum()), ((m.best - chosen) / t).max()))
    assert np.array_equal(idx[clear], m.idx[clear]), "%d clear queries differ" % int((idx[clear] != m.idx[clear]).sum())
    assert (m.best[~clear] - chosen[~clear] <= t[~clear]).all()
    assert (~clear).mean() <= (0.05 if match == "whitened" else 0.20)
    # the blended feature where every covering query agrees with the oracle
    h, w = cFn.shape[:2]
    agree = (idx == m.idx).reshape(h - 2, w - 2)
    ok = np.ones((h, w), bool)
    for oy in range(3):
        for ox in range(3):
            ok[oy:oy + h - 2, ox:ox + w - 2] &= agree
    assert ok.any()
    g = csF[0].cpu().numpy()
    rel = np.abs(g[ok] - want[ok]).max() / np.abs(want).max()
    print("level 3 %s: blended feature rel err %.3e on %d of %d pixels" % (match, rel, int(ok.sum()), h * w))
    assert rel <= 1e-5
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 6. bitwise composition
def compose_cascade(eng, c, s, swap_level, match, alpha, runs):
    img = c
    for _ in range(runs):
        for level in (5, 4, 3, 2, 1):
            img = eng.swap_level(level, img, s, match, alpha) if level == swap_level else eng.style_transfer_level(level, img, s, alpha)
    return img


@pytest.mark.parametrize("transform", ["wct", "ot"])
def test_stylize_swap_is_the_composition_of_the_public_calls(torch, transform):
    eng = sc.make_engine("16x")
    eng.set_transform(transform)
    c, s = sc.image(41, 80, 96), sc.image(42, 64, 72)
    plain = eng.stylize(c, s, alpha=0.6).clone()
    for swap_level, match in ((3, "whitened"), (4, "raw"), (4, "whitened")):
        for runs in (1, 2):
            want = compose_cascade(eng, c, s, swap_level, match, 0.6, runs).clone()
            got = eng.stylize_swap(c, s, swap_level, match, alpha=0.6, num_run=runs)
            assert tuple(got.shape) == (1, 3, 80, 96)
            assert torch.equal(got, want), (transform, swap_level, match, runs)
            assert bool(torch.isfinite(got).all()) and not torch.equal(got, plain)
    out = torch.empty((3, 80, 96), device="cuda")
    r = eng.stylize_swap(c, s, 4, "whitened", alpha=0.6, num_run=2, out=out)
    assert r.data_ptr() == out.data_ptr() and torch.equal(r, want)
    assert eng.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 7. allocation, 8. graph capture
def test_second_call_of_a_size_allocates_nothing(torch):
    eng = sc.make_engine("16x")
    c, s = sc.image(1, 250, 333), sc.image(2, 200, 160)
    q, k = sc.feature(3, 40, 50, 64), sc.feature(4, 35, 45, 64)
    combos = [(5, "whitened"), (4, "raw"), (3, "whitened"), (2, "raw")]
    for level, match in combos:
        eng.stylize_swap(c, s, level, match)
        eng.swap_level(level, c, s, match)
    eng.patch_match(q, k)
    allocs = eng.debug_get("ws_allocs")
    for level, match in combos:
        eng.stylize_swap(c, s, level, match, alpha=0.6, num_run=2)
        eng.swap_level(level, c, s, match, alpha=0.3)
    eng.stylize_swap(sc.image(5, 120, 200), sc.image(6, 90, 100), 3, "whitened")          # smaller: nothing either
    eng.patch_match(q, k, want_best=True)
    torch.cuda.synchronize()
    assert eng.debug_get("ws_allocs") == allocs
    assert eng.saturation_count() == 0


def test_stylize_swap_is_capturable_into_a_hip_graph():
    """wct_stylize_swap never synchronises and allocates nothing after the first call of a size: captured after a warm-up, the graph
    replays the eager bits, also with other images in the same buffers.  In a fresh process: a failed capture can leave the runtime in
    capture mode."""
    code = r"""
import sys
sys.path[:0] = [%r, %r]
import torch
from tests import state_cases as sc
wct = sc.make_engine("16x")
c1, c2, s1, s2 = sc.image(1, 144, 176), sc.image(2, 144, 176), sc.image(3, 112, 128), sc.image(4, 112, 128)
for level, match in ((3, "whitened"), (4, "raw")):
    want1 = wct.stylize_swap(c1, s1, level, match, alpha=0.6).clone()
    want2 = wct.stylize_swap(c2, s2, level, match, alpha=0.6).clone()
    c, s = c1.clone(), s1.clone()
    out = torch.empty((3, 144, 176), device="cuda")
    wct.stylize_swap(c, s, level, match, alpha=0.6, out=out)      # warm-up on the buffers the graph will use
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        wct.stylize_swap(c, s, level, match, alpha=0.6, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(1, 3, 144, 176), want1), match + ": replay 1 differs"
    c.copy_(c2); s.copy_(s2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(1, 3, 144, 176), want2), match + ": replay 2 (new images, same graph) differs"
assert wct.saturation_count() == 0
print("GRAPH_OK")
""" % (REPO, PKG)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "GRAPH_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------------------- 9. history independence
Case = collections.namedtuple("Case", "fn covers size family")
CASES = collections.OrderedDict()


def case(family, covers):
    def deco(f):
        for size in ("small", "large"):
            CASES["%s/%s" % (family, size)] = Case((lambda eng, seed, _f=f, _s=size: _f(eng, seed, _s)), tuple(covers), size, family)
        return f
    return deco


FEATS = {"small": (19, 23, 21, 18, 36), "large": (75, 112, 65, 87, 64)}      # h, w, hs, ws, C


@case("patch_match", ["wct_patch_match"])
def _patch_match(eng, seed, size):
    h, w, hs, ws, C = FEATS[size]
    idx, best = eng.patch_match(sc.feature(seed, h, w, C), sc.feature(seed + 1, hs, ws, C), want_best=True)
    return {"idx": idx, "best": best}


@case("patch_assemble", ["wct_patch_assemble"])
def _patch_assemble(eng, seed, size):
    import torch as t
    h, w, hs, ws, C = FEATS[size]
    idx = t.randint(0, (hs - 2) * (ws - 2), ((h - 2) * (w - 2),), generator=sc._gen(seed), dtype=t.int32).cuda()
    v, base = sc.feature(seed + 1, hs, ws, C), sc.feature(seed + 2, h, w, C)
    return {"a1": eng.patch_assemble(idx, h, w, v), "a06": eng.patch_assemble(idx, h, w, v, base, 0.6)}


@case("swap_level", ["wct_swap_level"])
def _swap_level(eng, seed, size):
    H, W, Hs, Ws = sc.SIZES[size]
    c, s = sc.image(seed, H, W), sc.image(seed + 1, Hs, Ws)
    return {"l3_whitened": eng.swap_level(3, c, s, "whitened"), "l4_raw_a06": eng.swap_level(4, c, s, "raw", alpha=0.6)}


@case("stylize_swap", ["wct_stylize_swap"])
def _stylize_swap(eng, seed, size):
    H, W, Hs, Ws = sc.SIZES[size]
    c, s = sc.image(seed, H, W), sc.image(seed + 1, Hs, Ws)
    return {"l4_whitened": eng.stylize_swap(c, s, 4), "l3_raw_a06_run2": eng.stylize_swap(c, s, 3, "raw", alpha=0.6, num_run=2)}


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
    for other in CASES:                      # ... and the other swap entries at the other size
        if CASES[other].size != CASES[name].size and CASES[other].family != CASES[name].family:
            run(eng, other, sc.SEED + 7)
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


# ---------------------------------------------------------------------------------------------------------------- 10. refusals, command line
def test_refusals_name_the_entry_and_write_nothing(torch, wct):
    L, ctx = wct._lib, wct._ctx
    wct._stream()
    C = 8
    q = torch.rand((6, 7, C), device="cuda")
    k = torch.rand((5, 9, C), device="cuda")
    keep_q, keep_k = q.clone(), k.clone()
    img = torch.rand((3, 48, 64), device="cuda")
    sty = torch.rand((3, 40, 48), device="cuda")
    idx = torch.full((4 * 5,), -7, device="cuda", dtype=torch.int32)
    best = torch.full((4 * 5,), -3.0, device="cuda")
    outf = torch.full((3 * 48 * 64,), -3.0, device="cuda")
    p = lambda x: x.data_ptr()
    ho, wo = ctypes.c_int(-1), ctypes.c_int(-1)
    inf, nan = float("inf"), float("nan")
    pm = lambda *a: L.wct_patch_match(ctx, *a)
    pa = lambda *a: L.wct_patch_assemble(ctx, *a)
    sl = lambda *a: L.wct_swap_level(ctx, *a, ctypes.byref(ho), ctypes.byref(wo))
    ss = lambda *a: L.wct_stylize_swap(ctx, *a, ctypes.byref(ho), ctypes.byref(wo))
    refusals = [
        ("wct_patch_match", lambda: pm(None, 6, 7, p(k), 5, 9, C, p(idx), p(best))),
        ("wct_patch_match", lambda: pm(p(q), 6, 7, None, 5, 9, C, p(idx), p(best))),
        ("wct_patch_match", lambda: pm(p(q), 6, 7, p(k), 5, 9, C, None, p(best))),
        ("wct_patch_match", lambda: pm(p(q), 2, 7, p(k), 5, 9, C, p(idx), p(best))),
        ("wct_patch_match", lambda: pm(p(q), 6, 2, p(k), 5, 9, C, p(idx), p(best))),
        ("wct_patch_match", lambda: pm(p(q), 6, 7, p(k), 2, 9, C, p(idx), p(best))),
        ("wct_patch_match", lambda: pm(p(q), 6, 7, p(k), 5, -1, C, p(idx), p(best))),
        ("wct_patch_match", lambda: pm(p(q), 6, 7, p(k), 5, 9, 0, p(idx), p(best))),
        ("wct_patch_match", lambda: pm(p(q), 6, 7, p(k), 5, 9, 6, p(idx), p(best))),          # C not a multiple of 4
        ("wct_patch_match", lambda: pm(p(q), 6, 7, p(k), 5, 9, 516, p(idx), p(best))),
        ("wct_patch_match", lambda: pm(p(q), 6, 7, p(k), 46343, 46343, C, p(idx), p(best))),  # Nk >= 2^31
        ("wct_patch_match", lambda: pm(p(q) + 4, 6, 7, p(k), 5, 9, C, p(idx), p(best))),      # not 16-byte aligned
        ("wct_patch_match", lambda: pm(p(q), 6, 7, p(k), 5, 9, C, p(q) + 64, p(best))),       # idx inside the query map
        ("wct_patch_match", lambda: pm(p(q), 6, 7, p(k), 5, 9, C, p(idx), p(k))),             # best is the key map
        ("wct_patch_match", lambda: pm(p(q), 6, 7, p(k), 5, 9, C, p(idx), p(idx))),           # best is idx
        ("wct_patch_assemble", lambda: pa(None, 6, 7, p(k), 5, 9, C, p(q), 0.5, p(outf))),
        ("wct_patch_assemble", lambda: pa(p(idx), 6, 7, None, 5, 9, C, p(q), 0.5, p(outf))),
        ("wct_patch_assemble", lambda: pa(p(idx), 6, 7, p(k), 5, 9, C, p(q), 0.5, None)),
        ("wct_patch_assemble", lambda: pa(p(idx), 6, 7, p(k), 5, 9, C, None, 0.5, p(outf))),  # NULL base needs alpha == 1
        ("wct_patch_assemble", lambda: pa(p(idx), 6, 7, p(k), 5, 9, C, p(q), nan, p(outf))),
        ("wct_patch_assemble", lambda: pa(p(idx), 6, 7, p(k), 5, 9, C, p(q), inf, p(outf))),
        ("wct_patch_assemble", lambda: pa(p(idx), 2, 7, p(k), 5, 9, C, p(q), 0.5, p(outf))),
        ("wct_patch_assemble", lambda: pa(p(idx), 6, 7, p(k), 5, 2, C, p(q), 0.5, p(outf))),
        ("wct_patch_assemble", lambda: pa(p(idx), 6, 7, p(k), 5, 9, 10, p(q), 0.5, p(outf))),
        ("wct_patch_assemble", lambda: pa(p(idx), 6, 7, p(k), 5, 9, C, p(q), 0.5, p(k))),     # out is the value map
        ("wct_swap_level", lambda: sl(3, None, 48, 64, p(sty), 40, 48, 0, 1.0, p(outf))),
        ("wct_swap_level", lambda: sl(3, p(img), 48, 64, None, 40, 48, 0, 1.0, p(outf))),
        ("wct_swap_level", lambda: sl(3, p(img), 48, 64, p(sty), 40, 48, 0, 1.0, None)),
        ("wct_swap_level", lambda: sl(1, p(img), 48, 64, p(sty), 40, 48, 0, 1.0, p(outf))),   # level 1 is out of scope
        ("wct_swap_level", lambda: sl(6, p(img), 48, 64, p(sty), 40, 48, 0, 1.0, p(outf))),
        ("wct_swap_level", lambda: sl(3, p(img), 48, 64, p(sty), 40, 48, 2, 1.0, p(outf))),
        ("wct_swap_level", lambda: sl(3, p(img), 48, 64, p(sty), 40, 48, 0, nan, p(outf))),
        ("wct_swap_level", lambda: sl(5, p(img), 48, 64, p(sty), 40, 48, 0, 1.0, p(outf))),   # 3x4 and 2x3 maps at level 5: smaller than a patch
        ("wct_swap_level", lambda: sl(3, p(img), 0, 64, p(sty), 40, 48, 0, 1.0, p(outf))),
        ("wct_stylize_swap", lambda: ss(None, 48, 64, p(sty), 40, 48, 3, 0, 1.0, 1, p(outf))),
        ("wct_stylize_swap", lambda: ss(p(img), 48, 64, None, 40, 48, 3, 0, 1.0, 1, p(outf))),
        ("wct_stylize_swap", lambda: ss(p(img), 48, 64, p(sty), 40, 48, 3, 0, 1.0, 1, None)),
        ("wct_stylize_swap", lambda: ss(p(img), 48, 64, p(sty), 40, 48, 3, 0, 1.0, 0, p(outf))),
        ("wct_stylize_swap", lambda: ss(p(img), 48, 64, p(sty), 40, 48, 1, 0, 1.0, 1, p(outf))),
        ("wct_stylize_swap", lambda: ss(p(img), 48, 64, p(sty), 40, 48, 3, -1, 1.0, 1, p(outf))),
        ("wct_stylize_swap", lambda: ss(p(img), 48, 64, p(sty), 40, 48, 3, 0, inf, 1, p(outf))),
        ("wct_stylize_swap", lambda: ss(p(img), 48, 64, p(sty), 40, 48, 5, 0, 1.0, 1, p(outf))),
        ("wct_stylize_swap", lambda: ss(p(img), 8, 64, p(sty), 40, 48, 3, 0, 1.0, 1, p(outf))),
    ]
    for i, (name, call) in enumerate(refusals):
        assert call() == _lib.WCT_ERR_INVALID, (i, name)
        msg = L.wct_last_error(ctx).decode()
        assert name in msg, (i, name, msg)
    torch.cuda.synchronize()
    assert torch.equal(q, keep_q) and torch.equal(k, keep_k)
    assert bool((outf == -3.0).all()) and bool((idx == -7).all()) and bool((best == -3.0).all()) and (ho.value, wo.value) == (-1, -1)
    # the Python surface refuses the same way
    with pytest.raises(ValueError, match="match"):
        wct.swap_level(3, img[None], sty[None], "cosine")
    with pytest.raises(ValueError, match="match"):
        wct.stylize_swap(img[None], sty[None], 3, "cosine")
    with pytest.raises(ValueError):
        wct.stylize_swap(img[None], sty[None], 1)
    with pytest.raises(ValueError):
        wct.patch_match(q[None], torch.rand((5, 9, 12), device="cuda")[None])
    with pytest.raises(ValueError):
        wct.patch_assemble(idx[:3], 6, 7, k[None])
    with pytest.raises(ValueError):
        wct.patch_assemble(idx, 6, 7, k[None], None, 0.5)
    assert wct.saturation_count() == 0


def test_a_value_beyond_the_f16_range_raises_the_range_flag(torch):
    eng = sc.make_engine("16x")
    eng.strict_range = False
    Q, K = normal(1, 6, 7, 8), normal(2, 5, 9, 8)
    eng.patch_match(cu(torch, Q)[None], cu(torch, K)[None])
    torch.cuda.synchronize()
    assert eng.saturation_count() == 0
    K[2, 3, 1] = 7e4
    eng.patch_match(cu(torch, Q)[None], cu(torch, K)[None])
    torch.cuda.synchronize()
    assert eng.saturation_count(reset=True) > 0


def test_cli_swap_level(torch, tmp_path):
    """One content x one style: --swap_level 4 writes a file with _swap=4 in its name whose pixels are those of stylize_swap + to_u8
    saved through the same Pillow call; --pipeline is ignored."""
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
                     "--swap_level", "4", "--pipeline", "3"]) == 0
    files = sorted(f for f in os.listdir(o) if f.endswith(".jpg"))
    assert files == ["C_mode=16x_alpha=0.8_swap=4_c1+s1.jpg"]
    w = WCT(types.SimpleNamespace(mode="16x", alpha=0.8))
    cf = w.to_tensor_u8(torch.from_numpy(cli.load_rgb_u8(str(c / "c1.png"))).cuda())
    sf = w.to_tensor_u8(torch.from_numpy(cli.load_rgb_u8(str(s / "s1.png"))).cuda())
    want = w.to_u8(w.stylize_swap(cf, sf, 4, "whitened", alpha=0.8), 0).cpu().numpy()
    Image.fromarray(want).save(tmp_path / "ref.jpg")
    assert (o / files[0]).read_bytes() == (tmp_path / "ref.jpg").read_bytes()
    assert np.array_equal(np.array(Image.open(o / files[0])), np.array(Image.open(tmp_path / "ref.jpg")))
    log = open(o / "log_C_16x.txt").read()
    assert "--pipeline is ignored with --swap_level" in log
