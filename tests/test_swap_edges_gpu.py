"""wct_patch_match and wct_patch_assemble at the edges of their launchers (tests/swap_cases.py), against the numpy fp64 reference
(tests/swap_oracle.py) and against planted answers that only a correct kernel finds:

  C1  a workgroup that walks 2 and 4 key tiles: the running (score, index) across tiles and the fold after the walk
  C2  the default key chunk: two launches with no debug key set
  C3  chunk borders in key maps with three tiles per row: inside a row, at a row end, inside a tile, at a tile-row end
  C4  the channel tail of the staging at 16 widths: the first, the last and the chunk-border channel groups each decide a case alone
  C5  each of the nine taps decides a ninth of a case alone
  C6  negative scores, all-zero key and query patches, NaN keys
  C7  assemble: indices outside 0 .. Nk - 1, and out == base
  C8  one level against the fp64 decorator at levels 2 and 4

Every match also reads back what the launcher chose (wct_debug_set("prof_forms", 1)) and holds it against swap_cases.plan().  The
criteria are those of tests/test_swap_gpu.py: a planted index exactly and best = |patch_Q| to 1e-5, everything else by
check_against_fp64 under O.tau(C).  Every test prints "edges <section> ..." with its worst |best - fp64 score| / (tau |patch_Q|) and
the share of queries inside the gate's gap.  The fp64 references are computed once (swap_cases.reference) and shared.

The module imports without a GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import state_cases as sc
from tests import swap_cases as S
from tests import swap_oracle as O
from tests import test_swap_gpu as T
from tests.conftest import PKG, REPO

pytestmark = pytest.mark.gpu

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "-m gpu tests need the MI355X"
    return t


def reporting_engine():
    eng = sc.make_engine("16x")
    eng.profile(True)
    eng.debug_set("prof_forms", 1)
    return eng


@pytest.fixture(scope="module")
def wct(torch):
    return reporting_engine()


def gpu_match(torch, eng, Q, K):
    """(idx, best, the profile names of the call)"""
    eng.profile_reset()
    idx, best = T.gpu_match(torch, eng, np.array(Q), np.array(K))          # copies: the shared references are read-only
    return idx, best, [e["name"] for e in eng.profile_read()]


def form_is_the_plan(names, Q, K, chunk=S.KEY_CHUNK):
    want = S.profile_name(Q.shape[0], Q.shape[1], K.shape[0], K.shape[1], chunk)
    assert names == [want], (names, want)
    return want


def held_against_fp64(m, idx, best, C, what):
    """check_against_fp64 of tests/test_swap_gpu.py; prints the figures of DESIGN.md 4.7"""
    T.check_against_fp64(m, idx, best, C, what)
    t = O.tau(C) * m.qnorm
    chosen = m.S[np.arange(len(idx)), idx]
    fin = np.isfinite(chosen)
    print("edges %s: worst |best - fp64 score| / (tau |patch_Q|) = %.3e, %.2f %% inside the gate's gap"
          % (what, (np.abs(best - chosen)[fin] / t[fin]).max(), 100.0 * (m.gap < t).mean()))


def planted_exactly(m, idx, best, planted, what):
    p = planted >= 0
    rel = np.abs(best[p] / m.qnorm[p] - 1).max()
    print("edges %s: %d planted queries, max rel |best - |patch_Q|| = %.3e" % (what, int(p.sum()), rel))
    assert np.array_equal(idx[p], planted[p]), "%s: %d planted queries got another key" % (what, int((idx[p] != planted[p]).sum()))
    assert rel <= 1e-5
    return p


# ---------------------------------------------------------------------------------------------------------------- C1. the walk
@pytest.mark.parametrize("name", list(S.WALK))
def test_c1_a_workgroup_walks_several_key_tiles(torch, wct, name):
    """Three-row strips of a 27 x 18 key map side by side: 342, 513 and 1024 query tiles against four key tiles, dealt to 3, 2 and 1
    workgroups per query tile -- walks of 2, 2 and 4 tiles, the first two with a ragged last round.  The planted winners lie in every
    key tile, so a best found early must survive the rest of the walk and one found late must displace it."""
    Q, K, planted, m = S.reference(name)
    C = Q.shape[2]
    idx, best, names = gpu_match(torch, wct, Q, K)
    what = "C1 %s %s" % (name, form_is_the_plan(names, Q, K))
    p = planted_exactly(m, idx, best, planted, what)
    held_against_fp64(S.subset(m, ~p), idx[~p], best[~p], C, what + " seams")
    held_against_fp64(m, idx, best, C, what + " all")
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- C2. the default chunk
def test_c2_the_default_key_chunk_makes_two_launches(torch, wct):
    """34x66 against 42x274 (10880 keys, 17 key tiles per row): no debug key, launches of 8192 and 2688 keys, the border inside key row
    30; 68 key tiles on 64 workgroups in the first (a ragged walk of 2), a band that starts at row 30 in the second.  With "prof_forms"
    off the name is the plain one and not a bit of the result changes."""
    name = S.CHUNK_CASE[0]
    Q, K, _, m = S.reference(name)
    idx, best, names = gpu_match(torch, wct, Q, K)
    assert form_is_the_plan(names, Q, K) == "patch_match<f16x3>:q16.l2.68/64.34/34"
    held_against_fp64(m, idx, best, Q.shape[2], "C2 34x66 vs 42x274 C=8")
    wct.debug_set("prof_forms", 0)
    try:
        idx0, best0, names0 = gpu_match(torch, wct, Q, K)
    finally:
        wct.debug_set("prof_forms", 1)
    assert names0 == [S.PROFILE_NAME]
    assert np.array_equal(idx0, idx) and np.array_equal(best0.view(np.int32), best.view(np.int32))
    plain = sc.make_engine("16x")                       # never profiled
    idx1, best1 = T.gpu_match(torch, plain, np.array(Q), np.array(K))
    assert np.array_equal(idx1, idx) and np.array_equal(best1.view(np.int32), best.view(np.int32))
    assert wct.saturation_count() == 0 and plain.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- C3. chunk borders
BORDER_CASES = (S.BORDER_RANDOM[0], "tap")


@pytest.fixture(scope="module")
def border_runs(torch, tmp_path_factory):
    """One child process (the key needs WCT_DEBUG): per case the single-launch (idx, best), asserted there to be bit for bit what every
    chunk of BORDER_CHUNKS gives, and the profile names of every run."""
    path = str(tmp_path_factory.mktemp("swap_edges") / "border.npz")
    code = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
from tests import swap_cases as S
from tests import test_swap_edges_gpu as G
eng = G.reporting_engine()
out = {}
for name in %r:
    Q, K = S.inputs(name)[:2]
    wi, wb, names = G.gpu_match(torch, eng, Q, K)
    forms = ["|".join(names)]
    for chunk in S.BORDER_CHUNKS:
        eng.debug_set("swap_key_chunk", chunk)
        gi, gb, names = G.gpu_match(torch, eng, Q, K)
        eng.debug_set("swap_key_chunk", 0)
        forms.append("|".join(names))
        assert np.array_equal(gi, wi), "%%s chunk %%d: %%d indices differ" %% (name, chunk, int((gi != wi).sum()))
        assert np.array_equal(gb.view(np.int32), wb.view(np.int32)), "%%s chunk %%d: best differs" %% (name, chunk)
    out[name + "_idx"], out[name + "_best"], out[name + "_forms"] = wi, wb, np.array(forms)
assert eng.saturation_count() == 0
np.savez(%r, **out)
print("BORDERS_OK")
""" % (REPO, PKG, BORDER_CASES, path)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, WCT_DEBUG="1"))
    assert r.returncode == 0 and "BORDERS_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    return np.load(path)


@pytest.mark.parametrize("name", BORDER_CASES)
def test_c3_chunk_borders_with_several_tiles_per_key_row(torch, border_runs, name):
    """Key maps of 35 keys per row (three key tiles): chunks of 1, 16 +- 1 (a tile border inside a row), 35 +- 1 (a row end), 280 +- 1 (the
    end of a tile row: every band but the first starts off the multiples of 8 for 279 and 281) and Nk +- 1 give the bits of the
    single launch, which meets the fp64 criterion (and, for the tap case, the planted indices)."""
    Q, K, planted, m = S.reference(name)
    idx, best, forms = border_runs[name + "_idx"], border_runs[name + "_best"], [str(f) for f in border_runs[name + "_forms"]]
    want = [S.profile_name(Q.shape[0], Q.shape[1], K.shape[0], K.shape[1], c) for c in (S.KEY_CHUNK,) + S.BORDER_CHUNKS]
    assert forms == want
    nk = m.S.shape[1]
    assert all(f != forms[0] for f, c in zip(forms[1:], S.BORDER_CHUNKS) if c < nk), "a chunk below Nk really makes several launches"
    if planted is not None:
        planted_exactly(m, idx, best, planted, "C3 " + name)
    held_against_fp64(m, idx, best, Q.shape[2], "C3 %s, single launch" % name)


# ---------------------------------------------------------------------------------------------------------------- C4. widths
@pytest.mark.parametrize("C", S.GROUP_WIDTHS)
def test_c4_the_channel_tail_decides(torch, wct, C):
    """Every key patch has exact copies at lower indices in all channels but four (tests/test_swap_cases_cpu.py: the oracle picks a copy
    for every query once those four are zeroed): a staging that drops, doubles or misplaces that group -- the first, the last, or the
    one either side of a 32- or 64-channel border -- loses the planted index to a copy by the tie rule."""
    for g in S.groups_of(C):
        Q, K, planted = S.decisive_group(C, g)
        idx, best, names = gpu_match(torch, wct, Q, K)
        form_is_the_plan(names, Q, K)
        qnorm = np.sqrt((O.patches(np.asarray(Q, np.float64)) ** 2).sum(1))
        rel = np.abs(best / qnorm - 1).max()
        print("edges C4 C=%d group %d: max rel |best - |patch_Q|| = %.3e = %.3e tau" % (C, g, rel, rel / O.tau(C)))
        assert np.array_equal(idx, planted), "C=%d group %d: %d of %d queries got another key" % (C, g, int((idx != planted).sum()), len(idx))
        assert rel <= 1e-5
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- C5. taps
def test_c5_every_tap_decides(torch, wct):
    """One pixel of every key patch is unique, at each of the nine taps for a ninth of the queries: a kernel that skips a tap, or pairs
    the query's tap (dy, dx) with the key's (dx, dy), picks copies (5 .. 10 % and 65 % of the queries by the oracle)."""
    Q, K, planted, m = S.reference("tap")
    idx, best, names = gpu_match(torch, wct, Q, K)
    form_is_the_plan(names, Q, K)
    planted_exactly(m, idx, best, planted, "C5 decisive_tap")
    held_against_fp64(m, idx, best, Q.shape[2], "C5 decisive_tap")
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- C6. signs, zeros, NaN
@pytest.mark.parametrize("name", list(S.NEGATIVE))
def test_c6_every_score_negative(torch, wct, name):
    """Channel c_off is +5 in Q and -5 in K (the first channel of the first group; the last channel of a 4-channel tail): every score is
    below -1, so every comparison runs on the negative branch of the ordered bits, against each other and against "nothing yet"."""
    Q, K, _, m = S.reference(name)
    idx, best, names = gpu_match(torch, wct, Q, K)
    form_is_the_plan(names, Q, K)
    assert (best < 0).all()
    held_against_fp64(m, idx, best, Q.shape[2], "C6 " + name)
    assert wct.saturation_count() == 0


def test_c6_all_zero_patches(torch, wct):
    """Nine all-zero key patches among negative scores: rnorm = 1e6, score +0.0, and the lowest of the nine wins every query.  An
    all-zero query patch scores 0 against every key and gets key 0 (its partly zero neighbours tie at 0 with partly zero keys at lower
    indices: every score of that case is exactly 0 or hundreds of tau below, so the oracle's index is the answer bit for bit)."""
    Q, K, _, m = S.reference("neg24zero")
    lowest = int(S.zero_block_keys(K.shape[1] - 2).min())
    idx, best, _ = gpu_match(torch, wct, Q, K)
    assert (idx == lowest).all() and (best.view(np.int32) == 0).all(), "+0.0, bit for bit"
    Q, K, _, m = S.reference("neg24zeroq")
    idx, best, _ = gpu_match(torch, wct, Q, K)
    assert idx[0] == 0 and (best.view(np.int32) == 0).all()
    assert np.array_equal(idx, m.idx) and (idx <= lowest).all()
    assert wct.saturation_count() == 0


def test_c6_a_nan_score_never_wins(torch):
    """One NaN in the key map: the nine keys that cover it have a NaN norm, hence NaN scores, and are never chosen, although some query
    would choose one of them (tests/test_swap_cases_cpu.py); every query meets the fp64 criterion against the oracle without those keys;
    the range flag is raised.  Where every key is NaN, idx is 0 and best is NaN."""
    eng = reporting_engine()
    eng.strict_range = False
    Q, K, _, m = S.reference("neg24nan")
    idx, best, names = gpu_match(torch, eng, Q, K)
    form_is_the_plan(names, Q, K)
    bad = S.covering_keys(*S.NAN_PIXEL, *K.shape[:2])
    assert not np.isin(idx, bad).any() and (best < 0).all()
    held_against_fp64(m, idx, best, Q.shape[2], "C6 one NaN key pixel")
    assert eng.saturation_count(reset=True) > 0
    K = S.normal(77, 4, 5, 24)
    K[1, 2, 5] = np.nan
    idx, best, _ = gpu_match(torch, eng, Q, K)
    assert (idx == 0).all() and np.isnan(best).all()
    assert eng.saturation_count(reset=True) > 0


# ---------------------------------------------------------------------------------------------------------------- C7. assemble
V_SHAPE = (12, 14)
OUTSIDE = {"nk": lambda nk: [nk], "wild": lambda nk: [-1, INT32_MIN, nk, nk + 7, INT32_MAX]}


def value_map(torch, C):
    """(V on the host, V on the device): the first 12 rows of a 16-row allocation, so that the row below the map exists"""
    big = S.normal(300 + C, V_SHAPE[0] + 4, V_SHAPE[1], C)
    dev = T.cu(torch, big)
    return big[:V_SHAPE[0]], dev[:V_SHAPE[0]][None]


@pytest.mark.parametrize("which", list(OUTSIDE))
@pytest.mark.parametrize("C", [4, 24, 512])
@pytest.mark.parametrize("h,w", [(3, 3), (19, 23)])
def test_c7_an_index_outside_the_keys_is_clamped(torch, wct, h, w, C, which):
    """Bit for bit the fp32 emulation of the same indices clipped to 0 .. Nk - 1 ("nk": Nk alone, one past the last key)."""
    V, Vd = value_map(torch, C)
    base = S.normal(400 + C, h, w, C)
    nq, nk = (h - 2) * (w - 2), (V_SHAPE[0] - 2) * (V_SHAPE[1] - 2)
    outside = OUTSIDE[which](nk)
    valid = np.random.default_rng(h * w + C).integers(0, nk, nq)
    vectors = []
    if nq == 1:
        vectors = [np.array([o]) for o in outside]
    else:
        v = valid.copy()
        at = [0, w - 3, nq // 2, nq - (w - 2), nq - 1, 7, 100]           # the corners of the query map, and inside
        for i, p in enumerate(at):
            v[p] = outside[i % len(outside)]
        vectors = [v]
    for v in vectors:
        assert ((v < 0) | (v >= nk)).any()
        for alpha, b in ((1.0, None), (0.6, base)):
            got = wct.patch_assemble(T.cu(torch, v, np.int32), h, w, Vd, None if b is None else T.cu(torch, b)[None], alpha)
            want = O.assemble(np.clip(v, 0, nk - 1), h, w, V, b, alpha, dtype=np.float32)
            assert np.array_equal(got[0].cpu().numpy().view(np.int32), want.view(np.int32)), (v[:8], alpha)
    assert wct.saturation_count() == 0


@pytest.mark.parametrize("alpha", [0.6, 0.0])
def test_c7_out_may_be_base(torch, wct, alpha):
    """Through the C ABI: out == base gives the bits of the out-of-place call and leaves v alone."""
    h, w, C = 19, 23, 24
    V, Vd = value_map(torch, C)
    keep = Vd.clone()
    nq, nk = (h - 2) * (w - 2), (V_SHAPE[0] - 2) * (V_SHAPE[1] - 2)
    idx = T.cu(torch, np.random.default_rng(5).integers(0, nk, nq), np.int32)
    base = T.cu(torch, S.normal(500, h, w, C))
    want = wct.patch_assemble(idx, h, w, Vd, base[None], alpha)
    assert np.array_equal(want[0].cpu().numpy().view(np.int32),
                          O.assemble(idx.cpu().numpy(), h, w, V, base.cpu().numpy(), alpha, dtype=np.float32).view(np.int32))
    buf = base.clone()
    wct._stream()
    rc = wct._lib.wct_patch_assemble(wct._ctx, idx.data_ptr(), h, w, Vd.data_ptr(), V_SHAPE[0], V_SHAPE[1], C, buf.data_ptr(),
                                     ctypes.c_float(alpha), buf.data_ptr())
    assert rc == 0, wct._lib.wct_last_error(wct._ctx).decode()
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), want[0].view(torch.int32))
    assert torch.equal(Vd, keep)
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- C8. levels 2 and 4
#: (level, match) -> the cap on the share of queries inside the gate's gap.  NOT read off the library: the fp64 decorator on the fp32
#: reference encoder's features of the same images (tests/test_swap_cases_cpu.py, nothing of the library involved) puts 0.09 % (level 2
#: whitened), 4.65 % (level 2 raw) and 0 % (level 4 whitened) of the queries inside the gap; a share of at most 2.5 % gets the cap 5 %, one
#: of at most 10 % the cap 20 %.  Level 4 raw is left out: its oracle share is 25 % (12 of 48 queries), beyond any cap that would mean
#: something.
LEVEL_CAPS = {(2, "whitened"): 0.05, (2, "raw"): 0.20, (4, "whitened"): 0.05}


@pytest.mark.parametrize("level,match", list(LEVEL_CAPS))
def test_c8_one_level_against_the_fp64_decorator_at_levels_2_and_4(torch, wct, level, match):
    """test_one_level_against_the_fp64_decorator of tests/test_swap_gpu.py with the level a parameter: content 64x80, style 72x56 --
    32x40 and 36x28 maps of 32 channels at level 2 (1140 queries: six query tiles, several key tiles), 8x10 and 9x7 maps of 128 channels
    at level 4 (fewer pixels than channels: the whitening is a pseudo-inverse).  The caps are LEVEL_CAPS, from the oracle's own share on
    the reference encoder's features: 0.09 % (level 2 whitened, cap 5 %), 4.65 % (level 2 raw, cap 20 %), 0 % (level 4 whitened, cap 5 %);
    level 4 raw, 25 %, is left out.  Measured on the MI355X: the same three shares, no index differs from fp64, |best - fp64 score| at
    most 0.049 tau |patch_Q|, blended feature within 1.4e-7."""
    c, s = sc.image(31, 64, 80), sc.image(32, 72, 56)
    alpha = 0.6
    got = wct.swap_level(level, c, s, match, alpha)
    img, idx, best, csF, cF, sF = T.compose_level(torch, wct, level, c, s, match, alpha)
    assert tuple(got.shape) == (1, 3, 64, 80) and torch.equal(got, img), "wct_swap_level is not the composition of the public calls"
    cFn, sFn = cF[0].cpu().numpy(), sF[0].cpu().numpy()
    m, want, Q, K = O.decorate(cFn, sFn, match, alpha)
    idx, best = idx.cpu().numpy().astype(np.int64), best.cpu().numpy()
    C = cFn.shape[2]
    t = O.tau(C) * m.qnorm
    clear = m.gap >= t
    chosen = m.S[np.arange(len(idx)), idx]
    print("edges C8 level %d %s: %d queries, %d keys, C=%d, %.2f %% inside the gate's gap, %d indices differ from fp64, "
          "worst (best_fp64 - chosen) / (tau |patch_Q|) = %.3e" % (level, match, len(idx), m.S.shape[1], C, 100.0 * (~clear).mean(),
                                                                    int((idx != m.idx).sum()), ((m.best - chosen) / t).max()))
    print("edges C8 level %d %s: worst |best - fp64 score| / (tau |patch_Q|) = %.3e" % (level, match, (np.abs(best - chosen) / t).max()))
    assert np.array_equal(idx[clear], m.idx[clear]), "%d clear queries differ" % int((idx[clear] != m.idx[clear]).sum())
    assert (m.best[~clear] - chosen[~clear] <= t[~clear]).all()
    assert (np.abs(best - chosen) <= t).all()
    assert (~clear).mean() <= LEVEL_CAPS[level, match]
    h, w = cFn.shape[:2]
    agree = (idx == m.idx).reshape(h - 2, w - 2)
    ok = np.ones((h, w), bool)
    for oy in range(3):
        for ox in range(3):
            ok[oy:oy + h - 2, ox:ox + w - 2] &= agree
    assert ok.any()
    g = csF[0].cpu().numpy()
    rel = np.abs(g[ok] - want[ok]).max() / np.abs(want).max()
    print("edges C8 level %d %s: blended feature rel err %.3e on %d of %d pixels" % (level, match, rel, int(ok.sum()), h * w))
    assert rel <= 1e-5
    assert wct.saturation_count() == 0
