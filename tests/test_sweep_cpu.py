"""tests/sweep_cases.py without a GPU: the invariants the feature-space kernels rely on at every width and pixel count, that the
sweep's cases reach every form the plans can produce, and that the numpy references are sensitive to the faults the cases are for."""
import numpy as np
import pytest

from tests import sweep_cases as S

NPIX = np.arange(1, 3001, dtype=np.int64)


def _big_cases(C):
    return sorted({S.npix_of(c) for c in S.moments_cases(C) + S.kw_cases(C)} | {4096, 65536, 66049})


def _covers(npix, chunk, npc):
    return np.all((npc - 1) * chunk < npix) and np.all(npix <= npc * chunk)


def test_bands_deal_every_width_once():
    flat = [C for band in S.BANDS for C in band]
    assert sorted(flat) == list(S.WIDTHS) and len(S.BANDS) == 16 and all(len(b) == 8 for b in S.BANDS)
    for band in S.BANDS:
        assert min(band) <= 64 and max(band) >= 452                          # small and large mixed
        d = np.sign(np.diff(band))
        assert (d > 0).any() and (d < 0).any() and band[0] > band[1]          # not monotonic: a grown buffer meets a smaller width


@pytest.mark.parametrize("C", S.WIDTHS)
def test_plan_invariants(C):
    g = S.geometry(C)
    assert g["MP"] % 16 == 0 and 16 <= g["MP"] <= 256
    assert not g["pixsplit"] or g["MP"] % 64 == 0
    assert g["NLD"] <= S.MAXLD and g["NLD"] == -(-g["MP"] * (C // 4) // 256)
    assert g["PW"] in (3, 6) and (g["pixsplit"] or g["NPG"] * 4 * g["PW"] >= g["NP"]) and (not g["pixsplit"] or g["NP"] <= g["PW"])
    assert g["Cs"] % 32 == 16 and g["Cs"] >= g["T"] * 16
    kw = S.plan_kw(C, 1)
    assert kw["MP"] * (C // 4) <= 256 * S.MW_PRE and kw["MP"] % 16 == 0 and kw["MP"] <= 64      # one label / weight per thread of a wave
    assert kw["NPG"] * 4 * kw["PW"] >= kw["NP"] and kw["Cs"] % 32 == 16
    assert max(S.apply_lds(C, 8, True), S.apply_lds(C, 8, False), kw["lds"]) <= S.LDS_LIMIT
    for npix in [NPIX] + _big_cases(C):
        for f32 in (False, True):
            a = S.moments_launch(C, npix, f32)
            assert np.all(a["chunk"] % a["gran"] == 0), (C, f32)
            assert _covers(npix, a["chunk"], a["NPC"]), (C, f32)
            assert np.all(S.moments_partials_doubles(a) <= S.moments_workspace_doubles(C, npix)), (C, f32)
            assert a["lds"] <= S.LDS_LIMIT
            if a["family"] == "l":
                assert np.all(a["chunk"] % a["MP"] == 0)
        if C >= 256 and C % 128 == 0:                                                            # moments_blk_kernel, whichever form asks for it
            chunk, npc = S.blk_plan(C, npix)
            assert np.all(chunk % 64 == 0) and _covers(npix, chunk, npc)
            assert np.all(npc * (g["NP"] * 256 + g["T"] * 16) <= S.moments_workspace_doubles(C, npix))
        k = S.plan_kw(C, npix)
        assert np.all(k["chunk"] % k["MP"] == 0) and _covers(npix, k["chunk"], k["NPC"])


@pytest.mark.parametrize("C", S.WIDTHS)
def test_cases_sit_on_the_plan_boundaries(C):
    for cases, tile, npc_t, planf in ((S.moments_cases(C), S.geometry(C)["MP"], S.npc_target(C), lambda n: S.plan(C, n)),
                                      (S.kw_cases(C), S.apply_pt(C), S.plan_kw(C, 1)["npc_target"], lambda n: S.plan_kw(C, n))):
        by = {c.name: c for c in cases}
        assert [S.npix_of(by[k]) for k in ("one", "row-1", "row", "row+1", "two", "two+1")] == [1, tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1]
        n3 = S.npix_of(by["win3"])
        assert by["win3"].h == 3 and n3 % 3 == 0 and 2 * tile < n3 <= 2 * tile + 3
        assert S.npix_of(by["col"]) in (7, 63) and by["col"].h == 7 and by["col"].wfull == 9
        nb = S.npix_of(by["three+1"])
        assert planf(nb)["chunk"] == 3 * tile and planf(nb - 2)["chunk"] == 2 * tile          # nb - 1: the smallest count with three tiles
        assert nb % planf(nb)["chunk"] not in (0,) and nb <= 262146
        for c in cases:
            assert 0 <= c.x0 < c.x1 <= c.wfull and c.h >= 1
    w = {c.name: c for c in S.moments_cases(C)}
    assert w["win3"].x0 == 2 and w["win3"].wfull == (w["win3"].x1 - w["win3"].x0) + 5 and w["col"].x0 == 8 and w["col"].x1 == 9
    assert (S.npix_of(w["three+1"]) >= 262146) == (C <= 32)


def test_cases_reach_every_form():
    triples, mps, kws = set(), set(), set()
    for band in S.BANDS:
        for C in band:
            for c in S.moments_cases(C):
                for f32 in (False, True):
                    a = S.moments_launch(C, S.npix_of(c), f32)
                    if a["family"] == "l":
                        triples.add((a["NLD"], a["PW"], a["pixsplit"], f32))
                        mps.add(a["MP"])
                    else:
                        assert a["family"] == "r" and f32 and C in (32, 64)
            kws.add(S.kw_suffix(C, False))
    geo = {(g["NLD"], g["PW"], g["pixsplit"]) for g in map(S.geometry, S.WIDTHS)}
    assert len(geo) == 16 and (6, 6, True) in geo and {(2, 3, True), (4, 3, True), (7, 3, True)} <= geo
    assert {t[:3] for t in triples if not t[3]} == geo                                 # every instantiation in the fp64 form
    assert {t[:3] for t in triples if t[3]} == geo - {(8, 3, True)} | {(8, 3, False)}   # fp32 form: C = 32 runs moments_reg_kernel instead
    assert mps == {16, 32, 48, 64, 80, 128, 144, 256}
    assert {s[:-1].split(".")[2] for s in kws} == {"2", "8"} and {s.split(".")[0] for s in kws} == {"l64", "l32", "l16"}
    # folds: section e (thin C -> 3 and square C -> C -> 3 decoders, foldgemm 1 and 0) and section g (the fast fold)
    folds = set()
    for C in S.WIDTHS:
        folds |= {S.fold_form(C, 3), S.fold_form(C, C, True), S.fold_form(C, C, False)}
    folds |= {S.fold_form(C, 3 if C <= 64 else 64, fast=True) for C in (8, 12, 16, 52, 60, 116, 120, 124)}
    assert folds == set(S.FOLD_FORMS)
    assert all(S.fold_fast_capable(C) for C in (8, 12, 16, 52, 60, 116, 120, 124))
    assert [C for C in S.WIDTHS if S.fold_form(C, C, True) == "fg"] == [256, 384, 512]
    # solves: section f (every width; 100..128 again under a wide model)
    fes = {S.eig_front_end(C) for C in S.WIDTHS} | {S.eig_front_end(C, True) for C in range(100, 129, 4)}
    assert fes == set(S.EIG_FRONT_ENDS)
    assert {S.eig_front_end(C, True) for C in range(100, 129, 4)} == {"deflated4"} and S.eig_front_end(96, True) == "multi96"
    assert {C: S.ns_pad(C) for C in (4, 32, 36, 64, 68, 96, 100, 128, 132, 192, 196, 512)} == \
        {4: 32, 32: 32, 36: 64, 64: 64, 68: 96, 96: 96, 100: 128, 128: 128, 132: 192, 192: 192, 196: 256, 512: 512}


# ---------------------------------------------------------------------------------------------------- sensitivity of the references
def _moved(ref, mut, f32):
    """by how many gates the mutation moves the reference: the fp64 form's relative gate, or the fp32 form's entrywise bound"""
    (rs, rss, asum, asq), (ms, mss) = ref, mut
    if not f32:
        return max(np.abs(ms - rs).max() / np.abs(rs).max(), np.abs(mss - rss).max() / np.abs(rss).max()) / S.GATE64
    bs, bq = S.bound_f32(asum, asq, rss)
    return max((np.abs(ms - rs)[bs > 0] / bs[bs > 0]).max(), (np.abs(mss - rss)[bq > 0] / bq[bq > 0]).max())


def _mutations(f, case, tile):
    """name -> pixels [n][C] of the mutated window"""
    X = S.window_pixels(f, case)
    n, C = X.shape
    out = {"drop the last pixel": X[:-1] if n > 1 else None,
           "duplicate the first pixel of the second tile": np.vstack([X, X[tile:tile + 1]]) if n > tile else None,
           "drop channel C - 1": X * (np.arange(C) < C - 1)}
    if case.x0 > 0:
        out["shift the window by one column"] = S.window_pixels(f, case._replace(x0=case.x0 - 1, x1=case.x1 - 1))
    return {k: v for k, v in out.items() if v is not None}


@pytest.mark.parametrize("C", (4, 48, 64, 100, 512))
def test_references_see_the_faults_the_cases_are_for(C):
    tile = S.geometry(C)["MP"]
    seen = set()
    for case in S.moments_cases(C):
        f = S.feature(C, case, tile, seed=C)
        ref = S.raw_moments(S.window_pixels(f, case))
        for name, Xm in _mutations(f, case, tile).items():
            mut = S.raw_moments(Xm)[:2]
            for f32 in (False, True):
                moved = _moved(ref, mut, f32)
                assert moved > 10, "C=%d %s: '%s' moves the %s reference by %.2f gates only" % (C, case.name, name, "fp32-form" if f32 else "fp64", moved)
            seen.add(name)
    assert len(seen) == 4
    # labeled / weighted: the same pixels through a label / weight vector (the last pixel and the sentinel carry weight)
    tile = S.apply_pt(C)
    for case in S.kw_cases(C):
        if S.npix_of(case) > 70000 and C > 4:
            continue                                                     # the big case class is covered at C = 4 (and above for wct_moments)
        f = S.feature(C, case, tile, seed=C + 1)
        X = S.window_pixels(f, case)
        n = X.shape[0]
        w = np.random.default_rng(C).random(n)
        w[n - 1] = 1
        ref = S.raw_moments(X, w)
        muts = {"drop the last pixel": (X[:-1], w[:-1]) if n > 1 else None,
                "duplicate the first pixel of the second tile": (np.vstack([X, X[tile:tile + 1]]), np.append(w, w[tile])) if n > tile else None,
                "drop channel C - 1": (X * (np.arange(C) < C - 1), w)}
        for name, m in muts.items():
            if m is None:
                continue
            for f32 in (False, True):
                moved = _moved(ref, S.raw_moments(*m)[:2], f32)
                assert moved > 10, "C=%d %s weighted: '%s' moves the %s reference by %.2f gates only" % (C, case.name, name, "fp32-form" if f32 else "fp64", moved)


def test_apply_references_see_a_missing_pixel_or_channel():
    """the apply kernels' gate is 1e-6 of the largest output: a pixel left unwritten, or channel C - 1 left out of the product, moves
    the fp64 reference M x + b far beyond it"""
    for C in (4, 132, 512):
        rng = np.random.default_rng(C)
        M, b = rng.standard_normal((C, C)) / np.sqrt(C), rng.standard_normal(C)
        X = rng.standard_normal((S.apply_pt(C) + 1, C))
        ref = X @ M.T + b
        lost = ref.copy()
        lost[-1] = X[-1]
        short = (X * (np.arange(C) < C - 1)) @ M.T + b
        for mut in (lost, short):
            assert np.abs(mut - ref).max() / np.abs(ref).max() > 10 * 1e-6
