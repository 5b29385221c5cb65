"""tests/swap_cases.py without a GPU: the restated launcher is self-consistent and reaches the edges it is meant to reach, and every input
of tests/test_swap_edges_gpu.py has the property that keeps its GPU test from passing vacuously -- measured on the fp64 oracle
(tests/swap_oracle.py) alone, nothing of the library involved."""
import numpy as np
import pytest

from tests import swap_cases as S
from tests import swap_oracle as O


# ---------------------------------------------------------------------------------------------------------------- the plan
def test_plan_reproduces_the_values_worked_out_by_hand():
    want = {
        (3, 5472, 27, 18): (342, [(0, 400, 0, 4, 3, 2)]),
        (3, 8208, 27, 18): (513, [(0, 400, 0, 4, 2, 2)]),
        (3, 16380, 27, 18): (1024, [(0, 400, 0, 4, 1, 4)]),
        (34, 66, 42, 274): (16, [(0, 8192, 0, 68, 64, 2), (8192, 10880, 30, 34, 34, 1)]),
    }
    for shape, (qtiles, launches) in want.items():
        p = S.plan(*shape)
        assert p.qtiles_x * p.qtiles_y == qtiles and [tuple(l) for l in p.launches] == launches, shape
    assert S.profile_name(34, 66, 42, 274) == "patch_match<f16x3>:q16.l2.68/64.34/34"
    assert S.profile_name(3, 16380, 27, 18) == "patch_match<f16x3>:q1024.l1.4/1.4/1"


def test_every_key_belongs_to_one_launch_and_lies_inside_its_band():
    """All key maps up to 20 x 40 and all chunks 1 .. Nk + 1, for a small and a large number of query tiles: the launches' [k0, k1) cut
    0 .. Nk - 1 without gap or overlap, the first and the last key of a launch (hence all of them: the index is monotonic in the row)
    lie in the rows of the band's tiles, every key column lies in a tile, and split <= nkt."""
    for hs in range(3, 21):
        for ws in range(3, 41):
            kh, kw = hs - 2, ws - 2
            nk = kh * kw
            ktiles_x = S._cdiv(kw, S.TX)
            assert ktiles_x * S.TX >= kw
            chunk = np.repeat(np.arange(1, nk + 2), [S._cdiv(nk, c) for c in range(1, nk + 2)])
            first = np.flatnonzero(np.r_[True, chunk[1:] != chunk[:-1]])
            c0 = (np.arange(len(chunk)) - np.repeat(first, np.diff(np.r_[first, len(chunk)]))) * chunk
            c1 = np.minimum(c0 + chunk, nk)
            last = np.r_[first[1:] - 1, len(chunk) - 1]
            assert (c0[first] == 0).all() and (c1[last] == nk).all() and (c0 < c1).all()
            inner = np.ones(len(chunk), bool)
            inner[last] = False
            assert (c1[inner] == c0[1:][inner[:-1]]).all()
            for qtiles in (1, 400):
                ky0, nkt, split = S.band(c0, c1, kw, ktiles_x, qtiles)
                rows = nkt // ktiles_x * S.TY
                assert (nkt % ktiles_x == 0).all() and (split >= 1).all() and (split <= nkt).all()
                assert (ky0 <= c0 // kw).all() and ((c1 - 1) // kw < ky0 + rows).all()
                assert (rows < (c1 - 1) // kw - ky0 + 1 + S.TY).all(), "a band holds no tile row without a key"


def test_plan_is_the_loop_over_band():
    for shape in ((19, 23, 21, 18), (11, 21, 12, 37), (130, 200, 20, 40)):
        kh, kw = shape[2] - 2, shape[3] - 2
        for chunk in range(1, kh * kw + 2):
            p = S.plan(*shape, chunk=chunk)
            assert [l.k0 for l in p.launches] == list(range(0, kh * kw, chunk)) and p.launches[-1].k1 == kh * kw
            for l in p.launches:
                assert l.k1 - l.k0 <= chunk and l.split <= l.nkt and l.depth == -(-l.nkt // l.split)
                assert l.ky0 * kw <= l.k0 and l.k1 <= (l.ky0 + l.nkt // p.ktiles_x * S.TY) * kw


def _launches():
    for name, (h, w, hs, ws, C, chunks) in S.match_cases().items():
        for chunk in chunks:
            p = S.plan(h, w, hs, ws, chunk)
            for l in p.launches:
                yield name, ws - 2, p, l


def test_the_cases_reach_every_walk_depth_and_band_offset():
    L = list(_launches())
    depths = {l.depth for _, _, _, l in L}
    assert {1, 2} <= depths and max(depths) >= 4
    assert any(l.depth >= 2 and l.nkt % l.split for _, _, _, l in L), "a walk whose last round is ragged"
    assert any(l.depth >= 2 and l.nkt % l.split == 0 for _, _, _, l in L), "and one whose rounds are all full"
    assert any(l.ky0 % S.TY and p.ktiles_x > 1 for _, _, p, l in L), "a band off the multiples of 8 with several tiles per row"
    assert any(len(p.launches) == 2 and p.launches[0].k1 - p.launches[0].k0 == S.KEY_CHUNK for _, _, p, _ in L), "the default chunk, twice"


def test_the_cases_reach_every_kind_of_chunk_border():
    borders = [(kw, l.k0) for _, kw, p, l in _launches() if l.k0 and p.ktiles_x > 1]
    assert any(k0 % kw for kw, k0 in borders), "inside a key row"
    assert any(k0 % kw == 0 for kw, k0 in borders), "at a row end"
    assert any(k0 % kw % S.TX for kw, k0 in borders), "inside a tile"
    assert any(k0 % kw and k0 % kw % S.TX == 0 for kw, k0 in borders), "between two tiles of a row"
    assert any(k0 % (S.TY * kw) == 0 for kw, k0 in borders), "at a tile-row end"
    assert any(k0 % kw == 0 and k0 % (S.TY * kw) for kw, k0 in borders), "at a row end inside a tile row"


# ---------------------------------------------------------------------------------------------------------------- the inputs
RANDOM = list(S.WALK) + [S.CHUNK_CASE[0], S.BORDER_RANDOM[0]] + list(S.NEGATIVE)


@pytest.mark.parametrize("name", RANDOM)
def test_the_oracle_itself_is_decided(name):
    """At most 1 % of the queries of a random case lie inside the gate's gap by the fp64 oracle's own gaps (measured: 0 % for the strips
    at C = 8 and 0.22 % at C = 36, 0.10 % for 34x66 vs 42x274, 0 % for 11x21 vs 12x37 and for the two negative cases); the GPU tests
    cap the share at 5 %."""
    Q, K, planted, m = S.reference(name)
    share = S.inside_the_gap(m, Q.shape[2])
    print("%s: %.2f %% of %d queries inside the gate's gap" % (name, 100 * share, len(m.idx)))
    assert share <= 0.01
    assert Q.dtype == np.float32 and K.dtype == np.float32
    assert Q.shape[:2] == S.match_cases()[name][:2] and K.shape[:2] == S.match_cases()[name][2:4]


def _planted_ok(m, planted, C, what):
    p = planted >= 0
    assert p.any() and np.array_equal(m.idx[p], planted[p]), what
    r = (m.gap[p] / (O.tau(C) * m.qnorm[p])).min()
    print("%s: smallest top-2 gap of a planted query = %.0f tau |patch_Q|" % (what, r))
    assert r >= 10, what
    return p


@pytest.mark.parametrize("name", list(S.WALK))
def test_strips_plant_winners_in_every_key_tile(name):
    Q, K, planted, m = S.reference(name)
    n, C = S.WALK[name]
    p = _planted_ok(m, planted, C, name)
    assert Q.shape == (3, n * K.shape[1], C) and (~p).sum() == 2 * (n - 1), "two seam queries per seam"
    x = np.flatnonzero(p)
    ws = K.shape[1]
    assert all(np.array_equal(Q[:, xx:xx + 3], K[r:r + 3, xx % ws:xx % ws + 3]) for xx, r in list(zip(x, S.strip_rows(K.shape[0], n)[x // ws]))[::97])
    # per query tile of 16 columns: which key tile (= tile row: the key map is one tile wide) holds the winner
    tile = planted[p] // (K.shape[1] - 2) // S.TY
    assert set(tile) == {0, 1, 2, 3}
    depth = S.plan(*S.match_cases()[name][:4]).launches[0].depth
    assert depth >= 2 and (depth >= 4) == (n == 910)


@pytest.mark.parametrize("C", S.GROUP_WIDTHS)
def test_decisive_group_is_decided_by_its_group_alone(C):
    """The oracle finds the planted key with a gap of at least 10 tau |patch_Q| (measured: >= 17 tau at C = 508 / 512, more below), and
    with group g zeroed in both maps it picks another key for at least 90 % of the queries (measured 100 % everywhere)."""
    assert S.groups_of(C)[0] == 0 and S.groups_of(C)[-1] == C // 4 - 1
    for g in S.groups_of(C):
        Q, K, planted = S.decisive_group(C, g)
        m = O.match(Q, K)
        _planted_ok(m, planted, C, "decisive_group(%d, %d)" % (C, g))
        if C > 4:
            assert (O.lowest_duplicate(np.delete(K, np.s_[4 * g:4 * g + 4], 2))[planted] < planted).all(), "a copy at a lower index"
        Q0, K0 = Q.copy(), K.copy()
        Q0[:, :, 4 * g:4 * g + 4] = 0
        K0[:, :, 4 * g:4 * g + 4] = 0
        changed = (O.match(Q0, K0).idx != planted).mean()
        assert changed >= 0.9, (C, g, changed)


def test_decisive_tap_is_decided_by_every_tap():
    """Planted and found by the oracle with a gap of thousands of tau; the unique pixel sits at each of the nine taps; leaving one tap out
    of the products changes 5 .. 10 % of the indices (about the ninth of the queries whose unique pixel sits there), and reading the key
    taps transposed changes 65 %."""
    Q, K, planted, m = S.reference("tap")
    C = Q.shape[2]
    _planted_ok(m, planted, C, "decisive_tap")
    at = S.tap_of_the_unique_pixel((6, 9), 13, 22)
    assert (np.bincount(at, minlength=9) >= 18).all()
    lattice = np.zeros(K.shape[:2], bool)
    lattice[0::3, 0::3] = True
    qy, qx = np.divmod(planted, K.shape[1] - 2)
    assert all(lattice[y + t // 3, x + t % 3] and lattice[y:y + 3, x:x + 3].sum() == 1 for y, x, t in zip(qy, qx, at))
    pq, pk = O.patches(np.asarray(Q, np.float64)), O.patches(np.asarray(K, np.float64))
    rn = 1.0 / np.sqrt((pk * pk).sum(1) + O.EPS)
    for t in range(9):
        keep = np.ones(9 * C, bool)
        keep[t * C:(t + 1) * C] = False
        changed = (((pq[:, keep] @ pk[:, keep].T) * rn).argmax(1) != planted).mean()
        print("decisive_tap without tap %d: %.1f %% of the indices change" % (t, 100 * changed))
        assert changed >= 0.05, t
    pkT = pk.reshape(-1, 3, 3, C).transpose(0, 2, 1, 3).reshape(-1, 9 * C)
    changed = (((pq @ pkT.T) * rn).argmax(1) != planted).mean()
    print("decisive_tap with the key taps transposed: %.1f %%" % (100 * changed))
    assert changed >= 0.5


@pytest.mark.parametrize("name", list(S.NEGATIVE))
def test_negative_cases_have_no_score_above_zero(name):
    Q, K, _, m = S.reference(name)
    assert (m.S < 0).all() and m.best.max() < -1


def test_degenerate_key_patches():
    """The zero block makes nine all-zero key patches whose fp64 score is exactly 0 above a field of negative scores, the lowest of them
    134; the NaN pixel is covered by nine keys, none of which the barred oracle picks; the 4 x 5 map's pixel (1, 2) by all six."""
    Q, K, _, m = S.reference("neg24zero")
    zk = S.zero_block_keys(K.shape[1] - 2)
    assert len(zk) == 9 and (O.patches(K)[zk] == 0).all() and (np.abs(O.patches(K)).sum(1) == 0).sum() == 9
    assert (m.idx == zk.min()).all() and zk.min() == 134 and (m.best == 0).all()
    assert (np.delete(m.S, zk, 1) < 0).all()
    m = S.reference("neg24zeroq")[3]
    # the partly zero queries beside query 0 score exactly 0 against partly zero keys too, where the two supports do not meet: the lowest
    # index among ALL zero scores wins; every other score is negative and far below in units of the gate
    assert (m.S[0] == 0).all() and m.idx[0] == 0 and (m.best == 0).all() and (m.S <= 0).all()
    assert (np.where(m.S == 0, -np.inf, m.S).max(1) <= -100 * O.tau(24) * m.qnorm).all()
    assert (m.idx[m.idx != zk.min()] < zk.min()).all() and 1 < (m.idx != zk.min()).sum() < 9
    Q, K, _, m = S.reference("neg24nan")
    bad = S.covering_keys(*S.NAN_PIXEL, *K.shape[:2])
    assert len(bad) == 9 and np.isnan(K).sum() == 1 and np.array_equal(np.flatnonzero(np.isnan(O.patches(K)).any(1)), np.sort(bad))
    assert not np.isin(m.idx, bad).any() and S.inside_the_gap(m, 24) <= 0.01 and (m.best < 0).all()
    assert np.isin(S.reference("neg24")[3].idx, bad).any(), "some query would have chosen a barred key"
    assert len(S.covering_keys(1, 2, 4, 5)) == 6


def test_the_decorator_caps_come_from_the_oracle():
    """The caps of test_one_level_against_the_fp64_decorator_at_levels_2_and_4 (tests/test_swap_edges_gpu.py): the share of queries inside
    the gate's gap by the fp64 decorator on the fp32 REFERENCE encoder's features of the same two images -- at most 2.5 % for a cap of
    5 %, at most 10 % for a cap of 20 %, above that the pair is left out.  Measured: level 2 whitened 0.09 %, level 2 raw 4.65 %, level 4
    whitened 0 %, level 4 raw 25 % (left out)."""
    torch = pytest.importorskip("torch")
    import os
    from oracle import wct_oracle
    from tests.conftest import PKG
    from tests import test_swap_edges_gpu as G
    from wct_hip import model_zoo
    mods = wct_oracle.Modules("16x", model_zoo.load_npz_weights(os.path.join(PKG, "weights", "16x.npz")))

    def image(seed, H, W):          # tests/state_cases.py image(), on the host
        g = torch.Generator()
        g.manual_seed(seed)
        return torch.rand((1, 3, H, W), generator=g).numpy()[0]
    c, s = image(31, 64, 80), image(32, 72, 56)
    seen = {}
    for level in (2, 4):
        cF, sF = (np.ascontiguousarray(mods.encode(level, x).transpose(1, 2, 0)) for x in (c, s))
        for match in ("whitened", "raw"):
            m = O.decorate(cF, sF, match, 0.6)[0]
            seen[level, match] = S.inside_the_gap(m, cF.shape[2])
            print("level %d %s: %.2f %% of %d queries inside the gate's gap" % (level, match, 100 * seen[level, match], len(m.idx)))
    for key, share in seen.items():
        if share > 0.10:
            assert key not in G.LEVEL_CAPS, key
        else:
            assert G.LEVEL_CAPS[key] == (0.05 if share <= 0.025 else 0.20), (key, share)
