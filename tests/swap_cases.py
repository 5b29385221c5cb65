"""The patch-swap match at its launcher's edges: the launch arithmetic restated, and the inputs derived from it.
CPU only: no torch, no GPU (tests/test_swap_cases_cpu.py checks it, tests/test_swap_edges_gpu.py runs it).

`launch_patch_match` (csrc/swap.hip) cuts the queries into tiles of 8 x 16 patches, the keys into chunks of consecutive indices (one
launch each), the band of key rows a chunk touches into tiles of 8 x 16 patches, and deals those key tiles to `split` workgroups per
query tile.  This module restates that arithmetic:

    band(c0, c1, kw, ktiles_x, qtiles)    (ky0, nkt, split) of the launch for keys [c0, c1); ints or numpy int64 arrays
    plan(h, w, hs, ws, chunk)             Plan(qtiles_x, qtiles_y, ktiles_x, launches); a launch is (k0, k1, ky0, nkt, split, depth)
    form(plan)                            what the library reports behind "patch_match<f16x3>:" under wct_debug_set("prof_forms", 1)
                                          (include/wct_hip.h): the GPU test holds every report against it, so a restatement that
                                          drifts from the C++ fails there

and builds the inputs whose answer only a correct walk / tail / tap order / sign handling finds:

    strips(K, n)               n three-row strips of K side by side: planted winners in every key tile, hundreds of query tiles
    decisive_group(C, g)       only channel group g tells the planted key from exact copies at lower indices
    decisive_tap(C)            only one pixel of every patch does, at each of the nine taps in turn
    negative(C, c_off, ...)    every score of every query is negative

`reference(name)` computes the fp64 oracle of a named case once and shares it, read-only, between the tests that need it."""
from __future__ import annotations

import collections

import numpy as np

from tests import swap_oracle as O

# --------------------------------------------------------------------------------------------------------- the launcher
TY, TX = 8, 16                 # SW_TY, SW_TX: patches per tile, queries and keys alike
KEY_CHUNK = 8192               # WCT_SWAP_KEY_CHUNK
WG_TARGET = 1024               # workgroups a launch aims at
GRID_Y_MAX = 65535

Plan = collections.namedtuple("Plan", "qtiles_x qtiles_y ktiles_x launches")
Launch = collections.namedtuple("Launch", "k0 k1 ky0 nkt split depth")


def _cdiv(a, b):
    return (a + b - 1) // b


def band(c0, c1, kw, ktiles_x, qtiles):
    """Keys [c0, c1): the first key row of the band, the key tiles of the band, the workgroups per query tile they are dealt to."""
    ky0, ky1 = c0 // kw, (c1 - 1) // kw
    nkt = _cdiv(ky1 - ky0 + 1, TY) * ktiles_x
    split = np.minimum(np.minimum(_cdiv(WG_TARGET, qtiles), nkt), GRID_Y_MAX)
    return ky0, nkt, split


def plan(h, w, hs, ws, chunk=KEY_CHUNK):
    qh, qw, kh, kw = h - 2, w - 2, hs - 2, ws - 2
    assert min(qh, qw, kh, kw) >= 1 and chunk >= 1
    nk = kh * kw
    qtiles_x, qtiles_y, ktiles_x = _cdiv(qw, TX), _cdiv(qh, TY), _cdiv(kw, TX)
    launches = []
    for c0 in range(0, nk, chunk):
        c1 = min(c0 + chunk, nk)
        ky0, nkt, split = (int(v) for v in band(c0, c1, kw, ktiles_x, qtiles_x * qtiles_y))
        launches.append(Launch(c0, c1, ky0, nkt, split, _cdiv(nkt, split)))
    return Plan(qtiles_x, qtiles_y, ktiles_x, tuple(launches))


def form(p: Plan) -> str:
    """":q<query tiles>.l<launches>.<nkt>/<split> of the first launch.<nkt>/<split> of the last", cut at 23 characters as the library's"""
    a, b = p.launches[0], p.launches[-1]
    return ("q%d.l%d.%d/%d.%d/%d" % (p.qtiles_x * p.qtiles_y, len(p.launches), a.nkt, a.split, b.nkt, b.split))[:23]


PROFILE_NAME = "patch_match<f16x3>"


def profile_name(h, w, hs, ws, chunk=KEY_CHUNK) -> str:
    return PROFILE_NAME + ":" + form(plan(h, w, hs, ws, chunk))


# --------------------------------------------------------------------------------------------------------- inputs
def normal(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


STRIP_KEYS = (27, 18)          # 25 x 16 keys: four key tiles, one per tile row


def strip_keys(C):
    return normal(4000 + C, STRIP_KEYS[0], STRIP_KEYS[1], C)


def strip_rows(hs, n):
    return (7 * np.arange(n)) % (hs - 2)


def strips(K, n):
    """(Q [3, n ws, C], planted [n ws - 2], -1 at the seam queries)."""
    hs, ws, _ = K.shape
    r = strip_rows(hs, n)
    Q = np.ascontiguousarray(np.concatenate([K[ri:ri + 3] for ri in r], axis=1))
    x = np.arange(n * ws - 2)
    planted = np.where(x % ws < ws - 2, r[x // ws] * (ws - 2) + x % ws, -1)
    return Q, planted


def _tiled(seed, hs, ws, C):
    """a 4 x 5 block of normals tiled to hs x ws: every patch at (y >= 4, x >= 5) has exact copies at lower indices"""
    return np.ascontiguousarray(np.tile(normal(seed, 4, 5, C), (_cdiv(hs, 4), _cdiv(ws, 5), 1))[:hs, :ws])


def _crop(K, off, h, w):
    """(Q, planted): the h x w crop of K at `off` and the key index of every query"""
    ws = K.shape[1]
    Q = np.ascontiguousarray(K[off[0]:off[0] + h, off[1]:off[1] + w])
    qy, qx = np.divmod(np.arange((h - 2) * (w - 2)), w - 2)
    return Q, (qy + off[0]) * (ws - 2) + qx + off[1]


GROUP_WIDTHS = (4, 8, 12, 20, 28, 32, 36, 44, 60, 64, 68, 100, 252, 260, 508, 512)


def groups_of(C):
    """the first and the last channel group, and the groups either side of the 32- and 64-channel chunk borders"""
    n = C // 4
    return sorted({0, n - 1} | {g for g in (7, 8, 15, 16) if g < n})


def decisive_group(C, g):
    """(Q 7 x 22, K 13 x 37, planted): K is tiled from a 4 x 5 block except in channels 4g .. 4g + 3"""
    K = _tiled(5000 + C, 13, 37, C)
    K[:, :, 4 * g:4 * g + 4] = 2 * normal(6000 + 64 * C + g, 13, 37, 4)
    Q, planted = _crop(K, (5, 9), 7, 22)
    return Q, K, planted


def decisive_tap(C=24):
    """(Q 13 x 22, K 22 x 37, planted): K is tiled from a 4 x 5 block except at the pixels of the 3 x 3 lattice, one per patch"""
    K = _tiled(7000 + C, 22, 37, C)
    lat = K[0::3, 0::3]
    K[0::3, 0::3] = 2 * normal(7105, *lat.shape)
    Q, planted = _crop(K, (6, 9), 13, 22)
    return Q, K, planted


def tap_of_the_unique_pixel(off, h, w):
    """per query of the decisive_tap crop: 3 dy + dx of its lattice pixel"""
    qy, qx = np.divmod(np.arange((h - 2) * (w - 2)), w - 2)
    return 3 * ((-(qy + off[0])) % 3) + (-(qx + off[1])) % 3


NEGATIVE = {"neg24": (24, 0, (21, 18)), "neg36": (36, 35, (12, 37))}       # C, c_off, key map
NEG_Q = (19, 23)


def negative(C, c_off, kshape):
    Q, K = normal(8000 + C, NEG_Q[0], NEG_Q[1], C), normal(8001 + C, kshape[0], kshape[1], C)
    Q[:, :, c_off] = 5
    K[:, :, c_off] = -5
    return Q, K


ZERO_BLOCK = (8, 6)            # K[8:13, 6:11] = 0 in "neg24": nine all-zero key patches, rows 8..10 x columns 6..8
NAN_PIXEL = (9, 7)             # an interior pixel of the 21 x 18 key map


def zero_block_keys(kw):
    y, x = ZERO_BLOCK
    return np.array([(y + dy) * kw + x + dx for dy in range(3) for dx in range(3)])


def covering_keys(py, px, hs, ws):
    """the keys whose 3 x 3 patch holds pixel (py, px)"""
    kh, kw = hs - 2, ws - 2
    return np.array([ky * kw + kx for ky in range(max(py - 2, 0), min(py, kh - 1) + 1) for kx in range(max(px - 2, 0), min(px, kw - 1) + 1)])


# --------------------------------------------------------------------------------------------------------- the match cases
#: name -> (h, w, hs, ws, C, chunks): every match of tests/test_swap_edges_gpu.py that is held against plan(); chunks None = the default
BORDER_CHUNKS = (1, 16, 17, 34, 35, 36, 279, 280, 281, 349, 350, 351)
WALK = {"strips304c8": (304, 8), "strips456c8": (456, 8), "strips910c8": (910, 8), "strips304c36": (304, 36)}
CHUNK_CASE = ("chunk", 34, 66, 42, 274, 8)
BORDER_RANDOM = ("border", 11, 21, 12, 37, 24)


def match_cases():
    out = collections.OrderedDict()
    for name, (n, C) in WALK.items():
        out[name] = (3, n * STRIP_KEYS[1], STRIP_KEYS[0], STRIP_KEYS[1], C, (KEY_CHUNK,))
    out[CHUNK_CASE[0]] = CHUNK_CASE[1:] + ((KEY_CHUNK,),)
    out[BORDER_RANDOM[0]] = BORDER_RANDOM[1:] + ((KEY_CHUNK,) + BORDER_CHUNKS,)
    out["tap"] = (13, 22, 22, 37, 24, (KEY_CHUNK,) + BORDER_CHUNKS)
    for C in GROUP_WIDTHS:
        out["group%d" % C] = (7, 22, 13, 37, C, (KEY_CHUNK,))
    for name, (C, _, ks) in NEGATIVE.items():
        out[name] = NEG_Q + ks + (C, (KEY_CHUNK,))
    return out


def random_pair(name):
    """the two random-map cases: (Q, K)"""
    _, h, w, hs, ws, C = {c[0]: c for c in (CHUNK_CASE, BORDER_RANDOM)}[name]
    return normal(9000 + C, h, w, C), normal(9001 + C, hs, ws, C)


# --------------------------------------------------------------------------------------------------------- references
def rematch(S, qnorm):
    """O.match's result from a score matrix (a column of -inf is a key that may not win)"""
    idx = S.argmax(1)
    n = np.arange(len(idx))
    best = S[n, idx]
    rest = S.copy()
    rest[n, idx] = -np.inf
    return O.Match(idx, best, best - rest.max(1), qnorm, S)


def subset(m, mask):
    return O.Match(m.idx[mask], m.best[mask], m.gap[mask], m.qnorm[mask], m.S[mask])


def inputs(name):
    """(Q, K, planted or None) of a named case"""
    if name in WALK:
        n, C = WALK[name]
        K = strip_keys(C)
        Q, planted = strips(K, n)
        return Q, K, planted
    if name in (CHUNK_CASE[0], BORDER_RANDOM[0]):
        return random_pair(name) + (None,)
    if name == "tap":
        return decisive_tap()
    if name in NEGATIVE:
        return negative(*NEGATIVE[name]) + (None,)
    if name in ("neg24zero", "neg24zeroq"):                      # ... and with an all-zero query patch 0
        Q, K = negative(*NEGATIVE["neg24"])
        K[ZERO_BLOCK[0]:ZERO_BLOCK[0] + 5, ZERO_BLOCK[1]:ZERO_BLOCK[1] + 5] = 0
        if name == "neg24zeroq":
            Q[0:3, 0:3] = 0
        return Q, K, None
    raise KeyError(name)


_REF = {}


def reference(name):
    """(Q, K, planted, Match): the fp64 oracle of a named case, computed once and shared (read-only).  "neg24nan" is "neg24" with the
    nine keys that cover NAN_PIXEL barred (the K returned holds the NaN)."""
    if name not in _REF:
        if name == "neg24nan":
            Q, K, _, m0 = reference("neg24")
            S = m0.S.copy()
            S[:, covering_keys(NAN_PIXEL[0], NAN_PIXEL[1], K.shape[0], K.shape[1])] = -np.inf
            K = K.copy()
            K[NAN_PIXEL[0], NAN_PIXEL[1], 3] = np.nan
            planted, m = None, rematch(S, m0.qnorm)
        else:
            Q, K, planted = inputs(name)
            m = O.match(Q, K)
        for a in (Q, K, planted) + tuple(m):
            if a is not None:
                a.setflags(write=False)
        _REF[name] = (Q, K, planted, m)
    return _REF[name]


def inside_the_gap(m, C):
    """the share of queries whose fp64 top-2 gap is inside the gate of the f16x3 arithmetic"""
    return float((m.gap < O.tau(C) * m.qnorm).mean())
