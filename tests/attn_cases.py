"""The cases tests/test_attn_cpu.py, tests/test_attn_gpu.py and tests/test_attn_edges_gpu.py share: the shapes of the wct_attn_stats test, the
models, images and fp64 references of the wct_attn_level test (computed once per process; the CPU test checks their input condition, the GPU
test runs them), and -- from "the launch plan" on -- launch_attn_stats' arithmetic restated and the edge cases derived from it."""
import collections
import functools

import numpy as np

from tests import attn_oracle as A
from tests import width_models as wm

QUERY_TILE, KEY_TILE = 64, 32          # WCT_ATTN_QUERY_TILE, WCT_ATTN_KEY_TILE: held against the header and attn.hip by name

#: (query h x w, key hs x ws, C) of the wct_attn_stats test; the last: a multiple of the query tile and of the key tile, plus one
STATS_SHAPES = [(7, 9, 5, 6, 8), (19, 23, 21, 18, 36), (33, 31, 40, 37, 128), (9, 11, 10, 13, 512), (3, 3, 1, 2, 4),
                (1, 2 * QUERY_TILE + 1, 1, 3 * KEY_TILE + 1, 24)]
TAUS = (0.0, 4.0, 32.0)
#: the three non-degenerate shapes of the input-condition statement
CONDITION_SHAPES = STATS_SHAPES[1:4]

#: wct_attn_level: content 64 x 80, style 48 x 72, tau 4, alpha 0.6 on stand-in models at the shipped 16x widths and one wide model
LEVEL_CONTENT, LEVEL_STYLE, LEVEL_TAU, LEVEL_ALPHA = (64, 80), (48, 72), 4.0, 0.6
ORIGINAL = {1: 64, 2: 128, 3: 256, 4: 512, 5: 512, "l1": 64}          # --mode original
LEVEL_MODELS = {"16x": (wm.W16X, 11), "wide": (ORIGINAL, 7)}
LEVEL_CASES = [(model, level, domain) for model in ("16x", "wide") for level in (2, 4) for domain in (A.STANDARD, A.WHITENED)]
MIN_VAR = 1e-4                         # the input condition: min over queries and live channels of the fp64 var
#: tests/test_attn_edges_gpu.py E8: level 3 of the un-pruned widths (C = 256: two full value slabs, the width --mode original ships there) and of
#: a stand-in whose relu3_1 has 132 channels (a second slab of 4 channels)
W132 = {1: 16, 2: 32, 3: 132, 4: 128, 5: 128, "l1": 24}
ALL_LEVEL_MODELS = dict(LEVEL_MODELS, w132=(W132, 13))
EDGE_LEVEL_CASES = [(model, 3, domain) for model in ("wide", "w132") for domain in (A.STANDARD, A.WHITENED)]


def stats_inputs(h, w, hs, ws, C):
    """(qhat, khat, V) fp32 of ReLU-like random maps: the fp64 projections of tests/attn_oracle.py, rounded once."""
    cF, sF = A.relu_map(1000 + C, h, w, C), A.relu_map(2000 + C, hs, ws, C)
    qhat, _ = A.project(cF, A.STANDARD)
    khat, sstd = A.project(sF, A.STANDARD)
    f = lambda a: np.ascontiguousarray(a.reshape(-1, C), np.float32)
    return f(qhat), f(khat), f(sstd)


@functools.lru_cache(maxsize=None)
def model_weights(model):
    from wct_hip import model_zoo
    widths, seed = ALL_LEVEL_MODELS[model]
    return model_zoo.synth_weights("original", seed) if model == "wide" else wm.synth(widths, seed=seed)


@functools.lru_cache(maxsize=None)
def level_images():
    rng = np.random.default_rng(404)
    return wm.smooth_image(rng, *LEVEL_CONTENT), wm.smooth_image(rng, *LEVEL_STYLE)


@functools.lru_cache(maxsize=None)
def level_features(model, level, f64=True):
    """(cF, sF) [h, w, C] of the model's encoder in fp64 or in the reference's fp32."""
    widths, w = ALL_LEVEL_MODELS[model][0], model_weights(model)
    c, s = level_images()
    return tuple(np.ascontiguousarray(wm.encode(widths, w, level, img, f64).transpose(1, 2, 0)) for img in (c, s))


@functools.lru_cache(maxsize=None)
def level_reference(model, level, domain, f64=True):
    """(image [3, H, W], csF, var) of the whole level in fp64, or in fp32 throughout (the e32 arm)."""
    widths, w = ALL_LEVEL_MODELS[model][0], model_weights(model)
    cF, sF = level_features(model, level, f64)
    csF, _, var = A.level_feature(cF, sF, domain, LEVEL_TAU, LEVEL_ALPHA, np.float64 if f64 else np.float32)
    img = wm.decode(widths, w, level, np.ascontiguousarray(csF.transpose(2, 0, 1)), f64)
    return img, csF, var


# ---------------------------------------------------------------------------------------------------------------- the launch plan
# launch_attn_stats (csrc/attn.hip) restated.  tests/test_attn_cpu.py holds the constants against the source by name; the GPU tests hold the
# form the launcher reports under wct_debug_set("prof_forms", 1) against `form` here.
VALUE_SLAB = 128                       # AT_CS: value channels of one workgroup (blockIdx.y); also the channels of one score chunk
QUERY_CHUNK = 32768                    # WCT_ATTN_QUERY_CHUNK
PROFILE_NAME = "attn_stats<f16x3>"
WIDTHS = tuple(range(4, 513, 4))       # what attn_c_check accepts

Plan = collections.namedtuple("Plan", "launches slabs query_tiles key_tiles nct_last nks_last half_live form")


def _cdiv(a, b):
    return (a + b - 1) // b


def plan(Nq, Nk, C, chunk=QUERY_CHUNK):
    """launches; value slabs; query tiles of each launch; key tiles; nct (16-channel value tiles) of the last slab; nks (32-channel score
    steps) of the last 128-channel chunk; whether the last 8-channel group has only its first half live (C % 8 == 4: the `c + 4 < C` half
    of load_q and of the key staging fails there); the text the launcher reports."""
    assert Nq >= 1 and Nk >= 1 and C in WIDTHS and chunk >= 1
    launches = _cdiv(Nq, chunk)
    slabs = _cdiv(C, VALUE_SLAB)
    tiles = tuple(_cdiv(min(b + chunk, Nq) - b, QUERY_TILE) for b in range(0, Nq, chunk))
    left = C - VALUE_SLAB * (slabs - 1)                    # channels of the last slab == channels of the last score chunk
    nks = 4 if left >= 128 else _cdiv(left, 32)
    return Plan(launches, slabs, tiles, _cdiv(Nk, KEY_TILE), _cdiv(left, 16), nks, C % 8 == 4, "l%d.s%d" % (launches, slabs))


def profile_name(Nq, Nk, C, chunk=QUERY_CHUNK):
    return "%s:%s" % (PROFILE_NAME, plan(Nq, Nk, C, chunk).form)


def tail_class(C):
    """What the channel guards of attn_stats_kernel can tell apart at the end of a width."""
    p = plan(2, 2, C)
    return p.nct_last, p.nks_last, p.half_live


# ---------------------------------------------------------------------------------------------------------------- the edge cases
#: E1 / E2: Nq = 65 (one full query tile and one live lane), Nk = 33 (one full key tile and one key): the smallest shape with a full and a
#: ragged tile on each axis
EDGE_SHAPE = (5, 13, 3, 11)
assert EDGE_SHAPE[0] * EDGE_SHAPE[1] == QUERY_TILE + 1 and EDGE_SHAPE[2] * EDGE_SHAPE[3] == KEY_TILE + 1

#: E2: the widths the issue names, and eleven more so that every tail_class of the 128 widths occurs, and occurs in a slab other than the
#: first (tests/test_attn_cpu.py asserts both)
PLANT_WIDTHS = (4, 8, 12, 20, 28, 36, 100, 124, 132, 136, 156, 252, 256, 260, 264, 380, 388, 508, 512,
                160, 304, 180, 448, 324, 208, 468, 224, 496, 292, 484)
PLANT_TAU = 32.0
PLANT_DAMP = 0.05


def plants(C):
    """{name: first channel of the planted group of 4}: the last 4 channels; channels 4..7 of the last complete 8-channel group; the first
    4 channels of the last 128-channel chunk -- each where it exists and is not one of the others."""
    out = {"last4": C - 4}
    if C >= 8:
        out["hi_half"] = (C // 8 - 1) * 8 + 4
    if C > 128:
        out["chunk_first"] = (_cdiv(C, 128) - 1) * 128
    seen, keep = set(), {}
    for name, c0 in out.items():
        if c0 not in seen:
            keep[name] = c0
            seen.add(c0)
    return keep


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def edge_inputs(C):
    return _frozen(*stats_inputs(*EDGE_SHAPE, C))


def damp_to_group(rows, c0, damp=PLANT_DAMP):
    """Every channel outside c0 .. c0 + 3 multiplied by `damp`, unit rows again in fp64, rounded to fp32 once."""
    a = np.array(rows, np.float64)
    keep = np.zeros(a.shape[1], bool)
    keep[c0:c0 + 4] = True
    a[:, ~keep] *= damp
    a /= np.sqrt((a * a).sum(1, keepdims=True))
    return np.ascontiguousarray(a, np.float32)


@functools.lru_cache(maxsize=None)
def planted_inputs(C, c0):
    """(q^, k^, V) of E2: the scores are decided by channels c0 .. c0 + 3."""
    q, k, v = edge_inputs(C)
    return _frozen(damp_to_group(q, c0), damp_to_group(k, c0), v)


def reference(q, k, v, tau):
    """((mean64, var64), (e32 of the mean, e32 of the var), max |V|): the fp64 arm and the fp32 arm's error by the gate's measure."""
    m64, v64 = A.stats(q, k, v, tau)
    m32, v32 = A.stats(q, k, v, tau, np.float32)
    vmax = float(np.abs(v).max())
    return _frozen(m64, v64), (float(np.abs(m32 - m64).max()) / vmax, float(np.abs(v32 - v64).max()) / vmax ** 2), vmax


#: E3: widths with 2, 3, 4 and 4 slabs (the last of 4, 4, 4 and 128 channels) and the column rotations of V
ROLL_WIDTHS, ROLLS, ROLL_TAU = (132, 260, 388, 512), (4, 16, 128), 8.0

#: E4: tile borders on both axes, rows of one draw
BORDER_NK, BORDER_NQ, BORDER_WIDTHS, BORDER_TAUS = (2, 31, 32, 33, 63, 64, 65), (2, 63, 64, 65), (36, 132), (0.0, 32.0)


@functools.lru_cache(maxsize=None)
def border_draw(C):
    """(q^ [65, C], k^ [65, C], V [65, C], the raw style rows [65, C]) of which E4 takes the first Nq / Nk rows."""
    q, k, v = stats_inputs(5, 13, 5, 13, C)
    raw = A.relu_map(2000 + C, 5, 13, C).reshape(-1, C)
    return _frozen(q, k, v, raw)


def border_inputs(C, Nq, Nk):
    q, k, v, _ = border_draw(C)
    return q[:Nq], k[:Nk], v[:Nk]


def border_standardised(C, Nk):
    """(V = the standardised map of the first Nk raw style rows themselves, rounded once; the header's tau = 0 variance
    (Nk - 1) / Nk  v / (v + eps) of it per channel, v the unbiased variance)."""
    raw = np.asarray(border_draw(C)[3][:Nk], np.float64)
    vs = raw.var(0, ddof=1)
    return np.ascontiguousarray(A.standardise(raw), np.float32), (Nk - 1) / Nk * vs / (vs + A.ADAIN_EPS)


#: E5: the running maximum.  Nk = 129: five key tiles, the last of one key
RUN_NK, RUN_NQ, RUN_WIDTHS, RUN_TAU = 4 * KEY_TILE + 1, 70, (36, 132), 32.0
#: "up" / "down" / "own": ONE key set -- the query direction u itself and 128 keys with scores in [-0.95, -0.7] -- ascending, descending and
#: with u first and the rest shuffled.  "spread_up" / "spread_down": scores spread over [0.6, 0.92], so that a tile's step of the maximum
#: (about 2.6 in the logit) leaves the earlier tiles a share of the result and every rescale is felt in it.
RUN_ORDERS = ("up", "down", "own", "spread_up", "spread_down")
RUN_JITTER = 2e-4                      # the queries are u + RUN_JITTER x noise: below half the score spacing (1.97e-3, 2.5e-3) of either set


@functools.lru_cache(maxsize=None)
def running_inputs(C, order):
    """(q^ [70, C], k^ [129, C], V [129, C]) fp32.  k_j = s_j u + sqrt(1 - s_j^2) w_j with w_j a unit row orthogonal to u: <u, k_j> = s_j."""
    rng = np.random.default_rng(5000 + C)
    u = rng.standard_normal(C)
    u /= np.linalg.norm(u)
    w = rng.standard_normal((RUN_NK, C))
    w -= np.outer(w @ u, u)
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    if order.startswith("spread"):
        s = np.linspace(0.6, 0.92, RUN_NK)
    else:
        s = np.concatenate([np.linspace(-0.95, -0.7, RUN_NK - 1), [1.0]])
    k = s[:, None] * u + np.sqrt(1 - s * s)[:, None] * w                      # ascending score
    v = A.project(A.relu_map(6000 + C, 1, RUN_NK, C), A.STANDARD)[1].reshape(-1, C)
    if order in ("down", "spread_down"):
        k, v = k[::-1], v[::-1]
    elif order == "own":
        perm = np.concatenate([[RUN_NK - 1], np.random.default_rng(7).permutation(RUN_NK - 1)])
        k, v = k[perm], v[perm]
    q = u + RUN_JITTER * rng.standard_normal((RUN_NQ, C)) / np.sqrt(C)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return _frozen(f(q), f(k), f(v))


def tile_maxima(q, k, tau):
    """[Nq, key tiles] fp64: the largest logit of every query in every key tile."""
    s = tau * (np.asarray(q, np.float64) @ np.asarray(k, np.float64).T)
    return np.stack([s[:, t:t + KEY_TILE].max(1) for t in range(0, s.shape[1], KEY_TILE)], 1)


def online_stats(q, k, v, tau, rescale=True, count_pad=False):
    """The kernel's walk in fp64: key tiles of KEY_TILE, a running maximum, sum and accumulators multiplied by exp(old - new).  With the
    defaults it is attn_oracle.stats (tests/test_attn_cpu.py).  Two mutants, to show on the CPU that the cases would catch them:
    rescale = False never multiplies; count_pad = True gives the keys past the end of the last tile the score 0 instead of weight 0."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    nq, nk = q.shape[0], k.shape[0]
    m_run, l_run = np.full(nq, -np.inf), np.zeros(nq)
    accv, accw = np.zeros((nq, v.shape[1])), np.zeros((nq, v.shape[1]))
    for t in range(0, nk, KEY_TILE):
        kt, vt = k[t:t + KEY_TILE], v[t:t + KEY_TILE]
        s = tau * (q @ kt.T)
        if count_pad and kt.shape[0] < KEY_TILE:
            pad = KEY_TILE - kt.shape[0]
            s = np.concatenate([s, np.zeros((nq, pad))], 1)
            vt = np.concatenate([vt, np.zeros((pad, v.shape[1]))], 0)
        m_new = np.maximum(m_run, s.max(1))
        f = np.exp(m_run - m_new) if rescale else np.ones(nq)
        p = np.exp(s - m_new[:, None])
        l_run = l_run * f + p.sum(1)
        accv = accv * f[:, None] + p @ vt
        accw = accw * f[:, None] + p @ (vt * vt)
        m_run = m_new
    m = accv / l_run[:, None]
    return m, np.maximum(accw / l_run[:, None] - m * m, 0)


#: E6: the default launch split, no debug key: two launches of 512 and 2 query tiles
SPLIT_NQ, SPLIT_WIDTHS, SPLIT_TAU = QUERY_CHUNK + QUERY_TILE + 1, (4, 132), 8.0


@functools.lru_cache(maxsize=None)
def split_inputs(C):
    return _frozen(*stats_inputs(1, SPLIT_NQ, EDGE_SHAPE[2], EDGE_SHAPE[3], C))


#: E7: the whitened projection either side of attn_whiten_kernel's one / two output channels per thread (C <= 256 / C > 256), on maps of
#: 2 C + 3 positions (ragged against AW_PIX = 8; the covariance has full rank)
WHITEN_WIDTHS = (4, 12, 36, 68, 132, 252, 256, 260, 508, 512)
WHITEN_PIX = 8                         # AW_PIX


def project_map(C):
    """E7, standard domain: 1 x 17 positions -- one full 16-row group of attn_unit_kernel and one row."""
    return A.relu_map(7000 + C, 1, 17, C)


def whiten_map(C):
    return A.relu_map(8000 + C, 1, 2 * C + 3, C)


def apply_inputs(C, n=QUERY_TILE + 1):
    """(mean, var, c_std, cF, mu_s, sigma_s) of E7's wct_attn_apply: the construction of tests/test_attn_gpu.py's apply test."""
    rng = np.random.default_rng(9000 + C)
    m, z = (rng.standard_normal((n, C)).astype(np.float32) for _ in range(2))
    x = np.maximum(rng.standard_normal((n, C)), 0).astype(np.float32)
    v = (rng.random((n, C)) ** 4).astype(np.float32)
    v[::7, 1] = 0.0
    return m, v, z, x, rng.standard_normal(C) * 3, rng.random(C) * 2 + 1e-3
