"""The cases tests/test_attn_cpu.py and tests/test_attn_gpu.py share: the shapes of the wct_attn_stats test, and the models, images and fp64
references of the wct_attn_level test (computed once per process; the CPU test checks their input condition, the GPU test runs them)."""
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
    widths, seed = LEVEL_MODELS[model]
    return wm.synth(widths, seed=seed) if model == "16x" else model_zoo.synth_weights("original", seed)


@functools.lru_cache(maxsize=None)
def level_images():
    rng = np.random.default_rng(404)
    return wm.smooth_image(rng, *LEVEL_CONTENT), wm.smooth_image(rng, *LEVEL_STYLE)


@functools.lru_cache(maxsize=None)
def level_features(model, level, f64=True):
    """(cF, sF) [h, w, C] of the model's encoder in fp64 or in the reference's fp32."""
    widths, w = LEVEL_MODELS[model][0], model_weights(model)
    c, s = level_images()
    return tuple(np.ascontiguousarray(wm.encode(widths, w, level, img, f64).transpose(1, 2, 0)) for img in (c, s))


@functools.lru_cache(maxsize=None)
def level_reference(model, level, domain, f64=True):
    """(image [3, H, W], csF, var) of the whole level in fp64, or in fp32 throughout (the e32 arm)."""
    widths, w = LEVEL_MODELS[model][0], model_weights(model)
    cF, sF = level_features(model, level, f64)
    csF, _, var = A.level_feature(cF, sF, domain, LEVEL_TAU, LEVEL_ALPHA, np.float64 if f64 else np.float32)
    img = wm.decode(widths, w, level, np.ascontiguousarray(csF.transpose(2, 0, 1)), f64)
    return img, csF, var
