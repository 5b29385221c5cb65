"""The column-sharded cascade off the shipped models: its geometry as data, the cases of tests/test_shard_widths_gpu.py and their fp64
references.  CPU only: no torch, no GPU (tests/test_shard_cases_cpu.py checks this file against wct_shard_geometry and wct_hip/sharded.py).

    geometry(W, world, rank, halo_mode)      what wct_shard_geometry / ShardedStylizer must answer, or None where they must refuse
    content_windows(W, world, halo_mode)     per level, per rank: the strip [lo, hi) that the level is fed, its owned feature window
                                             (f0, f1) as the library passes it, the window's place on the whole feature map
    style_windows(Ws, world)                 the same for the style strips of style_mode "strips"
    CASES                                    the fp64-compared jobs (models A and B of tests/width_models.py)
    Reference(model, mode)                   the fp64 and fp32 arms of the five levels of a case, level-isolated

The geometry is restated here from the description in wct_hip/sharded.py's docstring, not imported from it: the CPU test holds the two
(and the library's third copy) against each other."""
from __future__ import annotations

import types
from typing import Dict, List, Optional, Tuple

import numpy as np

from tests import transform_oracle as O
from tests import width_models as wm

LEVELS = (5, 4, 3, 2, 1)
#: encode -> decode receptive field per side (image columns of the level), its cumulative form, the encoder's alone
LEVEL_HALO = {5: 160, 4: 72, 3: 24, 2: 10, 1: 2}
CUM_HALO = {5: 272, 4: 112, 3: 40, 2: 16, 1: 6}
STYLE_HALO = {5: 80, 4: 32, 3: 12, 2: 4, 1: 1}
AUTO_EXCHANGE_BELOW = 2560
HALO_MODES = ("auto", "recompute", "exchange")


# --------------------------------------------------------------------------------------------------------- geometry
def strip_bounds(W: int, world: int) -> Optional[List[Tuple[int, int]]]:
    """Owned columns per rank (origins are multiples of 16, the last strip takes the rest); None: W cannot be cut into `world` strips."""
    xs = [min(W, (r * W // world) // 16 * 16) for r in range(world)] + [W]
    if world > 1 and any(xs[r + 1] - xs[r] < 16 for r in range(world)):
        return None
    return [(xs[r], xs[r + 1]) for r in range(world)]


def resolve_halo_mode(halo_mode: str, world: int, bounds) -> Optional[str]:
    narrowest = min(b[1] - b[0] for b in bounds)
    room = narrowest >= 2 * LEVEL_HALO[4]        # a neighbour must own the (at most 72) columns it is asked for
    if halo_mode == "auto":
        return "exchange" if world > 1 and narrowest < AUTO_EXCHANGE_BELOW and room else "recompute"
    if halo_mode == "exchange" and world > 1 and not room:
        return None
    return halo_mode


def geometry(W: int, world: int, rank: int, halo_mode: str):
    """(own0, own1, in0, in1, resolved halo mode) or None where the job must be refused."""
    bounds = strip_bounds(W, world)
    if bounds is None:
        return None
    mode = resolve_halo_mode(halo_mode, world, bounds)
    if mode is None:
        return None
    h5 = (LEVEL_HALO if mode == "exchange" else CUM_HALO)[5]
    own = bounds[rank]
    return own[0], own[1], max(0, own[0] - h5), min(W, own[1] + h5), mode


def content_windows(W: int, world: int, halo_mode: str) -> Optional[Dict[int, List[types.SimpleNamespace]]]:
    """The cascade's walk over the levels (the running width is floor-shrunk by every level, the last strip with it).  Per level a list
    over the ranks of: own (at the level's input), lo, hi (the strip fed to the level), f0, f1 (owned feature columns of the strip, f1 = -1:
    to the end), g0, n (first owned column on the whole feature map, how many), Wc (the width of the level's whole input), wf (feature
    columns of the whole map)."""
    bounds = strip_bounds(W, world)
    if bounds is None:
        return None
    mode = resolve_halo_mode(halo_mode, world, bounds)
    if mode is None:
        return None
    halo = LEVEL_HALO if mode == "exchange" else CUM_HALO
    out = {}
    Wc = W
    own = list(bounds)
    for L in LEVELS:
        sh = L - 1
        row = []
        for r in range(world):
            o0, o1 = own[r]
            lo, hi = max(0, o0 - halo[L]), min(Wc, o1 + halo[L])
            f0 = (o0 - lo) >> sh
            f1 = -1 if o1 >= Wc else (o1 - lo) >> sh
            end = ((hi - lo) >> sh) if f1 < 0 else f1
            row.append(types.SimpleNamespace(rank=r, own=(o0, o1), lo=lo, hi=hi, f0=f0, f1=f1, g0=(lo >> sh) + f0, n=end - f0, Wc=Wc, wf=Wc >> sh,
                                             aligned=lo % (1 << sh) == 0))
        out[L] = row
        Wc = (Wc >> sh) << sh
        own = [(o0, min(o1, Wc)) for o0, o1 in own]
    return out


def style_windows(Ws: int, world: int) -> Optional[Dict[int, List[types.SimpleNamespace]]]:
    """style_mode "strips": every level encodes the strip of the ORIGINAL style image with the encoder's margin."""
    bounds = strip_bounds(Ws, world)
    if bounds is None:
        return None
    out = {}
    for L in LEVELS:
        sh = L - 1
        row = []
        for r, (s0, s1) in enumerate(bounds):
            lo, hi = max(0, s0 - STYLE_HALO[L]), min(Ws, s1 + STYLE_HALO[L])
            f0 = (s0 - lo) >> sh
            f1 = -1 if s1 >= Ws else (s1 - lo) >> sh
            end = ((hi - lo) >> sh) if f1 < 0 else f1
            row.append(types.SimpleNamespace(rank=r, own=(s0, s1), lo=lo, hi=hi, f0=f0, f1=f1, g0=(lo >> sh) + f0, n=end - f0, Wc=Ws, wf=Ws >> sh,
                                             aligned=lo % (1 << sh) == 0))
        out[L] = row
    return out


def partition_error(row) -> Optional[str]:
    """None if the ranks' windows of one level cover 0 .. wf - 1 exactly once, in rank order; else what is wrong."""
    at = 0
    for p in row:
        if not p.aligned:
            return "rank %d: strip origin %d is not on the level's pooling grid" % (p.rank, p.lo)
        if p.n < 1:
            return "rank %d owns %d feature columns" % (p.rank, p.n)
        if p.g0 != at:
            return "rank %d starts at feature column %d, expected %d" % (p.rank, p.g0, at)
        at += p.n
    return None if at == row[0].wf else "windows end at %d of %d feature columns" % (at, row[0].wf)


def sweep_widths(seed: int = 7, count: int = 300, top: int = 40000) -> List[int]:
    """Every W from 16 to 700, and `count` seeded ones up to `top`."""
    rng = np.random.default_rng(seed)
    return list(range(16, 701)) + sorted(int(v) for v in rng.integers(701, top + 1, count))


# --------------------------------------------------------------------------------------------------------- cases
ALPHA = 0.6
TRANSFORMS = ("wct", "ot", "adain")
WORLDS = (3, 2)
#: W = 541 in three strips: 176 / 176 / 189 with an interior strip that is a proper crop on both sides at every level; floor pooling takes
#: 13 columns from the last one at level 5.  H is not a multiple of 16.  Level 5 has just over 2 C content and style pixels (231 / 204 for
#: 100 channels, 297 / 300 for 136).  img_seed: the first seed from 31 (A) / 32 (B) on whose fp64 arms meet the conditioning bounds of
#: tests/test_shard_cases_cpu.py at every level under all three transforms (cond(cov_c) swings by 1e3 from one draw to the next).
CASES = {
    "A": dict(seed=ord("A"), H=120, W=541, Hs=200, Ws=280, img_seed=43),
    "B": dict(seed=ord("B"), H=152, W=541, Hs=240, Ws=320, img_seed=39),
}
#: model C runs the bitwise and cascade checks only (its level 5 is singular by rank at any affordable size)
C_CASE = dict(seed=ord("C"), H=88, W=541, Hs=96, Ws=280, img_seed=33)
#: model D: A with the widths of levels 4 and 5 exchanged.  In A, B and C level 5 is the widest level, so a packed-buffer offset stepped by
#: level 5's size for every level merely spreads the buffers out; here level 4's (100 channels) would run into level 3's.  Cascade checks only.
MODEL_D = {1: 12, 2: 20, 3: 36, 4: 100, 5: 68, "l1": 28}
D_CASE = dict(seed=ord("D"), H=88, W=541, Hs=96, Ws=280, img_seed=34)


def widths_of(model: str) -> Dict:
    return MODEL_D if model == "D" else wm.MODELS[model]


def case_of(model: str) -> dict:
    return {"C": C_CASE, "D": D_CASE}.get(model) or CASES[model]


def case_images(model: str, passes: int = 2):
    c = case_of(model)
    rng = np.random.default_rng(c["img_seed"])
    return wm.smooth_image(rng, c["H"], c["W"], passes), wm.smooth_image(rng, c["Hs"], c["Ws"], passes)


def fast_fold_levels(widths: Dict) -> List[int]:
    """Levels whose decoder takes the fast fold (misc.hip fold_fast_capable: cin <= 128 and its 16-padding divides 256)."""
    out = []
    for L in LEVELS:
        C = wm.feature_channels(widths, L)
        ipad = (C + 15) // 16 * 16
        if C <= 128 and 256 % ipad == 0:
            out.append(L)
    return out


# --------------------------------------------------------------------------------------------------------- level references
def level_reference(widths, w, mode, level, img, sF, alpha, f64=True):
    """One level under `mode` in fp64, or in the reference's fp32 arithmetic with fp64 statistics (as wm.style_transfer for wct): the encoded
    content cF, (M, b) from tests/transform_oracle.py, the decoded image.  sF: the style's feature of the same arm."""
    cF = wm.encode(widths, w, level, img, f64)
    sm, ssq = wm.raw_moments(cF)
    mu_s, cov_s = O.mean_cov(sF.shape[1] * sF.shape[2], *wm.raw_moments(sF))
    M, b = O.solve(mode, cF.shape[1] * cF.shape[2], sm, ssq, O.stats(O.sym_pow(cov_s, 0.5), mu_s), alpha)
    return types.SimpleNamespace(cF=cF, sF=sF, M=M, b=b, out=wm.decode_affine(widths, w, level, cF, M, b, f64))


_STYLE_FEATS: Dict = {}
_REFS: Dict = {}


def style_feature(model: str, level: int, f64: bool):
    key = (model, level, f64)
    if key not in _STYLE_FEATS:
        _STYLE_FEATS[key] = wm.encode(widths_of(model), weights(model), level, case_images(model)[1], f64)
    return _STYLE_FEATS[key]


_WEIGHTS: Dict = {}


def weights(model: str):
    if model not in _WEIGHTS:
        _WEIGHTS[model] = wm.synth(widths_of(model), seed=case_of(model)["seed"])
    return _WEIGHTS[model]


class Reference:
    """The five levels of a case under one transform, level-isolated: level L's input is the fp64 arm's output of level L + 1 rounded to
    fp32 (tests/test_widths_gpu.py test_model_a_levels_and_cascade).  inputs[L], r64[L], r32[L] (level_reference results), e32[L]."""

    def __init__(self, model: str, mode: str):
        widths, w = widths_of(model), weights(model)
        img = case_images(model)[0]
        self.model, self.mode, self.inputs, self.r64, self.r32, self.e32 = model, mode, {}, {}, {}, {}
        for L in LEVELS:
            self.inputs[L] = img
            self.r64[L] = level_reference(widths, w, mode, L, img, style_feature(model, L, True), ALPHA, True)
            self.r32[L] = level_reference(widths, w, mode, L, img, style_feature(model, L, False), ALPHA, False)
            ref = self.r64[L].out
            self.e32[L] = float(np.abs(self.r32[L].out - ref).max() / np.abs(ref).max())
            img = ref.astype(np.float32)


def reference(model: str, mode: str) -> Reference:
    """Computed once per process and left unchanged."""
    if (model, mode) not in _REFS:
        _REFS[model, mode] = Reference(model, mode)
    return _REFS[model, mode]


def conditioning(ref: Reference, level: int) -> dict:
    """What the solves of a level meet, from the fp64 arm alone: pixels of both sides and, per matrix (cov_c, cov_s, the ot map's B), its live
    channels, its rank and its condition number on the live block.

    Live channels: the seeded stand-in weights leave some channels behind a ReLU exactly zero on every pixel of any image (a third of
    level 5's), which is a zero row and column of the covariance, not a matter of the image size; the solvers set such channels aside
    exactly (tests/test_transform_gpu.py check_solve counts them the same way: diagonal > 1e-13 of the largest).  "Full rank" is therefore
    rank == live: no direction is lost to too few pixels."""
    r = ref.r64[level]
    C = r.cF.shape[0]
    n_c, n_s = r.cF.shape[1] * r.cF.shape[2], r.sF.shape[1] * r.sF.shape[2]
    _, cov_c = O.mean_cov(n_c, *wm.raw_moments(r.cF))
    _, cov_s = O.mean_cov(n_s, *wm.raw_moments(r.sF))
    out = dict(C=C, n_c=n_c, n_s=n_s)
    for tag, A in (("c", cov_c), ("s", cov_s), ("B", O.ot_B(cov_c, O.sym_pow(cov_s, 0.5)))):
        d = np.diag(A)
        live = int((d > 1e-13 * d.max()).sum())
        lam = np.linalg.eigvalsh(O.sym(A))
        keep = lam[lam > O.REL * lam.max()]
        out["live_" + tag], out["rank_" + tag] = live, int(keep.size)
        out["cond_" + tag] = float(lam[-1] / max(lam[C - live], 1e-300))          # the live block's: inf-like where rank < live
    # B = S cov_c S is singular by rank wherever a channel is dead in the content and live in the style (a null direction that is not an
    # axis); the reference and the solver drop such directions exactly (tests/test_transform_gpu.py cond_live): cond(B) on the kept spectrum
    out["cond_B"] = float(keep.max() / keep.min())
    return out
