"""Video mode off the shipped model: model E, a three-frame clip and its level-isolated fp64 reference (tests/test_clip_cases_cpu.py holds
its preconditions, tests/test_clip_widths_gpu.py runs it on the device).  CPU only: no torch, no GPU.

    MODEL_E                      the widths; weights(): wm.synth(MODEL_E, seed=ord("E"))
    images(img_seed)             (frame 1, frame 2, frame 3, style)
    Reference(mode, img_seed)    per frame 1..3 and level 5..1: the fp64 and fp32 arms of the TRACKED level, e32, frame 2 untracked
    conditioning(ref, t, L)      what the solves of a tracked level meet (shard_cases.conditioning on the tracked covariance)

Every level of a frame does: encode, raw sums, video_oracle.track against the sums the same arm kept from the previous frame at that level
(the first frame and a cut take c itself), transform_oracle.solve on the tracked sums, wm.decode_affine.  The cut is decided at level 5, by
video_oracle.decision on the fp64 arm's sums, and holds for the frame's other levels and for the fp32 arm."""
from __future__ import annotations

import types
from typing import Dict

import numpy as np

from tests import transform_oracle as O
from tests import video_oracle as V
from tests import width_models as wm

LEVELS = (5, 4, 3, 2, 1)
FRAMES = (1, 2, 3)
TRANSFORMS = ("wct", "ot", "adain")
ALPHA = 0.6
RATE = 0.25

#: level 4 (52) is wider than level 5 (44): a packed per-level offset stepped by level 5's size lands inside a neighbour (shard_cases.MODEL_D's
#: reason).  Level 1 (20) takes the fused level-1 kernels.  Levels 5 and 3 (16-paddings 48) take the map-based fold, 4, 2 and 1 (64, 32, 32)
#: the fast one.  Nothing is wider than 128 channels, so wct_stylize_clip does not refuse the model as wide.  Narrow, so that frames can be small.
MODEL_E = {1: 12, 2: 20, 3: 36, 4: 52, 5: 44, "l1": 20}
SEED_E = ord("E")
#: frames of 164 x 183 are cropped to 160 x 176 by the cascade (strides differ from the output's); level 5 then has 10 x 11 = 110 pixels for
#: 44 channels, the 150 x 200 style 9 x 12 = 108
H, W, HS, WS = 164, 183, 150, 200
HO, WO = H // 16 * 16, W // 16 * 16
#: the first seed from 51 on whose reference meets every precondition of tests/test_clip_cases_cpu.py, for all three transforms and all three
#: frames.  EARLIER_SEEDS: where each seed before it first misses one (transform, frame, level: cond(cov_c) beyond SOLVE_MAX_COND there; 53
#: also loses rank); that file replays these.
IMG_SEED = 63
FIRST_SEED = 51
EARLIER_SEEDS = {51: ("ot", 1, 2), 52: ("wct", 1, 4), 53: ("adain", 2, 3), 54: ("wct", 1, 4), 55: ("ot", 1, 2), 56: ("wct", 1, 5), 57: ("wct", 2, 2),
                 58: ("wct", 2, 2), 59: ("adain", 3, 4), 60: ("wct", 2, 3), 61: ("adain", 1, 2), 62: ("wct", 2, 5)}
_CACHE: Dict = {}


def weights():
    if "w" not in _CACHE:
        _CACHE["w"] = wm.synth(MODEL_E, seed=SEED_E)
    return _CACHE["w"]


def images(img_seed: int = IMG_SEED):
    """One default_rng(img_seed), in this order: frame 1; the image frame 2 = clip(0.8 frame1 + 0.2 other) is mixed from; the style.  Frame 3
    is another scene: smooth(default_rng(img_seed + 1), one pass).

    Frame 3 at full contrast, not 0.5 x + 0.25: D3 is taken against the sums TRACKED over frames 1 and 2 (cut_distances), and with the
    compressed frame it came out BELOW D2, twice within 0.1 % above it, for every seed from 51 to 129 (D2 4.9 .. 8.2, D3 4.3 .. 6.1; 6.19 and
    5.30 at seed 59) -- no threshold makes frame 2 tracked and that frame 3 a cut.  At full contrast D3 is 22 .. 31 for seeds 51 .. 63."""
    rng = np.random.default_rng(img_seed)
    f1 = wm.smooth_image(rng, H, W)
    other = wm.smooth_image(rng, H, W)
    f2 = np.ascontiguousarray(np.clip(np.float32(0.8) * f1 + np.float32(0.2) * other, 0.0, 1.0), np.float32)
    style = wm.smooth_image(rng, HS, WS)
    f3 = wm.smooth_image(np.random.default_rng(img_seed + 1), H, W, passes=1)
    return f1, f2, f3, style


def pixels(level: int) -> float:
    """n of a level: fixed by the clip's size (wct_clip_create: (Ho >> (L - 1)) (Wo >> (L - 1)))."""
    return float((HO >> (level - 1)) * (WO >> (level - 1)))


def cut_distances(img_seed: int = IMG_SEED):
    """(D2, D3) of video_oracle.decision from the fp64 level-5 sums of the three frames alone (level 5 sees the frames themselves, so these
    do not depend on the transform): frame 2 against frame 1's sums, frame 3 against the sums tracked over frames 1 and 2 -- what the device
    holds when frame 2 was not a cut.  The tracked second moment carries rate (1 - rate) (mu_2 - mu_1)^2 on top of the two frames' variances,
    so D3 is measured against a LARGER variance than D2: another scene is not automatically the larger distance."""
    f1, f2, f3, _ = images(img_seed)
    c = [wm.raw_moments(wm.encode(MODEL_E, weights(), 5, f, True)) for f in (f1, f2, f3)]
    r2 = tuple(V.track(c[0][k], c[1][k], RATE, False) for k in (0, 1))
    return V.decision(pixels(5), c[1][0], c[0][0], c[0][1], 1, np.inf)[1], V.decision(pixels(5), c[2][0], r2[0], r2[1], 2, np.inf)[1]


def solved_level(level, cF, sums, st, mode, f64):
    """(M, b) of `mode` from the given raw sums and the style statistics, and the decoded image."""
    M, b = O.solve(mode, cF.shape[1] * cF.shape[2], sums[0], sums[1], st, ALPHA)
    return M, b, wm.decode_affine(MODEL_E, weights(), level, cF, M, b, f64)


class Reference:
    """inputs[t][L]; r64[t][L], r32[t][L]: cF, raw (sum, sumsq), tracked (sum, sumsq), M, b, out; e32[t][L]; cut[t], D[t] (t = 2, 3), cut_thr;
    untracked[L]: frame 2's fp64 output from its raw sums on the same input.  Computed once and never written to.
    upto = (t, L): the fp64 arm alone, as far as that frame's level (enough for conditioning(); the search of IMG_SEED replays with it)."""

    def __init__(self, mode: str, img_seed: int = IMG_SEED, upto=None):
        w = weights()
        f1, f2, f3, style = images(img_seed)
        self.mode, self.img_seed = mode, img_seed
        self.frames = {1: f1, 2: f2, 3: f3}
        self.style = style
        self.st, self.sF = {}, {}
        arms_run = (True, False) if upto is None else (True,)
        self.inputs, self.r64, self.r32, self.e32 = {}, {}, {}, {}
        self.cut, self.D, self.untracked = {1: True}, {}, {}
        kept: Dict = {}                                      # (f64, L) -> the arm's tracked sums of the previous frame
        # the threshold lies between the two distances, which do not depend on it as long as frame 2 is not a cut: its tracked sums are r + rate (c - r)
        self.cut_thr = None
        for t in FRAMES:
            img = self.frames[t]
            self.inputs[t], self.r64[t], self.r32[t], self.e32[t] = {}, {}, {}, {}
            for L in LEVELS:
                self.inputs[t][L] = img
                arms = {}
                for f64 in arms_run:
                    if (f64, L) not in self.st:
                        sF = wm.encode(MODEL_E, w, L, style, f64)
                        mu_s, cov_s = O.mean_cov(sF.shape[1] * sF.shape[2], *wm.raw_moments(sF))
                        self.st[f64, L], self.sF[f64, L] = O.stats(O.sym_pow(cov_s, 0.5), mu_s), sF
                    cF = wm.encode(MODEL_E, w, L, img, f64)
                    raw = wm.raw_moments(cF)
                    if L == 5 and f64 and t > 1:
                        _, self.D[t] = V.decision(pixels(5), raw[0], kept[True, 5][0], kept[True, 5][1], t - 1, np.inf)
                        if t == 3:
                            self.cut_thr = float(np.sqrt(self.D[2] * self.D[3]))
                        self.cut[t] = t == 3                  # by construction; D[2] < cut_thr < D[3] is tests/test_clip_cases_cpu.py's to check
                    if self.cut[t]:
                        tracked = (raw[0].copy(), raw[1].copy())
                    else:
                        tracked = tuple(V.track(kept[f64, L][k], raw[k], RATE, False) for k in (0, 1))
                    M, b, out = solved_level(L, cF, tracked, self.st[f64, L], mode, f64)
                    arms[f64] = types.SimpleNamespace(cF=cF, sF=self.sF[f64, L], raw=raw, tracked=tracked, M=M, b=b, out=out)
                    kept[f64, L] = tracked
                    if f64 and t == 2 and upto is None:
                        self.untracked[L] = solved_level(L, cF, raw, self.st[True, L], mode, True)[2]
                self.r64[t][L] = arms[True]
                ref = arms[True].out
                if upto == (t, L):
                    return
                if upto is None:
                    self.r32[t][L] = arms[False]
                    self.e32[t][L] = float(np.abs(arms[False].out - ref).max() / np.abs(ref).max())
                img = ref.astype(np.float32)

    def gate(self, t: int, L: int) -> float:
        """The project's level gate (tests/test_widths_gpu.py, tests/test_shard_widths_gpu.py) on rel_err against the fp64 arm."""
        return 4 * self.e32[t][L] + 1e-4

    def decisions(self):
        """{t: (cut, D)} of frames 2 and 3 as video_oracle.decision gives them at cut_thr from the fp64 arm's sums."""
        out = {}
        for t in (2, 3):
            r = self.r64[t - 1][5].tracked
            out[t] = V.decision(pixels(5), self.r64[t][5].raw[0], r[0], r[1], t - 1, self.cut_thr)
        return out


def reference(mode: str, img_seed: int = IMG_SEED) -> Reference:
    """Computed once per process and left unchanged."""
    if (mode, img_seed) not in _CACHE:
        _CACHE[mode, img_seed] = Reference(mode, img_seed)
    return _CACHE[mode, img_seed]


def spectrum(A) -> dict:
    """shard_cases.conditioning's figures of one symmetric matrix: live channels (diagonal > 1e-13 of the largest: the stand-in weights leave
    some channels behind a ReLU exactly zero), rank (eigenvalues above transform_oracle.REL of the largest), cond of the live block and of the
    kept spectrum."""
    C = A.shape[0]
    d = np.diag(A)
    live = int((d > 1e-13 * d.max()).sum())
    lam = np.linalg.eigvalsh(O.sym(A))
    keep = lam[lam > O.REL * lam.max()]
    return dict(live=live, rank=int(keep.size), cond=float(lam[-1] / max(lam[C - live], 1e-300)), cond_kept=float(keep.max() / keep.min()))


def conditioning(ref: Reference, t: int, level: int) -> dict:
    """What the solves of frame t's level meet, from the fp64 arm alone: pixels of both sides and, for the TRACKED cov_c, cov_s and the ot map's
    B = S cov_c S, live channels, rank and condition number (B's on its kept spectrum: it is singular by rank wherever a channel is dead in
    the content and live in the style, and solver and reference drop such directions exactly)."""
    r = ref.r64[t][level]
    n_c, n_s = r.cF.shape[1] * r.cF.shape[2], r.sF.shape[1] * r.sF.shape[2]
    assert n_c == pixels(level)
    _, cov_c = O.mean_cov(n_c, *r.tracked)
    _, cov_s = O.mean_cov(n_s, *wm.raw_moments(r.sF))
    c, s, B = spectrum(cov_c), spectrum(cov_s), spectrum(O.ot_B(cov_c, O.sym_pow(cov_s, 0.5)))
    return dict(C=r.cF.shape[0], n_c=n_c, n_s=n_s, live_c=c["live"], rank_c=c["rank"], cond_c=c["cond"], live_s=s["live"], rank_s=s["rank"],
                cond_s=s["cond"], cond_B=B["cond_kept"])
