"""Case tables of the ot / adain width sweep (tests/test_transform_widths_gpu.py, tests/test_transform_cpu.py) as data.  CPU only: numpy
and the fp64 reference (tests/transform_oracle.py), no torch, no GPU.

The code that makes (M, b) branches on the channel count C in two places:

    csrc/transform.hip   one wave per 16 x 16 tile, 4 values of k per MFMA step: nt = ceil(C / 16) tiles a side, a ragged last tile where
                         C % 16 != 0, a k-tail (the `k < C` mask inside a step) where C % 4 == 2
    csrc/solve.hip       launch_eig's front end by ns_pad(C): 32 / 64 one LDS workgroup, 96 the plain multi-launch iteration (split-k
                         needs Cp % 64 == 0), 128 the single-launch kernel (or split-k multi-launch with it switched off), wider the
                         deflated iteration on ns_stage*_wide<4> (Cp % 128 != 0 or Cp < 256) or <8>

WIDTHS names every width of the sweep by the front end it reaches.  Every width has a full-rank case and one with dead channels in the
ragged tail; RANK_WIDTHS add a content side that is singular by rank (n < C): at 88 the plain iteration runs out of budget and the LDS
Jacobi net takes over (info[0] >= 100), at 260 the deflated iteration converges on the singular B itself and the global-memory Jacobi
behind it is not reached."""
import collections

import numpy as np

from tests import transform_oracle as O

#: front end -> widths
FRONT_ENDS = collections.OrderedDict((
    ("lds32", (4, 6, 12, 20, 30)),                                  # ns_lds_kernel<32>; nt = 1, 2 with a ragged last tile; k-tail at 6, 30
    ("lds64", (36, 38, 62)),                                        # ns_lds_kernel<64>; nt = 3, 4 with a ragged last tile; k-tail at 38, 62
    ("plain96", (66, 68, 88, 96)),                                  # ns_prep + 32 x ns_stage1 / ns_stage2 under the ot schedule; k-tail at 66
    ("single128", (100, 126)),                                      # the single-launch kernel (nscoop) on a ragged matrix; k-tail at 126
    ("deflated", (130, 132, 196, 258, 260, 388, 508, 510)),         # wide<4>: Cp 192, 320, 448; wide<8>: Cp 256, 512; nt = 9 .. 32; k-tail at 130, 258, 510
))
WIDTHS = collections.OrderedDict((C, fe) for fe, cs in FRONT_ENDS.items() for C in cs)

#: widths with a content-rank-deficient case: n = C - 11 pixels, rank n - 1 (the LDS Jacobi net under Cp = 96; the deflated iteration at 260)
RANK_WIDTHS = (88, 260)

LO = 1e-2          # lo_c = lo_s: eigenvalues 1 .. 1e-2 on both sides, cond(B) <= 1e4


def ns_pad(C):
    """solve.hip ns_pad"""
    return (C + 63) // 64 * 64 if C > 128 else (C + 31) // 32 * 32


def tiles(C):
    return (C + 15) // 16


def k_tail(C):
    return C % 4 == 2


def dead_tail(C):
    """The first channel of the last 16-tile and channel C - 1."""
    return (16 * ((C - 1) // 16), C - 1)


def _spec(C, kind):
    if kind == "full":
        return dict(C=C, lo_c=LO, lo_s=LO)
    if kind == "dead":
        return dict(C=C, lo_c=LO, lo_s=LO, dead_c=dead_tail(C), dead_s=dead_tail(C))
    assert kind == "rank" and C in RANK_WIDTHS
    return dict(C=C, lo_c=LO, lo_s=LO, n=C - 11, rank_c=C - 12)


#: name -> keyword arguments of make_case; the seed is a function of the name
CASES = collections.OrderedDict()
for _C in WIDTHS:
    for _kind in ("full", "dead") + (("rank",) if _C in RANK_WIDTHS else ()):
        CASES["C%d_%s" % (_C, _kind)] = _spec(_C, _kind)


def names(C):
    return [n for n, s in CASES.items() if s["C"] == C]


def seed_of(name):
    return 1000 * CASES[name]["C"] + ("full", "dead", "rank").index(name.split("_")[1])


def make_case(seed, C, lo_c, lo_s, n=50000, dead_c=(), dead_s=(), rank_c=None, rank_s=None):
    """(n, sum_c, sumsq_c, style statistics in the export layout) of two seeded covariances with eigenvalues 1 .. lo_c / lo_s; dead_*:
    channels whose rows and columns are exactly zero; rank_*: only that many eigen-directions are kept."""
    rng = np.random.default_rng(seed)
    cov_c = O.spd(rng, C, lo_c, dead_c, rank_c)
    cov_s = O.spd(rng, C, lo_s, dead_s, rank_s)
    mu_c, mu_s = rng.random(C), rng.random(C)
    for d in dead_c:
        mu_c[d] = 0.0
    for d in dead_s:
        mu_s[d] = 0.0
    n, s, ss = O.raw(n, mu_c, cov_c)
    S = O.sym_pow(cov_s, 0.5)
    S[list(dead_s), :] = 0.0                    # a slot's dead channels are exact zeros (solve.hip zeroes them in its result)
    S[:, list(dead_s)] = 0.0
    return n, s, ss, O.stats(S, mu_s)


def build(name):
    return make_case(seed_of(name), **CASES[name])


def describe(n, s, ss, st):
    """What the reference alone says of a case: cond(B) on B's live block, its rank there, the number of live (not axis-aligned zero)
    channels of B, and the content covariance's rank."""
    _, cov_c = O.mean_cov(n, s, ss)
    S, _ = O.split_stats(st)
    B = O.ot_B(cov_c, S)
    lam = np.linalg.eigvalsh(B)
    keep = lam[lam > O.REL * lam.max()]
    dB = np.diag(B)
    lc = np.linalg.eigvalsh(cov_c)
    return dict(cond=float(keep.max() / keep.min()), rank=int(keep.size), live=int((dB > 1e-13 * dB.max()).sum()),
                rank_c=int((lc > O.REL * lc.max()).sum()))
