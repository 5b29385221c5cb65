"""Every loadable width through the feature-space kernels: the launch arithmetic restated, and the cases derived from it.
CPU only: no torch, no GPU (tests/test_sweep_cpu.py checks it, tests/test_sweep_gpu.py runs it).

`wct_load_module` accepts every width that is a multiple of 4 up to 512, and every kernel that consumes a C-channel feature map sizes
its tiles from C and the pixel count.  This module restates that arithmetic, one function per launcher:

    plan / blk_plan / moments_launch    moments.hip plan(), blk_plan(), launch_moments (with moments_reg_kernel's re-chunking)
    plan_kw                             regions.hip plan_labeled() == blend.hip plan_weighted()
    apply_pt                            the PT tile of apply_labeled_kernel / apply_mixed_kernel
    fold_form                           wct_api.hip fold_impl / fold_fast_impl -> misc.hip launch_fold_affine, launch_fold_fast, solve.hip launch_fold_gemm
    eig_front_end                       solve.hip launch_eig

and derives, per width, the boundary shapes at which those plans can go wrong.  The library reports what it really chose through the
profile names under wct_debug_set("prof_forms", 1) (include/wct_hip.h); the GPU test holds every report against `suffix` here, so a
restatement that drifts from the C++ fails there.

The plan functions take npix as an int or as a numpy int64 array (the CPU test walks 1..3000 at once)."""
from __future__ import annotations

import collections

import numpy as np

# --------------------------------------------------------------------------------------------------------- widths and bands
WIDTHS = tuple(range(4, 513, 4))
N_BANDS = 16
#: inside a band: large, small, largest, ... -- a buffer grown for a wide map is reused by a narrow one (never monotonic)
_BAND_ORDER = (5, 0, 7, 2, 4, 1, 6, 3)


def band(b: int):
    """The 8 widths of band b: 4 (b + 1) + 64 k -- one width out of every 64-channel octave, in a fixed non-monotonic order."""
    assert 0 <= b < N_BANDS
    return tuple(4 * (b + 1) + 64 * k for k in _BAND_ORDER)


BANDS = tuple(band(b) for b in range(N_BANDS))

# --------------------------------------------------------------------------------------------------------- moments.hip
MAXLD = 8                # float4 load slots per thread and tile the kernel is instantiated for
MAXLD6 = 6               # with six pairs per wave
NPC_TARGET = 512         # chunks over all pair groups
MW_PRE = 8               # blend.hip: float4 per thread of one tile
LDS_LIMIT = 160 * 1024   # bytes of LDS a workgroup may ask for on gfx950
MOM32_MIN_PIXELS = 65536


def _cdiv(a, b):
    return (a + b - 1) // b


def geometry(C: int):
    """The part of plan() that depends on C alone."""
    T = (C + 15) // 16
    NP = T * (T + 1) // 2
    pixsplit = NP <= 6
    pw = (3 if NP <= 3 else 6) if pixsplit else (3 if NP <= 12 else 6)
    NPG = 1 if pixsplit else _cdiv(NP, 4 * pw)
    Cs = T * 16 if T & 1 else T * 16 + 16
    maxld = MAXLD6 if pw == 6 else MAXLD
    MP = max(16, min(256, (maxld * 256 * 4 // C) // 16 * 16))
    if pixsplit:
        MP = max(64, MP // 64 * 64)
    NLD = _cdiv(MP * (C // 4), 256)
    return dict(C=C, T=T, NP=NP, pixsplit=pixsplit, PW=pw, NPG=NPG, Cs=Cs, MP=MP, NLD=NLD)


def plan(C: int, npix):
    """moments.hip plan(): geometry + the chunking of npix pixels."""
    g = geometry(C)
    MP = g["MP"]
    npc = NPC_TARGET // g["NPG"]
    if g["NP"] > 16 and npc > 512:
        npc = 512
    npc = np.maximum(np.minimum(npc, _cdiv(npix, MP)), 1)
    chunk = _cdiv(_cdiv(npix, npc), MP) * MP
    g.update(npix=npix, chunk=chunk, NPC=np.maximum(_cdiv(npix, chunk), 1))
    return g


def npc_target(C: int) -> int:
    g = geometry(C)
    npc = NPC_TARGET // g["NPG"]
    return max(1, 512 if (g["NP"] > 16 and npc > 512) else npc)


def blk_plan(C: int, npix):
    """moments.hip blk_plan(): chunks of moments_blk_kernel (C a multiple of 128)."""
    nb = C >> 7
    nbp = nb * (nb + 1) // 2
    npc = np.maximum(1, np.minimum(512 // nbp, _cdiv(npix, 256)))
    chunk = _cdiv(_cdiv(npix, npc), 64) * 64
    return chunk, _cdiv(npix, chunk)


def moments_launch(C: int, npix, f32: bool):
    """launch_moments: which kernel, its chunking, its LDS bytes and the profile suffix it reports."""
    a = plan(C, npix)
    if f32 and C in (32, 64):                                   # moments_reg_kernel: chunks of whole 256-pixel passes
        chunk = _cdiv(a["chunk"], 256) * 256
        a.update(family="r", chunk=chunk, NPC=_cdiv(npix, chunk), lds=(2 * a["NP"] * 256 + 2 * C) * 8, gran=256,
                 suffix="r256.16.%d%s" % (a["NP"], "f"))
        return a
    big = np.asarray(npix) >= 4096
    assert big.all() or not big.any(), "an npix array must lie on one side of the 4096-pixel threshold"
    if not f32 and C >= 512 and C % 128 == 0 and big.all():
        chunk, npc = blk_plan(C, npix)
        a.update(family="b", chunk=chunk, NPC=npc, lds=0, gran=64, suffix="b64.2.4d")
        return a
    lds = a["MP"] * a["Cs"] * 4
    if a["pixsplit"]:
        lds = max(lds, (4 * a["NP"] * 256 + 4 * a["T"] * 16) * 8)
    a.update(family="l", lds=lds, gran=a["MP"],
             suffix="l%d.%d.%d%s%s" % (a["MP"], min(a["NLD"], MAXLD), a["PW"], "s" if a["pixsplit"] else "", "f" if f32 else "d"))
    return a


def moments_workspace_doubles(C: int, npix):
    """moments_workspace_bytes / 8"""
    a = plan(C, npix)
    npc = a["NPC"]
    if C >= 256 and C % 128 == 0:
        npc = np.maximum(npc, blk_plan(C, npix)[1])
    return npc * a["NP"] * 256 + npc * a["T"] * 16


def moments_partials_doubles(launch):
    """what the chosen kernel writes: [NPC][NP][256] + [NPC][T * 16]"""
    return launch["NPC"] * launch["NP"] * 256 + launch["NPC"] * launch["T"] * 16


# --------------------------------------------------------------------------------------------------------- regions.hip / blend.hip
def apply_pt(C: int) -> int:
    """pixels per workgroup of apply_labeled_kernel / apply_mixed_kernel (and the MP of the labeled / weighted moments)"""
    return 64 if C <= 128 else 32 if C <= 256 else 16


def plan_kw(C: int, npix):
    """regions.hip plan_labeled() and blend.hip plan_weighted(): the same arithmetic."""
    T = (C + 15) // 16
    NP = T * (T + 1) // 2
    Cs = T * 16 if T & 1 else T * 16 + 16
    MP = apply_pt(C)
    PW = 2 if NP <= 8 else 8
    npg = _cdiv(NP, 4 * PW)
    npc = np.minimum(max(1, 1024 // npg), _cdiv(npix, MP))
    chunk = _cdiv(_cdiv(npix, npc), MP) * MP
    return dict(C=C, T=T, NP=NP, Cs=Cs, MP=MP, PW=PW, NPG=npg, NLD=_cdiv(MP * (C // 4), 256), npix=npix, chunk=chunk, NPC=_cdiv(npix, chunk),
                lds=MP * Cs * 4 + MP * 4, npc_target=max(1, 1024 // npg))


def kw_suffix(C: int, f32: bool) -> str:
    a = plan_kw(C, 1)
    return "l%d.%d.%d%s" % (a["MP"], a["NLD"], a["PW"], "f" if f32 else "d")


def apply_lds(C: int, K: int, mixed: bool) -> int:
    Cp = (C + 15) // 16 * 16
    PT = apply_pt(C)
    return PT * (Cp + 4) * 4 + (K * PT * 4 if mixed else PT * 4)


# --------------------------------------------------------------------------------------------------------- folds
def pad_cout(c: int) -> int:
    return 16 if c <= 16 else 32 if c <= 32 else 64 if c <= 64 else (c + 127) // 128 * 128


def fold_gemm_capable(cout: int, cin: int, cout_pad: int) -> bool:
    return cin >= 256 and cin % 128 == 0 and cout % 32 == 0 and cout_pad == cout


def fold_fast_capable(cin: int) -> bool:
    ipad = (cin + 15) // 16 * 16
    return cin <= 128 and ipad <= 128 and 256 % ipad == 0


FOLD_FORMS = ("fra", "frg", "fb", "fg", "ff")     # row kernel aligned / generic path, block kernel, fp64 GEMM, fast fold


def fold_form(cin: int, cout: int, foldgemm: bool = True, fast: bool = False) -> str:
    """The suffix of "fold_affine" for a decoder whose first conv is cin -> cout.  fast: the call folds on the cascade's path (the
    level / stylize entries) with "fastfold" on; wct_decode_affine and wct_content_decode fold from (M, b)."""
    if fast and fold_fast_capable(cin):
        return "ff"
    if foldgemm and fold_gemm_capable(cout, cin, pad_cout(cout)):
        return "fg"
    if cin >= 256:
        return "fb"
    ipad = (cin + 15) // 16 * 16
    return "fra" if 256 % ipad == 0 else "frg"


# --------------------------------------------------------------------------------------------------------- launch_eig
def ns_pad(C: int) -> int:
    return (C + 63) // 64 * 64 if C > 128 else (C + 31) // 32 * 32


def eig_is_big(C: int, wide_model: bool) -> bool:
    return C > 128 or (wide_model and C > 64 and ns_pad(C) % 64 == 0)


EIG_FRONT_ENDS = ("lds32", "lds64", "multi96", "coop128", "deflated4", "deflated8")


def eig_front_end(C: int, wide_model: bool = False, nscoop: bool = True) -> str:
    """The front end of launch_eig; deflated<NS>: the deflated iteration on ns_*_wide_kernel<NS> tiles."""
    Cp = ns_pad(C)
    if eig_is_big(C, wide_model):
        return "deflated8" if Cp >= 256 and Cp % 128 == 0 else "deflated4"
    if Cp <= 32:
        return "lds32"
    if Cp == 64:
        return "lds64"
    if Cp == 128:
        return "coop128" if nscoop else "multi128"
    return "multi96"


# --------------------------------------------------------------------------------------------------------- cases
Case = collections.namedtuple("Case", "name h wfull x0 x1")      # window rows [0, h) x cols [x0, x1) of an h x wfull map


def npix_of(c: Case) -> int:
    return c.h * (c.x1 - c.x0)


def three_tile_npix(tile: int, npc_t: int) -> int:
    """The smallest pixel count at which a chunk holds three tiles, plus 1: the last chunk is ragged and the prefetch wraps."""
    return 2 * tile * npc_t + 2


def tile_cases(tile: int, npc_t: int, window: bool = True, big: bool = True):
    """The boundary shapes of a kernel that walks `tile` pixels at a time in at most `npc_t` chunks.  window = False: the entry takes
    whole maps only (labeled / weighted moments, the apply kernels): the windowed cases keep their pixel counts."""
    n3 = (2 * tile // 3 + 1) * 3
    ww = n3 // 3
    out = [Case("one", 1, 1, 0, 1),
           Case("row-1", 1, tile - 1, 0, tile - 1) if tile > 1 else None,
           Case("row", 1, tile, 0, tile),
           Case("row+1", 1, tile + 1, 0, tile + 1),
           Case("two", 2, tile, 0, tile),
           Case("two+1", 1, 2 * tile + 1, 0, 2 * tile + 1),
           Case("win3", 3, ww + 5, 2, 2 + ww) if window else Case("win3", 3, ww, 0, ww),
           Case("col", 7, 9, 8, 9) if window else Case("col", 7, 9, 0, 9)]
    if big:
        n = three_tile_npix(tile, npc_t)
        out.append(Case("three+1", 2, n // 2, 0, n // 2))
    return [c for c in out if c is not None]


def moments_cases(C: int):
    return tile_cases(geometry(C)["MP"], npc_target(C))


def kw_cases(C: int):
    a = plan_kw(C, 1)
    return tile_cases(a["MP"], a["npc_target"], window=False)


def apply_cases(C: int):
    """(h, w) of the apply kernels: the small boundary counts with PT in place of MP (2 x 2 is the smallest map wct_apply takes)"""
    return [c for c in tile_cases(apply_pt(C), 1, window=False, big=False)]


# --------------------------------------------------------------------------------------------------------- inputs and references
DEAD_CH, SMALL_CH = 1, 2


def spike(npix: int) -> float:
    """The factor on the two sentinel pixels (the last one, the first of the second tile): a lost or doubled pixel must move the fp64
    reference by more than ten times the fp32-form bound, which grows with the pixel count (tests/test_sweep_cpu.py)."""
    return 4.0 + 0.05 * float(np.sqrt(npix))


def feature(C: int, case: Case, tile: int, seed: int) -> np.ndarray:
    """h x wfull x C fp32, mixed sign, channel 1 dead, channel 2 at 1e-3 scale, the window's sentinel pixels spiked."""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((case.h, case.wfull, C), dtype=np.float32)
    f += np.float32(0.25)
    f[..., DEAD_CH] = 0
    f[..., SMALL_CH] *= np.float32(1e-3)
    ww, n = case.x1 - case.x0, npix_of(case)
    for p in {n - 1, tile if tile < n else n - 1}:
        f[p // ww, case.x0 + p % ww] *= np.float32(spike(n))
    return f


def window_pixels(f: np.ndarray, case: Case) -> np.ndarray:
    """the window's pixels in the kernels' order, fp64 [npix][C]"""
    return np.asarray(f[:, case.x0:case.x1], np.float64).reshape(-1, f.shape[-1])


def raw_moments(X: np.ndarray, w: np.ndarray = None):
    """(sum, sumsq, |.| sum, |.| sumsq) of fp64 pixels [n][C], optionally weighted per pixel: the reference and the magnitudes that
    the fp32-form bound scales with."""
    Xw = X if w is None else X * np.asarray(w, np.float64)[:, None]
    A, Aw = np.abs(X), np.abs(Xw)
    return Xw.sum(0), Xw.T @ X, Aw.sum(0), Aw.T @ A


#: the project's gate of the fp64 form: 1e-13 of the largest entry
GATE64 = 1e-13
#: fp32 products in blocks of <= 64 pixels, block totals in fp64: one rounding per product and one per addition of a block
F32_SQ, F32_SUM = 130 * 2.0 ** -24, 65 * 2.0 ** -24


def bound_f32(asum: np.ndarray, asq: np.ndarray, sq: np.ndarray):
    """entrywise bounds (sum, sumsq) of the fp32-block form"""
    return F32_SUM * asum, F32_SQ * asq + GATE64 * max(float(np.abs(sq).max()), 1e-300)
