"""Image sizes that put every size-selected convolution kernel form on the path, with ragged tiles (tests/test_geometry_cpu.py,
tests/test_geometry_gpu.py).  CPU only: no torch, no GPU.

The convolution launchers choose a kernel form from the image size and the CU count (conv3x3_f16.hip launch_enc_head,
launch_dec_tail, launch_conv3x3_f16; level1.hip launch_l1_decode; conv3x3_sp.hip launch_conv3x3_sp).  This module restates those
choices in Python (`*_form`), walks a module's layer graph the way wct_api.hip encode_impl / decode_impl do (`predict_names`: the
profile names a call must produce under wct_debug_set("prof_forms", 1)), and searches, for a CU count, the image sizes that sit
just below and at / just above every threshold with the same kind of raggedness on both sides (`cases`).

A case is (kind, mode, level, H, W, switches, expect):
    kind      "enc": wct_encode of an H x W image;  "dec": wct_decode of the level's feature of an H x W image (H x W is the decoded
              image);  "l1": wct_content_encode + wct_content_decode at level 1 (fused level-1 moments and decode)
    mode      "16x" (weights/16x.npz, tests/width_models.W16X) or "original" (model_zoo.synth_weights("original", 7))
    switches  wct_debug_set keys other than their defaults, e.g. {"upconv": 0}
    expect    the profile names (with form suffix) the call must produce in conv mode 1
"""
from __future__ import annotations

import functools
import math
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from tests import width_models as wm
from wct_hip import model_zoo

FTW = 32          # tile width of every conv kernel (conv_f16_dev.h)
SPH = 16          # tile height of the persistent DMA-staged kernels (conv3x3_sp.hip)

#: the intended size limit of a case's image (the fp64 reference of a 16x encoder takes seconds there), and the hard one: the 9 % more
#: that a 304-CU part needs to cross the thresholds that count whole tiles per CU.  A search goes past the first only when it must.
TARGET_PIXELS = 2_200_000
MAX_PIXELS = 2_400_000

#: widths of --mode original in width_models' terms
W_ORIGINAL = {1: 64, 2: 128, 3: 256, 4: 512, 5: 512, "l1": 64}
WIDTHS = {"16x": wm.W16X, "original": W_ORIGINAL}

#: every kernel form the DEFAULT switches must reach over `cases(cus)` -- "<family prefix>#<form><tile height>".  A threshold change that
#: orphans a kernel shows up as a form missing here (test_geometry_gpu.py part c).  Not listed: enc_head_kernel<24> (runs only with
#: the two-role head off, WCT_HEAD_ROLES=0 / WCT_HEAD_TH=24) and the nine-tap fused tails (debug_set("upconv", 0)).
FORMS = (
    "enc_head_fused<3-16-16,pool>#t8", "enc_head_fused<3-16-16,pool>#r16",
    "dec_tail_fused<16-16-3>#u8", "dec_tail_fused<16-16-3>#u16",
    "l1_decode_fused<3-24-3>#t8", "l1_decode_fused<3-24-3>#t16",
    "conv3x3_f16x3<co=128>#s8", "conv3x3_f16x3<co=128>#t16", "conv3x3_f16x3<co=64>#t8", "conv3x3_f16x3<co=16>#t8",
    "conv3x3_f16x3<co=32,dma>#316", "conv3x3_f16x3<co=32,pool,dma>#316", "conv3x3_f16x3<co=64,dma>#t16", "conv3x3_f16x3<co=128,dma>#t16",
    "conv3x3_f16x3<co=32,dma,up>#u16", "conv3x3_f16x3<co=64,dma,up>#u16", "conv3x3_f16x3<co=128,dma,up>#u16",
)
#: forms that need a switch (covered by cases with `switches`)
FORMS_SWITCHED = ("dec_tail_fused<16-16-3>#t8", "dec_tail_fused<16-16-3>#t16", "dec_tail_fused<16-16-3>#t24")


class Case(NamedTuple):
    kind: str
    mode: str
    level: int
    H: int
    W: int
    switches: Tuple[Tuple[str, int], ...]
    expect: Tuple[str, ...]
    why: str

    @property
    def id(self) -> str:
        sw = "".join("-%s%d" % kv for kv in self.switches)
        return "%s%d-%s-%dx%d%s" % (self.kind, self.level, self.mode, self.H, self.W, sw)

    @property
    def multi(self) -> bool:
        """some launch of the case walks more than one (tile, cout group) unit per workgroup"""
        return any(n.endswith("m") and "#" in n for n in self.expect)


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


# --------------------------------------------------------------------------------------------------------- launcher restatements
def _sfx(form: str, th: int, units: int, grid: int) -> str:
    return "#%s%d%s" % (form, th, "m" if units > grid else "")


def head_form(H: int, W: int, cus: int) -> str:
    """launch_enc_head: two roles on 32 x 16 tiles from 4 tiles per CU on, else 32 x 8 tiles, three workgroups per CU."""
    tx = _cdiv(W, FTW)
    if _cdiv(H, 16) * tx >= 4 * cus:
        nt = tx * _cdiv(H, 16)
        return _sfx("r", 16, nt, min(nt, cus))
    nt = tx * _cdiv(H, 8)
    return _sfx("t", 8, nt, min(nt, 3 * cus))


def tail_form(H: int, W: int, cus: int, up: bool) -> str:
    """launch_dec_tail: tile height 8 / 16 (2 CUs' worth of 16-row tiles) / 24 (4 CUs' worth of 24-row tiles); the upsample form runs
    16 where the nine-tap form runs 24, two workgroups per CU."""
    tx = _cdiv(W, FTW)
    th = 24 if _cdiv(H, 24) * tx >= 4 * cus else 16 if _cdiv(H, 16) * tx >= 2 * cus else 8
    if up:
        th = 16 if th == 24 else th
        nt = tx * _cdiv(H, th)
        return _sfx("u", th, nt, min(nt, 2 * cus))
    nt = tx * _cdiv(H, th)
    return _sfx("t", th, nt, min(nt, (2 if th == 8 else 1) * cus))


def l1dec_form(H: int, W: int, cus: int) -> str:
    """launch_l1_decode: 32 x 16 tiles, one workgroup per CU, from 2 tiles per CU on; else 32 x 8, two per CU."""
    tx = _cdiv(W, FTW)
    tall = _cdiv(H, 16) * tx >= 2 * cus
    nt = tx * _cdiv(H, 16 if tall else 8)
    return _sfx("t", 16 if tall else 8, nt, min(nt, (1 if tall else 2) * cus))


def f16_form(h: int, w: int, cout_pad: int, cus: int) -> str:
    """launch_conv3x3_f16 (register-staged): 128-cout layers on 32 x 16 tiles, or the small-map form (32 x 8, cout groups of 64) while
    the 32 x 16 tiles do not fill the chip; one workgroup per (tile, group)."""
    if cout_pad == 16:
        return "#t8"
    ct, groups = cout_pad // 32, 1
    if ct > 4:
        groups, ct = cout_pad // 128, 4
    if ct == 4 and _cdiv(w, FTW) * _cdiv(h, 16) * groups < cus:
        return "#s8"
    return "#t16" if ct == 4 else "#t8"


def sp_units(h: int, w: int, cin: int, cout_pad: int, up: bool, cus: int) -> Tuple[str, int, int, int]:
    """launch_conv3x3_sp on an h x w output: (form, tiles, units = tiles x cout groups, grid)."""
    if up:
        nt, groups, form = _cdiv(w // 2, FTW) * _cdiv(h // 2, SPH), 2 * (cout_pad // 32), "u"
    else:
        ct = 2 if cout_pad % 64 == 0 else 1
        nt, groups = _cdiv(w, FTW) * _cdiv(h, SPH), cout_pad // (ct * 32)
        form = "3" if cout_pad == 32 and _cdiv(cin, 16) <= 2 else "t"
    grid = min(8 * _cdiv(nt, 8) * groups, max(cus & ~7, 8))
    return form, nt, nt * groups, grid


def sp_form(h: int, w: int, cin: int, cout_pad: int, up: bool, cus: int) -> str:
    form, _, units, grid = sp_units(h, w, cin, cout_pad, up, cus)
    return _sfx(form, SPH, units, grid)


def _family(cout_pad: int, pool: bool, out3: bool, dma: bool, up: bool) -> str:
    """wct_api.hip run_conv's family name of an f16x3 layer behind the first conv"""
    return "conv3x3_f16x3<co=%d%s%s%s%s>" % (min(cout_pad, 128), ",pool" if pool else "", ",out3" if out3 else "", ",dma" if dma else "",
                                             ",up" if up else "")


def _sp_ok(cin: int, cout: int, cout_pad: int, out3: bool) -> bool:
    """conv_sp_supported"""
    return not out3 and cin % 16 == 0 and 32 <= cout_pad <= 512 and cout % 8 == 0


def predict_names(kind: str, mode: str, level: int, H: int, W: int, cus: int, switches: Dict[str, int] = {}) -> Tuple[str, ...]:
    """Profile names (prof_forms on, conv mode 1, the given non-default switches) of the size-selected launches of one call, in launch
    order, duplicates removed.  Supports what `cases` uses: the shipped 16x and the original layer graphs, the "upconv" switch."""
    assert set(switches) <= {"upconv"}, switches
    upconv = bool(switches.get("upconv", 1))
    names: List[str] = []
    if kind == "l1":
        assert mode == "16x" and level == 1
        return ("l1_moments_fused<3-24>", "l1_decode_fused<3-24-3>" + l1dec_form(H, W, cus))
    if kind == "enc":
        layers = model_zoo.encoder_layers(mode, level)
        n, h, w, i0 = len(layers), H, W, 1
        if mode == "16x" and level == 1:
            return ("l1_encode<3-24>",)
        if mode == "16x":                                   # conv11 + conv12 + pool in one kernel
            names.append("enc_head_fused<3-16-16,pool>" + head_form(H, W, cus))
            h, w, i0 = h // 2, w // 2, 2
        else:                                               # the 3 -> 64 first conv: one form
            names.append("conv3x3_fp32<co=64,in3>")
        for i in range(i0, n):                              # every later layer reads SP16 (cin % 16 == 0 in both graphs)
            l = layers[i]
            cp = wm.pad_cout(l.cout)
            assert _sp_ok(l.cin, l.cout, cp, False)
            names.append(_family(cp, l.pool_after, False, True, False) + sp_form(h, w, l.cin, cp, False, cus))
            if l.pool_after:
                h, w = h // 2, w // 2
    else:
        layers = model_zoo.decoder_layers(mode, level)
        n = len(layers)
        h, w = H >> (level - 1), W >> (level - 1)
        cur_sp = False
        for i, l in enumerate(layers):
            up_in = i > 0 and layers[i - 1].up_after
            if up_in:
                h, w = 2 * h, 2 * w
            last = i + 1 == n
            cp = wm.pad_cout(l.cout)
            if i + 2 == n and l.cin == 16 and l.cout == 16 and layers[i + 1].cin == 16 and layers[i + 1].cout == 3:
                names.append("dec_tail_fused<16-16-3>" + tail_form(h, w, cus, up_in and upconv))
                break
            dma = cur_sp and _sp_ok(l.cin, l.cout, cp, last)
            up = dma and upconv and up_in                  # wup16 exists for every SP-capable layer behind an upsample
            names.append(_family(cp, False, last, dma, up) + (sp_form(h, w, l.cin, cp, up, cus) if dma else f16_form(h, w, cp, cus)))
            cur_sp = not last and l.cout % 8 == 0
    return tuple(dict.fromkeys(names))


# --------------------------------------------------------------------------------------------------------- size search
def _search(what: str, prefer: Sequence[Tuple[int, int]], ok: Callable[[int, int], Optional[float]], h_mod: Tuple[int, Sequence[int]],
            w_mod: Tuple[int, Sequence[int]], scale: int = 1) -> Tuple[int, int]:
    """The image size (H, W) with the smallest ok(H, W) (distance from the threshold; None = not a candidate) among H = scale h,
    W = scale w... with H % h_mod[0] in h_mod[1], W % w_mod[0] in w_mod[1], W >= H, W <= 16 H, H W <= MAX_PIXELS.  `prefer` sizes win
    when they are candidates at all (the issue's table for 256 CUs).  Deterministic; raises when nothing qualifies."""
    for H, W in prefer:
        if H % h_mod[0] in h_mod[1] and W % w_mod[0] in w_mod[1] and H * W <= MAX_PIXELS and ok(H, W) is not None:
            return H, W
    for limit in (TARGET_PIXELS, MAX_PIXELS):            # the larger limit only where the intended one reaches nothing
        best = None
        for H in (b + r for b in range(0, 2200, h_mod[0]) for r in h_mod[1]):
            if H < 34:
                continue
            for W in (b + r for b in range(H // w_mod[0] * w_mod[0], min(16 * H, limit // H) + 1, w_mod[0]) for r in w_mod[1]):
                if W < max(H, 66) or H * W > limit:
                    continue
                d = ok(H, W)
                if d is None:
                    continue
                key = (d, abs(math.log(W / H / 1.9)), H, W)
                if best is None or key < best:
                    best = key
        if best is not None:
            return best[2], best[3]
    raise ValueError("geometry_cases: no image of at most %d pixels reaches '%s'" % (MAX_PIXELS, what))


def cases(cus: int) -> List[Case]:
    """Every case for a device with `cus` compute units (the preferred sizes are those of 256).  Raises if a form cannot be reached."""
    return list(_cases(int(cus)))


@functools.lru_cache(maxsize=None)
def _cases(cus: int) -> Tuple[Case, ...]:
    out: List[Case] = []

    def add(kind, mode, level, H, W, why, **switches):
        assert H * W <= MAX_PIXELS, (kind, level, H, W)
        sw = tuple(sorted(switches.items()))
        if any((c.kind, c.mode, c.level, c.H, c.W, c.switches) == (kind, mode, level, H, W, sw) for c in out):
            return
        out.append(Case(kind, mode, level, H, W, sw, predict_names(kind, mode, level, H, W, cus, switches), why))

    odd_w = (32, (1, 9, 31))

    # ---- fused encoder head (levels 5 and 2): H, W odd (floor pooling drops a row / column), ragged right and bottom tiles
    def head_n(H, W):
        return _cdiv(H, 16) * _cdiv(W, FTW)
    T = 4 * cus
    below = _search("head below the two-role threshold", [(489, 1001)], lambda H, W: (T - head_n(H, W)) if T - _cdiv(W, FTW) <= head_n(H, W) < T and
                    _cdiv(H, 8) * _cdiv(W, FTW) > 3 * cus else None, (16, (7, 9)), odd_w)
    at = _search("head at the two-role threshold", [(505, 1001)], lambda H, W: (head_n(H, W) - T) if head_n(H, W) >= T else None, (16, (7, 9)), odd_w)
    for level in (5, 2):
        add("enc", "16x", level, *below, "head: 32 x 8 tiles, several per workgroup, one tile row below the two-role threshold")
        add("enc", "16x", level, 67, 95, "head: 32 x 8 tiles, one per workgroup")
        add("enc", "16x", level, *at, "head: two roles at the threshold")
        add("enc", "16x", level, 1031, 1953, "head: two roles, many tiles per workgroup; 272 tiles of the 1/4-resolution layers")

    # ---- persistent DMA-staged kernels inside the 16x encoders: the 64-cout layers at 1/4 resolution, one cout group
    def sp_pred(scale, cin, cp, up, groups_above: bool, rem: int):
        def ok(H, W):
            form, nt, units, grid = sp_units(H // scale, W // scale, cin, cp, up, cus)
            if nt % 8 != rem or (units > grid) != groups_above:
                return None
            return abs(units - max(cus & ~7, 8))
        return ok
    sp_enc = [(False, 7, [(1031, 1889)]), (False, 1, []), (True, 0, [(1031, 1953)]), (True, 1, []), (True, 7, [])]
    for above, rem, prefer in sp_enc:
        H, W = _search("1/4-resolution SP layer, units %s the grid, tiles %% 8 = %d" % (">" if above else "<=", rem), prefer,
                       sp_pred(4, 64, 64, False, above, rem), (16, (7, 9)), odd_w)
        for level in ((5, 4, 3) if rem in (7, 0) else (5,)):
            add("enc", "16x", level, H, W, "SP kernels: %d tiles at 1/4 resolution (%s the grid, tiles %% 8 = %d)" %
                (sp_units(H // 4, W // 4, 64, 64, False, cus)[1], "above" if above else "within", rem))
    if 1095 * 1953 <= MAX_PIXELS:
        add("enc", "16x", 5, 1095, 1953, "SP kernels: 288 tiles at 1/4 resolution")

    # ---- fused decoder tail behind d2 (H, W = 2 x odd) and d3 (multiples of 4), upsample and nine-tap forms
    def tail_n(H, W, th):
        return _cdiv(H, th) * _cdiv(W, FTW)
    for level, hm, hm24, wmod, pref in ((2, (16, (14,)), (24, (2,)), (32, (2, 30)), [(494, 510), (510, 510), (526, 510), (1034, 770)]),
                                        (3, (16, (12,)), (24, (4,)), (32, (4, 28)), [(492, 508), (508, 508), (524, 508), (1036, 772)])):
        T16, T24 = 2 * cus, 4 * cus
        sizes = [
            _search("tail below 16 rows", pref[0:1], lambda H, W: (T16 - tail_n(H, W, 16)) if tail_n(H, W, 16) < T16 else None, hm, wmod),
            _search("tail at 16 rows", pref[1:2], lambda H, W: (tail_n(H, W, 16) - T16) if tail_n(H, W, 16) >= T16 and tail_n(H, W, 24) < T24 else None, hm, wmod),
            _search("tail above 16 rows", pref[2:3], lambda H, W: (tail_n(H, W, 16) - T16) if tail_n(H, W, 16) > T16 and tail_n(H, W, 24) < T24 else None, hm, wmod),
            _search("tail at 24 rows", pref[3:4], lambda H, W: (tail_n(H, W, 24) - T24) if tail_n(H, W, 24) >= T24 else None, hm24, wmod),
        ]
        if level == 3:
            sizes = [sizes[0], sizes[3]]
        for H, W in sizes:
            for upconv in (1, 0):
                sw = {} if upconv else {"upconv": 0}
                add("dec", "16x", level, H, W, "tail: %s" % tail_form(H, W, cus, bool(upconv)), **sw)

    # ---- level 1: fused moments + fused decode
    def l1_n(H, W):
        return _cdiv(H, 16) * _cdiv(W, FTW)
    T = 2 * cus
    l1 = [_search("level-1 decode below 16 rows", [(239, 1001)], lambda H, W: (T - l1_n(H, W)) if l1_n(H, W) < T else None, (16, (11, 15)), (32, (9,))),
          _search("level-1 decode at 16 rows", [(251, 1001)], lambda H, W: (l1_n(H, W) - T) if l1_n(H, W) >= T else None, (16, (11,)), (32, (9,))),
          _search("level-1 decode above 16 rows", [(523, 1001)], lambda H, W: abs(l1_n(H, W) - 2 * T) if l1_n(H, W) > T + T // 2 else None, (16, (11,)), (32, (9,)))]
    for H, W in l1:
        add("l1", "16x", 1, H, W, "level-1 decode: %s" % l1dec_form(H, W, cus))

    # ---- register-staged kernel, 128 couts from an fp32 feature: the first conv of --mode original's d3 (256 -> 128)
    def f16_n(H, W):
        return _cdiv(H // 4, 16) * _cdiv(W // 4, FTW)
    small = _search("first decoder conv, small-map form", [(956, 2000)], lambda H, W: (cus - f16_n(H, W)) if f16_n(H, W) < cus else None, (64, (60,)), (128, (80,)))
    tall = _search("first decoder conv, 32 x 16 form", [(1000, 2000)], lambda H, W: (f16_n(H, W) - cus) if f16_n(H, W) >= cus else None, (64, (40,)), (128, (80,)))
    add("dec", "original", 3, *small, "first decoder conv (128 couts, fp32 input): small-map form; cout groups in the SP layers behind it")
    add("dec", "original", 3, *tall, "first decoder conv (128 couts, fp32 input): 32 x 16 form")

    # ---- persistent kernels inside the 16x decoders: d3 (upsample form, 2 groups), d4 (plain 64-cout layers at 2h x 2w), d5 (cout groups)
    for above, rem in ((False, 1), (True, 7), (True, 0)):
        H, W = _search("d3 upsample-form SP layer", [], sp_pred(2, 32, 32, True, above, rem), (16, (4, 12)), (32, (4, 12, 20, 28)))
        add("dec", "16x", 3, H, W, "SP upsample form: units %s the grid, tiles %% 8 = %d" % ("above" if above else "within", rem))
    for above, rem in ((False, 7), (True, 1)):
        H, W = _search("d4 plain SP layer", [], sp_pred(4, 64, 64, False, above, rem), (32, (8, 24)), (32, (8, 24)))
        add("dec", "16x", 4, H, W, "SP layers of d4: units %s the grid, tiles %% 8 = %d" % ("above" if above else "within", rem))
    H, W = _search("d5 SP layers with cout groups", [], sp_pred(8, 128, 128, False, False, 1), (16, (0,)), (32, (16,)))
    add("dec", "16x", 5, H, W, "SP layers of d5: two cout groups, units within the grid, tiles % 8 = 1")

    # ---- cout groups above the grid: --mode original e4 (128 -> 256 at 1/4 resolution: 4 groups) and d4
    H, W = _search("original e4, units above the grid", [(521, 1001)], sp_pred(4, 128, 256, False, True, 0), (16, (7, 9)), odd_w)
    add("enc", "original", 4, H, W, "SP kernel with cout groups: %d tiles x 4 groups at 1/4 resolution" % sp_units(H // 4, W // 4, 128, 256, False, cus)[1])
    add("dec", "original", 4, H - H % 8, W - W % 8, "SP kernels with cout groups in a decoder; small-map form with two groups of 128")
    return tuple(out)


# --------------------------------------------------------------------------------------------------------- failure reports
def locate(got: np.ndarray, ref: np.ndarray, tile_w: int, tile_h: int) -> str:
    """Where a (C, H, W) result differs most from its reference, in the terms a tiling bug is found by: the worst pixel, its place inside
    its tile_w x tile_h tile, whether it lies in the one-pixel border ring (reflect padding), the last tile row / column (ragged
    tiles) or the interior, and the worst error of those three regions (taken disjoint: the ring first, then the rest of the last tile
    row / column, then the interior).  Errors are relative to max |ref|."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and got.ndim == 3, (got.shape, ref.shape)
    C, H, W = ref.shape
    scale = max(float(np.abs(ref).max()), 1e-30)
    err = np.abs(got - ref).max(axis=0) / scale                      # worst channel per pixel
    c, y, x = (int(v) for v in np.unravel_index(int(np.argmax(np.abs(got - ref))), ref.shape))
    yy, xx = np.mgrid[0:H, 0:W]
    ring = (yy == 0) | (yy == H - 1) | (xx == 0) | (xx == W - 1)
    last = ((yy >= (H - 1) // tile_h * tile_h) | (xx >= (W - 1) // tile_w * tile_w)) & ~ring
    regions = (("border ring", ring), ("last tile row/column", last), ("interior", ~ring & ~last))
    where = " and ".join(n for n, hit in (("border ring", bool(ring[y, x])), ("last tile row", y >= (H - 1) // tile_h * tile_h),
                                          ("last tile column", x >= (W - 1) // tile_w * tile_w)) if hit) or "interior"
    worst = ", ".join("%s %.3e" % (name, float(err[m].max()) if m.any() else 0.0) for name, m in regions)
    return ("max error %.3e at (c, y, x) = (%d, %d, %d) of %d x %d x %d: y %% %d = %d, x %% 32 = %d, tile (row %d, column %d) of %d x %d tiles of %d x %d, "
            "in the %s; worst per region: %s" % (float(err[y, x]), c, y, x, C, H, W, tile_h, y % tile_h, x % 32, y // tile_h, x // tile_w, _cdiv(H, tile_h),
                                          _cdiv(W, tile_w), tile_w, tile_h, where, worst))
