"""The cases tests/test_proxy_cpu.py and tests/test_proxy_edges_gpu.py share: the bilateral grid's fit and slice (include/wct_hip_bgrid.h) at the
edges of their launchers -- column supports either side of the fit's weight table, lane strides against the support's width, row chunks past
a vertex's support, more than 64 slabs of totals, a guide that leaves [0, 1], grids of one vertex per axis, slice launches that mix the LDS
and the global-memory path -- with their images and fp64 references (tests/proxy_oracle.py; computed once per process, read-only).

The counts the CPU test asserts (support widths, row chunks, slabs, tile footprints) are derived here from the header's rule through the
oracle's tent, not from the product.  numpy only: imports without a GPU."""
import functools

import numpy as np

from tests import color_oracle as CO
from tests import proxy_oracle as O
from tests.test_proxy_gpu import fit_pair, full_image, tone_curve          # that module imports without a GPU
from wct_hip import lib

ROWS, TW, TH, CAP = lib.BGRID_FIT_ROWS, lib.BGRID_TILE_W, lib.BGRID_TILE_H, lib.BGRID_LDS_VERTICES
SLAB = 256          # vertices per partial total (the header's "slabs of 256 vertices"; BG_SLAB of csrc/bgrid.hip)
TABLE = 256         # columns of a support whose tent weights the fit tabulates (BG_WX of csrc/bgrid.hip)
EPS, SMOOTH = (1e-2, 1e-4), (0, 1, 4)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---------------------------------------------------------------------------------------------------------------- images
def wide_image(seed, h, w):
    """CO.natural stretched over about [-0.74, 2] (unquantised fp32): tens to hundreds of pixels whose guide clamps to 0 and to 1.  The
    first four pixels in row-major order are 0, 1, 2 and -0.5 in all three channels, as many as the image has: luminance exactly 0 and
    exactly 1 (the last bin with f == 1), and one pixel beyond either end."""
    x = (CO.natural(seed, h, w) - 0.2) / 0.54 * 1.75 - 0.25
    x = np.ascontiguousarray(x, np.float32)
    flat = x.reshape(3, -1)
    for p, v in enumerate((0.0, 1.0, 2.0, -0.5)[:h * w]):
        flat[:, p] = v
    return x


def wide_pair(h, w):
    """(a wide-range reduced content, fit_pair's tone curve of it clipped at 0): what a cascade result or an HDR input hands the fit."""
    c = wide_image(h * 7 + w, h, w)
    return c, tone_curve(np.maximum(c, 0.0))


@functools.lru_cache(maxsize=None)
def fit_images(h, w, kind):
    return _frozen(*(wide_pair(h, w) if kind == "wide" else fit_pair(h, w)))


@functools.lru_cache(maxsize=None)
def slice_image(H, W, kind):
    return _frozen(wide_image(H * 11 + W + 3, H, W) if kind == "wide" else full_image(H, W))[0]


# ---------------------------------------------------------------------------------------------------------------- the fit's cases
#: (h, w, gz, gh, gw, image kind, why).  rw: the columns of a vertex's support
EDGE_FIT_SHAPES = [
    # column supports against the weight table of TABLE columns
    (4, 256, 2, 2, 2, "fit", "rw at the table's size"),
    (5, 257, 2, 2, 2, "fit", "one column over the table: every weight evaluated in the loop"),
    (3, 300, 2, 1, 1, "fit", "one vertex across the image, untabulated"),
    (3, 600, 2, 1, 3, "fit", "three vertices, all untabulated: the outer two weigh on 300 columns, the inner one on 600"),
    (3, 500, 2, 1, 3, "fit", "the inner vertex untabulated (500 columns), the outer two tabulated (250): both branches in one launch"),
    (2, 1024, 1, 1, 2, "fit", "wide, one bin"),
    # the lane stride (64 / rw, 64 % rw) against the support's width
    (9, 63, 2, 1, 1, "fit", "rw one below 64"),
    (9, 64, 2, 1, 1, "fit", "rw at 64: a lane stays in its column"),
    (9, 65, 2, 1, 1, "fit", "rw one above 64"),
    (6, 128, 2, 1, 1, "fit", "rw a multiple of 64"),
    (100, 1, 2, 3, 1, "fit", "rw == 1: a lane advances 64 rows"),
    # row chunks past a vertex's support
    (200, 7, 2, 3, 2, "fit", "the inner vertex has 4 row chunks, the outer ones 2: all-zero partials"),
    (193, 5, 3, 4, 1, "fit", "supports that start inside a chunk of the image's rows"),
    # the totals over the slabs
    (24, 24, 16, 32, 32, "fit", "64 slabs exactly: one per lane"),
    (24, 24, 5, 29, 113, "fit", "16385 vertices: 65 slabs, the last of one vertex"),
    (24, 24, 32, 23, 23, "fit", "67 slabs: two for three lanes"),
    (24, 24, 2, 91, 91, "fit", "65 slabs, and the 65th carries weight: z is the slowest axis, so under a grid of many bins the slabs past the "
                               "64th are the brightest bins, which no pixel of the three cases above reaches"),
    (24, 24, 2, 92, 92, "fit", "67 slabs, 2.5 % of all weight past the 64th"),
    (32, 40, 32, 2, 256, "fit", "the largest z and x axes together"),
    (20, 12, 1, 256, 3, "fit", "the largest y axis"),
    # the guide's clamp and the top bin
    (40, 56, 8, 3, 4, "wide", "eight bins under a guide that leaves [0, 1]"),
    (64, 96, 16, 5, 7, "wide", "sixteen bins"),
    (70, 90, 32, 6, 7, "wide", "the largest z axis"),
    (3, 5, 3, 4, 6, "wide", "more vertices than pixels"),
    (1, 1, 1, 1, 1, "wide", "a single black pixel"),
]
EDGE_FIT_CASES = [s[:6] + (eps, smooth) for s in EDGE_FIT_SHAPES for eps in EPS for smooth in SMOOTH]
POISON_SHAPES = [(200, 7, 2, 3, 2, "fit"), (193, 5, 3, 4, 1, "fit"), (5, 257, 2, 2, 2, "fit")]
POISON_CASES = [s + (eps, smooth) for s in POISON_SHAPES for eps, smooth in ((1e-2, 1), (1e-4, 0))]
#: smooth 0, most vertices unreached: they hold Ag, the totals of 65 slabs (the 65th all zero) and of 67 (weight in every one)
UNREACHED = [(24, 24, 5, 29, 113, "fit", 1e-2, 0), (24, 24, 2, 92, 92, "fit", 1e-2, 0)]


def fit_id(c):
    return "%dx%d-g%dx%dx%d-%s-eps%g-s%d" % c


@functools.lru_cache(maxsize=None)
def fit_reference(h, w, gz, gh, gw, kind, eps, smooth):
    """(cl, sl, the oracle's grid, Ag, the largest cond(Gv + lambda I)) of a fit case."""
    cl, sl = fit_images(h, w, kind)
    A, Ag, cond, _ = O.fit(cl, sl, gz, gh, gw, eps, smooth, details=True)
    return _frozen(cl, sl, A, Ag) + (cond,)


# ---------------------------------------------------------------------------------------------------------------- the header's rule, counted
def vertex_spans(n, G):
    """Per vertex of an axis with n samples and G vertices: (first, last) sample with a non-zero tent weight, None where there is none.
    The fit may cut its supports up to two samples more generously; never tighter."""
    i0, i1, f = O.axis(n, G)
    out = []
    for v in range(G):
        hit = np.nonzero(np.where(i0 == v, 1.0 - f, 0.0) + np.where(i1 == v, f, 0.0))[0]
        out.append((int(hit[0]), int(hit[-1])) if hit.size else None)
    return out


def support_widths(n, G):
    return [0 if s is None else s[1] - s[0] + 1 for s in vertex_spans(n, G)]


def row_chunks(h, gh):
    """Per y vertex (at least, at most) the row chunks of its support: of the weighted rows, and of two rows more."""
    return [(-(-n // ROWS), -(-min(n + 2, h) // ROWS)) for n in support_widths(h, gh)]


def slabs(gz, gh, gw):
    return -(-gz * gh * gw // SLAB)


def weight_past_slab(h, w, gz, gh, gw, kind, first=64):
    """The oracle's weight sum (before any blur) over the vertices of the slabs first, first + 1, ..: what a lane's second step adds."""
    Gv, _ = O.sums(*fit_images(h, w, kind), gz, gh, gw)
    return float(Gv[..., 3, 3].reshape(-1)[first * SLAB:].sum())


# ---------------------------------------------------------------------------------------------------------------- the slice's cases
#: (gz, gh, gw, H, W, image kind, why)
EDGE_SLICE_CASES = [
    (1, 1, 1, 9, 130, "full", "one vertex: both taps of every axis are vertex 0"),
    (1, 5, 7, 9, 130, "full", "one vertex along z"),
    (8, 1, 7, 9, 130, "full", "one vertex along y"),
    (8, 5, 1, 9, 130, "full", "one vertex along x"),
    (32, 3, 3, 9, 130, "wide", "the largest z axis; black, white and out-of-range pixels: the clamp and the last bin"),
    (8, 5, 7, 37, 53, "wide", "the clamp and the last bin on an ordinary grid"),
    (2, 256, 3, 300, 5, "full", "the largest y axis"),
    (2, 3, 256, 5, 300, "full", "the largest x axis"),
    (4, 2, 100, 8, 130, "full", "two tiles: one global (792 vertices), one LDS (24)"),
    (4, 20, 100, 17, 258, "full", "nine tiles: six global, three LDS"),
    (5, 8, 8, 8, 8, "full", "320 vertices: at the cap"),
    (10, 1, 32, 1, 128, "full", "320 vertices in one row of the grid: at the cap"),
    (3, 1, 107, 1, 128, "full", "321 vertices: one over the cap"),
    (10, 1, 33, 1, 128, "full", "330 vertices: over the cap"),
    (8, 5, 7, 1, 1000, "full", "one row, 8 tiles"),
    (8, 5, 7, 1000, 1, "full", "one column, 125 tiles, every access scalar"),
    (8, 5, 7, 3, 2, "full", "W < 4"),
    (8, 5, 7, 9, 130, "full", "W % 4 == 2"),
]
#: launches whose tiles take both paths, and launches of one tile at the cap or just over it: the default path is asserted from tile_footprints
MIXED = [(4, 2, 100, 8, 130, "full"), (4, 20, 100, 17, 258, "full")]
AT_CAP = [(5, 8, 8, 8, 8, "full"), (10, 1, 32, 1, 128, "full")]
OVER_CAP = [(3, 1, 107, 1, 128, "full"), (10, 1, 33, 1, 128, "full")]
BITWISE = [(8, 5, 7, 3, 2, "full"), (8, 5, 7, 9, 130, "full"), (8, 5, 7, 1, 1000, "full"), (8, 5, 7, 1000, 1, "full"), (4, 20, 100, 17, 258, "full")]
NONFINITE = (8, 5, 7, 9, 130, "full")


def slice_id(c):
    return "g%dx%dx%d-%dx%d-%s" % c[:6]


def random_grid(gz, gh, gw):
    """Seeded uniform in [-0.3, 0.7), rounded to fp32: neighbouring vertices are unrelated, so a vertex index off by one shows."""
    rng = np.random.default_rng(gz * 100003 + gh * 1009 + gw)
    return np.ascontiguousarray(rng.random((gz, gh, gw, 3, 4)) - 0.3, np.float32)


@functools.lru_cache(maxsize=None)
def slice_reference(gz, gh, gw, H, W, kind):
    """(the fp32 grid, the image, O.slice_ of the two in fp64)."""
    grid, c = random_grid(gz, gh, gw), slice_image(H, W, kind)
    return _frozen(grid, c, O.slice_(grid, c))


def tile_footprints(gz, gh, gw, H, W):
    """The vertices each TH x TW tile of an H x W image touches, tiles in row-major order: gz times the span of y vertices times the span
    of x vertices that any pixel of the tile has a tap on."""
    j0, j1, _ = O.axis(H, gh)
    i0, i1, _ = O.axis(W, gw)
    out = []
    for y in range(0, H, TH):
        nj = int(j1[y:y + TH].max() - j0[y:y + TH].min()) + 1
        for x in range(0, W, TW):
            out.append(gz * nj * (int(i1[x:x + TW].max() - i0[x:x + TW].min()) + 1))
    return out
