"""numpy fp64 reference of the resampler R and the merge M of include/wct_hip_scale.h: the weights of the header's rule in fp64 (no
fixed-point step, NOT rounded to fp32), both passes in fp64 with nothing rounded in between.  Also what the tests' bounds are made of
(the largest tap count and the largest SUM |w| of an axis, from these same tables) and the shapes the device tests share."""
import numpy as np

BILINEAR, BICUBIC = "bilinear", "bicubic"
FILTER_SUPPORT = {BILINEAR: 1.0, BICUBIC: 2.0}
U = 2.0 ** -24                       # unit round-off of fp32
TILE_W, TILE_H = 64, 16              # scale.hip SC_TILE_W x SC_TILE_H: the output tile of a workgroup (tests/test_scale_cpu.py pins the two)
TILE_W_NARROW = 32                   # ... SC_TILE_W_NARROW: columns per tile when the width shrinks by more than 8

# (H, W) -> (oH, oW): the shapes of the issue, then output sizes one below, at and one above the tile's dimensions (and the narrow tile's
# width, which a width shrinking by more than 8 takes), reached by enlarging, by reducing and by a mixed pair of ratios
RESAMPLE_SHAPES = [
    ((131, 257), (16, 32)), ((16, 32), (131, 257)), ((208, 280), (208, 272)), ((208, 280), (48, 64)), ((5, 7), (1, 1)), ((1, 3), (4, 9)),
    ((9, 40), (TILE_H - 1, TILE_W - 1)), ((40, 150), (TILE_H, TILE_W)), ((9, 150), (TILE_H + 1, TILE_W + 1)),
    ((23, 300), (2 * TILE_H + 1, TILE_W_NARROW - 1)), ((40, 310), (TILE_H - 1, TILE_W_NARROW + 1)),
    ((300, 40), (31, 20)),           # a height shrinking by 9.7: the tile's height halves so that its window of rows fits
]
MERGE_SHAPES = [((48, 64), (96, 128)), ((96, 128), (208, 272))]


def kernel(x, name):
    """Pillow's bilinear_filter / bicubic_filter (a = -0.5) on an array."""
    x = np.abs(np.asarray(x, np.float64))
    if name == BILINEAR:
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0, np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * a, 0.0))


def axis_rows(n_in, n_out, name):
    """[(first tap, fp64 weights)] per output sample: the rule of the header, operation for operation."""
    scale = float(n_in) / float(n_out)
    fs = max(scale, 1.0)
    support = FILTER_SUPPORT[name] * fs
    rows = []
    for i in range(n_out):
        centre = (i + 0.5) * scale
        lo = max(int(centre - support + 0.5), 0)
        hi = min(int(centre + support + 0.5), n_in)
        v = kernel((np.arange(lo, hi, dtype=np.float64) - centre + 0.5) / fs, name)
        ww = 0.0
        for t in v:                       # ascending, like the kernel
            ww += float(t)
        rows.append((lo, v / ww if ww != 0.0 else v))
    return rows


def axis_matrix(n_in, n_out, name):
    m = np.zeros((n_out, n_in), np.float64)
    for i, (lo, w) in enumerate(axis_rows(n_in, n_out, name)):
        m[i, lo:lo + len(w)] = w
    return m


def axis_stats(n_in, n_out, name):
    """(n, A): the largest tap count and the largest SUM |w| of the axis."""
    rows = axis_rows(n_in, n_out, name)
    return max(len(w) for _, w in rows), max(float(np.abs(w).sum()) for _, w in rows)


def resample(x, oh, ow, name):
    """R(x -> oh x ow) of a [3, h, w] array in fp64: horizontal pass, then vertical."""
    x = np.asarray(x, np.float64)
    return np.einsum("yr,crx->cyx", axis_matrix(x.shape[1], oh, name), x @ axis_matrix(x.shape[2], ow, name).T)


def merge(a, b, c, g):
    """M(a, b, c, g) = R(a - g b -> c's size, bicubic) + g c in fp64."""
    a, b, c = (np.asarray(t, np.float64) for t in (a, b, c))
    return resample(a - g * b, c.shape[1], c.shape[2], BICUBIC) + g * c


def resample_bound(shape, oh, ow, name, peak, extra=4):
    """(n_h + n_v + extra) u A_h A_v max|x|: the first-order bound of two recursive fp32 sums with fp32-rounded weights."""
    nv, av = axis_stats(shape[0], oh, name)
    nh, ah = axis_stats(shape[1], ow, name)
    return (nh + nv + extra) * U * ah * av * peak


def merge_bound(shape, oh, ow, g, peak_a, peak_b, peak_c):
    return resample_bound(shape, oh, ow, BICUBIC, peak_a + g * peak_b, extra=6) + 2 * U * g * peak_c


def resample_f32(x, oh, ow, name):
    """The device's arithmetic in numpy: fp32-rounded weights, fp32 sums in ascending tap order (multiply and add rounded separately --
    the device's fma rounds once, which is no further from the exact sum), horizontal pass first, fp32 in between."""
    x = np.asarray(x, np.float32)

    def one_pass(src, rows):                # along the last axis
        out = np.zeros(src.shape[:-1] + (len(rows),), np.float32)
        for i, (lo, w) in enumerate(rows):
            acc = np.zeros(src.shape[:-1], np.float32)
            for t, wt in enumerate(w.astype(np.float32)):
                acc = acc + wt * src[..., lo + t]
            out[..., i] = acc
        return out

    t = one_pass(x, axis_rows(x.shape[2], ow, name))
    return one_pass(t.transpose(0, 2, 1), axis_rows(x.shape[1], oh, name)).transpose(0, 2, 1)


def image(shape, seed):
    """[3, h, w] fp32 in [-0.5, 1.5]."""
    return (np.random.default_rng(seed).random((3,) + tuple(shape)) * 2.0 - 0.5).astype(np.float32)
