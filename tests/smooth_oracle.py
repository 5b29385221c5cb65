"""numpy fp64 reference of the guided-filter smoothing entries (include/wct_hip_smooth.h).  Test infrastructure: the product never
imports it.  Images are 3 x H x W arrays."""
import numpy as np

EPS = 1e-3          # WCT_SMOOTH_EPS


def box_sum_axis(x, r, axis):
    """Sums over [i - r, i + r] clipped to the array along `axis`, by one cumulative sum along that axis (fp64)."""
    x = np.moveaxis(np.asarray(x, np.float64), axis, -1)
    n = x.shape[-1]
    c = np.concatenate([np.zeros(x.shape[:-1] + (1,)), np.cumsum(x, -1)], -1)
    i = np.arange(n)
    hi, lo = np.minimum(i + r, n - 1) + 1, np.maximum(i - r, 0)
    return np.moveaxis(c[..., hi] - c[..., lo], -1, axis)


def box_count(H, W, r):
    """Number of in-image pixels of every clipped window: H x W."""
    y, x = np.arange(H), np.arange(W)
    ny = np.minimum(y + r, H - 1) - np.maximum(y - r, 0) + 1
    nx = np.minimum(x + r, W - 1) - np.maximum(x - r, 0) + 1
    return np.outer(ny, nx).astype(np.float64)


def box_mean(x, r):
    """Windowed mean over [y - r, y + r] x [x - r, x + r] clipped to the image, of the last two axes of x: the box filter of He et
    al.'s reference implementation (no padding: every mean divides by its window's pixel count)."""
    x = np.asarray(x, np.float64)
    s = box_sum_axis(box_sum_axis(x, r, x.ndim - 2), r, x.ndim - 1)
    return s / box_count(x.shape[-2], x.shape[-1], r)


def box_mean_brute(x, r):
    """The same by a double loop over the pixels of a 2-D array."""
    x = np.asarray(x, np.float64)
    H, W = x.shape
    out = np.empty_like(x)
    for y in range(H):
        for c in range(W):
            out[y, c] = x[max(0, y - r): y + r + 1, max(0, c - r): c + r + 1].mean()
    return out


def coefficients(src, guide, r, eps):
    """a [3(i), 3(c), H, W] and b [3(c), H, W] of the colour-guide filter, fp64; the guide's top-left window of the source's size."""
    p = np.asarray(src, np.float64)
    I = np.asarray(guide, np.float64)[:, :p.shape[1], :p.shape[2]]
    mean_I, mean_p = box_mean(I, r), box_mean(p, r)
    corr_II = box_mean(I[:, None] * I[None, :], r)                 # [i, j, H, W]
    corr_Ip = box_mean(I[:, None] * p[None, :], r)                 # [i, c, H, W]
    Sigma = corr_II - mean_I[:, None] * mean_I[None, :] + eps * np.eye(3)[:, :, None, None]
    cov_Ip = corr_Ip - mean_I[:, None] * mean_p[None, :]
    a = np.linalg.solve(Sigma.transpose(2, 3, 0, 1), cov_Ip.transpose(2, 3, 0, 1)).transpose(2, 3, 0, 1)
    b = mean_p - np.einsum("ichw,ihw->chw", a, mean_I)
    return a, b


def guided_filter(src, guide, r, eps=EPS, ab_fp32=False):
    """q_c = SUM_i mean_a[i][c] I_i + mean_b[c], fp64, not clamped.  ab_fp32: a and b rounded to fp32 between the two stages, which
    is what the library stores."""
    p = np.asarray(src, np.float64)
    I = np.asarray(guide, np.float64)[:, :p.shape[1], :p.shape[2]]
    a, b = coefficients(p, I, r, eps)
    if ab_fp32:
        a, b = a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
    return np.einsum("ichw,ihw->chw", box_mean(a, r), I) + box_mean(b, r)
