"""numpy fp64 reference of video mode (include/wct_hip_video.h): the tracking step (bit-exact by construction), its scene-cut decision,
the temporal blend, and the first-order bound of the blend's fp32 evaluation."""
import numpy as np

DBL_MIN = np.finfo(np.float64).tiny
U = 2.0 ** -24                       # fp32 unit roundoff
TILE_W, TILE_H = 64, 16              # video.hip TB_W, TB_H (tests/test_video_cpu.py holds them against the source)
MAX_RADIUS = 8


def track(r, c, rate, cut):
    """r' of one array of raw sums: c on a cut or with rate == 1, else r + rate (c - r) as three separately rounded fp64 operations --
    numpy rounds every elementwise operation on its own, so this is the device's result bit for bit."""
    r, c = np.asarray(r, np.float64), np.asarray(c, np.float64)
    if cut or rate == 1.0:
        return c.copy()
    d = c - r
    m = np.float64(rate) * d
    return r + m


def decision(n, sum_c, rs, rss, frames, cut_threshold):
    """(cut, D): D = SUM_k (mu_c - mu_r)^2 / max(SUM_k var_r, DBL_MIN); cut = frames == 0 or not (D <= threshold) -- NaN is a cut."""
    sum_c, rs, rss = (np.asarray(a, np.float64) for a in (sum_c, rs, rss))
    C = sum_c.shape[0]
    with np.errstate(all="ignore"):
        mu_c, mu_r = sum_c / n, rs / n
        var_r = np.diagonal(rss.reshape(C, C)) / n - mu_r * mu_r
        a, v = float(np.sum((mu_c - mu_r) ** 2)), float(np.sum(var_r))
        D = a / (v if v > DBL_MIN else DBL_MIN)          # fmax(v, DBL_MIN): a NaN v gives DBL_MIN
    return bool(frames == 0 or not (D <= cut_threshold)), D


def window_mean(e, radius):
    """Mean of e over the (2 radius + 1)^2 window clipped to the image, divided by the clipped pixel count."""
    H, W = e.shape
    ii = np.zeros((H + 1, W + 1), np.float64)
    ii[1:, 1:] = e.cumsum(0).cumsum(1)               # fp64 integral image: exact enough to serve as the reference of an fp32 sum
    y0, y1 = np.maximum(np.arange(H) - radius, 0), np.minimum(np.arange(H) + radius, H - 1) + 1
    x0, x1 = np.maximum(np.arange(W) - radius, 0), np.minimum(np.arange(W) + radius, W - 1) + 1
    s = ii[y1][:, x1] - ii[y0][:, x1] - ii[y1][:, x0] + ii[y0][:, x0]
    return s / ((y1 - y0)[:, None] * (x1 - x0)[None, :])


def blend(cur, prev, s, p, blend_w, sigma, radius, cut=False):
    """out = s + w (p - s), w = blend exp(-d / (2 sigma^2)); cur may be larger than the other three: its top-left window is used.
    sigma is taken as the fp32 value the device receives."""
    s, p = np.asarray(s, np.float64), np.asarray(p, np.float64)
    if cut:
        return s.copy()
    _, Ho, Wo = s.shape
    c, q = np.asarray(cur, np.float64)[:, :Ho, :Wo], np.asarray(prev, np.float64)
    e = ((c - q) ** 2).sum(0)
    d = window_mean(e, radius)
    sg = float(np.float32(sigma))
    w = float(np.float32(blend_w)) * np.exp(-d / (2.0 * sg * sg))
    return s + w[None] * (p - s)


def blend_bound(radius, blend_w, p, s):
    """2 u ((0.368 (n_win + 5) + 3) blend max|p - s| + 4 max(|s|, |p|)), n_win = (2 radius + 1)^2: the relative error of an n_win-term
    fp32 sum of non-negative terms (and the few roundings of e, the division and the exponent's argument: the + 5) enters w through
    x e^-x <= 0.368; a 1-2 ulp expf and blend's product (the + 3); three roundings of the combine on values no larger than
    max(|s|, |p|); a factor 2 of slack for the compiler's fma choices."""
    p, s = np.asarray(p, np.float64), np.asarray(s, np.float64)
    n_win = (2 * radius + 1) ** 2
    return 2 * U * ((0.368 * (n_win + 5) + 3) * blend_w * float(np.abs(p - s).max()) + 4 * max(float(np.abs(s).max()), float(np.abs(p).max())))


def clip_bytes(H, W, C):
    """wct_clip_bytes: two blocks of sums, the flags, three images, each part rounded up to 256 bytes."""
    up = lambda b: (b + 255) // 256 * 256
    sums = up(8 * sum(c + c * c for c in C))
    return 2 * sums + 256 + 3 * up(12 * (H // 16 * 16) * (W // 16 * 16))


def image(shape, seed):
    """A smooth planar 3 x H x W fp32 image in [0, 1]."""
    rng = np.random.default_rng(seed)
    x = rng.random((3,) + tuple(shape), dtype=np.float32)
    for _ in range(2):
        x = (x + np.roll(x, 1, 1) + np.roll(x, 1, 2)) / 3
    return np.ascontiguousarray(x, np.float32)
