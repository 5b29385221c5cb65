"""numpy fp64 reference of the colour preservation entries (include/wct_hip_color.h).  Test infrastructure: the product never
imports it.  Images are 3 x H x W arrays."""
import numpy as np

EPS = 1e-5          # WCT_COLOR_EPS
LUMA = np.array([0.299, 0.587, 0.114])


def natural(seed, H, W, cast=(1.0, 0.8, 0.6), shift=(0.05, 0.1, 0.2)):
    """A test image: smoothed noise with correlated channels and a colour cast, values in [0, 1]."""
    rng = np.random.default_rng(seed)
    x = rng.random((3, H, W))
    for _ in range(3):
        x = (x + np.roll(x, 1, 1) + np.roll(x, -1, 1) + np.roll(x, 1, 2) + np.roll(x, -1, 2)) / 5
    x = 0.6 * x + 0.4 * x.mean(0, keepdims=True)
    x = (x - x.min()) / (x.max() - x.min())
    return np.clip(x * np.array(cast)[:, None, None] * 0.8 + np.array(shift)[:, None, None], 0, 1).astype(np.float32)


def moments(img):
    """(n, sum[3], sumsq[3, 3]): raw fp64 sums over all pixels."""
    x = np.asarray(img, np.float64).reshape(3, -1)
    # numpy's pairwise summation (error ~ log n ulps) for the products too: a BLAS dot product of 8 million terms promises less
    ss = np.array([[(x[i] * x[j]).sum() for j in range(3)] for i in range(3)])
    return float(x.shape[1]), x.sum(1), ss


def cov(n, s, ss, eps=EPS):
    """mu and the unbiased covariance + eps I from raw sums."""
    s, ss = np.asarray(s, np.float64).reshape(3), np.asarray(ss, np.float64).reshape(3, 3)
    mu = s / n
    return mu, (ss - n * np.outer(mu, mu)) / (n - 1.0) + eps * np.eye(3)


def sym_power(S, p):
    lam, V = np.linalg.eigh((S + S.T) / 2)
    return (V * lam ** p) @ V.T


def solve(n_c, sum_c, sumsq_c, n_s, sum_s, sumsq_s, eps=EPS):
    """A = cov_c^(1/2) cov_s^(-1/2), t = mu_c - A mu_s."""
    mu_c, Sc = cov(n_c, sum_c, sumsq_c, eps)
    mu_s, Ss = cov(n_s, sum_s, sumsq_s, eps)
    A = sym_power(Sc, 0.5) @ sym_power(Ss, -0.5)
    return A, mu_c - A @ mu_s


def apply(img, A, t):
    """A x + t per pixel in fp64 (not rounded to fp32, not clamped)."""
    x = np.asarray(img, np.float64)
    return (A @ x.reshape(3, -1) + np.asarray(t, np.float64).reshape(3, 1)).reshape(x.shape)


def match(style, content, eps=EPS):
    """The style with its colours mapped onto the content's colour distribution, fp64."""
    A, t = solve(*moments(content), *moments(style), eps)
    return apply(style, A, t)


def luma(img):
    return np.tensordot(LUMA, np.asarray(img, np.float64), 1)


def luma_merge(stylised, content):
    """content_c + (Y(stylised) - Y(content)) over the content's top-left window of the stylised size, fp64."""
    s = np.asarray(stylised, np.float64)
    c = np.asarray(content, np.float64)[:, :s.shape[1], :s.shape[2]]
    return c + (luma(s) - luma(c))[None]


def to_u8(planar, round_mode=0):
    """save_image's conversion as the existing tests do it (tests/test_cli.py): fp32 mul(255), + 0.5 with round_mode 1, clamp,
    truncation; 3 x H x W fp32 -> H x W x 3 uint8."""
    x = np.asarray(planar, np.float32) * np.float32(255)
    if round_mode:
        x = x + np.float32(0.5)
    return np.ascontiguousarray(np.clip(x, 0, 255).astype(np.uint8).transpose(1, 2, 0))
