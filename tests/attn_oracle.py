"""Numpy reference of the attention-weighted style statistics (include/wct_hip_attn.h): an fp64 arm (the yardstick), a plain-fp32 arm of the
same formulas (what "fp32-class" means for a result: the gates of tests/test_attn_gpu.py are multiples of ITS error), and the fp32
emulation of wct_attn_apply's stated evaluation order (bit for bit).  No Nq x Nk matrix is avoided here: the test shapes are small."""
import numpy as np

from tests import swap_oracle as SO

EPS = 1e-12            # WCT_ATTN_EPS
ADAIN_EPS = 1e-5       # WCT_ADAIN_EPS
MAX_TEMP = 32          # WCT_ATTN_MAX_TEMP
STANDARD, WHITENED = 0, 1


def relu_map(seed, h, w, C):
    """A ReLU-like feature map: correlated channels, about half of the entries zero, fp32."""
    rng = np.random.default_rng(seed)
    mix = np.eye(C) + rng.standard_normal((C, C)) * (0.5 / np.sqrt(C))
    x = rng.standard_normal((h, w, C)) @ mix + 0.1 * rng.standard_normal(C)
    return np.maximum(x, 0).astype(np.float32)


def moments(X, dtype=np.float64):
    """(mu, sigma) per channel of X [..., C]: unbiased variance, sigma = sqrt(v + ADAIN_EPS)."""
    X = np.asarray(X, dtype).reshape(-1, X.shape[-1])
    n = X.shape[0]
    mu = X.sum(0) / dtype(n)
    v = np.maximum(((X * X).sum(0) - dtype(n) * mu * mu) / dtype(n - 1), 0)
    return mu, np.sqrt(v + dtype(ADAIN_EPS))


def standardise(X, dtype=np.float64):
    mu, sigma = moments(X, dtype)
    return ((np.asarray(X, dtype) - mu) / sigma).astype(dtype)


def unit(Q, dtype=np.float64):
    Q = np.asarray(Q, dtype)
    return (Q / np.sqrt((Q * Q).sum(-1, keepdims=True) + dtype(EPS))).astype(dtype)


def project(X, domain, dtype=np.float64):
    """(unit rows of the projected map, standardised map) of X [h, w, C]."""
    std = standardise(X, dtype)
    proj = std if domain == STANDARD else SO.whiten(X).astype(dtype)
    return unit(proj, dtype), std


def weights(qhat, khat, tau, dtype=np.float64):
    q, k = np.asarray(qhat, dtype).reshape(-1, qhat.shape[-1]), np.asarray(khat, dtype).reshape(-1, khat.shape[-1])
    s = dtype(tau) * (q @ k.T)
    p = np.exp(s - s.max(1, keepdims=True))
    return (p / p.sum(1, keepdims=True)).astype(dtype)


def stats(qhat, khat, V, tau, dtype=np.float64):
    """(mean, var) [Nq, C]."""
    A = weights(qhat, khat, tau, dtype)
    V = np.asarray(V, dtype).reshape(-1, V.shape[-1])
    m = A @ V
    e = A @ (V * V)
    return m, np.maximum(e - m * m, 0)


def apply(mean, var, c_std, cF, mu_s, sigma_s, alpha, dtype=np.float64):
    d = lambda a: np.asarray(a, dtype)
    return dtype(alpha) * (d(sigma_s) * (np.sqrt(d(var)) * d(c_std) + d(mean)) + d(mu_s)) + (dtype(1) - dtype(alpha)) * d(cF)


def apply_f32_emulation(mean, var, c_std, cF, mu_s, sigma_s, alpha):
    """The header's order, every operation rounded to fp32 once; mu_s, sigma_s fp64 [C], rounded to fp32 first."""
    f = np.float32
    m, v, z, x = (np.asarray(a, f) for a in (mean, var, c_std, cF))
    sg, mu = np.asarray(sigma_s, np.float64).astype(f), np.asarray(mu_s, np.float64).astype(f)
    a = f(alpha)
    oma = f(f(1) - a)
    y = ((sg * ((np.sqrt(v) * z).astype(f) + m).astype(f)).astype(f) + mu).astype(f)
    return ((a * y).astype(f) + (oma * x).astype(f)).astype(f)


def level_feature(cF, sF, domain, tau, alpha, dtype=np.float64):
    """cF [h, w, C], sF [hs, ws, C] -> (csF [h, w, C], mean, var)."""
    qhat, cstd = project(cF, domain, dtype)
    khat, sstd = project(sF, domain, dtype)
    mu_s, sigma_s = moments(sF, dtype)
    m, v = stats(qhat, khat, sstd, tau, dtype)
    C = cF.shape[-1]
    out = apply(m, v, cstd.reshape(-1, C), np.asarray(cF, dtype).reshape(-1, C), mu_s, sigma_s, alpha, dtype)
    return out.reshape(cF.shape), m, v


def live_channels(sF):
    X = np.asarray(sF, np.float64).reshape(-1, sF.shape[-1])
    return X.var(0) > 0
