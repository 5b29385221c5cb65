"""numpy fp64 reference of the patch swap of include/wct_hip_swap.h, in its brute-force form: unfold + matmul + arg-max with the lowest
index.  Test infrastructure: the product never imports it.

    patches(x)            [h, w, C] -> [(h-2)(w-2), 9C], patch q = qy (w-2) + qx, elements in (dy, dx, c) order
    scores(Q, K)          S[q, k] = <patch_Q(q), patch_K(k)> / sqrt(|patch_K(k)|^2 + EPS)
    match(Q, K)           Match(idx, best, gap, qnorm, S): arg-max (lowest index among equal scores), its score, the distance to the best
                          score of any OTHER key, |patch_Q|
    assemble(...)         alpha * (mean of the covering value patches) + (1 - alpha) * base; dtype=np.float32 is the library's own
                          arithmetic (fp32 sums from 0 in ascending (qy, qx) order, one division, an uncontracted blend) bit for bit
    whiten(x)             cov^(-1/2) (x - mu) with the unbiased covariance and the pseudo-inverse square root
    decorate(cF, sF, ..)  the one-level decorator: (idx, csF, Q, K)"""
import collections

import numpy as np

from tests import transform_oracle as TO

EPS = 1e-12           # WCT_SWAP_EPS

Match = collections.namedtuple("Match", "idx best gap qnorm S")


def patches(x):
    x = np.asarray(x)
    h, w, C = x.shape
    assert h >= 3 and w >= 3
    return np.stack([x[dy:dy + h - 2, dx:dx + w - 2] for dy in range(3) for dx in range(3)], axis=2).reshape((h - 2) * (w - 2), 9 * C)


def scores(Q, K):
    pq, pk = patches(np.asarray(Q, np.float64)), patches(np.asarray(K, np.float64))
    return pq @ (pk / np.sqrt((pk * pk).sum(1) + EPS)[:, None]).T


def match(Q, K):
    S = scores(Q, K)
    idx = S.argmax(1)                       # numpy returns the first (lowest) index of the maximum
    best = S[np.arange(len(idx)), idx]
    if S.shape[1] > 1:
        rest = S.copy()
        rest[np.arange(len(idx)), idx] = -np.inf
        gap = best - rest.max(1)
    else:
        gap = np.full(len(idx), np.inf)
    qnorm = np.sqrt((patches(np.asarray(Q, np.float64)) ** 2).sum(1))
    return Match(idx, best, gap, qnorm, S)


def tau(C):
    """The gate of the f16x3 match relative to |patch_Q| (scores are key-normalised): twice the worst-case bound of the dropped lo.lo
    term (2^-22) plus fp32 accumulation over K = 9C terms (K 2^-24), by Cauchy-Schwarz."""
    return 2.0 ** -21 + 9 * C * 2.0 ** -23


def lowest_duplicate(K):
    """rep[k] = the lowest index of a key patch with exactly the values of patch k."""
    pk = patches(np.asarray(K))
    _, first, inv = np.unique(pk, axis=0, return_index=True, return_inverse=True)
    # np.unique's return_index is the first occurrence in the ORIGINAL order
    return first[np.asarray(inv).reshape(-1)]


def assemble(idx, h, w, V, base=None, alpha=1.0, dtype=np.float64):
    V = np.asarray(V, dtype)
    hs, ws, C = V.shape
    kw = ws - 2
    idx = np.asarray(idx).reshape(h - 2, w - 2)
    ky, kx = idx // kw, idx % kw
    acc = np.zeros((h, w, C), dtype)
    cnt = np.zeros((h, w), dtype)
    # pixel (y, x) is covered by the queries (y - oy, x - ox), oy, ox in 0..2: ascending (qy, qx) = descending (oy, ox)
    for oy in (2, 1, 0):
        for ox in (2, 1, 0):
            acc[oy:oy + h - 2, ox:ox + w - 2] = acc[oy:oy + h - 2, ox:ox + w - 2] + V[ky + oy, kx + ox]
            cnt[oy:oy + h - 2, ox:ox + w - 2] += 1
    # NOTE: for one pixel the (oy, ox) loop above visits its queries in ascending (qy, qx) order, each sum rounded in `dtype`
    mean = acc / cnt[:, :, None]
    a = dtype(alpha)
    if base is None:
        assert alpha == 1.0
        return a * mean
    return a * mean + (dtype(1) - a) * np.asarray(base, dtype)


def whiten(x):
    x = np.asarray(x, np.float64)
    h, w, C = x.shape
    X = x.reshape(-1, C)
    n = X.shape[0]
    mu, cov = TO.mean_cov(n, X.sum(0), X.T @ X)
    W = TO.sym_pow(cov, -0.5)
    return ((X - mu) @ W.T).reshape(h, w, C)


def decorate(cF, sF, mode="whitened", alpha=1.0):
    """cF [h, w, C], sF [hs, ws, C] -> (Match, csF, Q, K) in fp64."""
    cF, sF = np.asarray(cF, np.float64), np.asarray(sF, np.float64)
    Q, K = (whiten(cF), whiten(sF)) if mode == "whitened" else (cF, sF)
    m = match(Q, K)
    return m, assemble(m.idx, cF.shape[0], cF.shape[1], sF, cF, alpha), Q, K
