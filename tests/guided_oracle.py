"""The definitions of include/wct_hip_guided.h in numpy -- a test helper, not a fixture file.

Guided transfer: tests/region_oracle.py's level with the STYLE columns of region k restricted to the style's own level label map
    lab_s,L[i, j] = style_labels[i s + s//2, j s + s//2], s = 2^(L-1), over the style's (uncropped) level feature map;
a region keeps cF where it has fewer than 2 content pixels or fewer than 2 style pixels.

K-means: z = (x - fp32(sh)) * fp32(sc) formed in fp32 (two roundings, no fused step), everything after that in fp64:
    d_k = sum_c (z_c - fp32(m_kc))^2, label = arg-min (lowest k on ties), sums of z per label, cost = sum of min d.
"""
import numpy as np

from oracle import wct_oracle
from tests import region_oracle

CLEAR = 1e-4          # a pixel is clear when d2 - d1 >= CLEAR (d2 + |z|^2): 3 x the fp32 error of the direct form at C = 512
DEAD_VARIANCE = 1e-12


# ---------------------------------------------------------------------------------------------------------------- guided transfer
def region_transfer(mods, level, img, labels, styles, style_labels, region_style, alpha):
    """One level: region k of the content against the label-k pixels of style region_style[k] (its whole map when unmapped)."""
    fp64 = getattr(mods, "precision", "fp32") == "fp64"
    cF = mods.encode(level, img)
    C, h, w = cF.shape
    lab = region_oracle.level_labels(labels, level, h, w).reshape(-1)
    c = np.asarray(cF, np.float64).reshape(C, -1)
    out = c.copy()
    feats = {}
    for k, s in enumerate(region_style):
        sel = lab == k
        if int(sel.sum()) < 2:
            continue
        if s not in feats:
            feats[s] = np.asarray(mods.encode(level, styles[s]), np.float64)
        sF = feats[s]
        cols = sF.reshape(C, -1)
        if style_labels is not None and style_labels[s] is not None:
            slab = region_oracle.level_labels(style_labels[s], level, sF.shape[1], sF.shape[2]).reshape(-1)
            if int((slab == k).sum()) < 2:
                continue
            cols = cols[:, slab == k]
        cs = c if sel.all() else c[:, sel]
        target = wct_oracle.whiten_and_color(cs, cols)
        out[:, sel] = alpha[k] * target + (1.0 - alpha[k]) * cs
    csF = out.reshape(C, h, w).astype(np.float64 if fp64 else np.float32)
    return mods.decode(level, csF)


def stylize_guided(mods, content, styles, labels, style_labels=None, region_style=None, alpha=1.0, num_run=1, levels=(5, 4, 3, 2, 1)):
    rs = list(range(len(styles))) if region_style is None else [int(v) for v in region_style]
    K = len(rs)
    al = [float(alpha)] * K if np.isscalar(alpha) else [float(a) for a in alpha]
    fp64 = getattr(mods, "precision", "fp32") == "fp64"
    cast = (lambda x: np.asarray(x, np.float64)) if fp64 else (lambda x: np.ascontiguousarray(x, np.float32))
    img = cast(content)
    st = [cast(s) for s in styles]
    for _ in range(num_run):
        for L in levels:
            img = region_transfer(mods, L, img, labels, st, style_labels, rs, al)
    return img


# ---------------------------------------------------------------------------------------------------------------- k-means
def standardisation(n, s, ss_diag):
    """(sh, sc) fp64 from raw moments: the mean and 1 / sqrt(population variance), 0 for a channel at or under 1e-12 of the largest."""
    mu = np.asarray(s, np.float64) / n
    var = np.asarray(ss_diag, np.float64) / n - mu * mu
    sc = np.zeros_like(var)
    ok = var > DEAD_VARIANCE * var.max()
    sc[ok] = 1.0 / np.sqrt(var[ok])
    return mu, sc


def standardisation_of(feat):
    x = np.asarray(feat, np.float64).reshape(-1, feat.shape[-1])
    return standardisation(x.shape[0], x.sum(0), np.einsum("pc,pc->c", x, x))


def zmap(feat, sh, sc):
    """z in fp32 exactly as specified, [npix, C]."""
    x = np.ascontiguousarray(feat, np.float32).reshape(-1, feat.shape[-1])
    return (x - np.asarray(sh, np.float64).astype(np.float32)) * np.asarray(sc, np.float64).astype(np.float32)


BIG = 1 << 22     # elements of a map from which the fp64 distances are taken in the expanded form (one BLAS product)


def _sqdist(z64, m, zz=None):
    """fp64 |z - m_k|^2 [npix, K].  Small maps: the direct form, so exactly equal centroids give exactly equal distances.  Large maps:
    |z|^2 - 2 z.m + |m|^2 -- in fp64 its error is ~C 2^-53 (|z|^2 + |m|^2), nine orders under the margin CLEAR puts around a decision."""
    if z64.size < BIG:
        return np.stack([((z64 - m[k]) ** 2).sum(1) for k in range(m.shape[0])], 1)
    zz = np.einsum("pc,pc->p", z64, z64) if zz is None else zz
    return np.maximum(zz[:, None] - 2.0 * (z64 @ m.T) + (m * m).sum(1)[None, :], 0.0)


def distances(z, cent):
    """fp64 d[npix, K] of fp32 z against the centroids rounded to fp32."""
    m = np.asarray(cent, np.float64).astype(np.float32).astype(np.float64)
    return _sqdist(z.astype(np.float64), m)


def clear_pixels(d, z):
    """(clear mask, margin): d2 - d1 >= CLEAR (d2 + |z|^2) with d1 <= d2 the two smallest distances; K = 1: every pixel is clear."""
    z64 = z.astype(np.float64)
    zz = np.einsum("pc,pc->p", z64, z64)
    if d.shape[1] == 1:
        return np.ones(d.shape[0], bool), CLEAR * (d[:, 0] + zz)
    two = np.partition(d, 1, axis=1)[:, :2]
    margin = CLEAR * (two[:, 1] + zz)
    return two[:, 1] - two[:, 0] >= margin, margin


def assign(z, cent):
    """One Lloyd step: labels, n[K], sum[K, C], cost, next[K, C], d."""
    cent = np.asarray(cent, np.float64)
    d = distances(z, cent)
    lab = d.argmin(1)                                   # the first minimum: the lowest k on ties
    K = cent.shape[0]
    z64 = z.astype(np.float64)
    n = np.array([(lab == k).sum() for k in range(K)], np.float64)
    s = (lab[None, :] == np.arange(K)[:, None]).astype(np.float64) @ z64
    nxt = cent.copy()
    nxt[n > 0] = s[n > 0] / n[n > 0, None]
    return lab.astype(np.uint8), n, s, float(d.min(1).sum()), nxt, d


def seed(z, K):
    """Farthest-first: centroids [K, C] (fp64 of the chosen z), idx [K], and the relative margin of each arg-max decision over the best
    pixel with a DIFFERENT value (1.0 where there is none)."""
    z64 = z.astype(np.float64)
    zz = np.einsum("pc,pc->p", z64, z64)
    mind = zz.copy()
    idx, margins = [], []
    for j in range(K):
        i = int(mind.argmax())                          # the first maximum: the lowest index on ties
        other = mind[mind < mind[i]]
        margins.append(1.0 if other.size == 0 or mind[i] == 0 else float((mind[i] - other.max()) / mind[i]))
        idx.append(i)
        d = _sqdist(z64, z64[i:i + 1], zz)[:, 0]
        d[i] = 0.0
        mind = np.minimum(mind, d)
    return z64[idx].copy(), np.array(idx, np.int32), margins


def lloyd(z, K, iters):
    """seed + `iters` steps: (final centroids, idx, costs per step, unclear pixels per step, seed margins)."""
    cent, idx, margins = seed(z, K)
    costs, unclear = [], []
    for _ in range(iters):
        _, _, _, cost, nxt, d = assign(z, cent)
        costs.append(cost)
        unclear.append(int((~clear_pixels(d, z)[0]).sum()))
        cent = nxt
    return cent, idx, costs, unclear, margins


def expand(lab, level, H, W):
    """label(y, x) = lab[min(y // s, h - 1), min(x // s, w - 1)], s = 2^(level-1)."""
    s = 1 << (level - 1)
    h, w = lab.shape
    return lab[np.minimum(np.arange(H) // s, h - 1)][:, np.minimum(np.arange(W) // s, w - 1)]


def cluster_features(K, h, w, C, seed_):
    """The k-means fixture: relu(centre[label] + N(0, 1) + 0.9) with centres 3 N(0, 1), one channel exactly zero; NHWC fp32."""
    rng = np.random.default_rng(seed_)
    centre = 3 * rng.standard_normal((K, C))
    truth = rng.integers(0, K, size=(h, w))
    f = np.maximum(centre[truth] + rng.standard_normal((h, w, C)) + 0.9, 0).astype(np.float32)
    f[..., 1 if C > 1 else 0] = 0
    return np.ascontiguousarray(f)
