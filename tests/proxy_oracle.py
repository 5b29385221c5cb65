"""numpy fp64 reference of proxy mode's bilateral grid (include/wct_hip_bgrid.h), straight from the definition: the tent weights, the
fit of a grid of 3 x 4 affine colour maps from a reduced (content, result) pair, and the slice that applies it to a full image.
Nothing here is shared with the product; every image is 3 x h x w."""
import numpy as np

LUMA = np.array([0.299, 0.587, 0.114])
CELL, BINS, EPS, SMOOTH = 16, 8, 1e-2, 1      # WCT_BGRID_CELL, _BINS, _EPS, _SMOOTH
MAX_XY, MAX_Z = 256, 32


def shape(h, w, cell=CELL):
    """(gh, gw) = (ceil(h / cell) + 1, ceil(w / cell) + 1)."""
    return -(-h // cell) + 1, -(-w // cell) + 1


def guide(img):
    x = np.asarray(img, np.float64)
    return np.clip(LUMA[0] * x[0] + LUMA[1] * x[1] + LUMA[2] * x[2], 0.0, 1.0)


def tent(u, G):
    """(i0, i1, f): weight 1 - f on vertex i0 and f on vertex i1 = min(i0 + 1, G - 1)."""
    u = np.asarray(u, np.float64)
    i0 = np.minimum(np.floor(u).astype(np.int64), max(G - 2, 0))
    return i0, np.minimum(i0 + 1, G - 1), u - i0


def axis(n, G):
    """The tent of every sample x of an axis with n samples and G vertices: u = (x + 0.5) / n * (G - 1)."""
    return tent((np.arange(n) + 0.5) / n * (G - 1), G)


def weights(img, gz, gh, gw):
    """Per pixel the 8 (vertex index, weight) pairs: lists of flat indices [h, w] into a gz x gh x gw grid, and weights [h, w]."""
    x = np.asarray(img, np.float64)
    h, w = x.shape[1:]
    k0, k1, fz = tent(guide(x) * (gz - 1), gz)
    j0, j1, fy = axis(h, gh)
    i0, i1, fx = axis(w, gw)
    out = []
    for k, wz in ((k0, 1.0 - fz), (k1, fz)):
        for j, wy in ((j0, 1.0 - fy), (j1, fy)):
            for i, wx in ((i0, 1.0 - fx), (i1, fx)):
                out.append(((k * gh + j[:, None]) * gw + i[None, :], wz * wy[:, None] * wx[None, :]))
    return out


def blur(S, times):
    """`times` x ([1 2 1] / 4 along z, then y, then x), the edge vertex repeated; S is [gz, gh, gw, ...]."""
    for _ in range(times):
        for ax in range(3):
            n = S.shape[ax]
            idx = np.arange(n)
            lo, hi = np.take(S, np.maximum(idx - 1, 0), ax), np.take(S, np.minimum(idx + 1, n - 1), ax)
            S = 0.25 * ((lo + hi) + 2.0 * S)
    return S


def sums(cl, sl, gz, gh, gw):
    """Per vertex Gv [gz, gh, gw, 4, 4] and Rv [gz, gh, gw, 4, 3] before any blur."""
    c, s = np.asarray(cl, np.float64), np.asarray(sl, np.float64)
    h, w = c.shape[1:]
    v = np.concatenate([c, np.ones((1, h, w))]).reshape(4, -1).T            # [p, 4]
    vv = v[:, :, None] * v[:, None, :]
    vs = v[:, :, None] * s.reshape(3, -1).T[:, None, :]
    Gv, Rv = np.zeros((gz * gh * gw, 4, 4)), np.zeros((gz * gh * gw, 4, 3))
    for idx, wt in weights(c, gz, gh, gw):
        np.add.at(Gv, idx.reshape(-1), wt.reshape(-1, 1, 1) * vv)
        np.add.at(Rv, idx.reshape(-1), wt.reshape(-1, 1, 1) * vs)
    return Gv.reshape(gz, gh, gw, 4, 4), Rv.reshape(gz, gh, gw, 4, 3)


def fit(cl, sl, gz, gh, gw, eps=EPS, smooth=SMOOTH, details=False):
    """The grid A [gz, gh, gw, 3, 4] in fp64 (the product rounds it once to fp32).  details: also (Ag [3, 4], the largest condition
    number of Gv + lambda I, lambda)."""
    h, w = np.asarray(cl).shape[1:]
    Gv, Rv = sums(cl, sl, gz, gh, gw)
    Gv, Rv = blur(Gv, smooth), blur(Rv, smooth)
    lam = eps * h * w / (gz * gh * gw)
    I = np.eye(4)
    Ag = np.linalg.solve(Gv.sum((0, 1, 2)) + lam * I, Rv.sum((0, 1, 2)))                 # [4, 3]
    A = np.linalg.solve(Gv + lam * I, Rv + lam * Ag)                                     # [gz, gh, gw, 4, 3]
    A = np.ascontiguousarray(np.swapaxes(A, -1, -2))
    if details:
        return A, Ag.T.copy(), float(np.linalg.cond(Gv + lam * I).max()), lam
    return A


def slice_(grid, content):
    """The grid [gz, gh, gw, 3, 4] applied to the full image [3, H, W]: fp64, not rounded, not clamped."""
    A = np.asarray(grid, np.float64)
    gz, gh, gw = A.shape[:3]
    c = np.asarray(content, np.float64)
    H, W = c.shape[1:]
    flat = A.reshape(-1, 12)
    coef = np.zeros((H, W, 12))
    for idx, wt in weights(c, gz, gh, gw):
        coef += wt[:, :, None] * flat[idx]
    coef = coef.reshape(H, W, 3, 4)
    v = np.concatenate([c, np.ones((1, H, W))]).transpose(1, 2, 0)                       # [H, W, 4]
    return np.einsum("hwca,hwa->chw", coef, v)
