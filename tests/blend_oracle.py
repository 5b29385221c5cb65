"""The definition of style interpolation (wct_stylize_interp) and per-pixel style weights (wct_stylize_blend) in numpy -- a test helper,
not a fixture file.

Tier 1, uniform weights: l = lambda / sum(lambda); per level L = 5..1 (and run), from the level's current image:
  cF = e_L(img)
  csF = alpha sum_k l_k whiten_and_color(cF, e_L(style_k)) + (1 - alpha) cF
  img <- d_L(csF)

Tier 2, weight maps w[K][H][W] (each in [0, 1], sum_k <= 1), alpha[K]; per level L with s = 2^(L-1):
  w_k,L[i, j] = mean of w[k] over [i s, (i+1) s) x [j s, (j+1) s)       (an area average)
  V1 = sum_p w_k,L(p),  V2 = sum_p w_k,L(p)^2
  mu_k = sum w x / V1,  cov_k = sum w (x - mu_k)(x - mu_k)^T / (V1 - V2 / V1)   (unbiased, reliability weights)
  k active iff V1 > 0 and V1^2 / V2 >= 2
  target_k(x) = S_k W_k (x - mu_k) + mu_s,k     (W_k from cov_k, S_k from the whole style image; the reference's svd + 1e-100 steps)
  csF(p) = x_p + sum_{k active} w_k,L(p) alpha_k (target_k(x_p) - x_p);  img <- d_L(csF)
"""
import numpy as np

from oracle import wct_oracle


def _cast(mods):
    if getattr(mods, "precision", "fp32") == "fp64":
        return lambda x: np.asarray(x, np.float64)
    return lambda x: np.ascontiguousarray(x, np.float32)


def normalised(lam):
    lam = np.asarray(lam, np.float64)
    return lam / lam.sum()


def svd_power(cov: np.ndarray, p: float) -> np.ndarray:
    """V diag(e^p) V^T of a covariance with the reference's steps (util_wct.py:74-86, 117-125): torch.svd, keep the eigenvalues before
    the first one below 1e-100."""
    _, e, vh = np.linalg.svd(cov, full_matrices=True)
    v = vh.T
    k = cov.shape[0]
    for i in range(cov.shape[0]):
        if e[i] < wct_oracle.EigenValueThre:
            k = i
            break
    return (v[:, :k] @ np.diag(e[:k] ** p)) @ v[:, :k].T


def whiten_and_color_moments(x: np.ndarray, mu_c, cov_c, mu_s, cov_s) -> np.ndarray:
    """whiten_and_color with the content's and the style's (mu, cov) given instead of computed from feature columns: x [C, n] fp64."""
    whiten = svd_power(cov_c, -0.5) @ (x - np.asarray(mu_c)[:, None])
    return svd_power(cov_s, 0.5) @ whiten + np.asarray(mu_s)[:, None]


# ---------------------------------------------------------------------------------------------------- tier 1
def interp_transfer(mods, level: int, img: np.ndarray, styles, lam, alpha: float) -> np.ndarray:
    """One level of the interpolation cascade: the per-style sum of the reference's transforms."""
    fp64 = getattr(mods, "precision", "fp32") == "fp64"
    lh = normalised(lam)
    cF = mods.encode(level, img)
    C = cF.shape[0]
    c = np.asarray(cF, np.float64).reshape(C, -1)
    acc = np.zeros_like(c)
    for k, st in enumerate(styles):
        sF = np.asarray(mods.encode(level, st), np.float64).reshape(C, -1)
        acc += lh[k] * wct_oracle.whiten_and_color(c, sF)
    csF = (alpha * acc + (1.0 - alpha) * c).reshape(cF.shape).astype(np.float64 if fp64 else np.float32)
    return mods.decode(level, csF)


def stylize_interp(mods, content, styles, lam, alpha: float = 1.0, num_run: int = 1, levels=(5, 4, 3, 2, 1)):
    cast = _cast(mods)
    img = cast(content)
    st = [cast(s) for s in styles]
    for _ in range(num_run):
        for L in levels:
            img = interp_transfer(mods, L, img, st, lam, alpha)
    return img


def interp_blended_slot(c: np.ndarray, sFs, lam) -> np.ndarray:
    """The same map as sum_k l_k whiten_and_color(c, sF_k) through ONE blended style slot: (sum l_k S_k) Wc (x - mu_c) + sum l_k mu_s,k."""
    lh = normalised(lam)
    _, mu_c, cov_c = wct_oracle.moments(c[:, :, None])
    S = sum(lh[k] * svd_power(wct_oracle.moments(s[:, :, None])[2], 0.5) for k, s in enumerate(sFs))
    mu_s = sum(lh[k] * s.mean(axis=1) for k, s in enumerate(sFs))
    return S @ (svd_power(cov_c, -0.5) @ (c - mu_c[:, None])) + mu_s[:, None]


# ---------------------------------------------------------------------------------------------------- tier 2
def pool_weights(weights: np.ndarray, level: int, h: int, w: int) -> np.ndarray:
    """w_k,L [K, h, w] (fp64) of the K x H x W maps: the mean over each feature pixel's s x s window."""
    s = 1 << (level - 1)
    K = weights.shape[0]
    return np.asarray(weights, np.float64)[:, : h * s, : w * s].reshape(K, h, s, w, s).mean(axis=(2, 4))


def weighted_moments(x: np.ndarray, wk: np.ndarray):
    """(V1, V2, mu, cov) of columns x [C, n] under weights wk [n]: the reliability-weighted unbiased covariance."""
    V1, V2 = float(wk.sum()), float((wk * wk).sum())
    mu = (x * wk).sum(axis=1) / V1
    xc = x - mu[:, None]
    cov = (xc * wk) @ xc.T / (V1 - V2 / V1)
    return V1, V2, mu, cov


def active(V1: float, V2: float) -> bool:
    return V1 > 0 and V2 > 0 and V1 * V1 / V2 >= 2


def blend_transfer(mods, level: int, img: np.ndarray, weights: np.ndarray, styles, alpha) -> np.ndarray:
    """One level of the weight-map cascade on the oracle's modules."""
    fp64 = getattr(mods, "precision", "fp32") == "fp64"
    cF = mods.encode(level, img)
    C, h, w = cF.shape
    wl = pool_weights(weights, level, h, w).reshape(len(styles), -1)
    x = np.asarray(cF, np.float64).reshape(C, -1)
    out = x.copy()
    for k, st in enumerate(styles):
        V1, V2 = float(wl[k].sum()), float((wl[k] * wl[k]).sum())
        if not active(V1, V2):
            continue
        _, _, mu, cov = weighted_moments(x, wl[k])
        _, mu_s, cov_s = wct_oracle.moments(np.asarray(mods.encode(level, st), np.float64))
        target = whiten_and_color_moments(x, mu, cov, mu_s, cov_s)
        out += wl[k] * alpha[k] * (target - x)
    csF = out.reshape(C, h, w).astype(np.float64 if fp64 else np.float32)
    return mods.decode(level, csF)


def stylize_blend(mods, content: np.ndarray, styles, weights: np.ndarray, alpha, num_run: int = 1, levels=(5, 4, 3, 2, 1)):
    """The cascade of WCT.py:120-125 with per-pixel style weights; `alpha` is a float or one per style."""
    K = len(styles)
    al = [float(alpha)] * K if np.isscalar(alpha) else [float(a) for a in alpha]
    cast = _cast(mods)
    img = cast(content)
    st = [cast(s) for s in styles]
    for _ in range(num_run):
        for L in levels:
            img = blend_transfer(mods, L, img, weights, st, al)
    return img
