"""The definition of spatial control (wct_stylize_regions) in numpy -- a test helper, not a fixture file.

Per level L = 5..1 (and run), from the level's current image:
  cF = e_L(img)                                   C x h x w (oracle.Modules)
  lab_L[i, j] = labels[i s + s//2, j s + s//2]    s = 2^(L-1): the centre of the pooling window, in ORIGINAL image coordinates
  region k (n_k = |{lab_L == k}| >= 2):  csF[:, P_k] = alpha_k whiten_and_color(cF[:, P_k], e_L(style_k)) + (1 - alpha_k) cF[:, P_k]
  n_k < 2, label 255:                    csF[:, P_k] = cF[:, P_k]
  img <- d_L(csF)
"""
import numpy as np

from oracle import wct_oracle

UNSTYLED = 255


def level_labels(labels: np.ndarray, level: int, h: int, w: int) -> np.ndarray:
    """lab_L of an h x w feature map of level L from the H x W label map."""
    s = 1 << (level - 1)
    return labels[s // 2 + s * np.arange(h)][:, s // 2 + s * np.arange(w)]


def region_transfer(mods, level: int, img: np.ndarray, labels: np.ndarray, styles, alpha) -> np.ndarray:
    """One level of the regions cascade on the oracle's modules."""
    fp64 = getattr(mods, "precision", "fp32") == "fp64"
    cF = mods.encode(level, img)
    C, h, w = cF.shape
    lab = level_labels(labels, level, h, w).reshape(-1)
    c = np.asarray(cF, np.float64).reshape(C, -1)
    out = c.copy()
    for k, st in enumerate(styles):
        sel = lab == k
        if int(sel.sum()) < 2:
            continue
        sF = np.asarray(mods.encode(level, st), np.float64)
        cs = c if sel.all() else c[:, sel]          # (the same array as oracle.transform's when one region covers the map)
        target = wct_oracle.whiten_and_color(cs, sF.reshape(C, -1))
        out[:, sel] = alpha[k] * target + (1.0 - alpha[k]) * cs
    csF = out.reshape(C, h, w).astype(np.float64 if fp64 else np.float32)
    return mods.decode(level, csF)


def stylize_regions(mods, content: np.ndarray, styles, labels: np.ndarray, alpha, num_run: int = 1, levels=(5, 4, 3, 2, 1)):
    """The cascade of WCT.py:120-125 with per-region transforms; `alpha` is a float or one per style."""
    K = len(styles)
    al = [float(alpha)] * K if np.isscalar(alpha) else [float(a) for a in alpha]
    fp64 = getattr(mods, "precision", "fp32") == "fp64"
    cast = (lambda x: np.asarray(x, np.float64)) if fp64 else (lambda x: np.ascontiguousarray(x, np.float32))
    img = cast(content)
    st = [cast(s) for s in styles]
    for _ in range(num_run):
        for L in levels:
            img = region_transfer(mods, L, img, labels, st, al)
    return img
