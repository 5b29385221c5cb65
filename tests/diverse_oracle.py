"""numpy fp64 restatement of include/wct_hip_diverse.h -- TEST INFRASTRUCTURE ONLY (the product never imports this).

    words / skew   the seeded skew-symmetric A of Z(C, seed, stream_id, tag, strength): Philox4x32-10 as tests/synth_oracle.py restates it,
                   counter (i, i >> 32, stream_id, 0x524F5400 | tag); bit for bit what the device makes
    rotation       Z = (I - A)(I + A)^(-1) by a linear solve (LAPACK's LU: independent of the device's B^(-1/2) route)
    T_diverse      T = S Z cov_c^(-1/2), the colouring map of a rotated slot
"""
import numpy as np

from tests import synth_oracle as S
from tests import transform_oracle as O

TAG_BASE = 0x524F5400
MAX_STRENGTH = 8


def tag_word(tag):
    assert 0 <= int(tag) <= 255
    return TAG_BASE | int(tag)


def words(C, seed, stream_id, tag):
    """g of the C x C matrix G as exact integers (int64): element e = r C + c is word e & 3 of block e >> 2, read as int32."""
    total = C * C
    i = np.arange((total + 3) // 4, dtype=np.uint64)
    w = S.philox4x32_10((i & np.uint64(S.MASK), i >> np.uint64(32), np.full(i.shape, stream_id, np.uint64), np.full(i.shape, tag_word(tag), np.uint64)),
                        (seed & S.MASK, (seed >> 32) & S.MASK))
    flat = np.stack(w, axis=1).reshape(-1)[:total]
    return flat.view(np.int32).astype(np.int64).reshape(C, C)


def scale(C, strength):
    """s = strength / (2.0 * sqrt(2.0 * C / 3.0)), in IEEE double, in that order."""
    return float(strength) / (2.0 * float(np.sqrt(np.float64(2.0 * C / 3.0))))


def skew(C, seed, stream_id, tag, strength):
    g = words(C, seed, stream_id, tag)
    d = (g - g.T).astype(np.float64) * 2.0 ** -31          # |g_rc - g_cr| < 2^32: exact as a double, exact scaled
    up = np.triu(np.float64(scale(C, strength)) * d, 1)     # one rounding per entry
    return up + (0.0 - up.T)


def rotation(C, seed, stream_id, tag, strength):
    if strength == 0:
        return np.eye(C)
    A = skew(C, seed, stream_id, tag, strength)
    I = np.eye(C)
    return np.linalg.solve((I + A).T, (I - A).T).T           # (I - A)(I + A)^(-1)


def spectral_radius(C, seed, stream_id, tag):
    """of A / strength"""
    return float(np.abs(np.linalg.eigvals(skew(C, seed, stream_id, tag, 1.0))).max())


def rotate_stats(st, Z):
    """Style statistics in the export layout with S <- S Z."""
    Sm, mu = O.split_stats(st)
    return O.stats(Sm @ Z, mu)


def T_diverse(cov_c, Sm, Z):
    return Sm @ Z @ O.sym_pow(cov_c, -0.5)


def solve(n, s, ss, st, Z, alpha):
    """(M, b) of the wct transform against the slot rotated by Z."""
    mu_c, cov_c = O.mean_cov(n, s, ss)
    Sm, mu_s = O.split_stats(st)
    return O.mb(T_diverse(cov_c, Sm, Z), mu_c, mu_s, alpha)


def transform_features(cF, sF, Z, alpha):
    """csF of a CHW content feature against a CHW style feature whose cov_s^(1/2) is post-multiplied by Z, in fp64."""
    C = cF.shape[0]
    X, Y = np.asarray(cF, np.float64).reshape(C, -1), np.asarray(sF, np.float64).reshape(C, -1)
    mu_c, cov_c = O.mean_cov(X.shape[1], X.sum(1), X @ X.T)
    mu_s, cov_s = O.mean_cov(Y.shape[1], Y.sum(1), Y @ Y.T)
    M, b = O.mb(T_diverse(cov_c, O.sym_pow(cov_s, 0.5), Z), mu_c, mu_s, alpha)
    return (M @ X + b[:, None]).reshape(cF.shape)
