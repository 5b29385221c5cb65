"""numpy fp64 reference of the feature transforms of include/wct_hip_transform.h.  Test infrastructure: the product never imports it.

All three are csF = M cF + b with M = alpha T + (1 - alpha) I, b = alpha (mu_s - T mu_c); S = cov_s^(1/2) and mu_s are what a style
slot holds (the wct_style_export layout).

    wct    T = S cov_c^(-1/2)
    ot     T = S B^(-1/2) S,  B = sym(S cov_c S)                      (the form the library computes)
           T = cov_c^(-1/2) (cov_c^(1/2) cov_s cov_c^(1/2))^(1/2) cov_c^(-1/2)    (ot_sigma_form: the textbook form, for full-rank cov_c)
    adain  T = diag(sqrt((cov_s_ii + eps) / (cov_c_ii + eps))),  cov_s_ii = SUM_k S_ik^2

Matrix functions are symmetric eigen-decompositions; directions with lambda <= REL lambda_max are dropped (pseudo-inverse)."""
import numpy as np

REL = 1e-12
ADAIN_EPS = 1e-5
MODES = ("wct", "ot", "adain")


def sym(A):
    return (A + A.T) / 2


def sym_pow(A, p, rel=REL):
    """A^p of a symmetric positive semi-definite A on the eigen-directions with lambda > rel lambda_max; the others contribute zero."""
    lam, V = np.linalg.eigh(sym(np.asarray(A, np.float64)))
    keep = lam > rel * max(float(lam.max()), 0.0)
    return (V[:, keep] * lam[keep] ** p) @ V[:, keep].T


def mean_cov(n, s, ss):
    """Unbiased mean and covariance from the raw moments (n, sum, sumsq), as solve.hip cov_value forms them."""
    s, ss = np.asarray(s, np.float64), np.asarray(ss, np.float64)
    mu = s / n
    return mu, sym((ss - n * np.outer(mu, mu)) / (n - 1.0))


def raw(n, mu, cov):
    """The raw moments (n, n mu, (n - 1) cov + n mu mu^T) of a mean and a covariance."""
    return float(n), n * mu, (n - 1) * cov + n * np.outer(mu, mu)


def stats(S, mu_s):
    """The wct_style_export layout: S [C*C] then mu_s [C]."""
    return np.concatenate([np.asarray(S, np.float64).reshape(-1), np.asarray(mu_s, np.float64)])


def split_stats(st):
    st = np.asarray(st, np.float64)
    C = int(round((np.sqrt(1 + 4 * st.size) - 1) / 2))
    assert C * C + C == st.size
    return st[:C * C].reshape(C, C), st[C * C:]


def T_wct(cov_c, S):
    return S @ sym_pow(cov_c, -0.5)


def ot_B(cov_c, S):
    return sym(S @ cov_c @ S)


def T_ot(cov_c, S):
    return S @ sym_pow(ot_B(cov_c, S), -0.5) @ S


def T_ot_sigma_form(cov_c, cov_s):
    """The Monge map in its textbook form; needs cov_c^(-1/2), so it is the same operator only where cov_c has full rank."""
    Cm, Cp = sym_pow(cov_c, -0.5), sym_pow(cov_c, 0.5)
    return Cm @ sym_pow(Cp @ cov_s @ Cp, 0.5) @ Cm


def T_adain(cov_c, S, eps=ADAIN_EPS):
    var_s = (np.asarray(S, np.float64) ** 2).sum(1)
    return np.diag(np.sqrt((var_s + eps) / (np.maximum(np.diag(cov_c), 0.0) + eps)))


def T_of(mode, cov_c, S):
    return {"wct": T_wct, "ot": T_ot, "adain": T_adain}[mode](cov_c, S)


def mb(T, mu_c, mu_s, alpha):
    C = T.shape[0]
    return alpha * T + (1.0 - alpha) * np.eye(C), alpha * (mu_s - T @ mu_c)


def solve(mode, n, s, ss, st, alpha):
    """(M, b) of `mode` from raw content moments and style statistics in the export layout."""
    mu_c, cov_c = mean_cov(n, s, ss)
    S, mu_s = split_stats(st)
    return mb(T_of(mode, cov_c, S), mu_c, mu_s, alpha)


def support_root(n, s, ss):
    """R = cov_c^(1/2): M R is the action of M on the content's support (centred content features are R times white noise)."""
    return sym_pow(mean_cov(n, s, ss)[1], 0.5)


def rel_fro(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300))


def transform_features(mode, cF, sF, alpha):
    """csF of a CHW content feature against a CHW style feature, in fp64 (the cascade arms of the GPU tests)."""
    C = cF.shape[0]
    X, Y = np.asarray(cF, np.float64).reshape(C, -1), np.asarray(sF, np.float64).reshape(C, -1)
    mu_c, cov_c = mean_cov(X.shape[1], X.sum(1), X @ X.T)
    mu_s, cov_s = mean_cov(Y.shape[1], Y.sum(1), Y @ Y.T)
    M, b = mb(T_of(mode, cov_c, sym_pow(cov_s, 0.5)), mu_c, mu_s, alpha)
    return (M @ X + b[:, None]).reshape(cF.shape)


def spd(rng, C, lo, dead=(), rank=None):
    """A covariance with log-uniform eigenvalues from 1 down to `lo` (tests/state_cases.raw_moments' spectra) on the channels not in
    `dead` (their rows and columns are exactly zero); rank: only that many eigen-directions are kept."""
    live = [i for i in range(C) if i not in set(dead)]
    m = len(live)
    Q, _ = np.linalg.qr(rng.standard_normal((m, m)))
    lam = np.exp(np.linspace(0.0, np.log(lo), m))
    if rank is not None:
        lam[rank:] = 0.0
    A = np.zeros((C, C))
    A[np.ix_(live, live)] = sym((Q * lam) @ Q.T)
    return A
