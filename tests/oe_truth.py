"""The optimal-estimation step of monortm_hip_oe_step restated in numpy long double, and the cases of its tests.

step() is the m-form as include/monortm_hip.h states it - a Cholesky factorisation and triangular solves written as plain loops over the
pivots, every operation in np.longdouble (64-bit mantissa on x86: eps = 1.1e-19).  step_nform() is the textbook n-form,
  x + [(1 + gamma) Sa^-1 + K^T Se^-1 K]^-1 [K^T Se^-1 (y - F) - Sa^-1 (x - xa)],
with the same plain-loop factorisations: an independent route to x_new and to the posterior variances (the diagonal of the bracket's
inverse), and through A = S_hat K^T Se^-1 K to the averaging kernel.

make_case() builds a problem of m measurements and n states for nprof profiles:
  Sa    sigma_b^2 exp(-|i - j| / ell_b) on blocks b of the state vector (0 between blocks), sigma in [0.5, 3], ell in [2, 8] elements
  K     smooth weighting functions - a Gaussian bump per measurement along the state index, amplitude in [0.3, 1.5] - plus 5 % noise
  se    in [0.5, 2] sigma_e^2, sigma_e^2 = lambda_max(K Sa K^T) / 2000: cond(M) <= (2000 + 2) / 0.5 < 1e4 at gamma = 0, where it is largest;
        make_case asserts cond(M) < 1e4 in float64
  x     xa + a draw from Sa;  y = F + K (x_true - x) + noise of variance se."""
import numpy as np

LD = np.longdouble


def cholesky(M):
    """Lower L with L L^T = M, right-looking; a pivot <= 0 or not finite raises ArithmeticError."""
    A = np.array(M, LD)
    m = A.shape[0]
    L = np.zeros((m, m), LD)
    for k in range(m):
        d = A[k, k]
        if not (d > 0 and np.isfinite(d)):
            raise ArithmeticError(f"pivot {k}: {d}")
        L[k, k] = np.sqrt(d)
        L[k + 1:, k] = A[k + 1:, k] / L[k, k]
        A[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], L[k + 1:, k])
    return L


def solve_lower(L, B):
    """L^-1 B by forward substitution (B [m] or [m, nrhs])."""
    X = np.array(B, LD)
    for k in range(L.shape[0]):
        X[k] = X[k] / L[k, k]
        if k + 1 < L.shape[0]:
            X[k + 1:] -= np.multiply.outer(L[k + 1:, k], X[k])
    return X


def solve_upper_t(L, B):
    """L^-T B by back substitution."""
    X = np.array(B, LD)
    for k in range(L.shape[0] - 1, -1, -1):
        X[k] = X[k] / L[k, k]
        if k:
            X[:k] -= np.multiply.outer(L[k, :k], X[k])
    return X


def step(K, Sa, se, xa, x, y, F, gamma=0.0):
    """One profile, the m-form in long double: dict of x_new, post_var, avk_diag [n], chi2 and M's factor L."""
    K, Sa, se, xa, x, y, F = (np.asarray(a, LD) for a in (K, Sa, se, xa, x, y, F))
    Sa = np.tril(Sa) + np.tril(Sa, -1).T          # the lower triangle is the matrix
    g = LD(1) + LD(gamma)
    d = (xa - x) / g
    W = Sa @ K.T / g                               # [n][m]
    M = K @ W + np.diag(se)
    L = cholesky(M)
    r = (y - F) - K @ d
    z = solve_upper_t(L, solve_lower(L, r))
    a = solve_lower(L, W.T)                        # [m][n]: column i is L^-1 W_i
    b = solve_lower(L, K)
    return dict(x_new=x + d + W @ z, post_var=np.diag(Sa) / g - np.sum(a * a, axis=0), avk_diag=np.sum(a * b, axis=0),
                chi2=np.sum((y - F) ** 2 / se), L=L, M=M)


def inverse_spd(A):
    L = cholesky(A)
    Li = solve_lower(L, np.eye(A.shape[0], dtype=LD))
    return Li.T @ Li


def step_nform(K, Sa, se, xa, x, y, F, gamma=0.0):
    """One profile, the n-form in long double: dict of x_new, post_var, avk_diag."""
    K, Sa, se, xa, x, y, F = (np.asarray(a, LD) for a in (K, Sa, se, xa, x, y, F))
    Sa = np.tril(Sa) + np.tril(Sa, -1).T
    Sai = inverse_spd(Sa)
    KtSe = K.T / se
    S = inverse_spd((LD(1) + LD(gamma)) * Sai + KtSe @ K)
    return dict(x_new=x + S @ (KtSe @ (y - F) - Sai @ (x - xa)), post_var=np.diag(S).copy(), avk_diag=np.diag(S @ (KtSe @ K)).copy())


def blocks_cov(n, rng):
    """sigma_b^2 exp(-|i - j| / ell_b) on up to five blocks of the state vector."""
    nb = min(5, n)
    edges = np.unique(np.concatenate([[0, n], rng.choice(np.arange(1, n), nb - 1, replace=False)])) if n > 1 else np.array([0, 1])
    Sa = np.zeros((n, n))
    for a, b in zip(edges[:-1], edges[1:]):
        i = np.arange(b - a)
        Sa[a:b, a:b] = rng.uniform(0.5, 3.0) ** 2 * np.exp(-np.abs(i[:, None] - i[None, :]) / rng.uniform(2.0, 8.0))
    return Sa


def smooth_k(m, n, rng):
    u = (np.arange(n) + 0.5) / n
    c, w, amp = rng.uniform(0.0, 1.0, m), rng.uniform(0.05, 0.4, m), rng.uniform(0.3, 1.5, m) * rng.choice([-1.0, 1.0], m)
    return amp[:, None] * np.exp(-(((u[None, :] - c[:, None]) / w[:, None]) ** 2)) * (1.0 + 0.05 * rng.normal(size=(m, n)))


def finish_case(K, Sa, rng, shared_se=False):
    """se, xa, x, y, F for given K [nprof][m][n] and Sa [nprof][n][n]: dict of float64 arrays, cond(M) < 1e4 asserted for every profile.
    shared_se: one se for all profiles, sigma_e^2 from the largest lambda_max among them."""
    nprof, m, n = K.shape
    se, xa, x, y, F = (np.zeros(s) for s in ((nprof, m), (nprof, n), (nprof, n), (nprof, m), (nprof, m)))
    lam = [max(float(np.linalg.eigvalsh(K[p] @ Sa[p] @ K[p].T)[-1]), 1e-300) for p in range(nprof)]
    one = rng.uniform(0.5, 2.0, m) * max(lam) / 2000.0
    for p in range(nprof):
        S = K[p] @ Sa[p] @ K[p].T
        se[p] = one if shared_se else rng.uniform(0.5, 2.0, m) * lam[p] / 2000.0
        cond = np.linalg.cond(S + np.diag(se[p]))
        assert cond < 1e4, f"profile {p}: cond(M) = {cond:.3g}"
        C = np.linalg.cholesky(Sa[p])
        xa[p] = rng.normal(0.0, 5.0, n)
        x[p] = xa[p] + 0.5 * C @ rng.normal(size=n)
        F[p] = rng.normal(250.0, 20.0, m)
        y[p] = F[p] + K[p] @ (C @ rng.normal(size=n)) + np.sqrt(se[p]) * rng.normal(size=m)
    return dict(K=K, Sa=Sa, se=se, xa=xa, x=x, y=y, F=F)


def make_case(m, n, nprof=1, seed=0):
    rng = np.random.default_rng(1000 * m + n + 7919 * seed)
    K = np.stack([smooth_k(m, n, rng) for _ in range(nprof)])
    Sa = np.stack([blocks_cov(n, rng) for _ in range(nprof)])
    return finish_case(K, Sa, rng)
