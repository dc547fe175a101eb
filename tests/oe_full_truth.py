"""The full optimal-estimation step of monortm_hip_oe_step_full restated in numpy long double, an independent
n-form with a full Se, and the generator of the full measurement-error covariances its tests use.

step_full() is the m-form as include/monortm_hip.h states it, built from the plain-loop Cholesky and triangular solves of oe_truth:
  M = K W + Se = L L^T,  a = L^-1 W^T,  b = L^-1 K,  gain_t = L^-T a,  avk = a^T b,  post_cov = Sa / (1 + gamma) - a^T a,  dofs = tr avk,
  chi2 = |L_e^-1 (y - F)|^2 with Se = L_e L_e^T.
nform_full() is the textbook route, S = [(1 + gamma) Sa^-1 + K^T Se^-1 K]^-1, G = S K^T Se^-1, A = G K: no factor of M appears in it.

full_se() draws Se = D^1/2 C D^1/2 + k_b k_b^T per profile:
  C     exp(-|j - j'| / ell), ell in [0.5, 2] channels: correlated channel noise
  D_jj  in [0.5, 2] sigma_e^2, sigma_e^2 = lambda_max(K Sa K^T) / 500
  k_b   ~ N(0, 0.25 sigma_e^2): one forward-model parameter's error, K_b S_b K_b^T of rank one
and asserts cond(M) < 1e4 (at gamma = 0, where it is largest) and cond(Se) < 1e3 in float64 for every profile.  (With the divisor 2000 of
oe_truth's diagonal generator cond(M) passes 1e4 at some shapes: the correlations lower Se's smallest eigenvalue.)"""
import numpy as np

import oe_truth as ot

LD = ot.LD


def sym_lower(S):
    """The matrix whose lower triangle S holds."""
    S = np.asarray(S, LD)
    return np.tril(S) + np.tril(S, -1).T


def step_full(K, Sa, Se, xa, x, y, F, gamma=0.0):
    """One profile in long double.  Se [m] (variances) or [m][m] (lower triangle read).  Dict of x_new, post_var, avk_diag [n], chi2,
    gain_t [m][n], avk, post_cov [n][n], dofs, and M, L, Se as used."""
    K, xa, x, y, F = (np.asarray(a, LD) for a in (K, xa, x, y, F))
    Sa = sym_lower(Sa)
    Se = np.diag(np.asarray(Se, LD)) if np.ndim(Se) == 1 else sym_lower(Se)
    g = LD(1) + LD(gamma)
    d = (xa - x) / g
    W = Sa @ K.T / g                               # [n][m]
    M = K @ W + Se
    L = ot.cholesky(M)
    r = (y - F) - K @ d
    z = ot.solve_upper_t(L, ot.solve_lower(L, r))
    a = ot.solve_lower(L, W.T)                     # [m][n]
    b = ot.solve_lower(L, K)
    avk = a.T @ b
    post_cov = Sa / g - a.T @ a
    ue = ot.solve_lower(ot.cholesky(Se), y - F)
    return dict(x_new=x + d + W @ z, post_var=np.diag(post_cov).copy(), avk_diag=np.diag(avk).copy(), chi2=np.sum(ue * ue),
                gain_t=ot.solve_upper_t(L, a), avk=avk, post_cov=post_cov, dofs=np.sum(np.diag(avk)), M=M, L=L, Se=Se)


def nform_full(K, Sa, Se, xa, x, y, F, gamma=0.0):
    """One profile, the n-form in long double with a full Se: dict of x_new, gain [n][m], avk, post_cov."""
    K, xa, x, y, F = (np.asarray(a, LD) for a in (K, xa, x, y, F))
    Sa = sym_lower(Sa)
    Se = np.diag(np.asarray(Se, LD)) if np.ndim(Se) == 1 else sym_lower(Se)
    Sai, Sei = ot.inverse_spd(Sa), ot.inverse_spd(Se)
    KtSe = K.T @ Sei
    S = ot.inverse_spd((LD(1) + LD(gamma)) * Sai + KtSe @ K)
    G = S @ KtSe
    return dict(x_new=x + S @ (KtSe @ (y - F) - Sai @ (x - xa)), gain=G, avk=G @ K, post_cov=S)


def full_se(K, Sa, rng, shared=False):
    """Se [nprof][m][m] for K [nprof][m][n] and Sa [nprof][n][n]; shared: one Se for all profiles, scaled by the largest lambda_max among
    them.  Asserts cond(M) < 1e4 and cond(Se) < 1e3 for every profile."""
    nprof, m, _ = K.shape
    S = [K[p] @ Sa[p] @ K[p].T for p in range(nprof)]
    lam = [max(float(np.linalg.eigvalsh(s)[-1]), 1e-300) for s in S]
    j = np.arange(m)

    def draw(sig2):
        C = np.exp(-np.abs(j[:, None] - j[None, :]) / rng.uniform(0.5, 2.0))
        dh = np.sqrt(rng.uniform(0.5, 2.0, m) * sig2)
        kb = rng.normal(0.0, np.sqrt(0.25 * sig2), m)
        return dh[:, None] * C * dh[None, :] + np.outer(kb, kb)

    one = draw(max(lam) / 500.0)
    Se = np.stack([one if shared else draw(lam[p] / 500.0) for p in range(nprof)])
    for p in range(nprof):
        cm, ce = np.linalg.cond(S[p] + Se[p]), np.linalg.cond(Se[p])
        assert cm < 1e4, f"profile {p}: cond(M) = {cm:.3g}"
        assert ce < 1e3, f"profile {p}: cond(Se) = {ce:.3g}"
    return Se


def finish_full(K, Sa, rng, shared_se=False):
    """Se (full_se), xa, x, y, F for given K and Sa, as oe_truth.finish_case draws them; the noise of y has covariance Se."""
    nprof, m, n = K.shape
    Se = full_se(K, Sa, rng, shared=shared_se)
    xa, x, y, F = (np.zeros(s) for s in ((nprof, n), (nprof, n), (nprof, m), (nprof, m)))
    for p in range(nprof):
        C = np.linalg.cholesky(Sa[p])
        xa[p] = rng.normal(0.0, 5.0, n)
        x[p] = xa[p] + 0.5 * C @ rng.normal(size=n)
        F[p] = rng.normal(250.0, 20.0, m)
        y[p] = F[p] + K[p] @ (C @ rng.normal(size=n)) + np.linalg.cholesky(Se[p]) @ rng.normal(size=m)
    return dict(K=K, Sa=Sa, Se=Se, xa=xa, x=x, y=y, F=F)


def make_case(m, n, nprof=1, seed=0):
    """oe_truth.make_case with a full Se."""
    rng = np.random.default_rng(1000 * m + n + 7919 * seed + 1)
    K = np.stack([ot.smooth_k(m, n, rng) for _ in range(nprof)])
    Sa = np.stack([ot.blocks_cov(n, rng) for _ in range(nprof)])
    return finish_full(K, Sa, rng)


# ---- the cases of tests/test_oe_full.py: K of all five kinds through a scrambled state map, as test_oe_step.make builds it ---------------
NFULL = [1, 7, 64, 65, 130, 300]     # against the 64-wide tiles of oe_cov_kernel: one state; less than a tile row; one tile exactly; one
#                                      tile plus one; three tiles (mirrored off-diagonal tiles exist); more than the 256 threads of a workgroup


def make_gpu_case(nview, nchan, n, seed=0, nprof=3, shared_sa=False, shared_se=False):
    import test_oe_step as tos

    rng = np.random.default_rng(11 + 31 * nview + 1009 * nchan + 17 * n + 7919 * seed)
    lm = max(2, -(-n // 5) + 1)
    ka = tos.k_arrays(nprof, nview, nchan, lm, rng)
    kind, row = tos.state_map(n, lm, rng)
    Sa = np.stack([ot.blocks_cov(n, rng) for _ in range(nprof)])
    if shared_sa:
        Sa[:] = Sa[0]
    c = finish_full(tos.gather(ka, kind, row), Sa, rng, shared_se=shared_se)
    c.update(ka=ka, kind=kind, row=row, lm=lm, nview=nview, nchan=nchan, shared_sa=shared_sa, shared_se=shared_se)
    return c
