"""NumPy oracle of the k-degree-of-freedom scan (blmm_bulkscan_multidf), stated from its contract (include/bulklmm_hip.h) and
independent of the device formulation: the locus columns are orthogonalised (Gram-Schmidt with re-orthogonalisation on the weighted,
rotated columns, batched over loci) and R^2 is the squared norm of the trait residual's projection -- no normal equations.

Each trait's h2 is an INPUT (pin it to the device's h2_null_list); the rotation and weights are oracle.bulklmm_oracle's.
`tau` is the rank rule's threshold (the contract's BLMM_MULTIDF_TAU by default); `return_rho` also gives, for every locus, column
and trait, the ratio rho = |r_a|^2 / |x~_a|^2 the rule compares with tau (r_a: the part of the weighted column orthogonal to the
covariates and to the accepted columns before it), so tests can tell decisive entries from those at the threshold."""
from __future__ import annotations

import numpy as np

from oracle.bulklmm_oracle import _apply_weights, _mat, makeweights, transform_rotation

TAU = 1e-8                                                               # BLMM_MULTIDF_TAU


def _rotate(Y, G, K, Covar, addIntercept, weights, decomp_scheme):
    Y = _mat(Y); G = _mat(G); K = _mat(K)
    n = Y.shape[0]
    if Covar is None:
        Covar = np.ones((n, 1))
        addIntercept = False
    Covar = _mat(Covar)
    c = Covar.shape[1] + (1 if addIntercept else 0)
    Y_st, G_st, Cov_st, K_st, addI = _apply_weights(Y, G, Covar, K, weights, addIntercept)
    Y0, X0, lam = transform_rotation(Y_st, np.hstack([Cov_st, G_st]), K_st, addIntercept=addI, decomp_scheme=decomp_scheme)
    return Y0, X0[:, :c], X0[:, c:], lam


def _lod_block(y0, Z0, X0, k, s, n, tau=TAU):
    """LODs of every locus (rows) for the traits of y0 (n x mj) that share the weights' square roots s, and rho (P x k)."""
    Zt = s[:, None] * Z0
    Qz, _ = np.linalg.qr(Zt)
    yt = s[:, None] * y0
    e = yt - Qz @ (Qz.T @ yt)
    e = e - Qz @ (Qz.T @ e)
    ee = np.sum(e * e, axis=0)
    P = X0.shape[1] // k
    Xt = (s[:, None] * X0).reshape(n, P, k).transpose(1, 0, 2)          # (P, n, k)
    R = Xt - np.einsum("nq,pqa->pna", Qz, np.einsum("nq,pna->pqa", Qz, Xt))
    R = R - np.einsum("nq,pqa->pna", Qz, np.einsum("nq,pna->pqa", Qz, R))
    Q = np.zeros_like(R)
    rho = np.empty((P, k))
    for a in range(k):
        v = R[:, :, a].copy()
        for _ in range(2):
            for b in range(a):
                v -= Q[:, :, b] * np.sum(Q[:, :, b] * v, axis=1, keepdims=True)
        nv = np.sum(v * v, axis=1)
        d0 = np.sum(Xt[:, :, a] ** 2, axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            rho[:, a] = nv / d0
        keep = nv > tau * d0
        Q[:, :, a] = np.where(keep[:, None], v / np.sqrt(np.where(keep, nv, 1.0))[:, None], 0.0)
    C = Q.transpose(0, 2, 1).reshape(P * k, n) @ e                     # (P k, mj)
    r2 = np.sum(C.reshape(P, k, -1) ** 2, axis=1) / ee[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        return -(n / 2.0) * np.log10(1.0 - r2), rho


def bulkscan_multidf_ref(Y, G, K, k: int, h2, Covar=None, addIntercept: bool = True, weights=None, decomp_scheme: str = "eigen",
                         tau: float = TAU, return_rho: bool = False):
    """L (P x m) of the contract, for the given per-trait heritabilities h2 (m), with the rank rule at `tau`.
    return_rho: (L, rho) with rho (P x k x m) -- trait j's entries are those of its h2 (traits of one h2 share them)."""
    Y0, Z0, X0, lam = _rotate(Y, G, K, Covar, addIntercept, weights, decomp_scheme)
    n, m = Y0.shape
    P = X0.shape[1] // k
    assert X0.shape[1] == P * k
    h2 = np.asarray(h2, dtype=np.float64).ravel()
    L = np.empty((P, m))
    rho = np.empty((P, k, m))
    for h in np.unique(h2):                                              # traits of one h2 share their weights (null-grid bins)
        idx = np.nonzero(h2 == h)[0]
        s = np.sqrt(np.abs(makeweights(float(h), lam)))
        L[:, idx], r = _lod_block(Y0[:, idx], Z0, X0, k, s, n, tau)
        rho[:, :, idx] = r[:, :, None]
    return (L, rho) if return_rho else L
