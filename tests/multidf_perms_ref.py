"""NumPy oracle of the k-degree-of-freedom permutation scan (blmm_bulkscan_multidf_perms), stated from its contract
(include/bulklmm_hip.h) in the manner of multidf_ref._lod_block: QR of the weighted covariates, Gram-Schmidt with
re-orthogonalisation of the locus columns, and R^2 as the squared norm of a projection -- no normal equations, no factor table.

For trait j with s = sqrt(|makeweights(h2_j)|):  r0 = the residual of s .* y0_j on span(s .* Z0);  v_0 = r0, v_b = r0[perm[:, b - 1]];
  L_b[l] = -(n/2) log10(1 - |P_Q (I - P_Z~) v_b|^2 / |v_b|^2),   Q = the accepted residuals of the locus's weighted columns.
Each trait's h2 is an INPUT (pin it to the device's h2_null); the rotation and the weights are oracle.bulklmm_oracle's.  A
permutation acts on the coordinates of the kinship's eigenbasis, whose signs (and order within equal eigenvalues) are arbitrary, so
the permuted columns are defined only up to that choice: `rotation` = (Y0, Z0, X0, lam) pins it to the device's (as the 1-df
permutation tests pin O.scan's with rotation_override)."""
from __future__ import annotations

import numpy as np

from multidf_ref import TAU, _rotate
from oracle.bulklmm_oracle import makeweights


def _locus_basis(Qz, Xt, tau):
    """Orthonormal bases of the loci's accepted residual columns: Xt (P, n, k) weighted columns -> Q (P, n, k) (a dropped column
    is zero) and rho (P, k), the ratios the rank rule compares with tau."""
    P, n, k = Xt.shape
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
    return Q, rho


def bulkscan_multidf_perms_ref(Y, G, K, k: int, h2, perm_idx, Covar=None, addIntercept: bool = True, weights=None,
                               decomp_scheme: str = "eigen", tau: float = TAU, traits=None, return_rho: bool = False, rotation=None):
    """{trait j: L_j (P x (nperms + 1)), column 0 the unpermuted scan} for `traits` (default: all), with h2 the per-trait
    heritabilities of ALL traits (m) and perm_idx n x nperms (0-based; None or zero columns: no permutations).
    return_rho: (that dict, {j: rho_j (P x k)})."""
    Y0, Z0, X0, lam = rotation if rotation is not None else _rotate(Y, G, K, Covar, addIntercept, weights, decomp_scheme)
    n, m = Y0.shape
    P = X0.shape[1] // k
    assert X0.shape[1] == P * k
    h2 = np.asarray(h2, dtype=np.float64).ravel()
    perm = np.zeros((n, 0), dtype=np.int64) if perm_idx is None else np.asarray(perm_idx, dtype=np.int64)
    out, rhos = {}, {}
    for j in (range(m) if traits is None else traits):
        s = np.sqrt(np.abs(makeweights(float(h2[j]), lam)))
        Qz, _ = np.linalg.qr(s[:, None] * Z0)
        r0 = s * Y0[:, j]
        r0 = r0 - Qz @ (Qz.T @ r0)
        r0 = r0 - Qz @ (Qz.T @ r0)
        V = np.concatenate([r0[:, None], r0[perm]], axis=1)                  # (n, nperms + 1): v_b[i] = r0[perm[i, b - 1]]
        vv = np.sum(V * V, axis=0)
        E = V - Qz @ (Qz.T @ V)
        E = E - Qz @ (Qz.T @ E)
        Xt = (s[:, None] * X0).reshape(n, P, k).transpose(1, 0, 2)
        Q, rho = _locus_basis(Qz, Xt, tau)
        C = Q.transpose(0, 2, 1).reshape(P * k, n) @ E                        # (P k, nperms + 1)
        r2 = np.sum(C.reshape(P, k, -1) ** 2, axis=1) / vv[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            out[j] = -(n / 2.0) * np.log10(1.0 - r2)
        rhos[j] = rho
    return (out, rhos) if return_rho else out
