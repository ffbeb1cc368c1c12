"""NumPy oracle of blmm_bulkscan_effects, stated from its contract (include/bulklmm_hip.h) with oracle.bulklmm_oracle's own pieces:
transform_rotation (through multidf_ref._rotate), makeweights and wls -- the restatement of the reference's src/wls.jl -- and
multidf_ref's rank rule.  For test (locus l, trait j) it calls wls(y0_j, [Z0, accepted columns of the locus], w, prior, reml) and
takes beta and sigma2 from it; se comes from an explicit inverse of D~'D~ through the QR factor of D~ = sqrt(w) .* [Z0, columns].

Each trait's h2 is an INPUT (pin it to the device's h2_null_list, itself checked against bulkscan's).  Beside the outputs of the
contract the oracle returns `rho` (T x k: the ratios the rank rule compares with tau; NaN behind a column that has none) and `xe`
(T x k: x~_res' e~ for each column taken alone, whose sign is the sign of a k = 1 coefficient)."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from multidf_ref import TAU, _lod_block, _rotate
from oracle.bulklmm_oracle import makeweights, wls


class EffectsRef(NamedTuple):
    beta: np.ndarray
    se: np.ndarray
    sigma2: np.ndarray
    lod: np.ndarray
    accepted: np.ndarray
    rho: np.ndarray
    xe: np.ndarray


def effects_ref(Y, G, K, k: int, locus, trait, h2, Covar=None, addIntercept: bool = True, weights=None, prior_variance: float = 1.0,
                prior_sample_size: float = 0.0, reml: bool = False, decomp_scheme: str = "eigen", method: str = "qr",
                tau: float = TAU) -> EffectsRef:
    Y0, Z0, X0, lam = _rotate(Y, G, K, Covar, addIntercept, weights, decomp_scheme)
    n = Y0.shape[0]
    locus = np.asarray(locus, dtype=np.int64).ravel()
    trait = np.asarray(trait, dtype=np.int64).ravel()
    T = locus.shape[0]
    prior = (float(prior_variance), float(prior_sample_size))
    beta, se = np.zeros((T, k)), np.zeros((T, k))
    sigma2, lod = np.empty(T), np.empty(T)
    acc = np.zeros(T, dtype=np.int32)
    rho, xe = np.empty((T, k)), np.empty((T, k))
    cache = {}
    for t in range(T):
        l, j = int(locus[t]), int(trait[t])
        if (l, j) in cache:
            beta[t], se[t], sigma2[t], lod[t], acc[t], rho[t], xe[t] = cache[(l, j)]
            continue
        w = np.abs(makeweights(float(h2[j]), lam))
        s = np.sqrt(w)
        y0 = Y0[:, j]
        Xl = X0[:, l * k:(l + 1) * k]
        _, r = _lod_block(y0[:, None], Z0, Xl, k, s, n, tau)             # multidf_ref's rank rule on this locus alone
        rho[t] = r[0]
        keep = rho[t] > tau
        D = np.hstack([Z0, Xl[:, keep]])
        fit = wls(y0, D, w, prior, reml, loglik=False, method=method)
        b = np.asarray(fit.b).ravel()
        c = Z0.shape[1]
        beta[t, keep] = b[c:]
        sigma2[t] = fit.sigma2
        Dt = s[:, None] * D
        R = np.linalg.qr(Dt, mode="r")
        Ri = np.linalg.solve(R, np.eye(R.shape[0]))                      # (D~'D~)^-1 = R^-1 R^-T
        se[t, keep] = np.sqrt(fit.sigma2 * np.sum(Ri * Ri, axis=1)[c:])
        rss1 = float(np.sum((s * (y0 - D @ b)) ** 2))
        b0 = np.asarray(wls(y0, Z0, w, prior, reml, loglik=False, method=method).b).ravel()
        e = s * (y0 - Z0 @ b0)
        rss0 = float(e @ e)
        with np.errstate(divide="ignore", invalid="ignore"):
            lod[t] = -(n / 2.0) * np.log10(rss1 / rss0)
        acc[t] = int(sum(1 << a for a in range(k) if keep[a]))
        Qz, _ = np.linalg.qr(s[:, None] * Z0)
        xr = s[:, None] * Xl
        xr = xr - Qz @ (Qz.T @ xr)
        xr = xr - Qz @ (Qz.T @ xr)
        xe[t] = xr.T @ e
        cache[(l, j)] = (beta[t].copy(), se[t].copy(), sigma2[t], lod[t], acc[t], rho[t].copy(), xe[t].copy())
    return EffectsRef(beta, se, sigma2, lod, acc, rho, xe)
