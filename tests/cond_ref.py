"""NumPy oracle of the conditional scan (blmm_bulkscan_cond), stated from its contract (include/bulklmm_hip.h) and independent of the
device formulation: the rotation, `fitlmm`, `wls` and `makeweights` are oracle.bulklmm_oracle's; every projection is Gram-Schmidt
done twice on explicit columns -- no normal equations.

Per trait j: step 1 keeps the conditioning columns whose part orthogonal to [Z0, the kept ones before] has squared norm > tau |x0|^2
(unweighted); the null model is fitted on D_j = [Z0, kept] (null-exact: fitlmm; null-grid: first arg-max of wls(...).ell over the
grid) unless `h2` is given (pin it to the device's h2_null_list); the scan applies the rank rule at the trait's weights.
Returns L (p x m), h2 (m), rho (p x m; |r_i|^2 / |x~_i|^2, what the rule compares with tau), kept (list of index arrays) and
n_dropped (conditioning entries dropped in step 1)."""
from __future__ import annotations

import numpy as np

from oracle.bulklmm_oracle import fitlmm, makeweights, wls
from multidf_ref import _rotate

TAU = 1e-8                                                               # BLMM_COND_TAU


def _gs2(v, Q):
    for _ in range(2):
        for q in Q:
            v = v - q * (q @ v)
    return v


def cond_table(cond, m):
    c = np.asarray(cond, dtype=np.int64)
    return c.reshape(m, -1) if c.size else np.zeros((m, 0), dtype=np.int64)


def step1(Z0, Xm, cj, tau=TAU):
    """The kept entries of cj (valid ones, in order) and the number dropped."""
    Q = []
    for a in range(Z0.shape[1]):
        v = _gs2(Z0[:, a].copy(), Q)
        Q.append(v / np.sqrt(v @ v))
    kept = []
    for q in cj:
        if q < 0:
            continue
        x = Xm[:, q]
        v = _gs2(x.copy(), Q)
        if v @ v > tau * (x @ x):
            Q.append(v / np.sqrt(v @ v))
            kept.append(int(q))
    return np.asarray(kept, dtype=np.int64), int((np.asarray(cj) >= 0).sum()) - len(kept)


def bulkscan_cond_ref(Y, G, K, cond, Covar=None, method="null-exact", h2_grid=None, h2=None, addIntercept=True, weights=None,
                      prior_variance=1.0, prior_sample_size=0.0, reml=False, optim_interval=1, decomp_scheme="eigen", tau=TAU,
                      traits=None):
    """`traits`: only these columns are computed (the others' outputs stay NaN) -- the BXD-shape test looks at 64 of 35,554."""
    Y0, Z0, Xm, lam = _rotate(Y, G, K, Covar, addIntercept, weights, decomp_scheme)
    n, m = Y0.shape
    p = Xm.shape[1]
    ctab = cond_table(cond, m)
    prior = [prior_variance, prior_sample_size]
    L = np.full((p, m), np.nan); H = np.full(m, np.nan); RHO = np.full((p, m), np.nan)
    kept_all, ndrop = [None] * m, 0
    for j in (range(m) if traits is None else traits):
        kept, nd = step1(Z0, Xm, ctab[j], tau)
        kept_all[j] = kept; ndrop += nd
        Dj = np.hstack([Z0, Xm[:, kept]])
        if h2 is not None:
            H[j] = h2[j]
        elif method == "null-exact":
            H[j] = fitlmm(Y0[:, [j]], Dj, lam, prior, reml=reml, optim_interval=optim_interval).h2
        else:
            ell = [wls(Y0[:, [j]], Dj, makeweights(float(g), lam), prior, reml=reml).ell for g in h2_grid]
            H[j] = h2_grid[int(np.argmax(ell))]
        s = np.sqrt(np.abs(makeweights(float(H[j]), lam)))
        Q = []
        for a in range(Dj.shape[1]):
            v = _gs2(s * Dj[:, a], Q)
            Q.append(v / np.sqrt(v @ v))
        Q = np.array(Q).T
        e = s * Y0[:, j]
        for _ in range(2):
            e = e - Q @ (Q.T @ e)
        Xt = s[:, None] * Xm
        R = Xt - Q @ (Q.T @ Xt)
        R = R - Q @ (Q.T @ R)
        nv = np.sum(R * R, axis=0); d0 = np.sum(Xt * Xt, axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            RHO[:, j] = nv / d0
        keep = nv > tau * d0
        r = np.where(keep, (R.T @ e) / np.sqrt(np.where(keep, nv, 1.0) * (e @ e)), 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            L[:, j] = np.where(keep, -(n / 2.0) * np.log10(1.0 - r * r), 0.0)
    return L, H, RHO, kept_all, ndrop


def assert_cond_close(got, h2_dev, Y, G, K, cond, assert_lod_close, traits=None, **kw):
    """got (p x m) against the oracle pinned at the device's h2: decisive entries within the parity bound; rule rows exactly +0.0;
    entries with rho in [TAU / 100, 100 TAU] (the band) must equal the oracle at one of the two thresholds, and at most 1e-4 of
    the entries may lie there.  Returns (number of rule entries of the oracle, band size)."""
    L, _, RHO, _, _ = bulkscan_cond_ref(Y, G, K, cond, h2=h2_dev, traits=traits, **kw)
    cols = np.arange(got.shape[1]) if traits is None else np.asarray(traits)
    got = got[:, cols]; L = L[:, cols]; RHO = RHO[:, cols]
    band = (RHO >= TAU / 100) & (RHO <= 100 * TAU)
    nband = int(band.sum())
    assert nband <= 1e-4 * band.size, f"{nband} of {band.size} entries in the rank-rule band"
    if nband:
        Llo = bulkscan_cond_ref(Y, G, K, cond, h2=h2_dev, traits=traits, tau=TAU / 100, **kw)[0][:, cols]
        Lhi = bulkscan_cond_ref(Y, G, K, cond, h2=h2_dev, traits=traits, tau=100 * TAU, **kw)[0][:, cols]
        bound = lambda ref: np.abs(got[band] - ref[band]) <= 1e-6 * np.abs(ref[band]) + 1e-10
        assert np.all(bound(Llo) | bound(Lhi)), "a band entry matches the oracle at neither threshold"
    rule = ~(RHO > TAU) & ~band
    zero = got[rule]
    assert np.all(zero == 0.0) and not np.signbit(zero).any(), "rule rows must be exactly +0.0"
    dec = ~band & ~rule
    assert_lod_close(got[dec], L[dec], what="conditional LOD")
    return int((~(RHO > TAU)).sum()), nband
