"""Oracles for the grid and permutation methods composed from pieces that are already tied to the reference (test
infrastructure, like bulklmm_oracle.py and cref.py: only tests/ may use it).

  null-grid    (src/bulkscan.jl:321-385, src/bulkscan_helpers.jl:239-292): the NumPy Ell table picks each trait's grid value
               (find_optim_h2, first maximum); the LODs are weighted_liteqtl at that value, which is the C/OpenMP restatement
               oracle/bulkscan_null_ref.c with its search skipped (cref.bulkscan_null(..., h2_override=h, skip_search=True)).
  alt-grid     (src/bulkscan.jl:428-526): logL1_g = ln10 LOD_g + Ell_g for every grid value g, one C pass each, folded with tmax!'s
               strict `<` (src/bulkscan_helpers.jl:330-350) under either h2_panel rule; L = (max_g logL1_g - max_g Ell_g) / ln10.
               Run over blocks of traits so that the per-grid LOD blocks of one block are held at once (the tie check needs them).
  permutations (src/scan.jl:485-557): bulklmm_oracle.scan on a shared rotation, over chunks of markers (a marker's row depends on
               no other marker), so that every marker of a large panel is compared.

Weights are applied as bulklmm_oracle._apply_weights does (pre-scaled Y, G, [1 Covar], W K W; no intercept added afterwards)."""
import math
import warnings

import numpy as np

from oracle import bulklmm_oracle as O
from oracle import cref

LN10 = math.log(10.0)


def prepare(Y, G, K, Covar=None, weights=None, addIntercept=True):
    """(Y, G, K, Covar, addIntercept) as the oracle's bulkscan_* see them after their Covar default and the weights."""
    Y = O._mat(Y)
    G = O._mat(G)
    K = O._mat(K)
    if Covar is None:
        Covar = np.ones((Y.shape[0], 1))
        addIntercept = False
    Y, G, Covar, K, addIntercept = O._apply_weights(Y, G, O._mat(Covar), K, weights, addIntercept)
    return Y, G, K, Covar, addIntercept


def ell_table(Y, K, Covar, addIntercept, grid, prior=(1.0, 0.0), reml=False):
    """Ell[g, j]: the null log-likelihood of trait j at grid value g (wls_multivar on the rotated covariates, vectorised over the
    traits) -- the table gridscan_by_bin and bulkscan_alt_grid maximise.  Inputs as returned by prepare()."""
    Y0, X0, lam = O.transform_rotation(Y, Covar, K, addIntercept=addIntercept)
    rows = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for h in grid:
            rows.append(O.wls_multivar(Y0, X0, O.makeweights(float(h), lam), list(prior), reml=reml).Ell[0])
    return np.vstack(rows)


def lod_at(Y, G, K, Covar, addIntercept, h2, nthreads=0):
    """p x m LODs of weighted_liteqtl at the heritabilities h2 (one per trait) through the C restatement."""
    h2 = np.broadcast_to(np.asarray(h2, dtype=np.float64), (Y.shape[1],))
    L, _ = cref.bulkscan_null(Y, G, K, Covar, addIntercept=addIntercept, nthreads=nthreads, h2_override=h2, skip_search=True)
    return L


def null_grid(Y, G, K, grid, Covar=None, weights=None, prior=(1.0, 0.0), reml=False, h2=None, nthreads=0):
    """null-grid: (L, h2 of the oracle's own first-maximum pick, Ell table).  L is evaluated at `h2` when given (the device's
    choice), else at the oracle's."""
    Y, G, K, Covar, ai = prepare(Y, G, K, Covar, weights)
    grid = np.asarray(grid, dtype=np.float64)
    Ell = ell_table(Y, K, Covar, ai, grid, prior, reml)
    pick = grid[np.argmax(Ell, axis=0)]
    L = lod_at(Y, G, K, Covar, ai, pick if h2 is None else h2, nthreads)
    return L, pick, Ell


def alt_grid(Y, G, K, grid, Covar=None, weights=None, prior=(1.0, 0.0), reml=False, quirk=False, dev_panel=None, block=1024,
             nthreads=0, Ell=None):
    """alt-grid: (L, h2_panel, mismatches).  h2_panel follows the first arg-max, or with `quirk` the reference's improvement counter
    (SURVEY.md B2).  `dev_panel` (p x m): a panel to hold against this one; every entry where the two differ is returned in
    `mismatches` as (marker, trait, gap), gap the relative distance in logL1 that separates the two candidates (first arg-max:
    |logL1 at the device's value - logL1 at the oracle's|; counter rule: the smallest |logL1_g - running max before g| along the
    grid, since the counter depends on every comparison), both over max(1, max_g |logL1_g|).  Ties at rounding level are the only
    acceptable mismatches (tests/common.py: assert_h2_panel_ties_only)."""
    Y, G, K, Covar, ai = prepare(Y, G, K, Covar, weights)
    grid = np.asarray(grid, dtype=np.float64)
    ng = grid.size
    if Ell is None:
        Ell = ell_table(Y, K, Covar, ai, grid, prior, reml)
    p, m = G.shape[1], Y.shape[1]
    L = np.empty((p, m))
    panel = np.empty((p, m))
    mism = []
    for j0 in range(0, m, block):
        j1 = min(m, j0 + block)
        tab = np.empty((ng, p, j1 - j0))
        for g in range(ng):
            tab[g] = LN10 * lod_at(Y[:, j0:j1], G, K, Covar, ai, grid[g], nthreads) + Ell[g, j0:j1]
        best = tab[0].copy()
        idx = np.zeros((p, j1 - j0), dtype=np.int64)        # first arg-max, or the improvement counter - 1
        for g in range(1, ng):
            better = best < tab[g]
            best = np.where(better, tab[g], best)
            idx = idx + better if quirk else np.where(better, g, idx)
        L[:, j0:j1] = (best - Ell[:, j0:j1].max(axis=0)) / LN10
        panel[:, j0:j1] = grid[np.minimum(idx, ng - 1)]
        if dev_panel is not None:
            for i, jj in np.argwhere(dev_panel[:, j0:j1] != panel[:, j0:j1]):
                col = tab[:, i, jj]
                scale = max(1.0, float(np.abs(col).max()))
                if quirk:
                    run = np.maximum.accumulate(col)
                    gap = float(np.abs(col[1:] - run[:-1]).min()) if ng > 1 else math.inf
                else:
                    gd = np.flatnonzero(grid == dev_panel[i, j0 + jj])
                    gap = abs(float(col[gd[0]]) - float(col[idx[i, jj]])) if gd.size else math.inf
                mism.append((int(i), int(j0 + jj), gap / scale))
    return L, panel, mism


def perms(y, G, K, perm_idx, h2, rotation, chunk=16384):
    """scan(..., permutation_test=True) at the null heritability h2 and on a shared rotation (y0, X0 with the intercept column
    first, lambda), over chunks of `chunk` markers: (lod p, L_perms p x nperms)."""
    y0, X0, lam = rotation
    n, p = G.shape
    nperms = perm_idx.shape[1]
    lod = np.empty(p)
    Lp = np.empty((p, nperms))
    for i0 in range(0, p, chunk):
        i1 = min(p, i0 + chunk)
        X0s = np.hstack([X0[:, :1], X0[:, 1 + i0:1 + i1]])
        r = O.scan(y, G[:, i0:i1], K, covar=np.ones((n, 1)), addIntercept=False, permutation_test=True, nperms=nperms,
                   perm_idx=perm_idx, h2_override=h2, rotation_override=(y0, X0s, lam))
        lod[i0:i1] = r["lod"]
        Lp[i0:i1] = r["L_perms"]
    return lod, Lp
