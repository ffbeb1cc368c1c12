"""The front of a call on the fast eigen path (3 <= n <= 124): its first kernel, k_eigf_reduce, builds the weighted kinship Ks and
the design block Zs itself and zeroes the status block (no fill and no k_design launch in front of it), and the post-eigen work
(ranks, signs, U, Z0, the Gram matrix, Bq, Rp) runs on the whole workgroup.

  * null-exact scans at n = 3, 5, 79, 124 (the ends and the interior of the fast path) and n = 125 (the unchanged route: memset,
    k_design, the divide-and-conquer solver), each with and without weights, with the intercept alone (c = 1) and with three
    covariates and no intercept (c = 3; not at n = 3, where c < n rules it out), against the NumPy oracle at the project
    criterion, h2 within 1e-6; p = 130 and m = 70: ragged second tiles in both directions;
  * a kinship with a block of identical individuals (numerically repeated eigenvalues): the fast path's checks fail on the device
    and the Jacobi behind it consumes the Ks and Zs the new path wrote: U diag(lambda) U' gives the weighted K back to
    1e-12 |K| (spectral norms), the largest-magnitude component of every eigenvector is positive, a scan on it meets the oracle;
  * the status block does not leak between calls: after a call that sets counters (an indefinite kinship: n_neg_eig) a clean call
    on the same context reports what a fresh context reports, directly and behind another entry point (null-grid, scan_perms).
"""
import ctypes as C

import numpy as np
import pytest

from common import assert_lod_close, kinship_of, make_data
from f32_ref import weighted_kinship
from oracle import bulklmm_oracle as O

pytestmark = pytest.mark.gpu

P, M = 130, 70
SIZES = [3, 5, 79, 124, 125]
CASES = [(n, w, c) for n in SIZES for w in (False, True) for c in (1, 3) if c < n]
COUNTERS = ("n_neg_eig", "n_nonpos_weight", "n_zero_norm", "n_nan_lod", "n_brent_maxiter", "jacobi_sweeps", "lowrank_rank",
            "lowrank_fallback", "lowrank_shared", "n_h2_boundary", "n_h2_multimodal", "n_illcond_rescan")


def _weights(n, seed):
    return np.random.Generator(np.random.PCG64(seed)).uniform(0.5, 2.0, size=n)


def _bulkscan(blmm, ctx, Y, G, K, Covar=None, weights=None, addIntercept=True, method="null-exact", h2_grid=None):
    """blmm_bulkscan through the package's own argument plumbing, returning (L, h2, status) WITHOUT turning the counters into
    warnings or errors."""
    A, L = blmm.api, blmm.api.L
    meth = A._method(method)
    Y, G, K, n, m, p = A._host_arrays(Y, G, K)
    cov, ncov, w, addIntercept = A._host_covariates(Covar, weights, n, addIntercept)
    grid, ngrid = A._grid(meth, h2_grid)
    o = A._opts(meth, False, addIntercept, "eigen", 1, 1.0, 0.0, 0)
    Lout = np.empty((p, m), order="F")
    h2 = np.empty(m)
    st = L.blmm_status()
    ctx.check(ctx.lib.blmm_bulkscan(ctx.h, C.byref(o), A._p(Y), n, m, A._p(G), p, A._p(cov), ncov, A._p(K), A._p(w), A._p(grid), ngrid,
                                    A._p(Lout), A._p(h2), C.byref(st)))
    return Lout, h2, st


def _scan_perms(blmm, ctx, y, G, K, nperms=8, seed=3):
    A, L = blmm.api, blmm.api.L
    y, G, K, n, _, p = A._host_arrays(y.reshape(-1, 1), G, K)
    o = A._opts(L.BLMM_NULL_EXACT, False, True, "eigen", 1, 0.0, 0.0)
    scal, lod, Lp, st = np.zeros(2), np.empty(p), np.empty((p, nperms), order="F"), L.blmm_status()
    ctx.check(ctx.lib.blmm_scan_perms(ctx.h, C.byref(o), A._p(y), n, A._p(G), p, None, 0, A._p(K), None, nperms, C.c_uint64(seed), None,
                                      A._p(scal), A._p(lod), A._p(Lp), C.byref(st)))
    return lod, Lp, st


def _counters(st):
    return {f: int(getattr(st, f)) for f in COUNTERS}


def _data(n, c):
    Y, G, K, Cov = make_data(n=n, p=P, m=M, seed=7000 + n, ncov=3 if c == 3 else 0)
    if n < 10:
        # a handful of individuals: two-state genotypes would leave constant columns (zero norm once the covariates are projected out,
        # an error in the reference); genotype probabilities strictly inside (0, 1) instead, and their kinship
        G = np.random.Generator(np.random.PCG64(40 + n)).uniform(0.05, 0.95, size=(n, P))
        K = kinship_of(G)
    return Y, G, K, Cov


@pytest.mark.parametrize("n,weighted,c", CASES)
def test_scan_meets_the_oracle(blmm, gpu_ctx, n, weighted, c):
    Y, G, K, Cov = _data(n, c)
    w = _weights(n, 11 + n) if weighted else None
    kw = dict(Covar=Cov, addIntercept=(c == 1), weights=w)
    L, h2, st = _bulkscan(blmm, gpu_ctx, Y, G, K, **kw)
    own = O.bulkscan_null(Y, G, K, **kw)
    ref = O.bulkscan_null(Y, G, K, h2_override=h2, **kw)
    print(f"n {n} weights {weighted} c {c}: max |dh2| {np.abs(h2 - own.h2_null_list).max():.3e}, "
          f"max |dL| {np.nanmax(np.abs(L - ref.L)):.3e}, jacobi_sweeps {st.jacobi_sweeps}")
    assert np.abs(h2 - own.h2_null_list).max() <= 1e-6
    assert_lod_close(L, ref.L)
    assert st.n_neg_eig == 0 and st.n_nan_lod == 0 and st.n_zero_norm == 0


def _duplicated(n=79):
    """Individuals 0 .. 5 identical: six equal rows and columns of K, a five-fold eigenvalue at zero."""
    rng = np.random.Generator(np.random.PCG64(515))
    Y, G, _, _ = make_data(n=n, p=P, m=M, seed=9100, bxd=False)
    G[1:6] = G[0]
    X = G - 0.5
    K = np.round(2.0 * (X @ X.T) / P + 0.5, 12)     # (no unit diagonal: the six rows stay identical)
    Y[1:6] += 0.1 * rng.standard_normal((5, M))
    return Y, G, K


@pytest.mark.parametrize("weighted", [False, True])
def test_repeated_eigenvalues_take_the_jacobi_behind_the_new_front(blmm, gpu_ctx, weighted):
    Y, G, K = _duplicated()
    n = K.shape[0]
    w = _weights(n, 77) if weighted else None
    Kw = weighted_kinship(K, w)
    A, L = blmm.api, blmm.api.L
    o = A._opts(decomp_scheme="eigen", addIntercept=True)
    eye, g1 = np.asfortranarray(np.eye(n)), np.zeros((n, 1), order="F")
    Ut, X0, lam, st = np.empty((n, n), order="F"), np.empty((n, 2), order="F"), np.empty(n), L.blmm_status()
    Kf = np.asfortranarray(Kw)
    gpu_ctx.check(gpu_ctx.lib.blmm_rotate(gpu_ctx.h, C.byref(o), A._p(eye), n, n, A._p(g1), 1, None, 0, A._p(Kf), A._p(Ut), A._p(X0),
                                          A._p(lam), C.byref(st)))
    assert st.jacobi_sweeps > 0, "the fast path's checks passed: this kinship does not exercise the fallback"
    err = np.linalg.norm(Ut.T @ (lam[:, None] * Ut) - Kw, 2)
    nk = np.linalg.norm(Kw, 2)
    print(f"weights {weighted}: |U diag(lam) U' - K| {err:.3e}, |K| {nk:.3e}, sweeps {st.jacobi_sweeps}")
    assert err <= 1e-12 * nk
    assert np.all(np.diff(lam) >= 0)
    big = Ut[np.arange(n), np.argmax(np.abs(Ut), axis=1)]          # (argmax: the first of equal magnitudes, the kernel's rule)
    assert np.all(big > 0)
    # ... and a scan on it, weights through the library this time
    Lg, h2, st2 = _bulkscan(blmm, gpu_ctx, Y, G, K, weights=w)
    assert st2.jacobi_sweeps > 0
    own = O.bulkscan_null(Y, G, K, weights=w)
    ref = O.bulkscan_null(Y, G, K, weights=w, h2_override=h2)
    print(f"   scan: max |dh2| {np.abs(h2 - own.h2_null_list).max():.3e}, max |dL| {np.abs(Lg - ref.L).max():.3e}")
    assert np.abs(h2 - own.h2_null_list).max() <= 1e-6
    assert_lod_close(Lg, ref.L)


GRID = [i / 10.0 for i in range(10)]


@pytest.mark.parametrize("between", ["nothing", "null-grid", "scan_perms"])
def test_status_does_not_leak_between_calls(blmm, between):
    Y, G, K, _ = make_data(n=79, p=P, m=M, seed=8300)
    Kbad = K - 0.05 * np.eye(79)                      # indefinite: the smallest eigenvalues of the BXD kinship are ~1e-2
    assert np.linalg.eigvalsh(Kbad)[0] < -1e-3
    Ybad = Y.copy()
    Ybad[:, 0] = 10.0 + G[:, 5]                       # an exact fit at marker 5: LOD beyond every table range
    fresh, used = blmm.Context(0), blmm.Context(0)
    try:
        L0, h0, st0 = _bulkscan(blmm, fresh, Y, G, K)
        _, _, dirty = _bulkscan(blmm, used, Ybad, G, Kbad)
        print("dirty call:", _counters(dirty))
        assert dirty.n_neg_eig > 0
        if between == "null-grid":
            f = _bulkscan(blmm, fresh, Y, G, K, method="null-grid", h2_grid=GRID)
            u = _bulkscan(blmm, used, Y, G, K, method="null-grid", h2_grid=GRID)
            assert np.array_equal(f[0], u[0]) and _counters(f[2]) == _counters(u[2])
        elif between == "scan_perms":
            f = _scan_perms(blmm, fresh, Y[:, 1], G, K)
            u = _scan_perms(blmm, used, Y[:, 1], G, K)
            assert np.array_equal(f[0], u[0]) and np.array_equal(f[1], u[1]) and _counters(f[2]) == _counters(u[2])
        if between != "nothing":
            L0, h0, st0 = _bulkscan(blmm, fresh, Y, G, K)
        L1, h1, st1 = _bulkscan(blmm, used, Y, G, K)
        print("clean call:", _counters(st1))
        assert _counters(st1) == _counters(st0)
        assert st1.n_neg_eig == 0 and st1.n_nan_lod == 0
        assert np.array_equal(L1, L0) and np.array_equal(h1, h0)
    finally:
        fresh.close()
        used.close()
