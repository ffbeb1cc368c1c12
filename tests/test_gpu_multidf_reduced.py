"""bulkscan_multidf_reduced on the GPU: the peaks and LOD > thr triplets of the k-df scan out of the scan kernels' epilogues, held
bit for bit against the consumers (lod_colmax, lod_threshold) applied to the matrix bulkscan_multidf writes for the same inputs; an
oracle check that does not involve the sibling kernel; the order and special-value rules; the conditioning guard's traits; the _dev
form; the hand-off of the peaks to bulkscan_effects; the BXD shape."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from common import ATOL, RTOL, DevBuf, assert_lod_close, make_data
from multidf_ref import bulkscan_multidf_ref
from test_gpu_multidf import _founder_data, _opts_of

pytestmark = pytest.mark.gpu

GRID = np.array([i / 10.0 for i in range(10)])


def _tj(method, k):
    """Traits per wave of the scan kernel instance (kernels_mdf.hip: mdf_tj_grid / mdf_tj_exact)."""
    if method == "null-grid":
        return 16 if k <= 4 else 8
    return 16 if k == 1 else 8 if k == 2 else 4


def last_dims(ctx):
    pp, mm = C.c_int64(-1), C.c_int64(-1)
    rc = ctx.lib.blmm_last_dims(ctx.h, C.byref(pp), C.byref(mm))
    return rc, pp.value, mm.value


def _thr_of(L, q=0.9):
    fin = L[np.isfinite(L)]
    return float(np.quantile(fin, q)) if fin.size else 0.0


def _same_as_stored(blmm, red, stored, thr, what=""):
    """red (bulkscan_multidf_reduced's dict, with status) against the consumers on stored["L"], bit for bit."""
    L = stored["L"]
    mx, arg = blmm.lod_colmax(L)
    np.testing.assert_array_equal(red["max_lod"], mx, err_msg=f"{what}: maxima")
    np.testing.assert_array_equal(red["argmax"], arg, err_msg=f"{what}: arg-maxima")
    np.testing.assert_array_equal(red["h2_null_list"], stored["h2_null_list"], err_msg=f"{what}: h2")
    if thr is not None:
        ii, jj, ll = blmm.lod_threshold(L, thr)
        ti, tj, tl = red["triplets"]
        assert len(ti) == len(ii), (what, len(ti), len(ii))
        np.testing.assert_array_equal(ti, ii, err_msg=f"{what}: triplet loci")
        np.testing.assert_array_equal(tj, jj, err_msg=f"{what}: triplet traits")
        np.testing.assert_array_equal(tl, ll, err_msg=f"{what}: triplet LODs")
    a, b = red["status"], stored["status"]
    for f in ("n_nan_lod", "n_illcond_rescan", "n_zero_norm", "n_neg_eig", "n_nonpos_weight", "n_h2_boundary"):
        assert getattr(a, f) == getattr(b, f), (what, f, getattr(a, f), getattr(b, f))


def _both(blmm, Y, G, K, k, Cov, method, q=0.9, **kw):
    stored = blmm.bulkscan_multidf(Y, G, K, k, Cov, method=method, return_status=True, **kw)
    thr = _thr_of(stored["L"], q)
    ctx = blmm.default_context()
    red = blmm.bulkscan_multidf_reduced(Y, G, K, k, Cov, method=method, threshold=thr, return_status=True, **kw)
    assert last_dims(ctx) == (-1, 0, 0)                   # no resident matrix after the reduced call
    return stored, red, thr


# ---- 1. bit-identity at the wave and trait-tile edges ----------------------------------------------------------------------------
INSTANCES = [("null-grid", 1), ("null-grid", 2), ("null-grid", 5), ("null-grid", 8), ("null-exact", 1), ("null-exact", 2),
             ("null-exact", 4)]


@pytest.mark.parametrize("P", [63, 64, 65, 130])
@pytest.mark.parametrize("method,k", INSTANCES)
def test_bit_identical_to_the_consumers_on_the_stored_matrix(blmm, method, k, P):
    tj = _tj(method, k)
    for m in (4 * tj - 1, 4 * tj + 1):
        Y, G, K, Cov = _founder_data(79, P, k, m, seed=9000 + 100 * k + P + m, ncov=1)
        stored, red, thr = _both(blmm, Y, G, K, k, Cov, method)
        assert len(red["triplets"][0]) > 0
        assert red["route"] == 1
        _same_as_stored(blmm, red, stored, thr, f"{method} k = {k} P = {P} m = {m}")


def _host_abi(blmm, ctx, Y, G, K, k, method, thr, cap):
    """blmm_bulkscan_multidf_reduced itself (the Python wrapper would call again with a larger cap)."""
    n, m = Y.shape
    p = G.shape[1]
    Yf, Gf, Kf = (np.asfortranarray(a, dtype=np.float64) for a in (Y, G, K))
    mx = np.empty(m); arg = np.empty(m, dtype=np.int64); h2 = np.empty(m)
    ii = np.full(cap + 3, -7, dtype=np.int32); jj = np.full(cap + 3, -7, dtype=np.int32); ll = np.full(cap + 3, -7.0)
    cnt = C.c_int64(-1)
    meth = blmm._lib.BLMM_NULL_EXACT if method == "null-exact" else blmm._lib.BLMM_NULL_GRID
    o = blmm.api._opts(meth)
    r = blmm._lib.blmm_reduced(mx.ctypes.data, arg.ctypes.data, 1, thr, cap, ii.ctypes.data, jj.ctypes.data, ll.ctypes.data,
                               C.addressof(cnt))
    st = blmm._lib.blmm_status()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ctx.check(ctx.lib.blmm_bulkscan_multidf_reduced(ctx.h, C.byref(o), vp(Yf), n, m, vp(Gf), p, k, None, 0, vp(Kf), None,
                                                    None if method == "null-exact" else vp(GRID),
                                                    0 if method == "null-exact" else len(GRID), C.byref(r), vp(h2), C.byref(st)))
    return mx, arg, h2, ii, jj, ll, cnt.value


@pytest.mark.parametrize("method,k", [("null-grid", 2), ("null-exact", 2)])
def test_count_is_exact_beyond_cap(blmm, method, k):
    P, m = 130, 4 * _tj(method, k) + 1
    Y, G, K, _ = _founder_data(79, P, k, m, seed=9100 + k)
    ctx = blmm.default_context()
    L = blmm.bulkscan_multidf(Y, G, K, k, method=method)["L"]
    thr = _thr_of(L)
    ei, ej, el = blmm.lod_threshold(L, thr)
    cap = len(ei) // 3
    assert cap >= 8
    mx, arg, h2, ii, jj, ll, cnt = _host_abi(blmm, ctx, Y, G, K, k, method, thr, cap)
    assert cnt == len(ei) > cap
    assert (ii[cap:] == -7).all() and (jj[cap:] == -7).all() and (ll[cap:] == -7.0).all()        # nothing beyond cap
    got = set(zip(ii[:cap].tolist(), jj[:cap].tolist()))
    assert len(got) == cap                                                                       # distinct
    assert got <= set(zip(ei.tolist(), ej.tolist()))                                             # genuine
    np.testing.assert_array_equal(ll[:cap], L[ii[:cap], jj[:cap]])
    emx, earg = blmm.lod_colmax(L)
    np.testing.assert_array_equal(mx, emx); np.testing.assert_array_equal(arg, earg)


# ---- 2. independent of the sibling kernel --------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,k", [("null-grid", 5), ("null-exact", 4)])
def test_peaks_against_the_oracle(blmm, method, k):
    P, m = 130, 4 * _tj(method, k) + 1
    Y, G, K, Cov = _founder_data(79, P, k, m, seed=9200 + k, ncov=1)
    red = blmm.bulkscan_multidf_reduced(Y, G, K, k, Cov, method=method)
    ref = bulkscan_multidf_ref(Y, G, K, k, red["h2_null_list"], Covar=Cov)
    assert np.isfinite(ref).all()
    top = np.sort(ref, axis=0)[::-1]
    assert_lod_close(red["max_lod"], top[0], what=f"{method}: peak LOD")
    clear = top[0] - top[1] > 2.0 * (RTOL * np.abs(top[0]) + ATOL)
    assert clear.sum() >= m - 2
    np.testing.assert_array_equal(red["argmax"][clear], np.argmax(ref, axis=0)[clear])


# ---- 3. order and special values -------------------------------------------------------------------------------------------------
def _dev_pair(blmm, ctx, method, Y, G, K, k, Cov, thr, cap):
    """blmm_bulkscan_multidf_dev and blmm_bulkscan_multidf_reduced_dev on the same device buffers (the _dev forms report counters
    the host forms raise for).  Returns (L, its status), (colmax, argmax, h2, triplets sorted by (trait, locus), count, status)."""
    n, m = Y.shape
    p = G.shape[1]
    P = p // k
    ncov = 0 if Cov is None else Cov.shape[1]
    dY, dG, dK = DevBuf(Y.T), DevBuf(G.T), DevBuf(K)
    dC = DevBuf(Cov.T) if ncov else None
    dL, dh = DevBuf(nbytes=8 * P * m), DevBuf(nbytes=8 * m)
    dmx, darg, dh2 = DevBuf(nbytes=8 * m), DevBuf(nbytes=8 * m), DevBuf(nbytes=8 * m)
    dti, dtj, dtl, dcnt = DevBuf(nbytes=4 * cap), DevBuf(nbytes=4 * cap), DevBuf(nbytes=8 * cap), DevBuf(nbytes=8)
    bufs = [dY, dG, dK, dL, dh, dmx, darg, dh2, dti, dtj, dtl, dcnt] + ([dC] if dC else [])
    meth = blmm._lib.BLMM_NULL_EXACT if method == "null-exact" else blmm._lib.BLMM_NULL_GRID
    o = blmm.api._opts(meth)
    grid = None if method == "null-exact" else GRID.ctypes.data_as(C.c_void_p)
    ngrid = 0 if method == "null-exact" else len(GRID)
    cp = lambda b: C.c_void_p(b.ptr) if b else None  # noqa: E731
    st, sr = blmm._lib.blmm_status(), blmm._lib.blmm_status()
    try:
        ctx.check(ctx.lib.blmm_bulkscan_multidf_dev(ctx.h, C.byref(o), cp(dY), n, m, cp(dG), p, k, cp(dC), ncov, cp(dK), None, grid, ngrid,
                                                    cp(dL), P, cp(dh), C.byref(st)))
        ctx.synchronize()
        L = dL.get((m, P)).T.copy()
        r = blmm._lib.blmm_reduced(dmx.ptr, darg.ptr, 1, thr, cap, dti.ptr, dtj.ptr, dtl.ptr, dcnt.ptr)
        ctx.check(ctx.lib.blmm_bulkscan_multidf_reduced_dev(ctx.h, C.byref(o), cp(dY), n, m, cp(dG), p, k, cp(dC), ncov, cp(dK), None, grid,
                                                            ngrid, C.byref(r), cp(dh2), C.byref(sr)))
        assert last_dims(ctx) == (-1, 0, 0)               # the stored call's matrix is not served as the reduced call's
        cnt = int(dcnt.get(1, dtype=np.int64)[0])
        assert cnt <= cap
        ti, tj, tl = dti.get(cap, dtype=np.int32)[:cnt], dtj.get(cap, dtype=np.int32)[:cnt], dtl.get(cap)[:cnt]
        order = np.lexsort((ti, tj))
        np.testing.assert_array_equal(dh2.get(m), dh.get(m))
        return (L, st), (dmx.get(m), darg.get(m, dtype=np.int64), dh2.get(m), (ti[order], tj[order], tl[order]), cnt, sr)
    finally:
        for b in bufs:
            b.free()


def _check_pair(blmm, L, st, got, thr, what):
    mx, arg, _, (ti, tj, tl), cnt, sr = got
    emx, earg = blmm.lod_colmax(L)
    np.testing.assert_array_equal(mx, emx, err_msg=what); np.testing.assert_array_equal(arg, earg, err_msg=what)
    ei, ej, el = blmm.lod_threshold(L, thr)
    assert cnt == len(ei), (what, cnt, len(ei))
    np.testing.assert_array_equal(ti, ei, err_msg=what); np.testing.assert_array_equal(tj, ej, err_msg=what)
    np.testing.assert_array_equal(tl, el, err_msg=what)
    assert sr.n_nan_lod == st.n_nan_lod == int(np.isnan(L).sum()), (what, sr.n_nan_lod, st.n_nan_lod)
    assert sr.n_illcond_rescan == st.n_illcond_rescan and sr.n_zero_norm == st.n_zero_norm, what


@pytest.mark.parametrize("method,k,route", [("null-grid", 1, ""), ("null-exact", 1, ""), ("null-exact", 1, "qr")])
def test_order_and_special_values(blmm, method, k, route):
    """Locus 11 copied to locus 47 and trait 0 driven by it: the arg-max is 11.  Trait 5 is zero (zero null residual: every LOD NaN):
    (-inf, -1), no triplet, n_nan_lod = P as the stored scan counts it.  Trait 7 equals a covariate column: whatever the stored
    scan makes of its rounding-level residual, the reduced scan makes the same.  Traits 8 .. m - 1 are exact combinations of one
    locus's columns each: 1 - R^2 rounds to a tiny positive number, to 0 (+Inf) or below 0 (NaN) there.  At k = 1, R^2 is one
    square and about one exact fit in seven is +Inf on the device (at k = 3, a sum of three squares, one in fifty: too few to rest
    a test on), so the case runs at k = 1, where the m - 8 = 57 fits give several.  At every +Inf the locus is the trait's maximum
    (the lowest such locus) and is reported above thr = 1e300.  route "qr": c = 3 with illcond_rho = 2, every trait through
    k_mdf_qr's scratch."""
    n, P, m = 79, 70, 4 * _tj(method, k) + 1
    Y, G, K, Cov = _founder_data(n, P, k, m, seed=9300 + k, ncov=2)
    Y, G = Y.copy(), G.copy()
    rng = np.random.default_rng(9301)
    G[:, 47 * k:48 * k] = G[:, 11 * k:12 * k]
    Y[:, 0] = 10.0 + G[:, 11 * k:12 * k] @ rng.uniform(2.0, 3.0, k) + 0.3 * rng.standard_normal(n)
    Y[:, 5] = 0.0
    Y[:, 7] = Cov[:, 0]
    fit = {j: int(rng.integers(0, P)) for j in range(8, m)}
    for j, q in fit.items():
        Y[:, j] = 2.5 + G[:, q * k:(q + 1) * k] @ rng.uniform(1.0, 2.0, k)
    ctx = blmm.default_context()
    if route == "qr":
        ctx.set_tuning("illcond_rho", 2)                    # (reset by the conftest fixture)
    cap = P * m
    (L, st), first = _dev_pair(blmm, ctx, method, Y, G, K, k, Cov, 1.0, cap)      # thr = 1: the quantile needs L first
    if route == "qr":
        assert st.n_illcond_rescan == m
    _check_pair(blmm, L, st, first, 1.0, f"{method} {route}: thr = 1")
    thr = _thr_of(L)
    (L2, _), got = _dev_pair(blmm, ctx, method, Y, G, K, k, Cov, thr, cap)
    np.testing.assert_array_equal(L2, L)
    _check_pair(blmm, L, st, got, thr, f"{method} {route}")
    mx, arg, _, (ti, tj, tl), cnt, sr = got
    # the duplicated locus
    assert L[11, 0] == L[47, 0] == mx[0] and arg[0] == 11
    # the all-NaN trait
    assert np.isnan(L[:, 5]).all() and mx[5] == -math.inf and arg[5] == -1 and not (tj == 5).any()
    assert sr.n_nan_lod >= P and sr.n_zero_norm >= 1
    # +Inf
    (_, _), big = _dev_pair(blmm, ctx, method, Y, G, K, k, Cov, 1e300, cap)
    inf_i, inf_j = np.nonzero(L == math.inf)
    at_fit = np.array([L[q, j] for j, q in fit.items()])
    print(f"{method} {route}: exact fits: {int((at_fit == math.inf).sum())} +Inf, {int(np.isnan(at_fit).sum())} NaN, "
          f"{int(np.isfinite(at_fit).sum())} finite (min {np.nanmin(at_fit):.1f}); +Inf entries of L {len(inf_i)}")
    assert len(inf_i) >= 1
    order = np.lexsort((inf_i, inf_j))
    np.testing.assert_array_equal(big[3][0], inf_i[order]); np.testing.assert_array_equal(big[3][1], inf_j[order])
    assert (big[3][2] == math.inf).all() and big[4] == len(inf_i)
    for j in np.unique(inf_j):
        assert mx[j] == math.inf and arg[j] == int(np.flatnonzero(L[:, j] == math.inf)[0]), j
    # strict >
    fin = np.where(np.isfinite(L), L, -np.inf)
    i0, j0 = np.unravel_index(np.argsort(fin, axis=None)[-20], L.shape)
    at = float(L[i0, j0])
    (_, _), eq = _dev_pair(blmm, ctx, method, Y, G, K, k, Cov, at, cap)
    _check_pair(blmm, L, st, eq, at, f"{method} {route}: thr = an attained LOD")
    assert not ((eq[3][0] == i0) & (eq[3][1] == j0)).any() and (eq[3][2] > at).all() and eq[4] == int((L > at).sum())


# ---- 4. the conditioning guard ---------------------------------------------------------------------------------------------------
def test_guard_collinear_covariates_at_h2_one(blmm):
    """test_gpu_multidf.py's ill-conditioned case (n = 13, 7 covariates + intercept, traits at the h2 -> 1 boundary) at k = 2: the
    guard lists those traits, the epilogue leaves them out and k_mdf_qr's scratch supplies their peaks and triplets."""
    Y, G, K, Cov = make_data(n=13, p=63, m=15, seed=1000 + 237 + 7919 * 201, ncov=7, bxd=False)
    const = np.ptp(G, axis=0) == 0
    if const.any():
        G = G.copy(); G[:, const] = np.random.default_rng(237).random((13, int(const.sum())))
    G = np.ascontiguousarray(G[:, :62])
    stored, red, thr = _both(blmm, Y, G, K, 2, Cov, "null-exact", q=0.7)
    n_ill = stored["status"].n_illcond_rescan
    assert 0 < n_ill < Y.shape[1] and red["status"].n_illcond_rescan == n_ill
    assert red["route"] == 3
    _same_as_stored(blmm, red, stored, thr, "collinear covariates")
    flagged_hits = np.isin(red["triplets"][1], np.flatnonzero(stored["h2_null_list"] > 1.0 - 1e-6))
    print(f"re-scanned {n_ill}; triplets {len(flagged_hits)}, of flagged-range traits {int(flagged_hits.sum())}")


@pytest.mark.parametrize("chunk", [0, 7])
def test_guard_every_trait(blmm, chunk):
    """illcond_rho = 2: every trait goes through the scratch; chunk = 7 walks the list in chunks of 7, 7, 7, 7 and 2 traits."""
    Y, G, K, Cov = _founder_data(79, 77, 2, 30, seed=515, ncov=2)
    ctx = blmm.default_context()
    ctx.set_tuning("illcond_rho", 2)                        # (reset by the conftest fixture)
    ctx.set_tuning("mdf_red_chunk", chunk)
    stored, red, thr = _both(blmm, Y, G, K, 2, Cov, "null-exact")
    assert stored["status"].n_illcond_rescan == red["status"].n_illcond_rescan == Y.shape[1]
    assert red["route"] == 3 and len(red["triplets"][0]) > 0
    _same_as_stored(blmm, red, stored, thr, f"every trait, chunk {chunk}")


# ---- 5. options ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,k", [("null-grid", 5), ("null-exact", 2)])
def test_weights_reml_prior_three_covariates(blmm, method, k):
    P, m = 65, 4 * _tj(method, k) + 1
    Y, G, K, Cov = _founder_data(79, P, k, m, seed=9500 + k, ncov=2)
    stored, red, thr = _both(blmm, Y, G, K, k, Cov, method, **_opts_of("c3_reml_weights_prior"))
    _same_as_stored(blmm, red, stored, thr, f"{method} options")


# ---- 6. the torch wrapper --------------------------------------------------------------------------------------------------------
def test_torch_wrapper_in_its_own_process():
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "helpers", "multidf_reduced_dev_check.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "multidf_reduced_dev ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- 7. the peaks handed to bulkscan_effects -------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["null-grid", "null-exact"])
def test_effects_at_the_peaks(blmm, method):
    k, P, m = 2, 130, 33
    Y, G, K, _ = _founder_data(79, P, k, m, seed=9700)
    red = blmm.bulkscan_multidf_reduced(Y, G, K, k, method=method)
    assert (red["argmax"] >= 0).all()
    eff = blmm.bulkscan_effects(Y, G, K, k=k, locus=red["argmax"], trait=np.arange(m), method=method)
    np.testing.assert_array_equal(eff["h2_null_list"], red["h2_null_list"])
    assert_lod_close(eff["lod"], red["max_lod"], atol=ATOL, what="effects' lod at the peaks vs max_lod")


# ---- 8. the BXD shape ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["null-grid", "null-exact"])
def test_bxd_shape(blmm, method):
    n, P, k = 79, 7321, 2
    m = 4096 if method == "null-grid" else 256
    Y, G, K, _ = _founder_data(n, P, k, m, seed=79 + len(method))
    stored, red, thr = _both(blmm, Y, G, K, k, None, method, q=0.999)
    _same_as_stored(blmm, red, stored, thr, f"{method} BXD shape")
