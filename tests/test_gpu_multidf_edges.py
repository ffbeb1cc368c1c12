"""bulkscan_multidf at its edges: strong signals, exact fits, the rank rule's neighbourhood, the launch shapes of every scan kernel
instance, the sizes and covariate limit of the table and guard kernels, the options at k >= 2 and the torch wrapper.  Every LOD is
held against the NumPy oracle (multidf_ref) at the device's own h2_null_list under the project bound 1e-6 |ref| + 1e-10, except
where a section says otherwise.

Strong signals (test_gpu_strong_signal.py's rule): an error delta in R^2 moves L = -(n/2) log10(1 - R^2) by (n / ln 10) delta / u,
u = 1 - R^2, so entries are compared up to u = 2^-20 (LOD 237.8 at n = 79) and those beyond only have to be beyond it on both sides.
The oracle's own r^2 form agrees with a least-squares rss form to 1e-9 there (test_multidf_args.py).

Rank rule: a column is kept iff its pivot exceeds tau P_aa (tau = 1e-8).  The device forms the pivot by normal equations (S = P - U
U'), the oracle by Gram-Schmidt, so at rho = pivot / P_aa ~ tau the two may decide differently.  Adding a column never lowers R^2, so
every entry must lie between the oracle at 100 tau (fewer columns) and at tau / 100 (more), each with the bound; where rho is
decisive the two agree and this is the ordinary bound."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from common import ATOL, RTOL, DevBuf, assert_lod_close
from multidf_ref import TAU, bulkscan_multidf_ref
from oracle import bulklmm_oracle as O
from test_gpu_multidf import _founder_data, _opts_of
from test_gpu_strong_signal import cap_of, check

pytestmark = pytest.mark.gpu

MIN_PER_BAND = 24


def _tj(method, k):
    """Traits per wave of the scan kernel instance (kernels_mdf.hip: mdf_tj_grid / mdf_tj_exact)."""
    if method == "null-grid":
        return 16 if k <= 4 else 8
    return 16 if k == 1 else 8 if k == 2 else 4


def _run(blmm, Y, G, K, k, Cov, method, **kw):
    return blmm.bulkscan_multidf(Y, G, K, k, Cov, method=method, return_status=True, **kw)


# ---- a. strong signals -------------------------------------------------------------------------------------------------------
def strong_mdf(k, n=79, P=100, m_strong=320, m_plain=32, seed=4700, ncov=0, lo=-11.0, hi=-1.0):
    """_founder_data's traits with the first m_strong replaced by y = 10 + X_l beta + sigma (e + polygenic part on every other
    trait), sigma = 2^U(lo, hi): their peaks fill every octave band of u up to and beyond the cap."""
    Y, G, K, Cov = _founder_data(n, P, k, m_strong + m_plain, seed, ncov=ncov)
    rng = np.random.default_rng(seed + 1)
    lam, U = np.linalg.eigh(K)
    lam = np.maximum(lam, 0.0)
    q = rng.integers(0, P, size=m_strong)
    sigma = 2.0 ** rng.uniform(lo, hi, size=m_strong)
    for t in range(m_strong):
        e = rng.standard_normal(n)
        if t % 2:
            e = e + (U * np.sqrt(lam)) @ rng.standard_normal(n)
        Y[:, t] = 10.0 + G[:, q[t] * k:(q[t] + 1) * k] @ (2.0 * rng.standard_normal(k)) + sigma[t] * e
        if ncov:
            Y[:, t] += Cov @ rng.standard_normal(ncov)
    return Y, G, K, Cov


@pytest.mark.parametrize("method,k,route", [("null-grid", 2, ""), ("null-grid", 5, ""), ("null-grid", 8, ""),
                                            ("null-exact", 2, ""), ("null-exact", 3, ""), ("null-exact", 4, ""),
                                            ("null-exact", 3, "qr")])
def test_strong_signals(blmm, method, k, route):
    """Every u band up to 2^-20 held to the bound, the entries beyond the cap beyond it; the fused -log10 p (df = k) equal to the
    device's lod2log10p of the same L and, within the LOD bound (the slope of -log10 p in L is at most 1 for df >= 2), to the
    chi-square(k) tail of the oracle's L.  route "qr": c = 3 with illcond_rho = 2, every trait re-scanned by k_mdf_qr."""
    ncov = 2 if route == "qr" else 0
    Y, G, K, Cov = strong_mdf(k, ncov=ncov, seed=4700 + 10 * k + ncov)
    if route == "qr":
        blmm.default_context().set_tuning("illcond_rho", 2)          # (reset by the conftest fixture)
    r = _run(blmm, Y, G, K, k, Cov, method, output_pvals=True)
    n = Y.shape[0]
    st = r["status"]
    if route == "qr":
        assert st.n_illcond_rescan == Y.shape[1]
    assert st.n_nan_lod == 0
    Lref = bulkscan_multidf_ref(Y, G, K, k, r["h2_null_list"], Covar=Cov)
    L = r["L"]
    check(f"{method} k = {k} {route}", L, Lref, n, min_count=MIN_PER_BAND)
    assert r["Chisq_df"] == k
    Pv = r["log10Pvals_mat"]
    np.testing.assert_allclose(Pv, blmm.lod2log10p(L, k), rtol=1e-12, atol=1e-13)
    ok = Lref <= cap_of(n)
    Pref = O.lod2log10p(Lref[ok], k)
    assert np.isfinite(Pref).all()
    err = np.abs(Pv[ok] - Pref)
    assert np.all(err <= RTOL * np.abs(Lref[ok]) + ATOL + 1e-8 * Pref), float(np.max(err - RTOL * np.abs(Lref[ok])))


# ---- b. exact fits -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,k,route", [("null-grid", 3, ""), ("null-exact", 3, ""), ("null-exact", 2, "qr")])
def test_exact_fit_traits(blmm, method, k, route):
    """Trait 3 equals a + X_q beta; trait 9 equals a + X_q2 beta with locus q2 copied to q3, so two loci fit it.  Those entries must
    be +Inf, a LOD of at least 0.5 n 9 (u <= 1e-9) or NaN, every NaN of L counted once in n_nan_lod (the re-scan of k_mdf_qr
    replaces entries the scan already counted); every other entry meets the bound; the resident L's colmax follows k_colmax's rule
    (NaN never wins, +Inf does, ties go to the lower locus)."""
    ncov = 2 if route == "qr" else 0
    n, P, m = 79, 60, 16
    Y, G, K, Cov = _founder_data(n, P, k, m, seed=4800 + k + ncov, ncov=ncov)
    G = G.copy()
    q, q2, q3 = 11, 40, 47
    G[:, q3 * k:(q3 + 1) * k] = G[:, q2 * k:(q2 + 1) * k]
    rng = np.random.default_rng(4801)
    Y[:, 3] = 2.5 + G[:, q * k:(q + 1) * k] @ rng.uniform(1.0, 2.0, k)
    Y[:, 9] = -1.0 + G[:, q2 * k:(q2 + 1) * k] @ rng.uniform(-2.0, -1.0, k)
    if ncov:
        Y[:, 9] += Cov @ np.array([0.5, -0.25])
    exact = [(q, 3), (q2, 9), (q3, 9)]
    if route == "qr":
        blmm.default_context().set_tuning("illcond_rho", 2)
    r = _run(blmm, Y, G, K, k, Cov, method)
    L, st = r["L"], r["status"]
    if route == "qr":
        assert st.n_illcond_rescan == m
    mask = np.zeros(L.shape, bool)
    for i, j in exact:
        mask[i, j] = True
    vals = [float(v) for v in L[mask]]
    print(f"{method} k = {k} {route}: exact-fit entries {vals}; n_nan_lod {st.n_nan_lod}")
    assert all(v == math.inf or v >= 0.5 * n * 9 or math.isnan(v) for v in vals), vals
    assert st.n_nan_lod == int(np.isnan(L).sum())
    Lref = bulkscan_multidf_ref(Y, G, K, k, r["h2_null_list"], Covar=Cov)
    rest = ~mask
    assert np.isfinite(L[rest]).all() and np.isfinite(Lref[rest]).all()
    assert_lod_close(L[rest], Lref[rest], what=f"{method}: the other entries")
    kd = blmm.bulkscan_multidf(Y, G, K, k, Cov, method=method, keep_on_device=True)
    mx, arg = kd["L"].colmax()
    Lm = np.where(np.isnan(L), -np.inf, L)
    want = np.argmax(Lm, axis=0)
    np.testing.assert_array_equal(arg, want)
    np.testing.assert_array_equal(mx, Lm[want, np.arange(m)])


@pytest.mark.parametrize("method,route", [("null-grid", ""), ("null-exact", ""), ("null-exact", "qr")])
def test_nan_entries_are_counted_once(blmm, method, route):
    """A trait that is zero everywhere has a zero null residual: its unit residual is 0 / 0, so every LOD of it is NaN (and
    n_zero_norm is set: the host form raises, so this goes through the _dev form, which only reports).  n_nan_lod must count each
    NaN of L once -- also when k_mdf_qr re-scans the trait after the scan has counted its entries (route "qr": c = 3,
    illcond_rho = 2).  Every other trait meets the oracle."""
    n, P, m, k, z = 79, 70, 12, 2, 5
    Y, G, K, Cov = _founder_data(n, P, k, m, seed=4850, ncov=2)
    Y = Y.copy()
    Y[:, z] = 0.0
    ctx = blmm.default_context()
    if route == "qr":
        ctx.set_tuning("illcond_rho", 2)
    raw, h2, st = _dev_call(blmm, ctx, method, Y, G, K, k, Cov, P)
    L = raw[:P, :m].view(np.float64)
    print(f"{method} {route}: h2 of the zero trait {h2[z]!r}; n_nan_lod {st.n_nan_lod}, NaNs in L {int(np.isnan(L).sum())}, "
          f"n_zero_norm {st.n_zero_norm}, re-scanned {st.n_illcond_rescan}")
    assert np.isnan(L[:, z]).all() and st.n_zero_norm >= 1
    if route == "qr":
        assert st.n_illcond_rescan == m
    assert st.n_nan_lod == int(np.isnan(L).sum()) == P
    rest = np.arange(m) != z
    assert_lod_close(L[:, rest], bulkscan_multidf_ref(Y[:, rest], G, K, k, h2[rest], Covar=Cov))


# ---- c. the rank rule's neighbourhood --------------------------------------------------------------------------------------------
def near_collinear_loci(n, k, rng, per=4):
    """(n, P, k) loci whose last column is nearly in the span of the intercept and the others, rho from ~1e-1 down to ~1e-18:
    perturbed complements (B, 1 - B + delta N(0, 1)) (k = 3: two founders and their perturbed complement), additive + dominance
    codings with a rare heterozygote (probability 1e-3 everywhere but at two individuals, 1e-3 (1 + r)) and founder probabilities
    with a nearly absent founder (the k present ones sum to 1 - eps U(0, 1))."""
    out = []
    for d in 10.0 ** -np.arange(1.0, 8.01, 0.5):
        for _ in range(per):
            if k == 2:
                B = rng.random(n)
                out.append(np.stack([B, 1.0 - B + d * rng.standard_normal(n)], axis=1))
            else:
                B = rng.dirichlet(np.ones(3), n)[:, :2]
                out.append(np.column_stack([B, 1.0 - B.sum(axis=1) + d * rng.standard_normal(n)]))
    for r in 10.0 ** -np.arange(0.5, 6.01, 0.5):
        for _ in range(per):
            a = rng.integers(0, 2, n) * 2 - 1.0
            het = np.full(n, 1e-3)
            het[rng.choice(n, 2, replace=False)] *= 1.0 + r
            cols = [rng.random(n)] if k == 3 else []
            out.append(np.column_stack(cols + [a * (1.0 - het), het]))
    for e in 10.0 ** -np.arange(1.0, 8.01, 0.5):
        for _ in range(per):
            F = rng.dirichlet(np.full(k, 0.7), n)
            out.append(F * (1.0 - e * rng.random(n))[:, None])
    return np.stack(out, axis=1)


@pytest.mark.parametrize("method", ["null-grid", "null-exact"])
@pytest.mark.parametrize("k,ncov", [(2, 0), (2, 2), (3, 0), (3, 2)])
def test_rank_rule_neighbourhood(blmm, method, k, ncov):
    n, m = 79, 24
    rng = np.random.default_rng(4900 + 10 * k + ncov)
    X = near_collinear_loci(n, k, rng)
    P = X.shape[1]
    G = X.reshape(n, P * k)
    Y, _, K, Cov = _founder_data(n, 4, 1, m, seed=4901 + k + ncov, ncov=ncov)
    r = _run(blmm, Y, G, K, k, Cov, method)
    L, h2 = r["L"], r["h2_null_list"]
    assert r["status"].n_nan_lod == 0 and np.isfinite(L).all()
    _, rho = bulkscan_multidf_ref(Y, G, K, k, h2, Covar=Cov, return_rho=True)
    lo = bulkscan_multidf_ref(Y, G, K, k, h2, Covar=Cov, tau=100 * TAU)        # fewer columns: the smaller LOD
    hi = bulkscan_multidf_ref(Y, G, K, k, h2, Covar=Cov, tau=TAU / 100)        # more columns: the larger LOD
    amb = ((rho > TAU / 100) & (rho < 100 * TAU)).any(axis=1)
    kept = (rho >= 100 * TAU).all(axis=1)
    dropped = ~amb & ~kept
    print(f"{method} k = {k} c = {1 + ncov}: {P} loci; entries ambiguous {int(amb.sum())}, kept (rho >= 100 tau) "
          f"{int(kept.sum())}, dropped (rho <= tau / 100) {int(dropped.sum())}; mean LOD gain of the ambiguous columns "
          f"{float((hi - lo)[amb].mean()):.3f}")
    assert amb.sum() >= 20 and kept.sum() >= 20 and dropped.sum() >= 20
    assert np.all(L >= lo - (RTOL * np.abs(lo) + ATOL)), float(np.min(L - lo))
    assert np.all(L <= hi + (RTOL * np.abs(hi) + ATOL)), float(np.max(L - hi))
    assert_lod_close(L[~amb], hi[~amb], what="decisive entries")


# ---- d. launch shapes --------------------------------------------------------------------------------------------------------
SENTINEL = np.uint64(0x7FF8DEAD5EA7BEEF)          # a NaN with a payload no kernel writes
INSTANCES = [("null-grid", 2, ""), ("null-grid", 5, ""), ("null-exact", 1, ""), ("null-exact", 2, ""), ("null-exact", 4, ""),
             ("null-exact", 3, "qr")]


def _dev_call(blmm, ctx, method, Y, G, K, k, Cov, ldL, spare=1):
    """blmm_bulkscan_multidf_dev on DevBuf buffers; L (ldL x (m + spare), column-major) starts as SENTINEL everywhere."""
    n, m = Y.shape
    p = G.shape[1]
    ncov = 0 if Cov is None else Cov.shape[1]
    bufs = [DevBuf(Y.T), DevBuf(G.T), DevBuf(K)]
    dC = DevBuf(Cov.T) if ncov else None
    dL = DevBuf(np.full((m + spare, ldL), SENTINEL, dtype=np.uint64))
    dh = DevBuf(nbytes=8 * max(m, 1))
    grid = np.array([i / 10.0 for i in range(10)])
    meth = blmm._lib.BLMM_NULL_EXACT if method == "null-exact" else blmm._lib.BLMM_NULL_GRID
    o = blmm.api._opts(meth)
    st = blmm._lib.blmm_status()
    try:
        ctx.check(ctx.lib.blmm_bulkscan_multidf_dev(ctx.h, C.byref(o), C.c_void_p(bufs[0].ptr), n, m, C.c_void_p(bufs[1].ptr), p, k,
                                                    C.c_void_p(dC.ptr) if dC else None, ncov, C.c_void_p(bufs[2].ptr), None,
                                                    None if method == "null-exact" else grid.ctypes.data_as(C.c_void_p),
                                                    0 if method == "null-exact" else 10, C.c_void_p(dL.ptr), ldL, C.c_void_p(dh.ptr),
                                                    C.byref(st)))
        ctx.synchronize()
        return dL.get((m + spare, ldL), dtype=np.uint64).T, dh.get(m), st
    finally:
        for b in bufs + [dL, dh] + ([dC] if dC else []):
            b.free()


@pytest.mark.parametrize("method,k,route", INSTANCES)
def test_launch_shapes(blmm, method, k, route):
    """P in {63, 64, 65, 255, 256, 257} x m in {4 TJ - 1, 4 TJ, 4 TJ + 1}, and P = m = 1, through the _dev entry point with
    ldL = P + 5 and a spare column after m: every in-range entry meets the oracle; the padding rows (the clamped lanes of the last
    wave) and the spare column (the trait tail) still hold the sentinel."""
    tj = _tj(method, k)
    ncov = 1 if route == "qr" else 0
    Pmax, mmax = 257, 4 * tj + 1
    Yall, Gall, K, Cov = _founder_data(79, Pmax, k, mmax, seed=5000 + 10 * k + len(method) + ncov, ncov=ncov)
    ctx = blmm.default_context()
    if route == "qr":
        ctx.set_tuning("illcond_rho", 2)
    shapes = [(P, m) for P in (63, 64, 65, 255, 256, 257) for m in (4 * tj - 1, 4 * tj, 4 * tj + 1)] + [(1, 1)]
    for P, m in shapes:
        Y, G = Yall[:, :m], Gall[:, :P * k]
        ldL = P + 5
        raw, h2, st = _dev_call(blmm, ctx, method, Y, G, K, k, Cov, ldL)
        what = f"{method} k = {k} {route} P = {P} m = {m}"
        assert np.all(raw[P:, :m] == SENTINEL), f"{what}: a padding row was written"
        assert np.all(raw[:, m] == SENTINEL), f"{what}: the column after m was written"
        assert st.n_nan_lod == 0 and (st.n_illcond_rescan == m if route == "qr" else True), what
        Lref = bulkscan_multidf_ref(Y, G, K, k, h2, Covar=Cov)
        assert_lod_close(raw[:P, :m].view(np.float64), Lref, what=what)


# ---- e. sizes and the covariate limit --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,k", [("null-grid", 2), ("null-grid", 8), ("null-exact", 4)])
@pytest.mark.parametrize("n", [1000, 2048])
def test_sizes_and_covariate_limit(blmm, method, k, n):
    """n in {1000, 2048} x c in {2, 8}: k_mdf_table holds n (1 + c) doubles of dynamic LDS, 24 .. 144 KiB (above the 48 KiB
    default at every shape here but n = 1000, c = 2)."""
    for ncov in (1, 7):
        Y, G, K, Cov = _founder_data(n, 13, k, 10, seed=5100 + n + k + ncov, ncov=ncov)
        r = _run(blmm, Y, G, K, k, Cov, method)
        assert r["status"].n_nan_lod == 0
        Lref = bulkscan_multidf_ref(Y, G, K, k, r["h2_null_list"], Covar=Cov)
        assert_lod_close(r["L"], Lref, what=f"{method} k = {k} n = {n} c = {1 + ncov}")


@pytest.mark.parametrize("n,ncov,k", [(1000, 7, 3), (500, 2, 2)])
def test_guard_sizes(blmm, n, ncov, k):
    """illcond_rho = 2: every trait through k_mdf_qr, whose buffer of (c + 2) n doubles is 80 KB at n = 1000, c = 8 (the
    global-memory slab) and 20 KB at n = 500, c = 3 (LDS)."""
    Y, G, K, Cov = _founder_data(n, 21, k, 12, seed=5200 + n + ncov, ncov=ncov)
    blmm.default_context().set_tuning("illcond_rho", 2)
    r = _run(blmm, Y, G, K, k, Cov, "null-exact")
    assert r["status"].n_illcond_rescan == Y.shape[1] and r["status"].n_nan_lod == 0
    Lref = bulkscan_multidf_ref(Y, G, K, k, r["h2_null_list"], Covar=Cov)
    assert_lod_close(r["L"], Lref)


# ---- f. options at k >= 2 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["null-grid", "null-exact"])
def test_weights_reml_prior_at_k3(blmm, method):
    Y, G, K, Cov = _founder_data(79, 90, 3, 40, seed=5300, ncov=2)
    kw = _opts_of("c3_reml_weights_prior")
    r = _run(blmm, Y, G, K, 3, Cov, method, **kw)
    ref = blmm.bulkscan(Y, G, K, Cov, method=method, **kw)
    assert np.array_equal(r["h2_null_list"], ref["h2_null_list"])
    Lref = bulkscan_multidf_ref(Y, G, K, 3, r["h2_null_list"], Covar=Cov, weights=kw["weights"])
    assert_lod_close(r["L"], Lref)


@pytest.mark.parametrize("grid", ["dup", "zero", "high"])
def test_h2_grids_at_k4(blmm, grid):
    """test_gpu_grid_edges.DUP (unsorted, with duplicates), a single point at 0 and a grid reaching 0.95 / 0.99."""
    from test_gpu_grid_edges import DUP
    g = {"dup": DUP, "zero": [0.0], "high": [0.0, 0.3, 0.6, 0.8, 0.9, 0.95, 0.99]}[grid]
    Y, G, K, _ = _founder_data(79, 70, 4, 48, seed=5400 + len(grid))
    r = _run(blmm, Y, G, K, 4, None, "null-grid", h2_grid=g)
    ref = blmm.bulkscan(Y, G, K, method="null-grid", h2_grid=g)
    assert np.array_equal(r["h2_null_list"], ref["h2_null_list"])
    assert set(r["h2_null_list"].tolist()) <= set(g)
    assert_lod_close(r["L"], bulkscan_multidf_ref(Y, G, K, 4, r["h2_null_list"]))


# ---- g. the torch wrapper --------------------------------------------------------------------------------------------------------
def test_torch_wrapper_in_its_own_process():
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "helpers", "multidf_dev_check.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "multidf_dev ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
