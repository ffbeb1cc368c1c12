"""Strong-signal traits: LODs beyond 0.602 n, where the scan epilogues leave their LOD table.

The fp64 epilogues turn u = 1 - r^2 into a LOD with a table over u in [2^-4, 1] (fastmath.h: fast_lod5); below that,
lod_out_of_range brings u into the table by exact powers of 16 (u 16^sh), and u = 0 gives +Inf, u < 0 NaN (counted in
n_nan_lod).  LOD = -(n/2) log10(u), so the edges u = 2^-4, 2^-8, 2^-12, 2^-16 sit at LOD 0.602 n k, k = 1..4: 47.6, 95.1, 142.7
and 190.2 at n = 79, 301 at n = 500 for the first.  Ordinary synthetic data never gets there (the largest headline LOD is 38);
a real cis-eQTL often does.  Here traits y = 10 + b G[:, q] + sigma (e + polygenic) with sigma swept log-uniformly put their
peaks and the LD shoulders of their peaks into every band up to the cap, mixed with ordinary traits, and every route that
writes or reduces a LOD is held against the oracle at the device's own heritability.

Conditioning: the comparison is only meaningful where u is not too small.  An absolute error delta in r moves
L = -(n/2) log10(1 - r^2) by dL = (n / ln 10) r delta / u ~ (n / ln 10) delta / u.  With delta ~ 1e-13 (the level of the low-rank
residual guard) that is 3.6e-6 at u = 2^-20 and n = 79, well inside 1e-6 L = 2.4e-4 there.  So entries are compared under the
project bound 1e-6 |ref| + 1e-10 up to u = 2^-20 (LOD 237.8 at n = 79); the few entries beyond that cap are only required to be
beyond it on both sides."""
import math

import numpy as np
import pytest

from common import RTOL, ATOL, assert_lod_close, kinship_of, make_data, make_geno
from oracle import bulklmm_oracle as O
from oracle import cref
from oracle import grid_ref as R

pytestmark = pytest.mark.gpu

LN2_LOG10 = math.log10(2.0)
GRID = [i / 16.0 for i in range(16)]
MIN_PER_BAND = 24


def strong_data(n=79, p=400, m_strong=320, m_plain=64, seed=4400, ncov=0, bxd=True, lo=-10.5, hi=-1.0):
    """make_data's traits with the first m_strong replaced by strong single-QTL traits; half of those have no polygenic part
    (h2 estimated at 0: the shared-weights class of the low-rank scan), half a polygenic share of 0.5 of the noise (rank-R class).
    sigma = 2^U(lo, hi): u at the peak ~ 4 sigma^2."""
    Y, G, K, Cov = make_data(n=n, p=p, m=m_strong + m_plain, seed=seed, ncov=ncov, bxd=bxd)
    rng = np.random.default_rng(seed + 1)
    if not bxd:     # a kinship independent of the scanned markers (as the BXD one is): one built from G itself absorbs the QTL
        K = kinship_of(make_geno(n, 1000, rng))
    lam, U = np.linalg.eigh(K)
    lam = np.maximum(lam, 0.0)
    q = rng.integers(0, p, size=m_strong)
    sigma = 2.0 ** rng.uniform(lo, hi, size=m_strong)
    for t in range(m_strong):
        e = rng.standard_normal(n)
        if t % 2:
            e = e + (U * np.sqrt(lam)) @ rng.standard_normal(n)
        Y[:, t] = 10.0 + G[:, q[t]] + sigma[t] * e
        if ncov:
            Y[:, t] += Cov @ rng.standard_normal(ncov)
    return Y, G, K, Cov


def bands(Lref, n):
    """Counts of entries per octave band of u: band 0 is u >= 2^-4 (the table), band k has u in [2^-4(k+1), 2^-4k)."""
    with np.errstate(over="ignore"):
        lg = 2.0 * Lref / n / LN2_LOG10                # -log2 u
    lg = lg[np.isfinite(lg)]
    return np.bincount(np.clip(np.floor(lg / 4.0).astype(np.int64), 0, 5), minlength=6)


def cap_of(n):
    return 0.5 * n * 20 * LN2_LOG10                  # u = 2^-20


def check(what, got, ref, n, min_bands=5, min_count=MIN_PER_BAND, rtol=RTOL, atol=ATOL):
    """The bound on every entry under the cap, both sides beyond it elsewhere; prints the band counts of the compared entries."""
    cap = cap_of(n)
    under = ref <= cap
    c = bands(np.where(under, ref, np.nan), n)
    print(f"{what}: {int(under.sum())} entries compared, {int((~under).sum())} beyond the cap LOD {cap:.1f}; per u band "
          f"[>=2^-4, 2^-8.., 2^-12.., 2^-16.., 2^-20..]: {c[:5].tolist()}; max LOD {float(np.nanmax(ref)):.1f}")
    assert np.isfinite(got).all()
    assert_lod_close(got[under], ref[under], rtol=rtol, atol=atol, what=what)
    assert (got[~under] > 0.99 * cap).all()
    assert (c[:min_bands] >= min_count).all(), c
    return c


@pytest.fixture(scope="module")
def strong():
    return strong_data()


@pytest.mark.parametrize("route", ["lowrank-c1", "lowrank-c3", "exact-c5", "exact-c11", "fix-rescan", "qr-rescan"])
def test_null_exact_routes_at_large_lod(blmm, route):
    """Every null-exact scan kernel at LODs up to 237.8 (n = 79): k_scan_lr (c = 1), k_scan_lr3 (c = 3), the exact kernel k_scan
    at c = 5 and c = 11 (run-time c), and the per-trait re-scans of the two guards (lr_tol = 0: every trait through k_scan_fix;
    illcond_rho = 2: every trait through k_scan_qr).  Fused -log10 p from the same call at every entry with LOD <= 300."""
    ncov = {"lowrank-c3": 2, "exact-c5": 4, "exact-c11": 10, "qr-rescan": 2}.get(route, 0)
    Y, G, K, Cov = strong_data(ncov=ncov, seed=4400 + ncov)
    ctx = blmm.default_context()
    if route == "fix-rescan":
        ctx.set_tuning("lr_tol", 0)                  # (reset by the conftest fixture)
    if route == "qr-rescan":
        ctx.set_tuning("illcond_rho", 2)
    L, h2, st = blmm.api._bulkscan_call(blmm._lib.BLMM_NULL_EXACT, Y, G, K, Cov, None, True, None, 1.0, 0.0, False, 1, "eigen", 0,
                                        ctx, return_status=True, pvals_df=1)
    P = blmm.api._last_log10p(ctx, L.shape, 1)
    if route == "fix-rescan":
        assert st.lowrank_fallback == Y.shape[1]
    if route == "qr-rescan":
        assert st.n_illcond_rescan == Y.shape[1]
    assert st.n_nan_lod == 0
    Lref, _ = cref.bulkscan_null(Y, G, K, Cov, h2_override=h2, skip_search=True)
    check(f"null-exact {route}", L, Lref, Y.shape[0])
    if route.startswith("lowrank"):                 # both weight classes hold strong traits
        rank_r = np.flatnonzero(h2[:320] > 1e-9)
        print(f"  strong traits in the shared-weights class {320 - rank_r.size}, in the rank-R class {rank_r.size}; "
              f"bands of the rank-R ones {bands(Lref[:, rank_r], Y.shape[0])[:5].tolist()}")
        assert rank_r.size >= 4 and 320 - rank_r.size >= 100 and bands(Lref[:, rank_r], Y.shape[0])[1] >= 1
    ok = L <= 300.0
    Pref = O.lod2log10p(L[ok], 1)
    assert np.isfinite(Pref).all()
    assert np.all(np.abs(P[ok] - Pref) <= 1e-10 * np.abs(Pref) + 1e-14), float(np.max(np.abs(P[ok] - Pref) / np.maximum(Pref, 1e-300)))


def test_null_grid_and_alt_grid_at_large_lod(blmm, strong):
    """k_scan's table class at the grid choice (null-grid) and k_scan_alt's fold at LODs up to the cap; fused p-values on null-grid."""
    Y, G, K, _ = strong
    n = Y.shape[0]
    r = blmm.bulkscan(Y, G, K, method="null-grid", h2_grid=GRID, output_pvals=True)
    Lref, pick, Ell = R.null_grid(Y, G, K, GRID, h2=r["h2_null_list"])
    check("null-grid", r["L"], Lref, n)
    diff = np.flatnonzero(r["h2_null_list"] != pick)
    for j in diff:
        gi = GRID.index(float(r["h2_null_list"][j]))
        assert abs(Ell[gi, j] - Ell[:, j].max()) <= 1e-12 * max(1.0, abs(Ell[:, j].max()))
    ok = r["L"] <= 300.0
    Pref = O.lod2log10p(r["L"][ok], 1)
    assert np.all(np.abs(r["log10Pvals_mat"][ok] - Pref) <= 1e-10 * np.abs(Pref) + 1e-14)
    for quirk in (False, True):
        a = blmm.bulkscan_alt_grid(Y, G, K, GRID, compat_counter_quirk=quirk)
        La, panel, mism = R.alt_grid(Y, G, K, GRID, quirk=quirk, dev_panel=a.h2_panel, Ell=Ell)
        check(f"alt-grid{' (counter rule)' if quirk else ''}", a.L, La, n)
        print(f"  h2_panel: {len(mism)} of {panel.size} entries differ from the oracle's, worst gap {max([g for *_, g in mism], default=0):.2e}")
        assert all(g <= 1e-12 for *_, g in mism)


@pytest.mark.parametrize("method", ["null-exact", "null-grid", "alt-grid"])
def test_reduced_calls_at_large_lod(blmm, strong, method):
    """bulkscan_reduced and bulkscan_reduced_async: peak, arg-max and the LOD > 150 triplets bit-equal to the stored matrix."""
    from test_gpu_reduced_async import Problem, assert_equal_to_stored, run_async
    Y, G, K, _ = strong
    full = blmm.bulkscan(Y, G, K, method=method, h2_grid=GRID)
    L = full["L"]
    thr = 150.0
    assert int((L > thr).sum()) >= MIN_PER_BAND
    red = blmm.bulkscan_reduced(Y, G, K, method=method, h2_grid=GRID, threshold=thr)
    arg = np.argmax(L, axis=0)
    assert np.array_equal(red["max_lod"], L[arg, np.arange(L.shape[1])]) and np.array_equal(red["argmax"], arg)
    ti, tj, tl = red["triplets"]
    assert ti.size == int((L > thr).sum()) and np.array_equal(tl, L[ti, tj])
    ctx = blmm.default_context()
    pr = Problem(blmm, Y, G, K, method=method, grid=np.asarray(GRID))
    try:
        Ls, h2s = pr.stored(ctx)
        assert np.array_equal(Ls, L)
        assert_equal_to_stored(run_async(ctx, pr, thr), Ls, h2s, thr, alt=method == "alt-grid")
    finally:
        pr.free()


def test_permutation_scan_at_large_lod(blmm, strong):
    """scan(..., permutation_test=True) on strong traits: the fp64 `lod` against the oracle on the shared rotation at 1e-6.
    The fp32 path rotates the markers in fp32, so the marker norms carry a relative error eps ~ 1e-7: r moves by r eps and
    L by (n / ln 10) r^2 eps / u, which at u = 2^-20 is O(1).  Its bound is therefore conditioning-aware:
    1e-6 |ref| + 1e-10 + (n / ln 10) 1e-6 r^2 / u; the ordinary-data assertion (tests/test_gpu_configs.py) is unchanged."""
    Y, G, K, _ = strong
    n, p = G.shape
    pidx = O.make_perm_idx(n, 7, 11)
    lods, ref_all = [], []
    worst32 = 0.0
    for t in range(0, 48):
        y = Y[:, t]
        g64 = blmm.scan(y, G, K, permutation_test=True, nperms=7, perm_idx=pidx)
        g32 = blmm.scan(y, G, K, permutation_test=True, nperms=7, perm_idx=pidx, perm_precision="f32")
        rot = blmm.transform_rotation(y.reshape(-1, 1), np.hstack([np.ones((n, 1)), G]), K, addIntercept=False)
        lod, Lp = R.perms(y, G, K, pidx, g64["h2_null"], rot)
        lods.append(g64["lod"]); ref_all.append(lod)
        assert_lod_close(g64["L_perms"], Lp, what="L_perms (fp64)")
        u = 10.0 ** (-2.0 * lod / n)
        under = lod <= cap_of(n)
        b32 = RTOL * np.abs(lod) + ATOL + (n / math.log(10.0)) * 1e-6 * (1.0 - u) / u
        err = np.abs(g32["lod"] - lod)
        worst32 = max(worst32, float((err[under] / b32[under]).max()))
        assert np.all(err[under] <= b32[under])
    print(f"  fp32 permutation path: worst error / conditioning-aware bound {worst32:.3e}")
    check("scan permutation lod (fp64)", np.stack(lods, 1), np.stack(ref_all, 1), n, min_count=4)


def test_n500_branch_starts_at_lod_301(blmm):
    """n = 500 (k_scan_lr at two waves, own eigensolver path for n > 79): the out-of-table branch starts at LOD 301."""
    Y, G, K, _ = strong_data(n=500, p=300, m_strong=128, m_plain=16, seed=4500, bxd=False, lo=-6.0, hi=-1.0)
    L, h2, st = blmm.api._bulkscan_call(blmm._lib.BLMM_NULL_EXACT, Y, G, K, None, None, True, None, 1.0, 0.0, False, 1, "eigen", 0,
                                        None, return_status=True)
    Lref, _ = cref.bulkscan_null(Y, G, K, None, h2_override=h2, skip_search=True)
    c = check("n = 500 null-exact", L, Lref, 500, min_bands=2)
    assert st.n_nan_lod == 0 and c[1] >= MIN_PER_BAND


@pytest.mark.parametrize("method", ["null-exact", "null-grid", "alt-grid"])
def test_exact_fit_traits(blmm, method):
    """A trait equal to a + b G[:, q] -- alone, and with G[:, q] copied into a second column, so two markers fit it exactly.  The
    exact-fit entries must be +Inf, a LOD of at least 0.5 n 9 (u <= 1e-9, allowing for the rounding of r), or NaN counted in
    n_nan_lod; every other entry of those traits meets the bound against the oracle; the reduced call follows k_colmax's rule
    (strictly larger, or equal at the lower marker; NaN never wins; +Inf does)."""
    Y, G, K, _ = strong_data(m_strong=8, m_plain=24, seed=4600)
    G = G.copy()
    n = Y.shape[0]
    q, q2, q3 = 17, 251, 90
    G[:, q2] = G[:, q]
    Y[:, 3] = 2.5 + 1.75 * G[:, q]                    # fits markers q and q2 exactly
    Y[:, 9] = -1.0 + 0.5 * G[:, q3]                   # fits marker q3 exactly
    exact = {(q, 3), (q2, 3), (q3, 9)}
    meth = {"null-exact": blmm._lib.BLMM_NULL_EXACT, "null-grid": blmm._lib.BLMM_NULL_GRID, "alt-grid": blmm._lib.BLMM_ALT_GRID}[method]
    L, h2, st = blmm.api._bulkscan_call(meth, Y, G, K, None, GRID, True, None, 1.0, 0.0, False, 1, "eigen", 0, None, return_status=True)
    if method == "null-exact":
        Lref, _ = cref.bulkscan_null(Y, G, K, None, h2_override=h2, skip_search=True)
    elif method == "null-grid":
        Lref, _, _ = R.null_grid(Y, G, K, GRID, h2=h2)
    else:
        Lref, _, _ = R.alt_grid(Y, G, K, GRID)
    mask = np.zeros(L.shape, bool)
    for i, j in exact:
        mask[i, j] = True
    ex = L[mask]
    vals = [float(v) for v in ex]
    print(f"{method}: exact-fit entries {vals}; n_nan_lod {st.n_nan_lod}")
    assert all(v == math.inf or v >= 0.5 * n * 9 or math.isnan(v) for v in vals), vals
    assert st.n_nan_lod == int(np.isnan(L).sum())
    rest = ~mask & np.isfinite(Lref) & (Lref <= cap_of(n))
    assert_lod_close(L[rest], Lref[rest], what=f"{method}: the other entries")
    assert np.isfinite(L[~mask]).all()
    red = blmm.bulkscan_reduced(Y, G, K, method=method, h2_grid=GRID)
    Lm = np.where(np.isnan(L), -np.inf, L)
    arg = np.argmax(Lm, axis=0)
    assert np.array_equal(red["argmax"], arg) and np.array_equal(red["max_lod"], Lm[arg, np.arange(L.shape[1])])
