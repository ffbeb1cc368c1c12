"""GPU checks of bulkscan_cond (blmm_bulkscan_cond) against the NumPy oracle of its contract (tests/cond_ref.py) and against the
library's own entry points where they state the same thing.  Bound: the project's |d| <= 1e-6 |ref| + 1e-10 with the oracle pinned
at the device's h2; rule rows exactly +0.0; at most 1e-4 of a test's entries in the rank-rule band (cond_ref.assert_cond_close)."""
import ctypes as C

import numpy as np
import pytest

from common import DevBuf, assert_lod_close, make_data
from cond_ref import assert_cond_close, bulkscan_cond_ref
from oracle import bulklmm_oracle as O
from test_gpu_parity import _fuzz_case

pytestmark = pytest.mark.gpu

GRID = [i / 10.0 for i in range(10)]


def _cond(rng, m, p, s, none_share=0.15):
    c = rng.integers(0, p, size=(m, s))
    c[rng.random((m, s)) < none_share] = -1
    return c


def _check(blmm, Y, G, K, cond, Cov, method, **kw):
    r = blmm.bulkscan_cond(Y, G, K, cond, Cov, method=method, return_status=True, **kw)
    okw = dict(Covar=Cov, **kw)
    nrule, nband = assert_cond_close(r["L"], r["h2_null_list"], Y, G, K, r["cond"], assert_lod_close, **okw)
    if nband == 0:
        assert r["n_rule_zero"] == nrule
    own = bulkscan_cond_ref(Y, G, K, r["cond"], method=method, h2_grid=GRID, **okw)
    if method == "null-grid":
        assert np.array_equal(r["h2_null_list"], own[1])
    else:
        assert np.abs(r["h2_null_list"] - own[1]).max() <= 1e-6
    assert r["n_cond_dropped"] == own[4] and r["n_cond_traits"] == sum(len(k) > 0 for k in own[3])
    return r


@pytest.mark.parametrize("method", ["null-grid", "null-exact"])
@pytest.mark.parametrize("s", [1, 2, 4])
@pytest.mark.parametrize("n,ncov", [(79, 0), (200, 1), (500, 2), (1000, 0)])
def test_against_the_oracle(blmm, method, s, n, ncov):
    """(n, c) in {(79, 1), (200, 2), (500, 3), (1000, 1)}: c counts the intercept."""
    m, p = (12, 150) if n <= 200 else (8, 130)
    Y, G, K, Cov = make_data(n=n, p=p, m=m, seed=100 * n + 10 * s + ncov, ncov=ncov)
    cond = _cond(np.random.default_rng(n + s), m, p, s)
    cond[0, 0] = int(np.argmax(O.bulkscan_null(Y[:, :1], G, K, Cov).L[:, 0]))     # one trait on its own peak
    _check(blmm, Y, G, K, cond, Cov, method)


@pytest.mark.parametrize("method", ["null-grid", "null-exact"])
def test_weights_reml_and_prior(blmm, method):
    Y, G, K, Cov = make_data(n=79, p=200, m=10, seed=77, ncov=2)
    w = np.random.default_rng(3).uniform(0.5, 2.0, 79)
    _check(blmm, Y, G, K, _cond(np.random.default_rng(9), 10, 200, 2), Cov, method, weights=w, reml=True, prior_variance=1.3,
           prior_sample_size=0.2)


@pytest.mark.parametrize("method", ["null-grid", "null-exact"])
def test_one_shared_locus_is_bulkscan_with_the_marker_as_covariate(blmm, method):
    Y, G, K, Cov = make_data(n=79, p=400, m=70, seed=31, ncov=1)
    q = 123
    r = blmm.bulkscan_cond(Y, G, K, np.full(70, q), Cov, method=method)
    ref = blmm.bulkscan(Y, G, K, np.hstack([Cov, G[:, [q]]]), method=method)
    ref_L, ref_h2 = (ref["L"], ref["h2_null_list"]) if isinstance(ref, dict) else (ref.L, ref.h2_null_list)
    if method == "null-grid":
        assert np.array_equal(r["h2_null_list"], ref_h2)
    else:
        assert np.abs(r["h2_null_list"] - ref_h2).max() <= 1e-6
    pin = bulkscan_cond_ref(Y, G, K, np.full(70, q), Covar=Cov, h2=r["h2_null_list"])
    dec = pin[2] > 1e-6                                   # decisive rows: away from the rule (bulkscan has no rule there)
    close = np.abs(r["h2_null_list"] - ref_h2) <= 1e-8    # both sides with their own h2
    assert_lod_close(r["L"][:, close][dec[:, close]], ref_L[:, close][dec[:, close]], rtol=1e-6, atol=1e-9)
    assert np.all(r["L"][q] == 0.0)


@pytest.mark.parametrize("method", ["null-grid", "null-exact"])
def test_no_conditioning_is_bulkscan(blmm, method):
    Y, G, K, Cov = make_data(n=79, p=300, m=50, seed=8, ncov=1)
    ref = blmm.bulkscan(Y, G, K, Cov, method=method)
    ref_L, ref_h2 = (ref["L"], ref["h2_null_list"]) if isinstance(ref, dict) else (ref.L, ref.h2_null_list)
    cond = np.full((50, 2), -1)
    cond[::3, 1] = 17
    for c in (np.full(50, -1), np.zeros((50, 0), dtype=int), cond):
        r = blmm.bulkscan_cond(Y, G, K, c, Cov, method=method)
        free = np.ones(50, dtype=bool) if c.ndim == 1 or c.shape[1] == 0 else (c < 0).all(axis=1)
        if method == "null-grid":
            assert np.array_equal(r["h2_null_list"][free], ref_h2[free])
        else:
            assert np.abs(r["h2_null_list"][free] - ref_h2[free]).max() <= 1e-6
        pin = O.bulkscan_null(Y[:, free], G, K, Covar=Cov, h2_override=r["h2_null_list"][free])
        assert_lod_close(r["L"][:, free], pin.L)
        assert_lod_close(r["L"][:, free], ref_L[:, free], rtol=1e-6, atol=1e-7)
        assert r["n_cond_traits"] == int((~free).sum())


@pytest.mark.parametrize("method", ["null-grid", "null-exact"])
def test_step_one(blmm, method):
    """Repeated index, a marker equal to a covariate, a constant marker: the result is the call with the shorter list and
    n_cond_dropped counts them; a trait's loci in another order give the same L within the bound."""
    Y, G, K, Cov = make_data(n=79, p=200, m=20, seed=5, ncov=1)
    G = G.copy(); G[:, 50] = Cov[:, 0]; G[:, 51] = 0.75
    long = np.stack([np.full(20, 10), np.full(20, 10), np.full(20, 50), np.full(20, 51)], axis=1)
    short = np.stack([np.full(20, 10)], axis=1)
    a = blmm.bulkscan_cond(Y, G, K, long, Cov, method=method)
    b = blmm.bulkscan_cond(Y, G, K, short, Cov, method=method)
    assert a["n_cond_dropped"] == 60 and b["n_cond_dropped"] == 0 and a["n_cond_traits"] == 20
    assert np.array_equal(a["h2_null_list"], b["h2_null_list"]) and np.array_equal(a["L"], b["L"])
    assert np.all(a["L"][[10, 50, 51]] == 0.0)
    x = blmm.bulkscan_cond(Y, G, K, np.stack([np.full(20, 10), np.full(20, 90), np.full(20, 150)], axis=1), method=method)
    y = blmm.bulkscan_cond(Y, G, K, np.stack([np.full(20, 150), np.full(20, 10), np.full(20, 90)], axis=1), method=method)
    if method == "null-grid":
        assert np.array_equal(x["h2_null_list"], y["h2_null_list"])
        assert_lod_close(x["L"], y["L"], rtol=2e-6, atol=2e-10)       # both within the bound of the same exact value
    else:
        assert np.abs(x["h2_null_list"] - y["h2_null_list"]).max() <= 1e-6
    _check(blmm, Y, G, K, long, Cov, method)


@pytest.mark.parametrize("method", ["null-grid", "null-exact"])
def test_duplicates_and_peak(blmm, method):
    Y, G, K, _ = make_data(n=79, p=300, m=40, seed=12)
    red = blmm.bulkscan_reduced(Y, G, K, method=method)
    r = blmm.bulkscan_cond(Y, G, K, "peak", method=method)
    assert np.array_equal(r["cond"][:, 0], red["argmax"]) and r["cond"].shape == (40, 1)
    assert all(r["L"][red["argmax"][j], j] == 0.0 for j in range(40))
    G2 = np.hstack([G, G[:, red["argmax"][:5]]])          # duplicates of five traits' conditioning markers at the end
    r2 = blmm.bulkscan_cond(Y, G2, K, red["argmax"], method=method)
    for j in range(5):
        z = r2["L"][300 + j, j]
        assert z == 0.0 and not np.signbit(z)
    assert_cond_close(r2["L"], r2["h2_null_list"], Y, G2, K, r2["cond"], assert_lod_close)


@pytest.mark.parametrize("p", [1, 63, 64, 65, 129, 257])
@pytest.mark.parametrize("m", [1, 5, 127, 129])
def test_tile_edges(blmm, p, m):
    """The seeds are chosen so that the ORACLE's rank-rule band is empty on the compared columns (smallest kept rho 2e-5 at h2 in
    {0, 0.5, 0.9}; with 1000 p + m one of 378 entries sat at rho = 2e-8): the 1e-4 cap is a statement about the inputs."""
    Y, G, K, _ = make_data(n=79, p=p, m=m, seed=3000 * p + m)
    cond = _cond(np.random.default_rng(p + m), m, p, 2)
    for method in ("null-grid", "null-exact"):
        r = blmm.bulkscan_cond(Y, G, K, cond, method=method)
        assert r["L"].shape == (p, m)
        cols = list(range(m)) if m <= 5 else [0, 1, 63, 64, m - 2, m - 1]
        assert_cond_close(r["L"], r["h2_null_list"], Y, G, K, cond, assert_lod_close, traits=cols)


SENTINEL = 0x7FF8DEADBEEF0001


def _dev_call(blmm, ctx, method, Y, G, K, cond, ldL, status=True, spare=1):
    n, m = Y.shape
    p = G.shape[1]
    s = cond.shape[1]
    bufs = [DevBuf(Y.T), DevBuf(G.T), DevBuf(K), DevBuf(np.ascontiguousarray(cond, dtype=np.int64))]
    dL = DevBuf(np.full((m + spare, ldL), SENTINEL, dtype=np.uint64))
    dh = DevBuf(nbytes=8 * m)
    di = DevBuf(nbytes=8 * 4)
    grid = np.array(GRID)
    o = blmm.api._opts(blmm._lib.BLMM_NULL_EXACT if method == "null-exact" else blmm._lib.BLMM_NULL_GRID)
    st = blmm._lib.blmm_status()
    try:
        rc = ctx.lib.blmm_bulkscan_cond_dev(ctx.h, C.byref(o), C.c_void_p(bufs[0].ptr), n, m, C.c_void_p(bufs[1].ptr), p, None, 0,
                                            C.c_void_p(bufs[2].ptr), None, None if method == "null-exact" else grid.ctypes.data_as(C.c_void_p),
                                            0 if method == "null-exact" else 10, C.c_void_p(bufs[3].ptr), s, C.c_void_p(dL.ptr), ldL,
                                            C.c_void_p(dh.ptr), C.c_void_p(di.ptr), C.byref(st) if status else None)
        ctx.synchronize()
        return rc, dL.get((m + spare, ldL), dtype=np.uint64).T, dh.get(m), di.get(4, dtype=np.int64)
    finally:
        for b in bufs + [dL, dh, di]:
            b.free()


@pytest.mark.parametrize("method", ["null-grid", "null-exact"])
def test_dev_form_padded_rows_and_out_of_range_indices(blmm, gpu_ctx, method):
    Y, G, K, _ = make_data(n=79, p=131, m=37, seed=44)
    cond = _cond(np.random.default_rng(1), 37, 131, 2)
    host = blmm.bulkscan_cond(Y, G, K, cond, method=method)
    rc, raw, h2, info = _dev_call(blmm, gpu_ctx, method, Y, G, K, cond, 131 + 5)
    assert rc == 0
    assert np.all(raw[131:, :] == SENTINEL) and np.all(raw[:, 37:] == SENTINEL)       # nothing outside the p x m block changes
    L = raw[:131, :37].copy().view(np.float64)
    assert np.array_equal(L, host["L"]) and np.array_equal(h2, host["h2_null_list"])
    assert info.tolist() == [host["n_rule_zero"], host["n_cond_dropped"], host["n_cond_traits"], 0]
    bad = cond.copy(); bad[7, 1] = 131; bad[20, 0] = -2
    rc, raw, h2b, _ = _dev_call(blmm, gpu_ctx, method, Y, G, K, bad, 131 + 5)
    assert rc == -1 and "outside [-1, p)" in blmm.load().blmm_last_error(gpu_ctx.h).decode()
    Lb = raw[:131, :37].copy().view(np.float64)
    assert np.isnan(Lb[:, [7, 20]]).all() and np.isnan(h2b[[7, 20]]).all()
    ok = np.setdiff1d(np.arange(37), [7, 20])
    assert np.array_equal(Lb[:, ok], host["L"][:, ok]) and np.array_equal(h2b[ok], host["h2_null_list"][ok])
    assert np.all(raw[131:, :] == SENTINEL) and np.all(raw[:, 37:] == SENTINEL)
    rc, _, _, _ = _dev_call(blmm, gpu_ctx, method, Y, G, K, bad, 131, status=False)
    assert rc == 0                                                                 # no status asked for: nothing to report yet


@pytest.mark.parametrize("method", ["null-grid", "null-exact"])
def test_keep_on_device_and_pvals(blmm, method):
    from scipy.stats import chi2
    Y, G, K, _ = make_data(n=79, p=260, m=30, seed=3)
    cond = _cond(np.random.default_rng(2), 30, 260, 1)
    host = blmm.bulkscan_cond(Y, G, K, cond, method=method, output_pvals=True)
    dev = blmm.bulkscan_cond(Y, G, K, cond, method=method, keep_on_device=True)
    mx, arg = dev["L"].colmax()
    assert np.array_equal(mx, host["L"].max(axis=0)) and np.array_equal(arg, host["L"].argmax(axis=0))
    assert np.array_equal(dev["L"].columns([0, 29, 7]), host["L"][:, [0, 29, 7]])
    ref = -chi2.logsf(2.0 * np.log(10.0) * host["L"], 1) / np.log(10.0)
    assert host["Chisq_df"] == 1
    assert np.abs(host["log10Pvals_mat"] - ref).max() <= 1e-9 * np.maximum(1.0, np.abs(ref)).max()


def test_conditioning_guard(blmm):
    """test_gpu_parity's ill-conditioned data (n = 13, fuzz seed 201 case 237) with 6 of its 7 covariates and one conditioning locus
    (c + s = 8).  Which covariate is left out and which locus is taken comes from the ORACLE's own fit: the first (covariate, marker)
    pair in order for which fitlmm on [1, six covariates, g_q] puts a trait at h2 > 1 - 1e-6 with a pivot share below the guard's
    1e-4 -- covariate 0 out, marker 0, trait 7 (share 1.5e-6).  That trait goes through the orthogonalised re-scan and the bound
    holds; with illcond_rho = 2 every trait does."""
    Y, G, K, Cov = _fuzz_case(13, 63, 15, 7, 237, 201)
    Cov, cond = Cov[:, 1:], np.full(15, 0)
    r = blmm.bulkscan_cond(Y, G, K, cond, Cov, method="null-exact", return_status=True)
    print("h2:", r["h2_null_list"], "n_illcond_rescan:", r["status"].n_illcond_rescan)
    assert r["h2_null_list"][7] > 1.0 - 1e-6 and r["status"].n_illcond_rescan > 0
    nrule, _ = assert_cond_close(r["L"], r["h2_null_list"], Y, G, K, cond, assert_lod_close, Covar=Cov)
    assert r["n_rule_zero"] == nrule
    blmm.default_context().set_tuning("illcond_rho", 2)         # every trait through the re-scan (reset by the conftest fixture)
    r2 = blmm.bulkscan_cond(Y, G, K, cond, Cov, method="null-exact", return_status=True)
    assert r2["status"].n_illcond_rescan == 15 and r2["n_rule_zero"] == nrule
    assert_cond_close(r2["L"], r2["h2_null_list"], Y, G, K, cond, assert_lod_close, Covar=Cov)


def test_conditioning_guard_in_the_global_memory_slab(blmm):
    """n = 900 with c + s = 8 (intercept, four covariates, three loci): the (c + s + 2) n doubles of k_cond_qr's basis are 72 KB,
    beyond the 64 KiB that stay in LDS, so every workgroup builds it in its slab of global memory (qr_workspace)."""
    m, p = 12, 130
    Y, G, K, Cov = make_data(n=900, p=p, m=m, seed=90038, ncov=4)
    cond = _cond(np.random.default_rng(903), m, p, 3)
    cond[0] = [5, 77, 120]                                      # one trait with all three
    blmm.default_context().set_tuning("illcond_rho", 2)         # every trait through the re-scan (reset by the conftest fixture)
    r = blmm.bulkscan_cond(Y, G, K, cond, Cov, method="null-exact", return_status=True)
    assert r["status"].n_illcond_rescan == m
    nrule, nband = assert_cond_close(r["L"], r["h2_null_list"], Y, G, K, r["cond"], assert_lod_close, Covar=Cov)
    if nband == 0:
        assert r["n_rule_zero"] == nrule


@pytest.mark.parametrize("method", ["null-grid", "null-exact"])
def test_bxd_shape_peaks(blmm, method):
    n, p, m = 79, 7321, 35554
    Y, G, K = make_data(n=n, p=p, m=m, seed=20241)[:3]
    r = blmm.bulkscan_cond(Y, G, K, "peak", method=method)
    L, cond = r["L"], r["cond"][:, 0]
    assert L.shape == (p, m) and np.all(L[cond, np.arange(m)] == 0.0)
    # host count of the rule's entries: per trait, the markers that are an affine function of its conditioning marker (make_geno
    # repeats a column where no line switches between two markers) -- equal standardised columns up to sign
    Z = G - G.mean(axis=0)
    Z /= np.sqrt((Z * Z).sum(axis=0))
    Z *= np.sign(Z[np.abs(Z).argmax(axis=0), np.arange(p)])
    _, inv, cnt = np.unique(np.round(Z, 9), axis=1, return_inverse=True, return_counts=True)
    same = cnt[inv.ravel()]
    assert r["n_cond_traits"] == m and r["n_cond_dropped"] == 0 and r["n_rule_zero"] == int(same[cond].sum())
    assert int((L == 0.0).sum()) >= r["n_rule_zero"]            # (a few r^2 below 1e-16 round to LOD 0 as well)
    cols = sorted(set(np.linspace(0, m - 1, 58).astype(int).tolist() + [1, 63, 64, 127, 128, m - 2]))[:64]
    assert_cond_close(L, r["h2_null_list"], Y, G, K, r["cond"], assert_lod_close, traits=cols)
    own = bulkscan_cond_ref(Y, G, K, r["cond"], method=method, h2_grid=GRID, traits=cols[:8])[1][cols[:8]]
    if method == "null-grid":
        assert np.array_equal(r["h2_null_list"][cols[:8]], own)
    else:
        assert np.abs(r["h2_null_list"][cols[:8]] - own).max() <= 1e-6
