"""bulkscan_multidf on the GPU: the k-degree-of-freedom scan against bulkscan (k = 1), the NumPy oracle (multidf_ref), the
reference's genotype-probability file format, the rank rule, the conditioning guard, p-values and the resident L."""
import numpy as np
import pytest

from common import DevBuf, assert_lod_close, bxd_kinship, kinship_of, make_data
from multidf_ref import bulkscan_multidf_ref

pytestmark = pytest.mark.gpu


def _founder_data(n, P, k, m, seed, founders=None, ncov=0):
    """Dirichlet founder probabilities (Diversity-Outbred-like): the first k of `founders` (default k + 1) columns of every locus."""
    rng = np.random.default_rng(seed)
    f = founders or k + 1
    prob = rng.dirichlet(np.full(f, 0.7), size=(n, P))[:, :, :k]
    G = prob.reshape(n, P * k)
    K = bxd_kinship() if n == 79 else kinship_of(rng.integers(0, 3, size=(n, 400)).astype(float) / 2.0)
    Y = rng.standard_normal((n, m)) + 5.0
    causal = rng.integers(0, P, size=m)
    beta = rng.standard_normal((k, m)) * 1.5
    for j in range(m):
        if j % 3 == 0:
            Y[:, j] += G[:, causal[j] * k:(causal[j] + 1) * k] @ beta[:, j]
    Cov = rng.standard_normal((n, ncov)) if ncov else None
    if ncov:
        Y += Cov @ rng.standard_normal((ncov, m))
    return Y, G, K, Cov


def _opts_of(case):
    if case == "c1":
        return dict()
    return dict(reml=True, weights=np.random.default_rng(3).uniform(0.5, 2.0, 79), prior_variance=0.8, prior_sample_size=2.0)


@pytest.mark.parametrize("method", ["null-grid", "null-exact"])
@pytest.mark.parametrize("case", ["c1", "c3_reml_weights_prior"])
def test_k1_through_the_new_kernels_equals_bulkscan(blmm, method, case):
    ncov = 0 if case == "c1" else 2
    Y, G, K, Cov = make_data(n=79, p=301, m=45, seed=710 + ncov, ncov=ncov)
    kw = _opts_of(case)
    ref = blmm.bulkscan(Y, G, K, Cov, method=method, **kw)
    got = blmm.bulkscan_multidf(Y, G, K, 1, Cov, method=method, **kw)
    assert np.array_equal(got["h2_null_list"], ref["h2_null_list"])      # bit for bit: the null model does not involve G
    assert_lod_close(got["L"], ref["L"])


CASES = [  # method, k, n, P, m
    ("null-grid", 2, 79, 333, 70), ("null-grid", 3, 200, 129, 37), ("null-grid", 4, 500, 65, 131),
    ("null-grid", 5, 79, 97, 19), ("null-grid", 8, 200, 41, 33), ("null-grid", 2, 79, 1, 9), ("null-grid", 3, 79, 50, 1),
    ("null-exact", 2, 79, 333, 70), ("null-exact", 3, 200, 129, 37), ("null-exact", 4, 500, 65, 23),
    ("null-exact", 2, 79, 1, 9), ("null-exact", 4, 79, 50, 1),
]


@pytest.mark.parametrize("method,k,n,P,m", CASES)
def test_against_the_oracle(blmm, method, k, n, P, m):
    Y, G, K, Cov = _founder_data(n, P, k, m, seed=31 * k + n + P, ncov=1)
    got = blmm.bulkscan_multidf(Y, G, K, k, Cov, method=method)
    ref = bulkscan_multidf_ref(Y, G, K, k, got["h2_null_list"], Covar=Cov)
    assert got["L"].shape == (P, m)
    assert_lod_close(got["L"], ref)


def _geno_csv(path, prob):
    n, pm = prob.shape
    geno = np.empty((n, 2 * pm))
    geno[:, 0::2] = prob
    geno[:, 1::2] = 1.0 - prob
    with open(path, "w") as f:
        f.write(",".join(['"id"'] + [f'"m{j}_{ab}"' for j in range(pm) for ab in "BD"]) + "\n")
        for i in range(n):
            f.write(",".join([f'"BXD{i}"'] + [repr(float(x)) for x in geno[i]]) + "\n")


@pytest.mark.parametrize("method", ["null-grid", "null-exact"])
def test_complement_pairs_from_the_reference_file_format(blmm, tmp_path, method):
    rng = np.random.default_rng(77)
    n, pm, m = 79, 211, 40
    prob = rng.random((n, pm))
    f = tmp_path / "geno_prob.csv"
    _geno_csv(str(f), prob)
    Y, _, K, _ = make_data(n=n, p=20, m=m, seed=78)
    ref = blmm.bulkscan(Y, blmm.readGenoProb_ExcludeComplements(str(f)), K, method=method)
    got = blmm.bulkscan_multidf(Y, blmm.readGenoProb(str(f)), K, 2, method=method)
    assert np.array_equal(got["h2_null_list"], ref["h2_null_list"])
    assert_lod_close(got["L"], ref["L"])


def test_eight_founders_equal_seven(blmm):
    Y, G8, K, _ = _founder_data(79, 60, 8, 25, seed=88, founders=8)
    G7 = G8.reshape(79, 60, 8)[:, :, :7].reshape(79, 60 * 7)
    a = blmm.bulkscan_multidf(Y, G8, K, 8)
    b = blmm.bulkscan_multidf(Y, G7, K, 7)
    assert_lod_close(a["L"], b["L"])
    ref = bulkscan_multidf_ref(Y, G7, K, 7, a["h2_null_list"])
    assert_lod_close(a["L"], ref)


@pytest.mark.parametrize("method", ["null-grid", "null-exact"])
@pytest.mark.parametrize("extra", ["zero", "duplicate", "constant"])
def test_rank_rule_drops_columns_that_add_nothing(blmm, method, extra):
    n, P, m = 79, 90, 21
    Y, G2, K, _ = _founder_data(n, P, 2, m, seed=404)
    X = G2.reshape(n, P, 2)
    add = {"zero": np.zeros((n, P)), "duplicate": X[:, :, 0], "constant": np.full((n, P), 0.37)}[extra]
    G3 = np.concatenate([X[:, :, :1], add[:, :, None], X[:, :, 1:]], axis=2).reshape(n, P * 3)
    a = blmm.bulkscan_multidf(Y, G3, K, 3, method=method)
    b = blmm.bulkscan_multidf(Y, G2, K, 2, method=method)
    assert_lod_close(a["L"], b["L"])


def test_conditioning_guard_collinear_covariates_at_h2_one(blmm):
    """test_gpu_parity.py's ill-conditioned case (tools/fuzz_parity.py seed 201, case 237: n = 13, 7 covariates + intercept,
    traits at the h2 -> 1 boundary, weighted covariates of condition ~2e4): the guard must list those traits and their columns,
    recomputed orthogonalised, must meet the oracle."""
    Y, G, K, Cov = make_data(n=13, p=63, m=15, seed=1000 + 237 + 7919 * 201, ncov=7, bxd=False)
    const = np.ptp(G, axis=0) == 0
    if const.any():
        G = G.copy(); G[:, const] = np.random.default_rng(237).random((13, int(const.sum())))
    got = blmm.bulkscan_multidf(Y, G, K, 3, Cov, method="null-exact", return_status=True)
    h2, st = got["h2_null_list"], got["status"]
    edge = h2 > 1.0 - 1e-6
    assert edge.any() and st.n_illcond_rescan >= edge.sum()
    ref = bulkscan_multidf_ref(Y, G, K, 3, h2, Covar=Cov)
    assert_lod_close(got["L"], ref)


def test_conditioning_guard_every_trait(blmm):
    Y, G, K, Cov = _founder_data(79, 77, 2, 30, seed=515, ncov=2)
    ctx = blmm.default_context()
    ctx.set_tuning("illcond_rho", 2)                    # every trait with c >= 2 on the list (reset by the conftest fixture)
    got = blmm.bulkscan_multidf(Y, G, K, 2, Cov, method="null-exact", return_status=True)
    assert got["status"].n_illcond_rescan == Y.shape[1]
    ref = bulkscan_multidf_ref(Y, G, K, 2, got["h2_null_list"], Covar=Cov)
    assert_lod_close(got["L"], ref)
    ctx.set_tuning("illcond_rho", 0)
    off = blmm.bulkscan_multidf(Y, G, K, 2, Cov, method="null-exact", return_status=True)
    assert off["status"].n_illcond_rescan == 0
    assert_lod_close(off["L"], ref)


def test_pvalues_resident_l_and_the_dev_form(blmm):
    Y, G, K, _ = _founder_data(79, 150, 3, 50, seed=616)
    r = blmm.bulkscan_multidf(Y, G, K, 3, output_pvals=True)
    assert r["Chisq_df"] == 3
    np.testing.assert_allclose(r["log10Pvals_mat"], blmm.lod2log10p(r["L"], 3), rtol=1e-12, atol=1e-13)
    r2 = blmm.bulkscan_multidf(Y, G, K, 3, output_pvals=True, chisq_df=2)
    np.testing.assert_allclose(r2["log10Pvals_mat"], blmm.lod2log10p(r["L"], 2), rtol=1e-12, atol=1e-13)
    kd = blmm.bulkscan_multidf(Y, G, K, 3, keep_on_device=True)
    dl = kd["L"]
    assert dl.shape == (150, 50)
    mx, arg = dl.colmax()
    np.testing.assert_array_equal(mx, r["L"].max(axis=0))
    np.testing.assert_array_equal(arg, r["L"].argmax(axis=0))
    np.testing.assert_array_equal(dl.columns([0, 7, 49]), r["L"][:, [0, 7, 49]])
    thr = float(np.quantile(r["L"], 0.95))
    ii, jj, ll = dl.threshold(thr)
    ei, ej = np.nonzero(r["L"] > thr)
    order = np.lexsort((ei, ej))
    np.testing.assert_array_equal(ii, ei[order]); np.testing.assert_array_equal(jj, ej[order])
    np.testing.assert_array_equal(ll, r["L"][ei[order], ej[order]])
    # the _dev form (device buffers through the HIP runtime: tests/common.py:DevBuf) with an armed -log10 p request, chisq_df 3
    import ctypes as C
    ctx = blmm.default_context()
    n, m, p, P = 79, 50, 450, 150
    dY, dG, dK = DevBuf(Y.T), DevBuf(G.T), DevBuf(K)
    ldL = P + 6                                          # padded leading dimension
    dL, dPv, dh = DevBuf(nbytes=8 * ldL * m), DevBuf(nbytes=8 * ldL * m), DevBuf(nbytes=8 * m)
    grid = np.array([i / 10.0 for i in range(10)])
    o = blmm.api._opts(blmm._lib.BLMM_NULL_GRID)
    ctx.check(ctx.lib.blmm_set_log10p_output(ctx.h, C.c_void_p(dPv.ptr), ldL, 3))
    ctx.check(ctx.lib.blmm_bulkscan_multidf_dev(ctx.h, C.byref(o), C.c_void_p(dY.ptr), n, m, C.c_void_p(dG.ptr), p, 3, None, 0,
                                                C.c_void_p(dK.ptr), None, grid.ctypes.data_as(C.c_void_p), 10, C.c_void_p(dL.ptr), ldL,
                                                C.c_void_p(dh.ptr), None))
    ctx.synchronize()
    Lh = dL.get((m, ldL)).T[:P]
    assert_lod_close(Lh, r["L"])
    np.testing.assert_array_equal(dh.get(m), r["h2_null_list"])
    np.testing.assert_allclose(dPv.get((m, ldL)).T[:P], blmm.lod2log10p(Lh, 3), rtol=1e-12, atol=1e-13)
    for b in (dY, dG, dK, dL, dPv, dh):
        b.free()


@pytest.mark.parametrize("method", ["null-grid", "null-exact"])
def test_bxd_shape(blmm, method):
    n, P, k = 79, 7321, 2
    m = 4096 if method == "null-grid" else 256
    Y, G, K, _ = _founder_data(n, P, k, m, seed=79 + len(method))
    got = blmm.bulkscan_multidf(Y, G, K, k, method=method)
    ref = bulkscan_multidf_ref(Y, G, K, k, got["h2_null_list"])
    assert_lod_close(got["L"], ref)
