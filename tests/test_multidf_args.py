"""bulkscan_multidf without a GPU: every refusal (code and message, before a context exists) and self-checks of the NumPy
oracle (tests/multidf_ref.py) that the GPU tests hold the device against."""
import os
import re

import numpy as np
import pytest

from common import bxd_kinship, make_data
from multidf_ref import _rotate, bulkscan_multidf_ref
from oracle import bulklmm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_context(blmm):
    return blmm.api._default_ctx is None


def test_bulkscan_multidf_is_exported(blmm):
    assert "bulkscan_multidf" in blmm.__all__ and "bulkscan_multidf_dev" in blmm.__all__
    lib = blmm.load()
    for sym in ("blmm_bulkscan_multidf", "blmm_bulkscan_multidf_dev"):
        assert sym in blmm.EXPORTS and hasattr(lib, sym)
    hdr = open(os.path.join(ROOT, "include", "bulklmm_hip.h")).read()
    assert re.search(r"#define BLMM_MULTIDF_TAU 1e-8\b", hdr)
    jl = open(os.path.join(ROOT, "bulklmm.jl_amd", "julia", "BulkLMMHIP.jl")).read()
    assert re.search(r"ccall\(\(:blmm_bulkscan_multidf, libblmm\)", jl)
    assert re.search(r"^export .*\bbulkscan_multidf\b", jl, flags=re.M)


def _refused(blmm, code, msg, *args, **kw):
    before = _no_context(blmm)
    with pytest.raises(blmm.BulkLMMError) as e:
        blmm.bulkscan_multidf(*args, **kw)
    assert e.value.code == code, (e.value.code, e.value.msg)
    assert msg in e.value.msg, e.value.msg
    assert _no_context(blmm) == before


@pytest.mark.parametrize("k,p", [(0, 6), (-1, 6), (4, 6), (5, 12)])
def test_p_not_a_multiple_of_k_is_refused(blmm, k, p):
    _refused(blmm, -2, "multiple of k", np.zeros((6, 2)), np.zeros((6, p)), np.eye(6), k)


@pytest.mark.parametrize("method,k", [("null-grid", 9), ("null-exact", 5), ("null-exact", 8)])
def test_k_above_the_method_limit_is_refused(blmm, method, k):
    _refused(blmm, -10, "takes 1 <= k <= %d" % (8 if method == "null-grid" else 4), np.zeros((12, 2)), np.zeros((12, 2 * k)),
             np.eye(12), k, method=method)


def test_alt_grid_and_unknown_methods_are_refused(blmm):
    _refused(blmm, -10, "alt-grid is not supported", np.zeros((6, 2)), np.zeros((6, 4)), np.eye(6), 2, method="alt-grid")
    _refused(blmm, -5, "Unknown method", np.zeros((6, 2)), np.zeros((6, 4)), np.eye(6), 2, method="grid")


def test_more_than_eight_covariates_are_refused(blmm):
    n = 20
    _refused(blmm, -10, "more than 8 null covariates", np.zeros((n, 2)), np.zeros((n, 4)), np.eye(n), 2, np.zeros((n, 8)))
    _refused(blmm, -10, "more than 8 null covariates", np.zeros((n, 2)), np.zeros((n, 4)), np.eye(n), 2, np.zeros((n, 9)),
             addIntercept=False)


def test_more_than_2048_individuals_is_refused(blmm):
    n = 2049
    _refused(blmm, -10, "2048", np.zeros((n, 1)), np.zeros((n, 2)), np.eye(n), 2)


@pytest.mark.parametrize("case", ["G_rows", "K_rows", "Covar_rows", "weights_len"])
def test_shape_mismatches_are_refused(blmm, case):
    n = 6
    Y = np.zeros((n, 2)); G = np.zeros((n, 4)); K = np.eye(n); kw = {}
    if case == "G_rows":
        G = np.zeros((n + 1, 4))
    elif case == "K_rows":
        K = np.eye(n + 1)[:, :n]
    elif case == "Covar_rows":
        kw["Covar"] = np.zeros((n - 1, 1))
    else:
        kw["weights"] = np.ones(n + 1)
    _refused(blmm, -2, "Dimension mismatch.", Y, G, K, 2, **kw)


# ---- the oracle --------------------------------------------------------------------------------------------------------------
def test_oracle_k1_equals_the_1df_oracle():
    Y, G, K, Cov = make_data(n=40, p=57, m=9, seed=4242, ncov=2, bxd=False)
    ref = O.bulkscan(Y, G, K, Covar=Cov, method="null-grid")
    got = bulkscan_multidf_ref(Y, G, K, 1, ref["h2_null_list"], Covar=Cov)
    np.testing.assert_allclose(got, ref["L"], rtol=1e-9, atol=1e-10)
    ex = O.bulkscan_null(Y, G, K, Covar=Cov)
    got = bulkscan_multidf_ref(Y, G, K, 1, ex.h2_null_list, Covar=Cov)
    np.testing.assert_allclose(got, ex.L, rtol=1e-9, atol=1e-10)


def test_oracle_complement_column_changes_nothing():
    rng = np.random.default_rng(11)
    Y, _, K, _ = make_data(n=30, p=10, m=5, seed=12, bxd=False)
    g = rng.random((30, 17))
    G2 = np.stack([g, 1.0 - g], axis=2).reshape(30, 34)
    h2 = rng.uniform(0, 0.9, 5)
    a = bulkscan_multidf_ref(Y, G2, K, 2, h2)
    b = bulkscan_multidf_ref(Y, g, K, 1, h2)
    np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-10)


def test_oracle_lod_is_invariant_under_mixing_a_locus():
    rng = np.random.default_rng(13)
    n, P, k = 35, 12, 3
    Y, _, K, Cov = make_data(n=n, p=10, m=6, seed=14, ncov=1, bxd=False)
    G = rng.random((n, P * k))
    A = rng.standard_normal((k, k)) + 3 * np.eye(k)
    Gm = (G.reshape(n, P, k) @ A).reshape(n, P * k)
    h2 = rng.uniform(0, 0.9, 6)
    np.testing.assert_allclose(bulkscan_multidf_ref(Y, Gm, K, k, h2, Covar=Cov), bulkscan_multidf_ref(Y, G, K, k, h2, Covar=Cov),
                               rtol=1e-9, atol=1e-10)


def test_oracle_tau_is_a_switch():
    """A complement perturbed by 1e-4 N(0, 1) has rho ~ 1e-8 .. 1e-9 (n = 30): kept at tau = 1e-10, dropped at 1e-6, where L is the
    scan of the other column alone."""
    rng = np.random.default_rng(15)
    n, P = 30, 11
    Y, _, K, _ = make_data(n=n, p=10, m=4, seed=16, bxd=False)
    g = rng.random((n, P))
    G2 = np.stack([g, 1.0 - g + 1e-4 * rng.standard_normal((n, P))], axis=2).reshape(n, 2 * P)
    h2 = rng.uniform(0, 0.9, 4)
    L1 = bulkscan_multidf_ref(Y, g, K, 1, h2)
    lo, rho = bulkscan_multidf_ref(Y, G2, K, 2, h2, tau=1e-10, return_rho=True)
    hi = bulkscan_multidf_ref(Y, G2, K, 2, h2, tau=1e-6)
    assert rho.shape == (P, 2, 4) and (rho[:, 0] > 0.1).all() and ((rho[:, 1] > 1e-10) & (rho[:, 1] < 1e-6)).all()
    np.testing.assert_allclose(hi, L1, rtol=1e-9, atol=1e-10)
    assert (lo > L1 + 1e-6).all()                       # the kept column explains a little more of every trait
    np.testing.assert_array_equal(bulkscan_multidf_ref(Y, G2, K, 2, h2), bulkscan_multidf_ref(Y, G2, K, 2, h2, tau=1e-8))


def test_oracle_rho_of_an_exact_complement_is_at_rounding_level():
    rng = np.random.default_rng(17)
    n, P = 79, 25
    Y, _, K, Cov = make_data(n=n, p=10, m=6, seed=18, ncov=2)
    g = rng.random((n, P))
    G2 = np.stack([g, 1.0 - g], axis=2).reshape(n, 2 * P)
    _, rho = bulkscan_multidf_ref(Y, G2, K, 2, rng.uniform(0, 0.9, 6), Covar=Cov, return_rho=True)
    assert (rho[:, 0] > 1e-2).all() and (rho[:, 1] < 1e-25).all(), float(rho[:, 1].max())


def test_oracle_r2_form_agrees_with_least_squares_at_strong_signals():
    """The oracle's L = -(n/2) log10(1 - |Q'e|^2) against the rss form u = |r1|^2 / |r0|^2 (np.linalg.lstsq on the weighted design
    with and without the locus), on traits y = 10 + X_l beta + sigma e with sigma log-uniform: LODs up to ~270 at n = 79, k = 3.
    1 - R^2 cancels: its error grows as 1 / u.  Both forms agree to 1e-9 relative up to LOD 290 (worst seen ~5e-10 near 270, ~1e-12
    at 200), so the oracle holds the device's 1e-6 bound with a wide margin out to the strong-signal cap (LOD 238)."""
    rng = np.random.default_rng(9100)
    n, P, k, m = 79, 40, 3, 96
    G = rng.dirichlet(np.full(k + 1, 0.7), size=(n, P))[:, :, :k].reshape(n, P * k)
    K = bxd_kinship()
    Y = rng.standard_normal((n, m))
    q = rng.integers(0, P, m)
    sig = 2.0 ** rng.uniform(-12, 0, m)
    for t in range(m):
        Y[:, t] = 10 + G[:, q[t] * k:(q[t] + 1) * k] @ rng.standard_normal(k) * 2 + sig[t] * Y[:, t]
    h2 = np.array([0.0, 0.3, 0.7])[np.arange(m) % 3]
    L = bulkscan_multidf_ref(Y, G, K, k, h2)
    Y0, Z0, X0, lam = _rotate(Y, G, K, None, True, None, "eigen")
    Lls = np.empty_like(L)
    for h in np.unique(h2):
        idx = np.flatnonzero(h2 == h)
        s = np.sqrt(np.abs(O.makeweights(h, lam)))
        Zs, ys = s[:, None] * Z0, s[:, None] * Y0[:, idx]
        r0 = ys - Zs @ np.linalg.lstsq(Zs, ys, rcond=None)[0]
        for l in range(P):
            A = np.hstack([Zs, s[:, None] * X0[:, l * k:(l + 1) * k]])
            r1 = ys - A @ np.linalg.lstsq(A, ys, rcond=None)[0]
            Lls[l, idx] = -(n / 2.0) * np.log10(np.sum(r1 ** 2, axis=0) / np.sum(r0 ** 2, axis=0))
    ok = L <= 290.0
    assert (L[ok] > 200.0).sum() >= 10 and ok.sum() >= 0.95 * L.size
    np.testing.assert_allclose(L[ok], Lls[ok], rtol=1e-9, atol=1e-10)
