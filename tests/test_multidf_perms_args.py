"""bulkscan_multidf_perms without a GPU: the entry points are exported at every layer, every refusal is raised with its code by the
host mirror before a context exists, and the NumPy oracle (tests/multidf_perms_ref.py) agrees with bulkscan_multidf's at b = 0."""
import os
import re

import numpy as np
import pytest

from common import make_data
from multidf_perms_ref import bulkscan_multidf_perms_ref
from multidf_ref import bulkscan_multidf_ref
from oracle import bulklmm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_context(blmm):
    return blmm.api._default_ctx is None


def test_bulkscan_multidf_perms_is_exported(blmm):
    assert "bulkscan_multidf_perms" in blmm.__all__ and "bulkscan_multidf_perms_dev" in blmm.__all__
    assert callable(blmm.bulkscan_multidf_perms) and callable(blmm.bulkscan_multidf_perms_dev)
    lib = blmm.load()
    for sym in ("blmm_bulkscan_multidf_perms", "blmm_bulkscan_multidf_perms_dev"):
        assert sym in blmm.EXPORTS and hasattr(lib, sym)
    hdr = open(os.path.join(ROOT, "include", "bulklmm_hip.h")).read()
    assert re.search(r"^int blmm_bulkscan_multidf_perms\(", hdr, flags=re.M)
    assert re.search(r"^int blmm_bulkscan_multidf_perms_dev\(", hdr, flags=re.M)
    assert re.search(r"#define BLMM_VERSION 210\b", hdr)                      # appended to the comment only
    jl = open(os.path.join(ROOT, "bulklmm.jl_amd", "julia", "BulkLMMHIP.jl")).read()
    assert re.search(r"ccall\(\(:blmm_bulkscan_multidf_perms, libblmm\)", jl)
    assert re.search(r"^export .*\bbulkscan_multidf_perms\b", jl, flags=re.M)


def _refused(blmm, code, msg, *args, **kw):
    before = _no_context(blmm)
    with pytest.raises(blmm.BulkLMMError) as e:
        blmm.bulkscan_multidf_perms(*args, **kw)
    assert e.value.code == code, (e.value.code, e.value.msg)
    assert msg in e.value.msg, e.value.msg
    assert _no_context(blmm) == before


@pytest.mark.parametrize("k,p", [(0, 6), (-1, 6), (4, 6), (5, 12)])
def test_p_not_a_multiple_of_k_is_refused(blmm, k, p):
    _refused(blmm, -2, "multiple of k", np.zeros((6, 2)), np.zeros((6, p)), np.eye(6), k, nperms=3)


def test_k_above_eight_is_refused(blmm):
    _refused(blmm, -10, "takes 1 <= k <= 8", np.zeros((12, 2)), np.zeros((12, 18)), np.eye(12), 9, nperms=3)


def test_more_than_eight_covariates_are_refused(blmm):
    n = 20
    _refused(blmm, -10, "more than 8 null covariates", np.zeros((n, 2)), np.zeros((n, 4)), np.eye(n), 2, np.zeros((n, 8)), nperms=3)
    _refused(blmm, -10, "more than 8 null covariates", np.zeros((n, 2)), np.zeros((n, 4)), np.eye(n), 2, np.zeros((n, 9)), nperms=3,
             addIntercept=False)


def test_too_many_permutations_are_refused(blmm):
    _refused(blmm, -10, "more than 16384 permutations", np.zeros((6, 2)), np.zeros((6, 4)), np.eye(6), 2, nperms=16385)


def test_more_than_2048_individuals_is_refused(blmm):
    n = 2049
    _refused(blmm, -10, "2048", np.zeros((n, 1)), np.zeros((n, 2)), np.eye(n), 2, nperms=2)


def test_negative_nperms_is_refused(blmm):
    _refused(blmm, -9, "The required number of permutations must be a positive integer.", np.zeros((6, 2)), np.zeros((6, 4)),
             np.eye(6), 2, nperms=-1)


def test_bad_levels_and_perm_idx_entries_are_refused(blmm):
    Y = np.zeros((6, 2)); G = np.zeros((6, 4)); K = np.eye(6)
    _refused(blmm, -1, "0 .. 64 threshold levels", Y, G, K, 2, nperms=3, signif_level=np.linspace(0.01, 0.9, 65))
    for bad in (-1, 6):
        pidx = np.tile(np.arange(6, dtype=np.int32)[:, None], (1, 3))
        pidx[2, 1] = bad
        _refused(blmm, -1, "perm_idx entries must lie in 0 .. n - 1", Y, G, K, 2, nperms=3, perm_idx=pidx)


@pytest.mark.parametrize("case", ["G_rows", "K_rows", "Covar_rows", "weights_len", "perm_idx_shape"])
def test_shape_mismatches_are_refused(blmm, case):
    n = 6
    Y = np.zeros((n, 2)); G = np.zeros((n, 4)); K = np.eye(n); kw = {"nperms": 4}
    if case == "G_rows":
        G = np.zeros((n + 1, 4))
    elif case == "K_rows":
        K = np.eye(n + 1)[:, :n]
    elif case == "Covar_rows":
        kw["Covar"] = np.zeros((n - 1, 1))
    elif case == "weights_len":
        kw["weights"] = np.ones(n + 1)
    else:
        kw["perm_idx"] = np.zeros((n, 3), dtype=np.int32)
    _refused(blmm, -2, "Dimension mismatch.", Y, G, K, 2, **kw)


# ---- the oracle --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,ncov,weighted", [(1, 0, False), (2, 2, True), (3, 1, False)])
def test_oracle_unpermuted_column_is_the_multidf_oracle(k, ncov, weighted):
    """At b = 0 the permutation oracle is bulkscan_multidf_ref (v_0 = r0 is orthogonal to the weighted covariates, so both
    denominators are |r0|^2), and an identity permutation repeats that column."""
    rng = np.random.default_rng(90 + k)
    n, P, m, nperms = 37, 23, 5, 4
    Y, _, K, Cov = make_data(n=n, p=10, m=m, seed=91 + k, ncov=ncov, bxd=False)
    G = rng.dirichlet(np.full(k + 1, 0.7), size=(n, P))[:, :, :k].reshape(n, P * k)
    w = rng.uniform(0.5, 2.0, n) if weighted else None
    h2 = rng.uniform(0.0, 0.9, m)
    pidx = O.make_perm_idx(n, nperms, 5)
    pidx[:, 2] = np.arange(n)
    got = bulkscan_multidf_perms_ref(Y, G, K, k, h2, pidx, Covar=Cov, weights=w)
    ref = bulkscan_multidf_ref(Y, G, K, k, h2, Covar=Cov, weights=w)
    for j in range(m):
        assert got[j].shape == (P, nperms + 1)
        np.testing.assert_allclose(got[j][:, 0], ref[:, j], rtol=1e-9, atol=1e-10)
        np.testing.assert_array_equal(got[j][:, 3], got[j][:, 0])
        assert not np.allclose(got[j][:, 1], got[j][:, 0])


def test_oracle_k1_is_the_1df_permutation_oracle():
    """k = 1 against scan_perms_lite as the 1-df oracle states it (shared rotation and h2)."""
    n, nperms = 31, 6
    Y, G, K, _ = make_data(n=n, p=29, m=3, seed=123, bxd=False)
    pidx = O.make_perm_idx(n, nperms, 9)
    h2 = np.array([0.1, 0.5, 0.8])
    got = bulkscan_multidf_perms_ref(Y, G, K, 1, h2, pidx)
    for j in range(3):
        ref = O.scan(Y[:, j], G, K, permutation_test=True, nperms=nperms, perm_idx=pidx, h2_override=h2[j])
        np.testing.assert_allclose(got[j][:, 1:], ref["L_perms"], rtol=1e-9, atol=1e-10)
        np.testing.assert_allclose(got[j][:, 0], ref["lod"], rtol=1e-9, atol=1e-10)
