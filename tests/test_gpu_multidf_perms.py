"""bulkscan_multidf_perms on the GPU: permutation thresholds of the k-degree-of-freedom scan against the NumPy oracle
(multidf_perms_ref), against bulkscan_perms (k = 1) and bulkscan_multidf (b = 0), across slot edges, panel routes and trait chunks,
its summaries, its device form and one BXD-width pass."""
import os
import subprocess
import sys

import numpy as np
import pytest

from common import ATOL, RTOL, assert_lod_close, make_data
from multidf_perms_ref import bulkscan_multidf_perms_ref
from multidf_ref import TAU
from oracle import bulklmm_oracle as O
from test_gpu_multidf import _founder_data

pytestmark = pytest.mark.gpu

SIG = (0.10, 0.05)
PLAIN = dict()
FULL = dict(reml=True, prior_variance=0.8, prior_sample_size=2.0)


def _weights(n, seed=3):
    return np.random.default_rng(seed).uniform(0.5, 2.0, n)


def _pvals(mp, lm):
    hit = (mp >= lm[None, :]) & (mp != -np.inf)
    return (1.0 + hit.sum(axis=0)) / (mp.shape[0] + 1.0)


def _quantiles(mp, probs):
    """k_quantiles' rule (Julia's default type 7) on each column."""
    nperms, m = mp.shape
    out = np.empty((len(probs), m))
    s = np.sort(mp, axis=0)
    for t, q in enumerate(probs):
        h = (nperms - 1) * min(max(q, 0.0), 1.0)
        lo = int(np.floor(h))
        hi = min(lo + 1, nperms - 1)
        out[t] = s[lo] + (h - lo) * (s[hi] - s[lo])
    return out


def _device_rotation(blmm, Y, G, K, Cov, weights):
    """(Y0, Z0, X0, lam) in the device's eigenbasis (a permutation acts on its coordinates: multidf_perms_ref), from the prescaled
    data as the oracle prescales it."""
    n = Y.shape[0]
    cov = np.ones((n, 1)) if Cov is None else np.hstack([np.ones((n, 1)), Cov])
    Y_st, G_st, cov_st, K_st, _ = O._apply_weights(Y, G, cov, K, weights, False)
    Y0, X0, lam = blmm.transform_rotation(Y_st, np.hstack([cov_st, G_st]), K_st, addIntercept=False)
    c = cov.shape[1]
    return Y0, X0[:, :c], X0[:, c:], lam


def _check_against_oracle(blmm, res, Y, G, K, k, pidx, traits, Cov=None, weights=None):
    """max_perms, lod_max and lod_argmax of `traits` against the oracle's column maxima at the device's h2 and in the device's
    eigenbasis, after asserting that every rank decision of those traits is decisive (no entry is left out)."""
    ref, rho = bulkscan_multidf_perms_ref(Y, G, K, k, res["h2_null"], pidx, traits=traits, return_rho=True,
                                          rotation=_device_rotation(blmm, Y, G, K, Cov, weights))
    for j in traits:
        assert ((rho[j] > 100 * TAU) | (rho[j] < TAU / 100)).all(), f"trait {j}: a rank decision at the threshold; change the seed"
        Lj = ref[j]
        assert np.isfinite(Lj).all()
        assert_lod_close(res["lod_max"][j], Lj[:, 0].max(), what=f"lod_max[{j}]")
        assert_lod_close(res["max_perms"][:, j], Lj[:, 1:].max(axis=0), what=f"max_perms[:, {j}]")
        a, b = int(res["lod_argmax"][j]), int(np.argmax(Lj[:, 0]))
        assert 0 <= a < Lj.shape[0]
        assert a == b or abs(Lj[a, 0] - Lj[b, 0]) <= RTOL * abs(Lj[b, 0]) + ATOL, (j, a, b, Lj[a, 0], Lj[b, 0])


# ---- 1. oracle parity: k, covariates / weights / REML / prior, the slot edges; n = 79 takes the one-thread panel route ----------
@pytest.mark.parametrize("P", [63, 64, 65, 129])
@pytest.mark.parametrize("case", ["c1", "c3_reml_weights_prior"])
@pytest.mark.parametrize("k", [2, 5, 8])
def test_against_the_oracle(blmm, k, case, P):
    n, m, nperms = 79, 7, 37                                       # m (nperms + 1) = 266 columns: no multiple of 4 TJ (64 or 32)
    full = case != "c1"
    Y, G, K, Cov = _founder_data(n, P, k, m, seed=1000 * k + P + (7 if full else 0), ncov=2 if full else 0)
    w = _weights(n) if full else None
    pidx = O.make_perm_idx(n, nperms, 41 + k)
    res = blmm.bulkscan_multidf_perms(Y, G, K, k, Cov, nperms=nperms, perm_idx=pidx, signif_level=SIG, weights=w,
                                      **(FULL if full else PLAIN))
    assert res["max_perms"].shape == (nperms, m) and res["thresholds"].shape == (2, m)
    _check_against_oracle(blmm, res, Y, G, K, k, pidx, range(m), Cov, w)
    np.testing.assert_array_equal(res["pvals_perm"], _pvals(res["max_perms"], res["lod_max"]))


# ---- 2. dropped columns ---------------------------------------------------------------------------------------------------------
def test_complement_pairs_equal_the_single_column_call(blmm):
    rng = np.random.default_rng(202)
    n, P, m, nperms = 79, 97, 9, 25
    Y, _, K, _ = make_data(n=n, p=20, m=m, seed=203)
    x = rng.random((n, P))
    G2 = np.stack([x, 1.0 - x], axis=2).reshape(n, 2 * P)
    pidx = O.make_perm_idx(n, nperms, 204)
    a = blmm.bulkscan_multidf_perms(Y, G2, K, 2, nperms=nperms, perm_idx=pidx)
    b = blmm.bulkscan_multidf_perms(Y, x, K, 1, nperms=nperms, perm_idx=pidx)
    np.testing.assert_array_equal(a["h2_null"], b["h2_null"])
    assert_lod_close(a["lod_max"], b["lod_max"], what="lod_max")
    assert_lod_close(a["max_perms"], b["max_perms"], what="max_perms")


@pytest.mark.parametrize("k", [1, 3])
def test_constant_loci_have_lod_zero_in_every_permutation(blmm, k):
    n, P, m, nperms = 79, 5, 4, 12
    Y, _, K, _ = make_data(n=n, p=20, m=m, seed=210)
    G = np.tile(np.linspace(0.1, 0.9, P * k)[None, :], (n, 1))
    res = blmm.bulkscan_multidf_perms(Y, G, K, k, nperms=nperms, rndseed=4, return_status=True)
    assert (res["lod_max"] == 0.0).all() and (res["max_perms"] == 0.0).all()
    assert (res["lod_argmax"] == 0).all()                            # every locus ties at 0: the lowest index
    assert res["status"].n_nan_lod == 0 and res["status"].n_zero_norm == 0


# ---- 3. k = 1 against bulkscan_perms: the same null fit and the same permutation set from the seed ---------------------------
@pytest.mark.parametrize("ncov", [0, 2])
def test_k1_equals_bulkscan_perms(blmm, ncov):
    Y, G, K, Cov = make_data(n=79, p=301, m=11, seed=330 + ncov, ncov=ncov)
    const = np.ptp(G, axis=0) == 0
    G[:, const] = np.random.default_rng(331).random((79, int(const.sum())))
    nperms = 33
    ref = blmm.bulkscan_perms(Y, G, K, Cov, nperms=nperms, rndseed=19)
    got = blmm.bulkscan_multidf_perms(Y, G, K, 1, Cov, nperms=nperms, rndseed=19)
    np.testing.assert_array_equal(got["h2_null"], ref["h2_null"])
    np.testing.assert_array_equal(got["sigma2_e"], ref["sigma2_e"])
    assert_lod_close(got["lod_max"], ref["lod_max"], what="lod_max")
    assert_lod_close(got["max_perms"], ref["max_perms"], what="max_perms")
    other = blmm.bulkscan_multidf_perms(Y, G, K, 1, Cov, nperms=nperms, rndseed=20)
    assert not np.array_equal(other["max_perms"], got["max_perms"])  # (the seed matters: the agreement above is the same set)


# ---- 4. b = 0 against bulkscan_multidf's null-exact scan ----------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 4])
def test_unpermuted_column_equals_multidf_null_exact(blmm, k):
    Y, G, K, Cov = _founder_data(79, 130, k, 17, seed=440 + k, ncov=1)
    prior = dict(prior_variance=1.0, prior_sample_size=0.1)
    ref = blmm.bulkscan_multidf(Y, G, K, k, Cov, method="null-exact", **prior)
    got = blmm.bulkscan_multidf_perms(Y, G, K, k, Cov, nperms=5, rndseed=1, **prior)
    np.testing.assert_allclose(got["h2_null"], ref["h2_null_list"], rtol=0, atol=1e-7)   # (bulkscan_perms' null fit, not multidf's bits)
    assert_lod_close(got["lod_max"], ref["L"].max(axis=0), what="lod_max")
    a, b = got["lod_argmax"], ref["L"].argmax(axis=0)
    cols = np.arange(17)
    assert_lod_close(ref["L"][a, cols], ref["L"][b, cols], what="L at the two arg-maxima")


# ---- 5. large n (the multi-kernel panel route) and trait chunks -----------------------------------------------------------------
def test_large_n_and_chunks(blmm):
    n, k, P, m, nperms = 300, 3, 111, 13, 20
    Y, G, K, Cov = _founder_data(n, P, k, m, seed=550, ncov=1)
    ctx = blmm.default_context()
    one = blmm.bulkscan_multidf_perms(Y, G, K, k, Cov, nperms=nperms, rndseed=3, ctx=ctx)
    ctx.set_tuning("bulk_perm_cols", 5 * (nperms + 1))              # chunks of 5, 5 and 3 traits
    try:
        many = blmm.bulkscan_multidf_perms(Y, G, K, k, Cov, nperms=nperms, rndseed=3, ctx=ctx)
    finally:
        ctx.set_tuning("defaults", 0)
    for key in ("h2_null", "sigma2_e", "lod_max", "lod_argmax", "max_perms", "thresholds", "pvals_perm"):
        np.testing.assert_array_equal(one[key], many[key], err_msg=key)
    pidx = O.make_perm_idx(n, nperms, 8)
    res = blmm.bulkscan_multidf_perms(Y, G, K, k, Cov, nperms=nperms, perm_idx=pidx, ctx=ctx)
    np.testing.assert_array_equal(res["lod_max"], one["lod_max"])   # the unpermuted column does not depend on the set
    _check_against_oracle(blmm, res, Y, G, K, k, pidx, [0, 6, m - 1], Cov)


def test_n1000_eight_covariates(blmm):
    """k_mdf_table's weights and covariates (n (1 + c) doubles = 72 KB) take the dynamic LDS beyond 48 KB."""
    n, k, P, m, nperms = 1000, 2, 70, 5, 6
    Y, G, K, Cov = _founder_data(n, P, k, m, seed=560, ncov=7)
    pidx = O.make_perm_idx(n, nperms, 9)
    res = blmm.bulkscan_multidf_perms(Y, G, K, k, Cov, nperms=nperms, perm_idx=pidx)
    _check_against_oracle(blmm, res, Y, G, K, k, pidx, [0, 2, 4], Cov)


# ---- 6. summaries -----------------------------------------------------------------------------------------------------------
def test_summaries(blmm):
    n, k, P, m, nperms = 79, 2, 70, 6, 30
    Y, G, K, _ = _founder_data(n, P, k, m, seed=660)
    pidx = O.make_perm_idx(n, nperms, 21)
    pidx[:, 0] = np.arange(n)
    pidx[:, 5] = np.arange(n)
    res = blmm.bulkscan_multidf_perms(Y, G, K, k, nperms=nperms, perm_idx=pidx, signif_level=SIG)
    mp, lm = res["max_perms"], res["lod_max"]
    assert (mp[0] == lm).all() and (mp[5] == lm).all()              # identity permutations reproduce the peak exactly
    np.testing.assert_array_equal(res["pvals_perm"], _pvals(mp, lm))
    assert (res["pvals_perm"] >= 3.0 / (nperms + 1)).all()          # ... and both count
    np.testing.assert_allclose(res["thresholds"], _quantiles(mp, 1.0 - np.asarray(SIG)), rtol=1e-12, atol=0)
    # no permutations: the fit and the peaks, thresholds and p-values NaN
    zero = blmm.bulkscan_multidf_perms(Y, G, K, k, nperms=0)
    assert zero["max_perms"].shape == (0, m)
    assert np.isnan(zero["thresholds"]).all() and np.isnan(zero["pvals_perm"]).all()
    np.testing.assert_array_equal(zero["lod_max"], lm)
    np.testing.assert_array_equal(zero["lod_argmax"], res["lod_argmax"])
    # no loci: nothing compares
    none = blmm.bulkscan_multidf_perms(Y, np.zeros((n, 0)), K, k, nperms=4, rndseed=1)
    assert (none["lod_max"] == -np.inf).all() and (none["lod_argmax"] == -1).all() and (none["max_perms"] == -np.inf).all()
    np.testing.assert_array_equal(none["h2_null"], res["h2_null"])
    # every locus twice (the copies sit in the same and in later 64-locus slots): ties go to the lowest index
    dup = blmm.bulkscan_multidf_perms(Y, np.hstack([G, G]), K, k, nperms=4, rndseed=1)
    assert ((dup["lod_argmax"] >= 0) & (dup["lod_argmax"] < P)).all()
    np.testing.assert_array_equal(dup["lod_argmax"], res["lod_argmax"])
    assert_lod_close(dup["lod_max"], lm, what="lod_max with every locus duplicated")


# ---- 7. the device form, on torch tensors in a fresh process -------------------------------------------------------------------
def test_dev_form_in_its_own_process():
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "helpers", "multidf_perms_dev_check.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "multidf_perms_dev ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- 8. one pass at the BXD width -------------------------------------------------------------------------------------------
def test_bxd_width(blmm):
    n, P, k, m, nperms = 79, 7321, 2, 8, 100
    Y, G, K, _ = _founder_data(n, P, k, m, seed=880)
    pidx = O.make_perm_idx(n, nperms, 88)
    res = blmm.bulkscan_multidf_perms(Y, G, K, k, nperms=nperms, perm_idx=pidx)
    assert np.isfinite(res["max_perms"]).all()
    _check_against_oracle(blmm, res, Y, G, K, k, pidx, [0, 3, m - 1])
    np.testing.assert_array_equal(res["pvals_perm"], _pvals(res["max_perms"], res["lod_max"]))
