"""bulkscan_effects on the GPU against the NumPy oracle (tests/effects_ref.py: oracle.bulklmm_oracle's wls on the rotated data) and
against the scans it sits beside: lod[t] is bulkscan's / bulkscan_multidf's L[locus, trait], h2_null_list theirs bit for bit.

Criterion: the project's own (tests/common.py), |d| <= 1e-6 |ref| + atol, with atol = 1e-10 for lod and, for beta / se / sigma2,
1e-10 x the largest |ref| of that output in the call (they carry the traits' units: a fixed absolute floor would mean nothing).
Rank rule: `accepted` equals the oracle's except where the oracle's pivot ratio rho lies in [tau / 100, 100 tau]; such tests are
left out of the value comparison, and every case asserts that at most 1 % of its tests are."""
import os
import subprocess
import sys

import numpy as np
import pytest

from common import ATOL, RTOL, assert_lod_close
from effects_cases import GRID, PARITY, collinear_case, rank_rule_case
from effects_ref import effects_ref
from multidf_ref import TAU

pytestmark = pytest.mark.gpu


def _run(blmm, c, locus=None, trait=None, **extra):
    return blmm.bulkscan_effects(c["Y"], c["G"], c["K"], c["Cov"], k=c["k"], locus=c["locus"] if locus is None else locus,
                                 trait=c["trait"] if trait is None else trait, method=c["method"], **c["kw"], **extra)


def _ref(c, h2, locus=None, trait=None):
    return effects_ref(c["Y"], c["G"], c["K"], c["k"], c["locus"] if locus is None else locus, c["trait"] if trait is None else trait,
                       h2, Covar=c["Cov"], **c["kw"])


def _close(got, ref, what, scaled=True):
    ref = np.asarray(ref)
    atol = ATOL * (float(np.max(np.abs(ref))) if scaled and ref.size else 1.0)
    err = np.abs(np.asarray(got) - ref)
    print(f"{what}: max |d| {float(err.max()) if err.size else 0.0:.3e}, max |ref| {float(np.abs(ref).max()) if ref.size else 0.0:.3e}, "
          f"max |d| / (rtol |ref| + atol) {float(np.max(err / (RTOL * np.abs(ref) + atol))) if err.size else 0.0:.3e}")
    assert_lod_close(got, ref, atol=atol, what=what)


def _check(got, ref, what):
    """The value comparison of one call, outside the rank rule's band."""
    band = ((ref.rho >= TAU / 100) & (ref.rho <= 100 * TAU)).any(axis=1)
    print(f"{what}: {int(band.sum())} of {band.size} tests in the rank rule's band")
    assert band.mean() <= 0.01
    ok = ~band
    np.testing.assert_array_equal(got["accepted"][ok], ref.accepted[ok])
    _close(got["beta"][ok], ref.beta[ok], what + " beta")
    _close(got["se"][ok], ref.se[ok], what + " se")
    _close(got["sigma2"][ok], ref.sigma2[ok], what + " sigma2")
    _close(got["lod"][ok], ref.lod[ok], what + " lod", scaled=False)
    dropped = (ref.accepted[ok, None] >> np.arange(ref.beta.shape[1])) & 1 == 0
    assert np.all(got["beta"][ok][dropped] == 0.0) and np.all(got["se"][ok][dropped] == 0.0)
    return ok


@pytest.mark.parametrize("name", list(PARITY))
def test_parity_with_the_oracle_and_the_scans(blmm, name):
    c = PARITY[name]()
    k, method = c["k"], c["method"]
    got = _run(blmm, c, return_status=True)
    assert got["status"].n_nan_lod == 0
    scan = blmm.bulkscan(c["Y"], c["G"][:, ::k], c["K"], c["Cov"], method=method, **c["kw"])      # (the null model does not involve G)
    assert np.array_equal(got["h2_null_list"], scan["h2_null_list"])
    ref = _ref(c, got["h2_null_list"])
    ok = _check(got, ref, name)
    if k == 1:
        _close(got["lod"][ok], scan["L"][c["locus"], c["trait"]][ok], name + " lod vs bulkscan", scaled=False)
    elif method == "null-grid" or k <= blmm._lib.BLMM_MULTIDF_MAX_K_EXACT:
        md = blmm.bulkscan_multidf(c["Y"], c["G"], c["K"], k, c["Cov"], method=method, **c["kw"])
        assert np.array_equal(got["h2_null_list"], md["h2_null_list"])
        _close(got["lod"][ok], md["L"][c["locus"], c["trait"]][ok], name + " lod vs bulkscan_multidf", scaled=False)


@pytest.mark.parametrize("method", ["null-grid", "null-exact"])
def test_k1_lod_is_the_t_statistic(blmm, method):
    """k = 1, ML, no prior: sigma2 = rss1 / n and rss0 / rss1 = 1 + t^2 / n with t = beta / se, so lod = (n / 2) log10(1 + t^2 / n);
    the sign of beta is the sign of x~_res' e~.  This holds se to the LOD without the oracle's inverse."""
    c = PARITY["grid_k1_n79_c1" if method == "null-grid" else "exact_k1_n79_c2_weights"]()
    n = c["Y"].shape[0]
    got = _run(blmm, c, prior_variance=0.0, prior_sample_size=0.0)
    t = got["beta"][:, 0] / got["se"][:, 0]
    _close(0.5 * n * np.log10(1.0 + t * t / n), got["lod"], "lod from t", scaled=False)
    ref = _ref(c, got["h2_null_list"])
    assert np.all(ref.xe[:, 0] != 0.0)
    np.testing.assert_array_equal(np.sign(got["beta"][:, 0]), np.sign(ref.xe[:, 0]))


@pytest.mark.parametrize("extra,mask", [("full", 0x7f), ("duplicate", 0xff & ~(1 << 5)), ("constant", 0xff & ~(1 << 3))])
def test_rank_rule(blmm, extra, mask):
    c = rank_rule_case(extra)
    got = _run(blmm, c)
    assert np.all(got["accepted"] == mask)
    a = {"full": 7, "duplicate": 5, "constant": 3}[extra]
    assert np.all(got["beta"][:, a] == 0.0) and np.all(got["se"][:, a] == 0.0)
    ref = _ref(c, got["h2_null_list"])
    _check(got, ref, "rank rule " + extra)
    md = blmm.bulkscan_multidf(c["Y"], c["G"], c["K"], 8)
    _close(got["lod"], md["L"][c["locus"], c["trait"]], "lod vs bulkscan_multidf", scaled=False)


def test_nearly_collinear_covariates_at_h2_one(blmm):
    c = collinear_case()
    got = _run(blmm, c)
    edge = got["h2_null_list"] > 1.0 - 1e-6
    assert edge.sum() >= 5 and np.isin(c["trait"], np.nonzero(edge)[0]).sum() >= 50
    ref = _ref(c, got["h2_null_list"])
    _check(got, ref, "collinear covariates")


FIELDS = ("beta", "se", "sigma2", "lod", "accepted")


def test_order_and_repeats(blmm):
    """A shuffled list with repeats returns, entry by entry, what the sorted unique list returns -- bit for bit."""
    for name in ("grid_k3_n1000_c2", "exact_k2_n79_c1_reml_prior"):                     # the slab form and the LDS form
        c = PARITY[name]()
        P, m = c["G"].shape[1] // c["k"], c["Y"].shape[1]
        rng = np.random.default_rng(77)
        pairs = np.unique(np.stack([rng.integers(0, P, 120), rng.integers(0, m, 120)], axis=1), axis=0)
        pairs = pairs[np.lexsort((pairs[:, 0], pairs[:, 1]))]
        base = _run(blmm, c, pairs[:, 0], pairs[:, 1])
        pick = rng.integers(0, len(pairs), 500)
        mixed = _run(blmm, c, pairs[pick, 0], pairs[pick, 1])
        for f in FIELDS:
            np.testing.assert_array_equal(mixed[f], base[f][pick], err_msg=f)
        one = _run(blmm, c, pairs[7:8, 0], pairs[7:8, 1])                                # T = 1
        for f in FIELDS:
            np.testing.assert_array_equal(one[f], base[f][7:8], err_msg=f)
        assert _run(blmm, c, [], [])["beta"].shape == (0, c["k"])                        # T = 0


def test_one_trait_one_test_per_trait_and_a_long_list(blmm):
    c = PARITY["exact_k1_n79_c2_weights"]()
    P, m = c["G"].shape[1], c["Y"].shape[1]
    grid = _run(blmm, c, np.repeat(np.arange(P), m), np.tile(np.arange(m), P))           # every (locus, trait), trait fastest
    full = {f: grid[f].reshape((P, m) + grid[f].shape[1:]) for f in FIELDS}
    scan = blmm.bulkscan(c["Y"], c["G"], c["K"], c["Cov"], method=c["method"], **c["kw"])
    _close(full["lod"], scan["L"], "every test against bulkscan", scaled=False)
    one_trait = _run(blmm, c, np.arange(P)[::-1], np.full(P, 3))                         # every test on one trait
    per_trait = _run(blmm, c, np.arange(m) % P, np.arange(m))                            # one test per trait
    rng = np.random.default_rng(78)
    T = 300000                                                                           # the sort's multi-workgroup path
    loc, tr = rng.integers(0, P, T), rng.integers(0, m, T)
    big = _run(blmm, c, loc, tr)
    for f in FIELDS:
        np.testing.assert_array_equal(one_trait[f], full[f][::-1, 3], err_msg=f)
        np.testing.assert_array_equal(per_trait[f], full[f][np.arange(m) % P, np.arange(m)], err_msg=f)
        np.testing.assert_array_equal(big[f], full[f][loc, tr], err_msg=f)


@pytest.mark.parametrize("method", ["null-grid", "null-exact"])
def test_peaks_convenience(blmm, method):
    c = PARITY["grid_k1_n79_c1"]()
    red = blmm.bulkscan_reduced(c["Y"], c["G"], c["K"], method=method)
    peaks = blmm.bulkscan_effects(c["Y"], c["G"], c["K"], method=method)
    m = c["Y"].shape[1]
    np.testing.assert_array_equal(peaks["locus"], red["argmax"])
    np.testing.assert_array_equal(peaks["trait"], np.arange(m))
    explicit = blmm.bulkscan_effects(c["Y"], c["G"], c["K"], locus=red["argmax"], trait=np.arange(m), method=method)
    for f in FIELDS + ("h2_null_list",):
        np.testing.assert_array_equal(peaks[f], explicit[f], err_msg=f)
    _close(peaks["lod"], red["max_lod"], "peak lod vs bulkscan_reduced", scaled=False)
    with pytest.raises(blmm.BulkLMMError):
        blmm.bulkscan_effects(c["Y"], np.hstack([c["G"], c["G"]]), c["K"], k=2)          # k > 1: the lists are required


@pytest.mark.parametrize("method", ["null-grid", "null-exact"])
def test_the_call_leaves_other_calls_alone(blmm, method):
    """bulkscan and bulkscan_reduced, bulkscan_effects, then the two again on one context: the second pair equals the first bit for
    bit, peaks, triplets and status counters included (marker 0 is constant)."""
    c = PARITY["exact_k2_n79_c1_reml_prior"]()
    G1 = c["G"][:, ::2].copy()
    G1[:, 0] = 0.5

    def scans():
        return (blmm.bulkscan(c["Y"], G1, c["K"], method=method),
                blmm.bulkscan_reduced(c["Y"], G1, c["K"], method=method, threshold=2.0, return_status=True))
    a, ra = scans()
    blmm.bulkscan_effects(c["Y"], c["G"], c["K"], k=2, locus=c["locus"], trait=c["trait"], method=method)
    b, rb = scans()
    np.testing.assert_array_equal(a["L"], b["L"])
    np.testing.assert_array_equal(a["h2_null_list"], b["h2_null_list"])
    for f in ("max_lod", "argmax", "h2_null_list"):
        np.testing.assert_array_equal(ra[f], rb[f], err_msg=f)
    for x, y in zip(ra["triplets"], rb["triplets"]):
        np.testing.assert_array_equal(x, y)
    print("n_nan_lod", ra["status"].n_nan_lod, "NaNs in L", int(np.isnan(a["L"]).sum()))
    for f in ("n_nan_lod", "n_zero_norm", "n_neg_eig", "n_nonpos_weight", "n_illcond_rescan", "lowrank_fallback", "n_h2_boundary"):
        assert getattr(ra["status"], f) == getattr(rb["status"], f), f


def test_torch_wrapper_in_its_own_process():
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "helpers", "effects_dev_check.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "effects_dev ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
