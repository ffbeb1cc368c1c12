"""bulkscan_perms -- the permutation test for every trait of a bulk call -- against the single-trait path (trait j of the bulk
call is scan(Y[:, j], ...; permutation_test=True) under the same permutations: the same kernels' arithmetic, so the per-trait
reductions of L_perms are expected bit for bit), against the oracle on a shared rotation and h2, across trait chunks, at
large n and at the full BXD shape."""
import time

import numpy as np
import pytest

from common import assert_lod_close, make_data
from oracle import bulklmm_oracle as O

pytestmark = pytest.mark.gpu

SIG = (0.10, 0.05)
TIGHT = dict(rtol=1e-12, atol=1e-13)


def _pvals(mp, lm):
    nperms = mp.shape[0]
    hit = (mp >= lm[None, :]) & (mp != -np.inf)
    return (1.0 + hit.sum(axis=0)) / (nperms + 1.0)


def _quantiles(mp, probs):
    """k_quantiles' rule (Julia's default type 7) on each column, NaN sorted last."""
    nperms, m = mp.shape
    out = np.empty((len(probs), m))
    s = np.sort(mp, axis=0)
    for t, q in enumerate(probs):
        h = (nperms - 1) * min(max(q, 0.0), 1.0)
        lo = int(np.floor(h))
        hi = min(lo + 1, nperms - 1)
        out[t] = s[lo] + (h - lo) * (s[hi] - s[lo])
    return out


def _check_against_scan(blmm, res, Y, G, K, Cov, traits, nperms, *, seed=0, perm_idx=None, **kw):
    """Item 1 of the issue on the given traits; returns how many compared entries differ at all (bit equality is expected)."""
    ndiff = 0
    for j in traits:
        ref = blmm.scan(Y[:, j], G, K, Cov, permutation_test=nperms > 0, nperms=nperms, rndseed=seed, perm_idx=perm_idx, **kw)
        assert res["h2_null"][j] == ref["h2_null"] and res["sigma2_e"][j] == ref["sigma2_e"], j
        lod = ref["lod"]
        assert_lod_close(res["lod_max"][j], lod.max(), what=f"lod_max[{j}]", **TIGHT)
        assert res["lod_argmax"][j] == int(np.argmax(lod)), j
        ndiff += int(res["lod_max"][j] != lod.max())
        if nperms == 0:
            continue
        Lp = ref["L_perms"]
        assert_lod_close(res["max_perms"][:, j], Lp.max(axis=0), what=f"max_perms[:, {j}]", **TIGHT)
        ndiff += int(np.count_nonzero(res["max_perms"][:, j] != Lp.max(axis=0)))
        thr = blmm.get_thresholds(Lp, list(SIG))["thrs"]
        assert_lod_close(res["thresholds"][:, j], thr, what=f"thresholds[:, {j}]", **TIGHT)
        ndiff += int(np.count_nonzero(res["thresholds"][:, j] != thr))
    return ndiff


@pytest.mark.parametrize("ncov,weighted,reml", [(0, False, False), (2, False, False), (0, True, False), (2, True, True)])
@pytest.mark.parametrize("explicit", [False, True])
def test_bulk_perms_matches_scan_per_trait(blmm, ncov, weighted, reml, explicit):
    """BXD kinship, p = 500, m = 40, nperms = 64; c = 1 and 3, with and without weights, ML and REML with a prior; the library's
    generator from rndseed and an explicit perm_idx."""
    Y, G, K, Cov = make_data(p=500, m=40, seed=811 + ncov, ncov=ncov)
    n = Y.shape[0]
    nperms = 64
    kw = dict(reml=reml)
    if weighted:
        kw["weights"] = np.random.Generator(np.random.PCG64(5)).uniform(0.5, 2.0, n)
    if reml:
        kw.update(prior_variance=1.0, prior_sample_size=0.1)
    pidx = O.make_perm_idx(n, nperms, 13) if explicit else None
    res = blmm.bulkscan_perms(Y, G, K, Cov, nperms=nperms, rndseed=17, perm_idx=pidx, signif_level=SIG, **kw)
    assert res["max_perms"].shape == (nperms, 40) and res["thresholds"].shape == (2, 40)
    ndiff = _check_against_scan(blmm, res, Y, G, K, Cov, range(40), nperms, seed=17, perm_idx=pidx, **kw)
    assert ndiff == 0, f"{ndiff} entries within 1e-12 relative but not bit-identical"
    np.testing.assert_array_equal(res["pvals_perm"], _pvals(res["max_perms"], res["lod_max"]))


def test_bulk_perms_matches_oracle(blmm):
    """Shared rotation and h2 (as test_scan_perms_matches_oracle): every permutation maximum and the observed peak of 8 traits."""
    Y, G, K, _ = make_data(p=250, m=8, seed=909)
    n = Y.shape[0]
    nperms = 37
    pidx = O.make_perm_idx(n, nperms, 7)
    res = blmm.bulkscan_perms(Y, G, K, nperms=nperms, perm_idx=pidx, prior_variance=1.0, prior_sample_size=0.1)
    cov1 = np.ones((n, 1))
    for j in range(8):
        rot = blmm.transform_rotation(Y[:, j:j + 1], np.hstack([cov1, G]), K, addIntercept=False)
        pin = O.scan(Y[:, j], G, K, covar=cov1, addIntercept=False, permutation_test=True, nperms=nperms, perm_idx=pidx,
                     prior_variance=1.0, prior_sample_size=0.1, h2_override=res["h2_null"][j], rotation_override=rot)
        assert_lod_close(res["max_perms"][:, j], pin["L_perms"].max(axis=0), what=f"max_perms[:, {j}]")
        assert_lod_close(res["lod_max"][j], pin["lod"].max(), what=f"lod_max[{j}]")


@pytest.mark.parametrize("n", [300, 1000])
def test_bulk_perms_large_n_and_chunks(blmm, n):
    """The multi-kernel panel route (n > 256), c = 2: a few traits against scan, and one chunk against at least three (a ragged
    last chunk; m = 13 traits, 21 columns each, not a multiple of the scan's 64-column tile)."""
    m, nperms = 13, 20
    Y, G, K, Cov = make_data(n=n, p=333, m=m, seed=1200 + n, bxd=False, ncov=1)
    ctx = blmm.default_context()
    one = blmm.bulkscan_perms(Y, G, K, Cov, nperms=nperms, rndseed=3, ctx=ctx)
    ctx.set_tuning("bulk_perm_cols", 5 * (nperms + 1))          # chunks of 5, 5 and 3 traits
    try:
        many = blmm.bulkscan_perms(Y, G, K, Cov, nperms=nperms, rndseed=3, ctx=ctx)
    finally:
        ctx.set_tuning("defaults", 0)
    assert ctx.get_tuning("bulk_perm_cols") == 0
    for key in ("h2_null", "sigma2_e", "lod_max", "lod_argmax", "max_perms", "thresholds", "pvals_perm"):
        np.testing.assert_array_equal(one[key], many[key], err_msg=key)
    assert _check_against_scan(blmm, one, Y, G, K, Cov, [0, 6, m - 1], nperms, seed=3) == 0


def test_bulk_perms_single_trait_and_no_perms(blmm):
    Y, G, K, _ = make_data(p=300, m=5, seed=4242)
    one = blmm.bulkscan_perms(Y[:, :1], G, K, nperms=50, rndseed=9)
    assert _check_against_scan(blmm, one, Y[:, :1], G, K, None, [0], 50, seed=9) == 0
    zero = blmm.bulkscan_perms(Y, G, K, nperms=0)
    assert zero["max_perms"].shape == (0, 5)
    assert np.isnan(zero["thresholds"]).all() and np.isnan(zero["pvals_perm"]).all()
    assert _check_against_scan(blmm, zero, Y, G, K, None, range(5), 0) == 0


def test_bulk_perms_zero_norm_marker_raises_as_scan(blmm):
    Y, G, K, _ = make_data(p=40, m=3, seed=121)
    G = G.copy()
    G[:, 7] = 0.0
    with pytest.raises(blmm.BulkLMMError) as e:
        blmm.scan(Y[:, 0], G, K, permutation_test=True, nperms=8)
    with pytest.raises(blmm.BulkLMMError) as e2:
        blmm.bulkscan_perms(Y, G, K, nperms=8)
    assert e2.value.msg == e.value.msg == "Dividing by zeros: the input vector can not contain any zeros!"


def test_bulk_perms_pval_ties(blmm):
    """Permutations 0 and 5 are the identity: their maxima equal the observed peak exactly, and both count."""
    Y, G, K, _ = make_data(p=200, m=6, seed=77)
    n = Y.shape[0]
    nperms = 30
    pidx = O.make_perm_idx(n, nperms, 21)
    pidx[:, 0] = np.arange(n)
    pidx[:, 5] = np.arange(n)
    res = blmm.bulkscan_perms(Y, G, K, nperms=nperms, perm_idx=pidx)
    mp, lm = res["max_perms"], res["lod_max"]
    assert (mp[0] == lm).all() and (mp[5] == lm).all()
    np.testing.assert_array_equal(res["pvals_perm"], _pvals(mp, lm))
    assert (res["pvals_perm"] >= 3.0 / (nperms + 1)).all()


def test_bulk_perms_fullsize(blmm):
    """BASELINE.json configs[1] (n = 79, p = 7321, m = 35554) with 32 permutations: 32 sampled traits against scan, and the
    p-values and thresholds of every trait against NumPy on the returned maxima."""
    N, P, M = 79, 7321, 35554
    nperms = 32
    Y, G, K, _ = make_data(n=N, p=P, m=M, seed=20241)
    blmm.bulkscan_perms(Y[:, :64], G, K, nperms=nperms)             # warm-up (workspace, code objects)
    t0 = time.perf_counter()
    res = blmm.bulkscan_perms(Y, G, K, nperms=nperms, rndseed=1)
    wall = time.perf_counter() - t0
    print(f"\nbulkscan_perms n={N} p={P} m={M} nperms={nperms}: {wall:.3f} s wall (host form, inputs uploaded)")
    assert res["max_perms"].shape == (nperms, M) and np.isfinite(res["max_perms"]).all()
    traits = sorted(set(np.linspace(0, M - 1, 30).astype(int).tolist() + [1, M - 2]))[:32]
    assert _check_against_scan(blmm, res, Y, G, K, None, traits, nperms, seed=1) == 0
    np.testing.assert_array_equal(res["pvals_perm"], _pvals(res["max_perms"], res["lod_max"]))
    assert_lod_close(res["thresholds"], _quantiles(res["max_perms"], 1.0 - np.asarray(SIG)), what="thresholds", **TIGHT)
