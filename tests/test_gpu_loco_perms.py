"""The leave-one-chromosome-out permutation test on the GPU (blmm_bulkscan_loco_perms).

The contract is the composition of the library's own calls.  With K_c = calcKinship_loco(G, chrom, kinship_digits)[c] and
    ref_c = bulkscan_perms(Y, G[:, rows_c], K_c, Covar; same nperms, rndseed / perm_idx, options),
every per-chromosome table of bulkscan_loco_perms is ref_c's bit for bit (markers global: + chr_start[c]), and the genome-wide
tables are what NumPy gets from those: the maximum over chromosomes of each permutation's maximum (copies paired by permutation
index), the peak with the lowest global marker on ties, the quantile rule and the p-value formula."""
import json
import os
import time

import numpy as np
import pytest

from common import GOLDEN, assert_lod_close, make_data, make_geno
from oracle import bulklmm_oracle as O

pytestmark = pytest.mark.gpu

SIG = (0.10, 0.05)
TIGHT = dict(rtol=1e-12, atol=1e-13)
SIZES = (110, 40, 90, 60)          # 4 unequal chromosomes, not in size order


def runs_of(sizes):
    return [str(c + 1) for c, k in enumerate(sizes) for _ in range(k)]


def bxd_runs():
    fx = json.load(open(os.path.join(GOLDEN, "bxd_chr_runs.json")))
    return [lab for lab, k in zip(fx["chromosomes"], fx["counts"]) for _ in range(k)]


def make(n=60, sizes=SIZES, m=20, seed=1, ncov=0, qtl=True):
    """Genotypes, m traits (polygenic background, a mean of 10, a QTL in about a third of them) and ncov covariates."""
    rng = np.random.default_rng(seed)
    p = sum(sizes)
    G = make_geno(n, p, rng)
    X = (G - G.mean(0)) / np.maximum(G.std(0), 1e-6)
    g = X @ rng.standard_normal((p, m)) / np.sqrt(p)
    g /= np.maximum(g.std(0), 1e-12)
    Y = 10.0 + np.sqrt(0.4) * g + np.sqrt(0.6) * rng.standard_normal((n, m))
    if qtl:
        hit = rng.random(m) < 0.35
        q = rng.integers(0, p, size=m)
        Y[:, hit] += 1.2 * G[:, q[hit]]
    Cov = rng.standard_normal((n, ncov)) if ncov else None
    if ncov:
        Y += Cov @ rng.standard_normal((ncov, m))
    return Y, G, Cov, runs_of(sizes)


def references(blmm, Y, G, chrom, Cov, kinship_digits=None, **kw):
    """ref_c for every chromosome in run order, and the offsets."""
    runs, cs = blmm.chromosome_runs(chrom, G.shape[1])
    Kl = blmm.calcKinship_loco(G, chrom, digits=kinship_digits)
    refs = [blmm.bulkscan_perms(Y, G[:, cs[c]:cs[c + 1]], np.ascontiguousarray(Kl[c]), Cov, signif_level=SIG, **kw)
            for c in range(len(runs))]
    return refs, cs


def check_chromosomes(res, refs, cs):
    """Item 1: every per-chromosome field against ref_c, bit for bit."""
    for c, r in enumerate(refs):
        np.testing.assert_array_equal(res["h2_null"][c], r["h2_null"], err_msg=f"h2_null[{c}]")
        np.testing.assert_array_equal(res["sigma2_e"][c], r["sigma2_e"], err_msg=f"sigma2_e[{c}]")
        np.testing.assert_array_equal(res["chr_lod_max"][c], r["lod_max"], err_msg=f"chr_lod_max[{c}]")
        a = r["lod_argmax"]
        np.testing.assert_array_equal(res["chr_lod_argmax"][c], np.where(a >= 0, a + cs[c], -1), err_msg=f"chr_lod_argmax[{c}]")
        np.testing.assert_array_equal(res["chr_thresholds"][c], r["thresholds"], err_msg=f"chr_thresholds[{c}]")
        np.testing.assert_array_equal(res["chr_pvals_perm"][c], r["pvals_perm"], err_msg=f"chr_pvals_perm[{c}]")
        if "chr_max_perms" in res:
            np.testing.assert_array_equal(res["chr_max_perms"][c], r["max_perms"], err_msg=f"chr_max_perms[{c}]")


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


def genome_from(cmx, carg, cmp):
    """The genome-wide peak, its marker and the permutation maxima from per-chromosome tables (NumPy): larger value wins, an equal
    one only with a lower valid global marker (so NaN is never the maximum and run order cannot decide a tie)."""
    best = np.full(cmx.shape[1], -np.inf)
    bi = np.full(cmx.shape[1], -1, dtype=np.int64)
    for v, i in zip(cmx, carg):
        take = (v > best) | ((v == best) & (i >= 0) & ((bi < 0) | (i < bi)))
        best[take] = v[take]
        bi[take] = i[take]
    return best, bi, (cmp.max(axis=0) if cmp is not None else None)


def check_genome(blmm, res, cmx, carg, cmp, nperms, exact_thresholds=True):
    """Item 2: the genome-wide tables against NumPy on the per-chromosome values."""
    lm, la, mp = genome_from(cmx, carg, cmp)
    np.testing.assert_array_equal(res["lod_max"], lm)
    np.testing.assert_array_equal(res["lod_argmax"], la)
    assert res["max_perms"].shape == (nperms, lm.shape[0])
    if nperms == 0:
        assert np.isnan(res["thresholds"]).all() and np.isnan(res["pvals_perm"]).all()
        return
    np.testing.assert_array_equal(res["max_perms"], mp)
    np.testing.assert_array_equal(res["pvals_perm"], _pvals(mp, lm))
    assert_lod_close(res["thresholds"], _quantiles(mp, 1.0 - np.asarray(SIG)), what="thresholds", **TIGHT)
    if exact_thresholds:
        # the quantile rule exactly: get_thresholds of a one-marker permutation matrix whose maxima are max_perms[:, j]
        for j in range(lm.shape[0]):
            thr = blmm.get_thresholds(mp[:, j][None, :], list(SIG))["thrs"]
            np.testing.assert_array_equal(res["thresholds"][:, j], thr, err_msg=f"thresholds[:, {j}]")


# ---- 1 + 2: each chromosome against bulkscan_perms; the genome-wide tables against NumPy -------------------------------------------
@pytest.mark.parametrize("ncov,weighted,reml", [(0, False, False), (2, False, False), (0, True, False), (2, True, True)])
@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("kdig", [None, 12])
def test_each_chromosome_matches_bulkscan_perms(blmm, ncov, weighted, reml, explicit, kdig):
    Y, G, Cov, chrom = make(seed=31 + ncov, ncov=ncov)
    n = Y.shape[0]
    nperms = 48
    kw = dict(reml=reml)
    if weighted:
        kw["weights"] = np.random.default_rng(5).uniform(0.5, 2.0, n)
    if reml:
        kw.update(prior_variance=1.0, prior_sample_size=0.1)
    pidx = O.make_perm_idx(n, nperms, 13) if explicit else None
    res = blmm.bulkscan_loco_perms(Y, G, chrom, Cov, nperms=nperms, rndseed=17, perm_idx=pidx, signif_level=SIG, kinship_digits=kdig,
                                   chr_max_perms=True, **kw)
    refs, cs = references(blmm, Y, G, chrom, Cov, kdig, nperms=nperms, rndseed=17, perm_idx=pidx, **kw)
    assert res["chr_max_perms"].shape == (4, nperms, 20) and res["chr_thresholds"].shape == (4, 2, 20)
    assert res["chromosomes"] == ["1", "2", "3", "4"] and res["chr_start"].tolist() == [0, 110, 150, 240, 300]
    check_chromosomes(res, refs, cs)
    check_genome(blmm, res, res["chr_lod_max"], res["chr_lod_argmax"], res["chr_max_perms"], nperms)


def test_genome_wide_against_numpy_on_the_references(blmm):
    """Item 2 from ref_c alone (no chr_max_perms asked for: the call downloads nothing nperms-sized per chromosome)."""
    Y, G, Cov, chrom = make(seed=77, ncov=1)
    nperms = 40
    res = blmm.bulkscan_loco_perms(Y, G, chrom, Cov, nperms=nperms, rndseed=4)
    assert "chr_max_perms" not in res
    refs, cs = references(blmm, Y, G, chrom, Cov, nperms=nperms, rndseed=4)
    cmx = np.stack([r["lod_max"] for r in refs])
    carg = np.stack([np.where(r["lod_argmax"] >= 0, r["lod_argmax"] + cs[c], -1) for c, r in enumerate(refs)])
    cmp = np.stack([r["max_perms"] for r in refs])
    check_genome(blmm, res, cmx, carg, cmp, nperms)
    check_chromosomes(res, refs, cs)


# ---- 3. large n: the multi-kernel panel route, and ragged chunks ----------------------------------------------------------------
def test_large_n_and_ragged_chunks(blmm):
    Y, G, Cov, chrom = make(n=300, m=7, seed=300, ncov=1)
    nperms = 20
    ctx = blmm.default_context()
    one = blmm.bulkscan_loco_perms(Y, G, chrom, Cov, nperms=nperms, rndseed=3, chr_max_perms=True, ctx=ctx)
    ctx.set_tuning("bulk_perm_cols", 3 * (nperms + 1))          # chunks of 3, 3 and 1 traits on every chromosome
    try:
        many = blmm.bulkscan_loco_perms(Y, G, chrom, Cov, nperms=nperms, rndseed=3, chr_max_perms=True, ctx=ctx)
    finally:
        ctx.set_tuning("defaults", 0)
    assert ctx.get_tuning("bulk_perm_cols") == 0
    for key in ("h2_null", "sigma2_e", "lod_max", "lod_argmax", "max_perms", "thresholds", "pvals_perm", "chr_lod_max",
                "chr_lod_argmax", "chr_max_perms", "chr_thresholds", "chr_pvals_perm"):
        np.testing.assert_array_equal(one[key], many[key], err_msg=key)
    refs, cs = references(blmm, Y, G, chrom, Cov, nperms=nperms, rndseed=3)
    check_chromosomes(one, refs, cs)
    check_genome(blmm, one, one["chr_lod_max"], one["chr_lod_argmax"], one["chr_max_perms"], nperms)


# ---- 4. ties --------------------------------------------------------------------------------------------------------------------
def test_tie_between_identical_chromosomes_goes_to_the_lower_marker(blmm):
    """Chromosomes 1 and 3 hold the same marker columns: their LOCO kinships (each the sum of the other two blocks) and LODs are
    equal, so every trait's peak ties between them and must sit on chromosome 1.  Permutations 0 and 5 are the identity."""
    rng = np.random.default_rng(8)
    n, m, nperms = 60, 12, 30
    A = make_geno(n, 90, rng)
    B = make_geno(n, 50, rng)
    G = np.hstack([A, B, A])
    chrom = runs_of((90, 50, 90))
    Y = 10.0 + rng.standard_normal((n, m))
    Y += 1.5 * A[:, rng.integers(0, 90, size=m)]                # every trait's QTL on the repeated block
    pidx = O.make_perm_idx(n, nperms, 21)
    pidx[:, 0] = np.arange(n)
    pidx[:, 5] = np.arange(n)
    res = blmm.bulkscan_loco_perms(Y, G, chrom, nperms=nperms, perm_idx=pidx, chr_max_perms=True)
    np.testing.assert_array_equal(res["chr_lod_max"][0], res["chr_lod_max"][2])
    np.testing.assert_array_equal(res["chr_lod_argmax"][2], res["chr_lod_argmax"][0] + 140)
    np.testing.assert_array_equal(res["chr_max_perms"][0], res["chr_max_perms"][2])
    assert (res["lod_max"] == res["chr_lod_max"][0]).all()
    np.testing.assert_array_equal(res["lod_argmax"], res["chr_lod_argmax"][0])
    assert (res["lod_argmax"] < 90).all()
    mp, lm = res["max_perms"], res["lod_max"]
    assert (mp[0] == lm).all() and (mp[5] == lm).all()
    np.testing.assert_array_equal(res["pvals_perm"], _pvals(mp, lm))
    assert (res["pvals_perm"] >= 3.0 / (nperms + 1)).all()
    check_genome(blmm, res, res["chr_lod_max"], res["chr_lod_argmax"], res["chr_max_perms"], nperms)


# ---- 5. edge cases --------------------------------------------------------------------------------------------------------------
def test_no_permutations(blmm):
    Y, G, Cov, chrom = make(m=5, seed=50)
    res = blmm.bulkscan_loco_perms(Y, G, chrom, nperms=0, chr_max_perms=True)
    assert res["max_perms"].shape == (0, 5) and res["chr_max_perms"].shape == (4, 0, 5)
    for key in ("thresholds", "pvals_perm", "chr_thresholds", "chr_pvals_perm"):
        assert np.isnan(res[key]).all(), key
    refs, cs = references(blmm, Y, G, chrom, None, nperms=0)
    check_chromosomes(res, refs, cs)
    check_genome(blmm, res, res["chr_lod_max"], res["chr_lod_argmax"], None, 0)


def test_one_trait(blmm):
    Y, G, Cov, chrom = make(m=3, seed=51)
    res = blmm.bulkscan_loco_perms(Y[:, 1:2], G, chrom, nperms=25, rndseed=2, chr_max_perms=True)
    assert res["lod_max"].shape == (1,) and res["chr_max_perms"].shape == (4, 25, 1)
    refs, cs = references(blmm, Y[:, 1:2], G, chrom, None, nperms=25, rndseed=2)
    check_chromosomes(res, refs, cs)
    check_genome(blmm, res, res["chr_lod_max"], res["chr_lod_argmax"], res["chr_max_perms"], 25)


def test_zero_norm_marker_raises_as_bulkscan_perms(blmm):
    Y, G, Cov, chrom = make(m=3, seed=52)
    G = G.copy()
    G[:, 170] = 0.0                                             # on chromosome 3
    with pytest.raises(blmm.BulkLMMError) as e:
        blmm.bulkscan_perms(Y, G[:, 150:240], np.eye(Y.shape[0]), nperms=8)
    with pytest.raises(blmm.BulkLMMError) as e2:
        blmm.bulkscan_loco_perms(Y, G, chrom, nperms=8)
    assert e2.value.msg == e.value.msg == "Dividing by zeros: the input vector can not contain any zeros!"


# ---- 6. the device form ---------------------------------------------------------------------------------------------------------
class _Dev:
    """A device array for the _dev wrapper: a DevBuf (the HIP runtime itself -- tests/common.py:DevBuf on why not torch) with the
    shape and data_ptr() the wrapper reads."""
    def __init__(self, arr=None, shape=None, dtype=np.float64):
        from common import DevBuf
        self.shape = tuple(arr.shape if arr is not None else shape)
        self.dtype = np.dtype(arr.dtype if arr is not None else dtype)
        self.buf = DevBuf(arr) if arr is not None else DevBuf(nbytes=int(np.prod(self.shape)) * self.dtype.itemsize)

    def data_ptr(self):
        return self.buf.ptr

    def get(self):
        return self.buf.get(self.shape, self.dtype)


@pytest.mark.parametrize("given_kinships", [False, True])
def test_dev_form_equals_host_form(blmm, given_kinships):
    Y, G, Cov, chrom = make(seed=60, ncov=2)
    n, m = Y.shape
    nperms = 33
    pidx = O.make_perm_idx(n, nperms, 6)
    ctx = blmm.default_context()
    host = blmm.bulkscan_loco_perms(Y, G, chrom, Cov, nperms=nperms, perm_idx=pidx, kinship_digits=12, chr_max_perms=True,
                                    return_status=True, ctx=ctx)
    _, cs = blmm.chromosome_runs(chrom, G.shape[1])
    nchr = len(cs) - 1
    dY, dG, dC = _Dev(np.ascontiguousarray(Y.T)), _Dev(np.ascontiguousarray(G.T)), _Dev(np.ascontiguousarray(Cov.T))
    dP = _Dev(np.ascontiguousarray(pidx.T))
    dK = _Dev(np.ascontiguousarray(blmm.calcKinship_loco(G, chrom, digits=12, ctx=ctx))) if given_kinships else None
    i64 = np.int64
    outs = {"h2_null": _Dev(shape=(nchr, m)), "sigma2_e": _Dev(shape=(nchr, m)), "lod_max": _Dev(shape=(m,)),
            "lod_argmax": _Dev(shape=(m,), dtype=i64), "max_perms": _Dev(shape=(m, nperms)), "thresholds": _Dev(shape=(m, 2)),
            "pvals_perm": _Dev(shape=(m,)), "chr_lod_max": _Dev(shape=(nchr, m)), "chr_lod_argmax": _Dev(shape=(nchr, m), dtype=i64),
            "chr_max_perms": _Dev(shape=(nchr, m, nperms)), "chr_thresholds": _Dev(shape=(nchr, m, 2)),
            "chr_pvals_perm": _Dev(shape=(nchr, m))}
    st = blmm.bulkscan_loco_perms_dev(ctx, dY, dG, cs, *outs.values(), nperms=nperms, perm_idx=dP, K_loco=dK, kinship_digits=12,
                                      Covar=dC, status=True)
    assert st.n_zero_norm == 0 and st.n_h2_boundary == host["status"].n_h2_boundary
    for key, d in outs.items():
        got = d.get()
        if key in ("max_perms", "thresholds"):
            got = got.T                                         # (m, k) rows = k x m column-major
        elif key in ("chr_max_perms", "chr_thresholds"):
            got = got.transpose(0, 2, 1)
        np.testing.assert_array_equal(got, host[key], err_msg=key)
    for d in [dY, dG, dC, dP] + ([dK] if dK else []) + list(outs.values()):
        d.buf.free()


# ---- 7. planted QTL and calibration ---------------------------------------------------------------------------------------------
def test_planted_qtl_on_the_third_chromosome(blmm):
    Y, G, Cov, chrom = make(m=6, seed=70, qtl=False)
    Y = Y.copy()
    Y[:, 2] += 3.0 * G[:, 200]                                  # chromosome 3: markers 150 .. 239
    nperms = 99
    res = blmm.bulkscan_loco_perms(Y, G, chrom, nperms=nperms, rndseed=11)
    assert res["pvals_perm"][2] == 1.0 / (nperms + 1)
    assert 150 <= res["lod_argmax"][2] < 240
    assert res["lod_max"][2] > res["thresholds"][1, 2]


def test_calibration_on_polygenic_traits(blmm):
    """400 purely polygenic traits under fixed seeds: the share with a genome-wide p-value <= 0.05 lies in [0.02, 0.09].  The genetic
    background is spread over 1000 unlinked markers in 10 chromosomes, so that no marker or chromosome carries a QTL-sized share
    (RIL-like haplotype blocks of ~100 markers would concentrate a chromosome's share on one or two loci).  Deterministic."""
    rng = np.random.default_rng(2024)
    n, p, m = 60, 1000, 400
    G = rng.integers(0, 2, size=(n, p)).astype(np.float64)
    X = (G - G.mean(0)) / G.std(0)
    g = X @ rng.standard_normal((p, m)) / np.sqrt(p)
    Y = 10.0 + np.sqrt(0.4) * g / g.std(0) + np.sqrt(0.6) * rng.standard_normal((n, m))
    res = blmm.bulkscan_loco_perms(Y, G, runs_of((100,) * 10), nperms=199, rndseed=5)
    frac = float(np.mean(res["pvals_perm"] <= 0.05))
    print(f"\nshare of genome-wide p <= 0.05 over 400 polygenic traits: {frac:.4f}")
    assert 0.02 <= frac <= 0.09, frac


# ---- 8. the full BXD shape ------------------------------------------------------------------------------------------------------
def test_loco_perms_fullsize(blmm):
    """The BXD chromosome runs (n = 79, p = 7321), m = 35554, 32 permutations: 16 sampled traits against every chromosome's
    bulkscan_perms, and the genome-wide tables of every trait against NumPy on chr_max_perms."""
    chrom = bxd_runs()
    N, P, M = 79, len(chrom), 35554
    nperms = 32
    Y, G, _, _ = make_data(n=N, p=P, m=M, seed=20241)
    blmm.bulkscan_loco_perms(Y[:, :64], G, chrom, nperms=nperms)      # warm-up (workspace, code objects)
    t0 = time.perf_counter()
    res = blmm.bulkscan_loco_perms(Y, G, chrom, nperms=nperms, rndseed=1, chr_max_perms=True)
    wall = time.perf_counter() - t0
    print(f"\nbulkscan_loco_perms n={N} p={P} m={M} nchr={len(res['chromosomes'])} nperms={nperms}: {wall:.3f} s wall "
          f"(host form, inputs uploaded, chr_max_perms downloaded)")
    assert res["chr_max_perms"].shape == (20, nperms, M) and np.isfinite(res["max_perms"]).all()
    traits = sorted(set(np.linspace(0, M - 1, 14).astype(int).tolist() + [1, M - 2]))
    assert len(traits) == 16
    refs, cs = references(blmm, Y[:, traits], G, chrom, None, nperms=nperms, rndseed=1)
    sub = {k: (v[..., traits] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[-1] == M else v) for k, v in res.items()}
    check_chromosomes(sub, refs, cs)
    check_genome(blmm, res, res["chr_lod_max"], res["chr_lod_argmax"], res["chr_max_perms"], nperms, exact_thresholds=False)
