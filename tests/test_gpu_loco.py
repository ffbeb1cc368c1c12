"""Leave-one-chromosome-out bulkscan on the GPU (blmm_kinship_loco, blmm_bulkscan_loco).

The contract is the composition of the library's own calls: for the markers of chromosome c,
    bulkscan_loco(Y, G, chrom).L[rows_c] == bulkscan(Y, G[:, rows_c], calcKinship_loco(G, chrom)[c]).L   (bit for bit)
and calcKinship_loco(G, chrom)[c] is calcKinship(G[:, not rows_c]) (src/kinship.jl:4-14) to 1e-13."""
import json
import os
import time

import numpy as np
import pytest

from common import GOLDEN, assert_lod_close, make_geno
from oracle import bulklmm_oracle as O

pytestmark = pytest.mark.gpu

GRID = [i / 10.0 for i in range(10)]


def bxd_runs():
    fx = json.load(open(os.path.join(GOLDEN, "bxd_chr_runs.json")))
    return [lab for lab, k in zip(fx["chromosomes"], fx["counts"]) for _ in range(k)]


def equal_runs(p, nchr):
    b = np.linspace(0, p, nchr + 1).round().astype(int)
    return [str(c + 1) for c in range(nchr) for _ in range(b[c + 1] - b[c])]


def rows_of(res):
    cs = res["chr_start"]
    return [np.arange(cs[c], cs[c + 1]) for c in range(len(cs) - 1)]


def traits(G, m, seed, h2=0.5):
    """m traits with a polygenic background of heritability ~h2 over every marker, plus a mean of 10."""
    rng = np.random.default_rng(seed)
    n, p = G.shape
    X = (G - G.mean(0)) / np.maximum(G.std(0), 1e-6)
    g = X @ rng.standard_normal((p, m)) / np.sqrt(p)
    g /= g.std(0)
    return 10.0 + np.sqrt(h2) * g + np.sqrt(1.0 - h2) * rng.standard_normal((n, m))


# ---- 1. the kinships ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["bxd", "n300"])
def test_kinship_loco_against_calcKinship(blmm, shape):
    rng = np.random.default_rng(11)
    if shape == "bxd":
        chrom = bxd_runs()
        G = make_geno(79, len(chrom), rng)
    else:
        chrom = equal_runs(3000, 7)
        G = make_geno(300, 3000, rng)
    Kl = blmm.calcKinship_loco(G, chrom)
    _, cs = blmm.chromosome_runs(chrom, G.shape[1])
    assert Kl.shape == (len(cs) - 1, G.shape[0], G.shape[0])
    Kr = blmm.calcKinship_loco(G, chrom, digits=12)
    near = 0
    for c in range(len(cs) - 1):
        keep = np.ones(G.shape[1], bool)
        keep[cs[c]:cs[c + 1]] = False
        ref = O.calcKinship(G[:, keep])
        assert np.abs(Kl[c] - ref).max() <= 1e-13, (c, np.abs(Kl[c] - ref).max())
        assert np.array_equal(Kl[c], Kl[c].T)
        # digits = 12: np.round of the oracle's, except where the oracle sits within 1e-13 of a rounding boundary
        frac = np.abs(ref * 1e12 - np.floor(ref * 1e12) - 0.5)
        edge = frac * 1e-12 <= 1e-13
        near += int(edge.sum())
        assert np.array_equal(Kr[c][~edge], np.round(ref, 12)[~edge]), c
    print(f"kinship_loco {shape}: {near} entries within 1e-13 of a 12-digit rounding boundary (not compared)")


# ---- 2. bit equality with the composed calls ---------------------------------------------------------------------------------
def composed_check(blmm, Y, G, chrom, res, method, **kw):
    Kl = blmm.calcKinship_loco(G, chrom, digits=kw.pop("kinship_digits", None))
    for c, rows in enumerate(rows_of(res)):
        one = blmm.bulkscan(Y, G[:, rows], np.ascontiguousarray(Kl[c]), method=method, **kw)
        assert np.array_equal(res["L"][rows], one["L"], equal_nan=True), (method, c)
        if method == "alt-grid":
            assert np.array_equal(res["h2_panel"][rows], one["h2_panel"]), c
        else:
            assert np.array_equal(res["h2_null_list"][c], one["h2_null_list"]), c


@pytest.mark.parametrize("method", ["null-exact", "null-grid", "alt-grid"])
def test_loco_equals_composed_calls_bxd_shape(blmm, method):
    rng = np.random.default_rng(21)
    chrom = bxd_runs()[::5]                          # every fifth marker of the real map: the 20 runs, 1465 markers
    G = make_geno(79, len(chrom), rng)
    Y = traits(G, 24, 22)
    res = blmm.bulkscan_loco(Y, G, chrom, method=method, h2_grid=GRID)
    assert res["chromosomes"] == [str(i) for i in range(1, 20)] + ["X"]
    assert res["L"].shape == (G.shape[1], 24)
    composed_check(blmm, Y, G, chrom, res, method, h2_grid=GRID)


@pytest.mark.parametrize("method", ["null-exact", "null-grid"])
def test_loco_covariates_weights_reml(blmm, method):
    rng = np.random.default_rng(31)
    chrom = equal_runs(900, 5)
    G = make_geno(79, 900, rng)
    Y = traits(G, 16, 32)
    Cov = rng.standard_normal((79, 2))                # c = 3 with the intercept
    Y += Cov @ rng.standard_normal((2, 16))
    w = rng.uniform(0.5, 2.0, 79)
    res = blmm.bulkscan_loco(Y, G, chrom, Cov, method=method, h2_grid=GRID, kinship_digits=12)
    composed_check(blmm, Y, G, chrom, res, method, Covar=Cov, h2_grid=GRID, kinship_digits=12)
    res = blmm.bulkscan_loco(Y, G, chrom, method=method, h2_grid=GRID, weights=w, reml=True, prior_sample_size=0.1)
    composed_check(blmm, Y, G, chrom, res, method, h2_grid=GRID, weights=w, reml=True, prior_sample_size=0.1)


@pytest.mark.parametrize("case", ["c4", "exact_full_rank"])
def test_loco_null_exact_full_rank_form(blmm, case):
    """null-exact through the full-rank scan (no low-rank weights form): three covariates plus the intercept (c = 4), or the tuning
    exact_full_rank.  n = 79 <= 160, so the grid methods would rotate the markers on the side stream -- this method must not."""
    rng = np.random.default_rng(35)
    chrom = equal_runs(1100, 6)
    G = make_geno(79, 1100, rng)
    Y = traits(G, 40, 36)
    ctx = blmm.Context(0)
    kw = {"ctx": ctx}
    if case == "c4":
        Cov = rng.standard_normal((79, 3))
        Y += Cov @ rng.standard_normal((3, 40))
        kw["Covar"] = Cov
    else:
        ctx.set_tuning("exact_full_rank", 1)
    for _ in range(2):                               # the second call reuses the workspace of the first
        res = blmm.bulkscan_loco(Y, G, chrom, method="null-exact", **kw)
        composed_check(blmm, Y, G, chrom, res, "null-exact", **kw)
    ctx.close()


@pytest.mark.parametrize("n,p,nchr", [(124, 1200, 6), (300, 1500, 4), (1000, 2000, 3)])
def test_loco_equals_composed_calls_sizes(blmm, n, p, nchr):
    rng = np.random.default_rng(n)
    chrom = equal_runs(p, nchr)
    G = make_geno(n, p, rng)
    Y = traits(G, 12, n + 1)
    for method in ("null-exact", "null-grid"):
        res = blmm.bulkscan_loco(Y, G, chrom, method=method, h2_grid=GRID)
        composed_check(blmm, Y, G, chrom, res, method, h2_grid=GRID)


def test_rank_deficient_complement_takes_the_fallback_alone(blmm):
    """Chromosome "A" holds all but three markers: K_{-A} comes from three 0/1 markers (rank <= 4, a 75-fold repeated eigenvalue)
    and takes the Jacobi fallback; "B" and "C" do not.  Each matches its own single call."""
    rng = np.random.default_rng(41)
    n, p = 79, 600
    G = make_geno(n, p, rng)
    G[:, -3:] = (rng.random((n, 3)) < 0.5).astype(float)
    chrom = ["A"] * (p - 3) + ["B"] * 2 + ["C"]
    Y = traits(G, 10, 42)
    res = blmm.bulkscan_loco(Y, G, chrom, method="null-exact", return_status=True)
    Kl = blmm.calcKinship_loco(G, chrom)
    sweeps = []
    for c, rows in enumerate(rows_of(res)):
        L1, h1, st = blmm.api._bulkscan_call(blmm._lib.BLMM_NULL_EXACT, Y, G[:, rows], np.ascontiguousarray(Kl[c]), None, None, True, None,
                                             1.0, 0.0, False, 1, "eigen", 0, None, return_status=True)
        assert np.array_equal(res["L"][rows], L1, equal_nan=True), c
        assert np.array_equal(res["h2_null_list"][c], h1), c
        sweeps.append(int(st.jacobi_sweeps))
    print("Jacobi sweeps per chromosome (A, B, C):", sweeps)
    assert sweeps[0] > 0 and sweeps[1] == 0 and sweeps[2] == 0
    assert res["status"].jacobi_sweeps == sum(sweeps)


# ---- 3. against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["null-exact", "null-grid"])
def test_loco_against_oracle(blmm, method):
    rng = np.random.default_rng(51)
    chrom = bxd_runs()[::4]
    G = make_geno(79, len(chrom), rng)
    Y = traits(G, 6, 52)
    res = blmm.bulkscan_loco(Y, G, chrom, method=method)
    for c, rows in enumerate(rows_of(res)):
        keep = np.ones(G.shape[1], bool)
        keep[rows] = False
        K = O.calcKinship(G[:, keep])
        if method == "null-exact":
            own = O.bulkscan_null(Y, G[:, rows], K)
            assert np.abs(res["h2_null_list"][c] - own.h2_null_list).max() <= 1e-6
            ref = O.bulkscan_null(Y, G[:, rows], K, h2_override=res["h2_null_list"][c])
            assert_lod_close(res["L"][rows], ref.L)
        else:
            ref = O.bulkscan(Y, G[:, rows], K, method="null-grid")
            assert np.array_equal(res["h2_null_list"][c], ref["h2_null_list"])
            assert_lod_close(res["L"][rows], ref["L"])


# ---- 4. the resident matrix --------------------------------------------------------------------------------------------------
def test_loco_resident_matrix(blmm):
    rng = np.random.default_rng(61)
    chrom = bxd_runs()[::3]
    G = make_geno(79, len(chrom), rng)
    Y = traits(G, 40, 62)
    p, m = G.shape[1], Y.shape[1]
    ctx = blmm.Context(0)
    host = blmm.bulkscan_loco(Y, G, chrom, method="null-exact", ctx=ctx)
    Lh = host["L"]
    res = blmm.bulkscan_loco(Y, G, chrom, method="null-exact", ctx=ctx, keep_on_device=True, output_pvals=True)
    d = res["L"]
    assert isinstance(d, blmm.DeviceLOD) and d.shape == (p, m)
    import ctypes as C
    pp, mm = C.c_int64(0), C.c_int64(0)
    ctx.check(ctx.lib.blmm_last_dims(ctx.h, C.byref(pp), C.byref(mm)))
    assert (pp.value, mm.value) == (p, m)
    mx, arg = d.colmax()
    assert np.array_equal(mx, Lh.max(0)) and np.array_equal(arg, Lh.argmax(0))
    i, j, lod = d.threshold(5.0)
    ii, jj = np.nonzero(Lh > 5.0)
    order = np.lexsort((ii, jj))
    assert np.array_equal(i, ii[order]) and np.array_equal(j, jj[order]) and np.array_equal(lod, Lh[ii[order], jj[order]])
    cols = [0, 7, m - 1]
    assert np.array_equal(d.columns(cols), Lh[:, cols])
    P = res["log10Pvals_mat"]
    ref = O.lod2log10p(Lh, 1)
    fin = np.isfinite(ref)
    assert np.all(np.abs(P[fin] - ref[fin]) <= 1e-10 * np.abs(ref[fin]) + 1e-14)
    assert np.array_equal(res["h2_null_list"], host["h2_null_list"])


def test_loco_dev_form(blmm):
    """blmm_bulkscan_loco_dev on resident inputs, a padded leading dimension and the kinships passed in or not: the host form's bits.
    Odd n and p put the chromosome blocks of G and L at 8-byte offsets.  (Device buffers through the HIP runtime: torch cannot be
    initialised in a process whose HIP runtime the library brought up first -- tests/common.py:DevBuf.)"""
    import ctypes as C
    from common import DevBuf
    rng = np.random.default_rng(71)
    n, p, m, ld = 79, 701, 20, 705
    chrom = equal_runs(p, 4)
    G = make_geno(n, p, rng)
    Y = traits(G, m, 72)
    ctx = blmm.Context(0)
    host = blmm.bulkscan_loco(Y, G, chrom, method="null-grid", ctx=ctx)
    _, cs = blmm.chromosome_runs(chrom, p)
    Kl = blmm.calcKinship_loco(G, chrom, ctx=ctx)
    dY, dG, dK = DevBuf(Y.T), DevBuf(G.T), DevBuf(np.ascontiguousarray(Kl))
    grid = np.asarray(GRID)
    o = blmm.api._opts(blmm._lib.BLMM_NULL_GRID)
    for K in (None, dK):
        dL = DevBuf(np.full((m, ld), np.nan))
        dh = DevBuf(nbytes=8 * 4 * m)
        st = blmm._lib.blmm_status()
        ctx.check(ctx.lib.blmm_bulkscan_loco_dev(ctx.h, C.byref(o), dY.ptr, n, m, dG.ptr, p, cs.ctypes.data, 4, -1, None, 0, None,
                                                 grid.ctypes.data, grid.size, None if K is None else K.ptr, dL.ptr, ld, dh.ptr,
                                                 C.byref(st)))
        Lb = dL.get((m, ld))
        assert np.array_equal(Lb[:, :p].T, host["L"])
        assert np.isnan(Lb[:, p:]).all()
        assert np.array_equal(dh.get((4, m)), host["h2_null_list"])
        assert st.n_nan_lod == 0
        for b in (dL, dh):
            b.free()
    for b in (dY, dG, dK):
        b.free()
    ctx.close()


# ---- 5. the full BXD shape -----------------------------------------------------------------------------------------------------
def test_loco_full_bxd_shape(blmm):
    rng = np.random.default_rng(81)
    chrom = bxd_runs()
    G = make_geno(79, len(chrom), rng)
    Y = traits(G, 35554, 82)
    ctx = blmm.Context(0)
    t0 = time.time()
    res = blmm.bulkscan_loco(Y, G, chrom, method="null-exact", ctx=ctx, return_status=True)
    print(f"bulkscan_loco BXD shape (host to host): {time.time() - t0:.2f} s")
    Kl = blmm.calcKinship_loco(G, chrom, ctx=ctx)
    tot = {k: 0 for k in ("n_neg_eig", "n_nonpos_weight", "n_zero_norm", "n_nan_lod", "n_brent_maxiter", "jacobi_sweeps",
                          "lowrank_fallback", "n_h2_boundary", "n_illcond_rescan")}
    for c, rows in enumerate(rows_of(res)):
        L1, h1, st = blmm.api._bulkscan_call(blmm._lib.BLMM_NULL_EXACT, Y, G[:, rows], np.ascontiguousarray(Kl[c]), None, None, True, None,
                                             1.0, 0.0, False, 1, "eigen", 0, ctx, return_status=True)
        assert np.array_equal(res["L"][rows], L1, equal_nan=True), c
        assert np.array_equal(res["h2_null_list"][c], h1), c
        for k in tot:
            tot[k] += getattr(st, k)
    for k, v in tot.items():
        assert getattr(res["status"], k) == v, k


# ---- 6. what LOCO is for -------------------------------------------------------------------------------------------------------
def test_loco_recovers_proximal_contamination(blmm):
    """A QTL planted on chromosome 5 of a BXD-shaped trait with h2 ~ 0.5: the plain kinship contains the QTL's chromosome, its random
    effect absorbs part of the QTL and the LOD at the QTL drops; the LOCO kinship does not."""
    rng = np.random.default_rng(91)
    chrom = bxd_runs()
    G = make_geno(79, len(chrom), rng)
    _, cs = blmm.chromosome_runs(chrom, G.shape[1])
    q = int(cs[4] + 200)
    Y = traits(G, 16, 92)
    Y += 0.8 * (G[:, [q]] - 0.5) / np.std(G[:, q])
    K = blmm.calcKinship(G)
    plain = blmm.bulkscan(Y, G, K, method="null-exact")["L"][q]
    loco = blmm.bulkscan_loco(Y, G, chrom, method="null-exact")["L"][q]
    print("LOD at the planted marker, plain vs LOCO:", np.round(plain, 2), np.round(loco, 2))
    # (traits whose null h2 sits at 0 under both kinships get the same LOD from both, up to rounding)
    higher, lower = int((loco > plain + 1e-6).sum()), int((loco < plain - 1e-6).sum())
    print(f"LOCO higher for {higher} traits, lower for {lower}")
    assert loco[0] > plain[0]
    assert higher > 2 * lower and loco.mean() > plain.mean()
