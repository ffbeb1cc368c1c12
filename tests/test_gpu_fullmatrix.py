"""EVERY entry of the LOD matrix, not a sample of columns: BASELINE.json configs[1] (n=79, p=7321, m=35554: all 260,290,834
LODs), the configs[2] shard (n=500, p=50000, m=2500: 125,000,000) and a BXD-shaped run with two null covariates against the
C/OpenMP restatement oracle/bulkscan_null_ref.c (src/bulkscan.jl:263-309, src/bulkscan_helpers.jl:127-150) evaluated at the
device's own heritabilities -- `1e-6 |ref| + 1e-10` element-wise, the north-star bound -- and every heritability against that
restatement's own Brent run.

Why every entry: since round 2 the panel column a trait's LOD is computed in depends on the DATA -- two panel regions split by the
h2 search's hand-over, in each the shared-weights class from the front and six weight-basis segments from the back, every run
rounded to 64-column tiles, written back through `perm` -- so a mistake at a class / segment / region seam would land in columns
that a sample of 31 does not visit.  Each test prints the worst entry with its (trait, marker) and where that trait sat in the
layout, and a histogram of the relative errors."""
import math
import time

import numpy as np
import pytest

from common import assert_lod_close, make_data
from oracle import bulklmm_oracle as O

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-6, 1e-10
EDGES = [0.0, 0.25, 0.5, 0.7, 0.85, 0.95, 2.0]          # default weight-basis segments for n <= 80 (kernels_lowrank.hip)


def compare_every_entry(L, Lref, what):
    """Chunked over columns (the matrices are 2 GB each).  Returns (count outside the bound, worst relative error, (marker, trait),
    histogram of log10(relative error) over entries with |ref| > 1e-4)."""
    p, m = L.shape
    nbad, worst, at = 0, 0.0, (0, 0)
    bins = np.arange(-17, 1)                     # log10 edges: <1e-17 ... >=1
    hist = np.zeros(bins.size + 1, dtype=np.int64)
    finite = True
    for j0 in range(0, m, 1024):
        a = L[:, j0:j0 + 1024]; r = Lref[:, j0:j0 + 1024]
        finite = finite and bool(np.isfinite(a).all())
        err = np.abs(a - r)
        bad = ~(err <= RTOL * np.abs(r) + ATOL)
        nbad += int(bad.sum())
        rel = err / np.maximum(np.abs(r), 1e-4)
        k = int(np.argmax(rel))
        if rel.flat[k] > worst:
            worst = float(rel.flat[k]); i, j = np.unravel_index(k, rel.shape); at = (int(i), j0 + int(j))
        big = np.abs(r) > 1e-4
        with np.errstate(divide="ignore"):
            lg = np.log10(rel[big])
        hist += np.bincount(np.searchsorted(bins, lg, side="right"), minlength=hist.size)
    print(f"{what}: {p} x {m} = {p * m} entries; outside {RTOL}|ref| + {ATOL}: {nbad}; worst relative error {worst:.3e} at marker {at[0]}, trait {at[1]}")
    lo = [f"<1e{bins[0]}"] + [f"1e{b}" for b in bins]
    print("  log10(rel err) histogram (|ref| > 1e-4): " + ", ".join(f"{lo[k]}:{int(c)}" for k, c in enumerate(hist) if c))
    assert finite, what + ": non-finite LOD"
    return nbad, worst, at


def where(ctx, h2, lam, m, j):
    col, width, cnt = ctx.lowrank_columns(m)
    delta = h2[j] / (1.0 - h2[j])
    shared = delta * np.sqrt((lam ** 2).sum() / lam.size) <= 1e-13
    seg = int(np.searchsorted(EDGES, h2[j], side="right") - 1)
    c = int(col[j])
    return (f"trait {j}: h2 {h2[j]:.6g}, panel column {c} (region {c // width if c >= 0 else -1}, offset {c % width if c >= 0 else -1} "
            f"of {width}; region counts [shared, other columns] {cnt}), class {'shared-weights' if shared else f'rank-R, segment {seg}'}")


def run_case(blmm, Y, G, K, Cov, what, own_tol_outliers, weights=None, prior=(1.0, 0.0), reml=False):
    from oracle import cref
    from oracle import grid_ref as R
    ctx = blmm.default_context()
    t0 = time.time()
    L, h2, st = blmm.api._bulkscan_call(blmm._lib.BLMM_NULL_EXACT, Y, G, K, Cov, None, True, weights, prior[0], prior[1], reml, 1, "eigen",
                                        0, ctx, return_status=True)
    t1 = time.time()
    if weights is None:
        Lref, h2own = cref.bulkscan_null(Y, G, K, Cov, prior_variance=prior[0], prior_sample_size=prior[1], reml=reml, h2_override=h2)
    else:                                         # the C oracle on the pre-scaled inputs (src/bulkscan.jl:231-250), no intercept added
        Ys, Gs, Ks, Cs, ai = R.prepare(Y, G, K, Cov, weights)
        Lref, h2own = cref.bulkscan_null(Ys, Gs, Ks, Cs, addIntercept=ai, prior_variance=prior[0], prior_sample_size=prior[1], reml=reml,
                                         h2_override=h2)
        K = Ks
    t2 = time.time()
    lam = np.linalg.eigvalsh(K)
    p, m = L.shape
    print(f"{what}: GPU call {t1 - t0:.2f} s host to host, C/OpenMP oracle ({cref.load().blmm_ref_max_threads()} threads) {t2 - t1:.2f} s; "
          f"shared-weights traits {st.lowrank_shared}, rank {st.lowrank_rank}, re-scanned {st.lowrank_fallback} + {st.n_illcond_rescan}")
    nbad, worst, at = compare_every_entry(L, Lref, what)
    print("  worst entry: " + where(ctx, h2, lam, m, at[1]))
    assert nbad == 0, f"{what}: {nbad} entries outside the bound; " + where(ctx, h2, lam, m, at[1])
    # every heritability against the restatement's own search; the known exceptions are traits with a two-humped profile likelihood
    # (tests/test_gpu_guard.py::test_fullsize_h2_audit_all_traits examines each of them)
    dh = np.abs(h2 - h2own)
    out = np.flatnonzero(dh > 1e-6)
    print(f"  h2 against the oracle's own Brent: max |dh2| {dh.max():.3e}; {out.size} of {m} beyond 1e-6: "
          + ", ".join(f"{int(j)} ({h2[j]:.4g} vs {h2own[j]:.4g})" for j in out[:8]))
    assert out.size <= own_tol_outliers
    return L, h2, st


def test_every_entry_of_the_headline_matrix(blmm):
    """BASELINE.json configs[1]: all 260 M LODs of the BXD-shaped null-exact bulkscan."""
    Y, G, K, _ = make_data(n=79, p=7321, m=35554, seed=20241)
    L, h2, st = run_case(blmm, Y, G, K, None, "configs[1] null-exact", own_tol_outliers=int(0.0005 * 35554))
    # the layout under test really had both classes, both regions and several segments
    col, width, cnt = blmm.default_context().lowrank_columns(35554)
    assert (col >= 0).all() and len(np.unique(col)) == 35554
    assert cnt[0] + cnt[2] == st.lowrank_shared and cnt[2] + cnt[3] > 0 and min(cnt) >= 0
    segs = np.searchsorted(EDGES, h2[h2 > 1e-12], side="right") - 1
    assert len(np.unique(segs)) >= 4
    # the same call WITHOUT the matrix (blmm_bulkscan_reduced: the scan kernels reduce in their epilogues, both panel regions, both
    # classes): per-trait maxima / arg-maxima and the LOD > 5 triplets, bit for bit those of the stored matrix
    red = blmm.bulkscan_reduced(Y, G, K, method="null-exact", threshold=5.0)
    assert red["route"] == 1 and np.array_equal(red["h2_null_list"], h2)
    arg = np.argmax(L, axis=0)
    assert np.array_equal(red["max_lod"], L[arg, np.arange(L.shape[1])]) and np.array_equal(red["argmax"], arg)
    ti, tj, tl = red["triplets"]
    assert ti.size == int((L > 5.0).sum()) and np.array_equal(tl, L[ti, tj]) and bool((tl > 5.0).all())
    assert np.array_equal(np.lexsort((ti, tj)), np.arange(ti.size)) and len(set(zip(ti.tolist(), tj.tolist()))) == ti.size
    print(f"  reduced call: {ti.size} triplets with LOD > 5; largest peak {red['max_lod'].max():.3f}")


def test_every_entry_with_two_null_covariates(blmm):
    """c = 2 (k_scan_lr3<2>: phase 2 in chunks, a 2 x 2 L^-1 per trait), enough traits for two panel regions."""
    Y, G, K, Cov = make_data(n=79, p=7321, m=12000, seed=20247, ncov=1)
    run_case(blmm, Y, G, K, Cov, "BXD shape, c = 2, m = 12000", own_tol_outliers=8)


def test_every_entry_of_the_config2_shard(blmm):
    """BASELINE.json configs[2], one of 8 shards: n = 500, p = 50000, m = 2500 (single weight basis, k_scan_lr at two waves,
    the divide-and-conquer eigensolver, k_rotate_big)."""
    Y, G, K, _ = make_data(n=500, p=50000, m=2500, seed=20242, bxd=False)
    run_case(blmm, Y, G, K, None, "configs[2] shard null-exact", own_tol_outliers=4)


def test_every_entry_with_three_covariates(blmm):
    """c = 3 (k_scan_lr3<3>), two panel regions as the c = 2 case."""
    Y, G, K, Cov = make_data(n=79, p=7321, m=12000, seed=20248, ncov=2)
    run_case(blmm, Y, G, K, Cov, "BXD shape, c = 3, m = 12000", own_tol_outliers=8)


def test_every_entry_with_weights_reml_and_prior(blmm):
    """Weights (W Y, W G, W [1 Covar], W K W), REML and the prior (1.0, 0.1): the C oracle on the pre-scaled inputs."""
    Y, G, K, Cov = make_data(n=79, p=7321, m=12000, seed=20249, ncov=1)
    w = np.random.default_rng(20249).uniform(0.5, 2.0, 79)
    run_case(blmm, Y, G, K, Cov, "BXD shape, weights + REML + prior (1.0, 0.1), m = 12000", own_tol_outliers=8, weights=w,
             prior=(1.0, 0.1), reml=True)


# ---- the grid methods and the permutation test: the oracles of oracle/grid_ref.py --------------------------------------------
GRID16 = [i / 16.0 for i in range(16)]


def grid_choices_ties_only(h2_dev, pick, Ell, grid, what):
    grid = list(grid)
    bad = np.flatnonzero(h2_dev != pick)
    for j in bad:                                 # only a tie in the oracle's own table may resolve differently
        gi = grid.index(float(h2_dev[j]))
        top = Ell[:, j].max()
        assert abs(Ell[gi, j] - top) <= 1e-12 * max(1.0, abs(top)), (what, j, h2_dev[j], pick[j])
    print(f"  {what}: {bad.size} of {pick.size} grid choices differ from the oracle's (all ties)")


def test_every_entry_of_config3_null_grid(blmm):
    """BASELINE.json configs[3], null-grid: all 260 M LODs against the C oracle at the device's grid choice."""
    from oracle import grid_ref as R
    Y, G, K, _ = make_data(n=79, p=7321, m=35554, seed=20241)
    t0 = time.time()
    g = blmm.bulkscan_null_grid(Y, G, K, GRID16)
    t1 = time.time()
    Lref, pick, Ell = R.null_grid(Y, G, K, GRID16, h2=g.h2_null_list)
    print(f"configs[3] null-grid: GPU call {t1 - t0:.2f} s, oracle {time.time() - t1:.2f} s")
    nbad, _, at = compare_every_entry(g.L, Lref, "configs[3] null-grid")
    print(f"  worst entry: grid value {g.h2_null_list[at[1]]}, trait mod 32 = {at[1] % 32}, marker mod 128 = {at[0] % 128}")
    grid_choices_ties_only(g.h2_null_list, pick, Ell, GRID16, "configs[3] null-grid")
    assert nbad == 0


def test_every_entry_of_config3_alt_grid(blmm):
    """BASELINE.json configs[3], alt-grid (k_scan_alt): all 260 M LODs at 1e-6 |ref| + 1e-10 against the composed oracle (16 C passes,
    the NumPy Ell table, tmax!'s fold), and every h2_panel entry equal to the oracle's or tied in its logL1 to 1e-12 relative."""
    from oracle import grid_ref as R
    Y, G, K, _ = make_data(n=79, p=7321, m=35554, seed=20241)
    t0 = time.time()
    a = blmm.bulkscan_alt_grid(Y, G, K, GRID16)
    t1 = time.time()
    Lref, panel, mism = R.alt_grid(Y, G, K, GRID16, dev_panel=a.h2_panel, block=2048)
    print(f"configs[3] alt-grid: GPU call {t1 - t0:.2f} s, oracle {time.time() - t1:.2f} s")
    nbad, _, at = compare_every_entry(a.L, Lref, "configs[3] alt-grid")
    i, j = at
    print(f"  worst entry: winning grid index {GRID16.index(float(a.h2_panel[i, j]))} (oracle {GRID16.index(float(panel[i, j]))}), "
          f"trait mod 32 = {j % 32}, marker mod 128 = {i % 128}")
    worst_gap = max([gp for *_, gp in mism], default=0.0)
    print(f"  h2_panel: {len(mism)} of {panel.size} entries differ from the oracle's; largest logL1 gap between the two {worst_gap:.2e}")
    assert worst_gap <= 1e-12
    assert nbad == 0


def test_every_entry_of_config2_shard_null_grid(blmm):
    """BASELINE.json configs[2], one of 8 shards, null-grid on 0:0.1:0.9: all 125 M LODs."""
    from oracle import grid_ref as R
    Y, G, K, _ = make_data(n=500, p=50000, m=2500, seed=20242, bxd=False)
    grid = [i / 10.0 for i in range(10)]
    t0 = time.time()
    g = blmm.bulkscan_null_grid(Y, G, K, grid)
    t1 = time.time()
    Lref, pick, Ell = R.null_grid(Y, G, K, grid, h2=g.h2_null_list)
    print(f"configs[2] shard null-grid: GPU call {t1 - t0:.2f} s, oracle {time.time() - t1:.2f} s")
    nbad, _, _ = compare_every_entry(g.L, Lref, "configs[2] shard null-grid")
    grid_choices_ties_only(g.h2_null_list, pick, Ell, grid, "configs[2] shard null-grid")
    assert nbad == 0


def test_every_entry_of_config4_shard_permutations(blmm):
    """BASELINE.json configs[4], one of 8 shards: n = 1000, p = 100000, 1250 permutations.  fp64: all 1.25e8 L_perms and all 100,000
    `lod` at 1e-6 |ref| + 1e-10; fp32 (k_rotate_f32 and the fp32 matrix-core scan): all 1.25e8 at SURVEY's 1e-3 |ref| + 1e-4."""
    from oracle import grid_ref as R
    Y, G, K, _ = make_data(n=1000, p=100000, m=1, seed=20244, bxd=False)
    y = Y[:, 0].copy()
    n, p = G.shape
    pidx = O.make_perm_idx(1000, 1250, 44)
    t0 = time.time()
    g64 = blmm.scan(y, G, K, permutation_test=True, nperms=1250, perm_idx=pidx)
    g32 = blmm.scan(y, G, K, permutation_test=True, nperms=1250, perm_idx=pidx, perm_precision="f32")
    t1 = time.time()
    rot = blmm.transform_rotation(y.reshape(-1, 1), np.hstack([np.ones((n, 1)), G]), K, addIntercept=False)
    lod, Lp = R.perms(y, G, K, pidx, g64["h2_null"], rot)
    del rot
    print(f"configs[4] shard permutations: GPU calls {t1 - t0:.2f} s, oracle {time.time() - t1:.2f} s")
    nbad, _, _ = compare_every_entry(g64["L_perms"], Lp, "configs[4] L_perms fp64")
    assert nbad == 0
    assert_lod_close(g64["lod"], lod, what="configs[4] lod fp64")
    L32 = g32["L_perms"]
    bad32, worst32 = 0, 0.0
    for i0 in range(0, p, 8192):
        a = L32[i0:i0 + 8192].astype(np.float64); r = Lp[i0:i0 + 8192]
        err = np.abs(a - r)
        bad32 += int((~(err <= 1e-3 * np.abs(r) + 1e-4)).sum())
        worst32 = max(worst32, float((err / (1e-3 * np.abs(r) + 1e-4)).max()))
    print(f"configs[4] L_perms fp32: {Lp.size} entries; outside 1e-3|ref| + 1e-4: {bad32}; worst error / bound {worst32:.3e}")
    assert bad32 == 0


def test_every_entry_of_the_fused_pvalues(blmm):
    """configs[1] with output_pvals: every -log10 p the scan epilogues wrote against the device's own L through the df = 1 formula
    -log10 p = -(ln 2 + log_ndtr(-sqrt(2 ln10 L))) / ln 10 (equal to bulklmm_oracle.lod2log10p to 1e-13 on a sample, checked here),
    at 1e-10 relative.  A p-value written to the wrong column at a layout seam fails it."""
    from scipy.special import log_ndtr
    Y, G, K, _ = make_data(n=79, p=7321, m=35554, seed=20241)
    t0 = time.time()
    r = blmm.bulkscan(Y, G, K, method="null-exact", output_pvals=True)
    print(f"configs[1] fused p-values: GPU call {time.time() - t0:.2f} s")
    L, P = r["L"], r["log10Pvals_mat"]

    def ref(lod):
        return -(math.log(2.0) + log_ndtr(-np.sqrt(2.0 * math.log(10.0) * np.maximum(lod, 0.0)))) / math.log(10.0)

    smp = L[::37, ::101].ravel()
    o = O.lod2log10p(smp, 1)
    d = np.abs(ref(smp) - o)
    print(f"  vectorised formula against lod2log10p on {smp.size} sampled entries: worst |d| {d.max():.2e}")
    assert np.all(d <= 1e-13 * np.abs(o) + 1e-15)
    nbad, worst, at = 0, 0.0, (0, 0)
    for j0 in range(0, L.shape[1], 1024):
        pr = ref(L[:, j0:j0 + 1024]); pg = P[:, j0:j0 + 1024]
        err = np.abs(pg - pr)
        nbad += int((~(err <= 1e-10 * np.abs(pr) + 1e-14)).sum())
        rel = err / np.maximum(np.abs(pr), 1e-4)
        k = int(np.argmax(rel))
        if rel.flat[k] > worst:
            worst = float(rel.flat[k]); i, jj = np.unravel_index(k, rel.shape); at = (int(i), j0 + int(jj))
    print(f"configs[1] -log10 p: {P.size} entries; outside 1e-10 relative: {nbad}; worst relative error {worst:.3e} at marker {at[0]}, trait {at[1]}")
    assert nbad == 0
