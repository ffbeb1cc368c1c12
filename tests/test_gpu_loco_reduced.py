"""The reduced leave-one-chromosome-out bulkscan on the GPU (blmm_bulkscan_loco_reduced).

Its contract is stated against the matrix blmm_bulkscan_loco writes under the same opts, tuning and inputs, bit for bit:
    max_lod / argmax        = lod_colmax(L)
    chr_max_lod[c] / chr_argmax[c]  = lod_colmax(L[rows_c]), the arg-max + chr_start[c] (a global marker; -1 stays -1)
    triplets                = lod_threshold(L, thr)      (the exact count; with a small cap, `cap` distinct members of that set)
    h2_null_list            = bulkscan_loco's
The reference reductions run on the library's own lod_colmax / lod_threshold over bulkscan_loco(...)["L"]."""
import ctypes as C
import json
import os
import time

import numpy as np
import pytest

from common import GOLDEN, DevBuf, make_geno

pytestmark = pytest.mark.gpu

GRID = [i / 10.0 for i in range(10)]


def bxd_runs():
    fx = json.load(open(os.path.join(GOLDEN, "bxd_chr_runs.json")))
    return [lab for lab, k in zip(fx["chromosomes"], fx["counts"]) for _ in range(k)]


def equal_runs(p, nchr):
    b = np.linspace(0, p, nchr + 1).round().astype(int)
    return [str(c + 1) for c in range(nchr) for _ in range(b[c + 1] - b[c])]


def traits(G, m, seed, h2=0.5):
    """m traits with a polygenic background of heritability ~h2 over every marker, plus a mean of 10 (as test_gpu_loco.py)."""
    rng = np.random.default_rng(seed)
    n, p = G.shape
    X = (G - G.mean(0)) / np.maximum(G.std(0), 1e-6)
    g = X @ rng.standard_normal((p, m)) / np.sqrt(p)
    g /= g.std(0)
    return 10.0 + np.sqrt(h2) * g + np.sqrt(1.0 - h2) * rng.standard_normal((n, m))


def check(blmm, full, red, thr, ctx=None, alt=False):
    """Every output of the reduced call against the reductions of the LOCO matrix."""
    L = full["L"]
    cs = full["chr_start"]
    assert red["chromosomes"] == full["chromosomes"] and np.array_equal(red["chr_start"], cs)
    mx, arg = blmm.lod_colmax(L, ctx)
    assert np.array_equal(red["max_lod"], mx) and np.array_equal(red["argmax"], arg)
    nchr = len(cs) - 1
    assert red["chr_max_lod"].shape == (nchr, L.shape[1]) and red["chr_argmax"].shape == (nchr, L.shape[1])
    for c in range(nchr):
        cm, ca = blmm.lod_colmax(L[cs[c]:cs[c + 1]], ctx)
        ca = np.where(ca >= 0, ca + cs[c], -1)
        assert np.array_equal(red["chr_max_lod"][c], cm), c
        assert np.array_equal(red["chr_argmax"][c], ca), c
    if thr is not None:
        i, j, lod = blmm.lod_threshold(L, thr, ctx)
        ri, rj, rl = red["triplets"]
        assert np.array_equal(ri, i) and np.array_equal(rj, j) and np.array_equal(rl, lod)
    if alt:
        assert "h2_null_list" not in red
    else:
        assert np.array_equal(red["h2_null_list"], full["h2_null_list"])


def fused_route(red):
    st = red["status"]
    return 3 if st.lowrank_fallback > 0 or st.n_illcond_rescan > 0 else 1


def last_dims(ctx):
    pp, mm = C.c_int64(-1), C.c_int64(-1)
    rc = ctx.lib.blmm_last_dims(ctx.h, C.byref(pp), C.byref(mm))
    return rc, pp.value, mm.value


# ---- 1. methods, covariates, routes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["null-exact", "null-grid", "alt-grid"])
def test_bxd_runs_every_method(blmm, method):
    rng = np.random.default_rng(121)
    chrom = bxd_runs()[::5]                          # the 20 runs of the real map, 1465 markers
    G = make_geno(79, len(chrom), rng)
    m = 600 if method == "alt-grid" else 3000
    Y = traits(G, m, 122)
    ctx = blmm.Context(0)
    full = blmm.bulkscan_loco(Y, G, chrom, method=method, h2_grid=GRID, ctx=ctx)
    assert last_dims(ctx)[1:] == (G.shape[1], m)     # bulkscan_loco left its matrix resident ...
    red = blmm.bulkscan_loco_reduced(Y, G, chrom, method=method, h2_grid=GRID, threshold=2.5, ctx=ctx, return_status=True)
    assert last_dims(ctx) == (-1, 0, 0)              # ... the reduced call leaves none, whichever route ran
    assert len(red["triplets"][0]) > 0
    check(blmm, full, red, 2.5, ctx, alt=method == "alt-grid")
    assert red["route"] == (2 if method == "alt-grid" else fused_route(red))
    ctx.close()


@pytest.mark.parametrize("method", ["null-exact", "null-grid"])
def test_covariates_weights_reml(blmm, method):
    rng = np.random.default_rng(131)
    chrom = equal_runs(900, 5)
    G = make_geno(79, 900, rng)
    Y = traits(G, 200, 132)
    Cov = rng.standard_normal((79, 2))
    Y += Cov @ rng.standard_normal((2, 200))
    w = rng.uniform(0.5, 2.0, 79)
    kw = dict(method=method, h2_grid=GRID, weights=w, reml=True, prior_sample_size=0.1, kinship_digits=12)
    full = blmm.bulkscan_loco(Y, G, chrom, Cov, **kw)
    red = blmm.bulkscan_loco_reduced(Y, G, chrom, Cov, threshold=2.0, return_status=True, **kw)
    check(blmm, full, red, 2.0)
    assert red["route"] in (1, 3)


@pytest.mark.parametrize("case", ["c4", "exact_full_rank"])
def test_resident_route(blmm, case):
    """No fused instantiation: every chromosome through the resident block of the largest chromosome's rows (route 2)."""
    rng = np.random.default_rng(141)
    chrom = equal_runs(1100, 6)
    G = make_geno(79, 1100, rng)
    Y = traits(G, 300, 142)
    ctx = blmm.Context(0)
    kw = {"ctx": ctx}
    if case == "c4":
        Cov = rng.standard_normal((79, 3))
        Y += Cov @ rng.standard_normal((3, 300))
        kw["Covar"] = Cov
    else:
        ctx.set_tuning("exact_full_rank", 1)
    full = blmm.bulkscan_loco(Y, G, chrom, method="null-exact", **kw)
    for _ in range(2):                               # the second call reuses the workspace of the first
        red = blmm.bulkscan_loco_reduced(Y, G, chrom, method="null-exact", threshold=2.0, **kw)
        assert last_dims(ctx) == (-1, 0, 0)          # the block of the last chromosome is not served as a whole-genome matrix
        assert red["route"] == 2
        check(blmm, full, red, 2.0, ctx)             # (lod_colmax on a host matrix leaves that matrix resident)
    ctx.close()


@pytest.mark.parametrize("ncov,key,value,field", [(0, "lr_tol", 0.0, "lowrank_fallback"),
                                                  (2, "illcond_rho", 2.0, "n_illcond_rescan")])
def test_every_trait_flagged_is_rescanned_on_the_device(blmm, ncov, key, value, field):
    """lr_tol = 0 flags every trait for k_scan_fix, illcond_rho = 2 puts every trait on the conditioning guard's list (k_scan_qr):
    route 3, the same results, and no second run."""
    rng = np.random.default_rng(151 + ncov)
    chrom = equal_runs(1000, 4)
    G = make_geno(79, 1000, rng)
    Y = traits(G, 250, 152)
    Cov = None
    if ncov:
        Cov = rng.standard_normal((79, ncov))
        Y += Cov @ rng.standard_normal((ncov, 250))
    ctx = blmm.Context(0)
    ctx.set_tuning(key, value)
    if ncov:
        ctx.set_tuning("lr_tol", 0.0)                # both guards: k_scan_fix, then k_scan_qr over the same traits
    full = blmm.bulkscan_loco(Y, G, chrom, Cov, method="null-exact", ctx=ctx)
    red = blmm.bulkscan_loco_reduced(Y, G, chrom, Cov, method="null-exact", threshold=2.0, ctx=ctx, return_status=True)
    assert red["route"] == 3
    assert getattr(red["status"], field) == 4 * 250          # every trait of every chromosome
    if ncov:
        assert red["status"].lowrank_fallback == 4 * 250
    check(blmm, full, red, 2.0, ctx)
    ctx.close()


@pytest.mark.parametrize("n,p,nchr", [(124, 1200, 6), (300, 1500, 4), (1000, 2000, 3)])
def test_sizes(blmm, n, p, nchr):
    rng = np.random.default_rng(n + 7)
    chrom = equal_runs(p, nchr)
    G = make_geno(n, p, rng)
    Y = traits(G, 150, n + 8)
    for method in ("null-exact", "null-grid"):
        full = blmm.bulkscan_loco(Y, G, chrom, method=method, h2_grid=GRID)
        red = blmm.bulkscan_loco_reduced(Y, G, chrom, method=method, h2_grid=GRID, threshold=2.0)
        check(blmm, full, red, 2.0)


# ---- 2. edge cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["null-exact", "null-grid"])
def test_nan_lods_and_an_all_nan_chromosome(blmm, monkeypatch, method):
    """All-zero markers have no norm: their LODs are NaN (null-grid also counts them as zero-norm markers, which the host wrappers
    raise as the reference does -- switched off here, the comparison is of the numbers).  Chromosome "3" holds only such markers:
    its table row is -inf / -1; elsewhere NaN is never a maximum."""
    monkeypatch.setattr(blmm.api, "_raise_status", lambda st: None)
    rng = np.random.default_rng(161)
    chrom = ["1"] * 300 + ["2"] * 250 + ["3"] * 40 + ["4"] * 310
    G = make_geno(79, 900, rng)
    G[:, 300 + 250:300 + 250 + 40] = 0.0
    G[:, [5, 77, 400]] = 0.0
    Y = traits(G, 160, 162)
    full = blmm.bulkscan_loco(Y, G, chrom, method=method, h2_grid=GRID)
    L = full["L"]
    assert np.isnan(L[550:590]).all() and np.isnan(L[[5, 77, 400]]).all()
    red = blmm.bulkscan_loco_reduced(Y, G, chrom, method=method, h2_grid=GRID, threshold=1.5)
    check(blmm, full, red, 1.5)
    assert np.all(np.isneginf(red["chr_max_lod"][2])) and np.all(red["chr_argmax"][2] == -1)
    assert np.all(np.isfinite(red["max_lod"]))


def test_duplicate_markers_tie_to_the_lowest_global_index(blmm):
    rng = np.random.default_rng(171)
    chrom = equal_runs(800, 4)
    G = make_geno(79, 800, rng)
    q, d = 250, 330                                  # both on chromosome 2 (rows 200 .. 399)
    G[:, d] = G[:, q]
    Y = traits(G, 64, 172)
    Y[:, :16] += 2.0 * (G[:, [q]] - G[:, q].mean()) / G[:, q].std()
    full = blmm.bulkscan_loco(Y, G, chrom, method="null-exact")
    assert np.array_equal(full["L"][q], full["L"][d])
    red = blmm.bulkscan_loco_reduced(Y, G, chrom, method="null-exact", threshold=3.0)
    check(blmm, full, red, 3.0)
    assert np.all(red["chr_argmax"][1][:16] == q) and np.all(red["argmax"][:16] == q)


def _raw_call(blmm, ctx, Y, G, cs, thr, cap, method=0):
    """blmm_bulkscan_loco_reduced with a fixed cap (the Python wrapper would retry with the count)."""
    Y = np.asfortranarray(Y); G = np.asfortranarray(G)
    n, m = Y.shape
    p = G.shape[1]
    nchr = len(cs) - 1
    mx = np.empty(m); arg = np.empty(m, dtype=np.int64); h2 = np.empty((nchr, m))
    ii = np.empty(max(cap, 1), dtype=np.int32); jj = np.empty(max(cap, 1), dtype=np.int32); ll = np.empty(max(cap, 1))
    cnt = C.c_int64(-1)
    r = blmm._lib.blmm_reduced(mx.ctypes.data, arg.ctypes.data, 1, float(thr), cap, ii.ctypes.data, jj.ctypes.data, ll.ctypes.data,
                               C.addressof(cnt))
    o = blmm.api._opts(method)
    rc = ctx.lib.blmm_bulkscan_loco_reduced(ctx.h, C.byref(o), Y.ctypes.data, n, m, G.ctypes.data, p, cs.ctypes.data, nchr, -1, None, 0,
                                            None, None, 0, C.byref(r), None, None, h2.ctypes.data, None)
    k = min(max(cnt.value, 0), cap)
    return rc, cnt.value, (ii[:k], jj[:k], ll[:k]), mx, arg


def test_cap_below_the_count(blmm):
    rng = np.random.default_rng(181)
    chrom = equal_runs(700, 3)
    G = make_geno(79, 700, rng)
    Y = traits(G, 120, 182)
    ctx = blmm.Context(0)
    full = blmm.bulkscan_loco(Y, G, chrom, method="null-exact", ctx=ctx)
    i, j, lod = blmm.lod_threshold(full["L"], 1.0, ctx)
    assert len(i) > 500
    cs = full["chr_start"]
    for cap in (0, 37, 500):
        rc, cnt, (ti, tj, tl), mx, arg = _raw_call(blmm, ctx, Y, G, cs, 1.0, cap)
        assert rc == 0 and cnt == len(i)
        assert len(ti) == cap
        pairs = set(zip(ti.tolist(), tj.tolist()))
        assert len(pairs) == cap                              # distinct
        ref = {(a, b): v for a, b, v in zip(i.tolist(), j.tolist(), lod.tolist())}
        assert all((a, b) in ref and ref[(a, b)] == v for a, b, v in zip(ti.tolist(), tj.tolist(), tl.tolist()))
        m0, a0 = blmm.lod_colmax(full["L"], ctx)
        assert np.array_equal(mx, m0) and np.array_equal(arg, a0)
    ctx.close()


def test_one_trait_and_no_hits(blmm):
    rng = np.random.default_rng(191)
    chrom = bxd_runs()[::9]
    G = make_geno(79, len(chrom), rng)
    Y = traits(G, 1, 192)
    for method in ("null-exact", "null-grid", "alt-grid"):
        full = blmm.bulkscan_loco(Y, G, chrom, method=method, h2_grid=GRID)
        red = blmm.bulkscan_loco_reduced(Y, G, chrom, method=method, h2_grid=GRID, threshold=1e6)
        assert red["max_lod"].shape == (1,) and red["chr_max_lod"].shape == (20, 1)
        assert len(red["triplets"][0]) == 0
        check(blmm, full, red, 1e6, alt=method == "alt-grid")


# ---- 3. the entry point's other promises ---------------------------------------------------------------------------------------
def test_pending_log10p_request_is_refused_and_consumed(blmm):
    rng = np.random.default_rng(201)
    chrom = equal_runs(400, 2)
    G = make_geno(79, 400, rng)
    Y = traits(G, 30, 202)
    ctx = blmm.Context(0)
    full = blmm.bulkscan_loco(Y, G, chrom, method="null-exact", ctx=ctx)
    dP = DevBuf(np.full(400 * 30, -7.0))
    assert ctx.lib.blmm_set_log10p_output(ctx.h, dP.ptr, 400, 1) == 0
    with pytest.raises(blmm.BulkLMMError) as e:
        blmm.bulkscan_loco_reduced(Y, G, chrom, method="null-exact", ctx=ctx)
    assert e.value.code == -1 and "log10p" in e.value.msg
    red = blmm.bulkscan_loco_reduced(Y, G, chrom, method="null-exact", threshold=2.0, ctx=ctx)   # the request is gone
    check(blmm, full, red, 2.0, ctx)
    ctx.synchronize()
    assert np.all(dP.get(400 * 30) == -7.0)
    dP.free()
    ctx.close()


def test_dev_form_equals_the_host_form(blmm):
    """blmm_bulkscan_loco_reduced_dev on resident inputs, with the kinships passed in or not (device buffers through the HIP runtime,
    as test_gpu_loco.py:test_loco_dev_form)."""
    rng = np.random.default_rng(211)
    n, p, m = 79, 701, 90
    chrom = equal_runs(p, 4)
    G = make_geno(n, p, rng)
    Y = traits(G, m, 212)
    ctx = blmm.Context(0)
    _, cs = blmm.chromosome_runs(chrom, p)
    Kl = blmm.calcKinship_loco(G, chrom, ctx=ctx)
    dY, dG, dK = DevBuf(Y.T), DevBuf(G.T), DevBuf(np.ascontiguousarray(Kl))
    grid = np.asarray(GRID)
    cap = 1 << 14
    for method, code in (("null-grid", blmm._lib.BLMM_NULL_GRID), ("null-exact", blmm._lib.BLMM_NULL_EXACT)):
        host = blmm.bulkscan_loco_reduced(Y, G, chrom, method=method, h2_grid=GRID, threshold=2.0, ctx=ctx)
        o = blmm.api._opts(code)
        for K, want_status in ((None, True), (dK, False)):
            dmx, darg = DevBuf(nbytes=8 * m), DevBuf(nbytes=8 * m)
            dcm, dca, dh = DevBuf(nbytes=8 * 4 * m), DevBuf(nbytes=8 * 4 * m), DevBuf(nbytes=8 * 4 * m)
            di, dj, dl, dc = DevBuf(nbytes=4 * cap), DevBuf(nbytes=4 * cap), DevBuf(nbytes=8 * cap), DevBuf(nbytes=8)
            r = blmm._lib.blmm_reduced(dmx.ptr, darg.ptr, 1, 2.0, cap, di.ptr, dj.ptr, dl.ptr, dc.ptr)
            st = blmm._lib.blmm_status()
            ctx.check(ctx.lib.blmm_bulkscan_loco_reduced_dev(ctx.h, C.byref(o), dY.ptr, n, m, dG.ptr, p, cs.ctypes.data, 4, -1, None, 0,
                                                             None, grid.ctypes.data, grid.size, None if K is None else K.ptr, C.byref(r),
                                                             dcm.ptr, dca.ptr, dh.ptr, C.byref(st) if want_status else None))
            ctx.synchronize()
            assert ctx.lib.blmm_last_reduced_route(ctx.h) == (host["route"] if want_status else 0)
            assert np.array_equal(dmx.get(m), host["max_lod"]) and np.array_equal(darg.get(m, np.int64), host["argmax"])
            assert np.array_equal(dcm.get((4, m)), host["chr_max_lod"]) and np.array_equal(dca.get((4, m), np.int64), host["chr_argmax"])
            assert np.array_equal(dh.get((4, m)), host["h2_null_list"])
            k = int(dc.get(1, np.int64)[0])
            assert k == len(host["triplets"][0])
            ti, tj, tl = di.get(k, np.int32), dj.get(k, np.int32), dl.get(k)
            order = np.lexsort((ti, tj))
            assert np.array_equal(ti[order], host["triplets"][0]) and np.array_equal(tj[order], host["triplets"][1])
            assert np.array_equal(tl[order], host["triplets"][2])
            for b in (dmx, darg, dcm, dca, dh, di, dj, dl, dc):
                b.free()
    for b in (dY, dG, dK):
        b.free()
    ctx.close()


def test_planted_qtl_is_its_chromosomes_peak(blmm):
    rng = np.random.default_rng(221)
    chrom = bxd_runs()
    G = make_geno(79, len(chrom), rng)
    _, cs = blmm.chromosome_runs(chrom, G.shape[1])
    q = int(cs[4] + 200)                             # on chromosome 5
    Y = traits(G, 32, 222)
    Y[:, :8] += 3.0 * (G[:, [q]] - G[:, q].mean()) / G[:, q].std()
    red = blmm.bulkscan_loco_reduced(Y, G, chrom, method="null-exact")
    assert np.all(red["chr_argmax"][4][:8] == q) and np.all(red["argmax"][:8] == q)
    others = np.delete(np.arange(20), 4)
    assert np.all(red["chr_max_lod"][4][:8] > red["chr_max_lod"][others][:, :8].max(0))


def test_full_bxd_shape(blmm):
    rng = np.random.default_rng(231)
    chrom = bxd_runs()
    G = make_geno(79, len(chrom), rng)
    Y = traits(G, 35554, 232)
    ctx = blmm.Context(0)
    full = blmm.bulkscan_loco(Y, G, chrom, method="null-exact", ctx=ctx, return_status=True)
    t0 = time.time()
    red = blmm.bulkscan_loco_reduced(Y, G, chrom, method="null-exact", threshold=4.0, ctx=ctx, return_status=True)
    print(f"bulkscan_loco_reduced BXD shape (host to host, first call): {time.time() - t0:.3f} s, route {red['route']}")
    check(blmm, full, red, 4.0, ctx)
    assert red["route"] == fused_route(red)
    for k in ("n_nan_lod", "n_zero_norm", "lowrank_fallback", "n_illcond_rescan", "n_h2_boundary"):
        assert getattr(red["status"], k) == getattr(full["status"], k), k
    ctx.close()
