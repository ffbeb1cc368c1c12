"""GPU checks of bulkscan_stepwise (blmm_bulkscan_stepwise).  The reference is the loop the call replaces, written here: round after
round the EXISTING bulkscan_cond with the table so far (padded to max_loci), the column maxima of its L under blmm_lod_colmax's rule
in NumPy, and the contract's selection rule.  Every output is compared bit for bit (np.array_equal; NaN slots equal NaN slots).  One
case is also held against the independent oracle of the conditional scan (tests/cond_ref.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from common import DevBuf, make_data
from cond_ref import bulkscan_cond_ref
from test_gpu_parity import _fuzz_case

pytestmark = pytest.mark.gpu

GRID = [i / 10.0 for i in range(10)]
METHODS = ["null-grid", "null-exact"]


def colmax(L):
    """blmm_lod_colmax's rule: the largest entry at its lowest row; NaN never; nothing above -inf: (-inf, -1)."""
    p, m = L.shape
    if p == 0:
        return np.full(m, -np.inf), np.full(m, -1, dtype=np.int64)
    V = np.where(np.isnan(L), -np.inf, L)
    arg = V.argmax(axis=0).astype(np.int64)            # the first of equal maxima
    mx = V[arg, np.arange(m)]
    arg[mx == -np.inf] = -1
    return mx, arg


def loop(blmm, Y, G, K, Cov=None, *, S, thr, method, cond_fn=None, **kw):
    """The forward selection on the host.  Counts are taken over the active traits: NaNs from the columns A_t of L_t; the rule's
    zeros and the guard's re-scans from bulkscan_cond on the active traits alone (a column depends on its trait only)."""
    m = Y.shape[1]
    T = np.full((m, S), -1, dtype=np.int64)
    out = {"loci": T, "lod": np.full((m, S + 1), np.nan), "argmax": np.full((m, S + 1), -1, dtype=np.int64),
           "h2": np.full((m, S + 1), np.nan), "nloci": np.zeros(m, dtype=np.int64), "active": np.zeros(S + 1, dtype=np.int64),
           "rounds": 0, "n_nan_lod": 0, "n_rule_zero": 0, "n_illcond_rescan": 0, "n_zero_norm": 0, "L": []}
    A = np.arange(m)
    cond_fn = cond_fn or blmm.bulkscan_cond
    for t in range(S + 1):
        if A.size == 0:
            break
        r = cond_fn(Y, G, K, T.copy(), Cov, method=method, return_status=True, **kw)
        L = r["L"]
        mx, arg = colmax(L)
        out["lod"][A, t] = mx[A]; out["argmax"][A, t] = arg[A]; out["h2"][A, t] = r["h2_null_list"][A]
        out["active"][t] = A.size; out["rounds"] = t + 1
        out["n_nan_lod"] += int(np.isnan(L[:, A]).sum())
        ra = r if A.size == m else cond_fn(Y[:, A], G, K, T[A], Cov, method=method, return_status=True, **kw)
        assert np.array_equal(ra["L"], L[:, A], equal_nan=True)              # the premise of the counts
        out["n_rule_zero"] += ra["n_rule_zero"]; out["n_illcond_rescan"] += ra["status"].n_illcond_rescan
        if t == 0:
            out["n_zero_norm"] = r["status"].n_zero_norm
        out["L"].append((A.copy(), L))
        if t == S:
            break
        sel = A[mx[A] > thr]
        T[sel, t] = arg[sel]; out["nloci"][sel] = t + 1
        A = sel
    out["n_cond_traits"] = int((out["nloci"] > 0).sum())
    return out


def same(got, ref, S):
    assert got["rounds"] == ref["rounds"], (got["rounds"], ref["rounds"])
    assert np.array_equal(got["active"], ref["active"]), (got["active"], ref["active"])
    for k in ("loci", "argmax", "nloci"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], ref[k]), k
    for k in ("lod", "h2"):
        assert got[k].shape == (ref[k].shape[0], S + 1)
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), k + ": NaN slots"
        ok = ~np.isnan(ref[k])
        assert np.array_equal(got[k][ok], ref[k][ok]), (k, float(np.abs(got[k][ok] - ref[k][ok]).max()))
    assert got["n_rule_zero"] == ref["n_rule_zero"] and got["n_cond_traits"] == ref["n_cond_traits"]
    if "status" in got:
        st = got["status"]
        assert st.n_nan_lod == ref["n_nan_lod"] and st.n_illcond_rescan == ref["n_illcond_rescan"]
        assert st.n_zero_norm == ref["n_zero_norm"]


def plant(Y, G, seed, groups):
    """Y with marker effects added: groups = [(traits, [effect sizes])], the markers drawn per trait."""
    rng = np.random.default_rng(seed)
    Y = Y.copy()
    for traits, effects in groups:
        for j in traits:
            for b, q in zip(effects, rng.choice(G.shape[1], size=len(effects), replace=False)):
                Y[:, j] += b * G[:, q]
    return Y


# ---- 1. planted loci ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_planted_loci(blmm, method):
    Y, G, K, _ = make_data(n=79, p=300, m=40, seed=611)
    Y = plant(Y, G, 612, [(range(0, 8), [3.0, 2.0, 1.4]), (range(8, 16), [2.5, 1.6]), (range(16, 24), [2.2])])
    ref = loop(blmm, Y, G, K, S=4, thr=3.0, method=method)
    print("nloci:", ref["nloci"].tolist(), "active:", ref["active"].tolist())
    assert (ref["nloci"] == 0).any() and (ref["nloci"] == 1).any() and (ref["nloci"] >= 2).any() and ref["active"][1] < 40
    got = blmm.bulkscan_stepwise(Y, G, K, max_loci=4, threshold=3.0, method=method, return_status=True)
    same(got, ref, 4)


# ---- 2. covariates, weights, REML, prior -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("ncov,S,thr,need", [(2, 2, 2.5, 2), (3, 4, 1.0, 4)])
def test_covariates_weights_reml_prior(blmm, method, ncov, S, thr, need):
    """c = 3, S = 2 and c = 4, S = 4 (eight design columns: the reducing scan's form for more than four)."""
    Y, G, K, Cov = make_data(n=79, p=200, m=36, seed=7100 + ncov, ncov=ncov)
    Y = plant(Y, G, 7200 + ncov, [(range(0, 10), [3.0, 2.4, 2.0, 1.7]), (range(10, 18), [2.5])])
    kw = dict(weights=np.random.default_rng(3).uniform(0.5, 2.0, 79), reml=True, prior_variance=1.3, prior_sample_size=0.2)
    ref = loop(blmm, Y, G, K, Cov, S=S, thr=thr, method=method, **kw)
    print("nloci:", ref["nloci"].tolist(), "active:", ref["active"].tolist())
    assert (ref["nloci"] >= need).any() and ref["active"][1] < 36
    got = blmm.bulkscan_stepwise(Y, G, K, Cov, max_loci=S, threshold=thr, method=method, return_status=True, **kw)
    same(got, ref, S)


# ---- 3. tile and slot edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 63, 64, 65, 129, 257])
@pytest.mark.parametrize("m", [1, 5, 127, 129])
def test_tile_and_slot_edges(blmm, p, m):
    Y, G, K, _ = make_data(n=79, p=p, m=m, seed=3000 * p + m)
    for method in METHODS:
        ref = loop(blmm, Y, G, K, S=2, thr=0.5, method=method)
        got = blmm.bulkscan_stepwise(Y, G, K, max_loci=2, threshold=0.5, method=method, return_status=True)
        same(got, ref, 2)


# ---- 4. the conditioning guard -------------------------------------------------------------------------------------------------------
def test_conditioning_guard(blmm):
    """tests/test_gpu_cond.py's construction (test_gpu_parity's ill-conditioned data, fuzz seed 201 case 237: n = 13, six of its seven
    covariates) with max_loci = 1 (eight columns), every trait through the re-scan (illcond_rho = 2), in chunks of 1, 3 and by the
    budget."""
    Y, G, K, Cov = _fuzz_case(13, 63, 15, 7, 237, 201)
    Cov = Cov[:, 1:]
    ctx = blmm.default_context()
    ctx.set_tuning("illcond_rho", 2)                            # (reset by the conftest fixture)
    ref = loop(blmm, Y, G, K, Cov, S=1, thr=0.3, method="null-exact")
    print("active:", ref["active"].tolist(), "re-scans:", ref["n_illcond_rescan"])
    assert ref["n_illcond_rescan"] > 0 and ref["active"][1] > 0
    outs = []
    for chunk in (1, 3, 0):
        ctx.set_tuning("cond_red_chunk", chunk)
        got = blmm.bulkscan_stepwise(Y, G, K, Cov, max_loci=1, threshold=0.3, method="null-exact", return_status=True)
        assert got["status"].n_illcond_rescan > 0
        same(got, ref, 1)
        outs.append(got)
    for o in outs[1:]:
        for k in ("loci", "lod", "argmax", "h2", "nloci"):
            assert np.array_equal(o[k], outs[0][k], equal_nan=True)


def test_conditioning_guard_at_its_own_threshold(blmm):
    """The same data with the guard's threshold at 0.05: some traits are flagged and some are not, so flagged and unflagged columns
    share a tile of the reducing scan."""
    Y, G, K, Cov = _fuzz_case(13, 63, 15, 7, 237, 201)
    Cov = Cov[:, 1:]
    blmm.default_context().set_tuning("illcond_rho", 0.05)
    ref = loop(blmm, Y, G, K, Cov, S=1, thr=0.3, method="null-exact")
    got = blmm.bulkscan_stepwise(Y, G, K, Cov, max_loci=1, threshold=0.3, method="null-exact", return_status=True)
    print("re-scans:", got["status"].n_illcond_rescan, "of", int(ref["active"].sum()))
    assert 0 < got["status"].n_illcond_rescan < ref["active"].sum()
    same(got, ref, 1)


def test_conditioning_guard_in_the_global_memory_slab(blmm):
    """n = 900 with c + S = 8 (intercept, four covariates, three loci): k_cond_qr's basis lives in its slab of global memory."""
    m, p = 12, 130
    Y, G, K, Cov = make_data(n=900, p=p, m=m, seed=90038, ncov=4)
    ctx = blmm.default_context()
    ctx.set_tuning("illcond_rho", 2)
    ref = loop(blmm, Y, G, K, Cov, S=3, thr=1.0, method="null-exact")
    print("active:", ref["active"].tolist())
    assert ref["n_illcond_rescan"] > m                          # more than round 0's
    for chunk in (1, 3, 0):
        ctx.set_tuning("cond_red_chunk", chunk)
        got = blmm.bulkscan_stepwise(Y, G, K, Cov, max_loci=3, threshold=1.0, method="null-exact", return_status=True)
        assert got["status"].n_illcond_rescan > 0
        same(got, ref, 3)


# ---- 5. stopping ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_an_infinite_threshold_is_one_round(blmm, method):
    Y, G, K, _ = make_data(n=79, p=150, m=33, seed=51)
    got = blmm.bulkscan_stepwise(Y, G, K, max_loci=3, threshold=np.inf, method=method)
    r = blmm.bulkscan_cond(Y, G, K, np.full((33, 3), -1), method=method)
    mx, arg = colmax(r["L"])
    assert got["rounds"] == 1 and got["active"].tolist() == [33, 0, 0, 0] and not got["nloci"].any() and (got["loci"] == -1).all()
    assert np.array_equal(got["lod"][:, 0], mx) and np.array_equal(got["argmax"][:, 0], arg)
    assert np.array_equal(got["h2"][:, 0], r["h2_null_list"])
    assert np.isnan(got["lod"][:, 1:]).all() and np.isnan(got["h2"][:, 1:]).all() and (got["argmax"][:, 1:] == -1).all()


def _host_abi(blmm, ctx, method):
    """The two host forms straight through the C ABI, intercept-only: the Python mirror raises on n_zero_norm as the reference does."""
    Lc = blmm._lib
    o = blmm.api._opts(Lc.BLMM_NULL_EXACT if method == "null-exact" else Lc.BLMM_NULL_GRID)
    grid = np.array(GRID)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def cond(Y, G, K, T, Cov=None, **kw):
        (n, m), p, s = Y.shape, G.shape[1], T.shape[1]
        Yf, Gf, Kf, Tc = np.asfortranarray(Y), np.asfortranarray(G), np.asfortranarray(K), np.ascontiguousarray(T, dtype=np.int64)
        L = np.empty((p, m), order="F"); h2 = np.empty(m); info = np.zeros(4, dtype=np.int64); st = Lc.blmm_status()
        rc = ctx.lib.blmm_bulkscan_cond(ctx.h, C.byref(o), vp(Yf), n, m, vp(Gf), p, None, 0, vp(Kf), None, vp(grid), 10, vp(Tc), s,
                                        vp(L), vp(h2), vp(info), C.byref(st))
        assert rc == 0, ctx_err(blmm, ctx)
        return {"L": L, "h2_null_list": h2, "n_rule_zero": int(info[0]), "status": st}

    def step(Y, G, K, S, thr):
        (n, m), p = Y.shape, G.shape[1]
        Yf, Gf, Kf = np.asfortranarray(Y), np.asfortranarray(G), np.asfortranarray(K)
        out = {"loci": np.empty((m, S), dtype=np.int64), "lod": np.empty((m, S + 1)), "argmax": np.empty((m, S + 1), dtype=np.int64),
               "h2": np.empty((m, S + 1)), "nloci": np.empty(m, dtype=np.int64)}
        info = np.zeros(Lc.BLMM_STEP_INFO_LEN, dtype=np.int64); st = Lc.blmm_status()
        rc = ctx.lib.blmm_bulkscan_stepwise(ctx.h, C.byref(o), vp(Yf), n, m, vp(Gf), p, None, 0, vp(Kf), None, vp(grid), 10, S, thr,
                                            vp(out["loci"]), vp(out["lod"]), vp(out["argmax"]), vp(out["h2"]), vp(out["nloci"]),
                                            vp(info), C.byref(st))
        assert rc == 0, ctx_err(blmm, ctx)
        out.update(rounds=int(info[0]), n_cond_traits=int(info[1]), n_rule_zero=int(info[2]), active=info[3:4 + S].copy(), status=st)
        return out
    return cond, step


@pytest.mark.parametrize("method", METHODS)
def test_threshold_zero_and_a_zero_trait(blmm, gpu_ctx, method):
    """threshold 0, S = 4: every trait with a positive peak goes on.  Trait 3 is constant at 0: a zero null residual, a NaN column,
    (-inf, -1) in round 0, no locus, counted in n_zero_norm; n_nan_lod is the loop's count over the active columns."""
    Y, G, K, _ = make_data(n=79, p=90, m=21, seed=52)
    Y[:, 3] = 0.0
    cond, step = _host_abi(blmm, gpu_ctx, method)
    ref = loop(blmm, Y, G, K, S=4, thr=0.0, method=method, cond_fn=cond)
    print("active:", ref["active"].tolist(), "NaN:", ref["n_nan_lod"], "zero norm:", ref["n_zero_norm"])
    assert ref["lod"][3, 0] == -np.inf and ref["argmax"][3, 0] == -1 and ref["nloci"][3] == 0
    assert ref["n_zero_norm"] >= 1 and ref["n_nan_lod"] >= 90 and ref["active"][4] > 0
    got = step(Y, G, K, 4, 0.0)
    same(got, ref, 4)
    assert got["lod"][3, 0] == -np.inf and got["argmax"][3, 0] == -1 and np.isnan(got["lod"][3, 1:]).all()
    with pytest.raises(blmm.BulkLMMError):                       # the mirror re-issues the reference's error for such a trait
        blmm.bulkscan_stepwise(Y, G, K, max_loci=4, threshold=0.0, method=method, ctx=gpu_ctx)


# ---- 6. ties and the rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_ties_and_the_rank_rule(blmm, method):
    Y, G, K, _ = make_data(n=79, p=120, m=9, seed=61)
    Y = plant(Y, G, 62, [(range(9), [2.5])])
    first = blmm.bulkscan_stepwise(Y, G, K, max_loci=1, threshold=np.inf, method=method)
    q = int(first["argmax"][0, 0])                              # trait 0's peak; copies of it in front of and behind everything
    assert 0 <= q < 120
    G2 = np.hstack([G[:, [q]], G, G[:, [q]]])
    ref = loop(blmm, Y, G2, K, S=2, thr=1.0, method=method)
    got = blmm.bulkscan_stepwise(Y, G2, K, max_loci=2, threshold=1.0, method=method, return_status=True)
    same(got, ref, 2)
    assert got["nloci"][0] >= 1 and got["loci"][0, 0] == 0      # the lowest of the three equal columns
    assert 0 in ref["L"][1][0]
    L1 = ref["L"][1][1][:, 0]                                   # trait 0's column of round 1
    for i in (0, q + 1, 121):
        assert L1[i] == 0.0 and not np.signbit(L1[i])
    assert got["argmax"][0, 1] not in (0, q + 1, 121) and (got["loci"][0] == 0).sum() == 1
    assert got["n_rule_zero"] == ref["n_rule_zero"] >= 3


# ---- 7. against the independent oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_against_the_oracle_of_the_conditional_scan(blmm, method):
    Y, G, K, Cov = make_data(n=79, p=110, m=10, seed=71, ncov=1)
    Y = plant(Y, G, 72, [(range(0, 6), [2.8, 1.8])])
    S = 2
    got = blmm.bulkscan_stepwise(Y, G, K, Cov, max_loci=S, threshold=2.0, method=method)
    assert got["active"][1] > 0
    T = np.full((10, S), -1, dtype=np.int64)
    for t in range(got["rounds"]):
        act = np.flatnonzero(~np.isnan(got["h2"][:, t]))
        assert act.size == got["active"][t]
        L = bulkscan_cond_ref(Y, G, K, T, Covar=Cov, h2=got["h2"][:, t], traits=act.tolist())[0]
        for j in act:
            ref = float(np.nanmax(L[:, j]))
            assert abs(got["lod"][j, t] - ref) <= 1e-6 * abs(ref) + 1e-10, (t, j, got["lod"][j, t], ref)
        if t < S:
            T[:, t] = got["loci"][:, t]


# ---- 8. the C ABI: refusals in the same order in both forms, the _dev form ------------------------------------------------------------
def _abi(blmm, ctx, dev, opts, n, m, p, Cov, ncov, S, thr, bufs, sinfo=True, status=None):
    f = ctx.lib.blmm_bulkscan_stepwise_dev if dev else ctx.lib.blmm_bulkscan_stepwise
    grid = np.array(GRID)
    return f(ctx.h, None if opts is None else C.byref(opts), bufs[0], n, m, bufs[1], p, Cov, ncov, bufs[2], None,
             grid.ctypes.data_as(C.c_void_p), 10, S, thr, bufs[3], bufs[4], bufs[5], bufs[6], bufs[7], bufs[8] if sinfo else None,
             None if status is None else C.byref(status))


@pytest.mark.parametrize("dev", [False, True])
def test_refusals_through_the_c_abi(blmm, gpu_ctx, dev):
    """Nothing is dereferenced before the refusals: every buffer is a small live allocation of the right kind anyway."""
    Lc = blmm._lib
    n, m, p = 12, 3, 6
    host = [np.zeros(4096) for _ in range(9)]
    dbuf = [DevBuf(nbytes=4096 * 8) for _ in range(9)] if dev else []
    bufs = [C.c_void_p(b.ptr) for b in dbuf] if dev else [h.ctypes.data_as(C.c_void_p) for h in host]
    err = lambda: ctx_err(blmm, gpu_ctx)
    o = blmm.api._opts(Lc.BLMM_NULL_GRID)
    alt = blmm.api._opts(Lc.BLMM_ALT_GRID)
    unk = blmm.api._opts(Lc.BLMM_NULL_GRID); unk.method = 77
    cases = [
        ((alt, n, 0, 0, -1.0), -1, "max_loci must be at least 1"),
        ((alt, n, 0, 5, -1.0), -10, "at most 4 loci per trait"),
        ((unk, n, 7, 1, -1.0), -10, "more than 8 null-design columns"),
        ((unk, n, 0, 2, float("nan")), -1, "the threshold must be"),
        ((unk, n, 0, 2, -0.5), -1, "the threshold must be"),
        ((unk, 2049, 0, 2, 1.0), -5, "Unknown method"),
        ((alt, 2049, 0, 2, 1.0), -10, "alt-grid is not supported"),
        ((o, 2049, 0, 2, 1.0), -10, "more than 2048 individuals"),
        ((o, 5, 0, 4, 1.0), -2, "Dimension mismatch."),
    ]
    try:
        for (opts, nn, ncov, S, thr), code, msg in cases:
            rc = _abi(blmm, gpu_ctx, dev, opts, nn, m, p, bufs[0] if ncov else None, ncov, S, thr, bufs)
            assert rc == code and msg in err(), (rc, err(), msg)
        for miss in (0, 1, 2, 3, 4, 5, 6, 7):
            b = list(bufs); b[miss] = None
            rc = _abi(blmm, gpu_ctx, dev, o, n, m, p, None, 0, 2, 1.0, b)
            assert rc == -1 and "NULL buffer" in err(), (miss, rc, err())
        # a pending -log10 p request is refused and consumed
        assert gpu_ctx.lib.blmm_set_log10p_output(gpu_ctx.h, None, 0, 1) == 0
        rc = _abi(blmm, gpu_ctx, dev, o, n, m, p, None, 0, 2, 1.0, bufs)
        assert rc == -1 and "blmm_set_log10p_output request is pending" in err()
    finally:
        for b in dbuf:
            b.free()
    Y, G, K, _ = make_data(n=79, p=40, m=5, seed=81)
    r = blmm.bulkscan_stepwise(Y, G, K, max_loci=1, threshold=1.0, ctx=gpu_ctx)       # the request is gone: this one runs
    assert r["rounds"] >= 1


def ctx_err(blmm, ctx):
    return blmm.load().blmm_last_error(ctx.h).decode()


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("status", [True, False])
def test_dev_form_through_the_c_abi(blmm, gpu_ctx, method, status):
    """Device buffers between guard words; equal to the host form; sinfo_out = NULL is accepted; without a status the results are
    there after blmm_synchronize; no matrix is left for blmm_last_dims."""
    Lc = blmm._lib
    n, p, m, S, thr = 79, 131, 37, 3, 2.0
    Y, G, K, _ = make_data(n=n, p=p, m=m, seed=82)
    Y = plant(Y, G, 83, [(range(0, 12), [2.6, 1.9])])
    host = blmm.bulkscan_stepwise(Y, G, K, max_loci=S, threshold=thr, method=method, ctx=gpu_ctx)
    assert host["active"][1] > 0
    blmm.bulkscan(Y[:, :2], G, K, ctx=gpu_ctx)                   # leaves a resident matrix behind
    pp, mm = C.c_int64(-5), C.c_int64(-5)
    assert gpu_ctx.lib.blmm_last_dims(gpu_ctx.h, C.byref(pp), C.byref(mm)) == 0 and (pp.value, mm.value) == (p, 2)
    GI, GF = -424242, -12345.5
    shapes = [(m * S, np.int64), (m * (S + 1), np.float64), (m * (S + 1), np.int64), (m * (S + 1), np.float64), (m, np.int64),
              (Lc.BLMM_STEP_INFO_LEN, np.int64)]
    ins = [DevBuf(Y.T), DevBuf(G.T), DevBuf(K)]
    outs = [DevBuf(np.full(cnt + 2, GI if dt == np.int64 else GF, dtype=dt)) for cnt, dt in shapes]
    o = blmm.api._opts(Lc.BLMM_NULL_EXACT if method == "null-exact" else Lc.BLMM_NULL_GRID)
    st = Lc.blmm_status()
    try:
        bufs = [C.c_void_p(b.ptr) for b in ins] + [C.c_void_p(b.ptr + 8) for b in outs]
        rc = _abi(blmm, gpu_ctx, True, o, n, m, p, None, 0, S, thr, bufs, sinfo=status, status=st if status else None)
        assert rc == 0, ctx_err(blmm, gpu_ctx)
        gpu_ctx.synchronize()
        raw = [b.get(cnt + 2, dtype=dt) for b, (cnt, dt) in zip(outs, shapes)]
    finally:
        for b in ins + outs:
            b.free()
    for a, (cnt, dt) in zip(raw, shapes):
        g = GI if dt == np.int64 else GF
        assert a[0] == g and a[-1] == g, "a guard word was overwritten"
    loci, lod, arg, h2, nloci, info = [a[1:-1] for a in raw]
    got = {"loci": loci.reshape(m, S), "lod": lod.reshape(m, S + 1), "argmax": arg.reshape(m, S + 1), "h2": h2.reshape(m, S + 1),
           "nloci": nloci}
    for k in got:
        assert np.array_equal(got[k], host[k], equal_nan=True), k
    if status:
        assert info[0] == host["rounds"] and info[1] == host["n_cond_traits"] and info[2] == host["n_rule_zero"]
        assert info[3:4 + S].tolist() == host["active"].tolist() and info[4 + S:].tolist() == [0] * (4 - S)
    else:
        assert (info == GI).all()
    pp, mm = C.c_int64(-5), C.c_int64(-5)
    assert gpu_ctx.lib.blmm_last_dims(gpu_ctx.h, C.byref(pp), C.byref(mm)) != 0          # no resident matrix


def test_torch_wrapper_in_its_own_process():
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "helpers", "stepwise_dev_check.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "stepwise_dev ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
