"""The shortened front of a single null-exact call on the fast eigen route:

  * the weight basis is built behind k_eigf_pairs, from the solver's raw eigenvalues ranked by the basis kernel itself, ahead of the
    eigen phase's end (n <= 80: the register-resident basis kernel); where the device rejects the fast path, a second launch behind
    the Jacobi rebuilds the basis from the final eigenvalues;
  * the traits are rotated inside k_brent (four lanes per trait: n <= 80), by k_rotate's own wave code, instead of by a launch of
    their own.

Shapes: n = 8, 12, 79, 80 (the last n of both) and 81 (the control: neither part runs); m = 1, 17, 130 (a lone column, a ragged
wave, a ragged workgroup of the in-workgroup repack form) and 1100 (the two-kernel form, its last workgroup partly empty, and a
workgroup of padding columns only); p = 25; c = 1, 2, 3; one case with weights (folded into the rotation), one with decomp = "svd"
(the other rank rule); two with numerically repeated eigenvalues (duplicated individuals at n = 79; at n = 12 the identity with
six of its twelve eigenvalues moved apart, since under the identity itself every heritability gives the same weights, every trait
lands in the shared-weights class and the basis is never read), where the Jacobi runs and the basis is rebuilt.

Every case is checked three ways: (a) the default build in this process, which reports through blmm_last_front_route that the new
route ran (bits 0 and 1; bit 3 exactly where the Jacobi ran, as it must in the two fallback cases; none at n = 81); (b) a fresh
child process with the developer switches BLMM_EARLY_WB=0 BLMM_FUSE_ROT=0 on the same inputs: L, h2 and -- at
c = 1, m = 130 -- -log10 p, peaks and arg-maxima must be np.array_equal; (c) every entry against the C oracle at the device's heritabilities, at the bound of
tests/test_gpu_fullmatrix.py.  A case must not pass by missing the code: no trait re-scanned by the guards, and with m >= 130 at
least 65 traits in the rank-R class, the two fallback cases included: the basis rebuilt from the Jacobi's eigenvalues is what their
scans read; the seeds are such that the CPU oracle's own search gives h2 > 0.05 for that many traits, which is checked on the CPU
before the GPU runs."""
import ctypes as C
import functools
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from common import DevBuf, make_data

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-6, 1e-10           # tests/test_gpu_fullmatrix.py
P = 25
MIN_RANK_R = 65
EARLY_WB, FUSED_ROT, WB_REBUILT = 1, 2, 8
HERE = os.path.dirname(os.path.abspath(__file__))

# tests/common.make_data seeds: (n, m, c) -> seed
SEEDS = {(8, 1, 1): 5100, (8, 17, 1): 5100, (8, 130, 1): 5106, (8, 1100, 1): 5100,
         (12, 1, 1): 5100, (12, 17, 1): 5100, (12, 130, 1): 5120, (12, 1100, 1): 5100,
         (79, 1, 1): 5101, (79, 17, 1): 5100, (79, 130, 1): 5102, (79, 1100, 1): 5100,
         (80, 1, 1): 5101, (80, 17, 1): 5213, (80, 130, 1): 5100, (80, 1100, 1): 5100,
         (81, 1, 1): 5100, (81, 17, 1): 5157, (81, 130, 1): 5100, (81, 1100, 1): 5100,
         (12, 130, 2): 5108, (12, 130, 3): 5116, (12, 1100, 2): 5101, (12, 1100, 3): 5100,
         (79, 130, 2): 5105, (79, 130, 3): 5105, (79, 1100, 2): 5100, (79, 1100, 3): 5100,
         (80, 130, 2): 5100, (80, 130, 3): 5100, (80, 1100, 2): 5100, (80, 1100, 3): 5100,
         (81, 130, 2): 5100, (81, 130, 3): 5100}
# (n, m, c, kind)
CASES = [k + ("plain",) for k in sorted(SEEDS)] + [(79, 130, 1, "weights"), (79, 130, 1, "svd"), (79, 130, 1, "duplicated"),
                                                   (12, 130, 1, "identity")]
FALLBACK = ("duplicated", "identity")


def case_id(case):
    return "n%d-m%d-c%d-%s" % case


@functools.lru_cache(maxsize=None)
def case_data(case):
    """(Y, G, K, Covar, weights)"""
    n, m, c, kind = case
    if kind == "duplicated":           # individuals 0 .. 5 identical: six equal rows and columns of K, a five-fold eigenvalue at zero
        rng = np.random.Generator(np.random.PCG64(515))
        Y, G, _, _ = make_data(n=n, p=P, m=m, seed=9100, bxd=False)
        G[1:6] = G[0]
        X = G - 0.5
        K = np.round(2.0 * (X @ X.T) / P + 0.5, 12)
        Y[1:6] += 0.1 * rng.standard_normal((5, m))
        return Y, G, K, None, None
    if kind == "identity":             # Q diag(1, 1, 1, 1, 1, 1, 1.75, 2.5, .. 5.5) Q': a six-fold eigenvalue at one, six distinct ones
        rng = np.random.Generator(np.random.PCG64(9200))
        _, G, _, _ = make_data(n=n, p=P, m=m, seed=9200)
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        d = np.ones(n)
        d[6:] += 0.75 * np.arange(1, n - 5)
        K = (Q * d) @ Q.T
        h2 = rng.uniform(0.5, 0.95, size=m)    # traits with this kinship as their genetic covariance
        Y = (Q * np.sqrt(d)) @ rng.standard_normal((n, m)) * np.sqrt(h2 / (1 - h2)) + rng.standard_normal((n, m)) + 10.0
        return Y, G, 0.5 * (K + K.T), None, None
    Y, G, K, Cov = make_data(n=n, p=P, m=m, seed=SEEDS[(n, m, c)], ncov=c - 1)
    w = np.random.Generator(np.random.PCG64(77)).uniform(0.5, 2.0, size=n) if kind == "weights" else None
    return Y, G, K, Cov, w


def oracle_inputs(case):
    """The case as the C oracle takes it: weights w scale the rows of Y, G and the design (the intercept becomes the column w) and
    both sides of K."""
    Y, G, K, Cov, w = case_data(case)
    if w is None:
        return Y, G, K, Cov, True
    return w[:, None] * Y, w[:, None] * G, K * np.outer(w, w), w[:, None].copy(), False


def bulkscan(blmm, ctx, case, pvals=False):
    """blmm_bulkscan through the package's argument plumbing: (L, h2, status[, -log10 p]) without turning counters into warnings."""
    A, L = blmm.api, blmm.api.L
    Y, G, K, Cov, w = case_data(case)
    Y, G, K, n, m, p = A._host_arrays(Y, G, K)
    cov, ncov, w, add = A._host_covariates(Cov, w, n, True)
    o = A._opts(L.BLMM_NULL_EXACT, False, add, "svd" if case[3] == "svd" else "eigen", 1, 1.0, 0.0, 0)
    Lout, h2, st = np.empty((p, m), order="F"), np.empty(m), L.blmm_status()
    with A._log10p_output(ctx, 1 if pvals else None):
        ctx.check(ctx.lib.blmm_bulkscan(ctx.h, C.byref(o), A._p(Y), n, m, A._p(G), p, A._p(cov), ncov, A._p(K), A._p(w), None, 0,
                                        A._p(Lout), A._p(h2), C.byref(st)))
    if pvals:
        return Lout, h2, st, A._last_log10p(ctx, Lout.shape, 1)
    return Lout, h2, st


def reduced_dev(blmm, ctx, case):
    """blmm_bulkscan_reduced_dev (c = 1) on device copies: (peak LOD, its marker, h2, route)."""
    Y, G, K, _, _ = case_data(case)
    n, m = Y.shape
    o = blmm.api._opts(blmm._lib.BLMM_NULL_EXACT)
    bufs = [DevBuf(np.asfortranarray(x).ravel("F")) for x in (Y, G, K)] + [DevBuf(nbytes=8 * m) for _ in range(3)]
    dY, dG, dK, dmx, dax, dh2 = bufs
    r = blmm._lib.blmm_reduced(dmx.ptr, dax.ptr, 0, 0.0, 0, None, None, None, None)
    ctx.check(ctx.lib.blmm_bulkscan_reduced_dev(ctx.h, C.byref(o), dY.ptr, n, m, dG.ptr, P, None, 0, dK.ptr, None, None, 0, C.byref(r),
                                                dh2.ptr, None))
    ctx.synchronize()
    out = dmx.get(m), dax.get(m, np.int64), dh2.get(m), int(ctx.lib.blmm_last_reduced_route(ctx.h))
    for b in bufs:
        b.free()
    return out


def run_case(blmm, ctx, case):
    """Every output of one case from the library as this process loaded it, with the route its front took."""
    n, m, c, kind = case
    L, h2, st = bulkscan(blmm, ctx, case)
    route = int(ctx.lib.blmm_last_front_route(ctx.h))
    shared, prof = ctx.lowrank_profile()
    out = {"L": L, "h2": h2, "front": route, "sweeps": int(st.jacobi_sweeps), "rank": int(st.lowrank_rank),
           "fallback": int(st.lowrank_fallback) + int(st.n_illcond_rescan), "shared": int(st.lowrank_shared),
           "rank_r": sum(t for t, _ in prof), "ranks": [r for t, r in prof if t]}
    if c == 1 and m == 130 and kind == "plain":
        Lp, h2p, stp, lp = bulkscan(blmm, ctx, case, pvals=True)
        out.update(L_pv=Lp, h2_pv=h2p, log10p=lp, front_pv=int(ctx.lib.blmm_last_front_route(ctx.h)))
        out["fallback"] += int(stp.lowrank_fallback) + int(stp.n_illcond_rescan)
        out["max_lod"], out["argmax"], out["h2_red"], out["route"] = reduced_dev(blmm, ctx, case)
        out["front_red"] = int(ctx.lib.blmm_last_front_route(ctx.h))
    return out


def child_main(path):
    """The child of `old_front`: every case on the path the change replaces (the environment of this process selects it)."""
    sys.path.insert(0, os.path.dirname(HERE))
    import bulklmm_jl_amd as blmm
    blmm.load()
    ctx = blmm.Context(0)
    res = {case: run_case(blmm, ctx, case) for case in CASES}
    ctx.close()
    with open(path, "wb") as f:
        pickle.dump(res, f)


@pytest.fixture(scope="module")
def old_front(tmp_path_factory):
    """All cases once in a fresh process with both parts switched off (developer switches: read only with BLMM_DEV_ENV=1)."""
    path = str(tmp_path_factory.mktemp("front_chain") / "old_front.pkl")
    env = dict(os.environ, BLMM_DEV_ENV="1", BLMM_EARLY_WB="0", BLMM_FUSE_ROT="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, cwd=HERE,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(path, "rb") as f:
        return pickle.load(f)


@pytest.fixture(scope="module")
def ctx(blmm):
    c = blmm.Context(0)
    yield c
    c.close()


def assert_every_entry(L, Lref, what):
    err = np.abs(L - Lref)
    bad = ~(err <= RTOL * np.abs(Lref) + ATOL)
    rel = err / np.maximum(np.abs(Lref), 1e-4)
    print(f"{what}: {L.size} entries, outside {RTOL}|ref| + {ATOL}: {int(bad.sum())}, worst relative error {rel.max():.3e}")
    assert np.isfinite(L).all() and not bad.any(), what


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_front_chain_against_the_old_front_and_the_oracle(blmm, ctx, old_front, case):
    from oracle import cref
    n, m, c, kind = case
    oY, oG, oK, oCov, oInt = oracle_inputs(case)
    if m >= 130:
        # on the CPU, before the GPU runs: the oracle's own search puts enough traits well inside the rank-R class
        _, h2cpu = cref.bulkscan_null(oY, oG, oK, oCov, addIntercept=oInt)
        assert int((h2cpu > 0.05).sum()) >= MIN_RANK_R, int((h2cpu > 0.05).sum())
    got, ref = run_case(blmm, ctx, case), old_front[case]
    print(f"{case_id(case)}: front route {got['front']} (old front: {ref['front']}), jacobi sweeps {got['sweeps']}, rank-R traits "
          f"{got['rank_r']} (ranks {got['ranks']}), shared-weights {got['shared']}, re-scanned {got['fallback']}")
    # (a) the new route ran here and not in the child
    want = (EARLY_WB | FUSED_ROT) if n <= 80 else 0
    if kind in FALLBACK:
        assert got["sweeps"] > 0 and ref["sweeps"] > 0, "the fast path's checks passed: this kinship does not exercise the fallback"
    if got["sweeps"] > 0 and n <= 80:     # the device rejected the fast path (it does on some of the small synthetic kinships too)
        want |= WB_REBUILT
    assert got["front"] == want and ref["front"] == 0 and got["sweeps"] == ref["sweeps"]
    if "front_pv" in got:
        assert got["front_pv"] == want and got["front_red"] == want
    # neither run passed by missing the code
    for r in (got, ref):
        assert r["fallback"] == 0 and r["rank_r"] + r["shared"] == m
        if m >= 130:
            assert r["rank_r"] >= MIN_RANK_R
    assert got["rank_r"] == ref["rank_r"] and got["ranks"] == ref["ranks"] and got["rank"] == ref["rank"]
    # (b) bit for bit the old front's
    for k in [k for k in got if isinstance(got[k], np.ndarray)]:
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), (k, int((got[k] != ref[k]).sum()))
    # (c) every entry against the C oracle at the device's heritabilities
    Lref, _ = cref.bulkscan_null(oY, oG, oK, oCov, addIntercept=oInt, h2_override=got["h2"], skip_search=True)
    assert_every_entry(got["L"], Lref, "L")
    if "L_pv" in got:
        from oracle import bulklmm_oracle as O
        assert got["route"] == 1 and ref["route"] == 1       # the fused route: the peaks came out of the scan's epilogue
        assert np.array_equal(got["L_pv"], got["L"]) and np.array_equal(got["h2_pv"], got["h2"]) and np.array_equal(got["h2_red"], got["h2"])
        arg = np.argmax(got["L"], axis=0)
        assert np.array_equal(got["argmax"], arg) and np.array_equal(got["max_lod"], got["L"][arg, np.arange(m)])
        pref = O.lod2log10p(np.maximum(got["L"], 0.0).ravel(), 1).reshape(got["L"].shape)
        perr = np.abs(got["log10p"] - pref)
        assert (perr <= 1e-10 * np.abs(pref) + 1e-14).all(), float(perr.max())


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    child_main(sys.argv[1])
