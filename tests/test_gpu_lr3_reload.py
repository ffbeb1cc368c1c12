"""k_scan_lr3 with each operand requested again right behind the last MFMA that reads it (kernels_scan.hip): the smallest shapes that
reach every edge of its two K loops.

  n = 8, 12, 79      ks = 2, 4, 20 steps of the numerator loop (one trip and its peeled last step; several), weight bases of rank <= 8 at
                     n = 8 and ~20 at n = 79 (KR = 1 .. 2 and 5 .. 6 steps per chunk of the other loop: the peeled last step alone, loop + it)
  m = 130            two rank-R trait tiles, the second ragged, with perm = -1 padding columns
  p = 25, 129        one marker tile whose second wave is wholly out of range; two marker tiles
  c = 1, 2, 3        covariates incl. the intercept: chunks of four (c = 1) and of two marker blocks (c = 2, 3)

and at c = 1 also with the -log10 p output (the PV instantiation) and through blmm_bulkscan_reduced_dev (the RED instantiation).

Every case is checked three ways: (a) the default kernel in this process; (b) a fresh child process (BLMM_DEV_ENV=1 BLMM_LR3=0) that
runs the two-wave kernel k_scan_lr on the same inputs -- the kernels claim "same arithmetic per output, same bits", so L, h2, -log10 p,
peaks and arg-maxima must be np.array_equal; (c) every entry against the C oracle at the device's heritabilities, at the bound of
tests/test_gpu_fullmatrix.py.  A case must not pass by missing the kernel: no trait re-scanned by the guards and at least 65 traits
in the rank-R class (so that the second trait tile exists); the seeds are such that the CPU oracle's own search gives h2 > 0.05 for
at least that many traits, which is checked on the CPU before the GPU runs."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from common import DevBuf, make_data

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-6, 1e-10           # tests/test_gpu_fullmatrix.py
M = 130
MIN_RANK_R = 65
# tests/common.make_data seeds: (n, p, c) -> seed
SEEDS = {(8, 25, 1): 5106, (8, 25, 2): 5106, (8, 25, 3): 5106, (8, 129, 1): 5147, (8, 129, 2): 5131, (8, 129, 3): 5104,
         (12, 25, 1): 5120, (12, 25, 2): 5108, (12, 25, 3): 5116, (12, 129, 1): 5109, (12, 129, 2): 5109, (12, 129, 3): 5102,
         (79, 25, 1): 5102, (79, 25, 2): 5105, (79, 25, 3): 5105, (79, 129, 1): 5100, (79, 129, 2): 5100, (79, 129, 3): 5101}
CASES = sorted(SEEDS)
HERE = os.path.dirname(os.path.abspath(__file__))


def case_data(case):
    n, p, c = case
    return make_data(n=n, p=p, m=M, seed=SEEDS[case], ncov=c - 1)


def reduced_dev(blmm, ctx, Y, G, K):
    """blmm_bulkscan_reduced_dev (c = 1) on device copies: (peak LOD, its marker, h2, route)."""
    n, m = Y.shape
    p = G.shape[1]
    o = blmm.api._opts(blmm._lib.BLMM_NULL_EXACT)
    bufs = [DevBuf(np.asfortranarray(x).ravel("F")) for x in (Y, G, K)] + [DevBuf(nbytes=8 * m) for _ in range(3)]
    dY, dG, dK, dmx, dax, dh2 = bufs
    r = blmm._lib.blmm_reduced(dmx.ptr, dax.ptr, 0, 0.0, 0, None, None, None, None)
    ctx.check(ctx.lib.blmm_bulkscan_reduced_dev(ctx.h, C.byref(o), dY.ptr, n, m, dG.ptr, p, None, 0, dK.ptr, None, None, 0, C.byref(r),
                                                dh2.ptr, None))
    ctx.synchronize()
    out = dmx.get(m), dax.get(m, np.int64), dh2.get(m), int(ctx.lib.blmm_last_reduced_route(ctx.h))
    for b in bufs:
        b.free()
    return out


def run_case(blmm, ctx, case):
    """Every output of one case from the library as this process loaded it, with what the low-rank form executed."""
    Y, G, K, Cov = case_data(case)
    ex = blmm._lib.BLMM_NULL_EXACT
    L, h2, st = blmm.api._bulkscan_call(ex, Y, G, K, Cov, None, True, None, 1.0, 0.0, False, 1, "eigen", 0, ctx, return_status=True)
    shared, prof = ctx.lowrank_profile()
    out = {"L": L, "h2": h2, "fallback": int(st.lowrank_fallback) + int(st.n_illcond_rescan), "shared": int(st.lowrank_shared),
           "rank_r": sum(t for t, _ in prof), "ranks": [r for t, r in prof if t]}
    if case[2] == 1:
        Lp, h2p, stp = blmm.api._bulkscan_call(ex, Y, G, K, Cov, None, True, None, 1.0, 0.0, False, 1, "eigen", 0, ctx, return_status=True,
                                               pvals_df=1)
        out.update(L_pv=Lp, h2_pv=h2p, log10p=blmm.api._last_log10p(ctx, Lp.shape, 1))
        out["fallback"] += int(stp.lowrank_fallback) + int(stp.n_illcond_rescan)
        out["max_lod"], out["argmax"], out["h2_red"], out["route"] = reduced_dev(blmm, ctx, Y, G, K)
    return out


def child_main(path):
    """The child of `two_wave`: every case through k_scan_lr (the environment of this process selects it)."""
    sys.path.insert(0, os.path.dirname(HERE))
    import bulklmm_jl_amd as blmm
    blmm.load()
    ctx = blmm.Context(0)
    res = {case: run_case(blmm, ctx, case) for case in CASES}
    ctx.close()
    with open(path, "wb") as f:
        pickle.dump(res, f)


@pytest.fixture(scope="module")
def two_wave(tmp_path_factory):
    """All cases once in a fresh process with BLMM_LR3=0 (developer switch: read only with BLMM_DEV_ENV=1)."""
    path = str(tmp_path_factory.mktemp("lr3") / "two_wave.pkl")
    env = dict(os.environ, BLMM_DEV_ENV="1", BLMM_LR3="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, cwd=HERE)
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


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d-p%d-c%d" % c)
def test_reloaded_loops_against_the_two_wave_kernel_and_the_oracle(blmm, ctx, two_wave, case):
    from oracle import cref
    n, p, c = case
    Y, G, K, Cov = case_data(case)
    # on the CPU, before the GPU runs: the oracle's own search puts enough traits well inside the rank-R class
    _, h2cpu = cref.bulkscan_null(Y, G, K, Cov)
    assert int((h2cpu > 0.05).sum()) >= MIN_RANK_R, int((h2cpu > 0.05).sum())
    got, ref = run_case(blmm, ctx, case), two_wave[case]
    print(f"n {n} p {p} c {c}: rank-R traits {got['rank_r']} (ranks {got['ranks']}), shared-weights {got['shared']}, re-scanned {got['fallback']}")
    for r in (got, ref):                       # neither run passed by missing its kernel
        assert r["fallback"] == 0 and r["rank_r"] >= MIN_RANK_R and r["rank_r"] + r["shared"] == M
    assert got["rank_r"] == ref["rank_r"] and got["ranks"] == ref["ranks"]
    # (b) bit for bit the two-wave kernel's
    keys = ["L", "h2"] + (["L_pv", "h2_pv", "log10p", "max_lod", "argmax", "h2_red"] if c == 1 else [])
    for k in keys:
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), (k, int((got[k] != ref[k]).sum()))
    # (c) every entry against the C oracle at the device's heritabilities
    Lref, _ = cref.bulkscan_null(Y, G, K, Cov, h2_override=got["h2"])
    assert_every_entry(got["L"], Lref, "L")
    if c == 1:
        from oracle import bulklmm_oracle as O
        assert got["route"] == 1 and ref["route"] == 1       # the fused route: the peaks came out of the scan's epilogue
        assert np.array_equal(got["L_pv"], got["L"]) and np.array_equal(got["h2_pv"], got["h2"]) and np.array_equal(got["h2_red"], got["h2"])
        arg = np.argmax(got["L"], axis=0)
        assert np.array_equal(got["argmax"], arg) and np.array_equal(got["max_lod"], got["L"][arg, np.arange(M)])
        # -log10 p against the oracle's lod2log10p of the device's own L at 1e-10 relative, as test_every_entry_of_the_fused_pvalues does
        pref = O.lod2log10p(np.maximum(got["L"], 0.0).ravel(), 1).reshape(got["L"].shape)
        perr = np.abs(got["log10p"] - pref)
        assert (perr <= 1e-10 * np.abs(pref) + 1e-14).all(), float(perr.max())


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    child_main(sys.argv[1])
