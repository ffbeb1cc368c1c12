"""scan(...; permutation_test=True, perm_precision="f32") at its tile edges, every L_perms entry held to the derived error bound of
tests/f32_ref.py (the module docstring there has the derivation) against the oracle on the device's own rotation and h2.

Shapes are a covering design: every n, p and nperms of the lists below appears with a small and with a large partner, so that the
paddings (npad = n rounded to 8, kpad to 128, ldrr to 16), the 256-marker and 128-permutation tiles, a last group of fewer than 8
permutation tiles and a remainder in xcd_swizzle32 (p = 2600: 11 scan and 22 rotate workgroups per row of tiles) are all reached.
Routes: c = 1 rotates G on the fp32 matrix cores (k_rotate_f32, isx from the fp32 columns); c >= 2 or tuning f32_rotation = 0
converts the fp64 rotated markers (k_cvt_f32).  `lod` is fp64 on both: held to 1e-6 |ref| + 1e-10 on the fp64 route and, on the
own route (fp64 numerator, norms from the fp32 columns), to test_gpu_strong_signal.py's conditioning-aware form.

Each case prints its worst error / bound and where that entry sits."""
import ctypes as C
import math

import numpy as np
import pytest

import f32_ref as F
from common import ATOL, RTOL, DevBuf, assert_lod_close, kinship_of, make_geno
from oracle import bulklmm_oracle as O

pytestmark = pytest.mark.gpu

INVALID = -1
NS = [5, 8, 9, 16, 17, 79, 127, 128, 129, 256, 257, 1023, 1024, 2048]
PS = [1, 2, 127, 128, 129, 255, 256, 257]
MS = [1, 2, 127, 128, 129, 1025, 2047]
# n_i with (p, nperms) = (PS[i % 8], MS[(i + 3) % 7]) and (PS[(i + 4) % 8], MS[i % 7]): every p and every nperms meets both an
# n <= 129 and an n >= 256, and every n two different shapes
SHAPES = [(n, PS[i % 8], MS[(i + 3) % 7]) for i, n in enumerate(NS)] + [(n, PS[(i + 4) % 8], MS[i % 7]) for i, n in enumerate(NS)]
SHAPES.append((79, 2600, 129))


def data(n, p, seed, ncov=0, weights=False):
    rng = np.random.default_rng(seed)
    G = make_geno(n, p, rng)
    G[0], G[1] = 0.0, 1.0                        # no constant marker at tiny n
    K = kinship_of(make_geno(n, 200, rng))
    y = 10.0 + 0.8 * G[:, p // 2] + rng.standard_normal(n)
    Cov = rng.standard_normal((n, ncov)) if ncov else None
    if ncov:
        y = y + Cov @ rng.standard_normal(ncov)
    w = rng.uniform(0.5, 1.5, n) if weights else None
    return y, G, K, Cov, w


def oracle(y, G, K, Cov, w, Ut, lam, h2, pidx, **kw):
    """scan_perms_lite on the device's rotation (uncentred: U' W [y | 1 Cov G]) at the device's h2."""
    n = y.shape[0]
    Z = np.ones((n, 1)) if Cov is None else np.hstack([np.ones((n, 1)), Cov])
    W = np.ones(n) if w is None else w
    rot = (Ut @ (W * y), Ut @ (W[:, None] * np.hstack([Z, G])), lam)
    return O.scan(y, G, K, covar=Z, addIntercept=False, weights=w, permutation_test=True, nperms=pidx.shape[1], perm_idx=pidx,
                  h2_override=h2, rotation_override=rot, **kw)


def check_perms(what, got, ref, op, own):
    """Every entry within the derived bound (entries whose bound is infinite -- |r| + Dr >= 1 -- are counted, not compared) and
    within the fp32 contract 1e-3 |ref| + 1e-4; prints the worst error / bound and where it sits."""
    got = np.asarray(got, dtype=np.float64)
    b = op.bound(own)
    err = np.abs(got - ref)
    fin = np.isfinite(b)
    ratio = np.where(fin, err / b, 0.0)
    print(f"{what}: worst error / bound {ratio.max():.3g} at {F.locate(ratio, op)}; median {np.median(ratio):.3g}; "
          f"{int((~fin).sum())} entries without a bound")
    assert np.isfinite(got).all()
    assert np.all(err[fin] <= b[fin]), f"{what}: {int((err[fin] > b[fin]).sum())} entries beyond the bound"
    assert np.all(err <= 1e-3 * np.abs(ref) + 1e-4)
    return ratio.max()


def check_lod(what, lod, ref, n, own):
    if not own:
        assert_lod_close(lod, ref, what=f"{what}: lod")
        return
    u = 10.0 ** (-2.0 * ref / n)
    b32 = RTOL * np.abs(ref) + ATOL + (n / math.log(10.0)) * 1e-6 * (1.0 - u) / u
    assert np.all(np.abs(lod - ref) <= b32), f"{what}: lod, worst {float(np.max(np.abs(lod - ref) / b32)):.3g} of the bound"


def run(blmm, n, p, nperms, seed, ncov=0, weights=False, reml=False, prior=(0.0, 0.0), rotation=1, ctx=None):
    """One fp32 permutation scan on supplied permutations, held against the oracle.  Returns the device's result."""
    y, G, K, Cov, w = data(n, p, seed, ncov, weights)
    pidx = O.make_perm_idx(n, nperms, seed + 1)
    ctx = ctx or blmm.default_context()
    ctx.set_tuning("f32_rotation", rotation)          # (the conftest fixture resets the default context's tuning)
    got = blmm.scan(y, G, K, Cov, weights=w, reml=reml, prior_variance=prior[0], prior_sample_size=prior[1], permutation_test=True,
                    nperms=nperms, perm_idx=pidx, perm_precision="f32", ctx=ctx)
    assert got["L_perms"].dtype == np.float32 and got["L_perms"].shape == (p, nperms)
    Ut, lam = F.device_rotation(blmm, K, w, ctx)
    h2 = got["h2_null"]
    ref = oracle(y, G, K, Cov, w, Ut, lam, h2, pidx, reml=reml, prior_variance=prior[0], prior_sample_size=prior[1])
    op = F.Operands(y, G, Ut, lam, h2, pidx, Covar=Cov, weights=w)
    own = ncov == 0 and rotation == 1
    what = (f"n {n} p {p} nperms {nperms} c {ncov + 1}{' weights' if weights else ''}{' reml' if reml else ''}"
            f"{' prior' if prior[1] else ''} {'own' if own else 'fp64'} rotation")
    check_perms(what, got["L_perms"], ref["L_perms"], op, own)
    check_lod(what, got["lod"], ref["lod"], n, own)
    return got


@pytest.mark.parametrize("n,p,nperms", SHAPES)
def test_shapes_own_rotation(blmm, n, p, nperms):
    run(blmm, n, p, nperms, seed=7000 + n + p + nperms)


@pytest.mark.parametrize("n,p,nperms", [(8, 129, 2), (79, 257, 129), (257, 2600, 1025), (1024, 255, 128), (2048, 128, 127)])
def test_shapes_fp64_rotation(blmm, n, p, nperms):
    """c = 1 with tuning f32_rotation = 0: the converted fp64 rotated markers."""
    run(blmm, n, p, nperms, seed=7100 + n, rotation=0)


@pytest.mark.parametrize("ncov,n,p,nperms", [(1, 257, 129, 129), (2, 79, 257, 1025), (3, 128, 256, 127), (7, 17, 255, 128),
                                             (7, 1023, 2, 2047), (31, 79, 129, 129)])
def test_covariates(blmm, ncov, n, p, nperms):
    """c = 2, 3, 4, 8 and 32 (CMAX, the largest the single-trait scan takes): the fp64 rotation route."""
    run(blmm, n, p, nperms, seed=7200 + ncov, ncov=ncov)


@pytest.mark.parametrize("ncov,weights,reml,prior,n", [(0, True, False, (0.0, 0.0), 79), (0, False, True, (1.0, 0.1), 257),
                                                       (2, True, False, (0.0, 0.0), 129), (1, True, True, (1.0, 0.1), 1023)])
def test_weights_reml_prior(blmm, ncov, weights, reml, prior, n):
    run(blmm, n, 257, 129, seed=7300 + n, ncov=ncov, weights=weights, reml=reml, prior=prior)


@pytest.mark.parametrize("n,ncov", [(79, 0), (256, 2), (257, 0), (1000, 0), (1000, 2)])
def test_library_rng(blmm, n, ncov):
    """The library's own permutations (n > 256: generated on the side stream, the multi-kernel panel): the fp64 L_perms of the same
    seed is the reference, with the bound plus 1e-6 |ref|; the fp64 result itself matches the oracle on the host's replay of the
    generator (f32_ref.splitmix_perms)."""
    p, nperms, seed = 257, 129, 31
    y, G, K, Cov, _ = data(n, p, 7400 + n, ncov)
    g64 = blmm.scan(y, G, K, Cov, permutation_test=True, nperms=nperms, rndseed=seed)
    g32 = blmm.scan(y, G, K, Cov, permutation_test=True, nperms=nperms, rndseed=seed, perm_precision="f32")
    assert g32["h2_null"] == g64["h2_null"]
    pidx = F.splitmix_perms(n, nperms, seed)
    Ut, lam = F.device_rotation(blmm, K)
    ref = oracle(y, G, K, Cov, None, Ut, lam, g64["h2_null"], pidx)
    assert_lod_close(g64["L_perms"], ref["L_perms"], what="fp64 L_perms on the replayed permutations")
    op = F.Operands(y, G, Ut, lam, g64["h2_null"], pidx, Covar=Cov)
    own = ncov == 0
    b = op.bound(own) + RTOL * np.abs(g64["L_perms"])
    err = np.abs(g32["L_perms"].astype(np.float64) - g64["L_perms"])
    ratio = err / b
    print(f"library RNG n {n} c {ncov + 1}: worst error / bound {ratio.max():.3g} at {F.locate(ratio, op)}")
    assert np.all(err <= b)


def test_workspace_reuse_is_bit_identical(blmm):
    """One context, calls of descending and then ascending (n, p, nperms) -- both routes -- each bit-identical to a fresh context."""
    shapes = [(1024, 257, 1025, 0), (257, 129, 129, 2), (79, 2, 2, 0)]
    fresh = {}
    for s in shapes:
        ctx = blmm.Context(0)
        fresh[s] = run(blmm, *s[:3], seed=7500 + s[0], ncov=s[3], ctx=ctx)
        ctx.close()
    shared = blmm.Context(0)
    try:
        for s in shapes + shapes[::-1]:
            y, G, K, Cov, w = data(s[0], s[1], 7500 + s[0], s[3])
            pidx = O.make_perm_idx(s[0], s[2], 7500 + s[0] + 1)
            got = blmm.scan(y, G, K, Cov, permutation_test=True, nperms=s[2], perm_idx=pidx, perm_precision="f32", ctx=shared)
            for key in ("L_perms", "lod"):
                assert np.array_equal(got[key], fresh[s][key]), (s, key)
            assert got["h2_null"] == fresh[s]["h2_null"]
    finally:
        shared.close()


def test_dev_form_leaves_the_tail_and_last_refuses(blmm):
    """blmm_scan_perms_f32_dev writes p x nperms floats and nothing beyond (a sentinel tail), equal to the host form; the blmm_last_*
    consumers refuse the fp32 matrix a host-form call leaves resident, with their documented message."""
    n, p, nperms = 79, 257, 129
    y, G, K, _, _ = data(n, p, 7600)
    pidx = O.make_perm_idx(n, nperms, 7601)
    ctx = blmm.Context(0)
    try:
        host = blmm.scan(y, G, K, permutation_test=True, nperms=nperms, perm_idx=pidx, perm_precision="f32", ctx=ctx)
        o = blmm.api._opts(blmm._lib.BLMM_NULL_EXACT, False, True, "eigen", 1, 0.0, 0.0)
        col = lambda a: np.asfortranarray(np.asarray(a, dtype=np.float64)).ravel("F")
        dY, dG, dK = DevBuf(col(y)), DevBuf(col(G)), DevBuf(col(K))
        dP = DevBuf(np.asfortranarray(pidx).ravel("F").astype(np.int32))
        dsc, dlod = DevBuf(nbytes=16), DevBuf(nbytes=8 * p)
        tail = 4096
        sentinel = np.full(p * nperms + tail, -12345.5, dtype=np.float32)
        dLp = DevBuf(sentinel)
        vp = lambda b: C.c_void_p(b.ptr)
        ctx.check(ctx.lib.blmm_scan_perms_f32_dev(ctx.h, C.byref(o), vp(dY), n, vp(dG), p, None, 0, vp(dK), None, nperms,
                                                  C.c_uint64(0), vp(dP), vp(dsc), vp(dlod), vp(dLp), None))
        ctx.synchronize()
        out = dLp.get(p * nperms + tail, np.float32)
        assert np.array_equal(out[p * nperms:], sentinel[p * nperms:])
        assert np.array_equal(out[:p * nperms].reshape(nperms, p).T, host["L_perms"])
        assert np.array_equal(dlod.get(p), host["lod"])
        for b in (dY, dG, dK, dP, dsc, dlod, dLp):
            b.free()
        blmm.scan(y, G, K, permutation_test=True, nperms=nperms, perm_idx=pidx, perm_precision="f32", ctx=ctx)
        pp, mm = C.c_int64(0), C.c_int64(0)
        assert ctx.lib.blmm_last_dims(ctx.h, C.byref(pp), C.byref(mm)) == 0 and (pp.value, mm.value) == (p, nperms)
        buf = np.empty(p * nperms)
        ii = np.empty(16, np.int32)
        idx = np.zeros(1, np.int64)
        cnt = C.c_int64(0)
        probs = np.array([0.9])
        calls = {
            "last_log10p": lambda: ctx.lib.blmm_last_log10p(ctx.h, 1, buf.ctypes.data_as(C.c_void_p)),
            "last_lod_threshold": lambda: ctx.lib.blmm_last_lod_threshold(ctx.h, 1.0, 16, ii.ctypes.data_as(C.c_void_p),
                                                                          ii.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p),
                                                                          C.byref(cnt)),
            "last_get_thresholds": lambda: ctx.lib.blmm_last_get_thresholds(ctx.h, probs.ctypes.data_as(C.c_void_p), 1,
                                                                            buf.ctypes.data_as(C.c_void_p)),
            "last_lod_colmax": lambda: ctx.lib.blmm_last_lod_colmax(ctx.h, buf.ctypes.data_as(C.c_void_p), None),
            "last_lod_columns": lambda: ctx.lib.blmm_last_lod_columns(ctx.h, idx.ctypes.data_as(C.c_void_p), 1,
                                                                      buf.ctypes.data_as(C.c_void_p)),
        }
        for name, call in calls.items():
            assert call() == INVALID, name
            assert ctx.lib.blmm_last_error(ctx.h).decode() == \
                f"{name}: no fp64 LOD matrix of a previous host-pointer call is resident"
    finally:
        ctx.close()
