"""The contract of every host-pointer entry point that has a device-pointer twin: the host form uploads its inputs, runs the
twin and downloads the result, so it returns what the twin returns -- bit for bit, NaN positions included.  One small seeded
shape per entry point; a dropped upload or a wrong buffer offset in the host layer (host_path.hip: HostCall) fails here.

The twins run in-process on buffers of the HIP runtime (common.DevBuf), on the context's own stream: the test synchronises the
context before it reads them back."""
import ctypes as C

import numpy as np
import pytest

from common import DevBuf, make_data

pytestmark = pytest.mark.gpu

GRID = [i / 10.0 for i in range(10)]


def col(a):
    """A host matrix as the column-major bytes the C ABI reads."""
    return np.asfortranarray(np.asarray(a, dtype=np.float64)).ravel("F")


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def opts(blmm, method, **kw):
    return blmm.api._opts(method, kw.get("reml", False), True, "eigen", 1, kw.get("prior_variance", 1.0), 0.0)


def inputs(Y, G, K, Cov=None, w=None):
    return (DevBuf(col(Y)), DevBuf(col(G)), DevBuf(col(K)), DevBuf(col(Cov)) if Cov is not None else None,
            DevBuf(np.asarray(w, dtype=np.float64)) if w is not None else None)


def vp(b):
    return None if b is None else C.c_void_p(b.ptr)


@pytest.mark.parametrize("method,ncov,weighted", [("null-exact", 2, True), ("null-grid", 0, False), ("alt-grid", 1, False)])
def test_bulkscan_host_equals_dev(blmm, method, ncov, weighted):
    Y, G, K, Cov = make_data(p=333, m=70, seed=8100 + ncov, ncov=ncov)
    n, m = Y.shape
    p = G.shape[1]
    w = np.linspace(0.5, 2.0, n) if weighted else None
    ctx = blmm.Context(0)
    host = blmm.bulkscan(Y, G, K, Cov, method=method, h2_grid=GRID, weights=w, ctx=ctx)
    meth = blmm.api._METHODS[method]
    o = opts(blmm, meth)
    dY, dG, dK, dC, dW = inputs(Y, G, K, Cov, w)
    alt = method == "alt-grid"
    dL, dH = DevBuf(nbytes=8 * p * m), DevBuf(nbytes=8 * (p * m if alt else m))
    grid = np.asarray(GRID) if meth != blmm._lib.BLMM_NULL_EXACT else None
    ctx.check(ctx.lib.blmm_bulkscan_dev(ctx.h, C.byref(o), vp(dY), n, m, vp(dG), p, vp(dC), ncov, vp(dK), vp(dW),
                                        None if grid is None else grid.ctypes.data_as(C.c_void_p), 0 if grid is None else len(grid),
                                        vp(dL), p, vp(dH), None))
    ctx.synchronize()
    same(host["L"], dL.get((m, p)).T)
    if alt:
        same(host["h2_panel"], dH.get((m, p)).T)
    else:
        same(host["h2_null_list"], dH.get(m))


@pytest.mark.parametrize("method", ["null-exact", "alt-grid"])
def test_bulkscan_reduced_host_equals_dev(blmm, method):
    Y, G, K, Cov = make_data(p=700, m=90, seed=8200, ncov=1)
    n, m = Y.shape
    p = G.shape[1]
    ctx = blmm.Context(0)
    thr = 2.5
    host = blmm.bulkscan_reduced(Y, G, K, Cov, method=method, h2_grid=GRID, threshold=thr, cap=1 << 16, ctx=ctx)
    route = host["route"]
    meth = blmm.api._METHODS[method]
    o = opts(blmm, meth)
    dY, dG, dK, dC, _ = inputs(Y, G, K, Cov)
    cap = 1 << 16
    dmx, dax, dh2 = DevBuf(nbytes=8 * m), DevBuf(nbytes=8 * m), DevBuf(nbytes=8 * m)
    dti, dtj, dtl, dtc = DevBuf(nbytes=4 * cap), DevBuf(nbytes=4 * cap), DevBuf(nbytes=8 * cap), DevBuf(np.zeros(1, dtype=np.int64))
    r = blmm._lib.blmm_reduced(dmx.ptr, dax.ptr, 1, thr, cap, dti.ptr, dtj.ptr, dtl.ptr, dtc.ptr)
    grid = np.asarray(GRID) if meth != blmm._lib.BLMM_NULL_EXACT else None
    ctx.check(ctx.lib.blmm_bulkscan_reduced_dev(ctx.h, C.byref(o), vp(dY), n, m, vp(dG), p, vp(dC), 1, vp(dK), None,
                                                None if grid is None else grid.ctypes.data_as(C.c_void_p),
                                                0 if grid is None else len(grid), C.byref(r), vp(dh2), None))
    ctx.synchronize()
    assert int(ctx.lib.blmm_last_reduced_route(ctx.h)) == route
    same(host["max_lod"], dmx.get(m))
    same(host["argmax"], dax.get(m, np.int64))
    if method != "alt-grid":
        same(host["h2_null_list"], dh2.get(m))
    k = int(dtc.get(1, np.int64)[0])
    assert k == len(host["triplets"][0]) > 0
    ii, jj, ll = dti.get(k, np.int32), dtj.get(k, np.int32), dtl.get(k)
    order = np.lexsort((ii, jj))
    for h, d in zip(host["triplets"], (ii[order], jj[order], ll[order])):
        same(h, d)


@pytest.mark.parametrize("f32", [False, True])
def test_scan_perms_host_equals_dev(blmm, f32):
    Y, G, K, Cov = make_data(p=257, m=1, seed=8300, ncov=1)
    n, p, nperms = Y.shape[0], G.shape[1], 40
    w = np.linspace(0.8, 1.2, n)
    ctx = blmm.Context(0)
    host = blmm.scan(Y[:, 0], G, K, Cov, weights=w, permutation_test=True, nperms=nperms, rndseed=11,
                     perm_precision="f32" if f32 else "f64", ctx=ctx)
    o = opts(blmm, blmm._lib.BLMM_NULL_EXACT, prior_variance=0.0)
    dY, dG, dK, dC, dW = inputs(Y[:, 0], G, K, Cov, w)
    dsc, dlod = DevBuf(nbytes=16), DevBuf(nbytes=8 * p)
    dLp = DevBuf(nbytes=(4 if f32 else 8) * p * nperms)
    fn = ctx.lib.blmm_scan_perms_f32_dev if f32 else ctx.lib.blmm_scan_perms_dev
    ctx.check(fn(ctx.h, C.byref(o), vp(dY), n, vp(dG), p, vp(dC), 1, vp(dK), vp(dW), nperms, C.c_uint64(11), None,
                 vp(dsc), vp(dlod), vp(dLp), None))
    ctx.synchronize()
    sc = dsc.get(2)
    assert host["sigma2_e"] == sc[0] and host["h2_null"] == sc[1]
    same(host["lod"], dlod.get(p))
    same(host["L_perms"], dLp.get((nperms, p), np.float32 if f32 else np.float64).T)


def test_scan_alt_host_equals_dev(blmm):
    Y, G, K, Cov = make_data(p=150, m=1, seed=8400, ncov=2)
    n, p = Y.shape[0], G.shape[1]
    ctx = blmm.Context(0)
    host = blmm.scan(Y[:, 0], G, K, Cov, assumption="alt", ctx=ctx)
    o = opts(blmm, blmm._lib.BLMM_NULL_EXACT, prior_variance=0.0)
    dY, dG, dK, dC, _ = inputs(Y[:, 0], G, K, Cov)
    dsc, dlod, dh2 = DevBuf(nbytes=16), DevBuf(nbytes=8 * p), DevBuf(nbytes=8 * p)
    ctx.check(ctx.lib.blmm_scan_alt_dev(ctx.h, C.byref(o), vp(dY), n, vp(dG), p, vp(dC), 2, vp(dK), None, vp(dsc), vp(dlod), vp(dh2), None))
    ctx.synchronize()
    sc = dsc.get(2)
    assert host["sigma2_e"] == sc[0] and host["h2_null"] == sc[1]
    same(host["lod"], dlod.get(p))
    same(host["h2_each_marker"], dh2.get(p))


def test_bulkscan_alt_exact_host_equals_dev(blmm):
    Y, G, K, Cov = make_data(p=130, m=9, seed=8500, ncov=1)
    n, m = Y.shape
    p = G.shape[1]
    w = np.linspace(0.7, 1.4, n)
    ctx = blmm.Context(0)
    host = blmm.bulkscan_alt_exact(Y, G, K, Cov, weights=w, ctx=ctx)
    o = opts(blmm, blmm._lib.BLMM_NULL_EXACT, prior_variance=0.0)
    dY, dG, dK, dC, dW = inputs(Y, G, K, Cov, w)
    dL, dH, dh2, ds2 = DevBuf(nbytes=8 * p * m), DevBuf(nbytes=8 * p * m), DevBuf(nbytes=8 * m), DevBuf(nbytes=8 * m)
    ctx.check(ctx.lib.blmm_bulkscan_alt_exact_dev(ctx.h, C.byref(o), vp(dY), n, m, vp(dG), p, vp(dC), 1, vp(dK), vp(dW),
                                                  vp(dL), p, vp(dH), p, vp(dh2), vp(ds2), None))
    ctx.synchronize()
    same(host["L"], dL.get((m, p)).T)
    same(host["h2_panel"], dH.get((m, p)).T)
    same(host["h2_null_list"], dh2.get(m))
    same(host["sigma2_e"], ds2.get(m))


def test_kinship_host_equals_dev(blmm):
    _, G, _, _ = make_data(n=97, p=411, m=1, seed=8600, bxd=False)
    n, p = G.shape
    ctx = blmm.Context(0)
    dG, dK = DevBuf(col(G)), DevBuf(nbytes=8 * n * n)
    ctx.check(ctx.lib.blmm_kinship_dev(ctx.h, vp(dG), n, p, vp(dK)))
    ctx.synchronize()
    Kd = dK.get((n, n)).T
    same(blmm.calcKinship(G, ctx=ctx), Kd)
    # digits: k_round_digits is rint(v * 10^d) / 10^d -- NumPy's round, on the same unrounded matrix
    same(blmm.calcKinship(G, ctx=ctx, digits=6), np.round(Kd, 6))


def test_lod_consumers_host_equal_dev(blmm):
    Y, G, K, _ = make_data(p=300, m=50, seed=8700)
    ctx = blmm.Context(0)
    Lm = np.asfortranarray(blmm.bulkscan(Y, G, K, method="null-grid", h2_grid=GRID, ctx=ctx)["L"])
    Lm[5, 3] = np.nan
    Lm[:, 7] = np.nan
    Lm[11, 9] = Lm[200, 9] = Lm[:, 9].max() + 1.0            # a tie: the lowest marker wins in both forms
    p, m = Lm.shape
    dL = DevBuf(col(Lm))

    mx, arg = blmm.lod_colmax(Lm, ctx=ctx)
    dmx, dax = DevBuf(nbytes=8 * m), DevBuf(nbytes=8 * m)
    ctx.check(ctx.lib.blmm_lod_colmax_dev(ctx.h, vp(dL), p, m, p, vp(dmx), vp(dax)))
    ctx.synchronize()
    same(mx, dmx.get(m))
    same(arg, dax.get(m, np.int64))
    lmx, larg = np.empty(m), np.empty(m, dtype=np.int64)   # the host form's upload is the context's resident matrix now
    ctx.check(ctx.lib.blmm_last_lod_colmax(ctx.h, lmx.ctypes.data_as(C.c_void_p), larg.ctypes.data_as(C.c_void_p)))
    same(mx, lmx)
    same(arg, larg)

    P = blmm.lod2log10p(Lm, 1, ctx=ctx)
    dP = DevBuf(nbytes=8 * p * m)
    ctx.check(ctx.lib.blmm_lod2log10p_dev(ctx.h, vp(dL), p, m, p, 1, vp(dP), p))
    ctx.synchronize()
    same(P, dP.get((m, p)).T)

    thr, cap = float(np.nanquantile(Lm, 0.9)), 4096
    ti, tj, tl = blmm.lod_threshold(Lm, thr, ctx=ctx, cap=cap)
    dti, dtj, dtl, dtc = DevBuf(nbytes=4 * cap), DevBuf(nbytes=4 * cap), DevBuf(nbytes=8 * cap), DevBuf(nbytes=8)
    ctx.check(ctx.lib.blmm_lod_threshold_dev(ctx.h, vp(dL), p, m, p, thr, cap, vp(dti), vp(dtj), vp(dtl), vp(dtc)))
    ctx.synchronize()
    k = int(dtc.get(1, np.int64)[0])
    assert 0 < k == len(ti) <= cap
    ii, jj, ll = dti.get(k, np.int32), dtj.get(k, np.int32), dtl.get(k)
    order = np.lexsort((ii, jj))
    for h, d in zip((ti, tj, tl), (ii[order], jj[order], ll[order])):
        same(h, d)
    li, lj, ll2 = (np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.int32), np.empty(cap))
    cnt = C.c_int64(0)
    ctx.check(ctx.lib.blmm_last_lod_threshold(ctx.h, thr, cap, li.ctypes.data_as(C.c_void_p), lj.ctypes.data_as(C.c_void_p),
                                              ll2.ctypes.data_as(C.c_void_p), C.byref(cnt)))
    assert cnt.value == k
    order = np.lexsort((li[:k], lj[:k]))
    for h, d in zip((ti, tj, tl), (li[:k][order], lj[:k][order], ll2[:k][order])):
        same(h, d)

    Lp = np.asfortranarray(Lm[:, 10:])                      # as permutation maxima: no NaN column
    dLp = DevBuf(col(Lp))
    host = blmm.get_thresholds(Lp, [0.5, 0.1, 0.05], ctx=ctx)
    got = np.empty(3)
    ctx.check(ctx.lib.blmm_get_thresholds_dev(ctx.h, vp(dLp), p, Lp.shape[1], p, host["probs"].ctypes.data_as(C.c_void_p), 3,
                                              got.ctypes.data_as(C.c_void_p)))
    same(host["thrs"], got)


# ---- refusals: one bad argument per call, the exact (code, message) of blmm_last_error ------------------------------------------
# The device forms refuse before they touch the device; the host forms marked after-uploads refuse in their device twin, behind
# the HostCall uploads of their inputs.  Every output buffer is large enough for the call to run, should a check ever go missing.
RN, RM, RP = 8, 3, 6
OUT = 1 << 16
INVALID, DIM, DECOMP, METHOD, NPERMS = -1, -2, -4, -5, -9
UNKNOWN = "Unknown method; choose null-exact, null-grid or alt-grid."
BAD_DECOMP = "Please choose either `eigen` or `svd` for decomposition of the kinship matrix."


class RefusalEnv:
    def __init__(self, blmm, ctx):
        rng = np.random.Generator(np.random.PCG64(9100))
        A = rng.standard_normal((RN, RN))
        self.blmm, self.lib, self.h = blmm, ctx.lib, ctx.h
        self.Y, self.G = rng.standard_normal(RN * RM), rng.standard_normal(RN * RP)
        self.K, self.Cov = col(A @ A.T / RN + np.eye(RN)), rng.standard_normal(RN * RN)
        self.w, self.grid = np.linspace(0.5, 2.0, RN), np.array([0.0, 0.3, 0.6])
        self.perm = np.tile(np.arange(RN, dtype=np.int32), 4)
        self.dY, self.dG, self.dK = DevBuf(self.Y), DevBuf(self.G), DevBuf(self.K)
        self.dout = [DevBuf(nbytes=OUT) for _ in range(8)]
        self.hout = [np.zeros(OUT // 8) for _ in range(8)]

    def o(self, method=1, decomp="eigen"):
        return C.byref(self.blmm.api._opts(method, decomp_scheme=decomp))

    def d(self, i):
        return self.dout[i].ptr

    def hp(self, a):
        return a.ctypes.data

    def reduced(self, host, cap=0):
        pick = self.hp if host else (lambda a: a.ptr)
        out = self.hout if host else self.dout
        return C.byref(self.blmm._lib.blmm_reduced(pick(out[0]), pick(out[1]), 0, 0.0, cap, None, None, None, pick(out[2])))

    def prepare(self):
        assert self.lib.blmm_prepare_dev(self.h, self.o(), RN, None, 0, self.dK.ptr, None, None) == 0


def _bulkscan_dev(e, method=1, decomp="eigen", dY=True, ldL=RP):
    return e.lib.blmm_bulkscan_dev(e.h, e.o(method, decomp), e.dY.ptr if dY else None, RN, RM, e.dG.ptr, RP, None, 0, e.dK.ptr, None,
                                   e.hp(e.grid), 3, e.d(0), ldL, e.d(1), None)


def _bulkscan(e, method=1, decomp="eigen", Y=True, ncov=0):
    return e.lib.blmm_bulkscan(e.h, e.o(method, decomp), e.hp(e.Y) if Y else None, RN, RM, e.hp(e.G), RP, e.hp(e.Cov) if ncov else None,
                               ncov, e.hp(e.K), e.hp(e.w), e.hp(e.grid), 3, e.hp(e.hout[0]), e.hp(e.hout[1]), None)


def _reduced_async(e, method=1, armed=False, ngrid=3):
    if armed:
        assert e.lib.blmm_set_log10p_output(e.h, None, 0, 1) == 0
    return e.lib.blmm_bulkscan_reduced_async(e.h, e.o(method), e.dY.ptr, RN, RM, e.dG.ptr, RP, None, 0, e.dK.ptr, None, e.hp(e.grid),
                                             ngrid, e.reduced(False), e.d(3), e.d(4))


def _prerotated(e, prepare=True, method=1, ldL=RP):
    if prepare:
        e.prepare()
    return e.lib.blmm_bulkscan_prerotated_dev(e.h, e.o(method), e.dY.ptr, RM, RP, e.d(5), 1, RP, RP, e.hp(e.grid), 3, e.d(0), ldL,
                                              e.d(1), None)


def _perms_prerotated(e, prepare=True, both=False):
    if prepare:
        e.prepare()
    return e.lib.blmm_scan_perms_prerotated_dev(e.h, e.o(), e.dY.ptr, RP, e.d(5), 1, RP, RP, 4, 7, None, e.d(0), e.d(1), e.d(2),
                                                e.d(3) if both else None, None)


def _loco_dev(e, chr_start=(0, 3, 6), method=1):
    cs = np.asarray(chr_start, dtype=np.int64)
    return e.lib.blmm_bulkscan_loco_dev(e.h, e.o(method), e.dY.ptr, RN, RM, e.dG.ptr, RP, e.hp(cs), len(cs) - 1, -1, None, 0, None,
                                        e.hp(e.grid), 3, None, e.d(0), RP, e.d(1), None)


def _loco(e, chr_start=(0, 3, 6), method=1):
    cs = np.asarray(chr_start, dtype=np.int64)
    return e.lib.blmm_bulkscan_loco(e.h, e.o(method), e.hp(e.Y), RN, RM, e.hp(e.G), RP, e.hp(cs), len(cs) - 1, -1, e.hp(e.Cov), 1,
                                    e.hp(e.w), e.hp(e.grid), 3, e.hp(e.hout[0]), e.hp(e.hout[1]), None)


def _kinship_loco(e, dev, chr_start):
    cs = np.asarray(chr_start, dtype=np.int64)
    f = e.lib.blmm_kinship_loco_dev if dev else e.lib.blmm_kinship_loco
    return f(e.h, e.dG.ptr if dev else e.hp(e.G), RN, RP, e.hp(cs), len(cs) - 1, -1, e.d(0) if dev else e.hp(e.hout[0]))


def _scan_perms(e, f32=False, decomp="eigen", nperms=4):
    f = e.lib.blmm_scan_perms_f32 if f32 else e.lib.blmm_scan_perms
    return f(e.h, e.o(0, decomp), e.hp(e.Y), RN, e.hp(e.G), RP, e.hp(e.Cov), 1, e.hp(e.K), e.hp(e.w), nperms, 7, e.hp(e.perm),
             e.hp(e.hout[0]), e.hp(e.hout[1]), e.hp(e.hout[2]), None)


def _scan_perms_dev(e, f32=False, nperms=4, scalars=True):
    f = e.lib.blmm_scan_perms_f32_dev if f32 else e.lib.blmm_scan_perms_dev
    return f(e.h, e.o(0), e.dY.ptr, RN, e.dG.ptr, RP, None, 0, e.dK.ptr, None, nperms, 7, None, e.d(0) if scalars else None, e.d(1),
             e.d(2), None)


def _bulk_perms(e, dev, decomp="eigen", nprobs=1, bad_perm=False):
    probs = np.full(65, 0.05)
    perm = e.perm.copy()
    if bad_perm:
        perm[5] = RN
    if dev:
        return e.lib.blmm_bulkscan_perms_dev(e.h, e.o(0, decomp), e.dY.ptr, RN, RM, e.dG.ptr, RP, None, 0, e.dK.ptr, None, 4, 7, None,
                                             e.hp(probs), nprobs, *[e.d(i) for i in range(7)], None)
    return e.lib.blmm_bulkscan_perms(e.h, e.o(0, decomp), e.hp(e.Y), RN, RM, e.hp(e.G), RP, e.hp(e.Cov), 1, e.hp(e.K), e.hp(e.w), 4, 7,
                                     e.hp(perm), e.hp(probs), nprobs, *[e.hp(e.hout[i]) for i in range(7)], None)


def _scan_alt(e, dev, decomp="eigen"):
    if dev:
        return e.lib.blmm_scan_alt_dev(e.h, e.o(0, decomp), e.dY.ptr, RN, e.dG.ptr, RP, None, 0, e.dK.ptr, None, e.d(0), e.d(1), None, None)
    return e.lib.blmm_scan_alt(e.h, e.o(0, decomp), e.hp(e.Y), RN, e.hp(e.G), RP, e.hp(e.Cov), 1, e.hp(e.K), e.hp(e.w), e.hp(e.hout[0]),
                               e.hp(e.hout[1]), e.hp(e.hout[2]), None)


def _alt_exact(e, dev, decomp="eigen", ldH=RP):
    if dev:
        return e.lib.blmm_bulkscan_alt_exact_dev(e.h, e.o(0, decomp), e.dY.ptr, RN, RM, e.dG.ptr, RP, None, 0, e.dK.ptr, None, e.d(0), RP,
                                                 e.d(1), ldH, e.d(2), e.d(3), None)
    return e.lib.blmm_bulkscan_alt_exact(e.h, e.o(0, decomp), e.hp(e.Y), RN, RM, e.hp(e.G), RP, e.hp(e.Cov), 1, e.hp(e.K), e.hp(e.w),
                                         *[e.hp(e.hout[i]) for i in range(4)], None)


def _rotate(e, decomp="eigen", ncov=1):
    return e.lib.blmm_rotate(e.h, e.o(0, decomp), e.hp(e.Y), RN, RM, e.hp(e.G), RP, e.hp(e.Cov), ncov, e.hp(e.K), *[e.hp(e.hout[i]) for i in range(3)],
                             None)


REFUSALS = {
    "bulkscan_dev-null-Y": (lambda e: _bulkscan_dev(e, dY=False), INVALID, "bulkscan: NULL buffer"),
    "bulkscan_dev-method": (lambda e: _bulkscan_dev(e, method=7), METHOD, UNKNOWN),
    "bulkscan_dev-ldL": (lambda e: _bulkscan_dev(e, ldL=RP - 1), INVALID, "bulkscan: ldL < p"),
    "bulkscan_dev-decomp": (lambda e: _bulkscan_dev(e, decomp="bad"), DECOMP, BAD_DECOMP),
    "bulkscan-null-Y": (lambda e: _bulkscan(e, Y=False), INVALID, "bulkscan: NULL buffer"),
    "bulkscan-method-after-uploads": (lambda e: _bulkscan(e, method=7), METHOD, UNKNOWN),
    "bulkscan-decomp-after-uploads": (lambda e: _bulkscan(e, decomp="bad"), DECOMP, BAD_DECOMP),
    "bulkscan-covariates-after-uploads": (lambda e: _bulkscan(e, ncov=RN), DIM, "Dimension mismatch."),
    "bulkscan_reduced-method-after-uploads": (
        lambda e: e.lib.blmm_bulkscan_reduced(e.h, e.o(7), e.hp(e.Y), RN, RM, e.hp(e.G), RP, e.hp(e.Cov), 1, e.hp(e.K), e.hp(e.w),
                                              e.hp(e.grid), 3, e.reduced(True), e.hp(e.hout[3]), None), METHOD, UNKNOWN),
    "bulkscan_reduced_dev-null-out": (
        lambda e: e.lib.blmm_bulkscan_reduced_dev(e.h, e.o(), e.dY.ptr, RN, RM, e.dG.ptr, RP, None, 0, e.dK.ptr, None, e.hp(e.grid), 3,
                                                  None, e.d(3), None), INVALID, "bulkscan_reduced: NULL buffer"),
    "bulkscan_reduced_dev-triplets": (
        lambda e: e.lib.blmm_bulkscan_reduced_dev(e.h, e.o(), e.dY.ptr, RN, RM, e.dG.ptr, RP, None, 0, e.dK.ptr, None, e.hp(e.grid), 3,
                                                  e.reduced(False, cap=8), e.d(3), None), INVALID, "bulkscan_reduced: triplet buffers"),
    "bulkscan_reduced_async-log10p": (lambda e: _reduced_async(e, armed=True), INVALID,
                                      "bulkscan_reduced_async: a blmm_set_log10p_output request is pending (the reduced call writes no matrix)"),
    "bulkscan_reduced_async-method": (lambda e: _reduced_async(e, method=7), METHOD, UNKNOWN),
    "bulkscan_reduced_async-grid": (lambda e: _reduced_async(e, ngrid=0), INVALID, "h2 grid is empty"),
    "prepare_dev-null-K": (lambda e: e.lib.blmm_prepare_dev(e.h, e.o(), RN, None, 0, None, None, None), INVALID, "prepare: NULL buffer"),
    "prerotated_dev-unprepared": (lambda e: _prerotated(e, prepare=False), INVALID,
                                  "bulkscan_prerotated: blmm_prepare_dev has not run on this context"),
    "prerotated_dev-method": (lambda e: _prerotated(e, method=7), METHOD, UNKNOWN),
    "prerotated_dev-ldL": (lambda e: _prerotated(e, ldL=RP - 1), INVALID, "bulkscan: ldL < p"),
    "scan_perms_prerotated_dev-unprepared": (lambda e: _perms_prerotated(e, prepare=False), INVALID,
                                             "scan_perms_prerotated: blmm_prepare_dev has not run on this context"),
    "scan_perms_prerotated_dev-both": (lambda e: _perms_prerotated(e, both=True), INVALID,
                                       "scan_perms_prerotated: NULL buffer (exactly one of the fp64 / fp32 permutation matrices)"),
    "bulkscan_loco_dev-empty": (lambda e: _loco_dev(e, (0, 3, 3, 6)), INVALID, "bulkscan_loco: chromosome 1 is empty"),
    "bulkscan_loco_dev-start": (lambda e: _loco_dev(e, (1, 3, 6)), INVALID, "bulkscan_loco: chromosome offsets must run from 0 to p"),
    "bulkscan_loco_dev-one": (lambda e: _loco_dev(e, (0, 6)), INVALID,
                              "bulkscan_loco: leave-one-chromosome-out needs at least 2 chromosomes"),
    "bulkscan_loco_dev-method": (lambda e: _loco_dev(e, method=7), METHOD, UNKNOWN),
    "bulkscan_loco-order": (lambda e: _loco(e, (0, 4, 2, 6)), INVALID, "bulkscan_loco: chromosome offsets are not increasing"),
    "bulkscan_loco-method-after-uploads": (lambda e: _loco(e, method=7), METHOD, UNKNOWN),
    "kinship_loco-every-marker": (lambda e: _kinship_loco(e, False, (0, 6, 6)), INVALID,
                                  "kinship_loco: a chromosome holds every marker (no kinship is left)"),
    "kinship_loco_dev-empty": (lambda e: _kinship_loco(e, True, (0, 3, 3, 6)), INVALID, "kinship_loco: chromosome 1 is empty"),
    "scan_perms-decomp-after-uploads": (lambda e: _scan_perms(e, decomp="bad"), DECOMP, BAD_DECOMP),
    "scan_perms_f32-decomp-after-uploads": (lambda e: _scan_perms(e, f32=True, decomp="bad"), DECOMP, BAD_DECOMP),
    "scan_perms_dev-null": (lambda e: _scan_perms_dev(e, scalars=False), INVALID, "scan_perms: NULL buffer"),
    "scan_perms_f32_dev-nperms": (lambda e: _scan_perms_dev(e, f32=True, nperms=-1), NPERMS,
                                  "The required number of permutations must be a positive integer."),
    "bulkscan_perms-perm_idx": (lambda e: _bulk_perms(e, False, bad_perm=True), INVALID,
                                "bulkscan_perms: perm_idx entries must lie in 0 .. n - 1"),
    "bulkscan_perms-decomp": (lambda e: _bulk_perms(e, False, decomp="bad"), DECOMP, BAD_DECOMP),
    "bulkscan_perms_dev-levels": (lambda e: _bulk_perms(e, True, nprobs=65), INVALID, "bulkscan_perms: 0 .. 64 threshold levels"),
    "scan_alt-decomp-after-uploads": (lambda e: _scan_alt(e, False, decomp="bad"), DECOMP, BAD_DECOMP),
    "scan_alt_dev-null": (lambda e: _scan_alt(e, True), INVALID, "scan_alt: NULL buffer"),
    "bulkscan_alt_exact-decomp-after-uploads": (lambda e: _alt_exact(e, False, decomp="bad"), DECOMP, BAD_DECOMP),
    "bulkscan_alt_exact_dev-ldH": (lambda e: _alt_exact(e, True, ldH=RP - 1), INVALID, "bulkscan_alt_exact: leading dimension < p"),
    "rotate-decomp": (lambda e: _rotate(e, decomp="bad"), DECOMP, BAD_DECOMP),
    "rotate-covariates-after-uploads": (lambda e: _rotate(e, ncov=RN), DIM, "Dimension mismatch."),
}
# chisq_df runs over [1, 10^6] at every -log10 p entry point (blmm_lod2log10p_dev and blmm_set_log10p_output refuse beyond): a df
# of 2^32 + 1 must not reach the kernel's int as 1, nor 2^31 as a negative df
for _df in (1000000 + 1, 1 << 31, (1 << 32) + 1):
    REFUSALS[f"lod2log10p-df-{_df}"] = (lambda e, df=_df: e.lib.blmm_lod2log10p(e.h, e.hp(e.G), RP, 1, df, e.hp(e.hout[0])), INVALID,
                                        "lod2log10p: bad arguments")
    REFUSALS[f"last_log10p-df-{_df}"] = (lambda e, df=_df: e.lib.blmm_last_log10p(e.h, df, e.hp(e.hout[0])), INVALID,
                                         "last_log10p: bad arguments")


@pytest.mark.parametrize("case", list(REFUSALS))
def test_entry_point_refusals(blmm, case):
    call, code, msg = REFUSALS[case]
    ctx = blmm.Context(0)
    e = RefusalEnv(blmm, ctx)
    rc = call(e)
    assert (rc, ctx.lib.blmm_last_error(ctx.h).decode()) == (code, msg)
    ctx.synchronize()
    ctx.close()
