"""blmm_bulkscan_reduced_async: the stream-ordered reduced bulkscan.  It only enqueues (no host round trip, no wait on an upload),
and the traits a guard flags -- the weight-basis residual (k_scan_fix) and the conditioning guard (k_scan_qr) -- are re-scanned on
the device into the reduction instead of a second run through a resident matrix.  Every result must equal the reductions of
the matrix blmm_bulkscan_dev stores under the same tuning, bit for bit: maxima, arg-maxima, the exact triplet count and the
stored triplets.  Driven through the C ABI with tests/common.py:DevBuf (torch: tests/helpers/reduced_async_check.py)."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from common import DevBuf, make_data

pytestmark = pytest.mark.gpu

RINFO_LEN = 9
ROUTE, LOWRANK, ILLCOND, TRIPLETS = 0, 1, 2, 7


def colmax_ref(L):
    Lm = np.where(np.isnan(L), -np.inf, L)
    arg = np.argmax(Lm, axis=0)
    return Lm[arg, np.arange(L.shape[1])], arg


def triplets_ref(L, thr):
    i, j = np.nonzero(L > thr)
    order = np.lexsort((i, j))
    return i[order].astype(np.int32), j[order].astype(np.int32), L[i[order], j[order]]


def _col(a):
    return DevBuf(np.asfortranarray(a).ravel("F"))


class Problem:
    """Device copies of one problem and the pieces every entry point takes."""

    def __init__(self, blmm, Y, G, K, Cov=None, method="null-exact", grid=None):
        L_ = blmm._lib
        self.blmm = blmm
        self.n, self.m = Y.shape
        self.p = G.shape[1]
        self.dY, self.dG, self.dK = _col(Y), _col(G), _col(K)
        self.dC = _col(Cov) if Cov is not None else None
        self.ncov = 0 if Cov is None else Cov.shape[1]
        self.meth = {"null-exact": L_.BLMM_NULL_EXACT, "null-grid": L_.BLMM_NULL_GRID, "alt-grid": L_.BLMM_ALT_GRID}[method]
        self.alt = method == "alt-grid"
        self.o = blmm.api._opts(self.meth)
        self.grid = None if method == "null-exact" else np.ascontiguousarray(grid if grid is not None else np.arange(10) / 10.0)
        self.bufs = [self.dY, self.dG, self.dK] + ([self.dC] if self.dC else [])

    def args(self):
        gp = None if self.grid is None else self.grid.ctypes.data
        return (self.dY.ptr, self.n, self.m, self.dG.ptr, self.p, self.dC.ptr if self.dC else None, self.ncov, self.dK.ptr, None,
                gp, 0 if self.grid is None else self.grid.size)

    def stored(self, ctx):
        """blmm_bulkscan_dev's matrix (p x m) and h2, synchronised."""
        p, m = self.p, self.m
        dL = DevBuf(nbytes=8 * max(p * m, 1))
        dh = DevBuf(nbytes=8 * max(p * m if self.alt else m, 1))
        ctx.check(ctx.lib.blmm_bulkscan_dev(ctx.h, C.byref(self.o), *self.args(), dL.ptr, max(p, 1), dh.ptr, None))
        ctx.synchronize()
        L = dL.get((m, p)).T if p * m else np.zeros((p, m))
        h2 = dh.get(m) if m and not self.alt else None
        dL.free(); dh.free()
        return L, h2

    def outputs(self, cap):
        m = max(self.m, 1)
        return {"mx": DevBuf(nbytes=8 * m), "ax": DevBuf(nbytes=8 * m), "h2": DevBuf(nbytes=8 * m),
                "ti": DevBuf(nbytes=4 * max(cap, 1)), "tj": DevBuf(nbytes=4 * max(cap, 1)), "tl": DevBuf(nbytes=8 * max(cap, 1)),
                "cnt": DevBuf(np.full(1, -5, dtype=np.int64)), "info": DevBuf(np.full(RINFO_LEN, -9, dtype=np.int64)), "cap": cap}

    def reduced(self, ob, thr):
        L_ = self.blmm._lib
        want = thr is not None
        return L_.blmm_reduced(ob["mx"].ptr, ob["ax"].ptr, 1 if want else 0, float(thr) if want else 0.0, ob["cap"] if want else 0,
                               ob["ti"].ptr, ob["tj"].ptr, ob["tl"].ptr, ob["cnt"].ptr)

    def enqueue_async(self, ctx, ob, thr, keep):
        r = self.reduced(ob, thr)
        keep.append(r)
        return ctx.lib.blmm_bulkscan_reduced_async(ctx.h, C.byref(self.o), *self.args(), C.byref(r), ob["h2"].ptr, ob["info"].ptr)

    def run_sync(self, ctx, ob, thr):
        r = self.reduced(ob, thr)
        ctx.check(ctx.lib.blmm_bulkscan_reduced_dev(ctx.h, C.byref(self.o), *self.args(), C.byref(r), ob["h2"].ptr, None))

    def read(self, ob, thr):
        m = self.m
        out = {"mx": ob["mx"].get(m), "ax": ob["ax"].get(m, np.int64), "h2": ob["h2"].get(m), "info": ob["info"].get(RINFO_LEN, np.int64)}
        if thr is not None:
            k = int(ob["cnt"].get(1, np.int64)[0])
            s = min(k, ob["cap"])
            gi, gj, gl = ob["ti"].get(ob["cap"], np.int32)[:s], ob["tj"].get(ob["cap"], np.int32)[:s], ob["tl"].get(ob["cap"])[:s]
            order = np.lexsort((gi, gj))
            out.update(count=k, ti=gi[order], tj=gj[order], tl=gl[order])
        return out

    def free(self):
        for b in self.bufs:
            b.free()

    @staticmethod
    def release(ob):
        for v in ob.values():
            if isinstance(v, DevBuf):
                v.free()


def run_async(ctx, pr, thr, cap=1 << 16):
    ob = pr.outputs(cap)
    keep = []
    ctx.check(pr.enqueue_async(ctx, ob, thr, keep))
    ctx.synchronize()
    res = pr.read(ob, thr)
    pr.release(ob)
    return res


def assert_equal_to_stored(res, L, h2, thr, alt=False):
    mx, arg = colmax_ref(L)
    assert np.array_equal(res["mx"], mx) and np.array_equal(res["ax"], arg)
    ti, tj, tl = triplets_ref(L, thr)
    assert res["count"] == ti.size == res["info"][TRIPLETS]
    assert np.array_equal(res["ti"], ti) and np.array_equal(res["tj"], tj) and np.array_equal(res["tl"], tl)
    if not alt:
        assert np.array_equal(res["h2"], h2)


@pytest.mark.parametrize("method,ncov,m,route", [("null-exact", 0, 700, 1), ("null-exact", 2, 300, 1), ("null-grid", 1, 500, 1),
                                                  ("alt-grid", 0, 130, 2), ("null-exact", 5, 90, 2)])
def test_async_equals_the_reductions_of_the_stored_matrix(blmm, method, ncov, m, route):
    Y, G, K, Cov = make_data(p=1013, m=m, seed=3300 + ncov + m, ncov=ncov)   # (the seeds of test_gpu_reduced.py: its routes are known)
    G = G.copy(); G[:, 700] = G[:, 3]                       # a duplicated marker: the arg-max tie rule matters
    ctx = blmm.Context(0)
    pr = Problem(blmm, Y, G, K, Cov, method)
    L, h2 = pr.stored(ctx)
    thr = float(np.quantile(L, 0.999))
    res = run_async(ctx, pr, thr)
    assert res["info"][ROUTE] == route
    assert_equal_to_stored(res, L, h2, thr, alt=pr.alt)
    if route == 1:
        last_p, last_m = C.c_int64(-1), C.c_int64(-1)
        ctx.lib.blmm_last_dims(ctx.h, C.byref(last_p), C.byref(last_m))
        assert last_m.value <= 0                            # routes 1 / 3 leave no resident matrix behind
    pr.free()
    ctx.close()


def _status_count(ctx, pr, field):
    st = pr.blmm._lib.blmm_status()
    dL, dh = DevBuf(nbytes=8 * pr.p * pr.m), DevBuf(nbytes=8 * pr.m)
    ctx.check(ctx.lib.blmm_bulkscan_dev(ctx.h, C.byref(pr.o), *pr.args(), dL.ptr, pr.p, dh.ptr, C.byref(st)))
    dL.free(); dh.free()
    return getattr(st, field)


@pytest.mark.parametrize("ncov,key,value,field", [(0, "lr_tol", 0.0, LOWRANK), (2, "illcond_rho", 2.0, ILLCOND)])
def test_every_trait_flagged_is_rescanned_on_the_device(blmm, ncov, key, value, field):
    Y, G, K, Cov = make_data(p=500, m=200, seed=5201 + ncov, ncov=ncov)
    ctx = blmm.Context(0)
    ctx.set_tuning(key, value)
    if ncov:
        ctx.set_tuning("lr_tol", 0.0)                       # both guards: k_scan_fix, then k_scan_qr over the same traits
    pr = Problem(blmm, Y, G, K, Cov)
    L, h2 = pr.stored(ctx)
    thr = float(np.quantile(L, 0.99))
    res = run_async(ctx, pr, thr)
    assert res["info"][ROUTE] == 3 and res["info"][field] == 200
    if ncov:
        assert res["info"][LOWRANK] == 200
    assert_equal_to_stored(res, L, h2, thr)
    pr.free()
    ctx.close()


@pytest.mark.parametrize("ncov", [0, 2])
def test_some_traits_flagged_count_stays_exact_also_beyond_cap(blmm, ncov):
    """Only a fraction of the traits flagged: flagged and unflagged traits both contribute triplets.  Then the same with `cap`
    below the count: the count stays exact, every stored triplet is genuine and none is stored twice."""
    Y, G, K, Cov = make_data(p=600, m=300, seed=5300 + ncov, ncov=ncov)
    ctx = blmm.Context(0)
    pr = Problem(blmm, Y, G, K, Cov)
    if ncov == 0:
        key, cands, field = "lr_tol", [10.0 ** (-e / 4) for e in range(52, 68)], "lowrank_fallback"
    else:
        key, cands, field = "illcond_rho", list(np.linspace(0.3, 1.0, 36)), "n_illcond_rescan"
    chosen = None
    for v in cands:
        ctx.set_tuning(key, float(v))
        k = _status_count(ctx, pr, field)
        if 0 < k < pr.m:
            chosen = (float(v), k)
            break
    assert chosen is not None, f"no {key} flags only a fraction of the traits"
    L, h2 = pr.stored(ctx)
    thr = float(np.quantile(L, 0.9))
    res = run_async(ctx, pr, thr)
    assert res["info"][ROUTE] == 3 and res["info"][LOWRANK if ncov == 0 else ILLCOND] == chosen[1]
    assert np.unique(res["tj"]).size > 0.9 * pr.m           # nearly every trait has triplets: flagged and unflagged ones
    assert_equal_to_stored(res, L, h2, thr)
    cap = res["count"] // 3
    small = run_async(ctx, pr, thr, cap=cap)
    assert small["count"] == res["count"] and small["ti"].size == cap
    pairs = set(zip(small["ti"].tolist(), small["tj"].tolist()))
    assert len(pairs) == cap
    assert np.array_equal(small["tl"], L[small["ti"], small["tj"]]) and np.all(small["tl"] > thr)
    pr.free()
    ctx.close()


def _hip():
    h = C.CDLL("libamdhip64.so")
    h.hipStreamQuery.argtypes = [C.c_void_p]
    h.hipStreamSynchronize.argtypes = [C.c_void_p]
    h.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    h.hipStreamDestroy.argtypes = [C.c_void_p]
    h.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
    h.hipHostFree.argtypes = [C.c_void_p]
    h.hipHostGetDevicePointer.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint]
    h.hipStreamWaitValue32.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint, C.c_uint32]
    h.hipDeviceGetAttribute.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int]
    h.hipLaunchHostFunc.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    return h


HOSTFN = C.CFUNCTYPE(None, C.c_void_p)


class Gate:
    """Holds a stream at a point of its queue until open(): hipStreamWaitValue32 on a pinned host word where the device supports
    it, else a host callback waiting on an Event.  A watchdog opens it after 30 s whatever happens."""

    def __init__(self, hip, stream):
        self.hip, self.stream = hip, stream
        can = C.c_int(0)
        hip.hipDeviceGetAttribute(C.byref(can), 10013, 0)      # hipDeviceAttributeCanUseStreamWaitValue
        self.wait_value = can.value == 1
        self.ev = threading.Event()
        if self.wait_value:
            self.word = C.c_void_p()
            assert hip.hipHostMalloc(C.byref(self.word), 64, 2) == 0   # hipHostMallocMapped
            C.memset(self.word, 0, 64)
            dptr = C.c_void_p()
            assert hip.hipHostGetDevicePointer(C.byref(dptr), self.word, 0) == 0
            assert hip.hipStreamWaitValue32(stream, dptr, 1, 0, 0xFFFFFFFF) == 0   # hipStreamWaitValueGte
        else:
            self.cb = HOSTFN(lambda _: self.ev.wait(30.0))
            assert hip.hipLaunchHostFunc(stream, C.cast(self.cb, C.c_void_p), None) == 0
        self.dog = threading.Timer(30.0, self.open)
        self.dog.start()

    def open(self):
        if self.wait_value:
            C.c_uint32.from_address(self.word.value).value = 1
        self.ev.set()

    def close(self):
        self.open()
        self.dog.cancel()
        self.hip.hipStreamSynchronize(self.stream)
        if self.wait_value:
            self.hip.hipHostFree(self.word)


@pytest.mark.parametrize("method", ["null-exact", "null-grid"])
def test_the_call_does_not_block_the_host(blmm, method):
    hip = _hip()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    ctx = blmm.Context(0, stream.value)
    Y, G, K, _ = make_data(p=900, m=400, seed=5400)
    pr = Problem(blmm, Y, G, K, None, method)
    L, h2 = pr.stored(ctx)
    thr = float(np.quantile(L, 0.999))
    warm = run_async(ctx, pr, thr)                           # the same shapes first: no workspace grows in the gated call
    ob = pr.outputs(1 << 14)
    keep = []
    gate = Gate(hip, stream)
    try:
        rc = pr.enqueue_async(ctx, ob, thr, keep)
        still_closed = not gate.ev.is_set() and (not gate.wait_value or C.c_uint32.from_address(gate.word.value).value == 0)
        pending = hip.hipStreamQuery(stream)
    finally:
        gate.close()
    ctx.check(rc)
    assert still_closed, "the call returned only after the gate was opened"
    assert pending == 600                                    # hipErrorNotReady: its work was still queued behind the gate
    ctx.synchronize()
    res = pr.read(ob, thr)
    assert res["info"][ROUTE] == 1
    assert_equal_to_stored(res, L, h2, thr)
    assert np.array_equal(res["mx"], warm["mx"]) and res["count"] == warm["count"]
    pr.release(ob)
    pr.free()
    ctx.close()
    hip.hipStreamDestroy(stream)


def test_back_to_back_calls_without_a_sync_in_between(blmm):
    """Four calls on one shape that forks both side streams (n <= 160, low-rank null-exact), different traits, separate outputs,
    one synchronisation at the end: each equals its own synchronous blmm_bulkscan_reduced_dev."""
    ctx = blmm.Context(0)
    probs, obs, keep = [], [], []
    _, G, K, _ = make_data(p=1100, m=900, seed=5500)
    for s in range(4):
        Y, _, _, _ = make_data(p=1100, m=900, seed=5501 + s)
        probs.append(Problem(blmm, Y, G, K))
    thr = 4.0
    run_async(ctx, probs[0], thr)                            # warm-up
    for pr in probs:
        ob = pr.outputs(1 << 15)
        obs.append(ob)
        ctx.check(pr.enqueue_async(ctx, ob, thr, keep))
    ctx.synchronize()
    got = [pr.read(ob, thr) for pr, ob in zip(probs, obs)]
    for pr, g in zip(probs, got):
        ob = pr.outputs(1 << 15)
        pr.run_sync(ctx, ob, thr)
        ref = pr.read(ob, thr)
        assert np.array_equal(g["mx"], ref["mx"]) and np.array_equal(g["ax"], ref["ax"]) and np.array_equal(g["h2"], ref["h2"])
        assert g["count"] == ref["count"] and np.array_equal(g["ti"], ref["ti"]) and np.array_equal(g["tj"], ref["tj"])
        assert np.array_equal(g["tl"], ref["tl"])
        pr.release(ob)
    assert not all(np.array_equal(got[0]["mx"], g["mx"]) for g in got[1:])   # the four calls did see different traits
    for pr, ob in zip(probs, obs):
        pr.release(ob)
        pr.free()
    ctx.close()


def test_log10p_request_is_refused_and_consumed_and_empty_shapes(blmm):
    Y, G, K, _ = make_data(p=300, m=120, seed=5600)
    ctx = blmm.Context(0)
    pr = Problem(blmm, Y, G, K)
    L, h2 = pr.stored(ctx)
    dP = DevBuf(np.full(300 * 120, -7.0))
    assert ctx.lib.blmm_set_log10p_output(ctx.h, dP.ptr, 300, 1) == 0
    ob = pr.outputs(4096)
    keep = []
    assert pr.enqueue_async(ctx, ob, 3.0, keep) == -1       # BLMM_ERR_INVALID
    assert b"log10p" in ctx.lib.blmm_last_error(ctx.h)
    res = run_async(ctx, pr, 3.0)                            # the request is gone: an ordinary call
    assert_equal_to_stored(res, L, h2, 3.0)
    ctx.synchronize()
    assert np.all(dP.get(300 * 120) == -7.0)
    # no markers / no traits: as the synchronous form (-inf, -1, zero triplets)
    for Ys, Gs in ((Y, G[:, :0]), (Y[:, :0], G)):
        for meth in ("null-exact", "null-grid"):
            e = Problem(blmm, Ys, Gs, K, None, meth)
            a = run_async(ctx, e, 1.0)
            ob2 = e.outputs(16)
            e.run_sync(ctx, ob2, 1.0)
            s = e.read(ob2, 1.0)
            assert a["count"] == s["count"] == 0 and a["info"][TRIPLETS] == 0 and a["info"][ROUTE] == 2
            assert np.array_equal(a["mx"], s["mx"]) and np.array_equal(a["ax"], s["ax"]) and np.array_equal(a["h2"], s["h2"])
            if e.m:
                assert np.all(np.isneginf(a["mx"])) and np.all(a["ax"] == -1)
            e.release(ob2)
            e.free()
    pr.release(ob)
    pr.free()
    dP.free()
    ctx.close()


def test_torch_binding_in_its_own_process():
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "helpers", "reduced_async_check.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "reduced_async ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
