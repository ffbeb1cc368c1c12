"""Host-side mirror of BulkLMM.jl's API for the bulkscan hot path, over the C ABI of libbulklmm_hip.so.

Same names, argument meaning, defaults, return field names and error strings as the reference
(src/bulkscan.jl:81-162,188-314,321-397,428-526; src/scan.jl:94-271,485-557; src/kinship.jl:4-14;
src/transform_helpers.jl:1-54; src/bulkscan_helpers.jl:175-201), so the parity tests read like the
reference's own tests.  All arithmetic happens on the GPU; there is no CPU fallback."""
from __future__ import annotations

import contextlib
import ctypes as C
import operator
import warnings
from typing import NamedTuple, Optional

import numpy as np

from . import _lib as L


class BulkLMMError(Exception):
    """Julia ErrorException stand-in; `.msg` is the reference's message, `.code` the blmm_err."""

    def __init__(self, msg: str, code: int = -1):
        super().__init__(msg)
        self.msg = msg
        self.code = code


def _stream_arg(stream: Optional[int]):
    """None -> NULL (private stream); 0 -> BLMM_STREAM_NULL (adopt the legacy default stream); else the handle."""
    if stream is None:
        return None
    if int(stream) == 0:
        return C.c_void_p(-1)  # BLMM_STREAM_NULL, include/bulklmm_hip.h
    return C.c_void_p(int(stream))


class Context:
    """One GPU.  Not thread-safe (include/bulklmm_hip.h)."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        """stream=None: a private non-blocking stream of the library (no ordering against the caller's streams);
        an integer hipStream_t handle: every *_dev call enqueues there.  The handle 0 -- torch.cuda's default stream,
        the legacy null stream -- is adopted as such (BLMM_STREAM_NULL), NOT replaced by a private stream."""
        self.lib = L.load()
        h = C.c_void_p()
        rc = self.lib.blmm_create(int(device), _stream_arg(stream), C.byref(h))
        if rc != 0:
            raise BulkLMMError(self.lib.blmm_err_string(rc).decode(), rc)
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.lib.blmm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc: int):
        if rc != 0:
            msg = self.lib.blmm_last_error(self.h).decode() or self.lib.blmm_err_string(rc).decode()
            raise BulkLMMError(msg, rc)

    def set_timing(self, on: bool):
        self.check(self.lib.blmm_set_timing(self.h, 1 if on else 0))

    def read_timings(self):
        """Sum of per-phase device times (ms) over the calls since the last read, and their count."""
        sums = (C.c_double * 6)()
        cnt = C.c_int64(0)
        self.check(self.lib.blmm_read_timings(self.h, sums, C.byref(cnt)))
        names = ("eigen", "rotate", "h2", "prep", "scan", "total")
        return {k: float(v) for k, v in zip(names, sums)}, int(cnt.value)

    def lowrank_profile(self):
        """blmm_lowrank_profile: (traits of the shared-weights class, [(traits, rank) per segment of the heritability axis]) of the
        last null-exact call -- what its low-rank weights form executed."""
        out = (C.c_int64 * 18)()
        self.check(self.lib.blmm_lowrank_profile(self.h, out))
        return int(out[1]), [(int(out[2 + 2 * s]), int(out[3 + 2 * s])) for s in range(int(out[0]))]

    def lowrank_columns(self, m: int):
        """blmm_lowrank_columns: (panel column of each of the m traits, region width, [shared, others] per region) of the last
        null-exact call's low-rank form."""
        col = np.empty(m, dtype=np.int32)
        w = C.c_int64(0)
        cnt = (C.c_int64 * 4)()
        self.check(self.lib.blmm_lowrank_columns(self.h, int(m), col.ctypes.data_as(C.c_void_p), C.byref(w), cnt))
        return col, int(w.value), [int(x) for x in cnt]

    def set_tuning(self, key: str, value: float):
        """blmm_set_tuning: the switches that select another arithmetic path (include/bulklmm_hip.h); key "defaults" resets."""
        self.check(self.lib.blmm_set_tuning(self.h, key.encode(), float(value)))

    def get_tuning(self, key: str) -> float:
        v = C.c_double(0.0)
        if self.lib.blmm_get_tuning(self.h, key.encode(), C.byref(v)) != 0:
            raise BulkLMMError("get_tuning: unknown key " + key)
        return float(v.value)

    def set_stream(self, stream: Optional[int]):
        self.check(self.lib.blmm_set_stream(self.h, _stream_arg(stream)))

    def synchronize(self):
        self.check(self.lib.blmm_synchronize(self.h))


class MultiContext:
    """Several GPUs of one node behind ONE call (blmm_create_multi): one host worker thread and one blmm_ctx per device.
    `devices=None`: every visible device; an id may be repeated (several shards on one GPU)."""

    def __init__(self, devices=None):
        self.lib = L.load()
        h = C.c_void_p()
        if devices is None:
            rc = self.lib.blmm_create_multi(None, 0, C.byref(h))
        else:
            ids = (C.c_int32 * len(devices))(*[int(d) for d in devices])
            rc = self.lib.blmm_create_multi(ids, len(devices), C.byref(h))
        if rc != 0:
            raise BulkLMMError(self.lib.blmm_err_string(rc).decode(), rc)
        self.h = h
        self.ndev = int(self.lib.blmm_multi_ndev(h))

    def close(self):
        if getattr(self, "h", None):
            self.lib.blmm_destroy_multi(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc: int):
        if rc != 0:
            msg = self.lib.blmm_multi_last_error(self.h).decode() or self.lib.blmm_err_string(rc).decode()
            raise BulkLMMError(msg, rc)

    def shard(self, m: int, rank: int):
        lo, hi = C.c_int64(0), C.c_int64(0)
        self.lib.blmm_multi_shard(int(m), int(rank), self.ndev, C.byref(lo), C.byref(hi))
        return int(lo.value), int(hi.value)

    def device_result(self, rank: int):
        """(device pointer of L, ld, col_lo, col_hi, device pointer of h2) after a gather='none' / 'allgather' call."""
        dL, dH = C.c_void_p(), C.c_void_p()
        ld, lo, hi = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self.check(self.lib.blmm_multi_device_result(self.h, int(rank), C.byref(dL), C.byref(ld), C.byref(lo), C.byref(hi), C.byref(dH)))
        return dL.value, int(ld.value), int(lo.value), int(hi.value), dH.value


    def last_colmax(self):
        """Per-trait maximum LOD and its marker (0-based) of the last bulkscan_multi call, reduced on the devices."""
        m = self._last_m
        mx = np.empty(m); arg = np.empty(m, dtype=np.int64)
        self.check(self.lib.blmm_multi_last_colmax(self.h, _p(mx), arg.ctypes.data_as(C.c_void_p)))
        return mx, arg

    def last_lod_threshold(self, thr: float, cap: int = 1 << 16):
        """(marker, trait, LOD) of every LOD > thr of the last bulkscan_multi call, sorted by (trait, marker)."""
        while True:
            ii = np.empty(cap, dtype=np.int32); jj = np.empty(cap, dtype=np.int32); ll = np.empty(cap)
            cnt = C.c_int64(0)
            self.check(self.lib.blmm_multi_last_lod_threshold(self.h, float(thr), cap, ii.ctypes.data_as(C.c_void_p),
                                                              jj.ctypes.data_as(C.c_void_p), _p(ll), C.byref(cnt)))
            if cnt.value <= cap:
                break
            cap = int(cnt.value)
        k = int(cnt.value)
        order = np.lexsort((ii[:k], jj[:k]))
        return ii[:k][order], jj[:k][order], ll[:k][order]


_GATHER = {"none": L.BLMM_GATHER_NONE, "host_shards": L.BLMM_GATHER_HOST_SHARDS, "allgather": L.BLMM_GATHER_ALLGATHER}

_default_ctx: Optional[Context] = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


MAX_INDIVIDUALS = 2048   # blmm_api.hip: prepare_eigen -- the device eigensolver (tridiagonalisation + divide and conquer) stops there


def _check_n(n: int):
    """The one documented capability gap against the reference (whose LAPACK eigen has no size limit, src/transform_helpers.jl:21-34):
    refused HERE, before anything is uploaded, with the library's own message and code."""
    if n > MAX_INDIVIDUALS:
        raise BulkLMMError("more than 2048 individuals: the device eigensolver (tridiagonalisation + divide and conquer) stops at n = 2048", -10)


def _F(a, ndim=2) -> np.ndarray:
    a = np.asarray(a, dtype=np.float64)
    if ndim == 2 and a.ndim == 1:
        a = a.reshape(-1, 1)
    return np.asfortranarray(a)


def _p(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _opts(method=L.BLMM_NULL_GRID, reml=False, addIntercept=True, decomp_scheme="eigen", optim_interval=1,
          prior_variance=1.0, prior_sample_size=0.0, compat_flags=0) -> L.blmm_opts:
    if decomp_scheme == "eigen":
        d = L.BLMM_EIGEN
    elif decomp_scheme == "svd":
        d = L.BLMM_SVD
    else:
        d = 99  # the library raises the reference's message (src/transform_helpers.jl:51)
    return L.blmm_opts(int(method), int(bool(reml)), int(bool(addIntercept)), d, int(optim_interval), int(compat_flags),
                       float(prior_variance), float(prior_sample_size))


def _raise_status(st: L.blmm_status):
    """Re-issue the reference's warnings / errors from the device counters."""
    if st.n_neg_eig:
        warnings.warn("Negative eigenvalues exist. The kinship matrix supplied may not be SPD.")  # src/transform_helpers.jl:29
    if st.n_nonpos_weight:
        warnings.warn("Some weights are not positive.")  # src/wls.jl:36
    if st.n_zero_norm:
        raise BulkLMMError(L.ERR_ZERO_NORM_MSG, -8)  # src/util.jl:70


class BulkscanNullResult(NamedTuple):
    L: np.ndarray
    h2_null_list: np.ndarray


class BulkscanAltResult(NamedTuple):
    L: np.ndarray
    h2_panel: np.ndarray


_METHODS = {"null-exact": L.BLMM_NULL_EXACT, "null-grid": L.BLMM_NULL_GRID, "alt-grid": L.BLMM_ALT_GRID}


# ---- the argument plumbing every entry point shares (each raises the reference's error, before any context exists) -----------

def _method(method: str) -> int:
    if method not in _METHODS:
        raise BulkLMMError("Unknown method `%s`; choose null-exact, null-grid or alt-grid." % method, -5)
    return _METHODS[method]


def _grid(meth: int, h2_grid):
    """(grid, ngrid) of a scan: none for null-exact; otherwise h2_grid raveled, None meaning collect(0.0:0.1:0.9)."""
    if meth == L.BLMM_NULL_EXACT:
        return None, 0
    grid = np.ascontiguousarray(np.asarray([i / 10.0 for i in range(10)] if h2_grid is None else h2_grid, dtype=np.float64).ravel())
    return grid, grid.shape[0]


def _host_arrays(Y, G, *K):
    """Y, G and K (the LOCO forms pass none) through _F, and n, m, p.  G must have n rows, K be n x n (src/transform_helpers.jl:9-11)."""
    Y = _F(Y)
    G = _F(G)
    K = _F(K[0]) if K else None
    n, m = Y.shape
    p = G.shape[1]
    if G.shape[0] != n or (K is not None and (K.shape[0] != n or K.shape[1] != n)):
        raise BulkLMMError("Dimension mismatch.", -2)
    return Y, G, K, n, m, p


def _host_covariates(Covar, weights, n: int, addIntercept: bool):
    """(cov, ncov, w, addIntercept): Covar through _F and the weights as a flat float64 array, n rows each.  Without Covar the
    intercept is the only covariate (bulkscan(Y, G, K): ones(n,1), src/bulkscan.jl:97-104)."""
    cov, ncov = None, 0
    if Covar is not None:
        cov = _F(Covar)
        if cov.shape[0] != n:
            raise BulkLMMError("Dimension mismatch.", -2)
        ncov = cov.shape[1]
    else:
        addIntercept = True
    w = None if weights is None else np.ascontiguousarray(np.asarray(weights, dtype=np.float64).ravel())
    if w is not None and w.shape[0] != n:
        raise BulkLMMError("Dimension mismatch.", -2)
    return cov, ncov, w, addIntercept


def _perm_idx(perm_idx, n: int, nperms: int):
    """perm_idx as an n x nperms column-major int32 array, or None (no permutations, or the library draws them)."""
    if perm_idx is None or nperms <= 0:
        return None
    pidx = np.asfortranarray(np.asarray(perm_idx, dtype=np.int32))
    if pidx.shape != (n, nperms):
        raise BulkLMMError("Dimension mismatch.", -2)
    return pidx


def _null_covariates(ncov: int, addIntercept: bool) -> int:
    """Columns of the null design: the covariates and the intercept, or the intercept alone."""
    return ncov + (1 if addIntercept else 0) if ncov > 0 else 1


def _probs(signif_level) -> np.ndarray:
    return np.ascontiguousarray(1.0 - np.atleast_1d(np.asarray(signif_level, dtype=np.float64)))


def _kdigits(kinship_digits: Optional[int]) -> int:
    """The LOCO kinships' rounding: -1 for none."""
    return -1 if kinship_digits is None else int(kinship_digits)


def _dptr(t):
    return None if t is None else t.data_ptr()


def _dev_args(Covar, addIntercept: bool, status: bool):
    """(ncov, addIntercept, status struct or None) of a device form; Covar is (ncov, n), and without it the intercept is the only
    covariate."""
    st = L.blmm_status() if status else None
    if Covar is None:
        return 0, True, st
    return Covar.shape[0], addIntercept, st


@contextlib.contextmanager
def _log10p_output(ctx, df, out=None, rows: int = 0):
    """`output_pvals` (src/bulkscan.jl:154-157) for the one library call in the block: asked for with df (None: not at all) into
    `out` (a tensor holding a rows x cols column-major matrix) or a buffer of the context.  Enter it after every check that can
    raise, so that no request is left armed by an exception; the library consumes it first thing in the call whatever happens next,
    and it is disarmed on the way out."""
    if df is None:
        yield
        return
    ctx.check(ctx.lib.blmm_set_log10p_output(ctx.h, _dptr(out), 0 if out is None else _ld(out, rows), int(df)))
    try:
        yield
    finally:
        ctx.lib.blmm_set_log10p_output(ctx.h, None, 0, 0)


def _reduced_host(ctx: Context, m: int, threshold, cap, call, extra: dict, h2, return_status: bool) -> dict:
    """The reduced host forms' call: call(r, st) runs the library once with byrefs of the blmm_reduced and the status; more than
    `cap` triplets and the WHOLE call runs again with the count it reported.  Returns {"max_lod", "argmax", **extra, "route"
    [, "h2_null_list": h2 unless None] [, "triplets": (i, j, lod) sorted by (trait, marker)] [, "status"]}."""
    mx = np.empty(m); arg = np.empty(m, dtype=np.int64)
    st = L.blmm_status()
    want = threshold is not None
    while True:
        cnt = C.c_int64(0)
        ii = np.empty(max(cap, 1), dtype=np.int32); jj = np.empty(max(cap, 1), dtype=np.int32); ll = np.empty(max(cap, 1))
        r = L.blmm_reduced(mx.ctypes.data, arg.ctypes.data, 1 if want else 0, float(threshold) if want else 0.0, int(cap) if want else 0,
                           ii.ctypes.data, jj.ctypes.data, ll.ctypes.data, C.addressof(cnt))
        ctx.check(call(C.byref(r), C.byref(st)))
        if not want or cnt.value <= cap:
            break
        cap = int(cnt.value)
    _raise_status(st)
    out = {"max_lod": mx, "argmax": arg, **extra, "route": int(ctx.lib.blmm_last_reduced_route(ctx.h))}
    if h2 is not None:
        out["h2_null_list"] = h2
    if want:
        k = int(cnt.value)
        order = np.lexsort((ii[:k], jj[:k]))
        out["triplets"] = (ii[:k][order], jj[:k][order], ll[:k][order])
    if return_status:
        out["status"] = st
    return out


def calcKinship(geno, ctx: Optional[Context] = None, digits: Optional[int] = None) -> np.ndarray:
    """src/kinship.jl:4-14.  `digits=12` gives `round.(calcKinship(geno), digits = 12)`, the README's convention
    (README.md:176-181), rounded on the device."""
    ctx = ctx or default_context()
    G = _F(geno)
    n, p = G.shape
    K = np.empty((n, n), dtype=np.float64, order="F")
    if digits is None:
        ctx.check(ctx.lib.blmm_kinship(ctx.h, _p(G), n, p, _p(K)))
    else:
        ctx.check(ctx.lib.blmm_kinship_rounded(ctx.h, _p(G), n, p, int(digits), _p(K)))
    return K


def _read_table(kind: str, path: str, *args) -> np.ndarray:
    lib = L.load()
    h = C.c_void_p()
    rc = lib.blmm_read_he(path.encode(), C.byref(h)) if kind == "he" else lib.blmm_read_csv(path.encode(), *args, C.byref(h))
    if rc != 0:
        raise BulkLMMError("could not read %s (%s)" % (path, lib.blmm_err_string(rc).decode()), rc)
    try:
        out = np.empty((int(lib.blmm_table_rows(h)), int(lib.blmm_table_cols(h))), order="F")
        lib.blmm_table_copy(h, _p(out))
    finally:
        lib.blmm_table_free(h)
    return out


def readGenoProb(file: str) -> np.ndarray:
    """src/readData.jl:41-70 (getmarkernames = getids = true): header line and id column dropped."""
    return _read_table("csv", file, 1, 1, 1, 0)


def readGenoProb_ExcludeComplements(file: str) -> np.ndarray:
    """src/readData.jl:85-96: the odd (1-based) probability columns of readGenoProb."""
    return _read_table("csv", file, 1, 1, 2, 0)


def readBXDpheno(file: str) -> np.ndarray:
    """src/readData.jl:159-161: readdlm(file, ','; skipstart=1)[:, 2:end-1]."""
    return _read_table("csv", file, 1, 1, 1, 1)


def readBXDgeno(file: str, skipstart: int = 1) -> np.ndarray:
    """src/readData.jl:163-165: readdlm(file, ','; skipstart)[:, 2:2:end]."""
    return _read_table("csv", file, int(skipstart), 1, 2, 0)


def readhe(file: str) -> np.ndarray:
    """Helium .he matrix (test/kinship_test.jl:5)."""
    return _read_table("he", file)


class DeviceLOD:
    """The LOD matrix of a `keep_on_device=True` call: it stays in the context's HBM workspace (blmm_bulkscan with L_out == NULL)
    and is reduced there -- what README.md:246-255, 354-359 and get_thresholds do with L -- until the context's next call that
    produces a matrix.  `shape`, `colmax()`, `threshold(t)`, `get_thresholds(probs)`, `columns(idx)`, `log10p(df)`,
    `to_host()`."""

    def __init__(self, ctx: Context, p: int, m: int):
        self.ctx, self.shape = ctx, (p, m)

    def _alive(self):
        pp, mm = C.c_int64(0), C.c_int64(0)
        if self.ctx.lib.blmm_last_dims(self.ctx.h, C.byref(pp), C.byref(mm)) != 0 or (pp.value, mm.value) != self.shape:
            raise BulkLMMError("the device-resident LOD matrix has been replaced by a later call on its context")

    def colmax(self):
        self._alive()
        m = self.shape[1]
        mx = np.empty(m); arg = np.empty(m, dtype=np.int64)
        self.ctx.check(self.ctx.lib.blmm_last_lod_colmax(self.ctx.h, _p(mx), arg.ctypes.data_as(C.c_void_p)))
        return mx, arg

    def threshold(self, thr: float, cap: int = 1 << 16):
        """(marker, trait, LOD) triplets of every LOD > thr, 0-based, sorted by (trait, marker)."""
        self._alive()
        while True:
            ii = np.empty(cap, dtype=np.int32); jj = np.empty(cap, dtype=np.int32); ll = np.empty(cap)
            cnt = C.c_int64(0)
            self.ctx.check(self.ctx.lib.blmm_last_lod_threshold(self.ctx.h, float(thr), cap, ii.ctypes.data_as(C.c_void_p),
                                                                jj.ctypes.data_as(C.c_void_p), _p(ll), C.byref(cnt)))
            if cnt.value <= cap:
                break
            cap = int(cnt.value)
        k = int(cnt.value)
        order = np.lexsort((ii[:k], jj[:k]))
        return ii[:k][order], jj[:k][order], ll[:k][order]

    def get_thresholds(self, probs):
        self._alive()
        pr = np.ascontiguousarray(np.asarray(probs, dtype=np.float64).ravel())
        out = np.empty(pr.shape[0])
        self.ctx.check(self.ctx.lib.blmm_last_get_thresholds(self.ctx.h, _p(pr), pr.shape[0], _p(out)))
        return out

    def columns(self, idx):
        """L[:, idx] (p x len(idx)) -- the LOD profiles of a few traits, the only part of L that crosses PCIe."""
        self._alive()
        ix = np.ascontiguousarray(np.asarray(idx, dtype=np.int64).ravel())
        out = np.empty((self.shape[0], ix.shape[0]), order="F")
        self.ctx.check(self.ctx.lib.blmm_last_lod_columns(self.ctx.h, ix.ctypes.data_as(C.c_void_p), ix.shape[0], _p(out)))
        return out

    def log10p(self, df: int = 1):
        self._alive()
        return _last_log10p(self.ctx, self.shape, df)

    def to_host(self):
        return self.columns(np.arange(self.shape[1]))


def _bulkscan_call(method, Y, G, K, Covar, h2_grid, addIntercept, weights, prior_variance, prior_sample_size, reml,
                   optim_interval, decomp_scheme, compat_flags, ctx, return_status=False, keep_on_device=False, pvals_df=None):
    Y, G, K, n, m, p = _host_arrays(Y, G, K)
    _check_n(n)
    cov, ncov, w, addIntercept = _host_covariates(Covar, weights, n, addIntercept)
    grid, ngrid = _grid(method, h2_grid)
    o = _opts(method, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size, compat_flags)
    ctx = ctx or default_context()  # after the argument checks: those must not need a GPU
    Lout = None if keep_on_device else np.empty((p, m), dtype=np.float64, order="F")
    h2 = np.empty((p, m) if method == L.BLMM_ALT_GRID else (m,), dtype=np.float64, order="F")
    st = L.blmm_status()
    with _log10p_output(ctx, pvals_df):
        ctx.check(ctx.lib.blmm_bulkscan(ctx.h, C.byref(o), _p(Y), n, m, _p(G), p, _p(cov), ncov, _p(K), _p(w), _p(grid), ngrid,
                                        _p(Lout), _p(h2), C.byref(st)))
    _raise_status(st)
    if keep_on_device:
        Lout = DeviceLOD(ctx, p, m)
    if return_status:
        return Lout, h2, st
    return Lout, h2


def host_register(a: np.ndarray):
    """Pin the pages of an existing array (blmm_host_register): as an output it is then filled at PCIe link rate."""
    lib = L.load()
    if lib.blmm_host_register(a.ctypes.data_as(C.c_void_p), a.nbytes) != 0:
        raise BulkLMMError("hipHostRegister failed", -12)


def host_unregister(a: np.ndarray):
    L.load().blmm_host_unregister(a.ctypes.data_as(C.c_void_p))


def bulkscan_into(ctx: Context, method: int, Y, G, K, L_out: np.ndarray, h2_out: Optional[np.ndarray] = None, *, h2_grid=None,
                  prior_variance: float = 1.0, prior_sample_size: float = 0.0, reml: bool = False, optim_interval: int = 1):
    """blmm_bulkscan (host pointers) writing into caller-provided Fortran-ordered outputs -- what a Julia caller that
    reuses its result Array does; used by bench.py for the end-to-end time."""
    Y = _F(Y); G = _F(G); K = _F(K)
    n, m = Y.shape
    p = G.shape[1]
    assert L_out.flags.f_contiguous and L_out.shape == (p, m)
    if h2_out is None:
        h2_out = np.empty((p, m) if method == L.BLMM_ALT_GRID else (m,), order="F")
    grid, ngrid = _grid(method, h2_grid)
    o = _opts(method, reml, True, "eigen", optim_interval, prior_variance, prior_sample_size)
    ctx.check(ctx.lib.blmm_bulkscan(ctx.h, C.byref(o), _p(Y), n, m, _p(G), p, None, 0, _p(K), None, _p(grid), ngrid,
                                    _p(L_out), _p(h2_out), None))
    return L_out, h2_out


def bulkscan_null(Y, G, K, Covar=None, *, nb: int = 1, nt_blas: int = 1, addIntercept: bool = True, weights=None,
                  prior_variance: float = 1.0, prior_sample_size: float = 0.0, reml: bool = False, optim_interval: int = 1,
                  decomp_scheme: str = "eigen", ctx: Optional[Context] = None, keep_on_device: bool = False,
                  _pvals_df=None) -> BulkscanNullResult:
    """src/bulkscan.jl:188-314.  `nb` / `nt_blas` are accepted and ignored (CPU thread blocking).  keep_on_device: `L` is a
    DeviceLOD (the matrix stays in HBM)."""
    Lo, h2 = _bulkscan_call(L.BLMM_NULL_EXACT, Y, G, K, Covar, None, addIntercept, weights, prior_variance, prior_sample_size,
                            reml, optim_interval, decomp_scheme, 0, ctx, keep_on_device=keep_on_device, pvals_df=_pvals_df)
    return BulkscanNullResult(Lo, h2)


def bulkscan_null_grid(Y, G, K, grid_list, Covar=None, *, weights=None, addIntercept: bool = True, prior_variance: float = 1.0,
                       prior_sample_size: float = 0.0, reml: bool = False, decomp_scheme: str = "eigen",
                       ctx: Optional[Context] = None, keep_on_device: bool = False, _pvals_df=None) -> BulkscanNullResult:
    """src/bulkscan.jl:321-385."""
    Lo, h2 = _bulkscan_call(L.BLMM_NULL_GRID, Y, G, K, Covar, grid_list, addIntercept, weights, prior_variance,
                            prior_sample_size, reml, 1, decomp_scheme, 0, ctx, keep_on_device=keep_on_device, pvals_df=_pvals_df)
    return BulkscanNullResult(Lo, h2)


def bulkscan_alt_grid(Y, G, K, hsq_list, Covar=None, *, reml: bool = False, prior_variance: float = 1.0,
                      prior_sample_size: float = 0.0, weights=None, addIntercept: bool = True, decomp_scheme: str = "eigen",
                      compat_counter_quirk: bool = False, ctx: Optional[Context] = None, keep_on_device: bool = False,
                      _pvals_df=None) -> BulkscanAltResult:
    """src/bulkscan.jl:428-526 (h2_panel = grid value at the arg-max)."""
    Lo, h2 = _bulkscan_call(L.BLMM_ALT_GRID, Y, G, K, Covar, hsq_list, addIntercept, weights, prior_variance,
                            prior_sample_size, reml, 1, decomp_scheme,
                            L.BLMM_COMPAT_ALT_COUNTER if compat_counter_quirk else 0, ctx, keep_on_device=keep_on_device,
                            pvals_df=_pvals_df)
    return BulkscanAltResult(Lo, h2)


def bulkscan_alt_exact(Y, G, K, Covar=None, *, reml: bool = False, prior_variance: float = 0.0, prior_sample_size: float = 0.0,
                       weights=None, addIntercept: bool = True, optim_interval: int = 1, decomp_scheme: str = "eigen",
                       alt_true_weights: bool = False, ctx: Optional[Context] = None) -> dict:
    """The bulk form of `scan(...; assumption = "alt")` (scan_alt, src/scan.jl:397-453; SURVEY.md N3 -- the reference itself only
    has the single-trait function and the grid approximation bulkscan_alt_grid): for every (trait, marker) the exact
    heritability under the alternative, one Brent search per test on the device.  Returns L (p x m), h2_panel (p x m),
    h2_null_list (m), sigma2_e (m); column j equals scan(Y[:, j], ...; assumption = "alt") bit for bit.  Defaults are
    scan's (prior 0 / 0), not bulkscan's."""
    Y, G, K, n, m, p = _host_arrays(Y, G, K)
    _check_n(n)
    if Covar is None and not addIntercept:
        raise BulkLMMError("Intercept has to be added when no other covariate is given.", -7)
    cov, ncov, w, addIntercept = _host_covariates(Covar, weights, n, addIntercept)
    o = _opts(L.BLMM_NULL_EXACT, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    if alt_true_weights:
        o.compat_flags |= L.BLMM_COMPAT_ALT_TRUE_WEIGHTS
    st = L.blmm_status()
    ctx = ctx or default_context()
    Lo = np.empty((p, m), order="F"); H = np.empty((p, m), order="F"); h2 = np.empty(m); s2 = np.empty(m)
    ctx.check(ctx.lib.blmm_bulkscan_alt_exact(ctx.h, C.byref(o), _p(Y), n, m, _p(G), p, _p(cov), ncov, _p(K), _p(w), _p(Lo), _p(H),
                                              _p(h2), _p(s2), C.byref(st)))
    _raise_status(st)
    return {"L": Lo, "h2_panel": H, "h2_null_list": h2, "sigma2_e": s2}


def bulkscan_multi(mctx: MultiContext, Y, G, K, Covar=None, *, method: str = "null-grid", h2_grid=None, gather: str = "host_shards",
                   addIntercept: bool = True, weights=None, prior_variance: float = 1.0, prior_sample_size: float = 0.0,
                   reml: bool = False, optim_interval: int = 1, decomp_scheme: str = "eigen", return_status: bool = False,
                   keep_on_device: bool = False) -> dict:
    """bulkscan over every GPU of `mctx` in ONE call (blmm_bulkscan_multi): the trait blocks the reference deals to its
    threads (src/bulkscan.jl:263-309) go to the devices.  Same result fields as `bulkscan`; `gather` = "host_shards"
    (default), "none" or "allgather" (include/bulklmm_hip.h)."""
    meth = _method(method)
    if gather not in _GATHER:
        raise BulkLMMError("gather must be one of none, host_shards, allgather")
    Y, G, K, n, m, p = _host_arrays(Y, G, K)
    _check_n(n)
    cov, ncov, w, addIntercept = _host_covariates(Covar, weights, n, addIntercept)
    grid, ngrid = _grid(meth, h2_grid)
    o = _opts(meth, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    mo = L.blmm_multi_opts(_GATHER[gather], 0)
    # keep_on_device: no L_out -- every device keeps its block in HBM; mctx.last_colmax() / last_lod_threshold() reduce them there
    Lout = None if keep_on_device else np.empty((p, m), dtype=np.float64, order="F")
    h2 = np.empty((p, m) if meth == L.BLMM_ALT_GRID else (m,), dtype=np.float64, order="F")
    mctx._last_m = m
    sts = (L.blmm_status * mctx.ndev)()
    mctx.check(mctx.lib.blmm_bulkscan_multi(mctx.h, C.byref(o), C.byref(mo), _p(Y), n, m, _p(G), p, _p(cov), ncov, _p(K), _p(w),
                                            _p(grid), ngrid, _p(Lout), _p(h2), sts))
    for st in sts:
        _raise_status(st)
    out = {"L": Lout, ("h2_panel" if meth == L.BLMM_ALT_GRID else "h2_null_list"): h2}
    if return_status:
        out["status"] = list(sts)
    return out


def lod2log10p(lod, df: int = 1, ctx: Optional[Context] = None):
    """lod2log10p.(lod, df), src/util.jl:199-206, on the GPU (kernels_post.hip: erfc / erfcx for df = 1, ln Q(df/2, .) in
    log space otherwise)."""
    ctx = ctx or default_context()
    a = np.asarray(lod, dtype=np.float64)
    flat = np.asfortranarray(a.reshape(-1, 1) if a.ndim != 2 else a)
    out = np.empty(flat.shape, order="F")
    ctx.check(ctx.lib.blmm_lod2log10p(ctx.h, _p(flat), flat.shape[0], flat.shape[1], int(df), _p(out)))
    return out.reshape(a.shape) if a.ndim != 2 else out


def _last_log10p(ctx: Context, shape, df: int) -> np.ndarray:
    """-log10 p of the LOD matrix the context's last host-pointer call produced (still in HBM: no re-upload)."""
    out = np.empty(shape, order="F")
    ctx.check(ctx.lib.blmm_last_log10p(ctx.h, int(df), _p(out)))
    return out


def lod_threshold(L_mat, thr: float, ctx: Optional[Context] = None, cap: Optional[int] = None):
    """Sparse triplets (marker, trait, LOD) of every LOD > thr, 0-based, sorted by (trait, marker) -- the filter behind
    plot_eQTL(...; threshold) (README.md:354-359), run on the GPU with a device-side count."""
    ctx = ctx or default_context()
    Lm = _F(L_mat)
    p, m = Lm.shape
    cap = int(cap) if cap is not None else max(1024, Lm.size // 64)
    while True:
        ii = np.empty(cap, dtype=np.int32); jj = np.empty(cap, dtype=np.int32); ll = np.empty(cap)
        cnt = C.c_int64(0)
        ctx.check(ctx.lib.blmm_lod_threshold(ctx.h, _p(Lm), p, m, float(thr), cap, ii.ctypes.data_as(C.c_void_p),
                                             jj.ctypes.data_as(C.c_void_p), _p(ll), C.byref(cnt)))
        if cnt.value <= cap:
            break
        cap = int(cnt.value)
    k = int(cnt.value)
    order = np.lexsort((ii[:k], jj[:k]))
    return ii[:k][order], jj[:k][order], ll[:k][order]


def bulkscan(Y, G, K, Covar=None, *, method: str = "null-grid", h2_grid=None, nb: int = 1, nt_blas: int = 1,
             addIntercept: bool = True, weights=None, prior_variance: float = 1.0, prior_sample_size: float = 0.0,
             reml: bool = False, optim_interval: int = 1, decomp_scheme: str = "eigen", output_pvals: bool = False,
             chisq_df: int = 1, ctx: Optional[Context] = None, keep_on_device: bool = False) -> dict:
    """src/bulkscan.jl:81-162.  Returns a dict with the reference NamedTuple's field names.  keep_on_device=True (not in the
    reference): `L` is a DeviceLOD handle -- the p x m matrix stays in HBM and is reduced there (colmax, threshold triplets,
    permutation quantiles, single columns); the call then costs ~2 ms at BXD size instead of ~39 ms, 36 of which are L's trip
    over PCIe."""
    _method(method)
    # lod2log10p.(L, chisq_df) merged into the result (src/bulkscan.jl:154-157): asked for with the scan, so that the scan
    # kernels write it from their epilogues (chisq_df = 1, null-* methods) into a buffer of the context
    pv = int(chisq_df) if output_pvals else None
    if method == "null-exact":
        r = bulkscan_null(Y, G, K, Covar, addIntercept=addIntercept, weights=weights, prior_variance=prior_variance,
                          prior_sample_size=prior_sample_size, reml=reml, optim_interval=optim_interval,
                          decomp_scheme=decomp_scheme, ctx=ctx, keep_on_device=keep_on_device, _pvals_df=pv)
        out = {"L": r.L, "h2_null_list": r.h2_null_list}
    elif method == "null-grid":
        r = bulkscan_null_grid(Y, G, K, h2_grid, Covar, weights=weights, addIntercept=addIntercept,
                               prior_variance=prior_variance, prior_sample_size=prior_sample_size, reml=reml,
                               decomp_scheme=decomp_scheme, ctx=ctx, keep_on_device=keep_on_device, _pvals_df=pv)
        out = {"L": r.L, "h2_null_list": r.h2_null_list}
    else:
        r = bulkscan_alt_grid(Y, G, K, h2_grid, Covar, reml=reml, prior_variance=prior_variance,
                              prior_sample_size=prior_sample_size, weights=weights, addIntercept=addIntercept,
                              decomp_scheme=decomp_scheme, ctx=ctx, keep_on_device=keep_on_device, _pvals_df=pv)
        out = {"L": r.L, "h2_panel": r.h2_panel}
    if output_pvals:
        out["log10Pvals_mat"] = _last_log10p(ctx or default_context(), out["L"].shape, chisq_df)
        out["Chisq_df"] = chisq_df
    return out


def bulkscan_reduced(Y, G, K, Covar=None, *, method: str = "null-grid", h2_grid=None, threshold: Optional[float] = None,
                     cap: int = 1 << 20, addIntercept: bool = True, weights=None, prior_variance: float = 1.0,
                     prior_sample_size: float = 0.0, reml: bool = False, optim_interval: int = 1, decomp_scheme: str = "eigen",
                     ctx: Optional[Context] = None, return_status: bool = False) -> dict:
    """bulkscan WITHOUT the LOD matrix (blmm_bulkscan_reduced; not in the reference, whose users reduce L on the CPU:
    README.md:246-255, 354-359): per trait the peak LOD and its marker, and -- `threshold` given -- every (marker, trait, LOD) with
    LOD > threshold, computed in the scan kernels' epilogues; L is never written.  Returns {"max_lod": m, "argmax": m (0-based),
    "h2_null_list": m [, "triplets": (i, j, lod) sorted by (trait, marker)], "route": 1 fused | 2 through a resident matrix}.
    `cap`: room for the triplets (16 bytes each, untouched pages cost nothing); more hits than that and the WHOLE call runs again
    with the count it reported -- at the BXD shape, LOD > 5 gives 1e5 triplets, hence the default of 2^20."""
    meth = _method(method)
    Y, G, K, n, m, p = _host_arrays(Y, G, K)
    _check_n(n)
    cov, ncov, w, addIntercept = _host_covariates(Covar, weights, n, addIntercept)
    grid, ngrid = _grid(meth, h2_grid)
    o = _opts(meth, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    ctx = ctx or default_context()
    h2 = np.empty(m)

    def call(r, st):
        return ctx.lib.blmm_bulkscan_reduced(ctx.h, C.byref(o), _p(Y), n, m, _p(G), p, _p(cov), ncov, _p(K), _p(w), _p(grid), ngrid,
                                             r, _p(h2), st)
    return _reduced_host(ctx, m, threshold, cap, call, {}, None if meth == L.BLMM_ALT_GRID else h2, return_status)


def scan(y, g, K, covar=None, *, weights=None, prior_variance: float = 0.0, prior_sample_size: float = 0.0,
         addIntercept: bool = True, reml: bool = False, assumption: str = "null", method: str = "qr", optim_interval: int = 1,
         permutation_test: bool = False, nperms: int = 1024, rndseed: int = 0, profileLL: bool = False, markerID: int = 0,
         h2_grid=None, decomp_scheme: str = "eigen",
         output_pvals: bool = False, chisq_df: int = 1, perm_idx=None, perm_precision: str = "f64",
         alt_true_weights: bool = False, ctx: Optional[Context] = None) -> dict:
    """src/scan.jl:94-271: the single-trait scan routed through the same GPU kernels (Brent + exact-weights LOD kernel with
    m = 1), the permutation test (src/scan.jl:485-557), and assumption == "alt" (scan_alt, src/scan.jl:397-453: one Brent
    search per marker on the device; adds `h2_each_marker`; `alt_true_weights` see BLMM_COMPAT_ALT_TRUE_WEIGHTS).
    `perm_idx` (n x nperms, 0-based) supplies the permutations; otherwise the library draws them from
    `rndseed` with its own generator (Julia's MersenneTwister stream is not reproducible).
    `perm_precision="f32"` (not in the reference; BASELINE.json configs[4]) computes L_perms on the fp32 matrix cores
    and returns it as float32; the null model and `lod` stay fp64."""
    y = _F(y)
    if covar is None and not addIntercept:
        raise BulkLMMError("Intercept has to be added when no other covariate is given.", -7)  # src/scan.jl:167-169
    if profileLL:   # src/scan.jl:252-267 (profile_LL of src/analysis_helpers): not part of the GPU path
        raise NotImplementedError("profileLL = true (profile_LL) is outside the GPU hot path; `markerID` / `h2_grid` only matter there")
    # `method` ("qr" / "cholesky") picks a CPU factorisation in the reference; the GPU path has one (closed-form WLS)
    if assumption == "alt" and permutation_test:
        raise BulkLMMError("Permutation test option currently is not supported for the alternative assumption.")
    if assumption not in ("null", "alt"):
        raise BulkLMMError("Assumption keyword is not supported. Please enter null or alt.")
    if y.shape[1] != 1:
        raise BulkLMMError("Can only handle one trait.", -6)  # src/scan.jl:496-498
    y, G, K, n, _, p = _host_arrays(y, g, K)
    _check_n(n)
    cov, ncov, w, addIntercept = _host_covariates(covar, weights, n, addIntercept)
    o = _opts(L.BLMM_NULL_EXACT, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    st = L.blmm_status()
    if not permutation_test:
        nperms = 0
    if nperms < 0:
        raise BulkLMMError("The required number of permutations must be a positive integer.", -9)
    pidx = _perm_idx(perm_idx, n, nperms)
    if perm_precision not in ("f64", "f32"):
        raise BulkLMMError("perm_precision must be \"f64\" or \"f32\".")
    ctx = ctx or default_context()
    scal = np.zeros(2)
    lod = np.empty(p)
    if assumption == "alt":
        if alt_true_weights:
            o.compat_flags |= L.BLMM_COMPAT_ALT_TRUE_WEIGHTS
        h2e = np.empty(p)
        ctx.check(ctx.lib.blmm_scan_alt(ctx.h, C.byref(o), _p(y), n, _p(G), p, _p(cov), ncov, _p(K), _p(w), _p(scal), _p(lod),
                                        _p(h2e), C.byref(st)))
        _raise_status(st)
        out = {"sigma2_e": float(scal[0]), "h2_null": float(scal[1]), "h2_each_marker": h2e, "lod": lod}
        if output_pvals:
            out["log10pvals"] = lod2log10p(lod, chisq_df, ctx=ctx)
        return out
    f32 = perm_precision == "f32"
    Lp = np.empty((p, max(nperms, 1)), order="F", dtype=np.float32 if f32 else np.float64)
    fn = ctx.lib.blmm_scan_perms_f32 if f32 else ctx.lib.blmm_scan_perms
    ctx.check(fn(ctx.h, C.byref(o), _p(y), n, _p(G), p, _p(cov), ncov, _p(K), _p(w), nperms,
                                      C.c_uint64(int(rndseed)), _p(pidx), _p(scal), _p(lod), _p(Lp), C.byref(st)))
    _raise_status(st)
    out = {"sigma2_e": float(scal[0]), "h2_null": float(scal[1]), "lod": lod}
    if permutation_test:
        out["L_perms"] = Lp[:, :nperms]
    if output_pvals:
        out["log10pvals"] = lod2log10p(lod, chisq_df, ctx=ctx)
        if permutation_test and not f32 and nperms > 0:
            out["log10Pvals_perms"] = _last_log10p(ctx, (p, nperms), chisq_df)  # the reference's UndefVarError fixed (B3)
    return out


def lod_colmax(L_mat, ctx: Optional[Context] = None):
    """Per-column maximum of an LOD matrix and the (0-based) marker where it sits, computed on the GPU."""
    ctx = ctx or default_context()
    Lm = _F(L_mat)
    p, m = Lm.shape
    mx = np.empty(m)
    arg = np.empty(m, dtype=np.int64)
    ctx.check(ctx.lib.blmm_lod_colmax(ctx.h, _p(Lm), p, m, _p(mx), arg.ctypes.data_as(C.c_void_p)))
    return mx, arg


def get_thresholds(L_perms, signif_level, ctx: Optional[Context] = None):
    """src/analysis_helpers/single_trait_analysis.jl:13-23: quantiles of the per-permutation peak LODs; column maxima,
    sort and Julia's default (linear interpolation) quantile all on the GPU (blmm_get_thresholds)."""
    ctx = ctx or default_context()
    Lm = _F(L_perms)
    p, nperms = Lm.shape
    thr_probs = _probs(signif_level)
    thrs = np.empty(thr_probs.shape[0])
    ctx.check(ctx.lib.blmm_get_thresholds(ctx.h, _p(Lm), p, nperms, _p(thr_probs), thr_probs.shape[0], _p(thrs)))
    return {"probs": thr_probs, "thrs": thrs}


def bulkscan_perms(Y, G, K, Covar=None, *, nperms: int = 1024, rndseed: int = 0, perm_idx=None, signif_level=(0.10, 0.05),
                   weights=None, prior_variance: float = 0.0, prior_sample_size: float = 0.0, addIntercept: bool = True,
                   reml: bool = False, optim_interval: int = 1, decomp_scheme: str = "eigen", ctx: Optional[Context] = None) -> dict:
    """The permutation test for every trait (blmm_bulkscan_perms): for trait j, scan(Y[:, j], G, K, Covar; permutation_test=True,
    nperms, rndseed / perm_idx) (src/scan.jl:485-557) under ONE permutation set shared by all traits -- bit for bit that call's
    L_perms reduced on the device; the p x m x nperms LOD tensor is never written.  Keyword defaults are scan's.  Returns
    {"h2_null", "sigma2_e", "lod_max", "lod_argmax" (0-based): m each; "max_perms": nperms x m (genome-wide maximum LOD of each
    permuted copy); "thresholds": len(signif_level) x m (get_thresholds(L_perms_j, signif_level)); "pvals_perm": m,
    (1 + #{k : max_perms[k, j] >= lod_max[j]}) / (nperms + 1); "probs": 1 - signif_level}.  nperms = 0: the fit and the peaks,
    thresholds and p-values NaN."""
    Y, G, K, n, m, p = _host_arrays(Y, G, K)
    _check_n(n)
    if nperms < 0:
        raise BulkLMMError("The required number of permutations must be a positive integer.", -9)
    cov, ncov, w, addIntercept = _host_covariates(Covar, weights, n, addIntercept)
    pidx = _perm_idx(perm_idx, n, nperms)
    probs = _probs(signif_level)
    ctx = ctx or default_context()
    o = _opts(L.BLMM_NULL_EXACT, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    st = L.blmm_status()
    h2, s2, mx, pv = np.empty(m), np.empty(m), np.empty(m), np.empty(m)
    arg = np.empty(m, dtype=np.int64)
    mp = np.empty((max(nperms, 1), m), order="F")
    thr = np.empty((probs.shape[0], m), order="F")
    ctx.check(ctx.lib.blmm_bulkscan_perms(ctx.h, C.byref(o), _p(Y), n, m, _p(G), p, _p(cov), ncov, _p(K), _p(w), int(nperms),
                                          C.c_uint64(int(rndseed)), _p(pidx), _p(probs), probs.shape[0], _p(h2), _p(s2), _p(mx),
                                          _p(arg), _p(mp), _p(thr), _p(pv), C.byref(st)))
    _raise_status(st)
    return {"h2_null": h2, "sigma2_e": s2, "lod_max": mx, "lod_argmax": arg, "max_perms": mp[:nperms], "thresholds": thr,
            "pvals_perm": pv, "probs": probs}


# ---- lower-level seams ------------------------------------------------------------------------------

def transform_rotation(y, g, K, *, addIntercept: bool = True, decomp_scheme: str = "eigen", ctx: Optional[Context] = None):
    """src/transform_helpers.jl:1-54: (Ut*y, Ut*[1 g], lambda).  Eigenvector signs/order within equal
    eigenvalues are arbitrary, exactly as with LAPACK."""
    y = _F(y)
    g = _F(g)
    K = _F(K)
    n, m = y.shape
    if g.shape[0] != n or K.shape[0] != n:
        raise BulkLMMError("Dimension mismatch.", -2)
    _check_n(n)
    ctx = ctx or default_context()  # after the argument checks: those must not need a GPU
    o = _opts(decomp_scheme=decomp_scheme, addIntercept=addIntercept)
    if addIntercept:
        cov, ncov, G, c = None, 0, g, 1
    else:
        # the first column of g plays the covariate role only for the layout of X0; rotation is column-wise
        cov, ncov, G, c = np.asfortranarray(g[:, :1]), 1, np.asfortranarray(g[:, 1:]), 1
        if G.shape[1] == 0:
            raise BulkLMMError("Dimension mismatch.", -2)
    p = G.shape[1]
    Y0 = np.empty((n, m), order="F")
    X0 = np.empty((n, c + p), order="F")
    lam = np.empty(n)
    st = L.blmm_status()
    ctx.check(ctx.lib.blmm_rotate(ctx.h, C.byref(o), _p(y), n, m, _p(G), p, _p(cov), ncov, _p(K), _p(Y0), _p(X0), _p(lam), C.byref(st)))
    _raise_status(st)
    return Y0, X0, lam


def fitlmm_bulk(Y0, Z0, lambda0, prior=(0.0, 0.0), *, reml: bool = False, optim_interval: int = 1, ctx: Optional[Context] = None):
    """fitlmm (src/lmm.jl:56-86) for every column of Y0: returns (h2, sigma2, ell), m each."""
    ctx = ctx or default_context()
    Y0 = _F(Y0)
    Z0 = _F(Z0)
    lam = np.ascontiguousarray(np.asarray(lambda0, dtype=np.float64))
    n, m = Y0.shape
    o = _opts(reml=reml, optim_interval=optim_interval, prior_variance=prior[0], prior_sample_size=prior[1])
    h2, s2, ell = np.empty(m), np.empty(m), np.empty(m)
    st = L.blmm_status()
    ctx.check(ctx.lib.blmm_null_h2_brent(ctx.h, C.byref(o), _p(Y0), n, m, _p(Z0), Z0.shape[1], _p(lam), _p(h2), _p(s2), _p(ell), C.byref(st)))
    return h2, s2, ell


def null_loglik_grid(Y0, Z0, lambda0, h2_grid, prior=(1.0, 0.0), *, reml: bool = False, ctx: Optional[Context] = None):
    """wls_multivar(...).Ell over a grid (src/bulkscan_helpers.jl:267-269): ngrid x m."""
    ctx = ctx or default_context()
    Y0 = _F(Y0)
    Z0 = _F(Z0)
    lam = np.ascontiguousarray(np.asarray(lambda0, dtype=np.float64))
    grid = np.ascontiguousarray(np.asarray(h2_grid, dtype=np.float64))
    n, m = Y0.shape
    o = _opts(reml=reml, prior_variance=prior[0], prior_sample_size=prior[1])
    Ell = np.empty((grid.shape[0], m), order="F")
    st = L.blmm_status()
    ctx.check(ctx.lib.blmm_null_loglik_grid(ctx.h, C.byref(o), _p(Y0), n, m, _p(Z0), Z0.shape[1], _p(lam), _p(grid), grid.shape[0], _p(Ell), C.byref(st)))
    return Ell


def weighted_liteqtl(Y0, X0, lambda0, hsq: float, *, num_of_covar: int = 1, ctx: Optional[Context] = None):
    """src/bulkscan_helpers.jl:175-201."""
    ctx = ctx or default_context()
    Y0 = _F(Y0)
    X0 = _F(X0)
    lam = np.ascontiguousarray(np.asarray(lambda0, dtype=np.float64))
    n, m = Y0.shape
    p = X0.shape[1] - num_of_covar
    out = np.empty((p, m), order="F")
    st = L.blmm_status()
    ctx.check(ctx.lib.blmm_weighted_liteqtl(ctx.h, _p(Y0), n, m, _p(X0), num_of_covar, p, _p(lam), float(hsq), _p(out), C.byref(st)))
    _raise_status(st)
    return out


def liteqtl_given_h2(Y0, X0, lambda0, h2, *, num_of_covar: int = 1, ctx: Optional[Context] = None):
    """univar_liteqtl's scan part (src/bulkscan_helpers.jl:138-146) for every column of Y0 with per-trait h2."""
    ctx = ctx or default_context()
    Y0 = _F(Y0)
    X0 = _F(X0)
    lam = np.ascontiguousarray(np.asarray(lambda0, dtype=np.float64))
    h2 = np.ascontiguousarray(np.asarray(h2, dtype=np.float64))
    n, m = Y0.shape
    p = X0.shape[1] - num_of_covar
    out = np.empty((p, m), order="F")
    st = L.blmm_status()
    ctx.check(ctx.lib.blmm_liteqtl_given_h2(ctx.h, _p(Y0), n, m, _p(X0), num_of_covar, p, _p(lam), _p(h2), _p(out), C.byref(st)))
    _raise_status(st)
    return out


# ---- device-resident entry points (torch tensors; used by bench.py and the multi-GPU path) -------------

def bulkscan_dev(ctx: Context, Y, G, K, L_out, h2_out, *, method: str = "null-exact", h2_grid=None, Covar=None, weights=None,
                 addIntercept: bool = True, prior_variance: float = 1.0, prior_sample_size: float = 0.0, reml: bool = False,
                 optim_interval: int = 1, decomp_scheme: str = "eigen", status: bool = False, log10p_out=None, chisq_df: int = 1):
    """blmm_bulkscan_dev on torch CUDA tensors laid out column-major: pass Y as a (m, n) contiguous tensor
    (= n x m column-major), G as (p, n), K as (n, n), L_out as (m, p) (= p x m column-major; rows may be padded: the
    leading dimension passed on is L_out.stride(0)).  `log10p_out` (same layout as L_out): `output_pvals` inside the scan
    (blmm_set_log10p_output).
    Enqueues on the context's stream and does not synchronise unless `status` is requested."""
    m, n = Y.shape
    p = G.shape[0]
    meth = _method(method)
    grid, ngrid = _grid(meth, h2_grid)
    ncov, addIntercept, st = _dev_args(Covar, addIntercept, status)
    o = _opts(meth, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    with _log10p_output(ctx, None if log10p_out is None else chisq_df, log10p_out, p):
        ctx.check(ctx.lib.blmm_bulkscan_dev(ctx.h, C.byref(o), Y.data_ptr(), n, m, G.data_ptr(), p, _dptr(Covar), ncov, K.data_ptr(),
                                            _dptr(weights), _p(grid), ngrid, L_out.data_ptr(), _ld(L_out, p), h2_out.data_ptr(),
                                            C.byref(st) if status else None))
    return st


def bulkscan_reduced_dev(ctx: Context, Y, G, K, max_out, argmax_out, h2_out, *, method: str = "null-exact", h2_grid=None, Covar=None,
                         weights=None, addIntercept: bool = True, prior_variance: float = 1.0, prior_sample_size: float = 0.0,
                         reml: bool = False, optim_interval: int = 1, decomp_scheme: str = "eigen", threshold: Optional[float] = None,
                         trip_i=None, trip_j=None, trip_lod=None, trip_count=None, status: bool = False):
    """blmm_bulkscan_reduced_dev on torch CUDA tensors (layouts as bulkscan_dev): max_out (m, float64), argmax_out (m, int64);
    threshold given: trip_i / trip_j (int32, cap), trip_lod (float64, cap), trip_count (int64, 1).  Synchronises the stream."""
    m, n = Y.shape
    p = G.shape[0]
    meth = _method(method)
    grid, ngrid = _grid(meth, h2_grid)
    ncov, addIntercept, st = _dev_args(Covar, addIntercept, status)
    o = _opts(meth, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    want = threshold is not None
    r = L.blmm_reduced(_dptr(max_out), _dptr(argmax_out), 1 if want else 0, float(threshold) if want else 0.0,
                       int(trip_i.numel()) if want else 0, trip_i.data_ptr() if want else None, trip_j.data_ptr() if want else None,
                       trip_lod.data_ptr() if want else None, trip_count.data_ptr() if want else None)
    ctx.check(ctx.lib.blmm_bulkscan_reduced_dev(ctx.h, C.byref(o), Y.data_ptr(), n, m, G.data_ptr(), p, _dptr(Covar), ncov, K.data_ptr(),
                                                _dptr(weights), _p(grid), ngrid, C.byref(r), _dptr(h2_out),
                                                C.byref(st) if status else None))
    return st


def bulkscan_reduced_async(ctx: Context, Y, G, K, max_out, argmax_out, h2_out, info_out, *, method: str = "null-exact", h2_grid=None,
                           Covar=None, weights=None, addIntercept: bool = True, prior_variance: float = 1.0, prior_sample_size: float = 0.0,
                           reml: bool = False, optim_interval: int = 1, decomp_scheme: str = "eigen", threshold: Optional[float] = None,
                           trip_i=None, trip_j=None, trip_lod=None, trip_count=None):
    """blmm_bulkscan_reduced_async on torch CUDA tensors (layouts as bulkscan_reduced_dev; info_out: int64, BLMM_RINFO_LEN = 9, or
    None).  Only enqueues on the context's stream and returns: the outputs are valid after ctx.synchronize() or a sync of that
    stream.  Flagged traits are re-scanned on the device (route 3) instead of a second run; reduced_info() decodes info_out."""
    m, n = Y.shape
    p = G.shape[0]
    meth = _method(method)
    grid, ngrid = _grid(meth, h2_grid)
    ncov, addIntercept, _ = _dev_args(Covar, addIntercept, False)
    if info_out is not None and info_out.numel() < L.BLMM_RINFO_LEN:
        raise BulkLMMError(f"info_out holds {info_out.numel()} entries, the info block {L.BLMM_RINFO_LEN}")
    o = _opts(meth, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    want = threshold is not None
    r = L.blmm_reduced(_dptr(max_out), _dptr(argmax_out), 1 if want else 0, float(threshold) if want else 0.0,
                       int(trip_i.numel()) if want else 0, trip_i.data_ptr() if want else None, trip_j.data_ptr() if want else None,
                       trip_lod.data_ptr() if want else None, trip_count.data_ptr() if want else None)
    ctx.check(ctx.lib.blmm_bulkscan_reduced_async(ctx.h, C.byref(o), Y.data_ptr(), n, m, G.data_ptr(), p, _dptr(Covar), ncov,
                                                  K.data_ptr(), _dptr(weights), _p(grid), ngrid, C.byref(r), _dptr(h2_out),
                                                  _dptr(info_out)))


def reduced_info(info) -> dict:
    """The info block of bulkscan_reduced_async (host copy: a numpy array or list of BLMM_RINFO_LEN int64) as a dict:
    route (1 fused, 2 resident matrix, 3 fused + on-device re-scans), lowrank_rescan, illcond_rescan, nan_lod, zero_norm, neg_eig,
    nonpos_weight, triplets (the exact count of LOD > threshold), device_error (0, or as blmm_status' failure)."""
    a = np.asarray(info, dtype=np.int64).ravel()
    if a.size < L.BLMM_RINFO_LEN:
        raise BulkLMMError(f"an info block holds {L.BLMM_RINFO_LEN} entries, got {a.size}")
    return {k: int(a[i]) for i, k in enumerate(L.RINFO_FIELDS)}


def prepare_dev(ctx: Context, K, *, Covar=None, weights=None, addIntercept: bool = True, decomp_scheme: str = "eigen", status: bool = False):
    """blmm_prepare_dev on torch CUDA tensors (K (n, n); Covar (ncov, n) = n x ncov column-major): design, eigen-decomposition and
    rotation matrix; the context then serves rotate_block_dev / bulkscan_prerotated_dev (one process per GPU: the marker
    rotation is sharded over the ranks, include/bulklmm_hip.h)."""
    n = K.shape[0]
    ncov, addIntercept, st = _dev_args(Covar, addIntercept, status)
    o = _opts(L.BLMM_NULL_EXACT, False, addIntercept, decomp_scheme)
    ctx.check(ctx.lib.blmm_prepare_dev(ctx.h, C.byref(o), n, _dptr(Covar), ncov, K.data_ptr(), _dptr(weights),
                                       C.byref(st) if status else None))
    return st


def rotated_rows(ctx: Context) -> int:
    return int(ctx.lib.blmm_rotated_rows(ctx.h))


def rotate_block_dev(ctx: Context, G_block, Xt_block):
    """blmm_rotate_block_dev: G_block (pb, n) contiguous (= n x pb column-major) -> Xt_block (rows, ld) contiguous, k-major."""
    pb = G_block.shape[0]
    ctx.check(ctx.lib.blmm_rotate_block_dev(ctx.h, G_block.data_ptr(), pb, Xt_block.data_ptr(), Xt_block.stride(0)))


def bulkscan_prerotated_dev(ctx: Context, Y, Xt_blocks, p: int, block_cols: int, L_out, h2_out, *, method: str = "null-exact", h2_grid=None,
                            prior_variance: float = 1.0, prior_sample_size: float = 0.0, reml: bool = False, optim_interval: int = 1,
                            status: bool = False):
    """blmm_bulkscan_prerotated_dev: Y (m, n); Xt_blocks (nblocks, rows, block_ld) contiguous -- the all-gathered output of
    rotate_block_dev, block b = markers [b block_cols, min(p, (b+1) block_cols)); L_out (m, p) [ld = stride(0)]."""
    m = Y.shape[0]
    meth = _method(method)
    grid, ngrid = _grid(meth, h2_grid)
    o = _opts(meth, reml, True, "eigen", optim_interval, prior_variance, prior_sample_size)
    st = L.blmm_status() if status else None
    nb, rows, bld = Xt_blocks.shape
    assert Xt_blocks.is_contiguous() and rows == rotated_rows(ctx)
    ctx.check(ctx.lib.blmm_bulkscan_prerotated_dev(ctx.h, C.byref(o), Y.data_ptr(), m, int(p), Xt_blocks.data_ptr(), nb, int(block_cols), bld,
                                                   _p(grid), ngrid, L_out.data_ptr(), _ld(L_out, int(p)), h2_out.data_ptr(),
                                                   C.byref(st) if status else None))
    return st


def _ld(t, p):
    """Leading dimension of a (cols, p) tensor that holds a p x cols column-major matrix."""
    if t.dim() != 2 or t.shape[1] != p or (p > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < p):
        raise ValueError("L_out must be a (m, p) tensor with unit stride along p")
    return t.stride(0) if t.shape[0] > 1 else max(p, t.stride(0))


def scan_perms_prerotated_dev(ctx: Context, y, Xt_blocks, p: int, block_cols: int, scalars_out, lod_out, Lperms_out, *, nperms: int,
                              seed: int = 0, perm_idx=None, prior_variance: float = 0.0, prior_sample_size: float = 0.0,
                              reml: bool = False, optim_interval: int = 1, status: bool = False):
    """blmm_scan_perms_prerotated_dev (after prepare_dev on this context): the permutation test on the gathered rotated marker
    blocks Xt_blocks (nblocks, rows, block_ld); y (n,), scalars_out (2,), lod_out (p,), Lperms_out (nperms, p) float64 or float32
    (fp32 matrix cores), perm_idx (nperms, n) int32 or None (the library's generator with `seed`)."""
    import torch
    o = _opts(L.BLMM_NULL_EXACT, reml, True, "eigen", optim_interval, prior_variance, prior_sample_size)
    st = L.blmm_status() if status else None
    nb, rows, bld = Xt_blocks.shape
    assert Xt_blocks.is_contiguous() and rows == rotated_rows(ctx)
    f32 = Lperms_out is not None and Lperms_out.dtype == torch.float32
    ctx.check(ctx.lib.blmm_scan_perms_prerotated_dev(ctx.h, C.byref(o), y.data_ptr(), int(p), Xt_blocks.data_ptr(), nb, int(block_cols), bld,
                                                     int(nperms), C.c_uint64(int(seed)), _dptr(perm_idx), scalars_out.data_ptr(),
                                                     lod_out.data_ptr(),
                                                     None if (f32 or Lperms_out is None) else Lperms_out.data_ptr(),
                                                     Lperms_out.data_ptr() if f32 else None, C.byref(st) if status else None))
    return st


def scan_perms_dev(ctx: Context, y, G, K, scalars_out, lod_out, Lperms_out, *, nperms: int, seed: int = 0, perm_idx=None,
                   Covar=None, weights=None, addIntercept: bool = True, prior_variance: float = 0.0,
                   prior_sample_size: float = 0.0, reml: bool = False, optim_interval: int = 1,
                   decomp_scheme: str = "eigen", status: bool = False):
    """blmm_scan_perms_dev on torch CUDA tensors: y (n,), G (p, n) [= n x p column-major], K (n, n),
    scalars_out (2,), lod_out (p,), Lperms_out (nperms, p) [= p x nperms column-major], perm_idx (nperms, n) int32.
    A float32 Lperms_out selects the fp32 permutation kernel (blmm_scan_perms_f32_dev)."""
    n = y.shape[0]
    p = G.shape[0]
    ncov, addIntercept, st = _dev_args(Covar, addIntercept, status)
    o = _opts(L.BLMM_NULL_EXACT, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    import torch
    f32 = Lperms_out is not None and Lperms_out.dtype == torch.float32
    fn = ctx.lib.blmm_scan_perms_f32_dev if f32 else ctx.lib.blmm_scan_perms_dev
    ctx.check(fn(ctx.h, C.byref(o), y.data_ptr(), n, G.data_ptr(), p, _dptr(Covar), ncov, K.data_ptr(), _dptr(weights), int(nperms),
                 C.c_uint64(int(seed)), _dptr(perm_idx), scalars_out.data_ptr(), lod_out.data_ptr(), _dptr(Lperms_out),
                 C.byref(st) if status else None))
    return st


def bulkscan_perms_dev(ctx: Context, Y, G, K, h2_out, sigma2_out, lod_max_out, lod_argmax_out, max_perms_out=None, thr_out=None,
                       pval_out=None, *, nperms: int, seed: int = 0, perm_idx=None, signif_level=(0.10, 0.05), Covar=None,
                       weights=None, addIntercept: bool = True, prior_variance: float = 0.0, prior_sample_size: float = 0.0,
                       reml: bool = False, optim_interval: int = 1, decomp_scheme: str = "eigen", status: bool = False):
    """blmm_bulkscan_perms_dev on torch CUDA tensors (layouts as bulkscan_dev / scan_perms_dev): Y (m, n), G (p, n), K (n, n);
    h2_out / sigma2_out / lod_max_out / pval_out (m,) float64, lod_argmax_out (m,) int64, max_perms_out (m, nperms) [= nperms x m
    column-major], thr_out (m, len(signif_level)), perm_idx (nperms, n) int32 or None (the library's generator with `seed`).
    Enqueues on the context's stream (status=True synchronises it)."""
    m, n = Y.shape
    p = G.shape[0]
    ncov, addIntercept, st = _dev_args(Covar, addIntercept, status)
    o = _opts(L.BLMM_NULL_EXACT, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    probs = _probs(signif_level)
    ctx.check(ctx.lib.blmm_bulkscan_perms_dev(ctx.h, C.byref(o), Y.data_ptr(), n, m, G.data_ptr(), p, _dptr(Covar), ncov,
                                              K.data_ptr(), _dptr(weights), int(nperms), C.c_uint64(int(seed)), _dptr(perm_idx),
                                              _p(probs), probs.shape[0], h2_out.data_ptr(), sigma2_out.data_ptr(),
                                              lod_max_out.data_ptr(), lod_argmax_out.data_ptr(), _dptr(max_perms_out), _dptr(thr_out),
                                              _dptr(pval_out), C.byref(st) if status else None))
    return st


# ---- leave-one-chromosome-out (LOCO) ---------------------------------------------------------------------------------------------
def chromosome_runs(chrom, p: int):
    """(labels in run order, chr_start int64 nchr + 1) of a length-p sequence of chromosome labels whose equal values form contiguous
    runs (the order of a genetic map).  A label that comes back after another chromosome is refused with its name."""
    labels = list(chrom.tolist() if hasattr(chrom, "tolist") else chrom)
    if len(labels) != p:
        raise BulkLMMError("Dimension mismatch.", -2)
    runs, starts, seen = [], [], set()
    for i, lab in enumerate(labels):
        if i == 0 or lab != labels[i - 1]:
            if lab in seen:
                raise BulkLMMError("chromosome %r appears again after another chromosome: the markers must be ordered by "
                                   "chromosome (contiguous runs)" % (lab,), -1)
            seen.add(lab)
            runs.append(lab)
            starts.append(i)
    starts.append(p)
    chr_start = np.asarray(starts, dtype=np.int64)
    _check_chr_start(chr_start, p)
    return runs, chr_start


def _check_chr_start(chr_start, p: int) -> np.ndarray:
    """The library's own offset checks (blmm_api.hip: loco_check), here before any context exists."""
    cs = np.ascontiguousarray(np.asarray(chr_start, dtype=np.int64).ravel())
    nchr = cs.shape[0] - 1
    if nchr < 2:
        raise BulkLMMError("leave-one-chromosome-out needs at least 2 chromosomes", -1)
    if nchr > 65535:
        raise BulkLMMError("at most 65535 chromosomes", -1)
    if cs[0] != 0 or cs[-1] != p:
        raise BulkLMMError("chromosome offsets must run from 0 to p", -1)
    d = np.diff(cs)
    if (d == 0).any():
        raise BulkLMMError("chromosome %d is empty" % int(np.flatnonzero(d == 0)[0]), -1)
    if (d < 0).any():
        raise BulkLMMError("chromosome offsets are not increasing", -1)
    if (d == p).any():
        raise BulkLMMError("a chromosome holds every marker (no kinship is left)", -1)
    return cs


def calcKinship_loco(G, chrom, digits: Optional[int] = None, ctx: Optional[Context] = None) -> np.ndarray:
    """calcKinship of every leave-one-chromosome-out genotype matrix (src/kinship.jl:4-14 on G[:, not chromosome c]), all from one
    pass over G on the device: shape (nchr, n, n), matrix c for the c-th chromosome in run order.  `digits`: rounded as calcKinship."""
    Gf = _F(G)
    n, p = Gf.shape
    _, cs = chromosome_runs(chrom, p)
    nchr = cs.shape[0] - 1
    ctx = ctx or default_context()
    out = np.empty((nchr, n, n), dtype=np.float64)     # block c = matrix c, column-major
    ctx.check(ctx.lib.blmm_kinship_loco(ctx.h, _p(Gf), n, p, _p(cs), nchr, _kdigits(digits), _p(out)))
    return out.transpose(0, 2, 1)


def bulkscan_loco(Y, G, chrom, Covar=None, *, method: str = "null-grid", h2_grid=None, kinship_digits: Optional[int] = None,
                  addIntercept: bool = True, weights=None, prior_variance: float = 1.0, prior_sample_size: float = 0.0,
                  reml: bool = False, optim_interval: int = 1, decomp_scheme: str = "eigen", output_pvals: bool = False,
                  chisq_df: int = 1, ctx: Optional[Context] = None, keep_on_device: bool = False,
                  return_status: bool = False) -> dict:
    """Leave-one-chromosome-out bulkscan (blmm_bulkscan_loco): the markers of each chromosome are scanned against the kinship of
    all the others, so that the random effect does not absorb the QTL under test (proximal contamination).  For the c-th
    chromosome in run order, L[rows_c] is bulkscan(Y, G[:, rows_c], calcKinship_loco(G, chrom, kinship_digits)[c]; same
    options)["L"] bit for bit.  `chrom`: a length-p sequence of labels in contiguous runs.  Returns {"L": p x m (or a DeviceLOD),
    "h2_null_list": nchr x m (null-* methods) or "h2_panel": p x m (alt-grid), "chromosomes": labels in run order,
    "chr_start": nchr + 1 offsets [, "log10Pvals_mat", "Chisq_df"] [, "status"]}."""
    meth = _method(method)
    Y, G, _, n, m, p = _host_arrays(Y, G)
    runs, cs = chromosome_runs(chrom, p)
    nchr = cs.shape[0] - 1
    _check_n(n)
    cov, ncov, w, addIntercept = _host_covariates(Covar, weights, n, addIntercept)
    grid, ngrid = _grid(meth, h2_grid)
    o = _opts(meth, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    ctx = ctx or default_context()  # after the argument checks: those must not need a GPU
    Lout = None if keep_on_device else np.empty((p, m), dtype=np.float64, order="F")
    h2 = np.empty((p, m), order="F") if meth == L.BLMM_ALT_GRID else np.empty((nchr, m))   # row c: chromosome c's h2 (C order)
    st = L.blmm_status()
    ctx.check(ctx.lib.blmm_bulkscan_loco(ctx.h, C.byref(o), _p(Y), n, m, _p(G), p, _p(cs), nchr, _kdigits(kinship_digits), _p(cov),
                                         ncov, _p(w), _p(grid), ngrid, _p(Lout), _p(h2), C.byref(st)))
    _raise_status(st)
    out = {"L": DeviceLOD(ctx, p, m) if keep_on_device else Lout, "chromosomes": runs, "chr_start": cs}
    out["h2_panel" if meth == L.BLMM_ALT_GRID else "h2_null_list"] = h2
    if output_pvals:
        out["log10Pvals_mat"] = _last_log10p(ctx, (p, m), chisq_df)
        out["Chisq_df"] = chisq_df
    if return_status:
        out["status"] = st
    return out


def bulkscan_loco_dev(ctx: Context, Y, G, chr_start, L_out, h2_out, *, method: str = "null-exact", h2_grid=None, K_loco=None,
                      kinship_digits: Optional[int] = None, Covar=None, weights=None, addIntercept: bool = True,
                      prior_variance: float = 1.0, prior_sample_size: float = 0.0, reml: bool = False, optim_interval: int = 1,
                      decomp_scheme: str = "eigen", status: bool = False):
    """blmm_bulkscan_loco_dev on torch CUDA tensors (layouts as bulkscan_dev: Y (m, n), G (p, n), L_out (m, p) with rows possibly
    padded); chr_start: nchr + 1 host offsets; h2_out: (nchr, m) for the null-* methods, (m, p) [= p x m] for alt-grid; K_loco:
    (nchr, n, n) as calcKinship_loco, or None (computed on the device).  Enqueues on the context's stream; status=True synchronises."""
    m, n = Y.shape
    p = G.shape[0]
    cs = _check_chr_start(chr_start, p)
    nchr = cs.shape[0] - 1
    _check_n(n)
    meth = _method(method)
    grid, ngrid = _grid(meth, h2_grid)
    ncov, addIntercept, st = _dev_args(Covar, addIntercept, status)
    o = _opts(meth, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    ctx.check(ctx.lib.blmm_bulkscan_loco_dev(ctx.h, C.byref(o), Y.data_ptr(), n, m, G.data_ptr(), p, _p(cs), nchr, _kdigits(kinship_digits),
                                             _dptr(Covar), ncov, _dptr(weights), _p(grid), ngrid, _dptr(K_loco), L_out.data_ptr(),
                                             _ld(L_out, p), _dptr(h2_out), C.byref(st) if status else None))
    return st


def bulkscan_loco_reduced(Y, G, chrom, Covar=None, *, method: str = "null-grid", h2_grid=None, threshold: Optional[float] = None,
                          cap: int = 1 << 20, kinship_digits: Optional[int] = None, addIntercept: bool = True, weights=None,
                          prior_variance: float = 1.0, prior_sample_size: float = 0.0, reml: bool = False, optim_interval: int = 1,
                          decomp_scheme: str = "eigen", ctx: Optional[Context] = None, return_status: bool = False) -> dict:
    """bulkscan_loco WITHOUT the LOD matrix (blmm_bulkscan_loco_reduced): the reductions of bulkscan_reduced over the LOCO L, plus
    every chromosome's peak, computed on the device; no p x m matrix exists there or here.  Bit for bit what lod_colmax /
    lod_threshold give on bulkscan_loco(...)["L"] with the same arguments.  Returns {"max_lod": m, "argmax": m (0-based global
    marker), "chr_max_lod": (nchr, m), "chr_argmax": (nchr, m) (row c: the peak over chromosome c's rows, still a global marker;
    -inf / -1 where every LOD is NaN), "h2_null_list": (nchr, m) (null-* methods), "chromosomes", "chr_start" [, "triplets": (i, j,
    lod) sorted by (trait, marker)], "route": 1 fused | 3 fused with on-device re-scans | 2 per-chromosome resident block
    [, "status"]}.  `cap` as bulkscan_reduced: more hits than that and the whole call runs again with the count it reported."""
    meth = _method(method)
    if int(cap) < 0:
        raise BulkLMMError("bulkscan_loco_reduced: triplet buffers (cap < 0)", -1)
    Y, G, _, n, m, p = _host_arrays(Y, G)
    runs, cs = chromosome_runs(chrom, p)
    nchr = cs.shape[0] - 1
    _check_n(n)
    cov, ncov, w, addIntercept = _host_covariates(Covar, weights, n, addIntercept)
    grid, ngrid = _grid(meth, h2_grid)
    o = _opts(meth, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    ctx = ctx or default_context()  # after the argument checks: those must not need a GPU
    cmx = np.empty((nchr, m)); carg = np.empty((nchr, m), dtype=np.int64)     # row c: chromosome c (C order = the library's blocks)
    h2 = np.empty((nchr, m))

    def call(r, st):
        return ctx.lib.blmm_bulkscan_loco_reduced(ctx.h, C.byref(o), _p(Y), n, m, _p(G), p, _p(cs), nchr, _kdigits(kinship_digits),
                                                  _p(cov), ncov, _p(w), _p(grid), ngrid, r, _p(cmx), _p(carg), _p(h2), st)
    return _reduced_host(ctx, m, threshold, int(cap), call,
                         {"chr_max_lod": cmx, "chr_argmax": carg, "chromosomes": runs, "chr_start": cs},
                         None if meth == L.BLMM_ALT_GRID else h2, return_status)


def bulkscan_loco_reduced_dev(ctx: Context, Y, G, chr_start, max_out, argmax_out, chr_max_out, chr_argmax_out, h2_out, *,
                              method: str = "null-exact", h2_grid=None, K_loco=None, kinship_digits: Optional[int] = None, Covar=None,
                              weights=None, addIntercept: bool = True, prior_variance: float = 1.0, prior_sample_size: float = 0.0,
                              reml: bool = False, optim_interval: int = 1, decomp_scheme: str = "eigen",
                              threshold: Optional[float] = None, trip_i=None, trip_j=None, trip_lod=None, trip_count=None,
                              status: bool = False):
    """blmm_bulkscan_loco_reduced_dev on torch CUDA tensors (layouts as bulkscan_loco_dev): max_out (m, float64), argmax_out (m,
    int64), chr_max_out (nchr, m, float64), chr_argmax_out (nchr, m, int64), h2_out (nchr, m; None for alt-grid) -- each may be
    None; threshold given: trip_i / trip_j (int32, cap), trip_lod (float64, cap), trip_count (int64, 1).  Enqueues on the context's
    stream; status=True synchronises."""
    m, n = Y.shape
    p = G.shape[0]
    cs = _check_chr_start(chr_start, p)
    nchr = cs.shape[0] - 1
    _check_n(n)
    meth = _method(method)
    grid, ngrid = _grid(meth, h2_grid)
    ncov, addIntercept, st = _dev_args(Covar, addIntercept, status)
    o = _opts(meth, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    want = threshold is not None
    r = L.blmm_reduced(_dptr(max_out), _dptr(argmax_out), 1 if want else 0, float(threshold) if want else 0.0,
                       int(trip_i.numel()) if want else 0, _dptr(trip_i) if want else None, _dptr(trip_j) if want else None,
                       _dptr(trip_lod) if want else None, _dptr(trip_count) if want else None)
    ctx.check(ctx.lib.blmm_bulkscan_loco_reduced_dev(ctx.h, C.byref(o), Y.data_ptr(), n, m, G.data_ptr(), p, _p(cs), nchr,
                                                     _kdigits(kinship_digits), _dptr(Covar), ncov, _dptr(weights), _p(grid), ngrid,
                                                     _dptr(K_loco), C.byref(r), _dptr(chr_max_out), _dptr(chr_argmax_out),
                                                     _dptr(h2_out), C.byref(st) if status else None))
    return st


# ---- the LOCO permutation test ---------------------------------------------------------------------------------------------------
BPERM_MAX_NPERMS = 16384   # blmm_api.hip: bperm_check -- k_bperm_summary sorts a trait's maxima in LDS
BPERM_MAX_COVARIATES = 8   # null covariates incl. the intercept (CTPL)


def _loco_perms_checks(n: int, nperms: int, ncov: int, addIntercept: bool, nprobs: int):
    """The library's refusals of blmm_bulkscan_loco_perms that need no data (blmm_api.hip: loco_perms_check), before any context."""
    _check_n(n)
    if nperms < 0:
        raise BulkLMMError("The required number of permutations must be a positive integer.", -9)
    if nperms > BPERM_MAX_NPERMS:
        raise BulkLMMError("bulkscan_loco_perms: more than 16384 permutations (the per-trait sort runs in LDS)", -10)
    if _null_covariates(ncov, addIntercept) > BPERM_MAX_COVARIATES:
        raise BulkLMMError("bulkscan_loco_perms: more than 8 null covariates (incl. intercept) are not supported", -10)
    if nprobs > 64:
        raise BulkLMMError("bulkscan_loco_perms: 0 .. 64 threshold levels", -1)


def bulkscan_loco_perms(Y, G, chrom, Covar=None, *, nperms: int = 1024, rndseed: int = 0, perm_idx=None, signif_level=(0.10, 0.05),
                        kinship_digits: Optional[int] = None, weights=None, prior_variance: float = 0.0, prior_sample_size: float = 0.0,
                        addIntercept: bool = True, reml: bool = False, optim_interval: int = 1, decomp_scheme: str = "eigen",
                        chr_max_perms: bool = False, ctx: Optional[Context] = None, return_status: bool = False) -> dict:
    """The leave-one-chromosome-out permutation test (blmm_bulkscan_loco_perms): bulkscan_perms on every chromosome's markers under
    its LOCO kinship, with ONE permutation set (perm_idx, or the generator seeded once by rndseed) for every chromosome and trait,
    and the genome-wide tables computed on the device.  With K_c = calcKinship_loco(G, chrom, kinship_digits)[c] and ref_c =
    bulkscan_perms(Y, G[:, rows_c], K_c, Covar; same options), row c of every "chr_" table is ref_c's, bit for bit (markers global
    and 0-based: ref_c's lod_argmax + chr_start[c], -1 kept).  Genome-wide: max_perms[b, j] = max_c chr_max_perms[c, b, j]; lod_max /
    lod_argmax the peak over all chromosomes (lowest global marker on ties, NaN never the maximum, -inf / -1 when nothing compares);
    thresholds get_thresholds' rule on max_perms[:, j]; pvals_perm (1 + #{b : max_perms[b, j] >= lod_max[j]}) / (nperms + 1).
    Convention: each chromosome permutes its own rotated, reweighted null residuals (scan_perms_lite under K_c), and permutation b's
    genome-wide maximum pairs the chromosomes' copies by b -- not one permutation of the individuals across chromosomes.  Keyword
    defaults are bulkscan_perms'.  Returns {"h2_null", "sigma2_e": (nchr, m); "lod_max", "lod_argmax", "pvals_perm": m;
    "max_perms": (nperms, m); "thresholds": (len(signif_level), m); "chr_lod_max", "chr_lod_argmax", "chr_pvals_perm": (nchr, m);
    "chr_thresholds": (nchr, len(signif_level), m) [; "chr_max_perms": (nchr, nperms, m) when chr_max_perms]; "probs";
    "chromosomes"; "chr_start" [; "status"]}.  nperms = 0: thresholds and p-values NaN."""
    Y, G, _, n, m, p = _host_arrays(Y, G)
    runs, cs = chromosome_runs(chrom, p)
    nchr = cs.shape[0] - 1
    nperms = int(nperms)
    cov, ncov, w, addIntercept = _host_covariates(Covar, weights, n, addIntercept)
    probs = _probs(signif_level)
    _loco_perms_checks(n, nperms, ncov, addIntercept, probs.shape[0])
    pidx = _perm_idx(perm_idx, n, nperms)
    if pidx is not None and pidx.size and (pidx.min() < 0 or pidx.max() >= n):
        raise BulkLMMError("bulkscan_loco_perms: perm_idx entries must lie in 0 .. n - 1", -1)
    o = _opts(L.BLMM_NULL_EXACT, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    ctx = ctx or default_context()  # after the argument checks: those must not need a GPU
    npr = probs.shape[0]
    h2, s2 = np.empty((nchr, m)), np.empty((nchr, m))          # row c: chromosome c (C order = the library's blocks)
    mx, pv = np.empty(m), np.empty(m)
    arg = np.empty(m, dtype=np.int64)
    mp = np.empty((max(nperms, 1), m), order="F")
    thr = np.empty((npr, m), order="F")
    cmx, cpv = np.empty((nchr, m)), np.empty((nchr, m))
    carg = np.empty((nchr, m), dtype=np.int64)
    cthr = np.empty((nchr, m, npr))                             # block c: nprobs x m column-major
    cmp = np.empty((nchr, m, max(nperms, 1))) if chr_max_perms else None
    st = L.blmm_status()
    ctx.check(ctx.lib.blmm_bulkscan_loco_perms(ctx.h, C.byref(o), _p(Y), n, m, _p(G), p, _p(cs), nchr,
                                               _kdigits(kinship_digits), _p(cov), ncov, _p(w), nperms,
                                               C.c_uint64(int(rndseed)), _p(pidx), _p(probs), npr, _p(h2), _p(s2), _p(mx), _p(arg),
                                               _p(mp), _p(thr), _p(pv), _p(cmx), _p(carg), _p(cmp), _p(cthr), _p(cpv), C.byref(st)))
    _raise_status(st)
    out = {"h2_null": h2, "sigma2_e": s2, "lod_max": mx, "lod_argmax": arg, "max_perms": mp[:nperms], "thresholds": thr,
           "pvals_perm": pv, "chr_lod_max": cmx, "chr_lod_argmax": carg, "chr_thresholds": cthr.transpose(0, 2, 1),
           "chr_pvals_perm": cpv, "probs": probs, "chromosomes": runs, "chr_start": cs}
    if chr_max_perms:
        out["chr_max_perms"] = cmp.transpose(0, 2, 1)[:, :nperms]
    if return_status:
        out["status"] = st
    return out


def bulkscan_loco_perms_dev(ctx: Context, Y, G, chr_start, h2_out, sigma2_out, lod_max_out, lod_argmax_out, max_perms_out=None,
                            thr_out=None, pval_out=None, chr_lod_max_out=None, chr_lod_argmax_out=None, chr_max_perms_out=None,
                            chr_thr_out=None, chr_pval_out=None, *, nperms: int, seed: int = 0, perm_idx=None,
                            signif_level=(0.10, 0.05), K_loco=None, kinship_digits: Optional[int] = None, Covar=None, weights=None,
                            addIntercept: bool = True, prior_variance: float = 0.0, prior_sample_size: float = 0.0, reml: bool = False,
                            optim_interval: int = 1, decomp_scheme: str = "eigen", status: bool = False):
    """blmm_bulkscan_loco_perms_dev on torch CUDA tensors (layouts as bulkscan_loco_dev / bulkscan_perms_dev): Y (m, n), G (p, n);
    chr_start: nchr + 1 host offsets; K_loco (nchr, n, n) as calcKinship_loco, or None (computed on the device); h2_out /
    sigma2_out / chr_lod_max_out / chr_pval_out (nchr, m) float64, chr_lod_argmax_out (nchr, m) int64; lod_max_out / pval_out (m,)
    float64, lod_argmax_out (m,) int64; max_perms_out (m, nperms) [= nperms x m column-major]; thr_out (m, len(signif_level));
    chr_thr_out (nchr, m, len(signif_level)); chr_max_perms_out (nchr, m, nperms); perm_idx (nperms, n) int32 or None (the
    library's generator with `seed`).  Outputs after lod_argmax_out may be None.  Enqueues on the context's stream (status=True
    synchronises it)."""
    m, n = Y.shape
    p = G.shape[0]
    cs = _check_chr_start(chr_start, p)
    nchr = cs.shape[0] - 1
    ncov, addIntercept, st = _dev_args(Covar, addIntercept, status)
    probs = _probs(signif_level)
    _loco_perms_checks(n, int(nperms), ncov, addIntercept, probs.shape[0])
    o = _opts(L.BLMM_NULL_EXACT, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    ctx.check(ctx.lib.blmm_bulkscan_loco_perms_dev(ctx.h, C.byref(o), Y.data_ptr(), n, m, G.data_ptr(), p, _p(cs), nchr,
                                                   _kdigits(kinship_digits), _dptr(Covar), ncov, _dptr(weights), int(nperms),
                                                   C.c_uint64(int(seed)), _dptr(perm_idx), _p(probs), probs.shape[0], _dptr(K_loco),
                                                   _dptr(h2_out), _dptr(sigma2_out), _dptr(lod_max_out), _dptr(lod_argmax_out),
                                                   _dptr(max_perms_out), _dptr(thr_out), _dptr(pval_out), _dptr(chr_lod_max_out),
                                                   _dptr(chr_lod_argmax_out), _dptr(chr_max_perms_out), _dptr(chr_thr_out),
                                                   _dptr(chr_pval_out), C.byref(st) if status else None))
    return st


# ---- the k-degree-of-freedom scan (blmm_bulkscan_multidf) ----------------------------------------------------------------------
_MULTIDF_KMAX = {"null-grid": L.BLMM_MULTIDF_MAX_K_GRID, "null-exact": L.BLMM_MULTIDF_MAX_K_EXACT}


def _multidf_checks(method: str, n: int, p: int, k, ncov: int, addIntercept: bool):
    """The library's refusals of blmm_bulkscan_multidf that need no data (blmm_api.hip: multidf_check), before any context."""
    if method not in _METHODS:
        raise BulkLMMError("Unknown method; choose null-exact, null-grid or alt-grid.", -5)
    k = int(k)
    if k < 1 or p % k != 0:
        raise BulkLMMError("bulkscan_multidf: the number of columns of G must be a multiple of k >= 1", -2)
    if method == "alt-grid":
        raise BulkLMMError("bulkscan_multidf: alt-grid is not supported; use null-grid or null-exact", -10)
    if k > _MULTIDF_KMAX[method]:
        raise BulkLMMError("bulkscan_multidf: %s takes 1 <= k <= %d" % (method, _MULTIDF_KMAX[method]), -10)
    if _null_covariates(ncov, addIntercept) > L.BLMM_MULTIDF_MAX_COVARIATES:
        raise BulkLMMError("bulkscan_multidf: more than 8 null covariates (incl. intercept) are not supported", -10)
    _check_n(n)
    return k


def bulkscan_multidf(Y, G, K, k: int, Covar=None, *, method: str = "null-grid", h2_grid=None, addIntercept: bool = True, weights=None,
                     prior_variance: float = 1.0, prior_sample_size: float = 0.0, reml: bool = False, optim_interval: int = 1,
                     decomp_scheme: str = "eigen", output_pvals: bool = False, chisq_df: Optional[int] = None,
                     keep_on_device: bool = False, ctx: Optional[Context] = None, return_status: bool = False) -> dict:
    """k-degree-of-freedom bulkscan (blmm_bulkscan_multidf; the reference's README lists it as future work): G is n x (P k), locus l
    is the columns l k .. l k + k - 1 (genotype or founder probabilities, additive + dominance codings) and every (locus, trait)
    pair gets one test of all its columns at once, L[l, j] = -(n/2) log10(1 - R^2) with R^2 the share of the trait's null residual
    that the locus explains.  Columns of a locus that add nothing beyond the covariates and the locus's earlier columns (|r|^2 <=
    1e-8 |x|^2: complements, duplicates, absent genotypes) are dropped.  Every other argument is bulkscan's; h2_null_list is
    bulkscan's, bit for bit.  `chisq_df` (output_pvals) defaults to k -- callers who pass complement columns choose k - 1.
    Returns {"L": P x m ndarray (DeviceLOD when keep_on_device), "h2_null_list": m [, "log10Pvals_mat", "Chisq_df"] [, "status"]}."""
    Y, G, K, n, m, p = _host_arrays(Y, G, K)
    cov, ncov, w, addIntercept = _host_covariates(Covar, weights, n, addIntercept)
    k = _multidf_checks(method, n, p, k, ncov, addIntercept)
    df = k if chisq_df is None else int(chisq_df)
    if output_pvals and not 1 <= df <= 1000000:
        raise BulkLMMError("chisq_df must lie in 1 .. 10^6", -1)
    meth = _METHODS[method]
    grid, ngrid = _grid(meth, h2_grid)
    o = _opts(meth, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    ctx = ctx or default_context()  # after the argument checks: those must not need a GPU
    P = p // k
    Lout = None if keep_on_device else np.empty((P, m), dtype=np.float64, order="F")
    h2 = np.empty(m, dtype=np.float64)
    st = L.blmm_status()
    with _log10p_output(ctx, df if output_pvals else None):
        ctx.check(ctx.lib.blmm_bulkscan_multidf(ctx.h, C.byref(o), _p(Y), n, m, _p(G), p, k, _p(cov), ncov, _p(K), _p(w), _p(grid), ngrid,
                                                _p(Lout), _p(h2), C.byref(st)))
    _raise_status(st)
    out = {"L": DeviceLOD(ctx, P, m) if keep_on_device else Lout, "h2_null_list": h2}
    if output_pvals:
        out["log10Pvals_mat"] = _last_log10p(ctx, (P, m), df)
        out["Chisq_df"] = df
    if return_status:
        out["status"] = st
    return out


def bulkscan_multidf_dev(ctx: Context, Y, G, K, k: int, L_out, h2_out, *, method: str = "null-grid", h2_grid=None, Covar=None,
                         weights=None, addIntercept: bool = True, prior_variance: float = 1.0, prior_sample_size: float = 0.0,
                         reml: bool = False, optim_interval: int = 1, decomp_scheme: str = "eigen", status: bool = False,
                         log10p_out=None, chisq_df: Optional[int] = None):
    """blmm_bulkscan_multidf_dev on torch tensors in bulkscan_dev's layout: Y (m, n), G (p, n) with p = P k, K (n, n), L_out (m, P)
    (= P x m column-major; rows may be padded), h2_out (m).  `log10p_out` (L_out's layout): -log10 p with chisq_df (default k) from
    the same call (blmm_set_log10p_output).  Enqueues on the context's stream; synchronises only for `status`."""
    m, n = Y.shape
    p = G.shape[0]
    ncov, addIntercept, st = _dev_args(Covar, addIntercept, status)
    k = _multidf_checks(method, n, p, k, ncov, addIntercept)
    P = p // k
    meth = _METHODS[method]
    grid, ngrid = _grid(meth, h2_grid)
    o = _opts(meth, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    with _log10p_output(ctx, None if log10p_out is None else (k if chisq_df is None else chisq_df), log10p_out, P):
        ctx.check(ctx.lib.blmm_bulkscan_multidf_dev(ctx.h, C.byref(o), Y.data_ptr(), n, m, G.data_ptr(), p, k, _dptr(Covar), ncov,
                                                    K.data_ptr(), _dptr(weights), _p(grid), ngrid, L_out.data_ptr(), _ld(L_out, P),
                                                    h2_out.data_ptr(), C.byref(st) if status else None))
    return st


def _reduced_cap(threshold, cap):
    if threshold is not None and int(cap) < 1:
        raise BulkLMMError("bulkscan_multidf_reduced: `threshold` needs a positive `cap`", -1)


def bulkscan_multidf_reduced(Y, G, K, k: int, Covar=None, *, method: str = "null-grid", h2_grid=None, threshold: Optional[float] = None,
                             cap: int = 1 << 20, addIntercept: bool = True, weights=None, prior_variance: float = 1.0,
                             prior_sample_size: float = 0.0, reml: bool = False, optim_interval: int = 1, decomp_scheme: str = "eigen",
                             ctx: Optional[Context] = None, return_status: bool = False) -> dict:
    """bulkscan_multidf WITHOUT the P x m matrix (blmm_bulkscan_multidf_reduced): per trait the peak LOD and its LOCUS and --
    `threshold` given -- every (locus, trait, LOD) with LOD > threshold, out of the k-df scan kernels' epilogues; bit-identical to
    lod_colmax / lod_threshold on bulkscan_multidf(...)["L"].  Arguments and refusals are bulkscan_multidf's; `cap` as in
    bulkscan_reduced.  Returns {"max_lod": m, "argmax": m (0-based locus, -1: no comparable entry), "h2_null_list": m [, "triplets":
    (locus, trait, lod) sorted by (trait, locus)], "route": 1 | 3 (traits the conditioning guard flagged were re-scanned)}."""
    Y, G, K, n, m, p = _host_arrays(Y, G, K)
    cov, ncov, w, addIntercept = _host_covariates(Covar, weights, n, addIntercept)
    k = _multidf_checks(method, n, p, k, ncov, addIntercept)
    _reduced_cap(threshold, cap)
    meth = _METHODS[method]
    grid, ngrid = _grid(meth, h2_grid)
    o = _opts(meth, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    ctx = ctx or default_context()  # after the argument checks: those must not need a GPU
    h2 = np.empty(m)

    def call(r, st):
        return ctx.lib.blmm_bulkscan_multidf_reduced(ctx.h, C.byref(o), _p(Y), n, m, _p(G), p, k, _p(cov), ncov, _p(K), _p(w), _p(grid),
                                                     ngrid, r, _p(h2), st)
    return _reduced_host(ctx, m, threshold, cap, call, {}, h2, return_status)


def bulkscan_multidf_reduced_dev(ctx: Context, Y, G, K, k: int, max_out, argmax_out, h2_out, *, method: str = "null-grid", h2_grid=None,
                                 Covar=None, weights=None, addIntercept: bool = True, prior_variance: float = 1.0,
                                 prior_sample_size: float = 0.0, reml: bool = False, optim_interval: int = 1,
                                 decomp_scheme: str = "eigen", threshold: Optional[float] = None, trip_i=None, trip_j=None,
                                 trip_lod=None, trip_count=None, status: bool = False):
    """blmm_bulkscan_multidf_reduced_dev on torch tensors (layouts as bulkscan_multidf_dev): max_out (m, float64) and argmax_out
    (m, int64), either may be None; threshold given: trip_i / trip_j (int32, cap), trip_lod (float64, cap), trip_count (int64, 1).
    Synchronises the stream."""
    m, n = Y.shape
    p = G.shape[0]
    ncov, addIntercept, st = _dev_args(Covar, addIntercept, status)
    k = _multidf_checks(method, n, p, k, ncov, addIntercept)
    want = threshold is not None
    _reduced_cap(threshold, trip_i.numel() if want and trip_i is not None else 0)
    meth = _METHODS[method]
    grid, ngrid = _grid(meth, h2_grid)
    o = _opts(meth, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    r = L.blmm_reduced(_dptr(max_out), _dptr(argmax_out), 1 if want else 0, float(threshold) if want else 0.0,
                       int(trip_i.numel()) if want else 0, _dptr(trip_i) if want else None, _dptr(trip_j) if want else None,
                       _dptr(trip_lod) if want else None, _dptr(trip_count) if want else None)
    ctx.check(ctx.lib.blmm_bulkscan_multidf_reduced_dev(ctx.h, C.byref(o), Y.data_ptr(), n, m, G.data_ptr(), p, k, _dptr(Covar), ncov,
                                                        K.data_ptr(), _dptr(weights), _p(grid), ngrid, C.byref(r), h2_out.data_ptr(),
                                                        C.byref(st) if status else None))
    return st


# ---- permutation thresholds of the k-degree-of-freedom scan (blmm_bulkscan_multidf_perms) --------------------------------------
def _multidf_perms_checks(n: int, p: int, k, nperms: int, ncov: int, addIntercept: bool, nprobs: int):
    """The library's refusals of blmm_bulkscan_multidf_perms that need no data (blmm_api.hip: mdf_perms_check), before any context:
    bulkscan_perms' on nperms, the covariates and the levels, bulkscan_multidf's (null-grid's limit on k) on k, p and n."""
    nperms = int(nperms)
    if nperms < 0:
        raise BulkLMMError("The required number of permutations must be a positive integer.", -9)
    if nprobs > 64:
        raise BulkLMMError("bulkscan_multidf_perms: 0 .. 64 threshold levels", -1)
    if nperms > BPERM_MAX_NPERMS:
        raise BulkLMMError("bulkscan_multidf_perms: more than 16384 permutations (the per-trait sort runs in LDS)", -10)
    if _null_covariates(ncov, addIntercept) > BPERM_MAX_COVARIATES:
        raise BulkLMMError("bulkscan_multidf_perms: more than 8 null covariates (incl. intercept) are not supported", -10)
    k = int(k)
    if k < 1 or p % k != 0:
        raise BulkLMMError("bulkscan_multidf_perms: the number of columns of G must be a multiple of k >= 1", -2)
    if k > L.BLMM_MULTIDF_MAX_K_GRID:
        raise BulkLMMError("bulkscan_multidf_perms: takes 1 <= k <= %d" % L.BLMM_MULTIDF_MAX_K_GRID, -10)
    _check_n(n)
    return k, nperms


def bulkscan_multidf_perms(Y, G, K, k: int, Covar=None, *, nperms: int = 1024, rndseed: int = 0, perm_idx=None,
                           signif_level=(0.10, 0.05), weights=None, prior_variance: float = 0.0, prior_sample_size: float = 0.0,
                           addIntercept: bool = True, reml: bool = False, optim_interval: int = 1, decomp_scheme: str = "eigen",
                           ctx: Optional[Context] = None, return_status: bool = False) -> dict:
    """Permutation thresholds for the k-degree-of-freedom scan (blmm_bulkscan_multidf_perms): bulkscan_perms with bulkscan_multidf's
    loci.  G is n x (P k), locus l the columns l k .. l k + k - 1; every trait's null model is bulkscan_perms' (h2_null and sigma2_e
    bit for bit, the same permutation set for the same rndseed / perm_idx), and permutation b of trait j is scanned as
    L_b[l] = -(n/2) log10(1 - |P_Q (I - P_Z) v_b|^2 / |v_b|^2), v_b the permuted, reweighted null residual and Q the locus's accepted
    columns (bulkscan_multidf's rank rule at the trait's own weights, 1 <= k <= 8).  The unpermuted column is bulkscan_multidf's
    null-exact LOD.  Only the reductions leave the device.  Returns bulkscan_perms' keys: {"h2_null", "sigma2_e", "lod_max",
    "lod_argmax" (0-based LOCUS, -1 with lod_max = -inf when nothing compares): m each; "max_perms": nperms x m; "thresholds":
    len(signif_level) x m; "pvals_perm": m; "probs" [; "status"]}.  nperms = 0: thresholds and p-values NaN."""
    Y, G, K, n, m, p = _host_arrays(Y, G, K)
    cov, ncov, w, addIntercept = _host_covariates(Covar, weights, n, addIntercept)
    probs = _probs(signif_level)
    k, nperms = _multidf_perms_checks(n, p, k, nperms, ncov, addIntercept, probs.shape[0])
    pidx = _perm_idx(perm_idx, n, nperms)
    if pidx is not None and pidx.size and (pidx.min() < 0 or pidx.max() >= n):
        raise BulkLMMError("bulkscan_multidf_perms: perm_idx entries must lie in 0 .. n - 1", -1)
    o = _opts(L.BLMM_NULL_EXACT, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    ctx = ctx or default_context()  # after the argument checks: those must not need a GPU
    st = L.blmm_status()
    h2, s2, mx, pv = np.empty(m), np.empty(m), np.empty(m), np.empty(m)
    arg = np.empty(m, dtype=np.int64)
    mp = np.empty((max(nperms, 1), m), order="F")
    thr = np.empty((probs.shape[0], m), order="F")
    ctx.check(ctx.lib.blmm_bulkscan_multidf_perms(ctx.h, C.byref(o), _p(Y), n, m, _p(G), p, k, _p(cov), ncov, _p(K), _p(w), nperms,
                                                  C.c_uint64(int(rndseed)), _p(pidx), _p(probs), probs.shape[0], _p(h2), _p(s2), _p(mx),
                                                  _p(arg), _p(mp), _p(thr), _p(pv), C.byref(st)))
    _raise_status(st)
    out = {"h2_null": h2, "sigma2_e": s2, "lod_max": mx, "lod_argmax": arg, "max_perms": mp[:nperms], "thresholds": thr,
           "pvals_perm": pv, "probs": probs}
    if return_status:
        out["status"] = st
    return out


def bulkscan_multidf_perms_dev(ctx: Context, Y, G, K, k: int, h2_out, sigma2_out, lod_max_out, lod_argmax_out, max_perms_out=None,
                               thr_out=None, pval_out=None, *, nperms: int, seed: int = 0, perm_idx=None, signif_level=(0.10, 0.05),
                               Covar=None, weights=None, addIntercept: bool = True, prior_variance: float = 0.0,
                               prior_sample_size: float = 0.0, reml: bool = False, optim_interval: int = 1,
                               decomp_scheme: str = "eigen", status: bool = False):
    """blmm_bulkscan_multidf_perms_dev on torch tensors in bulkscan_perms_dev's layout: Y (m, n), G (p, n) with p = P k, K (n, n);
    h2_out / sigma2_out / lod_max_out / pval_out (m,) float64, lod_argmax_out (m,) int64 (loci), max_perms_out (m, nperms),
    thr_out (m, len(signif_level)), perm_idx (nperms, n) int32 or None (the library's generator with `seed`).  Enqueues on the
    context's stream (status=True synchronises it)."""
    m, n = Y.shape
    p = G.shape[0]
    ncov, addIntercept, st = _dev_args(Covar, addIntercept, status)
    probs = _probs(signif_level)
    k, nperms = _multidf_perms_checks(n, p, k, nperms, ncov, addIntercept, probs.shape[0])
    o = _opts(L.BLMM_NULL_EXACT, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    ctx.check(ctx.lib.blmm_bulkscan_multidf_perms_dev(ctx.h, C.byref(o), Y.data_ptr(), n, m, G.data_ptr(), p, k, _dptr(Covar), ncov,
                                                      K.data_ptr(), _dptr(weights), nperms, C.c_uint64(int(seed)), _dptr(perm_idx),
                                                      _p(probs), probs.shape[0], h2_out.data_ptr(), sigma2_out.data_ptr(),
                                                      lod_max_out.data_ptr(), lod_argmax_out.data_ptr(), _dptr(max_perms_out),
                                                      _dptr(thr_out), _dptr(pval_out), C.byref(st) if status else None))
    return st


# ---- effects at chosen tests (blmm_bulkscan_effects) ---------------------------------------------------------------------------
def _effects_checks(method: str, n: int, p: int, k, ncov: int, addIntercept: bool):
    """The library's refusals of blmm_bulkscan_effects that need no data (blmm_api.hip: effects_check), before any context."""
    if method not in _METHODS:
        raise BulkLMMError("Unknown method; choose null-exact, null-grid or alt-grid.", -5)
    k = int(k)
    if k < 1 or p % k != 0:
        raise BulkLMMError("bulkscan_effects: the number of columns of G must be a multiple of k >= 1", -2)
    if method == "alt-grid":
        raise BulkLMMError("bulkscan_effects: alt-grid is not supported; use null-grid or null-exact", -10)
    if k > L.BLMM_EFFECTS_MAX_K:
        raise BulkLMMError("bulkscan_effects: takes 1 <= k <= %d" % L.BLMM_EFFECTS_MAX_K, -10)
    if _null_covariates(ncov, addIntercept) > L.BLMM_MULTIDF_MAX_COVARIATES:
        raise BulkLMMError("bulkscan_effects: more than 8 null covariates (incl. intercept) are not supported", -10)
    _check_n(n)
    return k


def _effects_tests(locus, trait, nloci: int, m: int):
    """The test lists as flat int64 arrays of one length with every index in range (BLMM_ERR_INVALID otherwise)."""
    loc = np.ascontiguousarray(np.asarray(locus, dtype=np.int64).ravel())
    tr = np.ascontiguousarray(np.asarray(trait, dtype=np.int64).ravel())
    if loc.shape[0] != tr.shape[0]:
        raise BulkLMMError("bulkscan_effects: locus and trait must have the same length", -1)
    if loc.size and (loc.min() < 0 or loc.max() >= nloci or tr.min() < 0 or tr.max() >= m):
        raise BulkLMMError("bulkscan_effects: a locus or trait index is out of range", -1)
    return loc, tr


def bulkscan_effects(Y, G, K, Covar=None, *, k: int = 1, locus=None, trait=None, method: str = "null-grid", h2_grid=None,
                     addIntercept: bool = True, weights=None, prior_variance: float = 1.0, prior_sample_size: float = 0.0,
                     reml: bool = False, optim_interval: int = 1, decomp_scheme: str = "eigen", ctx: Optional[Context] = None,
                     return_status: bool = False) -> dict:
    """Coefficients and standard errors at chosen tests (blmm_bulkscan_effects; the reference's scan_null fits them per marker and
    keeps only the rss).  G is n x (P k), locus l the columns l k .. l k + k - 1 (k = 1: the ordinary marker test); test t is
    (locus[t], trait[t]), 0-based, in any order, repeats allowed.  Per test: `beta` and `se` (T x k) of the locus columns in the
    weighted least-squares fit wls(y0_j, [Z0 X0_l], w) under the trait's null h2 (a column the rank rule of bulkscan_multidf drops has
    beta = se = 0), `sigma2` (wls's sigma2_e of that fit: (rss1 + prior) / (n + prior_df), n - (c + accepted columns) under reml),
    `lod` (what bulkscan / bulkscan_multidf writes at L[locus, trait]) and `accepted` (int32 bit mask of the columns kept).
    `h2_null_list` is bulkscan's, bit for bit.  Every other argument is bulkscan's; alt-grid is refused, k <= 8, at most 8 null
    covariates.  With locus and trait both omitted (k = 1 only) the matching bulkscan_reduced runs first and the tests are every
    trait's peak: locus = its argmax, trait = 0 .. m - 1 (both are returned).  LOCO: call once per chromosome with calcKinship_loco's
    kinship of that chromosome and its tests.
    Returns {"beta", "se", "sigma2", "lod", "accepted", "h2_null_list", "locus", "trait" [, "status"]}."""
    Y, G, K, n, m, p = _host_arrays(Y, G, K)
    cov, ncov, w, addIntercept = _host_covariates(Covar, weights, n, addIntercept)
    k = _effects_checks(method, n, p, k, ncov, addIntercept)
    if (locus is None) != (trait is None):
        raise BulkLMMError("bulkscan_effects: give both locus and trait, or neither (every trait's peak, k = 1)", -1)
    if locus is None:
        if k != 1:
            raise BulkLMMError("bulkscan_effects: locus and trait are required for k > 1 (bulkscan_multidf_reduced gives every trait's peak locus)", -1)
        peaks = bulkscan_reduced(Y, G, K, Covar, method=method, h2_grid=h2_grid, addIntercept=addIntercept, weights=weights,
                                 prior_variance=prior_variance, prior_sample_size=prior_sample_size, reml=reml,
                                 optim_interval=optim_interval, decomp_scheme=decomp_scheme, ctx=ctx)
        locus, trait = np.maximum(peaks["argmax"], 0), np.arange(m)   # (-1: a trait without a finite LOD -- its marker 0 then)
    loc, tr = _effects_tests(locus, trait, p // k, m)
    T = loc.shape[0]
    meth = _METHODS[method]
    grid, ngrid = _grid(meth, h2_grid)
    o = _opts(meth, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    ctx = ctx or default_context()  # after the argument checks: those must not need a GPU
    beta, se = np.empty((T, k)), np.empty((T, k))
    sigma2, lod, acc, h2 = np.empty(T), np.empty(T), np.empty(T, dtype=np.int32), np.empty(m)
    st = L.blmm_status()
    ctx.check(ctx.lib.blmm_bulkscan_effects(ctx.h, C.byref(o), _p(Y), n, m, _p(G), p, k, _p(cov), ncov, _p(K), _p(w), _p(grid), ngrid,
                                            _p(loc), _p(tr), T, _p(beta), _p(se), _p(sigma2), _p(lod), _p(acc), _p(h2), C.byref(st)))
    _raise_status(st)
    out = {"beta": beta, "se": se, "sigma2": sigma2, "lod": lod, "accepted": acc, "h2_null_list": h2, "locus": loc, "trait": tr}
    if return_status:
        out["status"] = st
    return out


def bulkscan_effects_dev(ctx: Context, Y, G, K, k: int, locus, trait, beta_out, se_out, sigma2_out, lod_out, accepted_out, h2_out, *,
                         method: str = "null-grid", h2_grid=None, Covar=None, weights=None, addIntercept: bool = True,
                         prior_variance: float = 1.0, prior_sample_size: float = 0.0, reml: bool = False, optim_interval: int = 1,
                         decomp_scheme: str = "eigen", status: bool = False):
    """blmm_bulkscan_effects_dev on torch tensors in bulkscan_dev's layout: Y (m, n), G (p, n) with p = P k, K (n, n); locus, trait
    (T,) int64; beta_out, se_out (T, k) contiguous float64; sigma2_out, lod_out (T,) float64; accepted_out (T,) int32; h2_out (m).
    Enqueues on the context's stream; synchronises only for `status`.  The indices are on the device and not inspected here: a test
    out of range gets NaN / accepted = -1 and, with `status`, the call raises."""
    m, n = Y.shape
    p = G.shape[0]
    ncov, addIntercept, st = _dev_args(Covar, addIntercept, status)
    k = _effects_checks(method, n, p, k, ncov, addIntercept)
    T = locus.shape[0]
    if trait.shape[0] != T:
        raise BulkLMMError("bulkscan_effects: locus and trait must have the same length", -1)
    if tuple(beta_out.shape) != (T, k) or tuple(se_out.shape) != (T, k) or not beta_out.is_contiguous() or not se_out.is_contiguous():
        raise ValueError("beta_out and se_out must be contiguous (T, k) tensors")
    meth = _METHODS[method]
    grid, ngrid = _grid(meth, h2_grid)
    o = _opts(meth, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    ctx.check(ctx.lib.blmm_bulkscan_effects_dev(ctx.h, C.byref(o), Y.data_ptr(), n, m, G.data_ptr(), p, k, _dptr(Covar), ncov,
                                                K.data_ptr(), _dptr(weights), _p(grid), ngrid, locus.data_ptr(), trait.data_ptr(), T,
                                                beta_out.data_ptr(), se_out.data_ptr(), sigma2_out.data_ptr(), lod_out.data_ptr(),
                                                accepted_out.data_ptr(), h2_out.data_ptr(), C.byref(st) if status else None))
    return st


# ---- the conditional scan (blmm_bulkscan_cond) -----------------------------------------------------------------------------------
def _cond_table(cond, m: int, p: int):
    """cond as the library takes it: (m, s) int64, C order (entry [j, a] at j s + a); indices in [-1, p)."""
    c = np.asarray(cond)
    if c.dtype.kind not in "iu":
        raise BulkLMMError("bulkscan_cond: cond must hold integer column indices of G (or -1), or be \"peak\"", -1)
    if c.ndim == 1:
        c = c.reshape(-1, 1)
    if c.ndim != 2 or c.shape[0] != m:
        raise BulkLMMError("bulkscan_cond: cond must have shape (m,) or (m, s)", -2)
    return np.ascontiguousarray(c, dtype=np.int64)


def _cond_checks(method: str, n: int, s: int, ncov: int, addIntercept: bool):
    """The library's refusals of blmm_bulkscan_cond that need no data (blmm_api.hip: cond_check), before any context."""
    if method not in _METHODS:
        raise BulkLMMError("Unknown method; choose null-exact, null-grid or alt-grid.", -5)
    if method == "alt-grid":
        raise BulkLMMError("bulkscan_cond: alt-grid is not supported; use null-grid or null-exact", -10)
    if s > L.BLMM_COND_MAX_LOCI:
        raise BulkLMMError("bulkscan_cond: at most 4 conditioning loci per trait", -10)
    c = _null_covariates(ncov, addIntercept)
    if c + s > L.BLMM_MULTIDF_MAX_COVARIATES:
        raise BulkLMMError("bulkscan_cond: more than 8 null-design columns (covariates incl. intercept + conditioning loci) are not supported", -10)
    _check_n(n)
    if c + s >= n:
        raise BulkLMMError("Dimension mismatch.", -2)


def _cond_indices(c: np.ndarray, p: int):
    bad = np.nonzero(((c < -1) | (c >= p)).any(axis=1))[0]
    if bad.size:
        raise BulkLMMError("bulkscan_cond: trait %d has a conditioning index outside [-1, p)" % int(bad[0]), -1)


def bulkscan_cond(Y, G, K, cond, Covar=None, *, method: str = "null-grid", h2_grid=None, addIntercept: bool = True, weights=None,
                  prior_variance: float = 1.0, prior_sample_size: float = 0.0, reml: bool = False, optim_interval: int = 1,
                  decomp_scheme: str = "eigen", output_pvals: bool = False, chisq_df: int = 1, keep_on_device: bool = False,
                  return_status: bool = False, ctx: Optional[Context] = None) -> dict:
    """bulkscan of every trait CONDITIONAL on its own loci (blmm_bulkscan_cond): column j of L is the scan of trait j with the null
    design [Covar, G[:, cond[j]]] -- secondary QTL given the peak, forward selection.  `cond`: (m,) or (m, s) integer column indices
    of G (0-based), -1 for none, s <= 4; or the string "peak": bulkscan_reduced runs first with the same method and options and
    every trait is conditioned on its arg-max marker.  Conditioning columns that add nothing beyond the covariates and the trait's
    earlier ones (repeats, constants) are dropped; markers collinear with a trait's design (the conditioning marker itself, its
    duplicates) get LOD +0.0.  h2_null_list is the null model WITH the conditioning loci.
    Returns {"L": p x m (DeviceLOD when keep_on_device), "h2_null_list": m, "cond": (m, s) as used, "n_rule_zero", "n_cond_dropped",
    "n_cond_traits" [, "log10Pvals_mat", "Chisq_df"] [, "status"]}."""
    Y, G, K, n, m, p = _host_arrays(Y, G, K)
    cov, ncov, w, addIntercept = _host_covariates(Covar, weights, n, addIntercept)
    peak = isinstance(cond, str)
    if peak and cond != "peak":
        raise BulkLMMError("bulkscan_cond: cond is an index array or the string \"peak\"", -1)
    ctab = None if peak else _cond_table(cond, m, p)
    s = 1 if peak else ctab.shape[1]
    _cond_checks(method, n, s, ncov, addIntercept)
    if not peak:
        _cond_indices(ctab, p)
    if output_pvals and not 1 <= int(chisq_df) <= 1000000:
        raise BulkLMMError("chisq_df must lie in 1 .. 10^6", -1)
    meth = _METHODS[method]
    grid, ngrid = _grid(meth, h2_grid)
    o = _opts(meth, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    ctx = ctx or default_context()  # after the argument checks: those must not need a GPU
    if peak:
        red = bulkscan_reduced(Y, G, K, Covar, method=method, h2_grid=h2_grid, addIntercept=addIntercept, weights=weights,
                               prior_variance=prior_variance, prior_sample_size=prior_sample_size, reml=reml,
                               optim_interval=optim_interval, decomp_scheme=decomp_scheme, ctx=ctx)
        ctab = np.ascontiguousarray(np.asarray(red["argmax"], dtype=np.int64).reshape(m, 1))
    Lout = None if keep_on_device else np.empty((p, m), dtype=np.float64, order="F")
    h2 = np.empty(m, dtype=np.float64)
    info = np.zeros(L.BLMM_COND_INFO_LEN, dtype=np.int64)
    st = L.blmm_status()
    with _log10p_output(ctx, int(chisq_df) if output_pvals else None):
        ctx.check(ctx.lib.blmm_bulkscan_cond(ctx.h, C.byref(o), _p(Y), n, m, _p(G), p, _p(cov), ncov, _p(K), _p(w), _p(grid), ngrid,
                                             _p(ctab) if s > 0 else None, s, _p(Lout), _p(h2), _p(info), C.byref(st)))
    _raise_status(st)
    out = {"L": DeviceLOD(ctx, p, m) if keep_on_device else Lout, "h2_null_list": h2, "cond": ctab,
           "n_rule_zero": int(info[0]), "n_cond_dropped": int(info[1]), "n_cond_traits": int(info[2])}
    if output_pvals:
        out["log10Pvals_mat"] = _last_log10p(ctx, (p, m), int(chisq_df))
        out["Chisq_df"] = int(chisq_df)
    if return_status:
        out["status"] = st
    return out


def bulkscan_cond_dev(ctx: Context, Y, G, K, cond, L_out, h2_out, *, cinfo_out=None, method: str = "null-grid", h2_grid=None,
                      Covar=None, weights=None, addIntercept: bool = True, prior_variance: float = 1.0,
                      prior_sample_size: float = 0.0, reml: bool = False, optim_interval: int = 1, decomp_scheme: str = "eigen",
                      status: bool = False, log10p_out=None, chisq_df: int = 1):
    """blmm_bulkscan_cond_dev on torch tensors in bulkscan_dev's layout: Y (m, n), G (p, n), K (n, n), cond (m, s) int64 contiguous (or
    None), L_out (m, p) (= p x m column-major; rows may be padded), h2_out (m), cinfo_out (4) int64 or None.  The indices are not
    looked at on the host: a trait with one outside [-1, p) gets NaNs, and the call raises when `status` is asked for.  Enqueues on
    the context's stream; synchronises only for `status`."""
    m, n = Y.shape
    p = G.shape[0]
    ncov, addIntercept, st = _dev_args(Covar, addIntercept, status)
    s = 0 if cond is None else int(cond.shape[1])
    if cond is not None and (cond.dim() != 2 or cond.shape[0] != m or not cond.is_contiguous() or cond.element_size() != 8):
        raise BulkLMMError("bulkscan_cond: cond must be a contiguous (m, s) int64 tensor", -2)
    _cond_checks(method, n, s, ncov, addIntercept)
    meth = _METHODS[method]
    grid, ngrid = _grid(meth, h2_grid)
    o = _opts(meth, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    with _log10p_output(ctx, None if log10p_out is None else chisq_df, log10p_out, p):
        ctx.check(ctx.lib.blmm_bulkscan_cond_dev(ctx.h, C.byref(o), Y.data_ptr(), n, m, G.data_ptr(), p, _dptr(Covar), ncov, K.data_ptr(),
                                                 _dptr(weights), _p(grid), ngrid, _dptr(cond) if s > 0 else None, s, L_out.data_ptr(),
                                                 _ld(L_out, p), h2_out.data_ptr(), _dptr(cinfo_out), C.byref(st) if status else None))
    return st


# ---- forward selection (blmm_bulkscan_stepwise) ----------------------------------------------------------------------------------
def _stepwise_checks(method: str, n: int, max_loci, threshold, ncov: int, addIntercept: bool):
    """The library's refusals of blmm_bulkscan_stepwise that need no data (blmm_api.hip: stepwise_check), in its order."""
    try:
        S = operator.index(max_loci)
    except TypeError:
        raise BulkLMMError("bulkscan_stepwise: max_loci must be an integer", -1) from None
    if S < 1:
        raise BulkLMMError("bulkscan_stepwise: max_loci must be at least 1", -1)
    if S > L.BLMM_COND_MAX_LOCI:
        raise BulkLMMError("bulkscan_stepwise: at most 4 loci per trait", -10)
    if _null_covariates(ncov, addIntercept) + S > L.BLMM_MULTIDF_MAX_COVARIATES:
        raise BulkLMMError("bulkscan_stepwise: more than 8 null-design columns (covariates incl. intercept + max_loci) are not supported", -10)
    if not float(threshold) >= 0.0:
        raise BulkLMMError("bulkscan_stepwise: the threshold must be a number >= 0", -1)
    _cond_checks(method, n, S, ncov, addIntercept)
    return S


def bulkscan_stepwise(Y, G, K, Covar=None, *, max_loci: int = 4, threshold: float, method: str = "null-grid", h2_grid=None,
                      addIntercept: bool = True, weights=None, prior_variance: float = 1.0, prior_sample_size: float = 0.0,
                      reml: bool = False, optim_interval: int = 1, decomp_scheme: str = "eigen", return_status: bool = False,
                      ctx: Optional[Context] = None) -> dict:
    """Forward selection of up to `max_loci` loci per trait (blmm_bulkscan_stepwise): round t scans every trait still active with
    the loci it has so far in its null model -- bit for bit bulkscan_cond with the table of the round, reduced to the column
    maxima -- and a trait whose peak LOD is above `threshold` (strictly) takes the peak marker as its next locus.  One upload, one
    eigen phase, no p x m matrix; from round 1 on only the active traits are scanned.
    Returns {"loci": (m, S) int64, -1 beyond a trait's loci (bulkscan_cond takes it as `cond`), "lod", "argmax", "h2": (m, S + 1),
    NaN / -1 / NaN for the rounds a trait was not active in, "nloci": (m,), "rounds", "active": (S + 1,) traits per round,
    "n_rule_zero", "n_cond_traits" [, "status"]}."""
    Y, G, K, n, m, p = _host_arrays(Y, G, K)
    cov, ncov, w, addIntercept = _host_covariates(Covar, weights, n, addIntercept)
    S = _stepwise_checks(method, n, max_loci, threshold, ncov, addIntercept)
    meth = _METHODS[method]
    grid, ngrid = _grid(meth, h2_grid)
    o = _opts(meth, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    ctx = ctx or default_context()  # after the argument checks: those must not need a GPU
    loci = np.empty((m, S), dtype=np.int64)
    lod = np.empty((m, S + 1), dtype=np.float64)
    arg = np.empty((m, S + 1), dtype=np.int64)
    h2 = np.empty((m, S + 1), dtype=np.float64)
    nloci = np.empty(m, dtype=np.int64)
    info = np.zeros(L.BLMM_STEP_INFO_LEN, dtype=np.int64)
    st = L.blmm_status()
    ctx.check(ctx.lib.blmm_bulkscan_stepwise(ctx.h, C.byref(o), _p(Y), n, m, _p(G), p, _p(cov), ncov, _p(K), _p(w), _p(grid), ngrid,
                                             S, float(threshold), _p(loci), _p(lod), _p(arg), _p(h2), _p(nloci), _p(info), C.byref(st)))
    _raise_status(st)
    out = {"loci": loci, "lod": lod, "argmax": arg, "h2": h2, "nloci": nloci, "rounds": int(info[0]),
           "active": info[3:4 + S].copy(), "n_rule_zero": int(info[2]), "n_cond_traits": int(info[1])}
    if return_status:
        out["status"] = st
    return out


def bulkscan_stepwise_dev(ctx: Context, Y, G, K, loci_out, lod_out, argmax_out, h2_out, nloci_out, *, threshold: float, sinfo_out=None,
                          method: str = "null-grid", h2_grid=None, Covar=None, weights=None, addIntercept: bool = True,
                          prior_variance: float = 1.0, prior_sample_size: float = 0.0, reml: bool = False, optim_interval: int = 1,
                          decomp_scheme: str = "eigen", status: bool = False):
    """blmm_bulkscan_stepwise_dev on torch tensors in bulkscan_dev's layout: Y (m, n), G (p, n), K (n, n); loci_out (m, S) int64 --
    its width is max_loci --, lod_out / argmax_out / h2_out (m, S + 1) (float64 / int64 / float64), nloci_out (m) int64, sinfo_out (8)
    int64 or None, all contiguous.  Enqueues on the context's stream and waits for it between the rounds; without `status` the
    results are valid after ctx.synchronize()."""
    m, n = Y.shape
    p = G.shape[0]
    ncov, addIntercept, st = _dev_args(Covar, addIntercept, status)
    if loci_out.dim() != 2:
        raise BulkLMMError("bulkscan_stepwise: loci_out must be a contiguous (m, max_loci) int64 tensor", -2)
    S = _stepwise_checks(method, n, int(loci_out.shape[1]), threshold, ncov, addIntercept)   # the library's refusals first, in its order
    if loci_out.shape[0] != m or not loci_out.is_contiguous() or loci_out.element_size() != 8:
        raise BulkLMMError("bulkscan_stepwise: loci_out must be a contiguous (m, max_loci) int64 tensor", -2)
    for t in (lod_out, argmax_out, h2_out):
        if tuple(t.shape) != (m, S + 1) or not t.is_contiguous() or t.element_size() != 8:
            raise BulkLMMError("bulkscan_stepwise: lod_out, argmax_out and h2_out must be contiguous (m, max_loci + 1) 8-byte tensors", -2)
    if nloci_out.numel() != m or nloci_out.element_size() != 8:
        raise BulkLMMError("bulkscan_stepwise: nloci_out must hold m int64 values", -2)
    meth = _METHODS[method]
    grid, ngrid = _grid(meth, h2_grid)
    o = _opts(meth, reml, addIntercept, decomp_scheme, optim_interval, prior_variance, prior_sample_size)
    ctx.check(ctx.lib.blmm_bulkscan_stepwise_dev(ctx.h, C.byref(o), Y.data_ptr(), n, m, G.data_ptr(), p, _dptr(Covar), ncov, K.data_ptr(),
                                                 _dptr(weights), _p(grid), ngrid, S, float(threshold), loci_out.data_ptr(),
                                                 lod_out.data_ptr(), argmax_out.data_ptr(), h2_out.data_ptr(), nloci_out.data_ptr(),
                                                 _dptr(sinfo_out), C.byref(st) if status else None))
    return st
