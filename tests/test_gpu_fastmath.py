"""The device's LOD, logarithm, reciprocal and -log10 p primitives (bulklmm.jl_amd/csrc/fastmath.h, kernels_post.hip) over their whole
ranges, each against an independent high-precision reference: long double (64-bit mantissa), exact rationals or mpmath.

tests/hip/math_probe.hip runs the product's own inline functions one value per lane, with the tables staged as the kernels stage
them; it is built here with the library's compiler flags.  The end-to-end suites compare at 1e-6 relative; these bounds are the
functions' own claims.  Every test prints its worst error and where it occurs."""
import ctypes as C
import os
import re
import shutil
import subprocess

import mpmath as mp
import numpy as np
import pytest

from fastmath_tables import CSRC, ROOT, log_tables, pv_bucket, pval_table

pytestmark = pytest.mark.gpu

LN10 = np.log(10.0)
HI0 = 0x3FB00000                    # BLMM_LOD_HI0: u = 2^-4
LOD_BOUND = 4e-16                   # fast_lod5 / lod_out_of_range, relative
LIBM_ULPS = 4                       # fast map against the re-scan kernels' scale * log10(u), ulps of the larger
LOG_ULPS = 2                        # fast_log<false>, fast_log<true>
FAST_LOD_ULPS = 3                   # fast_lod: scale * log10(c) is rounded once more in the staged table (2.24 measured)
RSQRT_ULPS = 2                      # nr_rsqrt, fast_rsqrt
PV_BOUND = 1e-14                    # fast_log10p1 and the libm route, relative (absolute below t = LOD ln 10 = 1e-290)
DF_RTOL, DF_ATOL = 1e-10, 1e-14     # general df (test_gpu_parity.py's bound for lod2log10p)


def _ld(x):
    return np.asarray(x, dtype=np.longdouble)


def _ulps(got, ref):
    """|got - ref| in units of the last place of ref rounded to double (ref: long double)"""
    r64 = ref.astype(np.float64)
    return (np.abs(_ld(got) - ref) / _ld(np.spacing(np.abs(r64)))).astype(np.float64)


def _worst(err, arg, label):
    k = int(np.nanargmax(err))
    print(f"{label}: worst {float(err[k]):.4g} at {float(arg[k])!r}")
    return float(err[k]), float(arg[k])


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    assert np.finfo(np.longdouble).nmant >= 63, "the references need an x87 long double (64-bit mantissa)"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.isfile(hipcc) or shutil.which(hipcc)):
        pytest.fail(f"hipcc not found at {hipcc}: the probe cannot be built")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", arch).split()
    assert "-ffp-contract=on" in flags
    out = str(tmp_path_factory.mktemp("math_probe") / "math_probe.so")
    src = os.path.join(ROOT, "tests", "hip", "math_probe.hip")
    r = subprocess.run(["timeout", "-k", "10", "300", hipcc, *flags, "-shared", "-I", CSRC, src, "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lib = C.CDLL(out)
    vp, i64, dbl_t = C.c_void_p, C.c_int64, C.c_double
    lib.probe_lod5.argtypes = [vp, vp, vp, i64, dbl_t, C.c_int, vp]
    lib.probe_log.argtypes = [vp, vp, vp, vp, i64, dbl_t]
    lib.probe_rcp.argtypes = [vp, vp, i64]
    lib.probe_log10p1.argtypes = [vp, vp, i64]
    lib.probe_f32_scan.argtypes = [C.c_uint32, i64, C.c_float, dbl_t, C.c_int, vp, vp]
    lib.probe_stage.argtypes = [C.c_int, dbl_t, dbl_t, vp, vp, vp]
    return lib


def _p(a):
    return a.ctypes.data


def lod5(probe, u, scale, counted=True):
    u = np.ascontiguousarray(u, dtype=np.float64)
    out, libm, cnt = np.empty_like(u), np.empty_like(u), np.zeros(1, np.int64)
    assert probe.probe_lod5(_p(u), _p(out), _p(libm), u.size, scale, int(counted), _p(cnt)) == 0
    return out, libm, int(cnt[0])


def log10p1(probe, lod):
    lod = np.ascontiguousarray(lod, dtype=np.float64)
    out = np.empty_like(lod)
    assert probe.probe_log10p1(_p(lod), _p(out), lod.size) == 0
    return out


# ---- 1 + 3: the scan epilogues' LOD map on [2^-4, 1], every high word ----------------------------------------------------------
@pytest.mark.parametrize("n", [3, 79, 500, 2048])
def test_fast_lod5_every_high_word(probe, n):
    """lod_fast_ok ? fast_lod5 : lod_out_of_range (kernels_scan.hip's epilogue) for every high word of [2^-4, 1] with the low
    words 0, 1, 2^31, 2^32 - 1 and one random: within 4e-16 relative of -n/2 log10(u), exactly 0 at u = 1; and within a few
    ulps of the libm map scale * log10(u) of the re-scan kernels, so that a flagged trait's LODs agree with its neighbours'."""
    scale = -0.5 * n
    rng = np.random.default_rng(n)
    his = np.arange(HI0, 0x3FF00000, dtype=np.uint64)
    los = [np.zeros_like(his), np.ones_like(his), np.full_like(his, 1 << 31), np.full_like(his, 0xFFFFFFFF),
           rng.integers(0, 1 << 32, his.size, dtype=np.uint64)]
    bits = np.concatenate([(his << np.uint64(32)) | lo for lo in los] + [np.array([0x3FF0000000000000], np.uint64)])
    u = bits.view(np.float64)
    got, libm, cnt = lod5(probe, u, scale)
    assert cnt == 0
    ref = _ld(scale) * np.log10(_ld(u))
    one = u == 1.0
    assert np.all(got[one] == 0.0) and np.all(libm[one] == 0.0)
    rel = (np.abs(_ld(got) - ref) / np.abs(ref).clip(min=np.finfo(np.longdouble).tiny)).astype(np.float64)
    rel[one] = 0.0
    w, at = _worst(rel, u, f"fast_lod5 n={n}: relative error")
    _worst(_ulps(got, ref), u, f"fast_lod5 n={n}: ulps")
    assert w <= LOD_BOUND, (w, at)
    # the libm map: both are ~1 ulp from the truth, so the two differ by a few ulps
    d = np.abs(got - libm) / np.spacing(np.maximum(np.abs(got), np.abs(libm)))
    d[one] = 0.0
    dw, dat = _worst(d, u, f"fast_lod5 against scale * log10(u) n={n}: ulps")
    assert dw <= LIBM_ULPS, (dw, dat)


# ---- 2: u in (0, 2^-4), the specials ---------------------------------------------------------------------------------------------
def test_lod_out_of_range(probe):
    rng = np.random.default_rng(7)
    pts = []
    for e in range(-1074, -4):                       # every octave down to the smallest subnormal
        lo = np.ldexp(1.0, e)
        pts += [lo, np.nextafter(lo, 0.0), np.nextafter(lo, 1.0)]
        if e >= -1022:
            pts += list(np.ldexp(rng.uniform(1.0, 2.0, 24), e))
        else:
            pts += list(np.ldexp(np.floor(rng.uniform(1.0, 2.0, 4) * 2.0 ** (e + 1074)) / 2.0 ** (e + 1074), e))
    for k in range(1, 269):                          # the 2^-4k edges, where sh changes, +- 1 ulp
        x = np.ldexp(1.0, -4 * k)
        pts += [x, np.nextafter(x, 0.0), np.nextafter(x, 1.0)]
    pts += list(rng.uniform(0.0, 0.0625, 4096))
    u = np.array([x for x in pts if 0.0 < x < 0.0625])
    for n in (3, 2048):
        got, _, cnt = lod5(probe, u, -0.5 * n)
        assert cnt == 0
        ref = _ld(-0.5 * n) * np.log10(_ld(u))
        rel = (np.abs(_ld(got) - ref) / np.abs(ref)).astype(np.float64)
        w, at = _worst(rel, u, f"lod_out_of_range n={n}: relative error")
        _worst(_ulps(got, ref), u, f"lod_out_of_range n={n}: ulps")
        assert w <= LOD_BOUND, (w, at)
    sp = np.array([0.0, -0.0, -1e-300, -0.5, -1.0, -np.inf, np.nan, -5e-324])
    for counted in (True, False):
        got, _, cnt = lod5(probe, sp, -5.0, counted)
        assert np.all(got[:2] == np.inf)
        assert np.all(np.isnan(got[2:]))
        assert cnt == (6 if counted else 0)


# ---- 4: the table-driven logarithm of the h2 search ------------------------------------------------------------------------------
def test_fast_log_and_fast_lod(probe):
    rng = np.random.default_rng(11)
    exps = np.arange(-1022, 1024)
    xs = [np.ldexp(rng.uniform(1.0, 2.0, (exps.size, 16)), exps[:, None]).ravel(), np.ldexp(1.0, exps)]
    off = 0x3FE6000000000000
    edges = np.array([off + (i << 45) for i in range(129)], dtype=np.uint64).view(np.float64)
    xs += [edges, np.nextafter(edges, 0.0), np.nextafter(edges, 2.0), 0.5 * (edges[1:] + edges[:-1])]
    k = np.arange(1, 2001, dtype=np.float64)
    xs += [1.0 + k * 2.0 ** -52, 1.0 - k * 2.0 ** -53, 1.0 + 2.0 ** -np.arange(1, 53), 1.0 - 2.0 ** -np.arange(1, 54),
           [np.finfo(np.float64).tiny, np.finfo(np.float64).max]]
    x = np.concatenate([np.asarray(a, np.float64) for a in xs])
    scale = -1024.0
    ln, lg, lod = (np.empty_like(x) for _ in range(3))
    assert probe.probe_log(_p(x), _p(ln), _p(lg), _p(lod), x.size, scale) == 0
    lx = _ld(x)
    for got, ref, label, bound in ((ln, np.log(lx), "fast_log<false>", LOG_ULPS), (lg, np.log10(lx), "fast_log<true>", LOG_ULPS),
                                   (lod, _ld(scale) * np.log10(lx), "fast_lod", FAST_LOD_ULPS)):
        u = _ulps(got, ref)
        u[x == 1.0] = 0.0
        assert np.all(got[x == 1.0] == 0.0), label
        w, at = _worst(u, x, f"{label}: ulps")
        assert w <= bound, (label, w, at)


# ---- 5: reciprocals and reciprocal square roots ----------------------------------------------------------------------------------
def test_reciprocals(probe):
    rng = np.random.default_rng(5)
    exps = np.arange(-1022, 1022)
    m = np.concatenate([rng.uniform(1.0, 2.0, (exps.size, 24)), np.ones((exps.size, 1)),
                        np.full((exps.size, 1), np.nextafter(2.0, 0.0))], axis=1)
    x = np.ldexp(m, exps[:, None]).ravel()
    x = np.concatenate([x, -x])
    out = np.empty(4 * x.size)
    assert probe.probe_rcp(_p(x), _p(out), x.size) == 0
    out = out.reshape(-1, 4)
    rcp = _ld(1.0) / _ld(x)
    u = _ulps(out[:, 0], rcp)
    w, at = _worst(u, x, "fast_rcp: ulps")
    assert w <= 1.0, (w, at)
    rel = (np.abs(_ld(out[:, 1]) - rcp) / np.abs(rcp)).astype(np.float64)
    w, at = _worst(rel, x, "fast_rcp1: relative error")
    _worst(_ulps(out[:, 1], rcp), x, "fast_rcp1: ulps")
    assert w <= 2.2e-15, (w, at)
    pos = x > 0
    rs = _ld(1.0) / np.sqrt(_ld(x[pos]))
    for col, label in ((2, "nr_rsqrt"), (3, "fast_rsqrt")):
        w, at = _worst(_ulps(out[pos, col], rs), x[pos], f"{label}: ulps")
        assert w <= RSQRT_ULPS, (label, w, at)


# ---- 6: -log10 p, one degree of freedom --------------------------------------------------------------------------------------------
def _pv_ref(lod):
    mp.mp.dps = 40
    out = np.empty(lod.size)
    for i, v in enumerate(lod):
        if np.isnan(v):
            out[i] = np.nan
        elif v <= 0.0:
            out[i] = 0.0
        elif np.isinf(v):
            out[i] = np.inf
        else:
            x = mp.sqrt(mp.mpf(float(v)) * mp.log(10))
            if x < 1:      # through erf: erfc(x) = 1 - erf(x) rounds to 1 at 40 digits for x < 1e-40
                lnp = mp.log1p(-mp.erf(x))
            elif x < 1e100:
                lnp = mp.log(mp.erfc(x))
            else:          # mpmath's erfc overflows near x = 1e154; the asymptotic series, whose next term is ~x^-8
                lnp = -x * x - mp.log(x * mp.sqrt(mp.pi)) + mp.log1p(-1 / (2 * x * x) + 3 / (4 * x ** 4) - 15 / (8 * x ** 6))
            out[i] = float(-lnp / mp.log(10))
    return out


def _pv_inputs():
    d, tab = pval_table()
    rng = np.random.default_rng(1)
    xs = []
    for b in range(tab.shape[0]):
        lo, hi, _ = pv_bucket(b, d)
        xs += [lo, np.nextafter(hi, 0.0), np.nextafter(lo, 1e9)] + list(rng.uniform(lo, hi, 6))
    x = np.array([v for v in xs if v > 0.0])
    lod = x * x / LN10
    t0 = 1e-290 / LN10                                 # t = LOD ln 10 = 1e-290: the underflow cut
    x16 = 16384.0 ** 2 / LN10                          # x = 16384: the end of the table
    near = [np.nextafter(t0, 0.0), t0, np.nextafter(t0, 1.0), 1e-300, 1e-200, 1e-30,
            x16, np.nextafter(x16, 0.0), np.nextafter(x16, np.inf)] + [x16 * (1 + k * 1e-15) for k in range(-40, 41, 4)]
    far = [2e8, 1e9, 1e12, 1e20, 1e50, 1e100, 1e200, 1e300]
    return np.concatenate([lod, near, far, [0.0, -0.0, -1e-13, -5.0, np.nan, np.inf]])


def _check_pv(got, ref, lod, label):
    sp = ~np.isfinite(ref) | (lod <= 0.0)
    assert np.array_equal(np.isnan(got[sp]), np.isnan(ref[sp])) and np.all(got[sp & ~np.isnan(ref)] == ref[sp & ~np.isnan(ref)]), label
    assert np.all(np.signbit(got[lod == 0.0]) == False), label    # -0.0 -> +0
    fin = ~sp
    small = fin & (lod * LN10 < 1e-290)
    assert np.all(np.abs(got[small] - ref[small]) <= 1e-14), label     # the underflow floor: p = 1 - 1e-145 -> 0
    big = fin & ~small
    rel = np.abs(got[big] - ref[big]) / ref[big]
    w, at = _worst(rel, lod[big], f"{label}: relative error")
    assert w <= PV_BOUND, (label, w, at)


def test_fast_log10p1(probe, blmm):
    """fast_log10p1 through the probe and through lod2log10p(., 1)'s default (table) route; the pval_libm route on the same inputs:
    every bucket (edges and interior), bucket 0, both sides of t = 1e-290 and of x = 16384, far beyond, and the specials."""
    lod = _pv_inputs()
    ref = _pv_ref(lod)
    _check_pv(log10p1(probe, lod), ref, lod, "fast_log10p1 (probe)")
    _check_pv(blmm.lod2log10p(lod, 1), ref, lod, "lod2log10p df=1 (table route)")
    ctx = blmm.Context(0)
    try:
        ctx.set_tuning("pval_libm", 1)
        _check_pv(blmm.lod2log10p(lod, 1, ctx=ctx), ref, lod, "lod2log10p df=1 (pval_libm route)")
    finally:
        ctx.close()
    # the table route beyond LOD ~ 7.8e307, where t = LOD ln 10 overflows
    huge = np.array([1e308, np.finfo(np.float64).max])
    assert np.all(np.abs(log10p1(probe, huge) - _pv_ref(huge)) <= PV_BOUND * huge)


# ---- 7: general df ----------------------------------------------------------------------------------------------------------------
def _lnq_ref(a, z):
    """ln Q(a, z) at 50 digits with no term cap: log1p(-P) from the series below z = a + 1, Legendre's continued fraction above"""
    a, z = mp.mpf(a), mp.mpf(z)
    eps = mp.mpf(10) ** -48
    pre = -z + a * mp.log(z) - mp.loggamma(a)
    if z < a + 1:
        term = s = 1 / a
        k = 0
        while True:
            k += 1
            term *= z / (a + k)
            s += term
            if term < s * eps:
                break
        return mp.log1p(-mp.exp(pre + mp.log(s)))
    tiny = mp.mpf(10) ** -300
    b = z + 1 - a
    c, d = 1 / tiny, 1 / b
    h = d
    i = 0
    while True:
        i += 1
        an = -i * (i - a)
        b += 2
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1 / d
        de = d * c
        h *= de
        if abs(de - 1) < eps:
            break
    return pre + mp.log(h)


DFS = list(range(2, 13)) + [16, 31, 32, 33, 64, 100, 1000, 10 ** 4, 10 ** 5, 10 ** 6]


def _df_lods(df):
    a = 0.5 * df
    z = a * np.logspace(-3, 2, 31)
    z = np.concatenate([z, a + 1 + np.array([-3, -1, -0.5, -1e-3, -1e-9, 0.0, 1e-9, 1e-3, 0.5, 1, 3]) * max(1.0, np.sqrt(a) / 10)])
    z = np.concatenate([z, [800.0, 2000.0, 1e4] if a < 400 else []])       # p below 1e-300
    z = z[z > 0]
    return z / LN10


@pytest.mark.parametrize("df", DFS)
def test_general_df(blmm, df):
    """lod2log10p and blmm_lod2log10p_dev for chisq_df > 1 against an uncapped 50-digit restatement of ln Q(df/2, LOD ln 10),
    itself cross-checked with SciPy's gammaincc where Q is in [1e-300, 0.999]: z / a log-spaced over 1e-3 .. 1e2, dense around
    the series / fraction switch z = a + 1, out to p < 1e-300."""
    from common import DevBuf
    from scipy.special import gammaincc
    mp.mp.dps = 50
    a = 0.5 * df
    lod = _df_lods(df)
    z = lod * LN10
    lnq = [_lnq_ref(a, float(v)) for v in z]
    ref = np.array([float(-q / mp.log(10)) for q in lnq])
    q = gammaincc(a, z)
    chk = (q >= 1e-300) & (q <= 0.999)
    assert chk.sum() >= 3
    assert np.allclose(-np.log10(q[chk]), ref[chk], rtol=1e-8, atol=0), (df, np.max(np.abs(-np.log10(q[chk]) - ref[chk]) / ref[chk]))
    assert np.any(ref > 300)
    got = blmm.lod2log10p(lod, df)
    err = np.abs(got - ref) / (DF_RTOL * np.abs(ref) + DF_ATOL)
    w, at = _worst(err, lod, f"lod2log10p df={df}: error / (1e-10 |ref| + 1e-14)")
    k = int(np.argmax(err))
    print(f"  at z / a = {z[k] / a:.6g}: got {got[k]!r} ref {ref[k]!r}")
    assert w <= 1.0, (df, w, at)
    ctx = blmm.default_context()
    dL, dP = DevBuf(lod), DevBuf(np.full(lod.size, np.nan))
    try:
        ctx.check(ctx.lib.blmm_lod2log10p_dev(ctx.h, dL.ptr, lod.size, 1, lod.size, df, dP.ptr, lod.size))
        ctx.synchronize()
        assert np.array_equal(dP.get(lod.size), got)
    finally:
        dL.free()
        dP.free()


# ---- 9: the fp32 LOD map, every fp32 r^2 in [0, 1] ---------------------------------------------------------------------------------
def test_lod_f32_exhaustive(probe):
    """lod_f32 (k_scan_f32's epilogue) for all 1,065,353,217 fp32 r^2 in [0, 1], reduced on the device, against the fp64
    -n/(2 ln 10) log1p(-r^2): the fp32 contract of the permutation scans, 1e-3 |ref| + 1e-4, on every value."""
    n = 2048
    scale32 = np.float32(-0.5 * n / 2.302585092994046)
    count = 0x3F800000 + 1
    nb = 8192
    part = np.empty(4 * nb)
    cnt = np.zeros(1, np.int64)
    assert probe.probe_f32_scan(0, count, float(scale32), -0.5 * n / LN10, nb, _p(part), _p(cnt)) == 0
    part = part.reshape(nb, 4)
    assert cnt[0] == 0
    k = int(np.argmax(part[:, 0]))
    r2 = np.array([int(part[k, 1])], np.uint32).view(np.float32)[0]
    print(f"lod_f32: worst error / (1e-3 |ref| + 1e-4) {part[k, 0]:.4g} at r^2 = {float(r2)!r}")
    assert part[k, 0] <= 1.0
    k = int(np.argmax(part[:, 2]))
    r2 = np.array([int(part[k, 3])], np.uint32).view(np.float32)[0]
    print(f"lod_f32: worst relative error where LOD >= 1: {part[k, 2]:.4g} at r^2 = {float(r2)!r}")
    # r^2 > 1 and NaN: NaN, counted once each (r^2 = 1 -> +Inf is inside the scan above: its ratio is 0 only if got == ref == +Inf)
    nan_from = 0x3F800001
    part2 = np.empty(4)
    assert probe.probe_f32_scan(nan_from, 5, float(scale32), -0.5 * n / LN10, 1, _p(part2), _p(cnt)) == 0
    assert cnt[0] == 5
    assert probe.probe_f32_scan(0x7FC00000, 3, float(scale32), -0.5 * n / LN10, 1, _p(part2), _p(cnt)) == 0
    assert cnt[0] == 3


# ---- 10: table staging -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [64, 128, 256, 512, 1024])
def test_table_staging(probe, nt):
    """lod_stage_load/store<NT> and pv_stage_load/store<NT> fill LDS bit for bit with {invc, scale * log10 c} and the p-value table,
    the clamped tail included, and write nothing past either table."""
    _, _, lodtab = log_tables()
    _, pvtab = pval_table()
    scale, fill = -0.5 * 79, -12345.678
    pad = C.c_int(0)
    lod_out = np.empty((2049 + 64) * 2)
    pv_out = np.empty((1045 + 64) * 2)
    assert probe.probe_stage(nt, scale, fill, _p(lod_out), _p(pv_out), C.byref(pad)) == 0
    assert pad.value == 64
    lod_out = lod_out.reshape(-1, 2)
    want = np.stack([lodtab[:, 0], scale * lodtab[:, 1]], axis=1)
    assert np.array_equal(lod_out[:2049].view(np.uint64), want.view(np.uint64))
    assert np.all(lod_out[2049:] == fill)
    pv = pv_out.reshape(-1, 2)
    assert np.array_equal(pv[:1045].view(np.uint64), pvtab.reshape(-1, 2).view(np.uint64))
    assert np.all(pv[1045:] == fill)
