"""The consumers of a LOD matrix -- column maxima, the LOD > t filter, the permutation quantiles, the -log10 p column pass and the
column gather -- against the plain references of tests/consumers_ref.py, at the shapes where their indexing changes: the
grid-stride loops over traits (4096 columns for the filter and the general -log10 p pass, 64 for the one-degree-of-freedom pass),
the 16384-row stride and the 32768-column launch chunks of the gather, the switch of the sort at 16384 values, leading dimensions
above p in every device-pointer form, ties across lanes, and columns / thresholds of NaN, +-inf and +-0.0.  Half the suite
compares other features with these calls bit for bit; this module is what those comparisons stand on.

Every padded input (ld > p) carries poison in its padding rows -- NaN for the -log10 p pass and for half the quantile cases, a
huge finite value above every threshold elsewhere -- and every device output is prefilled with a sentinel that has to survive
outside the entries the call owns.

The bound of the quantile tests.  For finite neighbouring order statistics a <= b the kernel evaluates a + g (b - a) in binary64
(eps = 2^-53, the unit roundoff), with h = (count - 1) q rounded once and g = h - floor(h) exact (h < 2^53 and floor(h) share h's
binade or a lower one, so the difference is representable):
  * fl(h) = h (1 + d0), |d0| <= eps: g is off by at most eps h <= (count - 1) eps, the result by (count - 1) eps |b - a|.  Rounding
    is monotone, so fl(h) never crosses an integer, it can only land on one from below: the kernel then returns b where the exact
    value is b - (1 - g)(b - a) with 1 - g <= (count - 1) eps -- inside the same term;
  * fl(b - a) = (b - a)(1 + d1) and the product g fl(b - a) rounds once more (d2): with g < 1 together at most 2 eps |b - a| to
    first order, which the (count + 2) below covers with a whole eps |b - a| to spare for the second-order terms;
  * the final sum rounds once: eps |result| <= eps max(|a|, |b|); a second eps max(|a|, |b|) is granted for the reference's own
    conversion of the returned double and so that a contracted multiply-add (one rounding fewer) and a separate one both fit.
Hence |got - exact| <= (count + 2) eps |b - a| + 2 eps max(|a|, |b|), against the exact rational value.  Where a neighbour is
infinite nothing is rounded: the result must equal the reference's, and no result may be NaN.  The largest observed ratio of
error to bound is printed by the quantile test (run with -s)."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from common import DevBuf, make_data
from consumers_ref import colmax_ref, colmax_ref_fast, quantile7_bound, quantile7_ref, threshold_ref

pytestmark = pytest.mark.gpu

INF, NAN = math.inf, math.nan
HUGE = 1e300          # poison above every threshold used here
SENT = -777.0         # sentinel of the double outputs
ISENT = -7            # sentinel of the integer outputs


@pytest.fixture(scope="module")
def ctx(blmm):
    c = blmm.Context(0)
    yield c
    c.close()


def vp(b):
    return None if b is None else C.c_void_p(b.ptr)


def hp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def padded(L, ld, poison):
    """The p x m matrix L as the column-major storage of leading dimension ld, the rows p .. ld - 1 of every column = poison."""
    p, m = L.shape
    buf = np.full((ld, m), poison, dtype=np.float64, order="F")
    buf[:p, :] = L
    return buf.ravel("F")


def flat(L):
    return np.asfortranarray(L, dtype=np.float64).ravel("F")


# ---- column maxima -------------------------------------------------------------------------------------------------------------
NKINDS = 12


def colmax_column(kind, p, rng):
    """One column of length p of the given kind (the kinds are listed in test_colmax)."""
    base = rng.standard_normal(p) * 3.0
    neg = -np.abs(base) - 0.5
    # rows i < i2 with i mod 64 > i2 mod 64 (the lower marker in the higher lane); rows i, i + 64 (one lane)
    k = max(0, (p - 65) // 64 // 2)
    cross = (64 * k + 63, min(64 * (k + 1) + 5, p - 1)) if p >= 65 else (0, p - 1)
    lane = (64 * k + 7, 64 * k + 71) if p > 64 * k + 71 else ((0, 64) if p >= 65 else (0, p - 1))
    if kind == 0:
        return base
    if kind == 1:
        return neg
    if kind == 2:
        base[rng.random(p) < 0.2] = NAN
        return base
    if kind == 3:
        return np.full(p, NAN)
    if kind == 4:
        return np.full(p, -INF)
    if kind == 5:
        base[p // 3] = INF
        return base
    if kind == 6:
        base[cross[0]] = base[cross[1]] = INF
        return base
    if kind == 7:
        base[cross[0]] = base[cross[1]] = np.abs(base).max() + 1.0
        return base
    if kind == 8:
        base[lane[0]] = base[lane[1]] = np.abs(base).max() + 1.0
        return base
    if kind == 9:
        neg[cross[1]] = 0.0
        neg[cross[0]] = -0.0                    # written second: at p = 1 the column is the single -0.0
        return neg
    if kind == 10:
        base[p - 1] = np.abs(base).max() + 1.0
        return base
    return (rng.random(p) - 0.5) * 1e-309       # denormals of both signs


def colmax_matrix(p, m, offset, seed):
    rng = np.random.default_rng(seed)
    return np.column_stack([colmax_column((j + offset) % NKINDS, p, rng) for j in range(m)])


# the offsets walk the twelve kinds so that m = 1, 3, 4, 5 together hold every kind once at each p (and m = 9 nine of them again)
COLMAX_CASES = [(p, m, off) for p in (1, 63, 64, 65, 127, 128, 129, 1003, 70001)
                for m, off in ((1, 0), (3, 1), (4, 4), (5, 8), (9, 1))] + [(70, 4099, 0)]


@pytest.mark.parametrize("p,m,off", COLMAX_CASES)
def test_colmax(ctx, p, m, off):
    """blmm_lod_colmax, blmm_lod_colmax_dev (ldL = p and p + 3) and blmm_last_lod_colmax equal colmax_ref exactly.  Columns by
    turns: random; all negative; NaN scattered; all NaN; all -inf; one +Inf; two +Inf; the maximum twice with the lower marker in
    the higher lane; the maximum twice in one lane (rows i, i + 64); -0.0 before +0.0 in a negative column; the maximum in the
    last row; denormals.  argmax_out == NULL is accepted by every form."""
    L = colmax_matrix(p, m, off, 1000 * p + m)
    rmx, rarg = colmax_ref(L)
    lib = ctx.lib

    def check(mx, arg, what):
        assert not np.isnan(mx).any(), what
        assert np.array_equal(mx, rmx), (what, np.flatnonzero(mx != rmx)[:5], mx[mx != rmx][:5], rmx[mx != rmx][:5])
        if arg is not None:
            assert np.array_equal(arg, rarg), (what, np.flatnonzero(arg != rarg)[:5], arg[arg != rarg][:5], rarg[arg != rarg][:5])

    host = flat(L)
    mx, arg = np.full(m, SENT), np.full(m, ISENT, dtype=np.int64)
    ctx.check(lib.blmm_lod_colmax(ctx.h, hp(host), p, m, hp(mx), hp(arg)))
    check(mx, arg, "host")
    mx2 = np.full(m, SENT)
    ctx.check(lib.blmm_lod_colmax(ctx.h, hp(host), p, m, hp(mx2), None))
    check(mx2, None, "host, no argmax")
    # the host form's upload is the resident matrix now
    mx, arg = np.full(m, SENT), np.full(m, ISENT, dtype=np.int64)
    ctx.check(lib.blmm_last_lod_colmax(ctx.h, hp(mx), hp(arg)))
    check(mx, arg, "last")
    mx2 = np.full(m, SENT)
    ctx.check(lib.blmm_last_lod_colmax(ctx.h, hp(mx2), None))
    check(mx2, None, "last, no argmax")

    for ld in (p, p + 3):
        dL = DevBuf(padded(L, ld, 1e308))
        dmx, dax = DevBuf(np.full(m + 2, SENT)), DevBuf(np.full(m + 2, ISENT, dtype=np.int64))
        ctx.check(lib.blmm_lod_colmax_dev(ctx.h, vp(dL), p, m, ld, vp(dmx), vp(dax)))
        ctx.synchronize()
        gm, ga = dmx.get(m + 2), dax.get(m + 2, np.int64)
        check(gm[:m], ga[:m], f"dev ld={ld}")
        assert np.all(gm[m:] == SENT) and np.all(ga[m:] == ISENT), f"dev ld={ld}: wrote past m"
        dmx.fill(np.full(m + 2, SENT))
        ctx.check(lib.blmm_lod_colmax_dev(ctx.h, vp(dL), p, m, ld, vp(dmx), None))
        ctx.synchronize()
        gm = dmx.get(m + 2)
        check(gm[:m], None, f"dev ld={ld}, no argmax")
        assert np.all(gm[m:] == SENT)
        for b in (dL, dmx, dax):
            b.free()


# ---- threshold filter ----------------------------------------------------------------------------------------------------------
def threshold_matrix(p, m, seed):
    """Values on a grid of 0.1 (every value occurs many times), with NaN, +Inf and -inf scattered."""
    rng = np.random.default_rng(seed)
    L = np.round(rng.standard_normal((p, m)) * 2.0, 1)
    if p * m >= 16:
        u = rng.random((p, m))
        L[u < 0.01] = NAN
        L[(u >= 0.01) & (u < 0.02)] = INF
        L[(u >= 0.02) & (u < 0.03)] = -INF
    return L


class Triplets:
    """Host or device room for `cap` triplets and the count, prefilled with sentinels, `extra` slots beyond cap."""

    def __init__(self, cap, dev, extra=4):
        self.cap, self.dev, self.n = cap, dev, cap + extra
        i, j, l = np.full(self.n, ISENT, dtype=np.int32), np.full(self.n, ISENT, dtype=np.int32), np.full(self.n, SENT)
        if dev:
            self.i, self.j, self.l, self.c = DevBuf(i), DevBuf(j), DevBuf(l), DevBuf(np.full(1, ISENT, dtype=np.int64))
        else:
            self.i, self.j, self.l, self.c = i, j, l, C.c_int64(ISENT)

    def args(self):
        if self.dev:
            return vp(self.i), vp(self.j), vp(self.l), vp(self.c)
        return hp(self.i), hp(self.j), hp(self.l), C.byref(self.c)

    def result(self):
        if self.dev:
            out = (int(self.c.get(1, np.int64)[0]), self.i.get(self.n, np.int32), self.j.get(self.n, np.int32), self.l.get(self.n))
            for b in (self.i, self.j, self.l, self.c):
                b.free()
            return out
        return int(self.c.value), self.i, self.j, self.l


def run_threshold(ctx, form, L, thr, cap, ld=None, dL=None):
    """(count, i, j, lod) of one form with room for cap triplets (+ sentinel slots); cap = None: NULL triplet pointers, cap 0."""
    p, m = L.shape
    lib = ctx.lib
    t = Triplets(cap or 0, form == "dev")
    ai, aj, al, ac = t.args()
    if cap is None:
        ai = aj = al = None
    ncap = cap or 0
    if form == "host":
        ctx.check(lib.blmm_lod_threshold(ctx.h, hp(flat(L)), p, m, thr, ncap, ai, aj, al, ac))
    elif form == "last":               # the resident matrix: whatever the last host-form upload left
        ctx.check(lib.blmm_last_lod_threshold(ctx.h, thr, ncap, ai, aj, al, ac))
    else:
        ctx.check(lib.blmm_lod_threshold_dev(ctx.h, vp(dL), p, m, ld, thr, ncap, ai, aj, al, ac))
        ctx.synchronize()
    return t.result()


def check_full(res, ref, cap, what):
    """All of the reference set stored (count <= cap), nothing beyond it touched."""
    cnt, ii, jj, ll = res
    ri, rj, rl = ref
    assert cnt == len(ri), (what, cnt, len(ri))
    assert cnt <= cap
    order = np.lexsort((ii[:cnt], jj[:cnt]))
    assert np.array_equal(ii[:cnt][order], ri) and np.array_equal(jj[:cnt][order], rj), what
    assert np.array_equal(ll[:cnt][order], rl), what                   # no NaN passes: == compares everything, +Inf included
    assert np.all(ii[cnt:] == ISENT) and np.all(jj[cnt:] == ISENT) and np.all(ll[cnt:] == SENT), (what, "wrote beyond count")


def each_form(ctx, L, pad=5):
    """(name, runner(thr, cap)) of the host form, the last form on its upload, and the device form at ldL = p and p + pad with
    the padding above every threshold."""
    p, m = L.shape
    yield "host", lambda thr, cap: run_threshold(ctx, "host", L, thr, cap)
    yield "last", lambda thr, cap: run_threshold(ctx, "last", L, thr, cap)
    for ld in (p, p + pad):
        dL = DevBuf(padded(L, ld, HUGE))
        yield f"dev ld={ld}", lambda thr, cap, ld=ld, dL=dL: run_threshold(ctx, "dev", L, thr, cap, ld, dL)
        dL.free()


@pytest.mark.parametrize("p,m", [(300, 4100), (70001, 3), (257, 65), (1, 1)])
def test_threshold_filter(ctx, p, m):
    """*count and the stored triplets, sorted by (trait, marker), equal threshold_ref for a thr that occurs in the matrix (the
    comparison is strict), thr = -inf (everything finite and +Inf, but neither -inf nor NaN), +inf and NaN (nothing); a cap below
    the count stores exactly cap distinct members of the set; cap = 0 with NULL pointers returns the count."""
    L = threshold_matrix(p, m, 31 * p + m)
    vals = L[np.isfinite(L)]
    occurs = float(np.sort(vals)[(3 * vals.size) // 4])               # a value of the matrix, many times over at the larger shapes
    assert (L == occurs).sum() >= 1
    refs = {thr: threshold_ref(L, thr) for thr in (occurs, -INF, INF, NAN)}
    assert len(refs[INF][0]) == 0 and len(refs[NAN][0]) == 0
    assert len(refs[-INF][0]) == int((np.isfinite(L) | (L == INF)).sum())
    if p * m > 1:
        assert 0 < len(refs[occurs][0]) < len(refs[-INF][0])
    room = p * m + 3
    for name, run in each_form(ctx, L):
        for thr, ref in refs.items():
            check_full(run(thr, room), ref, room, (name, thr))
            res = run(thr, None)                                       # cap = 0, NULL pointers
            assert res[0] == len(ref[0]), (name, thr, "cap = 0")
        ri, rj, rl = refs[occurs]
        if len(ri) >= 4:
            cap = len(ri) // 3
            cnt, ii, jj, ll = run(occurs, cap)
            assert cnt == len(ri), (name, "count with a small cap")
            assert np.all(ii[cap:] == ISENT) and np.all(jj[cap:] == ISENT) and np.all(ll[cap:] == SENT), (name, "wrote beyond cap")
            key = jj[:cap].astype(np.int64) * p + ii[:cap]
            assert np.all((ii[:cap] >= 0) & (ii[:cap] < p) & (jj[:cap] >= 0) & (jj[:cap] < m)), name
            assert np.unique(key).size == cap, (name, "stored triplets repeat")
            assert np.all(np.isin(key, rj.astype(np.int64) * p + ri)), (name, "a stored triplet is not in the set")
            assert np.array_equal(ll[:cap], L[ii[:cap], jj[:cap]]), (name, "a stored triplet carries another entry's LOD")


def test_threshold_filter_dense(ctx):
    """Every entry of a 1000 x 1000 matrix passes: the count is 10^6 exactly (every wave-aggregated reservation counted once),
    the stored set is the whole matrix, and a small cap stores exactly cap distinct entries."""
    rng = np.random.default_rng(99)
    L = rng.random((1000, 1000)) + 1.0
    ref = threshold_ref(L, 0.5)
    assert len(ref[0]) == 10 ** 6
    for name, run in each_form(ctx, L):
        res = run(0.5, 10 ** 6)
        assert res[0] == 10 ** 6, name
        check_full(res, ref, 10 ** 6, name)
        cnt, ii, jj, ll = run(0.5, 12345)
        assert cnt == 10 ** 6, name
        assert np.all(ii[12345:] == ISENT) and np.all(ll[12345:] == SENT), name
        assert np.unique(jj[:12345].astype(np.int64) * 1000 + ii[:12345]).size == 12345, name
        assert np.array_equal(ll[:12345], L[ii[:12345], jj[:12345]]), name
        assert run(0.5, None)[0] == 10 ** 6, name


# ---- quantiles -----------------------------------------------------------------------------------------------------------------
NPERMS = [1, 2, 3, 64, 101, 1000, 4095, 4096, 4097, 16383, 16384, 16385, 20000, 32768, 65537]
VECTORS = ["random", "ascending", "descending", "equal", "ten", "pinf", "ninf", "all_ninf"]
_worst = {"ratio": 0.0, "at": None}


def maxima_vector(kind, n, rng):
    if kind == "random":
        return rng.random(n) * 6.0
    if kind == "ascending":
        return np.sort(rng.random(n) * 6.0)
    if kind == "descending":
        return np.sort(rng.random(n) * 6.0)[::-1].copy()
    if kind == "equal":
        return np.full(n, 3.25)
    if kind == "ten":
        return rng.permutation(np.resize(rng.random(10) * 6.0, n))
    v = rng.random(n) * 6.0
    k = max(1, n // 100)
    if kind == "pinf":
        v[rng.choice(n, k, replace=False)] = INF
    elif kind == "ninf":
        v[rng.choice(n, k, replace=False)] = -INF
    else:
        v[:] = -INF
    return v


def perms_matrix(v, p, rng):
    """A p x n matrix whose column maxima are v: column k holds v[k] in one row and smaller values elsewhere.  A maximum of -inf is
    a column of NaN (no comparable entry), or, every second time, a column of -inf."""
    n = v.shape[0]
    top = np.where(np.isfinite(v), v, 0.0)
    L = top[None, :] - 0.5 - rng.random((p, n)) * 3.0
    L[rng.integers(0, p, n), np.arange(n)] = v
    none = np.flatnonzero(v == -INF)
    L[:, none[0::2]] = NAN
    L[:, none[1::2]] = -INF
    return L


def prob_sets(n, rng):
    """The 64-level maximum (two sets of it), one level, 0 and 1, levels outside [0, 1], and -- n = 101 -- the levels k / 100,
    for which (count - 1) q is an integer in exact arithmetic."""
    sets = [np.concatenate([[0.9, 0.95, 0.99, 0.5], rng.random(60)]),
            np.concatenate([np.linspace(0.0, 1.0, 33), 1.0 - 2.0 ** -np.arange(1, 32)]),
            np.array([0.95]), np.array([0.0, 1.0]), np.array([-0.25, 1.5, -INF, INF, -1e-300, 1.0 + 2.0 ** -52])]
    if n == 101:
        sets += [np.arange(0, 64) / 100.0, np.arange(64, 101) / 100.0]
    return [np.ascontiguousarray(s, dtype=np.float64) for s in sets]


def check_quantiles(got, vs, probs, what):
    assert not np.isnan(got).any(), (what, "NaN threshold", probs[np.isnan(got)][:5])
    for g, q in zip(got.tolist(), probs.tolist()):
        exact, bound = quantile7_ref(vs, q), quantile7_bound(vs, q)
        if not isinstance(exact, Fraction):
            assert g == exact, (what, q, g, exact)                     # an infinite threshold: exactly that infinity
        elif bound is None:
            assert g == float(exact), (what, q, g, float(exact))       # an order statistic beside an infinite neighbour
        else:
            err = abs(Fraction(g) - exact)
            if bound > 0 and float(err / bound) > _worst["ratio"]:
                _worst["ratio"], _worst["at"] = float(err / bound), (what, q)
            assert err <= bound, (what, q, g, float(exact), float(err), float(bound))


@pytest.mark.parametrize("p", [1, 37])
@pytest.mark.parametrize("nperms", NPERMS)
def test_quantiles(ctx, nperms, p):
    """blmm_get_thresholds, blmm_get_thresholds_dev at ld = p + 2 and blmm_last_get_thresholds against the exact type-7 quantile of
    colmax_ref's maxima: inside the derived bound for finite neighbours, exactly the reference's value beside an infinity, never
    NaN.  nperms walks the switch of the sort at 16384 values (one workgroup in LDS below, one launch per step above) and the
    LDS opt-in above 48 KiB (from 8192 values on)."""
    lib = ctx.lib
    for vi, kind in enumerate(VECTORS):
        rng = np.random.default_rng([nperms, p, vi])
        v = maxima_vector(kind, nperms, rng)
        L = perms_matrix(v, p, rng)
        rmx, _ = colmax_ref_fast(L)
        assert np.array_equal(rmx, v)                                  # the matrix holds the maxima it was built for
        vs = np.sort(rmx)
        host = flat(L)
        ld = p + 2
        dL = DevBuf(padded(L, ld, NAN if p == 1 else 1e308))
        mx = np.empty(nperms)
        for probs in prob_sets(nperms, rng):
            k = probs.shape[0]
            out = np.full(k + 1, SENT)
            ctx.check(lib.blmm_get_thresholds(ctx.h, hp(host), p, nperms, hp(probs), k, hp(out)))
            assert out[k] == SENT
            check_quantiles(out[:k], vs, probs, (kind, "host"))
            out_dev = np.full(k + 1, SENT)
            ctx.check(lib.blmm_get_thresholds_dev(ctx.h, vp(dL), p, nperms, ld, hp(probs), k, hp(out_dev)))
            assert out_dev[k] == SENT
            check_quantiles(out_dev[:k], vs, probs, (kind, "dev"))
            assert np.array_equal(out[:k], out_dev[:k]), (kind, "host and dev forms differ")
        # the resident form: the upload of blmm_lod_colmax, whose maxima are the sorted vector's
        ctx.check(lib.blmm_lod_colmax(ctx.h, hp(host), p, nperms, hp(mx), None))
        assert np.array_equal(mx, rmx), kind
        for probs in prob_sets(nperms, rng)[:2]:
            k = probs.shape[0]
            out = np.full(k + 1, SENT)
            ctx.check(lib.blmm_last_get_thresholds(ctx.h, hp(probs), k, hp(out)))
            assert out[k] == SENT
            check_quantiles(out[:k], vs, probs, (kind, "last"))
        dL.free()
    print(f"\nquantiles nperms={nperms} p={p}: largest error / bound so far {_worst['ratio']:.4f} at {_worst['at']}")


def test_quantiles_opposite_infinities(ctx):
    """-inf beside +inf: the limit of (2 g - 1) M -- -inf below g = 1/2, +inf above it, 0 at it; never NaN."""
    L = np.array([[NAN, INF, NAN, INF]])                               # maxima -inf, +inf, -inf, +inf
    probs = np.array([0.0, 1.0 / 3.0, 0.4, 0.5, 0.6, 2.0 / 3.0, 1.0])  # h = 3 q: between ranks 1 and 2 from 1/3 to 2/3
    out = np.full(probs.shape[0], SENT)
    ctx.check(ctx.lib.blmm_get_thresholds(ctx.h, hp(flat(L)), 1, 4, hp(probs), probs.shape[0], hp(out)))
    vs = np.sort(colmax_ref(L)[0])
    assert vs.tolist() == [-INF, -INF, INF, INF]
    check_quantiles(out, vs, probs, "opposite infinities")
    assert out.tolist() == [-INF, -INF, -INF, 0.0, INF, INF, INF]


# ---- -log10 p: indexing ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("df,m", [(1, 1), (1, 63), (1, 64), (1, 65), (1, 200), (3, 5), (3, 4097)])
@pytest.mark.parametrize("p", [1, 255, 256, 257])
def test_log10p_indexing(ctx, df, m, p):
    """blmm_lod2log10p_dev at ldL = p + 1, ldP = p + 2 and blmm_last_log10p: every entry is bit-equal to what the same call gives
    for that LOD when all p m values stand in ONE column (no trait index, no leading dimension: the values' accuracy is the
    subject of test_gpu_fastmath.py); NaN and +Inf keep their place; the output's padding keeps its sentinel."""
    lib = ctx.lib
    rng = np.random.default_rng([df, m, p])
    L = rng.random((p, m)) * 10.0 ** rng.integers(-3, 3, size=(p, m))
    u = rng.random((p, m))
    L[u < 0.03] = NAN
    L[(u >= 0.03) & (u < 0.06)] = INF
    L[(u >= 0.06) & (u < 0.08)] = 0.0
    n = p * m
    d1, dP1 = DevBuf(flat(L)), DevBuf(np.full(n, SENT))
    ctx.check(lib.blmm_lod2log10p_dev(ctx.h, vp(d1), n, 1, n, df, vp(dP1), n))
    ctx.synchronize()
    ref = dP1.get(n).reshape((m, p)).T
    assert np.array_equal(np.isnan(ref), np.isnan(L)) and np.array_equal(ref == INF, L == INF)
    assert np.all(ref[np.isfinite(L)] >= 0.0) and np.all(ref[L == 0.0] == 0.0) and np.all(ref[np.isfinite(L) & (L > 0)] > 0.0)

    ldL, ldP = p + 1, p + 2
    dL, dP = DevBuf(padded(L, ldL, NAN)), DevBuf(np.full(ldP * m, SENT))
    ctx.check(lib.blmm_lod2log10p_dev(ctx.h, vp(dL), p, m, ldL, df, vp(dP), ldP))
    ctx.synchronize()
    got = dP.get((m, ldP)).T
    same = (got[:p] == ref) | (np.isnan(got[:p]) & np.isnan(ref))
    assert same.all(), (np.argwhere(~same)[:5], got[:p][~same][:5], ref[~same][:5])
    assert np.array_equal(np.signbit(got[:p]), np.signbit(ref))
    assert np.array_equal(np.isnan(got[:p]), np.isnan(L)) and np.array_equal(got[:p] == INF, L == INF)
    assert np.all(got[p:] == SENT), "the output's padding rows were written"

    mx = np.empty(m)
    ctx.check(lib.blmm_lod_colmax(ctx.h, hp(flat(L)), p, m, hp(mx), None))      # leaves L resident
    out = np.full(n + 2, SENT)
    ctx.check(lib.blmm_last_log10p(ctx.h, df, hp(out)))
    assert np.array_equal(out[:n].reshape((m, p)).T, ref, equal_nan=True)
    assert np.all(out[n:] == SENT)
    for b in (d1, dP1, dL, dP):
        b.free()


# ---- column gather ---------------------------------------------------------------------------------------------------------------
def resident(ctx, L):
    p, m = L.shape
    mx = np.empty(m)
    ctx.check(ctx.lib.blmm_lod_colmax(ctx.h, hp(flat(L)), p, m, hp(mx), None))
    pp, mm = C.c_int64(0), C.c_int64(0)
    assert ctx.lib.blmm_last_dims(ctx.h, C.byref(pp), C.byref(mm)) == 0 and (pp.value, mm.value) == (p, m)


def gather(ctx, p, cols, sentinel_tail=3):
    cols = np.ascontiguousarray(cols, dtype=np.int64)
    out = np.full(p * cols.shape[0] + sentinel_tail, SENT)
    ctx.check(ctx.lib.blmm_last_lod_columns(ctx.h, hp(cols), cols.shape[0], hp(out)))
    assert np.all(out[p * cols.shape[0]:] == SENT)
    return out[:p * cols.shape[0]].reshape((cols.shape[0], p)).T


def test_column_gather(ctx, blmm):
    """blmm_last_lod_columns: 40000 columns of a 5 x 7 matrix in arbitrary order with repeats (two launch chunks of 32768), three
    of a 20000 x 3 matrix (rows beyond the 16384 of one sweep of the launch), none at all; an index of m or of -1 is refused with
    the documented message before anything is written."""
    rng = np.random.default_rng(5)
    L = rng.standard_normal((5, 7))
    L[2, 3], L[4, 6] = NAN, INF
    resident(ctx, L)
    cols = rng.integers(0, 7, 40000)
    cols[32766:32770] = [6, 0, 6, 5]
    assert np.array_equal(gather(ctx, 5, cols), L[:, cols], equal_nan=True)
    assert gather(ctx, 5, np.empty(0, dtype=np.int64)).shape == (5, 0)
    ctx.check(ctx.lib.blmm_last_lod_columns(ctx.h, None, 0, None))
    for bad in (7, -1):
        for where in (0, 39999):
            c = cols.copy()
            c[where] = bad
            out = np.full(5 * 40000, SENT)
            with pytest.raises(blmm.BulkLMMError, match="last_lod_columns: column index out of range"):
                ctx.check(ctx.lib.blmm_last_lod_columns(ctx.h, hp(c), 40000, hp(out)))
            assert np.all(out == SENT), "a refused call wrote"
    L = rng.standard_normal((20000, 3))
    L[16383:16386, 2] = [NAN, INF, -INF]
    resident(ctx, L)
    assert np.array_equal(gather(ctx, 20000, [2, 0, 2]), L[:, [2, 0, 2]], equal_nan=True)
    assert np.array_equal(gather(ctx, 20000, [1]), L[:, [1]])


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_last_reductions_after_a_resident_bulkscan(ctx, blmm):
    """blmm_bulkscan with L_out == NULL: the three blmm_last_* reductions equal the references applied to the matrix that
    blmm_last_lod_columns hands out."""
    Y, G, K, _ = make_data(p=1500, m=70, seed=606)
    r = blmm.bulkscan(Y, G, K, method="null-grid", h2_grid=[i / 10.0 for i in range(10)], ctx=ctx, keep_on_device=True)
    h = r["L"]
    assert h.shape == (1500, 70)
    L = h.to_host()
    assert L.shape == (1500, 70) and np.isfinite(L).all() and L.max() > 3.0
    mx, arg = h.colmax()
    rmx, rarg = colmax_ref(L)
    assert np.array_equal(mx, rmx) and np.array_equal(arg, rarg)
    thr = float(np.sort(L, axis=None)[-500])                           # a value of the matrix: 499 or fewer lie above it
    ii, jj, ll = h.threshold(thr, cap=1 << 12)
    ri, rj, rl = threshold_ref(L, thr)
    assert 0 < len(ri) < 500
    assert np.array_equal(ii, ri) and np.array_equal(jj, rj) and np.array_equal(ll, rl)
    probs = np.concatenate([[0.0, 1.0, 0.5, 0.9, 0.95], np.random.default_rng(1).random(20)])
    check_quantiles(h.get_thresholds(probs), np.sort(rmx), probs, "resident bulkscan")
