"""Plain references for the consumers of a LOD matrix (column maxima, the LOD > t filter, the permutation quantiles): NumPy and
`fractions.Fraction` only, no call into the library, so that tests/test_gpu_consumers.py has something outside the library to
stand on.  tests/test_consumers_ref.py checks these references themselves on a CPU."""
import math
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -53   # unit roundoff of binary64


def colmax_ref(L):
    """(max, argmax) per column of the p x m matrix L: the maximum over the entries that are not NaN and the LOWEST row that
    holds it (compared with ==, so +0.0 and -0.0 are one value and the first of them wins); (-inf, -1) when no entry compares
    greater than -inf -- an empty column, a column of NaN, a column of -inf."""
    L = np.asarray(L, dtype=np.float64)
    p, m = L.shape
    mx = np.full(m, -np.inf)
    arg = np.full(m, -1, dtype=np.int64)
    for j in range(m):
        best, bi = -math.inf, -1
        for i, v in enumerate(L[:, j].tolist()):
            if v > best:                      # False for NaN and for a repeat of the maximum: the lowest row stays
                best, bi = v, i
        mx[j], arg[j] = best, bi
    return mx, arg


def colmax_ref_fast(L):
    """colmax_ref with NumPy's column operations, for the long columns (tests/test_consumers_ref.py holds the two together)."""
    L = np.asarray(L, dtype=np.float64)
    p, m = L.shape
    if p == 0:
        return np.full(m, -np.inf), np.full(m, -1, dtype=np.int64)
    W = np.where(np.isnan(L), -np.inf, L)
    mx = W.max(axis=0)
    arg = np.argmax(W == mx[None, :], axis=0).astype(np.int64)     # the first row equal to the maximum (0.0 == -0.0)
    arg[mx == -np.inf] = -1
    mx = W[np.maximum(arg, 0), np.arange(m)]                        # the sign of a zero maximum: that of its lowest row
    mx[arg < 0] = -np.inf
    return mx, arg


def threshold_ref(L, thr):
    """The set {(i, j, L[i, j]) : L[i, j] > thr} under IEEE > (a NaN entry never passes, a NaN thr passes nothing), as arrays
    (i, j, lod) sorted by (trait j, marker i)."""
    L = np.asarray(L, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        hit = np.argwhere(L.T > thr)          # rows of (j, i), sorted by j then i
    jj, ii = hit[:, 0].astype(np.int32), hit[:, 1].astype(np.int32)
    return ii, jj, L[ii, jj]


def quantile7_neighbours(values, q):
    """(a, b, g, count): the order statistics a <= b around the type-7 quantile of `values` at level q (clamped to [0, 1]) and
    the exact fraction g = h - floor(h), h = (count - 1) q, as a Fraction.  NaN sorts last."""
    v = np.sort(np.asarray(values, dtype=np.float64))      # NumPy sorts NaN last, -inf first, +inf before NaN
    n = int(v.shape[0])
    assert n >= 1 and not math.isnan(q)
    qq = Fraction(0) if q < 0 else (Fraction(1) if q > 1 else Fraction(float(q)))     # +-inf clamp too
    h = (n - 1) * qq
    lo = h.numerator // h.denominator
    hi = min(lo + 1, n - 1)
    return float(v[lo]), float(v[hi]), h - lo, n


def quantile7_ref(values, q):
    """The exact type-7 quantile (Julia's and NumPy's default) of `values` at level q, as a Fraction when it is finite and as a
    float (+-inf, or NaN only beside a NaN input) otherwise.  Neighbours a <= b with fraction g:
        g == 0 or a == b   a
        both finite        a + g (b - a), in rational arithmetic
        otherwise          (1 - g) a + g b in the extended reals: a finite a beside +inf with g > 0 gives +inf, -inf beside a
                           finite b with g < 1 gives -inf; -inf beside +inf is the limit of (2 g - 1) M as M grows: -inf below
                           g = 1/2, +inf above it, 0 at it."""
    a, b, g, _ = quantile7_neighbours(values, q)
    if g == 0 or a == b:
        return Fraction(a) if math.isfinite(a) else a
    if math.isnan(a) or math.isnan(b):
        return math.nan
    if math.isfinite(a) and math.isfinite(b):
        return Fraction(a) + g * (Fraction(b) - Fraction(a))
    if math.isfinite(a):
        return b                       # b = +inf, g > 0
    if math.isfinite(b):
        return a                       # a = -inf, g < 1
    return a if g < Fraction(1, 2) else (b if g > Fraction(1, 2) else Fraction(0))


def quantile7_bound(values, q):
    """The rounding bound of a + g (b - a) in binary64 for finite neighbours (derivation: tests/test_gpu_consumers.py):
    (count + 2) eps |b - a| + 2 eps max(|a|, |b|), as a Fraction; None when a neighbour is not finite (then the match is exact)."""
    a, b, _, n = quantile7_neighbours(values, q)
    if not (math.isfinite(a) and math.isfinite(b)):
        return None
    e = Fraction(EPS)
    return (n + 2) * e * abs(Fraction(b) - Fraction(a)) + 2 * e * max(abs(Fraction(a)), abs(Fraction(b)))
