"""The references of tests/consumers_ref.py stand on their own: the exact quantile against np.quantile on finite vectors (to the
rounding bound the GPU tests use), the rule for infinite order statistics on the vectors where np.quantile itself returns NaN, and
the column maxima / the filter on matrices small enough to check by eye.  No GPU, no library call."""
import math
from fractions import Fraction

import numpy as np
import pytest

from consumers_ref import colmax_ref, colmax_ref_fast, quantile7_bound, quantile7_neighbours, quantile7_ref, threshold_ref

INF, NAN = math.inf, math.nan


@pytest.mark.parametrize("n", [1, 2, 3, 64, 101, 1000, 4097])
def test_quantile7_ref_against_numpy_on_finite_vectors(n):
    rng = np.random.default_rng(100 + n)
    probs = [0.0, 1.0, 0.5, 0.9, 0.95, 1.0 / 3.0, 0.07, 1e-9, 1.0 - 2.0 ** -53] + list(rng.random(20))
    for v in (rng.random(n) * 6.0, rng.standard_normal(n) * 1e3, np.sort(rng.random(n)), np.full(n, 2.5),
              np.repeat(rng.random(10), (n + 9) // 10)[:n]):
        for q in probs:
            exact, bound = quantile7_ref(v, q), quantile7_bound(v, q)
            assert isinstance(exact, Fraction) and bound is not None
            # np.quantile evaluates the same expression in binary64 (with its own rounding of h and of the lerp)
            assert abs(Fraction(float(np.quantile(v, q))) - exact) <= bound, (n, q)
            a, b, g, cnt = quantile7_neighbours(v, q)
            assert cnt == n and a <= exact <= b and 0 <= g < 1


def test_quantile7_ref_exact_levels_and_clamping():
    v = np.arange(101.0)[::-1] ** 2
    s = np.sort(v)
    for k in range(101):
        # (count - 1) q is the integer k in exact arithmetic only where k / 100 is a double; elsewhere it is within 100 eps of it
        got = quantile7_ref(v, k / 100)
        assert abs(got - Fraction(float(s[k]))) <= 100 * 2.0 ** -53 * 201
    for k in (0, 25, 50, 75, 100):
        assert quantile7_ref(v, k / 100) == Fraction(float(s[k]))
    assert quantile7_ref(v, -0.5) == quantile7_ref(v, 0.0) == 0
    assert quantile7_ref(v, 1.5) == quantile7_ref(v, 1.0) == quantile7_ref(v, INF) == 10000
    assert quantile7_ref([3.0, 1.0], 0.25) == Fraction(3, 2)
    assert quantile7_ref([7.0], 0.3) == 7


def test_quantile7_ref_rule_for_infinite_order_statistics():
    # the vectors on which a + g (b - a) -- np.quantile's expression too -- is inf - inf = NaN without a NaN among the inputs
    assert quantile7_ref([1.0, 2.0, INF, INF], 0.5) == INF            # h = 1.5: between 2 and +inf
    assert quantile7_ref([1.0, 2.0, INF, INF], 0.9) == INF            # between +inf and +inf: that infinity
    assert quantile7_ref([1.0, 2.0, INF, INF], 1.0 / 3.0) == Fraction(float(1.0 / 3.0)) * 3 + 1   # both neighbours finite
    assert quantile7_ref([1.0, 2.0, INF, INF], 0.25) == Fraction(7, 4)
    for q in (0.0, 0.1, 0.5, 0.99, 1.0):
        assert quantile7_ref([-INF, -INF, -INF], q) == -INF
    assert quantile7_ref([-INF, 1.0, 2.0], 0.25) == -INF              # -inf beside a finite b, g = 1/2 < 1
    assert quantile7_ref([-INF, 1.0, 2.0], 0.5) == 1                  # g == 0: the order statistic itself
    assert quantile7_ref([-INF, 1.0, 2.0], 0.0) == -INF
    assert quantile7_ref([1.0, INF], 0.0) == 1                        # g == 0 beside +inf stays finite
    assert quantile7_ref([1.0, INF], 2.0 ** -60) == INF               # any g > 0 does not
    # opposite infinities: the limit of (2 g - 1) M
    assert quantile7_ref([-INF, INF], 0.25) == -INF and quantile7_ref([-INF, INF], 0.75) == INF
    assert quantile7_ref([-INF, INF], 0.5) == 0
    # NaN only beside a NaN input (NaN sorts last)
    assert quantile7_ref([1.0, 2.0, NAN], 0.5) == 2 and math.isnan(quantile7_ref([1.0, 2.0, NAN], 0.75))
    for vec in ([1.0, 2.0, INF, INF], [-INF, -INF, -INF], [-INF, 1.0, INF], [-INF, INF]):
        for q in np.linspace(0.0, 1.0, 41):
            r = quantile7_ref(vec, float(q))
            assert isinstance(r, Fraction) or not math.isnan(r)
            assert quantile7_bound(vec, float(q)) is None or isinstance(r, Fraction)


def test_colmax_ref_by_hand():
    L = np.array([[1.0, NAN, -INF],
                  [3.0, NAN, -INF],
                  [3.0, NAN, NAN]])
    for f in (colmax_ref, colmax_ref_fast):
        mx, arg = f(L)
        assert mx.tolist() == [3.0, -INF, -INF] and arg.tolist() == [1, -1, -1] and arg.dtype == np.int64
    L = np.array([[-1.0, NAN, INF],
                  [-0.0, 5.0, 2.0],
                  [0.0, -INF, INF]])
    for f in (colmax_ref, colmax_ref_fast):
        mx, arg = f(L)
        assert mx.tolist() == [0.0, 5.0, INF] and arg.tolist() == [1, 1, 0]
        assert math.copysign(1.0, mx[0]) == -1.0                      # the zero of the lowest row
    for f in (colmax_ref, colmax_ref_fast):
        mx, arg = f(np.empty((0, 2)))
        assert mx.tolist() == [-INF, -INF] and arg.tolist() == [-1, -1]


def test_colmax_ref_fast_equals_the_plain_loop():
    rng = np.random.default_rng(7)
    L = rng.standard_normal((200, 40))
    L[rng.random(L.shape) < 0.05] = NAN
    L[rng.random(L.shape) < 0.02] = -INF
    L[:, 3] = NAN
    L[:, 4] = -INF
    L[17, 5] = L[150, 5] = INF
    L[130, 6] = L[2, 6] = 50.0
    L[:, 7] = -np.abs(L[:, 7]) - 1.0
    L[9, 7], L[11, 7] = -0.0, 0.0
    L[:, 7][np.isnan(L[:, 7])] = -2.0
    a, b = colmax_ref(L), colmax_ref_fast(L)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(np.signbit(a[0]), np.signbit(b[0]))
    assert a[1][5] == 17 and a[1][6] == 2 and a[1][7] == 9


def test_threshold_ref_by_hand():
    L = np.array([[1.0, NAN, -INF],
                  [2.0, 2.0, INF],
                  [3.0, -1.0, 2.0]])
    def trip(thr):
        i, j, l = threshold_ref(L, thr)
        assert i.dtype == np.int32 and j.dtype == np.int32
        return list(zip(i.tolist(), j.tolist(), l.tolist()))
    assert trip(2.0) == [(2, 0, 3.0), (1, 2, INF)]                    # strict: the three 2.0 stay out
    assert trip(-INF) == [(0, 0, 1.0), (1, 0, 2.0), (2, 0, 3.0), (1, 1, 2.0), (2, 1, -1.0), (1, 2, INF), (2, 2, 2.0)]
    assert trip(INF) == [] and trip(NAN) == []
    assert trip(2.5) == [(2, 0, 3.0), (1, 2, INF)]
