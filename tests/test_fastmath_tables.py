"""The generated tables behind the device's LOD and p-value maps (bulklmm.jl_amd/csrc/log_table.h, pval_table.h), checked entry by
entry against high-precision references, and against their generators (tools/gen_log_table.py, tools/gen_pval_table.py).
No GPU: what is checked is the data every LOD and -log10 p of the library is computed from."""
import os
import struct
import subprocess
import sys
from fractions import Fraction

import mpmath as mp
import numpy as np
import pytest

from fastmath_tables import (LOG_TABLE_H, PVAL_TABLE_H, ROOT, dbl, fma, hiword, log_tables, pv_bucket, pv_eval, pval_table,
                             w_ref)

# tools/gen_pval_table.py prints 4.27e-15 for the largest relative error of -log10 p = LOD + x w(x) over the table's range (33
# points a bucket); the 66 points a bucket here are held to that figure with a margin of 20 %
PV_TOTAL_BOUND = 5.2e-15
# and w itself, the polynomial of each bucket against -log10(erfcx(x)) / x: 1e-12 relative (the largest seen is 8.1e-13, bucket 201
# at x = 8192, where x w(x) is 6e-8 of LOD; below x = 8 it is under 1e-14)
PV_W_BOUND = 1e-12


@pytest.mark.parametrize("gen,header", [("gen_log_table.py", LOG_TABLE_H), ("gen_pval_table.py", PVAL_TABLE_H)])
def test_generator_reproduces_header(tmp_path, gen, header):
    out = tmp_path / os.path.basename(header)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", gen), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == open(header, "rb").read(), f"{gen} no longer writes the committed {os.path.basename(header)}"


def test_log_table_entries():
    """{invc, ln c, log10 c}: with c = 1 / invc taken exactly, both logarithms are its correctly rounded values, c inside interval i of fast_log
    (x in [0.6875, 1.375) cut by the 7 mantissa bits after OFF), and the intervals that touch 1 with invc = 1, log(c) = 0."""
    mp.mp.dps = 50
    d, tab, _ = log_tables()
    assert tab.shape == (int(d["BLMM_LOG_TABLE_N"]), 3) == (128, 3)
    assert float(d["BLMM_LN2"]) == float(mp.log(2)) and float(d["BLMM_LOG10_2"]) == float(mp.log10(2))
    assert float(d["BLMM_INV_LN10"]) == float(1 / mp.log(10))
    off = 0x3FE6000000000000
    for i, (invc, lnc, lgc) in enumerate(tab):
        lo = struct.unpack("<d", struct.pack("<Q", off + (i << 45)))[0]
        hi = struct.unpack("<d", struct.pack("<Q", off + ((i + 1) << 45)))[0]
        c = 1 / mp.mpf(invc)                          # exactly 1 / invc at 50 digits
        assert lnc == float(mp.log(c)), (i, lnc)
        assert lgc == float(mp.log10(c)), (i, lgc)
        assert lo <= c < hi or (invc == 1.0 and lo <= 1.0 <= hi), (i, lo, hi, invc)
        if lo <= 1.0 < hi or lo < 1.0 <= hi:
            assert (invc, lnc, lgc) == (1.0, 0.0, 0.0), i


def test_lod_table_entries():
    """The directly indexed LOD table: entry i belongs to c_i = the double with high word HI0 + (i << 11), which fast_lod5 maps back
    to i ((hi - HI0 + 2^10) >> 11); invc is 1 / c_i correctly rounded; log10(c) = -log10(invc) correctly rounded; the last entry
    is c = 1 (invc = 1, log10 c = 0) and its bucket runs up to u = 1."""
    mp.mp.dps = 50
    d, _, lod = log_tables()
    n, hi0 = int(d["BLMM_LOD_TABLE_N"]), int(d["BLMM_LOD_HI0"].rstrip("u"), 16)
    assert lod.shape == (n, 2) == (2049, 2) and hi0 == 0x3FB00000
    for i, (invc, lgc) in enumerate(lod):
        c = dbl(hi0 + (i << 11))
        assert ((hiword(c) - hi0 + (1 << 10)) >> 11) == i
        assert invc == float(Fraction(1) / Fraction(c)), i              # Fraction -> float rounds once, to nearest
        assert abs(Fraction(invc) * Fraction(c) - 1) <= Fraction(1, 2 ** 53), i
        assert lgc == float(-mp.log10(mp.mpf(invc))), (i, lgc)
    assert dbl(hi0 + ((n - 1) << 11)) == 1.0 and tuple(lod[-1]) == (1.0, 0.0)
    assert ((hiword(1.0) - hi0 + (1 << 10)) >> 11) == n - 1
    assert ((hiword(0.0625) - hi0 + (1 << 10)) >> 11) == 0


def _bucket_points(b, d, rng):
    lo, hi, _ = pv_bucket(b, d)
    top = float(np.nextafter(hi, 0.0))
    pts = [lo, top] + list(rng.uniform(lo, hi, 64))
    return [x for x in pts if x > 0.0 or b == 0]


def test_pval_table_buckets():
    """Every bucket's degree-7 polynomial in s = x - c, evaluated as fast_log10p1 does (Horner, one fma a step), at both edges and 64
    interior points, against 40-digit w(x) = -log10(erfcx(x)) / x, and the -log10 p it makes, LOD + x w(x) (fma)."""
    mp.mp.dps = 40
    d, tab = pval_table()
    assert tab.shape == (209, 10) and int(d["BLMM_PV_SHIFT"]) == 17
    assert np.all(tab[:, 8:] == 0.0)
    ln10 = mp.log(10)
    rng = np.random.default_rng(20240)
    worst_w, worst_t = (0.0, None), (0.0, None)
    for b in range(tab.shape[0]):
        _, _, c = pv_bucket(b, d)
        for x in _bucket_points(b, d, rng):
            w = pv_eval(tab[b], c, x)
            wr = w_ref(x, mp)
            ew = float(abs(mp.mpf(w) - wr) / wr)
            if ew > worst_w[0]:
                worst_w = (ew, (b, x))
            if x == 0.0:
                continue
            lod = float(mp.mpf(x) ** 2 / ln10)
            got = fma(x, w, lod)
            ref = -mp.log10(mp.erfc(mp.sqrt(mp.mpf(lod) * ln10)))
            et = float(abs(mp.mpf(got) - ref) / ref)
            if et > worst_t[0]:
                worst_t = (et, (b, x))
    print(f"pval_table: worst relative error of w {worst_w[0]:.3g} at (bucket, x) {worst_w[1]}; of -log10 p {worst_t[0]:.3g} at {worst_t[1]}")
    assert worst_w[0] <= PV_W_BOUND, worst_w
    assert worst_t[0] <= PV_TOTAL_BOUND, worst_t
