"""The generated tables of bulklmm.jl_amd/csrc (log_table.h, pval_table.h) read back as numbers, and exact references for the
arithmetic the device does on them (tests/test_fastmath_tables.py, tests/test_gpu_fastmath.py)."""
import os
import re
import struct
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bulklmm.jl_amd", "csrc")
LOG_TABLE_H = os.path.join(CSRC, "log_table.h")
PVAL_TABLE_H = os.path.join(CSRC, "pval_table.h")


def _defines(text):
    return {m.group(1): m.group(2) for m in re.finditer(r"^#define (\w+) (\S+)", text, re.M)}


def _array(text, name):
    body = re.search(r"%s\[[^\]]*\] = \{(.*?)\};" % name, text, re.S).group(1)
    return np.array([float.fromhex(v) for v in re.findall(r"-?0x[0-9a-f.]+p[+-]\d+", body)], dtype=np.float64)


def log_tables():
    """(defines, {invc, ln c, log10 c} rows of the 128-entry table, {invc, log10 c} rows of the directly indexed LOD table)"""
    text = open(LOG_TABLE_H).read()
    d = _defines(text)
    return d, _array(text, "blmm_log_table_host").reshape(-1, 3), _array(text, "blmm_lod_table_host").reshape(-1, 2)


def pval_table():
    """(defines, the p-value table as BLMM_PV_TABLE_N rows of BLMM_PV_STRIDE doubles)"""
    text = open(PVAL_TABLE_H).read()
    d = _defines(text)
    return d, _array(text, "blmm_pv_table_host").reshape(int(d["BLMM_PV_TABLE_N"]), int(d["BLMM_PV_STRIDE"]))


def dbl(hi, lo=0):
    return struct.unpack("<d", struct.pack("<Q", ((hi & 0xFFFFFFFF) << 32) | (lo & 0xFFFFFFFF)))[0]


def hiword(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0] >> 32


def fma(a, b, c):
    """a * b + c rounded once (Fraction -> float rounds to nearest even)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def pv_bucket(b, d):
    """(lo, hi, centre) of bucket b of pval_table.h as doubles (tools/gen_pval_table.py: bucket)"""
    hi0, shift = int(d["BLMM_PV_HI0"].rstrip("u"), 16), int(d["BLMM_PV_SHIFT"])
    if b == 0:
        return 0.0, dbl(hi0), 0.0
    h = hi0 + ((b - 1) << shift)
    return dbl(h), dbl(h + (1 << shift)), dbl(h + (1 << (shift - 1)))


def pv_eval(row, centre, x):
    """fast_log10p1's evaluation of w(x) on one bucket row: s = x - c, Horner with an fma per step from c7 down to c0"""
    s = x - centre
    w = row[7]
    for k in range(6, -1, -1):
        w = fma(w, s, row[k])
    return w


def w_ref(x, mp):
    """w(x) = -log10(erfcx(x)) / x in mpmath at its current precision"""
    x = mp.mpf(x)
    if x == 0:
        return 2 / (mp.sqrt(mp.pi) * mp.log(10))
    return -(mp.log(mp.erfc(x)) + x * x) / (mp.log(10) * x)
