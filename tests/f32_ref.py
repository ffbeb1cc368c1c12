"""Host model of the fp32 permutation scan (bulklmm.jl_amd/csrc/kernels_scan_f32.hip) and a per-entry error bound derived from the
operations its kernels perform.  Test infrastructure: tests/test_f32_bound.py checks the bound on the host, tests/
test_gpu_perms_f32_edges.py holds the device to it.

THE OPERANDS (fp64, on the library's own rotation).  With the device's eigenvectors U' (blmm_rotate of the identity: device_rotation),
design Zs = W [1 Cov] (W = diag(weights), k_design), Z0 = U' Zs and the unweighted projection Q = I - Z0 (Z0'Z0)^-1 Z0', the
rotation is R = Q U' W (k_post_eigen, centered = 1) and the rotated marker columns are x~_i = R g_i.  At the device's h2, with
w_k = 1 / (1 + delta lambda_k), delta = h2 / (1 - h2), and B = sqrt(w) Z0, P = I - B (B'B)^-1 B' (a Euclidean orthogonal projection):
    r0  = sqrt(w) (R y - Z0 beta)        (the weighted-LS residual: P r0 = r0)
    a_b = sqrt(w) P pi_b(r0) / |r0|      (k_perm_panel / k_perm_fill; column 0 of the "original" panel is a_0 = sqrt(w) r0 / |r0|)
    isx_i = 1 / |P sqrt(w) x~_i|         (k_isx; from the fp32 columns on the own-rotation route: k_isx<C, true>)
    s_ib = x~_i' a_b,   r_ib = s_ib isx_i,   L_ib = -(n/2) log10(1 - r_ib^2).

THE BOUND.  u = 2^-24, gamma_k = k u / (1 - k u); sums run over k < n (the padding to npad, kpad and ldrr holds exact zeros on
one side of every product: k_cvt_f32 writes 0 beyond `rows_valid`, k_cvt_r32 beyond n, and 0 * finite = 0 adds nothing).
  (1) Operands.  fp64 route: k_cvt_f32 converts x~ and a_b with round-to-nearest, xf = x~ (1 + d), af = a (1 + d'), |d|, |d'| <= u.
      Own-rotation route (c = 1, tuning f32_rotation = 1): k_cvt_r32 converts R and k_rotate_f32's store_chunk converts G in
      registers, then 32x32x2 fp32 MFMAs form XF = R G as one fp32 fma chain of n terms per element; the accumulator IS the stored
      operand (no further conversion).  Per element
          |XF_ki - x~_ki| <= E_ki := gamma_{n+2} (|R| |G|)_ki  + t_rot,
      gamma_{n+2} >= (1 + gamma_2)(1 + gamma_n) - 1 covering the two conversions and the chain.  The panel is still k_cvt_f32's.
  (2) Contraction.  k_scan_f32's mfma_f32_32x32x2f32 is bit for bit a k-ordered fp32 fma chain (one rounding per step; the order
      k = 8 kb + 2 j + h is ascending k), so for a chain of n products |fl(sum) - sum| <= gamma_n sum |xf af|.  Together with (1):
          fp64 route:  e_num <= gamma_{n+2} S + t_scan,                         S = sum_k |x~_k| |a_k|
          own route:   e_num <= SE + gamma_{n+1} (S + SE) + t_scan,             SE = sum_k E_k |a_k|
      (own route: one conversion (of a) and the chain on the operand XF = x~ + (XF - x~)).
  (3) Marker scale.  fp64 route: isx is fp64 from the fp64 x~ (its error belongs to term (6)).  Own route: isx_dev = 1 / |P sqrt(w)
      XF_i|, fp64 sums of fp32 columns; since P has norm 1, | |P sqrt(w) XF_i| - |P sqrt(w) x~_i| | <= |sqrt(w) E_i| =: e_i, so
      |isx_dev / isx - 1| <= d_isx := rho / (1 - rho),  rho = e_i isx_i   (no bound where rho >= 1).
  (4) r.  The device forms rr = fl(acc * fl32(isx_dev)) (epilogue: sc[nb], then acc * sc): relative gamma_2 on top of
          |acc isx_dev - r| <= D1 := e_num isx (1 + d_isx) + |s| isx d_isx,      Dr = D1 + gamma_2 (|r| + D1),
      and r2 = fl(rr * rr) adds one more relative u:  r2_dev in [ (|r| - Dr)_+^2 (1 - u), (|r| + Dr)^2 (1 + u) ] =: [lo, hi].
  (5) r to LOD.  L(r2) = -(n/2) log10(1 - r2) is increasing, so |L(r2_dev) - L(r^2)| <= max(L(hi) - L, L - L(lo)) -- the exact
      image of the interval, not the first-order dL = (n / ln 10) r dr / (1 - r^2) it reduces to for small Dr; hi >= 1 gives no
      bound (+inf: such entries are counted, not compared).  Then the fp32 epilogue lod_f32, whose error against the fp64 log1p of
      its own fp32 input was measured exhaustively over every fp32 r^2 in [0, 1] (tests/test_gpu_fastmath.py::
      test_lod_f32_exhaustive, n = 2048; figure recorded in fastmath.h): <= 2.5e-7 |L| where L >= 1 and <= 2.5e-4 (1e-3 |L| + 1e-4)
      everywhere.  That measurement includes the fp32 scale, the final fp32 rounding of the result (the value k_scan_f32 stores) and,
      at n < 2048, overstates the absolute part (it scales with n).  Both figures are added, at L(hi).
  (6) Reference.  The device's fp64 operands (rotation, panel, fp64 isx) differ from these host ones by fp64 rounding; the fp64
      route is held to RTOL |L| + ATOL (tests/common.py) against the oracle, and that term is added.
  Subnormals (fp32 subnormals are kept: hipcc's default mode): each rounding of a chain may add 2^-150 absolute, times at most
  (1 + max |operand|) where it is multiplied: t_rot = (n + 2) 2^-150 (1 + |R|max) (1 + |G|max), t_scan = (n + 2) 2^-150 (1 + |x~|max
  + |E|max) (1 + |a|max).
Every constant above is a unit roundoff, a chain length, or the recorded epilogue figure: nothing is fitted.

The emulation (emulate_scan, emulate_rotation) replays the kernels' arithmetic on the host: fp32 operands, one fp32 rounding per
fma step in the kernels' order, each step's sum formed in fp64 with round-to-odd before the rounding to fp32 (round-to-odd at
53 >= 24 + 2 bits makes the double rounding exact), checked against exact rational arithmetic by tests/test_f32_bound.py."""
import math

import numpy as np

U32 = 2.0 ** -24
TINY = 2.0 ** -150
EPI_REL = 2.5e-7          # lod_f32, |d| / |L| where L >= 1 (fastmath.h)
EPI_CONTRACT = 2.5e-4     # lod_f32, |d| / (1e-3 |L| + 1e-4) everywhere (fastmath.h)
FP64_RTOL, FP64_ATOL = 1e-6, 1e-10
LN10 = math.log(10.0)


def gamma(k):
    return k * U32 / (1.0 - k * U32)


def r2lod(r2, n):
    with np.errstate(divide="ignore", invalid="ignore"):
        return -(n / 2.0) * np.log1p(-np.asarray(r2, dtype=np.float64)) / LN10


# ---- the library's own permutations (k_perm_panel / k_perm_gen: Fisher-Yates from a splitmix64 counter stream) ------------------
M64 = (1 << 64) - 1


def splitmix_perms(n, nperms, seed):
    """n x nperms (0-based) permutations the device draws for `seed` (column b: permbuf[b * n + k])."""
    out = np.empty((n, nperms), dtype=np.int32)
    for b in range(nperms):
        s = (seed * 0xD1342543DE82EF95 + b + 1) & M64
        perm = list(range(n))
        for k in range(n - 1, 0, -1):
            s = (s + 0x9E3779B97F4A7C15) & M64
            z = s
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
            z ^= z >> 31
            r = z % (k + 1)
            perm[k], perm[r] = perm[r], perm[k]
        out[:, b] = perm
    return out


def weighted_kinship(K, weights):
    """k_design's Ks: K_ij (w_i w_j), bit for bit."""
    K = np.asarray(K, dtype=np.float64)
    return K if weights is None else K * np.outer(weights, weights)


def device_rotation(blmm, K, weights=None, ctx=None):
    """(U', lambda) of the device's eigen-decomposition of W K W: blmm_rotate (uncentred) of the identity."""
    n = K.shape[0]
    Ut, _, lam = blmm.transform_rotation(np.eye(n), np.zeros((n, 1)), weighted_kinship(K, weights), ctx=ctx)
    return Ut, lam


class Operands:
    """The fp64 operands of one permutation scan on a given rotation (see the module docstring)."""

    def __init__(self, y, G, Ut, lam, h2, perm_idx, Covar=None, weights=None):
        y = np.asarray(y, dtype=np.float64).ravel()
        G = np.asarray(G, dtype=np.float64)
        n = y.shape[0]
        w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
        Z = np.ones((n, 1)) if Covar is None else np.hstack([np.ones((n, 1)), np.asarray(Covar, dtype=np.float64).reshape(n, -1)])
        Z0 = Ut @ (w[:, None] * Z)
        Q = np.eye(n) - Z0 @ np.linalg.solve(Z0.T @ Z0, Z0.T)
        self.n, self.G = n, G
        self.R = Q @ (Ut * w[None, :])
        self.X = self.R @ G
        y0 = self.R @ y
        delta = h2 / (1.0 - h2)
        self.sw = np.sqrt(1.0 / (delta * lam + 1.0))
        Qb, _ = np.linalg.qr(self.sw[:, None] * Z0)
        self.proj = lambda V: V - Qb @ (Qb.T @ V)
        r0 = self.proj(self.sw * y0)
        nr = np.linalg.norm(r0)
        self.a0 = self.sw * r0 / nr
        self.A = self.sw[:, None] * self.proj(r0[np.asarray(perm_idx)]) / nr
        self.isx = 1.0 / np.linalg.norm(self.proj(self.sw[:, None] * self.X), axis=0)

    def r(self, X=None, isx=None):
        X = self.X if X is None else X
        return (X.T @ self.A) * (self.isx if isx is None else isx)[:, None]

    def L(self):
        """fp64 L_perms (p x nperms) on these operands."""
        r = self.r()
        return r2lod(r * r, self.n)

    def lod(self):
        r = (self.X.T @ self.a0) * self.isx
        return r2lod(r * r, self.n)

    def rotation_error(self):
        """E (n x p): the bound (1) on |XF - x~| of the own-rotation route."""
        n = self.n
        t_rot = (n + 2) * TINY * (1.0 + np.abs(self.R).max()) * (1.0 + np.abs(self.G).max())
        return gamma(n + 2) * (np.abs(self.R) @ np.abs(self.G)) + t_rot

    def bound(self, own_rotation):
        """Per-entry bound (p x nperms) on |L_dev - L| for the fp32 route; own_rotation: c = 1 with tuning f32_rotation = 1."""
        n = self.n
        aA = np.abs(self.A)
        S = np.abs(self.X).T @ aA
        if own_rotation:
            E = self.rotation_error()
            SE = E.T @ aA
            t_scan = (n + 2) * TINY * (1.0 + np.abs(self.X).max() + E.max()) * (1.0 + aA.max())
            e_num = SE + gamma(n + 1) * (S + SE) + t_scan
            rho = np.linalg.norm(self.sw[:, None] * E, axis=0) * self.isx
            with np.errstate(divide="ignore"):
                d_isx = np.where(rho < 1.0, rho / (1.0 - rho), np.inf)
        else:
            t_scan = (n + 2) * TINY * (1.0 + np.abs(self.X).max()) * (1.0 + aA.max())
            e_num = gamma(n + 2) * S + t_scan
            d_isx = np.zeros(self.X.shape[1])
        s = self.X.T @ self.A
        isx = self.isx[:, None]
        r = np.abs(s) * isx
        d1 = e_num * isx * (1.0 + d_isx[:, None]) + np.abs(s) * isx * d_isx[:, None]
        dr = d1 + gamma(2) * (r + d1)
        hi = (r + dr) ** 2 * (1.0 + U32)
        lo = np.maximum(r - dr, 0.0) ** 2 * (1.0 - U32)
        L = r2lod(r * r, n)
        with np.errstate(invalid="ignore"):
            Lhi = np.where(hi < 1.0, r2lod(np.minimum(hi, 1.0), n), np.inf)
        Llo = r2lod(lo, n)
        with np.errstate(invalid="ignore"):
            dL = np.maximum(Lhi - L, L - Llo)
        epi = EPI_REL * Lhi + EPI_CONTRACT * (1e-3 * Lhi + 1e-4)
        return dL + epi + FP64_RTOL * L + FP64_ATOL


# ---- emulation of the kernels' fp32 arithmetic ---------------------------------------------------------------------------------
def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def fma32(acc, x, y):
    """fl32(acc + x y) for fp32 values held in fp64 arrays: x y is exact in fp64 (48 bits); the sum is rounded to odd in fp64
    (TwoSum, then the neighbour with an odd last bit when inexact), which makes the final rounding to fp32 correct."""
    p = x * y
    s = acc + p
    bb = s - acc
    err = (acc - (s - bb)) + (p - bb)
    fix = (err != 0.0) & ((s.view(np.int64) & 1) == 0)
    if fix.any():
        s = s.copy()
        s[fix] = np.nextafter(s[fix], np.where(err[fix] > 0, np.inf, -np.inf))
    return f32(s)


def emulate_chain(Xf, Af, order):
    """acc[i, b] = the fp32 fma chain of Xf[k, i] Af[k, b] over k in `order` (Xf, Af: fp32 values)."""
    acc = np.zeros((Xf.shape[1], Af.shape[1]))
    for k in order:
        acc = fma32(acc, Xf[k][:, None], Af[k][None, :])
    return acc


def rotate_order(n):
    """k_rotate_f32's contraction order: chunks of 16 rows R0, eight MFMA steps s8, each with slots h = 0, 1 at R0 + 8 h + s8."""
    return [r for R0 in range(0, n, 16) for s8 in range(8) for r in (R0 + s8, R0 + 8 + s8) if r < n]


def emulate_rotation(op):
    """XF of k_rotate_f32 (n x p, fp32 values)."""
    return emulate_chain(f32(op.R).T.copy(), f32(op.G), rotate_order(op.n))


def emulate_scan(op, XF=None, isx=None, order=None, a_index=None):
    """L_perms of k_scan_f32 (p x nperms): fp32 operands (k_cvt_f32 of x~ unless XF is given), the ascending-k fma chain (or
    `order`), r = fl(acc fl32(isx)), r2 = fl(r r), and the exact L of that fp32 r2 (the epilogue's own error is term (5) of the
    bound, measured on the device).  a_index[k]: the panel row that step k reads (planted mistakes)."""
    n = op.n
    Xf = f32(op.X) if XF is None else XF
    Af = f32(op.A)
    if a_index is not None:
        Af = Af[np.asarray(a_index)]
    acc = emulate_chain(Xf, Af, range(n) if order is None else order)
    sc = f32(op.isx if isx is None else isx)[:, None]
    rr = f32(acc * sc)
    r2 = f32(rr * rr)
    return r2lod(r2, n)


def isx_of(op, XF):
    """k_isx<C, true>: 1 / |P sqrt(w) XF_i| in fp64 from the fp32 columns."""
    return 1.0 / np.linalg.norm(op.proj(op.sw[:, None] * XF), axis=0)


def locate(ratio, op):
    """Where the worst entry of a p x nperms error/bound array sits in k_scan_f32's tiling: marker, permutation, marker tile of 256,
    permutation tile of 128 and its group of 8, and the K block of 8 that carries the entry's largest product |x~_k a_k|."""
    i, b = np.unravel_index(int(np.nanargmax(ratio)), ratio.shape)
    k = int(np.argmax(np.abs(op.X[:, i]) * np.abs(op.A[:, b])))
    return (f"marker {i} (tile {i // 256}), permutation {b} (tile {b // 128}, group {b // 1024}), "
            f"K block {k // 8} of {(op.n + 7) // 8}")
