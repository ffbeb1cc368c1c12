// kernels_cond.hip -- blmm_bulkscan_cond: every trait scanned with its OWN conditioning loci in the null design.
//
// Trait j's null design is D_j = [Z0, the kept columns among x0_{cond[j, 0]}, .., x0_{cond[j, s - 1]}] (rotated, uncentred: k_mdf_rawrot),
// c + r_j <= CT = c + s <= 8 columns.  The kernels are templates over CT; a trait with fewer columns runs them with `ct` live columns,
// the dead ones being zero columns whose Cholesky pivot is replaced by 1 (they then contribute nothing anywhere).
//
//   k_cond_null    one wave per trait.  Step 1: the unweighted Gram of [Z0, the trait's valid columns] factored with multidf's rank
//                  rule (column a kept iff its pivot, the squared norm of the part orthogonal to Z0 and the kept columns before it,
//                  exceeds MDF_TAU |x0_a|^2) -> kept[], r_j.  Then the null model on D_j: fitlmm (the scalar Brent of brent_scalar.h
//                  on -ell, src/lmm.jl:56-86) or the first arg-max of ell over the grid (src/wls.jl:27-97 per point); the 64 lanes
//                  split the individuals, the (c + r_j)(c + r_j + 1)/2 + c + r_j + 2 sums are wave reductions, the factorisation
//                  is closed form in registers.  A trait with r_j = 0 gets bulkscan's null model through the same code.
//   k_cond_panels  one thread per trait (coalesced panel rows, as k_panels): panel 0 = w .* residual / |.|, panel 1 = w,
//                  panels 2 .. 1 + ct = w .* (D_j L^-T)_q, zero panels up to 1 + CT.  Also the conditioning guard's criterion
//                  (k_illcond_flag's: the smallest pivot share of D_j'WD_j below rho_min) -> flag[], list, stat[ST_ILLCOND].
//   the scan       k_scan<.., COND> (kernels_scan.hip): the f64-MFMA contraction with 2 + CT accumulators and the rank-rule epilogue.
//   k_cond_qr      the listed traits again with an orthonormal basis of span(sqrt(W) D_j) (Gram-Schmidt twice) and explicit
//                  residuals (ortho_basis.h), the rank rule on the explicit norms.
// blmm_bulkscan_stepwise runs the same kernels round after round on a compact list of active traits (CondArgs::act: panel column jj
// is trait act[jj]; kept / nk / flag / h2 are per column), the scan in its reducing form, k_cond_qr<RED> into a compact scratch, and
//   k_step_update  one workgroup: a round's (maximum, marker) per column -> the caller's tables, the trait's next locus, and the
//                  next round's list in ascending trait order.
#include "blmm_internal.h"
#include "fastmath.h"
#include "ortho_basis.h"
#include "brent_scalar.h"
#include <cmath>

namespace blmm {

#define KCHECK()                                                                                      \
  do {                                                                                                \
    hipError_t e__ = hipGetLastError();                                                               \
    if (e__ != hipSuccess) return fail(ctx, BLMM_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e__)); \
  } while (0)

// ---- the sums of one evaluation, wave-wide: A = D'WD (packed lower), v = D'Wy, y'Wy, sum ln(delta lambda + 1) ---------------------
template <int CT>
struct CondSums { double A[CT * (CT + 1) / 2], v[CT], syy, logsum; int bad; };

// column q of the design at individual k: Z0's for q < c, the trait's staged conditioning column q - c for q < ct, else 0
template <int CT>
__device__ __forceinline__ void cond_row(double (&z)[CT], int k, int n, int c, int ct, const double* __restrict__ Z0, const double* sX) {
#pragma unroll
  for (int q = 0; q < CT; ++q) z[q] = (q < c) ? Z0[(size_t)q * n + k] : (q < ct ? sX[(size_t)(q - c) * n + k] : 0.0);
}

// unit: weights 1 (step 1's Gram); otherwise w = 1 / (delta lambda + 1) as the likelihood uses it (src/wls.jl:40)
template <int CT>
__device__ __forceinline__ void cond_sums(CondSums<CT>& S, bool unit, double h2, int n, int c, int ct, const double* __restrict__ Z0,
                                          const double* __restrict__ lam, const double* sY, const double* sX) {
  constexpr int NA = CT * (CT + 1) / 2;
  const int lane = threadIdx.x & 63;
  const double delta = h2 / (1.0 - h2);
#pragma unroll
  for (int a = 0; a < NA; ++a) S.A[a] = 0.0;
#pragma unroll
  for (int q = 0; q < CT; ++q) S.v[q] = 0.0;
  S.syy = 0.0; S.logsum = 0.0; S.bad = 0;
  for (int k = lane; k < n; k += 64) {
    double w = 1.0;
    if (!unit) {
      const double t = fma(delta, lam[k], 1.0);
      w = 1.0 / t;
      S.bad |= !(w > 0.0);
      S.logsum += log(t);
    }
    double z[CT];
    cond_row<CT>(z, k, n, c, ct, Z0, sX);
    const double y = sY[k], wy = w * y;
    S.syy = fma(wy, y, S.syy);
#pragma unroll
    for (int q = 0; q < CT; ++q) {
      S.v[q] = fma(wy, z[q], S.v[q]);
      const double wz = w * z[q];
#pragma unroll
      for (int r = 0; r <= q; ++r) S.A[q * (q + 1) / 2 + r] = fma(wz, z[r], S.A[q * (q + 1) / 2 + r]);
    }
  }
#pragma unroll
  for (int a = 0; a < NA; ++a) S.A[a] = group_sum<64>(S.A[a]);
#pragma unroll
  for (int q = 0; q < CT; ++q) S.v[q] = group_sum<64>(S.v[q]);
  S.syy = group_sum<64>(S.syy); S.logsum = group_sum<64>(S.logsum);
  S.bad = __any(S.bad) ? 1 : 0;
}

// ell of wls(y0_j, D_j, w, prior; reml) from the sums (null_ell's formula, kernels_prep.hip; REML's p is ct)
template <int CT>
__device__ __forceinline__ double cond_ell(const CondSums<CT>& S, int n, int ct, double prior_a, double prior_b, int reml) {
  constexpr int NA = CT * (CT + 1) / 2;
  double L[NA], t[CT], logdet = 0.0, tt = 0.0;
#pragma unroll
  for (int q = 0; q < CT; ++q) {
    const bool live = q < ct;
#pragma unroll
    for (int r = 0; r <= q; ++r) {
      double s = S.A[q * (q + 1) / 2 + r];
#pragma unroll
      for (int u = 0; u < r; ++u) s = fma(-L[q * (q + 1) / 2 + u], L[r * (r + 1) / 2 + u], s);
      if (r == q) { L[q * (q + 1) / 2 + q] = live ? sqrt(s) : 1.0; logdet += live ? log(s) : 0.0; }
      else L[q * (q + 1) / 2 + r] = live ? s / L[r * (r + 1) / 2 + r] : 0.0;
    }
    double s = S.v[q];
#pragma unroll
    for (int u = 0; u < q; ++u) s = fma(-L[q * (q + 1) / 2 + u], t[u], s);
    t[q] = live ? s / L[q * (q + 1) / 2 + q] : 0.0;
    tt = fma(t[q], t[q], tt);
  }
  const double rss = S.syy - tt;
  const double prior_df = prior_b > 0.0 ? prior_b + 2.0 : prior_b;
  const double num = rss + prior_a * prior_b;
  const double sigma2 = num / ((reml ? (double)(n - ct) : (double)n) + prior_df);
  const double ls = log(sigma2);
  double ell = -0.5 * (((double)n + prior_b) * ls + S.logsum + num / sigma2);
  if (reml) ell += 0.5 * ((double)ct * ls - logdet);
  return ell;
}

constexpr int COND_SMAX = BLMM_COND_MAX_LOCI;

// LDS: sY (n), sX (s n)
template <int CT>
__global__ void __launch_bounds__(64) k_cond_null(NullModel nm, CondArgs a, const double* __restrict__ grid, int ngrid) {
  constexpr int NA = CT * (CT + 1) / 2;
  extern __shared__ __attribute__((aligned(16))) double sh[];
  const int n = a.n, c = a.c, s = a.s, lane = threadIdx.x;
  double* sY = sh;
  double* sX = sh + n;
  const int64_t jj = blockIdx.x, j = a.act ? a.act[jj] : jj;   // column jj of the per-column arrays, trait j of Yt and cond
  // the trait's entries: valid ones in order; an index outside [-1, p) makes the whole trait NaN
  int idx[COND_SMAX], nv = 0;
  bool invalid = false;
#pragma unroll
  for (int e = 0; e < COND_SMAX; ++e) {
    idx[e] = -1;
    if (e < s) {
      const int64_t q = a.cond[j * s + e];
      if (q < -1 || q >= a.p) invalid = true;
      else if (q >= 0) {
#pragma unroll
        for (int f = 0; f < COND_SMAX; ++f) if (f == nv) idx[f] = (int)q;
        ++nv;
      }
    }
  }
  if (invalid) {
    if (lane == 0) {
      a.nk[jj] = -1; a.flag[jj] = 0; a.h2[jj] = NAN;
      for (int e = 0; e < s; ++e) a.kept[jj * s + e] = -1;
      atomicAdd((unsigned long long*)&a.info[4], 1ull);
    }
    return;
  }
  for (int k = lane; k < n; k += 64) {
    sY[k] = a.Yt[(int64_t)k * a.ldy + j];
#pragma unroll
    for (int e = 0; e < COND_SMAX; ++e)
      if (e < nv) sX[(size_t)e * n + k] = a.Xt[(int64_t)k * a.ldx + idx[e]];
  }
  __syncthreads();
  CondSums<CT> S;
  // ---- step 1: unweighted, in order ------------------------------------------------------------------------------------------
  int r = 0;
  if (nv > 0) {
    cond_sums<CT>(S, true, 0.0, n, c, c + nv, a.Z0, a.lam, sY, sX);
    double L[NA];
    unsigned keepmask = 0;
#pragma unroll
    for (int q = 0; q < CT; ++q) {
#pragma unroll
      for (int u = 0; u <= q; ++u) {
        double t = S.A[q * (q + 1) / 2 + u];
#pragma unroll
        for (int v = 0; v < u; ++v) t = fma(-L[q * (q + 1) / 2 + v], L[u * (u + 1) / 2 + v], t);
        if (u == q) {
          const bool keep = (q < c) ? true : (q < c + nv && t > MDF_TAU * S.A[q * (q + 1) / 2 + q]);
          L[q * (q + 1) / 2 + q] = keep ? sqrt(t) : 0.0;
          if (keep && q >= c) keepmask |= 1u << (q - c);
        } else {
          const double luu = L[u * (u + 1) / 2 + u];
          L[q * (q + 1) / 2 + u] = (luu > 0.0) ? t / luu : 0.0;
        }
      }
    }
    // compact the kept columns to the front of sX (a column only ever moves to a lower slot; ascending order keeps sources intact)
    int kidx[COND_SMAX];
#pragma unroll
    for (int e = 0; e < COND_SMAX; ++e) kidx[e] = -1;
#pragma unroll
    for (int e = 0; e < COND_SMAX; ++e) {
      if (e < nv && ((keepmask >> e) & 1u)) {
        if (r != e)
          for (int k = lane; k < n; k += 64) sX[(size_t)r * n + k] = sX[(size_t)e * n + k];
#pragma unroll
        for (int f = 0; f < COND_SMAX; ++f) if (f == r) kidx[f] = idx[e];
        ++r;
      }
    }
#pragma unroll
    for (int e = 0; e < COND_SMAX; ++e) idx[e] = kidx[e];
    __syncthreads();
  }
  if (lane == 0) {
    a.nk[jj] = r;
#pragma unroll
    for (int e = 0; e < COND_SMAX; ++e) if (e < s) a.kept[jj * s + e] = (e < r) ? idx[e] : -1;
    if (nv > r) atomicAdd((unsigned long long*)&a.info[1], (unsigned long long)(nv - r));
    if (r >= 1) atomicAdd((unsigned long long*)&a.info[2], 1ull);
  }
  // ---- the null model on D_j ---------------------------------------------------------------------------------------------------
  const int ct = c + r;
  int nonpos = 0, hit_max = 0;
  double best;
  if (grid) {
    int bi = 0;
    double bv = -INFINITY;
    for (int g = 0; g < ngrid; ++g) {
      cond_sums<CT>(S, false, grid[g], n, c, ct, a.Z0, a.lam, sY, sX);
      nonpos |= S.bad;
      const double e = cond_ell<CT>(S, n, ct, nm.prior_a, nm.prior_b, nm.reml);
      if (g == 0 || e > bv) { bv = e; bi = g; }
    }
    best = grid[bi];
  } else {
    auto f = [&](double h2) {
      cond_sums<CT>(S, false, h2, n, c, ct, a.Z0, a.lam, sY, sX);
      nonpos |= S.bad;
      return -cond_ell<CT>(S, n, ct, nm.prior_a, nm.prior_b, nm.reml);
    };
    best = dyn_brent_search(f, nm.optim_interval < 1 ? 1 : nm.optim_interval, &hit_max);
    wave_count(&a.stat[ST_H2_BOUNDARY], lane == 0 && h2_on_boundary(best));
  }
  if (lane == 0) {
    a.h2[jj] = best;
    if (hit_max) atomicAdd((unsigned long long*)&a.stat[ST_BRENT_MAXIT], 1ull);
    if (nonpos) atomicAdd((unsigned long long*)&a.stat[ST_NONPOS_W], 1ull);
  }
}

// ---- panels: k_panels (kernels_prep.hip) on the per-trait design; LDS: lam (n), Z0 (n c) ------------------------------------------------
template <int CT>
__global__ void __launch_bounds__(256) k_cond_panels(NullModel nm, CondArgs a, double* __restrict__ P, int64_t ldp, double rho_min,
                                                     int* __restrict__ list) {
  constexpr int NA = CT * (CT + 1) / 2;
  extern __shared__ __attribute__((aligned(16))) double sh[];
  const int n = a.n, npad = a.npad, c = a.c, s = a.s;
  double* sLam = sh;
  double* sZ = sh + n;
  for (int e = threadIdx.x; e < n; e += blockDim.x) sLam[e] = a.lam[e];
  for (int e = threadIdx.x; e < n * c; e += blockDim.x) sZ[e] = a.Z0[e];
  __syncthreads();
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ldp) return;
  const int64_t pstride = (int64_t)npad * ldp;
  constexpr int NPAN = 2 + CT;
  const int rj = j < a.m ? a.nk[j] : 0;
  if (j >= a.m || rj < 0) {   // padding columns: zero; a trait with an index out of range: NaN numerators, unit weights
    const double p0 = (j < a.m) ? NAN : 0.0, p1 = (j < a.m) ? 1.0 : 0.0;
    for (int k = 0; k < npad; ++k) {
      P[(int64_t)k * ldp + j] = k < n ? p0 : 0.0;
      P[pstride + (int64_t)k * ldp + j] = k < n ? p1 : 0.0;
      for (int q = 2; q < NPAN; ++q) P[q * pstride + (int64_t)k * ldp + j] = 0.0;
    }
    return;
  }
  const int ct = c + rj;
  const int64_t yj = a.act ? a.act[j] : j;   // the column's trait in Yt
  int kc[COND_SMAX];
#pragma unroll
  for (int e = 0; e < COND_SMAX; ++e) kc[e] = (e < rj && e < s) ? a.kept[j * s + e] : 0;
  auto row = [&](double (&z)[CT], int k) {
#pragma unroll
    for (int q = 0; q < CT; ++q) {
      double v = 0.0;
      if (q < c) v = sZ[q * n + k];
      else if (q < ct) {
        int col = 0;
#pragma unroll
        for (int e = 0; e < COND_SMAX; ++e) if (e == q - c) col = kc[e];
        v = a.Xt[(int64_t)k * a.ldx + col];
      }
      z[q] = v;
    }
  };
  const double h2 = a.h2[j];
  const double delta = h2 / (1.0 - h2);
  double A[NA], v[CT], syy = 0.0;
#pragma unroll
  for (int e = 0; e < NA; ++e) A[e] = 0.0;
#pragma unroll
  for (int q = 0; q < CT; ++q) v[q] = 0.0;
  for (int k = 0; k < n; ++k) {
    const double w = fabs(1.0 / fma(delta, sLam[k], 1.0));
    const double y = a.Yt[(int64_t)k * a.ldy + yj];
    const double wy = w * y;
    syy = fma(wy, y, syy);
    double z[CT];
    row(z, k);
#pragma unroll
    for (int q = 0; q < CT; ++q) {
      v[q] = fma(wy, z[q], v[q]);
      const double wz = w * z[q];
#pragma unroll
      for (int r = 0; r <= q; ++r) A[q * (q + 1) / 2 + r] = fma(wz, z[r], A[q * (q + 1) / 2 + r]);
    }
  }
  double L[NA], Li[NA], t[CT], beta[CT], tt = 0.0, rho = 1.0;
#pragma unroll
  for (int q = 0; q < CT; ++q) {
    const bool live = q < ct;
#pragma unroll
    for (int r = 0; r <= q; ++r) {
      double sacc = A[q * (q + 1) / 2 + r];
#pragma unroll
      for (int u = 0; u < r; ++u) sacc = fma(-L[q * (q + 1) / 2 + u], L[r * (r + 1) / 2 + u], sacc);
      if (r == q) {
        if (live) {
          const double share = sacc / A[q * (q + 1) / 2 + q];
          rho = (share < rho || !(share == share)) ? share : rho;   // NaN sticks (k_illcond_flag)
        }
        L[q * (q + 1) / 2 + q] = live ? sqrt(sacc) : 1.0;
      } else {
        L[q * (q + 1) / 2 + r] = live ? sacc / L[r * (r + 1) / 2 + r] : 0.0;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < CT; ++q) {
#pragma unroll
    for (int r = 0; r <= q; ++r) {
      double sacc = (r == q) ? 1.0 : 0.0;
#pragma unroll
      for (int u = r; u < q; ++u) sacc = fma(-L[q * (q + 1) / 2 + u], Li[u * (u + 1) / 2 + r], sacc);
      Li[q * (q + 1) / 2 + r] = sacc / L[q * (q + 1) / 2 + q];
    }
    double sacc = 0.0;
#pragma unroll
    for (int r = 0; r <= q; ++r) sacc = fma(Li[q * (q + 1) / 2 + r], v[r], sacc);
    t[q] = sacc;
    tt = fma(sacc, sacc, tt);
  }
#pragma unroll
  for (int q = 0; q < CT; ++q) {
    double sacc = 0.0;
#pragma unroll
    for (int u = q; u < CT; ++u) sacc = fma(Li[u * (u + 1) / 2 + q], t[u], sacc);
    beta[q] = sacc;
  }
  const double yy = syy - tt;
  if (!(sqrt(fabs(yy)) > 2.220446049250313e-16)) atomicAdd((unsigned long long*)&a.stat[ST_ZERO_NORM], 1ull);
  const double isy = 1.0 / sqrt(yy);
  // the conditioning guard (a design of >= 2 columns): the trait goes on the list of k_cond_qr
  int flagged = 0;
  if (ct >= 2 && !(rho >= rho_min)) {
    const unsigned long long slot = atomicAdd((unsigned long long*)&a.stat[ST_ILLCOND], 1ull);
    list[slot] = (int)j;
    flagged = 1;
  }
  a.flag[j] = flagged;
  for (int k = 0; k < npad; ++k) {
    double p0 = 0.0, w = 0.0;
    double zl[CT];
#pragma unroll
    for (int q = 0; q < CT; ++q) zl[q] = 0.0;
    if (k < n) {
      w = fabs(1.0 / fma(delta, sLam[k], 1.0));
      double z[CT];
      row(z, k);
      double res = a.Yt[(int64_t)k * a.ldy + yj];
#pragma unroll
      for (int q = 0; q < CT; ++q) res = fma(-beta[q], z[q], res);
      p0 = w * res * isy;
#pragma unroll
      for (int q = 0; q < CT; ++q) {
        double sacc = 0.0;
#pragma unroll
        for (int r = 0; r <= q; ++r) sacc = fma(Li[q * (q + 1) / 2 + r], z[r], sacc);
        zl[q] = w * sacc;
      }
    }
    P[(int64_t)k * ldp + j] = p0;
    P[pstride + (int64_t)k * ldp + j] = w;
#pragma unroll
    for (int q = 0; q < CT; ++q) P[(2 + q) * pstride + (int64_t)k * ldp + j] = zl[q];
  }
}

// ---- the guard's re-scan: ortho_basis.h's front on the per-trait design, one column per test ------------------------------------------
constexpr int COND_CT = BLMM_MULTIDF_MAX_COVARIATES;
// One workgroup per listed trait at a time; buf: (CTmax + 2) n doubles (sqrt weights, the orthonormal basis, the unit trait residual)
// RED (blmm_bulkscan_stepwise): there is no L.  The listed columns item0 .. item0 + nitem - 1 go to the columns 0 .. nitem - 1 of a
// compact scratch (L, ld ldL) for k_mdf_flag_red, as k_mdf_qr<K, RED> does it.
template <bool RED>
__global__ void __launch_bounds__(256) k_cond_qr(CondArgs a, int ctmax, const int* __restrict__ list, double* slab,
                                                 double* __restrict__ L, int64_t ldL, int64_t item0, int64_t nitem) {
  extern __shared__ __attribute__((aligned(16))) double sh[];
  __shared__ double s_red[4];
  int64_t cnt = a.stat[ST_ILLCOND];
  if (RED && cnt > item0 + nitem) cnt = item0 + nitem;
  if (cnt <= 0) return;
  const int n = a.n, c = a.c, s = a.s;
  double* buf = slab ? slab + (size_t)blockIdx.x * (size_t)(ctmax + 2) * n : sh;
  double* Sw = buf;
  double* Qb = buf + n;
  double* yb = buf + (size_t)(1 + ctmax) * n;
  const double scale = -0.5 * (double)n;
  int nnan = 0, nrule = 0;
  for (int64_t item = (RED ? item0 : 0) + blockIdx.x; item < cnt; item += gridDim.x) {
    const int64_t j = list[item];
    const int64_t yj = a.act ? a.act[j] : j;
    double* __restrict__ out = L + (RED ? item - item0 : j) * ldL;
    const int ct = c + a.nk[j];
    const int* kj = a.kept + j * s;
    auto col = [&](int q, int k) { return q < c ? a.Z0[(size_t)q * n + k] : a.Xt[(int64_t)k * a.ldx + kj[q - c]]; };
    const double nn = weighted_basis<256, 1>(n, ct, a.h2[j], a.lam, col, a.Yt + yj, a.ldy, Sw, Qb, yb, s_red);
    const double inv = 1.0 / sqrt(nn);
    for (int k = threadIdx.x; k < n; k += 256) yb[k] *= inv;
    __syncthreads();
    for (int64_t i = threadIdx.x; i < a.p; i += 256) {
      double t[COND_CT];
      ortho_coeffs<COND_CT>(Sw, Qb, n, ct, a.Xt + i, a.ldx, t);
      double xx = 0.0, d0 = 0.0, num = 0.0;
      for (int k = 0; k < n; ++k) {
        const double x = Sw[k] * a.Xt[(int64_t)k * a.ldx + i];
        d0 = fma(x, x, d0);
        double v = x;
#pragma unroll
        for (int q = 0; q < COND_CT; ++q)
          if (q < ct) v = fma(-t[q], Qb[(size_t)q * n + k], v);
        xx = fma(v, v, xx);
        num = fma(v, yb[k], num);
      }
      double lod;
      if (!(xx > MDF_TAU * d0)) { lod = 0.0; ++nrule; }
      else {
        const double u1 = 1.0 - (num * num) / xx;
        lod = scale * log10(u1);
        if (!(u1 > 0.0)) { lod = (u1 == 0.0) ? INFINITY : NAN; nnan += (u1 == 0.0) ? 0 : 1; }
      }
      out[i] = lod;
    }
  }
  if (nnan) atomicAdd((unsigned long long*)&a.stat[ST_NAN_LOD], (unsigned long long)nnan);
  if (nrule) atomicAdd((unsigned long long*)&a.info[0], (unsigned long long)nrule);
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------
int launch_cond_null(blmm_ctx* ctx, const NullModel& nm, const CondArgs& a, const double* grid_dev, int ngrid) {
  if (a.m <= 0) return BLMM_OK;
  const size_t lds = sizeof(double) * (size_t)a.n * (1 + a.s);
#define CN(CT) do { if (lds > 48 * 1024) BLMM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cond_null<CT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
    hipLaunchKernelGGL(k_cond_null<CT>, dim3((unsigned)a.m), dim3(64), lds, ctx->stream, nm, a, grid_dev, ngrid); } while (0)
  switch (a.c + a.s) {
    BLMM_FOR_EACH_C(CN)
    default: return fail(ctx, BLMM_ERR_UNSUPPORTED, "bulkscan_cond: 1 .. 8 null-design columns");
  }
#undef CN
  KCHECK();
  return BLMM_OK;
}

int launch_cond_panels(blmm_ctx* ctx, const NullModel& nm, const CondArgs& a, double* panels, int64_t ldp, double rho_min, int* list) {
  const unsigned blocks = (unsigned)((ldp + 255) / 256);
  const size_t lds = sizeof(double) * (size_t)a.n * (1 + a.c);
#define CP(CT) do { if (lds > 48 * 1024) BLMM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cond_panels<CT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
    hipLaunchKernelGGL(k_cond_panels<CT>, dim3(blocks), dim3(256), lds, ctx->stream, nm, a, panels, ldp, rho_min, list); } while (0)
  switch (a.c + a.s) {
    BLMM_FOR_EACH_C(CP)
    default: return fail(ctx, BLMM_ERR_UNSUPPORTED, "bulkscan_cond: 1 .. 8 null-design columns");
  }
#undef CP
  KCHECK();
  return BLMM_OK;
}

int launch_cond_qr(blmm_ctx* ctx, const NullModel& nm, const CondArgs& a, const int* list, double* L, int64_t ldL, double* scr,
                   int64_t item0, int64_t nitem) {
  const int ctmax = a.c + a.s;
  if (a.p <= 0 || ctmax < 2 || (scr && nitem <= 0)) return BLMM_OK;
  size_t lds; double* slab; unsigned grid;
  if (int rc = qr_workspace(ctx, ctmax, nm.n, &lds, &slab, &grid)) return rc;
#define QR(RED, OUT, LD) do { if (lds > 48 * 1024) BLMM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cond_qr<RED>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
    hipLaunchKernelGGL(k_cond_qr<RED>, dim3(grid), dim3(256), lds, ctx->stream, a, ctmax, list, slab, OUT, LD, item0, nitem); } while (0)
  if (scr) QR(true, scr, a.p); else QR(false, L, ldL);
#undef QR
  KCHECK();
  return BLMM_OK;
}

// ---- blmm_bulkscan_stepwise: the caller's tables and the active list between the rounds ----------------------------------------------
__global__ void __launch_bounds__(256) k_step_init(StepArgs s) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= s.m) return;
  for (int t = 0; t <= s.S; ++t) { s.lod[j * (s.S + 1) + t] = NAN; s.arg[j * (s.S + 1) + t] = -1; s.h2[j * (s.S + 1) + t] = NAN; }
  for (int e = 0; e < s.S; ++e) s.loci[j * s.S + e] = -1;
  s.nloci[j] = 0;
}

// One workgroup walks the round's nact columns (act == nullptr: column jj is trait jj) with a running offset, so the next list is
// in ascending trait order whatever the launch.  Column jj's (mx, arg, h2) go to slot t of trait j's rows; a trait whose maximum is
// above the threshold (strictly; never in round S) gets the marker as its locus t and stays on the list.  Then the work counters:
// w[0] = the next round's traits; the guard's list length is added to w[1] and zeroed for the next round's k_cond_panels;
// n_zero_norm stays what round 0 counted (w[2]).
__global__ void __launch_bounds__(1024) k_step_update(StepArgs s, int t, int64_t nact, const int* __restrict__ act, int* __restrict__ next,
                                                      const double* __restrict__ mx, const int64_t* __restrict__ arg,
                                                      const double* __restrict__ h2, int64_t* __restrict__ stat) {
  __shared__ int s_cnt[16];
  __shared__ int64_t s_base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_base = 0;
  __syncthreads();
  for (int64_t j0 = 0; j0 < nact; j0 += 1024) {
    const int64_t jj = j0 + threadIdx.x;
    bool sel = false;
    int64_t j = -1;
    if (jj < nact) {
      j = act ? act[jj] : jj;
      const double v = mx[jj];
      const int64_t ai = arg[jj];
      s.lod[j * (s.S + 1) + t] = v; s.arg[j * (s.S + 1) + t] = ai; s.h2[j * (s.S + 1) + t] = h2[jj];
      sel = t < s.S && v > s.thr;
      if (sel) { s.loci[j * s.S + t] = ai; s.nloci[j] = t + 1; }
    }
    const unsigned long long b = __ballot(sel);
    if (lane == 0) s_cnt[wave] = __builtin_popcountll(b);
    __syncthreads();
    int64_t at = s_base + __builtin_popcountll(b & ((1ull << lane) - 1ull));
    int tot = 0;
    for (int w = 0; w < 16; ++w) { at += w < wave ? s_cnt[w] : 0; tot += s_cnt[w]; }
    if (sel) next[at] = (int)j;
    __syncthreads();
    if (threadIdx.x == 0) s_base += tot;
    __syncthreads();
  }
  // Between the rounds the status block is not the caller's: ST_ILLCOND is zero and ST_ZERO_NORM is the current round's until
  // k_step_finish puts the sums back.  A call that fails in between returns its error and no status, so nobody reads that state.
  if (threadIdx.x == 0) {
    s.w[0] = s_base;
    s.w[1] += stat[ST_ILLCOND]; stat[ST_ILLCOND] = 0;
    if (t == 0) { s.w[2] = stat[ST_ZERO_NORM]; s.w[3] = s_base; }
    else stat[ST_ZERO_NORM] = s.w[2];
  }
}

// the end of the call: the guard's count back into the status block, the caller's info block
__global__ void k_step_finish(StepArgs s, StepRounds r, const int64_t* __restrict__ cinfo, int64_t* __restrict__ stat,
                              int64_t* __restrict__ sinfo) {
  stat[ST_ILLCOND] = s.w[1];
  if (!sinfo) return;
  sinfo[0] = r.rounds; sinfo[1] = s.w[3]; sinfo[2] = cinfo[0];
  for (int t = 0; t < 5; ++t) sinfo[3 + t] = r.nact[t];
}

int launch_step_init(blmm_ctx* ctx, const StepArgs& s) {
  if (s.m <= 0) return BLMM_OK;
  hipLaunchKernelGGL(k_step_init, dim3((unsigned)((s.m + 255) / 256)), dim3(256), 0, ctx->stream, s);
  KCHECK();
  return BLMM_OK;
}

int launch_step_update(blmm_ctx* ctx, const StepArgs& s, int t, int64_t nact, const int* act, int* next, const double* mx,
                       const int64_t* arg, const double* h2, int64_t* stat) {
  hipLaunchKernelGGL(k_step_update, dim3(1), dim3(1024), 0, ctx->stream, s, t, nact, act, next, mx, arg, h2, stat);
  KCHECK();
  return BLMM_OK;
}

int launch_step_finish(blmm_ctx* ctx, const StepArgs& s, const StepRounds& r, const int64_t* cinfo, int64_t* stat, int64_t* sinfo) {
  hipLaunchKernelGGL(k_step_finish, dim3(1), dim3(1), 0, ctx->stream, s, r, cinfo, stat, sinfo);
  KCHECK();
  return BLMM_OK;
}

}  // namespace blmm
