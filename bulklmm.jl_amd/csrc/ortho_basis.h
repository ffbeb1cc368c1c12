// ortho_basis.h -- the Gram-Schmidt front of the QR-grade re-scans, written once: k_scan_qr (kernels_dyn.hip), k_mdf_qr
// (kernels_mdf.hip), k_cond_qr (kernels_cond.hip) and k_effects (kernels_effects.hip).
//
// With s = sqrt|1 / (1 + delta lambda)| a team of NT threads (a 256-thread workgroup, or one wave) builds an ORTHONORMAL basis of
// the weighted design columns s .* col_q by Gram-Schmidt with every projection done twice (backward stable like Householder QR:
// error ~ cond, not cond^2), and the trait's residual s .* y off that basis.  Thread t owns the rows t, t + NT, .. of every vector.
// Every sum has a fixed order, and each kernel keeps the order it was written with (its results do not change with the code
// that is shared):
//   NT     256: four waves folded through s_red as (s0 + s1) + (s2 + s3);  64: one wave, no barrier and no LDS
//   CHUNK  coefficients per reduction of project_out: classical Gram-Schmidt inside a chunk, modified across chunks
//   FAR    the wave's butterfly starts at lane ^ 32 (the plain __shfl_xor loop from 32 down to 1) instead of group_sum<64>'s
//          lane ^ 1: the same additions paired in another order, so other bits in the last place
#pragma once
#include "fastmath.h"

namespace blmm {

// Team-wide sums of the first nv of NV values per thread (the others must be zero in every thread); every thread gets the totals.
// s_red: [4][NV] doubles of LDS for NT == 256, unused for NT == 64.
template <int NT, int NV, bool FAR = false>
__device__ __forceinline__ void team_sum(double (&v)[NV], double* s_red, int nv = NV) {
  static_assert(NT == 64 || NT == 256, "one wave or four");
#pragma unroll
  for (int q = 0; q < NV; ++q)
    if (q < nv) {                               // nv is the same in every thread
      if constexpr (FAR) { for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_xor(v[q], off); }
      else v[q] = group_sum<64>(v[q]);
    }
  if constexpr (NT == 256) {
    const int w = threadIdx.x >> 6;
    __syncthreads();                            // the readers of the previous reduction are done with s_red
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int q = 0; q < NV; ++q) s_red[w * NV + q] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = (s_red[q] + s_red[NV + q]) + (s_red[2 * NV + q] + s_red[3 * NV + q]);
  }
}

template <int NT, bool FAR = false>
__device__ __forceinline__ double team_norm2(const double* v, int n, double* s_red) {
  double nn[1] = {0.0};
  for (int k = threadIdx.x; k < n; k += NT) nn[0] = fma(v[k], v[k], nn[0]);
  team_sum<NT, 1, FAR>(nn, s_red);
  return nn[0];
}

// Removes from column `tgt` (n doubles) its components along the columns Qb[0 .. nq) (orthonormal, or zero), CHUNK coefficients per
// reduction; coef (nq values, the same in every thread) += the components.
template <int NT, int CHUNK, bool FAR = false>
__device__ __forceinline__ void project_out(double* tgt, const double* Qb, int nq, int n, double* s_red, double* coef = nullptr) {
  for (int r0 = 0; r0 < nq; r0 += CHUNK) {
    double t[CHUNK];
#pragma unroll
    for (int u = 0; u < CHUNK; ++u) t[u] = 0.0;
    for (int k = threadIdx.x; k < n; k += NT) {
      const double v = tgt[k];
#pragma unroll
      for (int u = 0; u < CHUNK; ++u)
        if (r0 + u < nq) t[u] = fma(Qb[(size_t)(r0 + u) * n + k], v, t[u]);
    }
    team_sum<NT, CHUNK, FAR>(t, s_red, nq - r0);
    for (int k = threadIdx.x; k < n; k += NT) {
      double v = tgt[k];
#pragma unroll
      for (int u = 0; u < CHUNK; ++u)
        if (r0 + u < nq) v = fma(-t[u], Qb[(size_t)(r0 + u) * n + k], v);
      tgt[k] = v;
    }
    if (coef) {
#pragma unroll
      for (int u = 0; u < CHUNK; ++u)
        if (r0 + u < nq) coef[r0 + u] += t[u];
    }
  }
}

// The front itself, for the trait y (row k at y[k ldy]) with heritability h2 and the nc design columns col(q, k):
//   Sw <- sqrt.(abs.(makeweights(h2, lambda)))  (src/bulkscan_helpers.jl:138-141),  Qb <- the orthonormal basis (nc columns of n),
//   yb <- s .* y minus its components along Qb, NOT normalised: returns |yb|^2 (the same in every thread).
// NT == 256: one barrier before the fill (whoever read the buffers before has finished) -- after the caller's own last pass over
// its rows of yb it needs another before any thread reads rows it does not own.  NT == 64 needs neither: each lane only ever
// reads the rows it wrote itself.
template <int NT, int CHUNK, bool FAR = false, class Col>
__device__ __forceinline__ double weighted_basis(int n, int nc, double h2, const double* __restrict__ lam, Col col,
                                                 const double* __restrict__ y, int64_t ldy, double* Sw, double* Qb, double* yb,
                                                 double* s_red) {
  const double delta = h2 / (1.0 - h2);
  if constexpr (NT == 256) __syncthreads();
  for (int k = threadIdx.x; k < n; k += NT) {
    const double s = sqrt(fabs(1.0 / fma(delta, lam[k], 1.0)));
    Sw[k] = s;
    for (int q = 0; q < nc; ++q) Qb[(size_t)q * n + k] = s * col(q, k);
    yb[k] = s * y[(int64_t)k * ldy];
  }
  for (int q = 0; q < nc; ++q) {
    double* cq = Qb + (size_t)q * n;
    project_out<NT, CHUNK, FAR>(cq, Qb, q, n, s_red);
    project_out<NT, CHUNK, FAR>(cq, Qb, q, n, s_red);        // "twice is enough": orthogonal to rounding
    const double inv = 1.0 / sqrt(team_norm2<NT, FAR>(cq, n, s_red));
    for (int k = threadIdx.x; k < n; k += NT) cq[k] *= inv;
  }
  project_out<NT, CHUNK, FAR>(yb, Qb, nc, n, s_red);
  project_out<NT, CHUNK, FAR>(yb, Qb, nc, n, s_red);
  return team_norm2<NT, FAR>(yb, n, s_red);
}

// One thread, one marker column x (row k at x[k ldx]): the coefficients of s .* x along the nc <= CQ basis columns, from two
// passes -- t of the column itself, t2 of its first residual; t <- t + t2, for the caller's explicit residual pass.
template <int CQ>
__device__ __forceinline__ void ortho_coeffs(const double* Sw, const double* Qb, int n, int nc, const double* __restrict__ x,
                                             int64_t ldx, double (&t)[CQ]) {
  double t2[CQ];
#pragma unroll
  for (int q = 0; q < CQ; ++q) { t[q] = 0.0; t2[q] = 0.0; }
  for (int k = 0; k < n; ++k) {
    const double xk = Sw[k] * x[(int64_t)k * ldx];
#pragma unroll
    for (int q = 0; q < CQ; ++q)
      if (q < nc) t[q] = fma(Qb[(size_t)q * n + k], xk, t[q]);
  }
  for (int k = 0; k < n; ++k) {
    double xp = Sw[k] * x[(int64_t)k * ldx];
#pragma unroll
    for (int q = 0; q < CQ; ++q)
      if (q < nc) xp = fma(-t[q], Qb[(size_t)q * n + k], xp);
#pragma unroll
    for (int q = 0; q < CQ; ++q)
      if (q < nc) t2[q] = fma(Qb[(size_t)q * n + k], xp, t2[q]);
  }
#pragma unroll
  for (int q = 0; q < CQ; ++q) t[q] += t2[q];
}

}  // namespace blmm
