// kernels_bperm.hip -- the permutation test for every trait of a bulk call (blmm_bulkscan_perms; the reference's
// scan_perms_lite, src/scan.jl:485-557, run once per trait under the trait's own null heritability) with only its reductions
// leaving the device: the p x m x nperms LOD tensor (2 TB at BXD size with 1000 permutations) is never written.
//
// A chunk of traits [j0, j0 + mt) becomes mt * (nperms + 1) panel columns, column jj (nperms + 1) + b = trait j0 + jj under
// permutation b - 1 (b = 0: the trait itself).  The arithmetic of a column is the single-trait panel's (kernels_prep.hip:
// k_perm_r0 / k_perm_panel for n <= 256, k_perm_r0_wg / k_perm_coef / k_perm_fill beyond), statement for statement, so that
// trait j's columns are those blmm_scan_perms builds for Y[:, j] bit for bit.  The shared-weights table kernel then scans the
// chunk with bin[column] = trait (marker norms of the trait's h2: launch_isx with the chunk's h2 as its "grid") and reduces in
// its epilogue (RedArgs + k_red_final), and k_bperm_summary turns every trait's nperms + 1 column maxima into the peak, the
// thresholds (k_quantiles' rule on k_bitonic_lds' order) and the empirical p-value.
//
// blmm_bulkscan_loco_perms runs the same chunks once per chromosome (its column block of G, its LOCO kinship's eigenbasis and h2),
// with one permutation set for every chromosome.  k_bperm_summary writes each chromosome's tables into its slot (marker indices
// shifted to global ones by row0), and k_bperm_loco_merge folds the chunk's column maxima into a genome-wide (nperms + 1) x m buffer,
// which one more k_bperm_summary turns into the genome-wide tables.  Convention: the genome-wide maximum of permutation b pairs
// the chromosomes' copies by b -- each chromosome permutes its own rotated, reweighted null residuals, as scan_perms_lite does under
// that chromosome's kinship; it is not one permutation of the individuals carried across chromosomes.
#include "blmm_internal.h"
#include <cmath>
#include <cstring>

namespace blmm {

#define KCHECK()                                                                                      \
  do {                                                                                                \
    hipError_t e__ = hipGetLastError();                                                               \
    if (e__ != hipSuccess) return fail(ctx, BLMM_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e__)); \
  } while (0)

// C x C Cholesky solve A beta = g (A packed lower), the operation order of k_perm_panel / k_perm_r0 / k_perm_coef
template <int C>
__device__ __forceinline__ void bperm_solve(const double (&A)[C * (C + 1) / 2], const double (&g)[C], double (&beta)[C]) {
  constexpr int NA = C * (C + 1) / 2;
  double L[NA], t[C];
  for (int q = 0; q < C; ++q) {
    for (int r = 0; r <= q; ++r) {
      double s = A[q * (q + 1) / 2 + r];
      for (int u = 0; u < r; ++u) s = fma(-L[q * (q + 1) / 2 + u], L[r * (r + 1) / 2 + u], s);
      L[q * (q + 1) / 2 + r] = (r == q) ? sqrt(s) : s / L[r * (r + 1) / 2 + r];
    }
    double s = g[q];
    for (int u = 0; u < q; ++u) s = fma(-L[q * (q + 1) / 2 + u], t[u], s);
    t[q] = s / L[q * (q + 1) / 2 + q];
  }
  for (int q = C - 1; q >= 0; --q) {
    double s = t[q];
    for (int u = q + 1; u < C; ++u) s = fma(-L[u * (u + 1) / 2 + q], beta[u], s);
    beta[q] = s / L[q * (q + 1) / 2 + q];
  }
}

// r0_j = sqrt(w_j) .* (y0_j - Z0 b_j) of the chunk's traits (k_perm_r0's serial sums): one thread per trait
template <int C>
__global__ void __launch_bounds__(64) k_bperm_r0(NullModel nm, const double* __restrict__ Yt, int64_t ldy, const double* __restrict__ Z0,
                                                 const double* __restrict__ lam, const double* __restrict__ h2c, int64_t mt,
                                                 double* __restrict__ r0buf) {
  const int64_t jj = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (jj >= mt) return;
  const int n = nm.n;
  constexpr int NA = C * (C + 1) / 2;
  const double h2 = h2c[jj];
  const double delta = h2 / (1.0 - h2);
  const double* y = Yt + jj;
  double A[NA], g[C], beta[C];
  for (int a = 0; a < NA; ++a) A[a] = 0.0;
  for (int q = 0; q < C; ++q) g[q] = 0.0;
  for (int k = 0; k < n; ++k) {
    const double w = 1.0 / fma(delta, lam[k], 1.0);
    const double yk = y[(int64_t)k * ldy];
    for (int q = 0; q < C; ++q) {
      const double wz = w * Z0[q * n + k];
      g[q] = fma(wz, yk, g[q]);
      for (int r = 0; r <= q; ++r) A[q * (q + 1) / 2 + r] = fma(wz, Z0[r * n + k], A[q * (q + 1) / 2 + r]);
    }
  }
  bperm_solve<C>(A, g, beta);
  double* r0 = r0buf + jj * n;
  for (int k = 0; k < n; ++k) {
    const double w = 1.0 / fma(delta, lam[k], 1.0);
    double v = y[(int64_t)k * ldy];
    for (int q = 0; q < C; ++q) v = fma(-beta[q], Z0[q * n + k], v);
    r0[k] = sqrt(w) * v;
  }
}

// ... k_perm_r0_wg's sums (256 threads, four waves folded in a fixed order): one workgroup per trait
template <int C>
__global__ void __launch_bounds__(256) k_bperm_r0_wg(NullModel nm, const double* __restrict__ Yt, int64_t ldy,
                                                     const double* __restrict__ Z0, const double* __restrict__ lam,
                                                     const double* __restrict__ h2c, double* __restrict__ r0buf) {
  constexpr int NA = C * (C + 1) / 2;
  __shared__ double s_part[NA + C][4], s_beta[C];
  const int64_t jj = blockIdx.x;
  const int n = nm.n, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const double h2 = h2c[jj];
  const double delta = h2 / (1.0 - h2);
  const double* y = Yt + jj;
  double A[NA], g[C];
  for (int a = 0; a < NA; ++a) A[a] = 0.0;
  for (int q = 0; q < C; ++q) g[q] = 0.0;
  for (int k = t; k < n; k += 256) {
    const double w = 1.0 / fma(delta, lam[k], 1.0);
    const double yk = y[(int64_t)k * ldy];
    for (int q = 0; q < C; ++q) {
      const double wz = w * Z0[q * n + k];
      g[q] = fma(wz, yk, g[q]);
      for (int r = 0; r <= q; ++r) A[q * (q + 1) / 2 + r] = fma(wz, Z0[r * n + k], A[q * (q + 1) / 2 + r]);
    }
  }
  for (int a = 0; a < NA + C; ++a) {
    double v = (a < NA) ? A[a] : g[a - NA];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) s_part[a][wave] = v;
  }
  __syncthreads();
  if (t == 0) {
    for (int a = 0; a < NA; ++a) A[a] = (s_part[a][0] + s_part[a][1]) + (s_part[a][2] + s_part[a][3]);
    for (int q = 0; q < C; ++q) g[q] = (s_part[NA + q][0] + s_part[NA + q][1]) + (s_part[NA + q][2] + s_part[NA + q][3]);
    double beta[C];
    bperm_solve<C>(A, g, beta);
    for (int q = 0; q < C; ++q) s_beta[q] = beta[q];
  }
  __syncthreads();
  double* r0 = r0buf + jj * n;
  for (int k = t; k < n; k += 256) {
    const double w = 1.0 / fma(delta, lam[k], 1.0);
    double v = y[(int64_t)k * ldy];
    for (int q = 0; q < C; ++q) v = fma(-s_beta[q], Z0[q * n + k], v);
    r0[k] = sqrt(w) * v;
  }
}

// Column -> (trait of the chunk, permutation; b = 0: the trait itself).  perm: n x nperms, column b - 1 = permutation b.
struct BpermCol { int64_t jj; int64_t b; };
__device__ __forceinline__ BpermCol bperm_col(int64_t col, int64_t np1) { BpermCol c; c.jj = col / np1; c.b = col - c.jj * np1; return c; }

// k_perm_panel's column (one thread, serial sums over the n rows): n <= 256
template <int C>
__global__ void __launch_bounds__(64) k_bperm_panel(NullModel nm, const double* __restrict__ Z0, const double* __restrict__ lam,
                                                    const double* __restrict__ h2c, const int32_t* __restrict__ perm, int64_t np1,
                                                    int64_t ncols, const double* __restrict__ r0buf, double* __restrict__ P,
                                                    int64_t ldp, int64_t* stat) {
  const int n = nm.n, npad = nm.npad;
  const int64_t col = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= ldp) return;
  if (col >= ncols) {
    for (int k = 0; k < npad; ++k) P[(int64_t)k * ldp + col] = 0.0;
    return;
  }
  const BpermCol cc = bperm_col(col, np1);
  const bool orig = cc.b == 0;
  const int32_t* pc = orig ? nullptr : perm + (cc.b - 1) * (int64_t)n;
  const double* r0 = r0buf + cc.jj * n;
  constexpr int NA = C * (C + 1) / 2;
  const double h2 = h2c[cc.jj];
  const double delta = h2 / (1.0 - h2);
  double A[NA], g[C], beta[C];
  for (int a = 0; a < NA; ++a) A[a] = 0.0;
  for (int q = 0; q < C; ++q) g[q] = 0.0;
  double rr = 0.0;
  for (int k = 0; k < n; ++k) {
    const double w = 1.0 / fma(delta, lam[k], 1.0);
    const double sw = sqrt(w);
    const int src = orig ? k : pc[k];
    const double v = r0[src];
    rr = fma(v, v, rr);
    for (int q = 0; q < C; ++q) {
      const double zq = sw * Z0[q * n + k];
      g[q] = fma(zq, v, g[q]);
      for (int r = 0; r <= q; ++r) A[q * (q + 1) / 2 + r] = fma(zq, sw * Z0[r * n + k], A[q * (q + 1) / 2 + r]);
    }
  }
  bperm_solve<C>(A, g, beta);
  const double inr = 1.0 / sqrt(rr);
  if (orig && !(sqrt(rr) > 2.220446049250313e-16)) atomicAdd((unsigned long long*)&stat[ST_ZERO_NORM], 1ull);
  for (int k = 0; k < npad; ++k) {
    double out = 0.0;
    if (k < n) {
      const double w = 1.0 / fma(delta, lam[k], 1.0);
      const double sw = sqrt(w);
      const int src = orig ? k : pc[k];
      double v = r0[src];
      for (int q = 0; q < C; ++q) v = fma(-beta[q], sw * Z0[q * n + k], v);
      out = sw * v * inr;
    }
    P[(int64_t)k * ldp + col] = out;
  }
}

// k_perm_coef's column (one wave, lane-strided sums folded by xor shuffles): n > 256.  coef[col][C + 1] = {beta, 1 / ||v||}
template <int C>
__global__ void __launch_bounds__(256) k_bperm_coef(NullModel nm, const double* __restrict__ Z0, const double* __restrict__ lam,
                                                    const double* __restrict__ h2c, const int32_t* __restrict__ perm, int64_t np1,
                                                    int64_t ncols, const double* __restrict__ r0buf, double* __restrict__ coef,
                                                    int64_t* stat) {
  constexpr int NA = C * (C + 1) / 2;
  const int n = nm.n, lane = threadIdx.x & 63;
  const int64_t col = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (col >= ncols) return;
  const BpermCol cc = bperm_col(col, np1);
  const bool orig = cc.b == 0;
  const int32_t* pc = orig ? nullptr : perm + (cc.b - 1) * (int64_t)n;
  const double* r0 = r0buf + cc.jj * n;
  const double h2 = h2c[cc.jj];
  const double delta = h2 / (1.0 - h2);
  double A[NA], g[C], rr = 0.0;
  for (int a = 0; a < NA; ++a) A[a] = 0.0;
  for (int q = 0; q < C; ++q) g[q] = 0.0;
  for (int k = lane; k < n; k += 64) {
    const double w = 1.0 / fma(delta, lam[k], 1.0);
    const double sw = sqrt(w);
    const int src = orig ? k : pc[k];
    const double v = r0[src];
    rr = fma(v, v, rr);
    for (int q = 0; q < C; ++q) {
      const double zq = sw * Z0[q * n + k];
      g[q] = fma(zq, v, g[q]);
      for (int r = 0; r <= q; ++r) A[q * (q + 1) / 2 + r] = fma(zq, sw * Z0[r * n + k], A[q * (q + 1) / 2 + r]);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    rr += __shfl_xor(rr, o, 64);
    for (int a = 0; a < NA; ++a) A[a] += __shfl_xor(A[a], o, 64);
    for (int q = 0; q < C; ++q) g[q] += __shfl_xor(g[q], o, 64);
  }
  if (lane == 0) {
    double beta[C];
    bperm_solve<C>(A, g, beta);
    for (int q = 0; q < C; ++q) coef[col * (C + 1) + q] = beta[q];
    coef[col * (C + 1) + C] = 1.0 / sqrt(rr);
    if (orig && !(sqrt(rr) > 2.220446049250313e-16)) atomicAdd((unsigned long long*)&stat[ST_ZERO_NORM], 1ull);
  }
}

// k_perm_fill's column: P[k][col] = sqrt(w_k) (v_k - sum_q beta_q sqrt(w_k) z_qk) / ||v||, zero beyond ncols / n
template <int C>
__global__ void __launch_bounds__(256) k_bperm_fill(NullModel nm, const double* __restrict__ Z0, const double* __restrict__ lam,
                                                    const double* __restrict__ h2c, const int32_t* __restrict__ perm, int64_t np1,
                                                    int64_t ncols, const double* __restrict__ r0buf, const double* __restrict__ coef,
                                                    double* __restrict__ P, int64_t ldp) {
  const int n = nm.n, npad = nm.npad;
  const int64_t col = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
  const int k0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * 16;
  if (col >= ldp) return;
  const bool live = col < ncols;
  BpermCol cc = {0, 0};
  if (live) cc = bperm_col(col, np1);
  const bool orig = cc.b == 0;
  const int32_t* pc = orig ? nullptr : perm + (cc.b - 1) * (int64_t)n;
  const double* r0 = r0buf + cc.jj * n;
  const double h2 = live ? h2c[cc.jj] : 0.0;
  const double delta = h2 / (1.0 - h2);
  double beta[C], inr = 0.0;
  for (int q = 0; q < C; ++q) beta[q] = live ? coef[col * (C + 1) + q] : 0.0;
  if (live) inr = coef[col * (C + 1) + C];
  for (int k = k0; k < k0 + 16 && k < npad; ++k) {
    double out = 0.0;
    if (live && k < n) {
      const double w = 1.0 / fma(delta, lam[k], 1.0);
      const double sw = sqrt(w);
      const int src = orig ? k : pc[k];
      double v = r0[src];
      for (int q = 0; q < C; ++q) v = fma(-beta[q], sw * Z0[q * n + k], v);
      out = sw * v * inr;
    }
    P[(int64_t)k * ldp + col] = out;
  }
}

__global__ void k_bperm_bin(int64_t ncols, int64_t np1, int* __restrict__ bin) {
  const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (col < ncols) bin[col] = (int)(col / np1);
}

int launch_bperm_panels(blmm_ctx* ctx, const NullModel& nm, const double* Yt, int64_t ldy, const double* Z0, const double* lam,
                        const double* h2c, int64_t mt, const int32_t* perm, int64_t nperms, double* panel, int64_t ldp, int* bin,
                        int64_t* stat) {
  if (nm.c < 1 || nm.c > CTPL) return fail(ctx, BLMM_ERR_UNSUPPORTED, "bulkscan_perms: more than 8 null covariates (incl. intercept) are not supported");
  const int64_t np1 = nperms + 1, ncols = mt * np1;
  int rc = ensure(ctx, ctx->r0, sizeof(double) * (size_t)nm.n * (size_t)mt);
  if (rc) return rc;
  double* r0 = ptr<double>(ctx->r0);
  // the single-trait path's choice (launch_perm_panel), BLMM_PERM_PATH included, so that a trait's columns are its panel's
  const char* path_env = dev_env("BLMM_PERM_PATH");
  const bool newpath = path_env ? std::strcmp(path_env, "new") == 0 : nm.n > 256;
  double* coef = nullptr;
  if (newpath) {
    if ((rc = ensure(ctx, ctx->tmpB, sizeof(double) * (size_t)ncols * (CMAX + 1) + 64))) return rc;
    coef = ptr<double>(ctx->tmpB);
  }
  hipLaunchKernelGGL(k_bperm_bin, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, ctx->stream, ncols, np1, bin);
  KCHECK();
  const dim3 fgrid((unsigned)((ldp + 63) / 64), (unsigned)((nm.npad + 63) / 64));
#define BP(C)                                                                                                                  \
  if (newpath) {                                                                                                               \
    hipLaunchKernelGGL(k_bperm_r0_wg<C>, dim3((unsigned)mt), dim3(256), 0, ctx->stream, nm, Yt, ldy, Z0, lam, h2c, r0);        \
    hipLaunchKernelGGL(k_bperm_coef<C>, dim3((unsigned)((ncols + 3) / 4)), dim3(256), 0, ctx->stream, nm, Z0, lam, h2c, perm,  \
                       np1, ncols, r0, coef, stat);                                                                            \
    hipLaunchKernelGGL(k_bperm_fill<C>, fgrid, dim3(256), 0, ctx->stream, nm, Z0, lam, h2c, perm, np1, ncols, r0, coef, panel, ldp); \
  } else {                                                                                                                     \
    hipLaunchKernelGGL(k_bperm_r0<C>, dim3((unsigned)((mt + 63) / 64)), dim3(64), 0, ctx->stream, nm, Yt, ldy, Z0, lam, h2c, mt, r0); \
    hipLaunchKernelGGL(k_bperm_panel<C>, dim3((unsigned)((ldp + 63) / 64)), dim3(64), 0, ctx->stream, nm, Z0, lam, h2c, perm,  \
                       np1, ncols, r0, panel, ldp, stat);                                                                      \
  }
  switch (nm.c) {
    BLMM_FOR_EACH_C(BP)
    default: return fail(ctx, BLMM_ERR_UNSUPPORTED, BLMM_C_ERR);
  }
#undef BP
  KCHECK();
  return BLMM_OK;
}

// ---- per-trait summary: one workgroup per trait of the chunk ---------------------------------------------------------------
// mx / arg: the chunk's column maxima and their markers (k_red_final).  The nperms permutation maxima are sorted in LDS by
// k_bitonic_lds' network (same key order -- NaN last -- and +inf padding to npow), so the quantiles (k_quantiles' rule: Julia's
// default type 7) equal blmm_get_thresholds on the trait's L_perms bit for bit.  pval = (1 + #{b : max_b >= peak}) / (nperms + 1),
// a -inf maximum (no finite-comparable LOD) never counted.  row0 is added to every marker written (-1 stays -1); lod_max /
// lod_argmax may be NULL.
__global__ void __launch_bounds__(256) k_bperm_summary(const double* __restrict__ mx, const int64_t* __restrict__ arg, int64_t nperms,
                                                       int npow, BpermProbs probs, int nprobs, int64_t j0, int64_t row0,
                                                       double* __restrict__ lod_max, int64_t* __restrict__ lod_argmax,
                                                       double* __restrict__ max_perms, double* __restrict__ thr,
                                                       double* __restrict__ pval) {
  extern __shared__ double sv[];
  __shared__ unsigned long long s_cnt;
  const int64_t jj = blockIdx.x, j = j0 + jj, np1 = nperms + 1;
  const double* c = mx + jj * np1;
  const double peak = c[0];
  if (threadIdx.x == 0) {
    s_cnt = 0ull;
    if (lod_max) lod_max[j] = peak;
    if (lod_argmax) { const int64_t a = arg[jj * np1]; lod_argmax[j] = a >= 0 ? a + row0 : a; }
  }
  __syncthreads();
  unsigned long long my = 0;
  for (int e = threadIdx.x; e < npow; e += blockDim.x) {
    double v = INFINITY;
    if (e < nperms) {
      v = c[1 + e];
      if (max_perms) max_perms[j * nperms + e] = v;
      if (v >= peak && v != -INFINITY) ++my;
    }
    sv[e] = v;
  }
  if (my) atomicAdd(&s_cnt, my);
  __syncthreads();
  for (int k = 2; k <= npow; k <<= 1)
    for (int h = k >> 1; h > 0; h >>= 1) {
      for (int e = threadIdx.x; e < npow; e += blockDim.x) {
        const int x = e ^ h;
        if (x > e) {
          const double a = sv[e], b = sv[x];
          const bool up = (e & k) == 0;
          if (up ? key_less(b, a) : key_less(a, b)) { sv[e] = b; sv[x] = a; }
        }
      }
      __syncthreads();
    }
  const int t = threadIdx.x;
  if (t < nprobs && thr) {
    double out = NAN;
    if (nperms > 0) {
      double q = probs.v[t];
      q = q < 0.0 ? 0.0 : (q > 1.0 ? 1.0 : q);
      const double hq = (double)(nperms - 1) * q;
      const int64_t lo = (int64_t)floor(hq);
      const int64_t hi = lo + 1 < nperms ? lo + 1 : nperms - 1;
      const double a = sv[lo], b = sv[hi];
      out = quantile7_interp(a, b, hq - (double)lo);
    }
    thr[j * nprobs + t] = out;
  }
  if (t == 0 && pval) pval[j] = nperms > 0 ? (double)(1ull + s_cnt) / (double)np1 : NAN;
}

int launch_bperm_summary(blmm_ctx* ctx, const double* mx, const int64_t* arg, int64_t mt, int64_t nperms, const BpermProbs& probs,
                         int nprobs, int64_t j0, double* lod_max, int64_t* lod_argmax, double* max_perms, double* thr, double* pval,
                         int64_t row0) {
  if (mt <= 0) return BLMM_OK;
  int npow = 1;
  while (npow < nperms) npow <<= 1;
  const size_t lds = sizeof(double) * (size_t)npow;
  if (lds > 48 * 1024) BLMM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bperm_summary), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_bperm_summary, dim3((unsigned)mt), dim3(256), lds, ctx->stream, mx, arg, nperms, npow, probs, nprobs, j0,
                     row0, lod_max, lod_argmax, max_perms, thr, pval);
  KCHECK();
  return BLMM_OK;
}

// ---- blmm_bulkscan_loco_perms: a chunk's column maxima into the genome-wide buffer ------------------------------------------
// One thread per panel column: column col of the chunk (trait j0 + col / (nperms + 1)) is column j0 (nperms + 1) + col of gmx /
// garg.  k_red_final's rule: the larger value wins, an equal one only with a lower valid marker, so that NaN (never in mx: k_red_final
// does not keep one) is never the maximum and a tie goes to the lowest GLOBAL marker whatever order the chromosomes run in.  The
// chunk's markers are its chromosome's: row0 (its first marker) makes them global.  gmx / garg start at -inf / -1.
__global__ void __launch_bounds__(256) k_bperm_loco_merge(const double* __restrict__ mx, const int64_t* __restrict__ arg, int64_t ncols,
                                                          int64_t row0, double* __restrict__ gmx, int64_t* __restrict__ garg) {
  const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (col >= ncols) return;
  const double v = mx[col];
  const int64_t a = arg[col];
  const int64_t i = a >= 0 ? a + row0 : -1;
  const double best = gmx[col];
  const int64_t bi = garg[col];
  if (v > best || (v == best && i >= 0 && (bi < 0 || i < bi))) { gmx[col] = v; garg[col] = i; }
}

int launch_bperm_loco_merge(blmm_ctx* ctx, const double* mx, const int64_t* arg, int64_t ncols, int64_t row0, double* gmx, int64_t* garg) {
  if (ncols <= 0) return BLMM_OK;
  hipLaunchKernelGGL(k_bperm_loco_merge, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, ctx->stream, mx, arg, ncols, row0, gmx, garg);
  KCHECK();
  return BLMM_OK;
}

// gmx / garg = -inf / -1 (the merge's identity), n entries
__global__ void __launch_bounds__(256) k_bperm_loco_init(int64_t n, double* __restrict__ gmx, int64_t* __restrict__ garg) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n) { gmx[e] = -INFINITY; garg[e] = -1; }
}

int launch_bperm_loco_init(blmm_ctx* ctx, int64_t n, double* gmx, int64_t* garg) {
  if (n <= 0) return BLMM_OK;
  hipLaunchKernelGGL(k_bperm_loco_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n, gmx, garg);
  KCHECK();
  return BLMM_OK;
}

}  // namespace blmm
