// kernels_mdf.hip -- the k-degree-of-freedom scan: one test per LOCUS, a span of k adjacent columns of G (blmm_bulkscan_multidf).
//
// Locus l is the columns l k .. l k + k - 1.  For trait j with weights w = |makeweights(h2_j)| and s = sqrt(w):
//   x~_a = s .* x0_a (the locus's rotated columns),  e~ = s .* (y0 - Z0 beta) / |s .* (y0 - Z0 beta)|  (unit norm, orthogonal to span(Z~))
//   b_a  = x~_a' e~                              = x_a' panel0_j              (k_panels' panel 0, kernels_prep.hip)
//   P_ab = x~_a' x~_b                            = (x_a .* x_b)' panel1_j     (panel 1 = w)
//   u_aq = x~_a' q~_q                            = x_a' panel(2+q)_j          (q~ = s .* Z0 L^-T: orthonormal basis of span(Z~))
//   S    = P - U U'   (Gram of the locus columns' residuals on span(Z~))
//   S    = L L' by an unpivoted Cholesky with the RANK RULE: column a is accepted iff its pivot (= |r_a|^2, the part of x~_a
//          orthogonal to span(Z~) and to the accepted columns before it) exceeds MDF_TAU |x~_a|^2 = MDF_TAU P_aa; a dropped column
//          gets a zero row and column of L
//   R^2  = |L^-1 b|^2 over the accepted columns,   LOD = -(n/2) log10(1 - R^2)   (scan_null's (-n/2)(log10 rss1 - log10 rss0))
// k = 1 is computeR_LMM's r^2 (kernels_scan.hip) through the same panels.
//
// The markers are rotated WITHOUT the centring projection of the 1-df path (R = U' Wd, not Q U' Wd: k_mdf_rawrot), because the
// rank rule compares against the norm of the rotated column itself; the statistic is the same either way.
//
//   null-grid  (weights shared per grid bin): k_mdf_table forms, per (bin g, locus l), T = L^-1 (packed k(k+1)/2, the rank rule
//              applied) from the bin's Gram; k_mdf_grid contracts b = X_l' panel0 for every (locus, trait) and its epilogue is
//              z = T[bin_j, l] b, R^2 = |z|^2.
//   permutations (blmm_bulkscan_multidf_perms): the null-grid kernels with the chunk's own h2 values as the "grid" and
//              bin[column] = the trait of the chunk, i.e. the null-grid algebra at every trait's exact heritability; the columns
//              are kernels_bperm.hip's panel columns (trait x permutation), and k_mdf_grid_red reduces every column to slot
//              partials (maximum, locus) in its epilogue instead of writing L.
//   null-exact (per-trait weights): k_mdf_exact accumulates b, P (from products x_a x_b formed in registers) and, one covariate
//              per pass, u_q -- folded into S at once -- then factors S per (locus, trait) in its epilogue.
//   reduced    (blmm_bulkscan_multidf_reduced): the traits' own columns through k_mdf_grid_red<.., SCAN> / k_mdf_exact_red -- slot
//              partials for k_red_final and the LOD > thr triplets, no L; flagged traits through k_mdf_qr's compact scratch and
//              k_mdf_flag_red.
//   guard      (null-exact, c >= 2, traits launch_illcond_flag listed: nearly collinear weighted covariates at h2 -> 1):
//              k_mdf_qr recomputes their columns with an orthonormal basis of span(Z~) from Gram-Schmidt with re-orthogonalisation
//              and explicit residuals (ortho_basis.h).
//
// Layout of the scan kernels: one wave = 64 consecutive loci (one per lane) x TJ traits; the traits are wave-uniform, so their
// panel values come in through scalar loads and every lane reuses them for its own locus (k vector loads per individual, k TJ
// FMAs for the grid form).  Four waves per workgroup share the loci (the Xt rows hit L1) and take four trait groups.
#include "blmm_internal.h"
#include "ortho_basis.h"
#include <cmath>

namespace blmm {

#define KCHECK()                                                                                      \
  do {                                                                                                \
    hipError_t e__ = hipGetLastError();                                                               \
    if (e__ != hipSuccess) return fail(ctx, BLMM_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e__)); \
  } while (0)

// ---- the per-(locus, trait) algebra ---------------------------------------------------------------------------------------------
// S (packed lower, row q at q (q + 1) / 2) -> its Cholesky factor with the rank rule against d0 (the raw norms |x~_a|^2), in place.
template <int K>
__device__ __forceinline__ void mdf_chol(double (&S)[K * (K + 1) / 2], const double (&d0)[K]) {
#pragma unroll
  for (int q = 0; q < K; ++q) {
#pragma unroll
    for (int r = 0; r <= q; ++r) {
      double s = S[q * (q + 1) / 2 + r];
#pragma unroll
      for (int u = 0; u < r; ++u) s = fma(-S[q * (q + 1) / 2 + u], S[r * (r + 1) / 2 + u], s);
      if (r == q) {
        S[q * (q + 1) / 2 + q] = (s > MDF_TAU * d0[q]) ? sqrt(s) : 0.0;   // NaN / not above the threshold: dropped
      } else {
        const double lrr = S[r * (r + 1) / 2 + r];
        S[q * (q + 1) / 2 + r] = (lrr > 0.0) ? s / lrr : 0.0;
      }
    }
  }
}
// |L^-1 b|^2 over the accepted columns (L from mdf_chol)
template <int K>
__device__ __forceinline__ double mdf_r2(const double (&Lc)[K * (K + 1) / 2], const double (&b)[K]) {
  double z[K], r2 = 0.0;
#pragma unroll
  for (int q = 0; q < K; ++q) {
    double s = b[q];
#pragma unroll
    for (int u = 0; u < q; ++u) s = fma(-Lc[q * (q + 1) / 2 + u], z[u], s);
    const double lqq = Lc[q * (q + 1) / 2 + q];
    z[q] = (lqq > 0.0) ? s / lqq : 0.0;
    r2 = fma(z[q], z[q], r2);
  }
  return r2;
}
// r2lod (src/bulkscan_helpers.jl:22-24) for the k-df R^2: 1 - R^2 = 0 -> +Inf; < 0 (R^2 > 1) or NaN -> NaN, counted when `valid`
__device__ __forceinline__ double mdf_lod(double r2, double scale, bool valid, int* nnan) {
  const double u = 1.0 - r2;
  if (u > 0.0) return scale * log10(u);
  if (u == 0.0) return INFINITY;
  *nnan += valid ? 1 : 0;
  return NAN;
}

// ---- the uncentred rotation  Rraw[i][k] = U[k][i] wd_i  (k_post_eigen's R with centered = 0), zero padded to npad x ldr --------
__global__ void __launch_bounds__(256) k_mdf_rawrot(const double* __restrict__ U, const double* __restrict__ wd, int n, int npad,
                                                    int ldr, double* __restrict__ R) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)npad * ldr) return;
  const int k = (int)(e % ldr), i = (int)(e / ldr);
  R[e] = (i < n && k < n) ? U[(size_t)k * n + i] * (wd ? wd[i] : 1.0) : 0.0;
}

int launch_mdf_rawrot(blmm_ctx* ctx, const double* U, const double* wd, int n, int npad, int ldr, double* R) {
  const int64_t tot = (int64_t)npad * ldr;
  hipLaunchKernelGGL(k_mdf_rawrot, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, U, wd, n, npad, ldr, R);
  KCHECK();
  return BLMM_OK;
}

// ---- null-grid: T[g][l] = L^-1 of the locus's residual Gram under grid point g's weights ----------------------------------------
// grid = (loci / 256, ngrid); LDS: the weights and Z0 (n (1 + c) doubles), L_Z^-1 of Z0'W_g Z0 (thread 0, as k_isx).
template <int K>
__global__ void __launch_bounds__(256) k_mdf_table(int n, int c, const double* __restrict__ Xt, int64_t ldx, int64_t nloci,
                                                   const double* __restrict__ Z0, const double* __restrict__ lam,
                                                   const double* __restrict__ grid, double* __restrict__ T) {
  constexpr int NP = K * (K + 1) / 2;
  extern __shared__ __attribute__((aligned(16))) double sh[];
  double* sW = sh;
  double* sZ = sh + n;
  __shared__ double sLi[MDF_CMAX * MDF_CMAX];
  const int g = blockIdx.y;
  const double h2 = grid[g];
  const double delta = h2 / (1.0 - h2);
  for (int e = threadIdx.x; e < n; e += blockDim.x) sW[e] = fabs(1.0 / fma(delta, lam[e], 1.0));
  for (int e = threadIdx.x; e < n * c; e += blockDim.x) sZ[e] = Z0[e];
  __syncthreads();
  if (threadIdx.x == 0) {
    constexpr int NA = MDF_CMAX * (MDF_CMAX + 1) / 2;
    double A[NA], Lz[NA];
    for (int a = 0; a < NA; ++a) A[a] = 0.0;
    for (int k = 0; k < n; ++k)
      for (int q = 0; q < c; ++q)
        for (int r = 0; r <= q; ++r) A[q * (q + 1) / 2 + r] = fma(sW[k] * sZ[q * n + k], sZ[r * n + k], A[q * (q + 1) / 2 + r]);
    for (int q = 0; q < c; ++q)
      for (int r = 0; r <= q; ++r) {
        double s = A[q * (q + 1) / 2 + r];
        for (int u = 0; u < r; ++u) s = fma(-Lz[q * (q + 1) / 2 + u], Lz[r * (r + 1) / 2 + u], s);
        Lz[q * (q + 1) / 2 + r] = (r == q) ? sqrt(s) : s / Lz[r * (r + 1) / 2 + r];
      }
    for (int q = 0; q < c; ++q)
      for (int r = 0; r < MDF_CMAX; ++r) {
        double s = 0.0;
        if (r <= q) {
          s = (r == q) ? 1.0 : 0.0;
          for (int u = r; u < q; ++u) s = fma(-Lz[q * (q + 1) / 2 + u], sLi[u * MDF_CMAX + r], s);
          s /= Lz[q * (q + 1) / 2 + q];
        }
        sLi[q * MDF_CMAX + r] = s;
      }
  }
  __syncthreads();
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= nloci) return;
  double S[NP], d0[K], xz[K][MDF_CMAX];
#pragma unroll
  for (int a = 0; a < NP; ++a) S[a] = 0.0;
#pragma unroll
  for (int a = 0; a < K; ++a)
#pragma unroll
    for (int q = 0; q < MDF_CMAX; ++q) xz[a][q] = 0.0;
  const double* xp = Xt + l * K;
  for (int k = 0; k < n; ++k) {
    double x[K];
#pragma unroll
    for (int a = 0; a < K; ++a) x[a] = xp[(int64_t)k * ldx + a];
    const double w = sW[k];
#pragma unroll
    for (int a = 0; a < K; ++a) {
      const double wx = w * x[a];
#pragma unroll
      for (int b = 0; b <= a; ++b) S[a * (a + 1) / 2 + b] = fma(wx, x[b], S[a * (a + 1) / 2 + b]);
#pragma unroll
      for (int q = 0; q < MDF_CMAX; ++q)
        if (q < c) xz[a][q] = fma(wx, sZ[q * n + k], xz[a][q]);
    }
  }
#pragma unroll
  for (int a = 0; a < K; ++a) d0[a] = S[a * (a + 1) / 2 + a];
  // u_aq = (L_Z^-1 Z'W x_a)_q, folded into S one covariate at a time
#pragma unroll
  for (int q = 0; q < MDF_CMAX; ++q) {
    if (q >= c) break;
    double u[K];
#pragma unroll
    for (int a = 0; a < K; ++a) {
      double s = 0.0;
#pragma unroll
      for (int r = 0; r <= q; ++r) s = fma(sLi[q * MDF_CMAX + r], xz[a][r], s);
      u[a] = s;
    }
#pragma unroll
    for (int a = 0; a < K; ++a)
#pragma unroll
      for (int b = 0; b <= a; ++b) S[a * (a + 1) / 2 + b] = fma(-u[a], u[b], S[a * (a + 1) / 2 + b]);
  }
  mdf_chol<K>(S, d0);
  // T = L^-1 (packed lower), rows / columns of dropped loci columns zero
  double Ti[NP];
#pragma unroll
  for (int q = 0; q < K; ++q) {
    const double lqq = S[q * (q + 1) / 2 + q];
#pragma unroll
    for (int r = 0; r <= q; ++r) {
      double s = (r == q) ? 1.0 : 0.0;
#pragma unroll
      for (int u = r; u < q; ++u) s = fma(-S[q * (q + 1) / 2 + u], Ti[u * (u + 1) / 2 + r], s);
      Ti[q * (q + 1) / 2 + r] = (lqq > 0.0) ? s / lqq : 0.0;
    }
  }
  double* out = T + ((int64_t)g * nloci + l) * NP;
#pragma unroll
  for (int a = 0; a < NP; ++a) out[a] = Ti[a];
}

// ---- null-grid scan ----------------------------------------------------------------------------------------------------------
template <int K, int TJ>
__global__ void __launch_bounds__(256) k_mdf_grid(MdfArgs a) {
  constexpr int NP = K * (K + 1) / 2;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t j0 = ((int64_t)blockIdx.y * 4 + wv) * TJ;
  if (j0 >= a.m) return;                                     // the whole wave
  const int64_t l = (int64_t)blockIdx.x * 64 + lane;
  const int64_t lc = l < a.nloci ? l : a.nloci - 1;
  const double* __restrict__ xp = a.Xt + lc * K;
  const double* __restrict__ ap = a.P + j0;                 // panel 0, traits j0 .. j0 + TJ - 1 (padding columns are zero: j0 + TJ <= ldp)
  double acc[TJ][K];
#pragma unroll
  for (int t = 0; t < TJ; ++t)
#pragma unroll
    for (int q = 0; q < K; ++q) acc[t][q] = 0.0;
  for (int i = 0; i < a.n; ++i) {
    double x[K], av[TJ];
#pragma unroll
    for (int q = 0; q < K; ++q) x[q] = xp[(int64_t)i * a.ldx + q];
#pragma unroll
    for (int t = 0; t < TJ; ++t) av[t] = ap[(int64_t)i * a.ldp + t];
#pragma unroll
    for (int t = 0; t < TJ; ++t)
#pragma unroll
      for (int q = 0; q < K; ++q) acc[t][q] = fma(x[q], av[t], acc[t][q]);
  }
  const double scale = -0.5 * (double)a.n;
  const bool valid = l < a.nloci;
  int nnan = 0;
#pragma unroll
  for (int t = 0; t < TJ; ++t) {
    const int64_t j = j0 + t;
    if (j >= a.m) break;
    const double* Tp = a.T + ((int64_t)a.bin[j] * a.nloci + lc) * NP;
    double r2 = 0.0;
#pragma unroll
    for (int q = 0; q < K; ++q) {
      double z = 0.0;
#pragma unroll
      for (int r = 0; r <= q; ++r) z = fma(Tp[q * (q + 1) / 2 + r], acc[t][r], z);
      r2 = fma(z, z, r2);
    }
    const double lod = mdf_lod(r2, scale, valid, &nnan);
    if (valid) a.L[j * a.ldL + l] = lod;
  }
  if (nnan) atomicAdd((unsigned long long*)&a.stat[ST_NAN_LOD], (unsigned long long)nnan);
}

// ---- null-grid scan, reduced in the epilogue (blmm_bulkscan_multidf_perms) ------------------------------------------------------
// k_mdf_grid's contraction and z = T b over the panel columns of a trait chunk; nothing goes to L.  Every column's 64 LODs of the wave are
// reduced to (maximum, locus) -- candidates are (value, locus) pairs under k_colmax's order (larger value, then lower locus), a NaN
// or a lane beyond nloci is no candidate, so the result does not depend on the order of the exchanges: four DPP steps inside the
// 16-lane rows, then the rows across 16 and 32 lanes -- and lane 0 writes the partial of (slot = blockIdx.x, column) for k_red_final.
// A slot without a candidate holds (-inf, -1).  NaN LODs are counted (ST_NAN_LOD) in the UNPERMUTED columns only (the first column
// of each bin): the count is that of the data's own scan, whatever nperms is.
//
// SCAN (blmm_bulkscan_multidf_reduced): the columns are the traits themselves, bin[j] their grid bins -- every column's NaNs count,
// and with r.want_trip every LOD > r.thr is appended as a (locus, trait, LOD) triplet, one wave-aggregated atomic reserving the
// wave's slots (as k_threshold and the 1-df epilogue, kernels_scan.hip: red_row).  r is read by the SCAN instantiations only; it
// comes last so that the permutation instantiations keep their kernel-argument offsets, instruction for instruction.
template <int CTRL>
__device__ __forceinline__ int mdf_dpp_movi(int x) { return __builtin_amdgcn_update_dpp(x, x, CTRL, 0xf, 0xf, false); }
__device__ __forceinline__ void mdf_red_comb(double& best, int& bi, double ob, int oi) {
  if (ob > best || (ob == best && oi >= 0 && (bi < 0 || oi < bi))) { best = ob; bi = oi; }
}
// every lane's candidate -> the wave's best, in all lanes
__device__ __forceinline__ void mdf_red_wave(double& best, int& bi) {
  { const double ob = blmm_dpp_mov<0xB1>(best); const int oi = mdf_dpp_movi<0xB1>(bi); mdf_red_comb(best, bi, ob, oi); }     // lane ^ 1
  { const double ob = blmm_dpp_mov<0x4E>(best); const int oi = mdf_dpp_movi<0x4E>(bi); mdf_red_comb(best, bi, ob, oi); }     // lane ^ 2
  { const double ob = blmm_dpp_mov<0x141>(best); const int oi = mdf_dpp_movi<0x141>(bi); mdf_red_comb(best, bi, ob, oi); }   // row_half_mirror
  { const double ob = blmm_dpp_mov<0x140>(best); const int oi = mdf_dpp_movi<0x140>(bi); mdf_red_comb(best, bi, ob, oi); }   // row_mirror
  { const double ob = __shfl_xor(best, 16, 64); const int oi = __shfl_xor(bi, 16, 64); mdf_red_comb(best, bi, ob, oi); }
  { const double ob = __shfl_xor(best, 32, 64); const int oi = __shfl_xor(bi, 32, 64); mdf_red_comb(best, bi, ob, oi); }
}
// the wave's 64 LODs of trait j (lane = locus blockIdx.x * 64 + lane; `valid`: the locus exists)
__device__ __forceinline__ void mdf_trip_append(const RedArgs& r, double lod, bool valid, int lane, int64_t j) {
  const bool hit = valid && lod > r.thr;                       // a NaN never passes
  const unsigned long long mask = __ballot(hit);
  if (mask == 0ull) return;
  const int leader = (int)__builtin_ctzll(mask);
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd(r.cnt, (unsigned long long)__builtin_popcountll(mask));
  const unsigned int blo = __builtin_amdgcn_readlane((unsigned int)base, leader);
  const unsigned int bhi = __builtin_amdgcn_readlane((unsigned int)(base >> 32), leader);
  if (hit) {
    const unsigned long long slot = (((unsigned long long)bhi << 32) | blo) + (unsigned long long)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
    if ((int64_t)slot < r.cap) { r.ti[slot] = (int32_t)(blockIdx.x * 64 + lane); r.tj[slot] = (int32_t)j; r.tl[slot] = lod; }
  }
}
template <int K, int TJ, bool SCAN = false>
__global__ void __launch_bounds__(256) k_mdf_grid_red(MdfArgs a, double* pmax, int* parg, int64_t ldm, RedArgs r) {
  constexpr int NP = K * (K + 1) / 2;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t j0 = ((int64_t)blockIdx.y * 4 + wv) * TJ;
  if (j0 >= a.m) return;                                     // the whole wave
  const int64_t l = (int64_t)blockIdx.x * 64 + lane;
  const int64_t lc = l < a.nloci ? l : a.nloci - 1;
  const double* __restrict__ xp = a.Xt + lc * K;
  const double* __restrict__ ap = a.P + j0;                 // the panel columns j0 .. j0 + TJ - 1 (padding columns are zero: j0 + TJ <= ldp)
  double acc[TJ][K];
#pragma unroll
  for (int t = 0; t < TJ; ++t)
#pragma unroll
    for (int q = 0; q < K; ++q) acc[t][q] = 0.0;
  for (int i = 0; i < a.n; ++i) {                            // k_mdf_grid's loop, statement for statement
    double x[K], av[TJ];
#pragma unroll
    for (int q = 0; q < K; ++q) x[q] = xp[(int64_t)i * a.ldx + q];
#pragma unroll
    for (int t = 0; t < TJ; ++t) av[t] = ap[(int64_t)i * a.ldp + t];
#pragma unroll
    for (int t = 0; t < TJ; ++t)
#pragma unroll
      for (int q = 0; q < K; ++q) acc[t][q] = fma(x[q], av[t], acc[t][q]);
  }
  const double scale = -0.5 * (double)a.n;
  const bool valid = l < a.nloci;
  int nnan = 0;
#pragma unroll
  for (int t = 0; t < TJ; ++t) {
    const int64_t j = j0 + t;
    if (j >= a.m) break;                                     // wave-uniform
    const int bj = a.bin[j];
    const bool orig = SCAN || j == 0 || a.bin[j - 1] != bj;  // the trait itself: the first column of its bin (SCAN: every column)
    const double* Tp = a.T + ((int64_t)bj * a.nloci + lc) * NP;
    double r2 = 0.0;
#pragma unroll
    for (int q = 0; q < K; ++q) {
      double z = 0.0;
#pragma unroll
      for (int r = 0; r <= q; ++r) z = fma(Tp[q * (q + 1) / 2 + r], acc[t][r], z);
      r2 = fma(z, z, r2);
    }
    int now = 0;
    const double lod = mdf_lod(r2, scale, valid, &now);
    nnan += orig ? now : 0;
    const bool cand = valid && lod == lod;
    double best = cand ? lod : -INFINITY;
    int bi = cand ? lane : -1;
    { const double ob = blmm_dpp_mov<0xB1>(best); const int oi = mdf_dpp_movi<0xB1>(bi); mdf_red_comb(best, bi, ob, oi); }     // lane ^ 1
    { const double ob = blmm_dpp_mov<0x4E>(best); const int oi = mdf_dpp_movi<0x4E>(bi); mdf_red_comb(best, bi, ob, oi); }     // lane ^ 2
    { const double ob = blmm_dpp_mov<0x141>(best); const int oi = mdf_dpp_movi<0x141>(bi); mdf_red_comb(best, bi, ob, oi); }   // row_half_mirror
    { const double ob = blmm_dpp_mov<0x140>(best); const int oi = mdf_dpp_movi<0x140>(bi); mdf_red_comb(best, bi, ob, oi); }   // row_mirror
    { const double ob = __shfl_xor(best, 16, 64); const int oi = __shfl_xor(bi, 16, 64); mdf_red_comb(best, bi, ob, oi); }
    { const double ob = __shfl_xor(best, 32, 64); const int oi = __shfl_xor(bi, 32, 64); mdf_red_comb(best, bi, ob, oi); }
    if (lane == 0) {
      const int64_t at = (int64_t)blockIdx.x * ldm + j;
      pmax[at] = best;
      parg[at] = bi < 0 ? -1 : (int)(blockIdx.x * 64 + bi);
    }
    if constexpr (SCAN) {
      if (r.want_trip) mdf_trip_append(r, lod, valid, lane, j);   // kernel argument: a scalar branch
    }
  }
  if (nnan) atomicAdd((unsigned long long*)&a.stat[ST_NAN_LOD], (unsigned long long)nnan);
}

// ---- null-exact scan ---------------------------------------------------------------------------------------------------------
template <int K, int TJ>
__global__ void __launch_bounds__(256) k_mdf_exact(MdfArgs a) {
  constexpr int NP = K * (K + 1) / 2;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t j0 = ((int64_t)blockIdx.y * 4 + wv) * TJ;
  if (j0 >= a.m) return;
  const int64_t l = (int64_t)blockIdx.x * 64 + lane;
  const int64_t lc = l < a.nloci ? l : a.nloci - 1;
  const double* __restrict__ xp = a.Xt + lc * K;
  const double* __restrict__ a0 = a.P + j0;
  const double* __restrict__ a1 = a.P + a.pstride + j0;
  double b[TJ][K], S[TJ][NP], d0[TJ][K];
#pragma unroll
  for (int t = 0; t < TJ; ++t) {
#pragma unroll
    for (int q = 0; q < K; ++q) b[t][q] = 0.0;
#pragma unroll
    for (int q = 0; q < NP; ++q) S[t][q] = 0.0;
  }
  // pass 0: numerators b and the weighted Gram P of the locus columns
  for (int i = 0; i < a.n; ++i) {
    double x[K], xx[NP], v0[TJ], v1[TJ];
#pragma unroll
    for (int q = 0; q < K; ++q) x[q] = xp[(int64_t)i * a.ldx + q];
#pragma unroll
    for (int q = 0; q < K; ++q)
#pragma unroll
      for (int r = 0; r <= q; ++r) xx[q * (q + 1) / 2 + r] = x[q] * x[r];
#pragma unroll
    for (int t = 0; t < TJ; ++t) { v0[t] = a0[(int64_t)i * a.ldp + t]; v1[t] = a1[(int64_t)i * a.ldp + t]; }
#pragma unroll
    for (int t = 0; t < TJ; ++t) {
#pragma unroll
      for (int q = 0; q < K; ++q) b[t][q] = fma(x[q], v0[t], b[t][q]);
#pragma unroll
      for (int q = 0; q < NP; ++q) S[t][q] = fma(xx[q], v1[t], S[t][q]);
    }
  }
#pragma unroll
  for (int t = 0; t < TJ; ++t)
#pragma unroll
    for (int q = 0; q < K; ++q) d0[t][q] = S[t][q * (q + 1) / 2 + q];
  // one pass per covariate: u_q = X_l' panel(2+q), S -= u_q u_q'
  for (int cq = 0; cq < a.c; ++cq) {
    const double* __restrict__ aq = a.P + (int64_t)(2 + cq) * a.pstride + j0;
    double u[TJ][K];
#pragma unroll
    for (int t = 0; t < TJ; ++t)
#pragma unroll
      for (int q = 0; q < K; ++q) u[t][q] = 0.0;
    for (int i = 0; i < a.n; ++i) {
      double x[K], v[TJ];
#pragma unroll
      for (int q = 0; q < K; ++q) x[q] = xp[(int64_t)i * a.ldx + q];
#pragma unroll
      for (int t = 0; t < TJ; ++t) v[t] = aq[(int64_t)i * a.ldp + t];
#pragma unroll
      for (int t = 0; t < TJ; ++t)
#pragma unroll
        for (int q = 0; q < K; ++q) u[t][q] = fma(x[q], v[t], u[t][q]);
    }
#pragma unroll
    for (int t = 0; t < TJ; ++t)
#pragma unroll
      for (int q = 0; q < K; ++q)
#pragma unroll
        for (int r = 0; r <= q; ++r) S[t][q * (q + 1) / 2 + r] = fma(-u[t][q], u[t][r], S[t][q * (q + 1) / 2 + r]);
  }
  const double scale = -0.5 * (double)a.n;
  const bool valid = l < a.nloci;
  int nnan = 0;
#pragma unroll
  for (int t = 0; t < TJ; ++t) {
    const int64_t j = j0 + t;
    if (j >= a.m) break;
    mdf_chol<K>(S[t], d0[t]);
    const double lod = mdf_lod(mdf_r2<K>(S[t], b[t]), scale, valid, &nnan);
    if (valid) a.L[j * a.ldL + l] = lod;
  }
  if (nnan) atomicAdd((unsigned long long*)&a.stat[ST_NAN_LOD], (unsigned long long)nnan);
}

// ---- null-exact scan, reduced in the epilogue (blmm_bulkscan_multidf_reduced) -----------------------------------------------------
// k_mdf_exact's contraction and factorisation repeated statement for statement (the LODs carry its bits; shared as a device function
// the two passes scheduled differently in k_mdf_exact itself, which stays as it was); the store is replaced by
// k_mdf_grid_red's SCAN epilogue.  A trait the conditioning guard flagged (r.flags, written before this kernel runs) keeps the
// partial (-inf, -1), appends no triplet and counts no NaN: k_mdf_qr's reduced form and k_mdf_flag_red supply all three.
template <int K, int TJ>
__global__ void __launch_bounds__(256) k_mdf_exact_red(MdfArgs a, RedArgs r) {
  constexpr int NP = K * (K + 1) / 2;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t j0 = ((int64_t)blockIdx.y * 4 + wv) * TJ;
  if (j0 >= a.m) return;
  const int64_t l = (int64_t)blockIdx.x * 64 + lane;
  const int64_t lc = l < a.nloci ? l : a.nloci - 1;
  const double* __restrict__ xp = a.Xt + lc * K;
  const double* __restrict__ a0 = a.P + j0;
  const double* __restrict__ a1 = a.P + a.pstride + j0;
  double b[TJ][K], S[TJ][NP], d0[TJ][K];
#pragma unroll
  for (int t = 0; t < TJ; ++t) {
#pragma unroll
    for (int q = 0; q < K; ++q) b[t][q] = 0.0;
#pragma unroll
    for (int q = 0; q < NP; ++q) S[t][q] = 0.0;
  }
  // pass 0: numerators b and the weighted Gram P of the locus columns
  for (int i = 0; i < a.n; ++i) {
    double x[K], xx[NP], v0[TJ], v1[TJ];
#pragma unroll
    for (int q = 0; q < K; ++q) x[q] = xp[(int64_t)i * a.ldx + q];
#pragma unroll
    for (int q = 0; q < K; ++q)
#pragma unroll
      for (int r = 0; r <= q; ++r) xx[q * (q + 1) / 2 + r] = x[q] * x[r];
#pragma unroll
    for (int t = 0; t < TJ; ++t) { v0[t] = a0[(int64_t)i * a.ldp + t]; v1[t] = a1[(int64_t)i * a.ldp + t]; }
#pragma unroll
    for (int t = 0; t < TJ; ++t) {
#pragma unroll
      for (int q = 0; q < K; ++q) b[t][q] = fma(x[q], v0[t], b[t][q]);
#pragma unroll
      for (int q = 0; q < NP; ++q) S[t][q] = fma(xx[q], v1[t], S[t][q]);
    }
  }
#pragma unroll
  for (int t = 0; t < TJ; ++t)
#pragma unroll
    for (int q = 0; q < K; ++q) d0[t][q] = S[t][q * (q + 1) / 2 + q];
  // one pass per covariate: u_q = X_l' panel(2+q), S -= u_q u_q'
  for (int cq = 0; cq < a.c; ++cq) {
    const double* __restrict__ aq = a.P + (int64_t)(2 + cq) * a.pstride + j0;
    double u[TJ][K];
#pragma unroll
    for (int t = 0; t < TJ; ++t)
#pragma unroll
      for (int q = 0; q < K; ++q) u[t][q] = 0.0;
    for (int i = 0; i < a.n; ++i) {
      double x[K], v[TJ];
#pragma unroll
      for (int q = 0; q < K; ++q) x[q] = xp[(int64_t)i * a.ldx + q];
#pragma unroll
      for (int t = 0; t < TJ; ++t) v[t] = aq[(int64_t)i * a.ldp + t];
#pragma unroll
      for (int t = 0; t < TJ; ++t)
#pragma unroll
        for (int q = 0; q < K; ++q) u[t][q] = fma(x[q], v[t], u[t][q]);
    }
#pragma unroll
    for (int t = 0; t < TJ; ++t)
#pragma unroll
      for (int q = 0; q < K; ++q)
#pragma unroll
        for (int r = 0; r <= q; ++r) S[t][q * (q + 1) / 2 + r] = fma(-u[t][q], u[t][r], S[t][q * (q + 1) / 2 + r]);
  }
  const double scale = -0.5 * (double)a.n;
  const bool valid = l < a.nloci;
  int nnan = 0;
#pragma unroll
  for (int t = 0; t < TJ; ++t) {
    const int64_t j = j0 + t;
    if (j >= a.m) break;                                     // wave-uniform
    const int64_t at = (int64_t)blockIdx.x * r.ldm + j;
    if (r.flags && r.flags[j] != 0) {                        // wave-uniform
      if (lane == 0) { r.pmax[at] = -INFINITY; r.parg[at] = -1; }
      continue;
    }
    mdf_chol<K>(S[t], d0[t]);
    const double lod = mdf_lod(mdf_r2<K>(S[t], b[t]), scale, valid, &nnan);
    const bool cand = valid && lod == lod;
    double best = cand ? lod : -INFINITY;
    int bi = cand ? lane : -1;
    mdf_red_wave(best, bi);
    if (lane == 0) {
      r.pmax[at] = best;
      r.parg[at] = bi < 0 ? -1 : (int)(blockIdx.x * 64 + bi);
    }
    if (r.want_trip) mdf_trip_append(r, lod, valid, lane, j);   // kernel argument: a scalar branch
  }
  if (nnan) atomicAdd((unsigned long long*)&a.stat[ST_NAN_LOD], (unsigned long long)nnan);
}

// ---- the conditioning guard's re-scan of listed traits (null-exact, c >= 2) ------------------------------------------------------
// One workgroup per listed trait at a time (grid-stride over the device count stat[ST_ILLCOND]); buf: (c + 2) n doubles (weights'
// square roots, the orthonormal basis, the unit trait residual), in LDS or in a per-workgroup slab of global memory.
// RED (blmm_bulkscan_multidf_reduced): there is no L.  The listed traits item0 .. item0 + nitem - 1 go to the columns 0 .. nitem - 1
// of a compact scratch (L, ld ldL) for k_mdf_flag_red, and every NaN counts: k_mdf_exact_red counted none for a flagged trait.
template <int K, bool RED = false>
__global__ void __launch_bounds__(256) k_mdf_qr(int n, int c, const double* __restrict__ Yt, int64_t ldy,
                                                const double* __restrict__ Xt, int64_t ldx, int64_t nloci,
                                                const double* __restrict__ Z0, const double* __restrict__ lam,
                                                const double* __restrict__ h2v, const int* __restrict__ list, double* slab,
                                                double* __restrict__ L, int64_t ldL, int64_t* stat, int64_t item0, int64_t nitem) {
  constexpr int NP = K * (K + 1) / 2;
  extern __shared__ __attribute__((aligned(16))) double sh[];
  __shared__ double s_red[4];
  int64_t cnt = stat[ST_ILLCOND];
  if (RED && cnt > item0 + nitem) cnt = item0 + nitem;
  if (cnt <= 0) return;
  double* buf = slab ? slab + (size_t)blockIdx.x * (size_t)(c + 2) * n : sh;
  double* Sw = buf;
  double* Qb = buf + n;
  double* yb = buf + (size_t)(1 + c) * n;
  const double scale = -0.5 * (double)n;
  int nnan = 0;
  for (int64_t item = (RED ? item0 : 0) + blockIdx.x; item < cnt; item += gridDim.x) {
    const int64_t j = list[item];
    double* __restrict__ col = L + (RED ? item - item0 : j) * ldL;
    const double nn = weighted_basis<256, 1, true>(n, c, h2v[j], lam, [&](int q, int k) { return Z0[(size_t)q * n + k]; },
                                                   Yt + j, ldy, Sw, Qb, yb, s_red);
    const double inv = 1.0 / sqrt(nn);
    for (int k = threadIdx.x; k < n; k += 256) yb[k] *= inv;
    __syncthreads();
    for (int64_t l = threadIdx.x; l < nloci; l += 256) {
      const double* xp = Xt + l * K;
      double t[K][MDF_CMAX], t2[K][MDF_CMAX];
#pragma unroll
      for (int a = 0; a < K; ++a)
#pragma unroll
        for (int q = 0; q < MDF_CMAX; ++q) { t[a][q] = 0.0; t2[a][q] = 0.0; }
      for (int k = 0; k < n; ++k) {
#pragma unroll
        for (int a = 0; a < K; ++a) {
          const double x = Sw[k] * xp[(int64_t)k * ldx + a];
#pragma unroll
          for (int q = 0; q < MDF_CMAX; ++q)
            if (q < c) t[a][q] = fma(Qb[(size_t)q * n + k], x, t[a][q]);
        }
      }
      for (int k = 0; k < n; ++k) {                  // second projection pass on the first residual
#pragma unroll
        for (int a = 0; a < K; ++a) {
          double x = Sw[k] * xp[(int64_t)k * ldx + a];
#pragma unroll
          for (int q = 0; q < MDF_CMAX; ++q)
            if (q < c) x = fma(-t[a][q], Qb[(size_t)q * n + k], x);
#pragma unroll
          for (int q = 0; q < MDF_CMAX; ++q)
            if (q < c) t2[a][q] = fma(Qb[(size_t)q * n + k], x, t2[a][q]);
        }
      }
#pragma unroll
      for (int a = 0; a < K; ++a)
#pragma unroll
        for (int q = 0; q < MDF_CMAX; ++q) t[a][q] += t2[a][q];
      double S[NP], bb[K], d0[K];
#pragma unroll
      for (int a = 0; a < NP; ++a) S[a] = 0.0;
#pragma unroll
      for (int a = 0; a < K; ++a) { bb[a] = 0.0; d0[a] = 0.0; }
      for (int k = 0; k < n; ++k) {
        double r[K];
#pragma unroll
        for (int a = 0; a < K; ++a) {
          const double x = Sw[k] * xp[(int64_t)k * ldx + a];
          d0[a] = fma(x, x, d0[a]);
          double v = x;
#pragma unroll
          for (int q = 0; q < MDF_CMAX; ++q)
            if (q < c) v = fma(-t[a][q], Qb[(size_t)q * n + k], v);
          r[a] = v;
          bb[a] = fma(v, yb[k], bb[a]);
        }
#pragma unroll
        for (int a = 0; a < K; ++a)
#pragma unroll
          for (int b = 0; b <= a; ++b) S[a * (a + 1) / 2 + b] = fma(r[a], r[b], S[a * (a + 1) / 2 + b]);
      }
      mdf_chol<K>(S, d0);
      // the scan already wrote (and counted, if NaN) this entry: n_nan_lod counts the NaNs of the finished L, so the re-scan
      // adds its own NaN and takes back the scan's
      int now = 0;
      const double lod = mdf_lod(mdf_r2<K>(S, bb), scale, true, &now);
      nnan += RED ? now : now - (isnan(col[l]) ? 1 : 0);
      col[l] = lod;
    }
  }
  if (nnan) atomicAdd((unsigned long long*)&stat[ST_NAN_LOD], (unsigned long long)(long long)nnan);   // (two's complement: may be < 0)
}

// ---- the flagged traits' scratch columns -> their maxima and triplets (blmm_bulkscan_multidf_reduced) ----------------------------
// One wave per column of k_mdf_qr's scratch (column e = listed trait item0 + e); k_colmax's rule into mx / arg (either may be null)
// at the TRAIT's index and k_threshold's append with the trait's index, written over what k_red_final left for a flagged trait.
__global__ void __launch_bounds__(256) k_mdf_flag_red(const double* __restrict__ S, int64_t nloci, const int* __restrict__ list,
                                                      const int64_t* __restrict__ stat, int64_t item0, int64_t nitem,
                                                      double* __restrict__ mx, int64_t* __restrict__ arg, RedArgs r) {
  const int lane = threadIdx.x & 63;
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t left = stat[ST_ILLCOND] - item0;
  if (e >= nitem || e >= left) return;                       // the whole wave
  const int64_t j = list[item0 + e];
  const double* col = S + e * nloci;
  double best = -INFINITY;
  int64_t bi = -1;
  for (int64_t i0 = 0; i0 < nloci; i0 += 64) {
    const int64_t i = i0 + lane;
    const double v = i < nloci ? col[i] : -INFINITY;
    if (v > best) { best = v; bi = i; }
    if (r.want_trip) {
      const bool hit = v > r.thr;
      const unsigned long long mask = __ballot(hit);
      if (mask == 0ull) continue;
      unsigned long long base = 0;
      if (lane == (int)__builtin_ctzll(mask)) base = atomicAdd(r.cnt, (unsigned long long)__builtin_popcountll(mask));
      base = __shfl(base, (int)__builtin_ctzll(mask), 64);
      if (hit) {
        const unsigned long long slot = base + (unsigned long long)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
        if ((int64_t)slot < r.cap) { r.ti[slot] = (int32_t)i; r.tj[slot] = (int32_t)j; r.tl[slot] = v; }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ob = __shfl_xor(best, o, 64);
    const int64_t oi = __shfl_xor(bi, o, 64);
    if (ob > best || (ob == best && oi >= 0 && (bi < 0 || oi < bi))) { best = ob; bi = oi; }
  }
  if (lane == 0) { if (mx) mx[j] = best; if (arg) arg[j] = bi; }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------
int launch_mdf_table(blmm_ctx* ctx, const NullModel& nm, const double* Xt, int64_t ldx, int64_t nloci, int k, const double* Z0,
                     const double* lam, const double* grid_dev, int ngrid, double* T) {
  if (nloci <= 0 || ngrid <= 0) return BLMM_OK;
  const dim3 grid((unsigned)((nloci + 255) / 256), (unsigned)ngrid);
  const size_t lds = sizeof(double) * (size_t)nm.n * (1 + nm.c);
#define TB(K) do { if (lds > 48 * 1024) BLMM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mdf_table<K>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
    hipLaunchKernelGGL(k_mdf_table<K>, grid, dim3(256), lds, ctx->stream, nm.n, nm.c, Xt, ldx, nloci, Z0, lam, grid_dev, T); } while (0)
  switch (k) {
    case 1: TB(1); break; case 2: TB(2); break; case 3: TB(3); break; case 4: TB(4); break;
    case 5: TB(5); break; case 6: TB(6); break; case 7: TB(7); break; case 8: TB(8); break;
    default: return fail(ctx, BLMM_ERR_UNSUPPORTED, "bulkscan_multidf: null-grid takes 1 <= k <= 8");
  }
#undef TB
  KCHECK();
  return BLMM_OK;
}

// traits per wave: the accumulators of one lane stay within ~64 doubles
template <int K> constexpr int mdf_tj_grid() { return K <= 4 ? 16 : 8; }
template <int K> constexpr int mdf_tj_exact() { return K == 1 ? 16 : K == 2 ? 8 : 4; }

int launch_mdf_scan(blmm_ctx* ctx, const MdfArgs& a, bool exact) {
  if (a.nloci <= 0 || a.m <= 0) return BLMM_OK;
  const unsigned gx = (unsigned)((a.nloci + 63) / 64);
#define SG(K) do { constexpr int TJ = mdf_tj_grid<K>(); \
    hipLaunchKernelGGL((k_mdf_grid<K, TJ>), dim3(gx, (unsigned)((a.m + 4 * TJ - 1) / (4 * TJ))), dim3(256), 0, ctx->stream, a); } while (0)
#define SE(K) do { constexpr int TJ = mdf_tj_exact<K>(); \
    hipLaunchKernelGGL((k_mdf_exact<K, TJ>), dim3(gx, (unsigned)((a.m + 4 * TJ - 1) / (4 * TJ))), dim3(256), 0, ctx->stream, a); } while (0)
  if (exact) {
    switch (a.k) {
      case 1: SE(1); break; case 2: SE(2); break; case 3: SE(3); break; case 4: SE(4); break;
      default: return fail(ctx, BLMM_ERR_UNSUPPORTED, "bulkscan_multidf: null-exact takes 1 <= k <= 4");
    }
  } else {
    switch (a.k) {
      case 1: SG(1); break; case 2: SG(2); break; case 3: SG(3); break; case 4: SG(4); break;
      case 5: SG(5); break; case 6: SG(6); break; case 7: SG(7); break; case 8: SG(8); break;
      default: return fail(ctx, BLMM_ERR_UNSUPPORTED, "bulkscan_multidf: null-grid takes 1 <= k <= 8");
    }
  }
#undef SG
#undef SE
  KCHECK();
  return BLMM_OK;
}

// The reducing null-grid scan: r.pmax / r.parg [slot = locus / 64][r.ldm] (ceil(nloci / 64) slots), a.L is not touched.  The same
// (K, TJ) pairs as the grid form; a.m (panel columns) is bounded by the grid's y extent: MDF_RED_MAX_COLS.
int launch_mdf_scan_red(blmm_ctx* ctx, const MdfArgs& a, const RedArgs& r) {
  if (a.nloci <= 0 || a.m <= 0) return BLMM_OK;
  if (a.m > MDF_RED_MAX_COLS) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_multidf_perms: too many panel columns in one chunk");
  const unsigned gx = (unsigned)((a.nloci + 63) / 64);
#define SR(K) do { constexpr int TJ = mdf_tj_grid<K>(); \
    hipLaunchKernelGGL((k_mdf_grid_red<K, TJ>), dim3(gx, (unsigned)((a.m + 4 * TJ - 1) / (4 * TJ))), dim3(256), 0, ctx->stream, a, r.pmax, r.parg, r.ldm, r); } while (0)
  switch (a.k) {
    case 1: SR(1); break; case 2: SR(2); break; case 3: SR(3); break; case 4: SR(4); break;
    case 5: SR(5); break; case 6: SR(6); break; case 7: SR(7); break; case 8: SR(8); break;
    default: return fail(ctx, BLMM_ERR_UNSUPPORTED, "bulkscan_multidf_perms: takes 1 <= k <= 8");
  }
#undef SR
  KCHECK();
  return BLMM_OK;
}

// The reducing scan of the traits themselves (blmm_bulkscan_multidf_reduced): k_mdf_grid_red's SCAN instantiations, or
// k_mdf_exact_red; partials as launch_mdf_scan_red, triplets behind r.cnt, r.flags (null-exact) the guard's flags.
int launch_mdf_scan_traits_red(blmm_ctx* ctx, const MdfArgs& a, const RedArgs& r, bool exact) {
  if (a.nloci <= 0 || a.m <= 0) return BLMM_OK;
  const unsigned gx = (unsigned)((a.nloci + 63) / 64);
#define GY(TJ) \
    const int64_t gy = (a.m + 4 * TJ - 1) / (4 * TJ); \
    if (gy > 65535) return fail(ctx, BLMM_ERR_UNSUPPORTED, "bulkscan_multidf_reduced: more than " + std::to_string(65535ll * 4 * TJ) + " traits in one call")
#define SG(K) do { constexpr int TJ = mdf_tj_grid<K>(); GY(TJ); \
    hipLaunchKernelGGL((k_mdf_grid_red<K, TJ, true>), dim3(gx, (unsigned)gy), dim3(256), 0, ctx->stream, a, r.pmax, r.parg, r.ldm, r); } while (0)
#define SE(K) do { constexpr int TJ = mdf_tj_exact<K>(); GY(TJ); \
    hipLaunchKernelGGL((k_mdf_exact_red<K, TJ>), dim3(gx, (unsigned)gy), dim3(256), 0, ctx->stream, a, r); } while (0)
  if (exact) {
    switch (a.k) {
      case 1: SE(1); break; case 2: SE(2); break; case 3: SE(3); break; case 4: SE(4); break;
      default: return fail(ctx, BLMM_ERR_UNSUPPORTED, "bulkscan_multidf: null-exact takes 1 <= k <= 4");
    }
  } else {
    switch (a.k) {
      case 1: SG(1); break; case 2: SG(2); break; case 3: SG(3); break; case 4: SG(4); break;
      case 5: SG(5); break; case 6: SG(6); break; case 7: SG(7); break; case 8: SG(8); break;
      default: return fail(ctx, BLMM_ERR_UNSUPPORTED, "bulkscan_multidf: null-grid takes 1 <= k <= 8");
    }
  }
#undef SG
#undef SE
#undef GY
  KCHECK();
  return BLMM_OK;
}

// scr != nullptr (the reduced form): the listed traits item0 .. item0 + nitem - 1 into the compact scratch scr (ld nloci) instead of L
int launch_mdf_qr(blmm_ctx* ctx, const NullModel& nm, const double* Yt, int64_t ldy, const double* Xt, int64_t ldx, int64_t nloci, int k,
                  const double* Z0, const double* lam, const double* h2, const int* list, double* L, int64_t ldL, int64_t* stat,
                  double* scr, int64_t item0, int64_t nitem) {
  if (nloci <= 0 || nm.c < 2) return BLMM_OK;
  size_t lds; double* slab; unsigned grid;
  if (int rc = qr_workspace(ctx, nm.c, nm.n, &lds, &slab, &grid)) return rc;
#define QR1(K, RED, OUT, LD) do { if (lds > 48 * 1024) BLMM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mdf_qr<K, RED>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
    hipLaunchKernelGGL((k_mdf_qr<K, RED>), dim3(grid), dim3(256), lds, ctx->stream, nm.n, nm.c, Yt, ldy, Xt, ldx, nloci, Z0, lam, h2, list, slab, OUT, LD, stat, item0, nitem); } while (0)
#define QR(K) do { if (scr) QR1(K, true, scr, nloci); else QR1(K, false, L, ldL); } while (0)
  switch (k) {
    case 1: QR(1); break; case 2: QR(2); break; case 3: QR(3); break; case 4: QR(4); break;
    default: return fail(ctx, BLMM_ERR_UNSUPPORTED, "bulkscan_multidf: null-exact takes 1 <= k <= 4");
  }
#undef QR
#undef QR1
  KCHECK();
  return BLMM_OK;
}

int launch_mdf_flag_red(blmm_ctx* ctx, const double* scr, int64_t nloci, const int* list, const int64_t* stat, int64_t item0,
                        int64_t nitem, double* mx, int64_t* arg, const RedArgs& r) {
  if (nitem <= 0) return BLMM_OK;
  hipLaunchKernelGGL(k_mdf_flag_red, dim3((unsigned)((nitem + 3) / 4)), dim3(256), 0, ctx->stream, scr, nloci, list, stat, item0, nitem,
                     mx, arg, r);
  KCHECK();
  return BLMM_OK;
}

}  // namespace blmm
