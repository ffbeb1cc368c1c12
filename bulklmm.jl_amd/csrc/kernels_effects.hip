// kernels_effects.hip -- coefficients and standard errors at a LIST of (locus, trait) tests (blmm_bulkscan_effects).
//
// Test t = (locus l: the k columns l k .. l k + k - 1 of G, trait j).  With w = |makeweights(h2_j)|, s = sqrt(w), everything in the
// rotated space of transform_rotation:
//   q~   orthonormal basis of span(s .* Z0)   (Gram-Schmidt, every projection done twice: ortho_basis.h, so nearly
//        collinear weighted covariates at h2 -> 1 need no separate guard)
//   e~ = s .* y0_j minus its q~ components,  rss0 = |e~|^2                                   -- these three depend on the trait only
//   r_a = s .* x0_a minus its q~ components;  u_a = r_a minus its components along the accepted u_b (b < a), normalised, ACCEPTED iff
//        |.|^2 > MDF_TAU |s .* x0_a|^2 (bulkscan_multidf's rank rule, in column order);  R_ba = u_b' r_a, R_aa = |.|: r = u R
//   z_a = u_a' e~,  rss1 = |e~ - sum z_a u_a|^2,  beta = R^-1 z,  [(D~'D~)^-1]_aa = sum_b (R^-1)_ab^2  (D~ = [s .* Z0, accepted columns]:
//        the locus block of the inverse is the inverse of the residual columns' Gram R'R),  lod = -(n/2) log10(rss1 / rss0)
// A dropped column has beta = se = 0 and takes no part in anything after it.
//
// Layout.  The tests are ordered by trait on the device (counting sort over trait[]: k_eff_hist, k_eff_scan, k_eff_scatter; the
// permutation `order` takes a sorted position back to the caller's index, so the outputs land in the caller's order).  The sorted
// list is cut into chunks of `chunk` positions and ONE WAVE (a 64-thread workgroup) takes a chunk: it rebuilds the trait part only
// when the trait changes, so a long run of one trait is split over many waves (each builds the trait part once) and a chunk of
// one-test traits builds it per test.  Every vector lives in the wave's buffer of (c + 2 + k) n doubles -- LDS, or beyond
// EFF_LDS_MAX bytes a per-workgroup slab of global memory with a bounded grid striding over the chunks (as qr_workspace,
// blmm_internal.h).  Lane t owns the elements t, t + 64, .. of every vector and only ever reads what it wrote itself, so neither form needs
// a barrier; sums go through the wave's xor butterfly (the same bits in every lane, in a fixed order: results do not depend on where
// a test lands in the sorted list).  The markers come column-major (launch_untranspose of bulkscan_multidf's uncentred rotation),
// so a test reads k n contiguous doubles.
#include "blmm_internal.h"
#include "ortho_basis.h"
#include <cmath>

namespace blmm {

#define KCHECK()                                                                                      \
  do {                                                                                                \
    hipError_t e__ = hipGetLastError();                                                               \
    if (e__ != hipSuccess) return fail(ctx, BLMM_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e__)); \
  } while (0)

constexpr size_t EFF_LDS_MAX = 40 * 1024;   // per wave: four or more waves of a CU's 160 KiB stay resident

// ---- counting sort of the tests by trait ----------------------------------------------------------------------------------------
// cnt: m + 2 ints, zeroed.  A test with an index out of range is counted in cnt[m + 1], gets NaN / -1 outputs and is left out.
__global__ void __launch_bounds__(256) k_eff_hist(EffArgs a) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.T) return;
  const int64_t j = a.trait[t], l = a.locus[t];
  if (j >= 0 && j < a.m && l >= 0 && l < a.nloci) { atomicAdd(&a.cnt[j], 1); return; }
  atomicAdd(&a.cnt[a.m + 1], 1);
  for (int q = 0; q < a.k; ++q) { a.beta[t * a.k + q] = NAN; a.se[t * a.k + q] = NAN; }
  a.sigma2[t] = NAN; a.lod[t] = NAN; a.accepted[t] = -1;
}
// cnt[0 .. m) -> its exclusive prefix sums, cnt[m] = the number of valid tests; one workgroup of 1024
__global__ void __launch_bounds__(1024) k_eff_scan(int* __restrict__ cnt, int64_t m) {
  __shared__ int tile[1024];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int64_t base = 0; base < m; base += 1024) {
    const int64_t e = base + threadIdx.x;
    const int v = e < m ? cnt[e] : 0;
    tile[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const int add = (int)threadIdx.x >= off ? tile[threadIdx.x - off] : 0;
      __syncthreads();
      tile[threadIdx.x] += add;
      __syncthreads();
    }
    const int c0 = carry;
    if (e < m) cnt[e] = c0 + tile[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry = c0 + tile[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) cnt[m] = carry;
}
// (the order inside a trait's run is whatever the atomics give: no output depends on it)
__global__ void __launch_bounds__(256) k_eff_scatter(EffArgs a) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.T) return;
  const int64_t j = a.trait[t], l = a.locus[t];
  if (j >= 0 && j < a.m && l >= 0 && l < a.nloci) a.order[atomicAdd(&a.cnt[j], 1)] = (int)t;
}

// ---- the wave's vector algebra ----------------------------------------------------------------------------------------------------
// (the wave's sums: ortho_basis.h's 64-thread forms with the plain xor butterfly, which take no LDS)
__device__ __forceinline__ double eff_wsum(double v) {
  double t[1] = {v};
  team_sum<64, 1, true>(t, nullptr);
  return t[0];
}

template <int K>
__global__ void __launch_bounds__(64) k_effects(EffArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sh[];
  // R (upper triangle; a dropped column's row and column are zero), z = u'e~, beta, the diagonal, a column of R^-1: the same in every
  // lane, and every lane stores them itself (same address, same bits), so each reads back what it wrote
  __shared__ double sR[K * K], sz[K], sb[K], sd[K], si[K];
  const int lane = threadIdx.x;
  const int n = a.n, c = a.c;
  double* buf = a.slab ? a.slab + (size_t)blockIdx.x * (size_t)(c + 2 + K) * n : sh;
  double* Sw = buf;                            // s
  double* Qb = buf + n;                        // q~ (c columns)
  double* eb = buf + (size_t)(1 + c) * n;      // e~
  double* Rb = buf + (size_t)(2 + c) * n;      // the locus's columns: r_a, then u_a (K columns)
  const int64_t nvalid = a.cnt[a.m];
  const double prior_df = a.prior_b > 0.0 ? a.prior_b + 2.0 : a.prior_b;   // src/wls.jl:72
  int64_t cur = -1;
  double rss0 = 0.0;
  int nnan = 0;
  for (int64_t ch = blockIdx.x; ch * a.chunk < nvalid; ch += gridDim.x) {
    const int64_t p0 = ch * a.chunk, p1 = p0 + a.chunk < nvalid ? p0 + a.chunk : nvalid;
    for (int64_t pos = p0; pos < p1; ++pos) {
      const int64_t t = a.order[pos];
      const int64_t j = a.trait[t], l = a.locus[t];
      if (j != cur) {
        cur = j;
        rss0 = weighted_basis<64, MDF_CMAX, true>(n, c, a.h2[j], a.lam, [&](int q, int i) { return a.Z0[(size_t)q * n + i]; },
                                                  a.Yt + j, a.ldy, Sw, Qb, eb, nullptr);
      }
      const double* xp = a.Xc + (size_t)l * K * n;
      int mask = 0;
      for (int q = 0; q < K; ++q) {
        double* col = Rb + (size_t)q * n;
        double x2 = 0.0;
        for (int i = lane; i < n; i += 64) {
          const double v = Sw[i] * xp[(size_t)q * n + i];
          col[i] = v;
          x2 = fma(v, v, x2);
        }
        x2 = eff_wsum(x2);
        project_out<64, MDF_CMAX, true>(col, Qb, c, n, nullptr);
        project_out<64, MDF_CMAX, true>(col, Qb, c, n, nullptr);
        double coef[K];
#pragma unroll
        for (int r = 0; r < K; ++r) coef[r] = 0.0;
        project_out<64, K, true>(col, Rb, q, n, nullptr, coef);   // the accepted u_b before it, or zero columns
        project_out<64, K, true>(col, Rb, q, n, nullptr, coef);
        const double nv = team_norm2<64, true>(col, n, nullptr);
        const bool acc = nv > MDF_TAU * x2;            // NaN / not above the threshold: dropped
        const double rqq = acc ? sqrt(nv) : 0.0;
        const double inv = acc ? 1.0 / rqq : 0.0;
        double ze = 0.0;
        for (int i = lane; i < n; i += 64) {
          const double u = acc ? col[i] * inv : 0.0;
          col[i] = u;
          ze = fma(u, eb[i], ze);
        }
        sz[q] = eff_wsum(ze);
        mask |= acc ? (1 << q) : 0;
#pragma unroll
        for (int r = 0; r < K; ++r) sR[r * K + q] = r < q ? (acc ? coef[r] : 0.0) : (r == q ? rqq : 0.0);
      }
      double rss1 = 0.0;
      for (int i = lane; i < n; i += 64) {
        double v = eb[i];
        for (int q = 0; q < K; ++q) v = fma(-sz[q], Rb[(size_t)q * n + i], v);
        rss1 = fma(v, v, rss1);
      }
      rss1 = eff_wsum(rss1);
      // beta = R^-1 z and the diagonal of R^-1 R^-T (back substitution)
      for (int q = K - 1; q >= 0; --q) {
        double s = sz[q];
        for (int r = q + 1; r < K; ++r) s = fma(-sR[q * K + r], sb[r], s);
        const double rqq = sR[q * K + q];
        sb[q] = rqq > 0.0 ? s / rqq : 0.0;
        sd[q] = 0.0;
      }
      for (int cc = 0; cc < K; ++cc) {                  // column cc of R^-1
        const bool on = sR[cc * K + cc] > 0.0;
        for (int q = cc; q >= 0; --q) {
          double s = q == cc ? 1.0 : 0.0;
          for (int r = q + 1; r <= cc; ++r) s = fma(-sR[q * K + r], si[r], s);
          const double rqq = sR[q * K + q];
          const double v = (on && rqq > 0.0) ? s / rqq : 0.0;
          si[q] = v;
          sd[q] = fma(v, v, sd[q]);
        }
      }
      const int r = __popc(mask);
      const double df = a.reml ? (double)(n - (c + r)) + prior_df : (double)n + prior_df;
      const double sigma2 = (rss1 + a.prior_a * a.prior_b) / df;
      const double ratio = rss1 / rss0;
      double lod;
      if (ratio > 0.0) lod = -0.5 * (double)n * log10(ratio);
      else if (ratio == 0.0) lod = INFINITY;
      else { lod = NAN; ++nnan; }
      if (lane == 0) {
#pragma unroll
        for (int q = 0; q < K; ++q) {
          a.beta[t * K + q] = sb[q];
          a.se[t * K + q] = sqrt(sigma2 * sd[q]);
        }
        a.sigma2[t] = sigma2; a.lod[t] = lod; a.accepted[t] = mask;
      }
    }
  }
  if (nnan && lane == 0) atomicAdd((unsigned long long*)&a.stat[ST_NAN_LOD], (unsigned long long)nnan);
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
// a.cnt: m + 2 ints, a.order: T ints
int launch_effects_sort(blmm_ctx* ctx, const EffArgs& a) {
  BLMM_HIP(hipMemsetAsync(a.cnt, 0, sizeof(int) * (size_t)(a.m + 2), ctx->stream));
  if (a.T <= 0) return BLMM_OK;
  const unsigned gt = (unsigned)((a.T + 255) / 256);
  hipLaunchKernelGGL(k_eff_hist, dim3(gt), dim3(256), 0, ctx->stream, a);
  KCHECK();
  hipLaunchKernelGGL(k_eff_scan, dim3(1), dim3(1024), 0, ctx->stream, a.cnt, a.m);
  KCHECK();
  hipLaunchKernelGGL(k_eff_scatter, dim3(gt), dim3(256), 0, ctx->stream, a);
  KCHECK();
  return BLMM_OK;
}

int launch_effects(blmm_ctx* ctx, EffArgs a) {
  if (a.T <= 0) return BLMM_OK;
  const int cus = ctx->num_cus > 0 ? ctx->num_cus : 256;
  // tests per wave: enough waves for every CU (32 each) before a wave takes a second test, at most 64 tests behind one trait part
  const int64_t want = (a.T + 32 * (int64_t)cus - 1) / (32 * (int64_t)cus);
  a.chunk = (int)(want < 1 ? 1 : want > 64 ? 64 : want);
  const int64_t nchunks = (a.T + a.chunk - 1) / a.chunk;
  const size_t per = (size_t)(a.c + 2 + a.k) * a.n;
  size_t lds = sizeof(double) * per;
  unsigned grid = (unsigned)nchunks;
  a.slab = nullptr;
  if (lds > EFF_LDS_MAX) {
    if (nchunks > 4 * (int64_t)cus) grid = (unsigned)(4 * cus);
    int rc = ensure(ctx, ctx->effSlab, sizeof(double) * per * grid);
    if (rc) return rc;
    a.slab = ptr<double>(ctx->effSlab);
    lds = 0;
  }
#define EF(K) hipLaunchKernelGGL(k_effects<K>, dim3(grid), dim3(64), lds, ctx->stream, a)
  switch (a.k) {
    case 1: EF(1); break; case 2: EF(2); break; case 3: EF(3); break; case 4: EF(4); break;
    case 5: EF(5); break; case 6: EF(6); break; case 7: EF(7); break; case 8: EF(8); break;
    default: return fail(ctx, BLMM_ERR_UNSUPPORTED, "bulkscan_effects: takes 1 <= k <= 8");
  }
#undef EF
  KCHECK();
  return BLMM_OK;
}

}  // namespace blmm
