// kernels_loco.hip -- leave-one-chromosome-out kinships (blmm_kinship_loco, blmm_bulkscan_loco).
//
// calcKinship (src/kinship.jl:4-14) is linear in the markers: with X = G - 1/2 and S_d = X_d X_d' over the markers of chromosome d,
//   K_{-c} = 2 (sum_{d != c} S_d) / (p - p_c) + 1/2,   diagonal 1.
// Stage 1 (k_kinship_loco_partial) forms every S_d in one pass over G: the 32 x 32 lower tiles of k_kinship_partial, grid.z =
// chromosome x split of its markers (deterministic, no atomics).  Stage 2 (k_kinship_loco_final) sums, per matrix entry, the other
// chromosomes' blocks in a fixed order -- the suffix sum over d > c parked in K_out[c] on a first sweep, the prefix sum over d < c
// carried on the second -- never S - S_c, which cancels badly.
#include "blmm_internal.h"
#include <cmath>

namespace blmm {

#define KCHECK()                                                                                      \
  do {                                                                                                \
    hipError_t e__ = hipGetLastError();                                                               \
    if (e__ != hipSuccess) return fail(ctx, BLMM_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e__)); \
  } while (0)

namespace {

// block (ti, tj, z): z = c * nsplit + q, split q of chromosome c's markers; part[(z n + j) n + i] = sum over that split of x_ik x_jk
__global__ void __launch_bounds__(256) k_kinship_loco_partial(const double* __restrict__ G, int64_t n, const int64_t* __restrict__ chr,
                                                              int nsplit, double* __restrict__ part) {
  __shared__ double sa[32][33], sb[32][33];
  const int ti = blockIdx.x, tj = blockIdx.y, z = blockIdx.z;
  if (tj > ti) return;  // symmetric: lower tiles only
  const int c = z / nsplit, q = z - c * nsplit;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int64_t c0 = chr[c], c1 = chr[c + 1];
  const int64_t chunk = (c1 - c0 + nsplit - 1) / nsplit;
  const int64_t k0 = c0 + q * chunk, k1 = (k0 + chunk < c1) ? k0 + chunk : c1;
  double acc[4] = {0, 0, 0, 0};
  for (int64_t kb = k0; kb < k1; kb += 32) {
    for (int r = ty; r < 32; r += 8) {
      const int64_t k = kb + r;
      const int64_t ia = (int64_t)ti * 32 + tx, ib = (int64_t)tj * 32 + tx;
      sa[r][tx] = (k < k1 && ia < n) ? G[k * n + ia] - 0.5 : 0.0;
      sb[r][tx] = (k < k1 && ib < n) ? G[k * n + ib] - 0.5 : 0.0;
    }
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < 32; ++r) {
      const double a = sa[r][tx];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = fma(a, sb[r][ty + 8 * u], acc[u]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t i = (int64_t)ti * 32 + tx, j = (int64_t)tj * 32 + ty + 8 * u;
    if (i < n && j < n) part[((int64_t)z * n + j) * n + i] = acc[u];
  }
}

// one thread per entry (i, j) of all nchr matrices; scale > 0: rounded to 1/scale as k_round_digits does
__global__ void k_kinship_loco_final(const double* __restrict__ part, int64_t n, const int64_t* __restrict__ chr, int nchr, int nsplit,
                                     double scale, double* __restrict__ K) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nn = n * n;
  if (e >= nn) return;
  int64_t i = e % n, j = e / n;
  if (i == j) {
    const double one = scale > 0.0 ? rint(1.0 * scale) / scale : 1.0;
    for (int c = 0; c < nchr; ++c) K[(int64_t)c * nn + e] = one;
    return;
  }
  if (i / 32 < j / 32) { const int64_t t = i; i = j; j = t; }  // only lower tiles were computed
  auto block = [&](int d) {
    double s = 0.0;
    for (int q = 0; q < nsplit; ++q) s += part[(((int64_t)d * nsplit + q) * n + j) * n + i];
    return s;
  };
  double suf = 0.0;                                   // sum over d > c, parked in K[c]
  for (int c = nchr - 1; c >= 0; --c) { K[(int64_t)c * nn + e] = suf; suf += block(c); }
  double pre = 0.0;                                   // sum over d < c
  const int64_t p = chr[nchr];
  for (int c = 0; c < nchr; ++c) {
    const double s = pre + K[(int64_t)c * nn + e];
    const double v = 2.0 * s / (double)(p - (chr[c + 1] - chr[c])) + 0.5;
    K[(int64_t)c * nn + e] = scale > 0.0 ? rint(v * scale) / scale : v;
    pre += block(c);
  }
}

}  // namespace

// dchr: the nchr + 1 offsets on the device.  The splits per chromosome (1 .. 8) keep the partial sums within 256 MiB where they can
// (BXD: 8; n = 1000 with 20 chromosomes: 1): the workspace is at most 256 MiB or the size of the output (nchr n^2 doubles), the
// larger of the two; nchr * nsplit stays within grid.z's 65535.
int loco_kinship_splits(int64_t n, int64_t nchr) {
  const double per = (double)nchr * (double)n * (double)n * sizeof(double);
  int s = (int)((256.0 * 1024 * 1024) / per);
  s = s < 1 ? 1 : (s > 8 ? 8 : s);
  while (s > 1 && nchr * s > 65535) --s;
  return s;
}

int launch_kinship_loco(blmm_ctx* ctx, const double* dG, int64_t n, const int64_t* dchr, int64_t nchr, int64_t digits, double* dK,
                        double* partial, int nsplit) {
  const unsigned nt = (unsigned)((n + 31) / 32);
  const int64_t nz = nchr * nsplit;
  if (nz > 65535) return fail(ctx, BLMM_ERR_UNSUPPORTED, "kinship_loco: more than 65535 chromosome blocks");
  hipLaunchKernelGGL(k_kinship_loco_partial, dim3(nt, nt, (unsigned)nz), dim3(256), 0, ctx->stream, dG, n, dchr, nsplit, partial);
  KCHECK();
  // beyond 17 digits rounding a double changes nothing (and 10^digits would overflow): as blmm_kinship_rounded
  const double scale = (digits >= 0 && digits <= 17) ? std::pow(10.0, (double)digits) : 0.0;
  hipLaunchKernelGGL(k_kinship_loco_final, dim3((unsigned)((n * n + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)partial, n, dchr,
                     (int)nchr, nsplit, scale, dK);
  KCHECK();
  return BLMM_OK;
}

}  // namespace blmm
