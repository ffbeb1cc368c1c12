// math_probe.hip -- test-only probe of the fp64 / fp32 primitives of bulklmm.jl_amd/csrc/fastmath.h (tests/test_gpu_fastmath.py).
// It includes the library's own headers, so what runs here is the product's inline code, staged the way the kernels stage it:
// one value per lane, host buffers in and out, every HIP status returned (0 = hipSuccess).  Not part of the library.
#include "blmm_internal.h"
#include "fastmath.h"
#include <cmath>

using namespace blmm;

#define CK(x)                                       \
  do {                                              \
    const hipError_t e__ = (x);                     \
    if (e__ != hipSuccess) { rc = (int)e__; goto done; } \
  } while (0)

namespace {

constexpr int NT = 256;
constexpr int PV_N = BLMM_PV_TABLE_N * (BLMM_PV_STRIDE / 2);

unsigned blocks_for(int64_t n) { return (unsigned)((n + NT - 1) / NT); }

// kernels_scan.hip's epilogue for one value: lod_fast_ok ? fast_lod5 : lod_out_of_range; next to it the libm map of the re-scan
// kernels (kernels_dyn.hip, kernels_lowrank.hip): scale * log10(u)
struct Lod5Coef { double c[6]; };
__global__ void __launch_bounds__(NT) k_lod5(const double* __restrict__ u, double* __restrict__ out, double* __restrict__ libm_out,
                                            int64_t n, const double* __restrict__ lodtab, Lod5Coef cf, int counted,
                                            unsigned long long* __restrict__ nnan) {
  __shared__ dpair s_lod[BLMM_LOD_TABLE_N];
  LodStage<NT> st;
  lod_stage_load<NT>(st, lodtab);
  lod_stage_store<NT>(st, s_lod, cf.c[0]);
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const double scale = cf.c[0];
  const LodPoly5 lp = lod_poly5_of(cf.c);
  const double x = u[i];
  int cnt = 0;
  out[i] = lod_fast_ok(x) ? fast_lod5(x, s_lod, lp) : lod_out_of_range(x, s_lod, lp, scale, counted != 0, &cnt);
  libm_out[i] = scale * log10(x);
  if (cnt) atomicAdd(nnan, (unsigned long long)cnt);
}

// fast_log<false>, fast_log<true> and fast_lod (scale folded into the table, make_lod_poly)
__global__ void __launch_bounds__(NT) k_log(const double* __restrict__ x, double* __restrict__ ln_out, double* __restrict__ lg_out,
                                           double* __restrict__ lod_out, int64_t n, const double* __restrict__ logtab, double scale) {
  __shared__ dpair s_ln[BLMM_LOG_TABLE_N], s_lg[BLMM_LOG_TABLE_N], s_lod[BLMM_LOG_TABLE_N];
  stage_log_table<false>(s_ln, logtab);
  stage_log_table<true>(s_lg, logtab);
  stage_lod_table(s_lod, logtab, scale);
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const LodPoly P = make_lod_poly(scale);
  ln_out[i] = fast_log<false>(x[i], s_ln);
  lg_out[i] = fast_log<true>(x[i], s_lg);
  lod_out[i] = fast_lod(x[i], s_lod, P);
}

__global__ void __launch_bounds__(NT) k_rcp(const double* __restrict__ x, double* __restrict__ o, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const double v = x[i];
  o[4 * i + 0] = fast_rcp(v);
  o[4 * i + 1] = fast_rcp1(v);
  o[4 * i + 2] = nr_rsqrt(v);
  o[4 * i + 3] = fast_rsqrt(v);
}

__global__ void __launch_bounds__(NT) k_log10p1(const double* __restrict__ lod, double* __restrict__ out, int64_t n,
                                               const double* __restrict__ pvtab) {
  __shared__ dpair s_pv[PV_N];
  PvStage<NT> st;
  pv_stage_load<NT>(st, pvtab);
  pv_stage_store<NT>(st, s_pv);
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  out[i] = fast_log10p1(lod[i], s_pv);
}

// Every fp32 r^2 with bits in [b0, b0 + count) through lod_f32 against scale_ref * log1p(-(double) r^2), reduced on the device:
// per block {worst err / (1e-3 |ref| + 1e-4), its bits, worst relative error where ref >= 1, its bits}.  A value whose finiteness
// differs from the reference's counts as an infinite error.
__global__ void __launch_bounds__(NT) k_f32_scan(uint32_t b0, int64_t count, float scale, double scale_ref, double* __restrict__ part,
                                                unsigned long long* __restrict__ nnan) {
  __shared__ double s_v[2][NT];
  __shared__ uint32_t s_a[2][NT];
  double wr = -1.0, wl = -1.0;
  uint32_t ar = 0, al = 0;
  int cnt = 0;
  for (int64_t k = (int64_t)blockIdx.x * NT + threadIdx.x; k < count; k += (int64_t)gridDim.x * NT) {
    const uint32_t bits = b0 + (uint32_t)k;
    const float r2 = __uint_as_float(bits);
    const double got = (double)lod_f32(r2, scale, true, &cnt);
    const double ref = scale_ref * log1p(-(double)r2);
    double ratio, rel = -1.0;
    if (ref == got) ratio = 0.0;
    else if (!isfinite(ref) || !isfinite(got)) ratio = INFINITY;
    else {
      const double d = fabs(got - ref);
      ratio = d / fma(1e-3, fabs(ref), 1e-4);
      if (fabs(ref) >= 1.0) rel = d / fabs(ref);
    }
    if (ref == got && isfinite(ref) && fabs(ref) >= 1.0) rel = 0.0;
    if (ratio > wr) { wr = ratio; ar = bits; }
    if (rel > wl) { wl = rel; al = bits; }
  }
  if (cnt) atomicAdd(nnan, (unsigned long long)cnt);
  s_v[0][threadIdx.x] = wr; s_a[0][threadIdx.x] = ar;
  s_v[1][threadIdx.x] = wl; s_a[1][threadIdx.x] = al;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      for (int q = 0; q < 2; ++q)
        if (s_v[q][threadIdx.x + s] > s_v[q][threadIdx.x]) { s_v[q][threadIdx.x] = s_v[q][threadIdx.x + s]; s_a[q][threadIdx.x] = s_a[q][threadIdx.x + s]; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    part[4 * blockIdx.x + 0] = s_v[0][0]; part[4 * blockIdx.x + 1] = (double)s_a[0][0];
    part[4 * blockIdx.x + 2] = s_v[1][0]; part[4 * blockIdx.x + 3] = (double)s_a[1][0];
  }
}

// One workgroup of T threads stages both tables through the split load / store pair into LDS pre-filled with `fill`, with PAD
// entries of guard beyond each table; the whole of both LDS arrays, guards included, is copied out.
constexpr int PAD = 64;
template <int T>
__global__ void __launch_bounds__(T) k_stage(const double* __restrict__ lodtab, const double* __restrict__ pvtab, double scale, double fill,
                                             double* __restrict__ lod_out, double* __restrict__ pv_out) {
  __shared__ dpair s_lod[BLMM_LOD_TABLE_N + PAD], s_pv[PV_N + PAD];
  for (int i = threadIdx.x; i < BLMM_LOD_TABLE_N + PAD; i += T) s_lod[i] = (dpair){fill, fill};
  for (int i = threadIdx.x; i < PV_N + PAD; i += T) s_pv[i] = (dpair){fill, fill};
  __syncthreads();
  LodStage<T> ls;
  PvStage<T> ps;
  lod_stage_load<T>(ls, lodtab);
  pv_stage_load<T>(ps, pvtab);
  lod_stage_store<T>(ls, s_lod, scale);
  pv_stage_store<T>(ps, s_pv);
  __syncthreads();
  for (int i = threadIdx.x; i < BLMM_LOD_TABLE_N + PAD; i += T) { lod_out[2 * i] = s_lod[i][0]; lod_out[2 * i + 1] = s_lod[i][1]; }
  for (int i = threadIdx.x; i < PV_N + PAD; i += T) { pv_out[2 * i] = s_pv[i][0]; pv_out[2 * i + 1] = s_pv[i][1]; }
}

template <typename T>
hipError_t upload(T** d, const T* h, size_t count) {
  hipError_t e = hipMalloc(reinterpret_cast<void**>(d), sizeof(T) * (count ? count : 1));
  if (e == hipSuccess && count) e = hipMemcpy(*d, h, sizeof(T) * count, hipMemcpyHostToDevice);
  return e;
}
template <typename T>
hipError_t alloc(T** d, size_t count) { return hipMalloc(reinterpret_cast<void**>(d), sizeof(T) * (count ? count : 1)); }

}  // namespace

extern "C" {

// out[i] = the scan epilogue's LOD of u[i] at scale (-n / 2); libm_out[i] = scale * log10(u[i]); *nnan_out = lod_out_of_range's count
int probe_lod5(const double* u, double* out, double* libm_out, int64_t n, double scale, int counted, int64_t* nnan_out) {
  int rc = 0;
  double *du = nullptr, *dout = nullptr, *dlibm = nullptr, *dtab = nullptr;
  unsigned long long* dcnt = nullptr;
  Lod5Coef cf;
  lod_poly5_host(scale, cf.c);
  CK(upload(&du, u, (size_t)n));
  CK(alloc(&dout, (size_t)n));
  CK(alloc(&dlibm, (size_t)n));
  CK(upload(&dtab, blmm_lod_table_host, (size_t)BLMM_LOD_TABLE_N * 2));
  CK(alloc(&dcnt, 1));
  CK(hipMemset(dcnt, 0, sizeof(unsigned long long)));
  if (n > 0) {
    hipLaunchKernelGGL(k_lod5, dim3(blocks_for(n)), dim3(NT), 0, 0, du, dout, dlibm, n, dtab, cf, counted, dcnt);
    CK(hipGetLastError());
  }
  CK(hipMemcpy(out, dout, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  CK(hipMemcpy(libm_out, dlibm, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  CK(hipMemcpy(nnan_out, dcnt, sizeof(int64_t), hipMemcpyDeviceToHost));
done:
  (void)hipFree(du); (void)hipFree(dout); (void)hipFree(dlibm); (void)hipFree(dtab); (void)hipFree(dcnt);
  return rc;
}

// ln_out = fast_log<false>(x), lg_out = fast_log<true>(x), lod_out = fast_lod(x) with the table and polynomial scaled by `scale`
int probe_log(const double* x, double* ln_out, double* lg_out, double* lod_out, int64_t n, double scale) {
  int rc = 0;
  double *dx = nullptr, *dln = nullptr, *dlg = nullptr, *dlod = nullptr, *dtab = nullptr;
  CK(upload(&dx, x, (size_t)n));
  CK(alloc(&dln, (size_t)n));
  CK(alloc(&dlg, (size_t)n));
  CK(alloc(&dlod, (size_t)n));
  CK(upload(&dtab, blmm_log_table_host, (size_t)BLMM_LOG_TABLE_N * 3));
  if (n > 0) {
    hipLaunchKernelGGL(k_log, dim3(blocks_for(n)), dim3(NT), 0, 0, dx, dln, dlg, dlod, n, dtab, scale);
    CK(hipGetLastError());
  }
  CK(hipMemcpy(ln_out, dln, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  CK(hipMemcpy(lg_out, dlg, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  CK(hipMemcpy(lod_out, dlod, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
done:
  (void)hipFree(dx); (void)hipFree(dln); (void)hipFree(dlg); (void)hipFree(dlod); (void)hipFree(dtab);
  return rc;
}

// out[4 i .. 4 i + 3] = fast_rcp, fast_rcp1, nr_rsqrt, fast_rsqrt of x[i]
int probe_rcp(const double* x, double* out, int64_t n) {
  int rc = 0;
  double *dx = nullptr, *dout = nullptr;
  CK(upload(&dx, x, (size_t)n));
  CK(alloc(&dout, (size_t)n * 4));
  if (n > 0) {
    hipLaunchKernelGGL(k_rcp, dim3(blocks_for(n)), dim3(NT), 0, 0, dx, dout, n);
    CK(hipGetLastError());
  }
  CK(hipMemcpy(out, dout, sizeof(double) * (size_t)n * 4, hipMemcpyDeviceToHost));
done:
  (void)hipFree(dx); (void)hipFree(dout);
  return rc;
}

// out[i] = fast_log10p1(lod[i]) with the p-value table staged by pv_stage_load / pv_stage_store
int probe_log10p1(const double* lod, double* out, int64_t n) {
  int rc = 0;
  double *dl = nullptr, *dout = nullptr, *dtab = nullptr;
  CK(upload(&dl, lod, (size_t)n));
  CK(alloc(&dout, (size_t)n));
  CK(upload(&dtab, blmm_pv_table_host, (size_t)BLMM_PV_TABLE_N * BLMM_PV_STRIDE));
  if (n > 0) {
    hipLaunchKernelGGL(k_log10p1, dim3(blocks_for(n)), dim3(NT), 0, 0, dl, dout, n, dtab);
    CK(hipGetLastError());
  }
  CK(hipMemcpy(out, dout, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
done:
  (void)hipFree(dl); (void)hipFree(dout); (void)hipFree(dtab);
  return rc;
}

// lod_f32 over the fp32 r^2 bit patterns [b0, b0 + count); part_out: nblocks x {ratio, bits, rel, bits} (see k_f32_scan)
int probe_f32_scan(uint32_t b0, int64_t count, float scale, double scale_ref, int nblocks, double* part_out, int64_t* nnan_out) {
  int rc = 0;
  double* dpart = nullptr;
  unsigned long long* dcnt = nullptr;
  if (nblocks < 1 || count < 0 || b0 + (uint64_t)count > 0x100000000ull) return (int)hipErrorInvalidValue;
  CK(alloc(&dpart, (size_t)nblocks * 4));
  CK(alloc(&dcnt, 1));
  CK(hipMemset(dcnt, 0, sizeof(unsigned long long)));
  hipLaunchKernelGGL(k_f32_scan, dim3((unsigned)nblocks), dim3(NT), 0, 0, b0, count, scale, scale_ref, dpart, dcnt);
  CK(hipGetLastError());
  CK(hipMemcpy(part_out, dpart, sizeof(double) * (size_t)nblocks * 4, hipMemcpyDeviceToHost));
  CK(hipMemcpy(nnan_out, dcnt, sizeof(int64_t), hipMemcpyDeviceToHost));
done:
  (void)hipFree(dpart); (void)hipFree(dcnt);
  return rc;
}

// LDS after lod_stage_load/store<nt> and pv_stage_load/store<nt>: lod_out (BLMM_LOD_TABLE_N + pad) x 2, pv_out (PV_N + pad) x 2
// doubles; *pad_out = the guard entries past each table, which must still hold `fill`
int probe_stage(int nt, double scale, double fill, double* lod_out, double* pv_out, int* pad_out) {
  int rc = 0;
  double *dlt = nullptr, *dpt = nullptr, *dlo = nullptr, *dpo = nullptr;
  *pad_out = PAD;
  CK(upload(&dlt, blmm_lod_table_host, (size_t)BLMM_LOD_TABLE_N * 2));
  CK(upload(&dpt, blmm_pv_table_host, (size_t)BLMM_PV_TABLE_N * BLMM_PV_STRIDE));
  CK(alloc(&dlo, (size_t)(BLMM_LOD_TABLE_N + PAD) * 2));
  CK(alloc(&dpo, (size_t)(PV_N + PAD) * 2));
  switch (nt) {
    case 64: hipLaunchKernelGGL(k_stage<64>, dim3(1), dim3(64), 0, 0, dlt, dpt, scale, fill, dlo, dpo); break;
    case 128: hipLaunchKernelGGL(k_stage<128>, dim3(1), dim3(128), 0, 0, dlt, dpt, scale, fill, dlo, dpo); break;
    case 256: hipLaunchKernelGGL(k_stage<256>, dim3(1), dim3(256), 0, 0, dlt, dpt, scale, fill, dlo, dpo); break;
    case 512: hipLaunchKernelGGL(k_stage<512>, dim3(1), dim3(512), 0, 0, dlt, dpt, scale, fill, dlo, dpo); break;
    case 1024: hipLaunchKernelGGL(k_stage<1024>, dim3(1), dim3(1024), 0, 0, dlt, dpt, scale, fill, dlo, dpo); break;
    default: rc = (int)hipErrorInvalidValue; goto done;
  }
  CK(hipGetLastError());
  CK(hipMemcpy(lod_out, dlo, sizeof(double) * (size_t)(BLMM_LOD_TABLE_N + PAD) * 2, hipMemcpyDeviceToHost));
  CK(hipMemcpy(pv_out, dpo, sizeof(double) * (size_t)(PV_N + PAD) * 2, hipMemcpyDeviceToHost));
done:
  (void)hipFree(dlt); (void)hipFree(dpt); (void)hipFree(dlo); (void)hipFree(dpo);
  return rc;
}

}  // extern "C"
