// blmm_api.hip -- C ABI (include/bulklmm_hip.h) and the host orchestration of the bulkscan pipeline:
//   design -> eigen (device Jacobi) -> rotation GEMM -> null-model h2 (Brent / grid) -> panels -> LOD kernels.
// Mirrors bulkscan / bulkscan_null / bulkscan_null_grid / bulkscan_alt_grid (src/bulkscan.jl) and
// scan_perms_lite (src/scan.jl:485-557) of BulkLMM.jl; nothing here falls back to a CPU path.
#include "blmm_internal.h"
#include "fastmath.h"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <chrono>
#include <cstring>
#include <limits>
#include <cstdlib>
#include <mutex>

using namespace blmm;

namespace blmm {

int fail(blmm_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}

int ensure(blmm_ctx* ctx, DevBuf& b, size_t bytes) {
  // whoever asks for the output buffer is about to overwrite (or reallocate) it: the blmm_last_* consumers must not see the
  // previous call's matrix through it.  The entry points set last_L again once their own result is in place.
  if (&b == &ctx->outL) clear_last(ctx);
  if (&b == &ctx->outL || &b == &ctx->outP) ctx->last_P = nullptr;
  if (bytes == 0) bytes = 8;
  if (b.cap >= bytes) return BLMM_OK;
  if (b.p) {
    // outstanding work may still use the old buffer
    hipStreamSynchronize(ctx->stream);
    hipFree(b.p);
    b.p = nullptr; b.cap = 0;
  }
  size_t want = bytes + bytes / 8 + 256;
  hipError_t e = hipMalloc(&b.p, want);
  if (e != hipSuccess) {
    b.p = nullptr;
    return fail(ctx, BLMM_ERR_ALLOC, std::string("hipMalloc(") + std::to_string(want) + "): " + hipGetErrorString(e));
  }
  b.cap = want;
  return BLMM_OK;
}

namespace {
std::mutex g_grid_mu[64];           // one per device: held across wait -> launch -> record (GridKernelGuard)
hipEvent_t g_grid_ev[64];
bool g_grid_has[64];
}  // namespace

GridKernelGuard::GridKernelGuard(blmm_ctx* c) : ctx(c), dev(c->device & 63) {
  g_grid_mu[dev].lock();
  if (g_grid_has[dev] && hipStreamWaitEvent(ctx->stream, g_grid_ev[dev], 0) != hipSuccess)
    rc = fail(ctx, BLMM_ERR_HIP, "hipStreamWaitEvent (grid-kernel order) failed");
}

int GridKernelGuard::record() {
  if (!g_grid_has[dev]) {
    if (hipEventCreateWithFlags(&g_grid_ev[dev], hipEventDisableTiming) != hipSuccess)
      return fail(ctx, BLMM_ERR_HIP, "hipEventCreate (grid-kernel order) failed");
    g_grid_has[dev] = true;
  }
  if (hipEventRecord(g_grid_ev[dev], ctx->stream) != hipSuccess)
    return fail(ctx, BLMM_ERR_HIP, "hipEventRecord (grid-kernel order) failed");
  return BLMM_OK;
}

GridKernelGuard::~GridKernelGuard() { g_grid_mu[dev].unlock(); }

__global__ void k_fill(double* p, int64_t n, double v) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
// column-major n x ncols  ->  row-major npad x ld (zero padded)
__global__ void k_to_rowmajor(const double* __restrict__ In, int n, int64_t ncols, double* __restrict__ Out, int npad, int64_t ld) {
  __shared__ double tile[32][33];
  const int64_t c0 = (int64_t)blockIdx.x * 32;
  const int r0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int cc = ty; cc < 32; cc += 8) {
    const int64_t col = c0 + cc; const int row = r0 + tx;
    tile[cc][tx] = (row < n && col < ncols) ? In[col * n + row] : 0.0;
  }
  __syncthreads();
  for (int rr = ty; rr < 32; rr += 8) {
    const int row = r0 + rr; const int64_t col = c0 + tx;
    if (row < npad && col < ld) Out[(int64_t)row * ld + col] = tile[tx][rr];
  }
}

// Copies the device-side "gave up" conditions of a call into the context's pinned host word (system-scope store):
// bit 0: the multi-workgroup weight-basis kernel timed out at its grid barrier (stat[ST_LR_RANK] < 0);
// bit 1: the eigensolver gave up (stat[ST_EIG_ABORT]: -7 grid barrier of the tridiagonalisation timed out, -8 QL iteration limit).
__global__ void k_sticky(const int64_t* __restrict__ stat, int64_t* hflag) {
  int64_t f = 0;
  if (stat[ST_LR_RANK] < 0) f |= 1;
  if (stat[ST_EIG_ABORT] != 0) { f |= 2; hflag[1] = stat[ST_EIG_ABORT]; }      // the code itself: -7 / -8, the own solver's aborts
  if (f) __hip_atomic_fetch_or(hflag, f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace blmm

namespace {

// A device-side failure of an EARLIER call made without a blmm_status (nothing synchronised then) surfaces here.
int check_sticky(blmm_ctx* ctx) {
  if (!ctx->hflag) return BLMM_OK;
  const int64_t f = *ctx->hflag;
  if (!f) return BLMM_OK;
  *ctx->hflag = 0;
  if (f & 1) return fail(ctx, BLMM_ERR_HIP, "a call failed on the device: the weight-basis kernel timed out at its grid barrier (its LOD output is NaN)");
  const long long code = (long long)ctx->hflag[1];
  return fail(ctx, BLMM_ERR_HIP, "a call failed on the device: the eigensolver did not converge (code " + std::to_string(code) +
                                 ": -7 grid barrier of the tridiagonalisation timed out, -8 QL iteration limit)");
}

// The prologue of every device entry point once its arguments are checked: select the device, then report an earlier failure
int enter_device(blmm_ctx* ctx) {
  BLMM_HIP(hipSetDevice(ctx->device));
  return check_sticky(ctx);
}

// The launchers enqueue on ctx->stream: an OnStream points it at another stream for its scope and restores it on every exit
struct OnStream {
  blmm_ctx* ctx; hipStream_t prev;
  OnStream(blmm_ctx* c, hipStream_t s) : ctx(c), prev(c->stream) { c->stream = s; }
  ~OnStream() { ctx->stream = prev; }
  OnStream(const OnStream&) = delete;
  OnStream& operator=(const OnStream&) = delete;
};

struct Timer {
  blmm_ctx* ctx; blmm_ctx::EvSet* set = nullptr;
  explicit Timer(blmm_ctx* c) : ctx(c) {
    if (!ctx->timing) return;
    if (ctx->ev_used >= 4096) ctx->ev_used = 0;  // nobody is reading: recycle
    if (ctx->ev_used == ctx->evsets.size()) {
      blmm_ctx::EvSet s; s.n = 0;
      for (auto& e : s.e) (void)hipEventCreate(&e);
      ctx->evsets.push_back(s);
    }
    set = &ctx->evsets[ctx->ev_used++];
    set->n = 0;
  }
  void mark() { if (set && set->n < 8) (void)hipEventRecord(set->e[set->n++], ctx->stream); }
};

// phase times of one event set; marks: 0 start, 1 eigen done, 2 rotate done, 3 h2 done, 4 prep done, 5 scan done
void phase_times(const blmm_ctx::EvSet& s, double out[6]) {
  for (int i = 0; i < 6; ++i) out[i] = 0.0;
  for (int i = 0; i + 1 < s.n && i < 5; ++i) { float ms = 0; (void)hipEventElapsedTime(&ms, s.e[i], s.e[i + 1]); out[i] = ms; }
  if (s.n >= 2) { float tot = 0; (void)hipEventElapsedTime(&tot, s.e[0], s.e[s.n - 1]); out[5] = tot; }
}

int to_rowmajor(blmm_ctx* ctx, const double* In, int n, int64_t ncols, double* Out, int npad, int64_t ld) {
  dim3 grid((unsigned)((ld + 31) / 32), (unsigned)((npad + 31) / 32));
  hipLaunchKernelGGL(k_to_rowmajor, grid, dim3(256), 0, ctx->stream, In, n, ncols, Out, npad, ld);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(ctx, BLMM_ERR_HIP, std::string("k_to_rowmajor: ") + hipGetErrorString(e));
  return BLMM_OK;
}

int fill(blmm_ctx* ctx, double* p, int64_t n, double v) {
  if (n <= 0) return BLMM_OK;
  hipLaunchKernelGGL(k_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, p, n, v);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(ctx, BLMM_ERR_HIP, std::string("k_fill: ") + hipGetErrorString(e));
  return BLMM_OK;
}

int check_opts(blmm_ctx* ctx, const blmm_opts* o) {
  if (!o) return fail(ctx, BLMM_ERR_INVALID, "opts is NULL");
  if (o->decomp_scheme != BLMM_EIGEN && o->decomp_scheme != BLMM_SVD)
    return fail(ctx, BLMM_ERR_DECOMP, "Please choose either `eigen` or `svd` for decomposition of the kinship matrix.");
  return BLMM_OK;
}

int check_method(blmm_ctx* ctx, const blmm_opts* o) {
  if (o->method != BLMM_NULL_EXACT && o->method != BLMM_NULL_GRID && o->method != BLMM_ALT_GRID)
    return fail(ctx, BLMM_ERR_METHOD, "Unknown method; choose null-exact, null-grid or alt-grid.");
  return BLMM_OK;
}

// the host side of a fresh status block; the device words are zeroed by reset_stat's fill or by the call's first kernel
// (prepare_eigen: k_eigf_reduce<true>)
int reset_stat_host(blmm_ctx* ctx, int64_t** stat) {
  int rc = ensure(ctx, ctx->stat, sizeof(int64_t) * NSTAT);
  if (rc) return rc;
  *stat = ptr<int64_t>(ctx->stat);
  ctx->audit_ran = false;
  ctx->brent_cnt_used = false;
  return BLMM_OK;
}
int reset_stat(blmm_ctx* ctx, int64_t** stat) {
  int rc = reset_stat_host(ctx, stat);
  if (rc) return rc;
  BLMM_HIP(hipMemsetAsync(*stat, 0, sizeof(int64_t) * NSTAT, ctx->stream));
  return BLMM_OK;
}

// Synchronises and fills *status (only when the caller asked for it).
// *st from one call's status block h (on the host); fails on the device-side aborts it records
int fill_status(blmm_ctx* ctx, const int64_t* h, blmm_status* st) {
  std::memset(st, 0, sizeof(*st));
  st->n_neg_eig = h[ST_NEG_EIG];
  st->n_nonpos_weight = h[ST_NONPOS_W];
  st->n_zero_norm = h[ST_ZERO_NORM];
  st->n_nan_lod = h[ST_NAN_LOD];
  st->n_brent_maxiter = h[ST_BRENT_MAXIT];
  st->jacobi_sweeps = h[ST_JACOBI_SWEEPS];
  st->jacobi_cycles = h[ST_EIG_CYCLES]; st->jacobi_ticks_100mhz = h[ST_EIG_TICKS];
  st->lowrank_rank = h[ST_LR_RANK];
  st->lowrank_fallback = h[ST_LR_FIX];
  st->lowrank_shared = h[ST_LR_SHARED0] + h[ST_LR_SHARED1];
  st->n_h2_boundary = h[ST_H2_BOUNDARY];
  st->n_h2_multimodal = ctx->audit_ran ? h[ST_H2_MULTIMODAL] : -1;
  st->n_illcond_rescan = h[ST_ILLCOND];
  if (h[ST_LR_RANK] < 0) return fail(ctx, BLMM_ERR_HIP, "weight-basis kernel: a workgroup timed out at the grid barrier");
  if (h[ST_EIG_ABORT] != 0) return fail(ctx, BLMM_ERR_HIP, "the eigensolver did not converge (code " + std::to_string((long long)h[ST_EIG_ABORT]) +
                              ": -7 grid barrier of the tridiagonalisation timed out, -8 QL iteration limit)");
  if (ctx->hflag && *ctx->hflag) return check_sticky(ctx);
  { double r2; std::memcpy(&r2, &h[ST_LR_RESID2], sizeof(double)); st->lowrank_resid = std::sqrt(r2 < 0 ? 0.0 : r2); }
  return BLMM_OK;
}

// blmm_bulkscan_loco's sum over its chromosomes: the counts add up, the weight basis's rank and residual are the largest
void add_status(blmm_status* sum, const blmm_status& one) {
  sum->n_neg_eig += one.n_neg_eig; sum->n_nonpos_weight += one.n_nonpos_weight; sum->n_zero_norm += one.n_zero_norm;
  sum->n_nan_lod += one.n_nan_lod; sum->n_brent_maxiter += one.n_brent_maxiter; sum->jacobi_sweeps += one.jacobi_sweeps;
  sum->jacobi_cycles += one.jacobi_cycles; sum->jacobi_ticks_100mhz += one.jacobi_ticks_100mhz;
  sum->lowrank_rank = std::max(sum->lowrank_rank, one.lowrank_rank);
  sum->lowrank_fallback += one.lowrank_fallback; sum->lowrank_shared += one.lowrank_shared;
  sum->lowrank_resid = std::max(sum->lowrank_resid, one.lowrank_resid);
  sum->n_h2_boundary += one.n_h2_boundary; sum->n_h2_multimodal += one.n_h2_multimodal; sum->n_illcond_rescan += one.n_illcond_rescan;
}

// adds the phase times of one call's event set to *st; returns its total (phase_times: out[5])
double add_phase_times(blmm_status* st, const Timer& tm) {
  if (!tm.set || tm.set->n < 2) return 0.0;
  double t[6];
  phase_times(*tm.set, t);
  st->t_eigen_ms += t[0]; st->t_rotate_ms += t[1]; st->t_h2_ms += t[2]; st->t_prep_ms += t[3]; st->t_scan_ms += t[4];
  return t[5];
}

int finish_status(blmm_ctx* ctx, blmm_status* st, Timer* tm) {
  if (!st) return BLMM_OK;
  int64_t h[NSTAT];
  BLMM_HIP(hipMemcpyAsync(h, ctx->stat.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  BLMM_HIP(hipStreamSynchronize(ctx->stream));
  int rc = fill_status(ctx, h, st);
  if (rc) return rc;
  if (tm) st->t_total_ms = add_phase_times(st, *tm);
  return BLMM_OK;
}

// Every bulkscan / scan call ends here.  Large-n calls (multi-workgroup weight basis, vendor eigensolver) first copy
// their device-side failure conditions into the sticky host word, so that they are reported even without a status.
int end_call(blmm_ctx* ctx, const Pipe& P, blmm_status* st, Timer* tm) {
  if (P.big && ctx->hflag && P.stat) {
    hipLaunchKernelGGL(k_sticky, dim3(1), dim3(1), 0, ctx->stream, P.stat, const_cast<int64_t*>(ctx->hflag));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, BLMM_ERR_HIP, std::string("k_sticky: ") + hipGetErrorString(e));
  }
  return finish_status(ctx, st, tm);
}

// The eigen phase of one matrix done ahead by a batched launch (blmm_bulkscan_loco: launch_eig_fast_batch over the weighted kinships
// Ks, with their own vectors, eigenvalues and status words, which the design of the call has filled and zeroed): prepare_eigen then
// runs only what follows the fast solver -- the Jacobi behind it (a no-op when its checks passed) and the post-eigen work.
struct EigPre { double* Ks; double* V; double* lraw; int64_t* stat; };

// The null model's covariates: none given (ncov == 0 or no matrix) is bulkscan(Y, G, K)'s intercept-only model.  c: the columns
// incl. the intercept
struct NullCov { const double* d; int64_t ncov; int add_int; int64_t c; };
NullCov null_cov(const blmm_opts* o, const double* dCovar, int64_t ncov) {
  if (ncov == 0 || !dCovar) return {nullptr, 0, 1, 1};
  const int add_int = o->add_intercept ? 1 : 0;
  return {dCovar, ncov, add_int, ncov + add_int};
}

// design -> eigen (prepare_eigen) -> rotation of Y and G (prepare_rotate).  centered = 1: the rotation also removes the
// unweighted projection on the null covariates (kernels_prep.hip:k_post_eigen).
int prepare_eigen(blmm_ctx* ctx, const blmm_opts* o, int64_t n, const double* dCovar, int64_t ncov, const double* dK,
                  const double* dweights, int centered, Pipe& P, Timer& tm, const EigPre* pre = nullptr) {
  // whatever blmm_prepare_dev left in this context (Rp, Z0, lambda, the status block) is about to be overwritten or reallocated:
  // the *_prerotated entry points must not run on it afterwards (blmm_prepare_dev sets the flag again when IT got here)
  ctx->prep_valid = false;
  if (n < 1 || ncov < 0) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  if (n > 2048) return fail(ctx, BLMM_ERR_UNSUPPORTED, "more than 2048 individuals: the device eigensolver (tridiagonalisation + divide and conquer) stops at n = 2048");
  const NullCov nc = null_cov(o, dCovar, ncov);
  const int c = (int)nc.c;
  if (c < 1 || c > CMAX) return fail(ctx, BLMM_ERR_UNSUPPORTED, BLMM_C_ERR);
  if (c >= n) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  P.n = (int)n; P.c = c; P.npad = (int)round_up(n, 8); P.ldr = (int)round_up(P.npad, 16);   // K padded to 8: even K-step count
  int rc;
  if ((rc = ensure(ctx, ctx->U, sizeof(double) * n * n))) return rc;
  if ((rc = ensure(ctx, ctx->lam, sizeof(double) * n))) return rc;
  if ((rc = ensure(ctx, ctx->Zs, sizeof(double) * n * c))) return rc;
  if ((rc = ensure(ctx, ctx->Z0, sizeof(double) * n * c))) return rc;
  if ((rc = ensure(ctx, ctx->Rp, sizeof(double) * (size_t)P.npad * P.ldr))) return rc;
  P.Z0 = ptr<double>(ctx->Z0); P.lam = ptr<double>(ctx->lam);
  if (pre) {
    P.stat = pre->stat;
    ctx->audit_ran = false;
    ctx->brent_cnt_used = false;
    P.big = n > jacobi_lds_max_n();
    bool post_done = false;
    tm.mark();
    if ((rc = launch_jacobi_post(ctx, pre->Ks, pre->V, (int)n, pre->lraw, P.stat, ptr<double>(ctx->Zs), dweights, c, P.npad, P.ldr,
                                 o->decomp_scheme, centered, P.lam, ptr<double>(ctx->U), P.Z0, ptr<double>(ctx->Rp), &post_done))) return rc;
    if (!post_done && (rc = launch_post_eigen(ctx, pre->lraw, pre->V, ptr<double>(ctx->Zs), dweights, (int)n, c, P.npad, P.ldr,
                                              o->decomp_scheme, centered, P.lam, ptr<double>(ctx->U), P.Z0, ptr<double>(ctx->Rp), P.stat))) return rc;
    tm.mark();
    return BLMM_OK;
  }
  if ((rc = ensure(ctx, ctx->Ks, sizeof(double) * n * n))) return rc;
  if ((rc = ensure(ctx, ctx->V, sizeof(double) * (n * n + 4 * n + 16)))) return rc;
  if ((rc = ensure(ctx, ctx->lraw, sizeof(double) * n))) return rc;
  const double* evec = ptr<double>(ctx->V);
  // n <= 124: LDS Jacobi.  Beyond: the own tridiagonalisation + divide-and-conquer solver (kernels_eig.hip) up to n = 2048 (its
  // reduction keeps the matrix in LDS up to ~1450 and in L2-resident global memory beyond).  No vendor library: rocSOLVER's first
  // use in a process takes MINUTES on this image (code-object load) and its path could not be part of the default test run.
  // BLMM_EIGEN = dc | jacobi overrides the choice (A/B timing and tests; "dc" also for n <= 124; "jacobi" beyond 124 is the
  // single-workgroup global-memory Jacobi: 0.74 s at n = 333).
  const char* eig_env = dev_env("BLMM_EIGEN");                 // tuning key "eigen_solver": 1 = "jacobi", 2 = "dc"
  if (!eig_env && ctx->tune.eigen_solver == 1) eig_env = "jacobi";
  if (!eig_env && ctx->tune.eigen_solver == 2) eig_env = "dc";
  const bool big = n > jacobi_lds_max_n();
  P.big = big;
  bool done = false, post_done = false;
  const bool want_dc = eig_env ? std::strcmp(eig_env, "dc") == 0 : big;
  // n <= 124: the fast path first (tridiagonalisation, Sturm multi-section, twisted factorisation; kernels_eig.hip: k_eigf_*).
  // It checks its own result on the device; the Jacobi behind it is a no-op when the checks passed and the whole solver when
  // they did not (numerically repeated eigenvalues).  BLMM_EIGEN=jacobi: the Jacobi alone (A/B timing, tests).
  const bool want_fast = !(eig_env && std::strcmp(eig_env, "jacobi") == 0) && n >= 3 && n <= eig_fast_max_n();
  // Where the fast path is the call's first solver, its first kernel -- one workgroup that starts by loading the matrix -- builds
  // Ks and Zs itself and zeroes the status block: no fill and no design launch in front of it (two dependent steps of a chain on
  // which one workgroup runs at a time).  Every other route keeps both.
  const DesignFold fold{dK, nc.d, dweights, ptr<double>(ctx->Ks), ptr<double>(ctx->Zs), (int)nc.ncov, nc.add_int};
  const bool folded = want_fast && !want_dc;
  auto design = [&]() { return launch_design(ctx, dK, nc.d, (int)nc.ncov, nc.add_int, dweights, (int)n, fold.Ks, fold.Zs); };
  if ((rc = folded ? reset_stat_host(ctx, &P.stat) : reset_stat(ctx, &P.stat))) return rc;
  tm.mark();
  if (!folded && (rc = design())) return rc;
  if (!done && want_dc && n >= 3) {
    rc = launch_eig_dc(ctx, ptr<double>(ctx->Ks), (int)n, ptr<double>(ctx->lraw), ptr<double>(ctx->V), P.stat);
    if (rc == BLMM_OK) { done = true; P.big = true; }
    else if (rc != BLMM_ERR_UNSUPPORTED) return rc;
  }
  if (!done) {
    if (want_fast) {
      rc = launch_eig_fast(ctx, ptr<double>(ctx->Ks), (int)n, ptr<double>(ctx->lraw), ptr<double>(ctx->V), P.stat, folded ? &fold : nullptr);
      if (rc != BLMM_OK && rc != BLMM_ERR_UNSUPPORTED) return rc;
      if (rc == BLMM_ERR_UNSUPPORTED && folded) {    // (it launched nothing: the Jacobi alone, behind the fill and the design)
        BLMM_HIP(hipMemsetAsync(P.stat, 0, sizeof(int64_t) * NSTAT, ctx->stream));
        if ((rc = design())) return rc;
      }
    }
    // (the post-eigen work rides in the tail of this launch where its LDS fits: one dependent-launch boundary less)
    if ((rc = launch_jacobi_post(ctx, ptr<double>(ctx->Ks), ptr<double>(ctx->V), (int)n, ptr<double>(ctx->lraw), P.stat, ptr<double>(ctx->Zs),
                                 dweights, c, P.npad, P.ldr, o->decomp_scheme, centered, P.lam, ptr<double>(ctx->U), P.Z0, ptr<double>(ctx->Rp),
                                 &post_done))) return rc;
  }
  if (!post_done && (rc = launch_post_eigen(ctx, ptr<double>(ctx->lraw), evec, ptr<double>(ctx->Zs), dweights, (int)n, c,
                              P.npad, P.ldr, o->decomp_scheme, centered, P.lam, ptr<double>(ctx->U), P.Z0,
                              ptr<double>(ctx->Rp), P.stat))) return rc;
  tm.mark();
  return BLMM_OK;
}

// the host entry points' deferred uploads (blmm_ctx::up_pending): on the copy stream, behind nothing; ev_in says when they are there
static int flush_upload(blmm_ctx* ctx) {
  if (!ctx->up_pending) return BLMM_OK;
  ctx->up_pending = false;
  for (int i = 0; i < 2; ++i) {
    if (ctx->up_bytes[i]) BLMM_HIP(hipMemcpyAsync(ctx->up_dst[i], ctx->up_src[i], ctx->up_bytes[i], hipMemcpyHostToDevice, ctx->copy));
    if (i == 0) BLMM_HIP(hipEventRecord(ctx->ev_inY, ctx->copy));     // the traits first: the main stream's rotation is the critical one
  }
  BLMM_HIP(hipEventRecord(ctx->ev_in, ctx->copy));
  ctx->in_wait = true;
  return BLMM_OK;
}

// null-exact, low-rank weights form: the basis of the weight family needs only the sorted eigenvalues, so it starts on the side
// stream right behind the eigen-decomposition, beside the rotation and the Brent search (joined before k_lr_panels)
int rotate_markers(blmm_ctx* ctx, Pipe& P, const double* dG, int64_t p);
// dG != nullptr: the marker rotation goes to the side stream as well, in front of the basis (the h2 search on the main stream needs
// only the rotated traits; the marker-side products that follow the basis on the side stream and -- behind ev_join -- the scan
// need Xt): 12 us less in front of k_brent at the BXD shape
// early_decomp >= 0: k_eigf_pairs has recorded ev_pairs (prepare): the basis is built from the solver's raw eigenvalues right behind
// that kernel, ~50 us before the eigen phase ends, and a second launch behind the phase's end stands in for it should the device have
// rejected the fast path (kernels_lowrank.hip: WbMode) -- the basis and the marker-side products behind it leave the critical path
enum FrontRoute { FRONT_EARLY_WB = 1, FRONT_FUSED_ROT = 2, FRONT_WB_REBUILT = 8 };   // (bit 2: kept free for region 0's counts from k_brent)
static bool front_switch(const char* name) { const char* e = dev_env(name); return !(e && e[0] == '0'); }
int start_wbasis(blmm_ctx* ctx, Pipe& P, const double* dG = nullptr, int64_t p = 0, bool xt_recorded = false, int early_decomp = -1) {
  int rc;
  const int64_t n = P.n;
  const LrSeg seg = lr_segments(ctx, P.n);
  if ((rc = ensure(ctx, ctx->wbQ, sizeof(double) * (size_t)seg.S * P.npad * n))) return rc;
  if ((rc = ensure(ctx, ctx->wbW, sizeof(double) * (size_t)n * (256 + 16)))) return rc;
  if ((rc = ensure(ctx, ctx->wbRk, sizeof(int) * 4 * LR_SEG_MAX))) return rc;
  if (!xt_recorded) BLMM_HIP(hipEventRecord(ctx->ev_xt, ctx->stream));     // (else: recorded by the eigen phase's last kernel itself)
  BLMM_HIP(hipStreamWaitEvent(ctx->side, ctx->ev_xt, 0));
  ctx->wb_on_side2 = false;
  if (!dG) {
    OnStream on(ctx, ctx->side);
    return launch_wbasis(ctx, P.lam, (int)n, P.npad, seg, ptr<double>(ctx->wbW), ptr<double>(ctx->wbQ), ptr<int>(ctx->wbRk), P.stat);
  }
  {
    // The basis (a handful of 1024-thread workgroups, 70 us of dependent steps) goes to the SECOND side stream, beside the marker
    // rotation instead of behind it: queued behind the rotation it became dispatchable at the same moment as the h2 search,
    // whose 2,200 waves then held every CU until the first of them retired -- 126 us instead of 70, and with the marker-side
    // products behind it the critical path of the front whenever nothing else delayed the main stream (a caller that does not
    // ask for phase timings: +35 us per call; profiles/r04_timeline_notiming_*.txt).  The marker-side products follow the basis
    // on ITS stream (lr_begin: no cross-queue wait between the two, each of which costs 14-20 us here) and wait there for
    // the rotation (ev_wb), which is done long before.
    ctx->wb_on_side2 = true;
    OnStream on(ctx, ctx->side2);
    if (early_decomp >= 0) {
      BLMM_HIP(hipStreamWaitEvent(ctx->side2, ctx->ev_pairs, 0));
      if ((rc = launch_wbasis(ctx, P.lam, (int)n, P.npad, seg, ptr<double>(ctx->wbW), ptr<double>(ctx->wbQ), ptr<int>(ctx->wbRk), P.stat,
                              WB_EARLY, ptr<double>(ctx->lraw), early_decomp))) return rc;
      ctx->last_front_route |= FRONT_EARLY_WB;
    }
    BLMM_HIP(hipStreamWaitEvent(ctx->side2, ctx->ev_xt, 0));
    if ((rc = launch_wbasis(ctx, P.lam, (int)n, P.npad, seg, ptr<double>(ctx->wbW), ptr<double>(ctx->wbQ), ptr<int>(ctx->wbRk), P.stat,
                            early_decomp >= 0 ? WB_REDO : WB_LAM))) return rc;
  }
  OnStream on(ctx, ctx->side);
  if (ctx->in_wait) BLMM_HIP(hipStreamWaitEvent(ctx->side, ctx->ev_in, 0));
  if ((rc = rotate_markers(ctx, P, dG, p))) return rc;
  BLMM_HIP(hipEventRecord(ctx->ev_wb, ctx->side));                  // ev_wb: the rotated markers
  return BLMM_OK;
}

// The own rotation kernels sum every output element in a fixed order, so a trait's (or marker's) rotated column does not depend on
// how many OTHER columns are in the call (the sharding contract: a column block scanned alone is bit-identical,
// tests/test_gpu_configs.py; a vendor GEMM picks its kernel -- tile shape, split-K -- from the problem shape and broke exactly
// that in round 1).
int rotate_traits(blmm_ctx* ctx, Pipe& P, const double* dY, int64_t m) {
  if (m < 0) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  P.m = m; P.ldy = round_up(m > 0 ? m : 1, 128);
  int rc = ensure(ctx, ctx->Yt, sizeof(double) * (size_t)P.npad * P.ldy);
  if (rc) return rc;
  P.Yt = ptr<double>(ctx->Yt);
  return launch_rotate(ctx, ptr<double>(ctx->Rp), P.ldr, P.n, P.npad, dY, m, P.Yt, P.ldy, P.ldy);
}
int rotate_markers(blmm_ctx* ctx, Pipe& P, const double* dG, int64_t p) {
  if (p < 0) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  P.p = p; P.ldx = round_up(p > 0 ? p : 1, 128);
  int rc = ensure(ctx, ctx->Xt, sizeof(double) * (size_t)P.npad * P.ldx);
  if (rc) return rc;
  P.Xt = ptr<double>(ctx->Xt);
  return launch_rotate(ctx, ptr<double>(ctx->Rp), P.ldr, P.n, P.npad, dG, p, P.Xt, P.ldx, P.ldx);
}

int prepare(blmm_ctx* ctx, const blmm_opts* o, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
            const double* dCovar, int64_t ncov, const double* dK, const double* dweights, int centered, Pipe& P, Timer& tm,
            bool early_wbasis = false, bool grid_side = false, bool skip_markers = false, const EigPre* pre = nullptr) {
  if (m < 0 || p < 0) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  // the side streams fork where the eigen phase ends: its last kernel records the fork event itself (BLMM_LAUNCH_STOP)
  const bool forks = m > 0 && p > 0 && (early_wbasis || grid_side);
  ctx->stop_event_used = false;
  ctx->stop_event_next = forks ? ctx->ev_xt : nullptr;
  // (BLMM_ROTATE_SIDE=0: the marker rotation stays on the main stream behind the traits' -- A/B testing)
  static const bool rot_side = !(dev_env("BLMM_ROTATE_SIDE") && dev_env("BLMM_ROTATE_SIDE")[0] == '0');
  // only where the rotation is the small latency-bound kernel (n <= 160): the GEMM of larger n fills the chip by itself, and behind it
  // the basis and the marker-side products come later (n = 500 shard: 6.32 against 6.29 ms; BXD: 1.714 against 1.734 ms, 4 A/B rounds)
  const bool side_g = early_wbasis && m > 0 && p > 0 && rot_side && n <= 160;
  // the weight basis behind k_eigf_pairs: a single call's fast eigen route, the register-resident basis kernel on its own stream
  // (BLMM_EARLY_WB=0: behind the eigen phase's end as before -- A/B testing)
  static const char* mw_env = dev_env("BLMM_WBASIS");
  ctx->last_front_route = 0;
  ctx->pairs_event_used = false;
  ctx->pairs_event_next = (side_g && !pre && n <= 80 && !(mw_env && std::strcmp(mw_env, "lds") == 0) && front_switch("BLMM_EARLY_WB")) ? ctx->ev_pairs : nullptr;
  int rc = prepare_eigen(ctx, o, n, dCovar, ncov, dK, dweights, centered, P, tm, pre);
  const bool xt_recorded = ctx->stop_event_used;
  ctx->stop_event_next = nullptr; ctx->stop_event_used = false;
  const bool early_basis = ctx->pairs_event_used;
  ctx->pairs_event_next = nullptr; ctx->pairs_event_used = false;
  if (rc) return rc;
  // (host entry points) the eigen phase is queued: now the traits and the markers go up, beside it; this stream reads them next
  if (ctx->up_pending) {
    if ((rc = flush_upload(ctx))) return rc;
    BLMM_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_inY, 0));
  }
  const bool up_flight = ctx->in_wait;
  if (early_wbasis && m > 0 && p > 0 && (rc = start_wbasis(ctx, P, side_g ? dG : nullptr, p, xt_recorded, early_basis ? (int)o->decomp_scheme : -1))) return rc;
  P.xt_side = side_g;
  // the grid methods (grid_side): the marker rotation and, later, the marker norms of every grid point (launch_isx) on the side stream,
  // beside the traits' rotation, the grid log-likelihoods and the trait panels on the main stream; joined in front of the scan
  if (grid_side && !early_wbasis && m > 0 && p > 0 && rot_side && n <= 160) {
    if (!xt_recorded) BLMM_HIP(hipEventRecord(ctx->ev_xt, ctx->stream));
    BLMM_HIP(hipStreamWaitEvent(ctx->side, ctx->ev_xt, 0));
    if (ctx->in_wait) BLMM_HIP(hipStreamWaitEvent(ctx->side, ctx->ev_in, 0));
    OnStream on(ctx, ctx->side);
    if ((rc = rotate_markers(ctx, P, dG, p))) return rc;
    P.xt_side = true;
  }
  // the single null-exact call at n <= 80: k_brent, the next kernel of this stream, rotates its traits itself (scan_pipeline hands it
  // P.fuseY) -- no launch of its own, no write -> read round trip of Yt in front of the search (BLMM_FUSE_ROT=0: A/B testing)
  if (early_wbasis && !pre && m > 0 && p > 0 && brent_fuses_rotation(P.n, P.c) && front_switch("BLMM_FUSE_ROT")) {
    P.m = m; P.ldy = round_up(m, 128);
    if ((rc = ensure(ctx, ctx->Yt, sizeof(double) * (size_t)P.npad * P.ldy))) return rc;
    P.Yt = ptr<double>(ctx->Yt);
    P.fuseY = dY;
    ctx->last_front_route |= FRONT_FUSED_ROT;
  } else if ((rc = rotate_traits(ctx, P, dY, m))) return rc;
  if (skip_markers) { P.p = p; P.ldx = round_up(p > 0 ? p : 1, 128); P.Xt = nullptr; }   // the caller rotates them itself (fp32 permutation path)
  else if (!P.xt_side) {
    if (up_flight) BLMM_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_in, 0));     // (the markers on this stream: they went up second)
    if ((rc = rotate_markers(ctx, P, dG, p))) return rc;
  }
  ctx->in_wait = false;                     // every reader of the uploaded inputs is queued behind ev_in
  tm.mark();
  return BLMM_OK;
}

NullModel null_model(const Pipe& P, const blmm_opts* o) {
  NullModel nm;
  nm.n = P.n; nm.c = P.c; nm.npad = P.npad; nm.reml = o->reml ? 1 : 0;
  nm.optim_interval = o->optim_interval < 1 ? 1 : o->optim_interval;
  nm.prior_a = o->prior_variance; nm.prior_b = o->prior_sample_size;
  return nm;
}

// Caller memory -> dst on ctx->stream without waiting: through a pinned slot of the context.  A slot whose copy has not run yet
// (its event is pending: back-to-back calls) is left alone and the ring grows instead -- to the depth of the caller's queue at most.
int stage_to_device(blmm_ctx* ctx, DevBuf& dst, const void* src, size_t bytes) {
  blmm_ctx::GridSlot* slot = nullptr;
  for (auto& g : ctx->gstage)
    if (g.cap >= bytes && (!g.used || hipEventQuery(g.ev) == hipSuccess)) { slot = &g; break; }
  if (!slot) {
    blmm_ctx::GridSlot g;
    g.cap = bytes < 4096 ? 4096 : bytes;
    void* h = nullptr;
    BLMM_HIP(hipHostMalloc(&h, g.cap, hipHostMallocDefault));
    g.h = h;
    if (hipEventCreateWithFlags(&g.ev, hipEventDisableTiming) != hipSuccess) { (void)hipHostFree(h); return fail(ctx, BLMM_ERR_HIP, "hipEventCreate failed"); }
    ctx->gstage.push_back(g);
    slot = &ctx->gstage.back();
  }
  std::memcpy(slot->h, src, bytes);
  BLMM_HIP(hipMemcpyAsync(dst.p, slot->h, bytes, hipMemcpyHostToDevice, ctx->stream));
  BLMM_HIP(hipEventRecord(slot->ev, ctx->stream));
  slot->used = true;
  return BLMM_OK;
}

int check_grid(blmm_ctx* ctx, const double* h2_grid_host, int64_t ngrid) {
  if (!h2_grid_host || ngrid < 1) return fail(ctx, BLMM_ERR_INVALID, "h2 grid is empty");
  for (int64_t g = 0; g < ngrid; ++g) {
    const double h = h2_grid_host[g];
    if (std::isinf(h / (1.0 - h))) return fail(ctx, BLMM_ERR_H2_ONE, "Heritability of 1 is not allowed.");
  }
  return BLMM_OK;
}

int grid_to_device(blmm_ctx* ctx, const double* h2_grid_host, int64_t ngrid, double** out) {
  int rc;
  if ((rc = check_grid(ctx, h2_grid_host, ngrid)) || (rc = ensure(ctx, ctx->gridd, sizeof(double) * ngrid))) return rc;
  const size_t bytes = sizeof(double) * (size_t)ngrid;
  if (ctx->grid_async) {                     // blmm_bulkscan_reduced_async: no wait
    if ((rc = stage_to_device(ctx, ctx->gridd, h2_grid_host, bytes))) return rc;
  } else {
    BLMM_HIP(hipMemcpyAsync(ctx->gridd.p, h2_grid_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    // the source is caller memory: make sure the copy has left it before we return
    BLMM_HIP(hipStreamSynchronize(ctx->stream));
  }
  *out = ptr<double>(ctx->gridd);
  return BLMM_OK;
}

ScanArgs scan_args(blmm_ctx* ctx, const Pipe& P, const double* panels, int64_t ldp, double* L, int64_t ldL, int64_t m) {
  ScanArgs a;
  a.Xt = P.Xt; a.ldx = P.ldx; a.P = panels; a.ldp = ldp; a.pstride = (int64_t)P.npad * ldp;
  a.ks = P.npad / 4; a.n = P.n; a.p = P.p; a.m = m; a.L = L; a.ldL = ldL;
  a.isx = nullptr; a.ld_isx = 0; a.bin = nullptr; a.stat = P.stat; a.logtab = ptr<double>(ctx->logtab); a.lodtab = ptr<double>(ctx->lodtab);
  a.Pv = ctx->pv_cur; a.ldPv = ctx->pv_cur_ld; a.pvtab = ptr<double>(ctx->pvtab);
  a.red = ctx->red_cur;                    // blmm_bulkscan_reduced: the scan kernels reduce in their epilogues, L == nullptr
  a.c = P.c;
  lod_poly5_host(-0.5 * (double)P.n, a.lodc);
  return a;
}

// ---- null-exact LOD scan in the low-rank weights form (kernels_lowrank.hip), shared by bulkscan(null-exact) and the
// liteqtl_given_h2 seam.  lr_begin: weight basis (unless prepare() already started it) and the marker-side products on
// the side stream; the caller may then enqueue the h2 search on the main stream; lr_finish: per-trait panels, the
// MFMA scan, the all-trait residual guard beside it, and the full-rank re-scan of the flagged traits.
double lr_tolerance(const blmm_ctx* ctx) {
  // relative residual |w_j - Q Q'w_j| / |w_j| above which a trait's column is recomputed from the full-length sums: tuning key
  // "lr_tol" (tests: 0 flags every trait, so the re-scan kernel is compared with the oracle as a whole)
  const char* e = dev_env("BLMM_LR_TOL");
  return e ? atof(e) : ctx->tune.lr_tol;
}

// Width of one region of the panel arrays (LrRegion): k_lr_classify fills it from both ends, so it needs a whole padding
// tile beyond the traits.  The arrays hold two regions (leading dimension 2 * lr_ldq): the second one is used when the
// h2 search is split and its second kernel runs beside the scan of the traits the first kernel finished.
int64_t lr_ldq(const Pipe& P) { return P.ldy + 128 + LR_TILE * LR_SEG_MAX; }   // + a partly filled tile per weight-basis segment
// the per-region device counters of the class / segment layout (blmm_internal.h: NSTAT)
static LrRegion lr_region(const Pipe& P, int r) {
  LrRegion rg;
  rg.col0 = r * lr_ldq(P); rg.ncol = lr_ldq(P); rg.counts = P.stat + ST_LR_SHARED0 + 2 * r; rg.segcnt = P.stat + 24 + 20 * r;
  return rg;
}

int lr_begin(blmm_ctx* ctx, const Pipe& P, bool wbasis_started) {
  int rc;
  ctx->lr_last_ldq = lr_ldq(P); ctx->lr_last_m = P.m;            // blmm_lowrank_columns
  const int64_t ldp = 2 * lr_ldq(P), tstride = (int64_t)P.npad * P.ldx;
  if ((rc = ensure(ctx, ctx->lrPerm, sizeof(int) * (size_t)ldp))) return rc;
  if ((rc = ensure(ctx, ctx->lrDen0, sizeof(double) * (size_t)P.ldx))) return rc;
  const LrSeg seg = lr_segments(ctx, P.n);
  if ((rc = ensure(ctx, ctx->lrT, sizeof(double) * (size_t)seg.S * (1 + P.c) * tstride))) return rc;
  if ((rc = ensure(ctx, ctx->lrC, sizeof(double) * (size_t)P.npad * ldp))) return rc;
  if ((rc = ensure(ctx, ctx->lrL, sizeof(double) * (size_t)(P.c * (P.c + 1) / 2) * ldp))) return rc;
  if ((rc = ensure(ctx, ctx->lrFlag, sizeof(int) * (size_t)ldp))) return rc;
  if ((rc = ensure(ctx, ctx->lrPart, sizeof(double) * 2 * (size_t)((P.n + 63) / 64) * ldp))) return rc;
  if ((rc = ensure(ctx, ctx->panels, sizeof(double) * (size_t)P.npad * ldp))) return rc;
  if ((rc = ensure(ctx, ctx->wbQ, sizeof(double) * (size_t)seg.S * P.npad * P.n))) return rc;
  if ((rc = ensure(ctx, ctx->wbW, sizeof(double) * (size_t)P.n * (256 + 16)))) return rc;
  if ((rc = ensure(ctx, ctx->wbRk, sizeof(int) * 4 * LR_SEG_MAX))) return rc;
  int* rk = ptr<int>(ctx->wbRk);
  if (!(wbasis_started && P.xt_side)) {                            // (the side stream rotated the markers itself: nothing of the main stream to wait for)
    BLMM_HIP(hipEventRecord(ctx->ev_fork, ctx->stream));          // rotated operands are ready
    BLMM_HIP(hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
  }
  // (start_wbasis put the basis on the second side stream: the marker-side products follow it THERE, behind the rotation's event)
  const bool on2 = wbasis_started && P.xt_side && ctx->wb_on_side2;
  hipStream_t lr_side = on2 ? ctx->side2 : ctx->side;
  OnStream on(ctx, lr_side);
  if (!wbasis_started && (rc = launch_wbasis(ctx, P.lam, P.n, P.npad, seg, ptr<double>(ctx->wbW), ptr<double>(ctx->wbQ), rk, P.stat))) return rc;
  BLMM_HIP(hipEventRecord(ctx->ev_q, lr_side));                     // what the panels need
  if (on2) BLMM_HIP(hipStreamWaitEvent(lr_side, ctx->ev_wb, 0));
  if ((rc = launch_lr_tpanels(ctx, P.Xt, P.ldx, P.p, P.n, P.c, P.npad, P.Z0, ptr<double>(ctx->wbQ), rk, seg, ptr<double>(ctx->lrT), tstride,
                              ptr<double>(ctx->lrDen0)))) return rc;
  BLMM_HIP(hipEventRecord(ctx->ev_join, lr_side));                  // ... and what the scan needs on top
  // (the column order's preset, -1 = padding, is written by the count pass of k_lr_classify)
  return BLMM_OK;
}

namespace {
// the shared-weights class uses the tolerance of the expansion guard; BLMM_LR_SHARED=0 switches the class off (A/B testing)
double lr_shared_tol(const blmm_ctx* ctx) {
  // tuning key "lr_shared" = 0: no class (bench.py times the same process with and without it: ms_per_step_all_rank_form)
  const char* e = dev_env("BLMM_LR_SHARED");
  const bool on = e ? e[0] != '0' : ctx->tune.lr_shared != 0;
  return on ? lr_tolerance(ctx) : 0.0;
}
LrArgs lr_args(blmm_ctx* ctx, const Pipe& P, const LrRegion& rg, double* dL, int64_t ldL) {
  const int64_t ldp = 2 * lr_ldq(P);
  LrArgs la;
  // a.m sizes the grid only: a region holds at most m traits, in at most m/64 + 3 trait tiles
  la.s = scan_args(ctx, P, ptr<double>(ctx->panels), ldp, dL, ldL, P.m + 192 < rg.ncol ? P.m + 192 : rg.ncol);
  la.Cp = ptr<double>(ctx->lrC); la.T = ptr<double>(ctx->lrT); la.tstride = (int64_t)P.npad * P.ldx; la.Ls = ptr<double>(ctx->lrL);
  la.rk = ptr<int>(ctx->wbRk); la.c = P.c; la.perm = ptr<int>(ctx->lrPerm); la.rg = rg; la.den0 = ptr<double>(ctx->lrDen0);
  la.skip_shared = 0;
  la.seg = lr_segments(ctx, P.n);
  return la;
}
// LOD scan of one region on the current stream: the shared-weights class through the table kernel (one bin, 4 waves per
// SIMD), the other traits through k_scan_lr.  BLMM_LR_LEAN=0: both classes in k_scan_lr (A/B testing).
int lr_region_scan(blmm_ctx* ctx, const Pipe& P, const LrRegion& rg, double* dL, int64_t ldL) {
  static const bool lean = !(dev_env("BLMM_LR_LEAN") && dev_env("BLMM_LR_LEAN")[0] == '0');
  // diagnostic: the scan kernels alone on the chip (their rocprofv3 durations are then free of the side streams' kernels)
  static const bool serial = dev_env("BLMM_LR_SERIAL") && dev_env("BLMM_LR_SERIAL")[0] == '1';
  if (serial) { (void)hipStreamSynchronize(ctx->side); (void)hipStreamSynchronize(ctx->side2); (void)hipStreamSynchronize(ctx->stream); }
  LrArgs la = lr_args(ctx, P, rg, dL, ldL);
  int rc;
  if (lean) {
    ScanArgs a = la.s;
    a.isx = la.den0; a.ld_isx = P.ldx; a.bin = nullptr;
    a.perm = la.perm; a.col0 = rg.col0; a.count = rg.counts;
    if ((rc = launch_scan_shared(ctx, a))) return rc;
    la.skip_shared = 1;
  }
  return launch_scan_lr(ctx, la);
}
// panels of one region on the current stream
int lr_region_panels(blmm_ctx* ctx, const Pipe& P, const NullModel& nm, const double* dh2, const LrRegion& rg) {
  return launch_lr_panels(ctx, nm, P.Yt, P.ldy, P.m, P.Z0, P.lam, dh2, ptr<double>(ctx->wbQ), ptr<int>(ctx->wbRk), lr_segments(ctx, P.n), ptr<int>(ctx->lrPerm),
                          rg, ptr<double>(ctx->panels), ptr<double>(ctx->lrC), ptr<double>(ctx->lrL), 2 * lr_ldq(P), P.stat);
}
// residual guard of one region on the side stream (beside the region's scan)
int lr_region_resid(blmm_ctx* ctx, const Pipe& P, const NullModel& nm, const double* dh2, const LrRegion& rg) {
  OnStream on(ctx, ctx->side);
  return launch_lr_resid(ctx, nm, P.m, lr_tolerance(ctx), P.lam, dh2, ptr<double>(ctx->wbQ), ptr<int>(ctx->wbRk), lr_segments(ctx, P.n), ptr<int>(ctx->lrPerm), rg,
                         ptr<double>(ctx->lrC), 2 * lr_ldq(P), ptr<int>(ctx->lrFlag), ptr<double>(ctx->lrPart), P.stat, ctx->red_cur.flags);
}
int lr_fix(blmm_ctx* ctx, const Pipe& P, const NullModel& nm, const double* dh2, double* dL, int64_t ldL) {
  // flagged traits (normally none: the kernel reads the count on the device and returns): full-length sums
  // reduce-in-epilogue: there is no L to patch -- reduced_impl() reads the count and re-runs; reduced_async_impl() (red_cur.flags)
  // has the reduced form of the kernel patch the slot partials instead
  if (ctx->red_cur.pmax && !ctx->red_cur.flags) return BLMM_OK;
  return launch_scan_fix(ctx, nm, P.Xt, P.ldx, P.p, ptr<double>(ctx->panels), ptr<double>(ctx->lrL), 2 * lr_ldq(P), P.Z0, P.lam, dh2,
                         ptr<int>(ctx->lrFlag), ptr<int>(ctx->lrPerm), dL, ldL, P.stat, ctx->red_cur);
}
}  // namespace

// Conditioning guard (kernels_dyn.hip): traits whose weighted null design is nearly collinear (several covariates, h2 -> 1)
// get their LOD columns recomputed with an orthogonalised projection; a no-op for c = 1.  Runs on the current stream after
// the scan kernels that wrote dL.
int illcond_rescan(blmm_ctx* ctx, const Pipe& P, const NullModel& nm, int64_t m, const double* dh2, double* dL, int64_t ldL) {
  if (P.c < 2 || m <= 0 || P.p <= 0) return BLMM_OK;
  int rc = ensure(ctx, ctx->illList, sizeof(int) * (size_t)m);
  if (rc) return rc;
  const bool patch = ctx->red_cur.pmax && ctx->red_cur.flags;   // reduced_async_impl(): flagged beside the scan (lr_finish) already
  if (!patch && (rc = launch_illcond_flag(ctx, nm, m, P.Z0, P.lam, dh2, ptr<int>(ctx->illList), P.stat))) return rc;
  if (ctx->red_cur.pmax && !patch) return BLMM_OK;   // (as lr_fix)
  return launch_scan_qr(ctx, nm, P.Yt, P.ldy, P.Xt, P.ldx, P.p, P.Z0, P.lam, dh2, ptr<int>(ctx->illList), dL, ldL, P.stat, ctx->red_cur);
}

// every trait's h2 is final: one region
int lr_finish(blmm_ctx* ctx, const Pipe& P, const NullModel& nm, const double* dh2, double* dL, int64_t ldL, Timer& tm) {
  int rc;
  const LrRegion rg = lr_region(P, 0);
  const LrSeg seg = lr_segments(ctx, P.n);
  hipStream_t main_stream = ctx->stream;
  BLMM_HIP(hipStreamWaitEvent(main_stream, ctx->ev_join, 0));
  if ((rc = launch_lr_classify(ctx, P.n, P.m, lr_shared_tol(ctx), P.lam, dh2, nullptr, nullptr, nullptr, ptr<int>(ctx->lrPerm), rg, seg))) return rc;
  if ((rc = lr_region_panels(ctx, P, nm, dh2, rg))) return rc;
  tm.mark();
  // residual guard of the weight basis, every trait: side stream, beside the scan kernel; joined below
  // (reduced_async_impl, red_cur.flags: the conditioning guard joins it there, and when triplets are wanted the scan waits for
  // both -- its epilogue appends none for a flagged trait, the re-scan kernels append those)
  const bool ahead = ctx->red_cur.flags != nullptr;
  if (ahead && P.c >= 2 && (rc = ensure(ctx, ctx->illList, sizeof(int) * (size_t)P.m))) return rc;
  BLMM_HIP(hipEventRecord(ctx->ev_fork, main_stream));
  BLMM_HIP(hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
  if ((rc = lr_region_resid(ctx, P, nm, dh2, rg))) return rc;
  if (ahead && P.c >= 2) {
    OnStream on(ctx, ctx->side);
    if ((rc = launch_illcond_flag(ctx, nm, P.m, P.Z0, P.lam, dh2, ptr<int>(ctx->illList), P.stat, ctx->red_cur.flags))) return rc;
  }
  BLMM_HIP(hipEventRecord(ctx->ev_join, ctx->side));
  if (ahead && ctx->red_cur.want_trip) BLMM_HIP(hipStreamWaitEvent(main_stream, ctx->ev_join, 0));
  if ((rc = lr_region_scan(ctx, P, rg, dL, ldL))) return rc;
  BLMM_HIP(hipStreamWaitEvent(main_stream, ctx->ev_join, 0));
  if ((rc = lr_fix(ctx, P, nm, dh2, dL, ldL))) return rc;
  if ((rc = illcond_rescan(ctx, P, nm, P.m, dh2, dL, ldL))) return rc;
  tm.mark();
  return BLMM_OK;
}

// The h2 search was split (launch_brent phase 1 came back with sp.active): the traits k_brent finished (fin[j] == 1) form
// region 0 and are scanned at once; k_brent2, the classification and the panels of its traits (region 1) run on a
// second side stream beside that scan, and region 1 is scanned after it.
int lr_finish_split(blmm_ctx* ctx, const Pipe& P, const NullModel& nm, double* dh2, double* dL, int64_t ldL, Timer& tm,
                    const BrentSplit& sp) {
  int rc;
  const LrRegion r0 = lr_region(P, 0), r1 = lr_region(P, 1);
  const LrSeg seg = lr_segments(ctx, P.n);
  hipStream_t main_stream = ctx->stream;
  // ---- main stream: region 0's classification and panels (the weight basis is ready at ev_q, the marker-side products at ev_join) ...
  if ((rc = launch_lr_classify(ctx, P.n, P.m, lr_shared_tol(ctx), P.lam, dh2, sp.fin, nullptr, nullptr, ptr<int>(ctx->lrPerm), r0, seg))) return rc;
  // ONE wait: ev_join is recorded on the side stream behind ev_q (the basis) and behind the marker-side products, which are done
  // before the panels kernel can start anyway (profiles/r03_timeline_bxd_step.txt: 410 us against 425) -- every barrier packet
  // between two dependent kernels of this stream costs ~10 us
  BLMM_HIP(hipStreamWaitEvent(main_stream, ctx->ev_join, 0));
  ctx->stop_event_used = false;
  ctx->stop_event_next = ctx->ev_b1;                                 // recorded by the panels kernel itself
  rc = lr_region_panels(ctx, P, nm, dh2, r0);
  const bool b1_recorded = ctx->stop_event_used;
  ctx->stop_event_next = nullptr; ctx->stop_event_used = false;
  if (rc) return rc;
  // ---- ... and only then the second side stream: the rest of the h2 search, then region 1's columns.  Forked right behind
  //      k_brent (rounds 2-3a) k_brent2's older waves won the issue arbitration against the 16-lane panels kernel on the
  //      critical path (45 us beside it, 28 alone); its chain has ~0.5 ms of slack before region 1's scan needs it
  if (!b1_recorded) BLMM_HIP(hipEventRecord(ctx->ev_b1, main_stream));
  BLMM_HIP(hipStreamWaitEvent(ctx->side2, ctx->ev_b1, 0));
  {
    OnStream on(ctx, ctx->side2);
    BrentSplit sp2 = sp;
    if ((rc = launch_brent(ctx, nm, P.Yt, P.ldy, P.m, P.Z0, P.lam, dh2, nullptr, nullptr, P.stat, 2, &sp2))) return rc;
    BLMM_HIP(hipStreamWaitEvent(ctx->side2, ctx->ev_q, 0));
    if ((rc = launch_lr_classify(ctx, P.n, P.m, lr_shared_tol(ctx), P.lam, dh2, nullptr, sp.list, sp.cnt, ptr<int>(ctx->lrPerm), r1, seg)) ||
        (rc = lr_region_panels(ctx, P, nm, dh2, r1))) return rc;
  }
  BLMM_HIP(hipEventRecord(ctx->ev_b2, ctx->side2));
  tm.mark();
  BLMM_HIP(hipStreamWaitEvent(ctx->side, ctx->ev_b1, 0));            // region 0's panels are done (the same point the second side stream forks at)
  if ((rc = lr_region_resid(ctx, P, nm, dh2, r0))) return rc;
  // (reduced_async_impl with triplets: each region's scan waits for its guard -- see lr_finish; it splits only at c = 1)
  const bool ahead = ctx->red_cur.flags != nullptr && ctx->red_cur.want_trip;
  if (ahead) {
    BLMM_HIP(hipEventRecord(ctx->ev_join, ctx->side));
    BLMM_HIP(hipStreamWaitEvent(main_stream, ctx->ev_join, 0));
  }
  if ((rc = lr_region_scan(ctx, P, r0, dL, ldL))) return rc;
  // ---- region 1: its guard on the first side stream (behind region 0's), its scan on the main stream
  BLMM_HIP(hipStreamWaitEvent(ctx->side, ctx->ev_b2, 0));
  if ((rc = lr_region_resid(ctx, P, nm, dh2, r1))) return rc;
  BLMM_HIP(hipEventRecord(ctx->ev_join, ctx->side));
  BLMM_HIP(hipStreamWaitEvent(main_stream, ctx->ev_b2, 0));
  if (ahead) BLMM_HIP(hipStreamWaitEvent(main_stream, ctx->ev_join, 0));
  if ((rc = lr_region_scan(ctx, P, r1, dL, ldL))) return rc;
  BLMM_HIP(hipStreamWaitEvent(main_stream, ctx->ev_join, 0));
  if ((rc = lr_fix(ctx, P, nm, dh2, dL, ldL))) return rc;
  if ((rc = illcond_rescan(ctx, P, nm, P.m, dh2, dL, ldL))) return rc;
  tm.mark();
  return BLMM_OK;
}

}  // namespace

extern "C" {

int blmm_version(void) { return BLMM_VERSION; }

int blmm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* blmm_err_string(int code) {
  switch (code) {
    case BLMM_OK: return "ok";
    case BLMM_ERR_INVALID: return "invalid argument";
    case BLMM_ERR_DIM: return "Dimension mismatch.";
    case BLMM_ERR_H2_ONE: return "Heritability of 1 is not allowed.";
    case BLMM_ERR_DECOMP: return "Please choose either `eigen` or `svd` for decomposition of the kinship matrix.";
    case BLMM_ERR_METHOD: return "unknown bulkscan method";
    case BLMM_ERR_ONE_TRAIT: return "Can only handle one trait.";
    case BLMM_ERR_NO_INTERCEPT: return "Intercept has to be added when no other covariate is given.";
    case BLMM_ERR_ZERO_NORM: return "Dividing by zeros: the input vector can not contain any zeros!";
    case BLMM_ERR_NPERMS: return "The required number of permutations must be a positive integer.";
    case BLMM_ERR_UNSUPPORTED: return "unsupported configuration";
    case BLMM_ERR_NO_DEVICE: return "no usable HIP device";
    case BLMM_ERR_HIP: return "HIP runtime error";
    case BLMM_ERR_ALLOC: return "device allocation failed";
  }
  return "unknown error";
}

int blmm_create(int device_id, void* hip_stream, blmm_ctx** out) {
  if (!out) return BLMM_ERR_INVALID;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev) return BLMM_ERR_NO_DEVICE;
  if (hipSetDevice(device_id) != hipSuccess) return BLMM_ERR_NO_DEVICE;
  blmm_ctx* ctx = new blmm_ctx();
  ctx->device = device_id;
  if (hip_stream == BLMM_STREAM_NULL) {
    ctx->stream = nullptr;   // the legacy default stream (handle 0)
  } else if (hip_stream) {
    ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
  } else {
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return BLMM_ERR_HIP; }
    ctx->own_stream = true;
  }
  if (hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_xt, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_pairs, hipEventDisableTiming) != hipSuccess ||
      hipStreamCreateWithFlags(&ctx->side2, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_b1, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_b2, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_q, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_m, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_wb, hipEventDisableTiming) != hipSuccess ||
      hipStreamCreateWithFlags(&ctx->copy, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_in, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_inY, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_call, hipEventDisableTiming) != hipSuccess) {
    blmm_destroy(ctx);
    return BLMM_ERR_HIP;
  }
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess) ctx->num_cus = cus;
    void* hp = nullptr;
    if (hipHostMalloc(&hp, 64, hipHostMallocMapped) != hipSuccess) { blmm_destroy(ctx); return BLMM_ERR_HIP; }
    std::memset(hp, 0, 64);
    ctx->hflag = reinterpret_cast<volatile int64_t*>(hp);
  }
  if (ensure(ctx, ctx->logtab, sizeof(blmm_log_table_host)) != BLMM_OK ||
      hipMemcpy(ctx->logtab.p, blmm_log_table_host, sizeof(blmm_log_table_host), hipMemcpyHostToDevice) != hipSuccess ||
      ensure(ctx, ctx->lodtab, sizeof(blmm_lod_table_host)) != BLMM_OK ||
      hipMemcpy(ctx->lodtab.p, blmm_lod_table_host, sizeof(blmm_lod_table_host), hipMemcpyHostToDevice) != hipSuccess ||
      ensure(ctx, ctx->pvtab, sizeof(blmm_pv_table_host)) != BLMM_OK ||
      hipMemcpy(ctx->pvtab.p, blmm_pv_table_host, sizeof(blmm_pv_table_host), hipMemcpyHostToDevice) != hipSuccess) {
    blmm_destroy(ctx);
    return BLMM_ERR_HIP;
  }
  *out = ctx;
  return BLMM_OK;
}

void blmm_destroy(blmm_ctx* ctx) {
  if (!ctx) return;
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  DevBuf* bufs[] = {&ctx->Ks, &ctx->V, &ctx->lam, &ctx->U, &ctx->Zs, &ctx->Z0, &ctx->Rp, &ctx->Yt, &ctx->Xt, &ctx->panels,
                    &ctx->iyy, &ctx->h2, &ctx->h2idx, &ctx->sig2, &ctx->ell, &ctx->isx, &ctx->stat, &ctx->gridd, &ctx->misc,
                    &ctx->EllTab, &ctx->inY, &ctx->inG, &ctx->inK, &ctx->inCov, &ctx->inW, &ctx->outL, &ctx->outH2,
                    &ctx->tmpA, &ctx->tmpB, &ctx->tmpC, &ctx->perm, &ctx->r0, &ctx->altbuf, &ctx->logtab, &ctx->lraw,
                    &ctx->wbQ, &ctx->wbW, &ctx->wbRk, &ctx->lrT, &ctx->lrC, &ctx->lrL, &ctx->lrFlag, &ctx->lrPart, &ctx->lrPerm, &ctx->lrDen0, &ctx->eigW, &ctx->xf32, &ctx->pf32, &ctx->brSt, &ctx->brList, &ctx->illList, &ctx->qrSlab, &ctx->lodtab, &ctx->dynFac, &ctx->pvtab, &ctx->outP, &ctx->redbuf, &ctx->redtrip, &ctx->altC, &ctx->rf32, &ctx->btG, &ctx->redflag, &ctx->bperm,
                    &ctx->locoK, &ctx->locoPart, &ctx->locoChr, &ctx->locoStat, &ctx->locoKs, &ctx->locoV, &ctx->locoLraw,
                    &ctx->locoCmx, &ctx->locoCarg, &ctx->locoPerm, &ctx->mdfR, &ctx->mdfT, &ctx->mdfScr,
                    &ctx->effX, &ctx->effIdx, &ctx->effWork, &ctx->effOut, &ctx->effSlab, &ctx->condIdx, &ctx->condWork,
                    &ctx->stepWork, &ctx->stepOut, &ctx->condScr};
  for (DevBuf* b : bufs) if (b->p) hipFree(b->p);
  for (auto& s : ctx->evsets) for (auto& e : s.e) (void)hipEventDestroy(e);
  if (ctx->side) { (void)hipStreamSynchronize(ctx->side); (void)hipStreamDestroy(ctx->side); }
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
  if (ctx->ev_xt) (void)hipEventDestroy(ctx->ev_xt);
  if (ctx->ev_pairs) (void)hipEventDestroy(ctx->ev_pairs);
  if (ctx->ev_b1) (void)hipEventDestroy(ctx->ev_b1);
  if (ctx->ev_b2) (void)hipEventDestroy(ctx->ev_b2);
  if (ctx->ev_q) (void)hipEventDestroy(ctx->ev_q);
  if (ctx->ev_m) (void)hipEventDestroy(ctx->ev_m);
  if (ctx->ev_wb) (void)hipEventDestroy(ctx->ev_wb);
  if (ctx->ev_in) (void)hipEventDestroy(ctx->ev_in);
  if (ctx->ev_inY) (void)hipEventDestroy(ctx->ev_inY);
  if (ctx->ev_call) (void)hipEventDestroy(ctx->ev_call);
  for (auto& g : ctx->gstage) {
    if (g.ev) { (void)hipEventSynchronize(g.ev); (void)hipEventDestroy(g.ev); }
    if (g.h) (void)hipHostFree(g.h);
  }
  if (ctx->copy) { (void)hipStreamSynchronize(ctx->copy); (void)hipStreamDestroy(ctx->copy); }
  if (ctx->side2) { (void)hipStreamSynchronize(ctx->side2); (void)hipStreamDestroy(ctx->side2); }
  if (ctx->own_stream) hipStreamDestroy(ctx->stream);
  if (ctx->hflag) (void)hipHostFree(const_cast<int64_t*>(ctx->hflag));
  destroy_host_stage(ctx->hstage);
  delete ctx;
}

const char* blmm_last_error(const blmm_ctx* ctx) { return ctx ? ctx->err.c_str() : "ctx is NULL"; }

int blmm_set_stream(blmm_ctx* ctx, void* hip_stream) {
  if (!ctx) return BLMM_ERR_INVALID;
  hipStreamSynchronize(ctx->stream);
  if (ctx->own_stream) { hipStreamDestroy(ctx->stream); ctx->own_stream = false; }
  if (hip_stream == BLMM_STREAM_NULL) ctx->stream = nullptr;
  else if (hip_stream) ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
  else {
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) return fail(ctx, BLMM_ERR_HIP, "hipStreamCreate");
    ctx->own_stream = true;
  }
  return BLMM_OK;
}

int blmm_set_timing(blmm_ctx* ctx, int on) {
  if (!ctx) return BLMM_ERR_INVALID;
  ctx->timing = on != 0;
  return BLMM_OK;
}

int blmm_read_timings(blmm_ctx* ctx, double* sums_ms, int64_t* ncalls) {
  if (!ctx || !sums_ms || !ncalls) return BLMM_ERR_INVALID;
  BLMM_HIP(hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < 6; ++i) sums_ms[i] = 0.0;
  for (size_t k = 0; k < ctx->ev_used; ++k) {
    double t[6];
    phase_times(ctx->evsets[k], t);
    for (int i = 0; i < 6; ++i) sums_ms[i] += t[i];
  }
  *ncalls = (int64_t)ctx->ev_used;
  ctx->ev_used = 0;
  return BLMM_OK;
}

int blmm_lowrank_profile(blmm_ctx* ctx, int64_t* out) {
  if (!ctx || !out) return BLMM_ERR_INVALID;
  for (int i = 0; i < 2 + 2 * LR_SEG_MAX; ++i) out[i] = 0;
  if (!ctx->stat.p || !ctx->wbRk.p) return BLMM_OK;           // no null-exact call yet
  BLMM_HIP(hipSetDevice(ctx->device));
  int64_t h[NSTAT];
  int rk[4 * LR_SEG_MAX];
  BLMM_HIP(hipMemcpyAsync(h, ctx->stat.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  BLMM_HIP(hipMemcpyAsync(rk, ctx->wbRk.p, sizeof(rk), hipMemcpyDeviceToHost, ctx->stream));
  BLMM_HIP(hipStreamSynchronize(ctx->stream));
  // the segments in use: those whose rank the basis kernel wrote (a single basis: segment 0 only, the other counts are zero)
  int S = 0;
  for (int s = 0; s < LR_SEG_MAX; ++s) {
    const int64_t cnt = h[24 + s] + h[44 + s];
    if (cnt > 0) { S = s + 1; out[2 + 2 * s] = cnt; out[3 + 2 * s] = rk[4 * s]; }
  }
  out[0] = S; out[1] = h[ST_LR_SHARED0] + h[ST_LR_SHARED1];
  return BLMM_OK;
}

// Diagnostic for tests that report WHERE in the data-dependent panel layout a trait sat (k_lr_classify: two regions split by the
// h2 search's hand-over, in each the shared-weights class from the front and the weight-basis segments from the back): col_out[j] =
// panel column of trait j in the last null-exact call (-1: none), *region_width = columns per region (region = col / width),
// counts_out[4] = {shared-weights traits, columns of the other class} of region 0, then of region 1.
int blmm_lowrank_columns(blmm_ctx* ctx, int64_t m, int32_t* col_out, int64_t* region_width, int64_t* counts_out) {
  if (!ctx || !col_out || m < 0) return BLMM_ERR_INVALID;
  for (int64_t j = 0; j < m; ++j) col_out[j] = -1;
  if (region_width) *region_width = ctx->lr_last_ldq;
  if (counts_out) for (int i = 0; i < 4; ++i) counts_out[i] = 0;
  if (!ctx->lrPerm.p || !ctx->stat.p || ctx->lr_last_ldq <= 0) return BLMM_OK;
  BLMM_HIP(hipSetDevice(ctx->device));
  const int64_t ldq = ctx->lr_last_ldq;
  std::vector<int> perm((size_t)(2 * ldq));
  int64_t h[NSTAT];
  BLMM_HIP(hipMemcpyAsync(perm.data(), ctx->lrPerm.p, sizeof(int) * perm.size(), hipMemcpyDeviceToHost, ctx->stream));
  BLMM_HIP(hipMemcpyAsync(h, ctx->stat.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  BLMM_HIP(hipStreamSynchronize(ctx->stream));
  for (int r = 0; r < 2; ++r) {
    const int64_t nsh = h[ST_LR_SHARED0 + 2 * r], noth = h[ST_LR_OTHER0 + 2 * r];
    if (counts_out) { counts_out[2 * r] = nsh; counts_out[2 * r + 1] = noth; }
    for (int64_t cidx = 0; cidx < ldq; ++cidx) {
      if (!(cidx < nsh || cidx >= ldq - noth)) continue;
      const int t = perm[(size_t)(r * ldq + cidx)];
      if (t >= 0 && t < m) col_out[t] = (int32_t)(r * ldq + cidx);
    }
  }
  return BLMM_OK;
}

int blmm_synchronize(blmm_ctx* ctx) {
  if (!ctx) return BLMM_ERR_INVALID;
  BLMM_HIP(hipStreamSynchronize(ctx->stream));
  return check_sticky(ctx);
}

void blmm_default_opts(blmm_opts* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->method = BLMM_NULL_GRID; o->reml = 0; o->add_intercept = 1; o->decomp_scheme = BLMM_EIGEN;
  o->optim_interval = 1; o->compat_flags = 0; o->prior_variance = 1.0; o->prior_sample_size = 0.0;
}

// What selects another ARITHMETIC path is a property of the context, not of the caller's environment (blmm_internal.h: Tuning).
static const struct { const char* key; int kind; size_t off; double lo, hi; } kTune[] = {
  {"lr_tol", 0, offsetof(blmm::Tuning, lr_tol), 0.0, 1.0},
  {"illcond_rho", 0, offsetof(blmm::Tuning, illcond_rho), 0.0, 1e300},
  {"exact_full_rank", 1, offsetof(blmm::Tuning, exact_full_rank), 0, 1},
  {"pval_libm", 1, offsetof(blmm::Tuning, pval_libm), 0, 1},
  {"pval_fused", 1, offsetof(blmm::Tuning, pval_fused), 0, 1},
  {"lr_segments", 1, offsetof(blmm::Tuning, lr_segments), 0, LR_SEG_MAX},
  {"lr_shared", 1, offsetof(blmm::Tuning, lr_shared), 0, 1},
  {"lr_split", 1, offsetof(blmm::Tuning, lr_split), -1, 1},
  {"eigen_solver", 1, offsetof(blmm::Tuning, eigen_solver), 0, 2},
  {"f32_rotation", 1, offsetof(blmm::Tuning, f32_rotation), 0, 1},
  {"bulk_perm_cols", 1, offsetof(blmm::Tuning, bulk_perm_cols), 0, 2147483647.0},
  {"mdf_red_chunk", 1, offsetof(blmm::Tuning, mdf_red_chunk), 0, 2147483647.0},
  {"cond_red_chunk", 1, offsetof(blmm::Tuning, cond_red_chunk), 0, 2147483647.0},
};
int blmm_set_tuning(blmm_ctx* ctx, const char* key, double value) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (!key) return fail(ctx, BLMM_ERR_INVALID, "set_tuning: key is NULL");
  if (std::strcmp(key, "defaults") == 0) { ctx->tune = blmm::Tuning(); return BLMM_OK; }
  for (const auto& t : kTune)
    if (std::strcmp(key, t.key) == 0) {
      if (!(value >= t.lo && value <= t.hi) || (t.kind == 1 && value != std::floor(value)))
        return fail(ctx, BLMM_ERR_INVALID, std::string("set_tuning: value out of range for ") + key);
      char* base = reinterpret_cast<char*>(&ctx->tune) + t.off;
      if (t.kind == 0) *reinterpret_cast<double*>(base) = value; else *reinterpret_cast<int*>(base) = (int)value;
      return BLMM_OK;
    }
  return fail(ctx, BLMM_ERR_INVALID, std::string("set_tuning: unknown key ") + key);
}
int blmm_get_tuning(const blmm_ctx* ctx, const char* key, double* value) {
  if (!ctx || !key || !value) return BLMM_ERR_INVALID;
  for (const auto& t : kTune)
    if (std::strcmp(key, t.key) == 0) {
      const char* base = reinterpret_cast<const char*>(&ctx->tune) + t.off;
      *value = t.kind == 0 ? *reinterpret_cast<const double*>(base) : (double)*reinterpret_cast<const int*>(base);
      return BLMM_OK;
    }
  return BLMM_ERR_INVALID;
}

// ---------------------------------------------------------------------------------------------------
int blmm_kinship_dev(blmm_ctx* ctx, const double* dG, int64_t n, int64_t p, double* dK_out) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (!dG || !dK_out || n < 1 || p < 1) return fail(ctx, BLMM_ERR_INVALID, "calcKinship: bad arguments");
  BLMM_HIP(hipSetDevice(ctx->device));
  int rc = ensure(ctx, ctx->tmpA, sizeof(double) * (size_t)64 * n * n);
  if (rc) return rc;
  return launch_kinship(ctx, dG, n, p, dK_out, ptr<double>(ctx->tmpA));
}

__global__ void k_round_digits(double* __restrict__ v, int64_t cnt, double scale) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cnt) v[i] = rint(v[i] * scale) / scale;
}

// digits < 0: blmm_kinship
int blmm_kinship_rounded(blmm_ctx* ctx, const double* G, int64_t n, int64_t p, int64_t digits, double* K_out) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (!G || !K_out || n < 1 || p < 1 || digits > 300) return fail(ctx, BLMM_ERR_INVALID, "calcKinship: bad arguments");
  HostCall hc(ctx);
  int rc;
  if ((rc = hc.begin()) || (rc = ensure(ctx, ctx->inK, sizeof(double) * n * n)) || (rc = hc.up(ctx->inG, G, sizeof(double) * n * p))) return rc;
  if ((rc = blmm_kinship_dev(ctx, ptr<double>(ctx->inG), n, p, ptr<double>(ctx->inK)))) return rc;
  if (digits >= 0 && digits <= 17)   // beyond 17 digits rounding a double changes nothing (and 10^digits would overflow)
    hipLaunchKernelGGL(k_round_digits, dim3((unsigned)((n * n + 255) / 256)), dim3(256), 0, ctx->stream, ptr<double>(ctx->inK), n * n, std::pow(10.0, (double)digits));
  if ((rc = hc.down(K_out, ctx->inK.p, sizeof(double) * n * n))) return rc;
  return hc.finish();
}

int blmm_kinship(blmm_ctx* ctx, const double* G, int64_t n, int64_t p, double* K_out) {
  return blmm_kinship_rounded(ctx, G, n, p, -1, K_out);
}

// ---------------------------------------------------------------------------------------------------
int blmm_lod_colmax_dev(blmm_ctx* ctx, const double* dL, int64_t p, int64_t m, int64_t ldL, double* dmax_out, int64_t* dargmax_out) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (!dL || !dmax_out || p < 1 || m < 0 || ldL < p) return fail(ctx, BLMM_ERR_INVALID, "lod_colmax: bad arguments");
  BLMM_HIP(hipSetDevice(ctx->device));
  return launch_colmax(ctx, dL, p, m, ldL, dmax_out, dargmax_out);
}

int blmm_lod_colmax(blmm_ctx* ctx, const double* L, int64_t p, int64_t m, double* max_out, int64_t* argmax_out) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (!L || !max_out || p < 1 || m < 0) return fail(ctx, BLMM_ERR_INVALID, "lod_colmax: bad arguments");
  HostCall hc(ctx);
  const size_t mm = m > 0 ? m : 1;
  int rc;
  if ((rc = hc.begin()) || (rc = hc.up(ctx->outL, L, sizeof(double) * (size_t)p * m)) || (rc = ensure(ctx, ctx->tmpA, sizeof(double) * mm)) ||
      (rc = ensure(ctx, ctx->tmpB, sizeof(int64_t) * mm))) return rc;
  if (m > 0) set_last(ctx, ptr<double>(ctx->outL), p, m);
  if ((rc = launch_colmax(ctx, ptr<double>(ctx->outL), p, m, p, ptr<double>(ctx->tmpA), ptr<int64_t>(ctx->tmpB))) ||
      (rc = hc.down(max_out, ctx->tmpA.p, sizeof(double) * (size_t)m)) || (rc = hc.down(argmax_out, ctx->tmpB.p, sizeof(int64_t) * (size_t)m)))
    return rc;
  return hc.finish();
}

// host-pointer forms of the consumers (upload, reduce on the device, download the small result)
int blmm_lod2log10p(blmm_ctx* ctx, const double* L, int64_t p, int64_t m, int64_t chisq_df, double* P_out) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (!L || !P_out || p < 0 || m < 0 || chisq_df < 1 || chisq_df > 1000000) return fail(ctx, BLMM_ERR_INVALID, "lod2log10p: bad arguments");
  if ((size_t)p * m == 0) return BLMM_OK;
  HostCall hc(ctx);
  int rc;
  if ((rc = hc.begin()) || (rc = ensure(ctx, ctx->altbuf, sizeof(double) * (size_t)p * m * 2))) return rc;
  double* dL = ptr<double>(ctx->altbuf);
  double* dP = dL + (size_t)p * m;
  if ((rc = hc.up(dL, L, sizeof(double) * (size_t)p * m)) || (rc = launch_lod2log10p(ctx, dL, p, m, p, (int)chisq_df, dP, p)) ||
      (rc = copy_to_host(ctx, P_out, dP, sizeof(double) * (size_t)p * m))) return rc;
  return hc.finish(false);
}

int blmm_lod_threshold(blmm_ctx* ctx, const double* L, int64_t p, int64_t m, double thr, int64_t cap, int32_t* i_out,
                       int32_t* j_out, double* lod_out, int64_t* count_out) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (!L || p < 1 || m < 1) return fail(ctx, BLMM_ERR_INVALID, "lod_threshold: bad arguments");
  HostCall hc(ctx);
  int rc;
  if ((rc = hc.begin()) || (rc = hc.up(ctx->outL, L, sizeof(double) * (size_t)p * m))) return rc;
  set_last(ctx, ptr<double>(ctx->outL), p, m);
  if ((rc = blmm_last_lod_threshold(ctx, thr, cap, i_out, j_out, lod_out, count_out))) return rc;
  return hc.finish(false);
}

int blmm_get_thresholds(blmm_ctx* ctx, const double* Lperms, int64_t p, int64_t nperms, const double* probs, int64_t nprobs,
                        double* thrs_out) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (!Lperms || p < 1 || nperms < 1) return fail(ctx, BLMM_ERR_INVALID, "get_thresholds: bad arguments");
  HostCall hc(ctx);
  int rc;
  if ((rc = hc.begin()) || (rc = hc.up(ctx->altbuf, Lperms, sizeof(double) * (size_t)p * nperms)) ||
      (rc = blmm_get_thresholds_dev(ctx, ptr<double>(ctx->altbuf), p, nperms, p, probs, nprobs, thrs_out))) return rc;
  return hc.finish(false);
}

// ---------------------------------------------------------------------------------------------------
// Everything behind the rotations: the h2 search / grid log-likelihoods, the panels and the LOD kernels of one method, then the
// status.  Shared by blmm_bulkscan_dev and blmm_bulkscan_prerotated_dev.
// `output_pvals` inside the scan (blmm_set_log10p_output): resolves the armed request for THIS call.  One degree of freedom and a
// null-* method: the scan kernels write -log10 p from their epilogues (ScanArgs::Pv, set through ctx->pv_cur while they run);
// otherwise (alt-grid: the LOD is only final after the last grid point; other degrees of freedom: incomplete gamma function)
// the column pass of kernels_post.hip runs over the finished L, still inside the call.
extern "C++" {
namespace {
// The request of blmm_set_log10p_output, TAKEN out of the context by the first statement of every bulkscan entry point: whatever
// that call then does -- fail its argument checks, fail in prepare, succeed -- the context is disarmed, so a later unrelated call
// can never write to a stale pointer.
struct PvReq { bool armed = false; double* out = nullptr; int64_t ld = 0, df = 1; };
PvReq pv_take(blmm_ctx* ctx) {
  PvReq r; r.armed = ctx->pv_armed; r.out = ctx->pv_out; r.ld = ctx->pv_ld; r.df = ctx->pv_df;
  ctx->pv_armed = false; ctx->pv_out = nullptr; ctx->pv_ld = 0; ctx->pv_df = 1;
  return r;
}
void pv_hand_over(blmm_ctx* ctx, const PvReq& r) {   // host-pointer entry point -> the *_dev call it makes next
  ctx->pv_armed = r.armed; ctx->pv_out = r.out; ctx->pv_ld = r.ld; ctx->pv_df = r.df;
}
struct PvCall {
  blmm_ctx* ctx; PvReq req; double* P = nullptr; int64_t ld = 0; bool fused = false, owned = false;
  PvCall(blmm_ctx* c, const PvReq& r) : ctx(c), req(r) {}
  ~PvCall() { ctx->pv_cur = nullptr; ctx->pv_cur_ld = 0; }
  // where the request's p x m matrix goes: the caller's buffer (refused when ldP < p) or the context's outP
  int resolve(int64_t p, int64_t m) {
    if (!req.armed) return BLMM_OK;
    if (p <= 0 || m <= 0) return BLMM_OK;
    P = req.out; ld = req.ld;
    if (P && ld < p) { P = nullptr; return fail(ctx, BLMM_ERR_INVALID, "log10p output: ldP < p"); }
    if (!P) {
      int rc = ensure(ctx, ctx->outP, sizeof(double) * (size_t)p * (size_t)m);
      if (rc) return rc;
      P = ptr<double>(ctx->outP); ld = p; owned = true;
    }
    return BLMM_OK;
  }
  int begin(const Pipe& Pp, const blmm_opts* o) {
    int rc = resolve(Pp.p, Pp.m);
    if (rc || !P) return rc;
    const char* pf = dev_env("BLMM_PVAL_FUSED");             // tuning key "pval_fused"
    fused = req.df == 1 && o->method != BLMM_ALT_GRID && (pf ? pf[0] != '0' : ctx->tune.pval_fused != 0);
    if (fused) { ctx->pv_cur = P; ctx->pv_cur_ld = ld; }
    return BLMM_OK;
  }
  // the column pass over the finished L unless the scan epilogues wrote P; a matrix in outP is what blmm_last_log10p serves
  int finish(int64_t p, int64_t m, const double* dL, int64_t ldL) {
    ctx->pv_cur = nullptr; ctx->pv_cur_ld = 0;
    if (!P) return BLMM_OK;
    if (!fused) { int rc = launch_lod2log10p(ctx, dL, p, m, ldL, (int)req.df, P, ld); if (rc) return rc; }
    if (owned) { ctx->last_P = P; ctx->last_P_ld = ld; ctx->last_P_df = req.df; }
    return BLMM_OK;
  }
};
}  // namespace
}  // extern "C++"

// marker norms of every grid point; on the side stream behind the marker rotation when prepare() put that there (P.xt_side), then
// joined into the main stream: the scan that follows needs both
static int isx_maybe_side(blmm_ctx* ctx, const Pipe& P, const NullModel& nm, const double* dgrid, int ngrid) {
  int rc;
  if ((rc = ensure(ctx, ctx->isx, sizeof(double) * (size_t)ngrid * P.ldx))) return rc;
  {
    OnStream on(ctx, P.xt_side ? ctx->side : ctx->stream);
    if ((rc = launch_isx(ctx, nm, P.Xt, P.ldx, P.p, P.Z0, P.lam, dgrid, ngrid, ptr<double>(ctx->isx), P.ldx, P.stat))) return rc;
  }
  if (P.xt_side) {
    BLMM_HIP(hipEventRecord(ctx->ev_join, ctx->side));
    BLMM_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
  }
  return BLMM_OK;
}

static int scan_pipeline(blmm_ctx* ctx, const blmm_opts* opts, Pipe& P, Timer& tm, bool lowrank, bool wbasis_started, double* dgrid,
                         const double* h2_grid_host, int64_t ngrid, double* dL_out, int64_t ldL, double* dh2_out, blmm_status* status,
                         const PvReq& pvreq, int64_t ldH = -1) {   // ldH: leading dimension of alt-grid's h2_panel (-1: p)
  int rc;
  const int64_t m = P.m, p = P.p;
  const NullModel nm = null_model(P, opts);
  const int64_t ldp = P.ldy;
  PvCall pvc(ctx, pvreq);
  if ((rc = pvc.begin(P, opts))) return rc;
  if (m == 0) { tm.mark(); tm.mark(); tm.mark(); return end_call(ctx, P, status, &tm); }
  if (p == 0) {
    // no markers: only the per-trait null model (h2_null_list does not depend on G); alt-grid's h2_panel is p x m = empty
    if (opts->method == BLMM_NULL_EXACT) {
      if ((rc = launch_brent(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, dh2_out, nullptr, nullptr, P.stat))) return rc;
    } else if (opts->method == BLMM_NULL_GRID) {
      if ((rc = ensure(ctx, ctx->h2idx, sizeof(int) * (size_t)m))) return rc;
      if ((rc = launch_loglik_grid(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, dgrid, (int)ngrid, nullptr, ptr<int>(ctx->h2idx), dh2_out, P.stat))) return rc;
    }
    tm.mark(); tm.mark(); tm.mark();
    return end_call(ctx, P, status, &tm);
  }

  if (opts->method == BLMM_NULL_EXACT) {
    if (lowrank) {
      // the basis (started in prepare) and the marker-side products (Q, Xt) run on the side stream beside the
      // per-trait Brent search
      if ((rc = lr_begin(ctx, P, wbasis_started))) return rc;
      // the second kernel of a split h2 search runs beside the scan of the traits the first one finished (BLMM_LR_SPLIT=0: A/B)
      // ... when there are enough traits for two regions (BLMM_LR_SPLIT unset): below ~8 k each region's scan is a few dispatch rounds
      // with their ramps, and one region wins (m = 4445, a rank's share of the BXD problem on 8 GPUs: 0.651 against 0.677 ms per
      // step; m = 8889: 0.777 against 0.776; m = 35554: the split is worth 2.7 %).  BLMM_LR_SPLIT=1: always
      const char* split_env = dev_env("BLMM_LR_SPLIT");                // tuning key "lr_split" (tests hold the two forms against each other)
      // (reduced_async_impl at c >= 2: one region -- its conditioning guard runs ahead of the scan over every trait's final h2;
      // the split and the single-region forms give the same bits, tests/test_gpu_guard.py)
      const bool split_on = (ctx->red_cur.flags && P.c >= 2) ? false
                          : split_env ? split_env[0] != '0' : (ctx->tune.lr_split < 0 ? m >= 8192 : ctx->tune.lr_split != 0);
      BrentSplit sp;
      BrentRot rot;
      if (P.fuseY) { rot.Y = P.fuseY; rot.Rp = ptr<double>(ctx->Rp); rot.Yt = P.Yt; rot.ldr = P.ldr; rot.npad = P.npad; rot.ncols_pad = P.ldy; }
      if ((rc = launch_brent(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, dh2_out, nullptr, nullptr, P.stat, split_on ? 1 : 0, &sp, &rot))) return rc;
      P.fuseY = nullptr;                       // Yt is written
      tm.mark();
      if (sp.active) { if ((rc = lr_finish_split(ctx, P, nm, dh2_out, dL_out, ldL, tm, sp))) return rc; }
      else if ((rc = lr_finish(ctx, P, nm, dh2_out, dL_out, ldL, tm))) return rc;
    } else {
      if ((rc = launch_brent(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, dh2_out, nullptr, nullptr, P.stat))) return rc;
      tm.mark();
      if ((rc = ensure(ctx, ctx->panels, sizeof(double) * (size_t)(2 + P.c) * P.npad * ldp))) return rc;
      if ((rc = launch_panels(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, dh2_out, 1, ptr<double>(ctx->panels), ldp, P.stat))) return rc;
      tm.mark();
      ScanArgs a = scan_args(ctx, P, ptr<double>(ctx->panels), ldp, dL_out, ldL, m);
      if ((rc = launch_scan_exact(ctx, a, P.c))) return rc;
      if ((rc = illcond_rescan(ctx, P, nm, m, dh2_out, dL_out, ldL))) return rc;
      tm.mark();
    }
    if (opts->compat_flags & BLMM_FLAG_H2_AUDIT) {
      // opt-in diagnostic: the profile log-likelihood of every trait on the grid 0, 1/16, .., 15/16 -> n_h2_multimodal
      double gridh[16];
      for (int g = 0; g < 16; ++g) gridh[g] = g / 16.0;
      double* dg = nullptr;
      if ((rc = grid_to_device(ctx, gridh, 16, &dg))) return rc;
      if ((rc = ensure(ctx, ctx->EllTab, sizeof(double) * (size_t)16 * m))) return rc;
      if ((rc = launch_loglik_grid(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, dg, 16, ptr<double>(ctx->EllTab), nullptr, nullptr, P.stat))) return rc;
      if ((rc = launch_h2_audit(ctx, ptr<double>(ctx->EllTab), 16, m, P.stat))) return rc;
      ctx->audit_ran = true;
    }
  } else if (opts->method == BLMM_NULL_GRID) {
    if ((rc = ensure(ctx, ctx->h2idx, sizeof(int) * (size_t)m))) return rc;
    if ((rc = launch_loglik_grid(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, dgrid, (int)ngrid, nullptr, ptr<int>(ctx->h2idx), dh2_out, P.stat))) return rc;
    tm.mark();
    if ((rc = ensure(ctx, ctx->panels, sizeof(double) * (size_t)P.npad * ldp))) return rc;
    if ((rc = launch_panels(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, dh2_out, 0, ptr<double>(ctx->panels), ldp, P.stat))) return rc;
    if ((rc = isx_maybe_side(ctx, P, nm, dgrid, (int)ngrid))) return rc;
    tm.mark();
    ScanArgs a = scan_args(ctx, P, ptr<double>(ctx->panels), ldp, dL_out, ldL, m);
    a.isx = ptr<double>(ctx->isx); a.ld_isx = P.ldx; a.bin = ptr<int>(ctx->h2idx);
    if ((rc = launch_scan_table(ctx, a))) return rc;
    tm.mark();
  } else {  // alt-grid
    if ((rc = ensure(ctx, ctx->EllTab, sizeof(double) * (size_t)ngrid * m))) return rc;
    if ((rc = launch_loglik_grid(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, dgrid, (int)ngrid, ptr<double>(ctx->EllTab), nullptr, nullptr, P.stat))) return rc;
    tm.mark();
    if ((rc = ensure(ctx, ctx->panels, sizeof(double) * (size_t)ngrid * P.npad * ldp))) return rc;
    if ((rc = ensure(ctx, ctx->h2, sizeof(double) * (size_t)m))) return rc;
    if (nm.c <= CTPL) {
      // every grid point's panel in one launch (grid point on blockIdx.y)
      if ((rc = launch_panels(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, nullptr, 0, ptr<double>(ctx->panels), ldp, P.stat, dgrid, (int)ngrid))) return rc;
    } else {
      for (int64_t g = 0; g < ngrid; ++g) {
        if ((rc = fill(ctx, ptr<double>(ctx->h2), m, h2_grid_host[g]))) return rc;
        if ((rc = launch_panels(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, ptr<double>(ctx->h2), 0,
                                ptr<double>(ctx->panels) + (size_t)g * P.npad * ldp, ldp, P.stat))) return rc;
      }
    }
    if ((rc = isx_maybe_side(ctx, P, nm, dgrid, (int)ngrid))) return rc;
    if ((rc = ensure(ctx, ctx->altC, sizeof(double) * (size_t)ngrid * m))) return rc;
    if ((rc = launch_alt_ctab(ctx, ptr<double>(ctx->EllTab), (int)ngrid, m, P.n, ptr<double>(ctx->altC)))) return rc;
    tm.mark();
    AltArgs aa;
    aa.s = scan_args(ctx, P, ptr<double>(ctx->panels), ldp, dL_out, ldL, m);
    aa.s.isx = ptr<double>(ctx->isx); aa.s.ld_isx = P.ldx;
    aa.ngrid = (int)ngrid; aa.EllTab = ptr<double>(ctx->EllTab); aa.grid_dev = dgrid; aa.H2 = dh2_out; aa.ldH = ldH < 0 ? p : ldH;
    aa.Ctab = ptr<double>(ctx->altC);
    aa.counter_quirk = (opts->compat_flags & BLMM_COMPAT_ALT_COUNTER) ? 1 : 0;
    if ((rc = launch_scan_alt(ctx, aa))) return rc;
    tm.mark();
  }
  if ((rc = pvc.finish(p, m, dL_out, ldL))) return rc;
  return end_call(ctx, P, status, &tm);
}

int blmm_set_log10p_output(blmm_ctx* ctx, double* dP_out, int64_t ldP, int64_t chisq_df) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (chisq_df < 0 || chisq_df > 1000000 || (dP_out && ldP < 1)) return fail(ctx, BLMM_ERR_INVALID, "set_log10p_output: bad arguments");
  ctx->pv_armed = chisq_df > 0;
  ctx->pv_out = dP_out; ctx->pv_ld = ldP; ctx->pv_df = chisq_df > 0 ? chisq_df : 1;
  return BLMM_OK;
}

// null-exact runs the low-rank weights form (kernels_lowrank.hip) unless BLMM_EXACT=full (A/B testing), c >= 4 (the
// kernel would spill) or n is beyond what the basis kernel keeps in LDS
static bool exact_full(const blmm_ctx* ctx) {   // tuning key "exact_full_rank"
  const char* e = dev_env("BLMM_EXACT");
  return e ? std::strcmp(e, "full") == 0 : ctx->tune.exact_full_rank != 0;
}
static bool lowrank_form(const blmm_ctx* ctx, int c, int64_t n) { return !exact_full(ctx) && c <= 3 && n <= 6000; }
static bool wants_lowrank(const blmm_ctx* ctx, const blmm_opts* opts, int64_t n, const double* dCovar, int64_t ncov) {
  return opts->method == BLMM_NULL_EXACT && lowrank_form(ctx, (int)null_cov(opts, dCovar, ncov).c, n);
}

// dL_out == nullptr: only with ctx->red_cur set (blmm_bulkscan_reduced: the scan kernels reduce in their epilogues)
static int bulkscan_dev_impl(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG,
                             int64_t p, const double* dCovar, int64_t ncov, const double* dK, const double* dweights,
                             const double* h2_grid_host, int64_t ngrid, double* dL_out, int64_t ldL, double* dh2_out,
                             blmm_status* status, const PvReq& pvreq) {
  int rc = check_opts(ctx, opts);
  if (rc) return rc;
  if (!dY || !dG || !dK || (!dL_out && !ctx->red_cur.pmax) || !dh2_out) return fail(ctx, BLMM_ERR_INVALID, "bulkscan: NULL buffer");
  if (ldL < p) return fail(ctx, BLMM_ERR_INVALID, "bulkscan: ldL < p");
  if ((rc = check_method(ctx, opts)) || (rc = enter_device(ctx))) return rc;
  Timer tm(ctx);
  Pipe P;
  double* dgrid = nullptr;
  if (opts->method != BLMM_NULL_EXACT) {
    if ((rc = grid_to_device(ctx, h2_grid_host, ngrid, &dgrid))) return rc;
  }
  const bool lowrank = wants_lowrank(ctx, opts, n, dCovar, ncov);
  if ((rc = prepare(ctx, opts, dY, n, m, dG, p, dCovar, ncov, dK, dweights, 1, P, tm, lowrank, opts->method != BLMM_NULL_EXACT))) return rc;
  return scan_pipeline(ctx, opts, P, tm, lowrank, /*wbasis_started*/ lowrank && m > 0 && p > 0, dgrid, h2_grid_host, ngrid, dL_out, ldL, dh2_out, status, pvreq);
}

int blmm_bulkscan_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG,
                      int64_t p, const double* dCovar, int64_t ncov, const double* dK, const double* dweights,
                      const double* h2_grid_host, int64_t ngrid, double* dL_out, int64_t ldL, double* dh2_out,
                      blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  const PvReq pvreq = pv_take(ctx);
  ctx->red_cur = RedArgs();
  return bulkscan_dev_impl(ctx, opts, dY, n, m, dG, p, dCovar, ncov, dK, dweights, h2_grid_host, ngrid, dL_out, ldL, dh2_out, status, pvreq);
}

// ---------------------------------------------------------------------------------------------------
// The argument checks of both reduced implementations; `who` prefixes the messages.
static int reduced_check(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                         const double* dK, const blmm_reduced* out, const double* dh2_out, const char* who) {
  int rc = check_opts(ctx, opts);
  if (rc) return rc;
  if (!out || !dY || !dG || !dK || (!dh2_out && opts->method != BLMM_ALT_GRID)) return fail(ctx, BLMM_ERR_INVALID, std::string(who) + ": NULL buffer");
  if (out->cap < 0 || (out->cap > 0 && (!out->ti || !out->tj || !out->tlod)) || (out->want_triplets && !out->count))
    return fail(ctx, BLMM_ERR_INVALID, std::string(who) + ": triplet buffers");
  if ((rc = check_method(ctx, opts))) return rc;
  if (n < 1 || m < 0 || p < 0 || p > 0x7fffffffLL || m > 0x7fffffffLL) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  return BLMM_OK;
}

// The fused route's reduction state over ctx->redbuf: nslot per-(trait, 64-marker slot) partials, the triplet outputs of `out`
static int red_state(blmm_ctx* ctx, const blmm_reduced* out, int64_t nslot, int64_t m, RedArgs* r) {
  const int64_t ldm = round_up(m, 64);
  int rc = ensure(ctx, ctx->redbuf, (sizeof(double) + sizeof(int)) * (size_t)nslot * (size_t)ldm);
  if (rc) return rc;
  r->pmax = ptr<double>(ctx->redbuf); r->parg = reinterpret_cast<int*>(r->pmax + (size_t)nslot * ldm); r->ldm = ldm;
  r->want_trip = out->want_triplets ? 1 : 0; r->thr = out->thr; r->cap = out->cap;
  r->ti = out->ti; r->tj = out->tj; r->tl = out->tlod; r->cnt = reinterpret_cast<unsigned long long*>(out->count);
  if (out->count) BLMM_HIP(hipMemsetAsync(out->count, 0, sizeof(int64_t), ctx->stream));
  return BLMM_OK;
}
// ... for one scan of p markers: 2 ceil(p / 128) slots
static int reduced_args(blmm_ctx* ctx, const blmm_reduced* out, int64_t p, int64_t m, RedArgs* r, int* nslot) {
  *nslot = 2 * (int)((p + 127) / 128);
  return red_state(ctx, out, *nslot, m, r);
}

// The route through a resident L: the whole bulkscan into the context's outL (alt-grid: h2_panel, p x m, into the workspace -- it is
// not part of the reduced result), then k_colmax / k_threshold over it; the blmm_last_* consumers serve that matrix afterwards.
static int reduced_resident(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                            const double* dCovar, int64_t ncov, const double* dK, const double* dweights, const double* h2_grid_host,
                            int64_t ngrid, const blmm_reduced* out, double* dh2_out, blmm_status* status) {
  const int64_t ldL = p > 0 ? p : 1;
  const size_t pm = (size_t)ldL * (size_t)(m > 0 ? m : 1);
  int rc;
  if ((rc = ensure(ctx, ctx->outL, sizeof(double) * pm))) return rc;
  double* dL = ptr<double>(ctx->outL);
  double* dH = dh2_out;
  if (opts->method == BLMM_ALT_GRID) {
    if ((rc = ensure(ctx, ctx->altbuf, sizeof(double) * pm))) return rc;
    dH = ptr<double>(ctx->altbuf);
  }
  if ((rc = bulkscan_dev_impl(ctx, opts, dY, n, m, dG, p, dCovar, ncov, dK, dweights, h2_grid_host, ngrid, dL, ldL, dH, status, PvReq()))) return rc;
  if (m > 0) set_last(ctx, dL, p, m);
  if (out->colmax && m > 0 && (rc = launch_colmax(ctx, dL, p, m, ldL, out->colmax, out->argmax))) return rc;
  if (out->want_triplets && (rc = launch_threshold(ctx, dL, p, m, ldL, out->thr, out->cap, out->ti, out->tj, out->tlod, out->count))) return rc;
  return BLMM_OK;
}

// bulkscan without the LOD matrix (include/bulklmm_hip.h: blmm_bulkscan_reduced).  `out` holds DEVICE pointers here.
// Native route (null-grid; null-exact in the low-rank weights form): the scan kernels' reduce-in-epilogue instantiations write
// per-(trait, 64-marker slot) partial maxima and the triplets, k_red_final finishes the maxima -- L is never written.  The rare
// per-trait re-scans (k_scan_fix: expansion residual of the weight basis; k_scan_qr: ill-conditioned weighted covariates) patch
// columns of a stored L, which does not exist here: the route SPECULATES that no trait is flagged, reads the two device counts at
// the end, and when one is non-zero -- or the method / covariate count has no fused instantiation (alt-grid, c >= 4, BLMM_EXACT=full)
// -- the call runs once more into the context's resident L and reduces it with k_colmax / k_threshold (the same values by
// construction).  Synchronises the stream before it returns.
static int reduced_impl(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                        const double* dCovar, int64_t ncov, const double* dK, const double* dweights, const double* h2_grid_host,
                        int64_t ngrid, const blmm_reduced* out, double* dh2_out, blmm_status* status, int* route_out) {
  int rc = reduced_check(ctx, opts, dY, n, m, dG, p, dK, out, dh2_out, "bulkscan_reduced");
  if (rc) return rc;
  BLMM_HIP(hipSetDevice(ctx->device));
  const bool native = p > 0 && m > 0 && (opts->method == BLMM_NULL_GRID || wants_lowrank(ctx, opts, n, dCovar, ncov));
  if (route_out) *route_out = 0;
  if (native) {
    RedArgs r;
    int nslot;
    if ((rc = reduced_args(ctx, out, p, m, &r, &nslot))) return rc;
    ctx->red_cur = r;
    rc = bulkscan_dev_impl(ctx, opts, dY, n, m, dG, p, dCovar, ncov, dK, dweights, h2_grid_host, ngrid, nullptr, p, dh2_out, status, PvReq());
    ctx->red_cur = RedArgs();
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    if ((rc = launch_red_final(ctx, r, nslot, m, out->colmax, out->argmax))) return rc;
    int64_t h[NSTAT];
    BLMM_HIP(hipMemcpyAsync(h, ctx->stat.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    BLMM_HIP(hipStreamSynchronize(ctx->stream));
    if ((rc = check_sticky(ctx))) return rc;
    if (h[ST_LR_FIX] == 0 && h[ST_ILLCOND] == 0) { if (route_out) *route_out = 1; return BLMM_OK; }
  }
  if ((rc = reduced_resident(ctx, opts, dY, n, m, dG, p, dCovar, ncov, dK, dweights, h2_grid_host, ngrid, out, dh2_out, status))) {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  BLMM_HIP(hipStreamSynchronize(ctx->stream));
  if (route_out) *route_out = 2;
  return check_sticky(ctx);
}

int blmm_bulkscan_reduced_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG,
                              int64_t p, const double* dCovar, int64_t ncov, const double* dK, const double* dweights,
                              const double* h2_grid_host, int64_t ngrid, const blmm_reduced* out, double* dh2_out,
                              blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  (void)pv_take(ctx);
  return reduced_impl(ctx, opts, dY, n, m, dG, p, dCovar, ncov, dK, dweights, h2_grid_host, ngrid, out, dh2_out, status, &ctx->last_reduced_route);
}

// ---------------------------------------------------------------------------------------------------
// One process per GPU (torch.distributed / MPI hosts): the pipeline in three calls, so that the marker rotation -- replicated
// work when every rank runs blmm_bulkscan_dev on the full G -- is SHARDED.  At n >= 500 it is 10-25 % of a rank's step
// (configs[4]: 3.8 ms of 16.5), against ~0.7 ms for an all-gather of the rotated blocks over xGMI; the eigen-decomposition stays
// replicated (broadcasting U would synchronise all devices in the middle of the call).
//   blmm_prepare_dev               design, eigen, post-eigen: the context then holds U, lambda, Z0 and the rotation matrix
//   blmm_rotate_block_dev          rank r rotates ITS column block of G into a k-major block (rows = blmm_rotated_rows())
//   [the host all-gathers the blocks: RCCL ncclAllGather / torch.distributed.all_gather_into_tensor]
//   blmm_bulkscan_prerotated_dev   assembles Xt from the gathered blocks, rotates this rank's traits, runs the method
// A marker's rotated column is the same bits whichever rank and block shape produced it (fixed summation order), so the result
// equals blmm_bulkscan_dev's bit for bit (tests/test_gpu_configs.py).
int blmm_prepare_dev(blmm_ctx* ctx, const blmm_opts* opts, int64_t n, const double* dCovar, int64_t ncov, const double* dK,
                     const double* dweights, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  int rc = check_opts(ctx, opts);
  if (rc) return rc;
  if (!dK) return fail(ctx, BLMM_ERR_INVALID, "prepare: NULL buffer");
  if ((rc = enter_device(ctx))) return rc;
  ctx->prep_valid = false;
  Timer tm(ctx);
  Pipe P;
  if ((rc = prepare_eigen(ctx, opts, n, dCovar, ncov, dK, dweights, 1, P, tm))) return rc;
  ctx->prep = P;
  ctx->prep_valid = true;
  return end_call(ctx, P, status, &tm);
}

// The state blmm_prepare_dev left, with the device pointers taken from the workspace as it is NOW (never from the copy)
static Pipe prepared_pipe(blmm_ctx* ctx) {
  Pipe P = ctx->prep;
  P.Z0 = ptr<double>(ctx->Z0); P.lam = ptr<double>(ctx->lam); P.stat = ptr<int64_t>(ctx->stat);
  P.Yt = nullptr; P.Xt = nullptr;
  return P;
}

int64_t blmm_rotated_rows(const blmm_ctx* ctx) { return (ctx && ctx->prep_valid) ? ctx->prep.npad : 0; }

int blmm_rotate_block_dev(blmm_ctx* ctx, const double* dG_block, int64_t pb, double* dXt_block, int64_t ld) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (!ctx->prep_valid) return fail(ctx, BLMM_ERR_INVALID, "rotate_block: blmm_prepare_dev has not run on this context");
  if (!dG_block || !dXt_block || pb < 0 || ld < pb) return fail(ctx, BLMM_ERR_INVALID, "rotate_block: bad arguments");
  BLMM_HIP(hipSetDevice(ctx->device));
  const Pipe P = prepared_pipe(ctx);
  return launch_rotate(ctx, ptr<double>(ctx->Rp), P.ldr, P.n, P.npad, dG_block, pb, dXt_block, ld, ld);
}

// Xt (k-major, npad x ldx) from the gathered blocks [nblocks][npad][block_ld]: block b holds the columns [b block_cols, ..)
static int assemble_prerotated(blmm_ctx* ctx, Pipe& P, int64_t p, const double* dXt_blocks, int64_t nblocks, int64_t block_cols,
                               int64_t block_ld) {
  int rc;
  P.p = p; P.ldx = round_up(p > 0 ? p : 1, 128);
  if ((rc = ensure(ctx, ctx->Xt, sizeof(double) * (size_t)P.npad * P.ldx))) return rc;
  P.Xt = ptr<double>(ctx->Xt);
  if (P.ldx > p) BLMM_HIP(hipMemset2DAsync(P.Xt + p, sizeof(double) * P.ldx, 0, sizeof(double) * (P.ldx - p), P.npad, ctx->stream));
  for (int64_t b = 0; b < nblocks; ++b) {
    const int64_t lo = b * block_cols, hi = (lo + block_cols < p) ? lo + block_cols : p;
    if (hi <= lo) break;
    BLMM_HIP(hipMemcpy2DAsync(P.Xt + lo, sizeof(double) * P.ldx, dXt_blocks + (size_t)b * P.npad * block_ld, sizeof(double) * block_ld,
                              sizeof(double) * (hi - lo), P.npad, hipMemcpyDeviceToDevice, ctx->stream));
  }
  return BLMM_OK;
}

// A scan on the state blmm_prepare_dev left: its counters start from zero except what the eigen-decomposition left (negative
// eigenvalues, its sweeps and clocks); the eigen and rotation phases have nothing to time
static int reset_prepared(blmm_ctx* ctx, const Pipe& P, Timer& tm) {
  BLMM_HIP(hipMemsetAsync(P.stat + ST_NONPOS_W, 0, sizeof(int64_t) * (ST_JACOBI_SWEEPS - ST_NONPOS_W), ctx->stream));
  BLMM_HIP(hipMemsetAsync(P.stat + ST_LR_RANK, 0, sizeof(int64_t) * (NSTAT - ST_LR_RANK), ctx->stream));
  ctx->audit_ran = false;
  ctx->brent_cnt_used = false;
  tm.mark(); tm.mark();
  return BLMM_OK;
}

int blmm_bulkscan_prerotated_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t m, int64_t p,
                                 const double* dXt_blocks, int64_t nblocks, int64_t block_cols, int64_t block_ld,
                                 const double* h2_grid_host, int64_t ngrid, double* dL_out, int64_t ldL, double* dh2_out,
                                 blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  const PvReq pvreq = pv_take(ctx);
  int rc = check_opts(ctx, opts);
  if (rc) return rc;
  if (!ctx->prep_valid) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_prerotated: blmm_prepare_dev has not run on this context");
  if (!dY || !dXt_blocks || !dL_out || !dh2_out) return fail(ctx, BLMM_ERR_INVALID, "bulkscan: NULL buffer");
  if (m < 0 || p < 0 || nblocks < 1 || block_cols < 1 || block_ld < block_cols || nblocks * block_cols < p)
    return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  if (ldL < p) return fail(ctx, BLMM_ERR_INVALID, "bulkscan: ldL < p");
  if ((rc = check_method(ctx, opts)) || (rc = enter_device(ctx))) return rc;
  Timer tm(ctx);
  Pipe P = prepared_pipe(ctx);
  double* dgrid = nullptr;
  if (opts->method != BLMM_NULL_EXACT) {
    if ((rc = grid_to_device(ctx, h2_grid_host, ngrid, &dgrid))) return rc;
  }
  if ((rc = reset_prepared(ctx, P, tm))) return rc;
  const bool lowrank = opts->method == BLMM_NULL_EXACT && lowrank_form(ctx, P.c, P.n);
  if (lowrank && m > 0 && p > 0 && (rc = start_wbasis(ctx, P))) return rc;
  if ((rc = rotate_traits(ctx, P, dY, m))) return rc;
  if ((rc = assemble_prerotated(ctx, P, p, dXt_blocks, nblocks, block_cols, block_ld))) return rc;
  tm.mark();
  return scan_pipeline(ctx, opts, P, tm, lowrank, lowrank && m > 0 && p > 0, dgrid, h2_grid_host, ngrid, dL_out, ldL, dh2_out, status, pvreq);
}

// L_out == NULL: the matrix stays in HBM (2.08 GB at BXD size: 36 of the call's 39 ms are its trip over PCIe) and the blmm_last_*
// consumers serve it -- peaks, LOD > t triplets, permutation quantiles, -log10 p, single columns (README.md:246-255, 354-359;
// src/analysis_helpers/single_trait_analysis.jl:13-23 are what the reference's users do with L).  alt-grid: h2_out (the p x m
// h2_panel) may be NULL likewise.
int blmm_bulkscan(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                  const double* Covar, int64_t ncov, const double* K, const double* weights, const double* h2_grid,
                  int64_t ngrid, double* L_out, double* h2_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  const PvReq pvreq = pv_take(ctx);
  if (!opts) return fail(ctx, BLMM_ERR_INVALID, "opts is NULL");
  const bool alt = opts->method == BLMM_ALT_GRID;
  if (!Y || !G || !K || (!h2_out && !alt)) return fail(ctx, BLMM_ERR_INVALID, "bulkscan: NULL buffer");
  if (n < 1 || m < 0 || p < 0) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  HostCall hc(ctx);
  int rc;
  const size_t h2_elems = alt ? (size_t)p * m : (size_t)m;
  if ((rc = hc.begin()) || (rc = ensure(ctx, ctx->outL, sizeof(double) * (size_t)p * m)) || (rc = ensure(ctx, ctx->outH2, sizeof(double) * h2_elems)))
    return rc;
  // BLMM_HOST_PROF=1: wall-clock of the call's legs on stderr (diagnostic: it synchronises between them)
  static const bool hprof = getenv("BLMM_HOST_PROF") && getenv("BLMM_HOST_PROF")[0] == '1';
  auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double hp0 = hprof ? now() : 0.0;
  HostCall::In d;
  if ((rc = hc.inputs(Y, n, m, G, p, K, Covar, ncov, weights, /*defer*/ true, &d))) return rc;
  if (hprof) (void)hipStreamSynchronize(ctx->stream);
  const double hp1 = hprof ? now() : 0.0;
  pv_hand_over(ctx, pvreq);
  if ((rc = blmm_bulkscan_dev(ctx, opts, d.Y, n, m, d.G, p, d.Cov, d.ncov, d.K, d.W, h2_grid, ngrid, ptr<double>(ctx->outL), p,
                              ptr<double>(ctx->outH2), status))) return rc;
  const double hp2 = hprof ? now() : 0.0;
  if (hprof) (void)hipStreamSynchronize(ctx->stream);
  const double hp3 = hprof ? now() : 0.0;
  set_last(ctx, ptr<double>(ctx->outL), p, m);
  if (L_out && (size_t)p * m > 0 && (rc = copy_to_host(ctx, L_out, ctx->outL.p, sizeof(double) * (size_t)p * m))) return rc;
  const double hp4 = hprof ? now() : 0.0;
  if (h2_out && h2_elems > 0 && (rc = copy_to_host(ctx, h2_out, ctx->outH2.p, sizeof(double) * h2_elems))) return rc;
  if ((rc = hc.finish())) return rc;
  if (hprof)
    fprintf(stderr, "blmm_bulkscan legs (ms): uploads %.2f | enqueue %.2f | device %.2f | L to host %.2f | h2 to host + sync %.2f\n", hp1 - hp0, hp2 - hp1,
            hp3 - hp2, hp4 - hp3, now() - hp4);
  return check_sticky(ctx);   // a device-side failure of THIS call (no status passed): reported now, not by the next call
}

// ---------------------------------------------------------------------------------------------------
// Leave-one-chromosome-out (include/bulklmm_hip.h: blmm_kinship_loco, blmm_bulkscan_loco).  The argument checks come before anything
// touches the device.
static int loco_check(blmm_ctx* ctx, int64_t n, int64_t p, const int64_t* chr, int64_t nchr, const char* who) {
  const std::string w(who);
  if (n < 1 || p < 1) return fail(ctx, BLMM_ERR_INVALID, w + ": bad arguments");
  if (!chr) return fail(ctx, BLMM_ERR_INVALID, w + ": chr_start is NULL");
  if (nchr < 2) return fail(ctx, BLMM_ERR_INVALID, w + ": leave-one-chromosome-out needs at least 2 chromosomes");
  if (nchr > 65535) return fail(ctx, BLMM_ERR_INVALID, w + ": at most 65535 chromosomes");
  if (chr[0] != 0 || chr[nchr] != p) return fail(ctx, BLMM_ERR_INVALID, w + ": chromosome offsets must run from 0 to p");
  for (int64_t c = 0; c < nchr; ++c) {
    if (chr[c + 1] == chr[c]) return fail(ctx, BLMM_ERR_INVALID, w + ": chromosome " + std::to_string((long long)c) + " is empty");
    if (chr[c + 1] < chr[c]) return fail(ctx, BLMM_ERR_INVALID, w + ": chromosome offsets are not increasing");
    if (chr[c + 1] - chr[c] == p) return fail(ctx, BLMM_ERR_INVALID, w + ": a chromosome holds every marker (no kinship is left)");
  }
  return BLMM_OK;
}

// the chromosome offsets on the device (locoChr), in stream order and without waiting (stage_to_device)
static int loco_offsets(blmm_ctx* ctx, const int64_t* chr, int64_t nchr, const int64_t** dchr) {
  const size_t bytes = sizeof(int64_t) * (size_t)(nchr + 1);
  int rc;
  if ((rc = ensure(ctx, ctx->locoChr, bytes)) || (rc = stage_to_device(ctx, ctx->locoChr, chr, bytes))) return rc;
  *dchr = ptr<int64_t>(ctx->locoChr);
  return BLMM_OK;
}

static int kinship_loco_impl(blmm_ctx* ctx, const double* dG, int64_t n, const int64_t* chr, int64_t nchr, int64_t digits, double* dK) {
  const int64_t* dchr = nullptr;
  const int ns = loco_kinship_splits(n, nchr);
  int rc;
  if ((rc = loco_offsets(ctx, chr, nchr, &dchr)) || (rc = ensure(ctx, ctx->locoPart, sizeof(double) * (size_t)nchr * ns * n * n))) return rc;
  return launch_kinship_loco(ctx, dG, n, dchr, nchr, digits, dK, ptr<double>(ctx->locoPart), ns);
}

int blmm_kinship_loco_dev(blmm_ctx* ctx, const double* dG, int64_t n, int64_t p, const int64_t* chr_start, int64_t nchr,
                          int64_t digits, double* dK_out) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (!dG || !dK_out || digits > 300) return fail(ctx, BLMM_ERR_INVALID, "kinship_loco: bad arguments");
  int rc = loco_check(ctx, n, p, chr_start, nchr, "kinship_loco");
  if (rc) return rc;
  BLMM_HIP(hipSetDevice(ctx->device));
  return kinship_loco_impl(ctx, dG, n, chr_start, nchr, digits, dK_out);
}

int blmm_kinship_loco(blmm_ctx* ctx, const double* G, int64_t n, int64_t p, const int64_t* chr_start, int64_t nchr,
                      int64_t digits, double* K_out) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (!G || !K_out || digits > 300) return fail(ctx, BLMM_ERR_INVALID, "kinship_loco: bad arguments");
  int rc = loco_check(ctx, n, p, chr_start, nchr, "kinship_loco");
  if (rc) return rc;
  HostCall hc(ctx);
  const size_t kb = sizeof(double) * (size_t)n * n * nchr;
  if ((rc = hc.begin()) || (rc = ensure(ctx, ctx->locoK, kb)) || (rc = hc.up(ctx->inG, G, sizeof(double) * n * p)) ||
      (rc = kinship_loco_impl(ctx, ptr<double>(ctx->inG), n, chr_start, nchr, digits, ptr<double>(ctx->locoK))) ||
      (rc = copy_to_host(ctx, K_out, ctx->locoK.p, kb))) return rc;
  return hc.finish(false);
}

// blmm_bulkscan_loco_reduced: what each chromosome's scan produces instead of its rows of L.  fused: the scan epilogues reduce into
// the chromosome's own range of r's slot partials (slot0[c], by chromosome index) and append their triplets with the chromosome's
// first marker as row offset (RedArgs::row0); the guards flag traits into r.flags, zeroed for each chromosome, and k_scan_fix /
// k_scan_qr re-scan those into the same partials.  Otherwise (route 2) the chromosome's rows go to a resident block of ld rows
// (outL, sized by the largest chromosome), which k_colmax and k_threshold reduce into cmx / carg and the triplets before the next
// chromosome overwrites it.  Either way launch_red_final_loco merges the chromosomes after the last one.
struct LocoRed {
  const blmm_reduced* out = nullptr;   // device pointers
  bool fused = false;
  RedArgs r;
  std::vector<int64_t> slot0;
  double* cmx = nullptr; int64_t* carg = nullptr;   // nchr x m (fused: may be null)
  int64_t ld = 0;
};

// The chromosomes largest first (blmm_bulkscan_loco's run order), ties in genome order
static std::vector<int64_t> loco_order(const int64_t* chr, int64_t nchr) {
  std::vector<int64_t> order((size_t)nchr);
  for (int64_t c = 0; c < nchr; ++c) order[(size_t)c] = c;
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return chr[a + 1] - chr[a] > chr[b + 1] - chr[b]; });
  return order;
}

// per-matrix strides of the batched eigen phase's workspace (locoKs, locoV, locoLraw)
static int64_t loco_sA(int64_t n) { return round_up(n * n, 32); }
static int64_t loco_sE(int64_t n) { return round_up(n * n + 4 * n + 16, 32); }
static int64_t loco_sL(int64_t n) { return round_up(n, 32); }

// n <= eig_fast_max_n() (the fast path is what a single call runs there): the design of every chromosome's kinship, then ONE set of
// eigen launches for all of them (launch_eig_fast_batch: matrix c on blockIdx.y, its own workspace and status words); each
// chromosome's prepare_eigen runs only the Jacobi check behind it and the post-eigen work (loco_eig_pre).  Beyond: per chromosome,
// unbatched (*batched = false).
static int loco_eigen_batch(blmm_ctx* ctx, const blmm_opts* opts, int64_t n, const double* dK, int64_t nchr, const double* dCovar,
                            int64_t ncov, const double* dweights, int64_t* dst_all, Timer& tb, bool* batched) {
  *batched = n >= 3 && n <= eig_fast_max_n() && !dev_env("BLMM_EIGEN") && ctx->tune.eigen_solver == 0;
  if (!*batched) return BLMM_OK;
  const int64_t sA = loco_sA(n), sE = loco_sE(n), sL = loco_sL(n);
  const NullCov nc = null_cov(opts, dCovar, ncov);
  if (nc.c < 1 || nc.c > CMAX) return fail(ctx, BLMM_ERR_UNSUPPORTED, BLMM_C_ERR);
  if (nc.c >= n) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  int rc;
  if ((rc = ensure(ctx, ctx->locoKs, sizeof(double) * (size_t)nchr * sA)) || (rc = ensure(ctx, ctx->locoV, sizeof(double) * (size_t)nchr * sE)) ||
      (rc = ensure(ctx, ctx->locoLraw, sizeof(double) * (size_t)nchr * sL)) || (rc = ensure(ctx, ctx->Zs, sizeof(double) * n * nc.c))) return rc;
  BLMM_HIP(hipMemsetAsync(dst_all, 0, sizeof(int64_t) * NSTAT * (size_t)nchr, ctx->stream));
  tb.mark();
  for (int64_t c = 0; c < nchr; ++c)
    if ((rc = launch_design(ctx, dK + (size_t)c * n * n, nc.d, (int)nc.ncov, nc.add_int, dweights, (int)n, ptr<double>(ctx->locoKs) + (size_t)c * sA,
                            ptr<double>(ctx->Zs)))) return rc;
  if ((rc = launch_eig_fast_batch(ctx, ptr<double>(ctx->locoKs), sA, (int)n, (int)nchr, ptr<double>(ctx->locoLraw), sL,
                                  ptr<double>(ctx->locoV), sE, dst_all, NSTAT))) return rc;
  tb.mark();
  return BLMM_OK;
}

// chromosome c's share of the batched eigen phase (prepare's `pre`; used only when loco_eigen_batch ran)
static EigPre loco_eig_pre(blmm_ctx* ctx, int64_t n, int64_t c, int64_t* dst_all) {
  return EigPre{ptr<double>(ctx->locoKs) + (size_t)c * loco_sA(n), ptr<double>(ctx->locoV) + (size_t)c * loco_sE(n),
                ptr<double>(ctx->locoLraw) + (size_t)c * loco_sL(n), dst_all + (size_t)c * NSTAT};
}

// after chromosome c: the next one reuses every buffer this one's side-stream work reads, so the main stream waits for both side
// streams; its status block goes aside (dst_all + c NSTAT) unless the batched eigen phase already kept it there
static int loco_chr_done(blmm_ctx* ctx, const Pipe& P, int64_t c, int64_t* dst_all) {
  BLMM_HIP(hipEventRecord(ctx->ev_fork, ctx->side));
  BLMM_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_fork, 0));
  BLMM_HIP(hipEventRecord(ctx->ev_fork, ctx->side2));
  BLMM_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_fork, 0));
  if (P.stat != dst_all + (size_t)c * NSTAT)
    BLMM_HIP(hipMemcpyAsync(dst_all + (size_t)c * NSTAT, P.stat, sizeof(int64_t) * NSTAT, hipMemcpyDeviceToDevice, ctx->stream));
  return BLMM_OK;
}

// the context's status block is what blmm_lowrank_profile / blmm_lowrank_columns read: the last chromosome's, as after a run of
// single calls (the batched path kept every chromosome's block in locoStat instead)
static int loco_last_stat(blmm_ctx* ctx, bool batched, const std::vector<int64_t>& order, const int64_t* dst_all) {
  if (!batched || order.empty()) return BLMM_OK;
  int rc;
  if ((rc = ensure(ctx, ctx->stat, sizeof(int64_t) * NSTAT))) return rc;
  BLMM_HIP(hipMemcpyAsync(ctx->stat.p, dst_all + (size_t)order.back() * NSTAT, sizeof(int64_t) * NSTAT, hipMemcpyDeviceToDevice, ctx->stream));
  return BLMM_OK;
}

static int loco_status(blmm_ctx* ctx, const int64_t* dst_all, int64_t nchr, bool audit, const Timer& t0, const Timer& tb,
                       const std::vector<Timer>& tms, blmm_status* status);

// The pipeline: the kinships (unless given), then per chromosome the whole bulkscan front and scan on its column block, into its rows
// of L (or, red given, into its reduction).  The chromosomes run largest first, so that no p-sized workspace grows -- and no buffer is
// freed under queued work -- after the first of them; each one's status block is copied aside (locoStat) and summed once at the end.
static int loco_pipeline(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                         const int64_t* chr, int64_t nchr, int64_t kdigits, const double* dCovar, int64_t ncov, const double* dweights,
                         const double* h2_grid_host, int64_t ngrid, const double* dK_loco, double* dL, int64_t ldL, double* dh2,
                         blmm_status* status, const PvReq& pvreq, LocoRed* red) {
  int rc;
  double* dgrid = nullptr;
  if (opts->method != BLMM_NULL_EXACT && (rc = grid_to_device(ctx, h2_grid_host, ngrid, &dgrid))) return rc;
  // one event set for the start of the call (t_total_ms spans the kinships computed inside it, which count in no phase), one for the
  // batched eigen phase, one per chromosome: none may be reallocated or recycled under another one's Timer
  if (ctx->ev_used + (size_t)nchr + 2 >= 4096) ctx->ev_used = 0;
  ctx->evsets.reserve(ctx->ev_used + (size_t)nchr + 2);
  Timer t0(ctx);
  t0.mark();
  const double* dK = dK_loco;
  if (!dK) {
    if ((rc = ensure(ctx, ctx->locoK, sizeof(double) * (size_t)n * n * nchr)) ||
        (rc = kinship_loco_impl(ctx, dG, n, chr, nchr, kdigits, ptr<double>(ctx->locoK)))) return rc;
    dK = ptr<double>(ctx->locoK);
  }
  if ((rc = ensure(ctx, ctx->locoStat, sizeof(int64_t) * NSTAT * (size_t)nchr))) return rc;
  int64_t* dst_all = ptr<int64_t>(ctx->locoStat);
  const std::vector<int64_t> order = loco_order(chr, nchr);
  Timer tb(ctx);
  bool batched = false;
  if ((rc = loco_eigen_batch(ctx, opts, n, dK, nchr, dCovar, ncov, dweights, dst_all, tb, &batched))) return rc;
  std::vector<Timer> tms;
  tms.reserve((size_t)nchr);
  const bool alt = opts->method == BLMM_ALT_GRID;
  const bool lowrank = wants_lowrank(ctx, opts, n, dCovar, ncov);
  bool audit = false;
  for (int64_t c : order) {
    const int64_t s0 = chr[c], pc = chr[c + 1] - chr[c];
    tms.emplace_back(ctx);
    Timer& tm = tms.back();
    Pipe P;
    const EigPre pre = loco_eig_pre(ctx, n, c, dst_all);
    if ((rc = prepare(ctx, opts, dY, n, m, dG + (size_t)n * s0, pc, dCovar, ncov, dK + (size_t)c * n * n, dweights, 1, P, tm, lowrank,
                      opts->method != BLMM_NULL_EXACT, false, batched ? &pre : nullptr)))
      return rc;
    double* h2c = alt ? (dh2 ? dh2 + s0 : nullptr) : dh2 + (size_t)c * m;
    if (alt && !h2c) {   // the h2_panel was not asked for: the context's scratch (p x m at most, this chromosome's rows only)
      if ((rc = ensure(ctx, ctx->outH2, sizeof(double) * (size_t)pc * (m > 0 ? m : 1)))) return rc;
      h2c = ptr<double>(ctx->outH2);
    }
    double* Lc = dL ? dL + s0 : nullptr;
    int64_t ldc = ldL;
    if (red && red->fused) {
      RedArgs r = red->r;
      r.pmax += (size_t)red->slot0[(size_t)c] * r.ldm; r.parg += (size_t)red->slot0[(size_t)c] * r.ldm; r.row0 = s0;
      BLMM_HIP(hipMemsetAsync(r.flags, 0, sizeof(int) * (size_t)m, ctx->stream));
      ctx->red_cur = r;
    } else if (red) {
      Lc = ptr<double>(ctx->outL); ldc = red->ld;
    }
    rc = scan_pipeline(ctx, opts, P, tm, lowrank, lowrank && m > 0, dgrid, h2_grid_host, ngrid, Lc, ldc, h2c, nullptr, PvReq(),
                       (alt && dh2) ? p : pc);
    ctx->red_cur = RedArgs();
    if (rc) return rc;
    if (red && !red->fused) {
      const blmm_reduced* o = red->out;
      if ((rc = launch_colmax_rows(ctx, Lc, pc, m, ldc, red->cmx + (size_t)c * m, red->carg + (size_t)c * m, s0))) return rc;
      if (o->want_triplets && (rc = launch_threshold_rows(ctx, Lc, pc, m, ldc, o->thr, o->cap, o->ti, o->tj, o->tlod, o->count, s0))) return rc;
    }
    audit = audit || ctx->audit_ran;
    if ((rc = loco_chr_done(ctx, P, c, dst_all))) return rc;
  }
  if ((rc = loco_last_stat(ctx, batched, order, dst_all))) return rc;
  if (red) {
    const int64_t* dchr = nullptr;
    const bool sl = red->fused;
    if ((rc = loco_offsets(ctx, chr, nchr, &dchr)) ||
        (rc = launch_red_final_loco(ctx, sl ? red->r.pmax : nullptr, sl ? red->r.parg : nullptr, red->r.ldm, dchr, nchr, m, red->cmx, red->carg,
                                    red->out->colmax, red->out->argmax))) return rc;
  }
  PvCall pvc(ctx, pvreq);                    // (never fused: a column pass over the finished L)
  if ((rc = pvc.resolve(p, m)) || (rc = pvc.finish(p, m, dL, ldL))) return rc;
  return loco_status(ctx, dst_all, nchr, audit, t0, tb, tms, status);
}

// The chromosomes' status blocks (dst_all, nchr x NSTAT) summed into *status, with the phase times of every chromosome's Timer (tms),
// the batched eigen phase (tb) and the whole call from t0's mark; nothing without a status.
static int loco_status(blmm_ctx* ctx, const int64_t* dst_all, int64_t nchr, bool audit, const Timer& t0, const Timer& tb,
                       const std::vector<Timer>& tms, blmm_status* status) {
  if (!status) return BLMM_OK;
  int rc;
  std::vector<int64_t> h((size_t)nchr * NSTAT);
  BLMM_HIP(hipMemcpyAsync(h.data(), dst_all, sizeof(int64_t) * h.size(), hipMemcpyDeviceToHost, ctx->stream));
  BLMM_HIP(hipStreamSynchronize(ctx->stream));
  blmm_status sum;
  std::memset(&sum, 0, sizeof(sum));
  for (int64_t c = 0; c < nchr; ++c) {
    blmm_status one;
    if ((rc = fill_status(ctx, h.data() + (size_t)c * NSTAT, &one))) return rc;
    add_status(&sum, one);
  }
  if (!audit) sum.n_h2_multimodal = -1;
  for (const Timer& tm : tms) add_phase_times(&sum, tm);
  if (tb.set && tb.set->n >= 2) {            // the batched eigen phase (the chromosomes' own eigen phases are their post-eigen work)
    float te = 0;
    (void)hipEventElapsedTime(&te, tb.set->e[0], tb.set->e[1]);
    sum.t_eigen_ms += te;
  }
  if (!tms.empty() && tms.front().set && tms.back().set && tms.back().set->n >= 2) {
    float tot = 0;
    const hipEvent_t first = t0.set ? t0.set->e[0] : tms.front().set->e[0];
    (void)hipEventElapsedTime(&tot, first, tms.back().set->e[tms.back().set->n - 1]);
    sum.t_total_ms = tot;
  }
  *status = sum;
  return BLMM_OK;
}

static int bulkscan_loco_dev_impl(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG,
                                  int64_t p, const int64_t* chr, int64_t nchr, int64_t kdigits, const double* dCovar, int64_t ncov,
                                  const double* dweights, const double* h2_grid_host, int64_t ngrid, const double* dK_loco,
                                  double* dL, int64_t ldL, double* dh2, blmm_status* status, const PvReq& pvreq) {
  int rc = check_opts(ctx, opts);
  if (rc) return rc;
  if (!dY || !dG || !dL || (!dh2 && opts->method != BLMM_ALT_GRID)) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_loco: NULL buffer");
  if ((rc = check_method(ctx, opts)) || (rc = loco_check(ctx, n, p, chr, nchr, "bulkscan_loco"))) return rc;
  if (m < 0 || ldL < p || kdigits > 300) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_loco: bad arguments");
  if (n > 2048) return fail(ctx, BLMM_ERR_UNSUPPORTED, "more than 2048 individuals: the device eigensolver (tridiagonalisation + divide and conquer) stops at n = 2048");
  if ((rc = enter_device(ctx))) return rc;
  return loco_pipeline(ctx, opts, dY, n, m, dG, p, chr, nchr, kdigits, dCovar, ncov, dweights, h2_grid_host, ngrid, dK_loco, dL, ldL, dh2,
                       status, pvreq, nullptr);
}

int blmm_bulkscan_loco_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                           const int64_t* chr_start, int64_t nchr, int64_t kinship_digits, const double* dCovar, int64_t ncov,
                           const double* dweights, const double* h2_grid, int64_t ngrid, const double* dK_loco, double* dL_out,
                           int64_t ldL, double* dh2_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  const PvReq pvreq = pv_take(ctx);
  ctx->red_cur = RedArgs();
  if (ncov == 0) dCovar = nullptr;
  return bulkscan_loco_dev_impl(ctx, opts, dY, n, m, dG, p, chr_start, nchr, kinship_digits, dCovar, dCovar ? ncov : 0, dweights, h2_grid,
                                ngrid, dK_loco, dL_out, ldL, dh2_out, status, pvreq);
}

int blmm_bulkscan_loco(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                       const int64_t* chr_start, int64_t nchr, int64_t kinship_digits, const double* Covar, int64_t ncov,
                       const double* weights, const double* h2_grid, int64_t ngrid, double* L_out, double* h2_out,
                       blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  const PvReq pvreq = pv_take(ctx);
  if (!opts) return fail(ctx, BLMM_ERR_INVALID, "opts is NULL");
  const bool alt = opts->method == BLMM_ALT_GRID;
  if (!Y || !G || (!h2_out && !alt)) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_loco: NULL buffer");
  if (m < 0 || ncov < 0) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  int rc = loco_check(ctx, n, p, chr_start, nchr, "bulkscan_loco");
  if (rc) return rc;
  if (n > 2048) return fail(ctx, BLMM_ERR_UNSUPPORTED, "more than 2048 individuals: the device eigensolver (tridiagonalisation + divide and conquer) stops at n = 2048");
  HostCall hc(ctx);
  const size_t h2_elems = alt ? (size_t)p * m : (size_t)m * nchr;
  HostCall::In d;
  if ((rc = hc.begin()) || (rc = ensure(ctx, ctx->outL, sizeof(double) * (size_t)p * m)) || (rc = ensure(ctx, ctx->outH2, sizeof(double) * h2_elems)) ||
      (rc = hc.inputs(Y, n, m, G, p, nullptr, Covar, ncov, weights, false, &d))) return rc;
  ctx->red_cur = RedArgs();
  if ((rc = bulkscan_loco_dev_impl(ctx, opts, d.Y, n, m, d.G, p, chr_start, nchr, kinship_digits, d.Cov, d.ncov, d.W, h2_grid, ngrid, nullptr,
                                   ptr<double>(ctx->outL), p, (alt && !h2_out) ? nullptr : ptr<double>(ctx->outH2), status, pvreq))) return rc;
  set_last(ctx, ptr<double>(ctx->outL), p, m);
  if (L_out && (size_t)p * m > 0 && (rc = copy_to_host(ctx, L_out, ctx->outL.p, sizeof(double) * (size_t)p * m))) return rc;
  if (h2_out && h2_elems > 0 && (rc = copy_to_host(ctx, h2_out, ctx->outH2.p, sizeof(double) * h2_elems))) return rc;
  if ((rc = hc.finish())) return rc;
  return check_sticky(ctx);
}

// ---------------------------------------------------------------------------------------------------
// Leave-one-chromosome-out without the LOD matrix (include/bulklmm_hip.h: blmm_bulkscan_loco_reduced).  `out`, dcmx, dcarg and dh2 are
// DEVICE pointers here.  Fused (null-grid; null-exact in the low-rank weights form): every chromosome reduces in its scan epilogues
// into its own slot range, flagged traits are re-scanned into it on the device (route 3), and one k_red_final_loco finishes all of
// them.  Otherwise every chromosome's rows go through one resident block of the largest chromosome's size (route 2).  Either way no
// p x m matrix exists.  Only a status makes it wait for the device.
static int loco_reduced_impl(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                             const int64_t* chr, int64_t nchr, int64_t kdigits, const double* dCovar, int64_t ncov, const double* dweights,
                             const double* h2_grid_host, int64_t ngrid, const double* dK_loco, const blmm_reduced* out, double* dcmx,
                             int64_t* dcarg, double* dh2, blmm_status* status) {
  int rc = check_opts(ctx, opts);
  if (rc) return rc;
  const bool alt = opts->method == BLMM_ALT_GRID;
  if (!out || !dY || !dG || (!dh2 && !alt)) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_loco_reduced: NULL buffer");
  if (out->cap < 0 || (out->cap > 0 && (!out->ti || !out->tj || !out->tlod)) || (out->want_triplets && !out->count))
    return fail(ctx, BLMM_ERR_INVALID, "bulkscan_loco_reduced: triplet buffers");
  if ((rc = check_method(ctx, opts)) || (rc = loco_check(ctx, n, p, chr, nchr, "bulkscan_loco_reduced"))) return rc;
  if (m < 0 || kdigits > 300) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_loco_reduced: bad arguments");
  if (n > 2048) return fail(ctx, BLMM_ERR_UNSUPPORTED, "more than 2048 individuals: the device eigensolver (tridiagonalisation + divide and conquer) stops at n = 2048");
  if (p > 0x7fffffffLL || m > 0x7fffffffLL) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  if ((rc = enter_device(ctx))) return rc;
  LocoRed red;
  red.out = out;
  red.fused = m > 0 && (opts->method == BLMM_NULL_GRID || wants_lowrank(ctx, opts, n, dCovar, ncov));
  if (red.fused) {
    red.slot0.resize((size_t)nchr + 1, 0);
    for (int64_t c = 0; c < nchr; ++c) red.slot0[(size_t)c + 1] = red.slot0[(size_t)c] + 2 * ((chr[c + 1] - chr[c] + 127) / 128);
    if ((rc = red_state(ctx, out, red.slot0.back(), m, &red.r)) || (rc = ensure(ctx, ctx->redflag, sizeof(int) * (size_t)m))) return rc;
    red.r.flags = ptr<int>(ctx->redflag);
    red.cmx = dcmx; red.carg = dcarg;
  } else {
    for (int64_t c = 0; c < nchr; ++c) red.ld = std::max(red.ld, chr[c + 1] - chr[c]);
    const size_t tab = (size_t)nchr * (size_t)(m > 0 ? m : 1);
    if ((rc = ensure(ctx, ctx->outL, sizeof(double) * (size_t)red.ld * (size_t)(m > 0 ? m : 1)))) return rc;
    if (!dcmx && (rc = ensure(ctx, ctx->locoCmx, sizeof(double) * tab))) return rc;
    if (!dcarg && (rc = ensure(ctx, ctx->locoCarg, sizeof(int64_t) * tab))) return rc;
    red.cmx = dcmx ? dcmx : ptr<double>(ctx->locoCmx);
    red.carg = dcarg ? dcarg : ptr<int64_t>(ctx->locoCarg);
    if (out->count) BLMM_HIP(hipMemsetAsync(out->count, 0, sizeof(int64_t), ctx->stream));
  }
  rc = loco_pipeline(ctx, opts, dY, n, m, dG, p, chr, nchr, kdigits, dCovar, ncov, dweights, h2_grid_host, ngrid, dK_loco, nullptr, 0,
                     alt ? nullptr : dh2, status, PvReq(), &red);
  ctx->red_cur = RedArgs();
  if (rc) return rc;
  clear_last(ctx);                          // no p x m matrix of this call: an earlier one is not served as its result
  // 1 / 3 need the device's counts: known when a status was read, else 0 (fused, not yet known)
  ctx->last_reduced_route = !red.fused ? 2 : !status ? 0 : (status->lowrank_fallback > 0 || status->n_illcond_rescan > 0) ? 3 : 1;
  return BLMM_OK;
}

int blmm_bulkscan_loco_reduced_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                                   const int64_t* chr_start, int64_t nchr, int64_t kinship_digits, const double* dCovar, int64_t ncov,
                                   const double* dweights, const double* h2_grid, int64_t ngrid, const double* dK_loco, const blmm_reduced* out,
                                   double* dchr_max_out, int64_t* dchr_argmax_out, double* dh2_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (pv_take(ctx).armed) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_loco_reduced: a blmm_set_log10p_output request is pending (the reduced call writes no matrix)");
  if (ncov == 0) dCovar = nullptr;
  return loco_reduced_impl(ctx, opts, dY, n, m, dG, p, chr_start, nchr, kinship_digits, dCovar, dCovar ? ncov : 0, dweights, h2_grid, ngrid,
                           dK_loco, out, dchr_max_out, dchr_argmax_out, dh2_out, status);
}

int blmm_bulkscan_loco_reduced(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                               const int64_t* chr_start, int64_t nchr, int64_t kinship_digits, const double* Covar, int64_t ncov,
                               const double* weights, const double* h2_grid, int64_t ngrid, const blmm_reduced* out, double* chr_max_out,
                               int64_t* chr_argmax_out, double* h2_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (pv_take(ctx).armed) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_loco_reduced: a blmm_set_log10p_output request is pending (the reduced call writes no matrix)");
  if (!opts) return fail(ctx, BLMM_ERR_INVALID, "opts is NULL");
  const bool alt = opts->method == BLMM_ALT_GRID;
  if (!out || !Y || !G || (!h2_out && !alt)) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_loco_reduced: NULL buffer");
  if (out->cap < 0 || (out->cap > 0 && (!out->ti || !out->tj || !out->tlod)) || (out->want_triplets && !out->count))
    return fail(ctx, BLMM_ERR_INVALID, "bulkscan_loco_reduced: triplet buffers");
  if (m < 0 || ncov < 0) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  int rc = loco_check(ctx, n, p, chr_start, nchr, "bulkscan_loco_reduced");
  if (rc) return rc;
  if (n > 2048) return fail(ctx, BLMM_ERR_UNSUPPORTED, "more than 2048 individuals: the device eigensolver (tridiagonalisation + divide and conquer) stops at n = 2048");
  // (loco_reduced_impl checks these again: here they come before the uploads)
  if ((rc = check_opts(ctx, opts)) || (rc = check_method(ctx, opts))) return rc;
  if (kinship_digits > 300) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_loco_reduced: bad arguments");
  if (p > 0x7fffffffLL || m > 0x7fffffffLL) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  if (opts->method != BLMM_NULL_EXACT && (rc = check_grid(ctx, h2_grid, ngrid))) return rc;
  HostCall hc(ctx);
  const size_t cap = out->cap > 0 ? out->cap : 1, mm = m > 0 ? m : 1, tab = (size_t)nchr * mm;
  // device side: maxima / arg-maxima (tmpA / tmpB), the per-chromosome tables (locoCmx / locoCarg), triplets + count (redtrip),
  // h2 (outH2, nchr x m)
  if ((rc = hc.begin()) || (rc = ensure(ctx, ctx->tmpA, sizeof(double) * mm)) || (rc = ensure(ctx, ctx->tmpB, sizeof(int64_t) * mm)) ||
      (rc = ensure(ctx, ctx->locoCmx, sizeof(double) * tab)) || (rc = ensure(ctx, ctx->locoCarg, sizeof(int64_t) * tab)) ||
      (rc = ensure(ctx, ctx->redtrip, (sizeof(double) + 2 * sizeof(int32_t)) * cap + 64)) || (rc = ensure(ctx, ctx->outH2, sizeof(double) * tab)))
    return rc;
  blmm_reduced d = *out;
  d.colmax = (out->colmax || out->argmax) ? ptr<double>(ctx->tmpA) : nullptr;
  d.argmax = out->argmax ? ptr<int64_t>(ctx->tmpB) : nullptr;
  d.count = ptr<int64_t>(ctx->redtrip);
  d.tlod = reinterpret_cast<double*>(d.count + 8);
  d.ti = reinterpret_cast<int32_t*>(d.tlod + cap);
  d.tj = d.ti + cap;
  HostCall::In in;
  // (the host form always reads the status: it waits for the device anyway, and that is what tells route 1 from route 3)
  blmm_status st;
  if ((rc = hc.inputs(Y, n, m, G, p, nullptr, Covar, ncov, weights, false, &in)) ||
      (rc = loco_reduced_impl(ctx, opts, in.Y, n, m, in.G, p, chr_start, nchr, kinship_digits, in.Cov, in.ncov, in.W, h2_grid, ngrid, nullptr, &d,
                              ptr<double>(ctx->locoCmx), ptr<int64_t>(ctx->locoCarg), alt ? nullptr : ptr<double>(ctx->outH2), &st))) return rc;
  if (status) *status = st;
  if (m > 0 && ((rc = hc.down(out->colmax, d.colmax, sizeof(double) * m)) || (rc = hc.down(out->argmax, d.argmax, sizeof(int64_t) * m)))) return rc;
  if (m > 0 && ((chr_max_out && (rc = copy_to_host(ctx, chr_max_out, ctx->locoCmx.p, sizeof(double) * (size_t)nchr * m))) ||
                (chr_argmax_out && (rc = copy_to_host(ctx, chr_argmax_out, ctx->locoCarg.p, sizeof(int64_t) * (size_t)nchr * m))) ||
                (!alt && h2_out && (rc = copy_to_host(ctx, h2_out, ctx->outH2.p, sizeof(double) * (size_t)nchr * m))))) return rc;
  if (out->want_triplets) {
    // the count first: only what it says is copied back
    if ((rc = hc.down(out->count, d.count, sizeof(int64_t)))) return rc;
    BLMM_HIP(hipStreamSynchronize(ctx->stream));
    const size_t got = *out->count < out->cap ? *out->count : out->cap;
    if ((rc = hc.down(out->tlod, d.tlod, sizeof(double) * got)) || (rc = hc.down(out->ti, d.ti, sizeof(int32_t) * got)) ||
        (rc = hc.down(out->tj, d.tj, sizeof(int32_t) * got))) return rc;
  }
  return (rc = hc.finish()) ? rc : check_sticky(ctx);
}

// host-pointer form of the reduce-in-epilogue scan: `out` holds HOST pointers; the small results come back, nothing p x m moves
int blmm_bulkscan_reduced(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                          const double* Covar, int64_t ncov, const double* K, const double* weights, const double* h2_grid,
                          int64_t ngrid, const blmm_reduced* out, double* h2_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  (void)pv_take(ctx);
  if (!opts) return fail(ctx, BLMM_ERR_INVALID, "opts is NULL");
  const bool alt = opts->method == BLMM_ALT_GRID;
  if (!out || !Y || !G || !K || (!h2_out && !alt)) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_reduced: NULL buffer");
  if (out->cap < 0 || (out->cap > 0 && (!out->ti || !out->tj || !out->tlod)) || (out->want_triplets && !out->count))
    return fail(ctx, BLMM_ERR_INVALID, "bulkscan_reduced: triplet buffers");
  if (n < 1 || m < 0 || p < 0) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  HostCall hc(ctx);
  int rc;
  const size_t cap = out->cap > 0 ? out->cap : 1, mm = m > 0 ? m : 1;
  // device side of `out`: maxima / arg-maxima (tmpA / tmpB), triplets + count (redtrip), h2 (outH2)
  if ((rc = hc.begin()) || (rc = ensure(ctx, ctx->tmpA, sizeof(double) * mm)) || (rc = ensure(ctx, ctx->tmpB, sizeof(int64_t) * mm)) ||
      (rc = ensure(ctx, ctx->redtrip, (sizeof(double) + 2 * sizeof(int32_t)) * cap + 64)) || (rc = ensure(ctx, ctx->outH2, sizeof(double) * mm)))
    return rc;
  blmm_reduced d = *out;
  d.colmax = (out->colmax || out->argmax) ? ptr<double>(ctx->tmpA) : nullptr;
  d.argmax = out->argmax ? ptr<int64_t>(ctx->tmpB) : nullptr;
  d.count = ptr<int64_t>(ctx->redtrip);
  d.tlod = reinterpret_cast<double*>(d.count + 8);
  d.ti = reinterpret_cast<int32_t*>(d.tlod + cap);
  d.tj = d.ti + cap;
  HostCall::In in;
  if ((rc = hc.inputs(Y, n, m, G, p, K, Covar, ncov, weights, /*defer*/ true, &in)) ||
      (rc = reduced_impl(ctx, opts, in.Y, n, m, in.G, p, in.Cov, in.ncov, in.K, in.W, h2_grid, ngrid, &d, ptr<double>(ctx->outH2), status,
                         &ctx->last_reduced_route))) return rc;
  if (m > 0 && ((rc = hc.down(out->colmax, d.colmax, sizeof(double) * m)) || (rc = hc.down(out->argmax, d.argmax, sizeof(int64_t) * m)) ||
                (rc = hc.down(alt ? nullptr : h2_out, ctx->outH2.p, sizeof(double) * m)))) return rc;
  if (out->want_triplets) {
    // the count first: only what it says is copied back
    if ((rc = hc.down(out->count, d.count, sizeof(int64_t)))) return rc;
    BLMM_HIP(hipStreamSynchronize(ctx->stream));
    const size_t got = *out->count < out->cap ? *out->count : out->cap;
    if ((rc = hc.down(out->tlod, d.tlod, sizeof(double) * got)) || (rc = hc.down(out->ti, d.ti, sizeof(int32_t) * got)) ||
        (rc = hc.down(out->tj, d.tj, sizeof(int32_t) * got))) return rc;
  }
  return (rc = hc.finish()) ? rc : check_sticky(ctx);
}

int blmm_last_reduced_route(const blmm_ctx* ctx) { return ctx ? ctx->last_reduced_route : 0; }

// Which parts of the shortened null-exact front the last call took: bit 0 the weight basis behind k_eigf_pairs, bit 1 the traits
// rotated inside k_brent, bit 3 the basis was rebuilt behind the Jacobi fallback (read from the device: the basis kernel reports
// it).  Waits for the stream.  < 0: an error code
int blmm_last_front_route(blmm_ctx* ctx) {
  if (!ctx) return BLMM_ERR_INVALID;
  int route = ctx->last_front_route;
  if ((route & FRONT_EARLY_WB) && ctx->wbRk.p) {
    int rk[4] = {0, 0, 0, 0};
    if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess ||
        hipMemcpy(rk, ctx->wbRk.p, sizeof(rk), hipMemcpyDeviceToHost) != hipSuccess) return BLMM_ERR_HIP;
    if (rk[3] == 1) route |= FRONT_WB_REBUILT;
  }
  return route;
}

// ---------------------------------------------------------------------------------------------------
// Stream-ordered reduced bulkscan (include/bulklmm_hip.h: blmm_bulkscan_reduced_async).  The fused route does not speculate: the
// per-trait guards write flags (RedArgs::flags), the reduced forms of k_scan_fix / k_scan_qr write the flagged traits' slot
// partials over the epilogue's before k_red_final and append their triplets, and the epilogue appends none for a flagged trait
// (when triplets are wanted the guards run ahead of the scan: lr_finish) -- so *count is exact with no second run and no host
// round trip.  Routes without a fused instantiation go through the resident L as reduced_impl's route 2 does.
static int reduced_async_impl(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                              const double* dCovar, int64_t ncov, const double* dK, const double* dweights, const double* h2_grid_host,
                              int64_t ngrid, const blmm_reduced* out, double* dh2_out, int64_t* dinfo) {
  int rc = reduced_check(ctx, opts, dY, n, m, dG, p, dK, out, dh2_out, "bulkscan_reduced_async");
  if (rc) return rc;
  // (grid_to_device checks the grid again; here: before anything is enqueued)
  if (opts->method != BLMM_NULL_EXACT && (rc = check_grid(ctx, h2_grid_host, ngrid))) return rc;
  if ((rc = enter_device(ctx))) return rc;
  // the side streams start behind everything already on the stream (a previous call's readers of the shared workspace)
  BLMM_HIP(hipEventRecord(ctx->ev_call, ctx->stream));
  BLMM_HIP(hipStreamWaitEvent(ctx->side, ctx->ev_call, 0));
  BLMM_HIP(hipStreamWaitEvent(ctx->side2, ctx->ev_call, 0));
  const bool fused = p > 0 && m > 0 && (opts->method == BLMM_NULL_GRID || wants_lowrank(ctx, opts, n, dCovar, ncov));
  if (fused) {
    RedArgs r;
    int nslot;
    if ((rc = reduced_args(ctx, out, p, m, &r, &nslot))) return rc;
    if ((rc = ensure(ctx, ctx->redflag, sizeof(int) * (size_t)m))) return rc;
    r.flags = ptr<int>(ctx->redflag);
    BLMM_HIP(hipMemsetAsync(r.flags, 0, sizeof(int) * (size_t)m, ctx->stream));
    ctx->red_cur = r;
    ctx->grid_async = true;
    rc = bulkscan_dev_impl(ctx, opts, dY, n, m, dG, p, dCovar, ncov, dK, dweights, h2_grid_host, ngrid, nullptr, p, dh2_out, nullptr, PvReq());
    ctx->red_cur = RedArgs();
    ctx->grid_async = false;
    if (rc) return rc;
    if ((rc = launch_red_final(ctx, r, nslot, m, out->colmax, out->argmax))) return rc;
    clear_last(ctx);                          // no matrix of this call: an earlier one is not served as its result
    return dinfo ? launch_red_info(ctx, ptr<int64_t>(ctx->stat), 0, out->want_triplets ? out->count : nullptr, dinfo) : BLMM_OK;
  }
  ctx->grid_async = true;
  rc = reduced_resident(ctx, opts, dY, n, m, dG, p, dCovar, ncov, dK, dweights, h2_grid_host, ngrid, out, dh2_out, nullptr);
  ctx->grid_async = false;
  if (rc) return rc;
  if (!dinfo) return BLMM_OK;
  if (!ctx->stat.p && (rc = ensure(ctx, ctx->stat, sizeof(int64_t) * NSTAT))) return rc;
  return launch_red_info(ctx, ptr<int64_t>(ctx->stat), 2, out->want_triplets ? out->count : nullptr, dinfo);
}

int blmm_bulkscan_reduced_async(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG,
                                int64_t p, const double* dCovar, int64_t ncov, const double* dK, const double* dweights,
                                const double* h2_grid_host, int64_t ngrid, const blmm_reduced* out, double* dh2_out,
                                int64_t* dinfo) {
  if (!ctx) return BLMM_ERR_INVALID;
  // a -log10 p request has nothing to attach to here (no matrix): refused, and consumed like every entry point's
  if (pv_take(ctx).armed) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_reduced_async: a blmm_set_log10p_output request is pending (the reduced call writes no matrix)");
  return reduced_async_impl(ctx, opts, dY, n, m, dG, p, dCovar, ncov, dK, dweights, h2_grid_host, ngrid, out, dh2_out, dinfo);
}

// ---------------------------------------------------------------------------------------------------
// dLperms_out (fp64) or dLperms32_out (fp32, kernels_scan_f32.hip): exactly one of them when nperms > 0
static int perms_pipeline(blmm_ctx* ctx, const blmm_opts* opts, Pipe& P, Timer& tm, int64_t nperms, uint64_t seed,
                          const int32_t* dperm_idx, double* dscalars_out, double* dlod_out, double* dLperms_out,
                          float* dLperms32_out, blmm_status* status, const double* dG_raw = nullptr);
// fp32 permutation path with its own fp32 rotation (kernels_scan_f32.hip: k_rotate_f32): intercept-only null model (the
// conditioning guard of more covariates re-scans from the fp64 rotated markers), tuning key "f32_rotation"
static bool f32_rotation_route(const blmm_ctx* ctx, const blmm_opts* o, const double* dCovar, int64_t ncov, int64_t nperms, int64_t p, bool f32) {
  return f32 && nperms > 0 && p > 0 && (int)null_cov(o, dCovar, ncov).c == 1 && ctx->tune.f32_rotation != 0;
}

static int scan_perms_impl(blmm_ctx* ctx, const blmm_opts* opts, const double* dy, int64_t n, const double* dG, int64_t p,
                           const double* dCovar, int64_t ncov, const double* dK, const double* dweights, int64_t nperms,
                           uint64_t seed, const int32_t* dperm_idx, double* dscalars_out, double* dlod_out,
                           double* dLperms_out, float* dLperms32_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  int rc = check_opts(ctx, opts);
  if (rc) return rc;
  if (nperms < 0) return fail(ctx, BLMM_ERR_NPERMS, "The required number of permutations must be a positive integer.");
  if (!dy || !dG || !dK || !dscalars_out || !dlod_out || (nperms > 0 && !dLperms_out && !dLperms32_out))
    return fail(ctx, BLMM_ERR_INVALID, "scan_perms: NULL buffer");
  if ((rc = enter_device(ctx))) return rc;
  Timer tm(ctx);
  Pipe P;
  // the library's own permutation indices depend on nothing in the call: generated on the side stream, beside the eigen-decomposition
  // (the multi-kernel panel form, n > 256, consumes them; ev_m orders them in front of the panels)
  ctx->perm_ready = false;
  bool perm_side = false;
  if (!dperm_idx && nperms > 0 && n > 256 && n <= 65535) {
    BLMM_HIP(hipEventRecord(ctx->ev_xt, ctx->stream));
    BLMM_HIP(hipStreamWaitEvent(ctx->side, ctx->ev_xt, 0));
    {
      OnStream on(ctx, ctx->side);
      if ((rc = launch_perm_gen(ctx, (int)n, nperms, seed))) return rc;
    }
    BLMM_HIP(hipEventRecord(ctx->ev_m, ctx->side));
    perm_side = true;
  }
  const bool own_rot = f32_rotation_route(ctx, opts, dCovar, ncov, nperms, p, dLperms32_out != nullptr);
  rc = prepare(ctx, opts, dy, n, 1, dG, p, dCovar, ncov, dK, dweights, 1, P, tm, false, false, /*skip_markers*/ own_rot);
  if (perm_side) BLMM_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_m, 0));      // (also on the error path: the side stream joins the call)
  if (rc) { ctx->perm_ready = false; return rc; }
  return perms_pipeline(ctx, opts, P, tm, nperms, seed, dperm_idx, dscalars_out, dlod_out, dLperms_out, dLperms32_out, status, own_rot ? dG : nullptr);
}

// Everything of the permutation test behind the rotations (shared with blmm_scan_perms_prerotated_dev)
static int perms_pipeline(blmm_ctx* ctx, const blmm_opts* opts, Pipe& P, Timer& tm, int64_t nperms, uint64_t seed,
                          const int32_t* dperm_idx, double* dscalars_out, double* dlod_out, double* dLperms_out,
                          float* dLperms32_out, blmm_status* status, const double* dG_raw) {
  int rc;
  const int64_t p = P.p;
  const NullModel nm = null_model(P, opts);
  // scalars: [sigma2_e, h2_null]
  if ((rc = launch_brent(ctx, nm, P.Yt, P.ldy, 1, P.Z0, P.lam, dscalars_out + 1, dscalars_out, nullptr, P.stat))) return rc;
  tm.mark();
  const int64_t ldp0 = 128, ldp1 = round_up(nperms > 0 ? nperms : 1, 128);
  if ((rc = ensure(ctx, ctx->panels, sizeof(double) * (size_t)P.npad * (ldp0 + ldp1)))) return rc;
  double* pan0 = ptr<double>(ctx->panels);
  double* pan1 = pan0 + (size_t)P.npad * ldp0;
  if ((rc = launch_perm_panel(ctx, nm, P.Yt, P.ldy, P.Z0, P.lam, dscalars_out + 1, nullptr, 0, seed, 1, pan0, ldp0, P.stat))) return rc;
  if (nperms > 0)
    if ((rc = launch_perm_panel(ctx, nm, P.Yt, P.ldy, P.Z0, P.lam, dscalars_out + 1, dperm_idx, nperms, seed, 0, pan1, ldp1, P.stat))) return rc;
  if ((rc = ensure(ctx, ctx->isx, sizeof(double) * (size_t)P.ldx))) return rc;
  if (dG_raw) {
    // ---- fp32 from the rotation on (round 4): XF = R G on the fp32 matrix cores straight into k_scan_f32's operand layout (no fp64
    //      rotated markers, no conversion pass), the marker norms from XF (fp64 sums), and the original trait's LOD vector with an
    //      fp64 numerator taken from G itself (g_i' R'a0) -- it agrees with the fp64 path to ~1e-7 relative (the norms carry the
    //      fp32 rounding of the rotated markers, averaged over n)
    const int64_t ldxf = round_up(p, 256), ldpf = ldp1;
    const int kpad = (int)round_up(P.npad, 128), ldrr = (int)round_up(P.n, 16);
    if ((rc = ensure(ctx, ctx->xf32, sizeof(float) * (size_t)P.npad * ldxf))) return rc;
    if ((rc = ensure(ctx, ctx->pf32, sizeof(float) * (size_t)P.npad * ldpf))) return rc;
    if ((rc = ensure(ctx, ctx->rf32, sizeof(float) * (size_t)kpad * ldrr + sizeof(double) * ((size_t)ldrr + (size_t)p) + 64))) return rc;
    float* RF = ptr<float>(ctx->rf32);
    double* vwork = reinterpret_cast<double*>(RF + (((size_t)kpad * ldrr + 3) & ~(size_t)3));
    double* numv = vwork + ldrr;
    if ((rc = launch_rotate_f32(ctx, ptr<double>(ctx->Rp), P.ldr, P.n, P.npad, dG_raw, p, RF, ptr<float>(ctx->xf32), ldxf, pan0, ldp0, vwork, numv))) return rc;
    if ((rc = launch_isx_f32(ctx, nm, ptr<float>(ctx->xf32), ldxf, p, P.Z0, P.lam, dscalars_out + 1, ptr<double>(ctx->isx), P.ldx, P.stat))) return rc;
    tm.mark();
    if ((rc = launch_lod_from_num(ctx, numv, ptr<double>(ctx->isx), P.n, p, dlod_out, P.stat))) return rc;
    if ((rc = launch_cvt_f32(ctx, pan1, ldp1, P.n, nperms, ptr<float>(ctx->pf32), ldpf, P.npad / 8))) return rc;
    if ((rc = launch_scan_f32(ctx, ptr<float>(ctx->xf32), ldxf, ptr<float>(ctx->pf32), ldpf, P.npad, P.n, p, nperms,
                              ptr<double>(ctx->isx), dLperms32_out, p, P.stat))) return rc;
    tm.mark();
    return end_call(ctx, P, status, &tm);
  }
  if ((rc = launch_isx(ctx, nm, P.Xt, P.ldx, p, P.Z0, P.lam, dscalars_out + 1, 1, ptr<double>(ctx->isx), P.ldx, P.stat))) return rc;
  tm.mark();
  if (p > 0) {
    ScanArgs a = scan_args(ctx, P, pan0, ldp0, dlod_out, p, 1);
    a.isx = ptr<double>(ctx->isx); a.ld_isx = P.ldx;
    if ((rc = launch_scan_table(ctx, a))) return rc;
    // the trait's own LOD vector (scan_null's result) gets the conditioning guard; the permutation matrix keeps the Cholesky form
    if ((rc = illcond_rescan(ctx, P, nm, 1, dscalars_out + 1, dlod_out, p))) return rc;
    if (nperms > 0 && dLperms32_out) {
      // fp32 path: fp32 fragment-major copies of the rotated markers and of the permutation panel, fp32 MFMA, fp32 L
      const int64_t ldxf = round_up(p, 256), ldpf = ldp1;
      if ((rc = ensure(ctx, ctx->xf32, sizeof(float) * (size_t)P.npad * ldxf))) return rc;
      if ((rc = ensure(ctx, ctx->pf32, sizeof(float) * (size_t)P.npad * ldpf))) return rc;
      if ((rc = launch_cvt_f32(ctx, P.Xt, P.ldx, P.n, p, ptr<float>(ctx->xf32), ldxf, P.npad / 8))) return rc;
      if ((rc = launch_cvt_f32(ctx, pan1, ldp1, P.n, nperms, ptr<float>(ctx->pf32), ldpf, P.npad / 8))) return rc;
      if ((rc = launch_scan_f32(ctx, ptr<float>(ctx->xf32), ldxf, ptr<float>(ctx->pf32), ldpf, P.npad, P.n, p, nperms,
                                ptr<double>(ctx->isx), dLperms32_out, p, P.stat))) return rc;
    } else if (nperms > 0) {
      ScanArgs b = scan_args(ctx, P, pan1, ldp1, dLperms_out, p, nperms);
      b.isx = ptr<double>(ctx->isx); b.ld_isx = P.ldx;
      if ((rc = launch_scan_table(ctx, b))) return rc;
    }
  }
  tm.mark();
  return end_call(ctx, P, status, &tm);
}

int blmm_scan_perms_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dy, int64_t n, const double* dG, int64_t p,
                        const double* dCovar, int64_t ncov, const double* dK, const double* dweights, int64_t nperms,
                        uint64_t seed, const int32_t* dperm_idx, double* dscalars_out, double* dlod_out,
                        double* dLperms_out, blmm_status* status) {
  if (ctx && nperms > 0 && !dLperms_out) return fail(ctx, BLMM_ERR_INVALID, "scan_perms: NULL buffer");
  return scan_perms_impl(ctx, opts, dy, n, dG, p, dCovar, ncov, dK, dweights, nperms, seed, dperm_idx, dscalars_out,
                         dlod_out, dLperms_out, nullptr, status);
}

int blmm_scan_perms_f32_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dy, int64_t n, const double* dG, int64_t p,
                            const double* dCovar, int64_t ncov, const double* dK, const double* dweights, int64_t nperms,
                            uint64_t seed, const int32_t* dperm_idx, double* dscalars_out, double* dlod_out,
                            float* dLperms_out, blmm_status* status) {
  if (ctx && nperms > 0 && !dLperms_out) return fail(ctx, BLMM_ERR_INVALID, "scan_perms: NULL buffer");
  return scan_perms_impl(ctx, opts, dy, n, dG, p, dCovar, ncov, dK, dweights, nperms, seed, dperm_idx, dscalars_out,
                         dlod_out, nullptr, dLperms_out, status);
}

// One process per GPU (include/bulklmm_hip.h: the pipeline in three calls): the permutation test on marker blocks rotated by the
// ranks and gathered by the host -- this rank's permutations (nperms, seed / dperm_idx) against all p markers.  Exactly one of
// dLperms_out (fp64) / dLperms32_out (fp32 matrix cores) is given.  Bit-identical to blmm_scan_perms[_f32]_dev.
int blmm_scan_perms_prerotated_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dy, int64_t p, const double* dXt_blocks,
                                   int64_t nblocks, int64_t block_cols, int64_t block_ld, int64_t nperms, uint64_t seed,
                                   const int32_t* dperm_idx, double* dscalars_out, double* dlod_out, double* dLperms_out,
                                   float* dLperms32_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  int rc = check_opts(ctx, opts);
  if (rc) return rc;
  if (!ctx->prep_valid) return fail(ctx, BLMM_ERR_INVALID, "scan_perms_prerotated: blmm_prepare_dev has not run on this context");
  if (nperms < 0) return fail(ctx, BLMM_ERR_NPERMS, "The required number of permutations must be a positive integer.");
  if (!dy || !dXt_blocks || !dscalars_out || !dlod_out || (nperms > 0 && !dLperms_out == !dLperms32_out))
    return fail(ctx, BLMM_ERR_INVALID, "scan_perms_prerotated: NULL buffer (exactly one of the fp64 / fp32 permutation matrices)");
  if (p < 0 || nblocks < 1 || block_cols < 1 || block_ld < block_cols || nblocks * block_cols < p) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  if ((rc = enter_device(ctx))) return rc;
  Timer tm(ctx);
  Pipe P = prepared_pipe(ctx);
  if ((rc = reset_prepared(ctx, P, tm))) return rc;
  ctx->perm_ready = false;
  if ((rc = rotate_traits(ctx, P, dy, 1))) return rc;
  if ((rc = assemble_prerotated(ctx, P, p, dXt_blocks, nblocks, block_cols, block_ld))) return rc;
  tm.mark();
  return perms_pipeline(ctx, opts, P, tm, nperms, seed, dperm_idx, dscalars_out, dlod_out, dLperms_out, dLperms32_out, status);
}

// caller-supplied permutation indices (n x nperms) -> tmpC; nullptr: the library draws its own
static int up_perm_idx(HostCall& hc, const int32_t* perm_idx, int64_t n, int64_t nperms, const int32_t** dperm) {
  *dperm = nullptr;
  if (!perm_idx || nperms <= 0) return BLMM_OK;
  int rc = hc.up(hc.ctx->tmpC, perm_idx, sizeof(int32_t) * (size_t)n * nperms);
  if (!rc) *dperm = ptr<int32_t>(hc.ctx->tmpC);
  return rc;
}

static int scan_perms_host(blmm_ctx* ctx, const blmm_opts* opts, const double* y, int64_t n, const double* G, int64_t p,
                           const double* Covar, int64_t ncov, const double* K, const double* weights, int64_t nperms,
                           uint64_t seed, const int32_t* perm_idx, double* scalars_out, double* lod_out, void* Lperms_out,
                           bool f32, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (!opts) return fail(ctx, BLMM_ERR_INVALID, "opts is NULL");
  if (nperms < 0) return fail(ctx, BLMM_ERR_NPERMS, "The required number of permutations must be a positive integer.");
  if (!y || !G || !K || !scalars_out || !lod_out || (nperms > 0 && !Lperms_out)) return fail(ctx, BLMM_ERR_INVALID, "scan_perms: NULL buffer");
  if (n < 1 || p < 0) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  HostCall hc(ctx);
  const size_t esz = f32 ? sizeof(float) : sizeof(double);
  int rc;
  if ((rc = hc.begin()) || (rc = ensure(ctx, ctx->outL, sizeof(double) * (size_t)p + esz * (size_t)p * nperms)) ||
      (rc = ensure(ctx, ctx->outH2, sizeof(double) * 2))) return rc;
  HostCall::In d;
  const int32_t* dperm;
  if ((rc = hc.inputs(y, n, 1, G, p, K, Covar, ncov, weights, false, &d)) || (rc = up_perm_idx(hc, perm_idx, n, nperms, &dperm))) return rc;
  double* dL = ptr<double>(ctx->outL);
  void* dLp = dL + p;                       // 8-byte aligned; the fp32 kernel needs 4
  if ((rc = scan_perms_impl(ctx, opts, d.Y, n, d.G, p, d.Cov, d.ncov, d.K, d.W, nperms, seed, dperm, ptr<double>(ctx->outH2), dL,
                            f32 ? nullptr : reinterpret_cast<double*>(dLp), f32 ? reinterpret_cast<float*>(dLp) : nullptr, status))) return rc;
  set_last(ctx, reinterpret_cast<const double*>(dLp), p, nperms, f32);
  if ((rc = hc.down(scalars_out, ctx->outH2.p, sizeof(double) * 2)) || (rc = hc.down(lod_out, dL, sizeof(double) * p))) return rc;
  if (p > 0 && nperms > 0 && (rc = copy_to_host(ctx, Lperms_out, dLp, esz * (size_t)p * nperms))) return rc;
  return (rc = hc.finish()) ? rc : check_sticky(ctx);
}

int blmm_scan_perms(blmm_ctx* ctx, const blmm_opts* opts, const double* y, int64_t n, const double* G, int64_t p,
                    const double* Covar, int64_t ncov, const double* K, const double* weights, int64_t nperms, uint64_t seed,
                    const int32_t* perm_idx, double* scalars_out, double* lod_out, double* Lperms_out, blmm_status* status) {
  return scan_perms_host(ctx, opts, y, n, G, p, Covar, ncov, K, weights, nperms, seed, perm_idx, scalars_out, lod_out,
                         Lperms_out, false, status);
}

int blmm_scan_perms_f32(blmm_ctx* ctx, const blmm_opts* opts, const double* y, int64_t n, const double* G, int64_t p,
                        const double* Covar, int64_t ncov, const double* K, const double* weights, int64_t nperms, uint64_t seed,
                        const int32_t* perm_idx, double* scalars_out, double* lod_out, float* Lperms_out, blmm_status* status) {
  return scan_perms_host(ctx, opts, y, n, G, p, Covar, ncov, K, weights, nperms, seed, perm_idx, scalars_out, lod_out,
                         Lperms_out, true, status);
}

// ---------------------------------------------------------------------------------------------------
// The permutation test of every trait (include/bulklmm_hip.h: blmm_bulkscan_perms): the bulk null fit, then trait chunks of
// panel columns (kernels_bperm.hip) through the table kernel's reduce-in-epilogue instantiation -- its slot partials and
// k_red_final give every column's maximum exactly as k_colmax on the stored column would -- and the per-trait summary.
// blmm_bulkscan_multidf_perms is the same call with k > 0: loci of k adjacent columns, scanned by the k-df table / reducing scan
// kernels (kernels_mdf.hip) on the uncentred marker rotation; k = 0 is the 1-df form everywhere below.
struct BpermOut {
  double *h2, *sigma2, *lod_max; int64_t* lod_argmax; double *max_perms, *thr, *pval;
};
static int bperm_check(blmm_ctx* ctx, const blmm_opts* opts, int64_t n, int64_t m, int64_t p, const double* Covar, int64_t ncov,
                       int64_t nperms, const double* probs, int64_t nprobs, bool have_in, const BpermOut& o,
                       const char* who = "bulkscan_perms") {
  const std::string w(who);
  int rc = check_opts(ctx, opts);
  if (rc) return rc;
  if (nperms < 0) return fail(ctx, BLMM_ERR_NPERMS, "The required number of permutations must be a positive integer.");
  if (!have_in || !o.h2 || !o.sigma2 || !o.lod_max || !o.lod_argmax) return fail(ctx, BLMM_ERR_INVALID, w + ": NULL buffer");
  if (nprobs < 0 || nprobs > 64 || (nprobs > 0 && !probs)) return fail(ctx, BLMM_ERR_INVALID, w + ": 0 .. 64 threshold levels");
  if (n < 1 || m < 0 || p < 0 || ncov < 0 || m > 0x7fffffffLL || p > 0x7fffffffLL) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  if (nperms > BPERM_MAX_NPERMS)
    return fail(ctx, BLMM_ERR_UNSUPPORTED, w + ": more than 16384 permutations (the per-trait sort runs in LDS)");
  if (null_cov(opts, Covar, ncov).c > CTPL)
    return fail(ctx, BLMM_ERR_UNSUPPORTED, w + ": more than 8 null covariates (incl. intercept) are not supported");
  return BLMM_OK;
}
// ... of blmm_bulkscan_multidf_perms: bperm_check's, then blmm_bulkscan_multidf's on k and p (null-grid's limit on k: the scan is
// the null-grid algebra) and on n
static_assert(CTPL == BLMM_MULTIDF_MAX_COVARIATES, "bperm_check's covariate limit is the k-df kernels'");
static int mdf_perms_check(blmm_ctx* ctx, const blmm_opts* opts, int64_t n, int64_t m, int64_t p, int64_t k, const double* Covar,
                           int64_t ncov, int64_t nperms, const double* probs, int64_t nprobs, bool have_in, const BpermOut& o) {
  int rc = bperm_check(ctx, opts, n, m, p, Covar, ncov, nperms, probs, nprobs, have_in, o, "bulkscan_multidf_perms");
  if (rc) return rc;
  if (k < 1 || p % k != 0) return fail(ctx, BLMM_ERR_DIM, "bulkscan_multidf_perms: the number of columns of G must be a multiple of k >= 1");
  if (k > BLMM_MULTIDF_MAX_K_GRID) return fail(ctx, BLMM_ERR_UNSUPPORTED, "bulkscan_multidf_perms: takes 1 <= k <= 8");
  if (n > 2048) return fail(ctx, BLMM_ERR_UNSUPPORTED, "more than 2048 individuals: the device eigensolver (tridiagonalisation + divide and conquer) stops at n = 2048");
  return BLMM_OK;
}

// Slots of the reduction partials: two per 128 markers (the table kernel's tiles), or one per 64 loci of k columns (k_mdf_grid_red)
static int bperm_nslot(int64_t p, int64_t k) { return k > 0 ? (int)((p / k + 63) / 64) : 2 * (int)((p + 127) / 128); }

// Traits per chunk: per panel column its k-major panel (npad doubles), its reduction partials (nslot x 12 bytes), bin, maximum and
// marker; per trait its row of marker norms (k > 0: its k (k + 1) / 2 factor entries per locus), r0 and the panel coefficients.
// Default budget 4 GiB of workspace.  At most 65535 traits (a grid extent of launch_isx / launch_mdf_table / the summary) and, k > 0,
// MDF_RED_MAX_COLS panel columns.
static int64_t bperm_chunk_traits(const blmm_ctx* ctx, int64_t npad, int64_t ldx, int64_t n, int64_t p, int64_t nperms, int64_t k = 0) {
  const int64_t np1 = nperms + 1;
  const int nslot = bperm_nslot(p, k);
  const double col_bytes = 8.0 * npad + 12.0 * nslot + 20.0 + 8.0 * (CMAX + 1);
  const double table_bytes = k > 0 ? 8.0 * (double)(k * (k + 1) / 2) * (double)(p / k) : 8.0 * (double)ldx;
  const double trait_bytes = np1 * col_bytes + table_bytes + 8.0 * n;
  int64_t mt_max = ctx->tune.bulk_perm_cols > 0 ? ctx->tune.bulk_perm_cols / np1 : (int64_t)((double)(4ll << 30) / trait_bytes);
  if (k > 0) mt_max = std::min<int64_t>(mt_max, MDF_RED_MAX_COLS / np1);
  return std::max<int64_t>(1, std::min<int64_t>(mt_max, 65535));
}

// The genome-wide buffer of blmm_bulkscan_loco_perms: (nperms + 1) x m column maxima and their global markers
struct BpermMerge { double* gmx = nullptr; int64_t* garg = nullptr; };

// Chunks of whole traits of one rotation (P: the p markers and the m rotated traits; nm its null model; o.h2 the traits' h2): the
// isx / panel / reduce-in-epilogue scan / k_red_final chain, then the per-trait summary into o (markers + row0).  mg (LOCO): every
// chunk's column maxima also fold into the genome-wide buffer.  k > 0: P.Xt is the uncentred rotation, the table is k_mdf_table's
// factors at the chunk's own h2 values (its "grid"; bin[column] = trait, as for launch_isx), the scan k_mdf_grid_red, and every
// index a locus.
static int bperm_chunks(blmm_ctx* ctx, const Pipe& P, const NullModel& nm, int64_t m, int64_t p, const int32_t* perm, int64_t nperms,
                        int64_t mt_max, const BpermProbs& pr, int64_t nprobs, const BpermOut& o, int64_t row0, const BpermMerge* mg,
                        int64_t k = 0) {
  int rc;
  const int64_t np1 = nperms + 1;
  const int nslot = bperm_nslot(p, k);
  const int64_t nloci = k > 0 ? p / k : p, ntab = k * (k + 1) / 2;
  const bool summary = o.lod_max || o.lod_argmax || o.max_perms || o.thr || o.pval;
  for (int64_t j0 = 0; j0 < m; j0 += mt_max) {
    const int64_t mt = std::min(mt_max, m - j0), ncols = mt * np1, ldp = round_up(ncols, 128), ldm = round_up(ncols, 64);
    if ((rc = ensure(ctx, ctx->panels, sizeof(double) * (size_t)P.npad * ldp)) ||
        (rc = k > 0 ? ensure(ctx, ctx->mdfT, sizeof(double) * (size_t)ntab * (size_t)nloci * mt)
                    : ensure(ctx, ctx->isx, sizeof(double) * (size_t)P.ldx * mt)) ||
        (rc = ensure(ctx, ctx->redbuf, (sizeof(double) + sizeof(int)) * (size_t)nslot * (size_t)ldm)) ||
        (rc = ensure(ctx, ctx->bperm, (sizeof(double) + sizeof(int64_t) + sizeof(int)) * (size_t)ldp))) return rc;
    double* mx = ptr<double>(ctx->bperm);
    int64_t* arg = reinterpret_cast<int64_t*>(mx + ldp);
    int* bin = reinterpret_cast<int*>(arg + ldp);
    const double* h2c = o.h2 + j0;
    if (p > 0 && (rc = k > 0 ? launch_mdf_table(ctx, nm, P.Xt, P.ldx, nloci, (int)k, P.Z0, P.lam, h2c, (int)mt, ptr<double>(ctx->mdfT))
                             : launch_isx(ctx, nm, P.Xt, P.ldx, p, P.Z0, P.lam, h2c, (int)mt, ptr<double>(ctx->isx), P.ldx, P.stat))) return rc;
    if ((rc = launch_bperm_panels(ctx, nm, P.Yt + j0, P.ldy, P.Z0, P.lam, h2c, mt, perm, nperms, ptr<double>(ctx->panels), ldp, bin, P.stat))) return rc;
    if (p > 0) {
      RedArgs r;
      r.pmax = ptr<double>(ctx->redbuf); r.parg = reinterpret_cast<int*>(r.pmax + (size_t)nslot * ldm); r.ldm = ldm;
      if (k > 0) {
        MdfArgs a;
        a.Xt = P.Xt; a.ldx = P.ldx; a.nloci = nloci; a.k = (int)k; a.n = P.n; a.m = ncols;
        a.P = ptr<double>(ctx->panels); a.ldp = ldp; a.pstride = 0; a.c = P.c;
        a.T = ptr<double>(ctx->mdfT); a.bin = bin; a.L = nullptr; a.ldL = 0; a.stat = P.stat;
        rc = launch_mdf_scan_red(ctx, a, r);
      } else {
        ScanArgs a = scan_args(ctx, P, ptr<double>(ctx->panels), ldp, nullptr, 0, ncols);
        a.isx = ptr<double>(ctx->isx); a.ld_isx = P.ldx; a.bin = bin;
        a.Pv = nullptr; a.red = r;
        rc = launch_scan_table(ctx, a);
      }
      if (rc || (rc = launch_red_final(ctx, r, nslot, ncols, mx, arg))) return rc;
    } else {                                    // no markers: every column's maximum is -inf at marker -1 (k_colmax's empty column)
      if ((rc = fill(ctx, mx, ncols, -INFINITY))) return rc;
      BLMM_HIP(hipMemsetAsync(arg, 0xff, sizeof(int64_t) * (size_t)ncols, ctx->stream));
    }
    if (summary && (rc = launch_bperm_summary(ctx, mx, arg, mt, nperms, pr, (int)nprobs, j0, o.lod_max, o.lod_argmax, o.max_perms, o.thr,
                                              o.pval, row0))) return rc;
    if (mg && (rc = launch_bperm_loco_merge(ctx, mx, arg, ncols, row0, mg->gmx + (size_t)j0 * np1, mg->garg + (size_t)j0 * np1))) return rc;
  }
  return BLMM_OK;
}

static int bulk_perms_impl(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                           int64_t k, const double* dCovar, int64_t ncov, const double* dK, const double* dweights, int64_t nperms,
                           uint64_t seed, const int32_t* dperm_idx, const double* probs, int64_t nprobs, const BpermOut& o,
                           blmm_status* status) {
  int rc = k > 0 ? mdf_perms_check(ctx, opts, n, m, p, k, dCovar, ncov, nperms, probs, nprobs, dY && dG && dK, o)
                 : bperm_check(ctx, opts, n, m, p, dCovar, ncov, nperms, probs, nprobs, dY && dG && dK, o);
  if (rc || (rc = enter_device(ctx))) return rc;
  BpermProbs pr;
  for (int t = 0; t < 64; ++t) pr.v[t] = t < nprobs ? probs[t] : 0.0;
  Timer tm(ctx);
  Pipe P;
  ctx->perm_ready = false;
  clear_last(ctx);                              // no matrix of this call (and the workspace it sat in is reused)
  // the traits are rotated as scan rotates its one (launch_rotate picks its kernel by the column count as well as by n)
  // (k > 0: the markers are left to the uncentred rotation below, as blmm_bulkscan_multidf rotates them)
  if ((rc = prepare(ctx, opts, dY, n, 0, dG, p, dCovar, ncov, dK, dweights, 1, P, tm, false, false, /*skip_markers*/ k > 0))) return rc;
  P.m = m; P.ldy = round_up(m > 0 ? m : 1, 128);
  if ((rc = ensure(ctx, ctx->Yt, sizeof(double) * (size_t)P.npad * P.ldy))) return rc;
  P.Yt = ptr<double>(ctx->Yt);
  if ((rc = launch_rotate_single(ctx, ptr<double>(ctx->Rp), P.ldr, P.n, P.npad, dY, m, P.Yt, P.ldy))) return rc;
  const NullModel nm = null_model(P, opts);
  if (m > 0 && (rc = launch_brent(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, o.h2, o.sigma2, nullptr, P.stat))) return rc;
  if (k > 0 && p > 0 && m > 0) {
    if ((rc = ensure(ctx, ctx->mdfR, sizeof(double) * (size_t)P.npad * P.ldr)) ||
        (rc = ensure(ctx, ctx->Xt, sizeof(double) * (size_t)P.npad * P.ldx))) return rc;
    if ((rc = launch_mdf_rawrot(ctx, ptr<double>(ctx->U), dweights, P.n, P.npad, P.ldr, ptr<double>(ctx->mdfR)))) return rc;
    P.Xt = ptr<double>(ctx->Xt);
    if ((rc = launch_rotate(ctx, ptr<double>(ctx->mdfR), P.ldr, P.n, P.npad, dG, p, P.Xt, P.ldx, P.ldx))) return rc;
  }
  tm.mark();
  const int32_t* perm = dperm_idx;
  if (m > 0 && nperms > 0 && !perm) {
    if ((rc = launch_perm_gen(ctx, (int)n, nperms, seed))) return rc;
    ctx->perm_ready = false;                    // consumed here, not by a later launch_perm_panel
    perm = ptr<int32_t>(ctx->perm);
  }
  const int64_t mt_max = bperm_chunk_traits(ctx, P.npad, P.ldx, n, p, nperms, k);
  if ((rc = bperm_chunks(ctx, P, nm, m, p, perm, nperms, mt_max, pr, nprobs, o, 0, nullptr, k))) return rc;
  tm.mark();
  return end_call(ctx, P, status, &tm);
}

int blmm_bulkscan_perms_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                            const double* dCovar, int64_t ncov, const double* dK, const double* dweights, int64_t nperms,
                            uint64_t seed, const int32_t* dperm_idx, const double* probs, int64_t nprobs, double* dh2_out,
                            double* dsigma2_out, double* dlod_max_out, int64_t* dlod_argmax_out, double* dmax_perms_out,
                            double* dthr_out, double* dpval_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  const BpermOut o{dh2_out, dsigma2_out, dlod_max_out, dlod_argmax_out, dmax_perms_out, dthr_out, dpval_out};
  return bulk_perms_impl(ctx, opts, dY, n, m, dG, p, 0, dCovar, ncov, dK, dweights, nperms, seed, dperm_idx, probs, nprobs, o, status);
}

// The host forms of blmm_bulkscan_perms (k = 0) and blmm_bulkscan_multidf_perms (k: the call's own argument, checked here)
static int bulk_perms_host(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                           int64_t k, bool mdf, const double* Covar, int64_t ncov, const double* K, const double* weights, int64_t nperms,
                           uint64_t seed, const int32_t* perm_idx, const double* probs, int64_t nprobs, double* h2_out,
                           double* sigma2_out, double* lod_max_out, int64_t* lod_argmax_out, double* max_perms_out, double* thr_out,
                           double* pval_out, blmm_status* status) {
  const BpermOut ho{h2_out, sigma2_out, lod_max_out, lod_argmax_out, max_perms_out, thr_out, pval_out};
  int rc = mdf ? mdf_perms_check(ctx, opts, n, m, p, k, Covar, ncov, nperms, probs, nprobs, Y && G && K, ho)
               : bperm_check(ctx, opts, n, m, p, Covar, ncov, nperms, probs, nprobs, Y && G && K, ho);
  if (rc) return rc;
  // caller-supplied permutations are indices into the trait's n entries: checked here, before a kernel reads through them
  if (perm_idx && nperms > 0)
    for (int64_t e = 0; e < n * nperms; ++e)
      if (perm_idx[e] < 0 || perm_idx[e] >= n)
        return fail(ctx, BLMM_ERR_INVALID, std::string(mdf ? "bulkscan_multidf_perms" : "bulkscan_perms") + ": perm_idx entries must lie in 0 .. n - 1");
  HostCall hc(ctx);
  // device outputs in outL: h2, sigma2, lod_max, lod_argmax (m each), pval (m), thresholds (nprobs x m), max_perms (nperms x m)
  const size_t mm = (size_t)m;
  if ((rc = hc.begin()) || (rc = ensure(ctx, ctx->outL, sizeof(double) * (mm * (5 + (size_t)nprobs + (size_t)nperms) + 1)))) return rc;
  double* d = ptr<double>(ctx->outL);
  const BpermOut o{d, d + mm, d + 2 * mm, reinterpret_cast<int64_t*>(d + 3 * mm), max_perms_out ? d + (5 + nprobs) * mm : nullptr,
                   thr_out ? d + 5 * mm : nullptr, pval_out ? d + 4 * mm : nullptr};
  HostCall::In in;
  const int32_t* dperm;
  if ((rc = hc.inputs(Y, n, m, G, p, K, Covar, ncov, weights, false, &in)) || (rc = up_perm_idx(hc, perm_idx, n, nperms, &dperm)) ||
      (rc = bulk_perms_impl(ctx, opts, in.Y, n, m, in.G, p, k, in.Cov, in.ncov, in.K, in.W, nperms, seed, dperm, probs, nprobs, o, status))) return rc;
  if ((rc = hc.down(h2_out, o.h2, sizeof(double) * mm)) || (rc = hc.down(sigma2_out, o.sigma2, sizeof(double) * mm)) ||
      (rc = hc.down(lod_max_out, o.lod_max, sizeof(double) * mm)) || (rc = hc.down(lod_argmax_out, o.lod_argmax, sizeof(int64_t) * mm)) ||
      (rc = hc.down(pval_out, o.pval, sizeof(double) * mm)) || (rc = hc.down(thr_out, o.thr, sizeof(double) * mm * nprobs))) return rc;
  if (max_perms_out && (rc = copy_to_host(ctx, max_perms_out, o.max_perms, sizeof(double) * mm * nperms))) return rc;
  return (rc = hc.finish()) ? rc : check_sticky(ctx);
}

int blmm_bulkscan_perms(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                        const double* Covar, int64_t ncov, const double* K, const double* weights, int64_t nperms, uint64_t seed,
                        const int32_t* perm_idx, const double* probs, int64_t nprobs, double* h2_out, double* sigma2_out,
                        double* lod_max_out, int64_t* lod_argmax_out, double* max_perms_out, double* thr_out, double* pval_out,
                        blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  return bulk_perms_host(ctx, opts, Y, n, m, G, p, 0, false, Covar, ncov, K, weights, nperms, seed, perm_idx, probs, nprobs, h2_out,
                         sigma2_out, lod_max_out, lod_argmax_out, max_perms_out, thr_out, pval_out, status);
}

// The k-df permutation test (include/bulklmm_hip.h: blmm_bulkscan_multidf_perms).  A pending -log10 p request does not apply to this
// call: disarmed, as by every entry point that writes no matrix.
int blmm_bulkscan_multidf_perms_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG,
                                    int64_t p, int64_t k, const double* dCovar, int64_t ncov, const double* dK, const double* dweights,
                                    int64_t nperms, uint64_t seed, const int32_t* dperm_idx, const double* probs, int64_t nprobs,
                                    double* dh2_out, double* dsigma2_out, double* dlod_max_out, int64_t* dlod_argmax_out,
                                    double* dmax_perms_out, double* dthr_out, double* dpval_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  (void)pv_take(ctx);
  const BpermOut o{dh2_out, dsigma2_out, dlod_max_out, dlod_argmax_out, dmax_perms_out, dthr_out, dpval_out};
  // (checked here as in the host form: k < 1 must be refused, not read as the 1-df form)
  if (int rc = mdf_perms_check(ctx, opts, n, m, p, k, dCovar, ncov, nperms, probs, nprobs, dY && dG && dK, o)) return rc;
  return bulk_perms_impl(ctx, opts, dY, n, m, dG, p, k, dCovar, ncov, dK, dweights, nperms, seed, dperm_idx, probs, nprobs, o, status);
}

int blmm_bulkscan_multidf_perms(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                                int64_t k, const double* Covar, int64_t ncov, const double* K, const double* weights, int64_t nperms,
                                uint64_t seed, const int32_t* perm_idx, const double* probs, int64_t nprobs, double* h2_out,
                                double* sigma2_out, double* lod_max_out, int64_t* lod_argmax_out, double* max_perms_out, double* thr_out,
                                double* pval_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  (void)pv_take(ctx);
  return bulk_perms_host(ctx, opts, Y, n, m, G, p, k, true, Covar, ncov, K, weights, nperms, seed, perm_idx, probs, nprobs, h2_out,
                         sigma2_out, lod_max_out, lod_argmax_out, max_perms_out, thr_out, pval_out, status);
}

// ---------------------------------------------------------------------------------------------------
// The LOCO permutation test (include/bulklmm_hip.h: blmm_bulkscan_loco_perms): blmm_bulkscan_perms on every chromosome's column block
// under its LOCO kinship, with one permutation set for all of them, and the genome-wide tables from the chromosomes' column maxima
// paired by permutation index.  g: the genome-wide outputs (g.h2 / g.sigma2: nchr x m); chr_*: the per-chromosome tables, each
// optional, block c at + c (m, nprobs m, nperms m).
struct LocoPermOut {
  BpermOut g;
  double* chr_lod_max; int64_t* chr_lod_argmax; double *chr_max_perms, *chr_thr, *chr_pval;
};

// every refusal of the call that needs no device: bperm_check's, loco_check's, n > 2048
static int loco_perms_check(blmm_ctx* ctx, const blmm_opts* opts, int64_t n, int64_t m, int64_t p, const int64_t* chr, int64_t nchr,
                            int64_t kdigits, const double* Covar, int64_t ncov, int64_t nperms, const double* probs, int64_t nprobs,
                            bool have_in, const LocoPermOut& o) {
  int rc = bperm_check(ctx, opts, n, m, p, Covar, ncov, nperms, probs, nprobs, have_in, o.g, "bulkscan_loco_perms");
  if (rc || (rc = loco_check(ctx, n, p, chr, nchr, "bulkscan_loco_perms"))) return rc;
  if (kdigits > 300) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_loco_perms: bad arguments");
  if (n > 2048) return fail(ctx, BLMM_ERR_UNSUPPORTED, "more than 2048 individuals: the device eigensolver (tridiagonalisation + divide and conquer) stops at n = 2048");
  return BLMM_OK;
}

// The kinships (unless given) and the batched eigen phase as blmm_bulkscan_loco; the permutation set once; then per chromosome,
// largest first, bulk_perms_impl's front (prepare on its column block, launch_rotate_single, launch_brent) and trait chunks, whose
// column maxima also fold into the genome-wide buffer (locoPerm); one summary of that buffer after the last chromosome.
static int loco_perms_impl(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                           const int64_t* chr, int64_t nchr, int64_t kdigits, const double* dCovar, int64_t ncov, const double* dweights,
                           const double* dK_loco, int64_t nperms, uint64_t seed, const int32_t* dperm_idx, const double* probs,
                           int64_t nprobs, const LocoPermOut& o, blmm_status* status) {
  int rc = loco_perms_check(ctx, opts, n, m, p, chr, nchr, kdigits, dCovar, ncov, nperms, probs, nprobs, dY && dG, o);
  if (rc || (rc = enter_device(ctx))) return rc;
  BpermProbs pr;
  for (int t = 0; t < 64; ++t) pr.v[t] = t < nprobs ? probs[t] : 0.0;
  if (ctx->ev_used + (size_t)nchr + 2 >= 4096) ctx->ev_used = 0;
  ctx->evsets.reserve(ctx->ev_used + (size_t)nchr + 2);
  Timer t0(ctx);
  t0.mark();
  ctx->perm_ready = false;
  clear_last(ctx);                              // no matrix of this call (and the workspace it sat in is reused)
  const double* dK = dK_loco;
  if (!dK) {
    if ((rc = ensure(ctx, ctx->locoK, sizeof(double) * (size_t)n * n * nchr)) ||
        (rc = kinship_loco_impl(ctx, dG, n, chr, nchr, kdigits, ptr<double>(ctx->locoK)))) return rc;
    dK = ptr<double>(ctx->locoK);
  }
  if ((rc = ensure(ctx, ctx->locoStat, sizeof(int64_t) * NSTAT * (size_t)nchr))) return rc;
  int64_t* dst_all = ptr<int64_t>(ctx->locoStat);
  const std::vector<int64_t> order = loco_order(chr, nchr);
  Timer tb(ctx);
  bool batched = false;
  if ((rc = loco_eigen_batch(ctx, opts, n, dK, nchr, dCovar, ncov, dweights, dst_all, tb, &batched))) return rc;
  // the genome-wide column maxima, -inf / -1 until the first chromosome folds in
  const int64_t np1 = nperms + 1, gcols = np1 * m;
  BpermMerge mg;
  if (m > 0) {
    if ((rc = ensure(ctx, ctx->locoPerm, (sizeof(double) + sizeof(int64_t)) * (size_t)gcols))) return rc;
    mg.gmx = ptr<double>(ctx->locoPerm);
    mg.garg = reinterpret_cast<int64_t*>(mg.gmx + gcols);
    if ((rc = launch_bperm_loco_init(ctx, gcols, mg.gmx, mg.garg))) return rc;
  }
  // ONE permutation set for every chromosome and trait: generated here, read by every chromosome's panels, never regenerated
  const int32_t* perm = dperm_idx;
  if (m > 0 && nperms > 0 && !perm) {
    if ((rc = launch_perm_gen(ctx, (int)n, nperms, seed))) return rc;
    ctx->perm_ready = false;                    // consumed here, not by a later launch_perm_panel
    perm = ptr<int32_t>(ctx->perm);
  }
  std::vector<Timer> tms;
  tms.reserve((size_t)nchr);
  bool audit = false;
  int64_t mt_max = 0;
  for (int64_t c : order) {
    const int64_t s0 = chr[c], pc = chr[c + 1] - chr[c];
    tms.emplace_back(ctx);
    Timer& tm = tms.back();
    Pipe P;
    const EigPre pre = loco_eig_pre(ctx, n, c, dst_all);
    if ((rc = prepare(ctx, opts, dY, n, 0, dG + (size_t)n * s0, pc, dCovar, ncov, dK + (size_t)c * n * n, dweights, 1, P, tm, false, false,
                      false, batched ? &pre : nullptr))) return rc;
    P.m = m; P.ldy = round_up(m > 0 ? m : 1, 128);
    if ((rc = ensure(ctx, ctx->Yt, sizeof(double) * (size_t)P.npad * P.ldy))) return rc;
    P.Yt = ptr<double>(ctx->Yt);
    // (launch_rotate_single, as bulk_perms_impl: the rotation scan gives its one trait, which the bit identity rests on)
    if ((rc = launch_rotate_single(ctx, ptr<double>(ctx->Rp), P.ldr, P.n, P.npad, dY, m, P.Yt, P.ldy))) return rc;
    const NullModel nm = null_model(P, opts);
    const size_t cm = (size_t)c * m;
    const BpermOut oc{o.g.h2 + cm, o.g.sigma2 + cm, o.chr_lod_max ? o.chr_lod_max + cm : nullptr,
                      o.chr_lod_argmax ? o.chr_lod_argmax + cm : nullptr, o.chr_max_perms ? o.chr_max_perms + cm * nperms : nullptr,
                      o.chr_thr ? o.chr_thr + cm * nprobs : nullptr, o.chr_pval ? o.chr_pval + cm : nullptr};
    if (m > 0 && (rc = launch_brent(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, oc.h2, oc.sigma2, nullptr, P.stat))) return rc;
    tm.mark();
    // chunks sized by the first (largest) chromosome for all of them: no workspace grows after it
    if (!mt_max) mt_max = bperm_chunk_traits(ctx, P.npad, P.ldx, n, pc, nperms);
    if ((rc = bperm_chunks(ctx, P, nm, m, pc, perm, nperms, mt_max, pr, nprobs, oc, s0, &mg))) return rc;
    tm.mark();
    if ((rc = end_call(ctx, P, nullptr, nullptr))) return rc;
    audit = audit || ctx->audit_ran;
    if ((rc = loco_chr_done(ctx, P, c, dst_all))) return rc;
  }
  if ((rc = loco_last_stat(ctx, batched, order, dst_all))) return rc;
  for (int64_t j0 = 0; j0 < m; j0 += 65535)     // the genome-wide tables
    if ((rc = launch_bperm_summary(ctx, mg.gmx + (size_t)j0 * np1, mg.garg + (size_t)j0 * np1, std::min<int64_t>(65535, m - j0), nperms, pr,
                                   (int)nprobs, j0, o.g.lod_max, o.g.lod_argmax, o.g.max_perms, o.g.thr, o.g.pval))) return rc;
  return loco_status(ctx, dst_all, nchr, audit, t0, tb, tms, status);
}

int blmm_bulkscan_loco_perms_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                                 const int64_t* chr_start, int64_t nchr, int64_t kinship_digits, const double* dCovar, int64_t ncov,
                                 const double* dweights, int64_t nperms, uint64_t seed, const int32_t* dperm_idx, const double* probs,
                                 int64_t nprobs, const double* dK_loco, double* dh2_out, double* dsigma2_out, double* dlod_max_out,
                                 int64_t* dlod_argmax_out, double* dmax_perms_out, double* dthr_out, double* dpval_out,
                                 double* dchr_lod_max_out, int64_t* dchr_lod_argmax_out, double* dchr_max_perms_out, double* dchr_thr_out,
                                 double* dchr_pval_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (ncov == 0) dCovar = nullptr;
  const LocoPermOut o{{dh2_out, dsigma2_out, dlod_max_out, dlod_argmax_out, dmax_perms_out, dthr_out, dpval_out},
                      dchr_lod_max_out, dchr_lod_argmax_out, dchr_max_perms_out, dchr_thr_out, dchr_pval_out};
  return loco_perms_impl(ctx, opts, dY, n, m, dG, p, chr_start, nchr, kinship_digits, dCovar, dCovar ? ncov : 0, dweights, dK_loco, nperms,
                         seed, dperm_idx, probs, nprobs, o, status);
}

int blmm_bulkscan_loco_perms(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                             const int64_t* chr_start, int64_t nchr, int64_t kinship_digits, const double* Covar, int64_t ncov,
                             const double* weights, int64_t nperms, uint64_t seed, const int32_t* perm_idx, const double* probs,
                             int64_t nprobs, double* h2_out, double* sigma2_out, double* lod_max_out, int64_t* lod_argmax_out,
                             double* max_perms_out, double* thr_out, double* pval_out, double* chr_lod_max_out,
                             int64_t* chr_lod_argmax_out, double* chr_max_perms_out, double* chr_thr_out, double* chr_pval_out,
                             blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  const LocoPermOut ho{{h2_out, sigma2_out, lod_max_out, lod_argmax_out, max_perms_out, thr_out, pval_out},
                       chr_lod_max_out, chr_lod_argmax_out, chr_max_perms_out, chr_thr_out, chr_pval_out};
  int rc = loco_perms_check(ctx, opts, n, m, p, chr_start, nchr, kinship_digits, Covar, ncov, nperms, probs, nprobs, Y && G, ho);
  if (rc) return rc;
  // caller-supplied permutations are indices into the trait's n entries: checked here, before a kernel reads through them
  if (perm_idx && nperms > 0)
    for (int64_t e = 0; e < n * nperms; ++e)
      if (perm_idx[e] < 0 || perm_idx[e] >= n) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_loco_perms: perm_idx entries must lie in 0 .. n - 1");
  HostCall hc(ctx);
  // device outputs in outL, m doubles per row: h2, sigma2 (nchr each); lod_max, lod_argmax, pval (1 each); thresholds (nprobs);
  // chr_lod_max, chr_lod_argmax, chr_pval (nchr each); chr_thresholds (nchr nprobs); then, when asked for, max_perms (nperms) and
  // chr_max_perms (nchr nperms)
  const size_t mm = (size_t)m, nc = (size_t)nchr, npr = (size_t)nprobs, npm = (size_t)nperms;
  const size_t o_thr = 2 * nc + 3, o_cmx = o_thr + npr, o_carg = o_cmx + nc, o_cpv = o_carg + nc, o_cthr = o_cpv + nc, o_mp = o_cthr + nc * npr;
  const size_t o_cmp = o_mp + (max_perms_out ? npm : 0), rows = o_cmp + (chr_max_perms_out ? nc * npm : 0);
  if ((rc = hc.begin()) || (rc = ensure(ctx, ctx->outL, sizeof(double) * (mm * rows + 1)))) return rc;
  double* d = ptr<double>(ctx->outL);
  const LocoPermOut o{{d, d + nc * mm, d + 2 * nc * mm, reinterpret_cast<int64_t*>(d + (2 * nc + 1) * mm), max_perms_out ? d + o_mp * mm : nullptr,
                       thr_out ? d + o_thr * mm : nullptr, pval_out ? d + (2 * nc + 2) * mm : nullptr},
                      chr_lod_max_out ? d + o_cmx * mm : nullptr, chr_lod_argmax_out ? reinterpret_cast<int64_t*>(d + o_carg * mm) : nullptr,
                      chr_max_perms_out ? d + o_cmp * mm : nullptr, chr_thr_out ? d + o_cthr * mm : nullptr,
                      chr_pval_out ? d + o_cpv * mm : nullptr};
  HostCall::In in;
  const int32_t* dperm;
  if ((rc = hc.inputs(Y, n, m, G, p, nullptr, Covar, ncov, weights, false, &in)) || (rc = up_perm_idx(hc, perm_idx, n, nperms, &dperm)) ||
      (rc = loco_perms_impl(ctx, opts, in.Y, n, m, in.G, p, chr_start, nchr, kinship_digits, in.Cov, in.ncov, in.W, nullptr, nperms, seed,
                            dperm, probs, nprobs, o, status))) return rc;
  if ((rc = hc.down(h2_out, o.g.h2, sizeof(double) * nc * mm)) || (rc = hc.down(sigma2_out, o.g.sigma2, sizeof(double) * nc * mm)) ||
      (rc = hc.down(lod_max_out, o.g.lod_max, sizeof(double) * mm)) || (rc = hc.down(lod_argmax_out, o.g.lod_argmax, sizeof(int64_t) * mm)) ||
      (rc = hc.down(pval_out, o.g.pval, sizeof(double) * mm)) || (rc = hc.down(thr_out, o.g.thr, sizeof(double) * mm * npr)) ||
      (rc = hc.down(chr_lod_max_out, o.chr_lod_max, sizeof(double) * nc * mm)) ||
      (rc = hc.down(chr_lod_argmax_out, o.chr_lod_argmax, sizeof(int64_t) * nc * mm)) ||
      (rc = hc.down(chr_pval_out, o.chr_pval, sizeof(double) * nc * mm)) || (rc = hc.down(chr_thr_out, o.chr_thr, sizeof(double) * nc * mm * npr)))
    return rc;
  if (max_perms_out && (rc = copy_to_host(ctx, max_perms_out, o.g.max_perms, sizeof(double) * mm * npm))) return rc;
  if (chr_max_perms_out && (rc = copy_to_host(ctx, chr_max_perms_out, o.chr_max_perms, sizeof(double) * nc * mm * npm))) return rc;
  return (rc = hc.finish()) ? rc : check_sticky(ctx);
}

// ---------------------------------------------------------------------------------------------------
// scan(...; assumption = "alt") -> scan_alt (src/scan.jl:397-453): scalars [sigma2_e, h2_null], lod p, h2_each_marker p
int blmm_scan_alt_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dy, int64_t n, const double* dG, int64_t p,
                      const double* dCovar, int64_t ncov, const double* dK, const double* dweights, double* dscalars_out,
                      double* dlod_out, double* dh2_each_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  int rc = check_opts(ctx, opts);
  if (rc) return rc;
  if (!dy || !dG || !dK || !dscalars_out || !dlod_out || !dh2_each_out) return fail(ctx, BLMM_ERR_INVALID, "scan_alt: NULL buffer");
  if ((rc = enter_device(ctx))) return rc;
  Timer tm(ctx);
  Pipe P;
  if ((rc = prepare(ctx, opts, dy, n, 1, dG, p, dCovar, ncov, dK, dweights, 1, P, tm))) return rc;
  const NullModel nm = null_model(P, opts);
  if (P.c + 1 >= P.n) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  if ((rc = launch_brent(ctx, nm, P.Yt, P.ldy, 1, P.Z0, P.lam, dscalars_out + 1, dscalars_out, nullptr, P.stat))) return rc;
  tm.mark();
  if ((rc = launch_alt_brent(ctx, nm, P.Yt, P.ldy, P.Xt, P.ldx, p, P.Z0, P.lam, dscalars_out + 1,
                             (opts->compat_flags & BLMM_COMPAT_ALT_TRUE_WEIGHTS) ? 1 : 0, dlod_out, dh2_each_out, P.stat))) return rc;
  tm.mark();
  return end_call(ctx, P, status, &tm);
}

// Bulk form of scan_alt (second half; the reference has only the single-trait function, src/scan.jl:397-453, and
// the grid approximation bulkscan_alt_grid): for EVERY (trait, marker) the exact heritability under the alternative -- one Brent
// search per test on the design [Z0 x_i] -- and the LOD against the trait's null model.  The per-trait null searches run in bulk
// (k_brent), the per-test searches as k_alt_brent with the trait on blockIdx.y: bit-identical, column by column, to
// blmm_scan_alt_dev on that trait.  ~0.02 us per test at n = 79 (64 traits x 7321 markers: 8.6 ms host to host; the whole BXD
// matrix would take ~5 s against the grid kernel's 15 ms): meant for trait subsets.
int blmm_bulkscan_alt_exact_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG,
                                int64_t p, const double* dCovar, int64_t ncov, const double* dK, const double* dweights,
                                double* dL_out, int64_t ldL, double* dh2_panel_out, int64_t ldH, double* dh2_null_out,
                                double* dsigma2_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  int rc = check_opts(ctx, opts);
  if (rc) return rc;
  if (!dY || !dG || !dK || !dL_out || !dh2_panel_out || !dh2_null_out) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_alt_exact: NULL buffer");
  if (ldL < p || ldH < p) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_alt_exact: leading dimension < p");
  if ((rc = enter_device(ctx))) return rc;
  Timer tm(ctx);
  Pipe P;
  if ((rc = prepare(ctx, opts, dY, n, m, dG, p, dCovar, ncov, dK, dweights, 1, P, tm))) return rc;
  const NullModel nm = null_model(P, opts);
  if (P.c + 1 >= P.n) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  if (m > 0) {
    double* dsig = dsigma2_out;
    if (!dsig) { if ((rc = ensure(ctx, ctx->sig2, sizeof(double) * (size_t)m))) return rc; dsig = ptr<double>(ctx->sig2); }
    if ((rc = launch_brent(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, dh2_null_out, dsig, nullptr, P.stat))) return rc;
  }
  tm.mark();
  if ((rc = launch_alt_brent(ctx, nm, P.Yt, P.ldy, P.Xt, P.ldx, p, P.Z0, P.lam, dh2_null_out,
                             (opts->compat_flags & BLMM_COMPAT_ALT_TRUE_WEIGHTS) ? 1 : 0, dL_out, dh2_panel_out, P.stat, m, ldL, ldH))) return rc;
  tm.mark(); tm.mark();
  return end_call(ctx, P, status, &tm);
}

int blmm_bulkscan_alt_exact(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                            const double* Covar, int64_t ncov, const double* K, const double* weights, double* L_out,
                            double* h2_panel_out, double* h2_null_out, double* sigma2_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (!opts) return fail(ctx, BLMM_ERR_INVALID, "opts is NULL");
  if (!Y || !G || !K || !L_out || !h2_panel_out || !h2_null_out) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_alt_exact: NULL buffer");
  if (n < 1 || p < 1 || m < 1) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  HostCall hc(ctx);
  int rc;
  if ((rc = hc.begin()) || (rc = ensure(ctx, ctx->outL, sizeof(double) * 2 * (size_t)p * m)) || (rc = ensure(ctx, ctx->outH2, sizeof(double) * 2 * (size_t)m)))
    return rc;
  HostCall::In d;
  if ((rc = hc.inputs(Y, n, m, G, p, K, Covar, ncov, weights, false, &d))) return rc;
  double* dL = ptr<double>(ctx->outL);
  double* dH = dL + (size_t)p * m;
  double* dh2 = ptr<double>(ctx->outH2);
  if ((rc = blmm_bulkscan_alt_exact_dev(ctx, opts, d.Y, n, m, d.G, p, d.Cov, d.ncov, d.K, d.W, dL, p, dH, p, dh2, dh2 + m, status))) return rc;
  set_last(ctx, dL, p, m);
  if ((rc = copy_to_host(ctx, L_out, dL, sizeof(double) * (size_t)p * m)) || (rc = copy_to_host(ctx, h2_panel_out, dH, sizeof(double) * (size_t)p * m)) ||
      (rc = hc.down(h2_null_out, dh2, sizeof(double) * (size_t)m)) || (rc = hc.down(sigma2_out, dh2 + m, sizeof(double) * (size_t)m))) return rc;
  return (rc = hc.finish()) ? rc : check_sticky(ctx);
}

int blmm_scan_alt(blmm_ctx* ctx, const blmm_opts* opts, const double* y, int64_t n, const double* G, int64_t p,
                  const double* Covar, int64_t ncov, const double* K, const double* weights, double* scalars_out,
                  double* lod_out, double* h2_each_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (!opts) return fail(ctx, BLMM_ERR_INVALID, "opts is NULL");
  if (!y || !G || !K || !scalars_out || !lod_out || !h2_each_out) return fail(ctx, BLMM_ERR_INVALID, "scan_alt: NULL buffer");
  if (n < 1 || p < 1) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  HostCall hc(ctx);
  int rc;
  if ((rc = hc.begin()) || (rc = ensure(ctx, ctx->outL, sizeof(double) * 2 * (size_t)p)) || (rc = ensure(ctx, ctx->outH2, sizeof(double) * 2))) return rc;
  HostCall::In d;
  if ((rc = hc.inputs(y, n, 1, G, p, K, Covar, ncov, weights, false, &d))) return rc;
  double* dL = ptr<double>(ctx->outL);
  if ((rc = blmm_scan_alt_dev(ctx, opts, d.Y, n, d.G, p, d.Cov, d.ncov, d.K, d.W, ptr<double>(ctx->outH2), dL, dL + p, status))) return rc;
  set_last(ctx, dL, p, 1);
  if ((rc = hc.down(scalars_out, ctx->outH2.p, sizeof(double) * 2)) || (rc = hc.down(lod_out, dL, sizeof(double) * p)) ||
      (rc = hc.down(h2_each_out, dL + p, sizeof(double) * p))) return rc;
  return (rc = hc.finish()) ? rc : check_sticky(ctx);
}

// ---------------------------------------------------------------------------------------------------
// lower-level seams (host pointers)
// ---------------------------------------------------------------------------------------------------
int blmm_rotate(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                const double* Covar, int64_t ncov, const double* K, double* Y0_out, double* X0_out, double* lambda_out,
                blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  int rc = check_opts(ctx, opts);
  if (rc) return rc;
  if (!Y || !G || !K || !Y0_out || !X0_out || !lambda_out) return fail(ctx, BLMM_ERR_INVALID, "rotate: NULL buffer");
  if (n < 1 || m < 1 || p < 1) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  HostCall hc(ctx);
  HostCall::In d;
  if ((rc = hc.begin()) || (rc = hc.inputs(Y, n, m, G, p, K, Covar, ncov, nullptr, false, &d))) return rc;
  Timer tm(ctx);
  Pipe P;
  if ((rc = prepare(ctx, opts, d.Y, n, m, d.G, p, d.Cov, d.ncov, d.K, nullptr, 0, P, tm))) return rc;
  if ((rc = ensure(ctx, ctx->outL, sizeof(double) * n * (size_t)(m > p ? m : p)))) return rc;
  double* tmp = ptr<double>(ctx->outL);
  if ((rc = launch_untranspose(ctx, P.Yt, P.ldy, (int)n, m, tmp)) || (rc = hc.down(Y0_out, tmp, sizeof(double) * n * m))) return rc;
  BLMM_HIP(hipStreamSynchronize(ctx->stream));      // tmp is reused for the markers
  if ((rc = launch_untranspose(ctx, P.Xt, P.ldx, (int)n, p, tmp)) || (rc = hc.down(X0_out + (size_t)n * P.c, tmp, sizeof(double) * n * p)) ||
      (rc = hc.down(X0_out, P.Z0, sizeof(double) * n * P.c)) || (rc = hc.down(lambda_out, P.lam, sizeof(double) * n))) return rc;
  return (rc = hc.finish()) ? rc : finish_status(ctx, status, nullptr);
}

namespace {
// uploads rotated host inputs into the pipeline's internal layouts (no eigen / rotation)
int upload_rotated(HostCall& hc, const double* Y0, int64_t n, int64_t m, const double* Z0, int64_t c, const double* X0m,
                   int64_t p, const double* lambda, Pipe& P) {
  blmm_ctx* ctx = hc.ctx;
  if (n < 1 || m < 1 || c < 1 || c > CMAX || c >= n) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  ctx->prep_valid = false;   // Z0 / lambda / the status block of a blmm_prepare_dev are overwritten below
  P.n = (int)n; P.c = (int)c; P.npad = (int)round_up(n, 8); P.ldr = (int)round_up(P.npad, 16);
  P.m = m; P.p = p; P.ldy = round_up(m, 128); P.ldx = round_up(p > 0 ? p : 1, 128);
  int rc;
  if ((rc = ensure(ctx, ctx->Yt, sizeof(double) * (size_t)P.npad * P.ldy)) || (rc = reset_stat(ctx, &P.stat)) ||
      (rc = hc.up(ctx->inY, Y0, sizeof(double) * n * m)) || (rc = hc.up(ctx->Z0, Z0, sizeof(double) * n * c)) ||
      (rc = hc.up(ctx->lam, lambda, sizeof(double) * n))) return rc;
  P.Yt = ptr<double>(ctx->Yt); P.Z0 = ptr<double>(ctx->Z0); P.lam = ptr<double>(ctx->lam);
  if ((rc = to_rowmajor(ctx, ptr<double>(ctx->inY), (int)n, m, P.Yt, P.npad, P.ldy))) return rc;
  if (X0m && p > 0) {
    if ((rc = ensure(ctx, ctx->Xt, sizeof(double) * (size_t)P.npad * P.ldx)) || (rc = hc.up(ctx->inG, X0m, sizeof(double) * n * p))) return rc;
    P.Xt = ptr<double>(ctx->Xt);
    if ((rc = to_rowmajor(ctx, ptr<double>(ctx->inG), (int)n, p, P.Xt, P.npad, P.ldx))) return rc;
  }
  return BLMM_OK;
}
}  // namespace

int blmm_null_h2_brent(blmm_ctx* ctx, const blmm_opts* opts, const double* Y0, int64_t n, int64_t m, const double* Z0,
                       int64_t c, const double* lambda, double* h2_out, double* sigma2_out, double* ell_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (!opts || !Y0 || !Z0 || !lambda || !h2_out) return fail(ctx, BLMM_ERR_INVALID, "null_h2_brent: NULL buffer");
  HostCall hc(ctx);
  Pipe P;
  int rc;
  if ((rc = hc.begin()) || (rc = upload_rotated(hc, Y0, n, m, Z0, c, nullptr, 0, lambda, P))) return rc;
  const NullModel nm = null_model(P, opts);
  if ((rc = ensure(ctx, ctx->h2, sizeof(double) * m)) || (rc = ensure(ctx, ctx->sig2, sizeof(double) * m)) || (rc = ensure(ctx, ctx->ell, sizeof(double) * m)) ||
      (rc = launch_brent(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, ptr<double>(ctx->h2), ptr<double>(ctx->sig2), ptr<double>(ctx->ell), P.stat)) ||
      (rc = hc.down(h2_out, ctx->h2.p, sizeof(double) * m)) || (rc = hc.down(sigma2_out, ctx->sig2.p, sizeof(double) * m)) ||
      (rc = hc.down(ell_out, ctx->ell.p, sizeof(double) * m))) return rc;
  return (rc = hc.finish()) ? rc : finish_status(ctx, status, nullptr);
}

int blmm_null_loglik_grid(blmm_ctx* ctx, const blmm_opts* opts, const double* Y0, int64_t n, int64_t m, const double* Z0,
                          int64_t c, const double* lambda, const double* h2_grid, int64_t ngrid, double* Ell_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (!opts || !Y0 || !Z0 || !lambda || !Ell_out) return fail(ctx, BLMM_ERR_INVALID, "null_loglik_grid: NULL buffer");
  HostCall hc(ctx);
  double* dgrid = nullptr;
  Pipe P;
  int rc;
  if ((rc = hc.begin()) || (rc = grid_to_device(ctx, h2_grid, ngrid, &dgrid)) || (rc = upload_rotated(hc, Y0, n, m, Z0, c, nullptr, 0, lambda, P)))
    return rc;
  const NullModel nm = null_model(P, opts);
  if ((rc = ensure(ctx, ctx->EllTab, sizeof(double) * (size_t)ngrid * m)) ||
      (rc = launch_loglik_grid(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, dgrid, (int)ngrid, ptr<double>(ctx->EllTab), nullptr, nullptr, P.stat)) ||
      (rc = hc.down(Ell_out, ctx->EllTab.p, sizeof(double) * (size_t)ngrid * m))) return rc;
  return (rc = hc.finish()) ? rc : finish_status(ctx, status, nullptr);
}

int blmm_weighted_liteqtl(blmm_ctx* ctx, const double* Y0, int64_t n, int64_t m, const double* X0, int64_t c, int64_t p,
                          const double* lambda, double hsq, double* LOD_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (!Y0 || !X0 || !lambda || !LOD_out || p < 1) return fail(ctx, BLMM_ERR_INVALID, "weighted_liteqtl: bad arguments");
  if (std::isinf(hsq / (1.0 - hsq))) return fail(ctx, BLMM_ERR_H2_ONE, "Heritability of 1 is not allowed.");
  HostCall hc(ctx);
  Pipe P;
  int rc;
  if ((rc = hc.begin()) || (rc = upload_rotated(hc, Y0, n, m, X0, c, X0 + (size_t)n * c, p, lambda, P))) return rc;
  blmm_opts o; blmm_default_opts(&o);
  const NullModel nm = null_model(P, &o);
  if ((rc = ensure(ctx, ctx->h2, sizeof(double) * m))) return rc;
  if ((rc = fill(ctx, ptr<double>(ctx->h2), m, hsq))) return rc;
  if ((rc = ensure(ctx, ctx->panels, sizeof(double) * (size_t)P.npad * P.ldy))) return rc;
  if ((rc = launch_panels(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, ptr<double>(ctx->h2), 0, ptr<double>(ctx->panels), P.ldy, P.stat))) return rc;
  if ((rc = ensure(ctx, ctx->isx, sizeof(double) * (size_t)P.ldx))) return rc;
  if ((rc = launch_isx(ctx, nm, P.Xt, P.ldx, p, P.Z0, P.lam, ptr<double>(ctx->h2), 1, ptr<double>(ctx->isx), P.ldx, P.stat))) return rc;
  if ((rc = ensure(ctx, ctx->outL, sizeof(double) * (size_t)p * m))) return rc;
  ScanArgs a = scan_args(ctx, P, ptr<double>(ctx->panels), P.ldy, ptr<double>(ctx->outL), p, m);
  a.isx = ptr<double>(ctx->isx); a.ld_isx = P.ldx;
  if ((rc = launch_scan_table(ctx, a)) || (rc = hc.down(LOD_out, ctx->outL.p, sizeof(double) * (size_t)p * m))) return rc;
  return (rc = hc.finish()) ? rc : finish_status(ctx, status, nullptr);
}

int blmm_liteqtl_given_h2(blmm_ctx* ctx, const double* Y0, int64_t n, int64_t m, const double* X0, int64_t c, int64_t p,
                          const double* lambda, const double* h2, double* LOD_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (!Y0 || !X0 || !lambda || !h2 || !LOD_out || p < 1) return fail(ctx, BLMM_ERR_INVALID, "liteqtl_given_h2: bad arguments");
  for (int64_t j = 0; j < m; ++j)
    if (std::isinf(h2[j] / (1.0 - h2[j]))) return fail(ctx, BLMM_ERR_H2_ONE, "Heritability of 1 is not allowed.");
  HostCall hc(ctx);
  Pipe P;
  int rc;
  if ((rc = hc.begin()) || (rc = upload_rotated(hc, Y0, n, m, X0, c, X0 + (size_t)n * c, p, lambda, P))) return rc;
  blmm_opts o; blmm_default_opts(&o);
  const NullModel nm = null_model(P, &o);
  if ((rc = hc.up(ctx->h2, h2, sizeof(double) * m)) || (rc = ensure(ctx, ctx->outL, sizeof(double) * (size_t)p * m))) return rc;
  // the same kernel choice as bulkscan(method = null-exact): low-rank weights form with its residual guard unless
  // BLMM_EXACT=full, c = 4 or n beyond the basis kernel
  if (lowrank_form(ctx, P.c, n)) {
    Timer tm(ctx);
    if ((rc = lr_begin(ctx, P, /*wbasis_started*/ false))) return rc;
    if ((rc = lr_finish(ctx, P, nm, ptr<double>(ctx->h2), ptr<double>(ctx->outL), p, tm))) return rc;
  } else {
    if ((rc = ensure(ctx, ctx->panels, sizeof(double) * (size_t)(2 + P.c) * P.npad * P.ldy))) return rc;
    if ((rc = launch_panels(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, ptr<double>(ctx->h2), 1, ptr<double>(ctx->panels), P.ldy, P.stat))) return rc;
    ScanArgs a = scan_args(ctx, P, ptr<double>(ctx->panels), P.ldy, ptr<double>(ctx->outL), p, m);
    if ((rc = launch_scan_exact(ctx, a, P.c))) return rc;
    if ((rc = illcond_rescan(ctx, P, nm, m, ptr<double>(ctx->h2), ptr<double>(ctx->outL), p))) return rc;
  }
  if ((rc = hc.down(LOD_out, ctx->outL.p, sizeof(double) * (size_t)p * m))) return rc;
  return (rc = hc.finish()) ? rc : finish_status(ctx, status, nullptr);
}


// ---------------------------------------------------------------------------------------------------
// The k-degree-of-freedom scan (include/bulklmm_hip.h: blmm_bulkscan_multidf; kernels_mdf.hip).  Every refusal that needs no device
// comes first, in the same order in the host and the device forms.
static int multidf_check(blmm_ctx* ctx, const blmm_opts* opts, int64_t n, int64_t m, int64_t p, int64_t k, const double* Covar,
                         int64_t ncov) {
  int rc = check_opts(ctx, opts);
  if (rc) return rc;
  if (n < 1 || m < 0 || p < 0 || ncov < 0 || p > 0x7fffffffLL || m > 0x7fffffffLL) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  if (k < 1 || p % k != 0) return fail(ctx, BLMM_ERR_DIM, "bulkscan_multidf: the number of columns of G must be a multiple of k >= 1");
  if ((rc = check_method(ctx, opts))) return rc;
  if (opts->method == BLMM_ALT_GRID) return fail(ctx, BLMM_ERR_UNSUPPORTED, "bulkscan_multidf: alt-grid is not supported; use null-grid or null-exact");
  const int64_t kmax = opts->method == BLMM_NULL_EXACT ? BLMM_MULTIDF_MAX_K_EXACT : BLMM_MULTIDF_MAX_K_GRID;
  if (k > kmax)
    return fail(ctx, BLMM_ERR_UNSUPPORTED, std::string("bulkscan_multidf: ") + (opts->method == BLMM_NULL_EXACT ? "null-exact" : "null-grid") +
                " takes 1 <= k <= " + std::to_string((long long)kmax));
  if (null_cov(opts, Covar, ncov).c > BLMM_MULTIDF_MAX_COVARIATES)
    return fail(ctx, BLMM_ERR_UNSUPPORTED, "bulkscan_multidf: more than 8 null covariates (incl. intercept) are not supported");
  if (n > 2048) return fail(ctx, BLMM_ERR_UNSUPPORTED, "more than 2048 individuals: the device eigensolver (tridiagonalisation + divide and conquer) stops at n = 2048");
  return BLMM_OK;
}

// The triplet buffers of a blmm_reduced, as reduced_check asks for them
static int multidf_reduced_check(blmm_ctx* ctx, const blmm_reduced* out) {
  if (!out) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_multidf_reduced: NULL buffer");
  if (out->cap < 0 || (out->cap > 0 && (!out->ti || !out->tj || !out->tlod)) || (out->want_triplets && !out->count))
    return fail(ctx, BLMM_ERR_INVALID, "bulkscan_multidf_reduced: triplet buffers");
  return BLMM_OK;
}

// The traits the conditioning guard listed (blmm_bulkscan_multidf_reduced, null-exact, c >= 2), behind the reducing scan and
// k_red_final: a chunk of the list at a time, k_mdf_qr recomputes the traits' columns into a scratch of that many columns and
// k_mdf_flag_red reduces them over the (-inf, -1) the scan left for them and appends their triplets.  Waits for the stream once, for
// the length of the list.
static int multidf_reduced_flagged(blmm_ctx* ctx, const Pipe& P, const NullModel& nm, int64_t nloci, int k, const double* dh2,
                                   const RedArgs& r, const blmm_reduced* red) {
  int64_t cnt = 0;
  BLMM_HIP(hipMemcpyAsync(&cnt, P.stat + ST_ILLCOND, sizeof(cnt), hipMemcpyDeviceToHost, ctx->stream));
  BLMM_HIP(hipStreamSynchronize(ctx->stream));
  if (cnt <= 0) return BLMM_OK;
  ctx->last_reduced_route = 3;
  int64_t chunk = ctx->tune.mdf_red_chunk > 0 ? ctx->tune.mdf_red_chunk : (int64_t)(64ll << 20) / (int64_t)(sizeof(double) * (size_t)nloci);
  chunk = std::min(std::max<int64_t>(chunk, 1), cnt);
  int rc = ensure(ctx, ctx->mdfScr, sizeof(double) * (size_t)nloci * (size_t)chunk);
  if (rc) return rc;
  double* scr = ptr<double>(ctx->mdfScr);
  for (int64_t item0 = 0; item0 < cnt; item0 += chunk) {
    const int64_t nitem = std::min(chunk, cnt - item0);
    if ((rc = launch_mdf_qr(ctx, nm, P.Yt, P.ldy, P.Xt, P.ldx, nloci, k, P.Z0, P.lam, dh2, ptr<int>(ctx->illList), nullptr, 0, P.stat,
                            scr, item0, nitem)) ||
        (rc = launch_mdf_flag_red(ctx, scr, nloci, ptr<int>(ctx->illList), P.stat, item0, nitem, red->colmax, red->argmax, r))) return rc;
  }
  return BLMM_OK;
}

// red != nullptr: blmm_bulkscan_multidf_reduced -- `red` (device pointers) instead of dL_out / ldL, no P x m matrix anywhere
static int multidf_dev_impl(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                            int64_t k, const double* dCovar, int64_t ncov, const double* dK, const double* dweights,
                            const double* h2_grid_host, int64_t ngrid, double* dL_out, int64_t ldL, double* dh2_out,
                            blmm_status* status, const PvReq& pvreq, const blmm_reduced* red = nullptr) {
  int rc = multidf_check(ctx, opts, n, m, p, k, dCovar, ncov);
  if (rc) return rc;
  const int64_t nloci = p / k;
  if (!dY || !dG || !dK || (!red && !dL_out) || !dh2_out)
    return fail(ctx, BLMM_ERR_INVALID, red ? "bulkscan_multidf_reduced: NULL buffer" : "bulkscan_multidf: NULL buffer");
  if (red && (rc = multidf_reduced_check(ctx, red))) return rc;
  if (!red && ldL < nloci) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_multidf: ldL < p / k");
  const bool exact = opts->method == BLMM_NULL_EXACT;
  if ((rc = enter_device(ctx))) return rc;
  Timer tm(ctx);
  Pipe P;
  double* dgrid = nullptr;
  if (!exact && (rc = grid_to_device(ctx, h2_grid_host, ngrid, &dgrid))) return rc;
  // blmm_bulkscan's design, eigen phase and trait rotation (so the null model is its own, bit for bit); the markers are rotated
  // below without the centring projection
  const bool g_in_flight = ctx->up_pending || ctx->in_wait;   // (host form) G may still be on its way up: ev_in says when it is there
  if ((rc = prepare(ctx, opts, dY, n, m, dG, p, dCovar, ncov, dK, dweights, 1, P, tm, false, false, /*skip_markers*/ true))) return rc;
  if (g_in_flight) BLMM_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_in, 0));
  const NullModel nm = null_model(P, opts);
  PvCall pvc(ctx, pvreq);
  if ((rc = pvc.resolve(nloci, m))) return rc;   // always the column pass over the finished L (fused stays false)
  // the reduced form's state: one slot per 64 loci (k_mdf_grid_red / k_mdf_exact_red), finished by k_red_final; *count zeroed
  RedArgs r;
  const int nslot = (int)((nloci + 63) / 64);
  if (red && (rc = red_state(ctx, red, std::max(nslot, 1), m, &r))) return rc;
  if (m == 0) { tm.mark(); tm.mark(); tm.mark(); return end_call(ctx, P, status, &tm); }
  if (nloci == 0) {
    if (exact) {
      if ((rc = launch_brent(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, dh2_out, nullptr, nullptr, P.stat))) return rc;
    } else {
      if ((rc = ensure(ctx, ctx->h2idx, sizeof(int) * (size_t)m))) return rc;
      if ((rc = launch_loglik_grid(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, dgrid, (int)ngrid, nullptr, ptr<int>(ctx->h2idx), dh2_out, P.stat))) return rc;
    }
    if (red && (rc = launch_red_final(ctx, r, 0, m, red->colmax, red->argmax))) return rc;   // no locus: (-inf, -1)
    tm.mark(); tm.mark(); tm.mark();
    return end_call(ctx, P, status, &tm);
  }
  if ((rc = ensure(ctx, ctx->mdfR, sizeof(double) * (size_t)P.npad * P.ldr)) ||
      (rc = ensure(ctx, ctx->Xt, sizeof(double) * (size_t)P.npad * P.ldx))) return rc;
  if ((rc = launch_mdf_rawrot(ctx, ptr<double>(ctx->U), dweights, P.n, P.npad, P.ldr, ptr<double>(ctx->mdfR)))) return rc;
  P.Xt = ptr<double>(ctx->Xt);
  if ((rc = launch_rotate(ctx, ptr<double>(ctx->mdfR), P.ldr, P.n, P.npad, dG, p, P.Xt, P.ldx, P.ldx))) return rc;
  MdfArgs a;
  a.Xt = P.Xt; a.ldx = P.ldx; a.nloci = nloci; a.k = (int)k; a.n = P.n; a.m = m;
  a.ldp = P.ldy; a.pstride = (int64_t)P.npad * P.ldy; a.c = P.c;
  a.T = nullptr; a.bin = nullptr; a.L = dL_out; a.ldL = ldL; a.stat = P.stat;
  const int64_t ldp = P.ldy;
  if (exact) {
    if ((rc = launch_brent(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, dh2_out, nullptr, nullptr, P.stat))) return rc;
    tm.mark();
    if ((rc = ensure(ctx, ctx->panels, sizeof(double) * (size_t)(2 + P.c) * P.npad * ldp))) return rc;
    if ((rc = launch_panels(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, dh2_out, 1, ptr<double>(ctx->panels), ldp, P.stat))) return rc;
    tm.mark();
    a.P = ptr<double>(ctx->panels);
    if (red) {
      // the guard runs AHEAD of the scan: its flags tell the epilogue which traits to leave to the re-scan
      if (P.c >= 2) {
        if ((rc = ensure(ctx, ctx->illList, sizeof(int) * (size_t)m)) || (rc = ensure(ctx, ctx->redflag, sizeof(int) * (size_t)m))) return rc;
        r.flags = ptr<int>(ctx->redflag);
        BLMM_HIP(hipMemsetAsync(r.flags, 0, sizeof(int) * (size_t)m, ctx->stream));
        if ((rc = launch_illcond_flag(ctx, nm, m, P.Z0, P.lam, dh2_out, ptr<int>(ctx->illList), P.stat, r.flags))) return rc;
      }
      if ((rc = launch_mdf_scan_traits_red(ctx, a, r, true)) || (rc = launch_red_final(ctx, r, nslot, m, red->colmax, red->argmax))) return rc;
      if (P.c >= 2 && (rc = multidf_reduced_flagged(ctx, P, nm, nloci, (int)k, dh2_out, r, red))) return rc;
    } else {
    if ((rc = launch_mdf_scan(ctx, a, true))) return rc;
    // conditioning guard (c >= 2): the flagged traits' columns again, orthogonalised
    if (P.c >= 2) {
      if ((rc = ensure(ctx, ctx->illList, sizeof(int) * (size_t)m))) return rc;
      if ((rc = launch_illcond_flag(ctx, nm, m, P.Z0, P.lam, dh2_out, ptr<int>(ctx->illList), P.stat))) return rc;
      if ((rc = launch_mdf_qr(ctx, nm, P.Yt, P.ldy, P.Xt, P.ldx, nloci, (int)k, P.Z0, P.lam, dh2_out, ptr<int>(ctx->illList), dL_out, ldL, P.stat))) return rc;
    }
    }
    tm.mark();
  } else {
    if ((rc = ensure(ctx, ctx->h2idx, sizeof(int) * (size_t)m))) return rc;
    if ((rc = launch_loglik_grid(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, dgrid, (int)ngrid, nullptr, ptr<int>(ctx->h2idx), dh2_out, P.stat))) return rc;
    tm.mark();
    if ((rc = ensure(ctx, ctx->panels, sizeof(double) * (size_t)P.npad * ldp))) return rc;
    if ((rc = launch_panels(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, dh2_out, 0, ptr<double>(ctx->panels), ldp, P.stat))) return rc;
    const int64_t np = k * (k + 1) / 2;
    if ((rc = ensure(ctx, ctx->mdfT, sizeof(double) * (size_t)ngrid * nloci * np))) return rc;
    if ((rc = launch_mdf_table(ctx, nm, P.Xt, P.ldx, nloci, (int)k, P.Z0, P.lam, dgrid, (int)ngrid, ptr<double>(ctx->mdfT)))) return rc;
    tm.mark();
    a.P = ptr<double>(ctx->panels); a.T = ptr<double>(ctx->mdfT); a.bin = ptr<int>(ctx->h2idx);
    if (red) {
      if ((rc = launch_mdf_scan_traits_red(ctx, a, r, false)) || (rc = launch_red_final(ctx, r, nslot, m, red->colmax, red->argmax))) return rc;
    } else if ((rc = launch_mdf_scan(ctx, a, false))) return rc;
    tm.mark();
  }
  if (!red && (rc = pvc.finish(nloci, m, dL_out, ldL))) return rc;
  return end_call(ctx, P, status, &tm);
}

int blmm_bulkscan_multidf_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG,
                              int64_t p, int64_t k, const double* dCovar, int64_t ncov, const double* dK, const double* dweights,
                              const double* h2_grid, int64_t ngrid, double* dL_out, int64_t ldL, double* dh2_out,
                              blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  const PvReq pvreq = pv_take(ctx);
  ctx->red_cur = RedArgs();
  return multidf_dev_impl(ctx, opts, dY, n, m, dG, p, k, dCovar, ncov, dK, dweights, h2_grid, ngrid, dL_out, ldL, dh2_out, status, pvreq);
}

// L_out == NULL: L (P x m) stays resident for the blmm_last_* consumers, as blmm_bulkscan
int blmm_bulkscan_multidf(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                          int64_t k, const double* Covar, int64_t ncov, const double* K, const double* weights,
                          const double* h2_grid, int64_t ngrid, double* L_out, double* h2_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  const PvReq pvreq = pv_take(ctx);
  int rc = multidf_check(ctx, opts, n, m, p, k, Covar, ncov);
  if (rc) return rc;
  if (!Y || !G || !K || !h2_out) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_multidf: NULL buffer");
  const int64_t nloci = p / k;
  HostCall hc(ctx);
  if ((rc = hc.begin()) || (rc = ensure(ctx, ctx->outL, sizeof(double) * (size_t)(nloci > 0 ? nloci : 1) * (m > 0 ? m : 1))) ||
      (rc = ensure(ctx, ctx->outH2, sizeof(double) * (size_t)(m > 0 ? m : 1))))
    return rc;
  HostCall::In d;
  if ((rc = hc.inputs(Y, n, m, G, p, K, Covar, ncov, weights, /*defer*/ true, &d))) return rc;
  ctx->red_cur = RedArgs();
  if ((rc = multidf_dev_impl(ctx, opts, d.Y, n, m, d.G, p, k, d.Cov, d.ncov, d.K, d.W, h2_grid, ngrid, ptr<double>(ctx->outL),
                             nloci > 0 ? nloci : 1, ptr<double>(ctx->outH2), status, pvreq))) return rc;
  set_last(ctx, ptr<double>(ctx->outL), nloci, m);
  if (L_out && (size_t)nloci * m > 0 && (rc = copy_to_host(ctx, L_out, ctx->outL.p, sizeof(double) * (size_t)nloci * m))) return rc;
  if (m > 0 && (rc = copy_to_host(ctx, h2_out, ctx->outH2.p, sizeof(double) * (size_t)m))) return rc;
  if ((rc = hc.finish())) return rc;
  return check_sticky(ctx);
}

// The k-df scan without the matrix (include/bulklmm_hip.h: blmm_bulkscan_multidf_reduced).  `out` holds DEVICE pointers here.  The
// call writes no matrix, so a pending -log10 p request is refused (and consumed); it waits for the stream before it returns.
static const char* const kMdfRedPv = "bulkscan_multidf_reduced: a blmm_set_log10p_output request is pending (the reduced call writes no matrix)";
static int multidf_reduced_run(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                               int64_t k, const double* dCovar, int64_t ncov, const double* dK, const double* dweights,
                               const double* h2_grid, int64_t ngrid, const blmm_reduced* out, double* dh2_out, blmm_status* status) {
  ctx->red_cur = RedArgs();
  ctx->last_reduced_route = 1;              // 3: traits the conditioning guard flagged were re-scanned (multidf_reduced_flagged)
  int rc = multidf_dev_impl(ctx, opts, dY, n, m, dG, p, k, dCovar, ncov, dK, dweights, h2_grid, ngrid, nullptr, 0, dh2_out, status, PvReq(), out);
  if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
  clear_last(ctx);                          // no matrix of this call: an earlier one is not served as its result
  BLMM_HIP(hipStreamSynchronize(ctx->stream));
  return check_sticky(ctx);
}

int blmm_bulkscan_multidf_reduced_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG,
                                      int64_t p, int64_t k, const double* dCovar, int64_t ncov, const double* dK, const double* dweights,
                                      const double* h2_grid, int64_t ngrid, const blmm_reduced* out, double* dh2_out,
                                      blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (pv_take(ctx).armed) return fail(ctx, BLMM_ERR_INVALID, kMdfRedPv);
  return multidf_reduced_run(ctx, opts, dY, n, m, dG, p, k, dCovar, ncov, dK, dweights, h2_grid, ngrid, out, dh2_out, status);
}

// host-pointer form: `out` holds HOST pointers; the small results come back, nothing P x m exists
int blmm_bulkscan_multidf_reduced(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                                  int64_t k, const double* Covar, int64_t ncov, const double* K, const double* weights,
                                  const double* h2_grid, int64_t ngrid, const blmm_reduced* out, double* h2_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (pv_take(ctx).armed) return fail(ctx, BLMM_ERR_INVALID, kMdfRedPv);
  int rc = multidf_check(ctx, opts, n, m, p, k, Covar, ncov);
  if (rc) return rc;
  if (!Y || !G || !K || !h2_out) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_multidf_reduced: NULL buffer");
  if ((rc = multidf_reduced_check(ctx, out))) return rc;
  HostCall hc(ctx);
  const size_t cap = out->cap > 0 ? out->cap : 1, mm = m > 0 ? m : 1;
  // device side of `out`: maxima / arg-maxima (tmpA / tmpB), triplets + count (redtrip), h2 (outH2), as blmm_bulkscan_reduced
  if ((rc = hc.begin()) || (rc = ensure(ctx, ctx->tmpA, sizeof(double) * mm)) || (rc = ensure(ctx, ctx->tmpB, sizeof(int64_t) * mm)) ||
      (rc = ensure(ctx, ctx->redtrip, (sizeof(double) + 2 * sizeof(int32_t)) * cap + 64)) || (rc = ensure(ctx, ctx->outH2, sizeof(double) * mm)))
    return rc;
  blmm_reduced d = *out;
  d.colmax = (out->colmax || out->argmax) ? ptr<double>(ctx->tmpA) : nullptr;
  d.argmax = out->argmax ? ptr<int64_t>(ctx->tmpB) : nullptr;
  d.count = ptr<int64_t>(ctx->redtrip);
  d.tlod = reinterpret_cast<double*>(d.count + 8);
  d.ti = reinterpret_cast<int32_t*>(d.tlod + cap);
  d.tj = d.ti + cap;
  HostCall::In in;
  if ((rc = hc.inputs(Y, n, m, G, p, K, Covar, ncov, weights, /*defer*/ true, &in)) ||
      (rc = multidf_reduced_run(ctx, opts, in.Y, n, m, in.G, p, k, in.Cov, in.ncov, in.K, in.W, h2_grid, ngrid, &d, ptr<double>(ctx->outH2), status)))
    return rc;
  if (m > 0 && ((rc = hc.down(out->colmax, d.colmax, sizeof(double) * m)) || (rc = hc.down(out->argmax, d.argmax, sizeof(int64_t) * m)) ||
                (rc = hc.down(h2_out, ctx->outH2.p, sizeof(double) * m)))) return rc;
  if (out->want_triplets) {
    // the count first: only what it says is copied back
    if ((rc = hc.down(out->count, d.count, sizeof(int64_t)))) return rc;
    BLMM_HIP(hipStreamSynchronize(ctx->stream));
    const size_t got = *out->count < out->cap ? *out->count : out->cap;
    if ((rc = hc.down(out->tlod, d.tlod, sizeof(double) * got)) || (rc = hc.down(out->ti, d.ti, sizeof(int32_t) * got)) ||
        (rc = hc.down(out->tj, d.tj, sizeof(int32_t) * got))) return rc;
  }
  return (rc = hc.finish()) ? rc : check_sticky(ctx);
}

// ---------------------------------------------------------------------------------------------------
// The conditional scan (include/bulklmm_hip.h: blmm_bulkscan_cond; kernels_cond.hip).  Every refusal that needs no device comes
// first, in the same order in the host and the device forms.
static int cond_check(blmm_ctx* ctx, const blmm_opts* opts, int64_t n, int64_t m, int64_t p, int64_t s, const double* Covar, int64_t ncov) {
  int rc = check_opts(ctx, opts);
  if (rc) return rc;
  if (n < 1 || m < 0 || p < 0 || ncov < 0 || s < 0 || p > 0x7fffffffLL || m > 0x7fffffffLL) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  if ((rc = check_method(ctx, opts))) return rc;
  if (opts->method == BLMM_ALT_GRID) return fail(ctx, BLMM_ERR_UNSUPPORTED, "bulkscan_cond: alt-grid is not supported; use null-grid or null-exact");
  if (s > BLMM_COND_MAX_LOCI) return fail(ctx, BLMM_ERR_UNSUPPORTED, "bulkscan_cond: at most 4 conditioning loci per trait");
  const int64_t c = null_cov(opts, Covar, ncov).c;
  if (c + s > BLMM_MULTIDF_MAX_COVARIATES)
    return fail(ctx, BLMM_ERR_UNSUPPORTED, "bulkscan_cond: more than 8 null-design columns (covariates incl. intercept + conditioning loci) are not supported");
  if (n > 2048) return fail(ctx, BLMM_ERR_UNSUPPORTED, "more than 2048 individuals: the device eigensolver (tridiagonalisation + divide and conquer) stops at n = 2048");
  if (c + s >= n) return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  return BLMM_OK;
}

static int cond_dev_impl(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                         const double* dCovar, int64_t ncov, const double* dK, const double* dweights, const double* h2_grid_host,
                         int64_t ngrid, const int64_t* dcond, int64_t s, double* dL_out, int64_t ldL, double* dh2_out,
                         int64_t* dcinfo_out, blmm_status* status, const PvReq& pvreq) {
  if (!dcond) s = 0;
  int rc = cond_check(ctx, opts, n, m, p, s, dCovar, ncov);
  if (rc) return rc;
  if (!dY || !dG || !dK || !dL_out || !dh2_out) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_cond: NULL buffer");
  if (ldL < p) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_cond: ldL < p");
  const bool exact = opts->method == BLMM_NULL_EXACT;
  if ((rc = enter_device(ctx))) return rc;
  Timer tm(ctx);
  Pipe P;
  double* dgrid = nullptr;
  if (!exact && (rc = grid_to_device(ctx, h2_grid_host, ngrid, &dgrid))) return rc;
  // blmm_bulkscan's design, eigen phase and trait rotation; the markers are rotated below without the centring projection (the
  // rank rule compares against the norm of the rotated column itself), as blmm_bulkscan_multidf does
  const bool g_in_flight = ctx->up_pending || ctx->in_wait;
  if ((rc = prepare(ctx, opts, dY, n, m, dG, p, dCovar, ncov, dK, dweights, 1, P, tm, false, false, /*skip_markers*/ true))) return rc;
  if (g_in_flight) BLMM_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_in, 0));
  const NullModel nm = null_model(P, opts);
  PvCall pvc(ctx, pvreq);
  if ((rc = pvc.resolve(p, m))) return rc;
  // work area: the info counters, then per trait the kept columns (s), r_j and the guard's flag
  const size_t mm = (size_t)(m > 0 ? m : 1);
  if ((rc = ensure(ctx, ctx->condWork, sizeof(int64_t) * COND_NINFO + sizeof(int) * mm * (size_t)(s + 2)))) return rc;
  int64_t* info = ptr<int64_t>(ctx->condWork);
  BLMM_HIP(hipMemsetAsync(info, 0, sizeof(int64_t) * COND_NINFO, ctx->stream));
  auto finish = [&]() -> int {
    if (dcinfo_out) BLMM_HIP(hipMemcpyAsync(dcinfo_out, info, sizeof(int64_t) * BLMM_COND_INFO_LEN, hipMemcpyDeviceToDevice, ctx->stream));
    int rc2 = end_call(ctx, P, status, &tm);
    if (rc2 || !status) return rc2;
    int64_t bad = 0;   // the stream has been synchronised
    BLMM_HIP(hipMemcpy(&bad, info + 4, sizeof(int64_t), hipMemcpyDeviceToHost));
    if (bad) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_cond: " + std::to_string((long long)bad) + " trait(s) with a conditioning index outside [-1, p)");
    return BLMM_OK;
  };
  if (m == 0) { tm.mark(); tm.mark(); tm.mark(); return finish(); }
  CondArgs a;
  a.n = P.n; a.c = P.c; a.s = (int)s; a.npad = P.npad; a.m = m; a.p = p;
  a.Xt = nullptr; a.ldx = P.ldx; a.Yt = P.Yt; a.ldy = P.ldy; a.Z0 = P.Z0; a.lam = P.lam; a.cond = dcond;
  a.kept = reinterpret_cast<int*>(info + COND_NINFO); a.nk = a.kept + mm * (size_t)s; a.flag = a.nk + mm;
  a.info = info; a.h2 = dh2_out; a.stat = P.stat;
  if (p > 0) {
    if ((rc = ensure(ctx, ctx->mdfR, sizeof(double) * (size_t)P.npad * P.ldr)) ||
        (rc = ensure(ctx, ctx->Xt, sizeof(double) * (size_t)P.npad * P.ldx))) return rc;
    if ((rc = launch_mdf_rawrot(ctx, ptr<double>(ctx->U), dweights, P.n, P.npad, P.ldr, ptr<double>(ctx->mdfR)))) return rc;
    P.Xt = ptr<double>(ctx->Xt);
    if ((rc = launch_rotate(ctx, ptr<double>(ctx->mdfR), P.ldr, P.n, P.npad, dG, p, P.Xt, P.ldx, P.ldx))) return rc;
    a.Xt = P.Xt;
  }
  if ((rc = launch_cond_null(ctx, nm, a, exact ? nullptr : dgrid, (int)ngrid))) return rc;
  tm.mark();
  if (p == 0) { tm.mark(); tm.mark(); return finish(); }
  const int ct = P.c + (int)s;
  const int64_t ldp = P.ldy;
  if ((rc = ensure(ctx, ctx->panels, sizeof(double) * (size_t)(2 + ct) * P.npad * ldp)) ||
      (rc = ensure(ctx, ctx->illList, sizeof(int) * mm))) return rc;
  if ((rc = launch_cond_panels(ctx, nm, a, ptr<double>(ctx->panels), ldp, ctx->tune.illcond_rho, ptr<int>(ctx->illList)))) return rc;
  tm.mark();
  ScanArgs sa = scan_args(ctx, P, ptr<double>(ctx->panels), ldp, dL_out, ldL, m);
  sa.c = ct; sa.Pv = nullptr; sa.red = RedArgs(); sa.cflag = a.flag; sa.cinfo = info;
  if ((rc = launch_scan_cond(ctx, sa, ct))) return rc;
  if ((rc = launch_cond_qr(ctx, nm, a, ptr<int>(ctx->illList), dL_out, ldL))) return rc;
  tm.mark();
  if ((rc = pvc.finish(p, m, dL_out, ldL))) return rc;
  return finish();
}

int blmm_bulkscan_cond_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                           const double* dCovar, int64_t ncov, const double* dK, const double* dweights, const double* h2_grid,
                           int64_t ngrid, const int64_t* dcond, int64_t s, double* dL_out, int64_t ldL, double* dh2_out,
                           int64_t* dcinfo_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  const PvReq pvreq = pv_take(ctx);
  ctx->red_cur = RedArgs();
  return cond_dev_impl(ctx, opts, dY, n, m, dG, p, dCovar, ncov, dK, dweights, h2_grid, ngrid, dcond, s, dL_out, ldL, dh2_out, dcinfo_out,
                       status, pvreq);
}

// L_out == NULL: L (p x m) stays resident for the blmm_last_* consumers, as blmm_bulkscan
int blmm_bulkscan_cond(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                       const double* Covar, int64_t ncov, const double* K, const double* weights, const double* h2_grid,
                       int64_t ngrid, const int64_t* cond, int64_t s, double* L_out, double* h2_out, int64_t* cinfo_out,
                       blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  const PvReq pvreq = pv_take(ctx);
  if (!cond) s = 0;
  int rc = cond_check(ctx, opts, n, m, p, s, Covar, ncov);
  if (rc) return rc;
  if (!Y || !G || !K || !h2_out) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_cond: NULL buffer");
  for (int64_t e = 0; e < s * m; ++e)
    if (cond[e] < -1 || cond[e] >= p)
      return fail(ctx, BLMM_ERR_INVALID, "bulkscan_cond: trait " + std::to_string((long long)(e / s)) + " has a conditioning index outside [-1, p)");
  HostCall hc(ctx);
  const size_t mm = (size_t)(m > 0 ? m : 1);
  if ((rc = hc.begin()) || (rc = ensure(ctx, ctx->outL, sizeof(double) * (size_t)(p > 0 ? p : 1) * mm)) ||
      (rc = ensure(ctx, ctx->outH2, sizeof(double) * mm)))
    return rc;
  const int64_t* dcond = nullptr;
  if (s > 0 && m > 0) {
    if ((rc = hc.up(ctx->condIdx, cond, sizeof(int64_t) * (size_t)s * (size_t)m))) return rc;
    dcond = ptr<int64_t>(ctx->condIdx);
  } else s = 0;
  HostCall::In d;
  if ((rc = hc.inputs(Y, n, m, G, p, K, Covar, ncov, weights, /*defer*/ true, &d))) return rc;
  ctx->red_cur = RedArgs();
  if ((rc = cond_dev_impl(ctx, opts, d.Y, n, m, d.G, p, d.Cov, d.ncov, d.K, d.W, h2_grid, ngrid, dcond, s, ptr<double>(ctx->outL),
                          p > 0 ? p : 1, ptr<double>(ctx->outH2), nullptr, status, pvreq))) return rc;
  set_last(ctx, ptr<double>(ctx->outL), p, m);
  if (L_out && (size_t)p * m > 0 && (rc = copy_to_host(ctx, L_out, ctx->outL.p, sizeof(double) * (size_t)p * m))) return rc;
  if (m > 0 && (rc = copy_to_host(ctx, h2_out, ctx->outH2.p, sizeof(double) * (size_t)m))) return rc;
  if ((rc = hc.down(cinfo_out, ctx->condWork.p, sizeof(int64_t) * BLMM_COND_INFO_LEN))) return rc;
  if ((rc = hc.finish())) return rc;
  return check_sticky(ctx);
}

// ---------------------------------------------------------------------------------------------------
// Forward selection of up to max_loci loci per trait (include/bulklmm_hip.h: blmm_bulkscan_stepwise): the rounds of
// blmm_bulkscan_cond on one upload, one eigen phase and one pair of rotations, every round reduced to its column maxima in the scan's
// epilogue (no p x m buffer) and run on the traits still active.  Refusals first, in the same order in both forms.
static int stepwise_check(blmm_ctx* ctx, const blmm_opts* opts, int64_t n, int64_t m, int64_t p, int64_t S, double thr, const double* Covar,
                          int64_t ncov) {
  int rc = check_opts(ctx, opts);
  if (rc) return rc;
  if (S < 1) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_stepwise: max_loci must be at least 1");
  if (S > BLMM_COND_MAX_LOCI) return fail(ctx, BLMM_ERR_UNSUPPORTED, "bulkscan_stepwise: at most 4 loci per trait");
  if (ncov >= 0 && null_cov(opts, Covar, ncov).c + S > BLMM_MULTIDF_MAX_COVARIATES)
    return fail(ctx, BLMM_ERR_UNSUPPORTED, "bulkscan_stepwise: more than 8 null-design columns (covariates incl. intercept + max_loci) are not supported");
  if (!(thr >= 0.0)) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_stepwise: the threshold must be a number >= 0");
  return cond_check(ctx, opts, n, m, p, S, Covar, ncov);
}
static const char* const kStepPv = "bulkscan_stepwise: a blmm_set_log10p_output request is pending (the call writes no matrix)";

// The guard's list of one round (columns of the active list), behind the reducing scan and k_red_final: k_cond_qr<RED> recomputes a
// chunk of the listed columns into the scratch and k_mdf_flag_red reduces them over the (-inf, -1) the scan left.  The length of the
// list stays on the device: every chunk the round's nact columns could fill is launched, and the kernels of a chunk beyond the list
// return at once, so the round waits for the stream only once (for the next round's size).
static int stepwise_flagged(blmm_ctx* ctx, const NullModel& nm, const CondArgs& a, double* mx, int64_t* arg) {
  int64_t chunk = ctx->tune.cond_red_chunk > 0 ? ctx->tune.cond_red_chunk : (int64_t)(64ll << 20) / (int64_t)(sizeof(double) * (size_t)a.p);
  chunk = std::min(std::max<int64_t>(chunk, 1), a.m);
  int rc = ensure(ctx, ctx->condScr, sizeof(double) * (size_t)a.p * (size_t)chunk);
  if (rc) return rc;
  double* scr = ptr<double>(ctx->condScr);
  for (int64_t item0 = 0; item0 < a.m; item0 += chunk) {
    const int64_t nitem = std::min(chunk, a.m - item0);
    if ((rc = launch_cond_qr(ctx, nm, a, ptr<int>(ctx->illList), nullptr, 0, scr, item0, nitem)) ||
        (rc = launch_mdf_flag_red(ctx, scr, a.p, ptr<int>(ctx->illList), a.stat, item0, nitem, mx, arg, RedArgs()))) return rc;
  }
  return BLMM_OK;
}

static int stepwise_dev_impl(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                             const double* dCovar, int64_t ncov, const double* dK, const double* dweights, const double* h2_grid_host,
                             int64_t ngrid, int64_t S, double thr, int64_t* dloci, double* dlod, int64_t* darg, double* dh2,
                             int64_t* dnloci, int64_t* dsinfo, blmm_status* status) {
  int rc = stepwise_check(ctx, opts, n, m, p, S, thr, dCovar, ncov);
  if (rc) return rc;
  if (!dY || !dG || !dK || !dloci || !dlod || !darg || !dh2 || !dnloci) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_stepwise: NULL buffer");
  const bool exact = opts->method == BLMM_NULL_EXACT;
  if ((rc = enter_device(ctx))) return rc;
  Timer tm(ctx);
  Pipe P;
  double* dgrid = nullptr;
  if (!exact && (rc = grid_to_device(ctx, h2_grid_host, ngrid, &dgrid))) return rc;
  // blmm_bulkscan_cond's front, once
  const bool g_in_flight = ctx->up_pending || ctx->in_wait;
  if ((rc = prepare(ctx, opts, dY, n, m, dG, p, dCovar, ncov, dK, dweights, 1, P, tm, false, false, /*skip_markers*/ true))) return rc;
  if (g_in_flight) BLMM_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_in, 0));
  const NullModel nm = null_model(P, opts);
  // work areas.  condWork as blmm_bulkscan_cond's (per COLUMN here); stepWork: 8 counters, then per column the round's arg-maximum,
  // h2 and maximum, then the two lists
  const size_t mm = (size_t)(m > 0 ? m : 1);
  if ((rc = ensure(ctx, ctx->condWork, sizeof(int64_t) * COND_NINFO + sizeof(int) * mm * (size_t)(S + 2))) ||
      (rc = ensure(ctx, ctx->stepWork, sizeof(int64_t) * 8 + (sizeof(int64_t) + 2 * sizeof(double) + 2 * sizeof(int)) * mm))) return rc;
  int64_t* info = ptr<int64_t>(ctx->condWork);
  int64_t* w = ptr<int64_t>(ctx->stepWork);
  int64_t* argc = w + 8;
  double* h2c = reinterpret_cast<double*>(argc + mm);
  double* mxc = h2c + mm;
  int* lists[2] = {reinterpret_cast<int*>(mxc + mm), reinterpret_cast<int*>(mxc + mm) + mm};
  BLMM_HIP(hipMemsetAsync(info, 0, sizeof(int64_t) * COND_NINFO, ctx->stream));
  BLMM_HIP(hipMemsetAsync(w, 0, sizeof(int64_t) * 8, ctx->stream));
  StepArgs st;
  st.S = (int)S; st.m = m; st.thr = thr; st.loci = dloci; st.lod = dlod; st.arg = darg; st.h2 = dh2; st.nloci = dnloci; st.w = w;
  StepRounds sr = {};
  if ((rc = launch_step_init(ctx, st))) return rc;
  CondArgs a;
  a.n = P.n; a.c = P.c; a.s = (int)S; a.npad = P.npad; a.m = m; a.p = p;
  a.Xt = nullptr; a.ldx = P.ldx; a.Yt = P.Yt; a.ldy = P.ldy; a.Z0 = P.Z0; a.lam = P.lam; a.cond = dloci;
  a.kept = reinterpret_cast<int*>(info + COND_NINFO); a.nk = a.kept + mm * (size_t)S; a.flag = a.nk + mm;
  a.info = info; a.h2 = h2c; a.stat = P.stat;
  const int ct = P.c + (int)S;
  const int nslot = 2 * (int)((p + 127) / 128);
  RedArgs r;
  if (m > 0 && p > 0) {
    if ((rc = ensure(ctx, ctx->mdfR, sizeof(double) * (size_t)P.npad * P.ldr)) ||
        (rc = ensure(ctx, ctx->Xt, sizeof(double) * (size_t)P.npad * P.ldx))) return rc;
    if ((rc = launch_mdf_rawrot(ctx, ptr<double>(ctx->U), dweights, P.n, P.npad, P.ldr, ptr<double>(ctx->mdfR)))) return rc;
    P.Xt = ptr<double>(ctx->Xt);
    if ((rc = launch_rotate(ctx, ptr<double>(ctx->mdfR), P.ldr, P.n, P.npad, dG, p, P.Xt, P.ldx, P.ldx))) return rc;
    a.Xt = P.Xt;
    r.ldm = round_up(m, 64);
    if ((rc = ensure(ctx, ctx->redbuf, (sizeof(double) + sizeof(int)) * (size_t)nslot * (size_t)r.ldm)) ||
        (rc = ensure(ctx, ctx->panels, sizeof(double) * (size_t)(2 + ct) * P.npad * P.ldy)) ||
        (rc = ensure(ctx, ctx->illList, sizeof(int) * mm))) return rc;
    r.pmax = ptr<double>(ctx->redbuf); r.parg = reinterpret_cast<int*>(r.pmax + (size_t)nslot * r.ldm);
  }
  // the rounds: every one on the list the round before left; the design is c + S columns wide in all of them (absent loci are zero
  // panels), which is what blmm_bulkscan_cond runs at s = S
  int64_t nact = m;
  for (int t = 0; t <= (int)S && nact > 0; ++t) {
    sr.nact[t] = nact; sr.rounds = t + 1;
    a.m = nact; a.act = t == 0 ? nullptr : lists[t & 1];
    if ((rc = launch_cond_null(ctx, nm, a, exact ? nullptr : dgrid, (int)ngrid))) return rc;
    if (t == 0) tm.mark();
    if (p > 0) {
      const int64_t ldp = round_up(nact, 128);
      if ((rc = launch_cond_panels(ctx, nm, a, ptr<double>(ctx->panels), ldp, ctx->tune.illcond_rho, ptr<int>(ctx->illList)))) return rc;
      if (t == 0) tm.mark();
      ScanArgs sa = scan_args(ctx, P, ptr<double>(ctx->panels), ldp, nullptr, 0, nact);
      sa.c = ct; sa.Pv = nullptr; sa.red = r; sa.cflag = a.flag; sa.cinfo = info;
      if ((rc = launch_scan_cond(ctx, sa, ct))) return rc;
    } else if (t == 0) tm.mark();
    if ((rc = launch_red_final(ctx, r, p > 0 ? nslot : 0, nact, mxc, argc))) return rc;
    if (p > 0 && P.c + t >= 2 && (rc = stepwise_flagged(ctx, nm, a, mxc, argc))) return rc;   // a design of >= 2 columns exists
    if ((rc = launch_step_update(ctx, st, t, nact, a.act, lists[(t + 1) & 1], mxc, argc, h2c, P.stat))) return rc;
    if (t == (int)S) break;
    BLMM_HIP(hipMemcpyAsync(&nact, w, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    BLMM_HIP(hipStreamSynchronize(ctx->stream));
  }
  if (m == 0) { tm.mark(); tm.mark(); }
  tm.mark();
  if ((rc = launch_step_finish(ctx, st, sr, info, P.stat, dsinfo))) return rc;
  return end_call(ctx, P, status, &tm);
}

int blmm_bulkscan_stepwise_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                               const double* dCovar, int64_t ncov, const double* dK, const double* dweights, const double* h2_grid,
                               int64_t ngrid, int64_t max_loci, double threshold, int64_t* dloci_out, double* dlod_out,
                               int64_t* dargmax_out, double* dh2_out, int64_t* dnloci_out, int64_t* dsinfo_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (pv_take(ctx).armed) return fail(ctx, BLMM_ERR_INVALID, kStepPv);
  ctx->red_cur = RedArgs();
  int rc = stepwise_dev_impl(ctx, opts, dY, n, m, dG, p, dCovar, ncov, dK, dweights, h2_grid, ngrid, max_loci, threshold, dloci_out,
                             dlod_out, dargmax_out, dh2_out, dnloci_out, dsinfo_out, status);
  if (rc) return rc;
  clear_last(ctx);                          // no matrix of this call: an earlier one is not served as its result
  return BLMM_OK;
}

int blmm_bulkscan_stepwise(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                           const double* Covar, int64_t ncov, const double* K, const double* weights, const double* h2_grid,
                           int64_t ngrid, int64_t max_loci, double threshold, int64_t* loci_out, double* lod_out, int64_t* argmax_out,
                           double* h2_out, int64_t* nloci_out, int64_t* sinfo_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  if (pv_take(ctx).armed) return fail(ctx, BLMM_ERR_INVALID, kStepPv);
  int rc = stepwise_check(ctx, opts, n, m, p, max_loci, threshold, Covar, ncov);
  if (rc) return rc;
  if (!Y || !G || !K || !loci_out || !lod_out || !argmax_out || !h2_out || !nloci_out) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_stepwise: NULL buffer");
  HostCall hc(ctx);
  // device side of the outputs: int64 loci (S m), argmax ((S + 1) m), nloci (m), sinfo; double lod, h2 ((S + 1) m each)
  const size_t mm = (size_t)(m > 0 ? m : 1), S = (size_t)max_loci, um = (size_t)m;
  if ((rc = hc.begin()) || (rc = ensure(ctx, ctx->stepOut, sizeof(int64_t) * (mm * (2 * S + 2) + BLMM_STEP_INFO_LEN) + sizeof(double) * 2 * (S + 1) * mm)))
    return rc;
  int64_t* dloci = ptr<int64_t>(ctx->stepOut);
  int64_t* darg = dloci + S * mm;
  int64_t* dnloci = darg + (S + 1) * mm;
  int64_t* dsinfo = dnloci + mm;
  double* dlod = reinterpret_cast<double*>(dsinfo + BLMM_STEP_INFO_LEN);
  double* dh2 = dlod + (S + 1) * mm;
  HostCall::In d;
  if ((rc = hc.inputs(Y, n, m, G, p, K, Covar, ncov, weights, /*defer*/ true, &d))) return rc;
  ctx->red_cur = RedArgs();
  if ((rc = stepwise_dev_impl(ctx, opts, d.Y, n, m, d.G, p, d.Cov, d.ncov, d.K, d.W, h2_grid, ngrid, max_loci, threshold, dloci, dlod,
                              darg, dh2, dnloci, dsinfo, status))) return rc;
  clear_last(ctx);
  if (m > 0 && ((rc = hc.down(loci_out, dloci, sizeof(int64_t) * S * um)) || (rc = hc.down(lod_out, dlod, sizeof(double) * (S + 1) * um)) ||
                (rc = hc.down(argmax_out, darg, sizeof(int64_t) * (S + 1) * um)) || (rc = hc.down(h2_out, dh2, sizeof(double) * (S + 1) * um)) ||
                (rc = hc.down(nloci_out, dnloci, sizeof(int64_t) * um)))) return rc;
  if ((rc = hc.down(sinfo_out, dsinfo, sizeof(int64_t) * BLMM_STEP_INFO_LEN))) return rc;
  return (rc = hc.finish()) ? rc : check_sticky(ctx);
}

// ---------------------------------------------------------------------------------------------------
// Coefficients and standard errors at a list of tests (include/bulklmm_hip.h: blmm_bulkscan_effects; kernels_effects.hip).  The
// refusals that need no device come first, in the same order in the host and the device forms (multidf_check's, with k up to
// BLMM_EFFECTS_MAX_K for both methods).
static int effects_check(blmm_ctx* ctx, const blmm_opts* opts, int64_t n, int64_t m, int64_t p, int64_t k, const double* Covar,
                         int64_t ncov, int64_t T) {
  int rc = check_opts(ctx, opts);
  if (rc) return rc;
  if (n < 1 || m < 0 || p < 0 || ncov < 0 || T < 0 || p > 0x7fffffffLL || m > 0x7ffffff0LL || T > 0x7fffffffLL)
    return fail(ctx, BLMM_ERR_DIM, "Dimension mismatch.");
  if (k < 1 || p % k != 0) return fail(ctx, BLMM_ERR_DIM, "bulkscan_effects: the number of columns of G must be a multiple of k >= 1");
  if ((rc = check_method(ctx, opts))) return rc;
  if (opts->method == BLMM_ALT_GRID) return fail(ctx, BLMM_ERR_UNSUPPORTED, "bulkscan_effects: alt-grid is not supported; use null-grid or null-exact");
  if (k > BLMM_EFFECTS_MAX_K) return fail(ctx, BLMM_ERR_UNSUPPORTED, "bulkscan_effects: takes 1 <= k <= " + std::to_string(BLMM_EFFECTS_MAX_K));
  if (null_cov(opts, Covar, ncov).c > BLMM_MULTIDF_MAX_COVARIATES)
    return fail(ctx, BLMM_ERR_UNSUPPORTED, "bulkscan_effects: more than 8 null covariates (incl. intercept) are not supported");
  if (n > 2048) return fail(ctx, BLMM_ERR_UNSUPPORTED, "more than 2048 individuals: the device eigensolver (tridiagonalisation + divide and conquer) stops at n = 2048");
  return BLMM_OK;
}

static int effects_dev_impl(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                            int64_t k, const double* dCovar, int64_t ncov, const double* dK, const double* dweights,
                            const double* h2_grid_host, int64_t ngrid, const int64_t* dlocus, const int64_t* dtrait, int64_t T,
                            double* dbeta, double* dse, double* dsigma2, double* dlod, int32_t* dacc, double* dh2_out,
                            blmm_status* status) {
  int rc = effects_check(ctx, opts, n, m, p, k, dCovar, ncov, T);
  if (rc) return rc;
  const int64_t nloci = p / k;
  if (!dY || !dG || !dK || !dh2_out || (T > 0 && (!dlocus || !dtrait || !dbeta || !dse || !dsigma2 || !dlod || !dacc)))
    return fail(ctx, BLMM_ERR_INVALID, "bulkscan_effects: NULL buffer");
  const bool exact = opts->method == BLMM_NULL_EXACT;
  if ((rc = enter_device(ctx))) return rc;
  Timer tm(ctx);
  Pipe P;
  double* dgrid = nullptr;
  if (!exact && (rc = grid_to_device(ctx, h2_grid_host, ngrid, &dgrid))) return rc;
  // blmm_bulkscan's design, eigen phase and trait rotation (the null model is its own, bit for bit), as blmm_bulkscan_multidf
  const bool g_in_flight = ctx->up_pending || ctx->in_wait;
  if ((rc = prepare(ctx, opts, dY, n, m, dG, p, dCovar, ncov, dK, dweights, 1, P, tm, false, false, /*skip_markers*/ true))) return rc;
  if (g_in_flight) BLMM_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_in, 0));
  const NullModel nm = null_model(P, opts);
  if (m == 0) { tm.mark(); tm.mark(); tm.mark(); return end_call(ctx, P, status, &tm); }
  if (exact) {
    if ((rc = launch_brent(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, dh2_out, nullptr, nullptr, P.stat))) return rc;
  } else {
    if ((rc = ensure(ctx, ctx->h2idx, sizeof(int) * (size_t)m))) return rc;
    if ((rc = launch_loglik_grid(ctx, nm, P.Yt, P.ldy, m, P.Z0, P.lam, dgrid, (int)ngrid, nullptr, ptr<int>(ctx->h2idx), dh2_out, P.stat))) return rc;
  }
  tm.mark();
  if (T == 0 || nloci == 0) {   // (nloci == 0 with T > 0: every index is out of range; the host form has refused it)
    tm.mark(); tm.mark();
    if (T > 0) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_effects: a locus index is out of range (G has no columns)");
    return end_call(ctx, P, status, &tm);
  }
  // the uncentred rotation of every marker (blmm_bulkscan_multidf's), then column-major: a test's k columns are k n contiguous doubles
  if ((rc = ensure(ctx, ctx->mdfR, sizeof(double) * (size_t)P.npad * P.ldr)) ||
      (rc = ensure(ctx, ctx->Xt, sizeof(double) * (size_t)P.npad * P.ldx)) ||
      (rc = ensure(ctx, ctx->effX, sizeof(double) * (size_t)P.n * (size_t)p)) ||
      (rc = ensure(ctx, ctx->effWork, sizeof(int) * (size_t)(m + 2 + T)))) return rc;
  if ((rc = launch_mdf_rawrot(ctx, ptr<double>(ctx->U), dweights, P.n, P.npad, P.ldr, ptr<double>(ctx->mdfR)))) return rc;
  P.Xt = ptr<double>(ctx->Xt);
  if ((rc = launch_rotate(ctx, ptr<double>(ctx->mdfR), P.ldr, P.n, P.npad, dG, p, P.Xt, P.ldx, P.ldx))) return rc;
  if ((rc = launch_untranspose(ctx, P.Xt, P.ldx, P.n, p, ptr<double>(ctx->effX)))) return rc;
  EffArgs a;
  a.n = P.n; a.c = P.c; a.k = (int)k; a.m = m; a.nloci = nloci; a.T = T;
  a.Xc = ptr<double>(ctx->effX); a.Yt = P.Yt; a.ldy = P.ldy; a.Z0 = P.Z0; a.lam = P.lam; a.h2 = dh2_out;
  a.locus = dlocus; a.trait = dtrait; a.cnt = ptr<int>(ctx->effWork); a.order = a.cnt + (m + 2);
  a.reml = nm.reml; a.prior_a = nm.prior_a; a.prior_b = nm.prior_b;
  a.beta = dbeta; a.se = dse; a.sigma2 = dsigma2; a.lod = dlod; a.accepted = dacc; a.stat = P.stat;
  a.slab = nullptr; a.chunk = 1;
  if ((rc = launch_effects_sort(ctx, a))) return rc;
  tm.mark();
  if ((rc = launch_effects(ctx, a))) return rc;
  tm.mark();
  if ((rc = end_call(ctx, P, status, &tm))) return rc;
  if (status) {   // the stream has been synchronised: tests out of range (their outputs are NaN / accepted = -1) are an error
    int bad = 0;
    BLMM_HIP(hipMemcpy(&bad, a.cnt + m + 1, sizeof(int), hipMemcpyDeviceToHost));
    if (bad) return fail(ctx, BLMM_ERR_INVALID, "bulkscan_effects: " + std::to_string(bad) + " test(s) with a locus or trait index out of range");
  }
  return BLMM_OK;
}

int blmm_bulkscan_effects_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG,
                              int64_t p, int64_t k, const double* dCovar, int64_t ncov, const double* dK, const double* dweights,
                              const double* h2_grid, int64_t ngrid, const int64_t* dlocus, const int64_t* dtrait, int64_t ntests,
                              double* dbeta_out, double* dse_out, double* dsigma2_out, double* dlod_out, int32_t* daccepted_out,
                              double* dh2_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  (void)pv_take(ctx);   // a pending -log10 p request does not apply to this call: disarmed, as by every entry point
  ctx->red_cur = RedArgs();
  return effects_dev_impl(ctx, opts, dY, n, m, dG, p, k, dCovar, ncov, dK, dweights, h2_grid, ngrid, dlocus, dtrait, ntests, dbeta_out,
                          dse_out, dsigma2_out, dlod_out, daccepted_out, dh2_out, status);
}

int blmm_bulkscan_effects(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                          int64_t k, const double* Covar, int64_t ncov, const double* K, const double* weights,
                          const double* h2_grid, int64_t ngrid, const int64_t* locus, const int64_t* trait, int64_t ntests,
                          double* beta_out, double* se_out, double* sigma2_out, double* lod_out, int32_t* accepted_out,
                          double* h2_out, blmm_status* status) {
  if (!ctx) return BLMM_ERR_INVALID;
  (void)pv_take(ctx);
  const int64_t T = ntests;
  int rc = effects_check(ctx, opts, n, m, p, k, Covar, ncov, T);
  if (rc) return rc;
  if (!Y || !G || !K || !h2_out || (T > 0 && (!locus || !trait || !beta_out || !se_out || !sigma2_out || !lod_out || !accepted_out)))
    return fail(ctx, BLMM_ERR_INVALID, "bulkscan_effects: NULL buffer");
  const int64_t nloci = p / k;
  for (int64_t t = 0; t < T; ++t)
    if (locus[t] < 0 || locus[t] >= nloci || trait[t] < 0 || trait[t] >= m)
      return fail(ctx, BLMM_ERR_INVALID, "bulkscan_effects: test " + std::to_string((long long)t) + " has a locus or trait index out of range");
  HostCall hc(ctx);
  const size_t Tn = (size_t)(T > 0 ? T : 1);
  // outputs in one block: beta, se (T k each), sigma2, lod (T each), accepted (T int32)
  if ((rc = hc.begin()) || (rc = ensure(ctx, ctx->effOut, sizeof(double) * Tn * (size_t)(2 * k + 2) + sizeof(int32_t) * Tn)) ||
      (rc = ensure(ctx, ctx->effIdx, sizeof(int64_t) * 2 * Tn)) || (rc = ensure(ctx, ctx->outH2, sizeof(double) * (size_t)(m > 0 ? m : 1))))
    return rc;
  int64_t* dloc = ptr<int64_t>(ctx->effIdx);
  int64_t* dtr = dloc + Tn;
  if (T > 0 && ((rc = hc.up(dloc, locus, sizeof(int64_t) * (size_t)T)) || (rc = hc.up(dtr, trait, sizeof(int64_t) * (size_t)T)))) return rc;
  HostCall::In d;
  if ((rc = hc.inputs(Y, n, m, G, p, K, Covar, ncov, weights, /*defer*/ true, &d))) return rc;
  ctx->red_cur = RedArgs();
  double* dbeta = ptr<double>(ctx->effOut);
  double* dse = dbeta + Tn * (size_t)k;
  double* dsig = dse + Tn * (size_t)k;
  double* dlod = dsig + Tn;
  int32_t* dacc = reinterpret_cast<int32_t*>(dlod + Tn);
  if ((rc = effects_dev_impl(ctx, opts, d.Y, n, m, d.G, p, k, d.Cov, d.ncov, d.K, d.W, h2_grid, ngrid, dloc, dtr, T, dbeta, dse, dsig, dlod,
                             dacc, ptr<double>(ctx->outH2), status))) return rc;
  if (T > 0 && m > 0 &&
      ((rc = copy_to_host(ctx, beta_out, dbeta, sizeof(double) * (size_t)T * k)) || (rc = copy_to_host(ctx, se_out, dse, sizeof(double) * (size_t)T * k)) ||
       (rc = copy_to_host(ctx, sigma2_out, dsig, sizeof(double) * (size_t)T)) || (rc = copy_to_host(ctx, lod_out, dlod, sizeof(double) * (size_t)T)) ||
       (rc = copy_to_host(ctx, accepted_out, dacc, sizeof(int32_t) * (size_t)T)))) return rc;
  if (m > 0 && (rc = copy_to_host(ctx, h2_out, ctx->outH2.p, sizeof(double) * (size_t)m))) return rc;
  if ((rc = hc.finish())) return rc;
  return check_sticky(ctx);
}

}  // extern "C"
