// Internal declarations shared by the HIP translation units of libbulklmm_hip.so.
// Not part of the public ABI (that is include/bulklmm_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "../../include/bulklmm_hip.h"

namespace blmm {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int CMAX = 32;         // null covariates (incl. intercept) the library takes: 1 .. CTPL through kernels that are templates over c,
constexpr int CTPL = 8;          // CTPL + 1 .. CMAX through the run-time-c kernels of kernels_dyn.hip (the reference has no cap: src/wls.jl:27-60)
constexpr int CFAST = 4;         // ... with the tuned forms (LDS-resident evaluators, single-pass exact scan); beyond: the generic evaluators and a covariate-chunked scan
#define BLMM_C_ERR "number of null covariates (incl. intercept) must be 1..32"
// one `case C: M(C); break;` per instantiated covariate count (1 .. CTPL)
#define BLMM_FOR_EACH_C(M) \
  case 1: M(1); break; case 2: M(2); break; case 3: M(3); break; case 4: M(4); break; \
  case 5: M(5); break; case 6: M(6); break; case 7: M(7); break; case 8: M(8); break;
constexpr int TILE_T = 64;       // traits per workgroup tile of the scan kernels
constexpr int TILE_I = 128;      // markers per workgroup tile of the scan kernels
constexpr int NSTAT = 64;        // device status counters ([24 + 20 r ..]: per panel region r, 8 counts of traits per weight-basis segment and the 9 placement cursors of k_lr_classify)

enum StatIdx { ST_NEG_EIG = 0, ST_NONPOS_W = 1, ST_ZERO_NORM = 2, ST_NAN_LOD = 3, ST_BRENT_MAXIT = 4, ST_JACOBI_SWEEPS = 5,
               ST_EIG_CYCLES = 6, ST_EIG_TICKS = 7 /* the eigensolver's shader cycles / 100 MHz ticks */,
               ST_LR_RANK = 8 /* weight-basis rank (< 0: the multi-workgroup basis kernel timed out) */,
               ST_LR_RESID2 = 9 /* its largest squared residual, bits of a double */, ST_LR_FIX = 10 /* traits re-scanned full rank */,
               ST_EIG_ABORT = 11 /* eigensolver abort code */,
               ST_LR_SHARED0 = 12, ST_LR_OTHER0 = 13, ST_LR_SHARED1 = 14, ST_LR_OTHER1 = 15
               /* per panel region (k_lr_classify): its shared-weights traits, the columns of the other class */,
               ST_H2_BOUNDARY = 16, ST_H2_MULTIMODAL = 17, ST_ILLCOND = 18,
               ST_EIG_FAST = 19 /* 1: the fast eigen path ran */, ST_EIG_BAD = 20 /* its largest check / bound, bits of a double: accepted up to 1.0 */,
               ST_BRENT_CNT = 21 /* [21..22]: hand-over counter of the split h2 search (kernels_prep.hip: launch_brent_t) */,
               ST_EIG_DONE = 23 /* workgroups of k_jacobi_lds that have finished (the last one does the post-eigen work) */ };

inline int64_t round_up(int64_t x, int64_t q) { return (x + q - 1) / q * q; }

// BLMM_* environment switches are DEVELOPER switches (A/B timing, diagnostics): the library reads them only when BLMM_DEV_ENV=1 is
// set as well, so that a caller's environment can never silently select another code path.  What changes the arithmetic of a
// result is a property of the context instead: blmm_set_tuning (include/bulklmm_hip.h); under BLMM_DEV_ENV=1 the old variable
// names still override it (tools/*.sh).
inline const char* dev_env(const char* name) {
  const char* on = getenv("BLMM_DEV_ENV");
  return (on && on[0] == '1') ? getenv(name) : nullptr;
}
// blmm_set_tuning / blmm_get_tuning (keys = the field names)
struct Tuning {
  double lr_tol = 1e-13;        // residual |w - QQ'w| / |w| above which a trait's column is re-scanned full rank; tolerance of the shared-weights class (0: every trait flagged, class empty)
  double illcond_rho = 1e-4;    // pivot-share threshold of the conditioning guard (0: off; 2: every trait with c >= 2 re-scanned)
  int exact_full_rank = 0;      // 1: null-exact through the full-rank kernel k_scan<NX = 1 + c> instead of the low-rank weights form
  int pval_libm = 0;            // 1: -log10 p through erfc / erfcx / log instead of the bucketed polynomials (df = 1)
  int pval_fused = 1;           // 0: output_pvals as a column pass over the finished L instead of the scan epilogues
  int lr_segments = 0;          // 0: default (six segments of the heritability axis for n <= 80); 1: one weight basis; 2..8: that many equal segments
  int lr_shared = 1;            // 0: no shared-weights class (every trait through the rank-R form)
  int lr_split = -1;            // -1: split the h2 search into two panel regions from 8192 traits on; 0 / 1: never / always
  int f32_rotation = 1;         // fp32 permutation path (blmm_scan_perms_f32, c <= 3): 1 = rotate G on the fp32 matrix cores straight into k_scan_f32's operand layout; 0 = fp64 rotation + conversion (round 3)
  int eigen_solver = 0;         // 0: by n (fast path + Jacobi up to 124, tridiagonalisation + divide and conquer beyond); 1: Jacobi; 2: divide and conquer
  int mdf_red_chunk = 0;        // blmm_bulkscan_multidf_reduced: flagged traits re-scanned per chunk of the scratch; 0: from a 64 MiB budget
  int cond_red_chunk = 0;       // blmm_bulkscan_stepwise: the same for the conditional scan's flagged traits
  int bulk_perm_cols = 0;       // blmm_bulkscan_perms: largest trait chunk in panel columns (traits x (nperms + 1)); 0: from the memory budget
};

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
};

// What the stages of a call hand to one another: shapes, the rotated operands and the null model's rotated covariates.
struct Pipe {
  int n = 0, c = 0, npad = 0, ldr = 0;
  int64_t m = 0, p = 0, ldy = 0, ldx = 0;
  double *Yt = nullptr, *Xt = nullptr, *Z0 = nullptr, *lam = nullptr;
  int64_t* stat = nullptr;
  bool big = false;                // n beyond the LDS Jacobi: the call ends with k_sticky
  bool xt_side = false;            // the marker rotation was enqueued on the side stream (in front of the weight basis): Xt is ordered there
  const double* fuseY = nullptr;   // prepare() left the traits' rotation to the h2 search's kernel (BrentRot): the caller's Y, Yt not written yet
};

// Reduce-in-epilogue output of the scan kernels (blmm_bulkscan_reduced; SURVEY.md N1: "the matrix never has to leave HBM" -- here
// it is never WRITTEN): instead of a lane's four LODs of one trait going to L, the 16 lanes of the MFMA row reduce them to the
// trait's (maximum, marker) over the wave's 64 markers -> pmax / parg [slot = first marker / 64][ldm], finished by k_red_final;
// and every LOD > thr becomes a (marker, trait, LOD) triplet behind a device counter.  Same values, same tie rule (lowest marker)
// and same NaN rule (never the maximum, never > thr) as k_colmax / k_threshold on a stored L: the results are bit-identical.
struct RedArgs {
  double* pmax = nullptr; int* parg = nullptr; int64_t ldm = 0;
  int want_trip = 0; double thr = 0.0; int64_t cap = 0;
  int32_t* ti = nullptr; int32_t* tj = nullptr; double* tl = nullptr; unsigned long long* cnt = nullptr;
  // blmm_bulkscan_reduced_async: per-trait guard flags (bit 0: the weight-basis residual guard, bit 1: the conditioning guard).
  // Non-null: the re-scan kernels (k_scan_fix, k_scan_qr) patch the flagged traits' partials and append their triplets on the
  // device, and the scan epilogues append none for a flagged trait (the guards have run before them when triplets are wanted).
  int* flags = nullptr;
  // the rows this scan's markers are in the caller's result (blmm_bulkscan_loco_reduced: the chromosome's first marker), added to
  // the marker index of every triplet appended; 0 elsewhere.  The slot partials keep the scan's own marker index.
  int64_t row0 = 0;
};
}  // namespace blmm

namespace blmm { struct HostStage; }

struct blmm_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  bool timing = false;
  std::string err;
  // grow-only workspace
  blmm::DevBuf Ks, V, lam, U, Zs, Z0, Rp, Yt, Xt, panels, iyy, h2, h2idx, sig2, ell, isx, stat, gridd, misc, EllTab,
      inY, inG, inK, inCov, inW, outL, outH2, tmpA, tmpB, tmpC, perm, r0, altbuf, logtab, lraw, wbQ, wbW, wbRk, lrT, lrC, lrL, lrFlag, lrPart, lrPerm, lrDen0, eigW, xf32, pf32, brSt, brList, illList, qrSlab, lodtab, dynFac, pvtab, outP, redbuf, redtrip, altC, rf32, btG, redflag, bperm,
      locoK, locoPart, locoChr, locoStat, locoKs, locoV, locoLraw,   // blmm_kinship_loco / blmm_bulkscan_loco (kernels_loco.hip)
      locoCmx, locoCarg,   // blmm_bulkscan_loco_reduced: the per-chromosome maxima / arg-maxima when the caller's tables are not on the device
      locoPerm,            // blmm_bulkscan_loco_perms: the genome-wide (nperms + 1) x m column maxima and their global markers
      mdfR, mdfT,          // blmm_bulkscan_multidf: the uncentred rotation and the null-grid factor table (kernels_mdf.hip)
      mdfScr,              // blmm_bulkscan_multidf_reduced: the flagged traits' columns, a chunk of the guard's list wide
      condIdx, condWork,   // blmm_bulkscan_cond (kernels_cond.hip): the host form's index table; kept columns, counts, guard flags, info counters
      stepWork, stepOut, condScr,   // blmm_bulkscan_stepwise: per-column results, the two lists, counters; the host form's tables; the flagged columns
      effX, effIdx, effWork, effOut, effSlab;   // blmm_bulkscan_effects (kernels_effects.hip): the rotated markers column-major, the host form's
                                                // test lists, the sort's counters + permutation, the host form's outputs, the waves' slab
  // event sets: one per timed call since the last blmm_read_timings (grown on demand, reused afterwards)
  struct EvSet { hipEvent_t e[8]; int n; };
  std::vector<EvSet> evsets;
  size_t ev_used = 0;
  // side stream: work that only depends on the eigenvalues / rotated markers runs beside the per-trait Brent search
  hipStream_t side = nullptr, side2 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_xt = nullptr, ev_b1 = nullptr, ev_b2 = nullptr, ev_q = nullptr, ev_m = nullptr, ev_wb = nullptr;
  // An event to be recorded BY the next launch that honours it (BLMM_LAUNCH_STOP: hipExtLaunchKernel's stop event = the kernel's own
  // completion signal) instead of by a marker packet behind that kernel: a hipEventRecord between two dependent kernels of the main
  // stream cost 10-12 us of its critical path (profiles/r04_timeline_notiming_*.txt).  stop_event_used: the launch took it.
  hipEvent_t stop_event_next = nullptr; bool stop_event_used = false;
  // ... and one for the fast eigen path's k_eigf_pairs (a single matrix's launch): the eigenvalues are final there unless the
  // device rejects the path later, and the weight basis needs nothing else (blmm_api.hip: start_wbasis)
  hipEvent_t ev_pairs = nullptr, pairs_event_next = nullptr; bool pairs_event_used = false;
  // The null-exact front of the last call (blmm_last_front_route): FRONT_* bits known to the host
  int last_front_route = 0;
  bool wb_on_side2 = false;            // start_wbasis: the weight basis went to the second side stream (lr_begin follows it there)
  // Host entry points (blmm_bulkscan, blmm_bulkscan_reduced): K, the covariates and the weights go up first, the eigen phase is
  // queued, and only then Y and G are copied -- on their own stream, beside the eigen kernels (0.23 ms at n = 79 that the caller
  // used to wait for behind 27 MB of uploads).  up_pending: HostCall::defer_yg left them for prepare(); in_wait: the copies are
  // in flight, whoever reads inY / inG waits for ev_in first.  HostCall owns this state: it sets it, and its destructor clears it
  // at the end of every host-pointer call.
  hipStream_t copy = nullptr; hipEvent_t ev_in = nullptr, ev_inY = nullptr;   // ev_inY: the traits are there (the main stream's need), ev_in: the markers too
  bool up_pending = false, in_wait = false;
  const void* up_src[2] = {nullptr, nullptr}; void* up_dst[2] = {nullptr, nullptr}; size_t up_bytes[2] = {0, 0};
  int num_cus = 0;                 // multiProcessorCount of the device (bounds every co-resident grid)
  // sticky device-side abort word in pinned, device-mapped host memory: a kernel that gives up (bounded spin of the
  // multi-workgroup weight-basis kernel) is reported by the NEXT API call / blmm_synchronize even when the failing
  // call was made without a blmm_status (blmm_api.hip: check_sticky)
  volatile int64_t* hflag = nullptr;
  // the LOD matrix of the last host-pointer call, still resident in the workspace (kernels_post.hip: blmm_last_*)
  const double* last_L = nullptr; int64_t last_p = 0, last_m = 0; bool last_f32 = false;
  // blmm_set_log10p_output: the next bulkscan call also writes -log10 p (pv_out == nullptr: into outP, dense); pv_cur is set
  // while that call's scan kernels run (blmm_api.hip: scan_args).  last_P: the matrix that call left (blmm_last_log10p).
  bool pv_armed = false; double* pv_out = nullptr; int64_t pv_ld = 0, pv_df = 1;
  double* pv_cur = nullptr; int64_t pv_cur_ld = 0;
  const double* last_P = nullptr; int64_t last_P_ld = 0, last_P_df = 0;
  // blmm_bulkscan_reduced: set while that call's scan kernels run (blmm_api.hip: scan_args); last_reduced_route: 1 = the
  // reduce-in-epilogue kernels stood, 2 = through a resident L (no fused instantiation, or a trait needed a re-scan)
  blmm::RedArgs red_cur; int last_reduced_route = 0;
  // blmm_bulkscan_reduced_async: no host-blocking call in steady state.  grid_async: grid_to_device stages the caller's grid in
  // a pinned slot (blmm_api.hip: stage_to_device; gstage: a slot is reused once its event says its copy has run; a new slot is
  // added otherwise) instead of waiting for a pageable upload.  ev_call: recorded on the stream where a call starts; the side
  // streams wait for it.
  bool grid_async = false;
  struct GridSlot { void* h = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool used = false; };
  std::vector<GridSlot> gstage;
  hipEvent_t ev_call = nullptr;
  blmm::Tuning tune;                   // blmm_set_tuning
  bool perm_ready = false; int perm_ready_n = 0; int64_t perm_ready_nperms = 0; uint64_t perm_ready_seed = 0;   // launch_perm_gen -> launch_perm_panel
  int64_t lr_last_ldq = 0, lr_last_m = 0;   // panel-region width / trait count of the last low-rank null-exact scan (blmm_lowrank_columns)
  blmm::Pipe prep; bool prep_valid = false;   // state left by blmm_prepare_dev for blmm_rotate_block_dev / blmm_bulkscan_prerotated_dev
  bool brent_cnt_used = false;         // the current call has run a split h2 search already (its counter in the status block is spent)
  bool audit_ran = false;              // the current call ran the BLMM_FLAG_H2_AUDIT pass (finish_status: n_h2_multimodal, else -1)
  int eig_plan_n = -1;                 // n whose merge tree sits in eigW (kernels_eig.hip)
  blmm::HostStage* hstage = nullptr;   // pinned staging ring + copy threads of the host-pointer entry points (host_path.hip)
};

namespace blmm {

// The only writer of the matrix the blmm_last_* consumers serve (kernels_post.hip); clear_last: none
inline void set_last(blmm_ctx* ctx, const double* L, int64_t p, int64_t m, bool f32 = false) {
  ctx->last_L = L; ctx->last_p = p; ctx->last_m = m; ctx->last_f32 = f32;
}
inline void clear_last(blmm_ctx* ctx) { set_last(ctx, nullptr, 0, 0); }

// ---- error helpers -------------------------------------------------------------------------------
int fail(blmm_ctx* ctx, int code, const std::string& msg);
#define BLMM_HIP(call)                                                                              \
  do {                                                                                              \
    hipError_t e__ = (call);                                                                        \
    if (e__ != hipSuccess)                                                                          \
      return blmm::fail(ctx, BLMM_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__));     \
  } while (0)

int ensure(blmm_ctx* ctx, DevBuf& b, size_t bytes);
// Kernels whose workgroups meet at a grid barrier (k_sytrd, k_wbasis_mw) need ALL their workgroups resident at once.  Two of
// them launched from different contexts / streams on one device could each hold part of the CUs and starve the other (their
// bounded spins would then fail the calls).  A GridKernelGuard makes the stream wait for the previous such kernel on that
// device and, after the launch, record() marks this one: they run one after the other on the device, with no host
// synchronisation.  The guard holds the device's mutex from the wait to its destruction, so that wait -> launch -> record is
// one step against the other contexts' threads (blmm_bulkscan_multi with repeated device ids drives several contexts of one
// device from different threads; with begin / end as two separately locked calls both could pass the wait before either
// recorded).
struct GridKernelGuard {
  blmm_ctx* ctx; int dev; int rc = 0;
  explicit GridKernelGuard(blmm_ctx* c);
  int record();
  ~GridKernelGuard();
  GridKernelGuard(const GridKernelGuard&) = delete;
  GridKernelGuard& operator=(const GridKernelGuard&) = delete;
};
// host_path.hip: device -> caller memory in stream order; returns when the bytes are in place
int copy_to_host(blmm_ctx* ctx, void* dst, const void* dsrc, size_t bytes);
// host_path.hip: the host-pointer leg of an entry point that takes caller memory, one on the stack per call.  begin() selects the
// device; up() copies a caller array into device memory on ctx->stream (the DevBuf form ensures the buffer first); up_opt() does so
// for an optional input and yields nullptr for a null pointer or an empty array; defer_yg() leaves Y and G to prepare()
// (blmm_ctx::up_pending); inputs() does all of it for the standard input set (In); down() is a small device -> host copy on
// ctx->stream, skipped for a null destination (copy_to_host moves the large blocks); finish() is the success path's final
// synchronisation.  Every other exit -- an error rc, a BLMM_HIP early return, a failed ensure -- leaves through the destructor,
// which waits for the context's four streams: nothing the call enqueued still reads caller memory or the context's input buffers
// once it has returned.
struct HostCall {
  blmm_ctx* ctx;
  bool done = false;
  explicit HostCall(blmm_ctx* c) : ctx(c) {}
  ~HostCall();
  HostCall(const HostCall&) = delete;
  HostCall& operator=(const HostCall&) = delete;
  int begin();
  int up(void* dst, const void* src, size_t bytes);
  int up(DevBuf& b, const void* src, size_t bytes);
  int up_opt(DevBuf& b, const double* src, int64_t count, const double** dev);
  int defer_yg(const double* Y, size_t ybytes, const double* G, size_t gbytes);
  // Y (n x m) -> inY and G (n x p) -> inG, deferred when `defer`; then K (n x n, unless NULL) -> inK, the optional covariates
  // (n x ncov) -> inCov and weights (n) -> inW.  The device pointers come back with ncov = 0 when there are no covariates.
  struct In { const double *Y, *G, *K, *Cov, *W; int64_t ncov; };
  int inputs(const double* Y, int64_t n, int64_t m, const double* G, int64_t p, const double* K, const double* Covar, int64_t ncov,
             const double* weights, bool defer, In* in);
  int down(void* dst, const void* dsrc, size_t bytes);
  int finish(bool sync = true);   // sync = false: the last copy has waited already (copy_to_host, the blmm_last_* consumers)
};
void destroy_host_stage(HostStage* hs);
template <typename T>
inline T* ptr(DevBuf& b) { return reinterpret_cast<T*>(b.p); }

// ---- kernel launchers (kernels_prep.hip) ----------------------------------------------------------
struct Design {
  int n = 0, c = 0, npad = 0;   // npad: n rounded up to 4 (K dimension of the f64 MFMA)
  int ldr = 0;                  // leading dimension of Rp (npad rounded up to 16)
};

// Builds Zs = wd .* [1 Covar] (n x c) and Ks = wd_i wd_j K_ij (n x n).
int launch_design(blmm_ctx* ctx, const double* dK, const double* dCovar, int ncov, int add_intercept,
                  const double* dweights, int n, double* Ks, double* Zs);
// One-sided Jacobi eigen-decomposition of the symmetric n x n matrix in A (destroyed); V gets the eigenvectors
// (unsorted), then post_eigen sorts/derives everything the rotation needs.
struct PostEigenArgs;
int launch_jacobi(blmm_ctx* ctx, double* A, double* V, int n, double* lraw, int64_t* stat, const PostEigenArgs* pe = nullptr, bool* fused = nullptr);
// ... with launch_post_eigen's work in the tail of the same launch where its LDS fits (*fused)
int launch_jacobi_post(blmm_ctx* ctx, double* A, double* V, int n, double* lraw, int64_t* stat, const double* Zs, const double* dweights,
                       int c, int npad, int ldr, int decomp, int centered, double* lam, double* U, double* Z0, double* Rp, bool* fused);
// kernels_eig.hip: tridiagonalisation + divide and conquer for n beyond the LDS Jacobi; A is not modified
int launch_eig_dc(blmm_ctx* ctx, const double* A, int n, double* lraw, double* evec, int64_t* stat);
int eig_dc_max_n(const blmm_ctx* ctx);
// fold != nullptr: the first kernel of the fast path does launch_design's work on its way in (A = fold->Ks is WRITTEN, from fold->K and
// the weights, and so is fold->Zs) and zeroes the NSTAT words of stat: the caller then queues neither the design nor the memset.
struct DesignFold { const double* K; const double* Covar; const double* wd; double* Ks; double* Zs; int ncov, add_intercept; };
int launch_eig_fast(blmm_ctx* ctx, const double* A, int n, double* lraw, double* evec, int64_t* stat, const DesignFold* fold = nullptr);
// ... for nb matrices in one set of launches (batch on blockIdx.y): matrix b at A + b sA -> lraw + b sL, evec + b sE, stat + b sS
int launch_eig_fast_batch(blmm_ctx* ctx, const double* A, int64_t sA, int n, int nb, double* lraw, int64_t sL, double* evec, int64_t sE,
                          int64_t* stat, int64_t sS);
int eig_fast_max_n();
int jacobi_lds_max_n();
// lambda (ascending, or |lambda| descending for svd), U sorted, Z0 = U' Zs, Rp = (centered ? Q U' Wd : U' Wd)'
int launch_post_eigen(blmm_ctx* ctx, const double* lraw, const double* V, const double* Zs, const double* dweights, int n,
                      int c, int npad, int ldr, int decomp, int centered, double* lam, double* U, double* Z0, double* Rp,
                      int64_t* stat);
// Out (row-major, npad x ldo) = R * In  (In column-major n x ncols); pads with zeros up to ncols_pad / npad.
int launch_rotate(blmm_ctx* ctx, const double* Rp, int ldr, int n, int npad, const double* In, int64_t ncols,
                  double* Out, int64_t ldo, int64_t ncols_pad);
// launch_rotate's arithmetic for ONE column (scan's trait), applied to ncols columns; Out padded with zeros up to ldo columns
int launch_rotate_single(blmm_ctx* ctx, const double* Rp, int ldr, int n, int npad, const double* In, int64_t ncols, double* Out, int64_t ldo);
// row-major (npad x ld) -> column-major (n x ncols)
int launch_untranspose(blmm_ctx* ctx, const double* In, int64_t ld, int n, int64_t ncols, double* Out);

struct NullModel {
  int n, c, npad, reml, optim_interval;
  double prior_a, prior_b;
};
// per-trait Brent h2 (fitlmm) from centred/rotated Yt; outputs m each (sigma2/ell may be null).
// phase 0: the whole search.  phase 1: the first kernel only -- when sp->active comes back true, the traits with
// fin[j] == 1 are final and the other `*cnt` traits (list[]) are finished by a later phase-2 call with the same
// arguments (possibly on another stream); when false the search is already complete.
struct BrentSplit {
  bool active = false;
  const int* fin = nullptr;
  const int* list = nullptr;
  const unsigned int* cnt = nullptr;
};
// The traits' rotation inside k_brent (four lanes per trait, register evaluator: n <= 80): every wave rotates its own 16 columns of
// the caller's Y with k_rotate's arithmetic (rotate_wave), writes them to Yt -- rows up to npad, columns up to ncols_pad, as
// launch_rotate does -- and straight into its LDS slab.  Y == nullptr: Yt holds the rotated traits already.
struct BrentRot { const double* Y = nullptr; const double* Rp = nullptr; double* Yt = nullptr; int ldr = 0, npad = 0; int64_t ncols_pad = 0; };
bool brent_fuses_rotation(int n, int c);     // launch_brent takes a BrentRot at this size
int launch_brent(blmm_ctx* ctx, const NullModel& nm, const double* Yt, int64_t ldy, int64_t m, const double* Z0,
                 const double* lam, double* h2, double* sigma2, double* ell, int64_t* stat, int phase = 0,
                 BrentSplit* sp = nullptr, const BrentRot* rot = nullptr);
// scan_alt: per-marker fitlmm on [Z0 x_i] and the LOD against the null model (the trait is column 0 of Yt)
int launch_alt_brent(blmm_ctx* ctx, const NullModel& nm, const double* Yt, int64_t ldy, const double* Xt, int64_t ldx, int64_t p,
                     const double* Z0, const double* lam, const double* h2null, int true_w, double* lod, double* h2each,
                     int64_t* stat, int64_t m = 1, int64_t ldL = 0, int64_t ldH = 0);
// Ell[g, j] for every grid point and first-argmax; EllTab (ngrid x m, ld = ngrid) may be null
int launch_loglik_grid(blmm_ctx* ctx, const NullModel& nm, const double* Yt, int64_t ldy, int64_t m, const double* Z0,
                       const double* lam, const double* grid_dev, int ngrid, double* EllTab, int* h2idx, double* h2,
                       int64_t* stat);
// BLMM_FLAG_H2_AUDIT: counts the traits whose grid profile (EllTab, ngrid x m) has two or more local maxima
int launch_h2_audit(blmm_ctx* ctx, const double* EllTab, int ngrid, int64_t m, int64_t* stat);
// A-side panels for the scan kernels from per-trait h2: panel 0 = w.*resid/sqrt(yy); if full: panel 1 = w,
// panels 2..1+c = w .* (Z0 Linv')_q.  panels: [np][npad][ldp]
int launch_panels(blmm_ctx* ctx, const NullModel& nm, const double* Yt, int64_t ldy, int64_t m, const double* Z0,
                  const double* lam, const double* h2, int full, double* panels, int64_t ldp, int64_t* stat,
                  const double* gridv = nullptr, int ngrid = 0);   // gridv (c <= CTPL, !full): panel g = every trait at h2 = gridv[g], one launch
// isx[g][i] = 1/||P_g sqrt(w_g) x_i|| for every grid point
int launch_isx(blmm_ctx* ctx, const NullModel& nm, const double* Xt, int64_t ldx, int64_t p, const double* Z0,
               const double* lam, const double* grid_dev, int ngrid, double* isx, int64_t ld_isx, int64_t* stat);
int launch_kinship(blmm_ctx* ctx, const double* dG, int64_t n, int64_t p, double* dK, double* partial);
// kernels_loco.hip: the nchr leave-one-chromosome-out kinships (n x n each, stacked) from one pass over G; dchr = the nchr + 1
// chromosome offsets on the device; partial: nchr * nsplit * n * n doubles, nsplit from loco_kinship_splits
int loco_kinship_splits(int64_t n, int64_t nchr);
int launch_kinship_loco(blmm_ctx* ctx, const double* dG, int64_t n, const int64_t* dchr, int64_t nchr, int64_t digits, double* dK,
                        double* partial, int nsplit);
int launch_colmax(blmm_ctx* ctx, const double* L, int64_t p, int64_t m, int64_t ldL, double* mx, int64_t* arg);
// ... of rows row0 .. row0 + p - 1 of a larger matrix: row0 is added to every arg-maximum found (-1 stays -1)
int launch_colmax_rows(blmm_ctx* ctx, const double* L, int64_t p, int64_t m, int64_t ldL, double* mx, int64_t* arg, int64_t row0);
// kernels_post.hip
int launch_lod2log10p(blmm_ctx* ctx, const double* dL, int64_t p, int64_t m, int64_t ldL, int df, double* dP, int64_t ldP);
// permutation panel: column b = sqrt(w) .* P_w( pi_b(r0) ) / ||r0||  etc.  (see kernels_prep.hip)
int launch_perm_gen(blmm_ctx* ctx, int n, int64_t nperms, uint64_t seed);   // the library's own permutation indices into ctx->perm, ahead of launch_perm_panel
int launch_perm_panel(blmm_ctx* ctx, const NullModel& nm, const double* Yt, int64_t ldy, const double* Z0,
                      const double* lam, const double* h2, const int32_t* perm_idx, int64_t nperms, uint64_t seed,
                      int orig, double* panel, int64_t ldp, int64_t* stat);

// ---- kernel launchers (kernels_scan.hip) ----------------------------------------------------------
struct ScanArgs {
  const double* Xt; int64_t ldx;           // markers, row-major npad x ldx (unweighted, centred, rotated)
  const double* P; int64_t ldp; int64_t pstride;  // A-side panels [np][npad][ldp]
  int ks;                                  // npad / 4
  int n;                                   // sample size (LOD scale = -n/2)
  int64_t p, m;
  double* L; int64_t ldL;
  const double* isx; int64_t ld_isx; const int* bin;  // table mode
  // permuted-column mode of the table kernel (the shared-weights class of the low-rank form): panel column -> trait, the
  // region's first column, and the device count of the class (columns [col0, col0 + *count))
  const int* perm = nullptr; int64_t col0 = 0; const int64_t* count = nullptr;
  int c = 1;                               // null covariates (exact mode beyond CFAST: panels 2 + CFAST .. 1 + c are folded in chunks)
  const double* logtab;                    // device copy of log_table.h
  const double* lodtab;                    // ... of its directly indexed LOD table (fastmath.h: fast_lod5)
  double lodc[6];                          // {scale = -n/2, c1..c5}: the LOD polynomial of fast_lod5, computed on the host so that
                                           // the kernels hold it in SGPRs (gfx950 has no scalar fp64 arithmetic: derived in the
                                           // kernel the five coefficients cost 10 VGPRs in kernels at the register limit)
  int64_t* stat;
  // optional second output of the epilogue: -log10 p, one degree of freedom (blmm_set_log10p_output); pvtab = device copy of
  // pval_table.h.  Kernels without the fused form (alt-grid, fp32 permutations, the rare per-trait re-scans) leave Pv to a
  // column pass over the finished L (launch_lod2log10p / launch_pv_list).
  double* Pv = nullptr; int64_t ldPv = 0; const double* pvtab = nullptr;
  RedArgs red;                             // red.pmax != nullptr: the reduce-in-epilogue instantiation runs and L is not touched
  // launch_scan_cond (blmm_bulkscan_cond): per-trait flag (1: the conditioning guard re-scans the trait, its NaNs and rule hits are
  // counted there) and the call's info counters ([0]: entries the rank rule set to 0)
  const int* cflag = nullptr; int64_t* cinfo = nullptr;
};
// kernels_post.hip: threshold triplets of a resident L; the second pass of the reduce-in-epilogue scan (RedArgs partials -> per trait)
int launch_threshold(blmm_ctx* ctx, const double* dL, int64_t p, int64_t m, int64_t ldL, double thr, int64_t cap,
                     int32_t* di, int32_t* dj, double* dlod, int64_t* dcount);
// ... of rows row0 .. row0 + p - 1 of a larger matrix: row0 is added to every triplet's marker index, and *dcount is not zeroed
// first (the triplets of several row blocks accumulate behind one counter)
int launch_threshold_rows(blmm_ctx* ctx, const double* dL, int64_t p, int64_t m, int64_t ldL, double thr, int64_t cap,
                          int32_t* di, int32_t* dj, double* dlod, int64_t* dcount, int64_t row0);
int launch_red_final(blmm_ctx* ctx, const RedArgs& r, int nslot, int64_t m, double* mx, int64_t* arg);
// blmm_bulkscan_loco_reduced: per trait, every chromosome's (max, global argmax) -> cmx / carg (nchr x m, chromosome c at + c m) and
// their merge in ascending chromosome order -> mx / arg.  pmax != nullptr: from the slot partials (chromosome c's at slot
// sum_{c' < c} 2 ceil(pc' / 128), in the chromosomes' own marker index); nullptr: cmx / carg hold the chromosomes' results already
int launch_red_final_loco(blmm_ctx* ctx, const double* pmax, const int* parg, int64_t ldm, const int64_t* dchr, int64_t nchr, int64_t m,
                          double* cmx, int64_t* carg, double* mx, int64_t* arg);
// blmm_bulkscan_reduced_async: the info block (BLMM_RINFO_*) from the status counters, in stream order; route 0: 3 when a guard
// flagged a trait, else 1.  Also raises the context's sticky word on a device-side failure (as k_sticky).
int launch_red_info(blmm_ctx* ctx, const int64_t* stat, int route, const int64_t* count, int64_t* info);
int launch_scan_exact(blmm_ctx* ctx, const ScanArgs& a, int c);
int launch_scan_cond(blmm_ctx* ctx, const ScanArgs& a, int ct);   // a.c = ct = covariates + conditioning loci, uncentred markers
// A region of the panel arrays of the low-rank form: columns [col0, col0 + ncol), the shared-weights class at its front
// (counts[0] traits) and the other class at its back (counts[1]); counts live on the device.
constexpr int LR_TILE = 64;   // a multiple of every trait-tile width of k_scan_lr (32 * MB); regions are multiples of it
struct LrRegion {
  int64_t col0 = 0, ncol = 0;
  int64_t* counts = nullptr;        // {shared-weights traits, columns of the other class (every segment's run rounded up to LR_TILE)}
  int64_t* segcnt = nullptr;        // [LR_SEG_MAX] traits of the other class per weight-basis segment; segcnt + 8: the placement cursors {shared, segment 0, ..}
};
// Segments of the heritability axis, each with its OWN weight basis (kernels_lowrank.hip): the family { w(h2) : h2 in a segment }
// has a far smaller numerical rank than the whole family (BXD spectrum: 11-12 per segment of the six below against 23), so the
// rank-R phase of k_scan_lr runs 3 K steps where the single basis needs 6.  The other class of a region is laid out segment by
// segment from the back of the region, every segment's run rounded up to LR_TILE columns: a tile of the scan never mixes segments.
constexpr int LR_SEG_MAX = 8;
struct LrSeg {
  int S = 1;
  double edge[LR_SEG_MAX + 1] = {0.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0};   // segment s: edge[s] <= h2 < edge[s + 1] (the last one takes the rest)
};
// columns of the other class in front of segment s's run, counted from the END of the region, and the run's width
__host__ __device__ inline int64_t lr_seg_width(int64_t cnt) { return (cnt + LR_TILE - 1) / LR_TILE * LR_TILE; }
// segment of the column `dist` columns before the region's end (dist = 0: the last column); S - 1 beyond every run (padding)
__host__ __device__ inline int lr_seg_of(int64_t dist, const int64_t* segcnt, int S) {
  for (int s = 0; s + 1 < S; ++s) {
    const int64_t w = lr_seg_width(segcnt[s]);
    if (dist < w) return s;
    dist -= w;
  }
  return S - 1;
}
struct LrArgs {
  ScanArgs s;                       // s.P = panel 0 only
  const double* Cp;                 // weight-basis coefficients [4*KR][ldp]
  const double* T; int64_t tstride; // marker-side basis products [1+c][4*KR][ldx]
  const double* Ls;                 // packed L_j^-1 [c(c+1)/2][ldp]
  const int* rk;                    // {R, KR, -, -} per segment on the device
  LrSeg seg;                        // T, Q of segment s: s * (1 + c) * tstride, s * npad * n doubles further on
  const int* perm;                  // panel column -> trait (k_lr_classify; -1: padding)
  LrRegion rg;                      // the region of the panel arrays this launch scans
  const double* den0;               // the shared-weights class's 1/sqrt(Sxx - |u|^2), per marker (= isx of the unweighted model)
  int skip_shared;                  // 1: the class's tiles were scanned by launch_scan_shared
  int c;
};
int launch_scan_lr(blmm_ctx* ctx, const LrArgs& la);
int launch_lr_resid(blmm_ctx* ctx, const NullModel& nm, int64_t m, double tol, const double* lam, const double* h2,
                    const double* Q, const int* rk, const LrSeg& seg, const int* perm, const LrRegion& rg, const double* Cp, int64_t ldp,
                    int* flag_list, double* part, int64_t* stat, int* flags = nullptr);
// red.pmax != nullptr: the reduced form (k_scan_fix<C, true>): the flagged traits' slot partials and triplets instead of L's columns
int launch_scan_fix(blmm_ctx* ctx, const NullModel& nm, const double* Xt, int64_t ldx, int64_t p, const double* P0,
                    const double* Ls, int64_t ldp, const double* Z0, const double* lam, const double* h2,
                    const int* flag_list, const int* perm, double* L, int64_t ldL, int64_t* stat, const RedArgs& red = RedArgs());
// shared-weights class: column order of the panels (perm, info) and the per-marker denominators of the unweighted model
int launch_lr_classify(blmm_ctx* ctx, int n, int64_t m, double tol, const double* lam, const double* h2, const int* fin,
                       const int* list, const unsigned int* list_cnt, int* perm, const LrRegion& rg, const LrSeg& seg);
// kernels_scan_f32.hip: fp32 permutation LOD kernel and the fp64 k-major -> fp32 fragment-major conversion
int launch_cvt_f32(blmm_ctx* ctx, const double* M, int64_t ld_in, int rows_valid, int64_t cols_valid, float* F,
                   int64_t ld_out, int kblocks);
// fp32 rotation of the fp32 permutation path: XF (fragment-major) = R G from the caller's fp64 column-major G; the marker norms
// from XF; the original trait's fp64 LOD from G itself (kernels_scan_f32.hip, kernels_prep.hip)
int launch_rotate_f32(blmm_ctx* ctx, const double* Rp, int ldr, int n, int npad, const double* dG, int64_t p, float* RF, float* XF, int64_t ldxf,
                      const double* a0, int64_t lda, double* v_work /* n rounded up to 16 */, double* num /* p: g_i' R'a0 in fp64 */);
int launch_lod_from_num(blmm_ctx* ctx, const double* num, const double* isx, int n, int64_t p, double* lod, int64_t* stat);
int launch_isx_f32(blmm_ctx* ctx, const NullModel& nm, const float* XF, int64_t ldxf, int64_t p, const double* Z0, const double* lam,
                   const double* h2_dev, double* isx, int64_t ld_isx, int64_t* stat);
int launch_scan_f32(blmm_ctx* ctx, const float* XF, int64_t ldxf, const float* PF, int64_t ldpf, int npad, int n,
                    int64_t p, int64_t m, const double* isx, float* L, int64_t ldL, int64_t* stat);
// kernels_dyn.hip: run-time covariate counts (c = CTPL + 1 .. CMAX): the counterparts of launch_brent / launch_loglik_grid /
// launch_panels / launch_isx / launch_perm_panel, which route there
int launch_dyn_brent(blmm_ctx* ctx, const NullModel& nm, const double* Yt, int64_t ldy, int64_t m, const double* Z0, const double* lam,
                     double* h2, double* sigma2, double* ell, int64_t* stat);
// scan_alt's per-marker searches on the design [Z0 x_i] (c + 1 <= CMAX columns), the counterpart of launch_alt_brent
int launch_dyn_alt_brent(blmm_ctx* ctx, const NullModel& nm, const double* Yt, int64_t ldy, const double* Xt, int64_t ldx, int64_t p,
                         const double* Z0, const double* lam, const double* h2null, int true_w, double* lod, double* h2each,
                         int64_t* stat, int64_t m, int64_t ldL, int64_t ldH);
int launch_dyn_loglik_grid(blmm_ctx* ctx, const NullModel& nm, const double* Yt, int64_t ldy, int64_t m, const double* Z0,
                           const double* lam, const double* grid_dev, int ngrid, double* EllTab, int* h2idx, double* h2, int64_t* stat);
int launch_dyn_panels(blmm_ctx* ctx, const NullModel& nm, const double* Yt, int64_t ldy, int64_t m, const double* Z0, const double* lam,
                      const double* h2, int full, double* panels, int64_t ldp, int64_t* stat);
int launch_dyn_isx(blmm_ctx* ctx, const NullModel& nm, const double* Xt, int64_t ldx, int64_t p, const double* Z0, const double* lam,
                   const double* grid_dev, int ngrid, double* isx, int64_t ld_isx, int64_t* stat);
int launch_dyn_perm(blmm_ctx* ctx, const NullModel& nm, const double* Yt, int64_t ldy, const double* Z0, const double* lam, const double* h2,
                    const int32_t* perm, int64_t ncols, int orig, double* r0, double* panel, int64_t ldp, int64_t* stat);
// kernels_dyn.hip: conditioning guard of the null-exact scan (c >= 2) and the QR-grade re-scan of the flagged traits
int launch_illcond_flag(blmm_ctx* ctx, const NullModel& nm, int64_t m, const double* Z0, const double* lam, const double* h2,
                        int* list, int64_t* stat, int* flags = nullptr);
int launch_scan_qr(blmm_ctx* ctx, const NullModel& nm, const double* Yt, int64_t ldy, const double* Xt, int64_t ldx, int64_t p,
                   const double* Z0, const double* lam, const double* h2, const int* list, double* L, int64_t ldL, int64_t* stat,
                   const RedArgs& red = RedArgs());
// The workspace of the QR-grade re-scans (ortho_basis.h): (cols + 2) n doubles per workgroup -- the weights' square roots, `cols`
// basis columns, the trait residual -- as dynamic LDS up to 64 KiB (*slab = nullptr; the launcher raises the kernel's limit above
// 48 KiB), beyond that *lds = 0 and a slab of ctx->qrSlab per workgroup.  *grid: two workgroups per CU, striding over the listed traits.
inline int qr_workspace(blmm_ctx* ctx, int cols, int n, size_t* lds, double** slab, unsigned* grid) {
  const size_t per = (size_t)(cols + 2) * n;
  *grid = (unsigned)(2 * (ctx->num_cus > 0 ? ctx->num_cus : 256));
  *lds = sizeof(double) * per;
  *slab = nullptr;
  if (*lds <= 64 * 1024) return BLMM_OK;
  if (int rc = ensure(ctx, ctx->qrSlab, sizeof(double) * per * *grid)) return rc;
  *slab = ptr<double>(ctx->qrSlab);
  *lds = 0;
  return BLMM_OK;
}
// kernels_lowrank.hip
// the segments a call with n individuals uses (one when the basis comes from the multi-workgroup / LDS kernels: n > 80)
LrSeg lr_segments(const blmm_ctx* ctx, int n);
enum WbMode { WB_LAM = 0, WB_EARLY = 1, WB_REDO = 2 };   // kernels_lowrank.hip: k_wbasis_reg
int launch_wbasis(blmm_ctx* ctx, const double* lam, int n, int npad, const LrSeg& seg, double* Wk, double* Q, int* rk, int64_t* stat,
                  int mode = WB_LAM, const double* lraw = nullptr, int decomp = 0);
int launch_lr_tpanels(blmm_ctx* ctx, const double* Xt, int64_t ldx, int64_t p, int n, int c, int npad, const double* Z0,
                      const double* Q, const int* rk, const LrSeg& seg, double* T, int64_t tstride, double* den0);
int launch_lr_panels(blmm_ctx* ctx, const NullModel& nm, const double* Yt, int64_t ldy, int64_t m, const double* Z0,
                     const double* lam, const double* h2, const double* Q, const int* rk, const LrSeg& seg, const int* perm, const LrRegion& rg,
                     double* P0, double* Cp, double* Ls, int64_t ldp, int64_t* stat);
int launch_scan_table(blmm_ctx* ctx, const ScanArgs& a);
// the shared-weights class of one panel region through the table kernel (isx = 1/sqrt(den0), one bin, stores through perm)
int launch_scan_shared(blmm_ctx* ctx, const ScanArgs& a);
struct AltArgs {
  ScanArgs s;
  int ngrid; const double* EllTab; /* ngrid x m */ const double* grid_dev; double* H2; int64_t ldH; int counter_quirk;
  const double* Ctab;    // exp(-(2/n)(Ell[g, j] - max_g Ell[g, j])), ngrid x m (launch_alt_ctab): the fold's monotone image of logL1
};
int launch_scan_alt(blmm_ctx* ctx, const AltArgs& a);
int launch_alt_ctab(blmm_ctx* ctx, const double* EllTab, int ngrid, int64_t m, int n, double* C);
// kernels_bperm.hip: blmm_bulkscan_perms.  Panel columns of the chunk's mt traits (Yt, h2c: the chunk's first trait), column
// jj (nperms + 1) + b = trait jj under permutation b - 1 of perm (n x nperms; b = 0: unpermuted), bin[column] = jj; c <= CTPL
int launch_bperm_panels(blmm_ctx* ctx, const NullModel& nm, const double* Yt, int64_t ldy, const double* Z0, const double* lam,
                        const double* h2c, int64_t mt, const int32_t* perm, int64_t nperms, double* panel, int64_t ldp, int* bin,
                        int64_t* stat);
// ---- the quantiles of a vector of maxima, as every kernel that takes them sorts and interpolates (k_bitonic_*, k_quantiles,
// k_bperm_summary) ----
// total order of the sort: NaN is the largest key
__host__ __device__ inline bool key_less(double a, double b) {
  if (a != a) return false;
  if (b != b) return true;
  return a < b;
}
// Julia's default quantile (type 7) between the neighbouring order statistics a <= b, g = h - floor(h) in [0, 1), h = (n - 1) q:
//   g == 0 or a == b  ->  a              (an order statistic itself; two equal infinities are that infinity, not inf - inf)
//   both finite       ->  a + g (b - a)
//   otherwise         ->  (1 - g) a + g b in the extended reals: +inf above a finite a, -inf below a finite b; -inf beside +inf is
//                         the limit of (1 - g)(-M) + g M = (2 g - 1) M: -inf below g = 1/2, +inf above it, 0 at it
// so a threshold is NaN only when one of its two neighbours is.
__host__ __device__ inline double quantile7_interp(double a, double b, double g) {
  if (g == 0.0 || a == b) return a;
  const bool fa = a - a == 0.0, fb = b - b == 0.0;   // finite
  if (fa && fb) return a + g * (b - a);
  if (!fa && !fb && a < b) return g < 0.5 ? a : (g > 0.5 ? b : 0.0);
  return (1.0 - g) * a + g * b;
}
// quantile levels of the thresholds, passed by value (at most 64, as blmm_get_thresholds)
struct BpermProbs { double v[64]; };
// per trait of the chunk: peak and marker, the permutation maxima (max_perms: nperms x m, ld = nperms), thresholds (nprobs x m,
// ld = nprobs) and the empirical p-value (lod_max / lod_argmax / max_perms / thr / pval may be null); row0 is added to the markers
int launch_bperm_summary(blmm_ctx* ctx, const double* mx, const int64_t* arg, int64_t mt, int64_t nperms, const BpermProbs& probs,
                         int nprobs, int64_t j0, double* lod_max, int64_t* lod_argmax, double* max_perms, double* thr, double* pval,
                         int64_t row0 = 0);
// blmm_bulkscan_loco_perms: a chunk's ncols column maxima (markers + row0) into the genome-wide buffer at the chunk's columns
// (gmx / garg already offset), k_red_final's rule; and the buffer's -inf / -1 start
int launch_bperm_loco_merge(blmm_ctx* ctx, const double* mx, const int64_t* arg, int64_t ncols, int64_t row0, double* gmx, int64_t* garg);
int launch_bperm_loco_init(blmm_ctx* ctx, int64_t n, double* gmx, int64_t* garg);
constexpr int BPERM_MAX_NPERMS = 16384;

// kernels_mdf.hip: blmm_bulkscan_multidf, the k-degree-of-freedom scan (loci of k adjacent columns of G)
constexpr double MDF_TAU = BLMM_MULTIDF_TAU;          // rank rule: a locus column is kept iff |r_a|^2 > MDF_TAU |x~_a|^2
constexpr int MDF_CMAX = BLMM_MULTIDF_MAX_COVARIATES;  // null covariates incl. the intercept
struct MdfArgs {
  const double* Xt; int64_t ldx;       // rotated markers (uncentred: k_mdf_rawrot), npad x ldx row-major, locus l = columns l k ..
  int64_t nloci; int k; int n; int64_t m;
  const double* P; int64_t ldp; int64_t pstride;   // k_panels' panels (grid: panel 0; exact: 2 + c panels, pstride apart)
  int c;
  const double* T; const int* bin;     // null-grid: k_mdf_table's ngrid x nloci factors, each trait's grid bin
  double* L; int64_t ldL; int64_t* stat;
};
int launch_mdf_rawrot(blmm_ctx* ctx, const double* U, const double* wd, int n, int npad, int ldr, double* R);
int launch_mdf_table(blmm_ctx* ctx, const NullModel& nm, const double* Xt, int64_t ldx, int64_t nloci, int k, const double* Z0,
                     const double* lam, const double* grid_dev, int ngrid, double* T);
int launch_mdf_scan(blmm_ctx* ctx, const MdfArgs& a, bool exact);
// blmm_bulkscan_multidf_perms: the null-grid scan reduced in its epilogue to slot partials (r.pmax / r.parg / r.ldm, ceil(nloci / 64)
// slots, finished by launch_red_final); a.L unused.  At most MDF_RED_MAX_COLS columns (a.m) a launch: 65535 grid rows of 4 x 8 columns
constexpr int64_t MDF_RED_MAX_COLS = 65535ll * 32;
int launch_mdf_scan_red(blmm_ctx* ctx, const MdfArgs& a, const RedArgs& r);
// blmm_bulkscan_multidf_reduced: the traits' own scan reduced in its epilogue (r: partials as above, triplets, r.flags: the traits the
// conditioning guard flagged -- skipped here)
int launch_mdf_scan_traits_red(blmm_ctx* ctx, const MdfArgs& a, const RedArgs& r, bool exact);
// scr != nullptr: the listed traits item0 .. item0 + nitem - 1 into columns 0 .. of the compact scratch scr (ld nloci), L untouched
int launch_mdf_qr(blmm_ctx* ctx, const NullModel& nm, const double* Yt, int64_t ldy, const double* Xt, int64_t ldx, int64_t nloci, int k,
                  const double* Z0, const double* lam, const double* h2, const int* list, double* L, int64_t ldL, int64_t* stat,
                  double* scr = nullptr, int64_t item0 = 0, int64_t nitem = 0);
// ... and that scratch reduced into mx / arg (at the traits' indices; either may be null) and r's triplets
int launch_mdf_flag_red(blmm_ctx* ctx, const double* scr, int64_t nloci, const int* list, const int64_t* stat, int64_t item0,
                        int64_t nitem, double* mx, int64_t* arg, const RedArgs& r);
   // k_bperm_summary sorts a trait's maxima in LDS (128 KB)

// kernels_cond.hip: blmm_bulkscan_cond, every trait scanned with its own conditioning loci in the null design
constexpr int COND_NINFO = 8;          // device counters: [0 .. BLMM_COND_INFO_LEN) the caller's info block, [4] traits with an index out of range
struct CondArgs {
  int n, c, s, npad; int64_t m, p;
  const double* Xt; int64_t ldx;       // rotated markers (uncentred: k_mdf_rawrot), npad x ldx row-major
  const double* Yt; int64_t ldy;       // rotated traits, row-major
  const double *Z0, *lam;
  const int64_t* cond;                 // s x m: cond[j s + a] = trait j's a-th conditioning column of G, -1: none
  int* kept;                           // [m][s]: the columns step 1 keeps, in order (-1 beyond r_j)
  int* nk;                             // r_j; -1: an index outside [-1, p) (NaN column, NaN h2)
  int* flag;                           // 1: listed for k_cond_qr
  int64_t* info;                       // COND_NINFO counters
  double* h2;
  int64_t* stat;
  // blmm_bulkscan_stepwise: the active traits, ascending.  Non-null: a.m columns, column jj is trait act[jj] of Yt and cond, and
  // kept / nk / flag / h2 (and the panels, the guard's list) are indexed by COLUMN.  nullptr: column jj is trait jj.
  const int* act = nullptr;
};
// step 1 and the null model on D_j = [Z0, kept columns]: fitlmm (grid_dev == nullptr) or the first arg-max over the grid
int launch_cond_null(blmm_ctx* ctx, const NullModel& nm, const CondArgs& a, const double* grid_dev, int ngrid);
// k_panels' layout with 2 + c + s panels per trait (zero panels beyond 1 + c + r_j); flags the traits of the conditioning guard
int launch_cond_panels(blmm_ctx* ctx, const NullModel& nm, const CondArgs& a, double* panels, int64_t ldp, double rho_min, int* list);
// scr != nullptr: the listed columns item0 .. item0 + nitem - 1 into columns 0 .. of the compact scratch scr (ld p), L untouched
int launch_cond_qr(blmm_ctx* ctx, const NullModel& nm, const CondArgs& a, const int* list, double* L, int64_t ldL,
                   double* scr = nullptr, int64_t item0 = 0, int64_t nitem = 0);
// blmm_bulkscan_stepwise: the caller's tables (device) and four work counters: w[0] the next round's traits, w[1] the guard's
// re-scans so far, w[2] round 0's n_zero_norm, w[3] traits with at least one locus
struct StepArgs {
  int S; int64_t m; double thr;
  int64_t* loci; double* lod; int64_t* arg; double* h2; int64_t* nloci;
  int64_t* w;
};
struct StepRounds { int64_t rounds; int64_t nact[5]; };
int launch_step_init(blmm_ctx* ctx, const StepArgs& s);                      // NaN / -1 / NaN everywhere, no loci
int launch_step_update(blmm_ctx* ctx, const StepArgs& s, int t, int64_t nact, const int* act, int* next, const double* mx,
                       const int64_t* arg, const double* h2, int64_t* stat);
int launch_step_finish(blmm_ctx* ctx, const StepArgs& s, const StepRounds& r, const int64_t* cinfo, int64_t* stat, int64_t* sinfo);

// kernels_effects.hip: blmm_bulkscan_effects, coefficients and standard errors at a list of (locus, trait) tests
struct EffArgs {
  int n, c, k; int64_t m, nloci, T;
  const double* Xc;                    // rotated markers (uncentred), COLUMN-major: column i of G at Xc + i n
  const double* Yt; int64_t ldy;       // rotated traits, row-major
  const double *Z0, *lam, *h2;         // rotated covariates (column-major n x c), eigenvalues, each trait's null h2
  const int64_t *locus, *trait;        // the T tests
  int* cnt; int* order;                // the sort: m + 2 counters (offsets; [m] valid tests, [m + 1] tests out of range), sorted position -> test
  int reml; double prior_a, prior_b;
  double *beta, *se, *sigma2, *lod; int32_t* accepted;
  int64_t* stat;
  double* slab; int chunk;             // set by launch_effects
};
int launch_effects_sort(blmm_ctx* ctx, const EffArgs& a);
int launch_effects(blmm_ctx* ctx, EffArgs a);

}  // namespace blmm

// launch on ctx->stream; a pending event in the slot (next_, used_) of ctx is recorded by this kernel's completion (see blmm_ctx)
#define BLMM_LAUNCH_STOP_AT(ctx_, next_, used_, kernel_, grid_, block_, lds_, ...)                                         \
  do {                                                                                                                   \
    if ((ctx_)->next_) {                                                                                                 \
      hipExtLaunchKernelGGL(kernel_, grid_, block_, (std::uint32_t)(lds_), (ctx_)->stream, nullptr, (ctx_)->next_, 0, __VA_ARGS__); \
      (ctx_)->next_ = nullptr; (ctx_)->used_ = true;                                                                     \
    } else hipLaunchKernelGGL(kernel_, grid_, block_, lds_, (ctx_)->stream, __VA_ARGS__);                                 \
  } while (0)
// ... the slot of the phase-ending launches: ctx->stop_event_next
#define BLMM_LAUNCH_STOP(ctx_, ...) BLMM_LAUNCH_STOP_AT(ctx_, stop_event_next, stop_event_used, __VA_ARGS__)
