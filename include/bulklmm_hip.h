/*
 * bulklmm_hip.h -- C ABI of libbulklmm_hip.so: the MI355X (gfx950) bulkscan engine.
 *
 * This is the drop-in boundary for the `bulkscan` hot path of senresearch/BulkLMM.jl v1.2.0
 * (pure Julia; it has no FFI of its own, so the seam is placed under its exported API,
 * src/BulkLMM.jl:9-47).  A Julia host binds these entry points with `ccall`
 * (bulklmm.jl_amd/julia/BulkLMMHIP.jl); the Python host mirror
 * (bulklmm.jl_amd/api.py) binds the same symbols with ctypes.
 *
 * Conventions
 *   - every matrix is dense float64, column-major, leading dimension = row count unless an
 *     explicit `ld` argument is given (Julia Array{Float64,2} / NumPy order='F');
 *   - sizes are int64_t (Julia Int64);
 *   - the caller owns every buffer; the library never retains a caller pointer after return;
 *   - functions return 0 on success or a negative blmm_err code; blmm_last_error(ctx) gives the
 *     message (the reference's own message strings are used where the reference throws);
 *   - `*_dev` entry points take DEVICE pointers (HBM-resident operands, e.g. torch tensors) and
 *     enqueue on the context's stream without synchronising it; the un-suffixed entry points take
 *     HOST pointers, copy in/out and return when the outputs are complete in caller memory;
 *   - a blmm_ctx is bound to one GPU and is not thread-safe (one call at a time per ctx).
 */
#ifndef BULKLMM_HIP_H
#define BULKLMM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BLMM_VERSION 210 /* 0.2.3: L_out == NULL keeps the matrix in HBM (blmm_bulkscan, blmm_bulkscan_multi), blmm_last_lod_colmax /
                            blmm_last_lod_columns / blmm_last_dims, blmm_bulkscan_reduced[_dev] (no L at all), blmm_tuning,
                            blmm_bulkscan_reduced_async + BLMM_RINFO_* (stream-ordered, flagged traits re-scanned on the device);
                            205 (0.2.2): blmm_status.n_h2_boundary / n_h2_multimodal / n_illcond_rescan (appended), BLMM_FLAG_H2_AUDIT;
                            201: lowrank_shared, readers, blmm_scan_alt; 200: lowrank_fallback, BLMM_STREAM_NULL, multi-GPU;
                            added since without a new number: blmm_bulkscan_multidf_perms[_dev], blmm_bulkscan_multidf_reduced[_dev],
                            blmm_bulkscan_stepwise[_dev] + BLMM_STEP_INFO_LEN, tuning key "cond_red_chunk" */

typedef struct blmm_ctx blmm_ctx;

enum blmm_err {
  BLMM_OK = 0,
  BLMM_ERR_INVALID = -1,       /* bad argument */
  BLMM_ERR_DIM = -2,           /* "Dimension mismatch."                      src/transform_helpers.jl:9-11 */
  BLMM_ERR_H2_ONE = -3,        /* "Heritability of 1 is not allowed."        src/lmm.jl:19-21 */
  BLMM_ERR_DECOMP = -4,        /* "Please choose either `eigen` or `svd`..." src/transform_helpers.jl:51 */
  BLMM_ERR_METHOD = -5,        /* unknown bulkscan method                    src/bulkscan.jl:126-154 */
  BLMM_ERR_ONE_TRAIT = -6,     /* "Can only handle one trait."               src/scan.jl:496-498 */
  BLMM_ERR_NO_INTERCEPT = -7,  /* "Intercept has to be added when no other covariate is given." src/scan.jl:167-169 */
  BLMM_ERR_ZERO_NORM = -8,     /* "Dividing by zeros: the input vector can not contain any zeros!" src/util.jl:69-71 */
  BLMM_ERR_NPERMS = -9,        /* "The required number of permutations must be a positive integer." src/scan.jl:528-530 */
  BLMM_ERR_UNSUPPORTED = -10,  /* e.g. more null covariates than the kernels are instantiated for */
  BLMM_ERR_NO_DEVICE = -11,    /* no usable gfx950 device */
  BLMM_ERR_HIP = -12,          /* a HIP runtime call failed */
  BLMM_ERR_ALLOC = -13
};

enum blmm_method { BLMM_NULL_EXACT = 0, BLMM_NULL_GRID = 1, BLMM_ALT_GRID = 2 };
enum blmm_decomp { BLMM_EIGEN = 0, BLMM_SVD = 1 };

/* compat_flags bits */
#define BLMM_COMPAT_ALT_COUNTER 1 /* B2: h2_panel indexed by an improvement counter, src/bulkscan_helpers.jl:342-343 */
#define BLMM_COMPAT_ALT_TRUE_WEIGHTS 2 /* blmm_scan_alt: evaluate the closing log-likelihoods at makeweights(h2); the default
                                          restates src/scan.jl:431-436, which hands wls the square roots of the weights */
/* Not a compat switch but carried in the same word: null-exact only, opt-in diagnostic.  After the h2 search the profile
 * log-likelihood of EVERY trait is evaluated on the 16-point grid 0, 1/16, .., 15/16 and blmm_status.n_h2_multimodal counts
 * the traits whose grid profile has two or more local maxima.  Brent (src/gridbrent.jl:9-24, one run over [0, 1] when
 * optim_interval = 1) is a LOCAL method: on such a trait rounding-level differences decide which maximum a run ends in --
 * for the reference's arithmetic as much as for this library's -- so these are the traits whose h2 (and LOD column) may
 * legitimately differ between two correct implementations; raising optim_interval resolves them.  Costs one grid
 * log-likelihood pass (~0.06 ms at BXD size). */
#define BLMM_FLAG_H2_AUDIT 4

/* Mirrors the keyword arguments of bulkscan()/scan() 1:1 (src/bulkscan.jl:81-92, src/scan.jl:94-109).
 * `nb` and `nt_blas` (thread blocking knobs of the CPU reference) have no meaning here. */
typedef struct blmm_opts {
  int32_t method;         /* blmm_method; bulkscan(...; method=)           */
  int32_t reml;           /* reml::Bool                                     */
  int32_t add_intercept;  /* addIntercept::Bool (Covar given)               */
  int32_t decomp_scheme;  /* blmm_decomp; decomp_scheme::String             */
  int32_t optim_interval; /* optim_interval::Int64 (null-exact, scan)       */
  int32_t compat_flags;   /* BLMM_COMPAT_*                                  */
  double prior_variance;    /* prior_variance::Float64                      */
  double prior_sample_size; /* prior_sample_size::Float64                   */
} blmm_opts;

/* Counters behind the reference's warnings / exceptions, plus per-phase device timings (ms)
 * measured with HIP events when blmm_set_timing(ctx, 1) is on (0 otherwise). */
typedef struct blmm_status {
  int64_t n_neg_eig;       /* eigenvalues < -1e-7           -> warning, src/transform_helpers.jl:27-30 */
  int64_t n_nonpos_weight; /* weights <= 0                  -> warning, src/wls.jl:35-37               */
  int64_t n_zero_norm;     /* |column norm| <= eps          -> error,   src/util.jl:47-71              */
  int64_t n_nan_lod;       /* r^2 > 1 (DomainError in the reference, NaN here), src/bulkscan_helpers.jl:23 */
  int64_t n_brent_maxiter; /* traits whose Brent search hit 1000 iterations                            */
  int64_t jacobi_sweeps;   /* sweeps of the LDS Jacobi; 0: n <= 124 and the fast path's result stood, or n > 124 */
  int64_t jacobi_cycles;   /* shader cycles / 100 MHz ticks spent inside the eigensolver (diagnostic)  */
  int64_t jacobi_ticks_100mhz;
  int64_t lowrank_rank;    /* rank R of the weight-family basis used by the null-exact kernel (kernels_lowrank.hip) */
  int64_t lowrank_fallback;/* traits whose expansion residual exceeded 1e-13: their LOD columns were recomputed from
                              the full-length sums (k_scan_fix), so every returned LOD is either guarded or exact      */
  int64_t lowrank_shared;  /* traits whose weights are 1 to within the same tolerance (likelihood peaks at h2 = 0): their
                              denominators are the per-marker constants of the unweighted model, no basis needed          */
  double lowrank_resid;    /* largest relative residual |w_j - Q Q'w_j| / |w_j| over all traits of the rank-R class (before the
                              re-scan); the shared-weights class is bounded by its own criterion, the same tolerance         */
  double t_eigen_ms, t_rotate_ms, t_h2_ms, t_prep_ms, t_scan_ms, t_total_ms;
  int64_t n_h2_boundary;   /* null-exact / scan: traits whose h2 estimate sits on a boundary of [0, 1] (<= 1e-6 or >= 1 - 1e-6):
                              the likelihood is one-sided there and x_tol shrinks with x, so these are the long Brent runs  */
  int64_t n_h2_multimodal; /* BLMM_FLAG_H2_AUDIT: traits whose profile log-likelihood has >= 2 local maxima on the 16-point
                              grid (optimiser-sensitive: see the flag); -1 when the audit was not requested                  */
  int64_t n_illcond_rescan;/* traits whose weighted null design sqrt(w) .* Z0 is ill conditioned (Cholesky pivot ratio of
                              Z0'WZ0 above 1e4, i.e. cond(sqrt(W) Z0) > 100: h2 -> 1 with several covariates): their LOD
                              columns were recomputed with an orthogonalised (MGS2, QR-grade) projection, as the
                              reference's `resid` does by Householder QR (src/wls.jl:221-241)                               */
} blmm_status;

/* ---- library / context ------------------------------------------------------------------ */
int blmm_version(void);
int blmm_device_count(void);
/* Creates a context on HIP device `device_id`.
 *   hip_stream == NULL             : the library creates a PRIVATE non-blocking stream; nothing the caller enqueues on
 *                                    any other stream (the legacy default stream included) is ordered against the calls.
 *   hip_stream == BLMM_STREAM_NULL : adopt the legacy default ("null") stream, handle 0 -- what torch.cuda's default
 *                                    stream is.  The handle 0 itself cannot be passed because it reads as NULL.
 *   otherwise                      : a hipStream_t of the caller; every *_dev call enqueues on it. */
#define BLMM_STREAM_NULL ((void*)(intptr_t)-1)
int blmm_create(int device_id, void* hip_stream, blmm_ctx** out);
void blmm_destroy(blmm_ctx* ctx);
const char* blmm_last_error(const blmm_ctx* ctx);
const char* blmm_err_string(int code);
int blmm_set_stream(blmm_ctx* ctx, void* hip_stream);
/* on = 1: HIP events are recorded on the context's stream at every phase boundary of each bulkscan / scan call
 * (no synchronisation).  blmm_status then carries the LAST call's phase times, and blmm_read_timings() returns the
 * SUM over all calls since the previous read together with their count (it synchronises the stream). */
int blmm_set_timing(blmm_ctx* ctx, int on);
/* sums_ms[6] = {eigen, rotate, h2, prep, scan, total}; *ncalls = calls accumulated. */
int blmm_read_timings(blmm_ctx* ctx, double* sums_ms, int64_t* ncalls);
/* What the last null-exact call EXECUTED in its low-rank weights form (kernels_lowrank.hip; it synchronises the stream):
 * out[18] = {segments of the heritability axis with traits, traits of the shared-weights class (no basis: 2 n flop per test),
 * then per segment s: traits, rank R_s of its weight basis (2 (n + (1 + c) 4 ceil(R_s / 4)) flop per test)}.  A diagnostic for
 * benchmarks that price the executed arithmetic (bench.py); the reference has no counterpart. */
int blmm_lowrank_profile(blmm_ctx* ctx, int64_t* out);
/* Where each trait sat in that call's data-dependent panel layout (two regions split by the h2 search's hand-over; in each the
 * shared-weights class from the front, the weight-basis segments from the back): col_out[j] = panel column of trait j (-1: none),
 * *region_width = columns per region (region = col / width), counts_out[4] = {shared-weights traits, columns of the other class}
 * of region 0, then of region 1.  For tests that report the class / region of their worst entry. */
int blmm_lowrank_columns(blmm_ctx* ctx, int64_t m, int32_t* col_out, int64_t* region_width, int64_t* counts_out);
int blmm_synchronize(blmm_ctx* ctx);
/* ---- tuning: the switches that select another ARITHMETIC path are properties of the context (they were BLMM_* environment
 * variables up to 0.2.2; the environment is now read only under BLMM_DEV_ENV=1, for A/B timing by developers).  Keys and defaults:
 *   "lr_tol"          1e-13  relative residual of the weight-basis expansion above which a trait's LOD column is recomputed from
 *                            the full-length sums, and the tolerance of the shared-weights class (0: every trait re-scanned)
 *   "illcond_rho"     1e-4   pivot-share threshold of the conditioning guard (0: off; 2: every trait with >= 2 covariates re-scanned)
 *   "exact_full_rank" 0      1: null-exact through the full-rank kernel (2n(2+c) flop per test) instead of the low-rank weights form
 *   "pval_libm"       0      1: -log10 p through erfc / erfcx / log instead of the bucketed polynomials (chisq_df = 1)
 *   "pval_fused"      1      0: output_pvals as a pass over the finished L instead of a second output of the scan epilogues
 *   "lr_segments"     0      weight bases per heritability axis: 0 = default (six for n <= 80, else one), 1, or 2..8 equal segments
 *   "lr_shared"       1      0: no shared-weights class (traits with h2 = 0 go through the rank-R form like the others)
 *   "lr_split"        -1     split h2 search / two panel regions: -1 = from 8192 traits on, 0 never, 1 always
 *   "eigen_solver"    0      0 = by n; 1 = Jacobi; 2 = tridiagonalisation + divide and conquer
 *   "f32_rotation"    1      blmm_scan_perms_f32 with an intercept-only null model: 1 = the marker rotation runs on the fp32 matrix
 *                            cores as well; 0 = fp64 rotation, converted (0.2.2)
 *   "bulk_perm_cols"  0      blmm_bulkscan_perms: largest trait chunk in panel columns (0: sized by the workspace budget); results do
 *                            not depend on it
 *   "mdf_red_chunk"   0      blmm_bulkscan_multidf_reduced: flagged traits re-scanned per chunk of the scratch (0: a 64 MiB scratch);
 *                            results do not depend on it
 *   "cond_red_chunk"  0      blmm_bulkscan_stepwise: flagged traits re-scanned per chunk of the scratch (0: a 64 MiB scratch); results
 *                            do not depend on it.  A round enqueues ceil(active traits / chunk) launch pairs whatever the guard
 *                            lists (those beyond its list return at once), so small values are for tests only
 *   "defaults"               (set only) every key back to its default
 * Every setting gives results within the library's stated tolerances; they exist for tests and for A/B measurements. */
int blmm_set_tuning(blmm_ctx* ctx, const char* key, double value);
int blmm_get_tuning(const blmm_ctx* ctx, const char* key, double* value);
void blmm_default_opts(blmm_opts* o); /* bulkscan() defaults: null-grid, ML, prior (1.0, 0.0), eigen */

/* ---- pinned host memory for the outputs of the host-pointer entry points ------------------------------------------
 * L is p x m doubles (2.08 GB at BXD size) and has to cross ONE PCIe link: into a pinned destination it moves at link
 * rate in one asynchronous copy; into pageable memory the library pipelines 32 MB pieces through its own pinned ring
 * and copies them out with a few host threads.  A Julia caller either wraps blmm_host_alloc memory (unsafe_wrap) or
 * registers the Array it already has; both are optional. */
int blmm_host_register(void* p, uint64_t bytes);
int blmm_host_unregister(void* p);
void* blmm_host_alloc(uint64_t bytes);
void blmm_host_free(void* p);

/* ---- readers for the file formats the reference reads (host code, no GPU needed) ----------------------------------
 * blmm_read_csv: numeric CSV; `skip_lines` leading lines are dropped, then of every line the fields first_col, first_col +
 * col_step, ... (0-based) up to the last `drop_last` fields are parsed: readGenoProb = (1, 1, 1, 0),
 * readGenoProb_ExcludeComplements = (1, 1, 2, 0), readBXDpheno = (1, 1, 1, 1), readBXDgeno = (1, 1, 2, 0)
 * (src/readData.jl:41-96, 159-165).  blmm_read_he: Helium .he (test/kinship_test.jl:5).  The table is column-major;
 * blmm_table_copy writes it into the caller's rows x cols buffer (which may be pinned: blmm_host_alloc). */
typedef struct blmm_table blmm_table;
int blmm_read_csv(const char* path, int64_t skip_lines, int64_t first_col, int64_t col_step, int64_t drop_last, blmm_table** out);
int blmm_read_he(const char* path, blmm_table** out);
int64_t blmm_table_rows(const blmm_table* t);
int64_t blmm_table_cols(const blmm_table* t);
int blmm_table_copy(const blmm_table* t, double* dst);
void blmm_table_free(blmm_table* t);

/* ---- calcKinship(G)  (src/kinship.jl:4-14) ----------------------------------------------- */
int blmm_kinship(blmm_ctx* ctx, const double* G, int64_t n, int64_t p, double* K_out);
int blmm_kinship_dev(blmm_ctx* ctx, const double* dG, int64_t n, int64_t p, double* dK_out);
/* round.(calcKinship(G), digits = d) on the device, the convention of README.md:176-181 and test/generate_test_bxdData.jl:14
 * (Julia / NumPy: round(x * 10^d) / 10^d, ties to even); digits < 0: no rounding */
int blmm_kinship_rounded(blmm_ctx* ctx, const double* G, int64_t n, int64_t p, int64_t digits, double* K_out);
/* Leave-one-chromosome-out kinships: the markers of G (n x p) form nchr >= 2 contiguous chromosomes, chromosome c being columns
 * chr_start[c] .. chr_start[c + 1] - 1 (chr_start: nchr + 1 HOST int64 entries, 0 = chr_start[0] < chr_start[1] < .. <
 * chr_start[nchr] = p).  K_out (n x n x nchr; matrix c at K_out + c n n) gets calcKinship(G[:, not chromosome c]):
 * 2 (sum over d != c of S_d) / (p - p_c) + 1/2, diagonal 1, with S_d = X_d X_d' (X = G - 1/2) -- all of them from ONE pass over G
 * (one kinship's worth of FMAs), the other chromosomes' blocks summed in a fixed order (no S - S_c, no atomics).  digits >= 0:
 * each matrix rounded as blmm_kinship_rounded; < 0: not rounded.  Bad offsets (an empty chromosome, not increasing from 0 to p,
 * nchr < 2 or > 65535): BLMM_ERR_INVALID before anything is uploaded.  Workspace besides the output: the per-chromosome partial
 * sums, at most the larger of 256 MiB and the output's own size (nchr n^2 doubles).  The _dev form: device G / K_out, enqueued on
 * the context's stream without waiting for it (the offsets go through a pinned staging slot of the context). */
int blmm_kinship_loco(blmm_ctx* ctx, const double* G, int64_t n, int64_t p, const int64_t* chr_start, int64_t nchr,
                      int64_t digits, double* K_out);
int blmm_kinship_loco_dev(blmm_ctx* ctx, const double* dG, int64_t n, int64_t p, const int64_t* chr_start, int64_t nchr,
                          int64_t digits, double* dK_out);

/* ---- bulkscan(Y, G, [Covar], K; ...)  (src/bulkscan.jl:81-162, 188-314, 321-397, 428-526) --
 * Y n x m, G n x p, Covar n x ncov (NULL/0 = none: the intercept is the only null covariate),
 * K n x n, weights n (NULL = missing), h2_grid ngrid doubles in HOST memory for both variants
 * (ignored by null-exact).
 * Outputs: L p x m (column j = trait j, leading dimension ldL >= p); h2_out: m doubles
 * (h2_null_list; null-exact / null-grid) or p x m, ld = p (h2_panel; alt-grid).
 * blmm_bulkscan with L_out == NULL: the matrix is not copied to the host; it stays in the context's workspace, where
 * blmm_last_lod_colmax / blmm_last_lod_threshold / blmm_last_get_thresholds / blmm_last_log10p / blmm_last_lod_columns serve it
 * until the next call that produces a matrix (alt-grid: h2_out may be NULL likewise). */
int blmm_bulkscan(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G,
                  int64_t p, const double* Covar, int64_t ncov, const double* K, const double* weights,
                  const double* h2_grid, int64_t ngrid, double* L_out, double* h2_out, blmm_status* status);
int blmm_bulkscan_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m,
                      const double* dG, int64_t p, const double* dCovar, int64_t ncov, const double* dK,
                      const double* dweights, const double* h2_grid_host, int64_t ngrid, double* dL_out,
                      int64_t ldL, double* dh2_out, blmm_status* status);

/* ---- bulkscan WITHOUT the LOD matrix.  What the reference's users do with L is reduce it: the peak LOD of every
 * trait and its marker, the (marker, trait) pairs above a threshold (README.md:246-255, 354-359;
 * src/analysis_helpers/single_trait_analysis.jl:13-23).  Here the scan kernels do that in their epilogues and L is never
 * written (2.08 GB of HBM writes and 36 ms of PCIe at BXD size):
 *   colmax[j]  = max_i L[i, j],  argmax[j] = the lowest such i (0-based; -1: no finite-comparable entry)   -- m each, or NULL
 *   want_triplets != 0: every (i, j) with L[i, j] > thr as (ti, tj, tlod), order unspecified; *count = how many exist, the first
 *   `cap` of them are stored (call again with a larger cap when *count > cap)
 * bit-identical to blmm_lod_colmax_dev / blmm_lod_threshold_dev on the matrix blmm_bulkscan_dev writes.  The pointers inside
 * `out` are HOST pointers for blmm_bulkscan_reduced and DEVICE pointers for blmm_bulkscan_reduced_dev; h2_out as in
 * blmm_bulkscan (null-exact / null-grid: m; alt-grid: not written, may be NULL).  null-grid, and null-exact with up to 3 null
 * covariates, run fused; alt-grid, more covariates, or a call in which a trait needs one of the per-trait re-scans
 * (blmm_status.lowrank_fallback / n_illcond_rescan > 0) go through a matrix that stays in the context's workspace -- same results,
 * and the blmm_last_* consumers then serve that matrix.  blmm_last_reduced_route: 1 fused, 2 through the resident matrix.
 * Both forms return when the results are complete (they synchronise the stream). */
typedef struct blmm_reduced {
  double* colmax;
  int64_t* argmax;
  int64_t want_triplets;
  double thr;
  int64_t cap;
  int32_t* ti;
  int32_t* tj;
  double* tlod;
  int64_t* count;
} blmm_reduced;
int blmm_bulkscan_reduced(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G,
                          int64_t p, const double* Covar, int64_t ncov, const double* K, const double* weights,
                          const double* h2_grid, int64_t ngrid, const blmm_reduced* out, double* h2_out, blmm_status* status);
int blmm_bulkscan_reduced_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG,
                              int64_t p, const double* dCovar, int64_t ncov, const double* dK, const double* dweights,
                              const double* h2_grid_host, int64_t ngrid, const blmm_reduced* out, double* dh2_out,
                              blmm_status* status);
int blmm_last_reduced_route(const blmm_ctx* ctx);
/* Diagnostic for tests: which parts of the shortened null-exact front the context's last call took.  Bit 0: the weight basis was
 * built behind the eigenvalue kernel, ahead of the eigen phase's end; bit 1: the traits were rotated inside the h2 search's kernel;
 * bit 2: unused; bit 3: the device rejected the fast eigen path and the basis was rebuilt from the Jacobi's eigenvalues (reported by
 * the basis kernel itself).  Waits for the context's stream.  Negative: an error code. */
int blmm_last_front_route(blmm_ctx* ctx);

/* Stream-ordered form of blmm_bulkscan_reduced_dev (same arguments; `out` and dh2_out hold DEVICE pointers): the call only
 * enqueues on the context's stream and returns -- in steady state (the shapes of the previous call on this context) it makes
 * no host-blocking HIP call, so a caller can enqueue step k+1 while step k runs.  The results, *out->count and the info block
 * are valid once that stream has reached the end of the call (blmm_synchronize, or a wait on the caller's stream).  When a
 * workspace buffer has to grow the call may synchronise, as every entry point does.
 * Routes (dinfo[BLMM_RINFO_ROUTE]):
 *   1  fused: the scan epilogues reduce (as route 1 of blmm_bulkscan_reduced_dev); no trait was flagged;
 *   2  through the context's resident matrix + k_colmax / k_threshold (alt-grid, c >= 4 null covariates, tuning
 *      exact_full_rank, p = 0 or m = 0); the blmm_last_* consumers then serve that matrix;
 *   3  fused, and the traits a guard flagged (weight-basis residual: k_scan_fix; conditioning: k_scan_qr) were re-scanned on
 *      the device into the reduction -- no second run, no host round trip.
 * Routes 1 and 3 leave no resident matrix (blmm_last_dims reports none).  Maxima, arg-maxima, the triplet count and the stored
 * triplets are bit-identical to blmm_lod_colmax_dev / blmm_lod_threshold_dev on the matrix blmm_bulkscan_dev writes under the
 * same tuning; *count is exact also when it exceeds cap (then `cap` genuine, distinct triplets are stored; order unspecified).
 * A pending blmm_set_log10p_output request is refused (BLMM_ERR_INVALID) and consumed.  Argument errors return before anything
 * is enqueued.  The conditions blmm_status reports arrive in the info block instead (dinfo may be NULL):
 *   dinfo[BLMM_RINFO_LEN] (int64, device memory), written on the stream when the call's work completes:
 *     ROUTE             1 / 2 / 3 above
 *     LOWRANK_RESCAN    traits re-scanned because the weight-basis expansion residual was above lr_tol (blmm_status.lowrank_fallback)
 *     ILLCOND_RESCAN    traits re-scanned because the weighted null design was ill-conditioned (blmm_status.n_illcond_rescan)
 *     NAN_LOD, ZERO_NORM, NEG_EIG, NONPOS_WEIGHT   as blmm_status.n_nan_lod / n_zero_norm / n_neg_eig / n_nonpos_weight
 *     TRIPLETS          *count (0 when no triplets were asked for)
 *     DEVICE_ERROR      0; -1: the weight-basis kernel timed out at its grid barrier; -7 / -8: the eigensolver gave up (as
 *                       blmm_status' failure); the next blmm_synchronize / call on the context then returns BLMM_ERR_HIP */
#define BLMM_RINFO_LEN 9
enum { BLMM_RINFO_ROUTE = 0, BLMM_RINFO_LOWRANK_RESCAN, BLMM_RINFO_ILLCOND_RESCAN, BLMM_RINFO_NAN_LOD, BLMM_RINFO_ZERO_NORM,
       BLMM_RINFO_NEG_EIG, BLMM_RINFO_NONPOS_WEIGHT, BLMM_RINFO_TRIPLETS, BLMM_RINFO_DEVICE_ERROR };
int blmm_bulkscan_reduced_async(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG,
                                int64_t p, const double* dCovar, int64_t ncov, const double* dK, const double* dweights,
                                const double* h2_grid_host, int64_t ngrid, const blmm_reduced* out, double* dh2_out,
                                int64_t* dinfo);

/* ---- the pipeline in three calls, for hosts that run ONE PROCESS PER GPU (torch.distributed, MPI; bench.py --gpus N):
 * blmm_bulkscan_dev on every rank repeats the rotation of the whole G (10-25 % of a rank's step at n >= 500).  Instead every
 * rank prepares (design, eigen-decomposition, rotation matrix: replicated, as the reference's transform_rotation is one call,
 * src/transform_helpers.jl:21-34), rotates ITS column block of G, the host all-gathers the k-major blocks (RCCL over xGMI), and
 * the scan takes the gathered blocks.  Bit-identical to blmm_bulkscan_dev.
 *   blmm_prepare_dev              K n x n, Covar n x ncov (NULL/0: intercept only), weights n (NULL: missing)
 *   blmm_rotated_rows             rows of a rotated block (n rounded up to 8); 0 before blmm_prepare_dev
 *   blmm_rotate_block_dev         dG_block n x pb (column-major) -> dXt_block rows x ld (k-major: row k contiguous), ld >= pb
 *   blmm_bulkscan_prerotated_dev  dXt_blocks = nblocks consecutive blocks of rows x block_ld doubles, block b = the markers
 *                                 [b block_cols, min(p, (b+1) block_cols)); dY n x m = this rank's traits; outputs as blmm_bulkscan_dev
 *   blmm_scan_perms_prerotated_dev  the permutation test (blmm_scan_perms[_f32]_dev) on the same gathered blocks: this rank's
 *                                 nperms permutations against all p markers; exactly one of dLperms_out (fp64) / dLperms32_out (fp32) */
int blmm_prepare_dev(blmm_ctx* ctx, const blmm_opts* opts, int64_t n, const double* dCovar, int64_t ncov, const double* dK,
                     const double* dweights, blmm_status* status);
int64_t blmm_rotated_rows(const blmm_ctx* ctx);
int blmm_rotate_block_dev(blmm_ctx* ctx, const double* dG_block, int64_t pb, double* dXt_block, int64_t ld);
int blmm_bulkscan_prerotated_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t m, int64_t p,
                                 const double* dXt_blocks, int64_t nblocks, int64_t block_cols, int64_t block_ld,
                                 const double* h2_grid_host, int64_t ngrid, double* dL_out, int64_t ldL, double* dh2_out,
                                 blmm_status* status);
int blmm_scan_perms_prerotated_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dy, int64_t p, const double* dXt_blocks,
                                   int64_t nblocks, int64_t block_cols, int64_t block_ld, int64_t nperms, uint64_t seed,
                                   const int32_t* dperm_idx, double* dscalars_out, double* dlod_out, double* dLperms_out,
                                   float* dLperms32_out, blmm_status* status);

/* ---- the same call over several GPUs of one node (north_star: traits shard across the GPUs) -----------------------
 * Replaces the reference's thread blocking over contiguous trait ranges (src/bulkscan.jl:263-309): device r of R scans
 * the column block [r*ceil(m/R), min(m, (r+1)*ceil(m/R))) (blmm_multi_shard) and owns that block of the column-major
 * L.  One host worker thread per device; G/K/Covar/weights are replicated; no collective on the data path.
 *   gather_mode  BLMM_GATHER_HOST_SHARDS (default): every device copies its block straight into the caller's L_out /
 *                  h2_out over its own PCIe link -- the reference's result, L in host memory; L_out == NULL: the blocks stay in
 *                  HBM and blmm_multi_last_colmax / blmm_multi_last_lod_threshold reduce them there;
 *                BLMM_GATHER_NONE: the blocks stay in HBM (blmm_multi_device_result); L_out / h2_out may be NULL
 *                  (when given they are filled as well);
 *                BLMM_GATHER_ALLGATHER: an RCCL all-gather over xGMI leaves the FULL p x m matrix (ld = p, columns
 *                  padded to R*ceil(m/R)) on every device; librccl.so is loaded on first use.
 * status: NULL or an array of blmm_multi_ndev() entries, one per device.
 * device_ids == NULL or ndev <= 0: every visible device.  A device id may be repeated (several shards on one GPU). */
typedef struct blmm_multi blmm_multi;
enum blmm_gather { BLMM_GATHER_NONE = 0, BLMM_GATHER_HOST_SHARDS = 1, BLMM_GATHER_ALLGATHER = 2 };
typedef struct blmm_multi_opts {
  int32_t gather_mode; /* blmm_gather */
  int32_t reserved;
} blmm_multi_opts;
int blmm_create_multi(const int* device_ids, int ndev, blmm_multi** out);
void blmm_destroy_multi(blmm_multi* mc);
int blmm_multi_ndev(const blmm_multi* mc);
const char* blmm_multi_last_error(const blmm_multi* mc);
void blmm_default_multi_opts(blmm_multi_opts* o);
void blmm_multi_shard(int64_t m, int rank, int ndev, int64_t* lo, int64_t* hi);
int blmm_bulkscan_multi(blmm_multi* mc, const blmm_opts* opts, const blmm_multi_opts* mopts, const double* Y, int64_t n,
                        int64_t m, const double* G, int64_t p, const double* Covar, int64_t ncov, const double* K,
                        const double* weights, const double* h2_grid, int64_t ngrid, double* L_out, double* h2_out,
                        blmm_status* status);
/* Consumers of the last blmm_bulkscan_multi call's blocks WHERE THEY ARE (any gather mode; with host_shards and L_out == NULL the
 * matrix never leaves the devices): per-trait maxima (max_out m, argmax_out m or NULL) and LOD > thr triplets with global trait
 * indices, every device reducing its own block (the rules of blmm_lod_colmax / blmm_lod_threshold). */
int blmm_multi_last_colmax(blmm_multi* mc, double* max_out, int64_t* argmax_out);
int blmm_multi_last_lod_threshold(blmm_multi* mc, double thr, int64_t cap, int32_t* i_out, int32_t* j_out, double* lod_out,
                                  int64_t* count_out);
/* Device-resident result of the last blmm_bulkscan_multi with gather_mode none / allgather on device `rank`:
 * *dL (ld *ldL) holds the columns [*col_lo, *col_hi) of L, *dh2 the matching h2 entries. */
int blmm_multi_device_result(blmm_multi* mc, int rank, double** dL, int64_t* ldL, int64_t* col_lo, int64_t* col_hi,
                             double** dh2);

/* ---- scan(y, G, [Covar], K; permutation_test=true)  (src/scan.jl:485-557) ------------------
 * perm_idx: n x nperms int32, 0-based, column b = permutation b (r0perm[:, b+1] = r0[perm_idx[:, b]]);
 * NULL = the library draws them from its own counter-based generator seeded by `seed`
 * (Julia's MersenneTwister stream is not reproducible outside Julia).
 * Outputs: scalars[0] = sigma2_e, scalars[1] = h2_null; lod_out p; Lperms_out p x nperms (ld = p). */
int blmm_scan_perms(blmm_ctx* ctx, const blmm_opts* opts, const double* y, int64_t n, const double* G, int64_t p,
                    const double* Covar, int64_t ncov, const double* K, const double* weights, int64_t nperms,
                    uint64_t seed, const int32_t* perm_idx, double* scalars_out, double* lod_out,
                    double* Lperms_out, blmm_status* status);
int blmm_scan_perms_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dy, int64_t n, const double* dG,
                        int64_t p, const double* dCovar, int64_t ncov, const double* dK, const double* dweights,
                        int64_t nperms, uint64_t seed, const int32_t* dperm_idx, double* dscalars_out,
                        double* dlod_out, double* dLperms_out, blmm_status* status);

/* fp32 permutation matrix (BASELINE.json configs[4]): the null model (eigen-decomposition, h2, residuals, panel construction)
 * stays fp64; the marker rotation and the p x nperms contraction run on the fp32 matrix cores and Lperms_out is float
 * (p x nperms, ld = p).  Expected agreement with the fp64 path: |d| <= 1e-3 |ref| + 1e-4.  The original trait's lod_out keeps an
 * fp64 numerator (taken from G itself); its marker norms come from the fp32-rotated markers, so it agrees with blmm_scan_perms'
 * lod_out to ~1e-7 relative, not bit for bit.  With null covariates beyond the intercept (or tuning "f32_rotation" = 0) the
 * rotation is the fp64 one, converted, and lod_out is blmm_scan_perms' bit for bit. */
int blmm_scan_perms_f32(blmm_ctx* ctx, const blmm_opts* opts, const double* y, int64_t n, const double* G, int64_t p,
                        const double* Covar, int64_t ncov, const double* K, const double* weights, int64_t nperms,
                        uint64_t seed, const int32_t* perm_idx, double* scalars_out, double* lod_out,
                        float* Lperms_out, blmm_status* status);
int blmm_scan_perms_f32_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dy, int64_t n, const double* dG,
                            int64_t p, const double* dCovar, int64_t ncov, const double* dK, const double* dweights,
                            int64_t nperms, uint64_t seed, const int32_t* dperm_idx, double* dscalars_out,
                            double* dlod_out, float* dLperms_out, blmm_status* status);

/* ---- the permutation test for EVERY trait of a bulk call: genome-wide thresholds and p-values per trait -----------------
 * For each trait j of Y (n x m) the reference's scan_perms_lite (src/scan.jl:485-557) under the trait's own null heritability,
 * reduced on the device -- the p x m x nperms LOD tensor is never written.  ONE permutation set serves every trait: perm_idx
 * (n x nperms int32, 0-based, as blmm_scan_perms; entries in 0 .. n - 1) or, NULL, the library's generator seeded by `seed`.  So
 * trait j equals blmm_scan_perms(Y[:, j], same nperms / seed / perm_idx) bit for bit, and the correlation between traits within a
 * permutation is kept.  Null model as blmm_scan_perms (opts: reml, prior, optim_interval, add_intercept, decomp_scheme; Covar,
 * weights); 1 .. 8 null covariates incl. the intercept (more: BLMM_ERR_UNSUPPORTED); nperms 0 .. 16384 (more: BLMM_ERR_UNSUPPORTED;
 * < 0: BLMM_ERR_NPERMS); probs: nprobs (0 .. 64) quantile levels in HOST memory, 1 - signif_level as for blmm_get_thresholds.
 * Outputs (m each unless stated):
 *   h2_out, sigma2_out    the null fit (scan's h2_null, sigma2_e)
 *   lod_max_out           peak of the unpermuted LOD column; lod_argmax_out its marker (0-based, lowest on ties, NaN never the
 *                         maximum; -inf / -1 for a column without a comparable LOD, as blmm_lod_colmax)
 *   max_perms_out         nperms x m (ld = nperms): genome-wide maximum LOD of every permuted copy (or NULL)
 *   thr_out               nprobs x m (ld = nprobs): blmm_get_thresholds of the trait's permutation matrix (or NULL)
 *   pval_out              (1 + #{k : max_perms[k, j] >= lod_max[j]}) / (nperms + 1), a -inf maximum never counted (or NULL)
 *   nperms = 0: thresholds and p-values are NaN.
 * Traits run in chunks of at most 65535 traits, sized by a 4 GiB workspace budget (tuning key "bulk_perm_cols": the largest chunk
 * in panel columns, traits x (nperms + 1); 0 = the budget).  blmm_bulkscan_perms_dev: device pointers (probs still host), ordered
 * on the context's stream; with a status it synchronises, as blmm_scan_perms_dev.  The host form synchronises. */
int blmm_bulkscan_perms(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                        const double* Covar, int64_t ncov, const double* K, const double* weights, int64_t nperms, uint64_t seed,
                        const int32_t* perm_idx, const double* probs, int64_t nprobs, double* h2_out, double* sigma2_out,
                        double* lod_max_out, int64_t* lod_argmax_out, double* max_perms_out, double* thr_out, double* pval_out,
                        blmm_status* status);
int blmm_bulkscan_perms_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                            const double* dCovar, int64_t ncov, const double* dK, const double* dweights, int64_t nperms,
                            uint64_t seed, const int32_t* dperm_idx, const double* probs, int64_t nprobs, double* dh2_out,
                            double* dsigma2_out, double* dlod_max_out, int64_t* dlod_argmax_out, double* dmax_perms_out,
                            double* dthr_out, double* dpval_out, blmm_status* status);

/* ---- leave-one-chromosome-out (LOCO) bulkscan -----------------------------------------------------------------------------
 * The markers of chromosome c (columns chr_start[c] .. chr_start[c + 1] - 1 of G; chr_start as for blmm_kinship_loco) are scanned
 * against the kinship of every OTHER chromosome: for each c, rows chr_start[c] .. of L are
 *   blmm_bulkscan(Y, G[:, chromosome c], K_{-c}; same opts / Covar / weights / grid).L
 * bit for bit, with K_{-c} = blmm_kinship_loco(G, chr_start, kinship_digits)[c].  Y, G, Covar and the weights go up once; the
 * kinships come from one pass over G; then every chromosome runs the bulkscan pipeline on its column block (design, eigen,
 * rotation, h2, panels, scan) into its rows of ONE p x m L.  The chromosomes share the context's workspace and run one after the
 * other in stream order; no host synchronisation between them.
 *   L_out      p x m, or NULL: L stays resident in the context (blmm_last_dims = (p, m), blmm_last_lod_colmax, .._threshold,
 *              .._columns, blmm_last_log10p see the whole genome)
 *   h2_out     null-* methods: nchr blocks of m (block c = chromosome c's h2_null_list, at h2_out + c m); alt-grid: the p x m
 *              h2_panel (may be NULL then, as for blmm_bulkscan)
 *   status     summed over the chromosomes (counts and phase times; lowrank_rank and lowrank_resid: the largest).  t_eigen_ms
 *              holds the batched eigen phase (n <= 124) and every chromosome's post-eigen work; t_total_ms spans the whole
 *              call, including kinships computed inside it, which count in no phase.  blmm_lowrank_profile /
 *              blmm_lowrank_columns afterwards describe the last chromosome run (the chromosomes run largest first).
 * Refused with BLMM_ERR_INVALID before anything is uploaded: nchr < 2 or > 65535, an empty chromosome, offsets not increasing
 * from 0 to p, a chromosome holding every marker; n > 2048 as blmm_bulkscan.  A pending blmm_set_log10p_output request is
 * honoured by a column pass over the finished L.
 * The _dev form: device Y / G / Covar / weights, dK_loco (n x n x nchr as blmm_kinship_loco_dev writes it) or NULL: computed with
 * kinship_digits; dL_out p x m with leading dimension ldL >= p; dh2_out as h2_out (the alt-grid h2_panel with leading dimension p).
 * It enqueues on the context's stream and waits for it only for a status and, as blmm_bulkscan_dev does, to copy the null-grid /
 * alt-grid h2_grid out of host memory. */
int blmm_bulkscan_loco(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                       const int64_t* chr_start, int64_t nchr, int64_t kinship_digits, const double* Covar, int64_t ncov,
                       const double* weights, const double* h2_grid, int64_t ngrid, double* L_out, double* h2_out,
                       blmm_status* status);
int blmm_bulkscan_loco_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                           const int64_t* chr_start, int64_t nchr, int64_t kinship_digits, const double* dCovar, int64_t ncov,
                           const double* dweights, const double* h2_grid, int64_t ngrid, const double* dK_loco, double* dL_out,
                           int64_t ldL, double* dh2_out, blmm_status* status);

/* LOCO without the LOD matrix: what blmm_bulkscan_reduced is to blmm_bulkscan, plus every chromosome's peak (the cis / trans table
 * of an eQTL study).  Stated against the L that blmm_bulkscan_loco writes under the same opts, tuning and inputs, bit for bit:
 *   out            as blmm_bulkscan_reduced: colmax / argmax (m each, or NULL) = blmm_lod_colmax of the whole L (argmax: the lowest
 *                  global 0-based marker; -inf / -1 for a column with no comparable entry; NaN is never the maximum); triplets =
 *                  the set blmm_lod_threshold gives on L (global marker indices), *count exact also beyond cap (then `cap` genuine,
 *                  distinct triplets are stored; order unspecified)
 *   chr_max_out / chr_argmax_out   nchr blocks of m (block c at + c m, the layout of h2_out), or NULL: blmm_lod_colmax of rows
 *                  chr_start[c] .. chr_start[c + 1] - 1, the argmax still a GLOBAL marker index
 *   h2_out         null-* methods: as blmm_bulkscan_loco (nchr x m); alt-grid: not written, may be NULL
 *   status         summed over the chromosomes, as blmm_bulkscan_loco
 * Refused as blmm_bulkscan_loco (chromosome offsets, n > 2048, NULL buffers) plus blmm_bulkscan_reduced's triplet-buffer checks,
 * before anything is uploaded; a pending blmm_set_log10p_output request is refused (BLMM_ERR_INVALID) and consumed.
 * Every chromosome runs blmm_bulkscan_loco's pipeline.  null-grid, and null-exact in the low-rank weights form (up to 3 null
 * covariates), reduce in the scan epilogues into the chromosome's own partials; traits a guard flags are re-scanned into them on
 * the device; one final kernel gives the chromosome tables and their merge.  alt-grid, c >= 4 and tuning exact_full_rank scan each
 * chromosome into a resident block of the largest chromosome's rows and reduce it there.  No p x m matrix is allocated, and none is
 * left resident (blmm_last_dims reports none).  blmm_last_reduced_route: 1 fused with no trait flagged, 3 fused with on-device
 * re-scans, 2 through the per-chromosome block; the _dev form reports 0 for a fused call made without a status (it has not waited
 * for the counts that tell 1 from 3).
 * The _dev form: device Y / G / Covar / weights / out / tables / h2 and dK_loco as blmm_bulkscan_loco_dev; it only enqueues on the
 * context's stream, and waits for it only for a status or to copy a host h2_grid. */
int blmm_bulkscan_loco_reduced(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                               const int64_t* chr_start, int64_t nchr, int64_t kinship_digits, const double* Covar, int64_t ncov,
                               const double* weights, const double* h2_grid, int64_t ngrid, const blmm_reduced* out, double* chr_max_out,
                               int64_t* chr_argmax_out, double* h2_out, blmm_status* status);
int blmm_bulkscan_loco_reduced_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                                   const int64_t* chr_start, int64_t nchr, int64_t kinship_digits, const double* dCovar, int64_t ncov,
                                   const double* dweights, const double* h2_grid, int64_t ngrid, const double* dK_loco, const blmm_reduced* out,
                                   double* dchr_max_out, int64_t* dchr_argmax_out, double* dh2_out, blmm_status* status);

/* ---- the LOCO permutation test: blmm_bulkscan_perms under every chromosome's LOCO kinship, and genome-wide tables ------------
 * With K_c = blmm_kinship_loco(G, chr_start, kinship_digits)[c] and ref_c = blmm_bulkscan_perms(Y, G[:, chromosome c], K_c; same opts /
 * Covar / weights / nperms / seed or perm_idx / probs), bit for bit:
 *   h2_out, sigma2_out    nchr blocks of m (block c at + c m): ref_c's h2 / sigma2
 *   chr_lod_max_out       nchr x m as h2_out: ref_c's lod_max; chr_lod_argmax_out: ref_c's lod_argmax + chr_start[c] (a GLOBAL
 *                         0-based marker; -1 stays -1)
 *   chr_max_perms_out     nchr blocks of nperms x m (block c at + c nperms m, ld = nperms): ref_c's max_perms (5.7 GB at the BXD shape
 *                         with 1000 permutations: NULL unless needed)
 *   chr_thr_out           nchr blocks of nprobs x m (at + c nprobs m, ld = nprobs): ref_c's thresholds; chr_pval_out nchr x m: ref_c's
 *                         p-values
 * and genome-wide, from those values exactly:
 *   max_perms_out         nperms x m (ld = nperms): max over c of chr_max_perms[c]
 *   lod_max_out           max over c of chr_lod_max; lod_argmax_out its global marker (the lowest on ties, whatever order the
 *                         chromosomes run in; NaN never the maximum; -inf / -1 for a trait without a comparable LOD)
 *   thr_out               nprobs x m: blmm_get_thresholds' rule (Julia's type 7) on max_perms[:, j]
 *   pval_out              (1 + #{b : max_perms[b, j] >= lod_max[j]}) / (nperms + 1), a -inf maximum never counted
 *   nperms = 0: thresholds and p-values are NaN.
 * Convention: ONE permutation set (perm_idx, or the generator seeded once by `seed`) serves every chromosome and trait.  Each
 * chromosome permutes its own rotated, reweighted null residuals, as scan_perms_lite (src/scan.jl:485-557) does under K_c, and the
 * genome-wide maximum of permutation b pairs the chromosomes' copies by b -- what a loop of blmm_bulkscan_perms over the chromosomes
 * gives, not one permutation of the individuals carried across chromosomes.
 * Y, G, Covar and weights go up once, the kinships come from one pass over G, the eigen phase is blmm_bulkscan_loco's (batched
 * for n <= 124), and the p x m x nperms LOD tensor is never written: each chromosome's trait chunks (blmm_bulkscan_perms' kernels)
 * reduce to column maxima that fold into a (nperms + 1) x m device buffer, summarised once after the last chromosome.
 * h2_out, sigma2_out, lod_max_out and lod_argmax_out are required; every other output may be NULL.  status: summed over the
 * chromosomes, as blmm_bulkscan_loco.  Refused before anything is uploaded: what blmm_bulkscan_loco refuses (chromosome offsets,
 * n > 2048) and what blmm_bulkscan_perms refuses (nperms < 0: BLMM_ERR_NPERMS; more than 16384 permutations or more than 8 null
 * covariates: BLMM_ERR_UNSUPPORTED; 0 .. 64 levels; perm_idx entries outside 0 .. n - 1 in the host form).
 * The _dev form: device Y / G / Covar / weights / perm_idx and outputs (probs and chr_start still host), dK_loco as
 * blmm_bulkscan_loco_dev (NULL: computed on the device).  It enqueues on the context's stream and waits for it only for a status. */
int blmm_bulkscan_loco_perms(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                             const int64_t* chr_start, int64_t nchr, int64_t kinship_digits, const double* Covar, int64_t ncov,
                             const double* weights, int64_t nperms, uint64_t seed, const int32_t* perm_idx, const double* probs,
                             int64_t nprobs, double* h2_out, double* sigma2_out, double* lod_max_out, int64_t* lod_argmax_out,
                             double* max_perms_out, double* thr_out, double* pval_out, double* chr_lod_max_out,
                             int64_t* chr_lod_argmax_out, double* chr_max_perms_out, double* chr_thr_out, double* chr_pval_out,
                             blmm_status* status);
int blmm_bulkscan_loco_perms_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                                 const int64_t* chr_start, int64_t nchr, int64_t kinship_digits, const double* dCovar, int64_t ncov,
                                 const double* dweights, int64_t nperms, uint64_t seed, const int32_t* dperm_idx, const double* probs,
                                 int64_t nprobs, const double* dK_loco, double* dh2_out, double* dsigma2_out, double* dlod_max_out,
                                 int64_t* dlod_argmax_out, double* dmax_perms_out, double* dthr_out, double* dpval_out,
                                 double* dchr_lod_max_out, int64_t* dchr_lod_argmax_out, double* dchr_max_perms_out, double* dchr_thr_out,
                                 double* dchr_pval_out, blmm_status* status);

/* ---- k-degree-of-freedom bulkscan: one test per LOCUS of k adjacent columns (F2 / dominance codings, founder probabilities) --
 * G is n x p with p = P k; locus l is the columns l k .. l k + k - 1.  Y, K, Covar / add_intercept, weights (their pre-scaling
 * scales every column of G), reml, the prior, optim_interval, decomp_scheme and h2_grid are used as blmm_bulkscan uses them, and
 * h2_out (m) is blmm_bulkscan's h2_null_list for the same method and options, bit for bit (the null model does not involve G).
 * For trait j, with s = sqrt(|w(h2_j)|) and the rotated data: y~ = s .* y0, Z~ = s .* Z0, x~_a = s .* (rotated column a of the
 * locus); e = the residual of y~ on span(Z~).  Rank rule: taking the locus columns in order, column a is kept iff the part r_a of
 * x~_a orthogonal to span(Z~) and to the kept columns before it has |r_a|^2 > BLMM_MULTIDF_TAU |x~_a|^2 -- complement columns
 * (probabilities summing to 1 beside the intercept), duplicated columns and absent genotypes drop out.  With Q = span of the kept
 * r_a, R^2 = |P_Q e|^2 / |e|^2 and
 *   L[l, j] = -(n/2) log10(1 - R^2)     (scan_null's (-n/2)(log10 rss1 - log10 rss0), src/scan.jl, with the design [Z, G_l]).
 * k = 1 is blmm_bulkscan's LOD except where the rule drops the column (a constant marker: LOD 0 here).  1 - R^2 = 0 gives +Inf,
 * R^2 > 1 or NaN gives NaN (counted in n_nan_lod); a trait with e = 0 is counted in n_zero_norm, as blmm_bulkscan does.
 *   L_out      P x m (ld = P), or NULL: L stays resident (blmm_last_dims = (P, m), blmm_last_lod_colmax, .._threshold, .._columns,
 *              blmm_last_log10p see it)
 *   status     as blmm_bulkscan fills it; n_illcond_rescan: null-exact traits whose columns the conditioning guard recomputed
 *              with an orthogonalised projection (c >= 2)
 * Limits: null-grid 1 <= k <= BLMM_MULTIDF_MAX_K_GRID, null-exact 1 <= k <= BLMM_MULTIDF_MAX_K_EXACT, at most
 * BLMM_MULTIDF_MAX_COVARIATES null covariates (incl. the intercept), n <= 2048.  Refused before anything is uploaded: k < 1 or p not
 * a multiple of k (BLMM_ERR_DIM); k above the method's limit, more covariates, alt-grid (BLMM_ERR_UNSUPPORTED); an unknown method
 * (BLMM_ERR_METHOD); n > 2048 (BLMM_ERR_UNSUPPORTED, blmm_bulkscan's message).  A pending blmm_set_log10p_output request is
 * honoured with the request's chisq_df, by a column pass over the finished L (callers pass chisq_df = the number of kept columns,
 * usually k, or k - 1 for complement columns).
 * Kernels (kernels_mdf.hip): null-grid forms per (grid point, locus) the factor of the locus's residual Gram, then one contraction
 * of the markers with the traits' residual panel, 2 n p m flop; null-exact contracts each (locus, trait) pair's numerators, weighted
 * Gram and covariate products and factors in the epilogue.
 * The _dev form: device Y / G / Covar / weights / L_out (ld ldL >= P) / h2_out; it enqueues on the context's stream and waits only
 * for a status or to copy the host h2_grid. */
#define BLMM_MULTIDF_TAU 1e-8
#define BLMM_MULTIDF_MAX_K_GRID 8
#define BLMM_MULTIDF_MAX_K_EXACT 4
#define BLMM_MULTIDF_MAX_COVARIATES 8
int blmm_bulkscan_multidf(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                          int64_t k, const double* Covar, int64_t ncov, const double* K, const double* weights,
                          const double* h2_grid, int64_t ngrid, double* L_out, double* h2_out, blmm_status* status);
int blmm_bulkscan_multidf_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG,
                              int64_t p, int64_t k, const double* dCovar, int64_t ncov, const double* dK, const double* dweights,
                              const double* h2_grid, int64_t ngrid, double* dL_out, int64_t ldL, double* dh2_out,
                              blmm_status* status);

/* ---- the k-degree-of-freedom scan WITHOUT the matrix: blmm_bulkscan_reduced's outputs for blmm_bulkscan_multidf's loci ----------
 * Arguments are blmm_bulkscan_multidf's with `out` (blmm_reduced; HOST pointers for the host form, DEVICE pointers for _dev) in
 * place of L_out / ldL; limits and refusals are blmm_bulkscan_multidf's, with its messages.  With P = p / k and L the matrix
 * blmm_bulkscan_multidf_dev writes for the same inputs and tuning:
 *   colmax[j] = max_l L[l, j]; argmax[j] = the lowest such LOCUS (0-based), -1 with colmax = -inf when the column has no comparable
 *   entry (P = 0, all NaN); a NaN is never the maximum, +Inf can be.  want_triplets: every (l, j) with L[l, j] > thr as (ti = locus,
 *   tj = trait, tlod), order unspecified; *count is exact also beyond cap, and then cap genuine, distinct triplets are stored.
 * Bit-identical to blmm_lod_colmax_dev / blmm_lod_threshold_dev on that L; h2_out is blmm_bulkscan_multidf's bit for bit and the
 * status counters (n_nan_lod: the NaNs of the matrix that is never written; n_illcond_rescan) equal its own.
 * No P x m buffer exists in any route: the scan kernels reduce every trait's 64 loci of a wave to a (maximum, locus) partial in their
 * epilogues (k_mdf_grid_red, k_mdf_exact_red), k_red_final finishes the maxima; null-exact traits the conditioning guard flags
 * (c >= 2) are left out there and recomputed by k_mdf_qr into a scratch of a chunk of the flagged list (64 MiB; tuning key
 * "mdf_red_chunk": flagged traits per chunk, results do not depend on it), reduced with the same rules.  blmm_last_reduced_route:
 * 1, or 3 when flagged traits were re-scanned.  blmm_last_dims reports no resident matrix afterwards.  A pending
 * blmm_set_log10p_output request is refused with BLMM_ERR_INVALID and consumed.  Both forms return when the results are complete. */
int blmm_bulkscan_multidf_reduced(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                                  int64_t k, const double* Covar, int64_t ncov, const double* K, const double* weights,
                                  const double* h2_grid, int64_t ngrid, const blmm_reduced* out, double* h2_out, blmm_status* status);
int blmm_bulkscan_multidf_reduced_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG,
                                      int64_t p, int64_t k, const double* dCovar, int64_t ncov, const double* dK, const double* dweights,
                                      const double* h2_grid, int64_t ngrid, const blmm_reduced* out, double* dh2_out,
                                      blmm_status* status);

/* ---- permutation thresholds of the k-degree-of-freedom scan: blmm_bulkscan_perms with blmm_bulkscan_multidf's loci -----------
 * Arguments and outputs are blmm_bulkscan_perms', plus k placed as in blmm_bulkscan_multidf (p = P k; locus l is the columns
 * l k .. l k + k - 1 of G).
 * Null model: h2_out and sigma2_out are blmm_bulkscan_perms' for the same inputs and options, bit for bit (the same design, eigen
 *   phase, trait rotation and Brent search; the null model does not involve G).  opts->method is ignored, as there.
 * Statistic: for trait j, s = sqrt(|makeweights(h2_j)|), Z~ = s .* Z0, r0 = s .* (y0_j - Z0 beta_j) (the reweighted null residual);
 *   permutation b gives v_b = r0[perm_b], and v_0 = r0.  With Q the span of the accepted residuals of the locus's weighted columns
 *   on span(Z~),
 *     L_b[l] = -(n/2) log10(1 - |P_Q (I - P_Z~) v_b|^2 / |v_b|^2)
 *   -- the k-df form of scan_perms_lite (src/scan.jl:485-557): the permuted vector is normalised by its own norm and the markers are
 *   residualised on the weighted covariates.  Rank rule: blmm_bulkscan_multidf's (BLMM_MULTIDF_TAU, in column order), at the
 *   trait's own weights.  At b = 0 this is blmm_bulkscan_multidf's null-exact LOD.  1 - R^2 = 0 gives +Inf, R^2 > 1 or NaN gives
 *   NaN; a constant locus has LOD 0 in every permutation (the rank rule drops it -- not the zero-norm error of blmm_bulkscan_perms);
 *   a trait with r0 = 0 is counted in n_zero_norm.  n_nan_lod counts the NaN LODs of the UNPERMUTED columns only (the number
 *   blmm_bulkscan_multidf would report for the data, whatever nperms is); a NaN in a permuted copy is never that copy's maximum and
 *   is not counted.
 * Outputs: lod_max_out, lod_argmax_out (a 0-based LOCUS index), max_perms_out (nperms x m), thr_out (nprobs x m) and pval_out follow
 *   blmm_bulkscan_perms' rules: ties go to the lowest index, NaN is never a maximum, a trait with no comparable entry (P = 0
 *   included) gets -inf and -1, and with nperms = 0 thresholds and p-values are NaN.
 * Permutations: ONE set for every trait -- perm_idx, or the library's generator from `seed`: the set blmm_bulkscan_perms draws for
 *   that seed.
 * Limits: 1 <= k <= BLMM_MULTIDF_MAX_K_GRID (the scan is the null-grid algebra at every trait's exact heritability: the factor
 *   table of blmm_bulkscan_multidf's null-grid form with the chunk's h2 values as its grid, one row per trait shared by the trait's
 *   nperms + 1 columns), at most BLMM_MULTIDF_MAX_COVARIATES null covariates, nperms 0 .. 16384, nprobs 0 .. 64, n <= 2048.
 * Refused before anything is uploaded: nperms < 0 (BLMM_ERR_NPERMS); NULL required buffers, bad levels and, in the host form,
 *   perm_idx entries outside 0 .. n - 1 (BLMM_ERR_INVALID); k < 1 or p not a multiple of k (BLMM_ERR_DIM); k above the limit, too
 *   many covariates or permutations, n > 2048 (BLMM_ERR_UNSUPPORTED).
 * No conditioning guard (blmm_bulkscan_perms has none either): the factor table forms Z0'WZ0 and factors it by Cholesky, so traits
 *   with several nearly collinear weighted covariates at h2 -> 1 carry the accuracy of normal equations, not that of
 *   blmm_bulkscan_multidf's orthogonalised null-exact re-scan.
 * The call leaves no resident matrix (blmm_last_* see none, as after blmm_bulkscan_perms) and drops a pending
 * blmm_set_log10p_output request.  The P x m x (nperms + 1) LOD tensor is never written: the scan kernel reduces every panel
 * column to per-64-loci (maximum, locus) partials in its epilogue.  Trait chunks as blmm_bulkscan_perms (tuning key
 * "bulk_perm_cols"; results do not depend on it), the budget counting the chunk's factor table, 8 k (k + 1) / 2 P bytes per trait.
 * The _dev form: device pointers (probs host), ordered on the context's stream; with a status it synchronises. */
int blmm_bulkscan_multidf_perms(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                                int64_t k, const double* Covar, int64_t ncov, const double* K, const double* weights, int64_t nperms,
                                uint64_t seed, const int32_t* perm_idx, const double* probs, int64_t nprobs, double* h2_out,
                                double* sigma2_out, double* lod_max_out, int64_t* lod_argmax_out, double* max_perms_out, double* thr_out,
                                double* pval_out, blmm_status* status);
int blmm_bulkscan_multidf_perms_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG,
                                    int64_t p, int64_t k, const double* dCovar, int64_t ncov, const double* dK, const double* dweights,
                                    int64_t nperms, uint64_t seed, const int32_t* dperm_idx, const double* probs, int64_t nprobs,
                                    double* dh2_out, double* dsigma2_out, double* dlod_max_out, int64_t* dlod_argmax_out,
                                    double* dmax_perms_out, double* dthr_out, double* dpval_out, blmm_status* status);

/* ---- conditional bulkscan: every trait scanned with its OWN loci in the null model (secondary QTL given the peak) -----------------
 * Inputs as blmm_bulkscan_multidf with k = 1 (Y n x m, G n x p, Covar / add_intercept, K, weights, h2_grid; opts: null-grid or
 * null-exact, reml, the prior, optim_interval, decomp_scheme) plus cond: s x m int64, cond[j s + a] = the 0-based column of G that
 * is trait j's a-th conditioning locus, or -1 for none.  A trait may have 0 .. s loci; s = 0 or cond == NULL: none at all.
 * In the rotated space of transform_rotation, for trait j:
 *   1. Conditioning columns, decided once and unweighted: taking the trait's valid entries in order, column a is kept iff the part
 *      of x0_a orthogonal to span[Z0, the kept columns before it] has squared norm > BLMM_COND_TAU |x0_a|^2.  A repeated index, a
 *      marker equal to a covariate and a constant marker drop out.  D_j = [Z0, kept columns], r_j = the number kept.
 *   2. Null model on D_j: null-exact fitlmm(y0_j, D_j, lambda, prior; reml, optim_interval) (src/lmm.jl:56-86); null-grid the first
 *      arg-max over the grid of wls(y0_j, D_j, makeweights(g), prior; reml).ell (src/wls.jl:27-97; REML's p is c + r_j).  h2_out[j]
 *      is that h2; with r_j = 0 it is blmm_bulkscan's null model (the search's own tolerance apart for null-exact).
 *   3. Scan: sw = sqrt(|makeweights(h2_j)|), D~ = sw .* D_j, e = the residual of sw .* y0_j on span(D~), x~_i = sw .* x0_i, r_i = the
 *      residual of x~_i on span(D~).  Rank rule (blmm_bulkscan_multidf's, at the trait's weights): |r_i|^2 <= BLMM_COND_TAU |x~_i|^2
 *      gives L[i, j] = +0.0, else L[i, j] = -(n/2) log10(1 - (r_i'e)^2 / (|r_i|^2 |e|^2)).  NaN / +Inf / e = 0 as in multidf
 *      (n_nan_lod, n_zero_norm).
 * So column j is what the reference's scan returns for (y_j, G, [Covar G[:, cond_j]], K), except at the markers the rule sets to 0
 * (the conditioning markers themselves and their duplicates), where the reference divides by zero.
 *   L_out      p x m, or NULL: L stays resident for the blmm_last_* consumers
 *   cinfo_out  int64[BLMM_COND_INFO_LEN], may be NULL: [0] entries of L the rank rule set to 0, [1] conditioning entries dropped in
 *              step 1, [2] traits with r_j >= 1, [3] 0
 *   status     as blmm_bulkscan fills it; n_illcond_rescan: traits whose weighted design D~ was nearly collinear (a marker beside
 *              the intercept at h2 -> 1) and whose columns were recomputed with an orthonormal basis and explicit residuals
 * Limits: s <= BLMM_COND_MAX_LOCI, c + s <= BLMM_MULTIDF_MAX_COVARIATES (c: null covariates incl. the intercept), c + s < n,
 * n <= 2048.  Refused before anything is uploaded: alt-grid, s or c + s above the limit, n > 2048 (BLMM_ERR_UNSUPPORTED), an
 * unknown method (BLMM_ERR_METHOD), an index outside [-1, p) (BLMM_ERR_INVALID; host form).  The _dev form cannot see its indices:
 * such a trait gets a NaN column and a NaN h2, nothing out of range is touched, and the call returns BLMM_ERR_INVALID when a status
 * is asked for.  A pending blmm_set_log10p_output request is honoured by a column pass over the finished L.
 * The _dev form: device Y / G / Covar / weights / cond / L_out (ld ldL >= p) / h2_out / cinfo_out; stream-ordered like
 * blmm_bulkscan_multidf_dev. */
#define BLMM_COND_TAU BLMM_MULTIDF_TAU
#define BLMM_COND_MAX_LOCI 4
#define BLMM_COND_INFO_LEN 4
int blmm_bulkscan_cond(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                       const double* Covar, int64_t ncov, const double* K, const double* weights, const double* h2_grid,
                       int64_t ngrid, const int64_t* cond, int64_t s, double* L_out, double* h2_out, int64_t* cinfo_out,
                       blmm_status* status);
int blmm_bulkscan_cond_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                           const double* dCovar, int64_t ncov, const double* dK, const double* dweights, const double* h2_grid,
                           int64_t ngrid, const int64_t* dcond, int64_t s, double* dL_out, int64_t ldL, double* dh2_out,
                           int64_t* dcinfo_out, blmm_status* status);

/* ---- forward selection: up to max_loci loci per trait, one after the other, without the LOD matrix -------------------------------
 * Inputs as blmm_bulkscan_cond without the table: the call builds it.  S = max_loci; rounds t = 0 .. S.  A_0 is every trait, T_0 the
 * S x m table of -1 in blmm_bulkscan_cond's layout.  Round t is, for the traits of A_t and bit for bit,
 *   R_t = blmm_bulkscan_cond(Y, G, K, Covar, weights, opts, h2_grid; cond = T_t, s = S),
 *   (lod[t, j], argmax[t, j]) = blmm_lod_colmax of column j of R_t's L (the lowest marker wins a tie, NaN is never the maximum, a
 *   column without a comparable entry gives -inf / -1),  h2[t, j] = R_t's h2[j].
 * So round 0 is blmm_bulkscan_cond without loci (not blmm_bulkscan: null-exact h2 agrees to the search's tolerance only).
 * Trait j is in A_{t+1} iff t < S and lod[t, j] > threshold (strictly: -inf fails), and then T_{t+1}[j, t] = argmax[t, j].  The call
 * ends after the first round that leaves A empty, or after round S.  Upload, eigen phase and rotations happen once, no p x m
 * buffer is allocated, and from round 1 on only the active traits are scanned; a trait's results do not depend on which other
 * traits are active.
 *   loci_out    S x m, loci_out[j S + a]: the final table (-1 beyond the trait's loci); can go straight to blmm_bulkscan_cond
 *   lod_out, argmax_out, h2_out   (S + 1) x m, x[j (S + 1) + t]; NaN / -1 / NaN for the rounds in which j was not active
 *   nloci_out   m: the loci selected for trait j
 *   sinfo_out   int64[BLMM_STEP_INFO_LEN], may be NULL: [0] rounds run, [1] traits with at least one locus, [2] entries the rank
 *               rule set to +0.0, summed over the rounds and their active traits, [3 + t] |A_t| for t = 0 .. 4 (0: round not run)
 *   status      the eigen phase's fields once, the others summed over the rounds as blmm_bulkscan_loco sums its chromosomes;
 *               n_nan_lod (the NaNs in the columns A_t of R_t's L, summed over t) and n_illcond_rescan count ACTIVE traits only;
 *               n_zero_norm is round 0's, as blmm_bulkscan_cond reports it
 * Refused before anything is uploaded, in this order in both forms: max_loci < 1 (BLMM_ERR_INVALID); max_loci > BLMM_COND_MAX_LOCI
 * or c + max_loci > BLMM_MULTIDF_MAX_COVARIATES (BLMM_ERR_UNSUPPORTED); a threshold that is NaN or < 0 (BLMM_ERR_INVALID: below 0 a
 * conditioning marker's own +0.0 could be selected again; +inf is allowed and gives one round); then blmm_bulkscan_cond's refusals
 * (alt-grid, an unknown method, n > 2048, c + max_loci >= n); a NULL buffer other than sinfo_out / status.  A pending
 * blmm_set_log10p_output request is refused with BLMM_ERR_INVALID and consumed (the call writes no matrix), and blmm_last_dims
 * reports no matrix afterwards.
 * The _dev form: device Y / G / Covar / weights and outputs, h2_grid on the host; enqueued on the context's stream.  It waits for
 * the stream once per round but the last (the next round's launches are sized by |A_{t+1}|) and once more when a status is asked
 * for; without a status the results are valid after blmm_synchronize. */
#define BLMM_STEP_INFO_LEN 8
int blmm_bulkscan_stepwise(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                           const double* Covar, int64_t ncov, const double* K, const double* weights, const double* h2_grid,
                           int64_t ngrid, int64_t max_loci, double threshold, int64_t* loci_out, double* lod_out, int64_t* argmax_out,
                           double* h2_out, int64_t* nloci_out, int64_t* sinfo_out, blmm_status* status);
int blmm_bulkscan_stepwise_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG, int64_t p,
                               const double* dCovar, int64_t ncov, const double* dK, const double* dweights, const double* h2_grid,
                               int64_t ngrid, int64_t max_loci, double threshold, int64_t* dloci_out, double* dlod_out,
                               int64_t* dargmax_out, double* dh2_out, int64_t* dnloci_out, int64_t* dsinfo_out, blmm_status* status);

/* ---- effects at chosen tests: coefficients and standard errors where a scan found something ------------------------------------
 * Takes what blmm_bulkscan_multidf takes (opts: null-grid or null-exact, reml, the prior, add_intercept, optim_interval,
 * decomp_scheme; Y n x m; G n x p with p = P k, locus l = columns l k .. l k + k - 1, k = 1: the ordinary marker test; Covar, K,
 * weights, h2_grid) plus ntests tests as two int64 arrays, locus[t] (0-based, < P) and trait[t] (0-based, < m), in any order,
 * repeats allowed.  The null model is blmm_bulkscan's: h2_out (m) is its h2_null_list for the same method and options, bit for bit.
 * For test t = (l, j), with s = sqrt(|makeweights(h2_j, lambda)|), Z~ = s .* Z0, x~_a = s .* (rotated column a of locus l),
 * y~ = s .* y0_j in the rotated space of transform_rotation, and D~ = [Z~, the ACCEPTED x~_a] -- accepted by blmm_bulkscan_multidf's
 * rank rule (BLMM_MULTIDF_TAU, in column order):
 *   beta_out[t k + a]   the coefficient of column a in the weighted least-squares fit of y~ on D~, i.e. wls(y0_j, [Z0 X0_l], w).b
 *                       (src/wls.jl) restricted to the locus columns; a dropped column has beta = 0 and se = 0
 *   se_out[t k + a]     sqrt(sigma2[t] [(D~'D~)^-1]_aa)
 *   sigma2_out[t]       wls's sigma2_e of that fit: (rss1 + prior_variance prior_sample_size) / (n + prior_df), or
 *                       / (n - (c + r) + prior_df) under REML, with rss1 = |y~ - D~ b|^2, c the null covariates incl. the intercept,
 *                       r the accepted columns and prior_df = prior_sample_size + 2 when prior_sample_size > 0, else prior_sample_size
 *                       (src/wls.jl:72-77).  A caller who wants the unbiased rss1 / (n - c - r) rescales: without a prior,
 *                       rss1 = sigma2 n under ML, and se scales with sqrt(sigma2).
 *   lod_out[t]          -(n/2) log10(rss1 / rss0), rss0 the null fit's: the number blmm_bulkscan (k = 1) or blmm_bulkscan_multidf
 *                       writes at L[l, j] (rss1 = 0: +Inf; NaN is counted in n_nan_lod)
 *   accepted_out[t]     int32 bit mask of the accepted columns (bit a = column a)
 * Limits: 1 <= k <= BLMM_EFFECTS_MAX_K for BOTH methods (null-exact too: blmm_bulkscan_multidf's BLMM_MULTIDF_MAX_K_EXACT is not
 * this call's), at most BLMM_MULTIDF_MAX_COVARIATES null covariates (incl. the intercept) for every k -- k = 1 included, where
 * blmm_bulkscan itself takes 32 --, n <= 2048, ntests < 2^31.  Refused before anything is uploaded: k < 1 or p not a multiple of k
 * (BLMM_ERR_DIM); k above the limit, more covariates, alt-grid, n > 2048 (BLMM_ERR_UNSUPPORTED); an unknown method
 * (BLMM_ERR_METHOD); a locus or trait index out of range (BLMM_ERR_INVALID).  A pending blmm_set_log10p_output request is dropped.
 * LOCO: there is no leave-one-chromosome-out form; call once per chromosome with that chromosome's kinship (blmm_kinship_loco)
 * and its tests.
 * Kernels (kernels_effects.hip): the tests are ordered by trait on the device (counting sort); one wave takes a chunk of the
 * sorted list, builds what depends on the trait only (s, an orthonormal basis of span(Z~) by Gram-Schmidt with
 * re-orthogonalisation, the null residual) once per run, and for each test orthogonalises the locus's k weighted columns
 * explicitly (no normal equations) and back-substitutes.
 * The _dev form: device Y / G / Covar / weights / locus / trait and outputs; it enqueues on the context's stream and waits only for
 * a status or to copy the host h2_grid.  It cannot refuse an index it has not seen: a test out of range gets NaN in beta, se,
 * sigma2, lod and accepted = -1, touches no memory, and makes the call return BLMM_ERR_INVALID when a status is asked for. */
#define BLMM_EFFECTS_MAX_K 8
int blmm_bulkscan_effects(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                          int64_t k, const double* Covar, int64_t ncov, const double* K, const double* weights,
                          const double* h2_grid, int64_t ngrid, const int64_t* locus, const int64_t* trait, int64_t ntests,
                          double* beta_out, double* se_out, double* sigma2_out, double* lod_out, int32_t* accepted_out,
                          double* h2_out, blmm_status* status);
int blmm_bulkscan_effects_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG,
                              int64_t p, int64_t k, const double* dCovar, int64_t ncov, const double* dK, const double* dweights,
                              const double* h2_grid, int64_t ngrid, const int64_t* dlocus, const int64_t* dtrait, int64_t ntests,
                              double* dbeta_out, double* dse_out, double* dsigma2_out, double* dlod_out, int32_t* daccepted_out,
                              double* dh2_out, blmm_status* status);

/* ---- scan(y, G, [Z], K; assumption = "alt") -> scan_alt (src/scan.jl:397-453): the variance components are re-estimated for
 * every marker (fitlmm on [Z g_i], src/lmm.jl:56-86, one Brent search per marker on the device).
 * scalars_out = [sigma2_e, h2_null]; lod_out p; h2_each_out p (`h2_each_marker`).  opts->compat_flags:
 * BLMM_COMPAT_ALT_TRUE_WEIGHTS. */
int blmm_scan_alt(blmm_ctx* ctx, const blmm_opts* opts, const double* y, int64_t n, const double* G, int64_t p,
                  const double* Covar, int64_t ncov, const double* K, const double* weights, double* scalars_out,
                  double* lod_out, double* h2_each_out, blmm_status* status);
int blmm_scan_alt_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dy, int64_t n, const double* dG, int64_t p,
                      const double* dCovar, int64_t ncov, const double* dK, const double* dweights, double* dscalars_out,
                      double* dlod_out, double* dh2_each_out, blmm_status* status);
/* The bulk form of it (not in the reference, which has the single-trait scan_alt and the grid approximation
 * bulkscan_alt_grid): for EVERY (trait, marker) the exact heritability under the alternative (one Brent search per test) and
 * the LOD against the trait's null model.  L_out, h2_panel_out: p x m column-major (leading dimensions ldL, ldH in the _dev
 * form); h2_null_out m; sigma2_out m or NULL.  Column j equals blmm_scan_alt on trait j bit for bit.  ~0.02 us per test at
 * n = 79 (64 traits x 7321 markers: 8.6 ms host to host) -- the whole BXD matrix would take ~5 s where the 16-point grid of
 * bulkscan_alt_grid takes 15 ms: meant for subsets of traits.  At most 31 null covariates (the per-marker design [Z0 x] has c + 1 <= 32 columns; beyond 8 the run-time-c kernel k_dyn_alt_brent). */
int blmm_bulkscan_alt_exact(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G, int64_t p,
                            const double* Covar, int64_t ncov, const double* K, const double* weights, double* L_out,
                            double* h2_panel_out, double* h2_null_out, double* sigma2_out, blmm_status* status);
int blmm_bulkscan_alt_exact_dev(blmm_ctx* ctx, const blmm_opts* opts, const double* dY, int64_t n, int64_t m, const double* dG,
                                int64_t p, const double* dCovar, int64_t ncov, const double* dK, const double* dweights,
                                double* dL_out, int64_t ldL, double* dh2_panel_out, int64_t ldH, double* dh2_null_out,
                                double* dsigma2_out, blmm_status* status);

/* ---- on-device consumer of L: column maxima (per-trait / per-permutation peak LOD and its marker, 0-based) -------
 * The reduction behind get_thresholds (src/analysis_helpers/single_trait_analysis.jl:13-23); argmax_out may be NULL. */
int blmm_lod_colmax(blmm_ctx* ctx, const double* L, int64_t p, int64_t m, double* max_out, int64_t* argmax_out);
int blmm_lod_colmax_dev(blmm_ctx* ctx, const double* dL, int64_t p, int64_t m, int64_t ldL, double* dmax_out,
                        int64_t* dargmax_out);

/* ---- -log10 p-values: lod2log10p.(L, chisq_df)  (src/util.jl:199-206; `output_pvals`, src/bulkscan.jl:154-157,
 * src/scan.jl:353-355).  df = 1: LOD + x w(x), x = sqrt(LOD ln 10), w = -log10(erfcx(x)) / x from bucketed polynomials
 * (4e-15 relative; BLMM_PVAL_LIBM=1: erfc / erfcx / log instead); general df through ln Q(df/2, .) in log space.  chisq_df runs
 * from 1 to 10^6 at every entry point that takes one (here, blmm_set_log10p_output, blmm_last_log10p): BLMM_ERR_INVALID beyond. */
int blmm_lod2log10p(blmm_ctx* ctx, const double* L, int64_t p, int64_t m, int64_t chisq_df, double* P_out);
int blmm_lod2log10p_dev(blmm_ctx* ctx, const double* dL, int64_t p, int64_t m, int64_t ldL, int64_t chisq_df, double* dP_out,
                        int64_t ldP);
/* `output_pvals = true` of bulkscan (src/bulkscan.jl:154-157) INSIDE the scan: the next blmm_bulkscan / blmm_bulkscan_dev /
 * blmm_bulkscan_prerotated_dev call of this context also writes -log10 p, p x m with leading dimension ldP, into the DEVICE
 * buffer dP_out -- or, dP_out == NULL, into a buffer of the context that blmm_last_log10p then hands out without computing
 * anything.  chisq_df = 1 with a null-* method: a second output of the scan kernels' epilogues (the LOD matrix is not read
 * back from HBM for it); alt-grid or another chisq_df: the column pass above, run inside the call.  One-shot: the request is
 * consumed by that call; chisq_df = 0 withdraws it. */
int blmm_set_log10p_output(blmm_ctx* ctx, double* dP_out, int64_t ldP, int64_t chisq_df);
/* ---- threshold filter: every (marker, trait) with LOD > thr as a sparse triplet (0-based int32 indices), the count on
 * the device (README.md:354-359).  At most `cap` triplets are stored, *count is the total found; order unspecified. */
int blmm_lod_threshold(blmm_ctx* ctx, const double* L, int64_t p, int64_t m, double thr, int64_t cap, int32_t* i_out,
                       int32_t* j_out, double* lod_out, int64_t* count_out);
int blmm_lod_threshold_dev(blmm_ctx* ctx, const double* dL, int64_t p, int64_t m, int64_t ldL, double thr, int64_t cap,
                           int32_t* di_out, int32_t* dj_out, double* dlod_out, int64_t* dcount_out);
/* ---- get_thresholds (src/analysis_helpers/single_trait_analysis.jl:13-23): quantiles (Julia's default, linear
 * interpolation) at `probs` (HOST array, nprobs <= 64) of the per-permutation maxima; column maxima, sort and
 * interpolation on the device, thrs_out (nprobs doubles) in HOST memory.  A level is clamped to [0, 1]; with h = (nperms - 1) q,
 * a <= b the maxima of rank floor(h) and floor(h) + 1 and g = h - floor(h), the threshold is a + g (b - a) for finite a, b.
 * Maxima may be infinite (+inf: an LOD of 1 - R^2 = 0; -inf: a column without a comparable LOD): g == 0 or a == b gives a (two
 * equal infinities give that infinity, not inf - inf), otherwise (1 - g) a + g b in the extended reals -- +inf above a finite a,
 * -inf below a finite b, and -inf beside +inf the limit of (2 g - 1) M: -inf below g = 1/2, +inf above, 0 at it.  A threshold
 * lies between two order statistics and is never NaN. */
int blmm_get_thresholds(blmm_ctx* ctx, const double* Lperms, int64_t p, int64_t nperms, const double* probs, int64_t nprobs,
                        double* thrs_out);
int blmm_get_thresholds_dev(blmm_ctx* ctx, const double* dLperms, int64_t p, int64_t nperms, int64_t ld, const double* probs,
                            int64_t nprobs, double* thrs_out);
/* ---- the same consumers on the LOD matrix of the LAST host-pointer call of this context (blmm_bulkscan: L;
 * blmm_scan_perms: L_perms), which is still resident in HBM: nothing is uploaded again. */
int blmm_last_log10p(blmm_ctx* ctx, int64_t chisq_df, double* P_out);
int blmm_last_lod_threshold(blmm_ctx* ctx, double thr, int64_t cap, int32_t* i_out, int32_t* j_out, double* lod_out,
                            int64_t* count_out);
int blmm_last_get_thresholds(blmm_ctx* ctx, const double* probs, int64_t nprobs, double* thrs_out);
/* shape of the resident matrix (0 x 0 and BLMM_ERR_INVALID when there is none); its column maxima (max_out m, argmax_out m or
 * NULL; the rule of blmm_lod_colmax); selected columns: out is p x ncols, column k = L[:, cols[k]] (0-based) */
int blmm_last_dims(const blmm_ctx* ctx, int64_t* p_out, int64_t* m_out);
int blmm_last_lod_colmax(blmm_ctx* ctx, double* max_out, int64_t* argmax_out);
int blmm_last_lod_columns(blmm_ctx* ctx, const int64_t* cols, int64_t ncols, double* out);

/* ---- lower-level seams (1:1 with the reference's internal functions; used by the parity tests) ---- */
/* transform_rotation(y, [Z G], K)  (src/transform_helpers.jl:1-54): Y0 n x m, X0 n x (c+p) (first c
 * columns = rotated null covariates, intercept first when add_intercept), lambda n. */
int blmm_rotate(blmm_ctx* ctx, const blmm_opts* opts, const double* Y, int64_t n, int64_t m, const double* G,
                int64_t p, const double* Covar, int64_t ncov, const double* K, double* Y0_out, double* X0_out,
                double* lambda_out, blmm_status* status);
/* fitlmm over every column of Y0 (src/lmm.jl:56-86, src/gridbrent.jl:9-24): h2, sigma2, ell: m each. */
int blmm_null_h2_brent(blmm_ctx* ctx, const blmm_opts* opts, const double* Y0, int64_t n, int64_t m,
                       const double* Z0, int64_t c, const double* lambda, double* h2_out, double* sigma2_out,
                       double* ell_out, blmm_status* status);
/* wls_multivar(Y0, Z0, makeweights(h2_g), prior).Ell for every grid point (src/wls.jl:103-176,
 * src/bulkscan_helpers.jl:267-269): Ell_out ngrid x m (ld = ngrid). */
int blmm_null_loglik_grid(blmm_ctx* ctx, const blmm_opts* opts, const double* Y0, int64_t n, int64_t m,
                          const double* Z0, int64_t c, const double* lambda, const double* h2_grid, int64_t ngrid,
                          double* Ell_out, blmm_status* status);
/* weighted_liteqtl(Y0, X0, lambda, hsq; num_of_covar)  (src/bulkscan_helpers.jl:175-201): X0 n x (c+p). */
int blmm_weighted_liteqtl(blmm_ctx* ctx, const double* Y0, int64_t n, int64_t m, const double* X0, int64_t c,
                          int64_t p, const double* lambda, double hsq, double* LOD_out, blmm_status* status);
/* univar_liteqtl over every column of Y0 with the per-trait h2 supplied by the caller
 * (src/bulkscan_helpers.jl:138-146): the exact-weights LOD kernel on its own. */
int blmm_liteqtl_given_h2(blmm_ctx* ctx, const double* Y0, int64_t n, int64_t m, const double* X0, int64_t c,
                          int64_t p, const double* lambda, const double* h2, double* LOD_out, blmm_status* status);

#ifdef __cplusplus
}
#endif
#endif /* BULKLMM_HIP_H */
