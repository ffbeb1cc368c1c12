# BulkLMMHIP.jl -- thin `ccall` host for libbulklmm_hip.so (include/bulklmm_hip.h).
#
# Same signatures, keyword defaults and NamedTuple fields as BulkLMM.jl's bulkscan hot path
# (src/bulkscan.jl:81-162,188-314,321-397,428-526; src/scan.jl:94-271,485-557; src/kinship.jl:4-14), so that
#     using BulkLMMHIP: bulkscan, bulkscan_null, bulkscan_null_grid, bulkscan_alt_grid, scan, calcKinship
# is a drop-in for `using BulkLMM` on that path.  NOTE: there is no Julia in the build container, so THIS FILE HAS NEVER
# BEEN EXECUTED; it is the binding a maintainer adds (INTEGRATION.md) and mirrors bulklmm.jl_amd/api.py (the ctypes host
# that IS tested) 1:1.  What can be checked without Julia is checked as TEXT by tests/test_binding_kwargs.py: every keyword of
# the reference's signatures is accepted here and in api.py; the fields of BlmmOpts / BlmmStatus / BlmmMultiOpts (names, types,
# order, and through them offsets and sizes, against `offsetof` / `sizeof` printed by a C program compiled from the header);
# every `ccall`'s symbol, return type and argument tuple (arity and types) against the prototype in include/bulklmm_hip.h.
module BulkLMMHIP

export bulkscan_cond, bulkscan_stepwise, bulkscan_stepwise_dev!, bulkscan_effects, bulkscan_multidf, bulkscan_multidf_perms, bulkscan_multidf_reduced, bulkscan_multidf_reduced_dev!, calcKinship_loco, bulkscan_loco, bulkscan_loco_reduced, bulkscan_loco_perms, bulkscan_perms, bulkscan_reduced, bulkscan_reduced_async!, synchronize, DeviceLOD, lod_columns, set_tuning, calcKinship, bulkscan, bulkscan_null, bulkscan_null_grid, bulkscan_alt_grid, bulkscan_alt_exact, scan, bulkscan_multi, lod2log10p, get_thresholds,
       lod_threshold, lod_colmax, pinned_matrix, host_register, host_unregister

const libblmm = get(ENV, "BULKLMM_HIP_LIB", joinpath(@__DIR__, "..", "csrc", "libbulklmm_hip.so"))

struct BlmmOpts            # include/bulklmm_hip.h: blmm_opts
    method::Int32; reml::Int32; add_intercept::Int32; decomp_scheme::Int32
    optim_interval::Int32; compat_flags::Int32
    prior_variance::Float64; prior_sample_size::Float64
end

mutable struct BlmmStatus  # include/bulklmm_hip.h: blmm_status
    n_neg_eig::Int64; n_nonpos_weight::Int64; n_zero_norm::Int64; n_nan_lod::Int64
    n_brent_maxiter::Int64; jacobi_sweeps::Int64; jacobi_cycles::Int64; jacobi_ticks_100mhz::Int64
    lowrank_rank::Int64; lowrank_fallback::Int64; lowrank_shared::Int64; lowrank_resid::Float64
    t_eigen_ms::Float64; t_rotate_ms::Float64; t_h2_ms::Float64; t_prep_ms::Float64; t_scan_ms::Float64; t_total_ms::Float64
    n_h2_boundary::Int64; n_h2_multimodal::Int64; n_illcond_rescan::Int64
    BlmmStatus() = new(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0)
end

const NULL_EXACT, NULL_GRID, ALT_GRID = Int32(0), Int32(1), Int32(2)
const _ctx = Ref{Ptr{Cvoid}}(C_NULL)

function context(device::Integer = 0)
    if _ctx[] == C_NULL
        h = Ref{Ptr{Cvoid}}(C_NULL)
        rc = ccall((:blmm_create, libblmm), Cint, (Cint, Ptr{Cvoid}, Ref{Ptr{Cvoid}}), device, C_NULL, h)
        rc == 0 || error(unsafe_string(ccall((:blmm_err_string, libblmm), Cstring, (Cint,), rc)))
        _ctx[] = h[]
    end
    return _ctx[]
end

check(rc) = rc == 0 || error(unsafe_string(ccall((:blmm_last_error, libblmm), Cstring, (Ptr{Cvoid},), context())))

function raise_status(st)   # BlmmStatus, or one element of the per-device Vector of bulkscan_multi
    st.n_neg_eig > 0 && @warn "Negative eigenvalues exist. The kinship matrix supplied may not be SPD."   # src/transform_helpers.jl:29
    st.n_nonpos_weight > 0 && @warn "Some weights are not positive."                                      # src/wls.jl:36
    st.n_zero_norm > 0 && error("Dividing by zeros: the input vector can not contain any zeros!")         # src/util.jl:70
end

decomp(s::String) = s == "eigen" ? Int32(0) : s == "svd" ? Int32(1) : Int32(99)
# The one capability gap against the reference (LAPACK's eigen has no size limit, src/transform_helpers.jl:21-34): the device
# eigensolver stops at 2048 individuals.  Refused here, before anything is uploaded, with the library's own message.
const MAX_INDIVIDUALS = 2048
check_n(n) = n <= MAX_INDIVIDUALS || error("more than 2048 individuals: the device eigensolver (tridiagonalisation + divide and conquer) stops at n = 2048")
ptr_or_null(x) = x === missing || x === nothing ? Ptr{Float64}(C_NULL) : pointer(x)

function calcKinship(geno::Array{Float64, 2})
    (n, p) = size(geno)
    K = Array{Float64, 2}(undef, n, n)
    GC.@preserve geno K check(ccall((:blmm_kinship, libblmm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}),
                                    context(), geno, n, p, K))
    return K
end

function _bulkscan(method::Int32, Y::Array{Float64, 2}, G::Array{Float64, 2}, Covar, K::Array{Float64, 2}, grid::Vector{Float64};
                   addIntercept::Bool, weights, prior_variance::Float64, prior_sample_size::Float64, reml::Bool,
                   optim_interval::Int64, decomp_scheme::String, keep_on_device::Bool = false, pvals_df::Int64 = 0)
    (n, m) = size(Y); p = size(G, 2)
    (size(G, 1) != n || size(K, 1) != n || size(K, 2) != n) && error("Dimension mismatch.")
    check_n(n)   # src/transform_helpers.jl:9-11
    (Covar !== nothing && size(Covar, 1) != n) && error("Dimension mismatch.")
    (weights !== missing && length(weights) != n) && error("Dimension mismatch.")
    ncov = Covar === nothing ? 0 : size(Covar, 2)
    o = BlmmOpts(method, reml, Covar === nothing ? true : addIntercept, decomp(decomp_scheme), optim_interval, 0,
                 prior_variance, prior_sample_size)
    # keep_on_device: L_out == NULL -- the matrix stays in the context's HBM workspace and `L` is a DeviceLOD handle
    L = keep_on_device ? nothing : Array{Float64, 2}(undef, p, m)
    h2 = method == ALT_GRID ? Array{Float64, 2}(undef, p, m) : Array{Float64, 1}(undef, m)
    st = BlmmStatus()
    # `output_pvals`: asked for right in front of the scan (after every check above), so that the scan kernels write -log10 p from
    # their epilogues (chisq_df = 1, null-* methods; otherwise the column pass runs inside the call) into a buffer of the context
    # that _last_log10p hands out; the library consumes the request first thing in the call, whatever happens next
    if pvals_df > 0
        check(ccall((:blmm_set_log10p_output, libblmm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64),
                    context(), Ptr{Float64}(C_NULL), Int64(0), pvals_df))
    end
    GC.@preserve Y G Covar K weights grid L h2 begin
        check(ccall((:blmm_bulkscan, libblmm), Cint,
                    (Ptr{Cvoid}, Ref{BlmmOpts}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64,
                     Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ref{BlmmStatus}),
                    context(), o, Y, n, m, G, p, ptr_or_null(Covar), ncov, K, ptr_or_null(weights), grid, length(grid),
                    ptr_or_null(L), h2, st))
    end
    raise_status(st)
    return (keep_on_device ? DeviceLOD(p, m) : L), h2
end

# ---- the LOD matrix of a `keep_on_device = true` call: it stays in HBM (2.08 GB at BXD size: 36 of a call's 39 ms are its trip over
# PCIe) and is reduced there -- what README.md:246-255, 354-359 and get_thresholds do with L -- until the context's next call
struct DeviceLOD
    p::Int64
    m::Int64
end
Base.size(d::DeviceLOD) = (d.p, d.m)
function _alive(d::DeviceLOD)
    pp = Ref{Int64}(0); mm = Ref{Int64}(0)
    rc = ccall((:blmm_last_dims, libblmm), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), context(), pp, mm)
    (rc == 0 && pp[] == d.p && mm[] == d.m) || error("the device-resident LOD matrix has been replaced by a later call")
end
function lod_colmax(d::DeviceLOD)
    _alive(d)
    mx = Vector{Float64}(undef, d.m); arg = Vector{Int64}(undef, d.m)
    GC.@preserve mx arg check(ccall((:blmm_last_lod_colmax, libblmm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}), context(), mx, arg))
    return (max = mx, argmax = arg .+ 1)
end
function lod_threshold(d::DeviceLOD, thr::Float64; cap::Int64 = 65536)
    _alive(d)
    while true
        ii = Vector{Int32}(undef, cap); jj = Vector{Int32}(undef, cap); ll = Vector{Float64}(undef, cap)
        cnt = Ref{Int64}(0)
        GC.@preserve ii jj ll check(ccall((:blmm_last_lod_threshold, libblmm), Cint,
            (Ptr{Cvoid}, Float64, Int64, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ref{Int64}), context(), thr, cap, ii, jj, ll, cnt))
        if cnt[] <= cap
            k = cnt[]
            ord = sortperm(collect(zip(jj[1:k], ii[1:k])))
            return (marker = Int.(ii[1:k][ord]) .+ 1, trait = Int.(jj[1:k][ord]) .+ 1, lod = ll[1:k][ord])
        end
        cap = cnt[]
    end
end
function get_thresholds(d::DeviceLOD, signif_level::Array{Float64, 1})
    _alive(d)
    probs = 1.0 .- signif_level
    thrs = similar(probs)
    GC.@preserve probs thrs check(ccall((:blmm_last_get_thresholds, libblmm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}),
                                        context(), probs, length(probs), thrs))
    return (probs = probs, thrs = thrs)
end
# L[:, traits] (1-based): the LOD profiles of a few traits -- the only part of L that crosses PCIe
function lod_columns(d::DeviceLOD, traits::Vector{Int64})
    _alive(d)
    cols = traits .- 1
    out = Array{Float64, 2}(undef, d.p, length(cols))
    GC.@preserve cols out check(ccall((:blmm_last_lod_columns, libblmm), Cint, (Ptr{Cvoid}, Ptr{Int64}, Int64, Ptr{Float64}),
                                      context(), cols, length(cols), out))
    return out
end
Base.Array(d::DeviceLOD) = lod_columns(d, collect(1:d.m))

# ---- tuning (include/bulklmm_hip.h): the switches that select another arithmetic path are properties of the context
set_tuning(key::String, value::Real) = check(ccall((:blmm_set_tuning, libblmm), Cint, (Ptr{Cvoid}, Cstring, Float64), context(), key, Float64(value)))

# ---- bulkscan WITHOUT the LOD matrix (blmm_bulkscan_reduced): per trait the peak LOD and its marker and, `threshold` given, every
# (marker, trait, LOD) with LOD > threshold, out of the scan kernels' epilogues; L is never written.  Not in the reference, whose
# users reduce L on the CPU (README.md:246-255, 354-359).
struct BlmmReduced   # include/bulklmm_hip.h: blmm_reduced
    colmax::Ptr{Float64}; argmax::Ptr{Int64}; want_triplets::Int64; thr::Float64; cap::Int64
    ti::Ptr{Int32}; tj::Ptr{Int32}; tlod::Ptr{Float64}; count::Ptr{Int64}
end
function bulkscan_reduced(Y::Array{Float64, 2}, G::Array{Float64, 2}, Covar::Union{Nothing, Array{Float64, 2}}, K::Array{Float64, 2};
                          method::String = "null-grid", h2_grid::Array{Float64, 1} = collect(0.0:0.1:0.9),
                          threshold::Union{Nothing, Float64} = nothing, cap::Int64 = 1048576, addIntercept::Bool = true,
                          weights::Union{Missing, Array{Float64, 1}} = missing, prior_variance::Float64 = 1.0,
                          prior_sample_size::Float64 = 0.0, reml::Bool = false, optim_interval::Int64 = 1,
                          decomp_scheme::String = "eigen")
    meth = method == "null-exact" ? NULL_EXACT : method == "null-grid" ? NULL_GRID : method == "alt-grid" ? ALT_GRID :
           error("Unknown method `$method`; choose null-exact, null-grid or alt-grid.")
    (n, m) = size(Y); p = size(G, 2)
    (size(G, 1) != n || size(K, 1) != n || size(K, 2) != n) && error("Dimension mismatch.")
    check_n(n)
    (Covar !== nothing && size(Covar, 1) != n) && error("Dimension mismatch.")
    (weights !== missing && length(weights) != n) && error("Dimension mismatch.")
    ncov = Covar === nothing ? 0 : size(Covar, 2)
    o = BlmmOpts(meth, reml, Covar === nothing ? true : addIntercept, decomp(decomp_scheme), optim_interval, 0,
                 prior_variance, prior_sample_size)
    grid = meth == NULL_EXACT ? Float64[] : h2_grid
    mx = Vector{Float64}(undef, m); arg = Vector{Int64}(undef, m); h2 = Vector{Float64}(undef, m)
    want = threshold !== nothing
    st = BlmmStatus()
    while true
        c1 = max(cap, 1)
        ii = Vector{Int32}(undef, c1); jj = Vector{Int32}(undef, c1); ll = Vector{Float64}(undef, c1); cnt = zeros(Int64, 1)
        GC.@preserve Y G Covar K weights grid mx arg h2 ii jj ll cnt begin
            r = BlmmReduced(pointer(mx), pointer(arg), want ? 1 : 0, want ? threshold : 0.0, want ? cap : 0,
                            pointer(ii), pointer(jj), pointer(ll), pointer(cnt))
            check(ccall((:blmm_bulkscan_reduced, libblmm), Cint,
                        (Ptr{Cvoid}, Ref{BlmmOpts}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64,
                         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ref{BlmmReduced}, Ptr{Float64}, Ref{BlmmStatus}),
                        context(), o, Y, n, m, G, p, ptr_or_null(Covar), ncov, K, ptr_or_null(weights), grid, length(grid), r, h2, st))
        end
        if !want || cnt[1] <= cap
            raise_status(st)
            res = (max_lod = mx, argmax = arg .+ 1, h2_null_list = h2)
            want || return res
            k = cnt[1]
            ord = sortperm(collect(zip(jj[1:k], ii[1:k])))
            return merge(res, (marker = Int.(ii[1:k][ord]) .+ 1, trait = Int.(jj[1:k][ord]) .+ 1, lod = ll[1:k][ord]))
        end
        cap = cnt[1]
    end
end
bulkscan_reduced(Y::Array{Float64, 2}, G::Array{Float64, 2}, K::Array{Float64, 2}; kwargs...) = bulkscan_reduced(Y, G, nothing, K; kwargs...)

# ---- the stream-ordered form (blmm_bulkscan_reduced_async) on DEVICE buffers (e.g. AMDGPU.jl arrays' pointers): it enqueues and
# returns; `out`'s buffers, dh2 and the info block (RINFO_LEN Int64 in device memory: route, re-scan counts, status counts, the
# triplet count, device error; include/bulklmm_hip.h) are valid after `synchronize()`.  0-based markers / traits, as the C ABI.
const RINFO_LEN = 9
function bulkscan_reduced_async!(dY::Ptr{Float64}, n::Int64, m::Int64, dG::Ptr{Float64}, p::Int64, dK::Ptr{Float64},
                                 out::BlmmReduced, dh2::Ptr{Float64}, dinfo::Ptr{Int64}; method::String = "null-exact",
                                 h2_grid::Array{Float64, 1} = collect(0.0:0.1:0.9), dCovar::Ptr{Float64} = Ptr{Float64}(C_NULL),
                                 ncov::Int64 = 0, dweights::Ptr{Float64} = Ptr{Float64}(C_NULL), addIntercept::Bool = true,
                                 prior_variance::Float64 = 1.0, prior_sample_size::Float64 = 0.0, reml::Bool = false,
                                 optim_interval::Int64 = 1, decomp_scheme::String = "eigen")
    meth = method == "null-exact" ? NULL_EXACT : method == "null-grid" ? NULL_GRID : method == "alt-grid" ? ALT_GRID :
           error("Unknown method `$method`; choose null-exact, null-grid or alt-grid.")
    check_n(n)
    o = BlmmOpts(meth, reml, ncov == 0 ? true : addIntercept, decomp(decomp_scheme), optim_interval, 0, prior_variance, prior_sample_size)
    grid = meth == NULL_EXACT ? Float64[] : h2_grid
    GC.@preserve grid begin
        check(ccall((:blmm_bulkscan_reduced_async, libblmm), Cint,
                    (Ptr{Cvoid}, Ref{BlmmOpts}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64,
                     Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ref{BlmmReduced}, Ptr{Float64}, Ptr{Int64}),
                    context(), o, dY, n, m, dG, p, dCovar, ncov, dK, dweights, grid, length(grid), out, dh2, dinfo))
    end
    return nothing
end
# waits for the context's stream and reports a device-side failure of the calls before it
synchronize() = check(ccall((:blmm_synchronize, libblmm), Cint, (Ptr{Cvoid},), context()))

# nb / nt_blas are accepted and ignored (thread blocking knobs of the CPU implementation)
function bulkscan_null(Y::Array{Float64, 2}, G::Array{Float64, 2}, K::Array{Float64, 2};
                       nb::Int64 = Threads.nthreads(), nt_blas::Int64 = 1, weights = missing,
                       prior_variance::Float64 = 1.0, prior_sample_size::Float64 = 0.0, reml::Bool = false,
                       optim_interval::Int64 = 1, decomp_scheme::String = "eigen", keep_on_device::Bool = false, pvals_df::Int64 = 0)
    (L, h2) = _bulkscan(NULL_EXACT, Y, G, nothing, K, Float64[]; addIntercept = true, weights = weights,
                        prior_variance = prior_variance, prior_sample_size = prior_sample_size, reml = reml,
                        optim_interval = optim_interval, decomp_scheme = decomp_scheme, keep_on_device = keep_on_device, pvals_df = pvals_df)
    return (L = L, h2_null_list = h2)
end
function bulkscan_null(Y::Array{Float64, 2}, G::Array{Float64, 2}, Covar::Array{Float64, 2}, K::Array{Float64, 2};
                       nb::Int64 = Threads.nthreads(), nt_blas::Int64 = 1, addIntercept::Bool = true, weights = missing,
                       prior_variance::Float64 = 1.0, prior_sample_size::Float64 = 0.0, reml::Bool = false,
                       optim_interval::Int64 = 1, decomp_scheme::String = "eigen", keep_on_device::Bool = false, pvals_df::Int64 = 0)
    (L, h2) = _bulkscan(NULL_EXACT, Y, G, Covar, K, Float64[]; addIntercept = addIntercept, weights = weights,
                        prior_variance = prior_variance, prior_sample_size = prior_sample_size, reml = reml,
                        optim_interval = optim_interval, decomp_scheme = decomp_scheme, keep_on_device = keep_on_device, pvals_df = pvals_df)
    return (L = L, h2_null_list = h2)
end

function bulkscan_null_grid(Y::Array{Float64, 2}, G::Array{Float64, 2}, K::Array{Float64, 2}, grid_list::Array{Float64, 1};
                            weights = missing, prior_variance::Float64 = 1.0, prior_sample_size::Float64 = 0.0,
                            reml::Bool = false, decomp_scheme::String = "eigen", keep_on_device::Bool = false, pvals_df::Int64 = 0)
    (L, h2) = _bulkscan(NULL_GRID, Y, G, nothing, K, grid_list; addIntercept = true, weights = weights,
                        prior_variance = prior_variance, prior_sample_size = prior_sample_size, reml = reml,
                        optim_interval = 1, decomp_scheme = decomp_scheme, keep_on_device = keep_on_device, pvals_df = pvals_df)
    return (L = L, h2_null_list = h2)
end
function bulkscan_null_grid(Y::Array{Float64, 2}, G::Array{Float64, 2}, Covar::Array{Float64, 2}, K::Array{Float64, 2},
                            grid_list::Array{Float64, 1}; weights = missing, addIntercept::Bool = true,
                            prior_variance::Float64 = 1.0, prior_sample_size::Float64 = 0.0, reml::Bool = false,
                            decomp_scheme::String = "eigen", keep_on_device::Bool = false, pvals_df::Int64 = 0)
    (L, h2) = _bulkscan(NULL_GRID, Y, G, Covar, K, grid_list; addIntercept = addIntercept, weights = weights,
                        prior_variance = prior_variance, prior_sample_size = prior_sample_size, reml = reml,
                        optim_interval = 1, decomp_scheme = decomp_scheme, keep_on_device = keep_on_device, pvals_df = pvals_df)
    return (L = L, h2_null_list = h2)
end

function bulkscan_alt_grid(Y::Array{Float64, 2}, G::Array{Float64, 2}, K::Array{Float64, 2}, hsq_list::Array{Float64, 1};
                           reml::Bool = false, prior_variance::Float64 = 1.0, prior_sample_size::Float64 = 0.0,
                           weights = missing, decomp_scheme::String = "eigen", keep_on_device::Bool = false, pvals_df::Int64 = 0)
    (L, h2) = _bulkscan(ALT_GRID, Y, G, nothing, K, hsq_list; addIntercept = true, weights = weights,
                        prior_variance = prior_variance, prior_sample_size = prior_sample_size, reml = reml,
                        optim_interval = 1, decomp_scheme = decomp_scheme, keep_on_device = keep_on_device, pvals_df = pvals_df)
    return (L = L, h2_panel = h2)
end
function bulkscan_alt_grid(Y::Array{Float64, 2}, G::Array{Float64, 2}, Covar::Array{Float64, 2}, K::Array{Float64, 2},
                           hsq_list::Array{Float64, 1}; reml::Bool = false, prior_variance::Float64 = 1.0,
                           prior_sample_size::Float64 = 0.0, weights = missing, addIntercept::Bool = true,
                           decomp_scheme::String = "eigen", keep_on_device::Bool = false, pvals_df::Int64 = 0)
    (L, h2) = _bulkscan(ALT_GRID, Y, G, Covar, K, hsq_list; addIntercept = addIntercept, weights = weights,
                        prior_variance = prior_variance, prior_sample_size = prior_sample_size, reml = reml,
                        optim_interval = 1, decomp_scheme = decomp_scheme, keep_on_device = keep_on_device, pvals_df = pvals_df)
    return (L = L, h2_panel = h2)
end

# lod2log10p.(L, chisq_df) of the LOD matrix the last host-pointer call left in HBM (src/util.jl:199-206, on the GPU)
function _last_log10p(dims, chisq_df::Int64)
    P = Array{Float64}(undef, dims...)
    GC.@preserve P check(ccall((:blmm_last_log10p, libblmm), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}), context(), chisq_df, P))
    return P
end

# What the last null-exact call executed in its low-rank weights form (diagnostic; include/bulklmm_hip.h: blmm_lowrank_profile):
# (traits of the shared-weights class, [(traits, rank) per segment of the heritability axis])
function lowrank_profile()
    out = zeros(Int64, 18)
    GC.@preserve out check(ccall((:blmm_lowrank_profile, libblmm), Cint, (Ptr{Cvoid}, Ptr{Int64}), context(), out))
    return (shared = out[2], segments = [(traits = out[3 + 2s], rank = out[4 + 2s]) for s in 0:(out[1] - 1)])
end

function lod2log10p(lod::Array{Float64}, df::Int64)
    P = similar(lod)
    (p, m) = ndims(lod) == 2 ? size(lod) : (length(lod), 1)
    GC.@preserve lod P check(ccall((:blmm_lod2log10p, libblmm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}),
                                   context(), lod, p, m, df, P))
    return P
end
lod2log10p(lod::Float64, df::Int64) = lod2log10p([lod], df)[1]

# bulkscan(Y, G, K; ...) and bulkscan(Y, G, Covar, K; ...): src/bulkscan.jl:81-111, 113-162
function bulkscan(Y::Array{Float64, 2}, G::Array{Float64, 2}, K::Array{Float64, 2};
                  method::String = "null-grid", h2_grid::Array{Float64, 1} = collect(0.0:0.1:0.9),
                  nb::Int64 = Threads.nthreads(), nt_blas::Int64 = 1,
                  weights::Union{Missing, Array{Float64, 1}} = missing,
                  prior_variance::Float64 = 1.0, prior_sample_size::Float64 = 0.0,
                  reml::Bool = false, optim_interval::Int64 = 1,
                  decomp_scheme::String = "eigen",
                  output_pvals::Bool = false, chisq_df::Int64 = 1, keep_on_device::Bool = false)
    # when no covariates are added, make the intercept the only covariate (src/bulkscan.jl:97-108)
    return bulkscan(Y, G, ones(size(Y, 1), 1), K; method = method, h2_grid = h2_grid, nb = nb, nt_blas = nt_blas,
                    addIntercept = false, weights = weights, prior_variance = prior_variance,
                    prior_sample_size = prior_sample_size, reml = reml, optim_interval = optim_interval,
                    decomp_scheme = decomp_scheme, output_pvals = output_pvals, chisq_df = chisq_df, keep_on_device = keep_on_device)
end
function bulkscan(Y::Array{Float64, 2}, G::Array{Float64, 2}, Covar::Array{Float64, 2}, K::Array{Float64, 2};
                  method::String = "null-grid", h2_grid::Array{Float64, 1} = collect(0.0:0.1:0.9),
                  nb::Int64 = Threads.nthreads(), nt_blas::Int64 = 1, addIntercept::Bool = true,
                  weights::Union{Missing, Array{Float64, 1}} = missing,
                  prior_variance::Float64 = 1.0, prior_sample_size::Float64 = 0.0,
                  reml::Bool = false, optim_interval::Int64 = 1,
                  decomp_scheme::String = "eigen",
                  output_pvals::Bool = false, chisq_df::Int64 = 1, keep_on_device::Bool = false)
    # keep_on_device = true (not in the reference): `L` is a DeviceLOD -- the p x m matrix stays in HBM and lod_colmax /
    # lod_threshold / get_thresholds / lod_columns reduce it there
    pv = output_pvals ? chisq_df : Int64(0)
    if method == "null-exact"
        res = bulkscan_null(Y, G, Covar, K; addIntercept = addIntercept, weights = weights, prior_variance = prior_variance,
                            prior_sample_size = prior_sample_size, reml = reml, optim_interval = optim_interval,
                            decomp_scheme = decomp_scheme, keep_on_device = keep_on_device, pvals_df = pv)
    elseif method == "null-grid"
        res = bulkscan_null_grid(Y, G, Covar, K, h2_grid; addIntercept = addIntercept, weights = weights,
                                 prior_variance = prior_variance, prior_sample_size = prior_sample_size, reml = reml,
                                 decomp_scheme = decomp_scheme, keep_on_device = keep_on_device, pvals_df = pv)
    elseif method == "alt-grid"
        res = bulkscan_alt_grid(Y, G, Covar, K, h2_grid; addIntercept = addIntercept, weights = weights,
                                prior_variance = prior_variance, prior_sample_size = prior_sample_size, reml = reml,
                                decomp_scheme = decomp_scheme, keep_on_device = keep_on_device, pvals_df = pv)
    else
        error("Unknown method `$method`; choose null-exact, null-grid or alt-grid.")  # the reference hits an UndefVarError here
    end
    if output_pvals   # src/bulkscan.jl:154-157
        return merge(res, (log10Pvals_mat = _last_log10p(size(res.L), chisq_df), Chisq_df = chisq_df))
    end
    return res
end

# ---- k-degree-of-freedom bulkscan (blmm_bulkscan_multidf; the reference's README lists it as future work): locus l is the columns
# (l - 1) k + 1 .. l k of G and each (locus, trait) pair gets one test of all its columns; L is P x m (P = size(G, 2) / k).  Columns that
# add nothing beyond the covariates and the locus's earlier ones are dropped (complements, duplicates, absent genotypes).  Other
# keywords as bulkscan; chisq_df (output_pvals) defaults to k.  null-grid: k <= 8; null-exact: k <= 4; at most 8 null covariates.
function bulkscan_multidf(Y::Array{Float64, 2}, G::Array{Float64, 2}, K::Array{Float64, 2}, k::Integer; kwargs...)
    return bulkscan_multidf(Y, G, ones(size(Y, 1), 1), K, k; kwargs..., addIntercept = false)
end
function bulkscan_multidf(Y::Array{Float64, 2}, G::Array{Float64, 2}, Covar::Array{Float64, 2}, K::Array{Float64, 2}, k::Integer;
                          method::String = "null-grid", h2_grid::Array{Float64, 1} = collect(0.0:0.1:0.9), addIntercept::Bool = true,
                          weights::Union{Missing, Array{Float64, 1}} = missing, prior_variance::Float64 = 1.0,
                          prior_sample_size::Float64 = 0.0, reml::Bool = false, optim_interval::Int64 = 1,
                          decomp_scheme::String = "eigen", output_pvals::Bool = false, chisq_df::Int64 = Int64(k),
                          keep_on_device::Bool = false)
    (n, m) = size(Y); p = size(G, 2)
    (size(G, 1) != n || size(K, 1) != n || size(K, 2) != n || size(Covar, 1) != n) && error("Dimension mismatch.")
    (weights !== missing && length(weights) != n) && error("Dimension mismatch.")
    method in ("null-grid", "null-exact", "alt-grid") || error("Unknown method `$method`; choose null-exact, null-grid or alt-grid.")
    (k < 1 || p % k != 0) && error("bulkscan_multidf: the number of columns of G must be a multiple of k >= 1")
    check_n(n)
    meth = method == "null-exact" ? NULL_EXACT : method == "null-grid" ? NULL_GRID : ALT_GRID
    o = BlmmOpts(meth, reml, addIntercept, decomp(decomp_scheme), optim_interval, 0, prior_variance, prior_sample_size)
    P = div(p, k)
    L = keep_on_device ? nothing : Array{Float64, 2}(undef, P, m)
    h2 = Array{Float64, 1}(undef, m)
    st = BlmmStatus()
    if output_pvals
        check(ccall((:blmm_set_log10p_output, libblmm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64),
                    context(), Ptr{Float64}(C_NULL), Int64(0), chisq_df))
    end
    GC.@preserve Y G Covar K weights h2_grid L h2 begin
        check(ccall((:blmm_bulkscan_multidf, libblmm), Cint,
                    (Ptr{Cvoid}, Ref{BlmmOpts}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64,
                     Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ref{BlmmStatus}),
                    context(), o, Y, n, m, G, p, Int64(k), Covar, size(Covar, 2), K, ptr_or_null(weights), h2_grid,
                    length(h2_grid), ptr_or_null(L), h2, st))
    end
    raise_status(st)
    res = (L = keep_on_device ? DeviceLOD(P, m) : L, h2_null_list = h2)
    if output_pvals
        return merge(res, (log10Pvals_mat = _last_log10p((P, m), chisq_df), Chisq_df = chisq_df))
    end
    return res
end

# ---- bulkscan_multidf WITHOUT the matrix (blmm_bulkscan_multidf_reduced): per trait the peak LOD and its LOCUS and, `threshold`
# given, every (locus, trait, LOD) with LOD > threshold, out of the k-df scan kernels' epilogues; the P x m matrix is never written.
# The same values as the column maxima / the threshold filter of bulkscan_multidf's L, bit for bit.  Keywords as bulkscan_multidf.
function bulkscan_multidf_reduced(Y::Array{Float64, 2}, G::Array{Float64, 2}, K::Array{Float64, 2}, k::Integer; kwargs...)
    return bulkscan_multidf_reduced(Y, G, ones(size(Y, 1), 1), K, k; kwargs..., addIntercept = false)
end
function bulkscan_multidf_reduced(Y::Array{Float64, 2}, G::Array{Float64, 2}, Covar::Array{Float64, 2}, K::Array{Float64, 2}, k::Integer;
                                  method::String = "null-grid", h2_grid::Array{Float64, 1} = collect(0.0:0.1:0.9),
                                  threshold::Union{Nothing, Float64} = nothing, cap::Int64 = 1048576, addIntercept::Bool = true,
                                  weights::Union{Missing, Array{Float64, 1}} = missing, prior_variance::Float64 = 1.0,
                                  prior_sample_size::Float64 = 0.0, reml::Bool = false, optim_interval::Int64 = 1,
                                  decomp_scheme::String = "eigen")
    (n, m) = size(Y); p = size(G, 2)
    (size(G, 1) != n || size(K, 1) != n || size(K, 2) != n || size(Covar, 1) != n) && error("Dimension mismatch.")
    (weights !== missing && length(weights) != n) && error("Dimension mismatch.")
    method in ("null-grid", "null-exact", "alt-grid") || error("Unknown method `$method`; choose null-exact, null-grid or alt-grid.")
    (k < 1 || p % k != 0) && error("bulkscan_multidf: the number of columns of G must be a multiple of k >= 1")
    (threshold !== nothing && cap < 1) && error("bulkscan_multidf_reduced: `threshold` needs a positive `cap`")
    check_n(n)
    meth = method == "null-exact" ? NULL_EXACT : method == "null-grid" ? NULL_GRID : ALT_GRID
    o = BlmmOpts(meth, reml, addIntercept, decomp(decomp_scheme), optim_interval, 0, prior_variance, prior_sample_size)
    mx = Vector{Float64}(undef, m); arg = Vector{Int64}(undef, m); h2 = Vector{Float64}(undef, m)
    want = threshold !== nothing
    st = BlmmStatus()
    while true
        c1 = max(cap, 1)
        ii = Vector{Int32}(undef, c1); jj = Vector{Int32}(undef, c1); ll = Vector{Float64}(undef, c1); cnt = zeros(Int64, 1)
        GC.@preserve Y G Covar K weights h2_grid mx arg h2 ii jj ll cnt begin
            r = BlmmReduced(pointer(mx), pointer(arg), want ? 1 : 0, want ? threshold : 0.0, want ? cap : 0,
                            pointer(ii), pointer(jj), pointer(ll), pointer(cnt))
            check(ccall((:blmm_bulkscan_multidf_reduced, libblmm), Cint,
                        (Ptr{Cvoid}, Ref{BlmmOpts}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64,
                         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ref{BlmmReduced}, Ptr{Float64}, Ref{BlmmStatus}),
                        context(), o, Y, n, m, G, p, Int64(k), Covar, size(Covar, 2), K, ptr_or_null(weights), h2_grid,
                        length(h2_grid), r, h2, st))
        end
        if !want || cnt[1] <= cap
            raise_status(st)
            res = (max_lod = mx, argmax = arg .+ 1, h2_null_list = h2)   # argmax: 1-based locus, 0: no comparable entry
            want || return res
            nt = cnt[1]
            ord = sortperm(collect(zip(jj[1:nt], ii[1:nt])))
            return merge(res, (locus = Int.(ii[1:nt][ord]) .+ 1, trait = Int.(jj[1:nt][ord]) .+ 1, lod = ll[1:nt][ord]))
        end
        cap = cnt[1]
    end
end
# ... on DEVICE buffers (`out` holds device pointers; 0-based loci / traits, as the C ABI); returns when the results are complete
function bulkscan_multidf_reduced_dev!(dY::Ptr{Float64}, n::Int64, m::Int64, dG::Ptr{Float64}, p::Int64, k::Int64, dK::Ptr{Float64},
                                       out::BlmmReduced, dh2::Ptr{Float64}; method::String = "null-grid",
                                       h2_grid::Array{Float64, 1} = collect(0.0:0.1:0.9), dCovar::Ptr{Float64} = Ptr{Float64}(C_NULL),
                                       ncov::Int64 = 0, dweights::Ptr{Float64} = Ptr{Float64}(C_NULL), addIntercept::Bool = true,
                                       prior_variance::Float64 = 1.0, prior_sample_size::Float64 = 0.0, reml::Bool = false,
                                       optim_interval::Int64 = 1, decomp_scheme::String = "eigen")
    method in ("null-grid", "null-exact", "alt-grid") || error("Unknown method `$method`; choose null-exact, null-grid or alt-grid.")
    check_n(n)
    meth = method == "null-exact" ? NULL_EXACT : method == "null-grid" ? NULL_GRID : ALT_GRID
    o = BlmmOpts(meth, reml, ncov == 0 ? true : addIntercept, decomp(decomp_scheme), optim_interval, 0, prior_variance, prior_sample_size)
    st = BlmmStatus()
    GC.@preserve h2_grid begin
        check(ccall((:blmm_bulkscan_multidf_reduced_dev, libblmm), Cint,
                    (Ptr{Cvoid}, Ref{BlmmOpts}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64,
                     Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ref{BlmmReduced}, Ptr{Float64}, Ref{BlmmStatus}),
                    context(), o, dY, n, m, dG, p, k, dCovar, ncov, dK, dweights, h2_grid, length(h2_grid), out, dh2, st))
    end
    raise_status(st)
    return nothing
end

# ---- conditional bulkscan (blmm_bulkscan_cond): column j of L is the scan of trait j with the null design [Covar G[:, cond[j, :]]].
# cond: m (or m x s, s <= 4) 1-based columns of G, 0 for none; or "peak": bulkscan_reduced first, every trait conditioned on its peak.
# Markers collinear with a trait's design (the conditioning marker itself) get LOD 0.  Returns L, h2_null_list (with the loci in the
# null model), cond (as used, 1-based), n_rule_zero, n_cond_dropped, n_cond_traits.
function bulkscan_cond(Y::Array{Float64, 2}, G::Array{Float64, 2}, K::Array{Float64, 2}, cond; kwargs...)
    return bulkscan_cond(Y, G, ones(size(Y, 1), 1), K, cond; kwargs..., addIntercept = false)
end
function bulkscan_cond(Y::Array{Float64, 2}, G::Array{Float64, 2}, Covar::Array{Float64, 2}, K::Array{Float64, 2}, cond;
                       method::String = "null-grid", h2_grid::Array{Float64, 1} = collect(0.0:0.1:0.9), addIntercept::Bool = true,
                       weights::Union{Missing, Array{Float64, 1}} = missing, prior_variance::Float64 = 1.0,
                       prior_sample_size::Float64 = 0.0, reml::Bool = false, optim_interval::Int64 = 1,
                       decomp_scheme::String = "eigen", output_pvals::Bool = false, chisq_df::Int64 = 1,
                       keep_on_device::Bool = false)
    (n, m) = size(Y); p = size(G, 2)
    (size(G, 1) != n || size(K, 1) != n || size(K, 2) != n || size(Covar, 1) != n) && error("Dimension mismatch.")
    (weights !== missing && length(weights) != n) && error("Dimension mismatch.")
    method in ("null-grid", "null-exact", "alt-grid") || error("Unknown method `$method`; choose null-exact, null-grid or alt-grid.")
    method == "alt-grid" && error("bulkscan_cond: alt-grid is not supported; use null-grid or null-exact")
    check_n(n)
    if cond isa AbstractString
        cond == "peak" || error("bulkscan_cond: cond is an index array or the string \"peak\"")
        red = bulkscan_reduced(Y, G, Covar, K; method = method, h2_grid = h2_grid, addIntercept = addIntercept, weights = weights,
                               prior_variance = prior_variance, prior_sample_size = prior_sample_size, reml = reml,
                               optim_interval = optim_interval, decomp_scheme = decomp_scheme)
        cond = reshape(Int64.(red.argmax), m, 1)
    end
    cmat = ndims(cond) == 1 ? reshape(Int64.(cond), :, 1) : Int64.(cond)
    size(cmat, 1) == m || error("bulkscan_cond: cond must have m rows")
    s = size(cmat, 2)
    s <= 4 || error("bulkscan_cond: at most 4 conditioning loci per trait")
    all(0 .<= cmat .<= p) || error("bulkscan_cond: a conditioning index outside 0 .. p")
    ctab = Array{Int64, 2}(permutedims(cmat .- 1))      # s x m, 0-based, -1: none
    meth = method == "null-exact" ? NULL_EXACT : NULL_GRID
    o = BlmmOpts(meth, reml, addIntercept, decomp(decomp_scheme), optim_interval, 0, prior_variance, prior_sample_size)
    L = keep_on_device ? nothing : Array{Float64, 2}(undef, p, m)
    h2 = Array{Float64, 1}(undef, m)
    info = zeros(Int64, 4)
    st = BlmmStatus()
    if output_pvals
        check(ccall((:blmm_set_log10p_output, libblmm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64),
                    context(), Ptr{Float64}(C_NULL), Int64(0), chisq_df))
    end
    GC.@preserve Y G Covar K weights h2_grid ctab L h2 info begin
        check(ccall((:blmm_bulkscan_cond, libblmm), Cint,
                    (Ptr{Cvoid}, Ref{BlmmOpts}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64,
                     Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Int64},
                     Ref{BlmmStatus}),
                    context(), o, Y, n, m, G, p, Covar, size(Covar, 2), K, ptr_or_null(weights), h2_grid,
                    length(h2_grid), ctab, Int64(s), ptr_or_null(L), h2, info, st))
    end
    raise_status(st)
    res = (L = keep_on_device ? DeviceLOD(p, m) : L, h2_null_list = h2, cond = cmat, n_rule_zero = info[1],
           n_cond_dropped = info[2], n_cond_traits = info[3])
    if output_pvals
        return merge(res, (log10Pvals_mat = _last_log10p((p, m), chisq_df), Chisq_df = chisq_df))
    end
    return res
end

# blmm_bulkscan_stepwise's refusals that need no data (blmm_api.hip: stepwise_check, then cond_check), with its messages and in its order; c: the
# columns of the null design without the loci
function stepwise_checks(method::String, n::Int64, max_loci::Int64, threshold::Float64, c::Int64)
    max_loci >= 1 || error("bulkscan_stepwise: max_loci must be at least 1")
    max_loci <= 4 || error("bulkscan_stepwise: at most 4 loci per trait")
    c + max_loci <= 8 || error("bulkscan_stepwise: more than 8 null-design columns (covariates incl. intercept + max_loci) are not supported")
    threshold >= 0.0 || error("bulkscan_stepwise: the threshold must be a number >= 0")
    method in ("null-grid", "null-exact", "alt-grid") || error("Unknown method `$method`; choose null-exact, null-grid or alt-grid.")
    method == "alt-grid" && error("bulkscan_cond: alt-grid is not supported; use null-grid or null-exact")
    check_n(n)
    c + max_loci < n || error("Dimension mismatch.")
    return nothing
end

# ---- forward selection (blmm_bulkscan_stepwise): up to max_loci loci per trait.  Round t scans the traits still active with the loci
# they have so far in the null model (bulkscan_cond's column, reduced to its maximum); a trait whose peak LOD is above `threshold`
# takes the peak marker as its next locus.  Returns loci (m x S, 1-based, 0 beyond a trait's loci: bulkscan_cond takes it as cond),
# lod / argmax / h2 (m x (S + 1); NaN / 0 / NaN for the rounds a trait was not active in), nloci, rounds, active (traits per round),
# n_rule_zero, n_cond_traits.
function bulkscan_stepwise(Y::Array{Float64, 2}, G::Array{Float64, 2}, K::Array{Float64, 2}; kwargs...)
    return bulkscan_stepwise(Y, G, ones(size(Y, 1), 1), K; kwargs..., addIntercept = false)
end
function bulkscan_stepwise(Y::Array{Float64, 2}, G::Array{Float64, 2}, Covar::Array{Float64, 2}, K::Array{Float64, 2};
                           max_loci::Int64 = 4, threshold::Float64, method::String = "null-grid",
                           h2_grid::Array{Float64, 1} = collect(0.0:0.1:0.9), addIntercept::Bool = true,
                           weights::Union{Missing, Array{Float64, 1}} = missing, prior_variance::Float64 = 1.0,
                           prior_sample_size::Float64 = 0.0, reml::Bool = false, optim_interval::Int64 = 1,
                           decomp_scheme::String = "eigen")
    (n, m) = size(Y); p = size(G, 2)
    (size(G, 1) != n || size(K, 1) != n || size(K, 2) != n || size(Covar, 1) != n) && error("Dimension mismatch.")
    (weights !== missing && length(weights) != n) && error("Dimension mismatch.")
    stepwise_checks(method, n, max_loci, threshold, size(Covar, 2) + (addIntercept ? 1 : 0))
    S = max_loci
    meth = method == "null-exact" ? NULL_EXACT : NULL_GRID
    o = BlmmOpts(meth, reml, addIntercept, decomp(decomp_scheme), optim_interval, 0, prior_variance, prior_sample_size)
    loci = Array{Int64, 2}(undef, S, m)
    lod = Array{Float64, 2}(undef, S + 1, m); arg = Array{Int64, 2}(undef, S + 1, m); h2 = Array{Float64, 2}(undef, S + 1, m)
    nloci = Array{Int64, 1}(undef, m)
    info = zeros(Int64, 8)
    st = BlmmStatus()
    GC.@preserve Y G Covar K weights h2_grid loci lod arg h2 nloci info begin
        check(ccall((:blmm_bulkscan_stepwise, libblmm), Cint,
                    (Ptr{Cvoid}, Ref{BlmmOpts}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64,
                     Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Float64, Ptr{Int64}, Ptr{Float64}, Ptr{Int64},
                     Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ref{BlmmStatus}),
                    context(), o, Y, n, m, G, p, Covar, size(Covar, 2), K, ptr_or_null(weights), h2_grid,
                    length(h2_grid), Int64(S), threshold, loci, lod, arg, h2, nloci, info, st))
    end
    raise_status(st)
    return (loci = permutedims(loci) .+ 1, lod = permutedims(lod), argmax = permutedims(arg) .+ 1, h2 = permutedims(h2),
            nloci = nloci, rounds = info[1], active = info[4:4 + S], n_rule_zero = info[3], n_cond_traits = info[2])
end
# ... on DEVICE buffers (0-based markers, -1 for none, as the C ABI): dloci S x m, dlod / dargmax / dh2 (S + 1) x m, dnloci m,
# dsinfo 8 or C_NULL.  Returns when the results are complete.
function bulkscan_stepwise_dev!(dY::Ptr{Float64}, n::Int64, m::Int64, dG::Ptr{Float64}, p::Int64, dK::Ptr{Float64}, max_loci::Int64,
                                threshold::Float64, dloci::Ptr{Int64}, dlod::Ptr{Float64}, dargmax::Ptr{Int64}, dh2::Ptr{Float64},
                                dnloci::Ptr{Int64}; dsinfo::Ptr{Int64} = Ptr{Int64}(C_NULL), method::String = "null-grid",
                                h2_grid::Array{Float64, 1} = collect(0.0:0.1:0.9), dCovar::Ptr{Float64} = Ptr{Float64}(C_NULL),
                                ncov::Int64 = 0, dweights::Ptr{Float64} = Ptr{Float64}(C_NULL), addIntercept::Bool = true,
                                prior_variance::Float64 = 1.0, prior_sample_size::Float64 = 0.0, reml::Bool = false,
                                optim_interval::Int64 = 1, decomp_scheme::String = "eigen")
    stepwise_checks(method, n, max_loci, threshold, ncov == 0 ? 1 : ncov + (addIntercept ? 1 : 0))
    meth = method == "null-exact" ? NULL_EXACT : NULL_GRID
    o = BlmmOpts(meth, reml, ncov == 0 ? true : addIntercept, decomp(decomp_scheme), optim_interval, 0, prior_variance, prior_sample_size)
    st = BlmmStatus()
    GC.@preserve h2_grid begin
        check(ccall((:blmm_bulkscan_stepwise_dev, libblmm), Cint,
                    (Ptr{Cvoid}, Ref{BlmmOpts}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64,
                     Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Float64, Ptr{Int64}, Ptr{Float64}, Ptr{Int64},
                     Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ref{BlmmStatus}),
                    context(), o, dY, n, m, dG, p, dCovar, ncov, dK, dweights, h2_grid, length(h2_grid), max_loci, threshold,
                    dloci, dlod, dargmax, dh2, dnloci, dsinfo, st))
    end
    raise_status(st)
    return nothing
end

# ---- effects at chosen tests (blmm_bulkscan_effects): coefficients and standard errors of the locus columns in the weighted
# least-squares fit wls(y0_j, [Z0 X0_l], w) under trait j's null h2, for tests (locus[t], trait[t]) -- 1-based here -- in any order.
# beta, se: k x T (column t = test t; a column the rank rule drops has 0 in both); sigma2 (wls's sigma2_e of the fit), lod (what
# bulkscan / bulkscan_multidf has at L[locus, trait]), accepted (bit mask of the columns kept): T.  k <= 8 for both methods, at most
# 8 null covariates, alt-grid is refused.  LOCO: call once per chromosome with calcKinship_loco's kinship of it and its tests.
function bulkscan_effects(Y::Array{Float64, 2}, G::Array{Float64, 2}, K::Array{Float64, 2}, k::Integer, locus::Array{Int64, 1},
                          trait::Array{Int64, 1}; kwargs...)
    return bulkscan_effects(Y, G, ones(size(Y, 1), 1), K, k, locus, trait; kwargs..., addIntercept = false)
end
function bulkscan_effects(Y::Array{Float64, 2}, G::Array{Float64, 2}, Covar::Array{Float64, 2}, K::Array{Float64, 2}, k::Integer,
                          locus::Array{Int64, 1}, trait::Array{Int64, 1};
                          method::String = "null-grid", h2_grid::Array{Float64, 1} = collect(0.0:0.1:0.9), addIntercept::Bool = true,
                          weights::Union{Missing, Array{Float64, 1}} = missing, prior_variance::Float64 = 1.0,
                          prior_sample_size::Float64 = 0.0, reml::Bool = false, optim_interval::Int64 = 1,
                          decomp_scheme::String = "eigen")
    (n, m) = size(Y); p = size(G, 2)
    (size(G, 1) != n || size(K, 1) != n || size(K, 2) != n || size(Covar, 1) != n) && error("Dimension mismatch.")
    (weights !== missing && length(weights) != n) && error("Dimension mismatch.")
    method in ("null-grid", "null-exact", "alt-grid") || error("Unknown method `$method`; choose null-exact, null-grid or alt-grid.")
    (k < 1 || p % k != 0) && error("bulkscan_effects: the number of columns of G must be a multiple of k >= 1")
    check_n(n)
    T = length(locus)
    length(trait) == T || error("bulkscan_effects: locus and trait must have the same length")
    (all(1 .<= locus .<= div(p, k)) && all(1 .<= trait .<= m)) || error("bulkscan_effects: a locus or trait index is out of range")
    meth = method == "null-exact" ? NULL_EXACT : method == "null-grid" ? NULL_GRID : ALT_GRID
    o = BlmmOpts(meth, reml, addIntercept, decomp(decomp_scheme), optim_interval, 0, prior_variance, prior_sample_size)
    loc0 = locus .- 1; tr0 = trait .- 1
    beta = Array{Float64, 2}(undef, k, T); se = Array{Float64, 2}(undef, k, T)
    sigma2 = Array{Float64, 1}(undef, T); lod = Array{Float64, 1}(undef, T); accepted = Array{Int32, 1}(undef, T)
    h2 = Array{Float64, 1}(undef, m)
    st = BlmmStatus()
    GC.@preserve Y G Covar K weights h2_grid loc0 tr0 beta se sigma2 lod accepted h2 begin
        check(ccall((:blmm_bulkscan_effects, libblmm), Cint,
                    (Ptr{Cvoid}, Ref{BlmmOpts}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64,
                     Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Float64},
                     Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ref{BlmmStatus}),
                    context(), o, Y, n, m, G, p, Int64(k), Covar, size(Covar, 2), K, ptr_or_null(weights), h2_grid,
                    length(h2_grid), loc0, tr0, Int64(T), beta, se, sigma2, lod, accepted, h2, st))
    end
    raise_status(st)
    return (beta = beta, se = se, sigma2 = sigma2, lod = lod, accepted = accepted, h2_null_list = h2)
end

# ---- the bulk form of scan(...; assumption = "alt") (scan_alt, src/scan.jl:397-453; not in the reference, which has the
# single-trait function and the grid approximation bulkscan_alt_grid): the exact heritability of EVERY (trait, marker) test
function bulkscan_alt_exact(Y::Array{Float64, 2}, G::Array{Float64, 2}, Covar::Array{Float64, 2}, K::Array{Float64, 2};
                            addIntercept::Bool = true, weights::Union{Missing, Array{Float64, 1}} = missing,
                            prior_variance::Float64 = 0.0, prior_sample_size::Float64 = 0.0, reml::Bool = false,
                            optim_interval::Int64 = 1, decomp_scheme::String = "eigen")
    n = size(Y, 1); m = size(Y, 2); p = size(G, 2)
    (size(G, 1) != n || size(K, 1) != n || size(K, 2) != n || size(Covar, 1) != n) && error("Dimension mismatch.")
    check_n(n)
    (weights !== missing && length(weights) != n) && error("Dimension mismatch.")
    o = BlmmOpts(NULL_EXACT, reml, addIntercept, decomp(decomp_scheme), optim_interval, 0, prior_variance, prior_sample_size)
    L = Array{Float64, 2}(undef, p, m); H = Array{Float64, 2}(undef, p, m)
    h2 = Array{Float64, 1}(undef, m); s2 = Array{Float64, 1}(undef, m); st = BlmmStatus()
    GC.@preserve Y G Covar K weights L H h2 s2 check(ccall((:blmm_bulkscan_alt_exact, libblmm), Cint,
        (Ptr{Cvoid}, Ref{BlmmOpts}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{BlmmStatus}),
        context(), o, Y, n, m, G, p, Covar, size(Covar, 2), K, ptr_or_null(weights), L, H, h2, s2, st))
    raise_status(st)
    return (L = L, h2_panel = H, h2_null_list = h2, sigma2_e = s2)
end
bulkscan_alt_exact(Y::Array{Float64, 2}, G::Array{Float64, 2}, K::Array{Float64, 2}; kwargs...) =
    bulkscan_alt_exact(Y, G, ones(size(Y, 1), 1), K; addIntercept = false, kwargs...)

# ---- several GPUs of one node in ONE call (blmm_bulkscan_multi): the trait blocks the reference deals to its threads
# (src/bulkscan.jl:263-309) go to the devices; gather = :host_shards (default) | :none | :allgather
const _mctx = Ref{Ptr{Cvoid}}(C_NULL)
const _mctx_devices = Ref{Vector{Int32}}(Int32[])
function multi_context(devices::Vector{Int32} = Int32[])
    if _mctx[] != C_NULL && _mctx_devices[] != devices      # a different device list: a new context (the old one is released)
        ccall((:blmm_destroy_multi, libblmm), Cvoid, (Ptr{Cvoid},), _mctx[])
        _mctx[] = C_NULL
    end
    if _mctx[] == C_NULL
        h = Ref{Ptr{Cvoid}}(C_NULL)
        rc = GC.@preserve devices ccall((:blmm_create_multi, libblmm), Cint, (Ptr{Int32}, Cint, Ref{Ptr{Cvoid}}),
                                        isempty(devices) ? Ptr{Int32}(C_NULL) : pointer(devices), length(devices), h)
        rc == 0 || error(unsafe_string(ccall((:blmm_err_string, libblmm), Cstring, (Cint,), rc)))
        _mctx[] = h[]
        _mctx_devices[] = copy(devices)
    end
    return _mctx[]
end
struct BlmmMultiOpts; gather_mode::Int32; reserved::Int32; end
function bulkscan_multi(Y::Array{Float64, 2}, G::Array{Float64, 2}, K::Array{Float64, 2};
                        method::String = "null-grid", h2_grid::Array{Float64, 1} = collect(0.0:0.1:0.9),
                        gather::Symbol = :host_shards, devices::Vector{Int32} = Int32[],
                        weights::Union{Missing, Array{Float64, 1}} = missing,
                        prior_variance::Float64 = 1.0, prior_sample_size::Float64 = 0.0,
                        reml::Bool = false, optim_interval::Int64 = 1, decomp_scheme::String = "eigen")
    meth = method == "null-exact" ? NULL_EXACT : method == "null-grid" ? NULL_GRID : method == "alt-grid" ? ALT_GRID :
           error("Unknown method `$method`; choose null-exact, null-grid or alt-grid.")
    (n, m) = size(Y); p = size(G, 2)
    (size(G, 1) != n || size(K, 1) != n || size(K, 2) != n) && error("Dimension mismatch.")
    check_n(n)
    (weights !== missing && length(weights) != n) && error("Dimension mismatch.")
    o = BlmmOpts(meth, reml, true, decomp(decomp_scheme), optim_interval, 0, prior_variance, prior_sample_size)
    mo = BlmmMultiOpts(gather == :none ? 0 : gather == :allgather ? 2 : 1, 0)
    L = Array{Float64, 2}(undef, p, m)
    h2 = meth == ALT_GRID ? Array{Float64, 2}(undef, p, m) : Array{Float64, 1}(undef, m)
    mc = multi_context(devices)
    ndev = ccall((:blmm_multi_ndev, libblmm), Cint, (Ptr{Cvoid},), mc)
    sts = [BlmmStatus() for _ in 1:ndev]                 # one status per device: the warnings / errors of every shard are raised
    stbuf = Vector{UInt8}(undef, ndev * sizeof(BlmmStatus))
    GC.@preserve Y G K weights h2_grid L h2 stbuf begin
        rc = ccall((:blmm_bulkscan_multi, libblmm), Cint,
                   (Ptr{Cvoid}, Ref{BlmmOpts}, Ref{BlmmMultiOpts}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64,
                    Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
                   mc, o, mo, Y, n, m, G, p, C_NULL, 0, K, ptr_or_null(weights), h2_grid, length(h2_grid), L, h2, pointer(stbuf))
        rc == 0 || error(unsafe_string(ccall((:blmm_multi_last_error, libblmm), Cstring, (Ptr{Cvoid},), mc)))
        for r in 1:ndev
            sts[r] = unsafe_load(Ptr{BlmmStatus}(pointer(stbuf)) , r)
        end
    end
    foreach(raise_status, sts)
    return meth == ALT_GRID ? (L = L, h2_panel = h2) : (L = L, h2_null_list = h2)
end

# ---- scan: the reference's four methods (src/scan.jl:94-120, 122-148, 150-180, 182-271).  On the GPU path:
#   assumption = "null" and "alt" (scan_alt, src/scan.jl:397-453: one Brent search per marker on the device, blmm_scan_alt);
#   method ("qr" / "cholesky") selects a CPU factorisation and has no meaning here: accepted, ignored;
#   profileLL = true (profile_LL of src/analysis_helpers) is not part of this path: a clear error.
function scan(y::Array{Float64, 1}, g::Array{Float64, 2}, K::Array{Float64, 2};
              weights::Union{Missing, Array{Float64, 1}} = missing,
              prior_variance::Float64 = 0.0, prior_sample_size::Float64 = 0.0, addIntercept::Bool = true,
              reml::Bool = false, assumption::String = "null", method::String = "qr", optim_interval::Int64 = 1,
              permutation_test::Bool = false, nperms::Int64 = 1024, rndseed::Int64 = 0,
              profileLL::Bool = false, markerID::Int = 0, h2_grid::Array{Float64, 1} = Array{Float64, 1}(undef, 1),
              decomp_scheme::String = "eigen",
              output_pvals::Bool = false, chisq_df::Int64 = 1,
              perm_precision::String = "f64")   # "f32" (not in the reference): L_perms on the fp32 matrix cores, as Float32
    return scan(reshape(y, :, 1), g, K; weights = weights, addIntercept = addIntercept, prior_variance = prior_variance,
                prior_sample_size = prior_sample_size, reml = reml, assumption = assumption, method = method,
                optim_interval = optim_interval, permutation_test = permutation_test, nperms = nperms, rndseed = rndseed,
                profileLL = profileLL, markerID = markerID, h2_grid = h2_grid, decomp_scheme = decomp_scheme,
                output_pvals = output_pvals, chisq_df = chisq_df, perm_precision = perm_precision)
end
function scan(y::Array{Float64, 1}, g::Array{Float64, 2}, covar::Array{Float64, 2}, K::Array{Float64, 2};
              weights::Union{Missing, Array{Float64, 1}} = missing,
              prior_variance::Float64 = 0.0, prior_sample_size::Float64 = 0.0, addIntercept::Bool = true,
              reml::Bool = false, assumption::String = "null", method::String = "qr", optim_interval::Int64 = 1,
              permutation_test::Bool = false, nperms::Int64 = 1024, rndseed::Int64 = 0,
              profileLL::Bool = false, markerID::Int = 0, h2_grid::Array{Float64, 1} = Array{Float64, 1}(undef, 1),
              decomp_scheme::String = "eigen",
              output_pvals::Bool = false, chisq_df::Int64 = 1,
              perm_precision::String = "f64")
    return scan(reshape(y, :, 1), g, covar, K; weights = weights, addIntercept = addIntercept, prior_variance = prior_variance,
                prior_sample_size = prior_sample_size, reml = reml, assumption = assumption, method = method,
                optim_interval = optim_interval, permutation_test = permutation_test, nperms = nperms, rndseed = rndseed,
                profileLL = profileLL, markerID = markerID, h2_grid = h2_grid, decomp_scheme = decomp_scheme,
                output_pvals = output_pvals, chisq_df = chisq_df, perm_precision = perm_precision)
end
function scan(y::Array{Float64, 2}, g::Array{Float64, 2}, K::Array{Float64, 2};
              weights::Union{Missing, Array{Float64, 1}} = missing,
              prior_variance::Float64 = 0.0, prior_sample_size::Float64 = 0.0, addIntercept::Bool = true,
              reml::Bool = false, assumption::String = "null", method::String = "qr", optim_interval::Int64 = 1,
              permutation_test::Bool = false, nperms::Int64 = 1024, rndseed::Int64 = 0,
              profileLL::Bool = false, markerID::Int = 0, h2_grid::Array{Float64, 1} = Array{Float64, 1}(undef, 1),
              decomp_scheme::String = "eigen",
              output_pvals::Bool = false, chisq_df::Int64 = 1,
              perm_precision::String = "f64")
    addIntercept || error("Intercept has to be added when no other covariate is given.")   # src/scan.jl:167-169
    return scan(y, g, ones(size(y, 1), 1), K; weights = weights, addIntercept = false, prior_variance = prior_variance,
                prior_sample_size = prior_sample_size, reml = reml, assumption = assumption, method = method,
                optim_interval = optim_interval, permutation_test = permutation_test, nperms = nperms, rndseed = rndseed,
                profileLL = profileLL, markerID = markerID, h2_grid = h2_grid, decomp_scheme = decomp_scheme,
                output_pvals = output_pvals, chisq_df = chisq_df, perm_precision = perm_precision)
end
function scan(y::Array{Float64, 2}, g::Array{Float64, 2}, covar::Array{Float64, 2}, K::Array{Float64, 2};
              weights::Union{Missing, Array{Float64, 1}} = missing,
              prior_variance::Float64 = 0.0, prior_sample_size::Float64 = 0.0, addIntercept::Bool = true,
              reml::Bool = false, assumption::String = "null", method::String = "qr", optim_interval::Int64 = 1,
              permutation_test::Bool = false, nperms::Int64 = 1024, rndseed::Int64 = 0,
              profileLL::Bool = false, markerID::Int = 0, h2_grid::Array{Float64, 1} = Array{Float64, 1}(undef, 1),
              decomp_scheme::String = "eigen",
              output_pvals::Bool = false, chisq_df::Int64 = 1,
              perm_precision::String = "f64")
    assumption == "alt" && permutation_test && error("Permutation test option currently is not supported for the alternative assumption.")
    assumption in ("null", "alt") || error("Assumption keyword is not supported. Please enter null or alt.")
    profileLL && error("profileLL = true (profile_LL) is not part of the GPU path; call BulkLMM.scan for it")
    size(y, 2) == 1 || error("Can only handle one trait.")                                   # src/scan.jl:496-498
    n = size(y, 1); p = size(g, 2)
    (size(g, 1) != n || size(K, 1) != n || size(K, 2) != n || size(covar, 1) != n) && error("Dimension mismatch.")
    check_n(n)
    (weights !== missing && length(weights) != n) && error("Dimension mismatch.")
    np = permutation_test ? nperms : 0
    np < 0 && error("The required number of permutations must be a positive integer.")
    perm_precision in ("f64", "f32") || error("perm_precision must be \"f64\" or \"f32\".")
    # `weights`, the intercept and the covariates go to the library as they are: it applies W (src/scan.jl:200-221) itself
    o = BlmmOpts(NULL_EXACT, reml, addIntercept, decomp(decomp_scheme), optim_interval, 0, prior_variance, prior_sample_size)
    scal = zeros(2); lod = Array{Float64, 1}(undef, p); st = BlmmStatus()
    ncov = size(covar, 2)
    if assumption == "alt"   # scan_alt (src/scan.jl:397-453): one Brent search per marker on the device
        h2_each = Array{Float64, 1}(undef, p)
        GC.@preserve y g covar K weights scal lod h2_each check(ccall((:blmm_scan_alt, libblmm), Cint,
            (Ptr{Cvoid}, Ref{BlmmOpts}, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64},
             Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{BlmmStatus}),
            context(), o, y, n, g, p, covar, ncov, K, ptr_or_null(weights), scal, lod, h2_each, st))
        raise_status(st)
        res = (sigma2_e = scal[1], h2_null = scal[2], h2_each_marker = h2_each, lod = lod)
        return output_pvals ? merge(res, (log10pvals = lod2log10p(lod, chisq_df),)) : res
    end
    f32 = perm_precision == "f32"
    Lp = f32 ? Array{Float32, 2}(undef, p, max(np, 1)) : Array{Float64, 2}(undef, p, max(np, 1))
    GC.@preserve y g covar K weights scal lod Lp begin
        if f32
            check(ccall((:blmm_scan_perms_f32, libblmm), Cint,
                        (Ptr{Cvoid}, Ref{BlmmOpts}, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64},
                         Ptr{Float64}, Int64, UInt64, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float32}, Ref{BlmmStatus}),
                        context(), o, y, n, g, p, covar, ncov, K, ptr_or_null(weights), np, UInt64(rndseed), C_NULL, scal, lod, Lp, st))
        else
            check(ccall((:blmm_scan_perms, libblmm), Cint,
                        (Ptr{Cvoid}, Ref{BlmmOpts}, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64},
                         Ptr{Float64}, Int64, UInt64, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{BlmmStatus}),
                        context(), o, y, n, g, p, covar, ncov, K, ptr_or_null(weights), np, UInt64(rndseed), C_NULL, scal, lod, Lp, st))
        end
    end
    raise_status(st)
    res = permutation_test ? (sigma2_e = scal[1], h2_null = scal[2], lod = lod, L_perms = Lp[:, 1:np]) :
                             (sigma2_e = scal[1], h2_null = scal[2], lod = lod)
    if output_pvals   # src/scan.jl:353-355; with permutations the reference hits an UndefVarError (src/scan.jl:551): fixed
        res = merge(res, (log10pvals = lod2log10p(lod, chisq_df),))
    end
    return res
end

# get_thresholds (src/analysis_helpers/single_trait_analysis.jl:13-23): column maxima, sort, quantile on the GPU
function get_thresholds(L_perms::Array{Float64, 2}, signif_level::Array{Float64, 1})
    probs = 1.0 .- signif_level
    thrs = similar(probs)
    GC.@preserve L_perms probs thrs check(ccall((:blmm_get_thresholds, libblmm), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}),
        context(), L_perms, size(L_perms, 1), size(L_perms, 2), probs, length(probs), thrs))
    return (probs = probs, thrs = thrs)
end

# The permutation test for EVERY trait (blmm_bulkscan_perms): per trait scan(Y[:, j], ...; permutation_test = true) under ONE
# permutation set (the library's generator from rndseed), reduced on the device -- peak, genome-wide permutation maxima,
# get_thresholds and the empirical p-value; lod_argmax is 1-based here (0 = no comparable LOD).
function bulkscan_perms(Y::Array{Float64, 2}, G::Array{Float64, 2}, Covar::Union{Nothing, Array{Float64, 2}}, K::Array{Float64, 2};
                        nperms::Int64 = 1024, rndseed::Int64 = 0, signif_level::Array{Float64, 1} = [0.10, 0.05],
                        weights::Union{Missing, Array{Float64, 1}} = missing, prior_variance::Float64 = 0.0,
                        prior_sample_size::Float64 = 0.0, addIntercept::Bool = true, reml::Bool = false,
                        optim_interval::Int64 = 1, decomp_scheme::String = "eigen")
    n, m = size(Y); p = size(G, 2)
    (size(G, 1) != n || size(K, 1) != n || size(K, 2) != n || (Covar !== nothing && size(Covar, 1) != n)) && error("Dimension mismatch.")
    check_n(n)
    (weights !== missing && length(weights) != n) && error("Dimension mismatch.")
    nperms < 0 && error("The required number of permutations must be a positive integer.")
    o = BlmmOpts(NULL_EXACT, reml, addIntercept, decomp(decomp_scheme), optim_interval, 0, prior_variance, prior_sample_size)
    probs = 1.0 .- signif_level
    h2 = Array{Float64, 1}(undef, m); s2 = similar(h2); mx = similar(h2); pv = similar(h2)
    arg = Array{Int64, 1}(undef, m)
    mp = Array{Float64, 2}(undef, max(nperms, 1), m); thr = Array{Float64, 2}(undef, length(probs), m)
    st = BlmmStatus()
    ncov = Covar === nothing ? 0 : size(Covar, 2)
    GC.@preserve Y G Covar K weights probs h2 s2 mx arg mp thr pv check(ccall((:blmm_bulkscan_perms, libblmm), Cint,
        (Ptr{Cvoid}, Ref{BlmmOpts}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64},
         Ptr{Float64}, Int64, UInt64, Ptr{Int32}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{BlmmStatus}),
        context(), o, Y, n, m, G, p, ptr_or_null(Covar), ncov, K, ptr_or_null(weights), nperms, UInt64(rndseed), C_NULL, probs,
        length(probs), h2, s2, mx, arg, mp, thr, pv, st))
    raise_status(st)
    return (h2_null = h2, sigma2_e = s2, lod_max = mx, lod_argmax = arg .+ 1, max_perms = mp[1:nperms, :],
            thresholds = thr, pvals_perm = pv)
end

# Permutation thresholds of the k-degree-of-freedom scan (blmm_bulkscan_multidf_perms): bulkscan_perms with bulkscan_multidf's loci
# (locus l = columns (l - 1) k + 1 .. l k of G, 1 <= k <= 8, the rank rule at each trait's own weights).  The null fit and the
# permutation set are bulkscan_perms'; lod_argmax is a 1-based LOCUS here (0 = no comparable LOD).
function bulkscan_multidf_perms(Y::Array{Float64, 2}, G::Array{Float64, 2}, Covar::Union{Nothing, Array{Float64, 2}}, K::Array{Float64, 2},
                                k::Integer; nperms::Int64 = 1024, rndseed::Int64 = 0, signif_level::Array{Float64, 1} = [0.10, 0.05],
                                weights::Union{Missing, Array{Float64, 1}} = missing, prior_variance::Float64 = 0.0,
                                prior_sample_size::Float64 = 0.0, addIntercept::Bool = true, reml::Bool = false,
                                optim_interval::Int64 = 1, decomp_scheme::String = "eigen")
    n, m = size(Y); p = size(G, 2)
    (size(G, 1) != n || size(K, 1) != n || size(K, 2) != n || (Covar !== nothing && size(Covar, 1) != n)) && error("Dimension mismatch.")
    (weights !== missing && length(weights) != n) && error("Dimension mismatch.")
    nperms < 0 && error("The required number of permutations must be a positive integer.")
    (k < 1 || p % k != 0) && error("bulkscan_multidf_perms: the number of columns of G must be a multiple of k >= 1")
    check_n(n)
    o = BlmmOpts(NULL_EXACT, reml, addIntercept, decomp(decomp_scheme), optim_interval, 0, prior_variance, prior_sample_size)
    probs = 1.0 .- signif_level
    h2 = Array{Float64, 1}(undef, m); s2 = similar(h2); mx = similar(h2); pv = similar(h2)
    arg = Array{Int64, 1}(undef, m)
    mp = Array{Float64, 2}(undef, max(nperms, 1), m); thr = Array{Float64, 2}(undef, length(probs), m)
    st = BlmmStatus()
    ncov = Covar === nothing ? 0 : size(Covar, 2)
    GC.@preserve Y G Covar K weights probs h2 s2 mx arg mp thr pv check(ccall((:blmm_bulkscan_multidf_perms, libblmm), Cint,
        (Ptr{Cvoid}, Ref{BlmmOpts}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64},
         Ptr{Float64}, Int64, UInt64, Ptr{Int32}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{BlmmStatus}),
        context(), o, Y, n, m, G, p, Int64(k), ptr_or_null(Covar), ncov, K, ptr_or_null(weights), nperms, UInt64(rndseed), C_NULL,
        probs, length(probs), h2, s2, mx, arg, mp, thr, pv, st))
    raise_status(st)
    return (h2_null = h2, sigma2_e = s2, lod_max = mx, lod_argmax = arg .+ 1, max_perms = mp[1:nperms, :],
            thresholds = thr, pvals_perm = pv)
end

# ---- on-device consumers of L (README.md:246-255, 354-359) -------------------------------------------------------------
# (marker, trait, LOD) of every LOD > thr, 1-based like findall(L .> thr): the filter behind plot_eQTL(...; threshold)
function lod_threshold(L::Array{Float64, 2}, thr::Float64; cap::Int64 = max(1024, length(L) ÷ 64))
    (p, m) = size(L)
    while true
        ii = Vector{Int32}(undef, cap); jj = Vector{Int32}(undef, cap); ll = Vector{Float64}(undef, cap)
        cnt = Ref{Int64}(0)
        GC.@preserve L ii jj ll check(ccall((:blmm_lod_threshold, libblmm), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Float64, Int64, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ref{Int64}),
            context(), L, p, m, thr, cap, ii, jj, ll, cnt))
        if cnt[] <= cap
            k = cnt[]
            ord = sortperm(collect(zip(jj[1:k], ii[1:k])))
            return (marker = Int.(ii[1:k][ord]) .+ 1, trait = Int.(jj[1:k][ord]) .+ 1, lod = ll[1:k][ord])
        end
        cap = cnt[]
    end
end
# per-column maximum of an LOD matrix and the (1-based) marker where it sits
function lod_colmax(L::Array{Float64, 2})
    (p, m) = size(L)
    mx = Vector{Float64}(undef, m); arg = Vector{Int64}(undef, m)
    GC.@preserve L mx arg check(ccall((:blmm_lod_colmax, libblmm), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Int64}), context(), L, p, m, mx, arg))
    return (max = mx, argmax = arg .+ 1)
end

# ---- pinned host memory for the outputs: L (2.08 GB at BXD size) then crosses the PCIe link in one asynchronous copy at link rate
# (42 ms against 52 ms into pageable memory).  pinned_matrix wraps blmm_host_alloc memory (released by the finalizer);
# host_register pins the pages of an Array the caller already has.
function pinned_matrix(p::Integer, m::Integer)
    ptr = ccall((:blmm_host_alloc, libblmm), Ptr{Cvoid}, (UInt64,), UInt64(8 * p * m))
    ptr == C_NULL && error("blmm_host_alloc failed")
    A = unsafe_wrap(Array, Ptr{Float64}(ptr), (Int(p), Int(m)); own = false)
    finalizer(_ -> ccall((:blmm_host_free, libblmm), Cvoid, (Ptr{Cvoid},), ptr), A)
    return A
end
host_register(A::Array{Float64}) = (ccall((:blmm_host_register, libblmm), Cint, (Ptr{Cvoid}, UInt64), A, UInt64(sizeof(A))) == 0 || error("hipHostRegister failed"); A)
host_unregister(A::Array{Float64}) = (ccall((:blmm_host_unregister, libblmm), Cint, (Ptr{Cvoid},), A); nothing)

# Readers (src/readData.jl:41-96, 159-165): the numeric table is parsed by the library's host code and copied into a Julia array
check_io(rc) = rc == 0 || error("could not read the file: " * unsafe_string(ccall((:blmm_err_string, libblmm), Cstring, (Cint,), rc)))
function read_table(open_table::Function)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check_io(open_table(h))
    try
        A = Array{Float64, 2}(undef, ccall((:blmm_table_rows, libblmm), Int64, (Ptr{Cvoid},), h[]),
                              ccall((:blmm_table_cols, libblmm), Int64, (Ptr{Cvoid},), h[]))
        check_io(ccall((:blmm_table_copy, libblmm), Cint, (Ptr{Cvoid}, Ptr{Float64}), h[], A))
        return A
    finally
        ccall((:blmm_table_free, libblmm), Cvoid, (Ptr{Cvoid},), h[])
    end
end
read_csv(file, skip, first, step, drop) = read_table(h -> ccall((:blmm_read_csv, libblmm), Cint,
    (Cstring, Int64, Int64, Int64, Int64, Ref{Ptr{Cvoid}}), file, skip, first, step, drop, h))
readGenoProb(file::AbstractString) = read_csv(file, 1, 1, 1, 0)                       # header line and id column dropped (getmarkernames = getids = true)
readGenoProb_ExcludeComplements(file::AbstractString) = read_csv(file, 1, 1, 2, 0)
readBXDpheno(file::AbstractString) = read_csv(file, 1, 1, 1, 1)
readBXDgeno(file::AbstractString; skipstart = 1) = read_csv(file, skipstart, 1, 2, 0)
readhe(file::AbstractString) = read_table(h -> ccall((:blmm_read_he, libblmm), Cint, (Cstring, Ref{Ptr{Cvoid}}), file, h))

# round.(calcKinship(G), digits = d) in one device call (README.md:176-181)
function calcKinship(G::Array{Float64, 2}, digits::Integer)
    n, p = size(G)
    K = Array{Float64, 2}(undef, n, n)
    check(ccall((:blmm_kinship_rounded, libblmm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}),
                context(), G, n, p, digits, K))
    return K
end


# ---- leave-one-chromosome-out: markers ordered by chromosome, `chrom` the label of each (contiguous runs) ----------------------
function chromosome_runs(chrom::AbstractVector, p::Integer)
    length(chrom) == p || error("Dimension mismatch.")
    runs = Any[]; starts = Int64[]
    for i in 1:p
        if i == 1 || chrom[i] != chrom[i - 1]
            chrom[i] in runs && error("chromosome $(chrom[i]) appears again after another chromosome: the markers must be ordered by chromosome (contiguous runs)")
            push!(runs, chrom[i]); push!(starts, i - 1)
        end
    end
    push!(starts, p)
    length(runs) >= 2 || error("leave-one-chromosome-out needs at least 2 chromosomes")
    return runs, starts
end

# calcKinship(G[:, not chromosome c]) for every chromosome c, from one pass over G: n x n x nchr
function calcKinship_loco(G::Array{Float64, 2}, chrom::AbstractVector; digits::Integer = -1)
    n, p = size(G)
    _, cs = chromosome_runs(chrom, p)
    nchr = length(cs) - 1
    K = Array{Float64, 3}(undef, n, n, nchr)
    GC.@preserve G cs K check(ccall((:blmm_kinship_loco, libblmm), Cint,
                                    (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Int64}, Int64, Int64, Ptr{Float64}),
                                    context(), G, n, p, cs, nchr, digits, K))
    return K
end

# rows of chromosome c = bulkscan(Y, G[:, rows_c], calcKinship_loco(G, chrom)[:, :, c]; same options).L
function bulkscan_loco(Y::Array{Float64, 2}, G::Array{Float64, 2}, chrom::AbstractVector;
                       Covar::Union{Nothing, Array{Float64, 2}} = nothing, method::String = "null-grid",
                       h2_grid::Array{Float64, 1} = collect(0.0:0.1:0.9), kinship_digits::Integer = -1,
                       addIntercept::Bool = true, weights::Union{Missing, Array{Float64, 1}} = missing,
                       prior_variance::Float64 = 1.0, prior_sample_size::Float64 = 0.0, reml::Bool = false,
                       optim_interval::Int64 = 1, decomp_scheme::String = "eigen", keep_on_device::Bool = false)
    (n, m) = size(Y); p = size(G, 2)
    size(G, 1) != n && error("Dimension mismatch.")
    runs, cs = chromosome_runs(chrom, p)
    nchr = length(cs) - 1
    check_n(n)
    (Covar !== nothing && size(Covar, 1) != n) && error("Dimension mismatch.")
    (weights !== missing && length(weights) != n) && error("Dimension mismatch.")
    meth = method == "null-exact" ? NULL_EXACT : method == "null-grid" ? NULL_GRID : method == "alt-grid" ? ALT_GRID :
           error("Unknown method `$method`; choose null-exact, null-grid or alt-grid.")
    ncov = Covar === nothing ? 0 : size(Covar, 2)
    o = BlmmOpts(meth, reml, Covar === nothing ? true : addIntercept, decomp(decomp_scheme), optim_interval, 0,
                 prior_variance, prior_sample_size)
    L = keep_on_device ? nothing : Array{Float64, 2}(undef, p, m)
    h2 = meth == ALT_GRID ? Array{Float64, 2}(undef, p, m) : Array{Float64, 2}(undef, m, nchr)   # column c: chromosome c
    st = BlmmStatus()
    GC.@preserve Y G cs Covar weights h2_grid L h2 begin
        check(ccall((:blmm_bulkscan_loco, libblmm), Cint,
                    (Ptr{Cvoid}, Ref{BlmmOpts}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Int64, Int64,
                     Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ref{BlmmStatus}),
                    context(), o, Y, n, m, G, p, cs, nchr, kinship_digits, ptr_or_null(Covar), ncov, ptr_or_null(weights),
                    h2_grid, length(h2_grid), ptr_or_null(L), h2, st))
    end
    raise_status(st)
    Lr = keep_on_device ? DeviceLOD(p, m) : L
    return meth == ALT_GRID ? (L = Lr, h2_panel = h2, chromosomes = runs, chr_start = cs) :
                              (L = Lr, h2_null_list = permutedims(h2), chromosomes = runs, chr_start = cs)
end

# bulkscan_loco WITHOUT the LOD matrix: the genome-wide peak of every trait, its peak on every chromosome (cis / trans table; the
# marker index is genome-wide, 1-based) and, `threshold` given, every (marker, trait, LOD) with LOD > threshold -- bit for bit the
# reductions of bulkscan_loco's L, computed on the device
function bulkscan_loco_reduced(Y::Array{Float64, 2}, G::Array{Float64, 2}, chrom::AbstractVector;
                               Covar::Union{Nothing, Array{Float64, 2}} = nothing, method::String = "null-grid",
                               h2_grid::Array{Float64, 1} = collect(0.0:0.1:0.9), threshold::Union{Nothing, Float64} = nothing,
                               cap::Int64 = 1048576, kinship_digits::Integer = -1, addIntercept::Bool = true,
                               weights::Union{Missing, Array{Float64, 1}} = missing, prior_variance::Float64 = 1.0,
                               prior_sample_size::Float64 = 0.0, reml::Bool = false, optim_interval::Int64 = 1,
                               decomp_scheme::String = "eigen")
    (n, m) = size(Y); p = size(G, 2)
    size(G, 1) != n && error("Dimension mismatch.")
    runs, cs = chromosome_runs(chrom, p)
    nchr = length(cs) - 1
    check_n(n)
    (Covar !== nothing && size(Covar, 1) != n) && error("Dimension mismatch.")
    (weights !== missing && length(weights) != n) && error("Dimension mismatch.")
    cap < 0 && error("bulkscan_loco_reduced: triplet buffers (cap < 0)")
    meth = method == "null-exact" ? NULL_EXACT : method == "null-grid" ? NULL_GRID : method == "alt-grid" ? ALT_GRID :
           error("Unknown method `$method`; choose null-exact, null-grid or alt-grid.")
    ncov = Covar === nothing ? 0 : size(Covar, 2)
    o = BlmmOpts(meth, reml, Covar === nothing ? true : addIntercept, decomp(decomp_scheme), optim_interval, 0,
                 prior_variance, prior_sample_size)
    mx = Vector{Float64}(undef, m); arg = Vector{Int64}(undef, m)
    cmx = Array{Float64, 2}(undef, m, nchr); carg = Array{Int64, 2}(undef, m, nchr); h2 = Array{Float64, 2}(undef, m, nchr)   # column c: chromosome c
    want = threshold !== nothing
    st = BlmmStatus()
    while true
        c1 = max(cap, 1)
        ii = Vector{Int32}(undef, c1); jj = Vector{Int32}(undef, c1); ll = Vector{Float64}(undef, c1); cnt = zeros(Int64, 1)
        GC.@preserve Y G cs Covar weights h2_grid mx arg cmx carg h2 ii jj ll cnt begin
            r = BlmmReduced(pointer(mx), pointer(arg), want ? 1 : 0, want ? threshold : 0.0, want ? cap : 0,
                            pointer(ii), pointer(jj), pointer(ll), pointer(cnt))
            check(ccall((:blmm_bulkscan_loco_reduced, libblmm), Cint,
                        (Ptr{Cvoid}, Ref{BlmmOpts}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Int64, Int64,
                         Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Ref{BlmmReduced}, Ptr{Float64}, Ptr{Int64},
                         Ptr{Float64}, Ref{BlmmStatus}),
                        context(), o, Y, n, m, G, p, cs, nchr, kinship_digits, ptr_or_null(Covar), ncov, ptr_or_null(weights),
                        h2_grid, length(h2_grid), r, cmx, carg, h2, st))
        end
        if !want || cnt[1] <= cap
            raise_status(st)
            res = (max_lod = mx, argmax = arg .+ 1, chr_max_lod = permutedims(cmx), chr_argmax = permutedims(carg) .+ 1,
                   chromosomes = runs, chr_start = cs)
            meth == ALT_GRID || (res = merge(res, (h2_null_list = permutedims(h2),)))
            want || return res
            k = cnt[1]
            ord = sortperm(collect(zip(jj[1:k], ii[1:k])))
            return merge(res, (marker = Int.(ii[1:k][ord]) .+ 1, trait = Int.(jj[1:k][ord]) .+ 1, lod = ll[1:k][ord]))
        end
        cap = cnt[1]
    end
end

# The LOCO permutation test (blmm_bulkscan_loco_perms): bulkscan_perms under every chromosome's LOCO kinship with ONE permutation set
# (rndseed), plus the genome-wide tables -- permutation b's maximum over the chromosomes' copies paired by b.  Rows of the chr_*
# tables are chromosomes in run order; markers are 1-based and global (0 = no comparable LOD).
function bulkscan_loco_perms(Y::Array{Float64, 2}, G::Array{Float64, 2}, chrom::AbstractVector;
                             Covar::Union{Nothing, Array{Float64, 2}} = nothing, nperms::Int64 = 1024, rndseed::Int64 = 0,
                             signif_level::Array{Float64, 1} = [0.10, 0.05], kinship_digits::Integer = -1,
                             weights::Union{Missing, Array{Float64, 1}} = missing, prior_variance::Float64 = 0.0,
                             prior_sample_size::Float64 = 0.0, addIntercept::Bool = true, reml::Bool = false,
                             optim_interval::Int64 = 1, decomp_scheme::String = "eigen", chr_max_perms::Bool = false)
    (n, m) = size(Y); p = size(G, 2)
    size(G, 1) != n && error("Dimension mismatch.")
    runs, cs = chromosome_runs(chrom, p)
    nchr = length(cs) - 1
    check_n(n)
    (Covar !== nothing && size(Covar, 1) != n) && error("Dimension mismatch.")
    (weights !== missing && length(weights) != n) && error("Dimension mismatch.")
    nperms < 0 && error("The required number of permutations must be a positive integer.")
    o = BlmmOpts(NULL_EXACT, reml, Covar === nothing ? true : addIntercept, decomp(decomp_scheme), optim_interval, 0,
                 prior_variance, prior_sample_size)
    probs = 1.0 .- signif_level
    npr = length(probs)
    h2 = Array{Float64, 2}(undef, m, nchr); s2 = similar(h2); cmx = similar(h2); cpv = similar(h2)   # column c: chromosome c
    carg = Array{Int64, 2}(undef, m, nchr)
    cthr = Array{Float64, 3}(undef, npr, m, nchr)
    cmp = chr_max_perms ? Array{Float64, 3}(undef, max(nperms, 1), m, nchr) : nothing
    mx = Vector{Float64}(undef, m); pv = similar(mx); arg = Vector{Int64}(undef, m)
    mp = Array{Float64, 2}(undef, max(nperms, 1), m); thr = Array{Float64, 2}(undef, npr, m)
    st = BlmmStatus()
    ncov = Covar === nothing ? 0 : size(Covar, 2)
    GC.@preserve Y G cs Covar weights probs h2 s2 mx arg mp thr pv cmx carg cmp cthr cpv check(ccall((:blmm_bulkscan_loco_perms, libblmm), Cint,
        (Ptr{Cvoid}, Ref{BlmmOpts}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Int64, Int64, Ptr{Float64}, Int64,
         Ptr{Float64}, Int64, UInt64, Ptr{Int32}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{BlmmStatus}),
        context(), o, Y, n, m, G, p, cs, nchr, kinship_digits, ptr_or_null(Covar), ncov, ptr_or_null(weights), nperms,
        UInt64(rndseed), C_NULL, probs, npr, h2, s2, mx, arg, mp, thr, pv, cmx, carg, ptr_or_null(cmp), cthr, cpv, st))
    raise_status(st)
    res = (h2_null = permutedims(h2), sigma2_e = permutedims(s2), lod_max = mx, lod_argmax = arg .+ 1, max_perms = mp[1:nperms, :],
           thresholds = thr, pvals_perm = pv, chr_lod_max = permutedims(cmx), chr_lod_argmax = permutedims(carg) .+ 1,
           chr_thresholds = permutedims(cthr, (3, 1, 2)), chr_pvals_perm = permutedims(cpv), chromosomes = runs, chr_start = cs)
    chr_max_perms && (res = merge(res, (chr_max_perms = permutedims(cmp, (3, 1, 2))[:, 1:nperms, :],)))
    return res
end

end # module
