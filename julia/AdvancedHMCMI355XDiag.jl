# AdvancedHMCMI355XDiag.jl — MCMCChains' `summarystats` columns on the device (include/ahmc_diag.h), for draws that
# `ahmc_sample(samples_out = …)` left on the device.  Stands in for `summarystats(bundle_samples(…))` of
# ext/AdvancedHMCMCMCChainsExt.jl without copying the (D, N, K) draws to the host.  Included by AdvancedHMCMI355XExt.jl;
# its `ccall`s are declared in ahmc_diag.h (exported by libahmc_hip.so only).  NOT EXECUTED here (no Julia in the build
# environment): tests/test_diag_summary.py checks every `ccall` against the header.

const DIAG_NAMES = (:mean, :std, :mcse, :ess_bulk, :ess_tail, :rhat, :ess_basic, :rhat_bulk, :rhat_tail)

diag_version() = ccall((:ahmc_diag_version, LIB), Cint, ())

"""
    summarystats_device(z::MI355XChains, draws, K; max_lag=0)

The nine summary columns (mean, std, mcse, ess_bulk, ess_tail, rhat, ess_basic, rhat_bulk, rhat_tail) of every dimension,
pooled over all chains of `z`.  `draws`: the device pointer of the (D, N, K) buffer `ahmc_sample` filled.  Returns a
NamedTuple of length-D `Vector{Float64}`s.
"""
function summarystats_device(z::MI355XChains, draws::Ptr{Cvoid}, K::Integer; max_lag::Integer=0)
    out = Matrix{Float64}(undef, z.D, 9)                     # column s = row s of the C array: out[s*D + d]
    check(z.ctx, ccall((:ahmc_diag_summary, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Float64}),
                       z.ctx, draws, Int64(K), Int64(max_lag), out))
    return NamedTuple{DIAG_NAMES}(Tuple(out[:, s] for s in 1:9))
end

"""
    rank_normalize_device(z::MI355XChains, draws, K, d; folded=false)

z (or the folded z_f) of dimension `d` (1-based): a (N, K) `Matrix{Float64}` (chain × draw), NaN at a dropped middle draw.
"""
function rank_normalize_device(z::MI355XChains, draws::Ptr{Cvoid}, K::Integer, d::Integer; folded::Bool=false)
    out = Matrix{Float64}(undef, z.N, K)
    check(z.ctx, ccall((:ahmc_diag_rank_normalize, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Cint, Ptr{Float64}),
                       z.ctx, draws, Int64(K), Int64(d - 1), Cint(folded), out))
    return out
end
