# AdvancedHMCMI355XRankUpdate.jl — RankUpdateEuclideanMetric (src/metric.jl:179-245) on the engine: one M⁻¹ = A + B·D·Bᵀ shared by
# all chains (include/ahmc_rank_update.h; the reference's metric is single-chain, sharing it is this engine's extension as for
# DenseEuclideanMetric).  Included by AdvancedHMCMI355XExt.jl; its `ccall`s are declared in ahmc_rank_update.h (exported by
# libahmc_hip.so only).  NOT EXECUTED here (no Julia in the build environment): tests/test_rank_update_metric.py checks every
# `ccall` against the header.

rank_update_version() = ccall((:ahmc_rank_update_version, LIB), Cint, ())

function set_metric!(z::MI355XChains{T}, m::AdvancedHMC.RankUpdateEuclideanMetric) where {T}
    A = convert(Vector{T}, m.A.diag)
    B = convert(Matrix{T}, m.B)
    Dm = convert(Matrix{T}, m.D)
    check(z.ctx, ccall((:ahmc_set_metric_rank_update, LIB), Cint, (Ptr{Cvoid}, Ptr{T}, Ptr{T}, Ptr{T}, Int64),
                       z.ctx, A, B, Dm, Int64(size(B, 2))))
    return z
end

"""
    get_metric_rank_update(z::MI355XChains)

`(A, B, D)` of the context's RankUpdateEuclideanMetric: `RankUpdateEuclideanMetric(Diagonal(A), B, D)` rebuilds it.
"""
function get_metric_rank_update(z::MI355XChains{T}) where {T}
    k = Ref{Int64}(0)
    check(z.ctx, ccall((:ahmc_get_metric_rank_update, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int64}),
                       z.ctx, C_NULL, C_NULL, C_NULL, k))
    A = Vector{T}(undef, z.D)
    B = Matrix{T}(undef, z.D, k[])
    Dm = Matrix{T}(undef, k[], k[])
    check(z.ctx, ccall((:ahmc_get_metric_rank_update, LIB), Cint, (Ptr{Cvoid}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{Int64}),
                       z.ctx, A, B, Dm, k))
    return A, B, Dm
end
