# AdvancedHMCMI355XLowRankAdapt.jl — the mass-matrix adaptor of RankUpdateEuclideanMetric on the engine (include/ahmc_lowrank_adapt.h):
# M⁻¹ = A + B·D·Bᵀ of rank k, one for all chains, fitted to the draws of all of them.  The reference has no adaptor for this metric,
# so the type is this package's.  Included by AdvancedHMCMI355XExt.jl; its `ccall`s are declared in ahmc_lowrank_adapt.h (exported by
# libahmc_hip.so only).  NOT EXECUTED here (no Julia in the build environment): tests/test_lowrank_adaptation.py checks every `ccall`
# against the header.

lowrank_adapt_version() = ccall((:ahmc_lowrank_adapt_version, LIB), Cint, ())

"""
    LowRankVar(rank; oversample = 8, seed = 0)

The estimator behind `lowrank_adaptor_init!`: rank of `B`, oversampling of the test matrix, key of its normals.
"""
struct LowRankVar
    rank::Int
    oversample::Int
    seed::UInt64
end
LowRankVar(rank::Integer; oversample::Integer = 8, seed::Integer = 0) = LowRankVar(Int(rank), Int(oversample), UInt64(seed))

# mirror of ahmc_lowrank_state
mutable struct LowRankHeader
    k::Int64
    ell::Int64
    seed::UInt64
    n::Int64
    n_fits::Int64
end
LowRankHeader() = LowRankHeader(0, 0, 0, 0, 0)

"""
    lowrank_adaptor_init!(z, kind, pc::LowRankVar; δ = 0.8, init_buffer = 75, term_buffer = 50, window_size = 25)

`kind`: 2 (MassMatrixAdaptor), 3 (NaiveHMCAdaptor) or 4 (StanHMCAdaptor), the AHMC_ADAPT_* codes.  The context's metric becomes a
rank-`pc.rank` RankUpdateEuclideanMetric; `adapt!` / `sample` then run the estimator.
"""
function lowrank_adaptor_init!(z::MI355XChains, kind::Integer, pc::LowRankVar; δ::Real = 0.8, init_buffer::Integer = 75,
                               term_buffer::Integer = 50, window_size::Integer = 25)
    check(z.ctx, ccall((:ahmc_lowrank_adaptor_init, LIB), Cint, (Ptr{Cvoid}, Cint, Cdouble, Cint, Cint, Cint, Int64, Int64, UInt64),
                       z.ctx, Cint(kind), Cdouble(δ), Cint(init_buffer), Cint(term_buffer), Cint(window_size), Int64(pc.rank),
                       Int64(pc.oversample), pc.seed))
    return z
end

"""
    lowrank_get_state(z) -> (header, μ, m2, Z, s₀, Ω)
"""
function lowrank_get_state(z::MI355XChains)
    h = Ref(LowRankHeader())
    check(z.ctx, ccall((:ahmc_lowrank_get_state, LIB), Cint, (Ptr{Cvoid}, Ref{LowRankHeader}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                       z.ctx, h, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL))
    L = Int(h[].ell)
    μ, m2, s0 = Vector{Float64}(undef, z.D), Vector{Float64}(undef, z.D), Vector{Float64}(undef, z.D)
    Z, Ω = Matrix{Float64}(undef, z.D, L), Matrix{Float64}(undef, z.D, L)
    check(z.ctx, ccall((:ahmc_lowrank_get_state, LIB), Cint, (Ptr{Cvoid}, Ref{LowRankHeader}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                       z.ctx, h, μ, m2, Z, s0, Ω))
    return h[], μ, m2, Z, s0, Ω
end

function lowrank_set_state!(z::MI355XChains, h::LowRankHeader, μ::Vector{Float64}, m2::Vector{Float64}, Z::Matrix{Float64},
                            s0::Vector{Float64}, Ω::Matrix{Float64})
    check(z.ctx, ccall((:ahmc_lowrank_set_state, LIB), Cint, (Ptr{Cvoid}, Ref{LowRankHeader}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                       z.ctx, Ref(h), μ, m2, Z, s0, Ω))
    return z
end
