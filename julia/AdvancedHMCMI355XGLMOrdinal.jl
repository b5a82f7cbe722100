# AdvancedHMCMI355XGLMOrdinal.jl — the ordered-logit family of the GLM target (include/ahmc_glm_ordinal.h): y in ordered categories
# 1:C here (0 … C − 1 in the C ABI), P(y <= k) = σ(c_k − η), no intercept; θ = (the P coefficient parameters, log τ of each group, then κ:
# κ_1 = c_1, κ_j = log(c_j − c_{j−1})).  Included by AdvancedHMCMI355XExt.jl after AdvancedHMCMI355XGLMFactor.jl; the `ccall`s are
# declared in ahmc_glm_ordinal.h (exported by libahmc_hip.so only).  NOT EXECUTED here (no Julia in the build environment):
# tests/test_glm_ordinal.py checks every `ccall` against the header.

const GLM_ORDERED_LOGIT = Cint(5)
const GLM_ORDINAL_MAX_CATEGORIES = 16

glm_ordinal_version() = ccall((:ahmc_glm_ordinal_version, LIB), Cint, ())

"""
    OrdinalGLMTarget(X, y, n_categories; factors=Factor[], groups=CoefGroup[], cut_prior=(0.0, 2.5, 0.0, 1.0), prior_prec=nothing, offset=nothing)

`y[i] ∈ 1:n_categories`.  The context's `D` must be `P + length(groups) + n_categories - 1`; `cut_prior = (loc_1, scale_1, loc_gap,
scale_gap)` is the prior on κ itself.  A constant column in `X` is not identified: the cutpoints take the intercept's place.
"""
struct OrdinalGLMTarget{T} <: DeviceTarget
    X::Matrix{T}
    y::Vector{Int}
    n_categories::Int
    factors::Vector{Factor}
    groups::Vector{CoefGroup}
    cut_prior::NTuple{4,Float64}
    prior_prec::Union{Nothing,Vector{T}}
    offset::Union{Nothing,Vector{T}}
end
function OrdinalGLMTarget(X::AbstractMatrix{T}, y::AbstractVector{<:Integer}, n_categories::Integer; factors=Factor[], groups=CoefGroup[],
                          cut_prior=(0.0, 2.5, 0.0, 1.0), prior_prec=nothing, offset=nothing) where {T}
    2 <= n_categories <= GLM_ORDINAL_MAX_CATEGORIES || throw(DomainError(n_categories, "n_categories must be in 2:$GLM_ORDINAL_MAX_CATEGORIES"))
    all(1 .<= y .<= n_categories) || throw(DomainError(y, "y must hold categories in 1:$n_categories"))
    return OrdinalGLMTarget{T}(Matrix{T}(X), collect(Int, y), Int(n_categories), collect(Factor, factors), collect(CoefGroup, groups),
                               NTuple{4,Float64}(Float64.(cut_prior)), prior_prec === nothing ? nothing : Vector{T}(prior_prec),
                               offset === nothing ? nothing : Vector{T}(offset))
end

function set_target!(z::MI355XChains{T}, t::OrdinalGLMTarget) where {T}
    n, Px, G, F = size(t.X, 1), size(t.X, 2), length(t.groups), length(t.factors)
    P = Px + sum(Int[f.n_levels for f in t.factors])
    P + G + t.n_categories - 1 == z.D ||
        throw(DimensionMismatch("the model has P + G + (C - 1) = $P + $G + $(t.n_categories - 1) parameters, the context has D = $(z.D)"))
    X = convert(Matrix{T}, t.X)
    y = convert(Vector{T}, t.y .- 1)
    off = t.offset === nothing ? nothing : convert(Vector{T}, t.offset)
    p = t.prior_prec === nothing ? nothing : convert(Vector{T}, t.prior_prec)
    lo = Cint[first(g.range) - 1 for g in t.groups]
    hi = Cint[last(g.range) for g in t.groups]
    cen = Cint[g.centered for g in t.groups]
    A = Cdouble[g.scale for g in t.groups]
    nl = Cint[f.n_levels for f in t.factors]
    lev = Matrix{Cint}(undef, n, F)
    for (j, f) in enumerate(t.factors)
        lev[:, j] .= f.index .- 1
    end
    cp = Cdouble[t.cut_prior...]
    GC.@preserve off p check(z.ctx, ccall((:ahmc_glm_ordinal_set_target, LIB), Cint,
                                          (Ptr{Cvoid}, Int64, Int64, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Cint, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble},
                                           Cint, Ptr{Cint}, Ptr{Cint}, Cint, Ptr{Cdouble}),
                                          z.ctx, Int64(n), Int64(Px), X, y, off === nothing ? Ptr{T}(C_NULL) : pointer(off),
                                          p === nothing ? Ptr{T}(C_NULL) : pointer(p), Cint(G), lo, hi, cen, A, Cint(F), nl, lev, Cint(t.n_categories), cp))
    return z
end

"`(n_categories, cut_prior)` of the bound ordinal model"
function get_target_glm_ordinal(z::MI355XChains)
    C = Ref{Cint}(0)
    cp = zeros(Cdouble, 4)
    check(z.ctx, ccall((:ahmc_glm_ordinal_get_target, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}, Ptr{Cdouble}), z.ctx, C, cp))
    return Int(C[]), (cp...,)
end

"the cutpoints `c` `(C - 1, n)` of draws `theta` `(D, n)` (host memory) of the bound ordinal model"
function glm_cutpoints(z::MI355XChains{T}, theta::AbstractMatrix) where {T}
    C, _ = get_target_glm_ordinal(z)
    th = convert(Matrix{T}, theta)
    size(th, 1) == z.D || throw(DimensionMismatch("θ has $(size(th, 1)) rows, the context D = $(z.D)"))
    out = Matrix{T}(undef, C - 1, size(th, 2))
    check(z.ctx, ccall((:ahmc_glm_cutpoints, LIB), Cint, (Ptr{Cvoid}, Ptr{T}, Int64, Ptr{T}), z.ctx, th, Int64(size(th, 2)), out))
    return out
end
