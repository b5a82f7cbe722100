# AdvancedHMCMI355XGLMCategorical.jl — the categorical-logit family of the GLM target (include/ahmc_glm_categorical.h): y in unordered
# classes 1:C here (0 … C − 1 in the C ABI), class 1 the reference; K = C − 1 coefficient blocks of P_b = P_x + Σ n_levels rows,
# θ = (the K·P_b coefficient parameters, log τ of each group).  Included by AdvancedHMCMI355XExt.jl after AdvancedHMCMI355XGLMOrdinal.jl;
# the `ccall`s are declared in ahmc_glm_categorical.h (exported by libahmc_hip.so only).  NOT EXECUTED here (no Julia in the build
# environment): tests/test_glm_categorical.py checks every `ccall` against the header.

const GLM_CATEGORICAL_LOGIT = Cint(6)
const GLM_CATEGORICAL_MAX_CATEGORIES = 16

glm_categorical_version() = ccall((:ahmc_glm_categorical_version, LIB), Cint, ())

"""
    CategoricalGLMTarget(X, y, n_categories; factors=Factor[], groups=CoefGroup[], prior_prec=nothing, offset=nothing)

`y[i] ∈ 1:n_categories`, unordered; class 1 is the reference.  The context's `D` must be `(n_categories - 1) * P_b + length(groups)`
with `P_b = size(X, 2) + sum(n_levels)`; rows `(k - 2) * P_b + 1 : (k - 1) * P_b` are the coefficients of class `k >= 2`.  `offset` is
`n × (n_categories - 1)`; `prior_prec` has `(n_categories - 1) * P_b` entries.  A group lies inside one block or covers whole blocks.
"""
struct CategoricalGLMTarget{T} <: DeviceTarget
    X::Matrix{T}
    y::Vector{Int}
    n_categories::Int
    factors::Vector{Factor}
    groups::Vector{CoefGroup}
    prior_prec::Union{Nothing,Vector{T}}
    offset::Union{Nothing,Matrix{T}}
end
function CategoricalGLMTarget(X::AbstractMatrix{T}, y::AbstractVector{<:Integer}, n_categories::Integer; factors=Factor[], groups=CoefGroup[],
                              prior_prec=nothing, offset=nothing) where {T}
    2 <= n_categories <= GLM_CATEGORICAL_MAX_CATEGORIES || throw(DomainError(n_categories, "n_categories must be in 2:$GLM_CATEGORICAL_MAX_CATEGORIES"))
    all(1 .<= y .<= n_categories) || throw(DomainError(y, "y must hold classes in 1:$n_categories"))
    offset === nothing || size(offset) == (size(X, 1), n_categories - 1) ||
        throw(DimensionMismatch("offset is $(size(offset)), expected ($(size(X, 1)), $(n_categories - 1))"))
    return CategoricalGLMTarget{T}(Matrix{T}(X), collect(Int, y), Int(n_categories), collect(Factor, factors), collect(CoefGroup, groups),
                                   prior_prec === nothing ? nothing : Vector{T}(prior_prec), offset === nothing ? nothing : Matrix{T}(offset))
end

function set_target!(z::MI355XChains{T}, t::CategoricalGLMTarget) where {T}
    n, Px, G, F = size(t.X, 1), size(t.X, 2), length(t.groups), length(t.factors)
    K = t.n_categories - 1
    Pb = Px + sum(Int[f.n_levels for f in t.factors])
    K * Pb + G == z.D || throw(DimensionMismatch("the model has (C - 1) * P_b + G = $K * $Pb + $G parameters, the context has D = $(z.D)"))
    X = convert(Matrix{T}, t.X)
    y = convert(Vector{T}, t.y .- 1)
    off = t.offset === nothing ? nothing : convert(Matrix{T}, t.offset)
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
    GC.@preserve off p check(z.ctx, ccall((:ahmc_glm_categorical_set_target, LIB), Cint,
                                          (Ptr{Cvoid}, Int64, Int64, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Cint, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble},
                                           Cint, Ptr{Cint}, Ptr{Cint}, Cint),
                                          z.ctx, Int64(n), Int64(Px), X, y, off === nothing ? Ptr{T}(C_NULL) : pointer(off),
                                          p === nothing ? Ptr{T}(C_NULL) : pointer(p), Cint(G), lo, hi, cen, A, Cint(F), nl, lev, Cint(t.n_categories)))
    return z
end

"`(n_categories, P_b)` of the bound categorical model"
function get_target_glm_categorical(z::MI355XChains)
    C = Ref{Cint}(0)
    Pb = Ref{Int64}(0)
    check(z.ctx, ccall((:ahmc_glm_categorical_get_target, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Int64}), z.ctx, C, Pb))
    return Int(C[]), Int(Pb[])
end

"the class probabilities `(C, n_obs, n)` of every observation at draws `theta` `(D, n)` (host memory) of the bound categorical model"
function glm_class_probs(z::MI355XChains{T}, theta::AbstractMatrix, n_obs::Integer) where {T}
    C, _ = get_target_glm_categorical(z)
    th = convert(Matrix{T}, theta)
    size(th, 1) == z.D || throw(DimensionMismatch("θ has $(size(th, 1)) rows, the context D = $(z.D)"))
    out = Array{T,3}(undef, C, n_obs, size(th, 2))
    check(z.ctx, ccall((:ahmc_glm_class_probs, LIB), Cint, (Ptr{Cvoid}, Ptr{T}, Int64, Ptr{T}), z.ctx, th, Int64(size(th, 2)), out))
    return out
end
