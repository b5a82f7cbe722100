# AdvancedHMCMI355XGLMFactor.jl — index-coded factors of the GLM target (include/ahmc_glm_factor.h): a factor with L levels stands for
# L one-hot columns of X without storing or multiplying them; θ = (the P_x dense coefficients, the levels of factor 1, of factor 2, …,
# log τ of each group, then s for a family with a sampled dispersion).  Included by AdvancedHMCMI355XExt.jl after
# AdvancedHMCMI355XGLMAux.jl; the `ccall`s are declared in ahmc_glm_factor.h (exported by libahmc_hip.so only).  NOT EXECUTED here (no
# Julia in the build environment): tests/test_glm_factor.py checks every `ccall` against the header.

const GLM_FACTOR_MAX = 8

glm_factor_version() = ccall((:ahmc_glm_factor_version, LIB), Cint, ())

"""
    Factor(index; n_levels=maximum(index))

`index[i] ∈ 1:n_levels` is the level of observation `i` (1-based here; the C ABI takes zero-based indices).
"""
struct Factor
    index::Vector{Int}
    n_levels::Int
end
Factor(index::AbstractVector{<:Integer}; n_levels=maximum(index)) = Factor(collect(Int, index), Int(n_levels))

"the 1-based coefficient rows of each factor in a model with `P_x` dense columns"
function factor_ranges(P_x::Integer, factors)
    out = UnitRange{Int}[]
    lo = Int(P_x)
    for f in factors
        push!(out, lo + 1:lo + f.n_levels)
        lo += f.n_levels
    end
    return out
end

"""
    FactorGLMTarget(X, y, factors; family=GLM_BERNOULLI_LOGIT, groups=CoefGroup[], aux_prior=nothing, prior_prec=nothing, offset=nothing, scale=1.0)

`X` is `(n_obs, P_x)` and keeps the dense columns only; the model has `P = P_x + sum(f.n_levels for f in factors)` coefficient
parameters, which `groups`, `prior_prec` (length `P`) and `hglm_coefficients` address like columns of `X`.  The context's `D` must be
`P + length(groups)`, plus 1 for a family with a sampled dispersion (`aux_prior = (loc, scale)`).
"""
struct FactorGLMTarget{T} <: DeviceTarget
    glm::GLMTarget{T}
    factors::Vector{Factor}
    groups::Vector{CoefGroup}
    aux_prior::Union{Nothing,Tuple{Float64,Float64}}
end
function FactorGLMTarget(X::AbstractMatrix, y::AbstractVector, factors; groups=CoefGroup[], aux_prior=nothing, kw...)
    ap = aux_prior === nothing ? nothing : (Float64(aux_prior[1]), Float64(aux_prior[2]))
    return FactorGLMTarget(GLMTarget(X, y; kw...), collect(Factor, factors), collect(CoefGroup, groups), ap)
end

function set_target!(z::MI355XChains{T}, h::FactorGLMTarget) where {T}
    t = h.glm
    n, Px, G, F = size(t.X, 1), size(t.X, 2), length(h.groups), length(h.factors)
    F <= GLM_FACTOR_MAX || throw(ArgumentError("$F factors; at most $GLM_FACTOR_MAX"))
    P = Px + sum(Int[f.n_levels for f in h.factors])
    has_aux = h.aux_prior !== nothing
    P + G + has_aux == z.D || throw(DimensionMismatch("the model has P + G = $P + $G parameters$(has_aux ? " and the dispersion's row" : ""), the context has D = $(z.D)"))
    all(length(f.index) == n for f in h.factors) || throw(DimensionMismatch("a factor's index has one level per observation (n_obs = $n)"))
    X = convert(Matrix{T}, t.X)
    y = convert(Vector{T}, t.y)
    off = t.offset === nothing ? nothing : convert(Vector{T}, t.offset)
    p = t.prior_prec === nothing ? nothing : convert(Vector{T}, t.prior_prec)
    lo = Cint[first(g.range) - 1 for g in h.groups]
    hi = Cint[last(g.range) for g in h.groups]
    cen = Cint[g.centered for g in h.groups]
    A = Cdouble[g.scale for g in h.groups]
    nl = Cint[f.n_levels for f in h.factors]
    lev = Matrix{Cint}(undef, n, F)
    for (j, f) in enumerate(h.factors)
        lev[:, j] .= f.index .- 1
    end
    loc, sc = has_aux ? h.aux_prior : (0.0, 1.0)
    GC.@preserve off p check(z.ctx, ccall((:ahmc_glm_factor_set_target, LIB), Cint,
                                          (Ptr{Cvoid}, Cint, Int64, Int64, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Cdouble, Cint, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble},
                                           Cint, Ptr{Cint}, Ptr{Cint}, Cint, Cdouble, Cdouble),
                                          z.ctx, t.family, Int64(n), Int64(Px), X, y, off === nothing ? Ptr{T}(C_NULL) : pointer(off),
                                          p === nothing ? Ptr{T}(C_NULL) : pointer(p), t.scale, Cint(G), lo, hi, cen, A, Cint(F), nl, lev, Cint(has_aux), loc, sc))
    return z
end

"`(P_x, n_levels)` of the bound GLM: its dense columns and the levels of each factor (none for a model bound without factors)"
function get_target_glm_factor(z::MI355XChains)
    Px = Ref{Int64}(0); F = Ref{Cint}(0)
    nl = zeros(Cint, GLM_FACTOR_MAX)
    check(z.ctx, ccall((:ahmc_glm_factor_get_target, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Cint}, Ptr{Cint}), z.ctx, Px, F, nl))
    return Px[], Int[nl[f] for f in 1:F[]]
end
