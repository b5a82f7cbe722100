# AdvancedHMCMI355XGLMHier.jl — a generalised linear model with coefficient groups whose prior scale is sampled
# (include/ahmc_glm_hier.h): θ = (P coefficient parameters, then log τ of each group).  Included by AdvancedHMCMI355XExt.jl after
# AdvancedHMCMI355XGLM.jl; the `ccall`s are declared in ahmc_glm_hier.h (exported by libahmc_hip.so only).  NOT EXECUTED here (no
# Julia in the build environment): tests/test_glm_hier.py checks every `ccall` against the header.

const HGLM_MAX_GROUPS = 32

hglm_version() = ccall((:ahmc_hglm_version, LIB), Cint, ())

"""
    CoefGroup(range; centered=false, scale=1.0)

The coefficients `range` (1-based, contiguous) share a prior scale τ ~ half-normal(`scale`) that is sampled as log τ.  `centered`:
β_d ~ N(0, τ²) is sampled itself; otherwise β_d = τ·z_d with z_d ~ N(0, 1) (non-centred).
"""
struct CoefGroup
    range::UnitRange{Int}
    centered::Bool
    scale::Float64
end
CoefGroup(range::UnitRange; centered=false, scale=1.0) = CoefGroup(range, centered, Float64(scale))

"""
    HierGLMTarget(X, y, groups; family=GLM_BERNOULLI_LOGIT, prior_prec=nothing, offset=nothing, scale=1.0)

`X` is `(n_obs, P)`; the context's `D` must be `P + length(groups)`.  `prior_prec` covers the coefficients in no group and must
be 0 on members.
"""
struct HierGLMTarget{T} <: DeviceTarget
    glm::GLMTarget{T}
    groups::Vector{CoefGroup}
end
HierGLMTarget(X::AbstractMatrix, y::AbstractVector, groups; kw...) = HierGLMTarget(GLMTarget(X, y; kw...), collect(CoefGroup, groups))

function set_target!(z::MI355XChains{T}, h::HierGLMTarget) where {T}
    t = h.glm
    P, G = size(t.X, 2), length(h.groups)
    P + G == z.D || throw(DimensionMismatch("the model has P + G = $P + $G parameters, the context has D = $(z.D)"))
    X = convert(Matrix{T}, t.X)
    y = convert(Vector{T}, t.y)
    off = t.offset === nothing ? nothing : convert(Vector{T}, t.offset)
    p = t.prior_prec === nothing ? nothing : convert(Vector{T}, t.prior_prec)
    lo = Cint[first(g.range) - 1 for g in h.groups]
    hi = Cint[last(g.range) for g in h.groups]
    cen = Cint[g.centered for g in h.groups]
    A = Cdouble[g.scale for g in h.groups]
    GC.@preserve off p check(z.ctx, ccall((:ahmc_hglm_set_target, LIB), Cint,
                                          (Ptr{Cvoid}, Cint, Int64, Int64, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Cdouble, Cint, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}),
                                          z.ctx, t.family, Int64(size(X, 1)), Int64(P), X, y, off === nothing ? Ptr{T}(C_NULL) : pointer(off),
                                          p === nothing ? Ptr{T}(C_NULL) : pointer(p), t.scale, Cint(G), lo, hi, cen, A))
    return z
end

"`(n_coef, groups)` of the bound hierarchical model"
function get_target_hglm(z::MI355XChains)
    P = Ref{Int64}(0); G = Ref{Cint}(0)
    lo = zeros(Cint, HGLM_MAX_GROUPS); hi = zeros(Cint, HGLM_MAX_GROUPS); cen = zeros(Cint, HGLM_MAX_GROUPS); A = zeros(Cdouble, HGLM_MAX_GROUPS)
    check(z.ctx, ccall((:ahmc_hglm_get_target, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}),
                       z.ctx, P, G, lo, hi, cen, A))
    return P[], [CoefGroup(lo[k] + 1:hi[k], cen[k] != 0, A[k]) for k in 1:G[]]
end

"""
    hglm_coefficients(z::MI355XChains, θ::AbstractMatrix)

`(β, τ)` of the draws `θ` `(D, n)`: the coefficients on the model's own scale `(P, n)` and the group scales `(G, n)`.
"""
function hglm_coefficients(z::MI355XChains{T}, θ::AbstractMatrix) where {T}
    P, groups = get_target_hglm(z)
    th = convert(Matrix{T}, θ)
    size(th, 1) == P + length(groups) || throw(DimensionMismatch("θ has $(size(th, 1)) rows, the model P + G = $(P + length(groups))"))
    β = Matrix{T}(undef, P, size(th, 2))
    τ = Matrix{T}(undef, length(groups), size(th, 2))
    check(z.ctx, ccall((:ahmc_hglm_coefficients, LIB), Cint, (Ptr{Cvoid}, Ptr{T}, Int64, Ptr{T}, Ptr{T}), z.ctx, th, Int64(size(th, 2)), β, τ))
    return β, τ
end
