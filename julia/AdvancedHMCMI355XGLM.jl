# AdvancedHMCMI355XGLM.jl — a generalised linear model as the engine's target (include/ahmc_glm.h): ℓπ(θ) = Σᵢ ℓ(yᵢ, (Xθ + offset)ᵢ)
# − ½ Σ_d p_d θ_d², evaluated for all chains at once as X·Θ and Xᵀ·U on the MFMA units.  Included by AdvancedHMCMI355XExt.jl; its
# `ccall`s are declared in ahmc_glm.h (exported by libahmc_hip.so only).  NOT EXECUTED here (no Julia in the build environment):
# tests/test_glm_target.py checks every `ccall` against the header.

const GLM_BERNOULLI_LOGIT = Cint(0)
const GLM_POISSON_LOG = Cint(1)
const GLM_GAUSSIAN_IDENTITY = Cint(2)

glm_version() = ccall((:ahmc_glm_version, LIB), Cint, ())

"""
    GLMTarget(X, y; family=GLM_BERNOULLI_LOGIT, prior_prec=nothing, offset=nothing, scale=1.0)

`X` is `(n_obs, D)`; `prior_prec` the `D` precisions of the independent normal prior (`nothing`: flat); `scale = 1/σ²` of the
Gaussian family.
"""
struct GLMTarget{T} <: DeviceTarget
    X::Matrix{T}
    y::Vector{T}
    family::Cint
    prior_prec::Union{Nothing,Vector{T}}
    offset::Union{Nothing,Vector{T}}
    scale::Float64
end
GLMTarget(X::AbstractMatrix{T}, y::AbstractVector; family=GLM_BERNOULLI_LOGIT, prior_prec=nothing, offset=nothing, scale=1.0) where {T} =
    GLMTarget{T}(Matrix{T}(X), Vector{T}(y), Cint(family), prior_prec === nothing ? nothing : Vector{T}(prior_prec),
                 offset === nothing ? nothing : Vector{T}(offset), Float64(scale))

function set_target!(z::MI355XChains{T}, t::GLMTarget) where {T}
    size(t.X, 2) == z.D || throw(DimensionMismatch("X has $(size(t.X, 2)) columns, the context has D = $(z.D)"))
    X = convert(Matrix{T}, t.X)
    y = convert(Vector{T}, t.y)
    off = t.offset === nothing ? nothing : convert(Vector{T}, t.offset)
    p = t.prior_prec === nothing ? nothing : convert(Vector{T}, t.prior_prec)
    GC.@preserve off p check(z.ctx, ccall((:ahmc_set_target_glm, LIB), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Cdouble),
                                          z.ctx, t.family, Int64(size(X, 1)), X, y, off === nothing ? Ptr{T}(C_NULL) : pointer(off),
                                          p === nothing ? Ptr{T}(C_NULL) : pointer(p), t.scale))
    return z
end

"`(family, n_obs, scale)` of the bound model"
function get_target_glm(z::MI355XChains)
    fam = Ref{Cint}(0); n = Ref{Int64}(0); s = Ref{Cdouble}(0)
    check(z.ctx, ccall((:ahmc_get_target_glm, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Int64}, Ref{Cdouble}), z.ctx, fam, n, s))
    return fam[], n[], s[]
end

"""
    glm_pointwise(z::MI355XChains)

`(η, ℓ)` at the chains' current positions, each `(n_obs, N)`: the linear predictor and the pointwise log-likelihood (what a
posterior-predictive check or LOO needs).
"""
function glm_pointwise(z::MI355XChains{T}) where {T}
    _, n, _ = get_target_glm(z)
    η = Matrix{T}(undef, n, z.N)
    ℓ = Matrix{T}(undef, n, z.N)
    check(z.ctx, ccall((:ahmc_glm_pointwise, LIB), Cint, (Ptr{Cvoid}, Ptr{T}, Ptr{T}), z.ctx, η, ℓ))
    return η, ℓ
end
