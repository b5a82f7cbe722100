# AdvancedHMCMI355XGLMAux.jl — GLM families whose dispersion is sampled (include/ahmc_glm_aux.h): a Gaussian with unknown σ and the
# negative binomial; θ = (P coefficient parameters, log τ of each group, then s = log σ or log φ).  Included by
# AdvancedHMCMI355XExt.jl after AdvancedHMCMI355XGLMHier.jl; the `ccall`s are declared in ahmc_glm_aux.h (exported by libahmc_hip.so
# only).  NOT EXECUTED here (no Julia in the build environment): tests/test_glm_aux.py checks every `ccall` against the header.

const GLM_GAUSSIAN_IDENTITY_SIGMA = Cint(3)
const GLM_NEGBINOMIAL_LOG = Cint(4)
const GLM_AUX_MAX_GROUPS = 31

glm_aux_version() = ccall((:ahmc_glm_aux_version, LIB), Cint, ())

"""
    AuxGLMTarget(X, y; family=GLM_NEGBINOMIAL_LOG, groups=CoefGroup[], aux_prior=(0.0, 1.0), prior_prec=nothing, offset=nothing)

`X` is `(n_obs, P)`; the context's `D` must be `P + length(groups) + 1`: the last row of θ is `s`, the log of σ
(`GLM_GAUSSIAN_IDENTITY_SIGMA`) or of φ (`GLM_NEGBINOMIAL_LOG`), with the prior `s ~ Normal(aux_prior...)`.
"""
struct AuxGLMTarget{T} <: DeviceTarget
    glm::GLMTarget{T}
    groups::Vector{CoefGroup}
    aux_loc::Float64
    aux_scale::Float64
end
function AuxGLMTarget(X::AbstractMatrix, y::AbstractVector; family=GLM_NEGBINOMIAL_LOG, groups=CoefGroup[], aux_prior=(0.0, 1.0), kw...)
    return AuxGLMTarget(GLMTarget(X, y; family=family, kw...), collect(CoefGroup, groups), Float64(aux_prior[1]), Float64(aux_prior[2]))
end

function set_target!(z::MI355XChains{T}, h::AuxGLMTarget) where {T}
    t = h.glm
    P, G = size(t.X, 2), length(h.groups)
    P + G + 1 == z.D || throw(DimensionMismatch("the model has P + G + 1 = $P + $G + 1 parameters, the context has D = $(z.D)"))
    X = convert(Matrix{T}, t.X)
    y = convert(Vector{T}, t.y)
    off = t.offset === nothing ? nothing : convert(Vector{T}, t.offset)
    p = t.prior_prec === nothing ? nothing : convert(Vector{T}, t.prior_prec)
    lo = Cint[first(g.range) - 1 for g in h.groups]
    hi = Cint[last(g.range) for g in h.groups]
    cen = Cint[g.centered for g in h.groups]
    A = Cdouble[g.scale for g in h.groups]
    GC.@preserve off p check(z.ctx, ccall((:ahmc_glm_aux_set_target, LIB), Cint,
                                          (Ptr{Cvoid}, Cint, Int64, Int64, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Cint, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Cdouble, Cdouble),
                                          z.ctx, t.family, Int64(size(X, 1)), Int64(P), X, y, off === nothing ? Ptr{T}(C_NULL) : pointer(off),
                                          p === nothing ? Ptr{T}(C_NULL) : pointer(p), Cint(G), lo, hi, cen, A, h.aux_loc, h.aux_scale))
    return z
end

"`(aux_loc, aux_scale)` of the bound model's prior on s"
function get_target_glm_aux(z::MI355XChains)
    m = Ref{Cdouble}(0); a = Ref{Cdouble}(0)
    check(z.ctx, ccall((:ahmc_glm_aux_get_target, LIB), Cint, (Ptr{Cvoid}, Ref{Cdouble}, Ref{Cdouble}), z.ctx, m, a))
    return m[], a[]
end

"""
    glm_dispersion(z::MI355XChains, θ::AbstractMatrix)

σ or φ = exp(s) of every draw (column) of `θ` `(D, n)`.
"""
function glm_dispersion(z::MI355XChains{T}, θ::AbstractMatrix) where {T}
    th = convert(Matrix{T}, θ)
    size(th, 1) == z.D || throw(DimensionMismatch("θ has $(size(th, 1)) rows, the context D = $(z.D)"))
    out = Vector{T}(undef, size(th, 2))
    check(z.ctx, ccall((:ahmc_glm_dispersion, LIB), Cint, (Ptr{Cvoid}, Ptr{T}, Int64, Ptr{T}), z.ctx, th, Int64(size(th, 2)), out))
    return out
end
