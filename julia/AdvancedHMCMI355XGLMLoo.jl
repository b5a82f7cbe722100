# AdvancedHMCMI355XGLMLoo.jl — model comparison for the GLM targets from the kept draws (include/ahmc_glm_loo.h): the pointwise
# log-likelihood at any `(D, n)` array of draws, and PSIS-LOO / WAIC of it (elpd_loo, Pareto k̂, lpd, p_waic per observation).  Included by
# AdvancedHMCMI355XExt.jl after AdvancedHMCMI355XGLMCategorical.jl; the `ccall`s are declared in ahmc_glm_loo.h (exported by
# libahmc_hip.so only).  NOT EXECUTED here (no Julia in the build environment): tests/test_glm_loo.py checks every `ccall` against the
# header.

const GLM_LOO_MAX_VALUES = 2147483647
const GLM_LOO_MAX_TAIL = 4096

glm_loo_version() = ccall((:ahmc_glm_loo_version, LIB), Cint, ())

"`ℓ(y_i, η_i)`, `(n_obs, n)`, of the bound GLM at draws `theta` `(D, n)` (host memory)"
function glm_loglik(z::MI355XChains{T}, theta::AbstractMatrix) where {T}
    _, n_obs, _ = get_target_glm(z)
    th = convert(Matrix{T}, theta)
    size(th, 1) == z.D || throw(DimensionMismatch("θ has $(size(th, 1)) rows, the context D = $(z.D)"))
    out = Matrix{T}(undef, n_obs, size(th, 2))
    check(z.ctx, ccall((:ahmc_glm_loglik, LIB), Cint, (Ptr{Cvoid}, Ptr{T}, Int64, Ptr{T}), z.ctx, th, Int64(size(th, 2)), out))
    return out
end

"""
    glm_loo(z, theta; log_weights=false)

PSIS-LOO and WAIC of the bound GLM over draws `theta` `(D, n)` (host memory): a named tuple of `elpd_loo`, `pareto_k`, `lpd`, `p_waic`
(each of length `n_obs`) and, on request, the normalised `log_weights` `(n, n_obs)` in the draws' order (`nothing` otherwise).
`elpd_waic = lpd .- p_waic` and `p_loo = lpd .- elpd_loo`.
"""
function glm_loo(z::MI355XChains{T}, theta::AbstractMatrix; log_weights::Bool=false) where {T}
    _, n_obs, _ = get_target_glm(z)
    th = convert(Matrix{T}, theta)
    size(th, 1) == z.D || throw(DimensionMismatch("θ has $(size(th, 1)) rows, the context D = $(z.D)"))
    pw = Matrix{Cdouble}(undef, 4, n_obs)
    lw = log_weights ? Matrix{Cdouble}(undef, size(th, 2), n_obs) : nothing
    GC.@preserve lw check(z.ctx, ccall((:ahmc_glm_loo, LIB), Cint, (Ptr{Cvoid}, Ptr{T}, Int64, Ptr{Cdouble}, Ptr{Cdouble}), z.ctx, th, Int64(size(th, 2)), pw,
                                       lw === nothing ? Ptr{Cdouble}(C_NULL) : pointer(lw)))
    return (elpd_loo=pw[1, :], pareto_k=pw[2, :], lpd=pw[3, :], p_waic=pw[4, :], log_weights=lw)
end
