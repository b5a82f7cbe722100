# AdvancedHMCMI355XGLMPredict.jl — predictions of the bound GLM at new rows of data (include/ahmc_glm_predict.h): the linear predictor,
# the mean and variance of the outcome or the category / class probabilities, the log-likelihood at held-out outcomes, at any `(D, n)`
# array of draws, and their per-observation summaries over the draws with the held-out lpd.  Included by AdvancedHMCMI355XExt.jl after
# AdvancedHMCMI355XGLMLoo.jl; the `ccall`s are declared in ahmc_glm_predict.h (exported by libahmc_hip.so only).  NOT EXECUTED here (no
# Julia in the build environment): tests/test_glm_predict.py checks every `ccall` against the header.

const GLM_PRED_LINEAR = Cint(0)
const GLM_PRED_MEAN = Cint(1)
const GLM_PRED_VARIANCE = Cint(2)
const GLM_PRED_LOGLIK = Cint(3)

glm_predict_version() = ccall((:ahmc_glm_predict_version, LIB), Cint, ())

"struct ahmc_glm_newdata"
struct GLMNewDataRecord
    n_new::Int64
    X::Ptr{Cvoid}
    levels::Ptr{Cint}
    offset::Ptr{Cvoid}
    y::Ptr{Cvoid}
end

"""
    GLMNewData(X; levels=nothing, offset=nothing, y=nothing)

New rows for the bound GLM: `X` `(n_new, P_x)`; `levels` `(n_new, F)` zero-based level indices of the model's factors; `offset`
`(n_new,)` — `(n_new, C - 1)` for a categorical model; `y` `(n_new,)`, the held-out outcomes.
"""
struct GLMNewData
    X::Matrix
    levels::Union{Nothing,Matrix{Cint}}
    offset::Union{Nothing,VecOrMat}
    y::Union{Nothing,Vector}
end
GLMNewData(X::AbstractMatrix; levels=nothing, offset=nothing, y=nothing) =
    GLMNewData(Matrix(X), levels === nothing ? nothing : convert(Matrix{Cint}, levels), offset === nothing ? nothing : collect(offset),
               y === nothing ? nothing : collect(y))

# (K predictors, C categories or classes — 0 for the families with one mean) of the bound model
function glm_predict_quantities(z::MI355XChains)
    family, _, _ = get_target_glm(z)
    family == GLM_CATEGORICAL_LOGIT && return (get_target_glm_categorical(z)[1] - 1, get_target_glm_categorical(z)[1])
    family == GLM_ORDERED_LOGIT && return (1, get_target_glm_ordinal(z)[1])
    return (1, 0)
end

# the record of `nd` in the context's element type and the arrays it points into (keep them alive across the call)
function glm_newdata_record(::Type{T}, nd::GLMNewData) where {T}
    X = convert(Matrix{T}, nd.X)
    off = nd.offset === nothing ? nothing : convert(Array{T}, nd.offset)
    y = nd.y === nothing ? nothing : convert(Vector{T}, nd.y)
    rec = GLMNewDataRecord(Int64(size(X, 1)), pointer(X), nd.levels === nothing ? Ptr{Cint}(C_NULL) : pointer(nd.levels),
                           off === nothing ? C_NULL : pointer(off), y === nothing ? C_NULL : pointer(y))
    return rec, (X, nd.levels, off, y)
end

"""
    glm_predict(z, nd, theta; what=GLM_PRED_MEAN)

`(planes, n_new, n)`: the planes `what` names of the bound GLM at the rows of `nd` and draws `theta` `(D, n)` (host memory).
"""
function glm_predict(z::MI355XChains{T}, nd::GLMNewData, theta::AbstractMatrix; what::Cint=GLM_PRED_MEAN) where {T}
    K, C = glm_predict_quantities(z)
    planes = what == GLM_PRED_LINEAR ? K : what == GLM_PRED_MEAN ? max(C, 1) : 1
    th = convert(Matrix{T}, theta)
    size(th, 1) == z.D || throw(DimensionMismatch("θ has $(size(th, 1)) rows, the context D = $(z.D)"))
    rec, keep = glm_newdata_record(T, nd)
    out = Array{T,3}(undef, planes, rec.n_new, size(th, 2))
    GC.@preserve keep check(z.ctx, ccall((:ahmc_glm_predict, LIB), Cint, (Ptr{Cvoid}, Ref{GLMNewDataRecord}, Ptr{T}, Int64, Cint, Ptr{T}), z.ctx, Ref(rec), th,
                                         Int64(size(th, 2)), what, out))
    return out
end

"""
    glm_predict_summary(z, nd, theta)

`(2Q + 1, n_new)` `Float64`: rows `2q - 1`, `2q` (one-based) the mean and the variance over the draws `theta` `(D, n)` (host memory) of
quantity `q` of the header, the last row the log predictive density at `nd.y` (NaN without it).  The draws are reduced on the device.
"""
function glm_predict_summary(z::MI355XChains{T}, nd::GLMNewData, theta::AbstractMatrix) where {T}
    K, C = glm_predict_quantities(z)
    Q = K + (C == 0 ? 2 : C)
    th = convert(Matrix{T}, theta)
    size(th, 1) == z.D || throw(DimensionMismatch("θ has $(size(th, 1)) rows, the context D = $(z.D)"))
    rec, keep = glm_newdata_record(T, nd)
    out = fill(NaN, 2Q + 1, rec.n_new)
    GC.@preserve keep check(z.ctx, ccall((:ahmc_glm_predict_summary, LIB), Cint, (Ptr{Cvoid}, Ref{GLMNewDataRecord}, Ptr{T}, Int64, Ptr{Cdouble}), z.ctx, Ref(rec),
                                         th, Int64(size(th, 2)), out))
    return out
end
