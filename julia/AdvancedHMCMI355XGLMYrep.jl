# AdvancedHMCMI355XGLMYrep.jl — posterior-predictive draws y_rep of the bound GLM (include/ahmc_glm_yrep.h): one outcome per new row and
# draw from the family's counter-based sampler, their per-observation summaries, and the sampler on the caller's own planes.  Included by
# AdvancedHMCMI355XExt.jl after AdvancedHMCMI355XGLMPredict.jl, whose GLMNewData and record it uses; the `ccall`s are declared in
# ahmc_glm_yrep.h (exported by libahmc_hip.so only).  NOT EXECUTED here (no Julia in the build environment): tests/test_glm_yrep.py checks
# every `ccall` against the header.

glm_yrep_version() = ccall((:ahmc_glm_yrep_version, LIB), Cint, ())

"""
    glm_yrep_at(z, family, q; aux=nothing, row=nothing, col=nothing, seed=0, n_categories=0)

`(n,)`: one outcome per element from the sampler of `family` given its planes `q` `(planes, n)`, the log-dispersion `aux` `(n,)` of a
negative binomial and the counters `row`, `col` `(n,)` (`nothing`: `0 … n - 1` and `0`).  No GLM need be bound.
"""
function glm_yrep_at(z::MI355XChains{T}, family::Integer, q::AbstractMatrix; aux=nothing, row=nothing, col=nothing, seed::Integer=0,
                     n_categories::Integer=0) where {T}
    qa = convert(Matrix{T}, q)
    n = size(qa, 2)
    au = aux === nothing ? nothing : convert(Vector{T}, aux)
    ro = row === nothing ? nothing : convert(Vector{Cint}, row)
    co = col === nothing ? nothing : convert(Vector{Cint}, col)
    y = Vector{T}(undef, n)
    GC.@preserve qa au ro co check(z.ctx, ccall((:ahmc_glm_yrep_at, LIB), Cint,
                                                 (Ptr{Cvoid}, Cint, Cint, Int64, Ptr{T}, Ptr{T}, Ptr{Cint}, Ptr{Cint}, UInt64, Ptr{T}), z.ctx, Cint(family),
                                                 Cint(n_categories), Int64(n), qa, au === nothing ? Ptr{T}(C_NULL) : pointer(au),
                                                 ro === nothing ? Ptr{Cint}(C_NULL) : pointer(ro), co === nothing ? Ptr{Cint}(C_NULL) : pointer(co), UInt64(seed), y))
    return y
end

"""
    glm_yrep(z, nd, theta; seed=0)

`(n_new, n)`: y_rep of the bound GLM at the rows of `nd` for the draws `theta` `(D, n)` (host memory); element `(i, j)` depends on its
row, its draw, `(i, j)` and `seed` alone.
"""
function glm_yrep(z::MI355XChains{T}, nd::GLMNewData, theta::AbstractMatrix; seed::Integer=0) where {T}
    th = convert(Matrix{T}, theta)
    size(th, 1) == z.D || throw(DimensionMismatch("θ has $(size(th, 1)) rows, the context D = $(z.D)"))
    rec, keep = glm_newdata_record(T, nd)
    out = Matrix{T}(undef, rec.n_new, size(th, 2))
    GC.@preserve keep check(z.ctx, ccall((:ahmc_glm_yrep, LIB), Cint, (Ptr{Cvoid}, Ref{GLMNewDataRecord}, Ptr{T}, Int64, UInt64, Ptr{T}), z.ctx, Ref(rec), th,
                                         Int64(size(th, 2)), UInt64(seed), out))
    return out
end

"""
    glm_yrep_summary(z, nd, theta; seed=0)

`(4, n_new)` `Float64`: the mean and the variance of every row's y_rep over the draws `theta` `(D, n)` (host memory), and the shares of
them below and at `nd.y` (NaN without it).  The draws are reduced on the device.
"""
function glm_yrep_summary(z::MI355XChains{T}, nd::GLMNewData, theta::AbstractMatrix; seed::Integer=0) where {T}
    th = convert(Matrix{T}, theta)
    size(th, 1) == z.D || throw(DimensionMismatch("θ has $(size(th, 1)) rows, the context D = $(z.D)"))
    rec, keep = glm_newdata_record(T, nd)
    out = fill(NaN, 4, rec.n_new)
    GC.@preserve keep check(z.ctx, ccall((:ahmc_glm_yrep_summary, LIB), Cint, (Ptr{Cvoid}, Ref{GLMNewDataRecord}, Ptr{T}, Int64, UInt64, Ptr{Cdouble}), z.ctx,
                                         Ref(rec), th, Int64(size(th, 2)), UInt64(seed), out))
    return out
end
