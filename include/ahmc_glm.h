/*
 * ahmc_glm.h — optional generalised-linear-model target of the HIP engine: a regression posterior whose log-density and gradient
 * are evaluated for ALL chains at once as two matrix products on the MFMA units.
 *
 *     η = X·θ + offset            X: (n_obs, D) column-major, y, offset: (n_obs), prior precision p: (D) >= 0
 *     ℓπ(θ) = Σ_i ℓ(y_i, η_i) − ½ Σ_d p_d θ_d²
 *     −∇ℓπ  = −Xᵀu + p∘θ          u_i = ∂ℓ/∂η_i            (the engine's g)
 *
 * Families (terms that do not depend on θ — log y!, log binomial coefficients, ½ log(scale/2π) — are dropped):
 *     AHMC_GLM_BERNOULLI_LOGIT    ℓ = yη − softplus(η), u = y − σ(η), 0 <= y <= 1;  softplus(η) = max(η, 0) + log1p(exp(−|η|)) and σ
 *                                 from the same exp(−|η|): finite for any finite η
 *     AHMC_GLM_POISSON_LOG        ℓ = yη − exp(η), u = y − exp(η), y >= 0;  an overflowing exp makes ℓπ non-finite, which the engine
 *                                 sanitises to −Inf (a divergence)
 *     AHMC_GLM_GAUSSIAN_IDENTITY  ℓ = −½·scale·(y − η)², u = scale·(y − η);  scale = 1/σ² (ignored by the other families)
 * The host mirror advancedhmc.jl_amd/glm.py defines the arithmetic, including the order of every sum.
 *
 * While a GLM is bound the context's target kind is AHMC_TARGET_GLM and the step-synchronous engine serves it exactly as it serves
 * AHMC_TARGET_KERNEL: every metric and integrator, static HMC and NUTS, find_good_stepsize, ahmc_sample with every adaptor,
 * checkpoints, wide contexts (D > 4096).  ahmc_set_ref_compat is AHMC_ERR_UNSUPPORTED as for every target on that engine;
 * ahmc_lf_pre / ahmc_lf_post and ahmc_ext_* behave as for any target that is not AHMC_TARGET_EXTERNAL.  ahmc_set_target,
 * ahmc_set_target_plugin and ahmc_set_target_kernel replace the GLM and free its buffers.
 *
 * Kept apart from ahmc_hip.h: these entry points are exported by libahmc_hip.so only (the CPU checker under oracle/ does not
 * implement them) and they do not change AHMC_ABI_VERSION.  Conventions (status codes, ahmc_last_error) are ahmc_hip.h's.
 */
#ifndef AHMC_GLM_H
#define AHMC_GLM_H

#include "ahmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AHMC_GLM_VERSION 1
#define AHMC_TARGET_GLM 8 /* the context's target kind while a GLM is bound (ahmc_set_target does not accept it) */
#define AHMC_GLM_MAX_OBS 16777216 /* an engine limit: a larger n_obs is AHMC_ERR_UNSUPPORTED */

enum { AHMC_GLM_BERNOULLI_LOGIT = 0, AHMC_GLM_POISSON_LOG = 1, AHMC_GLM_GAUSSIAN_IDENTITY = 2 };
/* families whose dispersion is sampled: bound through ahmc_glm_aux_set_target (ahmc_glm_aux.h) only */
enum { AHMC_GLM_GAUSSIAN_IDENTITY_SIGMA = 3, AHMC_GLM_NEGBINOMIAL_LOG = 4 };

int32_t ahmc_glm_version(void);

/* Bind the model.  X (n_obs·D, column-major), y (n_obs), offset (n_obs, or NULL: none), prior_prec (D, or NULL: zeros) are of the
 * context's element type, on the host or the device; they are copied at the call, together with a transposed copy of X, and the
 * workspaces (n_obs·N + ⌈n_obs/64⌉·N [+ ⌈n_obs/1024⌉·D·N when n_obs > 1024] elements) are allocated: AHMC_ERR_RUNTIME naming the
 * size if that fails, with the previous target left intact.  Invalidates the current phase point like ahmc_set_target_kernel.
 * AHMC_ERR_ARGUMENT: n_obs < 1, NULL X or y, a non-finite X / offset / prior_prec value ("ArgumentError"), a negative precision or a
 * y outside the family's domain ("DomainError"), scale not finite and > 0, an unknown family. */
int32_t ahmc_set_target_glm(ahmc_ctx* ctx, int32_t family, int64_t n_obs, const void* X, const void* y, const void* offset,
                            const void* prior_prec, double scale);

/* The bound model's family, n_obs and scale (any output may be NULL).  AHMC_ERR_ARGUMENT: no GLM is bound. */
int32_t ahmc_get_target_glm(ahmc_ctx* ctx, int32_t* family, int64_t* n_obs, double* scale);

/* At the context's current θ: the linear predictor η and / or the pointwise log-likelihood ℓ(y_i, η_i), each (n_obs, N)
 * column-major of the context's element type, into host or device buffers; either may be NULL.  What a posterior-predictive check
 * or LOO needs.  A categorical model (ahmc_glm_categorical.h, C classes) has K = C − 1 predictors: eta_out then holds K planes of
 * (n_obs, N), plane k − 1 being η_k, and loglik_out (n_obs, N).  AHMC_ERR_ARGUMENT: no GLM is bound. */
int32_t ahmc_glm_pointwise(ahmc_ctx* ctx, void* eta_out, void* loglik_out);

#ifdef __cplusplus
}
#endif

#endif /* AHMC_GLM_H */
