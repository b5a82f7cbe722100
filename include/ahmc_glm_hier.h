/*
 * ahmc_glm_hier.h — optional hierarchical form of the generalised-linear-model target (ahmc_glm.h): blocks of coefficients whose
 * prior scale τ is itself a parameter — varying intercepts, varying slopes, a ridge block — evaluated for ALL chains at once
 * by the same two MFMA products.
 *
 *     θ (D), D = n_coef + n_groups:  θ[0:P] coefficient parameters (P = n_coef), θ[P + k] = s_k = log τ_k
 *     group k = the contiguous coefficients [lo_k, hi_k) (0-based), m_k = hi_k − lo_k >= 1, a flag centered_k, a hyper-scale A_k > 0
 *     w_d = θ_d                     coefficients in no group (fixed prior precision p_d) and members of a centred group
 *     w_d = exp(s_k)·θ_d            members of a non-centred group: θ_d is the standardised z_d
 *     η = X·w + offset              X: (n_obs, P) column-major;  (ℓ, u) from the family's link (ahmc_glm.h);  R = −Xᵀu
 *     τ_k ~ half-normal(A_k), with the Jacobian of s = log τ:   h_k = s_k − ½·e^{2s_k}/A_k²,   h′_k = 1 − e^{2s_k}/A_k²
 *     ℓπ(θ) = Σ_i ℓ − ½ Σ_fixed p_d θ_d² + Σ_k h_k + Σ_{k centred} (−m_k·s_k − ½·q_k·S_k) − ½ Σ_{k non-centred} S_k
 *             q_k = e^{−2s_k},  S_k = Σ_{d∈k} θ_d²
 *     g = −∇ℓπ:   fixed d: p_d·θ_d + R_d;   centred member: q_k·θ_d + R_d;   non-centred member: τ_k·R_d + θ_d;
 *                 s_k centred: m_k − q_k·S_k − h′_k;   s_k non-centred: T_k − h′_k,  T_k = Σ_{d∈k} R_d·w_d
 * A non-finite ℓπ (e^{2s} or a Poisson mean overflows) is sanitised to −Inf: a divergence.  The host mirror
 * advancedhmc.jl_amd/glm.py (hier_logdensity) defines the arithmetic, including the order of every sum.
 *
 * A bound hierarchical model has target kind AHMC_TARGET_GLM and is served like the plain one: every metric, integrator, sampler and
 * adaptor, find_good_stepsize, checkpoints, wide contexts.  ahmc_get_target_glm and ahmc_glm_pointwise (at the effective
 * coefficients) work on it.  n_groups = 0 is the plain model: the same chains as ahmc_set_target_glm, bit for bit.
 *
 * Kept apart from ahmc_glm.h and ahmc_hip.h: exported by libahmc_hip.so only; AHMC_ABI_VERSION and AHMC_GLM_VERSION do not change.
 */
#ifndef AHMC_GLM_HIER_H
#define AHMC_GLM_HIER_H

#include "ahmc_glm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AHMC_HGLM_VERSION 1
#define AHMC_HGLM_MAX_GROUPS 32 /* an engine limit: more groups are AHMC_ERR_UNSUPPORTED */

int32_t ahmc_hglm_version(void);

/* Bind the model.  X (n_obs·n_coef), y, offset, prior_prec (n_coef, or NULL: zeros; covers the coefficients in no group) and scale
 * are those of ahmc_set_target_glm, copied at the call; lo, hi, centered (NULL: none is centred) and hyper_scale are host arrays of
 * n_groups entries.  The workspaces of ahmc_set_target_glm grow by 2·n_coef·N elements when n_groups > 0.  Everything that can
 * fail happens before the previous target is touched.
 * AHMC_ERR_ARGUMENT: the context's D != n_coef + n_groups ("DimensionMismatch"); a range that is empty, out of bounds, overlapping
 * or out of order, a non-zero prior_prec on a member ("ArgumentError"); a hyper-scale that is not finite and > 0 ("DomainError");
 * everything ahmc_set_target_glm refuses.  AHMC_ERR_UNSUPPORTED: n_groups > AHMC_HGLM_MAX_GROUPS, n_obs > AHMC_GLM_MAX_OBS. */
int32_t ahmc_hglm_set_target(ahmc_ctx* ctx, int32_t family, int64_t n_obs, int64_t n_coef, const void* X, const void* y, const void* offset,
                             const void* prior_prec, double scale, int32_t n_groups, const int32_t* lo, const int32_t* hi, const int32_t* centered,
                             const double* hyper_scale);

/* The bound model's n_coef, n_groups and group table (arrays of AHMC_HGLM_MAX_GROUPS entries suffice; any output may be NULL).
 * AHMC_ERR_ARGUMENT: no model is bound through ahmc_hglm_set_target. */
int32_t ahmc_hglm_get_target(ahmc_ctx* ctx, int64_t* n_coef, int32_t* n_groups, int32_t* lo, int32_t* hi, int32_t* centered, double* hyper_scale);

/* From draws theta (D, n_cols) column-major of the context's element type, on the host or the device: the coefficients on the
 * model's own scale beta (n_coef, n_cols) = w, and the group scales tau (n_groups, n_cols) = exp(s); either output may be NULL.
 * AHMC_ERR_ARGUMENT: no model is bound through ahmc_hglm_set_target. */
int32_t ahmc_hglm_coefficients(ahmc_ctx* ctx, const void* theta, int64_t n_cols, void* beta_out, void* tau_out);

#ifdef __cplusplus
}
#endif

#endif /* AHMC_GLM_HIER_H */
