/*
 * ahmc_glm_categorical.h — optional: the categorical-logit family of the generalised-linear-model target (ahmc_glm.h, ahmc_glm_hier.h,
 * ahmc_glm_factor.h): an outcome in UNORDERED classes y_i ∈ {0, …, C − 1} — multinomial (softmax) regression: brms' categorical(),
 * Stan's categorical_logit, nnet::multinom.
 *
 *     Class 0 is the reference: η_0 ≡ 0.  K = C − 1 coefficient blocks; a block has P_b = P_x + Σ n_levels rows laid out as a
 *     non-categorical model's P rows are (dense rows first, then each factor's levels); the coefficient parameters are P = K·P_b rows,
 *     block k (k = 1 … K, the coefficients of class k) in rows [(k−1)·P_b, k·P_b).
 *     θ (D = P + n_groups): the family adds no rows of its own.  Groups and prior_prec address the P rows as in ahmc_glm_hier.h; a
 *     group must lie inside one block or be a union of whole blocks.
 *     η_k = X·W_k, then the factors' levels of block k in order, then offset[i, k] last (offset: (n_obs, K) column-major or NULL).
 *     Per observation:  m = max(0, η_1, …, η_K);  e_0 = exp(−m), e_k = exp(η_k − m);  s = e_0, then s += e_k for ascending k (one term
 *     is exactly 1: s ∈ [1, C]);  inv = 1/s, lse = m + log(s);  ℓ = η_y − lse;  p_k = e_k·inv;  u_k = ∂ℓ/∂η_k = 1 − p_k if y = k, else −p_k.
 *     Everything is finite for finite η.  ℓπ = Σ_i ℓ + the prior and group terms of ahmc_glm_hier.h on the P rows; the rows of
 *     g = −∇ℓπ of block k come from −Xᵀu_k.  A non-finite ℓπ is sanitised to −Inf like any other.
 * The order of every sum — what makes a chain's bits independent of N, of the chain's column, of the chain list and of the tile
 * shape — is defined with the host mirror, advancedhmc.jl_amd/glm.py (`categorical_logdensity`).  No atomics.
 *
 * A bound model has target kind AHMC_TARGET_GLM and is served like the other GLM targets: ahmc_get_target_glm (family
 * AHMC_GLM_CATEGORICAL_LOGIT), ahmc_hglm_get_target, ahmc_hglm_coefficients, ahmc_glm_factor_get_target (n_coef = P_x and the levels of
 * ONE block), and ahmc_glm_pointwise, for which eta_out then holds K planes of (n_obs, N) — plane k − 1 is η_k — and loglik_out
 * (n_obs, N).  It has no dispersion and no cutpoints: ahmc_glm_aux_get_target, ahmc_glm_dispersion, ahmc_glm_ordinal_get_target and
 * ahmc_glm_cutpoints refuse it.  The set-target entry points of the other headers refuse the family and name this header.
 *
 * Kept apart like ahmc_glm_ordinal.h: exported by libahmc_hip.so only; the versions of the other headers do not change.
 */
#ifndef AHMC_GLM_CATEGORICAL_H
#define AHMC_GLM_CATEGORICAL_H

#include "ahmc_glm_factor.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AHMC_GLM_CATEGORICAL_VERSION 1
#define AHMC_GLM_CATEGORICAL_MAX_CATEGORIES 16

enum { AHMC_GLM_CATEGORICAL_LOGIT = 6 };

int32_t ahmc_glm_categorical_version(void);

/* Bind the model: the arguments of ahmc_glm_ordinal_set_target without cut_prior (n_coef = P_x, the dense columns of X; n_factors may
 * be 0, n_levels and levels then NULL), y holding the class of each observation as an integral value in [0, n_categories).  offset has
 * K·n_obs entries ((n_obs, K) column-major) or is NULL; prior_prec has P = K·P_b entries or is NULL; the context's D must equal
 * P + n_groups.  Workspaces of the model's slab: U is K·n_obs·N elements (K planes of (n_obs, N)), W and R are P·N each, partial
 * ⌈n_obs/64⌉·N and the slice sums ⌈n_obs/1024⌉·P_x·N (n_obs > 1024 only); the slab stays one allocation, and everything that can fail
 * happens before the previous target is touched.
 * AHMC_ERR_ARGUMENT: the context's D != P + n_groups ("DimensionMismatch"); a y that is no integer in [0, C), n_categories < 2
 * ("DomainError"); a group that straddles blocks; everything ahmc_glm_factor_set_target refuses.
 * AHMC_ERR_UNSUPPORTED: n_categories > AHMC_GLM_CATEGORICAL_MAX_CATEGORIES, and the neighbours' limits. */
int32_t ahmc_glm_categorical_set_target(ahmc_ctx* ctx, int64_t n_obs, int64_t n_coef, const void* X, const void* y, const void* offset, const void* prior_prec,
                                        int32_t n_groups, const int32_t* lo, const int32_t* hi, const int32_t* centered, const double* hyper_scale,
                                        int32_t n_factors, const int32_t* n_levels, const int32_t* levels, int32_t n_categories);

/* The bound categorical model's C and the block length P_b (either output may be NULL).  AHMC_ERR_ARGUMENT: no categorical model is
 * bound. */
int32_t ahmc_glm_categorical_get_target(ahmc_ctx* ctx, int32_t* n_categories, int64_t* block_len);

/* out (C, n_obs, n_cols), column-major: the class probabilities p_0 … p_K of every observation at draws theta (D, n_cols); theta and
 * out are host or device pointers, like ahmc_glm_cutpoints'.  The draws are evaluated in chunks of at most N columns on the model's own
 * workspaces.  AHMC_ERR_ARGUMENT: no categorical model is bound; NULL theta or out with n_cols > 0; n_cols < 0. */
int32_t ahmc_glm_class_probs(ahmc_ctx* ctx, const void* theta, int64_t n_cols, void* out);

#ifdef __cplusplus
}
#endif

#endif /* AHMC_GLM_CATEGORICAL_H */
