/*
 * ahmc_glm_ordinal.h — optional: the ordered-logit family of the generalised-linear-model target (ahmc_glm.h, ahmc_glm_hier.h,
 * ahmc_glm_factor.h): an outcome in ordered categories y_i ∈ {0, …, C − 1} (brms' cumulative("logit"), Stan's ordered_logistic,
 * MASS::polr), whose C − 1 cutpoints are sampled with the coefficients.
 *
 *     η = X·W (+ the factors' levels) + offset as in the other headers; the model has NO intercept: the cutpoints take its place (a
 *     constant column in X is not refused, but it is not identified).
 *     c_1 < … < c_{C−1},  P(y <= k) = σ(c_{k+1} − η).
 *     θ (D = P + n_groups + C − 1): the P coefficient parameters and the log-scales of the groups as in ahmc_glm_hier.h / ahmc_glm_factor.h,
 *     then LAST the C − 1 rows κ:  κ_1 = c_1,  κ_j = log(c_j − c_{j−1}) for j >= 2 — every θ is a valid model.
 *     c_1 = κ_1;  δ_j = exp(κ_j), c_j = c_{j−1} + δ_j in ascending order.
 *     Prior, on κ itself (no Jacobian term): κ_1 ~ Normal(loc_1, scale_1²), κ_j ~ Normal(loc_gap, scale_gap²) for j >= 2 (a log-normal on
 *     each gap); cut_prior = (loc_1, scale_1, loc_gap, scale_gap).
 *     a = c_{y+1} − η (y < C − 1),  b = c_y − η (y > 0);  softplus(x) = max(x, 0) + log1p(exp(−|x|)), σ from the same exp(−|x|):
 *         y = 0:      ℓ = −softplus(−a)                        da = σ(−a)          db = 0
 *         y = C − 1:  ℓ = −softplus(b)                         da = 0              db = −σ(b)
 *         otherwise:  ℓ = −softplus(−a) − softplus(b) + lg_y   da = σ(−a) + r_y    db = −σ(b) − r_y
 *     with lg_j = log(1 − e^{−δ_j}) and r_j = 1/expm1(δ_j) of the gap between the two cutpoints, made once per (chain, cutpoint):
 *     σ(a) − σ(b) = σ(a)·σ(−b)·(1 − e^{b−a}), so no difference of two sigmoids is formed.  u = ∂ℓ/∂η = −(da + db).
 *     S_k = Σ_{y_i = k−1} da_i + Σ_{y_i = k} db_i,  T_j = Σ_{k >= j} S_k,  ∂ℓ/∂κ_1 = T_1,  ∂ℓ/∂κ_j = δ_j·T_j.
 * A non-finite ℓπ (δ_j overflows at κ_j ≈ 710, or 89 in Float32) is sanitised to −Inf like any other.  The order of every sum — what
 * makes a chain's bits independent of N, of the chain's column, of the chain list and of the tile shape — is defined with the host
 * mirror, advancedhmc.jl_amd/glm.py (`ordinal_logdensity`).  No atomics.
 *
 * A bound model has target kind AHMC_TARGET_GLM and is served like the other GLM targets: ahmc_get_target_glm (family
 * AHMC_GLM_ORDERED_LOGIT), ahmc_glm_pointwise, ahmc_hglm_get_target, ahmc_hglm_coefficients, ahmc_glm_factor_get_target.  It has no
 * dispersion: ahmc_glm_aux_get_target and ahmc_glm_dispersion refuse it.  The set-target entry points of the other headers refuse
 * the family and name this header.
 *
 * Kept apart like ahmc_glm_factor.h: exported by libahmc_hip.so only; the versions of the other headers do not change.
 */
#ifndef AHMC_GLM_ORDINAL_H
#define AHMC_GLM_ORDINAL_H

#include "ahmc_glm_factor.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AHMC_GLM_ORDINAL_VERSION 1
#define AHMC_GLM_ORDINAL_MAX_CATEGORIES 16

enum { AHMC_GLM_ORDERED_LOGIT = 5 };

int32_t ahmc_glm_ordinal_version(void);

/* Bind the model: the arguments of ahmc_glm_factor_set_target without family, scale and dispersion (n_coef = P_x, the dense columns of
 * X; prior_prec has P entries; n_factors may be 0, n_levels and levels then NULL), y holding the category of each observation as an
 * integral value in [0, n_categories), then n_categories = C and cut_prior (4 doubles, host memory).  The model's slab grows by the
 * cutpoint table (3·(C−1)·N) and the cutpoints' row-block sums ((C−1)·⌈n_obs/64⌉·N); it stays one allocation, and everything that can
 * fail happens before the previous target is touched.
 * AHMC_ERR_ARGUMENT: the context's D != P + n_groups + C − 1 ("DimensionMismatch"); a y that is no integer in [0, C), n_categories < 2, a
 * non-finite cut_prior entry or a scale <= 0 ("DomainError"); a NULL cut_prior; everything ahmc_glm_factor_set_target refuses.
 * AHMC_ERR_UNSUPPORTED: n_categories > AHMC_GLM_ORDINAL_MAX_CATEGORIES, and the neighbours' limits. */
int32_t ahmc_glm_ordinal_set_target(ahmc_ctx* ctx, int64_t n_obs, int64_t n_coef, const void* X, const void* y, const void* offset, const void* prior_prec,
                                    int32_t n_groups, const int32_t* lo, const int32_t* hi, const int32_t* centered, const double* hyper_scale,
                                    int32_t n_factors, const int32_t* n_levels, const int32_t* levels, int32_t n_categories, const double* cut_prior);

/* The bound ordinal model's C and its cut_prior (room for 4 doubles; either output may be NULL).  AHMC_ERR_ARGUMENT: no ordinal model
 * is bound. */
int32_t ahmc_glm_ordinal_get_target(ahmc_ctx* ctx, int32_t* n_categories, double* cut_prior);

/* out (C−1, n_cols), column-major: the cutpoints c of draws theta (D, n_cols) — κ is each column's last C − 1 rows; theta and out are
 * host or device pointers, like ahmc_glm_dispersion's.  AHMC_ERR_ARGUMENT: no ordinal model is bound; NULL theta or out with
 * n_cols > 0; n_cols < 0. */
int32_t ahmc_glm_cutpoints(ahmc_ctx* ctx, const void* theta, int64_t n_cols, void* out);

#ifdef __cplusplus
}
#endif

#endif /* AHMC_GLM_ORDINAL_H */
