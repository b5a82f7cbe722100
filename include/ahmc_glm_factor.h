/*
 * ahmc_glm_factor.h — optional: index-coded factors for the generalised-linear-model target (ahmc_glm.h, ahmc_glm_hier.h,
 * ahmc_glm_aux.h).  A factor f has n_levels[f] levels and one zero-based level index per observation; it stands for n_levels[f]
 * one-hot columns of X without storing or multiplying them.
 *
 *     X (n_obs, n_coef) keeps the dense columns only: P_x = n_coef >= 1.
 *     The model's coefficient parameters are P = P_x + Σ_f n_levels[f] rows: the dense coefficients first, then factor 0's levels,
 *     factor 1's levels, …  Group ranges (lo, hi), prior_prec (P entries), ahmc_hglm_coefficients and the rows after them (the
 *     log-scales of the groups, the dispersion's row) address these P rows exactly as they address the columns of X without factors.
 *     The context's D = P + n_groups + (has_aux ? 1 : 0).
 *
 *     η_i = [the k-ordered fma chain over the P_x dense columns] + W[off_0 + idx_0[i]] + W[off_1 + idx_1[i]] + … + offset_i
 *     R_d, d < P_x: from Xᵀu as without factors.  Row off_f + l of R: observations in slices of 1024; within a slice u summed over the
 *     observations with idx_f[i] = l in ascending i from +0; the slice sums added in ascending order; R is the negative of the result.
 * These are the numbers the other entry points compute for the same model with the factors written as one-hot columns appended to X
 * (fma(0, w, a) = a, fma(1, u, a) = a + u), up to the sign of a zero, whenever W is finite.  No atomics: a chain's bits do not depend
 * on N, on the chain's column, on the chain list or on the tile shape.  The host mirror advancedhmc.jl_amd/glm.py (`factors=`)
 * defines the arithmetic.
 *
 * A bound model has target kind AHMC_TARGET_GLM and is served like the other GLM targets: ahmc_get_target_glm, ahmc_glm_pointwise,
 * ahmc_hglm_get_target (n_coef = P), ahmc_hglm_coefficients, and with has_aux ahmc_glm_aux_get_target and ahmc_glm_dispersion.
 *
 * Kept apart like ahmc_glm_aux.h: exported by libahmc_hip.so only; AHMC_ABI_VERSION, AHMC_GLM_VERSION, AHMC_HGLM_VERSION and
 * AHMC_GLM_AUX_VERSION do not change.
 */
#ifndef AHMC_GLM_FACTOR_H
#define AHMC_GLM_FACTOR_H

#include "ahmc_glm_aux.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AHMC_GLM_FACTOR_VERSION 1
#define AHMC_GLM_FACTOR_MAX 8 /* factors of one model */

int32_t ahmc_glm_factor_version(void);

/* Bind the model: the arguments of ahmc_hglm_set_target with n_coef = P_x (prior_prec has P entries, lo / hi address the P rows);
 * then the factors: n_levels (n_factors, host memory) and levels (n_obs × n_factors, int32, column-major, zero-based, host memory);
 * then the dispersion: has_aux != 0 binds a family of ahmc_glm_aux.h with the prior Normal(aux_loc, aux_scale²) (scale is then not
 * used), has_aux = 0 one of the three families of ahmc_glm.h.  n_factors = 0 is ahmc_hglm_set_target / ahmc_glm_aux_set_target.
 * The model's slab grows by the level indices, per factor the stable permutation of the observations by level, and its row
 * pointers (2·n_obs·n_factors + Σ n_levels + 1 int32), and holds W and R (P × N) also when n_groups = 0.  Everything that can fail
 * happens before the previous target is touched.
 * AHMC_ERR_ARGUMENT: n_coef < 1 or the context's D != P + n_groups + (has_aux ? 1 : 0) ("DimensionMismatch"); n_factors < 0, a NULL
 * n_levels or levels; n_levels[f] < 1 or a level index outside [0, n_levels[f]) ("DomainError"); everything ahmc_hglm_set_target or
 * ahmc_glm_aux_set_target refuses.  AHMC_ERR_UNSUPPORTED: n_factors > AHMC_GLM_FACTOR_MAX, and the neighbours' limits. */
int32_t ahmc_glm_factor_set_target(ahmc_ctx* ctx, int32_t family, int64_t n_obs, int64_t n_coef, const void* X, const void* y, const void* offset,
                                   const void* prior_prec, double scale, int32_t n_groups, const int32_t* lo, const int32_t* hi, const int32_t* centered,
                                   const double* hyper_scale, int32_t n_factors, const int32_t* n_levels, const int32_t* levels, int32_t has_aux,
                                   double aux_loc, double aux_scale);

/* The bound model's P_x, its factors and their levels (n_levels: room for AHMC_GLM_FACTOR_MAX entries; any output may be NULL).  A
 * GLM bound through another entry point reports n_factors = 0.  AHMC_ERR_ARGUMENT: no GLM is bound. */
int32_t ahmc_glm_factor_get_target(ahmc_ctx* ctx, int64_t* n_coef, int32_t* n_factors, int32_t* n_levels);

#ifdef __cplusplus
}
#endif

#endif /* AHMC_GLM_FACTOR_H */
