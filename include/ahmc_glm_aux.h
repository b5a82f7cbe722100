/*
 * ahmc_glm_aux.h — optional families of the generalised-linear-model target (ahmc_glm.h, ahmc_glm_hier.h) whose dispersion parameter
 * is itself sampled: a linear regression with unknown noise σ, and the negative binomial for over-dispersed counts.
 *
 *     θ (D), D = n_coef + n_groups + 1:  the P = n_coef coefficient parameters, the log-scales of the n_groups coefficient groups of
 *     ahmc_glm_hier.h (n_groups may be 0), and LAST s, the log of the family's dispersion parameter.
 *     Prior: s ~ Normal(aux_loc, aux_scale²) — a log-normal on σ or φ, so no Jacobian term.
 *
 *     AHMC_GLM_GAUSSIAN_IDENTITY_SIGMA  σ = e^s:  r = y − η, q = exp(−2s), u = q·r, ℓ = −½·u·r − s, ∂ℓ/∂s = u·r − 1;  y finite
 *     AHMC_GLM_NEGBINOMIAL_LOG          NB2: mean μ = e^η, variance μ + μ²/φ, φ = e^s;  y >= 0 finite, not necessarily an integer
 *         d = η − s, e = exp(−|d|), lse = max(η, s) + log1p(e) = log(μ + φ), σ(d) and 1 − σ(d) from the same e
 *         ℓ = L + φ·(s − lse) + y·(η − lse),  u = y − (y + φ)·σ(d),  ∂ℓ/∂s = φ·(Ψ + s − lse) + φ − (y + φ)·(1 − σ(d))
 *         L = lgamma(y + φ) − lgamma(φ), Ψ = ψ(y + φ) − ψ(φ), both computed as differences (exact 0 at y = 0);  −lgamma(y + 1) is
 *         dropped like log y! of the Poisson family.  s − lse and η − lse are formed without cancellation (−softplus(±d)).
 *     ℓπ(θ) = [ℓπ of ahmc_glm_hier.h over the first P + n_groups rows] − ½((s − aux_loc)/aux_scale)²
 *     g[D−1] = −Σ_i ∂ℓ/∂s + (s − aux_loc)/aux_scale²
 * A φ that underflows to 0 or overflows to ∞ makes ℓ non-finite; a non-finite ℓπ is sanitised to −Inf: a divergence.  The host
 * mirror advancedhmc.jl_amd/glm.py (aux_logdensity, gamma_diffs) defines the arithmetic, including the order of every sum.
 *
 * A bound model has target kind AHMC_TARGET_GLM and is served like the other GLM targets.  ahmc_get_target_glm reports the family
 * (scale: 1); ahmc_glm_pointwise works at the current θ; ahmc_hglm_get_target and ahmc_hglm_coefficients (theta with all D rows)
 * work on it.  ahmc_set_target_glm and ahmc_hglm_set_target refuse the two families: they have no row for s.
 *
 * Kept apart like ahmc_glm_hier.h: exported by libahmc_hip.so only; AHMC_ABI_VERSION, AHMC_GLM_VERSION and AHMC_HGLM_VERSION do not change.
 */
#ifndef AHMC_GLM_AUX_H
#define AHMC_GLM_AUX_H

#include "ahmc_glm_hier.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AHMC_GLM_AUX_VERSION 1
#define AHMC_GLM_AUX_MAX_GROUPS 31 /* a limit this ABI version keeps: one below AHMC_HGLM_MAX_GROUPS */

int32_t ahmc_glm_aux_version(void);

/* Bind the model: the arguments of ahmc_hglm_set_target without scale, then the prior of s.  The workspaces of ahmc_hglm_set_target
 * grow by ⌈n_obs/64⌉·N elements (and hold W and R also when n_groups = 0).  Everything that can fail happens before the previous
 * target is touched.
 * AHMC_ERR_ARGUMENT: a family other than the two above; the context's D != n_coef + n_groups + 1 ("DimensionMismatch"); aux_loc not
 * finite, aux_scale not finite and > 0, a y outside the family's domain ("DomainError"); everything ahmc_hglm_set_target refuses.
 * AHMC_ERR_UNSUPPORTED: n_groups > AHMC_GLM_AUX_MAX_GROUPS, n_obs > AHMC_GLM_MAX_OBS. */
int32_t ahmc_glm_aux_set_target(ahmc_ctx* ctx, int32_t family, int64_t n_obs, int64_t n_coef, const void* X, const void* y, const void* offset,
                                const void* prior_prec, int32_t n_groups, const int32_t* lo, const int32_t* hi, const int32_t* centered,
                                const double* hyper_scale, double aux_loc, double aux_scale);

/* The bound model's prior of s (either output may be NULL).  AHMC_ERR_ARGUMENT: no model is bound through ahmc_glm_aux_set_target. */
int32_t ahmc_glm_aux_get_target(ahmc_ctx* ctx, double* aux_loc, double* aux_scale);

/* From draws theta (D, n_cols) column-major of the context's element type, on the host or the device: out (n_cols) = exp(s), the
 * dispersion σ or φ of every draw.  AHMC_ERR_ARGUMENT: no model is bound through ahmc_glm_aux_set_target. */
int32_t ahmc_glm_dispersion(ahmc_ctx* ctx, const void* theta, int64_t n_cols, void* out);

#ifdef __cplusplus
}
#endif

#endif /* AHMC_GLM_AUX_H */
