/*
 * ahmc_glm_loo.h — optional: model comparison for the generalised-linear-model targets (ahmc_glm.h and the headers built on it) from the
 * KEPT DRAWS, on the device: the pointwise log-likelihood ℓ(y_i, η_i) of every observation at any (D, n_cols) array of draws, and from
 * it, per observation, the Pareto-smoothed importance-sampling leave-one-out estimate elpd_loo with its Pareto shape k̂ (Vehtari,
 * Simpson, Gelman, Yao & Gabry, "Pareto smoothed importance sampling"; R loo::psis with r_eff = 1), the log pointwise predictive
 * density lpd and WAIC's p_waic — the numbers loo, ArviZ and brms report.
 *
 *     One observation, ℓ_1 … ℓ_S (S = n_cols):  lr_s = −ℓ_s − max_s(−ℓ_s);  M = ⌈min(0.2·S, 3·√S)⌉;  the draws are sorted by −ℓ, ascending
 *     and stably (ties keep the draws' order);  the tail is the top M values, cut the value just below it.  If M >= 5 and the tail is
 *     not constant, x_j = exp(tail_j) − exp(cut) is fitted with a generalised Pareto distribution by Zhang & Stephens' profile
 *     likelihood on a grid of 30 + ⌊√M⌋ points, k̂ = (M·k + 5)/(M + 10), and the j-th smallest tail weight becomes
 *     min(log(σ·expm1(−k̂·log1p(−(j − ½)/M))/k̂ + exp(cut)), 0);  otherwise, or if k̂ or σ is not finite, nothing is smoothed and k̂ = +Inf.
 *     lw = lr − logsumexp(lr);  elpd_loo = logsumexp(lw + ℓ);  lpd = logsumexp(ℓ) − log S;  p_waic = Σ(ℓ − mean ℓ)²/(S − 1) (NaN at S = 1).
 *     elpd_waic = lpd − p_waic and p_loo = lpd − elpd_loo are left to the caller.  An observation with a non-finite ℓ at any draw gets NaN
 *     in all four outputs and in its weights.
 * The order of every sum — what makes an observation's bits depend on its S values in the draws' order alone: not on n_obs, its row, N,
 * the chunking or the kind of pointer — is defined with the host mirror, advancedhmc.jl_amd/glm.py (`psis_loo`).  No float atomics.
 *
 * Neither call touches θ, the point caches, the RNG or the schedule: a transition after either has the bits it would have had without
 * it.  Both evaluate the draws in chunks of at most N columns on the model's own workspaces, like ahmc_glm_class_probs, and serve
 * every family of the GLM targets, with groups, factors, a sampled dispersion, cutpoints and classes.
 *
 * Kept apart like ahmc_glm_categorical.h: exported by libahmc_hip.so only; the versions of the other headers do not change.
 */
#ifndef AHMC_GLM_LOO_H
#define AHMC_GLM_LOO_H

#include "ahmc_glm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AHMC_GLM_LOO_VERSION 1
/* ahmc_glm_loo sorts all n_obs·n_cols values at once with 32-bit positions (observation blocking is the caller's) … */
#define AHMC_GLM_LOO_MAX_VALUES 2147483647
/* … and keeps an observation's tail of M values on chip: M <= 4096, which is n_cols <= 1864135 */
#define AHMC_GLM_LOO_MAX_TAIL 4096

int32_t ahmc_glm_loo_version(void);

/* out (n_obs, n_cols), column-major, in the context's element type: ℓ(y_i, η_i) at draws theta (D, n_cols); theta and out are host or
 * device pointers.  Column j has the bits ahmc_glm_pointwise's loglik_out has for a chain at that θ.  n_cols = 0 writes nothing.
 * AHMC_ERR_ARGUMENT: no GLM is bound; NULL theta or out with n_cols > 0; n_cols < 0.  AHMC_ERR_UNSUPPORTED: n_cols > 2^31 − 1.
 * AHMC_ERR_RUNTIME: the working set ((D + n_obs)·min(n_cols, N) elements) cannot be allocated; the message names the bytes. */
int32_t ahmc_glm_loglik(ahmc_ctx* ctx, const void* theta, int64_t n_cols, void* out);

/* pointwise_out (4, n_obs), column-major, DOUBLE whatever the element type: elpd_loo, pareto_k, lpd, p_waic of each observation over
 * the draws theta (D, n_cols).  log_weights_out (n_cols, n_obs), column-major, double, or NULL: the normalised log-weights lw of each
 * observation in the draws' own order.  All three are host or device pointers.  n_cols = 0 writes nothing.
 * The working set (24 bytes per value of the (n_obs, n_cols) matrix, 8 more with log_weights_out, and ahmc_glm_loglik's) is one
 * allocation made up front; if it cannot be had the call fails with AHMC_ERR_RUNTIME naming the bytes and nothing has changed.
 * AHMC_ERR_ARGUMENT: as ahmc_glm_loglik (pointwise_out in the place of out).  AHMC_ERR_UNSUPPORTED: n_cols > 2^31 − 1;
 * n_obs·n_cols > AHMC_GLM_LOO_MAX_VALUES; a tail longer than AHMC_GLM_LOO_MAX_TAIL. */
int32_t ahmc_glm_loo(ahmc_ctx* ctx, const void* theta, int64_t n_cols, double* pointwise_out, double* log_weights_out);

#ifdef __cplusplus
}
#endif

#endif /* AHMC_GLM_LOO_H */
