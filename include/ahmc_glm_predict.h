/*
 * ahmc_glm_predict.h — optional: predictions of a bound generalised-linear-model target (ahmc_glm.h and the headers built on it) at NEW
 * rows of data, for any (D, n_cols) array of draws, on the device: the linear predictor, the mean and variance of the outcome (or the
 * category / class probabilities), the log-likelihood at held-out outcomes, and, for the S = N·K kept draws of a run, whose (n_new, S)
 * matrix fits nowhere, the per-observation summaries of all of these with the draws reduced in the product's epilogue.
 *
 * The model's full path applies: the effective coefficients (centred and non-centred groups, the dispersion's row, the cutpoints), the
 * factors' levels gathered after the product, the offset added once, last.  η of an element is the k-ordered fma chain over X's columns
 * (tests/host_ref/glm_ref.cpp), plus the factors' rows in order, plus the offset: with the new data equal to the training data it has
 * the bits ahmc_glm_pointwise gives.
 *
 * Per observation and draw there are Q quantities:
 *     families 0 – 4 (one predictor):       η, μ = E[y | θ], v = Var[y | θ]                                   Q = 3
 *     ordered logit, C categories:          η, p_0 … p_{C−1}                                                  Q = 1 + C
 *     categorical logit, K = C − 1:         η_1 … η_K, p_0 … p_{C−1}                                          Q = K + C
 *   Bernoulli: μ = σ(η) from one exp(−|η|), v = μ(1 − μ).  Poisson: μ = exp(η), v = μ.  Gaussian, fixed scale: μ = η, v = 1/scale.
 *   Gaussian, sampled σ (s = log σ): μ = η, v = exp(2s).  Negative binomial (s = log φ): μ = exp(η), v = fma(μ·μ, exp(−s), μ).
 *   The probabilities are those of glm.ordinal_probs and glm.categorical_probs (advancedhmc.jl_amd/glm.py).
 *
 * Neither call touches θ, the point caches, the RNG, the schedule or the bound model's slab: a transition after either has the bits it
 * would have had without it.  Both run on a working set of their own — the new data, one chunk of θ, the chunk's effective coefficients
 * and cutpoint table, the chunk of the matrix or the block partials and the running state — which is ONE allocation made up front;
 * if it cannot be had the call fails with AHMC_ERR_RUNTIME naming the bytes, and nothing has changed.  The chunk is a multiple of 64
 * draws chosen from a byte budget (AHMC_GLM_PREDICT_BUDGET, bytes, read at every call; default 256 MiB), not from N.
 *
 * Out of scope: factor levels the bound model has not seen (random draws y_rep of the outcome are ahmc_glm_yrep.h, a second kernel on the
 * planes this header puts on the device); quantiles of the predictions; observation weights; and a matrix larger than the
 * caller's `out` can hold — ahmc_glm_predict writes planes·n_new·n_cols elements, the summary is what serves large n_cols.
 *
 * Kept apart like ahmc_glm_loo.h: exported by libahmc_hip.so only; the versions of the other headers do not change.
 */
#ifndef AHMC_GLM_PREDICT_H
#define AHMC_GLM_PREDICT_H

#include "ahmc_glm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AHMC_GLM_PREDICT_VERSION 1

/* `what` of ahmc_glm_predict */
#define AHMC_GLM_PRED_LINEAR 0   /* the η planes: 1, or K = C − 1 of a categorical model */
#define AHMC_GLM_PRED_MEAN 1     /* μ (1 plane) for families 0 – 4; the C probability planes of an ordinal or a categorical model */
#define AHMC_GLM_PRED_VARIANCE 2 /* v (1 plane), families 0 – 4 only */
#define AHMC_GLM_PRED_LOGLIK 3   /* ℓ(y_new, η) (1 plane); needs y */

/* New rows of data for the bound model.  X (n_new, P_x) column-major in the context's element type, P_x the bound model's dense columns;
 * levels (n_new, F) int32, zero-based, column-major, F the bound model's factors (NULL if F = 0); offset (n_new, K) column-major, K = 1
 * or the non-reference classes of a categorical model, or NULL: zeros (an offset may be given where the bound model has none); y (n_new)
 * or NULL.  X, offset and y are host or device pointers; levels is host memory, as at bind time. */
typedef struct ahmc_glm_newdata {
  int64_t n_new;
  const void* X;
  const int32_t* levels;
  const void* offset;
  const void* y;
} ahmc_glm_newdata;

int32_t ahmc_glm_predict_version(void);

/* out (planes, n_new, n_cols), column-major (the plane index runs fastest), in the context's element type, at a host or device pointer:
 * the planes `what` names at draws theta (D, n_cols), a host or device pointer.  With the new data equal to the training data
 * AHMC_GLM_PRED_LINEAR has the bits of ahmc_glm_pointwise's eta_out (a categorical model's K planes there are (n_obs, N) arrays one
 * after the other; here they are interleaved), AHMC_GLM_PRED_LOGLIK those of ahmc_glm_loglik, and a categorical model's
 * AHMC_GLM_PRED_MEAN those of ahmc_glm_class_probs.  n_new = 0 or n_cols = 0 writes nothing.
 * The refusals, in this order.  AHMC_ERR_ARGUMENT: no GLM is bound; newdata or its X is NULL; n_new < 0.  AHMC_ERR_UNSUPPORTED:
 * n_new > AHMC_GLM_MAX_OBS.  AHMC_ERR_ARGUMENT: levels is NULL although the model has factors; a level outside [0, n_levels_f) (the
 * message names the row and the factor); theta or out is NULL where something would be written (n_cols > 0 and n_new > 0), or
 * n_cols < 0 (AHMC_ERR_UNSUPPORTED: n_cols > 2^31 − 1); an unknown `what`; AHMC_GLM_PRED_VARIANCE of an ordinal or a categorical model;
 * AHMC_GLM_PRED_LOGLIK without y; a non-finite value in X or offset; y outside the family's domain (the conditions of the bind).
 * AHMC_ERR_RUNTIME: the working set cannot be allocated, or exceeds a budget given in the environment. */
int32_t ahmc_glm_predict(ahmc_ctx* ctx, const ahmc_glm_newdata* newdata, const void* theta, int64_t n_cols, int32_t what, void* out);

/* summary_out (2Q + 1, n_new), column-major, DOUBLE whatever the element type, at a host or device pointer: rows 2q and 2q + 1 are the
 * mean and the variance (divisor S − 1; NaN at S = 1) of quantity q over the S = n_cols draws; the last row is
 * lpd_i = logsumexp_s ℓ(y_i, η_is) − log S, NaN where y is NULL.  An observation with a non-finite value of a quantity at any draw gets
 * NaN in that quantity's two rows; likewise for lpd.  The quantities of at most one chunk of draws exist at a time, in registers and
 * LDS; what goes to memory is 16 bytes per quantity, observation and block of 64 draws — and, for a categorical model only, the K
 * predictors of the chunk (n_new·K·chunk elements of the working set, which the chunk's size accounts for).
 *     The order of the sums (advancedhmc.jl_amd/glm.py: predict_summary, the host mirror): the draws are cut into blocks of 64 — block b
 *     holds draws 64b … 64b + 63 whatever the chunking; inside a block, in double, ascending: n_b, mean_b = (Σx)/n_b, M2_b = Σ(x − mean_b)²,
 *     and for ℓ m_b = max, s_b = Σ exp(ℓ − m_b); the blocks are combined in ascending order by Chan's update (δ = mean_b − mean,
 *     n′ = n + n_b, mean += δ·n_b/n′, M2 += M2_b + δ·δ·n·n_b/n′) and the running (m, s) rescaling — plain IEEE operations, nothing fused.
 * An observation's bits therefore depend on its row of the new data and the S draws in their order alone: not on n_new, its row index,
 * N, the chunk, or the kind of pointer.  No float atomics.
 * The refusals are ahmc_glm_predict's (summary_out in the place of out; `what` does not apply). */
int32_t ahmc_glm_predict_summary(ahmc_ctx* ctx, const ahmc_glm_newdata* newdata, const void* theta, int64_t n_cols, double* summary_out);

#ifdef __cplusplus
}
#endif

#endif /* AHMC_GLM_PREDICT_H */
