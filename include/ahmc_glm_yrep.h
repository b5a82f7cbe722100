/*
 * ahmc_glm_yrep.h — optional: posterior-predictive draws y_rep ~ p(y | θ_s) of a bound generalised-linear-model target (ahmc_glm.h and the
 * headers built on it) at new rows of data, for any (D, n_cols) array of draws, on the device, and — for the S = N·K kept draws of a
 * run, whose (n_new, S) matrix fits nowhere — their per-observation summaries.  The planes the sampler reads (μ; μ and v; the category or
 * class probabilities) are those of ahmc_glm_predict.h, made by the same kernel into the chunk's workspace; the sampler is a second,
 * elementwise kernel on them.
 *
 * The sampler (advancedhmc.jl_amd/glm.py: yrep_at is the host mirror and defines it; csrc/ahmc_glm_yrep_draw.hpp is its C++ text, which
 * compiles into the kernel and into a CPU program alike).  Arithmetic is double whatever the element type: planes are converted on entry,
 * y on exit.  Randomness: Philox4x32-10 under key = the caller's `seed` (lo, hi) at counter (row, col, 0x59524550, slot): row the new
 * observation's index, col the draw's index among all n_cols (not within the chunk), slot the 4-word blocks the element has taken, from 0.
 * A block gives u = u53(v0, v1), u′ = u53(v2, v3) in (0, 1] and, where a normal is asked for, z = sqrt(−2·log u)·cos(2π·u′).  So an
 * element's y depends on its quantities, its (row, col) and the seed alone: not on N, n_new, the chunk or the kind of pointer — and a
 * PERMUTATION OF THE ROWS CHANGES y_rep, because the counter holds the row.  The engine's own key and streams are not used.
 *     0 Bernoulli (μ): y = [u <= μ].   2, 3 Gaussian (μ, v): y = fma(√v, z, μ).
 *     5 ordered logit, 6 categorical (p_0 … p_{C−1}): F accumulates p_c ascending from +0; y = #{c <= C − 2 : u > F_c}.
 *     1 Poisson (λ = μ): λ < 10 inversion with one u (at most 200 steps); λ >= 10 Hörmann's PTRS, one block a round.
 *     4 negative binomial (μ, s = log φ): g ~ Gamma(φ, 1) by Marsaglia–Tsang (φ < 1: shape φ + 1 and the boost u^(1/φ) from a block of its
 *       own, taken first; a round takes a normal block, then a uniform block), then y ~ Poisson(g·μ/φ), the slots running on.
 * Every rejection loop is capped at 64 rounds; the capped exit yields NaN, with probability below 1e-40 for every shape.  No loop is
 * unbounded, whatever the input bits.  A non-finite (or negative) quantity, or a dispersion that makes λ non-finite, gives NaN; λ = 0
 * gives 0.
 *
 * None of the three calls touches θ, the point caches, the engine's RNG, the schedule or the bound model's slab: a transition after any
 * of them has the bits it would have had without it.  ahmc_glm_yrep and ahmc_glm_yrep_summary run on ahmc_glm_predict's working set —
 * ONE allocation, a chunk of draws from AHMC_GLM_PREDICT_BUDGET / AHMC_GLM_PREDICT_CHUNK — plus the chunk's y_rep.
 *
 * Out of scope: quantiles of y_rep; factor levels the bound model has not seen; observation weights; test statistics T(y_rep) per draw.
 *
 * Kept apart like ahmc_glm_predict.h: exported by libahmc_hip.so only; the versions of the other headers do not change.
 */
#ifndef AHMC_GLM_YREP_H
#define AHMC_GLM_YREP_H

#include "ahmc_glm_predict.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AHMC_GLM_YREP_VERSION 1

int32_t ahmc_glm_yrep_version(void);

/* y_out (n), in the context's element type: one outcome per element from the family's sampler, given the element's quantities
 * q (planes, n), column-major (the plane index runs fastest; planes = 1, 2 for a Gaussian: μ then v, n_categories for families 5 and 6),
 * aux (n), the log-dispersion, for family 4 only (else NULL), and the element's counter row, col (n) each, NULL = 0 … n − 1 and 0.
 * Every array is a host or a device pointer.  No GLM need be bound.  n = 0 writes nothing.
 * The refusals, in this order, all AHMC_ERR_ARGUMENT: an unknown family; n_categories outside 2 … 16 for families 5 and 6; q, y_out or
 * (family 4) aux NULL where something would be read or written (n > 0); n < 0.  AHMC_ERR_RUNTIME: the working set cannot be allocated. */
int32_t ahmc_glm_yrep_at(ahmc_ctx* ctx, int32_t family, int32_t n_categories, int64_t n, const void* q, const void* aux, const int32_t* row, const int32_t* col,
                         uint64_t seed, void* y_out);

/* out (n_new, n_cols), column-major, in the context's element type, at a host or device pointer: y_rep of the bound model at the rows of
 * newdata for the draws theta (D, n_cols); element (i, j) has the counter (row, col) = (i, j).  newdata->y is checked but not used.
 * The refusals are ahmc_glm_predict's, in its order (`what` does not apply). */
int32_t ahmc_glm_yrep(ahmc_ctx* ctx, const ahmc_glm_newdata* newdata, const void* theta, int64_t n_cols, uint64_t seed, void* out);

/* summary_out (4, n_new), column-major, DOUBLE whatever the element type, at a host or device pointer: the mean and the variance
 * (divisor S − 1; NaN at S = 1) of the observation's y_rep — the values ahmc_glm_yrep writes, in the element type — over the S = n_cols
 * draws, in the order of ahmc_glm_predict_summary's sums (blocks of 64 draws, ascending; advancedhmc.jl_amd/glm.py: yrep_summary); and,
 * where newdata->y is given, p_less = #(y_rep < y)/S and p_equal = #(y_rep == y)/S from integer counts (NaN rows without y).  An
 * observation with a NaN draw gets NaN moments; a NaN draw is neither less nor equal.  No float atomics.
 * The refusals are ahmc_glm_predict's (summary_out in the place of out). */
int32_t ahmc_glm_yrep_summary(ahmc_ctx* ctx, const ahmc_glm_newdata* newdata, const void* theta, int64_t n_cols, uint64_t seed, double* summary_out);

#ifdef __cplusplus
}
#endif

#endif /* AHMC_GLM_YREP_H */
