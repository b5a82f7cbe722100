/*
 * ahmc_rank_update.h — optional RankUpdateEuclideanMetric of the HIP engine: one inverse mass matrix
 *     M⁻¹ = Diagonal(A) + B·Dm·Bᵀ,   A: D values > 0,  B: (D, k),  Dm: (k, k), both column-major,
 * shared by all chains of a context (the reference's RankUpdateEuclideanMetric(A, B, D), src/metric.jl:179-240; its k×k field `D`
 * is called Dm here so that D keeps meaning the dimension).  ∂H∂r(r) = A∘r + B·(Dm·(Bᵀr)); ℓκ = −½ r·(M⁻¹r); fresh momenta are
 * the reference's rand_momentum (src/metric.jl:322-337) applied to the engine's Philox normals, through the Woodbury factorization
 * (woodbury_factorize, src/metric.jl:164-177) computed on the host in double when the metric is set.  The host mirror
 * advancedhmc.jl_amd/rank_update.py defines the arithmetic.
 *
 * Served wherever the step-synchronous engine serves DenseEuclideanMetric (transitions, refreshes, find_good_stepsize, ahmc_sample
 * with AHMC_ADAPT_NONE / AHMC_ADAPT_STEPSIZE, ask / tell), and on wide contexts (D > 4096).  AHMC_ADAPT_MASSMATRIX / _NAIVE / _STAN,
 * ahmc_lf_pre / ahmc_lf_post are AHMC_ERR_UNSUPPORTED; ahmc_get_metric is AHMC_ERR_ARGUMENT (use ahmc_get_metric_rank_update).
 * ahmc_set_metric replaces the metric as before.
 *
 * Kept apart from ahmc_hip.h: these entry points are exported by libahmc_hip.so only (the CPU checker under oracle/ does not
 * implement them) and they do not change AHMC_ABI_VERSION.  Conventions (status codes, ahmc_last_error) are ahmc_hip.h's.
 */
#ifndef AHMC_RANK_UPDATE_H
#define AHMC_RANK_UPDATE_H

#include "ahmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AHMC_RANK_UPDATE_VERSION 1
#define AHMC_RANK_UPDATE_MAX_K 32 /* an engine limit: a larger k is AHMC_ERR_UNSUPPORTED */

int32_t ahmc_rank_update_version(void);

/* Set M⁻¹ = Diagonal(A) + B·Dm·Bᵀ of the context's element type.  Each pointer may be on the host or the device; A == NULL means
 * ones; B and Dm may be NULL when k == 0 (RankUpdateEuclideanMetric(n): the identity).  0 <= k <= min(D, AHMC_RANK_UPDATE_MAX_K).
 * AHMC_ERR_ARGUMENT, the message naming the reference's exception: k < 0 or k > D ("DimensionMismatch"), B / Dm NULL with k > 0, an
 * A value that is not finite and > 0 ("DomainError"), a non-finite B or Dm value ("ArgumentError"), or I + R·Dm·Rᵀ not positive
 * definite ("PosDefException").  AHMC_ERR_UNSUPPORTED: k > AHMC_RANK_UPDATE_MAX_K. */
int32_t ahmc_set_metric_rank_update(ahmc_ctx* ctx, const void* A, const void* B, const void* Dm, int64_t k);

/* The metric as set: A (D), B (D·k), Dm (k·k) into host or device buffers, k into *k.  Any output may be NULL (query k first).
 * AHMC_ERR_ARGUMENT: the context's metric is not a rank update. */
int32_t ahmc_get_metric_rank_update(ahmc_ctx* ctx, void* A, void* B, void* Dm, int64_t* k);

#ifdef __cplusplus
}
#endif

#endif /* AHMC_RANK_UPDATE_H */
