/*
 * ahmc_lowrank_adapt.h — optional mass-matrix adaptor of RankUpdateEuclideanMetric (include/ahmc_rank_update.h): the engine fits
 *     M⁻¹ = Diagonal(A) + B·Dm·Bᵀ,   B: (D, k),  Dm: (k, k) diagonal,
 * to the positions of all N chains of the context — one shared metric, every chain's draw at an iteration a sample — by a
 * diagonal-plus-low-rank estimator that never forms a D×D matrix, so it serves wide contexts (D > 4096) as well.  The reference has
 * no adaptor for this metric; the host mirror advancedhmc.jl_amd/rank_update.py (lowrank_init / _push / _fit / _restart) defines the
 * arithmetic:
 *   a window holds n, μ (D), m2 (D) = Σ(x − μ)² and Z (D, ℓ) = Σ(x − μ)(x − μ)ᵀ·W, W = Ω / s₀ row-wise, for a test matrix Ω (D, ℓ),
 *   ℓ = min(D, k + oversample), and a scaling s₀ (D); every adapting transition inside a window merges the N positions into it on the
 *   device (Chan's pooled update, csrc/ahmc_lowrank_adapt.hpp); at a window end the host fits (A, B, Dm) by a single-pass Nyström
 *   approximation of the covariance in s₀-scaled coordinates, with Stan's shrinkage, sets the metric as ahmc_set_metric_rank_update
 *   does, and starts the next window from s₀ ← the window's standard deviations and Ω ← [the k eigenvectors | fresh normals].
 * All of the state is double whatever the context's element type.
 *
 * Kept apart from ahmc_hip.h as ahmc_rank_update.h is: exported by libahmc_hip.so only, no change of AHMC_ABI_VERSION; status codes
 * and ahmc_last_error are ahmc_hip.h's.
 */
#ifndef AHMC_LOWRANK_ADAPT_H
#define AHMC_LOWRANK_ADAPT_H

#include "ahmc_rank_update.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AHMC_LOWRANK_ADAPT_VERSION 1
#define AHMC_LOWRANK_MAX_ELL 40 /* k + oversample may not exceed it */

int32_t ahmc_lowrank_adapt_version(void);

/* Set up the adaptor: kind = AHMC_ADAPT_MASSMATRIX, AHMC_ADAPT_NAIVE or AHMC_ADAPT_STAN, with delta / init_buffer / term_buffer /
 * window_size as ahmc_adaptor_init takes them; rank 1 <= k <= min(D, AHMC_RANK_UPDATE_MAX_K); oversample >= 0 with
 * k + oversample <= AHMC_LOWRANK_MAX_ELL; seed: the key of the adaptor's own Philox stream (the normals of Ω).
 * The context's metric must be UnitEuclideanMetric, one shared (D,) DiagEuclideanMetric or a rank update of rank <= k; the call
 * turns it into the same M⁻¹ written as a rank-k rank update (B and Dm padded with zeros) and s₀ = √diag(M⁻¹).  From then on
 * ahmc_adapt, ahmc_adapt_point, ahmc_sample and ahmc_sample_from run the adaptor: a push per adapting transition inside the windows
 * and a fit at every window end (AHMC_ADAPT_STAN), or a push and a fit of the draws so far at every transition (the other two
 * kinds); a fit is skipped while the window holds fewer than 10 draws.
 * AHMC_ERR_UNSUPPORTED: a per-chain (D, N) DiagEuclideanMetric, a DenseEuclideanMetric, a communicator set (the fit is not pooled
 * across ranks).  AHMC_ERR_ARGUMENT: k, oversample or kind out of range.  ahmc_adaptor_init ends the adaptor (and refuses a
 * mass-matrix adaptor on the rank-update metric as before); replacing the metric by another kind makes ahmc_adapt / ahmc_sample
 * refuse until an adaptor is set up again. */
int32_t ahmc_lowrank_adaptor_init(ahmc_ctx* ctx, int32_t kind, double delta, int32_t init_buffer, int32_t term_buffer, int32_t window_size,
                                  int64_t k, int64_t oversample, uint64_t seed);

/* The adaptor's parameters and counters: n = draws in the window so far, n_fits = windows started after the first (the counter of
 * the fresh normals' stream). */
typedef struct ahmc_lowrank_state {
  int64_t k;
  int64_t ell;
  uint64_t seed;
  int64_t n;
  int64_t n_fits;
} ahmc_lowrank_state;

/* Checkpoint / resume of the estimator: the header and mu (D), m2 (D), Z (D·ell), s0 (D), Omega (D·ell), column-major doubles, each
 * pointer on the host or the device.  get: any array may be NULL (query the header first).  set: the context must hold an adaptor
 * set up with the same k and ell (ahmc_lowrank_adaptor_init); every array is required.  Together with ahmc_get / set_adaptor_state
 * (which report n_welford = 0 for this adaptor) and the metric, a resumed run continues bit for bit.
 * AHMC_ERR_STATE: no low-rank adaptor on the context. */
int32_t ahmc_lowrank_get_state(ahmc_ctx* ctx, ahmc_lowrank_state* state, double* mu, double* m2, double* Z, double* s0, double* Omega);
int32_t ahmc_lowrank_set_state(ahmc_ctx* ctx, const ahmc_lowrank_state* state, const double* mu, const double* m2, const double* Z,
                               const double* s0, const double* Omega);

#ifdef __cplusplus
}
#endif

#endif /* AHMC_LOWRANK_ADAPT_H */
