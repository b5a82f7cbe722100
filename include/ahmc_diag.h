/*
 * ahmc_diag.h — optional convergence diagnostics of the HIP engine: the columns of MCMCChains' `summarystats`
 * (mean, std, mcse, ess_bulk, ess_tail, rhat, plus ess_basic, rhat_bulk, rhat_tail) computed on the device from the
 * draws buffer ahmc_sample(samples_out = …) fills.  The statistics are the rank-normalised split-chain diagnostics of
 * Vehtari, Gelman, Simpson, Carpenter & Bürkner (2021), Bayesian Analysis 16(2); the exact definition is the host mirror
 * advancedhmc.jl_amd/diagnostics.py: summarystats (bit-level agreement with MCMCDiagnosticTools.jl is not claimed).
 *
 * Kept apart from ahmc_hip.h: these entry points are exported by libahmc_hip.so only (the CPU checker under oracle/ does not
 * implement them) and they do not change AHMC_ABI_VERSION.  Conventions (status codes, ahmc_last_error) are ahmc_hip.h's.
 */
#ifndef AHMC_DIAG_H
#define AHMC_DIAG_H

#include "ahmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AHMC_DIAG_VERSION 1

/* row s of the summary: out[s*D + d] */
#define AHMC_DIAG_MEAN 0
#define AHMC_DIAG_STD 1
#define AHMC_DIAG_MCSE 2
#define AHMC_DIAG_ESS_BULK 3
#define AHMC_DIAG_ESS_TAIL 4
#define AHMC_DIAG_RHAT 5
#define AHMC_DIAG_ESS_BASIC 6
#define AHMC_DIAG_RHAT_BULK 7
#define AHMC_DIAG_RHAT_TAIL 8
#define AHMC_DIAG_NROWS 9

int32_t ahmc_diag_version(void);

/* The nine rows for every dimension, pooled over ALL N chains of ctx.  draws: the DEVICE buffer of the context's element type
 * in ahmc_sample's layout, element (d, c, k) at d + D*c + D*N*k, n_draws = K >= 4 (split chains: the first and the last
 * floor(K/2) draws of each chain; the middle draw of an odd K is dropped).  max_lag: cap on the autocorrelation lags of the
 * ESS (0: none).  out: 9*D doubles, host or device.  A dimension with a non-finite value gets NaN in all nine rows.
 * AHMC_ERR_ARGUMENT: draws not a device pointer, out NULL, n_draws < 4, max_lag < 0.  AHMC_ERR_UNSUPPORTED: 2*N*floor(K/2)
 * >= 2^31, or a communicator of more than one rank (ranks are not pooled across ranks). */
int32_t ahmc_diag_summary(ahmc_ctx* ctx, const void* draws, int64_t n_draws, int64_t max_lag, double* out);

/* The rank-normalised z (folded = 0) or the folded z_f (folded = 1) of dimension d: out (K, N) doubles, element (k, c) at
 * c + N*k, NaN at a dropped middle draw (and everywhere if the dimension holds a non-finite value).  Errors as above, plus
 * AHMC_ERR_ARGUMENT for d outside [0, D) or folded not 0 / 1. */
int32_t ahmc_diag_rank_normalize(ahmc_ctx* ctx, const void* draws, int64_t n_draws, int64_t d, int32_t folded, double* out);

#ifdef __cplusplus
}
#endif

#endif /* AHMC_DIAG_H */
