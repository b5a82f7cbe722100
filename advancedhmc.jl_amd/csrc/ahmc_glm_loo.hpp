// ahmc_glm_loo.hpp — PSIS-LOO and WAIC of a GLM target's kept draws on the device (include/ahmc_glm_loo.h): Pareto-smoothed importance
// sampling leave-one-out (Vehtari, Simpson, Gelman, Yao & Gabry; R loo::psis with r_eff = 1) of the (n_obs, S) pointwise
// log-likelihood.  The statistic is defined in advancedhmc.jl_amd/glm.py (`psis_loo`, the host mirror, whose docstring fixes the
// order of every sum); this file computes the same numbers.
//
// Pipeline (host side: ahmc_glm_host.hpp, glm_loo):
//   stage A   per chunk of at most N draws: k_hglm_coef / k_glm_cut / k_glm_eta / k_glm_eta_cat (unedited) write ℓ (n_obs, chunk);
//             k_loo_keys transposes the chunk through an LDS tile into rows of S draws per observation, as the order-preserving
//             u64 key of a = −ℓ widened to double (the key IS the value: diag::from_key gives it back, −0 as +0), with the draw's index
//   stage B   diag's stable segmented radix sort (k_dg_hist / dg_scan / k_dg_scatter), segment = observation, ascending in a
//   stage C   k_loo_psis, one workgroup per observation, all in double, on the sorted row alone
// No atomics but the sort's integer digit counts, no scratch, static LDS.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ahmc_diag.hpp"

namespace ahmc {
namespace loo {

constexpr int LOO_THREADS = 256;
constexpr int LOO_TILE = 32;         // k_loo_keys: observations × draws of one tile
constexpr int LOO_MAX_TAIL = 4096;   // AHMC_GLM_LOO_MAX_TAIL: the tail's M values live in LDS (32 KiB)
constexpr int LOO_MAX_GRID = 96;     // Mg = 30 + ⌊√M⌋ <= 30 + 64

// ---- stage A: ℓ (n_obs, nc) of one chunk, column stride n_obs → keys[i·S + j0 + j] = key(−ℓ[i, j]), idx[i·S + j0 + j] = j0 + j -------------
// One workgroup: 32 observations × 32 draws; the read runs along observations (contiguous in ℓ), the write along draws (contiguous in
// a row of keys), both through a padded LDS tile.
template <class T>
__global__ __launch_bounds__(LOO_THREADS) void k_loo_keys(const T* __restrict__ ll, int64_t n_obs, int64_t nc, int64_t j0, int64_t S,
                                                         uint64_t* __restrict__ keys, uint32_t* __restrict__ idx) {
  __shared__ double tile[LOO_TILE][LOO_TILE + 1];
  const int64_t nbo = (n_obs + LOO_TILE - 1) / LOO_TILE;
  const int64_t bo = (int64_t)blockIdx.x % nbo, bj = (int64_t)blockIdx.x / nbo;
  const int tx = threadIdx.x % LOO_TILE, ty = threadIdx.x / LOO_TILE;  // (ty < 8)
  for (int r = ty; r < LOO_TILE; r += LOO_THREADS / LOO_TILE) {
    const int64_t i = bo * LOO_TILE + tx, j = bj * LOO_TILE + r;
    if (i < n_obs && j < nc) tile[r][tx] = (double)ll[i + j * n_obs];
  }
  __syncthreads();
  for (int r = ty; r < LOO_TILE; r += LOO_THREADS / LOO_TILE) {
    const int64_t i = bo * LOO_TILE + r, j = bj * LOO_TILE + tx;
    if (i < n_obs && j < nc) {
      const int64_t g = i * S + j0 + j;
      keys[g] = diag::to_key(-tile[tx][r]);
      idx[g] = (uint32_t)(j0 + j);
    }
  }
}

// ---- stage C ----------------------------------------------------------------------------------------------------------------------
// Sums over a workgroup: every thread's partial (its elements in ascending index, stride 256), the butterfly over each wave, then the
// four waves' totals as ((w0 + w1) + w2) + w3.  Every thread gets the same bits.
__device__ inline double loo_block_sum(double v, double* sh4) {
  v = diag::dg_wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = ((sh4[0] + sh4[1]) + sh4[2]) + sh4[3];
  __syncthreads();
  return r;
}
__device__ inline double loo_block_max(double v, double* sh4) {
  for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = fmax(fmax(sh4[0], sh4[1]), fmax(sh4[2], sh4[3]));
  __syncthreads();
  return r;
}

// One workgroup per observation.  keys / idx: the observation's row of S sorted keys of a = −ℓ and the draws they came from; M: the tail
// length ⌈min(0.2·S, 3·√S)⌉ (host).  pw (4, n_obs): elpd_loo, pareto_k, lpd, p_waic; lw (S, n_obs) column-major or NULL.
// r below is the sorted position; lr_r = a_r − a_{S−1}; ℓ_r = −a_r.
__global__ __launch_bounds__(LOO_THREADS) void k_loo_psis(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx, int64_t S, int M,
                                                         double* __restrict__ pw, double* __restrict__ lw) {
#pragma clang fp contract(off)
  __shared__ double tail[LOO_MAX_TAIL];  // x_j = exp(tail_j) − exp(cut), then the smoothed log-weights of the tail
  __shared__ double g_th[LOO_MAX_GRID], g_l[LOO_MAX_GRID], g_w[LOO_MAX_GRID];
  __shared__ double sh4[4];
  __shared__ double s_fit[2];  // k̂, σ
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t obs = blockIdx.x;
  const uint64_t* kr = keys + obs * S;
  const uint32_t* ir = idx + obs * S;
  double* out = pw + obs * 4;
  const double a_min = diag::from_key(kr[0]), a_max = diag::from_key(kr[S - 1]);
  // NaN keys sort beyond ±Inf at either end, so a non-finite ℓ anywhere puts one at an end
  if (!(isfinite(a_min) && isfinite(a_max))) {  // (uniform over the workgroup)
    if (t < 4) out[t] = NAN;
    if (lw)
      for (int64_t r = t; r < S; r += LOO_THREADS) lw[obs * S + r] = NAN;
    return;
  }
  const int64_t T0 = S - M;  // the first sorted position of the tail
  double khat = HUGE_VAL;
  bool smoothed = false;
  if (M >= 5 && diag::from_key(kr[T0]) - a_max < 0.0) {  // (uniform: tail_max > tail_min)
    const double ec = exp(diag::from_key(kr[T0 - 1]) - a_max);
    for (int j = t; j < M; j += LOO_THREADS) tail[j] = exp(diag::from_key(kr[T0 + j]) - a_max) - ec;
    __syncthreads();
    // Zhang–Stephens: the profile likelihood on a grid of Mg values of θ
    const double Md = (double)M;
    const int Mg = 30 + (int)floor(sqrt(Md));
    const double xs = tail[(int)floor(Md / 4.0 + 0.5) - 1], xM = tail[M - 1];
    for (int j = w; j < Mg; j += LOO_THREADS / 64) {  // a wave per grid point: lanes stride the tail in ascending order
      const double th = 1.0 / xM + (1.0 - sqrt((double)Mg / ((double)(j + 1) - 0.5))) / (3.0 * xs);
      double s = 0;
      for (int i = lane; i < M; i += 64) s += log1p(-th * tail[i]);
      const double kj = diag::dg_wave_sum(s) / Md;
      if (lane == 0) {
        g_th[j] = th;
        g_l[j] = Md * (log(-th / kj) - kj - 1.0);
      }
    }
    __syncthreads();
    if (t < Mg) {
      double s = 0;
      for (int i = 0; i < Mg; ++i) s += exp(g_l[i] - g_l[t]);
      g_w[t] = 1.0 / s;
    }
    __syncthreads();
    if (w == 0) {
      double th = 0;
      for (int j = 0; j < Mg; ++j) th += g_th[j] * g_w[j];  // (every lane of the wave: the same bits)
      double s = 0;
      for (int i = lane; i < M; i += 64) s += log1p(-th * tail[i]);
      const double k = diag::dg_wave_sum(s) / Md;
      if (lane == 0) {
        s_fit[0] = (Md * k + 5.0) / (Md + 10.0);
        s_fit[1] = -k / th;
      }
    }
    __syncthreads();
    const double kh = s_fit[0], sigma = s_fit[1];
    __syncthreads();
    if (isfinite(kh) && isfinite(sigma)) {  // (uniform)
      khat = kh;
      smoothed = true;
      for (int j = t; j < M; j += LOO_THREADS) {
        const double p = ((double)(j + 1) - 0.5) / Md;
        const double q = sigma * expm1(-kh * log1p(-p)) / kh + ec;
        tail[j] = fmin(log(q), 0.0);
      }
      __syncthreads();
    }
  }
  // the weights before normalisation, by sorted position
  auto lr = [&](int64_t r) { return (smoothed && r >= T0) ? tail[r - T0] : diag::from_key(kr[r]) - a_max; };
  const double Sd = (double)S, l_max = -a_min;
  // pass 1: Σ exp(ℓ − max ℓ), Σ ℓ, max lr
  double s_lpd = 0, s_l = 0, m1 = -HUGE_VAL;
  for (int64_t r = t; r < S; r += LOO_THREADS) {
    const double l = -diag::from_key(kr[r]);
    s_lpd += exp(l - l_max);
    s_l += l;
    m1 = fmax(m1, lr(r));
  }
  s_lpd = loo_block_sum(s_lpd, sh4);
  const double mean = loo_block_sum(s_l, sh4) / Sd;
  m1 = loo_block_max(m1, sh4);
  // pass 2: Σ (ℓ − mean)², Σ exp(lr − max lr)
  double s_v = 0, s_w = 0;
  for (int64_t r = t; r < S; r += LOO_THREADS) {
    const double d = -diag::from_key(kr[r]) - mean;
    s_v += d * d;
    s_w += exp(lr(r) - m1);
  }
  s_v = loo_block_sum(s_v, sh4);
  const double lse = m1 + log(loo_block_sum(s_w, sh4));
  // pass 3: lw = lr − logsumexp(lr), back in the draws' order; max (lw + ℓ)
  double m2 = -HUGE_VAL;
  for (int64_t r = t; r < S; r += LOO_THREADS) {
    const double v = lr(r) - lse;
    if (lw) lw[obs * S + ir[r]] = v;
    m2 = fmax(m2, v - diag::from_key(kr[r]));
  }
  m2 = loo_block_max(m2, sh4);
  // pass 4: Σ exp(lw + ℓ − max)
  double s_e = 0;
  for (int64_t r = t; r < S; r += LOO_THREADS) s_e += exp(((lr(r) - lse) - diag::from_key(kr[r])) - m2);
  s_e = loo_block_sum(s_e, sh4);
  if (t == 0) {
    out[0] = m2 + log(s_e);
    out[1] = khat;
    out[2] = (l_max + log(s_lpd)) - log(Sd);
    out[3] = s_v / (Sd - 1.0);
  }
}

}  // namespace loo
}  // namespace ahmc
