// ahmc_lowrank_adapt.hpp — the push of the low-rank mass-matrix adaptor (include/ahmc_lowrank_adapt.h): the pooled Welford / Chan
// update of a window's state by one batch X (D, N) — every chain's position at one iteration —, projected on the thin matrix
// W (D, ℓ) = Ω / s₀ (advancedhmc.jl_amd/rank_update.py: lowrank_push defines the arithmetic):
//   m_b = row mean of X,  X_c = X − m_b,  δ = m_b − μ,  f = n·N/(n + N)
//   Z  += X_c·(X_cᵀW) + f·δ·(δᵀW)        (D, ℓ)
//   m2 += Σ_c X_c² + f·δ²                 (D)
//   μ  += δ·N/(n + N)
// X has the context's element type; every sum, and the whole state, is double.
//
//   k_lr_colsum_partial / _final   m_b, as k_d_colsum_partial / _final (ahmc_dense.hpp) but summed in double whatever X's type is:
//                                  μ and δ inherit m_b's error at first order, and the state is held to double's roundoff
//   k_lr_project                   T (ℓ, N + 1): T[:, c] = Wᵀ(X[:, c] − m_b) for c < N and T[:, N] = Wᵀδ — one full-D reduction per
//                                  column, CPW columns per workgroup so that a W fragment a thread loads serves CPW chains
//   k_lr_accumulate                a workgroup owns 64 rows d and one slice of the chains; a thread keeps its row's
//                                  ℓ partial sums of Z and the m2 column in registers and walks the slice's chains: x_d is a
//                                  coalesced load, T[:, c] is the same for the whole wave (scalar loads).  The number of slices
//                                  follows D alone (lr_slices): enough workgroups to fill the chip, partials that stay small
//   k_lr_merge                     adds the slices' partials in slice order, the f·δ·(δᵀW) term, and updates m2 and μ
//
// No atomics: the state's bits depend on (D, N, ℓ, and the slice counts LR_SLICES and lr_slices(D)) only.  Reduction order of
// k_lr_project: thread t takes rows t, t + 256, … in order, the partial sums meet in wave_allsum's and then the four waves' fixed order.
#pragma once

#include "ahmc_device.hpp"

namespace ahmc {

constexpr int LR_THREADS = 256;
constexpr int LR_SLICES = 64;   // chain slices of the column sums; the most k_lr_accumulate uses
constexpr int LR_ROWS = 64;     // rows per workgroup of k_lr_accumulate (one wave)
constexpr int LR_MAX_ELL = 40;  // AHMC_LOWRANK_MAX_ELL

// the ℓ bucket: LB = 8, 16 or 40 accumulators per thread and column
inline int lr_bucket(int ell) { return ell <= 8 ? 8 : ell <= 16 ? 16 : 40; }
// chain slices of k_lr_accumulate: about 2048 workgroups of 64 rows, at most LR_SLICES slices
inline int lr_slices(int64_t D) {
  const int64_t rb = (D + LR_ROWS - 1) / LR_ROWS, s = 2048 / rb;
  return (int)(s < 1 ? 1 : s > LR_SLICES ? LR_SLICES : s);
}
constexpr int lr_cpw(int LB) { return LB == 8 ? 4 : LB == 16 ? 2 : 1; }  // columns per workgroup of k_lr_project

template <class TX>
__global__ __launch_bounds__(256) void k_lr_colsum_partial(const TX* __restrict__ X, double* __restrict__ partial, int D, int64_t N) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  const int sl = blockIdx.y;
  if (d >= D) return;
  const int64_t per = (N + LR_SLICES - 1) / LR_SLICES;
  const int64_t n0 = sl * per, n1 = n0 + per < N ? n0 + per : N;
  double s = 0;
  for (int64_t n = n0; n < n1; ++n) s += (double)X[d + n * D];
  partial[(int64_t)sl * D + d] = s;
}

__global__ __launch_bounds__(256) void k_lr_colsum_final(const double* __restrict__ partial, double* __restrict__ mean, int D, int64_t N) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= D) return;
  double s = 0;
  for (int sl = 0; sl < LR_SLICES; ++sl) s += partial[(int64_t)sl * D + d];  // fixed order
  mean[d] = s / (double)N;
}

// T[j + c·ell] = Σ_d W[d + j·D]·(X[d + c·D] − mb[d]) for c < N; column N is Wᵀ(mb − mu).  Workgroup b serves columns b·CPW … ; the
// workgroup after the last of them serves column N alone.
template <class TX, int LB>
__global__ __launch_bounds__(LR_THREADS) void k_lr_project(const TX* __restrict__ X, const double* __restrict__ W, const double* __restrict__ mb,
                                                          const double* __restrict__ mu, double* __restrict__ Tm, int D, int64_t N, int ell) {
  constexpr int CPW = lr_cpw(LB);
  __shared__ double red_waves[(LR_THREADS / 64) * CPW * LB];
  const int t = threadIdx.x, w = t >> 6;
  const int64_t nb = (N + CPW - 1) / CPW;
  const bool extra = (int64_t)blockIdx.x == nb;  // the δ column
  const TX* xp[CPW];
  bool live[CPW];
#pragma unroll
  for (int s = 0; s < CPW; ++s) {
    const int64_t c = (int64_t)blockIdx.x * CPW + s;
    live[s] = !extra && c < N;
    xp[s] = X + (live[s] ? c : 0) * (int64_t)D;  // (a dead slot reads column 0 and stores nothing)
  }
  double acc[CPW * LB];
#pragma unroll
  for (int i = 0; i < CPW * LB; ++i) acc[i] = 0;
  for (int d = t; d < D; d += LR_THREADS) {
    const double m = mb[d];
    double xv[CPW];
#pragma unroll
    for (int s = 0; s < CPW; ++s) xv[s] = (double)xp[s][d] - m;
    if (extra) xv[0] = m - mu[d];
#pragma unroll
    for (int j = 0; j < LB; ++j) {
      if (j < ell) {
        const double wv = W[d + (int64_t)j * D];
#pragma unroll
        for (int s = 0; s < CPW; ++s) acc[s * LB + j] += wv * xv[s];
      }
    }
  }
  wave_allsum<64, double, CPW * LB>(acc);
  if ((t & 63) == 0) {
#pragma unroll
    for (int i = 0; i < CPW * LB; ++i) red_waves[w * CPW * LB + i] = acc[i];
  }
  __syncthreads();
  for (int i = t; i < CPW * LB; i += LR_THREADS) {
    const int s = i / LB, j = i % LB;
    double sum = 0;
#pragma unroll
    for (int q = 0; q < LR_THREADS / 64; ++q) sum += red_waves[q * CPW * LB + i];
    if (j >= ell) continue;
    if (extra) {
      if (s == 0) Tm[j + N * (int64_t)ell] = sum;
    } else if ((int64_t)blockIdx.x * CPW + s < N) {
      Tm[j + ((int64_t)blockIdx.x * CPW + s) * (int64_t)ell] = sum;
    }
  }
}

// P[(sl·(LB + 1) + j)·D + d] = Σ_{c in slice sl} x_c[d, c]·T[j, c] for j < LB (zero for j ≥ ell) and, at j = LB, Σ_c x_c[d, c]²
template <class TX, int LB>
__global__ __launch_bounds__(LR_ROWS) void k_lr_accumulate(const TX* __restrict__ X, const double* __restrict__ mb, const double* __restrict__ Tm,
                                                          double* __restrict__ P, int D, int64_t N, int ell) {
  const int d = blockIdx.x * LR_ROWS + threadIdx.x;
  const int sl = blockIdx.y;
  const int64_t per = (N + gridDim.y - 1) / gridDim.y;
  const int64_t n0 = sl * per, n1 = n0 + per < N ? n0 + per : N;
  const bool row = d < D;
  const int dd = row ? d : D - 1;  // (a thread past the last row reads it and stores nothing)
  const double m = mb[dd];
  double acc[LB + 1];
#pragma unroll
  for (int j = 0; j <= LB; ++j) acc[j] = 0;
  const TX* xp = X + dd;
#pragma unroll 2
  for (int64_t c = n0; c < n1; ++c) {
    const double x = (double)xp[c * D] - m;
    const double* tc = Tm + c * (int64_t)ell;  // wave-uniform
#pragma unroll
    for (int j = 0; j < LB; ++j)
      if (j < ell) acc[j] += x * tc[j];
    acc[LB] += x * x;
  }
  if (!row) return;
#pragma unroll
  for (int j = 0; j <= LB; ++j) P[((int64_t)sl * (LB + 1) + j) * D + d] = acc[j];
}

// the slices' partials in slice order, then Chan's cross term and the update of m2 and μ.  f = n·N/(n + N), g = N/(n + N).
template <int LB>
__global__ __launch_bounds__(256) void k_lr_merge(const double* __restrict__ P, const double* __restrict__ Tm, const double* __restrict__ mb,
                                                  double* __restrict__ Z, double* __restrict__ m2, double* __restrict__ mu, int D, int64_t N, int ell,
                                                  int nsl, double f, double g) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= D) return;
  const double delta = mb[d] - mu[d];
  const double* dw = Tm + N * (int64_t)ell;  // Wᵀδ
  for (int j = 0; j < ell; ++j) {
    double s = 0;
    for (int sl = 0; sl < nsl; ++sl) s += P[((int64_t)sl * (LB + 1) + j) * D + d];
    Z[d + (int64_t)j * D] += s + f * delta * dw[j];
  }
  double s = 0;
  for (int sl = 0; sl < nsl; ++sl) s += P[((int64_t)sl * (LB + 1) + LB) * D + d];
  m2[d] += s + f * delta * delta;
  mu[d] += delta * g;
}

// W = Ω / s₀ row-wise
__global__ __launch_bounds__(256) void k_lr_scale(const double* __restrict__ Om, const double* __restrict__ s0, double* __restrict__ W, int D, int ell) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)D * ell) return;
  W[i] = Om[i] / s0[i % D];
}

// Ω[:, j0 … ell) ← standard normals of the adaptor's own Philox stream: key = the adaptor's seed, counter = (column, draw, RNG_LOWRANK,
// pair of rows) — a stream no chain's transition reads (the chains' key is the context's seed, their purposes 0 … 3)
constexpr uint32_t RNG_LOWRANK = 4;
__global__ __launch_bounds__(256) void k_lr_normals(double* __restrict__ Om, int D, int j0, int ell, uint32_t k0, uint32_t k1, uint32_t draw) {
  const int pairs = (D + 1) / 2;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)pairs * (ell - j0)) return;
  const int j = j0 + (int)(i / pairs), p = (int)(i % pairs);
  const Rng rng{k0, k1, (uint32_t)j, draw};
  double a, b;
  rng.normal_pair(RNG_LOWRANK, (uint32_t)p, a, b);
  Om[2 * p + (int64_t)j * D] = a;
  if (2 * p + 1 < D) Om[2 * p + 1 + (int64_t)j * D] = b;
}

}  // namespace ahmc
