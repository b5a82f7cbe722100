// ahmc_glm_yrep.hpp — device side of include/ahmc_glm_yrep.h (host side: ahmc_glm_yrep_host.hpp; the sampler: ahmc_glm_yrep_draw.hpp; the
// contract: advancedhmc.jl_amd/glm.py: yrep_at, yrep_summary).
//
// k_glm_yrep is elementwise over planes that are already in memory — a chunk of k_glm_pred's matrix, or the caller's q — one thread per
// (row, col): it converts the element's planes to double, runs the family's sampler on the element's own Philox counter and stores y in
// the element type.  The summary's kernels reduce a chunk's y_rep per observation under the contract of the prediction summary: blocks
// of 64 draws (glm_pred_block_moments on a row of the transposed tile), folded in ascending block order by Chan's update; the two
// counts are integers.  ahmc_glm.hpp and the kernels of ahmc_glm_predict.hpp are used as they are.  No atomics, no scratch, static LDS.
#pragma once

#include "ahmc_glm_predict.hpp"
#include "ahmc_glm_yrep_draw.hpp"

namespace ahmc {

// the element's stream: Philox4x32-10 under the caller's seed at counter (row, col, YREP_PURPOSE, slot); the engine's key is not used
struct GlmYrepGen {
  uint32_t k0, k1, row, col, slot;
  __device__ __forceinline__ void next(double& u, double& u2) {
    const Philox4 p = philox4x32_10(row, col, YREP_PURPOSE, slot, k0, k1);
    ++slot;
    u = u53(p.v[0], p.v[1]);
    u2 = u53(p.v[2], p.v[3]);
  }
};

// element e = i + n_rows·j, i < n_rows, j < n_cols: planes q[planes·e …), aux[aux_ld·j] (or aux[e] if aux_ld < 0), counter
// (row ? row[e] : i, col ? col[e] : col0 + j)
template <class T>
struct GlmYrepArgs {
  const T* q;
  const T* aux;
  const int32_t* row;
  const int32_t* col;
  T* y;
  int64_t n_rows, n_cols, aux_ld, col0;
  int planes, C;
  uint32_t k0, k1;
};

template <class T>
struct GlmYrepPlanes {
  const T* q;
  __device__ __forceinline__ double operator()(int c) const { return (double)q[c]; }
};

template <class T, int FAM>
__global__ __launch_bounds__(256) void k_glm_yrep(const GlmYrepArgs<T> a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.n_rows * a.n_cols) return;
  const int64_t j = e / a.n_rows, i = e - j * a.n_rows;
  GlmYrepGen gen{a.k0, a.k1, a.row ? (uint32_t)a.row[e] : (uint32_t)i, a.col ? (uint32_t)a.col[e] : (uint32_t)(a.col0 + j), 0u};
  double aux = 0.0;
  if constexpr (FAM == 4) aux = (double)a.aux[a.aux_ld < 0 ? e : a.aux_ld * j];
  const GlmYrepPlanes<T> p{a.q + (int64_t)a.planes * e};
  a.y[e] = (T)yrep_draw<FAM>(p, aux, a.C, gen);
}

// what the summary keeps per observation and block of 64 draws, and as its running state: the moments and the two counts
struct GlmYrepPart {
  double2 mom;
  long long less, equal;
};

// y (n_new, nc) of one chunk, nc draws that begin at a block's first → part[row·nblk_cap + b].  A workgroup takes 64 rows × 64 draws
// through LDS ([row][column], as k_glm_pred's summary epilogue); thread r < 64 reduces row r's draws in ascending order.
template <class T>
__global__ __launch_bounds__(256) void k_glm_yrep_blocks(const T* __restrict__ y, const T* __restrict__ y_obs, GlmYrepPart* __restrict__ part, int n_new, int64_t nc,
                                                         int64_t nblk_cap) {
  constexpr int BN = GLM_PRED_BN;
  __shared__ T smem[64 * (BN + 1)];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nrb = (n_new + 63) / 64;
  const int rblk = blockIdx.x % nrb;
  const int64_t cb = blockIdx.x / nrb;
  const int m0 = rblk * 64;
  const int64_t n0 = cb * BN;
  const int nb = nc - n0 < BN ? (int)(nc - n0) : BN;
  for (int cl = w; cl < BN; cl += 4)  // a wave per column: 64 consecutive observations
    smem[lane * (BN + 1) + cl] = (cl < nb && m0 + lane < n_new) ? y[(m0 + lane) + (int64_t)n_new * (n0 + cl)] : T(0);
  __syncthreads();
  if (tid < 64 && m0 + tid < n_new) {
    const T* r = smem + tid * (BN + 1);
    GlmYrepPart p;
    p.mom = glm_pred_block_moments<T>(r, nb);
    p.less = 0;
    p.equal = 0;
    if (y_obs) {
      const double yo = (double)y_obs[m0 + tid];
      for (int c = 0; c < nb; ++c) {
        const double x = (double)r[c];
        p.less += x < yo ? 1 : 0;
        p.equal += x == yo ? 1 : 0;
      }
    }
    part[(int64_t)(m0 + tid) * nblk_cap + cb] = p;
  }
}

// the running state of an observation after the chunk's nblk partials, blocks b0 … b0 + nblk − 1 of the S draws (k_glm_pred_fold's
// update, operation for operation); last: summary (4, n_new) — mean, M2/(S − 1) (NaN at S = 1), and with has_y the two counts over S
__global__ __launch_bounds__(256) void k_glm_yrep_fold(const GlmYrepPart* __restrict__ part, GlmYrepPart* __restrict__ state, double* __restrict__ summary, int n_new,
                                                       int64_t nblk, int64_t nblk_cap, int64_t b0, int64_t S, int first, int last, int has_y) {
#pragma clang fp contract(off)
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_new) return;
  const GlmYrepPart* p = part + row * nblk_cap;
  GlmYrepPart st;
  if (first) {
    st.mom = make_double2(0.0, 0.0);
    st.less = 0;
    st.equal = 0;
  } else {
    st = state[row];
  }
  double mean = st.mom.x, M2 = st.mom.y;
  for (int64_t b = 0; b < nblk; ++b) {
    const double n = (double)(64 * (b0 + b));
    const int64_t left = S - 64 * (b0 + b);
    const double nb = (double)(left < 64 ? left : 64);
    const double np = n + nb;
    const double d = p[b].mom.x - mean;
    const double f = nb / np;
    const double df = d * f;
    mean = mean + df;
    double c = d * d;
    c = c * n;
    c = c * nb;
    c = c / np;
    const double add = p[b].mom.y + c;
    M2 = M2 + add;
    st.less += p[b].less;
    st.equal += p[b].equal;
  }
  st.mom = make_double2(mean, M2);
  state[row] = st;
  if (last) {
    double* o = summary + 4 * row;
    o[0] = mean;
    o[1] = S > 1 ? M2 / (double)(S - 1) : NAN;
    o[2] = has_y ? (double)st.less / (double)S : NAN;
    o[3] = has_y ? (double)st.equal / (double)S : NAN;
  }
}

}  // namespace ahmc
