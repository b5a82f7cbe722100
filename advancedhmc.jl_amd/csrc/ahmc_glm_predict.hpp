// ahmc_glm_predict.hpp — device side of include/ahmc_glm_predict.h (host side: ahmc_glm_predict_host.hpp; the quantities and the order of
// the summary's sums are defined by advancedhmc.jl_amd/glm.py: predict, predict_summary).
//
// The product X_new·W runs exactly as in k_glm_eta — glm_tile_product on the 64×64 tile, rows new observations, columns draws, K = the
// dense columns, then the factors' rows and the offset — so η of an element is the same fma chain.  What differs is the epilogue: the
// quantities of include/ahmc_glm_predict.h (η, μ, v or the probabilities, ℓ) are made in registers, one at a time, and leave through
// LDS either as planes of the chunk's matrix (a wave stores 64 consecutive observations of a draw) or, SUMMARY, transposed to
// [row][column] so that one thread per row reduces the tile's 64 draws — one block of the summary's contract — in ascending order and
// in double; only these block partials are written.  k_glm_pred_fold adds a chunk's partials to the running state.  ahmc_glm.hpp is
// not edited: its glm_tile_product, links, k_hglm_coef and k_glm_cut are used as they are.  No atomics, no scratch, static LDS.
#pragma once

#include "ahmc_glm.hpp"

namespace ahmc {

constexpr int GLM_PRED_BN = 64;  // the tile's columns: a block of draws of the summary (GLM_PRED_BLOCK of ahmc_glm_predict_spec.hpp)

// what a launch of k_glm_pred reads and writes.  Columns are the draws of one chunk: column j of W (stride ldw), of the chunk's θ
// (aux: its dispersion row, stride ldt), of the cutpoint table (3, C − 1, nc_cap) and of eta_ws.
template <class T>
struct GlmPredArgs {
  const T* X;          // (n_new, Px) column-major
  const T* y;          // (n_new) or nullptr
  const T* off;        // (n_new, K) or nullptr
  const int* lev;      // (n_new, F) column-major (FAC)
  const GlmFacTab* ft; // the bound model's factor table (FAC)
  const T* W;          // the effective coefficients
  const T* aux;        // FAM 3, 4: row D − 1 of the chunk's θ
  const T* cut;        // FAM 5: k_glm_cut's table
  T* eta_ws;           // FAM 6: (n_new, K, nc_cap), each element written and read back by the same thread
  T* out;              // !SUMMARY: (planes, n_new, ncols) of the chunk
  double2* part;       // SUMMARY: [(q·n_new + row)·nblk_cap + block] = (mean_b, M2_b), or (m_b, s_b) for ℓ
  T scale;
  int n_new, Px, Pb, K, Cm1;  // Pb: a class's rows of W (FAM 6); K predictors; C − 1 cutpoints (FAM 5)
  int Q, q0, q1;              // the model's quantities; [q0, q1) are made; quantity Q is ℓ
  int64_t ldw, ldt, ncols, nc_cap, nblk_cap;
};

// (mean_b, M2_b) of the nb values r[0 … nb), ascending, in double; (NaN, NaN) if one of them is not finite
template <class T>
__device__ __forceinline__ double2 glm_pred_block_moments(const T* r, int nb) {
#pragma clang fp contract(off)
  double s = 0.0;
  bool fin = true;
  for (int c = 0; c < nb; ++c) {
    const double x = (double)r[c];
    fin = fin && isfinite(x);
    s = s + x;
  }
  const double mean = s / (double)nb;
  double m2 = 0.0;
  for (int c = 0; c < nb; ++c) {
    const double d = (double)r[c] - mean;
    const double dd = d * d;
    m2 = m2 + dd;
  }
  return fin ? make_double2(mean, m2) : make_double2(NAN, NAN);
}

// (m_b, s_b) = (max, Σ exp(ℓ − m_b)) of the nb values r[0 … nb), ascending, in double; (NaN, NaN) if one of them is not finite
template <class T>
__device__ __forceinline__ double2 glm_pred_block_lse(const T* r, int nb) {
#pragma clang fp contract(off)
  double m = (double)r[0];
  bool fin = isfinite(m);
  for (int c = 1; c < nb; ++c) {
    const double x = (double)r[c];
    fin = fin && isfinite(x);
    m = x > m ? x : m;
  }
  double s = 0.0;
  for (int c = 0; c < nb; ++c) {
    const double e = exp((double)r[c] - m);
    s = s + e;
  }
  return fin ? make_double2(m, s) : make_double2(NAN, NAN);
}

// FAM: 0 – 4 as glm_link / glm_link_aux, 5 the ordered logit (glm_link_ord), 6 the categorical logit (its K predictors class after
// class through one accumulator set, as k_glm_eta_cat, then glm_link_cat's arithmetic).  FAC: the bound model has factors.
template <class T, int FAM, bool FAC, bool SUMMARY>
__global__ __launch_bounds__(256) void k_glm_pred(const GlmPredArgs<T> a) {
  constexpr int BN = GLM_PRED_BN;
  using S = GlmShape<BN>;
  using Mf = Mfma<T>;
  constexpr bool AUXF = FAM == 3 || FAM == 4, ORD = FAM == 5, CAT = FAM == 6;
  __shared__ T smem[S::SMEM];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n_new = a.n_new;
  const int nrb = (n_new + GB_M - 1) / GB_M;
  int rblk;
  int64_t cb;
  glm_block<BN>(nrb, rblk, cb);
  const int m0 = rblk * GB_M;
  const int64_t n0 = cb * BN, ncols = a.ncols;
  if (n0 >= ncols) return;
  const int wm = (w % S::WR) * 16 * S::MI, wn = (w / S::WR) * 16 * S::MI;
  const int bn = tid / (GB_K / S::BE);
  const int64_t bcol = n0 + bn < ncols ? n0 + bn : -1;
  // e0: η (FAM <= 5) or m = max(0, η_1 … η_K) (FAM 6) of this thread's elements; zero where the element is past the data
  T e0[S::MI][S::MI][4];
  constexpr int CM = CAT ? S::MI : 1;
  [[maybe_unused]] T inv[CM][CM][4], lse[CM][CM][4];
#pragma unroll
  for (int ti = 0; ti < S::MI; ++ti)
#pragma unroll
    for (int tj = 0; tj < S::MI; ++tj)
#pragma unroll
      for (int v = 0; v < 4; ++v) e0[ti][tj][v] = T(0);
  const int NK = CAT ? a.K : 1;
#pragma unroll 1
  for (int k = 0; k < NK; ++k) {
    typename Mf::acc_t acc[S::MI][S::MI];
#pragma unroll
    for (int i = 0; i < S::MI; ++i)
#pragma unroll
      for (int j = 0; j < S::MI; ++j) acc[i][j] = typename Mf::acc_t{0, 0, 0, 0};
    glm_tile_product<T, BN>(a.X, (int64_t)n_new, n_new, m0, bcol >= 0 ? a.W + bcol * a.ldw + (int64_t)k * a.Pb : nullptr, 0, a.Px, smem, acc);
#pragma unroll
    for (int ti = 0; ti < S::MI; ++ti)
#pragma unroll
      for (int tj = 0; tj < S::MI; ++tj) {
        const int64_t col = n0 + wn + tj * 16 + (lane & 15);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int row = m0 + wm + ti * 16 + Mf::row(lane, v);
          if (row < n_new && col < ncols) {
            T eta = acc[ti][tj][v];
            if constexpr (FAC) {
              const T* wc = a.W + col * a.ldw + (int64_t)k * a.Pb;
              const int F = a.ft->F;
              for (int f = 0; f < F; ++f) eta += wc[a.ft->off[f] + a.lev[row + (int64_t)f * n_new]];
            }
            if (a.off) eta += a.off[(int64_t)k * n_new + row];
            if constexpr (CAT) {
              a.eta_ws[row + (int64_t)n_new * (k + (int64_t)a.K * col)] = eta;
              const T m = e0[ti][tj][v];
              e0[ti][tj][v] = eta > m ? eta : m;
            } else {
              e0[ti][tj][v] = eta;
            }
          }
        }
      }
  }
  // per tile column: the dispersion's constants (FAM 3: exp(−2s) for ℓ, exp(2s) = v; FAM 4: φ = exp(s) for ℓ, exp(−s) for v)
  constexpr int AM = AUXF ? S::MI : 1;
  [[maybe_unused]] T sv[AM], cv[AM], vv[AM];
  if constexpr (AUXF) {
#pragma unroll
    for (int tj = 0; tj < S::MI; ++tj) {
      const int64_t j = n0 + wn + tj * 16 + (lane & 15);
      const T sj = j < ncols ? a.aux[j * a.ldt] : T(0);
      sv[tj] = sj;
      cv[tj] = FAM == 3 ? exp(T(-2) * sj) : exp(sj);
      vv[tj] = FAM == 3 ? exp(T(2) * sj) : exp(-sj);
    }
  }
  // FAM 6: s = exp(−m) + Σ_k exp(η_k − m) ascending, 1/s and the log-sum-exp, as glm_link_cat makes them
  if constexpr (CAT) {
#pragma unroll
    for (int ti = 0; ti < S::MI; ++ti)
#pragma unroll
      for (int tj = 0; tj < S::MI; ++tj) {
        const int64_t col = n0 + wn + tj * 16 + (lane & 15);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int row = m0 + wm + ti * 16 + Mf::row(lane, v);
          T iv = T(0), ls = T(0);
          if (row < n_new && col < ncols) {
            const T* e = a.eta_ws + row + (int64_t)n_new * ((int64_t)a.K * col);
            const T m = e0[ti][tj][v];
            T s = exp(-m);
#pragma unroll 1
            for (int k = 0; k < a.K; ++k) {
              const T ek = exp(e[(int64_t)k * n_new] - m);
              s += ek;
            }
            iv = T(1) / s;
            ls = m + log(s);
          }
          inv[ti][tj][v] = iv;
          lse[ti][tj][v] = ls;
        }
      }
  }
  // quantity q of element (ti, tj, v) at (row, col), both inside the data
  const auto value = [&](int q, int ti, int tj, int v, int row, int64_t col) -> T {
    const T eta = e0[ti][tj][v];
    if constexpr (CAT) {
      const T* e = a.eta_ws + row + (int64_t)n_new * ((int64_t)a.K * col);
      const T m = eta;
      if (q < a.K) return e[(int64_t)q * n_new];
      if (q < a.Q) {
        const int cls = q - a.K;
        const T ek = cls == 0 ? exp(-m) : exp(e[(int64_t)(cls - 1) * n_new] - m);
        return ek * inv[CAT ? ti : 0][CAT ? tj : 0][v];
      }
      const int yi = (int)a.y[row];
      const T ey = yi > 0 ? e[(int64_t)(yi - 1) * n_new] : T(0);
      return ey - lse[CAT ? ti : 0][CAT ? tj : 0][v];
    } else if constexpr (ORD) {
      if (q == 0) return eta;
      const int Cm1 = a.Cm1;
      const int yi = q < a.Q ? q - 1 : (int)a.y[row];
      const int ia = yi < Cm1 ? yi : Cm1 - 1, ib = yi > 0 ? yi - 1 : 0;
      const T* tc = a.cut + col;
      T l, u, da, db;
      glm_link_ord<T>(yi, Cm1, eta, tc[(int64_t)ia * a.nc_cap], tc[(int64_t)ib * a.nc_cap], tc[((int64_t)Cm1 + ia) * a.nc_cap], T(0), l, u, da, db);
      return q < a.Q ? exp(l) : l;
    } else {
      if (q == 0) return eta;
      if (q == a.Q) {
        T l, u;
        if constexpr (AUXF) {
          T dl;
          glm_link_aux<T, FAM>(a.y[row], eta, sv[AUXF ? tj : 0], cv[AUXF ? tj : 0], l, u, dl);
        } else {
          glm_link<T, FAM>(a.y[row], eta, a.scale, l, u);
        }
        return l;
      }
      if constexpr (FAM == 0) {
        const T e = exp(-fabs(eta));
        const T d = T(1) + e;
        const T sig = eta >= T(0) ? T(1) / d : e / d;
        return q == 1 ? sig : sig * (T(1) - sig);
      } else if constexpr (FAM == 1) {
        return exp(eta);
      } else if constexpr (FAM == 2) {
        return q == 1 ? eta : T(1) / a.scale;
      } else if constexpr (FAM == 3) {
        return q == 1 ? eta : vv[AUXF ? tj : 0];
      } else {
        const T mu = exp(eta);
        return q == 1 ? mu : fma(mu * mu, vv[AUXF ? tj : 0], mu);
      }
    }
  };
  const int planes = a.q1 - a.q0;
#pragma unroll 1
  for (int q = a.q0; q < a.q1; ++q) {
    // quantity q of the tile → smem: [row][column] for the row threads' sums, [column][row] for the stores
#pragma unroll
    for (int ti = 0; ti < S::MI; ++ti)
#pragma unroll
      for (int tj = 0; tj < S::MI; ++tj) {
        const int cl = wn + tj * 16 + (lane & 15);
        const int64_t col = n0 + cl;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int rl = wm + ti * 16 + Mf::row(lane, v);
          const int row = m0 + rl;
          const T x = row < n_new && col < ncols ? value(q, ti, tj, v, row, col) : T(0);
          if constexpr (SUMMARY) smem[rl * (BN + 1) + cl] = x;
          else smem[cl * S::LDE + rl] = x;
        }
      }
    __syncthreads();
    if constexpr (SUMMARY) {
      if (tid < GB_M && m0 + tid < n_new) {  // a thread per row: the block partial of its draws, ascending
        const int nb = ncols - n0 < BN ? (int)(ncols - n0) : BN;
        const T* r = smem + tid * (BN + 1);
        a.part[((int64_t)q * n_new + (m0 + tid)) * a.nblk_cap + cb] = q < a.Q ? glm_pred_block_moments<T>(r, nb) : glm_pred_block_lse<T>(r, nb);
      }
    } else {
      for (int cl = w; cl < BN; cl += 4) {  // a wave per column: 64 consecutive observations
        const int64_t j = n0 + cl;
        if (j < ncols && m0 + lane < n_new) a.out[(q - a.q0) + (int64_t)planes * ((m0 + lane) + (int64_t)n_new * j)] = smem[cl * S::LDE + lane];
      }
    }
    __syncthreads();
  }
}

// The running state of the summary: state[q·n_new + row] = (mean, M2) of quantity q < Q over the draws folded so far, (m, s) of ℓ
// (q = Q).  One thread per (quantity, row) adds the chunk's nblk block partials in ascending order: blocks b0 … b0 + nblk − 1 of the
// S draws, block b holding min(64, S − 64b) of them.  first: the state starts at (0, 0) / (−Inf, 0); last: the thread then writes its
// rows of summary (2Q + 1, n_new) — mean and M2/(S − 1) (NaN at S = 1), or lpd = m + log s − log S.
__global__ __launch_bounds__(256) void k_glm_pred_fold(const double2* __restrict__ part, double2* __restrict__ state, double* __restrict__ summary, int n_new, int Q,
                                                       int nq, int64_t nblk, int64_t nblk_cap, int64_t b0, int64_t S, int first, int last) {
#pragma clang fp contract(off)
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nq * n_new) return;
  const int q = (int)(t / n_new);
  const int64_t row = t % n_new;
  const double2* p = part + t * nblk_cap;
  double2 st = first ? make_double2(0.0, 0.0) : state[t];
  if (q < Q) {
    double mean = st.x, M2 = st.y;
    for (int64_t b = 0; b < nblk; ++b) {
      const double n = (double)(64 * (b0 + b));
      const int64_t left = S - 64 * (b0 + b);
      const double nb = (double)(left < 64 ? left : 64);
      const double np = n + nb;
      const double d = p[b].x - mean;
      const double f = nb / np;
      const double df = d * f;
      mean = mean + df;
      double c = d * d;
      c = c * n;
      c = c * nb;
      c = c / np;
      const double add = p[b].y + c;
      M2 = M2 + add;
    }
    st = make_double2(mean, M2);
    if (last) {
      summary[2 * q + (int64_t)(2 * Q + 1) * row] = mean;
      summary[2 * q + 1 + (int64_t)(2 * Q + 1) * row] = S > 1 ? M2 / (double)(S - 1) : NAN;
    }
  } else {
    double m = first ? -HUGE_VAL : st.x, s = first ? 0.0 : st.y;
    for (int64_t b = 0; b < nblk; ++b) {
      const double mb = p[b].x, sb = p[b].y;
      const double mn = mb > m ? mb : m;
      const double a0 = s * exp(m - mn);
      const double a1 = sb * exp(mb - mn);
      s = a0 + a1;
      m = mn;
    }
    st = make_double2(m, s);
    if (last) {
      const double l = m + log(s);
      summary[2 * Q + (int64_t)(2 * Q + 1) * row] = l - log((double)S);
    }
  }
  state[t] = st;
}

// summary row 2Q = NaN for every new observation: the lpd of a call without y
__global__ __launch_bounds__(256) void k_glm_pred_no_lpd(double* __restrict__ summary, int n_new, int Q) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_new) summary[2 * Q + (int64_t)(2 * Q + 1) * i] = NAN;
}

}  // namespace ahmc
