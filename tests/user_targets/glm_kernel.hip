// The logistic regression of include/ahmc_glm.h as a straightforward user KERNEL for ahmc_set_target_kernel (signature:
// include/ahmc_hip.h), one wavefront per chain, 4 chains per 256-thread block — what a user would write without the MFMA path, and
// the yardstick scripts/glm_bench.py sets GLMTarget against.  Every chain reads the whole design matrix:
//   pass 1, lanes over the observations:  η_i = Σ_d X[i,d]·θ_d + offset_i;  ℓ_i, u_i = y_i − σ(η_i);  u_i → the chain's column of U
//   pass 2, one coefficient at a time:    g_d = −Σ_i X[i,d]·u_i + p_d·θ_d  (lanes over i, a wave reduction per d)
// `user` points to a GlmUser in device memory.  Both passes read X coalesced (column-major, consecutive lanes = consecutive rows).
#include <hip/hip_runtime.h>
#include <stdint.h>

template <class T>
struct GlmUser {
  const T* X;     // (n_obs, D) column-major
  const T* y;     // (n_obs)
  const T* off;   // (n_obs) or null
  const T* prec;  // (D)
  T* U;           // workspace (n_obs, N)
  int64_t n_obs;
};

template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <class T>
__device__ __forceinline__ void glm_logit_chain(const T* __restrict__ theta, T* __restrict__ lp, T* __restrict__ grad_neg, const int32_t* __restrict__ cols,
                                                int64_t n_cols, int32_t D, const GlmUser<T>* __restrict__ m) {
  const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= n_cols) return;
  const int64_t c = cols ? (int64_t)cols[k] : k;
  const int lane = threadIdx.x & 63;
  const int64_t n = m->n_obs;
  const T* th = theta + c * D;
  T* u = m->U + c * n;
  T part = 0;
  for (int64_t i = lane; i < n; i += 64) {
    T eta = m->off ? m->off[i] : T(0);
    for (int d = 0; d < D; ++d) eta += m->X[i + d * n] * th[d];
    const T e = exp(-fabs(eta));
    const T sig = eta >= T(0) ? T(1) / (T(1) + e) : e / (T(1) + e);
    part += m->y[i] * eta - ((eta > T(0) ? eta : T(0)) + log1p(e));
    u[i] = m->y[i] - sig;
  }
  __threadfence_block();  // the wave's stores to u before its other lanes' loads below (no barrier: a wave past the list has already returned)
  T prior = 0;
  for (int d = 0; d < D; ++d) {
    T s = 0;
    for (int64_t i = lane; i < n; i += 64) s += m->X[i + d * n] * u[i];
    s = wave_sum(s);
    if (lane == 0) grad_neg[c * D + d] = -s + m->prec[d] * th[d];
    prior += m->prec[d] * th[d] * th[d];
  }
  part = wave_sum(part);
  if (lane == 0) lp[c] = part - prior / 2;
}

extern "C" __global__ __launch_bounds__(256) void glm_logit_f64(const double* __restrict__ theta, double* __restrict__ lp, double* __restrict__ grad_neg,
                                                                 const int32_t* __restrict__ cols, int64_t n_cols, int32_t D, int64_t N, void* user) {
  glm_logit_chain<double>(theta, lp, grad_neg, cols, n_cols, D, static_cast<const GlmUser<double>*>(user));
}

extern "C" __global__ __launch_bounds__(256) void glm_logit_f32(const float* __restrict__ theta, float* __restrict__ lp, float* __restrict__ grad_neg,
                                                                 const int32_t* __restrict__ cols, int64_t n_cols, int32_t D, int64_t N, void* user) {
  glm_logit_chain<float>(theta, lp, grad_neg, cols, n_cols, D, static_cast<const GlmUser<float>*>(user));
}
