// Device probe of tests/test_glm_categorical.py (csrc/ahmc_glm.hpp, compiled with the engine's own flags by build.build_probe_object):
// the two functions the categorical link adds to the exp the other families use, element by element as glm_link_cat calls them —
// L[i] = log(s[i]) and R[i] = 1/s[i] — and the link itself on given η planes, so that a test can apply it to the device's own η.
#include "ahmc_glm.hpp"

template <class T>
__device__ __forceinline__ void probe_log_inv(const T* s, T* L, T* R, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  L[i] = log(s[i]);
  R[i] = T(1) / s[i];
}
extern "C" __global__ void glm_categorical_probe_log_inv_f64(const double* s, double* L, double* R, int64_t n) { probe_log_inv(s, L, R, n); }
extern "C" __global__ void glm_categorical_probe_log_inv_f32(const float* s, float* L, float* R, int64_t n) { probe_log_inv(s, L, R, n); }

// glm_link_cat on E (K planes of (n_obs, N)) in place — the planes become u_k — with m made as k_glm_eta_cat makes it; ℓ (n_obs, N) and
// the probabilities pr (C, n_obs, N)
template <class T>
__device__ __forceinline__ void probe_link(const T* y, T* E, int K, int64_t n_obs, int64_t N, T* ll, T* pr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_obs * N) return;
  const int64_t plane = n_obs * N;
  T m = T(0);
  for (int k = 0; k < K; ++k) {
    const T eta = E[k * plane + i];
    m = eta > m ? eta : m;
  }
  ll[i] = ahmc::glm_link_cat<T>((int)y[i % n_obs], K, E + i, plane, m, pr + (int64_t)(K + 1) * i);
}
extern "C" __global__ void glm_categorical_probe_link_f64(const double* y, double* E, int K, int64_t n_obs, int64_t N, double* ll, double* pr) {
  probe_link(y, E, K, n_obs, N, ll, pr);
}
extern "C" __global__ void glm_categorical_probe_link_f32(const float* y, float* E, int K, int64_t n_obs, int64_t N, float* ll, float* pr) {
  probe_link(y, E, K, n_obs, N, ll, pr);
}

// The new kernel as it is, so that a test can launch it on a chain list of its choosing.
#define AHMC_PROBE_CAT_ETA(T, BN, FAC)                                                                                                          \
  template __global__ void ahmc::k_glm_eta_cat<T, BN, FAC>(const T*, const T*, const T*, const T*, T*, T*, int, int, int, int, int64_t, int64_t, \
                                                           int64_t, const int*, T*, T*, T*, const ahmc::GlmFacTab*, const int*);
#define AHMC_PROBE_CAT(T) AHMC_PROBE_CAT_ETA(T, 64, false) AHMC_PROBE_CAT_ETA(T, 16, false)
AHMC_PROBE_CAT(double)
AHMC_PROBE_CAT(float)
