// Device probe of tests/test_glm_aux.py: the two special functions of the negative-binomial link as the kernel calls them
// (glm_gamma_diffs of csrc/ahmc_glm.hpp, compiled with the engine's own flags by build.build_probe_object), element by element:
// L[i] = lgamma(y[i] + phi[i]) − lgamma(phi[i]), P[i] = ψ(y[i] + phi[i]) − ψ(phi[i]).
#include "ahmc_glm.hpp"

template <class T>
__device__ __forceinline__ void probe_gamma_diffs(const T* y, const T* phi, T* L, T* P, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  T l, p;
  ahmc::glm_gamma_diffs(y[i], phi[i], l, p);
  L[i] = l;
  P[i] = p;
}
extern "C" __global__ void glm_aux_probe_gamma_diffs_f64(const double* y, const double* phi, double* L, double* P, int64_t n) { probe_gamma_diffs(y, phi, L, P, n); }
extern "C" __global__ void glm_aux_probe_gamma_diffs_f32(const float* y, const float* phi, float* L, float* P, int64_t n) { probe_gamma_diffs(y, phi, L, P, n); }

// The new kernels as they are, so that a test can launch them on a chain list of its choosing.
#define AHMC_PROBE_AUX_ETA(T, FAM, BN)                                                                                                     \
  template __global__ void ahmc::k_glm_eta<T, FAM, BN>(const T*, const T*, const T*, T, const T*, T*, T*, int, int, int64_t, int64_t, \
                                                       const int*, T*, T*, const T*, int64_t, T*);
#define AHMC_PROBE_AUX(T)                                                                                                                   \
  AHMC_PROBE_AUX_ETA(T, 3, 64) AHMC_PROBE_AUX_ETA(T, 3, 16) AHMC_PROBE_AUX_ETA(T, 4, 64) AHMC_PROBE_AUX_ETA(T, 4, 16)                       \
  template __global__ void ahmc::k_hglm_finish_aux<T>(const T*, const T*, const T*, const T*, const T*, const T*, const ahmc::HglmTab<T>*, \
                                                      T*, T*, int, int, int, int64_t, int64_t, const int*, int, T, T);
AHMC_PROBE_AUX(double)
AHMC_PROBE_AUX(float)
