// Device probe of tests/test_glm_target.py: the GLM target's gradient kernels as they are (the templates of csrc/ahmc_glm.hpp
// compiled with the engine's own flags, build.build_probe_object), so that a test can launch the product Xᵀ·U alone on a U of its
// choosing; and one kernel that evaluates the two device functions of the link epilogue, exp and log1p, element by element.
#include "ahmc_glm.hpp"

#define AHMC_PROBE_GLM_GRAD(T, BN)                                                                                                \
  template __global__ void ahmc::k_glm_grad<T, BN>(const T*, const T*, const T*, const T*, T*, T*, int, int, int64_t, int64_t, \
                                                   const int*, int);
AHMC_PROBE_GLM_GRAD(double, 64)
AHMC_PROBE_GLM_GRAD(double, 16)
AHMC_PROBE_GLM_GRAD(float, 64)
AHMC_PROBE_GLM_GRAD(float, 16)

template __global__ void ahmc::k_glm_gsum<double>(const double*, const double*, const double*, double*, int, int64_t, int64_t, const int*, int);
template __global__ void ahmc::k_glm_gsum<float>(const float*, const float*, const float*, float*, int, int64_t, int64_t, const int*, int);

// e[i] = exp(x[i]), l[i] = log1p(x[i]): the device library's functions as glm_link calls them
template <class T>
__device__ __forceinline__ void probe_exp_log1p(const T* x, T* e, T* l, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  e[i] = exp(x[i]);
  l[i] = log1p(x[i]);
}
extern "C" __global__ void glm_probe_exp_log1p_f64(const double* x, double* e, double* l, int64_t n) { probe_exp_log1p(x, e, l, n); }
extern "C" __global__ void glm_probe_exp_log1p_f32(const float* x, float* e, float* l, int64_t n) { probe_exp_log1p(x, e, l, n); }
