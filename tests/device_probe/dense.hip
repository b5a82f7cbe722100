// Device probe of tests/test_dense_products.py: the dense engine's product kernels as they are, instantiated on their own so
// that a test can launch them with operands, strides and grids of its choosing.  No wrappers: these are the templates of
// csrc/ahmc_dense.hpp compiled with the engine's own flags (build.build_probe_object).
#include "ahmc_dense.hpp"

#define AHMC_PROBE_GEMM(K, T)                                                                                                  \
  template __global__ void ahmc::K<T>(const T*, const T*, T*, int, int64_t, const int*, const T*, T*, const int*, int64_t, \
                                      int64_t, int64_t, int64_t);
AHMC_PROBE_GEMM(k_dgemm, double)
AHMC_PROBE_GEMM(k_dgemm, float)
AHMC_PROBE_GEMM(k_dgemm_small, double)
AHMC_PROBE_GEMM(k_dgemm_small, float)

template __global__ void ahmc::k_d_coldot<double>(const double*, const double*, double*, double, int, int64_t, const int*);
template __global__ void ahmc::k_d_coldot<float>(const float*, const float*, float*, float, int, int64_t, const int*);
