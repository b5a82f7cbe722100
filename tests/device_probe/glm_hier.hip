// Device probe of tests/test_glm_hier.py: the two kernels of the hierarchical GLM target as they are (the templates of
// csrc/ahmc_glm.hpp compiled with the engine's own flags, build.build_probe_object), so that a test can launch them on a chain
// list of its choosing.
#include "ahmc_glm.hpp"

#define AHMC_PROBE_HGLM(T)                                                                                                                  \
  template __global__ void ahmc::k_hglm_coef<T>(const T*, const ahmc::HglmTab<T>*, T*, T*, int, int, int64_t, int64_t, const int*);         \
  template __global__ void ahmc::k_hglm_finish<T>(const T*, const T*, const T*, const T*, const T*, const ahmc::HglmTab<T>*, T*, T*, int, \
                                                  int, int, int64_t, int64_t, const int*, int);
AHMC_PROBE_HGLM(double)
AHMC_PROBE_HGLM(float)
