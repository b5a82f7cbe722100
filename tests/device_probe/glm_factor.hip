// Device probe of tests/test_glm_factor.py: the kernels of a GLM with index-coded factors (csrc/ahmc_glm.hpp, compiled with the
// engine's own flags by build.build_probe_object) as they are, so that a test can launch them on operands and a chain list of its
// choosing: k_glm_eta_f (both tile shapes), the dense gradient product with a leading dimension (k_glm_grad_ld, k_glm_gsum_ld) and
// the factors' rows of R (k_glm_fgrad).
#include "ahmc_glm.hpp"

#define AHMC_PROBE_FAC_ETA(T, FAM, BN)                                                                                                          \
  template __global__ void ahmc::k_glm_eta_f<T, FAM, BN>(const T*, const T*, const T*, T, const T*, T*, T*, int, int, int64_t, int64_t, int64_t, \
                                                         const int*, T*, T*, const T*, int64_t, T*, const ahmc::GlmFacTab*, const int*);
#define AHMC_PROBE_FAC_GRAD(T, BN)                                                                                                               \
  template __global__ void ahmc::k_glm_grad_ld<T, BN>(const T*, const T*, const T*, const T*, T*, T*, int, int, int64_t, int64_t, int64_t, const int*, int);
#define AHMC_PROBE_FAC(T)                                                                                                     \
  AHMC_PROBE_FAC_ETA(T, 0, 64) AHMC_PROBE_FAC_ETA(T, 0, 16) AHMC_PROBE_FAC_ETA(T, 4, 64) AHMC_PROBE_FAC_ETA(T, 4, 16)         \
  AHMC_PROBE_FAC_GRAD(T, 64) AHMC_PROBE_FAC_GRAD(T, 16)                                                                       \
  template __global__ void ahmc::k_glm_gsum_ld<T>(const T*, const T*, const T*, T*, int, int64_t, int64_t, int64_t, const int*, int); \
  template __global__ void ahmc::k_glm_fgrad<T>(const T*, const int*, const int*, T*, int, int, int, int64_t, int64_t, const int*);
AHMC_PROBE_FAC(double)
AHMC_PROBE_FAC(float)
