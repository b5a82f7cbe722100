// Driver of tests/test_glm_predict.py: the host-only steps of the calls of include/ahmc_glm_predict.h (csrc/ahmc_glm_predict_spec.hpp:
// glm_predict_spec_check, then glm_predict_spec_data on host copies of the new data) the way glm_predict_run
// (csrc/ahmc_glm_predict_host.hpp) runs them, with host arrays in the place of the staging copies from the device.  Built by the test
// itself with the host compiler: the header includes nothing of HIP.  The bound model is described by the fields the checks read.
#include "ahmc_glm_predict_spec.hpp"

#include <algorithm>

namespace {

// bound: a GLM is bound; (family, Px, F, n_levels, n_cat, n_cls): the bound model; has_nd: the record is not NULL; then its fields;
// has_theta / has_out: the pointers are not NULL; summary: ahmc_glm_predict_summary.  planes_out: the planes the call would write.
template <class T>
int run(int bound, int family, int64_t Px, int F, const int32_t* n_levels, int n_cat, int n_cls, int has_nd, int64_t n_new, const T* X, const int32_t* levels,
        const T* offset, const T* y, int has_theta, int64_t n_cols, int has_out, int what, int summary, int* planes_out, char* msg, int64_t msg_len) {
  ahmc::GlmBound b;
  b.family = family;
  b.Px = Px;
  b.F = F;
  for (int f = 0; f < F && f < AHMC_GLM_FACTOR_MAX; ++f) b.L[f] = n_levels[f];
  b.n_cat = n_cat;
  b.n_cls = n_cls;
  const ahmc_glm_newdata nd{n_new, X, levels, offset, y};
  static const char dummy = 0;
  ahmc::GlmPredPlan p;
  std::string err;
  const std::string who = summary ? "glm_predict_summary" : "glm_predict";
  int rc = ahmc::glm_predict_spec_check(who, bound != 0, b, has_nd ? &nd : nullptr, has_theta ? &dummy : nullptr, n_cols, has_out ? &dummy : nullptr, what,
                                        summary != 0, p, err);
  if (!rc && p.n_new > 0) rc = ahmc::glm_predict_spec_data<T>(who, b, p, X, offset, y, err);
  if (!rc && planes_out) *planes_out = p.planes();
  if (msg_len > 0) {
    const size_t n = std::min(err.size(), (size_t)msg_len - 1);
    memcpy(msg, err.data(), n);
    msg[n] = 0;
  }
  return rc;
}

}  // namespace

#define GLM_PREDICT_SPEC_RUN(NAME, T)                                                                                                                            \
  extern "C" int NAME(int bound, int family, int64_t Px, int F, const int32_t* n_levels, int n_cat, int n_cls, int has_nd, int64_t n_new, const T* X,            \
                      const int32_t* levels, const T* offset, const T* y, int has_theta, int64_t n_cols, int has_out, int what, int summary, int* planes_out,    \
                      char* msg, int64_t msg_len) {                                                                                                               \
    return run<T>(bound, family, Px, F, n_levels, n_cat, n_cls, has_nd, n_new, X, levels, offset, y, has_theta, n_cols, has_out, what, summary, planes_out, msg, \
                  msg_len);                                                                                                                                       \
  }
GLM_PREDICT_SPEC_RUN(glm_predict_spec_run_f64, double)
GLM_PREDICT_SPEC_RUN(glm_predict_spec_run_f32, float)
