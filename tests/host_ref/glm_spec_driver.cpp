// Driver of tests/test_glm_spec.py: the host-only steps of binding a GLM (csrc/ahmc_glm_spec.hpp: glm_spec_check, then
// glm_spec_build on a staging copy of the caller's arrays) the way glm_bind (csrc/ahmc_glm_host.hpp) runs them, with host arrays
// in the place of the staging copies from the device.  Built by the test itself with the host compiler: the header includes nothing
// of HIP.  The slab's two tables only have to have the kernels' fields here; their contents are not looked at.
#include "ahmc_glm_spec.hpp"

#include <algorithm>

namespace {

template <class T>
struct Tab {
  int lo[AHMC_HGLM_MAX_GROUPS], hi[AHMC_HGLM_MAX_GROUPS], centered[AHMC_HGLM_MAX_GROUPS];
  T inv_a2[AHMC_HGLM_MAX_GROUPS];
};

struct FTab {
  int F;
  int off[AHMC_GLM_FACTOR_MAX];
  int L[AHMC_GLM_FACTOR_MAX];
};

// entry: ahmc::GlmEntry; (D, N): the context; then the arguments of the entry point's header, those it does not have as 0 / NULL.
// Returns the status; the message goes to msg (at most msg_len bytes with the terminator).
template <class T>
int run(int entry, int64_t D, int64_t N, int family, int64_t n_obs, int64_t n_coef, const T* X, const T* y, const T* offset, const T* prior_prec, double scale,
        int n_groups, const int32_t* lo, const int32_t* hi, const int32_t* centered, const double* hyper_scale, int n_factors, const int32_t* n_levels,
        const int32_t* levels, int has_aux, double aux_loc, double aux_scale, int n_categories, const double* cut_prior, char* msg, int64_t msg_len) {
  const ahmc::GlmSpec s = ahmc::glm_spec(entry, family, n_obs, n_coef, X, y, offset, prior_prec, scale, n_groups, lo, hi, centered, hyper_scale, n_factors, n_levels,
                                         levels, has_aux != 0, aux_loc, aux_scale, n_categories, cut_prior);
  ahmc::GlmBound b;
  std::string err;
  int rc = ahmc::glm_spec_check<T, Tab<T>, FTab>(s, D, N, b, err);
  if (!rc) {
    std::vector<T> h((size_t)b.n_data, T(0));  // (glm_stage)
    std::copy(X, X + b.n_obs * b.Px, h.data() + b.off[ahmc::GLM_X]);
    std::copy(y, y + b.n_obs, h.data() + b.off[ahmc::GLM_Y]);
    if (offset) std::copy(offset, offset + b.n_obs * b.K(), h.data() + b.off[ahmc::GLM_OFF]);
    if (prior_prec) std::copy(prior_prec, prior_prec + b.P, h.data() + b.off[ahmc::GLM_PREC]);
    rc = ahmc::glm_spec_build<T, Tab<T>, FTab>(s, b, h.data(), err);
  }
  if (msg_len > 0) {
    const size_t n = std::min(err.size(), (size_t)msg_len - 1);
    memcpy(msg, err.data(), n);
    msg[n] = 0;
  }
  return rc;
}

}  // namespace

#define GLM_SPEC_RUN(NAME, T)                                                                                                                                       \
  extern "C" int NAME(int entry, int64_t D, int64_t N, int family, int64_t n_obs, int64_t n_coef, const T* X, const T* y, const T* offset, const T* prior_prec,        \
                      double scale, int n_groups, const int32_t* lo, const int32_t* hi, const int32_t* centered, const double* hyper_scale, int n_factors,           \
                      const int32_t* n_levels, const int32_t* levels, int has_aux, double aux_loc, double aux_scale, int n_categories, const double* cut_prior,      \
                      char* msg, int64_t msg_len) {                                                                                                                  \
    return run<T>(entry, D, N, family, n_obs, n_coef, X, y, offset, prior_prec, scale, n_groups, lo, hi, centered, hyper_scale, n_factors, n_levels, levels, has_aux, \
                  aux_loc, aux_scale, n_categories, cut_prior, msg, msg_len);                                                                                        \
  }
GLM_SPEC_RUN(glm_spec_run_f64, double)
GLM_SPEC_RUN(glm_spec_run_f32, float)
