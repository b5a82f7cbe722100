// ahmc_glm_predict_spec.hpp — what the calls of include/ahmc_glm_predict.h decide on the host, as plain C++: no HIP call, no HIP header,
// like ahmc_glm_spec.hpp, whose checked model (GlmBound) it reads.  glm_predict_spec_check refuses the arguments and the host array
// `levels` or turns them into GlmPredPlan: which quantities the bound model has and which of them the call asks for;
// glm_predict_spec_data checks the staged copies of X, offset and y.  glm_predict_run (ahmc_glm_predict_host.hpp) does the device work
// between and after the two.  The order of the lines below IS the order in which violated conditions are reported.
// tests/test_glm_predict.py runs both through tests/host_ref/glm_predict_spec_driver.cpp on a CPU.
#pragma once

#include "ahmc_glm_predict.h"
#include "ahmc_glm_spec.hpp"

namespace ahmc {

// the draws' block of the summary's sums (ahmc_glm_predict_host.hpp asserts that it is the kernels' tile width)
constexpr int64_t GLM_PRED_BLOCK = 64;

// Quantities of the bound model in the header's order — n_lin predictors, n_mean means or probabilities, n_var variances — and after
// them, as quantity Q, the log-likelihood.  [q0, q1): what this call computes (a summary: all of them, ℓ included if y is given).
struct GlmPredPlan {
  int64_t n_new = 0;
  int n_lin = 1, n_mean = 1, n_var = 1, Q = 3;
  int q0 = 0, q1 = 0;
  bool summary = false, has_y = false, has_offset = false;
  int planes() const { return q1 - q0; }
};

inline int glm_predict_spec_check(const std::string& who, bool bound, const GlmBound& b, const ahmc_glm_newdata* nd, const void* theta, int64_t n_cols,
                                  const void* out, int what, bool summary, GlmPredPlan& p, std::string& err) {
  const auto no = [&err, &who](int code, const std::string& msg) {
    err = who + ": " + msg;
    return code;
  };
  if (!bound) return no(AHMC_ERR_ARGUMENT, "no GLM is bound (ahmc_set_target_glm)");
  if (!nd) return no(AHMC_ERR_ARGUMENT, "newdata is NULL");
  if (!nd->X) return no(AHMC_ERR_ARGUMENT, "newdata.X is NULL");
  const int64_t n_new = nd->n_new;
  if (n_new < 0) return no(AHMC_ERR_ARGUMENT, "n_new must be >= 0; got " + std::to_string((long long)n_new));
  if (n_new > AHMC_GLM_MAX_OBS)
    return no(AHMC_ERR_UNSUPPORTED, "n_new = " + std::to_string((long long)n_new) + " is beyond the engine's limit AHMC_GLM_MAX_OBS = " +
                                        std::to_string((long long)AHMC_GLM_MAX_OBS));
  if (b.F > 0 && !nd->levels) return no(AHMC_ERR_ARGUMENT, "newdata.levels is NULL; the bound model has " + std::to_string(b.F) + " factors");
  for (int f = 0; f < b.F; ++f)
    for (int64_t i = 0; i < n_new; ++i) {
      const int32_t l = nd->levels[i + (int64_t)f * n_new];
      if (l < 0 || l >= b.L[f])
        return no(AHMC_ERR_ARGUMENT, "DomainError: levels[" + std::to_string((long long)i + 1) + ", " + std::to_string(f + 1) + "] = " + std::to_string(l) +
                                         " is outside [0, " + std::to_string(b.L[f]) + ") (zero-based level indices; a level the bound model has not seen is not predicted)");
    }
  if (n_cols < 0 || (n_cols > 0 && n_new > 0 && (!theta || !out))) return no(AHMC_ERR_ARGUMENT, "theta or the output is NULL, or n_cols < 0");
  if (n_cols > INT32_MAX) return no(AHMC_ERR_UNSUPPORTED, "n_cols beyond 2^31 - 1");
  // ---- the quantities
  const bool classes = b.n_cat > 0 || b.n_cls > 0;
  p.n_new = n_new;
  p.n_lin = b.K();
  p.n_mean = b.n_cat > 0 ? b.n_cat : b.n_cls > 0 ? b.n_cls : 1;
  p.n_var = classes ? 0 : 1;
  p.Q = p.n_lin + p.n_mean + p.n_var;
  p.summary = summary;
  p.has_y = nd->y != nullptr;
  p.has_offset = nd->offset != nullptr;
  if (summary) {
    p.q0 = 0;
    p.q1 = p.Q + (p.has_y ? 1 : 0);
    return AHMC_OK;
  }
  switch (what) {
    case AHMC_GLM_PRED_LINEAR: p.q0 = 0, p.q1 = p.n_lin; break;
    case AHMC_GLM_PRED_MEAN: p.q0 = p.n_lin, p.q1 = p.n_lin + p.n_mean; break;
    case AHMC_GLM_PRED_VARIANCE:
      if (classes)
        return no(AHMC_ERR_ARGUMENT, std::string("AHMC_GLM_PRED_VARIANCE of ") + (b.n_cat > 0 ? "an ordinal" : "a categorical") +
                                         " model: its outcome is a category; AHMC_GLM_PRED_MEAN gives the probabilities");
      p.q0 = p.n_lin + p.n_mean, p.q1 = p.Q;
      break;
    case AHMC_GLM_PRED_LOGLIK:
      if (!p.has_y) return no(AHMC_ERR_ARGUMENT, "AHMC_GLM_PRED_LOGLIK needs newdata.y, the outcomes to evaluate");
      p.q0 = p.Q, p.q1 = p.Q + 1;
      break;
    default: return no(AHMC_ERR_ARGUMENT, "unknown what = " + std::to_string(what));
  }
  return AHMC_OK;
}

// X (n_new, Px), off (n_new, K) or NULL, y (n_new) or NULL: host copies of the new data
template <class T>
int glm_predict_spec_data(const std::string& who, const GlmBound& b, const GlmPredPlan& p, const T* X, const T* off, const T* y, std::string& err) {
  const auto no = [&err, &who](const std::string& msg) {
    err = who + ": " + msg;
    return (int)AHMC_ERR_ARGUMENT;
  };
  const int64_t n = p.n_new;
  for (int64_t i = 0; i < n * b.Px; ++i)
    if (!std::isfinite((double)X[i])) return no("ArgumentError: newdata.X holds a non-finite value");
  if (off)
    for (int64_t i = 0; i < n * b.K(); ++i)
      if (!std::isfinite((double)off[i])) return no("ArgumentError: newdata.offset holds a non-finite value");
  if (!y) return AHMC_OK;
  const int family = b.family, n_int = b.n_cat > 0 ? b.n_cat : b.n_cls;  // y holds a category or a class
  const bool counts = family == AHMC_GLM_POISSON_LOG || family == AHMC_GLM_NEGBINOMIAL_LOG;
  for (int64_t i = 0; i < n; ++i) {
    const double yi = (double)y[i];
    const bool ok = n_int > 0                            ? (yi >= 0 && yi < n_int && yi == std::floor(yi))
                    : family == AHMC_GLM_BERNOULLI_LOGIT ? (yi >= 0 && yi <= 1)
                    : counts                             ? (std::isfinite(yi) && yi >= 0)
                                                         : std::isfinite(yi);
    if (!ok && n_int > 0)
      return no("DomainError: y[" + std::to_string(i + 1) + "] = " + std::to_string(yi) + " is not a category: an integer in [0, " + std::to_string(n_int) + ")");
    if (!ok)
      return no("DomainError: y[" + std::to_string(i + 1) + "] = " + std::to_string(yi) + " is outside the family's domain (" +
                (family == AHMC_GLM_BERNOULLI_LOGIT ? "0 <= y <= 1" : counts ? "y >= 0, finite" : "finite") + ")");
  }
  return AHMC_OK;
}

}  // namespace ahmc
