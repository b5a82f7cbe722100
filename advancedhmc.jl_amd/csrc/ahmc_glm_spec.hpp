// ahmc_glm_spec.hpp — what binding a GLM decides on the host, as plain C++: no HIP call, no HIP header.  One record, GlmSpec, says
// what an ahmc_*_set_target call of include/ahmc_glm*.h received; glm_spec_check refuses it or turns it into GlmBound, the checked
// description with the slab layout that GlmModel keeps; glm_spec_build checks the staged data and fills the slab's tables.
// glm_bind (ahmc_glm_host.hpp) does the device work between and after the two.  The order of the lines below IS the order in
// which violated conditions are reported.  The slab's two table structs live with the kernels (ahmc_glm.hpp) and come in as
// template arguments, so the host compiler alone builds this header: tests/test_glm_spec.py replays the recorded refusals of
// tests/golden/glm_bind_refusals.json through tests/host_ref/glm_spec_driver.cpp on a CPU.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "ahmc_glm_categorical.h"
#include "ahmc_glm_ordinal.h"

namespace ahmc {

// the parts of the model's slab (GlmBound::off)
enum { GLM_X = 0, GLM_XT, GLM_Y, GLM_OFF, GLM_PREC, GLM_U, GLM_PART, GLM_GS, GLM_W, GLM_R, GLM_ZERO, GLM_TAB, GLM_PART_S, GLM_FTAB, GLM_LEV, GLM_PERM, GLM_RP,
       GLM_CUT, GLM_PART_C, GLM_PARTS };

// the kernels' row block and K slice (ahmc_glm_host.hpp asserts that they are GB_M and GLM_K_SLICE)
constexpr int64_t GLM_SPEC_ROW_BLOCK = 64, GLM_SPEC_K_SLICE = 1024;

// which header's entry point binds; from GLM_BY_HIER on each takes what the one before it takes and more
enum GlmEntry { GLM_BY_PLAIN = 0, GLM_BY_HIER, GLM_BY_AUX, GLM_BY_FACTOR, GLM_BY_ORDINAL, GLM_BY_CATEGORICAL };

// a model to bind, as received; X, y, offset and prior_prec may be host or device memory, every other pointer is host memory
// (glm_spec below fills the fields in this order)
struct GlmSpec {
  int entry = GLM_BY_PLAIN;
  int family = 0;
  int64_t n_obs = 0;
  int64_t n_coef = 0;  // the columns of X (GLM_BY_PLAIN: not given, the context's D)
  const void *X = nullptr, *y = nullptr, *offset = nullptr, *prior_prec = nullptr;
  double scale = 1;
  // the coefficient groups (n_groups may be 0)
  int n_groups = 0;
  const int32_t *lo = nullptr, *hi = nullptr, *centered = nullptr;
  const double* hyper_scale = nullptr;
  // θ ends with s, the log dispersion, with the prior Normal(aux_loc, aux_scale²)
  bool aux = false;
  double aux_loc = 0, aux_scale = 1;
  // levels (n_obs, n_factors) column-major, zero-based
  int n_factors = 0;
  const int32_t *n_levels = nullptr, *levels = nullptr;
  // GLM_BY_ORDINAL: the categories, θ ends with the C − 1 rows κ, cut_prior = (loc_1, scale_1, loc_gap, scale_gap);
  // GLM_BY_CATEGORICAL: the classes, K = C − 1 coefficient blocks of n_coef + Σ n_levels rows each
  int32_t n_categories = 0;
  const double* cut_prior = nullptr;

  int n_cat() const { return entry == GLM_BY_ORDINAL ? n_categories : 0; }
  int n_cls() const { return entry == GLM_BY_CATEGORICAL ? n_categories : 0; }
};

// the record of an ahmc_*_set_target call, from its arguments in the headers' order; an entry point leaves out what its header
// does not have.  A model with a dispersion has no scale of its own: it is 1 (include/ahmc_glm_factor.h says so for has_aux).
inline GlmSpec glm_spec(int entry, int family, int64_t n_obs, int64_t n_coef, const void* X, const void* y, const void* offset, const void* prior_prec, double scale,
                        int n_groups = 0, const int32_t* lo = nullptr, const int32_t* hi = nullptr, const int32_t* centered = nullptr,
                        const double* hyper_scale = nullptr, int n_factors = 0, const int32_t* n_levels = nullptr, const int32_t* levels = nullptr, bool aux = false,
                        double aux_loc = 0, double aux_scale = 1, int32_t n_categories = 0, const double* cut_prior = nullptr) {
  return GlmSpec{entry, family, n_obs, n_coef, X, y, offset, prior_prec, aux ? 1.0 : scale, n_groups, lo, hi, centered, hyper_scale, aux, aux_loc, aux_scale,
                 n_factors, n_levels, levels, n_categories, cut_prior};
}

// the checked model: what the evaluations and the get_target calls read, and where the slab's parts are (in elements; part i starts
// at off[i], sizes 0 where the model has none)
struct GlmBound {
  int64_t off[GLM_PARTS] = {};
  int64_t total = 0, n_data = 0;  // the slab, and its leading part that is copied from the host (everything before U)
  int family = 0;
  int64_t n_obs = 0;
  bool has_offset = false;
  double scale = 1;
  int64_t P = 0;  // the coefficient rows: the columns of X and the factors' levels; θ has D = P + G (+ 1 with aux) rows
  int64_t Px = 0;  // the columns of X (= P without factors)
  int F = 0;       // the factors (ahmc_glm_factor.h) and their levels; Lt = Σ levels = P − Px
  int32_t L[AHMC_GLM_FACTOR_MAX] = {};
  int64_t Lt = 0;
  int G = 0;      // the coefficient groups (ahmc_glm_hier.h), as received
  int32_t lo[AHMC_HGLM_MAX_GROUPS] = {}, hi[AHMC_HGLM_MAX_GROUPS] = {}, centered[AHMC_HGLM_MAX_GROUPS] = {};
  double A[AHMC_HGLM_MAX_GROUPS] = {};
  bool bound_hier = false;  // bound through any entry point but ahmc_set_target_glm (n_groups = 0 included)
  bool aux = false;         // θ ends with s, the log dispersion (ahmc_glm_aux.h); its prior Normal(aux_loc, aux_scale²)
  double aux_loc = 0, aux_scale = 1;
  int n_cat = 0;  // the categories C of an ordinal model (ahmc_glm_ordinal.h; 0: not ordinal): θ ends with the C − 1 rows κ
  double cut_prior[4] = {0, 2.5, 0, 1};  // (loc_1, scale_1, loc_gap, scale_gap)
  int n_cls = 0;  // the classes C of a categorical model (ahmc_glm_categorical.h; 0: not categorical): P = (C − 1)·Pb, Pb = Px + Lt

  bool on_w() const { return G > 0 || aux || F > 0 || n_cat > 0 || n_cls > 0; }  // the products run on the effective coefficients W, not on θ
  int K() const { return n_cls > 0 ? n_cls - 1 : 1; }  // predictors per observation: the planes of U, the columns of offset
};

inline bool glm_aux_family(int family) { return family == AHMC_GLM_GAUSSIAN_IDENTITY_SIGMA || family == AHMC_GLM_NEGBINOMIAL_LOG; }

// what the entry points of the older headers answer to a family that has an entry point of its own
inline std::string glm_bound_elsewhere(int family, bool aux) {
  const std::string where = family == AHMC_GLM_ORDERED_LOGIT
                                ? "it samples its cutpoints and is bound through ahmc_glm_ordinal_set_target (include/ahmc_glm_ordinal.h)"
                                : "it has a coefficient block per class and is bound through ahmc_glm_categorical_set_target (include/ahmc_glm_categorical.h)";
  if (aux)
    return "glm_aux_set_target: family " + std::to_string(family) +
           " has no sampled dispersion (AHMC_GLM_GAUSSIAN_IDENTITY_SIGMA, AHMC_GLM_NEGBINOMIAL_LOG): " + where;
  return "set_target_glm: unknown family " + std::to_string(family) + " at this entry point: " + where;
}

// Step 1 of glm_bind: every check that needs the arguments alone (and the host arrays n_levels, levels, lo, hi, hyper_scale,
// cut_prior), then b: the checked copy and the slab layout for a context of (D, N).  Returns the status; err: the message.
template <class T, class Tab, class FTab>
int glm_spec_check(const GlmSpec& s, int64_t D, int64_t N, GlmBound& b, std::string& err) {
  const auto no = [&err](int code, const std::string& msg) {
    err = msg;
    return code;
  };
  const int family = s.family, n_cat = s.n_cat(), n_cls = s.n_cls(), n_groups = s.n_groups, F = s.n_factors;
  const int64_t n_obs = s.n_obs, Px = s.entry == GLM_BY_PLAIN ? D : s.n_coef;
  const bool aux = s.aux;
  const auto n_obs_refusal = [&](const std::string& who) {
    if (n_obs < 1) return no(AHMC_ERR_ARGUMENT, who + ": n_obs must be >= 1; got " + std::to_string(n_obs));
    if (n_obs > AHMC_GLM_MAX_OBS)
      return no(AHMC_ERR_UNSUPPORTED, who + ": n_obs = " + std::to_string(n_obs) + " is beyond the engine's limit AHMC_GLM_MAX_OBS = " +
                                          std::to_string((long long)AHMC_GLM_MAX_OBS));
    return (int)AHMC_OK;
  };
  // ---- include/ahmc_glm_categorical.h, include/ahmc_glm_ordinal.h
  if (s.entry == GLM_BY_CATEGORICAL) {
    if (n_cls < 2) return no(AHMC_ERR_ARGUMENT, "DomainError: n_categories = " + std::to_string(n_cls) + "; a categorical outcome has at least 2 classes");
    if (n_cls > AHMC_GLM_CATEGORICAL_MAX_CATEGORIES)
      return no(AHMC_ERR_UNSUPPORTED, "glm_categorical_set_target: n_categories = " + std::to_string(n_cls) +
                                          " is beyond the engine's limit AHMC_GLM_CATEGORICAL_MAX_CATEGORIES = " +
                                          std::to_string(AHMC_GLM_CATEGORICAL_MAX_CATEGORIES));
  }
  if (s.entry == GLM_BY_ORDINAL) {
    if (n_cat < 2) return no(AHMC_ERR_ARGUMENT, "DomainError: n_categories = " + std::to_string(n_cat) + "; an ordered outcome has at least 2 categories");
    if (n_cat > AHMC_GLM_ORDINAL_MAX_CATEGORIES)
      return no(AHMC_ERR_UNSUPPORTED, "glm_ordinal_set_target: n_categories = " + std::to_string(n_cat) +
                                          " is beyond the engine's limit AHMC_GLM_ORDINAL_MAX_CATEGORIES = " + std::to_string(AHMC_GLM_ORDINAL_MAX_CATEGORIES));
    if (!s.cut_prior) return no(AHMC_ERR_ARGUMENT, "glm_ordinal_set_target: cut_prior is NULL");
    for (int i = 0; i < 4; ++i)
      if (!std::isfinite(s.cut_prior[i]) || (i % 2 == 1 && !(s.cut_prior[i] > 0)))
        return no(AHMC_ERR_ARGUMENT, "DomainError: cut_prior[" + std::to_string(i + 1) + "] = " + std::to_string(s.cut_prior[i]) +
                                         (i % 2 == 1 ? " must be finite and > 0 (a scale)" : " must be finite (a location)"));
  }
  // ---- include/ahmc_glm_factor.h: the coefficient rows P = (Px + Σ levels) · blocks
  int64_t P = Px;
  if (s.entry >= GLM_BY_FACTOR) {
    if (F < 0) return no(AHMC_ERR_ARGUMENT, "glm_factor_set_target: n_factors must be >= 0; got " + std::to_string(F));
    if (F > AHMC_GLM_FACTOR_MAX)
      return no(AHMC_ERR_UNSUPPORTED, "glm_factor_set_target: n_factors = " + std::to_string(F) + " is beyond the engine's limit AHMC_GLM_FACTOR_MAX = " +
                                          std::to_string(AHMC_GLM_FACTOR_MAX));
    if (Px < 1) return no(AHMC_ERR_ARGUMENT, "DimensionMismatch: X must keep at least one dense column; n_coef = " + std::to_string((long long)Px));
    if (int rc = n_obs_refusal("glm_factor_set_target")) return rc;  // (before the level indices are read)
    if (F > 0 && (!s.n_levels || !s.levels)) return no(AHMC_ERR_ARGUMENT, "glm_factor_set_target: n_levels or levels is NULL");
    for (int f = 0; f < F; ++f) {
      const int32_t Lf = s.n_levels[f];
      if (Lf < 1) return no(AHMC_ERR_ARGUMENT, "DomainError: factor " + std::to_string(f + 1) + " has n_levels = " + std::to_string(Lf) + "; must be >= 1");
      P += Lf;
      b.L[f] = Lf;
    }
    if (P > INT32_MAX / 2) return no(AHMC_ERR_UNSUPPORTED, "glm_factor_set_target: " + std::to_string((long long)P) + " coefficient rows are beyond 2^30");
    for (int f = 0; f < F; ++f)
      for (int64_t i = 0; i < n_obs; ++i) {
        const int32_t l = s.levels[i + (int64_t)f * n_obs];
        if (l < 0 || l >= s.n_levels[f])
          return no(AHMC_ERR_ARGUMENT, "DomainError: levels[" + std::to_string((long long)i + 1) + ", " + std::to_string(f + 1) + "] = " + std::to_string(l) +
                                           " is outside [0, " + std::to_string(s.n_levels[f]) + ") (zero-based level indices)");
      }
    if (n_cls > 0) P *= n_cls - 1;  // (a categorical model: a block of these rows per non-reference class)
    if (P > INT32_MAX / 2) return no(AHMC_ERR_UNSUPPORTED, "glm_categorical_set_target: " + std::to_string((long long)P) + " coefficient rows are beyond 2^30");
  }
  if (family == AHMC_GLM_ORDERED_LOGIT && n_cat == 0) return no(AHMC_ERR_ARGUMENT, glm_bound_elsewhere(family, aux));  // (whatever D is)
  if (family == AHMC_GLM_CATEGORICAL_LOGIT && n_cls == 0) return no(AHMC_ERR_ARGUMENT, glm_bound_elsewhere(family, aux));
  // ---- include/ahmc_glm_hier.h, include/ahmc_glm_aux.h: the groups against the P rows, θ's rows against the context
  if (s.entry >= GLM_BY_HIER) {
    if (n_groups < 0) return no(AHMC_ERR_ARGUMENT, "hglm_set_target: n_groups must be >= 0; got " + std::to_string(n_groups));
    if (aux && n_groups > AHMC_GLM_AUX_MAX_GROUPS)
      return no(AHMC_ERR_UNSUPPORTED, "glm_aux_set_target: n_groups = " + std::to_string(n_groups) + " is beyond the engine's limit AHMC_GLM_AUX_MAX_GROUPS = " +
                                          std::to_string(AHMC_GLM_AUX_MAX_GROUPS));
    if (n_groups > AHMC_HGLM_MAX_GROUPS)
      return no(AHMC_ERR_UNSUPPORTED, "hglm_set_target: n_groups = " + std::to_string(n_groups) + " is beyond the engine's limit AHMC_HGLM_MAX_GROUPS = " +
                                          std::to_string(AHMC_HGLM_MAX_GROUPS));
    const int n_cut = n_cat > 0 ? n_cat - 1 : 0;
    if (P < 1 || D != P + n_groups + (aux ? 1 : 0) + n_cut)
      return no(AHMC_ERR_ARGUMENT, "DimensionMismatch: the context has D = " + std::to_string((long long)D) + ", the model n_coef + n_groups = " +
                                       std::to_string((long long)P) + " + " + std::to_string(n_groups) + (aux ? " (+ 1: the dispersion's row)" : "") +
                                       (n_cut ? " + " + std::to_string(n_cut) + " (n_categories - 1: the cutpoints' rows)" : "") +
                                       (n_cls > 0 ? " (n_coef: " + std::to_string(n_cls - 1) + " blocks, one per non-reference class, of " +
                                                        std::to_string((long long)(P / (n_cls - 1))) + " rows)"
                                        : F > 0   ? " (n_coef: " + std::to_string((long long)Px) + " columns of X and the factors' levels)"
                                                  : ""));
    if (aux && !std::isfinite(s.aux_loc)) return no(AHMC_ERR_ARGUMENT, "DomainError: aux_loc = " + std::to_string(s.aux_loc) + " must be finite");
    if (aux && !(std::isfinite(s.aux_scale) && s.aux_scale > 0))
      return no(AHMC_ERR_ARGUMENT, "DomainError: aux_scale = " + std::to_string(s.aux_scale) + " must be finite and > 0");
    if (n_groups > 0 && (!s.lo || !s.hi || !s.hyper_scale)) return no(AHMC_ERR_ARGUMENT, "hglm_set_target: lo, hi or hyper_scale is NULL");
    int64_t prev = 0;
    for (int k = 0; k < n_groups; ++k) {
      const int32_t lo = s.lo[k], hi = s.hi[k];
      const std::string grp = "group " + std::to_string(k + 1) + " = [" + std::to_string(lo) + ", " + std::to_string(hi) + ")";
      if (lo < 0 || hi > P) return no(AHMC_ERR_ARGUMENT, "ArgumentError: " + grp + " is out of bounds [0, " + std::to_string((long long)P) + ")");
      if (hi <= lo) return no(AHMC_ERR_ARGUMENT, "ArgumentError: " + grp + " is empty");
      if (lo < prev) return no(AHMC_ERR_ARGUMENT, "ArgumentError: " + grp + " overlaps the group before it or is out of order");
      if (n_cls > 0) {  // a categorical model: inside one class's block, or whole blocks
        const int64_t Pb = P / (n_cls - 1);
        if (lo / Pb != (hi - 1) / Pb && (lo % Pb != 0 || hi % Pb != 0))
          return no(AHMC_ERR_ARGUMENT, "ArgumentError: " + grp + " straddles the classes' blocks of " + std::to_string((long long)Pb) +
                                           " rows: a group lies inside one block or is a union of whole blocks");
      }
      if (!(std::isfinite(s.hyper_scale[k]) && s.hyper_scale[k] > 0))
        return no(AHMC_ERR_ARGUMENT, "DomainError: hyper_scale[" + std::to_string(k + 1) + "] = " + std::to_string(s.hyper_scale[k]) + " must be finite and > 0");
      b.lo[k] = lo;
      b.hi[k] = hi;
      b.centered[k] = s.centered && s.centered[k] ? 1 : 0;
      b.A[k] = s.hyper_scale[k];
      prev = hi;
    }
  }
  // ---- include/ahmc_glm.h
  if (glm_aux_family(family) && !aux)
    return no(AHMC_ERR_ARGUMENT, "set_target_glm: unknown family " + std::to_string(family) +
                                     " at this entry point: it samples its dispersion and is bound through ahmc_glm_aux_set_target (include/ahmc_glm_aux.h)");
  if (aux && !glm_aux_family(family))
    return no(AHMC_ERR_ARGUMENT, "glm_aux_set_target: family " + std::to_string(family) +
                                     " has no sampled dispersion (AHMC_GLM_GAUSSIAN_IDENTITY_SIGMA, AHMC_GLM_NEGBINOMIAL_LOG)");
  if (!aux && n_cat == 0 && n_cls == 0 && family != AHMC_GLM_BERNOULLI_LOGIT && family != AHMC_GLM_POISSON_LOG && family != AHMC_GLM_GAUSSIAN_IDENTITY)
    return no(AHMC_ERR_ARGUMENT, "set_target_glm: unknown family " + std::to_string(family));
  if (s.entry < GLM_BY_FACTOR)
    if (int rc = n_obs_refusal("set_target_glm")) return rc;
  if (!s.X || !s.y) return no(AHMC_ERR_ARGUMENT, "set_target_glm: X or y is NULL");
  if (!(std::isfinite(s.scale) && s.scale > 0)) return no(AHMC_ERR_ARGUMENT, "set_target_glm: scale must be finite and > 0; got " + std::to_string(s.scale));
  // ---- the checked copy
  b.family = family;
  b.n_obs = n_obs;
  b.has_offset = s.offset != nullptr;
  b.scale = s.scale;
  b.P = P;
  b.Px = Px;
  b.F = s.entry >= GLM_BY_FACTOR ? F : 0;
  b.G = s.entry >= GLM_BY_HIER ? n_groups : 0;
  b.bound_hier = s.entry != GLM_BY_PLAIN;
  b.aux = aux;
  if (aux) {
    b.aux_loc = s.aux_loc;
    b.aux_scale = s.aux_scale;
  }
  b.n_cat = n_cat;
  if (n_cat > 0)
    for (int i = 0; i < 4; ++i) b.cut_prior[i] = s.cut_prior[i];
  b.n_cls = n_cls;
  const int64_t K = b.K();
  b.Lt = P / K - Px;  // (the factors' levels together — of one block, where the model has K blocks)
  // ---- the slab: X, Xᵀ, y, offset, p [, a zero precision, the group table], then the workspaces U, partial [, partial_s], gs [, W, R].
  // A categorical model: offset K·n_obs, U K·n_obs·N (a plane per class), p / W / R over its P = K·Pb rows
  const int64_t nrb = (n_obs + GLM_SPEC_ROW_BLOCK - 1) / GLM_SPEC_ROW_BLOCK, ns = (n_obs + GLM_SPEC_K_SLICE - 1) / GLM_SPEC_K_SLICE;
  int64_t sizes[GLM_PARTS] = {};
  sizes[GLM_X] = sizes[GLM_XT] = n_obs * Px;
  sizes[GLM_Y] = n_obs;
  sizes[GLM_OFF] = n_obs * K;
  sizes[GLM_PREC] = P;
  sizes[GLM_U] = n_obs * N * K;
  sizes[GLM_PART] = nrb * N;
  sizes[GLM_GS] = ns > 1 ? ns * Px * N : 0;
  sizes[GLM_PART_S] = aux ? nrb * N : 0;
  sizes[GLM_CUT] = n_cat > 0 ? 3 * (int64_t)(n_cat - 1) * N : 0;
  sizes[GLM_PART_C] = n_cat > 0 ? (int64_t)(n_cat - 1) * nrb * N : 0;
  if (b.on_w()) {
    sizes[GLM_W] = sizes[GLM_R] = P * N;
    sizes[GLM_ZERO] = P;
    sizes[GLM_TAB] = (int64_t)((sizeof(Tab) + sizeof(T) - 1) / sizeof(T));
  }
  const auto int_elems = [](int64_t n_ints) { return (int64_t)((n_ints * sizeof(int) + sizeof(T) - 1) / sizeof(T)); };  // int32 parts, in elements
  if (b.F > 0) {
    sizes[GLM_FTAB] = int_elems((int64_t)(sizeof(FTab) / sizeof(int)));
    sizes[GLM_LEV] = sizes[GLM_PERM] = int_elems(n_obs * b.F);
    sizes[GLM_RP] = int_elems(b.Lt + 1);
  }
  const int layout[GLM_PARTS] = {GLM_X,    GLM_XT, GLM_Y, GLM_OFF,  GLM_PREC,   GLM_ZERO, GLM_TAB, GLM_FTAB, GLM_LEV,
                                 GLM_PERM, GLM_RP, GLM_U, GLM_PART, GLM_PART_S, GLM_GS,   GLM_W,   GLM_R,    GLM_CUT, GLM_PART_C};
  b.total = 0;
  for (int i : layout) {
    b.off[i] = b.total;
    b.total += (sizes[i] + 1) / 2 * 2;  // (16-byte alignment of every part, Float32 included)
  }
  b.n_data = b.off[GLM_U];
  return AHMC_OK;
}

// Step 3 of glm_bind.  h: the first b.n_data elements of the slab on the host, zero but for X, y, offset and prior_prec, which the
// caller staged at their offsets.  Checks the data, then fills in the group table, Xᵀ, the factor table, the level indices, per factor
// the stable permutation of the observations by level and the row pointers of all levels together.
template <class T, class Tab, class FTab>
int glm_spec_build(const GlmSpec& s, const GlmBound& b, T* h, std::string& err) {
  const auto no = [&err](const std::string& msg) {
    err = msg;
    return (int)AHMC_ERR_ARGUMENT;
  };
  const int64_t* const off = b.off;
  const int64_t n_obs = b.n_obs, Px = b.Px;
  const int family = b.family, K = b.K();
  const T* hX = h + off[GLM_X];
  for (int64_t i = 0; i < n_obs * Px; ++i)
    if (!std::isfinite((double)hX[i])) return no("ArgumentError: X holds a non-finite value");
  for (int64_t i = n_obs; i < n_obs * K; ++i)  // (the offset's columns of the classes after the first)
    if (!std::isfinite((double)h[off[GLM_OFF] + i])) return no("ArgumentError: offset holds a non-finite value");
  const int n_int = b.n_cat > 0 ? b.n_cat : b.n_cls;  // y holds a category or a class
  for (int64_t i = 0; i < n_obs; ++i) {
    const double yi = (double)h[off[GLM_Y] + i];
    if (!std::isfinite((double)h[off[GLM_OFF] + i])) return no("ArgumentError: offset holds a non-finite value");
    const bool counts = family == AHMC_GLM_POISSON_LOG || family == AHMC_GLM_NEGBINOMIAL_LOG;
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
  for (int64_t d = 0; d < b.P; ++d) {
    const double pd = (double)h[off[GLM_PREC] + d];
    if (!std::isfinite(pd)) return no("ArgumentError: prior_prec holds a non-finite value");
    if (pd < 0) return no("DomainError: prior_prec[" + std::to_string(d + 1) + "] = " + std::to_string(pd) + " is negative");
  }
  if (b.on_w()) {
    Tab tab{};
    for (int k = 0; k < b.G; ++k) {
      for (int64_t d = b.lo[k]; d < b.hi[k]; ++d)
        if ((double)h[off[GLM_PREC] + d] != 0)
          return no("ArgumentError: prior_prec[" + std::to_string(d + 1) + "] must be 0: the coefficient is a member of group " + std::to_string(k + 1));
      tab.lo[k] = b.lo[k];
      tab.hi[k] = b.hi[k];
      tab.centered[k] = b.centered[k];
      tab.inv_a2[k] = (T)(1.0 / (b.A[k] * b.A[k]));
    }
    memcpy(h + off[GLM_TAB], &tab, sizeof(tab));
  }
  T* hXt = h + off[GLM_XT];
  for (int64_t d = 0; d < Px; ++d)
    for (int64_t i = 0; i < n_obs; ++i) hXt[d + i * Px] = hX[i + d * n_obs];
  if (b.F > 0) {
    FTab ft{};
    int* lev = reinterpret_cast<int*>(h + off[GLM_LEV]);
    int* perm = reinterpret_cast<int*>(h + off[GLM_PERM]);
    int* rp = reinterpret_cast<int*>(h + off[GLM_RP]);
    ft.F = b.F;
    int64_t row = Px, q0 = 0;
    for (int f = 0; f < b.F; ++f) {
      const int Lf = b.L[f];
      ft.off[f] = (int)row;
      ft.L[f] = Lf;
      const int32_t* lf = s.levels + (int64_t)f * n_obs;
      std::vector<int64_t> cnt((size_t)Lf + 1, 0);  // a counting sort: ascending observations within a level
      for (int64_t i = 0; i < n_obs; ++i) {
        lev[i + f * n_obs] = lf[i];
        ++cnt[(size_t)lf[i] + 1];
      }
      for (int l = 0; l < Lf; ++l) cnt[(size_t)l + 1] += cnt[(size_t)l];
      for (int l = 0; l <= Lf; ++l) rp[q0 + l] = (int)((int64_t)f * n_obs + cnt[(size_t)l]);
      for (int64_t i = 0; i < n_obs; ++i) perm[(int64_t)f * n_obs + cnt[(size_t)lf[i]]++] = (int)i;
      row += Lf;
      q0 += Lf;
    }
    memcpy(h + off[GLM_FTAB], &ft, sizeof(ft));
  }
  return AHMC_OK;
}

}  // namespace ahmc
