// ahmc_glm_host.hpp — host side of the generalised-linear-model target (include/ahmc_glm.h; kernels: ahmc_glm.hpp) and of its
// hierarchical form (include/ahmc_glm_hier.h: coefficient groups whose prior scale is sampled) and of the families with a sampled
// dispersion (include/ahmc_glm_aux.h).  Included by ahmc_api.hip after the
// context, before ahmc_dense_host.hpp, whose dn_other_target routes to glm_target.
#pragma once

// the targets that fill lp and g for a LIST of chains from th, on the step-synchronous engine: the user's kernel and the GLM
template <class T>
bool listed_target(const Ctx<T>* c) {
  return c->target_kind == AHMC_TARGET_KERNEL || c->target_kind == AHMC_TARGET_GLM;
}

// a hierarchical model's groups as ahmc_hglm_set_target received them (n_groups may be 0: the plain model)
struct HglmSpec {
  int64_t P;
  int G;
  const int32_t *lo, *hi, *centered;
  const double* A;
  bool aux = false;  // ahmc_glm_aux_set_target: θ ends with s, the log dispersion, with the prior Normal(aux_loc, aux_scale²)
  double aux_loc = 0, aux_scale = 1;
  // ahmc_glm_factor_set_target: P = Px + Σ n_levels; levels (n_obs, F) column-major, zero-based (host memory)
  int F = 0;
  int64_t Px = 0;
  const int32_t *n_levels = nullptr, *levels = nullptr;
  // ahmc_glm_ordinal_set_target: C categories, θ ends with the C − 1 rows κ; cut_prior = (loc_1, scale_1, loc_gap, scale_gap)
  int n_cat = 0;
  const double* cut_prior = nullptr;
  // ahmc_glm_categorical_set_target: C classes, K = C − 1 coefficient blocks of Px + Σ n_levels rows each (P = K blocks)
  int n_cls = 0;
};

inline bool glm_aux_family(int family) { return family == AHMC_GLM_GAUSSIAN_IDENTITY_SIGMA || family == AHMC_GLM_NEGBINOMIAL_LOG; }

// what the entry points of the older headers answer to AHMC_GLM_ORDERED_LOGIT
inline std::string glm_ordinal_elsewhere(int family, bool aux) {
  const std::string where = "it samples its cutpoints and is bound through ahmc_glm_ordinal_set_target (include/ahmc_glm_ordinal.h)";
  if (aux)
    return "glm_aux_set_target: family " + std::to_string(family) +
           " has no sampled dispersion (AHMC_GLM_GAUSSIAN_IDENTITY_SIGMA, AHMC_GLM_NEGBINOMIAL_LOG): " + where;
  return "set_target_glm: unknown family " + std::to_string(family) + " at this entry point: " + where;
}

// … and to AHMC_GLM_CATEGORICAL_LOGIT
inline std::string glm_categorical_elsewhere(int family, bool aux) {
  const std::string where = "it has a coefficient block per class and is bound through ahmc_glm_categorical_set_target (include/ahmc_glm_categorical.h)";
  if (aux)
    return "glm_aux_set_target: family " + std::to_string(family) +
           " has no sampled dispersion (AHMC_GLM_GAUSSIAN_IDENTITY_SIGMA, AHMC_GLM_NEGBINOMIAL_LOG): " + where;
  return "set_target_glm: unknown family " + std::to_string(family) + " at this entry point: " + where;
}

template <class T>
int glm_slices(const Ctx<T>* c) {
  return (int)((c->glm.n_obs + GLM_K_SLICE - 1) / GLM_K_SLICE);
}

// drop the model's buffers (another target takes over; the stream is made idle first)
template <class T>
int glm_release(Ctx<T>* c) {
  if (!c->glm.buf) return AHMC_OK;
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipFree(c->glm.buf));
  c->glm = {};
  return AHMC_OK;
}

// η (and from it U, partial; on request η and ℓ themselves) for ncols listed chains; th: the coefficients, (D, N) with column stride D.
// A model with factors: the product over its Px dense columns, the factors' rows of th gathered in the epilogue (k_glm_eta_f).
// theta: the (D_θ, ·) array whose last row is the dispersion (default: the context's θ; ahmc_glm_loglik: a chunk of the caller's draws).
template <class T>
int glm_launch_eta(Ctx<T>* c, const T* th, int D, const int* list, int64_t ncols, bool small, T* eta_out, T* ll_out, const T* theta = nullptr) {
  const GlmModel<T>& m = c->glm;
  const int n_obs = (int)m.n_obs;
  const int64_t nrb = (n_obs + GB_M - 1) / GB_M;
  const T* X = m.at(GLM_X);
  const T* y = m.at(GLM_Y);
  const T* off = m.has_offset ? m.at(GLM_OFF) : nullptr;
  T* U = m.at(GLM_U);
  T* part = m.at(GLM_PART);
  // a sampled dispersion: s is row D − 1 of the chain's own θ (th holds W); Σ ∂ℓ/∂s per row block
  const T* aux = m.aux ? (theta ? theta : (const T*)c->th) + (c->D - 1) : nullptr;
  T* part_s = m.aux ? m.at(GLM_PART_S) : nullptr;
  if (glm_aux_family(m.family) != m.aux) return fail(c, AHMC_ERR_STATE, "glm: the family and the dispersion row disagree in the context");
  if ((m.family == AHMC_GLM_ORDERED_LOGIT) != (m.n_cat > 0)) return fail(c, AHMC_ERR_STATE, "glm: the family and the cutpoint rows disagree in the context");
  // an ordinal model: the cutpoint table k_glm_cut made, C − 1, and partial_c take the places of s, its stride and partial_s
  int64_t aux_ld = c->D;
  if (m.n_cat > 0) {
    aux = m.at(GLM_CUT);
    aux_ld = m.n_cat - 1;
    part_s = m.at(GLM_PART_C);
  }
  const dim3 grid = small ? dim3((unsigned)nrb, (unsigned)((ncols + 15) / 16)) : dim3((unsigned)(nrb * (((ncols + GB_N - 1) / GB_N + 7) / 8 * 8)));
#define AHMC_GLM_ETA(FAM, BN) \
  hipLaunchKernelGGL((k_glm_eta<T, FAM, BN>), grid, dim3(256), 0, c->stream, X, y, off, (T)m.scale, th, U, part, n_obs, D, ncols, c->N, list, eta_out, ll_out, aux, aux_ld, part_s)
#define AHMC_GLM_ETA_F(FAM, BN)                                                                                                                          \
  hipLaunchKernelGGL((k_glm_eta_f<T, FAM, BN>), grid, dim3(256), 0, c->stream, X, y, off, (T)m.scale, th, U, part, n_obs, (int)m.Px, (int64_t)D, ncols, c->N, list, \
                     eta_out, ll_out, aux, aux_ld, part_s, m.ftab(), m.ints(GLM_LEV))
  if (m.F > 0) {
    if (D != m.P) return fail(c, AHMC_ERR_STATE, "glm: a model with factors runs on its P rows of W");
    switch (m.family * 2 + (small ? 1 : 0)) {
      case 0: AHMC_GLM_ETA_F(0, 64); break;
      case 1: AHMC_GLM_ETA_F(0, 16); break;
      case 2: AHMC_GLM_ETA_F(1, 64); break;
      case 3: AHMC_GLM_ETA_F(1, 16); break;
      case 4: AHMC_GLM_ETA_F(2, 64); break;
      case 5: AHMC_GLM_ETA_F(2, 16); break;
      case 6: AHMC_GLM_ETA_F(3, 64); break;
      case 7: AHMC_GLM_ETA_F(3, 16); break;
      case 8: AHMC_GLM_ETA_F(4, 64); break;
      case 9: AHMC_GLM_ETA_F(4, 16); break;
      case 10: AHMC_GLM_ETA_F(5, 64); break;
      case 11: AHMC_GLM_ETA_F(5, 16); break;
      default: return fail(c, AHMC_ERR_STATE, "glm: unknown family in the context");
    }
    HIPCHK(hipGetLastError());
    return AHMC_OK;
  }
#undef AHMC_GLM_ETA_F
  switch (m.family * 2 + (small ? 1 : 0)) {
    case 0: AHMC_GLM_ETA(0, 64); break;
    case 1: AHMC_GLM_ETA(0, 16); break;
    case 2: AHMC_GLM_ETA(1, 64); break;
    case 3: AHMC_GLM_ETA(1, 16); break;
    case 4: AHMC_GLM_ETA(2, 64); break;
    case 5: AHMC_GLM_ETA(2, 16); break;
    case 6: AHMC_GLM_ETA(3, 64); break;
    case 7: AHMC_GLM_ETA(3, 16); break;
    case 8: AHMC_GLM_ETA(4, 64); break;
    case 9: AHMC_GLM_ETA(4, 16); break;
    case 10: AHMC_GLM_ETA(5, 64); break;
    case 11: AHMC_GLM_ETA(5, 16); break;
    default: return fail(c, AHMC_ERR_STATE, "glm: unknown family in the context");
  }
#undef AHMC_GLM_ETA
  HIPCHK(hipGetLastError());
  return AHMC_OK;
}

// a categorical model (include/ahmc_glm_categorical.h): the K predictors of ncols listed chains from W (P = K·Pb rows a column) into
// the K planes of U, turned into u_k in place, and Σℓ per row block into partial; on request η (K planes), ℓ and the class
// probabilities (C, n_obs, ncols; then without a chain list)
template <class T>
int glm_launch_eta_cat(Ctx<T>* c, const T* W, const int* list, int64_t ncols, bool small, T* eta_out, T* ll_out, T* prob_out) {
  const GlmModel<T>& m = c->glm;
  if (m.family != AHMC_GLM_CATEGORICAL_LOGIT || m.n_cls < 2) return fail(c, AHMC_ERR_STATE, "glm: the family and the class count disagree in the context");
  if (prob_out && list) return fail(c, AHMC_ERR_STATE, "glm: class probabilities are made without a chain list");
  const int n_obs = (int)m.n_obs, K = m.n_cls - 1, Pb = (int)(m.P / K);
  const int64_t nrb = (n_obs + GB_M - 1) / GB_M;
  const T* off = m.has_offset ? m.at(GLM_OFF) : nullptr;
  const dim3 grid = small ? dim3((unsigned)nrb, (unsigned)((ncols + 15) / 16)) : dim3((unsigned)(nrb * (((ncols + GB_N - 1) / GB_N + 7) / 8 * 8)));
#define AHMC_GLM_ETA_CAT(BN, FAC)                                                                                                                              \
  hipLaunchKernelGGL((k_glm_eta_cat<T, BN, FAC>), grid, dim3(256), 0, c->stream, (const T*)m.at(GLM_X), (const T*)m.at(GLM_Y), off, W, m.at(GLM_U), m.at(GLM_PART), \
                     n_obs, (int)m.Px, Pb, K, (int64_t)m.P, ncols, c->N, list, eta_out, ll_out, prob_out, m.F > 0 ? m.ftab() : (const GlmFacTab*)nullptr,           \
                     m.F > 0 ? m.ints(GLM_LEV) : (const int*)nullptr)
  if (m.F > 0) {
    if (small) AHMC_GLM_ETA_CAT(16, true);
    else AHMC_GLM_ETA_CAT(64, true);
  } else {
    if (small) AHMC_GLM_ETA_CAT(16, false);
    else AHMC_GLM_ETA_CAT(64, false);
  }
#undef AHMC_GLM_ETA_CAT
  HIPCHK(hipGetLastError());
  return AHMC_OK;
}

// an ordinal model's cutpoint table (c, lg, r) of the listed chains from the κ rows of the context's θ (or of `theta`, a chunk of the
// caller's draws), before k_glm_eta
template <class T>
void glm_launch_cut(Ctx<T>* c, const int* list, int64_t n, const T* theta = nullptr) {
  const GlmModel<T>& m = c->glm;
  hipLaunchKernelGGL((k_glm_cut<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, theta ? theta : (const T*)c->th, c->D, c->D - (m.n_cat - 1), m.n_cat - 1,
                     m.at(GLM_CUT), c->N, n, list, 1);
}

// few columns: the 64×16 tiles put 4× as many workgroups on the chip (dn_gemm's rule; same arithmetic per column, so the
// results do not depend on the choice).  AHMC_GLM_SMALL_BELOW overrides the threshold (0: never, a large value: always), read at
// every call so that a test can switch it.
template <class T>
bool glm_small(const Ctx<T>* c, int64_t row_blocks, int64_t ncols) {
  const char* e = getenv("AHMC_GLM_SMALL_BELOW");
  const int64_t small_below = e ? atoll(e) : 1;
  if ((ncols + 15) / 16 > 65535) return false;  // (grid.y)
  return (double)row_blocks * (double)((ncols + GB_N - 1) / GB_N) < (double)small_below * (double)c->n_cu;
}

// AHMC_TARGET_GLM: (ℓπ, g = −∇ℓπ) at θ of the listed chains — dn_user_target's contract: reads c->th, writes c->lp and c->g on the
// context's stream
template <class T>
int glm_target(Ctx<T>* c, const int* list, int64_t n, bool sanitize_lp = true) {
  if (n <= 0) return AHMC_OK;
  const GlmModel<T>& m = c->glm;
  if (!m.buf) return fail(c, AHMC_ERR_STATE, "AHMC_TARGET_GLM without a model (ahmc_set_target_glm)");
  // groups or a dispersion bound: the products run on the effective coefficients W (P, N) with a zero precision and leave
  // R = −Xᵀu; k_hglm_coef before them and k_hglm_finish after them are the model (ahmc_glm.hpp)
  const bool hier = m.on_w();
  // factors: the dense product covers rows [0, Px) of R, k_glm_fgrad the factors' rows; W and R keep the column stride P
  const int n_obs = (int)m.n_obs, D = (int)m.P, Px = (int)m.Px, G = m.G, ns = glm_slices(c);
  const int64_t nrb = (n_obs + GB_M - 1) / GB_M, nrbD = (int64_t)(Px + GB_M - 1) / GB_M * ns;
  const T* th = hier ? m.at(GLM_W) : (const T*)c->th;
  const T* prec = m.at(hier ? GLM_ZERO : GLM_PREC);
  T* g = hier ? m.at(GLM_R) : c->g;
  if (hier) hipLaunchKernelGGL((k_hglm_coef<T>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, (const T*)c->th, m.tab(), m.at(GLM_W), (T*)nullptr, D, G, c->D, n, list);
  if (m.n_cat > 0) glm_launch_cut(c, list, n);
  int rc = m.n_cls > 0 ? glm_launch_eta_cat(c, th, list, n, glm_small(c, nrb, n), (T*)nullptr, (T*)nullptr, (T*)nullptr)
                       : glm_launch_eta(c, th, D, list, n, glm_small(c, nrb, n), (T*)nullptr, (T*)nullptr);
  if (rc) return rc;
  const T* Xt = m.at(GLM_XT);
  const T* U = m.at(GLM_U);
  T* gs = m.at(GLM_GS);
  const dim3 grid16((unsigned)nrbD, (unsigned)((n + 15) / 16)), grid64((unsigned)(nrbD * (((n + GB_N - 1) / GB_N + 7) / 8 * 8)));
  if (m.n_cls > 0) {
    // per class k: rows [k·Pb, (k + 1)·Pb) of R = −Xᵀu_k from plane k of U, by the kernels of a model with factors (column stride P);
    // the slice workspace is reused stream-ordered
    const int K = m.n_cls - 1, Pb = D / K;
    const bool small = glm_small(c, nrbD, n);
    for (int k = 0; k < K; ++k) {
      const T* Uk = U + (int64_t)k * n_obs * c->N;
      const T* Wk = th + (int64_t)k * Pb;
      T* Rk = g + (int64_t)k * Pb;
      if (small)
        hipLaunchKernelGGL((k_glm_grad_ld<T, 16>), grid16, dim3(256), 0, c->stream, Xt, Uk, prec, Wk, Rk, gs, n_obs, Px, (int64_t)D, n, c->N, list, ns);
      else
        hipLaunchKernelGGL((k_glm_grad_ld<T, 64>), grid64, dim3(256), 0, c->stream, Xt, Uk, prec, Wk, Rk, gs, n_obs, Px, (int64_t)D, n, c->N, list, ns);
      if (ns > 1)
        hipLaunchKernelGGL((k_glm_gsum_ld<T>), dim3((unsigned)((n * Px + 255) / 256)), dim3(256), 0, c->stream, (const T*)gs, prec, Wk, Rk, Px, (int64_t)D, n, c->N,
                           list, ns);
      if (m.F > 0)
        hipLaunchKernelGGL((k_glm_fgrad<T>), dim3((unsigned)((n * m.Lt + 255) / 256)), dim3(256), 0, c->stream, Uk, m.ints(GLM_PERM), m.ints(GLM_RP), Rk, n_obs, Px,
                           (int)m.Lt, (int64_t)D, n, list);
    }
  } else if (m.F > 0) {
    if (glm_small(c, nrbD, n))
      hipLaunchKernelGGL((k_glm_grad_ld<T, 16>), grid16, dim3(256), 0, c->stream, Xt, U, prec, th, g, gs, n_obs, Px, (int64_t)D, n, c->N, list, ns);
    else
      hipLaunchKernelGGL((k_glm_grad_ld<T, 64>), grid64, dim3(256), 0, c->stream, Xt, U, prec, th, g, gs, n_obs, Px, (int64_t)D, n, c->N, list, ns);
    if (ns > 1)
      hipLaunchKernelGGL((k_glm_gsum_ld<T>), dim3((unsigned)((n * Px + 255) / 256)), dim3(256), 0, c->stream, (const T*)gs, prec, th, g, Px, (int64_t)D, n, c->N,
                         list, ns);
    hipLaunchKernelGGL((k_glm_fgrad<T>), dim3((unsigned)((n * m.Lt + 255) / 256)), dim3(256), 0, c->stream, U, m.ints(GLM_PERM), m.ints(GLM_RP), g, n_obs, Px,
                       (int)m.Lt, (int64_t)D, n, list);
  } else {
    if (glm_small(c, nrbD, n))
      hipLaunchKernelGGL((k_glm_grad<T, 16>), grid16, dim3(256), 0, c->stream, Xt, U, prec, th, g, gs, n_obs, D, n, c->N, list, ns);
    else
      hipLaunchKernelGGL((k_glm_grad<T, 64>), grid64, dim3(256), 0, c->stream, Xt, U, prec, th, g, gs, n_obs, D, n, c->N, list, ns);
    if (ns > 1)
      hipLaunchKernelGGL((k_glm_gsum<T>), dim3((unsigned)((n * D + 255) / 256)), dim3(256), 0, c->stream, (const T*)gs, prec, th, g, D, n, c->N, list, ns);
  }
  if (m.n_cat > 0) {
    const double* q = m.cut_prior;
    hipLaunchKernelGGL((k_hglm_finish_ord<T>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, (const T*)m.at(GLM_PART), (const T*)m.at(GLM_PART_C),
                       (const T*)g, th, (const T*)m.at(GLM_PREC), (const T*)c->th, m.tab(), c->lp, c->g, (int)nrb, D, G, n, c->N, list, sanitize_lp ? 1 : 0,
                       m.n_cat - 1, q[0], 1.0 / (q[1] * q[1]), q[2], 1.0 / (q[3] * q[3]));
  } else if (m.aux)
    hipLaunchKernelGGL((k_hglm_finish_aux<T>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, (const T*)m.at(GLM_PART), (const T*)m.at(GLM_PART_S),
                       (const T*)g, th, (const T*)m.at(GLM_PREC), (const T*)c->th, m.tab(), c->lp, c->g, (int)nrb, D, G, n, c->N, list, sanitize_lp ? 1 : 0,
                       (T)m.aux_loc, (T)(1.0 / (m.aux_scale * m.aux_scale)));
  else if (hier)
    hipLaunchKernelGGL((k_hglm_finish<T>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, (const T*)m.at(GLM_PART), (const T*)g, th,
                       (const T*)m.at(GLM_PREC), (const T*)c->th, m.tab(), c->lp, c->g, (int)nrb, D, G, n, c->N, list, sanitize_lp ? 1 : 0);
  else
    hipLaunchKernelGGL((k_glm_lp<T>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, (const T*)m.at(GLM_PART), prec, th, c->lp, (int)nrb, D, n, c->N, list,
                       sanitize_lp ? 1 : 0);
  HIPCHK(hipGetLastError());
  return AHMC_OK;
}

template <class T>
int glm_set(Ctx<T>* c, int family, int64_t n_obs, const T* X, const T* y, const T* offset, const T* prec, double scale, const HglmSpec* hs = nullptr) {
  const int G = hs ? hs->G : 0;
  const int n_cat = hs ? hs->n_cat : 0;  // (> 0: checked by glm_ordinal_set)
  const int n_cls = hs ? hs->n_cls : 0;  // (> 0: checked by glm_categorical_set)
  const int K = n_cls > 0 ? n_cls - 1 : 1;  // predictors per observation: the planes of U, the columns of offset
  const bool aux = hs && hs->aux, on_w = G > 0 || aux || (hs && hs->F > 0) || n_cat > 0 || n_cls > 0;
  const int64_t D = hs ? hs->P : c->D, N = c->N;  // (the coefficient rows: the record's P)
  const int F = hs ? hs->F : 0;
  // (the columns of X; the factors' levels together — of one block, where the model has K blocks)
  const int64_t Px = F > 0 || n_cls > 0 ? hs->Px : D, Lt = (n_cls > 0 ? D / K : D) - Px;
  if (family == AHMC_GLM_ORDERED_LOGIT && n_cat == 0) return fail(c, AHMC_ERR_ARGUMENT, glm_ordinal_elsewhere(family, aux));
  if (family == AHMC_GLM_CATEGORICAL_LOGIT && n_cls == 0) return fail(c, AHMC_ERR_ARGUMENT, glm_categorical_elsewhere(family, aux));
  if (glm_aux_family(family) && !aux)
    return fail(c, AHMC_ERR_ARGUMENT, "set_target_glm: unknown family " + std::to_string(family) +
                                          " at this entry point: it samples its dispersion and is bound through ahmc_glm_aux_set_target (include/ahmc_glm_aux.h)");
  if (aux && !glm_aux_family(family))
    return fail(c, AHMC_ERR_ARGUMENT, "glm_aux_set_target: family " + std::to_string(family) +
                                          " has no sampled dispersion (AHMC_GLM_GAUSSIAN_IDENTITY_SIGMA, AHMC_GLM_NEGBINOMIAL_LOG)");
  if (!aux && n_cat == 0 && n_cls == 0 && family != AHMC_GLM_BERNOULLI_LOGIT && family != AHMC_GLM_POISSON_LOG && family != AHMC_GLM_GAUSSIAN_IDENTITY)
    return fail(c, AHMC_ERR_ARGUMENT, "set_target_glm: unknown family " + std::to_string(family));
  if (n_obs < 1) return fail(c, AHMC_ERR_ARGUMENT, "set_target_glm: n_obs must be >= 1; got " + std::to_string(n_obs));
  if (n_obs > AHMC_GLM_MAX_OBS)
    return fail(c, AHMC_ERR_UNSUPPORTED, "set_target_glm: n_obs = " + std::to_string(n_obs) + " is beyond the engine's limit AHMC_GLM_MAX_OBS = " +
                                             std::to_string((long long)AHMC_GLM_MAX_OBS));
  if (!X || !y) return fail(c, AHMC_ERR_ARGUMENT, "set_target_glm: X or y is NULL");
  if (!(std::isfinite(scale) && scale > 0)) return fail(c, AHMC_ERR_ARGUMENT, "set_target_glm: scale must be finite and > 0; got " + std::to_string(scale));
  // the slab: X, Xᵀ, y, offset, p [, a zero precision, the group table], then the workspaces U, partial [, partial_s], gs [, W, R].
  // A categorical model: offset K·n_obs, U K·n_obs·N (a plane per class), p / W / R over its P = K·Pb rows
  const int64_t nrb = (n_obs + GB_M - 1) / GB_M, ns = (n_obs + GLM_K_SLICE - 1) / GLM_K_SLICE;
  const int64_t tab_elems = (int64_t)((sizeof(HglmTab<T>) + sizeof(T) - 1) / sizeof(T));
  int64_t sizes[GLM_PARTS] = {n_obs * Px, n_obs * Px, n_obs, n_obs * K, D, n_obs * N * K, nrb * N, ns > 1 ? ns * Px * N : 0, 0, 0, 0, 0, aux ? nrb * N : 0, 0, 0, 0, 0,
                              n_cat > 0 ? 3 * (int64_t)(n_cat - 1) * N : 0, n_cat > 0 ? (int64_t)(n_cat - 1) * nrb * N : 0};
  if (on_w) {
    sizes[GLM_W] = sizes[GLM_R] = D * N;
    sizes[GLM_ZERO] = D;
    sizes[GLM_TAB] = tab_elems;
  }
  const auto int_elems = [](int64_t n_ints) { return (int64_t)((n_ints * sizeof(int) + sizeof(T) - 1) / sizeof(T)); };  // int32 parts, in elements
  if (F > 0) {
    sizes[GLM_FTAB] = int_elems((int64_t)(sizeof(GlmFacTab) / sizeof(int)));
    sizes[GLM_LEV] = sizes[GLM_PERM] = int_elems(n_obs * F);
    sizes[GLM_RP] = int_elems(Lt + 1);
  }
  const int layout[GLM_PARTS] = {GLM_X,   GLM_XT, GLM_Y,    GLM_OFF,    GLM_PREC, GLM_ZERO, GLM_TAB, GLM_FTAB, GLM_LEV,
                                 GLM_PERM, GLM_RP, GLM_U,    GLM_PART,   GLM_PART_S, GLM_GS,  GLM_W,   GLM_R,   GLM_CUT, GLM_PART_C};
  GlmModel<T> m;  // (becomes the context's once nothing can fail any more)
  int64_t* const off = m.off;
  int64_t total = 0;
  for (int i : layout) {
    off[i] = total;
    total += (sizes[i] + 1) / 2 * 2;  // (16-byte alignment of every part, Float32 included)
  }
  const int64_t n_data = off[GLM_U];
  std::vector<T> h((size_t)n_data, T(0));
  HIPCHK(hipMemcpy(h.data() + off[GLM_X], X, sizeof(T) * n_obs * Px, hipMemcpyDefault));
  HIPCHK(hipMemcpy(h.data() + off[GLM_Y], y, sizeof(T) * n_obs, hipMemcpyDefault));
  if (offset) HIPCHK(hipMemcpy(h.data() + off[GLM_OFF], offset, sizeof(T) * n_obs * K, hipMemcpyDefault));
  if (prec) HIPCHK(hipMemcpy(h.data() + off[GLM_PREC], prec, sizeof(T) * D, hipMemcpyDefault));
  const T* hX = h.data() + off[GLM_X];
  for (int64_t i = 0; i < n_obs * Px; ++i)
    if (!std::isfinite((double)hX[i])) return fail(c, AHMC_ERR_ARGUMENT, "ArgumentError: X holds a non-finite value");
  for (int64_t i = n_obs; i < n_obs * K; ++i)  // (the offset's columns of the classes after the first)
    if (!std::isfinite((double)h[off[GLM_OFF] + i])) return fail(c, AHMC_ERR_ARGUMENT, "ArgumentError: offset holds a non-finite value");
  const int n_int = n_cat > 0 ? n_cat : n_cls;  // y holds a category or a class
  for (int64_t i = 0; i < n_obs; ++i) {
    const double yi = (double)h[off[GLM_Y] + i];
    if (!std::isfinite((double)h[off[GLM_OFF] + i])) return fail(c, AHMC_ERR_ARGUMENT, "ArgumentError: offset holds a non-finite value");
    const bool counts = family == AHMC_GLM_POISSON_LOG || family == AHMC_GLM_NEGBINOMIAL_LOG;
    const bool ok = n_int > 0                            ? (yi >= 0 && yi < n_int && yi == std::floor(yi))
                    : family == AHMC_GLM_BERNOULLI_LOGIT ? (yi >= 0 && yi <= 1)
                    : counts                             ? (std::isfinite(yi) && yi >= 0)
                                                         : std::isfinite(yi);
    if (!ok && n_int > 0)
      return fail(c, AHMC_ERR_ARGUMENT, "DomainError: y[" + std::to_string(i + 1) + "] = " + std::to_string(yi) + " is not a category: an integer in [0, " +
                                            std::to_string(n_int) + ")");
    if (!ok)
      return fail(c, AHMC_ERR_ARGUMENT, "DomainError: y[" + std::to_string(i + 1) + "] = " + std::to_string(yi) + " is outside the family's domain (" +
                                            (family == AHMC_GLM_BERNOULLI_LOGIT ? "0 <= y <= 1" : counts ? "y >= 0, finite" : "finite") + ")");
  }
  for (int64_t d = 0; d < D; ++d) {
    const double pd = (double)h[off[GLM_PREC] + d];
    if (!std::isfinite(pd)) return fail(c, AHMC_ERR_ARGUMENT, "ArgumentError: prior_prec holds a non-finite value");
    if (pd < 0) return fail(c, AHMC_ERR_ARGUMENT, "DomainError: prior_prec[" + std::to_string(d + 1) + "] = " + std::to_string(pd) + " is negative");
  }
  if (on_w) {
    HglmTab<T> tab{};
    for (int k = 0; k < G; ++k) {
      for (int64_t d = hs->lo[k]; d < hs->hi[k]; ++d)
        if ((double)h[off[GLM_PREC] + d] != 0)
          return fail(c, AHMC_ERR_ARGUMENT, "ArgumentError: prior_prec[" + std::to_string(d + 1) + "] must be 0: the coefficient is a member of group " + std::to_string(k + 1));
      tab.lo[k] = m.lo[k] = hs->lo[k];
      tab.hi[k] = m.hi[k] = hs->hi[k];
      tab.centered[k] = m.centered[k] = hs->centered && hs->centered[k] ? 1 : 0;
      tab.inv_a2[k] = (T)(1.0 / (hs->A[k] * hs->A[k]));
      m.A[k] = hs->A[k];
    }
    memcpy(h.data() + off[GLM_TAB], &tab, sizeof(tab));
  }
  T* hXt = h.data() + off[GLM_XT];
  for (int64_t d = 0; d < Px; ++d)
    for (int64_t i = 0; i < n_obs; ++i) hXt[d + i * Px] = hX[i + d * n_obs];
  if (F > 0) {
    // the factor table, the level indices as received (checked by glm_factor_set), and per factor the stable permutation of the
    // observations by level (a counting sort: ascending observations within a level) with the row pointers of all levels together
    GlmFacTab ft{};
    int* lev = reinterpret_cast<int*>(h.data() + off[GLM_LEV]);
    int* perm = reinterpret_cast<int*>(h.data() + off[GLM_PERM]);
    int* rp = reinterpret_cast<int*>(h.data() + off[GLM_RP]);
    ft.F = F;
    int64_t row = Px, q0 = 0;
    for (int f = 0; f < F; ++f) {
      const int Lf = hs->n_levels[f];
      ft.off[f] = (int)row;
      ft.L[f] = m.L[f] = Lf;
      const int32_t* lf = hs->levels + (int64_t)f * n_obs;
      std::vector<int64_t> cnt((size_t)Lf + 1, 0);
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
    memcpy(h.data() + off[GLM_FTAB], &ft, sizeof(ft));
  }
  // everything that can fail happens before the previous target is touched
  if (hipMalloc(reinterpret_cast<void**>(&m.buf), sizeof(T) * (size_t)total) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, AHMC_ERR_RUNTIME, "set_target_glm: cannot allocate " + std::to_string((long long)(sizeof(T) * (size_t)total)) + " bytes for the model (" +
                                         std::to_string((long long)(sizeof(T) * (size_t)n_data)) + ") and its workspaces U (n_obs × N), partial and the slice sums" +
                                         (on_w ? ", W and R (n_coef × N)" : "") + (aux ? ", partial_s" : "") +
                                         (n_cat > 0 ? ", the cutpoint table (3 × (C − 1) × N) and partial_c" : "") +
                                         (n_cls > 0 ? "; U holds a plane per non-reference class" : "") +
                                         (F > 0 ? "; the model holds the level indices, permutations and row pointers of " + std::to_string(F) + " factors" : ""));
  }
  if (hipMemcpy(m.buf, h.data(), sizeof(T) * (size_t)n_data, hipMemcpyHostToDevice) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
    (void)hipFree(m.buf);
    return fail(c, AHMC_ERR_RUNTIME, std::string("set_target_glm: copying the model failed: ") + hipGetErrorString(hipGetLastError()));
  }
  if (c->glm.buf) (void)hipFree(c->glm.buf);  // (the stream is idle)
  if (c->tparams) { (void)hipFree(c->tparams); c->tparams = nullptr; }
  m.family = family;
  m.n_obs = n_obs;
  m.has_offset = offset != nullptr;
  m.scale = scale;
  m.P = D;
  m.Px = Px;
  m.F = F;
  m.Lt = Lt;
  m.G = G;
  m.bound_hier = hs != nullptr;
  m.aux = aux;
  if (aux) { m.aux_loc = hs->aux_loc; m.aux_scale = hs->aux_scale; }
  m.n_cat = n_cat;
  if (n_cat > 0)
    for (int i = 0; i < 4; ++i) m.cut_prior[i] = hs->cut_prior[i];
  m.n_cls = n_cls;
  c->glm = m;
  c->target_kind = AHMC_TARGET_GLM;
  c->have_point = false;
  invalidate_schedule(c);
  return AHMC_OK;
}

template <class T>
int glm_pointwise(Ctx<T>* c, void* eta_out, void* ll_out) {
  const GlmModel<T>& m = c->glm;
  if (c->target_kind != AHMC_TARGET_GLM || !m.buf) return fail(c, AHMC_ERR_ARGUMENT, "glm_pointwise: no GLM is bound (ahmc_set_target_glm)");
  if (!eta_out && !ll_out) return AHMC_OK;
  const size_t n = (size_t)m.n_obs * (size_t)c->N;
  const size_t n_eta = n * (size_t)(m.n_cls > 0 ? m.n_cls - 1 : 1);  // (a categorical model: a plane of η per non-reference class)
  T* tmp = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&tmp), sizeof(T) * (n_eta + n)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, AHMC_ERR_RUNTIME, "glm_pointwise: cannot allocate " + std::to_string((long long)(sizeof(T) * (n_eta + n))) + " bytes");
  }
  const int64_t nrb = (m.n_obs + GB_M - 1) / GB_M;
  const T* th = c->th;
  if (m.on_w()) {  // the effective coefficients first
    hipLaunchKernelGGL((k_hglm_coef<T>), dim3((unsigned)((c->N + 3) / 4)), dim3(256), 0, c->stream, (const T*)c->th, m.tab(), m.at(GLM_W), (T*)nullptr, (int)m.P, m.G,
                       c->D, c->N, (const int*)nullptr);
    th = m.at(GLM_W);
  }
  if (m.n_cat > 0) glm_launch_cut(c, (const int*)nullptr, c->N);
  T* const eta_tmp = eta_out ? tmp : (T*)nullptr;
  T* const ll_tmp = ll_out ? tmp + n_eta : (T*)nullptr;
  int rc = m.n_cls > 0 ? glm_launch_eta_cat(c, th, (const int*)nullptr, c->N, glm_small(c, nrb, c->N), eta_tmp, ll_tmp, (T*)nullptr)
                       : glm_launch_eta(c, th, (int)m.P, (const int*)nullptr, c->N, glm_small(c, nrb, c->N), eta_tmp, ll_tmp);
  hipError_t e = hipSuccess;
  if (!rc && eta_out) e = hipMemcpyAsync(eta_out, tmp, sizeof(T) * n_eta, hipMemcpyDefault, c->stream);
  if (!rc && e == hipSuccess && ll_out) e = hipMemcpyAsync(ll_out, tmp + n_eta, sizeof(T) * n, hipMemcpyDefault, c->stream);
  const hipError_t es = hipStreamSynchronize(c->stream);
  (void)hipFree(tmp);
  if (rc) return rc;
  if (e != hipSuccess || es != hipSuccess) return fail(c, AHMC_ERR_RUNTIME, std::string("glm_pointwise: ") + hipGetErrorString(e != hipSuccess ? e : es));
  return AHMC_OK;
}

// ---- include/ahmc_glm_hier.h ----
template <class T>
int hglm_set(Ctx<T>* c, int family, int64_t n_obs, const T* X, const T* y, const T* offset, const T* prec, double scale, const HglmSpec& hs) {
  const int64_t n_coef = hs.P;
  const int n_groups = hs.G;
  const bool aux = hs.aux;
  if (family == AHMC_GLM_ORDERED_LOGIT && hs.n_cat == 0) return fail(c, AHMC_ERR_ARGUMENT, glm_ordinal_elsewhere(family, aux));  // (whatever D is)
  if (family == AHMC_GLM_CATEGORICAL_LOGIT && hs.n_cls == 0) return fail(c, AHMC_ERR_ARGUMENT, glm_categorical_elsewhere(family, aux));
  if (n_groups < 0) return fail(c, AHMC_ERR_ARGUMENT, "hglm_set_target: n_groups must be >= 0; got " + std::to_string(n_groups));
  if (aux && n_groups > AHMC_GLM_AUX_MAX_GROUPS)
    return fail(c, AHMC_ERR_UNSUPPORTED, "glm_aux_set_target: n_groups = " + std::to_string(n_groups) + " is beyond the engine's limit AHMC_GLM_AUX_MAX_GROUPS = " +
                                             std::to_string(AHMC_GLM_AUX_MAX_GROUPS));
  if (n_groups > AHMC_HGLM_MAX_GROUPS)
    return fail(c, AHMC_ERR_UNSUPPORTED, "hglm_set_target: n_groups = " + std::to_string(n_groups) + " is beyond the engine's limit AHMC_HGLM_MAX_GROUPS = " +
                                             std::to_string(AHMC_HGLM_MAX_GROUPS));
  const int n_cut = hs.n_cat > 0 ? hs.n_cat - 1 : 0;
  if (n_coef < 1 || c->D != n_coef + n_groups + (aux ? 1 : 0) + n_cut)
    return fail(c, AHMC_ERR_ARGUMENT, "DimensionMismatch: the context has D = " + std::to_string((long long)c->D) + ", the model n_coef + n_groups = " +
                                          std::to_string((long long)n_coef) + " + " + std::to_string(n_groups) + (aux ? " (+ 1: the dispersion's row)" : "") +
                                          (n_cut ? " + " + std::to_string(n_cut) + " (n_categories - 1: the cutpoints' rows)" : "") +
                                          (hs.n_cls > 0 ? " (n_coef: " + std::to_string(hs.n_cls - 1) + " blocks, one per non-reference class, of " +
                                                              std::to_string((long long)(n_coef / (hs.n_cls - 1))) + " rows)"
                                           : hs.F > 0   ? " (n_coef: " + std::to_string((long long)hs.Px) + " columns of X and the factors' levels)"
                                                        : ""));
  if (aux && !std::isfinite(hs.aux_loc)) return fail(c, AHMC_ERR_ARGUMENT, "DomainError: aux_loc = " + std::to_string(hs.aux_loc) + " must be finite");
  if (aux && !(std::isfinite(hs.aux_scale) && hs.aux_scale > 0))
    return fail(c, AHMC_ERR_ARGUMENT, "DomainError: aux_scale = " + std::to_string(hs.aux_scale) + " must be finite and > 0");
  if (n_groups > 0 && (!hs.lo || !hs.hi || !hs.A)) return fail(c, AHMC_ERR_ARGUMENT, "hglm_set_target: lo, hi or hyper_scale is NULL");
  int64_t prev = 0;
  for (int k = 0; k < n_groups; ++k) {
    const int32_t lo = hs.lo[k], hi = hs.hi[k];
    const std::string grp = "group " + std::to_string(k + 1) + " = [" + std::to_string(lo) + ", " + std::to_string(hi) + ")";
    if (lo < 0 || hi > n_coef) return fail(c, AHMC_ERR_ARGUMENT, "ArgumentError: " + grp + " is out of bounds [0, " + std::to_string((long long)n_coef) + ")");
    if (hi <= lo) return fail(c, AHMC_ERR_ARGUMENT, "ArgumentError: " + grp + " is empty");
    if (lo < prev) return fail(c, AHMC_ERR_ARGUMENT, "ArgumentError: " + grp + " overlaps the group before it or is out of order");
    if (hs.n_cls > 0) {  // a categorical model: inside one class's block, or whole blocks
      const int64_t Pb = n_coef / (hs.n_cls - 1);
      if (lo / Pb != (hi - 1) / Pb && (lo % Pb != 0 || hi % Pb != 0))
        return fail(c, AHMC_ERR_ARGUMENT, "ArgumentError: " + grp + " straddles the classes' blocks of " + std::to_string((long long)Pb) +
                                              " rows: a group lies inside one block or is a union of whole blocks");
    }
    if (!(std::isfinite(hs.A[k]) && hs.A[k] > 0))
      return fail(c, AHMC_ERR_ARGUMENT, "DomainError: hyper_scale[" + std::to_string(k + 1) + "] = " + std::to_string(hs.A[k]) + " must be finite and > 0");
    prev = hi;
  }
  return glm_set(c, family, n_obs, X, y, offset, prec, scale, &hs);
}

// ---- include/ahmc_glm_factor.h ----
// hs.Px, hs.F, hs.n_levels, hs.levels as received; hs.P is filled in here (Px + Σ levels), then hglm_set checks the groups against it
template <class T>
int glm_factor_set(Ctx<T>* c, int family, int64_t n_obs, const T* X, const T* y, const T* offset, const T* prec, double scale, HglmSpec hs) {
  const int F = hs.F;
  if (F < 0) return fail(c, AHMC_ERR_ARGUMENT, "glm_factor_set_target: n_factors must be >= 0; got " + std::to_string(F));
  if (F > AHMC_GLM_FACTOR_MAX)
    return fail(c, AHMC_ERR_UNSUPPORTED, "glm_factor_set_target: n_factors = " + std::to_string(F) + " is beyond the engine's limit AHMC_GLM_FACTOR_MAX = " +
                                             std::to_string(AHMC_GLM_FACTOR_MAX));
  if (hs.Px < 1)
    return fail(c, AHMC_ERR_ARGUMENT, "DimensionMismatch: X must keep at least one dense column; n_coef = " + std::to_string((long long)hs.Px));
  if (n_obs < 1) return fail(c, AHMC_ERR_ARGUMENT, "glm_factor_set_target: n_obs must be >= 1; got " + std::to_string(n_obs));
  if (n_obs > AHMC_GLM_MAX_OBS)  // (before the level indices are read)
    return fail(c, AHMC_ERR_UNSUPPORTED, "glm_factor_set_target: n_obs = " + std::to_string(n_obs) + " is beyond the engine's limit AHMC_GLM_MAX_OBS = " +
                                             std::to_string((long long)AHMC_GLM_MAX_OBS));
  if (F > 0 && (!hs.n_levels || !hs.levels)) return fail(c, AHMC_ERR_ARGUMENT, "glm_factor_set_target: n_levels or levels is NULL");
  int64_t P = hs.Px;
  for (int f = 0; f < F; ++f) {
    const int32_t Lf = hs.n_levels[f];
    if (Lf < 1) return fail(c, AHMC_ERR_ARGUMENT, "DomainError: factor " + std::to_string(f + 1) + " has n_levels = " + std::to_string(Lf) + "; must be >= 1");
    P += Lf;
  }
  if (P > INT32_MAX / 2) return fail(c, AHMC_ERR_UNSUPPORTED, "glm_factor_set_target: " + std::to_string((long long)P) + " coefficient rows are beyond 2^30");
  for (int f = 0; f < F; ++f)
    for (int64_t i = 0; i < n_obs; ++i) {
      const int32_t l = hs.levels[i + (int64_t)f * n_obs];
      if (l < 0 || l >= hs.n_levels[f])
        return fail(c, AHMC_ERR_ARGUMENT, "DomainError: levels[" + std::to_string((long long)i + 1) + ", " + std::to_string(f + 1) + "] = " + std::to_string(l) +
                                              " is outside [0, " + std::to_string(hs.n_levels[f]) + ") (zero-based level indices)");
    }
  if (hs.n_cls > 0) P *= hs.n_cls - 1;  // (a categorical model: a block of these rows per non-reference class)
  if (P > INT32_MAX / 2) return fail(c, AHMC_ERR_UNSUPPORTED, "glm_categorical_set_target: " + std::to_string((long long)P) + " coefficient rows are beyond 2^30");
  hs.P = P;
  return hglm_set(c, family, n_obs, X, y, offset, prec, scale, hs);
}

// ---- include/ahmc_glm_ordinal.h ----
// hs as glm_factor_set takes it (hs.F may be 0); the family is AHMC_GLM_ORDERED_LOGIT, there is no scale and no dispersion
template <class T>
int glm_ordinal_set(Ctx<T>* c, int64_t n_obs, const T* X, const T* y, const T* offset, const T* prec, HglmSpec hs, int32_t n_categories, const double* cut_prior) {
  if (n_categories < 2)
    return fail(c, AHMC_ERR_ARGUMENT, "DomainError: n_categories = " + std::to_string(n_categories) + "; an ordered outcome has at least 2 categories");
  if (n_categories > AHMC_GLM_ORDINAL_MAX_CATEGORIES)
    return fail(c, AHMC_ERR_UNSUPPORTED, "glm_ordinal_set_target: n_categories = " + std::to_string(n_categories) +
                                             " is beyond the engine's limit AHMC_GLM_ORDINAL_MAX_CATEGORIES = " + std::to_string(AHMC_GLM_ORDINAL_MAX_CATEGORIES));
  if (!cut_prior) return fail(c, AHMC_ERR_ARGUMENT, "glm_ordinal_set_target: cut_prior is NULL");
  for (int i = 0; i < 4; ++i)
    if (!std::isfinite(cut_prior[i]) || (i % 2 == 1 && !(cut_prior[i] > 0)))
      return fail(c, AHMC_ERR_ARGUMENT, "DomainError: cut_prior[" + std::to_string(i + 1) + "] = " + std::to_string(cut_prior[i]) +
                                            (i % 2 == 1 ? " must be finite and > 0 (a scale)" : " must be finite (a location)"));
  hs.n_cat = n_categories;
  hs.cut_prior = cut_prior;
  return glm_factor_set(c, AHMC_GLM_ORDERED_LOGIT, n_obs, X, y, offset, prec, 1.0, hs);
}

// ---- include/ahmc_glm_categorical.h ----
// hs as glm_ordinal_set takes it; the family is AHMC_GLM_CATEGORICAL_LOGIT, there is no scale, no dispersion and no row of its own
template <class T>
int glm_categorical_set(Ctx<T>* c, int64_t n_obs, const T* X, const T* y, const T* offset, const T* prec, HglmSpec hs, int32_t n_categories) {
  if (n_categories < 2)
    return fail(c, AHMC_ERR_ARGUMENT, "DomainError: n_categories = " + std::to_string(n_categories) + "; a categorical outcome has at least 2 classes");
  if (n_categories > AHMC_GLM_CATEGORICAL_MAX_CATEGORIES)
    return fail(c, AHMC_ERR_UNSUPPORTED, "glm_categorical_set_target: n_categories = " + std::to_string(n_categories) +
                                             " is beyond the engine's limit AHMC_GLM_CATEGORICAL_MAX_CATEGORIES = " +
                                             std::to_string(AHMC_GLM_CATEGORICAL_MAX_CATEGORIES));
  hs.n_cls = n_categories;
  return glm_factor_set(c, AHMC_GLM_CATEGORICAL_LOGIT, n_obs, X, y, offset, prec, 1.0, hs);
}

// ahmc_hglm_coefficients and ahmc_glm_dispersion: a temporary of `elems` elements that begins with the n_theta elements of the
// caller's draws (host or device memory); `run(tmp)` enqueues the kernel and the copies out and returns the first error
template <class T, class F>
int glm_on_draws(Ctx<T>* c, const char* who, const void* theta, size_t n_theta, size_t elems, F run) {
  T* tmp = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&tmp), sizeof(T) * elems) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, AHMC_ERR_RUNTIME, std::string(who) + ": cannot allocate " + std::to_string((long long)(sizeof(T) * elems)) + " bytes");
  }
  hipError_t e = hipMemcpyAsync(tmp, theta, sizeof(T) * n_theta, hipMemcpyDefault, c->stream);
  if (e == hipSuccess) e = run(tmp);
  const hipError_t es = hipStreamSynchronize(c->stream);
  (void)hipFree(tmp);
  if (e != hipSuccess || es != hipSuccess) return fail(c, AHMC_ERR_RUNTIME, std::string(who) + ": " + hipGetErrorString(e != hipSuccess ? e : es));
  return AHMC_OK;
}

// β (P, n_cols) and / or τ (G, n_cols) of any (D, n_cols) array of draws, host or device pointers
template <class T>
int hglm_coefficients(Ctx<T>* c, const void* theta, int64_t n_cols, void* beta_out, void* tau_out) {
  const GlmModel<T>& m = c->glm;
  if (c->target_kind != AHMC_TARGET_GLM || !m.buf || !m.bound_hier)
    return fail(c, AHMC_ERR_ARGUMENT, "hglm_coefficients: no hierarchical GLM is bound (ahmc_hglm_set_target)");
  if (n_cols < 0 || (n_cols > 0 && !theta)) return fail(c, AHMC_ERR_ARGUMENT, "hglm_coefficients: theta is NULL or n_cols < 0");
  if (n_cols > INT32_MAX) return fail(c, AHMC_ERR_UNSUPPORTED, "hglm_coefficients: n_cols beyond 2^31 - 1");
  if (n_cols == 0 || (!beta_out && !tau_out)) return AHMC_OK;
  const int64_t P = m.P, G = m.G, D = c->D;
  if (!m.on_w()) {  // the plain model: β = θ
    if (beta_out) HIPCHK(hipMemcpyAsync(beta_out, theta, sizeof(T) * (size_t)(P * n_cols), hipMemcpyDefault, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return AHMC_OK;
  }
  return glm_on_draws(c, "hglm_coefficients", theta, (size_t)(D * n_cols), (size_t)((D + P + G) * n_cols), [&](T* th) {
    T *W = th + D * n_cols, *tau = W + P * n_cols;
    hipLaunchKernelGGL((k_hglm_coef<T>), dim3((unsigned)((n_cols + 3) / 4)), dim3(256), 0, c->stream, (const T*)th, m.tab(), W, tau, (int)P, (int)G, D, n_cols,
                       (const int*)nullptr);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && beta_out) e = hipMemcpyAsync(beta_out, W, sizeof(T) * (size_t)(P * n_cols), hipMemcpyDefault, c->stream);
    if (e == hipSuccess && tau_out && G > 0) e = hipMemcpyAsync(tau_out, tau, sizeof(T) * (size_t)(G * n_cols), hipMemcpyDefault, c->stream);
    return e;
  });
}

// ---- include/ahmc_glm_aux.h ----
// exp(s) of any (D, n_cols) array of draws, host or device pointers: s is each column's last row
template <class T>
int glm_dispersion(Ctx<T>* c, const void* theta, int64_t n_cols, void* out) {
  if (c->target_kind != AHMC_TARGET_GLM || !c->glm.buf || !c->glm.aux)
    return fail(c, AHMC_ERR_ARGUMENT, "glm_dispersion: no model with a sampled dispersion is bound (ahmc_glm_aux_set_target)");
  if (n_cols < 0 || (n_cols > 0 && (!theta || !out))) return fail(c, AHMC_ERR_ARGUMENT, "glm_dispersion: theta or out is NULL, or n_cols < 0");
  if (n_cols > INT32_MAX) return fail(c, AHMC_ERR_UNSUPPORTED, "glm_dispersion: n_cols beyond 2^31 - 1");
  if (n_cols == 0) return AHMC_OK;
  const int64_t D = c->D;
  return glm_on_draws(c, "glm_dispersion", theta, (size_t)(D * n_cols), (size_t)((D + 1) * n_cols), [&](T* th) {
    T* e_s = th + D * n_cols;
    hipLaunchKernelGGL((k_glm_exp_row<T>), dim3((unsigned)((n_cols + 255) / 256)), dim3(256), 0, c->stream, (const T*)th, D, D - 1, n_cols, e_s);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : hipMemcpyAsync(out, e_s, sizeof(T) * (size_t)n_cols, hipMemcpyDefault, c->stream);
  });
}

// ---- include/ahmc_glm_ordinal.h ----
// the cutpoints c (C−1, n_cols) of any (D, n_cols) array of draws, host or device pointers: κ is each column's last C − 1 rows
template <class T>
int glm_cutpoints(Ctx<T>* c, const void* theta, int64_t n_cols, void* out) {
  if (c->target_kind != AHMC_TARGET_GLM || !c->glm.buf || c->glm.n_cat == 0)
    return fail(c, AHMC_ERR_ARGUMENT, "glm_cutpoints: no ordinal model is bound (ahmc_glm_ordinal_set_target)");
  if (n_cols < 0 || (n_cols > 0 && (!theta || !out))) return fail(c, AHMC_ERR_ARGUMENT, "glm_cutpoints: theta or out is NULL, or n_cols < 0");
  if (n_cols > INT32_MAX) return fail(c, AHMC_ERR_UNSUPPORTED, "glm_cutpoints: n_cols beyond 2^31 - 1");
  if (n_cols == 0) return AHMC_OK;
  const int64_t D = c->D, Cm1 = c->glm.n_cat - 1;
  return glm_on_draws(c, "glm_cutpoints", theta, (size_t)(D * n_cols), (size_t)((D + Cm1) * n_cols), [&](T* th) {
    T* cut = th + D * n_cols;
    hipLaunchKernelGGL((k_glm_cut<T>), dim3((unsigned)((n_cols + 255) / 256)), dim3(256), 0, c->stream, (const T*)th, D, D - Cm1, (int)Cm1, cut, n_cols, n_cols,
                       (const int*)nullptr, 0);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : hipMemcpyAsync(out, cut, sizeof(T) * (size_t)(Cm1 * n_cols), hipMemcpyDefault, c->stream);
  });
}

// ---- include/ahmc_glm_categorical.h ----
// the class probabilities (C, n_obs, n_cols) at any (D, n_cols) array of draws, host or device pointers: chunks of at most N columns
// through k_hglm_coef and k_glm_eta_cat on the model's own workspaces W, U and partial (stream-ordered with every evaluation)
template <class T>
int glm_class_probs(Ctx<T>* c, const void* theta, int64_t n_cols, void* out) {
  const GlmModel<T>& m = c->glm;
  if (c->target_kind != AHMC_TARGET_GLM || !m.buf || m.n_cls == 0)
    return fail(c, AHMC_ERR_ARGUMENT, "glm_class_probs: no categorical model is bound (ahmc_glm_categorical_set_target)");
  if (n_cols < 0 || (n_cols > 0 && (!theta || !out))) return fail(c, AHMC_ERR_ARGUMENT, "glm_class_probs: theta or out is NULL, or n_cols < 0");
  if (n_cols > INT32_MAX) return fail(c, AHMC_ERR_UNSUPPORTED, "glm_class_probs: n_cols beyond 2^31 - 1");
  if (n_cols == 0) return AHMC_OK;
  const int64_t D = c->D, chunk = n_cols < c->N ? n_cols : c->N, per_col = (int64_t)m.n_cls * m.n_obs, nrb = (m.n_obs + GB_M - 1) / GB_M;
  const size_t elems = (size_t)((D + per_col) * chunk);
  T* tmp = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&tmp), sizeof(T) * elems) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, AHMC_ERR_RUNTIME, "glm_class_probs: cannot allocate " + std::to_string((long long)(sizeof(T) * elems)) + " bytes");
  }
  T* const pr = tmp + D * chunk;
  hipError_t e = hipSuccess;
  int rc = AHMC_OK;
  for (int64_t j0 = 0; j0 < n_cols && !rc && e == hipSuccess; j0 += chunk) {
    const int64_t nc = n_cols - j0 < chunk ? n_cols - j0 : chunk;
    e = hipMemcpyAsync(tmp, static_cast<const T*>(theta) + j0 * D, sizeof(T) * (size_t)(D * nc), hipMemcpyDefault, c->stream);
    if (e != hipSuccess) break;
    hipLaunchKernelGGL((k_hglm_coef<T>), dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, c->stream, (const T*)tmp, m.tab(), m.at(GLM_W), (T*)nullptr, (int)m.P, m.G, D, nc,
                       (const int*)nullptr);
    rc = glm_launch_eta_cat(c, (const T*)m.at(GLM_W), (const int*)nullptr, nc, glm_small(c, nrb, nc), (T*)nullptr, (T*)nullptr, pr);
    if (!rc) e = hipMemcpyAsync(static_cast<T*>(out) + j0 * per_col, pr, sizeof(T) * (size_t)(per_col * nc), hipMemcpyDefault, c->stream);
  }
  const hipError_t es = hipStreamSynchronize(c->stream);
  (void)hipFree(tmp);
  if (rc) return rc;
  if (e != hipSuccess || es != hipSuccess) return fail(c, AHMC_ERR_RUNTIME, std::string("glm_class_probs: ") + hipGetErrorString(e != hipSuccess ? e : es));
  return AHMC_OK;
}
