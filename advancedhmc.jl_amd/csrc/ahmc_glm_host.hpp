// ahmc_glm_host.hpp — the device side of the host's work on the generalised-linear-model target (kernels: ahmc_glm.hpp), for every
// kind of model of include/ahmc_glm*.h.  glm_bind binds the model that a GlmSpec describes: ahmc_glm_spec.hpp checks and lays out,
// this file stages, allocates and commits.  glm_forward enqueues coefficients → cutpoints → η for whatever kind is bound, glm_launch_grad
// the gradient product of one coefficient block; glm_target is the two with the kind's finishing kernel.  glm_on_draws walks a
// caller's draws in chunks for the post-processing entry points.  Included by ahmc_api.hip after the context, before
// ahmc_dense_host.hpp, whose dn_other_target routes to glm_target.
#pragma once

static_assert(GLM_SPEC_ROW_BLOCK == GB_M && GLM_SPEC_K_SLICE == GLM_K_SLICE, "ahmc_glm_spec.hpp lays the slab out for other tiles than the kernels'");
static_assert(AHMC_GLM_FACTOR_MAX == GLM_MAX_FACTORS && AHMC_HGLM_MAX_GROUPS == HGLM_MAX_GROUPS, "the headers and the kernels disagree");

// the targets that fill lp and g for a LIST of chains from th, on the step-synchronous engine: the user's kernel and the GLM
template <class T>
bool listed_target(const Ctx<T>* c) {
  return c->target_kind == AHMC_TARGET_KERNEL || c->target_kind == AHMC_TARGET_GLM;
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
// theta: the (D_θ, ·) array whose last row is the dispersion (the context's θ, or a chunk of a caller's draws).
template <class T>
int glm_launch_eta(Ctx<T>* c, const T* th, int D, const int* list, int64_t ncols, bool small, T* eta_out, T* ll_out, const T* theta) {
  const GlmModel<T>& m = c->glm;
  const int n_obs = (int)m.n_obs;
  const int64_t nrb = (n_obs + GB_M - 1) / GB_M;
  const T* X = m.at(GLM_X);
  const T* y = m.at(GLM_Y);
  const T* off = m.has_offset ? m.at(GLM_OFF) : nullptr;
  T* U = m.at(GLM_U);
  T* part = m.at(GLM_PART);
  // a sampled dispersion: s is row D − 1 of the chain's own θ (th holds W); Σ ∂ℓ/∂s per row block
  const T* aux = m.aux ? theta + (c->D - 1) : nullptr;
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
  if (m.F > 0 && D != m.P) return fail(c, AHMC_ERR_STATE, "glm: a model with factors runs on its P rows of W");
  // the one launch site of either kernel; the family and the tile shape arrive as types
  const auto launch = [&](auto fam, auto bn) {
    constexpr int FAM = decltype(fam)::value, BN = decltype(bn)::value;
    if (m.F > 0)
      hipLaunchKernelGGL((k_glm_eta_f<T, FAM, BN>), grid, dim3(256), 0, c->stream, X, y, off, (T)m.scale, th, U, part, n_obs, (int)m.Px, (int64_t)D, ncols, c->N, list,
                         eta_out, ll_out, aux, aux_ld, part_s, m.ftab(), m.ints(GLM_LEV));
    else
      hipLaunchKernelGGL((k_glm_eta<T, FAM, BN>), grid, dim3(256), 0, c->stream, X, y, off, (T)m.scale, th, U, part, n_obs, D, ncols, c->N, list, eta_out, ll_out, aux,
                         aux_ld, part_s);
  };
  const auto shaped = [&](auto fam) {
    if (small) launch(fam, std::integral_constant<int, 16>{});
    else launch(fam, std::integral_constant<int, 64>{});
  };
  switch (m.family) {
    case 0: shaped(std::integral_constant<int, 0>{}); break;
    case 1: shaped(std::integral_constant<int, 1>{}); break;
    case 2: shaped(std::integral_constant<int, 2>{}); break;
    case 3: shaped(std::integral_constant<int, 3>{}); break;
    case 4: shaped(std::integral_constant<int, 4>{}); break;
    case 5: shaped(std::integral_constant<int, 5>{}); break;
    default: return fail(c, AHMC_ERR_STATE, "glm: unknown family in the context");
  }
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

// an ordinal model's cutpoint table (c, lg, r) of the listed chains from the κ rows of theta (column stride D), before k_glm_eta
template <class T>
void glm_launch_cut(Ctx<T>* c, const int* list, int64_t n, const T* theta) {
  const GlmModel<T>& m = c->glm;
  hipLaunchKernelGGL((k_glm_cut<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, theta, c->D, c->D - (m.n_cat - 1), m.n_cat - 1, m.at(GLM_CUT), c->N, n,
                     list, 1);
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

// The forward path of whatever kind is bound, enqueued on the context's stream: the effective coefficients W if the model runs on
// them (k_hglm_coef), the cutpoint table if it is ordinal, then η — U and the partial sums on the model's workspaces, and on request
// η, ℓ and the class probabilities themselves.  theta: (D, ·) with column stride D, the context's θ or a chunk of a caller's draws;
// list: the chains' columns, or none for the first ncols.  Returns the coefficients the products ran on through th_out.
template <class T>
int glm_forward(Ctx<T>* c, const T* theta, const int* list, int64_t ncols, T* eta_out, T* ll_out, T* prob_out, const T** th_out = nullptr) {
  const GlmModel<T>& m = c->glm;
  const int64_t nrb = (m.n_obs + GB_M - 1) / GB_M;
  const T* th = theta;
  if (m.on_w()) {
    hipLaunchKernelGGL((k_hglm_coef<T>), dim3((unsigned)((ncols + 3) / 4)), dim3(256), 0, c->stream, theta, m.tab(), m.at(GLM_W), (T*)nullptr, (int)m.P, m.G, c->D, ncols,
                       list);
    th = m.at(GLM_W);
  }
  if (th_out) *th_out = th;
  if (m.n_cat > 0) glm_launch_cut(c, list, ncols, theta);
  const bool small = glm_small(c, nrb, ncols);
  if (m.n_cls > 0) return glm_launch_eta_cat(c, th, list, ncols, small, eta_out, ll_out, prob_out);
  if (prob_out) return fail(c, AHMC_ERR_STATE, "glm: class probabilities of a model that is not categorical");
  return glm_launch_eta(c, th, (int)m.P, list, ncols, small, eta_out, ll_out, theta);
}

// One coefficient block's rows of the gradient product: R = prec∘W − Xᵀ·U over the Px dense columns (in K slices that k_glm_gsum
// adds in ascending order where n_obs spans more than one), then the factors' rows from U by level (k_glm_fgrad).  The plain
// model's block is all D rows of (W, R); a block of a model with factors or classes starts at W and R and keeps their column
// stride D (the _ld kernels).  The slice workspace is reused stream-ordered.
template <class T>
void glm_launch_grad(Ctx<T>* c, const T* U, const T* prec, const T* W, T* R, const int* list, int64_t n) {
  const GlmModel<T>& m = c->glm;
  const int n_obs = (int)m.n_obs, D = (int)m.P, Px = (int)m.Px, ns = glm_slices(c);
  const int64_t nrbD = (int64_t)(Px + GB_M - 1) / GB_M * ns;
  const bool small = glm_small(c, nrbD, n), blocks = m.F > 0 || m.n_cls > 0;
  const T* Xt = m.at(GLM_XT);
  T* gs = m.at(GLM_GS);
  const dim3 grid = small ? dim3((unsigned)nrbD, (unsigned)((n + 15) / 16)) : dim3((unsigned)(nrbD * (((n + GB_N - 1) / GB_N + 7) / 8 * 8)));
  const auto launch = [&](auto bn) {
    constexpr int BN = decltype(bn)::value;
    if (blocks) hipLaunchKernelGGL((k_glm_grad_ld<T, BN>), grid, dim3(256), 0, c->stream, Xt, U, prec, W, R, gs, n_obs, Px, (int64_t)D, n, c->N, list, ns);
    else hipLaunchKernelGGL((k_glm_grad<T, BN>), grid, dim3(256), 0, c->stream, Xt, U, prec, W, R, gs, n_obs, D, n, c->N, list, ns);
  };
  if (small) launch(std::integral_constant<int, 16>{});
  else launch(std::integral_constant<int, 64>{});
  const dim3 sum_grid((unsigned)((n * Px + 255) / 256));  // (Px = D where the model has one block)
  if (ns > 1 && blocks) hipLaunchKernelGGL((k_glm_gsum_ld<T>), sum_grid, dim3(256), 0, c->stream, (const T*)gs, prec, W, R, Px, (int64_t)D, n, c->N, list, ns);
  if (ns > 1 && !blocks) hipLaunchKernelGGL((k_glm_gsum<T>), sum_grid, dim3(256), 0, c->stream, (const T*)gs, prec, W, R, D, n, c->N, list, ns);
  if (m.F > 0)
    hipLaunchKernelGGL((k_glm_fgrad<T>), dim3((unsigned)((n * m.Lt + 255) / 256)), dim3(256), 0, c->stream, U, m.ints(GLM_PERM), m.ints(GLM_RP), R, n_obs, Px, (int)m.Lt,
                       (int64_t)D, n, list);
}

// AHMC_TARGET_GLM: (ℓπ, g = −∇ℓπ) at θ of the listed chains — dn_user_target's contract: reads c->th, writes c->lp and c->g on the
// context's stream
template <class T>
int glm_target(Ctx<T>* c, const int* list, int64_t n, bool sanitize_lp = true) {
  if (n <= 0) return AHMC_OK;
  const GlmModel<T>& m = c->glm;
  if (!m.buf) return fail(c, AHMC_ERR_STATE, "AHMC_TARGET_GLM without a model (ahmc_set_target_glm)");
  // groups, a dispersion, factors, cutpoints or classes bound: the products run on the effective coefficients W (P, N) with a zero
  // precision and leave R = −Xᵀu; k_hglm_coef before them and k_hglm_finish after them are the model (ahmc_glm.hpp)
  const bool hier = m.on_w();
  const int n_obs = (int)m.n_obs, D = (int)m.P, G = m.G;
  const int64_t nrb = (n_obs + GB_M - 1) / GB_M;
  const T* th = nullptr;
  if (int rc = glm_forward(c, (const T*)c->th, list, n, (T*)nullptr, (T*)nullptr, (T*)nullptr, &th)) return rc;
  const T* prec = m.at(hier ? GLM_ZERO : GLM_PREC);
  T* g = hier ? m.at(GLM_R) : c->g;
  // a categorical model, per class k: rows [k·Pb, (k + 1)·Pb) of R = −Xᵀu_k from plane k of U
  const int K = m.K(), Pb = D / K;
  for (int k = 0; k < K; ++k) glm_launch_grad(c, (const T*)m.at(GLM_U) + (int64_t)k * n_obs * c->N, prec, th + (int64_t)k * Pb, g + (int64_t)k * Pb, list, n);
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

// Step 2 of glm_bind: X, y, offset and prior_prec (host or device memory) to their places in the host copy h of the slab's data
template <class T>
int glm_stage(Ctx<T>* c, const GlmSpec& s, const GlmBound& b, T* h) {
  HIPCHK(hipMemcpy(h + b.off[GLM_X], s.X, sizeof(T) * b.n_obs * b.Px, hipMemcpyDefault));
  HIPCHK(hipMemcpy(h + b.off[GLM_Y], s.y, sizeof(T) * b.n_obs, hipMemcpyDefault));
  if (s.offset) HIPCHK(hipMemcpy(h + b.off[GLM_OFF], s.offset, sizeof(T) * b.n_obs * b.K(), hipMemcpyDefault));
  if (s.prior_prec) HIPCHK(hipMemcpy(h + b.off[GLM_PREC], s.prior_prec, sizeof(T) * b.P, hipMemcpyDefault));
  return AHMC_OK;
}

// Step 4 of glm_bind: the slab on the device, then the context takes the model.  Everything that can fail happens before the
// previous target is touched.
template <class T>
int glm_commit(Ctx<T>* c, GlmModel<T>& m, const T* h) {
  const size_t total = (size_t)m.total, n_data = (size_t)m.n_data;
  if (hipMalloc(reinterpret_cast<void**>(&m.buf), sizeof(T) * total) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, AHMC_ERR_RUNTIME, "set_target_glm: cannot allocate " + std::to_string((long long)(sizeof(T) * total)) + " bytes for the model (" +
                                         std::to_string((long long)(sizeof(T) * n_data)) + ") and its workspaces U (n_obs × N), partial and the slice sums" +
                                         (m.on_w() ? ", W and R (n_coef × N)" : "") + (m.aux ? ", partial_s" : "") +
                                         (m.n_cat > 0 ? ", the cutpoint table (3 × (C − 1) × N) and partial_c" : "") +
                                         (m.n_cls > 0 ? "; U holds a plane per non-reference class" : "") +
                                         (m.F > 0 ? "; the model holds the level indices, permutations and row pointers of " + std::to_string(m.F) + " factors" : ""));
  }
  if (hipMemcpy(m.buf, h, sizeof(T) * n_data, hipMemcpyHostToDevice) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
    (void)hipFree(m.buf);
    return fail(c, AHMC_ERR_RUNTIME, std::string("set_target_glm: copying the model failed: ") + hipGetErrorString(hipGetLastError()));
  }
  if (c->glm.buf) (void)hipFree(c->glm.buf);  // (the stream is idle)
  if (c->tparams) { (void)hipFree(c->tparams); c->tparams = nullptr; }
  c->glm = m;
  c->target_kind = AHMC_TARGET_GLM;
  c->have_point = false;
  invalidate_schedule(c);
  return AHMC_OK;
}

// every ahmc_*_set_target of include/ahmc_glm*.h: host-only checks and layout, staging, host-only data checks and tables, commit
template <class T>
int glm_bind(Ctx<T>* c, const GlmSpec& s) {
  GlmModel<T> m;  // (becomes the context's once nothing can fail any more)
  std::string err;
  if (int rc = glm_spec_check<T, HglmTab<T>, GlmFacTab>(s, c->D, c->N, m, err)) return fail(c, rc, err);
  std::vector<T> h((size_t)m.n_data, T(0));
  if (int rc = glm_stage(c, s, m, h.data())) return rc;
  if (int rc = glm_spec_build<T, HglmTab<T>, GlmFacTab>(s, m, h.data(), err)) return fail(c, rc, err);
  return glm_commit(c, m, h.data());
}

template <class T>
int glm_pointwise(Ctx<T>* c, void* eta_out, void* ll_out) {
  const GlmModel<T>& m = c->glm;
  if (c->target_kind != AHMC_TARGET_GLM || !m.buf) return fail(c, AHMC_ERR_ARGUMENT, "glm_pointwise: no GLM is bound (ahmc_set_target_glm)");
  if (!eta_out && !ll_out) return AHMC_OK;
  const size_t n = (size_t)m.n_obs * (size_t)c->N;
  const size_t n_eta = n * (size_t)m.K();  // (a categorical model: a plane of η per non-reference class)
  T* tmp = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&tmp), sizeof(T) * (n_eta + n)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, AHMC_ERR_RUNTIME, "glm_pointwise: cannot allocate " + std::to_string((long long)(sizeof(T) * (n_eta + n))) + " bytes");
  }
  int rc = glm_forward(c, (const T*)c->th, (const int*)nullptr, c->N, eta_out ? tmp : (T*)nullptr, ll_out ? tmp + n_eta : (T*)nullptr, (T*)nullptr);
  hipError_t e = hipSuccess;
  if (!rc && eta_out) e = hipMemcpyAsync(eta_out, tmp, sizeof(T) * n_eta, hipMemcpyDefault, c->stream);
  if (!rc && e == hipSuccess && ll_out) e = hipMemcpyAsync(ll_out, tmp + n_eta, sizeof(T) * n, hipMemcpyDefault, c->stream);
  const hipError_t es = hipStreamSynchronize(c->stream);
  (void)hipFree(tmp);
  if (rc) return rc;
  if (e != hipSuccess || es != hipSuccess) return fail(c, AHMC_ERR_RUNTIME, std::string("glm_pointwise: ") + hipGetErrorString(e != hipSuccess ? e : es));
  return AHMC_OK;
}

// ---- the entry points that take any (D, n_cols) array of draws, host or device pointers ----
// their argument checks; kind_bound: the kind of model the caller needs is bound; null_arg: a pointer it needs is NULL
template <class T>
int glm_draws_check(Ctx<T>* c, const std::string& who, bool kind_bound, const char* unbound, bool null_arg, const char* null_words, int64_t n_cols) {
  if (c->target_kind != AHMC_TARGET_GLM || !c->glm.buf || !kind_bound) return fail(c, AHMC_ERR_ARGUMENT, who + ": " + unbound);
  if (n_cols < 0 || (n_cols > 0 && null_arg)) return fail(c, AHMC_ERR_ARGUMENT, who + ": " + null_words + " n_cols < 0");
  if (n_cols > INT32_MAX) return fail(c, AHMC_ERR_UNSUPPORTED, who + ": n_cols beyond 2^31 - 1");
  return AHMC_OK;
}

// what a walk over draws has met so far: a refusal of the engine's own (the message is in the context) or a HIP error
struct GlmWalk {
  int rc = AHMC_OK;
  hipError_t e = hipSuccess;
  bool ok() const { return !rc && e == hipSuccess; }
};

// the draws in chunks of at most `chunk` columns: each is copied to th (device memory, D·chunk elements), then run(w, j0, nc)
// enqueues the chunk's kernels and copies out and records the first error in w.  Nothing is synchronised here.
template <class T, class F>
GlmWalk glm_walk_draws(Ctx<T>* c, const void* theta, int64_t n_cols, int64_t chunk, T* th, F run) {
  GlmWalk w;
  for (int64_t j0 = 0; j0 < n_cols && w.ok(); j0 += chunk) {
    const int64_t nc = n_cols - j0 < chunk ? n_cols - j0 : chunk;
    w.e = hipMemcpyAsync(th, static_cast<const T*>(theta) + j0 * c->D, sizeof(T) * (size_t)(c->D * nc), hipMemcpyDefault, c->stream);
    if (w.e == hipSuccess) run(w, j0, nc);
  }
  return w;
}

// the walk on a temporary of its own: chunk columns of θ, then out_per_col·chunk elements for run(w, th, out, j0, nc); the stream
// is synchronised before the temporary is freed
template <class T, class F>
int glm_on_draws(Ctx<T>* c, const char* who, const void* theta, int64_t n_cols, int64_t chunk, int64_t out_per_col, F run) {
  const size_t elems = (size_t)((c->D + out_per_col) * chunk);
  T* tmp = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&tmp), sizeof(T) * elems) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, AHMC_ERR_RUNTIME, std::string(who) + ": cannot allocate " + std::to_string((long long)(sizeof(T) * elems)) + " bytes");
  }
  T* const out = tmp + c->D * chunk;
  const GlmWalk w = glm_walk_draws(c, theta, n_cols, chunk, tmp, [&](GlmWalk& st, int64_t j0, int64_t nc) { run(st, (const T*)tmp, out, j0, nc); });
  const hipError_t es = hipStreamSynchronize(c->stream);
  (void)hipFree(tmp);
  if (w.rc) return w.rc;
  if (w.e != hipSuccess || es != hipSuccess) return fail(c, AHMC_ERR_RUNTIME, std::string(who) + ": " + hipGetErrorString(w.e != hipSuccess ? w.e : es));
  return AHMC_OK;
}

// ---- include/ahmc_glm_hier.h ----
// β (P, n_cols) and / or τ (G, n_cols)
template <class T>
int hglm_coefficients(Ctx<T>* c, const void* theta, int64_t n_cols, void* beta_out, void* tau_out) {
  const GlmModel<T>& m = c->glm;
  if (int rc = glm_draws_check(c, "hglm_coefficients", m.bound_hier, "no hierarchical GLM is bound (ahmc_hglm_set_target)", !theta, "theta is NULL or", n_cols)) return rc;
  if (n_cols == 0 || (!beta_out && !tau_out)) return AHMC_OK;
  const int64_t P = m.P, G = m.G, D = c->D;
  if (!m.on_w()) {  // the plain model: β = θ
    if (beta_out) HIPCHK(hipMemcpyAsync(beta_out, theta, sizeof(T) * (size_t)(P * n_cols), hipMemcpyDefault, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return AHMC_OK;
  }
  return glm_on_draws(c, "hglm_coefficients", theta, n_cols, n_cols, P + G, [&](GlmWalk& w, const T* th, T* W, int64_t, int64_t) {
    T* tau = W + P * n_cols;
    hipLaunchKernelGGL((k_hglm_coef<T>), dim3((unsigned)((n_cols + 3) / 4)), dim3(256), 0, c->stream, th, m.tab(), W, tau, (int)P, (int)G, D, n_cols, (const int*)nullptr);
    w.e = hipGetLastError();
    if (w.e == hipSuccess && beta_out) w.e = hipMemcpyAsync(beta_out, W, sizeof(T) * (size_t)(P * n_cols), hipMemcpyDefault, c->stream);
    if (w.e == hipSuccess && tau_out && G > 0) w.e = hipMemcpyAsync(tau_out, tau, sizeof(T) * (size_t)(G * n_cols), hipMemcpyDefault, c->stream);
  });
}

// ---- include/ahmc_glm_aux.h ----
// exp(s): s is each column's last row
template <class T>
int glm_dispersion(Ctx<T>* c, const void* theta, int64_t n_cols, void* out) {
  if (int rc = glm_draws_check(c, "glm_dispersion", c->glm.aux, "no model with a sampled dispersion is bound (ahmc_glm_aux_set_target)", !theta || !out,
                               "theta or out is NULL, or", n_cols))
    return rc;
  if (n_cols == 0) return AHMC_OK;
  const int64_t D = c->D;
  return glm_on_draws(c, "glm_dispersion", theta, n_cols, n_cols, 1, [&](GlmWalk& w, const T* th, T* e_s, int64_t, int64_t) {
    hipLaunchKernelGGL((k_glm_exp_row<T>), dim3((unsigned)((n_cols + 255) / 256)), dim3(256), 0, c->stream, th, D, D - 1, n_cols, e_s);
    w.e = hipGetLastError();
    if (w.e == hipSuccess) w.e = hipMemcpyAsync(out, e_s, sizeof(T) * (size_t)n_cols, hipMemcpyDefault, c->stream);
  });
}

// ---- include/ahmc_glm_ordinal.h ----
// the cutpoints c (C−1, n_cols): κ is each column's last C − 1 rows
template <class T>
int glm_cutpoints(Ctx<T>* c, const void* theta, int64_t n_cols, void* out) {
  if (int rc = glm_draws_check(c, "glm_cutpoints", c->glm.n_cat != 0, "no ordinal model is bound (ahmc_glm_ordinal_set_target)", !theta || !out,
                               "theta or out is NULL, or", n_cols))
    return rc;
  if (n_cols == 0) return AHMC_OK;
  const int64_t D = c->D, Cm1 = c->glm.n_cat - 1;
  return glm_on_draws(c, "glm_cutpoints", theta, n_cols, n_cols, Cm1, [&](GlmWalk& w, const T* th, T* cut, int64_t, int64_t) {
    hipLaunchKernelGGL((k_glm_cut<T>), dim3((unsigned)((n_cols + 255) / 256)), dim3(256), 0, c->stream, th, D, D - Cm1, (int)Cm1, cut, n_cols, n_cols, (const int*)nullptr,
                       0);
    w.e = hipGetLastError();
    if (w.e == hipSuccess) w.e = hipMemcpyAsync(out, cut, sizeof(T) * (size_t)(Cm1 * n_cols), hipMemcpyDefault, c->stream);
  });
}

// ---- include/ahmc_glm_categorical.h ----
// the class probabilities (C, n_obs, n_cols): chunks of at most N columns through glm_forward on the model's own workspaces W, U and
// partial (stream-ordered with every evaluation)
template <class T>
int glm_class_probs(Ctx<T>* c, const void* theta, int64_t n_cols, void* out) {
  const GlmModel<T>& m = c->glm;
  if (int rc = glm_draws_check(c, "glm_class_probs", m.n_cls != 0, "no categorical model is bound (ahmc_glm_categorical_set_target)", !theta || !out,
                               "theta or out is NULL, or", n_cols))
    return rc;
  if (n_cols == 0) return AHMC_OK;
  const int64_t per_col = (int64_t)m.n_cls * m.n_obs;
  return glm_on_draws(c, "glm_class_probs", theta, n_cols, n_cols < c->N ? n_cols : c->N, per_col, [&](GlmWalk& w, const T* th, T* pr, int64_t j0, int64_t nc) {
    w.rc = glm_forward(c, th, (const int*)nullptr, nc, (T*)nullptr, (T*)nullptr, pr);
    if (!w.rc) w.e = hipMemcpyAsync(static_cast<T*>(out) + j0 * per_col, pr, sizeof(T) * (size_t)(per_col * nc), hipMemcpyDefault, c->stream);
  });
}
