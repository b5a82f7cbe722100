// ahmc_glm_host.hpp — host side of the generalised-linear-model target (include/ahmc_glm.h; kernels: ahmc_glm.hpp).  Included by
// ahmc_api.hip after the context, before ahmc_dense_host.hpp, whose dn_other_target routes to glm_target.
#pragma once

// the targets that fill lp and g for a LIST of chains from th, on the step-synchronous engine: the user's kernel and the GLM
template <class T>
bool listed_target(const Ctx<T>* c) {
  return c->target_kind == AHMC_TARGET_KERNEL || c->target_kind == AHMC_TARGET_GLM;
}

enum { GLM_X = 0, GLM_XT, GLM_Y, GLM_OFF, GLM_PREC, GLM_U, GLM_PART, GLM_GS };

template <class T>
int glm_slices(const Ctx<T>* c) {
  return (int)((c->glm_nobs + GLM_K_SLICE - 1) / GLM_K_SLICE);
}

// drop the model's buffers (another target takes over; the stream is made idle first)
template <class T>
int glm_release(Ctx<T>* c) {
  if (!c->glm_buf) return AHMC_OK;
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipFree(c->glm_buf));
  c->glm_buf = nullptr;
  c->glm_nobs = 0;
  return AHMC_OK;
}

// η (and from it U, partial; on request η and ℓ themselves) for ncols listed chains
template <class T>
int glm_launch_eta(Ctx<T>* c, const int* list, int64_t ncols, bool small, T* eta_out, T* ll_out) {
  const T* b = c->glm_buf;
  const int n_obs = (int)c->glm_nobs, D = (int)c->D;
  const int64_t nrb = (n_obs + GB_M - 1) / GB_M;
  const T* X = b + c->glm_off[GLM_X];
  const T* y = b + c->glm_off[GLM_Y];
  const T* off = c->glm_has_offset ? b + c->glm_off[GLM_OFF] : nullptr;
  T* U = c->glm_buf + c->glm_off[GLM_U];
  T* part = c->glm_buf + c->glm_off[GLM_PART];
  const dim3 grid = small ? dim3((unsigned)nrb, (unsigned)((ncols + 15) / 16)) : dim3((unsigned)(nrb * (((ncols + GB_N - 1) / GB_N + 7) / 8 * 8)));
#define AHMC_GLM_ETA(FAM, BN) \
  hipLaunchKernelGGL((k_glm_eta<T, FAM, BN>), grid, dim3(256), 0, c->stream, X, y, off, (T)c->glm_scale, (const T*)c->th, U, part, n_obs, D, ncols, c->N, list, eta_out, ll_out)
  switch (c->glm_family * 2 + (small ? 1 : 0)) {
    case 0: AHMC_GLM_ETA(0, 64); break;
    case 1: AHMC_GLM_ETA(0, 16); break;
    case 2: AHMC_GLM_ETA(1, 64); break;
    case 3: AHMC_GLM_ETA(1, 16); break;
    case 4: AHMC_GLM_ETA(2, 64); break;
    case 5: AHMC_GLM_ETA(2, 16); break;
    default: return fail(c, AHMC_ERR_STATE, "glm: unknown family in the context");
  }
#undef AHMC_GLM_ETA
  HIPCHK(hipGetLastError());
  return AHMC_OK;
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
  if (!c->glm_buf) return fail(c, AHMC_ERR_STATE, "AHMC_TARGET_GLM without a model (ahmc_set_target_glm)");
  const int n_obs = (int)c->glm_nobs, D = (int)c->D, ns = glm_slices(c);
  const int64_t nrb = (n_obs + GB_M - 1) / GB_M, nrbD = (int64_t)(D + GB_M - 1) / GB_M * ns;
  int rc = glm_launch_eta(c, list, n, glm_small(c, nrb, n), (T*)nullptr, (T*)nullptr);
  if (rc) return rc;
  const T* b = c->glm_buf;
  const T* Xt = b + c->glm_off[GLM_XT];
  const T* U = b + c->glm_off[GLM_U];
  const T* prec = b + c->glm_off[GLM_PREC];
  T* gs = c->glm_buf + c->glm_off[GLM_GS];
  if (glm_small(c, nrbD, n))
    hipLaunchKernelGGL((k_glm_grad<T, 16>), dim3((unsigned)nrbD, (unsigned)((n + 15) / 16)), dim3(256), 0, c->stream, Xt, U, prec, (const T*)c->th, c->g, gs,
                       n_obs, D, n, c->N, list, ns);
  else
    hipLaunchKernelGGL((k_glm_grad<T, 64>), dim3((unsigned)(nrbD * (((n + GB_N - 1) / GB_N + 7) / 8 * 8))), dim3(256), 0, c->stream, Xt, U, prec,
                       (const T*)c->th, c->g, gs, n_obs, D, n, c->N, list, ns);
  if (ns > 1)
    hipLaunchKernelGGL((k_glm_gsum<T>), dim3((unsigned)((n * D + 255) / 256)), dim3(256), 0, c->stream, (const T*)gs, prec, (const T*)c->th, c->g, D, n, c->N,
                       list, ns);
  hipLaunchKernelGGL((k_glm_lp<T>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, b + c->glm_off[GLM_PART], prec, (const T*)c->th, c->lp, (int)nrb, D, n,
                     c->N, list, sanitize_lp ? 1 : 0);
  HIPCHK(hipGetLastError());
  return AHMC_OK;
}

template <class T>
int glm_set(Ctx<T>* c, int family, int64_t n_obs, const T* X, const T* y, const T* offset, const T* prec, double scale) {
  const int64_t D = c->D, N = c->N;
  if (family != AHMC_GLM_BERNOULLI_LOGIT && family != AHMC_GLM_POISSON_LOG && family != AHMC_GLM_GAUSSIAN_IDENTITY)
    return fail(c, AHMC_ERR_ARGUMENT, "set_target_glm: unknown family " + std::to_string(family));
  if (n_obs < 1) return fail(c, AHMC_ERR_ARGUMENT, "set_target_glm: n_obs must be >= 1; got " + std::to_string(n_obs));
  if (n_obs > AHMC_GLM_MAX_OBS)
    return fail(c, AHMC_ERR_UNSUPPORTED, "set_target_glm: n_obs = " + std::to_string(n_obs) + " is beyond the engine's limit AHMC_GLM_MAX_OBS = " +
                                             std::to_string((long long)AHMC_GLM_MAX_OBS));
  if (!X || !y) return fail(c, AHMC_ERR_ARGUMENT, "set_target_glm: X or y is NULL");
  if (!(std::isfinite(scale) && scale > 0)) return fail(c, AHMC_ERR_ARGUMENT, "set_target_glm: scale must be finite and > 0; got " + std::to_string(scale));
  // the slab: X, Xᵀ, y, offset, p, then the workspaces U, partial, gs
  const int64_t nrb = (n_obs + GB_M - 1) / GB_M, ns = (n_obs + GLM_K_SLICE - 1) / GLM_K_SLICE;
  const int64_t sizes[8] = {n_obs * D, n_obs * D, n_obs, n_obs, D, n_obs * N, nrb * N, ns > 1 ? ns * D * N : 0};
  int64_t off[8], total = 0;
  for (int i = 0; i < 8; ++i) {
    off[i] = total;
    total += (sizes[i] + 1) / 2 * 2;  // (16-byte alignment of every part, Float32 included)
  }
  const int64_t n_data = off[GLM_U];
  std::vector<T> h((size_t)n_data, T(0));
  HIPCHK(hipMemcpy(h.data() + off[GLM_X], X, sizeof(T) * n_obs * D, hipMemcpyDefault));
  HIPCHK(hipMemcpy(h.data() + off[GLM_Y], y, sizeof(T) * n_obs, hipMemcpyDefault));
  if (offset) HIPCHK(hipMemcpy(h.data() + off[GLM_OFF], offset, sizeof(T) * n_obs, hipMemcpyDefault));
  if (prec) HIPCHK(hipMemcpy(h.data() + off[GLM_PREC], prec, sizeof(T) * D, hipMemcpyDefault));
  const T* hX = h.data() + off[GLM_X];
  for (int64_t i = 0; i < n_obs * D; ++i)
    if (!std::isfinite((double)hX[i])) return fail(c, AHMC_ERR_ARGUMENT, "ArgumentError: X holds a non-finite value");
  for (int64_t i = 0; i < n_obs; ++i) {
    const double yi = (double)h[off[GLM_Y] + i];
    if (!std::isfinite((double)h[off[GLM_OFF] + i])) return fail(c, AHMC_ERR_ARGUMENT, "ArgumentError: offset holds a non-finite value");
    const bool ok = family == AHMC_GLM_BERNOULLI_LOGIT ? (yi >= 0 && yi <= 1) : family == AHMC_GLM_POISSON_LOG ? (std::isfinite(yi) && yi >= 0) : std::isfinite(yi);
    if (!ok)
      return fail(c, AHMC_ERR_ARGUMENT, "DomainError: y[" + std::to_string(i + 1) + "] = " + std::to_string(yi) + " is outside the family's domain (" +
                                            (family == AHMC_GLM_BERNOULLI_LOGIT ? "0 <= y <= 1" : family == AHMC_GLM_POISSON_LOG ? "y >= 0, finite" : "finite") + ")");
  }
  for (int64_t d = 0; d < D; ++d) {
    const double pd = (double)h[off[GLM_PREC] + d];
    if (!std::isfinite(pd)) return fail(c, AHMC_ERR_ARGUMENT, "ArgumentError: prior_prec holds a non-finite value");
    if (pd < 0) return fail(c, AHMC_ERR_ARGUMENT, "DomainError: prior_prec[" + std::to_string(d + 1) + "] = " + std::to_string(pd) + " is negative");
  }
  T* hXt = h.data() + off[GLM_XT];
  for (int64_t d = 0; d < D; ++d)
    for (int64_t i = 0; i < n_obs; ++i) hXt[d + i * D] = hX[i + d * n_obs];
  // everything that can fail happens before the previous target is touched
  T* buf = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&buf), sizeof(T) * (size_t)total) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, AHMC_ERR_RUNTIME, "set_target_glm: cannot allocate " + std::to_string((long long)(sizeof(T) * (size_t)total)) + " bytes for the model (" +
                                         std::to_string((long long)(sizeof(T) * (size_t)n_data)) + ") and its workspaces U (n_obs × N), partial and the slice sums");
  }
  if (hipMemcpy(buf, h.data(), sizeof(T) * (size_t)n_data, hipMemcpyHostToDevice) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
    (void)hipFree(buf);
    return fail(c, AHMC_ERR_RUNTIME, std::string("set_target_glm: copying the model failed: ") + hipGetErrorString(hipGetLastError()));
  }
  if (c->glm_buf) (void)hipFree(c->glm_buf);  // (the stream is idle)
  if (c->tparams) { (void)hipFree(c->tparams); c->tparams = nullptr; }
  c->glm_buf = buf;
  for (int i = 0; i < 8; ++i) c->glm_off[i] = off[i];
  c->glm_family = family;
  c->glm_nobs = n_obs;
  c->glm_has_offset = offset != nullptr;
  c->glm_scale = scale;
  c->target_kind = AHMC_TARGET_GLM;
  c->have_point = false;
  invalidate_schedule(c);
  return AHMC_OK;
}

template <class T>
int glm_pointwise(Ctx<T>* c, void* eta_out, void* ll_out) {
  if (c->target_kind != AHMC_TARGET_GLM || !c->glm_buf) return fail(c, AHMC_ERR_ARGUMENT, "glm_pointwise: no GLM is bound (ahmc_set_target_glm)");
  if (!eta_out && !ll_out) return AHMC_OK;
  const size_t n = (size_t)c->glm_nobs * (size_t)c->N;
  T* tmp = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&tmp), sizeof(T) * 2 * n) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, AHMC_ERR_RUNTIME, "glm_pointwise: cannot allocate " + std::to_string((long long)(sizeof(T) * 2 * n)) + " bytes");
  }
  const int64_t nrb = (c->glm_nobs + GB_M - 1) / GB_M;
  int rc = glm_launch_eta(c, (const int*)nullptr, c->N, glm_small(c, nrb, c->N), eta_out ? tmp : (T*)nullptr, ll_out ? tmp + n : (T*)nullptr);
  hipError_t e = hipSuccess;
  if (!rc && eta_out) e = hipMemcpyAsync(eta_out, tmp, sizeof(T) * n, hipMemcpyDefault, c->stream);
  if (!rc && e == hipSuccess && ll_out) e = hipMemcpyAsync(ll_out, tmp + n, sizeof(T) * n, hipMemcpyDefault, c->stream);
  const hipError_t es = hipStreamSynchronize(c->stream);
  (void)hipFree(tmp);
  if (rc) return rc;
  if (e != hipSuccess || es != hipSuccess) return fail(c, AHMC_ERR_RUNTIME, std::string("glm_pointwise: ") + hipGetErrorString(e != hipSuccess ? e : es));
  return AHMC_OK;
}
