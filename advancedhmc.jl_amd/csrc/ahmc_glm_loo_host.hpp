// ahmc_glm_loo_host.hpp — host side of include/ahmc_glm_loo.h (kernels: ahmc_glm_loo.hpp): the pointwise log-likelihood of a bound GLM
// at any (D, n_cols) array of draws, and PSIS-LOO / WAIC of it.  Included by ahmc_api.hip after ahmc_glm_host.hpp (the launches of the
// model's kernels) and ahmc_diag_host.hpp (dg_sort).

using namespace ahmc::loo;

// ℓ (n_obs, nc) of nc <= N draws th (D, nc), device memory, into ll_out (device memory): k_hglm_coef, the cutpoints kernel and
// k_glm_eta / k_glm_eta_cat on the model's own workspaces W, U, partial and the cutpoint table (stream-ordered with every evaluation)
template <class T>
int glm_loglik_chunk(Ctx<T>* c, const T* th, int64_t nc, T* ll_out) {
  const GlmModel<T>& m = c->glm;
  const int64_t nrb = (m.n_obs + GB_M - 1) / GB_M;
  const T* W = th;
  if (m.on_w()) {
    hipLaunchKernelGGL((k_hglm_coef<T>), dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, c->stream, th, m.tab(), m.at(GLM_W), (T*)nullptr, (int)m.P, m.G, c->D, nc,
                       (const int*)nullptr);
    W = m.at(GLM_W);
  }
  if (m.n_cat > 0) glm_launch_cut(c, (const int*)nullptr, nc, th);
  const bool small = glm_small(c, nrb, nc);
  return m.n_cls > 0 ? glm_launch_eta_cat(c, W, (const int*)nullptr, nc, small, (T*)nullptr, ll_out, (T*)nullptr)
                     : glm_launch_eta(c, W, (int)m.P, (const int*)nullptr, nc, small, (T*)nullptr, ll_out, th);
}

template <class T>
int glm_loo_check(Ctx<T>* c, const char* who, const void* theta, int64_t n_cols, const void* out) {
  const std::string w(who);
  if (c->target_kind != AHMC_TARGET_GLM || !c->glm.buf) return fail(c, AHMC_ERR_ARGUMENT, w + ": no GLM is bound (ahmc_set_target_glm)");
  if (n_cols < 0 || (n_cols > 0 && (!theta || !out))) return fail(c, AHMC_ERR_ARGUMENT, w + ": theta or the output is NULL, or n_cols < 0");
  if (n_cols > INT32_MAX) return fail(c, AHMC_ERR_UNSUPPORTED, w + ": n_cols beyond 2^31 - 1");
  return AHMC_OK;
}

// out (n_obs, n_cols): chunks of at most N columns, as glm_class_probs walks them
template <class T>
int glm_loglik(Ctx<T>* c, const void* theta, int64_t n_cols, void* out) {
  if (int rc = glm_loo_check(c, "glm_loglik", theta, n_cols, out)) return rc;
  if (n_cols == 0) return AHMC_OK;
  const GlmModel<T>& m = c->glm;
  const int64_t D = c->D, chunk = n_cols < c->N ? n_cols : c->N, n_obs = m.n_obs;
  const size_t elems = (size_t)((D + n_obs) * chunk);
  T* tmp = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&tmp), sizeof(T) * elems) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, AHMC_ERR_RUNTIME, "glm_loglik: cannot allocate " + std::to_string((long long)(sizeof(T) * elems)) + " bytes");
  }
  T* const ll = tmp + D * chunk;
  hipError_t e = hipSuccess;
  int rc = AHMC_OK;
  for (int64_t j0 = 0; j0 < n_cols && !rc && e == hipSuccess; j0 += chunk) {
    const int64_t nc = n_cols - j0 < chunk ? n_cols - j0 : chunk;
    e = hipMemcpyAsync(tmp, static_cast<const T*>(theta) + j0 * D, sizeof(T) * (size_t)(D * nc), hipMemcpyDefault, c->stream);
    if (e != hipSuccess) break;
    rc = glm_loglik_chunk(c, (const T*)tmp, nc, ll);
    if (!rc) e = hipMemcpyAsync(static_cast<T*>(out) + j0 * n_obs, ll, sizeof(T) * (size_t)(n_obs * nc), hipMemcpyDefault, c->stream);
  }
  const hipError_t es = hipStreamSynchronize(c->stream);
  (void)hipFree(tmp);
  if (rc) return rc;
  if (e != hipSuccess || es != hipSuccess) return fail(c, AHMC_ERR_RUNTIME, std::string("glm_loglik: ") + hipGetErrorString(e != hipSuccess ? e : es));
  return AHMC_OK;
}

// the tail length M = ⌈min(0.2·S, 3·√S)⌉ (glm.py: psis_tail_length — the same double operations)
inline int64_t loo_tail_length(int64_t S) {
  const double a = 0.2 * (double)S, b = 3.0 * std::sqrt((double)S);
  return (int64_t)std::ceil(a < b ? a : b);
}

// pointwise_out (4, n_obs) and log_weights_out (n_cols, n_obs) or NULL, both double
template <class T>
int glm_loo(Ctx<T>* c, const void* theta, int64_t n_cols, double* pw_out, double* lw_out) {
  if (int rc = glm_loo_check(c, "glm_loo", theta, n_cols, pw_out)) return rc;
  if (n_cols == 0) return AHMC_OK;
  const GlmModel<T>& m = c->glm;
  const int64_t D = c->D, S = n_cols, chunk = S < c->N ? S : c->N, n_obs = m.n_obs;
  if (n_obs > (int64_t)AHMC_GLM_LOO_MAX_VALUES / S)
    return fail(c, AHMC_ERR_UNSUPPORTED, "glm_loo: n_obs·n_cols = " + std::to_string((long long)n_obs) + "·" + std::to_string((long long)S) +
                                             " values; the sort's positions are 32 bits wide: the limit is AHMC_GLM_LOO_MAX_VALUES = 2^31 - 1");
  const int64_t M = loo_tail_length(S);
  if (M > AHMC_GLM_LOO_MAX_TAIL)
    return fail(c, AHMC_ERR_UNSUPPORTED, "glm_loo: n_cols = " + std::to_string((long long)S) + " draws have a tail of " + std::to_string((long long)M) +
                                             " values; the limit is AHMC_GLM_LOO_MAX_TAIL = " + std::to_string(AHMC_GLM_LOO_MAX_TAIL));
  static_assert(AHMC_GLM_LOO_MAX_TAIL == LOO_MAX_TAIL, "the header and the kernel disagree");
  // ---- the working set: one allocation
  const int64_t Mx = n_obs * S, tps = (S + DG_TILE - 1) / DG_TILE, L = n_obs * 256 * tps;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
  const size_t oTh = take(sizeof(T) * (size_t)(D * chunk)), oLl = take(sizeof(T) * (size_t)(n_obs * chunk)), oKA = take((size_t)Mx * 8), oKB = take((size_t)Mx * 8),
               oIA = take((size_t)Mx * 4), oIB = take((size_t)Mx * 4), oCnt = take((size_t)L * 4), oPart = take(((size_t)L / DG_SCAN_CHUNK + 2) * 4),
               oPw = take((size_t)n_obs * 32), oLw = take(lw_out ? (size_t)Mx * 8 : 0);
  DiagWorkspace ws;
  if (hipMalloc(&ws.p, off) != hipSuccess) {
    (void)hipGetLastError();
    ws.p = nullptr;
    return fail(c, AHMC_ERR_RUNTIME, "glm_loo: cannot allocate " + std::to_string((long long)off) + " bytes");
  }
  char* base = static_cast<char*>(ws.p);
  T* th = reinterpret_cast<T*>(base + oTh);
  T* ll = reinterpret_cast<T*>(base + oLl);
  uint64_t *ka = reinterpret_cast<uint64_t*>(base + oKA), *kb = reinterpret_cast<uint64_t*>(base + oKB);
  uint32_t *ia = reinterpret_cast<uint32_t*>(base + oIA), *ib = reinterpret_cast<uint32_t*>(base + oIB);
  uint32_t *cnt = reinterpret_cast<uint32_t*>(base + oCnt), *part = reinterpret_cast<uint32_t*>(base + oPart);
  double* pw = reinterpret_cast<double*>(base + oPw);
  double* lw = lw_out ? reinterpret_cast<double*>(base + oLw) : nullptr;
  hipStream_t s = c->stream;
  hipError_t e = hipSuccess;
  int rc = AHMC_OK;
  // ---- stage A
  const int64_t nbo = (n_obs + LOO_TILE - 1) / LOO_TILE;
  for (int64_t j0 = 0; j0 < S && !rc && e == hipSuccess; j0 += chunk) {
    const int64_t nc = S - j0 < chunk ? S - j0 : chunk;
    e = hipMemcpyAsync(th, static_cast<const T*>(theta) + j0 * D, sizeof(T) * (size_t)(D * nc), hipMemcpyDefault, s);
    if (e != hipSuccess) break;
    rc = glm_loglik_chunk(c, (const T*)th, nc, ll);
    if (rc) break;
    hipLaunchKernelGGL((k_loo_keys<T>), dim3((unsigned)(nbo * ((nc + LOO_TILE - 1) / LOO_TILE))), dim3(LOO_THREADS), 0, s, (const T*)ll, n_obs, nc, j0, S, ka, ia);
    e = hipGetLastError();
  }
  if (!rc && e == hipSuccess) {
    // ---- stage B: a float's key has its low 29 bits set by its sign alone, so the passes below bit 24 would move nothing
    dg_sort<uint64_t>(s, ka, kb, ia, ib, S, n_obs, tps, cnt, part, std::is_same<T, float>::value ? 24 : 0);
    // ---- stage C
    hipLaunchKernelGGL(k_loo_psis, dim3((unsigned)n_obs), dim3(LOO_THREADS), 0, s, (const uint64_t*)ka, (const uint32_t*)ia, S, (int)M, pw, lw);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(pw_out, pw, (size_t)n_obs * 32, hipMemcpyDefault, s);
    if (e == hipSuccess && lw_out) e = hipMemcpyAsync(lw_out, lw, (size_t)Mx * 8, hipMemcpyDefault, s);
  }
  const hipError_t es = hipStreamSynchronize(s);
  if (rc) return rc;
  if (e != hipSuccess || es != hipSuccess) return fail(c, AHMC_ERR_RUNTIME, std::string("glm_loo: ") + hipGetErrorString(e != hipSuccess ? e : es));
  return AHMC_OK;
}
