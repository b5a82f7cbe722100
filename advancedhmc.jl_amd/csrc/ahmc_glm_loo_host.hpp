// ahmc_glm_loo_host.hpp — host side of include/ahmc_glm_loo.h (kernels: ahmc_glm_loo.hpp): the pointwise log-likelihood of a bound GLM
// at any (D, n_cols) array of draws, and PSIS-LOO / WAIC of it.  Included by ahmc_api.hip after ahmc_glm_host.hpp (glm_forward, the
// draw walker and its argument check) and ahmc_diag_host.hpp (dg_sort).

using namespace ahmc::loo;

template <class T>
int glm_loo_check(Ctx<T>* c, const char* who, const void* theta, int64_t n_cols, const void* out) {
  return glm_draws_check(c, who, true, "no GLM is bound (ahmc_set_target_glm)", !theta || !out, "theta or the output is NULL, or", n_cols);
}

// out (n_obs, n_cols): chunks of at most N columns, each through glm_forward on the model's own workspaces W, U, partial and the
// cutpoint table (stream-ordered with every evaluation)
template <class T>
int glm_loglik(Ctx<T>* c, const void* theta, int64_t n_cols, void* out) {
  if (int rc = glm_loo_check(c, "glm_loglik", theta, n_cols, out)) return rc;
  if (n_cols == 0) return AHMC_OK;
  const int64_t n_obs = c->glm.n_obs;
  return glm_on_draws(c, "glm_loglik", theta, n_cols, n_cols < c->N ? n_cols : c->N, n_obs, [&](GlmWalk& w, const T* th, T* ll, int64_t j0, int64_t nc) {
    w.rc = glm_forward(c, th, (const int*)nullptr, nc, (T*)nullptr, ll, (T*)nullptr);
    if (!w.rc) w.e = hipMemcpyAsync(static_cast<T*>(out) + j0 * n_obs, ll, sizeof(T) * (size_t)(n_obs * nc), hipMemcpyDefault, c->stream);
  });
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
  // ---- stage A
  const int64_t nbo = (n_obs + LOO_TILE - 1) / LOO_TILE;
  GlmWalk w = glm_walk_draws(c, theta, S, chunk, th, [&](GlmWalk& st, int64_t j0, int64_t nc) {
    st.rc = glm_forward(c, (const T*)th, (const int*)nullptr, nc, (T*)nullptr, ll, (T*)nullptr);
    if (st.rc) return;
    hipLaunchKernelGGL((k_loo_keys<T>), dim3((unsigned)(nbo * ((nc + LOO_TILE - 1) / LOO_TILE))), dim3(LOO_THREADS), 0, s, (const T*)ll, n_obs, nc, j0, S, ka, ia);
    st.e = hipGetLastError();
  });
  if (w.ok()) {
    // ---- stage B: a float's key has its low 29 bits set by its sign alone, so the passes below bit 24 would move nothing
    dg_sort<uint64_t>(s, ka, kb, ia, ib, S, n_obs, tps, cnt, part, std::is_same<T, float>::value ? 24 : 0);
    // ---- stage C
    hipLaunchKernelGGL(k_loo_psis, dim3((unsigned)n_obs), dim3(LOO_THREADS), 0, s, (const uint64_t*)ka, (const uint32_t*)ia, S, (int)M, pw, lw);
    w.e = hipGetLastError();
    if (w.e == hipSuccess) w.e = hipMemcpyAsync(pw_out, pw, (size_t)n_obs * 32, hipMemcpyDefault, s);
    if (w.e == hipSuccess && lw_out) w.e = hipMemcpyAsync(lw_out, lw, (size_t)Mx * 8, hipMemcpyDefault, s);
  }
  const hipError_t es = hipStreamSynchronize(s);
  if (w.rc) return w.rc;
  if (w.e != hipSuccess || es != hipSuccess) return fail(c, AHMC_ERR_RUNTIME, std::string("glm_loo: ") + hipGetErrorString(w.e != hipSuccess ? w.e : es));
  return AHMC_OK;
}
