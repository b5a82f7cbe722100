// ahmc_glm_predict_host.hpp — host side of include/ahmc_glm_predict.h (kernels: ahmc_glm_predict.hpp; the host-only checks:
// ahmc_glm_predict_spec.hpp).  One function serves both calls: check, stage and check the new data, lay out and allocate the working
// set, then walk the draws in chunks (glm_walk_draws): the chunk's effective coefficients and cutpoint table on the working set's own
// arrays (the bound model's are sized by N and belong to the evaluations), k_glm_pred, and either the copy of the chunk's planes to the
// caller or k_glm_pred_fold.  Of the bound model's slab only the tables of the groups and the factors are read.  With a GlmYrepCall
// (ahmc_glm_yrep_host.hpp) the same walk serves include/ahmc_glm_yrep.h: the chunk's planes are those the family's sampler reads, they
// stay in the working set, k_glm_yrep draws from them, and the chunk's y_rep is copied to the caller or reduced per observation.
// Included by ahmc_api.hip after ahmc_glm_host.hpp and ahmc_glm_yrep_host.hpp.
#pragma once

static_assert(GLM_PRED_BLOCK == GLM_PRED_BN && GLM_PRED_BN == GB_N, "a block of the summary is the tile's 64 draws");

// The chunk is a multiple of 64 draws: as many as fit, with the rest of the working set, into AHMC_GLM_PREDICT_BUDGET bytes (default
// 256 MiB), at least 64; AHMC_GLM_PREDICT_CHUNK names it outright.  A budget given in the environment is binding: a working set of
// one block of draws that does not fit is refused like an allocation that failed.  Both are read at every call, so that a test can
// switch them (as AHMC_GLM_SMALL_BELOW).
inline int64_t glm_predict_env(const char* name) {
  const char* e = getenv(name);
  return e && *e ? atoll(e) : -1;
}

template <class T>
int glm_predict_run(Ctx<T>* c, const char* who, const ahmc_glm_newdata* nd, const void* theta, int64_t n_cols, int what, void* out, bool summary,
                    const GlmYrepCall* yr = nullptr) {
  const GlmModel<T>& m = c->glm;
  const bool bound = c->target_kind == AHMC_TARGET_GLM && m.buf;
  GlmPredPlan p;
  std::string err;
  if (int rc = glm_predict_spec_check(who, bound, m, nd, theta, n_cols, out, what, summary, p, err)) return fail(c, rc, err);
  if (p.n_new == 0) return AHMC_OK;
  const bool ysum = yr && yr->summary;
  if (yr && (m.family == AHMC_GLM_GAUSSIAN_IDENTITY || m.family == AHMC_GLM_GAUSSIAN_IDENTITY_SIGMA) && m.n_cat == 0 && m.n_cls == 0) p.q1 = p.Q;  // (μ, v)
  const int64_t n = p.n_new, K = m.K(), Px = m.Px, D = c->D, P = m.P, S = n_cols;
  // ---- the new data on the host, checked
  std::vector<T> hX((size_t)(n * Px)), hoff(p.has_offset ? (size_t)(n * K) : 0), hy(p.has_y ? (size_t)n : 0);
  HIPCHK(hipMemcpy(hX.data(), nd->X, sizeof(T) * hX.size(), hipMemcpyDefault));
  if (p.has_offset) HIPCHK(hipMemcpy(hoff.data(), nd->offset, sizeof(T) * hoff.size(), hipMemcpyDefault));
  if (p.has_y) HIPCHK(hipMemcpy(hy.data(), nd->y, sizeof(T) * hy.size(), hipMemcpyDefault));
  if (int rc = glm_predict_spec_data<T>(who, m, p, hX.data(), p.has_offset ? hoff.data() : nullptr, p.has_y ? hy.data() : nullptr, err)) return fail(c, rc, err);
  if (S == 0) return AHMC_OK;
  // ---- the chunk and the working set: one allocation
  const int64_t nq = p.planes(), Q = p.Q, Cm1 = m.n_cat > 0 ? m.n_cat - 1 : 0, nrb = (n + GB_M - 1) / GB_M;
  const int64_t col_elems = D + (m.on_w() ? P : 0) + 3 * Cm1 + (m.n_cls > 0 ? K * n : 0) + (summary ? 0 : nq * n) + (yr ? n : 0);
  const double col_bytes = (double)sizeof(T) * (double)col_elems + (summary ? (double)(nq * n) * 16.0 / 64.0 : 0.0) + (ysum ? (double)(n * sizeof(GlmYrepPart)) / 64.0 : 0.0);
  const auto layout = [&](int64_t chunk, size_t* o) {
    size_t off = 0;
    const auto take = [&off](size_t bytes) {
      const size_t at = off;
      off += (bytes + 255) & ~(size_t)255;
      return at;
    };
    o[0] = take(sizeof(T) * (size_t)(n * Px));                              // X
    o[1] = take(sizeof(T) * hoff.size());                                   // offset
    o[2] = take(sizeof(T) * hy.size());                                     // y
    o[3] = take(sizeof(int) * (size_t)(n * m.F));                           // levels
    o[4] = take(sizeof(T) * (size_t)(D * chunk));                           // θ of the chunk
    o[5] = take(m.on_w() ? sizeof(T) * (size_t)(P * chunk) : 0);            // W
    o[6] = take(sizeof(T) * (size_t)(3 * Cm1 * chunk));                     // the cutpoint table
    o[7] = take(m.n_cls > 0 ? sizeof(T) * (size_t)(K * n * chunk) : 0);     // a categorical model's predictors
    o[8] = take(summary ? 0 : sizeof(T) * (size_t)(nq * n * chunk));        // the chunk's planes
    o[9] = take(summary ? (size_t)(nq * n * (chunk / 64)) * 16 : 0);        // the block partials
    o[10] = take(summary ? (size_t)(nq * n) * 16 : 0);                      // the running state
    o[11] = take(summary ? (size_t)((2 * Q + 1) * n) * 8 : 0);              // the summary
    o[12] = take(yr ? sizeof(T) * (size_t)(n * chunk) : 0);                 // y_rep of the chunk
    o[13] = take(ysum ? (size_t)(n * (chunk / 64)) * sizeof(GlmYrepPart) : 0);  // its block partials
    o[14] = take(ysum ? (size_t)n * sizeof(GlmYrepPart) : 0);               // the running state of y_rep's summary
    o[15] = take(ysum ? (size_t)(4 * n) * 8 : 0);                           // y_rep's summary
    return off;
  };
  size_t o[16];
  const int64_t env_budget = glm_predict_env("AHMC_GLM_PREDICT_BUDGET"), env_chunk = glm_predict_env("AHMC_GLM_PREDICT_CHUNK");
  const double budget = env_budget >= 0 ? (double)env_budget : 256.0 * 1024 * 1024;
  int64_t chunk = 64;
  if (env_chunk > 0) {
    chunk = (env_chunk + 63) / 64 * 64;
  } else {
    const double room = budget - (double)layout(0, o);
    if (room > 64.0 * col_bytes) chunk = (int64_t)(room / col_bytes / 64.0) * 64;
  }
  const int64_t grid_cols = ((int64_t)INT32_MAX / nrb - 8) * 64;  // (the grid is row blocks × 8·⌈column blocks/8⌉ workgroups)
  if (chunk > grid_cols) chunk = grid_cols;
  if (chunk > (S + 63) / 64 * 64) chunk = (S + 63) / 64 * 64;
  const size_t total = layout(chunk, o);
  const std::string parts = std::string(" bytes for the new data, one chunk of ") + std::to_string((long long)chunk) + " draws (θ" + (m.on_w() ? ", W" : "") +
                            (Cm1 ? ", the cutpoint table" : "") + (m.n_cls > 0 ? ", the classes' predictors" : "") +
                            (summary ? "), the block partials and the running state" : ") and its planes of the matrix") +
                            (ysum ? ", y_rep of the chunk, its block partials and running state" : yr ? " and y_rep of the chunk" : "");
  if (env_budget >= 0 && (double)total > budget)
    return fail(c, AHMC_ERR_RUNTIME, std::string(who) + ": cannot allocate " + std::to_string((long long)total) + parts + " within AHMC_GLM_PREDICT_BUDGET = " +
                                         std::to_string((long long)env_budget));
  char* base = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&base), total) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, AHMC_ERR_RUNTIME, std::string(who) + ": cannot allocate " + std::to_string((long long)total) + parts);
  }
  const auto at = [&](int i) { return reinterpret_cast<T*>(base + o[i]); };
  T* th = at(4);
  double2* part = reinterpret_cast<double2*>(base + o[9]);
  double2* state = reinterpret_cast<double2*>(base + o[10]);
  double* sum = reinterpret_cast<double*>(base + o[11]);
  hipStream_t s = c->stream;
  GlmWalk w;
  w.e = hipMemcpyAsync(at(0), hX.data(), sizeof(T) * hX.size(), hipMemcpyHostToDevice, s);
  if (w.ok() && p.has_offset) w.e = hipMemcpyAsync(at(1), hoff.data(), sizeof(T) * hoff.size(), hipMemcpyHostToDevice, s);
  if (w.ok() && p.has_y) w.e = hipMemcpyAsync(at(2), hy.data(), sizeof(T) * hy.size(), hipMemcpyHostToDevice, s);
  if (w.ok() && m.F > 0) w.e = hipMemcpyAsync(base + o[3], nd->levels, sizeof(int) * (size_t)(n * m.F), hipMemcpyHostToDevice, s);
  GlmPredArgs<T> a{};
  a.X = at(0);
  a.y = p.has_y ? at(2) : nullptr;
  a.off = p.has_offset ? at(1) : nullptr;
  a.lev = reinterpret_cast<const int*>(base + o[3]);
  a.ft = m.F > 0 ? m.ftab() : nullptr;
  a.W = m.on_w() ? at(5) : th;
  a.aux = m.aux ? th + (D - 1) : nullptr;
  a.cut = at(6);
  a.eta_ws = at(7);
  a.out = at(8);
  a.part = part;
  a.scale = (T)m.scale;
  a.n_new = (int)n;
  a.Px = (int)Px;
  a.Pb = m.n_cls > 0 ? (int)(P / K) : 0;
  a.K = (int)K;
  a.Cm1 = (int)Cm1;
  a.Q = (int)Q;
  a.q0 = p.q0;
  a.q1 = p.q1;
  a.ldw = m.on_w() ? P : D;
  a.ldt = D;
  a.nc_cap = chunk;
  a.nblk_cap = chunk / 64;
  const int fam = m.n_cls > 0 ? 6 : m.n_cat > 0 ? 5 : m.family;
  // the one launch site: the family, the factors and the kind of epilogue arrive as types
  const auto launch = [&](auto fam_c, auto fac_c, auto sum_c, const dim3 grid) {
    hipLaunchKernelGGL((k_glm_pred<T, decltype(fam_c)::value, decltype(fac_c)::value, decltype(sum_c)::value>), grid, dim3(256), 0, s, a);
  };
  const auto by_kind = [&](auto fam_c, const dim3 grid) {
    using Yes = std::true_type;
    using No = std::false_type;
    if (m.F > 0 && summary) launch(fam_c, Yes{}, Yes{}, grid);
    else if (m.F > 0) launch(fam_c, Yes{}, No{}, grid);
    else if (summary) launch(fam_c, No{}, Yes{}, grid);
    else launch(fam_c, No{}, No{}, grid);
  };
  if (w.ok())
    w = glm_walk_draws(c, theta, S, chunk, th, [&](GlmWalk& st, int64_t j0, int64_t nc) {
      if (m.on_w())
        hipLaunchKernelGGL((k_hglm_coef<T>), dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, s, (const T*)th, m.tab(), at(5), (T*)nullptr, (int)P, m.G, D, nc, (const int*)nullptr);
      if (Cm1 > 0)
        hipLaunchKernelGGL((k_glm_cut<T>), dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, s, (const T*)th, D, D - Cm1, (int)Cm1, at(6), chunk, nc, (const int*)nullptr, 1);
      const int64_t nblk = (nc + 63) / 64;
      const dim3 grid((unsigned)(nrb * ((nblk + 7) / 8 * 8)));
      a.ncols = nc;
      switch (fam) {
        case 0: by_kind(std::integral_constant<int, 0>{}, grid); break;
        case 1: by_kind(std::integral_constant<int, 1>{}, grid); break;
        case 2: by_kind(std::integral_constant<int, 2>{}, grid); break;
        case 3: by_kind(std::integral_constant<int, 3>{}, grid); break;
        case 4: by_kind(std::integral_constant<int, 4>{}, grid); break;
        case 5: by_kind(std::integral_constant<int, 5>{}, grid); break;
        case 6: by_kind(std::integral_constant<int, 6>{}, grid); break;
        default: st.rc = fail(c, AHMC_ERR_STATE, std::string(who) + ": unknown family in the context"); return;
      }
      st.e = hipGetLastError();
      if (st.e != hipSuccess) return;
      if (summary) {
        hipLaunchKernelGGL(k_glm_pred_fold, dim3((unsigned)((nq * n + 255) / 256)), dim3(256), 0, s, (const double2*)part, state, sum, (int)n, (int)Q, (int)nq, nblk,
                           chunk / 64, j0 / 64, S, j0 == 0 ? 1 : 0, j0 + nc == S ? 1 : 0);
        st.e = hipGetLastError();
      } else if (yr) {
        GlmYrepArgs<T> ya{};
        ya.q = at(8);
        ya.aux = a.aux;
        ya.y = at(12);
        ya.n_rows = n;
        ya.n_cols = nc;
        ya.aux_ld = D;
        ya.col0 = j0;
        ya.planes = (int)nq;
        ya.C = m.n_cat > 0 ? m.n_cat : m.n_cls;
        ya.k0 = (uint32_t)yr->seed;
        ya.k1 = (uint32_t)(yr->seed >> 32);
        st.e = glm_yrep_launch<T>(s, fam, ya);
        if (st.e != hipSuccess) return;
        if (ysum) {
          GlmYrepPart* ypart = reinterpret_cast<GlmYrepPart*>(base + o[13]);
          hipLaunchKernelGGL((k_glm_yrep_blocks<T>), dim3((unsigned)(nrb * nblk)), dim3(256), 0, s, (const T*)at(12), (const T*)a.y, ypart, (int)n, nc, chunk / 64);
          hipLaunchKernelGGL(k_glm_yrep_fold, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const GlmYrepPart*)ypart, reinterpret_cast<GlmYrepPart*>(base + o[14]),
                             reinterpret_cast<double*>(base + o[15]), (int)n, nblk, chunk / 64, j0 / 64, S, j0 == 0 ? 1 : 0, j0 + nc == S ? 1 : 0, p.has_y ? 1 : 0);
          st.e = hipGetLastError();
        } else {
          st.e = hipMemcpyAsync(static_cast<T*>(out) + j0 * n, at(12), sizeof(T) * (size_t)(n * nc), hipMemcpyDefault, s);
        }
      } else {
        st.e = hipMemcpyAsync(static_cast<T*>(out) + j0 * nq * n, at(8), sizeof(T) * (size_t)(nq * n * nc), hipMemcpyDefault, s);
      }
    });
  if (w.ok() && ysum) w.e = hipMemcpyAsync(out, base + o[15], (size_t)(4 * n) * 8, hipMemcpyDefault, s);
  if (w.ok() && summary) {
    if (!p.has_y) hipLaunchKernelGGL(k_glm_pred_no_lpd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, sum, (int)n, (int)Q);
    w.e = hipGetLastError();
    if (w.e == hipSuccess) w.e = hipMemcpyAsync(out, sum, (size_t)((2 * Q + 1) * n) * 8, hipMemcpyDefault, s);
  }
  const hipError_t es = hipStreamSynchronize(s);
  (void)hipFree(base);
  if (w.rc) return w.rc;
  if (w.e != hipSuccess || es != hipSuccess) return fail(c, AHMC_ERR_RUNTIME, std::string(who) + ": " + hipGetErrorString(w.e != hipSuccess ? w.e : es));
  return AHMC_OK;
}
