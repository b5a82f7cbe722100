// ahmc_glm_yrep_host.hpp — host side of include/ahmc_glm_yrep.h (kernels: ahmc_glm_yrep.hpp; the sampler: ahmc_glm_yrep_draw.hpp).
// ahmc_glm_yrep and ahmc_glm_yrep_summary are glm_predict_run (ahmc_glm_predict_host.hpp) with a GlmYrepCall: the same staging, checks,
// single allocation, chunk and draw walker, the planes the family's sampler reads made by k_glm_pred into the chunk's workspace, then
// glm_yrep_launch on them.  ahmc_glm_yrep_at runs the same launch on the caller's planes; it needs no bound model.  Included by
// ahmc_api.hip before ahmc_glm_predict_host.hpp.
#pragma once

// what makes a glm_predict_run a y_rep call
struct GlmYrepCall {
  uint64_t seed;
  bool summary;
};

// the one launch site of k_glm_yrep: the sampler arrives as a type
template <class T>
hipError_t glm_yrep_launch(hipStream_t s, int family, const GlmYrepArgs<T>& a) {
  const int64_t n = a.n_rows * a.n_cols;
  if (n == 0) return hipSuccess;
  const dim3 grid((unsigned)((n + 255) / 256));
  switch (yrep_sampler_of(family)) {
    case 0: hipLaunchKernelGGL((k_glm_yrep<T, 0>), grid, dim3(256), 0, s, a); break;
    case 1: hipLaunchKernelGGL((k_glm_yrep<T, 1>), grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((k_glm_yrep<T, 2>), grid, dim3(256), 0, s, a); break;
    case 4: hipLaunchKernelGGL((k_glm_yrep<T, 4>), grid, dim3(256), 0, s, a); break;
    case 5: hipLaunchKernelGGL((k_glm_yrep<T, 5>), grid, dim3(256), 0, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

constexpr int64_t GLM_YREP_AT_MAX = (int64_t)1 << 38;  // elements of one ahmc_glm_yrep_at call (the grid: 2^31 − 1 workgroups of 256)

template <class T>
int glm_yrep_at(Ctx<T>* c, int family, int n_categories, int64_t n, const void* q, const void* aux, const int32_t* row, const int32_t* col, uint64_t seed,
                void* y_out) {
  const std::string who = "glm_yrep_at";
  switch (yrep_at_refusal(family, n_categories, n, q != nullptr, aux != nullptr, y_out != nullptr)) {
    case 1: return fail(c, AHMC_ERR_ARGUMENT, who + ": unknown family " + std::to_string(family));
    case 2: return fail(c, AHMC_ERR_ARGUMENT, who + ": n_categories = " + std::to_string(n_categories) + " is outside 2 … 16");
    case 3: return fail(c, AHMC_ERR_ARGUMENT, who + ": q, y_out or the dispersion aux of a negative binomial is NULL");
    case 4: return fail(c, AHMC_ERR_ARGUMENT, who + ": n must be >= 0; got " + std::to_string((long long)n));
    default: break;
  }
  if (n > GLM_YREP_AT_MAX) return fail(c, AHMC_ERR_UNSUPPORTED, who + ": n beyond 2^38");
  if (n == 0) return AHMC_OK;
  const int planes = yrep_planes_of(family, n_categories);
  const bool has_aux = family == 4;
  size_t off = 0;
  const auto take = [&off](size_t bytes) {
    const size_t at = off;
    off += (bytes + 255) & ~(size_t)255;
    return at;
  };
  const size_t oq = take(sizeof(T) * (size_t)planes * (size_t)n), oa = take(has_aux ? sizeof(T) * (size_t)n : 0), orow = take(row ? 4 * (size_t)n : 0),
               ocol = take(col ? 4 * (size_t)n : 0), oy = take(sizeof(T) * (size_t)n);
  char* base = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&base), off) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, AHMC_ERR_RUNTIME, who + ": cannot allocate " + std::to_string((long long)off) + " bytes for the planes, the counters and the outcomes");
  }
  hipStream_t s = c->stream;
  hipError_t e = hipMemcpyAsync(base + oq, q, sizeof(T) * (size_t)planes * (size_t)n, hipMemcpyDefault, s);
  if (e == hipSuccess && has_aux) e = hipMemcpyAsync(base + oa, aux, sizeof(T) * (size_t)n, hipMemcpyDefault, s);
  if (e == hipSuccess && row) e = hipMemcpyAsync(base + orow, row, 4 * (size_t)n, hipMemcpyDefault, s);
  if (e == hipSuccess && col) e = hipMemcpyAsync(base + ocol, col, 4 * (size_t)n, hipMemcpyDefault, s);
  GlmYrepArgs<T> a{};
  a.q = reinterpret_cast<const T*>(base + oq);
  a.aux = has_aux ? reinterpret_cast<const T*>(base + oa) : nullptr;
  a.row = row ? reinterpret_cast<const int32_t*>(base + orow) : nullptr;
  a.col = col ? reinterpret_cast<const int32_t*>(base + ocol) : nullptr;
  a.y = reinterpret_cast<T*>(base + oy);
  a.n_rows = n;
  a.n_cols = 1;
  a.aux_ld = -1;
  a.col0 = 0;
  a.planes = planes;
  a.C = n_categories;
  a.k0 = (uint32_t)seed;
  a.k1 = (uint32_t)(seed >> 32);
  if (e == hipSuccess) e = glm_yrep_launch<T>(s, family, a);
  if (e == hipSuccess) e = hipMemcpyAsync(y_out, base + oy, sizeof(T) * (size_t)n, hipMemcpyDefault, s);
  const hipError_t es = hipStreamSynchronize(s);
  (void)hipFree(base);
  if (e != hipSuccess || es != hipSuccess) return fail(c, AHMC_ERR_RUNTIME, who + ": " + hipGetErrorString(e != hipSuccess ? e : es));
  return AHMC_OK;
}
