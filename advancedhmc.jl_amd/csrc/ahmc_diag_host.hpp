// ahmc_diag_host.hpp — host side of include/ahmc_diag.h: argument checks, the workspace plan and the launch sequence of the
// kernels in ahmc_diag.hpp (see there for the pipeline).  Included by ahmc_api.hip after the context and the reductions' helpers.
//
// Workspace: one allocation per call, bounded by min(16 GiB, half of the free device memory), or by AHMC_DIAG_WORKSPACE_MB (read
// per call; the tests force small batches with it).  Dimensions go through in batches of as many as fit, and never more than
// 2³¹ − 1 values per batch (u32 positions).

using namespace ahmc::diag;

struct DiagWorkspace {
  void* p = nullptr;
  ~DiagWorkspace() {
    if (p) (void)hipFree(p);
  }
};

// exclusive (EXCL) or inclusive scan of L values: three launches, no inter-workgroup waiting
template <int MAXOP, bool EXCL, class G, class W>
static void dg_scan(hipStream_t s, G gen, int64_t L, W wr, uint32_t* part) {
  const int64_t P = (L + DG_SCAN_CHUNK - 1) / DG_SCAN_CHUNK;
  hipLaunchKernelGGL((k_sc_reduce<MAXOP, G>), dim3((unsigned)P), dim3(DG_THREADS), 0, s, gen, L, part);
  hipLaunchKernelGGL((k_sc_parts<MAXOP>), dim3(1), dim3(DG_THREADS), 0, s, part, P);
  hipLaunchKernelGGL((k_sc_apply<MAXOP, EXCL, G, W>), dim3((unsigned)P), dim3(DG_THREADS), 0, s, gen, L, part, wr);
}

// Stable ascending LSD radix sort of (key, position) in every one of `nseg` segments of S values, 8 bits per pass from bit `shift0`
// (bits below it: the same in every key, or a function of the bits above).  Tiles never straddle a segment.  The result is in (ka, ia)
// after an even number of passes, else in (kb, ib): the references are swapped to name it.  cnt: nseg·256·tps counters.
template <class KT>
static void dg_sort(hipStream_t s, KT*& ka, KT*& kb, uint32_t*& ia, uint32_t*& ib, int64_t S, int64_t nseg, int64_t tps, uint32_t* cnt, uint32_t* part,
                    int shift0 = 0) {
  const int64_t ntiles = nseg * tps, L = nseg * 256 * tps;
  for (int shift = shift0; shift < (int)(8 * sizeof(KT)); shift += 8) {
    hipLaunchKernelGGL((k_dg_hist<KT>), dim3((unsigned)ntiles), dim3(DG_THREADS), 0, s, ka, S, tps, shift, cnt);
    dg_scan<0, true>(s, GenArray{cnt}, L, WrArray{cnt}, part);
    hipLaunchKernelGGL((k_dg_scatter<KT>), dim3((unsigned)ntiles), dim3(DG_THREADS), 0, s, ka, ia, kb, ib, S, tps, shift, cnt);
    std::swap(ka, kb);
    std::swap(ia, ib);
  }
}

// average ranks of the tie runs of a sorted batch (eq: equality of sorted neighbours) → Φ⁻¹ → z[seg·S + idx[g]]
template <class E>
static void dg_rank_runs(hipStream_t s, E eq, int64_t S, int64_t M, const uint32_t* idx, uint32_t* rs, uint32_t* re, uint32_t* part, double* z) {
  dg_scan<1, false>(s, GenRunStart<E>{eq, S}, M, WrArray{rs}, part);
  dg_scan<1, false>(s, GenRunEndRev<E>{eq, S, M}, M, WrRunEndRev{re, M}, part);
  hipLaunchKernelGGL(k_dg_rank, dim3((unsigned)((M + DG_THREADS - 1) / DG_THREADS)), dim3(DG_THREADS), 0, s, rs, re, idx, S, M, z);
}

// dsel < 0: ahmc_diag_summary (the nine rows of every dimension into out[9·D]); dsel >= 0: ahmc_diag_rank_normalize of dimension
// dsel (z, or z_f if folded) into out[K·N]
template <class T>
int diag_impl(Ctx<T>* c, const void* draws, int64_t K, int64_t max_lag, int64_t dsel, int folded, double* out, const char* what) {
  using KT = typename KeyOf<T>::K;
  const std::string w(what);
  if (!draws || !out) return fail(c, AHMC_ERR_ARGUMENT, w + ": NULL argument");
  if (K < 4) return fail(c, AHMC_ERR_ARGUMENT, w + ": at least 4 draws per chain");
  if (max_lag < 0) return fail(c, AHMC_ERR_ARGUMENT, w + ": max_lag must be >= 0 (0: no cap)");
  if (dsel >= 0 && dsel >= c->D) return fail(c, AHMC_ERR_ARGUMENT, w + ": dimension out of range");
  if (dsel < -1) return fail(c, AHMC_ERR_ARGUMENT, w + ": dimension out of range");
  if (folded != 0 && folded != 1) return fail(c, AHMC_ERR_ARGUMENT, w + ": folded must be 0 or 1");
  hipPointerAttribute_t at;
  const bool dev = hipPointerGetAttributes(&at, draws) == hipSuccess && at.type == hipMemoryTypeDevice;
  (void)hipGetLastError();
  if (!dev) return fail(c, AHMC_ERR_ARGUMENT, w + ": draws must be the device buffer ahmc_sample filled");
  if (c->comm_ranks > 1)
    return fail(c, AHMC_ERR_UNSUPPORTED, w + ": the context has a communicator of " + std::to_string(c->comm_ranks) +
                                             " ranks; ranks pooled across ranks are not implemented (one rank's chains only)");
  const int64_t N = c->N, D = c->D, n = K / 2, m = 2 * N, S = m * n;
  if (S > (int64_t)INT32_MAX)
    return fail(c, AHMC_ERR_UNSUPPORTED, w + ": 2·N·⌊K/2⌋ = " + std::to_string(S) + " values per dimension; the limit is 2^31 - 1");
  const int64_t d_first = dsel >= 0 ? dsel : 0, d_end = dsel >= 0 ? dsel + 1 : D, nd = d_end - d_first;

  // ---- workspace plan
  const int64_t tps = (S + DG_TILE - 1) / DG_TILE, G = (m + DG_CPW - 1) / DG_CPW;
  const size_t ks = sizeof(KT);
  const size_t per_dim = (size_t)S * (48 + 2 * ks) + (size_t)tps * 256 * 4 + ((size_t)S / DG_SCAN_CHUNK + (size_t)tps * 256 / DG_SCAN_CHUNK + 2) * 4 + (size_t)DG_NSER * m * 16 +
                         (size_t)DG_NESS * G * DG_LB * 8 + (size_t)DG_NESS * (n + 3) * 16 + 256;
  size_t budget;
  if (const char* e = getenv("AHMC_DIAG_WORKSPACE_MB")) {
    budget = (size_t)(atoll(e) > 0 ? atoll(e) : 1) << 20;
  } else {
    size_t fr = 0, tot = 0;
    HIPCHK(hipMemGetInfo(&fr, &tot));
    budget = std::min<size_t>((size_t)16 << 30, fr / 2);
  }
  int64_t B = (int64_t)(budget / per_dim);
  B = std::max<int64_t>(1, std::min<int64_t>({B, nd, (int64_t)INT32_MAX / S}));
  const int64_t Mx = B * S;
  const size_t fixed = dsel >= 0 ? (size_t)K * N * 8 : (size_t)DG_NOUT * D * 8;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
  const size_t oX = take(Mx * 8), oKA = take(Mx * ks), oKB = take(Mx * ks), oIA = take(Mx * 4), oIB = take(Mx * 4), oZ = take(Mx * 8),
               oZF = take(Mx * 8), oFV = take(Mx * 8), oRS = take(Mx * 4), oRE = take(Mx * 4), oCnt = take((size_t)B * 256 * tps * 4),
               oPart = take((std::max<size_t>((size_t)Mx, (size_t)B * 256 * tps) / DG_SCAN_CHUNK + 2) * 4), oCM = take((size_t)DG_NSER * B * m * 8),
               oCV = take((size_t)DG_NSER * B * m * 8), oSlab = take((size_t)DG_NESS * B * G * DG_LB * 8),
               oRho = take((size_t)DG_NESS * B * (n + 3) * 8), oWork = take((size_t)DG_NESS * B * (n + 3) * 8), oSt = take((size_t)B * 32),
               oSplit = take((size_t)B * 4), oXs = take((size_t)B * 16), oDone = take((size_t)DG_NESS * B * 4),
               oTau = take((size_t)DG_NESS * B * 8), oPool = take((size_t)DG_NSER * B * 32), oOut = take(fixed);
  DiagWorkspace ws;
  {
    const hipError_t e = hipMalloc(&ws.p, off);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      ws.p = nullptr;
      return fail(c, AHMC_ERR_RUNTIME, w + ": hipMalloc of " + std::to_string(off >> 20) + " MiB of workspace failed (" + hipGetErrorString(e) +
                                           "); set AHMC_DIAG_WORKSPACE_MB lower");
    }
  }
  char* base = static_cast<char*>(ws.p);
  double* X = reinterpret_cast<double*>(base + oX);
  KT* KA = reinterpret_cast<KT*>(base + oKA);
  KT* KB = reinterpret_cast<KT*>(base + oKB);
  uint32_t* IA = reinterpret_cast<uint32_t*>(base + oIA);
  uint32_t* IB = reinterpret_cast<uint32_t*>(base + oIB);
  double* Z = reinterpret_cast<double*>(base + oZ);
  double* ZF = reinterpret_cast<double*>(base + oZF);
  double* FV = reinterpret_cast<double*>(base + oFV);
  uint32_t* RS = reinterpret_cast<uint32_t*>(base + oRS);
  uint32_t* RE = reinterpret_cast<uint32_t*>(base + oRE);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(base + oCnt);
  uint32_t* part = reinterpret_cast<uint32_t*>(base + oPart);
  double* cm = reinterpret_cast<double*>(base + oCM);
  double* cv = reinterpret_cast<double*>(base + oCV);
  double* slab = reinterpret_cast<double*>(base + oSlab);
  double* rho = reinterpret_cast<double*>(base + oRho);
  double* work = reinterpret_cast<double*>(base + oWork);
  double* st = reinterpret_cast<double*>(base + oSt);
  uint32_t* split = reinterpret_cast<uint32_t*>(base + oSplit);
  double* xs = reinterpret_cast<double*>(base + oXs);
  int32_t* done = reinterpret_cast<int32_t*>(base + oDone);
  double* tau = reinterpret_cast<double*>(base + oTau);
  double* pool = reinterpret_cast<double*>(base + oPool);
  double* dout = reinterpret_cast<double*>(base + oOut);
  hipStream_t s = c->stream;
  std::vector<int32_t> hdone;

  for (int64_t d0 = d_first; d0 < d_end; d0 += B) {
    const int Bb = (int)std::min<int64_t>(B, d_end - d0);
    const int64_t M = (int64_t)Bb * S;
    // 1. gather
    int TDW = 1;
    while (TDW < Bb && TDW < 32) TDW <<= 1;
    const int64_t TKW = DG_GATHER_TILE / TDW, ngather = N * ((Bb + TDW - 1) / TDW) * ((K + TKW - 1) / TKW);
    hipLaunchKernelGGL((k_dg_gather<T, KT>), dim3((unsigned)ngather), dim3(DG_THREADS), 0, s, static_cast<const T*>(draws), D, N, K, d0, Bb, n,
                       TDW, S, X, KA, IA);
    // 2. LSD radix sort of (key, position), 8 bits per pass; an even number of passes leaves the result in (KA, IA)
    KT *ksrc = KA, *kdst = KB;
    uint32_t *isrc = IA, *idst = IB;
    dg_sort<KT>(s, ksrc, kdst, isrc, idst, S, Bb, tps, cnt, part);
    // 3. order statistics; 4. z; 5. z_f
    hipLaunchKernelGGL((k_dg_segstat<KT>), dim3((unsigned)((Bb + 63) / 64)), dim3(64), 0, s, KA, S, Bb, st, split);
    dg_rank_runs(s, EqOf<KT>{KA}, S, M, IA, RS, RE, part, Z);
    const int64_t nfold = ((S + DG_FOLD_ITEMS - 1) / DG_FOLD_ITEMS) * Bb;
    hipLaunchKernelGGL((k_dg_fold<KT>), dim3((unsigned)((nfold + DG_THREADS - 1) / DG_THREADS)), dim3(DG_THREADS), 0, s, KA, IA, S, Bb, st, split,
                       FV, IB);
    dg_rank_runs(s, EqOf<double>{FV}, S, M, IB, RS, RE, part, ZF);
    if (dsel >= 0) {
      hipLaunchKernelGGL(k_dg_rank_out, dim3((unsigned)((N * K + DG_THREADS - 1) / DG_THREADS)), dim3(DG_THREADS), 0, s, folded ? ZF : Z, st, N, K,
                         n, dout);
      continue;
    }
    // 6. split-chain moments, R̂
    const int64_t nwaves = (int64_t)DG_NSER * Bb * m;
    hipLaunchKernelGGL(k_dg_moments, dim3((unsigned)((nwaves * 64 + DG_THREADS - 1) / DG_THREADS)), dim3(DG_THREADS), 0, s, X, Z, ZF, st, Bb, m, n, cm,
                       cv);
    hipLaunchKernelGGL(k_dg_pool, dim3((unsigned)(DG_NSER * Bb)), dim3(DG_THREADS), 0, s, cm, cv, Bb, m, n, pool, xs);
    // 7. autocovariances in lag blocks until every series has truncated
    HIPCHK(hipMemsetAsync(done, 0, sizeof(int32_t) * DG_NESS * Bb, s));
    const size_t shmem = n <= DG_LDS_N ? (size_t)(DG_THREADS / 64) * n * 8 : 0;
    hdone.assign((size_t)DG_NESS * Bb, 0);
    for (int64_t t0 = 0; t0 < n; t0 += DG_LB) {
      hipLaunchKernelGGL(k_dg_acov, dim3((unsigned)(DG_NESS * Bb * G)), dim3(DG_THREADS), shmem, s, X, Z, st, cm, done, Bb, m, n, G, t0, slab);
      hipLaunchKernelGGL(k_dg_acov_reduce, dim3((unsigned)(DG_NESS * Bb * DG_LB)), dim3(DG_THREADS), 0, s, slab, pool, done, Bb, m, n, G, t0, rho);
      const int64_t avail = std::min<int64_t>(n, t0 + DG_LB);
      hipLaunchKernelGGL(k_dg_finalize, dim3((unsigned)((DG_NESS * Bb + 63) / 64)), dim3(64), 0, s, rho, pool, st, Bb, n, max_lag, avail, work, done,
                         tau);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(hdone.data(), done, sizeof(int32_t) * hdone.size(), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      if (std::all_of(hdone.begin(), hdone.end(), [](int32_t v) { return v != 0; })) break;
    }
    hipLaunchKernelGGL(k_dg_output, dim3((unsigned)((Bb + 63) / 64)), dim3(64), 0, s, st, pool, xs, tau, Bb, S, D, d0, dout);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, dout, fixed, hipMemcpyDefault, s));
  HIPCHK(hipStreamSynchronize(s));
  return AHMC_OK;
}
