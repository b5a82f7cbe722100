// ahmc_diag.hpp — MCMCChains' `summarystats` columns on the device (include/ahmc_diag.h): rank-normalised split-chain R̂ and the
// bulk / tail / basic ESS of Vehtari, Gelman, Simpson, Carpenter & Bürkner (2021), pooled over all N chains of a context, for the
// (D, N, K) draws buffer ahmc_sample writes.  The statistic is defined in advancedhmc.jl_amd/diagnostics.py (summarystats, the
// host mirror); this file computes the same numbers.
//
// Pipeline, per batch of B dimensions (each dimension one SEGMENT of S = 2N·⌊K/2⌋ values, split-chain order p = j·n + k):
//   k_dg_gather      transposing gather (D, N, K) → X (widened to double), order-preserving keys, u32 index p
//   radix sort       per 8-bit digit: k_dg_hist (per tile of one segment) → exclusive scan of the (segment, digit, tile) counts
//                    (k_sc_reduce / k_sc_parts / k_sc_apply) → k_dg_scatter (stable: wave match + per-wave counts in LDS).
//                    Tiles never straddle a segment, so one launch sorts every segment of the batch, whatever their sizes.
//   k_dg_segstat     non-finite check (NaN / ±Inf keys sort to the ends), median, q05, q95, split point of the folded merge
//   tie runs         run start = inclusive max-scan of "first of its run", run end = the same scan on the reversed order;
//                    k_dg_rank turns (start, end) into the average rank, z = Φ⁻¹((r − 3/8)/(S + 1/4)), scattered to p
//   k_dg_fold        merge-path merge of the reversed lower half (median − x) and the upper half (x − median): |x − median| in
//                    ascending order without a second sort; then the same tie-run ranking gives z_f
//   k_dg_moments     split-chain means and variances of x, z, z_f, I05, I95 (one wave per split chain)
//   k_dg_pool        W, B/n, var⁺, R̂, and the mean / std of x (one workgroup per (series, dimension), fixed reduction tree)
//   lag blocks       k_dg_acov (per workgroup slabs of Σ_j acov_j(t) for DG_LB = 64 lags, one per lane) → k_dg_acov_reduce (second pass over the
//                    slabs) → k_dg_finalize (Stan's truncation on the device); a readback of the per-series "done" flags stops
//                    the loop once every series has truncated
//   k_dg_output      the nine rows
//
// Every reduction runs in an order fixed by (N, K) alone: no float atomics, no inter-workgroup waiting, so the result is bit for
// bit the same from call to call and for every batching.  Integer LDS atomics count digits only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ahmc {
namespace diag {

constexpr int DG_THREADS = 256;
constexpr int DG_RADIX_ITEMS = 16;
constexpr int DG_TILE = DG_THREADS * DG_RADIX_ITEMS;  // keys per radix tile (one segment each)
constexpr int DG_SCAN_ITEMS = 16;
constexpr int DG_SCAN_CHUNK = DG_THREADS * DG_SCAN_ITEMS;
constexpr int DG_GATHER_TILE = 2048;  // elements of one gather tile (TDW dimensions × TKW draws of one chain)
constexpr int DG_FOLD_ITEMS = 8;      // merged outputs per thread after one merge-path search
constexpr int DG_LB = 64;             // lags per block of the autocovariance loop (one per lane)
constexpr int DG_CPW = 16;            // split chains per workgroup of k_dg_acov (4 waves × 4)
constexpr int DG_LDS_N = 1920;        // longest split chain staged in LDS by k_dg_acov (4 waves × n doubles ≤ 60 KiB, + 1 KiB static)
constexpr int DG_NSER = 5;            // series: 0 x, 1 z, 2 z_f, 3 I05, 4 I95
constexpr int DG_NESS = 4;            // series with an ESS: x, z, I05, I95
constexpr int DG_NOUT = 9;

__host__ __device__ inline int dg_ess_series(int e) { return e < 2 ? e : e + 1; }

// ---- order-preserving keys (−0.0 → +0.0 first, so the two zeros tie) --------------------------------------------------------
template <class T> struct KeyOf;
template <> struct KeyOf<float> { using K = uint32_t; };
template <> struct KeyOf<double> { using K = uint64_t; };

__device__ inline uint32_t to_key(float v) {
  const uint32_t u = __float_as_uint(v == 0.0f ? 0.0f : v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline uint64_t to_key(double v) {
  const uint64_t u = (uint64_t)__double_as_longlong(v == 0.0 ? 0.0 : v);
  return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
__device__ inline double from_key(uint32_t k) { return (double)__uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
__device__ inline double from_key(uint64_t k) {
  return __longlong_as_double((long long)((k & 0x8000000000000000ull) ? (k ^ 0x8000000000000000ull) : ~k));
}

// ---- Φ⁻¹: Wichura's AS241 (PPND16), the same operations in the same order as diagnostics._ndtri -----------------------------
__device__ inline double ppnd16(double p) {
#pragma clang fp contract(off)
  const double q = p - 0.5;
  if (fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    return q * (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                    4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                  1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) /
           (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                 2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
             4.2313330701600911252e+1) * r + 1.0);
  }
  double r = q < 0 ? p : 1.0 - p;
  if (!(r > 0)) return q < 0 ? -HUGE_VAL : HUGE_VAL;
  r = sqrt(-log(r));
  double v;
  if (r <= 5.0) {
    r = r - 1.6;
    v = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
            1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
          4.63033784615654529590e+0) * r + 1.42343711074968357734e+0) /
        (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
             1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
          2.05319162663775882187e+0) * r + 1.0);
  } else {
    r = r - 5.0;
    v = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
            2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
          5.46378491116411436990e+0) * r + 6.65790464350110377720e+0) /
        (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
             7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
          5.99832206555887937690e-1) * r + 1.0);
  }
  return q < 0 ? -v : v;
}

__device__ inline double dg_wave_sum(double v) {
  // butterfly: every lane ends with the same bits (a + b == b + a)
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// sum over the 256 threads of a workgroup in a fixed tree; every thread gets the total
__device__ inline double dg_block_sum(double v, double* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int o = DG_THREADS / 2; o >= 1; o >>= 1) {
    if (t < o) sh[t] = sh[t] + sh[t + o];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// ---- 1. gather ------------------------------------------------------------------------------------------------------------------
// One workgroup: TDW dimensions [d0 + dt·TDW, …) × TKW consecutive draws of chain c, through an LDS tile so that both the read
// (along d, the contiguous axis of the draws) and the write (along k, the contiguous axis of a split chain) are coalesced.
// Draw kk of chain c lands in split chain 2c (kk < n) or 2c + 1 (kk ≥ K − n); the middle draw of an odd K is dropped.
template <class T, class KT>
__global__ __launch_bounds__(DG_THREADS) void k_dg_gather(const T* __restrict__ draws, int64_t D, int64_t N, int64_t K, int64_t d0, int B,
                                                          int64_t n, int TDW, int64_t S, double* __restrict__ X, KT* __restrict__ keys,
                                                          uint32_t* __restrict__ idx) {
  __shared__ double tile[2 * DG_GATHER_TILE];  // TKW·(TDW + 1) ≤ 2·DG_GATHER_TILE (padded rows)
  const int TKW = DG_GATHER_TILE / TDW;
  const int64_t nkt = (K + TKW - 1) / TKW, ndt = (B + TDW - 1) / TDW;
  int64_t b = blockIdx.x;
  const int64_t kt = b % nkt;
  b /= nkt;
  const int64_t dt = b % ndt;
  const int64_t c = b / ndt;
  if (c >= N) return;
  const int t = threadIdx.x;
  const int64_t k0 = kt * TKW;
  const int s0 = (int)(dt * TDW);
  for (int e = t; e < DG_GATHER_TILE; e += DG_THREADS) {
    const int dd = e % TDW, kq = e / TDW;
    const int64_t kk = k0 + kq;
    if (s0 + dd < B && kk < K) tile[kq * (TDW + 1) + dd] = (double)draws[(d0 + s0 + dd) + D * c + D * N * kk];
  }
  __syncthreads();
  for (int e = t; e < DG_GATHER_TILE; e += DG_THREADS) {
    const int kq = e % TKW, dd = e / TKW;
    const int64_t kk = k0 + kq;
    if (s0 + dd >= B || kk >= K) continue;
    int64_t p;
    if (kk < n) p = (2 * c) * n + kk;
    else if (kk >= K - n) p = (2 * c + 1) * n + (kk - (K - n));
    else continue;
    const double v = tile[kq * (TDW + 1) + dd];
    const int64_t g = (int64_t)(s0 + dd) * S + p;
    X[g] = v;
    keys[g] = to_key((T)v);
    idx[g] = (uint32_t)p;
  }
}

// ---- 2. radix sort: histogram → scan → stable scatter (separate launches) ----------------------------------------------------------
// counts[(seg·256 + digit)·tps + tile]: the exclusive scan of this array in index order is each (segment, digit, tile)'s first
// output position, segments in order (segment s starts at s·S), digits in order inside a segment, tiles in order inside a digit.
template <class KT>
__global__ __launch_bounds__(DG_THREADS) void k_dg_hist(const KT* __restrict__ keys, int64_t S, int64_t tps, int shift, uint32_t* __restrict__ counts) {
  __shared__ uint32_t h[256];
  const int t = threadIdx.x;
  const int64_t seg = blockIdx.x / tps, tile = blockIdx.x % tps;
  const int64_t lo = seg * S + tile * DG_TILE, hi = seg * S + (S < (tile + 1) * DG_TILE ? S : (tile + 1) * DG_TILE);
  h[t] = 0;
  __syncthreads();
  for (int64_t i = lo + t; i < hi; i += DG_THREADS) atomicAdd(&h[(uint32_t)(keys[i] >> shift) & 255u], 1u);
  __syncthreads();
  counts[(seg * 256 + t) * tps + tile] = h[t];
}

template <class KT>
__global__ __launch_bounds__(DG_THREADS) void k_dg_scatter(const KT* __restrict__ kin, const uint32_t* __restrict__ iin, KT* __restrict__ kout,
                                                           uint32_t* __restrict__ iout, int64_t S, int64_t tps, int shift,
                                                           const uint32_t* __restrict__ offs) {
  __shared__ uint32_t base[256];
  __shared__ uint32_t wc[DG_THREADS / 64][256];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t seg = blockIdx.x / tps, tile = blockIdx.x % tps;
  const int64_t lo = seg * S + tile * DG_TILE, hi = seg * S + (S < (tile + 1) * DG_TILE ? S : (tile + 1) * DG_TILE);
  base[t] = offs[(seg * 256 + t) * tps + tile];
#pragma unroll
  for (int v = 0; v < DG_THREADS / 64; ++v) wc[v][t] = 0;
  __syncthreads();
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  for (int r = 0; r < DG_RADIX_ITEMS; ++r) {
    const int64_t i = lo + (int64_t)r * DG_THREADS + t;
    const bool valid = i < hi;
    KT key = 0;
    uint32_t id = 0, digit = 0;
    if (valid) { key = kin[i]; id = iin[i]; digit = (uint32_t)(key >> shift) & 255u; }
    // lanes of this wave holding the same digit (all lanes take part in every ballot)
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool on = (digit >> bit) & 1u;
      const uint64_t bal = __ballot(valid && on);
      peers &= on ? bal : ~bal;
    }
    const uint32_t below = (uint32_t)__popcll(peers & lt);
    if (valid && below == 0) wc[w][digit] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (valid) {
      uint32_t pos = base[digit] + below;
      for (int v = 0; v < w; ++v) pos += wc[v][digit];
      kout[pos] = key;
      iout[pos] = id;
    }
    __syncthreads();
    uint32_t add = 0;
#pragma unroll
    for (int v = 0; v < DG_THREADS / 64; ++v) { add += wc[v][t]; wc[v][t] = 0; }
    base[t] += add;
    __syncthreads();
  }
}

// ---- generic three-launch scan of u32 values (sum or max; identity 0 for both) --------------------------------------------------
// k_sc_reduce: one total per chunk of DG_SCAN_CHUNK; k_sc_parts: exclusive scan of the totals in ONE workgroup; k_sc_apply: the chunk
// again with its carry-in.  G: value at index i; W: where the (exclusive or inclusive) result of index i goes.
template <int MAXOP>
__device__ inline uint32_t sc_op(uint32_t a, uint32_t b) { return MAXOP ? (a > b ? a : b) : a + b; }

template <int MAXOP>
__device__ inline uint32_t sc_block_excl(uint32_t v, uint32_t* sh, uint32_t& total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int o = 1; o < DG_THREADS; o <<= 1) {
    const uint32_t a = t >= o ? sh[t - o] : 0u;
    __syncthreads();
    if (t >= o) sh[t] = sc_op<MAXOP>(sh[t], a);
    __syncthreads();
  }
  total = sh[DG_THREADS - 1];
  const uint32_t ex = t ? sh[t - 1] : 0u;
  __syncthreads();
  return ex;
}

template <int MAXOP, class G>
__global__ __launch_bounds__(DG_THREADS) void k_sc_reduce(G gen, int64_t L, uint32_t* __restrict__ part) {
  __shared__ uint32_t sh[DG_THREADS];
  const int64_t i0 = (int64_t)blockIdx.x * DG_SCAN_CHUNK + (int64_t)threadIdx.x * DG_SCAN_ITEMS;
  uint32_t a = 0;
  for (int e = 0; e < DG_SCAN_ITEMS; ++e)
    if (i0 + e < L) a = sc_op<MAXOP>(a, gen(i0 + e));
  uint32_t total;
  sc_block_excl<MAXOP>(a, sh, total);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

template <int MAXOP>
__global__ __launch_bounds__(DG_THREADS) void k_sc_parts(uint32_t* __restrict__ part, int64_t P) {
  __shared__ uint32_t sh[DG_THREADS];
  uint32_t carry = 0;
  for (int64_t c0 = 0; c0 < P; c0 += DG_SCAN_CHUNK) {
    const int64_t i0 = c0 + (int64_t)threadIdx.x * DG_SCAN_ITEMS;
    uint32_t v[DG_SCAN_ITEMS], a = 0;
    for (int e = 0; e < DG_SCAN_ITEMS; ++e) {
      v[e] = i0 + e < P ? part[i0 + e] : 0u;
      a = sc_op<MAXOP>(a, v[e]);
    }
    uint32_t total;
    uint32_t run = sc_op<MAXOP>(carry, sc_block_excl<MAXOP>(a, sh, total));
    for (int e = 0; e < DG_SCAN_ITEMS; ++e) {
      if (i0 + e < P) part[i0 + e] = run;
      run = sc_op<MAXOP>(run, v[e]);
    }
    carry = sc_op<MAXOP>(carry, total);
  }
}

template <int MAXOP, bool EXCL, class G, class W>
__global__ __launch_bounds__(DG_THREADS) void k_sc_apply(G gen, int64_t L, const uint32_t* __restrict__ part, W wr) {
  __shared__ uint32_t sh[DG_THREADS];
  const int64_t i0 = (int64_t)blockIdx.x * DG_SCAN_CHUNK + (int64_t)threadIdx.x * DG_SCAN_ITEMS;
  uint32_t v[DG_SCAN_ITEMS], a = 0;
  for (int e = 0; e < DG_SCAN_ITEMS; ++e) {
    v[e] = i0 + e < L ? gen(i0 + e) : 0u;
    a = sc_op<MAXOP>(a, v[e]);
  }
  uint32_t total;
  uint32_t run = sc_op<MAXOP>(part[blockIdx.x], sc_block_excl<MAXOP>(a, sh, total));
  for (int e = 0; e < DG_SCAN_ITEMS; ++e) {
    if (i0 + e >= L) break;
    if (EXCL) { wr(i0 + e, run); run = sc_op<MAXOP>(run, v[e]); }
    else { run = sc_op<MAXOP>(run, v[e]); wr(i0 + e, run); }
  }
}

struct GenArray {
  const uint32_t* a;
  __device__ uint32_t operator()(int64_t i) const { return a[i]; }
};
struct WrArray {
  uint32_t* a;
  __device__ void operator()(int64_t i, uint32_t v) const { a[i] = v; }
};
// "index of the first element of my run" (forward) and the same on the reversed order (r = M − 1 − g), for sorted keys / folded values.
// Segment boundaries are run boundaries.
template <class V>
struct EqOf {
  const V* v;
  __device__ bool operator()(int64_t a, int64_t b) const { return v[a] == v[b]; }
};
template <class E>
struct GenRunStart {
  E eq;
  int64_t S;
  __device__ uint32_t operator()(int64_t g) const { return (g % S == 0 || !eq(g, g - 1)) ? (uint32_t)g : 0u; }
};
template <class E>
struct GenRunEndRev {
  E eq;
  int64_t S, M;
  __device__ uint32_t operator()(int64_t r) const {
    const int64_t g = M - 1 - r;
    return (g % S == S - 1 || !eq(g, g + 1)) ? (uint32_t)r : 0u;
  }
};
struct WrRunEndRev {
  uint32_t* a;
  int64_t M;
  __device__ void operator()(int64_t r, uint32_t v) const { a[M - 1 - r] = (uint32_t)(M - 1 - (int64_t)v); }
};

// ---- 3. per-segment order statistics --------------------------------------------------------------------------------------------
// st[seg·4 + {0 finite, 1 median, 2 q05, 3 q95}], split[seg] = first sorted position with x ≥ median
template <class KT>
__global__ __launch_bounds__(64) void k_dg_segstat(const KT* __restrict__ keys, int64_t S, int B, double* __restrict__ st, uint32_t* __restrict__ split) {
#pragma clang fp contract(off)
  const int seg = blockIdx.x * 64 + threadIdx.x;
  if (seg >= B) return;
  const KT* x = keys + (int64_t)seg * S;
  // NaN keys sort beyond ±Inf (either sign), so a non-finite value anywhere puts one at an end
  const double lo = from_key(x[0]), hi = from_key(x[S - 1]);
  const bool finite = isfinite(lo) && isfinite(hi);
  const double med = (S & 1) ? from_key(x[S / 2]) : 0.5 * (from_key(x[S / 2 - 1]) + from_key(x[S / 2]));
  double q[2];
  const double pr[2] = {0.05, 0.95};
  for (int u = 0; u < 2; ++u) {
    const double h = (double)(S - 1) * pr[u];
    const int64_t l = (int64_t)floor(h);
    const int64_t hh = l + 1 < S - 1 ? l + 1 : S - 1;
    const double xl = from_key(x[l]), xh = from_key(x[hh]);
    q[u] = xl + (h - (double)l) * (xh - xl);
  }
  int64_t a = 0, b = S;
  while (a < b) {
    const int64_t mid = (a + b) / 2;
    if (from_key(x[mid]) < med) a = mid + 1;
    else b = mid;
  }
  st[seg * 4 + 0] = finite ? 1.0 : 0.0;
  st[seg * 4 + 1] = med;
  st[seg * 4 + 2] = q[0];
  st[seg * 4 + 3] = q[1];
  split[seg] = (uint32_t)a;
}

// ---- 4. average ranks → z, scattered back to the split-chain position ------------------------------------------------------------
__global__ __launch_bounds__(DG_THREADS) void k_dg_rank(const uint32_t* __restrict__ rs, const uint32_t* __restrict__ re, const uint32_t* __restrict__ idx,
                                                        int64_t S, int64_t M, double* __restrict__ z) {
#pragma clang fp contract(off)
  const int64_t g = (int64_t)blockIdx.x * DG_THREADS + threadIdx.x;
  if (g >= M) return;
  const int64_t seg = g / S;
  const double r = (double)(((int64_t)rs[g] - seg * S) + ((int64_t)re[g] - seg * S) + 2) * 0.5;
  z[seg * S + idx[g]] = ppnd16((r - 0.375) / ((double)S + 0.25));
}

// ---- 5. |x − median| in ascending order: merge path over A[t] = med − x[L−1−t] (t < L) and B[t] = x[L+t] − med ------------------
template <class KT>
__global__ __launch_bounds__(DG_THREADS) void k_dg_fold(const KT* __restrict__ keys, const uint32_t* __restrict__ idx, int64_t S, int B,
                                                        const double* __restrict__ st, const uint32_t* __restrict__ split,
                                                        double* __restrict__ fv, uint32_t* __restrict__ fi) {
#pragma clang fp contract(off)
  const int64_t cps = (S + DG_FOLD_ITEMS - 1) / DG_FOLD_ITEMS;
  const int64_t q = (int64_t)blockIdx.x * DG_THREADS + threadIdx.x;
  if (q >= cps * B) return;
  const int64_t seg = q / cps, k0 = (q % cps) * DG_FOLD_ITEMS;
  const KT* x = keys + seg * S;
  const double med = st[seg * 4 + 1];
  const int64_t na = split[seg], nb = S - na;
  auto A = [&](int64_t t) { return med - from_key(x[na - 1 - t]); };
  auto Bv = [&](int64_t t) { return from_key(x[na + t]) - med; };
  int64_t lo = k0 - nb > 0 ? k0 - nb : 0, hi = k0 < na ? k0 : na;
  while (lo < hi) {
    const int64_t mid = (lo + hi) / 2;
    if (A(mid) <= Bv(k0 - 1 - mid)) lo = mid + 1;
    else hi = mid;
  }
  int64_t i = lo, j = k0 - lo;
  for (int e = 0; e < DG_FOLD_ITEMS; ++e) {
    const int64_t k = k0 + e;
    if (k >= S) break;
    const bool takeA = j >= nb || (i < na && A(i) <= Bv(j));
    if (takeA) { fv[seg * S + k] = A(i); fi[seg * S + k] = idx[seg * S + na - 1 - i]; ++i; }
    else { fv[seg * S + k] = Bv(j); fi[seg * S + k] = idx[seg * S + na + j]; ++j; }
  }
}

// ---- 6. split-chain moments ---------------------------------------------------------------------------------------------------
__device__ inline double dg_val(int ser, const double* __restrict__ X, const double* __restrict__ Z, const double* __restrict__ ZF, double q05,
                                double q95, int64_t g) {
  switch (ser) {
    case 0: return X[g];
    case 1: return Z[g];
    case 2: return ZF[g];
    case 3: return X[g] <= q05 ? 1.0 : 0.0;
    default: return X[g] <= q95 ? 1.0 : 0.0;
  }
}

// one wave per (series, segment, split chain): cm / cv[(ser·B + seg)·m + j]
__global__ __launch_bounds__(DG_THREADS) void k_dg_moments(const double* __restrict__ X, const double* __restrict__ Z, const double* __restrict__ ZF,
                                                           const double* __restrict__ st, int B, int64_t m, int64_t n,
                                                           double* __restrict__ cm, double* __restrict__ cv) {
#pragma clang fp contract(off)
  const int64_t wid = ((int64_t)blockIdx.x * DG_THREADS + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wid >= (int64_t)DG_NSER * B * m) return;  // (uniform over the wave)
  const int64_t j = wid % m, sb = wid / m, seg = sb % B;
  const int ser = (int)(sb / B);
  const double q05 = st[seg * 4 + 2], q95 = st[seg * 4 + 3];
  const int64_t g0 = seg * (m * n) + j * n;
  double s = 0;
  for (int64_t k = lane; k < n; k += 64) s += dg_val(ser, X, Z, ZF, q05, q95, g0 + k);
  const double mean = dg_wave_sum(s) / (double)n;
  double ss = 0;
  for (int64_t k = lane; k < n; k += 64) {
    const double d = dg_val(ser, X, Z, ZF, q05, q95, g0 + k) - mean;
    ss += d * d;
  }
  const double var = dg_wave_sum(ss) / (double)(n - 1);
  if (lane == 0) { cm[wid] = mean; cv[wid] = var; }
}

// one workgroup per (series, segment): pool[(ser·B + seg)·4 + {0 ȳ, 1 W, 2 var⁺, 3 R̂}]; xs[seg·2 + {0 mean, 1 std}] of x
__global__ __launch_bounds__(DG_THREADS) void k_dg_pool(const double* __restrict__ cm, const double* __restrict__ cv, int B, int64_t m, int64_t n,
                                                        double* __restrict__ pool, double* __restrict__ xs) {
#pragma clang fp contract(off)
  __shared__ double sh[DG_THREADS];
  const int64_t sb = blockIdx.x;
  const double* a = cm + sb * m;
  const double* v = cv + sb * m;
  double s = 0;
  for (int64_t j = threadIdx.x; j < m; j += DG_THREADS) s += a[j];
  const double ybar = dg_block_sum(s, sh) / (double)m;
  double w = 0, b = 0;
  for (int64_t j = threadIdx.x; j < m; j += DG_THREADS) {
    w += v[j];
    const double d = a[j] - ybar;
    b += d * d;
  }
  const double sw = dg_block_sum(w, sh), sbb = dg_block_sum(b, sh);
  if (threadIdx.x != 0) return;
  const double W = sw / (double)m, Bn = sbb / (double)(m - 1);
  const double varp = (double)(n - 1) / (double)n * W + Bn;
  pool[sb * 4 + 0] = ybar;
  pool[sb * 4 + 1] = W;
  pool[sb * 4 + 2] = varp;
  pool[sb * 4 + 3] = W == 0 ? NAN : sqrt(varp / W);
  if (sb < B) {  // series x: the mean and the S − 1 standard deviation of all S values
    const double S = (double)(m * n);
    xs[sb * 2 + 0] = ybar;
    xs[sb * 2 + 1] = sqrt(((double)(n - 1) * sw + (double)n * sbb) / (S - 1.0));
  }
}

// ---- 7. autocovariances in lag blocks ---------------------------------------------------------------------------------------------
// workgroup (e, seg, g): split chains [g·DG_CPW, …); wave w takes chains g·DG_CPW + 4w … + 3 in order, lane l the lag t = t0 + l:
// Σ_k c_k c_{k+t} in ascending k (the centred chain staged in LDS when it fits: c_k is a broadcast, c_{k+t} consecutive), summed
// over the wave's chains in order; the four waves are then added in a fixed order → slab[((e·B + seg)·G + g)·DG_LB + l].
__global__ __launch_bounds__(DG_THREADS) void k_dg_acov(const double* __restrict__ X, const double* __restrict__ Z, const double* __restrict__ st,
                                                        const double* __restrict__ cm, const int32_t* __restrict__ done, int B, int64_t m,
                                                        int64_t n, int64_t G, int64_t t0, double* __restrict__ slab) {
#pragma clang fp contract(off)
  extern __shared__ double lds[];
  __shared__ double part[DG_THREADS / 64][DG_LB];
  const int64_t g = blockIdx.x % G, es = blockIdx.x / G;
  const int64_t seg = es % B;
  const int e = (int)(es / B), ser = dg_ess_series(e);
  if (done[es]) return;  // (uniform over the workgroup)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const double q05 = st[seg * 4 + 2], q95 = st[seg * 4 + 3];
  const bool staged = n <= DG_LDS_N;
  double* cl = lds + (int64_t)w * n;
  const int64_t t = t0 + lane;
  double acc = 0;
  for (int u = 0; u < DG_CPW / 4; ++u) {
    const int64_t j = g * DG_CPW + w * (DG_CPW / 4) + u;
    const bool active = j < m;  // (uniform over the wave; every wave reaches the barriers)
    const double mu = active ? cm[((int64_t)ser * B + seg) * m + j] : 0.0;
    const int64_t g0 = seg * (m * n) + j * n;
    if (staged) {
      if (active)
        for (int64_t k = lane; k < n; k += 64) cl[k] = dg_val(ser, X, Z, Z, q05, q95, g0 + k) - mu;
      __syncthreads();
    }
    if (active) {
      double s = 0;
      if (staged) {
#pragma unroll 4
        for (int64_t k = 0; k + t < n; ++k) s += cl[k] * cl[k + t];
      } else {
        // (the same arithmetic on values read from memory: y = src[k], or the indicator [src[k] <= q])
        const double* src = (ser == 1 ? Z : X) + g0;
        const bool ind = ser >= 3;
        const double qq = ser == 3 ? q05 : q95;
#pragma unroll 1
        for (int64_t k = 0; k + t < n; ++k) {
          double a = src[k], b = src[k + t];
          if (ind) { a = a <= qq ? 1.0 : 0.0; b = b <= qq ? 1.0 : 0.0; }
          s += (a - mu) * (b - mu);
        }
      }
      acc += s;
    }
    if (staged) __syncthreads();
  }
  part[w][lane] = acc;
  __syncthreads();
  if (threadIdx.x < DG_LB) {
    const int l = threadIdx.x;
    slab[(es * G + g) * DG_LB + l] = ((part[0][l] + part[1][l]) + part[2][l]) + part[3][l];
  }
}

// one workgroup per (e, seg, l): ρ̂(t0 + l) = 1 − (W − mean_j acov_j)/var⁺ → rho[(e·B + seg)·(n + 3) + t]
__global__ __launch_bounds__(DG_THREADS) void k_dg_acov_reduce(const double* __restrict__ slab, const double* __restrict__ pool,
                                                               const int32_t* __restrict__ done, int B, int64_t m, int64_t n, int64_t G,
                                                               int64_t t0, double* __restrict__ rho) {
#pragma clang fp contract(off)
  __shared__ double sh[DG_THREADS];
  const int l = blockIdx.x % DG_LB;
  const int64_t es = blockIdx.x / DG_LB;
  const int64_t t = t0 + l;
  if (done[es] || t >= n) return;  // (uniform)
  double s = 0;
  for (int64_t g = threadIdx.x; g < G; g += DG_THREADS) s += slab[(es * G + g) * DG_LB + l];
  s = dg_block_sum(s, sh);
  if (threadIdx.x != 0) return;
  const int64_t seg = es % B;
  const int ser = dg_ess_series((int)(es / B));
  const double* p = pool + ((int64_t)ser * B + seg) * 4;
  const double acov = s / (double)n / (double)m;
  rho[es * (n + 3) + t] = 1.0 - (p[1] - acov) / p[2];
}

// Stan's truncation (diagnostics._ess_from_rho) with the lags [0, avail) computed so far; a series that needs a later lag stays open.
__global__ __launch_bounds__(64) void k_dg_finalize(const double* __restrict__ rho_hat, const double* __restrict__ pool, const double* __restrict__ st,
                                                    int B, int64_t n, int64_t max_lag, int64_t avail, double* __restrict__ work,
                                                    int32_t* __restrict__ done, double* __restrict__ tau_out) {
#pragma clang fp contract(off)
  const int64_t es = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (es >= (int64_t)DG_NESS * B || done[es]) return;
  const int64_t seg = es % B;
  const int ser = dg_ess_series((int)(es / B));
  const double* p = pool + ((int64_t)ser * B + seg) * 4;
  if (st[seg * 4 + 0] == 0.0 || p[1] == 0.0) { tau_out[es] = NAN; done[es] = 1; return; }
  const double* R = rho_hat + es * (n + 3);
  double* rho = work + es * (n + 3);
  const int64_t need_all = avail >= n;
  for (int64_t i = 0; i < n + 3; ++i) rho[i] = 0.0;
  rho[0] = 1.0;
  if (!need_all && avail < 2) return;
  rho[1] = R[1];
  double even = 1.0, odd = rho[1];
  int64_t t = 1;
  const int64_t cap = max_lag == 0 ? n - 4 : (n - 4 < max_lag ? n - 4 : max_lag);
  while (t < cap && even + odd > 0) {
    if (!need_all && t + 2 >= avail) return;
    even = R[t + 1];
    odd = R[t + 2];
    if (even + odd >= 0) { rho[t + 1] = even; rho[t + 2] = odd; }
    t += 2;
  }
  const int64_t tmax = t;
  if (even > 0) rho[tmax + 1] = even;
  t = 1;
  while (t <= tmax - 3) {
    if (rho[t + 1] + rho[t + 2] > rho[t - 1] + rho[t]) {
      rho[t + 1] = (rho[t - 1] + rho[t]) / 2;
      rho[t + 2] = rho[t + 1];
    }
    t += 2;
  }
  double sum = 0;
  for (int64_t i = 0; i < tmax; ++i) sum += rho[i];
  const double tau = -1.0 + 2.0 * sum + rho[tmax + 1];
  tau_out[es] = tau;  // (ESS = min(S/τ, S·log10 S) is taken in k_dg_output)
  done[es] = 1;
}

// the nine rows for the batch's dimensions: out[s·D + d0 + seg]
__global__ __launch_bounds__(64) void k_dg_output(const double* __restrict__ st, const double* __restrict__ pool, const double* __restrict__ xs,
                                                  const double* __restrict__ tau, int B, int64_t S, int64_t D, int64_t d0, double* __restrict__ out) {
#pragma clang fp contract(off)
  const int seg = blockIdx.x * 64 + threadIdx.x;
  if (seg >= B) return;
  double v[DG_NOUT];
  const double Sd = (double)S, cap = Sd * log10(Sd);
  double ess[DG_NESS];
  for (int e = 0; e < DG_NESS; ++e) {
    const double tt = tau[(int64_t)e * B + seg];
    const double r = Sd / tt;
    ess[e] = isnan(tt) ? NAN : (r < cap ? r : cap);
  }
  const double rb = pool[((int64_t)1 * B + seg) * 4 + 3], rt = pool[((int64_t)2 * B + seg) * 4 + 3];
  v[0] = xs[seg * 2 + 0];
  v[1] = xs[seg * 2 + 1];
  v[2] = v[1] / sqrt(ess[0]);
  v[3] = ess[1];
  v[4] = (isnan(ess[2]) || isnan(ess[3])) ? NAN : (ess[2] < ess[3] ? ess[2] : ess[3]);
  v[5] = (isnan(rb) || isnan(rt)) ? NAN : (rb > rt ? rb : rt);
  v[6] = ess[0];
  v[7] = rb;
  v[8] = rt;
  const bool finite = st[seg * 4 + 0] != 0.0;
  for (int s = 0; s < DG_NOUT; ++s) out[s * D + d0 + seg] = finite ? v[s] : NAN;
}

// z (or z_f) of one dimension back in the draws' (K, N) order: out[c + N·k], NaN at a dropped middle draw
__global__ __launch_bounds__(DG_THREADS) void k_dg_rank_out(const double* __restrict__ z, const double* __restrict__ st, int64_t N, int64_t K,
                                                            int64_t n, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * DG_THREADS + threadIdx.x;
  if (i >= N * K) return;
  const int64_t c = i % N, kk = i / N;
  double v = NAN;
  if (st[0] != 0.0) {
    if (kk < n) v = z[(2 * c) * n + kk];
    else if (kk >= K - n) v = z[(2 * c + 1) * n + (kk - (K - n))];
  }
  out[i] = v;
}

}  // namespace diag
}  // namespace ahmc
