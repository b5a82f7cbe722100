// pair_stats.hip — the scalar work of the two leaves of a pair step of k_nuts in its two forms, on the same data
// (tests/test_pair_lane_stats.py).  Compiled with the engine's own flags (build.build_probe_object) and loaded through hipModuleLoad.
//
// serial form (the engine's until round 10; it lives on here): wave64_pair_reduce, then the lines of the scalar block of k_nuts' single-leaf arm on each of the two broadcast
//   energies, one after the other — BOTH leaves always (the engine drops leaf b when leaf a diverges; the probe compares what is computed);
// lane-parallel form: wave64_pair_reduce_t, then pair_leaf_stats (ahmc_device.hpp).
//
// in : 4 values per lane, lane-major: ea, eb (lane partials of two leaves' energies), da, db (lane partials of the two U-turn dot products)
// par: 2 values per wave: H0, delta_max
// out: 42 values per wave, written by lane 0: for LINW = 1 and then LINW = 0, 21 values each —
//      serial [0..9]:  w_a, sa_a, dH_a, w_b, sa_b, dH_b, redo_a, div_a, redo_b, div_b (flags as 0 / 1)
//      lane-parallel [10..19]: the same ten;  [20]: 1 where the two reductions took the same U-turn decision
// Launch with blockDim a multiple of 64 (whole waves) and n a multiple of 64.  No lane returns before a cross-lane operation: out-of-range lanes
// compute on zeros and store nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ahmc_device.hpp"

using namespace ahmc;

// k_nuts' leaf_stats (ahmc_nuts.hpp), the lines that compute: the limit is LINW_LIMIT there (600; Float32: 60)
template <class T, bool LINW>
__device__ __forceinline__ void serial_leaf(const T ne, const T H0, const T delta_max, T& w, T& sa, T& dH, bool& redo, bool& div) {
  dH = -ne - H0;
  T sa_leaf = 0;
  if constexpr (!LINW) sa_leaf = alpha_from_logweight<T, true>(H0 + ne);
  redo = false;
  if constexpr (LINW) {
    const T lw = H0 + ne;
    w = leaf_weight_exp<true>(lw);
    sa_leaf = w >= T(1) ? T(1) : w;
    redo = __builtin_amdgcn_ballot_w64(lw > (sizeof(T) == 4 ? T(60) : T(600.0))) != 0;
  } else {
    w = H0 + ne;
  }
  div = __builtin_amdgcn_ballot_w64(!(-H0 < delta_max + ne)) != 0;
  sa = sa_leaf;
}

template <class T, bool LINW>
__device__ __forceinline__ void both_forms(const T ea, const T eb, const T da, const T db, const T H0, const T dmax, T* __restrict__ o, bool store) {
  T sa_ = ea, sb_ = eb;
  const bool t_ser = wave64_pair_reduce(da, db, sa_, sb_);
  T w[2], sa[2], dH[2];
  bool redo[2], div[2];
  serial_leaf<T, LINW>(neg_energy_sanitized(sa_), H0, dmax, w[0], sa[0], dH[0], redo[0], div[0]);
  serial_leaf<T, LINW>(neg_energy_sanitized(sb_), H0, dmax, w[1], sa[1], dH[1], redo[1], div[1]);
  T z;
  const bool t_par = wave64_pair_reduce_t(da, db, ea, eb, z);
  PairLeafStats<T> ps;
  pair_leaf_stats<T, LINW>(z, H0, dmax, sizeof(T) == 4 ? T(60) : T(600.0), ps);
  if (store) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      o[3 * i + 0] = w[i];
      o[3 * i + 1] = sa[i];
      o[3 * i + 2] = dH[i];
      o[6 + 2 * i + 0] = redo[i] ? T(1) : T(0);
      o[6 + 2 * i + 1] = div[i] ? T(1) : T(0);
      o[10 + 3 * i + 0] = ps.w[i];
      o[10 + 3 * i + 1] = ps.sa[i];
      o[10 + 3 * i + 2] = ps.dH[i];
      o[16 + 2 * i + 0] = ps.redo[i] ? T(1) : T(0);
      o[16 + 2 * i + 1] = ps.div[i] ? T(1) : T(0);
    }
    o[20] = t_ser == t_par ? T(1) : T(0);
  }
}

template <class T>
__device__ __forceinline__ void stats_body(const T* __restrict__ in, const T* __restrict__ par, T* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool ok = i < n;
  const T ea = ok ? in[i * 4 + 0] : T(0), eb = ok ? in[i * 4 + 1] : T(0);
  const T da = ok ? in[i * 4 + 2] : T(0), db = ok ? in[i * 4 + 3] : T(0);
  const long long wv = i >> 6;
  const T H0 = ok ? par[wv * 2 + 0] : T(0), dmax = ok ? par[wv * 2 + 1] : T(1);
  const bool store = ok && (threadIdx.x & 63u) == 0;
  T* o = out + wv * 42;
  both_forms<T, true>(ea, eb, da, db, H0, dmax, o, store);
  both_forms<T, false>(ea, eb, da, db, H0, dmax, o + 21, store);
}
#define PROBE_STATS(NAME, T) \
  extern "C" __global__ __launch_bounds__(256) void NAME(const T* __restrict__ in, const T* __restrict__ par, T* __restrict__ out, long long n) { stats_body<T>(in, par, out, n); }
PROBE_STATS(p_pair_stats_f64, double)
PROBE_STATS(p_pair_stats_f32, float)
