// quad_red.hip — the reduction and the scalar work of the four leaves of a quad step of k_nuts against the primitives they replace, on the
// same data (tests/test_leaf_quads.py).  Compiled with the engine's own flags (build.build_probe_object) and loaded through hipModuleLoad.
//
// pair form (the reference): wave64_pair_reduce_t + pair_leaf_stats on (a,b), the same on (c,d), wave64_any_le0_pair on the level-1 dot products;
// quad form: wave64_quad_reduce_t, then quad_leaf_stats (ahmc_device.hpp).
//
// in : 10 values per lane, lane-major: ea, eb, ec, ed (lane partials of four leaves' energies), dab0, dab1, dcd0, dcd1, dl0, dl1 (lane
//      partials of the U-turn dot products of the merges (a,b), (c,d) and of the level-1 merge)
// par: 2 values per wave: H0, delta_max
// out: 108 values per wave, written by lane 0: for LINW = 1 and then LINW = 0, 54 values each —
//      pair form [0..26]: the energy sums e_a .. e_d [0..3]; w, sa, dH of a, b, c, d [4..15]; redo, div of a, b, c, d [16..23];
//                         the U-turn decisions of (a,b), (c,d) and level 1 [24..26] (flags as 0 / 1)
//      quad form [27..53]: the same 27
// Launch with blockDim a multiple of 64 (whole waves) and n a multiple of 64.  No lane returns before a cross-lane operation: out-of-range lanes
// compute on zeros and store nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ahmc_device.hpp"

using namespace ahmc;

// the pair form: o[0..26]
template <class T, bool LINW>
__device__ __forceinline__ void pair_form(const T (&en)[4], const T (&dab)[2], const T (&dcd)[2], const T (&dl)[2], const T H0, const T dmax,
                                          T* __restrict__ o, bool store) {
  const T lim = sizeof(T) == 4 ? T(60) : T(600.0);
  constexpr int LA = 4 * AHMC_PAIR_RED_QUAD + 2, LB = 4 * AHMC_PAIR_RED_QUAD + 3;
  T z_ab, z_cd;
  const bool t_ab = wave64_pair_reduce_t(dab[0], dab[1], en[0], en[1], z_ab);
  const bool t_cd = wave64_pair_reduce_t(dcd[0], dcd[1], en[2], en[3], z_cd);
  const bool t_l1 = wave64_any_le0_pair(dl[0], dl[1]);
  PairLeafStats<T> pab, pcd;
  pair_leaf_stats<T, LINW>(z_ab, H0, dmax, lim, pab);
  pair_leaf_stats<T, LINW>(z_cd, H0, dmax, lim, pcd);
  const T e_ref[4] = {readlane_t<LA>(z_ab), readlane_t<LB>(z_ab), readlane_t<LA>(z_cd), readlane_t<LB>(z_cd)};
  if (store) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const PairLeafStats<T>& ps = i < 2 ? pab : pcd;
      const int j = i & 1;
      o[i] = e_ref[i];
      o[4 + 3 * i + 0] = ps.w[j];
      o[4 + 3 * i + 1] = ps.sa[j];
      o[4 + 3 * i + 2] = ps.dH[j];
      o[16 + 2 * i + 0] = ps.redo[j] ? T(1) : T(0);
      o[16 + 2 * i + 1] = ps.div[j] ? T(1) : T(0);
    }
    o[24] = t_ab ? T(1) : T(0);
    o[25] = t_cd ? T(1) : T(0);
    o[26] = t_l1 ? T(1) : T(0);
  }
}
// the quad form: o[0..26] of its own block
template <class T, bool LINW>
__device__ __forceinline__ void quad_form(const T (&en)[4], const T (&dab)[2], const T (&dcd)[2], const T (&dl)[2], const T H0, const T dmax,
                                          T* __restrict__ o, bool store) {
  const T lim = sizeof(T) == 4 ? T(60) : T(600.0);
  T w_t;
  const unsigned long long turns = wave64_quad_reduce_t(wave64_quad_pair(dab[0], dab[1]), wave64_quad_pair(dcd[0], dcd[1]), wave64_quad_pair(dl[0], dl[1]),
                                                        wave64_quad_pair(en[0], en[1]), wave64_quad_pair(en[2], en[3]), w_t);
  QuadLeafStats<T> qs;
  quad_leaf_stats<T, LINW>(w_t, H0, dmax, lim, qs);
  // Read with every lane active, as k_nuts reads them in wave-uniform control flow: under the lane-0 mask of `store` below the other
  // lanes' registers are not the compiler's to keep.
  const T e_q[4] = {readlane_t<4>(w_t), readlane_t<5>(w_t), readlane_t<6>(w_t), readlane_t<7>(w_t)};
  const T q_w[4] = {qs.w(0), qs.w(1), qs.w(2), qs.w(3)}, q_sa[4] = {qs.sa(0), qs.sa(1), qs.sa(2), qs.sa(3)}, q_dH[4] = {qs.dH(0), qs.dH(1), qs.dH(2), qs.dH(3)};
  if (store) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      o[i] = e_q[i];
      o[4 + 3 * i + 0] = q_w[i];
      o[4 + 3 * i + 1] = q_sa[i];
      o[4 + 3 * i + 2] = q_dH[i];
      o[16 + 2 * i + 0] = qs.redo(i) ? T(1) : T(0);
      o[16 + 2 * i + 1] = qs.div(i) ? T(1) : T(0);
    }
    o[24] = (turns & QUAD_TURN_AB) != 0ull ? T(1) : T(0);
    o[25] = (turns & QUAD_TURN_CD) != 0ull ? T(1) : T(0);
    o[26] = (turns & QUAD_TURN_L1) != 0ull ? T(1) : T(0);
  }
}

template <class T>
__device__ __forceinline__ void quad_body(const T* __restrict__ in, const T* __restrict__ par, T* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool ok = i < n;
  T v[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) v[k] = ok ? in[i * 10 + k] : T(0);
  const T en[4] = {v[0], v[1], v[2], v[3]}, dab[2] = {v[4], v[5]}, dcd[2] = {v[6], v[7]}, dl[2] = {v[8], v[9]};
  const long long wv = i >> 6;
  const T H0 = ok ? par[wv * 2 + 0] : T(0), dmax = ok ? par[wv * 2 + 1] : T(1);
  const bool store = ok && (threadIdx.x & 63u) == 0;
  T* o = out + wv * 108;
  pair_form<T, true>(en, dab, dcd, dl, H0, dmax, o, store);
  quad_form<T, true>(en, dab, dcd, dl, H0, dmax, o + 27, store);
  pair_form<T, false>(en, dab, dcd, dl, H0, dmax, o + 54, store);
  quad_form<T, false>(en, dab, dcd, dl, H0, dmax, o + 81, store);
}
#define PROBE_QUAD(NAME, T) \
  extern "C" __global__ __launch_bounds__(256) void NAME(const T* __restrict__ in, const T* __restrict__ par, T* __restrict__ out, long long n) { quad_body<T>(in, par, out, n); }
PROBE_QUAD(p_quad_red_f64, double)
PROBE_QUAD(p_quad_red_f32, float)
