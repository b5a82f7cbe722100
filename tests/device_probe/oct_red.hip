// oct_red.hip — the reduction and the scalar work of the eight leaves of an octo step of k_nuts against the primitives they replace, on the
// same data (tests/test_leaf_octs.py).  Compiled with the engine's own flags (build.build_probe_object) and loaded through hipModuleLoad.
//
// quad form (the reference): wave64_quad_reduce_t + quad_leaf_stats on (a,b,c,d), the same on (e,f,g,h), wave64_any_le0_pair on the level-2
//                            dot products;
// octo form: wave64_oct_rows_de + wave64_oct_rows on each half, wave64_oct_reduce_t, then oct_leaf_stats (ahmc_device.hpp);
// half form: the octo form with the first half's row given as the second half's too — how k_nuts runs the quad step of the third doubling
//            in the kernels with the octo step; leaves a .. d and their three decisions are compared.
//
// in : 22 values per lane, lane-major: e_a .. e_h [0..7] (lane partials of eight leaves' energies), then the lane partials of the U-turn dot
//      products of the seven merges, two each: (a,b), (c,d), level 1 of (abcd), (e,f), (g,h), level 1 of (efgh), level 2 [8..21]
// par: 2 values per wave: H0, delta_max
// out: 354 values per wave, written by lane 0: for LINW = 1 and then LINW = 0, 177 values each —
//      quad form [0..58]: the energy sums e_a .. e_h [0..7]; w, sa, dH of a .. h [8..31]; redo, div of a .. h [32..47]; the U-turn decisions
//                         in the order of `in` [48..54]; 55..58 unused (0)
//      octo form [59..117]: the same 59
//      half form [118..176]: the same layout, leaves a .. d and decisions 48..50 written, the rest left as the caller filled it
// Launch with blockDim a multiple of 64 (whole waves) and n a multiple of 64.  No lane returns before a cross-lane operation: out-of-range lanes
// compute on zeros and store nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ahmc_device.hpp"

using namespace ahmc;

constexpr int OCT_BLOCK = 59;

// one leaf's seven values / the seven decisions, stored by lane 0.  The values are wave-uniform (scalar registers): they are stored leaf by
// leaf, as they are read, so that no wrapper holds all of a form's scalars at once and spills them.
template <class T>
__device__ __forceinline__ void store_leaf(T* __restrict__ o, const int i, const T e, const T w, const T sa, const T dH, const bool redo, const bool div, bool store) {
  if (store) {
    o[i] = e;
    o[8 + 3 * i + 0] = w;
    o[8 + 3 * i + 1] = sa;
    o[8 + 3 * i + 2] = dH;
    o[32 + 2 * i + 0] = redo ? T(1) : T(0);
    o[32 + 2 * i + 1] = div ? T(1) : T(0);
  }
}
template <class T>
__device__ __forceinline__ void store_turns(T* __restrict__ o, const unsigned turn_bits, bool store) {
  if (store) {
#pragma unroll
    for (int m = 0; m < 7; ++m) o[48 + m] = ((turn_bits >> m) & 1u) != 0u ? T(1) : T(0);
#pragma unroll
    for (int m = 55; m < OCT_BLOCK; ++m) o[m] = T(0);
  }
}

// the quad form: two quad reductions with their passes, and the level-2 merge's predicate
template <class T, bool LINW>
__device__ __forceinline__ void quad_form(const T (&v)[22], const T H0, const T dmax, T* __restrict__ o, bool store) {
  const T lim = sizeof(T) == 4 ? T(60) : T(600.0);
  unsigned turn_bits = 0u;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int d = 8 + 6 * h;
    T w_t;
    const unsigned long long turns =
        wave64_quad_reduce_t(wave64_quad_pair(v[d + 0], v[d + 1]), wave64_quad_pair(v[d + 2], v[d + 3]), wave64_quad_pair(v[d + 4], v[d + 5]),
                             wave64_quad_pair(v[4 * h + 0], v[4 * h + 1]), wave64_quad_pair(v[4 * h + 2], v[4 * h + 3]), w_t);
    QuadLeafStats<T> qs;
    quad_leaf_stats<T, LINW>(w_t, H0, dmax, lim, qs);
    // (each value is read with every lane active, as k_nuts reads them in wave-uniform control flow, and stored under the lane-0 mask behind it)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const T e = readlane_at(w_t, 4 + k), w = qs.w(k), sa = qs.sa(k), dH = qs.dH(k);
      store_leaf(o, 4 * h + k, e, w, sa, dH, qs.redo(k), qs.div(k), store);
    }
    turn_bits |= ((turns & QUAD_TURN_AB) != 0ull ? 1u : 0u) << (3 * h);
    turn_bits |= ((turns & QUAD_TURN_CD) != 0ull ? 2u : 0u) << (3 * h);
    turn_bits |= ((turns & QUAD_TURN_L1) != 0ull ? 4u : 0u) << (3 * h);
  }
  if (wave64_any_le0_pair(v[20], v[21])) turn_bits |= 64u;
  store_turns(o, turn_bits, store);
}
// the octo form
template <class T, bool LINW>
__device__ __forceinline__ void oct_form(const T (&v)[22], const T H0, const T dmax, T* __restrict__ o, bool store) {
  const T lim = sizeof(T) == 4 ? T(60) : T(600.0);
  const T xl1 = wave64_quad_pair(v[12], v[13]);
  const T h1 = wave64_oct_rows(wave64_oct_rows_de(wave64_quad_pair(v[8], v[9]), wave64_quad_pair(v[10], v[11]), wave64_quad_pair(v[0], v[1]),
                                                  wave64_quad_pair(v[2], v[3])), xl1, xl1);
  const T h2 = wave64_oct_rows(wave64_oct_rows_de(wave64_quad_pair(v[14], v[15]), wave64_quad_pair(v[16], v[17]), wave64_quad_pair(v[4], v[5]),
                                                  wave64_quad_pair(v[6], v[7])), wave64_quad_pair(v[18], v[19]), wave64_quad_pair(v[20], v[21]));
  T w_t;
  const unsigned long long turns = wave64_oct_reduce_t(h1, h2, w_t);
  OctLeafStats<T> os;
  oct_leaf_stats<T, LINW>(w_t, H0, dmax, lim, os);
  // Each value is read with every lane active, as k_nuts reads them in wave-uniform control flow: under the lane-0 mask of `store` the other
  // lanes' registers are not the compiler's to keep.
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const T e = readlane_at(w_t, OctLeafStats<T>::lane_of(k)), w = os.w(k), sa = os.sa(k), dH = os.dH(k);
    store_leaf(o, k, e, w, sa, dH, os.redo(k), os.div(k), store);
  }
  constexpr unsigned long long M[7] = {OCT_TURN_AB, OCT_TURN_CD, OCT_TURN_ABCD, OCT_TURN_EF, OCT_TURN_GH, OCT_TURN_EFGH, OCT_TURN_L2};
  unsigned turn_bits = 0u;
#pragma unroll
  for (int m = 0; m < 7; ++m) turn_bits |= ((turns & M[m]) != 0ull ? 1u : 0u) << m;
  store_turns(o, turn_bits, store);
}

// the half form: the octo's primitives on (a,b,c,d) with h2 = h1
template <class T, bool LINW>
__device__ __forceinline__ void half_form(const T (&v)[22], const T H0, const T dmax, T* __restrict__ o, bool store) {
  const T lim = sizeof(T) == 4 ? T(60) : T(600.0);
  const T xl1 = wave64_quad_pair(v[12], v[13]);
  const T h1 = wave64_oct_rows(wave64_oct_rows_de(wave64_quad_pair(v[8], v[9]), wave64_quad_pair(v[10], v[11]), wave64_quad_pair(v[0], v[1]),
                                                  wave64_quad_pair(v[2], v[3])), xl1, xl1);
  T w_t;
  const unsigned long long turns = wave64_oct_reduce_t(h1, h1, w_t);
  OctLeafStats<T> os;
  oct_leaf_stats<T, LINW>(w_t, H0, dmax, lim, os);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const T e = readlane_at(w_t, OctLeafStats<T>::lane_of(k)), w = os.w(k), sa = os.sa(k), dH = os.dH(k);
    store_leaf(o, k, e, w, sa, dH, os.redo(k), os.div(k), store);
  }
  if (store) {
    o[48] = (turns & OCT_TURN_AB) != 0ull ? T(1) : T(0);
    o[49] = (turns & OCT_TURN_CD) != 0ull ? T(1) : T(0);
    o[50] = (turns & OCT_TURN_ABCD) != 0ull ? T(1) : T(0);
  }
}

template <class T>
__device__ __forceinline__ void oct_body(const T* __restrict__ in, const T* __restrict__ par, T* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool ok = i < n;
  T v[22];
#pragma unroll
  for (int k = 0; k < 22; ++k) v[k] = ok ? in[i * 22 + k] : T(0);
  const long long wv = i >> 6;
  const T H0 = ok ? par[wv * 2 + 0] : T(0), dmax = ok ? par[wv * 2 + 1] : T(1);
  const bool store = ok && (threadIdx.x & 63u) == 0;
  T* o = out + wv * (6 * OCT_BLOCK);
  quad_form<T, true>(v, H0, dmax, o, store);
  oct_form<T, true>(v, H0, dmax, o + OCT_BLOCK, store);
  half_form<T, true>(v, H0, dmax, o + 2 * OCT_BLOCK, store);
  quad_form<T, false>(v, H0, dmax, o + 3 * OCT_BLOCK, store);
  oct_form<T, false>(v, H0, dmax, o + 4 * OCT_BLOCK, store);
  half_form<T, false>(v, H0, dmax, o + 5 * OCT_BLOCK, store);
}
#define PROBE_OCT(NAME, T) \
  extern "C" __global__ __launch_bounds__(256) void NAME(const T* __restrict__ in, const T* __restrict__ par, T* __restrict__ out, long long n) { oct_body<T>(in, par, out, n); }
PROBE_OCT(p_oct_red_f64, double)
PROBE_OCT(p_oct_red_f32, float)
