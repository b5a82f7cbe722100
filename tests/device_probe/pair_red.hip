// pair_red.hip — wave64_pair_reduce (ahmc_device.hpp; the one reduction of a pair step of k_nuts) next to the primitives it replaces,
// on the same data (tests/test_leaf_pairs.py).  Compiled with the engine's own flags (build.build_probe_object) and loaded through
// hipModuleLoad (hipmod.Module).
//
// in : 4 values per lane, lane-major: ea, eb (lane partials of two leaves' energies), da, db (lane partials of the two U-turn dot products)
// out: 6 values per lane: [0] Σea and [1] Σeb from wave_allsum<64, T, 1>, [2] the decision of wave64_any_le0_pair(da, db) as 0 / 1,
//      [3] Σea, [4] Σeb and [5] the decision from wave64_pair_reduce
// p_pair_red_<T>: the quad the engine takes the energies from (AHMC_PAIR_RED_QUAD); p_pair_red_<T>_q<k>: quad k.  Which quads give the
// butterfly's bits depends on the direction row_ror rotates in, and the device decides that, not the manual.
// Launch with blockDim a multiple of 64 (whole waves).  No lane returns before a cross-lane operation: out-of-range lanes compute on
// zeros and store nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ahmc_device.hpp"

using namespace ahmc;

template <class T, int Q>
__device__ __forceinline__ void pair_body(const T* __restrict__ in, T* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const T ea = i < n ? in[i * 4 + 0] : T(0), eb = i < n ? in[i * 4 + 1] : T(0);
  const T da = i < n ? in[i * 4 + 2] : T(0), db = i < n ? in[i * 4 + 3] : T(0);
  T sa[1] = {ea}, sb[1] = {eb};
  wave_allsum<64>(sa);
  wave_allsum<64>(sb);
  const bool t_ref = wave64_any_le0_pair(da, db);
  T pa = ea, pb = eb;
  const bool t_new = wave64_pair_reduce<T, Q>(da, db, pa, pb);
  if (i < n) {
    out[i * 6 + 0] = sa[0];
    out[i * 6 + 1] = sb[0];
    out[i * 6 + 2] = t_ref ? T(1) : T(0);
    out[i * 6 + 3] = pa;
    out[i * 6 + 4] = pb;
    out[i * 6 + 5] = t_new ? T(1) : T(0);
  }
}
#define PROBE_PAIR(NAME, T, Q) \
  extern "C" __global__ __launch_bounds__(256) void NAME(const T* __restrict__ in, T* __restrict__ out, long long n) { pair_body<T, Q>(in, out, n); }
PROBE_PAIR(p_pair_red_f64, double, AHMC_PAIR_RED_QUAD)
PROBE_PAIR(p_pair_red_f32, float, AHMC_PAIR_RED_QUAD)
PROBE_PAIR(p_pair_red_f64_q0, double, 0) PROBE_PAIR(p_pair_red_f64_q1, double, 1) PROBE_PAIR(p_pair_red_f64_q2, double, 2) PROBE_PAIR(p_pair_red_f64_q3, double, 3)
PROBE_PAIR(p_pair_red_f32_q0, float, 0) PROBE_PAIR(p_pair_red_f32_q1, float, 1) PROBE_PAIR(p_pair_red_f32_q2, float, 2) PROBE_PAIR(p_pair_red_f32_q3, float, 3)
