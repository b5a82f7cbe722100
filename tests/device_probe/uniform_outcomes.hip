// uniform_outcomes.hip — test-only wrappers around the wave-uniform tree decisions of a chain that owns its wave
// (tests/test_uniform_outcomes.py): the U-turn predicate wave64_any_le0_pair (ahmc_device.hpp) next to wave_allsum2<64> + the two
// compares it replaces, and the wave-wide draw stream DrawStreamT<true> (ahmc_nuts.hpp) next to the narrow DrawStreamT<false> on the
// same Rng.  Compiled with the engine's own flags (build.build_probe_object), loaded through hipModuleLoad (hipmod.Module).
//
// Launch rules: blockDim a multiple of 64 (whole waves); out-of-range waves compute on zeros and store nothing; no lane returns
// before a cross-lane operation.  No atomics, no inline assembly beyond the headers', plain C++ stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ahmc_nuts.hpp"

using namespace ahmc;

#define PROBE __global__ __launch_bounds__(256)
#define GID ((long long)blockIdx.x * blockDim.x + threadIdx.x)

// in: (a, b) per lane.  out: 2 ints per lane — [0] the new predicate, [1] the reference, both as every lane sees them —
// sums: 2 values per lane, what wave_allsum2<64> returned (for the host's own look at the built cases).
template <class T>
__device__ __forceinline__ void pred_body(const T* __restrict__ in, int* __restrict__ out, T* __restrict__ sums, long long n) {
  const long long i = GID;
  const T a = i < n ? in[i * 2 + 0] : T(0), b = i < n ? in[i * 2 + 1] : T(0);
  const bool fast = wave64_any_le0_pair(a, b);
  T a2 = a, b2 = b;
  wave_allsum2<64>(a2, b2);
  const bool ref = (a2 <= T(0)) || (b2 <= T(0));
  if (i < n) {
    out[i * 2 + 0] = fast ? 1 : 0;
    out[i * 2 + 1] = ref ? 1 : 0;
    sums[i * 2 + 0] = a2;
    sums[i * 2 + 1] = b2;
  }
}
extern "C" PROBE void p_any_le0_f32(const float* __restrict__ in, int* __restrict__ out, float* __restrict__ sums, long long n) {
  pred_body<float>(in, out, sums, n);
}
extern "C" PROBE void p_any_le0_f64(const double* __restrict__ in, int* __restrict__ out, double* __restrict__ sums, long long n) {
  pred_body<double>(in, out, sums, n);
}

// prm: (k0, k1, chain, iter) shared by the launch.  Wave w of the launch resumes both streams at draw k0s[w] — through init() if
// `use_init` (then k0s must be 0), through resume(rng, k0s[w]) otherwise, k0 == 0 included — and takes `ndraw` words from each;
// out_wide / out_narrow: [wave][draw][lane] — every lane's copy of every word.
extern "C" PROBE void p_draw_streams(const uint32_t* __restrict__ prm, const uint32_t* __restrict__ k0s, int nwaves, int ndraw, int use_init,
                                     uint32_t* __restrict__ out_wide, uint32_t* __restrict__ out_narrow) {
  const long long w = GID >> 6;
  const int lane = (int)(threadIdx.x & 63u);
  const bool live = w < nwaves;
  const Rng rng{prm[0], prm[1], prm[2], prm[3]};
  const uint32_t k0 = live ? k0s[w] : 0u;  // one address per wave: wave-uniform
  DrawStreamT<true> wide;
  DrawStreamT<false> narrow;
  if (use_init != 0) {
    wide.init(rng);
    narrow.init(rng);
  } else {
    wide.resume(rng, k0);
    narrow.resume(rng, k0);
  }
  for (int j = 0; j < ndraw; ++j) {
    const uint32_t a = wide.word();
    const uint32_t b = narrow.word();
    if (live) {
      const long long o = (w * ndraw + j) * 64 + lane;
      out_wide[o] = a;
      out_narrow[o] = b;
    }
  }
}
