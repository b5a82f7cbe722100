// prims.hip — test-only wrappers around the device primitives of advancedhmc.jl_amd/csrc/ahmc_device.hpp
// (tests/test_device_primitives.py).  Each extern "C" kernel loads its inputs, calls ONE primitive at ONE template
// instantiation and stores every lane's result; the host compares them with exact references.  Compiled with the engine's
// own flags (build.build_probe_object) and loaded through hipModuleLoad (hipmod.Module).
//
// Launch rules (the wrappers check every index, but a reduction is only meaningful under these):
//   * the kernels for G <= 64 run with blockDim a multiple of 64 (whole waves; a group never straddles a wave);
//   * the kernels for G = 128 / 256 / 512 run with blockDim == G: ONE chain per workgroup, as the engine's launch plan
//     does (ahmc_kernels.hpp: group_grid).  Any other shape breaks the pairing of the exchange barriers;
//   * every wrapper is declared __launch_bounds__(512), so the G = 512 instantiations may be launched at blockDim 512;
//   * the wave-uniform wrappers (p_*_uniform: leaf_weight_exp<true>, whose table index is a readfirstlane) evaluate ONE
//     argument per step for the whole wave and keep the result in the lane it belongs to — never a per-lane argument;
//   * every launch uses several workgroups, so that a hazard that shows only on "some waves" has waves to show on;
//   * no lane returns before a cross-lane operation: out-of-range lanes compute on zeros and store nothing.
// No atomics (every lane stores its own outputs), no inline assembly beyond the header's, plain C++ stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ahmc_device.hpp"

using namespace ahmc;

#define PROBE __global__ __launch_bounds__(512)
#define GID ((long long)blockIdx.x * blockDim.x + threadIdx.x)

// ---------------------------------------------------------------------------------------------------------------------
// A/B/C. scalar maths: one argument per lane (y[i] = f(x[i])), or one argument per wave step (wave-uniform forms)
// ---------------------------------------------------------------------------------------------------------------------
#define PROBE_LANE1(NAME, T, EXPR)                                                                         \
  extern "C" PROBE void NAME(const T* __restrict__ x, T* __restrict__ y, long long n) {                    \
    const long long i = GID;                                                                               \
    if (i < n) {                                                                                           \
      const T a = x[i];                                                                                    \
      y[i] = (EXPR);                                                                                       \
    }                                                                                                      \
  }
#define PROBE_WAVE_UNIFORM(NAME, T, EXPR)                                                                  \
  extern "C" PROBE void NAME(const T* __restrict__ x, T* __restrict__ y, long long n) {                    \
    const long long w0 = GID & ~63LL;                                                                      \
    const int lane = (int)(threadIdx.x & 63u);                                                             \
    T mine = T(0);                                                                                         \
    for (int j = 0; j < 64; ++j) {                                                                         \
      const long long i = w0 + j;                                                                          \
      const T a = i < n ? x[i] : T(0); /* the same address in every lane: wave-uniform */                  \
      const T r = (EXPR);                                                                                  \
      mine = lane == j ? r : mine;                                                                         \
    }                                                                                                      \
    if (w0 + lane < n) y[w0 + lane] = mine;                                                                \
  }

PROBE_WAVE_UNIFORM(p_exp_table_uniform, double, leaf_weight_exp<true>(a))
PROBE_LANE1(p_exp_weight_lane, double, leaf_weight_exp<false>(a))
PROBE_LANE1(p_exp_horner, double, leaf_exp(a))
PROBE_LANE1(p_exp_lib_f64, double, exp(a))
PROBE_LANE1(p_exp_weight_f32, float, leaf_weight_exp<false>(a))
PROBE_LANE1(p_exp_lib_f32, float, exp(a))
PROBE_WAVE_UNIFORM(p_alpha_f64_uniform, double, (alpha_from_logweight<double, true>(a)))
PROBE_LANE1(p_alpha_f64_lane, double, (alpha_from_logweight<double, false>(a)))
PROBE_LANE1(p_alpha_f32_lane, float, (alpha_from_logweight<float, false>(a)))
PROBE_WAVE_UNIFORM(p_alpha_f32_uniform, float, (alpha_from_logweight<float, true>(a)))
PROBE_LANE1(p_log_f64, double, log(a))

#define PROBE_LOGADDEXP(NAME, T)                                                                                      \
  extern "C" PROBE void NAME(const T* __restrict__ x, const T* __restrict__ y, T* __restrict__ o, long long n) {        \
    const long long i = GID;                                                                                          \
    if (i < n) o[i] = logaddexp(x[i], y[i]);                                                                          \
  }
PROBE_LOGADDEXP(p_logaddexp_f64, double)
PROBE_LOGADDEXP(p_logaddexp_f32, float)

// ---------------------------------------------------------------------------------------------------------------------
// D. reductions.  in / out: K values per lane, lane-major (x[i*K + k]).
// ---------------------------------------------------------------------------------------------------------------------
template <int G, class T, int K>
__device__ __forceinline__ void red_body(const T* __restrict__ in, T* __restrict__ out, long long n) {
  const long long i = GID;
  T v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = i < n ? in[i * K + k] : T(0);
  group_allsum<G>(v);
  if (i < n) {
#pragma unroll
    for (int k = 0; k < K; ++k) out[i * K + k] = v[k];
  }
}
#define PROBE_RED(G, T, TN, K) \
  extern "C" PROBE void p_red_##TN##_g##G##_k##K(const T* __restrict__ in, T* __restrict__ out, long long n) { red_body<G, T, K>(in, out, n); }
#define PROBE_RED_K(G, T, TN) PROBE_RED(G, T, TN, 1) PROBE_RED(G, T, TN, 2) PROBE_RED(G, T, TN, 3) PROBE_RED(G, T, TN, 4) PROBE_RED(G, T, TN, 8)
#define FOR_ALL_G(X, ...) \
  X(1, __VA_ARGS__) X(2, __VA_ARGS__) X(4, __VA_ARGS__) X(8, __VA_ARGS__) X(16, __VA_ARGS__) X(32, __VA_ARGS__) X(64, __VA_ARGS__) \
  X(128, __VA_ARGS__) X(256, __VA_ARGS__) X(512, __VA_ARGS__)
FOR_ALL_G(PROBE_RED_K, float, f32)
FOR_ALL_G(PROBE_RED_K, double, f64)

// wave_allsum4(a, b, c, d) next to wave_allsum2(a, b); wave_allsum2(c, d) on the same inputs.  out: 8 per lane.
template <int G, class T>
__device__ __forceinline__ void quad_body(const T* __restrict__ in, T* __restrict__ out, long long n) {
  const long long i = GID;
  T a = i < n ? in[i * 4 + 0] : T(0), b = i < n ? in[i * 4 + 1] : T(0);
  T c = i < n ? in[i * 4 + 2] : T(0), d = i < n ? in[i * 4 + 3] : T(0);
  T a2 = a, b2 = b, c2 = c, d2 = d;
  wave_allsum4<G>(a, b, c, d);
  wave_allsum2<G>(a2, b2);
  wave_allsum2<G>(c2, d2);
  if (i < n) {
    T* o = out + i * 8;
    o[0] = a; o[1] = b; o[2] = c; o[3] = d;
    o[4] = a2; o[5] = b2; o[6] = c2; o[7] = d2;
  }
}
#define PROBE_QUAD(G, T, TN) \
  extern "C" PROBE void p_quad_##TN##_g##G(const T* __restrict__ in, T* __restrict__ out, long long n) { quad_body<G, T>(in, out, n); }
PROBE_QUAD(16, float, f32) PROBE_QUAD(32, float, f32) PROBE_QUAD(64, float, f32)
PROBE_QUAD(16, double, f64) PROBE_QUAD(32, double, f64) PROBE_QUAD(64, double, f64)

// multi-wave groups: group_allsum, group_allsum_once and leapfrog_allsum<G, TK = 3> on the same inputs.  out: 3K per lane.
template <int G, class T, int K>
__device__ __forceinline__ void once_body(const T* __restrict__ in, T* __restrict__ out, long long n) {
  __shared__ __attribute__((aligned(16))) double buf[8 * K];
  const long long i = GID;
  T v[K], w[K], x[K];
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = w[k] = x[k] = i < n ? in[i * K + k] : T(0);
  group_allsum<G>(v);
  group_allsum_once<G>(w, buf);
  leapfrog_allsum<G, 3>(x);
  if (i < n) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      out[i * 3 * K + k] = v[k];
      out[i * 3 * K + K + k] = w[k];
      out[i * 3 * K + 2 * K + k] = x[k];
    }
  }
}
#define PROBE_ONCE(G, T, TN, K) \
  extern "C" PROBE void p_once_##TN##_g##G##_k##K(const T* __restrict__ in, T* __restrict__ out, long long n) { once_body<G, T, K>(in, out, n); }
#define PROBE_ONCE_K(G, T, TN) PROBE_ONCE(G, T, TN, 1) PROBE_ONCE(G, T, TN, 2) PROBE_ONCE(G, T, TN, 3) PROBE_ONCE(G, T, TN, 4)
PROBE_ONCE_K(128, float, f32) PROBE_ONCE_K(256, float, f32) PROBE_ONCE_K(512, float, f32)
PROBE_ONCE_K(128, double, f64) PROBE_ONCE_K(256, double, f64) PROBE_ONCE_K(512, double, f64)

// ---------------------------------------------------------------------------------------------------------------------
// E. broadcasts: for every src = 0..G-1, out[src * n + i] = group_bcast<G>(in[i], src)
// ---------------------------------------------------------------------------------------------------------------------
template <int G, class T>
__device__ __forceinline__ void bcast_body(const T* __restrict__ in, T* __restrict__ out, long long n) {
  const long long i = GID;
  const T v = i < n ? in[i] : T(0);
  for (int s = 0; s < G; ++s) {
    const T r = group_bcast<G>(v, s);
    if (i < n) out[(long long)s * n + i] = r;
  }
}
template <int G>
__device__ __forceinline__ void bcast_i32_body(const int* __restrict__ in, int* __restrict__ out, long long n) {
  const long long i = GID;
  const int v = i < n ? in[i] : 0;
  for (int s = 0; s < G; ++s) {
    const int r = group_bcast_i32<G>(v, s);
    if (i < n) out[(long long)s * n + i] = r;
  }
}
#define PROBE_BCAST(G, T, TN) \
  extern "C" PROBE void p_bcast_##TN##_g##G(const T* __restrict__ in, T* __restrict__ out, long long n) { bcast_body<G, T>(in, out, n); }
#define PROBE_BCAST_I32(G) \
  extern "C" PROBE void p_bcast_i32_g##G(const int* __restrict__ in, int* __restrict__ out, long long n) { bcast_i32_body<G>(in, out, n); }
FOR_ALL_G(PROBE_BCAST, float, f32)
FOR_ALL_G(PROBE_BCAST, double, f64)
PROBE_BCAST_I32(1) PROBE_BCAST_I32(2) PROBE_BCAST_I32(4) PROBE_BCAST_I32(8) PROBE_BCAST_I32(16) PROBE_BCAST_I32(32) PROBE_BCAST_I32(64)

// ---------------------------------------------------------------------------------------------------------------------
// F. RNG
// ---------------------------------------------------------------------------------------------------------------------
// ck: (c0, c1, c2, c3, k0, k1) per item; out: 4 words per item
extern "C" PROBE void p_philox(const uint32_t* __restrict__ ck, uint32_t* __restrict__ out, long long n) {
  const long long i = GID;
  if (i >= n) return;
  const uint32_t* a = ck + i * 6;
  const Philox4 p = philox4x32_10(a[0], a[1], a[2], a[3], a[4], a[5]);
#pragma unroll
  for (int k = 0; k < 4; ++k) out[i * 4 + k] = p.v[k];
}
// hl: (hi, lo) per item
extern "C" PROBE void p_u53(const uint32_t* __restrict__ hl, double* __restrict__ out, long long n) {
  const long long i = GID;
  if (i < n) out[i] = u53(hl[i * 2], hl[i * 2 + 1]);
}
// prm: (k0, k1, chain, iter, purpose, slot) per item; out: uniform, randexp, z0, z1 (f64) and boolean (i32)
extern "C" PROBE void p_rng(const uint32_t* __restrict__ prm, double* __restrict__ out, int* __restrict__ bits, long long n) {
  const long long i = GID;
  if (i >= n) return;
  const uint32_t* a = prm + i * 6;
  const Rng rng{a[0], a[1], a[2], a[3]};
  double z0, z1;
  rng.normal_pair(a[4], a[5], z0, z1);
  out[i * 4 + 0] = rng.uniform(a[4], a[5]);
  out[i * 4 + 1] = rng.randexp(a[4], a[5]);
  out[i * 4 + 2] = z0;
  out[i * 4 + 3] = z1;
  bits[i] = rng.boolean(a[4], a[5]) ? 1 : 0;
}
// prm: (k0, k1, chain, iter, purpose, d0) per item; out: E normals per item
template <class T, int E>
__device__ __forceinline__ void normals_body(const uint32_t* __restrict__ prm, T* __restrict__ out, long long n) {
  const long long i = GID;
  if (i >= n) return;
  const uint32_t* a = prm + i * 6;
  const Rng rng{a[0], a[1], a[2], a[3]};
  T z[E];
  normals<T, E>(rng, a[4], (int)a[5], z);
#pragma unroll
  for (int e = 0; e < E; ++e) out[i * E + e] = z[e];
}
#define PROBE_NORMALS(T, TN, E) \
  extern "C" PROBE void p_normals_##TN##_e##E(const uint32_t* __restrict__ prm, T* __restrict__ out, long long n) { normals_body<T, E>(prm, out, n); }
PROBE_NORMALS(float, f32, 1) PROBE_NORMALS(float, f32, 2) PROBE_NORMALS(float, f32, 8)
PROBE_NORMALS(double, f64, 1) PROBE_NORMALS(double, f64, 2) PROBE_NORMALS(double, f64, 8)

// ---------------------------------------------------------------------------------------------------------------------
// G. targets and leapfrog pieces.  Chain c = gid / G owns lanes gid % G; θ, r, M⁻¹ are (nchains, D) row-major, loaded with
// load_vec (pad 0 / 0 / 1) as the kernels do; params are shared by all chains.  Per lane, REC values at out + gid * REC:
//   [0, E)      g0   = −∇ℓπ(θ)            fill_caches
//   [E, 2E)     θ1, [2E, 3E) r1, [3E, 4E) g1 after one leapfrog_step (untempered, as in the NUTS kernels)
//   4E + 0..1   ℓπ, ℓκ of fill_caches;   4E + 2..3  ℓπ, ℓκ after the step;   4E + 4..5  ℓπ, ℓκ of leapfrog_step_plus2
//   4E + 6..7   the two extra sums of leapfrog_step_plus2 (Σθ·r, Σr·r of the updated point)
//   4E + 8..9   what hier_publish_next left in xwave_buf_p after the step (chain's first lane; 0 where nothing is published)
//   4E + 10..11 θ[0], θ[1] after a SECOND leapfrog_step (its target_eval with `use_pre`) — the lane that owns them
// ---------------------------------------------------------------------------------------------------------------------
template <class T, int G, int E, int TK>
__device__ __forceinline__ void target_body(const T* __restrict__ theta, const T* __restrict__ mom, const T* __restrict__ minv_in,
                                            const T* __restrict__ params, int D, long long nchains, T eps, int use_pre, T* __restrict__ out) {
  constexpr int REC = 4 * E + 12;
  const long long gid = GID;
  const long long c = gid / G;
  const bool live = c < nchains;
  const long long cc = live ? c : 0;
  const int lane = (int)(gid % G), d0 = lane * E;
  const TargetP<T> tp{TK, D, params};
  const LeapfrogP<T> lf{0, T(1)};
  Point<T, E> z;
  T minv[E];
  load_vec(z.th, theta, cc * D, d0, D, T(0));
  load_vec(z.r, mom, cc * D, d0, D, T(0));
  load_vec(minv, minv_in, cc * D, d0, D, T(1));
  fill_caches<T, G, E, TK>(z, minv, tp, lane, d0);
  T* o = out + gid * REC;
  if (live) {
#pragma unroll
    for (int e = 0; e < E; ++e) o[e] = z.g[e];
    o[4 * E + 0] = z.lp;
    o[4 * E + 1] = z.lk;
  }
  const Point<T, E> z0 = z;
  leapfrog_step<T, G, E, TK, false>(z, minv, eps, tp, lf, lane, d0, 1, 1, false);
  T pub0 = 0, pub1 = 0;
  if constexpr (G > 64 && TK == 3) {
    if (threadIdx.x == 0) {  // published before the step's energy barrier: visible to every lane now
      pub0 = (T)xwave_buf_p()[0];
      pub1 = (T)xwave_buf_p()[1];
    }
  }
  if (live) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      o[E + e] = z.th[e];
      o[2 * E + e] = z.r[e];
      o[3 * E + e] = z.g[e];
    }
    o[4 * E + 2] = z.lp;
    o[4 * E + 3] = z.lk;
    o[4 * E + 8] = pub0;
    o[4 * E + 9] = pub1;
  }
  leapfrog_step<T, G, E, TK, false>(z, minv, eps, tp, lf, lane, d0, 2, 2, use_pre != 0);
  if (live) {
    o[4 * E + 10] = d0 == 0 ? z.th[0] : T(0);
    o[4 * E + 11] = d0 == 0 ? z.th[E >= 2 ? 1 : 0] : (d0 == 1 ? z.th[0] : T(0));
  }
  Point<T, E> z3 = z0;
  T extra[2];
  leapfrog_step_plus2<T, G, E, TK>(z3, minv, eps, tp, lane, d0, extra, [&](T& a, T& b) {
    a = 0;
    b = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      a += z3.th[e] * z3.r[e];
      b += z3.r[e] * z3.r[e];
    }
  });
  if (live) {
    o[4 * E + 4] = z3.lp;
    o[4 * E + 5] = z3.lk;
    o[4 * E + 6] = extra[0];
    o[4 * E + 7] = extra[1];
  }
}
#define PROBE_TARGET(T, TN, G, E, TK)                                                                                           \
  extern "C" PROBE void p_target_##TN##_g##G##_e##E##_t##TK(const T* __restrict__ theta, const T* __restrict__ mom,             \
                                                            const T* __restrict__ minv, const T* __restrict__ params, int D,    \
                                                            long long nchains, T eps, int use_pre, T* __restrict__ out) {       \
    target_body<T, G, E, TK>(theta, mom, minv, params, D, nchains, eps, use_pre, out);                                          \
  }
#define PROBE_TARGET_TK(T, TN, G, E) PROBE_TARGET(T, TN, G, E, 0) PROBE_TARGET(T, TN, G, E, 1) PROBE_TARGET(T, TN, G, E, 2) PROBE_TARGET(T, TN, G, E, 3)
#define PROBE_TARGET_GEOM(T, TN)                                                                                                 \
  PROBE_TARGET_TK(T, TN, 4, 1) PROBE_TARGET_TK(T, TN, 8, 2) PROBE_TARGET_TK(T, TN, 16, 2) PROBE_TARGET_TK(T, TN, 32, 4)          \
  PROBE_TARGET_TK(T, TN, 64, 8) PROBE_TARGET_TK(T, TN, 128, 4) PROBE_TARGET_TK(T, TN, 512, 8)
PROBE_TARGET_GEOM(float, f32)
PROBE_TARGET_GEOM(double, f64)

// ---------------------------------------------------------------------------------------------------------------------
// G2. Two consecutive leapfrog_steps of a multi-wave hierarchical chain (TK = 3, one chain per workgroup of G threads), the second
// with or without `use_pre`: with it, the other waves read μ and log τ that hier_publish_next computed during the FIRST step; without
// it, the ones lane 0 computed in the second.  Both are the half kick and the drift of elements 0 and 1 — one definition
// (leapfrog_kick / leapfrog_drift), so every lane's result must not depend on the switch.  Record per thread, REC = 3E + 4:
//   [0,E) θ   [E,2E) r   [2E,3E) −∇ℓπ   3E ℓπ   3E+1 ℓκ   (all after the second step)
//   3E+2..3  what hier_publish_next left in xwave_buf_p during the first step (the chain's first lane; 0 elsewhere)
// ---------------------------------------------------------------------------------------------------------------------
template <class T, int G, int E>
__device__ __forceinline__ void hier2_body(const T* __restrict__ theta, const T* __restrict__ mom, const T* __restrict__ minv_in, int D,
                                           long long nchains, T eps, int use_pre, T* __restrict__ out) {
  constexpr int TK = 3, REC = 3 * E + 4;
  const long long gid = GID;
  const long long c = gid / G;
  const bool live = c < nchains;
  const long long cc = live ? c : 0;
  const int lane = (int)(gid % G), d0 = lane * E;
  const TargetP<T> tp{TK, D, nullptr};
  const LeapfrogP<T> lf{0, T(1)};
  Point<T, E> z;
  T minv[E];
  load_vec(z.th, theta, cc * D, d0, D, T(0));
  load_vec(z.r, mom, cc * D, d0, D, T(0));
  load_vec(minv, minv_in, cc * D, d0, D, T(1));
  fill_caches<T, G, E, TK>(z, minv, tp, lane, d0);
  leapfrog_step<T, G, E, TK, false>(z, minv, eps, tp, lf, lane, d0, 1, 2, false);
  T pub0 = 0, pub1 = 0;
  if (threadIdx.x == 0) {  // published before the first step's energy barrier
    pub0 = (T)xwave_buf_p()[0];
    pub1 = (T)xwave_buf_p()[1];
  }
  leapfrog_step<T, G, E, TK, false>(z, minv, eps, tp, lf, lane, d0, 2, 2, use_pre != 0);
  if (live) {
    T* o = out + gid * REC;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      o[e] = z.th[e];
      o[E + e] = z.r[e];
      o[2 * E + e] = z.g[e];
    }
    o[3 * E + 0] = z.lp;
    o[3 * E + 1] = z.lk;
    o[3 * E + 2] = pub0;
    o[3 * E + 3] = pub1;
  }
}
#define PROBE_HIER2(T, TN, G, E)                                                                                             \
  extern "C" PROBE void p_hier2_##TN##_g##G##_e##E(const T* __restrict__ theta, const T* __restrict__ mom,                   \
                                                   const T* __restrict__ minv, int D, long long nchains, T eps, int use_pre, \
                                                   T* __restrict__ out) {                                                    \
    hier2_body<T, G, E>(theta, mom, minv, D, nchains, eps, use_pre, out);                                                    \
  }
PROBE_HIER2(float, f32, 128, 4) PROBE_HIER2(float, f32, 256, 8) PROBE_HIER2(float, f32, 512, 8)
PROBE_HIER2(double, f64, 128, 4) PROBE_HIER2(double, f64, 256, 8) PROBE_HIER2(double, f64, 512, 8)

// ---------------------------------------------------------------------------------------------------------------------
// H. load_vec / store_vec.  Chain c = gid / L (L lanes per chain, lane l owns d0 = l·E) lives at base[off0 + c·stride ..];
// `loaded` receives every lane's E registers (padding included), then store_vec writes them back into dst.
// ---------------------------------------------------------------------------------------------------------------------
template <class T, int E>
__device__ __forceinline__ void vec_body(const T* __restrict__ src, T* __restrict__ dst, T* __restrict__ loaded, long long off0, long long stride,
                                         int D, int L, T pad, long long nthreads) {
  const long long gid = GID;
  if (gid >= nthreads) return;
  const long long c = gid / L;
  const int d0 = (int)(gid % L) * E;
  T v[E];
  load_vec(v, src, off0 + c * stride, d0, D, pad);
#pragma unroll
  for (int e = 0; e < E; ++e) loaded[gid * E + e] = v[e];
  store_vec(v, dst, off0 + c * stride, d0, D);
}
#define PROBE_VEC(T, TN, E)                                                                                                \
  extern "C" PROBE void p_vec_##TN##_e##E(const T* __restrict__ src, T* __restrict__ dst, T* __restrict__ loaded, long long off0, \
                                          long long stride, int D, int L, T pad, long long nthreads) {                      \
    vec_body<T, E>(src, dst, loaded, off0, stride, D, L, pad, nthreads);                                                    \
  }
PROBE_VEC(float, f32, 1) PROBE_VEC(float, f32, 2) PROBE_VEC(float, f32, 4) PROBE_VEC(float, f32, 8)
PROBE_VEC(double, f64, 1) PROBE_VEC(double, f64, 2) PROBE_VEC(double, f64, 4) PROBE_VEC(double, f64, 8)
