// ahmc_device.hpp — device-side building blocks of the chain-batched HMC/NUTS engine (gfx950).
//
// Thread mapping: a chain is owned by a *group* of G consecutive lanes of one
// wave64 (G ∈ {4,8,16,32,64}); lane l of the group holds the E contiguous elements
// d = l*E .. l*E+E-1 of every (D,) vector of its chain in registers.  G*E >= D; padded elements
// are kept at exactly 0 (momentum/gradient) so they never contribute to a reduction.
// All per-chain scalars (energies, weights, RNG draws, control flow) are computed redundantly
// and bit-identically by every lane of the group, so control flow is uniform inside a group.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ahmc {

// ------------------------------------------------------------------------------------------------
// Philox4x32-10 counter-based RNG.  Stream layout is the specification shared with the oracle:
//   counter = (chain, iteration, purpose, slot), key = (seed_lo, seed_hi)
// ------------------------------------------------------------------------------------------------
enum : uint32_t { RNG_MOMENTUM = 0, RNG_TRANSITION = 1, RNG_JITTER = 2, RNG_FINDEPS = 3 };
constexpr uint32_t COUPLED_CHAIN = 0xFFFFFFFFu;

struct Philox4 {
  uint32_t v[4];
};

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                 uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += W0; k1 += W1;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// 53-bit uniform in (0, 1]: (bits + ½)·2^-53 is exact below 2^52; above, the + ½ is a tie rounded to even, so the top input
// bits = 2^53 − 1 gives exactly 1.0 (every other input lies in (0, 1); the oracle computes the same values)
__device__ __forceinline__ double u53(uint32_t hi, uint32_t lo) {
  uint64_t bits = ((uint64_t)(hi >> 5) << 26) | (uint64_t)(lo >> 6);
  return ((double)bits + 0.5) * (1.0 / 9007199254740992.0);
}

struct Rng {
  uint32_t k0, k1, chain, iter;
  __device__ __forceinline__ Philox4 raw(uint32_t purpose, uint32_t slot) const {
    return philox4x32_10(chain, iter, purpose, slot, k0, k1);
  }
  __device__ __forceinline__ double uniform(uint32_t purpose, uint32_t slot) const {
    Philox4 p = raw(purpose, slot);
    return u53(p.v[0], p.v[1]);
  }
  __device__ __forceinline__ bool boolean(uint32_t purpose, uint32_t slot) const {
    return (raw(purpose, slot).v[0] >> 31) != 0;
  }
  __device__ __forceinline__ double randexp(uint32_t purpose, uint32_t slot) const {
    return -log(uniform(purpose, slot));
  }
  // Box–Muller pair `pair` → (z0, z1) = standard normals of elements 2*pair, 2*pair+1
  __device__ __forceinline__ void normal_pair(uint32_t purpose, uint32_t pair, double& z0, double& z1) const {
    Philox4 p = raw(purpose, pair);
    double u1 = u53(p.v[0], p.v[1]), u2 = u53(p.v[2], p.v[3]);
    double rad = sqrt(-2.0 * log(u1));
    double s, c;
    sincos(6.283185307179586476925286766559 * u2, &s, &c);
    z0 = rad * c;
    z1 = rad * s;
  }
};

// E standard normals for the elements d0 .. d0+E-1 owned by this lane
template <class T, int E>
__device__ __forceinline__ void normals(const Rng& rng, uint32_t purpose, int d0, T (&z)[E]) {
  if constexpr (E == 1) {
    double a, b;
    rng.normal_pair(purpose, (uint32_t)d0 >> 1, a, b);
    z[0] = (T)((d0 & 1) ? b : a);
  } else {
    static_assert(E % 2 == 0, "E must be 1 or even");
#pragma unroll
    for (int e = 0; e < E; e += 2) {
      double a, b;
      rng.normal_pair(purpose, (uint32_t)(d0 + e) >> 1, a, b);
      z[e] = (T)a;
      z[e + 1] = (T)b;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// numerics helpers that must follow Julia semantics (NaN-propagating min/max; LogExpFunctions)
// ------------------------------------------------------------------------------------------------
template <class T> struct Lim;
template <> struct Lim<float> {
  static __device__ __forceinline__ float inf() { return __int_as_float(0x7f800000); }
  static __device__ __forceinline__ float nan() { return __int_as_float(0x7fc00000); }
};
template <> struct Lim<double> {
  static __device__ __forceinline__ double inf() { return __longlong_as_double(0x7ff0000000000000LL); }
  static __device__ __forceinline__ double nan() { return __longlong_as_double(0x7ff8000000000000LL); }
};

template <class T> __device__ __forceinline__ T jl_min(T a, T b) { return (a != a || b != b) ? Lim<T>::nan() : (a < b ? a : b); }
template <class T> __device__ __forceinline__ T jl_max(T a, T b) { return (a != a || b != b) ? Lim<T>::nan() : (a > b ? a : b); }
template <class T> __device__ __forceinline__ bool is_finite(T v) { return isfinite(v); }
// PhasePoint constructor: non-finite ℓπ/ℓκ values become -Inf (src/hamiltonian.jl:95-104)
template <class T> __device__ __forceinline__ T sanitize(T v) { return is_finite(v) ? v : -Lim<T>::inf(); }
// LogExpFunctions.logaddexp (src/trajectory.jl:192,198)
template <class T> __device__ __forceinline__ T logaddexp(T x, T y) {
  T d = (x == y) ? T(0) : fabs(x - y);
  return jl_max(x, y) + log1p(exp(-d));
}
// exp for the leaf weight of the linear-domain NUTS kernels, one call per leapfrog.  Float64: the ROCm device library's
// own algorithm (2^n range reduction with a two-part ln 2, degree-11 minimax Horner, ldexp; same constants, same
// operation order, so the same bits as `exp`), with the Horner steps issued as three-address v_fma_f64.  The
// compiler's version of that loop re-materialises each coefficient in front of a two-address v_fmac_f64 — 9 extra
// VALU instructions per leaf of a kernel that is VALU-issue bound.
__device__ __forceinline__ double fma3(double a, double b, double c) {
  double d;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}
// (The engine no longer calls leaf_exp — the leaf weight is leaf_weight_exp below.  It stays as the reference the device probe
// tests/device_probe/prims.hip holds the Horner form to, tests/test_device_primitives.py.)
__device__ __forceinline__ double leaf_exp(double x) {
  constexpr auto C = [](unsigned long long bits) { return __builtin_bit_cast(double, bits); };
  const double dn = __builtin_rint(x * C(0x3ff71547652b82feULL));                 // x·log2(e)
  double t = __builtin_fma(dn, C(0xbfe62e42fefa39efULL), x);                      // − n·ln2 (high part)
  t = __builtin_fma(dn, C(0xbc7abc9e3b39803fULL), t);                             // − n·ln2 (low part)
  double q = __builtin_fma(t, C(0x3e5ade156a5dcb37ULL), C(0x3e928af3fca7ab0cULL));
  q = fma3(t, q, C(0x3ec71dee623fde64ULL));
  q = fma3(t, q, C(0x3efa01997c89e6b0ULL));
  q = fma3(t, q, C(0x3f2a01a014761f6eULL));
  q = fma3(t, q, C(0x3f56c16c1852b7b0ULL));
  q = fma3(t, q, C(0x3f81111111122322ULL));
  q = fma3(t, q, C(0x3fa55555555502a1ULL));
  q = fma3(t, q, C(0x3fc5555555555511ULL));
  q = fma3(t, q, C(0x3fe000000000000bULL));
  q = __builtin_fma(t, q, 1.0);
  q = __builtin_fma(t, q, 1.0);
  double z = __builtin_ldexp(q, (int)dn);
  z = x > 1024.0 ? Lim<double>::inf() : z;
  z = x < -1075.0 ? 0.0 : z;
  return z;
}
__device__ __forceinline__ float leaf_exp(float x) { return exp(x); }

// The weight of a NUTS leaf in the linear-domain kernels: W = exp(ℓw) for ℓw <= LINW_LIMIT (a larger ℓw flags the chain
// for the log-domain redo pass and its W is never used), so the overflow branch of exp is dead; ℓw = -Inf (a divergent
// leaf) must give exactly 0.  Two forms:
//  * a chain that owns the wave (UNIFORM): table-assisted — x = (64 n + j)·ln2/64 + t, |t| <= ln2/128: exp(x) = 2^n · T[j] · (1 + (e^t − 1))
//    with a 64-entry table of 2^(j/64) (a scalar load) and a degree-5 polynomial: ≈9 VALU less than the
//    Horner-11 form; ≤ 1.34 ulp against the exact value (½ ulp of the rounded table entry, ≤ 0.32 ulp from truncating
//    e^t − 1 after t^5 at |t| = ln2/128, ½ ulp for the final fma; tests/test_device_primitives.py, > 2^22 arguments with both
//    edges of every table bucket: 1.27 ulp measured), i.e. last-ulp differences against the device library's exp().
//    Measured on cfg2 (sampling phase, in-kernel leapfrog/s): Horner 2.654e9, table 2.718e9.
//  * chains that SHARE a wave (G < 64): leaf_exp's algorithm (the device library's, 11 Horner steps) without the overflow and
//    underflow selects (same bits where it matters) — see below why not the table.
// 2^(j/64), j = 0..63, correctly rounded (generated with 60-digit decimal arithmetic)
static __device__ const unsigned long long EXP2_64_BITS[64] = {
    0x3ff0000000000000ULL, 0x3ff02c9a3e778061ULL, 0x3ff059b0d3158574ULL, 0x3ff0874518759bc8ULL,
    0x3ff0b5586cf9890fULL, 0x3ff0e3ec32d3d1a2ULL, 0x3ff11301d0125b51ULL, 0x3ff1429aaea92de0ULL,
    0x3ff172b83c7d517bULL, 0x3ff1a35beb6fcb75ULL, 0x3ff1d4873168b9aaULL, 0x3ff2063b88628cd6ULL,
    0x3ff2387a6e756238ULL, 0x3ff26b4565e27cddULL, 0x3ff29e9df51fdee1ULL, 0x3ff2d285a6e4030bULL,
    0x3ff306fe0a31b715ULL, 0x3ff33c08b26416ffULL, 0x3ff371a7373aa9cbULL, 0x3ff3a7db34e59ff7ULL,
    0x3ff3dea64c123422ULL, 0x3ff4160a21f72e2aULL, 0x3ff44e086061892dULL, 0x3ff486a2b5c13cd0ULL,
    0x3ff4bfdad5362a27ULL, 0x3ff4f9b2769d2ca7ULL, 0x3ff5342b569d4f82ULL, 0x3ff56f4736b527daULL,
    0x3ff5ab07dd485429ULL, 0x3ff5e76f15ad2148ULL, 0x3ff6247eb03a5585ULL, 0x3ff6623882552225ULL,
    0x3ff6a09e667f3bcdULL, 0x3ff6dfb23c651a2fULL, 0x3ff71f75e8ec5f74ULL, 0x3ff75feb564267c9ULL,
    0x3ff7a11473eb0187ULL, 0x3ff7e2f336cf4e62ULL, 0x3ff82589994cce13ULL, 0x3ff868d99b4492edULL,
    0x3ff8ace5422aa0dbULL, 0x3ff8f1ae99157736ULL, 0x3ff93737b0cdc5e5ULL, 0x3ff97d829fde4e50ULL,
    0x3ff9c49182a3f090ULL, 0x3ffa0c667b5de565ULL, 0x3ffa5503b23e255dULL, 0x3ffa9e6b5579fdbfULL,
    0x3ffae89f995ad3adULL, 0x3ffb33a2b84f15fbULL, 0x3ffb7f76f2fb5e47ULL, 0x3ffbcc1e904bc1d2ULL,
    0x3ffc199bdd85529cULL, 0x3ffc67f12e57d14bULL, 0x3ffcb720dcef9069ULL, 0x3ffd072d4a07897cULL,
    0x3ffd5818dcfba487ULL, 0x3ffda9e603db3285ULL, 0x3ffdfc97337b9b5fULL, 0x3ffe502ee78b3ff6ULL,
    0x3ffea4afa2a490daULL, 0x3ffefa1bee615a27ULL, 0x3fff50765b6e4540ULL, 0x3fffa7c1819e90d8ULL};
// Chains that SHARE a wave (G < 64): the table entry would be a per-lane GLOBAL load in the middle of the leaf's chain of dependent stages — and
// its s_waitcnt vmcnt(0) also waits for every slot store still in flight.  Round 5, stage stamps of a measurement build
// (profiles/r5_leaf_latency_cfg3.json): the weight stage took 1 112 of a lone wave's 2 905 cycles per leaf step on cfg3 (1 830 of 4 023 at
// the bench's occupancy) against 310 of 1 571 on cfg2, where the entry is a scalar load.  Those kernels evaluate the Horner-11 form
// (no memory access: 9 more VALU, ≈ 700 fewer cycles).
// (TWIN: leaf_weight_exp_pair below repeats the table form of this function, statement for statement, for two leaves in the two lane
// parities of a wave, and leaf_weight_exp_quad for four leaves in the four lanes of a quad, leaf_weight_exp_oct for eight — change all four)
template <bool UNIFORM>
__device__ __forceinline__ double leaf_weight_exp(double x) {
  constexpr auto C = [](unsigned long long bits) { return __builtin_bit_cast(double, bits); };
  if constexpr (UNIFORM) {
  // (clamped first: ℓw = −Inf is a routine input — every divergent leaf — and a float-to-int conversion of ±Inf is undefined
  // behaviour, however the hardware's v_cvt_i32_f64 saturates; the final select still returns 0 below −1075)
  const double xc = x < -1100.0 ? -1100.0 : x;
  const double dk = __builtin_rint(xc * 92.33248261689366);                // 64 / ln 2
  double t = __builtin_fma(dk, -0x1.62e42fef00000p-7, xc);                  // − k·ln2/64: high part (20 trailing zero bits: exact product)
  t = __builtin_fma(dk, -0x1.473de6af278edp-40, t);                         // low part
  int k = (int)dk;
  k = __builtin_amdgcn_readfirstlane(k);                                    // a chain owns the wave: scalar table load
  const double tj = C(EXP2_64_BITS[k & 63]);
  double q = __builtin_fma(t, 8.3333333333333332e-03, 4.1666666666666664e-02);  // 1/120, 1/24
  q = fma3(t, q, 1.6666666666666666e-01);
  q = fma3(t, q, 0.5);
  q = fma3(t, q, 1.0);
  q = q * t;                                                                // e^t − 1
  // (no select for the underflow: x is clamped at −1100 above — ℓw = −Inf included — and from −1075 down ldexp's exponent is ≤ −1551, below
  // the smallest subnormal: the result IS 0 there; a NaN x fails the clamp's compare and propagates.  Round 5: three VALU per leaf fewer.)
  return __builtin_ldexp(__builtin_fma(tj, q, tj), k >> 6);
  }
  {
  const double xh = x < -1100.0 ? -1100.0 : x;                                    // (as above: −Inf is a routine input; ldexp underflows to 0 for it)
  const double dn = __builtin_rint(xh * C(0x3ff71547652b82feULL));                // x·log2(e)
  double t = __builtin_fma(dn, C(0xbfe62e42fefa39efULL), xh);                     // − n·ln2 (high part)
  t = __builtin_fma(dn, C(0xbc7abc9e3b39803fULL), t);                             // − n·ln2 (low part)
  double q = __builtin_fma(t, C(0x3e5ade156a5dcb37ULL), C(0x3e928af3fca7ab0cULL));
  q = fma3(t, q, C(0x3ec71dee623fde64ULL));
  q = fma3(t, q, C(0x3efa01997c89e6b0ULL));
  q = fma3(t, q, C(0x3f2a01a014761f6eULL));
  q = fma3(t, q, C(0x3f56c16c1852b7b0ULL));
  q = fma3(t, q, C(0x3f81111111122322ULL));
  q = fma3(t, q, C(0x3fa55555555502a1ULL));
  q = fma3(t, q, C(0x3fc5555555555511ULL));
  q = fma3(t, q, C(0x3fe000000000000bULL));
  q = __builtin_fma(t, q, 1.0);
  q = __builtin_fma(t, q, 1.0);
  double z = __builtin_ldexp(q, (int)dn);
  return z;   // (the underflow needs no select either: clamped at −1100, ldexp's exponent −1587 gives 0)
  }
}
template <bool UNIFORM>
__device__ __forceinline__ float leaf_weight_exp(float x) { return exp(x); }

// exp(min(0, ℓw)) for the log-domain kernels, through leaf_weight_exp: min(1, W) of the linear-domain kernels, bit for bit
// (ℓw > 0 gives exactly 1 there as well: W >= 1).  NaN propagates (Julia's min): the compare fails and exp(NaN) = NaN.
template <class T, bool UNIFORM>
__device__ __forceinline__ T alpha_from_logweight(T lw) {
  const T w = leaf_weight_exp<UNIFORM>(lw > T(0) ? T(0) : lw);
  return w >= T(1) ? T(1) : w;
}

// leaf_weight_exp<true> for TWO leaves of a chain that owns the wave in one pass: even lanes carry leaf a's argument, odd lanes leaf
// b's (pair_leaf_stats below), and lanes LA / LB are the ones whose results are read.  The two table entries are two scalar loads issued
// together — their indices come from lanes LA / LB by v_readlane — and lane parity picks the entry; everything else is lane-local, so
// each of the two lanes runs the instructions of leaf_weight_exp<true> on its own argument and returns its bits.
// TWIN of the table form of leaf_weight_exp above and of leaf_weight_exp_quad / _oct below, statement for statement: change all four.  EVERY lane's
// argument must be a value whose (int)dk is defined (the caller hands every lane one of the two leaves' arguments, so it is wherever leaf_weight_exp's own is).
template <int LA, int LB>
__device__ __forceinline__ double leaf_weight_exp_pair(double x, bool odd) {
  constexpr auto C = [](unsigned long long bits) { return __builtin_bit_cast(double, bits); };
  const double xc = x < -1100.0 ? -1100.0 : x;
  const double dk = __builtin_rint(xc * 92.33248261689366);                // 64 / ln 2
  double t = __builtin_fma(dk, -0x1.62e42fef00000p-7, xc);                  // − k·ln2/64: high part (20 trailing zero bits: exact product)
  t = __builtin_fma(dk, -0x1.473de6af278edp-40, t);                         // low part
  const int k = (int)dk;
  const int ka = __builtin_amdgcn_readlane(k, LA), kb = __builtin_amdgcn_readlane(k, LB);
  const double tja = C(EXP2_64_BITS[ka & 63]), tjb = C(EXP2_64_BITS[kb & 63]);
  const double tj = odd ? tjb : tja;
  double q = __builtin_fma(t, 8.3333333333333332e-03, 4.1666666666666664e-02);  // 1/120, 1/24
  q = fma3(t, q, 1.6666666666666666e-01);
  q = fma3(t, q, 0.5);
  q = fma3(t, q, 1.0);
  q = q * t;                                                                // e^t − 1
  return __builtin_ldexp(__builtin_fma(tj, q, tj), k >> 6);
}
template <int LA, int LB>
__device__ __forceinline__ float leaf_weight_exp_pair(float x, bool) { return exp(x); }

// The same for FOUR leaves (quad_leaf_stats below): leaf k's argument in the lanes with lane & 3 == k, lanes L0 .. L0 + 3 the ones whose
// results are read.  The four table entries are four scalar loads issued together; lane & 3 picks the entry.
// TWIN of the table form of leaf_weight_exp and of leaf_weight_exp_pair above and of leaf_weight_exp_oct below, statement for statement: change all four.  The arguments of
// lanes L0 .. L0 + 3 must be values whose (int)dk is defined, as there; the other lanes' results are never read, and quad_leaf_stats hands
// eight of them dot-product sums (see there why that is left so).
template <int L0>
__device__ __forceinline__ double leaf_weight_exp_quad(double x, bool odd, bool up) {
  constexpr auto C = [](unsigned long long bits) { return __builtin_bit_cast(double, bits); };
  const double xc = x < -1100.0 ? -1100.0 : x;
  const double dk = __builtin_rint(xc * 92.33248261689366);                // 64 / ln 2
  double t = __builtin_fma(dk, -0x1.62e42fef00000p-7, xc);                  // − k·ln2/64: high part (20 trailing zero bits: exact product)
  t = __builtin_fma(dk, -0x1.473de6af278edp-40, t);                         // low part
  const int k = (int)dk;
  const int k0 = __builtin_amdgcn_readlane(k, L0), k1 = __builtin_amdgcn_readlane(k, L0 + 1);
  const int k2 = __builtin_amdgcn_readlane(k, L0 + 2), k3 = __builtin_amdgcn_readlane(k, L0 + 3);
  const double tj0 = C(EXP2_64_BITS[k0 & 63]), tj1 = C(EXP2_64_BITS[k1 & 63]);
  const double tj2 = C(EXP2_64_BITS[k2 & 63]), tj3 = C(EXP2_64_BITS[k3 & 63]);
  const double tjl = odd ? tj1 : tj0, tjh = odd ? tj3 : tj2;
  const double tj = up ? tjh : tjl;
  double q = __builtin_fma(t, 8.3333333333333332e-03, 4.1666666666666664e-02);  // 1/120, 1/24
  q = fma3(t, q, 1.6666666666666666e-01);
  q = fma3(t, q, 0.5);
  q = fma3(t, q, 1.0);
  q = q * t;                                                                // e^t − 1
  return __builtin_ldexp(__builtin_fma(tj, q, tj), k >> 6);
}
template <int L0>
__device__ __forceinline__ float leaf_weight_exp_quad(float x, bool, bool) { return exp(x); }

// a in the even 16-lane rows, b in the odd ones: a DPP move under row_mask 0b1010 — a select that needs no lane mask in scalar registers,
// which the draws kernel is short of
__device__ __forceinline__ double sel_odd_rows(double a, double b) {
  const int lo = __builtin_amdgcn_update_dpp(__double2loint(a), __double2loint(b), 0xE4, 0xA, 0xF, false);  // quad_perm [0,1,2,3]
  const int hi = __builtin_amdgcn_update_dpp(__double2hiint(a), __double2hiint(b), 0xE4, 0xA, 0xF, false);
  return __hiloint2double(hi, lo);
}
// The same for EIGHT leaves (oct_leaf_stats below): leaves a .. d in lanes L0 .. L0 + 3, leaves e .. h in lanes L1 .. L1 + 3, one 16-lane row
// apart (L1 = L0 + 16).  The eight table entries are eight scalar loads issued together; lane & 3 and the row (sel_odd_rows) pick the entry.
// TWIN of the table form of leaf_weight_exp, of leaf_weight_exp_pair and of leaf_weight_exp_quad above, statement for statement: change all
// four.  The arguments of the eight lanes read must be values whose (int)dk is defined, as there; the other lanes' results are never read.
template <int L0, int L1>
__device__ __forceinline__ double leaf_weight_exp_oct(double x, bool odd, bool up) {
  constexpr auto C = [](unsigned long long bits) { return __builtin_bit_cast(double, bits); };
  const double xc = x < -1100.0 ? -1100.0 : x;
  const double dk = __builtin_rint(xc * 92.33248261689366);                // 64 / ln 2
  double t = __builtin_fma(dk, -0x1.62e42fef00000p-7, xc);                  // − k·ln2/64: high part (20 trailing zero bits: exact product)
  t = __builtin_fma(dk, -0x1.473de6af278edp-40, t);                         // low part
  const int k = (int)dk;
  const int k0 = __builtin_amdgcn_readlane(k, L0), k1 = __builtin_amdgcn_readlane(k, L0 + 1);
  const int k2 = __builtin_amdgcn_readlane(k, L0 + 2), k3 = __builtin_amdgcn_readlane(k, L0 + 3);
  const int k4 = __builtin_amdgcn_readlane(k, L1), k5 = __builtin_amdgcn_readlane(k, L1 + 1);
  const int k6 = __builtin_amdgcn_readlane(k, L1 + 2), k7 = __builtin_amdgcn_readlane(k, L1 + 3);
  const double tj0 = C(EXP2_64_BITS[k0 & 63]), tj1 = C(EXP2_64_BITS[k1 & 63]);
  const double tj2 = C(EXP2_64_BITS[k2 & 63]), tj3 = C(EXP2_64_BITS[k3 & 63]);
  const double tj4 = C(EXP2_64_BITS[k4 & 63]), tj5 = C(EXP2_64_BITS[k5 & 63]);
  const double tj6 = C(EXP2_64_BITS[k6 & 63]), tj7 = C(EXP2_64_BITS[k7 & 63]);
  const double tjl = odd ? tj1 : tj0, tjh = odd ? tj3 : tj2;
  const double tjl2 = odd ? tj5 : tj4, tjh2 = odd ? tj7 : tj6;
  const double tja = up ? tjh : tjl, tjb = up ? tjh2 : tjl2;
  const double tj = sel_odd_rows(tja, tjb);
  double q = __builtin_fma(t, 8.3333333333333332e-03, 4.1666666666666664e-02);  // 1/120, 1/24
  q = fma3(t, q, 1.6666666666666666e-01);
  q = fma3(t, q, 0.5);
  q = fma3(t, q, 1.0);
  q = q * t;                                                                // e^t − 1
  return __builtin_ldexp(__builtin_fma(tj, q, tj), k >> 6);
}
template <int L0, int L1>
__device__ __forceinline__ float leaf_weight_exp_oct(float x, bool, bool) { return exp(x); }

template <class T> __device__ __forceinline__ T maxabs(T a, T b) { return fabs(a) > fabs(b) ? a : b; }  // :526

// ------------------------------------------------------------------------------------------------
// cross-lane primitives inside a group of G lanes.  Butterfly all-reduce built from DPP
// (quad_perm / row_half_mirror / row_mirror), ds_swizzle (xor 16) and v_permlane32_swap (xor 32):
// no LDS traffic, no address VGPRs.  Every lane of the group ends with the same bits.
// ------------------------------------------------------------------------------------------------
template <int CTRL> __device__ __forceinline__ int dpp_i32(int v) {
  // every control used here reads a valid lane for every lane, so `old` is never taken: mov_dpp
  // (old = undef, bound_ctrl) saves the two v_mov that initialise `old` per exchanged f64
  return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, true);
}
template <int CTRL> __device__ __forceinline__ float dpp_mov(float v) {
  return __int_as_float(dpp_i32<CTRL>(__float_as_int(v)));
}
template <int CTRL> __device__ __forceinline__ double dpp_mov(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  return __hiloint2double(dpp_i32<CTRL>(hi), dpp_i32<CTRL>(lo));
}
// partner = lane ^ 16 inside each half-wave (ds_swizzle bit-mode: and=0x1f, or=0, xor=0x10)
__device__ __forceinline__ float swz16(float v) {
  return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x401F));
}
__device__ __forceinline__ double swz16(double v) {
  int lo = __builtin_amdgcn_ds_swizzle(__double2loint(v), 0x401F);
  int hi = __builtin_amdgcn_ds_swizzle(__double2hiint(v), 0x401F);
  return __hiloint2double(hi, lo);
}
// own + value of lane ^ 32.  v_permlane32_swap swaps lanes [63:32] of its first operand with
// lanes [31:0] of its second; with both = v the returned pair is {own, partner} for lanes < 32
// and {partner, own} for lanes >= 32, so p[0] + p[1] is the same sum, bit for bit, in both.
// own + value of lane ^ 16: v_permlane16_swap swaps the odd 16-lane rows of its first operand with
// the even rows of its second, so with both = v the pair holds {row 2k, row 2k+1} in every lane of
// both rows — a pure VALU exchange (ds_swizzle would go through the LDS pipeline).
__device__ __forceinline__ float xor16_sum(float v) {
  auto p = __builtin_amdgcn_permlane16_swap(__float_as_int(v), __float_as_int(v), false, false);
  return __int_as_float(p[0]) + __int_as_float(p[1]);
}
__device__ __forceinline__ double xor16_sum(double v) {
  auto lo = __builtin_amdgcn_permlane16_swap(__double2loint(v), __double2loint(v), false, false);
  auto hi = __builtin_amdgcn_permlane16_swap(__double2hiint(v), __double2hiint(v), false, false);
  return __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
}
__device__ __forceinline__ float xor32_sum(float v) {
  auto p = __builtin_amdgcn_permlane32_swap(__float_as_int(v), __float_as_int(v), false, false);
  return __int_as_float(p[0]) + __int_as_float(p[1]);
}
__device__ __forceinline__ double xor32_sum(double v) {
  auto lo = __builtin_amdgcn_permlane32_swap(__double2loint(v), __double2loint(v), false, false);
  auto hi = __builtin_amdgcn_permlane32_swap(__double2hiint(v), __double2hiint(v), false, false);
  return __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
}

// The same pair all-reduce on the MATRIX pipe for a chain that owns a whole wave (G = 64).  The trajectory kernels are
// VALU-issue bound (≈95 % VALU busy) while the MFMA pipe idles; v_mfma_*_16x16x4 sums over its k index,
// which the operand layout (probed on gfx950, ahmc_dense.hpp) maps to the four 16-lane row groups of the wave:
//     a: A[i = lane%16][k = lane/16]     b: B[k = lane/16][j = lane%16]
//     f64 acc[v]: D[i = lane/16 + 4v][j]     f32 acc[v]: D[i = 4·(lane/16) + v][j]
//   1. D = A·1 with A = a: D[i][·] = Σ_k a[lane i + 16k]; every lane then adds its 4 accumulator rows: y = the sum of a
//      over a quarter of the lanes (which quarter depends on the dtype's row mapping; the four quarters tile the wave)
//   2. the same for b
//   3. D = A′·1 with A′[i][k] = (row i belongs to the "a" half ? ya : yb) of row group k: Σ_k over the four quarters —
//      the a-rows of D hold Σa, the b-rows Σb, and every lane owns one row of each (acc[0] and acc[2] / acc[1]).
// 3 MFMA + 6 adds + 2 selects instead of 30 VALU; all lanes receive the same bits (every output element goes through
// the same FMA chain on the same inputs).  The summation ORDER differs from the DPP butterfly, i.e. last-ulp
// differences against it — inside the 1e-9 parity tolerance against the oracle, which sums in index order anyway.
// (AHMC_MFMA_REDUCE is kept: tests/test_device_primitives.py builds the probe with it)
#ifndef AHMC_MFMA_REDUCE
#define AHMC_MFMA_REDUCE 0
#endif
template <class T> struct MfmaRed;
template <> struct MfmaRed<double> {
  typedef double acc_t __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ acc_t mma(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
  static constexpr unsigned SEL = 8u;  // rows i >= 8 (acc[2], acc[3]) carry b
  static constexpr int RA = 0, RB = 2;
};
template <> struct MfmaRed<float> {
  typedef float acc_t __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ acc_t mma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
  static constexpr unsigned SEL = 1u;  // odd rows (acc[1], acc[3]) carry b
  static constexpr int RA = 0, RB = 1;
};
template <class T>
__device__ __forceinline__ void wave64_allsum2_mfma(T& a, T& b) {
  using M = MfmaRed<T>;
  const typename M::acc_t z = {T(0), T(0), T(0), T(0)};
  const T one = T(1);
  const typename M::acc_t da = M::mma(a, one, z);
  const typename M::acc_t db = M::mma(b, one, z);
  const T ya = (da[0] + da[1]) + (da[2] + da[3]);
  const T yb = (db[0] + db[1]) + (db[2] + db[3]);
  const T sel = (threadIdx.x & M::SEL) ? yb : ya;
  const typename M::acc_t d = M::mma(sel, one, z);
  a = d[M::RA];
  b = d[M::RB];
}

// all-reduce of a PAIR of values across groups of 16/32/64 lanes in ~half the instructions of two
// butterflies.  The first exchange is transposed — even lanes collect `a`, odd lanes collect `b`
// — so every later stage moves one value instead of two; rotations inside the 16-lane row keep
// the lane parity, the row pairs/halves are joined as before, and lanes 0 / 1 of the row are
// broadcast back (row_newbcast).  Every lane ends with the bits of those two lanes.
//   f64: 7 + 3 + 3 + 3 (+5 +5) + 4 = 30 VALU for G = 64, against 2 x 22.
// The exchanges of a butterfly on the LDS pipe instead of the VALU: ds_swizzle_b32 (any lane pattern inside 32 lanes)
// and ds_bpermute_b32 (lane ^ 32) move the data, the VALU only adds.  An exchange costs 2 DS instructions instead of 2
// (DPP) or 4 (permlane: 2 copies + 2 swaps) VALU instructions; the LDS pipe has its own issue port and is almost idle in
// these kernels (≈17 of ≈900 wave-cycles per leapfrog), the VALU port is the bottleneck.  The price is latency
// (≈60-100 cycles per exchange against 8): it pays only while the other waves of the SIMD fill the gap.
// AHMC_DS_REDUCE: bit 0 = the xor-16 / xor-32 stages, bit 1 = also the four in-row stages, bit 2 = the final broadcast.
// (kept: tests/test_device_primitives.py builds the probe with it)
#ifndef AHMC_DS_REDUCE
#define AHMC_DS_REDUCE 0
#endif
template <int PATTERN> __device__ __forceinline__ float ds_swz(float v) {
  return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), PATTERN));
}
template <int PATTERN> __device__ __forceinline__ double ds_swz(double v) {
  return __hiloint2double(__builtin_amdgcn_ds_swizzle(__double2hiint(v), PATTERN), __builtin_amdgcn_ds_swizzle(__double2loint(v), PATTERN));
}
__device__ __forceinline__ float ds_xor32(float v) {
  return __int_as_float(__builtin_amdgcn_ds_bpermute((int)((__lane_id() ^ 32u) << 2), __float_as_int(v)));
}
__device__ __forceinline__ double ds_xor32(double v) {
  const int addr = (int)((__lane_id() ^ 32u) << 2);
  return __hiloint2double(__builtin_amdgcn_ds_bpermute(addr, __double2hiint(v)), __builtin_amdgcn_ds_bpermute(addr, __double2loint(v)));
}
// bit-mode swizzle patterns: offset = (xor << 10) | (or << 5) | and; lane' = ((lane & and) | or) ^ xor within 32 lanes
constexpr int SWZ_XOR1 = (1 << 10) | 0x1F, SWZ_XOR2 = (2 << 10) | 0x1F, SWZ_XOR4 = (4 << 10) | 0x1F, SWZ_XOR8 = (8 << 10) | 0x1F, SWZ_XOR16 = (16 << 10) | 0x1F;

template <int G, class T>
__device__ __forceinline__ void wave_allsum2(T& a, T& b) {
  static_assert(G == 16 || G == 32 || G == 64, "pair reduction needs whole 16-lane rows");
  if constexpr (AHMC_MFMA_REDUCE && G == 64) {
    wave64_allsum2_mfma(a, b);
    return;
  }
  if constexpr ((AHMC_DS_REDUCE & 2) != 0) {
    // every exchange on the LDS pipe: transposed first stage (even lanes collect a, odd lanes b), xor butterflies after
    const bool odd = (threadIdx.x & 1u) != 0;
    const T keep = odd ? b : a, send = odd ? a : b;
    T x = keep + ds_swz<SWZ_XOR1>(send);
    x += ds_swz<SWZ_XOR2>(x);
    x += ds_swz<SWZ_XOR4>(x);
    x += ds_swz<SWZ_XOR8>(x);
    if constexpr (G >= 32) x += ds_swz<SWZ_XOR16>(x);
    if constexpr (G >= 64) x += ds_xor32(x);
    const T y = ds_swz<SWZ_XOR1>(x);  // the partner lane holds the other sum
    a = odd ? y : x;
    b = odd ? x : y;
    return;
  }
  const bool odd = (threadIdx.x & 1u) != 0;
  const T keep = odd ? b : a, send = odd ? a : b;
  T x = keep + dpp_mov<0xB1>(send);  // quad_perm [1,0,3,2]
  x += dpp_mov<0x4E>(x);             // quad_perm [2,3,0,1]
  x += dpp_mov<0x124>(x);            // row_ror:4
  x += dpp_mov<0x128>(x);            // row_ror:8
  if constexpr ((AHMC_DS_REDUCE & 1) != 0) {
    if constexpr (G >= 32) x += ds_swz<SWZ_XOR16>(x);
    if constexpr (G >= 64) x += ds_xor32(x);
  } else {
    if constexpr (G >= 32) x = xor16_sum(x);
    if constexpr (G >= 64) x = xor32_sum(x);
  }
  a = dpp_mov<0x150>(x);  // row_newbcast:0
  b = dpp_mov<0x151>(x);  // row_newbcast:1
}

// Σa <= 0 || Σb <= 0 for a chain that owns one whole wave, as ONE wave-uniform (scalar) predicate — the generalised U-turn test, which
// needs two signs and no sums.  Σa and Σb go through exactly the additions of wave_allsum2<64> (same transposed first stage, same
// stages, same order), but the two row_newbcast that would hand lanes 0 / 1 of the row to all 64 lanes are not made: after the xor-32
// stage lane 0 already holds the final bits of Σa and lane 1 those of Σb, so one compare of that register and bits 0 / 1 of its lane
// mask are the two decisions.  ONLY those two lanes: the in-row rotations associate the four quads' sums in a rotated order from quad
// to quad ((Q0 + Q3) + (Q2 + Q1) in quad 0, (Q1 + Q0) + (Q3 + Q2) in quad 1: row_ror:n reads lane l − n), so another even lane may hold Σa rounded differently —
// wave_allsum2 returns lane 0's and lane 1's bits, and so must this.  Rows need no care: xor16 / xor32 add {lower, upper} in the
// same order on both sides.  NaN: `<=` is false, as in the two compares this replaces.
// (The first arm below — wave_allsum2 + two compares — is the arm of the experimental reductions alone: -DAHMC_MFMA_REDUCE=1, or
// -DAHMC_DS_REDUCE with bit 0 or 1, whose additions differ from the DPP butterfly's and which therefore go through their own
// wave_allsum2.  AHMC_DS_REDUCE=4 moves only the final broadcast to the LDS pipe, which this predicate does not make: it takes the
// second arm.)
template <class T>
__device__ __forceinline__ bool wave64_any_le0_pair(T a, T b) {
  if constexpr (AHMC_MFMA_REDUCE || (AHMC_DS_REDUCE & 3) != 0) {
    wave_allsum2<64>(a, b);
    return (__builtin_amdgcn_ballot_w64(a <= T(0)) != 0) || (__builtin_amdgcn_ballot_w64(b <= T(0)) != 0);
  } else {
    const bool odd = (threadIdx.x & 1u) != 0;
    const T keep = odd ? b : a, send = odd ? a : b;
    T x = keep + dpp_mov<0xB1>(send);  // quad_perm [1,0,3,2]
    x += dpp_mov<0x4E>(x);             // quad_perm [2,3,0,1]
    x += dpp_mov<0x124>(x);            // row_ror:4
    x += dpp_mov<0x128>(x);            // row_ror:8
    x = xor16_sum(x);
    x = xor32_sum(x);
    return (__builtin_amdgcn_ballot_w64(x <= T(0)) & 3ull) != 0ull;  // lane 0: Σa, lane 1: Σb
  }
}

// the same for FOUR values: two transposed exchanges (lane & 1, then lane & 2) leave one value per lane, lanes 0..3 of
// the row are broadcast back.  14 + 7 + 3 + 3 (+5 +5) + 8 = 45 VALU for G = 64 against 2 x 30, and the additions each
// value goes through are those of wave_allsum2 (a, b as there; c, d as a second pair), so the results are bit-identical.
template <int G, class T>
__device__ __forceinline__ void wave_allsum4(T& a, T& b, T& c, T& d) {
  static_assert(G == 16 || G == 32 || G == 64, "quad reduction needs whole 16-lane rows");
  const bool odd = (threadIdx.x & 1u) != 0, up = (threadIdx.x & 2u) != 0;
  const T x = (odd ? b : a) + dpp_mov<0xB1>(odd ? a : b);  // quad_perm [1,0,3,2]
  const T y = (odd ? d : c) + dpp_mov<0xB1>(odd ? c : d);
  T z = (up ? y : x) + dpp_mov<0x4E>(up ? x : y);          // quad_perm [2,3,0,1]
  z += dpp_mov<0x124>(z);                                   // row_ror:4
  z += dpp_mov<0x128>(z);                                   // row_ror:8
  if constexpr (G >= 32) z = xor16_sum(z);
  if constexpr (G >= 64) z = xor32_sum(z);
  a = dpp_mov<0x150>(z);  // row_newbcast:0..3
  b = dpp_mov<0x151>(z);
  c = dpp_mov<0x152>(z);
  d = dpp_mov<0x153>(z);
}

// What a PAIR of consecutive NUTS leaves and their level-0 merge need from the wave, in ONE reduction (the pair step of k_nuts): the two
// leaves' energies ea, eb (lane partials in, sums out, the same bits in every lane) and the generalised U-turn decision
// Σda <= 0 || Σdb <= 0 of the merged pair as one wave-uniform predicate.  The lane exchanges are wave_allsum4<64>'s with (da, db) as its
// first pair and (ea, eb) as its second:
//   * lanes 0 / 1 of the transposed register hold Σda / Σdb with the bits of wave_allsum2<64> — the decision is the one
//     wave64_any_le0_pair takes (one compare, bits 0 / 1 of its lane mask; no broadcast of the two sums);
//   * lanes 4q + 2 / 4q + 3 hold Σea / Σeb.  The single-value butterfly wave_allsum<64, T, 1> joins the four quad sums of a row as
//     (Q0 + Q1) + (Q2 + Q3); the two in-row rotations here join them as (Qq + Qq∓1) + (Qq∓2 + Qq∓3), which is that grouping (up to
//     the order of the operands of an addition, which changes no bit) in every second quad only.  row_ror:n on gfx950 hands lane l the
//     value of lane l − n — decided by the device probe (tests/device_probe/pair_red.hip), not by the manual — so the matching quads
//     are 1 and 3, and the energies are broadcast from lanes 6 / 7 of the row.  AHMC_PAIR_RED_QUAD names the quad (the probe
//     builds the other one as well).
// f64: 14 + 7 + 3 + 3 + 5 + 5 + 1 + 4 = 42 VALU, against 22 + 22 + 27 for two leaves' wave_allsum and the merge's predicate.
// (The engine calls only wave64_pair_reduce_t below.  This function stays because tests/device_probe/pair_red.hip and pair_stats.hip
// call it: it is what they hold the transposed form to.  TWIN of wave64_pair_reduce_t up to `le0`, and of wave64_quad_reduce_t in what each
// value goes through: change all.)
#ifndef AHMC_PAIR_RED_QUAD
#define AHMC_PAIR_RED_QUAD 1
#endif
template <class T, int Q = AHMC_PAIR_RED_QUAD>
__device__ __forceinline__ bool wave64_pair_reduce(T da, T db, T& ea, T& eb) {
  static_assert(Q >= 0 && Q <= 3, "a row has four quads");
  const bool odd = (threadIdx.x & 1u) != 0, up = (threadIdx.x & 2u) != 0;
  const T x = (odd ? db : da) + dpp_mov<0xB1>(odd ? da : db);  // quad_perm [1,0,3,2]
  const T y = (odd ? eb : ea) + dpp_mov<0xB1>(odd ? ea : eb);
  T z = (up ? y : x) + dpp_mov<0x4E>(up ? x : y);              // quad_perm [2,3,0,1]
  z += dpp_mov<0x124>(z);                                       // row_ror:4
  z += dpp_mov<0x128>(z);                                       // row_ror:8
  z = xor16_sum(z);
  z = xor32_sum(z);
  const bool le0 = (__builtin_amdgcn_ballot_w64(z <= T(0)) & 3ull) != 0ull;  // lane 0: Σda, lane 1: Σdb
  ea = dpp_mov<0x150 + 4 * Q + 2>(z);  // row_newbcast
  eb = dpp_mov<0x150 + 4 * Q + 3>(z);
  return le0;
}
// wave64_pair_reduce without the four row_newbcast moves: the same exchanges, additions and decision, and the TRANSPOSED register itself
// comes back in z — lanes 0 / 1 of a row hold Σda / Σdb, lanes 4q + 2 / 4q + 3 hold Σea / Σeb (with the butterfly's bits in quads 1 and 3,
// as above).  For pair_leaf_stats (below), which does both leaves' scalar work in the two lane parities instead of once per broadcast
// value.  TWIN of wave64_pair_reduce up to `le0`: change both (tests/device_probe/pair_stats.hip runs them on the same data); TWIN of
// wave64_quad_reduce_t below in what each value goes through (tests/device_probe/quad_red.hip).
template <class T>
__device__ __forceinline__ bool wave64_pair_reduce_t(T da, T db, T ea, T eb, T& z) {
  const bool odd = (threadIdx.x & 1u) != 0, up = (threadIdx.x & 2u) != 0;
  const T x = (odd ? db : da) + dpp_mov<0xB1>(odd ? da : db);  // quad_perm [1,0,3,2]
  const T y = (odd ? eb : ea) + dpp_mov<0xB1>(odd ? ea : eb);
  z = (up ? y : x) + dpp_mov<0x4E>(up ? x : y);                // quad_perm [2,3,0,1]
  z += dpp_mov<0x124>(z);                                       // row_ror:4
  z += dpp_mov<0x128>(z);                                       // row_ror:8
  z = xor16_sum(z);
  z = xor32_sum(z);
  return (__builtin_amdgcn_ballot_w64(z <= T(0)) & 3ull) != 0ull;  // lane 0: Σda, lane 1: Σdb
}

// What FOUR consecutive NUTS leaves a, b, c, d, their two level-0 merges and the level-1 merge of the two pairs need from the wave, in ONE
// reduction (the quad step of k_nuts): ten lane partials in — the four energies e[0..3], the dot products of the merges (a,b) and (c,d) and
// those of the level-1 merge — and one register out.  All FOUR exchanges inside a 16-lane row are transposed (lane & 1, lane & 2, then
// the quad's index bits lane & 4 and lane & 8), so a row of w holds
//     lanes 0 / 1: Σdab[0] / Σdab[1]     lanes 2 / 3: Σdcd[0] / Σdcd[1]     lanes 4 .. 7: Σe[0] .. Σe[3]     lanes 8 / 9: Σdl[0] / Σdl[1]
// and the three U-turn decisions are bits 0-1, 2-3 and 8-9 of ONE compare's lane mask (no sum is broadcast).  The bits are those of the
// primitives this replaces.  Inside a quad every slot sums (own pair) + (other pair), whichever lane collects it.  Across the quads of a row
// the rotations join (Qq + Qq−1) + (Qq−2 + Qq−3) in quad q (row_ror:n hands lane l the value of lane l − n, tests/device_probe/pair_red.hip):
//   * quad 0 has wave_allsum2<64>'s (Q0 + Q3) + (Q2 + Q1) — where wave64_pair_reduce_t and wave64_any_le0_pair read their dot products;
//     quad 2 has (Q2 + Q1) + (Q0 + Q3), the same two sums added in the other order: the same bits.  The dot products sit in quads 0 and 2;
//   * quad 1 has the single-value butterfly's (Q1 + Q0) + (Q3 + Q2) — where wave64_pair_reduce_t keeps its energies.  The energies sit in quad 1.
// The transposed rotation of a stage sends what the receiving quad collects, so a value's partner sums come from the quads the plain
// rotation would have read.  Rows: xor16 / xor32 add {lower, upper} in the same order on both sides, as everywhere.
// f64: 5 × 7 + (7 + 7 + 3) + (7 + 3) + 7 + 5 + 5 + 1 = 80 VALU, against 2 × 42 for two pair reductions and 27 for the level-1 merge's predicate.
// TWIN of wave64_pair_reduce_t and wave64_any_le0_pair in what each value goes through: change all (tests/device_probe/quad_red.hip runs
// them on the same data).
// The FIRST exchange is a function of its own (wave64_quad_pair): it needs one pair of values only, so the quad step makes it as soon as
// a pair's two partials exist and carries ONE register per pair, not two, across the leapfrogs that follow.
template <class T>
__device__ __forceinline__ T wave64_quad_pair(T a, T b) {
  const bool odd = (threadIdx.x & 1u) != 0;
  return (odd ? b : a) + dpp_mov<0xB1>(odd ? a : b);  // quad_perm [1,0,3,2]: even lanes collect a, odd lanes b
}
// xab, xcd, xl: wave64_quad_pair of the dot products of the merges (a,b), (c,d) and of the level-1 merge; yab, ycd: of (e_a, e_b), (e_c, e_d)
template <class T>
__device__ __forceinline__ unsigned long long wave64_quad_reduce_t(T xab, T xcd, T xl, T yab, T ycd, T& w) {
  const bool up = (threadIdx.x & 2u) != 0, oq = (threadIdx.x & 4u) != 0, hq = (threadIdx.x & 8u) != 0;
  const T rd = (up ? xcd : xab) + dpp_mov<0x4E>(up ? xab : xcd);               // quad_perm [2,3,0,1]
  const T re = (up ? ycd : yab) + dpp_mov<0x4E>(up ? yab : ycd);
  const T rl = xl + dpp_mov<0x4E>(xl);
  const T z = (oq ? re : rd) + dpp_mov<0x124>(oq ? rd : re);                   // row_ror:4
  const T zl = rl + dpp_mov<0x124>(rl);
  w = (hq ? zl : z) + dpp_mov<0x128>(hq ? z : zl);                             // row_ror:8
  w = xor16_sum(w);
  w = xor32_sum(w);
  return __builtin_amdgcn_ballot_w64(w <= T(0));
}
constexpr unsigned long long QUAD_TURN_AB = 0x3ull, QUAD_TURN_CD = 0xCull, QUAD_TURN_L1 = 0x300ull;  // lanes of the three decisions in that mask

// What EIGHT consecutive NUTS leaves a .. h, their four level-0 merges, their two level-1 merges and the level-2 merge of the two halves need
// from the wave, in ONE reduction (the octo step of k_nuts): 22 lane partials in — eight energies and seven pairs of dot products — and one
// register out.  Each half (a,b,c,d) / (e,f,g,h) goes through the four in-row exchanges of wave64_quad_reduce_t on its own, as soon as it is
// complete (wave64_oct_rows_de + wave64_oct_rows: ONE register per half crosses the other half's leapfrogs); the second half carries the level-2 merge's pair in the
// slots of quad 2 where the first has its level-1 sums a second time:
//     lanes 0 / 1: Σd(ab | ef)   lanes 2 / 3: Σd(cd | gh)   lanes 4 .. 7: Σe   lanes 8 / 9: Σd level 1   lanes 10 / 11: Σd level 2 (second half)
// Dot products sit in quads 0 and 2 and energies in quad 1 — where the groupings of the primitives this replaces hold, as derived at
// wave64_quad_reduce_t: quad 2 joins (Q2 + Q1) + (Q0 + Q3), wave_allsum2<64>'s two sums added in the other order, so the level-2 pair has
// wave64_any_le0_pair's bits there.  Inside a quad a slot of the upper two lanes sums (own pair) + (other pair) like one of the lower two.
// The xor-16 exchange is TRANSPOSED as well: v_permlane16_swap of the two halves' registers hands rows 0 / 2 the first half's
// {row 2k, row 2k + 1} and rows 1 / 3 the second half's, so one addition makes lower + upper for both — the order of xor16_sum — and ONE
// register goes through the xor-32 exchange: rows 0 and 2 hold the first half's sixteen slots, rows 1 and 3 the second half's.
// All seven U-turn decisions are bits of ONE compare's lane mask; no sum is broadcast.
// f64: 2 × 69 (the halves' in-row stages) + 7 + 3 (the level-2 pair) + 3 + 5 + 1 = 157 VALU, against 2 × 80 for two quad reductions and 27
// for the level-2 merge's predicate — and one chain of dependent stages instead of three.
// TWIN of wave64_quad_reduce_t (each half) and of wave64_any_le0_pair (the level-2 pair) in what each value goes through: change all
// (tests/device_probe/oct_red.hip runs them on the same data).
// xab, xcd, yab, ycd: as for wave64_quad_reduce_t; xl: wave64_quad_pair of the half's level-1 dot products; xl2: of the level-2 merge's (second
// half), or xl again (first half)
// (two steps: the four level-0 / energy pair registers are one register after wave64_oct_rows_de, made as soon as the half's last leapfrog
// is through, so that only it and the level-1 pair wait for the level-2 merge's vector work)
template <class T>
__device__ __forceinline__ T wave64_oct_rows_de(T xab, T xcd, T yab, T ycd) {
  const bool up = (threadIdx.x & 2u) != 0, oq = (threadIdx.x & 4u) != 0;
  const T rd = (up ? xcd : xab) + dpp_mov<0x4E>(up ? xab : xcd);               // quad_perm [2,3,0,1]
  const T re = (up ? ycd : yab) + dpp_mov<0x4E>(up ? yab : ycd);
  return (oq ? re : rd) + dpp_mov<0x124>(oq ? rd : re);                        // row_ror:4
}
template <class T>
__device__ __forceinline__ T wave64_oct_rows(T z, T xl, T xl2) {
  const bool up = (threadIdx.x & 2u) != 0, hq = (threadIdx.x & 8u) != 0;
  const T rl = (up ? xl2 : xl) + dpp_mov<0x4E>(up ? xl : xl2);                 // quad_perm [2,3,0,1]
  const T zl = rl + dpp_mov<0x124>(rl);                                        // row_ror:4
  return (hq ? zl : z) + dpp_mov<0x128>(hq ? z : zl);                          // row_ror:8
}
// own half's {row 2k} + {row 2k + 1}: even rows collect h1, odd rows h2 (v_permlane16_swap swaps the odd rows of its first operand with the
// even rows of its second)
__device__ __forceinline__ float xor16_sum_t(float h1, float h2) {
  auto p = __builtin_amdgcn_permlane16_swap(__float_as_int(h1), __float_as_int(h2), false, false);
  return __int_as_float(p[0]) + __int_as_float(p[1]);
}
__device__ __forceinline__ double xor16_sum_t(double h1, double h2) {
  auto lo = __builtin_amdgcn_permlane16_swap(__double2loint(h1), __double2loint(h2), false, false);
  auto hi = __builtin_amdgcn_permlane16_swap(__double2hiint(h1), __double2hiint(h2), false, false);
  return __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
}
// h1, h2: wave64_oct_rows of the two halves
template <class T>
__device__ __forceinline__ unsigned long long wave64_oct_reduce_t(T h1, T h2, T& w) {
  w = xor16_sum_t(h1, h2);
  w = xor32_sum(w);
  return __builtin_amdgcn_ballot_w64(w <= T(0));
}
// lanes of the seven decisions in that mask: the first half's as in a quad, the second half's one row up
constexpr unsigned long long OCT_TURN_AB = QUAD_TURN_AB, OCT_TURN_CD = QUAD_TURN_CD, OCT_TURN_ABCD = QUAD_TURN_L1;
constexpr unsigned long long OCT_TURN_EF = QUAD_TURN_AB << 16, OCT_TURN_GH = QUAD_TURN_CD << 16, OCT_TURN_EFGH = QUAD_TURN_L1 << 16;
constexpr unsigned long long OCT_TURN_L2 = 0xC00ull << 16;

// all-reduce (sum) of K independent values across the G lanes of each group
template <int G, class T, int K>
__device__ __forceinline__ void wave_allsum(T (&v)[K]) {
  static_assert(G == 1 || G == 2 || G == 4 || G == 8 || G == 16 || G == 32 || G == 64, "bad group size");
  if constexpr (G >= 16 && K == 4) {
    wave_allsum4<G>(v[0], v[1], v[2], v[3]);
    return;
  }
  if constexpr (G >= 16 && K % 2 == 0) {
#pragma unroll
    for (int k = 0; k < K; k += 2) wave_allsum2<G>(v[k], v[k + 1]);
    return;
  }
  if constexpr (G >= 2) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += dpp_mov<0xB1>(v[k]);  // quad_perm [1,0,3,2]
  }
  if constexpr (G >= 4) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += dpp_mov<0x4E>(v[k]);  // quad_perm [2,3,0,1]
  }
  if constexpr (G >= 8) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += dpp_mov<0x141>(v[k]);  // row_half_mirror
  }
  if constexpr (G >= 16) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += dpp_mov<0x140>(v[k]);  // row_mirror
  }
  if constexpr (G >= 32) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if constexpr ((AHMC_DS_REDUCE & 1) != 0) v[k] += ds_swz<SWZ_XOR16>(v[k]); else v[k] = xor16_sum(v[k]);
    }
  }
  if constexpr (G >= 64) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if constexpr ((AHMC_DS_REDUCE & 1) != 0) v[k] += ds_xor32(v[k]); else v[k] = xor32_sum(v[k]);
    }
  }
}
// Exchange buffer of the multi-wave groups (G = 128/256/512: one chain per workgroup of G/64 waves,
// D up to 4096).  All waves of such a group execute identical control flow (every decision is taken
// on values that are bit-identical in all lanes), so the barriers below are always reached together.
__device__ __forceinline__ double* xwave_buf() {
  __shared__ __attribute__((aligned(16))) double buf[8 * 8];
  return buf;
}

// all-reduce (sum) of K values across the G lanes of each group; G > 64 = G/64 whole waves
template <int G, class T, int K>
__device__ __forceinline__ void group_allsum(T (&v)[K]) {
  if constexpr (G <= 64) {
    wave_allsum<G>(v);
  } else {
    static_assert(G == 128 || G == 256 || G == 512, "bad multi-wave group size");
    static_assert(K <= 8, "at most 8 values per reduction");
    constexpr int NW = G / 64;
    wave_allsum<64>(v);
    double* b = xwave_buf();
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) b[w * 8 + k] = (double)v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
      T s = 0;
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) s += (T)b[ww * 8 + k];  // fixed order: same bits in every wave
      v[k] = s;
    }
    __syncthreads();
  }
}
template <int G, class T>
__device__ __forceinline__ T group_sum1(T x) {
  T v[1] = {x};
  group_allsum<G>(v);
  return v[0];
}

// The same sum with ONE barrier, for a call site whose next use of ITS OWN buffer is always preceded by another barrier of the
// workgroup (then every wave has read the buffer before it is written again).  Round 4: the hierarchical-Gaussian leaf of a
// multi-wave chain took eight barriers (two broadcasts, the target's two sums, ℓπ / ℓκ: two each); with an exchange buffer per
// site — the broadcast's next write follows the sums' barrier, the sums' follows the next leaf's broadcast, the energies' follows
// both — it takes three.  Same additions in the same order as group_allsum: the bits do not change.
__device__ __forceinline__ double* xwave_buf_h() {
  __shared__ __attribute__((aligned(16))) double buf[2];
  return buf;
}
__device__ __forceinline__ double* xwave_buf_s() {
  __shared__ __attribute__((aligned(16))) double buf[8 * 2];
  return buf;
}
__device__ __forceinline__ double* xwave_buf_f() {
  __shared__ __attribute__((aligned(16))) double buf[8 * 4];
  return buf;
}
// Round 6: μ and log τ of the NEXT leaf's position, written by the chain's first lane just before the barrier of THIS leaf's energy
// exchange (hier_publish_next) and read at the top of the next leaf's target_eval (use_pre) — the broadcast exchange of its own and its
// barrier are gone for every leaf but the first of a doubling.  Lifetime: read before the next leaf's sums' barrier, written again after it.
__device__ __forceinline__ double* xwave_buf_p() {
  __shared__ __attribute__((aligned(16))) double buf[2];
  return buf;
}
template <int G, class T, int K>
__device__ __forceinline__ void group_allsum_once(T (&v)[K], double* b) {
  static_assert(G == 128 || G == 256 || G == 512, "multi-wave groups only");
  constexpr int NW = G / 64;
  wave_allsum<64>(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) b[w * K + k] = (double)v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    T s = 0;
#pragma unroll
    for (int ww = 0; ww < NW; ++ww) s += (T)b[ww * K + k];  // fixed order: same bits in every wave
    v[k] = s;
  }
}
// the all-reduce that ends a leapfrog (ℓπ, ℓκ and what rides with them): one barrier where the target's own exchanges separate its uses
template <int G, int TK, class T, int K>
__device__ __forceinline__ void leapfrog_allsum(T (&v)[K]) {
  if constexpr (G > 64 && TK == 3) {
    static_assert(K <= 4, "xwave_buf_f holds four values per wave");
    group_allsum_once<G>(v, xwave_buf_f());
  } else {
    group_allsum<G>(v);
  }
}

// broadcast the value held by lane `src` (0..G-1) of the group to the whole group
template <int G>
__device__ __forceinline__ int group_bcast_i32(int v, int src) {
  int base = (int)(__lane_id() & ~(unsigned)((G > 64 ? 64 : G) - 1));
  return __builtin_amdgcn_ds_bpermute((base + src) << 2, v);
}
template <int G, class T>
__device__ __forceinline__ T xwave_bcast(T v, int src) {
  double* b = xwave_buf();
  if ((int)threadIdx.x == src) b[0] = (double)v;
  __syncthreads();
  T r = (T)b[0];
  __syncthreads();
  return r;
}
template <int G> __device__ __forceinline__ float group_bcast(float v, int src) {
  if constexpr (G > 64) return xwave_bcast<G>(v, src);
  else return __int_as_float(group_bcast_i32<G>(__float_as_int(v), src));
}
template <int G> __device__ __forceinline__ double group_bcast(double v, int src) {
  if constexpr (G > 64) return xwave_bcast<G>(v, src);
  else return __hiloint2double(group_bcast_i32<G>(__double2hiint(v), src), group_bcast_i32<G>(__double2loint(v), src));
}

// ------------------------------------------------------------------------------------------------
// built-in log-density families (include/ahmc_hip.h AHMC_TARGET_*).  `grad` receives the
// reference's cached gradient -∇ℓπ (src/hamiltonian.jl:45-48).  The return value is this lane's
// PARTIAL of ℓπ: the caller sums it over the group together with the kinetic partial, so the
// common Gaussian case costs one butterfly per leapfrog step.
// ------------------------------------------------------------------------------------------------
template <class T>
struct TargetP {
  int kind;
  int D;
  const T* params;
};

#define AHMC_LOG2PI 1.8378770664093454835606594728112

#ifdef AHMC_USER_TARGET_HEADER
// A target plugin: the user's log-density as a device function, compiled into every trajectory kernel (TK = 4).  The header
// defines, in namespace ahmc_user (contract and helpers: include/ahmc_user_target.h):
//   template <class T, int G, int E>
//   __device__ T logdensity(const T* params, int D, const T (&theta)[E], T (&grad_neg)[E], int lane, int d0);
}  // namespace ahmc
#include AHMC_USER_TARGET_HEADER
namespace ahmc {
#endif

// use_pre (multi-wave hierarchical target only): μ, log τ of this position were published by the previous leaf (xwave_buf_p)
template <class T, int G, int E, int TK>
__device__ __forceinline__ T target_eval(const TargetP<T>& tp, const T (&th)[E], T (&grad)[E], int lane, int d0, bool use_pre = false) {
  const T log2pi = (T)AHMC_LOG2PI;
  const int D = tp.D;
  T part = 0;
  {  // the target family is a compile-time parameter: a 4-way run-time switch costs 36 VGPRs in k_nuts
    if constexpr (TK == 0) {  // AHMC_TARGET_ISO_GAUSS (test/common.jl:40-44, m = 0, s = 1)
      // padded elements (d >= D) hold θ = 0 in every kernel, so they need no mask: Σθ² and g = θ are
      // already right, and the constant −D/2·log 2π goes in once (lane 0's partial)
      T ss = 0;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        ss += th[e] * th[e];
        grad[e] = th[e];
      }
      part = -ss / 2;
      if (lane == 0) part -= (T)D * log2pi / 2;
    }
    if constexpr (TK == 1) {  // AHMC_TARGET_DIAG_GAUSS: params = m[D], s[D]
#pragma unroll
      for (int e = 0; e < E; ++e) {
        // branch-free on purpose: padded elements (d >= D) read the last valid parameters and are zeroed by a select at the end.
        // (With `ok ? load : 0` the loads, the log and the divisions sat in exec-masked blocks — which is where the register
        // allocator then parked spills of values the other lanes need too: isa_check.py, round 4.)
        const bool ok = d0 + e < D;
        const int d = ok ? d0 + e : D - 1;
        const T m = tp.params[d];
        const T s = tp.params[D + d];
        const T diff = m - th[e];
        const T s2 = s * s;
        const T val = -(log2pi + 2 * log(s) + diff * diff / s2) / 2;
        const T gv = -(diff / s2);
        part += ok ? val : T(0);
        grad[e] = ok ? gv : T(0);
      }

    }
    if constexpr (TK == 2) {  // AHMC_TARGET_FUNNEL (research/notebooks/geweke_test.ipynb cell 4)
      T y = group_bcast<G>(th[0], 0);
      T ssp = 0;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        int d = d0 + e;
        ssp += (d >= 1 && d < D) ? th[e] * th[e] : T(0);
      }
      T ss = group_sum1<G>(ssp);
      T ey = exp(-y);
      T nm1 = (T)(D - 1);
      T total = -(log2pi + 2 * log(T(3)) + y * y / 9) / 2 - nm1 * (log2pi + y) / 2 - ss * ey / 2;
      part = (lane == 0) ? total : T(0);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        int d = d0 + e;
        T gv = (d == 0) ? -(-y / 9 - nm1 / 2 + ss * ey / 2) : th[e] * ey;
        grad[e] = (d < D) ? gv : T(0);
      }

    }
#ifdef AHMC_USER_TARGET_HEADER
    if constexpr (TK == 4) part = ::ahmc_user::logdensity<T, G, E>(tp.params, D, th, grad, lane, d0);  // target plugin
#endif
    if constexpr (TK == 3) {  // AHMC_TARGET_HIER_GAUSS: θ = (μ, log τ, x...)
      T mu, lt;
      if constexpr (G > 64) {  // (E >= 4 here: both leading elements sit in the chain's first lane; one exchange, one barrier)
        // Invariants of the one-barrier exchanges (xwave_buf_h / _s / _f): ONE chain per workgroup of G threads — threadIdx.x == 0 is the
        // chain's first lane and wave w = threadIdx.x >> 6 (the launch plan of every multi-wave geometry, ahmc_kernels.hpp: group_grid);
        // θ[0] and θ[1] in that lane; and every leapfrog_allsum<G,3> follows a target_eval, whose barriers separate two uses of a buffer.
        static_assert(E >= 2, "multi-wave hierarchical target: mu and log tau must both sit in the chain's first lane (E >= 2)");
        if (use_pre) {   // (chain-uniform: every wave of the workgroup takes the same branch)
          const double* hp = xwave_buf_p();
          mu = (T)hp[0];
          lt = (T)hp[1];
        } else {
          double* hb = xwave_buf_h();
          if (threadIdx.x == 0) {
            hb[0] = (double)th[0];
            hb[1] = (double)th[E >= 2 ? 1 : 0];
          }
          __syncthreads();
          mu = (T)hb[0];
          lt = (T)hb[1];
        }
      } else {
        mu = group_bcast<G>(th[0], 0);
        lt = (E >= 2) ? group_bcast<G>(th[E >= 2 ? 1 : 0], 0) : group_bcast<G>(th[0], 1);
      }
      T s[2] = {0, 0};
#pragma unroll
      for (int e = 0; e < E; ++e) {
        int d = d0 + e;
        T df = th[e] - mu;
        bool ok = d >= 2 && d < D;
        s[0] += ok ? df : T(0);
        s[1] += ok ? df * df : T(0);
      }
      if constexpr (G > 64) group_allsum_once<G>(s, xwave_buf_s());
      else group_allsum<G>(s);
      T itau2 = exp(-2 * lt);
      T n = (T)(D - 2);
      T total = -(log2pi + mu * mu) / 2 - (log2pi + lt * lt) / 2 - n * (log2pi + 2 * lt) / 2 - s[1] * itau2 / 2;
      part = (lane == 0) ? total : T(0);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        int d = d0 + e;
        T gv;
        if (d == 0) gv = -(-mu + s[0] * itau2);
        else if (d == 1) gv = -(-lt - n + s[1] * itau2);
        else gv = (th[e] - mu) * itau2;
        grad[e] = (d < D) ? gv : T(0);
      }

    }
#ifdef AHMC_USER_TARGET_HEADER
    constexpr int TK_MAX = 4;
#else
    constexpr int TK_MAX = 3;
#endif
    if constexpr (TK < 0 || TK > TK_MAX) {
#pragma unroll
      for (int e = 0; e < E; ++e) grad[e] = Lim<T>::nan();
      part = Lim<T>::nan();
    }
  }
  return part;
}

// ------------------------------------------------------------------------------------------------
// per-chain phase point in registers and one leapfrog step (src/integrator.jl:233-243)
// ------------------------------------------------------------------------------------------------
template <class T, int E>
struct Point {
  T th[E], r[E], g[E];  // θ, r, -∇ℓπ(θ)
  T lp, lk;             // ℓπ(θ), ℓκ = -K(r)  (sanitised)
};

template <class T, int E>
__device__ __forceinline__ void copy_vec(T (&dst)[E], const T (&src)[E]) {
#pragma unroll
  for (int e = 0; e < E; ++e) dst[e] = src[e];
}

template <class T> struct LeapfrogP {
  int kind;       // AHMC_INTEGRATOR_*
  T sqrt_alpha;   // TemperedLeapfrog: sqrt(α)
};

// temper(lf, r, (i, is_half), n_steps) (src/integrator.jl:198-209)
template <class T, int E>
__device__ __forceinline__ void temper(const LeapfrogP<T>& lf, T (&r)[E], int64_t i, bool is_half, int64_t n_steps) {
  if (lf.kind != 2) return;
  int64_t i_temper = 2 * (i - 1) + 1 + (is_half ? 0 : 1);
  if (i_temper <= n_steps) {
#pragma unroll
    for (int e = 0; e < E; ++e) r[e] = r[e] * lf.sqrt_alpha;
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) r[e] = r[e] / lf.sqrt_alpha;
  }
}

// kinetic partial: Σ_e M⁻¹ r² over this lane's elements (Unit: minv = 1)
template <class T, int E>
__device__ __forceinline__ T kinetic_partial(const T (&r)[E], const T (&minv)[E]) {
  T s = 0;
#pragma unroll
  for (int e = 0; e < E; ++e) s += (r[e] * r[e]) * minv[e];
  return s;
}

// The two updates of a leapfrog, each ONE definition with its contraction spelled out (src/integrator.jl:233-243):
//   kick   r − (ϵ/2)·g        one fma: the product is not rounded
//   drift  θ + ϵ·(M⁻¹·r)      M⁻¹·r rounded, then one fma
// Every leapfrog_step* below and hier_publish_next go through them: what -ffp-contract=on does with `a - b * c` written out in several
// places is the compiler's choice per place, and hier_publish_next must produce the very bits the next step's own lane 0 will.
template <class T>
__device__ __forceinline__ T leapfrog_kick(T r, T eh, T g) { return fma(-eh, g, r); }
template <class T>
__device__ __forceinline__ T leapfrog_drift(T th, T eps, T minv, T r) { return fma(eps, minv * r, th); }

// Multi-wave hierarchical target: the chain's first lane publishes θ′[0], θ′[1] of the leapfrog that would FOLLOW this one from the point
// just completed with the same signed step — leapfrog_kick, then leapfrog_drift, the functions the next leapfrog_step calls, so the bits
// are the ones its own lane 0 will compute (tests/test_device_primitives.py: test_hier_publish_next_is_the_leapfrog_own_expression) —
// into xwave_buf_p, before the barrier of the energy exchange.
template <class T, int G, int E, int TK>
__device__ __forceinline__ void hier_publish_next(const Point<T, E>& z, const T (&minv)[E], T eps) {
  if constexpr (G > 64 && TK == 3 && E >= 2) {
    if (threadIdx.x == 0) {
      const T eh = eps / 2;
      double* hp = xwave_buf_p();
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const T rh = leapfrog_kick(z.r[k], eh, z.g[k]);
        const T tn = leapfrog_drift(z.th[k], eps, minv[k], rh);
        hp[k] = (double)tn;
      }
    }
  }
}

// One leapfrog step of step i of n (tempering indices) with signed step size eps:
//   r -= ϵ/2 g ; θ += ϵ M⁻¹ r ; (ℓπ, g) = ∂H∂θ(θ) ; r -= ϵ/2 g ; ℓκ = -½ rᵀM⁻¹r ; sanitise
// TEMPER = false compiles the tempering out (the default NUTS kernels: the if-converted r·√α / r/√α
// select costs 6 VALU per leaf even when unused; TemperedLeapfrog runs the general instantiation)
template <class T, int G, int E, int TK, bool TEMPER = true>
__device__ __forceinline__ void leapfrog_step(Point<T, E>& z, const T (&minv)[E], T eps, const TargetP<T>& tp,
                                              const LeapfrogP<T>& lf, int lane, int d0, int64_t i, int64_t n, bool use_pre = false) {
  if constexpr (TEMPER) temper(lf, z.r, i, true, n);
  const T eh = eps / 2;
#pragma unroll
  for (int e = 0; e < E; ++e) z.r[e] = leapfrog_kick(z.r[e], eh, z.g[e]);
#pragma unroll
  for (int e = 0; e < E; ++e) z.th[e] = leapfrog_drift(z.th[e], eps, minv[e], z.r[e]);
  T red[2];
  red[0] = target_eval<T, G, E, TK>(tp, z.th, z.g, lane, d0, !TEMPER && use_pre);
#pragma unroll
  for (int e = 0; e < E; ++e) z.r[e] = leapfrog_kick(z.r[e], eh, z.g[e]);
  if constexpr (TEMPER) temper(lf, z.r, i, false, n);
  red[1] = kinetic_partial(z.r, minv);
  if constexpr (!TEMPER) hier_publish_next<T, G, E, TK>(z, minv, eps);
  leapfrog_allsum<G, TK>(red);
  z.lp = sanitize(red[0]);
  z.lk = sanitize(-red[1] / 2);
}

// The leaf of a NUTS tree needs ONE number from the new point: neg_energy(z′) = ℓπ + ℓκ (src/trajectory.jl:641-643) —
// the weight, the divergence test and ΔH all derive from it; ℓπ and ℓκ themselves are not read again until the
// candidate's caches are rebuilt at the end of the transition.  So the lane partials are combined BEFORE the all-reduce
// (one value, 22 VALU, instead of the pair's 34 incl. its selects) and the PhasePoint sanitation (non-finite ℓπ or ℓκ →
// −Inf, src/hamiltonian.jl:95-104) is applied to the sum: sanitize(ℓπ) + sanitize(ℓκ) is −Inf exactly when either is
// non-finite, and then ℓπ + ℓκ is non-finite too (the one exception, two finite values of ≈1e308 that overflow when
// added, does not occur for a log-density).  Returns neg_energy; z.lp / z.lk are NOT updated.
// (TWIN: leapfrog_step_ne_partial below repeats the vector work of this function for the pair step and the quad step of k_nuts — change both)
template <class T, int G, int E, int TK>
__device__ __forceinline__ T leapfrog_step_ne(Point<T, E>& z, const T (&minv)[E], T eps, const TargetP<T>& tp, int lane, int d0) {
  const T eh = eps / 2;
#pragma unroll
  for (int e = 0; e < E; ++e) z.r[e] = leapfrog_kick(z.r[e], eh, z.g[e]);
#pragma unroll
  for (int e = 0; e < E; ++e) z.th[e] = leapfrog_drift(z.th[e], eps, minv[e], z.r[e]);
  const T part = target_eval<T, G, E, TK>(tp, z.th, z.g, lane, d0);
#pragma unroll
  for (int e = 0; e < E; ++e) z.r[e] = leapfrog_kick(z.r[e], eh, z.g[e]);
  const T kin = kinetic_partial(z.r, minv);
  T sv[1] = {part - kin / 2};
  leapfrog_allsum<G, TK>(sv);
  const T s = sv[0];
  return is_finite(s) ? s : -Lim<T>::inf();
}

// The vector work of leapfrog_step_ne alone (the same expressions): returns this lane's partial of ℓπ − ½ rᵀM⁻¹r, NOT reduced (the pair step of k_nuts
// carries two leaves' partials through one reduction, the quad step four).
// TWIN of leapfrog_step_ne above, line for line up to the reduction: change both.  (Two texts on purpose: with leapfrog_step_ne written as a call of this one AND
// the leaf's scalar work of k_nuts in a shared lambda, the single-leaf loop no longer compiled to the device code it had before — 760 kernels differed; the
// two rewrites were not tried one by one.  tests/test_leaf_pairs.py holds the twins together.)
template <class T, int G, int E, int TK>
__device__ __forceinline__ T leapfrog_step_ne_partial(Point<T, E>& z, const T (&minv)[E], T eps, const TargetP<T>& tp, int lane, int d0) {
  const T eh = eps / 2;
#pragma unroll
  for (int e = 0; e < E; ++e) z.r[e] = leapfrog_kick(z.r[e], eh, z.g[e]);
#pragma unroll
  for (int e = 0; e < E; ++e) z.th[e] = leapfrog_drift(z.th[e], eps, minv[e], z.r[e]);
  const T part = target_eval<T, G, E, TK>(tp, z.th, z.g, lane, d0);
#pragma unroll
  for (int e = 0; e < E; ++e) z.r[e] = leapfrog_kick(z.r[e], eh, z.g[e]);
  const T kin = kinetic_partial(z.r, minv);
  return part - kin / 2;
}
template <class T>
__device__ __forceinline__ T neg_energy_sanitized(T s) { return is_finite(s) ? s : -Lim<T>::inf(); }

// v_readlane of a float / double: the value of lane L as a wave-uniform (scalar) one
template <int L> __device__ __forceinline__ float readlane_t(float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), L)); }
template <int L> __device__ __forceinline__ double readlane_t(double v) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), L), __builtin_amdgcn_readlane(__double2loint(v), L));
}

// The order-independent scalar work of the TWO leaves of a pair step of k_nuts, once, with lane parity picking
// the leaf — in the single-leaf arm of k_nuts it runs once per leaf in all 64 lanes on a wave-uniform value.
// z is wave64_pair_reduce_t's transposed register.  One quad_perm [2,3,2,3] gives EVERY lane an energy (even lanes Σea, odd lanes
// Σeb): lanes 0 / 1 of a quad hold dot-product sums, which may be ±Inf or NaN, and (int)dk of the weight's exp on those is undefined
// behaviour.  Quads 0 and 2 then hold the energies in another rounding (wave64_pair_reduce); nothing reads them.  Lanes 4Q + 2 / 4Q + 3
// (6 / 7) take leaf a's / leaf b's value through the expressions of the single-leaf arm's scalar block, in its order, and v_readlane and the compares' lane
// masks hand the results back as scalars.  No exec-masked region.  What depends on the ORDER of the two leaves (the running sums, maxabs,
// redo / numerical / sub_term, the branch that drops leaf b) stays with the caller.
// TWIN of the single-leaf arm's scalar block in k_nuts (ahmc_nuts.hpp, from `pos_cur += v;` to the running statistics): a change to a
// leaf's scalar work is made in both, and in quad_leaf_stats below, the TWIN for four leaves (tests/device_probe/pair_stats.hip repeats those lines as its
// serial reference; tests/device_probe/quad_red.hip holds quad_leaf_stats to this function).
template <class T> struct PairLeafStats {
  T w[2], sa[2], dH[2];     // leaf weight (LINW: W, else ℓw), α = min(1, W), ΔH
  bool redo[2], div[2];     // ℓw above the linear domain's limit; the divergence test !(−H0 < Δ_max + ne)
};
template <class T, bool LINW, int Q = AHMC_PAIR_RED_QUAD>
__device__ __forceinline__ void pair_leaf_stats(T z, T H0, T delta_max, T lw_limit, PairLeafStats<T>& o) {
  static_assert(Q >= 0 && Q <= 3, "a row has four quads");
  constexpr int LA = 4 * Q + 2, LB = 4 * Q + 3;
  const bool odd = (threadIdx.x & 1u) != 0;
  const T ne = neg_energy_sanitized(dpp_mov<0xEE>(z));  // quad_perm [2,3,2,3]
  const T dH = -ne - H0;
  const T lw = H0 + ne;
  T w, sa;
  if constexpr (LINW) {
    w = leaf_weight_exp_pair<LA, LB>(lw, odd);
    sa = w >= T(1) ? T(1) : w;
  } else {
    const T wa = leaf_weight_exp_pair<LA, LB>(lw > T(0) ? T(0) : lw, odd);  // alpha_from_logweight
    sa = wa >= T(1) ? T(1) : wa;
    w = lw;
  }
  const unsigned long long m_redo = __builtin_amdgcn_ballot_w64(lw > lw_limit);
  const unsigned long long m_div = __builtin_amdgcn_ballot_w64(!(-H0 < delta_max + ne));
  o.w[0] = readlane_t<LA>(w);
  o.w[1] = readlane_t<LB>(w);
  o.sa[0] = readlane_t<LA>(sa);
  o.sa[1] = readlane_t<LB>(sa);
  o.dH[0] = readlane_t<LA>(dH);
  o.dH[1] = readlane_t<LB>(dH);
  o.redo[0] = LINW && ((m_redo >> LA) & 1ull) != 0ull;
  o.redo[1] = LINW && ((m_redo >> LB) & 1ull) != 0ull;
  o.div[0] = ((m_div >> LA) & 1ull) != 0ull;
  o.div[1] = ((m_div >> LB) & 1ull) != 0ull;
}

// The same for the FOUR leaves of a quad step of k_nuts: w is wave64_quad_reduce_t's register, leaf k in the lanes with lane & 3 == k.
// Quad 1 of a row of w (lanes 4 .. 7) holds the four energies, and those four lanes are the ONLY ones read: the weight's table indices by
// v_readlane of lanes 4 .. 7, w / sa / ΔH by v_readlane of lane 4 + k, the flags as bits 4 .. 7 of the compares' lane masks.  Quad 2 takes
// quad 1's energies by the one row_ror:4 (it held level-1 dot products).  Quads 0 and 3 do NOT hold energies: quad 3 keeps its own level-1
// dot-product sums and quad 0 receives them, so those eight lanes run the pass on H0 + Σd.  ±Inf and NaN there are sanitised to −Inf like an
// energy; a large FINITE sum (behind a divergent leaf, where the leapfrogs are speculative) takes such a lane's float-to-int conversion in
// the weight's exp out of range.  That is the lane's own business — its k feeds only its own ldexp, v_cvt_i32_f64 saturates and does not trap,
// nothing of lanes 0 .. 3 and 12 .. 15 is ever read — which is why the pass does not spend the two further rotations that would hand them
// energies too (pair_leaf_stats gets an energy into every lane with the one quad_perm it needs anyway).  tests/device_probe/quad_red.hip
// puts ±1e300, ±Inf and NaN into those sums.
// TWIN of pair_leaf_stats above and of the single-leaf arm's scalar block in k_nuts: a change to a leaf's scalar work is made in all three
// (tests/device_probe/quad_red.hip holds this one to pair_leaf_stats run twice).
// The results stay in their lanes: leaf k's weight, α and ΔH are read (v_readlane of lane 4 + k) when the caller applies leaf k, not all
// twelve at once — 24 scalar registers fewer live across the apply sequence, where the kernel's scalar registers are short — and the flags
// are bits 4 + k of the two compares' lane masks.
__device__ __forceinline__ float readlane_at(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ double readlane_at(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
template <class T> struct QuadLeafStats {
  static constexpr int L0 = 4;
  T w_l, sa_l, dH_l;                   // per lane: leaf (lane & 3)'s weight (LINW: W, else ℓw), α = min(1, W), ΔH
  unsigned long long m_redo, m_div;    // lane masks: ℓw above the linear domain's limit; the divergence test !(−H0 < Δ_max + ne)
  __device__ __forceinline__ T w(int k) const { return readlane_at(w_l, L0 + k); }
  __device__ __forceinline__ T sa(int k) const { return readlane_at(sa_l, L0 + k); }
  __device__ __forceinline__ T dH(int k) const { return readlane_at(dH_l, L0 + k); }
  __device__ __forceinline__ bool redo(int k) const { return ((m_redo >> (L0 + k)) & 1ull) != 0ull; }
  __device__ __forceinline__ bool div(int k) const { return ((m_div >> (L0 + k)) & 1ull) != 0ull; }
};
template <class T, bool LINW>
__device__ __forceinline__ void quad_leaf_stats(T wz, T H0, T delta_max, T lw_limit, QuadLeafStats<T>& o) {
  constexpr int L0 = QuadLeafStats<T>::L0;
  const bool odd = (threadIdx.x & 1u) != 0, up = (threadIdx.x & 2u) != 0, oq = (threadIdx.x & 4u) != 0;
  const T from_prev = dpp_mov<0x124>(wz);  // row_ror:4
  const T ne = neg_energy_sanitized(oq ? wz : from_prev);
  const T dH = -ne - H0;
  const T lw = H0 + ne;
  T w, sa;
  if constexpr (LINW) {
    w = leaf_weight_exp_quad<L0>(lw, odd, up);
    sa = w >= T(1) ? T(1) : w;
  } else {
    const T wa = leaf_weight_exp_quad<L0>(lw > T(0) ? T(0) : lw, odd, up);  // alpha_from_logweight
    sa = wa >= T(1) ? T(1) : wa;
    w = lw;
  }
  o.m_redo = LINW ? __builtin_amdgcn_ballot_w64(lw > lw_limit) : 0ull;
  o.m_div = __builtin_amdgcn_ballot_w64(!(-H0 < delta_max + ne));
  o.w_l = w;
  o.sa_l = sa;
  o.dH_l = dH;
}

// The same for the EIGHT leaves of an octo step of k_nuts: w is wave64_oct_reduce_t's register — row 0 holds the first half's slots and row 1
// the second half's, each laid out as wave64_quad_reduce_t's row, so leaf k < 4 is read in lane 4 + k and leaf k >= 4 in lane 16 + k (quad 1
// of its row).  ONE pass: one row_ror:4, one exp chain, eight table indices by v_readlane and eight scalar table loads issued together.  What
// quad_leaf_stats says about the lanes that do not hold energies holds here row by row (quads 0 and 3 run the pass on H0 + Σd; nothing of
// them is read).
// TWIN of quad_leaf_stats and pair_leaf_stats above and of the single-leaf arm's scalar block in k_nuts: a change to a leaf's scalar work is
// made in all four (tests/device_probe/oct_red.hip holds this one to quad_leaf_stats run on each half).
template <class T> struct OctLeafStats {
  static constexpr int L0 = 4, L1 = 20;
  T w_l, sa_l, dH_l;                   // per lane: the row's leaf (lane & 3)'s weight (LINW: W, else ℓw), α = min(1, W), ΔH
  // the two compares' lane masks — the divergence test !(−H0 < Δ_max + ne); ℓw above the linear domain's limit — cut to the eight lanes that
  // are read and packed into ONE 32-bit scalar (divergence: bit lane_of(k); redo: bit lane_of(k) + 8, the lanes of quad 3, which hold no
  // energy): five scalar registers fewer live across the apply sequence, where the draws kernel is short of them
  unsigned m_flags;
  static constexpr unsigned LANES = (0xFu << L0) | (0xFu << L1);
  static __device__ __forceinline__ int lane_of(int k) { return k < 4 ? L0 + k : L1 + (k - 4); }
  __device__ __forceinline__ T w(int k) const { return readlane_at(w_l, lane_of(k)); }
  __device__ __forceinline__ T sa(int k) const { return readlane_at(sa_l, lane_of(k)); }
  __device__ __forceinline__ T dH(int k) const { return readlane_at(dH_l, lane_of(k)); }
  __device__ __forceinline__ bool redo(int k) const { return ((m_flags >> (lane_of(k) + 8)) & 1u) != 0u; }
  __device__ __forceinline__ bool div(int k) const { return ((m_flags >> lane_of(k)) & 1u) != 0u; }
};
template <class T, bool LINW>
__device__ __forceinline__ void oct_leaf_stats(T wz, T H0, T delta_max, T lw_limit, OctLeafStats<T>& o) {
  constexpr int L0 = OctLeafStats<T>::L0, L1 = OctLeafStats<T>::L1;
  const bool odd = (threadIdx.x & 1u) != 0, up = (threadIdx.x & 2u) != 0, oq = (threadIdx.x & 4u) != 0;
  const T from_prev = dpp_mov<0x124>(wz);  // row_ror:4
  const T ne = neg_energy_sanitized(oq ? wz : from_prev);
  const T dH = -ne - H0;
  const T lw = H0 + ne;
  T w, sa;
  if constexpr (LINW) {
    w = leaf_weight_exp_oct<L0, L1>(lw, odd, up);
    sa = w >= T(1) ? T(1) : w;
  } else {
    const T wa = leaf_weight_exp_oct<L0, L1>(lw > T(0) ? T(0) : lw, odd, up);  // alpha_from_logweight
    sa = wa >= T(1) ? T(1) : wa;
    w = lw;
  }
  const unsigned m_redo = LINW ? (unsigned)__builtin_amdgcn_ballot_w64(lw > lw_limit) : 0u;
  const unsigned m_div = (unsigned)__builtin_amdgcn_ballot_w64(!(-H0 < delta_max + ne));
  o.m_flags = (m_div & OctLeafStats<T>::LANES) | ((m_redo & OctLeafStats<T>::LANES) << 8);
  o.w_l = w;
  o.sa_l = sa;
  o.dH_l = dH;
}

// leapfrog_step (untempered) that sums two more caller-supplied partials of the UPDATED point in the same all-reduce
// as ℓπ and the kinetic energy: the NUTS kernels pass the two U-turn dot products of the merge that follows the
// leaf, which saves one of the two reductions of such a leaf (15 of 60 VALU; a barrier pair in the multi-wave groups).
// Every value takes exactly the additions it would take in a reduction of its own, so the bits do not change.
template <class T, int G, int E, int TK, class F>
__device__ __forceinline__ void leapfrog_step_plus2(Point<T, E>& z, const T (&minv)[E], T eps, const TargetP<T>& tp, int lane, int d0,
                                                    T (&extra)[2], F&& partials, bool use_pre = false) {
  const T eh = eps / 2;
#pragma unroll
  for (int e = 0; e < E; ++e) z.r[e] = leapfrog_kick(z.r[e], eh, z.g[e]);
#pragma unroll
  for (int e = 0; e < E; ++e) z.th[e] = leapfrog_drift(z.th[e], eps, minv[e], z.r[e]);
  T red[4];
  red[0] = target_eval<T, G, E, TK>(tp, z.th, z.g, lane, d0, use_pre);
#pragma unroll
  for (int e = 0; e < E; ++e) z.r[e] = leapfrog_kick(z.r[e], eh, z.g[e]);
  red[1] = kinetic_partial(z.r, minv);
  partials(red[2], red[3]);
  hier_publish_next<T, G, E, TK>(z, minv, eps);
  leapfrog_allsum<G, TK>(red);
  z.lp = sanitize(red[0]);
  z.lk = sanitize(-red[1] / 2);
  extra[0] = red[2];
  extra[1] = red[3];
}

// phasepoint(h, θ, r): fill the caches at the current (θ, r) (src/hamiltonian.jl:115-119)
template <class T, int G, int E, int TK>
__device__ __forceinline__ void fill_caches(Point<T, E>& z, const T (&minv)[E], const TargetP<T>& tp, int lane, int d0) {
  T red[2];
  red[0] = target_eval<T, G, E, TK>(tp, z.th, z.g, lane, d0);
  red[1] = kinetic_partial(z.r, minv);
  leapfrog_allsum<G, TK>(red);
  z.lp = sanitize(red[0]);
  z.lk = sanitize(-red[1] / 2);
}

// vector load/store of one chain's slice: element d0+e of chain c lives at base[off + d0 + e].
// Full, 16-byte aligned lanes use dwordx4/dwordx2 accesses (CH elements per access).
// SB (k_nuts where a chain owns a wave, its TSC): `base + off` is wave-uniform — formed in 64 bits on the scalar unit — and the
// lane adds only its BYTE offset d0·sizeof(T), a 32-bit value: the accesses take the scalar-base form (saddr + voffset) with no 64-bit
// per-lane address arithmetic.  d0·sizeof(T) is a multiple of the 16-byte piece (E is a multiple of CH), so the alignment test is the
// scalar base's.  Same elements, same addresses, same predicate as the per-lane form.
template <class T, int E, bool SB = false>
__device__ __forceinline__ void load_vec(T (&v)[E], const T* __restrict__ base, int64_t off, int d0, int D, T pad) {
  constexpr int CH = (E * sizeof(T) >= 16) ? (int)(16 / sizeof(T)) : E;
  if constexpr (SB) {
    const T* sb = base + off;
    if (CH > 1 && d0 + E <= D && (reinterpret_cast<uintptr_t>(sb) % (CH * sizeof(T)) == 0)) {
      using V = T __attribute__((ext_vector_type(CH)));
      // (the lane's byte offset is made opaque IN the arm that uses it, each arm its own: formed in front of the branch — or once per
      // transition — the instruction selector sees a 64-bit register in the arm, not zext(32-bit), and adds it with a vector instruction)
      unsigned bv = (unsigned)d0 * (unsigned)sizeof(T);
      asm("; full lane" : "+v"(bv));
      const T* ptr = reinterpret_cast<const T*>(reinterpret_cast<const char*>(sb) + bv);
#pragma unroll
      for (int e = 0; e < E; e += CH) {
        V t = *reinterpret_cast<const V*>(ptr + e);
#pragma unroll
        for (int k = 0; k < CH; ++k) v[e + k] = t[k];
      }
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e) {   // (every element is an arm of its own)
        v[e] = pad;
        if (d0 + e < D) {
          unsigned be = (unsigned)d0 * (unsigned)sizeof(T);
          asm("; ragged lane" : "+v"(be));
          v[e] = *reinterpret_cast<const T*>(reinterpret_cast<const char*>(sb + e) + be);
        }
      }
    }
    return;
  }
  const T* ptr = base + off + d0;
  if (CH > 1 && d0 + E <= D && (reinterpret_cast<uintptr_t>(ptr) % (CH * sizeof(T)) == 0)) {
    using V = T __attribute__((ext_vector_type(CH)));
#pragma unroll
    for (int e = 0; e < E; e += CH) {
      V t = *reinterpret_cast<const V*>(ptr + e);
#pragma unroll
      for (int k = 0; k < CH; ++k) v[e + k] = t[k];
    }
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = (d0 + e < D) ? ptr[e] : pad;
  }
}
template <class T, int E, bool SB = false>
__device__ __forceinline__ void store_vec(const T (&v)[E], T* __restrict__ base, int64_t off, int d0, int D) {
  constexpr int CH = (E * sizeof(T) >= 16) ? (int)(16 / sizeof(T)) : E;
  if constexpr (SB) {
    T* sb = base + off;
    if (CH > 1 && d0 + E <= D && (reinterpret_cast<uintptr_t>(sb) % (CH * sizeof(T)) == 0)) {
      using V = T __attribute__((ext_vector_type(CH)));
      unsigned bv = (unsigned)d0 * (unsigned)sizeof(T);   // (as in load_vec)
      asm("; full lane" : "+v"(bv));
      T* ptr = reinterpret_cast<T*>(reinterpret_cast<char*>(sb) + bv);
#pragma unroll
      for (int e = 0; e < E; e += CH) {
        V t;
#pragma unroll
        for (int k = 0; k < CH; ++k) t[k] = v[e + k];
        *reinterpret_cast<V*>(ptr + e) = t;
      }
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (d0 + e < D) {
          unsigned be = (unsigned)d0 * (unsigned)sizeof(T);
          asm("; ragged lane" : "+v"(be));
          *reinterpret_cast<T*>(reinterpret_cast<char*>(sb + e) + be) = v[e];
        }
    }
    return;
  }
  T* ptr = base + off + d0;
  if (CH > 1 && d0 + E <= D && (reinterpret_cast<uintptr_t>(ptr) % (CH * sizeof(T)) == 0)) {
    using V = T __attribute__((ext_vector_type(CH)));
#pragma unroll
    for (int e = 0; e < E; e += CH) {
      V t;
#pragma unroll
      for (int k = 0; k < CH; ++k) t[k] = v[e + k];
      *reinterpret_cast<V*>(ptr + e) = t;
    }
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (d0 + e < D) ptr[e] = v[e];
  }
}

}  // namespace ahmc
