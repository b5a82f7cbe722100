// ahmc_glm_yrep_draw.hpp — the outcome sampler of include/ahmc_glm_yrep.h: one y ~ p(y | the element's quantities) per call, as
// functions of (planes, aux, a block generator) with nothing else in them.  The contract is advancedhmc.jl_amd/glm.py: yrep_at, the host
// mirror; this text is its C++ form and compiles unchanged into k_glm_yrep (ahmc_glm_yrep.hpp) and into the stand-alone CPU program
// tests/host_ref/glm_yrep_driver.cpp, so it includes nothing of HIP and nothing of the engine.
//
// Randomness arrives through `Gen`: gen.next(u, u2) hands out the element's next 4-word block as two uniforms in (0, 1] — on the device
// Philox4x32-10 at counter (row, col, 0x59524550, slot) under the caller's seed (ahmc_glm_yrep.hpp: GlmYrepGen) — and counts the blocks
// taken.  All arithmetic is double and nothing is fused but the one fma the contract names; every loop has a constant bound:
// YREP_INVERSION_MAX steps of the inversion, YREP_MAX_ROUNDS rounds of a rejection loop, whose capped exit is NaN.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define AHMC_YREP_HD __host__ __device__ inline
#else
#define AHMC_YREP_HD inline
#endif
// nothing fused but the fma the contract names (a host compiler other than clang takes -ffp-contract=off)
#if defined(__clang__)
#define AHMC_YREP_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define AHMC_YREP_NO_CONTRACT
#endif

namespace ahmc {

constexpr int YREP_MAX_ROUNDS = 64;        // of PTRS and of Marsaglia–Tsang: P(capped exit) < 1e-40 for every shape
constexpr int YREP_INVERSION_MAX = 200;    // steps of the Poisson inversion (λ < 10: P(k > 200) = 0 in double)
constexpr double YREP_INVERSION_BELOW = 10.0;
constexpr uint32_t YREP_PURPOSE = 0x59524550u;

// the Box–Muller normal of a block: Rng::normal_pair's cosine branch
AHMC_YREP_HD double yrep_normal(double u, double u2) {
AHMC_YREP_NO_CONTRACT
  const double rad = sqrt(-2.0 * log(u));
  return rad * cos(6.283185307179586476925286766559 * u2);
}

// family 0: y = [u <= μ]
template <class Gen>
AHMC_YREP_HD double yrep_bernoulli(double mu, Gen& gen) {
  double u, u2;
  gen.next(u, u2);
  if (!isfinite(mu)) return NAN;
  return u <= mu ? 1.0 : 0.0;
}

// families 2, 3: y = fma(√v, z, μ)
template <class Gen>
AHMC_YREP_HD double yrep_gaussian(double mu, double v, Gen& gen) {
  double u, u2;
  gen.next(u, u2);
  if (!isfinite(mu) || !isfinite(v)) return NAN;
  return fma(sqrt(v), yrep_normal(u, u2), mu);
}

// families 5, 6: inversion over p(0) … p(C − 1); F ascending from +0, every add rounded on its own; y = #{c <= C − 2 : u > F_c}
template <class Planes, class Gen>
AHMC_YREP_HD double yrep_category(const Planes& p, int C, Gen& gen) {
AHMC_YREP_NO_CONTRACT
  double u, u2;
  gen.next(u, u2);
  double F = 0.0;
  int y = 0;
  bool fin = true;
  for (int c = 0; c < C; ++c) {
    const double pc = p(c);
    fin = fin && isfinite(pc);
    if (c < C - 1) {
      F = F + pc;
      y += u > F ? 1 : 0;
    }
  }
  return fin ? (double)y : NAN;
}

// family 1, and the last step of family 4: y ~ Poisson(λ).  λ < 10: inversion with one u.  Otherwise Hörmann's PTRS (Insurance:
// Mathematics and Economics 12 (1993)), one block per round.
template <class Gen>
AHMC_YREP_HD double yrep_poisson(double lam, Gen& gen) {
AHMC_YREP_NO_CONTRACT
  if (!isfinite(lam) || lam < 0.0) return NAN;
  double u, u2;
  if (lam < YREP_INVERSION_BELOW) {
    gen.next(u, u2);
    double p = exp(-lam), F = p;
    int k = 0;
    while (u > F && k < YREP_INVERSION_MAX) {
      k += 1;
      p = p * lam / (double)k;
      F = F + p;
    }
    return (double)k;
  }
  const double b = 0.931 + 2.53 * sqrt(lam);
  const double a = -0.059 + 0.02483 * b;
  const double inv_alpha = 1.1239 + 1.1328 / (b - 3.4);
  const double vr = 0.9277 - 3.6224 / (b - 2.0);
  const double log_lam = log(lam);
  for (int round = 0; round < YREP_MAX_ROUNDS; ++round) {
    gen.next(u, u2);
    const double U = u - 0.5, V = u2;
    const double us = 0.5 - fabs(U);
    const double k = floor((2.0 * a / us + b) * U + lam + 0.43);
    if (us >= 0.07 && V <= vr) return k;
    if (k < 0.0 || (us < 0.013 && V > us)) continue;
    const double lhs = log(V) + log(inv_alpha) - log(a / (us * us) + b);
    const double rhs = -lam + k * log_lam - lgamma(k + 1.0);
    if (lhs <= rhs) return k;
  }
  return NAN;
}

// family 4: g ~ Gamma(φ, 1) by Marsaglia–Tsang (φ < 1: shape φ + 1 and the boost u^{1/φ}, from a block of its own, taken first), then
// y ~ Poisson(g·μ/φ) with the slots running on
template <class Gen>
AHMC_YREP_HD double yrep_negbinomial(double mu, double s, Gen& gen) {
AHMC_YREP_NO_CONTRACT
  const double phi = exp(s);
  if (!isfinite(mu) || !isfinite(phi) || !(phi > 0.0) || mu < 0.0) return NAN;
  double u, u2, boost = 1.0, shape = phi;
  if (phi < 1.0) {
    gen.next(u, u2);
    boost = pow(u, 1.0 / phi);
    shape = phi + 1.0;
  }
  const double d = shape - 1.0 / 3.0;
  const double c = 1.0 / sqrt(9.0 * d);
  double g = NAN;
  for (int round = 0; round < YREP_MAX_ROUNDS; ++round) {
    gen.next(u, u2);
    const double z = yrep_normal(u, u2);
    gen.next(u, u2);
    const double w = 1.0 + c * z;
    const double t = w * w * w;
    if (t <= 0.0) continue;
    if (log(u) < 0.5 * z * z + d - d * t + d * log(t)) {
      g = d * t;
      break;
    }
  }
  if (!(g == g)) return NAN;
  return yrep_poisson(g * boost * mu / phi, gen);
}

// FAM: 0 Bernoulli (μ); 1 Poisson (μ); 2 the Gaussians (μ, v); 4 negative binomial (μ; aux = log φ); 5 the C probabilities of an
// ordered or a categorical model.  p(c): plane c of the element, in double.
template <int FAM, class Planes, class Gen>
AHMC_YREP_HD double yrep_draw(const Planes& p, double aux, int C, Gen& gen) {
  if constexpr (FAM == 0) return yrep_bernoulli(p(0), gen);
  else if constexpr (FAM == 1) return yrep_poisson(p(0), gen);
  else if constexpr (FAM == 2) return yrep_gaussian(p(0), p(1), gen);
  else if constexpr (FAM == 4) return yrep_negbinomial(p(0), aux, gen);
  else return yrep_category(p, C, gen);
}

// families 3 and 6 share the samplers of 2 and 5; −1: no such family
AHMC_YREP_HD int yrep_sampler_of(int family) { return family == 3 ? 2 : family == 6 ? 5 : (family >= 0 && family <= 5) ? family : -1; }
// the planes an element has: μ; (μ, v); or the C probabilities
AHMC_YREP_HD int yrep_planes_of(int family, int C) { return family == 2 || family == 3 ? 2 : family >= 5 ? C : 1; }

// what ahmc_glm_yrep_at refuses, in the header's order: 1 an unknown family; 2 n_categories outside 2 … 16 for families 5 and 6; 3 a NULL
// array where something would be read or written; 4 n < 0; 0: nothing
AHMC_YREP_HD int yrep_at_refusal(int family, int C, int64_t n, bool has_q, bool has_aux, bool has_y) {
  if (yrep_sampler_of(family) < 0) return 1;
  if (family >= 5 && (C < 2 || C > 16)) return 2;
  if (n > 0 && (!has_q || !has_y || (family == 4 && !has_aux))) return 3;
  if (n < 0) return 4;
  return 0;
}

}  // namespace ahmc
