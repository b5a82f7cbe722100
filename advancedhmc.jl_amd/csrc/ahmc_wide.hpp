// ahmc_wide.hpp — the built-in log-density families of a WIDE context (D > 4096, or AHMC_FORCE_WIDE=1): contexts that no
// fused-kernel geometry (G, E) covers and that the step-synchronous engine (ahmc_dense.hpp) serves end to end.
//
// k_w_target<T, TK>: (ℓπ, g = −∇ℓπ) at θ of the LISTED chains, one workgroup of WT_THREADS threads per chain striding over a
// run-time D.  Every family fits in one pass over θ: the per-element arithmetic is target_eval's (ahmc_device.hpp) — same
// formulas, same constants —, and the elements that depend on a reduction over the whole chain (funnel: g[0] after Σθ²;
// hierarchical: g[0], g[1] after Σ(x−μ), Σ(x−μ)²) are written by thread 0 once the reduction is done.
//
// Reduction order.  A chain's bits must not depend on which or how many chains are listed, on whether θ′ sits in a pool point
// or in the context's (D, N) array, or on the chain's column (an engine over a block of chains holds chain c at another
// column).  So the elements are cut into VIRTUAL vectors of 16 bytes counted from d = 0 — not from an aligned address —,
// thread t takes vectors t, t + WT_THREADS, … in that order and its elements in ascending d, the D mod VW left-over elements
// go to threads 0 … in ascending d after that, and the threads' partials meet in block_allsum2's fixed order.  Where θ and g
// are 16-byte aligned (D·sizeof(T) a multiple of 16: every column and every pool point) a virtual vector is one 16-byte load
// / store; elsewhere the same vector is moved element by element — same arithmetic in the same order.
#pragma once

#include "ahmc_dense.hpp"

namespace ahmc {

constexpr int WT_THREADS = 256;
constexpr int WT_UNROLL = 4;  // virtual vectors a thread has in flight: all loads of a chunk are issued before the first use

// X / Y: θ′ in, g′ out.  Chain c's column is at X + c·cs + ptidx[c]·ps (the addressing of dn_gemm's pool operands; ptidx null,
// cs = D: the plain (D, N) array).  params: the family's parameters (diagonal Gaussian: m[D], s[D], shared by all chains).
template <class T, int TK>
__global__ __launch_bounds__(WT_THREADS) void k_w_target(const T* __restrict__ params, const T* __restrict__ X, T* __restrict__ Y, T* __restrict__ lp,
                                                         int D, int64_t n, const int* __restrict__ list, const int* __restrict__ ptidx, int64_t ps,
                                                         int64_t cs) {
  static_assert(TK >= 0 && TK <= 3, "k_w_target: the built-in families are AHMC_TARGET_* 0..3");
  constexpr int VW = 16 / (int)sizeof(T);
  typedef T V __attribute__((ext_vector_type(VW)));
  const int64_t j = blockIdx.x;
  if (j >= n) return;  // (uniform over the workgroup)
  const int64_t c = list ? (int64_t)list[j] : j;
  const int64_t off = c * cs + (ptidx ? (int64_t)ptidx[c] * ps : 0);
  const T* __restrict__ th = X + off;
  T* __restrict__ g = Y + off;
  const int t = threadIdx.x;
  const T log2pi = (T)AHMC_LOG2PI;
  // per-chain scalars the element pass needs: funnel y = θ[0], e^{−y}; hierarchical μ = θ[0], log τ = θ[1], τ⁻² = e^{−2 log τ}
  T y0 = 0, y1 = 0, ek = 0;
  if constexpr (TK == 2) { y0 = th[0]; ek = exp(-y0); }
  if constexpr (TK == 3) { y0 = th[0]; y1 = th[1]; ek = exp(-2 * y1); }
  T a0 = 0, a1 = 0;  // the thread's partial sums
  // one element: returns g[d] and adds the element's terms to (a0, a1).  m, s: the diagonal Gaussian's parameters at d.
  auto elem = [&](int d, T x, T m, T s) -> T {
    if constexpr (TK == 0) {  // iso Gaussian: Σθ², g = θ
      a0 += x * x;
      return x;
    } else if constexpr (TK == 1) {  // diagonal Gaussian: Σ −(log 2π + 2 log s + (m−θ)²/s²)/2, g = −(m−θ)/s²
      const T diff = m - x;
      const T s2 = s * s;
      a0 += -(log2pi + 2 * log(s) + diff * diff / s2) / 2;
      return -(diff / s2);
    } else if constexpr (TK == 2) {  // funnel: Σ_{d≥1} θ², g[d] = θ_d·e^{−y} (g[0] after the reduction)
      const bool ok = d >= 1;
      a0 += ok ? x * x : T(0);
      return ok ? x * ek : T(0);
    } else {  // hierarchical: Σ_{d≥2} (x−μ), Σ_{d≥2} (x−μ)², g[d] = (x−μ)·τ⁻² (g[0], g[1] after the reduction)
      const bool ok = d >= 2;
      const T df = x - y0;
      a0 += ok ? df : T(0);
      a1 += ok ? df * df : T(0);
      return ok ? df * ek : T(0);
    }
  };
  const int nvec = D / VW;
  const bool vec_ok = ((reinterpret_cast<uintptr_t>(th) | reinterpret_cast<uintptr_t>(g)) & 15) == 0;
  const T* __restrict__ pm = TK == 1 ? params : nullptr;
  const T* __restrict__ psd = TK == 1 ? params + D : nullptr;
  const bool pvec_ok = TK == 1 && ((reinterpret_cast<uintptr_t>(pm) | reinterpret_cast<uintptr_t>(psd)) & 15) == 0;
  for (int k0 = t; k0 < nvec; k0 += WT_THREADS * WT_UNROLL) {
    V xv[WT_UNROLL], mv[WT_UNROLL], sv[WT_UNROLL];
#pragma unroll
    for (int u = 0; u < WT_UNROLL; ++u) {
      const int k = k0 + u * WT_THREADS;
      if (k < nvec) {
        if (vec_ok) xv[u] = *reinterpret_cast<const V*>(th + (int64_t)k * VW);
        else {
#pragma unroll
          for (int e = 0; e < VW; ++e) xv[u][e] = th[(int64_t)k * VW + e];
        }
        if constexpr (TK == 1) {
          if (pvec_ok) {
            mv[u] = *reinterpret_cast<const V*>(pm + (int64_t)k * VW);
            sv[u] = *reinterpret_cast<const V*>(psd + (int64_t)k * VW);
          } else {
#pragma unroll
            for (int e = 0; e < VW; ++e) { mv[u][e] = pm[(int64_t)k * VW + e]; sv[u][e] = psd[(int64_t)k * VW + e]; }
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < WT_UNROLL; ++u) {
      const int k = k0 + u * WT_THREADS;
      if (k < nvec) {
        V gv;
#pragma unroll
        for (int e = 0; e < VW; ++e) gv[e] = elem(k * VW + e, xv[u][e], TK == 1 ? mv[u][e] : T(0), TK == 1 ? sv[u][e] : T(0));
        if (vec_ok) *reinterpret_cast<V*>(g + (int64_t)k * VW) = gv;
        else {
#pragma unroll
          for (int e = 0; e < VW; ++e) g[(int64_t)k * VW + e] = gv[e];
        }
      }
    }
  }
  {  // the D mod VW elements after the last whole virtual vector
    const int d = nvec * VW + t;
    if (t < VW && d < D) g[d] = elem(d, th[d], TK == 1 ? pm[d] : T(0), TK == 1 ? psd[d] : T(0));
  }
  block_allsum2<WT_THREADS>(a0, a1);
  if (t != 0) return;
  T total;
  if constexpr (TK == 0) {
    total = -a0 / 2 - (T)D * log2pi / 2;
  } else if constexpr (TK == 1) {
    total = a0;
  } else if constexpr (TK == 2) {
    const T y = y0, ss = a0, nm1 = (T)(D - 1);
    total = -(log2pi + 2 * log(T(3)) + y * y / 9) / 2 - nm1 * (log2pi + y) / 2 - ss * ek / 2;
    g[0] = -(-y / 9 - nm1 / 2 + ss * ek / 2);
  } else {
    const T mu = y0, lt = y1, itau2 = ek, nn = (T)(D - 2);
    total = -(log2pi + mu * mu) / 2 - (log2pi + lt * lt) / 2 - nn * (log2pi + 2 * lt) / 2 - a1 * itau2 / 2;
    g[0] = -(-mu + a0 * itau2);
    g[1] = -(-lt - nn + a1 * itau2);
  }
  lp[c] = sanitize(total);  // (PhasePoint: a non-finite ℓπ → −Inf, src/hamiltonian.jl:95-104 — as k_u_sanitize)
}

}  // namespace ahmc
