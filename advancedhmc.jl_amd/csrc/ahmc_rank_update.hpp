// ahmc_rank_update.hpp — RankUpdateEuclideanMetric on the step-synchronous engine (include/ahmc_rank_update.h):
//   M⁻¹ = Diagonal(A) + B·Dm·Bᵀ, B (D, k), Dm (k, k), one metric for all chains.
//
// The engine treats a non-diagonal M⁻¹ as an opaque linear operator (ahmc_dense_host.hpp: dn_minv_apply, dn_momentum_map), so the
// two kernels here stand where dn_gemm(M⁻¹) / dn_gemm(U⁻¹) stand for the dense metric:
//   k_ru_apply     Y[:, c] = A∘X[:, c] + B·(Dm·(BᵀX[:, c]))               (∂H∂r, src/hamiltonian.jl:70-80)
//   k_ru_momentum  R[:, c] = U⁻¹·Q·[V⁻¹z[1:k]; z[k+1:D]],  Q = I − Y·T·Yᵀ  (rand_momentum, src/metric.jl:322-337)
// Each is a pass that reduces k dot products over the column, a k×k product in LDS, and a pass that writes the column.  The column
// is read by both passes and written once: the second read comes from the cache only while the CPW columns of the workgroup (and
// of every other resident workgroup) still fit in it — not measured; where it misses, the kernel moves 3 streams, not 2.
//
// B's traffic.  A workgroup serves CPW = RU_ACC / KB columns at once (KB: k rounded up to 4, 8, 16 or 32), so each B fragment a
// thread loads serves CPW chains: B costs 2·D·KB·sizeof(T) / CPW per chain and pass instead of 2·D·k·sizeof(T).
//
// Reduction order.  A chain's bits depend on (D, k) only — not on the list, N, the slot of the workgroup it lands in, or the
// addressing — as for k_w_target (ahmc_wide.hpp): the elements are cut into virtual 16-byte vectors counted from d = 0, thread t
// takes vectors t, t + RU_THREADS, … in order, the D mod VW left-over elements go to threads 0 … after that, and the partial sums
// meet in wave_allsum's and then the four waves' fixed order.
#pragma once

#include "ahmc_dense.hpp"

namespace ahmc {

constexpr int RU_THREADS = 256;
constexpr int RU_ACC = 32;  // partial sums per thread: CPW chains × KB columns of B
constexpr int RU_MAX_K = 32;

// the metric on the device (ahmc_dense_host.hpp: ru_set_metric); every array column-major
template <class T>
struct RUOp {
  const T* a;     // A (D)
  const T* isa;   // 1/√A (D)
  const T* B;     // (D, k)
  const T* Dm;    // (k, k)
  const T* Y;     // (D, k) Householder vectors of the QR of U⁻¹B (unit diagonal, zeros above it)
  const T* Tw;    // (k, k) the compact-WY factor: Q = I − Y·Tw·Yᵀ (upper triangular)
  const T* Vinv;  // (k, k) V⁻¹, V = chol(I + R·Dm·Rᵀ).U (upper triangular)
  int k;
};

// The element loop of both kernels: f(d0, nel, vec) for the virtual vectors of thread t in order (nel = VW elements from d0, loaded
// as one 16-byte vector where vec), then the D mod VW left-over elements one by one on threads 0 … VW−1 (nel = 1).
template <class T, class F>
__device__ __forceinline__ void ru_pass(int D, bool vec_ok, F&& f) {
  constexpr int VW = 16 / (int)sizeof(T);
  const int t = threadIdx.x;
  const int nvec = D / VW;
  for (int kv = t; kv < nvec; kv += RU_THREADS) f(kv * VW, VW, vec_ok);
  const int d = nvec * VW + t;
  if (t < VW && d < D) f(d, 1, false);
}

// the k sums of each of the CPW columns over the workgroup: acc → red (LDS, CPW·KB), fixed order
template <class T, int CPW, int KB>
__device__ __forceinline__ void ru_reduce(T (&acc)[CPW * KB], T* red_waves, T* red) {
  wave_allsum<64, T, CPW * KB>(acc);
  const int t = threadIdx.x, w = t >> 6;
  if ((t & 63) == 0) {
#pragma unroll
    for (int i = 0; i < CPW * KB; ++i) red_waves[w * CPW * KB + i] = acc[i];
  }
  __syncthreads();
  if (t < CPW * KB) {
    T s = 0;
#pragma unroll
    for (int q = 0; q < RU_THREADS / 64; ++q) s += red_waves[q * CPW * KB + t];
    red[t] = s;
  }
  __syncthreads();
}

// Y = M⁻¹X for the listed columns, dn_gemm's operand addressing: column c of X at X + c·xcs + ptidx[c]·xps (ptidx null: + 0), of Y at
// Y + c·ycs + ptidx[c]·yps.  One workgroup per CPW listed columns.
template <class T, int KB>
__global__ __launch_bounds__(RU_THREADS) void k_ru_apply(const RUOp<T> m, const T* __restrict__ X, T* __restrict__ Y, int D, int64_t n,
                                                         const int* __restrict__ list, const int* __restrict__ ptidx, int64_t xps, int64_t yps,
                                                         int64_t xcs, int64_t ycs) {
  constexpr int CPW = RU_ACC / KB;
  constexpr int VW = 16 / (int)sizeof(T);
  typedef T V __attribute__((ext_vector_type(VW)));
  __shared__ T red_waves[(RU_THREADS / 64) * CPW * KB];
  __shared__ T red[CPW * KB];
  __shared__ T us[CPW * KB];
  const int k = m.k;
  const int t = threadIdx.x;
  const T* xp[CPW];
  T* yp[CPW];
  bool live[CPW];
  bool vec_ok = ((reinterpret_cast<uintptr_t>(m.a) | reinterpret_cast<uintptr_t>(m.B)) & 15) == 0 && ((int64_t)D * (int64_t)sizeof(T)) % 16 == 0;
#pragma unroll
  for (int s = 0; s < CPW; ++s) {
    const int64_t j = (int64_t)blockIdx.x * CPW + s;
    live[s] = j < n;
    const int64_t jj = live[s] ? j : (int64_t)blockIdx.x * CPW;  // (a slot past the list reads slot 0's column and stores nothing)
    const int64_t c = list ? (int64_t)list[jj] : jj;
    xp[s] = X + c * xcs + (ptidx ? (int64_t)ptidx[c] * xps : 0);
    yp[s] = Y + c * ycs + (ptidx ? (int64_t)ptidx[c] * yps : 0);
    vec_ok = vec_ok && ((reinterpret_cast<uintptr_t>(xp[s]) | reinterpret_cast<uintptr_t>(yp[s])) & 15) == 0;
  }
  // pass 1: s_j = Σ_d B[d, j]·x[d]
  if (k > 0) {
    T acc[CPW * KB];
#pragma unroll
    for (int i = 0; i < CPW * KB; ++i) acc[i] = 0;
    auto body = [&](int d0, int nel, bool vec) {
      V xv[CPW];
#pragma unroll
      for (int s = 0; s < CPW; ++s) {
        if (vec) xv[s] = *reinterpret_cast<const V*>(xp[s] + d0);
        else {
#pragma unroll
          for (int e = 0; e < VW; ++e) xv[s][e] = e < nel ? xp[s][d0 + e] : T(0);
        }
      }
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        if (j < k) {
          V bv;
          const T* bp = m.B + (int64_t)j * D + d0;
          if (vec) bv = *reinterpret_cast<const V*>(bp);
          else {
#pragma unroll
            for (int e = 0; e < VW; ++e) bv[e] = e < nel ? bp[e] : T(0);
          }
#pragma unroll
          for (int e = 0; e < VW; ++e)
            if (e < nel) {
#pragma unroll
              for (int s = 0; s < CPW; ++s) acc[s * KB + j] += bv[e] * xv[s][e];
            }
        }
      }
    };
    ru_pass<T>(D, vec_ok, body);
    ru_reduce<T, CPW, KB>(acc, red_waves, red);
    // u = Dm·s (ascending column order)
    if (t < CPW * KB) {
      const int s = t / KB, i = t % KB;
      T u = 0;
      if (i < k)
        for (int j = 0; j < k; ++j) u += m.Dm[i + j * k] * red[s * KB + j];
      us[t] = u;
    }
    __syncthreads();
  }
  // pass 2: y[d] = a[d]·x[d] + Σ_j B[d, j]·u_j
  T u[CPW * KB];
#pragma unroll
  for (int i = 0; i < CPW * KB; ++i) u[i] = k > 0 ? us[i] : T(0);
  auto body2 = [&](int d0, int nel, bool vec) {
    V xv[CPW], av, tmp[CPW];
#pragma unroll
    for (int s = 0; s < CPW; ++s) {
      if (vec) xv[s] = *reinterpret_cast<const V*>(xp[s] + d0);
      else {
#pragma unroll
        for (int e = 0; e < VW; ++e) xv[s][e] = e < nel ? xp[s][d0 + e] : T(0);
      }
#pragma unroll
      for (int e = 0; e < VW; ++e) tmp[s][e] = 0;
    }
    if (vec) av = *reinterpret_cast<const V*>(m.a + d0);
    else {
#pragma unroll
      for (int e = 0; e < VW; ++e) av[e] = e < nel ? m.a[d0 + e] : T(0);
    }
#pragma unroll
    for (int j = 0; j < KB; ++j) {
      if (j < k) {
        V bv;
        const T* bp = m.B + (int64_t)j * D + d0;
        if (vec) bv = *reinterpret_cast<const V*>(bp);
        else {
#pragma unroll
          for (int e = 0; e < VW; ++e) bv[e] = e < nel ? bp[e] : T(0);
        }
#pragma unroll
        for (int s = 0; s < CPW; ++s)
#pragma unroll
          for (int e = 0; e < VW; ++e) tmp[s][e] += bv[e] * u[s * KB + j];
      }
    }
#pragma unroll
    for (int s = 0; s < CPW; ++s) {
      if (!live[s]) continue;
      V yv;
#pragma unroll
      for (int e = 0; e < VW; ++e) yv[e] = av[e] * xv[s][e] + tmp[s][e];
      if (vec) *reinterpret_cast<V*>(yp[s] + d0) = yv;
      else {
#pragma unroll
        for (int e = 0; e < VW; ++e)
          if (e < nel) yp[s][d0 + e] = yv[e];
      }
    }
  };
  ru_pass<T>(D, vec_ok, body2);
}

// R[:, c] = rand_momentum of the normals Z[:, c] for c < n (plain (D, n) arrays): z[1:k] ← V⁻¹z[1:k]; z ← z − Y·(Tw·(Yᵀz)); r = z ./ √A
template <class T, int KB>
__global__ __launch_bounds__(RU_THREADS) void k_ru_momentum(const RUOp<T> m, const T* __restrict__ Z, T* __restrict__ R, int D, int64_t n) {
  constexpr int CPW = RU_ACC / KB;
  constexpr int VW = 16 / (int)sizeof(T);
  typedef T V __attribute__((ext_vector_type(VW)));
  __shared__ T red_waves[(RU_THREADS / 64) * CPW * KB];
  __shared__ T red[CPW * KB];
  __shared__ T zk[CPW * KB];  // V⁻¹z[1:k] of each column
  __shared__ T hs[CPW * KB];  // Tw·(Yᵀz)
  const int k = m.k;
  const int t = threadIdx.x;
  const T* zp[CPW];
  T* rp[CPW];
  bool live[CPW];
  bool vec_ok = ((reinterpret_cast<uintptr_t>(m.isa) | reinterpret_cast<uintptr_t>(m.Y) | reinterpret_cast<uintptr_t>(Z) | reinterpret_cast<uintptr_t>(R)) & 15) == 0 &&
                ((int64_t)D * (int64_t)sizeof(T)) % 16 == 0;
#pragma unroll
  for (int s = 0; s < CPW; ++s) {
    const int64_t j = (int64_t)blockIdx.x * CPW + s;
    live[s] = j < n;
    const int64_t c = live[s] ? j : (int64_t)blockIdx.x * CPW;
    zp[s] = Z + c * D;
    rp[s] = R + c * D;
  }
  if (k > 0) {
    if (t < CPW * KB) {  // z[1:k] ← V⁻¹z[1:k] (V⁻¹ upper triangular, ascending column order)
      const int s = t / KB, i = t % KB;
      T w = 0;
      if (i < k)
        for (int j = i; j < k; ++j) w += m.Vinv[i + j * k] * zp[s][j];
      zk[t] = w;
    }
    __syncthreads();
  }
  // z′[d]: the normals with the first k replaced
  auto zval = [&](int s, int d, T z) -> T { return d < k ? zk[s * KB + d] : z; };
  if (k > 0) {
    T acc[CPW * KB];
#pragma unroll
    for (int i = 0; i < CPW * KB; ++i) acc[i] = 0;
    auto body = [&](int d0, int nel, bool vec) {
      V xv[CPW];
#pragma unroll
      for (int s = 0; s < CPW; ++s) {
        if (vec) xv[s] = *reinterpret_cast<const V*>(zp[s] + d0);
        else {
#pragma unroll
          for (int e = 0; e < VW; ++e) xv[s][e] = e < nel ? zp[s][d0 + e] : T(0);
        }
        if (d0 < k) {
#pragma unroll
          for (int e = 0; e < VW; ++e) xv[s][e] = zval(s, d0 + e, xv[s][e]);
        }
      }
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        if (j < k) {
          V yv;
          const T* yq = m.Y + (int64_t)j * D + d0;
          if (vec) yv = *reinterpret_cast<const V*>(yq);
          else {
#pragma unroll
            for (int e = 0; e < VW; ++e) yv[e] = e < nel ? yq[e] : T(0);
          }
#pragma unroll
          for (int e = 0; e < VW; ++e)
            if (e < nel) {
#pragma unroll
              for (int s = 0; s < CPW; ++s) acc[s * KB + j] += yv[e] * xv[s][e];
            }
        }
      }
    };
    ru_pass<T>(D, vec_ok, body);
    ru_reduce<T, CPW, KB>(acc, red_waves, red);
    if (t < CPW * KB) {  // h = Tw·(Yᵀz′) (Tw upper triangular)
      const int s = t / KB, i = t % KB;
      T h = 0;
      if (i < k)
        for (int j = i; j < k; ++j) h += m.Tw[i + j * k] * red[s * KB + j];
      hs[t] = h;
    }
    __syncthreads();
  }
  T h[CPW * KB];
#pragma unroll
  for (int i = 0; i < CPW * KB; ++i) h[i] = k > 0 ? hs[i] : T(0);
  auto body2 = [&](int d0, int nel, bool vec) {
    V xv[CPW], iv, tmp[CPW];
#pragma unroll
    for (int s = 0; s < CPW; ++s) {
      if (vec) xv[s] = *reinterpret_cast<const V*>(zp[s] + d0);
      else {
#pragma unroll
        for (int e = 0; e < VW; ++e) xv[s][e] = e < nel ? zp[s][d0 + e] : T(0);
      }
      if (d0 < k) {
#pragma unroll
        for (int e = 0; e < VW; ++e) xv[s][e] = zval(s, d0 + e, xv[s][e]);
      }
#pragma unroll
      for (int e = 0; e < VW; ++e) tmp[s][e] = 0;
    }
    if (vec) iv = *reinterpret_cast<const V*>(m.isa + d0);
    else {
#pragma unroll
      for (int e = 0; e < VW; ++e) iv[e] = e < nel ? m.isa[d0 + e] : T(0);
    }
#pragma unroll
    for (int j = 0; j < KB; ++j) {
      if (j < k) {
        V yv;
        const T* yq = m.Y + (int64_t)j * D + d0;
        if (vec) yv = *reinterpret_cast<const V*>(yq);
        else {
#pragma unroll
          for (int e = 0; e < VW; ++e) yv[e] = e < nel ? yq[e] : T(0);
        }
#pragma unroll
        for (int s = 0; s < CPW; ++s)
#pragma unroll
          for (int e = 0; e < VW; ++e) tmp[s][e] += yv[e] * h[s * KB + j];
      }
    }
#pragma unroll
    for (int s = 0; s < CPW; ++s) {
      if (!live[s]) continue;
      V rv;
#pragma unroll
      for (int e = 0; e < VW; ++e) rv[e] = (xv[s][e] - tmp[s][e]) * iv[e];
      if (vec) *reinterpret_cast<V*>(rp[s] + d0) = rv;
      else {
#pragma unroll
        for (int e = 0; e < VW; ++e)
          if (e < nel) rp[s][d0 + e] = rv[e];
      }
    }
  };
  ru_pass<T>(D, vec_ok, body2);
}

// the k bucket of a rank: KB = 4, 8, 16, 32 (k = 0 takes the smallest)
inline int ru_bucket(int k) { return k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : 32; }

}  // namespace ahmc
