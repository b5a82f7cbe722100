// ahmc_glm.hpp — device side of the generalised-linear-model target (include/ahmc_glm.h; host side: ahmc_glm_host.hpp; the
// arithmetic is defined by advancedhmc.jl_amd/glm.py).
//
// With the design matrix X (n_obs, D) and all chains' positions Θ (D, N) the linear predictor is ONE product X·Θ and the gradient
// ONE product Xᵀ·U — every chain shares X, as every chain shares M⁻¹ in k_dgemm, whose tiling, operand layout and k order these
// kernels take over (64×64 output tile per workgroup, or 64×16 when few chains are running; K stepped by GB_K through LDS, k
// ascending into one accumulator per element, zero padding past the end).  An accumulator therefore holds the k-ordered fma chain
// of its element, whichever tile shape computed it, and a chain's bits depend on (n_obs, D, family, element type) only — not on
// N, on the chain's column, on the chain list or on the tile shape.  No atomics; no kernel uses scratch.
#pragma once

#include "ahmc_dense.hpp"

namespace ahmc {

// Xᵀ·U runs over K = n_obs, a serial MFMA chain of n_obs/4 per wave however few chains are left; it is cut into slices of this
// fixed length (a multiple of GB_K), each a workgroup's own chain, and the slice sums are added in ascending order
// (k_glm_gsum).  The same constant is glm.K_SLICE of the mirror.
constexpr int GLM_K_SLICE = 1024;
static_assert(GLM_K_SLICE % GB_K == 0, "a slice is whole k tiles");

// tile shapes: BN = 64 (four waves as 2×2, each 32×32 = 2×2 MFMA tiles) or BN = 16 (four waves stacked, each one 16×16 MFMA tile)
template <int BN>
struct GlmShape {
  static_assert(BN == 64 || BN == 16, "64×64 or 64×16");
  static constexpr int WR = BN == 64 ? 2 : 4;              // waves along the rows
  static constexpr int MI = BN == 64 ? 2 : 1;              // MFMA tiles of a wave, each way
  static constexpr int BE = BN / 16;                       // B elements a thread stages per k tile
  static constexpr int LDA = GB_M + GB_PAD;
  static constexpr int LDB = BN + (BN == 64 ? GB_PAD : 4);
  static constexpr int SMEM = 2 * GB_K * (LDA + LDB);      // elements: the two LDS buffers of A and B; the epilogues reuse them
  static constexpr int LDE = GB_M + 1;                     // epilogue staging, [column][row] or [row][column]
  static_assert(BN * LDE <= SMEM && GB_M * (BN + 1) <= SMEM, "the epilogue's staging fits into the tile buffers");
};

// (row block, column block) of a workgroup.  BN = 64: a 1-D grid of row_blocks × 8·⌈col_blocks/8⌉ in k_dgemm's XCD-aware order (the
// row blocks of one column block share an L2); BN = 16: grid (row_blocks, col_blocks).
template <int BN>
__device__ __forceinline__ void glm_block(int nrb, int& rblk, int64_t& cb) {
  if constexpr (BN == 64) {
    const unsigned lin = blockIdx.x;
    const unsigned xcd = lin & 7u, slot = lin >> 3;
    cb = (int64_t)(slot / nrb) * 8 + xcd;
    rblk = (int)(slot % nrb);
  } else {
    rblk = blockIdx.x;
    cb = blockIdx.y;
  }
}

// acc += A[m0 .. m0+63, k0 .. k1) · B[k0 .. k1), this workgroup's BN columns].  A is column-major with leading dimension lda and M
// rows; Bcol is the column this THREAD stages (nullptr: a column past the list, zeros), indexed by k.  k_dgemm_small's pipeline:
// tile t in LDS buffer t & 1, tile t+1 in registers, the loads of tile t+2 issued before tile t is multiplied; one barrier per tile.
// On return all waves have passed the last barrier: smem is free.
template <class T, int BN>
__device__ __forceinline__ void glm_tile_product(const T* __restrict__ A, int64_t lda, int M, int m0, const T* __restrict__ Bcol, int k0, int k1,
                                                 T* __restrict__ smem, typename Mfma<T>::acc_t (&acc)[GlmShape<BN>::MI][GlmShape<BN>::MI]) {
  using S = GlmShape<BN>;
  using Mf = Mfma<T>;
  T* As = smem;                       // [2][GB_K][LDA]
  T* Bs = smem + 2 * GB_K * S::LDA;   // [2][GB_K][LDB]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = (w % S::WR) * 16 * S::MI, wn = (w / S::WR) * 16 * S::MI;
  const int ai = (tid & 31) * 2, ak = tid >> 5;                       // A tile: rows ai, ai+1 of k-rows ak and ak+8
  constexpr int KT = GB_K / S::BE;                                    // threads that share a B column
  const int bn = tid / KT, bk = (tid % KT) * S::BE;                   // B tile: column bn, k-rows bk .. bk+BE-1
  const bool arow0 = m0 + ai < M, arow1 = m0 + ai + 1 < M;
  const T* Ap = A + (m0 + ai);
  T ra[2][4], rb[2][S::BE];
  auto load_tile = [&](int kb, T (&a)[4], T (&b)[S::BE]) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int k = kb + ak + 8 * q;
      a[2 * q + 0] = (k < k1 && arow0) ? Ap[(int64_t)k * lda] : T(0);
      a[2 * q + 1] = (k < k1 && arow1) ? Ap[(int64_t)k * lda + 1] : T(0);
    }
#pragma unroll
    for (int e = 0; e < S::BE; ++e) {
      const int k = kb + bk + e;
      b[e] = (Bcol && k < k1) ? Bcol[k] : T(0);
    }
  };
  auto store_tile = [&](int buf, const T (&a)[4], const T (&b)[S::BE]) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int e = 0; e < 2; ++e) As[(buf * GB_K + ak + 8 * q) * S::LDA + ai + e] = a[2 * q + e];
#pragma unroll
    for (int e = 0; e < S::BE; ++e) Bs[(buf * GB_K + bk + e) * S::LDB + bn] = b[e];
  };
  const int nk = (k1 - k0 + GB_K - 1) / GB_K;
  const int nk_round = (nk + 1) / 2 * 2;  // tiles past k1 are all zero: harmless to multiply
  load_tile(k0, ra[0], rb[0]);
  load_tile(k0 + GB_K, ra[1], rb[1]);
  store_tile(0, ra[0], rb[0]);
  __syncthreads();
  for (int kt = 0; kt < nk_round; kt += 2) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      load_tile(k0 + (kt + s + 2) * GB_K, ra[s], rb[s]);
#pragma unroll
      for (int ks = 0; ks < GB_K / 4; ++ks) {
        const int kq = ks * 4 + (lane >> 4), l16 = lane & 15;
        T a[S::MI], b[S::MI];
#pragma unroll
        for (int i = 0; i < S::MI; ++i) {
          a[i] = As[(s * GB_K + kq) * S::LDA + wm + 16 * i + l16];
          b[i] = Bs[(s * GB_K + kq) * S::LDB + wn + 16 * i + l16];
        }
#pragma unroll
        for (int i = 0; i < S::MI; ++i)
#pragma unroll
          for (int j = 0; j < S::MI; ++j) acc[i][j] = Mf::mma(a[i], b[j], acc[i][j]);
      }
      store_tile(s ^ 1, ra[s ^ 1], rb[s ^ 1]);
      __syncthreads();
    }
  }
}

// (ℓ(y, η), u = ∂ℓ/∂η) of one observation.  Every multiply-add is an explicit fma, so the two tile shapes compile to the same
// arithmetic.  FAM: AHMC_GLM_BERNOULLI_LOGIT (0), AHMC_GLM_POISSON_LOG (1), AHMC_GLM_GAUSSIAN_IDENTITY (2).
template <class T, int FAM>
__device__ __forceinline__ void glm_link(T y, T eta, T scale, T& ll, T& u) {
  if constexpr (FAM == 0) {
    const T e = exp(-fabs(eta));
    const T sp = (eta > T(0) ? eta : T(0)) + log1p(e);   // softplus(η): finite for any finite η
    const T d = T(1) + e;
    const T sig = eta >= T(0) ? T(1) / d : e / d;        // σ(η) from the same exp(−|η|)
    ll = fma(y, eta, -sp);
    u = y - sig;
  } else if constexpr (FAM == 1) {
    const T ex = exp(eta);
    ll = fma(y, eta, -ex);
    u = y - ex;
  } else {
    const T r = y - eta;
    u = scale * r;
    ll = (T(-0.5) * u) * r;
  }
}

// ---- include/ahmc_glm_aux.h: families whose dispersion is sampled (FAM >= 3) -----------------------------------------------------------
// (L, Ψ) = (lgamma(y + φ) − lgamma(φ), ψ(y + φ) − ψ(φ)) as differences (glm.py: gamma_diffs): both arguments shifted by 8 with the
// recurrence, then Stirling's series, eight terms by Horner's rule in 1/x².  y = 0 gives exact zeros for a finite φ > 0; φ = 0 or
// φ = ∞ gives a non-finite L (ℓπ is then sanitised).  The recurrence loop stays rolled: one log1p and two divisions of code.
template <class T>
__device__ __forceinline__ T glm_stirling(const T (&c)[8], T z2) {
  T a = c[7];
#pragma unroll
  for (int k = 6; k >= 0; --k) a = fma(a, z2, c[k]);
  return a;
}

template <class T>
__device__ __forceinline__ void glm_gamma_diffs(T y, T phi, T& L, T& Psi) {
  const T cs[8] = {T(1.0 / 12), T(-1.0 / 360), T(1.0 / 1260), T(-1.0 / 1680), T(1.0 / 1188), T(-691.0 / 360360), T(1.0 / 156), T(-3617.0 / 122400)};
  const T ct[8] = {T(1.0 / 12), T(-1.0 / 120), T(1.0 / 252), T(-1.0 / 240), T(1.0 / 132), T(-691.0 / 32760), T(1.0 / 12), T(-3617.0 / 8160)};
  const T A = phi + T(8), B = A + y;
  const T z = y / A, lz = log1p(z);
  const T za = T(1) / A, zb = T(1) / B;
  const T za2 = za * za, zb2 = zb * zb;
  // (each product a statement of its own: written as one expression the difference contracts into fma(zb, S(B), −(za·S(A))), which
  // is not 0 at y = 0, where B = A)
  const T sb = zb * glm_stirling(cs, zb2), sa = za * glm_stirling(cs, za2);
  const T tb = zb2 * glm_stirling(ct, zb2), ta = za2 * glm_stirling(ct, za2);
  const T dS = sb - sa, dT = tb - ta;
  T sl = T(0), sp = T(0), pj = phi;
#pragma unroll 1
  for (int j = 0; j < 8; ++j) {
    const T t = y / pj;
    sl += log1p(t);
    sp += t / (y + pj);
    pj += T(1);  // (φ + j: exact steps whenever φ + j is, as in the mirror's phi + j, for φ < 2^p)
  }
  L = (fma(A - T(0.5), lz, y * (log(B) - T(1))) + dS) - sl;
  Psi = ((sp + lz) + (T(0.5) * z) / B) - dT;
}

// (ℓ, u = ∂ℓ/∂η, ∂ℓ/∂s) of one observation; s = the chain's log dispersion, cs = exp(−2s) (FAM 3) or φ = exp(s) (FAM 4), made
// once per tile column.  AHMC_GLM_GAUSSIAN_IDENTITY_SIGMA (3), AHMC_GLM_NEGBINOMIAL_LOG (4).
template <class T, int FAM>
__device__ __forceinline__ void glm_link_aux(T y, T eta, T s, T cs, T& ll, T& u, T& ds) {
  if constexpr (FAM == 3) {
    const T r = y - eta;
    u = cs * r;
    ll = fma(T(-0.5) * u, r, -s);
    ds = fma(u, r, T(-1));
  } else {
    const T d = eta - s;
    const T e = exp(-fabs(d));
    const T l = log1p(e);
    const T dd = T(1) + e;
    const T sig = d >= T(0) ? T(1) / dd : e / dd;    // σ(d) and 1 − σ(d) from the same exp(−|d|)
    const T nsig = d >= T(0) ? e / dd : T(1) / dd;
    const T sp = (d > T(0) ? d : T(0)) + l;          // log(μ + φ) − s
    const T sn = (d < T(0) ? -d : T(0)) + l;         // log(μ + φ) − η
    const T yp = y + cs;
    T L, Psi;
    glm_gamma_diffs(y, cs, L, Psi);
    ll = fma(-y, sn, fma(-cs, sp, L));
    u = fma(-yp, sig, y);
    ds = fma(cs, Psi - sp, fma(-yp, nsig, cs));
  }
}

// ---- include/ahmc_glm_ordinal.h: the ordered-logit family, whose C − 1 cutpoints are sampled (FAM == 5) -----------------------------
// θ ends with κ (C − 1 rows): c_1 = κ_1, δ_j = exp(κ_j) and c_j = c_{j−1} + δ_j for j >= 2 (glm.py: cutpoints).  Per (chain, cutpoint)
// constants of an interior category's link: lg_j = log(1 − e^{−δ_j}) — log(−expm1(−δ)) for δ <= log 2, log1p(−exp(−δ)) above — and
// r_j = 1/expm1(δ_j); both 0 at j = 1, which has no gap below it.
constexpr int GLM_ORD_MAX_CAT = 16;  // AHMC_GLM_ORDINAL_MAX_CATEGORIES

// (lg, r) of a gap δ > 0
template <class T>
__device__ __forceinline__ void glm_cut_gap(T d, T& lg, T& r) {
  const T em = exp(-d);
  lg = d <= T(0.693147180559945309417) ? log(-expm1(-d)) : log1p(-em);
  r = T(1) / expm1(d);
}

// the table of the listed columns of th (column stride ldt; κ begins at row k0): tab[(q·(C−1) + j)·ldo + column], q = 0 c, 1 lg, 2 r.
// One thread per column, j ascending.  With lgr = 0 only c is written (ahmc_glm_cutpoints: tab is then (C−1, n) with ldo = 1 and
// the column's stride C − 1: c_out).
template <class T>
__global__ __launch_bounds__(256) void k_glm_cut(const T* __restrict__ th, int64_t ldt, int64_t k0, int Cm1, T* __restrict__ tab, int64_t N, int64_t ncols,
                                                 const int* __restrict__ idx, int lgr) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ncols) return;
  const int64_t c = idx ? (int64_t)idx[j] : j;
  const T* kap = th + c * ldt + k0;
  // (lgr: tab (3, C−1, N), a chain per column; otherwise the draws' layout, a column's C − 1 cutpoints together)
  const int64_t sj = lgr ? N : 1, base = lgr ? c : c * Cm1;
  T cj = kap[0];
  tab[base] = cj;
  if (lgr) {
    tab[((int64_t)Cm1) * N + c] = T(0);
    tab[((int64_t)2 * Cm1) * N + c] = T(0);
  }
  for (int q = 1; q < Cm1; ++q) {
    const T d = exp(kap[q]);
    cj = cj + d;
    tab[base + q * sj] = cj;
    if (lgr) {
      T lg, r;
      glm_cut_gap(d, lg, r);
      tab[((int64_t)Cm1 + q) * N + c] = lg;
      tab[((int64_t)2 * Cm1 + q) * N + c] = r;
    }
  }
}

// (ℓ, u = ∂ℓ/∂η, da = ∂ℓ/∂a, db = ∂ℓ/∂b) of one observation in category yi of C: a = ca − η with ca = c_{y+1} (yi < C − 1),
// b = cb − η with cb = c_y (yi > 0); lg, r: the constants of the gap between them (used by an interior category only).  softplus and
// σ from one exp(−|x|) each, as FAM 0; no difference of two sigmoids is formed.
template <class T>
__device__ __forceinline__ void glm_link_ord(int yi, int Cm1, T eta, T ca, T cb, T lg, T r, T& ll, T& u, T& da, T& db) {
  const bool ha = yi < Cm1, hb = yi > 0;
  T spa = T(0), sna = T(0), spb = T(0), sb = T(0);
  if (ha) {
    const T a = ca - eta;
    const T e = exp(-fabs(a));
    const T d = T(1) + e;
    spa = (a < T(0) ? -a : T(0)) + log1p(e);   // softplus(−a)
    sna = a <= T(0) ? T(1) / d : e / d;        // σ(−a)
  }
  if (hb) {
    const T b = cb - eta;
    const T e = exp(-fabs(b));
    const T d = T(1) + e;
    spb = (b > T(0) ? b : T(0)) + log1p(e);    // softplus(b)
    sb = b >= T(0) ? T(1) / d : e / d;         // σ(b)
  }
  const bool in = ha && hb;
  ll = (-spa - spb) + (in ? lg : T(0));
  u = sb - sna;
  da = ha ? sna + (in ? r : T(0)) : T(0);
  db = hb ? -sb - (in ? r : T(0)) : T(0);
}

// η = X·Θ + offset for the listed chains, and from it in registers u → U (n_obs, N) and the tile's Σ_rows ℓ → partial[row block][chain].
// Tile rows are observations, tile columns chains, K = D.  η itself is stored only on request (ahmc_glm_pointwise: eta_out / ll_out,
// (n_obs, N) arrays).  U leaves through LDS so that a wave writes 64 consecutive observations of one chain; ℓ is summed over the
// tile's 64 rows in ascending row order by one thread per column (rows past n_obs contribute +0).
// FAM 3 and 4: the chain's log dispersion s is read from aux[col·aux_ld] (row D_θ − 1 of the chain's own θ, not of `th`, which holds the
// effective coefficients), once per tile column, and Σ_rows ∂ℓ/∂s goes to partial_s[row block][chain] by the same column sum.
// FAM == 5 (include/ahmc_glm_ordinal.h): y holds the category 0 … C − 1; aux is the cutpoint table of k_glm_cut (3, C−1, N), aux_ld
// = C − 1 and partial_s is partial_c (C−1, row blocks, N).  Each element gathers its chain's c / lg / r at the rows its y names from
// the table in global memory (at most 45 values per chain: L1 serves them).  da goes to an LDS array of its own as it is made, db
// through the tile buffers after ℓ; the column thread then forms, for k = 1 … C − 1, S_k of the tile: from +0, rows ascending, da
// of a row with y = k − 1, db of a row with y = k, nothing otherwise.
//
// FAC (include/ahmc_glm_factor.h): the product runs over the D dense columns only, `th` has column stride ldw (the model's P rows), and
// before the link each element takes W[off_f + lev[row, f]] of its chain's column for f = 0, 1, … in this order: what the fma chain
// would add for one-hot columns appended to X (fma(0, w, a) = a, fma(1, w, a) = a + w).
constexpr int GLM_MAX_FACTORS = 8;

struct GlmFacTab {  // the factor table, in the model's slab
  int F;                      // factors
  int off[GLM_MAX_FACTORS];   // the first coefficient row of factor f
  int L[GLM_MAX_FACTORS];     // its levels
};

template <class T, int FAM, int BN, bool FAC>
__device__ __forceinline__ void glm_eta_body(const T* __restrict__ X, const T* __restrict__ y, const T* __restrict__ off, T scale,
                                             const T* __restrict__ th, T* __restrict__ U, T* __restrict__ partial, int n_obs, int D, int64_t ncols, int64_t N,
                                             const int* __restrict__ idx, T* __restrict__ eta_out, T* __restrict__ ll_out, const T* __restrict__ aux,
                                             int64_t aux_ld, T* __restrict__ partial_s, int64_t ldw, const GlmFacTab* __restrict__ ft,
                                             const int* __restrict__ lev) {
  using S = GlmShape<BN>;
  using Mf = Mfma<T>;
  __shared__ T smem[S::SMEM];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nrb = (n_obs + GB_M - 1) / GB_M;
  int rblk;
  int64_t cb;
  glm_block<BN>(nrb, rblk, cb);
  const int m0 = rblk * GB_M;
  const int64_t n0 = cb * BN;
  if (n0 >= ncols) return;
  typename Mf::acc_t acc[S::MI][S::MI];
#pragma unroll
  for (int i = 0; i < S::MI; ++i)
#pragma unroll
    for (int j = 0; j < S::MI; ++j) acc[i][j] = typename Mf::acc_t{0, 0, 0, 0};
  {
    const int bn = tid / (GB_K / S::BE);
    const int64_t bcol = n0 + bn < ncols ? (idx ? (int64_t)idx[n0 + bn] : n0 + bn) : -1;
    glm_tile_product<T, BN>(X, (int64_t)n_obs, n_obs, m0, bcol >= 0 ? th + bcol * ldw : nullptr, 0, D, smem, acc);
  }
  const int wm = (w % S::WR) * 16 * S::MI, wn = (w / S::WR) * 16 * S::MI;
  [[maybe_unused]] T* ord_da = nullptr;
  [[maybe_unused]] int* ord_y = nullptr;
  if constexpr (FAM == 5) {
    __shared__ T s_da[GB_M * (BN + 1)];   // ∂ℓ/∂a, [row][column]
    __shared__ int s_y[GB_M];             // the tile rows' categories (−1 past n_obs: matches no cutpoint)
    ord_da = s_da;
    ord_y = s_y;
    if (tid < GB_M) s_y[tid] = m0 + tid < n_obs ? (int)y[m0 + tid] : -1;
    __syncthreads();
  }
  T ll[S::MI][S::MI][4];
  constexpr bool AUXF = FAM == 3 || FAM == 4, ORD = FAM == 5;
  constexpr int AM = AUXF ? S::MI : 1;              // (the legacy families carry none of the three)
  [[maybe_unused]] T ds[AM][AM][4];                 // ∂ℓ/∂s
  [[maybe_unused]] T sv[AM], cv[AM];                // s and exp(−2s) / exp(s) of this thread's tile columns
  constexpr int OM = ORD ? S::MI : 1;
  [[maybe_unused]] T dbv[OM][OM][4];                // ∂ℓ/∂b
  [[maybe_unused]] const int Cm1 = ORD ? (int)aux_ld : 0;
  if constexpr (AUXF) {
#pragma unroll
    for (int tj = 0; tj < S::MI; ++tj) {
      const int64_t j = n0 + wn + tj * 16 + (lane & 15);
      const T sj = j < ncols ? aux[(idx ? (int64_t)idx[j] : j) * aux_ld] : T(0);
      sv[tj] = sj;
      cv[tj] = FAM == 3 ? exp(T(-2) * sj) : exp(sj);
    }
  }
  // u → smem[column][row]
#pragma unroll
  for (int ti = 0; ti < S::MI; ++ti)
#pragma unroll
    for (int tj = 0; tj < S::MI; ++tj) {
      const int cl = wn + tj * 16 + (lane & 15);
      const int64_t j = n0 + cl;
      const int64_t col = j < ncols ? (idx ? (int64_t)idx[j] : j) : -1;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int rl = wm + ti * 16 + Mf::row(lane, v);
        const int row = m0 + rl;
        T l = T(0), u = T(0);
        [[maybe_unused]] T dl = T(0), dav = T(0), dbe = T(0);
        if (row < n_obs && col >= 0) {
          T eta = acc[ti][tj][v];
          if constexpr (FAC) {
            const T* wc = th + col * ldw;
            const int F = ft->F;
            for (int f = 0; f < F; ++f) eta += wc[ft->off[f] + lev[row + (int64_t)f * n_obs]];
          }
          if (off) eta += off[row];
          if constexpr (ORD) {
            const int yi = ord_y[rl];
            const int ia = yi < Cm1 ? yi : Cm1 - 1, ib = yi > 0 ? yi - 1 : 0;  // (clamped: the link ignores the side that does not exist)
            const T* tc = aux + col;
            glm_link_ord<T>(yi, Cm1, eta, tc[(int64_t)ia * N], tc[(int64_t)ib * N], tc[((int64_t)Cm1 + ia) * N], tc[((int64_t)2 * Cm1 + ia) * N], l, u, dav, dbe);
          } else if constexpr (AUXF) glm_link_aux<T, FAM>(y[row], eta, sv[tj], cv[tj], l, u, dl);
          else glm_link<T, FAM>(y[row], eta, scale, l, u);
          if (eta_out) eta_out[row + col * n_obs] = eta;
          if (ll_out) ll_out[row + col * n_obs] = l;
        }
        if constexpr (AUXF) ds[ti][tj][v] = dl;
        if constexpr (ORD) {
          dbv[ti][tj][v] = dbe;
          ord_da[rl * (BN + 1) + cl] = dav;
        }
        ll[ti][tj][v] = l;
        smem[cl * S::LDE + rl] = u;
      }
    }
  __syncthreads();
  for (int cl = w; cl < BN; cl += 4) {  // a wave per column: 64 consecutive observations
    const int64_t j = n0 + cl;
    if (j < ncols && m0 + lane < n_obs) {
      const int64_t col = idx ? (int64_t)idx[j] : j;
      U[(m0 + lane) + col * n_obs] = smem[cl * S::LDE + lane];
    }
  }
  __syncthreads();
  // ℓ → smem[row][column], then the column sums
#pragma unroll
  for (int ti = 0; ti < S::MI; ++ti)
#pragma unroll
    for (int tj = 0; tj < S::MI; ++tj)
#pragma unroll
      for (int v = 0; v < 4; ++v) smem[(wm + ti * 16 + Mf::row(lane, v)) * (BN + 1) + wn + tj * 16 + (lane & 15)] = ll[ti][tj][v];
  __syncthreads();
  if (tid < BN && n0 + tid < ncols) {
    const int64_t col = idx ? (int64_t)idx[n0 + tid] : n0 + tid;
    T s = T(0);
    for (int r = 0; r < GB_M; ++r) s += smem[r * (BN + 1) + tid];
    partial[(int64_t)rblk * N + col] = s;
  }
  if constexpr (ORD) {
    // ∂ℓ/∂b → smem[row][column] beside ∂ℓ/∂a; S_k of the tile, k outer, rows ascending, the term chosen by comparing y with k
    __syncthreads();
#pragma unroll
    for (int ti = 0; ti < S::MI; ++ti)
#pragma unroll
      for (int tj = 0; tj < S::MI; ++tj)
#pragma unroll
        for (int v = 0; v < 4; ++v) smem[(wm + ti * 16 + Mf::row(lane, v)) * (BN + 1) + wn + tj * 16 + (lane & 15)] = dbv[ti][tj][v];
    __syncthreads();
    if (tid < BN && n0 + tid < ncols) {
      const int64_t col = idx ? (int64_t)idx[n0 + tid] : n0 + tid;
      for (int k = 1; k <= Cm1; ++k) {
        T s = T(0);
        for (int r = 0; r < GB_M; ++r) {
          const int yr = ord_y[r];
          if (yr == k - 1) s += ord_da[r * (BN + 1) + tid];
          else if (yr == k) s += smem[r * (BN + 1) + tid];
        }
        partial_s[((int64_t)(k - 1) * nrb + rblk) * N + col] = s;
      }
    }
  }
  if constexpr (AUXF) {
    // ∂ℓ/∂s → smem[row][column], the same column sums
    __syncthreads();
#pragma unroll
    for (int ti = 0; ti < S::MI; ++ti)
#pragma unroll
      for (int tj = 0; tj < S::MI; ++tj)
#pragma unroll
        for (int v = 0; v < 4; ++v) smem[(wm + ti * 16 + Mf::row(lane, v)) * (BN + 1) + wn + tj * 16 + (lane & 15)] = ds[ti][tj][v];
    __syncthreads();
    if (tid < BN && n0 + tid < ncols) {
      const int64_t col = idx ? (int64_t)idx[n0 + tid] : n0 + tid;
      T s = T(0);
      for (int r = 0; r < GB_M; ++r) s += smem[r * (BN + 1) + tid];
      partial_s[(int64_t)rblk * N + col] = s;
    }
  }
}

template <class T, int FAM, int BN>
__global__ __launch_bounds__(256) void k_glm_eta(const T* __restrict__ X, const T* __restrict__ y, const T* __restrict__ off, T scale, const T* __restrict__ th,
                                                 T* __restrict__ U, T* __restrict__ partial, int n_obs, int D, int64_t ncols, int64_t N,
                                                 const int* __restrict__ idx, T* __restrict__ eta_out, T* __restrict__ ll_out, const T* __restrict__ aux,
                                                 int64_t aux_ld, T* __restrict__ partial_s) {
  glm_eta_body<T, FAM, BN, false>(X, y, off, scale, th, U, partial, n_obs, D, ncols, N, idx, eta_out, ll_out, aux, aux_ld, partial_s, (int64_t)D,
                                  (const GlmFacTab*)nullptr, (const int*)nullptr);
}

// k_glm_eta for a model with factors: X (n_obs, Px), W with column stride P, the level indices lev (n_obs, F) column-major
template <class T, int FAM, int BN>
__global__ __launch_bounds__(256) void k_glm_eta_f(const T* __restrict__ X, const T* __restrict__ y, const T* __restrict__ off, T scale, const T* __restrict__ W,
                                                   T* __restrict__ U, T* __restrict__ partial, int n_obs, int Px, int64_t P, int64_t ncols, int64_t N,
                                                   const int* __restrict__ idx, T* __restrict__ eta_out, T* __restrict__ ll_out, const T* __restrict__ aux,
                                                   int64_t aux_ld, T* __restrict__ partial_s, const GlmFacTab* __restrict__ ft, const int* __restrict__ lev) {
  glm_eta_body<T, FAM, BN, true>(X, y, off, scale, W, U, partial, n_obs, Px, ncols, N, idx, eta_out, ll_out, aux, aux_ld, partial_s, P, ft, lev);
}

// ---- include/ahmc_glm_categorical.h: the categorical-logit (softmax) family for unordered outcomes -------------------------------------
// y ∈ {0 … C − 1}, class 0 the reference (η_0 ≡ 0); K = C − 1 coefficient blocks of Pb rows, block k of a chain at W + col·ldw + k·Pb
// (glm.py: categorical_link).  The link of one observation of one chain, on its K predictors e[k·ps] (k = 0 … K − 1 stands for class
// k + 1) and m = max(0, η_1, …, η_K), made by the caller as  m = 0; m = η_k > m ? η_k : m  for ascending k:
//     e_0 = exp(−m), s = e_0, then s += exp(η_k − m) ascending;  inv = 1/s, lse = m + log(s);  ℓ = η_y − lse (η_0 = 0);
//     p_k = exp(η_k − m)·inv (the same exp of the same argument: the same bits),  u_k = 1 − p_k if y = k, else −p_k.
// u_k replaces η_k in place; ℓ is returned; pr (nullptr: none) receives the C probabilities p_0 … p_K.  One term of s is exactly 1, so
// s ∈ [1, C] and everything is finite for finite η.  There is no multiply-add in it.
constexpr int GLM_CAT_MAX_CAT = 16;  // AHMC_GLM_CATEGORICAL_MAX_CATEGORIES

template <class T>
__device__ __forceinline__ T glm_link_cat(int yi, int K, T* e, int64_t ps, T m, T* pr) {
  const T e0 = exp(-m);
  T s = e0, ey = T(0);
#pragma unroll 1
  for (int k = 0; k < K; ++k) {
    const T eta = e[(int64_t)k * ps];
    if (k + 1 == yi) ey = eta;
    const T ek = exp(eta - m);
    s += ek;
  }
  const T inv = T(1) / s;
  const T lse = m + log(s);
  if (pr) pr[0] = e0 * inv;
#pragma unroll 1
  for (int k = 0; k < K; ++k) {
    const T ek = exp(e[(int64_t)k * ps] - m);
    const T p = ek * inv;
    const T omp = T(1) - p;
    e[(int64_t)k * ps] = k + 1 == yi ? omp : -p;
    if (pr) pr[k + 1] = p;
  }
  return ey - lse;
}

// η_k = X·W_k (+ the factors' levels of block k) + off[k·n_obs + row] for k = 0 … K − 1 and the listed chains, one class at a time
// through ONE accumulator set: glm_tile_product with the B pointer moved to block k, then the tile leaves through LDS so that a wave
// writes 64 consecutive observations of one chain to plane k of U (K planes of (n_obs, N)).  The thread that writes (row m0 + lane,
// tile column w + 4·c) of plane k is the same for every k; it keeps the running m of its NS = BN/4 elements in an LDS array of its
// own, each word touched by that thread alone (in registers they would cost the 64×64 shape its second wave per SIMD), and, after
// the last class, runs glm_link_cat on the values it wrote itself (program order: no barrier between the two passes), which turns
// the planes into u_k.  ℓ goes to smem[row][column] and is summed over the tile's 64 rows in ascending row order by one thread per
// column, exactly as in k_glm_eta (rows past n_obs contribute +0).  eta_out (K planes of (n_obs, N)) / ll_out (n_obs, N) on request
// (ahmc_glm_pointwise); prob_out (C, n_obs, ·) column-major on request (ahmc_glm_class_probs: no chain list).  No atomics, no scratch.
template <class T, int BN, bool FAC>
__global__ __launch_bounds__(256) void k_glm_eta_cat(const T* __restrict__ X, const T* __restrict__ y, const T* __restrict__ off, const T* __restrict__ W,
                                                     T* U, T* __restrict__ partial, int n_obs, int Px, int Pb, int K, int64_t ldw, int64_t ncols, int64_t N,
                                                     const int* __restrict__ idx, T* __restrict__ eta_out, T* __restrict__ ll_out, T* __restrict__ prob_out,
                                                     const GlmFacTab* __restrict__ ft, const int* __restrict__ lev) {
  using S = GlmShape<BN>;
  using Mf = Mfma<T>;
  constexpr int NS = BN / 4;  // the tile columns a thread carries through LDS: w, w + 4, …
  __shared__ T smem[S::SMEM];
  __shared__ T s_m[BN * S::LDE];  // max(0, η_1 … η_k), [column][row]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nrb = (n_obs + GB_M - 1) / GB_M;
  int rblk;
  int64_t cb;
  glm_block<BN>(nrb, rblk, cb);
  const int m0 = rblk * GB_M;
  const int64_t n0 = cb * BN;
  if (n0 >= ncols) return;
  const int64_t plane = (int64_t)n_obs * N;
  const int bn = tid / (GB_K / S::BE);
  const int64_t bcol = n0 + bn < ncols ? (idx ? (int64_t)idx[n0 + bn] : n0 + bn) : -1;
  const int wm = (w % S::WR) * 16 * S::MI, wn = (w / S::WR) * 16 * S::MI;
  const int row_t = m0 + lane;
  const bool rok = row_t < n_obs;
  int colm[S::MI];  // the chains of this thread's accumulator columns (−1: past the list)
#pragma unroll
  for (int tj = 0; tj < S::MI; ++tj) {
    const int64_t j = n0 + wn + tj * 16 + (lane & 15);
    colm[tj] = j < ncols ? (idx ? idx[j] : (int)j) : -1;
  }
  // the chain of tile column cl for this thread's row (−1: nothing to write)
  auto chain_of = [&](int cl) -> int {
    const int64_t j = n0 + cl;
    return j < ncols && rok ? (idx ? idx[j] : (int)j) : -1;
  };
#pragma unroll
  for (int c = 0; c < NS; ++c) s_m[(w + 4 * c) * S::LDE + lane] = T(0);
#pragma unroll 1
  for (int k = 0; k < K; ++k) {
    typename Mf::acc_t acc[S::MI][S::MI];
#pragma unroll
    for (int i = 0; i < S::MI; ++i)
#pragma unroll
      for (int j = 0; j < S::MI; ++j) acc[i][j] = typename Mf::acc_t{0, 0, 0, 0};
    glm_tile_product<T, BN>(X, (int64_t)n_obs, n_obs, m0, bcol >= 0 ? W + bcol * ldw + (int64_t)k * Pb : nullptr, 0, Px, smem, acc);
    // η_k → smem[column][row]
#pragma unroll
    for (int ti = 0; ti < S::MI; ++ti)
#pragma unroll
      for (int tj = 0; tj < S::MI; ++tj) {
        const int cl = wn + tj * 16 + (lane & 15);
        const int col = colm[tj];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int rl = wm + ti * 16 + Mf::row(lane, v);
          const int row = m0 + rl;
          T eta = T(0);
          if (row < n_obs && col >= 0) {
            eta = acc[ti][tj][v];
            if constexpr (FAC) {
              const T* wc = W + (int64_t)col * ldw + (int64_t)k * Pb;
              const int F = ft->F;
              for (int f = 0; f < F; ++f) eta += wc[ft->off[f] + lev[row + (int64_t)f * n_obs]];
            }
            if (off) eta += off[(int64_t)k * n_obs + row];
          }
          smem[cl * S::LDE + rl] = eta;
        }
      }
    __syncthreads();
#pragma unroll 4
    for (int c = 0; c < NS; ++c) {  // a wave per column: 64 consecutive observations
      const int cl = w + 4 * c, col = chain_of(cl);
      if (col >= 0) {
        const T eta = smem[cl * S::LDE + lane];
        const int64_t at = (int64_t)k * plane + row_t + (int64_t)col * n_obs;
        U[at] = eta;
        if (eta_out) eta_out[at] = eta;
        const T m = s_m[cl * S::LDE + lane];
        s_m[cl * S::LDE + lane] = eta > m ? eta : m;
      }
    }
    __syncthreads();  // (the next class stages its tiles in smem)
  }
  // the link, each thread on the elements it wrote; ℓ → smem[row][column], then the column sums
  const int yi = rok ? (int)y[row_t] : 0;
#pragma unroll 1
  for (int c = 0; c < NS; ++c) {
    const int cl = w + 4 * c, col = chain_of(cl);
    T l = T(0);
    if (col >= 0) {
      const int64_t at = row_t + (int64_t)col * n_obs;
      l = glm_link_cat<T>(yi, K, U + at, plane, s_m[cl * S::LDE + lane], prob_out ? prob_out + (int64_t)(K + 1) * at : (T*)nullptr);
      if (ll_out) ll_out[at] = l;
    }
    smem[lane * (BN + 1) + cl] = l;
  }
  __syncthreads();
  if (tid < BN && n0 + tid < ncols) {
    const int64_t col = idx ? (int64_t)idx[n0 + tid] : n0 + tid;
    T s = T(0);
    for (int r = 0; r < GB_M; ++r) s += smem[r * (BN + 1) + tid];
    partial[(int64_t)rblk * N + col] = s;
  }
}

// Xᵀ·U for the listed chains.  Tile rows are coefficients, tile columns chains, K = the workgroup's slice of the observations; the
// A operand is the transposed copy Xt (D, n_obs) made when the target was set.  One slice (n_obs <= GLM_K_SLICE): the epilogue
// writes g = −acc + p∘θ to the chain's column of g.  More: the slice's sum goes to gs[slice][chain][d] and k_glm_gsum finishes.
// ldg: the column stride of th and g (D; the model's P when the D dense rows are the first of P: k_glm_grad_ld).
template <class T, int BN>
__device__ __forceinline__ void glm_grad_body(const T* __restrict__ Xt, const T* __restrict__ U, const T* __restrict__ prec,
                                              const T* __restrict__ th, T* __restrict__ g, T* __restrict__ gs, int n_obs, int D, int64_t ncols, int64_t N,
                                              const int* __restrict__ idx, int n_slices, int64_t ldg) {
  using S = GlmShape<BN>;
  using Mf = Mfma<T>;
  __shared__ T smem[S::SMEM];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nrb1 = (D + GB_M - 1) / GB_M;
  int rs;
  int64_t cb;
  glm_block<BN>(nrb1 * n_slices, rs, cb);
  const int slice = rs / nrb1, m0 = (rs % nrb1) * GB_M;
  const int64_t n0 = cb * BN;
  if (n0 >= ncols) return;
  typename Mf::acc_t acc[S::MI][S::MI];
#pragma unroll
  for (int i = 0; i < S::MI; ++i)
#pragma unroll
    for (int j = 0; j < S::MI; ++j) acc[i][j] = typename Mf::acc_t{0, 0, 0, 0};
  {
    const int bn = tid / (GB_K / S::BE);
    const int64_t bcol = n0 + bn < ncols ? (idx ? (int64_t)idx[n0 + bn] : n0 + bn) : -1;
    const int k0 = slice * GLM_K_SLICE, k1 = k0 + GLM_K_SLICE < n_obs ? k0 + GLM_K_SLICE : n_obs;
    glm_tile_product<T, BN>(Xt, (int64_t)D, D, m0, bcol >= 0 ? U + bcol * n_obs : nullptr, k0, k1, smem, acc);
  }
  const int wm = (w % S::WR) * 16 * S::MI, wn = (w / S::WR) * 16 * S::MI;
#pragma unroll
  for (int ti = 0; ti < S::MI; ++ti)
#pragma unroll
    for (int tj = 0; tj < S::MI; ++tj) {
      const int64_t j = n0 + wn + tj * 16 + (lane & 15);
      const int64_t col = j < ncols ? (idx ? (int64_t)idx[j] : j) : -1;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = m0 + wm + ti * 16 + Mf::row(lane, v);
        if (row < D && col >= 0) {
          if (n_slices == 1) g[row + col * ldg] = fma(prec[row], th[row + col * ldg], -acc[ti][tj][v]);
          else gs[((int64_t)slice * N + col) * D + row] = acc[ti][tj][v];
        }
      }
    }
}

template <class T, int BN>
__global__ __launch_bounds__(256) void k_glm_grad(const T* __restrict__ Xt, const T* __restrict__ U, const T* __restrict__ prec, const T* __restrict__ th,
                                                  T* __restrict__ g, T* __restrict__ gs, int n_obs, int D, int64_t ncols, int64_t N,
                                                  const int* __restrict__ idx, int n_slices) {
  glm_grad_body<T, BN>(Xt, U, prec, th, g, gs, n_obs, D, ncols, N, idx, n_slices, (int64_t)D);
}

// k_glm_grad over the Px dense columns of a model with factors: rows [0, Px) of R, whose column stride (and W's) is P
template <class T, int BN>
__global__ __launch_bounds__(256) void k_glm_grad_ld(const T* __restrict__ Xt, const T* __restrict__ U, const T* __restrict__ prec, const T* __restrict__ W,
                                                     T* __restrict__ R, T* __restrict__ gs, int n_obs, int Px, int64_t P, int64_t ncols, int64_t N,
                                                     const int* __restrict__ idx, int n_slices) {
  glm_grad_body<T, BN>(Xt, U, prec, W, R, gs, n_obs, Px, ncols, N, idx, n_slices, P);
}

// g = −(Σ_slices gs, ascending) + p∘θ for the listed chains (n_slices > 1); th and g have the column stride ldg
template <class T>
__device__ __forceinline__ void glm_gsum_body(const T* __restrict__ gs, const T* __restrict__ prec, const T* __restrict__ th, T* __restrict__ g, int D,
                                              int64_t ncols, int64_t N, const int* __restrict__ idx, int n_slices, int64_t ldg) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ncols * D) return;
  const int64_t j = i / D, col = idx ? (int64_t)idx[j] : j;
  const int d = (int)(i % D);
  T s = gs[col * D + d];
  for (int sl = 1; sl < n_slices; ++sl) s += gs[((int64_t)sl * N + col) * D + d];
  g[d + col * ldg] = fma(prec[d], th[d + col * ldg], -s);
}

template <class T>
__global__ __launch_bounds__(256) void k_glm_gsum(const T* __restrict__ gs, const T* __restrict__ prec, const T* __restrict__ th, T* __restrict__ g, int D,
                                                  int64_t ncols, int64_t N, const int* __restrict__ idx, int n_slices) {
  glm_gsum_body<T>(gs, prec, th, g, D, ncols, N, idx, n_slices, (int64_t)D);
}

template <class T>
__global__ __launch_bounds__(256) void k_glm_gsum_ld(const T* __restrict__ gs, const T* __restrict__ prec, const T* __restrict__ W, T* __restrict__ R, int Px,
                                                     int64_t P, int64_t ncols, int64_t N, const int* __restrict__ idx, int n_slices) {
  glm_gsum_body<T>(gs, prec, W, R, Px, ncols, N, idx, n_slices, P);
}

// The factor rows of R = −Xᵀu for the listed chains, without the one-hot columns: row Px + q of R is level q of the factors' levels
// taken together (factor 0's first).  perm lists, level after level, the observations of the level in ascending order (the stable
// permutation by level made when the target was set; rp[q] .. rp[q + 1] is level q's stretch).  One thread per (chain, level) walks
// its stretch: within a slice of GLM_K_SLICE observations u is summed in ascending order from +0, the slice sums are added in
// ascending order — the fma chain of a one-hot column and k_glm_gsum's order (a slice without a member adds +0: no change).  A
// chain's column of U is read once and stays in L2 meanwhile; consecutive lanes write consecutive rows of R.  An empty level writes
// a zero.  No atomics, no workspace.
template <class T>
__global__ __launch_bounds__(256) void k_glm_fgrad(const T* __restrict__ U, const int* __restrict__ perm, const int* __restrict__ rp, T* __restrict__ R, int n_obs,
                                                   int Px, int Lt, int64_t P, int64_t ncols, const int* __restrict__ idx) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ncols * Lt) return;
  const int64_t j = t / Lt, c = idx ? (int64_t)idx[j] : j;
  const int q = (int)(t % Lt);
  const T* u = U + c * n_obs;
  T tot = T(0), s = T(0);
  int sl = 0;
  const int k1 = rp[q + 1];
  for (int k = rp[q]; k < k1; ++k) {
    const int i = perm[k];
    const int si = i / GLM_K_SLICE;
    if (si != sl) {
      tot += s;
      s = T(0);
      sl = si;
    }
    s += u[i];
  }
  tot += s;
  R[(int64_t)Px + q + c * P] = -tot;
}

// ℓπ = Σ_row blocks partial − ½ Σ_d p_d θ_d², one wave per chain (as k_d_coldot): lane l sums the row blocks and the coefficients
// l, l+64, … in ascending order, then wave_allsum2.  sanitize_lp = 0: the caller's next kernel sanitises ℓπ as it reads it.
template <class T>
__global__ __launch_bounds__(256) void k_glm_lp(const T* __restrict__ partial, const T* __restrict__ prec, const T* __restrict__ th, T* __restrict__ lp, int nrb,
                                                int D, int64_t ncols, int64_t N, const int* __restrict__ idx, int sanitize_lp) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= ncols) return;
  const int64_t c = idx ? (int64_t)idx[j] : j;
  T s[2] = {0, 0};
  for (int rb = lane; rb < nrb; rb += 64) s[0] += partial[(int64_t)rb * N + c];
  for (int d = lane; d < D; d += 64) {
    const T t = th[c * D + d];
    s[1] = fma(prec[d] * t, t, s[1]);
  }
  wave_allsum2<64>(s[0], s[1]);
  const T v = fma(T(-0.5), s[1], s[0]);
  if (lane == 0) lp[c] = sanitize_lp ? sanitize(v) : v;
}

// ---- include/ahmc_glm_hier.h: coefficient groups whose prior scale is sampled -------------------------------------------------------
// θ (D = P + G): θ[0:P] coefficient parameters, θ[P + k] = s_k = log τ_k of group k = [lo_k, hi_k).  The products above run on the
// EFFECTIVE coefficients W (P, N) — w_d = θ_d, or τ_k·θ_d for a member of a non-centred group — with th := W, D := P, prec := 0 and
// g := R, so R = −Xᵀu; k_hglm_coef makes W before them and k_hglm_finish the chain's ℓπ and all D rows of g after them.  Formulas
// and the order of every sum: glm.py.  Both are one wave per chain, four chains per block, every group loop wave-uniform.
constexpr int HGLM_MAX_GROUPS = 32;

template <class T>
struct HglmTab {  // the group table, in the model's slab
  int lo[HGLM_MAX_GROUPS], hi[HGLM_MAX_GROUPS], centered[HGLM_MAX_GROUPS];
  T inv_a2[HGLM_MAX_GROUPS];  // 1/A_k²
};

// W (column stride P) and / or τ (column stride G) of the listed columns of th (column stride ldt: P + G, or P + G + 1 with a
// dispersion's row); either output may be nullptr.  One exp per (column, group).
template <class T>
__global__ __launch_bounds__(256) void k_hglm_coef(const T* __restrict__ th, const HglmTab<T>* __restrict__ tab, T* __restrict__ W, T* __restrict__ tau_out, int P,
                                                   int G, int64_t ldt, int64_t ncols, const int* __restrict__ idx) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= ncols) return;
  const int64_t c = idx ? (int64_t)idx[j] : j;
  const T* t = th + c * ldt;
  T* w = W ? W + c * P : nullptr;
  int prev = 0;
  for (int k = 0; k <= G; ++k) {
    const int lo = k < G ? tab->lo[k] : P;
    if (w)
      for (int d = prev + lane; d < lo; d += 64) w[d] = t[d];
    if (k == G) break;
    const int hi = tab->hi[k];
    const T tau = exp(t[P + k]);
    if (tau_out && lane == 0) tau_out[c * G + k] = tau;
    if (w) {
      if (tab->centered[k])
        for (int d = lo + lane; d < hi; d += 64) w[d] = t[d];
      else
        for (int d = lo + lane; d < hi; d += 64) w[d] = tau * t[d];
    }
    prev = hi;
  }
}

// out[j] = exp(th[row, j]), th (ld, n): the dispersion e^s of draws (ahmc_glm_dispersion), by the exp that makes τ above
template <class T>
__global__ __launch_bounds__(256) void k_glm_exp_row(const T* __restrict__ th, int64_t ld, int64_t row, int64_t n, T* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) out[j] = exp(th[j * ld + row]);
}

// ℓπ and g of the listed chains from partial (Σℓ per row block), R = −Xᵀu, W and θ.  k_glm_lp's sums first (Σ partial, Σ p_d θ_d² over
// d < P: members have p_d = 0), then per group, ascending: (S_k, T_k) lane-strided from lo_k and wave_allsum2, the hyperprior, the
// members' rows of g and the row of s_k; the coefficients in no group last.  No LDS, no atomics.
//
// AUX (include/ahmc_glm_aux.h): θ has one more row, s = the log of the family's dispersion, after the G log-scales.  Σ_row blocks
// partial_s (= Σ_i ∂ℓ/∂s) is summed beside Σ partial in the same lane-strided order and by a butterfly of its own; after the groups
// the prior s ~ Normal(m, A²) is added: r = s − m, ℓπ = fma((−½/A²)·r, r, ℓπ), g[D−1] = fma(r, 1/A², −Σ ∂ℓ/∂s).
//
// ORD (include/ahmc_glm_ordinal.h): θ's last n_cut = C − 1 rows are κ, after the G log-scales.  The prior first, j ascending:
// r_j = κ_j − loc, ℓπ = fma((−½/scale²)·r_j, r_j, ℓπ) with (loc_1, scale_1) for j = 1 and (loc_gap, scale_gap) above.  Then j
// descending: S_j = Σ_row blocks partial_c[j] (lane-strided, a butterfly of its own, as partial_s), T_j = S_j + T_{j+1},
// g[κ_1] = fma(r_1, 1/scale_1², −T_1), g[κ_j] = fma(−δ_j, T_j, r_j·(1/scale_gap²)) with δ_j = exp(κ_j), k_glm_cut's exp.
struct GlmCutPrior {
  double loc1, ia1, locg, iag;  // (loc_1, 1/scale_1², loc_gap, 1/scale_gap²)
};

template <class T, bool AUX, bool ORD = false>
__device__ __forceinline__ void hglm_finish_body(const T* __restrict__ partial, const T* __restrict__ R, const T* __restrict__ W, const T* __restrict__ prec,
                                                 const T* __restrict__ th, const HglmTab<T>* __restrict__ tab, T* __restrict__ lp, T* __restrict__ g, int nrb, int P,
                                                 int G, int64_t ncols, int64_t N, const int* __restrict__ idx, int sanitize_lp, const T* __restrict__ partial_s,
                                                 T aux_loc, T aux_ia2, int n_cut = 0, GlmCutPrior cp = {}) {
  const int64_t ldt = (int64_t)P + G + (AUX ? 1 : 0) + (ORD ? n_cut : 0);
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= ncols) return;
  const int64_t c = idx ? (int64_t)idx[j] : j;
  const T* t = th + c * ldt;
  const T* r = R + c * P;
  const T* w = W + c * P;
  T* gc = g + c * ldt;
  T s[2] = {0, 0};
  for (int rb = lane; rb < nrb; rb += 64) s[0] += partial[(int64_t)rb * N + c];
  for (int d = lane; d < P; d += 64) {
    const T td = t[d];
    s[1] = fma(prec[d] * td, td, s[1]);
  }
  wave_allsum2<64>(s[0], s[1]);
  T dsum[2] = {0, 0};
  if constexpr (AUX) {
    for (int rb = lane; rb < nrb; rb += 64) dsum[0] += partial_s[(int64_t)rb * N + c];
    wave_allsum2<64>(dsum[0], dsum[1]);
  }
  T v = fma(T(-0.5), s[1], s[0]);
  int prev = 0;
  for (int k = 0; k <= G; ++k) {
    const int lo = k < G ? tab->lo[k] : P;
    for (int d = prev + lane; d < lo; d += 64) gc[d] = fma(prec[d], t[d], r[d]);
    if (k == G) break;
    const int hi = tab->hi[k];
    const bool cen = tab->centered[k] != 0;
    const T sk = t[P + k], ia2 = tab->inv_a2[k], m = (T)(hi - lo);
    T a[2] = {0, 0};  // S_k, T_k
    for (int d = lo + lane; d < hi; d += 64) {
      const T td = t[d];
      a[0] = fma(td, td, a[0]);
      a[1] = fma(r[d], w[d], a[1]);
    }
    wave_allsum2<64>(a[0], a[1]);
    const T e2 = exp(T(2) * sk);
    const T h = fma(T(-0.5) * e2, ia2, sk), hp = fma(-e2, ia2, T(1));
    T b, gs;
    if (cen) {
      const T q = exp(T(-2) * sk);
      b = fma(-m, sk, (T(-0.5) * q) * a[0]);
      gs = fma(-q, a[0], m) - hp;
      for (int d = lo + lane; d < hi; d += 64) gc[d] = fma(q, t[d], r[d]);
    } else {
      const T tau = exp(sk);
      b = T(-0.5) * a[0];
      gs = a[1] - hp;
      for (int d = lo + lane; d < hi; d += 64) gc[d] = fma(tau, r[d], t[d]);
    }
    v += h + b;
    if (lane == 0) gc[P + k] = gs;
    prev = hi;
  }
  if constexpr (AUX) {
    const T ra = t[P + G] - aux_loc;
    v = fma((T(-0.5) * aux_ia2) * ra, ra, v);
    if (lane == 0) gc[P + G] = fma(ra, aux_ia2, -dsum[0]);
  }
  if constexpr (ORD) {
    const T* kap = t + P + G;
    const T ia1 = (T)cp.ia1, iag = (T)cp.iag, loc1 = (T)cp.loc1, locg = (T)cp.locg;
    for (int q = 0; q < n_cut; ++q) {
      const T rq = kap[q] - (q == 0 ? loc1 : locg);
      v = fma((T(-0.5) * (q == 0 ? ia1 : iag)) * rq, rq, v);
    }
    T Tq = T(0);
    for (int q = n_cut - 1; q >= 0; --q) {
      T sq[2] = {0, 0};
      const T* pc = partial_s + (int64_t)q * nrb * N + c;
      for (int rb = lane; rb < nrb; rb += 64) sq[0] += pc[(int64_t)rb * N];
      wave_allsum2<64>(sq[0], sq[1]);
      Tq = q == n_cut - 1 ? sq[0] : sq[0] + Tq;
      const T kq = kap[q];
      const T gq = q == 0 ? fma(kq - loc1, ia1, -Tq) : fma(-exp(kq), Tq, (kq - locg) * iag);
      if (lane == 0) gc[P + G + q] = gq;
    }
  }
  if (lane == 0) lp[c] = sanitize_lp ? sanitize(v) : v;
}

template <class T>
__global__ __launch_bounds__(256) void k_hglm_finish_ord(const T* __restrict__ partial, const T* __restrict__ partial_c, const T* __restrict__ R,
                                                         const T* __restrict__ W, const T* __restrict__ prec, const T* __restrict__ th,
                                                         const HglmTab<T>* __restrict__ tab, T* __restrict__ lp, T* __restrict__ g, int nrb, int P, int G,
                                                         int64_t ncols, int64_t N, const int* __restrict__ idx, int sanitize_lp, int n_cut, double loc1,
                                                         double ia1, double locg, double iag) {
  hglm_finish_body<T, false, true>(partial, R, W, prec, th, tab, lp, g, nrb, P, G, ncols, N, idx, sanitize_lp, partial_c, T(0), T(0), n_cut,
                                   GlmCutPrior{loc1, ia1, locg, iag});
}

template <class T>
__global__ __launch_bounds__(256) void k_hglm_finish(const T* __restrict__ partial, const T* __restrict__ R, const T* __restrict__ W, const T* __restrict__ prec,
                                                     const T* __restrict__ th, const HglmTab<T>* __restrict__ tab, T* __restrict__ lp, T* __restrict__ g, int nrb,
                                                     int P, int G, int64_t ncols, int64_t N, const int* __restrict__ idx, int sanitize_lp) {
  hglm_finish_body<T, false>(partial, R, W, prec, th, tab, lp, g, nrb, P, G, ncols, N, idx, sanitize_lp, (const T*)nullptr, T(0), T(0));
}

template <class T>
__global__ __launch_bounds__(256) void k_hglm_finish_aux(const T* __restrict__ partial, const T* __restrict__ partial_s, const T* __restrict__ R,
                                                         const T* __restrict__ W, const T* __restrict__ prec, const T* __restrict__ th,
                                                         const HglmTab<T>* __restrict__ tab, T* __restrict__ lp, T* __restrict__ g, int nrb, int P, int G,
                                                         int64_t ncols, int64_t N, const int* __restrict__ idx, int sanitize_lp, T aux_loc, T aux_ia2) {
  hglm_finish_body<T, true>(partial, R, W, prec, th, tab, lp, g, nrb, P, G, ncols, N, idx, sanitize_lp, partial_s, aux_loc, aux_ia2);
}

}  // namespace ahmc
