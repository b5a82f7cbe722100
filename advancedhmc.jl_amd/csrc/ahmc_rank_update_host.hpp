// ahmc_rank_update_host.hpp — host side of RankUpdateEuclideanMetric (include/ahmc_rank_update.h; kernels: ahmc_rank_update.hpp).
// Included by ahmc_api.hip after the context, before ahmc_dense_host.hpp, whose dn_minv_apply / dn_momentum_map route to the
// launches here.
#pragma once

template <class T>
RUOp<T> ru_op(const Ctx<T>* c) {
  RUOp<T> m;
  const T* b = c->ru_buf;
  m.a = b + c->ru_off[0];
  m.isa = b + c->ru_off[1];
  m.B = b + c->ru_off[2];
  m.Dm = b + c->ru_off[3];
  m.Y = b + c->ru_off[4];
  m.Tw = b + c->ru_off[5];
  m.Vinv = b + c->ru_off[6];
  m.k = c->ru_k;
  return m;
}

// Y = M⁻¹X for the listed columns, with dn_gemm's operand addressing (xcs / ycs = 0: the plain (D, N) array)
template <class T>
int ru_apply(Ctx<T>* c, const T* X, T* Y, int64_t ncols, const int* list, const int* ptidx, int64_t xps, int64_t yps, int64_t xcs, int64_t ycs) {
  if (ncols <= 0) return AHMC_OK;
  if (xcs == 0) xcs = c->D;
  if (ycs == 0) ycs = c->D;
  const RUOp<T> m = ru_op(c);
  const int kb = ru_bucket(c->ru_k), cpw = RU_ACC / kb;
  const dim3 grid((unsigned)((ncols + cpw - 1) / cpw)), block(RU_THREADS);
  switch (kb) {
#define AHMC_RU_APPLY(KB) case KB: hipLaunchKernelGGL((k_ru_apply<T, KB>), grid, block, 0, c->stream, m, X, Y, (int)c->D, ncols, list, ptidx, xps, yps, xcs, ycs); break
    AHMC_RU_APPLY(4); AHMC_RU_APPLY(8); AHMC_RU_APPLY(16); AHMC_RU_APPLY(32);
#undef AHMC_RU_APPLY
  }
  HIPCHK(hipGetLastError());
  return AHMC_OK;
}

// R = the momenta of the normals Z, ncols plain (D, ·) columns
template <class T>
int ru_momentum(Ctx<T>* c, const T* Z, T* R, int64_t ncols) {
  if (ncols <= 0) return AHMC_OK;
  const RUOp<T> m = ru_op(c);
  const int kb = ru_bucket(c->ru_k), cpw = RU_ACC / kb;
  const dim3 grid((unsigned)((ncols + cpw - 1) / cpw)), block(RU_THREADS);
  switch (kb) {
#define AHMC_RU_MOM(KB) case KB: hipLaunchKernelGGL((k_ru_momentum<T, KB>), grid, block, 0, c->stream, m, Z, R, (int)c->D, ncols); break
    AHMC_RU_MOM(4); AHMC_RU_MOM(8); AHMC_RU_MOM(16); AHMC_RU_MOM(32);
#undef AHMC_RU_MOM
  }
  HIPCHK(hipGetLastError());
  return AHMC_OK;
}

// M⁻¹ = Diagonal(A) + B·Dm·Bᵀ: the inputs and woodbury_factorize (src/metric.jl:164-177) in double on the host —
//   U = √A;  U⁻¹B = Q·R, thin Householder QR with LAPACK's dgeqr2 / dlarfg conventions (Q = H₁⋯H_k, H_j = I − τ_j v_j v_jᵀ, v_j(j) = 1),
//   so that Q = qr(U \ B).Q;  the compact-WY Tw of Q = I − Y·Tw·Yᵀ as dlarft (forward, columnwise) forms it;
//   V = chol(Symmetric(I + R·Dm·Rᵀ)).U, reading the upper triangle.
template <class T>
int ru_set_metric(Ctx<T>* c, const T* A_in, const T* B_in, const T* Dm_in, int64_t k) {
  const int64_t D = c->D;
  if (k < 0 || k > D)
    return fail(c, AHMC_ERR_ARGUMENT, "DimensionMismatch: set_metric_rank_update needs 0 <= k <= D (B is (D, k), Dm is (k, k)); got k = " + std::to_string(k));
  if (k > RU_MAX_K)
    return fail(c, AHMC_ERR_UNSUPPORTED, "set_metric_rank_update: rank k = " + std::to_string(k) + " is beyond the engine's limit AHMC_RANK_UPDATE_MAX_K = " +
                                             std::to_string(RU_MAX_K));
  if (k > 0 && (!B_in || !Dm_in)) return fail(c, AHMC_ERR_ARGUMENT, "set_metric_rank_update: B or Dm is NULL with k > 0");
  std::vector<T> hA((size_t)D, T(1)), hB((size_t)(D * k)), hD((size_t)(k * k));
  if (A_in) HIPCHK(hipMemcpy(hA.data(), A_in, sizeof(T) * D, hipMemcpyDefault));
  if (k > 0) {
    HIPCHK(hipMemcpy(hB.data(), B_in, sizeof(T) * D * k, hipMemcpyDefault));
    HIPCHK(hipMemcpy(hD.data(), Dm_in, sizeof(T) * k * k, hipMemcpyDefault));
  }
  for (int64_t d = 0; d < D; ++d)
    if (!(std::isfinite((double)hA[d]) && hA[d] > 0))
      return fail(c, AHMC_ERR_ARGUMENT, "DomainError: A must be a positive definite diagonal (every value finite and > 0); A[" + std::to_string(d + 1) + "] = " +
                                            std::to_string((double)hA[d]));
  for (int64_t i = 0; i < D * k; ++i)
    if (!std::isfinite((double)hB[i])) return fail(c, AHMC_ERR_ARGUMENT, "ArgumentError: B holds a non-finite value");
  for (int64_t i = 0; i < k * k; ++i)
    if (!std::isfinite((double)hD[i])) return fail(c, AHMC_ERR_ARGUMENT, "ArgumentError: Dm holds a non-finite value");
  // M = U⁻¹B, overwritten by the QR: R on and above the diagonal, v_j below
  std::vector<double> M((size_t)(D * k)), tau((size_t)k, 0.0);
  for (int64_t j = 0; j < k; ++j)
    for (int64_t d = 0; d < D; ++d) M[d + j * D] = (double)hB[d + j * D] / std::sqrt((double)hA[d]);
  for (int64_t j = 0; j < k; ++j) {
    double* col = M.data() + j * D;
    const double alpha = col[j];
    double xn = 0;
    for (int64_t i = j + 1; i < D; ++i) xn = std::hypot(xn, col[i]);
    if (xn == 0) {
      tau[j] = 0;  // H_j = I
    } else {
      const double beta = -std::copysign(std::hypot(alpha, xn), alpha);
      tau[j] = (beta - alpha) / beta;
      const double scal = 1 / (alpha - beta);
      for (int64_t i = j + 1; i < D; ++i) col[i] *= scal;
      col[j] = beta;
    }
    if (tau[j] == 0) continue;
    for (int64_t cc = j + 1; cc < k; ++cc) {  // apply H_j to the remaining columns
      double* x = M.data() + cc * D;
      double w = x[j];
      for (int64_t i = j + 1; i < D; ++i) w += col[i] * x[i];
      w *= tau[j];
      x[j] -= w;
      for (int64_t i = j + 1; i < D; ++i) x[i] -= w * col[i];
    }
  }
  std::vector<double> Y((size_t)(D * k), 0.0), Tw((size_t)(k * k), 0.0), R((size_t)(k * k), 0.0);
  for (int64_t j = 0; j < k; ++j) {
    Y[j + j * D] = 1;
    for (int64_t i = j + 1; i < D; ++i) Y[i + j * D] = M[i + j * D];
    for (int64_t i = 0; i <= j; ++i) R[i + j * k] = M[i + j * D];
  }
  for (int64_t i = 0; i < k; ++i) {  // dlarft: Tw(0:i, i) = −τ_i·Tw(0:i, 0:i)·(Y(:, 0:i)ᵀ v_i), Tw(i, i) = τ_i
    if (tau[i] == 0) continue;
    std::vector<double> w((size_t)i, 0.0);
    for (int64_t j = 0; j < i; ++j) {
      double s = 0;
      for (int64_t d = i; d < D; ++d) s += Y[d + j * D] * Y[d + i * D];
      w[j] = -tau[i] * s;
    }
    for (int64_t r = 0; r < i; ++r) {
      double s = 0;
      for (int64_t j = r; j < i; ++j) s += Tw[r + j * k] * w[j];
      Tw[r + i * k] = s;
    }
    Tw[i + i * k] = tau[i];
  }
  // S = I + R·Dm·Rᵀ, then its upper Cholesky factor V (the upper triangle of S is read, as Symmetric(S) does) and V⁻¹
  std::vector<double> RD((size_t)(k * k), 0.0), S((size_t)(k * k), 0.0), V((size_t)(k * k), 0.0), Vi((size_t)(k * k), 0.0);
  for (int64_t i = 0; i < k; ++i)
    for (int64_t j = 0; j < k; ++j) {
      double s = 0;
      for (int64_t l = 0; l < k; ++l) s += R[i + l * k] * (double)hD[l + j * k];
      RD[i + j * k] = s;
    }
  for (int64_t i = 0; i < k; ++i)
    for (int64_t j = 0; j < k; ++j) {
      double s = 0;
      for (int64_t l = 0; l < k; ++l) s += RD[i + l * k] * R[j + l * k];
      S[i + j * k] = s + (i == j ? 1.0 : 0.0);
    }
  for (int64_t j = 0; j < k; ++j) {
    for (int64_t i = 0; i <= j; ++i) {
      double s = S[i + j * k];
      for (int64_t l = 0; l < i; ++l) s -= V[l + i * k] * V[l + j * k];
      if (i == j) {
        if (!(s > 0)) return fail(c, AHMC_ERR_ARGUMENT, "PosDefException: I + R·Dm·Rᵀ is not positive definite (M⁻¹ = A + B·Dm·Bᵀ is not)");
        V[i + j * k] = std::sqrt(s);
      } else {
        V[i + j * k] = s / V[i + i * k];
      }
    }
  }
  for (int64_t j = 0; j < k; ++j)
    for (int64_t i = j; i >= 0; --i) {
      double s = (i == j) ? 1.0 : 0.0;
      for (int64_t l = i + 1; l <= j; ++l) s -= V[i + l * k] * Vi[l + j * k];
      Vi[i + j * k] = s / V[i + i * k];
    }
  // one slab: A, 1/√A, B, Dm, Y, Tw, V⁻¹, each starting on a 256-byte boundary
  const int64_t sizes[7] = {D, D, D * k, k * k, D * k, k * k, k * k};
  int64_t off[7], tot = 0;
  for (int i = 0; i < 7; ++i) {
    off[i] = tot;
    tot += (sizes[i] + 31) / 32 * 32;
  }
  std::vector<T> h((size_t)tot, T(0));
  for (int64_t d = 0; d < D; ++d) {
    h[off[0] + d] = hA[d];
    h[off[1] + d] = (T)(1 / std::sqrt((double)hA[d]));
  }
  for (int64_t i = 0; i < D * k; ++i) { h[off[2] + i] = hB[i]; h[off[4] + i] = (T)Y[i]; }
  for (int64_t i = 0; i < k * k; ++i) { h[off[3] + i] = hD[i]; h[off[5] + i] = (T)Tw[i]; h[off[6] + i] = (T)Vi[i]; }
  HIPCHK(hipStreamSynchronize(c->stream));
  if ((size_t)tot > c->ru_cap) {
    if (c->ru_buf) HIPCHK(hipFree(c->ru_buf));
    c->ru_buf = nullptr;
    c->ru_cap = 0;
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&c->ru_buf), sizeof(T) * (size_t)tot));
    c->ru_cap = (size_t)tot;
  }
  HIPCHK(hipMemcpy(c->ru_buf, h.data(), sizeof(T) * (size_t)tot, hipMemcpyHostToDevice));
  for (int i = 0; i < 7; ++i) c->ru_off[i] = off[i];
  c->ru_k = (int)k;
  c->metric_kind = AHMC_METRIC_RANK_UPDATE_CTX;
  c->minv_per_chain = false;
  c->minv_n = 0;
  c->dn_fused_ok = false;  // (dn_refresh_fused: the M⁻¹·P product is the dense metric's)
  return AHMC_OK;
}

template <class T>
int ru_get_metric(Ctx<T>* c, void* A, void* B, void* Dm, int64_t* k) {
  if (c->metric_kind != AHMC_METRIC_RANK_UPDATE_CTX) return fail(c, AHMC_ERR_ARGUMENT, "get_metric_rank_update: the context's metric is not a RankUpdateEuclideanMetric");
  const int64_t D = c->D, kk = c->ru_k;
  if (k) *k = kk;
  if (A) HIPCHK(hipMemcpyAsync(A, c->ru_buf + c->ru_off[0], sizeof(T) * D, hipMemcpyDefault, c->stream));
  if (B && kk > 0) HIPCHK(hipMemcpyAsync(B, c->ru_buf + c->ru_off[2], sizeof(T) * D * kk, hipMemcpyDefault, c->stream));
  if (Dm && kk > 0) HIPCHK(hipMemcpyAsync(Dm, c->ru_buf + c->ru_off[3], sizeof(T) * kk * kk, hipMemcpyDefault, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return AHMC_OK;
}
