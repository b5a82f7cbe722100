// ahmc_lowrank_adapt_host.hpp — host side of the low-rank mass-matrix adaptor (include/ahmc_lowrank_adapt.h; kernels:
// ahmc_lowrank_adapt.hpp; definition: advancedhmc.jl_amd/rank_update.py lowrank_*).  Included by ahmc_api.hip after
// ahmc_rank_update_host.hpp: a fit ends in ru_set_metric, the path of ahmc_set_metric_rank_update.
// The push runs on the device once per adapting transition; the fit is linear algebra at size ℓ <= 40 plus O(D·ℓ²) on the host, in
// double, once per window (AHMC_ADAPT_STAN) or per transition (the other kinds), as dn_cov_update's Cholesky factorization is.
#pragma once

// the adaptor's device arrays inside its slab (doubles)
template <class T>
struct LRBufs {
  double *mu, *m2, *s0, *mb, *Z, *Om, *W, *cs, *Tm, *P;
};
template <class T>
LRBufs<T> lr_bufs(const Ctx<T>* c) {
  const int64_t D = c->D, L = c->lr.ell;
  LRBufs<T> b;
  double* p = c->lr.buf;
  auto take = [&](int64_t n) { double* q = p; p += (n + 31) / 32 * 32; return q; };
  b.mu = take(D); b.m2 = take(D); b.s0 = take(D); b.mb = take(D);
  b.Z = take(D * L); b.Om = take(D * L); b.W = take(D * L);
  b.cs = take((int64_t)LR_SLICES * D);
  b.Tm = take(L * (c->N + 1));
  b.P = take((int64_t)lr_slices(D) * (lr_bucket((int)L) + 1) * D);
  return b;
}
template <class T>
size_t lr_buf_elems(const Ctx<T>* c) {
  const int64_t D = c->D, L = c->lr.ell;
  int64_t tot = 0;
  for (int64_t n : {D, D, D, D, D * L, D * L, D * L, (int64_t)LR_SLICES * D, L * (c->N + 1), (int64_t)lr_slices(D) * (lr_bucket((int)L) + 1) * D})
    tot += (n + 31) / 32 * 32;
  return (size_t)tot;
}

// W = Ω / s₀ (after Ω or s₀ changed)
template <class T>
int lr_refresh_w(Ctx<T>* c) {
  const LRBufs<T> b = lr_bufs(c);
  const int64_t tot = c->D * c->lr.ell;
  hipLaunchKernelGGL(k_lr_scale, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, b.Om, b.s0, b.W, (int)c->D, c->lr.ell);
  HIPCHK(hipGetLastError());
  return AHMC_OK;
}

// columns j0 … ℓ of Ω ← fresh normals, draw `draw` of the adaptor's stream
template <class T>
int lr_fresh_normals(Ctx<T>* c, int j0, uint32_t draw) {
  if (j0 >= c->lr.ell) return AHMC_OK;
  const LRBufs<T> b = lr_bufs(c);
  const int64_t tot = (c->D + 1) / 2 * (c->lr.ell - j0);
  hipLaunchKernelGGL(k_lr_normals, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, b.Om, (int)c->D, j0, c->lr.ell, (uint32_t)c->lr.seed,
                     (uint32_t)(c->lr.seed >> 32), draw);
  HIPCHK(hipGetLastError());
  return AHMC_OK;
}

template <class T>
int lr_zero_window(Ctx<T>* c) {
  const LRBufs<T> b = lr_bufs(c);
  HIPCHK(hipMemsetAsync(b.mu, 0, sizeof(double) * c->D, c->stream));
  HIPCHK(hipMemsetAsync(b.m2, 0, sizeof(double) * c->D, c->stream));
  HIPCHK(hipMemsetAsync(b.Z, 0, sizeof(double) * c->D * c->lr.ell, c->stream));
  c->lr.n = 0;
  return AHMC_OK;
}

// ahmc_lowrank_adaptor_init: the checks, the metric as a rank-k rank update, the estimator's first window, then the plain adaptor_init
template <class T>
int adaptor_init(Ctx<T>* c, int kind, double delta, int ib, int tb, int ws);

template <class T>
int lr_adaptor_init(Ctx<T>* c, int kind, double delta, int ib, int tb, int ws, int64_t k, int64_t oversample, uint64_t seed) {
  const int64_t D = c->D;
  if (kind != AHMC_ADAPT_MASSMATRIX && kind != AHMC_ADAPT_NAIVE && kind != AHMC_ADAPT_STAN)
    return fail(c, AHMC_ERR_ARGUMENT, "lowrank_adaptor_init: kind must be AHMC_ADAPT_MASSMATRIX, AHMC_ADAPT_NAIVE or AHMC_ADAPT_STAN");
  if (c->metric_kind == AHMC_METRIC_DENSE)
    return fail(c, AHMC_ERR_UNSUPPORTED, "lowrank_adaptor_init: DenseEuclideanMetric adapts by WelfordCov (ahmc_adaptor_init): set a Unit, a shared Diag or a "
                                         "RankUpdateEuclideanMetric first");
  if (c->metric_kind == AHMC_METRIC_DIAG && c->minv_per_chain)
    return fail(c, AHMC_ERR_UNSUPPORTED, "lowrank_adaptor_init: the low-rank adaptor fits ONE M⁻¹ shared by all chains: set a (D,) DiagEuclideanMetric, not (D, N)");
  if (c->comm)
    return fail(c, AHMC_ERR_UNSUPPORTED, "lowrank_adaptor_init: a communicator is set and the low-rank fit is not pooled across ranks");
  if (k < 1 || k > D || k > RU_MAX_K)
    return fail(c, AHMC_ERR_ARGUMENT, "DimensionMismatch: lowrank_adaptor_init needs 1 <= k <= min(D, AHMC_RANK_UPDATE_MAX_K = " + std::to_string(RU_MAX_K) +
                                          "); got k = " + std::to_string(k) + " at D = " + std::to_string(D));
  if (oversample < 0 || k + oversample > LR_MAX_ELL)
    return fail(c, AHMC_ERR_ARGUMENT, "lowrank_adaptor_init: needs oversample >= 0 and k + oversample <= AHMC_LOWRANK_MAX_ELL = " + std::to_string(LR_MAX_ELL) +
                                          "; got k + oversample = " + std::to_string(k + oversample));
  if (c->metric_kind == AHMC_METRIC_RANK_UPDATE_CTX && c->ru_k > k)
    return fail(c, AHMC_ERR_ARGUMENT, "DimensionMismatch: lowrank_adaptor_init: the context's RankUpdateEuclideanMetric has rank " + std::to_string(c->ru_k) +
                                          ", more than k = " + std::to_string(k));
  // the metric as (A, B, Dm) of rank k, and s₀ = √diag(M⁻¹)
  std::vector<T> hA((size_t)D, T(1)), hB((size_t)(D * k), T(0)), hD((size_t)(k * k), T(0));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->metric_kind == AHMC_METRIC_DIAG) {
    HIPCHK(hipMemcpy(hA.data(), c->minv, sizeof(T) * D, hipMemcpyDeviceToHost));
  } else if (c->metric_kind == AHMC_METRIC_RANK_UPDATE_CTX) {
    const int64_t k0 = c->ru_k;
    std::vector<T> d0((size_t)(k0 * k0));
    HIPCHK(hipMemcpy(hA.data(), c->ru_buf + c->ru_off[0], sizeof(T) * D, hipMemcpyDeviceToHost));
    if (k0 > 0) {
      HIPCHK(hipMemcpy(hB.data(), c->ru_buf + c->ru_off[2], sizeof(T) * D * k0, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(d0.data(), c->ru_buf + c->ru_off[3], sizeof(T) * k0 * k0, hipMemcpyDeviceToHost));
    }
    for (int64_t j = 0; j < k0; ++j)
      for (int64_t i = 0; i < k0; ++i) hD[i + j * k] = d0[i + j * k0];
  }
  std::vector<double> s0((size_t)D);
  for (int64_t d = 0; d < D; ++d) {
    double v = (double)hA[d];
    for (int64_t i = 0; i < k; ++i)
      for (int64_t j = 0; j < k; ++j) v += (double)hB[d + i * D] * (double)hD[i + j * k] * (double)hB[d + j * D];
    if (!(std::isfinite(v) && v > 0)) return fail(c, AHMC_ERR_ARGUMENT, "lowrank_adaptor_init: diag(M⁻¹) of the context's metric is not finite and > 0");
    s0[d] = std::sqrt(v);
  }
  int rc = ru_set_metric(c, hA.data(), hB.data(), hD.data(), k);
  if (rc) return rc;
  invalidate_schedule(c);
  c->lr.on = true;
  c->lr.k = (int)k;
  c->lr.ell = (int)std::min<int64_t>(D, k + oversample);
  c->lr.seed = seed;
  c->lr.n_fits = 0;
  c->lr.have_V = false;
  const size_t need = lr_buf_elems(c);
  if (need > c->lr.cap) {
    if (c->lr.buf) HIPCHK(hipFree(c->lr.buf));
    c->lr.buf = nullptr;
    c->lr.cap = 0;
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&c->lr.buf), sizeof(double) * need));
    c->lr.cap = need;
  }
  const LRBufs<T> b = lr_bufs(c);
  HIPCHK(hipMemcpy(b.s0, s0.data(), sizeof(double) * D, hipMemcpyHostToDevice));
  if ((rc = lr_zero_window(c))) return rc;
  if ((rc = lr_fresh_normals(c, 0, 0))) return rc;
  if ((rc = lr_refresh_w(c))) return rc;
  rc = adaptor_init(c, kind, delta, ib, tb, ws);
  if (rc) c->lr.on = false;
  return rc;
}

// one batch of positions th (D, N) merged into the window
template <class T>
int lr_push(Ctx<T>* c, const T* th) {
  const LRBufs<T> b = lr_bufs(c);
  const int D = (int)c->D, ell = c->lr.ell;
  const int64_t N = c->N;
  const unsigned db = (unsigned)((D + 255) / 256);
  hipLaunchKernelGGL((k_lr_colsum_partial<T>), dim3(db, LR_SLICES), dim3(256), 0, c->stream, th, b.cs, D, N);
  hipLaunchKernelGGL(k_lr_colsum_final, dim3(db), dim3(256), 0, c->stream, (const double*)b.cs, b.mb, D, N);
  const int nsl = lr_slices(D);
  const double n = (double)c->lr.n, nb = (double)N;
  const double f = n * nb / (n + nb), g = nb / (n + nb);
  switch (lr_bucket(ell)) {
#define AHMC_LR_PUSH(LB)                                                                                                                              \
  case LB:                                                                                                                                            \
    hipLaunchKernelGGL((k_lr_project<T, LB>), dim3((unsigned)((N + lr_cpw(LB) - 1) / lr_cpw(LB) + 1)), dim3(LR_THREADS), 0, c->stream, th,          \
                       (const double*)b.W, (const double*)b.mb, (const double*)b.mu, b.Tm, D, N, ell);                                              \
    hipLaunchKernelGGL((k_lr_accumulate<T, LB>), dim3((unsigned)((D + LR_ROWS - 1) / LR_ROWS), (unsigned)nsl), dim3(LR_ROWS), 0, c->stream, th,     \
                       (const double*)b.mb, (const double*)b.Tm, b.P, D, N, ell);                                                                   \
    hipLaunchKernelGGL((k_lr_merge<LB>), dim3(db), dim3(256), 0, c->stream, (const double*)b.P, (const double*)b.Tm, (const double*)b.mb, b.Z, b.m2, \
                       b.mu, D, N, ell, nsl, f, g);                                                                                                 \
    break
    AHMC_LR_PUSH(8); AHMC_LR_PUSH(16); AHMC_LR_PUSH(40);
#undef AHMC_LR_PUSH
  }
  HIPCHK(hipGetLastError());
  c->lr.n += N;
  return AHMC_OK;
}

// eigenpairs of the symmetric (m, m) matrix G (column-major, overwritten): cyclic Jacobi; w unsorted, Q's columns the eigenvectors
inline void lr_jacobi_eig(std::vector<double>& G, int m, std::vector<double>& w, std::vector<double>& Q) {
  Q.assign((size_t)m * m, 0.0);
  for (int i = 0; i < m; ++i) Q[i + (size_t)i * m] = 1;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0, diag = 0;
    for (int j = 0; j < m; ++j)
      for (int i = 0; i < m; ++i) (i == j ? diag : off) += G[i + (size_t)j * m] * G[i + (size_t)j * m];
    if (!(off > 1e-32 * diag)) break;
    for (int p = 0; p < m - 1; ++p)
      for (int q = p + 1; q < m; ++q) {
        const double apq = G[p + (size_t)q * m];
        if (apq == 0) continue;
        const double theta = (G[q + (size_t)q * m] - G[p + (size_t)p * m]) / (2 * apq);
        const double t = std::copysign(1.0, theta) / (std::fabs(theta) + std::sqrt(theta * theta + 1));
        const double cs = 1 / std::sqrt(t * t + 1), sn = t * cs;
        for (int i = 0; i < m; ++i) {  // columns p, q
          const double gp = G[i + (size_t)p * m], gq = G[i + (size_t)q * m];
          G[i + (size_t)p * m] = cs * gp - sn * gq;
          G[i + (size_t)q * m] = sn * gp + cs * gq;
        }
        for (int i = 0; i < m; ++i) {  // rows p, q
          const double gp = G[p + (size_t)i * m], gq = G[q + (size_t)i * m];
          G[p + (size_t)i * m] = cs * gp - sn * gq;
          G[q + (size_t)i * m] = sn * gp + cs * gq;
        }
        for (int i = 0; i < m; ++i) {
          const double qp = Q[i + (size_t)p * m], qq = Q[i + (size_t)q * m];
          Q[i + (size_t)p * m] = cs * qp - sn * qq;
          Q[i + (size_t)q * m] = sn * qp + cs * qq;
        }
      }
  }
  w.resize((size_t)m);
  for (int i = 0; i < m; ++i) w[i] = G[i + (size_t)i * m];
}

// singular values (descending) and left singular vectors of the (m, m) matrix R (column-major), R = U·Σ·Vᵀ: one-sided Jacobi
// (Hestenes) orthogonalises the columns of M = Rᵀ by plane rotations from the right; at convergence M·J = V·Σ, so the accumulated
// rotations J are U and the column norms are σ.  RᵀR is never formed.
inline void lr_jacobi_svd_left(const std::vector<double>& R, int m, std::vector<double>& sig, std::vector<double>& U) {
  std::vector<double> M((size_t)m * m), J((size_t)m * m, 0.0);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) M[j + (size_t)i * m] = R[i + (size_t)j * m];
  for (int i = 0; i < m; ++i) J[i + (size_t)i * m] = 1;
  for (int sweep = 0; sweep < 60; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < m - 1; ++p)
      for (int q = p + 1; q < m; ++q) {
        double a = 0, b = 0, g = 0;
        for (int i = 0; i < m; ++i) {
          a += M[i + (size_t)p * m] * M[i + (size_t)p * m];
          b += M[i + (size_t)q * m] * M[i + (size_t)q * m];
          g += M[i + (size_t)p * m] * M[i + (size_t)q * m];
        }
        if (g == 0 || std::fabs(g) <= 1e-16 * std::sqrt(a * b)) continue;
        rotated = true;
        const double zeta = (b - a) / (2 * g);
        const double t = std::copysign(1.0, zeta) / (std::fabs(zeta) + std::sqrt(zeta * zeta + 1));
        const double cs = 1 / std::sqrt(t * t + 1), sn = t * cs;
        for (int i = 0; i < m; ++i) {
          const double mp = M[i + (size_t)p * m], mq = M[i + (size_t)q * m];
          M[i + (size_t)p * m] = cs * mp - sn * mq;
          M[i + (size_t)q * m] = sn * mp + cs * mq;
          const double jp = J[i + (size_t)p * m], jq = J[i + (size_t)q * m];
          J[i + (size_t)p * m] = cs * jp - sn * jq;
          J[i + (size_t)q * m] = sn * jp + cs * jq;
        }
      }
    if (!rotated) break;
  }
  std::vector<std::pair<double, int>> order((size_t)m);
  for (int j = 0; j < m; ++j) {
    double a = 0;
    for (int i = 0; i < m; ++i) a += M[i + (size_t)j * m] * M[i + (size_t)j * m];
    order[j] = {std::sqrt(a), j};
  }
  std::stable_sort(order.begin(), order.end(), [](const std::pair<double, int>& x, const std::pair<double, int>& y) { return x.first > y.first; });
  sig.resize((size_t)m);
  U.assign((size_t)m * m, 0.0);
  for (int j = 0; j < m; ++j) {
    sig[j] = order[j].first;
    for (int i = 0; i < m; ++i) U[i + (size_t)j * m] = J[i + (size_t)order[j].second * m];
  }
}

// lowrank_fit: (A, B, Dm) of the window → the context's metric; the eigenvectors stay in c->lr.V for lr_restart.  Skipped while the
// window holds fewer than wv_nmin draws (as dn_cov_update).
template <class T>
int lr_fit(Ctx<T>* c) {
  const int64_t n = c->lr.n;
  if (n < c->wv_nmin || n < 2) return AHMC_OK;
  const int64_t D = c->D;
  const int k = c->lr.k, L = c->lr.ell;
  const LRBufs<T> b = lr_bufs(c);
  std::vector<double> m2((size_t)D), s0((size_t)D), Z((size_t)(D * L)), Om((size_t)(D * L));
  HIPCHK(hipMemcpyAsync(m2.data(), b.m2, sizeof(double) * D, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(s0.data(), b.s0, sizeof(double) * D, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(Z.data(), b.Z, sizeof(double) * D * L, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(Om.data(), b.Om, sizeof(double) * D * L, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  const double nm1 = (double)(n - 1);
  // 1. c = diag(C_s), Y = C_s·Ω (in Z's storage)
  std::vector<double> cd((size_t)D);
  double csum = 0;
  for (int64_t d = 0; d < D; ++d) {
    cd[d] = m2[d] / nm1 / (s0[d] * s0[d]);
    csum += cd[d];
  }
  std::vector<double>& Y = Z;
  for (int j = 0; j < L; ++j)
    for (int64_t d = 0; d < D; ++d) Y[d + j * D] = Y[d + j * D] / nm1 / s0[d];
  // 2. G = sym(ΩᵀY), its eigenpairs, F = Y·Q·w^(−½) over the kept ones
  std::vector<double> G((size_t)L * L), w, Q;
  for (int i = 0; i < L; ++i)
    for (int j = 0; j < L; ++j) {
      double s = 0;
      for (int64_t d = 0; d < D; ++d) s += Om[d + i * D] * Y[d + j * D];
      G[i + (size_t)j * L] = s;
    }
  for (int i = 0; i < L; ++i)
    for (int j = i + 1; j < L; ++j) G[i + (size_t)j * L] = G[j + (size_t)i * L] = (G[i + (size_t)j * L] + G[j + (size_t)i * L]) / 2;
  lr_jacobi_eig(G, L, w, Q);
  double wmax = 0;
  for (int i = 0; i < L; ++i) wmax = std::max(wmax, w[i]);
  std::vector<int> keep;
  for (int i = 0; i < L; ++i)
    if (w[i] > 1e-12 * wmax) keep.push_back(i);
  const int r = (int)keep.size();
  std::vector<double> lam((size_t)k, 0.0), V((size_t)(D * k), 0.0);
  if (r > 0) {
    std::vector<double> F((size_t)(D * r));
    for (int a = 0; a < r; ++a) {
      const double isw = 1 / std::sqrt(w[keep[a]]);
      for (int64_t d = 0; d < D; ++d) {
        double s = 0;
        for (int j = 0; j < L; ++j) s += Y[d + j * D] * Q[j + (size_t)keep[a] * L];
        F[d + a * D] = s * isw;
      }
    }
    // 3. thin SVD of F: Householder QR (dgeqr2's conventions, as ru_set_metric), Jacobi SVD of R, V = H₁⋯H_r·[U_R(:, 1:k); 0]
    std::vector<double> tau((size_t)r, 0.0);
    for (int j = 0; j < r; ++j) {
      double* col = F.data() + (int64_t)j * D;
      const double alpha = col[j];
      double xn = 0;
      for (int64_t i = j + 1; i < D; ++i) xn = std::hypot(xn, col[i]);
      if (xn != 0) {
        const double beta = -std::copysign(std::hypot(alpha, xn), alpha);
        tau[j] = (beta - alpha) / beta;
        const double scal = 1 / (alpha - beta);
        for (int64_t i = j + 1; i < D; ++i) col[i] *= scal;
        col[j] = beta;
      }
      if (tau[j] == 0) continue;
      for (int cc = j + 1; cc < r; ++cc) {
        double* x = F.data() + (int64_t)cc * D;
        double s = x[j];
        for (int64_t i = j + 1; i < D; ++i) s += col[i] * x[i];
        s *= tau[j];
        x[j] -= s;
        for (int64_t i = j + 1; i < D; ++i) x[i] -= s * col[i];
      }
    }
    std::vector<double> Rm((size_t)r * r, 0.0), sig, Ur;
    for (int j = 0; j < r; ++j)
      for (int i = 0; i <= j; ++i) Rm[i + (size_t)j * r] = F[i + (int64_t)j * D];
    lr_jacobi_svd_left(Rm, r, sig, Ur);
    const int kk = std::min(k, r);
    for (int a = 0; a < kk; ++a) {
      lam[a] = sig[a] * sig[a];
      double* v = V.data() + (int64_t)a * D;
      for (int i = 0; i < r; ++i) v[i] = Ur[i + (size_t)a * r];
      for (int j = r - 1; j >= 0; --j) {  // v ← H_j·v
        if (tau[j] == 0) continue;
        const double* col = F.data() + (int64_t)j * D;
        double s = v[j];
        for (int64_t i = j + 1; i < D; ++i) s += col[i] * v[i];
        s *= tau[j];
        v[j] -= s;
        for (int64_t i = j + 1; i < D; ++i) v[i] -= s * col[i];
      }
    }
  }
  // 4.–6. the residual level, the diagonal, Stan's shrinkage
  double lsum = 0;
  for (int a = 0; a < k; ++a) lsum += lam[a];
  const double lres = D > k ? std::max((csum - lsum) / (double)(D - k), 0.0) : 0.0;
  std::vector<double> dm((size_t)k);
  for (int a = 0; a < k; ++a) dm[a] = std::max(lam[a] - lres, 0.0);
  const double sh = (double)n / ((double)n + 5), reg = 1e-3 * (5 / ((double)n + 5));
  std::vector<T> hA((size_t)D), hB((size_t)(D * k)), hD((size_t)(k * k), T(0));
  for (int64_t d = 0; d < D; ++d) {
    double low = 0;
    for (int a = 0; a < k; ++a) low += V[d + (int64_t)a * D] * V[d + (int64_t)a * D] * dm[a];
    const double dd = std::max(cd[d] - low, 1e-3 * cd[d]);
    hA[d] = (T)(s0[d] * s0[d] * (sh * dd + reg));
    for (int a = 0; a < k; ++a) hB[d + (int64_t)a * D] = (T)(s0[d] * V[d + (int64_t)a * D]);
  }
  for (int a = 0; a < k; ++a) hD[a + (size_t)a * k] = (T)(sh * dm[a]);
  c->lr.V.swap(V);
  c->lr.have_V = true;
  invalidate_schedule(c);
  return ru_set_metric(c, hA.data(), hB.data(), hD.data(), (int64_t)k);
}

// lowrank_restart: the next window
template <class T>
int lr_restart(Ctx<T>* c) {
  const LRBufs<T> b = lr_bufs(c);
  const int64_t D = c->D;
  int rc;
  if (c->lr.have_V) {
    if (c->lr.n >= 2) {
      std::vector<double> m2((size_t)D), s0((size_t)D);
      HIPCHK(hipMemcpyAsync(m2.data(), b.m2, sizeof(double) * D, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipMemcpyAsync(s0.data(), b.s0, sizeof(double) * D, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      for (int64_t d = 0; d < D; ++d) {
        const double sd = std::sqrt(m2[d] / (double)(c->lr.n - 1));
        if (sd > 0) s0[d] = sd;
      }
      HIPCHK(hipMemcpy(b.s0, s0.data(), sizeof(double) * D, hipMemcpyHostToDevice));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(b.Om, c->lr.V.data(), sizeof(double) * D * c->lr.k, hipMemcpyHostToDevice));
    if ((rc = lr_fresh_normals(c, c->lr.k, (uint32_t)(c->lr.n_fits + 1)))) return rc;
    if ((rc = lr_refresh_w(c))) return rc;
    c->lr.have_V = false;
  }
  c->lr.n_fits += 1;
  return lr_zero_window(c);
}

template <class T>
int lr_get_state(Ctx<T>* c, ahmc_lowrank_state* s, double* mu, double* m2, double* Z, double* s0, double* Om) {
  if (!c->lr.on) return fail(c, AHMC_ERR_STATE, "lowrank_get_state: the context has no low-rank adaptor (ahmc_lowrank_adaptor_init)");
  if (!s) return fail(c, AHMC_ERR_ARGUMENT, "lowrank_get_state: state is NULL");
  s->k = c->lr.k; s->ell = c->lr.ell; s->seed = c->lr.seed; s->n = c->lr.n; s->n_fits = c->lr.n_fits;
  const LRBufs<T> b = lr_bufs(c);
  const size_t D = (size_t)c->D, DL = D * (size_t)c->lr.ell;
  if (mu) HIPCHK(hipMemcpyAsync(mu, b.mu, sizeof(double) * D, hipMemcpyDefault, c->stream));
  if (m2) HIPCHK(hipMemcpyAsync(m2, b.m2, sizeof(double) * D, hipMemcpyDefault, c->stream));
  if (Z) HIPCHK(hipMemcpyAsync(Z, b.Z, sizeof(double) * DL, hipMemcpyDefault, c->stream));
  if (s0) HIPCHK(hipMemcpyAsync(s0, b.s0, sizeof(double) * D, hipMemcpyDefault, c->stream));
  if (Om) HIPCHK(hipMemcpyAsync(Om, b.Om, sizeof(double) * DL, hipMemcpyDefault, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return AHMC_OK;
}

template <class T>
int lr_set_state(Ctx<T>* c, const ahmc_lowrank_state* s, const double* mu, const double* m2, const double* Z, const double* s0, const double* Om) {
  if (!c->lr.on) return fail(c, AHMC_ERR_STATE, "lowrank_set_state: the context has no low-rank adaptor (ahmc_lowrank_adaptor_init first)");
  if (!s || !mu || !m2 || !Z || !s0 || !Om) return fail(c, AHMC_ERR_ARGUMENT, "lowrank_set_state: NULL argument");
  if (s->k != c->lr.k || s->ell != c->lr.ell)
    return fail(c, AHMC_ERR_ARGUMENT, "lowrank_set_state: the state has (k, ell) = (" + std::to_string(s->k) + ", " + std::to_string(s->ell) + "), the adaptor (" +
                                          std::to_string(c->lr.k) + ", " + std::to_string(c->lr.ell) + ")");
  if (s->n < 0 || s->n_fits < 0) return fail(c, AHMC_ERR_ARGUMENT, "lowrank_set_state: negative counter");
  const LRBufs<T> b = lr_bufs(c);
  const size_t D = (size_t)c->D, DL = D * (size_t)c->lr.ell;
  HIPCHK(hipMemcpyAsync(b.mu, mu, sizeof(double) * D, hipMemcpyDefault, c->stream));
  HIPCHK(hipMemcpyAsync(b.m2, m2, sizeof(double) * D, hipMemcpyDefault, c->stream));
  HIPCHK(hipMemcpyAsync(b.Z, Z, sizeof(double) * DL, hipMemcpyDefault, c->stream));
  HIPCHK(hipMemcpyAsync(b.s0, s0, sizeof(double) * D, hipMemcpyDefault, c->stream));
  HIPCHK(hipMemcpyAsync(b.Om, Om, sizeof(double) * DL, hipMemcpyDefault, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));  // (the sources may be pageable host buffers)
  c->lr.seed = s->seed;
  c->lr.n = s->n;
  c->lr.n_fits = s->n_fits;
  c->lr.have_V = false;
  return lr_refresh_w(c);
}
