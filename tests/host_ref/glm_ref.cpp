// Host references of tests/test_glm_target.py: the rectangular forms of tests/host_ref/fma_chain.cpp's chain / exact pair.  Built by
// the test itself with the host compiler (-ffp-contract=off, so the only fused operations are the std::fma calls written here).
//
//   fma_*     the correctly rounded fused multiply-add of the element type, element by element
//   chain_*   Y (M, N) = A[:, k0:k1] · X[k0:k1, :] as the k-ordered chain acc ← fma(A[i,k], X[k,j], acc), k = k0 … k1−1 from acc = +0, in
//             the element type: what one MFMA accumulator element goes through (η: A = X_design, K = D; a slice of Xᵀ·U: A = Xᵀ)
//   exact_*   the same product and the companion |A|·|X| in x86 80-bit long double, of the values as stored (X handed over in long double)
// A is column-major with leading dimension lda (M rows); column j of X starts at X + j·ldx, of Y at Y + j·M.
#include <cmath>
#include <cstdint>

namespace {
constexpr int64_t RB = 64;

template <class T>
void chain(const T* A, const T* X, T* Y, int64_t M, int64_t N, int64_t lda, int64_t ldx, int64_t k0, int64_t k1) {
  const int64_t nb = (M + RB - 1) / RB;
#pragma omp parallel for collapse(2) schedule(static)
  for (int64_t j = 0; j < N; ++j) {
    for (int64_t b = 0; b < nb; ++b) {
      const int64_t i0 = b * RB, i1 = i0 + RB < M ? i0 + RB : M;
      T* acc = Y + j * M;
      for (int64_t i = i0; i < i1; ++i) acc[i] = T(0);
      for (int64_t k = k0; k < k1; ++k) {
        const T x = X[j * ldx + k];
        const T* a = A + k * lda;
        for (int64_t i = i0; i < i1; ++i) acc[i] = std::fma(a[i], x, acc[i]);
      }
    }
  }
}

template <class T>
void exact(const T* A, const long double* X, long double* Y, long double* S, int64_t M, int64_t N, int64_t lda, int64_t ldx, int64_t k0, int64_t k1) {
  const int64_t nb = (M + RB - 1) / RB;
#pragma omp parallel for collapse(2) schedule(static)
  for (int64_t j = 0; j < N; ++j) {
    for (int64_t b = 0; b < nb; ++b) {
      const int64_t i0 = b * RB, i1 = i0 + RB < M ? i0 + RB : M;
      long double* y = Y + j * M;
      long double* s = S + j * M;
      for (int64_t i = i0; i < i1; ++i) y[i] = s[i] = 0.0L;
      for (int64_t k = k0; k < k1; ++k) {
        const long double x = X[j * ldx + k];
        const T* a = A + k * lda;
        for (int64_t i = i0; i < i1; ++i) {
          const long double p = (long double)a[i] * x;
          y[i] += p;
          s[i] += std::fabs(p);
        }
      }
    }
  }
}
}  // namespace

extern "C" {
void fma_f64(const double* a, const double* b, const double* c, double* out, int64_t n) {
  for (int64_t i = 0; i < n; ++i) out[i] = std::fma(a[i], b[i], c[i]);
}
void fma_f32(const float* a, const float* b, const float* c, float* out, int64_t n) {
  for (int64_t i = 0; i < n; ++i) out[i] = std::fma(a[i], b[i], c[i]);
}
void chain_f64(const double* A, const double* X, double* Y, int64_t M, int64_t N, int64_t lda, int64_t ldx, int64_t k0, int64_t k1) {
  chain(A, X, Y, M, N, lda, ldx, k0, k1);
}
void chain_f32(const float* A, const float* X, float* Y, int64_t M, int64_t N, int64_t lda, int64_t ldx, int64_t k0, int64_t k1) {
  chain(A, X, Y, M, N, lda, ldx, k0, k1);
}
void exact_f64(const double* A, const long double* X, long double* Y, long double* S, int64_t M, int64_t N, int64_t lda, int64_t ldx, int64_t k0, int64_t k1) {
  exact(A, X, Y, S, M, N, lda, ldx, k0, k1);
}
void exact_f32(const float* A, const long double* X, long double* Y, long double* S, int64_t M, int64_t N, int64_t lda, int64_t ldx, int64_t k0, int64_t k1) {
  exact(A, X, Y, S, M, N, lda, ldx, k0, k1);
}
}
