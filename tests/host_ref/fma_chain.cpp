// Host references of tests/test_dense_products.py.  Built by the test itself with the host compiler (-ffp-contract=off, so the
// only fused operations are the std::fma calls written here) into the build cache as its own small shared object.
//
//   fma_*        the correctly rounded fused multiply-add of the element type, element by element (checked against mpmath)
//   chain_*      Y = A·X as the k-ordered chain acc ← fma(A[i,k], X[k,j], acc), k = 0 … D−1 from acc = +0, one rounding per
//                product, in the element type: what one MFMA accumulator element goes through
//   exact_*      the same product and the companion |A|·|X| in x86 80-bit long double, of the values as stored (_ld: X in long double)
// A is column-major with leading dimension D; column j of X starts at X + j·ldx, of Y at Y + j·D.
#include <cmath>
#include <cstdint>
#include <vector>

namespace {
constexpr int64_t RB = 64;  // rows per task: a column's rows are independent, so few columns still use every thread

template <class T>
void chain(const T* A, const T* X, T* Y, int64_t D, int64_t N, int64_t ldx) {
  const int64_t nb = (D + RB - 1) / RB;
#pragma omp parallel for collapse(2) schedule(static)
  for (int64_t j = 0; j < N; ++j) {
    for (int64_t b = 0; b < nb; ++b) {
      const int64_t i0 = b * RB, i1 = i0 + RB < D ? i0 + RB : D;
      T* acc = Y + j * D;
      for (int64_t i = i0; i < i1; ++i) acc[i] = T(0);
      for (int64_t k = 0; k < D; ++k) {
        const T x = X[j * ldx + k];
        const T* a = A + k * D;
        for (int64_t i = i0; i < i1; ++i) acc[i] = std::fma(a[i], x, acc[i]);
      }
    }
  }
}

template <class T, class TX>
void exact(const T* A, const TX* X, long double* Y, long double* S, int64_t D, int64_t N, int64_t ldx) {
  const int64_t nb = (D + RB - 1) / RB;
#pragma omp parallel for collapse(2) schedule(static)
  for (int64_t j = 0; j < N; ++j) {
    for (int64_t b = 0; b < nb; ++b) {
      const int64_t i0 = b * RB, i1 = i0 + RB < D ? i0 + RB : D;
      long double* y = Y + j * D;
      long double* s = S + j * D;
      for (int64_t i = i0; i < i1; ++i) y[i] = s[i] = 0.0L;
      for (int64_t k = 0; k < D; ++k) {
        const long double x = X[j * ldx + k];
        const T* a = A + k * D;
        for (int64_t i = i0; i < i1; ++i) {
          const long double p = (long double)a[i] * x;  // (Float32: 48 bits, exact; Float64: 106 bits rounded to 64)
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
void chain_f64(const double* A, const double* X, double* Y, int64_t D, int64_t N, int64_t ldx) { chain(A, X, Y, D, N, ldx); }
void chain_f32(const float* A, const float* X, float* Y, int64_t D, int64_t N, int64_t ldx) { chain(A, X, Y, D, N, ldx); }
void exact_f64(const double* A, const double* X, long double* Y, long double* S, int64_t D, int64_t N, int64_t ldx) { exact(A, X, Y, S, D, N, ldx); }
void exact_f32(const float* A, const float* X, long double* Y, long double* S, int64_t D, int64_t N, int64_t ldx) { exact(A, X, Y, S, D, N, ldx); }
// (X itself in long double: the replay of a trajectory)
void exact_f64_ld(const double* A, const long double* X, long double* Y, long double* S, int64_t D, int64_t N, int64_t ldx) { exact(A, X, Y, S, D, N, ldx); }
void exact_f32_ld(const float* A, const long double* X, long double* Y, long double* S, int64_t D, int64_t N, int64_t ldx) { exact(A, X, Y, S, D, N, ldx); }
}
