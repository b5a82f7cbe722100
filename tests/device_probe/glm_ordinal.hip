// Device probe of tests/test_glm_ordinal.py (csrc/ahmc_glm.hpp, compiled with the engine's own flags by build.build_probe_object):
// the special functions of the ordered-logit family's gap constants as k_glm_cut calls them, element by element — E[i] = expm1(d[i]),
// (LG[i], R[i]) = glm_cut_gap(d[i]) — and the link itself on given η, so that a test sees ∂ℓ/∂a and ∂ℓ/∂b, which the engine only sums.
#include "ahmc_glm.hpp"

template <class T>
__device__ __forceinline__ void probe_gap(const T* d, T* E, T* LG, T* R, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  T lg, r;
  ahmc::glm_cut_gap(d[i], lg, r);
  E[i] = expm1(d[i]);
  LG[i] = lg;
  R[i] = r;
}
extern "C" __global__ void glm_ordinal_probe_gap_f64(const double* d, double* E, double* LG, double* R, int64_t n) { probe_gap(d, E, LG, R, n); }
extern "C" __global__ void glm_ordinal_probe_gap_f32(const float* d, float* E, float* LG, float* R, int64_t n) { probe_gap(d, E, LG, R, n); }

// glm_link_ord at η (n_obs, N) with the cutpoint table tab (3, C−1, N) of k_glm_cut: ℓ, u, da, db, each (n_obs, N)
template <class T>
__device__ __forceinline__ void probe_link(const T* y, const T* eta, const T* tab, int Cm1, int64_t n_obs, int64_t N, T* ll, T* u, T* da, T* db) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_obs * N) return;
  const int64_t row = i % n_obs, col = i / n_obs;
  const int yi = (int)y[row];
  const int ia = yi < Cm1 ? yi : Cm1 - 1, ib = yi > 0 ? yi - 1 : 0;
  const T* tc = tab + col;
  ahmc::glm_link_ord<T>(yi, Cm1, eta[i], tc[(int64_t)ia * N], tc[(int64_t)ib * N], tc[((int64_t)Cm1 + ia) * N], tc[((int64_t)2 * Cm1 + ia) * N], ll[i], u[i], da[i],
                        db[i]);
}
extern "C" __global__ void glm_ordinal_probe_link_f64(const double* y, const double* eta, const double* tab, int Cm1, int64_t n_obs, int64_t N, double* ll, double* u,
                                                      double* da, double* db) {
  probe_link(y, eta, tab, Cm1, n_obs, N, ll, u, da, db);
}
extern "C" __global__ void glm_ordinal_probe_link_f32(const float* y, const float* eta, const float* tab, int Cm1, int64_t n_obs, int64_t N, float* ll, float* u, float* da,
                                                      float* db) {
  probe_link(y, eta, tab, Cm1, n_obs, N, ll, u, da, db);
}

// The new kernels as they are, so that a test can launch them on a chain list of its choosing.
#define AHMC_PROBE_ORD_ETA(T, BN)                                                                                                        \
  template __global__ void ahmc::k_glm_eta<T, 5, BN>(const T*, const T*, const T*, T, const T*, T*, T*, int, int, int64_t, int64_t, \
                                                     const int*, T*, T*, const T*, int64_t, T*);
#define AHMC_PROBE_ORD(T)                                                                                                                 \
  AHMC_PROBE_ORD_ETA(T, 64) AHMC_PROBE_ORD_ETA(T, 16)                                                                                     \
  template __global__ void ahmc::k_glm_cut<T>(const T*, int64_t, int64_t, int, T*, int64_t, int64_t, const int*, int);                    \
  template __global__ void ahmc::k_hglm_finish_ord<T>(const T*, const T*, const T*, const T*, const T*, const T*, const ahmc::HglmTab<T>*, \
                                                      T*, T*, int, int, int, int64_t, int64_t, const int*, int, int, double, double, double, double);
AHMC_PROBE_ORD(double)
AHMC_PROBE_ORD(float)
