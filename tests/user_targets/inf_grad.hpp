// A user log-density for ahmc_set_target_plugin (contract: include/ahmc_user_target.h) whose VALUE stays finite where its
// GRADIENT does not: the isotropic Gaussian of iso_gauss.hpp, except that ∂ℓπ/∂θ₀ is +Inf once |θ₀| exceeds params[0].
// The reference's isfinite(z) asks for finite gradients too; tests/test_user_targets.py holds the coupled early exit to it.
namespace ahmc_user {
template <class T, int G, int E>
__device__ __forceinline__ T logdensity(const T* params, int D, const T (&th)[E], T (&grad_neg)[E], int lane, int d0) {
  T ss = 0;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    ss += th[e] * th[e];
    grad_neg[e] = th[e];
  }
  if (d0 == 0 && fabs(th[0]) > params[0]) grad_neg[0] = -(T)__builtin_inf();  // −∂ℓπ/∂θ₀ = −Inf
  T part = -ss / 2;
  if (lane == 0) part -= (T)D * (T)1.8378770664093454835606594728112 / 2;
  return part;
}
}  // namespace ahmc_user
