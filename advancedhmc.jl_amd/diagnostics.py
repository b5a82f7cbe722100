"""Output side of the hot path: what the callers do with the draws and the
stat arrays — `bundle_samples` (ext/AdvancedHMCMCMCChainsExt.jl:7-41), EBFMI (src/diagnosis.jl:1-3)
and an effective-sample-size estimator.

ESS: the reference never computes it itself (MCMCChains.jl does, and no reference test calls it:
parity unpinned).  Defined here as Geyer's initial-monotone-sequence estimator on the FFT
autocorrelation, per chain and dimension:  τ = −1 + 2 Σ_{t≥0} P̂_t with P̂_t = ρ̂_{2t} + ρ̂_{2t+1}
truncated at the first non-positive pair and made non-increasing;  ESS = n / τ."""
from __future__ import annotations

import numpy as np


def autocorrelation(x, axis=0):
    """normalised autocorrelation along `axis` by FFT (biased estimator, lag 0 = 1)"""
    x = np.moveaxis(np.asarray(x, dtype=np.float64), axis, 0)
    n = x.shape[0]
    xc = x - x.mean(axis=0, keepdims=True)
    m = 1 << (2 * n - 1).bit_length()
    f = np.fft.rfft(xc, n=m, axis=0)
    acov = np.fft.irfft(f * np.conj(f), n=m, axis=0)[:n] / n
    var = acov[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = acov / var
    return np.moveaxis(rho, 0, axis)


def ess(draws, axis=0):
    """Effective sample size of each series along `axis` (Geyer initial monotone sequence).
    draws: (n_draws, ...) → array of the remaining shape.  Constant series give n_draws; a series with any non-finite value
    gives NaN (as k_ess, the CPU checker and ahmc_diag_summary)."""
    x = np.moveaxis(np.asarray(draws, dtype=np.float64), axis, 0)
    n = x.shape[0]
    finite = np.isfinite(x).all(axis=0)
    with np.errstate(invalid="ignore"):
        rho = autocorrelation(np.where(finite, x, 0.0), axis=0)
    rho = np.where(np.isfinite(rho), rho, 0.0)
    npair = n // 2
    P = rho[0:2 * npair:2] + rho[1:2 * npair:2]          # P_t = ρ_2t + ρ_2t+1
    positive = np.cumprod(P > 0, axis=0).astype(bool)      # stop at the first non-positive pair
    P = np.where(positive, P, 0.0)
    P = np.minimum.accumulate(P, axis=0)                   # initial monotone sequence
    tau = -1.0 + 2.0 * P.sum(axis=0)
    tau = np.maximum(tau, 1.0 / n)
    # a series that never moved (every transition rejected) has no autocorrelation to estimate: n_draws, as k_ess and the CPU checker
    # (round 6: this function returned n² there — found by tests/test_random_configurations.py::test_random_diagnostics)
    with np.errstate(invalid="ignore"):
        still = x.max(axis=0) == x.min(axis=0)
    return np.where(finite, np.where(still, float(n), n / tau), np.nan)


def EBFMI(energies, axis=0):
    """mean((E_{i+1} − E_i)²) / var(E) per chain (src/diagnosis.jl:1-3; var with the n−1 divisor as Statistics.var)"""
    e = np.moveaxis(np.asarray(energies, dtype=np.float64), axis, 0)
    d = np.diff(e, axis=0)
    return (d * d).mean(axis=0) / e.var(axis=0, ddof=1)


INTERNALS = ("n_steps", "is_accept", "acceptance_rate", "log_density", "hamiltonian_energy", "hamiltonian_energy_error",
             "max_hamiltonian_energy_error", "tree_depth", "numerical_error", "step_size", "nom_step_size", "is_adapt")


def bundle_samples(thetas, stats, param_names=None, discard_initial=0, thinning=1):
    """The Chains-shaped bundle of ext/AdvancedHMCMCMCChainsExt.jl:7-41 as plain arrays:
    `value` (n_samples, n_params + n_internals, n_chains), `names`, `internals` (names of the stat
    columns).  `thetas`: list of (D, N) (or (D,)) draws; `stats`: list of stat dicts of `sample`."""
    th = np.stack([np.asarray(t).reshape(np.asarray(t).shape[0], -1) for t in thetas])[discard_initial::thinning]
    st = stats[discard_initial::thinning]
    n, D, N = th.shape
    names = list(param_names) if param_names is not None else [f"param_{i + 1}" for i in range(D)]
    if len(names) != D:
        raise ValueError("param_names must have one entry per dimension")
    internals = [k for k in INTERNALS if st and k in st[0]]
    cols = [np.stack([np.broadcast_to(np.asarray(s[k], dtype=np.float64), (N,)) for s in st]) for k in internals]
    value = np.concatenate([th] + [c[:, None, :] for c in cols], axis=1) if cols else th
    return {"value": value, "names": names + internals, "params": names, "internals": internals}


# ---- MCMCChains' `summarystats` columns: rank-normalised split-chain R̂ and bulk / tail / basic ESS ------------------------------
# Vehtari, Gelman, Simpson, Carpenter & Bürkner (2021), "Rank-normalization, folding, and localization: an improved R̂", Bayesian
# Analysis 16(2).  This is the host mirror of ahmc_diag_summary (include/ahmc_diag.h, csrc/ahmc_diag.hpp) and the definition the
# device is tested against; bit-level agreement with MCMCDiagnosticTools.jl is not claimed.
SUMMARY_NAMES = ("mean", "std", "mcse", "ess_bulk", "ess_tail", "rhat", "ess_basic", "rhat_bulk", "rhat_tail")

_A = (3.3871328727963666080e+0, 1.3314166789178437745e+2, 1.9715909503065514427e+3, 1.3731693765509461125e+4,
      4.5921953931549871457e+4, 6.7265770927008700853e+4, 3.3430575583588128105e+4, 2.5090809287301226727e+3)
_B = (1.0, 4.2313330701600911252e+1, 6.8718700749205790830e+2, 5.3941960214247511077e+3, 2.1213794301586595867e+4,
      3.9307895800092710610e+4, 2.8729085735721942674e+4, 5.2264952788528545610e+3)
_C = (1.42343711074968357734e+0, 4.63033784615654529590e+0, 5.76949722146069140550e+0, 3.64784832476320460504e+0,
      1.27045825245236838258e+0, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4)
_D = (1.0, 2.05319162663775882187e+0, 1.67638483018380384940e+0, 6.89767334985100004550e-1, 1.48103976427480074590e-1,
      1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9)
_E = (6.65790464350110377720e+0, 5.46378491116411436990e+0, 1.78482653991729133580e+0, 2.96560571828504891230e-1,
      2.65321895265761230930e-2, 1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7)
_F = (1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2, 7.86869131145613259100e-4,
      1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15)


def _horner(c, r):
    v = c[7] * r + c[6]
    for k in (5, 4, 3, 2, 1):
        v = v * r + c[k]
    return v * r + c[0]


def ndtri(p):
    """Φ⁻¹(p), Wichura's AS241 (PPND16) in numpy: the same operations in the same order as the device's ppnd16"""
    p = np.asarray(p, dtype=np.float64)
    q = p - 0.5
    with np.errstate(divide="ignore", invalid="ignore"):
        r0 = 0.180625 - q * q
        central = q * _horner(_A, r0) / _horner(_B, r0)
        r = np.where(q < 0, p, 1.0 - p)
        r = np.sqrt(-np.log(r))
        r1 = r - 1.6
        mid = _horner(_C, r1) / _horner(_D, r1)
        r2 = r - 5.0
        far = _horner(_E, r2) / _horner(_F, r2)
        tail = np.where(r <= 5.0, mid, far)
        tail = np.where(np.isfinite(r), tail, np.inf)
    return np.where(np.abs(q) <= 0.425, central, np.where(q < 0, -tail, tail))


def _split_chains(draws):
    """(K, D, N) → (D, 2N, ⌊K/2⌋): split chain 2c = the first ⌊K/2⌋ draws of chain c, 2c + 1 the last ⌊K/2⌋ (the middle draw of an
    odd K dropped); widened to double, −0.0 made +0.0"""
    x = np.asarray(draws)
    K, D, N = x.shape
    n = K // 2
    y = np.stack([np.moveaxis(x[:n], 0, -1), np.moveaxis(x[K - n:], 0, -1)], axis=2)  # (D, N, 2, n)
    return y.reshape(D, 2 * N, n).astype(np.float64) + 0.0


def _average_ranks(v):
    """average ranks 1…S along the last axis, tied values sharing the mean of their ranks"""
    order = np.argsort(v, axis=-1, kind="stable")
    s = np.take_along_axis(v, order, axis=-1)
    S = v.shape[-1]
    pos = np.broadcast_to(np.arange(S), v.shape)
    new = np.ones(v.shape, dtype=bool)
    new[..., 1:] = s[..., 1:] != s[..., :-1]
    start = np.maximum.accumulate(np.where(new, pos, 0), axis=-1)
    last = np.ones(v.shape, dtype=bool)
    last[..., :-1] = new[..., 1:]
    end = S - 1 - np.maximum.accumulate(np.where(last, pos, 0)[..., ::-1] * 0 + np.where(last[..., ::-1], pos, 0), axis=-1)[..., ::-1]
    r = np.empty(v.shape, dtype=np.float64)
    np.put_along_axis(r, order, (start + end + 2) * 0.5, axis=-1)
    return r


def _z_of(v):
    S = v.shape[-1]
    return ndtri((_average_ranks(v) - 0.375) / (S + 0.25))


def _quantile7(s, p):
    """type-7 quantile of the sorted rows s, written out (np.quantile's lerp rounds differently)"""
    S = s.shape[-1]
    h = (S - 1) * p
    lo = int(np.floor(h))
    hi = min(lo + 1, S - 1)
    return s[..., lo] + (h - lo) * (s[..., hi] - s[..., lo])


def _chain_moments(y):
    """y (D, m, n) → chain means, variances (n − 1), W, var⁺, R̂"""
    m, n = y.shape[1], y.shape[2]
    cm = y.mean(axis=2)
    cv = y.var(axis=2, ddof=1)
    W = cv.mean(axis=1)
    Bn = ((cm - cm.mean(axis=1, keepdims=True)) ** 2).sum(axis=1) / (m - 1)
    varp = (n - 1) / n * W + Bn
    with np.errstate(divide="ignore", invalid="ignore"):
        rhat = np.where(W == 0, np.nan, np.sqrt(varp / W))
    return cm, W, varp, rhat


def _ess_from_rho(R, n, S, max_lag):
    """Stan's multi-chain Geyer truncation on ρ̂(t) = R[t] (R[0] unused: ρ̂(0) := 1) → ESS"""
    rho = np.zeros(n + 3)
    rho[0] = 1.0
    rho[1] = R[1]
    even, odd, t = 1.0, rho[1], 1
    cap = n - 4 if max_lag == 0 else min(n - 4, max_lag)
    while t < cap and even + odd > 0:
        even, odd = R[t + 1], R[t + 2]
        if even + odd >= 0:
            rho[t + 1], rho[t + 2] = even, odd
        t += 2
    tmax = t
    if even > 0:
        rho[tmax + 1] = even
    t = 1
    while t <= tmax - 3:
        if rho[t + 1] + rho[t + 2] > rho[t - 1] + rho[t]:
            rho[t + 1] = rho[t + 2] = (rho[t - 1] + rho[t]) / 2
        t += 2
    tau = -1.0 + 2.0 * float(np.sum(rho[0:tmax])) + rho[tmax + 1]
    return min(S / tau, S * np.log10(S))


def _ess_rhat(y, max_lag):
    """ESS (D,) and R̂ (D,) of the split chains y (D, m, n)"""
    D, m, n = y.shape
    S = m * n
    cm, W, varp, rhat = _chain_moments(y)
    c = y - cm[..., None]
    L = 1 << (2 * n - 1).bit_length()
    f = np.fft.rfft(c, n=L, axis=2)
    acov = np.fft.irfft(f * np.conj(f), n=L, axis=2)[..., :n] / n      # (D, m, n): acov_j(t)
    mac = acov.mean(axis=1)
    ess = np.full(D, np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        R = 1.0 - (W[:, None] - mac) / varp[:, None]
    for d in range(D):
        if W[d] != 0 and np.isfinite(W[d]):
            ess[d] = _ess_from_rho(R[d], n, S, max_lag)
    return ess, rhat


def summarystats(draws, max_lag=0, chunk=1 << 22):
    """MCMCChains' `summarystats` columns of the draws (K, D, N) — `draws[k]` is the (D, N) draw k —, pooled over all N chains:
    a dict name → (D,) array of SUMMARY_NAMES.  Split chains (K ≥ 4), rank-normalised bulk / folded tail R̂, bulk / tail / basic
    ESS with Stan's multi-chain Geyer truncation (`max_lag`: cap on the lags, 0 = none); a dimension holding a non-finite value
    gets NaN everywhere.  Computed in chunks of dimensions of at most ~`chunk` values."""
    x = np.asarray(draws)
    if x.ndim != 3 or x.shape[0] < 4:
        raise ValueError("draws must be (K, D, N) with K >= 4")
    if max_lag < 0:
        raise ValueError("max_lag must be >= 0")
    K, D, N = x.shape
    n, m = K // 2, 2 * N
    S = m * n
    out = {k: np.full(D, np.nan) for k in SUMMARY_NAMES}
    step = max(1, chunk // S)
    for d0 in range(0, D, step):
        y = _split_chains(x[:, d0:d0 + step])                 # (Dc, m, n)
        Dc = y.shape[0]
        flat = y.reshape(Dc, S)
        ok = np.isfinite(flat).all(axis=1)
        sx = np.sort(flat, axis=1)
        med = 0.5 * (sx[:, S // 2 - 1] + sx[:, S // 2]) if S % 2 == 0 else sx[:, S // 2]
        q05, q95 = _quantile7(sx, 0.05), _quantile7(sx, 0.95)
        z = _z_of(flat).reshape(Dc, m, n)
        zf = _z_of(np.abs(flat - med[:, None])).reshape(Dc, m, n)
        with np.errstate(invalid="ignore"):
            i05 = (y <= q05[:, None, None]).astype(np.float64)
            i95 = (y <= q95[:, None, None]).astype(np.float64)
        ess_basic, _ = _ess_rhat(y, max_lag)
        ess_bulk, rhat_bulk = _ess_rhat(z, max_lag)
        _, rhat_tail = _ess_rhat(zf, max_lag)
        e05, _ = _ess_rhat(i05, max_lag)
        e95, _ = _ess_rhat(i95, max_lag)
        mean = flat.mean(axis=1)
        std = flat.std(axis=1, ddof=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            rows = {"mean": mean, "std": std, "mcse": std / np.sqrt(ess_basic), "ess_bulk": ess_bulk,
                    "ess_tail": np.where(np.isnan(e05) | np.isnan(e95), np.nan, np.minimum(e05, e95)),
                    "rhat": np.where(np.isnan(rhat_bulk) | np.isnan(rhat_tail), np.nan, np.maximum(rhat_bulk, rhat_tail)),
                    "ess_basic": ess_basic, "rhat_bulk": rhat_bulk, "rhat_tail": rhat_tail}
        for k, v in rows.items():
            out[k][d0:d0 + Dc] = np.where(ok, v, np.nan)
    return out
