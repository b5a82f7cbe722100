"""The adaptation half of the dense engine against an EXACT covariance.

What runs when a shared `DenseEuclideanMetric` adapts (csrc/ahmc_dense.hpp, ahmc_dense_host.hpp, `adapt` in ahmc_api.hip):
`k_d_colsum_partial` / `k_d_colsum_final` (batch mean over the N chains, COV_SLICES = 64 slices), `k_dsyrk` (S = Σₙ(xₙ − m)(xₙ − m)ᵀ,
a 64×64 tile per workgroup, K = the chains in steps of 16, MFMA), `k_d_cov_combine` / `k_d_cov_mean` (Chan's pairwise merge),
`k_d_cov_estimate` (n/((n+5)(n−1))·M + 10⁻³·5/(n+5)·I), then `dn_set_metric` (host Cholesky, U⁻¹), `dn_refresh_fused` (C = M⁻¹P) and
`k_dense_swizzle*` in the next NUTS batch.

§1  `exact_estimate`: the reference's estimate (src/adaptation/massmatrix.jl:323-340) computed two-pass in x86 80-bit `np.longdouble`
    from the pushed batches (checked against mpmath), with the companion matrix Σₙ|xᵢₙ − μᵢ||xⱼₙ − μⱼ|.  Two forward error bounds, each a
    recurrence that follows ONE algorithm's roundings with γₖ = k·u/(1 − k·u): `batch_bound` (the device's batch algorithm) and
    `welford_bound` (the oracle's / the reference's one-draw-at-a-time update).  Neither is fitted to any output.
§2  the device estimate against §1 element by element; §3 what an update leaves behind (bit for bit a fresh context with the same matrix);
§4  whole warm-ups with a dense adaptor; §5 non-finite positions.

Every estimate comparison records error / bound per case; a run writes them to dense_adaptation_margins.json in the directory
$AHMC_TEST_OUT (default: test_out/ in the repository root, ignored by git); a copy of the MI355X run is profiles/dense_adaptation_margins.json.
"""
import functools
import json
import os

import numpy as np
import pytest

import ahmc_amd as A
import parity_util as PU

LD = np.longdouble
U = {np.dtype(np.float64): LD(2) ** -53, np.dtype(np.float32): LD(2) ** -24}
N_MIN = 10         # WelfordCov.n_min (massmatrix.jl:300)
COV_SLICES = 64    # csrc/ahmc_dense.hpp
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MARGINS = {}       # case id -> largest error / bound seen


def _is_hip(lib):
    return lib.backend.startswith("hip")


def _record(what, dtype, err, bound):
    """largest err/bound of a comparison (0/0 counts as 0); asserts it is ≤ 1 element by element and keeps the figure"""
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    assert np.isfinite(err).all(), f"{what}: non-finite estimate"
    frac = np.where(err == 0, LD(0), err / np.where(bound > 0, bound, LD(1e-4900)))
    worst = float(frac.max())
    key = f"{what} [{np.dtype(dtype).name}]"
    MARGINS[key] = max(MARGINS.get(key, 0.0), worst)
    _dump_margins()
    ij = np.unravel_index(int(np.argmax(frac)), frac.shape)
    assert worst <= 1.0, f"{key}: error {float(err[ij]):.3e} is {worst:.3g} × its bound {float(bound[ij]):.3e} at element {ij}"
    return worst


def _dump_margins():
    out = os.environ.get("AHMC_TEST_OUT") or os.path.join(ROOT, "test_out")
    try:
        os.makedirs(out, exist_ok=True)
        worst = {}
        for k, v in MARGINS.items():
            dt = k[k.rindex("[") + 1:-1]
            worst[dt] = max(worst.get(dt, 0.0), v)
        with open(os.path.join(out, "dense_adaptation_margins.json"), "w") as f:
            json.dump({"dry_run_on_oracle": os.environ.get("AHMC_TEST_DRYRUN_ON_ORACLE") == "1", "worst_error_over_bound": worst,
                       "error_over_bound": dict(sorted(MARGINS.items()))}, f, indent=1)
    except OSError:
        pass


# ------------------------------------------------------------------------------------------------
# §1  the exact reference and the two bounds
# ------------------------------------------------------------------------------------------------
def gam(k, u):
    k = LD(k)
    assert k * u < 0.5
    return k * u / (1 - k * u)


def scale_and_reg(n, dtype):
    """get_estimation's two scalars (massmatrix.jl:335-340), exact in long double; ϵ = T(1e-3) is part of the specification"""
    n = LD(n)
    return n / ((n + 5) * (n - 1)), LD(np.dtype(dtype).type(1e-3)) * (5 / (n + 5))


def exact_estimate(batches, companion=True):
    """`batches`: the pushed (D, N) arrays since the last reset, already in the engine's dtype.  Two-pass in long double: pooled mean, then
    M = Σ(x − μ)(x − μ)ᵀ over ALL pushed columns, then get_estimation.  Returns (estimate, companion Σ|xᵢ − μᵢ||xⱼ − μⱼ|, M, μ, n).
    The bounds below use the companion through Cauchy–Schwarz, companionᵢⱼ ≤ √(MᵢᵢMⱼⱼ), i.e. through its diagonal, which is M's."""
    dtype = batches[0].dtype
    D = batches[0].shape[0]
    n = sum(b.shape[1] for b in batches)
    mu = sum(b.astype(LD).sum(axis=1) for b in batches) / LD(n)
    M, comp = np.zeros((D, D), dtype=LD), np.zeros((D, D), dtype=LD)
    for b in batches:
        xc = b.astype(LD) - mu[:, None]
        M += xc @ xc.T
        if companion:
            xa = np.abs(xc)
            comp += xa @ xa.T
    c, reg = scale_and_reg(n, dtype)
    return c * M + reg * np.eye(D, dtype=LD), comp if companion else None, M, mu, n


def _estimate_bound(EM, M, n, dtype):
    """the final scaling on both sides: ĉ = fl(n / fl(fl(n+5)·fl(n−1))) with n converted to T (4 roundings + the conversion), ĉ·M̂ (1), the
    regulariser fl(T(1e-3)·fl(5/fl(n+5))) (3 + the conversion), the final addition (1; none where it contracts to an FMA): γ₇ on either term"""
    u = U[np.dtype(dtype)]
    c, reg = scale_and_reg(n, dtype)
    g7 = gam(7, u)
    D = M.shape[0]
    return c * EM * (1 + g7) + g7 * (c * np.abs(M) + reg * np.eye(D, dtype=LD))


def batch_bound(batches):
    """Forward error bound of the DEVICE's estimate, push by push, in long double, from the kernels' arithmetic (u = unit roundoff):

    k_d_colsum_*   m̂ = the sum of 64 partial sums of per = ⌈N/64⌉ terms each, divided by N: (per − 1) + 63 additions and one division,
                   |m̂ᵢ − mᵢ| ≤ eᵢ = γ(per+64) · Σₙ|xᵢₙ| / N.
    k_dsyrk        ĉᵢₙ = fl(xᵢₙ − m̂ᵢ) (one rounding each), the N products added by MFMA in groups of four; whatever the order of the
                   additions, N − 1 of them and one rounding per product (none where fused) give
                   |Ŝᵢⱼ − Σₙ(xᵢₙ − m̂ᵢ)(xⱼₙ − m̂ⱼ)| ≤ γ(N+2) · Σₙ|xᵢₙ − m̂ᵢ||xⱼₙ − m̂ⱼ| ≤ γ(N+2) · √((Sᵢᵢ + N eᵢ²)(Sⱼⱼ + N eⱼ²))   (Cauchy–Schwarz)
                   and Σₙ(xᵢₙ − m̂ᵢ)(xⱼₙ − m̂ⱼ) = Sᵢⱼ + N (mᵢ − m̂ᵢ)(mⱼ − m̂ⱼ) exactly (the zero-padded chains of the K tail add exact zeros).
    k_d_cov_combine  d̂ᵢ = fl(m̂ᵢ − μ̂ᵢ): |d̂ᵢ − dᵢ| ≤ hᵢ = eᵢ + fᵢ + u(|dᵢ| + eᵢ + fᵢ) with fᵢ the bound on the running mean;
                   ŵ = fl(fl(n̂·N)/fl(n̂ + N)), n̂ = (T)n: relative γ₅; t̂ᵢⱼ = fl(fl(d̂ᵢd̂ⱼ)·ŵ): two more; M̂ ← fl(fl(M̂ + Ŝ) + t̂): two
                   roundings, each on a magnitude ≤ √(MᵢᵢMⱼⱼ) + √(SᵢᵢSⱼⱼ) + w|dᵢ||dⱼ| plus the errors so far.
    k_d_cov_mean   μ̂′ = fl(μ̂ + fl(d̂·fl(N/fl(n̂+N)))) = μ̂(1 − r) + m̂ r + (relative γ₄ on d̂ r), then one rounding:
                   f′ = ((1 − r) f + r e + γ₄ r (|d| + h) + u|μ′|)(1 + 2u),  r = N/(n + N).
    k_d_cov_estimate  `_estimate_bound`.
    Everything is expressed through exact quantities of the data: the diagonal of the companion matrix (Sᵢᵢ, Mᵢᵢ: for i = j the companion IS
    the scatter), the batch means and the mean absolute values.  Returns the (D, D) bound on |estimate − exact_estimate|."""
    dtype = np.dtype(batches[0].dtype)
    u = U[dtype]
    D = batches[0].shape[0]
    n = 0
    mu, f = np.zeros(D, dtype=LD), np.zeros(D, dtype=LD)
    Mdiag, E = np.zeros(D, dtype=LD), np.zeros((D, D), dtype=LD)
    for b in batches:
        x = b.astype(LD)
        N = x.shape[1]
        per = -(-N // COV_SLICES)
        m = x.sum(axis=1) / N
        e = gam(per + COV_SLICES, u) * np.abs(x).sum(axis=1) / N
        s2 = ((x - m[:, None]) ** 2).sum(axis=1)                    # diagonal of the batch scatter
        sp = np.sqrt(s2 + N * e * e)
        ES = gam(N + 2, u) * np.outer(sp, sp) + N * np.outer(e, e)
        d = np.abs(m - mu) if n else np.zeros(D, dtype=LD)           # (n = 0: w = 0, the term vanishes exactly)
        h = e + f + u * (d + e + f)
        w = LD(n) * N / (n + N)
        dh = d + h
        ET = w * (np.outer(d, h) + np.outer(h, d) + np.outer(h, h) + gam(7, u) * np.outer(dh, dh))
        mag = np.outer(np.sqrt(Mdiag), np.sqrt(Mdiag)) + np.outer(np.sqrt(s2), np.sqrt(s2)) + w * np.outer(d, d)
        E = (E + ES + ET) * (1 + 2 * u) + 2 * u * mag
        r = LD(N) / (n + N)
        mu_new = mu + (m - mu) * r
        f = ((1 - r) * f + r * e + gam(4, u) * r * (d + h) + u * np.abs(mu_new)) * (1 + 2 * u)
        Mdiag = Mdiag + s2 + w * d * d
        mu, n = mu_new, n + N
    return E, n


def welford_bound(batches):
    """Forward error bound of the ORACLE's estimate: push!(wc, s) (massmatrix.jl:323-331) one chain after another, k = 1 … n:
        δ̂ = fl(s − μ̂),  μ̂ ← fl(μ̂ + fl(δ̂/k)),  M̂ ← fl(M̂ + fl(fl(s − μ̂)·δ̂ᵀ)).
    With f the bound on the running mean: |δ̂ − δ| ≤ hδ = f + u(|δ| + f); μ̂′ = μ̂(1 − 1/k) + s/k + (relative γ₂ on δ̂/k), one more rounding:
    f′ = ((1 − 1/k) f + γ₂(|δ| + f)/k + u|μ′|)(1 + 2u); â = fl(s − μ̂′): |â − a| ≤ ha = f′ + u(|a| + f′), a = s − μ′.  The k-th product then
    carries |âᵢδ̂ⱼ − aᵢδⱼ| ≤ |aᵢ|hδⱼ + haᵢ|δⱼ| + haᵢhδⱼ, its own rounding u and the n − 1 additions γ(n−1), both on (|aᵢ| + haᵢ)(|δⱼ| + hδⱼ).
    Summed over k by Cauchy–Schwarz this needs only the per-dimension 2-norms of a, δ, ha, hδ.  The mean's error enters the products to FIRST
    order, so the bound grows with |mean|/spread: that is this algorithm (Chan, Golub & LeVeque 1983: n·κ·u), not slack.
    M̂ᵢⱼ pairs a (row) with δ (column), so the bound is not symmetric either."""
    dtype = np.dtype(batches[0].dtype)
    u = U[dtype]
    X = np.concatenate([b.astype(LD) for b in batches], axis=1)
    D, n = X.shape
    ks = np.arange(1, n + 1, dtype=LD)
    mus = np.cumsum(X, axis=1) / ks                                  # μ_k
    prev = np.concatenate([np.zeros((D, 1), dtype=LD), mus[:, :-1]], axis=1)
    delta = np.abs(X - prev)
    a = np.abs(X - mus)
    f = np.zeros(D, dtype=LD)
    hd2, ha2 = np.zeros(D, dtype=LD), np.zeros(D, dtype=LD)
    g2 = gam(2, u)
    for k in range(n):
        hd = f + u * (delta[:, k] + f)
        f = ((1 - 1 / ks[k]) * f + g2 * (delta[:, k] + f) / ks[k] + u * np.abs(mus[:, k])) * (1 + 2 * u)
        ha = f + u * (a[:, k] + f)
        hd2 += hd * hd
        ha2 += ha * ha
    na, nd, nha, nhd = np.sqrt((a * a).sum(axis=1)), np.sqrt((delta * delta).sum(axis=1)), np.sqrt(ha2), np.sqrt(hd2)
    E = np.outer(na, nhd) + np.outer(nha, nd) + np.outer(nha, nhd) + (u + gam(max(n - 1, 1), u) * (1 + u)) * np.outer(na + nha, nd + nhd)
    return E, n


def estimate_bound(batches, lib_is_hip, M):
    E, n = (batch_bound if lib_is_hip else welford_bound)(batches)
    return _estimate_bound(E, M, n, batches[0].dtype)


# ---- data ----
def _cov_factor(D, rs, cond):
    """L with LLᵀ = Σ, Σ's eigenvalues log-spaced over [1/cond, 1] in a random basis (correlated, condition number `cond`)"""
    Q, _ = np.linalg.qr(rs.normal(size=(D, D)))
    return Q * np.sqrt(np.logspace(-np.log10(cond), 0.0, D))


def make_batches(kind, D, N, pushes, dtype, rs):
    """the pushed positions, rounded to the engine's dtype.  `corr`: correlated Gaussian, cond(Σ) = 10⁴; `bigmean`: the same with a mean of
    10³ standard deviations in every third dimension (cancellation); `jump`: the batch mean moves between pushes, by 30 standard deviations in the first, the middle and the last dimension (every tile
    row and column of k_dsyrk's grid) and by 3 in the others, cond(Σ) = 10² — a rank-one term of 900 variances on top of cond 10⁴ has no Float32
    Cholesky factor in either implementation;
    `const`: dimension D//2 is 3.0 in every chain and push (3·N is exact in both dtypes, so the device's mean is exact as well)."""
    L = _cov_factor(D, rs, 1.0 if D == 1 else 1e2 if kind == "jump" else 1e4)
    sd = np.sqrt((L * L).sum(axis=1))
    out = []
    for p in range(pushes):
        x = L @ rs.normal(size=(D, N))
        if kind == "bigmean":
            x[::3] += 1e3 * sd[::3, None]
        elif kind == "jump":
            amp = np.full(D, 3.0)
            amp[[0, D // 2, D - 1]] = 30.0
            x += (amp * sd * rs.choice([-1.0, 1.0], size=D))[:, None]
        elif kind == "const":
            x[D // 2] = 3.0
        out.append(np.asfortranarray(x.astype(dtype)))
    return out


# (D, N, pushes per window, data).  D: below, at and above one and two 64-tiles; N: fewer chains than the 64 column-sum slices, the K-loop tail
# with N mod 16 ∈ {0, 1, 3, 15}, a prime; 1–8 pushes: Chan's merge with n = 0, n = N and n ≫ N.  Fewer pooled draws than D: rank-deficient S.
CASES = [
    (1, 1, 8, "corr"), (1, 17, 2, "corr"), (2, 3, 8, "corr"), (2, 15, 3, "bigmean"),
    (12, 96, 4, "corr"), (12, 16, 2, "jump"), (12, 4099, 3, "bigmean"),
    (63, 17, 3, "corr"), (63, 1000, 2, "bigmean"),
    (64, 16, 1, "corr"), (64, 96, 5, "jump"),
    (65, 17, 6, "corr"), (65, 1000, 3, "bigmean"), (65, 4099, 2, "corr"), (65, 15, 1, "corr"),
    (128, 96, 2, "jump"), (128, 4099, 1, "bigmean"),
    (129, 17, 8, "corr"), (129, 1000, 2, "const"), (129, 3, 5, "corr"),
    (200, 1000, 2, "corr"), (200, 15, 4, "const"), (200, 4099, 2, "jump"),
    (512, 96, 2, "corr"), (512, 1000, 1, "bigmean"), (512, 17, 3, "corr"), (512, 1000, 2, "jump"),
]
DTYPES = [np.float64, np.float32]


def _case_id(c):
    return "D{}-N{}-p{}-{}".format(*c)


@functools.lru_cache(maxsize=4)
def _case_data(case, dtype_name, n_batches):
    D, N, pushes, kind = case
    rs = np.random.default_rng([20260925, D, N, pushes, len(kind)])
    return make_batches(kind, D, N, n_batches, np.dtype(dtype_name), rs)


def _engine(lib, D, N, dtype, adaptor_of, minv0=None):
    minv0 = np.eye(D) if minv0 is None else minv0
    e = A.Engine(A.Hamiltonian(A.DenseEuclideanMetric(minv0), A.IsoGaussian(D)), N, dtype=dtype, rng=3, lib=lib)
    lf = A.Leapfrog(np.full(N, 0.1))
    e.set_integrator(lf)
    e.set_position(np.zeros((D, N)))
    e.adaptor_init(adaptor_of(lf))
    return e


def _minv(e):
    """the context's dense M⁻¹ as a (D, D) array (get_metric answers with the first shape of the right size)"""
    return np.asarray(e.get_metric()).reshape(e.D, e.D)


def _check_estimate(got, batches, lib, what, structural=True):
    """`got` (the engine's M⁻¹) against the exact estimate over `batches`, element by element inside the bound of the algorithm `lib` runs"""
    dtype = batches[0].dtype
    ref, _, M, mu, n = exact_estimate(batches, companion=False)   # (the bounds need the companion's diagonal only: that of M)
    bound = estimate_bound(batches, _is_hip(lib), M)
    bound = bound + U[np.dtype(dtype)] * np.abs(ref)   # (what the engine returns is rounded to T once more at most: it IS a T)
    frac = _record(what, dtype, np.abs(got.astype(LD) - ref), bound)
    if structural and _is_hip(lib):
        # tile (i, j) and tile (j, i) add the same products in the same order
        np.testing.assert_array_equal(got, got.T, err_msg=f"{what}: the estimate is not symmetric bit for bit")
    np.linalg.cholesky(got.astype(np.float64))   # it factorises (the 10⁻³ term where S is rank-deficient)
    return frac, ref, bound


def drive_massmatrix(lib, case, dtype, what):
    """MassMatrixAdaptor(DenseEuclideanMetric) alone: an estimate after EVERY push once n ≥ n_min (massmatrix.jl:60-62 via Adaptation.jl)"""
    D, N, pushes, kind = case
    batches = _case_data(case, np.dtype(dtype).name, pushes)
    e = _engine(lib, D, N, dtype, lambda lf: A.MassMatrixAdaptor(A.DenseEuclideanMetric(np.eye(D))))
    every = D * D * N * pushes <= 2e7   # (the long-double reference at every push where that is cheap, else at the last one)
    for p in range(1, pushes + 1):
        e.adapt(p, pushes + 5, theta=batches[p - 1])
        got = _minv(e)
        if p * N < N_MIN:
            np.testing.assert_array_equal(got, np.eye(D, dtype=dtype), err_msg=f"{what}: {p * N} < n_min draws must leave M⁻¹ untouched")
        elif every or p == pushes:
            _check_estimate(got, batches[:p], lib, what)
            if kind == "const":
                j = D // 2
                off = np.delete(np.arange(D), j)
                assert (got[j, off] == 0).all() and (got[off, j] == 0).all(), f"{what}: a constant dimension must have an exactly zero row and column"
                T = np.dtype(dtype).type
                assert got[j, j] == T(1e-3) * (T(5) / (T(p * N) + T(5))), f"{what}: …and exactly the regulariser on the diagonal"
    e.close()


def reference_windows(n_adapts, init_buffer, term_buffer, window_size):
    """initialize!(::StanHMCAdaptorState, …) (src/adaptation/stan_adaptor.jl:21-37), restated: (window_start, window_end, splits)"""
    start, end = init_buffer + 1, n_adapts - term_buffer
    splits, nxt = [], init_buffer + window_size
    while nxt <= end:
        if nxt + 2 * window_size > end:
            nxt = end
        splits.append(nxt)
        window_size *= 2
        nxt += window_size
    if splits and splits[-1] == n_adapts:
        splits.pop()
    return start, end, splits


def drive_stan(lib, case, dtype, what, w=None):
    """StanHMCAdaptor with windows of w and 2w pushes: the estimate read after a window end is the reference over exactly that window's draws
    (reset at the end: nothing carried over, nothing dropped); between window ends M⁻¹ does not move"""
    D, N, pushes, kind = case
    if w is None:
        w = pushes if D * D * N * pushes <= 2e7 else 1
    ib, tb = 2, 3
    n_adapts = ib + 3 * w + tb
    start, end, splits = reference_windows(n_adapts, ib, tb, w)
    assert (start, end, splits) == (ib + 1, ib + 3 * w, [ib + w, ib + 3 * w]), (start, end, splits)   # two window ends, by the reference's rule
    batches = _case_data(case, np.dtype(dtype).name, n_adapts)
    e = _engine(lib, D, N, dtype, lambda lf: A.StanHMCAdaptor(A.MassMatrixAdaptor(A.DenseEuclideanMetric(np.eye(D))), A.StepSizeAdaptor(0.8, lf),
                                                              init_buffer=ib, term_buffer=tb, window_size=w))
    current = np.eye(D, dtype=dtype)
    window = []
    for i in range(1, n_adapts + 1):
        e.adapt(i, n_adapts, theta=batches[i - 1], alpha=np.full(N, 0.8))
        if start <= i <= end:
            window.append(batches[i - 1])
        got = _minv(e)
        if i in splits:
            if len(window) * N >= N_MIN:
                _check_estimate(got, window, lib, what)
                current = got.copy()
            else:
                np.testing.assert_array_equal(got, current, err_msg=f"{what}: fewer than n_min pooled draws at iteration {i}")
            window = []
        else:
            np.testing.assert_array_equal(got, current, err_msg=f"{what}: M⁻¹ moved at iteration {i}, which is no window end")
    e.close()


# ---- CPU: the reference and the bounds are proven on the oracle before a GPU is involved ----
def test_exact_estimate_agrees_with_mpmath():
    """the long-double two-pass estimate and companion against 200-bit mpmath at the smallest shapes: a few 2⁻⁶⁴ relative to the companion"""
    import mpmath

    mpmath.mp.prec = 200
    rs = np.random.default_rng(7)
    for D, N, pushes, kind in ((1, 17, 2, "corr"), (2, 15, 3, "bigmean"), (3, 5, 4, "jump")):
        for dtype in DTYPES:
            batches = make_batches(kind, D, N, pushes, dtype, rs)
            est, comp, M, mu, n = exact_estimate(batches)
            cols = [[mpmath.mpf(float(v)) for v in col] for b in batches for col in b.T]
            assert n == len(cols) == N * pushes
            m = [sum(c[i] for c in cols) / n for i in range(D)]
            c_, reg = mpmath.mpf(n) / ((n + 5) * (n - 1)), mpmath.mpf(float(np.dtype(dtype).type(1e-3))) * 5 / (n + 5)
            for i in range(D):
                for j in range(D):
                    s = sum((c[i] - m[i]) * (c[j] - m[j]) for c in cols)
                    a = sum(abs(c[i] - m[i]) * abs(c[j] - m[j]) for c in cols)
                    # 80-bit arithmetic: n·2⁻⁶⁴ relative to the companion, the mean's own 2⁻⁶⁴·n·|μ| entering the scatter to second order only
                    tol = mpmath.mpf(2) ** -56 * a
                    assert abs(_mp(comp[i, j]) - a) <= tol
                    assert abs(_mp(M[i, j]) - s) <= tol, (D, N, kind, i, j)
                    assert abs(_mp(est[i, j]) - (c_ * s + (reg if i == j else 0))) <= c_ * tol + mpmath.mpf(2) ** -60 * reg


def _mp(x):
    """a long double as an exact mpmath number (hi + lo split through two doubles)"""
    import mpmath

    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - LD(hi)))


def test_reference_windows_match_the_engine_rule(oracle):
    """the restated window rule against `ahmc_stan_windows` on schedules with 0, 1 and several splits, a last split on n_adapts included"""
    for n_adapts, ib, tb, ws in ((1000, 75, 50, 25), (160, 75, 50, 25), (100, 75, 50, 25), (11, 2, 3, 2), (8, 2, 3, 1), (20, 5, 0, 5), (50, 10, 10, 7)):
        assert reference_windows(n_adapts, ib, tb, ws) == A.stan_windows(n_adapts, ib, tb, ws, lib=oracle), (n_adapts, ib, tb, ws)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_oracle_sequential_welford_within_its_bound(oracle, case, dtype):
    """the oracle's one-draw-at-a-time Welford update (the reference's algorithm) against the exact estimate, inside `welford_bound`, at every
    shape of the grid and after every push"""
    drive_massmatrix(oracle, case, dtype, "oracle " + _case_id(case))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case", [c for c in CASES if c[0] <= 129 and c[1] <= 1000], ids=_case_id)
def test_oracle_window_semantics(oracle, case, dtype):
    """StanHMCAdaptor on the oracle: window ends from the reference's rule, the estimate after each is over exactly that window's draws, fewer
    than n_min = 10 pooled draws leave M⁻¹ untouched (cases N = 1 and N = 3 with one push)"""
    drive_stan(oracle, case, dtype, "oracle windows " + _case_id(case))
    if case[1] <= 3:
        drive_stan(oracle, case, dtype, "oracle windows w=1 " + _case_id(case), w=1)


def test_bounds_are_not_vacuous():
    """the device bound, relative to √(refᵢᵢ·refⱼⱼ), is 1–3 × (N + pushes + 8)·u where the mean is small against the spread (a numpy model of the
    batch algorithm, rounded to the dtype at every step, errs by 0.004–0.13 of that): a lost chain of the K tail, a relative
    1/N of S and more, exceeds it by orders of magnitude except in Float32 at N = 4 099, where three lost chains of 4 099 exceed it 3-fold"""
    for dtype in DTYPES:
        for case in ((12, 96, 4, "corr"), (65, 17, 6, "corr"), (65, 1000, 3, "corr"), (65, 4099, 2, "corr")):
            batches = _case_data(case, np.dtype(dtype).name, case[2])
            ref, _, M, mu, n = exact_estimate(batches, companion=False)
            b = estimate_bound(batches, True, M)
            rel = float((b / np.sqrt(np.outer(np.diag(ref), np.diag(ref)))).max())
            assert rel < 4 * float((case[1] + case[2] + 8) * U[np.dtype(dtype)]), (case, rel)


# ------------------------------------------------------------------------------------------------
# §2  the device estimate against the exact reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_device_estimate_massmatrix_adaptor(hip, case, dtype):
    """MassMatrixAdaptor(DenseEuclideanMetric) alone on the HIP engine, caller-supplied positions: M⁻¹ after every push against the exact
    estimate, element by element inside `batch_bound`; symmetric bit for bit; untouched below n_min; a constant dimension exactly zero"""
    drive_massmatrix(hip, case, dtype, "massmatrix " + _case_id(case))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_device_estimate_stan_windows(hip, case, dtype):
    """StanHMCAdaptor on the HIP engine: windows of w and 2w pushes, each estimate over exactly its window's draws (dn_cov_init at the end)"""
    drive_stan(hip, case, dtype, "stan " + _case_id(case))


@pytest.mark.gpu
def test_device_estimate_float32_beyond_2_to_24_draws(hip):
    """Float32, D = 2, N = 65 536, 300 pushes: 19.7 million pooled draws, so (T)wc_n is not exact any more after push 256 (the conversion is one
    of the roundings `batch_bound` counts).  Checked at pushes 256, 257 and 300.  (A dry run on the CPU checker stops after 3 pushes: its
    bound is a Python loop over the draws.)"""
    D, N = 2, 65536
    pushes, at = (300, (256, 257, 300)) if _is_hip(hip) else (3, (3,))
    rs = np.random.default_rng(11)
    L = _cov_factor(D, rs, 1e2)
    batches = [np.asfortranarray((L @ rs.normal(size=(D, N)) + np.array([[5.0], [-2.0]])).astype(np.float32)) for _ in range(pushes)]
    e = _engine(hip, D, N, np.float32, lambda lf: A.MassMatrixAdaptor(A.DenseEuclideanMetric(np.eye(D))))
    for p in range(1, pushes + 1):
        e.adapt(p, pushes + 5, theta=batches[p - 1])
        if p in at:
            _check_estimate(_minv(e), batches[:p], hip, f"float32 2^24 draws, push {p}")
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_embedding_in_a_larger_problem_is_bit_identical(hip, dtype):
    """the D = 65 problem placed in the first 65 dimensions of a D = 129 problem (the rest independent noise): the same 65×65 block bit for
    bit — the element (i, j) sums the same N centred products in the same order whichever tile edge lies beyond it, and the column sums take
    the chains in the same 64 slices"""
    N, pushes = 1000, 3
    small = _case_data((65, N, pushes, "bigmean"), np.dtype(dtype).name, pushes)
    rs = np.random.default_rng(5)
    got = {}
    for D in (65, 129):
        e = _engine(hip, D, N, dtype, lambda lf: A.MassMatrixAdaptor(A.DenseEuclideanMetric(np.eye(D))))
        for p in range(pushes):
            x = np.asfortranarray(rs.normal(size=(D, N)).astype(dtype))
            x[:65] = small[p]
            e.adapt(p + 1, pushes + 5, theta=x)
        got[D] = _minv(e)
        e.close()
    np.testing.assert_array_equal(got[129][:65, :65], got[65])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_rank_deficient_and_non_finite_pushes_status(hip, oracle, dtype):
    """(i) fewer pooled draws than D (S is rank-deficient): the estimate still factorises thanks to the 10⁻³ term — the same status, OK, from the
    HIP engine and the oracle, and the same matrix inside the two bounds.  (ii) a non-finite position in ONE pushed chain (a Float32 divergence):
    both report the same status from `adapt` (PosDefException → AHMC_ERR_ARGUMENT), and the context keeps its previous metric, bit for bit, and
    can still refresh a momentum and take a leapfrog step with it"""
    D, N = 65, 15
    batches = _case_data((D, N, 1, "corr"), np.dtype(dtype).name, 1)
    for lib in (hip, oracle):
        e = _engine(lib, D, N, dtype, lambda lf: A.MassMatrixAdaptor(A.DenseEuclideanMetric(np.eye(D))))
        e.adapt(1, 5, theta=batches[0])    # no exception from either
        _check_estimate(_minv(e), batches, lib, "rank-deficient D65-N15")
        e.close()
    D, N = 12, 96
    clean = _case_data((D, N, 4, "corr"), np.dtype(dtype).name, 4)
    for bad_value in (np.nan, np.inf):
        codes = []
        for lib in (hip, oracle):
            e = _engine(lib, D, N, dtype, lambda lf: A.MassMatrixAdaptor(A.DenseEuclideanMetric(np.eye(D))))
            e.adapt(1, 9, theta=clean[0])
            e.adapt(2, 9, theta=clean[1])
            before = _minv(e).copy()
            bad = clean[2].copy()
            bad[5, 37] = bad_value
            with pytest.raises(A.capi.ArgumentError) as ei:
                e.adapt(3, 9, theta=bad)
            assert "PosDefException" in str(ei.value)
            codes.append(ei.value.code)
            np.testing.assert_array_equal(_minv(e), before, err_msg=f"{lib.backend}: a refused update must leave M⁻¹ as it was")
            e.set_position(clean[3])
            e.refresh()
            e.step(1)
            z = e.phasepoint()
            assert np.isfinite(z.theta).all() and np.isfinite(z.r).all() and np.isfinite(z.lk.value).all()
            e.close()
        assert codes[0] == codes[1] == A.capi.ERR_ARGUMENT


# ------------------------------------------------------------------------------------------------
# §3  what the update leaves behind
# ------------------------------------------------------------------------------------------------
def _ar1_precision(D):
    idx = np.arange(D)
    return np.asfortranarray(np.linalg.inv(0.9 ** np.abs(idx[:, None] - idx[None, :])))


def _nuts(lf, max_depth=6):
    return A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=max_depth, delta_max=1000.0)))


def _observe(e, k, th0, bulk):
    """refresh_momentum, the kinetic energy and ∂H∂r (through one leapfrog step) by the phase-point calls, then three NUTS transitions"""
    out = {}
    e.set_position(th0)
    e.refresh()
    z = e.phasepoint()
    out["r"], out["lk"] = z.r.copy(), z.lk.value.copy()
    e.step(1)
    z = e.phasepoint()
    out["theta1"], out["r1"], out["lk1"] = z.theta.copy(), z.r.copy(), z.lk.value.copy()
    e.set_position(th0)
    e.reset_accum()
    if bulk:
        e.run(k, 3, 0)
    else:
        out["n_steps_each"] = []
        for _ in range(3):
            e.transition(k)
            out["n_steps_each"].append(e.stats()["n_steps"].copy())
        out["n_steps_each"] = np.array(out["n_steps_each"])
    e.sync()
    st, acc = e.stats(), e.accum()
    out["n_steps"], out["theta"] = st["n_steps"].copy(), e.theta().copy()
    out["energy"] = st["hamiltonian_energy"].copy()
    out["total_n_steps"] = acc["total_n_steps"]
    if acc["sum_theta"] is not None and acc["n_transitions"]:
        out["sum_theta"], out["sumsq_theta"] = acc["sum_theta"].copy(), acc["sumsq_theta"].copy()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("D,dtype,epoch", [(65, np.float64, False), (65, np.float32, False), (200, np.float64, False), (200, np.float32, False),
                                           (256, np.float64, True), (384, np.float32, True), (512, np.float64, True), (512, np.float32, True)],
                         ids=lambda v: getattr(v, "__name__", str(v)))
def test_adapted_context_equals_fresh_context_with_the_same_matrix(hip, oracle, monkeypatch, D, dtype, epoch):
    """After an adaptation has replaced M⁻¹ (new U⁻¹, new C = M⁻¹P, new swizzled copy for the chain-complete kernels) the context behaves,
    bit for bit, like a FRESH context given the matrix `get_metric()` returns: refresh_momentum, the kinetic energy, one leapfrog, three NUTS
    transitions (n_steps, θ, the accumulators).  The adapting context has run NUTS with its OLD matrix first, so every derived copy existed and
    was stale-able.  D = 256 / 384 / 512: AHMC_DENSE_EPOCH_MIN = 32, `dense_epoch_launches` > 0 on both.  Then against the oracle given the same
    matrix, margin-aware (a chain may differ only at a near tie)."""
    monkeypatch.setenv("AHMC_DENSE_EPOCH_MIN", "32")
    monkeypatch.setenv("AHMC_DENSE_EPOCH", "1")
    N = 192 if epoch else 70
    rs = np.random.default_rng([D, 17])
    P = _ar1_precision(D)
    th0 = np.asfortranarray(rs.normal(size=(D, N)))
    eps = np.full(N, 0.1)
    lf = A.Leapfrog(eps)
    k = _nuts(lf)
    # the pushed positions: draws of N(0, P⁻¹), two pushes (the second merges into n = N)
    Lc = np.linalg.cholesky(np.linalg.inv(P))
    pushes = [np.asfortranarray((Lc @ rs.normal(size=(D, N))).astype(dtype)) for _ in range(2 + (D + N - 1) // N)]
    a = A.Engine(A.Hamiltonian(A.DenseEuclideanMetric(np.eye(D)), A.DenseGaussian(P)), N, dtype=dtype, rng=A.PhiloxRNG(31), lib=hip)
    a.set_integrator(lf)
    a.set_position(th0)
    a.run(k, 2, 0)                       # NUTS with the old matrix: C, the swizzled copy and U⁻¹ of M⁻¹ = I are in place
    launches_before = a.info("dense_epoch_launches")
    a.adaptor_init(A.MassMatrixAdaptor(A.DenseEuclideanMetric(np.eye(D))))
    for i, x in enumerate(pushes):
        a.adapt(i + 1, len(pushes) + 5, theta=x)
    M1 = _minv(a).copy()
    assert not np.array_equal(M1, np.eye(D, dtype=dtype))
    a.adaptor_init(A.NoAdaptation())
    a.seed(A.PhiloxRNG(32), iteration=0)
    got_a = _observe(a, k, th0, epoch)
    b = A.Engine(A.Hamiltonian(A.DenseEuclideanMetric(M1), A.DenseGaussian(P)), N, dtype=dtype, rng=A.PhiloxRNG(32), lib=hip)
    b.set_integrator(lf)
    b.seed(A.PhiloxRNG(32), iteration=0)
    got_b = _observe(b, k, th0, epoch)
    if epoch and _is_hip(hip):
        assert launches_before > 0 and a.info("dense_epoch_launches") > launches_before and b.info("dense_epoch_launches") > 0, (D, dtype)
    assert got_a.keys() == got_b.keys()
    for key in got_a:
        np.testing.assert_array_equal(got_a[key], got_b[key], err_msg=f"D={D} {np.dtype(dtype).name}: {key} differs from a fresh context's")
    a.close()
    b.close()
    # the oracle with the same matrix, on the first n chains
    n = 48 if epoch else N
    o = A.Engine(A.Hamiltonian(A.DenseEuclideanMetric(M1), A.DenseGaussian(P)), n, dtype=dtype, rng=A.PhiloxRNG(32), lib=oracle)
    o.set_integrator(A.Leapfrog(eps[:n]))
    o.seed(A.PhiloxRNG(32), iteration=0)
    PU.reset_margin(o)
    got_o = _observe(o, k, th0[:, :n], epoch)
    tol = 1e-9 if dtype == np.float64 else 2e-3
    for key in ("r", "lk", "theta1", "r1", "lk1"):
        ref = got_o[key]
        np.testing.assert_allclose(got_a[key][..., :n], ref, rtol=tol, atol=tol * max(1.0, float(np.abs(ref).max())), err_msg=key)
    same = PU.check_flips(got_a["n_steps"][:n] == got_o["n_steps"], PU.decision_margin(o), dtype, f"adapted dense metric D={D}", n_steps=got_o["n_steps"])
    np.testing.assert_allclose(got_a["theta"][:, :n][:, same], got_o["theta"][:, same], rtol=tol * 100, atol=tol * 100)
    o.close()


# ------------------------------------------------------------------------------------------------
# §4  whole warm-ups with a dense adaptor
# ------------------------------------------------------------------------------------------------
def _stan_dense(D, lf, ib, tb, ws):
    return A.StanHMCAdaptor(A.MassMatrixAdaptor(A.DenseEuclideanMetric(np.eye(D))), A.StepSizeAdaptor(0.8, lf), init_buffer=ib, term_buffer=tb,
                            window_size=ws)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("D", [24, 129])
def test_run_equals_transition_plus_adapt_with_a_dense_adaptor(hip, D, dtype):
    """`run(k, n_samples, n_adapts)` == per-iteration `transition` + `adapt`, bit for bit, with StanHMCAdaptor(MassMatrixAdaptor(Dense…),
    StepSizeAdaptor) over a schedule with two window ends (the family tests/test_random_configurations.py skips for a dense metric)"""
    N, n_adapts, n_samples = 64, 40, 44
    ib, tb, ws = 5, 5, 8
    assert reference_windows(n_adapts, ib, tb, ws)[2] == [13, 35]
    rs = np.random.default_rng([D, 4])
    P = _ar1_precision(D)
    th0 = np.asfortranarray(rs.normal(size=(D, N)))
    out = []
    for bulk in (True, False):
        lf = A.Leapfrog(np.full(N, 0.15))
        k = _nuts(lf, max_depth=5)
        e = A.Engine(A.Hamiltonian(A.DenseEuclideanMetric(np.eye(D)), A.DenseGaussian(P)), N, dtype=dtype, rng=A.PhiloxRNG(9), lib=hip)
        e.set_integrator(lf)
        e.set_position(th0)
        e.adaptor_init(_stan_dense(D, lf, ib, tb, ws))
        if bulk:
            e.run(k, n_samples, n_adapts)
        else:
            for i in range(1, n_samples + 1):
                e.transition(k)
                e.adapt(i, n_adapts)
        e.sync()
        out.append((_minv(e).copy(), e.get_stepsize().copy(), e.theta().copy(), e.stats()["n_steps"].copy()))
        e.close()
    assert not np.array_equal(out[0][0], np.eye(D, dtype=dtype))
    for x, y, name in zip(out[0], out[1], ("M⁻¹", "ϵ", "θ", "n_steps")):
        np.testing.assert_array_equal(x, y, err_msg=f"D={D}: {name} of run() differs from transition + adapt")


def _draw_buffer(lib, n, N, D, dtype):
    """a (n, N, D) buffer `run(samples_out=…)` fills: device memory for the HIP engine, host memory for the CPU checker"""
    if _is_hip(lib):
        import torch

        t = torch.empty((n, N, D), dtype=torch.float32 if np.dtype(dtype) == np.float32 else torch.float64, device="cuda")
        return t.data_ptr(), lambda: t.cpu().numpy()
    a = np.empty((n, N, D), dtype=dtype)
    return a.ctypes.data, lambda: a


@pytest.mark.gpu
@pytest.mark.parametrize("D,N,dtype", [(256, 1100, np.float64), (512, 600, np.float64), (256, 1100, np.float32), (512, 600, np.float32)],
                         ids=lambda v: getattr(v, "__name__", str(v)))
def test_dense_warmup_epoch_engine_equals_step_synchronous_engine(hip, monkeypatch, D, N, dtype):
    """The chain-complete kernels (AHMC_DENSE_EPOCH=1) against the step-synchronous ones (=0) through a whole Stan warm-up with a DENSE
    adaptor — M⁻¹, U⁻¹, C and the swizzled copy change at two window ends between launches — in the form and with the tolerances of
    test_dense_epoch_kernel_equals_step_synchronous_kernels (f64: equal n_steps, positions to 1e-9; f32: its share rule).  At each window end
    each engine's M⁻¹ is held against the exact estimate over ITS OWN draws of that window (`samples_out`), inside `batch_bound`: that places
    the two engines' matrices within the sum of their bounds plus the 1e-9 their draws differ by.
    Step sizes as in that test (ϵ₀ ≈ 0.12).  Measured on the MI355X: the engines' draws and both M⁻¹ are bit-identical through iteration 4 and
    differ by 6.5e-12 (f64, D = 256) / 1.4e-3 in one chain (f32, D = 256) after it.  With ϵ₀ ≈ 0.02 every chain moves in iterations 1–3 and the
    trees are deep: Float64 still agrees (max |Δθ| 2.3e-10 at D = 256, 4.1e-11 at D = 512, |ΔM⁻¹| ≤ 1e-13), while in Float32 the share of chains
    within 2e-3 falls from 0.999 (iteration 2) to 0.48 (D = 256) / 0.80 (D = 512) after the second window end: ONE shared estimate carries
    every chain that parted ways at a tie into the M⁻¹ of all chains (|ΔM⁻¹| 9e-6 after the first window, 6e-3 after the second), which a
    per-chain share rule cannot absorb.  That is the coupling a shared metric has by design, not a stale copy: §3 holds bit for bit."""
    f32 = dtype == np.float32
    n_adapts, n_samples, ib, tb, ws = 5, 6, 1, 1, 1     # six iterations as in that test; the shortest schedule with two window ends
    start, end, splits = reference_windows(n_adapts, ib, tb, ws)
    assert (start, splits) == (2, [2, 4])
    rs = np.random.default_rng([D, 8])
    P = _ar1_precision(D)
    th0 = np.asfortranarray(rs.normal(size=(D, N)))
    eps0 = 0.12 * (0.7 + 0.6 * rs.random(N))
    out = {}
    for engine in ("step", "epoch"):
        monkeypatch.setenv("AHMC_DENSE_EPOCH", "1" if engine == "epoch" else "0")
        monkeypatch.setenv("AHMC_DENSE_EPOCH_MIN", "32")
        lf = A.Leapfrog(eps0)
        k = _nuts(lf, max_depth=8)
        g = A.Engine(A.Hamiltonian(A.DenseEuclideanMetric(np.eye(D)), A.DenseGaussian(P)), N, dtype=dtype, rng=A.PhiloxRNG(78), lib=hip)
        g.set_integrator(lf)
        g.set_position(th0)
        g.adaptor_init(_stan_dense(D, lf, ib, tb, ws))
        ptr, fetch = _draw_buffer(hip, n_samples, N, D, dtype)
        minvs, first = [], 1
        for stop in splits + [n_samples]:
            g.run(k, stop, n_adapts, samples_out=ptr, i_first=first)
            g.sync()
            first = stop + 1
            if stop in splits:
                minvs.append(_minv(g).copy())
        draws = fetch()
        lo, refs = start, []
        for s, Mi in zip(splits, minvs):
            window = [np.asfortranarray(draws[i - 1].T) for i in range(lo, s + 1)]
            refs.append(_check_estimate(Mi, window, hip, f"warm-up {engine} engine D={D} window end {s}")[1:])
            lo = s + 1
        st = g.stats()
        out[engine] = (draws, st["n_steps"].copy(), g.accum()["total_n_steps"], g.get_stepsize().copy(), st["acceptance_rate"].copy(), g.theta().copy(), minvs, refs)
        if _is_hip(hip):
            assert (g.info("dense_epoch_launches") > 0) == (engine == "epoch"), (D, dtype, engine)
        g.close()
    a, b = out["step"], out["epoch"]
    for it in range(n_samples):   # (the figures, before anything is asserted)
        dd = np.abs(a[0][it] - b[0][it])
        print(f"D={D} {np.dtype(dtype).name} iteration {it + 1}: max |Δθ| = {dd.max():.3e}, chains within 2e-3: "
              f"{np.isclose(a[0][it], b[0][it], rtol=2e-3, atol=2e-3).all(axis=1).mean():.4f}, chains that moved: "
              f"{(a[0][it] != (a[0][it - 1] if it else th0.T.astype(dtype))).any(axis=1).mean():.3f}")
    # (dual averaging's first step size, 10·ϵ₀, is beyond the stability limit of this target: no chain moves in iteration 2, so window 1 holds
    # the draws of iteration 1 once more — a full-rank estimate all the same; the transitions after each window end do move)
    for s_ in splits:
        assert (a[0][s_] != a[0][s_ - 1]).any(axis=1).mean() > 0.5 and (b[0][s_] != b[0][s_ - 1]).any(axis=1).mean() > 0.5, s_
    for s_, Ma, Mb in zip(splits, a[6], b[6]):
        print(f"D={D} {np.dtype(dtype).name} window end {s_}: max |ΔM⁻¹| between the engines = {np.abs(Ma - Mb).max():.3e}")
    if not f32:
        # the two engines' M⁻¹ within the §2 bounds of each other: each bound on its own draws, plus what the exact estimates of the two
        # sets of draws differ by
        for s_, Ma, Mb, (ra, ba), (rb, bb) in zip(splits, a[6], b[6], a[7], b[7]):
            assert (np.abs(Ma.astype(LD) - Mb.astype(LD)) <= ba + bb + np.abs(ra - rb)).all(), f"M⁻¹ of the two engines at window end {s_}"
        np.testing.assert_array_equal(a[1], b[1])
        assert a[2] == b[2]
        np.testing.assert_allclose(a[3], b[3], rtol=1e-9)
        np.testing.assert_allclose(a[4], b[4], rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(a[0], b[0], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(a[5], b[5], rtol=1e-9, atol=1e-9)
    else:
        same = a[1] == b[1]
        on = same & np.isclose(a[5], b[5], rtol=2e-3, atol=2e-3).all(axis=0)
        assert on.mean() >= 0.97, (D, on.mean())
        np.testing.assert_allclose(a[3][on], b[3][on], rtol=1e-3)
        np.testing.assert_allclose(a[0][-2:][:, on, :], b[0][-2:][:, on, :], rtol=1e-2, atol=1e-2)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("D", [12, 65])
def test_dense_warmup_against_the_oracle_through_a_window_end(hip, oracle, D, dtype):
    """HIP against the oracle, NUTS + StanHMCAdaptor with a dense adaptor, through the first window end and the four transitions after it,
    margin-aware.  Every transition starts from a common restart (the oracle's θ and ϵ on both sides) and `adapt` gets the oracle's (θ, α) on
    both sides, so the two adaptor states see the same sequence; the two M⁻¹ estimates differ by rounding (each is held to its own bound
    here), so after the window end the oracle's M⁻¹ is set on both sides before the transitions that follow."""
    N, n_adapts, ib, tb, ws = 64, 30, 3, 3, 5
    start, end, splits = reference_windows(n_adapts, ib, tb, ws)
    assert splits == [8, 27]
    rs = np.random.default_rng([D, 6])
    P = _ar1_precision(D)
    th0 = np.asfortranarray(rs.normal(size=(D, N)).astype(dtype))
    engines = []
    for lib in (hip, oracle):
        lf = A.Leapfrog(np.full(N, 0.2))
        e = A.Engine(A.Hamiltonian(A.DenseEuclideanMetric(np.eye(D)), A.DenseGaussian(P)), N, dtype=dtype, rng=A.PhiloxRNG(41), lib=lib)
        e.set_integrator(lf)
        e.set_position(th0)
        e.adaptor_init(_stan_dense(D, lf, ib, tb, ws))
        engines.append(e)
    g, o = engines
    k = _nuts(A.Leapfrog(np.full(N, 0.2)), max_depth=6)
    PU.reset_margin(o)
    window = []
    tol = 1e-8 if dtype == np.float64 else 2e-3
    updated = False
    for i in range(1, splits[0] + 5):
        g.set_position(o.theta())
        g.set_integrator(A.Leapfrog(o.get_stepsize()))
        for e in (g, o):
            e.transition(k)
        sg, so = g.stats(), o.stats()
        same = (sg["n_steps"] == so["n_steps"]) & (sg["is_accept"] == so["is_accept"]) & (sg["tree_depth"] == so["tree_depth"])
        same = PU.check_flips(same, PU.decision_margin(o), dtype, f"dense warm-up D={D} iteration {i}", n_steps=so["n_steps"])
        th, al = o.theta().copy(), so["acceptance_rate"].copy()
        np.testing.assert_allclose(g.theta()[:, same], th[:, same], rtol=tol, atol=tol, err_msg=f"θ after transition {i}")
        for e in (g, o):
            e.adapt(i, n_adapts, theta=th, alpha=al)
        np.testing.assert_allclose(g.get_stepsize(), o.get_stepsize(), rtol=1e-9 if dtype == np.float64 else 1e-4, err_msg=f"ϵ after adapt! {i}")
        if start <= i <= end:
            window.append(np.asfortranarray(th))
        if i == splits[0]:
            for e in (g, o):
                _check_estimate(_minv(e), window, e.lib, f"warm-up vs oracle D={D} window end {i} ({e.lib.backend.split(':')[0]})")
            g.set_metric(A.DenseEuclideanMetric(_minv(o)))
            updated = True
        elif not updated:
            np.testing.assert_array_equal(_minv(g), np.eye(D, dtype=dtype))
    assert updated
    for e in engines:
        e.close()
