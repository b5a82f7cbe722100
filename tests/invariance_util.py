"""Exact-invariance testing: chains STARTED from the target must still be distributed as the target after any number of transitions.

Draw N starting points i.i.d. from π (every built-in family, the banana of tests/user_targets/banana.hpp and the Gaussian GLM posterior
can be sampled exactly on the host), give every chain its own Philox stream, apply T transitions of a kernel that leaves π invariant:
the N end points are again N i.i.d. draws from π — for ANY step size, tree depth or number of divergences.  Each family comes with a
whitening map θ → z under which z is i.i.d. N(0, 1), so every statistic of `battery` has an exactly known null distribution and the
tolerance is a false-alarm probability (ALPHA), not a measured number.  Nothing here imports the engine.

Two facts a user of this module needs:
  * `Engine.refresh()` does not advance the iteration counter, so a transition after it draws the SAME (chain, iteration, momentum)
    normals: with PartialMomentumRefreshment(α) it starts from r = (α + √(1 − α²))·ξ, variance 1.78 at α = 0.9.  A stationary momentum is
    handed in with `set_position(θ, r)`, r ~ N(0, M) from numpy (the Momentum* classes below).
  * two kernels of the reference are NOT invariant and are on no list: static HMC with PartialMomentumRefreshment and
    static MultinomialTS with TemperedLeapfrog.  Static MultinomialTS also couples the chains through one forward / backward split per
    transition (Q4): its configurations pass at the lists' N, the battery sees the coupling at 262 144 chains.
    tests/test_exact_invariance.py pins all three on the oracle.
"""
import math

import numpy as np
import torch

ALPHA = 1e-6          # false-alarm probability of one TEST (all of its checks together: each is held to ALPHA / m)
KS_MAX_COORDS = 64    # KS against Φ on at most this many coordinates
WAVE_ELEMS = 512      # coordinates one wave of a multi-wave chain holds (64 lanes × E = 8: every geometry with G > 64)


# ---------------------------------------------------------------------------------------------------------------------
# tail probabilities (float64; torch is what the GPU tests import anyway, scipy / mpmath may be absent there)
# ---------------------------------------------------------------------------------------------------------------------
def normal_two_sided(z):
    """P(|Z| >= |z|), Z ~ N(0, 1)"""
    z = np.atleast_1d(np.asarray(z, dtype=np.float64))
    return np.array([math.erfc(abs(v) / math.sqrt(2.0)) for v in z])


def chi2_tails(x, k):
    """(P(X <= x), P(X >= x)) for X ~ χ²_k; x an array, k a scalar or an array"""
    x = torch.as_tensor(np.atleast_1d(np.asarray(x, dtype=np.float64)))
    a = torch.as_tensor(np.broadcast_to(np.asarray(k, dtype=np.float64) / 2.0, x.shape).copy())
    return torch.special.gammainc(a, x / 2).numpy(), torch.special.gammaincc(a, x / 2).numpy()


def chi2_two_sided(x, k):
    lo, hi = chi2_tails(x, k)
    return np.minimum(1.0, 2.0 * np.minimum(lo, hi))


def normal_cdf(z):
    return torch.special.ndtr(torch.as_tensor(np.asarray(z, dtype=np.float64))).numpy()


def chi2_cdf(x, k):
    return chi2_tails(x, k)[0]


def kolmogorov_sf(lam):
    """Q(λ) = 2 Σ_{k>=1} (−1)^{k−1} exp(−2k²λ²), the asymptotic distribution of √n·D_n"""
    if lam < 0.27:      # 1 − Q(0.27) < 1e-10, and the alternating series converges slowly below
        return 1.0
    s = 0.0
    for k in range(1, 101):
        t = math.exp(-2.0 * k * k * lam * lam)
        s += t if k % 2 else -t
        if t < 1e-300:
            break
    return min(1.0, max(0.0, 2.0 * s))


def ks_pvalue(d, n):
    """two-sided one-sample KS: the Kolmogorov series at Stephens' (√n + 0.12 + 0.11/√n)·D — the one approximate null here (n >= 1024)"""
    rn = math.sqrt(n)
    return kolmogorov_sf((rn + 0.12 + 0.11 / rn) * d)


def ks_statistic(u):
    """sup |F_n − F| per row of `u` = F(sample), shape (m, n)"""
    u = np.sort(np.atleast_2d(u), axis=1)
    n = u.shape[1]
    i = np.arange(1, n + 1, dtype=np.float64)
    return np.maximum((i / n - u).max(axis=1), (u - (i - 1) / n).max(axis=1))


def ks_coordinates(D):
    """the fixed subset of coordinates that get a KS test: all of them up to 64; beyond, 64 that always hold 0, 1, 63, 64, D − 1 and the
    first and last coordinate of every wave of a multi-wave chain (a wave holds WAVE_ELEMS consecutive coordinates), the rest spread evenly"""
    if D <= KS_MAX_COORDS:
        return np.arange(D)
    must = {0, 1, 63, 64, D - 1}
    if D > WAVE_ELEMS:
        for w in range((D + WAVE_ELEMS - 1) // WAVE_ELEMS):
            must.add(w * WAVE_ELEMS)
            must.add(min(D, (w + 1) * WAVE_ELEMS) - 1)
    assert len(must) <= KS_MAX_COORDS
    for d in np.linspace(0, D - 1, KS_MAX_COORDS - len(must) + 2)[1:-1].astype(int):   # deterministic fill, evenly spread
        must.add(int(d))
    d = 2
    while len(must) < KS_MAX_COORDS:   # (a fill point fell on a fixed one)
        must.add(d)
        d += 1
    return np.array(sorted(must))


# ---------------------------------------------------------------------------------------------------------------------
# the battery
# ---------------------------------------------------------------------------------------------------------------------
def battery_checks(z, label=""):
    """Every check of one whitened (D, N) array, as (name, standardised statistic, two-sided p).  Under the null z is i.i.d. N(0, 1):
         mean[d]   √N·z̄_d ~ N(0, 1)                        sumsq[d]  Σ_c z² ~ χ²_N
         total     Σ z² ~ χ²_{DN} (= N × the mean of q)      q_ks      KS of q_c = Σ_d z² against χ²_D
         ks[d]     KS of coordinate d against Φ (ks_coordinates(D))
       A non-finite entry fails outright: no chain is left out of any statistic."""
    z = np.asarray(z, dtype=np.float64)
    assert z.ndim == 2 and z.shape[1] >= 1024, z.shape
    assert np.isfinite(z).all(), f"{label}: {int((~np.isfinite(z)).any(axis=0).sum())} chains hold a non-finite value"
    D, N = z.shape
    out = []
    zm = math.sqrt(N) * z.mean(axis=1)
    out += [(f"{label}mean[{d}]", float(zm[d]), float(p)) for d, p in enumerate(normal_two_sided(zm))]
    z2 = z * z
    ss = z2.sum(axis=1)
    out += [(f"{label}sumsq[{d}]", float((ss[d] - N) / math.sqrt(2.0 * N)), float(p)) for d, p in enumerate(chi2_two_sided(ss, N))]
    q = z2.sum(axis=0)
    tot = float(q.sum())
    out.append((f"{label}total", (tot - D * N) / math.sqrt(2.0 * D * N), float(chi2_two_sided(tot, D * N)[0])))
    dq = float(ks_statistic(chi2_cdf(q, D))[0])
    out.append((f"{label}q_ks", dq * math.sqrt(N), ks_pvalue(dq, N)))
    coords = ks_coordinates(D)
    dk = ks_statistic(normal_cdf(z[coords]))
    out += [(f"{label}ks[{int(d)}]", float(v) * math.sqrt(N), ks_pvalue(float(v), N)) for d, v in zip(coords, dk)]
    return out


def verdict(checks, alpha=ALPHA):
    """all checks of ONE test: it passes when every p >= alpha / m"""
    m = len(checks)
    worst = min(checks, key=lambda c: c[2])
    zs = [c for c in checks if "ks" not in c[0]]
    wz = max(zs, key=lambda c: abs(c[1])) if zs else worst
    failed = [c for c in checks if not c[2] >= alpha / m]
    return {"ok": not failed, "m": m, "alpha": alpha, "threshold": alpha / m, "min_p": worst[2], "min_p_check": worst[0],
            "worst_z": wz[1], "worst_z_check": wz[0], "failed": failed[:8], "n_failed": len(failed)}


def battery(arrays, alpha=ALPHA):
    """`arrays`: {label: whitened (D, N)} — all of one test's arrays share its ALPHA"""
    checks = []
    for label, z in arrays.items():
        checks += battery_checks(z, label + ".")
    return verdict(checks, alpha)


# ---------------------------------------------------------------------------------------------------------------------
# exact samplers and whiteners: family.draw(N, rng) -> θ0 (D, N), family.whiten(θ) -> z (D, N) i.i.d. N(0, 1) under π
# ---------------------------------------------------------------------------------------------------------------------
class Iso:
    name = "iso"

    def __init__(self, D):
        self.D = D

    def draw(self, N, rng):
        return rng.standard_normal((self.D, N))

    def whiten(self, th):
        return np.asarray(th, dtype=np.float64)


class Diag:
    """x_d ~ N(m_d, s_d²)"""
    name = "diag"

    def __init__(self, D, seed=1):
        rs = np.random.default_rng(seed)
        self.D, self.m, self.s = D, rs.normal(size=D), 0.5 + 1.5 * rs.random(D)

    def draw(self, N, rng):
        return self.m[:, None] + self.s[:, None] * rng.standard_normal((self.D, N))

    def whiten(self, th):
        return (np.asarray(th, dtype=np.float64) - self.m[:, None]) / self.s[:, None]


class Funnel:
    """y ~ N(0, 3²), x_d | y ~ N(0, e^y)"""
    name = "funnel"

    def __init__(self, D):
        self.D = D

    def draw(self, N, rng):
        xi = rng.standard_normal((self.D, N))
        y = 3.0 * xi[0]
        th = xi * np.exp(y / 2)
        th[0] = y
        return th

    def whiten(self, th):
        th = np.asarray(th, dtype=np.float64)
        z = th * np.exp(-th[0] / 2)
        z[0] = th[0] / 3.0
        return z


class Hier:
    """μ, log τ ~ N(0, 1), x_d ~ N(μ, τ²)"""
    name = "hier"

    def __init__(self, D):
        assert D >= 3
        self.D = D

    def draw(self, N, rng):
        th = rng.standard_normal((self.D, N))
        th[2:] = th[0] + np.exp(th[1]) * th[2:]
        return th

    def whiten(self, th):
        z = np.array(th, dtype=np.float64)
        z[2:] = (z[2:] - z[0]) * np.exp(-z[1])
        return z


class GaussianByPrecision:
    """θ ~ N(mean, P⁻¹), P = LLᵀ: z = Lᵀ(θ − mean)"""

    def __init__(self, P, mean=None):
        self.P = np.asarray(P, dtype=np.float64)
        self.D = self.P.shape[0]
        self.mean = np.zeros(self.D) if mean is None else np.asarray(mean, dtype=np.float64)
        self.L = np.linalg.cholesky(self.P)

    def draw(self, N, rng):
        return self.mean[:, None] + np.linalg.solve(self.L.T, rng.standard_normal((self.D, N)))

    def whiten(self, th):
        return self.L.T @ (np.asarray(th, dtype=np.float64) - self.mean[:, None])


class Dense(GaussianByPrecision):
    """ℓπ = −½ θᵀPθ with eigenvalues of P spread over [0.5, 2] in a random basis"""
    name = "dense"

    def __init__(self, D, seed=2):
        rs = np.random.default_rng(seed)
        Q, _ = np.linalg.qr(rs.normal(size=(D, D)))
        P = (Q * np.linspace(0.5, 2.0, D)) @ Q.T
        super().__init__((P + P.T) / 2)


class Banana:
    """tests/user_targets/banana.hpp: per pair (x, y) = (θ_2k, θ_2k+1): x ~ N(a, 1), y | x ~ N(x², 1/(2b)); an unpaired last one ~ N(0, 1)"""
    name = "banana"

    def __init__(self, D, a=0.5, b=0.5):
        self.D, self.a, self.b = D, a, b

    def draw(self, N, rng):
        th = rng.standard_normal((self.D, N))
        m = self.D // 2
        th[0:2 * m:2] += self.a
        th[1:2 * m:2] = th[0:2 * m:2] ** 2 + th[1:2 * m:2] / math.sqrt(2 * self.b)
        return th

    def whiten(self, th):
        z = np.array(th, dtype=np.float64)
        m = self.D // 2
        z[1:2 * m:2] = (z[1:2 * m:2] - z[0:2 * m:2] ** 2) * math.sqrt(2 * self.b)
        z[0:2 * m:2] -= self.a
        return z


class GaussianGLM(GaussianByPrecision):
    """the `gaussian_identity` GLM posterior: ℓπ = −½·scale·|y − Xθ − offset|² − ½ Σ p_d θ_d², i.e. precision scale·XᵀX + diag(p) and the
    mean of the normal equations P·mean = scale·Xᵀ(y − offset)"""
    name = "glm"

    def __init__(self, D, n_obs=200, seed=3, scale=1.7):
        rs = np.random.default_rng(seed)
        self.X = rs.normal(size=(n_obs, D)) / math.sqrt(n_obs)
        self.offset = 0.3 * rs.normal(size=n_obs)
        self.prior_prec = 0.5 + 2.0 * rs.random(D)
        self.y = self.X @ rs.normal(size=D) + self.offset + rs.normal(size=n_obs) / math.sqrt(scale)
        self.scale = scale
        P = scale * self.X.T @ self.X + np.diag(self.prior_prec)
        super().__init__(P, np.linalg.solve(P, scale * self.X.T @ (self.y - self.offset)))


FAMILIES = {"iso": Iso, "diag": Diag, "funnel": Funnel, "hier": Hier, "dense": Dense, "banana": Banana, "glm": GaussianGLM}


# ---------------------------------------------------------------------------------------------------------------------
# momenta: r0 ~ N(0, M) and the whitening of r, for every metric (given as M⁻¹)
# ---------------------------------------------------------------------------------------------------------------------
class MomentumUnit:
    def __init__(self, D):
        self.D = D

    def draw(self, N, rng):
        return rng.standard_normal((self.D, N))

    def whiten(self, r):
        return np.asarray(r, dtype=np.float64)


class MomentumDiag:
    """M⁻¹ diagonal: shared (D,) or per chain (D, N)"""

    def __init__(self, minv):
        minv = np.asarray(minv, dtype=np.float64)
        self.sq = np.sqrt(minv if minv.ndim == 2 else minv[:, None])
        self.D = minv.shape[0]

    def draw(self, N, rng):
        return rng.standard_normal((self.D, N)) / self.sq

    def whiten(self, r):
        return np.asarray(r, dtype=np.float64) * self.sq


class MomentumDense:
    """M⁻¹ = CCᵀ dense: rᵀM⁻¹r = |Cᵀr|²"""

    def __init__(self, Minv):
        self.C = np.linalg.cholesky(np.asarray(Minv, dtype=np.float64))
        self.D = self.C.shape[0]

    def draw(self, N, rng):
        return np.linalg.solve(self.C.T, rng.standard_normal((self.D, N)))

    def whiten(self, r):
        return self.C.T @ np.asarray(r, dtype=np.float64)


def momentum_rank_update(a, B, Dk):
    """M⁻¹ = diag(a) + B·Dk·Bᵀ written out as a dense matrix: a reading of the metric that does not go through rank_update.py"""
    a, B, Dk = (np.asarray(x, dtype=np.float64) for x in (a, B, Dk))
    return MomentumDense(np.diag(a) + B @ Dk @ B.T)


# ---------------------------------------------------------------------------------------------------------------------
# a plain numpy static HMC (unit metric, EndPoint, full refreshment) — the non-vacuity tests plant defects in it
# ---------------------------------------------------------------------------------------------------------------------
def funnel_logp_grad(th):
    y = th[0]
    ey = np.exp(-y)
    ss = (th[1:] ** 2).sum(axis=0)
    nm1 = th.shape[0] - 1
    lp = -y * y / 18 - nm1 * y / 2 - ss * ey / 2
    g = -th * ey
    g[0] = -y / 9 - nm1 / 2 + ss * ey / 2
    return lp, g


def numpy_static_hmc(logp_grad, th, eps, L, T, rng, kinetic_weight=1.0):
    """T transitions of static HMC on all columns of `th`, transition t at eps[t % len(eps)]; `kinetic_weight` ≠ 1 mis-weights the kinetic energy IN THE ACCEPT TEST only
    (the planted defect).  Returns (θ_T, mean acceptance probability)."""
    th = th.copy()
    acc = 0.0
    eps_all = eps if isinstance(eps, tuple) else (eps,)
    for t in range(T):
        eps = eps_all[t % len(eps_all)]
        r = rng.standard_normal(th.shape)
        lp, g = logp_grad(th)
        h0 = -lp + kinetic_weight * 0.5 * (r * r).sum(axis=0)
        x = th.copy()
        with np.errstate(over="ignore", invalid="ignore"):
            for _ in range(L):
                r = r + 0.5 * eps * g
                x = x + eps * r
                lpn, g = logp_grad(x)
                r = r + 0.5 * eps * g
            h1 = -lpn + kinetic_weight * 0.5 * (r * r).sum(axis=0)
            a = np.exp(np.minimum(0.0, h0 - h1))
        a = np.where(np.isfinite(h1), a, 0.0)
        take = rng.random(th.shape[1]) < a
        th[:, take] = x[:, take]
        acc += a.mean()
    return th, acc / T
