"""The generalised-linear-model target of include/ahmc_glm.h in numpy float64: the definition the device kernels
(csrc/ahmc_glm.hpp) are held to.

    η = X·θ + offset                 X (n_obs, D), y / offset (n_obs), prior precision p (D) >= 0, θ (D, N): a chain per column
    ℓπ(θ) = Σ_i ℓ(y_i, η_i) − ½ Σ_d p_d θ_d²
    ∇ℓπ   = Xᵀu − p∘θ                u_i = ∂ℓ/∂η_i            (the engine carries g = −∇ℓπ)

Families (terms that do not depend on θ are dropped):
    "bernoulli_logit"    ℓ = yη − softplus(η),  u = y − σ(η);  softplus(η) = max(η, 0) + log1p(exp(−|η|)), σ from the same exp(−|η|)
    "poisson_log"        ℓ = yη − exp(η),       u = y − exp(η)
    "gaussian_identity"  u = scale·(y − η),     ℓ = (−½·u)·(y − η);  scale = 1/σ²

Order of the sums — what fixes a chain's bits on the device, whatever N, the chain's column, the chain list or the tile shape:
  * η_i: the k-ordered fma chain  fma(X[i,D−1], θ[D−1], … fma(X[i,0], θ[0], 0))  (tests/host_ref/glm_ref.cpp), then + offset_i once;
  * Σ_i ℓ: observations in blocks of ROW_BLOCK; within a block ascending from 0 (`block_sums`); the blocks lane-strided over 64
    lanes, each lane ascending, then the wave's butterfly (ahmc_device.hpp: wave_allsum2);
  * Xᵀu: observations in slices of K_SLICE; within a slice the k-ordered fma chain, the slice sums added in ascending order;
    g_d = fma(p_d, θ_d, −Σ_slices);
  * ½ Σ p_d θ_d²: lane-strided fma((p_d·θ_d), θ_d, ·), then the same butterfly;  ℓπ = fma(−½, Σ_prior, Σ_ℓ).
The functions below follow the block and slice structure; numpy's own dot products stand in for the fma chains.
"""
import numpy as np

BERNOULLI_LOGIT, POISSON_LOG, GAUSSIAN_IDENTITY = 0, 1, 2
FAMILIES = {"bernoulli_logit": BERNOULLI_LOGIT, "poisson_log": POISSON_LOG, "gaussian_identity": GAUSSIAN_IDENTITY}
ROW_BLOCK = 64    # observations whose ℓ one workgroup sums (GB_M of csrc/ahmc_dense.hpp)
K_SLICE = 1024    # observations per slice of Xᵀu (GLM_K_SLICE of csrc/ahmc_glm.hpp)


def family_code(family):
    if isinstance(family, str):
        if family not in FAMILIES:
            raise ValueError(f"unknown GLM family {family!r}: one of {sorted(FAMILIES)}")
        return FAMILIES[family]
    if int(family) not in FAMILIES.values():
        raise ValueError(f"unknown GLM family {family!r}")
    return int(family)


def link(family, y, eta, scale=1.0):
    """(ℓ(y, η), u = ∂ℓ/∂η) elementwise; y broadcasts against η"""
    fam = family_code(family)
    eta = np.asarray(eta, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        if fam == BERNOULLI_LOGIT:
            e = np.exp(-np.abs(eta))
            sp = np.where(eta > 0, eta, 0.0) + np.log1p(e)
            d = 1.0 + e
            sig = np.where(eta >= 0, 1.0 / d, e / d)
            return y * eta - sp, y - sig
        if fam == POISSON_LOG:
            ex = np.exp(eta)
            return y * eta - ex, y - ex
        r = y - eta
        u = scale * r
        return (-0.5 * u) * r, u


def _theta(X, theta):
    X = np.asarray(X, dtype=np.float64)
    th = np.asarray(theta, dtype=np.float64)
    vec = th.ndim == 1
    if vec:
        th = th.reshape(-1, 1)
    if X.ndim != 2 or th.shape[0] != X.shape[1]:
        raise ValueError(f"DimensionMismatch: X {X.shape}, θ {th.shape}")
    return X, th, vec


def linear_predictor(X, theta, offset=None):
    X, th, _ = _theta(X, theta)
    eta = X @ th
    if offset is not None:
        eta = eta + np.asarray(offset, dtype=np.float64).reshape(-1, 1)
    return eta


def pointwise(family, X, y, theta, offset=None, scale=1.0):
    """(η, ℓ(y_i, η_i)), each (n_obs, N): the mirror of ahmc_glm_pointwise"""
    eta = linear_predictor(X, theta, offset)
    ll, _ = link(family, np.asarray(y, dtype=np.float64).reshape(-1, 1), eta, scale)
    return eta, ll


def block_sums(ll):
    """Σ ℓ over each block of ROW_BLOCK observations, ascending within the block: (n_blocks, N)"""
    n = ll.shape[0]
    nb = (n + ROW_BLOCK - 1) // ROW_BLOCK
    pad = np.zeros((nb * ROW_BLOCK,) + ll.shape[1:])   # (rows past n_obs add +0, as on the device)
    pad[:n] = ll
    return np.add.accumulate(pad.reshape((nb, ROW_BLOCK) + ll.shape[1:]), axis=1)[:, -1]


def sanitize(lp):
    """PhasePoint: a non-finite ℓπ is −Inf (src/hamiltonian.jl:95-104)"""
    lp = np.asarray(lp, dtype=np.float64)
    return np.where(np.isfinite(lp), lp, -np.inf)


def logdensity(family, X, y, theta, offset=None, prior_prec=None, scale=1.0):
    """(ℓπ (N,), ∇ℓπ (D, N)) at θ (D, N) — with the model bound (functools.partial, a lambda) the callback of an ExternalTarget.
    ℓπ is returned as computed: an overflowing Poisson gives a non-finite value, which the engine sanitises (`sanitize`)."""
    X, th, _ = _theta(X, theta)
    p = np.zeros(X.shape[1]) if prior_prec is None else np.asarray(prior_prec, dtype=np.float64).ravel()
    eta = linear_predictor(X, th, offset)
    ll, u = link(family, np.asarray(y, dtype=np.float64).reshape(-1, 1), eta, scale)
    with np.errstate(over="ignore", invalid="ignore"):
        lsum = block_sums(ll).sum(axis=0)
        xtu = np.zeros_like(th)
        for k0 in range(0, X.shape[0], K_SLICE):
            xtu = xtu + X[k0:k0 + K_SLICE].T @ u[k0:k0 + K_SLICE]
        pt = p.reshape(-1, 1) * th
        lp = lsum - 0.5 * (pt * th).sum(axis=0)
        grad = xtu - pt
    return lp, grad
