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


# ------------------------------------------------------------------------------------------------------------------------------
# include/ahmc_glm_hier.h: coefficient groups whose prior scale is sampled (csrc/ahmc_glm.hpp: k_hglm_coef, k_hglm_finish)
# ------------------------------------------------------------------------------------------------------------------------------
__doc__ += """
Coefficient groups whose prior scale is sampled (hier_logdensity, hier_coefficients, hier_pointwise):
    θ (D, N), D = P + G:  θ[0:P] coefficient parameters, θ[P + k] = s_k = log τ_k of group k = [lo_k, hi_k), m_k = hi_k − lo_k members
    w_d = θ_d (fixed and centred coefficients),  w_d = exp(s_k)·θ_d (members of a non-centred group: θ_d is the standardised z_d)
    η = X·W + offset,  (ℓ, u) from `link`,  R = −Xᵀu (P, N)
    h_k = s_k − ½·e^{2s_k}/A_k²,  h′_k = 1 − e^{2s_k}/A_k²           τ_k ~ half-normal(A_k) with the Jacobian of s = log τ
    ℓπ = Σ_i ℓ − ½ Σ_fixed p_d θ_d² + Σ_k [h_k + b_k],   b_k = −m_k·s_k − ½·q_k·S_k (centred)  or  −½·S_k (non-centred)
    q_k = e^{−2s_k},  S_k = Σ_{d∈k} θ_d²,  T_k = Σ_{d∈k} R_d·w_d
    g = −∇ℓπ:  fixed fma(p_d, θ_d, R_d);  centred member fma(q_k, θ_d, R_d);  non-centred member fma(τ_k, R_d, θ_d);
               s_k centred  fma(−q_k, S_k, m_k) − h′_k;   s_k non-centred  T_k − h′_k

Order of the new sums and operations (what fixes a chain's bits on the device; X·W and Xᵀu keep the orders of the header above
with θ := W, D := P, p := 0, so R = fma(0, w, −Σ_slices)):
  * τ_k = exp(s_k): one exp per (chain, group); e^{2s_k} = exp(2·s_k) and q_k = exp(−2·s_k) are exps of their own (2·s is exact);
  * S_k and T_k: lane-strided over 64 lanes from lo_k — lane l takes lo_k + l, lo_k + l + 64, … ascending, S = fma(θ_d, θ_d, S),
    T = fma(R_d, w_d, T) — then wave_allsum2 of the pair (S_k, T_k);
  * h_k = fma(−½·e^{2s_k}, 1/A_k², s_k),  h′_k = fma(−e^{2s_k}, 1/A_k², 1),  b_k = fma(−m_k, s_k, (−½·q_k)·S_k)  or  −½·S_k;
  * ℓπ = fma(−½, Σ_prior, Σ_ℓ) as before — Σ_ℓ and Σ p_d θ_d² in the existing orders over d < P, members counting with p_d = 0 —
    then ℓπ += (h_k + b_k) for k ascending.
`hier_logdensity` follows this structure; numpy's sums stand in for the lane-strided fma chains and the butterfly.
"""

HGLM_MAX_GROUPS = 32   # AHMC_HGLM_MAX_GROUPS


def check_groups(groups, P):
    """groups as a list of (lo, hi, centered, A): ascending, disjoint, inside [0, P), non-empty, A finite and > 0"""
    out, prev = [], 0
    for k, grp in enumerate(groups):
        lo, hi, cen, A = (grp.start, grp.stop, grp.centered, grp.scale) if hasattr(grp, "start") else grp
        lo, hi, cen, A = int(lo), int(hi), bool(cen), float(A)
        if not (0 <= lo < hi <= P):
            raise ValueError(f"ArgumentError: group {k + 1} = [{lo}, {hi}) is empty or outside [0, {P})")
        if lo < prev:
            raise ValueError(f"ArgumentError: group {k + 1} = [{lo}, {hi}) overlaps the group before it or is out of order")
        if not (np.isfinite(A) and A > 0):
            raise ValueError(f"DomainError: group {k + 1}: hyper-scale {A} must be finite and > 0")
        prev = hi
        out.append((lo, hi, cen, A))
    if len(out) > HGLM_MAX_GROUPS:
        raise ValueError(f"ArgumentError: {len(out)} groups; at most {HGLM_MAX_GROUPS}")
    return out


def _hier_theta(theta, P, groups):
    th = np.asarray(theta, dtype=np.float64)
    if th.ndim == 1:
        th = th.reshape(-1, 1)
    groups = check_groups(groups, P)
    if th.shape[0] != P + len(groups):
        raise ValueError(f"DimensionMismatch: θ {th.shape}, P + G = {P} + {len(groups)}")
    return th, groups


def hier_coefficients(theta, P, groups):
    """(β (P, N), τ (G, N)): the coefficients on the model's own scale (β = W) and the group scales, from draws θ (P + G, N) —
    the mirror of ahmc_hglm_coefficients"""
    th, groups = _hier_theta(theta, P, groups)
    with np.errstate(over="ignore", invalid="ignore"):
        tau = np.exp(th[P:])
        W = th[:P].copy()
        for k, (lo, hi, cen, _) in enumerate(groups):
            if not cen:
                W[lo:hi] = tau[k] * th[lo:hi]
    return W, tau


def hier_pointwise(family, X, y, theta, groups, offset=None, scale=1.0):
    """(η, ℓ(y_i, η_i)), each (n_obs, N): `pointwise` at the effective coefficients W"""
    X = np.asarray(X, dtype=np.float64)
    W, _ = hier_coefficients(theta, X.shape[1], groups)
    return pointwise(family, X, y, W, offset, scale)


def hier_logdensity(family, X, y, theta, groups, offset=None, prior_prec=None, scale=1.0):
    """(ℓπ (N,), ∇ℓπ (P + G, N)) at θ (P + G, N).  `prior_prec` (P) covers the coefficients in no group and must be 0 on members.
    ℓπ is returned as computed (`sanitize` makes a non-finite value −Inf, as the engine does)."""
    X = np.asarray(X, dtype=np.float64)
    P = X.shape[1]
    th, groups = _hier_theta(theta, P, groups)
    p = np.zeros(P) if prior_prec is None else np.asarray(prior_prec, dtype=np.float64).ravel()
    for lo, hi, _, _ in groups:
        if np.any(p[lo:hi] != 0):
            raise ValueError(f"ArgumentError: prior_prec must be 0 on the members of a group ([{lo}, {hi}))")
    if not groups:
        return logdensity(family, X, y, th, offset, p, scale)
    W, tau = hier_coefficients(th, P, groups)
    eta = linear_predictor(X, W, offset)
    ll, u = link(family, np.asarray(y, dtype=np.float64).reshape(-1, 1), eta, scale)
    with np.errstate(over="ignore", invalid="ignore"):
        lsum = block_sums(ll).sum(axis=0)
        xtu = np.zeros_like(W)
        for k0 in range(0, X.shape[0], K_SLICE):
            xtu = xtu + X[k0:k0 + K_SLICE].T @ u[k0:k0 + K_SLICE]
        R = -xtu
        b = th[:P]
        pt = p.reshape(-1, 1) * b
        lp = lsum - 0.5 * (pt * b).sum(axis=0)
        g = np.empty_like(th)
        g[:P] = pt + R
        for k, (lo, hi, cen, A) in enumerate(groups):
            s = th[P + k]
            ia2 = 1.0 / (A * A)
            e2 = np.exp(2.0 * s)
            S = (b[lo:hi] * b[lo:hi]).sum(axis=0)
            h = s - 0.5 * e2 * ia2
            hp = 1.0 - e2 * ia2
            if cen:
                q = np.exp(-2.0 * s)
                bk = -(hi - lo) * s + (-0.5 * q) * S
                g[lo:hi] = q * b[lo:hi] + R[lo:hi]
                g[P + k] = ((hi - lo) - q * S) - hp
            else:
                bk = -0.5 * S
                g[lo:hi] = tau[k] * R[lo:hi] + b[lo:hi]
                g[P + k] = (R[lo:hi] * W[lo:hi]).sum(axis=0) - hp
            lp = lp + (h + bk)
    return lp, -g
