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
import math

import numpy as np

BERNOULLI_LOGIT, POISSON_LOG, GAUSSIAN_IDENTITY = 0, 1, 2
GAUSSIAN_IDENTITY_SIGMA, NEGBINOMIAL_LOG = 3, 4   # include/ahmc_glm_aux.h: a sampled dispersion (the section at the end)
FAMILIES = {"bernoulli_logit": BERNOULLI_LOGIT, "poisson_log": POISSON_LOG, "gaussian_identity": GAUSSIAN_IDENTITY,
            "gaussian_identity_sigma": GAUSSIAN_IDENTITY_SIGMA, "negbinomial_log": NEGBINOMIAL_LOG}
AUX_FAMILIES = (GAUSSIAN_IDENTITY_SIGMA, NEGBINOMIAL_LOG)
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


def link(family, y, eta, scale=1.0, s=None):
    """(ℓ(y, η), u = ∂ℓ/∂η) elementwise; y broadcasts against η.  The families with a sampled dispersion take its log `s`
    (broadcast against η: one value per chain) and return a third value, ∂ℓ/∂s."""
    fam = family_code(family)
    eta = np.asarray(eta, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if fam in AUX_FAMILIES:
        if s is None:
            raise ValueError(f"ArgumentError: family {fam} needs s, the log of its dispersion")
        return _aux_link(fam, y, eta, np.asarray(s, dtype=np.float64))
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


def pointwise(family, X, y, theta, offset=None, scale=1.0, factors=None):
    """(η, ℓ(y_i, η_i)), each (n_obs, N): the mirror of ahmc_glm_pointwise.  A family with a sampled dispersion takes it from θ's
    last row (θ then has one row more than X has columns).  `factors`: index-coded factors (the section at the end)."""
    fam = family_code(family)
    if fam in AUX_FAMILIES or factors:
        return _link_at(fam, *_hier_pointwise_args(fam, X, theta, (), factors), y, offset, scale)[2:4]
    X, th, _ = _theta(X, theta)
    return _link_at(fam, X, th, [], [], y, offset, scale)[2:4]


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


def logdensity(family, X, y, theta, offset=None, prior_prec=None, scale=1.0, aux_prior=None, factors=None):
    """(ℓπ (N,), ∇ℓπ (D, N)) at θ (D, N) — with the model bound (functools.partial, a lambda) the callback of an ExternalTarget.
    ℓπ is returned as computed: an overflowing Poisson gives a non-finite value, which the engine sanitises (`sanitize`).
    `aux_prior` = (loc, scale) belongs to the families with a sampled dispersion (θ then has D + 1 rows)."""
    if family_code(family) in AUX_FAMILIES or aux_prior is not None or factors:
        return _logdensity(*_hier_args(family, X, theta, (), prior_prec, aux_prior, factors=factors), y, offset, scale)
    X, th, _ = _theta(X, theta)
    return _logdensity(family_code(family), X, th, [], _prior_prec(prior_prec, X.shape[1], []), None, [], y, offset, scale)


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


def hier_coefficients(theta, P, groups, factors=None):
    """(β (P, N), τ (G, N)): the coefficients on the model's own scale (β = W) and the group scales, from draws θ (P + G, N) —
    the mirror of ahmc_hglm_coefficients.  With `factors`, P counts the dense columns and the factors' levels are added to it."""
    P = P + sum(n_levels(f) for f in factors or ())
    th, groups = _hier_theta(theta, P, groups)
    with np.errstate(over="ignore", invalid="ignore"):
        tau = np.exp(th[P:])
        W = th[:P].copy()
        for k, (lo, hi, cen, _) in enumerate(groups):
            if not cen:
                W[lo:hi] = tau[k] * th[lo:hi]
    return W, tau


def hier_pointwise(family, X, y, theta, groups, offset=None, scale=1.0, factors=None):
    """(η, ℓ(y_i, η_i)), each (n_obs, N): `pointwise` at the effective coefficients W; the dispersion of a family that samples it
    comes from θ's last row"""
    fam = family_code(family)
    return _link_at(fam, *_hier_pointwise_args(fam, X, theta, groups, factors), y, offset, scale)[2:4]


def hier_logdensity(family, X, y, theta, groups, offset=None, prior_prec=None, scale=1.0, aux_prior=None, factors=None):
    """(ℓπ (N,), ∇ℓπ (P + G, N)) at θ (P + G, N).  `prior_prec` (P) covers the coefficients in no group and must be 0 on members.
    ℓπ is returned as computed (`sanitize` makes a non-finite value −Inf, as the engine does).  A family with a sampled dispersion
    has one more row, s, with the prior `aux_prior` = (loc, scale): `aux_logdensity`."""
    return _logdensity(*_hier_args(family, X, theta, groups, prior_prec, aux_prior, factors=factors), y, offset, scale)


def _hier_finish(th, W, tau, R, lsum, p, groups):
    """(ℓπ, g = −∇ℓπ) over the P + G rows of th from Σℓ and R = −Xᵀu: the arithmetic of k_hglm_finish"""
    P = W.shape[0]
    with np.errstate(over="ignore", invalid="ignore"):
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
    return lp, g


# ------------------------------------------------------------------------------------------------------------------------------
# include/ahmc_glm_aux.h: families whose dispersion is sampled (csrc/ahmc_glm.hpp: glm_link_aux, glm_gamma_diffs, k_hglm_finish<T, true>)
# ------------------------------------------------------------------------------------------------------------------------------
__doc__ += """
Families with a sampled dispersion (aux_logdensity; `link` with s; lgamma_diff, digamma_diff):
    θ (D, N), D = P + G + 1:  the P coefficient parameters, the G log group scales (G may be 0), and LAST s, the log of the family's
    dispersion parameter, with the prior s ~ Normal(m, A²) (a log-normal on σ or φ: no Jacobian term).
    "gaussian_identity_sigma"  σ = e^s:  r = y − η, q = exp(−2s), u = q·r, ℓ = fma(−½·u, r, −s), ∂ℓ/∂s = fma(u, r, −1)
    "negbinomial_log"          NB2, mean μ = e^η, variance μ + μ²/φ, φ = e^s, y >= 0 finite (not necessarily an integer):
        d = η − s, e = exp(−|d|), l = log1p(e), σ(d) and 1 − σ(d) both from the same e (1/(1+e), e/(1+e): no subtraction)
        sp = max(d, 0) + l = log(μ + φ) − s,   sn = max(−d, 0) + l = log(μ + φ) − η
        ℓ = fma(−y, sn, fma(−φ, sp, L)),  u = fma(−(y + φ), σ, y),  ∂ℓ/∂s = fma(φ, Ψ − sp, fma(−(y + φ), 1 − σ, φ))
        L = lgamma(y + φ) − lgamma(φ) (`lgamma_diff`),  Ψ = ψ(y + φ) − ψ(φ) (`digamma_diff`);  −lgamma(y + 1) is dropped.
    ℓπ = [the hierarchical ℓπ over the first P + G rows] − ½((s − m)/A)²,   g[D−1] = −Σ_i ∂ℓ/∂s + (s − m)/A²
L and Ψ are computed as differences (shift both arguments by 8 with the recurrence, then Stirling's series): with A = φ + 8,
B = A + y, z = y/A:
    L = fma(A − ½, log1p(z), y·(log B − 1)) + (S(B) − S(A)) − Σ_{j<8} log1p(y/(φ + j))
    Ψ = Σ_{j<8} (y/(φ + j))/(y + φ + j) + log1p(z) + (½·z)/B − (T(B) − T(A))
S(x) = Σ_k B_2k/(2k(2k−1)) x^{1−2k} and T(x) = Σ_k B_2k/(2k) x^{−2k}, eight terms each, by Horner's rule in 1/x² (fma); the sums over
j ascending.  y = 0 gives L = Ψ = 0 exactly for every finite φ > 0.  A φ that underflows to 0 makes y/φ infinite or NaN and one that
overflows makes (A − ½)·log1p(0) = ∞·0: either way ℓ is non-finite and ℓπ is sanitised to −Inf (a divergence).
Order of the new sums: Σ_i ∂ℓ/∂s exactly as Σ_i ℓ (`block_sums`, then lane-strided over the row blocks and the butterfly); the prior
of s is added to ℓπ after the groups' terms:  r = s − m, ℓπ = fma((−½/A²)·r, r, ℓπ), g[D−1] = fma(r, 1/A², −Σ ∂ℓ/∂s).
"""

_STIRLING_S = (1.0 / 12, -1.0 / 360, 1.0 / 1260, -1.0 / 1680, 1.0 / 1188, -691.0 / 360360, 1.0 / 156, -3617.0 / 122400)
_STIRLING_T = (1.0 / 12, -1.0 / 120, 1.0 / 252, -1.0 / 240, 1.0 / 132, -691.0 / 32760, 1.0 / 12, -3617.0 / 8160)
GAMMA_SHIFT = 8


def _horner(c, z2):
    acc = np.full_like(z2, c[-1])
    for ck in c[-2::-1]:
        acc = acc * z2 + z2.dtype.type(ck)
    return acc


def gamma_diffs(y, phi, dtype=np.float64):
    """(L, Ψ) = (lgamma(y + φ) − lgamma(φ), ψ(y + φ) − ψ(φ)) elementwise, y >= 0 and φ > 0 broadcast against each other; every
    operation in `dtype` (float64 defines the model; float32 is what a Float32 context's kernels are compared with)"""
    dt = np.dtype(dtype).type
    y, phi = np.broadcast_arrays(np.asarray(y, dtype=dt), np.asarray(phi, dtype=dt))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        A = phi + dt(GAMMA_SHIFT)
        B = A + y
        z = y / A
        lz = np.log1p(z)
        za, zb = dt(1) / A, dt(1) / B
        za2, zb2 = za * za, zb * zb
        dS = zb * _horner(_STIRLING_S, zb2) - za * _horner(_STIRLING_S, za2)
        dT = zb2 * _horner(_STIRLING_T, zb2) - za2 * _horner(_STIRLING_T, za2)
        sl = np.zeros_like(z)
        sp = np.zeros_like(z)
        pj = phi.copy()
        for j in range(GAMMA_SHIFT):
            t = y / pj
            sl = sl + np.log1p(t)
            sp = sp + t / (y + pj)
            pj = pj + dt(1)
        L = ((A - dt(0.5)) * lz + y * (np.log(B) - dt(1))) + dS - sl
        Psi = ((sp + lz) + (dt(0.5) * z) / B) - dT
    return L, Psi


def lgamma_diff(y, phi):
    """lgamma(y + φ) − lgamma(φ), computed as a difference: accurate when φ is large and exact 0 at y = 0"""
    return gamma_diffs(y, phi)[0]


def digamma_diff(y, phi):
    """ψ(y + φ) − ψ(φ), computed as a difference"""
    return gamma_diffs(y, phi)[1]


def _aux_link(fam, y, eta, s):
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if fam == GAUSSIAN_IDENTITY_SIGMA:
            r = y - eta
            u = np.exp(-2.0 * s) * r
            return (-0.5 * u) * r - s, u, u * r - 1.0
        phi = np.exp(s)
        d = eta - s
        e = np.exp(-np.abs(d))
        l = np.log1p(e)
        dd = 1.0 + e
        sig = np.where(d >= 0, 1.0 / dd, e / dd)
        nsig = np.where(d >= 0, e / dd, 1.0 / dd)
        sp = np.where(d > 0, d, 0.0) + l
        sn = np.where(d < 0, -d, 0.0) + l
        yp = y + phi
        L, Psi = gamma_diffs(y, phi)
        ll = -y * sn + (-phi * sp + L)
        u = -yp * sig + y
        ds = phi * (Psi - sp) + (-yp * nsig + phi)
        return ll, u, ds


def check_aux_prior(aux_prior):
    """(loc, scale) of the prior on s; scale finite and > 0.  None: the default (0, 1)"""
    loc, scale = (0.0, 1.0) if aux_prior is None else aux_prior
    loc, scale = float(loc), float(scale)
    if not np.isfinite(loc):
        raise ValueError(f"DomainError: aux_prior location {loc} must be finite")
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError(f"DomainError: aux_prior scale {scale} must be finite and > 0")
    return loc, scale


def dispersion(theta):
    """exp of the last row of draws θ (D, n): σ or φ — the mirror of ahmc_glm_dispersion"""
    th = np.asarray(theta, dtype=np.float64)
    with np.errstate(over="ignore"):
        return np.exp(th[-1])


def aux_logdensity(family, X, y, theta, groups=(), offset=None, prior_prec=None, aux_prior=None, factors=None):
    """(ℓπ (N,), ∇ℓπ (D, N)) at θ (D, N), D = P + G + 1, of a family with a sampled dispersion"""
    return _logdensity(*_hier_args(family, X, theta, groups, prior_prec, aux_prior, True, factors), y, offset)


# ------------------------------------------------------------------------------------------------------------------------------
# include/ahmc_glm_factor.h: index-coded factors instead of one-hot columns of X (csrc/ahmc_glm.hpp: k_glm_eta_f, k_glm_fgrad)
# ------------------------------------------------------------------------------------------------------------------------------
__doc__ += """
Index-coded factors (`factors=` of every function above; check_factors, factor_ranges, expand_factors):
    factor f has L_f levels and a level index idx_f[i] ∈ [0, L_f) per observation; X keeps the P_x >= 1 dense columns; the coefficient
    parameters are P = P_x + Σ L_f rows, the dense ones first, then factor 0's levels, factor 1's, …  Groups, prior_prec and the rows
    after the coefficients (log τ_k, s) address these P rows as they address the columns of X.
    η_i = (X·W[0:P_x])_i + W[off_0 + idx_0[i]] + W[off_1 + idx_1[i]] + … + offset_i        the gathers in this order, offset last
    R_d = −(Xᵀu)_d for d < P_x as above;  R[off_f + l] = −Σ_slices Σ_{i in the slice, idx_f[i] = l} u_i: observations in slices of
    K_SLICE, within a slice ascending i from +0, the slice sums added in ascending order.
This is what the orders of the first header give for the one-hot columns of `expand_factors(X, factors)`: fma(0, w, a) = a and
fma(1, u, a) = a + u for finite operands, so the two encodings give the same numbers (up to the sign of a zero).
"""

GLM_FACTOR_MAX = 8   # AHMC_GLM_FACTOR_MAX


def n_levels(factor):
    """the levels of a factor given as (index, n_levels) or an object with these attributes; n_levels None: max + 1"""
    idx, L = (factor.index, factor.n_levels) if hasattr(factor, "n_levels") else factor
    return int(np.max(idx)) + 1 if L is None else int(L)


def check_factors(factors, n_obs):
    """factors as a list of (index (n_obs,) int64, n_levels): integer indices in [0, n_levels), one per observation, at most GLM_FACTOR_MAX"""
    out = []
    for f, fac in enumerate(factors or ()):
        idx, L = (fac.index, fac.n_levels) if hasattr(fac, "n_levels") else fac
        idx = np.asarray(idx)
        if idx.ndim != 1 or idx.size != n_obs:
            raise ValueError(f"DimensionMismatch: factor {f + 1} has an index of shape {idx.shape}, n_obs = {n_obs}")
        if not np.issubdtype(idx.dtype, np.integer):
            raise ValueError(f"ArgumentError: factor {f + 1}: the level index must have an integer type, not {idx.dtype}")
        L = int(idx.max()) + 1 if L is None else int(L)
        if L < 1:
            raise ValueError(f"DomainError: factor {f + 1} has n_levels = {L}; must be >= 1")
        if idx.min() < 0 or idx.max() >= L:
            bad = int(np.flatnonzero((idx < 0) | (idx >= L))[0])
            raise ValueError(f"DomainError: factor {f + 1}: index[{bad}] = {int(idx[bad])} is outside [0, {L}) (zero-based level indices)")
        out.append((idx.astype(np.int64), L))
    if len(out) > GLM_FACTOR_MAX:
        raise ValueError(f"ArgumentError: {len(out)} factors; at most {GLM_FACTOR_MAX}")
    return out


def factor_ranges(P_x, factors):
    """[(start, stop)] of each factor's coefficient rows: P_x dense rows, then factor 0's levels, factor 1's, …"""
    out, lo = [], int(P_x)
    for fac in factors or ():
        out.append((lo, lo + n_levels(fac)))
        lo = out[-1][1]
    return out


def expand_factors(X, factors):
    """X with every factor written as one-hot columns appended in order: the dense (n_obs, P) equivalent of (X, factors)"""
    X = np.asarray(X, dtype=np.float64)
    return np.column_stack([X] + [np.eye(L)[idx] for idx, L in check_factors(factors, X.shape[0])])


# ------------------------------------------------------------------------------------------------------------------------------
# the one evaluation path: the public functions above check their arguments and end here
# ------------------------------------------------------------------------------------------------------------------------------
def _prior_prec(prior_prec, P, groups):
    p = np.zeros(P) if prior_prec is None else np.asarray(prior_prec, dtype=np.float64).ravel()
    for lo, hi, _, _ in groups:
        if np.any(p[lo:hi] != 0):
            raise ValueError(f"ArgumentError: prior_prec must be 0 on the members of a group ([{lo}, {hi}))")
    return p


def _hier_args(family, X, theta, groups, prior_prec, aux_prior, is_aux=False, factors=None):
    """the checks of θ (P + G, N), or (P + G + 1, N) for a family with a sampled dispersion: `_logdensity`'s first seven arguments"""
    fam = family_code(family)
    is_aux = is_aux or fam in AUX_FAMILIES or aux_prior is not None
    if is_aux and fam not in AUX_FAMILIES:
        raise ValueError(f"ArgumentError: family {fam} has no sampled dispersion (aux_prior belongs to {sorted(f for f in FAMILIES if FAMILIES[f] in AUX_FAMILIES)})")
    aux = check_aux_prior(aux_prior) if is_aux else None
    X = np.asarray(X, dtype=np.float64)
    factors = check_factors(factors, X.shape[0])
    P = X.shape[1] + sum(L for _, L in factors)
    th = np.asarray(theta, dtype=np.float64)
    th = th.reshape(-1, 1) if th.ndim == 1 else th
    if not is_aux:
        th, groups = _hier_theta(th, P, groups)
    else:
        groups = check_groups(groups, P)
        if th.shape[0] != P + len(groups) + 1:
            raise ValueError(f"DimensionMismatch: θ {th.shape}, P + G + 1 = {P} + {len(groups)} + 1")
    return fam, X, th, groups, _prior_prec(prior_prec, P, groups), aux, factors


def _hier_pointwise_args(fam, X, theta, groups, factors=None):
    X = np.asarray(X, dtype=np.float64)
    factors = check_factors(factors, X.shape[0])
    th = np.ascontiguousarray(theta, dtype=np.float64)   # (row-major, as W is below: numpy's product depends on the memory order)
    th = th.reshape(-1, 1) if th.ndim == 1 else th
    _, groups = _hier_theta(th[:-1] if fam in AUX_FAMILIES else th, X.shape[1] + sum(L for _, L in factors), groups)
    return X, th, groups, factors


def _link_at(fam, X, th, groups, factors, y, offset, scale):
    """θ (P + G [+ 1], N) split into the coefficient parameters, the log-scales and s: (W, τ, η, *`link`'s values at η); the plain
    model's W is θ itself, in the caller's memory order.  `factors` checked (maybe none): their rows of W are gathered into η after
    the product over X's columns, factor after factor, and before the offset"""
    Px, G = X.shape[1], len(groups)
    P = Px + sum(L for _, L in factors)
    W, tau = hier_coefficients(th[:P + G], P, groups) if th.shape[0] > P else (th, th[P:])
    if factors:
        eta = X @ W[:Px]
        for (lo, _), (idx, _) in zip(factor_ranges(Px, factors), factors):
            eta = eta + W[lo + idx]
        if offset is not None:
            eta = eta + np.asarray(offset, dtype=np.float64).reshape(-1, 1)
    else:
        eta = linear_predictor(X, W, offset)
    return (W, tau, eta, *link(fam, np.asarray(y, dtype=np.float64).reshape(-1, 1), eta, scale, th[P + G:] if fam in AUX_FAMILIES else None))


def _xtu(X, u, W, factors):
    """Xᵀu (P, N) by slices of K_SLICE observations, the slice sums added in ascending order; the factors' rows by ordered additions"""
    Px = X.shape[1]
    xtu = np.zeros_like(W)
    for k0 in range(0, X.shape[0], K_SLICE):
        part = np.zeros_like(W)
        part[:Px] = X[k0:k0 + K_SLICE].T @ u[k0:k0 + K_SLICE]
        for (lo, _), (idx, _) in zip(factor_ranges(Px, factors), factors):
            np.add.at(part, lo + idx[k0:k0 + K_SLICE], u[k0:k0 + K_SLICE])   # (in order: ascending i within the slice)
        xtu = xtu + part
    return xtu


def _logdensity(fam, X, th, groups, p, aux, factors, y, offset, scale=1.0):
    """(ℓπ, ∇ℓπ) of every model: `groups` and `factors` checked (maybe none), p (P), `aux` = (m, A) of the prior of s or None"""
    Px = X.shape[1]
    PG = Px + sum(L for _, L in factors) + len(groups)
    W, tau, _, ll, u, *ds = _link_at(fam, X, th, groups, factors, y, offset, scale)
    with np.errstate(over="ignore", invalid="ignore"):
        lsum = block_sums(ll).sum(axis=0)
        xtu = _xtu(X, u, W, factors)
        g = np.empty_like(th)
        lp, g[:PG] = _hier_finish(th[:PG], W, tau, -xtu, lsum, p, groups)
        if aux is not None:
            m, A = aux
            dsum = block_sums(ds[0]).sum(axis=0)
            ia2 = 1.0 / (A * A)
            r = th[-1] - m
            lp = lp + ((-0.5 * ia2) * r) * r
            g[-1] = r * ia2 - dsum
    return lp, -g


# ------------------------------------------------------------------------------------------------------------------------------
# include/ahmc_glm_ordinal.h: the ordered-logit family, whose cutpoints are sampled (csrc/ahmc_glm.hpp: k_glm_cut, glm_link_ord,
# k_glm_eta<T, 5, BN>, k_hglm_finish_ord)
# ------------------------------------------------------------------------------------------------------------------------------
__doc__ += """
The ordered-logit family (ordinal_logdensity, ordinal_pointwise, ordinal_link, cutpoints, ordinal_probs):
    y_i ∈ {0, …, C − 1};  c_1 < … < c_{C−1};  P(y <= k) = σ(c_{k+1} − η);  no intercept (a constant column of X is not identified).
    θ (D, N), D = P + G + (C − 1): the P coefficient parameters and the G log-scales as above, then LAST the C − 1 rows κ:
    κ_1 = c_1, κ_j = log(c_j − c_{j−1}) for j >= 2.  Prior on κ itself (no Jacobian term): κ_1 ~ Normal(loc_1, scale_1²),
    κ_j ~ Normal(loc_gap, scale_gap²); cut_prior = (loc_1, scale_1, loc_gap, scale_gap), default (0, 2.5, 0, 1).
    Once per (chain, cutpoint), j ascending:  c_1 = κ_1;  δ_j = exp(κ_j), c_j = c_{j−1} + δ_j;
        lg_j = log(−expm1(−δ_j)) for δ_j <= log 2, log1p(−exp(−δ_j)) above;  r_j = 1/expm1(δ_j);  lg_1 = r_1 = 0.
    Per element, a = c_{y+1} − η (y < C − 1), b = c_y − η (y > 0); e = exp(−|x|), softplus(x) = max(x, 0) + log1p(e), σ(x) = 1/(1 + e)
    for x >= 0 and e/(1 + e) below — softplus(−a) and σ(−a) from one e, softplus(b) and σ(b) from another; a side that does not exist
    contributes exact zeros:
        ℓ = (−softplus(−a) − softplus(b)) + lg_{y+1},   da = σ(−a) + r_{y+1},   db = −σ(b) − r_{y+1},   u = σ(b) − σ(−a)
    with lg and r only for an interior category (0 < y < C − 1).  No difference of two sigmoids is formed:
    σ(a) − σ(b) = σ(a)·σ(−b)·(1 − e^{b−a}) and a − b = δ_{y+1} does not depend on the observation.
    S_k = Σ_{y_i = k−1} da_i + Σ_{y_i = k} db_i (k = 1 … C − 1);  T_{C−1} = S_{C−1}, T_j = S_j + T_{j+1};  ∂ℓ/∂κ_1 = T_1, ∂ℓ/∂κ_j = δ_j·T_j.
    ℓπ = [the hierarchical ℓπ over the first P + G rows, with Σℓ from above] − ½ Σ_j ((κ_j − loc)/scale)².
Order of the new sums (Σℓ, X·W and Xᵀu keep theirs):
  * S_k: per block of ROW_BLOCK observations from +0 in ascending row order — a row with y = k − 1 adds its da, a row with y = k its db,
    any other row nothing — to partial_c[k][row block][chain]; the blocks then lane-strided ascending and the butterfly, as Σ_i ∂ℓ/∂s;
  * the prior, after the groups' terms, j ascending:  r_j = κ_j − loc,  ℓπ = fma((−½·(1/scale²))·r_j, r_j, ℓπ);
  * then j descending:  T_j = S_j + T_{j+1};  g[κ_1] = fma(r_1, 1/scale_1², −T_1);  g[κ_j] = fma(−δ_j, T_j, r_j·(1/scale_gap²)), with
    δ_j = exp(κ_j) once more (the same exp of the same κ_j: the same bits).
A chain's bits depend on (n_obs, P, groups, factors, C, element type) only.  δ_j overflows at κ_j ≈ 710 (89 in Float32): an observation
at or above category j − 1 then has ℓ = −∞ and ℓπ is sanitised to −Inf; κ_j → −∞ closes the gap (lg → −∞, r → ∞) but stays finite
down to κ_j ≈ −700.
"""

ORDERED_LOGIT = 5
ORDINAL_FAMILIES = {"ordered_logit": ORDERED_LOGIT}
ORDINAL_MAX_CATEGORIES = 16   # AHMC_GLM_ORDINAL_MAX_CATEGORIES
CUT_PRIOR = (0.0, 2.5, 0.0, 1.0)
_LOG2 = 0.6931471805599453


def check_cut_prior(cut_prior):
    """(loc_1, scale_1, loc_gap, scale_gap) of the prior on κ; all finite, both scales > 0.  None: the default (0, 2.5, 0, 1)"""
    cp = CUT_PRIOR if cut_prior is None else tuple(float(v) for v in cut_prior)
    if len(cp) != 4:
        raise ValueError(f"ArgumentError: cut_prior = (loc_1, scale_1, loc_gap, scale_gap); got {len(cp)} entries")
    for i, v in enumerate(cp):
        if not np.isfinite(v) or (i % 2 == 1 and not v > 0):
            raise ValueError(f"DomainError: cut_prior[{i + 1}] = {v} must be finite" + (" and > 0 (a scale)" if i % 2 else " (a location)"))
    return cp


def check_categories(y, n_categories):
    """y as int64 categories in [0, C), 2 <= C <= ORDINAL_MAX_CATEGORIES"""
    C = int(n_categories)
    if not 2 <= C <= ORDINAL_MAX_CATEGORIES:
        raise ValueError(f"DomainError: n_categories = {C}; must be in [2, {ORDINAL_MAX_CATEGORIES}]")
    y = np.asarray(y, dtype=np.float64).ravel()
    bad = np.flatnonzero(~((y >= 0) & (y < C) & (y == np.floor(y))))
    if bad.size:
        raise ValueError(f"DomainError: y[{int(bad[0]) + 1}] = {y[bad[0]]} is not a category: an integer in [0, {C})")
    return y.astype(np.int64), C


def cut_constants(kappa):
    """(c, lg, r, δ), each (C − 1, N), from κ (C − 1, N) in κ's floating type: what k_glm_cut writes (δ_1 is set to 1: ∂c_1/∂κ_1)"""
    k = np.asarray(kappa)
    k = k.astype(np.float64) if k.dtype.kind != "f" else k          # (float32: a Float32 context's arithmetic; long double: a reference)
    k = k.reshape(-1, 1) if k.ndim == 1 else k
    one = k.dtype.type(1)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        d = np.exp(k)
        d[0] = one
        c = np.add.accumulate(np.concatenate([k[:1], d[1:]]), axis=0)   # (sequential: c_j = c_{j−1} + δ_j ascending)
        em = np.exp(-d)
        lg = np.where(d <= k.dtype.type(_LOG2), np.log(-np.expm1(-d)), np.log1p(-em))
        r = one / np.expm1(d)
        lg[0] = 0
        r[0] = 0
    return c, lg, r, d


def cutpoints(kappa):
    """c (C − 1, n) of κ (C − 1, n): c_1 = κ_1, c_j = c_{j−1} + exp(κ_j) ascending — the mirror of ahmc_glm_cutpoints on the last C − 1
    rows of draws.  A vector gives a vector."""
    k = np.asarray(kappa)
    c = cut_constants(k)[0]
    return c[:, 0] if k.ndim == 1 else c


def ordinal_link(y, eta, c, lg, r):
    """(ℓ, u = ∂ℓ/∂η, da = ∂ℓ/∂a, db = ∂ℓ/∂b) elementwise in η's floating type: y integer categories (n_obs,), η (n_obs, N), and
    c, lg, r (C − 1, N) from `cut_constants`"""
    eta = np.asarray(eta)
    eta = eta.astype(np.float64) if eta.dtype.kind != "f" else eta
    y = np.asarray(y).astype(np.int64)
    Cm1 = c.shape[0]
    ia, ib = np.minimum(y, Cm1 - 1), np.maximum(y - 1, 0)     # (clamped: the side that does not exist is masked below)
    shape = y.shape + (1,) * (eta.ndim - y.ndim)
    ha, hb = (y < Cm1).reshape(shape), (y > 0).reshape(shape)
    inn = ha & hb
    zero = eta.dtype.type(0)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        a = c[ia] - eta
        e = np.exp(-np.abs(a))
        d = 1 + e
        spa = np.where(ha, np.where(a < 0, -a, zero) + np.log1p(e), zero)
        sna = np.where(ha, np.where(a <= 0, 1 / d, e / d), zero)
        b = c[ib] - eta
        e = np.exp(-np.abs(b))
        d = 1 + e
        spb = np.where(hb, np.where(b > 0, b, zero) + np.log1p(e), zero)
        sb = np.where(hb, np.where(b >= 0, 1 / d, e / d), zero)
        lgv, rv = np.where(inn, lg[ia], zero), np.where(inn, r[ia], zero)
        return (-spa - spb) + lgv, sb - sna, np.where(ha, sna + rv, zero), np.where(hb, -sb - rv, zero)


def ordinal_probs(eta, c):
    """(C, …) category probabilities at η (n_obs, N) [or (n_obs,)] and cutpoints c (C − 1, N) [or (C − 1,)], for posterior-predictive
    use: exp of `ordinal_link`'s ℓ at every category, the gaps' constants from δ_j = c_j − c_{j−1}"""
    eta, c = np.asarray(eta, dtype=np.float64), np.asarray(c, dtype=np.float64)
    vec = eta.ndim == 1
    eta2, c2 = (eta.reshape(-1, 1) if vec else eta), (c.reshape(-1, 1) if c.ndim == 1 else c)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        d = np.diff(c2, axis=0, prepend=c2[:1])
        lg = np.where(d <= _LOG2, np.log(-np.expm1(-d)), np.log1p(-np.exp(-d)))
        lg[0] = 0
        out = np.stack([np.exp(ordinal_link(np.full(eta2.shape[0], k), eta2, c2, lg, np.zeros_like(lg))[0]) for k in range(c2.shape[0] + 1)])
    return out[:, :, 0] if vec else out


def _ordinal_args(X, y, theta, n_categories, groups, factors):
    y, C = check_categories(y, n_categories)
    X = np.asarray(X, dtype=np.float64)
    factors = check_factors(factors, X.shape[0])
    P = X.shape[1] + sum(L for _, L in factors)
    th = np.ascontiguousarray(theta, dtype=np.float64)
    th = th.reshape(-1, 1) if th.ndim == 1 else th
    groups = check_groups(groups, P)
    if y.size != X.shape[0]:
        raise ValueError(f"DimensionMismatch: X {X.shape}, y {y.shape}")
    if th.shape[0] != P + len(groups) + C - 1:
        raise ValueError(f"DimensionMismatch: θ {th.shape}, P + G + (C − 1) = {P} + {len(groups)} + {C - 1}")
    return X, y, th, C, groups, factors, P + len(groups)


def _ordinal_at(X, y, th, PG, groups, factors, offset):
    """(W, τ, η, c, lg, r, δ, *`ordinal_link`'s values): the coefficient rows through `_link_at`'s path with a family that ignores y"""
    W, tau, eta = _link_at(GAUSSIAN_IDENTITY, X, th[:PG], groups, factors, np.zeros(X.shape[0]), offset, 1.0)[:3]
    c, lg, r, d = cut_constants(th[PG:])
    return (W, tau, eta, c, lg, r, d, *ordinal_link(y, eta, c, lg, r))


def ordinal_pointwise(X, y, theta, n_categories, groups=(), offset=None, factors=None):
    """(η, ℓ(y_i, η_i)), each (n_obs, N): the mirror of ahmc_glm_pointwise on an ordinal model"""
    X, y, th, C, groups, factors, PG = _ordinal_args(X, y, theta, n_categories, groups, factors)
    out = _ordinal_at(X, y, th, PG, groups, factors, offset)
    return out[2], out[7]


def ordinal_logdensity(X, y, theta, n_categories, groups=(), offset=None, prior_prec=None, cut_prior=None, factors=None):
    """(ℓπ (N,), ∇ℓπ (D, N)) at θ (D, N), D = P + G + (C − 1), of the ordered-logit model.  ℓπ is returned as computed (`sanitize`)."""
    X, y, th, C, groups, factors, PG = _ordinal_args(X, y, theta, n_categories, groups, factors)
    loc1, sc1, locg, scg = check_cut_prior(cut_prior)
    p = _prior_prec(prior_prec, PG - len(groups), groups)
    W, tau, _, _, _, _, d, ll, u, da, db = _ordinal_at(X, y, th, PG, groups, factors, offset)
    yc = y.reshape(-1, 1)
    with np.errstate(over="ignore", invalid="ignore"):
        g = np.empty_like(th)
        lp, g[:PG] = _hier_finish(th[:PG], W, tau, -_xtu(X, u, W, factors), block_sums(ll).sum(axis=0), p, groups)
        kap = th[PG:]
        S = [block_sums(np.where(yc == k - 1, da, np.where(yc == k, db, 0.0))).sum(axis=0) for k in range(1, C)]
        for j in range(C - 1):
            rj = kap[j] - (loc1 if j == 0 else locg)
            lp = lp + ((-0.5 * (1.0 / (sc1 * sc1) if j == 0 else 1.0 / (scg * scg))) * rj) * rj
        T = np.zeros_like(lp)
        for j in range(C - 2, -1, -1):
            T = S[j] if j == C - 2 else S[j] + T
            g[PG + j] = (kap[j] - loc1) * (1.0 / (sc1 * sc1)) - T if j == 0 else -d[j] * T + (kap[j] - locg) * (1.0 / (scg * scg))
    return lp, -g


# ------------------------------------------------------------------------------------------------------------------------------
# include/ahmc_glm_categorical.h: the categorical-logit family for unordered classes (csrc/ahmc_glm.hpp: glm_link_cat, k_glm_eta_cat)
# ------------------------------------------------------------------------------------------------------------------------------
__doc__ += """
The categorical-logit (softmax) family (categorical_logdensity, categorical_pointwise, categorical_link, categorical_probs):
    y_i ∈ {0, …, C − 1}, unordered; class 0 is the reference, η_0 ≡ 0; K = C − 1 coefficient blocks.  A block has P_b = P_x + Σ L_f rows
    laid out as a non-categorical model's P rows (dense first, then factor 0's levels, …); the coefficient parameters are P = K·P_b
    rows, block k (k = 1 … K, class k) in rows [(k−1)·P_b, k·P_b).  θ (D, N), D = P + G: no rows of the family's own.  Groups and
    prior_prec address the P rows; a group lies inside one block or is a union of whole blocks.
    η_k = X·W_k[0:P_x] + the factors' gathers from block k in order + offset[:, k−1] last      (offset (n_obs, K) or None)
    Per element:  m = 0, then m = η_k if η_k > m for ascending k (a NaN never wins the comparison);
        e_0 = exp(−m), e_k = exp(η_k − m);  s = e_0, then s = s + e_k for ascending k (one term is exactly 1: s ∈ [1, C]);
        inv = 1/s,  lse = m + log(s);  ℓ = η_y − lse with η_0 = 0;  p_0 = e_0·inv, p_k = e_k·inv;  u_k = 1 − p_k if y = k, else −p_k.
    Everything is finite for finite η.  η_k = NaN or +∞ makes s and so ℓ NaN; η_k = −∞ is a class of probability 0 (ℓ = −∞ if it is
    the observed one); ℓπ is sanitised to −Inf either way.
    ℓπ and g: Σℓ by `block_sums`; rows of block k of R = −Xᵀu_k by `_xtu` (slices of K_SLICE, slice sums ascending), class after
    class; the prior's and the groups' terms by `_hier_finish` on the P rows.
There is no multiply-add in the link.  A chain's bits depend on (n_obs, P_x, factors, groups, C, element type) only.
"""

CATEGORICAL_LOGIT = 6
CATEGORICAL_FAMILIES = {"categorical_logit": CATEGORICAL_LOGIT}
CATEGORICAL_MAX_CATEGORIES = 16   # AHMC_GLM_CATEGORICAL_MAX_CATEGORIES


def check_classes(y, n_categories):
    """y as int64 classes in [0, C), 2 <= C <= CATEGORICAL_MAX_CATEGORIES"""
    C = int(n_categories)
    if not 2 <= C <= CATEGORICAL_MAX_CATEGORIES:
        raise ValueError(f"DomainError: n_categories = {C}; must be in [2, {CATEGORICAL_MAX_CATEGORIES}]")
    y = np.asarray(y, dtype=np.float64).ravel()
    bad = np.flatnonzero(~((y >= 0) & (y < C) & (y == np.floor(y))))
    if bad.size:
        raise ValueError(f"DomainError: y[{int(bad[0]) + 1}] = {y[bad[0]]} is not a category: an integer in [0, {C})")
    return y.astype(np.int64), C


def check_class_groups(groups, P_b, K):
    """`check_groups` over the K·P_b rows, and each group inside one class's block or a union of whole blocks"""
    groups = check_groups(groups, K * P_b)
    for k, (lo, hi, _, _) in enumerate(groups):
        if lo // P_b != (hi - 1) // P_b and (lo % P_b or hi % P_b):
            raise ValueError(f"ArgumentError: group {k + 1} = [{lo}, {hi}) straddles the classes' blocks of {P_b} rows: a group lies inside one "
                             "block or is a union of whole blocks")
    return groups


def categorical_link(y, eta):
    """(ℓ (n_obs, N), u (K, n_obs, N), p (C, n_obs, N)) in η's floating type: y integer classes (n_obs,), η (K, n_obs, N) — plane
    k − 1 is η_k"""
    eta = np.asarray(eta)
    eta = eta.astype(np.float64) if eta.dtype.kind != "f" else eta
    y = np.asarray(y).astype(np.int64)
    K = eta.shape[0]
    yc = y.reshape(y.shape + (1,) * (eta.ndim - 1 - y.ndim))
    one = eta.dtype.type(1)
    with np.errstate(over="ignore", invalid="ignore", under="ignore", divide="ignore"):
        m = np.zeros(eta.shape[1:], dtype=eta.dtype)
        for k in range(K):
            m = np.where(eta[k] > m, eta[k], m)
        e0 = np.exp(-m)
        e = [np.exp(eta[k] - m) for k in range(K)]
        s = e0
        for k in range(K):
            s = s + e[k]
        inv = one / s
        lse = m + np.log(s)
        eta_y = np.zeros_like(m)
        for k in range(K):
            eta_y = np.where(yc == k + 1, eta[k], eta_y)
        p = np.stack([e0 * inv] + [e[k] * inv for k in range(K)])
        u = np.stack([np.where(yc == k + 1, one - p[k + 1], -p[k + 1]) for k in range(K)])
    return eta_y - lse, u, p


def categorical_probs(eta):
    """(C, …) class probabilities at η (K, n_obs, N) [or (K, n_obs)]: `categorical_link`'s p — the mirror of ahmc_glm_class_probs"""
    eta = np.asarray(eta, dtype=np.float64)
    return categorical_link(np.zeros(eta.shape[1], dtype=np.int64), eta)[2]


def _categorical_args(X, y, theta, n_categories, groups, factors):
    y, C = check_classes(y, n_categories)
    X = np.asarray(X, dtype=np.float64)
    factors = check_factors(factors, X.shape[0])
    K = C - 1
    Pb = X.shape[1] + sum(L for _, L in factors)
    th = np.ascontiguousarray(theta, dtype=np.float64)
    th = th.reshape(-1, 1) if th.ndim == 1 else th
    groups = check_class_groups(groups, Pb, K)
    if y.size != X.shape[0]:
        raise ValueError(f"DimensionMismatch: X {X.shape}, y {y.shape}")
    if th.shape[0] != K * Pb + len(groups):
        raise ValueError(f"DimensionMismatch: θ {th.shape}, (C − 1)·P_b + G = {K}·{Pb} + {len(groups)}")
    return X, y, th, K, Pb, groups, factors


def _class_offset(offset, n_obs, K):
    if offset is None:
        return None
    off = np.asarray(offset, dtype=np.float64)
    off = off.reshape(n_obs, 1) if off.ndim == 1 and K == 1 else off
    if off.shape != (n_obs, K):
        raise ValueError(f"DimensionMismatch: offset {off.shape}, expected (n_obs, C − 1) = ({n_obs}, {K})")
    return off


def _categorical_at(X, y, th, K, Pb, groups, factors, offset):
    """(W, τ, η (K, n_obs, N), ℓ, u, p): each class's predictor through `_link_at`'s path on its block, with a family that ignores y"""
    off = _class_offset(offset, X.shape[0], K)
    W, tau = hier_coefficients(th, K * Pb, groups)
    W = np.ascontiguousarray(W)
    eta = np.stack([_link_at(GAUSSIAN_IDENTITY, X, W[k * Pb:(k + 1) * Pb], [], factors, np.zeros(X.shape[0]), None if off is None else off[:, k], 1.0)[2]
                    for k in range(K)])
    return (W, tau, eta, *categorical_link(y, eta))


def categorical_pointwise(X, y, theta, n_categories, groups=(), offset=None, factors=None):
    """(η (K, n_obs, N), ℓ(y_i, η_i) (n_obs, N)): the mirror of ahmc_glm_pointwise on a categorical model"""
    X, y, th, K, Pb, groups, factors = _categorical_args(X, y, theta, n_categories, groups, factors)
    out = _categorical_at(X, y, th, K, Pb, groups, factors, offset)
    return out[2], out[3]


def categorical_logdensity(X, y, theta, n_categories, groups=(), offset=None, prior_prec=None, factors=None):
    """(ℓπ (N,), ∇ℓπ (D, N)) at θ (D, N), D = (C − 1)·P_b + G, of the categorical-logit model.  ℓπ is returned as computed (`sanitize`)."""
    X, y, th, K, Pb, groups, factors = _categorical_args(X, y, theta, n_categories, groups, factors)
    p = _prior_prec(prior_prec, K * Pb, groups)
    if p.size != K * Pb:
        raise ValueError(f"DimensionMismatch: the prior has {p.size} entries, the model (C − 1)·P_b = {K * Pb} coefficients")
    W, tau, _, ll, u, _ = _categorical_at(X, y, th, K, Pb, groups, factors, offset)
    with np.errstate(over="ignore", invalid="ignore"):
        xtu = np.concatenate([_xtu(X, u[k], W[k * Pb:(k + 1) * Pb], factors) for k in range(K)])
        lp, g = _hier_finish(th, W, tau, -xtu, block_sums(ll).sum(axis=0), p, groups)
    return lp, -g


# ------------------------------------------------------------------------------------------------------------------------------
# include/ahmc_glm_loo.h: PSIS-LOO and WAIC of the kept draws (csrc/ahmc_glm_loo.hpp: k_loo_keys, k_loo_psis; the sort of csrc/ahmc_diag.hpp)
# ------------------------------------------------------------------------------------------------------------------------------
__doc__ += """
Model comparison from the kept draws (psis_loo, psis_smooth_tail, gpd_fit, gpd_quantile, psis_tail_length, loo_summary, loo_compare):
    Pareto-smoothed importance-sampling leave-one-out (Vehtari, Simpson, Gelman, Yao & Gabry; R loo::psis with r_eff = 1) of a pointwise
    log-likelihood matrix (n_obs, S), one observation (row) at a time, in float64 (or the `dtype` asked for).
    a_s = −ℓ_s with −0 taken as +0.  The draws are sorted by a, ascending and stably (ties keep the draws' order); the sorted position is
    r = 0 … S − 1.  lr_r = a_r − a_{S−1} (the subtraction is monotone, so this order sorts lr too; draws whose a differ but whose lr round
    to the same value keep the order of a).  M = ⌈min(0.2·S, 3·√S)⌉ in float64; the tail is r >= S − M, cut = lr_{S−M−1}.
    The tail is smoothed iff M >= 5 and lr_{S−M} < lr_{S−1} (`psis_smooth_tail`): ec = exp(cut), x_j = exp(tail_j) − ec (j = 1 … M),
    `gpd_fit`: Mg = 30 + ⌊√M⌋, x* = x[⌊M/4 + ½⌋], θ_j = 1/x_M + (1 − √(Mg/(j − ½)))/(3·x*), k_j = W(log1p(−θ_j·x_i))/M,
    l_j = M·(log(−θ_j/k_j) − k_j − 1), w_j = 1/(Σ_i exp(l_i − l_j)) and θ̂ = Σ_j θ_j·w_j, both from +0 in ascending index, one term at a
    time; k = W(log1p(−θ̂·x_i))/M, σ = −k/θ̂, k̂ = (M·k + 5)/(M + 10).  k̂ or σ not finite: nothing is smoothed, k̂ = +Inf.  Otherwise the
    j-th smallest tail value becomes v = log(σ·expm1(−k̂·log1p(−p_j))/k̂ + ec), p_j = (j − ½)/M, and 0 where v > 0.
    With lr now holding the smoothed tail:  lw_r = lr_r − (m + log B(exp(lr_r − m))), m = max lr;  elpd_loo = m₂ + log B(exp(t_r − m₂)),
    t_r = lw_r − a_r, m₂ = max t;  lpd = (ℓ_max + log B(exp(ℓ_r − ℓ_max))) − log S, ℓ_r = −a_r, ℓ_max = −a_0;
    p_waic = B((ℓ_r − mean)²)/(S − 1), mean = B(ℓ_r)/S (NaN at S = 1).  A row with a non-finite ℓ: NaN everywhere.
    The sums.  W (one wave): lane l of 64 adds its elements i = l, l + 64, … from +0 in ascending order; then v_l = v_l + v_{l xor o}
    for o = 32, 16, 8, 4, 2, 1.  B (a workgroup, over the sorted positions): thread t of 256 adds r = t, t + 256, … from +0; the butterfly
    over each of the four waves; then ((w0 + w1) + w2) + w3.  No multiply-add.  An observation's outputs depend on its S values in the
    draws' order alone.
"""

LOO_MAX_TAIL = 4096   # AHMC_GLM_LOO_MAX_TAIL


def _wave_sum(v):
    """W over the last axis"""
    v = np.asarray(v)
    n = v.shape[-1]
    rows = max(1, -(-n // 64))
    p = np.zeros(v.shape[:-1] + (rows * 64,), dtype=v.dtype)
    p[..., :n] = v
    p = p.reshape(v.shape[:-1] + (rows, 64))
    acc = np.zeros(v.shape[:-1] + (64,), dtype=v.dtype)
    for r in range(rows):
        acc = acc + p[..., r, :]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lanes ^ o]
    return acc[..., 0]


def _block_sum(v):
    """B over the last axis"""
    v = np.asarray(v)
    n = v.shape[-1]
    rows = max(1, -(-n // 256))
    p = np.zeros(v.shape[:-1] + (rows * 256,), dtype=v.dtype)
    p[..., :n] = v
    p = p.reshape(v.shape[:-1] + (rows, 256))
    acc = np.zeros(v.shape[:-1] + (256,), dtype=v.dtype)
    for r in range(rows):
        acc = acc + p[..., r, :]
    acc = acc.reshape(v.shape[:-1] + (4, 64))
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lanes ^ o]
    w = acc[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def psis_tail_length(S):
    """M = ⌈min(0.2·S, 3·√S)⌉"""
    return int(np.ceil(min(0.2 * float(S), 3.0 * np.sqrt(float(S)))))


def gpd_quantile(p, k, sigma):
    """the quantile function of the generalised Pareto distribution with location 0: σ·expm1(−k·log1p(−p))/k"""
    return sigma * np.expm1(-k * np.log1p(-p)) / k


def gpd_fit(x):
    """(k̂, σ) of Zhang & Stephens' fit to x (M,), ascending and >= 0, k̂ shrunk towards ½ with weight 10: (M·k + 5)/(M + 10)"""
    x = np.asarray(x)
    x = x.astype(np.float64) if x.dtype.kind != "f" else x
    ft = x.dtype.type
    M = x.size
    Md = ft(M)
    Mg = 30 + int(np.floor(np.sqrt(float(M))))
    with np.errstate(all="ignore"):
        xs, xM = x[int(np.floor(M / 4.0 + 0.5)) - 1], x[-1]
        j = np.arange(1, Mg + 1).astype(x.dtype)
        th = ft(1) / xM + (ft(1) - np.sqrt(ft(Mg) / (j - ft(0.5)))) / (ft(3) * xs)
        kj = _wave_sum(np.log1p(-th[:, None] * x[None, :])) / Md
        l = Md * (np.log(-th / kj) - kj - ft(1))
        E = np.exp(l[None, :] - l[:, None])            # (j, i)
        s = np.zeros(Mg, dtype=x.dtype)
        for i in range(Mg):
            s = s + E[:, i]
        w = ft(1) / s
        that = ft(0)
        for q in range(Mg):
            that = that + th[q] * w[q]
        k = _wave_sum(np.log1p(-that * x)) / Md
        return (Md * k + ft(5)) / (Md + ft(10)), -k / that


def psis_smooth_tail(tail, cut):
    """(the smoothed tail, k̂) of the M largest lr, ascending, and the value just below them; (the tail as it was, +Inf) if it is not
    smoothed"""
    tail = np.asarray(tail)
    ft = tail.dtype.type
    M = tail.size
    if M < 5 or not tail[0] < tail[-1]:
        return tail, ft(np.inf)
    with np.errstate(all="ignore"):
        ec = np.exp(cut)
        khat, sigma = gpd_fit(np.exp(tail) - ec)
        if not (np.isfinite(khat) and np.isfinite(sigma)):
            return tail, ft(np.inf)
        p = (np.arange(1, M + 1).astype(tail.dtype) - ft(0.5)) / ft(M)
        v = np.log(gpd_quantile(p, khat, sigma) + ec)
        return np.where(v > 0, ft(0), v), khat


def psis_loo(loglik, dtype=np.float64, log_weights=True):
    """{"elpd_loo", "pareto_k", "lpd", "p_waic"} (n_obs,) each, and "log_weights" (S, n_obs) in the draws' order (on request), of the
    pointwise log-likelihood `loglik` (n_obs, S) — the mirror of ahmc_glm_loo"""
    ll = np.asarray(loglik)
    if ll.ndim != 2 or ll.shape[1] < 1:
        raise ValueError(f"DimensionMismatch: loglik {ll.shape}, expected (n_obs, S) with S >= 1")
    dt = np.dtype(dtype)
    ft = dt.type
    n_obs, S = ll.shape
    M = psis_tail_length(S)
    if M > LOO_MAX_TAIL:
        raise ValueError(f"ArgumentError: S = {S} draws have a tail of {M} values; the limit is {LOO_MAX_TAIL}")
    out = {k: np.full(n_obs, np.nan, dtype=dt) for k in ("elpd_loo", "pareto_k", "lpd", "p_waic")}
    lw_all = np.full((S, n_obs), np.nan, dtype=dt) if log_weights else None
    Sd = ft(S)
    with np.errstate(all="ignore"):
        for i in range(n_obs):
            a = -ll[i].astype(dt)
            if not np.isfinite(a).all():
                continue
            a = np.where(a == 0, ft(0), a)
            order = np.argsort(a, kind="stable")
            a = a[order]
            lr = a - a[-1]
            khat = ft(np.inf)
            if M >= 5:
                tail, khat = psis_smooth_tail(lr[S - M:], lr[S - M - 1])
                lr = np.concatenate([lr[:S - M], tail])
            l = -a
            l_max = l[0]
            s_lpd = _block_sum(np.exp(l - l_max))
            mean = _block_sum(l) / Sd
            m1 = lr.max()
            s_v = _block_sum((l - mean) * (l - mean))
            lse = m1 + np.log(_block_sum(np.exp(lr - m1)))
            lw = lr - lse
            t = lw - a
            m2 = t.max()
            out["elpd_loo"][i] = m2 + np.log(_block_sum(np.exp(t - m2)))
            out["pareto_k"][i] = khat
            out["lpd"][i] = (l_max + np.log(s_lpd)) - np.log(Sd)
            out["p_waic"][i] = s_v / (Sd - ft(1))
            if log_weights:
                lw_all[order, i] = lw
    if log_weights:
        out["log_weights"] = lw_all
    return out


def loo_summary(pw):
    """totals of `psis_loo`'s (or Engine.glm_loo's) pointwise numbers: Σ elpd_loo, Σ p_loo (p_loo = lpd − elpd_loo), Σ elpd_waic
    (elpd_waic = lpd − p_waic), each with se = √(n·var) of its pointwise values (var with n − 1), and the counts of k̂ in (0.5, 0.7],
    (0.7, 1] and (1, ∞]"""
    elpd, lpd, pwaic, k = (np.asarray(pw[n], dtype=np.float64) for n in ("elpd_loo", "lpd", "p_waic", "pareto_k"))
    n = elpd.size
    out = {"n_obs": n}
    with np.errstate(all="ignore"):
        for name, v in (("elpd_loo", elpd), ("p_loo", lpd - elpd), ("elpd_waic", lpd - pwaic)):
            out[name] = float(v.sum())
            out["se_" + name] = float(np.sqrt(n * v.var(ddof=1))) if n > 1 else float("nan")
    out["k_counts"] = {"(0.5, 0.7]": int(((k > 0.5) & (k <= 0.7)).sum()), "(0.7, 1]": int(((k > 0.7) & (k <= 1)).sum()), "(1, Inf]": int((k > 1).sum())}
    return out


def loo_compare(pw_a, pw_b):
    """{"elpd_diff": Σ (elpd_loo_a − elpd_loo_b), "se_diff": √(n·var) of the pointwise differences}: positive favours model a"""
    a, b = np.asarray(pw_a["elpd_loo"], dtype=np.float64), np.asarray(pw_b["elpd_loo"], dtype=np.float64)
    if a.shape != b.shape or a.ndim != 1:
        raise ValueError(f"DimensionMismatch: elpd_loo {a.shape} and {b.shape}: the two models must be fitted to the same observations")
    d = a - b
    with np.errstate(all="ignore"):
        return {"elpd_diff": float(d.sum()), "se_diff": float(np.sqrt(d.size * d.var(ddof=1))) if d.size > 1 else float("nan")}


# ------------------------------------------------------------------------------------------------------------------------------
# include/ahmc_glm_predict.h: predictions at new data, their summaries over the draws and the held-out lpd (csrc/ahmc_glm_predict.hpp)
# ------------------------------------------------------------------------------------------------------------------------------
__doc__ += """
Predictions at new rows of data (predict, predict_summary): the model's full path at X_new — the effective coefficients W, the
factors' levels gathered after the product, the offset last — and from η, per observation and draw, the Q quantities
    families 0 – 4:  η, μ = E[y|θ], v = Var[y|θ]     Bernoulli σ(η), μ(1 − μ);  Poisson exp(η), μ;  Gaussian η, 1/scale;
                                                       Gaussian with σ sampled η, exp(2s);  negative binomial exp(η), μ + μ²·exp(−s)
    ordered logit:   η, p_0 … p_{C−1} (`ordinal_probs`)          categorical logit:  η_1 … η_K, p_0 … p_{C−1} (`categorical_probs`)
and ℓ(y_new, η) where outcomes are given.  Summary over the S draws, per observation: mean and variance (divisor S − 1) of every
quantity and lpd = logsumexp_s ℓ − log S.  Order of the sums: the draws in blocks of PRED_BLOCK = 64 — block b holds draws 64b … 64b + 63
whatever the chunking; inside a block, ascending from +0: n_b, mean_b = (Σx)/n_b, M2_b = Σ(x − mean_b)², and for ℓ m_b = max,
s_b = Σ exp(ℓ − m_b); the blocks in ascending order:  δ = mean_b − mean, n′ = n + n_b, mean = mean + δ·(n_b/n′),
M2 = M2 + (M2_b + (((δ·δ)·n)·n_b)/n′)  and  m′ = max(m, m_b), s = s·exp(m − m′) + s_b·exp(m_b − m′)  from (−Inf, 0) — every
operation rounded on its own.  A block with a non-finite value is (NaN, NaN), which the updates carry to the end.
"""

PRED_BLOCK = 64   # GLM_PRED_BLOCK of csrc/ahmc_glm_predict_spec.hpp: the draws of one block of the summary's sums
PRED_WHAT = ("linear", "mean", "variance", "loglik")


def predict(family, X_new, theta, what="mean", factors=None, offset=None, y=None, groups=(), n_categories=None, scale=1.0):
    """The mirror of ahmc_glm_predict at new rows X_new (n_new, P_x) and draws θ (D, n), D as the bound model has it (coefficient rows,
    log-scales of the groups, then s or κ).  `what`: "linear" η (n_new, n) — (K, n_new, n) of a categorical model; "mean" μ (n_new, n),
    or the probabilities (C, n_new, n) of an ordinal or a categorical model; "variance" v (n_new, n), families 0 – 4 only; "loglik"
    ℓ(y, η) (n_new, n), which needs `y`.  `factors`: the new rows' level indices with the bound model's level counts."""
    if what not in PRED_WHAT:
        raise ValueError(f"ArgumentError: what = {what!r}; one of {PRED_WHAT}")
    if what == "loglik" and y is None:
        raise ValueError("ArgumentError: what = 'loglik' needs y, the outcomes to evaluate")
    ordinal = family in ORDINAL_FAMILIES or family == ORDERED_LOGIT
    categorical = family in CATEGORICAL_FAMILIES or family == CATEGORICAL_LOGIT
    n_new = np.asarray(X_new).shape[0]
    y0 = np.zeros(n_new) if y is None else y
    if ordinal or categorical:
        if what == "variance":
            raise ValueError("ArgumentError: what = 'variance' of a model whose outcome is a category; 'mean' gives the probabilities")
        if n_categories is None:
            raise ValueError("ArgumentError: the family needs n_categories")
    if ordinal:
        X, yi, th, C, grp, fac, PG = _ordinal_args(X_new, y0, theta, n_categories, groups, factors)
        out = _ordinal_at(X, yi, th, PG, grp, fac, offset)
        return {"linear": out[2], "loglik": out[7]}[what] if what != "mean" else ordinal_probs(out[2], out[3])
    if categorical:
        X, yi, th, K, Pb, grp, fac = _categorical_args(X_new, y0, theta, n_categories, groups, factors)
        out = _categorical_at(X, yi, th, K, Pb, grp, fac, offset)
        return {"linear": out[2], "mean": out[5], "loglik": out[3]}[what]
    fam = family_code(family)
    X, th, grp, fac = _hier_pointwise_args(fam, X_new, theta, groups, factors)
    eta, ll = _link_at(fam, X, th, grp, fac, y0, offset, scale)[2:4]
    if what in ("linear", "loglik"):
        return eta if what == "linear" else ll
    s = th[-1:] if fam in AUX_FAMILIES else None
    with np.errstate(over="ignore", invalid="ignore"):
        if fam == BERNOULLI_LOGIT:
            e = np.exp(-np.abs(eta))
            d = 1.0 + e
            mu = np.where(eta >= 0, 1.0 / d, e / d)
            v = mu * (1.0 - mu)
        elif fam == POISSON_LOG:
            mu = np.exp(eta)
            v = mu
        elif fam == GAUSSIAN_IDENTITY:
            mu, v = eta, np.full_like(eta, 1.0 / scale)
        elif fam == GAUSSIAN_IDENTITY_SIGMA:
            mu, v = eta, np.broadcast_to(np.exp(2.0 * s), eta.shape).copy()
        else:
            mu = np.exp(eta)
            v = (mu * mu) * np.exp(-s) + mu
    return mu if what == "mean" else v


def _pred_blocks(x, lse):
    """the block partials of x (…, nc), nc draws that begin at a block's first: (…, nblk, 2) — (mean_b, M2_b), or (m_b, s_b) with `lse`"""
    nc = x.shape[-1]
    out = np.empty(x.shape[:-1] + ((nc + PRED_BLOCK - 1) // PRED_BLOCK, 2))
    zero = np.zeros(x.shape[:-1] + (1,))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for b in range(out.shape[-2]):
            xb = x[..., b * PRED_BLOCK:(b + 1) * PRED_BLOCK].astype(np.float64)
            bad = ~np.isfinite(xb).all(axis=-1)
            if lse:
                m = np.maximum.accumulate(xb, axis=-1)[..., -1]
                first, second = m, np.add.accumulate(np.concatenate([zero, np.exp(xb - m[..., None])], axis=-1), axis=-1)[..., -1]
            else:
                first = np.add.accumulate(np.concatenate([zero, xb], axis=-1), axis=-1)[..., -1] / float(xb.shape[-1])
                d = xb - first[..., None]
                second = np.add.accumulate(np.concatenate([zero, d * d], axis=-1), axis=-1)[..., -1]
            out[..., b, 0] = np.where(bad, np.nan, first)
            out[..., b, 1] = np.where(bad, np.nan, second)
    return out


def _pred_fold(state, part, b0, S, lse):
    """the running state (…, 2) after the block partials `part` (…, nblk, 2) of blocks b0, b0 + 1, … of S draws"""
    a, c = state[..., 0].copy(), state[..., 1].copy()
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for b in range(part.shape[-2]):
            pa, pc = part[..., b, 0], part[..., b, 1]
            if lse:
                mn = np.where(pa > a, pa, a)
                c = c * np.exp(a - mn) + pc * np.exp(pa - mn)
                a = mn
            else:
                n = float(PRED_BLOCK * (b0 + b))
                nb = float(min(PRED_BLOCK, S - PRED_BLOCK * (b0 + b)))
                npr = n + nb
                d = pa - a
                a = a + d * (nb / npr)
                c = c + (pc + (((d * d) * n) * nb) / npr)
    return np.stack([a, c], axis=-1)


def predict_summary(values, loglik=None, chunk=None):
    """(2Q + 1, n_new) float64 from values (Q, n_new, S) — the quantities of every observation at S draws, in the header's order — and
    ℓ (n_new, S) or None: rows 2q, 2q + 1 the mean and the variance (divisor S − 1; NaN at S = 1) of quantity q, the last row
    lpd = logsumexp_s ℓ − log S (NaN without ℓ).  The mirror of ahmc_glm_predict_summary: this function DEFINES the order of its sums
    (the module docstring).  `chunk`: the draws are taken in pieces of this many (a multiple of PRED_BLOCK), as the device takes them; the
    result does not depend on it."""
    v = np.asarray(values)
    if v.ndim != 3:
        raise ValueError(f"DimensionMismatch: values {v.shape}, expected (Q, n_new, S)")
    Q, n_new, S = v.shape
    ll = None if loglik is None else np.asarray(loglik)
    if ll is not None and ll.shape != (n_new, S):
        raise ValueError(f"DimensionMismatch: loglik {ll.shape}, expected {(n_new, S)}")
    chunk = (S + PRED_BLOCK - 1) // PRED_BLOCK * PRED_BLOCK if chunk is None else int(chunk)
    if chunk < PRED_BLOCK or chunk % PRED_BLOCK:
        raise ValueError(f"ArgumentError: chunk = {chunk} is no multiple of {PRED_BLOCK}")
    out = np.full((2 * Q + 1, n_new), np.nan)
    if S == 0:
        return out
    st = np.zeros((Q, n_new, 2))
    sl = np.stack([np.full(n_new, -np.inf), np.zeros(n_new)], axis=-1)
    for j0 in range(0, S, chunk):
        st = _pred_fold(st, _pred_blocks(v[..., j0:j0 + chunk], False), j0 // PRED_BLOCK, S, False)
        if ll is not None:
            sl = _pred_fold(sl, _pred_blocks(ll[..., j0:j0 + chunk], True), j0 // PRED_BLOCK, S, True)
    out[0:2 * Q:2] = st[..., 0]
    if S > 1:
        out[1:2 * Q:2] = st[..., 1] / float(S - 1)
    if ll is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            out[2 * Q] = (sl[:, 0] + np.log(sl[:, 1])) - np.log(float(S))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# include/ahmc_glm_yrep.h: posterior-predictive draws y_rep ~ p(y | θ_s) and their per-observation summaries
# ---------------------------------------------------------------------------------------------------------------------
"""
yrep_at is the CONTRACT of the device sampler (csrc/ahmc_glm_yrep_draw.hpp).  Arithmetic is float64 whatever the element type: planes are
converted on entry, y on exit.  Randomness: Philox4x32-10 under key = seed (lo, hi) at counter (row, col, YREP_PURPOSE, slot); slot
counts the 4-word blocks the element has taken, from 0; a block gives u = u53(v0, v1), u′ = u53(v2, v3) in (0, 1] and, where a normal is
asked for, z = sqrt(−2·log u)·cos(2π·u′).  So an element's y depends on its quantities, its (row, col) and the seed alone.
    0 Bernoulli (μ):            y = [u <= μ]
    2, 3 Gaussian (μ, v):       y = fma(√v, z, μ)          (numpy has no fma: the mirror rounds the product, at most 1 u apart)
    5, 6 (p_0 … p_{C−1}):       F ascending from +0, each add rounded on its own; y = #{c <= C − 2 : u > F_c}
    1 Poisson (λ = μ) λ < 10:   one u;  p = exp(−λ), F = p, k = 0;  while u > F and k < 200: k += 1, p = (p·λ)/k, F = F + p
                      λ >= 10:  Hörmann's PTRS, one block (u, u′) a round:  b = 0.931 + 2.53√λ, a = −0.059 + 0.02483·b,
                                1/α = 1.1239 + 1.1328/(b − 3.4), v_r = 0.9277 − 3.6224/(b − 2);  U = u − ½, V = u′, us = ½ − |U|,
                                k = floor((((2a)/us + b)·U + λ) + 0.43);  accept if us >= 0.07 and V <= v_r;  reject if k < 0 or
                                (us < 0.013 and V > us);  else accept iff
                                (log V + log(1/α)) − log(a/(us·us) + b) <= (−λ + k·log λ) − lgamma(k + 1)
    4 negative binomial (μ, s): φ = exp(s);  g ~ Gamma(φ, 1) by Marsaglia–Tsang: φ < 1 takes a block FIRST for the boost u^(1/φ) and
                                uses shape φ + 1;  d = shape − 1/3, c = 1/sqrt(9d);  a round takes a normal block, then a uniform
                                block: w = 1 + c·z, t = (w·w)·w, reject if t <= 0, accept iff
                                log u < ((((½·z)·z) + d) − d·t) + d·log t, then g = d·t;  y ~ Poisson(((g·boost)·μ)/φ), slots running on
Every rejection loop stops after YREP_MAX_ROUNDS = 64 rounds with NaN (P < 1e-40).  A non-finite (or negative) quantity, or a dispersion
that makes λ non-finite, gives NaN; λ = 0 gives 0.  The margin of an element is the smallest, over the decisions it took, of
|lhs − rhs|/max(|lhs|, |rhs|, 1) of a comparison and of (distance to the nearest integer)/max(|x|, 1) of the floor.
"""

YREP_PURPOSE = 0x59524550
YREP_MAX_ROUNDS = 64
YREP_INVERSION_MAX = 200
YREP_INVERSION_BELOW = 10.0
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of csrc/ahmc_device.hpp on arrays of counters (uint64 holding 32-bit words): the four output words"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & _M32, np.uint64(k1) & _M32
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        n0, n2 = (p1 >> s32) ^ c1 ^ k0, (p0 >> s32) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & _M32, n2, p0 & _M32
        k0, k1 = (k0 + W0) & _M32, (k1 + W1) & _M32
    return c0, c1, c2, c3


def u53(hi, lo):
    """the 53-bit uniform in (0, 1] of csrc/ahmc_device.hpp"""
    b = ((hi >> np.uint64(5)) << np.uint64(26)) | (lo >> np.uint64(6))
    return (b.astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


class _YrepState:
    """the elements of one yrep_at call: their counters, the blocks taken, the outcome and the margin"""

    def __init__(self, row, col, seed, n, ones):
        self.row, self.col = row.astype(np.uint64), col.astype(np.uint64)
        self.k0, self.k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
        self.slot = np.zeros(n, dtype=np.uint64)
        self.y = np.full(n, np.nan)
        self.margin = np.full(n, np.inf)
        self.ones = ones

    def block(self, idx):
        """(u, u′) of the next block of the elements idx"""
        if self.ones:                                     # the driver's test hook: every uniform is 1
            u = up = np.ones(len(idx))
        else:
            v = philox4x32_10(self.row[idx], self.col[idx], np.full(len(idx), YREP_PURPOSE, dtype=np.uint64), self.slot[idx], self.k0, self.k1)
            u, up = u53(v[0], v[1]), u53(v[2], v[3])
        self.slot[idx] += np.uint64(1)
        return u, up

    def cmp(self, idx, lhs, rhs, threshold=False):
        """`threshold`: a branch threshold of the sampler (λ against 10, φ against 1); a quantity that EQUALS it — λ = 10 given as a
        plane, s = 0 — is decided alike everywhere and is not counted"""
        lhs, rhs = np.broadcast_to(np.asarray(lhs, dtype=np.float64), idx.shape), np.broadcast_to(np.asarray(rhs, dtype=np.float64), idx.shape)
        with np.errstate(invalid="ignore"):
            m = np.abs(lhs - rhs) / np.maximum(np.maximum(np.abs(lhs), np.abs(rhs)), 1.0)
        if threshold:
            m = np.where(lhs == rhs, np.inf, m)
        self.margin[idx] = np.fmin(self.margin[idx], m)

    def floor(self, idx, x):
        with np.errstate(invalid="ignore"):
            m = np.abs(x - np.rint(x)) / np.maximum(np.abs(x), 1.0)
        self.margin[idx] = np.fmin(self.margin[idx], m)


def _yrep_normal(u, up):
    return np.sqrt(-2.0 * np.log(u)) * np.cos(6.283185307179586476925286766559 * up)


def _lgamma1(x):
    try:
        return math.lgamma(x)
    except OverflowError:
        return math.inf


_lgamma = np.frompyfunc(_lgamma1, 1, 1)


def _yrep_poisson(st, idx, lam, plant):
    """y ~ Poisson(λ) for the elements idx (λ aligned with idx), written to st.y"""
    with np.errstate(all="ignore"):
        ok = np.isfinite(lam) & (lam >= 0.0)
        idx, lam = idx[ok], lam[ok]
        st.cmp(idx, lam, YREP_INVERSION_BELOW, threshold=True)
        small = lam < YREP_INVERSION_BELOW
        # ---- inversion
        i, l = idx[small], lam[small]
        if len(i):
            u, _ = st.block(i)
            p = np.exp(-l)
            F = p.copy()
            k = np.zeros(len(i))
            if plant == "inversion-from-1":
                k += 1.0
            live = np.arange(len(i))
            for _ in range(YREP_INVERSION_MAX):
                st.cmp(i[live], u[live], F[live])
                stop = (u[live] < F[live]) if plant == "strict" else (u[live] <= F[live])
                live = live[~stop]
                if not len(live):
                    break
                k[live] += 1.0
                p[live] = p[live] * l[live] / k[live]
                F[live] = F[live] + p[live]
            k = np.minimum(k, float(YREP_INVERSION_MAX))
            st.y[i] = k
        # ---- PTRS
        i, l = idx[~small], lam[~small]
        if not len(i):
            return
        b = 0.931 + 2.53 * np.sqrt(l)
        a = -0.059 + 0.02483 * b
        inv_alpha = 1.1239 + 1.1328 / (b - 3.4)
        vr = 0.9277 - 3.6224 / (b - 2.0)
        log_l = np.log(l)
        shift = 0.0 if plant == "ptrs-no-shift" else 0.43
        live = np.arange(len(i))
        for _ in range(YREP_MAX_ROUNDS):
            if not len(live):
                break
            j = i[live]
            u, V = st.block(j)
            U = u - 0.5
            us = 0.5 - np.abs(U)
            x = (2.0 * a[live] / us + b[live]) * U + l[live] + shift
            k = np.floor(x)
            st.floor(j, x)
            st.cmp(j, us, 0.07)
            big = us >= 0.07
            st.cmp(j[big], V[big], vr[live][big])
            acc = big & (V <= vr[live])
            rest = ~acc
            tiny = rest & (us < 0.013)
            st.cmp(j[rest], us[rest], 0.013)
            st.cmp(j[tiny], V[tiny], us[tiny])
            rej = rest & ((k < 0.0) | (tiny & (V > us)))
            test = rest & ~rej
            if test.any():
                lv = live[test]
                lhs = np.log(V[test]) + np.log(inv_alpha[lv]) - np.log(a[lv] / (us[test] * us[test]) + b[lv])
                rhs = -l[lv] + k[test] * log_l[lv] - _lgamma(k[test] + 1.0).astype(np.float64)
                st.cmp(j[test], lhs, rhs)
                acc[np.flatnonzero(test)[lhs <= rhs]] = True
            st.y[j[acc]] = k[acc]
            live = live[~acc]


def _yrep_negbinomial(st, idx, mu, s, plant):
    with np.errstate(all="ignore"):
        phi = np.exp(s)
        ok = np.isfinite(mu) & np.isfinite(phi) & (phi > 0.0) & (mu >= 0.0)
        idx, mu, phi = idx[ok], mu[ok], phi[ok]
        n = len(idx)
        st.cmp(idx, phi, 1.0, threshold=True)
        low = phi < 1.0
        boost = np.ones(n)
        if low.any():
            u, _ = st.block(idx[low])
            if plant != "gamma-no-boost":
                boost[low] = np.power(u, 1.0 / phi[low])
        shape = np.where(low, phi + 1.0, phi)
        d = shape - 1.0 / 3.0
        c = 1.0 / np.sqrt(9.0 * d)
        g = np.full(n, np.nan)
        live = np.arange(n)
        for _ in range(YREP_MAX_ROUNDS):
            if not len(live):
                break
            j = idx[live]
            z = _yrep_normal(*st.block(j))
            u, _ = st.block(j)
            w = 1.0 + c[live] * z
            t = w * w * w
            st.cmp(j, t, 0.0)
            pos = t > 0.0
            dl, tl, zl = d[live][pos], t[pos], z[pos]
            lhs = np.log(u[pos])
            rhs = 0.5 * zl * zl + dl - dl * tl + dl * np.log(tl)
            st.cmp(j[pos], lhs, rhs)
            acc = np.zeros(len(live), dtype=bool)
            acc[np.flatnonzero(pos)[lhs < rhs]] = True
            g[live[acc]] = (d[live] * t)[acc]
            live = live[~acc]
        done = g == g
        _yrep_poisson(st, idx[done], g[done] * boost[done] * mu[done] / phi[done], plant)


def _yrep_family(family):
    if family in ORDINAL_FAMILIES or family in CATEGORICAL_FAMILIES:
        return {**ORDINAL_FAMILIES, **CATEGORICAL_FAMILIES}[family]
    if not isinstance(family, str) and int(family) in (ORDERED_LOGIT, CATEGORICAL_LOGIT):
        return int(family)
    return family_code(family)


def yrep_at(family, q, aux=None, row=None, col=None, seed=0, n_categories=None, _plant=None, _ones=False):
    """(y, margin), each (n,) float64: one outcome per element from the family's sampler given the element's planes q (planes, n) —
    μ; (μ, v) of a Gaussian; the C probabilities of an ordinal or a categorical model — `aux` (n,), the log-dispersion of a negative
    binomial, and the element's counter (row, col) (default 0 … n − 1 and 0) under `seed`.  The mirror of ahmc_glm_yrep_at: this
    function DEFINES the sampler (the section's docstring).  `_plant` plants one of the defects the tests must catch; `_ones` makes every
    uniform 1, as the C++ driver's hook does."""
    fam = _yrep_family(family)
    q = np.asarray(q, dtype=np.float64)
    if q.ndim == 1:
        q = q[None]
    classes = fam in (ORDERED_LOGIT, CATEGORICAL_LOGIT)
    if classes and (n_categories is None or not 2 <= int(n_categories) <= CATEGORICAL_MAX_CATEGORIES):
        raise ValueError(f"ArgumentError: n_categories = {n_categories} is outside 2 … {CATEGORICAL_MAX_CATEGORIES}")
    planes = int(n_categories) if classes else 2 if fam in (GAUSSIAN_IDENTITY, GAUSSIAN_IDENTITY_SIGMA) else 1
    if q.ndim != 2 or q.shape[0] != planes:
        raise ValueError(f"DimensionMismatch: q {q.shape}, expected ({planes}, n)")
    n = q.shape[1]
    if fam == NEGBINOMIAL_LOG:
        if aux is None:
            raise ValueError("ArgumentError: the negative binomial needs aux, the log-dispersion of every element")
        aux = np.broadcast_to(np.asarray(aux, dtype=np.float64), (n,))
    row = np.arange(n, dtype=np.uint64) if row is None else np.broadcast_to(np.asarray(row), (n,))
    col = np.zeros(n, dtype=np.uint64) if col is None else np.broadcast_to(np.asarray(col), (n,))
    st = _YrepState(row, col, seed, n, _ones)
    idx = np.arange(n)
    with np.errstate(all="ignore"):
        if fam == BERNOULLI_LOGIT:
            u, _ = st.block(idx)
            fin = np.isfinite(q[0])
            st.cmp(idx, u, q[0])
            st.y[fin] = ((u < q[0]) if _plant == "strict" else (u <= q[0]))[fin].astype(np.float64)
        elif not classes and planes == 2:
            z = _yrep_normal(*st.block(idx))
            fin = np.isfinite(q[0]) & np.isfinite(q[1])
            st.y[fin] = (np.sqrt(q[1]) * z + q[0])[fin]
        elif classes:
            u, _ = st.block(idx)
            F = np.zeros(n)
            y = np.zeros(n)
            for c in range(planes - 1):
                F = F + q[c]
                st.cmp(idx, u, F)
                y += ~(u < F) if _plant == "strict" else (u > F)
            fin = np.isfinite(q).all(axis=0)
            st.y[fin] = y[fin]
        elif fam == POISSON_LOG:
            _yrep_poisson(st, idx, q[0], _plant)
        else:
            _yrep_negbinomial(st, idx, q[0], aux, _plant)
    return st.y, st.margin


def yrep(family, planes, aux=None, seed=0, n_categories=None):
    """(y_rep, margin), each (n_new, S): yrep_at for the planes (planes, n_new, S) of every new observation and draw — what
    ahmc_glm_predict gives for "mean" (and "variance" after it, for a Gaussian) — with `aux` (S,) the draws' log-dispersion; element
    (i, j) has the counter (row, col) = (i, j).  The mirror of ahmc_glm_yrep."""
    p = np.asarray(planes, dtype=np.float64)
    if p.ndim == 2:
        p = p[None]
    _, n_new, S = p.shape
    row, col = np.broadcast_to(np.arange(n_new)[:, None], (n_new, S)).ravel(), np.broadcast_to(np.arange(S)[None, :], (n_new, S)).ravel()
    a = None if aux is None else np.broadcast_to(np.asarray(aux, dtype=np.float64)[None, :], (n_new, S)).ravel()
    y, m = yrep_at(family, p.reshape(p.shape[0], -1), a, row, col, seed, n_categories)
    return y.reshape(n_new, S), m.reshape(n_new, S)


def yrep_summary(y_rep, y=None, chunk=None):
    """(4, n_new) float64 from y_rep (n_new, S): the mean and the variance (divisor S − 1; NaN at S = 1) of every observation's draws in
    the order of predict_summary's sums (blocks of PRED_BLOCK draws, ascending, whatever the chunk), and with the outcomes y (n_new)
    p_less = #(y_rep < y)/S and p_equal = #(y_rep == y)/S, the counts exact integers (NaN rows without y).  An observation with a
    NaN draw has NaN moments; a NaN draw counts as neither less nor equal.  The mirror of ahmc_glm_yrep_summary: this function DEFINES
    the order of its sums."""
    v = np.asarray(y_rep)
    if v.ndim != 2:
        raise ValueError(f"DimensionMismatch: y_rep {v.shape}, expected (n_new, S)")
    n_new, S = v.shape
    out = np.full((4, n_new), np.nan)
    if S == 0:
        return out
    out[0:2] = predict_summary(v[None], None, chunk)[0:2]
    if y is not None:
        yy = np.asarray(y, dtype=np.float64).reshape(n_new, 1)
        vd = v.astype(np.float64)
        with np.errstate(invalid="ignore"):
            out[2] = (vd < yy).sum(axis=1, dtype=np.int64) / float(S)
            out[3] = (vd == yy).sum(axis=1, dtype=np.int64) / float(S)
    return out
