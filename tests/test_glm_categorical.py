"""The categorical-logit family of the GLM target (include/ahmc_glm_categorical.h): y in unordered classes 0 … C − 1, class 0 the
reference, K = C − 1 coefficient blocks of P_b rows — k_glm_eta_cat makes the K predictors one class at a time into the K planes of U,
couples them through a log-sum-exp and turns the planes into u_k; every other kernel of the GLM targets runs unedited, class after
class.  The arithmetic is defined by advancedhmc.jl_amd/glm.py (`categorical_logdensity`).  Helpers come from tests/test_glm_target.py,
tests/test_glm_hier.py, tests/test_glm_aux.py and tests/test_glm_ordinal.py.

Shapes (n_obs, P_x, C): (70, 3, 3) two row blocks, the second partial; (1100, 4, 4) with a centred group inside block 1 and a
non-centred group that is the whole of block 2, 18 row blocks and two K slices, class 2 absent from y and class 1 absent from the
first row block, with a per-class offset; (130, 2, 2) binary; (130, 2, 16) the limit; (130, 2, 3) with factors (7, 1); (70, 3, 3) with
a per-class offset.  N = 37 (a partial tile under both shapes) or 48.

The bounds of the value comparison (`cat_check`; `cat_emulate` passes them on the host and fails them with each of three defects).
u = 2⁻⁵³ or 2⁻²⁴, γ_k = k·u/(1 − k·u); ε_exp twice the measured worst relative error of the device's exp on [−16, 16]
(tests/device_probe/glm.hip), ε_log and ε_inv twice those of log(s) and 1/s on s ∈ [1, 16] (tests/device_probe/glm_categorical.hip
against mpmath at 60 digits).  References are long double on the values as stored; the cases assert |η̂| <= 8, so every argument of
exp lies in [−16, 0].
  * η̂_k: Δη_k as in test_glm_hier.hier_check (γ_{P_b}·|X|·|W_k| + the rounding of the offset + |X|·E_W), the factors' gathers counted
    as columns.  Δ = max(Δη_1 … Δη_K) per element.
  * m is a selection: exact on η̂.  d_k = η̂_k − m is one rounding, |d_k|·u absolute, so ê_k = e_k(η̂)·(1 + ρ_k), ρ_k = ε_exp + |d_k|·u
    (e_0 = exp(−m): no subtraction, the same bound with d_0 = −m).  All terms of s are positive, K additions:
    ŝ = s(η̂)·(1 + ρ_s),  ρ_s = max_k ρ_k + γ_K.
  * lse is 1-Lipschitz in the sup norm:  |lse(η̂) − lse(η)| <= Δ.  log(ŝ) = log s + log(1 + ρ_s) and the log's own ε_log·log s; the
    additions m + log ŝ and η_y − lse round once each:
    E_ℓ = Δη_y + Δ + ρ_s + ε_log·log s + u·(|lse| + |ℓ|).
  * Σ_j |∂p_k/∂η_j| = 2·p_k·(1 − p_k) <= ½:  |p_k(η̂) − p_k(η)| <= Δ/2.  p̂_k = ê_k·(1/ŝ): ρ_k + ρ_s + ε_inv and one rounding of the product:
    E_p = Δ/2 + p_k·(ρ_k + ρ_s + ε_inv + u);   u_k = 1 − p_k or −p_k:  E_u = E_p + u·|u_k|.
  * Σℓ, R_k = −Xᵀu_k per class, the coefficient rows, the groups' rows and their terms of ℓπ: test_glm_hier.hier_check's bounds with
    (E_ℓ, E_u) above — ER = |X|ᵀ·E_u + γ_{n_obs+1}·|X|ᵀ(|u| + E_u), Σℓ through γ_{n_obs}.
SLACK = 1.01 covers products of two first-order terms.

C = 2 against the Bernoulli mirror (`test_binary_is_bernoulli`): m = max(0, η) and one term of s is exp(0) = 1, so s = 1 + e^{−|η|} = d
bit for bit; log(s) against log1p(e) differ by the rounding of 1 + e (<= u/s <= u) and the two functions' errors (<= 1 ulp = 2u each of
a value <= log 2): 4u together; lse = m + log s and softplus = max(η, 0) + log1p(e) round once each at their own size sp = softplus(η),
ℓ = η_y − lse and ℓ = yη − sp once each at the size of ℓ: |Δℓ| <= 4u + 2u·sp + 2u·|ℓ|.  p = e·(1/d) against e/d (or 1/d): two roundings against one,
|Δu| <= 4u.  ℓπ: Σ_i E_ℓ,i + 2·n·u·Σ|ℓ_i| + 16u·(prior + |ℓπ|); g: |X|ᵀ·4u + 2(n + 2)·u·|X|ᵀ·1 + 16u·(|g| + 1).
"""
import ctypes as C
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ahmc_amd as A
import test_buffer_bounds as TB
import test_glm_aux as TA
import test_glm_hier as TH
import test_glm_ordinal as TO
import test_glm_target as TG
from ahmc_amd import _capi as capi
from ahmc_amd import glm as G
from arena_util import In, Out
from test_glm_target import probe  # noqa: F401  (a fixture of the helpers)

LD = np.longdouble
ROOT = TG.ROOT
PROBE_C = os.path.join(ROOT, "tests", "device_probe", "glm_categorical.hip")
DTYPES = TG.DTYPES
gam, U, U_LD, SLACK = TG.gam, TG.U, TG.U_LD, TG.SLACK
record_bits, record_bound = TG.record_bits, TG.record_bound
MARGINS = TG.MARGINS
ETA_CAP = TG.ETA_MAX / 2
GROUPS2 = ((0, 2, True, 0.8), (4, 8, False, 1.3))      # (inside block 1; the whole of block 2)
# name: (n_obs, P_x, C, groups, levels, offset)
CASES = {"two-blocks": (70, 3, 3, (), (), False), "slices": (1100, 4, 4, GROUPS2, (), True), "binary": (130, 2, 2, (), (), False),
         "limit": (130, 2, 16, (), (), False), "factors": (130, 2, 3, (), (7, 1), False), "offset": (70, 3, 3, (), (), True)}
N_CHAINS = 37


# ------------------------------------------------------------------------------------------------
# the cases and their long-double references
# ------------------------------------------------------------------------------------------------
def classes(name, n_obs, Cn, rs):
    y = rs.integers(0, Cn, size=n_obs)
    y[:Cn] = np.arange(Cn)
    if name == "slices":
        y[y == 2] = 3                      # class 2 is absent altogether
        y[:64][y[:64] == 1] = 0            # class 1 is absent from the first row block
        assert not (y == 2).any() and not (y[:64] == 1).any() and (y[64:] == 1).any()
    assert all((y == k).any() for k in range(Cn) if not (name == "slices" and k == 2))
    return y


@functools.lru_cache(maxsize=None)
def ccase(name, N, dtname):
    """operands of one case in the element type and its long-double references, computed once"""
    n_obs, Px, Cn, groups, levels, has_off = CASES[name]
    dtype = np.dtype(dtname)
    rs = np.random.default_rng([n_obs, Px, Cn, len(groups), len(levels), N, dtype.itemsize, int(has_off)])
    X = np.asfortranarray(rs.normal(size=(n_obs, Px)) / np.sqrt(Px), dtype=dtype)
    factors = tuple(A.Factor(rs.integers(0, L, size=n_obs), L) for L in levels)
    K, Pb, Gn = Cn - 1, Px + sum(levels), len(groups)
    P = K * Pb
    th = np.asfortranarray(np.concatenate([0.4 * rs.normal(size=(P, N)), 0.25 * rs.normal(size=(Gn, N))]), dtype=dtype)
    y = classes(name, n_obs, Cn, rs)
    p = (2 * rs.random(P)).astype(dtype)
    p[::3] = 0
    for lo, hi, _, _ in groups:
        p[lo:hi] = 0
    off = np.asfortranarray(0.3 * rs.normal(size=(n_obs, K)), dtype=dtype) if has_off else None
    Xe = np.asfortranarray(G.expand_factors(X.astype(np.float64), factors), dtype=dtype)   # (0 and 1 are exact in either type)
    Xet = np.asfortranarray(Xe.T)
    ia2 = np.array([dtype.type(1.0 / (a * a)) for _, _, _, a in groups], dtype=dtype)
    D = P + Gn
    # ---- the references ----
    t = th.astype(LD)
    s = t[P:]
    tau = np.exp(s)
    W = t[:P].copy()
    for k, (lo, hi, cen, _) in enumerate(groups):
        if not cen:
            W[lo:hi] = tau[k] * t[lo:hi]
    ES = [TG.exact(Xe, W[k * Pb:(k + 1) * Pb]) for k in range(K)]
    eta = np.stack([ES[k][0] + (off[:, k].astype(LD).reshape(-1, 1) if has_off else 0) for k in range(K)])
    S_eta = np.stack([ES[k][1] for k in range(K)])
    assert np.abs(eta).max() <= 0.9 * ETA_CAP, (name, N, float(np.abs(eta).max()))     # (every argument of exp then lies in [−16, 0])
    ll, uu, pp = G.categorical_link(y, eta)
    assert ll.dtype == LD and uu.dtype == LD
    GS = [TG.exact(Xet, uu[k]) for k in range(K)]
    R = -np.concatenate([GS[k][0] for k in range(K)])
    Sg = np.concatenate([GS[k][1] for k in range(K)])
    pth = p.astype(LD).reshape(-1, 1) * t[:P]
    prior = (pth * t[:P]).sum(axis=0)
    lp0 = ll.sum(axis=0) - prior / 2
    g = np.empty((D, N), dtype=LD)
    g[:P] = pth + R
    grp = []
    for k, (lo, hi, cen, _) in enumerate(groups):
        m, a2 = LD(hi - lo), ia2[k].astype(LD)
        e2 = np.exp(2 * s[k])
        h, hp = s[k] - e2 * a2 / 2, 1 - e2 * a2
        Sk = (t[lo:hi] ** 2).sum(axis=0)
        q = np.exp(-2 * s[k])
        if cen:
            b = -m * s[k] - q * Sk / 2
            g[lo:hi] = q * t[lo:hi] + R[lo:hi]
            g[P + k] = m - q * Sk - hp
        else:
            b = -Sk / 2
            g[lo:hi] = tau[k] * R[lo:hi] + t[lo:hi]
            g[P + k] = (R[lo:hi] * W[lo:hi]).sum(axis=0) - hp
        grp.append({"e2a": e2 * a2, "h": h, "hp": hp, "S": Sk, "q": q, "b": b})
    lp = lp0 + sum(x["h"] + x["b"] for x in grp)
    return {"name": name, "X": X, "Xe": Xe, "Xet": Xet, "y": y, "yT": y.astype(dtype), "off": off, "p": p, "th": th, "dtype": dtype, "groups": groups,
            "factors": factors, "Px": Px, "Pb": Pb, "P": P, "K": K, "D": D, "C": Cn, "ia2": ia2, "tau": tau, "W": W, "S_eta": S_eta, "eta": eta, "ll": ll,
            "u": uu, "prob": pp, "Sg": Sg, "R": R, "prior": prior, "lp0": lp0, "grp": grp, "g": g, "lp": lp}


def target(c, onehot=False):
    """the case's model; `onehot`: the factors written as one-hot columns of X"""
    kw = dict(family="categorical_logit", n_categories=c["C"], prior_prec=c["p"], offset=c["off"])
    X, fk = (c["Xe"], {}) if onehot or not c["factors"] else (c["X"], {"factors": c["factors"]})
    return A.HierGLMTarget(X, c["y"], c["groups"], **kw, **fk) if c["groups"] else A.GLMTarget(X, c["y"], **kw, **fk)


def eta_chain(c, W):
    """η̂ (K, n_obs, N): the k-ordered fma chain of each class's block of the given W (the factors as one-hot columns), then the offset"""
    Pb = c["Pb"]
    return np.stack([TG.chain(c["Xe"], np.asfortranarray(W[k * Pb:(k + 1) * Pb])) + (c["off"][:, k].reshape(-1, 1) if c["off"] is not None else c["dtype"].type(0))
                     for k in range(c["K"])])


def link_bounds(c, eps, eta_hat, d_eta):
    """(E_ℓ, E_u (K, …), E_p (C, …)) of the module docstring, element by element"""
    u = U[c["dtype"]]
    ee, elog, einv = (LD(eps[k]) for k in ("exp", "log", "inv"))
    K = c["K"]
    eh = eta_hat.astype(LD)
    assert np.abs(eh).max() <= ETA_CAP
    m = np.maximum(eh.max(axis=0), 0)
    d = np.concatenate([-m[None], eh - m])                        # (C, …): the arguments of exp
    rho = ee + np.abs(d) * u
    rho_s = rho.max(axis=0) + gam(K, u)
    Dl = d_eta.max(axis=0)
    yc = c["y"].reshape(-1, 1)
    d_y = np.zeros_like(Dl)
    for k in range(K):
        d_y = np.where(yc == k + 1, d_eta[k], d_y)
    lse = -c["ll"] + np.where(yc == 0, 0, np.take_along_axis(c["eta"], np.maximum(yc - 1, 0)[None].repeat(eh.shape[2], axis=2), axis=0)[0])
    s = np.exp(lse - np.maximum(c["eta"].max(axis=0), 0))
    El = d_y + Dl + rho_s + elog * np.log(s) + u * (np.abs(lse) + np.abs(c["ll"]))
    Ep = Dl / 2 + c["prob"] * (rho + rho_s + einv + u)
    Eu = Ep[1:] + u * np.abs(c["u"])
    ld = 8 * U_LD * (np.abs(c["ll"]) + 1)
    return SLACK * El + ld, SLACK * Eu + ld, SLACK * Ep + ld


def cat_check(key, c, eps, W=None, tau=None, ll=None, lp=None, g=None, eta=None, prob=None):
    """the assertions of the value test on whatever results are given (the device's, or a host emulation's); `W` (the results' own
    effective coefficients, which fix η̂) is needed for everything but tau"""
    dtype, P, Pb, K, groups = c["dtype"], c["P"], c["Pb"], c["K"], c["groups"]
    n_obs = c["X"].shape[0]
    u, ee = U[dtype], LD(eps["exp"])
    t = c["th"].astype(LD)
    absW = np.abs(c["W"])
    Ew = np.zeros_like(absW)
    for lo, hi, cen, _ in groups:
        if not cen:
            Ew[lo:hi] = SLACK * (ee + u) * absW[lo:hi]
    ld = gam(n_obs + P + 64, U_LD)
    if tau is not None and len(groups):
        record_bound(f"cat-tau {key}", np.abs(tau.astype(LD) - c["tau"]), SLACK * ee * c["tau"] + ld * c["tau"])
    if W is None:
        return
    record_bound(f"cat-W {key}", np.abs(W.astype(LD) - c["W"]), Ew + ld * absW)
    absX = np.abs(c["Xe"]).astype(LD)
    eta_hat = eta_chain(c, W)
    if eta is not None:
        record_bits(f"cat-eta {key}", eta, eta_hat)
    d_eta = np.stack([(gam(Pb, u) + gam(Pb + 1, U_LD)) * c["S_eta"][k] * SLACK + (u + U_LD) * np.abs(eta_hat[k].astype(LD)) + absX @ Ew[k * Pb:(k + 1) * Pb]
                      for k in range(K)])
    El, Eu, Ep = link_bounds(c, eps, eta_hat, d_eta)
    if ll is not None:
        record_bound(f"cat-loglik {key}", np.abs(ll.astype(LD) - c["ll"]), El)
    if prob is not None:
        record_bound(f"cat-probs {key}", np.abs(prob.astype(LD) - c["prob"]), Ep)
    if lp is None and g is None:
        return
    XE = np.concatenate([absX.T @ Eu[k] for k in range(K)])
    ER = SLACK * (XE + (gam(n_obs + 1, u) + gam(n_obs + 1, U_LD)) * (c["Sg"] + XE))
    absR = np.abs(c["R"])
    Eg = np.empty_like(c["g"])
    Eg[:P] = ER
    Elp = El.sum(axis=0) + (gam(n_obs, u) + gam(n_obs, U_LD)) * (np.abs(c["ll"]) + El).sum(axis=0) + gam(P + 1, u) * c["prior"] / 2
    run = np.abs(c["lp0"])
    Elp = Elp + u * run
    for k, (lo, hi, cen, _) in enumerate(groups):     # (test_glm_hier.hier_check)
        x = c["grp"][k]
        m = hi - lo
        gc = gam((m + 63) // 64 + 6, u)
        ES = gc * x["S"]
        Ehp = ee * x["e2a"] + u * np.abs(x["hp"])
        Eh = ee * x["e2a"] / 2 + u * np.abs(x["h"])
        tk = c["tau"][k]
        if cen:
            EqS = ee * x["q"] * x["S"] + x["q"] * (1 + ee) * ES
            Eg[lo:hi] = ee * x["q"] * np.abs(t[lo:hi]) + ER[lo:hi]
            Eg[P + k] = EqS + u * np.abs(m - x["q"] * x["S"]) + Ehp
            Eb = EqS / 2 + u * x["q"] * x["S"] / 2 + u * np.abs(x["b"])
        else:
            Eg[lo:hi] = ee * tk * absR[lo:hi] + tk * (1 + ee) * ER[lo:hi]
            wb, rb = absW[lo:hi] + Ew[lo:hi], absR[lo:hi] + ER[lo:hi]
            Eg[P + k] = (ER[lo:hi] * wb + absR[lo:hi] * Ew[lo:hi]).sum(axis=0) + gc * (rb * wb).sum(axis=0) + Ehp
            Eb = ES / 2
        hb = np.abs(x["h"] + x["b"])
        run = run + hb
        Elp = Elp + Eh + Eb + u * hb + u * run
    if lp is not None:
        record_bound(f"cat-lp {key}", np.abs(lp.astype(LD) - c["lp"]), SLACK * Elp + ld * (np.abs(c["ll"]).sum(axis=0) + run))
    if g is not None:
        mag = np.abs(c["g"]) + 1
        mag[:P] += c["Sg"] * (1 + (np.abs(c["tau"]).max(axis=0) if len(groups) else 0))
        record_bound(f"cat-grad {key}", np.abs(g.astype(LD) - c["g"]), SLACK * (Eg + u * np.abs(g.astype(LD))) + ld * mag)


def cat_emulate(c, defect=None):
    """the device's arithmetic on the host in the element type and in the contract's order, numpy's functions for the device's.
    `defect`: "no_e0" leaves the reference's term e_0 out of s, "y_off_by_one" takes u_k = 1 − p_k where y = k − 1, "swap_planes"
    exchanges the first and the last plane of u before Xᵀu."""
    dtype, dt, P, Pb, K, groups = c["dtype"], c["dtype"].type, c["P"], c["Pb"], c["K"], c["groups"]
    th = c["th"]
    b, s = th[:P], th[P:]
    tau = np.exp(s)
    W = b.copy()
    for k, (lo, hi, cen, _) in enumerate(groups):
        if not cen:
            W[lo:hi] = tau[k] * b[lo:hi]
    eta_hat = eta_chain(c, W)
    y = c["y"]
    ll, uu, pp = G.categorical_link(y, eta_hat)
    assert all(a.dtype == dtype for a in (ll, uu, pp))
    if defect == "no_e0":
        m = np.maximum(eta_hat.max(axis=0), dt(0))
        e = np.exp(eta_hat - m)
        s_bad = e.sum(axis=0, dtype=dtype)
        eta_y = np.where(y.reshape(-1, 1) == 0, dt(0), np.take_along_axis(eta_hat, np.maximum(y - 1, 0).reshape(1, -1, 1).repeat(eta_hat.shape[2], axis=2), axis=0)[0])
        ll = (eta_y - (m + np.log(s_bad))).astype(dtype)
        pk = (e * (dt(1) / s_bad)).astype(dtype)
        uu = np.stack([np.where(y.reshape(-1, 1) == k + 1, dt(1) - pk[k], -pk[k]) for k in range(K)]).astype(dtype)
    elif defect == "y_off_by_one":
        uu = np.stack([np.where(y.reshape(-1, 1) == k, dt(1) - pp[k + 1], -pp[k + 1]) for k in range(K)]).astype(dtype)
    elif defect == "swap_planes":
        uu = uu[::-1].copy()
    zero = np.zeros(Pb, dtype=dtype)
    R = np.concatenate([TG.grad_model(c["Xet"], np.asfortranarray(uu[k]), zero, np.asfortranarray(W[k * Pb:(k + 1) * Pb])) for k in range(K)])   # (fma(0, w, −Σ) = −Xᵀu)
    lsum = TO.lane_tree(TO.block_sums_in(ll))
    lp, g = TA._in_dtype_finish(c, W, tau, R, lsum)
    assert lp.dtype == dtype and g.dtype == dtype
    return {"W": W, "tau": tau, "eta": eta_hat, "ll": ll, "lp": lp, "g": g, "prob": pp, "u": uu}


def log_inv_grid(dtype):
    rs = np.random.default_rng(4)
    return np.concatenate([np.linspace(1.0, 16.0, 4001), 1 + np.logspace(-16, 0, 2001), rs.uniform(1.0, 16.0, 4000)]).astype(dtype)


def log_inv_eps(fn, dtype):
    """twice the worst relative errors of log(s) and 1/s as `fn` computes them on s ∈ [1, 16], against mpmath at 60 digits"""
    import mpmath as mp

    dtype = np.dtype(dtype)
    s = log_inv_grid(dtype)
    L, R = (np.asarray(v) for v in fn(s))
    assert L.dtype == dtype and R.dtype == dtype
    worst = {"log": 0.0, "inv": 0.0}
    with mp.workdps(60):
        for i in range(s.size):
            x = mp.mpf(float(s[i]))
            if x > 1:
                worst["log"] = max(worst["log"], float(abs((mp.mpf(float(L[i])) - mp.log(x)) / mp.log(x))))
            else:
                assert L[i] == 0
            worst["inv"] = max(worst["inv"], float(abs(mp.mpf(float(R[i])) * x - 1)))
    u = float(U[dtype])
    out = {"log": 2 * worst["log"], "inv": 2 * worst["inv"], "log_worst_u": worst["log"] / u, "inv_worst_u": worst["inv"] / u}
    assert out["log_worst_u"] < 16 and out["inv_worst_u"] < 4, out   # (a function this far off is a finding of its own, not a margin)
    return out


@functools.lru_cache(maxsize=None)
def host_eps(dtname):
    """numpy's functions in the place of the device's"""
    dtype = np.dtype(dtname)
    eps = dict(TG.function_eps(np.exp, np.log1p, dtype))
    eps.update(log_inv_eps(lambda s: (np.log(s), dtype.type(1) / s), dtype))
    return eps


def dump_profile():
    """the categorical entries of the margins → $AHMC_TEST_OUT/glm_categorical_margins.json (copied to profiles/ by whoever runs the suite)"""
    out = os.environ.get("AHMC_TEST_OUT") or os.path.join(ROOT, "test_out")
    try:
        os.makedirs(out, exist_ok=True)
        mine = {k: v for k, v in sorted(MARGINS.items()) if k.startswith("cat-")}
        worst = {}
        for k, v in mine.items():
            if "error_over_bound" in v:
                worst[k.split(" ")[0]] = max(worst.get(k.split(" ")[0], 0.0), v["error_over_bound"])
        bits = {"compared": sum(v.get("bit_compared", 0) for v in mine.values()), "mismatch": sum(v.get("bit_mismatch", 0) for v in mine.values())}
        with open(os.path.join(out, "glm_categorical_margins.json"), "w") as f:
            json.dump({"worst_error_over_bound_per_quantity": worst, "elements_compared_bit_for_bit": bits, "cases": mine}, f, indent=1)
    except OSError:
        pass


# ------------------------------------------------------------------------------------------------
# CPU 1: the mirror
# ------------------------------------------------------------------------------------------------
def small_model(Cn, rs, groups=(), n_obs=23, Px=3, N=2):
    K = Cn - 1
    X = rs.normal(size=(n_obs, Px)) / 2
    y = rs.integers(0, Cn, size=n_obs)
    y[:Cn] = np.arange(Cn)
    th = np.concatenate([rs.normal(size=(K * Px, N)), 0.3 * rs.normal(size=(len(groups), N))])
    off = 0.2 * rs.normal(size=(n_obs, K))
    p = 0.5 + rs.random(K * Px)
    for lo, hi, _, _ in groups:
        p[lo:hi] = 0
    return X, y, th, off, p


def lp_mp(X, y, th, Cn, groups, off, p):
    """ℓπ of one chain straight from the definition, in mpmath at 40 digits"""
    import mpmath as mp

    K, Px = Cn - 1, X.shape[1]
    P = K * Px
    with mp.workdps(40):
        t = [mp.mpf(float(v)) for v in th]
        w = list(t[:P])
        lp = mp.mpf(0)
        for k, (lo, hi, cen, Asc) in enumerate(groups):
            sk = t[P + k]
            tau = mp.exp(sk)
            m = hi - lo
            S = sum(t[d] ** 2 for d in range(lo, hi))
            lp += sk - mp.exp(2 * sk) / (2 * mp.mpf(Asc) ** 2)                     # half-normal(A) on τ with the Jacobian of s = log τ
            if cen:
                lp += -m * sk - S / (2 * tau ** 2)
            else:
                lp += -S / 2
                for d in range(lo, hi):
                    w[d] = tau * t[d]
        for d in range(P):
            lp -= mp.mpf(float(p[d])) * t[d] ** 2 / 2
        for i in range(X.shape[0]):
            eta = [mp.mpf(0)] + [sum(mp.mpf(float(X[i, j])) * w[k * Px + j] for j in range(Px)) + mp.mpf(float(off[i, k])) for k in range(K)]
            lp += eta[int(y[i])] - mp.log(sum(mp.exp(e) for e in eta))
        return lp


@pytest.mark.parametrize("Cn", [2, 3, 5])
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "groups"])
def test_mirror_against_mpmath_and_central_differences(Cn, grouped):
    """ℓπ of the mirror against the definition in mpmath (40 digits), and ∇ℓπ against central differences of it (h = 1e-6: truncation
    h²·|ℓπ‴|/6 ≈ 1e-11)"""
    import mpmath as mp

    rs = np.random.default_rng(20 + Cn)
    groups = ((0, 2, True, 0.9),) + (((3, 6, False, 1.4),) if Cn > 2 else ()) if grouped else ()
    X, y, th, off, p = small_model(Cn, rs, groups)
    lp, grad = G.categorical_logdensity(X, y, th, Cn, groups, off, p)
    for n in range(th.shape[1]):
        ref = lp_mp(X, y, th[:, n], Cn, groups, off, p)
        assert abs(float(lp[n] - float(ref))) <= 1e-12 * (1 + abs(float(ref)))
        with mp.workdps(40):
            for d in range(th.shape[0]):
                tp, tm = [mp.mpf(float(v)) for v in th[:, n]], [mp.mpf(float(v)) for v in th[:, n]]
                tp[d] += mp.mpf("1e-6")
                tm[d] -= mp.mpf("1e-6")
                fd = (lp_mp(X, y, tp, Cn, groups, off, p) - lp_mp(X, y, tm, Cn, groups, off, p)) / mp.mpf("2e-6")
                assert abs(grad[d, n] - float(fd)) <= 1e-8 * (1 + abs(float(fd))), (d, n, grad[d, n], float(fd))
    eta, ll = G.categorical_pointwise(X, y, th, Cn, groups, off)
    assert eta.shape == (Cn - 1, X.shape[0], th.shape[1]) and ll.shape == eta.shape[1:]
    pr = G.categorical_probs(eta)
    np.testing.assert_allclose(pr.sum(axis=0), 1.0, rtol=1e-14)
    np.testing.assert_allclose(np.log(np.take_along_axis(pr, y.reshape(1, -1, 1).repeat(th.shape[1], axis=2), axis=0)[0]), ll, rtol=1e-13, atol=1e-13)
    lp1, g1 = G.categorical_logdensity(X, y, th[:, 0], Cn, groups, off, p)          # a vector θ is one chain
    np.testing.assert_allclose(lp1[0], lp[0], rtol=1e-14)
    np.testing.assert_allclose(g1[:, 0], grad[:, 0], rtol=1e-13, atol=1e-14)


def test_mirror_extremes():
    """|η| up to 800 (88 in Float32): ℓ, u and p finite with the right limits; a NaN or +∞ predictor makes ℓ NaN, which sanitises to −Inf"""
    for dtype, top in ((np.float64, 800.0), (np.float32, 88.0)):
        eta = np.array([[top, -top, top - 1], [-top, -top, -top], [top, top, -top], [0.0, 0.0, 0.0]], dtype=dtype).T.reshape(3, 4, 1)
        for yv in range(4):
            ll, u, p = G.categorical_link(np.full(4, yv), eta)
            assert ll.dtype == dtype and np.isfinite(ll).all() and np.isfinite(u).all() and np.isfinite(p).all()
            np.testing.assert_allclose(p.sum(axis=0), 1.0, rtol=1e-6)
        ll, u, p = G.categorical_link(np.array([1, 0, 2, 3]), eta)
        # (lse = m + log s rounds at the size of m: an absolute error of a few units in the last place of `top`)
        np.testing.assert_allclose(ll[:, 0], [-np.log1p(np.exp(-1.0)), 0.0, -np.log(2.0), -np.log(4.0)], rtol=1e-6, atol=4 * np.finfo(dtype).eps * top)
        np.testing.assert_allclose(u[:, 0, 0], [1 - 1 / (1 + np.exp(-1.0)), 0.0, -1 / (1 + np.e)], rtol=1e-6, atol=1e-30)
    for bad in (np.nan, np.inf):
        ll, _, _ = G.categorical_link(np.array([0, 1]), np.array([[bad, bad], [0.3, 0.3]]).reshape(2, 2, 1))
        assert np.isnan(ll).all() and (G.sanitize(ll) == -np.inf).all()
    ll, u, p = G.categorical_link(np.array([0, 1]), np.array([[-np.inf, -np.inf], [0.3, 0.3]]).reshape(2, 2, 1))     # a class of probability 0
    assert np.isfinite(ll[0, 0]) and ll[1, 0] == -np.inf and p[1, 0, 0] == 0 and G.sanitize(ll)[1, 0] == -np.inf


def test_binary_is_bernoulli():
    """C = 2 is the Bernoulli-logit model: ℓ, u and (ℓπ, g) of the two mirrors inside the bounds of the module docstring"""
    rs = np.random.default_rng(5)
    n_obs, Px, N = 130, 3, 4
    X = rs.normal(size=(n_obs, Px))
    y = (rs.random(n_obs) < 0.5).astype(np.int64)
    th = 1.5 * rs.normal(size=(Px, N))
    off, p = 0.3 * rs.normal(size=n_obs), 0.5 + rs.random(Px)
    u = 2.0 ** -53
    eta_c, ll_c = G.categorical_pointwise(X, y, th, 2, (), off.reshape(-1, 1))
    eta_b, ll_b = G.pointwise("bernoulli_logit", X, y.astype(float), th, off)
    np.testing.assert_array_equal(eta_c[0], eta_b)
    _, u_c, _ = G.categorical_link(y, eta_c)
    _, u_b = G.link("bernoulli_logit", y.reshape(-1, 1).astype(float), eta_b)
    sp = y.reshape(-1, 1) * eta_b - ll_b
    El = 4 * u + 2 * u * sp + 2 * u * np.abs(ll_b)
    assert np.all(np.abs(ll_c - ll_b) <= El), (np.abs(ll_c - ll_b) / El).max()
    assert np.all(np.abs(u_c[0] - u_b) <= 4 * u), (np.abs(u_c[0] - u_b) / (4 * u)).max()
    lp_c, g_c = G.categorical_logdensity(X, y, th, 2, (), off.reshape(-1, 1), p)
    lp_b, g_b = G.logdensity("bernoulli_logit", X, y.astype(float), th, off, p)
    prior = 0.5 * (p.reshape(-1, 1) * th * th).sum(axis=0)
    b_lp = El.sum(axis=0) + 2 * n_obs * u * np.abs(ll_b).sum(axis=0) + 16 * u * (prior + np.abs(lp_b))
    b_g = np.abs(X).T @ np.full_like(ll_b, 4 * u) + 2 * (n_obs + 2) * u * (np.abs(X).T @ np.ones_like(ll_b)) + 16 * u * (np.abs(g_b) + 1)
    assert np.all(np.abs(lp_c - lp_b) <= b_lp) and np.all(np.abs(g_c - g_b) <= b_g)
    MARGINS["cat-binary-is-bernoulli"] = {"error_over_bound": float(max((np.abs(ll_c - ll_b) / El).max(), (np.abs(u_c[0] - u_b) / (4 * u)).max(),
                                                                         (np.abs(lp_c - lp_b) / b_lp).max(), (np.abs(g_c - g_b) / b_g).max()))}
    dump_profile()


# ------------------------------------------------------------------------------------------------
# CPU 2: header == binding table == Julia ccalls == exported symbols; the kernels
# ------------------------------------------------------------------------------------------------
def header_prototypes():
    src = open(os.path.join(ROOT, "include", "ahmc_glm_categorical.h"), encoding="utf-8").read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(int32_t)\s+(ahmc_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        params = " ".join(m.group(3).split())
        protos[m.group(2)] = [] if params in ("", "void") else [p.strip() for p in params.split(",")]
    return protos, src


def test_header_and_bindings_agree():
    protos, src = header_prototypes()
    assert set(protos) == set(capi.GLM_CATEGORICAL_SIGNATURES) == {"ahmc_glm_categorical_version", "ahmc_glm_categorical_set_target",
                                                                  "ahmc_glm_categorical_get_target", "ahmc_glm_class_probs"}
    older = (set(capi.GLM_SIGNATURES) | set(capi.HGLM_SIGNATURES) | set(capi.GLM_AUX_SIGNATURES) | set(capi.GLM_FACTOR_SIGNATURES) | set(capi.GLM_ORDINAL_SIGNATURES)
             | set(capi.SIGNATURES))
    assert not set(capi.GLM_CATEGORICAL_SIGNATURES) & older
    ct = {"int64_t*": C.POINTER(C.c_int64), "int32_t*": C.POINTER(C.c_int32), "double*": C.POINTER(C.c_double), "int64_t": C.c_int64,
          "int32_t": C.c_int32, "double": C.c_double}
    for name, params in protos.items():
        res, args = capi.GLM_CATEGORICAL_SIGNATURES[name]
        assert res is C.c_int32 and len(args) == len(params), name
        for p, a in zip(params, args):
            typ = p.rsplit(" ", 1)[0].replace("const ", "").replace(" ", "")
            if typ in ("void*", "ahmc_ctx*"):
                assert a is C.c_void_p, (name, p)
            else:
                assert a is ct[typ], (name, p)
    # ahmc_glm_ordinal_set_target's arguments without cut_prior
    ordn = [p.split()[-1] for p in TO.header_prototypes()[0]["ahmc_glm_ordinal_set_target"]]
    assert [p.split()[-1] for p in protos["ahmc_glm_categorical_set_target"]] == [a for a in ordn if a != "cut_prior"]
    assert [p.split()[-1] for p in protos["ahmc_glm_class_probs"]] == ["ctx", "theta", "n_cols", "out"]
    assert [p.split()[-1] for p in protos["ahmc_glm_categorical_get_target"]] == ["ctx", "n_categories", "block_len"]
    assert re.search(r"#define AHMC_GLM_CATEGORICAL_VERSION (\d+)", src).group(1) == str(capi.AHMC_GLM_CATEGORICAL_VERSION) == "1"
    assert (re.search(r"#define AHMC_GLM_CATEGORICAL_MAX_CATEGORIES (\d+)", src).group(1) == str(capi.GLM_CATEGORICAL_MAX_CATEGORIES)
            == str(G.CATEGORICAL_MAX_CATEGORIES) == "16")
    assert re.search(r"AHMC_GLM_CATEGORICAL_LOGIT = (\d+)", src).group(1) == str(capi.GLM_CATEGORICAL_LOGIT) == str(G.CATEGORICAL_LOGIT) == "6"
    assert G.CATEGORICAL_FAMILIES == {"categorical_logit": 6}
    assert '#include "ahmc_glm_factor.h"' in src
    from ahmc_amd import build as B
    assert "ahmc_glm_categorical.h" in open(B.__file__, encoding="utf-8").read()
    dev = open(os.path.join(ROOT, "advancedhmc.jl_amd", "csrc", "ahmc_glm.hpp"), encoding="utf-8").read()
    assert re.search(r"constexpr int GLM_CAT_MAX_CAT = (\d+);", dev).group(1) == "16"
    # the older headers keep their versions; both headers say what ahmc_glm_pointwise writes for this family
    inc = os.path.join(ROOT, "include")
    hip_h = open(os.path.join(inc, "ahmc_hip.h"), encoding="utf-8").read()
    assert "glm" not in hip_h.lower() and re.search(r"#define AHMC_ABI_VERSION (\d+)", hip_h).group(1) == "6" == str(capi.AHMC_ABI_VERSION)
    for hdr, macro, v in (("ahmc_glm.h", "AHMC_GLM_VERSION", capi.AHMC_GLM_VERSION), ("ahmc_glm_hier.h", "AHMC_HGLM_VERSION", capi.AHMC_HGLM_VERSION),
                          ("ahmc_glm_aux.h", "AHMC_GLM_AUX_VERSION", capi.AHMC_GLM_AUX_VERSION),
                          ("ahmc_glm_factor.h", "AHMC_GLM_FACTOR_VERSION", capi.AHMC_GLM_FACTOR_VERSION),
                          ("ahmc_glm_ordinal.h", "AHMC_GLM_ORDINAL_VERSION", capi.AHMC_GLM_ORDINAL_VERSION)):
        assert re.search(rf"#define {macro} (\d+)", open(os.path.join(inc, hdr), encoding="utf-8").read()).group(1) == str(v) == "1"
    for hdr in ("ahmc_glm.h", "ahmc_glm_categorical.h"):
        text = " ".join(open(os.path.join(inc, hdr), encoding="utf-8").read().split())
        assert re.search(r"eta_out then holds K planes of \* ?\(n_obs, N\)|eta_out then holds K planes of \(n_obs, N\)", text), hdr
    assert G.FAMILIES == {"bernoulli_logit": 0, "poisson_log": 1, "gaussian_identity": 2, "gaussian_identity_sigma": 3, "negbinomial_log": 4}
    with pytest.raises(ValueError, match="unknown GLM family"):
        G.family_code("categorical_logit")


def test_julia_ccalls_match_the_header():
    protos, _ = header_prototypes()
    src = open(os.path.join(ROOT, "julia", "AdvancedHMCMI355XGLMCategorical.jl"), encoding="utf-8").read()
    src = re.sub(r"#[^\n]*", "", src)
    seen = set()
    for m in re.finditer(r"ccall\(\(:(ahmc_[a-z_0-9]+), LIB\),\s*(\w+),\s*\(", src):
        i, depth = m.end(), 1
        while depth:
            depth += {"(": 1, ")": -1}.get(src[i], 0)
            i += 1
        body, types, cur, depth = src[m.end():i - 1], [], "", 0
        for ch in body:
            depth += {"{": 1, "}": -1, "(": 1, ")": -1}.get(ch, 0)
            if ch == "," and depth == 0:
                types.append(cur.strip())
                cur = ""
            else:
                cur += ch
        if cur.strip():
            types.append(cur.strip())
        name = m.group(1)
        assert name not in seen, f"{name}: one ccall per entry"
        seen.add(name)
        assert m.group(2) == "Cint" and len(types) == len(protos[name]), (name, types)
        for t, p in zip(types, protos[name]):
            if "*" in p:
                assert t.startswith(("Ptr{", "Ref{")), (name, t, p)
            else:
                assert {"int64_t": "Int64", "int32_t": "Cint", "double": "Cdouble"}[p.split()[0]] == t, (name, t, p)
    assert seen == set(protos)
    ext = open(os.path.join(ROOT, "julia", "AdvancedHMCMI355XExt.jl"), encoding="utf-8").read()
    assert 'include("AdvancedHMCMI355XGLMCategorical.jl")' in ext and "ahmc_glm_categorical_set_target" not in ext
    assert ext.index('include("AdvancedHMCMI355XGLMOrdinal.jl")') < ext.index('include("AdvancedHMCMI355XGLMCategorical.jl")')


NEW_KERNELS = [f"k_glm_eta_cat<{t}, {bn}, {fac}>" for t in ("float", "double") for bn in (64, 16) for fac in ("false", "true")]


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="needs llvm-objdump")
def test_library_exports_and_kernels_without_scratch():
    """every entry point is in the dynamic symbol table (read without loading the library); the eight instantiations of the new kernel
    are in the code object with no private segment and no vector-register spill (scripts/kernel_meta.py); each fits two waves per SIMD
    by its registers (VGPR + AGPR <= 256) and two workgroups per CU by its LDS (<= 80 KiB)"""
    from ahmc_amd import build as B

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_meta
    finally:
        sys.path.pop(0)
    assert os.path.exists(B.OUT), "build() first"
    exported = {l.split()[-1] for l in subprocess.run(["nm", "-D", "--defined-only", B.OUT], capture_output=True, text=True, check=True).stdout.splitlines() if l.strip()}
    assert set(capi.GLM_CATEGORICAL_SIGNATURES) <= exported, set(capi.GLM_CATEGORICAL_SIGNATURES) - exported
    meta = kernel_meta.kernel_meta(B.OUT)
    names = subprocess.run(["c++filt"], input="\n".join(k["name"] for k in meta), capture_output=True, text=True, check=True).stdout.splitlines()
    found = {}
    for k, dn in zip(meta, names):
        for w in NEW_KERNELS:
            if dn.startswith(f"void ahmc::{w}("):
                found[w] = k
    assert sorted(found) == sorted(NEW_KERNELS), sorted(set(NEW_KERNELS) - set(found))
    for w, k in found.items():
        assert k["private_segment_fixed_size"] == 0, (w, k)
        assert k.get("vgpr_spill_count", 0) == 0, (w, k)
        assert k["vgpr_count"] + k.get("agpr_count", 0) <= 256, (w, k)
        assert k["group_segment_fixed_size"] <= 80 * 1024, (w, k)


# ------------------------------------------------------------------------------------------------
# CPU 3: the constructor, misuse, the checker's refusal
# ------------------------------------------------------------------------------------------------
def test_constructor_and_refusals():
    rs = np.random.default_rng(2)
    n = 20
    X, y = rs.normal(size=(n, 3)), rs.integers(0, 4, size=n)
    y[:4] = np.arange(4)
    t = A.GLMTarget(X, y, family="categorical_logit", n_categories=4, prior_scale=2.0)
    assert (t.family, t.n_classes, t.n_categories, t.D, t.P, t.P_b, t.P_x, t.aux) == (6, 4, 0, 9, 9, 3, 3, False)
    assert [t.class_rows(k) for k in (1, 2, 3)] == [(0, 3), (3, 6), (6, 9)] and t.prior_prec.shape == (9,)
    off = rs.normal(size=(n, 3))
    h = A.HierGLMTarget(X, y, [A.CoefGroup(0, 2, False, 1.0), A.CoefGroup(5, 15, True, 2.0)], family="categorical_logit", n_categories=4, factors=[A.Factor(y % 2, 2)],
                        offset=off)
    assert (h.D, h.P, h.P_b, h.class_rows(3), h.factor_ranges) == (15 + 2, 15, 5, (10, 15), [(3, 5)])
    th = rs.normal(size=(h.D, 2))
    lp, g = h.logdensity(th)
    lp2, g2 = G.categorical_logdensity(h.X, y, th, 4, [(0, 2, False, 1.0), (5, 15, True, 2.0)], off, None, factors=[(y % 2, 2)])
    np.testing.assert_array_equal(lp, lp2)
    np.testing.assert_array_equal(g, g2)
    beta, tau = h.coefficients(th)
    assert beta.shape == (15, 2) and tau.shape == (2, 2)
    pr = h.class_probs(th)
    assert pr.shape == (4, n, 2)
    np.testing.assert_allclose(pr.sum(axis=0), 1.0, rtol=1e-14)
    assert A.GLMTarget(X, y, family=6, n_categories=4).family == 6
    for kw in (dict(family="categorical_logit"), dict(family="categorical_logit", n_categories=4, scale=2.0),
               dict(family="categorical_logit", n_categories=4, aux_prior=(0.0, 1.0)), dict(family="categorical_logit", n_categories=4, cut_prior=(0, 1, 0, 1)),
               dict(family="categorical_logit", n_categories=1), dict(family="categorical_logit", n_categories=17), dict(family="categorical_logit", n_categories=3),
               dict(family="categorical_logit", n_categories=4, offset=np.zeros(n)), dict(family="categorical_logit", n_categories=4, prior_prec=np.ones(3))):
        with pytest.raises(A.ArgumentError):
            A.GLMTarget(X, y, **kw)
    with pytest.raises(A.ArgumentError, match="DomainError.*not a category"):
        A.GLMTarget(X, np.where(np.arange(n) == 3, 1.5, y), family="categorical_logit", n_categories=4)
    with pytest.raises(A.ArgumentError, match="straddles"):
        A.HierGLMTarget(X, y, [A.CoefGroup(2, 5, False, 1.0)], family="categorical_logit", n_categories=4)
    with pytest.raises(A.ArgumentError, match="no class blocks"):
        A.GLMTarget(X, (y > 1).astype(float)).class_rows(1)
    with pytest.raises(A.ArgumentError, match="reference"):
        t.class_rows(0)
    for bad in (lambda: G.categorical_logdensity(X, y, np.zeros((8, 2)), 4), lambda: G.categorical_logdensity(X, y, np.zeros((9, 2)), 3),
                lambda: G.check_classes(y, 17), lambda: G.categorical_logdensity(X, y, np.zeros((9, 2)), 4, offset=np.zeros((n, 2))),
                lambda: G.check_class_groups([(1, 4, False, 1.0)], 3, 3)):
        with pytest.raises(ValueError):
            bad()
    assert G.check_class_groups([(0, 6, False, 1.0), (7, 9, True, 1.0)], 3, 3) == [(0, 6, False, 1.0), (7, 9, True, 1.0)]


def test_cpu_checker_refuses_the_target(oracle):
    assert oracle.has_glm_categorical is False
    c = ccase("two-blocks", 3, "float64")
    t = target(c)
    with pytest.raises(A.UnsupportedError, match="ahmc_glm_categorical.h"):
        A.Engine(A.Hamiltonian(A.UnitEuclideanMetric(t.D), t), 3, lib=oracle)
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric(t.D), A.IsoGaussian(t.D)), 3, lib=oracle)
    with pytest.raises(A.UnsupportedError, match="ahmc_glm_categorical.h"):
        e.set_target(t)
    with pytest.raises(A.UnsupportedError, match="ahmc_glm_categorical.h"):
        e.glm_class_probs()
    e.close()


# ------------------------------------------------------------------------------------------------
# CPU 4: the bounds on a host emulation, and planted defects
# ------------------------------------------------------------------------------------------------
def check_emulation(key, c, eps, r):
    cat_check(key, c, eps, W=r["W"], tau=r["tau"], ll=r["ll"], lp=r["lp"], g=r["g"], eta=r["eta"], prob=r["prob"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_bounds_hold_for_a_host_emulation_and_catch_three_defects(dtype):
    """the device's arithmetic emulated in the element type and in the contract's order passes every bound of the GPU value test on
    every case; with e_0 missing from s, with `y == k` off by one, or with the class planes swapped, an assertion of it fails"""
    dtname = np.dtype(dtype).name
    eps = host_eps(dtname)
    for name in CASES:
        c = ccase(name, 5, dtname)
        check_emulation(f"emulation {dtname} {name}", c, eps, cat_emulate(c))
        for N in (N_CHAINS, 48):
            ccase(name, N, dtname)        # (the GPU test's operands: built here once, with their own assertions on y and on the range of η)
    for name in ("two-blocks", "slices", "factors"):
        c = ccase(name, 5, dtname)
        for defect, what in (("no_e0", "cat-loglik"), ("y_off_by_one", "cat-grad"), ("swap_planes", "cat-grad")):
            r = cat_emulate(c, defect)
            keep = dict(MARGINS)
            with pytest.raises(AssertionError, match=what):
                check_emulation(f"defect-{defect} {dtname} {name}", c, eps, r)
            for k in set(MARGINS) - set(keep):        # (a planted defect's ratios are no margins of the code)
                del MARGINS[k]
    dump_profile()


# ------------------------------------------------------------------------------------------------
# CPU 5 / GPU 4: the parity inputs, and their precondition on the oracle alone
# ------------------------------------------------------------------------------------------------
# name: (n_obs, P_x, C, groups, seed)
PARITY = {"(130, 3, C = 4)": (130, 3, 4, (), 1), "(130, 3 + 2, C = 4)": (130, 3, 4, ((0, 3, True, 1.0), (3, 9, False, 1.0)), 1)}
DENSE_CASE = "(130, 3 + 2, C = 4)"
WIDE = (70, 1400, 4, ((10, 200, False, 1.0),), 1)


def parity_inputs(n_obs, Px, Cn, groups, seed, N=64):
    K, Gn = Cn - 1, len(groups)
    P = K * Px
    rs = np.random.default_rng([n_obs, Px, Gn, Cn, seed, 6])
    X = rs.normal(size=(n_obs, Px)) / np.sqrt(Px)
    eta = np.column_stack([np.zeros(n_obs), X @ rs.normal(size=(Px, K))])
    y = (eta + rs.gumbel(size=eta.shape)).argmax(axis=1)
    p = np.ones(P)
    for lo, hi, _, _ in groups:
        p[lo:hi] = 0
    D = P + Gn
    minv = np.asfortranarray(0.5 + rs.random((D, N)))
    th0 = 0.5 * rs.normal(size=(D, N)) * (0.2 if P > 1000 else 1.0)
    eps = 0.1 * (0.7 + 0.6 * rs.random(N))
    kw = dict(family="categorical_logit", n_categories=Cn, prior_prec=p)
    t = A.HierGLMTarget(X, y, groups, **kw) if groups else A.GLMTarget(X, y, **kw)
    return t, minv, th0, eps


@pytest.mark.parametrize("name", list(PARITY) + ["dense", "wide"])
def test_parity_precondition_on_the_oracle_alone(oracle, name):
    """On the inputs of the GPU comparison no decision of the oracle (running the mirror as a host kernel) comes within the suite's
    bound for float64 of a tie, at any step of the sequence and for any chain"""
    if name == "wide":
        t, _, th0, eps = parity_inputs(*WIDE, N=8)
        assert t.D > 4096
        o = TH.oracle_engine(oracle, t, A.UnitEuclideanMetric(th0.shape), 8)
        smallest, n_div = TG.parity_sequence(o, None, th0, eps, "glm-categorical wide", nuts_depth=5, full=False)
    else:
        t, minv, th0, eps = parity_inputs(*PARITY[DENSE_CASE if name == "dense" else name])
        o = TH.oracle_engine(oracle, t, TA.dense_metric(t.D) if name == "dense" else A.DiagEuclideanMetric(minv), th0.shape[1])
        smallest, n_div = TG.parity_sequence(o, None, th0, eps, f"glm-categorical {name}")
    MARGINS[f"cat-oracle-margin {name}"] = {"smallest_decision_margin": smallest, "divergent_chains_max": n_div}
    TG._dump_margins()
    dump_profile()
    o.close()


# ---------------------------------------------------------------------------------------------------------------------
# the guard-band cases of the new entry points: registered in the table of tests/test_buffer_bounds.py, whose gate counts them
# ---------------------------------------------------------------------------------------------------------------------
_PRE = "ahmc_glm_categorical_set_target"
_SET_IN = ("X", "y", "offset", "prior_prec", "lo", "hi", "centered", "hyper_scale", "n_levels", "levels")
_B_PX, _B_C, _B_LEVELS = 3, 3, (2, 3)
_B_PB = _B_PX + sum(_B_LEVELS)
_B_P = (_B_C - 1) * _B_PB


def c_categorical_set_target(r, n_obs, where):
    """every array of ahmc_glm_categorical_set_target: the data in device or host memory, the tables in host memory"""
    N, K = 5, _B_C - 1
    i32 = lambda v: np.array(v, dtype=np.int32)  # noqa: E731
    for dtype in (TB.F64, TB.F32):
        rs = np.random.default_rng(n_obs)
        d = {"X": rs.normal(size=n_obs * _B_PX).astype(dtype), "y": rs.integers(0, _B_C, n_obs).astype(dtype), "offset": (0.1 * rs.normal(size=n_obs * K)).astype(dtype),
             "prior_prec": np.array([0.5, 0, 0] + [1.0] * (_B_P - 3), dtype=dtype)}
        ins = {f"{_PRE}.{k}": In(v, where) for k, v in d.items()}
        tab = {"lo": i32([1]), "hi": i32([3]), "centered": i32([0]), "hyper_scale": np.array([1.5]), "n_levels": i32(_B_LEVELS),
               "levels": np.concatenate([rs.integers(0, L, n_obs) for L in _B_LEVELS]).astype(np.int32)}
        ins.update({f"{_PRE}.{k}": In(v, "host") for k, v in tab.items()})

        def call(e, io):
            p = lambda k: io[f"{_PRE}.{k}"]  # noqa: E731
            pi, pd = C.POINTER(C.c_int32), C.POINTER(C.c_double)
            r.ok(e, r.lib.dll.ahmc_glm_categorical_set_target(e._ctx, n_obs, _B_PX, p("X"), p("y"), p("offset"), p("prior_prec"), 1, C.cast(p("lo"), pi), C.cast(p("hi"), pi),
                                                              C.cast(p("centered"), pi), C.cast(p("hyper_scale"), pd), 2, C.cast(p("n_levels"), pi), C.cast(p("levels"), pi),
                                                              _B_C))
            out = TB.glm_observe(r, e, n_obs, dtype)
            out["probs"] = e.glm_class_probs()
            return out
        r.probe(lambda: TB.engine(r.lib, _B_P + 1, N, dtype, metric="unit", position=False), call, ins=ins)


def bound_categorical(r, n_obs, dtype, N=5):
    rs = np.random.default_rng(n_obs)
    X = rs.normal(size=(n_obs, _B_PX))
    t = A.HierGLMTarget(X, rs.integers(0, _B_C, n_obs), [A.CoefGroup(1, 3, False, 1.5)], family="categorical_logit", n_categories=_B_C,
                        offset=0.1 * rs.normal(size=(n_obs, _B_C - 1)))
    return TB.engine(r.lib, t.D, N, dtype, metric="unit", target=t)


def c_categorical_post(r, n_obs, where):
    """theta and out of ahmc_glm_class_probs, sized exactly, for n_cols below, at and above N (three chunks), from device and host draws;
    the outputs of ahmc_glm_categorical_get_target (arrays of one); eta_out (K planes) and loglik_out of ahmc_glm_pointwise on the model"""
    K, N = _B_C - 1, 5
    D = K * _B_PX + 1
    dll = r.lib.dll
    for dtype in (TB.F64, TB.F32):
        for n_cols in (1, 5, 15):
            th = (0.4 * np.random.default_rng(n_cols).normal(size=D * n_cols)).astype(dtype)
            for w_in in ("device", "host"):
                r.probe(lambda: bound_categorical(r, n_obs, dtype), lambda e, io: r.ok(e, dll.ahmc_glm_class_probs(e._ctx, io["ahmc_glm_class_probs.theta"], n_cols,
                                                                                                                     io["ahmc_glm_class_probs.out"])),
                        ins={"ahmc_glm_class_probs.theta": In(th, w_in)}, outs={"ahmc_glm_class_probs.out": Out(dtype, _B_C * n_obs * n_cols, where)})
        r.probe(lambda: bound_categorical(r, n_obs, dtype),
                lambda e, io: r.ok(e, dll.ahmc_glm_pointwise(e._ctx, io["ahmc_glm_pointwise.eta_out"], io["ahmc_glm_pointwise.loglik_out"])),
                outs={"ahmc_glm_pointwise.eta_out": Out(dtype, K * n_obs * N, where), "ahmc_glm_pointwise.loglik_out": Out(dtype, n_obs * N, where)})

    def call(e, io):
        r.ok(e, dll.ahmc_glm_categorical_get_target(e._ctx, C.cast(io["ahmc_glm_categorical_get_target.n_categories"], C.POINTER(C.c_int32)),
                                                    C.cast(io["ahmc_glm_categorical_get_target.block_len"], C.POINTER(C.c_int64))))
    r.probe(lambda: bound_categorical(r, n_obs, TB.F64), call, outs={"ahmc_glm_categorical_get_target.n_categories": Out(np.int32, 1, "host"),
                                                                      "ahmc_glm_categorical_get_target.block_len": Out(np.int64, 1, "host")})


_POST = ["ahmc_glm_class_probs.theta", "ahmc_glm_class_probs.out", "ahmc_glm_categorical_get_target.n_categories", "ahmc_glm_categorical_get_target.block_len",
         "ahmc_glm_pointwise.eta_out", "ahmc_glm_pointwise.loglik_out"]
BOUNDS_CASES = []
for _n in (1, 70):
    for _w in ("device", "host"):
        for _cid, _fn, _probes in ((f"glm-categorical-set-target-nobs{_n}-{_w}", c_categorical_set_target, [f"{_PRE}.{k}" for k in _SET_IN]),
                                   (f"glm-categorical-post-nobs{_n}-{_w}", c_categorical_post, _POST)):
            if _cid not in TB.CASES:
                TB.add(_cid, _fn, _probes, oracle=False, n_obs=_n, where=_w)
            BOUNDS_CASES.append(_cid)


def test_bounds_cases_cover_the_header():
    """every pointer parameter of include/ahmc_glm_categorical.h but the context is probed by a case above, and so is the enlarged
    eta_out of ahmc_glm_pointwise"""
    params = {p for p in TB.header_pointer_params() if p[0] in capi.GLM_CATEGORICAL_SIGNATURES and p[1] != "ctx"}
    probed = {tuple(k.split(".")) for cid in BOUNDS_CASES for k in TB.CASES[cid].probes}
    assert params | {("ahmc_glm_pointwise", "eta_out"), ("ahmc_glm_pointwise", "loglik_out")} == probed and len(params) == 14


@pytest.mark.gpu
@pytest.mark.parametrize("cid", BOUNDS_CASES)
def test_hip_bounds(hip, monkeypatch, cid):
    """no call of the new entry points reads or writes outside the caller's arrays (tests/arena_util.py).  There is no path of these
    calls without a GPU: the CPU checker does not implement the header."""
    if hip.backend != "hip:gfx950":
        pytest.skip("the CPU checker does not implement include/ahmc_glm_categorical.h")
    TB.run_case(hip, monkeypatch, cid)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
_STATE = {}


@pytest.fixture(scope="module")
def probe_c(hip):
    import torch

    from ahmc_amd import build as B
    from ahmc_amd.hipmod import Module

    torch.cuda.init()
    if "probe_c" not in _STATE:
        _STATE["probe_c"] = Module(B.build_probe_object(PROBE_C))
    return _STATE["probe_c"]


def device_eps(probe, probe_c, dtype):  # noqa: F811
    """ε_exp of the existing probe and ε_log, ε_inv of the new one, measured once per element type"""
    key = ("eps", np.dtype(dtype).name)
    if key not in _STATE:
        import torch

        def log_inv(s):
            s_d = TG.dev(s)
            outs = [torch.empty_like(s_d) for _ in range(2)]
            probe_c.launch("glm_categorical_probe_log_inv_" + TG._sfx(dtype), (s.size + 255) // 256, 256, s_d, *outs, np.int64(s.size))
            return tuple(TG.host(o, s.shape) for o in outs)

        eps = dict(TG.device_eps(probe, dtype))
        eps.update(log_inv_eps(log_inv, dtype))
        _STATE[key] = eps
        MARGINS[f"cat-device-functions {np.dtype(dtype).name}"] = dict(eps)
        TG._dump_margins()
    return _STATE[key]


def engine(hip, c, onehot=False, cols=None, metric=None, seed=7):
    th = c["th"] if cols is None else c["th"][:, cols]
    D, N = th.shape
    e = A.Engine(A.Hamiltonian(metric or A.UnitEuclideanMetric((D, N)), target(c, onehot)), N, dtype=c["dtype"],
                 rng=seed if isinstance(seed, A.PhiloxRNG) else A.PhiloxRNG(seed), lib=hip)
    e.set_integrator(A.Leapfrog(np.full(N, 0.02)))
    e.set_position(th)
    return e


def evaluate(e, th=None):
    if th is not None:
        e.set_position(th)
    z = e.phasepoint()
    eta, ll = e.glm_pointwise()
    W, tau = e.hglm_coefficients()
    return {"eta": eta, "loglik": ll, "lp": z.lp.value.copy(), "grad": z.lp.gradient.copy(), "W": W, "tau": tau, "prob": e.glm_class_probs()}


# ---- §1 ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_values_against_exact_references(hip, probe, probe_c, dtype):  # noqa: F811
    """every case under either tile shape and both N: the η planes of ahmc_glm_pointwise are the k-ordered fma chain on the device's own
    W (the factors' gathers as one-hot columns) bit for bit; ℓ, ℓπ, the class probabilities and all rows of g inside the bounds of the
    module docstring; the getters report the model; the two tile shapes give the same bits"""
    dtname = np.dtype(dtype).name
    eps = device_eps(probe, probe_c, dtype)
    for name, (n_obs, Px, Cn, groups, levels, _) in CASES.items():
        for N in (N_CHAINS, 48):
            c = ccase(name, N, dtname)
            e = engine(hip, c)
            fam, nc, pb = C.c_int32(), C.c_int32(), C.c_int64()
            e._call("ahmc_get_target_glm", C.byref(fam), None, None)
            e._call("ahmc_glm_categorical_get_target", C.byref(nc), C.byref(pb))
            assert (fam.value, nc.value, pb.value) == (6, Cn, c["Pb"]) and e.glm_factors() == (Px, list(levels))
            with pytest.raises(A.ArgumentError, match="no model with a sampled dispersion"):
                e.glm_dispersion()
            with pytest.raises(A.ArgumentError, match="no ordinal model"):
                e.glm_cutpoints()
            res = {}
            for which in ("small", "big"):
                with TG.tile_shape(which):
                    r = res[which] = evaluate(e, c["th"])
                    e.sync()
                assert np.isfinite(r["lp"]).all() and np.isfinite(r["grad"]).all()
                cat_check(f"{dtname} {name} N{N} {which}", c, eps, W=r["W"], tau=r["tau"], ll=r["loglik"], lp=r["lp"], g=r["grad"], eta=r["eta"], prob=r["prob"])
            for k in res["small"]:
                record_bits(f"cat-tile-shapes-{k} {dtname} {name} N{N}", res["small"][k], res["big"][k])
            e.close()
    dump_profile()


# ---- §2 ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_new_kernel_on_a_chain_list(hip, probe_c, dtype):
    """k_glm_eta_cat (both tile shapes) launched from the probe on all chains and on every third chain, reversed: the listed columns of
    the U planes, partial, the η planes and ℓ carry the bits of the full launch, the others keep their NaN fill, both tile shapes give
    the same bits; the probe's stand-alone link on the device's own η reproduces ℓ and every u plane bit for bit; η is the engine's"""
    import torch

    dtype = np.dtype(dtype)
    tch = TG.TCH[dtype]
    N = N_CHAINS
    idx = np.arange(N)[::3][::-1].copy()
    rest = np.setdiff1d(np.arange(N), idx)
    for name in ("two-blocks", "limit", "slices"):
        n_obs, Px, Cn, groups, _, _ = CASES[name]
        c = ccase(name, N, dtype.name)
        P, Pb, K, nrb = c["P"], c["Pb"], c["K"], (n_obs + 63) // 64
        key = f"{dtype.name} {name}"
        e = engine(hip, c)
        ev = evaluate(e)
        e.close()
        W = np.asfortranarray(ev["W"])
        X_d, y_d, W_d = (TG.dev(a) for a in (c["X"], c["yT"], W))
        off_d = TG.NULL if c["off"] is None else TG.dev(c["off"])

        def nan(*shape):
            return torch.full((int(np.prod(shape)),), float("nan"), dtype=W_d.dtype, device="cuda")

        out = {}
        for bn in (64, 16):
            kern = f"_ZN4ahmc13k_glm_eta_catI{tch}Li{bn}ELb0EEEvPKT_S3_S3_S3_PS1_S4_iiiilllPKiS4_S4_S4_PKNS_9GlmFacTabES6_"
            for which, lst in (("all", None), ("list", idx)):
                n = N if lst is None else lst.size
                idx_d = TG.NULL if lst is None else TG.dev(lst)
                U_d, part_d, eta_d, ll_d = nan(n_obs, N, K), nan(nrb, N), nan(n_obs, N, K), nan(n_obs, N)
                grid = (nrb * (((n + 63) // 64 + 7) // 8 * 8),) if bn == 64 else (nrb, (n + 15) // 16)
                probe_c.launch(kern, grid, 256, X_d, y_d, off_d, W_d, U_d, part_d, n_obs, int(Px), int(Pb), int(K), np.int64(P), np.int64(n), np.int64(N), idx_d, eta_d,
                               ll_d, TG.NULL, TG.NULL, TG.NULL)
                out[(bn, which)] = [TG.host(U_d, (n_obs, N * K)), TG.host(part_d, (N, nrb)).T, TG.host(eta_d, (n_obs, N * K)), TG.host(ll_d, (n_obs, N))]
                if bn == 64 and lst is None:
                    E_d, l_d, pr_d = eta_d.clone(), nan(n_obs, N), nan(Cn, n_obs, N)
                    probe_c.launch("glm_categorical_probe_link_" + TG._sfx(dtype), (n_obs * N + 255) // 256, 256, y_d, E_d, int(K), np.int64(n_obs), np.int64(N), l_d, pr_d)
                    link = [TG.host(l_d, (n_obs, N)), TG.host(E_d, (n_obs, N * K)), TG.host(pr_d, (Cn, n_obs, N))]
        names = ("U", "partial", "eta", "loglik")
        cols = lambda a, sel: a[:, np.concatenate([k * N + sel for k in range(a.shape[1] // N)])]  # noqa: E731  (the chains `sel` of every plane)
        for bn in (64, 16):
            for nm, a, b, b64 in zip(names, out[(bn, "list")], out[(bn, "all")], out[(64, "all")]):
                assert np.isfinite(b).all(), (nm, bn)
                record_bits(f"cat-chain-list-{nm}-bn{bn} {key}", cols(a, idx), cols(b, idx))
                assert np.isnan(cols(a, rest)).all(), (nm, bn)
                record_bits(f"cat-tile-shapes-{nm} {key}", b, b64)
        full = dict(zip(names, out[(64, "all")]))
        record_bits(f"cat-probe-eta-is-the-engine's {key}", full["eta"].reshape(n_obs, K, N).transpose(1, 0, 2), ev["eta"])
        record_bits(f"cat-probe-link-loglik {key}", link[0], full["loglik"])
        record_bits(f"cat-probe-link-u {key}", link[1], full["U"])
        record_bits(f"cat-probe-link-probs {key}", link[2], ev["prob"])
        record_bits(f"cat-partial-is-the-block-sum {key}", full["partial"], TO.block_sums_in(full["loglik"]))
    dump_profile()


# ---- §3 ----
def all_stats_equal(a, b, what):
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def adapting_engine(hip, c, kern, adapt=True, **kw):
    D, N = c["D"], kw.get("cols", np.arange(c["th"].shape[1])).size
    e = engine(hip, c, metric=A.DiagEuclideanMetric((D, N)), **kw)
    e.set_integrator(kern.tau.integrator)
    if adapt:
        e.adaptor_init(A.StanHMCAdaptor(A.MassMatrixAdaptor(A.DiagEuclideanMetric((D, N))), A.StepSizeAdaptor(0.8, kern.tau.integrator), 5, 5, 5))
    return e


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_chain_blocks_bulk_and_resume(hip, dtype):
    """bit for bit: engines over blocks of the chains == one engine (the evaluation and three NUTS transitions, on the two-slice
    case); the bulk run == the stepwise loop of transition + adapt; get_state after 11 of 24 → a fresh context → the rest"""
    dtname = np.dtype(dtype).name
    N = 48
    c = ccase("slices", N, dtname)
    whole = engine(hip, c, seed=A.PhiloxRNG(17))
    ev = evaluate(whole)
    whole.run(TG.nuts_kernel(N, eps=0.02), 3)
    th_w, st_w = whole.theta(), whole.stats()
    whole.close()
    assert st_w["n_steps"].sum() > 3 * N
    for lo, hi in ((0, 5), (5, 22), (22, 48)):
        cols = np.arange(lo, hi)
        e = engine(hip, c, cols=cols, seed=A.PhiloxRNG(17, chain_offset=int(lo)))
        for k, a in evaluate(e).items():
            record_bits(f"cat-blocks-{k} {dtname}", a, ev[k][..., cols])
        e.run(TG.nuts_kernel(hi - lo, eps=0.02), 3)
        record_bits(f"cat-blocks-theta {dtname}", e.theta(), th_w[:, cols])
        all_stats_equal(e.stats(), {k: v[cols] for k, v in st_w.items()}, "chain blocks")
        e.close()
    c = ccase("two-blocks", N, dtname)
    kern = TG.nuts_kernel(N, eps=0.02)
    whole = adapting_engine(hip, c, kern)
    whole.run(kern, 24, n_adapts=20)
    part = adapting_engine(hip, c, kern)
    part.run(kern, 11, n_adapts=20)
    st = part.get_state()
    part.close()
    fresh = adapting_engine(hip, c, kern, adapt=False)
    fresh.set_state(st)
    fresh.run(kern, 24, n_adapts=20, i_first=12)
    step = adapting_engine(hip, c, kern)
    for i in range(1, 25):
        step.transition(kern)
        step.adapt(i, 20)
    for e in (fresh, step):
        np.testing.assert_array_equal(whole.theta(), e.theta())
        np.testing.assert_array_equal(whole.get_stepsize(), e.get_stepsize())
        np.testing.assert_array_equal(whole.get_metric(), e.get_metric())
        e.close()
    assert not np.array_equal(whole.get_metric(), np.ones((c["D"], N)))
    whole.close()
    dump_profile()


@pytest.mark.gpu
def test_rebinding_and_the_one_hot_expansion(hip):
    """the categorical model, then a plain GLMTarget of the same D on the same context == a fresh context on the plain model, and the
    categorical model bound again == a fresh context on it; the factor encoding == the one-hot expansion of the same model (values, up
    to the sign of a zero, and three NUTS transitions)"""
    N = N_CHAINS
    c = ccase("factors", N, "float64")
    plain = TG.case(64, c["D"], N, 1, "float64")
    kern = TG.nuts_kernel(N)
    a = engine(hip, c)
    a.transition(TG.nuts_kernel(N, eps=0.02))
    a.set_target(A.GLMTarget(plain["X"], plain["y"], family=1, prior_prec=plain["p"], offset=plain["off"], scale=plain["scale"]))
    with pytest.raises(A.ArgumentError, match="no categorical model"):
        a.glm_class_probs()
    a.seed(A.PhiloxRNG(7))
    a.set_integrator(A.Leapfrog(np.full(N, 0.05)))
    a.set_position(plain["th"])
    b = TG.glm_engine(hip, plain)
    for e in (a, b):
        e.run(kern, 3)
    np.testing.assert_array_equal(a.theta(), b.theta())
    all_stats_equal(a.stats(), b.stats(), "after re-binding")
    b.close()
    a.set_target(target(c))
    a.seed(A.PhiloxRNG(7))
    a.set_integrator(A.Leapfrog(np.full(N, 0.02)))
    a.set_position(c["th"])
    b, o = engine(hip, c), engine(hip, c, onehot=True)
    assert o.glm_factors() == (c["Pb"], [])
    ra, rb, ro = evaluate(a), evaluate(b), evaluate(o)
    for k in ra:
        record_bits(f"cat-rebound-{k}", ra[k], rb[k])
        record_bits(f"cat-one-hot-{k}", rb[k], ro[k])
    for e in (a, b, o):
        e.run(TG.nuts_kernel(N, eps=0.02), 3)
    np.testing.assert_array_equal(a.theta(), b.theta())
    np.testing.assert_array_equal(o.theta(), b.theta())
    all_stats_equal(a.stats(), b.stats(), "bound again")
    all_stats_equal(o.stats(), b.stats(), "one-hot")
    for e in (a, b, o):
        e.close()
    dump_profile()


# ---- §4 ----
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PARITY) + ["dense", "wide"])
def test_against_oracle(hip, oracle, name):
    """the HIP engine on the target against the oracle on the mirror as a host kernel: static HMC, two NUTS transitions,
    find_good_stepsize, a bulk run of three (the wide context: two NUTS transitions at max_depth 5) — every discrete statistic of
    every chain, under the suite's margin rule"""
    if name == "wide":
        t, _, th0, eps = parity_inputs(*WIDE, N=8)
        o = TH.oracle_engine(oracle, t, A.UnitEuclideanMetric((t.D, 8)), 8)
        g = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((t.D, 8)), t), 8, rng=A.PhiloxRNG(8), lib=hip)
        assert g.info("wide") and t.D > 4096
        TG.parity_sequence(o, g, th0, eps, "glm-categorical wide", nuts_depth=5, full=False)
    else:
        t, minv, th0, eps = parity_inputs(*PARITY[DENSE_CASE if name == "dense" else name])
        N = th0.shape[1]
        metric = (lambda: TA.dense_metric(t.D)) if name == "dense" else (lambda: A.DiagEuclideanMetric(minv))
        o = TH.oracle_engine(oracle, t, metric(), N)
        g = A.Engine(A.Hamiltonian(metric(), t), N, rng=A.PhiloxRNG(8), lib=hip)
        TG.parity_sequence(o, g, th0, eps, f"glm-categorical {name}")
    g.close()
    o.close()


# ---- §5 ----
POSTERIOR_BETA = np.array([[0.8, -0.5, 0.3], [-0.6, 0.4, 0.9], [0.2, 1.0, -0.7]])     # row k − 1: the coefficients of class k


def posterior_model():
    n_obs, Px, Cn = 400, 3, 4
    rs = np.random.default_rng(61)
    X = rs.normal(size=(n_obs, Px))
    eta = np.column_stack([np.zeros(n_obs), X @ POSTERIOR_BETA.T])
    y = (eta + rs.gumbel(size=eta.shape)).argmax(axis=1)
    return A.GLMTarget(X, y, family="categorical_logit", n_categories=Cn, prior_scale=3.0), 0.1 * rs.normal(size=((Cn - 1) * Px, 256))


def posterior_run(lib, tgt, t, th0, n_adapt=30, n_keep=30):
    D, N = th0.shape
    e = A.Engine(A.Hamiltonian(A.DiagEuclideanMetric((D, N)), tgt), N, rng=A.PhiloxRNG(5), lib=lib)
    kern = TG.nuts_kernel(N, eps=0.1, depth=6)
    e.set_integrator(kern.tau.integrator)
    e.set_position(th0)
    e.adaptor_init(A.StanHMCAdaptor(A.MassMatrixAdaptor(A.DiagEuclideanMetric((D, N))), A.StepSizeAdaptor(0.8, kern.tau.integrator)))
    e.run(kern, n_adapt, n_adapts=n_adapt)
    draws = np.empty((n_keep, D, N))
    for i in range(n_keep):
        e.transition(kern)
        draws[i] = e.theta()
    return e, draws


def test_posterior_seed_holds_the_truth_on_the_oracle(oracle):
    """the precondition of the GPU posterior test, on the CPU oracle with the mirror as a host kernel and the same seeds: every true
    coefficient lies inside the pooled 99 % interval of its draws"""
    from test_user_targets import host_kernel

    t, th0 = posterior_model()
    e, draws = posterior_run(oracle, A.KernelTarget(t.D, host_kernel(t.logdensity), handle_kind=capi.KERNEL_HOST), t, th0)
    e.close()
    lo, hi = np.quantile(draws.transpose(1, 0, 2).reshape(t.D, -1), [0.005, 0.995], axis=1)
    truth = POSTERIOR_BETA.ravel()
    MARGINS["cat-posterior-oracle"] = {"interval_99": [lo.tolist(), hi.tolist()], "truth": truth.tolist()}
    dump_profile()
    assert np.all((lo < truth) & (truth < hi)), (lo, truth, hi)


@pytest.mark.gpu
def test_posterior_against_ask_tell(hip):
    """Simulated (400, 3, C = 4) from known coefficients; N = 256, NUTS(0.8) with StanHMCAdaptor, 30 adapting + 30 kept transitions at
    max_depth 6: the target and ExternalTarget(t.logdensity) on the same engine with the same seeds — each parameter's pooled means
    within 4 pooled MCSE (√(mcse₁² + mcse₂²)) of each other; every true coefficient inside the pooled 99 % interval of its draws"""
    t, th0 = posterior_model()
    D = t.D
    assert D == 9 and t.class_rows(2) == (3, 6)
    stats, pooled = {}, None
    for name, tgt in (("glm-categorical", t), ("external", A.ExternalTarget(D, t.logdensity))):
        e, draws = posterior_run(hip, tgt, t, th0)
        stats[name] = A.summarystats(draws)
        if name == "glm-categorical":
            pr = e.glm_class_probs(draws[-1])
            np.testing.assert_allclose(pr, t.class_probs(draws[-1]), rtol=1e-11, atol=1e-13)
            pooled = draws.transpose(1, 0, 2).reshape(D, -1)
        e.close()
    diff = np.abs(stats["glm-categorical"]["mean"] - stats["external"]["mean"])
    tol = 4 * np.sqrt(stats["glm-categorical"]["mcse"] ** 2 + stats["external"]["mcse"] ** 2)
    lo, hi = np.quantile(pooled, [0.005, 0.995], axis=1)
    truth = POSTERIOR_BETA.ravel()
    MARGINS["cat-posterior"] = {"mean_difference_over_tolerance": float((diff / tol).max()), "mean": stats["glm-categorical"]["mean"].tolist(),
                                "rhat_max": float(stats["glm-categorical"]["rhat"].max()), "interval_99": [lo.tolist(), hi.tolist()], "truth": truth.tolist()}
    dump_profile()
    print(MARGINS["cat-posterior"])
    assert np.all(diff < tol), (diff / tol)
    assert np.all((lo < truth) & (truth < hi)), (lo, truth, hi)


# ---- §6 ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_refusals(hip, dtype):
    """every refusal of the header, with the status and message class of the Python side; after each refused call the context still
    runs a transition on the model it had; the older set-target entries refuse the family and name the new header; the dispersion and
    cutpoint entry points refuse the model"""
    N = 17
    c = ccase("two-blocks", N, np.dtype(dtype).name)
    e = engine(hip, c)
    kern = TG.nuts_kernel(N, eps=0.02)
    n_obs, Px, P = 70, c["Px"], c["P"]
    X, y, p = np.asfortranarray(c["X"]), c["yT"].copy(), c["p"].copy()

    def still_runs():
        e.transition(kern)
        assert np.isfinite(e.theta()).all() and e.stats()["n_steps"].min() >= 1
        nc = C.c_int32()
        e._call("ahmc_glm_categorical_get_target", C.byref(nc), None)
        assert nc.value == 3

    def refused(exc, match, n_coef=Px, y_=y, Cn=3, n_groups=0, n_factors=0, grp=None):
        lo, hi, cen, sc = (None,) * 4 if grp is None else ((C.c_int32 * 1)(grp[0]), (C.c_int32 * 1)(grp[1]), (C.c_int32 * 1)(0), (C.c_double * 1)(1.0))
        with pytest.raises(exc, match=match):
            e._call("ahmc_glm_categorical_set_target", n_obs, n_coef, capi.as_ptr(X), capi.as_ptr(y_), None, capi.as_ptr(p), n_groups, lo, hi, cen, sc,
                    n_factors, None, None, Cn)
        still_runs()

    def poked(i, v):
        b = y.copy()
        b[i] = v
        return b

    refused(A.ArgumentError, "DomainError.*not a category", y_=poked(5, 1.5))
    refused(A.ArgumentError, "DomainError.*not a category", y_=poked(69, 3))
    refused(A.ArgumentError, "DomainError.*not a category", y_=poked(0, -1))
    refused(A.ArgumentError, "DomainError.*at least 2", Cn=1)
    refused(A.UnsupportedError, "AHMC_GLM_CATEGORICAL_MAX_CATEGORIES", Cn=17)
    refused(A.ArgumentError, "DimensionMismatch.*blocks", Cn=4)
    refused(A.ArgumentError, "DimensionMismatch", n_coef=Px + 1)
    refused(A.ArgumentError, "DimensionMismatch", n_groups=1, grp=(0, 2))          # (the neighbours' refusals come through)
    refused(A.ArgumentError, "NULL", n_factors=1)
    data = (capi.as_ptr(X), capi.as_ptr(y), None, capi.as_ptr(p))
    for call in (lambda: e._call("ahmc_set_target_glm", 6, n_obs, *data, 1.0),
                 lambda: e._call("ahmc_hglm_set_target", 6, n_obs, P, *data, 1.0, 0, None, None, None, None),
                 lambda: e._call("ahmc_glm_aux_set_target", 6, n_obs, P, *data, 0, None, None, None, None, 0.0, 1.0),
                 lambda: e._call("ahmc_glm_factor_set_target", 6, n_obs, P, *data, 1.0, 0, None, None, None, None, 0, None, None, 0, 0.0, 1.0)):
        with pytest.raises(A.ArgumentError, match="unknown family 6 at this entry point.*ahmc_glm_categorical.h|no sampled dispersion.*ahmc_glm_categorical.h"):
            call()
        still_runs()
    with pytest.raises(A.ArgumentError, match="no model with a sampled dispersion"):
        e.glm_dispersion()
    with pytest.raises(A.ArgumentError, match="no ordinal model"):
        e.glm_cutpoints()
    with pytest.raises(A.ArgumentError, match="NULL"):
        e._call("ahmc_glm_class_probs", None, 3, None)
    assert e.glm_class_probs(np.zeros((c["D"], 0))).shape == (3, n_obs, 0)
    e.close()
    # a group that straddles two blocks, on a context of the right D
    d = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((P + 1, N)), A.IsoGaussian(P + 1)), N, dtype=dtype, rng=A.PhiloxRNG(1), lib=hip)
    pz = np.zeros(P, dtype=dtype)
    with pytest.raises(A.ArgumentError, match="straddles"):
        d._call("ahmc_glm_categorical_set_target", n_obs, Px, capi.as_ptr(X), capi.as_ptr(y), None, capi.as_ptr(pz), 1, (C.c_int32 * 1)(2), (C.c_int32 * 1)(5),
                (C.c_int32 * 1)(0), (C.c_double * 1)(1.0), 0, None, None, 3)
    with pytest.raises(A.ArgumentError, match="no categorical model"):
        d.glm_class_probs()
    d.set_position(0.1 * np.random.default_rng(3).normal(size=(P + 1, N)))
    d.transition(kern)          # (the refused call left the context's own target in place)
    assert np.isfinite(d.theta()).all()
    with pytest.raises(A.ArgumentError, match="DimensionMismatch"):
        d.set_target(target(c))
    d.close()
