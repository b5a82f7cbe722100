"""The ordered-logit family of the GLM target (include/ahmc_glm_ordinal.h): y in ordered categories 0 … C − 1, P(y <= k) = σ(c_{k+1} − η),
θ ending with the C − 1 rows κ (κ_1 = c_1, κ_j = log(c_j − c_{j−1})) — k_glm_cut makes the per-chain table (c, lg, r), k_glm_eta<T, 5, BN> the
link and the row-block sums partial_c of ∂ℓ/∂a and ∂ℓ/∂b, k_hglm_finish_ord the cutpoints' rows of g and their prior; everything else of
the GLM targets runs unedited.  The arithmetic is defined by advancedhmc.jl_amd/glm.py (`ordinal_logdensity`).  Helpers come from
tests/test_glm_target.py, tests/test_glm_hier.py and tests/test_glm_aux.py.

Shapes (n_obs, P_x, C): (70, 3, 3) two row blocks, the second partial, one interior category; (1100, 5, 5) with a centred and a
non-centred group, 18 row blocks and two K slices, category 3 absent from y and category 1 absent from the first row block;
(130, 2, 2) no interior category; (130, 2, 16) the limit; (130, 2, 4) with factors (7, 1) through k_glm_eta_f.  N = 37 or 48.  κ_j of a
gap in [−1.5, 1]; κ_1 puts the cutpoints around the η range.

The bounds of the value comparison (`ord_check`; `ord_emulate` passes them on the host and fails them with each of three defects).
u = 2⁻⁵³ or 2⁻²⁴, γ_k = k·u/(1 − k·u); ε_exp, ε_log1p twice the measured worst relative errors of the device's exp and log1p
(tests/device_probe/glm.hip), ε_lg and ε_r those of lg(δ) and r(δ) = 1/expm1(δ) as k_glm_cut computes them (tests/device_probe/
glm_ordinal.hip against mpmath at 60 digits on δ ∈ [10⁻¹⁸, 700]).  References are long double on the values as stored.
  * δ̂_j = exp(κ_j)(1 + ε_exp);  ĉ_j is a sum of j terms:  E_c[j] = ε_exp·Σ_{i<=j} δ_i + γ_j·(|κ_1| + Σ_{i<=j} δ_i).
  * lg(δ): δ·|d lg/dδ| = δ·r <= 1:  E_lg = ε_lg·|lg| + ε_exp·δ·r.   r(δ): δ·|dr/dδ| = r·δ/(1 − e^{−δ}):  E_r = r·(ε_r + ε_exp·δ/(1 − e^{−δ})).
  * η̂: Δη as in test_glm_hier.hier_check (γ_P·|X|·|W| + the rounding of the offset + |X|·E_W), the factors' gathers counted as columns.
  * â = ĉ − η̂: Δa = E_c + Δη + u·|a|, and Δb alike.  softplus is 1-Lipschitz, σ is ¼-Lipschitz (test_glm_target.link_bounds):
    E_sp(x) = Δx + log1p(e^{−|x|})·(ε_exp + ε_log1p) + u·softplus,   E_σ(x) = Δx/4 + σ·(2ε_exp + 2u).
  * ℓ = (−sp(−a) − sp(b)) + lg:  E_ℓ = E_sp(a) + E_sp(b) + E_lg + 2u·(sp(−a) + sp(b) + |lg|);  u = σ(b) − σ(−a): E_u = E_σ(a) + E_σ(b) + u·|u|;
    da = σ(−a) + r: E_da = E_σ(a) + E_r + u·|da|, db alike; a side that does not exist and the constants of a non-interior category
    are exact zeros.  ℓ, a, b and δ are perturbed independently: a − b = δ is not assumed of the device's numbers.
  * S_k sums terms of mixed signs, each through at most n_add = 64 + ⌈row blocks/64⌉ + 6 additions (the block, the lane, the
    butterfly):  E_S = ΣE_t + γ_{n_add}·Σ(|t| + E_t).   T_j = Σ_{k>=j} S_k:  E_T = Σ E_S + γ_C·Σ(|S_k| + E_S).
  * g[κ_1] = fma(r_1, 1/s_1², −T_1): E_T + 3u·|r_1/s_1²| + u·|g|;  g[κ_j] = fma(−δ̂_j, T̂_j, r_j/s_g²): δ_j(1 + ε_exp)·E_T + ε_exp·δ_j·|T_j| +
    3u·|r_j/s_g²| + u·|g|.  The prior's terms of ℓπ: 4u each, and u of the running sum.
  * Σℓ, R = −Xᵀu, the coefficient rows, the groups' rows and their terms of ℓπ: test_glm_hier.hier_check's bounds with (E_ℓ, E_u) above.
SLACK = 1.01 covers products of two first-order terms.
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
import test_glm_target as TG
from ahmc_amd import _capi as capi
from ahmc_amd import glm as G
from arena_util import In, Out
from test_glm_target import probe  # noqa: F401  (a fixture of the helpers)

LD = np.longdouble
ROOT = TG.ROOT
PROBE_O = os.path.join(ROOT, "tests", "device_probe", "glm_ordinal.hip")
DTYPES = TG.DTYPES
gam, U, U_LD, SLACK = TG.gam, TG.U, TG.U_LD, TG.SLACK
record_bits, record_bound = TG.record_bits, TG.record_bound
MARGINS = TG.MARGINS
CUT_PRIOR = (0.3, 2.0, -0.2, 0.8)
GROUPS2 = ((0, 2, True, 0.8), (2, 5, False, 1.3))
# name: (n_obs, P_x, C, groups, levels)
CASES = {"two-blocks": (70, 3, 3, (), ()), "slices": (1100, 5, 5, GROUPS2, ()), "binary": (130, 2, 2, (), ()), "limit": (130, 2, 16, (), ()),
         "factors": (130, 2, 4, (), (7, 1))}
N_CHAINS = 37


# ------------------------------------------------------------------------------------------------
# the cases and their long-double references
# ------------------------------------------------------------------------------------------------
def categories(name, n_obs, Cn, rs):
    y = rs.integers(0, Cn, size=n_obs)
    if name == "slices":
        y[y == 3] = 4                      # category 3 is absent altogether
        y[:64][y[:64] == 1] = 2            # category 1 is absent from the first row block
        assert not (y == 3).any() and not (y[:64] == 1).any() and (y[64:] == 1).any()
    assert all((y == k).any() for k in range(Cn) if not (name == "slices" and k == 3))
    return y


@functools.lru_cache(maxsize=None)
def ocase(name, N, dtname):
    """operands of one case in the element type and its long-double references, computed once"""
    n_obs, Px, Cn, groups, levels = CASES[name]
    dtype = np.dtype(dtname)
    rs = np.random.default_rng([n_obs, Px, Cn, len(groups), len(levels), N, dtype.itemsize])
    X = np.asfortranarray(rs.normal(size=(n_obs, Px)) / np.sqrt(Px), dtype=dtype)
    factors = tuple(A.Factor(rs.integers(0, L, size=n_obs), L) for L in levels)
    P = Px + sum(levels)
    Gn, Cm1 = len(groups), Cn - 1
    gaps = rs.uniform(-1.5, 1.0, size=(Cm1 - 1, N))
    k1 = -0.5 * np.exp(gaps).sum(axis=0) + 0.3 * rs.normal(size=N)          # (the cutpoints straddle η, which is centred at 0)
    th = np.asfortranarray(np.concatenate([0.5 * rs.normal(size=(P, N)), 0.4 * rs.normal(size=(Gn, N)), k1.reshape(1, N), gaps]), dtype=dtype)
    y = categories(name, n_obs, Cn, rs)
    p = (2 * rs.random(P)).astype(dtype)
    p[::3] = 0
    for lo, hi, _, _ in groups:
        p[lo:hi] = 0
    off = (0.3 * rs.normal(size=n_obs)).astype(dtype)
    Xe = np.asfortranarray(G.expand_factors(X.astype(np.float64), factors), dtype=dtype)   # (0 and 1 are exact in either type)
    Xet = np.asfortranarray(Xe.T)
    ia2 = np.array([dtype.type(1.0 / (a * a)) for _, _, _, a in groups], dtype=dtype)
    D, PG = P + Gn + Cm1, P + Gn
    # ---- the references ----
    t = th.astype(LD)
    s = t[P:PG]
    tau = np.exp(s)
    W = t[:P].copy()
    for k, (lo, hi, cen, _) in enumerate(groups):
        if not cen:
            W[lo:hi] = tau[k] * t[lo:hi]
    E, S_eta = TG.exact(Xe, W)
    eta = E + off.astype(LD).reshape(-1, 1)
    cut, lg, r, delta = G.cut_constants(t[PG:])
    assert cut.dtype == LD
    ll, uu, da, db = G.ordinal_link(y, eta, cut, lg, r)
    assert ll.dtype == LD
    Gx, Sg = TG.exact(Xet, uu)
    R = -Gx
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
    lp1 = lp0 + sum(x["h"] + x["b"] for x in grp)
    yc = y.reshape(-1, 1)
    terms = np.stack([np.where(yc == k - 1, da, np.where(yc == k, db, LD(0))) for k in range(1, Cn)])        # (C−1, n_obs, N)
    Ssum = terms.sum(axis=1)
    T = np.cumsum(Ssum[::-1], axis=0)[::-1]
    loc = np.array([CUT_PRIOR[0]] + [CUT_PRIOR[2]] * (Cm1 - 1), dtype=LD).reshape(-1, 1)
    ia = np.array([dtype.type(1.0 / CUT_PRIOR[1] ** 2)] + [dtype.type(1.0 / CUT_PRIOR[3] ** 2)] * (Cm1 - 1)).astype(LD).reshape(-1, 1)
    rk = t[PG:] - np.array([dtype.type(v) for v in loc[:, 0]]).astype(LD).reshape(-1, 1)
    pterm = -rk * rk * ia / 2
    g[PG:] = rk * ia - delta * T
    lp = lp1 + pterm.sum(axis=0)
    return {"name": name, "X": X, "Xe": Xe, "Xet": Xet, "y": y, "yT": y.astype(dtype), "off": off, "p": p, "th": th, "dtype": dtype, "groups": groups, "factors": factors,
            "Px": Px, "P": P, "PG": PG, "D": D, "C": Cn, "ia2": ia2, "tau": tau, "W": W, "S_eta": S_eta, "eta": eta, "cut": cut, "lg": lg, "r": r, "delta": delta,
            "ll": ll, "u": uu, "da": da, "db": db, "Sg": Sg, "R": R, "prior": prior, "lp0": lp0, "lp1": lp1, "grp": grp, "g": g, "lp": lp, "terms": terms,
            "S": Ssum, "T": T, "rk": rk, "cia": ia, "pterm": pterm}


def target(c, onehot=False):
    """the case's model; `onehot`: the factors written as one-hot columns of X"""
    kw = dict(family="ordered_logit", n_categories=c["C"], cut_prior=CUT_PRIOR, prior_prec=c["p"], offset=c["off"])
    X, fk = (c["Xe"], {}) if onehot or not c["factors"] else (c["X"], {"factors": c["factors"]})
    return A.HierGLMTarget(X, c["y"], c["groups"], **kw, **fk) if c["groups"] else A.GLMTarget(X, c["y"], **kw, **fk)


def link_bounds(c, eps, eta_hat, d_eta):
    """(E_ℓ, E_u, E_da, E_db, E_c) of the module docstring, element by element"""
    u = U[c["dtype"]]
    ee, el, elg, er = (LD(eps[k]) for k in ("exp", "log1p", "lg", "r"))
    Cm1 = c["C"] - 1
    d = c["delta"].copy()
    d[0] = 0
    dsum = np.cumsum(d, axis=0)
    k1 = np.abs(c["th"][c["PG"]].astype(LD))
    Ec = ee * dsum + np.array([gam(j + 1, u) for j in range(Cm1)]).reshape(-1, 1) * (k1 + dsum)
    dd = c["delta"]
    Elg = elg * np.abs(c["lg"]) + ee * dd * c["r"]
    Er = c["r"] * (er + ee * dd / -np.expm1(-dd))
    Elg[0] = Er[0] = 0
    y = c["y"]
    ia, ib = np.minimum(y, Cm1 - 1), np.maximum(y - 1, 0)
    ha, hb = (y < Cm1).reshape(-1, 1), (y > 0).reshape(-1, 1)
    inn = ha & hb
    eh = eta_hat.astype(LD)
    z = LD(0)

    def side(cc, Ecc, sign):
        x = cc - eh                                            # a or b
        assert np.abs(x).max() <= TG.ETA_MAX
        Dx = Ecc + d_eta + u * np.abs(x)
        e = np.exp(-np.abs(x))
        l1p = np.log1p(e)
        sp = np.maximum(sign * x, 0) + l1p                     # softplus(−a) (sign −1) or softplus(b)
        sg = np.where(sign * x >= 0, 1 / (1 + e), e / (1 + e))
        return Dx + l1p * (ee + el) + u * sp, Dx / 4 + sg * (2 * ee + 2 * u), sp

    Espa, Esna, spa = side(c["cut"][ia], Ec[ia], -1)
    Espb, Esb, spb = side(c["cut"][ib], Ec[ib], 1)
    Espa, Esna, spa = np.where(ha, Espa, z), np.where(ha, Esna, z), np.where(ha, spa, z)
    Espb, Esb, spb = np.where(hb, Espb, z), np.where(hb, Esb, z), np.where(hb, spb, z)
    Elg_e, Er_e, lg_e = np.where(inn, Elg[ia], z), np.where(inn, Er[ia], z), np.where(inn, np.abs(c["lg"][ia]), z)
    El = Espa + Espb + Elg_e + 2 * u * (spa + spb + lg_e)
    Eu = Esna + Esb + u * np.abs(c["u"])
    Eda = np.where(ha, Esna + Er_e + u * np.abs(c["da"]), z)
    Edb = np.where(hb, Esb + Er_e + u * np.abs(c["db"]), z)
    ld = 8 * U_LD * (np.abs(c["ll"]) + np.abs(c["da"]) + np.abs(c["db"]) + 1)
    return SLACK * El + ld, SLACK * Eu + ld, SLACK * Eda + ld, SLACK * Edb + ld, SLACK * Ec


def ord_check(key, c, eps, W=None, tau=None, cut=None, ll=None, lp=None, g=None, eta=None):
    """the assertions of the value test on whatever results are given (the device's, or a host emulation's); `W` (the results' own
    effective coefficients, which fix η̂) is needed for everything but tau"""
    dtype, P, PG, groups, Cn = c["dtype"], c["P"], c["PG"], c["groups"], c["C"]
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
        record_bound(f"ord-tau {key}", np.abs(tau.astype(LD) - c["tau"]), SLACK * ee * c["tau"] + ld * c["tau"])
    if W is None:
        return
    record_bound(f"ord-W {key}", np.abs(W.astype(LD) - c["W"]), Ew + ld * absW)
    absX = np.abs(c["Xe"]).astype(LD)
    eta_hat = TG.chain(c["Xe"], W) + c["off"].reshape(-1, 1)
    if eta is not None:
        record_bits(f"ord-eta {key}", eta, eta_hat)
    d_eta = (gam(P, u) + gam(P + 1, U_LD)) * c["S_eta"] * SLACK + (u + U_LD) * np.abs(eta_hat.astype(LD)) + absX @ Ew
    El, Eu, Eda, Edb, Ec = link_bounds(c, eps, eta_hat, d_eta)
    if cut is not None:
        record_bound(f"ord-cutpoints {key}", np.abs(cut.astype(LD) - c["cut"]), Ec + ld * (np.abs(c["cut"]) + 1))
    if ll is not None:
        record_bound(f"ord-loglik {key}", np.abs(ll.astype(LD) - c["ll"]), El)
    if lp is None and g is None:
        return
    XE = absX.T @ Eu
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
    # the cutpoints' rows and their prior
    yc = c["y"].reshape(-1, 1)
    Et = np.stack([np.where(yc == k - 1, Eda, np.where(yc == k, Edb, LD(0))) for k in range(1, Cn)])
    n_add = 64 + ((n_obs + 63) // 64 + 63) // 64 + 6
    ES = Et.sum(axis=1) + (gam(n_add, u) + gam(n_obs, U_LD)) * (np.abs(c["terms"]) + Et).sum(axis=1)
    ET = np.cumsum(ES[::-1], axis=0)[::-1] + gam(Cn, u) * np.cumsum((np.abs(c["S"]) + ES)[::-1], axis=0)[::-1]
    pr = np.abs(c["rk"] * c["cia"])
    dd = c["delta"]
    Eg[PG:] = dd * (1 + ee) * ET + ee * dd * np.abs(c["T"]) + 3 * u * pr
    Eg[PG] = ET[0] + 3 * u * pr[0]
    for j in range(Cn - 1):
        tj = np.abs(c["pterm"][j])
        run = run + tj
        Elp = Elp + 4 * u * tj + u * run
    if lp is not None:
        record_bound(f"ord-lp {key}", np.abs(lp.astype(LD) - c["lp"]), SLACK * Elp + ld * (np.abs(c["ll"]).sum(axis=0) + run))
    if g is not None:
        mag = np.abs(c["g"]) + 1
        mag[:P] += c["Sg"] * (1 + (np.abs(c["tau"]).max(axis=0) if len(groups) else 0))
        mag[PG:] += dd * np.abs(c["terms"]).sum(axis=1)[::-1].cumsum(axis=0)[::-1]
        err, bound = np.abs(g.astype(LD) - c["g"]), SLACK * (Eg + u * np.abs(g.astype(LD))) + ld * mag
        record_bound(f"ord-grad {key}", err[:PG], bound[:PG])
        record_bound(f"ord-cutgrad {key}", err[PG:], bound[PG:])


def block_sums_in(a):
    """Σ over each block of 64 rows, ascending from +0, in a's own type: (n_blocks, N)"""
    n = a.shape[0]
    nb = (n + 63) // 64
    pad = np.zeros((nb * 64,) + a.shape[1:], dtype=a.dtype)
    pad[:n] = a
    return np.add.accumulate(pad.reshape((nb, 64) + a.shape[1:]), axis=1)[:, -1]


def lane_tree(part):
    """Σ over the row blocks as the device sums them: lane l takes blocks l, l + 64, … ascending, then a six-stage pairwise tree"""
    lanes = np.zeros((64,) + part.shape[1:], dtype=part.dtype)
    for i in range(0, part.shape[0], 64):
        n = min(64, part.shape[0] - i)
        lanes[:n] = lanes[:n] + part[i:i + n]
    while lanes.shape[0] > 1:
        lanes = lanes[0::2] + lanes[1::2]
    return lanes[0]


def partial_c_of(y, da, db, Cn, drop_last=False):
    """partial_c (C−1, row blocks, N) by the contract's ordered additions of the given da / db, in their own type"""
    yc = y.reshape(-1, 1)
    z = da.dtype.type(0)
    out = np.stack([block_sums_in(np.where(yc == k - 1, da, np.where(yc == k, db, z))) for k in range(1, Cn)])
    if drop_last:
        out[:, -1] = 0
    return out


def ord_emulate(c, defect=None):
    """the device's arithmetic on the host in the element type and in the contract's order, numpy's functions for the device's.
    `defect`: "drop_r" leaves r out of db, "prefix" takes T as a prefix sum, "drop_block" loses the last row block of partial_c."""
    dtype, dt, P, PG, groups, Cn = c["dtype"], c["dtype"].type, c["P"], c["PG"], c["groups"], c["C"]
    th = c["th"]
    b, s, kap = th[:P], th[P:PG], th[PG:]
    tau = np.exp(s)
    W = b.copy()
    for k, (lo, hi, cen, _) in enumerate(groups):
        if not cen:
            W[lo:hi] = tau[k] * b[lo:hi]
    eta_hat = TG.chain(c["Xe"], W) + c["off"].reshape(-1, 1)
    cut, lg, r, delta = G.cut_constants(kap)
    ll, uu, da, db = G.ordinal_link(c["y"], eta_hat, cut, lg, r)
    assert all(a.dtype == dtype for a in (cut, lg, r, ll, uu, da, db))
    if defect == "drop_r":
        inn = ((c["y"] > 0) & (c["y"] < Cn - 1)).reshape(-1, 1)
        db = np.where(inn, db + r[np.minimum(c["y"], Cn - 2)], db).astype(dtype)
    R = -TG.grad_model(c["Xet"], uu, np.zeros(P, dtype=dtype), W) * dt(-1)            # (fma(0, w, −Σ) = −Xᵀu)
    lsum = lane_tree(block_sums_in(ll))
    p = c["p"].reshape(-1, 1)

    def fma(x, y, z):
        return TG.host_fma(*(np.asarray(v, dtype=dtype) for v in (x, y, z)))

    lp = lsum - ((p * b) * b).sum(axis=0, dtype=dtype) / dt(2)
    g = np.empty_like(th)
    g[:P] = TG.host_fma(p, b, R)
    for k, (lo, hi, cen, _) in enumerate(groups):           # (test_glm_hier.hier_emulate)
        m, a2, sk = dt(hi - lo), c["ia2"][k], s[k]
        S, T = TH.lane_sum(b[lo:hi], b[lo:hi]), TH.lane_sum(R[lo:hi], W[lo:hi])
        e2 = np.exp(dt(2) * sk)
        h, hp = fma(dt(-0.5) * e2, a2, sk), fma(-e2, a2, dt(1))
        if cen:
            q = np.exp(dt(-2) * sk)
            bk = fma(-m, sk, (dt(-0.5) * q) * S)
            g[lo:hi] = TG.host_fma(q.reshape(1, -1), b[lo:hi], R[lo:hi])
            g[P + k] = fma(-q, S, m) - hp
        else:
            bk = dt(-0.5) * S
            g[lo:hi] = TG.host_fma(tau[k].reshape(1, -1), R[lo:hi], b[lo:hi])
            g[P + k] = T - hp
        lp = lp + (h + bk)
    pc = partial_c_of(c["y"], da, db, Cn, drop_last=defect == "drop_block")
    Sk = [lane_tree(pc[k]) for k in range(Cn - 1)]
    loc1, ia1, locg, iag = dt(CUT_PRIOR[0]), dt(1.0 / CUT_PRIOR[1] ** 2), dt(CUT_PRIOR[2]), dt(1.0 / CUT_PRIOR[3] ** 2)
    for j in range(Cn - 1):
        rj = kap[j] - (loc1 if j == 0 else locg)
        lp = fma((dt(-0.5) * (ia1 if j == 0 else iag)) * rj, rj, lp)
    T = None
    order = range(Cn - 1) if defect == "prefix" else range(Cn - 2, -1, -1)
    Ts = {}
    for j in order:
        T = Sk[j] if T is None else Sk[j] + T
        Ts[j] = T
    for j in range(Cn - 1):
        g[PG + j] = fma(kap[j] - loc1, ia1, -Ts[j]) if j == 0 else fma(-np.exp(kap[j]), Ts[j], (kap[j] - locg) * iag)
    assert lp.dtype == dtype and g.dtype == dtype
    return {"W": W, "tau": tau, "cut": cut, "eta": eta_hat, "ll": ll, "lp": lp, "g": g, "pc": pc, "da": da, "db": db}


def host_eps(dtype):
    """numpy's functions in the place of the device's: ε_exp, ε_log1p by test_glm_target.function_eps, ε_lg and ε_r by `gap_eps`"""
    dtype = np.dtype(dtype)
    eps = dict(TG.function_eps(np.exp, np.log1p, dtype))

    def gap(d):
        _, lg, r, _ = G.cut_constants(np.stack([np.zeros_like(d), np.log(d)]))      # (δ = exp(log δ): the argument is re-rounded below)
        with np.errstate(over="ignore", under="ignore", divide="ignore"):
            dd = np.exp(np.log(d))
            return np.expm1(dd), lg[1], r[1], dd
    eps.update(gap_eps(gap, dtype))
    return eps


def gap_grid(dtype):
    top = 700.0 if np.dtype(dtype) == np.float64 else 85.0
    rs = np.random.default_rng(3)
    return np.concatenate([np.logspace(-18, np.log10(top), 4001), rs.uniform(np.exp(-1.5), np.exp(1.0), 4000), np.log(2.0) * (1 + np.linspace(-1e-3, 1e-3, 401))]).astype(dtype)


def gap_eps(fn, dtype):
    """twice the worst relative errors of expm1(δ), lg(δ) and r(δ) = 1/expm1(δ) as `fn` computes them on `gap_grid`, against mpmath at 60
    digits (values below the element type's normal range are left out: there the error is absolute, below the smallest normal)"""
    import mpmath as mp

    dtype = np.dtype(dtype)
    d = gap_grid(dtype)
    res = fn(d)
    em1, lg, r = (np.asarray(v) for v in res[:3])
    d_used = np.asarray(res[3]) if len(res) > 3 else d
    tiny = np.finfo(dtype).tiny
    worst = {"expm1": 0.0, "lg": 0.0, "r": 0.0}
    with mp.workdps(60):
        for i in range(d.size):
            x = mp.mpf(float(d_used[i]))
            refs = {"expm1": mp.expm1(x), "lg": mp.log(-mp.expm1(-x)) if x < 1 else mp.log1p(-mp.exp(-x)), "r": 1 / mp.expm1(x)}     # (either form at 60 digits)
            for k, got in (("expm1", em1[i]), ("lg", lg[i]), ("r", r[i])):
                ref = refs[k]
                if abs(ref) < 4 * tiny or abs(ref) > np.finfo(dtype).max / 4:
                    continue
                worst[k] = max(worst[k], float(abs((mp.mpf(float(got)) - ref) / ref)))
    u = float(U[dtype])
    out = {k: 2 * v for k, v in worst.items()}
    out.update({f"{k}_worst_u": v / u for k, v in worst.items()})
    assert all(out[f"{k}_worst_u"] < 16 for k in worst), out      # (a function this far off is a finding of its own, not a margin)
    return out


# ------------------------------------------------------------------------------------------------
# CPU 1: the mirror against exact references
# ------------------------------------------------------------------------------------------------
def direct_ll_mp(y, eta, cuts, dps=60):
    """log(σ(c_{y+1} − η) − σ(c_y − η)) by mpmath"""
    import mpmath as mp

    with mp.workdps(dps):
        sg = lambda x: 1 / (1 + mp.exp(-x))  # noqa: E731
        eta = mp.mpf(float(eta))
        hi = mp.mpf(1) if y == len(cuts) else sg(mp.mpf(float(cuts[y])) - eta)
        lo = mp.mpf(0) if y == 0 else sg(mp.mpf(float(cuts[y - 1])) - eta)
        return mp.log(hi - lo)


def test_mirror_loglik_against_the_direct_definition():
    """ℓ of the mirror against log(σ(c_{y+1} − η) − σ(c_y − η)) at 60 digits (the cutpoints as the mirror made them, so that only the
    link is compared); ordinal_probs sums to 1 and equals exp(ℓ) at the observed category"""
    import mpmath as mp

    rs = np.random.default_rng(11)
    worst = 0.0
    for Cn in (2, 3, 4, 6):
        kap = np.concatenate([rs.normal(size=(1, 5)), rs.uniform(-1.5, 1.0, size=(Cn - 2, 5))])
        cut, lg, r, _ = G.cut_constants(kap)
        eta = 3 * rs.normal(size=(40, 5))
        y = rs.integers(0, Cn, size=40)
        ll = G.ordinal_link(y, eta, cut, lg, r)[0]
        pr = G.ordinal_probs(eta, cut)
        assert pr.shape == (Cn, 40, 5)
        np.testing.assert_allclose(pr.sum(axis=0), 1.0, rtol=0, atol=8 * 2.0 ** -52)
        np.testing.assert_allclose(pr[y, np.arange(40)], np.exp(ll), rtol=64 * 2.0 ** -52)
        for i in range(40):
            for j in range(5):
                # lg is made from δ = exp(κ) while c_j − c_{j−1} is δ rounded into the sum: compare at the gap the cutpoints really have
                ref = direct_ll_mp(y[i], eta[i, j], cut[:, j])
                gap_err = 0.0
                if 0 < y[i] < Cn - 1:
                    with mp.workdps(60):
                        d_sum, d_exp = mp.mpf(float(cut[y[i], j])) - mp.mpf(float(cut[y[i] - 1, j])), mp.exp(mp.mpf(float(kap[y[i], j])))
                        gap_err = float(abs(d_sum - d_exp) / d_exp * (d_exp / mp.expm1(d_exp)))
                err = float(abs(mp.mpf(float(ll[i, j])) - ref))
                bound = 16 * 2.0 ** -53 * (abs(float(ref)) + 1) + 2 * gap_err
                worst = max(worst, err / bound)
                assert err <= bound, (Cn, i, j, err, bound)
    MARGINS["ord-mirror-vs-mpmath"] = {"error_over_bound": worst}
    dump_profile()


def lp_mp(X, y, th, Cn, groups, off, p, cut_prior, dps=40):
    """ℓπ of one chain by the direct definition in mpmath (groups as in glm.py)"""
    import mpmath as mp

    with mp.workdps(dps):
        P = X.shape[1]
        Gn = len(groups)
        t = [v if isinstance(v, mp.mpf) else mp.mpf(float(v)) for v in th]      # (a perturbed θ keeps its 40 digits)
        w = t[:P]
        lp = mp.mpf(0)
        member = set()
        for k, (lo, hi, cen, Asc) in enumerate(groups):
            s = t[P + k]
            tau = mp.exp(s)
            S = sum(t[d] ** 2 for d in range(lo, hi))
            lp += s - mp.exp(2 * s) / (2 * mp.mpf(Asc) ** 2)
            if cen:
                lp += -(hi - lo) * s - mp.exp(-2 * s) * S / 2
            else:
                lp += -S / 2
                for d in range(lo, hi):
                    w[d] = tau * t[d]
            member |= set(range(lo, hi))
        for d in range(P):
            if d not in member:
                lp -= mp.mpf(float(p[d])) * t[d] ** 2 / 2
        kap = t[P + Gn:]
        cuts = [kap[0]]
        for j in range(1, Cn - 1):
            cuts.append(cuts[-1] + mp.exp(kap[j]))
        sg = lambda x: 1 / (1 + mp.exp(-x))  # noqa: E731
        for i in range(X.shape[0]):
            eta = sum(mp.mpf(float(X[i, d])) * w[d] for d in range(P)) + mp.mpf(float(off[i]))
            hi_ = mp.mpf(1) if y[i] == Cn - 1 else sg(cuts[y[i]] - eta)
            lo_ = mp.mpf(0) if y[i] == 0 else sg(cuts[y[i] - 1] - eta)
            lp += mp.log(hi_ - lo_)
        lp -= ((kap[0] - cut_prior[0]) / cut_prior[1]) ** 2 / 2
        for j in range(1, Cn - 1):
            lp -= ((kap[j] - cut_prior[2]) / cut_prior[3]) ** 2 / 2
        return lp


@pytest.mark.parametrize("groups", [(), ((0, 2, True, 0.9), (2, 4, False, 1.4))], ids=["no-groups", "groups"])
@pytest.mark.parametrize("Cn", [2, 3, 5])
def test_mirror_gradient_against_central_differences(Cn, groups):
    """every row of the mirror's gradient — coefficients, log-scales, cutpoints — against central differences of ℓπ by the direct
    definition in mpmath at 40 digits (h = 1e-10: the truncation error h²·|f‴|/6 and the rounding 1e-40/h are both far below the
    tolerance), and ℓπ itself"""
    import mpmath as mp

    rs = np.random.default_rng([Cn, len(groups)])
    n_obs, P = 23, 4
    X = rs.normal(size=(n_obs, P)) / 2
    y = rs.integers(0, Cn, size=n_obs)
    off = 0.3 * rs.normal(size=n_obs)
    p = 2 * rs.random(P)
    for lo, hi, _, _ in groups:
        p[lo:hi] = 0
    D = P + len(groups) + Cn - 1
    th = np.concatenate([rs.normal(size=P), 0.4 * rs.normal(size=len(groups)), rs.normal(size=1), rs.uniform(-1.5, 1.0, size=Cn - 2)])
    lp, gr = G.ordinal_logdensity(X, y, th.reshape(-1, 1), Cn, groups, off, p, CUT_PRIOR)
    assert gr.shape == (D, 1)
    ref = lp_mp(X, y, th, Cn, groups, off, p, CUT_PRIOR)
    assert abs(float(mp.mpf(float(lp[0])) - ref)) <= 1e-12 * (abs(float(ref)) + 1)
    h = mp.mpf("1e-10")
    for d in range(D):
        with mp.workdps(40):
            tp, tm = [mp.mpf(float(v)) for v in th], [mp.mpf(float(v)) for v in th]
            tp[d] += h
            tm[d] -= h
            fd = (lp_mp(X, y, tp, Cn, groups, off, p, CUT_PRIOR) - lp_mp(X, y, tm, Cn, groups, off, p, CUT_PRIOR)) / (2 * h)
        assert abs(float(mp.mpf(float(gr[d, 0])) - fd)) <= 1e-11 * (abs(float(fd)) + 1), (d, float(fd), gr[d, 0])


def test_mirror_extremes():
    """η = ±800; a gap of 4·10⁻¹⁸ (κ_j = −40: lg ≈ −40, r ≈ 2·10¹⁷, finite); κ_j = 6.5 and 6.7 (e^{−δ} underflows: lg = 0, r = 0); κ_j = 800
    (non-finite, sanitised to −Inf)"""
    X = np.array([[800.0], [-800.0], [0.0], [1.0], [800.0], [-800.0]])
    y = np.array([0, 2, 1, 1, 2, 0])
    th = np.array([[1.0], [0.0], [0.0]])
    lp, g = G.ordinal_logdensity(X, y, th, 3)
    assert np.isfinite(lp).all() and np.isfinite(g).all()
    eta, ll = G.ordinal_pointwise(X, y, th, 3)
    np.testing.assert_allclose(ll[[0, 1], 0], [-800.0, -801.0], rtol=1e-15)        # (P(y = 0) = σ(0 − 800), P(y = 2) = σ(−800 − 1))
    np.testing.assert_allclose(ll[[4, 5], 0], [0.0, 0.0], atol=1e-300)
    c, lg, r, d = G.cut_constants(np.array([[0.0], [-40.0]]))
    assert np.isfinite(lg).all() and np.isfinite(r).all() and abs(lg[1, 0] + 40.0) < 1e-12 and abs(r[1, 0] * np.exp(-40.0) - 1) < 1e-12
    lp, g = G.ordinal_logdensity(X[2:4], y[2:4], np.array([[0.3], [0.0], [-40.0]]), 3)
    assert np.isfinite(lp).all() and np.isfinite(g).all() and lp[0] < -80                # (two observations inside a gap of 4e-18)
    # (δ = e^6.5 = 665: e^{−δ} = 1.4e−289 underflows in Float32 and is still a number in Float64, where it is gone at κ_j = 6.7, δ = 812)
    c, lg, r, d = G.cut_constants(np.array([[0.0], [6.5]]))
    assert -1e-280 < lg[1, 0] <= 0.0 and 0.0 <= r[1, 0] < 1e-280
    c, lg, r, d = G.cut_constants(np.array([[0.0], [6.5]], dtype=np.float32))
    assert lg.dtype == np.float32 and lg[1, 0] == 0.0 and r[1, 0] == 0.0
    c, lg, r, d = G.cut_constants(np.array([[0.0], [6.7]]))
    assert lg[1, 0] == 0.0 and r[1, 0] == 0.0
    for k2 in (6.5, 6.7):
        lp, g = G.ordinal_logdensity(X, y, np.array([[0.01], [0.0], [k2]]), 3)
        assert np.isfinite(lp).all() and np.isfinite(g).all()
    lp, g = G.ordinal_logdensity(X, y, np.array([[0.01], [0.0], [800.0]]), 3)
    assert not np.isfinite(lp[0]) and G.sanitize(lp)[0] == -np.inf
    np.testing.assert_array_equal(G.cutpoints(np.array([0.5, 0.0, np.log(2.0)])), [0.5, 1.5, 3.5])


# ------------------------------------------------------------------------------------------------
# CPU 2: C = 2 is Bernoulli
# ------------------------------------------------------------------------------------------------
def test_two_categories_is_the_bernoulli_mirror():
    """the ordinal mirror on (X, y) against the bernoulli_logit mirror on X′ = [X, −1], θ′ = [θ; c_1] with prior precision 1/scale_1² on
    the last coefficient and loc_1 = 0: P(y = 1) = 1 − σ(c_1 − η) = σ(η − c_1).  Both are float64 evaluations: η′ differs from η − c_1 by
    at most γ_{P+2}·(|X|·|θ| + |c_1| + |offset|) =: Δ; ℓ and u by the link's Lipschitz constants (1, ¼) at Δ plus 8u·(|ℓ| + 1) of their own
    roundings, once per side; the sums by γ_{n_obs}·Σ|terms|."""
    rs = np.random.default_rng(5)
    n_obs, P, N = 130, 3, 4
    X = rs.normal(size=(n_obs, P))
    y = rs.integers(0, 2, size=n_obs)
    off = 0.3 * rs.normal(size=n_obs)
    p = np.array([0.5, 0.0, 2.0])
    sc1 = 1.7
    th = np.concatenate([rs.normal(size=(P, N)), 0.5 * rs.normal(size=(1, N))])
    lp_o, g_o = G.ordinal_logdensity(X, y, th, 2, (), off, p, (0.0, sc1, 0.0, 1.0))
    Xb = np.column_stack([X, -np.ones(n_obs)])
    lp_b, g_b = G.logdensity("bernoulli_logit", Xb, y.astype(float), th, off, np.append(p, 1 / sc1 ** 2))
    u = 2.0 ** -53
    S = np.abs(Xb) @ np.abs(th) + np.abs(off).reshape(-1, 1)
    d = 2 * (P + 2) * u * S
    _, ll = G.pointwise("bernoulli_logit", Xb, y.astype(float), th, off)
    El = 2 * (d + 8 * u * (np.abs(ll) + 1))
    Eu = 2 * (d / 4 + 8 * u)
    prior = 0.5 * (np.append(p, 1 / sc1 ** 2).reshape(-1, 1) * th * th).sum(axis=0)
    b_lp = El.sum(axis=0) + 2 * n_obs * u * (np.abs(ll) + El).sum(axis=0) + 16 * u * (prior + np.abs(lp_b))
    assert np.all(np.abs(lp_o - lp_b) <= b_lp), (np.abs(lp_o - lp_b) / b_lp).max()
    b_g = np.abs(Xb).T @ Eu + 2 * (n_obs + 2) * u * (np.abs(Xb).T @ np.ones_like(Eu)) + 16 * u * (np.abs(g_b) + 1)
    assert np.all(np.abs(g_o - g_b) <= b_g), (np.abs(g_o - g_b) / b_g).max()
    MARGINS["ord-binary-is-bernoulli"] = {"error_over_bound": float(max((np.abs(lp_o - lp_b) / b_lp).max(), (np.abs(g_o - g_b) / b_g).max()))}


# ------------------------------------------------------------------------------------------------
# CPU 3: header == binding table == Julia ccalls == exported symbols; the kernels
# ------------------------------------------------------------------------------------------------
def header_prototypes():
    src = open(os.path.join(ROOT, "include", "ahmc_glm_ordinal.h"), encoding="utf-8").read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(int32_t)\s+(ahmc_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        params = " ".join(m.group(3).split())
        protos[m.group(2)] = [] if params in ("", "void") else [p.strip() for p in params.split(",")]
    return protos, src


def test_header_and_bindings_agree():
    protos, src = header_prototypes()
    assert set(protos) == set(capi.GLM_ORDINAL_SIGNATURES) == {"ahmc_glm_ordinal_version", "ahmc_glm_ordinal_set_target", "ahmc_glm_ordinal_get_target",
                                                              "ahmc_glm_cutpoints"}
    older = set(capi.GLM_SIGNATURES) | set(capi.HGLM_SIGNATURES) | set(capi.GLM_AUX_SIGNATURES) | set(capi.GLM_FACTOR_SIGNATURES) | set(capi.SIGNATURES)
    assert not set(capi.GLM_ORDINAL_SIGNATURES) & older
    ct = {"int64_t*": C.POINTER(C.c_int64), "int32_t*": C.POINTER(C.c_int32), "double*": C.POINTER(C.c_double), "int64_t": C.c_int64,
          "int32_t": C.c_int32, "double": C.c_double}
    for name, params in protos.items():
        res, args = capi.GLM_ORDINAL_SIGNATURES[name]
        assert res is C.c_int32 and len(args) == len(params), name
        for p, a in zip(params, args):
            typ = p.rsplit(" ", 1)[0].replace("const ", "").replace(" ", "")
            if typ in ("void*", "ahmc_ctx*"):
                assert a is C.c_void_p, (name, p)
            else:
                assert a is ct[typ], (name, p)
    # ahmc_glm_factor_set_target's arguments without family, scale and the dispersion, then the categories and their prior
    fac = [p.split()[-1] for p in __import__("test_glm_factor").header_prototypes()[0]["ahmc_glm_factor_set_target"]]
    want = [a for a in fac if a not in ("family", "scale", "has_aux", "aux_loc", "aux_scale")] + ["n_categories", "cut_prior"]
    assert [p.split()[-1] for p in protos["ahmc_glm_ordinal_set_target"]] == want
    assert [p.split()[-1] for p in protos["ahmc_glm_cutpoints"]] == ["ctx", "theta", "n_cols", "out"]
    assert re.search(r"#define AHMC_GLM_ORDINAL_VERSION (\d+)", src).group(1) == str(capi.AHMC_GLM_ORDINAL_VERSION) == "1"
    assert re.search(r"#define AHMC_GLM_ORDINAL_MAX_CATEGORIES (\d+)", src).group(1) == str(capi.GLM_ORDINAL_MAX_CATEGORIES) == str(G.ORDINAL_MAX_CATEGORIES) == "16"
    assert re.search(r"AHMC_GLM_ORDERED_LOGIT = (\d+)", src).group(1) == str(capi.GLM_ORDERED_LOGIT) == str(G.ORDERED_LOGIT) == "5"
    assert G.ORDINAL_FAMILIES == {"ordered_logit": 5}
    assert '#include "ahmc_glm_factor.h"' in src
    from ahmc_amd import build as B
    assert "ahmc_glm_ordinal.h" in open(B.__file__, encoding="utf-8").read()
    dev = open(os.path.join(ROOT, "advancedhmc.jl_amd", "csrc", "ahmc_glm.hpp"), encoding="utf-8").read()
    assert re.search(r"constexpr int GLM_ORD_MAX_CAT = (\d+);", dev).group(1) == "16"
    # ahmc_hip.h does not know the GLM; the four older GLM headers keep their versions and do not name the new one; FAMILIES and
    # AUX_FAMILIES are what they were
    inc = os.path.join(ROOT, "include")
    hip_h = open(os.path.join(inc, "ahmc_hip.h"), encoding="utf-8").read()
    assert "glm" not in hip_h.lower() and re.search(r"#define AHMC_ABI_VERSION (\d+)", hip_h).group(1) == "6" == str(capi.AHMC_ABI_VERSION)
    for hdr, macro, v in (("ahmc_glm.h", "AHMC_GLM_VERSION", capi.AHMC_GLM_VERSION), ("ahmc_glm_hier.h", "AHMC_HGLM_VERSION", capi.AHMC_HGLM_VERSION),
                          ("ahmc_glm_aux.h", "AHMC_GLM_AUX_VERSION", capi.AHMC_GLM_AUX_VERSION),
                          ("ahmc_glm_factor.h", "AHMC_GLM_FACTOR_VERSION", capi.AHMC_GLM_FACTOR_VERSION)):
        src = open(os.path.join(inc, hdr), encoding="utf-8").read()
        assert re.search(rf"#define {macro} (\d+)", src).group(1) == str(v) == "1" and "ordinal" not in src.lower() and "ORDERED" not in src
    assert G.FAMILIES == {"bernoulli_logit": 0, "poisson_log": 1, "gaussian_identity": 2, "gaussian_identity_sigma": 3, "negbinomial_log": 4}
    assert G.AUX_FAMILIES == (3, 4)
    with pytest.raises(ValueError, match="unknown GLM family"):
        G.family_code("ordered_logit")


def test_julia_ccalls_match_the_header():
    protos, _ = header_prototypes()
    src = open(os.path.join(ROOT, "julia", "AdvancedHMCMI355XGLMOrdinal.jl"), encoding="utf-8").read()
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
    assert 'include("AdvancedHMCMI355XGLMOrdinal.jl")' in ext and "ahmc_glm_ordinal_set_target" not in ext
    assert ext.index('include("AdvancedHMCMI355XGLMFactor.jl")') < ext.index('include("AdvancedHMCMI355XGLMOrdinal.jl")')


NEW_KERNELS = ([f"k_glm_eta{f}<{t}, 5, {bn}>" for t in ("float", "double") for f in ("", "_f") for bn in (64, 16)]
               + [f"k_{w}<{t}>" for w in ("glm_cut", "hglm_finish_ord") for t in ("float", "double")])


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="needs llvm-objdump")
def test_library_exports_and_kernels_without_scratch():
    """every entry point is in the dynamic symbol table (read without loading the library); the new kernels are in the code object
    with no private segment and no spill (scripts/kernel_meta.py); each FAM 5 eta instantiation fits two waves per SIMD by its
    registers (VGPR + AGPR <= 256) and two workgroups per CU by its LDS (<= 80 KiB)"""
    from ahmc_amd import build as B

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_meta
    finally:
        sys.path.pop(0)
    assert os.path.exists(B.OUT), "build() first"
    exported = {l.split()[-1] for l in subprocess.run(["nm", "-D", "--defined-only", B.OUT], capture_output=True, text=True, check=True).stdout.splitlines() if l.strip()}
    assert set(capi.GLM_ORDINAL_SIGNATURES) <= exported, set(capi.GLM_ORDINAL_SIGNATURES) - exported
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
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, (w, k)
        if w.startswith("k_glm_eta"):
            assert k["vgpr_count"] + k.get("agpr_count", 0) <= 256, (w, k)
            assert k["group_segment_fixed_size"] <= 80 * 1024, (w, k)


# ------------------------------------------------------------------------------------------------
# CPU 4: the constructor, misuse, the checker's refusal
# ------------------------------------------------------------------------------------------------
def test_constructor_and_refusals():
    rs = np.random.default_rng(2)
    n = 20
    X, y = rs.normal(size=(n, 3)), rs.integers(0, 4, size=n)
    y[:4] = np.arange(4)
    t = A.GLMTarget(X, y, family="ordered_logit", n_categories=4)
    assert (t.family, t.n_categories, t.D, t.P, t.cut_rows, t.cut_prior, t.aux) == (5, 4, 6, 3, (3, 6), (0.0, 2.5, 0.0, 1.0), False)
    h = A.HierGLMTarget(X, y, [A.CoefGroup(0, 2, False, 1.0)], family="ordered_logit", n_categories=4, cut_prior=CUT_PRIOR, factors=[A.Factor(y % 2, 2)])
    assert (h.D, h.P, h.cut_rows, h.cut_prior) == (5 + 1 + 3, 5, (6, 9), CUT_PRIOR)
    th = rs.normal(size=(h.D, 2))
    np.testing.assert_array_equal(h.cutpoints(th), G.cutpoints(th[6:]))
    lp, g = h.logdensity(th)
    lp2, g2 = G.ordinal_logdensity(h.X, y, th, 4, [(0, 2, False, 1.0)], None, None, CUT_PRIOR, factors=[(y % 2, 2)])
    np.testing.assert_array_equal(lp, lp2)
    np.testing.assert_array_equal(g, g2)
    beta, tau = h.coefficients(th)
    assert beta.shape == (5, 2) and tau.shape == (1, 2)
    assert A.GLMTarget(X, y, family=5, n_categories=4).family == 5
    for kw in (dict(family="bernoulli_logit", n_categories=2), dict(family="poisson_log", cut_prior=CUT_PRIOR), dict(family="ordered_logit"),
               dict(family="ordered_logit", n_categories=4, scale=2.0), dict(family="ordered_logit", n_categories=4, aux_prior=(0.0, 1.0)),
               dict(family="ordered_logit", n_categories=1), dict(family="ordered_logit", n_categories=17), dict(family="ordered_logit", n_categories=3),
               dict(family="ordered_logit", n_categories=4, cut_prior=(0.0, 0.0, 0.0, 1.0)), dict(family="ordered_logit", n_categories=4, cut_prior=(0.0, 1.0, np.inf, 1.0)),
               dict(family="ordered_logit", n_categories=4, cut_prior=(0.0, 1.0, 0.0, -1.0)), dict(family="ordered_logit", n_categories=4, cut_prior=(0.0, 1.0))):
        with pytest.raises(A.ArgumentError):
            A.GLMTarget(X, y, **kw)
    with pytest.raises(A.ArgumentError, match="DomainError.*not a category"):
        A.GLMTarget(X, np.where(np.arange(n) == 3, 1.5, y), family="ordered_logit", n_categories=4)
    with pytest.raises(A.ArgumentError, match="DomainError.*not a category"):
        A.GLMTarget(X, np.where(np.arange(n) == 3, -1, y), family="ordered_logit", n_categories=4)
    with pytest.raises(A.ArgumentError, match="no cutpoints"):
        A.GLMTarget(X, (y > 1).astype(float)).cut_rows
    for bad in (lambda: G.check_cut_prior((0, 1, 0)), lambda: G.check_cut_prior((0, 1, 0, 0)), lambda: G.check_cut_prior((np.nan, 1, 0, 1)),
                lambda: G.ordinal_logdensity(X, y, np.zeros((5, 2)), 4), lambda: G.ordinal_logdensity(X, y, np.zeros((6, 2)), 3),
                lambda: G.check_categories(y, 17)):
        with pytest.raises(ValueError):
            bad()
    assert G.check_cut_prior(None) == (0.0, 2.5, 0.0, 1.0)


def test_cpu_checker_refuses_the_target(oracle):
    assert oracle.has_glm_ordinal is False
    c = ocase("two-blocks", 3, "float64")
    t = target(c)
    with pytest.raises(A.UnsupportedError, match="ahmc_glm_ordinal.h"):
        A.Engine(A.Hamiltonian(A.UnitEuclideanMetric(t.D), t), 3, lib=oracle)
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric(t.D), A.IsoGaussian(t.D)), 3, lib=oracle)
    with pytest.raises(A.UnsupportedError, match="ahmc_glm_ordinal.h"):
        e.set_target(t)
    with pytest.raises(A.UnsupportedError, match="ahmc_glm_ordinal.h"):
        e.glm_cutpoints()
    e.close()


# ------------------------------------------------------------------------------------------------
# CPU 5: the bounds on a host emulation, and planted defects
# ------------------------------------------------------------------------------------------------
def check_emulation(key, c, eps, r):
    ord_check(key, c, eps, W=r["W"], tau=r["tau"], cut=r["cut"], ll=r["ll"], lp=r["lp"], g=r["g"], eta=r["eta"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_bounds_hold_for_a_host_emulation_and_catch_three_defects(dtype):
    """the device's arithmetic emulated in the element type and in the contract's order passes every bound of the GPU value test on
    every case; with r dropped from db, with the suffix sum taken as a prefix sum, or with the last row block of partial_c dropped,
    the cutpoint-gradient assertion fails (and only the defect's own quantities move)"""
    dtname = np.dtype(dtype).name
    eps = host_eps(dtype)
    for name in CASES:
        c = ocase(name, 5, dtname)
        check_emulation(f"emulation {dtname} {name}", c, eps, ord_emulate(c))
    for name in ("two-blocks", "slices", "factors"):
        c = ocase(name, 5, dtname)
        for defect in ("drop_r", "prefix", "drop_block"):
            r = ord_emulate(c, defect)
            keep = dict(MARGINS)
            with pytest.raises(AssertionError, match="ord-cutgrad"):
                check_emulation(f"defect-{defect} {dtname} {name}", c, eps, r)
            for k in set(MARGINS) - set(keep):        # (a planted defect's ratios are no margins of the code)
                del MARGINS[k]


# ------------------------------------------------------------------------------------------------
# CPU 7 / GPU 4: the parity inputs, and their precondition on the oracle alone
# ------------------------------------------------------------------------------------------------
# name: (n_obs, P, C, groups, seed)
PARITY = {"(130, 9, C = 4)": (130, 9, 4, (), 1), "(130, 9 + 2, C = 4)": (130, 9, 4, ((0, 4, True, 1.0), (4, 9, False, 1.0)), 1)}
DENSE_CASE = "(130, 9 + 2, C = 4)"
WIDE = (70, 4200, 3, ((10, 200, False, 1.0),), 1)


def parity_inputs(n_obs, P, Cn, groups, seed, N=64):
    Gn = len(groups)
    rs = np.random.default_rng([n_obs, P, Gn, Cn, seed, 5])
    X = rs.normal(size=(n_obs, P)) / np.sqrt(P)
    eta = X @ rs.normal(size=P)
    cuts = np.linspace(-1.0, 1.0, Cn - 1)
    y = (eta.reshape(-1, 1) + rs.logistic(size=(n_obs, 1)) > cuts).sum(axis=1)
    p = np.ones(P)
    for lo, hi, _, _ in groups:
        p[lo:hi] = 0
    D = P + Gn + Cn - 1
    minv = np.asfortranarray(0.5 + rs.random((D, N)))
    th0 = 0.5 * rs.normal(size=(D, N)) * (0.2 if P > 1000 else 1.0)
    eps = 0.1 * (0.7 + 0.6 * rs.random(N))
    kw = dict(family="ordered_logit", n_categories=Cn, prior_prec=p)
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
        smallest, n_div = TG.parity_sequence(o, None, th0, eps, "glm-ordinal wide", nuts_depth=5, full=False)
    else:
        t, minv, th0, eps = parity_inputs(*PARITY[DENSE_CASE if name == "dense" else name])
        o = TH.oracle_engine(oracle, t, TA.dense_metric(t.D) if name == "dense" else A.DiagEuclideanMetric(minv), th0.shape[1])
        smallest, n_div = TG.parity_sequence(o, None, th0, eps, f"glm-ordinal {name}")
    MARGINS[f"ord-oracle-margin {name}"] = {"smallest_decision_margin": smallest, "divergent_chains_max": n_div}
    TG._dump_margins()
    dump_profile()
    o.close()


# ---------------------------------------------------------------------------------------------------------------------
# the guard-band cases of the new entry points: registered in the table of tests/test_buffer_bounds.py, whose gate counts them
# ---------------------------------------------------------------------------------------------------------------------
_PRE = "ahmc_glm_ordinal_set_target"
_SET_IN = ("X", "y", "offset", "prior_prec", "lo", "hi", "centered", "hyper_scale", "n_levels", "levels", "cut_prior")


def c_ordinal_set_target(r, n_obs, where):
    """every array of ahmc_glm_ordinal_set_target: the data in device or host memory, the tables in host memory"""
    N, Px, Cn = 5, 3, 4
    P = Px + 5
    i32 = lambda v: np.array(v, dtype=np.int32)  # noqa: E731
    for dtype in (TB.F64, TB.F32):
        rs = np.random.default_rng(n_obs)
        d = {"X": rs.normal(size=n_obs * Px).astype(dtype), "y": rs.integers(0, Cn, n_obs).astype(dtype), "offset": (0.1 * rs.normal(size=n_obs)).astype(dtype),
             "prior_prec": np.array([0.5, 0, 0] + [1.0] * 5, dtype=dtype)}
        ins = {f"{_PRE}.{k}": In(v, where) for k, v in d.items()}
        tab = {"lo": i32([1]), "hi": i32([3]), "centered": i32([0]), "hyper_scale": np.array([1.5]), "n_levels": i32([2, 3]),
               "levels": np.concatenate([rs.integers(0, 2, n_obs), rs.integers(0, 3, n_obs)]).astype(np.int32), "cut_prior": np.array(CUT_PRIOR)}
        ins.update({f"{_PRE}.{k}": In(v, "host") for k, v in tab.items()})

        def call(e, io):
            p = lambda k: io[f"{_PRE}.{k}"]  # noqa: E731
            pi, pd = C.POINTER(C.c_int32), C.POINTER(C.c_double)
            r.ok(e, r.lib.dll.ahmc_glm_ordinal_set_target(e._ctx, n_obs, Px, p("X"), p("y"), p("offset"), p("prior_prec"), 1, C.cast(p("lo"), pi), C.cast(p("hi"), pi),
                                                          C.cast(p("centered"), pi), C.cast(p("hyper_scale"), pd), 2, C.cast(p("n_levels"), pi), C.cast(p("levels"), pi),
                                                          Cn, C.cast(p("cut_prior"), pd)))
            out = TB.glm_observe(r, e, n_obs, dtype)
            out["cutpoints"] = e.glm_cutpoints()
            return out
        r.probe(lambda: TB.engine(r.lib, P + 1 + Cn - 1, N, dtype, metric="unit", position=False), call, ins=ins)


def bound_ordinal(r, n_obs, dtype, N=5):
    rs = np.random.default_rng(n_obs)
    X = rs.normal(size=(n_obs, 3))
    t = A.HierGLMTarget(X, rs.integers(0, 4, n_obs), [A.CoefGroup(1, 3, False, 1.5)], family="ordered_logit", n_categories=4, cut_prior=CUT_PRIOR)
    return TB.engine(r.lib, t.D, N, dtype, metric="unit", target=t)


def c_ordinal_post(r, n_obs, where):
    """theta and out of ahmc_glm_cutpoints, sized exactly, for n_cols below, at and above N, from device and host draws; the outputs of
    ahmc_glm_ordinal_get_target (n_categories as an array of one)"""
    D, Cm1 = 3 + 1 + 3, 3
    dll = r.lib.dll
    for dtype in (TB.F64, TB.F32):
        for n_cols in (1, 5, 15):
            th = (0.4 * np.random.default_rng(n_cols).normal(size=D * n_cols)).astype(dtype)
            for w_in in ("device", "host"):
                r.probe(lambda: bound_ordinal(r, n_obs, dtype), lambda e, io: r.ok(e, dll.ahmc_glm_cutpoints(e._ctx, io["ahmc_glm_cutpoints.theta"], n_cols,
                                                                                                                 io["ahmc_glm_cutpoints.out"])),
                        ins={"ahmc_glm_cutpoints.theta": In(th, w_in)}, outs={"ahmc_glm_cutpoints.out": Out(dtype, Cm1 * n_cols, where)})

    def call(e, io):
        r.ok(e, dll.ahmc_glm_ordinal_get_target(e._ctx, C.cast(io["ahmc_glm_ordinal_get_target.n_categories"], C.POINTER(C.c_int32)),
                                                C.cast(io["ahmc_glm_ordinal_get_target.cut_prior"], C.POINTER(C.c_double))))
    r.probe(lambda: bound_ordinal(r, n_obs, TB.F64), call, outs={"ahmc_glm_ordinal_get_target.n_categories": Out(np.int32, 1, "host"),
                                                                  "ahmc_glm_ordinal_get_target.cut_prior": Out(np.float64, 4, "host")})


BOUNDS_CASES = []
for _n in (1, 70):
    for _w in ("device", "host"):
        for _cid, _fn, _probes in ((f"glm-ordinal-set-target-nobs{_n}-{_w}", c_ordinal_set_target, [f"{_PRE}.{k}" for k in _SET_IN]),
                                   (f"glm-ordinal-post-nobs{_n}-{_w}", c_ordinal_post, ["ahmc_glm_cutpoints.theta", "ahmc_glm_cutpoints.out",
                                                                                       "ahmc_glm_ordinal_get_target.n_categories", "ahmc_glm_ordinal_get_target.cut_prior"])):
            if _cid not in TB.CASES:
                TB.add(_cid, _fn, _probes, oracle=False, n_obs=_n, where=_w)
            BOUNDS_CASES.append(_cid)


def test_bounds_cases_cover_the_header():
    """every pointer parameter of include/ahmc_glm_ordinal.h but the context is probed by a case above"""
    params = {p for p in TB.header_pointer_params() if p[0] in capi.GLM_ORDINAL_SIGNATURES and p[1] != "ctx"}
    probed = {tuple(k.split(".")) for cid in BOUNDS_CASES for k in TB.CASES[cid].probes}
    assert params == probed and len(params) == 15


@pytest.mark.gpu
@pytest.mark.parametrize("cid", BOUNDS_CASES)
def test_hip_bounds(hip, monkeypatch, cid):
    """no call of the new entry points reads or writes outside the caller's arrays (tests/arena_util.py).  There is no path of these
    calls without a GPU: the CPU checker does not implement the header."""
    if hip.backend != "hip:gfx950":
        pytest.skip("the CPU checker does not implement include/ahmc_glm_ordinal.h")
    TB.run_case(hip, monkeypatch, cid)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
_STATE = {}


@pytest.fixture(scope="module")
def probe_o(hip):
    import torch

    from ahmc_amd import build as B
    from ahmc_amd.hipmod import Module

    torch.cuda.init()
    if "probe_o" not in _STATE:
        _STATE["probe_o"] = Module(B.build_probe_object(PROBE_O))
    return _STATE["probe_o"]


def device_eps(probe, probe_o, dtype):  # noqa: F811
    """ε_exp, ε_log1p of the existing probe and ε_lg, ε_r (with expm1's own error) of the new one, measured once per element type"""
    key = ("eps", np.dtype(dtype).name)
    if key not in _STATE:
        import torch

        def gap(d):
            d_d = TG.dev(d)
            outs = [torch.empty_like(d_d) for _ in range(3)]
            probe_o.launch("glm_ordinal_probe_gap_" + TG._sfx(dtype), (d.size + 255) // 256, 256, d_d, *outs, np.int64(d.size))
            return tuple(TG.host(o, d.shape) for o in outs)

        eps = dict(TG.device_eps(probe, dtype))
        eps.update(gap_eps(gap, dtype))
        _STATE[key] = eps
        MARGINS[f"ord-device-functions {np.dtype(dtype).name}"] = dict(eps)
        TG._dump_margins()
    return _STATE[key]


def dump_profile():
    """the ordinal entries of the margins → $AHMC_TEST_OUT/glm_ordinal_margins.json (copied to profiles/ by whoever runs the suite)"""
    out = os.environ.get("AHMC_TEST_OUT") or os.path.join(ROOT, "test_out")
    try:
        os.makedirs(out, exist_ok=True)
        mine = {k: v for k, v in sorted(MARGINS.items()) if k.startswith("ord-")}
        worst = {}
        for k, v in mine.items():
            if "error_over_bound" in v:
                worst[k.split(" ")[0]] = max(worst.get(k.split(" ")[0], 0.0), v["error_over_bound"])
        with open(os.path.join(out, "glm_ordinal_margins.json"), "w") as f:
            json.dump({"worst_error_over_bound_per_quantity": worst, "cases": mine}, f, indent=1)
    except OSError:
        pass


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
    return {"eta": eta, "loglik": ll, "lp": z.lp.value.copy(), "grad": z.lp.gradient.copy(), "W": W, "tau": tau, "cut": e.glm_cutpoints()}


# ---- §1 ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_values_against_exact_references(hip, probe, probe_o, dtype):  # noqa: F811
    """every case under either tile shape: η of ahmc_glm_pointwise is the k-ordered fma chain on the device's own W (the factors'
    gathers as one-hot columns) bit for bit; ahmc_glm_cutpoints, ℓ, ℓπ, the coefficient rows and the cutpoint rows of g inside the
    bounds of the module docstring; the getters report the model; the two tile shapes give the same bits"""
    dtname = np.dtype(dtype).name
    eps = device_eps(probe, probe_o, dtype)
    for name, (n_obs, Px, Cn, groups, levels) in CASES.items():
        for N in (N_CHAINS, 48):
            c = ocase(name, N, dtname)
            e = engine(hip, c)
            fam, nc, cp = C.c_int32(), C.c_int32(), (C.c_double * 4)()
            e._call("ahmc_get_target_glm", C.byref(fam), None, None)
            e._call("ahmc_glm_ordinal_get_target", C.byref(nc), cp)
            assert (fam.value, nc.value, tuple(cp)) == (5, Cn, CUT_PRIOR) and e.glm_factors() == (Px, list(levels))
            with pytest.raises(A.ArgumentError, match="no model with a sampled dispersion"):
                e.glm_dispersion()
            res = {}
            for which in ("small", "big"):
                with TG.tile_shape(which):
                    r = res[which] = evaluate(e, c["th"])
                    e.sync()
                assert np.isfinite(r["lp"]).all() and np.isfinite(r["grad"]).all()
                ord_check(f"{dtname} {name} N{N} {which}", c, eps, W=r["W"], tau=r["tau"], cut=r["cut"], ll=r["loglik"], lp=r["lp"], g=r["grad"], eta=r["eta"])
            for k in res["small"]:
                record_bits(f"ord-tile-shapes-{k} {dtname} {name} N{N}", res["small"][k], res["big"][k])
            e.close()
    dump_profile()


# ---- §2 ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_new_kernels_on_a_chain_list(hip, probe_o, dtype):
    """k_glm_cut, k_glm_eta<T, 5, BN> (both tile shapes) and k_hglm_finish_ord launched from the probe on all chains and on every third
    chain, reversed: the listed columns of U, partial, partial_c, the cutpoint table, ℓπ and all rows of g carry the bits of the full
    launch, the others keep their NaN fill, both tile shapes give the same bits; partial_c equals the host's ordered additions of the
    device's own da / db (the probe's link kernel on the device's own η and table) bit for bit; η is the engine's"""
    import torch

    dtype = np.dtype(dtype)
    tch = TG.TCH[dtype]
    N = N_CHAINS
    idx = np.arange(N)[::3][::-1].copy()
    rest = np.setdiff1d(np.arange(N), idx)
    for name in ("two-blocks", "limit", "slices"):
        n_obs, Px, Cn, groups, _ = CASES[name]
        c = ocase(name, N, dtype.name)
        P, PG, D, Cm1, nrb = c["P"], c["PG"], c["D"], Cn - 1, (n_obs + 63) // 64
        key = f"{dtype.name} {name}"
        e = engine(hip, c)
        ev = evaluate(e)
        e.close()
        W = np.asfortranarray(ev["W"])
        R = np.asfortranarray(np.random.default_rng(9).normal(size=(P, N)), dtype=dtype)      # (R = −Xᵀu is an input of the finishing kernel: any numbers)
        tabh = np.zeros(4 * 32 * 4 // 4 + 32 * dtype.itemsize // 4 * 1, dtype=np.int32)          # HglmTab<T>: lo, hi, centered (int[32] each), inv_a2 (T[32])
        for k, (lo, hi, cen, _) in enumerate(groups):
            tabh[k], tabh[32 + k], tabh[64 + k] = lo, hi, int(cen)
        tabh[96:96 + 32 * dtype.itemsize // 4] = np.concatenate([c["ia2"], np.zeros(32 - len(groups), dtype=dtype)]).view(np.int32)
        X_d, y_d, off_d, W_d, th_d, R_d, p_d = (TG.dev(a) for a in (c["X"], c["yT"], c["off"], W, c["th"], R, c["p"]))
        tab_d = torch.from_numpy(tabh).cuda()
        cp = (float(CUT_PRIOR[0]), 1.0 / CUT_PRIOR[1] ** 2, float(CUT_PRIOR[2]), 1.0 / CUT_PRIOR[3] ** 2)

        def nan(*shape):
            return torch.full((int(np.prod(shape)),), float("nan"), dtype=th_d.dtype, device="cuda")

        out = {}
        for bn in (64, 16):
            eta_k = f"_ZN4ahmc9k_glm_etaI{tch}Li5ELi{bn}EEEvPKT_S3_S3_S1_S3_PS1_S4_iillPKiS4_S4_S3_lS4_"
            for which, lst in (("all", None), ("list", idx)):
                n = N if lst is None else lst.size
                idx_d = TG.NULL if lst is None else TG.dev(lst)
                U_d, part_d, pc_d, cut_d, eta_d, ll_d, lp_d, g_d = (nan(n_obs, N), nan(nrb, N), nan(Cm1, nrb, N), nan(3, Cm1, N), nan(n_obs, N), nan(n_obs, N), nan(N),
                                                                     nan(D, N))
                probe_o.launch(f"_ZN4ahmc9k_glm_cutI{tch}EEvPKT_lliPS1_llPKii", (n + 255) // 256, 256, th_d, np.int64(D), np.int64(PG), int(Cm1), cut_d, np.int64(N),
                               np.int64(n), idx_d, 1)
                grid = (nrb * (((n + 63) // 64 + 7) // 8 * 8),) if bn == 64 else (nrb, (n + 15) // 16)
                probe_o.launch(eta_k, grid, 256, X_d, y_d, off_d, dtype.type(1), W_d, U_d, part_d, n_obs, int(P), np.int64(n), np.int64(N), idx_d, eta_d, ll_d,
                               cut_d, np.int64(Cm1), pc_d)
                probe_o.launch(f"_ZN4ahmc17k_hglm_finish_ordI{tch}EEvPKT_S3_S3_S3_S3_S3_PKNS_7HglmTabIS1_EEPS1_S8_iiillPKiiidddd", (n + 3) // 4, 256, part_d, pc_d,
                               R_d, W_d, p_d, th_d, tab_d, lp_d, g_d, int(nrb), int(P), len(groups), np.int64(n), np.int64(N), idx_d, 0, int(Cm1), *cp)
                out[(bn, which)] = [TG.host(U_d, (n_obs, N)), TG.host(part_d, (N, nrb)).T, TG.host(pc_d, (N, nrb, Cm1)).transpose(2, 1, 0).reshape(Cm1 * nrb, N),
                                    TG.host(cut_d, (N, Cm1, 3)).transpose(2, 1, 0).reshape(3 * Cm1, N), TG.host(eta_d, (n_obs, N)), TG.host(ll_d, (n_obs, N)),
                                    TG.host(lp_d, (1, N)), TG.host(g_d, (D, N))]
                if bn == 64 and lst is None:
                    lk = [nan(n_obs, N) for _ in range(4)]
                    probe_o.launch("glm_ordinal_probe_link_" + TG._sfx(dtype), (n_obs * N + 255) // 256, 256, y_d, eta_d, cut_d, int(Cm1), np.int64(n_obs), np.int64(N), *lk)
                    link = [TG.host(t, (n_obs, N)) for t in lk]
        names = ("U", "partial", "partial_c", "cut-table", "eta", "loglik", "lp", "grad")
        for bn in (64, 16):
            for nm, a, b, b64 in zip(names, out[(bn, "list")], out[(bn, "all")], out[(64, "all")]):
                assert np.isfinite(b).all(), (nm, bn)
                record_bits(f"ord-chain-list-{nm}-bn{bn} {key}", a[:, idx], b[:, idx])
                assert np.isnan(a[:, rest]).all(), (nm, bn)
                record_bits(f"ord-tile-shapes-{nm} {key}", b, b64)
        full = dict(zip(names, out[(64, "all")]))
        record_bits(f"ord-probe-eta-is-the-engine's {key}", full["eta"], ev["eta"])
        record_bits(f"ord-probe-link-loglik {key}", link[0], full["loglik"])
        record_bits(f"ord-probe-link-u {key}", link[1], full["U"])
        want = partial_c_of(c["y"], link[2], link[3], Cn).reshape(Cm1 * nrb, N)
        np.testing.assert_array_equal(TG.bits_of(np.where(full["partial_c"] == 0, 0, full["partial_c"])), TG.bits_of(np.where(want == 0, 0, want)), err_msg=f"partial_c {key}")
        record_bits(f"ord-cut-table-c {key}", full["cut-table"][:Cm1], ev["cut"])
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
    c = ocase("slices", N, dtname)
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
            record_bits(f"ord-blocks-{k} {dtname}", a, ev[k][..., cols])
        e.run(TG.nuts_kernel(hi - lo, eps=0.02), 3)
        record_bits(f"ord-blocks-theta {dtname}", e.theta(), th_w[:, cols])
        all_stats_equal(e.stats(), {k: v[cols] for k, v in st_w.items()}, "chain blocks")
        e.close()
    c = ocase("two-blocks", N, dtname)
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
    """the ordinal model, then a plain GLMTarget of the same D on the same context == a fresh context on the plain model, and the
    ordinal model bound again == a fresh context on it; the factor encoding == the one-hot expansion of the same model (values, up to
    the sign of a zero, and three NUTS transitions)"""
    N = N_CHAINS
    c = ocase("factors", N, "float64")
    plain = TG.case(64, c["D"], N, 1, "float64")
    kern = TG.nuts_kernel(N)
    a = engine(hip, c)
    a.transition(TG.nuts_kernel(N, eps=0.02))
    a.set_target(A.GLMTarget(plain["X"], plain["y"], family=1, prior_prec=plain["p"], offset=plain["off"], scale=plain["scale"]))
    with pytest.raises(A.ArgumentError, match="no ordinal model"):
        a.glm_cutpoints()
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
    assert o.glm_factors() == (c["P"], [])
    ra, rb, ro = evaluate(a), evaluate(b), evaluate(o)
    for k in ra:
        record_bits(f"ord-rebound-{k}", ra[k], rb[k])
        record_bits(f"ord-one-hot-{k}", rb[k], ro[k])
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
        TG.parity_sequence(o, g, th0, eps, "glm-ordinal wide", nuts_depth=5, full=False)
    else:
        t, minv, th0, eps = parity_inputs(*PARITY[DENSE_CASE if name == "dense" else name])
        N = th0.shape[1]
        metric = (lambda: TA.dense_metric(t.D)) if name == "dense" else (lambda: A.DiagEuclideanMetric(minv))
        o = TH.oracle_engine(oracle, t, metric(), N)
        g = A.Engine(A.Hamiltonian(metric(), t), N, rng=A.PhiloxRNG(8), lib=hip)
        TG.parity_sequence(o, g, th0, eps, f"glm-ordinal {name}")
    g.close()
    o.close()


# ---- §5 ----
@pytest.mark.gpu
def test_posterior_against_ask_tell(hip):
    """Simulated (400, 3, C = 4) from known β and c; N = 256, NUTS(0.8) with StanHMCAdaptor, 30 adapting + 30 kept transitions at
    max_depth 6 (the ask / tell side evaluates the mirror on the host at every leapfrog: more transitions cost seconds each): the target and ExternalTarget(t.logdensity) on the same engine with the same seeds — each parameter's pooled means
    within 4 pooled MCSE (√(mcse₁² + mcse₂²)) of each other; every true cutpoint inside the pooled 99 % interval of its draws"""
    n_obs, P, Cn, N = 400, 3, 4, 256
    rs = np.random.default_rng(53)
    X = rs.normal(size=(n_obs, P))
    beta, cuts = np.array([0.8, -0.5, 0.3]), np.array([-1.0, 0.2, 1.1])
    y = ((X @ beta).reshape(-1, 1) + rs.logistic(size=(n_obs, 1)) > cuts).sum(axis=1)
    t = A.GLMTarget(X, y, family="ordered_logit", n_categories=Cn, prior_scale=3.0)
    D = t.D
    assert D == 6 and t.cut_rows == (3, 6)
    th0 = 0.1 * rs.normal(size=(D, N))
    stats, cdraws = {}, None
    for name, tgt in (("glm-ordinal", t), ("external", A.ExternalTarget(D, t.logdensity))):
        e = A.Engine(A.Hamiltonian(A.DiagEuclideanMetric((D, N)), tgt), N, rng=A.PhiloxRNG(5), lib=hip)
        kern = TG.nuts_kernel(N, eps=0.1, depth=6)
        e.set_integrator(kern.tau.integrator)
        e.set_position(th0)
        e.adaptor_init(A.StanHMCAdaptor(A.MassMatrixAdaptor(A.DiagEuclideanMetric((D, N))), A.StepSizeAdaptor(0.8, kern.tau.integrator)))
        e.run(kern, 30, n_adapts=30)
        draws = np.empty((30, D + Cn - 1, N))
        for i in range(30):
            e.transition(kern)
            draws[i, :D] = e.theta()
            draws[i, D:] = t.cutpoints(draws[i, :D])          # the cutpoints as quantities of their own
        stats[name] = A.summarystats(draws)
        if name == "glm-ordinal":
            np.testing.assert_allclose(e.glm_cutpoints(draws[-1, :D]), draws[-1, D:], rtol=1e-12, atol=1e-12)
            cdraws = draws[:, D:].transpose(1, 0, 2).reshape(Cn - 1, -1)
        e.close()
    diff = np.abs(stats["glm-ordinal"]["mean"] - stats["external"]["mean"])
    tol = 4 * np.sqrt(stats["glm-ordinal"]["mcse"] ** 2 + stats["external"]["mcse"] ** 2)
    lo, hi = np.quantile(cdraws, [0.005, 0.995], axis=1)
    MARGINS["ord-posterior"] = {"mean_difference_over_tolerance": float((diff / tol).max()), "mean": stats["glm-ordinal"]["mean"].tolist(),
                                "rhat_max": float(stats["glm-ordinal"]["rhat"].max()), "cut_interval_99": [lo.tolist(), hi.tolist()], "cut_true": cuts.tolist()}
    dump_profile()
    print(MARGINS["ord-posterior"])
    assert np.all(diff < tol), (diff / tol)
    assert np.all((lo < cuts) & (cuts < hi)), (lo, cuts, hi)


# ---- §6 ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_refusals(hip, dtype):
    """every refusal of the header, with the status and message class of the Python side; after each refused call the context still
    runs a transition on the model it had; the older set-target entries refuse the family and name the new header"""
    N = 17
    c = ocase("two-blocks", N, np.dtype(dtype).name)
    e = engine(hip, c)
    kern = TG.nuts_kernel(N, eps=0.02)
    n_obs, P = 70, c["P"]
    X, y, off, p = np.asfortranarray(c["X"]), c["yT"].copy(), c["off"].copy(), c["p"].copy()

    def still_runs():
        e.transition(kern)
        assert np.isfinite(e.theta()).all() and e.stats()["n_steps"].min() >= 1
        nc = C.c_int32()
        e._call("ahmc_glm_ordinal_get_target", C.byref(nc), None)
        assert nc.value == 3

    def refused(exc, match, n_coef=P, y_=y, Cn=3, cp=CUT_PRIOR, n_groups=0, n_factors=0):
        with pytest.raises(exc, match=match):
            e._call("ahmc_glm_ordinal_set_target", n_obs, n_coef, capi.as_ptr(X), capi.as_ptr(y_), capi.as_ptr(off), capi.as_ptr(p), n_groups, None, None, None, None,
                    n_factors, None, None, Cn, None if cp is None else (C.c_double * 4)(*cp))
        still_runs()

    def poked(i, v):
        b = y.copy()
        b[i] = v
        return b

    refused(A.ArgumentError, "DomainError.*not a category", y_=poked(5, 1.5))
    refused(A.ArgumentError, "DomainError.*not a category", y_=poked(69, 3))
    refused(A.ArgumentError, "DomainError.*not a category", y_=poked(0, -1))
    refused(A.ArgumentError, "DomainError.*at least 2", Cn=1)
    refused(A.UnsupportedError, "AHMC_GLM_ORDINAL_MAX_CATEGORIES", Cn=17)
    refused(A.ArgumentError, "DimensionMismatch.*n_categories - 1", Cn=4, y_=y)
    refused(A.ArgumentError, "DimensionMismatch", n_coef=P + 1)
    refused(A.ArgumentError, "DomainError.*cut_prior\\[2\\]", cp=(0.0, 0.0, 0.0, 1.0))
    refused(A.ArgumentError, "DomainError.*cut_prior\\[4\\]", cp=(0.0, 1.0, 0.0, -1.0))
    refused(A.ArgumentError, "DomainError.*cut_prior\\[3\\]", cp=(0.0, 1.0, np.nan, 1.0))
    refused(A.ArgumentError, "DomainError.*cut_prior\\[1\\]", cp=(np.inf, 1.0, 0.0, 1.0))
    refused(A.ArgumentError, "NULL", cp=None)
    refused(A.ArgumentError, "DimensionMismatch", n_groups=1)          # (the neighbours' refusals come through)
    refused(A.ArgumentError, "NULL", n_factors=1)
    data = (capi.as_ptr(X), capi.as_ptr(y), capi.as_ptr(off), capi.as_ptr(p))
    for call in (lambda: e._call("ahmc_set_target_glm", 5, n_obs, *data, 1.0),
                 lambda: e._call("ahmc_hglm_set_target", 5, n_obs, P, *data, 1.0, 0, None, None, None, None),
                 lambda: e._call("ahmc_glm_aux_set_target", 5, n_obs, P, *data, 0, None, None, None, None, 0.0, 1.0),
                 lambda: e._call("ahmc_glm_factor_set_target", 5, n_obs, P, *data, 1.0, 0, None, None, None, None, 0, None, None, 0, 0.0, 1.0)):
        with pytest.raises(A.ArgumentError, match="ahmc_glm_ordinal.h"):
            call()
        still_runs()
    with pytest.raises(A.ArgumentError, match="NULL"):
        e._call("ahmc_glm_cutpoints", None, 3, None)
    assert e.glm_cutpoints(np.zeros((c["D"], 0))).shape == (2, 0)
    e.close()
    d = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((8, N)), A.IsoGaussian(8)), N, dtype=dtype, rng=A.PhiloxRNG(1), lib=hip)
    with pytest.raises(A.ArgumentError, match="no ordinal model"):
        d.glm_cutpoints()
    with pytest.raises(A.ArgumentError, match="DimensionMismatch"):
        d.set_target(target(c))
    d.close()
