"""HierGLMTarget (include/ahmc_glm_hier.h): a GLM whose coefficient groups have a sampled prior scale, evaluated for all chains at
once — k_hglm_coef (θ → the effective coefficients W), the GLM target's two MFMA products on W, k_hglm_finish (ℓπ and all D rows of
g); the arithmetic is defined by advancedhmc.jl_amd/glm.py (hier_logdensity).  Helpers come from tests/test_glm_target.py.

CPU: the mirror (gradient against central differences in long double, centred / non-centred equivalence, no groups == the plain
mirror, hier_coefficients, s = ±40 and 400); header == binding table == Julia ccalls == exported symbols; both kernel
instantiations present and scratch-free; the constructor; the CPU checker's refusal; the parity tests' precondition on the oracle
alone; the bounds of §1 on a host emulation, right and with two planted defects.

GPU:
 §1 values.  η through ahmc_glm_pointwise equals the k-ordered fma chain applied to the device's own W, bit for bit; W / β / τ
    (ahmc_hglm_coefficients), ℓπ and every row of g lie inside the bounds below; the two tile shapes give the same bits; the two new
    kernels launched on a scattered chain list (tests/device_probe/glm_hier.hip) give the listed columns the bits of the full launch
    and leave the others alone.
 §2 n_groups = 0 is the plain GLMTarget bit for bit; re-binding leaves no trace.
 §3 invariances, bit for bit: chain blocks, tile shape, bulk == stepwise, checkpoint → resume.
 §4 parity with the oracle running the mirror as a host kernel: every chain, exactly.
 §5 a posterior, against the same model through ask / tell.
 §6 every refusal of the header.

The bounds of §1.  u is the unit roundoff of the element type, γ_k = k·u/(1 − k·u), ε = ε_exp (twice the measured worst relative
error of the device's exp on [−ETA_MAX, ETA_MAX]; the cases assert |s| ≤ ETA_MAX/2 so that s, 2s and −2s are inside).  The
reference is a long-double evaluation of the header's formulas on the values as stored (X, θ, p, 1/A² in the element type).
    τ̂ − τ ≤ ε·τ                                                   one exp
    ŵ − w = 0 (fixed, centred);  ≤ (ε + u)·|w| =: E_w (non-centred)  one exp, one multiplication
    Δη = γ_P·|X|·|ŵ| + u·|η̂| + |X|·E_w                             §1 of test_glm_target.py, plus the error of its input W
    E_ℓ, E_u from Δη                                               the link's Lipschitz constants and roundings, test_glm_target.link_bounds
    R̂ − R ≤ |X|ᵀ·E_u + γ_{n_obs+1}·|X|ᵀ(|u| + E_u) =: E_R            any order of the n_obs products; fma(0, w, −Σ) adds no rounding
    g, fixed d:         E_R + u·|ĝ|                                 fma(p, θ, R̂)
    g, centred member:  ε·q·|θ| + E_R + u·|ĝ|                       fma(q̂, θ, R̂), q̂ one exp
    g, non-centred:     ε·τ·|R| + τ(1 + ε)·E_R + u·|ĝ|              fma(τ̂, R̂, θ)
    Ŝ − S ≤ γ_c·S =: E_S,  c = ⌈m/64⌉ + 6                           ⌈m/64⌉ fmas per lane, six butterfly stages
    T̂ − T ≤ Σ_d [E_R·(|w| + E_w) + |R|·E_w] + γ_c·Σ_d (|R| + E_R)(|w| + E_w) =: E_T
    ĥ′ − h′ ≤ ε·e^{2s}/A² + u·|ĥ′| =: E_h′,   ĥ − h ≤ ½·ε·e^{2s}/A² + u·|ĥ| =: E_h
    g, s_k centred:      ε·q·S + q(1 + ε)·E_S + u·|m − qS| + E_h′ + u·|ĝ|
    g, s_k non-centred:  E_T + E_h′ + u·|ĝ|
    b̂ − b ≤ ½(ε·q·S + q(1 + ε)·E_S) + u·½qS + u·|b̂| (centred);  ½·E_S (non-centred) =: E_b
    ℓπ̂ − ℓπ ≤ [§1's bound on fma(−½, Σ_prior, Σ_ℓ)] + Σ_k (E_h + E_b + u·|h + b|) + u·Σ_k (|ℓπ₀| + Σ_{j≤k} |h_j + b_j|)
Products of two first-order terms are covered by SLACK = 1.01 as in test_glm_target.py; the long-double reference's own roundings
by γ⁶⁴ terms.  Every error / bound is recorded in hglm_margins.json under $AHMC_TEST_OUT (default test_out/);
profiles/hglm_margins.json is the MI355X run.
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
import test_glm_target as TG
from ahmc_amd import _capi as capi
from ahmc_amd import glm as G
from test_glm_target import probe  # noqa: F401  (the fixture: exp / log1p of the device)

LD = np.longdouble
ROOT = TG.ROOT
PROBE_H = os.path.join(ROOT, "tests", "device_probe", "glm_hier.hip")
U, U_LD, SLACK, ETA_MAX, FAMS, DTYPES, gam = TG.U, TG.U_LD, TG.SLACK, TG.ETA_MAX, TG.FAMS, TG.DTYPES, TG.gam
MARGINS = {}
# (n_obs, P, groups (lo, hi, centred, A), family): one group; a centred and a non-centred one; two K slices and a group across the 64-lane stride
VALUE_CASES = ((23, 4, ((1, 3, True, 0.8),), 2), (130, 17, ((5, 11, True, 1.5), (11, 17, False, 0.7)), 0), (1100, 70, ((2, 68, False, 1.0),), 1))
INV_CASE = VALUE_CASES[1]


def _dump_margins():
    out = os.environ.get("AHMC_TEST_OUT") or os.path.join(ROOT, "test_out")
    try:
        os.makedirs(out, exist_ok=True)
        worst = {}
        for k, v in MARGINS.items():
            if "error_over_bound" in v:
                sec = k.split(" ")[0]
                worst[sec] = max(worst.get(sec, 0.0), v["error_over_bound"])
        bits = {"compared": sum(v.get("bit_compared", 0) for v in MARGINS.values()), "mismatch": sum(v.get("bit_mismatch", 0) for v in MARGINS.values())}
        with open(os.path.join(out, "hglm_margins.json"), "w") as f:
            json.dump({"worst_error_over_bound_per_quantity": worst, "elements_compared_bit_for_bit": bits, "cases": dict(sorted(MARGINS.items()))}, f, indent=1)
    except OSError:
        pass


def record_bound(key, err, bound):
    """largest err / bound of a comparison, kept under `key`; asserts it is ≤ 1 element by element"""
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    assert np.isfinite(err).all(), f"{key}: non-finite result"
    frac = np.where(err == 0, LD(0), err / np.where(bound > 0, bound, LD("1e-4900")))
    worst = float(frac.max()) if frac.size else 0.0
    e = MARGINS.setdefault(key, {})
    e["error_over_bound"] = max(e.get("error_over_bound", 0.0), worst)
    _dump_margins()
    print(f"{key}: error / bound = {worst:.4g}")
    if worst > 1.0:
        ij = np.unravel_index(int(np.argmax(frac)), frac.shape)
        raise AssertionError(f"{key}: error {float(err[ij]):.3e} is {worst:.3g} × its bound {float(bound[ij]):.3e} at element {ij}")
    return worst


def record_bits(key, got, want):
    """elements of `got` whose value differs from `want` (±0 one value, any NaN equals any NaN), kept under `key`; asserts there are none"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (key, got.shape, want.shape, got.dtype, want.dtype)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    e = MARGINS.setdefault(key, {})
    e["bit_compared"] = e.get("bit_compared", 0) + int(same.size)
    e["bit_mismatch"] = e.get("bit_mismatch", 0) + int((~same).sum())
    _dump_margins()
    if not same.all():
        bad = np.argwhere(~same)
        raise AssertionError(f"{key}: {len(bad)} of {same.size} elements differ; first at {tuple(bad[0])}: {got[tuple(bad[0])]!r} instead of "
                             f"{want[tuple(bad[0])]!r}")


# ------------------------------------------------------------------------------------------------
# §1's operands, exact references and bounds
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hcase(n_obs, P, groups, fam, N, dtname):
    """operands and long-double references of one case, computed once"""
    dtype = np.dtype(dtname)
    Gn = len(groups)
    D = P + Gn
    rs = np.random.default_rng([n_obs, P, Gn, N, fam, dtype.itemsize])
    X = np.asfortranarray(rs.normal(size=(n_obs, P)) / np.sqrt(P), dtype=dtype)
    th = np.asfortranarray(np.concatenate([rs.normal(size=(P, N)), 0.4 * rs.normal(size=(Gn, N))]), dtype=dtype)
    off = (0.3 * rs.normal(size=n_obs)).astype(dtype)
    if fam == G.BERNOULLI_LOGIT:
        y = np.where(np.arange(n_obs) % 3 == 2, rs.random(n_obs), (rs.random(n_obs) < 0.5).astype(np.float64)).astype(dtype)
    elif fam == G.POISSON_LOG:
        y = rs.poisson(3.0, size=n_obs).astype(dtype)
    else:
        y = rs.normal(size=n_obs).astype(dtype)
    p = (2 * rs.random(P)).astype(dtype)
    p[::3] = 0
    for lo, hi, _, _ in groups:
        p[lo:hi] = 0
    scale = 1.7
    ia2 = np.array([dtype.type(1.0 / (a * a)) for _, _, _, a in groups], dtype=dtype)
    assert np.abs(th[P:]).max() <= ETA_MAX / 2
    t = th.astype(LD)
    s = t[P:]
    tau = np.exp(s)
    W = t[:P].copy()
    for k, (lo, hi, cen, _) in enumerate(groups):
        if not cen:
            W[lo:hi] = tau[k] * t[lo:hi]
    E, S = TG.exact(X, W)
    eta = E + off.astype(LD).reshape(-1, 1)
    ll, uu = TG.link_ld(fam, y.reshape(-1, 1), eta, float(dtype.type(scale)))
    Xt = np.asfortranarray(X.T)
    Gx, Sg = TG.exact(Xt, uu)
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
    lp = lp0 + sum(x["h"] + x["b"] for x in grp)
    return {"X": X, "Xt": Xt, "y": y, "off": off, "p": p, "th": th, "scale": scale, "fam": fam, "dtype": dtype, "groups": groups, "P": P, "ia2": ia2,
            "tau": tau, "W": W, "S_eta": S, "eta": eta, "ll": ll, "u": uu, "Sg": Sg, "R": R, "prior": prior, "lp0": lp0, "g": g, "grp": grp, "lp": lp}


def hier_check(key, c, eps, W=None, tau=None, lp=None, g=None):
    """the assertions of §1 on whatever results are given (the device's, or a host emulation's); `W` (the results' own effective
    coefficients, which fix η̂) is needed for lp and g"""
    dtype, P, groups = c["dtype"], c["P"], c["groups"]
    n_obs = c["X"].shape[0]
    u, ee = U[dtype], LD(eps["exp"])
    t = c["th"].astype(LD)
    absW = np.abs(c["W"])
    Ew = np.zeros_like(absW)
    for lo, hi, cen, _ in groups:
        if not cen:
            Ew[lo:hi] = SLACK * (ee + u) * absW[lo:hi]
    ld = gam(n_obs + P + 64, U_LD)
    if tau is not None:
        record_bound(f"tau {key}", np.abs(tau.astype(LD) - c["tau"]), SLACK * ee * c["tau"] + ld * c["tau"])
    if W is None:
        return
    record_bound(f"W {key}", np.abs(W.astype(LD) - c["W"]), Ew + ld * absW)
    if lp is None and g is None:
        return
    absX = np.abs(c["X"]).astype(LD)
    eta_hat = TG.chain(c["X"], W) + c["off"].reshape(-1, 1)
    assert np.abs(eta_hat).max() <= ETA_MAX
    d_eta = (gam(P, u) + gam(P + 1, U_LD)) * c["S_eta"] * SLACK + (u + U_LD) * np.abs(eta_hat.astype(LD)) + absX @ Ew
    El, Eu = TG.link_bounds({"fam": c["fam"], "dtype": dtype, "eta_hat": eta_hat, "d_eta": d_eta, "y": c["y"], "scale": c["scale"], "ll": c["ll"], "u": c["u"]}, eps)
    XE = absX.T @ Eu
    ER = SLACK * (XE + (gam(n_obs + 1, u) + gam(n_obs + 1, U_LD)) * (c["Sg"] + XE))
    absR = np.abs(c["R"])
    Eg = np.empty_like(c["g"])
    Eg[:P] = ER
    # ℓπ₀ = fma(−½, Σ_prior, Σ_ℓ): §1 of test_glm_target.py (its final rounding is the first u·|·| term of the running sum below)
    Elp = El.sum(axis=0) + (gam(n_obs, u) + gam(n_obs, U_LD)) * (np.abs(c["ll"]) + El).sum(axis=0) + gam(P + 1, u) * c["prior"] / 2
    run = np.abs(c["lp0"])
    Elp = Elp + u * run
    for k, (lo, hi, cen, _) in enumerate(groups):
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
        record_bound(f"lp {key}", np.abs(lp.astype(LD) - c["lp"]), SLACK * Elp + ld * (np.abs(c["ll"]).sum(axis=0) + run))
    if g is not None:
        mag = np.abs(c["g"]) + 1
        mag[:P] += c["Sg"] * (1 + np.abs(c["tau"]).max(axis=0))
        record_bound(f"grad {key}", np.abs(g.astype(LD) - c["g"]), SLACK * (Eg + u * np.abs(g.astype(LD))) + ld * mag)


def lane_sum(a, b):
    """Σ_d a_d·b_d over the rows as the device sums a group: 64 lanes, lane l takes rows l, l + 64, … ascending with fma, then a
    six-stage pairwise tree (the butterfly's depth; its pairing is not modelled — the bound does not depend on it)"""
    lanes = np.zeros((64,) + a.shape[1:], dtype=a.dtype)
    for i in range(0, a.shape[0], 64):
        n = min(64, a.shape[0] - i)
        lanes[:n] = TG.host_fma(np.ascontiguousarray(a[i:i + n]), np.ascontiguousarray(b[i:i + n]), lanes[:n].copy())
    while lanes.shape[0] > 1:
        lanes = lanes[0::2] + lanes[1::2]
    return lanes[0]


def hier_emulate(c, defect=None):
    """the device's arithmetic on the host in the element type, numpy's functions for the device's.  `defect`: "t_sign" gives T_k the
    wrong sign, "drop_ms" drops the −m_k·s_k term of a centred group."""
    dt, P, groups = c["dtype"].type, c["P"], c["groups"]
    th = c["th"]
    b, s = th[:P], th[P:]
    tau = np.exp(s)
    W = b.copy()
    for k, (lo, hi, cen, _) in enumerate(groups):
        if not cen:
            W[lo:hi] = tau[k] * b[lo:hi]
    eta_hat = TG.chain(c["X"], W) + c["off"].reshape(-1, 1)
    ll, _, lsum, R = TG.emulate({"dtype": c["dtype"], "eta_hat": eta_hat, "y": c["y"], "fam": c["fam"], "scale": c["scale"], "Xt": c["Xt"],
                                 "p": np.zeros(P, dtype=c["dtype"]), "th": W})
    p = c["p"].reshape(-1, 1)

    def fma(x, y, z):
        return TG.host_fma(*(np.asarray(v, dtype=c["dtype"]) for v in (x, y, z)))

    lp = lsum - ((p * b) * b).sum(axis=0, dtype=c["dtype"]) / dt(2)
    g = np.empty_like(th)
    g[:P] = TG.host_fma(p, b, R)
    for k, (lo, hi, cen, _) in enumerate(groups):
        m, a2, sk = dt(hi - lo), c["ia2"][k], s[k]
        S, T = lane_sum(b[lo:hi], b[lo:hi]), lane_sum(R[lo:hi], W[lo:hi])
        e2 = np.exp(dt(2) * sk)
        h, hp = fma(dt(-0.5) * e2, a2, sk), fma(-e2, a2, dt(1))
        if cen:
            q = np.exp(dt(-2) * sk)
            bk = fma(dt(0) if defect == "drop_ms" else -m, sk, (dt(-0.5) * q) * S)
            g[lo:hi] = TG.host_fma(q.reshape(1, -1), b[lo:hi], R[lo:hi])
            g[P + k] = fma(-q, S, m) - hp
        else:
            bk = dt(-0.5) * S
            g[lo:hi] = TG.host_fma(tau[k].reshape(1, -1), R[lo:hi], b[lo:hi])
            g[P + k] = (-T if defect == "t_sign" else T) - hp
        lp = lp + (h + bk)
    assert lp.dtype == c["dtype"] and g.dtype == c["dtype"] and W.dtype == c["dtype"]
    return W, tau, lp, g


# ------------------------------------------------------------------------------------------------
# CPU: the mirror
# ------------------------------------------------------------------------------------------------
def small_hier_model(fam, rs, offset=True, prior=True, N=3):
    """P = 9: d = 0, 4, 8 fixed, [1, 4) centred, [5, 8) non-centred"""
    n_obs, P = 23, 9
    groups = ((1, 4, True, 0.7), (5, 8, False, 1.3))
    X, y, _, off, p, scale = TG.small_model(fam, rs, n_obs=n_obs, D=P, N=N, offset=offset, prior=prior)
    th = np.concatenate([rs.normal(size=(P, N)), 0.5 * rs.normal(size=(2, N))])
    if p is not None:
        for lo, hi, _, _ in groups:
            p[lo:hi] = 0
    return X, y, th, off, p, scale, groups


def lp_ld(fam, X, y, t, groups, off, p, scale):
    """ℓπ of the header in long double, written from the formulas and not from the mirror's structure"""
    P = X.shape[1]
    t = np.asarray(t, dtype=LD)
    w = t[:P].copy()
    out = 0
    for k, (lo, hi, cen, a) in enumerate(groups):
        s = t[P + k]
        S = (t[lo:hi] ** 2).sum(axis=0)
        out = out + s - np.exp(2 * s) / (2 * LD(a) ** 2)
        if cen:
            out = out - (hi - lo) * s - np.exp(-2 * s) * S / 2
        else:
            out = out - S / 2
            w[lo:hi] = np.exp(s) * t[lo:hi]
    eta = X.astype(LD) @ w + (0 if off is None else off.astype(LD).reshape(-1, 1))
    ll, _ = TG.link_ld(fam, y.reshape(-1, 1), eta, scale)
    return out + ll.sum(axis=0) - (0 if p is None else (p.astype(LD).reshape(-1, 1) * t[:P] ** 2).sum(axis=0) / 2)


@pytest.mark.parametrize("fam", [0, 1, 2], ids=FAMS)
@pytest.mark.parametrize("offset,prior", [(True, True), (False, False), (True, False)])
def test_hier_mirror_gradient_against_central_differences(fam, offset, prior):
    """∇ℓπ of the mirror against central differences of a long-double evaluation of ℓπ (h = 1e-6), every row: fixed, centred and
    non-centred members, both log-scales"""
    rs = np.random.default_rng(21 + fam)
    X, y, th, off, p, scale, groups = small_hier_model(fam, rs, offset, prior)
    lp, grad = G.hier_logdensity(FAMS[fam], X, y, th, groups, off, p, scale)
    assert lp.shape == (3,) and grad.shape == th.shape
    np.testing.assert_allclose(lp, lp_ld(fam, X, y, th, groups, off, p, scale).astype(np.float64), rtol=1e-13, atol=1e-13)
    h = LD("1e-6")
    for d in range(th.shape[0]):
        tp, tm = th.astype(LD), th.astype(LD)
        tp[d] += h
        tm[d] -= h
        fd = ((lp_ld(fam, X, y, tp, groups, off, p, scale) - lp_ld(fam, X, y, tm, groups, off, p, scale)) / (2 * h)).astype(np.float64)
        np.testing.assert_allclose(grad[d], fd, rtol=1e-8, atol=1e-8)
    eta, ll = G.hier_pointwise(FAMS[fam], X, y, th, groups, off, scale)
    beta, tau = G.hier_coefficients(th, 9, groups)
    np.testing.assert_allclose(eta, X @ beta + (0 if off is None else off.reshape(-1, 1)), rtol=1e-14, atol=1e-14)
    lp1, g1 = G.hier_logdensity(fam, X, y, th[:, 0], groups, off, p, scale)   # a vector θ is one chain
    np.testing.assert_allclose(lp1[0], lp[0], rtol=1e-14)
    np.testing.assert_allclose(g1[:, 0], grad[:, 0], rtol=1e-13, atol=1e-14)


@pytest.mark.parametrize("fam", [0, 1, 2], ids=FAMS)
def test_centred_and_non_centred_are_one_model(fam):
    """ℓπ_nc(z, s) = ℓπ_c(e^s·z, s) + Σ_{non-centred k} m_k·s_k (the Jacobian of β = τ·z), to a few ulps of the sum's magnitude"""
    rs = np.random.default_rng(31 + fam)
    X, y, th, off, p, scale, groups = small_hier_model(fam, rs)
    lp_nc, _ = G.hier_logdensity(fam, X, y, th, groups, off, p, scale)
    thc = th.copy()
    thc[5:8] = np.exp(th[10]) * th[5:8]
    centred = tuple((lo, hi, True, a) for lo, hi, _, a in groups)
    lp_c, _ = G.hier_logdensity(fam, X, y, thc, centred, off, p, scale)
    eta, ll = G.hier_pointwise(fam, X, y, th, groups, off, scale)
    mag = np.abs(ll).sum(axis=0) + (np.abs(th) ** 2).sum(axis=0) + 3 * np.abs(th[10]) + np.exp(2 * th[9:]).sum(axis=0)
    assert np.all(np.abs(lp_nc - (lp_c + 3 * th[10])) <= 8 * np.finfo(np.float64).eps * mag)
    b1, t1 = G.hier_coefficients(th, 9, groups)
    b2, t2 = G.hier_coefficients(thc, 9, centred)
    np.testing.assert_array_equal(b1, b2)
    np.testing.assert_array_equal(t1, t2)


def test_no_groups_is_the_plain_mirror_and_coefficients_round_trip():
    rs = np.random.default_rng(5)
    for fam in (0, 1, 2):
        X, y, th, off, p, scale = TG.small_model(fam, rs)
        a, b = G.hier_logdensity(fam, X, y, th, (), off, p, scale), G.logdensity(fam, X, y, th, off, p, scale)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        for x, y_ in zip(G.hier_pointwise(fam, X, y, th, (), off, scale), G.pointwise(fam, X, y, th, off, scale)):
            np.testing.assert_array_equal(x, y_)
        beta, tau = G.hier_coefficients(th, 4, ())
        np.testing.assert_array_equal(beta, th)
        assert tau.shape == (0, 3)
    X, y, th, off, p, scale, groups = small_hier_model(0, rs)
    beta, tau = G.hier_coefficients(th, 9, groups)
    np.testing.assert_array_equal(tau, np.exp(th[9:]))
    back = np.concatenate([beta, np.log(tau)])
    back[5:8] = beta[5:8] / tau[1]
    np.testing.assert_allclose(back, th, rtol=1e-14, atol=1e-15)
    np.testing.assert_array_equal(beta[[0, 1, 2, 3, 4, 8]], th[[0, 1, 2, 3, 4, 8]])
    for bad, msg in ((((1, 4, True, 1.0), (3, 6, False, 1.0)), "overlaps"), (((5, 8, True, 1.0), (1, 4, False, 1.0)), "out of order"),
                     (((2, 2, True, 1.0),), "empty"), (((7, 10, True, 1.0),), "outside"), (((1, 4, True, 0.0),), "DomainError"),
                     (((1, 4, True, np.inf),), "DomainError")):
        with pytest.raises(ValueError, match=msg):
            G.hier_logdensity(0, X, y, th[:9 + len(bad)], bad, off, None, scale)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        G.hier_logdensity(0, X, y, th[:10], groups, off, p, scale)
    with pytest.raises(ValueError, match="must be 0 on the members"):
        G.hier_logdensity(0, X, y, th, groups, off, np.ones(9), scale)


def test_hier_mirror_extremes():
    """s = ±40: ℓπ is finite or sanitises to −Inf, never NaN; s = 400: −Inf"""
    rs = np.random.default_rng(6)
    for fam in (0, 1, 2):
        X, y, th, off, p, scale, groups = small_hier_model(fam, rs, N=6)
        th[9] = [40, -40, 40, -40, 400, 0.1]
        th[10] = [40, -40, -40, 40, 0.1, 400]
        with np.errstate(all="ignore"):
            lp, g = G.hier_logdensity(fam, X, y, th, groups, off, p, scale)
        out = G.sanitize(lp)
        assert not np.isnan(out).any()
        assert np.all(np.isfinite(out) | (out == -np.inf))
        assert out[4] == -np.inf and out[5] == -np.inf
        assert np.isfinite(out[1])   # (τ → 0 non-centred: the likelihood at w = 0;  centred at s = −40: −½·e^{80}·S, finite in Float64)


def test_hierglmtarget_constructor():
    rs = np.random.default_rng(2)
    X, y = rs.normal(size=(12, 6)), (rs.random(12) < 0.5).astype(float)
    t = A.HierGLMTarget(X, y, [A.CoefGroup(1, 3), A.CoefGroup(3, 6, centered=True, scale=2.5)], prior_scale=2.0)
    assert (t.D, t.P, t.n_obs, t.family, t.kind) == (8, 6, 12, G.BERNOULLI_LOGIT, capi.TARGET_GLM)
    assert t.groups == (A.CoefGroup(1, 3, False, 1.0), A.CoefGroup(3, 6, True, 2.5))
    np.testing.assert_array_equal(t.prior_prec, [0.25, 0, 0, 0, 0, 0])   # members are forced to 0
    assert isinstance(t, A.GLMTarget)
    th = 0.3 * rs.normal(size=(8, 2))
    lp, g = t.logdensity(th)
    want = G.hier_logdensity(0, X, y, th, ((1, 3, False, 1.0), (3, 6, True, 2.5)), None, t.prior_prec, 1.0)
    np.testing.assert_array_equal(lp, want[0])
    np.testing.assert_array_equal(g, want[1])
    beta, tau = t.coefficients(th)
    assert beta.shape == (6, 2) and tau.shape == (2, 2)
    A.Hamiltonian(A.UnitEuclideanMetric(8), t)
    with pytest.raises(A.ArgumentError):
        A.Hamiltonian(A.UnitEuclideanMetric(6), t)
    t0 = A.HierGLMTarget(X, y, [], family="poisson_log")
    assert t0.D == 6 and t0.groups == () and t0.prior_prec is None
    assert A.HierGLMTarget(X, y, [(0, 6)]).groups == (A.CoefGroup(0, 6, False, 1.0),)
    for bad in (lambda: A.HierGLMTarget(X, y, [A.CoefGroup(1, 1)]), lambda: A.HierGLMTarget(X, y, [A.CoefGroup(4, 7)]),
                lambda: A.HierGLMTarget(X, y, [A.CoefGroup(-1, 2)]), lambda: A.HierGLMTarget(X, y, [A.CoefGroup(1, 4), A.CoefGroup(3, 5)]),
                lambda: A.HierGLMTarget(X, y, [A.CoefGroup(3, 5), A.CoefGroup(0, 2)]), lambda: A.HierGLMTarget(X, y, [A.CoefGroup(1, 3, scale=0.0)]),
                lambda: A.HierGLMTarget(X, y, [A.CoefGroup(1, 3, scale=np.nan)]), lambda: A.HierGLMTarget(X, y, [A.CoefGroup(0, 1)] * 2),
                lambda: A.HierGLMTarget(rs.normal(size=(12, 40)), y, [A.CoefGroup(k, k + 1) for k in range(33)]),
                lambda: A.HierGLMTarget(X, y[:-1], []), lambda: A.HierGLMTarget(X, y, [], family="probit"),
                lambda: A.HierGLMTarget(X, y, [], prior_scale=1.0, prior_prec=1.0)):
        with pytest.raises(A.ArgumentError):
            bad()


# ------------------------------------------------------------------------------------------------
# CPU: header, bindings, Julia, the shipped kernels, the checker
# ------------------------------------------------------------------------------------------------
def header_prototypes():
    src = open(os.path.join(ROOT, "include", "ahmc_glm_hier.h"), encoding="utf-8").read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(int32_t)\s+(ahmc_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        params = " ".join(m.group(3).split())
        protos[m.group(2)] = [] if params in ("", "void") else [p.strip() for p in params.split(",")]
    return protos, src


def test_header_and_bindings_agree():
    protos, src = header_prototypes()
    assert set(protos) == set(capi.HGLM_SIGNATURES) == {"ahmc_hglm_version", "ahmc_hglm_set_target", "ahmc_hglm_get_target", "ahmc_hglm_coefficients"}
    assert len(capi.GLM_SIGNATURES) == 4 and not set(capi.GLM_SIGNATURES) & set(capi.HGLM_SIGNATURES)
    ct = {"int64_t*": C.POINTER(C.c_int64), "int32_t*": C.POINTER(C.c_int32), "double*": C.POINTER(C.c_double), "int64_t": C.c_int64,
          "int32_t": C.c_int32, "double": C.c_double}
    for name, params in protos.items():
        res, args = capi.HGLM_SIGNATURES[name]
        assert res is C.c_int32 and len(args) == len(params), name
        for p, a in zip(params, args):
            typ = p.rsplit(" ", 1)[0].replace("const ", "").replace(" ", "")
            if typ in ("void*", "ahmc_ctx*"):
                assert a is C.c_void_p, (name, p)
            else:
                assert a is ct[typ], (name, p)
    assert [p.split()[-1] for p in protos["ahmc_hglm_set_target"]] == ["ctx", "family", "n_obs", "n_coef", "X", "y", "offset", "prior_prec", "scale", "n_groups",
                                                                      "lo", "hi", "centered", "hyper_scale"]
    assert re.search(r"#define AHMC_HGLM_VERSION (\d+)", src).group(1) == str(capi.AHMC_HGLM_VERSION) == "1"
    assert re.search(r"#define AHMC_HGLM_MAX_GROUPS (\d+)", src).group(1) == str(capi.HGLM_MAX_GROUPS) == str(G.HGLM_MAX_GROUPS) == "32"
    dev = open(os.path.join(ROOT, "advancedhmc.jl_amd", "csrc", "ahmc_glm.hpp"), encoding="utf-8").read()
    assert int(re.search(r"constexpr int HGLM_MAX_GROUPS = (\d+);", dev).group(1)) == 32
    # the headers of the plain model and of the ABI do not know the new one
    for other in ("ahmc_glm.h", "ahmc_hip.h"):
        assert "hglm" not in open(os.path.join(ROOT, "include", other), encoding="utf-8").read().lower()
    from ahmc_amd import build as B
    assert "ahmc_glm_hier.h" in open(B.__file__, encoding="utf-8").read()


def test_julia_ccalls_match_the_header():
    protos, _ = header_prototypes()
    src = open(os.path.join(ROOT, "julia", "AdvancedHMCMI355XGLMHier.jl"), encoding="utf-8").read()
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
    assert 'include("AdvancedHMCMI355XGLMHier.jl")' in ext and "ahmc_hglm" not in ext
    assert ext.index('include("AdvancedHMCMI355XGLM.jl")') < ext.index('include("AdvancedHMCMI355XGLMHier.jl")')


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="needs llvm-objdump")
def test_library_exports_and_kernels_without_scratch():
    """every entry point is exported; both instantiations of the two kernels are in the code object with no private segment and no
    VGPR spill (the code object's kernel metadata, scripts/kernel_meta.py)"""
    from ahmc_amd import build as B

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_meta
    finally:
        sys.path.pop(0)
    assert os.path.exists(B.OUT), "build() first"
    # (the dynamic symbol table, read without loading the library into this process)
    exported = {l.split()[-1] for l in subprocess.run(["nm", "-D", "--defined-only", B.OUT], capture_output=True, text=True, check=True).stdout.splitlines() if l.strip()}
    assert set(capi.HGLM_SIGNATURES) <= exported, set(capi.HGLM_SIGNATURES) - exported
    meta = kernel_meta.kernel_meta(B.OUT)
    names = subprocess.run(["c++filt"], input="\n".join(k["name"] for k in meta), capture_output=True, text=True, check=True).stdout.splitlines()
    want = [f"k_hglm_{w}<{t}>" for w in ("coef", "finish") for t in ("float", "double")]
    found = {}
    for k, dn in zip(meta, names):
        for w in want:
            if dn.startswith(f"void ahmc::{w}("):
                found[w] = k
    assert sorted(found) == sorted(want), sorted(set(want) - set(found))
    for w, k in found.items():
        assert k["private_segment_fixed_size"] == 0, (w, k)
        assert k.get("vgpr_spill_count", 0) == 0, (w, k)


def test_cpu_checker_refuses_hier_glm_target(oracle):
    assert oracle.has_hglm is False
    rs = np.random.default_rng(5)
    t = A.HierGLMTarget(rs.normal(size=(7, 4)), (rs.random(7) < 0.5).astype(float), [A.CoefGroup(1, 3)])
    with pytest.raises(A.UnsupportedError, match="ahmc_glm_hier.h"):
        A.Engine(A.Hamiltonian(A.UnitEuclideanMetric(5), t), 3, lib=oracle)
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric(5), A.IsoGaussian(5)), 3, lib=oracle)
    with pytest.raises(A.UnsupportedError, match="ahmc_glm_hier.h"):
        e.hglm_coefficients()
    with pytest.raises(A.UnsupportedError, match="ahmc_glm_hier.h"):
        e.set_target(t)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_bounds_hold_for_a_host_emulation_and_catch_two_defects(dtype):
    """The planted defects.  The device's arithmetic emulated on the host in the element type passes every assertion of §1 (numpy's
    exp / log1p measured the way the device's are); with T_k given the wrong sign the gradient assertion fails, with −m_k·s_k dropped
    the ℓπ assertion: the bounds can fail."""
    eps = TG.function_eps(np.exp, np.log1p, dtype)
    for n_obs, P, groups, fam in VALUE_CASES:
        c = hcase(n_obs, P, groups, fam, 5, np.dtype(dtype).name)
        key = f"host-emulation {FAMS[fam]} {np.dtype(dtype).name} ({n_obs}, {P})"
        W, tau, lp, g = hier_emulate(c)
        hier_check(key, c, eps, W=W, tau=tau, lp=lp, g=g)
        before = json.dumps({k: v for k, v in MARGINS.items() if k.endswith(key) and "planted" not in k})
        if any(not cen for _, _, cen, _ in groups):
            _, _, _, g_bad = hier_emulate(c, "t_sign")
            with pytest.raises(AssertionError, match="grad planted"):
                hier_check("planted " + key, c, eps, W=W, g=g_bad)
        if any(cen for _, _, cen, _ in groups):
            _, _, lp_bad, _ = hier_emulate(c, "drop_ms")
            with pytest.raises(AssertionError, match="lp planted"):
                hier_check("planted " + key, c, eps, W=W, lp=lp_bad)
        for k in [k for k in MARGINS if " planted " in k]:
            del MARGINS[k]
        assert json.dumps({k: v for k, v in MARGINS.items() if k.endswith(key)}) == before
    _dump_margins()


# ------------------------------------------------------------------------------------------------
# §4's inputs, and its precondition on the oracle alone
# ------------------------------------------------------------------------------------------------
# name: (n_obs, P, groups, family, seed, s0): s0 the starting value of every log-scale (None: random)
PARITY = {"logit (130, 17 + 2)": (130, 17, ((5, 11, True, 1.0), (11, 17, False, 1.0)), "bernoulli_logit", 1, None),
          "poisson (65, 40 + 1)": (65, 40, ((8, 40, False, 1.0),), "poisson_log", 1, None),
          "divergent (130, 17 + 1)": (130, 17, ((5, 17, True, 1.0),), "bernoulli_logit", 1, -3.0)}


def hier_parity_inputs(n_obs, P, groups, family, seed, s0, N=300):
    """test_glm_target.parity_inputs for the P coefficient columns (the same step sizes), the log-scales appended"""
    Gn = len(groups)
    X, y, p, _, _, eps = TG.parity_inputs(n_obs, P, family, N)
    rs = np.random.default_rng([n_obs, P, Gn, seed])
    p = p.copy()
    for lo, hi, _, _ in groups:
        p[lo:hi] = 0
    minv = np.asfortranarray(0.5 + rs.random((P + Gn, N)))
    th0 = 0.5 * rs.normal(size=(P + Gn, N))
    if s0 is not None:
        th0[P:] = s0
    t = A.HierGLMTarget(X, y, groups, family=family, prior_prec=p)
    return t, minv, th0, eps


def oracle_engine(oracle, t, metric, N, seed=8):
    """the oracle on the mirror as a host kernel, as test_glm_target.oracle_engine"""
    from test_user_targets import host_kernel

    cb = host_kernel(t.logdensity)
    return A.Engine(A.Hamiltonian(metric, A.KernelTarget(t.D, cb, handle_kind=capi.KERNEL_HOST)), N, rng=A.PhiloxRNG(seed), lib=oracle)


def first_transition_divergences(e, th0, eps):
    """chains of engine `e` whose first NUTS transition from th0 ends in a numerical error"""
    lf = A.Leapfrog(eps)
    e.set_integrator(lf)
    e.set_position(th0)
    e.transition(A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=6))))
    return int(e.stats()["numerical_error"].sum())


@pytest.mark.parametrize("name", list(PARITY))
def test_parity_precondition_on_the_oracle_alone(oracle, name):
    """On §4's inputs no decision of the oracle comes within MARGIN_BOUND[float64] of a tie, at any step of the sequence: the GPU
    comparison may demand exact agreement of every chain.  The divergent case (a centred group started at s = −3, q = e⁶, with the
    step sizes of the plain parity inputs): at least half of the chains diverge in their first transition."""
    t, minv, th0, eps = hier_parity_inputs(*PARITY[name])
    N = th0.shape[1]
    o = oracle_engine(oracle, t, A.DiagEuclideanMetric(minv), N)
    smallest, n_div = TG.parity_sequence(o, None, th0, eps, f"hglm {name}")
    MARGINS[f"oracle-margin {name}"] = {"smallest_decision_margin": smallest, "divergent_chains_max": n_div}
    if name.startswith("divergent"):
        o2 = oracle_engine(oracle, t, A.DiagEuclideanMetric(minv), N)
        first = first_transition_divergences(o2, th0, eps)
        o2.close()
        MARGINS[f"oracle-margin {name}"]["divergent_in_first_transition"] = first
        assert first >= N // 2, first
    _dump_margins()
    o.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
_STATE = {}


@pytest.fixture(scope="module")
def probe_h(hip):
    import torch

    from ahmc_amd import build as B
    from ahmc_amd.hipmod import Module

    torch.cuda.init()
    if "probe_h" not in _STATE:
        _STATE["probe_h"] = Module(B.build_probe_object(PROBE_H))
    return _STATE["probe_h"]


def hier_target(c):
    return A.HierGLMTarget(c["X"], c["y"], c["groups"], family=c["fam"], prior_prec=c["p"], offset=c["off"], scale=c["scale"])


def hglm_engine(hip, c, cols=None, metric=None, seed=7):
    """an engine on the case's model, positioned at the case's θ (or the columns `cols` of it)"""
    th = c["th"] if cols is None else c["th"][:, cols]
    D, N = th.shape
    e = A.Engine(A.Hamiltonian(metric or A.UnitEuclideanMetric((D, N)), hier_target(c)), N, dtype=c["dtype"],
                 rng=seed if isinstance(seed, A.PhiloxRNG) else A.PhiloxRNG(seed), lib=hip)
    e.set_integrator(A.Leapfrog(np.full(N, 0.05)))
    e.set_position(th)
    return e


def evaluate(e, th=None):
    if th is not None:
        e.set_position(th)
    z = e.phasepoint()
    eta, ll = e.glm_pointwise()
    W, tau = e.hglm_coefficients()
    return eta, ll, W, tau, z.lp.value.copy(), z.lp.gradient.copy()


NAMES = ("eta", "loglik", "W", "tau", "lp", "grad")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_values_against_exact_references(hip, probe, dtype):  # noqa: F811
    """§1: η bit for bit from the device's own W; W / β / τ, ℓπ and every row of g inside their bounds; the same bits from either
    tile shape; ahmc_hglm_get_target returns the table"""
    eps = TG.device_eps(probe, dtype)
    for n_obs, P, groups, fam in VALUE_CASES:
        c = hcase(n_obs, P, groups, fam, 300, np.dtype(dtype).name)
        key = f"{FAMS[fam]} {np.dtype(dtype).name} ({n_obs}, {P})"
        e = hglm_engine(hip, c)
        nc, ng = C.c_int64(), C.c_int32()
        lo, hi, cen, Asc = (C.c_int32 * 32)(), (C.c_int32 * 32)(), (C.c_int32 * 32)(), (C.c_double * 32)()
        e._call("ahmc_hglm_get_target", C.byref(nc), C.byref(ng), lo, hi, cen, Asc)
        assert (nc.value, ng.value) == (P, len(groups))
        assert tuple((lo[k], hi[k], bool(cen[k]), Asc[k]) for k in range(ng.value)) == groups
        fam_got, n_got = C.c_int32(), C.c_int64()
        e._call("ahmc_get_target_glm", C.byref(fam_got), C.byref(n_got), None)
        assert (fam_got.value, n_got.value) == (fam, n_obs)
        eta, ll, W, tau, lp, g = evaluate(e)
        record_bits(f"eta {key}", eta, TG.chain(c["X"], W) + c["off"].reshape(-1, 1))
        hier_check(key, c, eps, W=W, tau=tau, lp=lp, g=g)
        # draws given as an array of any width, and as a device pointer
        b2, t2 = e.hglm_coefficients(c["th"][:, :7])
        record_bits(f"coefficients-of-draws {key}", np.concatenate([b2, t2]), np.concatenate([W[:, :7], tau[:, :7]]))
        th_d = TG.dev(c["th"])
        b3, t3 = e.hglm_coefficients(int(th_d.data_ptr()), n_cols=300)
        record_bits(f"coefficients-of-device-draws {key}", np.concatenate([b3, t3]), np.concatenate([W, tau]))
        for which in ("small", "big"):
            with TG.tile_shape(which):
                got = evaluate(e, c["th"])
            for name, a, b in zip(NAMES, got, (eta, ll, W, tau, lp, g)):
                record_bits(f"tile-shape-{which}-{name} {key}", a, b)
        e.close()


def table_bytes(c):
    """HglmTab<T> of csrc/ahmc_glm.hpp: int lo[32], hi[32], centered[32]; T inv_a2[32]"""
    ints = np.zeros((3, 32), dtype=np.int32)
    for k, (lo, hi, cen, _) in enumerate(c["groups"]):
        ints[:, k] = (lo, hi, int(cen))
    a = np.zeros(32, dtype=c["dtype"])
    a[:len(c["groups"])] = c["ia2"]
    return np.frombuffer(ints.tobytes() + a.tobytes(), dtype=np.uint8).copy()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_new_kernels_on_a_chain_list(hip, probe_h, dtype):
    """§1: k_hglm_coef and k_hglm_finish launched from the probe on given `partial` and R, all chains and a scattered list: the listed
    columns have the bits of the full launch (which equal the engine's W), the columns off the list keep their NaN"""
    import torch

    dtype = np.dtype(dtype)
    tch = TG.TCH[dtype]
    coef = f"_ZN4ahmc11k_hglm_coefI{tch}EEvPKT_PKNS_7HglmTabIS1_EEPS1_S8_iillPKi"
    fin = f"_ZN4ahmc13k_hglm_finishI{tch}EEvPKT_S3_S3_S3_S3_PKNS_7HglmTabIS1_EEPS1_S8_iiillPKii"
    N = 300
    for n_obs, P, groups, fam in VALUE_CASES:
        c = hcase(n_obs, P, groups, fam, N, dtype.name)
        Gn, D, nrb = len(groups), P + len(groups), (n_obs + 63) // 64
        rs = np.random.default_rng([n_obs, P, 99])
        part = np.asfortranarray(rs.normal(size=(nrb, N)), dtype=dtype)
        Rm = np.asfortranarray(rs.normal(size=(P, N)), dtype=dtype)
        idx = np.sort(rs.choice(N, size=N // 3, replace=False))
        th_d, tab_d, part_d, R_d, p_d = TG.dev(c["th"]), torch.from_numpy(table_bytes(c)).cuda(), TG.dev(part), TG.dev(Rm), TG.dev(c["p"])
        out = {}
        for which, lst in (("all", None), ("list", idx)):
            n = N if lst is None else lst.size
            idx_d = TG.NULL if lst is None else TG.dev(lst)
            W_d = torch.full((P * N,), float("nan"), dtype=th_d.dtype, device="cuda")
            tau_d = torch.full((Gn * N,), float("nan"), dtype=th_d.dtype, device="cuda")
            lp_d = torch.full((N,), float("nan"), dtype=th_d.dtype, device="cuda")
            g_d = torch.full((D * N,), float("nan"), dtype=th_d.dtype, device="cuda")
            probe_h.launch(coef, (n + 3) // 4, 256, th_d, tab_d, W_d, tau_d, int(P), int(Gn), np.int64(D), np.int64(n), idx_d)
            if which == "list":  # (finish reads W of the listed columns only; give it the full W so that NaN in g can only be "not written")
                W_in = TG.dev(out["all"][0])
            else:
                W_in = W_d
            probe_h.launch(fin, (n + 3) // 4, 256, part_d, R_d, W_in, p_d, th_d, tab_d, lp_d, g_d, int(nrb), int(P), int(Gn), np.int64(n), np.int64(N), idx_d, 1)
            out[which] = (TG.host(W_d, (P, N)), TG.host(tau_d, (Gn, N)), TG.host(lp_d, (1, N)), TG.host(g_d, (D, N)))
        rest = np.setdiff1d(np.arange(N), idx)
        key = f"{dtype.name} ({n_obs}, {P})"
        for name, a, b in zip(("W", "tau", "lp", "grad"), out["list"], out["all"]):
            assert np.isfinite(b).all(), name
            record_bits(f"chain-list-{name} {key}", a[:, idx], b[:, idx])
            assert np.isnan(a[:, rest]).all(), name
        e = hglm_engine(hip, c)
        W, tau = e.hglm_coefficients()
        e.close()
        record_bits(f"probe-W-is-the-engine's {key}", out["all"][0], W)
        record_bits(f"probe-tau-is-the-engine's {key}", out["all"][1], tau)


# ---- §2 n_groups = 0 ----
def stats_equal(a, b, keys=("n_steps", "tree_depth", "log_density", "numerical_error")):
    for key in keys:
        np.testing.assert_array_equal(a.stats()[key], b.stats()[key])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_no_groups_is_the_plain_glm_bit_for_bit(hip, dtype):
    """HierGLMTarget(groups = []) == GLMTarget of the same X over a NUTS transition and a bulk run of 3; and a context that held a
    hierarchical model and then a plain one equals a fresh context"""
    N = 130
    c = TG.case(130, 17, N, 0, np.dtype(dtype).name)
    kern = TG.nuts_kernel(N)
    plain = TG.glm_engine(hip, c)
    t0 = A.HierGLMTarget(c["X"], c["y"], [], family=0, prior_prec=c["p"], offset=c["off"], scale=c["scale"])
    none = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((17, N)), t0), N, dtype=dtype, rng=A.PhiloxRNG(7), lib=hip)
    none.set_integrator(A.Leapfrog(np.full(N, 0.05)))
    none.set_position(c["th"])
    ng = C.c_int32(-1)
    none._call("ahmc_hglm_get_target", None, C.byref(ng), None, None, None, None)
    assert ng.value == 0
    with pytest.raises(A.ArgumentError, match="no hierarchical GLM"):
        plain._call("ahmc_hglm_get_target", None, C.byref(ng), None, None, None, None)
    beta, tau = none.hglm_coefficients()
    np.testing.assert_array_equal(beta, c["th"])
    assert tau.shape == (0, N)
    # a context that held a hierarchical model first
    hc = hcase(130, 16, ((5, 11, True, 1.5),), 1, N, np.dtype(dtype).name)   # (D = 16 + 1 = 17)
    was = hglm_engine(hip, hc)
    was.transition(kern)
    was.set_target(A.GLMTarget(c["X"], c["y"], family=0, prior_prec=c["p"], offset=c["off"], scale=c["scale"]))
    with pytest.raises(A.ArgumentError, match="no hierarchical GLM"):
        was.hglm_coefficients()
    was.seed(A.PhiloxRNG(7))
    was.set_position(c["th"])
    for e in (plain, none, was):
        e.transition(kern)
    for e in (none, was):
        np.testing.assert_array_equal(e.theta(), plain.theta())
        stats_equal(e, plain)
    for e in (plain, none, was):
        e.run(kern, 3)
    for e in (none, was):
        np.testing.assert_array_equal(e.theta(), plain.theta())
        stats_equal(e, plain)
        for x, y_ in zip(e.glm_pointwise(), plain.glm_pointwise()):
            np.testing.assert_array_equal(x, y_)
        z, zp = e.phasepoint(), plain.phasepoint()
        np.testing.assert_array_equal(z.lp.gradient, zp.lp.gradient)
    assert plain.stats()["n_steps"].sum() > N
    for e in (plain, none, was):
        e.close()


# ---- §3 invariances, bit for bit ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_chain_blocks_equal_one_engine(hip, dtype):
    """one engine over N chains == engines over random blocks of the chains: the evaluation at θ, and three NUTS transitions"""
    N = 130
    c = hcase(*INV_CASE, N, np.dtype(dtype).name)
    rs = np.random.default_rng(N)
    cuts = np.concatenate([[0], np.sort(rs.choice(np.arange(1, N), size=3, replace=False)), [N]])
    whole = hglm_engine(hip, c, seed=A.PhiloxRNG(17))
    ev = evaluate(whole)
    whole.run(TG.nuts_kernel(N), 3)
    th_w, st_w = whole.theta(), whole.stats()
    whole.close()
    assert st_w["n_steps"].sum() > 3 * N
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        cols = np.arange(lo, hi)
        e = hglm_engine(hip, c, cols=cols, seed=A.PhiloxRNG(17, chain_offset=int(lo)))
        for name, a, b in zip(NAMES, evaluate(e), ev):
            record_bits(f"blocks-{name} {np.dtype(dtype).name}", a, b[..., cols])
        e.run(TG.nuts_kernel(hi - lo), 3)
        record_bits(f"blocks-theta {np.dtype(dtype).name}", e.theta(), th_w[:, cols])
        np.testing.assert_array_equal(e.stats()["n_steps"], st_w["n_steps"][cols])
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_tile_shape_does_not_change_a_run(hip, dtype):
    """three NUTS transitions with the 64×16 tiles forced == with the 64×64 tiles forced == the default rule"""
    N = 130
    c = hcase(*INV_CASE, N, np.dtype(dtype).name)
    out = {}
    for which in ("default", "small", "big"):
        e = hglm_engine(hip, c)
        if which == "default":
            e.run(TG.nuts_kernel(N), 3)
        else:
            with TG.tile_shape(which):
                e.run(TG.nuts_kernel(N), 3)
                e.sync()
        out[which] = (e.theta(), e.stats()["n_steps"].copy())
        e.close()
    assert out["default"][1].sum() > 3 * N
    for which in ("small", "big"):
        record_bits(f"tile-shape-run-{which} {np.dtype(dtype).name}", out[which][0], out["default"][0])
        np.testing.assert_array_equal(out[which][1], out["default"][1])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_checkpoint_resume_and_bulk_equals_stepwise(hip, dtype):
    """get_state after 11 of 24 NUTS iterations (20 adapting, StanHMCAdaptor) → a fresh context with the target set again → the rest ==
    uninterrupted; and the bulk run == the stepwise loop of transition + adapt"""
    N, D = 70, 19
    c = hcase(*INV_CASE, N, np.dtype(dtype).name)
    kern = TG.nuts_kernel(N)

    def engine(adapt=True):
        e = hglm_engine(hip, c, metric=A.DiagEuclideanMetric((D, N)))
        e.set_integrator(kern.tau.integrator)
        if adapt:
            e.adaptor_init(A.StanHMCAdaptor(A.MassMatrixAdaptor(A.DiagEuclideanMetric((D, N))), A.StepSizeAdaptor(0.8, kern.tau.integrator), 5, 5, 5))
        return e

    whole = engine()
    whole.run(kern, 24, n_adapts=20)
    part = engine()
    part.run(kern, 11, n_adapts=20)
    st = part.get_state()
    part.close()
    fresh = engine(adapt=False)
    fresh.set_state(st)
    fresh.run(kern, 24, n_adapts=20, i_first=12)
    step = engine()
    for i in range(1, 25):
        step.transition(kern)
        step.adapt(i, 20)
    for e in (fresh, step):
        np.testing.assert_array_equal(whole.theta(), e.theta())
        np.testing.assert_array_equal(whole.get_stepsize(), e.get_stepsize())
        np.testing.assert_array_equal(whole.get_metric(), e.get_metric())
        e.close()
    assert not np.array_equal(whole.get_metric(), np.ones((D, N)))
    whole.close()


# ---- §4 parity with the oracle ----
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PARITY))
def test_hier_glm_target_against_oracle(hip, oracle, name):
    """the HIP engine on HierGLMTarget against the oracle on the mirror as a host kernel: static HMC, two NUTS transitions,
    find_good_stepsize, a bulk run of three — every discrete statistic of every chain"""
    t, minv, th0, eps = hier_parity_inputs(*PARITY[name])
    N = th0.shape[1]
    o = oracle_engine(oracle, t, A.DiagEuclideanMetric(minv), N)
    g = A.Engine(A.Hamiltonian(A.DiagEuclideanMetric(minv), t), N, rng=A.PhiloxRNG(8), lib=hip)
    smallest, n_div = TG.parity_sequence(o, g, th0, eps, f"hglm {name}")
    if name.startswith("divergent"):
        assert n_div >= N // 2, n_div
        g.seed(A.PhiloxRNG(8))
        assert first_transition_divergences(g, th0, eps) >= N // 2
    g.close()
    o.close()


@pytest.mark.gpu
def test_hier_glm_target_against_oracle_dense_metric(hip, oracle):
    """the same behind a shared DenseEuclideanMetric at (130, 17 + 2)"""
    t, _, th0, eps = hier_parity_inputs(*PARITY["logit (130, 17 + 2)"])
    D, N = th0.shape
    rs = np.random.default_rng(190)
    Q, _ = np.linalg.qr(rs.normal(size=(D, D)))
    Mi = (Q * np.linspace(0.6, 2.0, D)) @ Q.T
    make = lambda: A.DenseEuclideanMetric(np.asfortranarray((Mi + Mi.T) / 2))  # noqa: E731
    o = oracle_engine(oracle, t, make(), N)
    g = A.Engine(A.Hamiltonian(make(), t), N, rng=A.PhiloxRNG(8), lib=hip)
    TG.parity_sequence(o, g, th0, eps, "hglm dense metric (130, 17 + 2)")
    g.close()
    o.close()


@pytest.mark.gpu
def test_hier_glm_target_against_oracle_wide(hip, oracle):
    """a wide context through P: P = 5000 with a non-centred group of 190, n_obs = 40, N = 8, two NUTS transitions at max_depth 5"""
    n_obs, P, N = 40, 5000, 8
    rs = np.random.default_rng(n_obs + P + 1)
    X = rs.normal(size=(n_obs, P)) / np.sqrt(P)
    y = (rs.random(n_obs) < 1 / (1 + np.exp(-(X @ rs.normal(size=P))))).astype(np.float64)
    p = np.ones(P)
    t = A.HierGLMTarget(X, y, [A.CoefGroup(10, 200)], prior_prec=p)
    D = t.D
    th0 = 0.5 * rs.normal(size=(D, N))
    eps = 0.2 * (0.7 + 0.6 * rs.random(N))
    o = oracle_engine(oracle, t, A.UnitEuclideanMetric((D, N)), N)
    g = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((D, N)), t), N, rng=A.PhiloxRNG(8), lib=hip)
    assert g.info("wide")
    TG.parity_sequence(o, g, th0, eps, "hglm wide (40, 5000 + 1)", nuts_depth=5, full=False)
    g.close()
    o.close()


# ---- §5 a posterior ----
@pytest.mark.gpu
def test_posterior_against_ask_tell(hip):
    """Eight groups of 25 observations: an intercept plus one-hot varying intercepts, 8 columns in one non-centred group with A = 1
    (P = 9, D = 10); N = 256, StanHMCAdaptor, 150 adapting + 100 kept transitions: HierGLMTarget and ExternalTarget(t.logdensity) on the
    same engine — R-hat < 1.05 in every dimension for both, pooled means within 5·√(mcse₁² + mcse₂²)"""
    n_grp, per, N = 8, 25, 256
    n_obs, P = n_grp * per, 9
    rs = np.random.default_rng(43)
    X = np.zeros((n_obs, P))
    X[:, 0] = 1
    X[np.arange(n_obs), 1 + np.arange(n_obs) // per] = 1
    alpha = 0.7 * rs.normal(size=n_grp)
    y = (rs.random(n_obs) < 1 / (1 + np.exp(-(0.3 + alpha[np.arange(n_obs) // per])))).astype(np.float64)
    p = np.zeros(P)
    p[0] = 0.25
    t = A.HierGLMTarget(X, y, [A.CoefGroup(1, 9, centered=False, scale=1.0)], prior_prec=p)
    D = t.D
    assert D == 10
    th0 = 0.1 * rs.normal(size=(D, N))
    stats = {}
    for name, target in (("hglm", t), ("external", A.ExternalTarget(D, t.logdensity))):
        e = A.Engine(A.Hamiltonian(A.DiagEuclideanMetric((D, N)), target), N, rng=A.PhiloxRNG(5), lib=hip)
        kern = TG.nuts_kernel(N, eps=0.1, depth=8)
        e.set_integrator(kern.tau.integrator)
        e.set_position(th0)
        e.adaptor_init(A.StanHMCAdaptor(A.MassMatrixAdaptor(A.DiagEuclideanMetric((D, N))), A.StepSizeAdaptor(0.8, kern.tau.integrator)))
        e.run(kern, 150, n_adapts=150)
        draws = np.empty((100, D, N))
        for i in range(100):
            e.transition(kern)
            draws[i] = e.theta()
        stats[name] = A.summarystats(draws)
        if name == "hglm":
            beta, tau = e.hglm_coefficients(draws[-1])
            np.testing.assert_allclose(tau[0], np.exp(draws[-1][9]), rtol=1e-12)
            np.testing.assert_allclose(beta[1:], tau * draws[-1][1:9], rtol=1e-12)
        e.close()
    diff = np.abs(stats["hglm"]["mean"] - stats["external"]["mean"])
    tol = 5 * np.sqrt(stats["hglm"]["mcse"] ** 2 + stats["external"]["mcse"] ** 2)
    MARGINS["posterior"] = {"rhat_hglm": float(stats["hglm"]["rhat"].max()), "rhat_external": float(stats["external"]["rhat"].max()),
                            "mean_difference_over_tolerance": float((diff / tol).max())}
    _dump_margins()
    print(MARGINS["posterior"])
    for name in stats:
        assert np.all(stats[name]["rhat"] < 1.05), (name, stats[name]["rhat"])
    assert np.all(diff < tol), (diff / tol)


# ---- §6 errors ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_refusals(hip, dtype):
    """every AHMC_ERR_ARGUMENT / _UNSUPPORTED case of the header; after each refused call the context still runs a transition on the
    model it had"""
    n, P, N = 65, 6, 17
    groups = ((1, 3, True, 0.9), (3, 6, False, 1.1))
    c = hcase(n, P, groups, 0, N, np.dtype(dtype).name)
    e = hglm_engine(hip, c)
    kern = TG.nuts_kernel(N)
    X, y, off, p = (np.asfortranarray(c["X"]), c["y"].copy(), c["off"].copy(), c["p"].copy())

    def arr(ct, vals):
        return (ct * max(1, len(vals)))(*vals)

    def still_runs():
        e.transition(kern)
        assert np.isfinite(e.theta()).all() and e.stats()["n_steps"].min() >= 1
        ng, lo = C.c_int32(-1), (C.c_int32 * 32)()
        e._call("ahmc_hglm_get_target", None, C.byref(ng), lo, None, None, None)
        assert ng.value == 2 and lo[1] == 3

    def refused(exc, match, fam=0, n_obs=n, n_coef=P, X_=X, y_=y, off_=off, p_=p, scale=1.0, grp=groups, n_groups=None, null=()):
        lo, hi = arr(C.c_int32, [g[0] for g in grp]), arr(C.c_int32, [g[1] for g in grp])
        cen, Asc = arr(C.c_int32, [int(g[2]) for g in grp]), arr(C.c_double, [g[3] for g in grp])
        with pytest.raises(exc, match=match):
            e._call("ahmc_hglm_set_target", fam, n_obs, n_coef, capi.as_ptr(X_), capi.as_ptr(y_), capi.as_ptr(off_), capi.as_ptr(p_), scale,
                    len(grp) if n_groups is None else n_groups, None if "lo" in null else lo, None if "hi" in null else hi, cen, None if "A" in null else Asc)
        still_runs()

    def poked(a, i, v):
        b = a.copy(order="F")
        b.reshape(-1, order="F")[i] = v
        return b

    # D != n_coef + n_groups
    refused(A.ArgumentError, "DimensionMismatch", n_coef=P + 1)
    refused(A.ArgumentError, "DimensionMismatch", grp=groups[:1])
    refused(A.ArgumentError, "DimensionMismatch", n_coef=0)
    refused(A.ArgumentError, "n_groups", n_groups=-1)
    # the ranges
    refused(A.ArgumentError, "ArgumentError.*empty", grp=((1, 1, True, 1.0), (3, 6, False, 1.0)))
    refused(A.ArgumentError, "ArgumentError.*empty", grp=((3, 1, True, 1.0), (3, 6, False, 1.0)))
    refused(A.ArgumentError, "ArgumentError.*out of bounds", grp=((1, 3, True, 1.0), (3, 7, False, 1.0)))
    refused(A.ArgumentError, "ArgumentError.*out of bounds", grp=((-1, 3, True, 1.0), (3, 6, False, 1.0)))
    refused(A.ArgumentError, "ArgumentError.*overlaps", grp=((1, 4, True, 1.0), (3, 6, False, 1.0)))
    refused(A.ArgumentError, "ArgumentError.*out of order", grp=((3, 6, True, 1.0), (1, 3, False, 1.0)))
    refused(A.ArgumentError, "NULL", null=("lo",))
    refused(A.ArgumentError, "NULL", null=("A",))
    # the hyper-scales
    for a in (0.0, -1.0, np.inf, np.nan):
        refused(A.ArgumentError, "DomainError.*hyper_scale", grp=((1, 3, True, a), (3, 6, False, 1.0)))
    # a precision on a member
    refused(A.ArgumentError, "ArgumentError.*member of group 2", p_=poked(p, 4, 0.5))
    # more groups than the engine takes (refused before D is looked at)
    refused(A.UnsupportedError, "AHMC_HGLM_MAX_GROUPS", grp=tuple((k, k + 1, False, 1.0) for k in range(33)))
    # everything ahmc_set_target_glm refuses
    refused(A.UnsupportedError, "AHMC_GLM_MAX_OBS", n_obs=(1 << 24) + 1)
    refused(A.ArgumentError, "n_obs", n_obs=0)
    refused(A.ArgumentError, "NULL", X_=None)
    refused(A.ArgumentError, "NULL", y_=None)
    refused(A.ArgumentError, "X holds a non-finite", X_=poked(X, 7, np.nan))
    refused(A.ArgumentError, "offset holds a non-finite", off_=poked(off, 3, -np.inf))
    refused(A.ArgumentError, "prior_prec holds a non-finite", p_=poked(p, 0, np.nan))
    refused(A.ArgumentError, "negative", p_=poked(p, 0, -1e-3))
    refused(A.ArgumentError, "DomainError", y_=poked(y, 5, 1.5))
    refused(A.ArgumentError, "DomainError", fam=1, y_=poked(y, 64, -1.0))
    refused(A.ArgumentError, "DomainError", fam=2, y_=poked(y, 1, np.nan))
    for s in (0.0, -1.0, np.inf, np.nan):
        refused(A.ArgumentError, "scale", scale=s)
    refused(A.ArgumentError, "unknown family", fam=3)
    # ahmc_hglm_coefficients
    with pytest.raises(A.ArgumentError, match="NULL"):
        e._call("ahmc_hglm_coefficients", None, 3, None, None)
    with pytest.raises(A.ArgumentError, match="n_cols"):
        e._call("ahmc_hglm_coefficients", capi.as_ptr(np.zeros(8, dtype=dtype)), -1, None, None)
    with pytest.raises(A.ArgumentError, match="DimensionMismatch"):
        e.hglm_coefficients(np.zeros((P, 3)))
    still_runs()
    e.close()
    # without a hierarchical model bound
    d = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((8, N)), A.IsoGaussian(8)), N, dtype=dtype, rng=A.PhiloxRNG(1), lib=hip)
    with pytest.raises(A.ArgumentError, match="no hierarchical GLM"):
        d._call("ahmc_hglm_get_target", None, None, None, None, None, None)
    with pytest.raises(A.ArgumentError, match="no hierarchical GLM"):
        d._call("ahmc_hglm_coefficients", capi.as_ptr(np.zeros(8, dtype=dtype)), 1, None, None)
    d.set_integrator(kern.tau.integrator)
    d.set_position(c["th"])
    d.transition(kern)
    assert np.isfinite(d.theta()).all()
    d.close()
