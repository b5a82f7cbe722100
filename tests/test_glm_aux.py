"""GLM families whose dispersion is sampled (include/ahmc_glm_aux.h): "gaussian_identity_sigma" and "negbinomial_log".  θ has
D = P + G + 1 rows — coefficient parameters, the log-scales of the coefficient groups of ahmc_glm_hier.h (G may be 0), and last
s = log σ or log φ.  The arithmetic is defined by advancedhmc.jl_amd/glm.py (aux_logdensity, gamma_diffs); the kernels are
k_glm_eta<T, 3 | 4, BN> and k_hglm_finish_aux of csrc/ahmc_glm.hpp.  Helpers come from tests/test_glm_target.py and test_glm_hier.py.

CPU: the mirror (gradient against central differences; lgamma_diff / digamma_diff against mpmath on the grid of
tests/golden/glm_aux_special.npy; NB against scipy and its Poisson limit; the Gaussian at fixed s); header == binding table ==
Julia ccalls == exported symbols; the new instantiations scratch-free; the constructor; the CPU checker's refusal; the bounds of §1 on
a host emulation, right and with two planted defects; the parity tests' precondition on the oracle alone.

GPU: §1 values, §2 layout independence, §3 resume, §4 parity with the oracle, §5 a posterior against ask / tell, §6 dispersion and
the legacy families, the group table's two ends (no group, AHMC_GLM_AUX_MAX_GROUPS groups), §7 refusals.

The bounds of §1.  u is the unit roundoff of the element type; ε_e, ε_l twice the measured worst relative errors of exp and log1p
(test_glm_target.function_eps); m_L, m_Ψ twice the measured worst multiples of the special functions on the fixture grid:
    |L̂ − L| ≤ m_L·u·(|L| + y·|log(φ + y + 8)| + 1) =: E_L,     |Ψ̂ − Ψ| ≤ m_Ψ·u·(|Ψ| + 1) =: E_Ψ.
The reference is a long-double evaluation of the header's formulas on the values as stored (gamma_diffs with the shift 24 in long
double).  δ bounds |η̂ − η| (test_glm_hier: the k-ordered chain on the device's own W, and W's error); s is exact as stored.
  Gaussian (q = e^{−2s}, q̂ = q(1 + ε_e), r = y − η, δ′ = δ + u|r|):
    E_u = q·δ′ + q|r|(ε_e + u) + u|u|;   E_ℓ = q|r|δ′ + ½qδ′² + ½qr²(ε_e + 2u) + u|ℓ|;   E_∂s = 2q|r|δ′ + qδ′² + qr²(ε_e + 2u) + u|∂ₛℓ|
  NB (φ̂ = φ(1 + ε_e), d = η − s, δ′ = δ + u|d|, l = log1p(e^{−|d|}), E_sp = l(ε_e + ε_l) + u·sp, E_sn likewise; σ′ ≤ ¼):
    E_ℓ = (|u| + ¼(y + φ)δ′)·δ′ + φ|Ψ − sp|ε_e + φ·E_sp + y·E_sn + E_L + u|L − φ·sp| + u|ℓ|
    E_u = (y + φ)(¼δ′ + σ(2ε_e + 2u)) + σ(φε_e + u(y + φ)) + u|u|
    E_∂s = φ[E_Ψ + (1 + 1/φ)ε_e + E_sp + σδ′ + u|Ψ − sp|] + φε_e|Ψ − sp| + φε_e + (y + φ)(¼δ′ + (1 − σ)(2ε_e + 2u)) + (1 − σ)(φε_e + u(y + φ))
           + u|φ − (y + φ)(1 − σ)| + u|∂ₛℓ|             (φ·|∂Ψ/∂φ| ≤ 1 + 1/φ from ψ′(x) ≤ 1/x + 1/x²)
  Sums: Σ_i ∂ₛℓ in any order of n_obs additions: Σ E_∂s + γ_{n_obs}·Σ(|∂ₛℓ| + E_∂s); g[D−1] = fma(r, 1/A², −Σ): + u·|ĝ|, r = s − m adds
  u|r|/A².  ℓπ and rows 0 .. P + G − 1 of g: test_glm_hier.hier_check's bounds with (E_ℓ, E_u) above; the prior of s adds
  4u·½r²/A² + u|ℓπ̂| to ℓπ's bound.
Products of two first-order terms are covered by SLACK = 1.01.  Every error / bound is recorded in glm_aux_margins.json under
$AHMC_TEST_OUT (default test_out/); profiles/glm_aux_margins.json holds the recorded special-function multiples.
"""
import contextlib
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
import test_glm_hier as TH
import test_glm_target as TG
from ahmc_amd import _capi as capi
from ahmc_amd import glm as G
from test_glm_target import probe  # noqa: F401  (the fixture: exp / log1p of the device)

LD = np.longdouble
ROOT = TG.ROOT
PROBE_A = os.path.join(ROOT, "tests", "device_probe", "glm_aux.hip")
FIXTURE = os.path.join(ROOT, "tests", "golden", "glm_aux_special.npy")
PROFILE = os.path.join(ROOT, "profiles", "glm_aux_margins.json")
U, U_LD, SLACK, ETA_MAX, DTYPES, gam = TG.U, TG.U_LD, TG.SLACK, TG.ETA_MAX, TG.DTYPES, TG.gam
AUXFAMS = {3: "gaussian_identity_sigma", 4: "negbinomial_log"}
MARGINS = {}
GRID_Y = (0.0, 0.5, 1.0, 2.0, 7.0, 8.0, 9.0, 100.0, 1e4, 1e6)
GRID_PHI = np.logspace(-6, 8, 57)
# (n_obs, P, groups): across a row block without groups; across K_SLICE with a centred and a non-centred group
VALUE_CASES = ((70, 3, ()), (1100, 5, ((0, 2, True, 0.8), (2, 5, False, 1.3))))
AUX_PRIOR = (0.3, 1.2)


def _dump_margins():
    out = os.environ.get("AHMC_TEST_OUT") or os.path.join(ROOT, "test_out")
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "glm_aux_margins.json"), "w") as f:
            json.dump({"cases": dict(sorted(MARGINS.items()))}, f, indent=1)
    except OSError:
        pass


def record_bound(key, err, bound):
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
# the special functions: long-double reference, the fixture grid, measured multiples
# ------------------------------------------------------------------------------------------------
def gamma_diffs_ld(y, phi, shift=24):
    """(L, Ψ) in long double: the mirror's algorithm with the arguments shifted by 24 (truncation of the eight-term series < 1e-24)"""
    y, phi = np.broadcast_arrays(np.asarray(y, dtype=LD), np.asarray(phi, dtype=LD))
    Aa = phi + shift
    B = Aa + y
    z = y / Aa
    lz = np.log1p(z)

    def horner(c, z2):
        acc = np.full_like(z2, LD(c[-1]))
        for ck in c[-2::-1]:
            acc = acc * z2 + LD(ck)
        return acc

    cs = [LD(1) / 12, -LD(1) / 360, LD(1) / 1260, -LD(1) / 1680, LD(1) / 1188, -LD(691) / 360360, LD(1) / 156, -LD(3617) / 122400]
    ct = [LD(1) / 12, -LD(1) / 120, LD(1) / 252, -LD(1) / 240, LD(1) / 132, -LD(691) / 32760, LD(1) / 12, -LD(3617) / 8160]
    za, zb = 1 / Aa, 1 / B
    dS = zb * horner(cs, zb * zb) - za * horner(cs, za * za)
    dT = zb * zb * horner(ct, zb * zb) - za * za * horner(ct, za * za)
    sl, sp = np.zeros_like(z), np.zeros_like(z)
    for j in range(shift):
        t = y / (phi + j)
        sl = sl + np.log1p(t)
        sp = sp + t / (y + phi + j)
    return ((Aa - LD(0.5)) * lz + y * (np.log(B) - 1)) + dS - sl, ((sp + lz) + (z / 2) / B) - dT


def grid():
    phi, y = np.meshgrid(GRID_PHI, np.array(GRID_Y), indexing="ij")
    return phi.ravel(), y.ravel()


def special_units(y, phi, L, Psi):
    """the units of the two bounds: |L| + y·|log(φ + y + 8)| + 1 and |Ψ| + 1"""
    y, phi = np.asarray(y, dtype=LD), np.asarray(phi, dtype=LD)
    return np.abs(L) + y * np.abs(np.log(phi + y + 8)) + 1, np.abs(Psi) + 1


def special_multiples(fn, dtype):
    """worst |L̂ − L| and |Ψ̂ − Ψ| of `fn(y, φ)` in units of u·(…) on the fixture's grid, against the fixture's references"""
    dtype = np.dtype(dtype)
    fx = np.load(FIXTURE)
    phi, y = fx[:, 0].astype(dtype), fx[:, 1].astype(dtype)
    # (the grid as stored in the element type: the reference is re-evaluated there in long double when the cast moves φ)
    if dtype == np.float64:
        Lr, Pr = fx[:, 2].astype(LD) + fx[:, 3].astype(LD), fx[:, 4].astype(LD) + fx[:, 5].astype(LD)
    else:
        Lr, Pr = gamma_diffs_ld(y, phi)
    L, Ps = fn(y, phi)
    L, Ps = np.asarray(L), np.asarray(Ps)
    assert L.dtype == dtype and Ps.dtype == dtype
    zero = y == 0
    assert np.all(L[zero] == 0) and np.all(Ps[zero] == 0), "y = 0 must give exact zeros"
    uL, uP = special_units(y, phi, Lr, Pr)
    u = U[dtype]
    return float((np.abs(L.astype(LD) - Lr) / (u * uL)).max()), float((np.abs(Ps.astype(LD) - Pr) / (u * uP)).max())


def mirror_eps(dtype):
    """exp / log1p of numpy measured as the device's are, and twice the mirror's special-function multiples"""
    eps = dict(TG.function_eps(np.exp, np.log1p, dtype))
    mL, mP = special_multiples(lambda y, phi: G.gamma_diffs(y, phi, dtype), dtype)
    eps["L"], eps["Psi"] = 2 * mL, 2 * mP
    return eps


# ------------------------------------------------------------------------------------------------
# §1's operands, exact references and bounds
# ------------------------------------------------------------------------------------------------
def link_ld(fam, y, eta, s):
    """(ℓ, u, ∂ₛℓ) in long double, and the pieces the bounds use"""
    y, eta, s = np.asarray(y, dtype=LD), np.asarray(eta, dtype=LD), np.asarray(s, dtype=LD)
    if fam == G.GAUSSIAN_IDENTITY_SIGMA:
        q, r = np.exp(-2 * s), y - eta
        return -q * r * r / 2 - s, q * r, q * r * r - 1, {"q": q + 0 * r, "r": r}
    phi = np.exp(s)
    d = eta - s
    e = np.exp(-np.abs(d))
    l = np.log1p(e)
    sig, nsig = np.where(d >= 0, 1 / (1 + e), e / (1 + e)), np.where(d >= 0, e / (1 + e), 1 / (1 + e))
    sp, sn = np.maximum(d, 0) + l, np.maximum(-d, 0) + l
    L, Psi = gamma_diffs_ld(y + 0 * eta, phi + 0 * eta)
    ll = L - phi * sp - y * sn
    uu = y - (y + phi) * sig
    ds = phi * (Psi - sp) + phi - (y + phi) * nsig
    return ll, uu, ds, {"phi": phi + 0 * eta, "d": d, "l": l, "sig": sig, "nsig": nsig, "sp": sp, "sn": sn, "L": L, "Psi": Psi}


def aux_link_bounds(c, eps, eta_hat, d_eta):
    """(E_ℓ, E_u, E_∂s) of the module docstring, element by element"""
    fam, u = c["fam"], U[c["dtype"]]
    y = c["y"].astype(LD).reshape(-1, 1)
    ee, el = LD(eps["exp"]), LD(eps["log1p"])
    x = c["pieces"]
    ll, uu, ds = np.abs(c["ll"]), np.abs(c["u"]), np.abs(c["ds"])
    if fam == G.GAUSSIAN_IDENTITY_SIGMA:
        q, r = x["q"], np.abs(x["r"])
        dp = d_eta + u * r
        Eu = q * dp + q * r * (ee + u) + u * uu
        El = q * r * dp + q * dp * dp / 2 + q * r * r * (ee + 2 * u) / 2 + u * ll
        Ed = 2 * q * r * dp + q * dp * dp + q * r * r * (ee + 2 * u) + u * ds
    else:
        phi, sig, nsig, sp, sn, L, Psi, l = x["phi"], x["sig"], x["nsig"], x["sp"], x["sn"], x["L"], x["Psi"], x["l"]
        dp = d_eta + u * np.abs(x["d"])
        yp = y + phi
        Esp, Esn = l * (ee + el) + u * sp, l * (ee + el) + u * sn
        uL, uP = special_units(y + 0 * phi, phi, L, Psi)
        EL, EP = LD(eps["L"]) * u * uL, LD(eps["Psi"]) * u * uP
        El = (uu + yp * dp / 4) * dp + phi * np.abs(Psi - sp) * ee + phi * Esp + y * Esn + EL + u * np.abs(L - phi * sp) + u * ll
        Eu = yp * (dp / 4 + sig * (2 * ee + 2 * u)) + sig * (phi * ee + u * yp) + u * uu
        Ed = (phi * (EP + (1 + 1 / phi) * ee + Esp + sig * dp + u * np.abs(Psi - sp)) + phi * ee * np.abs(Psi - sp) + phi * ee
              + yp * (dp / 4 + nsig * (2 * ee + 2 * u)) + nsig * (phi * ee + u * yp) + u * np.abs(phi - yp * nsig) + u * ds)
    ld = 64 * U_LD * (ll + uu + ds + 1)
    return SLACK * El + ld, SLACK * Eu + ld, SLACK * Ed + ld


@functools.lru_cache(maxsize=None)
def acase(n_obs, P, groups, fam, N, dtname):
    """operands and long-double references of one case, computed once (the keys of test_glm_hier.hcase, plus the row of s)"""
    dtype = np.dtype(dtname)
    Gn = len(groups)
    rs = np.random.default_rng([n_obs, P, Gn, N, fam, dtype.itemsize])
    X = np.asfortranarray(rs.normal(size=(n_obs, P)) / np.sqrt(P), dtype=dtype)
    th = np.asfortranarray(np.concatenate([0.6 * rs.normal(size=(P, N)), 0.4 * rs.normal(size=(Gn, N)), 0.5 * rs.normal(size=(1, N))]), dtype=dtype)
    off = (0.3 * rs.normal(size=n_obs)).astype(dtype)
    if fam == G.NEGBINOMIAL_LOG:
        y = rs.poisson(3.0, size=n_obs).astype(dtype)
        y[::7] = 0
        y[3::11] += dtype.type(0.5)   # (not necessarily integers)
    else:
        y = rs.normal(size=n_obs).astype(dtype)
    p = (2 * rs.random(P)).astype(dtype)
    p[::3] = 0
    for lo, hi, _, _ in groups:
        p[lo:hi] = 0
    ia2 = np.array([dtype.type(1.0 / (a * a)) for _, _, _, a in groups], dtype=dtype)
    assert np.abs(th[P:]).max() <= ETA_MAX / 2
    t = th[:P + Gn].astype(LD)
    s = t[P:]
    sa = th[-1:].astype(LD)
    tau = np.exp(s)
    W = t[:P].copy()
    for k, (lo, hi, cen, _) in enumerate(groups):
        if not cen:
            W[lo:hi] = tau[k] * t[lo:hi]
    E, S = TG.exact(X, W)
    eta = E + off.astype(LD).reshape(-1, 1)
    ll, uu, ds, pieces = link_ld(fam, y.reshape(-1, 1), eta, sa)
    Xt = np.asfortranarray(X.T)
    Gx, Sg = TG.exact(Xt, uu)
    R = -Gx
    pth = p.astype(LD).reshape(-1, 1) * t[:P]
    prior = (pth * t[:P]).sum(axis=0)
    lp0 = ll.sum(axis=0) - prior / 2
    g = np.empty((P + Gn + 1, N), dtype=LD)
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
    lph = lp0 + sum(x["h"] + x["b"] for x in grp)
    aia2 = LD(dtype.type(1.0 / (AUX_PRIOR[1] * AUX_PRIOR[1])))
    ra = sa[0] - LD(dtype.type(AUX_PRIOR[0]))
    aprior = ra * ra * aia2 / 2
    g[-1] = ra * aia2 - ds.sum(axis=0)
    return {"X": X, "Xt": Xt, "y": y, "off": off, "p": p, "th": th, "th_h": np.asfortranarray(th[:P + Gn]), "scale": 1.0, "fam": fam, "dtype": dtype,
            "groups": groups, "P": P, "ia2": ia2, "tau": tau, "W": W, "S_eta": S, "eta": eta, "ll": ll, "u": uu, "ds": ds, "pieces": pieces, "Sg": Sg, "R": R,
            "prior": prior, "lp0": lp0, "g": g, "grp": grp, "lp_h": lph, "lp": lph - aprior, "aprior": aprior, "ra": ra, "aia2": aia2}


@contextlib.contextmanager
def _patched(mod, name, fn):
    old = getattr(mod, name)
    setattr(mod, name, fn)
    try:
        yield
    finally:
        setattr(mod, name, old)


def aux_check(key, c, eps, W=None, phi=None, ll=None, lp=None, g=None):
    """the assertions of §1 on whatever results are given (the device's, or a host emulation's).  ℓπ and rows 0 .. P + G − 1 of g go
    through test_glm_hier.hier_check with this module's (E_ℓ, E_u) in place of the three legacy families'."""
    dtype, P, Gn = c["dtype"], c["P"], len(c["groups"])
    n_obs = c["X"].shape[0]
    u, ee = U[dtype], LD(eps["exp"])
    if phi is not None:
        record_bound(f"dispersion {key}", np.abs(phi.astype(LD) - np.exp(c["th"][-1].astype(LD))), SLACK * ee * np.exp(c["th"][-1].astype(LD)))
    if W is None:
        return
    absW = np.abs(c["W"])
    Ew = np.zeros_like(absW)
    for lo, hi, cen, _ in c["groups"]:
        if not cen:
            Ew[lo:hi] = SLACK * (ee + u) * absW[lo:hi]
    eta_hat = TG.chain(c["X"], W) + c["off"].reshape(-1, 1)
    assert np.abs(eta_hat).max() + 2 * np.abs(c["th"][-1]).max() <= ETA_MAX   # (η − s, s and −2s inside the range exp was measured on)
    d_eta = (gam(P, u) + gam(P + 1, U_LD)) * c["S_eta"] * SLACK + (u + U_LD) * np.abs(eta_hat.astype(LD)) + np.abs(c["X"]).astype(LD) @ Ew
    El, Eu, Ed = aux_link_bounds(c, eps, eta_hat, d_eta)
    if ll is not None:
        record_bound(f"loglik {key}", np.abs(ll.astype(LD) - c["ll"]), El)
    # the hierarchical part: c as hier_check wants it (θ without the row of s, ℓπ without its prior)
    ch = dict(c, th=c["th_h"], g=c["g"][:-1], lp=c["lp_h"])
    if not Gn:
        ch["tau"] = np.zeros((1, c["th"].shape[1]), dtype=LD)   # (hier_check takes a maximum over the groups' scales)
    with _patched(TG, "link_bounds", lambda cc, ep: (El, Eu)):
        if g is not None:
            with _patched(TH, "record_bound", record_bound):
                TH.hier_check(key, ch, eps, W=W, g=g[:-1])
        if lp is not None:
            # the prior of s: r = s − m (u|r|), (−½/A²)·r, ·r and the fma's rounding: ≤ 4u·½r²/A² + u·|ℓπ̂|; hier_check gets ℓπ̂ minus the
            # prior as the long-double reference has it, and this term is added to the difference's allowance below
            extra = 4 * u * c["aprior"] + u * np.abs(lp.astype(LD))

            def rb(k, err, bound):
                return record_bound(k, np.maximum(err - SLACK * extra, 0), bound)

            with _patched(TH, "record_bound", rb):
                TH.hier_check(key, ch, eps, W=W, lp=(lp.astype(LD) + c["aprior"]))
    if g is not None:
        dsum = np.abs(c["ds"]).sum(axis=0)
        Es = Ed.sum(axis=0) + (gam(n_obs, u) + gam(n_obs, U_LD)) * (np.abs(c["ds"]) + Ed).sum(axis=0)
        b = Es + (2 * u + U_LD) * np.abs(c["ra"]) * c["aia2"] + u * np.abs(g[-1].astype(LD)) + 8 * U_LD * (dsum + 1)
        record_bound(f"grad-dispersion {key}", np.abs(g[-1].astype(LD) - c["g"][-1]), SLACK * b)


def aux_emulate(c, defect=None):
    """the device's arithmetic on the host in the element type: fma chains (tests/host_ref) and the mirror's special functions in the
    element type.  `defect`: "ds_sign" gives ∂ℓ/∂s the wrong sign, "drop_block" sums partial_s without the last row block."""
    dt, P, groups, fam = c["dtype"].type, c["P"], c["groups"], c["fam"]
    f = TG.host_fma
    th = c["th"]
    Gn = len(groups)
    s = th[-1:]
    with np.errstate(over="ignore"):
        tau = np.exp(th[P:P + Gn])
        W = th[:P].copy()
        for k, (lo, hi, cen, _) in enumerate(groups):
            if not cen:
                W[lo:hi] = tau[k] * th[lo:hi]
        W = np.asfortranarray(W)
        eh = TG.chain(c["X"], W) + c["off"].reshape(-1, 1)
        y = c["y"].reshape(-1, 1)
        if fam == G.GAUSSIAN_IDENTITY_SIGMA:
            r = y - eh
            uu = np.exp(dt(-2) * s) * r
            ll = f(dt(-0.5) * uu, r, -s + 0 * r)
            ds = f(uu, r, np.full_like(r, -1))
        else:
            phi = np.exp(s) + 0 * eh
            d = eh - s
            e = np.exp(-np.abs(d))
            l = np.log1p(e)
            dd = dt(1) + e
            sig, nsig = np.where(d >= 0, dt(1) / dd, e / dd), np.where(d >= 0, e / dd, dt(1) / dd)
            sp, sn = np.where(d > 0, d, dt(0)) + l, np.where(d < 0, -d, dt(0)) + l
            yp = y + phi
            L, Psi = G.gamma_diffs(y + 0 * eh, phi, c["dtype"])
            ll = f(-y + 0 * eh, sn, f(-phi, sp, L))
            uu = f(-yp, sig, y + 0 * eh)
            ds = f(phi, Psi - sp, f(-yp, nsig, phi))
        assert ll.dtype == c["dtype"] and uu.dtype == c["dtype"] and ds.dtype == c["dtype"]
        if defect == "ds_sign":
            ds = -ds
        R = TG.grad_model(c["Xt"], np.asfortranarray(uu), np.zeros(P, dtype=c["dtype"]), W)   # fma(0, w, −Σ) = −Xᵀu
        lsum = _block_sums(ll)
        dblocks = _block_sums(ds, raw=True)
        if defect == "drop_block":
            dblocks = dblocks[:-1]
        dsum = dblocks.sum(axis=0, dtype=c["dtype"])
        lp, g = _in_dtype_finish(c, W, tau, R, lsum)
        ia2, m = dt(1.0 / (AUX_PRIOR[1] * AUX_PRIOR[1])), dt(AUX_PRIOR[0])
        ra = th[-1] - m
        lp = f((dt(-0.5) * ia2) * ra, ra, lp)
        gs = f(ra, np.full_like(ra, ia2), -dsum)
    return W, ll, lp, np.concatenate([g, gs.reshape(1, -1)]).astype(c["dtype"])


def _block_sums(a, raw=False):
    """Σ over each block of 64 rows, ascending, in the element type; then (unless `raw`) over the blocks"""
    n = a.shape[0]
    nb = (n + 63) // 64
    pad = np.zeros((nb * 64,) + a.shape[1:], dtype=a.dtype)
    pad[:n] = a
    blocks = np.add.accumulate(pad.reshape((nb, 64) + a.shape[1:]), axis=1, dtype=a.dtype)[:, -1]
    return blocks if raw else blocks.sum(axis=0, dtype=a.dtype)


def _in_dtype_finish(c, W, tau, R, lsum):
    """k_hglm_finish's arithmetic in the element type (test_glm_hier.hier_emulate's second half on given W, τ, R, Σℓ)"""
    dt, P, groups = c["dtype"].type, c["P"], c["groups"]
    f = TG.host_fma
    th, p = c["th"][:P + len(groups)], c["p"].reshape(-1, 1)
    lp = f(np.full_like(lsum, dt(-0.5)), TH.lane_sum(p * th[:P], th[:P]), lsum)
    g = np.empty((P + len(groups), th.shape[1]), dtype=c["dtype"])
    g[:P] = f(p, th[:P], R)
    for k, (lo, hi, cen, _) in enumerate(groups):
        sk, ia2, m = th[P + k], c["ia2"][k], dt(hi - lo)
        S, T = TH.lane_sum(th[lo:hi], th[lo:hi]), TH.lane_sum(R[lo:hi], W[lo:hi])
        e2 = np.exp(dt(2) * sk)
        h, hp = f(dt(-0.5) * e2, np.full_like(e2, ia2), sk), f(-e2, np.full_like(e2, ia2), np.ones_like(e2))
        if cen:
            q = np.exp(dt(-2) * sk)
            b = f(np.full_like(sk, -m), sk, (dt(-0.5) * q) * S)
            g[P + k] = f(-q, S, np.full_like(S, m)) - hp
            g[lo:hi] = f(q.reshape(1, -1), th[lo:hi], R[lo:hi])
        else:
            b = dt(-0.5) * S
            g[P + k] = T - hp
            g[lo:hi] = f(tau[k].reshape(1, -1), R[lo:hi], th[lo:hi])
        lp = lp + (h + b)
    return lp, g


# ------------------------------------------------------------------------------------------------
# CPU 1: the mirror's gradient
# ------------------------------------------------------------------------------------------------
GROUP_SETS = {"none": (), "centred": ((0, 2, True, 0.9),), "non-centred": ((1, 4, False, 1.4),)}


@pytest.mark.parametrize("fam", [3, 4], ids=list(AUXFAMS.values()))
@pytest.mark.parametrize("groups", list(GROUP_SETS))
@pytest.mark.parametrize("offset,prior", [(True, True), (False, False)])
def test_mirror_gradient_against_central_differences(fam, groups, offset, prior):
    """all D rows of ∇ℓπ against central differences of the mirror's own ℓπ (h = 1e-6: truncation ≈ 1e-11·|ℓπ‴|, rounding ≈ 1e-16·|ℓπ|/h)"""
    rs = np.random.default_rng(31 + fam)
    n, P = 37, 4
    grp = GROUP_SETS[groups]
    X = rs.normal(size=(n, P)) / 2
    y = rs.poisson(3.0, size=n).astype(float) if fam == 4 else rs.normal(size=n)
    p = rs.random(P) if prior else None
    if p is not None:
        for lo, hi, _, _ in grp:
            p[lo:hi] = 0
    off = 0.3 * rs.normal(size=n) if offset else None
    D = P + len(grp) + 1
    th = 0.4 * rs.normal(size=(D, 3))
    f = lambda t: G.hier_logdensity(fam, X, y, t, grp, off, p, aux_prior=AUX_PRIOR if prior else None)  # noqa: E731
    lp, g = f(th)
    assert g.shape == (D, 3)
    h = 1e-6
    for d in range(D):
        tp, tm = th.copy(), th.copy()
        tp[d] += h
        tm[d] -= h
        fd = (f(tp)[0] - f(tm)[0]) / (2 * h)
        np.testing.assert_allclose(g[d], fd, rtol=2e-7, atol=2e-7 * (1 + np.abs(lp).max()))
    if not grp:
        np.testing.assert_array_equal(G.logdensity(fam, X, y, th, off, p, aux_prior=AUX_PRIOR if prior else None)[0], lp)


# ------------------------------------------------------------------------------------------------
# CPU 2: lgamma_diff / digamma_diff against mpmath; the fixture; the recorded multiples
# ------------------------------------------------------------------------------------------------
def test_gamma_diffs_against_mpmath_and_fixture():
    """The fixture (grid and 60-digit references split into two doubles) is written if absent and verified otherwise; the mirror's
    worst errors in units of u·(|L| + y·|log(φ + y + 8)| + 1) and u·(|Ψ| + 1), u = ε/2 the unit roundoff, are within twice the multiples recorded in
    profiles/glm_aux_margins.json; y = 0 gives exact zeros; the long-double reference of this file agrees with mpmath to 1e-18."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 60
    phi, y = grid()
    rows = []
    for ph, yy in zip(phi, y):
        a, b = mp.mpf(float(ph)), mp.mpf(float(yy))
        L = mp.loggamma(a + b) - mp.loggamma(a)
        Ps = mp.digamma(a + b) - mp.digamma(a)
        Lh, Ph = float(L), float(Ps)
        rows.append((ph, yy, Lh, float(L - mp.mpf(Lh)), Ph, float(Ps - mp.mpf(Ph))))
    fx = np.array(rows, dtype=np.float64)
    if not os.path.exists(FIXTURE):
        os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
        np.save(FIXTURE, fx)
    stored = np.load(FIXTURE)
    assert stored.nbytes <= 200 * 1024 and stored.shape == fx.shape
    np.testing.assert_array_equal(stored[:, :2], fx[:, :2])
    np.testing.assert_allclose(stored[:, 2] + stored[:, 3], fx[:, 2] + fx[:, 3], rtol=1e-15, atol=1e-300)
    np.testing.assert_allclose(stored[:, 4] + stored[:, 5], fx[:, 4] + fx[:, 5], rtol=1e-15, atol=1e-300)
    Lr, Pr = fx[:, 2].astype(LD) + fx[:, 3].astype(LD), fx[:, 4].astype(LD) + fx[:, 5].astype(LD)
    Ll, Pl = gamma_diffs_ld(y, phi)
    uL, uP = special_units(y, phi, Lr, Pr)
    if np.finfo(LD).eps < 1e-18:   # (an 80-bit long double: the reference of §1 is itself held to the fixture)
        assert (np.abs(Ll - Lr) / uL).max() < 1e-17 and (np.abs(Pl - Pr) / uP).max() < 1e-17
    assert np.all(G.lgamma_diff(0.0, GRID_PHI) == 0) and np.all(G.digamma_diff(0.0, GRID_PHI) == 0)
    np.testing.assert_array_equal(G.lgamma_diff(y, phi), G.gamma_diffs(y, phi)[0])
    np.testing.assert_array_equal(G.digamma_diff(y, phi), G.gamma_diffs(y, phi)[1])
    got = dict(zip(("f64", "f32"), (special_multiples(lambda a, b, dt=dt: G.gamma_diffs(a, b, dt), dt) for dt in DTYPES)))
    MARGINS["special numpy-mirror"] = {k: {"lgamma_diff_multiple_of_u": v[0], "digamma_diff_multiple_of_u": v[1]} for k, v in got.items()}
    _dump_margins()
    print(MARGINS["special numpy-mirror"])
    rec = json.load(open(PROFILE))["numpy_mirror"]
    for k, (mL, mP) in got.items():
        assert mL <= 2 * rec[k]["lgamma_diff_multiple_of_u"], (k, mL, rec[k])
        assert mP <= 2 * rec[k]["digamma_diff_multiple_of_u"], (k, mP, rec[k])


# ------------------------------------------------------------------------------------------------
# CPU 3, 4: NB against scipy and its Poisson limit; the Gaussian at fixed s
# ------------------------------------------------------------------------------------------------
def test_negbinomial_pointwise_against_scipy_and_poisson_limit():
    rs = np.random.default_rng(3)
    n, P = 60, 3
    X = rs.normal(size=(n, P)) / 2
    y = rs.poisson(4.0, size=n).astype(float)
    th = np.concatenate([0.5 * rs.normal(size=(P, 5)), rs.normal(size=(1, 5))])
    eta, ll = G.pointwise("negbinomial_log", X, y, th)
    np.testing.assert_array_equal(eta, X @ th[:P])
    # the Poisson limit: φ = e²⁵ ≫ μ; NB − Poisson = O((y − μ)²/φ + μ·u·…)
    thp = th.copy()
    thp[-1] = 25.0
    _, llnb = G.pointwise("negbinomial_log", X, y, thp)
    _, llp = G.pointwise("poisson_log", X, y, thp[:P])
    np.testing.assert_allclose(llnb, llp, rtol=0, atol=1e-8)
    st = pytest.importorskip("scipy.stats")
    sp = pytest.importorskip("scipy.special")
    phi, mu = np.exp(th[-1]).reshape(1, -1), np.exp(eta)
    ref = st.nbinom.logpmf(y.reshape(-1, 1), phi, phi / (phi + mu)) + sp.gammaln(y + 1).reshape(-1, 1)
    np.testing.assert_allclose(ll, ref, rtol=1e-13, atol=1e-13)


def test_gaussian_sigma_at_fixed_s_is_the_gaussian_family():
    rs = np.random.default_rng(4)
    y, eta = rs.normal(size=(40, 1)), rs.normal(size=(40, 6))
    for s in (-1.25, 0.0, 0.75):
        ll, u, ds = G.link("gaussian_identity_sigma", y, eta, s=np.full((1, 6), s))
        ll2, u2 = G.link("gaussian_identity", y, eta, scale=np.exp(-2.0 * s))
        np.testing.assert_array_equal(u, u2)
        assert np.all(np.abs((ll + s) - ll2) <= 4 * 2.0 ** -53 * (np.abs(ll2) + abs(s)))   # (−s is added, then taken away: two roundings)
        assert np.all(np.abs(ds - (u * (y - eta) - 1)) <= 4 * 2.0 ** -53 * (1 + np.abs(ds)))
    with pytest.raises(ValueError, match="needs s"):
        G.link("negbinomial_log", y, eta)
    assert len(G.link("negbinomial_log", np.abs(y), eta, s=np.zeros((1, 6)))) == 3


# ------------------------------------------------------------------------------------------------
# CPU 5: constructor, header, bindings, Julia, exported symbols, scratch, the checker
# ------------------------------------------------------------------------------------------------
def test_constructor_and_refusals():
    rs = np.random.default_rng(2)
    X, y = rs.normal(size=(12, 6)), rs.poisson(2.0, size=12).astype(float)
    t = A.GLMTarget(X, y, family="negbinomial_log", aux_prior=(0.5, 2.0), prior_scale=2.0)
    assert (t.D, t.P, t.n_obs, t.family, t.kind, t.aux, t.aux_prior) == (7, 6, 12, G.NEGBINOMIAL_LOG, capi.TARGET_GLM, True, (0.5, 2.0))
    th = 0.3 * rs.normal(size=(7, 2))
    want = G.logdensity(4, X, y, th, None, t.prior_prec, aux_prior=(0.5, 2.0))
    np.testing.assert_array_equal(t.logdensity(th)[0], want[0])
    np.testing.assert_array_equal(t.logdensity(th)[1], want[1])
    np.testing.assert_array_equal(t.dispersion(th), np.exp(th[-1]))
    assert A.GLMTarget(X, y, family="gaussian_identity_sigma").aux_prior == (0.0, 1.0)
    h = A.HierGLMTarget(X, y, [A.CoefGroup(1, 3), A.CoefGroup(3, 6, centered=True, scale=2.5)], family="gaussian_identity_sigma", aux_prior=(0.0, 1.5))
    assert (h.D, h.P, len(h.groups)) == (9, 6, 2)
    th = 0.3 * rs.normal(size=(9, 2))
    want = G.hier_logdensity(3, X, y, th, ((1, 3, False, 1.0), (3, 6, True, 2.5)), None, h.prior_prec, aux_prior=(0.0, 1.5))
    np.testing.assert_array_equal(h.logdensity(th)[0], want[0])
    beta, tau = h.coefficients(th)
    assert beta.shape == (6, 2) and tau.shape == (2, 2)
    A.Hamiltonian(A.UnitEuclideanMetric(9), h)
    with pytest.raises(A.ArgumentError):
        A.Hamiltonian(A.UnitEuclideanMetric(8), h)
    assert A.GLMTarget(X, y, family="poisson_log").D == 6   # (the legacy families are as they were)
    for bad in (lambda: A.GLMTarget(X, y, family="negbinomial_log", aux_prior=(0.0, 0.0)), lambda: A.GLMTarget(X, y, family="negbinomial_log", aux_prior=(0.0, -1.0)),
                lambda: A.GLMTarget(X, y, family="negbinomial_log", aux_prior=(0.0, np.inf)), lambda: A.GLMTarget(X, y, family="negbinomial_log", aux_prior=(np.nan, 1.0)),
                lambda: A.GLMTarget(X, y, family="poisson_log", aux_prior=(0.0, 1.0)), lambda: A.GLMTarget(X, y, family="gaussian_identity_sigma", scale=2.0),
                lambda: A.HierGLMTarget(X, y, [], family="bernoulli_logit", aux_prior=(0.0, 1.0)), lambda: t.__class__(X, y, family="negbinomial").D,
                lambda: A.GLMTarget(X, y, family="poisson_log").dispersion(th)):
        with pytest.raises(A.ArgumentError):
            bad()
    for bad in (lambda: G.logdensity(4, X, y, np.zeros((6, 2))), lambda: G.logdensity(1, X, y, np.zeros((7, 2)), aux_prior=(0.0, 1.0)),
                lambda: G.check_aux_prior((0.0, 0.0))):
        with pytest.raises(ValueError):
            bad()


def header_prototypes():
    src = open(os.path.join(ROOT, "include", "ahmc_glm_aux.h"), encoding="utf-8").read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(int32_t)\s+(ahmc_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        params = " ".join(m.group(3).split())
        protos[m.group(2)] = [] if params in ("", "void") else [p.strip() for p in params.split(",")]
    return protos, src


def test_header_and_bindings_agree():
    protos, src = header_prototypes()
    assert set(protos) == set(capi.GLM_AUX_SIGNATURES) == {"ahmc_glm_aux_version", "ahmc_glm_aux_set_target", "ahmc_glm_aux_get_target", "ahmc_glm_dispersion"}
    assert not set(capi.GLM_AUX_SIGNATURES) & (set(capi.GLM_SIGNATURES) | set(capi.HGLM_SIGNATURES))
    ct = {"int64_t*": C.POINTER(C.c_int64), "int32_t*": C.POINTER(C.c_int32), "double*": C.POINTER(C.c_double), "int64_t": C.c_int64,
          "int32_t": C.c_int32, "double": C.c_double}
    for name, params in protos.items():
        res, args = capi.GLM_AUX_SIGNATURES[name]
        assert res is C.c_int32 and len(args) == len(params), name
        for p, a in zip(params, args):
            typ = p.rsplit(" ", 1)[0].replace("const ", "").replace(" ", "")
            if typ in ("void*", "ahmc_ctx*"):
                assert a is C.c_void_p, (name, p)
            else:
                assert a is ct[typ], (name, p)
    # the arguments of ahmc_hglm_set_target without scale, then the prior
    hier = [p.split()[-1] for p in TH.header_prototypes()[0]["ahmc_hglm_set_target"]]
    assert [p.split()[-1] for p in protos["ahmc_glm_aux_set_target"]] == [a for a in hier if a != "scale"] + ["aux_loc", "aux_scale"]
    assert re.search(r"#define AHMC_GLM_AUX_VERSION (\d+)", src).group(1) == str(capi.AHMC_GLM_AUX_VERSION) == "1"
    assert re.search(r"#define AHMC_GLM_AUX_MAX_GROUPS (\d+)", src).group(1) == str(capi.GLM_AUX_MAX_GROUPS) == str(G.HGLM_MAX_GROUPS - 1)
    glm_h = open(os.path.join(ROOT, "include", "ahmc_glm.h"), encoding="utf-8").read()
    m = re.search(r"enum \{ AHMC_GLM_GAUSSIAN_IDENTITY_SIGMA = (\d+), AHMC_GLM_NEGBINOMIAL_LOG = (\d+) \}", glm_h)
    assert tuple(int(x) for x in m.groups()) == (capi.GLM_GAUSSIAN_IDENTITY_SIGMA, capi.GLM_NEGBINOMIAL_LOG) == (G.GAUSSIAN_IDENTITY_SIGMA, G.NEGBINOMIAL_LOG) == (3, 4)
    assert (G.FAMILIES["gaussian_identity_sigma"], G.FAMILIES["negbinomial_log"]) == (3, 4)
    hip_h = open(os.path.join(ROOT, "include", "ahmc_hip.h"), encoding="utf-8").read()
    assert "glm" not in hip_h.lower() and re.search(r"#define AHMC_ABI_VERSION (\d+)", hip_h).group(1) == "6"
    from ahmc_amd import build as B
    assert "ahmc_glm_aux.h" in open(B.__file__, encoding="utf-8").read()


def test_julia_ccalls_match_the_header():
    protos, _ = header_prototypes()
    src = open(os.path.join(ROOT, "julia", "AdvancedHMCMI355XGLMAux.jl"), encoding="utf-8").read()
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
    assert 'include("AdvancedHMCMI355XGLMAux.jl")' in ext and "ahmc_glm_aux_set_target" not in ext and "ahmc_glm_dispersion" not in ext
    assert ext.index('include("AdvancedHMCMI355XGLMHier.jl")') < ext.index('include("AdvancedHMCMI355XGLMAux.jl")')


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="needs llvm-objdump")
def test_library_exports_and_kernels_without_scratch():
    """every entry point is in the dynamic symbol table (read without loading the library); the four new instantiations of k_glm_eta
    the finishing kernel and k_glm_exp_row are in the code object with no private segment and no VGPR spill (scripts/kernel_meta.py)"""
    from ahmc_amd import build as B

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_meta
    finally:
        sys.path.pop(0)
    assert os.path.exists(B.OUT), "build() first"
    exported = {l.split()[-1] for l in subprocess.run(["nm", "-D", "--defined-only", B.OUT], capture_output=True, text=True, check=True).stdout.splitlines() if l.strip()}
    assert set(capi.GLM_AUX_SIGNATURES) <= exported, set(capi.GLM_AUX_SIGNATURES) - exported
    meta = kernel_meta.kernel_meta(B.OUT)
    names = subprocess.run(["c++filt"], input="\n".join(k["name"] for k in meta), capture_output=True, text=True, check=True).stdout.splitlines()
    want = [f"k_glm_eta<{t}, {f}, {bn}>" for t in ("float", "double") for f in (3, 4) for bn in (64, 16)]
    want += [f"k_{w}<{t}>" for w in ("hglm_finish_aux", "glm_exp_row") for t in ("float", "double")]
    found = {}
    for k, dn in zip(meta, names):
        for w in want:
            if dn.startswith(f"void ahmc::{w}("):
                found[w] = k
    assert sorted(found) == sorted(want), sorted(set(want) - set(found))
    for w, k in found.items():
        assert k["private_segment_fixed_size"] == 0, (w, k)
        assert k.get("vgpr_spill_count", 0) == 0, (w, k)


def test_cpu_checker_refuses_the_target(oracle):
    assert oracle.has_glm_aux is False
    rs = np.random.default_rng(5)
    t = A.GLMTarget(rs.normal(size=(7, 4)), rs.poisson(2.0, size=7).astype(float), family="negbinomial_log")
    with pytest.raises(A.UnsupportedError, match="ahmc_glm_aux.h"):
        A.Engine(A.Hamiltonian(A.UnitEuclideanMetric(5), t), 3, lib=oracle)
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric(5), A.IsoGaussian(5)), 3, lib=oracle)
    with pytest.raises(A.UnsupportedError, match="ahmc_glm_aux.h"):
        e.glm_dispersion()
    with pytest.raises(A.UnsupportedError, match="ahmc_glm_aux.h"):
        e.set_target(t)
    e.close()


# ------------------------------------------------------------------------------------------------
# CPU 6: the bounds on a host emulation, and two planted defects
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", [3, 4], ids=list(AUXFAMS.values()))
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_bounds_hold_for_a_host_emulation_and_catch_two_defects(fam, dtype):
    """The device's arithmetic emulated on the host in the element type passes every assertion of §1; with ∂ℓ/∂s given the wrong sign,
    and with partial_s summed without its last row block, the assertion on g[D−1] fails: the bound can fail."""
    eps = mirror_eps(dtype)
    for n_obs, P, groups in VALUE_CASES:
        c = acase(n_obs, P, groups, fam, 5, np.dtype(dtype).name)
        key = f"host-emulation {AUXFAMS[fam]} {np.dtype(dtype).name} ({n_obs}, {P}, {len(groups)})"
        W, ll, lp, g = aux_emulate(c)
        aux_check(key, c, eps, W=W, ll=ll, lp=lp, g=g)
        for defect in ("ds_sign", "drop_block"):
            g_bad = aux_emulate(c, defect)[3]
            with pytest.raises(AssertionError, match="grad-dispersion planted"):
                aux_check("planted " + key, c, eps, W=W, g=g_bad)
        for k in [k for k in MARGINS if "planted " in k]:
            del MARGINS[k]
    _dump_margins()


# ------------------------------------------------------------------------------------------------
# §4's inputs, and CPU 7: their precondition on the oracle alone
# ------------------------------------------------------------------------------------------------
GROUPS2 = ((5, 11, True, 1.0), (11, 17, False, 1.0))
# name: (n_obs, P, groups, family, seed)
PARITY = {"negbinomial (130, 17 + 0 + 1)": (130, 17, (), "negbinomial_log", 1),
          "negbinomial (130, 17 + 2 + 1)": (130, 17, GROUPS2, "negbinomial_log", 1),
          "gaussian-sigma (130, 17 + 0 + 1)": (130, 17, (), "gaussian_identity_sigma", 1),
          "gaussian-sigma (130, 17 + 2 + 1)": (130, 17, GROUPS2, "gaussian_identity_sigma", 1)}
DENSE_CASE = "negbinomial (130, 17 + 2 + 1)"
WIDE = (70, 4200, ((10, 200, False, 1.0),), "negbinomial_log", 1)


def aux_parity_inputs(n_obs, P, groups, family, seed, N=300):
    Gn = len(groups)
    rs = np.random.default_rng([n_obs, P, Gn, seed, G.family_code(family)])
    X = rs.normal(size=(n_obs, P)) / np.sqrt(P)
    eta = X @ rs.normal(size=P)
    if family == "negbinomial_log":
        y = rs.negative_binomial(3.0, 3.0 / (3.0 + np.exp(eta))).astype(np.float64)
    else:
        y = eta + 0.7 * rs.normal(size=n_obs)
    p = np.ones(P)
    for lo, hi, _, _ in groups:
        p[lo:hi] = 0
    D = P + Gn + 1
    minv = np.asfortranarray(0.5 + rs.random((D, N)))
    th0 = 0.5 * rs.normal(size=(D, N))
    th0[-1] *= 0.6
    eps = 0.1 * (0.7 + 0.6 * rs.random(N))
    t = A.HierGLMTarget(X, y, groups, family=family, prior_prec=p, aux_prior=(0.0, 1.0)) if groups else A.GLMTarget(X, y, family=family, prior_prec=p, aux_prior=(0.0, 1.0))
    return t, minv, th0, eps


def dense_metric(D):
    rs = np.random.default_rng(190)
    Q, _ = np.linalg.qr(rs.normal(size=(D, D)))
    Mi = (Q * np.linspace(0.6, 2.0, D)) @ Q.T
    return A.DenseEuclideanMetric(np.asfortranarray((Mi + Mi.T) / 2))


@pytest.mark.parametrize("name", list(PARITY) + ["dense", "wide"])
def test_parity_precondition_on_the_oracle_alone(oracle, name):
    """On §4's inputs no decision of the oracle (running the mirror as a host kernel) comes within the suite's bound for float64 of a
    tie, at any step of the sequence and for any chain: the GPU comparison may demand exact agreement of every chain."""
    if name == "wide":
        t, _, th0, eps = aux_parity_inputs(*WIDE, N=8)
        o = TH.oracle_engine(oracle, t, A.UnitEuclideanMetric(th0.shape), 8)
        smallest, n_div = TG.parity_sequence(o, None, th0, eps, "glm-aux wide", nuts_depth=5, full=False)
    else:
        t, minv, th0, eps = aux_parity_inputs(*PARITY[DENSE_CASE if name == "dense" else name])
        o = TH.oracle_engine(oracle, t, dense_metric(t.D) if name == "dense" else A.DiagEuclideanMetric(minv), th0.shape[1])
        smallest, n_div = TG.parity_sequence(o, None, th0, eps, f"glm-aux {name}")
    MARGINS[f"oracle-margin {name}"] = {"smallest_decision_margin": smallest, "divergent_chains_max": n_div}
    _dump_margins()
    o.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
_STATE = {}


@pytest.fixture(scope="module")
def probe_a(hip):
    import torch

    from ahmc_amd import build as B
    from ahmc_amd.hipmod import Module

    torch.cuda.init()
    if "probe_a" not in _STATE:
        _STATE["probe_a"] = Module(B.build_probe_object(PROBE_A))
    return _STATE["probe_a"]


def device_eps(probe, probe_a, dtype):  # noqa: F811
    """ε_exp, ε_log1p (tests/device_probe/glm.hip) and twice the device's special-function multiples (tests/device_probe/glm_aux.hip)"""
    key = ("eps", np.dtype(dtype).name)
    if key not in _STATE:
        import torch

        def fn(y, phi):
            y_d, p_d = TG.dev(y), TG.dev(phi)
            L_d, P_d = torch.empty_like(y_d), torch.empty_like(y_d)
            probe_a.launch("glm_aux_probe_gamma_diffs_" + TG._sfx(dtype), (y.size + 255) // 256, 256, y_d, p_d, L_d, P_d, np.int64(y.size))
            return TG.host(L_d, y.shape), TG.host(P_d, y.shape)

        eps = dict(TG.device_eps(probe, dtype))
        mL, mP = special_multiples(fn, dtype)
        eps["L"], eps["Psi"] = 2 * mL, 2 * mP
        MARGINS[f"special device {np.dtype(dtype).name}"] = {"lgamma_diff_multiple_of_u": mL, "digamma_diff_multiple_of_u": mP}
        _dump_margins()
        print(MARGINS[f"special device {np.dtype(dtype).name}"])
        _STATE[key] = eps
    return _STATE[key]


def aux_target(c):
    kw = dict(family=c["fam"], prior_prec=c["p"], offset=c["off"], aux_prior=AUX_PRIOR)
    return A.HierGLMTarget(c["X"], c["y"], c["groups"], **kw) if c["groups"] else A.GLMTarget(c["X"], c["y"], **kw)


def aux_engine(hip, c, cols=None, metric=None, seed=7):
    th = c["th"] if cols is None else c["th"][:, cols]
    D, N = th.shape
    e = A.Engine(A.Hamiltonian(metric or A.UnitEuclideanMetric((D, N)), aux_target(c)), N, dtype=c["dtype"],
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
    return eta, ll, W, tau, e.glm_dispersion(), z.lp.value.copy(), z.lp.gradient.copy()


NAMES = ("eta", "loglik", "W", "tau", "dispersion", "lp", "grad")


# ---- §1 ----
@pytest.mark.gpu
@pytest.mark.parametrize("fam", [3, 4], ids=list(AUXFAMS.values()))
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_values_against_exact_references(hip, probe, probe_a, fam, dtype):  # noqa: F811
    """η bit for bit the k-ordered fma chain on the device's own W (W = θ[:P] exactly without groups); ℓ (ahmc_glm_pointwise), ℓπ, every
    row of g and g[D−1] inside the bounds of the module docstring, fed by the two probes; the target's getters.  The gradient product bit
    for bit against its fma-chain model needs the device's U, which only the probe launch exposes: test_new_kernels_on_a_chain_list."""
    eps = device_eps(probe, probe_a, dtype)
    for n_obs, P, groups in VALUE_CASES:
        c = acase(n_obs, P, groups, fam, 300, np.dtype(dtype).name)
        key = f"{AUXFAMS[fam]} {np.dtype(dtype).name} ({n_obs}, {P}, {len(groups)})"
        e = aux_engine(hip, c)
        fam_got, n_got, sc = C.c_int32(), C.c_int64(), C.c_double()
        e._call("ahmc_get_target_glm", C.byref(fam_got), C.byref(n_got), C.byref(sc))
        assert (fam_got.value, n_got.value, sc.value) == (fam, n_obs, 1.0)
        nc, ng = C.c_int64(), C.c_int32()
        e._call("ahmc_hglm_get_target", C.byref(nc), C.byref(ng), None, None, None, None)
        assert (nc.value, ng.value) == (P, len(groups))
        m, a = C.c_double(), C.c_double()
        e._call("ahmc_glm_aux_get_target", C.byref(m), C.byref(a))
        assert (m.value, a.value) == AUX_PRIOR
        eta, ll, W, tau, phi, lp, g = evaluate(e)
        record_bits(f"eta {key}", eta, TG.chain(c["X"], W) + c["off"].reshape(-1, 1))
        if not groups:
            record_bits(f"W {key}", W, np.asfortranarray(c["th"][:P]))
        aux_check(key, c, eps, W=W, phi=phi, ll=ll, lp=lp, g=g)
        e.close()


def _ptr(t, elems):
    """the device pointer `elems` elements into tensor t"""
    return C.c_void_p(t.data_ptr() + elems * t.element_size())


@pytest.mark.gpu
@pytest.mark.parametrize("fam", [3, 4], ids=list(AUXFAMS.values()))
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_new_kernels_on_a_chain_list(hip, probe_a, fam, dtype):
    """k_glm_eta<T, 3 | 4, BN> (both tile shapes) and k_hglm_finish_aux launched from the probe, on all chains and on a chain list —
    every third chain, reversed.  The listed columns of U, partial, partial_s, η, ℓ, ℓπ and every row of g (g[D−1] included) carry the
    bits of the full launch; the columns off the list keep their NaN fill; both tile shapes give the same bits.  The full launch is the
    engine's: η and ℓ equal ahmc_glm_pointwise; and, without groups, rows 0 .. P − 1 of the engine's g equal fma(p, θ, R) with R the
    slice-ordered fma-chain model of −Xᵀ·U applied to this launch's U, bit for bit (the gradient product of §1)."""
    import torch

    dtype = np.dtype(dtype)
    tch = TG.TCH[dtype]
    N = 300
    idx = np.arange(N)[::3][::-1].copy()
    rest = np.setdiff1d(np.arange(N), idx)
    fin = f"_ZN4ahmc17k_hglm_finish_auxI{tch}EEvPKT_S3_S3_S3_S3_S3_PKNS_7HglmTabIS1_EEPS1_S8_iiillPKiiS1_S1_"
    for n_obs, P, groups in VALUE_CASES:
        c = acase(n_obs, P, groups, fam, N, dtype.name)
        Gn, D, nrb = len(groups), P + len(groups) + 1, (n_obs + 63) // 64
        key = f"{AUXFAMS[fam]} {dtype.name} ({n_obs}, {P}, {Gn})"
        e = aux_engine(hip, c)
        z = e.phasepoint()
        eta_e, ll_e = e.glm_pointwise()
        W, _ = e.hglm_coefficients()
        g_e = z.lp.gradient.copy()
        e.close()
        rs = np.random.default_rng([n_obs, P, 98])
        Rm = np.asfortranarray(rs.normal(size=(P, N)), dtype=dtype)
        X_d, y_d, off_d, W_d, th_d, p_d, R_d = (TG.dev(a) for a in (c["X"], c["y"], c["off"], np.asfortranarray(W), c["th"], c["p"], Rm))
        tab_d = torch.from_numpy(TH.table_bytes(c)).cuda()
        one, loc, ia2 = dtype.type(1.0), dtype.type(AUX_PRIOR[0]), dtype.type(1.0 / (AUX_PRIOR[1] * AUX_PRIOR[1]))

        def nan(*shape):
            return torch.full((int(np.prod(shape)),), float("nan"), dtype=th_d.dtype, device="cuda")

        out = {}
        for bn in (64, 16):
            eta_k = f"_ZN4ahmc9k_glm_etaI{tch}Li{fam}ELi{bn}EEEvPKT_S3_S3_S1_S3_PS1_S4_iillPKiS4_S4_S3_lS4_"
            for which, lst in (("all", None), ("list", idx)):
                n = N if lst is None else lst.size
                idx_d = TG.NULL if lst is None else TG.dev(lst)
                U_d, part_d, ps_d, eta_d, ll_d, lp_d, g_d = nan(n_obs, N), nan(nrb, N), nan(nrb, N), nan(n_obs, N), nan(n_obs, N), nan(N), nan(D, N)
                grid = (nrb * (((n + 63) // 64 + 7) // 8 * 8),) if bn == 64 else (nrb, (n + 15) // 16)
                probe_a.launch(eta_k, grid, 256, X_d, y_d, off_d, one, W_d, U_d, part_d, n_obs, int(P), np.int64(n), np.int64(N), idx_d, eta_d, ll_d,
                               _ptr(th_d, D - 1), np.int64(D), ps_d)
                # (partial[row block][chain]: the chain is the fast index)
                res = [TG.host(U_d, (n_obs, N)), TG.host(part_d, (N, nrb)).T, TG.host(ps_d, (N, nrb)).T, TG.host(eta_d, (n_obs, N)), TG.host(ll_d, (n_obs, N))]
                # (the finishing kernel reads partial and partial_s of the listed columns only; the list launch gets the full ones, so
                # that a NaN in ℓπ or g can only mean "not written")
                pin, psin = (part_d, ps_d) if lst is None else (TG.dev(out[(bn, "all")][1].T), TG.dev(out[(bn, "all")][2].T))
                probe_a.launch(fin, (n + 3) // 4, 256, pin, psin, R_d, W_d, p_d, th_d, tab_d, lp_d, g_d, int(nrb), int(P), int(Gn), np.int64(n), np.int64(N),
                               idx_d, 1, loc, ia2)
                out[(bn, which)] = res + [TG.host(lp_d, (1, N)), TG.host(g_d, (D, N))]
        names = ("U", "partial", "partial_s", "eta", "loglik", "lp", "grad")
        for bn in (64, 16):
            for name, a, b, b64 in zip(names, out[(bn, "list")], out[(bn, "all")], out[(64, "all")]):
                assert np.isfinite(b).all(), (name, bn)
                record_bits(f"chain-list-{name}-bn{bn} {key}", a[:, idx], b[:, idx])
                assert np.isnan(a[:, rest]).all(), (name, bn)
                record_bits(f"tile-shapes-{name} {key}", b, b64)
        U_full = out[(64, "all")][0]
        record_bits(f"probe-eta-is-the-engine's {key}", out[(64, "all")][3], eta_e)
        record_bits(f"probe-loglik-is-the-engine's {key}", out[(64, "all")][4], ll_e)
        if not groups:
            R = TG.grad_model(c["Xt"], np.asfortranarray(U_full), np.zeros(P, dtype=dtype), np.asfortranarray(W))
            record_bits(f"gradient-product {key}", g_e[:P], TG.host_fma(c["p"].reshape(-1, 1), np.ascontiguousarray(c["th"][:P]), R))


# ---- §2 ----
@pytest.mark.gpu
@pytest.mark.parametrize("fam", [3, 4], ids=list(AUXFAMS.values()))
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_layout_independence(hip, fam, dtype):
    """the evaluation and three NUTS transitions: either tile shape forced == the default rule; engines over chain blocks == one
    engine.  (The chain list `idx` itself: test_new_kernels_on_a_chain_list.)"""
    N = 130
    n_obs, P, groups = VALUE_CASES[1]
    c = acase(n_obs, P, groups, fam, N, np.dtype(dtype).name)
    tag = f"{AUXFAMS[fam]} {np.dtype(dtype).name}"
    whole = aux_engine(hip, c, seed=A.PhiloxRNG(17))
    ev = evaluate(whole)
    whole.run(TG.nuts_kernel(N, eps=0.02), 3)
    th_w, st_w = whole.theta(), whole.stats()
    whole.close()
    assert st_w["n_steps"].sum() > 3 * N
    for which in ("small", "big"):
        e = aux_engine(hip, c, seed=A.PhiloxRNG(17))
        with TG.tile_shape(which):
            for name, a, b in zip(NAMES, evaluate(e), ev):
                record_bits(f"tile-shape-{which}-{name} {tag}", a, b)
            e.run(TG.nuts_kernel(N, eps=0.02), 3)
            e.sync()
        record_bits(f"tile-shape-run-{which} {tag}", e.theta(), th_w)
        np.testing.assert_array_equal(e.stats()["n_steps"], st_w["n_steps"])
        e.close()
    rs = np.random.default_rng(N)
    cuts = np.concatenate([[0], np.sort(rs.choice(np.arange(1, N), size=3, replace=False)), [N]])
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        cols = np.arange(lo, hi)
        e = aux_engine(hip, c, cols=cols, seed=A.PhiloxRNG(17, chain_offset=int(lo)))
        for name, a, b in zip(NAMES, evaluate(e), ev):
            record_bits(f"blocks-{name} {tag}", a, b[..., cols])
        e.run(TG.nuts_kernel(hi - lo, eps=0.02), 3)
        record_bits(f"blocks-theta {tag}", e.theta(), th_w[:, cols])
        np.testing.assert_array_equal(e.stats()["n_steps"], st_w["n_steps"][cols])
        e.close()


# ---- §3 ----
@pytest.mark.gpu
@pytest.mark.parametrize("fam", [3, 4], ids=list(AUXFAMS.values()))
def test_checkpoint_resume_and_bulk_equals_stepwise(hip, fam):
    N = 70
    n_obs, P, groups = VALUE_CASES[1]
    c = acase(n_obs, P, groups, fam, N, "float64")
    D = c["th"].shape[0]
    kern = TG.nuts_kernel(N, eps=0.02)

    def engine(adapt=True):
        e = aux_engine(hip, c, metric=A.DiagEuclideanMetric((D, N)))
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


# ---- §4 ----
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PARITY))
def test_against_oracle(hip, oracle, name):
    """the HIP engine on the target against the oracle on the mirror as a host kernel: static HMC, two NUTS transitions,
    find_good_stepsize, a bulk run of three — every discrete statistic of every chain"""
    t, minv, th0, eps = aux_parity_inputs(*PARITY[name])
    N = th0.shape[1]
    o = TH.oracle_engine(oracle, t, A.DiagEuclideanMetric(minv), N)
    g = A.Engine(A.Hamiltonian(A.DiagEuclideanMetric(minv), t), N, rng=A.PhiloxRNG(8), lib=hip)
    TG.parity_sequence(o, g, th0, eps, f"glm-aux {name}")
    g.close()
    o.close()


@pytest.mark.gpu
def test_against_oracle_dense_metric(hip, oracle):
    t, _, th0, eps = aux_parity_inputs(*PARITY[DENSE_CASE])
    N = th0.shape[1]
    o = TH.oracle_engine(oracle, t, dense_metric(t.D), N)
    g = A.Engine(A.Hamiltonian(dense_metric(t.D), t), N, rng=A.PhiloxRNG(8), lib=hip)
    TG.parity_sequence(o, g, th0, eps, "glm-aux dense")
    g.close()
    o.close()


@pytest.mark.gpu
def test_against_oracle_wide(hip, oracle):
    """a wide context (D = 4200 + 1 + 1 > 4096) with n_obs = 70, N = 8, two NUTS transitions at max_depth 5"""
    t, _, th0, eps = aux_parity_inputs(*WIDE, N=8)
    D = t.D
    o = TH.oracle_engine(oracle, t, A.UnitEuclideanMetric((D, 8)), 8)
    g = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((D, 8)), t), 8, rng=A.PhiloxRNG(8), lib=hip)
    assert g.info("wide") and D > 4096
    TG.parity_sequence(o, g, th0, eps, "glm-aux wide", nuts_depth=5, full=False)
    g.close()
    o.close()


# ---- §5 ----
@pytest.mark.gpu
def test_posterior_against_ask_tell(hip):
    """Simulated NB2 counts, (n_obs, P) = (200, 3), φ = 2.5; N = 256, StanHMCAdaptor, 100 adapting + 60 kept transitions: the target
    and ExternalTarget(t.logdensity) on the same engine — R-hat < 1.05 in every dimension for both; the pooled means of the
    coefficients, of s and of φ within 5·√(mcse₁² + mcse₂²)"""
    n_obs, P, N = 200, 3, 256
    rs = np.random.default_rng(47)
    X = np.concatenate([np.ones((n_obs, 1)), rs.normal(size=(n_obs, P - 1))], axis=1)
    mu = np.exp(X @ np.array([1.0, 0.5, -0.4]))
    y = rs.negative_binomial(2.5, 2.5 / (2.5 + mu)).astype(np.float64)
    t = A.GLMTarget(X, y, family="negbinomial_log", prior_scale=3.0, aux_prior=(0.0, 1.5))
    D = t.D
    assert D == 4
    th0 = 0.1 * rs.normal(size=(D, N))
    stats = {}
    for name, target in (("glm-aux", t), ("external", A.ExternalTarget(D, t.logdensity))):
        e = A.Engine(A.Hamiltonian(A.DiagEuclideanMetric((D, N)), target), N, rng=A.PhiloxRNG(5), lib=hip)
        kern = TG.nuts_kernel(N, eps=0.1, depth=8)
        e.set_integrator(kern.tau.integrator)
        e.set_position(th0)
        e.adaptor_init(A.StanHMCAdaptor(A.MassMatrixAdaptor(A.DiagEuclideanMetric((D, N))), A.StepSizeAdaptor(0.8, kern.tau.integrator)))
        e.run(kern, 100, n_adapts=100)
        draws = np.empty((60, D + 1, N))
        for i in range(60):
            e.transition(kern)
            draws[i, :D] = e.theta()
            draws[i, D] = np.exp(draws[i, D - 1])   # φ as a quantity of its own
        stats[name] = A.summarystats(draws)
        if name == "glm-aux":
            np.testing.assert_allclose(e.glm_dispersion(draws[-1, :D]), draws[-1, D], rtol=1e-12)
        e.close()
    diff = np.abs(stats["glm-aux"]["mean"] - stats["external"]["mean"])
    tol = 5 * np.sqrt(stats["glm-aux"]["mcse"] ** 2 + stats["external"]["mcse"] ** 2)
    MARGINS["posterior"] = {"rhat_glm_aux": float(stats["glm-aux"]["rhat"].max()), "rhat_external": float(stats["external"]["rhat"].max()),
                            "mean_difference_over_tolerance": float((diff / tol).max()), "mean": stats["glm-aux"]["mean"].tolist()}
    _dump_margins()
    print(MARGINS["posterior"])
    for name in stats:
        assert np.all(stats[name]["rhat"] < 1.05), (name, stats[name]["rhat"])
    assert np.all(diff < tol), (diff / tol)


# ---- §6 ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_dispersion_of_draws_and_legacy_families(hip, dtype):
    """glm_dispersion of host and device draws == the device's exp of the last row (bit for bit among themselves, within 16 u of
    exp); a plain GLMTarget of family 0 and 1 runs exactly the chains of the same density served through ask / tell by the untouched
    mirror, family 2 the same chains but for near ties"""
    c = acase(*VALUE_CASES[0], 4, 40, np.dtype(dtype).name)
    e = aux_engine(hip, c)
    phi = e.glm_dispersion()
    record_bits(f"dispersion-host-draws {np.dtype(dtype).name}", e.glm_dispersion(c["th"][:, :7]), phi[:7])
    th_d = TG.dev(c["th"])
    record_bits(f"dispersion-device-draws {np.dtype(dtype).name}", e.glm_dispersion(int(th_d.data_ptr()), n_cols=40), phi)
    np.testing.assert_allclose(phi.astype(np.float64), np.exp(c["th"][-1].astype(np.float64)), rtol=16 * float(U[np.dtype(dtype)]))
    e.close()
    if np.dtype(dtype) != np.float64:
        return
    # the legacy families through the untouched mirror path (ask / tell on the same engine), on test_glm_target's parity inputs, whose
    # decision margins test_glm_target.test_parity_precondition_on_the_oracle_alone proves for exactly this sequence (seed 8: static HMC,
    # then two NUTS transitions, each from the mirror run's θ): no chain may differ.  The Gaussian family has no proven inputs there: its
    # chains may part at a near tie, and what holds its instantiation to its bits is test_glm_target's bit-for-bit tests.
    for n_obs, Dm, family in ((130, 17, "bernoulli_logit"), (65, 65, "poisson_log")):
        X, y, p, minv, th0, eps = TG.parity_inputs(n_obs, Dm, family)
        N = th0.shape[1]
        t = A.GLMTarget(X, y, family=family, prior_prec=p)
        lf = A.Leapfrog(eps)
        nuts = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=6)))
        hmc = A.HMCKernel(A.Trajectory(A.EndPointTS, lf, A.FixedNSteps(4)))
        es = [A.Engine(A.Hamiltonian(A.DiagEuclideanMetric(minv), target), N, rng=A.PhiloxRNG(8), lib=hip) for target in (t, A.ExternalTarget(Dm, t.logdensity))]
        for g in es:
            g.set_integrator(lf)
            g.set_position(th0)
        for k in (hmc, nuts, nuts):
            for g in es:
                g.transition(k)
            sa, sb = es[0].stats(), es[1].stats()
            for name in ("n_steps", "is_accept", "numerical_error"):
                np.testing.assert_array_equal(sa[name], sb[name], err_msg=f"{family} {name}")
            np.testing.assert_allclose(es[0].theta(), es[1].theta(), rtol=1e-8, atol=1e-8)
            th = es[1].theta()
            for g in es:
                g.set_position(th)
        for g in es:
            g.close()
    N = 40
    lc = TG.case(65, 5, N, 2, "float64")
    t = A.GLMTarget(lc["X"], lc["y"], family=2, prior_prec=lc["p"], offset=lc["off"], scale=lc["scale"])
    out = {}
    for name, target in (("glm", t), ("mirror", A.ExternalTarget(5, t.logdensity))):
        g = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((5, N)), target), N, rng=A.PhiloxRNG(3), lib=hip)
        kern = TG.nuts_kernel(N, eps=0.02, depth=4)
        g.set_integrator(kern.tau.integrator)
        g.set_position(0.2 * lc["th"])
        g.run(kern, 3)
        out[name] = (g.theta(), g.stats()["n_steps"].copy())
        g.close()
    same = out["glm"][1] == out["mirror"][1]
    assert same.mean() >= 0.9, same.mean()
    np.testing.assert_allclose(out["glm"][0][:, same], out["mirror"][0][:, same], rtol=1e-8, atol=1e-8)


# (P, groups) at the two ends of the group table, each with the row of s after it: no group at all, and AHMC_GLM_AUX_MAX_GROUPS
# one-member groups [k, k + 1), centred and non-centred in turn, with two free coefficients after them
EDGE_MODELS = ((3, ()), (33, tuple((k, k + 1, k % 2 == 0, 0.7 + 0.05 * k) for k in range(capi.GLM_AUX_MAX_GROUPS))))


def edge_mirror(c):
    """the numpy mirror at the case's θ: (β, τ, ℓπ, g = −∇ℓπ), the mirror's float64 rounded to the case's element type"""
    th = c["th"].astype(np.float64)
    t = aux_target(c)
    W, tau = t.coefficients(th) if c["groups"] else (th[:-1].copy(), np.empty((0, th.shape[1])))
    lp, grad = t.logdensity(th)
    assert np.isfinite(lp).all() and np.isfinite(grad).all()
    return tuple(np.asfortranarray(a, dtype=c["dtype"]) for a in (W, tau, lp, -grad))


def edge_check(key, c, eps, W, tau, lp, g, phi=None):
    """§1's bounds (aux_check; τ by test_glm_hier.hier_check) on β, τ, ℓπ and every row of g"""
    assert W.shape == (c["P"], c["th"].shape[1]) and tau.shape == (len(c["groups"]), c["th"].shape[1])
    aux_check(key, c, eps, W=W, phi=phi, lp=lp, g=g)
    if c["groups"]:
        with _patched(TH, "record_bound", record_bound):
            TH.hier_check(key, dict(c, th=c["th_h"]), eps, tau=tau)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_mirror_takes_the_edge_models(dtype):
    """the mirror accepts no group and the most groups the header admits; its ℓπ and gradient are finite at the generated θ and inside
    §1's bounds of the long-double references, as the device's have to be (test_table_edges_on_the_device)"""
    for P, groups in EDGE_MODELS:
        c = acase(65, P, groups, 3, 5, np.dtype(dtype).name)
        edge_check(f"edge-mirror {np.dtype(dtype).name} ({P}, {len(groups)})", c, mirror_eps(dtype), *edge_mirror(c))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_table_edges_on_the_device(hip, probe, probe_a, dtype):  # noqa: F811
    """A dispersion's row after no group and after AHMC_GLM_AUX_MAX_GROUPS groups, N = 5 chains (a block serves four): β (P, 5) and
    τ (G, 5) of ahmc_hglm_coefficients, ℓπ and every row of g of phasepoint() inside §1's bounds of the references that the mirror is
    held to by test_mirror_takes_the_edge_models; glm_dispersion of the current θ, of host draws and of a device pointer the same
    bits, within §6's 16 u of exp of the last row"""
    eps = device_eps(probe, probe_a, dtype)
    name = np.dtype(dtype).name
    for P, groups in EDGE_MODELS:
        c = acase(65, P, groups, 3, 5, name)
        key = f"edge {name} ({P}, {len(groups)})"
        e = aux_engine(hip, c)
        z = e.phasepoint()
        W, tau = e.hglm_coefficients()
        phi = e.glm_dispersion()
        edge_check(key, c, eps, W, tau, z.lp.value.copy(), z.lp.gradient.copy(), phi=phi)
        if not groups:
            record_bits(f"W {key}", W, np.asfortranarray(c["th"][:P]))
        record_bits(f"dispersion-host-draws {key}", e.glm_dispersion(c["th"][:, 1:4]), phi[1:4])
        th_d = TG.dev(c["th"])
        record_bits(f"dispersion-device-draws {key}", e.glm_dispersion(int(th_d.data_ptr()), n_cols=5), phi)
        np.testing.assert_allclose(phi.astype(np.float64), np.exp(c["th"][-1].astype(np.float64)), rtol=16 * float(U[np.dtype(dtype)]))
        e.close()


# ---- §7 ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_refusals(hip, dtype):
    """every refusal of the header; after each the context still runs a transition on the model it had"""
    n, P, N = 65, 6, 17
    groups = ((1, 3, True, 0.9), (3, 6, False, 1.1))
    c = acase(n, P, groups, 4, N, np.dtype(dtype).name)
    e = aux_engine(hip, c)
    kern = TG.nuts_kernel(N, eps=0.02)
    X, y, off, p = (np.asfortranarray(c["X"]), c["y"].copy(), c["off"].copy(), c["p"].copy())

    def arr(ct, vals):
        return (ct * max(1, len(vals)))(*vals)

    def still_runs():
        e.transition(kern)
        assert np.isfinite(e.theta()).all() and e.stats()["n_steps"].min() >= 1
        a = C.c_double()
        e._call("ahmc_glm_aux_get_target", None, C.byref(a))
        assert a.value == AUX_PRIOR[1]

    def tabs(grp):
        return (arr(C.c_int32, [g[0] for g in grp]), arr(C.c_int32, [g[1] for g in grp]), arr(C.c_int32, [int(g[2]) for g in grp]), arr(C.c_double, [g[3] for g in grp]))

    def refused(exc, match, fam=4, n_coef=P, y_=y, grp=groups, loc=0.0, scale=1.0):
        lo, hi, cen, Asc = tabs(grp)
        with pytest.raises(exc, match=match):
            e._call("ahmc_glm_aux_set_target", fam, n, n_coef, capi.as_ptr(X), capi.as_ptr(y_), capi.as_ptr(off), capi.as_ptr(p), len(grp), lo, hi, cen, Asc, loc, scale)
        still_runs()

    def poked(a, i, v):
        b = a.copy()
        b[i] = v
        return b

    refused(A.ArgumentError, "DimensionMismatch", n_coef=P + 1)
    refused(A.ArgumentError, "DimensionMismatch", grp=groups[:1])
    for s in (0.0, -1.0, np.inf, np.nan):
        refused(A.ArgumentError, "DomainError.*aux_scale", scale=s)
    refused(A.ArgumentError, "DomainError.*aux_loc", loc=np.nan)
    refused(A.ArgumentError, "DomainError.*y >= 0", y_=poked(y, 5, -1.0))
    refused(A.ArgumentError, "DomainError", fam=3, y_=poked(y, 5, np.nan))
    for fam in (0, 1, 2, 5):
        refused(A.ArgumentError, "no sampled dispersion", fam=fam)
    refused(A.ArgumentError, "ArgumentError.*overlaps", grp=((1, 4, True, 1.0), (3, 6, False, 1.0)))
    # the old entry points keep refusing the two families, naming the new one
    lo, hi, cen, Asc = tabs(groups)
    for fam in (3, 4):
        with pytest.raises(A.ArgumentError, match="ahmc_glm_aux_set_target"):
            e._call("ahmc_hglm_set_target", fam, n, P + 1, capi.as_ptr(X), capi.as_ptr(y), capi.as_ptr(off), capi.as_ptr(p), 1.0, 2, lo, hi, cen, Asc)
        still_runs()
    # ahmc_set_ref_compat: refused where the step-synchronous engine refuses it for every target
    hmc = A.HMCKernel(A.Trajectory(A.EndPointTS, kern.tau.integrator, A.FixedNSteps(3)))
    e.set_ref_compat(True)
    with pytest.raises(A.UnsupportedError, match="ahmc_set_ref_compat"):
        e.transition(hmc)
    e.set_ref_compat(False)
    e.transition(hmc)
    still_runs()
    with pytest.raises(A.ArgumentError, match="NULL"):
        e._call("ahmc_glm_dispersion", None, 3, None)
    with pytest.raises(A.ArgumentError, match="DimensionMismatch"):
        e.glm_dispersion(np.zeros((P, 3)))
    still_runs()
    e.close()
    # a plain context: ahmc_set_target_glm refuses the families; the aux queries refuse a context without such a model
    d = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((P + 3, N)), A.IsoGaussian(P + 3)), N, dtype=dtype, rng=A.PhiloxRNG(1), lib=hip)
    Xw = np.asfortranarray(np.concatenate([X, X[:, :3]], axis=1))
    for fam in (3, 4):
        with pytest.raises(A.ArgumentError, match="ahmc_glm_aux_set_target"):
            d._call("ahmc_set_target_glm", fam, n, capi.as_ptr(Xw), capi.as_ptr(y), None, None, 1.0)
    with pytest.raises(A.ArgumentError, match="no model with a sampled dispersion"):
        d._call("ahmc_glm_aux_get_target", None, None)
    with pytest.raises(A.ArgumentError, match="no model with a sampled dispersion"):
        d._call("ahmc_glm_dispersion", capi.as_ptr(np.zeros(P + 3, dtype=dtype)), 1, capi.as_ptr(np.zeros(1, dtype=dtype)))
    d.set_integrator(kern.tau.integrator)
    d.set_position(np.asfortranarray(c["th"]))
    d.transition(kern)
    assert np.isfinite(d.theta()).all()
    d.close()
