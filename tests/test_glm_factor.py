"""Index-coded factors of the GLM target (include/ahmc_glm_factor.h): a factor with L levels stands for L one-hot columns of X without
storing or multiplying them — k_glm_eta_f gathers its rows of W into η, k_glm_fgrad fills its rows of R = −Xᵀu by ordered segmented
sums, k_glm_grad_ld / k_glm_gsum_ld write the dense rows with the column stride P; everything else of the GLM targets runs unedited
on the P = P_x + Σ L_f rows.  The arithmetic is defined by advancedhmc.jl_amd/glm.py (`factors=`).  Helpers come from
tests/test_glm_target.py, tests/test_glm_hier.py and tests/test_glm_aux.py.

Most assertions rest on one identity: with the orders of glm.py, the model with factors and the same model with the factors written
as one-hot columns appended to X (`glm.expand_factors`) give the same numbers, up to the sign of a zero, whenever W is finite —
fma(0, w, a) = a and fma(1, u, a) = a + u.  `factor_check` states it against the bit-level models of tests/test_glm_target.py (the
k-ordered fma chain over the expanded X; the slice-ordered chains over its transpose); the GPU tests state it against the engine
itself, bound to the expanded model through the entry points that existed before.

Shapes (n_obs, P_x, levels): (23, 2, (5,)) one row block, one slice; (130, 3, (7, 1)) three row blocks, two factors, the second an
intercept; (1100, 2, (70, 3)) two K slices, more levels than a wave has lanes — one level empty, one with all its observations in
the second slice, one straddling observation 1024.  N = 37 or 48.

CPU: the mirror's gradient against central differences of a long-double ℓπ (five families, with and without groups on the factor
rows); the mirror with factors against the mirror on the expanded X inside a derived bound; a host emulation of the device's
arithmetic passes `factor_check` and fails it with each of two planted defects; the constructors' refusals; header == bindings ==
Julia ccalls; ahmc_hip.h untouched; exports; the new kernels scratch-free; the checker's refusal; the parity cases' precondition.

GPU: §1 values; §2 the new kernels on a chain list; §3 whole runs; §4 parity with the oracle; §5 refusals.

The bound of the mirror comparison.  Both sides are float64 evaluations of the same model; with u = 2⁻⁵³, γ_k = k·u/(1 − k·u),
S_i = (|X_e|·|W|)_i + |offset_i| (X_e the expanded X) each side's η̂ is within γ_{P+1}·S_i of the exact η whatever the order of its
P products and additions and the one addition of the offset, so the two differ by Δη ≤ 2·γ_{P+1}·S.  ℓ and u then differ by
test_glm_target.link_bounds / test_glm_aux.aux_link_bounds at Δη (the link's Lipschitz constants and the roundings of its
functions, measured for numpy by `function_eps` / `mirror_eps`), once per side: 2·E_ℓ, 2·E_u, 2·E_∂s.  R = −X_eᵀu: 2·(|X_e|ᵀ·E_u +
γ_{n_obs+1}·|X_e|ᵀ(|u| + E_u)) =: E_R, any order of the sums.  Σℓ: 2·(ΣE_ℓ + γ_{n_obs}·Σ(|ℓ| + E_ℓ)); the prior and the groups' terms
of ℓπ are computed from θ alone and are the same numbers on both sides, so ℓπ differs by that plus 4 roundings of the running sum.
g: a fixed or centred row is R plus a term of θ alone: E_R + u·|g|; a non-centred member is τ·R + θ: τ·E_R + u·|g|; the row of a
non-centred s_k is T_k − h′_k with T_k = Σ R_d·w_d: Σ_d E_R·|w_d| + γ_{m+1}·Σ|R_d·w_d| + u·|g|; the row of a centred s_k does not
depend on R; the dispersion's row is −Σ∂ℓ/∂s plus a term of θ alone: as Σℓ with E_∂s.  SLACK = 1.01 covers products of two
first-order terms, as in the modules this one borrows from.
"""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ahmc_amd as A
import test_glm_aux as TA
import test_glm_hier as TH
import test_glm_target as TG
from ahmc_amd import _capi as capi
from ahmc_amd import glm as G
from test_glm_target import probe  # noqa: F401  (a fixture of the helpers)

LD = np.longdouble
ROOT = TG.ROOT
PROBE_F = os.path.join(ROOT, "tests", "device_probe", "glm_factor.hip")
DTYPES = TG.DTYPES
FAMNAMES = {v: k for k, v in G.FAMILIES.items()}
AUX_PRIOR = (0.3, 1.2)
CASES = {"one-block": (23, 2, (5,)), "two-factors": (130, 3, (7, 1)), "two-slices": (1100, 2, (70, 3))}
N_CHAINS = 37
gam, U, U_LD, SLACK = TG.gam, TG.U, TG.U_LD, TG.SLACK
record_bits = TG.record_bits


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
def factor_index(n_obs, L, rs):
    """level indices; at L = 70 (n_obs = 1100): level 5 is empty, level 9 has all its observations in the second slice, level 11
    straddles observation 1024"""
    idx = rs.integers(0, L, size=n_obs)
    if L == 70:
        idx[idx == 5] = 6
        idx[:G.K_SLICE][idx[:G.K_SLICE] == 9] = 10
        idx[[1050, 1090]] = 9
        idx[[1023, 1024]] = 11
        assert not (idx == 5).any() and np.flatnonzero(idx == 9).min() >= G.K_SLICE
        assert (idx[:G.K_SLICE] == 11).any() and (idx[G.K_SLICE:] == 11).any()
    return idx


def case_groups(Px, ranges, grouped):
    """a non-centred group on factor 0's rows and a centred one: on factor 1's rows, or on the dense rows when there is one factor"""
    if not grouped:
        return ()
    nc = (*ranges[0], False, 1.3)
    return (nc, (*ranges[1], True, 0.8)) if len(ranges) > 1 else ((0, Px, True, 0.8), nc)


@functools.lru_cache(maxsize=None)
def fcase(name, fam, N, dtname, grouped=True):
    """operands of one case in the element type, computed once"""
    n_obs, Px, levels = CASES[name]
    dtype = np.dtype(dtname)
    aux = fam in G.AUX_FAMILIES
    rs = np.random.default_rng([n_obs, Px, len(levels), N, fam, dtype.itemsize, int(grouped)])
    X = np.asfortranarray(rs.normal(size=(n_obs, Px)) / np.sqrt(Px), dtype=dtype)
    factors = tuple(A.Factor(factor_index(n_obs, L, rs), L) for L in levels)
    ranges = G.factor_ranges(Px, factors)
    P = ranges[-1][1]
    groups = case_groups(Px, ranges, grouped)
    Gn = len(groups)
    D = P + Gn + (1 if aux else 0)
    th = np.concatenate([0.5 * rs.normal(size=(P, N)), 0.4 * rs.normal(size=(Gn, N)), 0.3 * rs.normal(size=(D - P - Gn, N))])
    th = np.asfortranarray(th, dtype=dtype)
    if fam == G.BERNOULLI_LOGIT:
        y = np.where(np.arange(n_obs) % 3 == 2, rs.random(n_obs), (rs.random(n_obs) < 0.5).astype(np.float64)).astype(dtype)
    elif fam in (G.POISSON_LOG, G.NEGBINOMIAL_LOG):
        y = rs.poisson(3.0, size=n_obs).astype(dtype)
    else:
        y = rs.normal(size=n_obs).astype(dtype)
    p = (2 * rs.random(P)).astype(dtype)
    p[::3] = 0
    for lo, hi, _, _ in groups:
        p[lo:hi] = 0
    off = (0.3 * rs.normal(size=n_obs)).astype(dtype)
    Xe = np.asfortranarray(G.expand_factors(X.astype(np.float64), factors), dtype=dtype)   # (0 and 1 are exact in either type)
    return {"name": name, "X": X, "Xe": Xe, "Xet": np.asfortranarray(Xe.T), "Xt": np.asfortranarray(X.T), "y": y, "off": off, "p": p, "th": th,
            "scale": 1.0 if aux else 1.7, "fam": fam, "aux": aux, "dtype": dtype, "groups": groups, "factors": factors, "ranges": ranges, "Px": Px, "P": P,
            "D": D, "U": np.asfortranarray(rs.normal(size=(n_obs, N)), dtype=dtype),
            "ia2": np.array([dtype.type(1.0 / (a * a)) for _, _, _, a in groups], dtype=dtype)}


def target(c, onehot=False):
    """the case's model with its factors, or the same model with the factors as one-hot columns of X through the older entry points"""
    kw = dict(family=c["fam"], prior_prec=c["p"], offset=c["off"], scale=c["scale"], aux_prior=AUX_PRIOR if c["aux"] else None)
    X, fk = (c["Xe"], {}) if onehot else (c["X"], {"factors": c["factors"]})
    return A.HierGLMTarget(X, c["y"], c["groups"], **kw, **fk) if c["groups"] else A.GLMTarget(X, c["y"], **kw, **fk)


def effective_coefficients(c):
    """W and τ in the element type, as k_hglm_coef makes them (numpy's exp for the device's)"""
    P, Gn, th = c["P"], len(c["groups"]), c["th"]
    tau = np.exp(th[P:P + Gn])
    W = np.asfortranarray(th[:P].copy())
    for k, (lo, hi, cen, _) in enumerate(c["groups"]):
        if not cen:
            W[lo:hi] = tau[k] * th[lo:hi]
    return W, tau


def ordered_level_sums(Um, idx, L, flush=True):
    """Σ u over the observations of each level in the element type: slices of K_SLICE, within a slice ascending i from +0, the slice
    sums added in ascending order (`flush` False: one run over all observations — the planted defect)"""
    n_obs = Um.shape[0]
    step = G.K_SLICE if flush else n_obs
    tot = np.zeros((L, Um.shape[1]), dtype=Um.dtype)
    for k0 in range(0, n_obs, step):
        s = np.zeros_like(tot)
        np.add.at(s, idx[k0:k0 + step], Um[k0:k0 + step])
        tot = tot + s
    assert tot.dtype == Um.dtype
    return tot


def factor_check(key, c, W, eta=None, Um=None, R=None):
    """what the GPU tests assert of the values, on whatever results are given (the device's, or a host emulation's): η is the k-ordered
    fma chain of the EXPANDED model at the results' own W, then the offset; R at a given U is the negated slice-ordered chain over
    the expanded Xᵀ — as numbers (−0 = +0)"""
    W = np.asfortranarray(W, dtype=c["dtype"])
    if eta is not None:
        record_bits(f"eta {key}", eta, TG.chain(c["Xe"], W) + c["off"].reshape(-1, 1))
    if R is not None:
        record_bits(f"R {key}", R, TG.grad_model(c["Xet"], np.asfortranarray(Um), np.zeros(c["P"], dtype=c["dtype"]), W))


def emulate(c, defect=None):
    """the device's arithmetic with factors on the host in the element type: (W, η, R at the case's U).  `defect`: "no_flush" adds a
    level's observations in one run without the flush at 1024; "drop_gather" drops the second factor's gather"""
    W, _ = effective_coefficients(c)
    Px = c["Px"]
    eta = TG.chain(c["X"], np.asfortranarray(W[:Px]))
    for f, ((lo, _), fac) in enumerate(zip(c["ranges"], c["factors"])):
        if defect == "drop_gather" and f == 1:
            continue
        eta = eta + W[lo + fac.index]
    eta = eta + c["off"].reshape(-1, 1)
    R = np.empty_like(W)
    R[:Px] = TG.grad_model(c["Xt"], c["U"], np.zeros(Px, dtype=c["dtype"]), np.asfortranarray(W[:Px]))
    for (lo, hi), fac in zip(c["ranges"], c["factors"]):
        R[lo:hi] = -ordered_level_sums(c["U"], fac.index, fac.n_levels, flush=defect != "no_flush")
    assert eta.dtype == c["dtype"] and R.dtype == c["dtype"]
    return W, eta, R


# ------------------------------------------------------------------------------------------------
# CPU 1: the mirror's gradient
# ------------------------------------------------------------------------------------------------
def lp_ld(fam, X, factors, y, t, groups, off, p, scale, aux_prior):
    """ℓπ of the headers in long double, written from the formulas (the gathers, not the one-hot columns)"""
    Px = X.shape[1]
    ranges = G.factor_ranges(Px, factors)
    P = ranges[-1][1] if ranges else Px
    Gn = len(groups)
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
    eta = X.astype(LD) @ w[:Px]
    for (lo, _), fac in zip(ranges, factors):
        eta = eta + w[lo + fac.index]
    if off is not None:
        eta = eta + off.astype(LD).reshape(-1, 1)
    if fam in G.AUX_FAMILIES:
        s = t[P + Gn]
        ll = TA.link_ld(fam, y.reshape(-1, 1), eta, s.reshape(1, -1))[0]
        m, a = aux_prior
        out = out - ((s - LD(m)) / LD(a)) ** 2 / 2
    else:
        ll = TG.link_ld(fam, y.reshape(-1, 1), eta, scale)[0]
    return out + ll.sum(axis=0) - (0 if p is None else (p.astype(LD).reshape(-1, 1) * t[:P] ** 2).sum(axis=0) / 2)


@pytest.mark.parametrize("fam", sorted(FAMNAMES), ids=[FAMNAMES[f] for f in sorted(FAMNAMES)])
@pytest.mark.parametrize("grouped", [True, False], ids=["groups", "no-groups"])
def test_mirror_gradient_against_central_differences(fam, grouped):
    """every row of ∇ℓπ of the mirror with two factors against central differences of a long-double ℓπ (h = 1e-6): dense rows, the
    levels of both factors (a non-centred group on one, a centred group on the other), the log-scales, the dispersion"""
    rs = np.random.default_rng(41 + fam)
    n, Px = 23, 2
    X = np.asfortranarray(rs.normal(size=(n, Px)) / 2)   # (the target keeps X column-major: numpy's product depends on the memory order)
    factors = (A.Factor(rs.integers(0, 5, size=n), 5), A.Factor(rs.integers(0, 3, size=n), 3))
    ranges = A.factor_ranges(Px, factors)
    assert ranges == [(2, 7), (7, 10)]
    groups = case_groups(Px, ranges, grouped)
    aux = fam in G.AUX_FAMILIES
    y = (rs.random(n) < 0.5).astype(float) if fam == 0 else rs.poisson(3.0, size=n).astype(float) if fam in (1, 4) else rs.normal(size=n)
    p = rs.random(10)
    for lo, hi, _, _ in groups:
        p[lo:hi] = 0
    off = 0.3 * rs.normal(size=n)
    scale = 1.0 if aux else 1.7
    D = 10 + len(groups) + aux
    th = 0.4 * rs.normal(size=(D, 3))
    ap = AUX_PRIOR if aux else None
    lp, grad = G.hier_logdensity(fam, X, y, th, groups, off, p, scale, ap, factors=factors)
    assert lp.shape == (3,) and grad.shape == th.shape
    np.testing.assert_allclose(lp, lp_ld(fam, X, factors, y, th, groups, off, p, scale, ap).astype(np.float64), rtol=1e-13, atol=1e-13)
    h = LD("1e-6")
    for d in range(D):
        tp, tm = th.astype(LD), th.astype(LD)
        tp[d] += h
        tm[d] -= h
        fd = ((lp_ld(fam, X, factors, y, tp, groups, off, p, scale, ap) - lp_ld(fam, X, factors, y, tm, groups, off, p, scale, ap)) / (2 * h)).astype(np.float64)
        np.testing.assert_allclose(grad[d], fd, rtol=1e-8, atol=1e-8)
    # the other doors into the one evaluation path
    t = target({"fam": fam, "p": p, "off": off, "scale": scale, "aux": aux, "X": X, "y": y, "groups": groups, "factors": factors})
    assert (t.P, t.P_x, t.D, t.factor_ranges) == (10, 2, D, ranges)
    np.testing.assert_array_equal(t.logdensity(th)[1], grad)
    if not groups:
        np.testing.assert_array_equal(G.logdensity(fam, X, y, th, off, p, scale, ap, factors=factors)[0], lp)
    if aux:
        np.testing.assert_array_equal(G.aux_logdensity(fam, X, y, th, groups, off, p, ap, factors=factors)[1], grad)
    eta, _ = G.hier_pointwise(fam, X, y, th, groups, off, scale, factors=factors)
    beta, tau = G.hier_coefficients(th[:-1] if aux else th, Px, groups, factors=factors)
    assert beta.shape == (10, 3) and tau.shape == (len(groups), 3)
    want = X @ beta[:2] + beta[2 + factors[0].index] + beta[7 + factors[1].index] + off.reshape(-1, 1)
    np.testing.assert_allclose(eta, want, rtol=1e-14, atol=1e-14)
    if not groups:
        np.testing.assert_array_equal(G.pointwise(fam, X, y, th, off, scale, factors=factors)[0], eta)


# ------------------------------------------------------------------------------------------------
# CPU 2: the mirror with factors against the mirror on the expanded X
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", sorted(FAMNAMES), ids=[FAMNAMES[f] for f in sorted(FAMNAMES)])
@pytest.mark.parametrize("name", list(CASES))
def test_mirror_with_factors_against_the_expanded_model(fam, name):
    """η, ℓπ and every row of ∇ℓπ of the two encodings inside the bound of the module docstring (numpy's products are not fma chains:
    a bound, not an identity); β and τ are the same numbers"""
    c = fcase(name, fam, 5, "float64")
    P, Px, groups, n_obs, aux = c["P"], c["Px"], c["groups"], CASES[name][0], c["aux"]
    u = U[c["dtype"]]
    eps = TA.mirror_eps(np.float64)
    t, te = target(c), target(c, onehot=True)
    th = c["th"]
    lp, grad = t.logdensity(th)
    lpe, grade = te.logdensity(th)
    ap = AUX_PRIOR if aux else None
    eta, ll = G.hier_pointwise(c["fam"], c["X"], c["y"], th, groups, c["off"], c["scale"], factors=c["factors"])
    etae, _ = G.hier_pointwise(c["fam"], c["Xe"], c["y"], th, groups, c["off"], c["scale"])
    W, tau = G.hier_coefficients(th[:-1] if aux else th, Px, groups, factors=c["factors"])
    We, taue = G.hier_coefficients(th[:-1] if aux else th, P, groups)
    np.testing.assert_array_equal(W, We)
    np.testing.assert_array_equal(tau, taue)
    absXe = np.abs(c["Xe"]).astype(LD)
    S = absXe @ np.abs(W).astype(LD) + np.abs(c["off"]).astype(LD).reshape(-1, 1)
    d_eta = SLACK * gam(P + 1, u) * S
    key = f"mirror {FAMNAMES[fam]} {name}"
    TG.record_bound(f"eta {key}", np.abs(eta.astype(LD) - etae.astype(LD)), 2 * d_eta)
    # the link's bounds at Δη, around this side's values (long double)
    if aux:
        s = th[-1].astype(LD).reshape(1, -1)
        llr, ur, dsr, pieces = TA.link_ld(fam, c["y"].reshape(-1, 1), eta.astype(LD), s)
        El, Eu, Eds = TA.aux_link_bounds({**c, "ll": llr, "u": ur, "ds": dsr, "pieces": pieces}, eps, eta, d_eta)
    else:
        llr, ur = TG.link_ld(fam, c["y"].reshape(-1, 1), eta.astype(LD), c["scale"])
        El, Eu = TG.link_bounds({"fam": fam, "dtype": c["dtype"], "eta_hat": eta, "d_eta": d_eta, "y": c["y"], "scale": c["scale"], "ll": llr, "u": ur}, eps)
    XE = absXe.T @ Eu
    ER = 2 * SLACK * (XE + gam(n_obs + 1, u) * (absXe.T @ (np.abs(ur) + Eu)))
    Elp = 2 * SLACK * (El.sum(axis=0) + gam(n_obs, u) * (np.abs(llr) + El).sum(axis=0)) + 4 * u * (np.abs(lp).astype(LD) + np.abs(llr).sum(axis=0))
    TG.record_bound(f"lp {key}", np.abs(lp.astype(LD) - lpe.astype(LD)), Elp)
    absg = np.abs(grad).astype(LD)
    Eg = np.zeros_like(absg)
    Eg[:P] = ER
    R = np.abs(absXe.T @ np.abs(ur))
    for k, (lo, hi, cen, _) in enumerate(groups):
        if not cen:
            tk = np.abs(tau[k]).astype(LD)
            Eg[lo:hi] = tk * ER[lo:hi]
            aw = np.abs(W[lo:hi]).astype(LD)
            Eg[P + k] = SLACK * ((ER[lo:hi] * aw).sum(axis=0) + gam(hi - lo + 1, u) * ((R[lo:hi] + ER[lo:hi]) * aw).sum(axis=0))
    if aux:
        Eg[-1] = 2 * SLACK * (Eds.sum(axis=0) + gam(n_obs, u) * (np.abs(dsr) + Eds).sum(axis=0))
    TG.record_bound(f"grad {key}", np.abs(grad.astype(LD) - grade.astype(LD)), Eg + 4 * u * absg)


# ------------------------------------------------------------------------------------------------
# CPU 3: a host emulation passes the GPU assertions, and two planted defects do not
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_host_emulation_passes_and_two_defects_are_caught(dtype):
    """The device's arithmetic with factors, emulated on the host in the element type, equals the bit-level models of the EXPANDED
    model (the identity of the module docstring); with a level's sum taken in one run over both slices, and with the second
    factor's gather dropped, `factor_check` fails"""
    dtname = np.dtype(dtype).name
    for name in CASES:
        c = fcase(name, 0, 5, dtname)
        W, eta, R = emulate(c)
        factor_check(f"host-emulation {dtname} {name}", c, W, eta=eta, Um=c["U"], R=R)
        for (lo, hi), fac in zip(c["ranges"], c["factors"]):
            empty = np.setdiff1d(np.arange(fac.n_levels), fac.index)
            assert np.all(R[lo + empty] == 0)
    c = fcase("two-slices", 0, 5, dtname)
    W, eta, R = emulate(c, "no_flush")
    with pytest.raises(AssertionError, match="R planted"):
        factor_check("planted", c, W, Um=c["U"], R=R)
    for name in ("two-factors", "two-slices"):
        c = fcase(name, 0, 5, dtname)
        W, eta, R = emulate(c, "drop_gather")
        with pytest.raises(AssertionError, match="eta planted"):
            factor_check("planted", c, W, eta=eta)
    for k in [k for k in TG.MARGINS if k.endswith(" planted")]:
        del TG.MARGINS[k]


# ------------------------------------------------------------------------------------------------
# CPU 4: constructors and refusals
# ------------------------------------------------------------------------------------------------
def test_constructor_and_refusals():
    rs = np.random.default_rng(3)
    n = 12
    X, y = rs.normal(size=(n, 2)), rs.poisson(2.0, size=n).astype(float)
    idx = rs.integers(0, 4, size=n)
    idx[0] = 3
    f = A.Factor(idx)
    assert (f.n_levels, f.index.dtype, repr(f)) == (4, np.int64, "Factor(n_obs=12, n_levels=4)")
    assert A.Factor(idx.astype(np.int32), 6).n_levels == 6 and A.Factor(list(map(int, idx))).n_levels == 4
    assert A.factor_ranges(2, [f, A.Factor(idx, 6)]) == [(2, 6), (6, 12)] and A.factor_ranges(3, []) == []
    t = A.GLMTarget(X, y, family="poisson_log", factors=[f], prior_scale=2.0)
    assert (t.P, t.P_x, t.D, t.n_obs, t.factor_ranges, t.kind, t.prior_prec.shape) == (6, 2, 6, n, [(2, 6)], capi.TARGET_GLM, (6,))
    np.testing.assert_array_equal(G.expand_factors(X, [f]), np.column_stack([X, np.eye(4)[idx]]))
    assert A.GLMTarget(X, y, family="negbinomial_log", factors=[f, (idx, 5)]).D == 2 + 4 + 5 + 1
    assert A.GLMTarget(X, y, family="poisson_log").factors == () and A.GLMTarget(X, y, family="poisson_log").P_x == 2
    A.Hamiltonian(A.UnitEuclideanMetric(6), t)
    with pytest.raises(A.ArgumentError):
        A.Hamiltonian(A.UnitEuclideanMetric(2), t)
    # a group may straddle a factor's boundary (the rows are coefficients like any other); overlap stays refused
    h = A.HierGLMTarget(X, y, [A.CoefGroup(1, 4), A.CoefGroup(4, 6, centered=True)], family="poisson_log", factors=[f])
    assert (h.D, h.P, [(g.start, g.stop) for g in h.groups]) == (8, 6, [(1, 4), (4, 6)])
    th = 0.3 * rs.normal(size=(8, 2))
    np.testing.assert_array_equal(h.coefficients(th)[0], G.hier_coefficients(th, 2, h.groups, factors=[f])[0])
    assert np.isfinite(h.logdensity(th)[0]).all()
    nine = [A.Factor(idx)] * 9
    assert A.GLMTarget(X, y, family="poisson_log", factors=nine[:8]).P == 2 + 32
    for bad in (lambda: A.Factor(idx, 3), lambda: A.Factor(-idx - 1, 4), lambda: A.Factor(np.where(idx == 0, -1, idx)), lambda: A.Factor(idx.astype(float)),
                lambda: A.Factor(idx > 1), lambda: A.Factor(idx.reshape(3, 4)), lambda: A.Factor(idx, 0), lambda: A.Factor([]),
                lambda: A.GLMTarget(X, y, family="poisson_log", factors=[A.Factor(idx[:-1])]), lambda: A.GLMTarget(X, y, family="poisson_log", factors=[(idx[:5], 4)]),
                lambda: A.GLMTarget(X, y, family="poisson_log", factors=nine), lambda: A.GLMTarget(X[:, :0], y, family="poisson_log", factors=[f]),
                lambda: A.GLMTarget(X, y, family="poisson_log", factors=[f], prior_prec=np.ones(2)),
                lambda: A.HierGLMTarget(X, y, [A.CoefGroup(1, 4), A.CoefGroup(3, 6)], family="poisson_log", factors=[f]),
                lambda: A.HierGLMTarget(X, y, [A.CoefGroup(2, 7)], family="poisson_log", factors=[f])):
        with pytest.raises(A.ArgumentError):
            bad()
    for bad in (lambda: G.check_factors([(idx, 3)], n), lambda: G.check_factors([(idx, 4)], n + 1), lambda: G.check_factors([(idx * 1.0, 4)], n),
                lambda: G.check_factors([(idx, 4)] * 9, n), lambda: G.logdensity(1, X, y, np.zeros((5, 2)), factors=[f]),
                lambda: G.expand_factors(X, [(idx - 1, 4)])):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------
# CPU 5: header == binding table == Julia ccalls == exported symbols; the kernels; the checker
# ------------------------------------------------------------------------------------------------
def header_prototypes():
    src = open(os.path.join(ROOT, "include", "ahmc_glm_factor.h"), encoding="utf-8").read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(int32_t)\s+(ahmc_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        params = " ".join(m.group(3).split())
        protos[m.group(2)] = [] if params in ("", "void") else [p.strip() for p in params.split(",")]
    return protos, src


def test_header_and_bindings_agree():
    protos, src = header_prototypes()
    assert set(protos) == set(capi.GLM_FACTOR_SIGNATURES) == {"ahmc_glm_factor_version", "ahmc_glm_factor_set_target", "ahmc_glm_factor_get_target"}
    assert not set(capi.GLM_FACTOR_SIGNATURES) & (set(capi.GLM_SIGNATURES) | set(capi.HGLM_SIGNATURES) | set(capi.GLM_AUX_SIGNATURES) | set(capi.SIGNATURES))
    ct = {"int64_t*": C.POINTER(C.c_int64), "int32_t*": C.POINTER(C.c_int32), "double*": C.POINTER(C.c_double), "int64_t": C.c_int64,
          "int32_t": C.c_int32, "double": C.c_double}
    for name, params in protos.items():
        res, args = capi.GLM_FACTOR_SIGNATURES[name]
        assert res is C.c_int32 and len(args) == len(params), name
        for p, a in zip(params, args):
            typ = p.rsplit(" ", 1)[0].replace("const ", "").replace(" ", "")
            if typ in ("void*", "ahmc_ctx*"):
                assert a is C.c_void_p, (name, p)
            else:
                assert a is ct[typ], (name, p)
    # ahmc_hglm_set_target's arguments, then the factors, then the dispersion
    hier = [p.split()[-1] for p in TH.header_prototypes()[0]["ahmc_hglm_set_target"]]
    assert [p.split()[-1] for p in protos["ahmc_glm_factor_set_target"]] == hier + ["n_factors", "n_levels", "levels", "has_aux", "aux_loc", "aux_scale"]
    assert [p.split()[-1] for p in protos["ahmc_glm_factor_get_target"]] == ["ctx", "n_coef", "n_factors", "n_levels"]
    assert re.search(r"#define AHMC_GLM_FACTOR_VERSION (\d+)", src).group(1) == str(capi.AHMC_GLM_FACTOR_VERSION) == "1"
    assert re.search(r"#define AHMC_GLM_FACTOR_MAX (\d+)", src).group(1) == str(capi.GLM_FACTOR_MAX) == str(G.GLM_FACTOR_MAX) == "8"
    from ahmc_amd import build as B
    assert "ahmc_glm_factor.h" in open(B.__file__, encoding="utf-8").read()
    dev = open(os.path.join(ROOT, "advancedhmc.jl_amd", "csrc", "ahmc_glm.hpp"), encoding="utf-8").read()
    assert re.search(r"constexpr int GLM_MAX_FACTORS = (\d+);", dev).group(1) == "8"


def test_the_other_headers_are_untouched():
    """ahmc_hip.h does not know the GLM and keeps its ABI version; the three GLM headers keep theirs and do not name the new one"""
    inc = os.path.join(ROOT, "include")
    hip_h = open(os.path.join(inc, "ahmc_hip.h"), encoding="utf-8").read()
    assert "glm" not in hip_h.lower() and re.search(r"#define AHMC_ABI_VERSION (\d+)", hip_h).group(1) == "6" == str(capi.AHMC_ABI_VERSION)
    for hdr, macro, v in (("ahmc_glm.h", "AHMC_GLM_VERSION", capi.AHMC_GLM_VERSION), ("ahmc_glm_hier.h", "AHMC_HGLM_VERSION", capi.AHMC_HGLM_VERSION),
                          ("ahmc_glm_aux.h", "AHMC_GLM_AUX_VERSION", capi.AHMC_GLM_AUX_VERSION)):
        src = open(os.path.join(inc, hdr), encoding="utf-8").read()
        assert re.search(rf"#define {macro} (\d+)", src).group(1) == str(v) == "1" and "ahmc_glm_factor" not in src
    assert not set(capi.GLM_FACTOR_SIGNATURES) & set(re.findall(r"\bahmc_[a-z_0-9]+", hip_h)) and "AHMC_GLM_FACTOR" not in hip_h


def test_julia_ccalls_match_the_header():
    protos, _ = header_prototypes()
    src = open(os.path.join(ROOT, "julia", "AdvancedHMCMI355XGLMFactor.jl"), encoding="utf-8").read()
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
    assert 'include("AdvancedHMCMI355XGLMFactor.jl")' in ext and "ahmc_glm_factor_set_target" not in ext
    assert ext.index('include("AdvancedHMCMI355XGLMAux.jl")') < ext.index('include("AdvancedHMCMI355XGLMFactor.jl")')


NEW_KERNELS = ([f"k_glm_eta_f<{t}, {f}, {bn}>" for t in ("float", "double") for f in range(5) for bn in (64, 16)]
               + [f"k_glm_grad_ld<{t}, {bn}>" for t in ("float", "double") for bn in (64, 16)]
               + [f"k_{w}<{t}>" for w in ("glm_gsum_ld", "glm_fgrad") for t in ("float", "double")])


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="needs llvm-objdump")
def test_library_exports_and_kernels_without_scratch():
    """every entry point is in the dynamic symbol table (read without loading the library); the new kernels are in the code object
    with no private segment and no VGPR spill (scripts/kernel_meta.py), and each k_glm_eta_f instantiation allocates no more LDS and
    fits as many waves per SIMD by its registers as the k_glm_eta instantiation beside it"""
    from ahmc_amd import build as B

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_meta
    finally:
        sys.path.pop(0)
    assert os.path.exists(B.OUT), "build() first"
    exported = {l.split()[-1] for l in subprocess.run(["nm", "-D", "--defined-only", B.OUT], capture_output=True, text=True, check=True).stdout.splitlines() if l.strip()}
    assert set(capi.GLM_FACTOR_SIGNATURES) <= exported, set(capi.GLM_FACTOR_SIGNATURES) - exported
    meta = kernel_meta.kernel_meta(B.OUT)
    names = subprocess.run(["c++filt"], input="\n".join(k["name"] for k in meta), capture_output=True, text=True, check=True).stdout.splitlines()
    want = NEW_KERNELS + [w.replace("k_glm_eta_f<", "k_glm_eta<") for w in NEW_KERNELS if w.startswith("k_glm_eta_f<")]
    found = {}
    for k, dn in zip(meta, names):
        for w in want:
            if dn.startswith(f"void ahmc::{w}("):
                found[w] = k
    assert sorted(found) == sorted(want), sorted(set(want) - set(found))

    def waves(k):   # (512 registers a lane and SIMD, allocated in blocks of 8; at most 8 waves)
        regs = (k["vgpr_count"] + k.get("agpr_count", 0) + 7) // 8 * 8
        return min(8, 512 // regs)

    for w in NEW_KERNELS:
        k = found[w]
        assert k["private_segment_fixed_size"] == 0, (w, k)
        assert k.get("vgpr_spill_count", 0) == 0, (w, k)
        if w.startswith("k_glm_eta_f<"):
            old = found[w.replace("k_glm_eta_f<", "k_glm_eta<")]
            assert waves(k) >= waves(old) and k["group_segment_fixed_size"] <= old["group_segment_fixed_size"], (w, k, old)


def test_cpu_checker_refuses_the_target(oracle):
    assert oracle.has_glm_factor is False
    c = fcase("one-block", 1, 3, "float64")
    t = target(c)
    with pytest.raises(A.UnsupportedError, match="ahmc_glm_factor.h"):
        A.Engine(A.Hamiltonian(A.UnitEuclideanMetric(t.D), t), 3, lib=oracle)
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric(t.D), A.IsoGaussian(t.D)), 3, lib=oracle)
    with pytest.raises(A.UnsupportedError, match="ahmc_glm_factor.h"):
        e.set_target(t)
    with pytest.raises(A.UnsupportedError, match="ahmc_glm_factor.h"):
        e.glm_factors()
    e.close()


# ------------------------------------------------------------------------------------------------
# §4's inputs, and their precondition on the oracle alone
# ------------------------------------------------------------------------------------------------
# name: (n_obs, P_x, levels, family, grouped, seed, N)
PARITY = {"logit, a non-centred factor": (130, 3, (7, 1), "bernoulli_logit", True, 1, 48),
          "poisson, divergent": (130, 3, (7,), "poisson_log", False, 3, 48),
          "dense": (130, 3, (7, 1), "bernoulli_logit", True, 1, 48),
          "wide": (130, 2, (5000,), "bernoulli_logit", True, 1, 64)}


def parity_inputs(n_obs, Px, levels, family, grouped, seed, N):
    rs = np.random.default_rng([n_obs, Px, len(levels), seed, G.family_code(family)])
    X = rs.normal(size=(n_obs, Px)) / np.sqrt(Px)
    factors = [A.Factor(rs.integers(0, L, size=n_obs), L) for L in levels]
    ranges = A.factor_ranges(Px, factors)
    P = ranges[-1][1]
    groups = (A.CoefGroup(*ranges[0], centered=False, scale=1.0),) if grouped else ()
    beta = rs.normal(size=P) * (0.5 if levels[0] < 100 else 0.1)
    eta = G.expand_factors(X, factors) @ beta
    divergent = family == "poisson_log"
    y = (rs.random(n_obs) < 1 / (1 + np.exp(-eta))).astype(np.float64) if family == "bernoulli_logit" else rs.poisson(np.exp(eta)).astype(np.float64)
    p = np.ones(P)
    for g in groups:
        p[g.start:g.stop] = 0
    D = P + len(groups)
    minv = np.asfortranarray(0.5 + rs.random((D, N)))
    th0 = (1.5 if divergent else 0.5) * rs.normal(size=(D, N))   # (Poisson: e^η overflows the energy within the first steps)
    if levels[0] >= 100:
        th0[Px:P] *= 0.2
    eps = (0.3 if divergent else 0.2) * (0.7 + 0.6 * rs.random(N))
    kw = dict(family=family, prior_prec=p, factors=factors)
    t = A.HierGLMTarget(X, y, groups, **kw) if groups else A.GLMTarget(X, y, **kw)
    return t, minv, th0, eps


def parity_metric(name, t, minv, N):
    if name == "dense":
        return TA.dense_metric(t.D)
    return A.UnitEuclideanMetric((t.D, N)) if name == "wide" else A.DiagEuclideanMetric(minv)


@pytest.mark.parametrize("name", list(PARITY))
def test_parity_precondition_on_the_oracle_alone(oracle, name):
    """On §4's inputs no decision of the oracle (running the mirror as a host kernel) comes within the suite's bound for float64 of a
    tie, at any step of the sequence and for any chain: the GPU comparison may demand exact agreement of every chain.  The Poisson
    case: most chains diverge in their first transition."""
    t, minv, th0, eps = parity_inputs(*PARITY[name])
    N = th0.shape[1]
    o = TH.oracle_engine(oracle, t, parity_metric(name, t, minv, N), N)
    if name == "wide":
        assert t.D > 4096
        smallest, n_div = TG.parity_sequence(o, None, th0, eps, f"glm-factor {name}", nuts_depth=3, full=False)
    else:
        smallest, n_div = TG.parity_sequence(o, None, th0, eps, f"glm-factor {name}")
    TG.MARGINS[f"factor oracle-margin {name}"] = {"smallest_decision_margin": smallest, "divergent_chains_max": n_div}
    o.close()
    if "divergent" in name:
        o2 = TH.oracle_engine(oracle, t, parity_metric(name, t, minv, N), N)
        first = TH.first_transition_divergences(o2, th0, eps)
        o2.close()
        assert first > N // 2, first


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
_STATE = {}


@pytest.fixture(scope="module")
def probe_f(hip):
    import torch

    from ahmc_amd import build as B
    from ahmc_amd.hipmod import Module

    torch.cuda.init()
    if "probe_f" not in _STATE:
        _STATE["probe_f"] = Module(B.build_probe_object(PROBE_F))
    return _STATE["probe_f"]


def engine(hip, c, onehot=False, cols=None, metric=None, seed=7):
    th = c["th"] if cols is None else c["th"][:, cols]
    D, N = th.shape
    e = A.Engine(A.Hamiltonian(metric or A.UnitEuclideanMetric((D, N)), target(c, onehot)), N, dtype=c["dtype"],
                 rng=seed if isinstance(seed, A.PhiloxRNG) else A.PhiloxRNG(seed), lib=hip)
    e.set_integrator(A.Leapfrog(np.full(N, 0.02)))
    e.set_position(th)
    return e


def evaluate(e, c, th=None, hier=True):
    """η, ℓ, ℓπ, g and — where the binding serves them — (β, τ) and the dispersion, at θ"""
    if th is not None:
        e.set_position(th)
    z = e.phasepoint()
    eta, ll = e.glm_pointwise()
    out = {"eta": eta, "loglik": ll, "lp": z.lp.value.copy(), "grad": z.lp.gradient.copy()}
    if hier:
        out["W"], out["tau"] = e.hglm_coefficients()
    if c["aux"]:
        out["dispersion"] = e.glm_dispersion()
    return out


# ---- §1 ----
@pytest.mark.gpu
@pytest.mark.parametrize("fam", sorted(FAMNAMES), ids=[FAMNAMES[f] for f in sorted(FAMNAMES)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_values_equal_the_one_hot_model(hip, fam, dtype):
    """With a non-centred group on a factor and a centred group, and without groups, under either tile shape: η of ahmc_glm_pointwise
    is the fma chain of the expanded model at the device's own W, bit for bit; η, ℓ, ℓπ, every row of g, ahmc_hglm_coefficients and
    ahmc_glm_dispersion equal, as numbers, what the engine computes for the expanded model bound through the older entry points;
    the getters report the model"""
    dtname = np.dtype(dtype).name
    for name, (n_obs, Px, levels) in CASES.items():
        for grouped in (True, False):
            c = fcase(name, fam, N_CHAINS, dtname, grouped)
            key = f"{FAMNAMES[fam]} {dtname} {name} {'groups' if grouped else 'no-groups'}"
            hier_e = bool(c["groups"]) or c["aux"]        # (the plain expanded model is bound by ahmc_set_target_glm: no β / τ)
            f, o = engine(hip, c), engine(hip, c, onehot=True)
            assert f.glm_factors() == (Px, list(levels)) and o.glm_factors() == (c["P"], [])
            nc, ng = C.c_int64(), C.c_int32()
            f._call("ahmc_hglm_get_target", C.byref(nc), C.byref(ng), None, None, None, None)
            assert (nc.value, ng.value) == (c["P"], len(c["groups"]))
            for which in ("small", "big"):
                with TG.tile_shape(which):
                    rf, ro = evaluate(f, c, c["th"]), evaluate(o, c, c["th"], hier=hier_e)
                    f.sync()
                    o.sync()
                factor_check(f"{key} {which}", c, rf["W"], eta=rf["eta"])
                if not c["groups"]:
                    record_bits(f"W {key} {which}", rf["W"], np.asfortranarray(c["th"][:c["P"]]))
                assert np.isfinite(rf["lp"]).all() and np.isfinite(rf["grad"]).all()
                for k in ro:
                    record_bits(f"one-hot-{k} {key} {which}", rf[k], ro[k])
            f.close()
            o.close()


# ---- §2 ----
def factor_tables(c):
    """GlmFacTab (int F, off[8], L[8]), the level indices (n_obs, F), and the permutations by level with their row pointers, as
    the host side lays them out"""
    n_obs = c["X"].shape[0]
    tab = np.zeros(17, dtype=np.int32)
    tab[0] = len(c["factors"])
    perm, rp = [], [0]
    for f, ((lo, _), fac) in enumerate(zip(c["ranges"], c["factors"])):
        tab[1 + f], tab[9 + f] = lo, fac.n_levels
        perm.append(np.argsort(fac.index, kind="stable"))
        rp.extend(f * n_obs + np.cumsum(np.bincount(fac.index, minlength=fac.n_levels)))
    lev = np.column_stack([fac.index for fac in c["factors"]])
    return tab, lev, np.concatenate(perm).astype(np.int32), np.asarray(rp, dtype=np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_new_kernels_on_a_chain_list(hip, probe_f, dtype):
    """k_glm_eta_f (both tile shapes, a legacy family and one with a dispersion), k_glm_grad_ld (both tile shapes), k_glm_gsum_ld and
    k_glm_fgrad launched from the probe on all chains and on a scattered, reversed list: the listed columns carry the bits of the
    full launch, the others keep their NaN fill, both tile shapes give the same bits.  On the given U the factors' rows of R equal the
    host's ordered additions in the element type bit for bit, and all rows the slice-ordered chains over the expanded Xᵀ; η of the
    full launch is the engine's."""
    import torch

    dtype = np.dtype(dtype)
    tch = TG.TCH[dtype]
    N = N_CHAINS
    idx = np.arange(N)[::3][::-1].copy()
    rest = np.setdiff1d(np.arange(N), idx)
    for name, (n_obs, Px, levels) in CASES.items():
        for fam in (0, 4):
            c = fcase(name, fam, N, dtype.name)
            P, D, Lt, nrb, ns = c["P"], c["D"], sum(levels), (n_obs + 63) // 64, (n_obs + G.K_SLICE - 1) // G.K_SLICE
            key = f"{FAMNAMES[fam]} {dtype.name} {name}"
            e = engine(hip, c)
            eta_e, _ = e.glm_pointwise()
            W, _ = e.hglm_coefficients()
            e.close()
            tab, lev, perm, rp = factor_tables(c)
            X_d, Xt_d, y_d, off_d, W_d, th_d, U_d = (TG.dev(a) for a in (c["X"], c["Xt"], c["y"], c["off"], np.asfortranarray(W), c["th"], c["U"]))
            zero_d = torch.zeros(P, dtype=th_d.dtype, device="cuda")
            tab_d, lev_d, perm_d, rp_d = torch.from_numpy(tab).cuda(), TG.dev(lev), TG.dev(perm), TG.dev(rp)
            aux_p, aux_ld = (TA._ptr(th_d, D - 1), np.int64(D)) if c["aux"] else (TG.NULL, np.int64(0))

            def nan(*shape):
                return torch.full((int(np.prod(shape)),), float("nan"), dtype=th_d.dtype, device="cuda")

            out = {}
            for bn in (64, 16):
                eta_k = f"_ZN4ahmc11k_glm_eta_fI{tch}Li{fam}ELi{bn}EEEvPKT_S3_S3_S1_S3_PS1_S4_iilllPKiS4_S4_S3_lS4_PKNS_9GlmFacTabES6_"
                grad_k = f"_ZN4ahmc13k_glm_grad_ldI{tch}Li{bn}EEEvPKT_S3_S3_S3_PS1_S4_iilllPKii"
                for which, lst in (("all", None), ("list", idx)):
                    n = N if lst is None else lst.size
                    idx_d = TG.NULL if lst is None else TG.dev(lst)
                    Uo_d, part_d, ps_d, eta_d, ll_d, R_d, gs_d = nan(n_obs, N), nan(nrb, N), nan(nrb, N), nan(n_obs, N), nan(n_obs, N), nan(P, N), nan(ns, Px, N)
                    grid = (nrb * (((n + 63) // 64 + 7) // 8 * 8),) if bn == 64 else (nrb, (n + 15) // 16)
                    probe_f.launch(eta_k, grid, 256, X_d, y_d, off_d, dtype.type(c["scale"]), W_d, Uo_d, part_d, n_obs, int(Px), np.int64(P), np.int64(n), np.int64(N),
                                   idx_d, eta_d, ll_d, aux_p, aux_ld, ps_d if c["aux"] else TG.NULL, tab_d, lev_d)
                    nrbD = (Px + 63) // 64 * ns
                    grid = (nrbD * (((n + 63) // 64 + 7) // 8 * 8),) if bn == 64 else (nrbD, (n + 15) // 16)
                    probe_f.launch(grad_k, grid, 256, Xt_d, U_d, zero_d, W_d, R_d, gs_d, n_obs, int(Px), np.int64(P), np.int64(n), np.int64(N), idx_d, int(ns))
                    if ns > 1:
                        probe_f.launch(f"_ZN4ahmc13k_glm_gsum_ldI{tch}EEvPKT_S3_S3_PS1_illlPKii", (n * Px + 255) // 256, 256, gs_d, zero_d, W_d, R_d, int(Px), np.int64(P),
                                       np.int64(n), np.int64(N), idx_d, int(ns))
                    probe_f.launch(f"_ZN4ahmc11k_glm_fgradI{tch}EEvPKT_PKiS5_PS1_iiillS5_", (n * Lt + 255) // 256, 256, U_d, perm_d, rp_d, R_d, n_obs, int(Px), int(Lt),
                                   np.int64(P), np.int64(n), idx_d)
                    out[(bn, which)] = [TG.host(Uo_d, (n_obs, N)), TG.host(part_d, (N, nrb)).T, TG.host(eta_d, (n_obs, N)), TG.host(ll_d, (n_obs, N)), TG.host(R_d, (P, N))]
                    if c["aux"]:
                        out[(bn, which)].append(TG.host(ps_d, (N, nrb)).T)
            names = ("U", "partial", "eta", "loglik", "R", "partial_s")
            for bn in (64, 16):
                for nm, a, b, b64 in zip(names, out[(bn, "list")], out[(bn, "all")], out[(64, "all")]):
                    assert np.isfinite(b).all(), (nm, bn)
                    record_bits(f"chain-list-{nm}-bn{bn} {key}", a[:, idx], b[:, idx])
                    assert np.isnan(a[:, rest]).all(), (nm, bn)
                    record_bits(f"tile-shapes-{nm} {key}", b, b64)
            R = out[(64, "all")][4]
            for (lo, hi), fac in zip(c["ranges"], c["factors"]):
                want = -ordered_level_sums(c["U"], fac.index, fac.n_levels)
                np.testing.assert_array_equal(TG.bits_of(np.where(R[lo:hi] == 0, 0, R[lo:hi])), TG.bits_of(np.where(want == 0, 0, want)), err_msg=f"fgrad {key}")
                assert np.all(R[lo:hi][np.setdiff1d(np.arange(fac.n_levels), fac.index)] == 0)
            factor_check(f"probe {key}", c, W, eta=out[(64, "all")][2], Um=c["U"], R=R)
            record_bits(f"probe-eta-is-the-engine's {key}", out[(64, "all")][2], eta_e)


# ---- §3 ----
def all_stats_equal(a, b, what):
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def adapting_engine(hip, c, kern, onehot=False, adapt=True, **kw):
    D, N = c["D"], kw.get("cols", np.arange(c["th"].shape[1])).size
    e = engine(hip, c, onehot=onehot, metric=A.DiagEuclideanMetric((D, N)), **kw)
    e.set_integrator(kern.tau.integrator)
    if adapt:
        e.adaptor_init(A.StanHMCAdaptor(A.MassMatrixAdaptor(A.DiagEuclideanMetric((D, N))), A.StepSizeAdaptor(0.8, kern.tau.integrator), 5, 5, 5))
    return e


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_whole_run_equals_the_one_hot_model(hip, dtype):
    """20 adapting + 20 sampling NUTS transitions with StanHMCAdaptor on the (130, 3, (7, 1)) case: after every transition every
    statistic, θ, the step sizes and the metric equal the run of the expanded model"""
    c = fcase("two-factors", 0, N_CHAINS, np.dtype(dtype).name)
    kern = TG.nuts_kernel(N_CHAINS, eps=0.02)
    f, o = adapting_engine(hip, c, kern), adapting_engine(hip, c, kern, onehot=True)
    steps = 0
    for i in range(1, 41):
        for e in (f, o):
            e.transition(kern)
            e.adapt(i, 20)
        all_stats_equal(f.stats(), o.stats(), f"transition {i}")
        np.testing.assert_array_equal(f.theta(), o.theta(), err_msg=f"transition {i}")
        steps += int(f.stats()["n_steps"].sum())
    np.testing.assert_array_equal(f.get_stepsize(), o.get_stepsize())
    np.testing.assert_array_equal(f.get_metric(), o.get_metric())
    assert steps > 40 * N_CHAINS and not np.array_equal(f.get_metric(), np.ones((c["D"], N_CHAINS)))
    f.close()
    o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_chain_blocks_bulk_and_resume(hip, dtype):
    """bit for bit: engines over blocks of the chains == one engine (the evaluation and three NUTS transitions, on the two-slice
    case); the bulk run == the stepwise loop of transition + adapt; get_state after 11 of 24 → a fresh context → the rest"""
    dtname = np.dtype(dtype).name
    N = 48
    c = fcase("two-slices", 4, N, dtname)
    whole = engine(hip, c, seed=A.PhiloxRNG(17))
    ev = evaluate(whole, c)
    whole.run(TG.nuts_kernel(N, eps=0.02), 3)
    th_w, st_w = whole.theta(), whole.stats()
    whole.close()
    assert st_w["n_steps"].sum() > 3 * N
    for lo, hi in ((0, 5), (5, 22), (22, 48)):
        cols = np.arange(lo, hi)
        e = engine(hip, c, cols=cols, seed=A.PhiloxRNG(17, chain_offset=int(lo)))
        for k, a in evaluate(e, c).items():
            record_bits(f"blocks-{k} {dtname}", a, ev[k][..., cols])
        e.run(TG.nuts_kernel(hi - lo, eps=0.02), 3)
        record_bits(f"blocks-theta {dtname}", e.theta(), th_w[:, cols])
        all_stats_equal(e.stats(), {k: v[cols] for k, v in st_w.items()}, "chain blocks")
        e.close()
    c = fcase("two-factors", 0, N, dtname)
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
    whole.close()


@pytest.mark.gpu
def test_rebinding_leaves_no_trace(hip):
    """the factor model, then a plain GLMTarget of the same D on the same context == a fresh context on the plain model; and back"""
    N = N_CHAINS
    c = fcase("two-factors", 0, N, "float64")
    plain = TG.case(64, c["D"], N, 1, "float64")
    kern = TG.nuts_kernel(N)
    a = engine(hip, c)
    a.transition(TG.nuts_kernel(N, eps=0.02))
    a.set_target(A.GLMTarget(plain["X"], plain["y"], family=1, prior_prec=plain["p"], offset=plain["off"], scale=plain["scale"]))
    assert a.glm_factors() == (c["D"], [])
    a.seed(A.PhiloxRNG(7))
    a.set_integrator(A.Leapfrog(np.full(N, 0.05)))
    a.set_position(plain["th"])
    b = TG.glm_engine(hip, plain)
    for e in (a, b):
        e.run(kern, 3)
    np.testing.assert_array_equal(a.theta(), b.theta())
    all_stats_equal(a.stats(), b.stats(), "after re-binding")
    for x, y_ in zip(a.glm_pointwise(), b.glm_pointwise()):
        np.testing.assert_array_equal(x, y_)
    b.close()
    a.set_target(target(c))
    a.seed(A.PhiloxRNG(7))
    a.set_integrator(A.Leapfrog(np.full(N, 0.02)))
    a.set_position(c["th"])
    b = engine(hip, c)
    for e in (a, b):
        e.run(TG.nuts_kernel(N, eps=0.02), 3)
    np.testing.assert_array_equal(a.theta(), b.theta())
    all_stats_equal(a.stats(), b.stats(), "bound again")
    a.close()
    b.close()


# ---- §4 ----
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PARITY))
def test_against_oracle(hip, oracle, name):
    """the HIP engine on the target against the oracle on the mirror as a host kernel: static HMC, two NUTS transitions,
    find_good_stepsize, a bulk run of three (the wide context: two NUTS transitions at max_depth 3) — every discrete statistic of
    every chain, under the suite's margin rule; in the Poisson case most chains diverge in the first transition, on both engines"""
    t, minv, th0, eps = parity_inputs(*PARITY[name])
    N = th0.shape[1]
    o = TH.oracle_engine(oracle, t, parity_metric(name, t, minv, N), N)
    g = A.Engine(A.Hamiltonian(parity_metric(name, t, minv, N), t), N, rng=A.PhiloxRNG(8), lib=hip)
    if name == "wide":
        assert g.info("wide") and t.D > 4096
        TG.parity_sequence(o, g, th0, eps, f"glm-factor {name}", nuts_depth=3, full=False)
    else:
        TG.parity_sequence(o, g, th0, eps, f"glm-factor {name}")
    g.close()
    o.close()
    if "divergent" in name:
        g = A.Engine(A.Hamiltonian(parity_metric(name, t, minv, N), t), N, rng=A.PhiloxRNG(8), lib=hip)
        first = TH.first_transition_divergences(g, th0, eps)
        g.close()
        assert first > N // 2, first


# ---- §5 ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_refusals(hip, dtype):
    """every refusal of the header, with the status and message class of the Python side; after each refused call the context still
    runs a transition on the model it had"""
    N = 17
    c = fcase("two-factors", 0, N, np.dtype(dtype).name)
    e = engine(hip, c)
    kern = TG.nuts_kernel(N, eps=0.02)
    n_obs, Px, P, groups = 130, c["Px"], c["P"], c["groups"]
    X, y, off, p = np.asfortranarray(c["X"]), c["y"].copy(), c["off"].copy(), c["p"].copy()
    lev0 = np.asfortranarray(np.column_stack([f.index for f in c["factors"]]), dtype=np.int32)

    def arr(ct, vals):
        return (ct * max(1, len(vals)))(*vals)

    def still_runs():
        e.transition(kern)
        assert np.isfinite(e.theta()).all() and e.stats()["n_steps"].min() >= 1
        assert e.glm_factors() == (Px, [7, 1])

    def refused(exc, match, fam=0, n_coef=Px, grp=groups, levels=(7, 1), lev=lev0, n_factors=None, has_aux=0, aux=(0.0, 1.0), null=(), n=n_obs, p_=p):
        lo, hi = arr(C.c_int32, [g[0] for g in grp]), arr(C.c_int32, [g[1] for g in grp])
        cen, Asc = arr(C.c_int32, [int(g[2]) for g in grp]), arr(C.c_double, [g[3] for g in grp])
        with pytest.raises(exc, match=match):
            e._call("ahmc_glm_factor_set_target", fam, n, n_coef, capi.as_ptr(X), capi.as_ptr(y), capi.as_ptr(off), capi.as_ptr(p_), c["scale"], len(grp), lo, hi,
                    cen, Asc, len(levels) if n_factors is None else n_factors, None if "n_levels" in null else arr(C.c_int32, levels),
                    None if "levels" in null else lev.ctypes.data_as(C.POINTER(C.c_int32)), has_aux, aux[0], aux[1])
        still_runs()

    def poked(i, f, v):
        b = lev0.copy(order="F")
        b[i, f] = v
        return b

    refused(A.ArgumentError, "DomainError.*outside", lev=poked(129, 0, 7))
    refused(A.ArgumentError, "DomainError.*outside", lev=poked(0, 1, -1))
    refused(A.ArgumentError, "DomainError.*n_levels", levels=(7, 0))
    refused(A.UnsupportedError, "AHMC_GLM_FACTOR_MAX", levels=(1,) * 9, lev=np.zeros((n_obs, 9), dtype=np.int32, order="F"))
    refused(A.ArgumentError, "n_factors", n_factors=-1)
    refused(A.ArgumentError, "DimensionMismatch", n_coef=0)
    refused(A.ArgumentError, "DimensionMismatch", n_coef=Px + 1)
    refused(A.ArgumentError, "DimensionMismatch", levels=(7,))
    refused(A.ArgumentError, "DimensionMismatch", has_aux=1, fam=4)
    refused(A.ArgumentError, "NULL", null=("levels",))
    refused(A.ArgumentError, "NULL", null=("n_levels",))
    # the neighbours' refusals come through
    refused(A.ArgumentError, "ArgumentError.*overlaps", grp=((3, 10, False, 1.0), (9, 11, True, 1.0)))
    refused(A.ArgumentError, "ArgumentError.*out of bounds", grp=((3, 10, False, 1.0), (10, 12, True, 1.0)))
    refused(A.ArgumentError, "unknown family", fam=4)
    refused(A.ArgumentError, "no sampled dispersion", has_aux=1, grp=groups[:1])
    refused(A.ArgumentError, "ArgumentError.*member of group", p_=np.where(np.arange(P) == 4, 0.5, p).astype(p.dtype))
    refused(A.UnsupportedError, "AHMC_GLM_MAX_OBS", n=(1 << 24) + 1)
    e.close()
    # the Python side refuses the same models before the call
    for bad in (lambda: A.Factor(poked(129, 0, 7)[:, 0], 7), lambda: A.Factor(poked(0, 1, -1)[:, 1], 1), lambda: A.Factor(lev0[:, 0], 0)):
        with pytest.raises(A.ArgumentError, match="DomainError"):
            bad()
    # without a GLM bound
    d = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((8, N)), A.IsoGaussian(8)), N, dtype=dtype, rng=A.PhiloxRNG(1), lib=hip)
    with pytest.raises(A.ArgumentError, match="no GLM is bound"):
        d.glm_factors()
    with pytest.raises(A.ArgumentError, match="DimensionMismatch"):
        d.set_target(target(c))
    d.close()
