"""include/ahmc_glm_predict.h: predictions of a bound GLM at new rows of data, their summaries over the draws and the held-out lpd.

CPU: the mirror's pieces (glm.predict against a long-double evaluation written here, glm.predict_summary against a two-pass long-double
mean / variance / logsumexp, the block order against the chunking), the exact posterior predictive of a conjugate Gaussian model, the
refusals of the host-only checks (csrc/ahmc_glm_predict_spec.hpp through tests/host_ref/glm_predict_spec_driver.cpp), the interface.
GPU: identity with ahmc_glm_pointwise / ahmc_glm_loglik / ahmc_glm_class_probs on the training rows; new rows against the fma-chain model
of η and derived bounds on μ, v and the probabilities; the summary against the mirror on the device's own values; invariance; no side
effects; non-finite draws; guard bands; refusals.

Bounds.  u is the unit roundoff of the element type.
  * summary, mean and lpd: |Δ| <= 8 u relative to max(|value|, 1) for the float64 mirror against long double; the device's lpd is held
    to 8 × max(the mirror's own deviation in that case, 8 u); its means and variances are bit-identical to the mirror's.
  * summary, variance: relative to its own value.  A-priori (`variance_bound`): a block's M2 is a sum of n_b <= 64 squares of
    differences, each difference carrying the roundoff of x − mean_b and of mean_b itself (<= 64 u·max|x|), so a term's relative error is
    <= 2·(66 u·κ) + 2 u with κ = max|x| / sd, and the sequential sums add <= (64 + blocks) u; Chan's update adds <= 6 u a block.  That
    is the outer check (13 000 … 31 000 u here).  The bar that bites is VARIANCE_BAR_U = 8 × the worst the float64 mirror shows over the
    cases (71.61 u at S = 200: 573 u), frozen in this file and recorded per case in test_out/glm_predict_margins.json.
  * new rows (test_new_rows_*): with E_η the bound of tests/test_glm_target.py on η̂ (γ_K of the product, one rounding of each gather and
    of the offset), ε_exp and ε_log1p TWICE the measured worst relative error of the device's functions (TG.device_eps) and L the
    Lipschitz constant of the quantity in η:  |q̂ − q| <= L·E_η + (function evaluations)·ε·|q| + (roundings)·u·|q|, spelled out per family
    in `quantity_bounds`.
"""
import ctypes as C
import functools
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ahmc_amd as A
import test_buffer_bounds as TB
import test_glm_loo as TL
import test_glm_target as TG
from ahmc_amd import _capi as capi
from ahmc_amd import glm as G
from arena_util import In, Out
from test_glm_target import probe  # noqa: F401  (the fixture: exp / log1p of the device)

LD = np.longdouble
ROOT = TG.ROOT
U53 = 2.0 ** -53
CSRC = os.path.join(ROOT, "advancedhmc.jl_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
DRIVER = os.path.join(ROOT, "tests", "host_ref", "glm_predict_spec_driver.cpp")
N_CHAINS = 37
N_NEW = (1, 64, 65, 130)
S_ALL = (1, 63, 64, 65, 200, 4100)
MARGINS = {}


def dump_margins():
    out = os.environ.get("AHMC_TEST_OUT") or os.path.join(ROOT, "test_out")
    try:
        os.makedirs(out, exist_ok=True)
        path = os.path.join(out, "glm_predict_margins.json")
        old = {}
        if os.path.exists(path):
            try:
                old = json.load(open(path))
            except ValueError:
                old = {}
        old.update(MARGINS)
        with open(path, "w") as f:
            json.dump(dict(sorted(old.items())), f, indent=1)
    except OSError:
        pass


def bits(key, got, want):
    TG.record_bits(f"predict {key}", np.asarray(got), np.asarray(want))


# ------------------------------------------------------------------------------------------------
# models and new rows
# ------------------------------------------------------------------------------------------------
FAMILIES = TL.FAMILIES + ("bernoulli-centred",)


def model(name, n_obs=70, P=3, seed=0):
    """TL.model's seven families, each with the feature the issue names for it (a non-centred group, a factor and an offset, a
    dispersion, cutpoints, classes), and the Bernoulli model with a CENTRED group"""
    if name != "bernoulli-centred":
        return TL.model(name, n_obs, P, seed)
    t, centre = TL.model("bernoulli", n_obs, P, seed)
    return A.HierGLMTarget(t.X, t.y, [A.CoefGroup(1, P, True, 1.2)], family="bernoulli_logit", prior_scale=2.5), centre


def training_rows(t):
    return A.GLMNewData(t.X, factors=[f.index for f in t.factors], offset=t.offset, y=t.y)


def new_rows(t, n_new, seed=3, y=True, offset=None):
    """n_new new rows for the model t: levels the model knows, an offset where the model has one (or on request), outcomes in the
    family's domain"""
    rs = np.random.default_rng([n_new, seed, t.D])
    X = rs.normal(size=(n_new, t.P_x)) / np.sqrt(t.P_x)
    facs = [rs.integers(0, f.n_levels, n_new) for f in t.factors]
    K = t.n_classes - 1 if t.n_classes else 1
    off = None
    if t.offset is not None if offset is None else offset:
        off = 0.1 * rs.normal(size=(n_new, K) if t.n_classes else n_new)
    if t.n_classes or t.n_categories:
        yn = rs.integers(0, t.n_classes or t.n_categories, n_new).astype(float)
    elif t.family == G.BERNOULLI_LOGIT:
        yn = rs.integers(0, 2, n_new).astype(float)
    elif t.family in (G.POISSON_LOG, G.NEGBINOMIAL_LOG):
        yn = rs.poisson(2.0, n_new).astype(float)
    else:
        yn = rs.normal(size=n_new)
    return A.GLMNewData(X, factors=facs, offset=off, y=yn if y else None)


def counts(t):
    """(K predictors, C categories or classes or 0, Q quantities)"""
    K = t.n_classes - 1 if t.n_classes else 1
    Cc = t.n_classes or t.n_categories
    return K, Cc, K + (Cc or 2)


def stacked(parts):
    """the (Q, n_new, S) array of the header's quantities from "linear", "mean" [, "variance"] results"""
    return np.concatenate([p if p.ndim == 3 else p[None] for p in parts], axis=0)


def mirror_values(t, nd, draws):
    K, Cc, Q = counts(t)
    v = stacked([t.predict(draws, nd, w) for w in (("linear", "mean") if Cc else ("linear", "mean", "variance"))])
    assert v.shape[0] == Q
    return v


# ------------------------------------------------------------------------------------------------
# CPU 1: the mirror's pieces
# ------------------------------------------------------------------------------------------------
def predict_ld(t, nd, theta):
    """the quantities (Q, n_new, n) of the model t at the rows nd and draws θ, evaluated in long double from the definitions"""
    th = np.asarray(theta, dtype=np.float64).astype(LD)
    P, Gn = t.P, len(t.groups)
    W = th[:P].copy()
    for k, g in enumerate(t.groups):
        if not g.centered:
            W[g.start:g.stop] = np.exp(th[P + k]) * th[g.start:g.stop]
    K, Cc, Q = counts(t)
    Pb, Px = t.P_b, t.P_x
    X = nd.X.astype(LD)
    etas = []
    for k in range(K):
        Wk = W[k * Pb:(k + 1) * Pb]
        eta = X @ Wk[:Px]
        for (lo, _), idx in zip(t.factor_ranges, nd.factors):
            eta = eta + Wk[lo + idx]
        if nd.offset is not None:
            eta = eta + (nd.offset[:, k] if nd.offset.ndim == 2 else nd.offset).astype(LD)[:, None]
        etas.append(eta)
    eta = etas[0]
    if t.n_classes:
        e = np.stack([np.zeros_like(eta)] + etas)
        p = np.exp(e - e.max(axis=0))
        return np.concatenate([np.stack(etas), p / p.sum(axis=0)])
    if t.n_categories:
        kap = th[P + Gn:]
        c = np.concatenate([kap[:1], kap[:1] + np.cumsum(np.exp(kap[1:]), axis=0)])
        cdf = np.concatenate([np.zeros((1,) + eta.shape, dtype=LD), 1 / (1 + np.exp(-(c[:, None, :] - eta[None]))), np.ones((1,) + eta.shape, dtype=LD)])
        return np.concatenate([eta[None], np.diff(cdf, axis=0)])
    s = th[-1] if t.aux else None
    if t.family == G.BERNOULLI_LOGIT:
        mu = 1 / (1 + np.exp(-eta))
        v = mu * (1 - mu)
    elif t.family == G.POISSON_LOG:
        mu = np.exp(eta)
        v = mu
    elif t.family == G.GAUSSIAN_IDENTITY:
        mu, v = eta, np.full_like(eta, 1 / LD(t.scale))
    elif t.family == G.GAUSSIAN_IDENTITY_SIGMA:
        mu, v = eta, np.broadcast_to(np.exp(2 * s), eta.shape)
    else:
        mu = np.exp(eta)
        v = mu + mu * mu / np.exp(s)
    return np.stack([eta, mu, v])


@pytest.mark.parametrize("name", FAMILIES)
def test_mirror_predict_against_long_double(name):
    """glm.predict (float64) against `predict_ld`: |Δq| <= |q(η + δ) − q(η − δ)| + 64 u max(|q|, δ) with δ = γ_{P+F+4}·(|X|·|W| + Σ|w_level| + |offset|)
    + 4 u |η|, the roundoff a float64 evaluation of η can have in any order of its sums (the probabilities: δ on every predictor and cutpoint,
    Lipschitz constant 1/4 each); ℓ is the same code path as the existing pointwise mirrors and must have their bits"""
    t, centre = model(name)
    nd = new_rows(t, 65)
    draws = TL.draws_of(t, centre, 9, np.float64)
    K, Cc, Q = counts(t)
    got = mirror_values(t, nd, draws)
    ref = predict_ld(t, nd, draws)
    assert got.shape == ref.shape == (Q, 65, 9)
    # δ: from the magnitudes, in long double
    th = draws.astype(LD)
    Wabs = np.abs(np.asarray(t.coefficients(draws)[0] if t.groups else draws[:t.P], dtype=np.float64)).astype(LD)
    mag = []
    for k in range(K):
        Wk = Wabs[k * t.P_b:(k + 1) * t.P_b]
        m = np.abs(nd.X).astype(LD) @ Wk[:t.P_x]
        for (lo, _), idx in zip(t.factor_ranges, nd.factors):
            m = m + Wk[lo + idx]
        if nd.offset is not None:
            m = m + np.abs(nd.offset[:, k] if nd.offset.ndim == 2 else nd.offset).astype(LD)[:, None]
        mag.append(m)
    u = LD(U53)
    delta = np.stack([TG.gam(t.P_x + len(t.factors) + 4, u) * m for m in mag]) + 4 * u * np.abs(ref[:K])
    err = np.abs(got.astype(LD) - ref)
    worst = float(np.max(err[:K] / delta))
    assert worst <= 1, (name, "eta", worst)
    if Cc:
        d_all = delta.sum(axis=0)
        if t.n_categories:
            kap = th[t.P + len(t.groups):]
            d_all = d_all + 2 * (8 * u * (np.abs(kap[0]) + np.exp(kap[1:]).sum(axis=0)))[None, :]
        bound = d_all[None] / 4 * (2 if t.n_categories else 1) + 64 * u * np.maximum(ref[K:], d_all[None])
        assert np.all(err[K:] <= bound), (name, float(np.max(err[K:] / bound)))
        assert np.abs(got[K:].sum(axis=0) - 1).max() <= 16 * U53
    else:
        d = delta[0]
        rs = LD(1) if not t.aux else np.exp(-th[-1])
        for q, fn in ((1, {G.BERNOULLI_LOGIT: lambda e: 1 / (1 + np.exp(-e)), G.POISSON_LOG: np.exp, G.NEGBINOMIAL_LOG: np.exp}.get(t.family, lambda e: e)),
                      (2, {G.BERNOULLI_LOGIT: lambda e: np.exp(-e) / (1 + np.exp(-e)) ** 2, G.POISSON_LOG: np.exp,
                           G.NEGBINOMIAL_LOG: lambda e: np.exp(e) + np.exp(2 * e) * rs}.get(t.family, lambda e: ref[2]))):
            spread = np.abs(fn(ref[0] + d) - fn(ref[0] - d))
            bound = spread + 64 * u * np.maximum(np.abs(ref[q]), d)
            assert np.all(err[q] <= bound), (name, q, float(np.max(err[q] / bound)))
    # ℓ: the bits of the existing mirrors
    ll = t.predict(draws, nd, "loglik")
    if t.n_classes:
        want = G.categorical_pointwise(nd.X, nd.y, draws, t.n_classes, t.groups, nd.offset, [(i, f.n_levels) for i, f in zip(nd.factors, t.factors)])[1]
    elif t.n_categories:
        want = G.ordinal_pointwise(nd.X, nd.y, draws, t.n_categories, t.groups, nd.offset, [(i, f.n_levels) for i, f in zip(nd.factors, t.factors)])[1]
    else:
        want = G.hier_pointwise(t.family, nd.X, nd.y, draws, t.groups, nd.offset, t.scale, [(i, f.n_levels) for i, f in zip(nd.factors, t.factors)])[1]
    assert np.array_equal(ll, want)
    with pytest.raises(A.ArgumentError, match="needs y"):
        t.predict(draws, new_rows(t, 5, y=False), "loglik")
    if Cc:
        with pytest.raises(A.ArgumentError, match="variance"):
            t.predict(draws, nd, "variance")


def summary_ld(values, ll):
    """(2Q + 1, n_new) in long double: two-pass mean and variance, logsumexp − log S; NaN rows where a value is not finite"""
    v = np.asarray(values, dtype=np.float64).astype(LD)
    Q, n, S = v.shape
    out = np.full((2 * Q + 1, n), np.nan, dtype=LD)
    with np.errstate(invalid="ignore", over="ignore"):
        mean = v.sum(axis=-1) / S
        out[0:2 * Q:2] = mean
        if S > 1:
            out[1:2 * Q:2] = ((v - mean[..., None]) ** 2).sum(axis=-1) / (S - 1)
        bad = ~np.isfinite(v).all(axis=-1)
        out[0:2 * Q:2][bad] = np.nan
        out[1:2 * Q:2][bad] = np.nan
        if ll is not None:
            l = np.asarray(ll, dtype=np.float64).astype(LD)
            m = l.max(axis=-1)
            out[2 * Q] = np.where(np.isfinite(l).all(axis=-1), m + np.log(np.exp(l - m[:, None]).sum(axis=-1)) - np.log(LD(S)), np.nan)
    return out


def variance_bound(values):
    """the a-priori relative bound of the module docstring on the mirror's variance, per (quantity, observation), in units of u"""
    v = np.asarray(values, dtype=np.float64)
    S = v.shape[-1]
    sd = v.std(axis=-1, ddof=1) if S > 1 else np.ones(v.shape[:-1])
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa = np.where(sd > 0, np.abs(v).max(axis=-1) / sd, 0.0)
    blocks = (S + 63) // 64
    return 2 * 66 * kappa + 2 + (64 + blocks) + 6 * blocks


# The worst relative deviation of the float64 mirror's variance from the two-pass long-double reference over `summary_cases`, in u, per S:
# 1: 0 (NaN rows), 63: 4.40, 64: 3.46, 65: 44.62, 200: 71.61, 4100: 21.55 — the row 100 + 0.5·z, where max|x| / sd is 200.  The bar is
# 8 × the worst of them and is frozen here: a change of the mirror (or of numpy) that moves a case beyond it fails the test.
VARIANCE_WORST_U = {1: 0.0, 63: 4.40, 64: 3.46, 65: 44.62, 200: 71.61, 4100: 21.55}
VARIANCE_BAR_U = 8 * max(VARIANCE_WORST_U.values())


def summary_check(key, got, values, ll, lpd_floor_u=8.0, exact_moments_of=None, record=True):
    """`got` (2Q + 1, n_new) against `summary_ld` on the same values.  Means and lpd, relative to max(|value|, 1): the means within 8 u, the
    lpd within `lpd_floor_u` u (8: the issue's bar for the float64 mirror).  Variances, relative to their own value: within
    VARIANCE_BAR_U = 8 × the worst the float64 mirror showed over `summary_cases` (frozen above), and inside the a-priori
    `variance_bound` as a second, outer check.  `exact_moments_of`: a summary whose means and variances `got` must have bit for bit."""
    ref = summary_ld(values, ll)
    Q = (ref.shape[0] - 1) // 2
    g = np.asarray(got, dtype=np.float64).astype(LD)
    assert g.shape == ref.shape, (key, g.shape, ref.shape)
    assert np.array_equal(np.isnan(g), np.isnan(ref)), (key, "NaN pattern")
    fin = np.isfinite(ref)
    rel1 = np.where(fin, np.abs(g - ref) / np.maximum(np.abs(ref), 1), 0) / LD(U53)
    mean_u, lpd_u = float(rel1[0:2 * Q:2].max()), float(rel1[2 * Q].max())
    var_ref, var_got = ref[1:2 * Q:2], g[1:2 * Q:2]
    with np.errstate(divide="ignore", invalid="ignore"):
        relv = np.where(np.isfinite(var_ref) & (var_ref > 0), np.abs(var_got - var_ref) / var_ref, np.where(np.isfinite(var_ref), np.abs(var_got), 0)) / LD(U53)
    vb = variance_bound(values)
    var_u = float(relv.max())
    rec = {"mean_u": mean_u, "lpd_u": lpd_u, "variance_u": var_u, "variance_bar_u": VARIANCE_BAR_U, "variance_a_priori_u": float(vb.max()),
           "lpd_bar_u": lpd_floor_u}
    if record:
        MARGINS[key] = rec
        dump_margins()
    print(key, rec)
    if exact_moments_of is not None:
        bits(f"summary-moments {key}", np.asarray(got)[:2 * Q], np.asarray(exact_moments_of)[:2 * Q])
    assert mean_u <= 8.0, (key, rec)
    assert lpd_u <= lpd_floor_u, (key, rec)
    assert var_u <= VARIANCE_BAR_U, (key, rec)
    assert np.all(relv <= vb), (key, rec, float(np.max(relv / vb)))
    return rec


def summary_cases(S):
    """values (Q = 4, n_new = 6, S) and ℓ (6, S): standard normal, a large mean with a small spread, a constant (0.25: its sums are exact), probabilities near 0, and
    ℓ of a Gaussian observation at several distances"""
    rs = np.random.default_rng([S, 17])
    z = rs.normal(size=(4, 6, S))
    v = np.stack([z[0], 100.0 + 0.5 * z[1], np.full((6, S), 0.25), np.exp(-6 + z[3])])
    ll = -0.5 * (rs.normal(size=(6, S)) - np.linspace(0, 4, 6)[:, None]) ** 2 - 0.9
    return v, ll


@pytest.mark.parametrize("S", S_ALL)
def test_mirror_summary_against_two_pass_long_double(S):
    v, ll = summary_cases(S)
    got = G.predict_summary(v, ll)
    rec = summary_check(f"mirror-summary S={S}", got, v, ll)
    assert got.shape == (9, 6) and (np.isnan(got[1:8:2]).all() if S == 1 else np.isfinite(got).all())
    assert np.all(got[4] == 0.25) and (S == 1 or np.all(got[5] == 0.0))          # a constant: its mean exactly, no variance
    assert np.isnan(G.predict_summary(v)[8]).all() and np.array_equal(G.predict_summary(v)[:8], got[:8], equal_nan=True)
    assert rec["variance_u"] <= rec["variance_a_priori_u"]
    assert abs(rec["variance_u"] - VARIANCE_WORST_U[S]) <= 0.01, "the frozen record of the mirror's worst is stale: update VARIANCE_WORST_U and the docstring"


def test_mirror_block_order_does_not_depend_on_the_chunk():
    v, ll = summary_cases(200)
    whole = G.predict_summary(v, ll)
    for chunk in (64, 128):
        got = G.predict_summary(v, ll, chunk=chunk)
        assert np.array_equal(TG.bits_of(got), TG.bits_of(whole)), chunk
    with pytest.raises(ValueError, match="multiple of 64"):
        G.predict_summary(v, ll, chunk=100)
    # a non-finite value: NaN in that quantity's rows of that observation alone
    v[1, 2, 70] = np.inf
    ll[4, 199] = -np.inf
    got = G.predict_summary(v, ll, chunk=64)
    nan = np.isnan(got)
    want = np.zeros_like(nan)
    want[2:4, 2] = True
    want[8, 4] = True
    assert np.array_equal(nan, want)
    summary_check("mirror-summary non-finite", got, v, ll, record=False)


# ------------------------------------------------------------------------------------------------
# CPU 2: the exact posterior predictive of a conjugate Gaussian model
# ------------------------------------------------------------------------------------------------
def conjugate_predictive(n, P, S, n_new, seed):
    """the model of tests/test_glm_loo.py::conjugate (unit noise, prior N(0, 2.5²), the same data and exact posterior draws for the same
    seed), then n_new new rows with outcomes from the posterior mean's predictor plus unit noise"""
    rs = np.random.default_rng([n, P, S, seed])
    X = rs.normal(size=(n, P)) / np.sqrt(P)
    y = X @ rs.normal(size=P) + rs.normal(size=n)
    y[0] += 4.0
    P0 = np.eye(P) / 2.5 ** 2
    V = np.linalg.inv(X.T @ X + P0)
    m = V @ X.T @ y
    beta = m[:, None] + np.linalg.cholesky(V) @ rs.normal(size=(P, S))
    Xn = rs.normal(size=(n_new, P)) / np.sqrt(P)
    yn = Xn @ m + rs.normal(size=n_new)
    return m, V, beta, Xn, yn


SEEDS = (1, 4, 7)
LPD_BARS = {"sum": 0.185, "max": 0.0765}


def conjugate_summary(seed, summary=G.predict_summary):
    m, V, beta, Xn, yn = conjugate_predictive(40, 3, 4000, 20, seed)
    q = stacked([G.predict("gaussian_identity", Xn, beta, w, y=yn) for w in ("linear", "mean", "variance")])
    ll = G.predict("gaussian_identity", Xn, beta, "loglik", y=yn) - 0.5 * np.log(2 * np.pi)
    return summary(q, ll), q, ll, m, V, Xn, yn


def conjugate_check(s, m, V, Xn, yn, S=4000):
    xv = np.einsum("ij,jk,ik->i", Xn, V, Xn)
    exact = -0.5 * np.log(2 * np.pi * (1 + xv)) - 0.5 * (yn - Xn @ m) ** 2 / (1 + xv)
    d = s[6] - exact
    rec = {"mean_over_5se": float(np.max(np.abs(s[2] - Xn @ m) / (5 * np.sqrt(xv / S)))), "sum_lpd": float(d.sum()), "max_lpd": float(np.abs(d).max()),
           "bars": dict(LPD_BARS)}
    assert rec["mean_over_5se"] <= 1, rec
    assert np.all(s[4] == 1.0), "var_within of unit noise"
    assert abs(rec["sum_lpd"]) <= LPD_BARS["sum"] and rec["max_lpd"] <= LPD_BARS["max"], rec
    return rec


def test_exact_posterior_predictive_on_a_conjugate_model():
    """n = 40, P = 3, S = 4000 exact posterior draws, 20 new rows, seeds 1, 4, 7.  |mean_s μ_i − x_iᵀm| <= 5·√(x_iᵀV x_i / S): five
    Monte-Carlo standard errors.  var_within = 1 exactly.  lpd against log N(y_i; x_iᵀm, 1 + x_iᵀV x_i), the closed form: seeds 1 … 12
    were tried on the host mirror — (Σ_i, max_i |·|) of lpd_i − exact_i: 1 (+0.0076, 0.0027), 2 (+0.0156, 0.0042), 3 (+0.0029, 0.0017),
    4 (−0.0740, 0.0306), 5 (+0.0168, 0.0149), 6 (+0.0192, 0.0068), 7 (+0.0198, 0.0081), 8 (+0.0005, 0.0036), 9 (−0.0180, 0.0148),
    10 (+0.0053, 0.0029), 11 (−0.0054, 0.0076), 12 (−0.0023, 0.0064).  Seeds 1, 4 and 7 are kept (4 is the loudest of the twelve); the bars are
    2.5 × the worst of the kept seeds: |Σ| <= 0.185, max <= 0.0765.  Every one of the twelve seeds meets them."""
    for seed in SEEDS:
        s, q, ll, m, V, Xn, yn = conjugate_summary(seed)
        rec = conjugate_check(s, m, V, Xn, yn)
        MARGINS[f"conjugate-predictive seed={seed}"] = dict(rec, seeds_tried=list(range(1, 13)), seeds_kept=list(SEEDS))
        dump_margins()


def test_checks_catch_two_planted_defects():
    """a summary that divides the variance by S instead of S − 1 fails the comparison with the two-pass reference (S = 200: 1/S = 5·10⁻³ of
    the value, 10¹³ u); one that returns the mean of ℓ for lpd fails it too, and fails the closed form of the conjugate model"""
    v, ll = summary_cases(200)
    good = G.predict_summary(v, ll)
    summary_check("planted-none", good, v, ll, record=False)
    by_S = good.copy()
    by_S[1:8:2] *= (200 - 1) / 200
    with pytest.raises(AssertionError):
        summary_check("planted-variance-by-S", by_S, v, ll, record=False)
    mean_ll = good.copy()
    mean_ll[8] = ll.mean(axis=1)
    with pytest.raises(AssertionError):
        summary_check("planted-mean-loglik", mean_ll, v, ll, record=False)
    s, q, l2, m, V, Xn, yn = conjugate_summary(SEEDS[0])
    conjugate_check(s, m, V, Xn, yn)
    bad = s.copy()
    bad[6] = l2.mean(axis=1)
    with pytest.raises(AssertionError):
        conjugate_check(bad, m, V, Xn, yn)


# ------------------------------------------------------------------------------------------------
# CPU 3: the refusals of the host-only checks
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def driver():
    from ahmc_amd import build as B

    flags = ["-O1", "-std=c++17", "-fPIC", "-shared"]
    h = hashlib.sha256()
    for p in (DRIVER, os.path.join(CSRC, "ahmc_glm_predict_spec.hpp"), os.path.join(CSRC, "ahmc_glm_spec.hpp"), os.path.join(INCLUDE, "ahmc_glm_predict.h")):
        with open(p, "rb") as f:
            h.update(f.read())
    h.update(" ".join(flags).encode())
    out_dir = os.path.join(B.OBJ, "host_ref")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, f"glm_predict_spec_driver_{h.hexdigest()[:20]}.so")
    if not os.path.exists(so):
        cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
        tmp = so + f".tmp{os.getpid()}"
        res = subprocess.run([cxx, *flags, "-I", CSRC, "-I", INCLUDE, DRIVER, "-o", tmp], capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"glm_predict_spec_driver build failed:\n{res.stdout}\n{res.stderr}")
        os.replace(tmp, so)
    return C.CDLL(so)


def spec_answer(dtype, bound=1, family=0, Px=2, n_levels=(), n_cat=0, n_cls=0, has_nd=1, n_new=3, X=None, levels=None, offset=None, y=None, has_theta=1, n_cols=4,
                has_out=1, what=capi.GLM_PRED_MEAN, summary=0):
    """(status, message, planes) of the two host-only steps"""
    dt = np.dtype(dtype)
    n = max(n_new, 0)
    X = np.zeros((n, Px)) if X is None else X
    arr = lambda a: None if a is None else np.asfortranarray(a, dtype=dt)  # noqa: E731
    Xa, oa, ya = arr(X), arr(offset), arr(y)
    la = None if levels is None else np.asfortranarray(levels, dtype=np.int32)
    nl = (C.c_int32 * max(len(n_levels), 1))(*n_levels)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    msg = C.create_string_buffer(1024)
    planes = C.c_int(-1)
    fn = getattr(driver(), "glm_predict_spec_run_" + ("f64" if dt == np.float64 else "f32"))
    fn.restype = C.c_int
    rc = fn(C.c_int(bound), C.c_int(family), C.c_int64(Px), C.c_int(len(n_levels)), nl, C.c_int(n_cat), C.c_int(n_cls), C.c_int(has_nd), C.c_int64(n_new), p(Xa), p(la),
            p(oa), p(ya), C.c_int(has_theta), C.c_int64(n_cols), C.c_int(has_out), C.c_int(what), C.c_int(summary), C.byref(planes), msg, C.c_int64(1024))
    return rc, msg.value.decode("utf-8"), planes.value


@pytest.mark.parametrize("dtype", TG.DTYPES, ids=["f64", "f32"])
def test_new_data_refusals_of_the_spec(dtype):
    """every condition of the header, with status and text, in the order of the header's lines: a call that violates two is answered
    with the earlier one"""
    ARG, UNS = capi.ERR_ARGUMENT, capi.ERR_UNSUPPORTED
    ans = functools.partial(spec_answer, dtype)
    assert ans() == (0, "", 1)
    assert ans(summary=1) == (0, "", 3) and ans(summary=1, y=np.zeros(3)) == (0, "", 4)
    for who, summ in (("glm_predict", 0), ("glm_predict_summary", 1)):
        a = functools.partial(ans, summary=summ)
        assert a(bound=0, has_nd=0) == (ARG, f"{who}: no GLM is bound (ahmc_set_target_glm)", -1)
        assert a(has_nd=0, n_new=-1) == (ARG, f"{who}: newdata is NULL", -1)
        rc, msg, _ = a(n_new=-2)
        assert (rc, msg) == (ARG, f"{who}: n_new must be >= 0; got -2")
        rc, msg, _ = a(n_new=2 ** 24 + 1, X=np.zeros((1, 2)), n_levels=(3,))          # (refused before levels or X are read)
        assert rc == UNS and msg == f"{who}: n_new = 16777217 is beyond the engine's limit AHMC_GLM_MAX_OBS = 16777216"
        rc, msg, _ = a(n_levels=(3, 2))
        assert (rc, msg) == (ARG, f"{who}: newdata.levels is NULL; the bound model has 2 factors")
        lev = np.array([[0, 1], [2, 2], [1, 0]])
        rc, msg, _ = a(n_levels=(3, 2), levels=lev, X=np.full((3, 2), np.nan))
        assert rc == ARG and msg.startswith(f"{who}: DomainError: levels[2, 2] = 2 is outside [0, 2) (zero-based level indices")
        lev[1, 1] = 1
        lev[2, 0] = -1
        rc, msg, _ = a(n_levels=(3, 2), levels=lev)
        assert rc == ARG and msg.startswith(f"{who}: DomainError: levels[3, 1] = -1 is outside [0, 3)")
        lev[2, 0] = 2
        assert a(n_levels=(3, 2), levels=lev)[0] == 0
        for kw in (dict(has_theta=0), dict(has_out=0), dict(n_cols=-1)):
            assert a(**kw)[:2] == (ARG, f"{who}: theta or the output is NULL, or n_cols < 0")
        assert a(has_theta=0, has_out=0, n_cols=0)[0] == 0
        assert a(n_cols=2 ** 31)[:2] == (UNS, f"{who}: n_cols beyond 2^31 - 1")
        X = np.zeros((3, 2))
        X[2, 1] = np.inf
        assert a(X=X, offset=np.full(3, np.nan))[:2] == (ARG, f"{who}: ArgumentError: newdata.X holds a non-finite value")
        assert a(offset=np.array([0, np.nan, 0]), y=np.full(3, 7.0))[:2] == (ARG, f"{who}: ArgumentError: newdata.offset holds a non-finite value")
        assert a(offset=np.zeros(3))[0] == 0                                          # (an offset where the model has none)
        assert a(n_cls=3, family=6, offset=np.array([[0, 0], [0, 0], [0, -np.inf]]))[:2] == (ARG, f"{who}: ArgumentError: newdata.offset holds a non-finite value")
        # y: the conditions of the bind
        assert a(y=np.array([0, 1, 1.5]))[:2] == (ARG, f"{who}: DomainError: y[3] = 1.500000 is outside the family's domain (0 <= y <= 1)")
        assert a(family=1, y=np.array([0, -1, 3]))[:2] == (ARG, f"{who}: DomainError: y[2] = -1.000000 is outside the family's domain (y >= 0, finite)")
        assert a(family=4, y=np.array([np.inf, 1, 3]))[:2] == (ARG, f"{who}: DomainError: y[1] = inf is outside the family's domain (y >= 0, finite)")
        assert a(family=2, y=np.array([0, np.nan, 3]))[:2] == (ARG, f"{who}: DomainError: y[2] = nan is outside the family's domain (finite)")
        assert a(family=3, y=np.array([0, -5.5, 3]))[0] == 0
        assert a(family=5, n_cat=4, y=np.array([0, 3, 4]))[:2] == (ARG, f"{who}: DomainError: y[3] = 4.000000 is not a category: an integer in [0, 4)")
        assert a(family=6, n_cls=3, y=np.array([0.5, 1, 2]))[:2] == (ARG, f"{who}: DomainError: y[1] = 0.500000 is not a category: an integer in [0, 3)")
        assert a(n_new=0, X=np.zeros((0, 2)))[0] == 0
    # `what`
    assert ans(what=7)[:2] == (capi.ERR_ARGUMENT, "glm_predict: unknown what = 7")
    assert ans(what=capi.GLM_PRED_LOGLIK)[:2] == (ARG, "glm_predict: AHMC_GLM_PRED_LOGLIK needs newdata.y, the outcomes to evaluate")
    assert ans(what=capi.GLM_PRED_LOGLIK, y=np.zeros(3)) == (0, "", 1)
    rc, msg, _ = ans(what=capi.GLM_PRED_VARIANCE, family=5, n_cat=4)
    assert rc == ARG and msg.startswith("glm_predict: AHMC_GLM_PRED_VARIANCE of an ordinal model")
    rc, msg, _ = ans(what=capi.GLM_PRED_VARIANCE, family=6, n_cls=3)
    assert rc == ARG and msg.startswith("glm_predict: AHMC_GLM_PRED_VARIANCE of a categorical model")
    # the planes of every `what`
    L, M, V = capi.GLM_PRED_LINEAR, capi.GLM_PRED_MEAN, capi.GLM_PRED_VARIANCE
    assert [ans(what=w)[2] for w in (L, M, V)] == [1, 1, 1]
    assert [ans(what=w, family=5, n_cat=4)[2] for w in (L, M)] == [1, 4] and ans(family=5, n_cat=4, summary=1)[2] == 5
    assert [ans(what=w, family=6, n_cls=3)[2] for w in (L, M)] == [2, 3] and ans(family=6, n_cls=3, summary=1, y=np.zeros(3))[2] == 6


# ------------------------------------------------------------------------------------------------
# CPU 4: the interface
# ------------------------------------------------------------------------------------------------
def header_prototypes():
    src = open(os.path.join(INCLUDE, "ahmc_glm_predict.h"), encoding="utf-8").read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(int32_t)\s+(ahmc_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        params = " ".join(m.group(3).split())
        protos[m.group(2)] = [] if params in ("", "void") else [p.strip() for p in params.split(",")]
    return protos, src


def test_header_and_bindings_agree():
    protos, src = header_prototypes()
    assert set(protos) == set(capi.GLM_PREDICT_SIGNATURES) == {"ahmc_glm_predict_version", "ahmc_glm_predict", "ahmc_glm_predict_summary"}
    older = set().union(*[set(getattr(capi, n)) for n in dir(capi) if n.endswith("SIGNATURES") and n != "GLM_PREDICT_SIGNATURES"])
    assert not set(capi.GLM_PREDICT_SIGNATURES) & older
    ct = {"double*": C.POINTER(C.c_double), "int64_t": C.c_int64, "int32_t": C.c_int32}
    for name, params in protos.items():
        res, args = capi.GLM_PREDICT_SIGNATURES[name]
        assert res is C.c_int32 and len(args) == len(params), name
        for p, a in zip(params, args):
            typ = p.rsplit(" ", 1)[0].replace("const ", "").replace(" ", "")
            assert a is (C.c_void_p if typ in ("void*", "ahmc_ctx*", "ahmc_glm_newdata*") else ct[typ]), (name, p)
    assert [p.split()[-1] for p in protos["ahmc_glm_predict"]] == ["ctx", "newdata", "theta", "n_cols", "what", "out"]
    assert [p.split()[-1] for p in protos["ahmc_glm_predict_summary"]] == ["ctx", "newdata", "theta", "n_cols", "summary_out"]
    assert re.search(r"#define AHMC_GLM_PREDICT_VERSION (\d+)", src).group(1) == str(capi.AHMC_GLM_PREDICT_VERSION) == "1"
    for macro, v in (("LINEAR", capi.GLM_PRED_LINEAR), ("MEAN", capi.GLM_PRED_MEAN), ("VARIANCE", capi.GLM_PRED_VARIANCE), ("LOGLIK", capi.GLM_PRED_LOGLIK)):
        assert re.search(rf"#define AHMC_GLM_PRED_{macro} (\d+)", src).group(1) == str(v)
    assert sorted(capi.GLM_PRED_WHAT.values()) == [0, 1, 2, 3] and tuple(capi.GLM_PRED_WHAT) == G.PRED_WHAT
    # the record: the header's fields in its order, as the binding has them
    body = re.search(r"typedef struct ahmc_glm_newdata \{(.*?)\} ahmc_glm_newdata;", src, flags=re.S).group(1)
    fields = [f.strip().rsplit(" ", 1) for f in body.split(";") if f.strip()]
    assert [(n.lstrip("*"), ty.replace("const ", "") + ("*" if n.startswith("*") else "")) for ty, n in fields] == \
        [("n_new", "int64_t"), ("X", "void*"), ("levels", "int32_t*"), ("offset", "void*"), ("y", "void*")]
    assert [(n, t) for n, t in capi.GLMNewDataRecord._fields_] == [("n_new", C.c_int64), ("X", C.c_void_p), ("levels", C.POINTER(C.c_int32)), ("offset", C.c_void_p),
                                                                   ("y", C.c_void_p)]
    assert '#include "ahmc_glm.h"' in src
    from ahmc_amd import build as B
    assert "ahmc_glm_predict.h" in open(B.__file__, encoding="utf-8").read()
    spec = open(os.path.join(CSRC, "ahmc_glm_predict_spec.hpp"), encoding="utf-8").read()
    assert re.search(r"constexpr int64_t GLM_PRED_BLOCK = (\d+);", spec).group(1) == str(G.PRED_BLOCK) == "64"
    assert "hip" not in re.sub(r"//[^\n]*", "", spec).lower().replace("ahmc_hip", "")      # the host compiler alone builds it
    # the older headers keep their versions
    for hdr, macro, v in (("ahmc_hip.h", "AHMC_ABI_VERSION", capi.AHMC_ABI_VERSION), ("ahmc_diag.h", "AHMC_DIAG_VERSION", capi.AHMC_DIAG_VERSION),
                          ("ahmc_glm.h", "AHMC_GLM_VERSION", capi.AHMC_GLM_VERSION), ("ahmc_glm_hier.h", "AHMC_HGLM_VERSION", capi.AHMC_HGLM_VERSION),
                          ("ahmc_glm_aux.h", "AHMC_GLM_AUX_VERSION", capi.AHMC_GLM_AUX_VERSION),
                          ("ahmc_glm_factor.h", "AHMC_GLM_FACTOR_VERSION", capi.AHMC_GLM_FACTOR_VERSION),
                          ("ahmc_glm_ordinal.h", "AHMC_GLM_ORDINAL_VERSION", capi.AHMC_GLM_ORDINAL_VERSION),
                          ("ahmc_glm_categorical.h", "AHMC_GLM_CATEGORICAL_VERSION", capi.AHMC_GLM_CATEGORICAL_VERSION),
                          ("ahmc_glm_loo.h", "AHMC_GLM_LOO_VERSION", capi.AHMC_GLM_LOO_VERSION)):
        assert re.search(rf"#define {macro} (\d+)", open(os.path.join(INCLUDE, hdr), encoding="utf-8").read()).group(1) == str(v), hdr


def test_julia_ccalls_match_the_header():
    protos, _ = header_prototypes()
    src = open(os.path.join(ROOT, "julia", "AdvancedHMCMI355XGLMPredict.jl"), encoding="utf-8").read()
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
                if p.startswith("double"):
                    assert t == "Ptr{Cdouble}", (name, t, p)
                if "ahmc_glm_newdata" in p:
                    assert t == "Ref{GLMNewDataRecord}", (name, t, p)
            else:
                assert {"int64_t": "Int64", "int32_t": "Cint", "double": "Cdouble"}[p.split()[0]] == t, (name, t, p)
    assert seen == set(protos)
    rec = re.search(r"struct GLMNewDataRecord\n(.*?)\nend", src, flags=re.S).group(1)
    assert [l.strip() for l in rec.splitlines()] == ["n_new::Int64", "X::Ptr{Cvoid}", "levels::Ptr{Cint}", "offset::Ptr{Cvoid}", "y::Ptr{Cvoid}"]
    ext = open(os.path.join(ROOT, "julia", "AdvancedHMCMI355XExt.jl"), encoding="utf-8").read()
    assert 'include("AdvancedHMCMI355XGLMPredict.jl")' in ext and "ahmc_glm_predict" not in ext.replace("ahmc_glm_predict.h", "")
    assert ext.index('include("AdvancedHMCMI355XGLMLoo.jl")') < ext.index('include("AdvancedHMCMI355XGLMPredict.jl")')


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="needs llvm-objdump")
def test_library_exports_and_kernels_without_scratch():
    """every entry point is in the dynamic symbol table; k_glm_pred of both element types, the seven families, with and without factors,
    with and without the summary's epilogue — 28 an element type, held to the count of k_glm_eta, k_glm_eta_f and k_glm_eta_cat together (the reading of
    "no more instantiations than k_glm_eta" taken here: the kernels that make η for the same families with and without factors) — and
    the fold are in the code object with no private segment, no vector-register spill, within a wave's registers, and 40 KiB of LDS"""
    from ahmc_amd import build as B

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_meta
    finally:
        sys.path.pop(0)
    assert os.path.exists(B.OUT), "build() first"
    exported = {l.split()[-1] for l in subprocess.run(["nm", "-D", "--defined-only", B.OUT], capture_output=True, text=True, check=True).stdout.splitlines() if l.strip()}
    assert set(capi.GLM_PREDICT_SIGNATURES) <= exported, set(capi.GLM_PREDICT_SIGNATURES) - exported
    meta = kernel_meta.kernel_meta(B.OUT)
    names = subprocess.run(["c++filt"], input="\n".join(k["name"] for k in meta), capture_output=True, text=True, check=True).stdout.splitlines()
    want = {f"k_glm_pred<{T}, {fam}, {fac}, {sm}>" for T in ("float", "double") for fam in range(7) for fac in ("true", "false") for sm in ("true", "false")}
    want |= {"k_glm_pred_fold", "k_glm_pred_no_lpd"}
    found, eta = {}, 0
    for k, dn in zip(meta, names):
        head = dn.split("(")[0].replace("void ", "")
        if head.startswith("ahmc::k_glm_pred"):
            found[head[len("ahmc::"):]] = k
        eta += head.startswith(("ahmc::k_glm_eta<", "ahmc::k_glm_eta_f<", "ahmc::k_glm_eta_cat<"))
    assert set(found) == want, (sorted(want - set(found)), sorted(set(found) - want))
    assert len([w for w in found if w.startswith("k_glm_pred<")]) <= eta, eta
    for w, k in found.items():
        assert k["private_segment_fixed_size"] == 0, (w, k)
        assert k.get("vgpr_spill_count", 0) == 0, (w, k)
        assert k["vgpr_count"] + k.get("agpr_count", 0) <= 512, (w, k)
        assert k["group_segment_fixed_size"] <= 40 * 1024, (w, k)


def test_engine_needs_the_header():
    """a library without the header's symbols answers UnsupportedError, not a fallback"""
    class Lib:
        has_glm_predict = False
        path = "libother.so"

    e = A.Engine.__new__(A.Engine)
    e.lib = Lib()
    nd = A.GLMNewData(np.zeros((2, 2)))
    for call in (e.glm_predict, e.glm_predict_summary):
        with pytest.raises(A.UnsupportedError, match="ahmc_glm_predict.h"):
            call(nd)


def test_newdata_and_summary_dict():
    nd = A.GLMNewData(np.zeros((4, 2)), factors=[np.arange(4)], offset=np.zeros(4), y=np.ones(4))
    assert nd.n_new == 4 and "n_new=4" in repr(nd)
    for kw in (dict(X=np.zeros(4)), dict(X=np.zeros((4, 2)), factors=[np.zeros(3, dtype=int)]), dict(X=np.zeros((4, 2)), factors=[np.zeros(4)]),
               dict(X=np.zeros((4, 2)), offset=np.zeros(5)), dict(X=np.zeros((4, 2)), y=np.zeros(3))):
        with pytest.raises(A.ArgumentError, match="DimensionMismatch"):
            A.GLMNewData(**kw)
    s = np.arange(7 * 2, dtype=float).reshape(7, 2)
    d = A.api.glm_summary_dict(s)
    assert sorted(d) == ["eta_mean", "eta_var", "lpd", "mean", "mean_var", "var_within"] and np.array_equal(d["var_within"], s[4]) and np.array_equal(d["lpd"], s[6])
    d = A.api.glm_summary_dict(np.arange(11 * 2, dtype=float).reshape(11, 2), 2, 3)
    assert d["eta_mean"].shape == (2, 2) and d["probs"].shape == (3, 2) and np.array_equal(d["probs_var"][0], [10, 11]) and np.array_equal(d["lpd"], [20, 21])
    with pytest.raises(A.ArgumentError, match="DimensionMismatch"):
        A.api.glm_summary_dict(s, 2, 3)


# ---------------------------------------------------------------------------------------------------------------------
# the guard-band cases of the new entry points: registered in the table of tests/test_buffer_bounds.py, whose gate counts them
# ---------------------------------------------------------------------------------------------------------------------
def c_predict(r, n_new, S, where):
    """newdata (the record itself, host memory), theta and out of ahmc_glm_predict for every `what`, and newdata, theta and summary_out of
    ahmc_glm_predict_summary, each sized exactly, from device and host draws, on the model with groups, factors and a dispersion
    (D = 10, N = 5); the arrays the record points to are the caller's own and are not probed here"""
    D, n_obs = 10, 70
    dll = r.lib.dll
    pd = C.POINTER(C.c_double)
    rs = np.random.default_rng([n_new, S])
    for dtype in (TB.F64, TB.F32):
        mk = lambda: TB.bound_glm(r, n_obs, dtype)  # noqa: E731
        X = np.asfortranarray(rs.normal(size=(n_new, 3)), dtype=dtype)
        lev = np.asfortranarray(np.column_stack([rs.integers(0, 2, n_new), rs.integers(0, 3, n_new)]), dtype=np.int32)
        y = rs.normal(size=n_new).astype(dtype)
        rec = capi.GLMNewDataRecord(n_new, X.ctypes.data, lev.ctypes.data_as(C.POINTER(C.c_int32)), None, y.ctypes.data)
        rec_bytes = np.frombuffer(bytes(rec), dtype=np.uint8).copy()
        th = (0.4 * rs.normal(size=D * S)).astype(dtype)
        for w_in in ("device", "host"):
            for what in range(4):
                r.probe(mk, lambda e, io: r.ok(e, dll.ahmc_glm_predict(e._ctx, io["ahmc_glm_predict.newdata"], io["ahmc_glm_predict.theta"], S, what,
                                                                       io["ahmc_glm_predict.out"])),
                        ins={"ahmc_glm_predict.newdata": In(rec_bytes, "host"), "ahmc_glm_predict.theta": In(th, w_in)},
                        outs={"ahmc_glm_predict.out": Out(dtype, n_new * S, where)})
            r.probe(mk, lambda e, io: r.ok(e, dll.ahmc_glm_predict_summary(e._ctx, io["ahmc_glm_predict_summary.newdata"], io["ahmc_glm_predict_summary.theta"], S,
                                                                           C.cast(io["ahmc_glm_predict_summary.summary_out"], pd))),
                    ins={"ahmc_glm_predict_summary.newdata": In(rec_bytes, "host"), "ahmc_glm_predict_summary.theta": In(th, w_in)},
                    outs={"ahmc_glm_predict_summary.summary_out": Out(np.float64, 7 * n_new if S else 0, where)})
        del X, lev, y


_PROBES = ["ahmc_glm_predict.newdata", "ahmc_glm_predict.theta", "ahmc_glm_predict.out", "ahmc_glm_predict_summary.newdata", "ahmc_glm_predict_summary.theta",
           "ahmc_glm_predict_summary.summary_out"]
BOUNDS_CASES = []
for _n, _s in ((65, 65), (1, 3)):
    for _w in ("device", "host"):
        _cid = f"glm-predict-nnew{_n}-S{_s}-{_w}"
        if _cid not in TB.CASES:
            TB.add(_cid, c_predict, _PROBES, oracle=False, n_new=_n, S=_s, where=_w)
        BOUNDS_CASES.append(_cid)


def test_bounds_cases_cover_the_header():
    params = {p for p in TB.header_pointer_params() if p[0] in capi.GLM_PREDICT_SIGNATURES and p[1] != "ctx"}
    probed = {tuple(k.split(".")) for cid in BOUNDS_CASES for k in TB.CASES[cid].probes}
    assert params == probed and len(params) == 6


@pytest.mark.gpu
@pytest.mark.parametrize("cid", BOUNDS_CASES)
def test_hip_bounds(hip, monkeypatch, cid):
    """§10: neither call reads or writes outside the caller's arrays (tests/arena_util.py), at n_new = 65 and S = 65 among others"""
    TB.run_case(hip, monkeypatch, cid)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def engine(hip, t, N, dtype, th=None, seed=7):
    return TL.engine(hip, t, N, dtype, th, seed)


def device_values(e, t, nd, draws, n_cols=None):
    K, Cc, Q = counts(t)
    return stacked([e.glm_predict(nd, draws, n_cols, what=w) for w in (("linear", "mean") if Cc else ("linear", "mean", "variance"))])


def raw_summary(e, t, nd, draws):
    """the whole (2Q + 1, n_new) array of ahmc_glm_predict_summary (Engine.glm_predict_summary names its rows but for the variance over the
    draws of Var[y | θ]), and the dict"""
    K, Cc, Q = counts(t)
    rec, keep = e._glm_newdata("glm_predict_summary", nd)
    ptr, n = e._draws("glm_predict_summary", draws, None)
    s = np.full((2 * Q + 1, nd.n_new), np.nan, order="F")
    e._call("ahmc_glm_predict_summary", C.byref(rec), ptr, n, s.ctypes.data_as(C.POINTER(C.c_double)))
    d = e.glm_predict_summary(nd, draws)
    want = A.api.glm_summary_dict(s, K, Cc)
    assert sorted(d) == sorted(want)
    for k in d:
        bits(f"dict-is-the-array {k}", d[k], want[k])
    return s


class chunk_of:
    """AHMC_GLM_PREDICT_CHUNK for the calls inside"""

    def __init__(self, mp, cols):
        self.mp, self.cols = mp, cols

    def __enter__(self):
        if self.cols is None:
            self.mp.delenv("AHMC_GLM_PREDICT_CHUNK", raising=False)
        else:
            self.mp.setenv("AHMC_GLM_PREDICT_CHUNK", str(self.cols))

    def __exit__(self, *a):
        self.mp.delenv("AHMC_GLM_PREDICT_CHUNK", raising=False)


# ---- §4 ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", TG.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", FAMILIES)
def test_identity_with_the_existing_entry_points(hip, name, dtype):
    """new data = the training data: LINEAR at the current θ has the bits of ahmc_glm_pointwise's η, LOGLIK at 2N + 3 host draws those of
    ahmc_glm_loglik, a categorical model's MEAN those of ahmc_glm_class_probs"""
    t, centre = model(name)
    th = TL.draws_of(t, centre, N_CHAINS, dtype)
    e = engine(hip, t, N_CHAINS, dtype, th)
    nd = training_rows(t)
    key = f"{name} {np.dtype(dtype).name}"
    eta, ll = e.glm_pointwise()
    bits(f"identity linear {key}", e.glm_predict(nd, what="linear"), eta)
    bits(f"identity loglik-current {key}", e.glm_predict(nd, what="loglik"), ll)
    draws = TL.draws_of(t, centre, 2 * N_CHAINS + 3, dtype)
    got = e.glm_predict(nd, draws, what="loglik")
    assert got.shape == (70, 2 * N_CHAINS + 3) and got.dtype == np.dtype(dtype) and np.isfinite(got).all()
    bits(f"identity loglik {key}", got, e.glm_loglik(draws))
    if t.n_classes:
        bits(f"identity class-probs {key}", e.glm_predict(nd, draws, what="mean"), e.glm_class_probs(draws))
    e.close()


# ---- §5 ----
def eta_model(t, nd, draws, dtype):
    """(η̂ (K, n_new, n) in the element type: the k-ordered fma chain over X's columns, then the factors' rows in order, then the offset —
    each one addition in the element type; the exact η in long double; E_η): W from the mirror's coefficients, rounded to the element type
    as the device holds them (a member of a non-centred group: exp and one product on the device, so W is taken from the device's own
    ahmc_hglm_coefficients where the model has groups — here the models with groups are excluded)"""
    dt = np.dtype(dtype)
    assert not t.groups
    K, Cc, Q = counts(t)
    W = np.asfortranarray(draws[:t.P], dtype=dt)
    X = np.asfortranarray(nd.X, dtype=dt)
    u = TG.U[dt]
    hats, exacts, des = [], [], []
    for k in range(K):
        Wk = W[k * t.P_b:(k + 1) * t.P_b]
        hat = TG.chain(X, np.asfortranarray(Wk[:t.P_x]))
        E, S = TG.exact(X, np.asfortranarray(Wk[:t.P_x]))
        adds = 0
        for (lo, _), idx in zip(t.factor_ranges, nd.factors):
            hat = hat + Wk[lo + idx]
            E, S = E + Wk[lo + idx].astype(LD), S + np.abs(Wk[lo + idx]).astype(LD)
            adds += 1
        if nd.offset is not None:
            off = np.asarray(nd.offset[:, k] if nd.offset.ndim == 2 else nd.offset, dtype=dt).reshape(-1, 1)
            hat = hat + off
            E, S = E + off.astype(LD), S + np.abs(off).astype(LD)
            adds += 1
        assert hat.dtype == dt
        hats.append(hat)
        exacts.append(E)
        des.append((TG.gam(t.P_x + adds, u) + TG.gam(t.P_x + adds + 1, TG.U_LD)) * S + (u + TG.U_LD) * np.abs(hat.astype(LD)))
    return np.stack(hats), np.stack(exacts), np.stack(des)


def quantity_ld(t, eta, draws, dtype):
    """the quantities after η in long double at the exact η (K, n_new, n), from the draws as the device holds them"""
    th = np.asarray(draws, dtype=dtype).astype(LD)
    if t.n_classes:
        e = np.concatenate([np.zeros_like(eta[:1]), eta])
        p = np.exp(e - e.max(axis=0))
        return p / p.sum(axis=0)
    eta = eta[0]
    if t.n_categories:
        kap = th[t.P:]
        c = np.concatenate([kap[:1], kap[:1] + np.cumsum(np.exp(kap[1:]), axis=0)])
        cdf = np.concatenate([np.zeros((1,) + eta.shape, dtype=LD), 1 / (1 + np.exp(-(c[:, None, :] - eta[None]))), np.ones((1,) + eta.shape, dtype=LD)])
        return np.diff(cdf, axis=0)
    s = th[-1] if t.aux else None
    if t.family == G.BERNOULLI_LOGIT:
        mu = 1 / (1 + np.exp(-eta))
        return np.stack([mu, mu * (1 - mu)])
    if t.family == G.POISSON_LOG:
        return np.stack([np.exp(eta)] * 2)
    if t.family == G.GAUSSIAN_IDENTITY:
        return np.stack([eta, np.full_like(eta, 1 / LD(float(np.dtype(dtype).type(t.scale))))])
    if t.family == G.GAUSSIAN_IDENTITY_SIGMA:
        return np.stack([eta, np.broadcast_to(np.exp(2 * s), eta.shape)])
    mu = np.exp(eta)
    return np.stack([mu, mu + mu * mu * np.exp(-s)])


def quantity_bounds(t, q, de, draws, dtype, eps):
    """the bound on each quantity of `quantity_ld` (same shape), from E_η = de (K, n_new, n), ε_exp, ε_log1p (doubled measurements) and u:
      Bernoulli   μ = σ(η): L = 1/4; one exp, one addition, one division: E_μ = E_η/4 + μ(2 ε_exp + 2u);  v = μ(1 − μ): |1 − 2μ| <= 1, so
                  E_v = E_μ + E_μ² + 2u·v
      Poisson     μ = exp(η): E = exp(η + E_η)·E_η + ε_exp·μ + u·μ;  v = μ
      Gaussian    μ = η: E_η;  v = 1/scale: one division, u·v;  with σ sampled v = exp(2s): 2s is exact, ε_exp·v
      neg. bin.   μ as Poisson;  v = fma(μ², e^{−s}, μ): (2μ e^{−s} + 1)·E_μ + e^{−s}·E_μ² + μ² e^{−s}(ε_exp + 2u) + u·v
      categorical p_c: |∂p_c/∂η_k| <= 1/4 for every k: Σ_k E_η_k / 4; K + 1 exps of arguments with one rounding each (|η − m| u <= 2·ETA u), the sum of
                  K + 1 terms, one division, one product: p·((K + 3)(ε_exp + 2u) + 2·ETA·u·2)
      ordinal     p_k = exp(ℓ_k), ℓ_k = −softplus(−a) − softplus(b) + lg with a = c_{k+1} − η, b = c_k − η.  c_j = κ_1 + Σ_{i<=j} exp(κ_i): E_c =
                  (ε_exp + (C + 1) u)·(|κ_1| + Σ exp κ_i); E_a = E_η + E_c + u|a|.  A softplus: σ(·) <= 1 times its argument's error, and
                  log1p(e)·(ε_exp + ε_log1p) + u·softplus; lg = log(1 − e^{−δ}) with δ = exp(κ) off by ε_exp·δ: dlg/dδ = 1/(e^δ − 1) = r, so
                  r·δ·ε_exp, and its own two function evaluations 2(ε_exp + ε_log1p)(|lg| + 1); two additions: 2u|ℓ|.  E_p = p·(E_ℓ + ε_exp) (and
                  the second-order term p·E_ℓ²)."""
    u = TG.U[np.dtype(dtype)]
    ee, el = LD(eps["exp"]), LD(eps["log1p"])
    th = np.asarray(draws, dtype=dtype).astype(LD)
    tiny = 8 * TG.U_LD * (np.abs(q) + 1)
    if t.n_classes:
        K = de.shape[0]
        return TG.SLACK * (de.sum(axis=0)[None] / 4 + q * ((K + 3) * (ee + 2 * u) + 4 * LD(TG.ETA_MAX) * u)) + tiny
    d = de[0]
    if t.n_categories:
        kap = th[t.P:]
        Cn = t.n_categories
        parts = np.abs(kap[0]) + np.exp(kap[1:]).sum(axis=0)
        Ec = (ee + (Cn + 1) * u) * parts
        delta = np.exp(kap)
        with np.errstate(divide="ignore", over="ignore"):
            r = np.where(np.arange(Cn - 1)[:, None] > 0, 1 / np.expm1(delta), 0)
            lg = np.where(np.arange(Cn - 1)[:, None] > 0, np.log(-np.expm1(-delta)), 0)
        lgE = np.concatenate([np.zeros((1,) + Ec.shape, dtype=LD), (r * delta * ee + 2 * (ee + el) * (np.abs(lg) + 1))[1:], np.zeros((1,) + Ec.shape, dtype=LD)])
        Ea = d + Ec[None] + u * (np.abs(kap).max() + parts[None] + LD(TG.ETA_MAX))
        l1p = LD(np.log(2.0))
        El = 2 * (Ea + l1p * (ee + el)) + lgE[:, None, :] + 4 * u * np.abs(np.log(np.maximum(q, LD("1e-4000"))))
        return TG.SLACK * q * (El + El * El + ee + u) + tiny
    ex = np.exp(th[-1]) if t.aux else None
    if t.family == G.BERNOULLI_LOGIT:
        Em = d / 4 + q[0] * (2 * ee + 2 * u)
        return TG.SLACK * np.stack([Em, Em + Em * Em + 2 * u * q[1]]) + tiny
    if t.family in (G.POISSON_LOG, G.NEGBINOMIAL_LOG):
        eta = np.log(q[0])
        Em = np.exp(eta + d) * d + (ee + u) * q[0]
        if t.family == G.POISSON_LOG:
            return TG.SLACK * np.stack([Em, Em]) + tiny
        return TG.SLACK * np.stack([Em, (2 * q[0] / ex + 1) * Em + Em * Em / ex + q[0] ** 2 / ex * (ee + 2 * u) + u * q[1]]) + tiny
    if t.family == G.GAUSSIAN_IDENTITY:
        return TG.SLACK * np.stack([d, u * q[1]]) + tiny
    return TG.SLACK * np.stack([d, ee * q[1]]) + tiny


def emulate_quantities(t, eta_hat, draws, dtype, sign=1.0):
    """the device's arithmetic after η̂ on the host in the element type (numpy's functions for the device's); `sign` = −1 plants a defect:
    σ(−η), exp(−η), the softmax of −η, the category probabilities of −η"""
    dt = np.dtype(dtype).type
    th = np.asarray(draws, dtype=dtype)
    eh = (dt(sign) * eta_hat).astype(dtype)
    with np.errstate(over="ignore"):
        if t.n_classes:
            return G.categorical_link(np.zeros(eh.shape[1], dtype=np.int64), eh)[2]
        eh = eh[0]
        if t.n_categories:
            c, lg, r, _ = G.cut_constants(th[t.P:])
            return np.stack([np.exp(G.ordinal_link(np.full(eh.shape[0], k), eh, c, lg, r)[0]) for k in range(t.n_categories)])
        if t.family == G.BERNOULLI_LOGIT:
            e = np.exp(-np.abs(eh))
            d = dt(1) + e
            mu = np.where(eh >= 0, dt(1) / d, e / d)
            return np.stack([mu, mu * (dt(1) - mu)])
        if t.family == G.POISSON_LOG:
            return np.stack([np.exp(eh)] * 2)
        if t.family == G.GAUSSIAN_IDENTITY:
            return np.stack([eh, np.full_like(eh, dt(1) / dt(t.scale))])
        if t.family == G.GAUSSIAN_IDENTITY_SIGMA:
            return np.stack([eh, np.broadcast_to(np.exp(dt(2) * th[-1]), eh.shape)])
        mu = np.exp(eh)
        return np.stack([mu, TG.host_fma(mu * mu, np.broadcast_to(np.exp(-th[-1]), eh.shape), mu)])


NEW_ROW_MODELS = ("bernoulli-plain", "poisson", "gaussian", "gaussian-sigma", "negbinomial", "ordered", "categorical")


def host_eps(dtype):
    return TG.function_eps(np.exp, np.log1p, dtype)


@pytest.mark.parametrize("dtype", TG.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", NEW_ROW_MODELS)
def test_new_row_bounds_hold_for_a_host_emulation_and_catch_a_wrong_sign(name, dtype):
    """CPU: `quantity_bounds` hold for the element type's arithmetic done with numpy's functions, and a sign error in η breaks them"""
    t, centre = model(name)
    nd = new_rows(t, 65)
    draws = TL.draws_of(t, centre, 9, dtype)
    eta_hat, eta, de = eta_model(t, nd, draws, dtype)
    q = quantity_ld(t, eta, draws, dtype)
    B = quantity_bounds(t, q, de, draws, dtype, host_eps(dtype))
    good = emulate_quantities(t, eta_hat, draws, dtype)
    assert good.dtype == np.dtype(dtype) and good.shape == q.shape
    assert np.all(np.abs(good.astype(LD) - q) <= B), (name, float(np.max(np.abs(good.astype(LD) - q) / B)))
    bad = emulate_quantities(t, eta_hat, draws, dtype, sign=-1.0)
    moved = [0] if t.family in (G.GAUSSIAN_IDENTITY, G.GAUSSIAN_IDENTITY_SIGMA) and not (t.n_classes or t.n_categories) else slice(None)
    assert np.any(np.abs(bad.astype(LD) - q)[moved] > B[moved]), name


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", TG.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", NEW_ROW_MODELS)
def test_new_rows_against_the_chain_model_and_derived_bounds(hip, probe, name, dtype):  # noqa: F811
    """new rows (n_new = 130: two row blocks and a partial one), 70 draws (a column block and a partial one): η has the bits of the fma-chain
    model; μ, v and the probabilities lie inside `quantity_bounds` with the device's measured ε_exp, ε_log1p"""
    t, centre = model(name)
    nd = new_rows(t, 130)
    draws = TL.draws_of(t, centre, 70, dtype)
    e = engine(hip, t, N_CHAINS, dtype)
    key = f"{name} {np.dtype(dtype).name}"
    eta_hat, eta, de = eta_model(t, nd, draws, dtype)
    lin = e.glm_predict(nd, draws, what="linear")
    bits(f"new-rows eta {key}", lin if t.n_classes else lin[None], eta_hat)
    q = quantity_ld(t, eta, draws, dtype)
    B = quantity_bounds(t, q, de, draws, dtype, TG.device_eps(probe, dtype))
    got = e.glm_predict(nd, draws, what="mean")
    got = got if (t.n_classes or t.n_categories) else np.stack([got, e.glm_predict(nd, draws, what="variance")])
    assert got.dtype == np.dtype(dtype)
    TG.record_bound(f"predict new-rows quantities {key}", np.abs(got.astype(LD) - q), B)
    if t.n_classes or t.n_categories:
        assert np.abs(got.astype(np.float64).sum(axis=0) - 1).max() <= 8 * float(TG.U[np.dtype(dtype)]) * (t.n_classes or t.n_categories)
    e.close()


# ---- §6 ----
SUMMARY_CASES = [(name, 65, S, np.float64) for name in TL.FAMILIES for S in (200,)] + \
                [("bernoulli", n, S, np.float64) for n in N_NEW for S in S_ALL] + \
                [("negbinomial", 65, 4100, np.float32), ("categorical", 130, 4100, np.float32), ("poisson", 64, 65, np.float32)]
SUMMARY_CASES = list(dict.fromkeys(SUMMARY_CASES))


@pytest.mark.gpu
@pytest.mark.parametrize("name,n_new,S,dtype", SUMMARY_CASES, ids=[f"{c[0]}-n{c[1]}-S{c[2]}-{np.dtype(c[3]).name}" for c in SUMMARY_CASES])
def test_summary_equals_the_mirror_on_the_devices_own_values(hip, monkeypatch, name, n_new, S, dtype):
    """ahmc_glm_predict_summary against glm.predict_summary applied to ahmc_glm_predict's full output: means and variances bit for bit, lpd
    within 8 × max(the float64 mirror's deviation from long double in this case, 8 u); S = 4100 runs in chunks of 1024 draws (five)"""
    t, centre = model(name)
    nd = new_rows(t, n_new)
    draws = TL.draws_of(t, centre, S, dtype, spread=0.3)
    e = engine(hip, t, N_CHAINS, dtype)
    vals = device_values(e, t, nd, draws)
    ll = e.glm_predict(nd, draws, what="loglik")
    with chunk_of(monkeypatch, 1024 if S > 1024 else None):
        got = raw_summary(e, t, nd, draws)
    mir = G.predict_summary(vals, ll)
    key = f"device-summary {name} n_new={n_new} S={S} {np.dtype(dtype).name}"
    ref = summary_ld(vals, ll)
    Q = vals.shape[0]
    mir_u = float(np.max(np.abs(mir[2 * Q].astype(LD) - ref[2 * Q]) / np.maximum(np.abs(ref[2 * Q]), 1)) / LD(U53))
    bits(f"summary-moments {key}", got[:2 * Q], mir[:2 * Q])
    dev_u = float(np.max(np.abs(got[2 * Q].astype(LD) - ref[2 * Q]) / np.maximum(np.abs(ref[2 * Q]), 1)) / LD(U53))
    MARGINS[key] = {"lpd_mirror_u": mir_u, "lpd_device_u": dev_u, "lpd_bar_u": 8 * max(mir_u, 8.0)}
    dump_margins()
    print(key, MARGINS[key])
    assert np.isfinite(got[2 * Q]).all() and dev_u <= 8 * max(mir_u, 8.0), MARGINS[key]
    assert np.isnan(got[1:2 * Q:2]).all() if S == 1 else np.isfinite(got[:2 * Q]).all()
    # without outcomes: the same moments, no lpd
    no_y = raw_summary(e, t, A.GLMNewData(nd.X, nd.factors, nd.offset), draws)
    bits(f"summary-without-y {key}", no_y[:2 * Q], got[:2 * Q])
    assert np.isnan(no_y[2 * Q]).all()
    e.close()


# ---- §7 ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", TG.DTYPES, ids=["f64", "f32"])
def test_invariances_bit_for_bit(hip, monkeypatch, dtype):
    """the same new rows and draws: contexts with N = 37 and N = 48; forced chunks of 64 and 192 draws; host arrays against device pointers
    for θ, X and the outputs; rows permuted ⇒ outputs permuted; the first 65 of 130 rows give the first 65 outputs"""
    import torch

    t, centre = model("poisson")
    dn = np.dtype(dtype).name
    S, n_new = 200, 130
    nd = new_rows(t, n_new)
    draws = TL.draws_of(t, centre, S, dtype)
    a = engine(hip, t, 37, dtype)
    full = {w: a.glm_predict(nd, draws, what=w) for w in G.PRED_WHAT}
    summ = a.glm_predict_summary(nd, draws)
    names = sorted(summ)
    for cols in (64, 192):
        with chunk_of(monkeypatch, cols):
            for w in G.PRED_WHAT:
                bits(f"inv-chunk{cols} {w} {dn}", a.glm_predict(nd, draws, what=w), full[w])
            sc = a.glm_predict_summary(nd, draws)
        for k in names:
            bits(f"inv-chunk{cols} summary {k} {dn}", sc[k], summ[k])
    # device pointers: θ, X (with offset and y) and the outputs
    d_dev = torch.from_numpy(np.ascontiguousarray(draws.T)).cuda()
    for w in G.PRED_WHAT:
        bits(f"inv-theta-pointer {w} {dn}", a.glm_predict(nd, d_dev.data_ptr(), n_cols=S, what=w), full[w])
    sp = a.glm_predict_summary(nd, d_dev.data_ptr(), n_cols=S)
    for k in names:
        bits(f"inv-theta-pointer summary {k} {dn}", sp[k], summ[k])
    X_dev, off_dev, y_dev = (TG.dev(np.asarray(v, dtype=dtype)) for v in (nd.X, nd.offset, nd.y))
    lev = np.asfortranarray(np.column_stack(nd.factors), dtype=np.int32)
    rec = capi.GLMNewDataRecord(n_new, X_dev.data_ptr(), lev.ctypes.data_as(C.POINTER(C.c_int32)), off_dev.data_ptr(), y_dev.data_ptr())
    out_dev = torch.empty(n_new * S, dtype=torch.float64 if np.dtype(dtype) == np.float64 else torch.float32, device="cuda")
    for w in G.PRED_WHAT:
        a._call("ahmc_glm_predict", C.byref(rec), C.c_void_p(d_dev.data_ptr()), S, capi.GLM_PRED_WHAT[w], C.c_void_p(out_dev.data_ptr()))
        bits(f"inv-device-data {w} {dn}", TG.host(out_dev, (n_new, S)), full[w])
    sum_dev = torch.empty(7 * n_new, dtype=torch.float64, device="cuda")
    a._call("ahmc_glm_predict_summary", C.byref(rec), C.c_void_p(d_dev.data_ptr()), S, C.cast(C.c_void_p(sum_dev.data_ptr()), C.POINTER(C.c_double)))
    sd = A.api.glm_summary_dict(TG.host(sum_dev, (7, n_new)))
    for k in names:
        bits(f"inv-device-data summary {k} {dn}", sd[k], summ[k])
    # the first 65 rows; rows permuted
    first = A.GLMNewData(nd.X[:65], [f[:65] for f in nd.factors], nd.offset[:65], nd.y[:65])
    perm = np.random.default_rng(3).permutation(n_new)
    permuted = A.GLMNewData(nd.X[perm], [f[perm] for f in nd.factors], nd.offset[perm], nd.y[perm])
    for w in G.PRED_WHAT:
        bits(f"inv-first65 {w} {dn}", a.glm_predict(first, draws, what=w), full[w][:65])
        bits(f"inv-rows {w} {dn}", a.glm_predict(permuted, draws, what=w), full[w][perm])
    s65, sq = a.glm_predict_summary(first, draws), a.glm_predict_summary(permuted, draws)
    for k in names:
        bits(f"inv-first65 summary {k} {dn}", s65[k], summ[k][:65])
        bits(f"inv-rows summary {k} {dn}", sq[k], summ[k][perm])
    a.close()
    # N = 48
    b = engine(hip, t, 48, dtype)
    for w in G.PRED_WHAT:
        bits(f"inv-N {w} {dn}", b.glm_predict(nd, draws, what=w), full[w])
    sb = b.glm_predict_summary(nd, draws)
    b.close()
    for k in names:
        bits(f"inv-N summary {k} {dn}", sb[k], summ[k])


# ---- §8 ----
@pytest.mark.gpu
@pytest.mark.parametrize("name", ("bernoulli", "categorical"))
def test_no_side_effects(hip, name):
    """a NUTS transition after both calls has the bits of a twin context that made neither: θ, r, the statistics and the RNG's position (a
    second transition); ahmc_glm_pointwise of the bound model is unchanged"""
    t, centre = model(name)
    N = N_CHAINS
    th0 = TL.draws_of(t, centre, N, np.float64)
    kern = TG.nuts_kernel(N, eps=0.1, depth=5)
    e, twin = (engine(hip, t, N, np.float64, th0, seed=21) for _ in range(2))
    for c in (e, twin):
        c.transition(kern)
    before = e.glm_pointwise()
    nd = new_rows(t, 65)
    draws = TL.draws_of(t, centre, 130, np.float64)
    for w in ("linear", "mean", "loglik"):
        e.glm_predict(nd, draws, what=w)
    e.glm_predict_summary(nd, draws)
    after = e.glm_pointwise()
    for k, (x, y) in enumerate(zip(before, after)):
        bits(f"side-effects pointwise {k} {name}", y, x)
    for step in range(2):
        e.transition(kern)
        twin.transition(kern)
        bits(f"side-effects theta {step} {name}", e.theta(), twin.theta())
        pe, pt = e.phasepoint(), twin.phasepoint()
        bits(f"side-effects r {step} {name}", pe.r, pt.r)
        se, st = e.stats(), twin.stats()
        for k in se:
            np.testing.assert_array_equal(se[k], st[k], err_msg=k)
    e.close()
    twin.close()


# ---- §9 ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", TG.DTYPES, ids=["f64", "f32"])
def test_non_finite_draws(hip, dtype):
    """a Poisson draw whose exp overflows: NaN in that observation's μ rows (mean, its variance, var_within) and lpd, finite numbers in its
    η rows and for its neighbours"""
    t, centre = model("poisson-plain", 70, 2)
    nd = new_rows(t, 65)
    X = nd.X.copy()
    X[9] = (1000.0, 0.0)
    nd = A.GLMNewData(X, y=nd.y)
    centre = centre.copy()
    centre[0] = 0.5
    draws = TL.draws_of(t, centre, 130, dtype, spread=0.1)
    draws[0, 77] = 1.0                                   # η_9 = 1000 at this draw: exp overflows in either element type
    e = engine(hip, t, N_CHAINS, dtype)
    mu = e.glm_predict(nd, draws, what="mean")
    assert np.isinf(mu[9, 77]) and np.isfinite(np.delete(mu, 9, axis=0)).all()
    s = e.glm_predict_summary(nd, draws)
    e.close()
    for k in ("mean", "mean_var", "var_within", "lpd"):
        assert np.isnan(s[k][9]) and np.isfinite(np.delete(s[k], 9)).all(), k
    assert np.isfinite(s["eta_mean"]).all() and np.isfinite(s["eta_var"]).all()
    mir = A.api.glm_summary_dict(G.predict_summary(stacked([e_ for e_ in (t.predict(draws, nd, w) for w in ("linear", "mean", "variance"))]),
                                                   t.predict(draws, nd, "loglik")))
    for k in s:
        assert np.array_equal(np.isnan(mir[k]), np.isnan(s[k])), k


# ---- §11 ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", TG.DTYPES, ids=["f64", "f32"])
def test_statuses(hip, monkeypatch, dtype):
    t, centre = model("poisson")
    N = 17
    e = engine(hip, t, N, dtype, TL.draws_of(t, centre, N, dtype))
    kern = TG.nuts_kernel(N, eps=0.02)
    nd = new_rows(t, 5)
    draws = TL.draws_of(t, centre, 3, dtype)

    def still_runs():
        e.transition(kern)
        assert np.isfinite(e.theta()).all() and e.stats()["n_steps"].min() >= 1

    with pytest.raises(A.ArgumentError, match="glm_predict: AHMC_GLM_PRED_LOGLIK needs newdata.y"):
        e.glm_predict(A.GLMNewData(nd.X, nd.factors, nd.offset), draws, what="loglik")
    bad = [f.copy() for f in nd.factors]
    bad[0][3] = 4
    for call in (lambda d: e.glm_predict(d, draws), lambda d: e.glm_predict_summary(d, draws)):
        with pytest.raises(A.ArgumentError, match=r"DomainError: levels\[4, 1\] = 4 is outside \[0, 4\)"):
            call(A.GLMNewData(nd.X, bad, nd.offset, nd.y))
        with pytest.raises(A.ArgumentError, match="newdata.levels is NULL; the bound model has 1 factors"):
            call(A.GLMNewData(nd.X, None, nd.offset, nd.y))
        Xn = nd.X.copy()
        Xn[2, 1] = np.nan
        with pytest.raises(A.ArgumentError, match="newdata.X holds a non-finite value"):
            call(A.GLMNewData(Xn, nd.factors, nd.offset, nd.y))
        yn = nd.y.copy()
        yn[4] = -1.0
        with pytest.raises(A.ArgumentError, match=r"y\[5\] = -1.000000 is outside the family's domain"):
            call(A.GLMNewData(nd.X, nd.factors, nd.offset, yn))
        still_runs()
    with pytest.raises(A.ArgumentError, match="unknown what = 9"):
        rec, keep = e._glm_newdata("glm_predict", nd)
        e._call("ahmc_glm_predict", C.byref(rec), capi.as_ptr(draws), 3, 9, capi.as_ptr(np.empty((5, 3), dtype=dtype)))
    with pytest.raises(A.ArgumentError, match="what = 'median'"):
        e.glm_predict(nd, draws, what="median")
    rec, keep = e._glm_newdata("glm_predict", nd)
    out = np.full((5, 3), 7.0, dtype=dtype, order="F")
    for args in ((None, capi.as_ptr(draws), 3, 1, capi.as_ptr(out)), (C.byref(rec), None, 3, 1, capi.as_ptr(out)), (C.byref(rec), capi.as_ptr(draws), 3, 1, None),
                 (C.byref(rec), capi.as_ptr(draws), -1, 1, capi.as_ptr(out))):
        with pytest.raises(A.ArgumentError, match="NULL|n_cols < 0"):
            e._call("ahmc_glm_predict", *args)
    with pytest.raises(A.UnsupportedError, match="2\\^31 - 1"):
        e._call("ahmc_glm_predict", C.byref(rec), capi.as_ptr(draws), 2 ** 31, 1, capi.as_ptr(out))
    # n_cols = 0 and n_new = 0 write nothing
    e._call("ahmc_glm_predict", C.byref(rec), None, 0, 1, None)
    e._call("ahmc_glm_predict", C.byref(rec), capi.as_ptr(draws), 0, 1, capi.as_ptr(out))
    assert np.all(out == 7.0)
    assert e.glm_predict(nd, np.zeros((t.D, 0))).shape == (5, 0)
    empty = A.GLMNewData(np.zeros((0, t.P_x)), [np.zeros(0, dtype=int)], None, None)
    assert e.glm_predict(empty, draws).shape == (0, 3) and e.glm_predict_summary(empty, draws)["lpd"].shape == (0,)
    assert np.isnan(e.glm_predict_summary(nd, np.zeros((t.D, 0)))["mean"]).all()
    # the byte budget: binding where it is given; a working set of one block of draws that does not fit is refused, naming the bytes
    monkeypatch.setenv("AHMC_GLM_PREDICT_BUDGET", "1000")
    for call in (lambda: e.glm_predict(nd, draws), lambda: e.glm_predict_summary(nd, draws)):
        with pytest.raises(A.AHMCError, match=r"cannot allocate \d+ bytes for the new data, one chunk of 64 draws .* within AHMC_GLM_PREDICT_BUDGET = 1000") as ei:
            call()
        assert ei.value.code == capi.ERR_RUNTIME
    monkeypatch.delenv("AHMC_GLM_PREDICT_BUDGET")
    still_runs()
    assert np.isfinite(e.glm_predict(nd, draws)).all()
    e.close()
    # VARIANCE of the class models
    for name in ("ordered", "categorical"):
        tc, cc = model(name)
        ec = engine(hip, tc, N, dtype)
        with pytest.raises(A.ArgumentError, match="AHMC_GLM_PRED_VARIANCE of a"):
            ec.glm_predict(new_rows(tc, 5), TL.draws_of(tc, cc, 3, dtype), what="variance")
        ec.close()
    # no GLM bound
    d = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((3, N)), A.IsoGaussian(3)), N, dtype=dtype, rng=A.PhiloxRNG(1), lib=hip)
    z = np.zeros((3, 2), dtype=dtype, order="F")
    rec0 = capi.GLMNewDataRecord(0, None, None, None, None)
    with pytest.raises(A.ArgumentError, match="glm_predict: no GLM is bound"):
        d._call("ahmc_glm_predict", C.byref(rec0), capi.as_ptr(z), 2, 1, capi.as_ptr(out))
    with pytest.raises(A.ArgumentError, match="glm_predict_summary: no GLM is bound"):
        d._call("ahmc_glm_predict_summary", C.byref(rec0), capi.as_ptr(z), 2, out.ctypes.data_as(C.POINTER(C.c_double)))
    d.close()
