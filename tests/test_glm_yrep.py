"""include/ahmc_glm_yrep.h: posterior-predictive draws y_rep of a GLM target and their per-observation summaries.

The sampler's contract is the host mirror glm.yrep_at.  On the CPU: the mirror draws from the right law (Pearson χ² against the exact
pmf, KS for the Gaussian), four planted defects fail that check, the C++ text of the sampler (csrc/ahmc_glm_yrep_draw.hpp, compiled into
tests/host_ref/glm_yrep_driver.cpp, a program of its own) equals the mirror, its loops are bounded whatever the input bits, the
summary's mirror agrees with a two-pass long-double reference, and the header, the bindings and the Julia ccalls agree.  On the device:
ahmc_glm_yrep_at against the mirror, the law of the device's output, the model path against the mirror applied to the device's own
planes, the invariances, the summary and the absence of side effects.

How two samplers are compared (the three rules):
  * Bernoulli and the class families: bit for bit.
  * Gaussian: |Δ| <= 8 × max(the mirror's deviation from long double, 8 u) × max(|y|, √v), u of the element type compared.
  * counts: equal wherever the mirror's margin (glm.py: the smallest relative distance of a decision it took) is >= 1e-9, the project's
    Float64 decision margin.  Poisson points with λ <= 10³ use seeds at which the mirror reports NO element under the margin, so nothing
    is excused there; elsewhere the mirror's own share under the margin must be <= 0.5 % and the excused share <= 1 %.  The negative
    binomial points fall under the second rule: Marsaglia–Tsang's `t <= 0` has the margin |t| = |1 + c·z|³ by the contract's formula,
    which is under 1e-9 for |1 + c·z| < 1e-3 — about 1e-4 of the elements at shape 1 (27 of 200 000 at (3, 1), 8 at (3, 0.2)); none of
    them differed.  At λ = 10¹² and 10¹⁵ the floor's margin (distance to an integer over |x|) is under 1e-9 for every element: there the
    rule excuses everything, and the test holds the two samplers to |Δ| <= 10·√λ instead — two draws from one law.
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
import tempfile

import numpy as np
import pytest

import ahmc_amd as A
import test_buffer_bounds as TB
import test_glm_loo as TL
import test_glm_predict as TP
import test_glm_target as TG
from ahmc_amd import _capi as capi
from ahmc_amd import glm as G
from arena_util import In, Out

LD = np.longdouble
ROOT = TG.ROOT
CSRC = os.path.join(ROOT, "advancedhmc.jl_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
DRIVER = os.path.join(ROOT, "tests", "host_ref", "glm_yrep_driver.cpp")
MARGIN = 1e-9
N_LAW = 200_000
P_BAR = 1e-4
MARGINS = {}


def dump_margins():
    out = os.environ.get("AHMC_TEST_OUT") or os.path.join(ROOT, "test_out")
    try:
        os.makedirs(out, exist_ok=True)
        path = os.path.join(out, "glm_yrep_margins.json")
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


def record(key, **kw):
    MARGINS[key] = kw
    dump_margins()
    print(key, kw)


def bits(key, got, want):
    TG.record_bits(f"yrep {key}", np.asarray(got), np.asarray(want))


# ------------------------------------------------------------------------------------------------
# the points: (family code, planes of one element, log-dispersion, categories)
# ------------------------------------------------------------------------------------------------
def _probs(C, zero=None):
    p = np.arange(1.0, C + 1.0)
    if zero is not None:
        p[zero] = 0.0
    return p / p.sum()


POINTS = {}
for _mu in (0.0, 1e-3, 0.5, 1.0):
    POINTS[f"bernoulli mu={_mu:g}"] = (0, (_mu,), None, 0)
for _lam in (1e-3, 0.5, 9.99, 10.0, 10.01, 37.0, 1e3, 1e6):
    POINTS[f"poisson lam={_lam:g}"] = (1, (_lam,), None, 0)
for _mu, _phi in ((3.0, 0.2), (3.0, 1.0), (50.0, 0.999), (50.0, 7.0), (1e4, 100.0)):
    POINTS[f"negbinomial mu={_mu:g} phi={_phi:g}"] = (4, (_mu,), float(np.log(_phi)), 0)
POINTS["gaussian mu=1 v=4"] = (2, (1.0, 4.0), None, 0)
POINTS["gaussian-sigma mu=-3 v=0.25"] = (3, (-3.0, 0.25), None, 0)
for _C in (2, 5, 16):
    POINTS[f"ordered C={_C}"] = (5, tuple(_probs(_C)), None, _C)
    POINTS[f"categorical C={_C} zero-class"] = (6, tuple(_probs(_C, zero=_C // 2)), None, _C)
LAW_POINTS = tuple(POINTS)
# the further points of the comparisons between two samplers
EDGE_POINTS = {"poisson lam=1e12": (1, (1e12,), None, 0), "poisson lam=0": (1, (0.0,), None, 0), "poisson lam=1e-300": (1, (1e-300,), None, 0),
               "poisson lam=1e15": (1, (1e15,), None, 0), "poisson lam=nan": (1, (np.nan,), None, 0), "poisson lam=inf": (1, (np.inf,), None, 0),
               "poisson lam=-inf": (1, (-np.inf,), None, 0), "bernoulli mu=nan": (0, (np.nan,), None, 0), "gaussian v=inf": (2, (0.0, np.inf), None, 0),
               "negbinomial mu=inf": (4, (np.inf,), 0.0, 0), "negbinomial s=inf": (4, (3.0,), np.inf, 0), "negbinomial s=-inf": (4, (3.0,), -np.inf, 0),
               "negbinomial s=nan": (4, (3.0,), np.nan, 0), "categorical C=5 nan": (6, (0.1, 0.2, np.nan, 0.3, 0.4), None, 5)}
ALL_POINTS = {**POINTS, **EDGE_POINTS}
# Seed of the comparisons: one at which the mirror reports no element under the margin at any Poisson point with λ <= 10³ (n = 200 000
# on the CPU, n = 4096 in either element type on the device) — the condition test 3 asserts.  Tried: 11 … 18.  Elements under the margin
# over those points and sizes together: 11: 1, 12: 1, 13: 1, 14 … 18: 0.  14, the first clear one, is kept.
SEED_CMP = 14
# Seeds of the law tests, tried on the host mirror: 1, 2, 3 (all three pass at every point); kept as they are.
SEEDS_LAW = (1, 2, 3)


def point_arrays(name, n, dtype=np.float64):
    """(family, q (planes, n), aux (n) or None, C) of a point, rounded to the element type compared"""
    fam, planes, s, Cc = ALL_POINTS[name]
    q = np.repeat(np.asarray(planes, dtype=np.float64)[:, None], n, axis=1).astype(dtype).astype(np.float64)
    aux = None if s is None else np.full(n, s).astype(dtype).astype(np.float64)
    return fam, q, aux, Cc


def counters(n, salt=0):
    """rows and columns that are not 0 … n − 1 and 0: the counter is what the element is given, not its position"""
    rs = np.random.default_rng([n, salt, 99])
    return rs.integers(0, 2 ** 31 - 1, n).astype(np.int32), rs.integers(0, 2 ** 31 - 1, n).astype(np.int32)


# ------------------------------------------------------------------------------------------------
# CPU 1, 2: the law
# ------------------------------------------------------------------------------------------------
def exact_law(name):
    """the scipy.stats distribution of a point's outcome (a frozen discrete law), or ("norm", μ, σ)"""
    from scipy import stats

    fam, planes, s, Cc = POINTS[name]
    if fam == 0:
        return stats.bernoulli(planes[0])
    if fam == 1:
        return stats.poisson(planes[0])
    if fam == 4:
        phi = np.exp(s)
        return stats.nbinom(phi, phi / (phi + planes[0]))
    if fam in (2, 3):
        return ("norm", planes[0], np.sqrt(planes[1]))
    return stats.rv_discrete(values=(np.arange(Cc), np.asarray(planes)))


def law_p_value(name, y):
    """p of Pearson's χ² of the outcomes y against the point's exact pmf, the cells (integers between the 1e-12 quantiles and the two
    tails) merged left to right until each expects >= 5; of the KS test for a Gaussian.  Outcomes the law gives probability 0 — a
    zero-probability class, a non-integer, a NaN — are an AssertionError of their own."""
    from scipy import stats

    law = exact_law(name)
    n = len(y)
    assert np.isfinite(y).all(), (name, "non-finite outcomes")
    if isinstance(law, tuple):
        return float(stats.kstest(y, "norm", args=law[1:]).pvalue)
    assert np.all(y == np.floor(y)) and y.min() >= 0, (name, "not a count")
    lo, hi = int(law.ppf(1e-12)), int(law.ppf(1 - 1e-12))
    lo = max(lo, 0)
    ks = np.arange(lo, hi + 1)
    pmf = law.pmf(ks)
    assert not np.any((pmf[(y[(y >= lo) & (y <= hi)] - lo).astype(np.int64)]) == 0.0), (name, "an outcome of probability 0")
    expect = np.concatenate([[law.cdf(lo - 1)], pmf, [law.sf(hi)]]) * n
    obs = np.bincount(np.clip(y - lo + 1, 0, len(ks) + 1).astype(np.int64), minlength=len(ks) + 2).astype(np.float64)
    cells_e, cells_o, e_acc, o_acc = [], [], 0.0, 0.0
    for e, o in zip(expect, obs):
        e_acc, o_acc = e_acc + e, o_acc + o
        if e_acc >= 5.0:
            cells_e.append(e_acc)
            cells_o.append(o_acc)
            e_acc = o_acc = 0.0
    if cells_e:
        cells_e[-1] += e_acc
        cells_o[-1] += o_acc
    else:
        cells_e, cells_o = [e_acc], [o_acc]
    ce, co = np.asarray(cells_e), np.asarray(cells_o)
    if len(ce) == 1:                                       # a point mass: every outcome is in the one cell
        return 1.0 if co[0] == n else 0.0
    stat = float(((co - ce) ** 2 / ce).sum())
    return float(stats.chi2.sf(stat, len(ce) - 1))


def edge_of_the_uniform(sampler):
    """u = 1 is a value of u53 (probability 2⁻⁵³, never met in 2·10⁵ draws): at μ = 1 the outcome is 1 with probability 1, so y = [u <= μ]
    must give 1 there, and a class model whose first class has probability 1 must give class 0.  `sampler(family, q, n_categories)`
    draws with every uniform equal to 1."""
    assert sampler(0, np.ones((1, 4)), None).tolist() == [1.0] * 4, "Bernoulli μ = 1 at u = 1"
    assert sampler(6, np.array([[1.0], [0.0], [0.0]]), 3).tolist() == [0.0], "class 0 of probability 1 at u = 1"
    assert sampler(1, np.zeros((1, 2)), None).tolist() == [0.0, 0.0], "Poisson λ = 0 at u = 1"


def law_check(name, seed, plant=None, sampler=None):
    """the whole of test 1 for one point and seed: p > 1e-4, and the edge u = 1"""
    fam, q, aux, Cc = point_arrays(name, N_LAW)
    row, col = counters(N_LAW, seed)
    if sampler is None:
        y, _ = G.yrep_at(fam, q, aux, row, col, seed=seed, n_categories=Cc or None, _plant=plant)
    else:
        y = sampler(fam, q, aux, row, col, seed, Cc)
    p = law_p_value(name, y)
    if sampler is None:
        edge_of_the_uniform(lambda f, qq, cc: G.yrep_at(f, qq, n_categories=cc, _plant=plant, _ones=True)[0])
    assert p > P_BAR, (name, seed, plant, p)
    return p


@pytest.mark.parametrize("name", LAW_POINTS)
def test_mirror_draws_from_the_right_law(name):
    """2·10⁵ elements of glm.yrep_at at fixed parameters against the exact pmf: Pearson's χ² (KS for the Gaussian) gives p > 1e-4 at seeds
    1, 2 and 3 — the three seeds tried; all pass at every point"""
    ps = {seed: law_check(name, seed) for seed in SEEDS_LAW}
    record(f"law mirror {name}", p_values={str(k): v for k, v in ps.items()}, seeds_tried=list(SEEDS_LAW), bar=P_BAR)


def test_mirror_mean_and_variance_at_a_huge_rate():
    """λ = 10¹²: the cells of a χ² would hold one outcome each; the mean within five standard errors √(λ/n), the variance within five
    standard errors λ·√(2/(n − 1))"""
    lam = 1e12
    for seed in SEEDS_LAW:
        row, col = counters(N_LAW, seed)
        y, _ = G.yrep_at(1, np.full((1, N_LAW), lam), None, row, col, seed=seed)
        zm = (y.mean() - lam) / np.sqrt(lam / N_LAW)
        zv = (y.var(ddof=1) - lam) / (lam * np.sqrt(2.0 / (N_LAW - 1)))
        record(f"law mirror poisson lam=1e12 seed={seed}", mean_in_se=float(zm), variance_in_se=float(zv))
        assert abs(zm) <= 5 and abs(zv) <= 5, (seed, zm, zv)


PLANTS = {"strict": ("bernoulli mu=1",), "ptrs-no-shift": ("poisson lam=10", "poisson lam=10.01", "poisson lam=37"),
          "gamma-no-boost": ("negbinomial mu=3 phi=0.2",), "inversion-from-1": ("poisson lam=0.5",)}


@pytest.mark.parametrize("plant", sorted(PLANTS))
def test_planted_defects_are_caught(plant):
    """`u < F` for `u <= F` (caught at the edge u = 1, where μ = 1 must still give 1), PTRS without the + 0.43, Marsaglia–Tsang without
    the u^(1/φ) boost, the inversion started at k = 1: each fails test 1 — its points at its three seeds — somewhere, at points that
    pass without the defect.
    The + 0.43 is the weak one, and the figures are kept here: PTRS's last step accepts against the exact pmf of whatever k was proposed,
    so dropping the shift moves the law only through the squeeze step — a mean 0.015 low at λ = 10 (two standard errors at n = 2·10⁵),
    less at λ = 37.  p of the χ² with the defect, seeds 1, 2, 3: λ = 10: 2.1e-4, 0.12, 0.047; λ = 10.01: 9.6e-5, 0.14, 0.065; λ = 37: 0.28,
    0.31, 0.38.  One of the nine is under the bar of 1e-4, so test 1 does fail with the defect in, but only just."""
    ps = {}
    for name in PLANTS[plant]:
        for seed in SEEDS_LAW:
            law_check(name, seed)
            try:
                law_check(name, seed, plant=plant)
                ps[f"{name} seed={seed}"] = "passed"
            except AssertionError as err:
                ps[f"{name} seed={seed}"] = "caught: " + str(err)[:80]
    record(f"planted {plant}", **ps)
    assert any(v.startswith("caught") for v in ps.values()), ps


# ------------------------------------------------------------------------------------------------
# CPU 3, 4: the C++ text of the sampler as a program of its own
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def driver():
    from ahmc_amd import build as B

    flags = ["-O1", "-std=c++17", "-ffp-contract=off"]
    h = hashlib.sha256()
    for p in (DRIVER, os.path.join(CSRC, "ahmc_glm_yrep_draw.hpp")):
        with open(p, "rb") as f:
            h.update(f.read())
    h.update(" ".join(flags).encode())
    out_dir = os.path.join(B.OBJ, "host_ref")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, f"glm_yrep_driver_{h.hexdigest()[:20]}")
    if not os.path.exists(exe):
        cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
        tmp = exe + f".tmp{os.getpid()}"
        res = subprocess.run([cxx, *flags, "-I", CSRC, DRIVER, "-o", tmp], capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"glm_yrep_driver build failed:\n{res.stdout}\n{res.stderr}")
        os.replace(tmp, exe)
    return exe


def driver_draw(fam, q, aux, row, col, seed, Cc, ones=False):
    """(y, blocks) of the C++ sampler for the elements given"""
    q = np.asarray(q, dtype=np.float64)
    n = q.shape[1]
    aux = np.zeros(n) if aux is None else np.broadcast_to(np.asarray(aux, dtype=np.float64), (n,))
    with tempfile.TemporaryDirectory(prefix="ahmc_yrep_") as td:
        fin, fout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(fin, "wb") as f:
            for a in (np.asfortranarray(q).tobytes(order="F"), np.ascontiguousarray(aux).tobytes(), np.asarray(row).astype(np.uint32).tobytes(),
                      np.asarray(col).astype(np.uint32).tobytes()):
                f.write(a)
        subprocess.run([driver(), str(int(fam)), str(int(Cc or 0)), str(n), str(int(seed)), "1" if ones else "0", fin, fout], check=True)
        raw = open(fout, "rb").read()
    return np.frombuffer(raw[:8 * n], dtype=np.float64).copy(), np.frombuffer(raw[8 * n:], dtype=np.int32).copy()


def gaussian_ld(q, row, col, seed):
    """the Gaussian outcome in long double from the element's own uniforms"""
    v = G.philox4x32_10(np.asarray(row).astype(np.uint64), np.asarray(col).astype(np.uint64), np.full(len(row), G.YREP_PURPOSE, dtype=np.uint64),
                        np.zeros(len(row), dtype=np.uint64), int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    u, up = G.u53(v[0], v[1]).astype(LD), G.u53(v[2], v[3]).astype(LD)
    z = np.sqrt(-2 * np.log(u)) * np.cos(2 * LD(np.pi) * up)      # (π to double: the contract's constant)
    return np.sqrt(q[1].astype(LD)) * z + q[0].astype(LD)


def same(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def compare(key, name, got, want, margin, q, row, col, seed, dtype=np.float64, zero_rule=True):
    """`got` against the mirror's `want` (both in the element type compared) under the module docstring's three rules; records what
    was measured"""
    fam = ALL_POINTS[name][0] if isinstance(name, str) else name
    u = float(TG.U[np.dtype(dtype)])
    if fam in (0, 5, 6):
        bits(key, got, want)
        return
    if fam in (2, 3):
        fin = np.isfinite(want.astype(np.float64))
        assert np.array_equal(np.isnan(got), np.isnan(want)), (key, "NaN pattern")
        if not fin.any():
            return
        scale = np.maximum(np.abs(want.astype(np.float64)), np.sqrt(q[1]))[fin]
        ref = gaussian_ld(q, row, col, seed)[fin]
        mir_u = float(np.max(np.abs(want.astype(LD)[fin] - ref) / scale) / u)
        dev_u = float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64))[fin] / scale) / u)
        record(key, mirror_from_long_double_u=mir_u, deviation_u=dev_u, bar_u=8 * max(mir_u, 8.0))
        assert dev_u <= 8 * max(mir_u, 8.0), MARGINS[key]
        return
    ne = ~same(got, want)
    under = margin < MARGIN
    lam = ALL_POINTS[name][1][0] if isinstance(name, str) and fam == 1 else None
    rec = dict(n=int(len(got)), differ=int(ne.sum()), under_margin=int(under.sum()), excused=int((ne & under).sum()), differ_above_margin=int((ne & ~under).sum()))
    record(key, **rec)
    assert rec["differ_above_margin"] == 0, (key, rec)
    if lam is not None and np.isfinite(lam) and lam > 1e6:
        # every element is under the floor's margin: two draws from one law instead (the module docstring)
        assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64))[ne] <= 10 * np.sqrt(lam) * (1 + 2 * u * np.sqrt(lam))), (key, rec)
        return
    if lam is not None and lam <= 1e3 and zero_rule:
        assert rec["under_margin"] == 0, (key, rec, "choose a seed at which the mirror is clear of the margin")
    assert rec["under_margin"] <= 0.005 * len(got) + (0 if len(got) >= 1000 else 1) and rec["excused"] <= 0.01 * len(got), (key, rec)


@pytest.mark.parametrize("name", tuple(ALL_POINTS))
def test_cpp_sampler_equals_the_mirror(name):
    """glm_yrep_driver — csrc/ahmc_glm_yrep_draw.hpp under the host compiler — against glm.yrep_at on 2·10⁵ elements per point, at
    counters that are not the elements' positions, under the three rules"""
    fam, q, aux, Cc = point_arrays(name, N_LAW)
    row, col = counters(N_LAW)
    want, margin = G.yrep_at(fam, q, aux, row, col, seed=SEED_CMP, n_categories=Cc or None)
    got, blocks = driver_draw(fam, q, aux, row, col, SEED_CMP, Cc)
    compare(f"cpp-vs-mirror {name}", name, got, want, margin, q, row, col, SEED_CMP)
    assert blocks.max() <= 1 + 3 * G.YREP_MAX_ROUNDS


def test_cpp_sampler_loops_are_bounded():
    """10⁶ random 64-bit patterns reinterpreted as (μ, s) through the negative binomial's sampler and as λ through the Poisson's: the
    program returns for every element, having taken at most 1 + 2·64 + 64 blocks (the boost, 64 rounds of two, 64 rounds of PTRS); with
    every uniform equal to 1 — PTRS rejects us = 0 for ever, Marsaglia–Tsang's log u = 0 is never below its bound at z = 0… — the
    capped exit is NaN after exactly the cap"""
    n = 10 ** 6
    pat = np.random.default_rng(5).integers(0, 2 ** 64, size=(2, n), dtype=np.uint64).view(np.float64)
    row, col = np.arange(n), np.zeros(n)
    y4, b4 = driver_draw(4, pat[:1], pat[1], row, col, 3, 0)
    y1, b1 = driver_draw(1, pat[:1], None, row, col, 3, 0)
    cap = 1 + 3 * G.YREP_MAX_ROUNDS
    assert b4.max() <= cap and b1.max() <= G.YREP_MAX_ROUNDS and len(y4) == len(y1) == n
    ok = np.isfinite(pat[0]) & (pat[0] >= 0)
    assert np.isnan(y1[~ok]).all() and np.isfinite(y1[ok]).all()
    m = 64
    yo, bo = driver_draw(1, np.full((1, m), 50.0), None, row[:m], col[:m], 3, 0, ones=True)
    assert np.isnan(yo).all() and np.all(bo == G.YREP_MAX_ROUNDS)
    yn, bn = driver_draw(4, np.full((1, m), 50.0), np.log(0.5), row[:m], col[:m], 3, 0, ones=True)
    ym, _ = G.yrep_at(4, np.full((1, m), 50.0), np.log(0.5), row[:m], col[:m], seed=3, _ones=True)
    assert np.array_equal(np.isnan(yn), np.isnan(ym)) and bn.max() <= cap
    record("bounded-loops", worst_blocks_random_negbinomial=int(b4.max()), worst_blocks_random_poisson=int(b1.max()), worst_blocks_all_ones_poisson=int(bo.max()),
           worst_blocks_all_ones_negbinomial=int(bn.max()), cap=cap, nan_share_random_negbinomial=float(np.isnan(y4).mean()))


def test_refusals_of_yrep_at_in_order():
    """yrep_at_refusal, the host-only decision of ahmc_glm_yrep_at: a call that violates two conditions is answered with the earlier"""
    def ans(family=1, Cc=0, n=3, q=1, aux=1, y=1):
        return int(subprocess.run([driver(), "check", str(family), str(Cc), str(n), str(q), str(aux), str(y)], capture_output=True, text=True, check=True).stdout)

    assert ans() == 0 and ans(family=4) == 0 and ans(family=6, Cc=16) == 0 and ans(family=5, Cc=2) == 0 and ans(n=0, q=0, y=0) == 0
    assert ans(family=7, Cc=1, n=-1, q=0) == 1 and ans(family=-1) == 1
    assert ans(family=5, Cc=1, n=-1, q=0) == 2 and ans(family=6, Cc=17) == 2 and ans(family=1, Cc=99) == 0
    assert ans(q=0) == 3 and ans(y=0) == 3 and ans(family=4, aux=0) == 3 and ans(family=1, aux=0) == 0
    assert ans(n=-1, q=0, y=0) == 4


# ------------------------------------------------------------------------------------------------
# CPU 5: the summary's mirror
# ------------------------------------------------------------------------------------------------
def yrep_cases(S):
    """y_rep (6, S) and outcomes y (6): Poisson counts small and large, Bernoulli, a Gaussian with a large mean, a constant, classes"""
    rs = np.random.default_rng([S, 23])
    v = np.stack([rs.poisson(0.7, S), rs.poisson(1e6, S), rs.integers(0, 2, S), 100.0 + 0.5 * rs.normal(size=S), np.full(S, 3.0), rs.integers(0, 5, S)]).astype(np.float64)
    y = np.array([1.0, 1e6, 1.0, 100.0, 3.0, 2.0])
    return v, y


@pytest.mark.parametrize("S", TP.S_ALL)
def test_mirror_summary_against_two_pass_long_double(S):
    """glm.yrep_summary against a two-pass long-double mean and variance under the bars of tests/test_glm_predict.py (means within 8 u,
    variances within VARIANCE_BAR_U and the a-priori bound); the counts are exact; chunks of 64 and 128 give the bits of one chunk"""
    v, y = yrep_cases(S)
    got = G.yrep_summary(v, y)
    assert got.shape == (4, 6)
    rec = TP.summary_check(f"yrep-summary S={S}", np.vstack([got[:2], np.full((1, 6), np.nan)]), v[None], None, record=False)
    record(f"mirror-summary S={S}", **rec)
    assert np.array_equal(got[2], (v < y[:, None]).sum(axis=1) / float(S)) and np.array_equal(got[3], (v == y[:, None]).sum(axis=1) / float(S))
    assert got[3, 4] == 1.0 and got[2, 4] == 0.0 and got[0, 4] == 3.0
    assert np.isnan(got[1]).all() if S == 1 else np.isfinite(got).all()
    for chunk in (64, 128):
        assert np.array_equal(TG.bits_of(G.yrep_summary(v, y, chunk=chunk)), TG.bits_of(got)), chunk
    no_y = G.yrep_summary(v)
    assert np.isnan(no_y[2:]).all() and np.array_equal(no_y[:2], got[:2], equal_nan=True)
    if S > 1:
        v[0, S // 2] = np.nan                                   # a capped exit: NaN moments for that observation, the counts skip it
        bad = G.yrep_summary(v, y)
        assert np.isnan(bad[:2, 0]).all() and np.isfinite(bad[:, 1:]).all() and bad[2, 0] == (v[0] < 1.0).sum() / float(S)


def test_mirror_yrep_is_yrep_at_on_the_matrix():
    """glm.yrep: element (i, j) is yrep_at with the counter (i, j) and the draw's dispersion"""
    rs = np.random.default_rng(2)
    mu, s = np.exp(rs.normal(size=(1, 5, 7))), rs.normal(size=7)
    y, m = G.yrep("negbinomial_log", mu, s, seed=9)
    for i, j in ((0, 0), (4, 6), (2, 3)):
        yi, mi = G.yrep_at(4, mu[:, i, j:j + 1], s[j], row=[i], col=[j], seed=9)
        assert yi[0] == y[i, j] and mi[0] == m[i, j]
    assert not np.array_equal(y, G.yrep("negbinomial_log", mu, s, seed=10)[0])


# ------------------------------------------------------------------------------------------------
# CPU 6: the interface
# ------------------------------------------------------------------------------------------------
def header_prototypes():
    src = open(os.path.join(INCLUDE, "ahmc_glm_yrep.h"), encoding="utf-8").read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(int32_t)\s+(ahmc_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", code, flags=re.S):
        params = " ".join(m.group(3).split())
        protos[m.group(2)] = [] if params in ("", "void") else [p.strip() for p in params.split(",")]
    return protos, code, src


NAMES = {"ahmc_glm_yrep_version", "ahmc_glm_yrep_at", "ahmc_glm_yrep", "ahmc_glm_yrep_summary"}


def test_header_and_bindings_agree():
    protos, code, src = header_prototypes()
    assert set(protos) == set(capi.GLM_YREP_SIGNATURES) == NAMES
    older = set().union(*[set(getattr(capi, n)) for n in dir(capi) if n.endswith("SIGNATURES") and n != "GLM_YREP_SIGNATURES"])
    assert not NAMES & older
    ct = {"double*": C.POINTER(C.c_double), "int32_t*": C.POINTER(C.c_int32), "int64_t": C.c_int64, "int32_t": C.c_int32, "uint64_t": C.c_uint64}
    for name, params in protos.items():
        res, args = capi.GLM_YREP_SIGNATURES[name]
        assert res is C.c_int32 and len(args) == len(params), name
        for p, a in zip(params, args):
            typ = p.rsplit(" ", 1)[0].replace("const ", "").replace(" ", "")
            assert a is (C.c_void_p if typ in ("void*", "ahmc_ctx*", "ahmc_glm_newdata*") else ct[typ]), (name, p)
    assert [p.split()[-1] for p in protos["ahmc_glm_yrep_at"]] == ["ctx", "family", "n_categories", "n", "q", "aux", "row", "col", "seed", "y_out"]
    assert [p.split()[-1] for p in protos["ahmc_glm_yrep"]] == ["ctx", "newdata", "theta", "n_cols", "seed", "out"]
    assert [p.split()[-1] for p in protos["ahmc_glm_yrep_summary"]] == ["ctx", "newdata", "theta", "n_cols", "seed", "summary_out"]
    assert re.search(r"#define AHMC_GLM_YREP_VERSION (\d+)", code).group(1) == str(capi.AHMC_GLM_YREP_VERSION) == "1"
    assert '#include "ahmc_glm_predict.h"' in code
    # what the header must say: the cap and its probability, and that a permutation of the rows changes y_rep
    assert "capped at 64 rounds" in src and "1e-40" in src and "PERMUTATION OF THE ROWS CHANGES y_rep" in src and "0x59524550" in src
    from ahmc_amd import build as B
    assert "ahmc_glm_yrep.h" in open(B.__file__, encoding="utf-8").read()
    draw = open(os.path.join(CSRC, "ahmc_glm_yrep_draw.hpp"), encoding="utf-8").read()
    assert "hip" not in re.sub(r"//[^\n]*", "", draw).lower().replace("__hipcc__", "")          # the host compiler alone builds it
    for const, v in (("YREP_MAX_ROUNDS", G.YREP_MAX_ROUNDS), ("YREP_INVERSION_MAX", G.YREP_INVERSION_MAX)):
        assert re.search(rf"constexpr int {const} = (\d+);", draw).group(1) == str(v)
    assert re.search(r"YREP_PURPOSE = 0x([0-9A-Fa-f]+)u;", draw).group(1).lower() == f"{G.YREP_PURPOSE:x}"
    # the older headers keep their versions
    for hdr, macro, v in (("ahmc_hip.h", "AHMC_ABI_VERSION", capi.AHMC_ABI_VERSION), ("ahmc_glm.h", "AHMC_GLM_VERSION", capi.AHMC_GLM_VERSION),
                          ("ahmc_glm_loo.h", "AHMC_GLM_LOO_VERSION", capi.AHMC_GLM_LOO_VERSION),
                          ("ahmc_glm_predict.h", "AHMC_GLM_PREDICT_VERSION", capi.AHMC_GLM_PREDICT_VERSION)):
        assert re.search(rf"#define {macro} (\d+)", open(os.path.join(INCLUDE, hdr), encoding="utf-8").read()).group(1) == str(v), hdr


def test_julia_ccalls_match_the_header():
    protos, _, _ = header_prototypes()
    src = open(os.path.join(ROOT, "julia", "AdvancedHMCMI355XGLMYrep.jl"), encoding="utf-8").read()
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
                if "int32_t" in p:
                    assert t == "Ptr{Cint}", (name, t, p)
                if "ahmc_glm_newdata" in p:
                    assert t == "Ref{GLMNewDataRecord}", (name, t, p)
            else:
                assert {"int64_t": "Int64", "int32_t": "Cint", "uint64_t": "UInt64"}[p.split()[0]] == t, (name, t, p)
    assert seen == set(protos)
    ext = open(os.path.join(ROOT, "julia", "AdvancedHMCMI355XExt.jl"), encoding="utf-8").read()
    assert 'include("AdvancedHMCMI355XGLMYrep.jl")' in ext and "ahmc_glm_yrep" not in ext.replace("ahmc_glm_yrep.h", "")
    assert ext.index('include("AdvancedHMCMI355XGLMPredict.jl")') < ext.index('include("AdvancedHMCMI355XGLMYrep.jl")')


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="needs llvm-objdump")
def test_library_exports_and_kernels_without_scratch():
    """every entry point is in the dynamic symbol table; k_glm_yrep of both element types and the five samplers, the block kernel of
    both and the fold are in the code object with no private segment, no vector-register spill, within a wave's registers and 40 KiB of
    LDS; and the y_rep calls brought no further instantiation of k_glm_pred"""
    from ahmc_amd import build as B

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_meta
    finally:
        sys.path.pop(0)
    assert os.path.exists(B.OUT), "build() first"
    exported = {l.split()[-1] for l in subprocess.run(["nm", "-D", "--defined-only", B.OUT], capture_output=True, text=True, check=True).stdout.splitlines() if l.strip()}
    assert NAMES <= exported, NAMES - exported
    meta = kernel_meta.kernel_meta(B.OUT)
    names = subprocess.run(["c++filt"], input="\n".join(k["name"] for k in meta), capture_output=True, text=True, check=True).stdout.splitlines()
    want = {f"k_glm_yrep<{T}, {fam}>" for T in ("float", "double") for fam in (0, 1, 2, 4, 5)} | {f"k_glm_yrep_blocks<{T}>" for T in ("float", "double")}
    want |= {"k_glm_yrep_fold"}
    found, pred = {}, 0
    for k, dn in zip(meta, names):
        head = dn.split("(")[0].replace("void ", "")
        if head.startswith("ahmc::k_glm_yrep"):
            found[head[len("ahmc::"):]] = k
        pred += head.startswith("ahmc::k_glm_pred<")
    assert set(found) == want, (sorted(want - set(found)), sorted(set(found) - want))
    assert pred == 56, pred
    for w, k in found.items():
        assert k["private_segment_fixed_size"] == 0, (w, k)
        assert k.get("vgpr_spill_count", 0) == 0, (w, k)
        assert k["vgpr_count"] + k.get("agpr_count", 0) <= 512, (w, k)
        assert k["group_segment_fixed_size"] <= 40 * 1024, (w, k)


def test_engine_needs_the_header():
    """a library without the header's symbols answers UnsupportedError, not a fallback; newdata=None needs a bound GLMTarget"""
    class Lib:
        has_glm_yrep = False
        has_glm_predict = True
        path = "libother.so"

    e = A.Engine.__new__(A.Engine)
    e.lib = Lib()
    for call in (lambda: e.glm_yrep(A.GLMNewData(np.zeros((2, 2)))), lambda: e.glm_yrep_summary(), lambda: e.glm_yrep_at(0, np.zeros((1, 2)))):
        with pytest.raises(A.UnsupportedError, match="ahmc_glm_yrep.h"):
            call()
    Lib.has_glm_yrep = True
    with pytest.raises(A.ArgumentError, match="newdata=None means the rows of the bound GLMTarget"):
        e.glm_yrep()
    with pytest.raises(ValueError, match="n_categories"):
        G.yrep_at("categorical_logit", np.zeros((3, 2)), n_categories=1)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        G.yrep_at("gaussian_identity", np.zeros((1, 2)))
    with pytest.raises(ValueError, match="needs aux"):
        G.yrep_at("negbinomial_log", np.ones((1, 2)))


# ---------------------------------------------------------------------------------------------------------------------
# the guard-band cases of the new entry points: registered in the table of tests/test_buffer_bounds.py, whose gate counts them
# ---------------------------------------------------------------------------------------------------------------------
def c_yrep(r, n_new, S, where):
    """newdata (the record itself, host memory), theta and out of ahmc_glm_yrep, newdata, theta and summary_out of ahmc_glm_yrep_summary,
    each sized exactly, from device and host draws, on the model with groups, factors and a dispersion (D = 10, N = 5); and q, aux, row,
    col and y_out of ahmc_glm_yrep_at for the negative binomial (every array is read) and a class family (C planes an element)"""
    D, n_obs = 10, 70
    dll = r.lib.dll
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rs = np.random.default_rng([n_new, S, 5])
    for dtype in (TB.F64, TB.F32):
        mk = lambda: TB.bound_glm(r, n_obs, dtype)  # noqa: E731
        X = np.asfortranarray(rs.normal(size=(n_new, 3)), dtype=dtype)
        lev = np.asfortranarray(np.column_stack([rs.integers(0, 2, n_new), rs.integers(0, 3, n_new)]), dtype=np.int32)
        y = rs.normal(size=n_new).astype(dtype)
        rec = capi.GLMNewDataRecord(n_new, X.ctypes.data, lev.ctypes.data_as(pi), None, y.ctypes.data)
        rec_bytes = np.frombuffer(bytes(rec), dtype=np.uint8).copy()
        th = (0.4 * rs.normal(size=D * S)).astype(dtype)
        for w_in in ("device", "host"):
            r.probe(mk, lambda e, io: r.ok(e, dll.ahmc_glm_yrep(e._ctx, io["ahmc_glm_yrep.newdata"], io["ahmc_glm_yrep.theta"], S, 5, io["ahmc_glm_yrep.out"])),
                    ins={"ahmc_glm_yrep.newdata": In(rec_bytes, "host"), "ahmc_glm_yrep.theta": In(th, w_in)}, outs={"ahmc_glm_yrep.out": Out(dtype, n_new * S, where)})
            r.probe(mk, lambda e, io: r.ok(e, dll.ahmc_glm_yrep_summary(e._ctx, io["ahmc_glm_yrep_summary.newdata"], io["ahmc_glm_yrep_summary.theta"], S, 5,
                                                                        C.cast(io["ahmc_glm_yrep_summary.summary_out"], pd))),
                    ins={"ahmc_glm_yrep_summary.newdata": In(rec_bytes, "host"), "ahmc_glm_yrep_summary.theta": In(th, w_in)},
                    outs={"ahmc_glm_yrep_summary.summary_out": Out(np.float64, 4 * n_new if S else 0, where)})
            n = n_new * max(S, 1)
            mu = np.exp(rs.normal(size=n)).astype(dtype)
            s = rs.normal(size=n).astype(dtype)
            row, col = counters(n)
            r.probe(mk, lambda e, io: r.ok(e, dll.ahmc_glm_yrep_at(e._ctx, 4, 0, n, io["ahmc_glm_yrep_at.q"], io["ahmc_glm_yrep_at.aux"], C.cast(io["ahmc_glm_yrep_at.row"], pi),
                                                                   C.cast(io["ahmc_glm_yrep_at.col"], pi), 5, io["ahmc_glm_yrep_at.y_out"])),
                    ins={"ahmc_glm_yrep_at.q": In(mu, w_in), "ahmc_glm_yrep_at.aux": In(s, w_in), "ahmc_glm_yrep_at.row": In(row, w_in), "ahmc_glm_yrep_at.col": In(col, w_in)},
                    outs={"ahmc_glm_yrep_at.y_out": Out(dtype, n, where)})
            p = np.tile(_probs(5), n).astype(dtype)
            r.probe(mk, lambda e, io: r.ok(e, dll.ahmc_glm_yrep_at(e._ctx, 6, 5, n, io["ahmc_glm_yrep_at.q"], None, None, None, 5, io["ahmc_glm_yrep_at.y_out"])),
                    ins={"ahmc_glm_yrep_at.q": In(p, w_in)}, outs={"ahmc_glm_yrep_at.y_out": Out(dtype, n, where)})
        del X, lev, y


_PROBES = ["ahmc_glm_yrep.newdata", "ahmc_glm_yrep.theta", "ahmc_glm_yrep.out", "ahmc_glm_yrep_summary.newdata", "ahmc_glm_yrep_summary.theta",
           "ahmc_glm_yrep_summary.summary_out", "ahmc_glm_yrep_at.q", "ahmc_glm_yrep_at.aux", "ahmc_glm_yrep_at.row", "ahmc_glm_yrep_at.col", "ahmc_glm_yrep_at.y_out"]
BOUNDS_CASES = []
for _n, _s in ((65, 65), (1, 3)):
    for _w in ("device", "host"):
        _cid = f"glm-yrep-nnew{_n}-S{_s}-{_w}"
        if _cid not in TB.CASES:
            TB.add(_cid, c_yrep, _PROBES, oracle=False, n_new=_n, S=_s, where=_w)
        BOUNDS_CASES.append(_cid)


def test_bounds_cases_cover_the_header():
    """the six pointers of the two model calls and the five arrays of ahmc_glm_yrep_at"""
    params = {p for p in TB.header_pointer_params() if p[0] in capi.GLM_YREP_SIGNATURES and p[1] != "ctx"}
    probed = {tuple(k.split(".")) for cid in BOUNDS_CASES for k in TB.CASES[cid].probes}
    assert params == probed and len(params) == 11 and len({p for p in params if p[0] != "ahmc_glm_yrep_at"}) == 6


@pytest.mark.gpu
@pytest.mark.parametrize("cid", BOUNDS_CASES)
def test_hip_bounds(hip, monkeypatch, cid):
    """no call reads or writes outside the caller's arrays (tests/arena_util.py), at n_new = 65 and S = 65 among others"""
    TB.run_case(hip, monkeypatch, cid)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bare(hip):
    """contexts with no GLM bound, one per element type: ahmc_glm_yrep_at needs none"""
    es = {np.dtype(dt): A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((3, 4)), A.IsoGaussian(3)), 4, dtype=dt, rng=A.PhiloxRNG(1), lib=hip) for dt in TG.DTYPES}
    yield es
    for e in es.values():
        e.close()


# ---- 7 ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", TG.DTYPES, ids=["f64", "f32"])
def test_yrep_at_against_the_mirror(bare, dtype):
    """ahmc_glm_yrep_at on every point of the CPU comparison, n = 4096 a point and n = 1, 63, 65 (a prefix: an element does not depend on
    n), against glm.yrep_at on the planes rounded to the element type, under the three rules"""
    e = bare[np.dtype(dtype)]
    dn = np.dtype(dtype).name
    n = 4096
    row, col = counters(n)
    for name in ALL_POINTS:
        fam, q, aux, Cc = point_arrays(name, n, dtype)
        want, margin = G.yrep_at(fam, q, aux, row, col, seed=SEED_CMP, n_categories=Cc or None)
        got = e.glm_yrep_at(fam, q, aux, row, col, seed=SEED_CMP, n_categories=Cc)
        assert got.dtype == np.dtype(dtype) and got.shape == (n,)
        with np.errstate(over="ignore"):
            compare(f"device-at {name} {dn}", name, got, want.astype(dtype), margin, q, row, col, SEED_CMP, dtype)
        for m in (1, 63, 65):
            part = e.glm_yrep_at(fam, q[:, :m], None if aux is None else aux[:m], row[:m], col[:m], seed=SEED_CMP, n_categories=Cc)
            bits(f"device-at prefix {name} n={m} {dn}", part, got[:m])
    # the default counters are 0 … n − 1 and 0
    fam, q, aux, Cc = point_arrays("poisson lam=37", 65, dtype)
    bits(f"device-at default-counters {dn}", e.glm_yrep_at(fam, q, seed=4), e.glm_yrep_at(fam, q, row=np.arange(65), col=np.zeros(65, dtype=int), seed=4))
    assert not np.array_equal(e.glm_yrep_at(fam, q, seed=4), e.glm_yrep_at(fam, q, seed=5))


# ---- 8 ----
@pytest.mark.gpu
@pytest.mark.parametrize("name", ("poisson lam=0.5", "poisson lam=37", "negbinomial mu=3 phi=0.2", "negbinomial mu=50 phi=7", "categorical C=5 zero-class"))
def test_law_on_the_device(bare, name):
    """test 1's χ² on the device's output, one point per branch of the sampler"""
    e = bare[np.dtype(np.float64)]
    p = law_check(name, SEEDS_LAW[0], sampler=lambda fam, q, aux, row, col, seed, Cc: e.glm_yrep_at(fam, q, aux, row, col, seed=seed, n_categories=Cc))
    record(f"law device {name}", p_value=p, seed=SEEDS_LAW[0], bar=P_BAR)


# ---- 9 ----
def device_planes(e, t, nd, draws, n_cols=None):
    """the planes the sampler reads, from the device's own ahmc_glm_predict: (planes, n_new, S), and the draws' log-dispersion"""
    mean = e.glm_predict(nd, draws, n_cols, what="mean")
    mean = mean if mean.ndim == 3 else mean[None]
    if t.family in (G.GAUSSIAN_IDENTITY, G.GAUSSIAN_IDENTITY_SIGMA) and not (t.n_classes or t.n_categories):
        mean = np.concatenate([mean, e.glm_predict(nd, draws, n_cols, what="variance")[None]], axis=0)
    return mean


def mirror_yrep(t, planes, draws, seed, dtype):
    fam = 6 if t.n_classes else 5 if t.n_categories else t.family
    aux = np.asarray(draws)[-1].astype(np.float64) if fam == G.NEGBINOMIAL_LOG else None
    y, m = G.yrep(fam, planes.astype(np.float64), aux, seed=seed, n_categories=(t.n_classes or t.n_categories or None))
    with np.errstate(over="ignore"):
        return y.astype(dtype), m, fam


def compare_matrix(key, fam, got, want, margin, planes, seed, dtype):
    n_new, S = got.shape
    row, col = np.repeat(np.arange(n_new), S), np.tile(np.arange(S), n_new)
    q = planes.astype(np.float64).reshape(planes.shape[0], -1)
    compare(key, fam, got.ravel(), want.ravel(), margin.ravel(), q, row, col, seed, dtype, zero_rule=False)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", TG.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", TP.FAMILIES)
def test_model_path_against_the_mirror_on_the_devices_planes(hip, monkeypatch, name, dtype):
    """ahmc_glm_yrep at new rows equals glm.yrep applied to the device's own ahmc_glm_predict planes (and the draws' dispersion), under
    the three rules, at n_new ∈ {1, 64, 65, 130} × S ∈ {1, 63, 64, 65, 200}; S = 4100 in five chunks of 832 draws once"""
    t, centre = TP.model(name)
    e = TP.engine(hip, t, TP.N_CHAINS, dtype)
    dn = np.dtype(dtype).name
    shapes = [(n_new, S, None) for n_new in TP.N_NEW for S in (1, 63, 64, 65, 200)] + ([(65, 4100, 832)] if dtype is np.float64 else [])
    worst = {}
    for n_new, S, chunk in shapes:
        nd = TP.new_rows(t, n_new)
        draws = TL.draws_of(t, centre, S, dtype, spread=0.3)
        planes = device_planes(e, t, nd, draws)
        with TP.chunk_of(monkeypatch, chunk):
            got = e.glm_yrep(nd, draws, seed=SEED_CMP)
        assert got.shape == (n_new, S) and got.dtype == np.dtype(dtype)
        want, margin, fam = mirror_yrep(t, planes, draws, SEED_CMP, dtype)
        key = f"model-path {name} n_new={n_new} S={S} {dn}"
        compare_matrix(key, fam, got, want, margin, planes, SEED_CMP, dtype)
        for k, v in MARGINS.pop(key, {}).items():
            worst[k] = max(worst.get(k, 0), v)
    record(f"model-path {name} {dn}", **worst)
    e.close()


# ---- 10 ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", TG.DTYPES, ids=["f64", "f32"])
def test_invariances_bit_for_bit(hip, monkeypatch, dtype):
    """the same new rows, draws and seed: contexts with N = 37 and N = 48; forced chunks of 64 and 192 draws; host arrays against device
    pointers for θ, the new data and the outputs; the first 65 of 130 rows give the first 65 outputs; newdata=None is the training rows
    given explicitly.  Two seeds differ, and a PERMUTATION OF THE ROWS CHANGES y_rep: the counter holds the row."""
    import torch

    t, centre = TP.model("negbinomial")
    dn = np.dtype(dtype).name
    S, n_new, seed = 200, 130, 77
    nd = TP.new_rows(t, n_new)
    draws = TL.draws_of(t, centre, S, dtype)
    a = TP.engine(hip, t, 37, dtype)
    full = a.glm_yrep(nd, draws, seed=seed)
    summ = a.glm_yrep_summary(nd, draws, seed=seed)
    names = sorted(summ)
    assert names == ["mean", "p_equal", "p_less", "var"] and np.isfinite(full).all()
    for cols in (64, 192):
        with TP.chunk_of(monkeypatch, cols):
            bits(f"inv-chunk{cols} {dn}", a.glm_yrep(nd, draws, seed=seed), full)
            sc = a.glm_yrep_summary(nd, draws, seed=seed)
        for k in names:
            bits(f"inv-chunk{cols} summary {k} {dn}", sc[k], summ[k])
    d_dev = torch.from_numpy(np.ascontiguousarray(draws.T)).cuda()
    bits(f"inv-theta-pointer {dn}", a.glm_yrep(nd, d_dev.data_ptr(), n_cols=S, seed=seed), full)
    sp = a.glm_yrep_summary(nd, d_dev.data_ptr(), n_cols=S, seed=seed)
    for k in names:
        bits(f"inv-theta-pointer summary {k} {dn}", sp[k], summ[k])
    X_dev, y_dev = (TG.dev(np.asarray(v, dtype=dtype)) for v in (nd.X, nd.y))
    rec = capi.GLMNewDataRecord(n_new, X_dev.data_ptr(), None, None, y_dev.data_ptr())
    out_dev = torch.empty(n_new * S, dtype=torch.float64 if np.dtype(dtype) == np.float64 else torch.float32, device="cuda")
    a._call("ahmc_glm_yrep", C.byref(rec), C.c_void_p(d_dev.data_ptr()), S, seed, C.c_void_p(out_dev.data_ptr()))
    bits(f"inv-device-data {dn}", TG.host(out_dev, (n_new, S)), full)
    sum_dev = torch.empty(4 * n_new, dtype=torch.float64, device="cuda")
    a._call("ahmc_glm_yrep_summary", C.byref(rec), C.c_void_p(d_dev.data_ptr()), S, seed, C.cast(C.c_void_p(sum_dev.data_ptr()), C.POINTER(C.c_double)))
    sd = TG.host(sum_dev, (4, n_new))
    for i, k in enumerate(("mean", "var", "p_less", "p_equal")):
        bits(f"inv-device-data summary {k} {dn}", sd[i], summ[k])
    first = A.GLMNewData(nd.X[:65], None, None, nd.y[:65])
    bits(f"inv-first65 {dn}", a.glm_yrep(first, draws, seed=seed), full[:65])
    s65 = a.glm_yrep_summary(first, draws, seed=seed)
    for k in names:
        bits(f"inv-first65 summary {k} {dn}", s65[k], summ[k][:65])
    # the counter holds the row: the permuted rows' planes are the rows' planes permuted, their outcomes are not
    perm = np.roll(np.arange(n_new), 1)
    permuted = A.GLMNewData(nd.X[perm], None, None, nd.y[perm])
    bits(f"inv-rows planes {dn}", a.glm_predict(permuted, draws), a.glm_predict(nd, draws)[perm])
    yp = a.glm_yrep(permuted, draws, seed=seed)
    assert (yp != full[perm]).mean() > 0.5, "a row permutation must change y_rep"
    assert (a.glm_yrep(nd, draws, seed=seed + 1) != full).mean() > 0.5, "two seeds differ"
    bits(f"inv-repeat {dn}", a.glm_yrep(nd, draws, seed=seed), full)
    # newdata=None: the bound target's own rows
    bits(f"inv-training-rows {dn}", a.glm_yrep(None, draws, seed=seed), a.glm_yrep(TP.training_rows(t), draws, seed=seed))
    st, sn = a.glm_yrep_summary(TP.training_rows(t), draws, seed=seed), a.glm_yrep_summary(None, draws, seed=seed)
    for k in names:
        bits(f"inv-training-rows summary {k} {dn}", sn[k], st[k])
    a.close()
    b = TP.engine(hip, t, 48, dtype)
    bits(f"inv-N {dn}", b.glm_yrep(nd, draws, seed=seed), full)
    sb = b.glm_yrep_summary(nd, draws, seed=seed)
    b.close()
    for k in names:
        bits(f"inv-N summary {k} {dn}", sb[k], summ[k])


# ---- 11 ----
SUMMARY_CASES = [(name, 65, 200, np.float64) for name in TL.FAMILIES] + [("negbinomial", n_new, S, np.float32) for n_new, S in ((1, 1), (64, 63), (130, 65), (65, 64))] + \
                [("poisson", 65, 4100, np.float64)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,n_new,S,dtype", SUMMARY_CASES, ids=[f"{c[0]}-n{c[1]}-S{c[2]}-{np.dtype(c[3]).name}" for c in SUMMARY_CASES])
def test_summary_equals_the_mirror_on_the_devices_own_yrep(hip, monkeypatch, name, n_new, S, dtype):
    """ahmc_glm_yrep_summary against glm.yrep_summary applied to ahmc_glm_yrep's matrix for the same seed: the moments bit for bit, the
    counts exact; S = 4100 runs in chunks of 1024 draws (five); without outcomes the same moments and NaN shares"""
    t, centre = TP.model(name)
    nd = TP.new_rows(t, n_new)
    draws = TL.draws_of(t, centre, S, dtype, spread=0.3)
    e = TP.engine(hip, t, TP.N_CHAINS, dtype)
    yrep = e.glm_yrep(nd, draws, seed=3)
    with TP.chunk_of(monkeypatch, 1024 if S > 1024 else None):
        got = e.glm_yrep_summary(nd, draws, seed=3)
    mir = G.yrep_summary(yrep, nd.y.astype(dtype))
    key = f"device-summary {name} n_new={n_new} S={S} {np.dtype(dtype).name}"
    for i, k in enumerate(("mean", "var", "p_less", "p_equal")):
        bits(f"{key} {k}", got[k], mir[i])
    assert np.isnan(got["var"]).all() if S == 1 else np.isfinite(got["var"]).all()
    no_y = e.glm_yrep_summary(A.GLMNewData(nd.X, nd.factors, nd.offset), draws, seed=3)
    bits(f"{key} without-y mean", no_y["mean"], got["mean"])
    bits(f"{key} without-y var", no_y["var"], got["var"])
    assert np.isnan(no_y["p_less"]).all() and np.isnan(no_y["p_equal"]).all()
    e.close()


@pytest.mark.gpu
def test_summary_on_the_conjugate_gaussian_model(hip):
    """the conjugate model of tests/test_glm_predict.py (n = 40, P = 3, S = 4000 exact posterior draws, unit noise), 200 new rows whose
    outcomes are drawn from the exact predictive N(x_iᵀm, 1 + x_iᵀV x_i): the mean of y_rep within five Monte-Carlo standard errors
    √((1 + x_iᵀV x_i)/S), its variance within five standard errors (1 + x_iᵀV x_i)·√(2/(S − 1)), and p_less — the PIT of outcomes that
    come from the predictive — uniform by KS at p > 1e-4.  Seeds 1, 4, 7 of that file's test are used as they are; no other was tried."""
    from scipy import stats

    S, n_new = 4000, 200
    for seed in TP.SEEDS:
        m, V, beta, Xn, _ = TP.conjugate_predictive(40, 3, S, n_new, seed)
        xv = 1.0 + np.einsum("ij,jk,ik->i", Xn, V, Xn)
        yn = Xn @ m + np.sqrt(xv) * np.random.default_rng([seed, 5]).normal(size=n_new)
        rs = np.random.default_rng(seed)
        t = A.GLMTarget(rs.normal(size=(40, 3)), rs.normal(size=40), family="gaussian_identity", prior_scale=2.5, scale=1.0)
        e = TP.engine(hip, t, 4, np.float64)
        s = e.glm_yrep_summary(A.GLMNewData(Xn, y=yn), beta, seed=seed)
        e.close()
        zm = np.abs(s["mean"] - Xn @ m) / np.sqrt(xv / S)
        zv = np.abs(s["var"] - xv) / (xv * np.sqrt(2.0 / (S - 1)))
        p = float(stats.kstest(s["p_less"], "uniform").pvalue)
        record(f"conjugate-yrep seed={seed}", mean_in_se=float(zm.max()), variance_in_se=float(zv.max()), pit_ks_p=p, seeds_tried=list(TP.SEEDS))
        assert zm.max() <= 5 and zv.max() <= 5 and p > P_BAR, MARGINS[f"conjugate-yrep seed={seed}"]
        assert np.all(s["p_equal"] == 0.0)


# ---- 12 ----
@pytest.mark.gpu
@pytest.mark.parametrize("name", ("negbinomial", "categorical"))
def test_no_side_effects(hip, bare, name):
    """a NUTS transition after the three calls has the bits of a twin context that made none: θ, r, the statistics and the RNG's position
    (a second transition); ahmc_glm_pointwise of the bound model is unchanged"""
    t, centre = TP.model(name)
    N = TP.N_CHAINS
    th0 = TL.draws_of(t, centre, N, np.float64)
    kern = TG.nuts_kernel(N, eps=0.1, depth=5)
    e, twin = (TP.engine(hip, t, N, np.float64, th0, seed=21) for _ in range(2))
    for c in (e, twin):
        c.transition(kern)
    before = e.glm_pointwise()
    nd = TP.new_rows(t, 65)
    draws = TL.draws_of(t, centre, 130, np.float64)
    e.glm_yrep(nd, draws, seed=1)
    e.glm_yrep_summary(nd, draws, seed=1)
    e.glm_yrep(seed=2)
    e.glm_yrep_at(1, np.full((1, 100), 20.0), seed=3)
    after = e.glm_pointwise()
    for k, (x, y) in enumerate(zip(before, after)):
        bits(f"side-effects pointwise {k} {name}", y, x)
    for step in range(2):
        e.transition(kern)
        twin.transition(kern)
        bits(f"side-effects theta {step} {name}", e.theta(), twin.theta())
        bits(f"side-effects r {step} {name}", e.phasepoint().r, twin.phasepoint().r)
        se, st = e.stats(), twin.stats()
        for k in se:
            np.testing.assert_array_equal(se[k], st[k], err_msg=k)
    e.close()
    twin.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", TG.DTYPES, ids=["f64", "f32"])
def test_non_finite_draws(hip, dtype):
    """Poisson draws whose exp overflows (observation 9: η = 1000·θ_0, at draw 77 and wherever else θ_0 is large enough for the element
    type): NaN for exactly the elements of y_rep whose μ the device gives as Inf, and in that observation's moments; the other
    observations are finite and the counts skip the NaN draws, as the mirror's do"""
    t, centre = TP.model("poisson-plain", 70, 2)
    nd = TP.new_rows(t, 65)
    X = nd.X.copy()
    X[9] = (1000.0, 0.0)
    nd = A.GLMNewData(X, y=nd.y)
    centre = centre.copy()
    centre[0] = 0.5
    draws = TL.draws_of(t, centre, 130, dtype, spread=0.1)
    draws[0, 77] = 1.0
    e = TP.engine(hip, t, TP.N_CHAINS, dtype)
    y = e.glm_yrep(nd, draws, seed=8)
    s = e.glm_yrep_summary(nd, draws, seed=8)
    bad = ~np.isfinite(e.glm_predict(nd, draws, what="mean"))
    e.close()
    assert bad[9, 77] and not np.delete(bad, 9, axis=0).any()
    assert np.array_equal(np.isnan(y), bad)
    mir = G.yrep_summary(y, nd.y.astype(dtype))
    for i, k in enumerate(("mean", "var", "p_less", "p_equal")):
        bits(f"non-finite {k} {np.dtype(dtype).name}", s[k], mir[i])
    assert np.isnan(s["mean"][9]) and np.isnan(s["var"][9]) and np.isfinite(np.delete(s["mean"], 9)).all() and np.isfinite(s["p_less"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", TG.DTYPES, ids=["f64", "f32"])
def test_statuses(hip, bare, monkeypatch, dtype):
    t, centre = TP.model("poisson")
    N = 17
    e = TP.engine(hip, t, N, dtype, TL.draws_of(t, centre, N, dtype))
    kern = TG.nuts_kernel(N, eps=0.02)
    nd = TP.new_rows(t, 5)
    draws = TL.draws_of(t, centre, 3, dtype)
    pd = C.POINTER(C.c_double)

    def still_runs():
        e.transition(kern)
        assert np.isfinite(e.theta()).all() and e.stats()["n_steps"].min() >= 1

    bad = [f.copy() for f in nd.factors]
    bad[0][3] = 4
    for who, call in (("glm_yrep", lambda d: e.glm_yrep(d, draws)), ("glm_yrep_summary", lambda d: e.glm_yrep_summary(d, draws))):
        with pytest.raises(A.ArgumentError, match=rf"{who}: DomainError: levels\[4, 1\] = 4 is outside \[0, 4\)"):
            call(A.GLMNewData(nd.X, bad, nd.offset, nd.y))
        with pytest.raises(A.ArgumentError, match=f"{who}: newdata.levels is NULL; the bound model has 1 factors"):
            call(A.GLMNewData(nd.X, None, nd.offset, nd.y))
        Xn = nd.X.copy()
        Xn[2, 1] = np.nan
        with pytest.raises(A.ArgumentError, match=f"{who}: ArgumentError: newdata.X holds a non-finite value"):
            call(A.GLMNewData(Xn, nd.factors, nd.offset, nd.y))
        yn = nd.y.copy()
        yn[4] = -1.0
        with pytest.raises(A.ArgumentError, match=rf"{who}: DomainError: y\[5\] = -1.000000 is outside the family's domain"):
            call(A.GLMNewData(nd.X, nd.factors, nd.offset, yn))
        still_runs()
    rec, keep = e._glm_newdata("glm_yrep", nd)
    out = np.full((5, 3), 7.0, dtype=dtype, order="F")
    sout = np.full((4, 5), 7.0, order="F")
    for args in ((None, capi.as_ptr(draws), 3, 1, capi.as_ptr(out)), (C.byref(rec), None, 3, 1, capi.as_ptr(out)), (C.byref(rec), capi.as_ptr(draws), 3, 1, None),
                 (C.byref(rec), capi.as_ptr(draws), -1, 1, capi.as_ptr(out))):
        with pytest.raises(A.ArgumentError, match="glm_yrep: .*(NULL|n_cols < 0)"):
            e._call("ahmc_glm_yrep", *args)
    with pytest.raises(A.ArgumentError, match="glm_yrep_summary: theta or the output is NULL"):
        e._call("ahmc_glm_yrep_summary", C.byref(rec), capi.as_ptr(draws), 3, 1, None)
    with pytest.raises(A.UnsupportedError, match="2\\^31 - 1"):
        e._call("ahmc_glm_yrep", C.byref(rec), capi.as_ptr(draws), 2 ** 31, 1, capi.as_ptr(out))
    e._call("ahmc_glm_yrep", C.byref(rec), None, 0, 1, None)
    e._call("ahmc_glm_yrep", C.byref(rec), capi.as_ptr(draws), 0, 1, capi.as_ptr(out))
    e._call("ahmc_glm_yrep_summary", C.byref(rec), capi.as_ptr(draws), 0, 1, sout.ctypes.data_as(pd))
    assert np.all(out == 7.0) and np.all(sout == 7.0)
    assert e.glm_yrep(nd, np.zeros((t.D, 0))).shape == (5, 0) and np.isnan(e.glm_yrep_summary(nd, np.zeros((t.D, 0)))["mean"]).all()
    empty = A.GLMNewData(np.zeros((0, t.P_x)), [np.zeros(0, dtype=int)], None, None)
    assert e.glm_yrep(empty, draws).shape == (0, 3) and e.glm_yrep_summary(empty, draws)["p_less"].shape == (0,)
    monkeypatch.setenv("AHMC_GLM_PREDICT_BUDGET", "1000")
    for call in (lambda: e.glm_yrep(nd, draws), lambda: e.glm_yrep_summary(nd, draws)):
        with pytest.raises(A.AHMCError, match=r"cannot allocate \d+ bytes for the new data, one chunk of 64 draws .*y_rep of the chunk.* within AHMC_GLM_PREDICT_BUDGET = 1000") as ei:
            call()
        assert ei.value.code == capi.ERR_RUNTIME
    monkeypatch.delenv("AHMC_GLM_PREDICT_BUDGET")
    still_runs()
    assert np.isfinite(e.glm_yrep(nd, draws)).all() and e.glm_yrep().shape == (70, N)
    e.close()
    # no GLM bound: the model calls refuse, ahmc_glm_yrep_at answers, and refuses in its own order
    d = bare[np.dtype(dtype)]
    z = np.zeros((3, 2), dtype=dtype, order="F")
    rec0 = capi.GLMNewDataRecord(0, None, None, None, None)
    with pytest.raises(A.ArgumentError, match="glm_yrep: no GLM is bound"):
        d._call("ahmc_glm_yrep", C.byref(rec0), capi.as_ptr(z), 2, 1, capi.as_ptr(out))
    with pytest.raises(A.ArgumentError, match="glm_yrep_summary: no GLM is bound"):
        d._call("ahmc_glm_yrep_summary", C.byref(rec0), capi.as_ptr(z), 2, 1, sout.ctypes.data_as(pd))
    q = np.ones(4, dtype=dtype)
    yo = np.full(4, 7.0, dtype=dtype)
    at = lambda fam, Cc, n, qq, aa, yy: d._call("ahmc_glm_yrep_at", fam, Cc, n, capi.as_ptr(qq), capi.as_ptr(aa), None, None, 1, capi.as_ptr(yy))  # noqa: E731
    with pytest.raises(A.ArgumentError, match="glm_yrep_at: unknown family 7"):
        at(7, 1, -1, None, None, None)
    with pytest.raises(A.ArgumentError, match="glm_yrep_at: n_categories = 17 is outside 2 … 16"):
        at(6, 17, -1, None, None, None)
    for qq, aa, yy in ((None, q, yo), (q, None, yo), (q, q, None)):
        with pytest.raises(A.ArgumentError, match="glm_yrep_at: q, y_out or the dispersion aux of a negative binomial is NULL"):
            at(4, 0, 4, qq, aa, yy)
    with pytest.raises(A.ArgumentError, match="glm_yrep_at: n must be >= 0; got -1"):
        at(1, 0, -1, None, None, None)
    at(1, 0, 0, None, None, None)
    assert np.all(yo == 7.0)
    at(1, 0, 4, q, None, yo)
    assert np.all(yo == np.floor(yo)) and np.all(yo >= 0)
