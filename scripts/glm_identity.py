"""Two builds of the engine do the same on every kind of GLM: results, refusals, launches, host cost → profiles/glm_host_refactor.json.

    python scripts/glm_identity.py identity  --base BASE.so --new NEW.so [--out FILE]
    python scripts/glm_identity.py refusals  --base BASE.so --new NEW.so [--write-golden]
    python scripts/glm_identity.py launches  --base BASE.so --new NEW.so
    python scripts/glm_identity.py speed     --base BASE.so --new NEW.so [--rounds 4]

For a change of the host side that must leave every result as it was (the method of profiles/glm_refactor_identity.json, for all
kinds of model).  The parent never opens the GPU.  Every measurement is a child process of its own under a time limit of its own,
AHMC_HIP_LIB selecting the library in it; the parent checks each exit status and stops at the first child that fails or times out.

  * identity.  Per kind (plain families 0, 1, 2; family 0 with groups; families 3 and 4 with groups; factors with a dispersion;
    ordinal with groups and a factor; categorical with a factor and a whole-block group — the group tables, level counts, category
    counts and cut prior of the tests' VALUE_CASES, ocase and ccase), at 130 observations (three row blocks, the last partial) and
    1100 (two K slices), Float64 and Float32, N = 40, a fixed PhiloxRNG, once with AHMC_GLM_SMALL_BELOW=0 and once with it large:
    phasepoint(), a static-HMC and two NUTS transitions with theta() and every stats() array after each, glm_pointwise(), every
    draw entry point that applies on the current θ and on 2N + 3 host draws, glm_loo with log weights.  sha256 over dtype, shape
    and bytes of every array; every hash must be equal.
  * refusals.  The table of tests/golden/glm_bind_refusals.json (defined here: refusal_table) through the C ABI, and the draw entry
    points' refusals; status and ahmc_last_error text must be equal.  --write-golden: the BASE library's answers become the file.
  * launches.  One evaluation and every draw entry point per kind under `rocprofv3 --kernel-trace --stats`, once per library: equal
    calls per kernel name.
  * speed.  Whole-loop host-clock windows where the host path is the largest share, children of the two libraries alternating:
    the NUTS loop at (8192, 256, 8192) Float64; evaluations of the categorical model (4096, 32, 4) at N = 16384; 16-chain
    evaluations at (8192, 256).  The new median must be no worse than the base's own worst window.
"""
import argparse
import csv
import ctypes as C
import glob
import hashlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "glm_host_refactor.json")
GOLDEN = os.path.join(ROOT, "tests", "golden", "glm_bind_refusals.json")
DTYPES = {"f64": np.float64, "f32": np.float32}
N_ID = 40
GROUPS2 = ((0, 2, True, 0.8), (2, 5, False, 1.3))      # (tests/test_glm_aux.py: VALUE_CASES; tests/test_glm_ordinal.py: GROUPS2)
CUT_PRIOR = (0.3, 2.0, -0.2, 0.8)                      # (tests/test_glm_ordinal.py)
KINDS = ("plain0", "plain1", "plain2", "hier0", "aux3", "aux4", "factor_aux", "ordinal", "categorical")


def merge(path, key, value):
    res = json.load(open(path)) if os.path.exists(path) else {}
    res[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


def target(kind, n_obs, seed=0):
    """the model of one kind at n_obs observations"""
    import ahmc_amd as A

    rs = np.random.default_rng([seed, n_obs, KINDS.index(kind)])
    Px = {"factor_aux": 2, "ordinal": 3, "categorical": 2}.get(kind, 5)
    X = rs.normal(size=(n_obs, Px)) / np.sqrt(Px)
    eta = X @ rs.normal(size=Px)
    off = 0.3 * rs.normal(size=n_obs)
    groups = [A.CoefGroup(*g) for g in GROUPS2]
    if kind in ("plain0", "hier0"):
        y = (rs.random(n_obs) < 1 / (1 + np.exp(-eta))).astype(np.float64)
        if kind == "plain0":
            return A.GLMTarget(X, y, prior_prec=2 * rs.random(Px), offset=off)
        return A.HierGLMTarget(X, y, groups, prior_prec=2 * rs.random(Px), offset=off)
    if kind == "plain1":
        return A.GLMTarget(X, rs.poisson(np.exp(eta)).astype(np.float64), family="poisson_log", prior_prec=2 * rs.random(Px), offset=off)
    if kind == "plain2":
        return A.GLMTarget(X, eta + rs.normal(size=n_obs), family="gaussian_identity", prior_prec=2 * rs.random(Px), offset=off, scale=1.7)
    if kind == "aux3":
        return A.HierGLMTarget(X, eta + 0.7 * rs.normal(size=n_obs), groups, family="gaussian_identity_sigma", prior_prec=2 * rs.random(Px), offset=off,
                               aux_prior=(0.2, 0.9))
    if kind == "aux4":
        return A.HierGLMTarget(X, rs.poisson(np.exp(eta)).astype(np.float64), groups, family="negbinomial_log", prior_prec=2 * rs.random(Px), offset=off,
                               aux_prior=(0.2, 0.9))
    facs = [A.Factor(rs.integers(0, L, size=n_obs), L) for L in ((7, 1) if kind == "factor_aux" else (4,) if kind == "ordinal" else (3,))]
    P = Px + sum(f.n_levels for f in facs)
    if kind == "factor_aux":
        return A.GLMTarget(X, eta + 0.7 * rs.normal(size=n_obs), family="gaussian_identity_sigma", prior_prec=2 * rs.random(P), offset=off, aux_prior=(0.2, 0.9),
                           factors=facs)
    if kind == "ordinal":
        return A.HierGLMTarget(X, rs.integers(0, 5, size=n_obs), [A.CoefGroup(0, 2, True, 0.8), A.CoefGroup(Px, P, False, 1.3)], family="ordered_logit",
                               prior_prec=2 * rs.random(P), offset=off, factors=facs, n_categories=5, cut_prior=CUT_PRIOR)
    # categorical: C = 4, blocks of P rows; a group inside the first block, the whole second block as one group
    return A.HierGLMTarget(X, rs.integers(0, 4, size=n_obs), [A.CoefGroup(0, 2, True, 0.8), A.CoefGroup(P, 2 * P, False, 1.3)], family="categorical_logit",
                           prior_prec=2 * rs.random(3 * P), offset=0.3 * rs.normal(size=(n_obs, 3)), factors=facs, n_categories=4)


def engine(t, N, dtype, lib, eps=0.05):
    import ahmc_amd as A

    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((t.D, N)), t), N, dtype=dtype, rng=A.PhiloxRNG(7), lib=lib)
    e.set_integrator(A.Leapfrog(eps))
    return e


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(f"{a.dtype.str}{a.shape}".encode() + a.tobytes()).hexdigest()[:24]


def draw_calls(e, t, draws, out, tag):
    """every draw entry point that applies to t"""
    if t.groups or t.aux or t.factors or t.n_categories or t.n_classes:
        b, tau = e.hglm_coefficients(draws)
        out[tag + "beta"], out[tag + "tau"] = digest(b), digest(tau)
    if t.aux:
        out[tag + "dispersion"] = digest(e.glm_dispersion(draws))
    if t.n_categories:
        out[tag + "cutpoints"] = digest(e.glm_cutpoints(draws))
    if t.n_classes:
        out[tag + "class_probs"] = digest(e.glm_class_probs(draws))
    out[tag + "loglik"] = digest(e.glm_loglik(draws))
    if draws is not None:
        for k, v in e.glm_loo(draws, log_weights=True).items():
            out[tag + "loo." + k] = digest(v)


# ---- children (these open the GPU) ----
def child_identity(dt):
    import ahmc_amd as A

    lib = A.load_hip_library()
    res = {}
    for kind in KINDS:
        for n_obs in (130, 1100):
            t = target(kind, n_obs)
            rs = np.random.default_rng([n_obs, KINDS.index(kind)])
            th0, draws = 0.2 * rs.normal(size=(t.D, N_ID)), 0.3 * rs.normal(size=(t.D, 2 * N_ID + 3))
            for small in ("0", "1000000000"):
                os.environ["AHMC_GLM_SMALL_BELOW"] = small
                out = res[f"{kind}/{n_obs}/{dt}/small_below={small}"] = {}
                e = engine(t, N_ID, DTYPES[dt], lib)
                e.set_position(th0)
                z = e.phasepoint()
                out.update({"z.theta": digest(z.theta), "z.r": digest(z.r), "z.lp": digest(z.lp.value), "z.grad": digest(z.lp.gradient)})
                lf = A.Leapfrog(0.05)
                hmc = A.HMCKernel(A.Trajectory(A.EndPointTS, lf, A.FixedNSteps(3)))
                nuts = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=4)))
                for i, kern in enumerate((hmc, nuts, nuts)):
                    e.transition(kern)
                    out[f"t{i}.theta"] = digest(e.theta())
                    for k, v in e.stats().items():
                        out[f"t{i}.{k}"] = digest(v)
                eta, ll = e.glm_pointwise()
                out["eta"], out["ll"] = digest(eta), digest(ll)
                draw_calls(e, t, None, out, "cur.")
                draw_calls(e, t, draws, out, "draws.")
                e.close()
    print("RESULT " + json.dumps(res), flush=True)


def num(v):
    return float(v) if isinstance(v, str) else v


def materialise(table, case, dtype):
    """the arguments of one case of the refusal table: its base model with the case's fields set and elements poked; arrays in the
    element type, the integer tables int32, hyper_scale and cut_prior double; None where the case passes NULL"""
    m = dict(table["bases"][case["base"]])
    m.update(case.get("set", {}))
    kinds = {"X": dtype, "y": dtype, "offset": dtype, "prior_prec": dtype, "lo": np.int32, "hi": np.int32, "centered": np.int32, "hyper_scale": np.float64,
             "n_levels": np.int32, "levels": np.int32, "cut_prior": np.float64}
    for k, dt in kinds.items():
        m[k] = None if m.get(k) is None else np.array([num(v) for v in m[k]], dtype=dt)
    for k, i, v in case.get("poke", ()):
        m[k][i] = num(v)
    m.setdefault("n_groups", 0 if m["lo"] is None else len(m["lo"]))
    m.setdefault("n_factors", 0 if m["n_levels"] is None else len(m["n_levels"]))
    for k in ("scale", "aux_loc", "aux_scale"):
        m[k] = num(m[k])
    return m


ENTRIES = ("plain", "hier", "aux", "factor", "ordinal", "categorical")   # (ahmc::GlmEntry)


def write_golden(table):
    """one line per base and per case; an answer that is the same in both element types is written once (expected())"""
    for c in table["cases"]:
        if isinstance(c["expect"], dict) and c["expect"]["f64"] == c["expect"]["f32"]:
            c["expect"] = c["expect"]["f64"]
    line = lambda v: json.dumps(v, ensure_ascii=False, separators=(",", ":"))
    with open(GOLDEN, "w") as f:
        f.write('{"bases":{\n' + ",\n".join(f"{json.dumps(k)}:{line(v)}" for k, v in table["bases"].items()) + '\n},\n"cases":[\n')
        f.write(",\n".join(line(c) for c in table["cases"]) + "\n]}\n")


def expected(case, dt):
    """[status, message] that the table records for one case in one element type"""
    return case["expect"][dt] if isinstance(case["expect"], dict) else case["expect"]


def refusal_table():
    """the bases and the cases of tests/golden/glm_bind_refusals.json, without the expectations.  Every value is exact in Float32."""
    rs = np.random.default_rng(5)
    n = 20

    def grid(size, s=16.0):
        return [float(v) for v in np.round(rs.normal(size=size) * s) / s]

    def base(entry, family, Px, D, groups=(), n_levels=(), has_aux=0, n_categories=0, cut_prior=None, K=1, y=None, P=None):
        P = P or (Px + sum(n_levels)) * K
        p = [float(v) for v in np.round(rs.random(P) * 8) / 8]
        for lo, hi, _, _ in groups:
            p[lo:hi] = [0.0] * (hi - lo)
        return dict(entry=ENTRIES.index(entry), D=D, N=4, family=family, n_obs=n, n_coef=Px, X=grid(n * Px), y=y, offset=grid(n * K, 8.0), prior_prec=p, scale=1.0,
                    lo=[g[0] for g in groups], hi=[g[1] for g in groups], centered=[int(g[2]) for g in groups], hyper_scale=[g[3] for g in groups],
                    n_levels=list(n_levels), levels=[int(v) for L in n_levels for v in rs.integers(0, L, size=n)], has_aux=has_aux, aux_loc=0.25, aux_scale=1.5,
                    n_categories=n_categories, cut_prior=cut_prior)

    y01 = [float(v) for v in rs.integers(0, 2, size=n)]
    yc = [float(v) for v in rs.integers(0, 3, size=n)]
    g2 = ((0, 1, True, 0.75), (1, 3, False, 1.25))
    bases = {
        "plain": base("plain", 0, 3, 3, y=y01),
        "hier": base("hier", 0, 3, 5, g2, y=y01),
        "aux": base("aux", 3, 3, 6, g2, has_aux=1, y=grid(n)),
        "factor": base("factor", 0, 2, 2 + 4 + 1, ((2, 5, False, 1.25),), (3, 1), y=y01),
        "ordinal": base("ordinal", 5, 2, 2 + 3 + 1 + 2, ((2, 5, False, 1.25),), (3,), n_categories=3, cut_prior=[0.25, 2.0, -0.25, 0.75], y=yc),
        "categorical": base("categorical", 6, 2, 2 * 5 + 2, ((0, 2, True, 0.75), (5, 10, False, 1.25)), (3,), n_categories=3, K=2, y=yc),
    }
    cases = []

    def add(b, name, **kw):
        poke = kw.pop("poke", None)
        c = {"name": f"{b}: {name}", "base": b}
        if kw:
            c["set"] = kw
        if poke:
            c["poke"] = [list(q) for q in poke]
        cases.append(c)

    big = (1 << 24) + 1
    for b in bases:
        add(b, "accepted")
        # what every entry point refuses (tests/test_glm_target.py: test_refusals, repeated by the other five)
        add(b, "n_obs = 0", n_obs=0)
        add(b, "n_obs = -3", n_obs=-3)
        add(b, "n_obs above AHMC_GLM_MAX_OBS", n_obs=big)
        add(b, "X NULL", X=None)
        add(b, "y NULL", y=None)
        add(b, "NaN in X", poke=[("X", 7, "nan")])
        add(b, "inf at the end of X", poke=[("X", n * bases[b]["n_coef"] - 1, "inf")])
        add(b, "-inf in offset", poke=[("offset", 3, "-inf")])
        add(b, "NaN in prior_prec", poke=[("prior_prec", 1, "nan")])
        add(b, "negative prior_prec", poke=[("prior_prec", len(bases[b]["prior_prec"]) - 1, -0.125)])
        add(b, "y = 1.5", poke=[("y", 5, 1.5)])
        add(b, "y = -0.125", poke=[("y", 5, -0.125)])
        add(b, "y NaN", poke=[("y", 0, "nan")])
        add(b, "y = -1 at the end", poke=[("y", n - 1, -1.0)])
        add(b, "y inf", poke=[("y", n - 1, "inf")])
        if b in ("plain", "hier", "factor"):
            for s in (0.0, -1.0, "inf", "nan"):
                add(b, f"scale = {s}", scale=s)
            for fam in (1, 2):
                add(b, f"family {fam}, y = -1", family=fam, poke=[("y", n - 1, -1.0)])
                add(b, f"family {fam}, y inf", family=fam, poke=[("y", n - 1, "inf")])
                add(b, f"family {fam}, y NaN", family=fam, poke=[("y", 1, "nan")])
        if b in ("plain", "hier", "aux", "factor"):
            for fam in (-1, 0, 1, 2, 3, 4, 5, 6, 7):
                add(b, f"family {fam}", family=fam)
        if b == "factor":
            for fam in (0, 3, 4, 5, 6):
                add(b, f"family {fam} with has_aux", family=fam, has_aux=1, D=bases[b]["D"] + 1)
        if b != "plain":
            # include/ahmc_glm_hier.h (tests/test_glm_hier.py)
            P = bases[b]["D"] - len(bases[b]["lo"]) - (1 if b == "aux" else 0) - (2 if b == "ordinal" else 0)
            add(b, "n_coef + 1", n_coef=bases[b]["n_coef"] + 1)
            add(b, "n_coef = 0", n_coef=0)
            add(b, "one group fewer", lo=bases[b]["lo"][:-1], hi=bases[b]["hi"][:-1], centered=bases[b]["centered"][:-1], hyper_scale=bases[b]["hyper_scale"][:-1])
            add(b, "n_groups = -1", n_groups=-1)
            lo, hi = list(bases[b]["lo"]), list(bases[b]["hi"])
            add(b, "an empty group", hi=[lo[0]] + hi[1:])
            add(b, "a reversed group", lo=[hi[0]] + lo[1:], hi=[lo[0]] + hi[1:])
            add(b, "a group beyond n_coef", hi=hi[:-1] + [P + 1])
            add(b, "a group from -1", lo=[-1] + lo[1:])
            if len(lo) > 1:
                add(b, "the first group one longer", hi=[hi[0] + 1] + hi[1:])
                add(b, "groups out of order", lo=lo[::-1], hi=hi[::-1])
            add(b, "lo NULL", lo=None, n_groups=len(lo))
            add(b, "hi NULL", hi=None)
            add(b, "hyper_scale NULL", hyper_scale=None)
            for a in (0.0, -1.0, "inf", "nan"):
                add(b, f"hyper_scale = {a}", hyper_scale=[a] + list(bases[b]["hyper_scale"][1:]))
            add(b, "a precision on a member", poke=[("prior_prec", hi[-1] - 1, 0.5)])
            for G in (32, 33):
                add(b, f"{G} groups", lo=list(range(G)), hi=list(range(1, G + 1)), centered=[0] * G, hyper_scale=[1.0] * G)
        if b in ("aux", "factor"):
            # include/ahmc_glm_aux.h (tests/test_glm_aux.py)
            extra = dict(has_aux=1, family=3, D=bases[b]["D"] + 1) if b == "factor" else {}
            for v in ("inf", "nan"):
                add(b, f"aux_loc = {v}", aux_loc=v, **extra)
            for v in (0.0, -1.0, "inf", "nan"):
                add(b, f"aux_scale = {v}", aux_scale=v, **extra)
            add(b, "family 4, y = -1", poke=[("y", 2, -1.0)], **dict(extra, family=4))
        if b in ("factor", "ordinal", "categorical"):
            # include/ahmc_glm_factor.h (tests/test_glm_factor.py)
            L = bases[b]["n_levels"]
            add(b, "n_factors = -1", n_factors=-1)
            add(b, "n_factors = 9", n_factors=9)
            add(b, "n_levels NULL", n_levels=None, n_factors=len(L))
            add(b, "levels NULL", levels=None)
            add(b, "a factor without levels", n_levels=[0] + L[1:])
            add(b, "a level index = n_levels", poke=[("levels", 4, L[0])])
            add(b, "a level index = -1", poke=[("levels", n - 1, -1)])
            add(b, "2^30 coefficient rows", n_levels=[1 << 30] + L[1:])
        if b == "ordinal":
            # include/ahmc_glm_ordinal.h (tests/test_glm_ordinal.py)
            for c in (1, 0, 17):
                add(b, f"n_categories = {c}", n_categories=c)
            add(b, "n_categories = 4", n_categories=4)
            add(b, "cut_prior NULL", cut_prior=None)
            for i, v in ((0, "nan"), (1, 0.0), (1, -1.0), (2, "inf"), (3, "nan"), (3, 0.0)):
                add(b, f"cut_prior[{i}] = {v}", poke=[("cut_prior", i, v)])
            add(b, "y = 3: not a category", poke=[("y", 4, 3.0)])
        if b == "categorical":
            # include/ahmc_glm_categorical.h (tests/test_glm_categorical.py)
            for c in (1, 0, 17):
                add(b, f"n_categories = {c}", n_categories=c)
            add(b, "n_categories = 4", n_categories=4)
            add(b, "y = 3: not a class", poke=[("y", 4, 3.0)])
            add(b, "a group that straddles the blocks", lo=[0, 4], hi=[2, 7])
            add(b, "-inf in the second class's offset", poke=[("offset", n + 3, "-inf")])
            add(b, "2^30 rows in all blocks", n_levels=[(1 << 29) + 5])
    # ---- two conditions violated at once: which one is reported
    add("categorical", "n_categories = 1 with n_factors = -1", n_categories=1, n_factors=-1)
    add("factor", "n_factors above the limit with n_obs = 0", n_factors=9, n_obs=0)
    add("factor", "n_coef = 0 with n_obs above AHMC_GLM_MAX_OBS", n_coef=0, n_obs=big)
    add("factor", "a level index out of range with a D that does not match", n_coef=3, poke=[("levels", 2, 3)])
    add("hier", "n_groups = -1 with a D that does not match", n_groups=-1, n_coef=4)
    add("aux", "n_groups above both group limits", lo=list(range(33)), hi=list(range(1, 34)), centered=[0] * 33, hyper_scale=[1.0] * 33)
    add("hier", "family 5 with a D that does not match", family=5, n_coef=4)
    add("hier", "family 6 with a D that does not match", family=6, n_coef=4)
    add("plain", "a dispersion family with n_obs = 0", family=3, n_obs=0)
    add("plain", "an unknown family with X NULL", family=9, X=None)
    for b in bases:
        if b in ("plain", "hier", "factor"):
            add(b, "scale = 0 with a NaN in X", scale=0.0, poke=[("X", 7, "nan")])
        add(b, "a NaN in X with y outside the domain", poke=[("X", 7, "nan"), ("y", 5, -7.0)])
        add(b, "a non-finite offset at row i with a bad y at rows i and i - 1", poke=[("offset", 6, "inf"), ("y", 6, -7.0), ("y", 5, -7.0)])
        if b != "plain":
            add(b, "a negative prior_prec with a non-zero one on a group member", poke=[("prior_prec", bases[b]["hi"][-1] - 1, 0.5), ("prior_prec", bases[b]["hi"][-1] - 2, -0.5)])
    add("hier", "the same group table overlapping and out of bounds", lo=[0, 0], hi=[2, 4])
    return {"bases": bases, "cases": cases}


SET_TARGET = {
    "plain": ("ahmc_set_target_glm", lambda m, p: (m["family"], m["n_obs"], *p["data"], m["scale"])),
    "hier": ("ahmc_hglm_set_target", lambda m, p: (m["family"], m["n_obs"], m["n_coef"], *p["data"], m["scale"], *p["groups"])),
    "aux": ("ahmc_glm_aux_set_target", lambda m, p: (m["family"], m["n_obs"], m["n_coef"], *p["data"], *p["groups"], m["aux_loc"], m["aux_scale"])),
    "factor": ("ahmc_glm_factor_set_target", lambda m, p: (m["family"], m["n_obs"], m["n_coef"], *p["data"], m["scale"], *p["groups"], *p["factors"], m["has_aux"],
                                                            m["aux_loc"], m["aux_scale"])),
    "ordinal": ("ahmc_glm_ordinal_set_target", lambda m, p: (m["n_obs"], m["n_coef"], *p["data"], *p["groups"], *p["factors"], m["n_categories"], p["cut_prior"])),
    "categorical": ("ahmc_glm_categorical_set_target", lambda m, p: (m["n_obs"], m["n_coef"], *p["data"], *p["groups"], *p["factors"], m["n_categories"])),
}


def pointers(m):
    """the ctypes arguments of materialise()'s arrays (which stay alive in m)"""
    def ptr(a, ct=C.c_void_p):
        return None if a is None else a.ctypes.data_as(ct)

    i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    return {"data": (ptr(m["X"]), ptr(m["y"]), ptr(m["offset"]), ptr(m["prior_prec"])),
            "groups": (m["n_groups"], ptr(m["lo"], i32), ptr(m["hi"], i32), ptr(m["centered"], i32), ptr(m["hyper_scale"], f64)),
            "factors": (m["n_factors"], ptr(m["n_levels"], i32), ptr(m["levels"], i32)), "cut_prior": ptr(m["cut_prior"], f64)}


def child_refusals():
    import ahmc_amd as A

    lib = A.load_hip_library()
    table = refusal_table()
    res = {}

    def answer(e, fn, *args):
        rc = getattr(lib.dll, fn)(e._ctx, *args)
        msg = lib.dll.ahmc_last_error(e._ctx)
        return [int(rc), (msg.decode("utf-8", "replace") if msg else "") if rc else ""]

    for dt, dtype in DTYPES.items():
        engines = {}
        for case in table["cases"]:
            m = materialise(table, case, dtype)
            key = (m["D"], m["N"])
            if key not in engines:
                engines[key] = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric(key), A.IsoGaussian(key[0])), key[1], dtype=dtype, rng=A.PhiloxRNG(1), lib=lib)
            fn, args = SET_TARGET[ENTRIES[m["entry"]]]
            res[f"{dt}/{case['name']}"] = answer(engines[key], fn, *args(m, pointers(m)))
        for e in engines.values():
            e.close()
        # ---- the draw entry points: nothing bound, each kind bound, and their arguments
        th = np.zeros((16, 8), dtype=dtype, order="F")
        out = np.zeros(4096, dtype=np.float64)
        tp, op = th.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
        calls = {"hglm_coefficients": lambda e, t, n, o: answer(e, "ahmc_hglm_coefficients", t, n, o, o),
                 "glm_dispersion": lambda e, t, n, o: answer(e, "ahmc_glm_dispersion", t, n, o),
                 "glm_cutpoints": lambda e, t, n, o: answer(e, "ahmc_glm_cutpoints", t, n, o),
                 "glm_class_probs": lambda e, t, n, o: answer(e, "ahmc_glm_class_probs", t, n, o),
                 "glm_loglik": lambda e, t, n, o: answer(e, "ahmc_glm_loglik", t, n, o),
                 "glm_loo": lambda e, t, n, o: answer(e, "ahmc_glm_loo", t, n, C.cast(o, C.POINTER(C.c_double)), None)}
        for bound in (None, *table["bases"]):
            b = table["bases"][bound or "plain"]
            e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((b["D"], b["N"])), A.IsoGaussian(b["D"])), b["N"], dtype=dtype, rng=A.PhiloxRNG(1), lib=lib)
            if bound:
                m = materialise(table, {"base": bound}, dtype)
                fn, args = SET_TARGET[bound]
                assert answer(e, fn, *args(m, pointers(m)))[0] == 0, bound
            for who, call in calls.items():
                for what, (t, ncol, o) in {"n_cols = -1": (tp, -1, op), "theta NULL": (None, 2, op), "out NULL": (tp, 2, None), "n_cols = 2^31": (tp, 1 << 31, op),
                                           "n_cols = 0": (tp, 0, op), "n_cols = 0, all NULL": (None, 0, None)}.items():
                    res[f"{dt}/draws/{bound}/{who}/{what}"] = call(e, t, ncol, o)
            e.close()
    print("RESULT " + json.dumps(res), flush=True)


def child_launches():
    import ahmc_amd as A

    lib = A.load_hip_library()
    for kind in KINDS:
        t = target(kind, 1100)
        rs = np.random.default_rng(3)
        e = engine(t, N_ID, np.float64, lib)
        e.set_position(0.2 * rs.normal(size=(t.D, N_ID)))
        e.glm_pointwise()
        draw_calls(e, t, 0.3 * rs.normal(size=(t.D, 2 * N_ID + 3)), {}, "")
        e.close()


def child_speed(windows):
    import ahmc_amd as A

    lib = A.load_hip_library()
    res = {}
    # the NUTS loop of glm_bench.py nuts
    n_obs, D, N = 8192, 256, 8192
    rs = np.random.default_rng(0)
    X = rs.normal(size=(n_obs, D)) / np.sqrt(D)
    y = (rs.random(n_obs) < 1 / (1 + np.exp(-(X @ rs.normal(size=D))))).astype(np.float64)
    kern = A.HMCKernel(A.Trajectory(A.MultinomialTS, A.Leapfrog(0.02), A.GeneralisedNoUTurn(max_depth=3)))
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((D, N)), A.GLMTarget(X, y, prior_prec=np.ones(D))), N, dtype=np.float64, rng=2, lib=lib)
    e.set_integrator(A.Leapfrog(0.02))
    e.set_position(0.1 * np.random.default_rng(1).normal(size=(D, N)))
    e.run(kern, 1)
    e.sync()
    res["nuts_8192x256x8192_f64_s_per_2_transitions"] = []
    for w in range(windows):
        t0 = time.perf_counter()
        e.run(kern, 2 * w + 3, i_first=2 * w + 2)
        e.sync()
        res["nuts_8192x256x8192_f64_s_per_2_transitions"].append(time.perf_counter() - t0)
    e.close()
    # 16 chains at (8192, 256): launch-bound evaluations (glm_bench.py tail)
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((D, 16)), A.GLMTarget(X, y, prior_prec=np.ones(D))), 16, dtype=np.float64, rng=2, lib=lib)
    e.set_integrator(A.Leapfrog(0.01))
    e.set_position(0.1 * np.random.default_rng(1).normal(size=(D, 16)))
    e.step(20)
    e.sync()
    res["tail_16_chains_8192x256_f64_us_per_evaluation"] = []
    for w in range(windows):
        t0 = time.perf_counter()
        e.step(200)
        e.sync()
        res["tail_16_chains_8192x256_f64_us_per_evaluation"].append((time.perf_counter() - t0) / 200 * 1e6)
    e.close()
    # the categorical model of glm_categorical_bench.py: K gradient launches per evaluation
    n_obs, Px, Cn, N = 4096, 32, 4, 16384
    X = rs.normal(size=(n_obs, Px)) / np.sqrt(Px)
    t = A.GLMTarget(X, rs.integers(0, Cn, size=n_obs), family="categorical_logit", n_categories=Cn, prior_prec=np.ones(Px * (Cn - 1)))
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((t.D, N)), t), N, dtype=np.float64, rng=2, lib=lib)
    e.set_integrator(A.Leapfrog(0.01))
    e.set_position(0.1 * np.random.default_rng(1).normal(size=(t.D, N)))
    e.step(3)
    e.sync()
    res["categorical_4096x32x4_N16384_f64_us_per_evaluation"] = []
    for w in range(windows):
        t0 = time.perf_counter()
        e.step(10)
        e.sync()
        res["categorical_4096x32x4_N16384_f64_us_per_evaluation"].append((time.perf_counter() - t0) / 10 * 1e6)
    e.close()
    print("RESULT " + json.dumps(res), flush=True)


# ---- the parent ----
def run_child(argv, lib, limit, prof=False):
    """one child under its own time limit with AHMC_HIP_LIB = lib; rocprofv3's calls per kernel if `prof`.  Raises on a failure: the
    caller stops there."""
    tmp = tempfile.mkdtemp(prefix="glm_identity_")
    try:
        cmd = [sys.executable, os.path.abspath(__file__), *argv]
        if prof:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "glm", "--output-format", "csv", "--", *cmd]
        res = subprocess.run(["timeout", "-k", "10", str(limit), *cmd], capture_output=True, text=True, env=dict(os.environ, AHMC_HIP_LIB=os.path.abspath(lib)))
        if res.returncode != 0:
            raise RuntimeError(f"child {argv} on {lib} ended with status {res.returncode}: nothing more is started\n{res.stdout[-2000:]}\n{res.stderr[-3000:]}")
        if not prof:
            return [json.loads(l[7:]) for l in res.stdout.splitlines() if l.startswith("RESULT ")][0]
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError(f"no kernel_stats.csv under {tmp}")
        return {row["Name"]: int(row["Calls"]) for row in csv.DictReader(open(files[0]))}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def differing(a, b):
    return sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))


def cmd_identity(args):
    rows = {}
    for dt in DTYPES:
        base, new = (run_child(["child-identity", "--dtype", dt], lib, 500) for lib in (args.base, args.new))
        diff = [f"{case}: {k}" for case in sorted(set(base) | set(new)) for k in differing(base.get(case, {}), new.get(case, {}))]
        rows[dt] = dict(cases=len(base), arrays_hashed=sum(len(v) for v in base.values()), differing=diff)
        print(json.dumps({dt: {k: v for k, v in rows[dt].items() if k != "differing"}, "differing": diff[:20]}), flush=True)
    merge(args.out, "identity", {"rows": rows, "method": "sha256 over dtype, shape and bytes of every array, one child per library and element type"})
    if any(r["differing"] for r in rows.values()):
        raise SystemExit("identity: the two libraries differ")


def cmd_refusals(args):
    base, new = (run_child(["child-refusals"], lib, 400) for lib in (args.base, args.new))
    diff = differing(base, new)
    for k in diff[:30]:
        print(k, base.get(k), new.get(k), flush=True)
    print(json.dumps(dict(refusals_compared=len(base), refused=sum(1 for v in base.values() if v[0]), differing=len(diff))), flush=True)
    merge(args.out, "refusals", dict(compared=len(base), refused=sum(1 for v in base.values() if v[0]), differing=diff))
    if args.write_golden:
        table = refusal_table()
        for c in table["cases"]:
            c["expect"] = {dt: base[f"{dt}/{c['name']}"] for dt in DTYPES}
        write_golden(table)
    if diff:
        raise SystemExit("refusals: the two libraries differ")


def cmd_launches(args):
    base, new = (run_child(["child-launches"], lib, 400, prof=True) for lib in (args.base, args.new))
    diff = differing(base, new)
    for k in diff:
        print(k, base.get(k), new.get(k), flush=True)
    print(json.dumps(dict(kernel_names=len(base), launches=sum(base.values()), differing=len(diff))), flush=True)
    merge(args.out, "launches", dict(kernel_names=len(base), launches=sum(base.values()), differing=diff, calls_per_kernel=base))
    if diff:
        raise SystemExit("launches: the two libraries differ")


def cmd_speed(args):
    win = {"base": {}, "new": {}}
    for _ in range(args.rounds):
        for which, lib in (("base", args.base), ("new", args.new)):
            for k, v in run_child(["child-speed", "--windows", "2"], lib, 400).items():
                win[which].setdefault(k, []).extend(v)
    rows = {}
    for k in win["base"]:
        b, n = win["base"][k], win["new"][k]
        rows[k] = dict(base_median=statistics.median(b), base_min=min(b), base_max=max(b), new_median=statistics.median(n), new_min=min(n), new_max=max(n),
                       base_windows=b, new_windows=n, new_median_no_worse_than_base_worst=statistics.median(n) <= max(b))
        print(json.dumps({k: {q: v for q, v in rows[k].items() if not q.endswith("windows")}}), flush=True)
    merge(args.out, "speed", {"rows": rows, "method": f"host clock around work that ends in a synchronise; {args.rounds} children per library alternating, 2 windows each; "
                                                      "lower is better; the margin is the base library's own spread in the same session"})
    if not all(r["new_median_no_worse_than_base_worst"] for r in rows.values()):
        raise SystemExit("speed: a median of the new library is worse than the base library's worst window")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("identity", "refusals", "launches", "speed", "child-identity", "child-refusals", "child-launches", "child-speed"))
    ap.add_argument("--base")
    ap.add_argument("--new")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--write-golden", action="store_true")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--windows", type=int, default=2)
    args = ap.parse_args()
    if args.what == "child-identity":
        child_identity(args.dtype)
    elif args.what == "child-refusals":
        child_refusals()
    elif args.what == "child-launches":
        child_launches()
    elif args.what == "child-speed":
        child_speed(args.windows)
    else:
        {"identity": cmd_identity, "refusals": cmd_refusals, "launches": cmd_launches, "speed": cmd_speed}[args.what](args)


if __name__ == "__main__":
    main()
