"""Low-rank mass-matrix adaptation of RankUpdateEuclideanMetric (include/ahmc_lowrank_adapt.h, csrc/ahmc_lowrank_adapt.hpp,
csrc/ahmc_lowrank_adapt_host.hpp, advancedhmc.jl_amd/rank_update.py lowrank_*): M⁻¹ = Diagonal(A) + B·Dm·Bᵀ fitted to the draws
of all chains.  The reference has no adaptor for this metric, so the references here are exact ones:

CPU: the mirror's push against the brute-force sums in np.longdouble inside a derived rounding bound; the fit's invariants and its
     convergence on exact population statistics; its quality (the condition number of the preconditioned covariance) against an exact
     top-k eigendecomposition of the same draws; header ↔ bindings ↔ exports ↔ Julia; the kernels' metadata.
GPU: the push kernels against the same brute force and bound, and bit-reproducible; the engine's fit against the mirror's inside the
     problem's own conditioning; ahmc_sample == transition + adapt, checkpoints, the adapted context == a fresh one with its metric;
     usefulness on a spiked Gaussian; refusals.

Measured ratios go to lowrank_adapt_margins.json in $AHMC_TEST_OUT (default: test_out/ in the repository root, ignored by git); a copy
of the MI355X run is profiles/lowrank_adapt_margins.json.

The rounding bound of the push (`push_bounds`).  Z[d, j] = Σ_c Σ_e x_c[d, c]·x_c[e, c]·W[e, j] over the n draws seen so far, x_c the
draw minus the mean.  However it is bracketed — T = X_cᵀW first (dot products of length D), then X_c·T (length N per batch), the batch
means (length N), Chan's merges of the batches (a constant number of operations each), the slices' partial sums — every one of the
D·n products of the double sum passes through at most D + n + c roundings of relative size u = 2⁻⁵³ (a product, at most D − 1
additions inside its projection, at most n − 1 additions across the draws, and c for the centring, the merge and f), so by the
standard dot-product bound (Higham, Accuracy and Stability, §3.1) |Ẑ − Z| ≤ γ_m·(|X_c|·(|X_c|ᵀ·|W|)) elementwise with m = D + n + c,
γ_m = m·u/(1 − m·u).  c = 16 is generous: centring 2, the merge 4, f and n/(n+N) 3 each, conversions 0 (float32 → double is exact).
The error of a computed batch mean moves Z only at second order (Σ_c x_c = 0).  Likewise |m̂2 − m2| ≤ γ_m·Σ_c x_c² and
|μ̂ − μ| ≤ γ_m·mean|x|.  n is an integer and exact.  The float32 engine converts X to double before any arithmetic, so the same
bound holds with the float32 inputs taken as exact.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ahmc_amd as A
from ahmc_amd import _capi as capi
from ahmc_amd import rank_update as RU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
U64 = LD(2) ** -53
MARGINS = {}


def _record(key, **vals):
    MARGINS.setdefault(key, {}).update({k: (float(v) if np.ndim(v) == 0 else [float(x) for x in v]) for k, v in vals.items()})
    out = os.environ.get("AHMC_TEST_OUT") or os.path.join(ROOT, "test_out")
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "lowrank_adapt_margins.json"), "w") as f:
            json.dump({"cases": dict(sorted(MARGINS.items()))}, f, indent=1)
    except OSError:
        pass


def gamma(m):
    return LD(m) * U64 / (1 - LD(m) * U64)


def push_bounds(batches, W):
    """exact (Z, m2, μ, n) of the concatenated draws in np.longdouble and the elementwise bounds of the module docstring"""
    X = np.concatenate([np.asarray(b, dtype=LD) for b in batches], axis=1)
    D, n = X.shape
    Wl = np.asarray(W, dtype=LD)
    mu = X.sum(axis=1) / n
    Xc = X - mu[:, None]
    Z = Xc @ (Xc.T @ Wl)
    m2 = np.sum(Xc * Xc, axis=1)
    g = gamma(D + n + 16)
    aXc = np.abs(Xc)
    return {"Z": Z, "m2": m2, "mu": mu, "n": n}, {"Z": g * (aXc @ (aXc.T @ np.abs(Wl))), "m2": g * m2, "mu": g * np.abs(X).sum(axis=1) / n}


def check_push(key, got, batches, W):
    want, bound = push_bounds(batches, W)
    assert int(got["n"]) == want["n"]
    ratios = {}
    for name in ("Z", "m2", "mu"):
        err = np.abs(np.asarray(got[name], dtype=LD) - want[name])
        assert np.isfinite(err).all(), (key, name)
        frac = np.where(err == 0, LD(0), err / np.where(bound[name] > 0, bound[name], LD("1e-4900")))
        ratios[name] = float(frac.max())
    _record(key, **{f"{k}_error_over_bound": v for k, v in ratios.items()})
    print(key, ratios)
    for name, r in ratios.items():
        assert r <= 1.0, f"{key}: {name} misses its bound by {r:.3g}×"
    return ratios


def batches_for(D, N, rs, dtype=np.float64, n_batches=3):
    """caller-supplied positions with mean offset 3 and unequal scales"""
    scale = np.exp(0.5 * rs.normal(size=(D, 1)))
    return [np.asfortranarray((3.0 + scale * rs.normal(size=(D, N))).astype(dtype)) for _ in range(n_batches)]


def spiked_cov(D, k, lam_lo, lam_hi, rs, a=1.0, sigma=1.0):
    """C = S(a·I + U·Γ·Uᵀ)S, Γ = linspace(lam_lo, lam_hi, k), S log-normal"""
    U, _ = np.linalg.qr(rs.normal(size=(D, k)))
    G = np.linspace(lam_lo, lam_hi, k)
    S = np.exp(sigma * rs.normal(size=D))
    return S[:, None] * (a * np.eye(D) + (U * G) @ U.T) * S[None, :]


def precond_cond(C, Minv):
    """cond(L⁻¹·C·L⁻ᵀ), L·Lᵀ = M⁻¹: 1 for the perfect preconditioner"""
    L = np.linalg.cholesky(Minv)
    Li = np.linalg.inv(L)
    w = np.linalg.eigvalsh(Li @ C @ Li.T)
    return w[-1] / w[0]


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the mirror
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N,k,p", [(1, 1, 1, 0), (7, 3, 2, 8), (48, 64, 3, 8), (130, 257, 32, 8), (513, 40, 5, 4)])
def test_mirror_push_against_brute_force(D, N, k, p):
    """lowrank_push over 3 batches with mean offset 3 == Σ(x − μ)(x − μ)ᵀW, Σ(x − μ)², μ and n of the concatenated draws, computed in
    np.longdouble, inside the bound derived in the module docstring"""
    rs = np.random.default_rng(100 + D)
    st = RU.lowrank_init(np.exp(0.3 * rs.normal(size=D)), k, p, seed=D)
    assert st.ell == min(D, k + p) and st.Omega.shape == (D, st.ell)
    W = st.W.copy()
    batches = batches_for(D, N, rs)
    for b in batches:
        RU.lowrank_push(st, b)
    check_push(f"mirror_push D={D} N={N} ell={st.ell}", {"Z": st.Z, "m2": st.m2, "mu": st.mu, "n": st.n}, batches, W)


def exact_window(st, C, n):
    """the window state n draws with exactly the population covariance C (and mean 0) would leave"""
    st.n = n
    st.mu = np.zeros(C.shape[0])
    st.m2 = (n - 1) * np.diag(C).copy()
    st.Z = (n - 1) * (C @ st.W)


@pytest.mark.parametrize("D,k", [(1, 1), (7, 2), (12, 12), (48, 3)])
def test_fit_properties(D, k):
    """A > 0, Dm diagonal and ⪰ 0, the metric constructs, diag(M⁻¹) = sh·var + 10⁻³·5/(n+5)·s₀² wherever the 10⁻³·c floor is inactive;
    and on exact population statistics of C = S(I + UΓUᵀ)S with s₀ = the true standard deviations the warm-started windows converge.
    The limit is not sh·C itself but the model's best: diag + the top-k eigenpairs of the correlation matrix (S(I + UΓUᵀ)S is diagonal
    plus rank k in correlation coordinates too, but its diagonal part is not flat there, so the eigenvectors are not U's).  The
    distance to sh·C therefore levels out at that model's own (measured at (48, 3): 0.194, 0.0220, 0.0221 — the limit 0.0221 is
    approached from below), and what is asserted to decrease from window to window is the distance to the limit, computed from
    numpy's eigendecomposition (measured: 0.18, 4.3·10⁻³, 3.4·10⁻⁴); the distance to sh·C must be smaller after windows 2 and 3 than
    after window 1.  Both are recorded.  Where ℓ = D Nyström is exact and every window is at the limit to rounding; with k = D all
    that is left of the distance to sh·C is the 10⁻³ floor of the diagonal and the regulariser."""
    rs = np.random.default_rng(200 + D)
    C = spiked_cov(D, min(k, 3), 10.0, 40.0, rs, sigma=0.7)
    Lc = np.linalg.cholesky(C)
    s0 = np.exp(0.3 * rs.normal(size=D))
    st = RU.lowrank_init(s0, k, seed=3)
    assert RU.lowrank_fit(st) is None  # (an empty window is not fitted)
    N = 40
    for _ in range(3):
        RU.lowrank_push(st, 3.0 + Lc @ rs.normal(size=(D, N)))
    n = st.n
    A_, B_, Dm_ = RU.lowrank_fit(st)
    assert np.all(np.isfinite(A_)) and np.all(A_ > 0)
    assert B_.shape == (D, k) and Dm_.shape == (k, k)
    assert np.all(Dm_ == np.diag(np.diag(Dm_))) and np.all(np.diag(Dm_) >= 0)
    m = A.RankUpdateEuclideanMetric(A_, B_, Dm_)
    assert m.rank == k
    np.linalg.cholesky(RU.dense(A_, B_, Dm_))  # positive definite
    var, sh = st.m2 / (n - 1), n / (n + 5.0)
    c = var / s0 ** 2
    dm = np.diag(Dm_) / sh
    V = B_ / s0[:, None]
    free = c - (V * V) @ dm > 1e-3 * c * (1 + 1e-9)
    assert free.any() or D == k
    want = sh * var + 1e-3 * (5.0 / (n + 5.0)) * s0 ** 2
    np.testing.assert_allclose(RU.diag_inv_metric(A_, B_, Dm_)[free], want[free], rtol=1e-12)
    # exact population statistics, warm-started windows
    sd = np.sqrt(np.diag(C))
    st = RU.lowrank_init(sd, k, seed=4)
    n = 1000
    sh = n / (n + 5.0)
    limit = exact_topk_model(C, k, sh, 1e-3 * 5.0 / (n + 5.0))
    dist, to_limit = [], []
    for w in range(3):
        exact_window(st, C, n)
        M = RU.dense(*RU.lowrank_fit(st))
        dist.append(np.linalg.norm(M - sh * C) / np.linalg.norm(C))
        to_limit.append(np.linalg.norm(M - limit) / np.linalg.norm(C))
        RU.lowrank_restart(st)
        np.testing.assert_allclose(st.s0, sd, rtol=1e-12)
        assert st.n == 0 and not st.Z.any() and not st.m2.any() and st.n_fits == w + 1
    _record(f"fit_exact_statistics D={D} k={k}", distance_to_shC_after_windows=dist, distance_to_limit_after_windows=to_limit)
    print(D, k, dist, to_limit)
    if st.ell < D:
        assert to_limit[0] > to_limit[1] > to_limit[2], to_limit
        assert dist[1] < dist[0] and dist[2] < dist[0], dist
    else:
        assert max(to_limit) < 1e-10, to_limit
    if D == k:  # the low-rank part takes everything: what is left is the 10⁻³·c floor of d and the regulariser
        assert dist[0] <= 1e-3 + 1e-3 * 5.0 / (n + 5.0), dist


def exact_topk_model(C, k, sh, reg):
    """what the estimator converges to on exact statistics of C with s₀ = its standard deviations: the same diagonal + rank-k model
    from numpy's eigendecomposition of the correlation matrix (not from the code under test)"""
    D = C.shape[0]
    sd = np.sqrt(np.diag(C))
    w, V = np.linalg.eigh(C / np.outer(sd, sd))
    w, V = w[::-1][:k], V[:, ::-1][:, :k]
    lres = max((D - w.sum()) / (D - k), 0.0) if D > k else 0.0
    dm = np.maximum(w - lres, 0.0)
    d = np.maximum(1.0 - (V * V) @ dm, 1e-3)
    B = sd[:, None] * V
    return np.diag(sd ** 2 * (sh * d + reg)) + (B * (sh * dm)) @ B.T


QUALITY = [(48, 3, 256, 1.0, 100.0), (130, 5, 512, 1.0, 50.0), (7, 2, 64, 1.0, 30.0)]


def exact_topk_fit(X, k):
    """the same diagonal + low-rank model from an exact eigendecomposition of the draws' correlation matrix (numpy only)"""
    D, n = X.shape
    Ce = np.cov(X)
    sd = np.sqrt(np.diag(Ce))
    w, V = np.linalg.eigh(Ce / np.outer(sd, sd))
    w, V = w[::-1][:k], V[:, ::-1][:, :k]
    lres = max((D - w.sum()) / (D - k), 0.0) if D > k else 0.0
    dm = np.maximum(w - lres, 0.0)
    d = np.maximum(1.0 - (V * V) @ dm, 1e-3)
    sh = n / (n + 5.0)
    B = sd[:, None] * V
    return np.diag(sd ** 2 * (sh * d + 1e-3 * 5.0 / (n + 5.0))) + (B * (sh * dm)) @ B.T


@pytest.mark.parametrize("D,k,N,a,lam_max", QUALITY)
def test_fit_quality_against_exact_topk(D, k, N, a, lam_max):
    """Draws from N(3, S(aI + UΓUᵀ)S), Γ = linspace(λmax/4, λmax, k), log-normal S; three windows of 25 pushes of N draws each (25
    iterations: Stan's smallest window).  After the third window cond(L⁻¹CL⁻ᵀ) is within 1.25× of the exact top-k fit of the third
    window's draws (numpy's eigendecomposition of their correlation matrix) and at most 1/10 of diag(C)'s."""
    rs = np.random.default_rng(300 + D)
    C = spiked_cov(D, k, lam_max / 4, lam_max, rs, a=a)
    Lc = np.linalg.cholesky(C)
    st = RU.lowrank_init(np.ones(D), k, seed=D)
    conds = []
    for _ in range(3):
        draws = [3.0 + Lc @ rs.normal(size=(D, N)) for _ in range(25)]
        for X in draws:
            RU.lowrank_push(st, X)
        conds.append(precond_cond(C, RU.dense(*RU.lowrank_fit(st))))
        RU.lowrank_restart(st)
    exact = precond_cond(C, exact_topk_fit(np.concatenate(draws, axis=1), k))
    diag = precond_cond(C, np.diag(np.diag(C)))
    _record(f"fit_quality D={D} k={k} N={N}", cond_after_windows=conds, cond_exact_topk=exact, cond_diag=diag)
    print(D, k, conds, exact, diag)
    assert conds[2] <= 1.25 * exact, (conds, exact)
    assert conds[2] <= diag / 10, (conds, diag)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: header, bindings, Julia, the shipped kernels
# ---------------------------------------------------------------------------------------------------------------------
def header_prototypes():
    src = open(os.path.join(ROOT, "include", "ahmc_lowrank_adapt.h"), encoding="utf-8").read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(int32_t)\s+(ahmc_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        params = " ".join(m.group(3).split())
        protos[m.group(2)] = [] if params in ("", "void") else [p.strip() for p in params.split(",")]
    return protos, src


def test_header_and_bindings_agree():
    protos, src = header_prototypes()
    assert set(protos) == set(capi.LR_SIGNATURES)
    C = capi.C
    ct = {"int64_t": C.c_int64, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "double": C.c_double,
          "ahmc_lowrank_state*": C.POINTER(capi.LowRankState)}
    for name, params in protos.items():
        res, args = capi.LR_SIGNATURES[name]
        assert res is C.c_int32 and len(args) == len(params), name
        for p, a in zip(params, args):
            typ = p.rsplit(" ", 1)[0].replace("const ", "").replace(" ", "")
            if typ in ("void*", "ahmc_ctx*", "double*"):
                assert a is C.c_void_p, (name, p)
            else:
                assert a is ct[typ], (name, p)
    assert re.search(r"#define AHMC_LOWRANK_ADAPT_VERSION (\d+)", src).group(1) == str(capi.AHMC_LOWRANK_ADAPT_VERSION)
    assert re.search(r"#define AHMC_LOWRANK_MAX_ELL (\d+)", src).group(1) == str(capi.AHMC_LOWRANK_MAX_ELL) == str(RU.LOWRANK_MAX_ELL)
    assert RU.LOWRANK_MAX_K == capi.AHMC_RANK_UPDATE_MAX_K
    fields = re.search(r"typedef struct ahmc_lowrank_state \{(.*?)\}", src, flags=re.S).group(1)
    got = [(t, n) for t, n in re.findall(r"(\w+)\s+(\w+);", fields)]
    want = [({C.c_int64: "int64_t", C.c_uint64: "uint64_t"}[t], n) for n, t in capi.LowRankState._fields_]
    assert got == want
    for other in ("ahmc_hip.h", "ahmc_rank_update.h"):  # (kept out of both, and out of AHMC_ABI_VERSION)
        assert "lowrank" not in open(os.path.join(ROOT, "include", other), encoding="utf-8").read()


def test_julia_ccalls_match_the_header():
    protos, _ = header_prototypes()
    src = open(os.path.join(ROOT, "julia", "AdvancedHMCMI355XLowRankAdapt.jl"), encoding="utf-8").read()
    src = re.sub(r"#[^\n]*", "", src)
    seen = set()
    jl = {"int64_t": "Int64", "int32_t": "Cint", "uint64_t": "UInt64", "double": "Cdouble"}
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
        seen.add(name)
        assert m.group(2) == "Cint" and len(types) == len(protos[name]), (name, types)
        for t, p in zip(types, protos[name]):
            if "*" in p:
                assert t.startswith(("Ptr{", "Ref{")), (name, t, p)
            else:
                assert jl[p.split()[0]] == t, (name, t, p)
    assert seen == set(protos)
    fields = re.search(r"mutable struct LowRankHeader(.*?)\nend", src, flags=re.S).group(1)
    assert re.findall(r"(\w+)::(\w+)", fields) == [(n, {capi.C.c_int64: "Int64", capi.C.c_uint64: "UInt64"}[t]) for n, t in capi.LowRankState._fields_]
    ext = open(os.path.join(ROOT, "julia", "AdvancedHMCMI355XExt.jl"), encoding="utf-8").read()
    assert 'include("AdvancedHMCMI355XLowRankAdapt.jl")' in ext and "ahmc_lowrank_adaptor_init" not in ext


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="needs llvm-objdump")
def test_library_exports_and_kernels_without_scratch():
    import ctypes

    from ahmc_amd import build as B

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_meta
    finally:
        sys.path.pop(0)
    assert os.path.exists(B.OUT), "build() first"
    dll = ctypes.CDLL(B.OUT)
    for name in capi.LR_SIGNATURES:
        getattr(dll, name)
    meta = kernel_meta.kernel_meta(B.OUT)
    names = subprocess.run(["c++filt"], input="\n".join(k["name"] for k in meta), capture_output=True, text=True, check=True).stdout.splitlines()
    want = [f"k_lr_{w}<{t}, {lb}>" for w in ("project", "accumulate") for t in ("float", "double") for lb in (8, 16, 40)]
    want += [f"k_lr_merge<{lb}>" for lb in (8, 16, 40)]
    found = {}
    for k, dn in zip(meta, names):
        for w in want:
            if dn.startswith(f"void ahmc::{w}("):
                found[w] = k
    assert sorted(found) == sorted(want), sorted(found)
    for w, k in found.items():  # (SGPR spills land in VGPR lanes, not in scratch)
        assert k["private_segment_fixed_size"] == 0, (w, k)
        assert k.get("vgpr_spill_count", 0) == 0, (w, k)


def test_cpu_checker_has_no_lowrank_adaptor(oracle):
    assert oracle.has_lowrank_adapt is False
    D = 4
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((D, 3)), A.IsoGaussian(D)), 3, lib=oracle)
    with pytest.raises(A.UnsupportedError, match="ahmc_lowrank_adapt.h"):
        e.adaptor_init(A.LowRankVar(D, 2))
    assert e.get_state()["lowrank"] is None
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def stan_lowrank(D, k, p=8, seed=0, eps=0.1, ib=0, tb=0, ws=100):
    return A.StanHMCAdaptor(A.LowRankVar(D, k, p, seed), A.StepSizeAdaptor(0.8, A.Leapfrog(eps)), init_buffer=ib, term_buffer=tb, window_size=ws)


# (D, N, k, oversample): ℓ = min(D, k + oversample) = 1, 7, 8 | 9, 16 | 17, 40 — both sides of each accumulator bucket —, N not a
# multiple of the slices or of the columns per workgroup, D below / across / far beyond one row tile, 5000 = a wide context
PUSH_CASES = [(1, 1, 1, 0), (1, 64, 1, 8), (7, 3, 1, 8), (7, 257, 7, 8), (130, 64, 1, 8), (130, 64, 4, 4), (130, 64, 8, 8), (130, 64, 9, 8),
              (130, 257, 32, 8), (130, 1000, 1, 0), (513, 3, 32, 8), (513, 257, 5, 4), (513, 1000, 8, 8), (5000, 1, 1, 8), (5000, 64, 32, 8),
              (5000, 257, 1, 8), (5000, 1000, 1, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("D,N,k,p", PUSH_CASES)
def test_push_kernels_against_brute_force(hip, D, N, k, p, dtype):
    """three ahmc_adapt pushes of caller-supplied θ (mean offset 3) inside one Stan window: Z, m2, μ, n from ahmc_lowrank_get_state
    against the np.longdouble brute force, inside the bound of the module docstring; a second identical context gives the same bits"""
    rs = np.random.default_rng(400 + D + N)
    minv = np.exp(0.6 * rs.normal(size=D)).astype(dtype)
    batches = batches_for(D, N, rs, dtype)
    states = []
    for rep in range(2):
        e = A.Engine(A.Hamiltonian(A.DiagEuclideanMetric(minv), A.IsoGaussian(D)), N, dtype=dtype, rng=A.PhiloxRNG(5), lib=hip)
        e.adaptor_init(stan_lowrank(D, k, p, seed=77))
        s0 = e.lowrank_state()
        assert (s0["k"], s0["ell"], s0["seed"], s0["n"], s0["n_fits"]) == (k, min(D, k + p), 77, 0, 0)
        np.testing.assert_array_equal(s0["s0"], np.sqrt(minv.astype(np.float64)))
        assert not s0["Z"].any() and not s0["m2"].any() and not s0["mu"].any()
        for i, b in enumerate(batches, 1):
            e.adapt(i, 1000, theta=b, alpha=np.ones(N))
        st = e.lowrank_state()
        np.testing.assert_array_equal(st["Omega"], s0["Omega"])
        ast = capi.AdaptorState()
        e._call("ahmc_get_adaptor_state", capi.C.byref(ast), None, None)
        assert ast.n_welford == 0 and ast.kind == capi.ADAPT_STAN and ast.stan_i == 3
        states.append(st)
        e.close()
    Om = states[0]["Omega"]
    assert np.isfinite(Om).all()
    if Om.size >= 5000:  # the normals of the adaptor's stream: mean 0 ± 5/√n, variance 1 ± 5·√(2/n)
        assert abs(Om.mean()) < 5 / np.sqrt(Om.size) and abs(Om.var() - 1) < 5 * np.sqrt(2 / Om.size)
        assert abs(np.corrcoef(Om[:-1, 0], Om[1:, 0])[0, 1]) < 5 / np.sqrt(D)
    W = Om / states[0]["s0"][:, None]
    check_push(f"gpu_push {np.dtype(dtype).name} D={D} N={N} ell={states[0]['ell']}", states[0], batches, W)
    for name in ("Z", "m2", "mu"):
        np.testing.assert_array_equal(states[0][name], states[1][name])


def sub_dense(Av, B, Dm, idx):
    return np.diag(np.asarray(Av, dtype=np.float64)[idx]) + np.asarray(B, dtype=np.float64)[idx] @ np.asarray(Dm, dtype=np.float64) @ np.asarray(B, dtype=np.float64)[idx].T


def mirror_state(s):
    st = RU.LowRankState(int(s["k"]), int(s["ell"]), int(s["seed"]), int(s["n"]), s["mu"].copy(), s["m2"].copy(), np.array(s["Z"]), s["s0"].copy(),
                         np.array(s["Omega"]), int(s["n_fits"]))
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("D,k,N", [(7, 2, 64), (130, 5, 257), (513, 3, 64), (5000, 4, 1000)])
def test_engine_fit_against_mirror(hip, D, k, N, dtype):
    """A Stan window of 3 pushes (init_buffer 0, window_size 3): at its end dense(A, B, Dm) from ahmc_get_metric_rank_update (on up to
    400 rows and columns) against the mirror's fit of the state read just before that push.  Draws with spikes Γ = linspace(20, 100, k)
    over a floor of 1.  The engine's Jacobi solvers and LAPACK differ, so the yardstick is the problem's own conditioning: 100× the
    change of the mirror's fit when Z and m2 are perturbed by relative 10⁻¹⁵ (float32 contexts: plus the rounding of A, B, Dm to
    float32, 2⁻²⁴·(|A| + 3·|B|·|Dm|·|B|ᵀ)).  The next window starts from the mirror's s₀ and spans the mirror's eigenvectors."""
    rs = np.random.default_rng(500 + D)
    C = spiked_cov(D, k, 20.0, 100.0, rs, sigma=0.5) if D <= 600 else None
    if C is not None:
        Lc = np.linalg.cholesky(C)
        draw = lambda: 3.0 + Lc @ rs.normal(size=(D, N))  # noqa: E731
    else:  # (no D×D factor at D = 5000: the same model drawn directly)
        Uq, _ = np.linalg.qr(rs.normal(size=(D, k)))
        S, G = np.exp(0.5 * rs.normal(size=(D, 1))), np.linspace(20.0, 100.0, k)
        draw = lambda: 3.0 + S * (rs.normal(size=(D, N)) + Uq @ (np.sqrt(G)[:, None] * rs.normal(size=(k, N))))  # noqa: E731
        C = None
    var = np.diag(C) if C is not None else S[:, 0] ** 2 * (1 + (Uq * Uq) @ G)
    batches = [np.asfortranarray(draw().astype(dtype)) for _ in range(3)]
    e = A.Engine(A.Hamiltonian(A.DiagEuclideanMetric(var.astype(dtype)), A.IsoGaussian(D)), N, dtype=dtype, rng=A.PhiloxRNG(6), lib=hip)
    e.adaptor_init(stan_lowrank(D, k, seed=9, ws=3))
    e.adapt(1, 1000, theta=batches[0], alpha=np.ones(N))
    e.adapt(2, 1000, theta=batches[1], alpha=np.ones(N))
    before = e.lowrank_state()
    assert before["n"] == 2 * N
    e.adapt(3, 1000, theta=batches[2], alpha=np.ones(N))
    Ae, Be, De = e.get_metric_rank_update()
    after = e.lowrank_state()
    e.close()
    st = mirror_state(before)
    RU.lowrank_push(st, batches[2])
    fit = RU.lowrank_fit(st)
    V = st.V.copy()
    pert = mirror_state(before)
    RU.lowrank_push(pert, batches[2])
    pert.Z *= 1 + 1e-15 * rs.choice([-1.0, 1.0], size=pert.Z.shape)
    pert.m2 *= 1 + 1e-15 * rs.choice([-1.0, 1.0], size=D)
    fit_p = RU.lowrank_fit(pert)
    idx = np.arange(D) if D <= 400 else np.sort(rs.choice(D, 400, replace=False))
    Mm, Mp, Me = sub_dense(*fit, idx), sub_dense(*fit_p, idx), sub_dense(Ae, Be, De, idx)
    scale = np.abs(Mm).max()
    yard = np.abs(Mm - Mp).max()
    tol = 100 * yard
    if dtype == np.float32:
        aB = np.abs(fit[1][idx])
        tol += float(2.0 ** -24 * (np.abs(np.diag(fit[0][idx])) + 3 * aB @ np.abs(fit[2]) @ aB.T).max())
    err = np.abs(Me - Mm).max()
    _record(f"gpu_fit {np.dtype(dtype).name} D={D} k={k} N={N}", error=err, tolerance=tol, perturbation_change=yard, largest_entry=scale)
    print(D, k, N, np.dtype(dtype).name, "err", err, "tol", tol, "scale", scale)
    assert yard > 0 and err <= tol, (err, tol)
    # the next window
    RU.lowrank_restart(st, fresh=after["Omega"][:, k:])
    assert (after["n"], after["n_fits"]) == (0, 1) and not after["Z"].any() and not after["m2"].any() and not after["mu"].any()
    np.testing.assert_allclose(after["s0"], st.s0, rtol=1e-12)
    overlap = np.abs(V.T @ after["Omega"][:, :k])
    np.testing.assert_allclose(overlap, np.eye(k), atol=max(1e-6, 1e4 * yard / scale))
    assert np.isfinite(after["Omega"]).all() and (k == after["ell"] or after["Omega"][:, k:].std() > 0.5)


def kern_for(N, eps, depth=5):
    return A.HMCKernel(A.Trajectory(A.MultinomialTS, A.Leapfrog(np.full(N, eps)), A.GeneralisedNoUTurn(max_depth=depth)))


def protocol_adaptor(kind, D, eps):
    pc, ssa = A.LowRankVar(D, 3, 8, seed=12), A.StepSizeAdaptor(0.8, A.Leapfrog(eps))
    if kind == "stan":
        return A.StanHMCAdaptor(pc, ssa, init_buffer=5, term_buffer=5, window_size=5)  # 40 adapts: windows end at 10 and 35
    return A.NaiveHMCAdaptor(pc, ssa) if kind == "naive" else pc


def protocol_target(name, D, rs):
    if name == "dense":
        return A.DenseGaussian(np.asfortranarray(np.linalg.inv(spiked_cov(D, 3, 10.0, 40.0, rs, sigma=0.5))))
    return A.IsoGaussian(D)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["stan", "naive", "massmatrix"])
@pytest.mark.parametrize("D,target", [(33, "dense"), (33, "iso"), (5000, "iso")])
def test_sample_equals_stepwise_and_resumes(hip, D, target, kind):
    """run(kernel, n, n_adapts) == transition + adapt per iteration, bit for bit; a checkpoint in the middle of a window + set_state on
    a fresh engine + the rest == the unbroken run; after adaptation the context == a fresh context given get_metric()"""
    N, n_adapts, n_total, cut = 16, 40, 46, 20
    rs = np.random.default_rng(600 + D)
    tgt = protocol_target(target, D, rs)
    eps = 0.2 * D ** -0.25
    th0 = rs.normal(size=(D, N))
    kern = kern_for(N, eps)

    def engine(metric=None):
        e = A.Engine(A.Hamiltonian(metric or A.UnitEuclideanMetric((D, N)), tgt), N, rng=A.PhiloxRNG(31), lib=hip)
        e.set_integrator(kern.tau.integrator)
        return e

    def fresh():
        e = engine()
        e.set_position(th0)
        e.adaptor_init(protocol_adaptor(kind, D, eps))
        return e

    def final(e):
        return (e.theta(), e.get_stepsize()) + tuple(e.get_metric())

    bulk = fresh()
    bulk.run(kern, n_adapts, n_adapts=n_adapts)
    st_end = bulk.get_state()               # adaptation has just ended
    bulk.run(kern, n_total, n_adapts=n_adapts, i_first=n_adapts + 1)
    want = final(bulk)
    bulk.close()
    assert not np.array_equal(want[3], np.zeros_like(want[3])), "the adaptor never fitted a B"

    step = fresh()
    for i in range(1, n_total + 1):
        step.transition(kern)
        step.adapt(i, n_adapts)
        if i == cut:
            st_cut = step.get_state()
    for a, b in zip(final(step), want):
        np.testing.assert_array_equal(a, b)
    step.close()
    assert st_cut["lowrank"]["n"] > 0 and st_cut["adaptor"]["n_welford"] == 0 and st_cut["metric_kind"] == capi.METRIC_RANK_UPDATE

    res = engine()
    res.set_state(st_cut)
    back = res.get_state()
    for key in ("mu", "m2", "Z", "s0", "Omega", "n", "n_fits", "k", "ell", "seed"):
        np.testing.assert_array_equal(back["lowrank"][key], st_cut["lowrank"][key])
    res.run(kern, n_total, n_adapts=n_adapts, i_first=cut + 1)
    for a, b in zip(final(res), want):
        np.testing.assert_array_equal(a, b)
    res.close()

    plain = dict(st_end)                    # the same point, step sizes and counters under the adapted metric, no adaptor
    plain["lowrank"] = None
    plain["adaptor"] = dict(st_end["adaptor"], kind=capi.ADAPT_NONE, has_da=0, adapting=0)
    plain["da"] = None
    new = engine(A.RankUpdateEuclideanMetric(*st_end["metric"]))
    new.set_state(plain)
    new.run(kern, n_total, n_adapts=0, i_first=n_adapts + 1)
    np.testing.assert_array_equal(new.theta(), want[0])
    new.close()


@pytest.mark.gpu
def test_sample_free_function(hip):
    """A.sample with StanHMCAdaptor(LowRankVar) == the engine's own loop, bit for bit"""
    D, N, n, n_adapts = 9, 16, 14, 10
    rs = np.random.default_rng(650)
    h = A.Hamiltonian(A.DiagEuclideanMetric(0.5 + rs.random(D)), A.IsoGaussian(D))
    kern = kern_for(N, 0.3)
    ad = A.StanHMCAdaptor(A.LowRankVar(h.metric, 2, 4, seed=1), A.StepSizeAdaptor(0.8, kern.tau.integrator), init_buffer=2, term_buffer=2, window_size=3)
    th0 = rs.normal(size=(D, N))
    thetas, stats = A.sample(A.PhiloxRNG(8), h, kern, th0, n, adaptor=ad, n_adapts=n_adapts, lib=hip)
    assert len(thetas) == n and [s["is_adapt"] for s in stats] == [True] * n_adapts + [False] * (n - n_adapts)
    e = A.Engine(h, N, rng=A.PhiloxRNG(8), lib=hip)
    e.set_integrator(kern.tau.integrator)
    e.set_position(th0)
    e.adaptor_init(ad)
    e.run(kern, n, n_adapts=n_adapts)
    np.testing.assert_array_equal(thetas[-1], e.theta())
    assert e.lowrank_state()["n_fits"] >= 1 and e.get_metric()[1].any()
    e.close()


@pytest.mark.gpu
def test_usefulness(hip):
    """DenseGaussian with C = S(I + UΓUᵀ)S at D = 64, k = 3, Γ = linspace(25, 100, 3), 256 chains, 150 adapting transitions of
    StanHMCAdaptor(LowRankVar) with buffers 10 / 20 and windows from 10 (they end at 20, 40 and 130): the final metric's
    cond(L⁻¹CL⁻ᵀ) is at most 1/10 of diag(C)'s (both from C, in numpy), and the 100 draws that follow have R-hat < 1.05
    (Engine.summarystats).  The numpy prototype of the estimator reached 1.3–1.8 at its third window on comparable targets."""
    import torch

    D, k, N, n_adapts, n_keep = 64, 3, 256, 150, 100
    rs = np.random.default_rng(700)
    C = spiked_cov(D, k, 25.0, 100.0, rs)
    P = np.asfortranarray(np.linalg.inv(C))
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((D, N)), A.DenseGaussian(P)), N, rng=A.PhiloxRNG(41), lib=hip)
    kern = A.HMCKernel(A.Trajectory(A.MultinomialTS, A.Leapfrog(np.full(N, 0.05)), A.GeneralisedNoUTurn(max_depth=8)))
    e.set_integrator(kern.tau.integrator)
    e.set_position(rs.normal(size=(D, N)))
    e.adaptor_init(A.StanHMCAdaptor(A.LowRankVar(D, k), A.StepSizeAdaptor(0.8, kern.tau.integrator), init_buffer=10, term_buffer=20, window_size=10))
    assert A.stan_windows(n_adapts, 10, 20, 10, lib=hip)[2] == [20, 40, 130]
    draws = torch.empty((n_keep, N, D), dtype=torch.float64, device="cuda")
    e.run(kern, n_adapts + n_keep, n_adapts=n_adapts, drop_warmup=True, samples_out=draws.data_ptr())
    e.sync()
    Av, B, Dm = e.get_metric()
    assert e.lowrank_state()["n_fits"] == 3
    cond, diag = precond_cond(C, RU.dense(Av, B, Dm)), precond_cond(C, np.diag(np.diag(C)))
    st = e.summarystats(draws.data_ptr(), n_keep)
    depth = float(e.stats()["tree_depth"].mean())
    e.close()
    _record("gpu_usefulness D=64 k=3 N=256", cond_final_metric=cond, cond_diag=diag, rhat_max=float(np.max(st["rhat"])), mean_tree_depth=depth,
            prototype_third_window=[1.82, 1.29, 2.70])
    print("cond", cond, "diag", diag, "rhat", np.max(st["rhat"]), "depth", depth)
    assert cond <= diag / 10, (cond, diag)
    assert np.max(st["rhat"]) < 1.05, np.max(st["rhat"])


@pytest.mark.gpu
def test_refusals_and_misuse(hip):
    D, N = 8, 16
    rs = np.random.default_rng(800)
    kern = kern_for(N, 0.2)
    th = rs.normal(size=(D, N))

    def engine(metric, d=D):
        e = A.Engine(A.Hamiltonian(metric, A.IsoGaussian(d)), N, rng=3, lib=hip)
        e.set_integrator(kern.tau.integrator)
        e.set_position(rs.normal(size=(d, N)))
        return e

    def still_runs(e):  # after a refusal the context samples with the metric it had
        e.transition(kern)
        assert np.all(np.isfinite(e.theta()))

    init = lambda e, k, p=8, kind=capi.ADAPT_STAN: e._call("ahmc_lowrank_adaptor_init", kind, 0.8, 75, 50, 25, k, p, 0)  # noqa: E731
    e = engine(A.DiagEuclideanMetric(np.asfortranarray(0.5 + rs.random((D, N)))))
    with pytest.raises(A.UnsupportedError, match="shared by all chains"):
        init(e, 2)
    still_runs(e)
    e.close()
    e = engine(A.DenseEuclideanMetric(np.eye(D)))
    with pytest.raises(A.UnsupportedError, match="DenseEuclideanMetric"):
        init(e, 2)
    still_runs(e)
    e.close()
    e = engine(A.UnitEuclideanMetric((D, N)))
    for k in (0, D + 1):
        with pytest.raises(A.ArgumentError, match="DimensionMismatch"):
            init(e, k)
    with pytest.raises(A.ArgumentError, match="AHMC_LOWRANK_MAX_ELL"):
        init(e, 2, 39)
    with pytest.raises(A.ArgumentError, match="kind"):
        init(e, 2, 8, capi.ADAPT_STEPSIZE)
    with pytest.raises(A.AHMCError, match="no low-rank adaptor"):
        e._call("ahmc_lowrank_get_state", capi.C.byref(capi.LowRankState()), None, None, None, None, None)
    still_runs(e)
    assert e.get_metric() is None  # (still the unit metric)
    e.close()
    big = engine(A.UnitEuclideanMetric((40, N)), 40)
    with pytest.raises(A.ArgumentError, match="AHMC_RANK_UPDATE_MAX_K"):
        init(big, 33, 0)
    still_runs(big)
    big.close()
    # a rank update of a higher rank than k
    Av, B, Dm = 0.5 + rs.random(D), rs.normal(size=(D, 3)), np.diag(rs.random(3))
    e = engine(A.RankUpdateEuclideanMetric(Av, B, Dm))
    with pytest.raises(A.ArgumentError, match="DimensionMismatch"):
        init(e, 2)
    # … and of a lower one: the same M⁻¹, padded
    init(e, 5)
    A5, B5, D5 = e.get_metric_rank_update()
    assert B5.shape == (D, 5) and not B5[:, 3:].any()
    np.testing.assert_array_equal(RU.dense(A5, B5, D5), RU.dense(Av, B, Dm))
    np.testing.assert_allclose(e.lowrank_state()["s0"], np.sqrt(RU.diag_inv_metric(Av, B, Dm)), rtol=1e-14)
    # the plain ahmc_adaptor_init keeps refusing this metric, and ends the low-rank adaptor
    with pytest.raises(A.UnsupportedError, match="RankUpdateEuclideanMetric"):
        e._call("ahmc_adaptor_init", capi.ADAPT_STAN, 0.8, 75, 50, 25)
    assert e.lowrank_state() is None
    still_runs(e)
    e.close()
    # a communicator
    e = engine(A.UnitEuclideanMetric((D, N)))
    e.comm_init(e.comm_unique_id(), 1, 0)
    with pytest.raises(A.UnsupportedError, match="communicator"):
        init(e, 2)
    still_runs(e)
    e.close()
    # ahmc_set_metric to Diag in the middle of the adaptation: the adaptor is refused from then on, by ahmc_adapt and by ahmc_sample
    e = engine(A.UnitEuclideanMetric((D, N)))
    e.adaptor_init(stan_lowrank(D, 2, ib=2, tb=2, ws=3, eps=0.2))
    e.run(kern, 4, n_adapts=20)
    e.set_metric(A.DiagEuclideanMetric(np.ones(D)))
    e.transition(kern)
    with pytest.raises(A.UnsupportedError, match="low-rank adaptor"):
        e.adapt(5, 20)
    with pytest.raises(A.UnsupportedError, match="low-rank adaptor"):
        e.run(kern, 8, n_adapts=20, i_first=6)
    still_runs(e)
    # … until an adaptor is set up again
    e.adaptor_init(A.StanHMCAdaptor(A.MassMatrixAdaptor(A.DiagEuclideanMetric(np.ones(D))), A.StepSizeAdaptor(0.8, A.Leapfrog(0.2))))
    e.run(kern, 3, n_adapts=3)
    e.close()
    # state of another shape
    e = engine(A.UnitEuclideanMetric((D, N)))
    e.adaptor_init(A.LowRankVar(D, 2, 3))
    s = e.lowrank_state()
    e.adaptor_init(A.LowRankVar(D, 3, 3))
    with pytest.raises(A.ArgumentError, match="k, ell"):
        e.set_lowrank_state(s)
    e.close()
