"""MCMCChains' `summarystats` columns (include/ahmc_diag.h): rank-normalised split-chain R̂ and bulk / tail / basic ESS.

CPU: the host mirror `diagnostics.summarystats` against a literal, slow transcription of the definition below; its statistical
sanity; AS241 against scipy; the header against `capi.DIAG_SIGNATURES` and the built library; the new kernels without scratch.
GPU: `Engine.summarystats` / `Engine.rank_normalize` (ahmc_diag_summary / ahmc_diag_rank_normalize) against the host mirror on
the same families, at scale, under dimension batching, on real sampler output, and the refusals.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ahmc_amd as A
from ahmc_amd import _capi as capi
from ahmc_amd import diagnostics as dg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ahmc_diag.h")
NAMES = dg.SUMMARY_NAMES
FAMILIES = ("iid", "ar-0.6", "ar0.5", "ar0.95", "offset", "cauchy", "grid", "zeros", "const_nan")


def family(name, K, D, N, rng):
    """draws (K, D, N) of one test family"""
    if name.startswith("ar"):
        phi = float(name[2:])
        e = rng.normal(size=(K, D, N))
        x = np.empty_like(e)
        x[0] = e[0] / np.sqrt(1 - phi * phi)
        for k in range(1, K):
            x[k] = phi * x[k - 1] + e[k]
        return x
    if name == "offset":
        return rng.normal(size=(K, D, N)) + 2.0 * np.arange(N)[None, None, :]
    if name == "cauchy":
        return rng.standard_cauchy(size=(K, D, N))
    if name == "grid":
        return np.round(rng.normal(size=(K, D, N)) * 4) / 4
    if name == "zeros":
        x = np.round(rng.normal(size=(K, D, N)))
        x[x == 0] = np.where(rng.random(size=(x == 0).sum()) < 0.5, -0.0, 0.0)
        return x
    if name == "const_nan":
        x = rng.normal(size=(K, D, N))
        x[:, 0, :] = 1.5                                # a constant dimension (exact chain means: W = 0)
        if D > 1:
            x[K // 3, 1, N - 1] = np.nan                # one NaN
        return x
    return rng.normal(size=(K, D, N))


# ---------------------------------------------------------------------------------------------------------------------
# the definition, transcribed literally (one dimension at a time, Python loops)
# ---------------------------------------------------------------------------------------------------------------------
def _spec_ranks(v):
    order = sorted(range(len(v)), key=lambda i: v[i])
    r = [0.0] * len(v)
    i = 0
    while i < len(order):
        j = i
        while j + 1 < len(order) and v[order[j + 1]] == v[order[i]]:
            j += 1
        for q in range(i, j + 1):
            r[order[q]] = ((i + 1) + (j + 1)) / 2
        i = j + 1
    return np.array(r)


def _spec_rhat_ess(chains, max_lag):
    """chains: list of m lists of n values → (ESS, R̂)"""
    y = np.array(chains, dtype=np.float64)
    m, n = y.shape
    S = m * n
    means = [sum(c) / n for c in y]
    vars_ = [sum((v - mu) ** 2 for v in c) / (n - 1) for c, mu in zip(y, means)]
    W = sum(vars_) / m
    ybar = sum(means) / m
    Bn = sum((mu - ybar) ** 2 for mu in means) / (m - 1)
    varp = (n - 1) / n * W + Bn
    if W == 0:
        return float("nan"), float("nan")
    rhat = np.sqrt(varp / W)

    def rho_hat(t):
        ac = [sum((c[k] - mu) * (c[k + t] - mu) for k in range(n - t)) / n for c, mu in zip(y, means)]
        return 1 - (W - sum(ac) / m) / varp

    rho = np.zeros(n + 3)
    rho[0] = 1
    rho[1] = rho_hat(1)
    even, odd, t = 1, rho[1], 1
    cap = n - 4 if max_lag == 0 else min(n - 4, max_lag)
    while t < cap and even + odd > 0:
        even, odd = rho_hat(t + 1), rho_hat(t + 2)
        if even + odd >= 0:
            rho[t + 1], rho[t + 2] = even, odd
        t += 2
    tmax = t
    if even > 0:
        rho[tmax + 1] = even
    t = 1
    while t <= tmax - 3:
        if rho[t + 1] + rho[t + 2] > rho[t - 1] + rho[t]:
            rho[t + 1] = rho[t + 2] = (rho[t - 1] + rho[t]) / 2
        t += 2
    tau = -1 + 2 * sum(rho[0:tmax]) + rho[tmax + 1]
    return min(S / tau, S * np.log10(S)), rhat


def spec_summary(draws, max_lag=0):
    K, D, N = draws.shape
    n = K // 2
    out = {k: np.full(D, np.nan) for k in NAMES}
    for d in range(D):
        chains = []
        for c in range(N):
            chains.append([float(draws[k, d, c]) for k in range(n)])
            chains.append([float(draws[k, d, c]) for k in range(K - n, K)])
        x = [v for ch in chains for v in ch]
        S = len(x)
        if not all(np.isfinite(x)):
            continue
        xs = sorted(x)
        med = 0.5 * (xs[S // 2 - 1] + xs[S // 2]) if S % 2 == 0 else xs[S // 2]

        def q7(p):
            h = (S - 1) * p
            lo = int(np.floor(h))
            hi = min(lo + 1, S - 1)
            return xs[lo] + (h - lo) * (xs[hi] - xs[lo])

        q05, q95 = q7(0.05), q7(0.95)
        z = dg.ndtri((_spec_ranks(x) - 0.375) / (S + 0.25))
        zf = dg.ndtri((_spec_ranks([abs(v - med) for v in x]) - 0.375) / (S + 0.25))

        def as_chains(v):
            return [list(v[j * n:(j + 1) * n]) for j in range(2 * N)]

        ess_basic, _ = _spec_rhat_ess(chains, max_lag)
        ess_bulk, rb = _spec_rhat_ess(as_chains(z), max_lag)
        _, rt = _spec_rhat_ess(as_chains(zf), max_lag)
        e05, _ = _spec_rhat_ess(as_chains([1.0 if v <= q05 else 0.0 for v in x]), max_lag)
        e95, _ = _spec_rhat_ess(as_chains([1.0 if v <= q95 else 0.0 for v in x]), max_lag)
        mean = sum(x) / S
        std = np.sqrt(sum((v - mean) ** 2 for v in x) / (S - 1))
        with np.errstate(invalid="ignore"):      # (tiny n: the truncation can give τ < 0, hence ESS < 0, as defined)
            mcse = std / np.sqrt(ess_basic)
        row = {"mean": mean, "std": std, "mcse": mcse, "ess_bulk": ess_bulk,
               "ess_tail": np.nan if np.isnan(e05) or np.isnan(e95) else min(e05, e95),
               "rhat": np.nan if np.isnan(rb) or np.isnan(rt) else max(rb, rt), "ess_basic": ess_basic, "rhat_bulk": rb, "rhat_tail": rt}
        for k, v in row.items():
            out[k][d] = v
    return out


def assert_summary_close(got, want, rtol_moments, rtol_ess, what=""):
    for k in NAMES:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=f"{what} {k}: NaN pattern")
        ok = ~np.isnan(w)
        rtol = rtol_moments if k in ("mean", "std") else rtol_ess
        np.testing.assert_allclose(g[ok], w[ok], rtol=rtol, atol=1e-300, err_msg=f"{what} {k}")


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_host_mirror_equals_the_literal_definition():
    rng = np.random.default_rng(20211)
    shapes = [(4, 2, 1), (5, 2, 3), (8, 3, 2), (13, 2, 4), (24, 3, 3), (31, 2, 2), (40, 2, 3)]
    n_sets = 0
    for i in range(108):
        fam = FAMILIES[i % len(FAMILIES)]
        K, D, N = shapes[(i // len(FAMILIES)) % len(shapes)]
        x = family(fam, K, D, N, rng)
        max_lag = 0 if i % 4 else 3
        got, want = dg.summarystats(x, max_lag=max_lag), spec_summary(x, max_lag=max_lag)
        assert_summary_close(got, want, 1e-12, 1e-12, what=f"{fam} K={K} D={D} N={N}")
        n_sets += 1
    assert n_sets >= 100


def test_host_mirror_statistical_sanity():
    rng = np.random.default_rng(7)
    K, D, N = 1000, 3, 8
    S = N * K
    r = dg.summarystats(rng.normal(size=(K, D, N)))
    assert np.all((r["ess_bulk"] / S > 0.9) & (r["ess_bulk"] / S < 1.1)), r["ess_bulk"] / S
    assert np.all(r["rhat"] < 1.005), r["rhat"]
    r = dg.summarystats(family("ar0.9", 4000, 3, 8, rng))
    np.testing.assert_allclose(r["ess_basic"] / (8 * 4000), 1 / 19, rtol=0.2)
    r = dg.summarystats(family("offset", K, D, N, rng))
    assert np.all(r["rhat"] > 1.1), r["rhat"]
    r = dg.summarystats(family("cauchy", K, D, N, rng))
    assert np.all((r["ess_bulk"] / S > 0.8) & (r["ess_bulk"] / S < 1.2)), r["ess_bulk"] / S
    # constant dimension: mean / std defined, ESS and R̂ NaN; a NaN anywhere in a dimension: NaN everywhere
    r = dg.summarystats(family("const_nan", 20, 3, 4, rng))
    assert r["mean"][0] == 1.5 and r["std"][0] == 0 and np.isnan(r["ess_bulk"][0]) and np.isnan(r["rhat"][0])
    assert all(np.isnan(r[k][1]) for k in NAMES)
    assert all(np.isfinite(r[k][2]) for k in NAMES)


def test_as241_against_scipy_ndtri():
    special = pytest.importorskip("scipy.special")
    rng = np.random.default_rng(3)
    grids = [(np.arange(1, 2 * S + 2) * 0.5 - 0.375) / (S + 0.25) for S in (4, 37, 1000, 4096, 10000)]
    p = np.concatenate(grids + [rng.random(20000), 10.0 ** -rng.uniform(1, 300, 5000), 1 - 10.0 ** -rng.uniform(1, 15, 2000)])
    np.testing.assert_allclose(dg.ndtri(p[:sum(len(g) for g in grids)]), special.ndtri(p[:sum(len(g) for g in grids)]), rtol=1e-15, atol=0)
    # everywhere else within a few ulp (AS241 and Cephes are both ~1e-16 approximations)
    np.testing.assert_allclose(dg.ndtri(p), special.ndtri(p), rtol=2e-15, atol=0)
    assert dg.ndtri(0.5) == 0 and dg.ndtri(0.0) == -np.inf and dg.ndtri(1.0) == np.inf


def diag_header_prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER, encoding="utf-8").read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"\bint32_t\s+(ahmc_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        params = " ".join(m.group(2).split())
        protos[m.group(1)] = [] if params in ("", "void") else [p.strip() for p in params.split(",")]
    return protos


def test_diag_header_binding_table_and_exports():
    protos = diag_header_prototypes()
    assert set(protos) == set(capi.DIAG_SIGNATURES)
    for name, params in protos.items():
        assert len(params) == len(capi.DIAG_SIGNATURES[name][1]), name
    assert re.search(r"#define AHMC_DIAG_VERSION (\d+)", open(HEADER).read()).group(1) == str(capi.AHMC_DIAG_VERSION)
    # not part of the main ABI: ahmc_hip.h keeps its version and declares none of them
    main = open(os.path.join(ROOT, "include", "ahmc_hip.h")).read()
    assert not any(n in main for n in protos) and "ahmc_diag" not in "".join(capi.SIGNATURES)
    so = A.build_hip_library()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert set(protos) <= set(re.findall(r"\bT (ahmc_[a-z_0-9]+)$", out, flags=re.M))
    import torch  # noqa: F401

    lib = A.CLib(so)
    assert lib.has_diag and lib.dll.ahmc_diag_version() == capi.AHMC_DIAG_VERSION


def test_checker_has_no_diag_and_engine_refuses(oracle):
    assert not oracle.has_diag
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric(2), A.IsoGaussian(2)), 3, lib=oracle)
    with pytest.raises(A.UnsupportedError):
        e.summarystats(np.zeros((8, 3, 2)), 8)
    with pytest.raises(A.UnsupportedError):
        e.rank_normalize(np.zeros((8, 3, 2)), 8, 0)
    e.close()


DIAG_KERNELS = ("k_dg_gather", "k_dg_hist", "k_dg_scatter", "k_sc_reduce", "k_sc_parts", "k_sc_apply", "k_dg_segstat", "k_dg_rank",
                "k_dg_fold", "k_dg_moments", "k_dg_pool", "k_dg_acov", "k_dg_acov_reduce", "k_dg_finalize", "k_dg_output", "k_dg_rank_out")


def test_diag_kernels_are_shipped_without_scratch():
    from ahmc_amd import build as B

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_meta
    finally:
        sys.path.pop(0)
    assert os.path.exists(B.OUT), "build() first"
    meta = kernel_meta.kernel_meta(B.OUT)
    demangled = subprocess.run(["c++filt"], input="\n".join(k["name"] for k in meta), capture_output=True, text=True, check=True).stdout.splitlines()
    found = {}
    for k, dn in zip(meta, demangled):
        m = re.search(r"ahmc::diag::(k_[a-z_]+)", dn)
        if m:
            found.setdefault(m.group(1), []).append((dn, k))
    assert sorted(found) == sorted(DIAG_KERNELS), sorted(found)
    for name, ks in found.items():
        for dn, k in ks:
            assert k["private_segment_fixed_size"] == 0, (dn, k)
            assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, (dn, k)
    # f32 and f64 keys both present
    assert any("unsigned int" in dn for dn, _ in found["k_dg_scatter"]) and any("unsigned long" in dn for dn, _ in found["k_dg_scatter"])


def test_julia_diag_ccalls_match_the_header():
    src = open(os.path.join(ROOT, "julia", "AdvancedHMCMI355XDiag.jl"), encoding="utf-8").read()
    src = re.sub(r"#[^\n]*", "", src)
    protos = diag_header_prototypes()
    jl = {"Cint": "int32_t", "Int64": "int64_t", "Int32": "int32_t"}
    calls = []
    for m in re.finditer(r"ccall\(\(:(ahmc_[a-z_0-9]+), LIB\),\s*(\w+),\s*\(", src):
        i, depth = m.end(), 1                                    # the argument-type tuple
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
        calls.append((m.group(1), m.group(2), types))
    assert {c[0] for c in calls} == set(protos), [c[0] for c in calls]
    for name, ret, types in calls:
        assert ret == "Cint", name
        assert len(types) == len(protos[name]), (name, types)
        for t, p in zip(types, protos[name]):
            if "*" in p:
                assert t.startswith(("Ptr{", "Ref{")), (name, t, p)
            else:
                assert jl.get(t) == p.split()[0], (name, t, p)
    ext = open(os.path.join(ROOT, "julia", "AdvancedHMCMI355XExt.jl"), encoding="utf-8").read()
    assert 'include("AdvancedHMCMI355XDiag.jl")' in ext


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def engine(lib, D, N, dtype=np.float64):
    return A.Engine(A.Hamiltonian(A.UnitEuclideanMetric(D), A.IsoGaussian(D)), N, dtype=dtype, lib=lib)


def to_device(x, dtype):
    """(K, D, N) host draws → the (D, N, K) device layout of ahmc_sample: (d, c, k) at d + D·c + D·N·k"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.transpose(x, (0, 2, 1)).astype(dtype))).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_device_summary_matches_host_mirror(hip, dtype):
    rng = np.random.default_rng(11 if dtype == np.float64 else 12)
    for i, fam in enumerate(FAMILIES):
        for K, D, N in ((64, 3, 4), (33, 2, 5), (4, 2, 3), (101, 2, 1)):
            x = family(fam, K, D, N, rng).astype(dtype)
            xd = to_device(x, dtype)
            e = engine(hip, D, N, dtype)
            got = e.summarystats(xd.data_ptr(), K)
            want = dg.summarystats(x.astype(np.float64))
            assert_summary_close(got, want, 1e-12, 1e-10, what=f"{fam} {np.dtype(dtype).name} K={K} D={D} N={N}")
            if i == 0:
                got3 = e.summarystats(xd.data_ptr(), K, max_lag=3)
                assert_summary_close(got3, dg.summarystats(x.astype(np.float64), max_lag=3), 1e-12, 1e-10, what="max_lag=3")
            e.close()


@pytest.mark.gpu
def test_device_rank_normalize_matches_numpy_ranks(hip):
    special = pytest.importorskip("scipy.special")
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(5)
    for fam, K, D, N, dtype in (("grid", 31, 2, 6, np.float64), ("zeros", 20, 2, 5, np.float64), ("iid", 17, 3, 4, np.float32),
                                ("cauchy", 40, 1, 3, np.float64)):
        x = family(fam, K, D, N, rng).astype(dtype)
        xd = to_device(x, dtype)
        e = engine(hip, D, N, dtype)
        n = K // 2
        for d in range(D):
            y = dg._split_chains(x[:, d:d + 1].astype(np.float64))[0]         # (2N, n)
            flat = y.reshape(-1)
            S = flat.size
            z = special.ndtri((stats.rankdata(flat) - 0.375) / (S + 0.25)).reshape(2 * N, n)
            med = np.median(flat)
            zf = special.ndtri((stats.rankdata(np.abs(flat - med)) - 0.375) / (S + 0.25)).reshape(2 * N, n)
            for folded, want_split in ((False, z), (True, zf)):
                got = e.rank_normalize(xd.data_ptr(), K, d, folded=folded)     # (K, N)
                want = np.full((K, N), np.nan)
                want[:n] = want_split[0::2].T
                want[K - n:] = want_split[1::2].T
                np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
                ok = ~np.isnan(want)
                np.testing.assert_allclose(got[ok], want[ok], rtol=1e-13, atol=1e-300, err_msg=f"{fam} d={d} folded={folded}")
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(256, 2, 65536), (64, 5000, 8)], ids=["one_large_segment", "wide_context"])
def test_device_summary_at_scale(hip, shape):
    K, D, N = shape
    rng = np.random.default_rng(9)
    x = family("ar0.5", K, D, N, rng)
    x[:, -1, :] = np.round(x[:, -1, :] * 4) / 4                          # ties in the last dimension
    xd = to_device(x, np.float64)
    e = engine(hip, D, N)
    got = e.summarystats(xd.data_ptr(), K)
    want = dg.summarystats(x)
    assert_summary_close(got, want, 1e-12, 1e-10, what=f"K={K} D={D} N={N}")
    e.close()


def _summary_child(D, N, K, seed, mb):
    """the summary of the same draws in a fresh process with AHMC_DIAG_WORKSPACE_MB = mb"""
    code = f"""
import sys, numpy as np
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
import torch, ahmc_amd as A
from test_diag_summary import family, to_device, engine
x = family("ar0.95", {K}, {D}, {N}, np.random.default_rng({seed}))
e = engine(A.load_hip_library(), {D}, {N})
r = e.summarystats(to_device(x, np.float64).data_ptr(), {K})
sys.stdout.buffer.write(np.stack([r[k] for k in A.diagnostics.SUMMARY_NAMES]).tobytes())
"""
    env = dict(os.environ, AHMC_DIAG_WORKSPACE_MB=str(mb))
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    return np.frombuffer(res.stdout, dtype=np.float64).reshape(9, D)


@pytest.mark.gpu
def test_device_summary_is_deterministic_and_batch_invariant(hip, monkeypatch):
    import torch

    D, N, K, seed = 40, 64, 200, 21
    x = family("ar0.95", K, D, N, np.random.default_rng(seed))
    xd = to_device(x, np.float64)
    e = engine(hip, D, N)
    a = e.summarystats(xd.data_ptr(), K)
    b = e.summarystats(xd.data_ptr(), K)
    for k in NAMES:
        np.testing.assert_array_equal(a[k], b[k])
    # host out == device out
    dev = torch.empty((9, D), dtype=torch.float64, device="cuda")
    e.summarystats(xd.data_ptr(), K, out=dev)
    np.testing.assert_array_equal(dev.cpu().numpy(), np.stack([a[k] for k in NAMES]))
    # small workspaces force batches of a few dimensions (read per call; and in fresh processes)
    monkeypatch.setenv("AHMC_DIAG_WORKSPACE_MB", "1")
    c = e.summarystats(xd.data_ptr(), K)
    monkeypatch.delenv("AHMC_DIAG_WORKSPACE_MB")
    for k in NAMES:
        np.testing.assert_array_equal(a[k], c[k])
    ref = np.stack([a[k] for k in NAMES])
    for mb in (3, 100000):
        np.testing.assert_array_equal(_summary_child(D, N, K, seed, mb), ref)
    assert_summary_close(a, dg.summarystats(x), 1e-12, 1e-10)
    e.close()


@pytest.mark.gpu
def test_device_summary_of_real_sampler_output(hip):
    import torch

    D, N, n_adapts, K = 16, 4096, 500, 500
    rng = np.random.default_rng(4)
    h = A.Hamiltonian(A.UnitEuclideanMetric(D), A.IsoGaussian(D))
    e = A.Engine(h, N, rng=17, lib=hip)
    lf = A.Leapfrog(np.full(N, 0.3))
    e.set_integrator(lf)
    e.set_position(rng.normal(size=(D, N)))
    e.adaptor_init(A.StepSizeAdaptor(0.8, lf))
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn()))
    e.run(k, n_adapts, n_adapts)
    draws = torch.empty((K, N, D), dtype=torch.float64, device="cuda")
    e.run(k, K, 0, samples_out=draws.data_ptr())
    e.sync()
    got = e.summarystats(draws.data_ptr(), K)
    x = np.transpose(draws.cpu().numpy(), (0, 2, 1))                     # (K, D, N)
    assert_summary_close(got, dg.summarystats(x), 1e-12, 1e-10)
    S = N * 2 * (K // 2)
    assert np.all(got["rhat"] < 1.01), got["rhat"]
    assert np.all(got["ess_bulk"] > 0.3 * S), got["ess_bulk"] / S
    e.close()


@pytest.mark.gpu
def test_diag_misuse_is_refused_and_the_context_still_runs(hip):
    import torch

    D, N, K = 3, 8, 16
    rng = np.random.default_rng(8)
    x = rng.normal(size=(K, D, N))
    xd = to_device(x, np.float64)
    e = engine(hip, D, N)
    e.set_integrator(A.Leapfrog(np.full(N, 0.2)))
    e.set_position(rng.normal(size=(D, N)))
    kern = A.HMCKernel(A.Trajectory(A.MultinomialTS, A.Leapfrog(np.full(N, 0.2)), A.GeneralisedNoUTurn()))
    out = np.empty((9, D))

    def call(*args):
        return hip.dll.ahmc_diag_summary(e._ctx, *args)

    def transition_ok():
        e.transition(kern)
        assert np.isfinite(e.theta()).all()

    assert call(capi.as_ptr(x), K, 0, capi.as_ptr(out)) == capi.ERR_ARGUMENT            # host draws
    transition_ok()
    assert call(capi.as_ptr(xd), K, 0, None) == capi.ERR_ARGUMENT                       # out NULL
    transition_ok()
    assert call(capi.as_ptr(xd), 3, 0, capi.as_ptr(out)) == capi.ERR_ARGUMENT           # n_draws < 4
    transition_ok()
    assert call(capi.as_ptr(xd), K, -1, capi.as_ptr(out)) == capi.ERR_ARGUMENT          # max_lag < 0
    transition_ok()
    rk = np.empty((K, N))
    assert hip.dll.ahmc_diag_rank_normalize(e._ctx, capi.as_ptr(xd), K, D, 0, capi.as_ptr(rk)) == capi.ERR_ARGUMENT  # d out of range
    assert hip.dll.ahmc_diag_rank_normalize(e._ctx, capi.as_ptr(xd), K, -1, 0, capi.as_ptr(rk)) == capi.ERR_ARGUMENT
    transition_ok()
    # S = 2·N·⌊K/2⌋ ≥ 2³¹: refused before anything is read (the pointer only has to be a device pointer)
    big = engine(hip, 1, 1 << 20)
    rc = hip.dll.ahmc_diag_summary(big._ctx, capi.as_ptr(xd), 1 << 12, 0, capi.as_ptr(np.empty((9, 1))))
    assert rc == capi.ERR_UNSUPPORTED and b"2^31" in hip.dll.ahmc_last_error(big._ctx)
    big.close()
    transition_ok()
    # (a communicator of more than one rank is refused with AHMC_ERR_UNSUPPORTED too: two processes on one GPU,
    # tests/test_multirank_loopback.py::test_refusals_of_a_context_with_more_than_one_rank)
    e.close()
