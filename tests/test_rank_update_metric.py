"""RankUpdateEuclideanMetric: M⁻¹ = Diagonal(A) + B·Dm·Bᵀ shared by all chains (include/ahmc_rank_update.h,
advancedhmc.jl_amd/csrc/ahmc_rank_update.hpp, advancedhmc.jl_amd/rank_update.py).

Two references:
  * the host mirror (rank_update.py) for the per-step quantities: ℓκ, ∂H∂r through a leapfrog, the momentum map;
  * for whole transitions, a restatement: oracle/ahmc_ref.py's transitions with a Hamiltonian whose dHdr, neg_energy_r and
    rand_momentum are the mirror's (its step, build_tree, nuts_transition, hmc_transition and refresh call only those three), on
    the engine's Philox streams.
CPU: the mirror against DenseEuclideanMetric(W) (the reference's test/metric.jl:41-110), the momentum map's covariance in exact
form, the restatement against ahmc_ref's own Diag Hamiltonian at k = 0, the header against the bindings and the Julia ccalls, the
shipped kernels.  GPU: energies, leapfrog, refresh, transitions, find_good_stepsize, a sampling run that needs the metric, bit-for-bit
invariances and the refusals.
"""
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ahmc_ref as R  # noqa: E402

sys.path.pop(0)


def make_ru(D, k, rs, scale=1.0):
    """A (D,) in [0.5, 1.5), B (D, k), Dm symmetric positive definite (k, k)"""
    Av = 0.5 + rs.random(D)
    B = rs.normal(size=(D, k)) * scale / np.sqrt(max(D, 1))
    G = rs.normal(size=(k, k))
    Dm = G @ G.T / max(k, 1) + 0.5 * np.eye(k)
    return Av, np.asfortranarray(B), np.asfortranarray(Dm)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the mirror
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 5, "D"])
def test_mirror_against_dense_metric(k):
    """∂H∂r, neg_energy and _diag_inv_metric of RankUpdateEuclideanMetric(A, B, D) against DenseEuclideanMetric(W), W = A + B·D·Bᵀ
    (test/metric.jl:41-110)"""
    rs = np.random.default_rng(1)
    D = 9
    kk = D if k == "D" else k
    Av, B, Dm = make_ru(D, kk, rs, scale=3.0)
    m = A.RankUpdateEuclideanMetric(Av, B, Dm)
    W = RU.dense(Av, B, Dm)
    r = rs.normal(size=(D, 6))
    np.testing.assert_allclose(RU.dHdr(m.A, m.B, m.D, r), W @ r, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(RU.neg_energy(m.A, m.B, m.D, r), -np.einsum("ij,ij->j", r, W @ r) / 2, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(m._diag_inv_metric, np.diag(W), rtol=1e-13, atol=1e-13)
    assert m.size == (D,) and m.rank == kk and m.eltype == np.float64


@pytest.mark.parametrize("D,k", [(1, 0), (1, 1), (7, 3), (20, 5), (12, 12)])
def test_momentum_map_covariance_is_the_mass_matrix(D, k):
    """r = L·z with z ~ N(0, I) has covariance L·Lᵀ = W⁻¹: L·Lᵀ·W = I (the exact form of the reference's 200 000-sample test)"""
    rs = np.random.default_rng(2 + D + k)
    Av, B, Dm = make_ru(D, k, rs, scale=2.0)
    m = A.RankUpdateEuclideanMetric(Av, B, Dm)
    L = RU.momentum_map(m.factorization)
    np.testing.assert_allclose(L @ L.T @ RU.dense(Av, B, Dm), np.eye(D), atol=1e-10)


def test_constructors_and_argument_errors():
    for args in ((5,), (np.float32, 5), ((5,),), (np.float32, (5,))):
        m = A.RankUpdateEuclideanMetric(*args)
        assert m.size == (5,) and m.rank == 0 and m.B.shape == (5, 0) and m.D.shape == (0, 0)
        np.testing.assert_array_equal(m.A, np.ones(5))
    assert A.RankUpdateEuclideanMetric(np.float32, 5).eltype == np.float32
    Av, B, Dm = make_ru(6, 2, np.random.default_rng(3))
    np.testing.assert_array_equal(A.RankUpdateEuclideanMetric(np.diag(Av), B, Dm).A, Av)  # A as a Diagonal matrix
    with pytest.raises(A.ArgumentError, match="DomainError"):
        A.RankUpdateEuclideanMetric(-Av, B, Dm)
    with pytest.raises(A.ArgumentError, match="DimensionMismatch"):
        A.RankUpdateEuclideanMetric(Av, B, np.eye(3))
    with pytest.raises(A.ArgumentError, match="PosDefException"):
        A.RankUpdateEuclideanMetric(Av, B, -50 * np.eye(2))


# ---------------------------------------------------------------------------------------------------------------------
# the restatement: ahmc_ref's transitions with the mirror's metric
# ---------------------------------------------------------------------------------------------------------------------
class RUHamiltonian(R.Hamiltonian):
    def __init__(self, Av, B, Dm, fn):
        super().__init__([float(a) for a in Av], fn)  # (minv: a Diag-shaped list; every use of it goes through the overrides)
        self.Av, self.B, self.Dm = np.asarray(Av, dtype=np.float64), np.asarray(B, dtype=np.float64), np.asarray(Dm, dtype=np.float64)
        self.f = RU.woodbury_factorize(self.Av, self.B, self.Dm)

    def dHdr(self, r):
        return RU.dHdr(self.Av, self.B, self.Dm, np.asarray(r)).tolist()

    def neg_energy_r(self, r):
        return float(RU.neg_energy(self.Av, self.B, self.Dm, np.asarray(r)))

    def rand_momentum(self, rng):
        z = [rng.normal(R.RNG_MOMENTUM, d) for d in range(self.D)]
        return RU.rand_momentum(self.f, np.asarray(z)).tolist()


def ref_find_good_stepsize(seed, chain, iteration, h, theta, initial_step_size=0.1, max_n_iters=100):
    """ahmc_ref.find_good_stepsize with its momentum line restated (it reads h.minv directly): rand_momentum on RNG_FINDEPS"""
    eps = epsp = float(initial_step_size)
    loghalf = np.log(0.5)
    log_a_min, log_a_cross, log_a_max = 2 * loghalf, loghalf, np.log(0.75)
    d, invd = 2.0, 0.5
    rng = R.Rng(seed, chain, iteration)
    z0 = np.asarray([rng.normal(R.RNG_FINDEPS, k) for k in range(h.D)])
    z = R.phasepoint(h, list(theta), RU.rand_momentum(h.f, z0).tolist())
    H = R.energy(z)

    def Aeps(e):
        return R.energy(R.step(e, h, z))

    Hp = Aeps(eps)
    ratio_too_high = H - Hp > log_a_cross
    for _ in range(max_n_iters):
        epsp = d * eps if ratio_too_high else invd * eps
        Hp = Aeps(eps)
        if ratio_too_high != (H - Hp > log_a_cross):
            break
        eps = epsp
    eps, epsp = (eps, epsp) if eps <= epsp else (epsp, eps)
    for _ in range(max_n_iters):
        mid = eps / 2 + epsp / 2
        dH = H - Aeps(mid)
        if dH > log_a_max:
            eps = mid
        elif dH < log_a_min:
            epsp = mid
        else:
            eps = mid
            break
    return eps


def ref_transition(h, kind, cfg, seed, chain, it, theta, r):
    """one transition of the restatement from (θ, r) at iteration `it`: kind = "nuts" | "hmc" | "hmc_mn"; cfg: TS, criterion, eps,
    max_depth, L, jitter, temper"""
    rng = R.Rng(seed, chain, it)
    z = R.phasepoint(h, list(theta), list(r))
    z = R.refresh(rng, h, z)
    eps = cfg["eps"]
    if cfg.get("jitter"):
        eps = R.jitter(rng, eps, cfg["jitter"])
    if kind == "nuts":
        nt = R.NUTS(cfg["TS"], cfg["criterion"], eps, max_depth=cfg["max_depth"], temper_alpha=cfg.get("temper"))
        return R.nuts_transition(rng, h, nt, z)
    if kind == "hmc_mn":
        return R.hmc_multinomial_transition(rng, h, eps, cfg["L"], z)
    return R.hmc_transition(rng, h, eps, cfg["L"], z, temper_alpha=cfg.get("temper"))


def test_restatement_at_rank_zero_is_ahmc_refs_diag_hamiltonian():
    """k = 0, A = a: the restatement gives ahmc_ref's own DiagEuclideanMetric(a) transitions — the overrides are wired to the same
    Philox streams and the same places"""
    D, seed = 5, 9
    rs = np.random.default_rng(4)
    a = 0.5 + rs.random(D)
    hr = RUHamiltonian(a, np.zeros((D, 0)), np.zeros((0, 0)), R.iso_gaussian)
    hd = R.Hamiltonian(a.tolist(), R.iso_gaussian)
    for TS in (R.MultinomialTS, R.SliceTS):
        for crit in (R.CLASSIC, R.GENERALISED, R.STRICT):
            cfg = dict(TS=TS, criterion=crit, eps=0.4, max_depth=6)
            for chain in range(4):
                th, r = rs.normal(size=D), np.zeros(D)
                for it in range(3):
                    z1, s1 = ref_transition(hr, "nuts", cfg, seed, chain, it, th, r)
                    z2, s2 = ref_transition(hd, "nuts", cfg, seed, chain, it, th, r)
                    for key in ("n_steps", "tree_depth", "is_accept", "numerical_error"):
                        assert s1[key] == s2[key], (TS, crit, chain, it, key)
                    np.testing.assert_allclose(z1.theta, z2.theta, rtol=1e-13, atol=1e-13)
                    th, r = np.asarray(z1.theta), np.asarray(z1.r)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: header, bindings, Julia, the shipped kernels, the checker
# ---------------------------------------------------------------------------------------------------------------------
def header_prototypes():
    src = open(os.path.join(ROOT, "include", "ahmc_rank_update.h"), encoding="utf-8").read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(int32_t)\s+(ahmc_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        params = " ".join(m.group(3).split())
        protos[m.group(2)] = [] if params in ("", "void") else [p.strip() for p in params.split(",")]
    return protos, src


def test_header_and_bindings_agree():
    protos, src = header_prototypes()
    assert set(protos) == set(capi.RU_SIGNATURES)
    ct = {"int64_t*": capi.C.POINTER(capi.C.c_int64), "int64_t": capi.C.c_int64, "int32_t": capi.C.c_int32}
    for name, params in protos.items():
        res, args = capi.RU_SIGNATURES[name]
        assert res is capi.C.c_int32 and len(args) == len(params), name
        for p, a in zip(params, args):
            typ = p.rsplit(" ", 1)[0].replace("const ", "").replace(" ", "")
            if typ in ("void*", "ahmc_ctx*"):
                assert a is capi.C.c_void_p, (name, p)
            else:
                assert a is ct[typ], (name, p)
    assert re.search(r"#define AHMC_RANK_UPDATE_VERSION (\d+)", src).group(1) == str(capi.AHMC_RANK_UPDATE_VERSION)
    assert re.search(r"#define AHMC_RANK_UPDATE_MAX_K (\d+)", src).group(1) == str(capi.AHMC_RANK_UPDATE_MAX_K)
    hip_h = open(os.path.join(ROOT, "include", "ahmc_hip.h"), encoding="utf-8").read()
    assert "rank_update" not in hip_h  # (kept out of ahmc_hip.h and AHMC_ABI_VERSION)


def test_julia_ccalls_match_the_header():
    protos, _ = header_prototypes()
    src = open(os.path.join(ROOT, "julia", "AdvancedHMCMI355XRankUpdate.jl"), encoding="utf-8").read()
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
        seen.add(name)
        assert m.group(2) == "Cint" and len(types) == len(protos[name]), (name, types)
        for t, p in zip(types, protos[name]):
            if "*" in p:
                assert t.startswith(("Ptr{", "Ref{")), (name, t, p)
            else:
                assert {"int64_t": "Int64", "int32_t": "Cint"}[p.split()[0]] == t, (name, t, p)
    assert seen == set(protos)
    ext = open(os.path.join(ROOT, "julia", "AdvancedHMCMI355XExt.jl"), encoding="utf-8").read()
    assert 'include("AdvancedHMCMI355XRankUpdate.jl")' in ext and "ahmc_set_metric_rank_update" not in ext


def _kernel_meta():
    from ahmc_amd import build as B

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_meta
    finally:
        sys.path.pop(0)
    assert os.path.exists(B.OUT), "build() first"
    meta = kernel_meta.kernel_meta(B.OUT)
    names = subprocess.run(["c++filt"], input="\n".join(k["name"] for k in meta), capture_output=True, text=True, check=True).stdout.splitlines()
    return B.OUT, meta, names


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="needs llvm-objdump")
def test_library_exports_and_kernels_without_scratch():
    import ctypes

    so, meta, names = _kernel_meta()
    dll = ctypes.CDLL(so)
    for name in capi.RU_SIGNATURES:
        getattr(dll, name)
    want = [f"k_ru_{w}<{t}, {kb}>" for w in ("apply", "momentum") for t in ("float", "double") for kb in (4, 8, 16, 32)]
    found = {}
    for k, dn in zip(meta, names):
        for w in want:
            if dn.startswith(f"void ahmc::{w}("):
                found[w] = k
    assert sorted(found) == sorted(want), sorted(found)
    for w, k in found.items():  # (SGPR spills land in VGPR lanes, not in scratch)
        assert k["private_segment_fixed_size"] == 0, (w, k)
        assert k.get("vgpr_spill_count", 0) == 0, (w, k)


def test_cpu_checker_has_no_rank_update(oracle):
    assert oracle.has_rank_update is False
    D = 4
    h = A.Hamiltonian(A.RankUpdateEuclideanMetric(*make_ru(D, 2, np.random.default_rng(5))), A.IsoGaussian(D))
    with pytest.raises(A.UnsupportedError, match="ahmc_rank_update.h"):
        A.Engine(h, 3, lib=oracle)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
TOL = {np.float64: 1e-11, np.float32: 2e-4}


def ru_engine(hip, D, N, Av, B, Dm, dtype=np.float64, target=None, seed=7, eps=0.1, lf=None):
    h = A.Hamiltonian(A.RankUpdateEuclideanMetric(Av, B, Dm), target or A.IsoGaussian(D))
    e = A.Engine(h, N, dtype=dtype, rng=A.PhiloxRNG(seed), lib=hip)
    e.set_integrator(lf or A.Leapfrog(eps))
    return e


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1, 7, 128, 513, 4096, 5000, 8192])
@pytest.mark.parametrize("k", [0, 1, 5, 32])
def test_energies(hip, D, k):
    """ahmc_set_position(θ, r): ℓκ = −½ r·(M⁻¹r) against the mirror's neg_energy (f64; f32 at D = 513)"""
    if k > D:
        pytest.skip("k <= D")
    rs = np.random.default_rng(100 + D + k)
    Av, B, Dm = make_ru(D, k, rs, scale=2.0)
    N = 5
    th, r = rs.normal(size=(D, N)), rs.normal(size=(D, N))
    want = RU.neg_energy(Av, B, Dm, r)
    for dtype in ((np.float64, np.float32) if D == 513 else (np.float64,)):
        e = ru_engine(hip, D, N, Av, B, Dm, dtype=dtype)
        assert e.info("wide") == (1 if D > 4096 else 0)
        e.set_position(th, r)
        lk = e.phasepoint().lk.value
        np.testing.assert_allclose(lk, want, rtol=TOL[dtype] * 10, err_msg=str(dtype))
        Ag, Bg, Dg = e.get_metric()
        np.testing.assert_array_equal(Ag, Av.astype(dtype))
        np.testing.assert_array_equal(Bg, B.astype(dtype))
        np.testing.assert_array_equal(Dg, Dm.astype(dtype))
        e.close()


def mirror_leapfrog(Av, B, Dm, th, r, eps, n):
    """n leapfrogs of the iso Gaussian (g = θ) with ∂H∂r from the mirror"""
    th, r = th.copy(), r.copy()
    for _ in range(n):
        r = r - eps / 2 * th
        th = th + eps * RU.dHdr(Av, B, Dm, r)
        r = r - eps / 2 * th
    return th, r


@pytest.mark.gpu
@pytest.mark.parametrize("D,k", [(7, 3), (128, 5), (513, 32), (4096, 8), (5000, 8)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_leapfrog(hip, D, k, dtype):
    """ahmc_leapfrog(16) against the mirror's leapfrog, and (D <= 4096, f64) against a HIP DenseEuclideanMetric(W) context"""
    rs = np.random.default_rng(200 + D)
    Av, B, Dm = make_ru(D, k, rs, scale=2.0)
    N, eps = 6, 0.05
    th, r = rs.normal(size=(D, N)), rs.normal(size=(D, N))
    e = ru_engine(hip, D, N, Av, B, Dm, dtype=dtype, eps=eps)
    e.set_position(th, r)
    e.step(16)
    z = e.phasepoint()
    tw, rw = mirror_leapfrog(Av, B, Dm, th, r, eps, 16)
    tol = TOL[dtype]
    np.testing.assert_allclose(z.theta, tw, rtol=tol, atol=tol * 10)
    np.testing.assert_allclose(z.r, rw, rtol=tol, atol=tol * 10)
    np.testing.assert_allclose(z.lk.value, RU.neg_energy(Av, B, Dm, rw), rtol=tol * 10)
    if dtype == np.float64 and D <= 4096:
        d = A.Engine(A.Hamiltonian(A.DenseEuclideanMetric(np.asfortranarray(RU.dense(Av, B, Dm))), A.IsoGaussian(D)), N, rng=7, lib=hip)
        d.set_integrator(A.Leapfrog(eps))
        d.set_position(th, r)
        d.step(16)
        zd = d.phasepoint()
        np.testing.assert_allclose(z.theta, zd.theta, rtol=1e-11, atol=1e-11)
        np.testing.assert_allclose(z.r, zd.r, rtol=1e-11, atol=1e-11)
        d.close()
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("D,k", [(1, 1), (7, 5), (128, 32), (513, 4), (5000, 16)])
def test_refresh(hip, D, k):
    """the rank-update refresh equals mirror.rand_momentum(z), z the raw normals a Unit context with the same seed and iteration
    draws (ahmc_refresh_momentum does not advance the counter); partial refreshment α = 0.3 as well"""
    rs = np.random.default_rng(300 + D)
    Av, B, Dm = make_ru(D, k, rs, scale=2.0)
    N = 9
    th, r0 = rs.normal(size=(D, N)), rs.normal(size=(D, N))
    u = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((D, N)), A.IsoGaussian(D)), N, rng=A.PhiloxRNG(5, iteration=3), lib=hip)
    u.set_position(th, r0)
    u.refresh()
    z = u.phasepoint().r
    u.close()
    e = A.Engine(A.Hamiltonian(A.RankUpdateEuclideanMetric(Av, B, Dm), A.IsoGaussian(D)), N, rng=A.PhiloxRNG(5, iteration=3), lib=hip)
    f = RU.woodbury_factorize(Av, B, Dm)
    e.set_position(th, r0)
    e.refresh()
    np.testing.assert_allclose(e.phasepoint().r, RU.rand_momentum(f, z), rtol=1e-12, atol=1e-12)
    e.set_position(th, r0)
    e.refresh(A.PartialMomentumRefreshment(0.3))
    np.testing.assert_allclose(e.phasepoint().r, 0.3 * r0 + np.sqrt(1 - 0.09) * RU.rand_momentum(f, z), rtol=1e-12, atol=1e-12)
    e.close()


TRANSITIONS = [
    # (name, kind, cfg): the full matrix at D = 7 / 128
    *[(f"nuts_{ts.__name__}_{cn}", "nuts", dict(TS=ts, criterion=cr, max_depth=8))
      for ts in (R.MultinomialTS, R.SliceTS) for cn, cr in (("classic", R.CLASSIC), ("generalised", R.GENERALISED), ("strict", R.STRICT))],
    ("hmc_endpoint", "hmc", dict(L=7)),
    ("hmc_multinomial", "hmc_mn", dict(L=7)),
    ("hmc_fixed_time", "hmc", dict(L=None, lam=0.9)),
    ("nuts_jittered", "nuts", dict(TS=R.MultinomialTS, criterion=R.GENERALISED, max_depth=8, jitter=0.3)),
    ("nuts_tempered", "nuts", dict(TS=R.MultinomialTS, criterion=R.GENERALISED, max_depth=8, temper=1.05)),
    ("hmc_tempered", "hmc", dict(L=6, temper=1.05)),
]
TS_API = {R.MultinomialTS: A.MultinomialTS, R.SliceTS: A.SliceTS}
TC_API = {R.CLASSIC: A.ClassicNoUTurn, R.GENERALISED: A.GeneralisedNoUTurn, R.STRICT: A.StrictGeneralisedNoUTurn}


def api_kernel(kind, cfg, eps, N):
    if cfg.get("lam"):  # (FixedIntegrationTime needs ONE nominal step size)
        lf = A.Leapfrog(eps)
    elif cfg.get("jitter"):
        lf = A.JitteredLeapfrog(np.full(N, eps), cfg["jitter"])
    elif cfg.get("temper"):
        lf = A.TemperedLeapfrog(np.full(N, eps), cfg["temper"])
    else:
        lf = A.Leapfrog(np.full(N, eps))
    if kind == "nuts":
        return A.HMCKernel(A.Trajectory(TS_API[cfg["TS"]], lf, TC_API[cfg["criterion"]](max_depth=cfg["max_depth"]))), lf
    TS = A.MultinomialTS if kind == "hmc_mn" else A.EndPointTS
    if cfg.get("lam"):
        return A.HMCKernel(A.Trajectory(TS, lf, A.FixedIntegrationTime(cfg["lam"]))), lf
    return A.HMCKernel(A.Trajectory(TS, lf, A.FixedNSteps(cfg["L"]))), lf


def dense_gaussian_fn(P):
    def fn(theta):  # the engine's AHMC_TARGET_DENSE_GAUSS: ℓπ = −½θᵀPθ, ∇ℓπ = −Pθ
        g = P @ np.asarray(theta)
        return float(-0.5 * np.dot(theta, g)), (-g).tolist()
    return fn


LOG2PI = 1.8378770664093454835606594728112


def iso_gaussian_columns(th):  # the built-in iso Gaussian for the columns of (D, N): (ℓπ, ∇ℓπ), ExternalTarget's signature
    return -(th * th).sum(axis=0) / 2 - th.shape[0] * LOG2PI / 2, -th


def kernel_target(D):
    """AHMC_TARGET_KERNEL: the iso Gaussian as a user device kernel (tests/user_targets/kernels.hip)"""
    import torch

    from ahmc_amd.build import build_code_object
    from ahmc_amd.hipmod import Module

    mod = Module(build_code_object(os.path.join(ROOT, "tests", "user_targets", "kernels.hip")))
    user = torch.tensor([0.0, 0.0], dtype=torch.float64, device="cuda")
    tg = A.KernelTarget(D, mod.function("iso_gauss_f64"), handle_kind=capi.KERNEL_HIP_FUNCTION, block_threads=256, chains_per_block=4,
                        user=user.data_ptr())
    return tg, (mod, user)


def run_against_restatement(hip, D, k, N, n_trans, name, kind, cfg, seed=11, target="iso"):
    """target: "iso" (built-in), "dense" (AHMC_TARGET_DENSE_GAUSS), "external" (ask / tell, ahmc_ext_*), "kernel" (AHMC_TARGET_KERNEL)"""
    rs = np.random.default_rng(400 + D + k)
    Av, B, Dm = make_ru(D, k, rs, scale=2.0)
    eps = 0.6 * D ** -0.25
    kern, lf = api_kernel(kind, cfg, eps, N)
    keep = None
    if target == "dense":
        G = rs.normal(size=(D, D))
        P = G @ G.T / D + np.eye(D)
        target, fn = A.DenseGaussian(np.asfortranarray(P)), dense_gaussian_fn(P)
    elif target == "external":
        target, fn = A.ExternalTarget(D, iso_gaussian_columns), R.iso_gaussian
    elif target == "kernel":
        (target, keep), fn = kernel_target(D), R.iso_gaussian
    else:
        target, fn = A.IsoGaussian(D), R.iso_gaussian
    e = A.Engine(A.Hamiltonian(A.RankUpdateEuclideanMetric(Av, B, Dm), target), N, rng=A.PhiloxRNG(seed), lib=hip)
    e.set_integrator(lf)
    hr = RUHamiltonian(Av, B, Dm, fn)
    assert keep is None or keep
    cfg = dict(cfg, eps=eps)
    if cfg.get("lam"):
        cfg["L"] = max(1, int(np.floor(cfg["lam"] / eps)))  # nsteps(τ) = max(1, floor(λ / ϵ)) (src/trajectory.jl:241-243)
    th = rs.normal(size=(D, N))
    r = np.zeros((D, N))
    e.set_position(th)
    for it in range(n_trans):
        e.transition(kern)
        z, st = e.phasepoint(), e.stats()
        ref = [ref_transition(hr, kind, cfg, seed, c, it, th[:, c], r[:, c]) for c in range(N)]
        for key in ("n_steps", "is_accept", "numerical_error") + (("tree_depth",) if kind == "nuts" else ()):
            got = st[key].astype(np.int64)
            want = np.asarray([s[key] for _, s in ref], dtype=np.int64)
            np.testing.assert_array_equal(got, want, err_msg=f"{name} D={D} it={it} {key}")
        tw = np.asarray([zz.theta for zz, _ in ref]).T
        rw = np.asarray([zz.r for zz, _ in ref]).T
        np.testing.assert_allclose(z.theta, tw, rtol=1e-10, atol=1e-10, err_msg=f"{name} θ")
        np.testing.assert_allclose(z.r, rw, rtol=1e-10, atol=1e-10, err_msg=f"{name} r")
        np.testing.assert_allclose(z.lp.value, [zz.lp for zz, _ in ref], rtol=1e-10, atol=1e-10, err_msg=f"{name} ℓπ")
        np.testing.assert_allclose(z.lk.value, [zz.lk for zz, _ in ref], rtol=1e-10, atol=1e-10, err_msg=f"{name} ℓκ")
        th, r = tw, rw
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind,cfg", TRANSITIONS, ids=[t[0] for t in TRANSITIONS])
@pytest.mark.parametrize("D,k", [(7, 3), (128, 8)])
def test_transitions_against_restatement(hip, D, k, name, kind, cfg):
    run_against_restatement(hip, D, k, 64, 5, name, kind, cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind,cfg", [TRANSITIONS[1], TRANSITIONS[6], TRANSITIONS[7]], ids=["nuts", "hmc", "hmc_mn"])
def test_dense_target_against_restatement(hip, name, kind, cfg):
    """the dense Gaussian target (g′ = Pθ′ by the GEMM, w′ = M⁻¹g′ by k_ru_apply on the pool points)"""
    run_against_restatement(hip, 24, 4, 32, 4, name, kind, cfg, target="dense")


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind,cfg", [TRANSITIONS[1], TRANSITIONS[4], TRANSITIONS[6], TRANSITIONS[7]], ids=["nuts", "nuts_strict", "hmc", "hmc_mn"])
def test_external_target_against_restatement(hip, name, kind, cfg):
    """ask / tell (ahmc_ext_*: the caller's gradient, then w′ = M⁻¹g′ by k_ru_apply on the listed chains)"""
    run_against_restatement(hip, 24, 4, 32, 3, name, kind, cfg, target="external")


@pytest.mark.gpu
@pytest.mark.parametrize("D,k", [(24, 4), (5000, 8)])
def test_kernel_target_against_restatement(hip, D, k):
    """AHMC_TARGET_KERNEL: the user's device kernel evaluates (ℓπ, g′), k_ru_apply the velocity (D = 5000: a wide context)"""
    run_against_restatement(hip, D, k, 32 if D == 24 else 8, 3, "nuts_kernel", "nuts", TRANSITIONS[1][2], target="kernel")


@pytest.mark.gpu
@pytest.mark.parametrize("D,k,N,n", [(513, 5, 16, 3), (5000, 8, 8, 3)])
def test_default_nuts_against_restatement_large(hip, D, k, N, n):
    run_against_restatement(hip, D, k, N, n, "nuts_default", "nuts", dict(TS=R.MultinomialTS, criterion=R.GENERALISED, max_depth=6))


@pytest.mark.gpu
@pytest.mark.parametrize("D,k", [(7, 3), (128, 8)])
def test_find_good_stepsize(hip, D, k):
    rs = np.random.default_rng(500 + D)
    Av, B, Dm = make_ru(D, k, rs, scale=2.0)
    N, seed = 16, 13
    e = A.Engine(A.Hamiltonian(A.RankUpdateEuclideanMetric(Av, B, Dm), A.IsoGaussian(D)), N, rng=A.PhiloxRNG(seed), lib=hip)
    th = rs.normal(size=(D, N))
    e.set_position(th)
    got = e.find_good_stepsize(0.1, 100)
    hr = RUHamiltonian(Av, B, Dm, R.iso_gaussian)
    want = [ref_find_good_stepsize(seed, c, 0, hr, th[:, c]) for c in range(N)]
    np.testing.assert_array_equal(got, want)
    e.close()


# ---- usefulness: a target whose covariance is a rank-4 update of I ----
def spiked_gaussian(D, k, lam_max, rs, a=1e-3):
    U, _ = np.linalg.qr(rs.normal(size=(D, k)))
    lam = np.geomspace(lam_max / 8, lam_max, k)
    Sigma = a * np.eye(D) + U @ np.diag(lam) @ U.T
    return U, lam, Sigma


@pytest.mark.gpu
def test_usefulness_and_sample_equals_stepwise(hip):
    """Dense Gaussian with Σ = a·I + U·diag(λ)·Uᵀ at D = 256, k = 4, λ up to 400, a = 10⁻³, M⁻¹ = Σ as a rank update: StepSizeAdaptor
    and 4 096 chains; the mean within 5 MCSE of 0 (Engine.summarystats), the mean tree depth at least 1 below the Unit metric's; and
    ahmc_sample equal, bit for bit, to the stepwise loop of transition + adapt.  (With a = 1 the 252 unit directions decide the U-turn
    for either metric and the trees are as deep: measured 5.8 against 6.1, and DenseEuclideanMetric(Σ) 5.8; at a = 0.01 6.5 against
    7.5; at a = 10⁻³ 6.5 against 8.0, short of the 2 levels first asked for — DESIGN §13.)"""
    D, k, N = 256, 4, 4096
    rs = np.random.default_rng(600)
    U, lam, Sigma = spiked_gaussian(D, k, 400.0, rs)
    P = np.asfortranarray(np.linalg.inv(Sigma))
    n_adapts, n_samples = 150, 250
    import torch

    depth = {}
    for metric in ("ru", "unit"):
        m = A.RankUpdateEuclideanMetric(np.full(D, 1e-3), U, np.diag(lam)) if metric == "ru" else A.UnitEuclideanMetric((D, N))
        e = A.Engine(A.Hamiltonian(m, A.DenseGaussian(P)), N, rng=A.PhiloxRNG(21), lib=hip)
        kern = A.HMCKernel(A.Trajectory(A.MultinomialTS, A.Leapfrog(np.full(N, 0.1)), A.GeneralisedNoUTurn(max_depth=10)))
        e.set_integrator(kern.tau.integrator)
        e.set_position(rs.normal(size=(D, N)) * 0.1)
        e.adaptor_init(A.StepSizeAdaptor(0.8, kern.tau.integrator))
        draws = torch.empty((n_samples - n_adapts, N, D), dtype=torch.float64, device="cuda")
        e.run(kern, n_samples, n_adapts=n_adapts, drop_warmup=True, samples_out=draws.data_ptr())
        e.sync()
        depth[metric] = e.stats()["tree_depth"].mean()
        if metric == "ru":
            st = e.summarystats(draws.data_ptr(), n_samples - n_adapts)
            assert np.all(np.abs(st["mean"]) < 5 * st["mcse"]), np.max(np.abs(st["mean"]) / st["mcse"])
        e.close()
    assert depth["ru"] <= depth["unit"] - 1, depth

    # ahmc_sample == stepwise transition + adapt!, bit for bit (a smaller run)
    Ns, ns, na = 64, 40, 20
    outs = []
    for mode in ("bulk", "step"):
        e = A.Engine(A.Hamiltonian(A.RankUpdateEuclideanMetric(np.full(D, 1e-3), U, np.diag(lam)), A.DenseGaussian(P)), Ns, rng=A.PhiloxRNG(3), lib=hip)
        kern = A.HMCKernel(A.Trajectory(A.MultinomialTS, A.Leapfrog(np.full(Ns, 0.1)), A.GeneralisedNoUTurn(max_depth=8)))
        e.set_integrator(kern.tau.integrator)
        e.set_position(np.random.default_rng(1).normal(size=(D, Ns)) * 0.1)
        e.adaptor_init(A.StepSizeAdaptor(0.8, kern.tau.integrator))
        if mode == "bulk":
            e.run(kern, ns, n_adapts=na)
        else:
            for i in range(1, ns + 1):
                e.transition(kern)
                e.adapt(i, na)
        outs.append((e.theta(), e.get_stepsize()))
        e.close()
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])


# ---- invariances, bit for bit ----
def nuts_kernel(N, eps=0.3):
    return A.HMCKernel(A.Trajectory(A.MultinomialTS, A.Leapfrog(np.full(N, eps)), A.GeneralisedNoUTurn(max_depth=8)))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [33, 5000])
def test_chain_split_and_checkpoint(hip, D):
    """one engine of N chains == two engines of N/2 with chain_offset; get_state → set_state on a fresh engine == uninterrupted"""
    rs = np.random.default_rng(700 + D)
    Av, B, Dm = make_ru(D, 6, rs, scale=2.0)
    N = 16
    th = rs.normal(size=(D, N))
    h = A.Hamiltonian(A.RankUpdateEuclideanMetric(Av, B, Dm), A.Funnel(D))
    kern = nuts_kernel(N, 0.1 * D ** -0.25)

    def engine(n, off):
        e = A.Engine(h, n, rng=A.PhiloxRNG(17, chain_offset=off), lib=hip)
        e.set_integrator(A.Leapfrog(np.full(n, 0.1 * D ** -0.25)))
        return e

    whole = engine(N, 0)
    whole.set_position(th)
    whole.run(kern, 4)
    halves = []
    for lo in (0, N // 2):
        e = engine(N // 2, lo)
        e.set_position(th[:, lo:lo + N // 2])
        e.run(A.HMCKernel(A.Trajectory(A.MultinomialTS, A.Leapfrog(np.full(N // 2, 0.1 * D ** -0.25)), A.GeneralisedNoUTurn(max_depth=8))), 4)
        halves.append(e.theta())
        e.close()
    np.testing.assert_array_equal(whole.theta(), np.concatenate(halves, axis=1))
    # checkpoint after 4 iterations, resume for 3 more on a fresh engine, against 7 uninterrupted
    st = whole.get_state()
    assert st["metric_kind"] == capi.METRIC_RANK_UPDATE
    whole.run(kern, 7, i_first=5)
    fresh = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((D, N)), A.Funnel(D)), N, rng=A.PhiloxRNG(17), lib=hip)
    fresh.set_integrator(A.Leapfrog(np.full(N, 0.1 * D ** -0.25)))
    fresh.set_state(st)
    fresh.run(kern, 7, i_first=5)
    np.testing.assert_array_equal(whole.theta(), fresh.theta())
    whole.close()
    fresh.close()


@pytest.mark.gpu
def test_rank_update_then_diag_is_a_fresh_diag_context(hip):
    """set the rank-update metric, run, then a Diag metric: bit-equal to a fresh Diag context (the fused path) — nothing is left behind"""
    D, N = 20, 128
    rs = np.random.default_rng(800)
    Av, B, Dm = make_ru(D, 4, rs)
    minv = 0.5 + rs.random(D)
    th = rs.normal(size=(D, N))
    kern = nuts_kernel(N)
    a = A.Engine(A.Hamiltonian(A.RankUpdateEuclideanMetric(Av, B, Dm), A.IsoGaussian(D)), N, rng=A.PhiloxRNG(4), lib=hip)
    a.set_integrator(kern.tau.integrator)
    a.set_position(th)
    a.transition(kern)
    a.set_metric(A.DiagEuclideanMetric(minv))
    a.seed(A.PhiloxRNG(4))
    a.set_position(th)
    b = A.Engine(A.Hamiltonian(A.DiagEuclideanMetric(minv), A.IsoGaussian(D)), N, rng=A.PhiloxRNG(4), lib=hip)
    b.set_integrator(kern.tau.integrator)
    b.set_position(th)
    for e in (a, b):
        e.transition(kern)
        e.transition(kern)
    np.testing.assert_array_equal(a.theta(), b.theta())
    for key in ("n_steps", "tree_depth"):
        np.testing.assert_array_equal(a.stats()[key], b.stats()[key])
    a.close()
    b.close()


# ---- refusals ----
@pytest.mark.gpu
def test_refusals(hip):
    D, N = 8, 4
    rs = np.random.default_rng(900)
    Av, B, Dm = make_ru(D, 3, rs)
    e = ru_engine(hip, D, N, Av, B, Dm)
    e.set_position(rs.normal(size=(D, N)))
    for code in (capi.ADAPT_MASSMATRIX, capi.ADAPT_NAIVE, capi.ADAPT_STAN):
        with pytest.raises(A.UnsupportedError, match="RankUpdateEuclideanMetric"):
            e._call("ahmc_adaptor_init", code, 0.8, 75, 50, 25)
    for call in (lambda: e._call("ahmc_lf_pre", 1, 1, 1), lambda: e._call("ahmc_lf_post", 1, 1, 1, capi.as_ptr(np.zeros(N)), capi.as_ptr(np.zeros((D, N))))):
        with pytest.raises(A.UnsupportedError, match="RankUpdateEuclideanMetric"):
            call()
    with pytest.raises(A.ArgumentError, match="ahmc_get_metric_rank_update"):
        e._call("ahmc_get_metric", capi.as_ptr(np.zeros(D)), D)
    e.set_ref_compat(True)
    with pytest.raises(A.UnsupportedError, match="ref_compat"):
        e.step(1)
    e.set_ref_compat(False)
    big = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((40, N)), A.IsoGaussian(40)), N, lib=hip)
    with pytest.raises(A.UnsupportedError, match="AHMC_RANK_UPDATE_MAX_K"):
        big._set_rank_update(np.ones(40), np.zeros((40, 33)), np.eye(33))
    big.close()
    with pytest.raises(A.ArgumentError, match="DomainError"):
        e._set_rank_update(-np.ones(D), B, Dm)
    with pytest.raises(A.ArgumentError, match="DimensionMismatch"):
        e._call("ahmc_set_metric_rank_update", None, capi.as_ptr(np.zeros((D, D + 1))), capi.as_ptr(np.eye(D + 1)), D + 1)
    with pytest.raises(A.ArgumentError, match="PosDefException"):
        e._set_rank_update(Av, B, -50 * np.eye(3))
    # after every refusal the context still samples with the metric it had
    e.set_position(rs.normal(size=(D, N)))
    e.transition(nuts_kernel(N))
    assert np.all(np.isfinite(e.theta()))
    e.close()
    # a mass-matrix adaptor set up under another metric is refused once the metric is a rank update: by ahmc_sample and by ahmc_adapt
    kern = nuts_kernel(N)
    for code in (capi.ADAPT_MASSMATRIX, capi.ADAPT_NAIVE, capi.ADAPT_STAN):
        d = A.Engine(A.Hamiltonian(A.DiagEuclideanMetric(Av), A.IsoGaussian(D)), N, rng=3, lib=hip)
        d.set_integrator(kern.tau.integrator)
        d.set_position(rs.normal(size=(D, N)))
        d._call("ahmc_adaptor_init", code, 0.8, 75, 50, 25)
        d._set_rank_update(Av, B, Dm)
        d.transition(kern)
        with pytest.raises(A.UnsupportedError, match="RankUpdateEuclideanMetric"):
            d.adapt(1, 10)
        with pytest.raises(A.UnsupportedError, match="RankUpdateEuclideanMetric"):
            d.run(kern, 5, n_adapts=3)
        d.close()
