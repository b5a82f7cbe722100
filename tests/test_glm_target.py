"""GLMTarget (include/ahmc_glm.h): regression log-densities evaluated for all chains at once, X·Θ and Xᵀ·U on the MFMA units
(csrc/ahmc_glm.hpp); the arithmetic is defined by advancedhmc.jl_amd/glm.py.

CPU: the mirror (gradient against central differences in long double, η = ±800, an overflowing Poisson, prior and offset present /
absent); header == binding table == Julia ccalls == exported symbols; every kernel instantiation present and scratch-free; the CPU
checker's refusal; the planted defect (the bounds of §1 applied to a host emulation, right and with one wrong sign); the parity
test's precondition on the oracle alone.

GPU:
 §1 values.  η read back through ahmc_glm_pointwise equals the k-ordered fma chain (tests/host_ref/glm_ref.cpp) bit for bit; the
    gradient product launched alone (tests/device_probe/glm.hip) equals its chain-per-slice model bit for bit; the pointwise ℓ, ℓπ
    and g through the C ABI lie inside bounds derived below from a long-double evaluation of the values as stored.
 §2 invariances, bit for bit: chain blocks, tile shape, re-binding, checkpoint / resume, bulk == stepwise.
 §3 parity with the oracle running the mirror as a host kernel: every chain, exactly.
 §4 a posterior, against the same model through ask / tell.
 §5 every refusal of the header.

The bounds of §1 (u the unit roundoff of the element type, γ_k = k·u/(1 − k·u), S = |X|·|θ| the companion of the product; the
long-double reference's own γ⁶⁴ terms are added everywhere and not repeated here):
    Δη  = γ_D·S + u·|η̂|                                  any order of the D products, then the one addition of the offset
    ℓ̂ − ℓ(η) ≤ L_ℓ·Δη + R_ℓ,   û − u(η) ≤ L_u·Δη + R_u     Lipschitz constant of the link between η and η̂, plus the epilogue's roundings:
      logit     L_ℓ = 1, L_u = ¼;  R_ℓ = log1p(e)·(ε_exp + ε_log1p) + u·softplus + u·|ℓ|   (e = exp(−|η̂|); the condition number of log1p
                with respect to e is ≤ 1; one rounding of max(η, 0) + log1p, one of the fma);  R_u = σ·(2ε_exp + 2u) + u·|u|
      Poisson   L_ℓ = y + exp(η̂ + Δη), L_u = exp(η̂ + Δη);  R_ℓ = ε_exp·exp(η̂) + u·|ℓ|;  R_u = ε_exp·exp(η̂) + u·|u|
      Gaussian  L_ℓ = scale·(|r| + Δη), L_u = scale;  R_ℓ = 4u·|ℓ| (r, scale·r, ·r: the −½ is exact);  R_u = 2u·|u|
    ε_exp, ε_log1p are twice the worst relative error of the device's exp on [−ETA_MAX, ETA_MAX] and log1p on [0, 1], measured by a
    one-kernel probe against long double (the cases assert |η̂| ≤ ETA_MAX).
    ĝ − g ≤ |X|ᵀ·E_u + γ_{n_obs+1}·|X|ᵀ(|u| + E_u) + u·|ĝ|      E_u the bound on û; any order of the n_obs products, slices or not; one fma
    ℓπ̂ − ℓπ ≤ Σ E_ℓ + γ_{n_obs}·Σ(|ℓ| + E_ℓ) + ½·γ_{D+1}·Σ p θ² + u·|ℓπ̂|
Products of two of these first-order terms are below 10⁻⁴ of them at the sizes used (γ_1030 in Float32 is 6·10⁻⁵): SLACK = 1.01.
Every error / bound is recorded in glm_margins.json under $AHMC_TEST_OUT (default test_out/); profiles/glm_margins.json is the
MI355X run.
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
from ahmc_amd import _capi as capi
from ahmc_amd import glm as G

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_REF = os.path.join(ROOT, "tests", "host_ref", "glm_ref.cpp")
PROBE = os.path.join(ROOT, "tests", "device_probe", "glm.hip")
U = {np.dtype(np.float64): LD(2) ** -53, np.dtype(np.float32): LD(2) ** -24}
U_LD = LD(2) ** -64
TCH = {np.dtype(np.float64): "d", np.dtype(np.float32): "f"}
SLACK = LD("1.01")
ETA_MAX = 16.0
FAMS = ("bernoulli_logit", "poisson_log", "gaussian_identity")
DTYPES = (np.float64, np.float32)
# every n_obs of {1, 5, 63, 64, 65, 130, 1030 (past one K slice)}, D of {1, 3, 16, 17, 65, 200}, N of {1, 17, 70, 130}
SHAPES = ((1, 1, 1), (5, 3, 17), (63, 16, 70), (64, 17, 130), (65, 65, 1), (130, 200, 17), (1030, 3, 70), (1030, 200, 130), (64, 1, 130),
          (5, 65, 70), (130, 16, 1), (63, 200, 17), (1030, 17, 17), (65, 3, 130))
NULL = C.c_void_p(None)
MARGINS = {}


def gam(k, u):
    k = LD(k)
    assert k * u < 0.5
    return k * u / (1 - k * u)


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
        with open(os.path.join(out, "glm_margins.json"), "w") as f:
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
    if worst > 1.0:
        ij = np.unravel_index(int(np.argmax(frac)), frac.shape)
        raise AssertionError(f"{key}: error {float(err[ij]):.3e} is {worst:.3g} × its bound {float(bound[ij]):.3e} at element {ij}")
    return worst


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def record_bits(key, got, want):
    """elements of `got` whose value differs from `want` (±0 are one value, any NaN equals any NaN), kept under `key`; asserts there are none"""
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
# the references
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_lib():
    """tests/host_ref/glm_ref.cpp as its own shared object in the build cache, by the host compiler"""
    from ahmc_amd import build as B

    flags = ["-O2", "-march=native", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-ffp-contract=off"]
    with open(HOST_REF, "rb") as f:
        h = hashlib.sha256(f.read() + " ".join(flags).encode()).hexdigest()[:20]
    out_dir = os.path.join(B.OBJ, "host_ref")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, f"glm_ref_{h}.so")
    if not os.path.exists(so):
        cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
        tmp = so + f".tmp{os.getpid()}"
        res = subprocess.run([cxx, *flags, HOST_REF, "-o", tmp], capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"host reference build failed:\n{res.stdout}\n{res.stderr}")
        os.replace(tmp, so)
    dll = C.CDLL(so)
    for name in ("fma_f64", "fma_f32", "chain_f64", "chain_f32", "exact_f64", "exact_f32"):
        getattr(dll, name).restype = None
    return dll


def _sfx(dtype):
    return "f64" if np.dtype(dtype) == np.float64 else "f32"


def _p(a):
    return C.c_void_p(a.ctypes.data)


def host_fma(a, b, c):
    dt = a.dtype
    a, b, c = (np.ascontiguousarray(np.broadcast_to(x, np.broadcast_shapes(a.shape, b.shape, c.shape)), dtype=dt) for x in (a, b, c))
    out = np.empty_like(a)
    getattr(ref_lib(), "fma_" + _sfx(dt))(_p(a), _p(b), _p(c), _p(out), C.c_int64(a.size))
    return out


def chain(Am, X, k0=0, k1=None):
    """Y (M, n) = A[:, k0:k1]·X[k0:k1] as the k-ordered fma chain of the element type; A (M, K) and X (K, n) column-major"""
    dtype = Am.dtype
    Am, X = np.asfortranarray(Am), np.asfortranarray(X, dtype=dtype)
    M, K = Am.shape
    assert X.shape[0] == K
    n = X.shape[1]
    Y = np.empty((M, n), dtype=dtype, order="F")
    getattr(ref_lib(), "chain_" + _sfx(dtype))(_p(Am), _p(X), _p(Y), C.c_int64(M), C.c_int64(n), C.c_int64(M), C.c_int64(K), C.c_int64(k0),
                                               C.c_int64(K if k1 is None else k1))
    return Y


def exact(Am, X):
    """(A·X, |A|·|X|) in 80-bit long double of the values as stored: A in its element type, X in long double"""
    dtype = Am.dtype
    Am, X = np.asfortranarray(Am), np.asfortranarray(X, dtype=LD)
    M, K = Am.shape
    n = X.shape[1]
    Y, S = np.empty((M, n), dtype=LD, order="F"), np.empty((M, n), dtype=LD, order="F")
    getattr(ref_lib(), "exact_" + _sfx(dtype))(_p(Am), _p(X), _p(Y), _p(S), C.c_int64(M), C.c_int64(n), C.c_int64(M), C.c_int64(K), C.c_int64(0), C.c_int64(K))
    return Y, S


def link_ld(fam, y, eta, scale):
    """(ℓ, u) in long double"""
    y, eta = np.asarray(y, dtype=LD), np.asarray(eta, dtype=LD)
    if fam == G.BERNOULLI_LOGIT:
        e = np.exp(-np.abs(eta))
        sig = np.where(eta >= 0, 1 / (1 + e), e / (1 + e))
        return y * eta - (np.maximum(eta, 0) + np.log1p(e)), y - sig
    if fam == G.POISSON_LOG:
        return y * eta - np.exp(eta), y - np.exp(eta)
    r = y - eta
    return -LD(scale) * r * r / 2, LD(scale) * r


def grad_model(Xt, Um, prec, th):
    """the bit-level model of g: a k-ordered chain per slice of K_SLICE observations, the slice sums added in ascending order, then
    fma(p, θ, −Σ);  Xt (D, n_obs), Um (n_obs, n), th (D, n)"""
    n_obs = Xt.shape[1]
    s = None
    for k0 in range(0, n_obs, G.K_SLICE):
        part = chain(Xt, Um, k0, min(n_obs, k0 + G.K_SLICE))
        s = part if s is None else s + part
    return host_fma(np.ascontiguousarray(prec.reshape(-1, 1)), np.asarray(th, dtype=Xt.dtype), -s)


@functools.lru_cache(maxsize=None)
def case(n_obs, D, N, fam, dtname):
    """operands and references of one §1 case, computed once"""
    dtype = np.dtype(dtname)
    rs = np.random.default_rng([n_obs, D, N, fam, dtype.itemsize])
    X = np.asfortranarray(rs.normal(size=(n_obs, D)) / np.sqrt(D), dtype=dtype)
    th = np.asfortranarray(1.5 * rs.normal(size=(D, N)), dtype=dtype)
    off = (0.3 * rs.normal(size=n_obs)).astype(dtype)
    if fam == G.BERNOULLI_LOGIT:
        y = np.where(np.arange(n_obs) % 3 == 2, rs.random(n_obs), (rs.random(n_obs) < 0.5).astype(np.float64)).astype(dtype)
    elif fam == G.POISSON_LOG:
        y = rs.poisson(3.0, size=n_obs).astype(dtype)
    else:
        y = rs.normal(size=n_obs).astype(dtype)
    p = (2 * rs.random(D)).astype(dtype)
    p[::3] = 0
    scale = 1.7
    u = U[dtype]
    E, S = exact(X, th)
    eta_hat = chain(X, th) + off.reshape(-1, 1)            # (the one addition of the offset, correctly rounded in the element type)
    eta = E + off.astype(LD).reshape(-1, 1)
    d_eta = (gam(D, u) + gam(D + 1, U_LD)) * S + (u + U_LD) * np.abs(eta_hat.astype(LD))
    assert np.abs(eta_hat).max() <= ETA_MAX
    ll, uu = link_ld(fam, y.reshape(-1, 1), eta, float(dtype.type(scale)))
    Xt = np.asfortranarray(X.T)
    Gx, Sg = exact(Xt, uu)
    pth = p.astype(LD).reshape(-1, 1) * th.astype(LD)
    return {"X": X, "Xt": Xt, "y": y, "off": off, "p": p, "th": th, "scale": scale, "fam": fam, "dtype": dtype, "eta_hat": eta_hat, "eta": eta,
            "d_eta": d_eta, "ll": ll, "u": uu, "Sg": Sg, "g": -Gx + pth, "lp": ll.sum(axis=0) - (pth * th.astype(LD)).sum(axis=0) / 2,
            "prior": (pth * th.astype(LD)).sum(axis=0)}


def link_bounds(c, eps):
    """(E_ℓ, E_u): the bounds of the module docstring on the device's ℓ̂ and û, element by element"""
    fam, u = c["fam"], U[c["dtype"]]
    eh, de = c["eta_hat"].astype(LD), c["d_eta"]
    y = c["y"].astype(LD).reshape(-1, 1)
    sc = LD(float(c["dtype"].type(c["scale"])))
    ll, uu = np.abs(c["ll"]), np.abs(c["u"])
    ee, el = LD(eps["exp"]), LD(eps["log1p"])
    if fam == G.BERNOULLI_LOGIT:
        e = np.exp(-np.abs(eh))
        l1p = np.log1p(e)
        sig = np.where(eh >= 0, 1 / (1 + e), e / (1 + e))
        El = de + l1p * (ee + el) + u * (np.maximum(eh, 0) + l1p) + u * ll
        Eu = de / 4 + sig * (2 * ee + 2 * u) + u * uu
    elif fam == G.POISSON_LOG:
        ex, exd = np.exp(eh), np.exp(eh + de)
        El = (y + exd) * de + ee * ex + u * ll
        Eu = exd * de + ee * ex + u * uu
    else:
        r = np.abs(y - eh)
        El = sc * (r + de) * de + 4 * u * ll
        Eu = sc * de + 2 * u * uu
    ld = 8 * U_LD * (ll + uu + 1)
    return SLACK * El + ld, SLACK * Eu + ld


def check_case(key, c, eps, eta=None, ll=None, lp=None, g=None):
    """the assertions of §1 on whatever results are given (the device's, or a host emulation's)"""
    n_obs, D = c["X"].shape
    u = U[c["dtype"]]
    El, Eu = link_bounds(c, eps)
    if eta is not None:
        record_bits(f"eta {key}", eta, c["eta_hat"])
    if ll is not None:
        record_bound(f"loglik {key}", np.abs(ll.astype(LD) - c["ll"]), El)
    if lp is not None:
        b = El.sum(axis=0) + (gam(n_obs, u) + gam(n_obs, U_LD)) * (np.abs(c["ll"]) + El).sum(axis=0) + gam(D + 1, u) * c["prior"] / 2 + u * np.abs(lp.astype(LD))
        record_bound(f"lp {key}", np.abs(lp.astype(LD) - c["lp"]), SLACK * b)
    if g is not None:
        XE = np.abs(c["Xt"]).astype(LD) @ Eu
        b = XE + (gam(n_obs + 1, u) + gam(n_obs + 1, U_LD)) * (c["Sg"] + XE) + u * np.abs(g.astype(LD)) + 4 * U_LD * np.abs(c["g"])
        record_bound(f"grad {key}", np.abs(g.astype(LD) - c["g"]), SLACK * b)


def emulate(c, sign=1.0):
    """the device's arithmetic on the host in the element type, numpy's functions for the device's (`sign` = −1 plants the defect: the
    data term of g with the wrong sign)"""
    dt = c["dtype"].type
    eh = c["eta_hat"]
    y = c["y"].reshape(-1, 1)
    with np.errstate(over="ignore"):
        if c["fam"] == G.BERNOULLI_LOGIT:
            e = np.exp(-np.abs(eh))
            sp = np.where(eh > 0, eh, dt(0)) + np.log1p(e)
            d = dt(1) + e
            ll, uu = host_fma(y, eh, -sp), y - np.where(eh >= 0, dt(1) / d, e / d)
        elif c["fam"] == G.POISSON_LOG:
            ex = np.exp(eh)
            ll, uu = host_fma(y, eh, -ex), y - ex
        else:
            r = y - eh
            uu = dt(c["scale"]) * r
            ll = (dt(-0.5) * uu) * r
    assert ll.dtype == c["dtype"] and uu.dtype == c["dtype"]
    s = chain(c["Xt"], uu)
    g = host_fma(c["p"].reshape(-1, 1), c["th"], dt(-sign) * s)
    lp = ll.sum(axis=0, dtype=c["dtype"]) - (c["p"].reshape(-1, 1) * c["th"] * c["th"]).sum(axis=0, dtype=c["dtype"]) / dt(2)
    return ll, uu, lp.astype(c["dtype"]), g


def function_eps(exp_fn, log1p_fn, dtype, n=200001):
    """twice the worst relative error of exp on [−ETA_MAX, ETA_MAX] and log1p on [0, 1] against long double, and the worst in ulps"""
    dtype = np.dtype(dtype)
    x = np.concatenate([np.linspace(-ETA_MAX, ETA_MAX, n), np.random.default_rng(1).uniform(-ETA_MAX, ETA_MAX, n)]).astype(dtype)
    z = np.concatenate([np.linspace(0.0, 1.0, n), np.exp(-np.abs(x.astype(np.float64)))]).astype(dtype)
    e, l = np.asarray(exp_fn(x)), np.asarray(log1p_fn(z))
    assert e.dtype == dtype and l.dtype == dtype
    re = np.abs(e.astype(LD) - np.exp(x.astype(LD))) / np.exp(x.astype(LD))
    ref = np.log1p(z.astype(LD))
    rl = np.where(ref > 0, np.abs(l.astype(LD) - ref) / np.where(ref > 0, ref, 1), np.abs(l.astype(LD)))
    u = U[dtype]
    out = {"exp": float(2 * re.max()), "log1p": float(2 * rl.max()), "exp_worst_u": float(re.max() / u), "log1p_worst_u": float(rl.max() / u)}
    assert out["exp_worst_u"] < 16 and out["log1p_worst_u"] < 16, out  # (a function this far off is a finding of its own, not a margin)
    return out


# ------------------------------------------------------------------------------------------------
# CPU: the mirror
# ------------------------------------------------------------------------------------------------
def small_model(fam, rs, n_obs=23, D=4, N=3, offset=True, prior=True):
    X = rs.normal(size=(n_obs, D)) / 2
    th = rs.normal(size=(D, N))
    if fam == G.BERNOULLI_LOGIT:
        y = np.where(np.arange(n_obs) % 2 == 0, (rs.random(n_obs) < 0.5).astype(float), rs.random(n_obs))
    elif fam == G.POISSON_LOG:
        y = rs.poisson(2.0, size=n_obs).astype(float)
    else:
        y = rs.normal(size=n_obs)
    return X, y, th, (0.2 * rs.normal(size=n_obs) if offset else None), (0.5 + rs.random(D) if prior else None), 1.3


@pytest.mark.parametrize("fam", [0, 1, 2], ids=FAMS)
@pytest.mark.parametrize("offset,prior", [(True, True), (False, False), (True, False)])
def test_mirror_gradient_against_central_differences(fam, offset, prior):
    """∇ℓπ of the mirror against central differences of a long-double evaluation of ℓπ (h = 1e-6: truncation h²·|ℓπ‴|/6 ≈ 1e-11)"""
    rs = np.random.default_rng(11 + fam)
    X, y, th, off, p, scale = small_model(fam, rs, offset=offset, prior=prior)

    def lp_ld(t):
        eta = X.astype(LD) @ t + (0 if off is None else off.astype(LD).reshape(-1, 1))
        ll, _ = link_ld(fam, y.reshape(-1, 1), eta, scale)
        return ll.sum(axis=0) - (0 if p is None else (p.astype(LD).reshape(-1, 1) * t * t).sum(axis=0) / 2)

    lp, grad = G.logdensity(FAMS[fam], X, y, th, off, p, scale)
    np.testing.assert_allclose(lp, lp_ld(th.astype(LD)).astype(np.float64), rtol=1e-13, atol=1e-13)
    h = LD("1e-6")
    for d in range(X.shape[1]):
        tp, tm = th.astype(LD), th.astype(LD)
        tp[d] += h
        tm[d] -= h
        fd = ((lp_ld(tp) - lp_ld(tm)) / (2 * h)).astype(np.float64)
        np.testing.assert_allclose(grad[d], fd, rtol=1e-8, atol=1e-8)
    eta, ll = G.pointwise(FAMS[fam], X, y, th, off, scale)
    np.testing.assert_allclose(eta, X @ th + (0 if off is None else off.reshape(-1, 1)), rtol=1e-14, atol=1e-14)
    np.testing.assert_allclose(ll.sum(axis=0) - (0 if p is None else (p.reshape(-1, 1) * th * th).sum(axis=0) / 2), lp, rtol=1e-13, atol=1e-13)
    # a vector θ is one chain
    lp1, g1 = G.logdensity(fam, X, y, th[:, 0], off, p, scale)
    np.testing.assert_allclose(lp1[0], lp[0], rtol=1e-14)
    np.testing.assert_allclose(g1[:, 0], grad[:, 0], rtol=1e-13, atol=1e-14)


def test_mirror_extremes():
    """logit: finite at η = ±800 with the right limits; Poisson: an overflowing exp is non-finite and sanitises to −Inf"""
    X = np.array([[800.0], [-800.0], [800.0], [-800.0]])
    y = np.array([1.0, 1.0, 0.0, 0.0])
    lp, g = G.logdensity("bernoulli_logit", X, y, np.array([[1.0]]))
    assert np.isfinite(lp).all() and np.isfinite(g).all()
    np.testing.assert_allclose(lp, [-1600.0], rtol=1e-15)          # ℓ = 0, −800, −800, 0
    np.testing.assert_allclose(g, [[800.0 * 0 - 800.0 * 1 + 800.0 * -1 - 800.0 * 0]], rtol=1e-15)  # u = y − σ = 0, 1, −1, 0
    eta, ll = G.pointwise("bernoulli_logit", X, y, np.array([[1.0]]))
    np.testing.assert_allclose(ll[:, 0], [0.0, -800.0, -800.0, 0.0], atol=1e-300)
    lp, g = G.logdensity("poisson_log", np.array([[800.0], [1.0]]), np.array([3.0, 1.0]), np.array([[1.0, 0.1]]))
    assert not np.isfinite(lp[0]) and np.isfinite(lp[1])
    assert G.sanitize(lp)[0] == -np.inf and G.sanitize(lp)[1] == lp[1]
    with pytest.raises(ValueError, match="unknown GLM family"):
        G.logdensity("probit", X, y, np.array([[1.0]]))


def test_glmtarget_constructor():
    rs = np.random.default_rng(2)
    X, y = rs.normal(size=(9, 3)), (rs.random(9) < 0.5).astype(float)
    t = A.GLMTarget(X, y, prior_scale=2.0)
    assert t.D == 3 and t.n_obs == 9 and t.family == G.BERNOULLI_LOGIT and t.kind == capi.TARGET_GLM
    np.testing.assert_allclose(t.prior_prec, np.full(3, 0.25))
    assert A.GLMTarget(X, y, family="poisson_log").prior_prec is None
    lp, g = t.logdensity(np.zeros((3, 2)))
    np.testing.assert_allclose(lp, np.full(2, -9 * np.log(2.0)))
    A.Hamiltonian(A.UnitEuclideanMetric(3), t)
    for bad in (lambda: A.GLMTarget(X, y[:-1]), lambda: A.GLMTarget(X, y, family="probit"), lambda: A.GLMTarget(X, y, prior_scale=1.0, prior_prec=1.0),
                lambda: A.GLMTarget(X, y, offset=np.zeros(4)), lambda: A.GLMTarget(X[:, 0], y)):
        with pytest.raises(A.ArgumentError):
            bad()


# ------------------------------------------------------------------------------------------------
# CPU: header, bindings, Julia, the shipped kernels, the checker
# ------------------------------------------------------------------------------------------------
def header_prototypes():
    src = open(os.path.join(ROOT, "include", "ahmc_glm.h"), encoding="utf-8").read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(int32_t)\s+(ahmc_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        params = " ".join(m.group(3).split())
        protos[m.group(2)] = [] if params in ("", "void") else [p.strip() for p in params.split(",")]
    return protos, src


def test_header_and_bindings_agree():
    protos, src = header_prototypes()
    assert set(protos) == set(capi.GLM_SIGNATURES) and len(protos) == 4
    ct = {"int64_t*": C.POINTER(C.c_int64), "int32_t*": C.POINTER(C.c_int32), "double*": C.POINTER(C.c_double), "int64_t": C.c_int64,
          "int32_t": C.c_int32, "double": C.c_double}
    for name, params in protos.items():
        res, args = capi.GLM_SIGNATURES[name]
        assert res is C.c_int32 and len(args) == len(params), name
        for p, a in zip(params, args):
            typ = p.rsplit(" ", 1)[0].replace("const ", "").replace(" ", "")
            if typ in ("void*", "ahmc_ctx*"):
                assert a is C.c_void_p, (name, p)
            else:
                assert a is ct[typ], (name, p)
    assert re.search(r"#define AHMC_GLM_VERSION (\d+)", src).group(1) == str(capi.AHMC_GLM_VERSION)
    assert re.search(r"#define AHMC_TARGET_GLM (\d+)", src).group(1) == str(capi.TARGET_GLM) == "8"
    m = re.search(r"enum \{ AHMC_GLM_BERNOULLI_LOGIT = (\d+), AHMC_GLM_POISSON_LOG = (\d+), AHMC_GLM_GAUSSIAN_IDENTITY = (\d+) \}", src)
    assert tuple(int(x) for x in m.groups()) == (capi.GLM_BERNOULLI_LOGIT, capi.GLM_POISSON_LOG, capi.GLM_GAUSSIAN_IDENTITY) == (G.BERNOULLI_LOGIT, G.POISSON_LOG, G.GAUSSIAN_IDENTITY)
    hip_h = open(os.path.join(ROOT, "include", "ahmc_hip.h"), encoding="utf-8").read()
    assert "glm" not in hip_h.lower()  # (kept out of ahmc_hip.h and AHMC_ABI_VERSION)
    assert re.search(r"#define AHMC_ABI_VERSION (\d+)", hip_h).group(1) == "6"
    # the K-slice constant is one number in the kernels and in the mirror
    dev = open(os.path.join(ROOT, "advancedhmc.jl_amd", "csrc", "ahmc_glm.hpp"), encoding="utf-8").read()
    assert int(re.search(r"constexpr int GLM_K_SLICE = (\d+);", dev).group(1)) == G.K_SLICE
    dense = open(os.path.join(ROOT, "advancedhmc.jl_amd", "csrc", "ahmc_dense.hpp"), encoding="utf-8").read()
    assert int(re.search(r"constexpr int GB_M = (\d+)", dense).group(1)) == G.ROW_BLOCK


def test_julia_ccalls_match_the_header():
    protos, _ = header_prototypes()
    src = open(os.path.join(ROOT, "julia", "AdvancedHMCMI355XGLM.jl"), encoding="utf-8").read()
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
                assert {"int64_t": "Int64", "int32_t": "Cint", "double": "Cdouble"}[p.split()[0]] == t, (name, t, p)
    assert seen == set(protos)
    ext = open(os.path.join(ROOT, "julia", "AdvancedHMCMI355XExt.jl"), encoding="utf-8").read()
    assert 'include("AdvancedHMCMI355XGLM.jl")' in ext and "ahmc_set_target_glm" not in ext


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="needs llvm-objdump")
def test_library_exports_and_kernels_without_scratch():
    """every entry point is exported; every GLM kernel instantiation is in the code object with no private segment and no VGPR spill
    (the code object's kernel metadata, scripts/kernel_meta.py)"""
    from ahmc_amd import build as B

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_meta
    finally:
        sys.path.pop(0)
    assert os.path.exists(B.OUT), "build() first"
    dll = C.CDLL(B.OUT)
    for name in capi.GLM_SIGNATURES:
        getattr(dll, name)
    meta = kernel_meta.kernel_meta(B.OUT)
    names = subprocess.run(["c++filt"], input="\n".join(k["name"] for k in meta), capture_output=True, text=True, check=True).stdout.splitlines()
    want = [f"k_glm_eta<{t}, {f}, {bn}>" for t in ("float", "double") for f in (0, 1, 2) for bn in (64, 16)]
    want += [f"k_glm_grad<{t}, {bn}>" for t in ("float", "double") for bn in (64, 16)]
    want += [f"k_glm_{w}<{t}>" for w in ("gsum", "lp") for t in ("float", "double")]
    found = {}
    for k, dn in zip(meta, names):
        for w in want:
            if dn.startswith(f"void ahmc::{w}("):
                found[w] = k
    assert sorted(found) == sorted(want), sorted(set(want) - set(found))
    for w, k in found.items():
        assert k["private_segment_fixed_size"] == 0, (w, k)
        assert k.get("vgpr_spill_count", 0) == 0, (w, k)


def test_cpu_checker_refuses_glm_target(oracle):
    assert oracle.has_glm is False
    rs = np.random.default_rng(5)
    t = A.GLMTarget(rs.normal(size=(7, 4)), (rs.random(7) < 0.5).astype(float))
    with pytest.raises(A.UnsupportedError, match="ahmc_glm.h"):
        A.Engine(A.Hamiltonian(A.UnitEuclideanMetric(4), t), 3, lib=oracle)
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric(4), A.IsoGaussian(4)), 3, lib=oracle)
    with pytest.raises(A.UnsupportedError, match="ahmc_glm.h"):
        e.glm_pointwise()
    with pytest.raises(A.UnsupportedError, match="ahmc_glm.h"):
        e.set_target(t)


@pytest.mark.parametrize("fam", [0, 1, 2], ids=FAMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_bounds_hold_for_a_host_emulation_and_catch_a_wrong_sign(fam, dtype):
    """The planted defect.  The device's arithmetic emulated on the host in the element type passes every assertion of §1 (with
    numpy's exp / log1p measured the way the device's are); the same emulation with the data term of g given the wrong sign — and,
    for ℓ, softplus added instead of subtracted — breaks the assertion meant for it: the bounds can fail."""
    eps = function_eps(np.exp, np.log1p, dtype)
    for shape in ((65, 17, 5), (1030, 3, 4)):
        c = case(*shape, fam, np.dtype(dtype).name)
        key = f"host-emulation {FAMS[fam]} {np.dtype(dtype).name} {shape}"
        ll, uu, lp, g = emulate(c)
        check_case(key, c, eps, eta=c["eta_hat"].copy(), ll=ll, lp=lp, g=g)
        _, Eu = link_bounds(c, eps)
        record_bound(f"u {key}", np.abs(uu.astype(LD) - c["u"]), Eu)
        before = json.dumps(MARGINS.get(f"grad {key}"))
        _, _, _, g_bad = emulate(c, sign=-1.0)
        with pytest.raises(AssertionError, match="grad planted"):
            check_case("planted " + key, c, eps, g=g_bad)
        if fam == G.BERNOULLI_LOGIT:
            ll_bad = ll + 2 * (np.where(c["eta_hat"] > 0, c["eta_hat"], 0) + np.log1p(np.exp(-np.abs(c["eta_hat"])))).astype(c["dtype"])
            with pytest.raises(AssertionError, match="loglik planted"):
                check_case("planted " + key, c, eps, ll=ll_bad)
        assert json.dumps(MARGINS.get(f"grad {key}")) == before
        for k in [k for k in MARGINS if " planted " in k]:
            del MARGINS[k]
    _dump_margins()


# ------------------------------------------------------------------------------------------------
# §3's inputs, and its precondition on the oracle alone
# ------------------------------------------------------------------------------------------------
PARITY_CASES = [(n, d, f) for (n, d) in ((130, 17), (65, 65), (200, 5)) for f in ("bernoulli_logit", "poisson_log")]


def parity_inputs(n_obs, D, family, N=300):
    rs = np.random.default_rng(n_obs + D)
    X = rs.normal(size=(n_obs, D)) / np.sqrt(D)
    beta = rs.normal(size=D)
    eta = X @ beta
    y = (rs.random(n_obs) < 1 / (1 + np.exp(-eta))).astype(np.float64) if family == "bernoulli_logit" else rs.poisson(np.exp(eta)).astype(np.float64)
    minv = np.asfortranarray(0.5 + rs.random((D, N)))
    th0 = 0.5 * rs.normal(size=(D, N))
    eps = 0.2 * (0.7 + 0.6 * rs.random(N))
    return X, y, np.ones(D), minv, th0, eps


def oracle_engine(oracle, X, y, family, p, metric, N, seed=8):
    from test_user_targets import host_kernel

    cb = host_kernel(lambda th: G.logdensity(family, X, y, th, None, p, 1.0))
    return A.Engine(A.Hamiltonian(metric, A.KernelTarget(X.shape[1], cb, handle_kind=capi.KERNEL_HOST)), N, rng=A.PhiloxRNG(seed), lib=oracle)


def parity_sequence(o, g, th0, eps, what, nuts_depth=6, full=True):
    """§3's sequence on the oracle engine `o` and, if given, the HIP engine `g`; returns the smallest decision margin of the oracle.
    With `g`: every discrete statistic of every chain must agree — the margins leave no chain an excuse."""
    import parity_util as PU
    from test_gpu_parity import compare_transition_stats

    lf = A.Leapfrog(eps)
    nuts = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=nuts_depth)))
    hmc = A.HMCKernel(A.Trajectory(A.EndPointTS, lf, A.FixedNSteps(4)))
    es = [e for e in (g, o) if e is not None]
    for e in es:
        e.set_integrator(lf)
        e.set_position(th0)
    PU.reset_margin(o)
    smallest = np.inf
    bound = PU.bound(np.float64)

    def step_margin(label):
        nonlocal smallest
        m = PU.decision_margin(o, reset=False)
        smallest = min(smallest, float(m.min()))
        assert m.min() >= bound, f"{what} {label}: the oracle took a decision within {m.min():g} of a tie: the inputs no longer serve the comparison"

    if g is not None:
        zg, zo = g.phasepoint(), o.phasepoint()
        np.testing.assert_allclose(zg.lp.value, zo.lp.value, rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(zg.lp.gradient, zo.lp.gradient, rtol=1e-10, atol=1e-10)
    n_div = 0
    for k, label in ((hmc, "hmc"), (nuts, "nuts 1"), (nuts, "nuts 2")) if full else ((nuts, "nuts 1"), (nuts, "nuts 2")):
        for e in es:
            e.transition(k)
        step_margin(label)
        so = o.stats()
        n_div = max(n_div, int(so["numerical_error"].sum()))
        if g is not None:
            same = compare_transition_stats(g.stats(), so, np.float64, o, f"{what} {label}")
            assert same.all(), f"{what} {label}: {int((~same).sum())} chains differ although every margin is above the bound"
            np.testing.assert_allclose(g.phasepoint().theta, o.phasepoint().theta, rtol=1e-8, atol=1e-8)
        else:
            PU.reset_margin(o)
        th = o.phasepoint().theta
        for e in es:
            e.set_position(th)
    if not full:
        return smallest, n_div
    PU.reset_margin(o)
    eo = o.find_good_stepsize()
    step_margin("find_good_stepsize")
    if g is not None:
        ok = PU.check_equal_or_near_tie(g.find_good_stepsize(), eo, PU.decision_margin(o), np.float64, f"{what} find_good_stepsize")
        assert ok.all()
    PU.reset_margin(o)
    for e in es:
        e.set_integrator(A.Leapfrog(eo))
        e.set_position(th0)
        e.run(nuts, 3)
    step_margin("bulk run of 3")
    if g is not None:
        on = np.isclose(g.phasepoint().theta, o.phasepoint().theta, rtol=1e-8, atol=1e-8).all(axis=0)
        ok = PU.check_flips(on, PU.decision_margin(o), np.float64, f"{what} bulk run of 3")
        assert ok.all()
        assert g.accum()["n_transitions"] == 3
    return smallest, n_div


@pytest.mark.parametrize("n_obs,D,family", PARITY_CASES)
def test_parity_precondition_on_the_oracle_alone(oracle, n_obs, D, family):
    """On §3's inputs no decision of the oracle comes within MARGIN_BOUND[float64] of a tie, at any step of the sequence: the GPU
    comparison may demand exact agreement of every chain.  Poisson (200, 5): most chains diverge in the first transition (the −Inf path)."""
    X, y, p, minv, th0, eps = parity_inputs(n_obs, D, family)
    o = oracle_engine(oracle, X, y, family, p, A.DiagEuclideanMetric(minv), th0.shape[1])
    smallest, n_div = parity_sequence(o, None, th0, eps, f"glm {family} ({n_obs}, {D})")
    MARGINS[f"oracle-margin {family} ({n_obs}, {D})"] = {"smallest_decision_margin": smallest, "divergent_chains_max": n_div}
    _dump_margins()
    if (n_obs, D, family) == (200, 5, "poisson_log"):
        assert n_div >= 150, n_div
    o.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
_STATE = {}


@pytest.fixture(scope="module")
def probe(hip):
    import torch

    from ahmc_amd import build as B
    from ahmc_amd.hipmod import Module

    torch.cuda.init()
    if "probe" not in _STATE:
        _STATE["probe"] = Module(B.build_probe_object(PROBE))
    return _STATE["probe"]


def dev(a):
    """a host array as device memory in column-major order (ints as int32)"""
    import torch

    a = np.asarray(a)
    if a.dtype.kind in "iu":
        a = a.astype(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a.reshape(-1, order="F"))).cuda()


def host(t, shape):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().reshape(shape, order="F")


def device_eps(probe, dtype):
    """ε_exp, ε_log1p of the device's functions (the probe kernel of tests/device_probe/glm.hip), measured once per element type"""
    key = ("eps", np.dtype(dtype).name)
    if key not in _STATE:
        import torch

        def run(which):
            def fn(x):
                x_d = dev(x)
                e_d, l_d = torch.empty_like(x_d), torch.empty_like(x_d)
                probe.launch("glm_probe_exp_log1p_" + _sfx(dtype), (x.size + 255) // 256, 256, x_d, e_d, l_d, np.int64(x.size))
                return host(e_d if which == "exp" else l_d, x.shape)
            return fn

        _STATE[key] = function_eps(run("exp"), run("log1p"), dtype)
        MARGINS[f"device-functions {np.dtype(dtype).name}"] = dict(_STATE[key])
        _dump_margins()
    return _STATE[key]


def glm_engine(hip, c, cols=None, metric=None, seed=7, offset=True, prior=True):
    """an engine on the case's model, positioned at the case's θ (or the columns `cols` of it)"""
    th = c["th"] if cols is None else c["th"][:, cols]
    D, N = th.shape
    t = A.GLMTarget(c["X"], c["y"], family=c["fam"], prior_prec=c["p"] if prior else None, offset=c["off"] if offset else None, scale=c["scale"])
    e = A.Engine(A.Hamiltonian(metric or A.UnitEuclideanMetric((D, N)), t), N, dtype=c["dtype"],
                 rng=seed if isinstance(seed, A.PhiloxRNG) else A.PhiloxRNG(seed), lib=hip)
    e.set_integrator(A.Leapfrog(np.full(N, 0.05)))
    e.set_position(th)
    return e


class tile_shape:
    """AHMC_GLM_SMALL_BELOW for the calls inside: "small" forces the 64×16 tiles, "big" the 64×64 ones"""

    def __init__(self, which):
        self.value = {"small": "1000000000", "big": "0"}[which]

    def __enter__(self):
        self.old = os.environ.get("AHMC_GLM_SMALL_BELOW")
        os.environ["AHMC_GLM_SMALL_BELOW"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ["AHMC_GLM_SMALL_BELOW"]
        else:
            os.environ["AHMC_GLM_SMALL_BELOW"] = self.old


def evaluate(e, th=None):
    if th is not None:
        e.set_position(th)
    z = e.phasepoint()
    eta, ll = e.glm_pointwise()
    return eta, ll, z.lp.value.copy(), z.lp.gradient.copy()


@pytest.mark.gpu
@pytest.mark.parametrize("fam", [0, 1, 2], ids=FAMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_values_against_exact_references(hip, probe, fam, dtype):
    """§1: η bit for bit, ℓ / ℓπ / g inside their bounds, for every shape; and the same bits from either tile shape"""
    eps = device_eps(probe, dtype)
    for shape in SHAPES:
        c = case(*shape, fam, np.dtype(dtype).name)
        key = f"{FAMS[fam]} {np.dtype(dtype).name} {shape}"
        e = glm_engine(hip, c)
        fam_got, n_got, scale_got = C.c_int32(), C.c_int64(), C.c_double()
        e._call("ahmc_get_target_glm", C.byref(fam_got), C.byref(n_got), C.byref(scale_got))
        assert (fam_got.value, n_got.value, scale_got.value) == (fam, shape[0], c["scale"])
        eta, ll, lp, g = evaluate(e)
        check_case(key, c, eps, eta=eta, ll=ll, lp=lp, g=g)
        for which in ("small", "big"):
            with tile_shape(which):
                got = evaluate(e, c["th"])
            for name, a, b in zip(("eta", "loglik", "lp", "grad"), got, (eta, ll, lp, g)):
                record_bits(f"tile-shape-{which}-{name} {key}", a, b)
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_offset_and_prior_absent(hip, probe, dtype):
    """offset = NULL and prior_prec = NULL are a zero offset and a zero precision"""
    for fam in (0, 1, 2):
        c = dict(case(130, 17, 17, fam, np.dtype(dtype).name))
        e = glm_engine(hip, c, offset=False, prior=False)
        eta, ll, lp, g = evaluate(e)
        e.close()
        z = dict(c)
        z["off"], z["p"] = np.zeros_like(c["off"]), np.zeros_like(c["p"])
        t = A.GLMTarget(z["X"], z["y"], family=fam, prior_prec=z["p"], offset=z["off"], scale=z["scale"])
        e2 = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((17, 17)), t), 17, dtype=dtype, rng=A.PhiloxRNG(7), lib=hip)
        e2.set_position(c["th"])
        for name, a, b in zip(("eta", "loglik", "lp", "grad"), evaluate(e2), (eta, ll, lp, g)):
            record_bits(f"absent-{name} {FAMS[fam]} {np.dtype(dtype).name}", a, b)
        e2.close()
        record_bits(f"absent-eta-chain {FAMS[fam]} {np.dtype(dtype).name}", eta, chain(c["X"], c["th"]))
        # without a prior ℓπ is the sum of the pointwise ℓ̂ the device itself returned: n_obs − 1 additions in some order
        u = U[np.dtype(dtype)]
        record_bound(f"absent-lp-is-the-sum {FAMS[fam]} {np.dtype(dtype).name}", np.abs(lp.astype(LD) - ll.astype(LD).sum(axis=0)),
                     SLACK * (gam(130, u) * np.abs(ll.astype(LD)).sum(axis=0) + u * np.abs(lp.astype(LD))))


def grad_kernel(dtype, bn):
    return f"_ZN4ahmc10k_glm_gradI{TCH[np.dtype(dtype)]}Li{bn}EEEvPKT_S3_S3_S3_PS1_S4_iillPKii"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_gradient_product_alone(hip, probe, dtype):
    """§1: k_glm_grad (+ k_glm_gsum past one slice) launched from the probe on a GIVEN U, both tile shapes, all chains and a chain
    list: g equals the chain-per-slice model bit for bit; columns off the list keep their NaN"""
    import torch

    dtype = np.dtype(dtype)
    for n_obs, D, N in SHAPES:
        rs = np.random.default_rng([n_obs, D, N, 77])
        c = case(n_obs, D, N, 2, dtype.name)
        Um = np.asfortranarray(rs.normal(size=(n_obs, N)) * 10.0 ** rs.uniform(-3, 3, size=(1, N)), dtype=dtype)
        want = grad_model(c["Xt"], Um, c["p"], c["th"])
        ns = (n_obs + G.K_SLICE - 1) // G.K_SLICE
        nrb = (D + 63) // 64 * ns
        lists = [None]
        if N > 1:
            lists.append(np.sort(rs.choice(N, size=max(1, N // 2), replace=False)))
        Xt_d, U_d, p_d, th_d = dev(c["Xt"]), dev(Um), dev(c["p"]), dev(c["th"])
        for idx in lists:
            n = N if idx is None else idx.size
            idx_d = NULL if idx is None else dev(idx)
            for bn in (64, 16):
                g_d = torch.full((D * N,), float("nan"), dtype=th_d.dtype, device="cuda")
                gs_d = torch.full((max(1, ns * D * N if ns > 1 else 1),), float("nan"), dtype=th_d.dtype, device="cuda")
                grid = (nrb * (((n + 63) // 64 + 7) // 8 * 8),) if bn == 64 else (nrb, (n + 15) // 16)   # (glm_target's grids)
                probe.launch(grad_kernel(dtype, bn), grid, 256, Xt_d, U_d, p_d, th_d, g_d, gs_d, int(n_obs), int(D), np.int64(n), np.int64(N), idx_d, int(ns))
                if ns > 1:
                    probe.launch(f"_ZN4ahmc10k_glm_gsumI{TCH[dtype]}EEvPKT_S3_S3_PS1_illPKii", (n * D + 255) // 256, 256, gs_d, p_d, th_d, g_d, int(D), np.int64(n),
                                 np.int64(N), idx_d, int(ns))
                got = host(g_d, (D, N))
                cols = np.arange(N) if idx is None else idx
                record_bits(f"grad-product {dtype.name} ({n_obs}, {D}, {N}) BN={bn} {'all' if idx is None else 'list'}", got[:, cols], want[:, cols])
                rest = np.setdiff1d(np.arange(N), cols)
                assert np.isnan(got[:, rest]).all()


# ---- §2 invariances, bit for bit ----
def nuts_kernel(N, eps=0.05, depth=6):
    return A.HMCKernel(A.Trajectory(A.MultinomialTS, A.Leapfrog(np.full(N, eps)), A.GeneralisedNoUTurn(max_depth=depth)))


INV_SHAPES = ((130, 17, 130), (1030, 65, 70))


@pytest.mark.gpu
@pytest.mark.parametrize("fam,dtype", [(0, np.float64), (1, np.float32), (2, np.float64), (0, np.float32)], ids=["logit-f64", "poisson-f32", "gauss-f64", "logit-f32"])
def test_chain_blocks_equal_one_engine(hip, fam, dtype):
    """one engine over N chains == engines over random blocks of the chains (chain_offset keeps each chain's random stream): the
    evaluation at θ, and three NUTS transitions — a chain's bits do not depend on N, its column or the chains beside it"""
    for shape in INV_SHAPES:
        c = case(*shape, fam, np.dtype(dtype).name)
        N = shape[2]
        rs = np.random.default_rng(N + fam)
        cuts = np.concatenate([[0], np.sort(rs.choice(np.arange(1, N), size=3, replace=False)), [N]])
        whole = glm_engine(hip, c, seed=A.PhiloxRNG(17))
        ev = evaluate(whole)
        whole.run(nuts_kernel(N), 3)
        th_w, st_w = whole.theta(), whole.stats()
        whole.close()
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            cols = np.arange(lo, hi)
            e = glm_engine(hip, c, cols=cols, seed=A.PhiloxRNG(17, chain_offset=int(lo)))
            for name, a, b in zip(("eta", "loglik", "lp", "grad"), evaluate(e), ev):
                record_bits(f"blocks-{name} {FAMS[fam]} {np.dtype(dtype).name} {shape}", a, b[..., cols])
            e.run(nuts_kernel(hi - lo), 3)
            record_bits(f"blocks-theta {FAMS[fam]} {np.dtype(dtype).name} {shape}", e.theta(), th_w[:, cols])
            np.testing.assert_array_equal(e.stats()["n_steps"], st_w["n_steps"][cols])
            e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_tile_shape_does_not_change_a_run(hip, dtype):
    """three NUTS transitions with the 64×16 tiles forced == with the 64×64 tiles forced == the default rule"""
    for fam in (0, 1):
        c = case(1030, 65, 70, fam, np.dtype(dtype).name)
        out = {}
        for which in ("default", "small", "big"):
            e = glm_engine(hip, c)
            if which == "default":
                e.run(nuts_kernel(70), 3)
            else:
                with tile_shape(which):
                    e.run(nuts_kernel(70), 3)
                    e.sync()
            out[which] = (e.theta(), e.stats()["n_steps"].copy())
            e.close()
        assert out["default"][1].sum() > 3 * 70
        for which in ("small", "big"):
            record_bits(f"tile-shape-run-{which} {FAMS[fam]} {np.dtype(dtype).name}", out[which][0], out["default"][0])
            np.testing.assert_array_equal(out[which][1], out["default"][1])


@pytest.mark.gpu
def test_rebinding_equals_a_fresh_context(hip):
    """GLM → IsoGaussian (runs on the fused kernels) → the GLM again == a fresh context; and a second model replaces the first"""
    c = case(130, 17, 130, 0, "float64")
    N = 130
    other = case(64, 17, 130, 1, "float64")
    a = glm_engine(hip, other)
    a.transition(nuts_kernel(N))
    a.set_target(A.IsoGaussian(17))
    with pytest.raises(A.ArgumentError, match="no GLM is bound"):
        a.glm_pointwise()
    a.set_position(c["th"])
    a.transition(nuts_kernel(N))
    a.set_target(A.GLMTarget(c["X"], c["y"], family=0, prior_prec=c["p"], offset=c["off"], scale=c["scale"]))
    a.seed(A.PhiloxRNG(7))
    a.set_position(c["th"])
    b = glm_engine(hip, c)
    for e in (a, b):
        e.run(nuts_kernel(N), 3)
    np.testing.assert_array_equal(a.theta(), b.theta())
    for key in ("n_steps", "tree_depth", "log_density"):
        np.testing.assert_array_equal(a.stats()[key], b.stats()[key])
    for x, y_ in zip(a.glm_pointwise(), b.glm_pointwise()):
        np.testing.assert_array_equal(x, y_)
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_checkpoint_resume_and_bulk_equals_stepwise(hip, dtype):
    """get_state after 11 of 24 NUTS iterations (20 adapting, StanHMCAdaptor) → a fresh context with the target set again → the rest == uninterrupted;
    and the bulk run == the stepwise loop of transition + adapt"""
    c = case(130, 17, 70, 0, np.dtype(dtype).name)
    N = 70
    kern = nuts_kernel(N)

    def engine():
        e = glm_engine(hip, c, metric=A.DiagEuclideanMetric((17, N)))
        e.set_integrator(kern.tau.integrator)
        e.adaptor_init(A.StanHMCAdaptor(A.MassMatrixAdaptor(A.DiagEuclideanMetric((17, N))), A.StepSizeAdaptor(0.8, kern.tau.integrator), 5, 5, 5))
        return e

    whole = engine()
    whole.run(kern, 24, n_adapts=20)
    part = engine()
    part.run(kern, 11, n_adapts=20)
    st = part.get_state()
    part.close()
    # (the same seed: a chain's random stream is (seed, chain, iteration); M⁻¹'s values, ϵ and the adaptor come with the state)
    fresh = glm_engine(hip, c, metric=A.DiagEuclideanMetric((17, N)))
    fresh.set_integrator(kern.tau.integrator)
    fresh.set_state(st)
    fresh.run(kern, 24, n_adapts=20, i_first=12)
    np.testing.assert_array_equal(whole.theta(), fresh.theta())
    np.testing.assert_array_equal(whole.get_stepsize(), fresh.get_stepsize())
    np.testing.assert_array_equal(whole.get_metric(), fresh.get_metric())
    fresh.close()
    step = engine()
    for i in range(1, 25):
        step.transition(kern)
        step.adapt(i, 20)
    np.testing.assert_array_equal(whole.theta(), step.theta())
    np.testing.assert_array_equal(whole.get_stepsize(), step.get_stepsize())
    np.testing.assert_array_equal(whole.get_metric(), step.get_metric())
    assert not np.array_equal(whole.get_metric(), np.ones((17, N)))
    step.close()
    whole.close()


# ---- §3 parity with the oracle ----
@pytest.mark.gpu
@pytest.mark.parametrize("n_obs,D,family", PARITY_CASES)
def test_glm_target_against_oracle(hip, oracle, n_obs, D, family):
    """the HIP engine on GLMTarget against the oracle on the mirror as a host kernel (AHMC_KERNEL_HOST): static HMC, two NUTS
    transitions, find_good_stepsize, a bulk run of three — every discrete statistic of every chain (the precondition test shows that
    no chain has an excuse)"""
    X, y, p, minv, th0, eps = parity_inputs(n_obs, D, family)
    N = th0.shape[1]
    o = oracle_engine(oracle, X, y, family, p, A.DiagEuclideanMetric(minv), N)
    g = A.Engine(A.Hamiltonian(A.DiagEuclideanMetric(minv), A.GLMTarget(X, y, family=family, prior_prec=p)), N, rng=A.PhiloxRNG(8), lib=hip)
    smallest, n_div = parity_sequence(o, g, th0, eps, f"glm {family} ({n_obs}, {D})")
    if (n_obs, D, family) == (200, 5, "poisson_log"):
        assert n_div >= 150, n_div
    g.close()
    o.close()


@pytest.mark.gpu
def test_glm_target_against_oracle_dense_metric(hip, oracle):
    """the same behind a shared DenseEuclideanMetric at (130, 17): w′ = M⁻¹g′ on MFMA from the GLM's gradient"""
    X, y, p, _, th0, eps = parity_inputs(130, 17, "bernoulli_logit")
    N, D = th0.shape[1], 17
    rs = np.random.default_rng(170)
    Q, _ = np.linalg.qr(rs.normal(size=(D, D)))
    Mi = (Q * np.linspace(0.6, 2.0, D)) @ Q.T
    make = lambda: A.DenseEuclideanMetric(np.asfortranarray((Mi + Mi.T) / 2))  # noqa: E731
    o = oracle_engine(oracle, X, y, "bernoulli_logit", p, make(), N)
    g = A.Engine(A.Hamiltonian(make(), A.GLMTarget(X, y, prior_prec=p)), N, rng=A.PhiloxRNG(8), lib=hip)
    parity_sequence(o, g, th0, eps, "glm dense metric (130, 17)")
    g.close()
    o.close()


@pytest.mark.gpu
def test_glm_target_against_oracle_wide(hip, oracle):
    """a wide context: D = 5000, n_obs = 40, N = 8, two NUTS transitions at max_depth 5"""
    n_obs, D, N = 40, 5000, 8
    rs = np.random.default_rng(n_obs + D)
    X = rs.normal(size=(n_obs, D)) / np.sqrt(D)
    y = (rs.random(n_obs) < 1 / (1 + np.exp(-(X @ rs.normal(size=D))))).astype(np.float64)
    p = np.ones(D)
    th0 = 0.5 * rs.normal(size=(D, N))
    eps = 0.2 * (0.7 + 0.6 * rs.random(N))
    o = oracle_engine(oracle, X, y, "bernoulli_logit", p, A.UnitEuclideanMetric((D, N)), N)
    g = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((D, N)), A.GLMTarget(X, y, prior_prec=p)), N, rng=A.PhiloxRNG(8), lib=hip)
    assert g.info("wide")
    parity_sequence(o, g, th0, eps, "glm wide (40, 5000)", nuts_depth=5, full=False)
    g.close()
    o.close()


# ---- §4 a posterior ----
@pytest.mark.gpu
def test_posterior_against_ask_tell(hip):
    """logit, n_obs = 200, D = 8, N = 256, StanHMCAdaptor, 150 adapting + 100 kept transitions: GLMTarget and ExternalTarget(glm.logdensity)
    on the same engine — R-hat < 1.05 in every dimension for both, pooled means within 5·√(mcse₁² + mcse₂²); then LowRankVar and a
    RankUpdateEuclideanMetric run on the model with finite statistics"""
    n_obs, D, N = 200, 8, 256
    rs = np.random.default_rng(41)
    X = rs.normal(size=(n_obs, D)) / np.sqrt(D)
    y = (rs.random(n_obs) < 1 / (1 + np.exp(-(X @ rs.normal(size=D))))).astype(np.float64)
    p = np.full(D, 0.25)
    th0 = 0.1 * rs.normal(size=(D, N))
    glm_t = A.GLMTarget(X, y, prior_prec=p)
    stats = {}
    for name, target in (("glm", glm_t), ("external", A.ExternalTarget(D, glm_t.logdensity))):
        e = A.Engine(A.Hamiltonian(A.DiagEuclideanMetric((D, N)), target), N, rng=A.PhiloxRNG(5), lib=hip)
        kern = nuts_kernel(N, eps=0.1, depth=8)
        e.set_integrator(kern.tau.integrator)
        e.set_position(th0)
        e.adaptor_init(A.StanHMCAdaptor(A.MassMatrixAdaptor(A.DiagEuclideanMetric((D, N))), A.StepSizeAdaptor(0.8, kern.tau.integrator)))
        e.run(kern, 150, n_adapts=150)
        draws = np.empty((100, D, N))
        for i in range(100):
            e.transition(kern)
            draws[i] = e.theta()
        stats[name] = A.summarystats(draws)
        assert np.all(stats[name]["rhat"] < 1.05), (name, stats[name]["rhat"])
        e.close()
    diff = np.abs(stats["glm"]["mean"] - stats["external"]["mean"])
    tol = 5 * np.sqrt(stats["glm"]["mcse"] ** 2 + stats["external"]["mcse"] ** 2)
    MARGINS["posterior"] = {"rhat_glm": stats["glm"]["rhat"].max(), "rhat_external": stats["external"]["rhat"].max(), "mean_difference_over_tolerance": float((diff / tol).max())}
    _dump_margins()
    assert np.all(diff < tol), (diff / tol)
    # the adaptors and metrics of the last pull requests on a model with data
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((D, N)), glm_t), N, rng=A.PhiloxRNG(6), lib=hip)
    kern = nuts_kernel(N, eps=0.1, depth=8)
    e.set_integrator(kern.tau.integrator)
    e.set_position(th0)
    e.adaptor_init(A.StanHMCAdaptor(A.LowRankVar(D, 2), A.StepSizeAdaptor(0.8, kern.tau.integrator), 10, 5, 5))
    e.run(kern, 40, n_adapts=30)
    st = e.stats()
    assert np.isfinite(e.theta()).all() and np.isfinite(st["log_density"]).all() and np.isfinite(st["step_size"]).all()
    Av, B, Dm = e.get_metric()
    assert B.shape == (D, 2) and np.isfinite(Av).all() and np.isfinite(B).all()
    e.close()
    B0 = np.asfortranarray(np.linalg.qr(rs.normal(size=(D, 2)))[0])
    e = A.Engine(A.Hamiltonian(A.RankUpdateEuclideanMetric(np.full(D, 0.5), B0, np.diag([2.0, 1.0])), glm_t), N, rng=A.PhiloxRNG(6), lib=hip)
    e.set_integrator(kern.tau.integrator)
    e.set_position(th0)
    e.run(kern, 5)
    st = e.stats()
    assert np.isfinite(e.theta()).all() and np.isfinite(st["log_density"]).all() and st["n_steps"].min() >= 1
    e.close()


# ---- §5 errors ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_refusals(hip, dtype):
    """every AHMC_ERR_ARGUMENT / _UNSUPPORTED case of the header; after each refused call the context still runs a transition on the
    model it had"""
    c = case(65, 3, 17, 0, np.dtype(dtype).name)
    D, N, n = 3, 17, 65
    e = glm_engine(hip, c)
    kern = nuts_kernel(N)
    X, y, off, p = (np.asfortranarray(c["X"]), c["y"].copy(), c["off"].copy(), c["p"].copy())

    def still_runs():
        e.transition(kern)
        assert np.isfinite(e.theta()).all() and e.stats()["n_steps"].min() >= 1
        fam = C.c_int32(-1)
        e._call("ahmc_get_target_glm", C.byref(fam), None, None)
        assert fam.value == 0

    def refused(exc, match, fam=0, n_obs=n, X_=X, y_=y, off_=off, p_=p, scale=1.0):
        with pytest.raises(exc, match=match):
            e._call("ahmc_set_target_glm", fam, n_obs, capi.as_ptr(X_), capi.as_ptr(y_), capi.as_ptr(off_), capi.as_ptr(p_), scale)
        still_runs()

    def poked(a, i, v):
        b = a.copy(order="F")
        b.reshape(-1, order="F")[i] = v
        return b

    refused(A.ArgumentError, "n_obs", n_obs=0)
    refused(A.ArgumentError, "n_obs", n_obs=-3)
    refused(A.ArgumentError, "NULL", X_=None)
    refused(A.ArgumentError, "NULL", y_=None)
    refused(A.ArgumentError, "X holds a non-finite", X_=poked(X, 7, np.nan))
    refused(A.ArgumentError, "X holds a non-finite", X_=poked(X, n * D - 1, np.inf))
    refused(A.ArgumentError, "offset holds a non-finite", off_=poked(off, 3, -np.inf))
    refused(A.ArgumentError, "prior_prec holds a non-finite", p_=poked(p, 1, np.nan))
    refused(A.ArgumentError, "negative", p_=poked(p, 2, -1e-3))
    refused(A.ArgumentError, "DomainError", y_=poked(y, 5, 1.5))
    refused(A.ArgumentError, "DomainError", y_=poked(y, 5, -0.1))
    refused(A.ArgumentError, "DomainError", y_=poked(y, 0, np.nan))
    refused(A.ArgumentError, "DomainError", fam=1, y_=poked(y, 64, -1.0))
    refused(A.ArgumentError, "DomainError", fam=1, y_=poked(y, 64, np.inf))
    refused(A.ArgumentError, "DomainError", fam=2, y_=poked(y, 1, np.nan))
    for s in (0.0, -1.0, np.inf, np.nan):
        refused(A.ArgumentError, "scale", scale=s)
    refused(A.ArgumentError, "unknown family", fam=3)
    refused(A.ArgumentError, "unknown family", fam=-1)
    refused(A.UnsupportedError, "AHMC_GLM_MAX_OBS", n_obs=(1 << 24) + 1)
    with pytest.raises(A.ArgumentError, match="ahmc_set_target_glm"):
        e._call("ahmc_set_target", capi.TARGET_GLM, None, 0)
    still_runs()
    # ahmc_set_ref_compat: refused where the step-synchronous engine refuses it for every target (a static EndPointTS transition, a leapfrog)
    hmc = A.HMCKernel(A.Trajectory(A.EndPointTS, kern.tau.integrator, A.FixedNSteps(3)))
    e.set_ref_compat(True)
    with pytest.raises(A.UnsupportedError, match="ahmc_set_ref_compat"):
        e.transition(hmc)
    with pytest.raises(A.UnsupportedError, match="ahmc_set_ref_compat"):
        e.step(2)
    e.set_ref_compat(False)
    e.transition(hmc)
    still_runs()
    # ahmc_ext_*: as for any target that is not AHMC_TARGET_EXTERNAL
    k = kern.cfg()
    with pytest.raises(A.AHMCError, match="not AHMC_TARGET_EXTERNAL"):
        e._call("ahmc_ext_begin", C.byref(k), 1)
    still_runs()
    e.close()
    # without a GLM bound
    d = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((D, N)), A.IsoGaussian(D)), N, dtype=dtype, rng=A.PhiloxRNG(1), lib=hip)
    with pytest.raises(A.ArgumentError, match="no GLM is bound"):
        d._call("ahmc_get_target_glm", None, None, None)
    with pytest.raises(A.ArgumentError, match="no GLM is bound"):
        d._call("ahmc_glm_pointwise", None, None)
    d.set_integrator(kern.tau.integrator)
    d.set_position(c["th"])
    d.transition(kern)
    assert np.isfinite(d.theta()).all()
    d.close()
