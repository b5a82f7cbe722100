"""The dense engine's products and caches (csrc/ahmc_dense.hpp, ahmc_dense_host.hpp) against EXACT references.

The parity tests hold the dense engine to the CPU oracle at 1e-8 (Float64) / 2e-3 (Float32): the oracle adds in another order, so
nothing tighter can be asked of that comparison.  Here the reference is mathematics instead:

  exact(A, X)   the product in x86 80-bit long double of the values as stored in the element type, with the companion |A|·|X|
                (tests/host_ref/fma_chain.cpp, checked against mpmath at 120 bits);
  chain(A, X)   acc ← fma(A[i,k], X[k,j], acc) for k = 0 … D−1 from acc = +0 in the element type with a correctly rounded host
                fma (std::fma, checked against mpmath).  `v_mfma_f32_16x16x4_f32` / `v_mfma_f64_16x16x4_f64` accumulate as a
                k-ordered chain of fused multiply-adds and k_dgemm / k_dgemm_small walk k upwards into one accumulator per element
                (`ks·4 + lane/16` inside a 16-deep tile; the zero padding past D adds fma(0, 0, acc) = acc), so every element of a
                product should equal the chain BIT FOR BIT.

u is the unit roundoff (2^-53 / 2^-24), γ_k = k·u / (1 − k·u) (Higham, Accuracy and Stability of Numerical Algorithms, §3.1).

§0  the references themselves and `test_bounds_are_not_vacuous` (CPU): a host emulation with one planted defect each breaks the
    assertion meant for it.
§1  k_dgemm and k_dgemm_small alone, launched from tests/device_probe/dense.hip (explicit instantiations of the engine's own
    templates) with the grids of `dn_gemm`: the componentwise bound |Y − exact| ≤ γ_D·|A|·|X| (any order of summation; no fitted
    factor; the reference's own γ⁶⁴_{D+1}·|A|·|X|, 2^-11 of it, is added), `== chain` bit for bit, independence of the kernel, of N,
    of the column's place in the tile and of the addressing mode (plain, `idx`, `A2/Y2`, the point pool `ptidx`), and a NaN pattern
    in every element the launch does not own.
§2  the same products through the C ABI on the step-synchronous path, with `dense_gemm_launches` / `dense_gemm_small_launches` asserting which kernel
    `dn_gemm` took: ∇ℓπ == −chain(P, θ) bit for bit, ℓπ / ℓκ inside the bound of k_d_coldot, the first leapfrog's velocity against the exact
    M⁻¹(r − ϵ/2·g), the fresh momentum against U⁻¹z with U the long-double Cholesky factor and z the normals of an identity-metric engine.
§3  the carried velocity v ← v − ϵ/2·w after n ∈ {1, 7, 63, 255, 1 023, −255} leapfrogs (plain and tempered): ℓκ against the exact −½ rᵀM⁻¹r of
    the device's own r inside a bound that grows linearly in n, its magnitudes from a long-double replay.
§4  what three NUTS transitions leave behind on the step-synchronous kernels, k_dense_epoch and every compiled shape of k_dense_epoch2: ∇ℓπ == −chain(P, θ)
    bit for bit for every chain (the swizzled operand copy and each product loop, to the last bit), ℓπ, ℓκ (normwise, magnitudes through the energy),
    hamiltonian_energy == −ℓπ − ℓκ, n_steps against tree_depth, and the engine asked for is the engine that ran.

Measured on the MI355X (profiles/dense_products_margins.json; the fresh-momentum cases of §2 were added after that run and are not in it): 1.67·10⁸ elements compared bit for bit with the chain, none differs — the chain model holds
for both MFMA instructions, so no comparison is an expected failure.  Largest error / bound: §1 0.97 (at D = 1, 2, where γ_D is one or two roundings; 0.64
on the ill-conditioned symmetric operand, 0.47 through the addressing modes, 0.10 at the large index); §2 0.99 and §4 1.00 on the single-rounding statements
(r after a leapfrog, H = −ℓπ − ℓκ), 0.31 on the first velocity, 0.16 on ℓπ / ℓκ; §3 0.015 on ℓκ (0.0011 at n = 1 023: the carried v drifts like √n, the bound
is linear in n); §4 0.0015 on ℓπ and 6·10⁻⁶ on ℓκ — its normwise bound goes through the energy and cond(M⁻¹)·cond(P), so there it proves little more than
that no half-kick is missing in Float64.

What was cut to keep the CPU references of the module under about five minutes: above D = 513 the column counts are
N ∈ {1, 17, 64, 65, 70} (D ≤ 1 024) and N ∈ {1, 17, 70} (D = 2 048, 4 096) instead of the thirteen of the smaller shapes.
The large-index case (D·N > 2³¹) runs for k_dgemm only: k_dgemm_small takes its column blocks from gridDim.y ≤ 65 535, i.e.
N ≤ 1 048 560 — `dn_gemm` never gives it more than n_cu·64 columns — so it cannot be launched at N = 2²⁵ + 70.

Every comparison records error / bound and the bit mismatches per case; a run writes them to dense_products_margins.json in
$AHMC_TEST_OUT (default: test_out/ in the repository root, ignored by git); a copy of the MI355X run is
profiles/dense_products_margins.json.
"""
import ctypes as C
import functools
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ahmc_amd as A

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "device_probe", "dense.hip")
HOST_REF = os.path.join(ROOT, "tests", "host_ref", "fma_chain.cpp")
DTYPES = (np.float64, np.float32)
U = {np.dtype(np.float64): LD(2) ** -53, np.dtype(np.float32): LD(2) ** -24}
U_LD = LD(2) ** -64
TCH = {np.dtype(np.float64): "d", np.dtype(np.float32): "f"}
GB_M, GB_N, GB_K = 64, 64, 16                      # csrc/ahmc_dense.hpp
PV_TH, PV_R, PV_G, PV_V, PV_W, PV_COUNT = 0, 1, 2, 3, 4, 5
KERNELS = ("k_dgemm", "k_dgemm_small")

D_ALL = (1, 2, 3, 4, 5, 15, 16, 17, 31, 33, 63, 64, 65, 100, 127, 128, 129, 200, 255, 256, 257, 384, 511, 512, 513, 768, 1000, 1024,
         2048, 4096)
N_SMALL_D = (1, 2, 15, 16, 17, 63, 64, 65, 70, 511, 512, 513, 520)
KINDS = ("spd", "triu", "identity")
D_MODES = (5, 64, 200, 512)
N_MODES = (1, 15, 16, 17, 63, 64, 65, 70)
NPT = 7                                            # points per chain of the test's pool


def n_list(D):
    return N_SMALL_D if D <= 513 else ((1, 17, 64, 65, 70) if D <= 1024 else (1, 17, 70))


def n_cols(D):
    """columns of a case's X: the largest N and twelve more for the `idx` lists that leave columns out"""
    return max(n_list(D)) + 12


MARGINS = {}       # case id -> {"error_over_bound", "bit_compared", "bit_mismatch"}


def _dump_margins():
    out = os.environ.get("AHMC_TEST_OUT") or os.path.join(ROOT, "test_out")
    try:
        os.makedirs(out, exist_ok=True)
        worst, bits = {}, {"compared": 0, "mismatch": 0}
        for k, v in MARGINS.items():
            sec = k.split(" ")[0]
            worst[sec] = max(worst.get(sec, 0.0), v["error_over_bound"])
            bits["compared"] += v["bit_compared"]
            bits["mismatch"] += v["bit_mismatch"]
        with open(os.path.join(out, "dense_products_margins.json"), "w") as f:
            json.dump({"dry_run_on_oracle": os.environ.get("AHMC_TEST_DRYRUN_ON_ORACLE") == "1", "worst_error_over_bound_per_section": worst,
                       "elements_compared_bit_for_bit": bits, "cases": dict(sorted(MARGINS.items()))}, f, indent=1)
    except OSError:
        pass


def _entry(key):
    return MARGINS.setdefault(key, {"error_over_bound": 0.0, "bit_compared": 0, "bit_mismatch": 0})


def record_bound(key, err, bound):
    """largest err / bound of a comparison (0/0 counts as 0), kept under `key`; asserts it is ≤ 1 element by element"""
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    assert np.isfinite(err).all(), f"{key}: non-finite result"
    frac = np.where(err == 0, LD(0), err / np.where(bound > 0, bound, LD("1e-4900")))
    worst = float(frac.max()) if frac.size else 0.0
    e = _entry(key)
    e["error_over_bound"] = max(e["error_over_bound"], worst)
    _dump_margins()
    if worst > 1.0:
        ij = np.unravel_index(int(np.argmax(frac)), frac.shape)
        raise AssertionError(f"{key}: error {float(err[ij]):.3e} is {worst:.3g} × its bound {float(bound[ij]):.3e} at element {ij}")
    return worst


def record_bits(key, got, want):
    """the number of elements of `got` whose bits differ from `want` (any NaN equals any NaN), kept under `key`; asserts it is 0"""
    same = same_bits(got, want)
    e = _entry(key)
    e["bit_compared"] += int(same.size)
    e["bit_mismatch"] += int((~same).sum())
    _dump_margins()
    if not same.all():
        bad = np.argwhere(~same)
        g, w = np.asarray(got)[tuple(bad[0])], np.asarray(want)[tuple(bad[0])]
        with np.errstate(all="ignore"):
            ulps = np.abs(bits_of(np.asarray(got)[~same]).astype(np.int64) - bits_of(np.asarray(want)[~same]).astype(np.int64))
        raise AssertionError(f"{key}: {len(bad)} of {same.size} elements differ in their bits, by up to {int(ulps.max())} ulps; first at "
                             f"{tuple(bad[0])}: {g!r} instead of {w!r}")


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return (bits_of(a) == bits_of(b)) | (np.isnan(a) & np.isnan(b))


def gam(k, u):
    k = LD(k)
    assert k * u < 0.5
    return k * u / (1 - k * u)


# ------------------------------------------------------------------------------------------------
# §0  the references
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_lib():
    """tests/host_ref/fma_chain.cpp as its own shared object in the build cache, by the host compiler"""
    from ahmc_amd import build as B

    flags = ["-O2", "-march=native", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-ffp-contract=off"]
    with open(HOST_REF, "rb") as f:
        h = hashlib.sha256(f.read() + " ".join(flags).encode()).hexdigest()[:20]
    out_dir = os.path.join(B.OBJ, "host_ref")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, f"fma_chain_{h}.so")
    if not os.path.exists(so):
        cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
        tmp = so + f".tmp{os.getpid()}"
        res = subprocess.run([cxx, *flags, HOST_REF, "-o", tmp], capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"host reference build failed:\n{res.stdout}\n{res.stderr}")
        os.replace(tmp, so)
    dll = C.CDLL(so)
    for name in ("fma_f64", "fma_f32", "chain_f64", "chain_f32", "exact_f64", "exact_f32", "exact_f64_ld", "exact_f32_ld"):
        getattr(dll, name).restype = None
    return dll


def _sfx(dtype):
    return "f64" if np.dtype(dtype) == np.float64 else "f32"


def host_fma(a, b, c):
    dt = a.dtype
    a, b, c = (np.ascontiguousarray(x, dtype=dt) for x in (a, b, c))
    out = np.empty_like(a)
    getattr(ref_lib(), "fma_" + _sfx(dt))(C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), C.c_void_p(c.ctypes.data), C.c_void_p(out.ctypes.data),
                                          C.c_int64(a.size))
    return out


def _cm(a, dtype):
    """(D, n) values as column-major memory of the element type; a vector is one column"""
    a = np.asarray(a)
    if a.ndim == 1:
        a = a.reshape(-1, 1)
    return np.asfortranarray(a, dtype=dtype)


def chain(Am, X, dtype):
    """Y = A·X as the k-ordered fma chain of the element type (see the module docstring); A (D, D), X (D, n)"""
    Am, X = _cm(Am, dtype), _cm(X, dtype)
    D, n = X.shape
    assert Am.shape == (D, D)
    Y = np.empty((D, n), dtype=dtype, order="F")
    getattr(ref_lib(), "chain_" + _sfx(dtype))(C.c_void_p(Am.ctypes.data), C.c_void_p(X.ctypes.data), C.c_void_p(Y.ctypes.data), C.c_int64(D), C.c_int64(n),
                                               C.c_int64(D))
    return Y


def exact(Am, X):
    """(A·X, |A|·|X|) in 80-bit long double of the values as stored: A in its element type; X in the same type, or in long double (the replay
    of a trajectory)"""
    dtype = np.asarray(Am).dtype
    xt = np.asarray(X).dtype
    assert dtype in (np.float64, np.float32) and xt in (dtype, np.dtype(LD))
    Am, X = _cm(Am, dtype), _cm(X, xt)
    D, n = X.shape
    assert Am.shape == (D, D)
    Y, S = np.empty((D, n), dtype=LD, order="F"), np.empty((D, n), dtype=LD, order="F")
    fn = getattr(ref_lib(), "exact_" + _sfx(dtype) + ("_ld" if xt == np.dtype(LD) else ""))
    fn(C.c_void_p(Am.ctypes.data), C.c_void_p(X.ctypes.data), C.c_void_p(Y.ctypes.data), C.c_void_p(S.ctypes.data), C.c_int64(D), C.c_int64(n), C.c_int64(D))
    return Y, S


def product_bound(S, D, dtype):
    """γ_D·|A|·|X| in the element type (any order of summation, fused or not) + the long-double reference's own γ⁶⁴_{D+1}·|A|·|X|"""
    return (gam(D, U[np.dtype(dtype)]) + gam(D + 1, U_LD)) * S


def make_matrix(kind, D, dtype, rs):
    """`spd`: symmetric positive definite, condition number 1e6 (Float64) / 1e4 (Float32), a log-uniform spectrum turned by three
    Householder reflectors (O(D²), entries of mixed sign); `triu`: a general upper-triangular matrix (the shape of U⁻¹ — the one
    non-symmetric operand of the engine); `identity`."""
    if kind == "identity":
        return np.asfortranarray(np.eye(D), dtype=dtype)
    if kind == "triu":
        T = np.triu(rs.normal(size=(D, D))) * np.exp2(rs.uniform(-6, 6, size=(D, 1)))
        T[np.arange(D), np.arange(D)] = 1.0 + rs.random(D)
        return np.asfortranarray(T, dtype=dtype)
    cond = 1e6 if np.dtype(dtype) == np.float64 else 1e4
    M = np.diag(np.exp(np.log(cond) * (rs.permutation(D) / max(D - 1, 1))))
    for _ in range(3):
        v = rs.normal(size=(D, 1))
        v /= np.linalg.norm(v)
        M = M - 2 * v @ (v.T @ M)
        M = M - 2 * (M @ v) @ v.T
    return np.asfortranarray((M + M.T) / 2, dtype=dtype)


def make_x(D, n, dtype, rs):
    """columns of widely different scale and mixed sign: 1e-20 … 1e20 (Float64), 1e-8 … 1e8 (Float32: with |A| ≥ 1e-8 where it is not
    zero, every product stays above 1e-24, far from the Float32 subnormals, so the bounds need no absolute term)"""
    span = 20 if np.dtype(dtype) == np.float64 else 8
    X = rs.normal(size=(D, n)) * 10.0 ** rs.uniform(-span, span, size=(1, n))
    return np.asfortranarray(X, dtype=dtype)


@functools.lru_cache(maxsize=8)
def gemm_case(D, dtname, kind):
    """operands and references of one §1 case: every N and every addressing mode uses a prefix / a subset of the SAME columns, so that
    a column's result can be compared across N, tile positions and modes"""
    dtype = np.dtype(dtname)
    rs = np.random.default_rng([D, dtype.itemsize, KINDS.index(kind)])
    Am = make_matrix(kind, D, dtype, rs)
    X = make_x(D, n_cols(D), dtype, rs)
    Ye, S = exact(Am, X)
    return {"A": Am, "X": X, "chain": chain(Am, X, dtype), "exact": Ye, "S": S}


def _mp(x):
    import mpmath

    return mpmath.mpf(np.format_float_scientific(LD(x), precision=30, unique=False))


def test_exact_agrees_with_mpmath():
    """exact() against mpmath at 120 bits on a few hundred entries: within γ⁶⁴_{D+1}·|A|·|X|, the term product_bound adds for it"""
    import mpmath

    assert np.finfo(LD).nmant >= 63, "the references need x86 80-bit long double"
    mpmath.mp.prec = 120
    rs = np.random.default_rng(5)
    n_checked = 0
    for dtype in DTYPES:
        for D, kind in ((5, "triu"), (100, "spd"), (257, "spd"), (513, "triu")):
            c = gemm_case(D, np.dtype(dtype).name, kind)
            for _ in range(40):
                i, j = int(rs.integers(D)), int(rs.integers(c["X"].shape[1]))
                ref = mpmath.fsum(mpmath.mpf(float(a)) * mpmath.mpf(float(x)) for a, x in zip(c["A"][i, :], c["X"][:, j]))
                s = mpmath.fsum(abs(mpmath.mpf(float(a)) * mpmath.mpf(float(x))) for a, x in zip(c["A"][i, :], c["X"][:, j]))
                assert abs(_mp(c["exact"][i, j]) - ref) <= _mp(gam(D + 1, U_LD)) * s
                assert abs(_mp(c["S"][i, j]) - s) <= _mp(gam(D + 1, U_LD)) * s
                n_checked += 1
    assert n_checked >= 300


def test_host_fma_is_correctly_rounded():
    """the helper's fma against mpmath (exact product and sum, ONE rounding to 53 / 24 bits, ties to even) on 10⁴ triples per type:
    random ones, massive cancellation (c ≈ −a·b, the residual far below an ulp of the product) and exact ties"""
    import mpmath

    rs = np.random.default_rng(6)
    for dtype, p in ((np.float64, 53), (np.float32, 24)):
        n = 10000
        a = (rs.normal(size=n) * np.exp2(rs.integers(-20, 20, n))).astype(dtype)
        b = (rs.normal(size=n) * np.exp2(rs.integers(-20, 20, n))).astype(dtype)
        c = (rs.normal(size=n) * np.exp2(rs.integers(-40, 40, n))).astype(dtype)
        k = n // 3
        c[:k] = -(a[:k] * b[:k])                                  # cancellation: fma returns the rounding error of the product exactly
        c[k:k + k // 2] = np.nextafter(c[:k // 2], dtype(0))      # … and one ulp beside it
        # ties: c = an integer m in [2^(p-1), 2^p) (ulp 1), a·b = (2j + 1)·½ = j + ½: the exact result m + j + ½ lies midway between neighbours
        t = slice(2 * k, 2 * k + 500)
        a[t] = (2 * rs.integers(0, 1000, 500) + 1).astype(dtype)
        b[t] = dtype(0.5)
        c[t] = rs.integers(2 ** (p - 1), 2 ** p - 2000, 500).astype(dtype)
        got = host_fma(a, b, c)
        with mpmath.workprec(400):
            for i in range(n):
                ex = mpmath.mpf(float(a[i])) * mpmath.mpf(float(b[i])) + mpmath.mpf(float(c[i]))
                with mpmath.workprec(p):
                    want = float(+ex)                             # one rounding to p bits, ties to even (the exponents stay in range)
                assert float(got[i]) == want, (dtype.__name__, i, a[i], b[i], c[i], got[i], want)
        # the ties were ties, and went to even
        assert (a[t] % 2 == 1).all() and (c[t] % 1 == 0).all() and (got[t] % 2 == 0).all() and (np.abs(got[t] - c[t] - a[t] // 2) <= 1).all()


def test_chain_is_the_k_ordered_fma_recurrence():
    """chain() is what its name says: the same recurrence written with host_fma, one k at a time"""
    rs = np.random.default_rng(7)
    for dtype in DTYPES:
        for D in (1, 5, 33):
            Am, X = make_matrix("triu", D, dtype, rs), make_x(D, 9, dtype, rs)
            acc = np.zeros((D, 9), dtype=dtype)
            for k in range(D):
                acc = host_fma(np.repeat(Am[:, k:k + 1], 9, axis=1), np.repeat(X[k:k + 1, :], D, axis=0), acc)
            assert same_bits(chain(Am, X, dtype), np.asfortranarray(acc)).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("D", D_ALL)
def test_chain_within_the_product_bound(D, dtype):
    """the reference arithmetic satisfies the componentwise bound of §1 at every shape of the GPU tests (or the bound could not be asked
    of the device)"""
    for kind in KINDS:
        c = gemm_case(D, np.dtype(dtype).name, kind)
        record_bound(f"§0 chain-vs-exact {kind} [{np.dtype(dtype).name}]", np.abs(c["chain"].astype(LD) - c["exact"]), product_bound(c["S"], D, dtype))
    if D > 64:  # the bound is not slack by orders of magnitude either: some element of the ill-conditioned product uses ≥ 1/D of it
        c = gemm_case(D, np.dtype(dtype).name, "spd")
        frac = np.abs(c["chain"].astype(LD) - c["exact"]) / product_bound(c["S"], D, dtype)
        assert frac.max() > 1.0 / D


def test_probe_compiles_like_the_library():
    """tests/device_probe/dense.hip compiles for gfx950 with the engine's flags, and its kernels have the register, LDS, scratch and spill
    figures of the same kernels inside libahmc_hip.so: the probe tests the code the engine runs"""
    from ahmc_amd import build as B

    co = B.build_probe_object(PROBE)
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_meta
    finally:
        sys.path.pop(0)
    probe = {k["name"]: k for k in kernel_meta.kernel_meta(co)}
    want = {kernel_name(k, dt) for k in KERNELS + ("k_d_coldot",) for dt in DTYPES}
    assert set(probe) == want
    lib = {k["name"]: k for k in kernel_meta.kernel_meta(B.build_hip_library())}
    for name in sorted(want):
        assert name in lib, name
        assert not probe[name]["private_segment_fixed_size"] and not probe[name]["vgpr_spill_count"] and not probe[name]["sgpr_spill_count"], probe[name]
        assert probe[name] == lib[name], (probe[name], lib[name])


def kernel_name(kernel, dtype):
    """the Itanium-mangled name of an instantiation of tests/device_probe/dense.hip"""
    t = TCH[np.dtype(dtype)]
    if kernel == "k_d_coldot":
        return f"_ZN4ahmc10k_d_coldotI{t}EEvPKT_S3_PS1_S1_ilPKi"
    return f"_ZN4ahmc{len(kernel)}{kernel}I{t}EEvPKT_S3_PS1_ilPKiS3_S4_S6_llll"


# -- the launch geometry, restated from ahmc_dense_host.hpp ------------------------------------------------------------------------
def gemm_takes_small(D, N, n_cu, two=False):
    """dn_gemm: the 64×16-tile kernel when the 64×64 tiles would not give every CU a workgroup"""
    row_blocks = (D + GB_M - 1) // GB_M * (2 if two else 1)
    return row_blocks * ((N + GB_N - 1) // GB_N) < n_cu


def gemm_grid(kernel, D, N, two=False):
    row_blocks = (D + GB_M - 1) // GB_M * (2 if two else 1)
    if kernel == "k_dgemm_small":
        return (row_blocks, (N + 15) // 16)
    cb8 = ((N + GB_N - 1) // GB_N + 7) // 8 * 8          # column blocks padded to the 8 XCDs
    return (row_blocks * cb8,)


def grid_chains(n):
    return (n + 3) // 4                                   # dn_grid_chains: one wave per chain, 4 per block


def grid_elems(D, n):
    return (D * n + 255) // 256                           # dn_grid_elems


def test_launch_geometry_restated():
    assert gemm_grid("k_dgemm", 512, 2304) == (8 * 40,) and gemm_grid("k_dgemm", 512, 2304, two=True) == (16 * 40,)
    assert gemm_grid("k_dgemm", 5, 1) == (8,) and gemm_grid("k_dgemm_small", 65, 17) == (2, 2) and gemm_grid("k_dgemm_small", 64, 16, two=True) == (2, 1)
    assert gemm_takes_small(512, 1984, 256) and not gemm_takes_small(512, 1985, 256)
    assert gemm_takes_small(512, 960, 256, two=True) and not gemm_takes_small(512, 961, 256, two=True)
    assert grid_chains(5) == 2 and grid_elems(5, 70) == 2


# -- host emulations of what the device does, each able to carry ONE planted defect ---------------------------------------------------
def emulate_gemm(Am, X, dtype, defect=None):
    """the product as k_dgemm forms it, with an optional planted defect"""
    Am, X = _cm(Am, dtype), _cm(X, dtype)
    D = Am.shape[0]
    if defect == "drop_last_k_tile":       # a loop bound of D / 16 tiles instead of ⌈D / 16⌉
        keep = D // GB_K * GB_K
        Az = Am.copy(order="F")
        Az[:, keep:] = 0
        return chain(Az, X, dtype)
    if defect == "transposed_A":
        return chain(Am.T, X, dtype)
    if defect == "f32_accumulate":         # products accumulated in Float32 inside a Float64 path
        return chain(Am.astype(np.float32), X.astype(np.float32), np.float32).astype(dtype)
    assert defect is None
    return chain(Am, X, dtype)


def pool_expected(pool0, Y, ptidx, cols, vec, D):
    """the pool after a launch that owns vector `vec` of point ptidx[c] of every chain c in `cols`; pool0 is (N, NPT, PV_COUNT, D)"""
    out = pool0.copy()
    for c in cols:
        out[c, ptidx[c], vec, :] = Y[:, c]
    return out


def emulate_pool_write(pool0, Y, ptidx, cols, vec, D, defect=None):
    if defect == "neighbour_point":        # a column written to its neighbour's pool point: ptidx[col + 1] where ptidx[col] belongs
        shifted = np.roll(ptidx, -1)
        return pool_expected(pool0, Y, shifted, cols, vec, D)
    return pool_expected(pool0, Y, ptidx, cols, vec, D)


def leapfrog_replay(Minv, P, th, r, eps, n, dtype, temper=None, defect=None):
    """A NumPy transcription of dn_leapfrog's arithmetic in the element type (k_d_pre / k_d_post with the carried v ← v − ϵ/2·w, the products
    as fma chains, `a - e / 2 * b` fused as -ffp-contract=on fuses it): returns (θ, r, v) after n signed steps."""
    dt = np.dtype(dtype).type
    th, r = _cm(th, dtype).copy(order="F"), _cm(r, dtype).copy(order="F")
    e = dt(eps) * dt(1 if n > 0 else -1)
    h = np.full(th.shape, -(e / dt(2)), dtype=dtype)
    ef = np.full(th.shape, e, dtype=dtype)
    g = chain(P, th, dtype)
    v = chain(Minv, r, dtype)
    w = chain(Minv, g, dtype)
    sa = None if temper is None else dt(np.sqrt(dt(temper)))

    def scaled(x, i, second_half):     # k_d_temper: × √α while 2(i−1)+1(+1) ≤ n, ÷ √α after
        up = 2 * (i - 1) + 1 + (1 if second_half else 0) <= abs(n)
        return (x * sa if up else x / sa).astype(dtype)

    for i in range(1, abs(n) + 1):
        if sa is not None:
            r, v = scaled(r, i, False), scaled(v, i, False)
        r = host_fma(h, g, r)
        v = host_fma(h, w, v)
        th = host_fma(ef, v, th)
        g = chain(P, th, dtype)
        w = chain(Minv, g, dtype)
        r = host_fma(h, g, r)
        if not (defect == "skip_second_v_half_kick" and i == abs(n)):
            v = host_fma(h, w, v)
        if sa is not None:
            r, v = scaled(r, i, True), scaled(v, i, True)
    return th, r, v


def coldot(a, b, dtype):
    """k_d_coldot's Σ_d a[d]·b[d] per column in the element type: lane l adds d = l, l + 64, … with fused multiply-adds, then six butterfly stages"""
    a, b = _cm(a, dtype), _cm(b, dtype)
    D, n = a.shape
    s = np.zeros((64, n), dtype=dtype)
    for d0 in range(0, D, 64):
        m = min(64, D - d0)
        s[:m] = host_fma(a[d0:d0 + m], b[d0:d0 + m], s[:m])
    for j in range(6):
        s = (s + s[np.arange(64) ^ (1 << j)]).astype(dtype)
    return s[0]


def coldot_bound(a_abs_b_abs_sum, D, dtype, any_order=False):
    """|computed − exact| of Σ_d a_d·b_d as k_d_coldot adds it: ⌈D/64⌉ fused multiply-adds per lane (γ_{⌈D/64⌉} of its own terms) and six
    butterfly additions (1 + u each): γ_{⌈D/64⌉+6}·Σ|a_d||b_d| (Higham §3.1, §4.2); the scale −½ and the reference's long double sum
    (γ⁶⁴_{D+1}) ride along"""
    k = D if any_order else (D + 63) // 64 + 6           # (any_order: γ_D holds for every order of summation — the tree and epoch kernels add in their own)
    return (gam(k, U[np.dtype(dtype)]) + gam(D + 1, U_LD)) * a_abs_b_abs_sum


def test_bounds_are_not_vacuous():
    """Host emulations of the device's arithmetic pass the assertions of §1 – §3; with ONE planted defect each, they break the assertion
    meant for that defect."""
    rs = np.random.default_rng(8)
    for dtype in DTYPES:
        D = 100                                                  # D mod 16 ≠ 0
        c = gemm_case(D, np.dtype(dtype).name, "spd")
        t = gemm_case(D, np.dtype(dtype).name, "triu")
        bound = product_bound(c["S"], D, dtype)
        ok = emulate_gemm(c["A"], c["X"], dtype)
        assert same_bits(ok, c["chain"]).all() and (np.abs(ok.astype(LD) - c["exact"]) <= bound).all()
        # a dropped last k-tile: breaks the bound and the chain
        bad = emulate_gemm(c["A"], c["X"], dtype, "drop_last_k_tile")
        assert not (np.abs(bad.astype(LD) - c["exact"]) <= bound).all() and not same_bits(bad, c["chain"]).all()
        # a transposed read: invisible on the symmetric operand (which is why the triangular one is a case), breaks both on U⁻¹'s shape
        assert same_bits(emulate_gemm(c["A"], c["X"], dtype, "transposed_A"), c["chain"]).all()
        bad = emulate_gemm(t["A"], t["X"], dtype, "transposed_A")
        assert not (np.abs(bad.astype(LD) - t["exact"]) <= product_bound(t["S"], D, dtype)).all() and not same_bits(bad, t["chain"]).all()
        # a column written to its neighbour's pool point: the whole-pool comparison sees both the hole and the stray vector
        N = 9
        pool0 = np.full((N, NPT, PV_COUNT, D), np.nan, dtype=dtype)
        ptidx = rs.integers(0, NPT, N)
        ptidx[1] = (ptidx[0] + 1) % NPT
        want = pool_expected(pool0, c["chain"], ptidx, range(N), PV_G, D)
        assert same_bits(emulate_pool_write(pool0, c["chain"], ptidx, range(N), PV_G, D), want).all()
        assert not same_bits(emulate_pool_write(pool0, c["chain"], ptidx, range(N), PV_G, D, "neighbour_point"), want).all()
    # products accumulated in Float32 inside a Float64 path: breaks the Float64 bound (by nine decades) and the chain
    c = gemm_case(100, "float64", "spd")
    bad = emulate_gemm(c["A"], c["X"], np.float64, "f32_accumulate")
    assert not (np.abs(bad.astype(LD) - c["exact"]) <= product_bound(c["S"], 100, np.float64)).all() and not same_bits(bad, c["chain"]).all()
    # one half-kick of v skipped: breaks the ℓκ bound of §3; the faithful replay stays inside it
    for dtype in DTYPES:
        D, N, n = 64, 5, 7
        Minv, P, th, r, eps = velocity_case(D, N, 1e3, dtype)
        for temper in (None, 1.05):
            rep = exact_replay(Minv, P, th, r, eps, n, temper)
            for defect, inside in ((None, True), ("skip_second_v_half_kick", False)):
                _, rn, vn = leapfrog_replay(Minv, P, th, r, eps, n, dtype, temper, defect)
                lk = (-coldot(rn, vn, dtype) / np.dtype(dtype).type(2)).astype(dtype)
                err, bnd = kinetic_error_and_bound(Minv, rn, lk, rep, n, eps, dtype, temper is not None)
                assert (err <= bnd).all() == inside, (dtype, temper, defect, float((err / bnd).max()))


# -- §3 on the host: the cases, the long-double replay and the bound on ℓκ ---------------------------------------------------------
def spd_with_spectrum(lam, rs):
    """Q·diag(lam)·Qᵀ with Q the product of three Householder reflectors (dense, entries of mixed sign)"""
    D = len(lam)
    M = np.diag(np.asarray(lam, dtype=np.float64))
    for _ in range(3):
        v = rs.normal(size=(D, 1))
        v /= np.linalg.norm(v)
        M = M - 2 * v @ (v.T @ M)
        M = M - 2 * (M @ v) @ v.T
    return (M + M.T) / 2


@functools.lru_cache(maxsize=4)
def velocity_case(D, N, cond, dtype):
    """(M⁻¹, P, θ₀, r₀, ϵ): cond(M⁻¹) = cond, cond(P) = 100, ϵ at half the stability limit 2/√λ_max(M⁻¹P) of the leapfrog, all as stored
    in the element type"""
    rs = np.random.default_rng([D, N, int(cond), np.dtype(dtype).itemsize])
    Minv = np.asfortranarray(spd_with_spectrum(np.exp(np.log(cond) * (rs.permutation(D) / max(D - 1, 1)) - np.log(cond) / 2), rs), dtype=dtype)
    P = np.asfortranarray(spd_with_spectrum(np.exp(np.log(100.0) * (rs.permutation(D) / max(D - 1, 1)) - np.log(10.0)), rs), dtype=dtype)
    lam_max = float(np.max(np.abs(np.linalg.eigvals(Minv.astype(np.float64) @ P.astype(np.float64)))))
    eps = np.dtype(dtype).type(1.0 / np.sqrt(lam_max))
    th = np.asfortranarray(rs.normal(size=(D, N)), dtype=dtype)
    r = np.asfortranarray(rs.normal(size=(D, N)), dtype=dtype)
    return Minv, P, th, r, eps


def temper_scale(sa, i, second_half, n):
    """k_d_temper: the i-th leapfrog's first / second tempering of an n-step trajectory multiplies by √α while 2(i−1)+1(+1) ≤ n, divides after"""
    return sa if 2 * (i - 1) + 1 + (1 if second_half else 0) <= n else 1 / sa


def exact_replay(Minv, P, th, r, eps, n, temper=None):
    """The trajectory dn_leapfrog integrates (|n| signed steps of ϵ from (θ, r); TemperedLeapfrog(α) if `temper`), replayed in long double
    with v = M⁻¹r formed afresh at every half-kick, and along it the bound E on |v_carried − M⁻¹r| of the DEVICE's recurrence, componentwise:

        E₀ = γ_D·|M⁻¹||r₀|                                             (v₀ = M⁻¹r₀ by the product kernel, dn_velocity)
        E ← E + u·|v′| + u·|M⁻¹||r′| + |ϵ|/2·γ_D·|M⁻¹||g|               per half-kick r′ = r − ϵ/2·g, v′ = v − ϵ/2·w, w = M⁻¹g by the product kernel:
                                                                       δ′ = δ − ϵ/2·(w − M⁻¹g) + ρ_v − M⁻¹ρ_r with one rounding each of the fused
                                                                       updates, |ρ_v| ≤ u|v′|, |ρ_r| ≤ u|r′|, and |w − M⁻¹g| ≤ γ_D|M⁻¹||g|
        E ← s·E + u·|v′| + u·|M⁻¹||r′|                                  per tempering r′ = s·r, v′ = s·v (one rounding each)

    — linear in n.  The magnitudes are the replay's own, never the device's.  Also returned: the largest |ℓπ| and |ℓκ| met (§4's energy bound)."""
    dtype = Minv.dtype
    u, D = U[dtype], Minv.shape[0]
    gD = gam(D, u)
    e = LD(eps) * (1 if n > 0 else -1)
    h = e / 2
    sa = None if temper is None else LD(np.sqrt(dtype.type(temper)))
    th, r = np.asfortranarray(th, dtype=LD), np.asfortranarray(r, dtype=LD)
    g, _ = exact(P, th)
    v, Sr = exact(Minv, r)
    _, Sg = exact(Minv, g)
    E = gD * Sr
    lp_max, lk_max = np.abs((th * g).sum(axis=0)) / 2, np.abs((r * v).sum(axis=0)) / 2

    def tempering(i, second):
        nonlocal r, v, Sr, E
        if sa is not None:
            s = temper_scale(sa, i, second, abs(n))
            r, v, Sr = r * s, v * s, Sr * s
            E = s * E + u * (np.abs(v) + Sr)

    def half_kick():
        nonlocal r, v, Sr, E
        r = r - h * g
        v, Sr = exact(Minv, r)
        E = E + u * (np.abs(v) + Sr) + abs(h) * gD * Sg

    for i in range(1, abs(n) + 1):
        tempering(i, False)
        half_kick()
        th = th + e * v
        g, _ = exact(P, th)
        _, Sg = exact(Minv, g)
        half_kick()
        tempering(i, True)
        lp_max = np.maximum(lp_max, np.abs((th * g).sum(axis=0)) / 2)
        lk_max = np.maximum(lk_max, np.abs((r * v).sum(axis=0)) / 2)
    return {"E": E, "theta": th, "r": r, "lp_max": lp_max, "lk_max": lk_max}


def kinetic_error_and_bound(Minv, rn, lk, rep, n, eps, dtype, tempered):
    """(|ℓκ − K|, its bound) per chain for the device's ℓκ and its own stored r_n: K = −½ r_nᵀM⁻¹r_n exactly (long double).

    ℓκ = fl(−½·Σ r_n·v_n) with the carried v_n = M⁻¹r_n + δ_n, |δ_n| ≤ E_n (exact_replay), so
        |ℓκ − K| ≤ ½·|r_n|ᵀE_n  +  ½·γ_{⌈D/64⌉+6(+6)}·|r_n|ᵀ(|M⁻¹||r_n| + E_n)  +  (the reference's own long-double error)
    — the second term is k_d_coldot's / k_d_post's summation (coldot_bound) on Σ|r_n||v_n| ≤ |r_n|ᵀ(|M⁻¹||r_n| + E_n); TemperedLeapfrog: ℓκ is
    the ℓκ before the last tempering times f·f, f = √α or fl(1/√α), while r_n and v_n were scaled by one rounded operation each: six more
    factors (1 + δ), |δ| ≤ u, between the stored ℓκ and −½ r_nᵀv_n (Higham, Lemma 3.1)."""
    D = Minv.shape[0]
    rn = _cm(rn, dtype)
    Y, S = exact(Minv, rn)
    r_abs = np.abs(rn.astype(LD))
    K = -(rn.astype(LD) * Y).sum(axis=0) / 2
    rE, rS = (r_abs * rep["E"]).sum(axis=0), (r_abs * S).sum(axis=0)
    k = (D + 63) // 64 + 6 + (6 if tempered else 0)
    bound = rE / 2 + gam(k, U[np.dtype(dtype)]) * (rS + rE) / 2 + 2 * gam(D + 1, U_LD) * rS
    return np.abs(np.asarray(lk, dtype=LD) - K), bound


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_reference_arithmetic_stays_inside_the_velocity_bound(dtype):
    """§3 on the CPU: the NumPy transcription of k_d_pre / k_d_post in the element type keeps ℓκ inside the bound, so the bound can be asked
    of the device — and the replay's largest |ℓπ|, |ℓκ| lie under the energy bound (4/3)·H₀ of a leapfrog at half its stability limit."""
    D, N = 64, 4
    for cond in (4.0, 1e3, 1e4):
        Minv, P, th, r, eps = velocity_case(D, N, cond, dtype)
        for n, temper in ((1, None), (63, None), (255, None), (-63, None), (63, 1.05)):
            rep = exact_replay(Minv, P, th, r, eps, n, temper)
            _, rn, vn = leapfrog_replay(Minv, P, th, r, eps, n, dtype, temper)
            lk = (-coldot(rn, vn, dtype) / np.dtype(dtype).type(2)).astype(dtype)
            err, bnd = kinetic_error_and_bound(Minv, rn, lk, rep, n, eps, dtype, temper is not None)
            record_bound(f"§0 host-transcription ℓκ n={n} [{np.dtype(dtype).name}]", err, bnd)
            if temper is None:
                # ϵ·ω ≤ 1 for every mode: the leapfrog conserves, per mode, a shadow energy between (1 − (ϵω/2)²)·H and H/(1 − (ϵω/2)²), i.e.
                # every visited point has ℓπ, ℓκ ≥ −H₀/(1 − ¼) = −(4/3)·H₀
                g0, _ = exact(P, th)
                v0, _ = exact(Minv, r)
                H0 = ((th.astype(LD) * g0).sum(axis=0) + (r.astype(LD) * v0).sum(axis=0)) / 2
                assert (rep["lp_max"] <= H0 * 4 / 3).all() and (rep["lk_max"] <= H0 * 4 / 3).all()


# =====================================================================================================================
# GPU part
# =====================================================================================================================
class Findings:
    """What one measured case found.  `chain`: elements that differ from the fma chain (the one family of assertions that rests on a property
    of the MFMA units, asserted by the `…_equals_chain` tests); `other`: everything else — bounds, independence, untouched memory.  A case is
    measured once and judged by both tests."""

    def __init__(self):
        self.chain, self.other = [], []

    def bound(self, key, err, bound):
        try:
            record_bound(key, err, bound)
        except AssertionError as e:
            self.other.append(str(e))

    def bits(self, key, got, want, chain=True):
        try:
            if chain:
                record_bits(key, got, want)
            else:
                same = same_bits(got, want)
                assert same.all(), f"{key}: {int((~same).sum())} of {same.size} elements differ in their bits; first at {tuple(np.argwhere(~same)[0])}"
        except AssertionError as e:
            (self.chain if chain else self.other).append(str(e))

    def check(self, cond, msg):
        if not cond:
            self.other.append(msg)


_FOUND = {}
_STATE = {}


def found(group, measure):
    if group not in _FOUND:
        _FOUND[group] = measure()
    return _FOUND[group]


def assert_none(msgs):
    assert not msgs, f"{len(msgs)} finding(s):\n" + "\n".join(msgs[:12])


@pytest.fixture(scope="module")
def probe(hip):
    import torch

    from ahmc_amd import build as B
    from ahmc_amd.hipmod import Module

    torch.cuda.init()
    if "probe" not in _STATE:
        _STATE["probe"] = Module(B.build_probe_object(PROBE))
    return _STATE["probe"]


def n_cu(lib):
    import torch

    if not lib.backend.startswith("hip"):  # (a dry run of the test code on the CPU checker)
        return 256
    return torch.cuda.get_device_properties(0).multi_processor_count


def dev(a):
    """a host array as device memory in column-major order (ints as int32)"""
    import torch

    a = np.asarray(a)
    if a.dtype.kind in "iu":
        a = a.astype(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a.reshape(-1, order="F"))).cuda()


def nan_buffer(n, dtype):
    import torch

    return torch.full((int(n),), float("nan"), dtype=torch.float64 if np.dtype(dtype) == np.float64 else torch.float32, device="cuda")


def host(t, shape):
    """device memory as a host array of `shape`, column-major"""
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().reshape(shape, order="F")


NULL = C.c_void_p(None)


def launch_gemm(probe, kernel, dtype, A_d, X_d, Y_d, D, N, idx=None, A2=None, Y2=None, ptidx=None, xps=0, yps=0, xcs=0, ycs=0):
    """one launch as dn_gemm makes it (its grid, its defaults for the strides of plain (D, N) arrays)"""
    probe.launch(kernel_name(kernel, dtype), gemm_grid(kernel, D, N, two=A2 is not None), 256, A_d, X_d, Y_d, int(D), np.int64(N),
                 NULL if idx is None else idx, NULL if A2 is None else A2, NULL if Y2 is None else Y2, NULL if ptidx is None else ptidx,
                 np.int64(xps), np.int64(yps), np.int64(xcs or D), np.int64(ycs or D))


def plain_product(probe, kernel, dtype, A_d, X_d, D, N, margin=3):
    """(Y (D, N), the margin columns behind it) of a plain launch into a NaN-filled array of N + margin columns"""
    Y_d = nan_buffer(D * (N + margin), dtype)
    launch_gemm(probe, kernel, dtype, A_d, X_d, Y_d, D, N)
    Y = host(Y_d, (D, N + margin))
    return Y[:, :N], Y[:, N:]


# ------------------------------------------------------------------------------------------------
# §1  the two GEMM kernels alone
# ------------------------------------------------------------------------------------------------
def measure_plain(probe, kernel, dtype, D):
    f = Findings()
    dtn = np.dtype(dtype).name
    for kind in KINDS:
        c = gemm_case(D, dtn, kind)
        key = f"§1 {kernel} plain {kind} [{dtn}]"
        A_d, X_d = dev(c["A"]), dev(c["X"])
        bound = product_bound(c["S"], D, dtype)
        widest = None
        for N in sorted(n_list(D), reverse=True):
            Y, margin = plain_product(probe, kernel, dtype, A_d, X_d, D, N)
            f.check(np.isnan(margin).all(), f"{key} N={N}: columns ≥ N were written")
            f.check(np.isfinite(Y).all(), f"{key} N={N}: an owned element was not written (or is not finite)")
            if np.isfinite(Y).all():
                f.bound(key, np.abs(Y.astype(LD) - c["exact"][:, :N]), bound[:, :N])
            f.bits(key, Y, c["chain"][:, :N])
            if widest is None:
                widest = Y
            else:  # a column's result depends neither on N nor on which tile of the launch it falls into
                f.bits(f"{key} N={N} against N={widest.shape[1]}", Y, widest[:, :N], chain=False)
    return f


GEMM_PARAMS = [pytest.param(k, dt, D, id=f"{k}-{_sfx(dt)}-D{D}") for k in KERNELS for dt in DTYPES for D in D_ALL]


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,dtype,D", GEMM_PARAMS)
def test_gemm_bound_independence_and_untouched_memory(probe, kernel, dtype, D):
    """every element of Y within γ_D·|A|·|X| of the exact product; the same bits at every N; NaN left in every column ≥ N"""
    assert_none(found(("plain", kernel, np.dtype(dtype).name, D), lambda: measure_plain(probe, kernel, dtype, D)).other)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,dtype,D", GEMM_PARAMS)
def test_gemm_equals_chain(probe, kernel, dtype, D):
    """Y == chain(A, X) bit for bit"""
    assert_none(found(("plain", kernel, np.dtype(dtype).name, D), lambda: measure_plain(probe, kernel, dtype, D)).chain)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("D", D_ALL)
def test_gemm_kernels_agree(probe, D, dtype):
    """dn_gemm's claim — "same arithmetic per column, so results do not depend on which kernel ran": k_dgemm == k_dgemm_small bit for bit"""
    dtn = np.dtype(dtype).name
    for kind in KINDS:
        c = gemm_case(D, dtn, kind)
        A_d, X_d = dev(c["A"]), dev(c["X"])
        N = max(n_list(D))
        big, _ = plain_product(probe, "k_dgemm", dtype, A_d, X_d, D, N)
        small, _ = plain_product(probe, "k_dgemm_small", dtype, A_d, X_d, D, N)
        same = same_bits(big, small)
        assert same.all(), f"{kind} D={D} [{dtn}]: {int((~same).sum())} of {same.size} elements differ between the two kernels"


def measure_modes(probe, kernel, dtype, D):
    """the addressing modes: a shuffled `idx` shorter than the array, `A2/Y2`, and the point pool with the engine's strides — X plain and Y
    in the pool (dn_staged_w), both in the pool (the tree step; with A2/Y2 its fused launch), X in the pool and Y plain — each with and
    without `idx`, different points per column.  Every result against the chain, against a plain launch of the same kernel, and the whole
    destination (array or pool) against what it held before wherever the launch owns nothing."""
    f = Findings()
    dtn = np.dtype(dtype).name
    rs = np.random.default_rng([D, 77])
    PS, itemsize = PV_COUNT * D, np.dtype(dtype).itemsize
    CS = NPT * PS
    cs, ct = gemm_case(D, dtn, "spd"), gemm_case(D, dtn, "triu")
    NC_MAX = max(N_MODES) + 9
    X = np.asfortranarray(cs["X"][:, :NC_MAX])
    for a_kind, Am, A2m in (("spd", cs["A"], ct["A"]), ("triu", ct["A"], cs["A"])):
        want1, want2 = chain(Am, X, dtype), chain(A2m, X, dtype)
        ex1, S1 = exact(Am, X)
        ex2, S2 = exact(A2m, X)
        b1, b2 = product_bound(S1, D, dtype), product_bound(S2, D, dtype)
        A_d, A2_d = dev(Am), dev(A2m)
        for N in N_MODES:
            NC = N + 9                                           # columns of the arrays / chains of the pool; N of them are listed
            X_d = dev(X[:, :NC])
            plain1, _ = plain_product(probe, kernel, dtype, A_d, X_d, D, NC)
            plain2, _ = plain_product(probe, kernel, dtype, A2_d, X_d, D, NC)
            idx = rs.permutation(NC)[:N]
            idx_d = dev(idx)
            ptidx = rs.integers(0, NPT, NC)
            pt_d = dev(ptidx)
            rest = np.setdiff1d(np.arange(NC), idx)

            def judge(mode, Y, cols, which=1):
                key = f"§1 {kernel} {mode} [{dtn}]"
                want, ex, b, plain = (want1, ex1, b1, plain1) if which == 1 else (want2, ex2, b2, plain2)
                f.check(np.isfinite(Y[:, cols]).all(), f"{key} {a_kind} N={N}: an owned element was not written (or is not finite)")
                if np.isfinite(Y[:, cols]).all():
                    f.bound(key, np.abs(Y[:, cols].astype(LD) - ex[:, :NC][:, cols]), b[:, :NC][:, cols])
                f.bits(key, Y[:, cols], want[:, :NC][:, cols])
                f.bits(f"{key} {a_kind} N={N} against a plain launch", Y[:, cols], plain[:, cols], chain=False)

            # a shuffled list of N of the NC columns
            Y_d = nan_buffer(D * NC, dtype)
            launch_gemm(probe, kernel, dtype, A_d, X_d, Y_d, D, N, idx=idx_d)
            Y = host(Y_d, (D, NC))
            f.check(np.isnan(Y[:, rest]).all(), f"§1 {kernel} idx {a_kind} N={N}: columns not in idx were written")
            judge("idx", Y, idx)
            # two products in one launch, with and without the list
            for cols, ix in ((np.arange(N), None), (idx, idx_d)):
                Y_d, Y2_d = nan_buffer(D * NC, dtype), nan_buffer(D * NC, dtype)
                launch_gemm(probe, kernel, dtype, A_d, X_d, Y_d, D, N, idx=ix, A2=A2_d, Y2=Y2_d)
                Y, Y2 = host(Y_d, (D, NC)), host(Y2_d, (D, NC))
                others = np.setdiff1d(np.arange(NC), cols)
                f.check(np.isnan(Y[:, others]).all() and np.isnan(Y2[:, others]).all(), f"§1 {kernel} A2/Y2 {a_kind} N={N}: columns not owned were written")
                judge("A2/Y2" + ("" if ix is None else "+idx"), Y, cols, 1)
                judge("A2/Y2" + ("" if ix is None else "+idx"), Y2, cols, 2)
            # the point pool [chain][point][vector][D]
            pool0 = np.full((D, PV_COUNT, NPT, NC), np.nan, dtype=dtype, order="F")      # column-major (d, vector, point, chain) = [chain][point][vector][d]
            for cidx in range(NC):
                pool0[:, PV_TH, ptidx[cidx], cidx] = X[:, cidx]
            for cols, ix in ((np.arange(N), None), (idx, idx_d)):
                tag = "" if ix is None else "+idx"
                for mode in ("pool x plain y pool", "pool both", "pool both A2/Y2", "pool x pool y plain"):
                    pool_d = dev(pool0)
                    x_pool, y_pool, two = mode != "pool x plain y pool", mode != "pool x pool y plain", mode == "pool both A2/Y2"
                    Yplain_d = None if y_pool else nan_buffer(D * NC, dtype)
                    launch_gemm(probe, kernel, dtype, A_d, pool_d[PV_TH * D:] if x_pool else X_d, pool_d[PV_G * D:] if y_pool else Yplain_d, D, N, idx=ix,
                                A2=A2_d if two else None, Y2=pool_d[PV_W * D:] if two else None, ptidx=pt_d,
                                xps=PS if x_pool else 0, xcs=CS if x_pool else D, yps=PS if y_pool else 0, ycs=CS if y_pool else D)
                    pool = host(pool_d, pool0.shape)
                    key = f"§1 {kernel} {mode}{tag} [{dtn}]"
                    mask = np.zeros(pool0.shape, dtype=bool)                               # what the launch owns
                    if y_pool:
                        mask[:, PV_G, ptidx[cols], cols] = True
                        if two:
                            mask[:, PV_W, ptidx[cols], cols] = True
                        judge(mode + tag, pool[:, PV_G, ptidx, np.arange(NC)], cols, 1)
                        if two:
                            judge(mode + tag, pool[:, PV_W, ptidx, np.arange(NC)], cols, 2)
                    else:
                        Y = host(Yplain_d, (D, NC))
                        f.check(np.isnan(Y[:, np.setdiff1d(np.arange(NC), cols)]).all(), f"{key} {a_kind} N={N}: columns not owned were written")
                        judge(mode + tag, Y, cols, 1)
                    f.check(same_bits(pool[~mask], pool0[~mask]).all(), f"{key} {a_kind} N={N}: the pool changed outside the points ptidx[col] of the listed columns")
    return f


MODE_PARAMS = [pytest.param(k, dt, D, id=f"{k}-{_sfx(dt)}-D{D}") for k in KERNELS for dt in DTYPES for D in D_MODES]


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,dtype,D", MODE_PARAMS)
def test_gemm_addressing_modes(probe, kernel, dtype, D):
    """`idx`, `A2/Y2` and the point pool: the bound, the bits of a plain launch, and nothing written that the launch does not own"""
    assert_none(found(("modes", kernel, np.dtype(dtype).name, D), lambda: measure_modes(probe, kernel, dtype, D)).other)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,dtype,D", MODE_PARAMS)
def test_gemm_addressing_modes_equal_chain(probe, kernel, dtype, D):
    assert_none(found(("modes", kernel, np.dtype(dtype).name, D), lambda: measure_modes(probe, kernel, dtype, D)).chain)


def measure_large_index(probe):
    """D = 64, N = 2²⁵ + 70 in Float32: D·N = 2³¹ + 4 480 elements, 8.6 GB per array.  Checked: the first 64 columns, the columns on either side of
    byte offset 2³² (column 2²⁴) and of element offset 2³¹ (column 2²⁵), the last 70, and a margin of 64 NaN columns behind Y.  (Element offset
    2³² lies outside an array of this size.)"""
    import torch

    f = Findings()
    D, N, margin, dtype = 64, 2 ** 25 + 70, 64, np.float32
    c = gemm_case(D, "float32", "triu")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    X_d = torch.randn(D * N, dtype=torch.float32, device="cuda", generator=gen)
    Y_d = nan_buffer(D * (N + margin), dtype)
    launch_gemm(probe, "k_dgemm", dtype, dev(c["A"]), X_d, Y_d, D, N)
    torch.cuda.synchronize()
    key = "§1 k_dgemm plain large-index [float32]"
    for lo, hi in ((0, 64), (2 ** 24 - 2, 2 ** 24 + 2), (2 ** 25 - 2, N)):
        X = X_d[lo * D:hi * D].cpu().numpy().reshape((D, hi - lo), order="F")
        Y = Y_d[lo * D:hi * D].cpu().numpy().reshape((D, hi - lo), order="F")
        ex, S = exact(c["A"], X)
        f.check(np.isfinite(Y).all(), f"{key}: columns {lo}…{hi} hold a non-finite element")
        if np.isfinite(Y).all():
            f.bound(key, np.abs(Y.astype(LD) - ex), product_bound(S, D, dtype))
        f.bits(key, Y, chain(c["A"], X, dtype))
    f.check(bool(torch.isnan(Y_d[N * D:]).all()), f"{key}: the NaN margin behind column N was written")
    f.check(int(torch.isnan(Y_d[:N * D]).sum()) == 0, f"{key}: some owned element was left unwritten")
    return f


def _large_index_findings(probe):
    import torch

    free, _ = torch.cuda.mem_get_info()
    if free < 40e9:
        pytest.skip(f"the device has {free / 1e9:.0f} GB free, the large-index case wants 40 GB")
    return found(("large",), lambda: measure_large_index(probe))


@pytest.mark.gpu
def test_gemm_large_index(probe):
    assert_none(_large_index_findings(probe).other)


@pytest.mark.gpu
def test_gemm_large_index_equals_chain(probe):
    assert_none(_large_index_findings(probe).chain)


# ------------------------------------------------------------------------------------------------
# §2  the same products through the C ABI (step-synchronous path)
# ------------------------------------------------------------------------------------------------
def dense_engine(hip, Minv, P, N, dtype, eps, temper=None, seed=11):
    lf = A.Leapfrog(np.full(N, eps)) if temper is None else A.TemperedLeapfrog(np.full(N, eps), temper)
    e = A.Engine(A.Hamiltonian(A.DenseEuclideanMetric(np.asfortranarray(Minv)), A.DenseGaussian(np.asfortranarray(P))), N, dtype=dtype, rng=A.PhiloxRNG(seed), lib=hip)
    e.set_integrator(lf)
    return e


def judge_point(f, key, z, Minv, P, dtype, check_lk=True, any_order=False):
    """the caches of a phase point against the device's own θ, r as stored: ∇ℓπ == −chain(P, θ) bit for bit (the C ABI keeps g = −∇ℓπ = Pθ, and
    phasepoint() hands it out as stored: `gradient` == chain(P, θ)); ℓπ (and ℓκ where v = M⁻¹r was
    formed afresh) inside the bound of the dot product:

        ℓπ = fl(−½·Σ_d θ_d·g_d), g the device's product: |ℓπ − (−½ θᵀPθ)| ≤ ½·γ_{⌈D/64⌉+6}·Σ|θ||g| + ½·|θ|ᵀ|g − Pθ|   (coldot_bound; the halving is exact)
                                                                         ≤ ½·γ_{⌈D/64⌉+6}·|θ|ᵀ(|Pθ| + b) + ½·|θ|ᵀb,   b = γ_D·|P||θ|   (product_bound)"""
    D = P.shape[0]
    th, r = _cm(z.theta, dtype), _cm(z.r, dtype)
    f.bits(key + " gradient", _cm(z.lp.gradient, dtype), chain(P, th, dtype))
    for name, val, Am, x in (("ℓπ", z.lp.value, P, th),) + ((("ℓκ", z.lk.value, Minv, r),) if check_lk else ()):
        Y, S = exact(Am, x)
        b = product_bound(S, D, dtype)
        xa = np.abs(x.astype(LD))
        want = -(x.astype(LD) * Y).sum(axis=0) / 2
        bound = (coldot_bound((xa * (np.abs(Y) + b)).sum(axis=0), D, dtype, any_order) + (xa * b).sum(axis=0)) / 2
        f.check(np.isfinite(np.asarray(val, dtype=np.float64)).all(), f"{key} {name}: not finite")
        if np.isfinite(np.asarray(val, dtype=np.float64)).all():
            f.bound(key + " " + name, np.abs(np.asarray(val, dtype=LD) - want), bound)


ENGINE_SHAPES = ((5, 70), (64, 70), (64, 16400), (200, 513), (512, 70), (512, 2100))


def measure_engine(hip, D, N, dtype):
    f = Findings()
    dtn = np.dtype(dtype).name
    Minv, P, _, _, eps = velocity_case(D, 4, 1e3, dtype)
    rs = np.random.default_rng([D, N, 3])
    th, r = np.asfortranarray(rs.normal(size=(D, N)), dtype=dtype), np.asfortranarray(rs.normal(size=(D, N)), dtype=dtype)
    e = dense_engine(hip, Minv, P, N, dtype, eps)
    small = gemm_takes_small(D, N, n_cu(hip))
    before = (e.info("dense_gemm_launches"), e.info("dense_gemm_small_launches"))
    e.set_position(th, r)
    z0 = e.phasepoint()
    after = (e.info("dense_gemm_launches"), e.info("dense_gemm_small_launches"))
    # set_position: g = Pθ and v = M⁻¹r, both by the kernel dn_gemm's rule picks
    f.check((after[0] - before[0], after[1] - before[1]) == ((0, 2) if small else (2, 0)),
            f"D={D} N={N}: set_position launched (k_dgemm, k_dgemm_small) {after[0] - before[0], after[1] - before[1]} times, expected {'small' if small else 'large'} twice")
    kname = "k_dgemm_small" if small else "k_dgemm"
    key = f"§2 engine {kname} set_position [{dtn}]"
    f.check(same_bits(_cm(z0.theta, dtype), th).all() and same_bits(_cm(z0.r, dtype), r).all(), f"{key}: θ, r are not what was set")
    judge_point(f, key, z0, Minv, P, dtype)
    # step(1) from the fresh point — the only place v is observable: θ′ = fl(θ + ϵ·v′), v′ = fl(v₀ − ϵ/2·w₀), v₀ = M⁻¹r + δ_v, w₀ = M⁻¹g + δ_w with g the
    # device's own gradient, |δ_v| ≤ γ_D·|M⁻¹||r|, |δ_w| ≤ γ_D·|M⁻¹||g|.  With V = M⁻¹(r − ϵ/2·g) exactly and S_V = |M⁻¹|(|r| + ϵ/2·|g|):
    #   |(θ′ − θ)/ϵ − V| ≤ γ_D·S_V + u·|v′| + u·|θ′|/ϵ,   |v′| ≤ (|V| + γ_D·S_V)/(1 − u)
    # (the difference and the quotient are formed in long double; r′ = fl(r − ϵ/2·g) is the third element-wise operation, checked on its own)
    e.step(1)
    z1 = e.phasepoint()
    u = U[np.dtype(dtype)]
    g0 = _cm(z0.lp.gradient, dtype).astype(LD)                 # g = −∇ℓπ = Pθ as stored
    h = LD(eps) / 2
    V, _ = exact(Minv, np.asfortranarray(r.astype(LD) - h * g0))
    _, S_V = exact(Minv, np.asfortranarray(np.abs(r.astype(LD)) + h * np.abs(g0)))
    pb = product_bound(S_V, D, dtype)
    th1 = _cm(z1.theta, dtype).astype(LD)
    q = (th1 - th.astype(LD)) / LD(eps)
    f.bound(f"§2 engine {kname} step(1) velocity [{dtn}]", np.abs(q - V), pb + u * (np.abs(V) + pb) / (1 - u) + u * np.abs(th1) / LD(eps))
    # r₁ = fl(fl(r − ϵ/2·g₀) − ϵ/2·g₁), g₁ the device's gradient at θ₁: two fused operations
    g1 = _cm(z1.lp.gradient, dtype).astype(LD)
    r_half = r.astype(LD) - h * g0
    r1 = r_half - h * g1
    f.bound(f"§2 engine {kname} step(1) momentum [{dtn}]", np.abs(_cm(z1.r, dtype).astype(LD) - r1), u * np.abs(r_half) * (1 + u) + u * np.abs(r1) / (1 - u) + 4 * U_LD * np.abs(r1))
    judge_point(f, f"§2 engine {kname} step(1) [{dtn}]", z1, Minv, P, dtype, check_lk=False)
    e.step(4)
    judge_point(f, f"§2 engine {kname} step(5) [{dtn}]", e.phasepoint(), Minv, P, dtype, check_lk=False)
    e.close()
    return f


ENGINE_PARAMS = [pytest.param(D, N, dt, id=f"D{D}-N{N}-{_sfx(dt)}") for dt in DTYPES for D, N in ENGINE_SHAPES]


@pytest.mark.gpu
@pytest.mark.parametrize("D,N,dtype", ENGINE_PARAMS)
def test_engine_products_bounds_and_kernel_choice(hip, D, N, dtype):
    """set_position and the first leapfrog through the C ABI: which kernel dn_gemm took, ℓπ and ℓκ inside the dot product's bound, the velocity of
    the first half-step against the exact M⁻¹(r − ϵ/2·g)"""
    assert_none(found(("engine", D, N, np.dtype(dtype).name), lambda: measure_engine(hip, D, N, dtype)).other)


@pytest.mark.gpu
@pytest.mark.parametrize("D,N,dtype", ENGINE_PARAMS)
def test_engine_gradient_equals_chain(hip, D, N, dtype):
    """∇ℓπ == −chain(P, θ) bit for bit after set_position, step(1) and step(5)"""
    assert_none(found(("engine", D, N, np.dtype(dtype).name), lambda: measure_engine(hip, D, N, dtype)).chain)


def test_engine_shapes_reach_both_kernels():
    """with the 256 CUs of an MI355X the §2 grid makes dn_gemm choose each kernel (the GPU test asserts the launch counters)"""
    picks = {gemm_takes_small(D, N, 256) for D, N in ENGINE_SHAPES}
    assert picks == {True, False}


# ------------------------------------------------------------------------------------------------
# §3  the carried velocity after long trajectories
# ------------------------------------------------------------------------------------------------
VELOCITY_STEPS = (1, 7, 63, 255, 1023, -255)
VELOCITY_CHAINS = 6
TEMPER_ALPHA = 1.05


def measure_velocity(hip, D, cond, dtype, tempered):
    f = Findings()
    dtn = np.dtype(dtype).name
    N = VELOCITY_CHAINS
    Minv, P, th, r, eps = velocity_case(D, N, cond, dtype)
    temper = TEMPER_ALPHA if tempered else None
    e = dense_engine(hip, Minv, P, N, dtype, eps, temper)
    for n in VELOCITY_STEPS:
        e.set_position(th, r)
        e.step(n)
        z = e.phasepoint()
        key = f"§3 {'tempered' if tempered else 'leapfrog'} n={n} [{dtn}]"
        finite = all(np.isfinite(np.asarray(a, dtype=np.float64)).all() for a in (z.theta, z.r, z.lk.value))
        f.check(finite, f"{key} D={D} cond={cond:g}: non-finite point")
        if not finite:
            continue
        judge_point(f, key, z, Minv, P, dtype, check_lk=False)
        rep = exact_replay(Minv, P, th, r, eps, n, temper)
        err, bnd = kinetic_error_and_bound(Minv, z.r, z.lk.value, rep, n, eps, dtype, tempered)
        f.bound(key + " ℓκ", err, bnd)
    e.close()
    return f


VELOCITY_PARAMS = [pytest.param(D, cond, dt, t, id=f"D{D}-cond{cond:g}-{_sfx(dt)}-{'tempered' if t else 'plain'}")
                   for dt in DTYPES for D in (64, 256, 512) for cond in (4.0, 1e3, 1e4) for t in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,cond,dtype,tempered", VELOCITY_PARAMS)
def test_carried_velocity_stays_consistent(hip, D, cond, dtype, tempered):
    """after n ∈ {1, 7, 63, 255, 1 023, −255} leapfrogs at half the stability limit, ℓκ — formed from the CARRIED v — is −½ r_nᵀM⁻¹r_n of the device's own
    r_n inside ½|r_n|ᵀE_n + the dot product's term (exact_replay, kinetic_error_and_bound); ℓπ inside its bound"""
    assert_none(found(("velocity", D, cond, np.dtype(dtype).name, tempered), lambda: measure_velocity(hip, D, cond, dtype, tempered)).other)


@pytest.mark.gpu
@pytest.mark.parametrize("D,cond,dtype,tempered", VELOCITY_PARAMS)
def test_gradient_after_long_trajectories_equals_chain(hip, D, cond, dtype, tempered):
    assert_none(found(("velocity", D, cond, np.dtype(dtype).name, tempered), lambda: measure_velocity(hip, D, cond, dtype, tempered)).chain)


# ------------------------------------------------------------------------------------------------
# §4  what a NUTS transition leaves behind: the tree kernel and the epoch kernels
# ------------------------------------------------------------------------------------------------
# (label, D, dtype, environment, criterion): the step-synchronous kernels, round 4's k_dense_epoch, every shape of AHMC_EPOCH2_SHAPES and the
# AHMC_EPOCH2_CRIT_SHAPES once each (ahmc_dense_host.hpp)
def _transition_cases():
    f64, f32 = np.float64, np.float32
    step, v1, v2 = {"AHMC_DENSE_EPOCH": "0"}, {"AHMC_DENSE_EPOCH": "1"}, {"AHMC_DENSE_EPOCH": "1", "AHMC_DENSE_EPOCH_V": "2"}
    cases = [("step", 256, f64, step, "generalised"), ("step", 512, f32, step, "generalised"),
             ("epoch", 256, f64, v1, "generalised"), ("epoch", 512, f64, v1, "generalised"),
             ("epoch2", 384, f64, v2, "generalised"),
             ("epoch2_nct1", 512, f64, dict(v2, AHMC_DENSE_EPOCH_NCT="1"), "generalised"), ("epoch2_nct2", 512, f64, dict(v2, AHMC_DENSE_EPOCH_NCT="2"), "generalised")]
    cases += [("epoch2", D, f32, v2, "generalised") for D in (256, 384, 512, 768, 1024)]
    cases += [("epoch2_" + c, 512, dt, v2, c) for dt in (f64, f32) for c in ("classic", "strict")]
    return cases


TRANSITION_CASES = _transition_cases()
TRANSITION_CHAINS = 150        # two pipelines of 75: two (or four) full workgroups of 32 (16) chains and one partly empty


def nuts_kinetic_bound(Minv, P, rn, n_steps, H0, eps, dtype):
    """The §3 bound on |ℓκ − (−½ r_nᵀM⁻¹r_n)| in its normwise form, for a point a NUTS transition returns.  The fresh momentum is not observable, so the
    magnitudes cannot come from a replay; they come from the energy.  With ϵ·ω ≤ 1 for every mode of the quadratic Hamiltonian the leapfrog conserves,
    mode by mode, a shadow energy that differs from the mode's energy by a factor of at most 1/(1 − (ϵω/2)²) ≤ 4/3, so every point of the trajectory has
    ½θᵀPθ ≤ (4/3)·H₀ and ½rᵀM⁻¹r ≤ (4/3)·H₀ (checked against the long-double replay in test_reference_arithmetic_stays_inside_the_velocity_bound), i.e.

        ‖θ‖² ≤ (8/3)·H₀/λ_min(P),   ‖r‖² ≤ (8/3)·H₀/λ_min(M⁻¹),   ‖v‖² = ‖M⁻¹r‖² ≤ λ_max(M⁻¹)·(8/3)·H₀.

    A transition's products are g = chain(P, θ′) and w = chain(C, θ′) with C = chain(M⁻¹, P) formed once on the device (dn_refresh_fused), so
    |w − M⁻¹g| ≤ |C − M⁻¹P||θ′| + γ_D|C||θ′| + |M⁻¹|·γ_D|P||θ′| ≤ (3γ_D + γ_D²)·|M⁻¹||P||θ′|, and the recurrence of exact_replay becomes, in 2-norms,

        ‖E_n‖ ≤ γ_D·‖|M⁻¹|‖·‖r‖ + 2n·( u·‖v‖ + u·‖|M⁻¹|‖·‖r‖ + ϵ/2·(3γ_D + γ_D²)·‖|M⁻¹|‖·‖|P|‖·‖θ‖ )

    with the maxima above (n = the transition's n_steps bounds the leapfrogs between the fresh momentum and any point of the tree, in either direction).
    Then |ℓκ − K| ≤ ½‖r_n‖‖E_n‖ + ½γ_D·‖r_n‖(‖|M⁻¹|‖‖r_n‖ + ‖E_n‖): the sum r·v in ANY order (the tree and epoch kernels add in their own).  The
    eigenvalues and norms are LAPACK's in double of the matrices as stored (relative 1e-13: far below anything here)."""
    D = Minv.shape[0]
    u = U[np.dtype(dtype)]
    gD = gam(D, u)
    M64, P64 = Minv.astype(np.float64), P.astype(np.float64)
    lamM, lamP = np.linalg.eigvalsh(M64), np.linalg.eigvalsh(P64)
    nM, nP = LD(np.linalg.norm(np.abs(M64), 2)), LD(np.linalg.norm(np.abs(P64), 2))
    Hb = np.maximum(np.asarray(H0, dtype=LD), 0) * 8 / 3
    th_max, r_max, v_max = np.sqrt(Hb / LD(lamP[0])), np.sqrt(Hb / LD(lamM[0])), np.sqrt(Hb * LD(lamM[-1]))
    per_half = u * v_max + u * nM * r_max + LD(eps) / 2 * (3 * gD + gD * gD) * nM * nP * th_max
    E = gD * nM * r_max + 2 * np.asarray(n_steps, dtype=LD) * per_half
    rn = _cm(rn, dtype)
    Y, S = exact(Minv, rn)
    K = -(rn.astype(LD) * Y).sum(axis=0) / 2
    r2 = np.sqrt((rn.astype(LD) ** 2).sum(axis=0))
    bound = r2 * E / 2 + gD * r2 * (nM * r2 + E) / 2 + 2 * gam(D + 1, U_LD) * (np.abs(rn.astype(LD)) * S).sum(axis=0)
    return K, bound


def measure_transitions(hip, monkeypatch, label, D, dtype, env, criterion):
    f = Findings()
    dtn = np.dtype(dtype).name
    N = TRANSITION_CHAINS
    for var in ("AHMC_DENSE_EPOCH", "AHMC_DENSE_EPOCH_V", "AHMC_DENSE_EPOCH_NCT", "AHMC_DENSE_EPOCH_WPE", "AHMC_DENSE_CHUNK"):
        monkeypatch.delenv(var, raising=False)
    for var, val in env.items():
        monkeypatch.setenv(var, val)
    monkeypatch.setenv("AHMC_DENSE_EPOCH_MIN", "32")
    TC = {"generalised": A.GeneralisedNoUTurn, "classic": A.ClassicNoUTurn, "strict": A.StrictGeneralisedNoUTurn}[criterion]
    depth_seen = 0
    for cond in (4.0, 1e3):
        Minv, P, _, _, eps = velocity_case(D, 4, cond, dtype)
        for sampler in (A.MultinomialTS, A.SliceTS):
            key = f"§4 {label} D={D} {sampler.__name__} [{dtn}]"
            rs = np.random.default_rng([D, int(cond), 9])
            lf = A.Leapfrog(np.full(N, eps))
            e = A.Engine(A.Hamiltonian(A.DenseEuclideanMetric(Minv), A.DenseGaussian(P)), N, dtype=dtype, rng=A.PhiloxRNG(31), lib=hip)
            e.set_integrator(lf)
            e.set_position(np.asfortranarray(rs.normal(size=(D, N)), dtype=dtype))
            e.run(A.HMCKernel(A.Trajectory(sampler, lf, TC(max_depth=10, delta_max=1000.0))), 3)
            e.sync()
            z, st = e.phasepoint(), e.stats()
            f.check((e.info("dense_epoch_launches") > 0) == (label != "step"), f"{key} cond={cond:g}: dense_epoch_launches = {e.info('dense_epoch_launches')}")
            e.close()
            finite = all(np.isfinite(np.asarray(a, dtype=np.float64)).all() for a in (z.theta, z.r, z.lp.value, z.lk.value, st["hamiltonian_energy"]))
            f.check(finite and not st["numerical_error"].any(), f"{key} cond={cond:g}: non-finite point or numerical_error")
            if not finite:
                continue
            judge_point(f, key, z, Minv, P, dtype, check_lk=False, any_order=True)
            lp, lk, H = (np.asarray(a, dtype=LD) for a in (z.lp.value, z.lk.value, st["hamiltonian_energy"]))
            # H = fl(−ℓπ − ℓκ) of the returned point: one rounding of the sum
            f.bound(key + " energy", np.abs(H - (-lp - lk)), U[np.dtype(dtype)] * np.abs(-lp - lk))
            ns, depth = st["n_steps"].astype(np.int64), st["tree_depth"].astype(np.int64)
            # tree_depth j counts the doublings that completed (src/trajectory.jl:708-709): they hold 2^j − 1 leapfrogs; a last doubling that ended early — a
            # turn or a divergence inside it — adds between 1 and 2^j more without raising j.  So 2^j − 1 ≤ n_steps ≤ 2^(j+1) − 1, and ≤ 2^max_depth − 1.
            f.check(((ns >= 2 ** depth - 1) & (ns <= 2 ** (depth + 1) - 1) & (ns <= 1023)).all() and (depth >= 0).all() and (depth <= 10).all(),
                    f"{key} cond={cond:g}: n_steps / tree_depth disagree")
            K, bound = nuts_kinetic_bound(Minv, P, z.r, ns, H - np.asarray(st["hamiltonian_energy_error"], dtype=LD), eps, dtype)
            f.bound(key + " ℓκ", np.abs(lk - K), bound)
            depth_seen = max(depth_seen, int(depth.max()))
    f.check(depth_seen >= 7, f"§4 {label} D={D} [{dtn}]: no tree deeper than {depth_seen}: the ℓκ bound was not exercised with n in the hundreds")
    return f


TRANSITION_PARAMS = [pytest.param(*c, id=f"{c[0]}-D{c[1]}-{_sfx(c[2])}") for c in TRANSITION_CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("label,D,dtype,env,criterion", TRANSITION_PARAMS)
def test_transition_leaves_a_consistent_point(hip, monkeypatch, label, D, dtype, env, criterion):
    """three NUTS transitions (max_depth 10, fixed ϵ at half the stability limit, 150 chains, MultinomialTS and SliceTS, cond(M⁻¹) = 4 and 1e3) on the
    step-synchronous kernels, k_dense_epoch and every k_dense_epoch2 shape: for every chain ℓπ and ℓκ of the returned point inside their bounds,
    hamiltonian_energy == −ℓπ − ℓκ to one rounding, 2^depth − 1 ≤ n_steps ≤ 2^(depth+1) − 1, the engine asked for is the engine that ran, some tree of depth ≥ 7"""
    assert_none(found(("nuts", label, D, np.dtype(dtype).name), lambda: measure_transitions(hip, monkeypatch, label, D, dtype, env, criterion)).other)


@pytest.mark.gpu
@pytest.mark.parametrize("label,D,dtype,env,criterion", TRANSITION_PARAMS)
def test_transition_gradient_equals_chain(hip, monkeypatch, label, D, dtype, env, criterion):
    """∇ℓπ of the returned point == −chain(P, θ) bit for bit: the swizzled operand layout and the product loop of every epoch instantiation, to the last bit"""
    assert_none(found(("nuts", label, D, np.dtype(dtype).name), lambda: measure_transitions(hip, monkeypatch, label, D, dtype, env, criterion)).chain)


# ------------------------------------------------------------------------------------------------
# §2 (continued)  the fresh momentum r = U⁻¹z
# ------------------------------------------------------------------------------------------------
def cholesky_upper_ld(M):
    """(U, U⁻¹) in long double: UᵀU = M, U upper triangular (row by row), and its inverse by back substitution on the unit vectors"""
    M = np.asarray(M, dtype=LD)
    D = M.shape[0]
    Uf = np.zeros((D, D), dtype=LD)
    for i in range(D):
        Uf[i, i] = np.sqrt(M[i, i] - (Uf[:i, i] ** 2).sum())
        if i + 1 < D:
            Uf[i, i + 1:] = (M[i, i + 1:] - Uf[:i, i] @ Uf[:i, i + 1:]) / Uf[i, i]
    Ui = np.zeros((D, D), dtype=LD)
    eye = np.eye(D, dtype=LD)
    for i in range(D - 1, -1, -1):
        Ui[i, :] = (eye[i, :] - Uf[i, i + 1:] @ Ui[i + 1:, :]) / Uf[i, i]
    return Uf, Ui


def momentum_map_bound(Minv, Uf, Ui, z, dtype):
    """‖r − U⁻¹z‖₂ per chain for r = k_dgemm(Û⁻¹_T, z), Û⁻¹_T what dn_set_metric uploads: the Cholesky factor and its inverse in double on the host, rounded
    to the element type.  With u₆₄ = 2^-53, γ⁶⁴_k = k·u₆₄/(1 − k·u₆₄), u the element type's roundoff:

      the product:      |r − Û⁻¹_T z| ≤ γ_D·|Û⁻¹_T||z|                                                      (product_bound)
      the rounding:     ‖Û⁻¹_T − X̂‖_F ≤ u·‖X̂‖_F,  X̂ the host's inverse in double
      the inversion:    column j solves (Û + Δ_j)x̂_j = e_j, |Δ_j| ≤ γ⁶⁴_D·|Û| (Higham, Thm 8.5): ‖X̂ − Û⁻¹‖_F ≤ γ⁶⁴_D·‖Û⁻¹‖₂‖Û‖_F‖X̂‖_F
      the factorisation: ÛᵀÛ = M⁻¹ + ΔM, |ΔM| ≤ γ⁶⁴_{D+1}·|Ûᵀ||Û| (Thm 10.3), ‖ΔM‖_F ≤ γ⁶⁴_{D+1}·‖Û‖_F².  W = ÛU⁻¹ is the Cholesky factor of
                        I + F, F = U⁻ᵀΔM U⁻¹, ‖F‖_F ≤ φ := γ⁶⁴_{D+1}·trace(M⁻¹)/λ_min(M⁻¹)  (= c·D·u₆₄·cond), so ‖W − I‖_F ≤ φ/(√2·(1 − φ)) (Thm 10.8 at A = I)
                        and ‖Û⁻¹ − U⁻¹‖₂ = ‖U⁻¹W⁻¹(W − I)‖ ≤ ‖U⁻¹‖₂·‖W − I‖_F/(1 − ‖W − I‖_F).

    The norms of the computed Û, X̂, Û⁻¹_T are taken from the exact U, U⁻¹: they differ by a relative φ + u (asserted < 1e-3), and the factor 1.01 covers
    the products of such terms — an allowance for the second order, not a fit."""
    D = Minv.shape[0]
    u, u64 = U[np.dtype(dtype)], U[np.dtype(np.float64)]
    lam_min = LD(np.linalg.eigvalsh(Minv.astype(np.float64))[0])
    nUi2, nUiF, nUF = 1 / np.sqrt(lam_min), np.sqrt((Ui ** 2).sum()), np.sqrt((Uf ** 2).sum())
    phi = gam(D + 1, u64) * np.trace(Minv.astype(LD)) / lam_min
    assert phi + u < 1e-3
    w = phi / (np.sqrt(LD(2)) * (1 - phi))
    dUi = u * nUiF + gam(D, u64) * nUi2 * nUF * nUiF + nUi2 * w / (1 - w)
    z = np.asarray(z, dtype=LD)
    prod = np.sqrt(((gam(D, u) * (np.abs(Ui) @ np.abs(z))) ** 2).sum(axis=0))
    return LD("1.01") * (prod + dUi * np.sqrt((z ** 2).sum(axis=0)))


REFRESH_SHAPES = ((5, 70), (64, 70), (200, 513), (512, 70), (512, 2100))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("D,N", REFRESH_SHAPES)
def test_fresh_momentum_against_the_exact_factor(hip, D, N, dtype):
    """refresh(): r against U⁻¹z, U the upper Cholesky factor of M⁻¹ in long double, z the normals a second HIP engine with the same seed, iteration and chain
    count returns from refresh() under the dense IDENTITY metric (U⁻¹ = I: its product fma(1, z, +0) … is z exactly — also asserted through its ℓκ)."""
    dtn = np.dtype(dtype).name
    Minv, P, _, _, eps = velocity_case(D, 4, 1e3, dtype)
    th = np.asfortranarray(np.random.default_rng([D, N, 4]).normal(size=(D, N)), dtype=dtype)
    out = []
    for metric in (np.asfortranarray(np.eye(D), dtype=dtype), Minv):
        e = dense_engine(hip, metric, P, N, dtype, eps, seed=21)
        e.set_position(th)
        e.refresh()
        out.append(e.phasepoint())
        e.close()
    zi, zm = out
    z = _cm(zi.r, dtype)
    assert np.isfinite(z).all() and 0.9 < z.std() < 1.1 and abs(z.mean()) < 0.05
    f = Findings()
    judge_point(f, f"§2 engine refresh identity [{dtn}]", zi, np.asfortranarray(np.eye(D), dtype=dtype), P, dtype)
    judge_point(f, f"§2 engine refresh [{dtn}]", zm, Minv, P, dtype)
    Uf, Ui = cholesky_upper_ld(Minv)
    assert np.abs(Uf.T @ Uf - Minv.astype(LD)).max() <= 64 * D * U_LD * np.abs(Minv.astype(LD)).max()
    want = Ui @ z.astype(LD)
    err = np.sqrt(((_cm(zm.r, dtype).astype(LD) - want) ** 2).sum(axis=0))
    f.bound(f"§2 engine refresh momentum [{dtn}]", err, momentum_map_bound(Minv, Uf, Ui, z, dtype))
    assert_none(f.other)
