"""The device primitives of advancedhmc.jl_amd/csrc/ahmc_device.hpp, each on its own, against exact references.

Every trajectory kernel is built from these primitives, and the parity tests see them only through whole transitions whose
comparison forgives a decision that differs at a near-tie (tests/parity_util.py) — exactly what a primitive that is a few ulps
off produces.  So here each one runs alone in tests/device_probe/prims.hip (one wrapper per instantiation, compiled with the
engine's own flags: build.build_probe_object) and is compared with mpmath or x86 80-bit `np.longdouble` (cross-checked against
mpmath below).  Every bound is stated next to its assertion with the error analysis it comes from; none is fitted to a
measurement.  u is the unit roundoff: 2^-53 (f64), 2^-24 (f32).
"""
import importlib.util
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "device_probe", "prims.hip")
U = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}
TN = {np.float64: "f64", np.float32: "f32"}
LD = np.longdouble
LOG2PI = LD("1.8378770664093454835606594728112353")
GS = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512)
VARIANTS = {"default": (), "mfma": ("AHMC_MFMA_REDUCE=1",), "ds": ("AHMC_DS_REDUCE=7",)}
# the (G, E) geometries of the trajectory kernels the target tests run at
GEOMS = ((4, 1), (8, 2), (16, 2), (32, 4), (64, 8), (128, 4), (512, 8))
FAMILY_MIN_D = {0: 1, 1: 1, 2: 2, 3: 3}


def _build():
    from ahmc_amd import build as B

    return B


def _oracle_ref():
    spec = importlib.util.spec_from_file_location("ahmc_ref_probe", os.path.join(ROOT, "oracle", "ahmc_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def ulp_of(exact, dtype):
    """ulp of the exact value in `dtype`: 2^(e - p) for exact = m·2^e, m in [0.5, 1) — the SMALLER ulp at a binade edge, so a
    bound in these ulps is never looser than one in the ulps of the rounded value"""
    p = 53 if dtype == np.float64 else 24
    emin = -1021 if dtype == np.float64 else -125
    _, e = np.frexp(np.abs(np.asarray(exact, dtype=LD)))
    return np.ldexp(LD(1), np.maximum(e, emin) - p)


def tree_depth(G):
    """h: additions a value takes in group_allsum<G> — log2(min(G, 64)) butterfly stages inside a wave, then G/64 − 1
    serial additions of the per-wave sums"""
    return int(math.log2(min(G, 64))) + max(0, G // 64 - 1)


# =====================================================================================================================
# CPU part
# =====================================================================================================================
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_probe_compiles_without_scratch_or_spills(variant):
    """The probe compiles for gfx950 with build.FLAGS (+ the variant's A/B switch), and no wrapper needs scratch or spills:
    a wrapper that spilled would test the spill code, not the primitive."""
    B = _build()
    co = B.build_probe_object(PROBE, VARIANTS[variant])
    assert os.path.exists(co)
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_meta
    finally:
        sys.path.pop(0)
    meta = kernel_meta.kernel_meta(co)
    names = {k["name"] for k in meta}
    for want in ("p_exp_table_uniform", "p_red_f64_g512_k8", "p_once_f32_g128_k3", "p_target_f64_g512_e8_t3", "p_vec_f32_e8", "p_philox",
                 "p_hier2_f32_g128_e4", "p_hier2_f64_g256_e8", "p_hier2_f64_g512_e8"):
        assert want in names, want
    bad = [(k["name"], k.get("private_segment_fixed_size"), k.get("vgpr_spill_count"), k.get("sgpr_spill_count")) for k in meta
           if k.get("private_segment_fixed_size") or k.get("vgpr_spill_count") or k.get("sgpr_spill_count")]
    assert not bad, bad


def test_probe_cache_key_follows_flags_and_defines(monkeypatch, tmp_path):
    """The probe's cache key covers the engine's FLAGS and the defines: a flag change reaches the probe (no copied list)."""
    B = _build()
    seen = []

    def fake_run(cmd, capture_output, text):
        seen.append(cmd)
        open(cmd[cmd.index("-o") + 1], "w").close()

        class R:
            returncode, stdout, stderr = 0, "", ""
        return R()

    monkeypatch.setattr(B, "OBJ", str(tmp_path))
    monkeypatch.setattr(B.subprocess, "run", fake_run)
    a = B.build_probe_object(PROBE)
    assert B.build_probe_object(PROBE) == a and len(seen) == 1
    b = B.build_probe_object(PROBE, ("AHMC_DS_REDUCE=7",))
    monkeypatch.setattr(B, "FLAGS", B.FLAGS + ["-DAHMC_PROBE_FLAG_CHANGE"])
    c = B.build_probe_object(PROBE)
    assert len({a, b, c}) == 3 and len(seen) == 3
    assert "-DAHMC_PROBE_FLAG_CHANGE" in seen[-1] and "-ffp-contract=on" in seen[0] and "-DAHMC_DS_REDUCE=7" in seen[1]
    assert seen[0][seen[0].index("-I") + 1] == B.INCLUDE and B.CSRC in seen[0]


def test_longdouble_references_agree_with_mpmath():
    """The bulk references use x86 80-bit long double (64-bit significand): its exp / log / log1p / sqrt / sin / cos agree
    with mpmath to a few 2^-64 relative, i.e. ≤ 2^-10 of a double ulp — three orders below every bound here."""
    import mpmath

    assert np.finfo(LD).nmant >= 63, "the references need x86 80-bit long double"
    mpmath.mp.prec = 120
    rs = np.random.default_rng(1)
    xs = np.concatenate([rs.uniform(-1100, 600, 300), rs.uniform(-40, 2, 300), [-708.4, -745.13, -1075.0]])
    for x in xs:
        ref = mpmath.exp(mpmath.mpf(float(x)))
        assert abs(_mp(np.exp(LD(x))) - ref) <= mpmath.mpf(2) ** -61 * ref
    for x in rs.uniform(1e-300, 1.0, 300) ** 3:
        for f, g in ((np.log, mpmath.log), (np.log1p, mpmath.log1p), (np.sqrt, mpmath.sqrt)):
            ref = g(mpmath.mpf(float(x)))
            assert abs(_mp(f(LD(x))) - ref) <= mpmath.mpf(2) ** -61 * abs(ref)
    for x in rs.uniform(0, 2 * math.pi, 300):
        for f, g in ((np.sin, mpmath.sin), (np.cos, mpmath.cos)):
            ref = g(mpmath.mpf(float(x)))
            assert abs(_mp(f(LD(x))) - ref) <= mpmath.mpf(2) ** -62


def test_reduction_bound_holds_for_host_trees():
    """The reduction bound |Σ̂ − Σ| ≤ h·u·Σ|x| / (1 − h·u) (Higham, Accuracy and Stability, §4.2: any summation tree of depth h)
    holds for numpy's own pairwise tree and for a host transcription of the butterfly (same inputs as the device test)."""
    rs = np.random.default_rng(2)
    for dt in (np.float64, np.float32):
        u = U[dt]
        for G in GS:
            x = _red_values(rs, G * 64, dt).reshape(64, G)
            for row in x:
                exact = math.fsum(row.astype(np.float64))
                s_abs = math.fsum(np.abs(row.astype(np.float64)))
                h = tree_depth(G)
                bound = h * u * s_abs / (1 - h * u)
                # butterfly: lane l adds lane l ^ 2^j at stage j (what every lane of a DPP / swizzle / permlane stage computes)
                v = row.copy()
                for j in range(int(math.log2(min(G, 64)))):
                    v = (v + v[np.arange(G) ^ (1 << j)]).astype(dt)
                if G > 64:
                    w = v.reshape(G // 64, 64)[:, 0]
                    acc = dt(0)
                    for t in w:
                        acc = dt(acc + t)
                    v = np.full(G, acc, dtype=dt)
                assert abs(float(v[0]) - exact) <= bound
                if G <= 64:  # numpy's pairwise sum (8 accumulators below 128 terms): whatever its tree, its depth is ≤ G − 1
                    hp = G - 1
                    assert abs(float(np.sum(row, dtype=dt)) - exact) <= hp * u * s_abs / (1 - hp * u)


def test_normals_mapping_transcription():
    """The host transcription of normals<T, E> used by the device test: element → (pair, half)."""
    assert _normals_map(1, 6) == [(3, 0)] and _normals_map(1, 7) == [(3, 1)]
    assert _normals_map(4, 8) == [(4, 0), (4, 1), (5, 0), (5, 1)]


# =====================================================================================================================
# shared host helpers
# =====================================================================================================================
def _red_values(rs, n, dt):
    """wide exponent spread with mixed signs (cancellation), ±0, and for f32 subnormals"""
    span = 40 if dt == np.float64 else 20
    v = rs.choice([-1.0, 1.0], n) * np.exp2(rs.uniform(-span, span, n)) * rs.uniform(1, 2, n)
    v[rs.random(n) < 0.03] = 0.0
    v[rs.random(n) < 0.03] = -0.0
    v = v.astype(dt)
    if dt == np.float32:
        sub = rs.random(n) < 0.05
        v[sub] = (rs.choice([-1, 1], sub.sum()) * rs.integers(1, 2 ** 23, sub.sum()) * 2.0 ** -149).astype(np.float32)
    return v


def _normals_map(E, d0):
    if E == 1:
        return [((d0 >> 1), d0 & 1)]
    return [((d0 + e) >> 1, e & 1) for e in range(E)]


def _mp(x):
    """a long double as an mpmath number (30 significant digits: far below the 2^-64 of its own significand)"""
    import mpmath

    return mpmath.mpf(np.format_float_scientific(LD(x), precision=30, unique=False))


def _exp2_64_table():
    """2^(j/64), j = 0..63, correctly rounded to f64 (mpmath at 200 bits)"""
    import mpmath

    with mpmath.workprec(200):
        return np.array([float(mpmath.power(2, mpmath.mpf(j) / 64)) for j in range(64)], dtype=np.float64)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _same_bits(a, b):
    """bitwise equal, with any NaN equal to any NaN (payloads are not specified)"""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a) & np.isnan(b)
    return (_bits(a) == _bits(b)) | nan


# =====================================================================================================================
# GPU part
# =====================================================================================================================
_MODULES = {}


def _probe(variant="default"):
    from ahmc_amd.hipmod import Module

    if variant not in _MODULES:
        _MODULES[variant] = Module(_build().build_probe_object(PROBE, VARIANTS[variant]))
    return _MODULES[variant]


@pytest.fixture(scope="module")
def probe(hip):
    import torch

    torch.cuda.init()
    return _probe()


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _empty(n, dt):
    import torch

    t = {np.float64: torch.float64, np.float32: torch.float32, np.int32: torch.int32, np.uint32: torch.int32}[dt]
    return torch.full((int(n),), float("nan") if t.is_floating_point else -7, dtype=t, device="cuda")


def _host(t, dt=None):
    import torch

    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a.view(dt) if dt is not None else a


def _run1(probe, name, x, dt):
    """y = name(x), one launch of 256-thread blocks over the whole array"""
    n = len(x)
    y = _empty(n, dt)
    probe.launch(name, (n + 255) // 256, 256, _dev(x.astype(dt)), y, np.int64(n))
    return _host(y)


def _exp_arguments():
    """≥ 2^22 arguments over the leaf weight's domain [−1100, 600]: dense uniform, extra density in [−40, 2], both edges of all
    64 table buckets (x ≈ (64n + j ± ½)·ln2/64 ± 3 ulps) for negative and positive n, and the underflow thresholds"""
    rs = np.random.default_rng(3)
    parts = [rs.uniform(-1100, 600, 1 << 22), rs.uniform(-40, 2, 1 << 20)]
    ns = np.concatenate([np.arange(-24, 24), rs.integers(-1587, 865, 200)])
    k = (64 * ns[:, None] + np.arange(64)[None, :]).ravel().astype(LD)
    edges = np.concatenate([(k - LD(0.5)), (k + LD(0.5))]) * (LD(np.log(LD(2))) / 64)
    e = edges.astype(np.float64)
    for s in range(-3, 4):
        q = e.copy()
        for _ in range(abs(s)):
            q = np.nextafter(q, np.inf if s > 0 else -np.inf)
        parts.append(q)
    for c in (-708.4, -745.13, -1075.0, -1100.0, -709.78):
        parts.append(c + rs.uniform(-0.5, 0.5, 1 << 15))
        parts.append(c + np.arange(-512, 512) * np.spacing(c))
    x = np.concatenate(parts)
    x = x[(x >= -1100) & (x <= 600)]
    return np.concatenate([x, [-np.inf, np.nan, 0.0, -0.0, -1e308]])


@pytest.fixture(scope="module")
def exp_args():
    x = _exp_arguments()
    assert len(x) >= 1 << 22
    return x


@pytest.mark.gpu
def test_table_exp_accuracy(probe, exp_args):
    """A. leaf_weight_exp<true> (the table form) against the exact exp."""
    x = exp_args
    y = _run1(probe, "p_exp_table_uniform", x, np.float64)
    fin = np.isfinite(x)
    ref = np.exp(x[fin].astype(LD))
    yf = y[fin]
    normal = ref >= LD(2.0 ** -1022)
    err_ulp = np.abs(yf[normal].astype(LD) - ref[normal]) / ulp_of(ref[normal], np.float64)
    worst = float(err_ulp.max())
    # ≤ 1.34 ulp, in ulps of the exact value.  With x = (64n + j)·ln2/64 + t, |t| ≤ ln2/128, the result is 2^n·fl(T[j] + T[j]·p(t)):
    #   the table entry T[j] ∈ [1, 2) is correctly rounded: ≤ 2^-53 absolute, times (1 + p) ≤ 1.0055        → ≤ 0.503 ulp
    #   p(t) is e^t − 1 truncated after t^5: ≤ |t|^6/720·1.01 ≤ 3.55e-17, times T[j] < 2 (ulp 2^-52)         → ≤ 0.32 ulp
    #   the Horner roundings of p (each ≤ u·|p| ≤ u·0.0055, times T < 2) and the reduced argument (the fma with the low
    #   part of ln2/64 rounds at ≤ 2^-61; the high part's product is exact: 20 trailing zero bits)               → ≤ 0.02 ulp
    #   the final fma rounds once                                                                                → ≤ 0.5 ulp
    # (ahmc_device.hpp used to say 1.01, from 2·10^5 arguments; the truncation term reaches its maximum only at bucket edges)
    assert worst <= 1.35, (worst, float(x[fin][normal][np.argmax(err_ulp)]))
    # The same result against the algorithm evaluated exactly: 2^(k >> 6)·T[k & 63]·(1 + p(t)) with T the CORRECTLY ROUNDED 2^(j/64)
    # (mpmath) and p the header's degree-5 polynomial in long double.  What is left is the final fma's rounding (½ ulp), the
    # roundings inside p and of t (≤ 0.02 ulp, above) — so a table entry or an exponent off by one shows here, where the
    # 1.35-ulp bound could hide it.
    xs = np.maximum(x[fin][normal], -1100.0)
    dk = np.rint(xs * 92.33248261689366)
    t = xs.astype(LD) - dk.astype(LD) * LD(float.fromhex("0x1.62e42fef00000p-7")) - dk.astype(LD) * LD(float.fromhex("0x1.473de6af278edp-40"))
    q = t * LD(8.3333333333333332e-03) + LD(4.1666666666666664e-02)
    for c in (1.6666666666666666e-01, 0.5, 1.0):
        q = t * q + LD(c)
    k = dk.astype(np.int64)
    pred = np.ldexp(_exp2_64_table()[k & 63].astype(LD) * (1 + q * t), (k >> 6).astype(np.int32))
    model = np.abs(yf[normal].astype(LD) - pred) / ulp_of(pred, np.float64)
    assert float(model.max()) <= 0.52, (float(model.max()), float(xs[np.argmax(model)]))
    sub = ~normal
    # subnormal outputs: the 53-bit result of the fma (≤ 1.35 of its ulps, each ≤ 2^-1074 once scaled) then ldexp's own rounding
    # to the subnormal grid (½·2^-1074)
    err_sub = np.abs(yf[sub].astype(LD) - ref[sub])
    assert float(err_sub.max() / LD(2.0 ** -1074)) <= 1.85
    # exactly +0 below −1075 (2^-1075·(1 + …) rounds to 0 or the min subnormal only above it) and for −Inf; NaN → NaN
    below = x < -1075.0
    assert np.all(_bits(y[below]) == 0), y[below][_bits(y[below]) != 0][:4]
    assert np.isnan(y[np.isnan(x)]).all()
    assert np.all(y[(x == 0)] == 1.0)
    print(f"table exp: max error {worst:.4f} ulp on {normal.sum()} normal outputs, subnormal max {float(err_sub.max() / LD(2.0 ** -1074)):.3f}·2^-1074")


@pytest.mark.gpu
def test_horner_exp_is_the_library_exp(probe, exp_args):
    """A. leaf_exp and leaf_weight_exp<false> (Horner-11) give the device library's exp bit for bit (ahmc_device.hpp: "the same
    constants, the same operation order"); leaf_exp also saturates to +Inf above 709.78 and to 0 below −1075."""
    rs = np.random.default_rng(4)
    x = exp_args
    lib = _run1(probe, "p_exp_lib_f64", x, np.float64)
    for name in ("p_exp_horner", "p_exp_weight_lane"):
        y = _run1(probe, name, x, np.float64)
        same = _same_bits(y, lib)
        assert same.all(), (name, x[~same][:4], y[~same][:4], lib[~same][:4])
    over = np.concatenate([rs.uniform(709.79, 1100, 4096), [709.7828, 1024.0, 1024.5, 1e308, np.inf]])
    y = _run1(probe, "p_exp_horner", over, np.float64)
    assert np.all(y == np.inf) and _same_bits(y, _run1(probe, "p_exp_lib_f64", over, np.float64)).all()
    under = np.concatenate([rs.uniform(-1100, -1075.0001, 4096), [-1e308, -np.inf]])
    assert np.all(_bits(_run1(probe, "p_exp_horner", under, np.float64)) == 0)


@pytest.mark.gpu
def test_alpha_from_logweight(probe):
    """B. alpha_from_logweight<T, U>(ℓw) = min(1, leaf_weight_exp<U>(min(0, ℓw))) bit for bit; ℓw ≥ 0 → exactly 1, −Inf → exactly
    0, NaN → NaN."""
    rs = np.random.default_rng(5)
    lw = np.concatenate([rs.uniform(-1100, 50, 1 << 18), rs.uniform(-3, 3, 1 << 16), -np.exp2(rs.uniform(-60, 0, 4096)),
                         [0.0, -0.0, 1e-300, -1e-300, 600.0, 1e308, np.inf, -np.inf, np.nan, -1e308]])
    for dt, lane, uni, exp_lane, exp_uni in ((np.float64, "p_alpha_f64_lane", "p_alpha_f64_uniform", "p_exp_weight_lane", "p_exp_table_uniform"),
                                             (np.float32, "p_alpha_f32_lane", "p_alpha_f32_uniform", "p_exp_weight_f32", "p_exp_weight_f32")):
        x = lw.astype(dt)
        m = np.where(x > 0, dt(0), x)
        for a_name, e_name in ((lane, exp_lane), (uni, exp_uni)):
            a = _run1(probe, a_name, x, dt)
            w = _run1(probe, e_name, m, dt)
            want = np.where(w >= 1, dt(1), w)
            same = _same_bits(a, want)
            assert same.all(), (a_name, x[~same][:4], a[~same][:4], want[~same][:4])
            assert np.all(a[x >= 0] == 1) and np.all(_bits(a[x == -np.inf]) == 0) and np.isnan(a[np.isnan(x)]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_logaddexp(probe, dt):
    """C. logaddexp(x, y) = max + log1p(exp(−|x − y|)) against the exact value, and its table of special cases."""
    rs = np.random.default_rng(6)
    n = 1 << 18
    span = 700 if dt == np.float64 else 80
    x = np.concatenate([rs.uniform(-span, span, n), rs.normal(0, 3, n)]).astype(dt)
    y = np.concatenate([rs.uniform(-span, span, n), rs.normal(0, 3, n)]).astype(dt)
    near = rs.random(2 * n) < 0.25
    y[near] = (x[near] + rs.normal(0, 1e-3, near.sum())).astype(dt)
    y[:64] = x[:64]
    o = _empty(len(x), dt)
    probe.launch(f"p_logaddexp_{TN[dt]}", (len(x) + 255) // 256, 256, _dev(x), _dev(y), o, np.int64(len(x)))
    got = _host(o)
    xl, yl = x.astype(LD), y.astype(LD)
    exact = np.maximum(xl, yl) + np.log1p(np.exp(-np.abs(xl - yl)))
    u = U[dt]
    # |Δ| ≤ ulp(result) + 4u: the log1p term lies in (0, log 2] and carries ≲ 3u of absolute error (exp of −d: 1 ulp; log1p: 1 ulp;
    # the subtraction x − y: ½ ulp of d, times d/dd log1p(e^-d) ≤ ½ — all absolute on a value ≤ log 2 < 1), and the final
    # addition max + term rounds once: ½ ulp(result) (taken as a full ulp of the exact value to cover a binade edge)
    bound = ulp_of(exact, dt) + LD(4 * u)
    err = np.abs(got.astype(LD) - exact)
    assert np.all(err <= bound), (float((err / bound).max()), x[np.argmax(err / bound)], y[np.argmax(err / bound)])
    print(f"logaddexp {TN[dt]}: max |Δ| / bound = {float((err / bound).max()):.3f}")
    # the edge table, exactly
    inf, nan = np.inf, np.nan
    cases = [(-inf, -inf, -inf), (-inf, 1.5, 1.5), (2.5, -inf, 2.5), (inf, 1.5, inf), (1.5, inf, inf), (inf, -inf, inf), (-inf, inf, inf),
             (inf, inf, inf), (nan, 1.0, nan), (1.0, nan, nan), (nan, -inf, nan), (inf, nan, nan), (nan, nan, nan)]
    a = np.array([c[0] for c in cases] + [c[1] for c in cases], dtype=dt)
    b = np.array([c[1] for c in cases] + [c[0] for c in cases], dtype=dt)
    want = np.array([c[2] for c in cases] * 2, dtype=dt)
    o = _empty(len(a), dt)
    probe.launch(f"p_logaddexp_{TN[dt]}", 1, 256, _dev(a), _dev(b), o, np.int64(len(a)))
    g = _host(o)
    assert _same_bits(g, want).all(), list(zip(a, b, g, want))
    # symmetric in its arguments, bit for bit
    o2 = _empty(len(x), dt)
    probe.launch(f"p_logaddexp_{TN[dt]}", (len(x) + 255) // 256, 256, _dev(y), _dev(x), o2, np.int64(len(x)))
    assert _same_bits(_host(o2), got).all()


# ---------------------------------------------------------------------------------------------------------------------
# D. reductions
# ---------------------------------------------------------------------------------------------------------------------
def _launch_shape(G):
    """G ≤ 64: 256-thread blocks (4 waves, 256/G groups each); G > 64: blockDim == G, one chain per workgroup.  8 workgroups."""
    return (8, 256) if G <= 64 else (8, G)


def _red_inputs(G, K, dt, seed):
    grid, block = _launch_shape(G)
    n = grid * block
    rs = np.random.default_rng(seed)
    x = _red_values(rs, n * K, dt).reshape(n // G, G, K)
    return x


def _run_red(mod, G, K, dt, x):
    grid, block = _launch_shape(G)
    n = grid * block
    o = _empty(n * K, dt)
    mod.launch(f"p_red_{TN[dt]}_g{G}_k{K}", grid, block, _dev(x.reshape(-1)), o, np.int64(n))
    return _host(o).reshape(n // G, G, K)


def _mfma_depth(G, K):
    """additions per value on the MFMA pair path (AHMC_MFMA_REDUCE, G ≥ 64 with K even, not 4): the first 16x16x4 MFMA sums 4
    values (3 roundings), the 2+2 adds of the four accumulator rows (2), the second MFMA (3) — 8 instead of 6 — then the
    G/64 − 1 additions across waves"""
    return 8 + max(0, G // 64 - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_group_allsum(probe, variant, dt):
    """D. group_allsum<G, T, K> for every G and K ∈ {1, 2, 3, 4, 8}: (1) every lane of a group holds the same bits, (2) the sum is
    within the tree bound of the exact one, (3) a non-finite value gives the IEEE result in its own group only, (4) a group's
    result does not depend on its slot, wave or workgroup.  Also under the two A/B switches of the reduction."""
    mod = _probe(variant)
    u = U[dt]
    for G in GS:
        for K in (1, 2, 3, 4, 8):
            x = _red_inputs(G, K, dt, seed=G * 16 + K)
            ng = x.shape[0]
            y = _run_red(mod, G, K, dt, x)
            # (1) identical bits in all lanes of a group
            assert (_bits(y) == _bits(y[:, :1, :])).all(), (G, K, "lanes of a group differ")
            # (2) |Σ̂ − Σ| ≤ h·u·Σ|x| / (1 − h·u), exact Σ by math.fsum of the float64 values (Higham §4.2: a tree of depth h)
            h = tree_depth(G)
            if variant == "mfma" and G >= 64 and K % 2 == 0 and K != 4:
                h = _mfma_depth(G, K)
            x64 = x.astype(np.float64)
            for gi in range(ng):
                for k in range(K):
                    exact = math.fsum(x64[gi, :, k])
                    s_abs = math.fsum(np.abs(x64[gi, :, k]))
                    bound = h * u * s_abs / (1 - h * u)
                    assert abs(float(y[gi, 0, k]) - exact) <= bound, (G, K, gi, k, float(y[gi, 0, k]), exact, bound)
            # (3) non-finite values: +Inf / −Inf / both / NaN in four groups
            xn = x.copy()
            bad = {0: (np.inf,), 1: (-np.inf,), 2: (np.inf, -np.inf), 3: (np.nan,)}
            if G == 1:  # (a one-lane group cannot hold both infinities)
                bad[2] = (-np.inf,)
            want = {}
            for gi, vals in bad.items():
                for j, v in enumerate(vals):
                    xn[gi, (j * 7 + 1) % G, K - 1] = v
                want[gi] = np.nan if (len(vals) == 2 or np.isnan(vals[0])) else vals[0]
            yn = _run_red(mod, G, K, dt, xn)
            for gi, w in want.items():
                got = yn[gi, :, K - 1]
                assert (np.isnan(got).all() if np.isnan(w) else (got == w).all()), (G, K, gi, got[:4], w)
            others = np.setdiff1d(np.arange(ng), list(bad))
            if len(others):
                assert (_bits(yn[others]) == _bits(y[others])).all(), (G, K, "a non-finite value leaked into another group")
            clean = [k for k in range(K - 1)]
            if clean:  # the other K − 1 values of the poisoned groups are untouched too
                assert (_bits(yn[:, :, clean]) == _bits(y[:, :, clean])).all(), (G, K, "leak across k")
            # (4) the same inputs at other slots, waves and workgroups give the same bits
            perm = np.random.default_rng(G + K).permutation(ng)
            yp = _run_red(mod, G, K, dt, x[perm])
            assert (_bits(yp) == _bits(y[perm])).all(), (G, K, "a group's bits depend on its position")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_reduction_identities(probe, dt):
    """D.5 the claimed identities, bit for bit: wave_allsum4(a, b, c, d) = wave_allsum2(a, b); wave_allsum2(c, d)
    (ahmc_device.hpp: "the additions each value goes through are those of wave_allsum2"), and group_allsum_once =
    group_allsum = leapfrog_allsum<G, TK = 3> for the multi-wave groups ("same additions in the same order")."""
    rs = np.random.default_rng(7)
    for G in (16, 32, 64):
        n = 8 * 256
        x = _red_values(rs, n * 4, dt)
        o = _empty(n * 8, dt)
        probe.launch(f"p_quad_{TN[dt]}_g{G}", 8, 256, _dev(x), o, np.int64(n))
        y = _host(o).reshape(n, 8)
        assert (_bits(y[:, :4]) == _bits(y[:, 4:])).all(), G
    for G in (128, 256, 512):
        for K in (1, 2, 3, 4):
            n = 8 * G
            x = _red_values(rs, n * K, dt)
            o = _empty(n * 3 * K, dt)
            probe.launch(f"p_once_{TN[dt]}_g{G}_k{K}", 8, G, _dev(x), o, np.int64(n))
            y = _host(o).reshape(n, 3, K)
            assert (_bits(y[:, 1]) == _bits(y[:, 0])).all(), (G, K, "group_allsum_once")
            assert (_bits(y[:, 2]) == _bits(y[:, 0])).all(), (G, K, "leapfrog_allsum")
            ref = _run_red(probe, G, K, dt, x.reshape(-1, G, K)).reshape(n, K)
            assert (_bits(y[:, 0]) == _bits(ref)).all()


# ---------------------------------------------------------------------------------------------------------------------
# E. broadcasts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_group_broadcasts(probe):
    """E. group_bcast<G> (f32, f64) for every G and every src, and group_bcast_i32<G> for the in-wave groups (G ≤ 64; the
    multi-wave groups broadcast through LDS): exactly lane src's value of the lane's own group."""
    rs = np.random.default_rng(8)
    for G in GS:
        grid, block = _launch_shape(G)
        n = grid * block
        base = (np.arange(n) // G) * G
        kinds = [(np.float64, f"p_bcast_f64_g{G}"), (np.float32, f"p_bcast_f32_g{G}")]
        if G <= 64:
            kinds.append((np.int32, f"p_bcast_i32_g{G}"))
        for dt, name in kinds:
            x = rs.integers(-2 ** 31, 2 ** 31, n).astype(np.int32) if dt == np.int32 else rs.normal(size=n).astype(dt)
            x[::17] = (np.nan if dt != np.int32 else 0)
            o = _empty(n * G, dt)
            probe.launch(name, grid, block, _dev(x), o, np.int64(n))
            y = _host(o).reshape(G, n)
            want = x[base[None, :] + np.arange(G)[:, None]]
            assert (_bits(y) == _bits(want)).all(), (G, name)


# ---------------------------------------------------------------------------------------------------------------------
# F. RNG
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_philox_and_u53(probe):
    """F. philox4x32_10: the Random123 known answers (as tests/test_oracle_golden.py) and oracle/ahmc_ref.py bit for bit on 10^5
    random (counter, key); u53: its integer formula bit for bit, in (0, 1) — except the top input, which rounds to 1.0."""
    ref = _oracle_ref()
    kat = [((0, 0, 0, 0, 0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 6, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    rs = np.random.default_rng(9)
    n = 100_000
    ck = rs.integers(0, 2 ** 32, (n, 6), dtype=np.uint64).astype(np.uint32)
    ck[:3] = np.array([k for k, _ in kat], dtype=np.uint32)
    o = _empty(n * 4, np.uint32)
    probe.launch("p_philox", (n + 255) // 256, 256, _dev(ck.view(np.int32)), o, np.int64(n))
    got = _host(o, np.uint32).reshape(n, 4)
    for i, (_, want) in enumerate(kat):
        assert tuple(int(v) for v in got[i]) == want
    for i in range(n):
        assert tuple(int(v) for v in got[i]) == ref.philox4x32_10(*(int(v) for v in ck[i])), i
    hl = got[:, :2].copy()
    hl[:6] = [[0, 0], [0, 63], [31, 0], [0xFFFFFFFF, 0xFFFFFFBF], [0xFFFFFFFF, 0xFFFFFFC0], [0xFFFFFFFF, 0xFFFFFFFF]]
    o = _empty(n, np.float64)
    probe.launch("p_u53", (n + 255) // 256, 256, _dev(hl.view(np.int32)), o, np.int64(n))
    u = _host(o)
    bits = ((hl[:, 0].astype(np.uint64) >> np.uint64(5)) << np.uint64(26)) | (hl[:, 1].astype(np.uint64) >> np.uint64(6))
    want = (bits.astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)
    assert (_bits(u) == _bits(want)).all()
    assert all(ref.Rng.u53(int(a), int(b)) == v for (a, b), v in zip(hl[:1000], u[:1000]))
    top = bits == np.uint64(2 ** 53 - 1)
    # (bits + 0.5)·2^-53 is exact below 2^52; above, + 0.5 is a tie rounded to even, so the top input 2^53 − 1 gives exactly 1.0:
    # the range is (0, 1) for every other input — which the RNG stream shares with the oracle, so the formula stays
    assert np.all(u[top] == 1.0) and top[3:6].tolist() == [False, True, True]
    assert np.all((u[~top] > 0) & (u[~top] < 1)) and u[0] == 2.0 ** -54


@pytest.mark.gpu
def test_rng_draws(probe):
    """F. Rng::boolean is the top bit of word 0; randexp within 1½ ulp of −log(u); normal_pair within 16·u·rad of the exact
    Box–Muller of the same u's; normals<T, E> maps elements to (pair, half) as the host transcription."""
    import mpmath

    ref = _oracle_ref()
    rs = np.random.default_rng(10)
    n = 1 << 16
    prm = rs.integers(0, 2 ** 32, (n, 6), dtype=np.uint64).astype(np.uint32)
    prm[:, 4] = rs.integers(0, 4, n)
    o, b = _empty(n * 4, np.float64), _empty(n, np.int32)
    probe.launch("p_rng", (n + 255) // 256, 256, _dev(prm.view(np.int32)), o, b, np.int64(n))
    out = _host(o).reshape(n, 4)
    bo = _host(b)
    words = np.array([ref.philox4x32_10(int(p[2]), int(p[3]), int(p[4]), int(p[5]), int(p[0]), int(p[1])) for p in prm], dtype=np.uint64)
    u1 = ((((words[:, 0] >> np.uint64(5)) << np.uint64(26)) | (words[:, 1] >> np.uint64(6))).astype(np.float64) + 0.5) / 2.0 ** 53
    u2 = ((((words[:, 2] >> np.uint64(5)) << np.uint64(26)) | (words[:, 3] >> np.uint64(6))).astype(np.float64) + 0.5) / 2.0 ** 53
    assert (_bits(out[:, 0]) == _bits(u1)).all()
    assert (bo == (words[:, 0] >> np.uint64(31)).astype(np.int32)).all()
    # randexp = −log(u), u exact: the device log's error (≤ 1 ulp, OCML) on top of the ½ ulp any rounding costs
    ex = -np.log(u1.astype(LD))
    assert np.all(np.abs(out[:, 1].astype(LD) - ex) <= LD(1.5) * ulp_of(ex, np.float64))
    # normal_pair: angle = fl(2π)·u2 rounded: |Δangle| ≤ |fl(2π) − 2π| + u·2π ≤ 4u + 6.3u; sincos adds ≤ 1 ulp of a value ≤ 1 (u… 2u);
    # rad = sqrt(−2 log u1): log 1 ulp, sqrt ½ ulp + half the argument's → ≤ 2u relative; the final product ½ ulp — in all
    # ≤ 10.3u + 2u + 2u + 1u < 16u, times rad
    rad = np.sqrt(-2 * np.log(u1.astype(LD)))
    ang = LD(2) * LD("3.14159265358979323846264338327950288") * u2.astype(LD)
    z0, z1 = rad * np.cos(ang), rad * np.sin(ang)
    bound = 16 * LD(2.0 ** -53) * rad
    assert np.all(np.abs(out[:, 2].astype(LD) - z0) <= bound) and np.all(np.abs(out[:, 3].astype(LD) - z1) <= bound)
    mpmath.mp.prec = 120
    for i in range(300):  # the long-double Box–Muller against mpmath on a subset
        r = mpmath.sqrt(-2 * mpmath.log(mpmath.mpf(float(u1[i]))))
        a = 2 * mpmath.pi * mpmath.mpf(float(u2[i]))
        assert abs(_mp(z0[i]) - r * mpmath.cos(a)) <= mpmath.mpf(2) ** -60 * (1 + r)
        assert abs(_mp(z1[i]) - r * mpmath.sin(a)) <= mpmath.mpf(2) ** -60 * (1 + r)
    # normals<T, E>: element → (pair, half) against the device's own normal_pair draws
    for dt in (np.float64, np.float32):
        for E in (1, 2, 8):
            m = 4096
            p = prm[:m].copy()
            p[:, 5] = rs.integers(0, 1000, m) * (E if E > 1 else 1) + (rs.integers(0, 2, m) if E == 1 else 0)
            oz = _empty(m * E, dt)
            probe.launch(f"p_normals_{TN[dt]}_e{E}", (m + 255) // 256, 256, _dev(p.view(np.int32)), oz, np.int64(m))
            z = _host(oz).reshape(m, E)
            q = np.repeat(p, E, axis=0)
            mp_ = [_normals_map(E, int(d)) for d in p[:, 5]]
            q[:, 5] = [pair for row in mp_ for pair, _ in row]
            half = np.array([h for row in mp_ for _, h in row])
            oq, bq = _empty(m * E * 4, np.float64), _empty(m * E, np.int32)
            probe.launch("p_rng", (m * E + 255) // 256, 256, _dev(q.view(np.int32)), oq, bq, np.int64(m * E))
            pairs = _host(oq).reshape(m * E, 4)
            want = np.where(half == 1, pairs[:, 3], pairs[:, 2]).astype(dt).reshape(m, E)
            assert (_bits(z) == _bits(want)).all(), (TN[dt], E)


# ---------------------------------------------------------------------------------------------------------------------
# G. targets and leapfrog pieces
# ---------------------------------------------------------------------------------------------------------------------
def target_exact(tk, th, params, D):
    """ℓπ, −∇ℓπ and the Σ|summands| of each (include/ahmc_hip.h definitions) in long double, th: (C, D)"""
    th = th.astype(LD)
    C = th.shape[0]
    g = np.zeros_like(th)
    sg = np.abs(g)
    if tk == 0:
        lp = -(th * th).sum(1) / 2 - D * LOG2PI / 2
        S = (th * th).sum(1) / 2 + D * LOG2PI / 2
        g = th.copy()
        sg = np.abs(th)
    elif tk == 1:
        m, s = params[:D].astype(LD), params[D:2 * D].astype(LD)
        diff = m[None, :] - th
        val = -(LOG2PI + 2 * np.log(s)[None, :] + diff * diff / (s * s)[None, :]) / 2
        lp = val.sum(1)
        S = ((LOG2PI + 2 * np.abs(np.log(s))[None, :] + diff * diff / (s * s)[None, :]) / 2).sum(1)
        g = -diff / (s * s)[None, :]
        sg = np.abs(g)
    elif tk == 2:
        y, x = th[:, 0], th[:, 1:]
        ss = (x * x).sum(1)
        ey = np.exp(-y)
        nm1 = LD(D - 1)
        l3 = np.log(LD(3))
        lp = -(LOG2PI + 2 * l3 + y * y / 9) / 2 - nm1 * (LOG2PI + y) / 2 - ss * ey / 2
        S = (LOG2PI + 2 * l3 + y * y / 9) / 2 + nm1 * (LOG2PI + np.abs(y)) / 2 + ss * ey / 2
        g[:, 0] = y / 9 + nm1 / 2 - ss * ey / 2
        sg[:, 0] = np.abs(y) / 9 + nm1 / 2 + ss * ey / 2
        g[:, 1:] = x * ey[:, None]
        sg[:, 1:] = np.abs(g[:, 1:])
    else:
        mu, lt, x = th[:, 0], th[:, 1], th[:, 2:]
        n = LD(D - 2)
        df = x - mu[:, None]
        s0, s1 = df.sum(1), (df * df).sum(1)
        it = np.exp(-2 * lt)
        lp = -(LOG2PI + mu * mu) / 2 - (LOG2PI + lt * lt) / 2 - n * (LOG2PI + 2 * lt) / 2 - s1 * it / 2
        S = (LOG2PI + mu * mu) / 2 + (LOG2PI + lt * lt) / 2 + n * (LOG2PI + 2 * np.abs(lt)) / 2 + s1 * it / 2
        g[:, 0] = mu - s0 * it
        sg[:, 0] = np.abs(mu) + np.abs(df).sum(1) * it
        g[:, 1] = lt + n - s1 * it
        sg[:, 1] = np.abs(lt) + n + s1 * it
        g[:, 2:] = df * it[:, None]
        sg[:, 2:] = np.abs(g[:, 2:])
    return lp, g, S, sg


def _target_launch(mod, dt, G, E, tk, th, r, minv, params, eps, use_pre):
    C, D = th.shape
    rec = 4 * E + 12
    grid = C if G > 64 else C * G // 256
    block = G if G > 64 else 256
    o = _empty(C * G * rec, dt)
    mod.launch(f"p_target_{TN[dt]}_g{G}_e{E}_t{tk}", grid, block, _dev(th.astype(dt)), _dev(r.astype(dt)), _dev(minv.astype(dt)),
               _dev(params.astype(dt)), int(D), np.int64(C), dt(eps), int(use_pre), o)
    return _host(o).reshape(C, G, rec)


def _check_target(tag, dt, G, E, tk, D, th, params, lp_dev, g_dev):
    """ℓπ within (E + t + 6)·u·Σ|summands| — E serial in-lane additions, t = tree depth of the group reduction, and at most 6
    roundings on the longest in-lane path of any family before them (diag: log s, +log 2π, m − θ, its square, /s², + ;
    hierarchical: the exp, the product, three subtractions; the rounded constant log 2π counts as one); gradient elements ≤ 4 ulp
    (each is ≤ 3 correctly rounded operations and one exp ≤ 1 ulp: e.g. (θ − μ)·exp(−2 log τ) ≤ ½ + 1 + ½ ulp), except funnel and
    hierarchical elements 0 / 1, which are reductions themselves and take the Σ|summands| bound; padded slots exactly 0"""
    u = LD(U[dt])
    lp_x, g_x, S, sg = target_exact(tk, th, params, D)
    t = tree_depth(G)
    bound = (E + t + 6) * u * S
    err = np.abs(lp_dev.astype(LD) - lp_x)
    assert np.all(err <= bound), (tag, float((err / bound).max()))
    ge = np.abs(g_dev[:, :D].astype(LD) - g_x)
    gb = LD(4) * ulp_of(g_x, dt)
    if tk in (2, 3):
        lead = 1 if tk == 2 else 2
        gb[:, :lead] = (E + t + 6) * u * sg[:, :lead]
    assert np.all(ge <= gb), (tag, float((ge / gb).max()), np.unravel_index(np.argmax(ge / gb), ge.shape))
    assert np.all(g_dev[:, D:] == 0), (tag, "padded gradient slots")
    return float((err / bound).max()), float((ge / gb).max())


def _target_inputs(rs, tk, C, D, dt):
    th = rs.normal(size=(C, D))
    if tk == 2:
        th[:, 0] = rs.uniform(-3, 3, C)
    if tk == 3:
        th[:, 1] = rs.uniform(-1, 1, C)
    r = rs.normal(size=(C, D))
    minv = rs.uniform(0.5, 2.0, (C, D))
    params = np.concatenate([rs.normal(size=D), rs.uniform(0.5, 2.0, D)]) if tk == 1 else np.zeros(2)
    return th.astype(dt), r.astype(dt), minv.astype(dt), params.astype(dt)


def _d_values(G, E, tk):
    ds = {G * E, G * E - 1, G * E - E - 1, FAMILY_MIN_D[tk]}
    return sorted(d for d in ds if d >= FAMILY_MIN_D[tk])


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("tk", [0, 1, 2, 3])
def test_targets_and_leapfrog(probe, dt, tk):
    """G. target_eval + fill_caches at every kernel geometry and D ∈ {G·E, G·E − 1, whole lanes padded, the family minimum}, θ / r /
    M⁻¹ loaded through load_vec (pad 0 / 0 / 1): ℓπ, −∇ℓπ against the exact values, ℓπ and ℓκ the same bits in every lane.
    Then one leapfrog_step against the exact update of the same inputs, leapfrog_step_plus2's ℓπ / ℓκ bit-identical to it, and for
    the multi-wave hierarchical geometries what hier_publish_next leaves in xwave_buf_p = θ[0..1] after the next step, with and
    without use_pre."""
    rs = np.random.default_rng(11 + tk)
    u = LD(U[dt])
    eps = 0.1
    worst = [0.0, 0.0]
    for G, E in GEOMS:
        C = 4 if G > 64 else 1024 // G
        for D in _d_values(G, E, tk):
            th, r, minv, params = _target_inputs(rs, tk, C, D, dt)
            for use_pre in ((0, 1) if (G > 64 and tk == 3) else (0,)):
                out = _target_launch(probe, dt, G, E, tk, th, r, minv, params, eps, use_pre)
                tag = (TN[dt], G, E, tk, D, use_pre)
                gpad = np.concatenate([out[:, :, k * E:(k + 1) * E] for k in range(4)], axis=2)  # (C, G, 4E)
                vec = lambda k: gpad[:, :, k * E:(k + 1) * E].reshape(C, G * E)  # noqa: E731
                g0, th1, r1, g1 = vec(0), vec(1), vec(2), vec(3)
                sc = out[:, :, 4 * E:]
                # ℓπ, ℓκ identical in every lane (fill_caches, the step, plus2)
                for k in range(6):
                    assert (_bits(sc[:, :, k]) == _bits(sc[:, :1, k])).all(), (tag, k)
                a, b = _check_target(tag, dt, G, E, tk, D, th, params, sc[:, 0, 0], g0)
                worst = [max(worst[0], a), max(worst[1], b)]
                # ℓκ = −½ Σ M⁻¹ r²: per element r·r and the fma into the lane sum (2), E serial, t tree: ≤ (E + t + 2)·u·Σ
                t = tree_depth(G)
                kin = (minv.astype(LD) * r.astype(LD) ** 2).sum(1) / 2
                assert np.all(np.abs(sc[:, 0, 1].astype(LD) + kin) <= (E + t + 2) * u * kin), tag
                # one leapfrog step from the device's own cached g0: r½ = r − ϵ/2·g0, θ′ = θ + ϵ·M⁻¹r½, g′ = −∇ℓπ(θ′), r′ = r½ − ϵ/2·g′
                e_ = LD(dt(eps))
                eh = e_ / 2
                rl, ml, g0l = r.astype(LD), minv.astype(LD), g0[:, :D].astype(LD)
                rh = rl - eh * g0l
                th1x = th.astype(LD) + e_ * (ml * rh)
                # r½: one fma (or a product and a difference): |δ| ≤ u(|r½| + |ϵ/2·g0|); M⁻¹r½ one rounding, the fma into θ one:
                # |Δθ′| ≤ u·(|θ′| + |ϵ M⁻¹|·(3|r½| + |ϵ/2·g0|))·(1 + 2u)
                b_th = u * (np.abs(th1x) + np.abs(e_ * ml) * (3 * np.abs(rh) + np.abs(eh * g0l))) * (1 + 2 * u)
                assert np.all(np.abs(th1[:, :D].astype(LD) - th1x) <= b_th), (tag, "θ′")
                assert np.all(th1[:, D:] == 0) and np.all(r1[:, D:] == 0), (tag, "padding after the step")
                # r′ from the device's g′ (itself checked at the device's θ′ just below): the r½ error carried plus one more rounding
                g1l = g1[:, :D].astype(LD)
                r1x = rh - eh * g1l
                b_r = u * (np.abs(rh) + np.abs(eh * g0l) + np.abs(r1x) + np.abs(eh * g1l)) * (1 + 2 * u)
                assert np.all(np.abs(r1[:, :D].astype(LD) - r1x) <= b_r), (tag, "r′")
                _check_target(tag + ("step",), dt, G, E, tk, D, th1[:, :D], params, sc[:, 0, 2], g1)
                kin1 = (ml * r1[:, :D].astype(LD) ** 2).sum(1) / 2
                assert np.all(np.abs(sc[:, 0, 3].astype(LD) + kin1) <= (E + t + 2) * u * kin1), tag
                # leapfrog_step_plus2 leaves ℓπ / ℓκ bit-identical to leapfrog_step ("every value takes exactly the additions it
                # would take in a reduction of its own")
                assert (_bits(sc[:, :, 4:6]) == _bits(sc[:, :, 2:4])).all(), (tag, "plus2")
                if G > 64 and tk == 3:
                    # hier_publish_next: xwave_buf_p = θ[0], θ[1] of the NEXT leapfrog, bit for bit
                    pub, nxt = sc[:, 0, 8:10], sc[:, 0, 10:12]
                    assert (_bits(pub) == _bits(nxt)).all(), (tag, pub[:2], nxt[:2])
    print(f"targets {TN[dt]} tk={tk}: worst ℓπ error / bound {worst[0]:.3f}, gradient {worst[1]:.3f}")


HIER2_GEOMS = ((128, 4), (256, 8), (512, 8))


def _hier2_inputs(rs, C, D, dt):
    """θ, r, M⁻¹ of mixed magnitudes (two decades each), μ and log τ kept where exp(−2 log τ) stays finite after two steps"""
    mag = lambda: 10.0 ** rs.uniform(-1, 1, (C, D))  # noqa: E731
    th, r, minv = rs.normal(size=(C, D)) * mag(), rs.normal(size=(C, D)) * mag(), mag()
    th[:, 1] = rs.uniform(-1, 1, C)
    return th.astype(dt), r.astype(dt), minv.astype(dt)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_hier_publish_next_is_the_leapfrog_own_expression(probe, dt):
    """G2. The multi-wave hierarchical chain's first lane publishes θ′[0..1] of the NEXT leapfrog (hier_publish_next) for the other waves.
    It is the half kick and the drift of the leapfrog itself — one definition with explicit fma, not a second copy the compiler may
    contract differently.  Two consecutive steps at (G, E) = (128, 4), (256, 8), (512, 8), the second with and without `use_pre`: θ, r,
    −∇ℓπ, ℓπ, ℓκ of EVERY lane bit-identical between the two runs, and the published pair bit-identical to lane 0's own θ[0], θ[1]
    after the second step."""
    rs = np.random.default_rng(77)
    eps = 0.1
    C = 16
    n_finite = n_all = 0
    for G, E in HIER2_GEOMS:
        rec = 3 * E + 4
        for D in (G * E, G * E - E - 1):
            th, r, minv = _hier2_inputs(rs, C, D, dt)
            # the inputs tell a fused drift from an unfused one: θ + ϵ·(M⁻¹r) with one rounding or two differ for a visible share
            prod = (minv * r).astype(dt)
            fused = (th.astype(LD) + LD(dt(eps)) * prod.astype(LD)).astype(dt)
            unfused = (th + (dt(eps) * prod).astype(dt)).astype(dt)
            assert (fused != unfused).mean() > 0.1, (TN[dt], G, D, float((fused != unfused).mean()))
            outs = []
            for use_pre in (0, 1):
                o = _empty(C * G * rec, dt)
                probe.launch(f"p_hier2_{TN[dt]}_g{G}_e{E}", C, G, _dev(th), _dev(r), _dev(minv), int(D), np.int64(C), dt(eps), int(use_pre), o)
                outs.append(_host(o).reshape(C, G, rec))
            a, b = outs
            tag = (TN[dt], G, E, D)
            assert not np.isnan(a[:, :, :3 * E + 2]).all(), tag                      # the kernel wrote its records
            for name, lo, hi in (("θ", 0, E), ("r", E, 2 * E), ("−∇ℓπ", 2 * E, 3 * E), ("ℓπ", 3 * E, 3 * E + 1), ("ℓκ", 3 * E + 1, 3 * E + 2)):
                same = _same_bits(a[:, :, lo:hi], b[:, :, lo:hi])
                assert same.all(), (tag, name, "use_pre changes the result", int((~same).sum()))
            for o_, pre in ((a, 0), (b, 1)):
                pub, own = o_[:, 0, 3 * E + 2:3 * E + 4], o_[:, 0, 0:2]
                assert _same_bits(pub, own).all(), (tag, pre, "published pair != lane 0's θ[0..1]", pub[:2], own[:2])
                assert (_bits(o_[:, :, 3 * E]) == _bits(o_[:, :1, 3 * E])).all(), (tag, pre, "ℓπ differs between lanes")
            n_finite += int(np.isfinite(a[:, 0, 3 * E]).sum())
            n_all += C
    print(f"hier2 {TN[dt]}: {n_finite} of {n_all} chains with a finite ℓπ after the second step")
    assert n_finite >= n_all // 2                                                     # (a −Inf compares equal to anything that overflowed)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_target_overflow_is_minus_inf(probe, dt):
    """G. Where exp(−y) (funnel) or exp(−2 log τ) (hierarchical) overflows T — Σθ² = 0 included, where 0·Inf is NaN — the
    sanitised ℓπ is exactly −Inf in every lane, never NaN or a finite value."""
    rs = np.random.default_rng(12)
    big = 800.0 if dt == np.float64 else 100.0
    for G, E in GEOMS:
        C = 4 if G > 64 else 1024 // G
        D = G * E - 1
        for tk in (2, 3):
            th, r, minv, params = _target_inputs(rs, tk, C, D, dt)
            if tk == 2:
                th[:, 0] = -big
            else:
                th[:, 1] = -big / 2
            if tk == 2:
                th[: C // 2, 1:] = 0  # Σθ² = 0: the exact ℓπ is finite, the device's 0·Inf is NaN
            else:
                th[: C // 2, 2:] = th[: C // 2, :1]  # Σ(x − μ)² = 0
            out = _target_launch(probe, dt, G, E, tk, th, r, minv, params, 0.0, 0)
            lp = out[:, :, 4 * E]
            assert np.all(lp == -np.inf), (TN[dt], G, E, tk, lp[:, 0])


# ---------------------------------------------------------------------------------------------------------------------
# H. load_vec / store_vec
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_load_store_vec(probe, dt):
    """H. Odd and even offsets (the vector and the scalar paths), D not a multiple of the access width: every loaded element is
    the source's bits, every padded register holds `pad`, store_vec writes the D elements back and the sentinels around each
    chain survive."""
    rs = np.random.default_rng(13)
    pad, sentinel = dt(7.25), dt(-12345.5)
    for E in (1, 2, 4, 8):
        for D in (3 * E, 3 * E - 1, 5 * E + 1, 1):
            for off0 in (0, 1, 2, 3):
                for extra in (0, 1, 3, 4):
                    stride = D + extra
                    L = -(-D // E) + 1
                    C = 37
                    nt = C * L
                    size = off0 + C * stride + 8
                    src = rs.normal(size=size).astype(dt)
                    dst = _dev(np.full(size, sentinel, dtype=dt))
                    loaded = _empty(nt * E, dt)
                    probe.launch(f"p_vec_{TN[dt]}_e{E}", (nt + 255) // 256, 256, _dev(src), dst, loaded, np.int64(off0), np.int64(stride),
                                 int(D), int(L), pad, np.int64(nt))
                    ld = _host(loaded).reshape(C, L * E)
                    d = _host(dst)
                    idx = off0 + np.arange(C)[:, None] * stride + np.arange(D)[None, :]
                    tag = (TN[dt], E, D, off0, stride)
                    assert (_bits(ld[:, :D]) == _bits(src[idx])).all(), tag
                    assert np.all(ld[:, D:] == pad), tag
                    want = np.full(size, sentinel, dtype=dt)
                    want[idx] = src[idx]
                    assert (_bits(d) == _bits(want)).all(), tag
