"""The wave-uniform tree decisions of a chain that owns its wave (G = 64), each against the form it replaces — no tolerance anywhere.

(a) `wave64_any_le0_pair(a, b)` (ahmc_device.hpp) — the generalised U-turn test as one scalar predicate taken from the pair
    reduction's transposed register — equals `wave_allsum2<64>` followed by `Σa <= 0 || Σb <= 0` on the same 64 partials: random
    partials, sums that hang on the ORDER of the additions (so the two forms must make the same additions, not just sum the same
    numbers), and built cases: sums exactly +0, −0, the smallest subnormal of either sign, cancellation to 0, one NaN lane, ±Inf —
    each with the roles of a and b swapped.
(b) the wave-wide draw stream `DrawStreamT<true>` (ahmc_nuts.hpp) returns, in every lane, the 32-bit words of the narrow
    `DrawStreamT<false>` on the same Rng: k = 0 … 1 100 from `init`, and from `resume` at every k0 in 0 … 300 and at
    255 / 256 / 257 / 1 023 / 1 024.  The narrow stream itself is held to the stream specification shared with the oracle
    (draw k = word k & 3 of Philox block k >> 2 of RNG_TRANSITION; oracle/ahmc_ref.py).

Both run in tests/device_probe/uniform_outcomes.hip, compiled with the engine's own flags (build.build_probe_object).
"""
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "device_probe", "uniform_outcomes.hip")
TN = {np.float64: "f64", np.float32: "f32"}
RESUME_AT = tuple(range(0, 301)) + (1023, 1024)   # every k0 in 0 … 300 (255 / 256 / 257 among them), 1 023, 1 024
N_FROM_INIT = 1101    # k = 0 … 1 100
N_AFTER_RESUME = 600  # every resumed stream crosses at least two refills of the 256-draw form


def _build():
    from ahmc_amd import build as B

    return B


def _oracle_ref():
    spec = importlib.util.spec_from_file_location("ahmc_ref_uniform", os.path.join(ROOT, "oracle", "ahmc_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# =====================================================================================================================
# inputs of (a): one row = the 64 lane partials of one wave
# =====================================================================================================================
def _tiny(dt):
    return np.finfo(dt).smallest_subnormal


def built_cases(dt):
    """(name, 64 partials, expected `Σ <= 0` or None where it hangs on the order of the additions)"""
    rs = np.random.default_rng(11)
    t, big = _tiny(dt), dt(2.0) ** (40 if dt == np.float32 else 80)
    z = np.zeros(64, dt)

    def at(pairs):
        v = z.copy()
        for lane, val in pairs:
            v[lane] = val
        return v

    cases = [("plus_zero", z.copy(), True), ("minus_zero", -z, True), ("mixed_zeros", at([(l, -0.0) for l in range(0, 64, 3)]), True)]
    for lane in (0, 1, 2, 17, 33, 62, 63):
        cases.append((f"subnormal_pos_lane{lane}", at([(lane, t)]), False))
        cases.append((f"subnormal_neg_lane{lane}", at([(lane, -t)]), True))
        cases.append((f"nan_lane{lane}_rest_pos", at([(lane, np.nan)]) + dt(1), False))
        cases.append((f"nan_lane{lane}_rest_neg", at([(lane, np.nan)]) - dt(1), False))
        cases.append((f"pinf_lane{lane}", at([(lane, np.inf)]) - dt(1), False))
        cases.append((f"ninf_lane{lane}", at([(lane, -np.inf)]) + dt(1), True))
        cases.append((f"both_inf_lane{lane}", at([(lane, np.inf), ((lane + 5) % 64, -np.inf)]), False))
    # cancellation to exactly 0: x and −x in two lanes (exact whatever the order), alone and over a background of zeros of either sign
    for _ in range(24):
        i, j = rs.choice(64, 2, replace=False)
        x = dt(rs.normal() * 10.0 ** rs.integers(-30, 30))
        cases.append((f"cancel_{i}_{j}", at([(i, x), (j, -x)]), True))
        cases.append((f"cancel_subnormal_{i}_{j}", at([(i, t), (j, -t)]), True))
    # every lane x, then −64x in one lane: 0 in exact arithmetic and in every order of a power-of-two tree
    for lane in (0, 1, 31, 32, 63):
        v = np.full(64, dt(0.75), dt)
        v[lane] = dt(0.75) - dt(48)
        cases.append((f"cancel_all_lane{lane}", v, True))
    # sums that hang on the ORDER: big, −big and a few ones — the ones are absorbed or survive according to where the tree meets them.
    # No expectation on the host: the two device forms must agree because they make the same additions.
    for n in range(160):
        v = z.copy()
        lanes = rs.choice(64, 2 + int(rs.integers(1, 6)), replace=False)
        v[lanes[0]], v[lanes[1]] = big, -big
        v[lanes[2:]] = dt(1) if n % 2 == 0 else dt(-1)
        cases.append((f"order_{n}", v, None))
    return cases


def predicate_inputs(dt):
    """rows of (a, b) partials, (n_waves, 64, 2), and the host's expectation of the predicate per wave (−1: none)"""
    rs = np.random.default_rng(12)
    rows, want = [], []
    pos, neg = np.full(64, 1, dt), np.full(64, -1, dt)
    for name, v, le0 in built_cases(dt):
        for other, other_le0 in ((pos, False), (neg, True)):
            for swap in (False, True):
                a, b = (other, v) if swap else (v, other)
                rows.append(np.stack([a, b], axis=1))
                want.append(-1 if (le0 is None and not other_le0) else int(bool(le0) or other_le0))
    # built against built: both values of a wave are special
    bc = built_cases(dt)
    for n in range(200):
        (_, va, la), (_, vb, lb) = bc[rs.integers(len(bc))], bc[rs.integers(len(bc))]
        rows.append(np.stack([va, vb], axis=1))
        want.append(-1 if (la is None or lb is None) else int(la or lb))
    # random partials: the dot products of a tree's momenta — 64 partials of mixed sign whose sum is small against Σ|x| in a good
    # share of the waves (shifted so that the exact sum is a few ulps of Σ|x| from 0), and plain ones
    for n in range(6000):
        x = rs.normal(size=(64, 2)) * 10.0 ** rs.integers(-8, 8)
        if n % 3:
            x -= x.mean(axis=0) * (1.0 + rs.normal(size=2) * 10.0 ** rs.integers(-17, -1, size=2))
        rows.append(x.astype(dt))
        want.append(-1)
    return np.stack(rows).astype(dt), np.array(want)


# =====================================================================================================================
# CPU part
# =====================================================================================================================
def test_probe_compiles_without_scratch_or_spills():
    """The probe compiles for gfx950 with build.FLAGS, and no wrapper needs scratch or spills (it would test the spill code)."""
    B = _build()
    co = B.build_probe_object(PROBE)
    assert os.path.exists(co)
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_meta
    finally:
        sys.path.pop(0)
    meta = kernel_meta.kernel_meta(co)
    names = {k["name"] for k in meta}
    for want in ("p_any_le0_f32", "p_any_le0_f64", "p_draw_streams"):
        assert want in names, want
    bad = [(k["name"], k.get("private_segment_fixed_size"), k.get("vgpr_spill_count"), k.get("sgpr_spill_count")) for k in meta
           if k.get("private_segment_fixed_size") or k.get("vgpr_spill_count") or k.get("sgpr_spill_count")]
    assert not bad, bad


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_built_cases_mean_what_they_say(dt):
    """The host's expectations of the built cases, checked against exact arithmetic (math.fsum) where the sum is finite — and the
    order-dependent cases really are order-dependent: two summation orders of the same row disagree about the sign."""
    import math

    seen_order = 0
    for name, v, le0 in built_cases(dt):
        assert v.dtype == dt and v.shape == (64,)
        if le0 is None:
            fwd = bwd = dt(0)
            for x in v:
                fwd = dt(fwd + x)
            for x in v[::-1]:
                bwd = dt(bwd + x)
            seen_order += int((fwd <= 0) != (bwd <= 0) or fwd != bwd)
        elif np.all(np.isfinite(v)):
            assert (math.fsum(v.astype(np.float64)) <= 0) == le0, name
        elif np.any(np.isnan(v)) or (np.any(v == np.inf) and np.any(v == -np.inf)):
            assert le0 is False, name   # NaN <= 0 is false
        else:
            assert le0 == bool(np.any(v == -np.inf)), name
    assert seen_order >= 40, seen_order


# =====================================================================================================================
# GPU part
# =====================================================================================================================
@pytest.fixture(scope="module")
def probe(hip):
    import torch

    from ahmc_amd.hipmod import Module

    torch.cuda.init()
    return Module(_build().build_probe_object(PROBE))


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_uturn_predicate_equals_allsum2_and_compares(probe, dt):
    """(a): in every lane of every wave, wave64_any_le0_pair(a, b) == (Σa <= 0 || Σb <= 0) with Σ from wave_allsum2<64>."""
    import torch

    x, want = predicate_inputs(dt)
    nw = x.shape[0]
    n = nw * 64
    out = torch.full((n * 2,), -7, dtype=torch.int32, device="cuda")
    sums = torch.full((n * 2,), float("nan"), dtype=torch.float64 if dt == np.float64 else torch.float32, device="cuda")
    probe.launch(f"p_any_le0_{TN[dt]}", (n + 255) // 256, 256, _dev(x.reshape(-1)), out, sums, np.int64(n))
    o = _host(out).reshape(nw, 64, 2)
    s = _host(sums).reshape(nw, 64, 2)
    fast, ref = o[:, :, 0], o[:, :, 1]
    assert set(np.unique(o)) <= {0, 1}, np.unique(o)
    # the reference is what the kernels computed before: the same bits of both sums in all 64 lanes
    sb = s.view(np.uint64 if dt == np.float64 else np.uint32)
    assert np.all(sb == sb[:, :1, :]), "wave_allsum2<64> did not return the same bits in every lane"
    assert np.all(ref == ref[:, :1]) and np.all(fast == fast[:, :1]), "a predicate differs between the lanes of a wave"
    with np.errstate(invalid="ignore"):
        assert np.array_equal(ref[:, 0] != 0, (s[:, 0, 0] <= 0) | (s[:, 0, 1] <= 0))
    bad = np.nonzero(fast[:, 0] != ref[:, 0])[0]
    print(f"{TN[dt]}: {nw} waves, predicate true in {int(ref[:, 0].sum())}, disagreements {len(bad)}")
    assert len(bad) == 0, (bad[:10], s[bad[:10], 0], x[bad[0]])
    # the host's own expectation where the case has one, and both outcomes well represented among the random partials
    known = want >= 0
    assert np.array_equal(fast[known, 0], want[known]), np.nonzero(fast[known, 0] != want[known])[0][:10]
    rnd = fast[-6000:, 0]
    assert 600 < rnd.sum() < 5400, rnd.sum()


@pytest.mark.gpu
def test_wide_draw_stream_equals_narrow_in_every_lane(probe):
    """(b): DrawStreamT<true> == DrawStreamT<false>, word for word, in every lane: from init and from every resume point."""
    import torch

    ref = _oracle_ref()
    seed, chain, it = 0x9E3779B97F4A7C15, 40507, 1234
    prm = np.array([seed & 0xFFFFFFFF, seed >> 32, chain, it], dtype=np.uint32)
    orng = ref.Rng(seed, chain, it)
    spec = np.array([orng._word() for _ in range(max(RESUME_AT) + N_AFTER_RESUME + 1)], dtype=np.uint32)
    for k0s, ndraw, use_init in ((np.zeros(3, np.uint32), N_FROM_INIT, 1), (np.array(RESUME_AT, np.uint32), N_AFTER_RESUME, 0)):
        nw = len(k0s)
        wide = torch.full((nw * ndraw * 64,), -7, dtype=torch.int32, device="cuda")
        narrow = torch.full((nw * ndraw * 64,), -9, dtype=torch.int32, device="cuda")
        probe.launch("p_draw_streams", (nw * 64 + 255) // 256, 256, _dev(prm.view(np.int32)), _dev(k0s.view(np.int32)), int(nw), int(ndraw),
                     int(use_init), wide, narrow)
        w = _host(wide).view(np.uint32).reshape(nw, ndraw, 64)
        nr = _host(narrow).view(np.uint32).reshape(nw, ndraw, 64)
        want = np.stack([spec[int(k0):int(k0) + ndraw] for k0 in k0s])
        assert np.array_equal(nr, np.broadcast_to(want[:, :, None], nr.shape)), "the narrow stream left the stream specification"
        bad = np.argwhere(w != nr)
        print(f"{'init' if use_init else 'resume'} at {len(k0s)} points x {ndraw} draws x 64 lanes: {len(bad)} words differ")
        assert len(bad) == 0, [(int(k0s[a]), int(k0s[a]) + int(b), int(c)) for a, b, c in bad[:10]]
