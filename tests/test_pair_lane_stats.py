"""The lane-parallel scalar work of a pair step of k_nuts (csrc/ahmc_device.hpp: wave64_pair_reduce_t + pair_leaf_stats)
against the serial form it replaced (wave64_pair_reduce, then the scalar block of k_nuts' single-leaf arm on each broadcast energy), on the
same data in tests/device_probe/pair_stats.hip: equal BITS for w, sa and ΔH of both leaves, equal redo and divergence flags, for the
linear-domain (LINW) and the log-domain kernels' expressions, f64 and f32.

The inputs are built and their coverage is checked in numpy, without a device (test_inputs_cover_*): every table bucket's two edges for
each leaf independently, ℓw around the linear domain's limit, below −1100 and in (−1100, −1075), ℓw = −Inf and NaN, sums that are ±Inf,
dot-product sums of ±1e300 / ±Inf / NaN in the lanes whose values the new form must never convert, Δ_max ∈ {0.5, 1000}; each leaf
diverges and each leaf is flagged `redo` in well over 1 % of the waves."""
import os
import sys

import numpy as np
import pytest

import ahmc_amd as A  # noqa: F401  (the package must import: the probe is compiled with its build module)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "device_probe", "pair_stats.hip")
N_WAVES = 4096
N_EDGE = 512                      # waves [0, 512): table-bucket edges
K64 = 92.33248261689366           # 64 / ln 2, the constant of leaf_weight_exp
LIMIT = {np.float64: 600.0, np.float32: 60.0}


def _edge_plan():
    """(wave, ja, side_a, jb, side_b, na, nb) for the 512 edge waves: leaf a walks the 64 buckets with both edges, leaf b walks them
    through the bijection j -> 5 j + c (mod 64), so the two leaves of a wave (almost always) read different table entries."""
    plan = []
    for j in range(64):
        for sa in range(2):
            for sb in range(2):
                for r in range(2):
                    w = ((j * 2 + sa) * 2 + sb) * 2 + r
                    jb = (5 * j + (3 if r == 0 else 20)) % 64
                    plan.append((w, j, sa, jb, sb, -8 + (w * 7) % 13, -8 + (w * 11 + 5) % 13))
    return plan


def _edge_value(n, j, side):
    k = 64 * n + j
    return (k - 0.5 + 1e-7) / K64 if side == 0 else (k + 0.5 - 1e-7) / K64


def _inputs(dt):
    """x: (N_WAVES, 64, 4) lane partials ea, eb, da, db;  par: (N_WAVES, 2) H0, Δ_max;  tgt: (N_WAVES, 2) the ℓw each leaf was aimed at
    (NaN where the energy was made non-finite on purpose)."""
    rs = np.random.default_rng(20251 if dt == np.float64 else 20252)
    lim = LIMIT[dt]
    big = 1e300 if dt == np.float64 else 1e30
    x = np.zeros((N_WAVES, 64, 4), dtype=np.float64)
    par = np.zeros((N_WAVES, 2), dtype=np.float64)
    tgt = np.full((N_WAVES, 2), np.nan)
    par[:, 1] = np.where(np.arange(N_WAVES) % 2 == 0, 0.5, 1000.0)
    # ---- table-bucket edges: H0 = 0 and ONE non-zero lane per energy, so that the sum, and with it ℓw, is exactly the aimed value ----
    for w, ja, sa, jb, sb, na, nb in _edge_plan():
        va, vb = _edge_value(na, ja, sa), _edge_value(nb, jb, sb)
        x[w, (w * 5) % 64, 0] = va
        x[w, (w * 3 + 7) % 64, 1] = vb
        tgt[w] = (va, vb)
    # ---- the rest: random lane partials over several binades, one lane corrected so that the sum lands near the aimed ℓw − H0 ----
    R = np.arange(N_EDGE, N_WAVES)
    par[R, 0] = np.round(rs.standard_normal(len(R)) * 20.0, 3)
    cat = rs.integers(0, 10, size=(len(R), 2))
    u = rs.random((len(R), 2))
    lw = np.select(
        [cat <= 2, cat == 3, cat == 4, cat == 5, cat == 6, cat == 7, cat == 8],
        [-30.0 + 35.0 * u,                                            # the bulk of a real run
         lim + (u - 0.5) * np.exp2(rs.integers(-30, 1, size=u.shape)),    # just below / above the linear domain's limit
         lim + 1e-3 + (lim / 6) * u,                                   # above it: redo
         -1100.0 - 1e-3 - 500.0 * u,                                   # below the clamp of the weight's exp
         -1075.0 - 25.0 * u,                                           # between the underflow and the clamp
         -1075.0 + 80.0 * u,                                           # subnormal weights and the smallest normal ones
         -0.5 + (u - 0.5) * 1e-6],                                     # at the divergence threshold of Δ_max = 0.5 … and far from Δ_max = 1000's
        default=np.nan)                                                # cat 9: a non-finite energy, below
    part = rs.standard_normal((len(R), 64, 2)) * np.exp2(rs.integers(-6, 4, size=(len(R), 64, 2)))
    want = lw - par[R, 0][:, None]
    fix = rs.integers(0, 64, size=(len(R), 2))
    for c in range(2):
        s = part[:, :, c].sum(axis=1) - part[np.arange(len(R)), fix[:, c], c]
        part[np.arange(len(R)), fix[:, c], c] = np.where(np.isnan(want[:, c]), 0.0, want[:, c] - s)
    x[R, :, 0:2] = part
    tgt[R] = lw
    # non-finite energies (ℓw = −Inf after the sanitising): +Inf, −Inf, both (NaN), NaN, and two finite partials that overflow in the sum
    near = float(np.finfo(dt).max) * 0.7
    bad = [(np.inf,), (-np.inf,), (np.inf, -np.inf), (np.nan,), (near, near)]
    for c in range(2):
        rows = R[cat[:, c] == 9]
        for n, w in enumerate(rows):
            for m, v in enumerate(bad[n % 5]):
                x[w, (w * 5 + 31 * m + c) % 64, c] = v
    # H0 that is not finite in a few waves: ℓw = NaN (H0 = NaN; H0 = +Inf against ne = −Inf) and ℓw = ±Inf
    par[N_EDGE + 0:N_EDGE + 40:4, 0] = np.nan
    par[N_EDGE + 1:N_EDGE + 40:4, 0] = np.inf
    par[N_EDGE + 2:N_EDGE + 40:8, 0] = -np.inf
    # ---- U-turn dot products: random everywhere; every third wave, edge waves included, carries sums of ±big, ±Inf or NaN in lanes 0 / 1 ----
    x[:, :, 2:4] = rs.standard_normal((N_WAVES, 64, 2)) * np.exp2(rs.integers(-8, 9, size=(N_WAVES, 64, 2)))
    garbage = [big, -big, np.inf, -np.inf, np.nan]
    for w in range(0, N_WAVES, 3):
        g = garbage[(w // 3) % 5]
        which = (w // 15) % 3    # da, db or both
        if which in (0, 2):
            x[w, (w * 7) % 64, 2] = g
        if which in (1, 2):
            x[w, (w * 7 + 9) % 64, 3] = garbage[(w // 3 + 2) % 5]
    with np.errstate(over="ignore"):
        return x.astype(dt), par.astype(dt), tgt


def _numpy_view(dt):
    """What numpy makes of the inputs: the sanitised energies, ℓw and the two flags per leaf (sums in numpy's order: the last bits may
    differ from the device's butterfly, which matters to none of the coverage counts below)."""
    x, par, tgt = _inputs(dt)
    with np.errstate(invalid="ignore", over="ignore"):
        s = x[:, :, 0:2].astype(np.float64).sum(axis=1).astype(dt)
        ne = np.where(np.isfinite(s), s, -np.inf).astype(dt)
        H0, dmax = par[:, 0:1], par[:, 1:2]
        lw = (H0 + ne).astype(dt)
        div = ~(-H0 < dmax + ne)
        redo = lw > dt(LIMIT[dt])
        dots = x[:, :, 2:4].astype(np.float64).sum(axis=1)
    return x, par, tgt, s, lw, div, redo, dots


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_inputs_cover_every_case_before_a_device_runs(dt):
    x, par, tgt, s, lw, div, redo, dots = _numpy_view(dt)
    lim = LIMIT[dt]
    assert x.shape == (N_WAVES, 64, 4) and par.shape == (N_WAVES, 2)
    assert set(np.unique(par[:, 1]).tolist()) == {0.5, 1000.0}
    for c, leaf in enumerate("ab"):
        assert div[:, c].mean() >= 0.01 and (~div[:, c]).mean() >= 0.01, (leaf, float(div[:, c].mean()))
        assert redo[:, c].mean() >= 0.01, (leaf, float(redo[:, c].mean()))
        for dm in (0.5, 1000.0):
            sel = par[:, 1] == dm
            assert div[sel, c].mean() >= 0.01 and (~div[sel, c]).mean() >= 0.01, (leaf, dm)
        l = lw[:, c].astype(np.float64)
        assert np.isneginf(l).sum() >= 20 and np.isnan(l).sum() >= 5, leaf                       # ℓw = −Inf, NaN
        assert np.isposinf(s[:, c]).sum() >= 5 and np.isneginf(s[:, c]).sum() >= 5, leaf           # sums that are ±Inf
        assert np.isnan(s[:, c]).sum() >= 5, leaf
        assert ((l > lim - 1e-3) & (l <= lim)).sum() >= 20 and ((l > lim) & (l < lim + 1e-3)).sum() >= 20, leaf
        assert (np.isfinite(l) & (l < -1100)).sum() >= 40 and ((l > -1100) & (l < -1075)).sum() >= 40, leaf
    # both edges of all 64 table buckets, for each leaf on its own; ℓw of an edge wave IS the aimed value (f64: exactly)
    E = slice(0, N_EDGE)
    assert (par[E, 0] == 0).all()
    if dt == np.float64:
        assert (lw[E] == tgt[E]).all()
        k = np.rint(lw[E] * K64)
        frac = lw[E] * K64 - k
        for c in range(2):
            lo = {int(v) & 63 for v in k[frac[:, c] < -0.49, c]}
            hi = {int(v) & 63 for v in k[frac[:, c] > 0.49, c]}
            assert lo == set(range(64)) and hi == set(range(64)), c
        assert np.abs(frac).min() > 0.49
        assert ((k[:, 0].astype(np.int64) & 63) != (k[:, 1].astype(np.int64) & 63)).mean() > 0.9      # two different table entries in one wave
        assert (lw[E] > 0).any() and (lw[E] < 0).any()
    # garbage in the lanes that hold dot-product sums
    big = 1e300 if dt == np.float64 else 1e30
    for c in range(2):
        d = dots[:, c]
        assert (d >= big / 2).sum() >= 20 and (d <= -big / 2).sum() >= 20 and np.isposinf(d).sum() >= 20 and np.isneginf(d).sum() >= 20 and np.isnan(d).sum() >= 20, c
    dE = dots[E]
    assert (~np.isfinite(dE) | (np.abs(dE) >= big / 2)).any(axis=1).sum() >= 100                      # … in the edge waves as well


def test_pair_stats_probe_compiles_without_scratch_or_spills():
    """The probe compiles for gfx950 with the engine's flags and needs neither scratch nor spills: a wrapper that spilled would test the
    spill code, not the two forms."""
    from ahmc_amd import build as B

    co = B.build_probe_object(PROBE)
    assert os.path.exists(co)
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_meta
    finally:
        sys.path.pop(0)
    meta = kernel_meta.kernel_meta(co)
    names = {k["name"] for k in meta}
    for want in ("p_pair_stats_f64", "p_pair_stats_f32"):
        assert want in names, want
    bad = [(k["name"], k.get("private_segment_fixed_size"), k.get("vgpr_spill_count"), k.get("sgpr_spill_count")) for k in meta
           if k.get("private_segment_fixed_size") or k.get("vgpr_spill_count") or k.get("sgpr_spill_count")]
    assert not bad, bad


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_lane_parallel_stats_have_the_serial_forms_bits(hip, dt):
    """4 096 waves, one launch: w, sa and ΔH of leaf a and of leaf b with the SAME BITS in both forms, the four flags equal — for the
    linear-domain expressions (LINW) and the log-domain ones; the two reductions take the same U-turn decision."""
    import torch

    from ahmc_amd import build as B
    from ahmc_amd.hipmod import Module

    torch.cuda.init()
    mod = Module(B.build_probe_object(PROBE))
    tn = "f64" if dt == np.float64 else "f32"
    x, par, tgt, s, lw, div, redo, dots = _numpy_view(dt)
    n = N_WAVES * 64
    tdt = torch.float64 if dt == np.float64 else torch.float32
    xin = torch.from_numpy(np.ascontiguousarray(x.reshape(-1))).cuda()
    pin = torch.from_numpy(np.ascontiguousarray(par.reshape(-1))).cuda()
    o = torch.full((N_WAVES * 42,), float("nan"), dtype=tdt, device="cuda")
    mod.launch(f"p_pair_stats_{tn}", n // 256, 256, xin, pin, o, np.int64(n))
    torch.cuda.synchronize()
    y = o.cpu().numpy().reshape(N_WAVES, 2, 21)
    for li, kind in enumerate(("LINW", "log-domain")):
        ser, par_, same_turn = y[:, li, 0:10], y[:, li, 10:20], y[:, li, 20]
        assert (same_turn == 1).all(), kind
        assert np.isin(ser[:, 6:], (0, 1)).all() and np.isin(par_[:, 6:], (0, 1)).all(), kind
        names = ("w_a", "sa_a", "dH_a", "w_b", "sa_b", "dH_b", "redo_a", "div_a", "redo_b", "div_b")
        for j, nm in enumerate(names):
            diff = np.flatnonzero(_bits(ser[:, j]) != _bits(par_[:, j]))
            print(f"{tn} {kind} {nm}: {len(diff)} of {N_WAVES} waves differ")
            assert len(diff) == 0, (kind, nm, diff[:8].tolist(), ser[diff[:4], j].tolist(), par_[diff[:4], j].tolist())
        # the serial form is the reference, and it saw what the inputs were built for
        for c in range(2):
            assert ser[:, 7 + 2 * c].mean() >= 0.01, (kind, "divergent", c)
            if li == 0:
                assert ser[:, 6 + 2 * c].mean() >= 0.01, (kind, "redo", c)
            else:
                assert (ser[:, 6 + 2 * c] == 0).all()
        assert np.isnan(ser[:, 0]).any() and (ser[:, 1] == 1).any() and (ser[:, 1] == 0).any(), kind
    # the divergence flags of the serial form against numpy wherever ℓw is at least 0.05 from the threshold −Δ_max (the sums are below 2 000:
    # more than a hundred ulp of either type, and the two orders of summation differ by a few)
    with np.errstate(invalid="ignore"):
        far = np.abs(lw.astype(np.float64) + par[:, 1:2].astype(np.float64)) > 0.05
    ser_div = y[:, 0, [7, 9]] != 0
    assert (ser_div[far] == div[far]).all()
