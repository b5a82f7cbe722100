"""The octo step of k_nuts (csrc/ahmc_nuts.hpp: OCT — eight leaves per step from the fourth doubling on, where a chain owns a wave).

a. its one reduction and its one lane-parallel scalar pass (csrc/ahmc_device.hpp: wave64_oct_rows_de + wave64_oct_rows + wave64_oct_reduce_t,
   oct_leaf_stats) in tests/device_probe/oct_red.hip next to what they replace, on the same data: wave64_quad_reduce_t + quad_leaf_stats on
   (a,b,c,d) and on (e,f,g,h), wave64_any_le0_pair on the level-2 dot products — equal BITS for every energy, w, sa and ΔH, equal flags, all
   seven U-turn decisions, for the linear-domain and the log-domain expressions, f64 and f32; and the same primitives with the first half's
   row given as the second half's too (the quad step of the third doubling in these kernels) against the quad's.  The inputs follow tests/test_leaf_quads.py's
   recipe extended to eight leaves, and their coverage is asserted in numpy before a device runs;
b. the shipped library reproduces, bit for bit, tests/golden/leaf_oct_parent.npz — chains recorded from the library of the parent commit
   (four leaves per step; tests/golden/make_leaf_oct_golden.py: the cases, and how) — one iteration per call and in one fused call.  The
   fixture itself is held to the exits each case exists for, so that the comparison cannot pass by leaving the paths out;
c. the same cases against the CPU oracle under the margin rule of tests/parity_util.py.
"""
import importlib.util
import os
import sys

import numpy as np
import pytest

import ahmc_amd as A
import parity_util as PU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "device_probe", "oct_red.hip")
N_WAVES = 4096
N_EDGE = 512                      # waves [0, 512): table-bucket edges
K64 = 92.33248261689366           # 64 / ln 2, the constant of leaf_weight_exp
LIMIT = {np.float64: 600.0, np.float32: 60.0}
NL = 8                            # leaves
NM = 7                            # merges: (a,b), (c,d), level 1 of abcd, (e,f), (g,h), level 1 of efgh, level 2
NX = NL + 2 * NM                  # values per lane
BLOCK = 59                        # values per form (oct_red.hip)
LEAVES = "abcdefgh"
MERGES = ("ab", "cd", "abcd", "ef", "gh", "efgh", "l2")


def _gen():
    spec = importlib.util.spec_from_file_location("make_leaf_oct_golden", os.path.join(ROOT, "tests", "golden", "make_leaf_oct_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _gen()
CASES = sorted(GEN.CASES)


@pytest.fixture(scope="module")
def golden():
    with np.load(GEN.FIXTURE) as z:
        return {k: z[k] for k in z.files}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _same_bits(a, b):
    """bitwise equal, with any NaN equal to any NaN (payloads are not specified)"""
    a, b = np.asarray(a), np.asarray(b)
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


# =====================================================================================================================
# a. the probe's inputs (numpy only)
# =====================================================================================================================
def _edge_value(n, j, side):
    k = 64 * n + j
    return (k - 0.5 + 1e-7) / K64 if side == 0 else (k + 0.5 - 1e-7) / K64


def _edge_plan():
    """(wave, [(j, side, n)] of the eight leaves) for the 512 edge waves: leaf a walks the 64 buckets with both edges four times over; leaf c
    walks them through the bijection j -> (4c + 1) j + offset (mod 64) (an odd multiplier), with its side taken from other bits of the wave
    index — so every leaf sees both edges of all 64 buckets, and the eight leaves of a wave read mostly different table entries."""
    plan = []
    for w in range(N_EDGE):
        j, s, r = w >> 3, (w >> 2) & 1, w & 3
        leaves = [(j, s, -8 + (w * 7) % 13)]
        for c in range(1, NL):
            side = ((w >> (c % 3)) ^ (w >> ((c + 1) % 3)) ^ (c >> 2)) & 1 if c >= 4 else ((w >> 1) & 1, w & 1, ((w >> 1) ^ w) & 1)[c - 1]
            leaves.append((((4 * c + 1) * j + 3 + 11 * c + (17 - 2 * c) * r) % 64, side, -8 + (w * (2 * c + 3) + 5 * c) % 13))
        plan.append((w, leaves))
    return plan


def _garbage_subset(w):
    """which of the seven merges carry a garbage dot product in wave w: every subset of the seven, 32 times over"""
    return [(w >> m) & 1 for m in range(NM)]


def _inputs(dt):
    """x: (N_WAVES, 64, 22) lane partials e_a .. e_h, then two dot products for each of the seven merges;  par: (N_WAVES, 2) H0, Δ_max;
    tgt: (N_WAVES, 8) the ℓw each leaf was aimed at (NaN where the energy was made non-finite on purpose)."""
    rs = np.random.default_rng(20271 if dt == np.float64 else 20272)
    lim = LIMIT[dt]
    big = 1e300 if dt == np.float64 else 1e30
    x = np.zeros((N_WAVES, 64, NX), dtype=np.float64)
    par = np.zeros((N_WAVES, 2), dtype=np.float64)
    tgt = np.full((N_WAVES, NL), np.nan)
    par[:, 1] = np.where((np.arange(N_WAVES) >> 7) % 2 == 0, 0.5, 1000.0)
    # ---- table-bucket edges: H0 = 0 and ONE non-zero lane per energy, so that the sum, and with it ℓw, is exactly the aimed value ----
    for w, leaves in _edge_plan():
        for c, (j, side, n) in enumerate(leaves):
            v = _edge_value(n, j, side)
            x[w, (w * 5 + 19 * c) % 64, c] = v
            tgt[w, c] = v
    # ---- the rest: random lane partials over several binades, one lane corrected so that the sum lands near the aimed ℓw − H0 ----
    R = np.arange(N_EDGE, N_WAVES)
    par[R, 0] = np.round(rs.standard_normal(len(R)) * 20.0, 3)
    cat = rs.integers(0, 10, size=(len(R), NL))
    u = rs.random((len(R), NL))
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
    part = rs.standard_normal((len(R), 64, NL)) * np.exp2(rs.integers(-6, 4, size=(len(R), 64, NL)))
    want = lw - par[R, 0][:, None]
    fix = rs.integers(0, 64, size=(len(R), NL))
    for c in range(NL):
        s = part[:, :, c].sum(axis=1) - part[np.arange(len(R)), fix[:, c], c]
        part[np.arange(len(R)), fix[:, c], c] = np.where(np.isnan(want[:, c]), 0.0, want[:, c] - s)
    x[R, :, 0:NL] = part
    tgt[R] = lw
    # non-finite energies (ℓw = −Inf after the sanitising): +Inf, −Inf, both (NaN), NaN, and two finite partials that overflow in the sum
    near = float(np.finfo(dt).max) * 0.7
    bad = [(np.inf,), (-np.inf,), (np.inf, -np.inf), (np.nan,), (near, near)]
    for c in range(NL):
        rows = R[cat[:, c] == 9]
        for n, w in enumerate(rows):
            for m, v in enumerate(bad[n % 5]):
                x[w, (w * 5 + 31 * m + c) % 64, c] = v
    # H0 that is not finite in a few waves: ℓw = NaN (H0 = NaN; H0 = +Inf against ne = −Inf) and ℓw = ±Inf
    par[N_EDGE + 0:N_EDGE + 80:4, 0] = np.nan
    par[N_EDGE + 1:N_EDGE + 80:4, 0] = np.inf
    par[N_EDGE + 2:N_EDGE + 80:8, 0] = -np.inf
    # ---- U-turn dot products: random everywhere; the merges of _garbage_subset(w) carry sums of ±big, ±Inf or NaN — in the first dot
    # product, the second or both — so every combination of the seven merges occurs, edge waves included ----
    x[:, :, NL:] = rs.standard_normal((N_WAVES, 64, 2 * NM)) * np.exp2(rs.integers(-8, 9, size=(N_WAVES, 64, 2 * NM)))
    garbage = [big, -big, np.inf, -np.inf, np.nan]
    for w in range(N_WAVES):
        t = w >> 7
        for m, on in enumerate(_garbage_subset(w)):
            if not on:
                continue
            which = (t + m) % 3     # first dot product, second, or both
            if which in (0, 2):
                x[w, (w * 7 + 11 * m) % 64, NL + 2 * m] = garbage[(t + w + m) % 5]
            if which in (1, 2):
                x[w, (w * 7 + 9 + 11 * m) % 64, NL + 1 + 2 * m] = garbage[(t + w + 2 + m) % 5]
    with np.errstate(over="ignore"):
        return x.astype(dt), par.astype(dt), tgt


_VIEW = {}


def _numpy_view(dt):
    """What numpy makes of the inputs: the sanitised energies, ℓw and the two flags per leaf (sums in numpy's order: the last bits may
    differ from the device's butterfly, which matters to none of the coverage counts below).  Computed once per dtype."""
    if dt not in _VIEW:
        x, par, tgt = _inputs(dt)
        with np.errstate(invalid="ignore", over="ignore"):
            s = x[:, :, 0:NL].astype(np.float64).sum(axis=1).astype(dt)
            ne = np.where(np.isfinite(s), s, -np.inf).astype(dt)
            H0, dmax = par[:, 0:1], par[:, 1:2]
            lw = (H0 + ne).astype(dt)
            div = ~(-H0 < dmax + ne)
            redo = lw > dt(LIMIT[dt])
            dots = x[:, :, NL:].astype(np.float64).sum(axis=1)
        _VIEW[dt] = (x, par, tgt, s, lw, div, redo, dots)
    return _VIEW[dt]


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_inputs_cover_every_case_before_a_device_runs(dt):
    x, par, tgt, s, lw, div, redo, dots = _numpy_view(dt)
    lim = LIMIT[dt]
    assert x.shape == (N_WAVES, 64, NX) and par.shape == (N_WAVES, 2)
    assert set(np.unique(par[:, 1]).tolist()) == {0.5, 1000.0}
    for c, leaf in enumerate(LEAVES):
        assert div[:, c].mean() >= 0.01 and (~div[:, c]).mean() >= 0.01, (leaf, float(div[:, c].mean()))
        assert redo[:, c].mean() >= 0.01, (leaf, float(redo[:, c].mean()))
        for dm in (0.5, 1000.0):
            sel = par[:, 1] == dm
            assert div[sel, c].mean() >= 0.01 and (~div[sel, c]).mean() >= 0.01, (leaf, dm)
        l = lw[:, c].astype(np.float64)
        assert np.isneginf(l).sum() >= 20 and np.isnan(l).sum() >= 5, leaf                       # ℓw = −Inf, NaN
        assert np.isposinf(s[:, c]).sum() >= 5 and np.isneginf(s[:, c]).sum() >= 5, leaf           # sums that are ±Inf
        assert np.isnan(s[:, c]).sum() >= 5, leaf
        assert ((l > lim - 1e-3) & (l <= lim)).sum() >= 20 and ((l > lim) & (l < lim + 1e-3)).sum() >= 20, leaf   # ± the linear domain's limit
        assert (np.isfinite(l) & (l < -1100)).sum() >= 40 and ((l > -1100) & (l < -1075)).sum() >= 40, leaf
    # both edges of all 64 table buckets, for each of the eight lane classes on its own; ℓw of an edge wave IS the aimed value (f64: exactly)
    E = slice(0, N_EDGE)
    assert (par[E, 0] == 0).all()
    if dt == np.float64:
        assert (lw[E] == tgt[E]).all()
        k = np.rint(lw[E] * K64)
        frac = lw[E] * K64 - k
        for c in range(NL):
            lo = {int(v) & 63 for v in k[frac[:, c] < -0.49, c]}
            hi = {int(v) & 63 for v in k[frac[:, c] > 0.49, c]}
            assert lo == set(range(64)) and hi == set(range(64)), c
        assert np.abs(frac).min() > 0.49
        kk = k.astype(np.int64) & 63
        distinct = np.array([len(set(row.tolist())) for row in kk])
        assert (distinct >= 6).mean() > 0.8 and (distinct >= 4).all()      # mostly different table entries in one wave
        # … and in particular the two halves differ: leaf k and leaf k + 4 (the same lane & 3, one row apart) read different entries
        assert (kk[:, 0:4] != kk[:, 4:8]).mean() > 0.9
        assert (lw[E] > 0).any() and (lw[E] < 0).any()
    # garbage in the lanes that hold dot-product sums, for each of the fourteen, and every combination of the seven merges
    big = 1e300 if dt == np.float64 else 1e30
    for c in range(2 * NM):
        d = dots[:, c]
        assert (d >= big / 2).sum() >= 20 and (d <= -big / 2).sum() >= 20 and np.isposinf(d).sum() >= 20 and np.isneginf(d).sum() >= 20 and np.isnan(d).sum() >= 20, c
    g = ~np.isfinite(dots) | (np.abs(dots) >= big / 2)
    gm = g[:, 0::2] | g[:, 1::2]                                  # per merge
    code = (gm * (1 << np.arange(NM))).sum(axis=1)
    assert (np.bincount(code, minlength=1 << NM) >= 16).all()     # all 128 subsets of the seven merges
    assert (np.bincount(code[E], minlength=1 << NM) >= 2).all()   # … in the edge waves as well
    for m in range(NM):                                           # first, second and both, for every merge
        assert (g[:, 2 * m] & ~g[:, 2 * m + 1]).sum() >= 100 and (~g[:, 2 * m] & g[:, 2 * m + 1]).sum() >= 100 and (g[:, 2 * m] & g[:, 2 * m + 1]).sum() >= 100, m


def test_oct_probe_compiles_without_scratch_or_spills():
    """The probe compiles for gfx950 with the engine's flags and needs neither scratch nor spills: a wrapper that spilled would test the
    spill code, not the primitives."""
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
    for want in ("p_oct_red_f64", "p_oct_red_f32"):
        assert want in names, want
    bad = [(k["name"], k.get("private_segment_fixed_size"), k.get("vgpr_spill_count"), k.get("sgpr_spill_count")) for k in meta
           if k.get("private_segment_fixed_size") or k.get("vgpr_spill_count") or k.get("sgpr_spill_count")]
    assert not bad, bad


# =====================================================================================================================
# b. the fixture (numpy only)
# =====================================================================================================================
def _case_record(golden, name):
    return {k.split("/", 1)[1]: v for k, v in golden.items() if k.startswith(name + "/")}


def _assert_exits(name, ns, ne):
    """the exits of the octo step the case exists for, on (n_steps, numerical_error): each occurs at least once — a missing position is a
    failure of the case"""
    div, inside = GEN.oct_ends(ns, ne)
    if name.startswith("div_uturn_"):
        assert min(inside) >= 1, (name, "non-divergent ends inside a subtree at p = 2 / 4 / 6 / 0 mod 8", inside)
    elif name.startswith("div_md4_"):
        assert sum(div) >= 1 and ((ns == 15) & (ne == 0)).sum() >= 1, (name, div)
    elif name.startswith("div_"):
        assert min(div) >= 1, (name, "divergent ends on a .. h", div)
    return div, inside


def _assert_reason_for_existing(name, rec):
    """Every case is there for an exit of the octo step; `rec` (a record of run_case, or the fixture's) must show that the case took it."""
    D, dt, max_depth, delta_max, _, n_adapts, n_total, _ = GEN.CASES[name]
    ns, ne, dep = rec["n_steps"], rec["numerical_error"], rec["tree_depth"]
    assert ns.shape == (n_total, GEN.N), name
    assert ns.max() <= 2 ** max_depth - 1 and dep.max() <= max_depth, name
    out = _assert_exits(name, ns, ne)
    over = GEN.handed_over(rec, name)
    if name.startswith("div_md4_"):
        assert delta_max == 0.1 and max_depth == 4, name
    elif name.startswith("md4_adapt_"):
        full = (dep == 4) & (ne == 0)                                  # leaf, pair, quad and exactly one octo
        assert max_depth == 4 and full.sum() >= 1000 and (ns[full] == 15).all(), (name, int(full.sum()))
        assert full[:n_adapts].sum() >= 100 and full[n_adapts:].sum() >= 100, name      # in the warm-up kernel and in the draws kernel
        assert np.abs(rec["metric_head"] - 1).max() > 0.05, name      # the window end did update M⁻¹
    elif name.endswith("_far"):
        assert over[:n_adapts].sum() >= 5, (name, int(over[:n_adapts].sum()))           # −ΔH > 600 in the warm-up: MODE 4
    elif name.startswith("fardraws_"):
        assert n_adapts == 0 and over.sum() >= 5 and ns[over].max() >= 8, (name, int(over.sum()))   # MODE 1, with trees that reach the fourth doubling
    elif name.startswith("div_uturn_"):
        assert delta_max == 1000.0, name
    else:
        assert delta_max in (0.1, 0.05), name
    return out


def test_fixture_takes_every_exit_of_the_octo_step(golden):
    """The fixture itself: every case is there at its recorded length, it is below the committed-file limit, and each case shows the exits
    it exists for (tests/golden/make_leaf_oct_golden.py): a divergent end on EACH of the eight leaves of an octo; non-divergent ends inside
    an unfinished subtree at p ≡ 2, 4, 6 and 0 (mod 8); one-octo trees that are complete whenever they reach depth 4; transitions handed to
    the log-domain kernels."""
    assert os.path.getsize(GEN.FIXTURE) < 1000 * 1024
    assert {k.split("/", 1)[0] for k in golden} == set(CASES)
    for name in CASES:
        rec = _case_record(golden, name)
        assert rec["theta_head"].shape == (GEN.CASES[name][6], 2, GEN.N), name
        print(name, _assert_reason_for_existing(name, rec))


# =====================================================================================================================
# GPU part
# =====================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_oct_reduce_and_stats_have_the_quad_forms_bits(hip, dt):
    """a. 4 096 waves, one launch: the eight energy sums, w, sa and ΔH of the eight leaves with the SAME BITS in both forms, the sixteen flags
    and the seven U-turn decisions equal — for the linear-domain expressions (LINW) and the log-domain ones."""
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
    assert xin.numel() == n * NX and pin.numel() == N_WAVES * 2
    o = torch.full((N_WAVES * 6 * BLOCK,), float("nan"), dtype=tdt, device="cuda")
    mod.launch(f"p_oct_red_{tn}", n // 256, 256, xin, pin, o, np.int64(n))
    torch.cuda.synchronize()
    y = o.cpu().numpy().reshape(N_WAVES, 2, 3, BLOCK)
    names = [f"e_{l}" for l in LEAVES] + [f"{f}_{l}" for l in LEAVES for f in ("w", "sa", "dH")] + [f"{f}_{l}" for l in LEAVES for f in ("redo", "div")] + \
            [f"turn_{m}" for m in MERGES]
    assert len(names) == 55
    n_diff = 0
    for li, kind in enumerate(("LINW", "log-domain")):
        ref, octo = y[:, li, 0], y[:, li, 1]
        assert np.isin(ref[:, 32:55], (0, 1)).all() and np.isin(octo[:, 32:55], (0, 1)).all(), kind
        for j, nm in enumerate(names):
            diff = np.flatnonzero(~_same_bits(ref[:, j], octo[:, j]))
            n_diff += len(diff)
            print(f"{tn} {kind} {nm}: {len(diff)} of {N_WAVES} waves differ")
            assert len(diff) == 0, (kind, nm, diff[:8].tolist(), ref[diff[:4], j].tolist(), octo[diff[:4], j].tolist())
        # the half form (the octo's primitives with the first half's row as the second half's too: the quad step of the third doubling in the
        # kernels with the octo step): leaves a .. d and their three decisions
        half = y[:, li, 2]
        half_idx = [j for j, nm in enumerate(names) if nm.split("_")[-1] in ("a", "b", "c", "d", "ab", "cd", "abcd")]
        assert len(half_idx) == 4 + 12 + 8 + 3
        for j in half_idx:
            diff = np.flatnonzero(~_same_bits(ref[:, j], half[:, j]))
            n_diff += len(diff)
            assert len(diff) == 0, (kind, "half form", names[j], diff[:8].tolist(), ref[diff[:4], j].tolist(), half[diff[:4], j].tolist())
        assert np.isin(half[:, [32, 33, 34, 35, 36, 37, 38, 39, 48, 49, 50]], (0, 1)).all(), kind
        # the quad form is the reference, and it saw what the inputs were built for
        for c in range(NL):
            assert ref[:, 33 + 2 * c].mean() >= 0.01, (kind, "divergent", c)
            if li == 0:
                assert ref[:, 32 + 2 * c].mean() >= 0.01, (kind, "redo", c)
            else:
                assert (ref[:, 32 + 2 * c] == 0).all()
            assert np.isnan(ref[:, 8 + 3 * c]).any() and (ref[:, 9 + 3 * c] == 1).any() and (ref[:, 9 + 3 * c] == 0).any(), (kind, c)
        for j in range(48, 55):
            assert 0.2 < ref[:, j].mean() < 0.95, (kind, names[j], float(ref[:, j].mean()))
    assert n_diff == 0
    # the divergence flags of the reference against numpy wherever ℓw is at least 0.05 from the threshold −Δ_max
    with np.errstate(invalid="ignore"):
        far = np.abs(lw.astype(np.float64) + par[:, 1:2].astype(np.float64)) > 0.05
    ref_div = y[:, 0, 0][:, 33:48:2] != 0
    assert (ref_div[far] == div[far]).all()


def _compare(name, rec, golden, what):
    for f in GEN.PER_TRANSITION + ("theta_sum", "theta_head"):
        a, b = rec[f], golden[f"{name}/{f}"]
        assert a.dtype == b.dtype and a.shape == b.shape, (name, f, a.dtype, b.dtype)
        same = _same_bits(a, b) if a.dtype.kind == "f" else (a == b)
        if not same.all():
            it = int(np.argwhere(~same.reshape(same.shape[0], -1).all(axis=1))[0, 0])
            raise AssertionError(f"{name} ({what}): {f} differs from the parent's first at transition {it + 1} "
                                 f"(chains {np.flatnonzero(~same[it].reshape(-1, GEN.N).all(axis=0) if same[it].ndim > 1 else ~same[it])[:8].tolist()})")
    assert (rec["metric_sum"] == golden[f"{name}/metric_sum"]).all() and _same_bits(rec["metric_head"], golden[f"{name}/metric_head"]).all(), (name, what, "M⁻¹")


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_same_chains_as_the_quad_loop(hip, golden, name):
    """b. every recorded transition of the case, one iteration per call, bit for bit; then the whole run again in ONE call (launches of
    many transitions): the same draws, final state and M⁻¹."""
    D, dt, max_depth, _, _, n_adapts, n_total, _ = GEN.CASES[name]
    probe, _, _, _ = GEN.setup(A, hip, name)
    if hip.backend == "hip:gfx950":
        assert (probe.info("group_lanes"), probe.info("elems_per_lane")) == GEN.GEOMETRY[D], name
    probe.close()
    rec = GEN.run_case(A, hip, name)
    _assert_reason_for_existing(name, rec)     # (on what THIS library ran, not only on the fixture)
    _compare(name, rec, golden, "one iteration per call")
    e, k, _, _ = GEN.setup(A, hip, name)
    out = np.zeros((D, GEN.N, n_total - n_adapts), dtype=rec["theta_head"].dtype, order="F")
    e.run(k, n_total, n_adapts, drop_warmup=n_adapts > 0, samples_out=out)
    e.sync()
    sums = np.stack([GEN.theta_sum(out[:, :, j]) for j in range(out.shape[2])])
    assert (sums == golden[f"{name}/theta_sum"][n_adapts:]).all(), (name, "draws of the one-call run")
    assert (GEN.theta_sum(e.theta()) == golden[f"{name}/theta_sum"][-1]).all() and (GEN.theta_sum(e.get_metric()) == golden[f"{name}/metric_sum"]).all(), name
    st = e.stats(list(GEN.PER_TRANSITION))
    for f in GEN.PER_TRANSITION:
        assert _same_bits(st[f], golden[f"{name}/{f}"][-1]).all() if st[f].dtype.kind == "f" else (st[f] == golden[f"{name}/{f}"][-1]).all(), (name, f)
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_oct_step_against_oracle(hip, oracle, name):
    """c. the same cases against the CPU oracle, one iteration at a time from the oracle's complete state: a chain may leave the oracle's
    track — n_steps, tree depth, divergence flag, position — only where the oracle took a decision within the margin bound of a tie
    (tests/parity_util.py), as in tests/test_leaf_quads.py::test_quad_step_against_oracle.  The bar applies to the transitions that were
    numerically stable on the oracle (|ΔH|_max < 2) or short (<= 8 leapfrogs); without adaptation ϵ stays at its fixed value inside the
    leapfrog's stability bound (ϵ < 2 for the unit Gaussian) and every chain is held to it."""
    D, dt, max_depth, delta_max, _, n_adapts, n_total, off = GEN.CASES[name]
    dtype = np.float64 if dt == "f64" else np.float32
    tol = 1e-7 if dt == "f64" else 1e-3     # (tests/test_leaf_pairs.py: the bars of the existing pipeline tests)
    g, k, _, _ = GEN.setup(A, hip, name)
    o, _, _, _ = GEN.setup(A, oracle, name)
    fixed_eps = n_adapts == 0
    n_checked = 0
    ends = {f: [] for f in ("n_steps", "numerical_error", "on")}
    for i in range(1, n_total + 1):
        g.set_state(o.get_state())
        for e in (g, o):
            e.run(k, i, n_adapts, i_first=i)
        g.sync()
        stg, sto = g.stats(), o.stats()
        same = np.isclose(g.theta(), o.theta(), rtol=tol, atol=tol).all(axis=0)
        for f in ("n_steps", "tree_depth", "numerical_error"):
            same &= stg[f] == sto[f]
        stable = (np.abs(sto["max_hamiltonian_energy_error"]) < 2.0) | (sto["n_steps"] <= 8)
        if fixed_eps:
            stable = np.ones(GEN.N, dtype=bool)
        on = PU.check_flips(same, PU.decision_margin(o), dtype, f"leaf octs {name} iteration {i}", sel=stable)
        n_checked += int(stable.sum())
        np.testing.assert_allclose(stg["acceptance_rate"][on], sto["acceptance_rate"][on], rtol=1e-4 if dt == "f64" else 1e-2, atol=1e-6 if dt == "f64" else 1e-4,
                                   err_msg=f"{name}: α at iteration {i}")
        np.testing.assert_allclose(g.get_stepsize()[on], o.get_stepsize()[on], rtol=1e-5 if dt == "f64" else 1e-3, err_msg=f"{name}: ϵ after iteration {i}")
        ends["n_steps"].append(sto["n_steps"].copy())
        ends["numerical_error"].append(sto["numerical_error"].copy())
        ends["on"].append(np.asarray(on).copy())
    assert n_checked >= (n_total * GEN.N) // 2, (name, n_checked)
    # the exits the case exists for, among the chain-transitions that were compared and agreed
    on = np.stack(ends["on"])
    ns = np.where(on, np.stack(ends["n_steps"]), 1)
    ne = np.where(on, np.stack(ends["numerical_error"]), 0)
    div, inside = _assert_exits(name, ns, ne)
    print(f"{name}: {n_checked} of {n_total * GEN.N} chain-transitions compared; agreed: divergent on a .. h {div}, "
          f"non-divergent ends inside a subtree at p = 2 / 4 / 6 / 0 mod 8 {inside}")
    g.close(); o.close()
