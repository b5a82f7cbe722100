"""The pair step of k_nuts (csrc/ahmc_nuts.hpp: PAIR — two leaves per step where a chain owns a wave).

a. its one reduction, wave64_pair_reduce, alone in tests/device_probe/pair_red.hip next to the primitives it replaces, on the same data:
   each energy with the bits of wave_allsum<64, T, 1>, the U-turn decision of wave64_any_le0_pair;
b. the shipped library reproduces, bit for bit, tests/golden/leaf_pair_single_loop.npz — the same chains recorded from a build with
   the single-leaf loop everywhere.  That was a build-time switch of the engine, since retired: the fixture was recorded at or before
   commit 9712c5e, and regenerating it means building that commit (tests/golden/make_leaf_pair_golden.py: the cases, and how);
c. the same configurations against the CPU oracle under the margin rule of tests/parity_util.py: the pair step is held to the
   reference, not only to its predecessor.
"""
import importlib.util
import os
import sys

import numpy as np
import pytest

import ahmc_amd as A
import parity_util as PU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "device_probe", "pair_red.hip")


def _gen():
    spec = importlib.util.spec_from_file_location("make_leaf_pair_golden", os.path.join(ROOT, "tests", "golden", "make_leaf_pair_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _gen()
CASES = sorted(GEN.CASES)
DIV_CASES = [c for c in CASES if c.startswith("div_")]


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


def _case_record(golden, name):
    return {k.split("/", 1)[1]: v for k, v in golden.items() if k.startswith(name + "/")}


def _assert_reason_for_existing(name, rec):
    """Every case is there for a kernel path; `rec` (a record of run_case, or the fixture's) must show that the case took it."""
    D, dt, max_depth, _, _, n_adapts, n_total, _ = GEN.CASES[name]
    ns, ne, dep = rec["n_steps"], rec["numerical_error"], rec["tree_depth"]
    assert ns.shape == (n_total, GEN.N), name
    assert ns.max() <= 2 ** max_depth - 1 and dep.max() <= max_depth, name
    over = GEN.handed_over(rec, name)
    if name.startswith("div_"):
        first = int(((ne != 0) & (ns % 2 == 0)).sum())               # the tree ended on the FIRST leaf of a pair
        second = int(((ne != 0) & (ns % 2 == 1) & (ns > 1)).sum())   # … on the SECOND
        assert first >= 5 and second >= 5, (name, first, second)
    elif name.endswith("_md1"):
        assert (ns == 1).all(), name                                  # a single leaf: the single-leaf arm of a pair kernel, never a pair
    elif name.endswith("_md2"):
        assert ns.max() == 3 and (ns == 3).sum() >= 100, (name, int((ns == 3).sum()))   # the first leaf and exactly ONE pair
    elif name.endswith("_far"):
        # the log-domain redo kernel of the WARM-UP (MODE 4): leaves with −ΔH > 600 in the adapting transitions, real trees there
        assert over[:n_adapts].sum() >= 5 and ns[:n_adapts][over[:n_adapts]].max() >= 3, (name, int(over[:n_adapts].sum()))
    elif name.startswith("fardraws_"):
        # the log-domain redo kernel of the DRAWS (MODE 1): no adaptation, so every handed-over transition is a draw; pairs in their trees
        assert n_adapts == 0 and over.sum() >= 5 and ns[over].max() >= 3, (name, int(over.sum()))
    else:
        assert dep.max() >= 4, (name, int(dep.max()))                 # real trees: pairs, and merges on several pending levels
        if dt == "f64":
            assert not over.any(), name                               # the linear-domain kernels alone (MODE 3, then MODE 0)
    if n_adapts:
        assert np.abs(rec["metric_head"] - 1).max() > 0.05, name      # the window end did update M⁻¹


# =====================================================================================================================
# CPU part
# =====================================================================================================================
def test_pair_probe_compiles_without_scratch_or_spills():
    """The probe compiles for gfx950 with the engine's flags and no wrapper needs scratch or spills: a wrapper that spilled would test
    the spill code, not the primitive."""
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
    for want in ("p_pair_red_f64", "p_pair_red_f32", "p_pair_red_f64_q0", "p_pair_red_f32_q3"):
        assert want in names, want
    bad = [(k["name"], k.get("private_segment_fixed_size"), k.get("vgpr_spill_count"), k.get("sgpr_spill_count")) for k in meta
           if k.get("private_segment_fixed_size") or k.get("vgpr_spill_count") or k.get("sgpr_spill_count")]
    assert not bad, bad


def test_fixture_holds_every_case_and_both_kinds_of_divergent_pair(golden):
    """The fixture itself: every case is there at its recorded length, it is far below the committed-file limit, and every case shows
    the kernel path it exists for: a divergence case at least 5 divergent transitions whose tree ended on the FIRST leaf of a pair
    (even n_steps) and at least 5 on the SECOND (odd n_steps > 1); the far cases transitions with −ΔH > 600 — handed to the log-domain
    redo kernels — in the warm-up (MODE 4) and in the draws (MODE 1); max_depth 1 single leaves only, max_depth 2 exactly one pair."""
    assert os.path.getsize(GEN.FIXTURE) < 768 * 1024
    for name in CASES:
        rec = _case_record(golden, name)
        assert rec["theta_head"].shape == (GEN.CASES[name][6], 2, GEN.N), name
        _assert_reason_for_existing(name, rec)
        over = GEN.handed_over(rec, name)
        print(f"{name}: handed to the log-domain kernel in {int(over.sum())} chain-transitions, n_steps max {int(rec['n_steps'].max())}")


# =====================================================================================================================
# GPU part
# =====================================================================================================================
def _pair_inputs(dt, n_waves, seed):
    """(n_waves, 64, 4): ea, eb, da, db per lane.  Magnitudes spread over 20 binades with both signs; every eighth wave has lanes that
    are exactly zero; waves 0 … 63 carry +Inf / −Inf / both / NaN in one or two lanes of one of the four values; a block of waves has
    dot products that cancel to exactly zero or to a rounding residue (the decision's tie)."""
    rs = np.random.default_rng(seed)
    x = rs.standard_normal((n_waves, 64, 4)) * np.exp2(rs.integers(-10, 11, size=(n_waves, 64, 4)))
    x[::8][rs.random((len(x[::8]), 64, 4)) < 0.3] = 0.0
    x = x.astype(dt)
    x[0::64, :, 2:] = 0                                   # all-zero dot products: Σ = 0 <= 0
    x[1::64, 32:, 2] = -x[1::64, :32, 2]                  # Σda cancels (exactly or to a residue), Σdb free
    x[2::64, 32:, 3] = -x[2::64, :32, 3]
    x[3::64, :, 2:] = np.abs(x[3::64, :, 2:]) + dt(1e-3)  # both sums positive: no turn
    bad = [(np.inf,), (-np.inf,), (np.inf, -np.inf), (np.nan,)]
    for w in range(64):
        k, vals = w % 4, bad[(w // 4) % 4]
        for j, v in enumerate(vals):
            x[4 + w * 8, (w * 5 + 31 * j) % 64, k] = v
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_pair_reduce_gives_the_bits_of_the_primitives_it_replaces(hip, dt):
    """a. 4 096 waves: wave64_pair_reduce returns Σea and Σeb with the bits of wave_allsum<64, T, 1> in every lane, and the decision
    wave64_any_le0_pair takes on the same dot products.  The quad the engine reads the energies from (AHMC_PAIR_RED_QUAD) is checked,
    and so is the reason for it: of the four quads exactly two give the butterfly's bits on all inputs — which two is the direction
    row_ror rotates in."""
    import torch

    from ahmc_amd import build as B
    from ahmc_amd.hipmod import Module

    torch.cuda.init()
    mod = Module(B.build_probe_object(PROBE))
    tn = "f64" if dt == np.float64 else "f32"
    n_waves = 4096
    x = _pair_inputs(dt, n_waves, seed=11)
    n = n_waves * 64
    xin = torch.from_numpy(np.ascontiguousarray(x.reshape(-1))).cuda()

    def run(name):
        o = torch.full((n * 6,), float("nan"), dtype=torch.float64 if dt == np.float64 else torch.float32, device="cuda")
        mod.launch(name, n // 256, 256, xin, o, np.int64(n))
        torch.cuda.synchronize()
        return o.cpu().numpy().reshape(n_waves, 64, 6)

    y = run(f"p_pair_red_{tn}")
    assert (_bits(y[:, :, :3]) == _bits(y[:, :1, :3])).all(), "the reference primitives: lanes of a wave differ"
    assert np.isin(y[:, :, 2], (0, 1)).all() and np.isin(y[:, :, 5], (0, 1)).all()
    turn = y[:, 0, 2]
    assert 0.2 < turn.mean() < 0.95 and np.isnan(y[:, 0, :2]).any() and np.isinf(y[:, 0, :2]).any()   # the inputs exercise both outcomes
    good = []
    for q in range(4):
        yq = run(f"p_pair_red_{tn}_q{q}")
        assert (yq[:, :, 5] == yq[:, :, 2]).all(), q      # the decision never depends on the quad
        good.append(bool(_same_bits(yq[:, :, 3], yq[:, :, 0]).all() and _same_bits(yq[:, :, 4], yq[:, :, 1]).all()))
    print(f"{tn}: quads whose lanes 2 / 3 hold the butterfly's bits: {[q for q in range(4) if good[q]]}")
    assert _same_bits(y[:, :, 3], y[:, :, 0]).all(), "Σea differs from wave_allsum<64, T, 1>"
    assert _same_bits(y[:, :, 4], y[:, :, 1]).all(), "Σeb differs from wave_allsum<64, T, 1>"
    assert (y[:, :, 5] == y[:, :, 2]).all(), "the U-turn decision differs from wave64_any_le0_pair"
    assert good in ([True, False, True, False], [False, True, False, True]), good


def _compare(name, rec, golden, what):
    for f in GEN.PER_TRANSITION + ("theta_sum", "theta_head"):
        a, b = rec[f], golden[f"{name}/{f}"]
        assert a.dtype == b.dtype and a.shape == b.shape, (name, f, a.dtype, b.dtype)
        same = _same_bits(a, b) if a.dtype.kind == "f" else (a == b)
        if not same.all():
            it = int(np.argwhere(~same.reshape(same.shape[0], -1).all(axis=1))[0, 0])
            raise AssertionError(f"{name} ({what}): {f} differs from the single-leaf loop's first at transition {it + 1} "
                                 f"(chains {np.flatnonzero(~same[it].reshape(-1, GEN.N).all(axis=0) if same[it].ndim > 1 else ~same[it])[:8].tolist()})")
    assert (rec["metric_sum"] == golden[f"{name}/metric_sum"]).all() and _same_bits(rec["metric_head"], golden[f"{name}/metric_head"]).all(), (name, what, "M⁻¹")


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_same_chains_as_the_single_leaf_loop(hip, golden, name):
    """b. every recorded transition of the case, one iteration per call (the fused warm-up kernel, then the sampling kernel), bit for
    bit; then the whole run again in ONE call (launches of many transitions): the same draws, final state and M⁻¹."""
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
def test_pair_step_against_oracle(hip, oracle, name):
    """c. the same configurations against the CPU oracle, one iteration at a time from the oracle's complete state (dual averaging
    doubles a last-bit difference per iteration, so a free-running comparison means nothing): a chain may leave the oracle's track —
    n_steps, tree depth, divergence flag, position — only where the oracle took a decision within the margin bound of a tie
    (tests/parity_util.py).  As in tests/test_pipeline_parity.py the bar applies to the transitions that were numerically stable on
    the oracle (|ΔH|_max < 2) or short (<= 8 leapfrogs); the divergence cases (Δ_max = 0.5) are stable throughout."""
    D, dt, max_depth, delta_max, _, n_adapts, n_total, off = GEN.CASES[name]
    dtype = np.float64 if dt == "f64" else np.float32
    # θ of a transition that took the same decisions: the two sides differ by rounding alone — up to 1 023 leapfrogs of ≈ 10 roundings
    # each on values of O(1 … 10): 1e4·u ≈ 1e-12 (f64), 6e-4 (f32) if they add up linearly; the bars are 1e-7 (the existing pipeline
    # tests') and 1e-3
    tol = 1e-7 if dt == "f64" else 1e-3
    g, k, _, _ = GEN.setup(A, hip, name)
    o, _, _, _ = GEN.setup(A, oracle, name)
    fixed_eps = n_adapts == 0
    n_checked = n_div_first = n_div_second = n_over = n_over_checked = 0
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
            # no adaptation: ϵ stays at its fixed value, far inside the leapfrog's stability bound (ϵ < 2 for the unit Gaussian), so a
            # trajectory amplifies no rounding however large its energy error — the −ΔH ≈ 1 340 of the far start is the integrator's
            # conserved H − ϵ²|θ|²/8, not an instability.  Every chain is held to the bar, the handed-over ones included.
            stable = np.ones(GEN.N, dtype=bool)
        on = PU.check_flips(same, PU.decision_margin(o), dtype, f"leaf pairs {name} iteration {i}", sel=stable)
        n_checked += int(stable.sum())
        np.testing.assert_allclose(stg["acceptance_rate"][on], sto["acceptance_rate"][on], rtol=1e-4 if dt == "f64" else 1e-2, atol=1e-6 if dt == "f64" else 1e-4,
                                   err_msg=f"{name}: α at iteration {i}")
        np.testing.assert_allclose(g.get_stepsize()[on], o.get_stepsize()[on], rtol=1e-5 if dt == "f64" else 1e-3, err_msg=f"{name}: ϵ after iteration {i}")
        over = sto["max_hamiltonian_energy_error"] < -GEN.LINW_LIMIT    # by the oracle: the chain needs the log-domain kernel (MODE 1 / 4)
        n_over += int(over.sum())
        n_over_checked += int((over & on & (sto["n_steps"] >= 3)).sum())
        div = on & (sto["numerical_error"] != 0)
        n_div_first += int((div & (sto["n_steps"] % 2 == 0)).sum())
        n_div_second += int((div & (sto["n_steps"] % 2 == 1) & (sto["n_steps"] > 1)).sum())
    print(f"{name}: {n_checked} of {n_total * GEN.N} chain-transitions compared, divergent on a first leaf {n_div_first}, on a second {n_div_second}")
    assert n_checked >= (n_total * GEN.N) // 2, (name, n_checked)
    if name.startswith("div_"):
        assert n_div_first >= 5 and n_div_second >= 5, (name, n_div_first, n_div_second)
    print(f"{name}: handed to the log-domain kernel {n_over}, of them compared with pairs in their trees {n_over_checked}")
    if name.startswith("fardraws_"):
        assert n_over_checked >= 5, (name, n_over, n_over_checked)    # MODE 1 itself is held to the oracle
    if name.endswith("_far"):
        # (MODE 4: those transitions run at the ϵ ≈ 1.4 dual averaging has just jumped to, −ΔH ≈ 3e4: they took the path, and the
        # chains among them that pass the stability filter are compared; the bit-for-bit fixture holds all of them)
        assert n_over >= 5, (name, n_over)
    g.close(); o.close()
