"""Every compiled thread geometry (G lanes per chain, E elements per lane) × log-density family × element type against the oracle.

csrc/ahmc_inst.hpp: AHMC_GEOMETRIES lists 19 geometries; csrc/ahmc_api.hip: pick_geometry selects 11 of them by D, the other eight
are reachable through AHMC_GEOMETRY=G,E only ("thread geometry").  Each (G, E, family, type) is its own machine code,
and the geometry-dependent code of target_eval (csrc/ahmc_device.hpp) sits in the funnel and the hierarchical Gaussian: the
broadcast of θ[0] (and of log τ, from lane 1 when E = 1), the one-barrier exchanges of the multi-wave chains, the `d < D` masks.

  1. host tests: the tables of this file equal AHMC_GEOMETRIES and pick_geometry (parsed from the sources), and the (G, E) that
     tests/test_buffer_bounds.py and tests/test_exact_invariance.py expect for their D equal the default table;
  2. the matrix: 19 geometries × 4 families × {Float64, Float32}, each at D_full = G·E and D_ragged = max(3, G·E/2 − 1) (the upper
     half of the lanes — for G > 64 of the workgroup's waves — idle, the last used lane partly filled when E >= 2), under the
     override in EVERY cell (D_ragged lies below a default geometry's own range), with the body of
     tests/test_gpu_parity.py: test_multiwave_chains and its bars;
  3. the fused launch shapes (warm-up / draws / general kernel) of the eight non-default geometries, bit for bit against the
     per-iteration path (tests/test_instantiations.py: bulk_equals_stepwise);
  4. what the override refuses.

The margin filter of tests/parity_util.py may excuse a chain one of whose decisions the oracle took within PU.bound(dtype) of a
tie; MIN_CLEAR keeps it from hiding a failure: in every compared transition at least three quarters of the chains must have had NO
such decision.  The condition depends on the oracle alone.

ADJUSTED CELLS.  The recipe is test_multiwave_chains' (diag_chain metric, ϵ = 0.3·D^-1/4, funnel 0.2·D^-1/4, θ₀ = 0.5·normal, NUTS depths
5 / 4 / 4); that test is Float64 only.  Every figure below is the oracle's alone (a dry run on the CPU gives it):
  * hier, D > 1000, both types: ϵ halved (HIER_WIDE_EPS_SCALE).  At 0.3·D^-1/4 every tree of the cells at D = 1024 … 4096 ended below
    depth 2 (the log τ coordinate, whose force grows like D, diverges in the first doubling): nothing of the tree code would run.
  * Float32, funnel and hier: ϵ = min(recipe, 0.35·D^-1/2) resp. min(recipe, 0.25·D^-1/2) (F32_NECK_EPS).  The frequency of the neck
    coordinate grows like √D, and at the recipe's ϵ the oracle's OWN Float32 and Float64 leapfrogs differ by up to 1.8e6 times the
    Float32 tolerance after step(7), step(−4) (hier, D = 1023; 138 times at D = 3, (8,1)): no implementation can meet RTOL there.
    With the cap the worst cell stands at 0.077 of the tolerance; every Float32 cell asserts <= F32_MAX_CONDITIONING = 0.25 on the
    oracle before it holds the HIP engine to the tolerance.  Float64 runs the recipe's ϵ.
  * Float32, the three-quarters condition, decided per (transition kind, D) over all cells of that D.  The scale of the weight
    comparisons is |H0| ≈ 1.5·D (the −D/2·log 2π of ℓπ alone is 0.92·D), so 1e-4 of it is 0.02 in ℓw at D = 127 and 0.6 at D = 4096.
    max_depth (F32_NUTS_DEPTHS) is the largest value, not above the recipe's, at which every cell of that D has >= 0.75 of its chains
    clear; smallest share over the cells at depth 5 / 4 / 3 / 2:
        Multinomial/Generalised   D = 63, 64: 0.56 / 0.76 / · / ·    127, 128: 0.32 / 0.68 / 0.88 / ·    255, 256: 0.04 / 0.44 / 0.68 / 0.88
                                  511, 512: 0 / 0.16 / 0.40 / 0.76   1023, 1024: 0 / 0 / 0.16 / 0.56     2047 …: <= 0.24 at depth 2
        Multinomial/Classic       63, 64: 0.56 / 0.80                127, 128: 0.40 / 0.72 / 0.80        255, 256: 0.24 / 0.48 / 0.68 / 0.80
                                  511, 512: 0.08 / 0.28 / 0.52 / 0.72                                     1023 …: <= 0.56 at depth 2
        Slice/Strict              >= 0.84 at depth 4 up to D = 512; 0.72 at every depth at 1023 / 1024, 0.64 at 2047 / 2048, 0.28 at 4096
    so Float32 runs 5 / 4 / 4 up to D = 32, 4 / 4 / 4 up to 64, 3 / 4 / 3 up to 128 and 2 / 4 / 2 above; every tree still reaches depth 2.
    MIN_CLEAR is asserted on every transition of every kind EXCEPT (F32_WAIVED_FROM) where no max_depth >= 2 meets it in every cell:
        static Multinomial  from D = 127 (seven comparisons of its index scan, |cum − u| / |H0| with cum, u in [0, 1]; L = 6 as given, it
                            has no depth: 0.68 at D = 127 / 128, 0.32 at 255, 0.04 at 511, none from 1023 on)
        static EndPoint     from D = 511 (one MH comparison: 0.80 at 255 / 256, 0.68 at 511, 0.52 at 4096)
        Multinomial/Classic from D = 511, Multinomial/Generalised and Slice/Strict from D = 1023 (figures above)
    The waived transitions still run, the multinomial NUTS kinds at depth 2 where most chains stay clear (>= 0.56 at D = 1023 / 1024):
    check_flips and its caps hold every chain's discrete statistics (a flip must be excused by a margin that few chains could
    claim), the continuous ones are compared on the clear chains, and the Float64 twin of each cell — same template, same inputs,
    the recipe's depths — has 0.96 at the least.  Smallest share where the condition is asserted in Float32: 0.76.

MUTATION CHECK (a scratch build of the funnel and hier units, MI355X; the three defects at once — the cells they can reach are disjoint):
  * E = 1 hier broadcast of log τ from lane 0 instead of lane 1: caught by all 20 hier cells of (4,1), (8,1), (16,1), (32,1), (64,1)
    — D_full and D_ragged, both types — and by no other.
  * xwave_buf_s summed over one wave too few in group_allsum_once: caught by the 12 D_full hier cells of the six multi-wave
    geometries, both types; NOT by their D_ragged cells, where the dropped wave is idle — which is why both D are in the matrix.
  * the `d < D` mask of the funnel's gradient dropped: caught by no cell, and no D closes it: a padded element holds θ = 0 in every
    kernel, so the unmasked value θ·e^{−y} is 0 too unless e^{−y} overflows (y < −709, Float32 −88) — a state the oracle rejects as
    non-finite as well.  The mask is redundant for finite e^{−y}; the iso family relies on the same invariant without a mask.
  Every one of the 32 catches is the first comparison of its cell, the gradient after refresh().

TIME (MI355X machine, pytest --durations=0, same figures within 0.01 s in three runs): slowest case here 0.20 s ((512,8) D = 4096 diag Float64; the matrix is
parametrised by D as well as by family because a case over both D of one family took 0.28 s); slowest case of
tests/test_gpu_parity.py::test_multiwave_chains at the parent commit's kernels 0.21 s (400-iso, the module's first launches) and
0.20 s (3000-diag).  Slowest fused-launch case 0.15 s.
"""
import os
import re

import numpy as np
import pytest

import ahmc_amd as A
import parity_util as PU
from parity_util import ALL_GEOMETRIES, DEFAULT_GEOMETRIES
from test_gpu_parity import ATOL, RTOL, assert_points_close, compare_transition_stats, make_metric, make_target, pair, realign
from test_instantiations import bulk_equals_stepwise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "advancedhmc.jl_amd", "csrc")

# ALL_GEOMETRIES (19) and DEFAULT_GEOMETRIES (11, each with its D range) live in tests/parity_util.py: tests/test_instantiations.py
# reads the default table too, and this module imports that one's helper
NON_DEFAULT = [(8, 1), (16, 1), (32, 1), (64, 1), (32, 4), (128, 4), (256, 4), (512, 4)]
FAMILIES = ["iso", "diag", "funnel", "hier"]
MIN_CLEAR = 0.75
KINDS = ("hmc-ep", "hmc-mn", "nuts-mn-gen", "nuts-sl-str", "nuts-mn-cls")
# Float32 (ADJUSTED CELLS, module docstring): max_depth of the three NUTS kinds for D up to the first column …
F32_NUTS_DEPTHS = [(32, (5, 4, 4)), (64, (4, 4, 4)), (128, (3, 4, 3)), (4096, (2, 4, 2))]
# … and the smallest D from which a kind cannot have three quarters of its chains clear at any max_depth >= 2
F32_WAIVED_FROM = {"hmc-ep": 511, "hmc-mn": 127, "nuts-mn-gen": 1023, "nuts-sl-str": 1023, "nuts-mn-cls": 511}
HIER_WIDE_EPS_SCALE = 0.5
F32_NECK_EPS = {"funnel": 0.35, "hier": 0.25}
F32_MAX_CONDITIONING = 0.25


def default_geometry(D):
    for lo, hi, G, E in DEFAULT_GEOMETRIES:
        if lo <= D <= hi:
            return G, E
    raise KeyError(D)


def d_full(G, E):
    return G * E


def d_ragged(G, E):
    return max(3, G * E // 2 - 1)


def n_chains(G):
    """odd: the last wave (G <= 64: 64/G chains per wave, 256/G per workgroup) and the last workgroup are ragged"""
    return max(25, 2 * (256 // G) + 64 // G + 1) if G <= 64 else 25


# ------------------------------------------------------------------------------------------------------------------------------
# 1. host: the tables cannot drift
# ------------------------------------------------------------------------------------------------------------------------------
def parse_compiled_geometries(text):
    """the X(G, E) list of the built-in AHMC_GEOMETRIES (the other definition is a plugin's single geometry)"""
    defs = re.findall(r"#define AHMC_GEOMETRIES\(X\)((?:[^\n]*\\\n)*[^\n]*)", text)
    body = [d for d in defs if "AHMC_GEOMETRIES_EXTRA" in d]
    assert len(defs) == 2 and len(body) == 1, defs
    assert re.search(r"#define AHMC_GEOMETRIES_EXTRA\(X\)[ \t]*(//[^\n]*)?\n", text), "the shipped build adds no extra geometry"
    return [(int(g), int(e)) for g, e in re.findall(r"X\((\d+), *(\d+)\)", body[0])]


def parse_default_table(text):
    """pick_geometry's `D <= hi → (G, E)` chain as (lo, hi, G, E) rows"""
    fn = re.search(r"inline bool pick_geometry\(int64_t D, int& G, int& E\) \{(.*?)else return false;", text, re.S)
    assert fn, "pick_geometry not found"
    rows, lo = [], 1
    # every branch of the chain, whatever it assigns: a branch of another shape must not slip through the pattern below
    n_branches = len(re.findall(r"\bif \(D <= ", fn.group(1)))
    for hi, g, e in re.findall(r"if \(D <= (\d+)\) \{ G = (\d+); E = (\d+); \}", fn.group(1)):
        rows.append((lo, int(hi), int(g), int(e)))
        lo = int(hi) + 1
    assert len(rows) == n_branches, (len(rows), n_branches)
    return rows


def _read(name):
    with open(os.path.join(CSRC, name), encoding="utf-8") as f:
        return f.read()


def test_tables_equal_the_sources():
    compiled = parse_compiled_geometries(_read("ahmc_inst.hpp"))
    assert compiled == ALL_GEOMETRIES and len(set(ALL_GEOMETRIES)) == 19
    table = parse_default_table(_read("ahmc_api.hip"))
    assert table == DEFAULT_GEOMETRIES and len(DEFAULT_GEOMETRIES) == 11
    defaults = [(G, E) for _, _, G, E in DEFAULT_GEOMETRIES]
    assert set(defaults) <= set(ALL_GEOMETRIES) and len(set(defaults)) == 11
    assert sorted(NON_DEFAULT) == sorted(set(ALL_GEOMETRIES) - set(defaults)) and len(NON_DEFAULT) == 8
    for lo, hi, G, E in DEFAULT_GEOMETRIES:      # a default geometry covers its range, and the ranges tile 1 … 4096
        assert lo <= hi <= G * E
    assert DEFAULT_GEOMETRIES[0][0] == 1 and DEFAULT_GEOMETRIES[-1][1] == 4096
    # the override accepts exactly the compiled list (the same macro) and only a geometry that covers D
    api = _read("ahmc_api.hip")
    assert re.search(r'getenv\("AHMC_GEOMETRY"\)', api) and "AHMC_GEOMETRIES(AHMC_GEO_OK)" in api
    assert re.search(r'sscanf\(ov, "%d,%d", &g, &e\) == 2 && \(int64_t\)g \* e >= D', api)


def test_parsers_notice_an_edit():
    """a geometry edited into or out of the build, or a moved threshold, changes what the parsers return"""
    inst, api = _read("ahmc_inst.hpp"), _read("ahmc_api.hip")
    assert parse_compiled_geometries(inst.replace("X(32, 4) ", "")) == [g for g in ALL_GEOMETRIES if g != (32, 4)]
    assert parse_compiled_geometries(inst.replace("X(512, 8)", "X(512, 8) X(8, 4)")) == ALL_GEOMETRIES + [(8, 4)]
    moved = parse_default_table(api.replace("D <= 256) { G = 64; E = 4; }", "D <= 192) { G = 32; E = 4; }"))
    assert moved != DEFAULT_GEOMETRIES and moved[6] == (129, 192, 32, 4) and moved[7][0] == 193
    with pytest.raises(AssertionError):
        parse_default_table(api.replace("D <= 256) { G = 64; E = 4; }", "D <= 256) { G = 64; E = pick_e(D); }"))


def test_other_files_expect_the_default_table():
    import test_buffer_bounds as BB
    import test_exact_invariance as EI
    import test_gpu_parity as GP

    assert sorted(BB.GEOM) == sorted(GP.GEOM_D)
    for D, ge in BB.GEOM.items():
        assert ge == default_geometry(D), (D, ge)
    seen = 0
    for cfg in EI.GEOMETRIES + EI.BATCHED:
        exp = {k: v for k, op, v in cfg.expect if op == "=="}
        if "group_lanes" in exp:
            assert (exp["group_lanes"], exp["elems_per_lane"]) == default_geometry(cfg.D), cfg.name
            seen += 1
    assert seen >= len(EI.GEOMETRIES) >= 6
    # the Ds those two files and GEOM_D name reach every default geometry between them
    reached = {default_geometry(D) for D in list(BB.GEOM) + [c.D for c in EI.GEOMETRIES]}
    assert reached == {(G, E) for _, _, G, E in DEFAULT_GEOMETRIES}


def test_matrix_shapes():
    """D_full, D_ragged and N as the cases use them: covered by the geometry, the upper half idle, ragged chain count"""
    for G, E in ALL_GEOMETRIES:
        Df, Dr, N = d_full(G, E), d_ragged(G, E), n_chains(G)
        assert 3 <= Dr <= Df == G * E <= 4096 and N % 2 == 1 and N >= 25
        if G * E >= 8:
            assert Dr < G * E // 2                      # lanes G/2 … G−1 hold padding only
            assert E == 1 or Dr % E != 0                # the last used lane is partly filled
        if G > 64:
            assert (Dr + E - 1) // E <= G // 2 and G // 2 >= 64   # waves G/128 … G/64−1 idle
        else:
            assert N % (64 // G) != 0 or G == 64        # a partly filled last wave
            assert N > 256 // G                         # more than one workgroup
    assert (d_ragged(128, 8), d_ragged(512, 4), d_ragged(4, 1), d_ragged(16, 1)) == (511, 1023, 3, 7)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the matrix
# ------------------------------------------------------------------------------------------------------------------------------
def nuts_depths(dtype, D):
    """max_depth of (Multinomial/Generalised, Slice/Strict, Multinomial/Classic); see ADJUSTED CELLS in the module docstring"""
    if dtype == np.float32:
        return next(depths for hi, depths in F32_NUTS_DEPTHS if D <= hi)
    return (5, 4, 4)


def cell_eps(family, D, dtype):
    eps = (0.2 if family == "funnel" else 0.3) * D ** -0.25
    if family == "hier" and D > 1000:
        eps *= HIER_WIDE_EPS_SCALE
    if dtype == np.float32 and family in F32_NECK_EPS:
        eps = min(eps, F32_NECK_EPS[family] * D ** -0.5)
    return eps


def conditioning(za, zb, dtype):
    """the largest |a − b| / (atol + rtol·|b|) over what assert_points_close compares: 1 is its bar"""
    rt, at = RTOL[dtype], ATOL[dtype]
    worst = 0.0
    for a, b, k in ((za.theta, zb.theta, 1), (za.r, zb.r, 1), (za.lp.gradient, zb.lp.gradient, 1), (za.lp.value, zb.lp.value, 10),
                    (za.lk.value, zb.lk.value, 10)):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        worst = max(worst, float(np.max(np.abs(a - b) / (at * k + rt * np.abs(b)))))
    return worst


def min_clear(dtype, D, kind):
    """the share of chains that must be clear of a tie in every compared transition of this kind; None: not attainable (module docstring)"""
    if dtype == np.float32 and D >= F32_WAIVED_FROM.get(kind, 1 << 30):
        return None
    return MIN_CLEAR


def assert_geometry(hip, e, G, E):
    if hip.backend == "hip:gfx950":   # (a dry run on the oracle still walks the Python)
        assert (e.info("group_lanes"), e.info("elems_per_lane")) == (G, E), (G, E)


def run_cell(hip, oracle, G, E, D, family, dtype):
    """one (G, E, D, family, type) cell: refresh, leapfrog, ten transitions of five kinds, find_good_stepsize.  The caller has set
    AHMC_GEOMETRY."""
    rng = np.random.default_rng([G, E, D, FAMILIES.index(family)])
    N = n_chains(G)
    what = f"({G},{E}) D={D} {family} {np.dtype(dtype).name}"
    h = A.Hamiltonian(make_metric("diag_chain", D, N, rng), make_target(family, D, rng))
    lf = A.Leapfrog(np.full(N, cell_eps(family, D, dtype)))
    g, o = pair(hip, oracle, h, N, dtype, seed=3, lf=lf)
    o64 = None
    try:
        assert_geometry(hip, g, G, E)
        th, r = 0.5 * rng.normal(size=(D, N)), rng.normal(size=(D, N))
        for e in (g, o):
            e.set_position(th)
            e.refresh()
        assert_points_close(g.phasepoint(), o.phasepoint(), dtype, what + " refresh")
        for e in (g, o):      # no decision is taken here: every chain is compared
            e.set_position(th, r)
        assert_points_close(g.phasepoint(), o.phasepoint(), dtype, what + " phasepoint")
        if dtype == np.float32:   # the oracle in Float64 on the same inputs: how far rounding alone moves these trajectories
            o64 = A.Engine(h, N, dtype=np.float64, rng=3, lib=oracle)
            o64.set_integrator(lf)
            o64.set_position(th, r)
        for n in (7, -4):
            for e in (g, o):
                e.step(n)
            if o64 is not None:
                o64.step(n)
                c = conditioning(o.phasepoint(), o64.phasepoint(), dtype)
                assert c <= F32_MAX_CONDITIONING, f"{what} step({n}): the oracle's own Float32 and Float64 differ by {c:.3g} of the tolerance"
            assert_points_close(g.phasepoint(), o.phasepoint(), dtype, what + f" step({n})")
        for e in (g, o):
            e.set_position(th)
        dg, ds, dc = nuts_depths(dtype, D)
        kernels = [   # (names: KINDS)
            ("hmc-ep", A.HMCKernel(A.Trajectory(A.EndPointTS, lf, A.FixedNSteps(6)))),
            ("hmc-mn", A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.FixedNSteps(6)))),
            ("nuts-mn-gen", A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=dg)))),
            ("nuts-sl-str", A.HMCKernel(A.Trajectory(A.SliceTS, lf, A.StrictGeneralisedNoUTurn(max_depth=ds)))),
            ("nuts-mn-cls", A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.ClassicNoUTurn(max_depth=dc)))),
        ]
        PU.reset_margin(o)
        for name, k in kernels:
            for it in range(2):
                w = f"{what} {name} #{it}"
                g.transition(k)
                o.transition(k)
                sg, so = g.stats(), o.stats()
                clear = float((PU.decision_margin(o, reset=False) >= PU.bound(dtype)).mean())
                need = min_clear(dtype, D, name)
                assert need is None or clear >= need, f"{w}: only {clear:.2f} of the chains took every decision clear of a tie"
                same = compare_transition_stats(sg, so, dtype, o, w)
                if name.startswith("nuts"):
                    assert sg["tree_depth"].max() >= 2 and so["tree_depth"].max() >= 2, w   # the trees are not trivial
                if dtype == np.float64:
                    zg, zo = g.phasepoint(), o.phasepoint()
                    np.testing.assert_allclose(zg.theta[:, same], zo.theta[:, same], rtol=1e-8, atol=1e-8, err_msg=w)
                realign(g, o, same)
            for e in (g, o):  # re-synchronise the two engines for the next kernel
                e.set_position(o.phasepoint().theta)
        PU.reset_margin(o)
        eg, eo = g.find_good_stepsize(), o.find_good_stepsize()
        PU.check_equal_or_near_tie(eg, eo, PU.decision_margin(o), dtype, what + " find_good_stepsize")
        assert_geometry(hip, g, G, E)
    finally:
        for e in (g, o, o64):
            if e is not None:
                e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", [d_full, d_ragged], ids=["full", "ragged"])
@pytest.mark.parametrize("G,E", ALL_GEOMETRIES)
def test_geometry_family_type_against_oracle(hip, oracle, monkeypatch, G, E, shape, family, dtype):
    monkeypatch.setenv("AHMC_GEOMETRY", f"{G},{E}")
    run_cell(hip, oracle, G, E, shape(G, E), family, dtype)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the fused launch shapes of the non-default geometries
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("tname", FAMILIES)
@pytest.mark.parametrize("G,E", NON_DEFAULT)
def test_non_default_instantiation_bulk_equals_stepwise(hip, monkeypatch, G, E, tname, dtype):
    monkeypatch.setenv("AHMC_GEOMETRY", f"{G},{E}")
    rng = np.random.default_rng(5)
    for D in (d_full(G, E), d_ragged(G, E)):
        assert default_geometry(D) != (G, E)
        geoms = bulk_equals_stepwise(hip, tname, dtype, D, rng, override=(G, E))
        if hip.backend == "hip:gfx950":
            assert geoms == {(G, E)}, geoms


# ------------------------------------------------------------------------------------------------------------------------------
# 4. what the override refuses
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_override_refusals(hip, monkeypatch):
    D, N = 10, 8
    assert default_geometry(D) == (8, 2)
    h = A.Hamiltonian(A.UnitEuclideanMetric((D, N)), A.HierGaussian(D))

    def geometry():
        e = A.Engine(h, N, rng=1, lib=hip)
        try:
            e.set_position(np.zeros((D, N)))      # the engine works, whatever the variable said
            assert np.isfinite(e.phasepoint().lp.value).all()
            return e.info("group_lanes"), e.info("elems_per_lane")
        finally:
            e.close()

    on_hip = hip.backend == "hip:gfx950"
    monkeypatch.delenv("AHMC_GEOMETRY", raising=False)
    assert not on_hip or geometry() == (8, 2)
    for refused in ("7,3",      # not compiled
                    "8,4",      # covers D, not compiled either (a variant build's AHMC_GEOMETRIES_EXTRA)
                    "4,1",      # compiled, does not cover D = 10
                    "8,1",      # compiled, 8 < 10
                    "16x2", "16", "", "G,E", ",2"):   # malformed
        monkeypatch.setenv("AHMC_GEOMETRY", refused)
        got = geometry()
        assert not on_hip or got == (8, 2), (refused, got)
    for taken in ((16, 1), (16, 2), (64, 8)):    # … and a compiled geometry that covers D is taken
        monkeypatch.setenv("AHMC_GEOMETRY", "%d,%d" % taken)
        got = geometry()
        assert not on_hip or got == taken, (taken, got)
    monkeypatch.delenv("AHMC_GEOMETRY")
    assert not on_hip or geometry() == (8, 2)
