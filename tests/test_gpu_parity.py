"""GPU parity: HIP engine (through the C ABI) vs the CPU oracle on identical seeded inputs.

Tolerances (north_star: "within a stated fp tolerance"):
  Float64: 1e-9 relative on energies/positions after a transition (the two sides differ only by
           FMA contraction and libm-vs-ocml last-ulp differences in log/exp/sincos).
  Float32: 2e-3 relative on single leapfrog trajectories, plus moment checks.
  Discrete statistics (n_steps, tree_depth, is_accept, numerical_error), both types, since round 6: EXACT on every chain —
           except a chain one of whose decisions the oracle itself took within 1e-9 (f64) / 1e-4 (f32) RELATIVE of a tie
           (tests/parity_util.py: the oracle reports the margin of every U-turn, sampling, divergence and MH comparison).
           Rounds 1–5 accepted "≥ 99.9 % / 97 % / 90 % of the chains agree"; those thresholds are gone.
"""
import numpy as np
import pytest

import ahmc_amd as A
import parity_util as PU

pytestmark = pytest.mark.gpu

KATOL = 2.5  # test/sampler-vec.jl:43: RNDATOL * n_chains with RNDATOL = 0.5, n_chains = 5
RTOL = {np.float64: 1e-9, np.float32: 2e-3}
ATOL = {np.float64: 1e-9, np.float32: 2e-3}


def make_target(name, D, rng):
    if name == "iso":
        return A.IsoGaussian(D)
    if name == "diag":
        return A.DiagGaussian(rng.normal(size=D), 0.5 + rng.random(D))
    if name == "funnel":
        return A.Funnel(D)
    if name == "hier":
        return A.HierGaussian(D)
    raise KeyError(name)


def make_metric(name, D, N, rng):
    if name == "unit":
        return A.UnitEuclideanMetric((D, N))
    if name == "diag_shared":
        return A.DiagEuclideanMetric(0.5 + rng.random(D))
    return A.DiagEuclideanMetric(np.asfortranarray(0.5 + rng.random((D, N))))


def pair(hip, oracle, h, N, dtype, seed=7, eps=None, lf=None):
    engines = []
    for lib in (hip, oracle):
        e = A.Engine(h, N, dtype=dtype, rng=seed, lib=lib)
        if lf is not None:
            e.set_integrator(lf)
        elif eps is not None:
            e.set_integrator(A.Leapfrog(eps))
        engines.append(e)
    return engines


def assert_points_close(zg, zo, dtype, what=""):
    rt, at = RTOL[dtype], ATOL[dtype]
    np.testing.assert_allclose(zg.theta, zo.theta, rtol=rt, atol=at, err_msg=what + " theta")
    np.testing.assert_allclose(zg.r, zo.r, rtol=rt, atol=at, err_msg=what + " r")
    np.testing.assert_allclose(zg.lp.gradient, zo.lp.gradient, rtol=rt, atol=at, err_msg=what + " grad")
    np.testing.assert_allclose(zg.lp.value, zo.lp.value, rtol=rt, atol=at * 10, err_msg=what + " lp")
    np.testing.assert_allclose(zg.lk.value, zo.lk.value, rtol=rt, atol=at * 10, err_msg=what + " lk")


GEOM_D = [3, 5, 10, 24, 32, 50, 100, 128, 200, 300, 600, 1500, 2048, 4096]  # every default thread geometry (G,E),
# incl. the multi-wave chains (D > 512: one chain per workgroup of 2/4/8 waves; BASELINE configs[4] is D = 2048)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D", GEOM_D)
def test_phasepoint_and_leapfrog_all_geometries(hip, oracle, rng, dtype, D):
    """phasepoint(h, θ, r) and step(lf, h, z, n) (src/hamiltonian.jl:115-119, src/integrator.jl:216-265)"""
    N = 37
    h = A.Hamiltonian(make_metric("diag_chain", D, N, rng), A.IsoGaussian(D))
    g, o = pair(hip, oracle, h, N, dtype, eps=0.05 + 0.1 * rng.random(N))
    th, r = rng.normal(size=(D, N)), rng.normal(size=(D, N))
    for e in (g, o):
        e.set_position(th, r)
    assert_points_close(g.phasepoint(), o.phasepoint(), dtype, "phasepoint")
    for n in (7, -4):
        for e in (g, o):
            e.step(n)
        assert_points_close(g.phasepoint(), o.phasepoint(), dtype, f"step({n})")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("target", ["iso", "diag", "funnel", "hier"])
@pytest.mark.parametrize("metric", ["unit", "diag_shared", "diag_chain"])
def test_targets_and_metrics(hip, oracle, rng, dtype, target, metric):
    """∂H∂θ for every built-in family, ∂H∂r / neg_energy for Unit and Diag (src/hamiltonian.jl:45-68,155-177)"""
    D, N = 10, 64
    h = A.Hamiltonian(make_metric(metric, D, N, rng), make_target(target, D, rng))
    g, o = pair(hip, oracle, h, N, dtype, eps=0.02)
    th, r = 0.5 * rng.normal(size=(D, N)), rng.normal(size=(D, N))
    for e in (g, o):
        e.set_position(th, r)
        e.step(5)
    assert_points_close(g.phasepoint(), o.phasepoint(), dtype, f"{target}/{metric}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_step_loop_equals_step_n(hip, dtype, rng):
    """test/integrator.jl:17-32: step looped 10x == step(.., 10) (DETATOL 5e-3; here exact)"""
    D, N = 5, 16
    h = A.Hamiltonian(A.UnitEuclideanMetric((D, N)), A.IsoGaussian(D))
    a = A.Engine(h, N, dtype=dtype, lib=hip)
    b = A.Engine(h, N, dtype=dtype, lib=hip)
    th, r = rng.normal(size=(D, N)), rng.normal(size=(D, N))
    for e in (a, b):
        e.set_integrator(A.Leapfrog(0.1))
        e.set_position(th, r)
    for _ in range(10):
        a.step(1)
    b.step(10)
    za, zb = a.phasepoint(), b.phasepoint()
    np.testing.assert_array_equal(za.theta, zb.theta)
    np.testing.assert_array_equal(za.r, zb.r)


def test_harmonic_oscillator(hip):
    """test/integrator.jl:108-153: 1-D harmonic oscillator, ϵ=0.01, radius and H within 2e-3 of their mean"""
    h = A.Hamiltonian(A.UnitEuclideanMetric((1, 4)), A.DiagGaussian([0.0], [1.0]))
    e = A.Engine(h, 4, lib=hip)
    e.set_integrator(A.Leapfrog(0.01))
    q0 = np.random.default_rng(1).normal(size=(1, 4))
    p0 = np.random.default_rng(2).normal(size=(1, 4))
    e.set_position(q0, p0)
    rs, Hs = [], []
    for i in range(2000):
        e.step(5)
        z = e.phasepoint()
        rs.append(np.sqrt(z.theta[0] ** 2 + z.r[0] ** 2))
        Hs.append(-(z.lp.value + z.lk.value))
    rs, Hs = np.array(rs)[200:], np.array(Hs)[200:]
    assert np.all(np.abs(rs - rs.mean(axis=0)) < 2e-3)
    assert np.all(np.abs(Hs - Hs.mean(axis=0)) < 2e-3)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("metric", ["unit", "diag_chain"])
def test_refresh_momentum(hip, oracle, rng, dtype, metric):
    """rand_momentum + refresh (src/metric.jl:290-309, src/hamiltonian.jl:213-220): same Philox stream"""
    D, N = 10, 50
    h = A.Hamiltonian(make_metric(metric, D, N, rng), A.IsoGaussian(D))
    g, o = pair(hip, oracle, h, N, dtype, seed=99)
    th = rng.normal(size=(D, N))
    for e in (g, o):
        e.set_position(th)
        e.refresh()
    assert_points_close(g.phasepoint(), o.phasepoint(), dtype, "refresh")
    # partial refreshment (src/hamiltonian.jl:243-254)
    for e in (g, o):
        e.refresh(A.PartialMomentumRefreshment(0.3))
    assert_points_close(g.phasepoint(), o.phasepoint(), dtype, "partial refresh")


def test_tempered_and_jittered(hip, oracle, rng):
    """TemperedLeapfrog / JitteredLeapfrog (src/integrator.jl:140-156, :198-209)"""
    D, N = 5, 32
    h = A.Hamiltonian(A.UnitEuclideanMetric((D, N)), A.IsoGaussian(D))
    g, o = pair(hip, oracle, h, N, np.float64, lf=A.TemperedLeapfrog(0.1, 1.05))
    th, r = rng.normal(size=(D, N)), rng.normal(size=(D, N))
    for e in (g, o):
        e.set_position(th, r)
        e.step(7)
    assert_points_close(g.phasepoint(), o.phasepoint(), np.float64, "tempered")
    k = A.HMCKernel(A.Trajectory(A.EndPointTS, A.JitteredLeapfrog(np.full(N, 0.1), 0.5), A.FixedNSteps(5)))
    g, o = pair(hip, oracle, h, N, np.float64, lf=k.tau.integrator)
    for e in (g, o):
        e.set_position(th)
        e.transition(k)
    sg, so = g.stats(), o.stats()
    np.testing.assert_allclose(sg["step_size"], so["step_size"], rtol=1e-12)
    assert np.ptp(sg["step_size"]) > 0
    assert_points_close(g.phasepoint(), o.phasepoint(), np.float64, "jittered transition")


def realign(g, o, same):
    """A chain that took another decision (a last-ulp difference at a U-turn or acceptance test) carries on from another
    state: put the HIP engine's chains back on the oracle's positions so that EVERY transition is held to the parity
    bar, not only the first (the next momentum is drawn afresh, so θ is the whole state that matters)."""
    if not same.all():
        th = o.phasepoint().theta
        g.set_position(th)
        o.set_position(th)


def compare_transition_stats(sg, so, dtype, o, what="transition", sel=None):
    """stats of the HIP engine against the oracle engine `o`'s after the same transition(s): every discrete statistic identical on
    every chain unless the oracle took one of that chain's decisions within PU.bound(dtype) of a tie (the margin record of `o` is
    read AND reset: one comparison per span of transitions); the continuous statistics to tolerance on the agreeing chains."""
    same = ((sg["n_steps"] == so["n_steps"]) & (sg["is_accept"] == so["is_accept"]) & (sg["tree_depth"] == so["tree_depth"])
            & (sg["numerical_error"] == so["numerical_error"]))
    margin = PU.decision_margin(o)
    same = PU.check_flips(same, margin, dtype, what, sel=sel, n_steps=so["n_steps"])
    rt = RTOL[dtype] * 100
    # The continuous statistics are held to the tolerance where they are well defined on both sides (found by the 10 000-configuration hunt of
    # tests/test_random_configurations.py, `profiles/r6_experiments.md` r6w): (i) a near-tie in the CHOICE of the candidate leaves every discrete
    # statistic alone and moves ℓπ, H and its error — chains with such a decision are left to the discrete check; (ii) ΔH_max is maxabs(a, b)
    # (src/trajectory.jl:526): +x against −x of nearly the same size is a tie of its own — compared in magnitude; (iii) on a trajectory that left
    # the stable region (|ΔH| beyond 20 on its way to Δ_max) the energies amplify rounding: a thousand times the tolerance there.
    with np.errstate(invalid="ignore"):
        wild = (np.abs(sg["max_hamiltonian_energy_error"]) > 20) | (np.abs(so["max_hamiltonian_energy_error"]) > 20)
        wild |= ~np.isfinite(sg["max_hamiltonian_energy_error"]) | ~np.isfinite(so["max_hamiltonian_energy_error"])
    clear = same & (margin >= PU.bound(dtype))
    for k in ("acceptance_rate", "log_density", "hamiltonian_energy", "hamiltonian_energy_error",
              "max_hamiltonian_energy_error", "step_size"):
        a, b = (np.abs(sg[k]), np.abs(so[k])) if k == "max_hamiltonian_energy_error" else (sg[k], so[k])
        calm = clear & ~wild
        np.testing.assert_allclose(a[calm], b[calm], rtol=rt, atol=rt, err_msg=f"{what}: {k}")
        rest = clear & wild & np.isfinite(a) & np.isfinite(b)
        if dtype == np.float64:
            np.testing.assert_allclose(a[rest], b[rest], rtol=rt * 1000, atol=rt * 1000, err_msg=f"{what}: {k} (unstable trajectories)")
    np.testing.assert_array_equal(sg["numerical_error"][same], so["numerical_error"][same])
    return same


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("TS", [A.EndPointTS, A.MultinomialTS])
@pytest.mark.parametrize("metric", ["unit", "diag_chain"])
def test_static_hmc_transitions(hip, oracle, rng, dtype, TS, metric):
    """static transition (src/trajectory.jl:271-390, :855-880): 5 consecutive transitions"""
    D, N = 5, 512
    h = A.Hamiltonian(make_metric(metric, D, N, rng), A.IsoGaussian(D))
    k = A.HMCKernel(A.Trajectory(TS, A.Leapfrog(np.full(N, 0.3)), A.FixedNSteps(10)))
    g, o = pair(hip, oracle, h, N, dtype, seed=3, lf=k.tau.integrator)
    th = rng.random((D, N))
    for e in (g, o):
        e.set_position(th)
    for it in range(5):
        for e in (g, o):
            e.transition(k)
        same = compare_transition_stats(g.stats(), o.stats(), dtype, o, "static hmc")
        if dtype == np.float64:
            zg, zo = g.phasepoint(), o.phasepoint()
            np.testing.assert_allclose(zg.theta[:, same], zo.theta[:, same], rtol=1e-8, atol=1e-8)
            np.testing.assert_allclose(zg.r[:, same], zo.r[:, same], rtol=1e-8, atol=1e-8)
        realign(g, o, same)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("TS", [A.MultinomialTS, A.SliceTS])
@pytest.mark.parametrize("TC", [A.GeneralisedNoUTurn, A.ClassicNoUTurn, A.StrictGeneralisedNoUTurn])
def test_nuts_transitions(hip, oracle, rng, dtype, TS, TC):
    """dynamic transition + build_tree (src/trajectory.jl:626-742): iterative kernel == recursion"""
    D, N = 10, 1024
    h = A.Hamiltonian(make_metric("diag_chain", D, N, rng), A.IsoGaussian(D))
    k = A.HMCKernel(A.Trajectory(TS, A.Leapfrog(np.full(N, 0.25)), TC(max_depth=8)))
    g, o = pair(hip, oracle, h, N, dtype, seed=11, lf=k.tau.integrator)
    th = rng.normal(size=(D, N))
    for e in (g, o):
        e.set_position(th)
    for it in range(4):
        for e in (g, o):
            e.transition(k)
        sg, so = g.stats(), o.stats()
        same = compare_transition_stats(sg, so, dtype, o, "nuts")
        assert sg["tree_depth"].max() >= 3  # the trees are non-trivial
        if dtype == np.float64:
            zg, zo = g.phasepoint(), o.phasepoint()
            np.testing.assert_allclose(zg.theta[:, same], zo.theta[:, same], rtol=1e-8, atol=1e-8)
            np.testing.assert_allclose(zg.lp.gradient[:, same], zo.lp.gradient[:, same], rtol=1e-8, atol=1e-8)
        realign(g, o, same)


@pytest.mark.parametrize("D,target", [(32, "funnel"), (128, "iso"), (100, "hier"), (3, "iso")])
def test_nuts_geometries_and_targets(hip, oracle, rng, D, target):
    """NUTS on the BASELINE config shapes at oracle-sized N, incl. divergent funnel paths"""
    N = 256
    h = A.Hamiltonian(A.DiagEuclideanMetric((D, N)), make_target(target, D, rng))
    eps = 0.5 if target == "funnel" else 0.2
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, A.Leapfrog(np.full(N, eps)), A.GeneralisedNoUTurn()))
    g, o = pair(hip, oracle, h, N, np.float64, seed=5, lf=k.tau.integrator)
    th = rng.normal(size=(D, N))
    for e in (g, o):
        e.set_position(th)
    n_div = 0
    for it in range(3):
        for e in (g, o):
            e.transition(k)
        sg, so = g.stats(), o.stats()
        same = compare_transition_stats(sg, so, np.float64, o, f"nuts {target} D={D}")
        n_div += int(sg["numerical_error"].sum())
        realign(g, o, same)
    if target == "funnel":
        assert n_div > 0, "the funnel at eps=0.5 must produce divergent transitions (Δ_max test, :500-507)"


@pytest.mark.parametrize("D,target", [(400, "iso"), (600, "hier"), (1000, "iso"), (2048, "iso"), (2048, "funnel"), (2048, "hier"), (3000, "diag")])
def test_multiwave_chains(hip, oracle, rng, D, target):
    """D > 512: a chain spans 2-8 wavefronts of one workgroup (cross-wave reductions through LDS).
    Every transition kind on those geometries — BASELINE.json configs[4] is D = 2048 hierarchical Gaussian: that
    very pair runs with 64 chains."""
    N = 64 if (D, target) == (2048, "hier") else 24
    dtype = np.float64
    h = A.Hamiltonian(make_metric("diag_chain", D, N, rng), make_target(target, D, rng))
    eps = 0.3 * D ** -0.25
    lf = A.Leapfrog(np.full(N, eps))
    g, o = pair(hip, oracle, h, N, dtype, seed=3, lf=lf)
    th = 0.5 * rng.normal(size=(D, N))
    for e in (g, o):
        e.set_position(th)
        e.refresh()
    assert_points_close(g.phasepoint(), o.phasepoint(), dtype, "refresh")
    kernels = [
        A.HMCKernel(A.Trajectory(A.EndPointTS, lf, A.FixedNSteps(6))),
        A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.FixedNSteps(6))),
        A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=6))),
        A.HMCKernel(A.Trajectory(A.SliceTS, lf, A.StrictGeneralisedNoUTurn(max_depth=5))),
        A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.ClassicNoUTurn(max_depth=5))),
    ]
    import os, sys
    dbg = os.environ.get("AHMC_TEST_TRACE") == "1"
    for ik, k in enumerate(kernels):
        for it in range(2):
            if dbg: print(f"[trace] D={D} kernel {ik} it {it}: transition", file=sys.stderr, flush=True)
            g.transition(k)
            if dbg: g.sync(); print("[trace]   hip transition done", file=sys.stderr, flush=True)
            o.transition(k)
            sg = g.stats()
            if dbg: print("[trace]   hip stats done", file=sys.stderr, flush=True)
            so = o.stats()
            same = compare_transition_stats(sg, so, dtype, o, f"multiwave D={D} {target} kernel {ik}")
            if dbg: print(f"[trace]   same {same.mean()}", file=sys.stderr, flush=True)
            zg, zo = g.phasepoint(), o.phasepoint()
            np.testing.assert_allclose(zg.theta[:, same], zo.theta[:, same], rtol=1e-8, atol=1e-8)
            realign(g, o, same)
        for e in (g, o):  # re-synchronise the two engines for the next kernel
            e.set_position(o.phasepoint().theta)
    PU.reset_margin(o)
    eg, eo = g.find_good_stepsize(), o.find_good_stepsize()
    PU.check_equal_or_near_tie(eg, eo, PU.decision_margin(o), dtype, f"find_good_stepsize multiwave D={D}")


def _spd(D, rng, cond=4.0):
    """a random symmetric positive-definite (D, D) matrix with a modest condition number"""
    Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
    M = (Q * np.linspace(1.0, cond, D)) @ Q.T
    return np.asfortranarray((M + M.T) / 2)


def _dense_hamiltonian(D, N, rng, metric, target):
    m = {"dense": lambda: A.DenseEuclideanMetric(_spd(D, rng)), "diag": lambda: make_metric("diag_chain", D, N, rng),
         "unit": lambda: A.UnitEuclideanMetric((D, N))}[metric]()
    t = A.DenseGaussian(_spd(D, rng, 3.0)) if target == "dense" else make_target(target, D, rng)
    return A.Hamiltonian(m, t)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D", [5, 64, 100, 200])
def test_dense_phasepoint_leapfrog_refresh(hip, oracle, rng, dtype, D):
    """DenseEuclideanMetric + dense Gaussian target on the MFMA path (src/hamiltonian.jl:60-68,179-184,
    src/metric.jl:311-320): caches, step(lf, h, z, n) both directions, rand_momentum"""
    N = 70  # not a multiple of the 64-column GEMM tile
    h = _dense_hamiltonian(D, N, rng, "dense", "dense")
    g, o = pair(hip, oracle, h, N, dtype, eps=0.05 + 0.05 * rng.random(N))
    th, r = rng.normal(size=(D, N)), rng.normal(size=(D, N))
    for e in (g, o):
        e.set_position(th, r)
    assert_points_close(g.phasepoint(), o.phasepoint(), dtype, "phasepoint")
    for n in (5, -3):
        for e in (g, o):
            e.step(n)
        assert_points_close(g.phasepoint(), o.phasepoint(), dtype, f"step({n})")
    for e in (g, o):
        e.refresh()
    assert_points_close(g.phasepoint(), o.phasepoint(), dtype, "refresh")


@pytest.mark.parametrize("metric,target", [("dense", "dense"), ("dense", "funnel"), ("dense", "iso"), ("diag", "dense"), ("unit", "dense")])
def test_dense_transitions(hip, oracle, rng, metric, target):
    """static HMC (EndPointTS) and NUTS (MultinomialTS / SliceTS + GeneralisedNoUTurn) through the
    step-synchronous dense engine == the oracle's per-chain recursion"""
    D, N = 24, 300
    dtype = np.float64
    h = _dense_hamiltonian(D, N, rng, metric, target)
    lf = A.Leapfrog(np.full(N, 0.2 if target != "funnel" else 0.3))
    g, o = pair(hip, oracle, h, N, dtype, seed=9, lf=lf)
    th = 0.5 * rng.normal(size=(D, N))
    for e in (g, o):
        e.set_position(th)
    kernels = [
        A.HMCKernel(A.Trajectory(A.EndPointTS, lf, A.FixedNSteps(7))),
        A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=7))),
        A.HMCKernel(A.Trajectory(A.SliceTS, lf, A.GeneralisedNoUTurn(max_depth=6))),
    ]
    for k in kernels:
        for it in range(3):
            for e in (g, o):
                e.transition(k)
            sg, so = g.stats(), o.stats()
            same = compare_transition_stats(sg, so, dtype, o, f"dense {metric}/{target}")
            zg, zo = g.phasepoint(), o.phasepoint()
            np.testing.assert_allclose(zg.theta[:, same], zo.theta[:, same], rtol=1e-8, atol=1e-8)
            np.testing.assert_allclose(zg.r[:, same], zo.r[:, same], rtol=1e-8, atol=1e-8)
            np.testing.assert_allclose(zg.lp.gradient[:, same], zo.lp.gradient[:, same], rtol=1e-8, atol=1e-8)
            realign(g, o, same)
        if not isinstance(k.tau.termination_criterion, A.FixedNSteps):
            assert sg["tree_depth"].max() >= 3
        for e in (g, o):
            e.set_position(o.phasepoint().theta)
    # find_good_stepsize (src/trajectory.jl:768-837) as a state machine over global steps; the point survives it
    z_before = g.phasepoint()
    PU.reset_margin(o)
    eg, eo = g.find_good_stepsize(), o.find_good_stepsize()
    PU.check_equal_or_near_tie(eg, eo, PU.decision_margin(o), dtype, f"find_good_stepsize dense {metric}/{target}")
    assert len(np.unique(eo)) > 1
    z_after = g.phasepoint()
    np.testing.assert_array_equal(z_before.theta, z_after.theta)
    np.testing.assert_array_equal(z_before.r, z_after.r)
    np.testing.assert_array_equal(z_before.lp.value, z_after.lp.value)


def test_dense_bulk_sample_and_stepsize_adaptation(hip, rng):
    """ahmc_sample on the dense engine: batched asynchronous transitions == one at a time; dual
    averaging drives the acceptance rate to δ; the draws have the target's covariance"""
    D, N = 16, 2048
    cov = _spd(D, rng, 5.0)
    h = A.Hamiltonian(A.DenseEuclideanMetric(cov), A.DenseGaussian(np.asfortranarray(np.linalg.inv(cov))))
    lf = A.Leapfrog(np.full(N, 0.1))
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=8)))
    th0 = rng.normal(size=(D, N))
    a = A.Engine(h, N, rng=21, lib=hip); a.set_integrator(lf); a.set_position(th0)
    b = A.Engine(h, N, rng=21, lib=hip); b.set_integrator(lf); b.set_position(th0)
    a.run(k, 6, 0)
    for _ in range(6):
        b.transition(k)
    np.testing.assert_array_equal(a.phasepoint().theta, b.phasepoint().theta)
    np.testing.assert_array_equal(a.stats()["n_steps"], b.stats()["n_steps"])
    # step-size adaptation + statistics (M⁻¹ = Σ makes the target isotropic for the sampler)
    a.adaptor_init(A.StepSizeAdaptor(0.8, lf))
    a.run(k, 150, 150)
    a.run(k, 40, 0)
    acc = a.accum()
    assert abs(np.mean(a.stats()["acceptance_rate"]) - 0.8) < 0.08
    n = acc["n_transitions"] * N
    mean = acc["sum_theta"].sum(axis=1) / n
    var = acc["sumsq_theta"].sum(axis=1) / n - mean ** 2
    assert np.abs(mean).max() < 0.05
    np.testing.assert_allclose(var, np.diag(cov), rtol=0.08)


@pytest.mark.parametrize("target", ["dense", "funnel"])
def test_dense_fused_stepsize_warmup_equals_stepwise(hip, rng, target):
    """dense engine, StepSizeAdaptor: the warm-up in BATCHES (every chain adapts its own ϵ at the end of each of its transitions
    inside the point-pool tree kernel, no per-transition barrier) == transition + adapt! once per iteration, bit for bit —
    for the dense target (pool addressed by the GEMM) and for a built-in family behind the dense metric (staged pool)"""
    D, N = 20, 700
    h = _dense_hamiltonian(D, N, rng, "dense", target)
    lf = A.Leapfrog(np.full(N, 0.12))
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=7)))
    th0 = 0.5 * rng.normal(size=(D, N))
    n_adapts, n_total = 14, 18
    a = A.Engine(h, N, rng=5, lib=hip); a.set_integrator(lf); a.set_position(th0); a.adaptor_init(A.StepSizeAdaptor(0.8, lf))
    b = A.Engine(h, N, rng=5, lib=hip); b.set_integrator(lf); b.set_position(th0); b.adaptor_init(A.StepSizeAdaptor(0.8, lf))
    a.run(k, n_total, n_adapts)                      # two launches: 14 adapting transitions in one batch, 4 draws in one
    assert a.info("dense_pool") == 1
    for i in range(1, n_total + 1):
        b.transition(k)
        b.adapt(i, n_adapts)
    za, zb = a.phasepoint(), b.phasepoint()
    np.testing.assert_array_equal(za.theta, zb.theta)
    np.testing.assert_array_equal(za.r, zb.r)
    np.testing.assert_array_equal(a.get_stepsize(), b.get_stepsize())
    sa, sb = a.get_state(), b.get_state()
    np.testing.assert_array_equal(sa["da"], sb["da"])
    assert sa["adaptor"] == sb["adaptor"]
    np.testing.assert_array_equal(a.stats()["n_steps"], b.stats()["n_steps"])
    assert len(np.unique(a.get_stepsize())) > N // 2   # every chain has its own adapted step size
    a.close(); b.close()


def test_dense_two_pipelines_equal_one(hip, rng, monkeypatch):
    """the dense NUTS loop cut into two chain halves, a stream per half (AHMC_DENSE_SPLIT=1, the default), must give exactly
    the chains of the single pipeline (=0): chains are independent and a column's arithmetic does not depend on which other
    columns share its GEMM launch"""
    D, N = 48, 2304
    h = _dense_hamiltonian(D, N, rng, "dense", "dense")
    lf = A.Leapfrog(np.full(N, 0.15) * (0.6 + 0.8 * rng.random(N)))
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=7)))
    th0 = 0.5 * rng.normal(size=(D, N))
    res = []
    for split in ("0", "1"):
        monkeypatch.setenv("AHMC_DENSE_SPLIT", split)
        e = A.Engine(h, N, rng=31, lib=hip)
        e.set_integrator(lf)
        e.set_position(th0)
        e.run(k, 5)
        res.append((e.phasepoint(), e.stats(), e.accum()))
        e.close()
    z0, s0, a0 = res[0]
    assert s0["tree_depth"].max() >= 3
    for z1, s1, a1 in res[1:]:
        np.testing.assert_array_equal(z1.theta, z0.theta)
        np.testing.assert_array_equal(z1.r, z0.r)
        np.testing.assert_array_equal(s1["n_steps"], s0["n_steps"])
        np.testing.assert_array_equal(a1["sum_theta"], a0["sum_theta"])
        assert a1["total_n_steps"] == a0["total_n_steps"]


def test_dense_covariance_adaptation(hip, oracle, rng):
    """WelfordCov behind the shared DenseEuclideanMetric (src/adaptation/massmatrix.jl:283-340): batch (Chan) update on
    the MFMA units == the oracle pushing the chains one after another, on identical (θ, α); then NUTS + StanHMCAdaptor
    end to end: the adapted M⁻¹ approaches the target covariance and the trees get shorter.
    (One partly filled k_dsyrk tile, Float64, N a multiple of 16, two differently rounded algorithms against each other: the estimate against
    an EXACT covariance at every tile shape, K-loop tail and element type, and what an update leaves behind, is tests/test_dense_adaptation.py.)"""
    D, N = 12, 96
    L = np.linalg.cholesky(_spd(D, rng, 6.0))
    h = A.Hamiltonian(A.DenseEuclideanMetric(np.eye(D)), A.IsoGaussian(D))
    lf = A.Leapfrog(np.full(N, 0.2))
    g, o = pair(hip, oracle, h, N, np.float64, lf=lf)
    for e in (g, o):
        e.set_position(np.zeros((D, N)))
        e.adaptor_init(A.StanHMCAdaptor(A.MassMatrixAdaptor(A.DenseEuclideanMetric(np.eye(D))), A.StepSizeAdaptor(0.8, lf)))
    for i in range(1, 161):
        th, al = L @ rng.normal(size=(D, N)) + 0.3, rng.random(N)
        for e in (g, o):
            e.adapt(i, 160, theta=th, alpha=al)
        if i in (100, 150, 160):  # window ends of the 160-step schedule fall before these
            np.testing.assert_allclose(g.get_metric(), o.get_metric(), rtol=1e-9, atol=1e-12, err_msg=f"M⁻¹ at {i}")
            np.testing.assert_allclose(g.get_stepsize(), o.get_stepsize(), rtol=1e-10)
    assert np.abs(g.get_metric() - L @ L.T).max() < 0.5 * np.abs(L @ L.T).max()  # a covariance estimate, not I any more
    # end to end on N(0, Σ)
    D, N = 16, 1024
    Sigma = _spd(D, rng, 30.0)
    h = A.Hamiltonian(A.DenseEuclideanMetric(np.eye(D)), A.DenseGaussian(np.asfortranarray(np.linalg.inv(Sigma))))
    lf = A.Leapfrog(np.full(N, 0.1))
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn()))
    e = A.Engine(h, N, rng=5, lib=hip)
    e.set_integrator(lf)
    e.set_position(rng.normal(size=(D, N)))
    e.find_good_stepsize()
    e.adaptor_init(A.StanHMCAdaptor(A.MassMatrixAdaptor(A.DenseEuclideanMetric(np.eye(D))), A.StepSizeAdaptor(0.8, lf)))
    e.run(k, 250, 250)
    e.run(k, 40, 0)
    acc = e.accum()
    np.testing.assert_allclose(e.get_metric(), Sigma, rtol=0.2, atol=0.2)
    # with M⁻¹ ≈ Σ the sampler sees an isotropic target: short trees at acceptance ≈ δ, right moments
    assert acc["total_n_steps"] / (40 * N) < 12
    assert abs(np.mean(e.stats()["acceptance_rate"]) - 0.8) < 0.1
    n = acc["n_transitions"] * N
    mean = acc["sum_theta"].sum(axis=1) / n
    var = acc["sumsq_theta"].sum(axis=1) / n - mean ** 2
    np.testing.assert_allclose(var, np.diag(Sigma), rtol=0.1)


@pytest.mark.parametrize("name", ["nuts_iso_diag", "nuts_funnel_slice", "hmc_endpoint", "hmc_multinomial"])
def test_against_committed_fixtures(hip, name):
    """HIP engine vs tests/golden/oracle_fixtures.npz (the oracle's results on fixed seeded inputs, committed with the
    script that made them: tests/golden/make_oracle_fixtures.py) — no oracle build needed on the GPU box"""
    import importlib.util
    import os

    here = os.path.join(os.path.dirname(__file__), "golden")
    spec = importlib.util.spec_from_file_location("make_oracle_fixtures", os.path.join(here, "make_oracle_fixtures.py"))
    mod = importlib.util.module_from_spec(spec)
    sys_path = list(__import__("sys").path)
    try:
        spec.loader.exec_module(mod)
    finally:
        __import__("sys").path[:] = sys_path
    ref = np.load(os.path.join(here, "oracle_fixtures.npz"))
    got = mod.run_case(name, hip)
    n = mod.CASES[name][6]
    margin = np.full(mod.CASES[name][2], np.inf)
    for it in range(n):
        same = got[f"{name}/n_steps{it}"] == ref[f"{name}/n_steps{it}"]
        # free-running transitions: a chain that took another branch stays off — allowed only from the oracle's first near-tie on
        margin = np.minimum(margin, ref[f"{name}/margin{it}"])
        same = PU.check_flips(same, margin, np.float64, f"fixture {name} transition {it}")
        np.testing.assert_allclose(got[f"{name}/theta{it}"][:, same], ref[f"{name}/theta{it}"][:, same], rtol=1e-8, atol=1e-8)
        np.testing.assert_allclose(got[f"{name}/H{it}"][same], ref[f"{name}/H{it}"][same], rtol=1e-8, atol=1e-8)
        np.testing.assert_allclose(got[f"{name}/acc{it}"][same], ref[f"{name}/acc{it}"][same], rtol=1e-7, atol=1e-9)


def test_max_depth_and_single_leaf(hip, oracle, rng):
    """max_depth = 1 (one leaf) and a tiny step size that always hits max_depth"""
    D, N = 5, 64
    h = A.Hamiltonian(A.UnitEuclideanMetric((D, N)), A.IsoGaussian(D))
    for md, eps in ((1, 0.2), (4, 1e-3)):
        k = A.HMCKernel(A.Trajectory(A.MultinomialTS, A.Leapfrog(eps), A.GeneralisedNoUTurn(max_depth=md)))
        g, o = pair(hip, oracle, h, N, np.float64, seed=2, lf=k.tau.integrator)
        th = rng.normal(size=(D, N))
        for e in (g, o):
            e.set_position(th)
            e.transition(k)
        sg, so = g.stats(), o.stats()
        compare_transition_stats(sg, so, np.float64, o, f"max_depth {md}")
        if eps < 0.01:
            assert np.all(sg["tree_depth"] == md) and np.all(sg["n_steps"] == 2 ** md - 1)


def test_nonfinite_start_is_rejected(hip, oracle, rng):
    """non-finite energies → -Inf, proposal rejected, numerical_error flagged (src/hamiltonian.jl:95-104)"""
    D, N = 5, 32
    h = A.Hamiltonian(A.UnitEuclideanMetric((D, N)), A.IsoGaussian(D))
    k = A.HMCKernel(A.Trajectory(A.EndPointTS, A.Leapfrog(1e200), A.FixedNSteps(3)))
    g, o = pair(hip, oracle, h, N, np.float64, lf=k.tau.integrator)
    th = rng.normal(size=(D, N))
    for e in (g, o):
        e.set_position(th)
        e.transition(k)
    sg, so = g.stats(), o.stats()
    assert not sg["is_accept"].any() and sg["numerical_error"].all()
    np.testing.assert_array_equal(sg["is_accept"], so["is_accept"])
    np.testing.assert_array_equal(sg["numerical_error"], so["numerical_error"])
    np.testing.assert_allclose(g.theta(), th)  # reverted columns (accept_phasepoint!, :312-332)


def test_find_good_stepsize(hip, oracle, rng):
    """find_good_stepsize per chain (src/trajectory.jl:768-837)"""
    D, N = 10, 128
    h = A.Hamiltonian(A.DiagEuclideanMetric((D, N)), A.IsoGaussian(D))
    g, o = pair(hip, oracle, h, N, np.float64, seed=21)
    th = rng.normal(size=(D, N))
    out = []
    for e in (g, o):
        e.set_position(th)
        out.append(e.find_good_stepsize())
    PU.check_equal_or_near_tie(out[0], out[1], PU.decision_margin(o), np.float64, "find_good_stepsize")
    assert np.all(out[0] > 0) and len(np.unique(out[0])) > 1


@pytest.mark.parametrize("kind", ["stan", "naive", "stepsize", "massmatrix"])
def test_adaptation(hip, oracle, rng, kind):
    """adapt! glue + dual averaging + Welford + Stan windows (src/sampler.jl:72-90, src/adaptation/*.jl)"""
    D, N, n_adapts = 5, 256, 150
    metric = A.DiagEuclideanMetric((D, N))
    h = A.Hamiltonian(metric, A.DiagGaussian(np.zeros(D), np.array([0.5, 1.0, 2.0, 1.0, 0.3])))
    lf = A.Leapfrog(np.full(N, 0.1))
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=6)))
    ad = {"stan": A.StanHMCAdaptor(A.MassMatrixAdaptor(metric), A.StepSizeAdaptor(0.8, lf)),
          "naive": A.NaiveHMCAdaptor(A.MassMatrixAdaptor(metric), A.StepSizeAdaptor(0.8, lf)),
          "stepsize": A.StepSizeAdaptor(0.8, lf), "massmatrix": A.MassMatrixAdaptor(metric)}[kind]
    g, o = pair(hip, oracle, h, N, np.float64, seed=17, lf=lf)
    th = rng.normal(size=(D, N))
    for e in (g, o):
        e.set_position(th)
        e.adaptor_init(ad)
    # The dual-averaging feedback loop (ϵ → α → ϵ, gain 20√m/(m+10) ≈ 3 around m = 10..30) is
    # not contractive per realisation: 1e-16 differences between two correct implementations
    # grow to 1e-6 within ~30 iterations (measured).  So the adaptor is compared on IDENTICAL
    # inputs: the oracle's chain drives both adaptors through adapt!(…, θ, α).
    for i in range(1, n_adapts + 21):
        o.transition(k)
        theta, alpha = o.theta(), o.stats(["acceptance_rate"])["acceptance_rate"]
        for e in (g, o):
            e.adapt(i, n_adapts, theta, alpha)
        if i in (1, 10, 99, 100, 101, n_adapts - 1, n_adapts, n_adapts + 5):
            np.testing.assert_allclose(g.get_stepsize(), o.get_stepsize(), rtol=1e-10, err_msg=f"ϵ at i={i}")
            if kind != "stepsize":
                np.testing.assert_allclose(g.get_metric(), o.get_metric(), rtol=1e-10, err_msg=f"M⁻¹ at i={i}")
        # the oracle keeps sampling with its own adapted (ϵ, M⁻¹)
    eg = g.get_stepsize()
    if kind != "stepsize":
        Mg = g.get_metric()
        if kind != "massmatrix":
            assert np.ptp(Mg) > 0
        # Welford estimate of the target variances (0.25, 1, 4, 1, 0.09), rtol 0.2 as test/adaptation.jl:173-227
        if kind in ("naive", "massmatrix"):
            np.testing.assert_allclose(np.median(Mg, axis=1), [0.25, 1.0, 4.0, 1.0, 0.09], rtol=0.35)
    if kind in ("stan", "naive", "stepsize"):
        assert np.all(eg != 0.1)
    # short-horizon end-to-end: HIP transitions + HIP adaptor vs oracle, before the feedback
    # loop has amplified rounding differences
    g2, o2 = pair(hip, oracle, h, N, np.float64, seed=23, lf=lf)
    for e in (g2, o2):
        e.set_position(th)
        e.adaptor_init(ad)
    for i in range(1, 9):
        for e in (g2, o2):
            e.transition(k)
            e.adapt(i, n_adapts)
    np.testing.assert_allclose(g2.get_stepsize(), o2.get_stepsize(), rtol=1e-7)


def test_dual_averaging_table_and_its_end(hip, oracle, rng):
    """adapt_stepsize! (src/adaptation/stepsize.jl:178-210) reads √m and m^(−κ) from a table built on the device for
    m < 4 096 (k_da_table) and evaluates them beyond: a StepSizeAdaptor driven with the same α on the HIP engine and on the
    oracle (which always evaluates them) agrees on both sides of the table's end and after finalize!"""
    D, N, n_adapts = 4, 128, 4200
    metric = A.DiagEuclideanMetric((D, N))
    h = A.Hamiltonian(metric, A.IsoGaussian(D))
    lf = A.Leapfrog(np.full(N, 0.3))
    g, o = pair(hip, oracle, h, N, np.float64, seed=3, lf=lf)
    th = rng.normal(size=(D, N))
    for e in (g, o):
        e.set_position(th)
        e.adaptor_init(A.StepSizeAdaptor(0.8, lf))
    base = rng.uniform(0.55, 0.95, size=N)  # per-chain mean acceptance: the chains settle on different step sizes
    for i in range(1, n_adapts + 1):
        alpha = np.clip(base + 0.05 * rng.standard_normal(N), 0.0, 1.0)
        for e in (g, o):
            e.adapt(i, n_adapts, th, alpha)
        if i in (1, 2, 100, 4094, 4095, 4096, 4097, 4150, n_adapts - 1, n_adapts):
            np.testing.assert_allclose(g.get_stepsize(), o.get_stepsize(), rtol=1e-12, err_msg=f"ϵ at i={i}")
    assert len(np.unique(g.get_stepsize())) > N // 2


def test_nutpie_var(hip, oracle, rng):
    """NutpieVar (src/adaptation/massmatrix.jl:160-250) on identical (θ, ∇, α) inputs: HIP == oracle; and as the
    estimator of a StanHMCAdaptor on a diagonal Gaussian it recovers σ² (test/adaptation.jl:183-192)"""
    D, N = 6, 64
    metric = A.DiagEuclideanMetric((D, N))
    h = A.Hamiltonian(metric, A.IsoGaussian(D))
    g, o = pair(hip, oracle, h, N, np.float64, eps=0.2)
    for e in (g, o):
        e.set_position(np.zeros((D, N)))
        e.adaptor_init(A.StanHMCAdaptor(A.NutpieVar(metric), A.StepSizeAdaptor(0.8, A.Leapfrog(0.2))))
    for i in range(1, 161):
        th, gr, al = rng.normal(size=(D, N)), rng.normal(size=(D, N)), rng.random(N)
        for e in (g, o):
            e.adapt(i, 160, theta=th, alpha=al, grad=gr)
        if i in (20, 100, 150, 160):
            np.testing.assert_allclose(g.get_metric(), o.get_metric(), rtol=1e-11, err_msg=f"M⁻¹ at {i}")
            np.testing.assert_allclose(g.get_stepsize(), o.get_stepsize(), rtol=1e-10, err_msg=f"ϵ at {i}")
    # end to end: NUTS + Stan windows with the nutpie estimator on N(0, diag σ²)
    D, N = 5, 512
    sig = 0.5 + 2 * rng.random(D)
    metric = A.DiagEuclideanMetric((D, N))
    h = A.Hamiltonian(metric, A.DiagGaussian(np.zeros(D), sig))
    lf = A.Leapfrog(np.full(N, 0.1))
    e = A.Engine(h, N, rng=77, lib=hip)
    e.set_integrator(lf)
    e.set_position(rng.normal(size=(D, N)))
    e.adaptor_init(A.StanHMCAdaptor(A.NutpieVar(metric), A.StepSizeAdaptor(0.8, lf)))
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn()))
    e.run(k, 300, 300)
    np.testing.assert_allclose(np.median(e.get_metric(), axis=1), sig ** 2, rtol=0.1)


def test_bulk_sample_equals_stepwise(hip, rng):
    """ahmc_sample (one enqueue for the whole loop of src/sampler.jl:182-228) == per-iteration calls"""
    D, N, n, n_adapts = 10, 200, 60, 40
    metric = A.DiagEuclideanMetric((D, N))
    h = A.Hamiltonian(metric, A.IsoGaussian(D))
    lf = A.Leapfrog(np.full(N, 0.2))
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn()))
    ad = A.StanHMCAdaptor(A.MassMatrixAdaptor(metric), A.StepSizeAdaptor(0.8, lf))
    th = rng.normal(size=(D, N))
    a = A.Engine(h, N, rng=5, lib=hip)
    b = A.Engine(h, N, rng=5, lib=hip)
    for e in (a, b):
        e.set_integrator(lf)
        e.set_position(th)
        e.adaptor_init(ad)
    out = np.zeros((D, N, n - n_adapts), order="F")
    a.run(k, n, n_adapts, drop_warmup=True, samples_out=out)
    a.sync()
    total = 0
    for i in range(1, n + 1):
        b.transition(k)
        b.adapt(i, n_adapts)
        if i > n_adapts:
            np.testing.assert_array_equal(out[:, :, i - n_adapts - 1], b.theta())
            total += int(b.stats(["n_steps"])["n_steps"].sum())
    acc = a.accum()
    assert acc["total_n_steps"] == total and acc["n_transitions"] == n - n_adapts
    np.testing.assert_allclose(acc["sum_theta"], out.sum(axis=2), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(acc["sumsq_theta"], (out ** 2).sum(axis=2), rtol=1e-12, atol=1e-12)


def test_host_draws_double_buffered(hip, rng):
    """ahmc_sample with a HOST samples_out: batches go through two device stages, the D2H copy of one overlapping the
    next batch's kernel; the draws equal those written straight into a device buffer (several batches, ragged last one)"""
    import torch
    D, N, n = 12, 300, 150
    metric = A.DiagEuclideanMetric((D, N))
    h = A.Hamiltonian(metric, A.IsoGaussian(D))
    lf = A.Leapfrog(np.full(N, 0.25))
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn()))
    th = rng.normal(size=(D, N))
    outs = []
    for where in ("host", "pinned", "device", "host_twice"):
        e = A.Engine(h, N, rng=11, lib=hip)
        e.set_integrator(lf)
        e.set_position(th)
        if where == "device":
            buf = torch.zeros(n * D * N, dtype=torch.float64, device="cuda")
        elif where == "pinned":
            buf = torch.zeros(n * D * N, dtype=torch.float64).pin_memory()
        else:
            buf = np.zeros(n * D * N)
        if where == "host_twice":  # a second call reuses the stages while the first call's copies may be in flight
            e.run(k, 70, samples_out=buf)
            e.run(k, n - 70, samples_out=buf[70 * D * N:])
        else:
            e.run(k, n, samples_out=buf)
        e.sync()
        outs.append(buf.cpu().numpy() if hasattr(buf, "cpu") else buf)
        assert np.all(np.isfinite(outs[-1])) and np.abs(outs[-1][-D * N:]).max() > 0
    for o in outs[1:]:
        np.testing.assert_array_equal(o, outs[0])


@pytest.mark.parametrize("case", ["stan", "stan_nutpie", "naive", "stepsize", "massmatrix", "stan_far_start", "stan_jitter_f32", "stan_endsearly"])
def test_fused_warmup_matches_stepwise(hip, rng, case):
    """Warm-up in batches (adapt! inside k_nuts, MODE 3 / 4) == transition + adapt! per iteration, bit for bit:
    every adaptor kind, NutpieVar, a start 30σ out (the linear-domain pass bails and the log-domain redo pass resumes
    mid-batch with the chain's adaptation state), jittered step sizes in Float32"""
    D, N, n_adapts, n = 8, 256, 160, 170  # Stan windows of 160 warm-up steps: one metric update, at 100
    if "endsearly" in case:
        n = 120  # the run stops inside the warm-up, after the metric update at 100
    dtype = np.float32 if case.endswith("f32") else np.float64
    metric = A.DiagEuclideanMetric((D, N))
    h = A.Hamiltonian(metric, A.DiagGaussian(np.zeros(D), 0.5 + np.arange(D) / 4.0))
    lf = A.JitteredLeapfrog(np.full(N, 0.2), 0.3) if "jitter" in case else A.Leapfrog(np.full(N, 0.2))
    pc = A.NutpieVar(metric) if "nutpie" in case else A.MassMatrixAdaptor(metric)
    ssa = A.StepSizeAdaptor(0.8, lf)
    ad = {"stan": A.StanHMCAdaptor(pc, ssa), "naive": A.NaiveHMCAdaptor(pc, ssa), "stepsize": ssa, "massmatrix": pc}[case.split("_")[0]]
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn()))
    th = rng.normal(size=(D, N)) + (30.0 if "far" in case else 0.0)
    a = A.Engine(h, N, dtype=dtype, rng=8, lib=hip)
    b = A.Engine(h, N, dtype=dtype, rng=8, lib=hip)
    for e in (a, b):
        e.set_integrator(lf)
        e.set_position(th)
        e.adaptor_init(ad)
    a.run(k, n, n_adapts)
    for i in range(1, n + 1):
        b.transition(k)
        b.adapt(i, n_adapts)
    np.testing.assert_array_equal(a.theta(), b.theta())
    np.testing.assert_array_equal(a.get_stepsize(), b.get_stepsize())
    ma, mb = a.get_metric(), b.get_metric()
    np.testing.assert_array_equal(ma, mb)
    sa, sb = a.stats(), b.stats()
    for f in ("n_steps", "acceptance_rate", "hamiltonian_energy", "tree_depth"):
        np.testing.assert_array_equal(sa[f], sb[f])
    if case.split("_")[0] not in ("stepsize",):
        assert np.abs(ma - 1).max() > 0.05  # the metric did adapt


def test_same_rng_vector_gives_identical_chains(hip, rng):
    """test/sampler-vec.jl:69-80: a vector of identically seeded RNGs ⇒ all chains bit-identical"""
    D, N = 5, 5
    for TS in (A.EndPointTS, A.MultinomialTS):
        h = A.Hamiltonian(A.DiagEuclideanMetric((D, N)), A.IsoGaussian(D))
        k = A.HMCKernel(A.Trajectory(TS, A.Leapfrog(np.full(N, 0.1)), A.FixedNSteps(10)))
        th0 = np.repeat(rng.random((D, 1)), N, axis=1)
        samples, _ = A.sample([A.PhiloxRNG(1) for _ in range(N)], h, k, th0, 20, lib=hip)
        for s in samples[1:10]:
            for j in range(1, N):
                np.testing.assert_array_equal(s[:, j], s[:, 0])


@pytest.mark.parametrize("metricT", [A.UnitEuclideanMetric, A.DiagEuclideanMetric])
@pytest.mark.parametrize("TS", [A.EndPointTS, A.MultinomialTS])
def test_sampler_vec_statistical(hip, metricT, TS):
    """test/sampler-vec.jl:36-43: 5 chains × D=5, mean(samples) ≈ 0 atol RNDATOL*n_chains = 2.5
    (2 000 samples here; the far tighter 0.2 bound is what we assert)"""
    D, N = 5, 5
    h = A.Hamiltonian(metricT((D, N)), A.IsoGaussian(D))
    k = A.HMCKernel(A.Trajectory(TS, A.Leapfrog(np.full(N, 0.1)), A.FixedNSteps(10)))
    th0 = np.random.default_rng(100).random((D, N))
    samples, stats = A.sample(100, h, k, th0, 2000, lib=hip)
    m = np.mean(samples, axis=0)
    assert np.all(np.abs(m) < KATOL)  # the reference's own bound (RNDATOL * n_chains = 2.5) ...
    assert np.all(np.abs(m) < 0.5)    # ... and a 5x tighter one (2 000 autocorrelated draws per chain)
    assert abs(np.var(np.stack(samples[200:])) - 1) < 0.15
    assert set(stats[0]) >= {"n_steps", "is_accept", "acceptance_rate", "log_density", "hamiltonian_energy",
                             "hamiltonian_energy_error", "numerical_error", "step_size", "nom_step_size", "is_adapt"}


def test_nuts_with_stan_adaptor_statistical(hip):
    """cfg2-shaped run at small N: NUTS(0.8)+StanHMCAdaptor recovers N(0, I) moments"""
    D, N = 16, 512
    metric = A.DiagEuclideanMetric((D, N))
    h = A.Hamiltonian(metric, A.IsoGaussian(D))
    e = A.Engine(h, N, rng=1, lib=hip)
    lf = A.Leapfrog(np.full(N, 0.1))
    e.set_integrator(lf)
    e.set_position(np.random.default_rng(0).random((D, N)))
    e.find_good_stepsize()
    e.adaptor_init(A.StanHMCAdaptor(A.MassMatrixAdaptor(metric), A.StepSizeAdaptor(0.8, lf)))
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn()))
    e.run(k, 500, 300, drop_warmup=True)
    acc = e.accum()
    n = acc["n_transitions"]
    assert n == 200
    mean = acc["sum_theta"].sum(axis=1) / (n * N)
    var = acc["sumsq_theta"].sum(axis=1) / (n * N) - mean ** 2
    assert np.all(np.abs(mean) < 0.03), mean
    assert np.all(np.abs(var - 1) < 0.06), var
    assert acc["n_divergent"] == 0
    assert 3 <= acc["total_n_steps"] / (n * N) <= 20


def test_full_size_properties(hip):
    """BASELINE cfg2 at full size (65 536 chains × D=128, Float64): size-independent properties —
    determinism under the same seed, energy bookkeeping H-H0 == stat, Σ n_steps == accumulator,
    2^depth-1 <= n_steps < 2^(depth+1), acceptance in [0,1], no write outside the state."""
    D, N = 128, 65536
    h = A.Hamiltonian(A.DiagEuclideanMetric((D,)), A.IsoGaussian(D))
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, A.Leapfrog(0.3), A.GeneralisedNoUTurn()))
    th0 = np.random.default_rng(3).random((D, N))
    res = []
    for rep in range(2):
        e = A.Engine(h, N, rng=42, lib=hip)
        e.set_integrator(k.tau.integrator)
        e.set_position(th0)
        e.run(k, 3)
        st = e.stats()
        z = e.phasepoint()
        acc = e.accum(moments=False)
        res.append((st, z, acc))
        e.close()
    (s1, z1, a1), (s2, z2, a2) = res
    np.testing.assert_array_equal(z1.theta, z2.theta)
    np.testing.assert_array_equal(s1["n_steps"], s2["n_steps"])
    assert a1["total_n_steps"] == a2["total_n_steps"] and a1["n_transitions"] == 3
    d, n = s1["tree_depth"], s1["n_steps"]
    assert np.all(n >= 2 ** d - 1) and np.all(n < 2 ** (d + 1))
    assert np.all((s1["acceptance_rate"] >= 0) & (s1["acceptance_rate"] <= 1))
    np.testing.assert_allclose(-(z1.lp.value + z1.lk.value), s1["hamiltonian_energy"], rtol=1e-12)
    np.testing.assert_allclose(z1.lp.gradient, z1.theta, rtol=1e-12)  # -∇ℓπ = θ for N(0, I)
    assert np.all(np.isfinite(z1.theta)) and not s1["numerical_error"].any()


def test_cfg2_pipeline_against_oracle(hip, oracle):
    """The pipeline bench.py times, against the oracle chain for chain: D=128 iso Gaussian, per-chain Diag metric,
    θ0 ~ U(0,1), find_good_stepsize, then NUTS(0.8) + StanHMCAdaptor through the FUSED warm-up (k_nuts MODE 3 / 4:
    adapt! inside the kernel, batches of transitions per launch) and the batched draws (MODE 0 / 1).

    Dual averaging feeds every transition's α back into the next step size, so a last-bit difference grows by ≈2× per
    iteration (1e-16 → 1e-6 in ≈30); a free-running comparison is therefore only meaningful over short horizons.  The
    run is cut into chunks — one iteration each through the warm-up, ten for the draws —: each chunk starts both engines from the
    ORACLE's complete state (θ, ϵ, M⁻¹, DAState, Welford (n, μ, M), window counter — ahmc_get/set_adaptor_state) and is compared at
    its end, which holds every iteration of the warm-up — init buffer, the window (76…100), the metric update and the dual-averaging
    reset at its end, the term buffer, finalize! at n_adapts — and the first draws to the chain-for-chain bar."""
    D, N, n_adapts, n_total, chunk = 128, 384, 150, 170, 10
    metric = A.DiagEuclideanMetric(np.ones((D, N), order="F"))
    h = A.Hamiltonian(metric, A.IsoGaussian(D))
    lf = A.Leapfrog(np.full(N, 0.1))
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=10, delta_max=1000.0)))
    th0 = np.asfortranarray(np.random.default_rng(2).random((D, N)))
    g, o = pair(hip, oracle, h, N, np.float64, seed=0x5EED0002, lf=lf)
    for e in (g, o):
        e.set_position(th0)
    eg, eo = g.find_good_stepsize(), o.find_good_stepsize()
    PU.check_equal_or_near_tie(eg, eo, PU.decision_margin(o), np.float64, "cfg2 pipeline find_good_stepsize")
    g.set_integrator(A.Leapfrog(eo))   # (a chain that sat on a tie of the search would start from another ϵ)
    for e in (g, o):
        e.adaptor_init(A.StanHMCAdaptor(A.MassMatrixAdaptor(metric), A.StepSizeAdaptor(0.8, lf)))
    # Chunks (round 6): ONE iteration through the warm-up, ten for the draws.  The margin rule — a chain may leave the oracle's track only
    # where the oracle was within 1e-9 of a tie — is a statement about one transition from identical states.  Dual averaging feeds the
    # energies' own rounding (|H| ≈ 230: 1e-13) into the next ϵ and multiplies it by 3 … 10 per iteration (scripts/dbg_flip.py: ϵ apart by
    # 4e-13 after one iteration, 4e-8 after ten), so over a ten-iteration chunk a decision with a margin of 4e-6 did flip legitimately
    # (profiles/r6_experiments.md r6l).  The batched launches of the fused warm-up are held to the per-iteration path bit for bit by
    # test_fused_warmup_matches_stepwise; here every iteration of the schedule is held to the oracle exactly.
    bounds, lo = [], 1
    while lo <= n_total:
        hi = lo if lo <= n_adapts else min(lo + chunk - 1, n_total)
        bounds.append((lo, hi))
        lo = hi + 1
    for lo, hi in bounds:
        so = o.get_state()
        g.set_state(so)                                     # both start the chunk from the oracle's state
        for e in (g, o):
            e.run(k, hi, n_adapts, i_first=lo)
        sg, so2 = g.get_state(), o.get_state()
        assert sg["adaptor"] == so2["adaptor"]              # iteration / window / Welford counters
        # A chain is "on track" if it took the same decisions throughout the chunk: the chunk's last tree is the same and its θ
        # agrees to the rounding ten dual-averaged iterations leave.  (Measured, scripts/dbg_flip.py: from identical states the two
        # sides' ϵ differ by 4e-13 after one iteration — the energies, |H| ≈ 230, round differently by 1e-13 and α′ = exp(−ΔH)
        # carries that into H̄ — and by up to 4e-8 after ten, θ by 6e-7, with every n_steps and tree_depth identical; a chain that
        # DID take another branch ends O(1) away.  Rounds 1–5 held θ to 1e-7 here and counted two such chains as "flips".)
        stg, sto = g.stats(), o.stats()
        on = np.isclose(sg["theta"], so2["theta"], rtol=1e-5, atol=1e-5).all(axis=0) & (stg["n_steps"] == sto["n_steps"]) & (stg["tree_depth"] == sto["tree_depth"])
        # … and may be off it only if the oracle took one of its decisions of this chunk within 1e-9 of a tie
        on = PU.check_flips(on, PU.decision_margin(o), np.float64, f"cfg2 pipeline iterations {lo}..{hi}")
        np.testing.assert_allclose(sg["stepsize"][on], so2["stepsize"][on], rtol=1e-6, err_msg=f"ϵ after iterations {lo}..{hi}")
        np.testing.assert_allclose(sg["metric"][:, on], so2["metric"][:, on], rtol=1e-6, err_msg=f"M⁻¹ after {lo}..{hi}")
        if sg["da"] is not None:
            np.testing.assert_allclose(sg["da"][:, on], so2["da"][:, on], rtol=1e-6, atol=1e-9, err_msg=f"DAState after {lo}..{hi}")
        if sg["welford"] is not None:
            w_g, w_o = sg["welford"][:, on, :], so2["welford"][:, on, :]
            np.testing.assert_allclose(w_g, w_o, rtol=1e-6, atol=1e-8, err_msg=f"Welford after {lo}..{hi}")
        if lo <= 100 <= hi:
            assert not np.allclose(so2["metric"], 1.0), "the window end at iteration 100 must have updated M⁻¹"
    st = o.get_state()
    assert st["adaptor"]["adapting"] == 0 and st["adaptor"]["iteration"] == n_total
    # after the warm-up both sides carry the finalized step sizes: NUTS on N(0, I) at δ = 0.8 in D = 128
    assert 0.3 < np.median(st["stepsize"]) < 0.8, np.median(st["stepsize"])
    g.close(); o.close()


def test_cfg2_pipeline_against_oracle_f32(hip, oracle):
    """The cfg2 pipeline in Float32 (the element type of the reference's own GPU smoke test, test/CUDA/cuda.jl:18) against the Float32
    oracle: fused warm-up (adapt! inside k_nuts<float,32,4,3,0> … the f32 geometry of D = 128) through a whole Stan schedule —
    init buffer 9, window splits at 24 and 54 with metric update + dual-averaging restart, term buffer, finalize! at 60 — and the first
    draws, ONE iteration per chunk from the oracle's complete state: in single precision a rounding is 1e-7 and dual averaging doubles
    it every iteration, so only the single transition + adapt! is held to the Float32 bar of this file (2e-3; identical discrete
    decisions on every chain the oracle did not take within 1e-3 of a tie), every iteration of the schedule."""
    D, N, n_adapts, n_total = 128, 256, 60, 66
    metric = A.DiagEuclideanMetric(np.ones((D, N), order="F"))
    h = A.Hamiltonian(metric, A.IsoGaussian(D))
    lf = A.Leapfrog(np.full(N, 0.1))
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=10, delta_max=1000.0)))
    th0 = np.asfortranarray(np.random.default_rng(2).random((D, N)))
    g, o = pair(hip, oracle, h, N, np.float32, seed=0x5EED0002, lf=lf)
    for e in (g, o):
        e.set_position(th0)
    eg, eo = g.find_good_stepsize(), o.find_good_stepsize()
    PU.check_equal_or_near_tie(eg, eo, PU.decision_margin(o), np.float32, "cfg2 f32 pipeline find_good_stepsize")
    g.set_integrator(A.Leapfrog(eo))
    ad = A.StanHMCAdaptor(A.MassMatrixAdaptor(metric), A.StepSizeAdaptor(0.8, lf), init_buffer=9, term_buffer=6, window_size=15)
    for e in (g, o):
        e.adaptor_init(ad)
    updated = False
    for i in range(1, n_total + 1):
        g.set_state(o.get_state())
        for e in (g, o):
            e.run(k, i, n_adapts, i_first=i)
        sg, so = g.get_state(), o.get_state()
        assert sg["adaptor"] == so["adaptor"]
        stg, sto = g.stats(), o.stats()
        same = (stg["n_steps"] == sto["n_steps"]) & (stg["tree_depth"] == sto["tree_depth"]) & (stg["numerical_error"] == sto["numerical_error"])
        on = same & np.isclose(sg["theta"], so["theta"], rtol=2e-3, atol=2e-3).all(axis=0)
        on = PU.check_flips(on, PU.decision_margin(o), np.float32, f"cfg2 f32 pipeline iteration {i}", n_steps=sto["n_steps"])
        np.testing.assert_allclose(stg["hamiltonian_energy"][on], sto["hamiltonian_energy"][on], rtol=2e-3, err_msg=f"H at iteration {i}")
        np.testing.assert_allclose(stg["acceptance_rate"][on], sto["acceptance_rate"][on], rtol=2e-2, atol=2e-3, err_msg=f"α at iteration {i}")
        np.testing.assert_allclose(sg["stepsize"][on], so["stepsize"][on], rtol=5e-3, err_msg=f"ϵ after adapt! {i}")
        np.testing.assert_allclose(sg["metric"][:, on], so["metric"][:, on], rtol=5e-3, atol=1e-5, err_msg=f"M⁻¹ after adapt! {i}")
        if sg["welford"] is not None:
            np.testing.assert_allclose(sg["welford"][:, on, :], so["welford"][:, on, :], rtol=5e-3, atol=5e-3, err_msg=f"Welford after {i}")
        updated = updated or not np.allclose(so["metric"], 1.0)
    st = o.get_state()
    assert st["adaptor"]["adapting"] == 0 and st["adaptor"]["iteration"] == n_total and updated
    assert 0.3 < np.median(st["stepsize"]) < 0.9, np.median(st["stepsize"])
    g.close(); o.close()


@pytest.mark.parametrize("cfg,offset", [("cfg2", 0), ("cfg2", 30000), ("cfg2", 65536 - 256), ("cfg3", 0), ("cfg3", 41000), ("cfg3", 65536 - 256)])
def test_full_size_slice_against_oracle(hip, oracle, cfg, offset):
    """cfg2 (65 536 chains × D = 128 iso Gaussian) and cfg3 (65 536 × D = 32 Neal's funnel, 4 chains per wave in lockstep,
    divergent paths) at FULL size on the HIP engine — per-chain M⁻¹ and ϵ, dispatch order by step size, batched launches —
    and 256 of its chains replayed by the oracle with the same global Philox stream (chain_offset): the chains of a full
    launch must be the chains of a small one, bit-for-decision."""
    N, n = 65536, 256
    D, target = (128, A.IsoGaussian(128)) if cfg == "cfg2" else (32, A.Funnel(32))
    rs = np.random.default_rng(11)
    minv = np.asfortranarray(0.5 + rs.random((D, N)))
    eps = (0.25 if cfg == "cfg2" else 0.35) * (0.6 + 0.8 * rs.random(N))
    th0 = np.asfortranarray(rs.normal(size=(D, N)))
    k_of = lambda e: A.HMCKernel(A.Trajectory(A.MultinomialTS, A.Leapfrog(e), A.GeneralisedNoUTurn(max_depth=10, delta_max=1000.0)))  # noqa: E731
    g = A.Engine(A.Hamiltonian(A.DiagEuclideanMetric(minv), target), N, rng=A.PhiloxRNG(42), lib=hip)
    g.set_integrator(A.Leapfrog(eps))
    g.set_position(th0)
    g.run(k_of(eps), 4)           # 4 transitions in ONE launch, chains dispatched in ascending-ϵ order
    sl = slice(offset, offset + n)
    o = A.Engine(A.Hamiltonian(A.DiagEuclideanMetric(np.asfortranarray(minv[:, sl])), target), n,
                 rng=A.PhiloxRNG(42, chain_offset=offset), lib=oracle)
    o.set_integrator(A.Leapfrog(eps[sl]))
    o.set_position(th0[:, sl])
    o.run(k_of(eps[sl]), 4)
    sg, so = g.stats(), o.stats()
    same = (sg["n_steps"][sl] == so["n_steps"]) & (sg["tree_depth"][sl] == so["tree_depth"])
    zg, zo = g.phasepoint(), o.phasepoint()
    on = np.isclose(zg.theta[:, sl], zo.theta, rtol=1e-8, atol=1e-8).all(axis=0)
    # 4 free-running transitions: a flipped decision stays flipped — allowed only where the oracle was within 1e-9 of a tie
    on = PU.check_flips(on, PU.decision_margin(o), np.float64, f"{cfg} full-size slice at {offset}")
    assert (same | ~on).all()
    np.testing.assert_allclose(sg["hamiltonian_energy"][sl][on], so["hamiltonian_energy"][on], rtol=1e-9)
    np.testing.assert_allclose(sg["acceptance_rate"][sl][on], so["acceptance_rate"][on], rtol=1e-8, atol=1e-10)
    np.testing.assert_array_equal(sg["numerical_error"][sl][on], so["numerical_error"][on])
    ag, ao = g.accum(), o.accum()
    np.testing.assert_allclose(ag["sum_theta"][:, sl][:, on], ao["sum_theta"][:, on], rtol=1e-8, atol=1e-8)
    if cfg == "cfg3":
        assert ao["n_divergent"] > 0, "the funnel slice must contain divergent transitions"
    g.close(); o.close()


def test_cfg5_full_size_slices_against_oracle(hip, oracle):
    """cfg5 at FULL size — 32 768 chains × D = 2 048 hierarchical Gaussian, one chain across the 4 wavefronts of a workgroup
    (k_nuts<double,256,8,·,3>), per-chain M⁻¹ and ϵ, 4 transitions in ONE launch dispatched in ascending-ϵ order, 512 MiB per (D, N)
    array, per-wave global scratch for the pending levels ≥ 3 — and 32 of its chains replayed by the oracle at three offsets (first,
    middle, last workgroups of the grid) with the same global Philox stream (src/trajectory.jl:626-742 at D = 2 048).  Round 2's silent
    bug was a size / instantiation effect: the chains of the full launch must be the chains of a small one, decision for decision.
    Step sizes ≈ 0.02 from θ0 ~ N(0, I): trees from one leaf to 512 leaves, divergent transitions among them."""
    N, n, D = 32768, 32, 2048
    rs = np.random.default_rng(11)
    minv = np.asfortranarray(0.5 + rs.random((D, N)))
    eps = 0.02 * (0.6 + 0.8 * rs.random(N))
    th0 = np.asfortranarray(rs.normal(size=(D, N)))
    target = A.HierGaussian(D)
    k_of = lambda e: A.HMCKernel(A.Trajectory(A.MultinomialTS, A.Leapfrog(e), A.GeneralisedNoUTurn(max_depth=10, delta_max=1000.0)))  # noqa: E731
    g = A.Engine(A.Hamiltonian(A.DiagEuclideanMetric(minv), target), N, rng=A.PhiloxRNG(42), lib=hip)
    assert hip.backend != "hip:gfx950" or (g.info("group_lanes"), g.info("elems_per_lane")) == (256, 8)
    g.set_integrator(A.Leapfrog(eps))
    g.set_position(th0)
    g.run(k_of(eps), 4)
    sg, zg, ag = g.stats(), g.phasepoint(), g.accum()
    g.close()
    depth_max, n_div, n_on = 0, 0, 0
    for offset in (0, 17000, N - n):
        sl = slice(offset, offset + n)
        o = A.Engine(A.Hamiltonian(A.DiagEuclideanMetric(np.asfortranarray(minv[:, sl])), target), n,
                     rng=A.PhiloxRNG(42, chain_offset=offset), lib=oracle)
        o.set_integrator(A.Leapfrog(eps[sl]))
        o.set_position(th0[:, sl])
        o.run(k_of(eps[sl]), 4)
        so, zo, ao = o.stats(), o.phasepoint(), o.accum()
        margin = PU.decision_margin(o)
        o.close()
        same = (sg["n_steps"][sl] == so["n_steps"]) & (sg["tree_depth"][sl] == so["tree_depth"])
        on = np.isclose(zg.theta[:, sl], zo.theta, rtol=1e-8, atol=1e-8).all(axis=0)
        # 4 free-running transitions of up to 512 leaves: a flipped decision stays flipped — allowed only at the oracle's near-ties
        on = PU.check_flips(on, margin, np.float64, f"cfg5 full-size slice at {offset}")
        assert (same | ~on).all(), offset
        np.testing.assert_allclose(sg["hamiltonian_energy"][sl][on], so["hamiltonian_energy"][on], rtol=1e-9)
        # (α = mean of exp(min(0, −ΔH)) over up to 512 leaves with |H| ≈ 10⁴: the rounding of ΔH after four free-running transitions
        # shows at 1e-6 relative — the bar of tests/test_pipeline_parity.py)
        np.testing.assert_allclose(sg["acceptance_rate"][sl][on], so["acceptance_rate"][on], rtol=1e-4, atol=1e-6)
        np.testing.assert_array_equal(sg["numerical_error"][sl][on], so["numerical_error"][on])
        np.testing.assert_allclose(zg.r[:, sl][:, on], zo.r[:, on], rtol=1e-8, atol=1e-8)
        np.testing.assert_allclose(ag["sum_theta"][:, sl][:, on], ao["sum_theta"][:, on], rtol=1e-8, atol=1e-8)
        depth_max = max(depth_max, int(so["tree_depth"].max()))
        n_div += int(ao["n_divergent"])
        n_on += int(on.sum())
    assert depth_max >= 7 and n_div > 0 and n_on >= 3 * n - 3, (depth_max, n_div, n_on)


@pytest.mark.parametrize("engine,metric", [("step", "identity"), ("step", "spd"), ("epoch", "identity"), ("epoch", "spd"), ("epoch_full_shard", "spd"),
                                           ("epoch_slice", "spd"), ("epoch_d256", "spd"), ("epoch_d256_slice", "identity"),
                                           # round 6: k_dense_epoch2 against the ORACLE (it is held to the step-synchronous kernels by the test below)
                                           ("epoch2_nct1", "spd"), ("epoch2_nct2", "identity"), ("epoch2_d384", "spd"), ("epoch2_f32", "spd"), ("epoch2_f32_d768", "identity"),
                                           ("epoch2_classic", "spd"), ("epoch2_strict_slice", "spd"), ("epoch_tempered", "spd"), ("epoch2_f32_strict_tempered", "spd")])
def test_cfg4_shape_against_oracle(hip, oracle, metric, engine, monkeypatch):
    """BASELINE configs[3] at its own shape: D = 512, Σᵢⱼ = 0.9^|i−j| as a dense Gaussian target (ℓπ = −½θᵀΣ⁻¹θ, the gradient
    a GEMM), shared DenseEuclideanMetric (`identity` = cfg4's initial M⁻¹ = I; `spd` = a well-conditioned full matrix, so the
    second product (M⁻¹P)θ′ and the momentum solve U⁻¹z are not trivial), NUTS(0.8) + StepSizeAdaptor — on 2 304 chains, so
    the engine runs what the bench runs: the 64×64-tile `k_dgemm` (both products in one launch, 16 × 18 workgroups per
    half), the two chain pipelines on two streams, compaction, `k_d_tree<T,256>`.  The oracle replays the FIRST and the LAST
    64 chains (one in each pipeline) through `chain_offset` (src/hamiltonian.jl:60-68,179-184, src/metric.jl:311-320,
    src/trajectory.jl:626-742 per chain).  Every iteration (transition + adapt!) starts from the oracle's state for those
    chains and is held to the bar: identical discrete decisions on every one of them (unless the oracle was within 1e-9 of a tie), 1e-8 on θ, r, ∇ℓπ.
    `engine`: "step" = the step-synchronous kernels (`k_dgemm` → `k_d_tree2` per global step); "epoch" = round 4's chain-complete
    `k_dense_epoch` (what the bench runs at 8 192 chains; here its threshold is lowered so that 1 152 chains per pipeline take it);
    "epoch_full_shard" = cfg4's own 8 192 chains per GPU with the engine's defaults, exactly the bench's pipeline;
    "epoch_slice" = `k_dense_epoch` with SliceTS (src/trajectory.jl:144-150,178-189,500-502) and "epoch_d256(_slice)" = its D = 256
    instantiation — round 5: both were HIP == HIP only (test_dense_epoch_kernel_equals_step_synchronous_kernels), now against the oracle.
    Round 6, "epoch2_*": `k_dense_epoch2` — the 16-chain / two-workgroup shape and the 32-chain shape at D = 512, six waves at D = 384, Float32
    (D = 512 and twelve waves at D = 768; 2e-3 and the Float32 margin bound), ClassicNoUTurn and StrictGeneralisedNoUTurn in its tree phase
    (src/trajectory.jl:551-557,579-617), and the TemperedLeapfrog (src/integrator.jl:198-209) in round 4's kernel and in `k_dense_epoch2`."""
    name = engine
    sampler = A.SliceTS if "_slice" in name else A.MultinomialTS
    D = 256 if "_d256" in name else (384 if "_d384" in name else (768 if "_d768" in name else 512))
    dtype = np.float32 if "_f32" in name else np.float64
    TC = A.ClassicNoUTurn if "_classic" in name else (A.StrictGeneralisedNoUTurn if "_strict" in name else A.GeneralisedNoUTurn)
    temper = 1.04 if "_tempered" in name else None
    for var in ("AHMC_DENSE_EPOCH_V", "AHMC_DENSE_EPOCH_NCT"):
        monkeypatch.delenv(var, raising=False)
    if name.startswith("epoch2"):
        monkeypatch.setenv("AHMC_DENSE_EPOCH_V", "2")
        if "_nct" in name:
            monkeypatch.setenv("AHMC_DENSE_EPOCH_NCT", name.split("_nct")[1][0])
    if engine.startswith("epoch") and engine not in ("epoch", "epoch_full_shard"):
        engine = "epoch"
    if engine == "epoch_full_shard":
        monkeypatch.delenv("AHMC_DENSE_EPOCH", raising=False)
        monkeypatch.delenv("AHMC_DENSE_EPOCH_MIN", raising=False)
    else:
        monkeypatch.setenv("AHMC_DENSE_EPOCH", "1" if engine == "epoch" else "0")
        monkeypatch.setenv("AHMC_DENSE_EPOCH_MIN", "32")
    N, n = (8192 if engine == "epoch_full_shard" else 2304), 64
    idx = np.arange(D)
    Sigma = 0.9 ** np.abs(idx[:, None] - idx[None, :])
    P = np.asfortranarray(np.linalg.inv(Sigma))
    rs = np.random.default_rng(2024)
    if metric == "identity":
        Minv = np.eye(D, order="F")
    else:
        Q, _ = np.linalg.qr(rs.normal(size=(D, D)))
        Minv = (Q * np.linspace(0.6, 2.0, D)) @ Q.T
        Minv = np.asfortranarray((Minv + Minv.T) / 2)
    target = A.DenseGaussian(P)
    th0 = np.asfortranarray(rs.normal(size=(D, N)))
    eps0 = 0.12 * (0.7 + 0.6 * rs.random(N))
    mk_lf = (lambda e: A.TemperedLeapfrog(e, temper)) if temper else A.Leapfrog
    lf = mk_lf(eps0)
    k = A.HMCKernel(A.Trajectory(sampler, lf, TC(max_depth=10, delta_max=1000.0)))
    g = A.Engine(A.Hamiltonian(A.DenseEuclideanMetric(Minv), target), N, dtype=dtype, rng=A.PhiloxRNG(77), lib=hip)
    g.set_integrator(lf)
    g.set_position(th0)
    g.adaptor_init(A.StepSizeAdaptor(0.8, lf))
    offsets = (0, N - n)
    os_ = []
    for off in offsets:
        o = A.Engine(A.Hamiltonian(A.DenseEuclideanMetric(Minv), target), n, dtype=dtype, rng=A.PhiloxRNG(77, chain_offset=off), lib=oracle)
        o.set_integrator(mk_lf(eps0[off:off + n]))
        o.set_position(th0[:, off:off + n])
        o.adaptor_init(A.StepSizeAdaptor(0.8, mk_lf(eps0[off:off + n])))
        os_.append(o)
    tol = 1e-8 if dtype == np.float64 else 2e-3
    n_adapts, n_iter = 3, 4            # three adapting iterations and one draw after finalize!
    depth_seen = 0
    for i in range(1, n_iter + 1):
        # start the iteration from the oracle's state on the replayed chains (θ, r, caches, ϵ, DAState)
        sg = g.get_state()
        for off, o in zip(offsets, os_):
            so = o.get_state()
            sl = slice(off, off + n)
            for key in ("theta", "r", "grad"):
                sg[key][:, sl] = so[key]
            sg["lp"][sl] = so["lp"]
            sg["stepsize"][sl] = so["stepsize"]
            if sg["da"] is not None:
                sg["da"][:, sl] = so["da"]
            # (the counters and flags identical; δ is reported in the element type by the Float32 checker: 0.8f)
            assert {kk: v for kk, v in sg["adaptor"].items() if kk != "delta"} == {kk: v for kk, v in so["adaptor"].items() if kk != "delta"}
            assert abs(sg["adaptor"]["delta"] - so["adaptor"]["delta"]) < 1e-6
        g.set_state(sg)
        g.run(k, i, n_adapts, i_first=i)
        st_g, zg, eg = g.stats(), g.phasepoint(), g.get_stepsize()
        for off, o in zip(offsets, os_):
            o.run(k, i, n_adapts, i_first=i)
            sl = slice(off, off + n)
            st_o, zo = o.stats(), o.phasepoint()
            sub = {key: v[sl] for key, v in st_g.items()}
            same = compare_transition_stats(sub, st_o, dtype, o, f"cfg4 {name}/{metric} D={D} iteration {i} offset {off}")
            np.testing.assert_allclose(zg.theta[:, sl][:, same], zo.theta[:, same], rtol=tol, atol=tol)
            np.testing.assert_allclose(zg.r[:, sl][:, same], zo.r[:, same], rtol=tol, atol=tol)
            np.testing.assert_allclose(zg.lp.gradient[:, sl][:, same], zo.lp.gradient[:, same], rtol=tol, atol=tol * 10)
            np.testing.assert_allclose(eg[sl][same], o.get_stepsize()[same], rtol=1e-9 if dtype == np.float64 else 1e-4, err_msg=f"ϵ after adapt! {i}")
            depth_seen = max(depth_seen, int(st_o["tree_depth"].max()))
    assert depth_seen >= 5, depth_seen   # trees of 32+ leaves: merges on several pending levels, compaction of finished chains
    # what ran: the 64×64-tile GEMM, two pipelines, the point-pool tree kernel
    assert g.info("dense_gemm_launches") + g.info("dense_gemm_small_launches") > 0 and g.info("dense_pipelines") == 2 and g.info("dense_pool") == 1
    assert (g.info("dense_epoch_launches") > 0) == (engine != "step")
    g.close()
    for o in os_:
        o.close()


def test_dense_epoch_kernel_equals_step_synchronous_kernels(hip, monkeypatch):
    """`k_dense_epoch` (chain-complete workgroups: both products, the second half-step and the speculative next one in the epilogue,
    four chains per wave in the tree phase) against `k_dgemm` + `k_d_tree2` on the HIP engine: the same 2 304 chains through a
    3-iteration warm-up (StepSizeAdaptor inside the kernel) and 3 draws kept on the device, trees up to the maximum depth —
    every chain takes the same number of leapfrogs in every transition and ends at the same point (the products accumulate in
    the same order; only the sums r·v, θ·g, ρ·v are added in another order: 1e-9).  Also with a chain count that leaves the
    last workgroup partly empty, with an epoch that ends in the middle of the trees (chunks of 5 steps), and with SliceTS on one
    pipeline, and at D = 256 (the kernel's other instantiation).  The epoch engine keeps g′, w′ of a point on record only where a leapfrog can start from it and begins every transition with
    the motionless step (`lazy_gw`) — the step-synchronous kernels of the batch's tail included."""
    import torch

    rs = np.random.default_rng(2025)
    mats = {}
    for D in (512, 256):
        idx = np.arange(D)
        P = np.asfortranarray(np.linalg.inv(0.9 ** np.abs(idx[:, None] - idx[None, :])))
        Q, _ = np.linalg.qr(rs.normal(size=(D, D)))
        Minv = (Q * np.linspace(0.6, 2.0, D)) @ Q.T
        mats[D] = (P, np.asfortranarray((Minv + Minv.T) / 2))
    # (D, N, chunk, sampler, dtype, AHMC_DENSE_EPOCH_NCT): round 6 — k_dense_epoch2 at D = 384 (six waves per workgroup, a ragged last chunk in
    # the vector passes) and 768 (twelve), in Float32 (v_mfma_f32_16x16x4_f32, two 32-chain workgroups per CU), and the 16-chain shape of D = 512
    cases = ((512, 2304, None, A.MultinomialTS, np.float64, None), (512, 2090, "5", A.MultinomialTS, np.float64, None),
             (512, 1100, None, A.SliceTS, np.float64, None), (256, 1300, None, A.MultinomialTS, np.float64, None),
             (512, 1200, None, A.MultinomialTS, np.float64, "1"), (512, 1100, None, A.MultinomialTS, np.float64, "2"),
             (384, 1100, None, A.MultinomialTS, np.float64, None),
             (512, 1300, None, A.MultinomialTS, np.float32, None), (512, 1100, "5", A.SliceTS, np.float32, "1"),
             (256, 1100, None, A.MultinomialTS, np.float32, None), (384, 1100, None, A.MultinomialTS, np.float32, None),
             (768, 1100, None, A.MultinomialTS, np.float32, None),
             (1024, 600, None, A.MultinomialTS, np.float32, None),   # sixteen waves per workgroup
             # TemperedLeapfrog (src/integrator.jl:198-209) in the epilogues and the speculative half-step: round 4's kernel, k_dense_epoch2, Float32
             (512, 1100, None, A.MultinomialTS, np.float64, None, 1.05), (384, 1100, "5", A.MultinomialTS, np.float64, None, 1.03),
             (512, 1100, None, A.SliceTS, np.float32, None, 1.05),
             # ClassicNoUTurn / StrictGeneralisedNoUTurn (src/trajectory.jl:551-557,579-617) in the epoch kernel's tree phase (k_dense_epoch2<…, CRIT>)
             (512, 1100, None, A.MultinomialTS, np.float64, None, None, A.ClassicNoUTurn), (512, 1100, "5", A.SliceTS, np.float64, None, None, A.StrictGeneralisedNoUTurn),
             (512, 1100, None, A.MultinomialTS, np.float32, None, 1.04, A.StrictGeneralisedNoUTurn), (512, 1100, None, A.MultinomialTS, np.float32, None, None, A.ClassicNoUTurn))
    for D, N, chunk, sampler, dtype, nct, *rest in cases:
        temper = [rest[0]] if rest and rest[0] else []
        TC = rest[1] if len(rest) > 1 else A.GeneralisedNoUTurn
        if D not in mats:
            idx = np.arange(D)
            Pm = np.asfortranarray(np.linalg.inv(0.9 ** np.abs(idx[:, None] - idx[None, :])))
            Q, _ = np.linalg.qr(rs.normal(size=(D, D)))
            Mi = (Q * np.linspace(0.6, 2.0, D)) @ Q.T
            mats[D] = (Pm, np.asfortranarray((Mi + Mi.T) / 2))
        P, Minv = mats[D]
        f32 = dtype == np.float32
        th0 = np.asfortranarray(rs.normal(size=(D, N)))
        eps0 = 0.12 * (0.7 + 0.6 * rs.random(N))
        out = {}
        for engine in ("step", "epoch"):
            monkeypatch.setenv("AHMC_DENSE_EPOCH", "1" if engine == "epoch" else "0")
            monkeypatch.setenv("AHMC_DENSE_EPOCH_MIN", "32")
            for var, val in (("AHMC_DENSE_CHUNK", chunk), ("AHMC_DENSE_EPOCH_NCT", nct), ("AHMC_DENSE_EPOCH_V", "2" if nct else None)):
                if val:
                    monkeypatch.setenv(var, val)
                else:
                    monkeypatch.delenv(var, raising=False)
            lf = A.TemperedLeapfrog(eps0, temper[0]) if temper else A.Leapfrog(eps0)
            k = A.HMCKernel(A.Trajectory(sampler, lf, TC(max_depth=10, delta_max=1000.0)))
            g = A.Engine(A.Hamiltonian(A.DenseEuclideanMetric(Minv), A.DenseGaussian(P)), N, dtype=dtype, rng=A.PhiloxRNG(78), lib=hip)
            g.set_integrator(lf)
            g.set_position(th0)
            g.adaptor_init(A.StepSizeAdaptor(0.8, lf))
            draws = torch.empty((3, N, D), dtype=torch.float32 if f32 else torch.float64, device="cuda")
            g.run(k, 6, 3, drop_warmup=True, samples_out=draws.data_ptr())
            g.sync()
            st, acc = g.stats(), g.accum()
            out[engine] = (draws.cpu().numpy(), st["n_steps"].copy(), acc["total_n_steps"], g.get_stepsize().copy(), st["acceptance_rate"].copy(), g.theta().copy())
            assert (g.info("dense_epoch_launches") > 0) == (engine == "epoch"), (D, dtype, engine)
            g.close()
        a, b = out["step"], out["epoch"]
        if not f32:
            np.testing.assert_array_equal(a[1], b[1])
            assert a[2] == b[2]
            np.testing.assert_allclose(a[3], b[3], rtol=1e-9)
            np.testing.assert_allclose(a[4], b[4], rtol=1e-6, atol=1e-12)   # (mean of exp(−ΔH): a rounding of ΔH ≈ 500 is a relative 1e-9 of it)
            np.testing.assert_allclose(a[0], b[0], rtol=1e-9, atol=1e-9)
            np.testing.assert_allclose(a[5], b[5], rtol=1e-9, atol=1e-9)
        else:
            # Float32: the two engines add r·v, θ·g, ρ·v in another order — 1e-7 per sum, 6 free-running transitions with dual averaging
            # in between: a handful of chains part ways at a tie (they end O(1) apart); every other chain agrees to single precision
            same = a[1] == b[1]
            on = same & np.isclose(a[5], b[5], rtol=2e-3, atol=2e-3).all(axis=0)
            assert on.mean() >= 0.97, (D, on.mean())
            np.testing.assert_allclose(a[3][on], b[3][on], rtol=1e-3)
            np.testing.assert_allclose(a[0][:, on, :], b[0][:, on, :], rtol=1e-2, atol=1e-2)   # (three draws of trees of up to 1 023 single-precision leapfrogs)


def test_fixed_integration_time_hmcda(hip, oracle, rng):
    """FixedIntegrationTime(λ) (src/trajectory.jl:240-243; the HMCDA sampler of src/constructors.jl): nsteps =
    max(1, floor(λ / ϵ_nominal)) with ONE nominal step size — scalar ϵ for many chains; a single chain's own adapted ϵ"""
    D, N = 12, 300
    h = A.Hamiltonian(make_metric("diag_chain", D, N, rng), A.IsoGaussian(D))
    th = rng.normal(size=(D, N))
    for lam, eps, L in ((1.0, 0.1, 10), (0.95, 0.3, 3), (0.05, 0.2, 1)):    # floor(1.0/0.1) = 10, floor(3.17) = 3, max(1, 0) = 1
        lf = A.Leapfrog(eps)
        k = A.HMCKernel(A.Trajectory(A.EndPointTS, lf, A.FixedIntegrationTime(lam)))
        g, o = pair(hip, oracle, h, N, np.float64, seed=21, lf=lf)
        for e in (g, o):
            e.set_position(th)
        for _ in range(3):
            for e in (g, o):
                e.transition(k)
            sg, so = g.stats(), o.stats()
            assert (sg["n_steps"] == L).all() and (so["n_steps"] == L).all()
            same = compare_transition_stats(sg, so, np.float64, o, f"hmcda λ={lam}")
            zg, zo = g.phasepoint(), o.phasepoint()
            np.testing.assert_allclose(zg.theta[:, same], zo.theta[:, same], rtol=1e-8, atol=1e-8)
            realign(g, o, same)
        g.close(); o.close()
    # a vector of step sizes is the reference's error (Q6), on both engines
    for lib in (hip, oracle):
        e = A.Engine(h, N, rng=1, lib=lib)
        e.set_integrator(A.Leapfrog(np.full(N, 0.1)))
        e.set_position(th)
        with pytest.raises(A.ArgumentError):
            e.transition(A.HMCKernel(A.Trajectory(A.EndPointTS, A.Leapfrog(np.full(N, 0.1)), A.FixedIntegrationTime(1.0))))
        e.close()
    # HMCDA proper: ONE chain, λ fixed, ϵ adapted by dual averaging — L follows the adapted ϵ (sample loop, bulk driver)
    h1 = A.Hamiltonian(A.DiagEuclideanMetric(np.ones(D)), A.IsoGaussian(D))
    res = []
    for lib in (hip, oracle):
        e = A.Engine(h1, 1, rng=5, lib=lib)
        lf = A.Leapfrog(0.05)
        e.set_integrator(lf)
        e.set_position(th[:, 0])
        e.adaptor_init(A.StepSizeAdaptor(0.8, lf))
        k = A.HMCKernel(A.Trajectory(A.EndPointTS, lf, A.FixedIntegrationTime(1.0)))
        ns = []
        for i in range(1, 41):
            e.run(k, i, 30, i_first=i)
            ns.append(int(e.stats()["n_steps"][0]))
        res.append((ns, e.get_stepsize()[0], e.theta().copy()))
        e.close()
    assert res[0][0] == res[1][0] and len(set(res[0][0])) > 2, res[0][0]     # L changed as ϵ adapted, identically
    np.testing.assert_allclose(res[0][1], res[1][1], rtol=1e-8)
    np.testing.assert_allclose(res[0][2], res[1][2], rtol=1e-6, atol=1e-8)


JIT_EXIT = dict(D=8, N=32, L=400, jitter=0.5, seed=3, marginal={3: 1.8, 11: 1.95, 20: 2.2, 27: 2.5})


def jittered_exit_case():
    """static EndPointTS on the unit-metric iso-Gaussian (the leapfrog's stability limit is ϵ = 2) with four chains whose NOMINAL step
    sizes sit on both sides of that limit and a jitter of ±50 %: whether, and after how many of the L steps, such a chain leaves the
    finite numbers depends on the step size the transition actually uses"""
    c = JIT_EXIT
    rs = np.random.default_rng(5)
    eps = 0.2 * (0.7 + 0.6 * rs.random(c["N"]))
    for ch, e in c["marginal"].items():
        eps[ch] = e
    th = rs.normal(size=(c["D"], c["N"]))
    h = A.Hamiltonian(A.UnitEuclideanMetric((c["D"], c["N"])), A.IsoGaussian(c["D"]))
    stable = np.ones(c["N"], dtype=bool)
    stable[list(c["marginal"])] = False
    return h, eps, th, stable


def compat_stop_step(oracle, h, lf, th, L, seed, iteration, stable):
    """how many leapfrog steps a ref_compat static EndPointTS transition of the ORACLE took (L: no chain left the finite numbers): the
    transition is run, then its momentum draw is repeated (`refresh` at the same iteration), and a second engine steps every chain
    with the step size the transition reports until the stable, accepted chains stand where the transition left them.  Returns
    (steps, the transition's statistics, its end positions)."""
    N = th.shape[1]
    e = A.Engine(h, N, dtype=np.float64, rng=A.PhiloxRNG(seed, iteration=iteration), lib=oracle)
    e.set_integrator(lf)
    e.set_ref_compat(True)
    e.set_position(th)
    e.transition(A.HMCKernel(A.Trajectory(A.EndPointTS, lf, A.FixedNSteps(L))))
    st, end = e.stats(), e.theta()
    e.close()
    m = A.Engine(h, N, dtype=np.float64, rng=A.PhiloxRNG(seed, iteration=iteration), lib=oracle)
    m.set_integrator(A.Leapfrog(st["step_size"]))
    m.set_position(th)
    m.refresh()
    on = stable & st["is_accept"]
    assert on.sum() >= 8, on.sum()
    taken = None
    for k in range(1, L + 1):
        m.step(1)
        if np.allclose(m.theta()[:, on], end[:, on], rtol=1e-12, atol=1e-12):
            taken = k
            break
    m.close()
    assert taken is not None
    return taken, st, end


def test_reference_batch_exit_compat_mode_jittered(hip, oracle):
    """`ahmc_set_ref_compat` with a JitteredLeapfrog: the dry run that finds the coupled stop step integrates with the step size the
    transition itself uses (the RNG_JITTER draw of its iteration), not the nominal one.  Not vacuous: on the oracle alone, the stop step
    under the jittered integrator differs from the one a plain Leapfrog(ϵ_nom) gives for the same configuration, in both iterations.
    Then HIP == oracle with this file's comparison: the n_steps statistic (the nominal L) and the end state of every chain."""
    c = JIT_EXIT
    h, eps, th, stable = jittered_exit_case()
    N, L = c["N"], c["L"]
    lf = A.JitteredLeapfrog(eps, c["jitter"])
    kern = A.HMCKernel(A.Trajectory(A.EndPointTS, lf, A.FixedNSteps(L)))
    for it in (0, 1):
        stop_j, so_ref, end_ref = compat_stop_step(oracle, h, lf, th, L, c["seed"], it, stable)
        stop_n, _, _ = compat_stop_step(oracle, h, A.Leapfrog(eps), th, L, c["seed"], it, stable)
        print(f"iteration {it}: the oracle stops after {stop_j} of {L} steps with the jittered step sizes, after {stop_n} with the nominal ones")
        assert stop_j != stop_n and min(stop_j, stop_n) < L, (it, stop_j, stop_n)
        assert np.ptp(so_ref["step_size"] / eps) > 0.5          # the jitter is there
        g, o = (A.Engine(h, N, dtype=np.float64, rng=A.PhiloxRNG(c["seed"], iteration=it), lib=lib) for lib in (hip, oracle))
        for e in (g, o):
            e.set_integrator(lf)
            e.set_ref_compat(True)
            e.set_position(th)
            e.transition(kern)
        sg, so = g.stats(), o.stats()
        np.testing.assert_array_equal(o.theta(), end_ref)
        same = compare_transition_stats(sg, so, np.float64, o, f"static hmc, jittered batch exit, iteration {it}")
        assert (sg["n_steps"] == L).all() and (so["n_steps"] == L).all()
        np.testing.assert_allclose(sg["step_size"], so["step_size"], rtol=1e-12)
        assert same[stable].all(), np.flatnonzero(~same)
        zg, zo = g.phasepoint(), o.phasepoint()
        # every chain: the stable ones to the file's tolerance; a chain beyond the stability limit has grown by up to 1e150 and is held
        # on its finiteness pattern and, where finite, to the same RELATIVE tolerance (no absolute one means anything at that size)
        np.testing.assert_allclose(zg.theta[:, same & stable], zo.theta[:, same & stable], rtol=1e-9, atol=1e-9)
        np.testing.assert_array_equal(np.isfinite(zg.theta), np.isfinite(zo.theta))
        np.testing.assert_array_equal(np.isfinite(zg.lp.value), np.isfinite(zo.lp.value))
        fin = np.isfinite(zo.theta)
        np.testing.assert_allclose(zg.theta[fin], zo.theta[fin], rtol=1e-6)
        g.close(); o.close()


def test_reference_batch_exit_compat_mode(hip, oracle, rng):
    """(ABI v6) `ahmc_set_ref_compat`: the reference's MATRIX-MODE early exit — `step` ends the integration of every chain at the first step
    after which ANY chain's phase point is non-finite (src/integrator.jl:252-258 with isfinite over all columns, src/hamiltonian.jl:141-142;
    SURVEY quirk Q1) — on the HIP engine against the oracle's literal form of it, for step(lf, h, z, n) both ways and for static EndPointTS
    transitions; and off (the default) each chain stops at its own first non-finite point on both sides."""
    D, N = 6, 200
    h = A.Hamiltonian(make_metric("diag_chain", D, N, rng), A.IsoGaussian(D))
    eps = np.full(N, 0.2)
    eps[17] = 1e160          # one chain blows up at its second step (θ ≈ 1e160·r, ℓπ overflows at the next gradient)
    th, r = rng.normal(size=(D, N)), rng.normal(size=(D, N))
    for compat in (True, False):
        g, o = pair(hip, oracle, h, N, np.float64, seed=4, eps=eps)
        for e in (g, o):
            e.set_ref_compat(compat)
            e.set_position(th, r)
            e.step(9)
        zg, zo = g.phasepoint(), o.phasepoint()
        ok = np.arange(N) != 17
        np.testing.assert_allclose(zg.theta[:, ok], zo.theta[:, ok], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(zg.r[:, ok], zo.r[:, ok], rtol=1e-9, atol=1e-9)
        np.testing.assert_array_equal(np.isfinite(zg.lp.value), np.isfinite(zo.lp.value))
        assert not np.isfinite(zo.lp.value[17]) or not np.isfinite(zo.lk.value[17])
        # how far did the OTHER chains get: a chain of the harmonic oscillator after k steps of 0.2 from (θ, r)
        ref = A.Engine(h, N, rng=4, lib=oracle)
        ref.set_integrator(A.Leapfrog(np.full(N, 0.2)))
        ref.set_position(th, r)
        taken = None
        for k in range(1, 10):
            ref.step(1)
            if np.allclose(ref.phasepoint().theta[:, ok], zo.theta[:, ok], rtol=1e-9, atol=1e-9):
                taken = k
                break
        assert taken is not None and (taken < 9 if compat else taken == 9), (compat, taken)   # coupled: everybody stopped with chain 17
        # static EndPointTS transitions: the same coupling inside transition (the dry run finds the step, k_hmc integrates that far)
        kern = A.HMCKernel(A.Trajectory(A.EndPointTS, A.Leapfrog(eps), A.FixedNSteps(7)))
        for e in (g, o):
            e.set_position(th)
        for _ in range(3):
            for e in (g, o):
                e.transition(kern)
            sg, so = g.stats(), o.stats()
            same = compare_transition_stats(sg, so, np.float64, o, f"static hmc, batch exit compat={compat}")
            assert (sg["n_steps"] == 7).all()
            np.testing.assert_allclose(g.phasepoint().theta[:, same & ok], o.phasepoint().theta[:, same & ok], rtol=1e-9, atol=1e-9)
            realign(g, o, same)
        g.close(); o.close(); ref.close()
