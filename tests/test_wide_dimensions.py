"""Wide contexts: D > 4096 (or AHMC_FORCE_WIDE=1 at ahmc_create) on the step-synchronous engine, no fused-kernel geometry.

The reference takes any D (src/metric.jl:52-72,89-120 and the whole trajectory path).  Beyond the largest fused geometry (512, 8) a
context is WIDE: G = E = 0, every call runs on the step-synchronous engine, and the built-in families are evaluated by k_w_target
(advancedhmc.jl_amd/csrc/ahmc_wide.hpp) for the listed chains only.  Held here:
  * CPU: the shipped code object holds the eight k_w_target instantiations, none with scratch;
  * creation at D = 4097 / 5000 / 8192 reports AHMC_INFO_WIDE = 1 (D = 4096 keeps its fused geometry);
  * every element of θ, r and g after ahmc_leapfrog against an exact numpy leapfrog at D = 5000 — the elements beyond 4096 included;
  * the oracle, under the margin rule of tests/parity_util.py, at D = 5000 and 8192: every family × Unit / Diag with NUTS, and at
    D = 5000 the other samplers, criteria, integrators, partial refreshment, find_good_stepsize, StanHMCAdaptor, KernelTarget,
    ExternalTarget (ask / tell) and Float32;
  * AHMC_FORCE_WIDE=1 at D = 128 / 600 / 4096 against the fused kernels on the same seeds;
  * bit-for-bit invariances on the wide path: bulk run == stepwise, checkpoint → resume, one engine == two engines over a chain split;
  * the refusals (dense metric, dense target, target plugin, ahmc_set_ref_compat) and a valid transition after each.
"""
import os

import numpy as np
import pytest

import ahmc_amd as A
import parity_util as PU
from ahmc_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UT = os.path.join(ROOT, "tests", "user_targets")
LOG2PI = 1.8378770664093454835606594728112
WIDE_KERNELS = [f"k_w_target<{t}, {k}>" for t in ("float", "double") for k in range(4)]


# ---------------------------------------------------------------------------------------------------------------------
# CPU side
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="needs llvm-objdump")
def test_wide_target_kernels_are_shipped_without_scratch():
    """the built library's gfx950 code object holds every k_w_target<T, TK> (f32 / f64 × iso, diag, funnel, hier), each with
    zero private-segment bytes (a spill would put the one-pass family evaluation on scratch)"""
    import subprocess
    import sys

    from ahmc_amd import build as B

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_meta
    finally:
        sys.path.pop(0)
    assert os.path.exists(B.OUT), "build() first"
    meta = kernel_meta.kernel_meta(B.OUT)
    names = [k["name"] for k in meta]
    demangled = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    found = {}
    for k, dn in zip(meta, demangled):
        for w in WIDE_KERNELS:
            if dn.startswith(f"void ahmc::{w}("):
                found[w] = k
    assert sorted(found) == sorted(WIDE_KERNELS), sorted(found)
    for w, k in found.items():
        assert k["private_segment_fixed_size"] == 0, (w, k)
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, (w, k)


# ---------------------------------------------------------------------------------------------------------------------
# GPU side
# ---------------------------------------------------------------------------------------------------------------------
def make_target(name, D, rng):
    if name == "iso":
        return A.IsoGaussian(D)
    if name == "diag":
        return A.DiagGaussian(rng.normal(size=D), 0.5 + rng.random(D))
    if name == "funnel":
        return A.Funnel(D)
    return A.HierGaussian(D)


def make_metric(name, D, N, rng):
    if name == "unit":
        return A.UnitEuclideanMetric((D, N))
    if name == "diag_shared":
        return A.DiagEuclideanMetric(0.5 + rng.random(D))
    return A.DiagEuclideanMetric(np.asfortranarray(0.5 + rng.random((D, N))))


def engines(hip, oracle, h, N, dtype, lf, seed):
    out = []
    for lib in (hip, oracle):
        e = A.Engine(h, N, dtype=dtype, rng=A.PhiloxRNG(seed), lib=lib)
        e.set_integrator(lf)
        out.append(e)
    return out


def compare(g, o, dtype, what):
    from test_gpu_parity import compare_transition_stats

    same = compare_transition_stats(g.stats(), o.stats(), dtype, o, what)
    zg, zo = g.phasepoint(), o.phasepoint()
    if dtype == np.float64:  # (Float32: a near-tie in the CHOICE of the candidate moves θ and leaves every discrete statistic alone — the
        # continuous statistics are held on the chains without one inside compare_transition_stats, as in test_gpu_parity.py)
        np.testing.assert_allclose(zg.theta[:, same], zo.theta[:, same], rtol=1e-8, atol=1e-8, err_msg=what)
        np.testing.assert_allclose(zg.lp.gradient[:, same], zo.lp.gradient[:, same], rtol=1e-8, atol=1e-8, err_msg=what + " grad")
    th = zo.theta
    g.set_position(th)
    o.set_position(th)
    return same


def eps_for(D, target):
    return (0.1 if target == "funnel" else 0.3) * D ** -0.25


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D", [4097, 5000, 8192])
def test_create_wide(hip, dtype, D):
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((D, 4)), A.IsoGaussian(D)), 4, dtype=dtype, rng=1, lib=hip)
    assert (e.info("wide"), e.info("group_lanes"), e.info("elems_per_lane")) == (1, 0, 0)
    e.close()
    f = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((4096, 4)), A.IsoGaussian(4096)), 4, dtype=dtype, rng=1, lib=hip)
    assert (f.info("wide"), f.info("group_lanes"), f.info("elems_per_lane")) == (0, 512, 8)  # the default routing at D <= 4096
    f.close()


@pytest.mark.gpu
def test_leapfrog_covers_every_element(hip):
    """D = 5000, diagonal Gaussian with its own (m, s) per dimension and a per-chain M⁻¹: θ, r and g of EVERY element after
    ahmc_leapfrog(n) against an exact numpy leapfrog (round 6's wide contexts kept the fused geometry, and the elements from
    4096 on never moved)"""
    D, N, n = 5000, 6, 7
    rs = np.random.default_rng(50)
    m, s = rs.normal(size=D), 0.5 + rs.random(D)
    minv = np.asfortranarray(0.5 + rs.random((D, N)))
    eps = 0.05 * (0.8 + 0.4 * rs.random(N))
    th, r = rs.normal(size=(D, N)), rs.normal(size=(D, N))
    e = A.Engine(A.Hamiltonian(A.DiagEuclideanMetric(minv), A.DiagGaussian(m, s)), N, rng=3, lib=hip)
    assert e.info("wide") == 1
    e.set_integrator(A.Leapfrog(eps))
    e.set_position(th, r)
    e.step(n)
    z = e.phasepoint()
    mm, s2 = m[:, None], (s * s)[:, None]
    grad = lambda t: (t - mm) / s2  # noqa: E731  (−∇ℓπ)
    for _ in range(n):
        r = r - eps / 2 * grad(th)
        th = th + eps * minv * r
        r = r - eps / 2 * grad(th)
    lp = (-(LOG2PI + 2 * np.log(s)[:, None] + (mm - th) ** 2 / s2) / 2).sum(axis=0)
    np.testing.assert_allclose(z.theta, th, rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(z.r, r, rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(z.lp.gradient, grad(th), rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(z.lp.value, lp, rtol=1e-11)
    np.testing.assert_allclose(z.lk.value, -(r * minv * r).sum(axis=0) / 2, rtol=1e-11)
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("D", [5000, 8192])
@pytest.mark.parametrize("target", ["iso", "diag", "funnel", "hier"])
@pytest.mark.parametrize("metric", ["unit", "diag_chain"])
def test_nuts_families_against_oracle(hip, oracle, D, target, metric):
    N = 64
    rs = np.random.default_rng(D + len(target))
    h = A.Hamiltonian(make_metric(metric, D, N, rs), make_target(target, D, rs))
    lf = A.Leapfrog(np.full(N, eps_for(D, target)) * (0.8 + 0.4 * rs.random(N)))
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=6)))
    g, o = engines(hip, oracle, h, N, np.float64, lf, 9)
    assert g.info("wide") == 1
    th = 0.5 * rs.normal(size=(D, N))
    for e in (g, o):
        e.set_position(th)
    for it in range(2):
        for e in (g, o):
            e.transition(k)
        compare(g, o, np.float64, f"wide nuts D={D} {target} {metric} it {it}")


VARIANTS = ["slice", "classic", "strict", "hmc_endpoint", "hmc_multinomial_time", "jittered", "tempered", "partial"]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_variants_against_oracle(hip, oracle, variant):
    D, N = 5000, 64
    rs = np.random.default_rng(7)
    eps = eps_for(D, "hier")
    h = A.Hamiltonian(make_metric("diag_shared", D, N, rs), make_target("hier", D, rs))
    lf = {"jittered": A.JitteredLeapfrog(eps, 0.2), "tempered": A.TemperedLeapfrog(eps, 1.05)}.get(variant, A.Leapfrog(eps))
    tau = {"slice": A.Trajectory(A.SliceTS, lf, A.GeneralisedNoUTurn(max_depth=6)),
           "classic": A.Trajectory(A.MultinomialTS, lf, A.ClassicNoUTurn(max_depth=6)),
           "strict": A.Trajectory(A.MultinomialTS, lf, A.StrictGeneralisedNoUTurn(max_depth=6)),
           "hmc_endpoint": A.Trajectory(A.EndPointTS, lf, A.FixedNSteps(8)),
           "hmc_multinomial_time": A.Trajectory(A.MultinomialTS, lf, A.FixedIntegrationTime(8.5 * eps))}.get(
        variant, A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=6)))
    k = A.HMCKernel(A.PartialMomentumRefreshment(0.4), tau) if variant == "partial" else A.HMCKernel(tau)
    g, o = engines(hip, oracle, h, N, np.float64, lf, 21)
    th = 0.5 * rs.normal(size=(D, N))
    for e in (g, o):
        e.set_position(th)
    for it in range(2):
        for e in (g, o):
            e.transition(k)
        compare(g, o, np.float64, f"wide {variant} it {it}")


@pytest.mark.gpu
def test_find_good_stepsize_and_stan_adaptor_against_oracle(hip, oracle):
    D, N, n_adapts = 5000, 64, 16
    rs = np.random.default_rng(11)
    metric = A.DiagEuclideanMetric(np.ones((D, N), order="F"))
    h = A.Hamiltonian(metric, make_target("diag", D, rs))
    lf = A.Leapfrog(np.full(N, 0.1))
    g, o = engines(hip, oracle, h, N, np.float64, lf, 33)
    th = 0.5 * rs.normal(size=(D, N))
    for e in (g, o):
        e.set_position(th)
    PU.reset_margin(o)
    eg, eo = g.find_good_stepsize(), o.find_good_stepsize()
    PU.check_equal_or_near_tie(eg, eo, PU.decision_margin(o), np.float64, "wide find_good_stepsize")
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=6)))
    ad = A.StanHMCAdaptor(A.MassMatrixAdaptor(metric), A.StepSizeAdaptor(0.8, lf), init_buffer=2, term_buffer=2, window_size=12)
    for e in (g, o):  # (one slow window of 12 draws, 3 … 14: the Welford estimate needs 10, so M⁻¹ is updated at its end)
        e.set_integrator(A.Leapfrog(eo))
        e.set_position(th)
        e.adaptor_init(ad)
    for i in range(1, n_adapts + 1):  # one iteration per chunk from the oracle's state: adapt! doubles a rounding every iteration
        g.set_state(o.get_state())
        for e in (g, o):
            e.run(k, i, n_adapts, i_first=i)
        sg, so = g.get_state(), o.get_state()
        assert sg["adaptor"] == so["adaptor"]
        stg, sto = g.stats(), o.stats()
        same = (stg["n_steps"] == sto["n_steps"]) & (stg["tree_depth"] == sto["tree_depth"]) & (stg["numerical_error"] == sto["numerical_error"])
        on = same & np.isclose(sg["theta"], so["theta"], rtol=1e-8, atol=1e-8).all(axis=0)
        on = PU.check_flips(on, PU.decision_margin(o), np.float64, f"wide stan iteration {i}", n_steps=sto["n_steps"])
        np.testing.assert_allclose(sg["stepsize"][on], so["stepsize"][on], rtol=1e-8, err_msg=f"ϵ after adapt! {i}")
        np.testing.assert_allclose(sg["metric"][:, on], so["metric"][:, on], rtol=1e-8, atol=1e-12, err_msg=f"M⁻¹ after adapt! {i}")
    assert not np.allclose(o.get_state()["metric"], 1.0)  # a window end updated M⁻¹


@pytest.mark.gpu
def test_kernel_target_against_oracle(hip, oracle):
    import torch

    from ahmc_amd.build import build_code_object
    from ahmc_amd.hipmod import Module
    from test_user_targets import host_kernel

    D, N = 5000, 64
    rs = np.random.default_rng(5)
    mod = Module(build_code_object(os.path.join(UT, "kernels.hip")))
    user = torch.tensor([0.0, 0.0], dtype=torch.float64, device="cuda")
    fn = lambda th: (-(th * th).sum(axis=0) / 2 - th.shape[0] * LOG2PI / 2, -th)  # noqa: E731
    minv = np.asfortranarray(0.5 + rs.random((D, N)))
    lf = A.Leapfrog(np.full(N, eps_for(D, "iso")))
    tg = A.KernelTarget(D, mod.function("iso_gauss_f64"), handle_kind=capi.KERNEL_HIP_FUNCTION, block_threads=256, chains_per_block=4, user=user.data_ptr())
    to = A.KernelTarget(D, host_kernel(fn), handle_kind=capi.KERNEL_HOST)
    g = A.Engine(A.Hamiltonian(A.DiagEuclideanMetric(minv), tg), N, rng=A.PhiloxRNG(8), lib=hip)
    o = A.Engine(A.Hamiltonian(A.DiagEuclideanMetric(minv), to), N, rng=A.PhiloxRNG(8), lib=oracle)
    assert g.info("wide") == 1
    th = 0.5 * rs.normal(size=(D, N))
    for e in (g, o):
        e.set_integrator(lf)
        e.set_position(th)
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=6)))
    for it in range(2):
        for e in (g, o):
            e.transition(k)
        compare(g, o, np.float64, f"wide kernel target it {it}")
    g.close(); o.close()


@pytest.mark.gpu
def test_external_target_against_oracle(hip, oracle):
    """ask / tell (ahmc_ext_*) and the split-step pair ahmc_lf_pre / ahmc_lf_post with the routed kinetic energy"""
    D, N = 5000, 64
    rs = np.random.default_rng(6)
    fn = lambda th: (-(th * th).sum(axis=0) / 2 - th.shape[0] * LOG2PI / 2, -th)  # noqa: E731
    minv = np.asfortranarray(0.5 + rs.random((D, N)))
    lf = A.Leapfrog(np.full(N, eps_for(D, "iso")))
    g = A.Engine(A.Hamiltonian(A.DiagEuclideanMetric(minv), A.ExternalTarget(D, fn)), N, rng=A.PhiloxRNG(4), lib=hip)
    o = A.Engine(A.Hamiltonian(A.DiagEuclideanMetric(minv), A.IsoGaussian(D)), N, rng=A.PhiloxRNG(4), lib=oracle)
    assert g.info("wide") == 1
    th, r = 0.5 * rs.normal(size=(D, N)), rs.normal(size=(D, N))
    for e in (g, o):
        e.set_integrator(lf)
        e.set_position(th, r)
    np.testing.assert_allclose(g.phasepoint().lk.value, o.phasepoint().lk.value, rtol=1e-10)
    for e in (g, o):
        e.step(3)
    zg, zo = g.phasepoint(), o.phasepoint()
    np.testing.assert_allclose(zg.theta, zo.theta, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(zg.lk.value, zo.lk.value, rtol=1e-9)
    for e in (g, o):
        e.set_position(th)
    for kk in (A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=6))),
               A.HMCKernel(A.Trajectory(A.EndPointTS, lf, A.FixedNSteps(5)))):
        for e in (g, o):
            e.transition(kk)
        compare(g, o, np.float64, "wide external target")
    g.close(); o.close()


@pytest.mark.gpu
def test_float32_against_oracle(hip, oracle):
    D, N = 5000, 128
    rs = np.random.default_rng(12)
    h = A.Hamiltonian(make_metric("diag_chain", D, N, rs), make_target("diag", D, rs))
    lf = A.Leapfrog(np.full(N, eps_for(D, "diag")))
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=6)))
    g, o = engines(hip, oracle, h, N, np.float32, lf, 13)
    assert g.info("wide") == 1
    th = 0.5 * rs.normal(size=(D, N))
    for e in (g, o):
        e.set_position(th)
    for it in range(2):
        for e in (g, o):
            e.transition(k)
        compare(g, o, np.float32, f"wide f32 it {it}")


@pytest.mark.gpu
@pytest.mark.parametrize("D,target", [(128, "funnel"), (600, "hier"), (4096, "diag")])
def test_forced_wide_against_fused(hip, oracle, monkeypatch, D, target):
    """AHMC_FORCE_WIDE=1 (read at ahmc_create) against the fused kernels on the same seeds: a chain may differ only where the
    oracle, on the same inputs, took a decision within the margin bound of a tie"""
    N = 128
    rs = np.random.default_rng(D)
    h = A.Hamiltonian(make_metric("diag_chain", D, N, rs), make_target(target, D, rs))
    lf = A.Leapfrog(np.full(N, eps_for(D, target)))
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=7)))
    monkeypatch.setenv("AHMC_FORCE_WIDE", "1")
    w = A.Engine(h, N, rng=A.PhiloxRNG(17), lib=hip)
    monkeypatch.delenv("AHMC_FORCE_WIDE")
    f = A.Engine(h, N, rng=A.PhiloxRNG(17), lib=hip)
    o = A.Engine(h, N, rng=A.PhiloxRNG(17), lib=oracle)
    assert (w.info("wide"), f.info("wide")) == (1, 0)
    th = 0.5 * rs.normal(size=(D, N))
    for e in (w, f, o):
        e.set_integrator(lf)
        e.set_position(th)
    for it in range(3):
        for e in (w, f, o):
            e.transition(k)
        sw, sf = w.stats(), f.stats()
        same = (sw["n_steps"] == sf["n_steps"]) & (sw["is_accept"] == sf["is_accept"]) & (sw["numerical_error"] == sf["numerical_error"])
        same = PU.check_flips(same, PU.decision_margin(o), np.float64, f"forced wide vs fused D={D} {target} it {it}")
        np.testing.assert_allclose(w.phasepoint().theta[:, same], f.phasepoint().theta[:, same], rtol=1e-8, atol=1e-8)
        np.testing.assert_allclose(sw["hamiltonian_energy"][same], sf["hamiltonian_energy"][same], rtol=1e-8, atol=1e-8)
        th = o.phasepoint().theta
        for e in (w, f, o):
            e.set_position(th)


def _wide_setup(N, seed=3):
    D = 5000
    rs = np.random.default_rng(seed)
    metric = A.DiagEuclideanMetric(np.ones((D, N), order="F"))
    h = A.Hamiltonian(metric, A.HierGaussian(D))
    lf = A.Leapfrog(np.full(N, eps_for(D, "hier")))
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=6)))
    ad = A.StanHMCAdaptor(A.MassMatrixAdaptor(metric), A.StepSizeAdaptor(0.8, lf), init_buffer=3, term_buffer=2, window_size=3)
    return D, h, lf, k, ad, 0.5 * rs.normal(size=(D, N))


@pytest.mark.gpu
def test_wide_bulk_equals_stepwise_and_resume(hip):
    """bit for bit: ahmc_sample (warm-up + batched draws) == per-iteration calls; get_state → set_state on a fresh engine resumes"""
    N, n, n_adapts, cut = 64, 14, 8, 10
    D, h, lf, k, ad, th = _wide_setup(N)
    a, b, c = (A.Engine(h, N, rng=A.PhiloxRNG(5), lib=hip) for _ in range(3))
    for e in (a, b, c):
        e.set_integrator(lf)
        e.set_position(th)
        e.adaptor_init(ad)
    out = np.zeros((D, N, n - n_adapts), order="F")
    a.run(k, n, n_adapts, drop_warmup=True, samples_out=out)
    a.sync()
    for i in range(1, n + 1):
        b.transition(k)
        b.adapt(i, n_adapts)
        if i > n_adapts:
            np.testing.assert_array_equal(out[:, :, i - n_adapts - 1], b.theta(), err_msg=f"draw {i}")
    c.run(k, cut, n_adapts)
    st = c.get_state()
    c.close()
    d = A.Engine(h, N, rng=A.PhiloxRNG(5), lib=hip)
    d.set_integrator(lf)
    d.adaptor_init(ad)
    d.set_position(th)
    d.set_state(st)
    d.run(k, n, n_adapts, i_first=cut + 1)
    np.testing.assert_array_equal(d.theta(), b.theta())
    np.testing.assert_array_equal(d.get_stepsize(), b.get_stepsize())
    for e in (a, b, d):
        e.close()


@pytest.mark.gpu
def test_wide_chain_split_equals_one_engine(hip):
    """one engine over N chains == two engines over a random split of them (each with its chains' Philox offsets), bit for bit"""
    N = 96
    D, h, lf, k, _, th = _wide_setup(N, seed=4)
    rs = np.random.default_rng(8)
    eps = np.full(N, eps_for(D, "hier")) * (0.8 + 0.4 * rs.random(N))
    full = A.Engine(h, N, rng=A.PhiloxRNG(9), lib=hip)
    full.set_integrator(A.Leapfrog(eps))
    full.set_position(th)
    full.run(k, 3)
    cut = int(rs.integers(10, N - 10))
    for lo, hi in ((0, cut), (cut, N)):
        n = hi - lo
        hs = A.Hamiltonian(A.DiagEuclideanMetric(np.ones((D, n), order="F")), A.HierGaussian(D))
        e = A.Engine(hs, n, rng=A.PhiloxRNG(9, chain_offset=lo), lib=hip)
        e.set_integrator(A.Leapfrog(eps[lo:hi]))
        e.set_position(th[:, lo:hi])
        e.run(k, 3)
        np.testing.assert_array_equal(e.theta(), full.theta()[:, lo:hi], err_msg=f"chains {lo}..{hi}")
        e.close()
    full.close()


@pytest.mark.gpu
def test_wide_refusals(hip):
    D, N = 5000, 16
    rs = np.random.default_rng(2)
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((D, N)), A.IsoGaussian(D)), N, rng=1, lib=hip)
    e.set_integrator(A.Leapfrog(np.full(N, eps_for(D, "iso"))))
    e.set_position(rs.normal(size=(D, N)))
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, A.Leapfrog(0.1), A.GeneralisedNoUTurn(max_depth=4)))
    refusals = [
        lambda: e.set_metric(A.DenseEuclideanMetric(np.eye(2))),
        lambda: e.set_target(A.DenseGaussian(np.eye(2))),
        lambda: e.set_target(A.PluginTarget(D, os.path.join(UT, "iso_gauss.hpp"))),
        lambda: e._call("ahmc_set_ref_compat", 1),
    ]
    for ref in refusals:
        with pytest.raises(capi.UnsupportedError, match="4096"):
            ref()
        e.transition(k)
        st = e.stats()
        assert (st["n_steps"] >= 1).all() and np.isfinite(st["hamiltonian_energy"]).all()
    e.close()
