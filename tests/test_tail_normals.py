"""The momentum normals of a k_nuts launch made in the TAIL of the launch before it (AHMC_NORMALS_TAIL; csrc/ahmc_sample_host.hpp:
tail_normals_plan, csrc/ahmc_nuts.hpp: the waves behind the chain waves of the G = 64 sampling / warm-up kernels).

The normals are a pure function of (seed, chain, iteration, element) — rand_momentum, src/metric.jl:290-309, on the Philox stream of
csrc/ahmc_device.hpp — so WHO makes them (k_normals in front of the launch, or the appended waves of the launch before) is not
allowed to show in any result: every comparison here is bit for bit, between AHMC_NORMALS_TAIL=0 and =2 (the tail for every launch
length; the default, 1, takes only launches above AHMC_NORMALS_PREFETCH_MAX_MB, which no quick test reaches).

k_normals itself (rewritten by rows) against the CPU oracle: test_k_normals_rows_against_oracle below — tests/test_gpu_parity.py::
test_refresh_momentum covers `refresh`, whose kernel draws its normals itself and never calls k_normals.
"""
import numpy as np
import pytest

import ahmc_amd as A

pytestmark = pytest.mark.gpu

ENV = ("AHMC_NORMALS_TAIL", "AHMC_NORMALS_TAIL_ROWS", "AHMC_NORMALS_PREFETCH", "AHMC_NORMALS_PREFETCH_MAX_MB", "AHMC_NUTS_BATCH", "AHMC_NUTS_DRAW_BATCH",
       "AHMC_NUTS_SCHED", "AHMC_NUTS_NO_ORDER", "AHMC_NUTS_ORDER_REFRESH", "AHMC_NUTS_FIRST_BATCH")
N_ADAPTS, N_DRAWS = 12, 20
STATS = ("n_steps", "acceptance_rate", "hamiltonian_energy", "tree_depth", "numerical_error")


def _engine(lib, D, N, target, dtype, seed):
    metric = A.DiagEuclideanMetric(np.ones((D, N), order="F"))
    h = A.Hamiltonian(metric, {"iso": A.IsoGaussian, "hier": A.HierGaussian, "funnel": A.Funnel}[target](D))
    lf = A.Leapfrog(np.full(N, 0.1))
    e = A.Engine(h, N, dtype=dtype, rng=A.PhiloxRNG(seed), lib=lib)
    e.set_integrator(lf)
    e.set_position(np.asfortranarray(np.random.default_rng(seed).random((D, N))))
    # n_adapts = 12: init buffer 1, one window 2..11 — ten samples, the fewest a variance estimate is taken from (WelfordVar's n_min);
    # its end updates M⁻¹ and restarts the dual averaging —, term buffer 1
    ad = A.StanHMCAdaptor(A.MassMatrixAdaptor(metric), A.StepSizeAdaptor(0.8, lf), init_buffer=1, term_buffer=1, window_size=10)
    return e, lf, ad


def _run(lib, monkeypatch, tail, D, N, target="iso", dtype=np.float64, alpha=0.0, again=False, extra=None):
    """warm-up + draws in ragged launches (12 adapting transitions in launches of 4, 20 draws in launches of 3 and 2: the hint a launch is
    given is the length of the one that follows or longer, and the last warm-up launch has none), then everything a run leaves behind"""
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("AHMC_NORMALS_TAIL", str(tail))
    monkeypatch.setenv("AHMC_NUTS_BATCH", "5")
    monkeypatch.setenv("AHMC_NUTS_DRAW_BATCH", "3")
    for kk, vv in (extra or {}).items():
        monkeypatch.setenv(kk, vv)
    e, lf, ad = _engine(lib, D, N, target, dtype, 0x5EED0008)
    tau = A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=8, delta_max=1000.0))
    k = A.HMCKernel(A.PartialMomentumRefreshment(alpha), tau) if alpha else A.HMCKernel(tau)
    e.find_good_stepsize()
    e.adaptor_init(ad)
    out = np.zeros((D, N, N_DRAWS), order="F", dtype=dtype)
    e.run(k, N_ADAPTS + N_DRAWS, N_ADAPTS, drop_warmup=True, samples_out=out)
    e.sync()
    res = {"draws": out, "stepsize": e.get_stepsize(), "metric": e.get_metric(), "stats": e.stats(), "accum": e.accum(),
           "geom": (e.info("group_lanes"), e.info("elems_per_lane")), "hits": e.info("norm_tail_hits")}
    if again:
        # the same engine again: one transition on its own moves the iteration counter past anything a tail could have prepared, then
        # a second run whose first launch has no predecessor
        e.transition(k)
        out2 = np.zeros((D, N, 8), order="F", dtype=dtype)
        e.run(k, 8, 0, samples_out=out2)
        e.sync()
        res.update(draws2=out2, stats2=e.stats(), accum2=e.accum(), hits2=e.info("norm_tail_hits"))
    e.close()
    return res


def _assert_same(a, b, what):
    np.testing.assert_array_equal(a["draws"], b["draws"], err_msg=f"{what}: draws")
    np.testing.assert_array_equal(a["stepsize"], b["stepsize"], err_msg=f"{what}: step sizes")
    np.testing.assert_array_equal(a["metric"], b["metric"], err_msg=f"{what}: metric")
    for sk, ak in (("stats", "accum"), ("stats2", "accum2")):
        if sk not in a:
            continue
        for f in STATS:
            np.testing.assert_array_equal(a[sk][f], b[sk][f], err_msg=f"{what}: {sk} {f}")
        for f in ("total_n_steps", "n_transitions", "n_divergent"):
            assert a[ak][f] == b[ak][f], (what, ak, f)
        np.testing.assert_array_equal(a[ak]["sum_theta"], b[ak]["sum_theta"], err_msg=f"{what}: {ak} Σθ")
        np.testing.assert_array_equal(a[ak]["sumsq_theta"], b[ak]["sumsq_theta"], err_msg=f"{what}: {ak} Σθ²")
    if "draws2" in a:
        np.testing.assert_array_equal(a["draws2"], b["draws2"], err_msg=f"{what}: draws of the second run")


# (D, N, target, dtype, geometry): odd D (33 pairs, the last one half); cfg2's geometry with N no multiple of anything; E = 4; E = 8; the store type
SHAPES = [(65, 3, "iso", np.float64, (64, 2)), (128, 130, "iso", np.float64, (64, 2)), (130, 5, "hier", np.float64, (64, 4)),
          (511, 2, "iso", np.float64, (64, 8)), (128, 7, "iso", np.float32, (64, 2))]


@pytest.mark.parametrize("D,N,target,dtype,geom", SHAPES)
def test_tail_normals_leave_the_chains_untouched(hip, monkeypatch, D, N, target, dtype, geom):
    """warm-up + draws with the next launch's normals made in every launch's tail == the same run with k_normals in front of every
    launch: draws, step sizes, metric, statistics, accumulators, bit for bit.  On the device the tail path must have RUN (hit counter)."""
    real = hip.backend == "hip:gfx950"
    again = (D, N) == (65, 3)
    ref = _run(hip, monkeypatch, 0, D, N, target, dtype, again=again)
    got = _run(hip, monkeypatch, 2, D, N, target, dtype, again=again)
    assert not real or (ref["geom"] == geom and got["geom"] == geom), (ref["geom"], got["geom"])
    assert np.isfinite(ref["draws"]).all() and np.abs(ref["metric"] - 1).max() > 1e-3, "the run must have adapted the metric"
    _assert_same(got, ref, f"D={D} N={N} {target}")
    if real:
        # 3 warm-up launches of 4: two of them hand normals on; 7 draws launches: six do
        print(f"D={D} N={N}: norm_tail_hits {got['hits']} with AHMC_NORMALS_TAIL=2, {ref['hits']} with =0")
        assert ref["hits"] == 0 and got["hits"] >= 6, (ref["hits"], got["hits"])
        if again:
            # the second run (8 draws: launches of 3, 3, 2) hits twice more — never in its first launch, whose iteration nothing prepared
            assert ref["hits2"] == 0 and 0 < got["hits2"] - got["hits"] <= 2, (got["hits"], got["hits2"])


def test_tail_normals_other_row_counts(hip, monkeypatch):
    """the rows a tail wave takes (AHMC_NORMALS_TAIL_ROWS) only cut the job differently: 1 row per wave, and more rows than the job has"""
    ref = _run(hip, monkeypatch, 0, 65, 3)
    for rows in ("1", "7", "100000"):
        got = _run(hip, monkeypatch, 2, 65, 3, extra={"AHMC_NORMALS_TAIL_ROWS": rows})
        _assert_same(got, ref, f"rows per tail wave {rows}")
        if hip.backend == "hip:gfx950":
            assert got["hits"] >= 6


def test_partial_refreshment_declines_the_tail(hip, monkeypatch):
    """PartialMomentumRefreshment(0.3): the normals are mixed with the stored momentum inside k_nuts, neither way of making them ahead of
    time applies — results equal, no hit"""
    ref = _run(hip, monkeypatch, 0, 65, 3, alpha=0.3)
    got = _run(hip, monkeypatch, 2, 65, 3, alpha=0.3)
    _assert_same(got, ref, "refresh_alpha = 0.3")
    assert got["hits"] == 0 and ref["hits"] == 0


def test_shared_wave_geometry_ignores_the_switch(hip, monkeypatch):
    """D = 32: four chains share a wave (G = 16), whose kernels have no tail job — AHMC_NORMALS_TAIL=2 changes nothing and counts nothing"""
    ref = _run(hip, monkeypatch, 0, 32, 9, target="funnel")
    got = _run(hip, monkeypatch, 2, 32, 9, target="funnel")
    assert hip.backend != "hip:gfx950" or got["geom"] == (16, 2), got["geom"]
    _assert_same(got, ref, "D = 32 (G = 16)")
    assert got["hits"] == 0 and ref["hits"] == 0


@pytest.mark.parametrize("D,N", [(65, 3), (128, 130)])
def test_k_normals_rows_against_oracle(hip, oracle, D, N):
    """k_normals by rows, element by element against the CPU oracle: ONE NUTS transition of depth 1 from θ = 0 with ϵ = 1e-6 under a unit
    metric.  The iso-Gaussian gradient at 0 is 0, so whichever of the tree's two points is chosen, its momentum is the freshly drawn r0
    up to a factor 1 − ϵ²/2 (5e-13): the stored momentum IS the launch's normals.  Tolerance: the parity suite's 1e-8
    (tests/test_gpu_parity.py) — a misplaced, missing or repeated element is off by O(1)."""
    h = A.Hamiltonian(A.UnitEuclideanMetric((D, N)), A.IsoGaussian(D))
    lf = A.Leapfrog(np.full(N, 1e-6))
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=1, delta_max=1000.0)))
    r = []
    for lib in (hip, oracle):
        e = A.Engine(h, N, dtype=np.float64, rng=A.PhiloxRNG(0x5EED0009), lib=lib)
        e.set_integrator(lf)
        e.set_position(np.zeros((D, N), order="F"))
        e.transition(k)
        r.append(np.array(e.phasepoint().r))
        e.close()
    assert r[0].shape == (D, N) and np.abs(r[1]).min() > 0 and 0.7 < r[1].std() < 1.3
    np.testing.assert_allclose(r[0], r[1], rtol=1e-8, atol=1e-8)
