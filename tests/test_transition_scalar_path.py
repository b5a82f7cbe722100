"""The once-per-transition code of k_nuts where one chain owns one wave (G = 64; TSC in k_nuts, csrc/ahmc_nuts.hpp): the chain index
lives in scalar registers, per-chain addresses are a 64-bit scalar base plus the lane's 32-bit byte offset
(load_vec / store_vec <…, SB>, csrc/ahmc_device.hpp), and the kernel-argument fields of the prologue and the epilogue are read where
they are used.  None of it touches an arithmetic expression, so everything here is BIT FOR BIT: the fused launches (several transitions
per launch, adapt! inside the kernel, the draws written by the kernel) against the one-transition-per-call path (`transition` + `adapt`,
whose launches have n_trans = 1, no dispatch order and no draws buffer) — θ, every statistic, step sizes, M⁻¹ and the draws buffer.

Shapes: where addressing can go wrong.  D = 127 / 65: the last lane with an element is half out of range, the lanes behind it wholly
(D = 65: 31 of them), and with an odd D every other chain's slice starts off the 16-byte grid (the ragged arm of load_vec / store_vec in
every lane); D = 128: every lane full.  D = 256 / 512: E = 4 / 8, two / four 16-byte pieces per lane.  The step sizes START in descending
order of the chain index, so the first fused launch's dispatch order (ascending step size) is the reversed one and every later launch
follows a launch with a non-identity order; the per-call path has none.

N = 3 and N = 5 — fewer chains than a workgroup has waves — put waves out of range only where a workgroup HAS several waves, and by default
it has one (AHMC_NUTS_WPB, csrc/ahmc_api.hip: plan_nuts; the library reads it once per process).  In this process the small N only make
short grids.  test_waves_out_of_range_in_four_wave_workgroups runs the same cases in a fresh child process with AHMC_NUTS_WPB=4: 256-thread
workgroups, N = 3 leaves one wave of the only workgroup and N = 5 three waves of the second one behind the last chain (they shadow chain 0
and must not write), and the waves 1 … 3 of a workgroup take their scratch and LDS bases from a non-zero wave index.

Launches: 12 adapting transitions in two launches of 6 and 6 draws in one launch of 6 with a device draws buffer (n_trans > 1 with
samples_out).  The Stan window is 2 … 11: its end — the M⁻¹ and √M⁻¹ stores, the Welford reset, the dual-averaging restart — lies INSIDE
the second warm-up launch.  (A launch of 6 adapting transitions alone cannot hold a window end that updates the metric: the variance
estimator wants ten samples, WelfordVar's n_min.)
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:   # (run as the child process of test_waves_out_of_range_in_four_wave_workgroups)
    sys.path.insert(0, ROOT)

import ahmc_amd as A  # noqa: E402

pytestmark = pytest.mark.gpu

ENV = ("AHMC_NORMALS_TAIL", "AHMC_NORMALS_TAIL_ROWS", "AHMC_NORMALS_PREFETCH", "AHMC_NORMALS_PREFETCH_MAX_MB", "AHMC_NUTS_BATCH", "AHMC_NUTS_DRAW_BATCH",
       "AHMC_NUTS_SCHED", "AHMC_NUTS_NO_ORDER", "AHMC_NUTS_ORDER_REFRESH", "AHMC_NUTS_FIRST_BATCH", "AHMC_GEOMETRY")
N_ADAPTS, N_DRAWS, LAUNCH = 12, 6, 6


def _clean_env(monkeypatch, batch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("AHMC_NUTS_BATCH", str(batch))
    monkeypatch.setenv("AHMC_NUTS_DRAW_BATCH", str(batch))


def _engine(lib, D, N, dtype, seed, eps):
    rng = np.random.default_rng(seed)
    metric = A.DiagEuclideanMetric(np.asfortranarray(0.5 + rng.random((D, N))))   # per-chain M⁻¹: the (D, N) loads of the prologue
    h = A.Hamiltonian(metric, A.IsoGaussian(D))
    lf = A.Leapfrog(np.asarray(eps, dtype=np.float64))
    e = A.Engine(h, N, dtype=dtype, rng=A.PhiloxRNG(seed), lib=lib)
    e.set_integrator(lf)
    e.set_position(np.asfortranarray(0.5 * rng.normal(size=(D, N))))
    return e, metric, lf


def _kernel(lf, max_depth=8):
    return A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=max_depth, delta_max=1000.0)))


def _to_host(t):
    return t.cpu().numpy()


def _step_sizes(D, N):
    return 0.25 * D ** -0.25 * np.linspace(1.3, 0.8, N)   # descending: the dispatch order by step size is the reversed one


def _run_both(lib, D, N, dtype):
    """the fused launches and the one-transition-per-call path on the engine `lib` (launch lengths from the environment): what each leaves"""
    import torch

    eps = _step_sizes(D, N)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    res = {}
    for which in ("fused", "step"):
        e, metric, lf = _engine(lib, D, N, dtype, 0x5EED0011, eps)
        minv0 = np.array(e.get_metric())
        k = _kernel(lf)
        e.adaptor_init(A.StanHMCAdaptor(A.MassMatrixAdaptor(metric), A.StepSizeAdaptor(0.8, lf), init_buffer=1, term_buffer=1, window_size=10))
        if which == "fused":
            draws_d = torch.zeros((N_DRAWS, N, D), dtype=tdt, device="cuda")
            e.run(k, N_ADAPTS + N_DRAWS, N_ADAPTS, drop_warmup=True, samples_out=draws_d)
            e.sync()
            draws = _to_host(draws_d).transpose(2, 1, 0)   # (D, N, draw)
            launches = (e.info("nuts_warm_launches"), e.info("nuts_launches"))
        else:
            draws = np.zeros((D, N, N_DRAWS), dtype=dtype)
            for i in range(1, N_ADAPTS + N_DRAWS + 1):
                e.transition(k)
                e.adapt(i, N_ADAPTS)
                if i > N_ADAPTS:
                    draws[:, :, i - N_ADAPTS - 1] = e.theta()
            launches = None
        res[which] = {"theta": np.array(e.theta()), "stats": e.stats(), "eps": np.array(e.get_stepsize()), "minv": np.array(e.get_metric()),
                      "minv0": minv0, "draws": draws, "geom": (e.info("group_lanes"), e.info("elems_per_lane")), "launches": launches}
        e.close()
    return res


def _assert_same(a, b, what):
    np.testing.assert_array_equal(a["theta"], b["theta"], err_msg=what + ": θ")
    np.testing.assert_array_equal(a["eps"], b["eps"], err_msg=what + ": ϵ")
    np.testing.assert_array_equal(a["minv"], b["minv"], err_msg=what + ": M⁻¹")
    np.testing.assert_array_equal(a["draws"], b["draws"], err_msg=what + ": the draws buffer")
    assert set(a["stats"]) == set(b["stats"]) and len(a["stats"]) >= 5
    for f in a["stats"]:
        np.testing.assert_array_equal(a["stats"][f], b["stats"][f], err_msg=what + ": " + f)


def _check(res, D, N, geom, dtype, on_device):
    a, b = res["fused"], res["step"]
    what = f"D={D} N={N} {np.dtype(dtype).name}"
    if on_device:
        assert a["geom"] == geom and b["geom"] == geom, (what, a["geom"], b["geom"])
        assert a["launches"] == (N_ADAPTS // LAUNCH, N_DRAWS // LAUNCH), (what, a["launches"])   # n_trans = 6 in every fused launch
    assert np.isfinite(b["theta"]).all() and np.isfinite(b["draws"]).all(), what
    assert (b["stats"]["n_steps"] >= 1).all(), what
    # the window end must have stored a NEW M⁻¹ for every element of every chain, and dual averaging moved every step size
    assert (b["minv"] != b["minv0"]).all() and (a["minv"] != a["minv0"]).all(), what + ": the warm-up must have replaced M⁻¹"
    assert (b["eps"] != _step_sizes(D, N).astype(dtype)).all(), what + ": the warm-up must have adapted ϵ"
    _assert_same(a, b, what)
    np.testing.assert_array_equal(a["draws"][:, :, -1], a["theta"], err_msg=what + ": last draw == θ")


SHAPES = [(127, 3, (64, 2)), (128, 5, (64, 2)), (65, 5, (64, 2)), (256, 3, (64, 4)), (512, 5, (64, 8))]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D,N,geom", SHAPES)
def test_fused_launches_equal_one_transition_per_call(hip, monkeypatch, D, N, geom, dtype):
    _clean_env(monkeypatch, LAUNCH)
    _check(_run_both(hip, D, N, dtype), D, N, geom, dtype, hip.backend == "hip:gfx950")


# (D, N, dtype) of the child process: every geometry with N = 3 or 5, and the store type
WPB4_CASES = [(127, 3, "float64"), (128, 5, "float64"), (65, 5, "float32"), (256, 3, "float64"), (512, 5, "float64")]


def _child_main(out_path):
    """the body of the child process (AHMC_NUTS_WPB=4 in its environment from the start): the cases of WPB4_CASES, fused against per call
    in THIS process; what the fused runs leave goes to `out_path` for the parent to hold against its own one-wave-per-workgroup runs"""
    lib = A.load_hip_library()
    assert lib.backend == "hip:gfx950" and os.environ.get("AHMC_NUTS_WPB") == "4"
    keep = {}
    for D, N, dt in WPB4_CASES:
        dtype = np.dtype(dt).type
        geom = next(g for d, n, g in SHAPES if (d, n) == (D, N))
        res = _run_both(lib, D, N, dtype)
        _check(res, D, N, geom, dtype, True)
        for f in ("theta", "eps", "minv", "draws"):
            keep[f"{D}_{N}_{f}"] = res["fused"][f]
        keep[f"{D}_{N}_n_steps"] = res["fused"]["stats"]["n_steps"]
    np.savez(out_path, **keep)
    print("WPB4 CHILD OK", len(WPB4_CASES))


def test_waves_out_of_range_in_four_wave_workgroups(hip, monkeypatch, tmp_path):
    """N = 3 and N = 5 in workgroups of FOUR waves (see the module's docstring): a fresh process with AHMC_NUTS_WPB=4 runs the fused launches
    against the per-call path bit for bit, and its results equal this process's, whose workgroups have one wave — chains do not depend on
    how the grid is cut."""
    _clean_env(monkeypatch, LAUNCH)
    env = dict(os.environ, AHMC_NUTS_WPB="4")
    out = str(tmp_path / "wpb4.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "WPB4 CHILD OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    got = np.load(out)
    for D, N, dt in WPB4_CASES:
        here = _run_both(hip, D, N, np.dtype(dt).type)["fused"]
        for f in ("theta", "eps", "minv", "draws"):
            np.testing.assert_array_equal(got[f"{D}_{N}_{f}"], here[f], err_msg=f"D={D} N={N} {dt}: {f}, four waves per workgroup against one")
        np.testing.assert_array_equal(got[f"{D}_{N}_n_steps"], here["stats"]["n_steps"])


def test_draws_buffer_above_4_gib(hip, monkeypatch):
    """N = 4 096, D = 128, 1 100 draws written by ONE launch into a device buffer of 4.3 GiB: the draw of transition kt of chain c starts
    (kt·N + c)·D elements into it — 2^32 bytes at kt = 1 024 — a base the kernel forms on the scalar unit in 64 bits.  The last draw
    must be θ; draw 1 023 (the last one wholly below the 4 GiB offset) and draw 1 024 (the first one at it) must be the per-call
    run's θ after as many transitions, bit for bit.  Short trees (max_depth 3): the test is about addresses."""
    import torch

    D, N, K = 128, 4096, 1100
    LO, HI = (1 << 32) // (D * N * 8) - 1, (1 << 32) // (D * N * 8)   # 1023, 1024
    assert (HI * N * D) * 8 == 1 << 32 and K > HI + 1
    _clean_env(monkeypatch, K)
    monkeypatch.setenv("AHMC_NUTS_SCHED", "0")
    eps = np.linspace(0.45, 0.3, N)
    e, metric, lf = _engine(hip, D, N, np.float64, 0x5EED0012, eps)
    k = _kernel(lf, max_depth=3)
    draws_d = torch.zeros((K, N, D), dtype=torch.float64, device="cuda")
    e.run(k, K, 0, samples_out=draws_d)
    e.sync()
    theta = np.array(e.theta())
    n_launches, geom = e.info("nuts_launches"), (e.info("group_lanes"), e.info("elems_per_lane"))
    e.close()
    last, lo, hi = (_to_host(draws_d[j]).T for j in (K - 1, LO, HI))
    del draws_d
    if hip.backend == "hip:gfx950":
        assert geom == (64, 2) and n_launches == 1, (geom, n_launches)
    np.testing.assert_array_equal(last, theta, err_msg="last draw == θ")
    e, metric, lf = _engine(hip, D, N, np.float64, 0x5EED0012, eps)
    k = _kernel(lf, max_depth=3)
    for i in range(HI + 1):
        e.transition(k)
        if i == LO:
            np.testing.assert_array_equal(lo, e.theta(), err_msg=f"draw {LO}: the last one below the 4 GiB offset")
    np.testing.assert_array_equal(hi, e.theta(), err_msg=f"draw {HI}: the first one at the 4 GiB offset")
    assert np.isfinite(hi).all() and not np.array_equal(hi, lo)
    e.close()


if __name__ == "__main__":
    _child_main(sys.argv[1])
