"""bench.py's output contract (one JSON line, the keys the driver and the judge read) on a reduced workload, and its
launcher: `--gpus N` must create N ranks."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_flag_spawns_that_many_ranks():
    """`bench.py --gpus 2` outside a torchrun environment re-executes itself under torch.distributed.run with two
    ranks (round 1 parsed the flag and ignored it).  --launch-check stops after the rendezvous (gloo, no GPU, no
    engine): rank 0 reports the world it saw."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launch-check"], capture_output=True, text=True,
                         timeout=300, cwd=ROOT, env=env)
    assert res.returncode == 0, res.stdout + res.stderr[-2000:]
    lines = [l for l in res.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["ranks_seen"] == 2 and d["gpus_requested"] == 2
    # one rank: no respawn
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--launch-check"], capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert res.returncode == 0 and json.loads(res.stdout.strip().splitlines()[-1])["n_gpus"] == 1
    # a torchrun world that disagrees with --gpus is an error, not a silently different run
    env2 = dict(env, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launch-check"], capture_output=True, text=True, timeout=120,
                         cwd=ROOT, env=env2)
    assert res.returncode != 0


def _run_bench(extra, tmp_path, timeout=900):
    detail = str(tmp_path / "detail.json")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--detail", detail] + extra
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout
    # what the driver does: the LAST line of stdout is the record, and it must fit its capture (round 4's 31.9 KB line did not)
    assert res.stdout.strip().splitlines()[-1] == lines[0]
    assert len(lines[0]) < 6000, len(lines[0])
    return json.loads(lines[0]), json.load(open(detail))


def _check_headline(d, steps, warmup, chains, n_adapts, n_draws):
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["steps"] == steps and d["warmup"] == warmup and d["n_gpus"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["dtype"] == "f64" and d["data"] == "synthetic" and d["vs_baseline"] is None
    c = d["config"]
    assert "workload" in c and c["n_adapts"] == n_adapts and c["n_draws"] == n_draws
    # value = leapfrogs of BOTH phases / the whole loop's wall time (adaptation inside the timed region); 6 significant digits in the line
    total = (c["warmup_phase"]["mean_leapfrogs_per_transition"] * c["n_adapts"] + c["post_adaptation"]["mean_leapfrogs_per_transition"] * c["n_draws"]) * chains
    assert abs(d["ms_per_step"] * d["steps"] / 1e3 * d["value"] - total) < 1e-4 * total
    assert abs(c["leapfrogs"]["adapt"] + c["leapfrogs"]["draw"] - total) < 1e-4 * total
    assert c["post_adaptation"]["value"] > 0 and c["warmup_phase"]["value"] > 0
    assert c["ess_per_sec"] > 0
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel"):
        assert k in r, k
    assert r["bound"] == "valu" and r["peak"] > 0
    if r["frac"] is not None:   # counters at HEAD present for this workload size only
        assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-4 and r["frac"] <= 1.0
    assert r["dominant"]["hbm_model_frac"] > 0 and r["dominant"]["avg_launch_ms"] > 0 and r["dominant"]["launches"] > 0
    b = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in b, k
    assert b["kind"] == "port" and b["value"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["cfg2", "cfg3"])
def test_bench_json_contract(config, tmp_path):
    d, full = _run_bench(["--full", "--config", config, "--steps", "4", "--warmup", "1", "--transitions-per-step", "20", "--chains", "4096",
                          "--cpu-chains", "64", "--cpu-transitions", "24", "--repeats", "2"], tmp_path)
    _check_headline(d, 4, 1, 4096, 40, 40)
    assert len(d["config"]["runs"]) == 2 and d["cpu_baseline"]["single_thread_value"] > 0
    assert "secondary" not in d["config"]
    # the side file holds the FULL record the line was made from
    assert d["config"]["detail"] and full["value"] == pytest.approx(d["value"], rel=1e-5)
    assert full["config"]["gathered_draws"] == 40 * 4096 and full["config"]["ess"]["ess_per_sec"] == pytest.approx(d["config"]["ess_per_sec"], rel=1e-5)
    assert full["cpu_baseline"]["single_thread"]["value"] > 0


@pytest.mark.gpu
def test_bench_default_invocation_line(tmp_path):
    """`python bench.py --full` with no --config, on reduced chains: ONE line under 6 000 characters that carries the
    headline AND config.secondary.{cfg3, cfg5, cfg4}, each with value / ms_per_step / steps / workload / dtype / roofline / cpu_baseline.
    (Round 4: this invocation was never tested, its line grew to 31.9 KB and the driver's 8 KB capture lost the headline.)"""
    d, full = _run_bench(["--full", "--steps", "4", "--warmup", "1", "--transitions-per-step", "20", "--chains", "2048", "--cpu-chains", "64",
                          "--cpu-transitions", "24", "--repeats", "1"], tmp_path, timeout=1500)
    _check_headline(d, 4, 1, 2048, 40, 40)
    sec = d["config"]["secondary"]
    assert sorted(sec) == ["cfg3", "cfg4", "cfg5"]
    for name, o in sec.items():
        assert "error" not in o, (name, o)
        for k in ("value", "ms_per_step", "steps", "workload", "dtype", "roofline", "cpu_baseline"):
            assert k in o, (name, k)
        assert o["value"] > 0 and o["dtype"] == "f64" and name in o["workload"]
        for k in ("bound", "frac", "achieved", "peak", "traffic", "kernel"):
            assert k in o["roofline"], (name, k)
        assert o["roofline"]["bound"] == ("mfma" if name == "cfg4" else "valu")
        assert o["cpu_baseline"]["value"] > 0 and o["cpu_baseline"]["kind"] == "port" and o["cpu_baseline"]["cores"] >= 1
        assert o["ess_per_sec"] is not None and o["ess_per_sec"] > 0     # the second half of BASELINE's metric, every config
        assert full["config"]["secondary"][name]["value"] == pytest.approx(o["value"], rel=1e-5)
    assert sec["cfg4"]["roofline"]["achieved"] > 0


def _dump_once(bench, A, lib, out_dir):
    import numpy as np
    import torch

    cfg = dict(bench.CONFIGS["cfg2"], D=8)
    N, n_adapts, n_draws, T = 96, 10, 12, 5
    eng, kernel = bench.build_engine(A, lib, cfg, N, cfg["seed"], 0)
    draws = torch.empty((n_draws, N, cfg["D"]), dtype=torch.float64)
    bench.sample_loop(eng, kernel, n_adapts, n_draws, eng.sync, draws_ptr=draws.data_ptr())
    names = bench.dump_outputs(str(out_dir), eng, draws, n_draws, T, np.float64)
    theta = eng.theta()
    eng.close()
    return names, theta


def test_dump_outputs_on_the_cpu_checker(oracle, tmp_path):
    """--dump-outputs' writer on the CPU checker (same C ABI as the HIP engine): float32 / float64 files only, under the budget, the
    last step's draws of the sampled chains end in their final θ, and the same arguments write the same arrays twice"""
    import numpy as np

    sys.path.insert(0, ROOT)
    import importlib

    import ahmc_amd as A

    bench = importlib.import_module("bench")
    names, theta = _dump_once(bench, A, oracle, tmp_path / "a")
    names2, _ = _dump_once(bench, A, oracle, tmp_path / "b")
    assert names == names2
    for k in ("draws_last_step", "draws_chains", "stat_n_steps", "stat_log_density", "stat_chains", "stepsize", "metric"):
        assert k in names, k
    total = 0
    for name in names:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.testing.assert_array_equal(a, b, err_msg=name)
        total += (tmp_path / "a" / f"{name}.npy").stat().st_size
    assert total <= bench.DUMP_BUDGET
    d = np.load(tmp_path / "a" / "draws_last_step.npy")
    pick = np.load(tmp_path / "a" / "draws_chains.npy").astype(np.int64)
    assert d.shape == (5, len(pick), 8)
    np.testing.assert_array_equal(d[-1], theta[:, pick].T)
    assert np.load(tmp_path / "a" / "metric.npy").shape == (8, len(pick))


@pytest.mark.gpu
def test_bench_plain_run_and_dump_outputs(tmp_path):
    """A plain run (no --full): ONE timed run of exactly --steps steps and the headline keys, none of what --full adds (CPU baseline,
    ESS, secondary configs, side file); --dump-outputs writes float32 / float64 arrays under the budget, the same ones on a second run
    with the same arguments"""
    import numpy as np

    sys.path.insert(0, ROOT)
    import importlib

    bench = importlib.import_module("bench")
    lines = []
    for run in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--transitions-per-step", "20",
               "--chains", "4096", "--dump-outputs", str(tmp_path / run)]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert res.returncode == 0, res.stderr[-2000:]
        lines.append(json.loads(res.stdout.strip().splitlines()[-1]))
    d = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "roofline"):
        assert k in d, k
    assert d["steps"] == 4 and d["warmup"] == 1 and d["dtype"] == "f64" and d["higher_is_better"] is True and d["unit"] == "leapfrog-steps/s"
    c = d["config"]
    assert len(c["runs"]) == 1 and c["n_adapts"] == 40 and c["n_draws"] == 40
    assert "cpu_baseline" not in d and "secondary" not in c and "ess_per_sec" not in c and "detail" not in c
    total = (c["warmup_phase"]["mean_leapfrogs_per_transition"] * c["n_adapts"] + c["post_adaptation"]["mean_leapfrogs_per_transition"] * c["n_draws"]) * 4096
    assert abs(d["ms_per_step"] * d["steps"] / 1e3 * d["value"] - total) < 1e-4 * total
    names = sorted(f for f in os.listdir(tmp_path / "a") if f.endswith(".npy"))
    assert names == sorted(f for f in os.listdir(tmp_path / "b") if f.endswith(".npy"))
    assert "draws_last_step.npy" in names and "stat_n_steps.npy" in names
    assert sum((tmp_path / "a" / f).stat().st_size for f in names) <= bench.DUMP_BUDGET
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64), (f, a.dtype)
        np.testing.assert_array_equal(a, b, err_msg=f)
    assert np.load(tmp_path / "a" / "draws_last_step.npy").shape[:1] == (20,)


def _stub_full_record():
    """a full default-invocation record as bench.py builds it (round 4's own: the 31.9 KB one the driver could not hold)"""
    return json.load(open(os.path.join(ROOT, "profiles", "r4_bench_default_line.json")))


def test_default_line_stays_under_the_drivers_capture():
    """compact_line on a full default-invocation record: < 6 000 characters, every key of the contract, the three secondary configs;
    and a record that grew (longer texts, more runs) still comes out under the budget — the line sheds optional fields, never grows"""
    sys.path.insert(0, ROOT)
    import importlib

    bench = importlib.import_module("bench")
    full = _stub_full_record()
    assert len(json.dumps(full)) > 30000
    d = bench.compact_line(full, "bench_detail.json")
    line = json.dumps(d)
    assert len(line) < 6000, len(line)
    assert json.loads(line) == d
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["value"] == pytest.approx(full["value"], rel=1e-5) and d["ms_per_step"] == pytest.approx(full["ms_per_step"], rel=1e-5)
    for k in ("bound", "unit", "peak", "achieved", "frac", "traffic", "kernel", "valu_efficiency", "dominant", "other"):
        assert k in d["roofline"], k
    for which in ("dominant", "other"):
        for k in ("launches", "avg_launch_ms", "leapfrogs_per_launch"):
            assert k in d["roofline"][which], (which, k)
    assert "valu_mix" not in line and "peak_definition" not in line
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in d["cpu_baseline"], k
    assert sorted(d["config"]["secondary"]) == ["cfg3", "cfg4", "cfg5"]
    for name, o in d["config"]["secondary"].items():
        for k in ("value", "ms_per_step", "steps", "workload", "dtype", "roofline", "cpu_baseline"):
            assert k in o, (name, k)
        for k in ("bound", "frac", "achieved", "peak", "traffic", "kernel"):
            assert k in o["roofline"], (name, k)
        for k in ("value", "cores", "kind"):
            assert k in o["cpu_baseline"], (name, k)
    assert d["config"]["detail"] == "bench_detail.json"
    # a record that grew: the budget holds, the contract's keys stay
    fat = _stub_full_record()
    fat["config"]["runs"] = [fat["value"] * (1 + 1e-3 * i) for i in range(50)]
    fat["config"]["workload"] *= 8
    fat["cpu_baseline"]["sample"] *= 8
    fat["roofline"]["kernel"] *= 20
    for o in fat["config"]["secondary"].values():
        o["config"]["workload"] = o["config"]["workload"] * 6
        o["roofline"]["kernel"] = o["roofline"]["kernel"] * 10
    d2 = bench.compact_line(fat, "bench_detail.json")
    assert len(json.dumps(d2)) <= bench.LINE_BUDGET
    assert d2["value"] == d["value"] and sorted(d2["config"]["secondary"]) == ["cfg3", "cfg4", "cfg5"] and d2["roofline"]["frac"] == d["roofline"]["frac"]
    # a secondary config that failed is an error entry, not a lost line
    fat["config"]["secondary"]["cfg5"] = {"error": "RuntimeError('out of memory')" * 30}
    d3 = bench.compact_line(fat, None)
    assert "error" in d3["config"]["secondary"]["cfg5"] and len(json.dumps(d3)) <= bench.LINE_BUDGET
    # round 6: the HBM roof beside the issue roof in every roofline, the secondaries' too
    d6 = bench.compact_line(json.load(open(os.path.join(ROOT, "profiles", "r6_bench_default_detail.json"))), "bench_detail.json")   # (a round-6 record)
    assert len(json.dumps(d6)) <= bench.LINE_BUDGET
    for r in [d6["roofline"]] + [o["roofline"] for o in d6["config"]["secondary"].values()]:
        assert "hbm_model_frac" in r and r["hbm_model_frac"] is not None, r
    assert d6["roofline"].get("hbm_measured_frac") is not None and d6["config"]["secondary"]["cfg4"]["roofline"].get("hbm_measured_frac") is not None
    # … and a record that NO shedding brings under the budget still comes out: the headline keys alone (the old code asserted and printed nothing)
    huge = _stub_full_record()
    for i in range(40):
        huge["config"]["secondary"][f"extra{i}"] = json.loads(json.dumps(huge["config"]["secondary"]["cfg3"]))
    d4 = bench.compact_line(huge, "bench_detail.json")
    line4 = json.dumps(d4)
    assert len(line4) <= bench.LINE_BUDGET
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d4, k
    assert d4["value"] == d["value"] and d4["config"]["detail"] == "bench_detail.json" and "line_shortened" in d4["config"]


def test_counters_are_refused_when_taken_on_other_kernels(tmp_path, monkeypatch):
    """bench.py's roofline reads PMC counters from profiles/counters_at_head.json only when they were taken on the device
    code of the library in use (round 1 rescaled constants from a stale file): a digest mismatch gives None + a reason"""
    sys.path.insert(0, ROOT)
    import importlib

    bench = importlib.import_module("bench")
    real = bench.sources_digest("cfg2")
    prof = tmp_path / "profiles"
    prof.mkdir()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    monkeypatch.setattr(bench, "sources_digest", lambda config="cfg2": real or "d" * 64)
    good = {"source": "test", "configs": {"cfg2": {"unit_digest": real or "d" * 64, "mode0": {"valu_per_leapfrog": 190.0}}}}
    (prof / "counters_at_head.json").write_text(json.dumps(good))
    c, why = bench.counters_at_head("cfg2")
    assert c["mode0"]["valu_per_leapfrog"] == 190.0 and why == "test"
    c, why = bench.counters_at_head("cfg3")
    assert c is None and "cfg3" in why
    good["configs"]["cfg2"]["unit_digest"] = "0" * 64
    (prof / "counters_at_head.json").write_text(json.dumps(good))
    c, why = bench.counters_at_head("cfg2")
    assert c is None and "stale" in why
    (prof / "counters_at_head.json").unlink()
    c, why = bench.counters_at_head("cfg2")
    assert c is None and "missing" in why


def test_wave_timeline_analysis_on_a_synthetic_launch(tmp_path):
    """scripts/wave_timeline.py (the per-wave records of a measurement build): a launch whose wave slots are exactly half
    full, with every leaf step advancing two of a wave's four chains, must come out as fill 0.5 / lockstep 0.5"""
    import importlib.util

    import numpy as np

    spec = importlib.util.spec_from_file_location("wave_timeline", os.path.join(ROOT, "scripts", "wave_timeline.py"))
    wt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(wt)
    slots, n = 8, 8
    rec = np.zeros((n, 8), dtype=np.uint64)
    for w in range(n):  # eight waves on eight slots, each running for the first half of a 2-second launch … except one
        rec[w] = [10**8, 2 * 10**8, 1000, 2000, 500, 10, w, w % 8]
    rec[0, 1] = 3 * 10**8                              # … which runs to the end: the launch lasts 2 s
    p = tmp_path / "tl.bin"
    rec.tofile(p)
    out = wt.analyse(str(p), cpw=4, slots=slots)
    assert out["waves"] == n and abs(out["launch_s"] - 2.0) < 1e-9
    assert abs(out["fill"] - (7 * 1.0 + 2.0) / (slots * 2.0)) < 1e-9
    assert abs(out["lockstep"] - 0.5) < 1e-12
    assert abs(out["longest_wave_share_of_launch"] - 1.0) < 1e-9
    assert out["resident_waves_by_twentieth_of_the_launch"][0] == 8.0 and out["resident_waves_by_twentieth_of_the_launch"][-1] == 1.0
