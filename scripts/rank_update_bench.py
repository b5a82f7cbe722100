"""Rates of RankUpdateEuclideanMetric (include/ahmc_rank_update.h) → profiles/rank_update_rates.json.  Each subcommand merges its
section into the JSON file:

    python scripts/rank_update_bench.py apply [--out FILE]   # k_ru_apply: one `rocprofv3 --kernel-trace --stats` child run per (D, k)
    python scripts/rank_update_bench.py nuts  [--out FILE]   # whole-loop NUTS, rank update against Diag, repeated
    python scripts/rank_update_bench.py demo  [--out FILE]   # the usefulness target: leapfrogs per transition, ESS per gradient
    python scripts/rank_update_bench.py kernel --D D --k K   # (the child: 22 applications of M⁻¹ to N chains)

  * apply.  The kernel's own duration from the rocprofv3 kernel trace of a child that runs 20 leapfrogs (every application has the
    same shape: N listed columns, plain (D, N) arrays).  Byte model: X read + Y written, 2·D·N·sizeof(T); N is chosen so that one (D, N)
    array is 1 GiB.  Bar: >= 0.6 of the 6.29 TB/s copy rate for k <= 8 at D >= 4096 (an estimate from k_w_target's measured 0.83).
  * nuts.  D = 8192 (wide), k = 8, 4 096 chains, max_depth 6: leapfrogs/s of `--repeats` timed windows of 10 transitions per metric,
    the metrics alternating.  Bar: a rank-update leapfrog costs <= 1.35× a Diag leapfrog.
  * demo.  The dense Gaussian of tests/test_rank_update_metric.py (Σ = a·I + U·diag(λ)·Uᵀ, D = 256, k = 4, λ up to 400, a = 10⁻³) with
    StepSizeAdaptor and 4 096 chains, for Unit, Diag(diag Σ) and the rank update M⁻¹ = Σ: leapfrogs per transition and ESS (bulk,
    MCMCChains' summarystats on the device) per gradient evaluation.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ahmc_amd as A  # noqa: E402

COPY_TBS = 6.29
OUT = os.path.join(ROOT, "profiles", "rank_update_rates.json")


def merge(path, key, value):
    res = json.load(open(path)) if os.path.exists(path) else {}
    res[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


def kernel_child(D, k, steps):
    """the child run: a rank-update context of N = 2^27 / D chains (one (D, N) array = 1 GiB), `steps` leapfrogs"""
    N = (1 << 27) // D
    rs = np.random.default_rng(0)
    m = A.RankUpdateEuclideanMetric(0.5 + rs.random(D), rs.normal(size=(D, k)) / np.sqrt(D), np.eye(k))
    e = A.Engine(A.Hamiltonian(m, A.IsoGaussian(D)), N, rng=1, lib=A.load_hip_library())
    e.set_integrator(A.Leapfrog(0.01))
    e.set_position(np.zeros((D, N), order="F"))
    e.step(steps)
    e.sync()
    e.close()


def kernel_stats(D, k, steps):
    """one child under rocprofv3 --kernel-trace --stats → {kernel: {calls, mean_ns, min_ns, max_ns, stddev_ns}}"""
    tmp = tempfile.mkdtemp(prefix="ru_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "ru", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "kernel", "--D", str(D), "--k", str(k), "--steps", str(steps)]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if res.returncode != 0:
            raise RuntimeError(f"rocprofv3 failed ({res.returncode}):\n{res.stderr[-3000:]}")
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError(f"no kernel_stats.csv under {tmp}")
        out = {}
        for row in csv.DictReader(open(files[0])):
            short = row["Name"].split("(")[0].replace("void ", "").replace("ahmc::", "")
            out[short] = {"calls": int(row["Calls"]), "mean_ns": float(row["AverageNs"]), "min_ns": float(row["MinNs"]),
                          "max_ns": float(row["MaxNs"]), "stddev_ns": float(row.get("StdDev") or 0)}
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def cmd_apply(args):
    rows = []
    for D in (512, 4096, 8192, 32768):
        N = (1 << 27) // D
        for k in (1, 4, 8, 16, 32):
            st = kernel_stats(D, k, args.steps)
            name = [n for n in st if n.startswith("k_ru_apply<")]
            assert len(name) == 1, st.keys()
            ka = st[name[0]]
            nbytes = 2 * D * N * 8
            row = dict(D=D, N=N, k=k, kernel=name[0], calls=ka["calls"], mean_us=ka["mean_ns"] / 1e3, min_us=ka["min_ns"] / 1e3,
                       max_us=ka["max_ns"] / 1e3, stddev_us=ka["stddev_ns"] / 1e3, TBps=nbytes / ka["mean_ns"] / 1e3,
                       fraction_of_copy=nbytes / ka["mean_ns"] / 1e3 / COPY_TBS,
                       other_kernels_mean_us={n: v["mean_ns"] / 1e3 for n, v in st.items() if n.startswith(("k_d_pre", "k_d_post", "k_w_target"))})
            if k <= 8 and D >= 4096:
                row["bar_met"] = row["fraction_of_copy"] >= 0.6
            rows.append(row)
            print(json.dumps(row), flush=True)
    merge(args.out, "apply", {"rows": rows, "method": "rocprofv3 --kernel-trace --stats, one child per (D, k); byte model X read + Y written",
                              "bar": {"fraction_of_copy": 0.6, "copy_TBps": COPY_TBS, "where": "k <= 8, D >= 4096"}})


def cmd_nuts(args):
    hip = A.load_hip_library()
    rs = np.random.default_rng(1)
    D, N, k = 8192, 4096, 8
    engines = {}
    for name in ("diag", "ru"):
        m = A.DiagEuclideanMetric(np.ones(D)) if name == "diag" else A.RankUpdateEuclideanMetric(np.ones(D), rs.normal(size=(D, k)) / np.sqrt(D), np.eye(k))
        e = A.Engine(A.Hamiltonian(m, A.IsoGaussian(D)), N, rng=2, lib=hip)
        e.set_integrator(A.Leapfrog(0.15))
        e.set_position(rs.normal(size=(D, N)))
        engines[name] = e
    kern = A.HMCKernel(A.Trajectory(A.MultinomialTS, A.Leapfrog(0.15), A.GeneralisedNoUTurn(max_depth=6)))
    for e in engines.values():
        e.run(kern, 2)
        e.sync()
    rates = {"diag": [], "ru": []}
    it = 3
    for _ in range(args.repeats):
        for name, e in engines.items():
            e.reset_accum()
            t = time.perf_counter()
            e.run(kern, it + 9, i_first=it)
            e.sync()
            dt = time.perf_counter() - t
            rates[name].append(e.accum(moments=False)["total_n_steps"] / dt)
        it += 10
    for e in engines.values():
        e.close()
    ratios = [d / r for d, r in zip(rates["diag"], rates["ru"])]
    out = dict(D=D, N=N, k=k, max_depth=6, repeats=args.repeats, diag_leapfrogs_per_s=rates["diag"], ru_leapfrogs_per_s=rates["ru"],
               ru_over_diag_per_leapfrog=ratios, median=statistics.median(ratios), min=min(ratios), max=max(ratios), bar=1.35,
               bar_met=statistics.median(ratios) <= 1.35)
    print(json.dumps(out), flush=True)
    merge(args.out, "nuts", out)


def cmd_demo(args):
    import torch

    hip = A.load_hip_library()
    D, k, N, n_adapts, n_samples = 256, 4, 4096, 150, 250
    rs = np.random.default_rng(600)
    U, _ = np.linalg.qr(rs.normal(size=(D, k)))
    lam = np.geomspace(50, 400, k)
    Sigma = 1e-3 * np.eye(D) + U @ np.diag(lam) @ U.T
    P = np.asfortranarray(np.linalg.inv(Sigma))
    out = {"D": D, "k": k, "N": N, "n_adapts": n_adapts, "kept": n_samples - n_adapts, "target": "Σ = 1e-3·I + U·diag(λ)·Uᵀ, λ 50 … 400"}
    metrics = {"unit": A.UnitEuclideanMetric((D, N)), "diag": A.DiagEuclideanMetric(np.diag(Sigma).copy()),
               "rank_update": A.RankUpdateEuclideanMetric(np.full(D, 1e-3), U, np.diag(lam))}
    for name, m in metrics.items():
        e = A.Engine(A.Hamiltonian(m, A.DenseGaussian(P)), N, rng=A.PhiloxRNG(21), lib=hip)
        kern = A.HMCKernel(A.Trajectory(A.MultinomialTS, A.Leapfrog(np.full(N, 0.1)), A.GeneralisedNoUTurn(max_depth=10)))
        e.set_integrator(kern.tau.integrator)
        e.set_position(np.random.default_rng(1).normal(size=(D, N)) * 0.1)
        e.adaptor_init(A.StepSizeAdaptor(0.8, kern.tau.integrator))
        K = n_samples - n_adapts
        draws = torch.empty((K, N, D), dtype=torch.float64, device="cuda")
        t = time.perf_counter()
        e.run(kern, n_samples, n_adapts=n_adapts, drop_warmup=True, samples_out=draws.data_ptr())
        e.sync()
        dt = time.perf_counter() - t
        acc = e.accum(moments=False)
        grads = acc["total_n_steps"]  # (kept transitions, all chains)
        st = e.summarystats(draws.data_ptr(), K)
        out[name] = dict(leapfrogs_per_transition=grads / (acc["n_transitions"] * N), ess_bulk_mean=float(np.mean(st["ess_bulk"])),
                         ess_bulk_min=float(np.min(st["ess_bulk"])), ess_bulk_mean_per_gradient=float(np.mean(st["ess_bulk"])) / grads,
                         ess_bulk_min_per_gradient=float(np.min(st["ess_bulk"])) / grads, rhat_max=float(np.max(st["rhat"])),
                         step_size_mean=float(e.get_stepsize().mean()), seconds=dt)
        print(name, json.dumps(out[name]), flush=True)
        e.close()
        del draws
    merge(args.out, "demo", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("apply", "nuts", "demo", "kernel"))
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--D", type=int)
    ap.add_argument("--k", type=int)
    args = ap.parse_args()
    if args.what == "kernel":
        kernel_child(args.D, args.k, args.steps)
    else:
        {"apply": cmd_apply, "nuts": cmd_nuts, "demo": cmd_demo}[args.what](args)


if __name__ == "__main__":
    main()
