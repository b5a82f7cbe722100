"""Rates of the low-rank mass-matrix adaptor (include/ahmc_lowrank_adapt.h) → profiles/lowrank_adapt_rates.json.  Each subcommand
merges its section into the JSON file:

    python scripts/lowrank_adapt_bench.py push [--out FILE]   # the push kernels: one `rocprofv3 --kernel-trace --stats` child per (D, ℓ)
    python scripts/lowrank_adapt_bench.py demo [--out FILE]   # the usefulness target: LowRankVar against PooledVar (report only)
    python scripts/lowrank_adapt_bench.py kernel --D D --k K --oversample P   # (the child: leapfrogs and pushes of one context)

  * push.  The kernels' own durations from the rocprofv3 kernel trace (no counters in the same run) of a child that runs `--steps`
    leapfrogs and `--steps` pushes of a float64 context of N = 2²⁷ / D chains (one (D, N) array = 1 GiB), D ∈ {512, 4096, 8192, 32768},
    ℓ ∈ {9, 16, 40} (k = ℓ − 8 with oversampling 8; k = 32 for ℓ = 40).  One child process per shape, each under its own time limit.
    A push = k_lr_colsum_partial + k_lr_colsum_final + k_lr_project + k_lr_accumulate + k_lr_merge; the leapfrog of the same context
    = k_d_pre + the target (k_w_target, or k_fill_caches below the wide limit) + k_ru_apply + k_d_post.
    Expectation from the byte model (unmeasured when it was written): the push reads X three times (the column sums, the projection,
    the accumulation) plus small partials, a leapfrog makes about ten array passes, so a push should cost no more than one leapfrog
    at ℓ <= 16.  `bar_met` says whether it does.
  * demo.  DESIGN §13's usefulness target (Σ = 10⁻³·I + U·diag(λ)·Uᵀ, D = 256, k = 4, λ 50 … 400) from the unit metric with
    StanHMCAdaptor(LowRankVar(rank 4)) and with StanHMCAdaptor(PooledVar): leapfrogs per transition and bulk ESS per gradient of the
    kept draws, R-hat, and the condition number of the preconditioned covariance.  Report only.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ahmc_amd as A  # noqa: E402
from ahmc_amd import rank_update as RU  # noqa: E402

COPY_TBS = 6.29
OUT = os.path.join(ROOT, "profiles", "lowrank_adapt_rates.json")
PUSH = ("k_lr_colsum_partial", "k_lr_colsum_final", "k_lr_project", "k_lr_accumulate", "k_lr_merge")
LEAPFROG = ("k_d_pre", "k_w_target", "k_fill_caches", "k_ru_apply", "k_d_post")


def merge(path, key, value):
    res = json.load(open(path)) if os.path.exists(path) else {}
    res[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


def kernel_child(D, k, p, steps):
    N = (1 << 27) // D
    lf = A.Leapfrog(0.01)
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((D, N)), A.IsoGaussian(D)), N, rng=1, lib=A.load_hip_library())
    e.set_integrator(lf)
    e.set_position(np.zeros((D, N), order="F"))
    e.adaptor_init(A.StanHMCAdaptor(A.LowRankVar(D, k, p), A.StepSizeAdaptor(0.8, lf), init_buffer=0, term_buffer=0, window_size=10 * steps))
    e.step(steps)
    for i in range(1, steps + 1):  # inside the first window: a push each, no fit
        e.adapt(i, 100 * steps, alpha=1.0)
    e.sync()
    e.close()


def kernel_stats(D, k, p, steps, limit):
    tmp = tempfile.mkdtemp(prefix="lr_prof_")
    try:
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "lr", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "kernel", "--D", str(D), "--k", str(k), "--oversample", str(p), "--steps", str(steps)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"child failed ({res.returncode}):\n{res.stderr[-3000:]}")
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError(f"no kernel_stats.csv under {tmp}")
        out = {}
        for row in csv.DictReader(open(files[0])):
            short = row["Name"].split("(")[0].replace("void ", "").replace("ahmc::", "")
            out[short] = {"calls": int(row["Calls"]), "mean_ns": float(row["AverageNs"]), "min_ns": float(row["MinNs"]), "max_ns": float(row["MaxNs"])}
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def cmd_push(args):
    rows = []
    for D in (512, 4096, 8192, 32768):
        N = (1 << 27) // D
        for ell, k in ((9, 1), (16, 8), (40, 32)):
            st = kernel_stats(D, k, ell - k, args.steps, args.limit)  # a failing child ends the whole run: nothing more is started
            part = lambda names: {n: v["mean_ns"] / 1e3 for n, v in st.items() if n.split("<")[0] in names}  # noqa: E731
            push, leap = part(PUSH), part(LEAPFROG)
            assert {n.split("<")[0] for n in push} == set(PUSH), st.keys()
            push_us, leap_us = sum(push.values()), sum(leap.values())
            xbytes = D * N * 8
            row = dict(D=D, N=N, k=k, ell=ell, steps=args.steps, push_us=push_us, leapfrog_us=leap_us, push_over_leapfrog=push_us / leap_us,
                       push_kernels_mean_us=push, leapfrog_kernels_mean_us=leap,
                       project_fraction_of_copy=xbytes / (push[[n for n in push if n.startswith("k_lr_project")][0]] * 1e3) / 1e3 / COPY_TBS,
                       accumulate_fraction_of_copy=xbytes / (push[[n for n in push if n.startswith("k_lr_accumulate")][0]] * 1e3) / 1e3 / COPY_TBS)
            if ell <= 16:
                row["bar_met"] = push_us <= leap_us
            rows.append(row)
            print(json.dumps(row), flush=True)
    merge(args.out, "push", {"rows": rows, "method": "rocprofv3 --kernel-trace --stats, one child per (D, ell), float64, one (D, N) array = 1 GiB; "
                                                     "fraction_of_copy: one read of X over the kernel's time, against the 6.29 TB/s copy rate",
                             "bar": "a push costs no more than one leapfrog of the same context at ell <= 16"})


def cmd_demo(args):
    import torch

    hip = A.load_hip_library()
    D, k, N, n_adapts, n_samples = 256, 4, 4096, 150, 250
    rs = np.random.default_rng(600)
    U, _ = np.linalg.qr(rs.normal(size=(D, k)))
    lam = np.geomspace(50, 400, k)
    Sigma = 1e-3 * np.eye(D) + U @ np.diag(lam) @ U.T
    P = np.asfortranarray(np.linalg.inv(Sigma))

    def cond(Minv):
        Li = np.linalg.inv(np.linalg.cholesky(Minv))
        w = np.linalg.eigvalsh(Li @ Sigma @ Li.T)
        return float(w[-1] / w[0])

    out = {"D": D, "k": k, "N": N, "n_adapts": n_adapts, "kept": n_samples - n_adapts, "target": "Σ = 1e-3·I + U·diag(λ)·Uᵀ, λ 50 … 400",
           "cond_unit": cond(np.eye(D)), "cond_diag_of_sigma": cond(np.diag(np.diag(Sigma)))}
    for name in ("lowrank", "pooled"):
        lf = A.Leapfrog(np.full(N, 0.1))
        kern = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=10)))
        metric = A.UnitEuclideanMetric((D, N)) if name == "lowrank" else A.DiagEuclideanMetric(np.ones(D))
        e = A.Engine(A.Hamiltonian(metric, A.DenseGaussian(P)), N, rng=A.PhiloxRNG(21), lib=hip)
        e.set_integrator(lf)
        e.set_position(np.random.default_rng(1).normal(size=(D, N)) * 0.1)
        pc = A.LowRankVar(D, k) if name == "lowrank" else A.PooledVar(metric)
        e.adaptor_init(A.StanHMCAdaptor(pc, A.StepSizeAdaptor(0.8, lf), init_buffer=15, term_buffer=20, window_size=15))
        K = n_samples - n_adapts
        draws = torch.empty((K, N, D), dtype=torch.float64, device="cuda")
        t = time.perf_counter()
        e.run(kern, n_samples, n_adapts=n_adapts, drop_warmup=True, samples_out=draws.data_ptr())
        e.sync()
        dt = time.perf_counter() - t
        acc = e.accum(moments=False)
        grads = acc["total_n_steps"]
        st = e.summarystats(draws.data_ptr(), K)
        m = e.get_metric()
        Minv = RU.dense(*m) if name == "lowrank" else np.diag(np.asarray(m, dtype=np.float64).ravel()[:D])
        out[name] = dict(leapfrogs_per_transition=grads / (acc["n_transitions"] * N), ess_bulk_mean=float(np.mean(st["ess_bulk"])),
                         ess_bulk_min=float(np.min(st["ess_bulk"])), ess_bulk_mean_per_gradient=float(np.mean(st["ess_bulk"])) / grads,
                         ess_bulk_min_per_gradient=float(np.min(st["ess_bulk"])) / grads, rhat_max=float(np.max(st["rhat"])),
                         step_size_mean=float(e.get_stepsize().mean()), cond_preconditioned=cond(Minv), seconds=dt)
        print(name, json.dumps(out[name]), flush=True)
        e.close()
        del draws
    merge(args.out, "demo", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("push", "demo", "kernel"))
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="time limit of one child, seconds")
    ap.add_argument("--D", type=int)
    ap.add_argument("--k", type=int)
    ap.add_argument("--oversample", type=int, default=8)
    args = ap.parse_args()
    if args.what == "kernel":
        kernel_child(args.D, args.k, args.oversample, args.steps)
    else:
        {"push": cmd_push, "demo": cmd_demo}[args.what](args)


if __name__ == "__main__":
    main()
