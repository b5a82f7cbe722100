"""Rates of HierGLMTarget (include/ahmc_glm_hier.h) → profiles/hglm_rates.json.

    python scripts/hglm_bench.py [--out FILE] [--steps 12]

The parent never opens the GPU.  Every measurement is a fresh child process under a time limit of its own and under
`rocprofv3 --kernel-trace --stats`; the parent checks each exit status and stops at the first child that fails or times out (nothing
more is started on a card that may be in trouble).

Shapes: the three (n_obs, P, N) of scripts/glm_bench.py, four non-centred groups covering half of the P columns (the context has
D = P + 4), 12 leapfrogs each, both element types.  Per shape, in the same session, a plain GLMTarget of the same X.  Reported:
  * k_hglm_coef + k_hglm_finish as a share of one whole evaluation;
  * each of the two against the byte model of its own reads and writes at the device's copy rate (6.29 TB/s):
      k_hglm_coef    reads θ (D·N), writes W (P·N)
      k_hglm_finish  reads partial (⌈n_obs/64⌉·N), R (P·N), θ (D·N) and W of the non-centred members, writes g (D·N) and ℓπ (N)
  * the whole evaluation against the plain model's: the difference should be the two kernels (the products are the same code; the
    plain model's k_glm_lp is replaced by k_hglm_finish).
Expectation, stated before the first run: both kernels are passes over (P, N) arrays beside two products of n_obs·P·N multiply-adds,
so their share is a few per cent where n_obs is in the thousands, and each runs at a good fraction (above half) of its byte model.
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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import glm_bench as GB  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "hglm_rates.json")
COPY_RATE = 6.29e12  # B/s
N_GROUPS = 4


def groups_of(P):
    """four non-centred groups over the upper half of the columns"""
    lo, m = P // 2, P // 2 // N_GROUPS
    return [(lo + k * m, lo + (k + 1) * m if k < N_GROUPS - 1 else P) for k in range(N_GROUPS)]


def child(n_obs, P, N, dt, steps, hier):
    import ahmc_amd as A

    X, y, p = GB.model(n_obs, P)
    if hier:
        t = A.HierGLMTarget(X, y, [A.CoefGroup(lo, hi) for lo, hi in groups_of(P)], prior_prec=p)
    else:
        t = A.GLMTarget(X, y, prior_prec=p)
    D = t.D
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((D, N)), t), N, dtype=GB.DTYPES[dt], rng=1, lib=A.load_hip_library())
    e.set_integrator(A.Leapfrog(0.01))
    e.set_position(0.1 * np.random.default_rng(1).normal(size=(D, N)))
    e.step(steps)
    e.sync()
    e.close()


def run_child(args, n_obs, P, N, dt, hier, limit=400):
    """one child under rocprofv3 and its own time limit → {kernel: calls, mean / min / max µs}.  Raises on a failure: the caller stops there."""
    argv = ["child", "--n_obs", str(n_obs), "--P", str(P), "--N", str(N), "--dtype", dt, "--steps", str(args.steps)] + (["--hier"] if hier else [])
    tmp = tempfile.mkdtemp(prefix="hglm_prof_")
    try:
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "hglm", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), *argv]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"child {argv} ended with status {res.returncode}: nothing more is started\n{res.stdout[-2000:]}\n{res.stderr[-3000:]}")
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError(f"no kernel_stats.csv under {tmp}")
        out = {}
        for row in csv.DictReader(open(files[0])):
            short = row["Name"].split("(")[0].replace("void ", "").replace("ahmc::", "")
            if short.startswith(("k_glm_", "k_hglm_")):
                out[short] = {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                              "max_us": float(row["MaxNs"]) / 1e3}
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all", choices=("all", "child"))
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--n_obs", type=int)
    ap.add_argument("--P", type=int)
    ap.add_argument("--N", type=int)
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--hier", action="store_true")
    args = ap.parse_args()
    if args.what == "child":
        child(args.n_obs, args.P, args.N, args.dtype, args.steps, args.hier)
        return
    rows = []
    for n_obs, P, N in GB.SHAPES:
        for dt, dtype in GB.DTYPES.items():
            plain = run_child(args, n_obs, P, N, dt, False)
            hier = run_child(args, n_obs, P, N, dt, True)
            size, D = np.dtype(dtype).itemsize, P + N_GROUPS
            coef = [v for k, v in hier.items() if k.startswith("k_hglm_coef<")][0]
            fin = [v for k, v in hier.items() if k.startswith("k_hglm_finish<")][0]
            bytes_coef = size * N * (D + P)
            bytes_fin = size * N * ((n_obs + 63) // 64 + P + D + (P - P // 2) + D + 1)
            ev_h, ev_p = sum(v["mean_us"] for v in hier.values()), sum(v["mean_us"] for v in plain.values())
            row = dict(n_obs=n_obs, P=P, D=D, N=N, dtype=dt, groups=groups_of(P), kernels=hier, plain_kernels=plain, evaluation_us=ev_h, plain_evaluation_us=ev_p,
                       new_kernels_us=coef["mean_us"] + fin["mean_us"], new_kernels_share=(coef["mean_us"] + fin["mean_us"]) / ev_h,
                       coef_fraction_of_copy_rate=bytes_coef / (coef["mean_us"] * 1e-6) / COPY_RATE,
                       finish_fraction_of_copy_rate=bytes_fin / (fin["mean_us"] * 1e-6) / COPY_RATE,
                       evaluation_minus_plain_us=ev_h - ev_p, evaluation_over_plain=ev_h / ev_p)
            rows.append(row)
            print(json.dumps({k: v for k, v in row.items() if k not in ("kernels", "plain_kernels", "groups")}), flush=True)
    GB.merge(args.out, "kernels", {"rows": rows, "copy_rate_TBps": COPY_RATE / 1e12,
                                   "method": "rocprofv3 --kernel-trace --stats, one fresh child per shape, element type and model; mean kernel durations over "
                                             f"{args.steps} leapfrogs + the first evaluation",
                                   "expectation": "stated before the run: the two new kernels are a few per cent of an evaluation where n_obs is in the thousands, "
                                                  "each above half of its byte model at the copy rate"})


if __name__ == "__main__":
    main()
