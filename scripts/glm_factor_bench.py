"""Rates of a GLM with index-coded factors (include/ahmc_glm_factor.h) → profiles/glm_factor_rates.json.

    python scripts/glm_factor_bench.py [--out FILE] [--steps 12]

The parent never opens the GPU.  Every measurement is a fresh child process under a time limit of its own and under
`rocprofv3 --kernel-trace --stats`; the parent checks each exit status and stops at the first child that fails or times out (nothing
more is started on a card that may be in trouble).

Shapes (n_obs, P_x, levels, N): (65536, 2, (4096,), 4096) and (8192, 16, (256, 32), 8192); 12 leapfrogs each, both element types.
Per shape and element type, in one session, three models on the same data:
  * "factor":  HierGLMTarget(X, factors=…) with a non-centred group on each factor's rows;
  * "one-hot": the same model with the factors as one-hot columns of X (glm.expand_factors), through ahmc_hglm_set_target;
  * "dense":   the plain GLMTarget on the P_x dense columns alone (what the regression costs without the factors).
Reported: the evaluation (the sum of the mean durations of the GLM kernels) of each, factor / dense and one-hot / factor; k_glm_eta_f
and k_glm_fgrad against their byte models at the device's copy rate (6.29 TB/s):
      k_glm_eta_f   writes U (n_obs·N); the gathers read W (P·N, from L2) and the level indices (n_obs·F int32, from L2)
      k_glm_fgrad   reads U once per factor (F·n_obs·N), writes the factors' rows of R (ΣL·N); every chain's threads also read
                    the permutation (F·n_obs int32), which stays in L2
Expectation, stated before the first run: at the first shape one evaluation with the factor costs little more than the dense
model's — the gathers and k_glm_fgrad are byte-bound, each about one pass over U, n_obs·N elements ≈ 0.34 ms in f64 at the copy
rate — while the one-hot model costs what a dense (65536 × 4098) regression costs: two products of 2.2·10¹² flop, about 55 ms each at
the measured 40 TFLOP/s, so two orders of magnitude more.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import glm_bench as GB  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "glm_factor_rates.json")
COPY_RATE = 6.29e12  # B/s
SHAPES = ((65536, 2, (4096,), 4096), (8192, 16, (256, 32), 8192))
ENCODINGS = ("dense", "factor", "one-hot")


def model(n_obs, Px, levels, seed=0):
    rs = np.random.default_rng(seed)
    X = rs.normal(size=(n_obs, Px)) / np.sqrt(Px)
    idx = [rs.integers(0, L, size=n_obs) for L in levels]
    eta = X @ rs.normal(size=Px) + sum(0.5 * rs.normal(size=L)[i] for L, i in zip(levels, idx))
    y = (rs.random(n_obs) < 1 / (1 + np.exp(-eta))).astype(np.float64)
    return X, y, idx


def child(n_obs, Px, levels, N, dt, steps, encoding):
    import ahmc_amd as A

    X, y, idx = model(n_obs, Px, levels)
    factors = [A.Factor(i, L) for i, L in zip(idx, levels)]
    groups = [A.CoefGroup(lo, hi, centered=False) for lo, hi in A.factor_ranges(Px, factors)]
    if encoding == "dense":
        t = A.GLMTarget(X, y, prior_scale=1.0)
    elif encoding == "factor":
        t = A.HierGLMTarget(X, y, groups, prior_scale=1.0, factors=factors)
    else:
        t = A.HierGLMTarget(A.glm.expand_factors(X, factors), y, groups, prior_scale=1.0)
    D = t.D
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((D, N)), t), N, dtype=GB.DTYPES[dt], rng=1, lib=A.load_hip_library())
    e.set_integrator(A.Leapfrog(0.01))
    e.set_position(0.1 * np.random.default_rng(1).normal(size=(D, N)))
    e.step(steps)
    e.sync()
    e.close()


def run_child(args, n_obs, Px, levels, N, dt, encoding, limit=400):
    """one child under rocprofv3 and its own time limit (hglm_bench.run_child's command, this file's child)"""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile

    argv = ["child", "--n_obs", str(n_obs), "--Px", str(Px), "--levels", ",".join(map(str, levels)), "--N", str(N), "--dtype", dt, "--steps", str(args.steps),
            "--encoding", encoding]
    tmp = tempfile.mkdtemp(prefix="glm_factor_prof_")
    try:
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "glmf", "--output-format", "csv", "--",
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
    ap.add_argument("--Px", type=int)
    ap.add_argument("--levels", default="")
    ap.add_argument("--N", type=int)
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--encoding", default="factor", choices=ENCODINGS)
    args = ap.parse_args()
    if args.what == "child":
        child(args.n_obs, args.Px, tuple(int(x) for x in args.levels.split(",")), args.N, args.dtype, args.steps, args.encoding)
        return
    rows = []
    for n_obs, Px, levels, N in SHAPES:
        for dt, dtype in GB.DTYPES.items():
            st = {enc: run_child(args, n_obs, Px, levels, N, dt, enc) for enc in ENCODINGS}
            ev = {enc: sum(v["mean_us"] for v in st[enc].values()) for enc in ENCODINGS}
            size, F, Lt = np.dtype(dtype).itemsize, len(levels), sum(levels)
            eta_f = [v for k, v in st["factor"].items() if k.startswith("k_glm_eta_f<")][0]
            fgrad = [v for k, v in st["factor"].items() if k.startswith("k_glm_fgrad<")][0]
            eta_d = [v for k, v in st["dense"].items() if k.startswith("k_glm_eta<")][0]
            pass_us = size * n_obs * N / COPY_RATE * 1e6
            bytes_fgrad = size * N * (F * n_obs + Lt)
            row = dict(n_obs=n_obs, P_x=Px, levels=list(levels), N=N, dtype=dt, kernels=st, evaluation_us=ev, factor_over_dense=ev["factor"] / ev["dense"],
                       one_hot_over_factor=ev["one-hot"] / ev["factor"], one_pass_over_U_us=pass_us, eta_f_us=eta_f["mean_us"], eta_dense_us=eta_d["mean_us"],
                       eta_f_minus_dense_us=eta_f["mean_us"] - eta_d["mean_us"], eta_f_fraction_of_copy_rate=pass_us / eta_f["mean_us"], fgrad_us=fgrad["mean_us"],
                       fgrad_fraction_of_copy_rate=bytes_fgrad / (fgrad["mean_us"] * 1e-6) / COPY_RATE)
            rows.append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "kernels"}), flush=True)
            GB.merge(args.out, "kernels", {"rows": rows, "copy_rate_TBps": COPY_RATE / 1e12,
                                           "method": "rocprofv3 --kernel-trace --stats, one fresh child per shape, element type and encoding; mean kernel "
                                                     f"durations over {args.steps} leapfrogs + the first evaluation",
                                           "expectation": "stated before the run: at (65536, 2, (4096,), 4096) the evaluation with the factor costs little more "
                                                          "than the dense model's (the gathers and k_glm_fgrad about one pass over U each), the one-hot model "
                                                          "what a dense (65536 x 4098) regression costs"})


if __name__ == "__main__":
    main()
