"""Cost of ahmc_glm_loo (include/ahmc_glm_loo.h) → profiles/glm_loo_rates.json.

    python scripts/glm_loo_bench.py all [--out FILE]

The parent never opens the GPU.  Every measurement is a child process of its own under a time limit of its own; the parent stops at
the first child that fails or times out.

One call on a bernoulli_logit model of (n_obs, P) = (8192, 256) at N = 8192 with S = 8192 draws (one chunk), in Float64 and Float32.
Two fresh children per element type:
  * wall: the second of two calls, host clock around the blocking call (the draws are in device memory, log_weights_out is given);
  * trace: ONE call under `rocprofv3 --kernel-trace --stats`: the total duration of every kernel of the call, by stage.
The expectations (stated before the run; none is a gate) are evaluated in "expectations".
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

OUT = os.path.join(ROOT, "profiles", "glm_loo_rates.json")
SHAPE = (8192, 256, 8192, 8192)   # n_obs, P, N, S
COPY_TBS = 6.29                   # the chip's copy rate
DIAG_SORT_NS_PER_KEY_PASS = 0.32e9 / (8192 * 256000) / 8   # profiles/diag_rates.json: D 8192 × S 256 000, u64 keys, 8 passes in 0.32 s
STAGES = {"A_model": ("k_glm_eta", "k_hglm_coef", "k_glm_cut"), "A_keys": ("loo::k_loo_keys",), "B_sort": ("diag::k_dg_hist", "diag::k_dg_scatter", "diag::k_sc_"),
          "C_psis": ("loo::k_loo_psis",)}


def child(dtname, calls):
    import torch

    import ahmc_amd as A

    n_obs, P, N, S = SHAPE
    dtype = np.dtype(dtname)
    rs = np.random.default_rng(0)
    X = rs.normal(size=(n_obs, P)) / np.sqrt(P)
    beta = rs.normal(size=P)
    y = (X @ beta + rs.logistic(size=n_obs) > 0).astype(np.float64)
    t = A.GLMTarget(X, y, family="bernoulli_logit", prior_scale=2.5)
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((t.D, N)), t), N, dtype=dtype, rng=1, lib=A.load_hip_library())
    draws = torch.from_numpy(np.ascontiguousarray((beta[:, None] + 0.05 * rs.normal(size=(P, S))).T.astype(dtype))).cuda()   # (S, D) row-major = (D, S) column-major
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        out = e.glm_loo(draws.data_ptr(), n_cols=S, log_weights=True)
        ms.append(1e3 * (time.perf_counter() - t0))
    s = A.loo_summary(out)
    print("RESULT " + json.dumps({"dtype": dtname, "ms_per_call": ms, "elpd_loo": s["elpd_loo"], "p_loo": s["p_loo"], "k_counts": s["k_counts"]}), flush=True)
    e.close()


def run_child(argv, limit, trace):
    tmp = tempfile.mkdtemp(prefix="glm_loo_prof_")
    try:
        cmd = [sys.executable, os.path.abspath(__file__), *argv]
        if trace:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "loo", "--output-format", "csv", "--", *cmd]
        res = subprocess.run(["timeout", "-k", "10", str(limit), *cmd], capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"child {argv} ended with status {res.returncode}: nothing more is started\n{res.stdout[-2000:]}\n{res.stderr[-3000:]}")
        if not trace:
            return json.loads(next(l for l in res.stdout.splitlines() if l.startswith("RESULT "))[7:])
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError(f"no kernel_stats.csv under {tmp}")
        out = {}
        for row in csv.DictReader(open(files[0])):
            short = row["Name"].split("(")[0].replace("void ", "").replace("ahmc::", "")
            if any(short.startswith(p) for ps in STAGES.values() for p in ps):
                out[short] = {"calls": int(row["Calls"]), "total_us": int(row["Calls"]) * float(row["AverageNs"]) / 1e3}
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def cmd_all(args):
    n_obs, P, N, S = SHAPE
    vals = n_obs * S
    rec = {"n_obs": n_obs, "P": P, "N": N, "S": S, "values": vals, "family": "bernoulli_logit", "dtypes": {},
           "method": "wall: host clock around the second of two blocking calls; kernels: rocprofv3 --kernel-trace --stats around ONE call in a child of its "
                     "own; one fresh child process per cell, one build, one session, one run per cell"}
    for dt in ("float64", "float32"):
        r = run_child(["child", "--dtype", dt, "--calls", "2"], 300, False)
        k = run_child(["child", "--dtype", dt, "--calls", "1"], 300, True)
        r["kernels"] = k
        r["stage_us"] = {st: sum(v["total_us"] for name, v in k.items() if any(name.startswith(p) for p in ps)) for st, ps in STAGES.items()}
        item = np.dtype(dt).itemsize
        passes = 8 if dt == "float64" else 5
        model = {"A_keys_us": vals * (item + 12) / (COPY_TBS * 1e6), "B_sort_us": vals * passes * DIAG_SORT_NS_PER_KEY_PASS / 1e3, "C_psis_us": vals * 20 / (COPY_TBS * 1e6)}
        su = r["stage_us"]
        r["model_us"] = model
        r["expectations"] = {
            "A: the transposing pass at the copy rate (within 2x of its byte model)": "held" if su["A_keys"] <= 2 * model["A_keys_us"] else "missed",
            "B: the diag path's measured rate per key and pass (within 1.25x)": "held" if su["B_sort"] <= 1.25 * model["B_sort_us"] else "missed",
            "C: within 4x of the byte model (sorted row read once, weights written once)": "held" if su["C_psis"] <= 4 * model["C_psis_us"] else "missed"}
        rec["dtypes"][dt] = r
        print(json.dumps({kk: v for kk, v in r.items() if kk != "kernels"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("all", "child"))
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--dtype", default="float64")
    ap.add_argument("--calls", type=int, default=2)
    args = ap.parse_args()
    if args.what == "child":
        child(args.dtype, args.calls)
    else:
        cmd_all(args)


if __name__ == "__main__":
    main()
