"""Cost of the categorical-logit family (include/ahmc_glm_categorical.h) → one JSON record (default test_out/glm_categorical_cost.json;
the MI355X run is kept under "cost" in profiles/glm_categorical_margins.json).

    python scripts/glm_categorical_bench.py all [--out FILE] [--evals 20]

The parent never opens the GPU.  Every measurement is a child process of its own under a time limit of its own; the parent stops at
the first child that fails or times out.

One evaluation (ℓπ and g) of (n_obs, P_x, C) = (4096, 32, 4) at N = 16 384 in Float64 against K = 3 evaluations of the unchanged
bernoulli_logit target at the same (n_obs, P_x, N) in the same build.  Two children per family:
  * events: two events on the context's stream around `--evals` leapfrogs after 5 of warm-up.  A leapfrog is one evaluation plus the
    position and momentum updates on (D, N), 1/128 of the elements of U here, for both targets alike;
  * trace: the same leapfrogs under `rocprofv3 --kernel-trace --stats`: the mean duration of every GLM kernel, which says where an
    evaluation's time goes.
The expectation (stated in the issue before any measurement): the same MFMA work as the three Bernoulli evaluations, plus a second exp
per element, a log, a division and one more pass over η: a ratio at or below about 1.5.
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

OUT = os.path.join(ROOT, "test_out", "glm_categorical_cost.json")
SHAPE = (4096, 32, 4, 16384)   # n_obs, P_x, C, N


def child(family, evals, events):
    import torch

    import ahmc_amd as A

    n_obs, Px, Cn, N = SHAPE
    rs = np.random.default_rng(0)
    X = rs.normal(size=(n_obs, Px)) / np.sqrt(Px)
    if family == "categorical_logit":
        eta = np.column_stack([np.zeros(n_obs), X @ rs.normal(size=(Px, Cn - 1))])
        y = (eta + rs.gumbel(size=eta.shape)).argmax(axis=1)
        t = A.GLMTarget(X, y, family=family, n_categories=Cn, prior_prec=np.ones((Cn - 1) * Px))
    else:
        y = (X @ rs.normal(size=Px) + rs.logistic(size=n_obs) > 0).astype(np.float64)
        t = A.GLMTarget(X, y, family=family, prior_prec=np.ones(Px))
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((t.D, N)), t), N, dtype=np.float64, rng=1, lib=A.load_hip_library())
    e.set_integrator(A.Leapfrog(0.01))
    e.set_position(0.1 * np.random.default_rng(1).normal(size=(t.D, N)))
    e.step(5)
    e.sync()
    if events:
        stream = torch.cuda.ExternalStream(int(e.lib.dll.ahmc_stream(e._ctx) or 0))
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        e.step(evals)
        t1.record(stream)
        e.sync()
        t1.synchronize()
        print("RESULT " + json.dumps({"family": family, "D": t.D, "evaluations": evals, "ms_per_evaluation": t0.elapsed_time(t1) / evals}), flush=True)
    else:
        e.step(evals)
        e.sync()
    e.close()


def run_child(argv, limit, trace):
    """one child of THIS file under its own time limit; with `trace` under rocprofv3's kernel statistics.  Raises on a failure: the
    caller stops there."""
    tmp = tempfile.mkdtemp(prefix="glm_categorical_prof_")
    try:
        cmd = [sys.executable, os.path.abspath(__file__), *argv]
        if trace:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "glm", "--output-format", "csv", "--", *cmd]
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
            if short.startswith(("k_glm_", "k_hglm_")):
                out[short] = {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) / 1e3, "total_us": int(row["Calls"]) * float(row["AverageNs"]) / 1e3}
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def cmd_all(args):
    n_obs, Px, Cn, N = SHAPE
    rec = {"n_obs": n_obs, "P_x": Px, "n_categories": Cn, "N": N, "dtype": "f64", "families": {},
           "method": f"two events on the context's stream around {args.evals} leapfrogs after 5 of warm-up, one child process per family; per-kernel "
                     "means from rocprofv3 --kernel-trace --stats in children of their own; one build, one session",
           "expectation": "ratio at or below about 1.5 (stated before any measurement)"}
    for fam in ("bernoulli_logit", "categorical_logit"):
        r = run_child(["child", "--family", fam, "--evals", str(args.evals), "--events", "1"], 300, False)
        r["kernels"] = run_child(["child", "--family", fam, "--evals", str(args.evals), "--events", "0"], 300, True)
        n_leap = args.evals + 5
        r["kernel_us_per_evaluation"] = {k: v["total_us"] / n_leap for k, v in r["kernels"].items()}
        rec["families"][fam] = r
        print(json.dumps({k: v for k, v in r.items() if k != "kernels"}), flush=True)
    K = Cn - 1
    cat, ber = rec["families"]["categorical_logit"]["ms_per_evaluation"], rec["families"]["bernoulli_logit"]["ms_per_evaluation"]
    rec["categorical_ms"] = cat
    rec["bernoulli_ms_times_K"] = K * ber
    rec["ratio"] = cat / (K * ber)
    print(json.dumps({"categorical_ms": cat, "bernoulli_ms_times_K": K * ber, "ratio": rec["ratio"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("all", "child"))
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--evals", type=int, default=20)
    ap.add_argument("--family", default="categorical_logit")
    ap.add_argument("--events", type=int, default=1)
    args = ap.parse_args()
    if args.what == "child":
        child(args.family, args.evals, bool(args.events))
    else:
        cmd_all(args)


if __name__ == "__main__":
    main()
