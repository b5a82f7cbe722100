"""Cost of ahmc_glm_predict / ahmc_glm_predict_summary (include/ahmc_glm_predict.h) → profiles/glm_predict_rates.json.

    python scripts/glm_predict_bench.py all [--out FILE]
    python scripts/glm_predict_bench.py run  [--out FILE]      # the whole call on the (D, N, K) buffer of a run: 8192 × 256, N = 8192, K = 100

The parent never opens the GPU.  Every cell is a child process of its own under a time limit of its own, run ONCE under
`rocprofv3 --kernel-trace --stats` (no counters in that run); the parent stops at the first child that fails or times out.

A cell: (n, P, columns) of DESIGN §14, bernoulli_logit or gaussian_identity, Float64 or Float32.  The child binds the model on n training
rows with N = columns chains and calls, on the same rows and `columns` draws in device memory: ahmc_glm_loglik (one launch of k_glm_eta:
the yardstick, device code untouched), ahmc_glm_predict_summary and ahmc_glm_predict(MEAN), both with the chunk forced to all columns so
that each is one launch of k_glm_pred.  The expectation (stated before the first run; not a gate): k_glm_pred<SUMMARY> <=
1.15 × k_glm_eta; the full-matrix path is reported against its byte model.
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

OUT = os.path.join(ROOT, "profiles", "glm_predict_rates.json")
SHAPES = ((8192, 256, 8192), (65536, 64, 4096), (2048, 1024, 8192))
FAMILIES = ("bernoulli_logit", "gaussian_identity")
COPY_TBS = 6.29   # the chip's copy rate
KERNELS = ("k_glm_eta<", "k_glm_pred<", "k_glm_pred_fold")


def setup(n, P, cols, family, dtname, N=None):
    import torch

    import ahmc_amd as A

    dtype = np.dtype(dtname)
    rs = np.random.default_rng(0)
    X = rs.normal(size=(n, P)) / np.sqrt(P)
    beta = rs.normal(size=P)
    y = (X @ beta + rs.logistic(size=n) > 0).astype(np.float64) if family == "bernoulli_logit" else X @ beta + rs.normal(size=n)
    t = A.GLMTarget(X, y, family=family, prior_scale=2.5)
    N = N or cols
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((t.D, N)), t), N, dtype=dtype, rng=1, lib=A.load_hip_library())
    draws = torch.from_numpy(np.ascontiguousarray((beta[:, None] + 0.05 * rs.normal(size=(P, cols))).T.astype(dtype))).cuda()   # (cols, D) row-major
    nd = A.GLMNewData(X, y=y)
    torch.cuda.synchronize()
    return A, torch, t, e, draws, nd


def child(n, P, cols, family, dtname):
    import ctypes as C

    A, torch, t, e, draws, nd = setup(n, P, cols, family, dtname)
    os.environ["AHMC_GLM_PREDICT_CHUNK"] = str(cols)
    os.environ["AHMC_GLM_PREDICT_BUDGET"] = ""
    tt = torch.float64 if dtname == "float64" else torch.float32
    out = torch.empty(n * cols, dtype=tt, device="cuda")
    summ = torch.empty(7 * n, dtype=torch.float64, device="cuda")
    rec, keep = e._glm_newdata("glm_predict", nd)
    th = C.c_void_p(draws.data_ptr())
    e._call("ahmc_glm_loglik", th, cols, C.c_void_p(out.data_ptr()))
    e._call("ahmc_glm_predict_summary", C.byref(rec), th, cols, C.cast(C.c_void_p(summ.data_ptr()), C.POINTER(C.c_double)))
    e._call("ahmc_glm_predict", C.byref(rec), th, cols, A.capi.GLM_PRED_MEAN, C.c_void_p(out.data_ptr()))
    torch.cuda.synchronize()
    s = summ.cpu().numpy().reshape(7, n, order="F")
    print("RESULT " + json.dumps({"lpd_sum": float(s[6].sum()), "mean_of_means": float(s[2].mean())}), flush=True)
    e.close()


def child_run(dtname):
    """the whole summary call on a (D, N, K) buffer: 8192 × 256, N = 8192, K = 100 draws a chain — S = 819 200 columns, default budget"""
    n, P, N, K = 8192, 256, 8192, 100
    A, torch, t, e, draws, nd = setup(n, P, N * K, "bernoulli_logit", dtname, N=N)
    ms = []
    for _ in range(2):
        t0 = time.perf_counter()
        s = e.glm_predict_summary(nd, draws.data_ptr(), n_cols=N * K)
        ms.append(1e3 * (time.perf_counter() - t0))
    print("RESULT " + json.dumps({"dtype": dtname, "S": N * K, "ms_per_call": ms, "lpd_sum": float(s["lpd"].sum())}), flush=True)
    e.close()


def run_child(argv, limit, trace):
    tmp = tempfile.mkdtemp(prefix="glm_predict_prof_")
    try:
        cmd = [sys.executable, os.path.abspath(__file__), *argv]
        if trace:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "pred", "--output-format", "csv", "--", *cmd]
        res = subprocess.run(["timeout", "-k", "10", str(limit), *cmd], capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"child {argv} ended with status {res.returncode}: nothing more is started\n{res.stdout[-2000:]}\n{res.stderr[-3000:]}")
        result = json.loads(next(l for l in res.stdout.splitlines() if l.startswith("RESULT "))[7:])
        if not trace:
            return result, {}
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError(f"no kernel_stats.csv under {tmp}")
        kern = {}
        for row in csv.DictReader(open(files[0])):
            short = row["Name"].split("(")[0].replace("void ", "").replace("ahmc::", "")
            if short.startswith(KERNELS):
                kern[short] = {"calls": int(row["Calls"]), "total_us": int(row["Calls"]) * float(row["AverageNs"]) / 1e3}
        return result, kern
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def load(path):
    try:
        return json.load(open(path))
    except (OSError, ValueError):
        return {}


def cmd_all(args):
    rec = load(args.out)
    rec["method"] = ("kernel durations from ONE rocprofv3 --kernel-trace --stats run per cell, a fresh child process per cell, one build, one session, one run per "
                     "cell; k_glm_eta of the same shape in the same child is the yardstick")
    cells = rec.setdefault("cells", {})
    for (n, P, cols) in SHAPES:
        for fam in FAMILIES:
            for dt in ("float64", "float32"):
                key = f"({n}, {P}, {cols}) {fam} {dt}"
                _, k = run_child(["child", "--shape", str(n), str(P), str(cols), "--family", fam, "--dtype", dt], 420, True)
                us = lambda pre, tail: sum(v["total_us"] for name, v in k.items() if name.startswith(pre) and name.rstrip(">").endswith(tail))  # noqa: E731
                eta, summ, full = us("k_glm_eta<", ""), us("k_glm_pred<", "true"), us("k_glm_pred<", "false")
                model_us = n * cols * np.dtype(dt).itemsize / (COPY_TBS * 1e6)
                cells[key] = {"kernels": k, "k_glm_eta_us": eta, "k_glm_pred_summary_us": summ, "k_glm_pred_full_us": full, "summary_over_eta": summ / eta if eta else None,
                              "expectation (summary <= 1.15 x k_glm_eta)": "held" if eta and summ <= 1.15 * eta else "missed",
                              "full_byte_model_us": model_us, "full_over_byte_model": full / model_us}
                print(key, json.dumps({kk: v for kk, v in cells[key].items() if kk != "kernels"}), flush=True)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump(rec, f, indent=1)


def cmd_run(args):
    rec = load(args.out)
    for dt in ("float64", "float32"):
        r, _ = run_child(["child_run", "--dtype", dt], 420, False)
        rec.setdefault("whole_call_on_a_run", {})[dt] = r
        print(json.dumps(r), flush=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("all", "run", "child", "child_run"))
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--shape", type=int, nargs=3, default=SHAPES[0])
    ap.add_argument("--family", default=FAMILIES[0])
    ap.add_argument("--dtype", default="float64")
    args = ap.parse_args()
    if args.what == "child":
        child(*args.shape, args.family, args.dtype)
    elif args.what == "child_run":
        child_run(args.dtype)
    else:
        {"all": cmd_all, "run": cmd_run}[args.what](args)


if __name__ == "__main__":
    main()
