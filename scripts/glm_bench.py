"""Rates of GLMTarget (include/ahmc_glm.h) → profiles/glm_rates.json.

    python scripts/glm_bench.py all [--out FILE]     # everything below, one child process per measurement
    python scripts/glm_bench.py kernels | nuts | tail [--out FILE]

The parent never opens the GPU.  Every measurement is a child process of its own under a time limit of its own; the parent checks
each exit status and stops at the first child that fails or times out (nothing more is started on a card that may be in trouble).

  * kernels.  Durations of k_glm_eta, k_glm_grad (+ k_glm_gsum, k_glm_lp) from `rocprofv3 --kernel-trace --stats`, one child per
    (n_obs, D, N, element type): logit at (8192, 256, 8192), (65536, 64, 4096), (2048, 1024, 8192), 12 leapfrogs each.  TFLOP/s
    counts 2·n_obs·D flop per chain for each of the two products.  Beside them k_dgemm timed the same way in the same session
    (dense Gaussian target, D = 512, N = 8192): the yardstick the two kernels share their tile shape with.
  * nuts.  Whole-loop NUTS leapfrogs/s at (8192, 256, 8192) for GLMTarget and for the same model as the one-wave-per-chain
    KernelTarget of tests/user_targets/glm_kernel.hip, the two alternating in one child, `--repeats` windows each; median and spread.
  * tail.  The time of one evaluation (all GLM kernels of a leapfrog, kernel trace) with 16 and 64 chains at (8192, 256): the shape of
    the end of a NUTS batch.  K is always sliced (GLM_K_SLICE is part of the bit-level contract): there is no unsliced build to compare.
"""
import argparse
import csv
import ctypes as C
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

OUT = os.path.join(ROOT, "profiles", "glm_rates.json")
SHAPES = ((8192, 256, 8192), (65536, 64, 4096), (2048, 1024, 8192))
DTYPES = {"f64": np.float64, "f32": np.float32}


def merge(path, key, value):
    res = json.load(open(path)) if os.path.exists(path) else {}
    res[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


def model(n_obs, D, seed=0):
    rs = np.random.default_rng(seed)
    X = rs.normal(size=(n_obs, D)) / np.sqrt(D)
    y = (rs.random(n_obs) < 1 / (1 + np.exp(-(X @ rs.normal(size=D))))).astype(np.float64)
    return X, y, np.ones(D)


# ---- children (these open the GPU) ----
def child_glm(n_obs, D, N, dt, steps, family):
    import ahmc_amd as A

    X, y, p = model(n_obs, D)
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((D, N)), A.GLMTarget(X, y, family=family, prior_prec=p)), N, dtype=DTYPES[dt], rng=1, lib=A.load_hip_library())
    e.set_integrator(A.Leapfrog(0.01))
    e.set_position(0.1 * np.random.default_rng(1).normal(size=(D, N)))
    e.step(steps)
    e.sync()
    e.close()


def child_dgemm(D, N, steps):
    import ahmc_amd as A

    rs = np.random.default_rng(0)
    Q, _ = np.linalg.qr(rs.normal(size=(D, D)))
    P = np.asfortranarray((Q * np.linspace(0.5, 2.0, D)) @ Q.T)
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((D, N)), A.DenseGaussian((P + P.T) / 2)), N, rng=1, lib=A.load_hip_library())
    e.set_integrator(A.Leapfrog(0.01))
    e.set_position(0.1 * rs.normal(size=(D, N)))
    e.step(steps)
    e.sync()
    e.close()


class GlmUser(C.Structure):
    _fields_ = [("X", C.c_void_p), ("y", C.c_void_p), ("off", C.c_void_p), ("prec", C.c_void_p), ("U", C.c_void_p), ("n_obs", C.c_int64)]


def child_nuts(n_obs, D, N, dt, repeats, depth):
    import torch

    import ahmc_amd as A
    from ahmc_amd import _capi as capi
    from ahmc_amd.build import build_code_object
    from ahmc_amd.hipmod import Module

    hip = A.load_hip_library()
    dtype = DTYPES[dt]
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    X, y, p = model(n_obs, D)
    th0 = 0.1 * np.random.default_rng(1).normal(size=(D, N))
    mod = Module(build_code_object(os.path.join(ROOT, "tests", "user_targets", "glm_kernel.hip")))
    keep = [torch.from_numpy(np.ascontiguousarray(X.reshape(-1, order="F"))).to(tdt).cuda(), torch.from_numpy(y).to(tdt).cuda(),
            torch.from_numpy(p).to(tdt).cuda(), torch.empty(n_obs * N, dtype=tdt, device="cuda")]
    us = GlmUser(keep[0].data_ptr(), keep[1].data_ptr(), None, keep[2].data_ptr(), keep[3].data_ptr(), n_obs)
    us_d = torch.frombuffer(bytearray(bytes(us)), dtype=torch.uint8).cuda()
    targets = {"glm_target": A.GLMTarget(X, y, prior_prec=p),
               "kernel_target": A.KernelTarget(D, mod.function("glm_logit_" + dt), handle_kind=capi.KERNEL_HIP_FUNCTION, block_threads=256, chains_per_block=4,
                                               user=us_d.data_ptr())}
    kern = A.HMCKernel(A.Trajectory(A.MultinomialTS, A.Leapfrog(0.02), A.GeneralisedNoUTurn(max_depth=depth)))
    engines = {}
    for name, t in targets.items():
        e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((D, N)), t), N, dtype=dtype, rng=2, lib=hip)
        e.set_integrator(A.Leapfrog(0.02))
        e.set_position(th0)
        engines[name] = e
    lp = {name: e.phasepoint().lp.value for name, e in engines.items()}   # (the two evaluations of the same θ)
    for e in engines.values():
        e.run(kern, 1)
        e.sync()
    rates = {name: [] for name in engines}
    it = 2
    for _ in range(repeats):
        for name, e in engines.items():
            e.reset_accum()
            t = time.perf_counter()
            e.run(kern, it + 1, i_first=it)
            e.sync()
            rates[name].append(e.accum(moments=False)["total_n_steps"] / (time.perf_counter() - t))
        it += 2
    for e in engines.values():
        e.close()
    ratios = [a / b for a, b in zip(rates["glm_target"], rates["kernel_target"])]
    print("RESULT " + json.dumps(dict(n_obs=n_obs, D=D, N=N, dtype=dt, max_depth=depth, transitions_per_window=2, repeats=repeats,
                                      leapfrogs_per_s=rates, glm_over_kernel=ratios, median=statistics.median(ratios), min=min(ratios), max=max(ratios),
                                      lp_at_the_same_theta_max_relative_difference=float(np.max(np.abs(lp["glm_target"] - lp["kernel_target"]) / np.abs(lp["glm_target"]))))),
          flush=True)


# ---- the parent ----
def run_child(argv, limit, prof=False):
    """one child under its own time limit; rocprofv3's kernel statistics if `prof`.  Raises on a failure: the caller stops there."""
    tmp = tempfile.mkdtemp(prefix="glm_prof_")
    try:
        cmd = [sys.executable, os.path.abspath(__file__), *argv]
        if prof:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "glm", "--output-format", "csv", "--", *cmd]
        res = subprocess.run(["timeout", "-k", "10", str(limit), *cmd], capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"child {argv} ended with status {res.returncode}: nothing more is started\n{res.stdout[-2000:]}\n{res.stderr[-3000:]}")
        if not prof:
            return [json.loads(l[7:]) for l in res.stdout.splitlines() if l.startswith("RESULT ")]
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError(f"no kernel_stats.csv under {tmp}")
        out = {}
        for row in csv.DictReader(open(files[0])):
            short = row["Name"].split("(")[0].replace("void ", "").replace("ahmc::", "")
            out[short] = {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                          "max_us": float(row["MaxNs"]) / 1e3}
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def glm_kernels(st):
    return {k: v for k, v in st.items() if k.startswith("k_glm_")}


def cmd_kernels(args):
    st = run_child(["child-dgemm", "--D", "512", "--N", "8192", "--steps", str(args.steps)], 300, prof=True)
    name = [k for k in st if k.startswith("k_dgemm<")]
    assert len(name) == 1, list(st)
    dg = st[name[0]]
    yard = dict(kernel=name[0], D=512, N=8192, **dg, TFLOPs=2 * 512 * 512 * 8192 / dg["mean_us"] / 1e6)
    print(json.dumps(yard), flush=True)
    rows = []
    for n_obs, D, N in SHAPES:
        for dt in DTYPES:
            st = glm_kernels(run_child(["child-glm", "--n_obs", str(n_obs), "--D", str(D), "--N", str(N), "--dtype", dt, "--steps", str(args.steps)], 400, prof=True))
            flop = 2.0 * n_obs * D * N
            eta = [v for k, v in st.items() if k.startswith("k_glm_eta<")][0]
            grad = [v for k, v in st.items() if k.startswith("k_glm_grad<")][0]
            row = dict(n_obs=n_obs, D=D, N=N, dtype=dt, kernels=st, eta_TFLOPs=flop / eta["mean_us"] / 1e6, grad_TFLOPs=flop / grad["mean_us"] / 1e6,
                       evaluation_us=sum(v["mean_us"] for v in st.values()))
            if dt == "f64":
                row["eta_over_dgemm"] = row["eta_TFLOPs"] / yard["TFLOPs"]
                row["grad_over_dgemm"] = row["grad_TFLOPs"] / yard["TFLOPs"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    merge(args.out, "kernels", {"k_dgemm_same_session": yard, "rows": rows,
                                "method": "rocprofv3 --kernel-trace --stats, one child per shape and element type; 2·n_obs·D flop per chain per product",
                                "expectation": "within 15 % of k_dgemm at K >= 256 (from the shared tile shape; stated before any measurement)"})


def cmd_nuts(args):
    n_obs, D, N = SHAPES[0]
    rows = []
    for dt in DTYPES:
        rows += run_child(["child-nuts", "--n_obs", str(n_obs), "--D", str(D), "--N", str(N), "--dtype", dt, "--repeats", str(args.repeats), "--depth", "3"], 500)
        print(json.dumps(rows[-1]), flush=True)
    merge(args.out, "nuts", {"rows": rows, "method": "wall clock of windows of 2 NUTS transitions, the two targets alternating in one process"})


def cmd_tail(args):
    n_obs, D = 8192, 256
    rows = []
    for N in (16, 64):
        for dt in DTYPES:
            st = glm_kernels(run_child(["child-glm", "--n_obs", str(n_obs), "--D", str(D), "--N", str(N), "--dtype", dt, "--steps", str(args.steps)], 300, prof=True))
            rows.append(dict(n_obs=n_obs, D=D, running_chains=N, dtype=dt, kernels=st, evaluation_us=sum(v["mean_us"] for v in st.values())))
            print(json.dumps(rows[-1]), flush=True)
    merge(args.out, "tail", {"rows": rows, "k_slice": 1024,
                             "not_measured": "an unsliced K: GLM_K_SLICE is part of the bit-level contract, there is no build without it"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("all", "kernels", "nuts", "tail", "child-glm", "child-dgemm", "child-nuts"))
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n_obs", type=int)
    ap.add_argument("--D", type=int)
    ap.add_argument("--N", type=int)
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--family", default="bernoulli_logit")
    args = ap.parse_args()
    if args.what == "child-glm":
        child_glm(args.n_obs, args.D, args.N, args.dtype, args.steps, args.family)
    elif args.what == "child-dgemm":
        child_dgemm(args.D, args.N, args.steps)
    elif args.what == "child-nuts":
        child_nuts(args.n_obs, args.D, args.N, args.dtype, args.repeats, args.depth)
    else:
        for what in (("kernels", "tail", "nuts") if args.what == "all" else (args.what,)):
            {"kernels": cmd_kernels, "nuts": cmd_nuts, "tail": cmd_tail}[what](args)


if __name__ == "__main__":
    main()
