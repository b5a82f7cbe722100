#!/usr/bin/env python
"""ahmc_diag_summary (include/ahmc_diag.h) on the MI355X: whole-call time and a per-kernel breakdown, on synthetic AR(1) draws.

    python scripts/diag_bench.py all    [--out profiles/diag_rates.json]   # both shapes: timings + one rocprofv3 run per shape
    python scripts/diag_bench.py rates  [--shape cfg2|wide] [--reps R]      # whole-call time only
    python scripts/diag_bench.py kernel --shape cfg2|wide                   # one call: run it under `rocprofv3 --kernel-trace --stats`

Shapes: cfg2 = D 128 × N 65 536 × K 1 000, f64 (the 67 GB draws buffer of bench.py's cfg2), and wide = D 8 192 × N 256 × K 1 000.
The draws are AR(1) with φ = 0.5 per (dimension, chain), synthesised on the device in ahmc_sample's (D, N, K) layout (the sampler
does not run).  The sort's byte model per 8-bit pass and key: the histogram reads the key, the scatter reads and writes key + u32
index; its rate is compared with the 6.29 TB/s device copy rate of DESIGN §10.6.
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

SHAPES = {"cfg2": (128, 65536, 1000), "wide": (8192, 256, 1000)}
COPY_RATE = 6.29e12


def synth(D, N, K, phi=0.5, seed=0):
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.empty((K, N, D), dtype=torch.float64, device="cuda")
    x[0] = torch.randn((N, D), generator=g, device="cuda", dtype=torch.float64) / (1 - phi * phi) ** 0.5
    for k in range(1, K):
        x[k] = phi * x[k - 1] + torch.randn((N, D), generator=g, device="cuda", dtype=torch.float64)
    torch.cuda.synchronize()
    return x


def timed(shape, reps):
    D, N, K = SHAPES[shape]
    x = synth(D, N, K)
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric(D), A.IsoGaussian(D)), N)
    ts, r = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = e.summarystats(x.data_ptr(), K)
        ts.append(time.perf_counter() - t0)
    e.close()
    S = 2 * N * (K // 2)
    return {"shape": shape, "D": D, "N": N, "K": K, "dtype": "f64", "draws_bytes": D * N * K * 8, "values_per_dimension": S,
            "call_s": ts, "call_s_min": min(ts), "ess_bulk_over_S_mean": float(np.nanmean(r["ess_bulk"]) / S),
            "ess_basic_over_S_mean": float(np.nanmean(r["ess_basic"]) / S), "rhat_max": float(np.nanmax(r["rhat"]))}


def kernel_stats(shape):
    """one call under rocprofv3 --kernel-trace --stats (a fresh child process) → {kernel: {calls, total_ns}}"""
    tmp = tempfile.mkdtemp(prefix="diag_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "diag", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "kernel", "--shape", shape]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if res.returncode != 0:
            raise RuntimeError(f"rocprofv3 failed ({res.returncode}):\n{res.stderr[-3000:]}")
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError(f"no kernel_stats.csv under {tmp}")
        out = {}
        for row in csv.DictReader(open(files[0])):
            name = row["Name"]
            short = name.split("(")[0].replace("void ", "").replace("ahmc::diag::", "")
            rec = out.setdefault(short, {"calls": 0, "total_ns": 0})
            rec["calls"] += int(row["Calls"])
            rec["total_ns"] += int(float(row["TotalDurationNs"]))
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def sort_rate(stats, D, S, key_bytes=8):
    passes = 8 * key_bytes // 8
    keys = D * S
    nbytes = passes * keys * (key_bytes + 2 * (key_bytes + 4))
    ns = sum(v["total_ns"] for k, v in stats.items() if k.startswith(("k_dg_hist", "k_dg_scatter")) or "GenArray" in k)
    return {"sort_bytes": nbytes, "sort_kernel_s": ns * 1e-9, "sort_bytes_per_s": nbytes / (ns * 1e-9) if ns else None,
            "fraction_of_copy_rate": nbytes / (ns * 1e-9) / COPY_RATE if ns else None, "copy_rate_bytes_per_s": COPY_RATE}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["all", "rates", "kernel"])
    ap.add_argument("--shape", choices=sorted(SHAPES), default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_rates.json"))
    args = ap.parse_args()
    shapes = [args.shape] if args.shape else ["cfg2", "wide"]
    if args.mode == "kernel":
        D, N, K = SHAPES[shapes[0]]
        x = synth(D, N, K)
        e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric(D), A.IsoGaussian(D)), N)
        e.summarystats(x.data_ptr(), K)
        e.close()
        return
    recs = []
    for sh in shapes:
        rec = timed(sh, args.reps)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if args.mode == "rates":
        return
    for rec in recs:
        st = kernel_stats(rec["shape"])
        rec["kernels"] = dict(sorted(st.items(), key=lambda kv: -kv[1]["total_ns"]))
        rec["kernel_total_s"] = sum(v["total_ns"] for v in st.values()) * 1e-9
        rec.update(sort_rate(st, rec["D"], rec["values_per_dimension"]))
        print(json.dumps({k: v for k, v in rec.items() if k != "kernels"}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"what": "ahmc_diag_summary on AR(1) draws (phi = 0.5), f64; call_s: wall time of whole calls; kernels: one call under "
                           "rocprofv3 --kernel-trace --stats", "shapes": recs}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
