#!/usr/bin/env python
"""Wide contexts (D > 4096, or AHMC_FORCE_WIDE=1) on the MI355X: NUTS(0.8) leapfrogs/s and k_w_target's own bandwidth.

    python scripts/wide_bench.py rates  [--out FILE]     # iso / hier Gaussian, f64: D = 4096 fused and forced wide, D = 8192, 32768
    python scripts/wide_bench.py kernel [--steps S]      # ahmc_leapfrog over every chain: run it under `rocprofv3 --kernel-trace --stats`

`rates`: N is sized so that one (D, N) vector is 1 GiB — four times the 256 MiB Infinity Cache — and the pool of the step-synchronous
engine then holds ~(2·max_depth + 3)·5 + max_depth + 2 of them.  Per configuration: find_good_stepsize, a StepSizeAdaptor(0.8) warm-up
of W transitions, then K timed draws (ahmc_sample, drop_warmup); leapfrogs = Σ n_steps of the draws (the accumulators).
`kernel`: S leapfrogs of every chain; each is one k_w_target launch over all N chains, whose byte model is θ′ read + g′ written
(2·D·N·sizeof(T), + 2·D·sizeof(T) of parameters for the diagonal Gaussian).  The script prints the model next to each configuration so
the trace's mean duration converts to bytes/s.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ahmc_amd as A  # noqa: E402

GIB = 1 << 30


def chains_for(D, itemsize=8):
    return max(1, GIB // (D * itemsize))


def target(name, D):
    return A.IsoGaussian(D) if name == "iso" else A.HierGaussian(D)


def engine(name, D, N, wide, lib, seed=1):
    if wide:
        os.environ["AHMC_FORCE_WIDE"] = "1"
    try:
        e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((D, N)), target(name, D)), N, rng=A.PhiloxRNG(seed), lib=lib)
    finally:
        os.environ.pop("AHMC_FORCE_WIDE", None)
    rs = np.random.default_rng(seed)
    th = np.asfortranarray(0.5 * rs.standard_normal((D, N)))
    e.set_integrator(A.Leapfrog(0.3 * D ** -0.25))
    e.set_position(th)
    return e


def rates(args, lib):
    configs = [(4096, False), (4096, True), (8192, True), (32768, True)]
    out = []
    for name in ("iso", "hier"):
        for D, force in configs:
            N = chains_for(D)
            if force or D > 4096:  # (wide: transitions per batch, which keeps the momentum buffers at 3·4 GiB beside the point pool)
                os.environ["AHMC_NUTS_BATCH"] = "4"
            else:
                os.environ.pop("AHMC_NUTS_BATCH", None)
            e = engine(name, D, N, force, lib)
            wide = e.info("wide")
            eps = e.find_good_stepsize()
            lf = A.Leapfrog(eps)
            e.set_integrator(lf)
            k = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=args.max_depth)))
            e.adaptor_init(A.StepSizeAdaptor(0.8, lf))
            W, K = args.warmup, args.draws
            e.run(k, W, W)
            e.sync()
            t0 = time.perf_counter()
            e.run(k, W + K, W, drop_warmup=True, i_first=W + 1)
            e.sync()
            dt = time.perf_counter() - t0
            acc = e.accum(moments=False)
            st = e.stats(["tree_depth", "acceptance_rate"])
            rec = {"target": name, "dtype": "f64", "D": D, "N": N, "path": "wide" if wide else "fused", "forced_wide": force, "max_depth": args.max_depth,
                   "warmup": W, "draws": K, "seconds": dt, "leapfrogs": acc["total_n_steps"], "leapfrogs_per_s": acc["total_n_steps"] / dt,
                   "mean_tree_depth_last": float(st["tree_depth"].mean()), "mean_accept_last": float(st["acceptance_rate"].mean())}
            print(json.dumps(rec), flush=True)
            out.append(rec)
            e.close()
    for name in ("iso", "hier"):
        f = [r for r in out if r["target"] == name and r["D"] == 4096 and r["path"] == "fused"]
        w = [r for r in out if r["target"] == name and r["D"] == 4096 and r["path"] == "wide"]
        if f and w:
            print(json.dumps({"target": name, "D": 4096, "forced_wide_over_fused": w[0]["leapfrogs_per_s"] / f[0]["leapfrogs_per_s"]}), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


def kernel(args, lib):
    for name, D in (("iso", 8192), ("hier", 8192), ("iso", 32768)):
        N = chains_for(D)
        e = engine(name, D, N, True, lib)
        assert e.info("wide") == 1
        e.step(2)  # (first-touch of the workspace)
        e.sync()
        t0 = time.perf_counter()
        e.step(args.steps)
        e.sync()
        dt = time.perf_counter() - t0
        print(json.dumps({"target": name, "D": D, "N": N, "steps": args.steps, "wall_s": dt, "k_w_target_bytes_per_launch": 2 * D * N * 8,
                          "kernel": f"k_w_target<double, {0 if name == 'iso' else 3}>"}), flush=True)
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("rates", "kernel"))
    ap.add_argument("--out", default="")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--draws", type=int, default=10)
    ap.add_argument("--max-depth", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    lib = A.load_hip_library()
    rates(args, lib) if args.mode == "rates" else kernel(args, lib)


if __name__ == "__main__":
    main()
