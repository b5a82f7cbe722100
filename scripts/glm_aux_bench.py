"""Cost of the families with a sampled dispersion (include/ahmc_glm_aux.h) → profiles/glm_aux_rates.json.

    python scripts/glm_aux_bench.py all [--out FILE] [--steps 12]

The parent never opens the GPU.  Every measurement is a child process of its own under a time limit of its own
(`rocprofv3 --kernel-trace --stats`, as scripts/glm_bench.py); the parent stops at the first child that fails or times out.

One child per (shape, element type, family) at the three shapes of DESIGN §14's table: Poisson (1) and negative binomial (4) on the same
counts, Gaussian (2) and Gaussian with a sampled σ (3) on the same responses — the four k_glm_eta instantiations of ONE build.  Reported:
the duration of k_glm_eta per family, FAM 4 − FAM 1 and FAM 3 − FAM 2 in µs and in ns per (observation, chain) element, and the share of
k_hglm_finish_aux in an evaluation (all GLM kernels of a leapfrog).  The expectation (stated before the run): the NB
epilogue is link-bound, so FAM 4 − FAM 1 per element is roughly constant across K = P.
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

import glm_bench as GB  # noqa: E402  (the shapes, the element types, merge)

OUT = os.path.join(ROOT, "profiles", "glm_aux_rates.json")
FAMILIES = {1: "poisson_log", 4: "negbinomial_log", 2: "gaussian_identity", 3: "gaussian_identity_sigma"}


def child(n_obs, P, N, dt, steps, fam):
    import ahmc_amd as A

    rs = np.random.default_rng(0)
    X = rs.normal(size=(n_obs, P)) / np.sqrt(P)
    eta = X @ rs.normal(size=P)
    y = rs.negative_binomial(3.0, 3.0 / (3.0 + np.exp(eta))).astype(np.float64) if fam in (1, 4) else eta + 0.7 * rs.normal(size=n_obs)
    t = A.GLMTarget(X, y, family=FAMILIES[fam], prior_prec=np.ones(P))
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((t.D, N)), t), N, dtype=GB.DTYPES[dt], rng=1, lib=A.load_hip_library())
    e.set_integrator(A.Leapfrog(0.01))
    e.set_position(0.1 * np.random.default_rng(1).normal(size=(t.D, N)))
    e.step(steps)
    e.sync()
    e.close()


def run_child(argv, limit):
    """one child of THIS file under its own time limit and rocprofv3's kernel statistics (as glm_bench.run_child).  Raises on a
    failure: the caller stops there."""
    tmp = tempfile.mkdtemp(prefix="glm_aux_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "glm", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), *argv]
        res = subprocess.run(["timeout", "-k", "10", str(limit), *cmd], capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"child {argv} ended with status {res.returncode}: nothing more is started\n{res.stdout[-2000:]}\n{res.stderr[-3000:]}")
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


def cmd_all(args):
    rows = []
    for n_obs, P, N in GB.SHAPES:
        for dt in GB.DTYPES:
            row = dict(n_obs=n_obs, P=P, N=N, dtype=dt, families={})
            for fam in FAMILIES:
                st = {k: v for k, v in run_child(["child", "--n_obs", str(n_obs), "--P", str(P), "--N", str(N), "--dtype", dt, "--steps", str(args.steps),
                                                  "--family", str(fam)], 300).items() if k.startswith(("k_glm_", "k_hglm_"))}
                eta = [v for k, v in st.items() if k.startswith("k_glm_eta<")]
                assert len(eta) == 1, list(st)
                ev = sum(v["mean_us"] for v in st.values())
                fin = [v["mean_us"] for k, v in st.items() if k.startswith("k_hglm_finish_aux<")]
                row["families"][FAMILIES[fam]] = dict(eta_us=eta[0]["mean_us"], evaluation_us=ev, kernels=st,
                                                     finish_share=(fin[0] / ev if fin else None))
            f = row["families"]
            elems = n_obs * N
            row["nb_minus_poisson_us"] = f["negbinomial_log"]["eta_us"] - f["poisson_log"]["eta_us"]
            row["nb_minus_poisson_ns_per_element"] = row["nb_minus_poisson_us"] * 1e3 / elems
            row["nb_over_poisson"] = f["negbinomial_log"]["eta_us"] / f["poisson_log"]["eta_us"]
            row["sigma_minus_gaussian_us"] = f["gaussian_identity_sigma"]["eta_us"] - f["gaussian_identity"]["eta_us"]
            row["sigma_over_gaussian"] = f["gaussian_identity_sigma"]["eta_us"] / f["gaussian_identity"]["eta_us"]
            rows.append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "families"} | {n: (round(v["eta_us"], 1), v["finish_share"]) for n, v in f.items()}), flush=True)
            GB.merge(args.out, "eta_by_family", {"rows": rows, "method": "rocprofv3 --kernel-trace --stats, one child per shape, element type and family, "
                                                 f"{args.steps} leapfrogs; the four k_glm_eta instantiations of one build",
                                                 "expectation": "NB − Poisson per (observation, chain) element roughly constant across K = P: the NB epilogue is "
                                                                "link-bound (stated before any measurement)"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("all", "child"))
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--n_obs", type=int)
    ap.add_argument("--P", type=int)
    ap.add_argument("--N", type=int)
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--family", type=int, default=4)
    args = ap.parse_args()
    if args.what == "child":
        child(args.n_obs, args.P, args.N, args.dtype, args.steps, args.family)
    else:
        cmd_all(args)


if __name__ == "__main__":
    main()
