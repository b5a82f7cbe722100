"""Cost of the ordered-logit family (include/ahmc_glm_ordinal.h) → profiles/glm_ordinal_rates.json.

    python scripts/glm_ordinal_bench.py all [--out FILE] [--steps 12]

The parent never opens the GPU.  Every measurement is a child process of its own under a time limit of its own
(`rocprofv3 --kernel-trace --stats`, as scripts/glm_aux_bench.py); the parent stops at the first child that fails or times out.

One child per (shape, element type, family) at the three shapes of DESIGN §14's table: bernoulli_logit (0) and ordered_logit (5) with
C = 5 on the same predictors — the k_glm_eta instantiations of ONE build in one session — and C = 16 at the first shape.  Reported: the
duration of k_glm_eta per family, FAM 5 − FAM 0 in µs and in ns per (observation, chain) element, and the shares of k_glm_cut and
k_hglm_finish_ord in an evaluation (all GLM kernels of a leapfrog).  The expectation (stated before the run): the FAM 5
epilogue is link-bound like FAM 0 with two softplus / σ pairs per element instead of one, so FAM 5 − FAM 0 is about one more FAM 0
link per element, nearly independent of K = P, and grows with C only through the C − 1 select-sums.
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

OUT = os.path.join(ROOT, "profiles", "glm_ordinal_rates.json")


def child(n_obs, P, N, dt, steps, n_cat):
    """n_cat = 0: bernoulli_logit on the same predictors"""
    import ahmc_amd as A

    rs = np.random.default_rng(0)
    X = rs.normal(size=(n_obs, P)) / np.sqrt(P)
    lat = X @ rs.normal(size=P) + rs.logistic(size=n_obs)
    if n_cat:
        y = (lat.reshape(-1, 1) > np.linspace(-1.5, 1.5, n_cat - 1)).sum(axis=1)
        t = A.GLMTarget(X, y, family="ordered_logit", n_categories=n_cat, prior_prec=np.ones(P))
    else:
        t = A.GLMTarget(X, (lat > 0).astype(np.float64), family="bernoulli_logit", prior_prec=np.ones(P))
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((t.D, N)), t), N, dtype=GB.DTYPES[dt], rng=1, lib=A.load_hip_library())
    e.set_integrator(A.Leapfrog(0.01))
    e.set_position(0.1 * np.random.default_rng(1).normal(size=(t.D, N)))
    e.step(steps)
    e.sync()
    e.close()


def run_child(argv, limit):
    """one child of THIS file under its own time limit and rocprofv3's kernel statistics (as glm_aux_bench.run_child).  Raises on a
    failure: the caller stops there."""
    tmp = tempfile.mkdtemp(prefix="glm_ordinal_prof_")
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
    cases = [(s, 5) for s in GB.SHAPES] + [(GB.SHAPES[0], 16)]
    for (n_obs, P, N), n_cat in cases:
        for dt in GB.DTYPES:
            row = dict(n_obs=n_obs, P=P, N=N, dtype=dt, n_categories=n_cat, families={})
            for name, nc in (("bernoulli_logit", 0), ("ordered_logit", n_cat)):
                st = {k: v for k, v in run_child(["child", "--n_obs", str(n_obs), "--P", str(P), "--N", str(N), "--dtype", dt, "--steps", str(args.steps),
                                                  "--n_cat", str(nc)], 300).items() if k.startswith(("k_glm_", "k_hglm_"))}
                eta = [v for k, v in st.items() if k.startswith("k_glm_eta<")]
                assert len(eta) == 1, list(st)
                ev = sum(v["mean_us"] for v in st.values())
                share = lambda pre: next((v["mean_us"] / ev for k, v in st.items() if k.startswith(pre)), None)  # noqa: E731
                row["families"][name] = dict(eta_us=eta[0]["mean_us"], evaluation_us=ev, kernels=st, cut_share=share("k_glm_cut<"),
                                             finish_share=share("k_hglm_finish_ord<"))
            f = row["families"]
            elems = n_obs * N
            row["ordinal_minus_bernoulli_us"] = f["ordered_logit"]["eta_us"] - f["bernoulli_logit"]["eta_us"]
            row["ordinal_minus_bernoulli_ns_per_element"] = row["ordinal_minus_bernoulli_us"] * 1e3 / elems
            row["ordinal_over_bernoulli"] = f["ordered_logit"]["eta_us"] / f["bernoulli_logit"]["eta_us"]
            row["evaluation_ordinal_over_bernoulli"] = f["ordered_logit"]["evaluation_us"] / f["bernoulli_logit"]["evaluation_us"]
            rows.append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "families"} | {n: round(v["eta_us"], 1) for n, v in f.items()}), flush=True)
            GB.merge(args.out, "eta_by_family", {"rows": rows, "method": "rocprofv3 --kernel-trace --stats, one child per shape, element type and family, "
                                                 f"{args.steps} leapfrogs; the k_glm_eta<T, 0, BN> and k_glm_eta<T, 5, BN> instantiations of one build in one session",
                                                 "expectation": "FAM 5 − FAM 0 about one more FAM 0 link per (observation, chain) element, nearly independent of K = P; it "
                                                                "grows with C only through the C − 1 select-sums (stated before any measurement)"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("all", "child"))
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--n_obs", type=int)
    ap.add_argument("--P", type=int)
    ap.add_argument("--N", type=int)
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--n_cat", type=int, default=5)
    args = ap.parse_args()
    if args.what == "child":
        child(args.n_obs, args.P, args.N, args.dtype, args.steps, args.n_cat)
    else:
        cmd_all(args)


if __name__ == "__main__":
    main()
