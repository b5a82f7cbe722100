"""Cost of ahmc_glm_yrep / ahmc_glm_yrep_at (include/ahmc_glm_yrep.h) → profiles/glm_yrep_rates.json.

    python scripts/glm_yrep_bench.py all [--out FILE]

The parent never opens the GPU.  Every cell is a child process of its own under a time limit of its own, run ONCE under
`rocprofv3 --kernel-trace` (no counters in that run); the parent stops at the first child that fails or times out.

A model cell: (n, P, columns) of DESIGN §14, one of four families, Float64 or Float32.  The child binds the model on n training rows and
calls, on the same rows and `columns` draws in device memory, with the chunk forced to all columns so that each call is one launch of
each kernel: ahmc_glm_predict(MEAN) — one launch of k_glm_pred, whose device code this header does not touch: the yardstick — and
ahmc_glm_yrep: k_glm_pred for the planes the sampler reads, then k_glm_yrep.  The Poisson and negative-binomial cells carry an offset of
3, so that the rates straddle 10 and most waves hold lanes of both Poisson branches.
The sampler cell: ahmc_glm_yrep_at on 2²² elements per launch — every family at fixed parameters, and for the Poisson the cost of a wave
of mixed rates against uniform ones: λ = 0.5 everywhere, λ = 37 everywhere, the two alternating lane by lane (every wave runs both
branches), and the two in halves (every wave uniform).
The expectations (stated before the first run; none is a gate): ahmc_glm_yrep <= 1.5 × ahmc_glm_predict(MEAN) for Bernoulli
and Gaussian, <= 2.5 × for the count families; a wave of mixed rates costs at most the sum of the two uniform ones.
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

OUT = os.path.join(ROOT, "profiles", "glm_yrep_rates.json")
SHAPES = ((8192, 256, 8192), (65536, 64, 4096))
FAMILIES = ("bernoulli_logit", "gaussian_identity", "poisson_log", "negbinomial_log")
BARS = {"bernoulli_logit": 1.5, "gaussian_identity": 1.5, "poisson_log": 2.5, "negbinomial_log": 2.5}
COPY_TBS = 6.29   # the chip's copy rate
N_AT = 1 << 22


def child(n, P, cols, family, dtname):
    import ctypes as C

    import torch

    import ahmc_amd as A

    dtype = np.dtype(dtname)
    rs = np.random.default_rng(0)
    X = rs.normal(size=(n, P)) / np.sqrt(P)
    beta = rs.normal(size=P)
    counts = family in ("poisson_log", "negbinomial_log")
    if family == "bernoulli_logit":
        y = (X @ beta + rs.logistic(size=n) > 0).astype(np.float64)
    elif counts:
        y = rs.poisson(np.exp(X @ beta)).astype(np.float64)
    else:
        y = X @ beta + rs.normal(size=n)
    t = A.GLMTarget(X, y, family=family, prior_scale=2.5)
    N = 64
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((t.D, N)), t), N, dtype=dtype, rng=1, lib=A.load_hip_library())
    centre = np.concatenate([beta, [1.0]]) if t.aux else beta
    draws = torch.from_numpy(np.ascontiguousarray((centre[:, None] + 0.05 * rs.normal(size=(t.D, cols))).T.astype(dtype))).cuda()   # (cols, D) row-major
    nd = A.GLMNewData(X, offset=np.full(n, 3.0) if counts else None)
    os.environ["AHMC_GLM_PREDICT_CHUNK"] = str(cols)
    os.environ["AHMC_GLM_PREDICT_BUDGET"] = ""
    out = torch.empty(n * cols, dtype=torch.float64 if dtname == "float64" else torch.float32, device="cuda")
    rec, keep = e._glm_newdata("glm_yrep", nd)
    th = C.c_void_p(draws.data_ptr())
    torch.cuda.synchronize()
    e._call("ahmc_glm_predict", C.byref(rec), th, cols, A.capi.GLM_PRED_MEAN, C.c_void_p(out.data_ptr()))
    torch.cuda.synchronize()
    mu_mean = float(out[: n * 64].double().mean())
    e._call("ahmc_glm_yrep", C.byref(rec), th, cols, 1, C.c_void_p(out.data_ptr()))
    torch.cuda.synchronize()
    head = out[: n * 64].double()
    print("RESULT " + json.dumps({"mean_of_mu": mu_mean, "mean_of_yrep": float(head.mean()), "nan": int(torch.isnan(head).sum())}), flush=True)
    e.close()


AT_CELLS = (("bernoulli mu=0.3", 0, (0.3,), None, 0), ("gaussian", 2, (1.0, 4.0), None, 0), ("categorical C=5", 6, (0.1, 0.2, 0.3, 0.15, 0.25), None, 5),
            ("poisson lam=0.5", 1, (0.5,), None, 0), ("poisson lam=37", 1, (37.0,), None, 0), ("poisson 0.5/37 lane by lane", 1, "alternate", None, 0),
            ("poisson 0.5/37 in halves", 1, "halves", None, 0), ("poisson lam=1e6", 1, (1e6,), None, 0), ("negbinomial mu=3 phi=0.2", 4, (3.0,), float(np.log(0.2)), 0),
            ("negbinomial mu=50 phi=7", 4, (50.0,), float(np.log(7.0)), 0))


def child_at(dtname):
    import ctypes as C

    import torch

    import ahmc_amd as A

    dtype = np.dtype(dtname)
    e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((3, 4)), A.IsoGaussian(3)), 4, dtype=dtype, rng=1, lib=A.load_hip_library())
    n = N_AT
    res = {}
    tt = torch.float64 if dtname == "float64" else torch.float32
    y = torch.empty(n, dtype=tt, device="cuda")
    for name, fam, planes, s, Cc in AT_CELLS:
        if planes == "alternate":
            q = np.where(np.arange(n) % 2 == 0, 0.5, 37.0)[None]
        elif planes == "halves":
            q = np.where(np.arange(n) < n // 2, 0.5, 37.0)[None]
        else:
            q = np.repeat(np.asarray(planes)[:, None], n, axis=1)
        qd = torch.from_numpy(np.ascontiguousarray(q.T.astype(dtype))).cuda()            # (n, planes) row-major: the plane index fastest
        ad = None if s is None else torch.full((n,), s, dtype=tt, device="cuda")
        torch.cuda.synchronize()
        e._call("ahmc_glm_yrep_at", fam, Cc, n, C.c_void_p(qd.data_ptr()), None if ad is None else C.c_void_p(ad.data_ptr()), None, None, 1, C.c_void_p(y.data_ptr()))
        torch.cuda.synchronize()
        res[name] = {"mean": float(y.double().mean()), "nan": int(torch.isnan(y).sum())}
    print("RESULT " + json.dumps(res), flush=True)
    e.close()


def run_child(argv, limit):
    """(the child's RESULT, its kernel dispatches in order: [(short name, µs)])"""
    tmp = tempfile.mkdtemp(prefix="glm_yrep_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "-d", tmp, "-o", "yrep", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), *argv]
        res = subprocess.run(["timeout", "-k", "10", str(limit), *cmd], capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"child {argv} ended with status {res.returncode}: nothing more is started\n{res.stdout[-2000:]}\n{res.stderr[-3000:]}")
        result = json.loads(next(l for l in res.stdout.splitlines() if l.startswith("RESULT "))[7:])
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError(f"no kernel_trace.csv under {tmp}")
        rows = list(csv.DictReader(open(files[0])))
        cols = {c.lower(): c for c in rows[0]} if rows else {}
        name, start, end = (next((cols[c] for c in cols if w in c), None) for w in ("kernel_name", "start_timestamp", "end_timestamp"))
        if not (name and start and end):
            raise RuntimeError(f"kernel_trace.csv has the columns {sorted(cols.values())}")
        rows.sort(key=lambda r: int(r[start]))
        disp = [(r[name].split("(")[0].replace("void ", "").replace("ahmc::", ""), (int(r[end]) - int(r[start])) / 1e3) for r in rows]
        return result, [(k, us) for k, us in disp if k.startswith(("k_glm_pred<", "k_glm_yrep"))]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def load(path):
    try:
        return json.load(open(path))
    except (OSError, ValueError):
        return {}


def save(rec, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)


def cmd_all(args):
    rec = load(args.out)
    rec["method"] = ("kernel durations from ONE rocprofv3 --kernel-trace run per cell, a fresh child process per cell, one build, one session, one run per cell; "
                     "k_glm_pred of ahmc_glm_predict(MEAN) on the same shape in the same child is the yardstick (its device code is the parent's)")
    at = rec.setdefault("sampler", {})
    for dt in ("float64", "float32"):
        r, disp = run_child(["child_at", "--dtype", dt], 300)
        ys = [us for k, us in disp if k.startswith("k_glm_yrep<")]
        if len(ys) != len(AT_CELLS):
            raise RuntimeError(f"{len(ys)} launches of k_glm_yrep for {len(AT_CELLS)} cells")
        cell = {}
        for (name, fam, planes, s, Cc), us in zip(AT_CELLS, ys):
            n_planes = len(planes) if not isinstance(planes, str) else 1
            byte_us = N_AT * np.dtype(dt).itemsize * (n_planes + 1 + (s is not None)) / (COPY_TBS * 1e6)
            cell[name] = {"us": us, "ps_per_element": 1e6 * us / N_AT, "byte_model_us": byte_us, "over_byte_model": us / byte_us, **r[name]}
        u05, u37, mix, halves = (cell[k]["us"] for k in ("poisson lam=0.5", "poisson lam=37", "poisson 0.5/37 lane by lane", "poisson 0.5/37 in halves"))
        cell["divergence"] = {"mixed_wave_over_uniform_waves": mix / halves, "mixed_wave_over_sum_of_branches": mix / (u05 + u37),
                              "expectation (mixed <= sum of the two uniform launches)": "held" if mix <= u05 + u37 else "missed"}
        at[dt] = cell
        print(dt, json.dumps(cell), flush=True)
        save(rec, args.out)
    cells = rec.setdefault("cells", {})
    for (n, P, cols) in SHAPES:
        for fam in FAMILIES:
            for dt in ("float64", "float32"):
                key = f"({n}, {P}, {cols}) {fam} {dt}"
                r, disp = run_child(["child", "--shape", str(n), str(P), str(cols), "--family", fam, "--dtype", dt], 420)
                names = [k.split("<")[0] for k, _ in disp]
                if names != ["k_glm_pred", "k_glm_pred", "k_glm_yrep"]:
                    raise RuntimeError(f"{key}: unexpected launches {disp}")
                pred, planes_us, draw_us = (us for _, us in disp)
                elems = n * cols
                n_planes = 2 if fam == "gaussian_identity" else 1
                detour_us = elems * np.dtype(dt).itemsize * 2 * n_planes / (COPY_TBS * 1e6)     # the planes stored, then loaded
                ratio = (planes_us + draw_us) / pred
                cells[key] = {"predict_mean_us": pred, "yrep_planes_us": planes_us, "yrep_draw_us": draw_us, "yrep_over_predict_mean": ratio,
                              "draw_ps_per_element": 1e6 * draw_us / elems, "workspace_detour_byte_model_us": detour_us, "draw_over_detour": draw_us / detour_us,
                              f"expectation (yrep <= {BARS[fam]} x predict(MEAN))": "held" if ratio <= BARS[fam] else "missed", **r}
                print(key, json.dumps(cells[key]), flush=True)
                save(rec, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("all", "child", "child_at"))
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--shape", type=int, nargs=3, default=SHAPES[0])
    ap.add_argument("--family", default=FAMILIES[0])
    ap.add_argument("--dtype", default="float64")
    args = ap.parse_args()
    if args.what == "child":
        child(*args.shape, args.family, args.dtype)
    elif args.what == "child_at":
        child_at(args.dtype)
    else:
        cmd_all(args)


if __name__ == "__main__":
    main()
