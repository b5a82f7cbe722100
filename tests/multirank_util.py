"""Helper of tests/test_multirank_loopback.py (no tests in here): R worker processes that share one GPU and meet through the
stand-in communicator tests/host_ref/loopback_rccl.cpp, which the engine picks up through AHMC_RCCL_LIB — set in the CHILDREN's
environment only (the engine reads it once per process, and pytest's own process keeps the real RCCL).

`run_world(R, scenarios, tmp)` builds the stand-in (build cache, keyed on source and flags), creates the meeting file and the
128-byte ids, starts the R workers as fresh child processes of `sys.executable` running THIS file, waits for each under a time
limit of its own, kills the siblings of one that failed, and returns every rank's results.  A worker runs the whole LIST of
scenarios in one process, so the start-up (import torch, load the library) is paid once per world size.

The scenario functions and the engine set-ups live here, so that a worker and the single-process run it is compared with are
configured by the same code."""
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
LOOPBACK_SRC = os.path.join(HERE, "host_ref", "loopback_rccl.cpp")
DRIVER_SRC = os.path.join(HERE, "host_ref", "loopback_rccl_driver.cpp")
REGION_BYTES, GLOBAL_BYTES, N_REGIONS = 2 << 20, 4096, 24      # the layout of loopback_rccl.cpp
MAX_WORKERS = 3
N_ADAPTS, WINDOW_END = 150, 100                                 # Stan windows of 150 adaptations: 76 … 100, one split at 100
FAULTED = []                                                    # world sizes after which nothing more is started


def rocm_path():
    return os.environ.get("ROCM_PATH") or "/opt/rocm"


def _build(sources, flags, stem, shared):
    from ahmc_amd import build as B

    h = hashlib.sha256()
    for s in sources:
        with open(s, "rb") as f:
            h.update(f.read())
    h.update(" ".join(flags).encode())
    out_dir = os.path.join(B.OBJ, "host_ref")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, f"{stem}_{h.hexdigest()[:20]}" + (".so" if shared else ""))
    if not os.path.exists(out):
        cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
        tmp = out + f".tmp{os.getpid()}"
        res = subprocess.run([cxx, *flags, *sources, "-o", tmp], capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"building {stem} failed:\n{res.stdout}\n{res.stderr}")
        os.replace(tmp, out)
    return out


def loopback_lib():
    """the stand-in communicator as a shared object in the build cache, by the host compiler, linked against the HIP runtime"""
    rocm = rocm_path()
    flags = ["-O2", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-L{rocm}/lib", f"-Wl,-rpath,{rocm}/lib"]
    return _build([LOOPBACK_SRC], flags + ["-Wl,--no-as-needed", "-lamdhip64"], "loopback_rccl", True)


def loopback_driver(sanitize):
    """the host-buffer build of the stand-in with its stand-alone driver (own main); `sanitize`: -fsanitize=address,undefined"""
    flags = ["-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-DLOOPBACK_HOST_BUFFERS", f"-I{rocm_path()}/include"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"]
    return _build([LOOPBACK_SRC, DRIVER_SRC], flags, "loopback_driver_san" if sanitize else "loopback_driver", False)


def make_id(region, seed=0):
    """128 id bytes: the region of the meeting file in the first four, the rest opaque (to the stand-in as to the engine)"""
    rest = np.random.default_rng([region, seed]).integers(0, 256, 124, dtype=np.uint8).tobytes()
    return int(region).to_bytes(4, "little") + rest


# ------------------------------------------------------------------------------------------------------------------------
# engine set-ups shared by the workers and the single-process runs
# ------------------------------------------------------------------------------------------------------------------------
def spans_of(split):
    off, out = 0, []
    for cnt in split:
        out.append((off, int(cnt)))
        off += int(cnt)
    return out


def injected_feed(D, n_tot, dtype, seed):
    """(θ_i (D, n_tot) in the element type, α_i (n_tot,)) for i = 1 … WINDOW_END: what every global chain is handed, whatever the
    partition.  |mean| < the pooled sd in every dimension (the bound of the merge check is stated for such data)."""
    rs = np.random.default_rng(seed)
    scale = np.linspace(0.5, 3.0, D) if D > 1 else np.array([1.5])
    th = [(rs.normal(size=(D, n_tot)) * scale[:, None] + 0.25 * scale[:, None]).astype(dtype) for _ in range(WINDOW_END)]
    al = [rs.random(n_tot) for _ in range(WINDOW_END)]
    return th, al


def pooled_engine(A, lib, D, n_tot, off, cnt, dtype, seed, eps0=0.2, setup_seed=5):
    """StanHMCAdaptor(PooledVar, StepSizeAdaptor(0.8)) + NUTS on a DiagGaussian for chains [off, off + cnt) of n_tot: every
    per-chain quantity is drawn for ALL chains and cut, and the Philox streams are the global chains'"""
    full = np.random.default_rng(setup_seed)
    minv, th0, epsv = 0.5 + full.random(D), full.normal(size=(D, n_tot)), eps0 * (0.7 + 0.6 * full.random(n_tot))
    metric = A.DiagEuclideanMetric(minv.astype(dtype))
    h = A.Hamiltonian(metric, A.DiagGaussian(np.linspace(-1, 1, D) if D > 1 else np.array([0.3]), np.linspace(0.5, 2.0, D) if D > 1 else np.array([1.3])))
    lf = A.Leapfrog(epsv[off:off + cnt].astype(dtype))
    e = A.Engine(h, cnt, dtype=dtype, rng=A.PhiloxRNG(seed, chain_offset=off), lib=lib)
    e.set_integrator(lf)
    e.set_position(th0[:, off:off + cnt].astype(dtype))
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=6)))

    def init_adaptor():
        e.adaptor_init(A.StanHMCAdaptor(A.PooledVar(metric), A.StepSizeAdaptor(0.8, lf)))
    return e, k, init_adaptor


def shared_metric(e):
    """the (D,) M⁻¹ of a pooled adaptor (with one chain Engine.get_metric cannot tell (D, 1) from (D,))"""
    m = e.get_metric().reshape(-1).copy()
    assert m.shape == (e.D,), m.shape
    return m


def injected_part(A, lib, p, off, cnt, attach=None, calls=None):
    """scenario (a) for chains [off, off + cnt): the per-chain Welford states after i = 99, the 100th positions, the metric after
    i = 100, and (with `calls`) the all-gathers served before and during the pooled update"""
    dtype = np.dtype(p["dtype"])
    D, n_tot = p["D"], sum(p["split"])
    e, k, init_adaptor = pooled_engine(A, lib, D, n_tot, off, cnt, dtype, seed=1)
    if attach:
        attach(e)
    init_adaptor()
    th, al = injected_feed(D, n_tot, dtype, p["seed"])
    c0 = calls() if calls else 0
    for i in range(1, WINDOW_END):
        e.adapt(i, N_ADAPTS, theta=th[i - 1][:, off:off + cnt], alpha=al[i - 1][off:off + cnt])
    st = e.get_state()
    c1 = calls() if calls else 0
    e.adapt(WINDOW_END, N_ADAPTS, theta=th[-1][:, off:off + cnt], alpha=al[-1][off:off + cnt])
    metric = shared_metric(e)
    c2 = calls() if calls else 0
    assert st["adaptor"]["wv_n"] == WINDOW_END - 76, st["adaptor"]
    assert st["welford"].dtype == dtype and metric.dtype == dtype
    e.close()
    return {"mu": st["welford"][0], "M": st["welford"][1], "th_last": th[-1][:, off:off + cnt], "metric": metric,
            "allgathers": np.array([c1 - c0, c2 - c1])}


def run_part(A, lib, p, off, cnt, attach=None, torch=None, calls=None):
    """scenarios (b), (c), (d) for chains [off, off + cnt): the fused warm-up through the first window end, ten more draws, the
    gathered moments, the gathered state and what the communicator reported"""
    dtype = np.dtype(p["dtype"])
    D, n_tot, R = p["D"], sum(p["split"]), len(p["split"])
    e, k, init_adaptor = pooled_engine(A, lib, D, n_tot, off, cnt, dtype, seed=p["seed"])
    if attach:
        attach(e)
    init_adaptor()
    c0 = calls() if calls else 0
    e.run(k, WINDOW_END, N_ADAPTS)
    out = {"theta": e.theta().copy(), "stepsize": e.get_stepsize().copy(), "metric": shared_metric(e), "run_allgathers": np.array((calls() if calls else 0) - c0)}
    for key, v in e.stats().items():
        out["stat_" + key] = v

    def moments(tag):
        acc, g = e.accum(), e.gather_moments()
        out.update({tag + "acc_sum": acc["sum_theta"], tag + "acc_sumsq": acc["sumsq_theta"],
                    tag + "acc_counts": np.array([acc["n_transitions"] * cnt, acc["total_n_steps"], acc["n_divergent"]], dtype=np.int64),
                    tag + "g_mean": g["mean"], tag + "g_var": g["var"],
                    tag + "g_counts": np.array([g["n_draws"], g["total_n_steps"], g["n_divergent"]], dtype=np.int64)})
    moments("w_")            # of the 100 warm-up transitions: the chains are the single-process run's, so are the counts
    e.run(k, 10, 0)
    e.sync()
    out["theta2"], out["metric2"] = e.theta().copy(), shared_metric(e)
    moments("d_")            # of the ten draws after the pooled update
    if attach:
        ci = e.comm_info()
        out["comm_info"] = np.array([ci["ranks_seen"], ci["chains_total"], ci["chains_min"], ci["chains_max"]], dtype=np.int64)
        all_d = torch.full((R, cnt, D), float("nan"), dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")
        c0 = calls() if calls else 0
        rc = lib.dll.ahmc_gather_state(e._ctx, C.c_void_p(all_d.data_ptr()))
        out["gather_rc"], out["gather_allgathers"] = np.array(rc), np.array((calls() if calls else 0) - c0)
        out["gather_msg"] = np.array(lib.dll.ahmc_last_error(e._ctx).decode("utf-8", "replace") if rc else "")
        out["gathered"] = all_d.cpu().numpy()
        e.transition(k)      # a refusal (or a gather) leaves the context usable
        out["theta3"] = e.theta().copy()
    e.close()
    return out


# ------------------------------------------------------------------------------------------------------------------------
# the worker: `python multirank_util.py <spec.json>` with RANK / WORLD_SIZE / AHMC_RCCL_LIB / LOOPBACK_RCCL_FILE set
# ------------------------------------------------------------------------------------------------------------------------
class _Worker:
    def __init__(self, spec):
        import torch

        import ahmc_amd as A
        from ahmc_amd import _capi as capi

        self.A, self.capi, self.torch, self.spec = A, capi, torch, spec
        self.rank, self.world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
        assert torch.cuda.is_available(), "a worker needs the GPU"
        self.lib = A.load_hip_library()
        self.lb = C.CDLL(os.environ["AHMC_RCCL_LIB"])     # the same mapped copy the engine resolves its entry points from
        self.lb.loopback_calls.restype = C.c_long
        self.ids = [bytes.fromhex(x) for x in spec["ids"]]
        self.next_id = 0

    def fresh_id(self):
        """the next id of the list the parent made: every rank takes them in the same order, one per communicator"""
        self.next_id += 1
        return self.ids[self.next_id - 1]

    def attach(self, e, n=None):
        e.comm_init(self.fresh_id(), n or self.world, self.rank)

    def allgathers(self):
        return int(self.lb.loopback_calls(2))

    def span(self, p):
        return spans_of(p["split"])[self.rank]

    # (a)
    def injected(self, p):
        off, cnt = self.span(p)
        return injected_part(self.A, self.lib, p, off, cnt, attach=self.attach, calls=self.allgathers)

    # (b), (c), (d)
    def run(self, p):
        off, cnt = self.span(p)
        return run_part(self.A, self.lib, p, off, cnt, attach=self.attach, torch=self.torch, calls=self.allgathers)

    def _plain_engine(self, D=3, N=8, shared_metric=False):
        A = self.A
        metric = A.DiagEuclideanMetric(np.ones(D) if shared_metric else np.ones((D, N), order="F"))
        e = A.Engine(A.Hamiltonian(metric, A.IsoGaussian(D)), N, rng=3 + self.rank, lib=self.lib)
        lf = A.Leapfrog(np.full(N, 0.2))
        e.set_integrator(lf)
        e.set_position(np.random.default_rng(self.rank).normal(size=(D, N)))
        return e, A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn()))

    def _own_comm(self, n):
        class Uid(C.Structure):
            _fields_ = [("internal", C.c_char * 128)]

        self.lb.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, Uid, C.c_int]
        self.lb.ncclCommDestroy.argtypes = [C.c_void_p]
        comm = C.c_void_p()
        rc = self.lb.ncclCommInitRank(C.byref(comm), n, Uid(self.fresh_id()), self.rank)
        assert rc == 0 and comm.value, rc
        return comm

    # (e) attachment and ownership: every figure is returned, the parent asserts
    def ownership(self, p):
        live = lambda: int(self.lb.loopback_live_comms())  # noqa: E731
        out = {"live_start": live()}
        # a communicator of the caller's, handed over with ahmc_set_comm: not destroyed with the context
        comm = self._own_comm(self.world)
        e, k = self._plain_engine()
        e._call("ahmc_set_comm", comm, self.world, self.rank)
        out["set_comm_seen"] = e.comm_info()["ranks_seen"]
        out["live_attached"] = live()
        e.close()
        out["live_after_close_of_borrower"] = live()
        assert self.lb.ncclCommDestroy(comm) == 0
        out["live_after_own_destroy"] = live()
        # one made by ahmc_comm_init: destroyed with the context
        e, k = self._plain_engine()
        self.attach(e)
        out["live_owned"] = live()
        e.close()
        out["live_after_close_of_owner"] = live()
        # re-attaching releases the previous one; detaching (NULL) releases the last
        e, k = self._plain_engine()
        self.attach(e)
        self.attach(e)
        out["live_after_reattach"] = live()
        e._call("ahmc_set_comm", None, 1, 0)
        out["live_after_detach"] = live()
        e.transition(k)
        out["finite_after_detach"] = bool(np.isfinite(e.theta()).all())
        e.close()
        # a communicator of `world` ranks announced as world + 1
        comm = self._own_comm(self.world)
        e, k = self._plain_engine()
        out["announce_rc"] = self.lib.dll.ahmc_set_comm(e._ctx, comm, self.world + 1, self.rank)
        out["announce_msg"] = self.lib.dll.ahmc_last_error(e._ctx).decode("utf-8", "replace")
        self.lib.dll.ahmc_set_comm(e._ctx, None, 1, 0)
        e.transition(k)
        out["finite_after_announce"] = bool(np.isfinite(e.theta()).all())
        e.close()
        assert self.lb.ncclCommDestroy(comm) == 0
        out["live_end"] = live()
        return {k2: np.array(v) for k2, v in out.items()}

    # (f) what a context with a communicator of more than one rank refuses
    def refusals(self, p):
        capi, torch = self.capi, self.torch
        D, N, K = 3, 8, 16
        e, k = self._plain_engine(D, N, shared_metric=True)
        self.attach(e)
        draws = torch.randn((K, N, D), dtype=torch.float64, device="cuda")
        summ, rk = np.empty((9, D)), np.empty((K, N))
        out = {}

        def after(name, rc):
            out[name + "_rc"] = rc
            out[name + "_msg"] = self.lib.dll.ahmc_last_error(e._ctx).decode("utf-8", "replace")
            e.transition(k)
            out[name + "_finite_after"] = bool(np.isfinite(e.theta()).all())

        after("summary", self.lib.dll.ahmc_diag_summary(e._ctx, C.c_void_p(draws.data_ptr()), K, 0, capi.as_ptr(summ)))
        after("rank_normalize", self.lib.dll.ahmc_diag_rank_normalize(e._ctx, C.c_void_p(draws.data_ptr()), K, 0, 0, capi.as_ptr(rk)))
        assert self.lib.has_lowrank_adapt
        after("lowrank", self.lib.dll.ahmc_lowrank_adaptor_init(e._ctx, capi.ADAPT_STAN, 0.8, 75, 50, 25, 2, 2, 1))
        e.close()
        return {k2: np.array(v) for k2, v in out.items()}

    # (g) the one-rank run of tests/test_v3_state_gather.py through the stand-in
    def one_rank(self, p):
        from test_v3_state_gather import make

        e, k, h = make(self.lib, 24, 300, "stan_pooled", np.random.default_rng(8), shared_metric=True)
        e.comm_init(e.comm_unique_id(), 1, 0)     # the stand-in's own ncclGetUniqueId
        seen = e.comm_info()["ranks_seen"]
        c0 = self.allgathers()
        e.run(k, 110, N_ADAPTS)
        out = {"metric": e.get_metric().copy(), "theta": e.theta().copy(), "stepsize": e.get_stepsize().copy(), "ranks_seen": np.array(seen),
               "allgathers": np.array(self.allgathers() - c0)}
        e.close()
        out["live_end"] = np.array(int(self.lb.loopback_live_comms()))
        return out


def _worker_main(spec_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    with open(spec_path) as f:
        spec = json.load(f)
    w = _Worker(spec)
    res = {}
    for i, sc in enumerate(spec["scenarios"]):
        t0 = time.monotonic()
        for key, v in getattr(w, sc["kind"])(sc).items():
            res[f"{i}:{key}"] = v
        res[f"{i}:seconds"] = np.array(time.monotonic() - t0)
    np.savez(spec["out"] % w.rank, **res)


# ------------------------------------------------------------------------------------------------------------------------
# the parent side
# ------------------------------------------------------------------------------------------------------------------------
def run_world(R, scenarios, tmp, deadline_s=30, worker_timeout_s=240):
    """R workers over `scenarios` (a list of dicts with a "kind" naming a method of _Worker); returns one list per scenario of the
    R ranks' result dicts, and the seconds the slowest worker took.  Raises with the children's stderr when one fails; after a
    fault, abort or time-out nothing more is started."""
    assert 1 <= R <= MAX_WORKERS
    if FAULTED:
        raise RuntimeError(f"a worker of world size {FAULTED[0]} ended by a fault, abort or time-out: nothing more is started")
    tmp = str(tmp)
    so = loopback_lib()
    meet = os.path.join(tmp, "meeting.bin")
    with open(meet, "wb") as f:
        f.truncate(GLOBAL_BYTES + N_REGIONS * REGION_BYTES)      # zero-filled
    spec = {"scenarios": scenarios, "ids": [make_id(r, R).hex() for r in range(N_REGIONS - 4)], "out": os.path.join(tmp, "rank%d.npz")}
    spec_path = os.path.join(tmp, "spec.json")
    with open(spec_path, "w") as f:
        json.dump(spec, f)
    procs, logs = [], []
    t0 = time.monotonic()
    for r in range(R):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(R), AHMC_RCCL_LIB=so, LOOPBACK_RCCL_FILE=meet, LOOPBACK_RCCL_DEADLINE_S=str(deadline_s))
        log = open(os.path.join(tmp, f"rank{r}.log"), "w+")
        logs.append(log)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), spec_path], env=env, stdout=log, stderr=subprocess.STDOUT, cwd=tmp))
    codes = [None] * R
    bad = None
    while any(c is None for c in codes) and bad is None:
        for r, p in enumerate(procs):
            if codes[r] is not None:
                continue
            try:
                codes[r] = p.wait(timeout=0.1)
            except subprocess.TimeoutExpired:
                if time.monotonic() - t0 > worker_timeout_s:
                    codes[r] = "time-out"
            if codes[r] not in (None, 0):
                bad = r
                break
    for p in procs:            # the siblings of a failed worker would only wait for it until their deadline
        if p.poll() is None:
            p.kill()
        p.wait()
    seconds = time.monotonic() - t0
    if bad is not None:
        text = []
        for r, log in enumerate(logs):
            log.seek(0)
            text.append(f"--- rank {r} (exit {codes[r] if codes[r] is not None else 'killed after rank %d failed' % bad}) ---\n{log.read()[-3000:]}")
            log.close()
        if codes[bad] == "time-out" or (isinstance(codes[bad], int) and (codes[bad] < 0 or codes[bad] in (134, 139))):
            FAULTED.append(R)
        raise RuntimeError(f"world of {R}: rank {bad} ended with {codes[bad]}\n" + "\n".join(text))
    for log in logs:
        log.close()
    ranks = [dict(np.load(spec["out"] % r, allow_pickle=False)) for r in range(R)]
    out = []
    for i in range(len(scenarios)):
        out.append([{k.split(":", 1)[1]: v for k, v in rk.items() if k.startswith(f"{i}:")} for rk in ranks])
    return out, seconds


if __name__ == "__main__":
    _worker_main(sys.argv[1])
