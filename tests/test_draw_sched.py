"""The launch-length controller of the sampling phase (csrc/ahmc_draw_sched.hpp) decides what the search decided while it was
written out inside the sampling loop — on a CPU, without a clock.

tests/host_ref/draw_sched_driver.cpp drives the header through whole calls the way csrc/ahmc_sample_host.hpp does, with a table
launch length -> throughput in the place of the measurement.  The expectation, tests/golden/draw_sched_traces.json, was written
by tests/golden/make_draw_sched_traces.py: a Python transcription of the loop BEFORE the controller was taken out of it, not of
the header.  Every field of every launch must agree: (transitions, timed or not, phase after it, best length after it).

Grid: (left, batch) in {(300, 256), (1000, 256), (2000, 256), (1000, 32), (300, 6), (40, 256)} x the switch variants of
tests/test_pipeline_parity.py's SCHEDULES x five throughput models (1/len, len, constant, a peak at 64, a peak at 16); the dispatch
order already on measured work at entry; a scalar step size; two calls on one context, the first cut off inside a timed group.
"""
import ctypes as C
import functools
import hashlib
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "host_ref", "draw_sched_driver.cpp")
CSRC = os.path.join(ROOT, "advancedhmc.jl_amd", "csrc")
HEADER = os.path.join(CSRC, "ahmc_draw_sched.hpp")
TRACES = os.path.join(ROOT, "tests", "golden", "draw_sched_traces.json")

MODELS = {
    "inv_len": lambda L: 1.0 / L,
    "len": lambda L: float(L),
    "const": lambda L: 1.0,
    "peak64": lambda L: 1.0 - 0.1 * abs(math.log2(L) - 6.0),
    "peak16": lambda L: 1.0 - 0.1 * abs(math.log2(L) - 4.0),
}
N_THR = 2049   # launch lengths the tables cover (the longest run of the grid is 2 000 transitions)


@functools.lru_cache(maxsize=None)
def driver():
    """tests/host_ref/draw_sched_driver.cpp as its own shared object in the build cache, by the host compiler (as
    tests/test_glm_target.py builds its host reference; keyed on the controller's header as well)"""
    from ahmc_amd import build as B

    flags = ["-O2", "-march=native", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off"]
    with open(DRIVER, "rb") as f, open(HEADER, "rb") as g:
        h = hashlib.sha256(f.read() + g.read() + " ".join(flags).encode()).hexdigest()[:20]
    out_dir = os.path.join(B.OBJ, "host_ref")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, f"draw_sched_driver_{h}.so")
    if not os.path.exists(so):
        cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
        tmp = so + f".tmp{os.getpid()}"
        res = subprocess.run([cxx, *flags, "-I", CSRC, DRIVER, "-o", tmp], capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"draw_sched_driver build failed:\n{res.stdout}\n{res.stderr}")
        os.replace(tmp, so)
    dll = C.CDLL(so)
    dll.draw_sched_run.restype = C.c_int64
    dll.draw_sched_run.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32,
                                   C.c_void_p, C.POINTER(C.c_double), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
    return dll


@functools.lru_cache(maxsize=None)
def table(model):
    return np.array([0.0] + [MODELS[model](L) for L in range(1, N_THR)], dtype=np.float64)


def replay(trace):
    """the trace's calls through the driver -> per call (launches [(k, probing, phase, best_len)], g_left after)"""
    draw_batch, sched, order_refresh, first_batch = trace["sw"]
    state = np.zeros(6, dtype=np.int64)          # phase, len, best_len, primed, g_len, g_left: a fresh context
    best_thr = C.c_double(0.0)
    ofw = C.c_int32(trace["order_from_work"])
    thr = table(trace["model"])
    calls = []
    for call in trace["calls"]:
        cap = call["left"] if call["cut"] is None else call["cut"]
        out = np.full((call["left"], 4), -1, dtype=np.int64)
        n = driver().draw_sched_run(call["left"], trace["batch"], draw_batch, sched, order_refresh, first_batch, C.byref(ofw), trace["eps_scalar"],
                                    state.ctypes.data, C.byref(best_thr), thr.ctypes.data, len(thr), out.ctypes.data, cap)
        assert n >= 0, trace
        calls.append(([tuple(int(v) for v in row) for row in out[:n]], int(state[5])))
    return calls


def unrle(launches):
    return [tuple(t[:4]) for t in launches for _ in range(t[4])]


@functools.lru_cache(maxsize=None)
def traces():
    with open(TRACES) as f:
        return json.load(f)


def test_the_controller_compiles_without_hip():
    """the header is plain C++17: the host compiler alone takes it, warnings on"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    res = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", CSRC, DRIVER], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_every_launch_of_every_trace():
    T = traces()
    assert len(T) >= 6 * 10 * 5
    for tr in T:
        got = replay(tr)
        assert len(got) == len(tr["calls"])
        for (launches, g_left), call in zip(got, tr["calls"]):
            assert launches == unrle(call["launches"]), (tr["sw"], tr["batch"], tr["model"], call["left"])
            assert g_left == call["g_left"]


def test_invariants_of_every_trace():
    """the lengths sum to what was asked for; no launch is longer than what is left; a timed group is never longer than what was
    left when it began; nothing is timed under a draw-batch override, AHMC_NUTS_SCHED=0, without the per-launch order, with a
    scalar step size or where batch < 2 * SCHED_MIN"""
    for tr in traces():
        draw_batch, sched, order_refresh, _ = tr["sw"]
        for (launches, _), call in zip(replay(tr), tr["calls"]):
            left = call["left"]
            if call["cut"] is None:
                assert sum(l[0] for l in launches) == left, tr
            i = 0
            while i < len(launches):
                k, probing = launches[i][:2]
                assert 1 <= k <= left, (tr, i)
                if probing:
                    assert draw_batch <= 0 and sched != 0 and order_refresh and not tr["eps_scalar"] and tr["batch"] >= 8, tr
                    # the group this launch begins: max(1, 64 // k) launches of k, all timed, all inside what is left
                    n_g = max(1, 64 // k)
                    group = launches[i:i + n_g]
                    if call["cut"] is None:
                        assert len(group) == n_g and all(l[:2] == (k, 1) for l in group), (tr, i)
                    assert k * n_g <= left, (tr, i)
                    left -= k * len(group)
                    i += len(group)
                else:
                    left -= k
                    i += 1


def _one(model, left, batch, sw=(0, 1, 1, 0), order_from_work=0, eps_scalar=0):
    for tr in traces():
        if (tr["model"], tr["batch"], tuple(tr["sw"]), tr["order_from_work"], tr["eps_scalar"]) == (model, batch, tuple(sw), order_from_work, eps_scalar) \
                and len(tr["calls"]) == 1 and tr["calls"][0]["left"] == left:
            return replay(tr)[0][0]
    raise KeyError((model, left, batch, sw))


def _short(launches):
    """8, 32*x2, 16*x4, … : lengths with a star where timed, runs folded"""
    out = []
    for k, p, _, _ in launches:
        if out and out[-1][:2] == [k, p]:
            out[-1][2] += 1
        else:
            out.append([k, p, 1])
    return ", ".join(f"{k}{'*' if p else ''}" + (f"x{n}" if n > 1 else "") for k, p, n in out)


# what the search does, spelled out (derived by hand from the rules: start at 32, halve while that gains > 2 %, else the longest
# launch unless it loses > 1.5 %, else one doubling at a time): (model, left, batch, switches) -> launches, phase and best at the end
SPELLED_OUT = [
    ("inv_len", 300, 256, (0, 1, 1, 0), "8, 32*x2, 16*x4, 8*x8, 4*x16, 4x9", 4, 4),
    ("len", 300, 256, (0, 1, 1, 0), "8, 32*x2, 16*x4, 28x2, 27x4", 3, 32),      # too little left to time the longest launch
    ("const", 300, 256, (0, 1, 1, 0), "8, 32*x2, 16*x4, 28x2, 27x4", 3, 32),
    ("len", 1000, 256, (0, 1, 1, 0), "8, 32*x2, 16*x4, 256*, 203x2, 202", 4, 256),
    ("const", 1000, 256, (0, 1, 1, 0), "8, 32*x2, 16*x4, 256*, 203x2, 202", 4, 256),
    ("peak64", 1000, 256, (0, 1, 1, 0), "8, 32*x2, 16*x4, 256*, 64*, 128*, 60x3, 59x4", 4, 64),   # the only route through phase 5
    ("peak16", 300, 256, (0, 1, 1, 0), "8, 32*x2, 16*x4, 8*x8, 15x2, 14x5", 4, 16),
    ("const", 300, 6, (0, 1, 1, 0), "6x50", 0, 0),                              # batch < 2 * SCHED_MIN: no search
    ("peak64", 40, 256, (0, 1, 1, 0), "40", 0, 0),
    ("const", 300, 256, (7, 1, 1, 0), "7x42, 6", 0, 0),                         # AHMC_NUTS_DRAW_BATCH=7
    ("const", 300, 256, (0, 0, 1, 0), "150x2", 0, 0),                           # AHMC_NUTS_SCHED=0
    ("inv_len", 300, 256, (0, 1, 1, 5), "5, 32*x2, 16*x4, 8*x8, 4*x16, 4x9, 3", 4, 4),   # AHMC_NUTS_FIRST_BATCH=5
]


@pytest.mark.parametrize("model,left,batch,sw,want,phase,best", SPELLED_OUT)
def test_spelled_out_searches(model, left, batch, sw, want, phase, best):
    launches = _one(model, left, batch, sw)
    assert _short(launches) == want
    assert launches[-1][2:] == (phase, best)


def test_no_priming_launch_and_no_search():
    """the dispatch order already on measured work at entry: no untimed 8 in front; a scalar step size: nothing is timed"""
    for model in MODELS:
        assert _one(model, 1000, 256, order_from_work=1)[0][:2] == (32, 1)
        assert _one(model, 1000, 256)[0][:2] == (8, 0)
        assert all(p == 0 for _, p, _, _ in _one(model, 1000, 256, eps_scalar=1))


def test_a_group_never_spans_two_calls():
    """a call cut off inside a timed group leaves g_left > 0; the next call drops the group at its entry and times the length afresh"""
    n = 0
    for tr in traces():
        if len(tr["calls"]) == 2 and tr["calls"][0]["cut"] is not None:
            (first, g_left), (second, _) = replay(tr)
            assert g_left > 0 and first[-1][1] == 1
            k = first[-1][0]
            n_g = max(1, 64 // k)
            assert [l[:2] for l in second[:n_g]] == [(k, 1)] * n_g, tr   # the whole group again, not the rest of it
            n += 1
    assert n == 2 * len(MODELS)
