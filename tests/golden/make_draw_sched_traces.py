"""Writes tests/golden/draw_sched_traces.json: what the launch-length search of the sampling phase decides, launch by launch, on a grid
of run lengths, switches and throughput models — the expectation of tests/test_draw_sched.py.

`plan_next` and `close_group` below are a transcription, statement by statement, of the search as it stood INSIDE the sampling loop
(`sample_from_impl` in csrc/ahmc_api.hip at commit 2ebaf18, before the loop was split: the draw branch up to the AHMC_NUTS_FIRST_BATCH
clamp, and the phase transition at the end of a timed group), with the clock replaced by a pure function of the launch length.  They
are NOT derived from csrc/ahmc_draw_sched.hpp — that header is what the traces test.  Do not "fix" this file to follow the header:
a difference between the two is a finding about the header.

    python tests/golden/make_draw_sched_traces.py        # rewrites the JSON next to this file
"""
import json
import math
import os

SCHED_MIN, SCHED_START, SCHED_GROUP = 4, 32, 64

# throughput of a timed group as a function of its launch length alone
MODELS = {
    "inv_len": lambda L: 1.0 / L,
    "len": lambda L: float(L),
    "const": lambda L: 1.0,
    "peak64": lambda L: 1.0 - 0.1 * abs(math.log2(L) - 6.0),
    "peak16": lambda L: 1.0 - 0.1 * abs(math.log2(L) - 4.0),
}

GRID = [(300, 256), (1000, 256), (2000, 256), (1000, 32), (300, 6), (40, 256)]

# SCHEDULES of tests/test_pipeline_parity.py (the two AHMC_NORMALS_PREFETCH* variants do not reach the controller: the second of
# them is its AHMC_NUTS_DRAW_BATCH=5)
SCHEDULES = [
    {},
    {"AHMC_NUTS_SCHED": "0"},
    {"AHMC_NUTS_SCHED": "0", "AHMC_NUTS_ORDER_REFRESH": "0"},
    {"AHMC_NUTS_NO_ORDER": "1"},
    {"AHMC_NUTS_DRAW_BATCH": "7"},
    {"AHMC_NUTS_DRAW_BATCH": "2"},
    {"AHMC_NUTS_FIRST_BATCH": "5"},
    {"AHMC_NUTS_ORDER_REFRESH": "0", "AHMC_NUTS_DRAW_BATCH": "9", "AHMC_NUTS_FIRST_BATCH": "4"},
    {"AHMC_NUTS_BATCH": "6"},
    {"AHMC_NUTS_DRAW_BATCH": "5"},
]


SWITCH_FIELDS = ("draw_batch", "sched", "order_refresh", "first_batch")   # the order of a trace's "sw"


def switches(env):
    """the environment as the loop parsed it: (draw_batch_env, sched_env, order-refresh switch before the context's own terms, first_batch)"""
    orf = env.get("AHMC_NUTS_ORDER_REFRESH")
    return {
        "draw_batch": int(env.get("AHMC_NUTS_DRAW_BATCH", 0)),
        "sched": int(env.get("AHMC_NUTS_SCHED", 1)),
        "order_refresh": int((int(orf) != 0 if orf is not None else True) and "AHMC_NUTS_NO_ORDER" not in env),
        "first_batch": int(env.get("AHMC_NUTS_FIRST_BATCH", 0)),
    }


def fresh_state():
    return {"phase": 0, "len": 0, "best_len": 0, "best_thr": 0.0, "primed": False, "g_len": 0, "g_left": 0}


def plan_next(sc, left, batch, draw_batch_env, sched_env, order_refresh, first_batch, order_from_work, eps_scalar):
    """-> (k, probing); `order_refresh` is the loop's own: the switch, no dense engine, per-chain step sizes"""
    probing = False
    if draw_batch_env <= 0 and sched_env != 0 and order_refresh and sc["phase"] != 4 and batch >= 2 * SCHED_MIN:
        if sc["g_left"] > 0 and sc["g_len"] > left:
            sc["g_left"] = 0
        if sc["g_left"] > 0:
            k = sc["g_len"]
            probing = True
        elif not sc["primed"] and not order_from_work and left >= 4 * SCHED_START:
            k = 2 * SCHED_MIN
            sc["primed"] = True
        else:
            if sc["phase"] == 0:
                L = min(SCHED_START, batch)
            elif sc["phase"] == 3:
                L = batch
            elif sc["phase"] == 5:
                L = min(sc["len"] * 2, batch)
            else:
                L = max(sc["len"] // 2, SCHED_MIN)
            n_g = max(1, SCHED_GROUP // L)
            if left >= L * n_g + L:
                sc["primed"] = True
                sc["g_len"] = L
                sc["g_left"] = n_g
                k = L
                probing = True
            else:
                dbatch = sc["best_len"] if sc["best_len"] > 0 else batch
                nb_left = (left + dbatch - 1) // dbatch
                k = (left + nb_left - 1) // nb_left
    else:
        if draw_batch_env > 0:
            dbatch = draw_batch_env
        else:
            dbatch = sc["best_len"] if (sc["phase"] == 4 and sched_env != 0 and order_refresh) else batch
        nb_left = (left + dbatch - 1) // dbatch
        k = (left + nb_left - 1) // nb_left
    if first_batch >= 4 and not order_from_work and not eps_scalar and left > 2 * first_batch and not probing:
        k = min(k, first_batch)
    return k, probing


def close_group(sc, k, thr, batch):
    if sc["phase"] == 0:
        sc["best_len"] = sc["len"] = k
        sc["best_thr"] = thr
        sc["phase"] = 1 if k // 2 >= SCHED_MIN else 3
    elif sc["phase"] == 1 or sc["phase"] == 2:
        if thr > sc["best_thr"] * 1.02:
            sc["best_len"] = sc["len"] = k
            sc["best_thr"] = thr
            sc["phase"] = 2 if k // 2 >= SCHED_MIN else 4
        elif sc["phase"] == 1:
            sc["len"] = sc["best_len"]
            sc["phase"] = 3 if sc["best_len"] * 2 <= batch else 4
        else:
            sc["phase"] = 4
    elif sc["phase"] == 3:
        if thr >= sc["best_thr"] * 0.985:
            sc["best_len"] = sc["len"] = k
            sc["best_thr"] = max(sc["best_thr"], thr)
            sc["phase"] = 4
        else:
            sc["phase"] = 5 if sc["best_len"] * 4 <= batch else 4
    elif sc["phase"] == 5:
        if thr >= sc["best_thr"] * 0.985:
            sc["best_len"] = sc["len"] = k
            sc["best_thr"] = max(sc["best_thr"], thr)
            sc["phase"] = 5 if k * 4 <= batch else 4
        else:
            sc["phase"] = 4


def run_call(sc, left, batch, sw, model, order_from_work, eps_scalar, max_launches=None):
    """one call's sampling phase (cut off after max_launches, as a call that failed half way would be):
    -> (launches [(k, probing, phase after, best_len after)], order_from_work after)"""
    sc["g_left"] = 0                       # the call's entry
    order_refresh = bool(sw["order_refresh"]) and not eps_scalar
    out = []
    while left > 0 and (max_launches is None or len(out) < max_launches):
        k, probing = plan_next(sc, left, batch, sw["draw_batch"], sw["sched"], order_refresh, sw["first_batch"], order_from_work, eps_scalar)
        if order_refresh and k >= 2:
            order_from_work = True         # the launch's work re-sorted the dispatch order
        if probing:
            sc["g_left"] -= 1
            if sc["g_left"] == 0:
                close_group(sc, k, MODELS[model](k), batch)
        out.append((k, int(probing), sc["phase"], sc["best_len"]))
        left -= k
    return out, order_from_work


def rle(launches):
    """[(k, probing, phase, best_len)] -> [[k, probing, phase, best_len, repeats]]"""
    out = []
    for t in launches:
        if out and tuple(out[-1][:4]) == t:
            out[-1][4] += 1
        else:
            out.append([*t, 1])
    return out


def cases():
    """calls: [(transitions asked for, launches after which the call is cut off or None)] on ONE controller state, in order"""
    for left, batch in GRID:
        for env in SCHEDULES:
            b = int(env.get("AHMC_NUTS_BATCH", batch))
            for model in MODELS:
                yield {"sw": switches(env), "calls": [(left, None)], "batch": b, "model": model, "order_from_work": 0, "eps_scalar": 0}
    for left, batch in GRID:
        for model in MODELS:
            # the dispatch order already on measured work at entry: no priming launch; a scalar step size: no search
            yield {"sw": switches({}), "calls": [(left, None)], "batch": batch, "model": model, "order_from_work": 1, "eps_scalar": 0}
            yield {"sw": switches({}), "calls": [(left, None)], "batch": batch, "model": model, "order_from_work": 0, "eps_scalar": 1}
    for model in MODELS:
        # Two calls on one context.  A group is only begun where the call has room to finish it, so a call ends inside one only by
        # failing: cut off after 8, 32* (one launch of a group of two) and after 8, 32*, 32*, 16* (one of four) — the next call drops
        # the group at its entry and begins it afresh.  And a first call that runs to its end, the search going on in the second.
        yield {"sw": switches({}), "calls": [(1000, 2), (1000, None)], "batch": 256, "model": model, "order_from_work": 0, "eps_scalar": 0}
        yield {"sw": switches({}), "calls": [(1000, 4), (300, None)], "batch": 256, "model": model, "order_from_work": 0, "eps_scalar": 0}
        yield {"sw": switches({}), "calls": [(136, None), (300, None)], "batch": 256, "model": model, "order_from_work": 0, "eps_scalar": 0}


def main():
    traces = []
    for c in cases():
        sc, ofw, calls = fresh_state(), bool(c["order_from_work"]), []
        for left, cut in c["calls"]:
            launches, ofw = run_call(sc, left, c["batch"], c["sw"], c["model"], ofw, bool(c["eps_scalar"]), cut)
            calls.append({"left": left, "cut": cut, "launches": rle(launches), "g_left": sc["g_left"]})
        c = dict(c)
        c["sw"] = [c["sw"][n] for n in SWITCH_FIELDS]
        c["calls"] = calls
        traces.append(c)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "draw_sched_traces.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(t, separators=(",", ":")) for t in traces) + "\n]\n")
    print(f"{len(traces)} traces -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
