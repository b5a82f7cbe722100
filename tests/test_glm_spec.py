"""Binding a GLM decides on the host what it decided before the decisions were gathered in csrc/ahmc_glm_spec.hpp — on a CPU.

tests/host_ref/glm_spec_driver.cpp runs the header's two host-only steps (glm_spec_check, then glm_spec_build on a staging copy of
the caller's arrays) the way glm_bind runs them between its device calls.  The expectation, tests/golden/glm_bind_refusals.json, holds
the status and the ahmc_last_error text that the library answered through the C ABI on the GPU BEFORE the header existed
(scripts/glm_identity.py refusals --write-golden, on a build of the commit before it): never what the header says.  Its cases are
every refusal that the test_refusals functions of the six tests/test_glm_*.py files provoke, on models of 20 observations, pairs of
violated conditions that pin which of the two is reported, and one accepted call per entry point; each in Float64 and Float32.
Status and text must be equal.
"""
import ctypes as C
import functools
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "host_ref", "glm_spec_driver.cpp")
CSRC = os.path.join(ROOT, "advancedhmc.jl_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(CSRC, "ahmc_glm_spec.hpp")
TABLE = os.path.join(ROOT, "tests", "golden", "glm_bind_refusals.json")
DTYPES = {"f64": np.float64, "f32": np.float32}

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import glm_identity as GI  # noqa: E402  (materialise: how a case of the table becomes arguments, shared with the recorder)


@functools.lru_cache(maxsize=None)
def driver():
    """tests/host_ref/glm_spec_driver.cpp as its own shared object in the build cache, by the host compiler (as tests/test_draw_sched.py
    builds its driver; keyed on the header as well)"""
    from ahmc_amd import build as B

    flags = ["-O1", "-std=c++17", "-fPIC", "-shared"]
    with open(DRIVER, "rb") as f, open(HEADER, "rb") as g:
        h = hashlib.sha256(f.read() + g.read() + " ".join(flags).encode()).hexdigest()[:20]
    out_dir = os.path.join(B.OBJ, "host_ref")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, f"glm_spec_driver_{h}.so")
    if not os.path.exists(so):
        cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
        tmp = so + f".tmp{os.getpid()}"
        res = subprocess.run([cxx, *flags, "-I", CSRC, "-I", INCLUDE, DRIVER, "-o", tmp], capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"glm_spec_driver build failed:\n{res.stdout}\n{res.stderr}")
        os.replace(tmp, so)
    dll = C.CDLL(so)
    i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    for name in ("glm_spec_run_f64", "glm_spec_run_f32"):
        fn = getattr(dll, name)
        fn.restype = C.c_int
        fn.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int, i32, i32,
                       i32, f64, C.c_int, i32, i32, C.c_int, C.c_double, C.c_double, C.c_int, f64, C.c_char_p, C.c_int64]
    return dll


@functools.lru_cache(maxsize=None)
def table():
    with open(TABLE) as f:
        return json.load(f)


def answer(case, dt):
    """[status, message] of the header for one case in one element type"""
    m = GI.materialise(table(), case, DTYPES[dt])
    p = GI.pointers(m)
    msg = C.create_string_buffer(1024)
    rc = getattr(driver(), "glm_spec_run_" + dt)(m["entry"], m["D"], m["N"], m["family"], m["n_obs"], m["n_coef"], *p["data"], m["scale"], *p["groups"], *p["factors"],
                                                m["has_aux"], m["aux_loc"], m["aux_scale"], m["n_categories"], p["cut_prior"], msg, len(msg))
    return [rc, msg.value.decode("utf-8") if rc else ""]


@pytest.mark.parametrize("dt", list(DTYPES))
def test_every_recorded_answer(dt):
    """status and text of every case of the table, in the table's order"""
    got = {c["name"]: answer(c, dt) for c in table()["cases"]}
    want = {c["name"]: GI.expected(c, dt) for c in table()["cases"]}
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


def test_the_table_holds_what_it_must():
    """one accepted call per entry point, the pairs of violated conditions, and only models of at most (70, 3)"""
    t = table()
    by_name = {c["name"]: c for c in t["cases"]}
    assert len(by_name) == len(t["cases"])
    for b in GI.ENTRIES:
        assert by_name[f"{b}: accepted"]["expect"] == [0, ""]
    for name in ("categorical: n_categories = 1 with n_factors = -1", "factor: n_factors above the limit with n_obs = 0",
                 "factor: n_coef = 0 with n_obs above AHMC_GLM_MAX_OBS", "factor: a level index out of range with a D that does not match",
                 "hier: n_groups = -1 with a D that does not match", "aux: n_groups above both group limits", "hier: family 5 with a D that does not match",
                 "hier: family 6 with a D that does not match", "plain: a dispersion family with n_obs = 0", "plain: an unknown family with X NULL",
                 "plain: scale = 0 with a NaN in X", "plain: a NaN in X with y outside the domain",
                 "plain: a non-finite offset at row i with a bad y at rows i and i - 1", "hier: a negative prior_prec with a non-zero one on a group member",
                 "hier: the same group table overlapping and out of bounds"):
        assert GI.expected(by_name[name], "f64")[0] != 0, name
    assert all(b["n_obs"] <= 70 and b["n_coef"] <= 3 for b in t["bases"].values())
    assert os.path.getsize(TABLE) < 100 * 1024
