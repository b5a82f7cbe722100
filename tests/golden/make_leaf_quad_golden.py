#!/usr/bin/env python
"""Record tests/golden/leaf_quad_parent.npz: the chains of tests/test_leaf_quads.py as the PAIR loop of k_nuts builds them.

The committed fixture was recorded from the library of commit 6fd8239, the parent of the commit that made k_nuts build its subtrees four
leaves per step where a chain owns a wave (the quad step).  Regenerating it means building THAT commit in a checkout of its own:

    git worktree add ../parent 6fd8239 && (cd ../parent && python -c "import ahmc_amd as A; A.build_hip_library()")
    AHMC_HIP_LIB=../parent/advancedhmc.jl_amd/csrc/libahmc_hip.so python tests/golden/make_leaf_quad_golden.py [OUT.npz]

The fixture is recorded from whichever HIP library AHMC_HIP_LIB names (needs the MI355X).  The shipped library has to reproduce it bit for
bit.  Fields, checksums and the set-up of a case are those of make_leaf_pair_golden.py (`setup`, `run_case`, `theta_sum`), with N = 64
chains of an IsoGaussian with a per-chain unit diagonal metric.

Where a transition's tree ended is read from n_steps: the last doubling is jw = floor(log2 n_steps), and p = n_steps − 2^jw + 1 leaves of
its subtree were built.  From jw = 2 on the subtree is built in quads a, b, c, d: p ≡ 1, 2, 3, 0 (mod 4) is an end on a, b, c, d.

The cases (each exists for an exit of the quad step; tests/test_leaf_quads.py asserts on the fixture that it is taken):
  div_*     Δ_max = 0.5 and a fixed ϵ: divergent ends on each of the four leaves of a quad, in every G = 64 geometry and in f32;
  md3_div_*  Δ_max = 0.5, ϵ = 0.3 and max_depth 3 from a start at θ0 ~ U(0,1): trees of at most ONE quad, most of them divergent;
  md3_adapt_*  max_depth 3 with 30 adapting transitions (the warm-up kernel) and 20 draws: every full tree is the leaf, the pair and one quad;
  div_uturn_*  (started in the typical set, as every div_ case is) Δ_max = 1000 and ϵ = 1.6 / 1.7: trees that end by the U-turn of the FIRST pair of a quad (p ≡ 2 mod 4 inside an unfinished
            subtree — leaves c and d were speculative), and many that end at p ≡ 0 (the second pair, the level-1 merge or a higher one);
            D = 129 and 257 are the smallest (64,4) and (64,8) geometries.
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIXTURE = os.path.join(ROOT, "tests", "golden", "leaf_quad_parent.npz")
N = 64


def _pair_generator():
    """a private copy of make_leaf_pair_golden (its N and CASES are module globals: the copy gets this file's)"""
    spec = importlib.util.spec_from_file_location("_leaf_pair_golden_for_quads", os.path.join(ROOT, "tests", "golden", "make_leaf_pair_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# name: D, dtype, max_depth, Δ_max, ϵ0, n_adapts, n_total, start offset
CASES = {
    "div_f64_d65": (65, "f64", 10, 0.5, 0.35, 0, 20, 0.0),
    "div_f64_d128": (128, "f64", 10, 0.5, 0.3, 0, 20, 0.0),
    "div_f32_d128": (128, "f32", 10, 0.5, 0.3, 0, 20, 0.0),
    "div_f64_d256": (256, "f64", 10, 0.5, 0.25, 0, 20, 0.0),
    "div_f64_d512": (512, "f64", 10, 0.5, 0.22, 0, 20, 0.0),
    "md3_div_f64_d128": (128, "f64", 3, 0.5, 0.3, 0, 20, 0.0),
    "md3_adapt_f64_d128": (128, "f64", 3, 1000.0, 0.1, 30, 50, 0.0),
    "div_uturn_f64_d65": (65, "f64", 10, 1000.0, 1.6, 0, 20, 0.0),
    "div_uturn_f32_d65": (65, "f32", 10, 1000.0, 1.6, 0, 20, 0.0),
    "div_uturn_f64_d128": (128, "f64", 10, 1000.0, 1.6, 0, 20, 0.0),
    "div_uturn_f64_d129": (129, "f64", 10, 1000.0, 1.7, 0, 20, 0.0),
    "div_uturn_f64_d257": (257, "f64", 10, 1000.0, 1.7, 0, 20, 0.0),
}
GEOMETRY = {65: (64, 2), 128: (64, 2), 129: (64, 4), 256: (64, 4), 257: (64, 8), 512: (64, 8)}   # (group_lanes, elems_per_lane) the engine must pick

PAIR_GEN = _pair_generator()
PAIR_GEN.N = N
PAIR_GEN.CASES = CASES
PER_TRANSITION = PAIR_GEN.PER_TRANSITION
theta_sum = PAIR_GEN.theta_sum
setup = PAIR_GEN.setup
run_case = PAIR_GEN.run_case


def quad_position(n_steps):
    """(jw, p) of the last doubling of each tree: its index and the number of leaves built in it"""
    ns = np.asarray(n_steps).astype(np.int64)
    jw = np.floor(np.log2(np.maximum(ns, 1))).astype(np.int64)
    return jw, ns - (1 << jw) + 1


def main():
    sys.path.insert(0, ROOT)
    import ahmc_amd as A

    lib = A.load_hip_library()
    data = {}
    for name in CASES:
        for f, v in run_case(A, lib, name).items():
            data[f"{name}/{f}"] = v
        ns, ne = data[f"{name}/n_steps"], data[f"{name}/numerical_error"]
        jw, p = quad_position(ns)
        q = jw >= 2
        print(f"{name}: mean n_steps {ns.mean():.1f}, max depth {int(data[name + '/tree_depth'].max())}, divergent ends on a / b / c / d "
              f"{[int((q & (ne != 0) & (p % 4 == r)).sum()) for r in (1, 2, 3, 0)]}, other ends inside a subtree at p = 2 / 0 mod 4 "
              f"{[int((q & (ne == 0) & (p < (1 << jw)) & (p % 4 == r)).sum()) for r in (2, 0)]}")
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    np.savez_compressed(out, **data)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
