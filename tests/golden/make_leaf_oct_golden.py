#!/usr/bin/env python
"""Record tests/golden/leaf_oct_parent.npz: the chains of tests/test_leaf_octs.py as the QUAD loop of k_nuts builds them.

The committed fixture was recorded from the library of commit 30a9c75, the parent of the commit that made k_nuts build its subtrees eight
leaves per step from the fourth doubling on where a chain owns a wave (the octo step).  Regenerating it means building THAT commit in a
checkout of its own:

    git worktree add ../parent 30a9c75 && (cd ../parent && python -c "import ahmc_amd as A; A.build_hip_library()")
    AHMC_HIP_LIB=../parent/advancedhmc.jl_amd/csrc/libahmc_hip.so python tests/golden/make_leaf_oct_golden.py [OUT.npz]

The fixture is recorded from whichever HIP library AHMC_HIP_LIB names (needs the MI355X).  The shipped library has to reproduce it bit for
bit.  Fields, checksums and the set-up of a case are those of make_leaf_pair_golden.py (`setup`, `run_case`, `theta_sum`), with N = 64
chains of an IsoGaussian with a per-chain unit diagonal metric, as in make_leaf_quad_golden.py.

Where a transition's tree ended is read from n_steps: the last doubling is jw = floor(log2 n_steps), and p = n_steps − 2^jw + 1 leaves of
its subtree were built.  From jw = 3 on the subtree is built in octos a .. h: p ≡ 1, 2, …, 7, 0 (mod 8) is an end on a, b, …, g, h.

The cases (each exists for an exit of the octo step; tests/test_leaf_octs.py asserts on the fixture that it is taken):
  div_*       Δ_max = 0.1 and ϵ = 0.16 (trees of depth <= 5): divergent ends on each of the eight leaves of an octo, in every G = 64
              geometry — D = 65 and 128 (64,2), 129 (64,4), 257 (64,8) — and in f32;
  div_deep_*  Δ_max = 0.05 and ϵ = 0.1: the same in trees up to depth 10;
  div_uturn_* Δ_max = 1000 and ϵ = 1.7 / 1.6: trees that end WITHOUT a divergence inside an unfinished subtree at p ≡ 2, 4, 6, 0 (mod 8) — the
              U-turn of a level-0, level-1 or level-2 merge inside the octo, or of a higher one behind it — with six, four, two and no
              speculative leaves behind the end;
  div_md4_*   max_depth 4 with Δ_max = 0.1: every tree that reaches the fourth doubling is the leaf, the pair, the quad and ONE octo;
  md4_adapt_* max_depth 4 with 30 adapting transitions (the warm-up kernel, window schedule 5 / 5 / 10) and 20 draws;
  pipe_*_far  a start 30σ out with adaptation, as make_leaf_pair_golden.py's: −ΔH > 600 on the way in hands chains to the log-domain redo
              kernels (MODE 4 in the warm-up; one iteration per call their trees are short, in one fused call the redo kernel carries
              the chain through the rest of its launch);
  fardraws_*  the same start without adaptation and with ϵ = 0.3, as make_leaf_pair_golden.py's: the redo kernel of the draws (MODE 1), with
              handed-over transitions whose trees reach the fourth doubling (n_steps >= 8).
(every div_ case starts in the typical set, the others at θ0 ~ U(0,1) + offset: make_leaf_pair_golden.py's `setup`)

Which kernels take the octo step is decided per instantiation (csrc/ahmc_nuts.hpp: nuts_oct_step): the (64,2) geometry does — D = 65 and
128, f64 and f32, the linear-domain kernels and the warm-up's log-domain kernel (MODE 4; f32: MODE 1 too) — and those cases run it.  The
Float64 redo kernel of the draws (MODE 1: fardraws_*) and the (64,4) and (64,8) geometries (D = 129, 257) keep the quad step; their cases hold
the same ends of the same trees to the parent's bits through whichever arm their kernels have, so that an instantiation that is switched on
later is held by a fixture that already has the exits.
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIXTURE = os.path.join(ROOT, "tests", "golden", "leaf_oct_parent.npz")
N = 64


def _pair_generator():
    """a private copy of make_leaf_pair_golden (its N and CASES are module globals: the copy gets this file's)"""
    spec = importlib.util.spec_from_file_location("_leaf_pair_golden_for_octs", os.path.join(ROOT, "tests", "golden", "make_leaf_pair_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# name: D, dtype, max_depth, Δ_max, ϵ0, n_adapts, n_total, start offset
CASES = {
    "div_f64_d65": (65, "f64", 10, 0.1, 0.16, 0, 20, 0.0),
    "div_f64_d128": (128, "f64", 10, 0.1, 0.16, 0, 20, 0.0),
    "div_f32_d128": (128, "f32", 10, 0.1, 0.16, 0, 20, 0.0),
    "div_f64_d129": (129, "f64", 10, 0.1, 0.16, 0, 20, 0.0),
    "div_f64_d257": (257, "f64", 10, 0.1, 0.16, 0, 20, 0.0),
    "div_deep_f64_d128": (128, "f64", 10, 0.05, 0.1, 0, 20, 0.0),
    "div_deep_f64_d129": (129, "f64", 10, 0.05, 0.1, 0, 20, 0.0),
    "div_deep_f64_d257": (257, "f64", 10, 0.05, 0.1, 0, 20, 0.0),
    "div_uturn_f32_d65": (65, "f32", 10, 1000.0, 1.6, 0, 20, 0.0),
    "div_uturn_f64_d129": (129, "f64", 10, 1000.0, 1.7, 0, 20, 0.0),
    "div_uturn_f64_d257": (257, "f64", 10, 1000.0, 1.7, 0, 20, 0.0),
    "div_md4_f64_d128": (128, "f64", 4, 0.1, 0.16, 0, 20, 0.0),
    "md4_adapt_f64_d128": (128, "f64", 4, 1000.0, 0.1, 30, 50, 0.0),
    "pipe_f64_d128_far": (128, "f64", 10, 1000.0, 0.1, 30, 50, 30.0),
    "fardraws_f64_d128": (128, "f64", 10, 1000.0, 0.3, 0, 20, 30.0),
}
GEOMETRY = {65: (64, 2), 128: (64, 2), 129: (64, 4), 257: (64, 8)}   # (group_lanes, elems_per_lane) the engine must pick

PAIR_GEN = _pair_generator()
PAIR_GEN.N = N
PAIR_GEN.CASES = CASES
PER_TRANSITION = PAIR_GEN.PER_TRANSITION
LINW_LIMIT = PAIR_GEN.LINW_LIMIT
theta_sum = PAIR_GEN.theta_sum
setup = PAIR_GEN.setup
run_case = PAIR_GEN.run_case
handed_over = PAIR_GEN.handed_over


def oct_position(n_steps):
    """(jw, p) of the last doubling of each tree: its index and the number of leaves built in it"""
    ns = np.asarray(n_steps).astype(np.int64)
    jw = np.floor(np.log2(np.maximum(ns, 1))).astype(np.int64)
    return jw, ns - (1 << jw) + 1


def oct_ends(n_steps, numerical_error):
    """counts of where trees ended, doublings jw >= 3 only: divergent ends on a .. h, and non-divergent ends inside an unfinished subtree
    at p ≡ 2, 4, 6, 0 (mod 8)"""
    ns, ne = np.asarray(n_steps), np.asarray(numerical_error)
    jw, p = oct_position(ns)
    q = jw >= 3
    div = [int((q & (ne != 0) & (p % 8 == r)).sum()) for r in (1, 2, 3, 4, 5, 6, 7, 0)]
    inside = q & (ne == 0) & (p < (1 << jw))
    return div, [int((inside & (p % 8 == r)).sum()) for r in (2, 4, 6, 0)]


def main():
    sys.path.insert(0, ROOT)
    import ahmc_amd as A

    lib = A.load_hip_library()
    data = {}
    for name in CASES:
        for f, v in run_case(A, lib, name).items():
            data[f"{name}/{f}"] = v
        ns, ne = data[f"{name}/n_steps"], data[f"{name}/numerical_error"]
        div, inside = oct_ends(ns, ne)
        print(f"{name}: mean n_steps {ns.mean():.1f}, max depth {int(data[name + '/tree_depth'].max())}, divergent ends on a .. h {div}, "
              f"other ends inside a subtree at p = 2 / 4 / 6 / 0 mod 8 {inside}, handed over {int(handed_over(data, name).sum())}", flush=True)
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    np.savez_compressed(out, **data)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
