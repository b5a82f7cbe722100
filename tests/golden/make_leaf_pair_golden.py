#!/usr/bin/env python
"""Record tests/golden/leaf_pair_single_loop.npz: the chains of tests/test_leaf_pairs.py as the SINGLE-LEAF loop of k_nuts builds them.

The committed fixture was recorded at or before commit 9712c5e, the last one whose engine could still be built with the single-leaf loop
everywhere (a build-time switch, since retired: DESIGN.md §9).  Regenerating it means building THAT commit:

    git checkout 9712c5e && python scripts/build_variant.py pair0 -DAHMC_LEAF_PAIR=0     # in a checkout of its own
    AHMC_HIP_LIB=<that checkout>/advancedhmc.jl_amd/csrc/variants/libahmc_hip_pair0.so python tests/golden/make_leaf_pair_golden.py [OUT.npz]

The fixture is recorded from whichever HIP library AHMC_HIP_LIB names (needs the MI355X), so a later toolchain can regenerate it.  The
shipped library (two leaves per step where a chain owns a wave) has to reproduce it bit for bit.

What is recorded, per case and per transition, for every chain: n_steps, acceptance_rate, numerical_error, tree_depth, step_size, the
largest energy error of the tree (ΔH_max, signed: below −600 the chain went through the log-domain redo kernel) and θ —
θ as a 64-bit position-weighted checksum of its bit patterns (`theta_sum`; the vectors themselves would be 3 MB for the D = 512 case
alone) with its first two components in full; after the last transition the adapted M⁻¹, as the same checksum and its first two rows.

The cases (16 chains of an IsoGaussian with a per-chain diagonal metric; the smallest shapes at which each G = 64 instantiation of k_nuts
can go wrong):
  pipe_*  30 StanHMCAdaptor transitions through the fused warm-up kernel (MODE 3) and 20 draws (MODE 0), one iteration per call:
          D = 65 (the padded (64,2) geometry), 128, 256 (64,4), 512 (64,8) in f64; D = 128 in f32; max_depth 1 (a single leaf: no pair
          step at all) and 2 (exactly one pair) at D = 128; `far`: a start 30σ out, where −ΔH > 600 on the way in makes the
          linear-domain kernels hand the chain to the log-domain redo kernels (MODE 4 in the warm-up);
  fardraws  the same start without adaptation and with ϵ = 0.3: the redo kernel of the draws (MODE 1).  The kick-drift-kick leapfrog on a unit
          Gaussian with a unit metric conserves H − ϵ²|θ|²/8, so −ΔH on the way in reaches ϵ²|θ0|²/8 ≈ 0.09 · 128 · 30.5² / 8 ≈ 1 340 > 600
          (with ϵ = 0.1 it would stay below 149 and never leave the linear-domain kernel);
  div_*   Δ_max = 0.5 with a fixed ϵ chosen (with the CPU oracle) so that subtrees end by divergence on first AND on second leaves of a
          pair: a transition's n_steps is even when its tree ended on the first leaf of a pair, odd (> 1) on the second.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIXTURE = os.path.join(ROOT, "tests", "golden", "leaf_pair_single_loop.npz")
N = 16
PER_TRANSITION = ("n_steps", "acceptance_rate", "numerical_error", "tree_depth", "step_size", "max_hamiltonian_energy_error")
LINW_LIMIT = 600.0   # csrc/ahmc_nuts.hpp: a leaf with −ΔH above it makes the linear-domain kernel hand its chain to the log-domain one

# name: D, dtype, max_depth, Δ_max, ϵ0, n_adapts, n_total, start offset
CASES = {
    "pipe_f64_d65": (65, "f64", 10, 1000.0, 0.1, 30, 50, 0.0),
    "pipe_f64_d128": (128, "f64", 10, 1000.0, 0.1, 30, 50, 0.0),
    "pipe_f64_d256": (256, "f64", 10, 1000.0, 0.1, 30, 50, 0.0),
    "pipe_f64_d512": (512, "f64", 10, 1000.0, 0.1, 30, 50, 0.0),
    "pipe_f32_d128": (128, "f32", 10, 1000.0, 0.1, 30, 50, 0.0),
    "pipe_f64_d128_md1": (128, "f64", 1, 1000.0, 0.1, 30, 50, 0.0),
    "pipe_f64_d128_md2": (128, "f64", 2, 1000.0, 0.1, 30, 50, 0.0),
    "pipe_f64_d128_far": (128, "f64", 10, 1000.0, 0.1, 30, 50, 30.0),
    "fardraws_f64_d128": (128, "f64", 10, 1000.0, 0.3, 0, 20, 30.0),
    "div_f64_d65": (65, "f64", 10, 0.5, 0.35, 0, 20, 0.0),
    "div_f64_d128": (128, "f64", 10, 0.5, 0.3, 0, 20, 0.0),
    "div_f64_d256": (256, "f64", 10, 0.5, 0.25, 0, 20, 0.0),
    "div_f64_d512": (512, "f64", 10, 0.5, 0.22, 0, 20, 0.0),
    "div_f32_d128": (128, "f32", 10, 0.5, 0.3, 0, 20, 0.0),
}
GEOMETRY = {65: (64, 2), 128: (64, 2), 256: (64, 4), 512: (64, 8)}   # (group_lanes, elems_per_lane) the engine must pick


def handed_over(rec_or_fixture, name):
    """per transition and chain: did a leaf of the tree have −ΔH > LINW_LIMIT, i.e. was the chain handed to the log-domain kernel
    (MODE 1 in the draws, MODE 4 in the warm-up)?  ΔH_max is the energy error of largest magnitude, signed."""
    key = "max_hamiltonian_energy_error"
    dh = rec_or_fixture[key] if key in rec_or_fixture else rec_or_fixture[f"{name}/{key}"]
    return dh < -LINW_LIMIT


def theta_sum(th):
    """per chain: Σ_d bits(θ[d]) · (2d + 1) mod 2^64 — a changed bit anywhere changes the sum (odd weights are invertible mod 2^64)"""
    th = np.ascontiguousarray(th)
    bits = th.view(np.uint64 if th.dtype.itemsize == 8 else np.uint32).astype(np.uint64)
    w = (2 * np.arange(th.shape[0], dtype=np.uint64) + 1)[:, None]
    with np.errstate(over="ignore"):
        return (bits * w).sum(axis=0, dtype=np.uint64)


def setup(A, lib, name):
    D, dt, max_depth, delta_max, eps0, n_adapts, n_total, off = CASES[name]
    dtype = np.float64 if dt == "f64" else np.float32
    metric = A.DiagEuclideanMetric(np.ones((D, N), order="F"))
    h = A.Hamiltonian(metric, A.IsoGaussian(D))
    lf = A.Leapfrog(np.full(N, eps0))
    e = A.Engine(h, N, dtype=dtype, rng=A.PhiloxRNG(0x1EAF + D), lib=lib)
    e.set_integrator(lf)
    rs = np.random.default_rng(D)
    # (the divergence cases start in the typical set, where a fixed ϵ gives sensible trees; the others at θ0 ~ U(0,1) as bench.py does)
    e.set_position(np.asfortranarray(rs.standard_normal((D, N)) if name.startswith("div_") else rs.random((D, N)) + off))
    k = A.HMCKernel(A.Trajectory(A.MultinomialTS, lf, A.GeneralisedNoUTurn(max_depth=max_depth, delta_max=delta_max)))
    # (the reference's window schedule does not shrink with n_adapts: 30 warm-up iterations take init_buffer = 5, term_buffer = 5,
    # window_size = 10 — a metric update and a dual-averaging restart inside the run)
    ad = A.StanHMCAdaptor(A.MassMatrixAdaptor(metric), A.StepSizeAdaptor(0.8, lf), init_buffer=5, term_buffer=5, window_size=10) if n_adapts else None
    if ad is not None:
        e.adaptor_init(ad)
    return e, k, n_adapts, n_total


def run_case(A, lib, name, each=None):
    """one iteration per call; returns the record of the case ({field: array}).  `each(i, engine)` runs after every transition."""
    e, k, n_adapts, n_total = setup(A, lib, name)
    rec = {f: [] for f in PER_TRANSITION + ("theta_sum", "theta_head")}
    for i in range(1, n_total + 1):
        e.run(k, i, n_adapts, i_first=i)
        e.sync()
        st = e.stats(list(PER_TRANSITION))
        th = e.theta()
        for f in PER_TRANSITION:
            rec[f].append(st[f].copy())
        rec["theta_sum"].append(theta_sum(th))
        rec["theta_head"].append(th[:2].copy())
        if each is not None:
            each(i, e)
    out = {f: np.stack(v) for f, v in rec.items()}
    m = e.get_metric()
    out["metric_sum"], out["metric_head"] = theta_sum(m), m[:2].copy()
    e.close()
    return out


def main():
    sys.path.insert(0, ROOT)
    import ahmc_amd as A

    lib = A.load_hip_library()
    data = {}
    for name in CASES:
        for f, v in run_case(A, lib, name).items():
            data[f"{name}/{f}"] = v
        ns, ne = data[f"{name}/n_steps"], data[f"{name}/numerical_error"]
        print(f"{name}: mean n_steps {ns.mean():.1f}, max depth {int(data[name + '/tree_depth'].max())}, divergent {int((ne != 0).sum())} "
              f"(even n_steps {int(((ne != 0) & (ns % 2 == 0)).sum())}, odd > 1 {int(((ne != 0) & (ns % 2 == 1) & (ns > 1)).sum())})")
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    np.savez_compressed(out, **data)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
