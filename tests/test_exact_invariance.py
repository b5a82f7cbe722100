"""Exact invariance: chains started from the target stay distributed as the target (tests/invariance_util.py has the method).

Every other correctness test of the engine is a PARITY test — HIP kernels against the oracle, the oracle against ahmc_ref.py and the
reference's known answers: readings of the same Julia source by the same hands, and for the RankUpdate metric, the GLM target and the
plugin / kernel targets the only second reading is the author's own host mirror.  The tests here ask the one question parity cannot:
does a transition leave π invariant?  N chains start i.i.d. from π (own Philox stream each, a stationary momentum handed in through
`set_position(θ, r)`), T transitions run, and the whitened end points must pass `invariance_util.battery` — exact null distributions,
ALPHA = 1e-6 per test split over its checks, fixed seeds.  A test cannot pass by standing still: the mean acceptance_rate must lie in
[0.4, 0.95] and at least 99 % of the chains must have moved; no chain is left out of any statistic.

CPU (`-m "not gpu"`): the battery accepts i.i.d. draws (200 seeds per family), rejects planted defects at the GPU tests' N and T, and every
configuration the oracle can run passes ON THE ORACLE at the same N, T and ϵ (the step sizes were chosen there).  The oracle has no
RankUpdate metric, no GLM target, no plugin and no device-kernel target: those configurations are GPU-only (`oracle=False`) and the
closed-form distribution is the only reference they have.
`test_static_hmc_with_partial_refreshment_is_not_invariant_in_the_reference` pins quirk Q8: the battery REJECTS static HMC
with PartialMomentumRefreshment on the oracle, which restates src/trajectory.jl:279-283 faithfully; that kernel is therefore on no list.
Likewise Q9 (static MultinomialTS with TemperedLeapfrog) and, at 262 144 chains, Q4 (the coupled split of static MultinomialTS).

GPU (`-m gpu`): the same configurations on the HIP engine.  Each test appends its worst z, smallest p, acceptance and moved share to
exact_invariance.json under $AHMC_TEST_OUT (default: test_out/ in the repository root, ignored by git) — the convention of the other
recording tests, not the directory the issue named —; profiles/exact_invariance_margins.json holds the oracle's and the MI355X's records.
Every configuration that is there for one code path asserts that the path ran (`Cfg.expect`: thread geometry, launches of the batched
loop, tail normals, the dense epoch kernel, a wide context).
"""
import json
import os
from dataclasses import dataclass

import numpy as np
import pytest

import ahmc_amd as A
from ahmc_amd import _capi as capi
import invariance_util as U

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
UT = os.path.join(HERE, "user_targets")

# mean acceptance_rate over the T transitions.  Where ϵ is a schedule (EPS_SCHEDULES below) the mean is over both step sizes: on the
# funnel about 0.72 at the large ϵ and 0.99 at the small one — neither meets the range alone, which is why they alternate.  In run mode
# the engine keeps only the LAST transition's statistics, so the mean is over the chains of that one transition; the run-mode targets
# are Gaussians started from π, where every transition has the same law.
ACCEPT_RANGE = (0.4, 0.95)
MIN_MOVED = 0.99
BANANA_AB = (0.5, 0.5)


@dataclass(frozen=True)
class Cfg:
    name: str
    family: str
    D: int
    N: int
    T: int
    kern: str            # nuts-{mn,sl}-{gen,cls,str} | hmc-{ep,mn}-{L<n>,time}
    eps: object          # ϵ, or a tuple of them: transition t runs at eps[t % len(eps)] (each a valid kernel of its own, see EPS_SCHEDULES)
    metric: str = "unit"   # unit | diag (shared (D,)) | diagN (per chain) | dense | ru4 (RankUpdate, k = 4)
    dtype: str = "f64"
    integ: str = "lf"      # lf | jitter (JitteredLeapfrog(ϵ, 0.5)) | temper (TemperedLeapfrog(ϵ, 1.1))
    alpha: float = 0.0     # PartialMomentumRefreshment(alpha); 0: full
    depth: int = 10
    dmax: float = 1000.0
    form: str = "builtin"  # builtin | glm | plugin | kernel | external
    mode: str = "step"     # step: T × transition(); run: run(kernel, T, 0, samples_out=…), ensembles of draws T/4, T/2, 3T/4, T
    oracle: bool = True    # can the CPU oracle run it
    env: tuple = ()        # ((name, value), …): environment switches of the engine, set for the run (the engine reads them per call)
    expect: tuple = ()     # ((Engine.info key, "==" | ">" | "<", value), …): what the HIP engine must report after the run — the path ran

    def __str__(self):
        return self.name


F6 = dict(family="funnel", D=6, N=65536, T=16, depth=7)   # (depth 7: at the small ϵ of the schedule the wide chains end at the depth limit)
# EPS_SCHEDULES.  The funnel and the hierarchical Gaussian have a neck (x on the scale e^{y/2}, resp. τ = e^{log τ}) that no single ϵ serves:
# on the oracle the funnel at D = 6, T = 16 gives acceptance 0.87 / moved 0.946 at ϵ = 0.2, 0.96 / 0.988 at 0.08 and 0.98 / 0.995 at 0.05 —
# the two conditions (acceptance <= 0.95, >= 99 % of the chains moved) exclude each other.  A composition of π-invariant kernels is
# π-invariant, so these targets ALTERNATE a large ϵ (rejections, divergences, deep trees) with a small one (the neck moves): both
# conditions hold, on the oracle and on the GPU, at the same schedule.  The batched run() has one ϵ and takes the Gaussian targets.
FUNNEL_EPS = (0.4, 0.03)
SAMPLERS = [
    Cfg("nuts-mn-gen-unit", kern="nuts-mn-gen", eps=FUNNEL_EPS, metric="unit", **F6),
    Cfg("nuts-mn-cls-diag", kern="nuts-mn-cls", eps=FUNNEL_EPS, metric="diag", **F6),
    Cfg("nuts-mn-str-diagN", kern="nuts-mn-str", eps=FUNNEL_EPS, metric="diagN", **F6),
    Cfg("nuts-sl-gen-diag", kern="nuts-sl-gen", eps=FUNNEL_EPS, metric="diag", **F6),
    Cfg("nuts-sl-cls-diagN", kern="nuts-sl-cls", eps=FUNNEL_EPS, metric="diagN", **F6),
    Cfg("nuts-sl-str-unit", kern="nuts-sl-str", eps=FUNNEL_EPS, metric="unit", **F6),
    Cfg("hmc-ep-L5-diagN", kern="hmc-ep-L5", eps=FUNNEL_EPS, metric="diagN", **F6),
    Cfg("hmc-ep-time-unit", kern="hmc-ep-time", eps=FUNNEL_EPS, metric="unit", **F6),
    Cfg("hmc-mn-L5-diag", kern="hmc-mn-L5", eps=FUNNEL_EPS, metric="diag", **F6),
    Cfg("hmc-mn-time-diagN", kern="hmc-mn-time", eps=FUNNEL_EPS, metric="diagN", **F6),
    Cfg("nuts-mn-gen-diagN-f32", kern="nuts-mn-gen", eps=FUNNEL_EPS, metric="diagN", dtype="f32", **F6),
    Cfg("hmc-ep-L5-diag-f32", kern="hmc-ep-L5", eps=FUNNEL_EPS, metric="diag", dtype="f32", **F6),
]
INTEGRATORS = [
    Cfg("jitter-nuts-mn", kern="nuts-mn-gen", eps=FUNNEL_EPS, integ="jitter", metric="diag", **F6),
    Cfg("jitter-hmc-ep", kern="hmc-ep-L5", eps=FUNNEL_EPS, integ="jitter", metric="diagN", **F6),
    Cfg("temper-nuts-mn", kern="nuts-mn-gen", eps=FUNNEL_EPS, integ="temper", metric="diagN", **F6),
    Cfg("temper-hmc-ep", kern="hmc-ep-L5", eps=FUNNEL_EPS, integ="temper", metric="diag", **F6),
    Cfg("partial0.3-nuts-mn", kern="nuts-mn-gen", eps=FUNNEL_EPS, alpha=0.3, metric="diag", **F6),
    Cfg("partial0.9-nuts-mn", kern="nuts-mn-gen", eps=FUNNEL_EPS, alpha=0.9, metric="diagN", **F6),
    Cfg("partial0.3-nuts-sl", kern="nuts-sl-gen", eps=FUNNEL_EPS, alpha=0.3, metric="unit", **F6),
    Cfg("partial0.9-nuts-sl", kern="nuts-sl-cls", eps=FUNNEL_EPS, alpha=0.9, metric="diag", **F6),
    Cfg("dmax5-nuts-mn", kern="nuts-mn-gen", eps=FUNNEL_EPS, dmax=5.0, metric="unit", **F6),
]
G = dict(T=6, depth=5, kern="nuts-mn-gen")


def GEO(lanes, elems):
    return (("group_lanes", "==", lanes), ("elems_per_lane", "==", elems))


GEOMETRIES = [   # (G, E) of ahmc_api.hip: pick_geometry — chains per wave / waves per chain
    Cfg("geo-D3-iso", family="iso", D=3, N=65536, eps=0.9, metric="diagN", expect=GEO(4, 1), **G),            # (4, 1): 16 chains per wave
    Cfg("geo-D33-funnel", family="funnel", D=33, N=65536, eps=(0.25, 0.02), metric="diag", expect=GEO(32, 2), **G),       # (32, 2): 2 chains per wave
    Cfg("geo-D128-hier", family="hier", D=128, N=65536, eps=(0.1, 0.015), metric="unit", expect=GEO(64, 2), **G),         # (64, 2): cfg2's, one chain per wave
    Cfg("geo-D300-diag", family="diag", D=300, N=16384, eps=0.2, metric="diagN", expect=GEO(64, 8), **G),        # (64, 8)
    Cfg("geo-D600-hier", family="hier", D=600, N=8192, eps=(0.05, 0.008), metric="diag", expect=GEO(128, 8), **G),         # (128, 8): two waves, one-barrier hier path
    Cfg("geo-D2048-funnel", family="funnel", D=2048, N=2048, eps=(0.04, 0.004), metric="unit", expect=GEO(256, 8), **G),   # (256, 8): four waves
]
BATCHED = [
    Cfg("run-D32-diag", family="diag", D=32, N=16384, T=16, kern="nuts-mn-gen", eps=0.5, metric="diagN", depth=6, mode="run",
        expect=GEO(16, 2) + (("nuts_launches", "<", 16),)),                      # several transitions per launch, the engine's own lengths
    Cfg("run-D128-iso", family="iso", D=128, N=16384, T=16, kern="nuts-mn-gen", eps=0.5, metric="diag", depth=6, mode="run",
        env=(("AHMC_NUTS_DRAW_BATCH", "4"), ("AHMC_NORMALS_TAIL", "2")),         # four launches of four; each makes the next one's normals in its tail
        expect=GEO(64, 2) + (("nuts_launches", ">", 1), ("nuts_launches", "<", 16), ("norm_tail_hits", ">", 0))),
]
D24 = dict(D=24, N=16384, T=6, metric="dense")
EPOCH = dict(D=256, N=2048, T=6, metric="dense", env=(("AHMC_DENSE_EPOCH_MIN", "32"),), expect=(("dense_epoch_launches", ">", 0),))
EPOCH_EPS = 0.3
DENSE = [
    Cfg("dense-D24-dense", family="dense", kern="nuts-mn-gen", eps=0.5, depth=6, **D24),
    Cfg("dense-D24-funnel", family="funnel", kern="nuts-mn-gen", eps=(0.25, 0.02), depth=6, **D24),
    # the chain-complete epoch kernels serve a DenseGaussian target under a dense metric, and a pipeline of at least AHMC_DENSE_EPOCH_MIN
    # (default 2 048) running chains; N = 2 048 is cut into two pipelines of 1 024, so the threshold is lowered as in tests/test_gpu_parity.py
    Cfg("dense-D256-epoch", family="dense", kern="nuts-mn-gen", eps=EPOCH_EPS, depth=6, **EPOCH),
    Cfg("dense-D256-epoch-f32", family="dense", kern="nuts-mn-gen", eps=EPOCH_EPS, depth=6, dtype="f32", **EPOCH),
    Cfg("dense-D24-hmc-mn", family="dense", kern="hmc-mn-L5", eps=0.5, **D24),
    # k_d_temper is launched by the STATIC dense transitions only (dn_temper; the dense NUTS loop tempers inside k_d_tree2)
    # (T = 12: the tempered trajectory does not conserve H — acceptance 0.4 … 0.6 at every ϵ on the oracle — so six transitions leave 3 % of
    # the chains where they started.  Tempered static MultinomialTS, which would put k_d_mn_* under tempering too, is quirk Q9: on no list.)
    Cfg("dense-D24-temper-hmc-ep", family="dense", kern="hmc-ep-L5", eps=0.65, integ="temper", **{**D24, "T": 12}),
    Cfg("dense-D24-temper", family="dense", kern="nuts-mn-gen", eps=0.5, integ="temper", depth=6, **D24),
    Cfg("dense-D24-partial-nuts", family="dense", kern="nuts-mn-gen", eps=0.5, alpha=0.9, depth=6, **D24),
]
ENGINE_ONLY = [
    Cfg("ru4-D128-diag", family="diag", D=128, N=16384, T=6, kern="nuts-mn-gen", eps=0.3, metric="ru4", depth=5, oracle=False),
    Cfg("ru4-D600-hier", family="hier", D=600, N=4096, T=6, kern="nuts-mn-gen", eps=(0.05, 0.008), metric="ru4", depth=5, oracle=False),
    Cfg("wide-D5000-iso", family="iso", D=5000, N=1024, T=4, kern="nuts-mn-gen", eps=0.15, metric="diag", depth=5, expect=(("wide", "==", 1),)),
    Cfg("wide-D5000-hier", family="hier", D=5000, N=1024, T=4, kern="nuts-mn-gen", eps=(0.02, 0.003), metric="unit", depth=5, expect=(("wide", "==", 1),)),
    Cfg("glm-D17", family="glm", D=17, N=16384, T=6, kern="nuts-mn-gen", eps=0.35, metric="diag", depth=5, form="glm", oracle=False),
    Cfg("glm-D64", family="glm", D=64, N=16384, T=6, kern="nuts-mn-gen", eps=0.3, metric="unit", depth=5, form="glm", oracle=False),
    Cfg("banana-plugin-D128", family="banana", D=128, N=16384, T=6, kern="nuts-mn-gen", eps=0.2, metric="diagN", depth=5, form="plugin", oracle=False),
    Cfg("banana-kernel-D50", family="banana", D=50, N=16384, T=4, kern="nuts-mn-gen", eps=0.2, metric="diag", depth=5, form="kernel", oracle=False),
    Cfg("banana-external-D10", family="banana", D=10, N=16384, T=4, kern="nuts-mn-gen", eps=0.3, metric="diagN", depth=5, form="external"),
]
ALL = SAMPLERS + INTEGRATORS + GEOMETRIES + BATCHED + DENSE + ENGINE_ONLY
assert len({c.name for c in ALL}) == len(ALL)

# Q8: static HMC with PartialMomentumRefreshment — on NO list above; pinned on the oracle below
Q8 = Cfg("q8-static-partial0.9", family="dense", D=6, N=65536, T=4, kern="hmc-ep-L5", eps=0.6, alpha=0.9, metric="unit")
# Q9: static MultinomialTS with TemperedLeapfrog — on no list either; pinned on the oracle below
Q9 = Cfg("q9-static-multinomial-tempered", family="dense", D=6, N=65536, T=4, kern="hmc-mn-L5", eps=0.6, integ="temper", metric="unit")
# Q4: static MultinomialTS draws ONE forward / backward split per transition for all chains.  The configurations of the lists that use it
# (hmc-mn-*, dense-D24-hmc-mn) stay and pass at their N; at four times the chains the coupling shows, pinned on the oracle below
Q4 = Cfg("c", family="dense", D=6, N=262144, T=4, kern="hmc-mn-L5", eps=0.6, metric="unit")


# ---------------------------------------------------------------------------------------------------------------------
# building a configuration
# ---------------------------------------------------------------------------------------------------------------------
def _seed(cfg):
    return 1000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(cfg.name)) % 100000


def make_family(cfg):
    if cfg.family == "banana":
        return U.Banana(cfg.D, *BANANA_AB)
    return U.FAMILIES[cfg.family](cfg.D)


def make_metric(cfg, rs):
    """(the engine's metric, the momentum sampler / whitener of invariance_util for the same M⁻¹)"""
    D, N = cfg.D, cfg.N
    if cfg.metric == "unit":
        return A.UnitEuclideanMetric((D, N)), U.MomentumUnit(D)
    if cfg.metric == "diag":
        minv = 0.5 + rs.random(D)
        return A.DiagEuclideanMetric(minv), U.MomentumDiag(minv)
    if cfg.metric == "diagN":
        minv = np.asfortranarray(0.5 + rs.random((D, N)))
        return A.DiagEuclideanMetric(minv), U.MomentumDiag(minv)
    if cfg.metric == "dense":
        Q, _ = np.linalg.qr(rs.normal(size=(D, D)))
        Mi = (Q * np.linspace(0.6, 2.0, D)) @ Q.T
        Mi = (Mi + Mi.T) / 2
        return A.DenseEuclideanMetric(np.asfortranarray(Mi)), U.MomentumDense(Mi)
    assert cfg.metric == "ru4"
    a = 0.5 + rs.random(D)
    B = rs.normal(size=(D, 4)) / np.sqrt(D)
    Gm = rs.normal(size=(4, 4))
    Dk = Gm @ Gm.T / 4 + 0.5 * np.eye(4)
    return A.RankUpdateEuclideanMetric(a, np.asfortranarray(B), np.asfortranarray(Dk)), U.momentum_rank_update(a, B, Dk)


def make_target(cfg, fam, keep):
    """the engine's target for the family in the form the configuration asks for; `keep` holds what must outlive the engine"""
    if cfg.form == "glm":
        return A.GLMTarget(fam.X, fam.y, family="gaussian_identity", prior_prec=fam.prior_prec, offset=fam.offset, scale=fam.scale)
    if cfg.family == "banana":
        a, b = BANANA_AB
        if cfg.form == "plugin":
            return A.PluginTarget(cfg.D, os.path.join(UT, "banana.hpp"), params=np.array([a, b]))
        if cfg.form == "external":
            from test_user_targets import banana_numpy

            return A.ExternalTarget(cfg.D, banana_numpy(a, b))
        assert cfg.form == "kernel"
        import torch
        from ahmc_amd.build import build_code_object
        from ahmc_amd.hipmod import Module

        mod = Module(build_code_object(os.path.join(UT, "kernels.hip")))
        user = torch.tensor([a, b], dtype=torch.float64, device="cuda")
        keep += [mod, user]
        return A.KernelTarget(cfg.D, mod.function("banana_f64"), handle_kind=capi.KERNEL_HIP_FUNCTION, block_threads=256, chains_per_block=4,
                              user=user.data_ptr())
    assert cfg.form == "builtin"
    if cfg.family == "iso":
        return A.IsoGaussian(cfg.D)
    if cfg.family == "diag":
        return A.DiagGaussian(fam.m, fam.s)
    if cfg.family == "funnel":
        return A.Funnel(cfg.D)
    if cfg.family == "hier":
        return A.HierGaussian(cfg.D)
    assert cfg.family == "dense"
    return A.DenseGaussian(fam.P)


def eps_at(cfg, t):
    return cfg.eps[t % len(cfg.eps)] if isinstance(cfg.eps, tuple) else cfg.eps


def make_kernel(cfg, t=0):
    eps = eps_at(cfg, t)
    lf = {"lf": lambda: A.Leapfrog(eps), "jitter": lambda: A.JitteredLeapfrog(eps, 0.5),
          "temper": lambda: A.TemperedLeapfrog(eps, 1.1)}[cfg.integ]()
    kind, ts, rule = cfg.kern.split("-")
    TS = {"ep": A.EndPointTS, "mn": A.MultinomialTS, "sl": A.SliceTS}[ts]
    if kind == "nuts":
        crit = {"gen": A.GeneralisedNoUTurn, "cls": A.ClassicNoUTurn, "str": A.StrictGeneralisedNoUTurn}[rule]
        tc = crit(max_depth=cfg.depth, delta_max=cfg.dmax)
    elif rule == "time":
        tc = A.FixedIntegrationTime(5.5 * eps)      # floor(λ/ϵ) = 5 leapfrog steps, away from the rounding of the quotient
    else:
        tc = A.FixedNSteps(int(rule[1:]))
    tau = A.Trajectory(TS, lf, tc)
    return lf, (A.HMCKernel(A.PartialMomentumRefreshment(cfg.alpha), tau) if cfg.alpha else A.HMCKernel(tau))


def jointly_invariant(cfg):
    """(θ, r) is invariant under every kernel of the lists; static + partial refreshment (Q8) is the exception and on no list"""
    return not (cfg.kern.startswith("hmc") and cfg.alpha)


def run_config(cfg, lib, alpha=U.ALPHA):
    """start from π, T transitions, battery; returns the record (verdicts, acceptance, moved share)"""
    dtype = {"f64": np.float64, "f32": np.float32}[cfg.dtype]
    rs = np.random.default_rng(_seed(cfg))
    fam = make_family(cfg)
    metric, mom = make_metric(cfg, rs)
    keep = []
    target = make_target(cfg, fam, keep)
    th0 = np.asfortranarray(fam.draw(cfg.N, rs))
    r0 = np.asfortranarray(mom.draw(cfg.N, rs))
    lf, kernel = make_kernel(cfg)
    saved = {k: os.environ.get(k) for k, _ in cfg.env}
    os.environ.update(dict(cfg.env))
    e = None
    try:
        e = A.Engine(A.Hamiltonian(metric, target), cfg.N, dtype=dtype, rng=A.PhiloxRNG(_seed(cfg)), lib=lib)
        e.set_integrator(lf)
        e.set_position(th0, r0)
        start = e.phasepoint().theta.astype(np.float64)     # (θ0 as the engine holds it: rounded once for Float32)
        ensembles = []
        if cfg.mode == "run":
            assert not isinstance(cfg.eps, tuple)
            draws = np.zeros((cfg.D, cfg.N, cfg.T), dtype=dtype, order="F")
            e.run(kernel, cfg.T, 0, samples_out=draws)
            e.sync()
            acc = [float(e.stats(["acceptance_rate"])["acceptance_rate"].astype(np.float64).mean())]   # (run() keeps the last transition's)
            for k in (cfg.T // 4, cfg.T // 2, 3 * cfg.T // 4, cfg.T):
                ensembles.append((f"draw{k}", draws[:, :, k - 1].astype(np.float64)))
            z = e.phasepoint()
            np.testing.assert_array_equal(z.theta, draws[:, :, cfg.T - 1])
        else:
            acc = []
            for t in range(cfg.T):
                if t and isinstance(cfg.eps, tuple):
                    lf, kernel = make_kernel(cfg, t)
                    e.set_integrator(lf)
                e.transition(kernel)
                acc.append(float(e.stats(["acceptance_rate"])["acceptance_rate"].astype(np.float64).mean()))
            z = e.phasepoint()
            ensembles.append(("end", z.theta.astype(np.float64)))
        r_end = z.r.astype(np.float64)
        if lib.backend.startswith("hip"):      # the path the configuration is there for RAN: no quiet fall-back to another kernel
            for key, op, want in cfg.expect:
                got = e.info(key)
                assert {"==": got == want, ">": got > want, "<": got < want}[op], (cfg.name, key, got, op, want)
    finally:
        if e is not None:
            e.close()
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    rec = {"config": cfg.name, "D": cfg.D, "N": cfg.N, "T": cfg.T, "eps": cfg.eps, "dtype": cfg.dtype, "acceptance": float(np.mean(acc)),
           "acceptance_over": "the last transition" if cfg.mode == "run" else "all T transitions", "ensembles": {}}
    for i, (label, th) in enumerate(ensembles):
        arrays = {"theta": fam.whiten(th)}
        if i == len(ensembles) - 1 and jointly_invariant(cfg):
            arrays["r"] = mom.whiten(r_end)
        v = U.battery(arrays, alpha / len(ensembles))
        v["moved"] = float((th != start).any(axis=0).mean())
        v["failed"] = [list(c) for c in v["failed"]]
        rec["ensembles"][label] = v
    rec["ok"] = all(v["ok"] for v in rec["ensembles"].values())
    rec["min_p"] = min(v["min_p"] for v in rec["ensembles"].values())
    rec["worst_z"] = max((v["worst_z"] for v in rec["ensembles"].values()), key=abs)
    rec["moved"] = min(v["moved"] for v in rec["ensembles"].values())
    return rec


def check_record(rec):
    print(json.dumps({k: rec[k] for k in ("config", "acceptance", "moved", "min_p", "worst_z")}))
    for label, v in rec["ensembles"].items():
        assert v["ok"], (f"{rec['config']} {label}: {v['n_failed']} of {v['m']} checks below p = {v['threshold']:.3g}: {v['failed']} "
                         f"(acceptance {rec['acceptance']:.3f}, moved {v['moved']:.4f})")
        assert v["moved"] >= MIN_MOVED, (rec["config"], label, v["moved"])
    assert ACCEPT_RANGE[0] <= rec["acceptance"] <= ACCEPT_RANGE[1], (rec["config"], rec["acceptance"])


# ---------------------------------------------------------------------------------------------------------------------
# the record of a run: $AHMC_TEST_OUT/exact_invariance.json (default test_out/), {backend: {configuration: record}}
# ---------------------------------------------------------------------------------------------------------------------
RECORD_FILE = os.path.join(os.environ.get("AHMC_TEST_OUT") or os.path.join(ROOT, "test_out"), "exact_invariance.json")


def record(backend, rec):
    try:
        os.makedirs(os.path.dirname(RECORD_FILE), exist_ok=True)
        try:
            with open(RECORD_FILE) as f:
                allrec = json.load(f)
        except (OSError, ValueError):
            allrec = {}
        slim = {k: rec[k] for k in ("D", "N", "T", "eps", "dtype", "acceptance", "acceptance_over", "moved", "min_p", "worst_z", "ok")}
        slim["checks"] = sum(v["m"] for v in rec["ensembles"].values())
        allrec.setdefault(backend, {})[rec["config"]] = slim
        with open(RECORD_FILE, "w") as f:
            json.dump(allrec, f, indent=1, sort_keys=True)
    except OSError:
        pass


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the statistics
# ---------------------------------------------------------------------------------------------------------------------
def test_tail_probabilities_against_scipy_and_mpmath():
    """erfc / torch.special.gammainc(c) in float64 against scipy and mpmath at the degrees of freedom (N, D·N, D of the lists) and the tail
    levels (p down to ALPHA / m ≈ 1e-10) the battery uses.  A p-value within 1e-6 relative is far more than the decision p >= ALPHA/m needs."""
    stats = pytest.importorskip("scipy.stats")
    mp = pytest.importorskip("mpmath")
    zs = np.array([-6.8, -6.0, -5.0, -3.0, -1.0, 0.0, 0.5, 3.0, 5.0, 6.0, 6.8])
    np.testing.assert_allclose(U.normal_two_sided(zs), 2 * stats.norm.sf(np.abs(zs)), rtol=1e-12)
    for v in (-6.0, 5.0):
        assert abs(U.normal_two_sided(v)[0] / float(mp.erfc(abs(v) / mp.sqrt(2))) - 1) < 1e-12
    dofs = sorted({c.N for c in ALL} | {c.D * c.N for c in ALL} | {c.D for c in ALL})
    for k in dofs:
        x = k + zs * np.sqrt(2.0 * k)
        x = x[x > 0]
        lo, hi = U.chi2_tails(x, k)
        np.testing.assert_allclose(lo, stats.chi2.cdf(x, k), rtol=1e-6, atol=1e-300)
        np.testing.assert_allclose(hi, stats.chi2.sf(x, k), rtol=1e-6, atol=1e-300)
        np.testing.assert_allclose(U.chi2_two_sided(x, k), np.minimum(1, 2 * np.minimum(stats.chi2.cdf(x, k), stats.chi2.sf(x, k))), rtol=1e-6)
    for k in (3, 6, 24, 128, 1024, 65536):     # mpmath: an implementation that shares no code with torch's or scipy's
        for v in (-5.0, 6.0):
            x = k + v * np.sqrt(2.0 * k)
            if x <= 0:
                continue
            lo, hi = U.chi2_tails(x, k)
            ref = mp.gammainc(mp.mpf(k) / 2, 0, mp.mpf(x) / 2, regularized=True) if v < 0 else mp.gammainc(mp.mpf(k) / 2, mp.mpf(x) / 2, mp.inf, regularized=True)
            assert abs((lo if v < 0 else hi)[0] / float(ref) - 1) < 1e-6, (k, v)
    # the Kolmogorov series against scipy's
    for lam in (0.3, 0.5, 1.0, 1.5, 2.0, 3.0, 3.5):
        assert abs(U.kolmogorov_sf(lam) / stats.kstwobign.sf(lam) - 1) < 1e-9, lam
    # … and the KS statistic and Stephens' correction against scipy's exact one-sample test (N >= 1024: within a few per cent of p)
    x = np.random.default_rng(0).standard_normal((3, 4096)) * np.array([[1.0], [1.03], [1.06]])
    d = U.ks_statistic(U.normal_cdf(x))
    for row, dv in zip(x, d):
        res = stats.kstest(row, "norm")
        assert abs(dv - res.statistic) < 1e-12
        assert abs(np.log(U.ks_pvalue(dv, 4096) / res.pvalue)) < 0.1, (U.ks_pvalue(dv, 4096), res.pvalue)


def test_ks_coordinates():
    for D in (3, 64, 65, 128, 300, 600, 2048, 5000):
        c = U.ks_coordinates(D)
        assert len(c) == min(D, 64) == len(set(c.tolist())) and c.min() >= 0 and c.max() < D
        if D > 64:
            assert {0, 1, 63, 64, D - 1} <= set(c.tolist())
    assert {0, 511, 512, 599} <= set(U.ks_coordinates(600).tolist())
    assert {0, 511, 512, 1023, 1024, 1535, 1536, 2047} <= set(U.ks_coordinates(2048).tolist())


@pytest.mark.parametrize("family", sorted(U.FAMILIES))
def test_battery_accepts_exact_draws(family):
    """i.i.d. draws of every family, whitened, over 200 seeds: the false-alarm probability of all 200 together is 2e-4"""
    fam = U.Banana(7, *BANANA_AB) if family == "banana" else U.FAMILIES[family](7)
    for seed in range(200):
        v = U.battery({"theta": fam.whiten(fam.draw(2048, np.random.default_rng(seed)))})
        assert v["ok"], (family, seed, v["failed"])


@pytest.mark.parametrize("metric", ["unit", "diag", "diagN", "dense", "ru4"])
def test_battery_accepts_exact_momenta(metric):
    """r ~ N(0, M) of every metric; and the whitened momentum has kinetic energy ½|z|² = ½ rᵀM⁻¹r as the package's metric defines it"""
    cfg = Cfg("m", "iso", 9, 2048, 1, "nuts-mn-gen", 0.1, metric=metric)
    m, mom = make_metric(cfg, np.random.default_rng(5))
    for seed in range(50):
        r = mom.draw(cfg.N, np.random.default_rng(seed))
        z = mom.whiten(r)
        assert U.battery({"r": z})["ok"], (metric, seed)
    if metric == "ru4":
        W = np.diag(m.A) + m.B @ m.D @ m.B.T
    elif metric == "unit":
        W = np.eye(cfg.D)
    else:
        W = None if metric == "diagN" else (np.diag(m.Minv) if metric == "diag" else m.Minv)
    ke = (r * (m.Minv * r)).sum(axis=0) if W is None else (r * (W @ r)).sum(axis=0)
    np.testing.assert_allclose((z * z).sum(axis=0), ke, rtol=1e-10)


def test_banana_and_glm_whiteners_match_the_densities():
    """the closed forms of invariance_util against the densities the engine is given: −½|whiten(θ)|² − ℓπ(θ) is one constant over θ"""
    from test_user_targets import banana_numpy

    rs = np.random.default_rng(1)
    for D in (7, 10):
        fam = U.Banana(D, *BANANA_AB)
        th = 2 * rs.normal(size=(D, 50))
        c = -0.5 * (fam.whiten(th) ** 2).sum(axis=0) - banana_numpy(*BANANA_AB)(th)[0]
        np.testing.assert_allclose(c, c[0], rtol=0, atol=1e-9)
    fam = U.GaussianGLM(17)
    t = A.GLMTarget(fam.X, fam.y, family="gaussian_identity", prior_prec=fam.prior_prec, offset=fam.offset, scale=fam.scale)
    th = 2 * rs.normal(size=(17, 50))
    c = -0.5 * (fam.whiten(th) ** 2).sum(axis=0) - t.logdensity(th)[0]
    np.testing.assert_allclose(c, c[0], rtol=0, atol=1e-8)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: non-vacuity — a correct numpy sampler passes, planted defects are rejected, at the N and T of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
def _numpy_hmc(kinetic_weight, seed=11):
    fam = U.Funnel(F6["D"])
    rs = np.random.default_rng(seed)
    th0 = fam.draw(F6["N"], rs)
    th, acc = U.numpy_static_hmc(U.funnel_logp_grad, th0, (0.5, 0.03), 7, F6["T"], rs, kinetic_weight)
    return U.battery({"theta": fam.whiten(th)}), acc, float((th != th0).any(axis=0).mean())


def test_correct_numpy_hmc_passes():
    v, acc, moved = _numpy_hmc(1.0)
    assert v["ok"], v["failed"]
    assert ACCEPT_RANGE[0] <= acc <= ACCEPT_RANGE[1] and moved >= MIN_MOVED, (acc, moved)


def test_kinetic_energy_misweighted_by_4_percent_is_rejected():
    v, acc, moved = _numpy_hmc(1.04)
    print(v["min_p"], v["worst_z"], acc, moved)
    assert not v["ok"] and v["min_p"] < 1e-20, v


def test_scale_error_of_2_percent_in_one_coordinate_is_rejected():
    """no transition at all: θ0 with one coordinate scaled by 1.02"""
    fam = U.Funnel(F6["D"])
    th = fam.draw(F6["N"], np.random.default_rng(12))
    assert U.battery({"theta": fam.whiten(th)})["ok"]
    th[3] *= 1.02
    v = U.battery({"theta": fam.whiten(th)})
    print(v["min_p"], v["worst_z"])
    assert not v["ok"], v


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the oracle on every configuration it can run, and the pinned quirk
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [c for c in ALL if c.oracle], ids=str)
def test_oracle_leaves_target_invariant(oracle, cfg):
    rec = run_config(cfg, oracle)
    record("oracle", rec)
    check_record(rec)


def test_gpu_only_configurations_say_so():
    """what the oracle cannot run: the RankUpdate metric, the GLM target, a target compiled into or launched by the engine"""
    assert {c.name for c in ALL if not c.oracle} == {c.name for c in ALL if c.metric == "ru4" or c.form in ("glm", "plugin", "kernel")}


def test_static_hmc_with_partial_refreshment_is_not_invariant_in_the_reference(oracle):
    """Q8.  src/trajectory.jl:279-283 reverses the momentum after accept AND after reject; with a momentum that persists
    (PartialMomentumRefreshment) that is no Metropolis step with an involution, and π is not left invariant.  The oracle restates the lines
    (oracle/ahmc_oracle.cpp: hmc_transition_chain), the engine keeps parity with them, and the battery REJECTS the kernel: dense Gaussian,
    D = 6, unit metric, ϵ = 0.6, L = 5, α = 0.9, N = 65 536, T = 4 — the real-sampler evidence that the battery has power.  The same
    refreshment with NUTS (no reversal there) is on the lists above and passes."""
    rec = run_config(Q8, oracle)
    record("oracle", rec)
    print(json.dumps({k: rec[k] for k in ("acceptance", "moved", "min_p", "worst_z")}))
    assert ACCEPT_RANGE[0] <= rec["acceptance"] <= ACCEPT_RANGE[1] and rec["moved"] >= MIN_MOVED   # it moves — and misses π
    assert not rec["ok"] and rec["min_p"] < 1e-20 and abs(rec["worst_z"]) > 8, rec


def test_static_multinomial_with_tempered_leapfrog_is_not_invariant_in_the_reference(oracle):
    """Q9.  `sample_phasepoint(::Trajectory{MultinomialTS})` (src/trajectory.jl:369-390) integrates n_fwd steps forward and
    L − n_fwd backward, each a `step` of its own, and weighs every point by exp(−H).  With TemperedLeapfrog each part is tempered over ITS
    OWN length (`temper`, src/integrator.jl:199-209: r·√α in the first half of the half-steps, r/√α in the second), so the intermediate
    points carry a momentum scaled by powers of √α: the map to them does not preserve volume and exp(−H) is not their weight.  The oracle
    restates the lines; the battery rejects the kernel (D = 6, unit metric, ϵ = 0.6, L = 5, α = 1.1, T = 4).  The same integrator with
    EndPointTS (whole trajectory: the scalings cancel) and with NUTS (one step per leaf) is on the lists and passes."""
    rec = run_config(Q9, oracle)
    record("oracle", rec)
    print(json.dumps({k: rec[k] for k in ("acceptance", "moved", "min_p", "worst_z")}))
    assert ACCEPT_RANGE[0] <= rec["acceptance"] <= ACCEPT_RANGE[1] and rec["moved"] >= MIN_MOVED
    assert not rec["ok"] and rec["min_p"] < 1e-20 and abs(rec["worst_z"]) > 8, rec


def test_static_multinomial_couples_the_chains_through_one_split(oracle):
    """Q4 seen by the battery.  Static MultinomialTS draws ONE n_steps_fwd per transition for ALL chains (src/trajectory.jl:371-373,
    `rand_coupled`).  Given the split, choosing among the points of a trajectory with a fixed offset does not leave π invariant — only the
    average over the split does — so the N end points are exchangeable draws with a common random component, not N independent ones: each
    chain's law is π, the ensemble's statistics are not those of an i.i.d. sample.  At 262 144 chains (D = 6, ϵ = 0.6, L = 5, T = 4) the
    battery rejects, with a sign that changes with the seed; at the 65 536 and 16 384 chains of the lists the same kernel passes (its
    records: hmc-mn-L5-diag, hmc-mn-time-diagN, dense-D24-hmc-mn), and those tests hold a per-chain defect to the same bounds as the
    others — but for this one trajectory sampler ALPHA is not an exact false-alarm probability."""
    rec = run_config(Q4, oracle)
    print(json.dumps({k: rec[k] for k in ("acceptance", "moved", "min_p", "worst_z")}))
    assert ACCEPT_RANGE[0] <= rec["acceptance"] <= ACCEPT_RANGE[1] and rec["moved"] >= MIN_MOVED
    assert not rec["ok"] and rec["min_p"] < 1e-20 and abs(rec["worst_z"]) > 8, rec


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _gpu(hip, cfg):
    rec = run_config(cfg, hip)
    record(hip.backend, rec)
    check_record(rec)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", SAMPLERS, ids=str)
def test_samplers_leave_target_invariant(hip, cfg):
    _gpu(hip, cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", INTEGRATORS, ids=str)
def test_integrators_and_refreshments_leave_target_invariant(hip, cfg):
    _gpu(hip, cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", GEOMETRIES, ids=str)
def test_thread_geometries_leave_target_invariant(hip, cfg):
    _gpu(hip, cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", BATCHED, ids=str)
def test_batched_loop_leaves_target_invariant(hip, cfg):
    """run(kernel, 16, 0, samples_out=…): the multi-transition launches, the dispatch order and the tail normals; the ensembles of draws
    4, 8, 12 and 16 each get their own battery at ALPHA / 4"""
    _gpu(hip, cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", DENSE, ids=str)
def test_dense_engine_leaves_target_invariant(hip, cfg):
    _gpu(hip, cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ENGINE_ONLY, ids=str)
def test_engine_only_paths_leave_target_invariant(hip, cfg):
    """RankUpdate metric, wide contexts, the GLM target, the banana as plugin / device kernel / external target: where `cfg.oracle` is
    False no oracle exists and the closed-form distribution is the only reference"""
    if cfg.D > 4096:
        e = A.Engine(A.Hamiltonian(A.UnitEuclideanMetric((cfg.D, 4)), A.IsoGaussian(cfg.D)), 4, lib=hip)
        assert e.info("wide") == 1
        e.close()
    _gpu(hip, cfg)
