"""Guard-band tests: no call of the C ABI reads or writes outside the caller's arrays.

include/ahmc_hip.h: "a `const void*`/`void*` array argument may be a host pointer or a device pointer … the caller owns every
pointer it passes" — and the callers' allocators pack the next tensor directly behind it.  Every array argument of every entry
point is handed in here as a view in the middle of an arena the test owns (tests/arena_util.py) and held, bit for bit, to

    W  no stray write   F  fully written   R  no stray read   C  inputs are const

The cases call the C ABI directly (`lib.dll.ahmc_*` with `e._ctx`): the `Engine` wrappers allocate their own outputs and would
hide the buffer.  One table of cases serves three runs: against the CPU checker in host arenas (not marked gpu: it proves the
cases and holds the checker to the same contract), against the HIP engine in device / host / pinned arenas (gpu), and the dry run
of the gpu cases on the checker.  `test_gate_every_array_argument_is_probed` parses the headers and fails when a pointer
parameter is neither probed by a case nor listed, with its reason, in NOT_ARRAYS.

What the thread geometry, the launch split and the engine routing of a case are is asserted through ahmc_get_info where the
engine reports them; the epoch kernels' routing is decided in csrc/ahmc_dense_host.hpp (dn_nuts_transition: `epoch_ok`).
"""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import ahmc_amd as A
import arena_util as AU
from ahmc_amd import capi
from arena_util import In, Out

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32 = np.float64, np.float32

# (G, E) the engine must pick for each D of tests/test_gpu_parity.py: GEOM_D (csrc/ahmc_api.hip: pick_geometry)
GEOM = {3: (4, 1), 5: (4, 2), 10: (8, 2), 24: (16, 2), 32: (16, 2), 50: (32, 2), 100: (64, 2), 128: (64, 2), 200: (64, 4), 300: (64, 8),
        600: (128, 8), 1500: (256, 8), 2048: (256, 8), 4096: (512, 8)}


# ------------------------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, cid, fn, probes, oracle, kw):
        self.cid, self.fn, self.probes, self.oracle, self.kw = cid, fn, tuple(probes), oracle, kw


CASES = {}


def add(cid, fn, probes, oracle=True, **kw):
    assert cid not in CASES, cid
    CASES[cid] = Case(cid, fn, probes, oracle, kw)


class Run:
    """what a case function gets: the library, whether it is the HIP engine (then 'device' / 'pinned' arenas are real), the
    monkeypatch fixture for the launch-length switches, and `probe`, which also records which arguments the case really probed"""

    def __init__(self, lib, mp, case):
        self.lib, self.mp, self.case = lib, mp, case
        self.dev = lib.backend == "hip:gfx950"
        self.used = set()

    def ok(self, e, rc):
        self.lib.check(rc, e._ctx if e is not None else None)

    def probe(self, setup, call, ins=None, outs=None, sync=True):
        ins, outs = ins or {}, outs or {}
        keys = set(ins) | set(outs)
        assert keys <= set(self.case.probes), f"{self.case.cid}: {sorted(keys - set(self.case.probes))} not declared in the case's probes"
        self.used |= keys
        sy = (lambda e: self.ok(e, self.lib.dll.ahmc_sync(e._ctx))) if sync else None
        return AU.probe(setup, call, ins, outs, on_device=self.dev, sync=sy)


def run_case(lib, mp, cid):
    case = CASES[cid]
    r = Run(lib, mp, case)
    case.fn(r, **case.kw)
    assert r.used == set(case.probes), f"{cid}: declared but not probed: {sorted(set(case.probes) - r.used)}"


# ------------------------------------------------------------------------------------------------------------------------------
# contexts
# ------------------------------------------------------------------------------------------------------------------------------
def spd(rs, D):
    W = rs.normal(size=(D, D)) / np.sqrt(D)
    return np.asfortranarray(W @ W.T + np.eye(D))


def engine(lib, D, N, dtype, metric="diag_chain", target="iso", seed=5, eps=0.3, adaptor=None, position=True):
    """a context in a state that depends on the arguments alone"""
    rs = np.random.default_rng(1000 * seed + D)
    if metric == "unit":
        m = A.UnitEuclideanMetric(dtype, (D, N))
    elif metric == "diag":
        m = A.DiagEuclideanMetric(0.5 + rs.random(D))
    elif metric == "diag_chain":
        m = A.DiagEuclideanMetric(np.asfortranarray(0.5 + rs.random((D, N))))
    else:
        m = A.DenseEuclideanMetric(spd(rs, D))
    if target == "iso":
        t = A.IsoGaussian(D)
    elif target == "dense":
        t = A.DenseGaussian(spd(rs, D))
    elif target == "external":
        t = A.ExternalTarget(D, lambda th: (-0.5 * np.sum(np.square(th), axis=0), -th))
    else:
        t = target
    e = A.Engine(A.Hamiltonian(m, t), N, dtype=dtype, rng=A.PhiloxRNG(seed), lib=lib)
    lf = A.Leapfrog(np.full(N, eps) * (0.8 + 0.4 * rs.random(N)))
    e.set_integrator(lf)
    if position:
        e.set_position(np.asfortranarray(rs.normal(size=(D, N))), np.asfortranarray(rs.normal(size=(D, N))))
    if adaptor == "stepsize":
        e.adaptor_init(A.StepSizeAdaptor(0.8, lf))
    elif adaptor in ("welford", "nutpie"):
        pc = (A.MassMatrixAdaptor if adaptor == "welford" else A.NutpieVar)(m)
        e.adaptor_init(A.StanHMCAdaptor(pc, A.StepSizeAdaptor(0.8, lf), init_buffer=2, term_buffer=2, window_size=3))
    return e


def nuts_cfg(max_depth=2):
    k = capi.KernelCfg()
    k.nuts, k.sampler, k.criterion, k.max_depth, k.delta_max = 1, capi.TS_MULTINOMIAL, capi.TC_GENERALISED, max_depth, 1000.0
    return k


def hmc_cfg(sampler, L=3):
    k = capi.KernelCfg()
    k.nuts, k.sampler, k.L = 0, sampler, L
    return k


def observe(e, transition=True):
    """the state a setter or an ingest path leaves behind, as arrays: the phase point, the step sizes and — the state in use — the
    position after one NUTS transition"""
    z = e.phasepoint()
    out = {"theta": z.theta, "r": z.r, "lp": z.lp.value, "grad": z.lp.gradient, "lk": z.lk.value, "eps": e.get_stepsize()}
    if transition:
        k = nuts_cfg()
        e._call("ahmc_nuts_transition", k.max_depth, k.delta_max, k.criterion, k.sampler)
        out["theta_after"] = e.theta()
    return {k: np.asarray(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------------------------------------
# ahmc_sample / ahmc_sample_from: samples_out
# ------------------------------------------------------------------------------------------------------------------------------
SO, SFO = "ahmc_sample.samples_out", "ahmc_sample_from.samples_out"


def sample_case(r, mk, cfg, D, N, dtype, n_samples=4, n_adapts=1, drop=0, where="device", check=None):
    n_keep = n_samples - (n_adapts if drop else 0)

    def call(e, io):
        k = cfg()
        r.ok(e, r.lib.dll.ahmc_sample(e._ctx, C.byref(k), n_samples, n_adapts, drop, io[SO]))
        r.ok(e, r.lib.dll.ahmc_sync(e._ctx))
        if check is not None:
            check(e)
        return {"theta_end": e.theta()}

    r.probe(mk, call, outs={SO: Out(dtype, D * N * n_keep, where)})


def c_sample_nuts(r, D, dtype):
    """every thread geometry of the fused NUTS kernels; drop_warmup = 1: an extent of 3 draws, the warm-up draw writes nothing"""
    for N in (1, 5, 67):
        def mk():
            e = engine(r.lib, D, N, dtype, adaptor="stepsize")
            assert not r.dev or (e.info("group_lanes"), e.info("elems_per_lane")) == GEOM[D]
            return e

        for drop in (0, 1):
            sample_case(r, mk, nuts_cfg, D, N, dtype, drop=drop)


def c_sample_hmc(r, D, sampler):
    for N, dtype in ((5, F64), (67, F64), (67, F32)):
        for drop in (0, 1):
            sample_case(r, lambda: engine(r.lib, D, N, dtype, adaptor="stepsize"), lambda: hmc_cfg(sampler), D, N, dtype, drop=drop)


def c_sample_dense(r, D):
    """DenseEuclideanMetric: the step-synchronous engine"""
    for N, dtype in ((5, F64), (67, F64), (67, F32)):
        def check(e):
            assert not r.dev or e.info("dense_pool") == 1
        for drop in (0, 1):
            sample_case(r, lambda: engine(r.lib, D, N, dtype, metric="dense", adaptor="stepsize"), nuts_cfg, D, N, dtype, drop=drop, check=check)


def c_sample_epoch(r, dtype):
    """the chain-complete dense kernels: D = 256 with a dense metric and a dense Gaussian target routes to k_dense_epoch in Float64 and
    to k_dense_epoch2 in Float32 once a pipeline has AHMC_DENSE_EPOCH_MIN running chains (csrc/ahmc_dense_host.hpp: epoch_ok).  N = 67:
    two full workgroups of chains and a partial one."""
    D, N = 256, 67
    r.mp.setenv("AHMC_DENSE_EPOCH_MIN", "32")
    for var in ("AHMC_DENSE_EPOCH", "AHMC_DENSE_EPOCH_V", "AHMC_DENSE_EPOCH_NCT", "AHMC_DENSE_EPOCH_WPE", "AHMC_DENSE_CHUNK"):
        r.mp.delenv(var, raising=False)

    def check(e):
        assert not r.dev or e.info("dense_epoch_launches") > 0

    sample_case(r, lambda: engine(r.lib, D, N, dtype, metric="dense", target="dense", eps=0.1), nuts_cfg, D, N, dtype, n_adapts=0, check=check)


def c_sample_wide(r):
    D, N = 4097, 3

    def mk():
        e = engine(r.lib, D, N, F64, adaptor="stepsize")
        assert not r.dev or e.info("wide") == 1
        return e

    for drop in (0, 1):
        sample_case(r, mk, nuts_cfg, D, N, F64, drop=drop)


def glm_target(n_obs=70, P=3, seed=3):
    rs = np.random.default_rng(seed)
    X = rs.normal(size=(n_obs, P))
    return A.GLMTarget(X, (rs.random(n_obs) < 0.5).astype(float), family="bernoulli_logit", prior_scale=2.0, offset=0.1 * rs.normal(size=n_obs))


def c_sample_glm(r):
    D, N = 3, 67
    for dtype in (F64, F32):
        sample_case(r, lambda: engine(r.lib, D, N, dtype, target=glm_target(), adaptor="stepsize"), nuts_cfg, D, N, dtype, drop=1)


def c_sample_split(r, where):
    """n_keep = 5 split across three launches (2 + 2 + 1 transitions): the per-launch offset into samples_out and, for a host
    buffer, the staged device-to-host copies and their byte counts.  The switches are read at every ahmc_sample call."""
    D, N = 10, 67
    r.mp.setenv("AHMC_NUTS_BATCH", "2")
    r.mp.setenv("AHMC_NUTS_DRAW_BATCH", "2")
    for dtype in (F64, F32):
        seen = []

        def mk():
            e = engine(r.lib, D, N, dtype)
            seen.append(e.info("nuts_launches"))
            return e

        def check(e):
            assert not r.dev or e.info("nuts_launches") - seen[-1] >= 2, (e.info("nuts_launches"), seen[-1])

        sample_case(r, mk, nuts_cfg, D, N, dtype, n_samples=5, n_adapts=0, where=where, check=check)


def c_sample_from(r, where):
    """a resumed run writes draws 3 … 5 of the full-size buffer; draws 1 – 2 keep their pre-fill"""
    D, N, n = 5, 67, 5
    for dtype in (F64, F32):
        def mk():
            e = engine(r.lib, D, N, dtype)
            k = nuts_cfg()
            e._call("ahmc_sample", C.byref(k), 2, 0, 0, None)
            return e

        def call(e, io):
            k = nuts_cfg()
            r.ok(e, r.lib.dll.ahmc_sample_from(e._ctx, C.byref(k), 3, n, 0, 0, io[SFO]))
            r.ok(e, r.lib.dll.ahmc_sync(e._ctx))
            return {"theta_end": e.theta()}

        first = np.arange(D * N * n) < 2 * D * N
        r.probe(mk, call, outs={SFO: Out(dtype, D * N * n, where, meaningful=~first, untouched=first)})


for _D in sorted(GEOM):
    for _dt in (F64, F32):
        add(f"sample-nuts-D{_D}-{np.dtype(_dt).name}", c_sample_nuts, [SO], D=_D, dtype=_dt)
for _D in (10, 300, 600):   # chains that share a wave, a whole wave per chain, several waves per chain
    add(f"sample-hmc-endpoint-D{_D}", c_sample_hmc, [SO], D=_D, sampler=capi.TS_ENDPOINT)
    add(f"sample-hmc-multinomial-D{_D}", c_sample_hmc, [SO], D=_D, sampler=capi.TS_MULTINOMIAL)
for _D in (5, 64, 100):
    add(f"sample-dense-D{_D}", c_sample_dense, [SO], D=_D)
add("sample-epoch-float64", c_sample_epoch, [SO], dtype=F64)
add("sample-epoch-float32", c_sample_epoch, [SO], dtype=F32)
add("sample-wide-D4097", c_sample_wide, [SO])
add("sample-glm", c_sample_glm, [SO], oracle=False)
for _w in ("device", "host", "pinned"):
    add(f"sample-split-{_w}", c_sample_split, [SO], where=_w)
    add(f"sample-from-{_w}", c_sample_from, [SFO], where=_w)


# ------------------------------------------------------------------------------------------------------------------------------
# diagnostics on draws: ahmc_ess, ahmc_diag_summary, ahmc_diag_rank_normalize
# ------------------------------------------------------------------------------------------------------------------------------
KDN = [(4, 1, 1), (33, 2, 5), (64, 3, 67)]


def draws_of(K, D, N, dtype):
    return np.random.default_rng(K + D + N).normal(size=K * D * N).astype(dtype)


def c_ess(r, K, D, N):
    for dtype in (F64, F32):
        for where in ("device", "host"):
            def call(e, io):
                r.ok(e, r.lib.dll.ahmc_ess(e._ctx, io["ahmc_ess.draws"], K, io["ahmc_ess.out"]))
            r.probe(lambda: engine(r.lib, D, N, dtype, metric="unit"), call, ins={"ahmc_ess.draws": In(draws_of(K, D, N, dtype), "device")},
                    outs={"ahmc_ess.out": Out(dtype, D * N, where)})


def c_diag(r, K, D, N):
    """the (d, c, k) layout of the summary's and the rank normalisation's kernels; AHMC_DIAG_WORKSPACE_MB=1 makes the summary take
    its dimensions in batches where the workspace of all D does not fit"""
    s_d, s_o, n_d, n_o = "ahmc_diag_summary.draws", "ahmc_diag_summary.out", "ahmc_diag_rank_normalize.draws", "ahmc_diag_rank_normalize.out"
    for dtype in (F64, F32):
        mk = lambda: engine(r.lib, D, N, dtype, metric="unit")  # noqa: E731
        x = draws_of(K, D, N, dtype)
        for where in ("device", "host"):
            for mb in (None, "1"):
                if mb is None:
                    r.mp.delenv("AHMC_DIAG_WORKSPACE_MB", raising=False)
                else:
                    r.mp.setenv("AHMC_DIAG_WORKSPACE_MB", mb)

                def call(e, io):
                    r.ok(e, r.lib.dll.ahmc_diag_summary(e._ctx, io[s_d], K, 0, io[s_o]))
                r.probe(mk, call, ins={s_d: In(x, "device")}, outs={s_o: Out(F64, 9 * D, where)})
            r.mp.delenv("AHMC_DIAG_WORKSPACE_MB", raising=False)
            for folded in (0, 1):
                def call(e, io):
                    r.ok(e, r.lib.dll.ahmc_diag_rank_normalize(e._ctx, io[n_d], K, D - 1, folded, io[n_o]))
                r.probe(mk, call, ins={n_d: In(x, "device")}, outs={n_o: Out(F64, K * N, where)})


_DIAG = ["ahmc_diag_summary.draws", "ahmc_diag_summary.out", "ahmc_diag_rank_normalize.draws", "ahmc_diag_rank_normalize.out"]
# With AHMC_DIAG_WORKSPACE_MB=1 the summary of (K, D, N) = (64, 3, 67) still takes its three dimensions at once: the plan of
# csrc/ahmc_diag_host.hpp needs about 0.30 MiB per dimension there (S = 2·N·⌊K/2⌋ = 4288 values, 48 + 2·8 bytes each, plus the
# autocovariance slabs).  Two more dimensions cross it: D = 5 runs as a batch of three dimensions and one of two.
add("diag-K64-D5-N67-batched", c_diag, _DIAG, oracle=False, K=64, D=5, N=67)
for _K, _D, _N in KDN:
    add(f"ess-K{_K}-D{_D}-N{_N}", c_ess, ["ahmc_ess.draws", "ahmc_ess.out"], K=_K, D=_D, N=_N)
    add(f"diag-K{_K}-D{_D}-N{_N}", c_diag, ["ahmc_diag_summary.draws", "ahmc_diag_summary.out", "ahmc_diag_rank_normalize.draws",
                                           "ahmc_diag_rank_normalize.out"], oracle=False, K=_K, D=_D, N=_N)


# ------------------------------------------------------------------------------------------------------------------------------
# getters
# ------------------------------------------------------------------------------------------------------------------------------
def sampled(r, D, N, dtype, adaptor="stepsize", comm=False, metric="diag_chain"):
    """a context after a short NUTS run with adaptation"""
    e = engine(r.lib, D, N, dtype, adaptor=adaptor, metric=metric)
    k = nuts_cfg()
    e._call("ahmc_sample", C.byref(k), 6, 4, 0, None)
    if comm:
        e.comm_init(e.comm_unique_id(), 1, 0)
    return e


class Borrowed:
    """a context the probe must not close"""

    def __init__(self, e):
        self._ctx = e._ctx


def c_ebfmi_gather(r, comm):
    D, N = 3, 5
    for dtype in (F64, F32):
        mk = lambda: sampled(r, D, N, dtype, comm=comm)  # noqa: E731
        shared = None
        if comm:   # setting up a communicator takes most of a second: one context serves every run (none of the calls probed here changes it)
            shared = mk()
            mk = lambda: Borrowed(shared)  # noqa: E731
        for where in ("device", "host"):
            r.probe(mk, lambda e, io: r.ok(e, r.lib.dll.ahmc_ebfmi(e._ctx, io["ahmc_ebfmi.out"])), outs={"ahmc_ebfmi.out": Out(dtype, N, where)})
        r.probe(mk, lambda e, io: r.ok(e, r.lib.dll.ahmc_gather_state(e._ctx, io["ahmc_gather_state.theta_all"])),
                outs={"ahmc_gather_state.theta_all": Out(dtype, D * N, "device")})

        def call(e, io):
            n = [C.c_int64() for _ in range(3)]
            r.ok(e, r.lib.dll.ahmc_gather_moments(e._ctx, io["ahmc_gather_moments.mean"], io["ahmc_gather_moments.var"], C.byref(n[0]), C.byref(n[1]), C.byref(n[2])))
            return {"counts": np.array([x.value for x in n])}
        r.probe(mk, call, outs={"ahmc_gather_moments.mean": Out(F64, D, "host"), "ahmc_gather_moments.var": Out(F64, D, "host")})
        if shared is not None:
            shared.close()


_EG = ["ahmc_ebfmi.out", "ahmc_gather_state.theta_all", "ahmc_gather_moments.mean", "ahmc_gather_moments.var"]
add("ebfmi-gather-no-comm", c_ebfmi_gather, _EG, comm=False)
add("ebfmi-gather-one-rank-comm", c_ebfmi_gather, _EG, comm=True)


def c_getters(r, where):
    D, N = 3, 5
    pp = [f"ahmc_get_phasepoint.{n}" for n in ("theta", "r", "lp", "grad", "lk")]
    acc = [f"ahmc_get_accum.{n}" for n in ("sum_theta", "sumsq_theta")]
    acs = [f"ahmc_get_accum_state.{n}" for n in ("n_steps", "n_divergent", "sum_theta", "sumsq_theta", "energy_sums")]
    for dtype in (F64, F32):
        mk = lambda: sampled(r, D, N, dtype)  # noqa: E731
        dll = r.lib.dll
        r.probe(mk, lambda e, io: r.ok(e, dll.ahmc_get_phasepoint(e._ctx, *[io[k] for k in pp])),
                outs={k: Out(dtype, n, where) for k, n in zip(pp, (D * N, D * N, N, D * N, N))})
        for name, (fid, is_int) in capi.STAT_FIELDS.items():
            r.probe(mk, lambda e, io: r.ok(e, dll.ahmc_get_stat(e._ctx, fid, io["ahmc_get_stat.out"])),
                    outs={"ahmc_get_stat.out": Out(np.int32 if is_int else dtype, N, where)})
        r.probe(mk, lambda e, io: r.ok(e, dll.ahmc_get_metric(e._ctx, io["ahmc_get_metric.Minv_out"], D * N)), outs={"ahmc_get_metric.Minv_out": Out(dtype, D * N, where)})
        r.probe(mk, lambda e, io: r.ok(e, dll.ahmc_get_stepsize(e._ctx, io["ahmc_get_stepsize.eps_out"])), outs={"ahmc_get_stepsize.eps_out": Out(dtype, N, where)})

        def call(e, io):
            n = [C.c_int64() for _ in range(3)]
            r.ok(e, dll.ahmc_get_accum(e._ctx, C.byref(n[0]), C.byref(n[1]), C.byref(n[2]), *[io[k] for k in acc]))
            return {"counts": np.array([x.value for x in n])}
        r.probe(mk, call, outs={k: Out(dtype, D * N, where) for k in acc})

        def call(e, io):
            n = C.c_int64()
            r.ok(e, dll.ahmc_get_accum_state(e._ctx, C.byref(n), *[io[k] for k in acs]))
            return {"n_transitions": np.array(n.value)}
        r.probe(mk, call, outs={k: Out(t, n, where) for k, t, n in zip(acs, (np.int64, np.int64, dtype, dtype, dtype), (N, N, D * N, D * N, 5 * N))})
    # the metric's other shapes: one shared (D,) M⁻¹, a dense (D, D)
    for metric, n in (("diag", D), ("dense", D * D)):
        r.probe(lambda: engine(r.lib, D, N, F64, metric=metric), lambda e, io: r.ok(e, r.lib.dll.ahmc_get_metric(e._ctx, io["ahmc_get_metric.Minv_out"], n)),
                outs={"ahmc_get_metric.Minv_out": Out(F64, n, where)})


_GET = ([f"ahmc_get_phasepoint.{n}" for n in ("theta", "r", "lp", "grad", "lk")] + ["ahmc_get_stat.out", "ahmc_get_metric.Minv_out", "ahmc_get_stepsize.eps_out"] +
        [f"ahmc_get_accum.{n}" for n in ("sum_theta", "sumsq_theta")] + [f"ahmc_get_accum_state.{n}" for n in ("n_steps", "n_divergent", "sum_theta", "sumsq_theta", "energy_sums")])
add("getters-device", c_getters, _GET, where="device")
add("getters-host", c_getters, _GET, where="host")


def adaptor_header(r, e):
    st = capi.AdaptorState()
    r.ok(e, r.lib.dll.ahmc_get_adaptor_state(e._ctx, C.byref(st), None, None))
    return st


def c_adaptor_state(r, estimator, where):
    D, N = 3, 5
    gda, gwv, sda, swv = "ahmc_get_adaptor_state.da", "ahmc_get_adaptor_state.welford", "ahmc_set_adaptor_state.da", "ahmc_set_adaptor_state.welford"
    for dtype in (F64, F32):
        mk = lambda: sampled(r, D, N, dtype, adaptor=estimator)  # noqa: E731
        donor = mk()
        st = adaptor_header(r, donor)
        nw = st.n_welford
        assert st.has_da == 1 and nw == (3 if estimator == "welford" else 5)
        da, wv = np.empty(5 * N, dtype=dtype), np.empty(nw * D * N, dtype=dtype)
        r.ok(donor, r.lib.dll.ahmc_get_adaptor_state(donor._ctx, C.byref(st), capi.as_ptr(da), capi.as_ptr(wv)))
        donor.close()

        def call(e, io):
            s = capi.AdaptorState()
            r.ok(e, r.lib.dll.ahmc_get_adaptor_state(e._ctx, C.byref(s), io[gda], io[gwv]))
            return {"header": np.frombuffer(bytes(s), dtype=np.uint8)}
        r.probe(mk, call, outs={gda: Out(dtype, 5 * N, where), gwv: Out(dtype, nw * D * N, where)})

        def call(e, io):
            s = capi.AdaptorState.from_buffer_copy(st)
            r.ok(e, r.lib.dll.ahmc_set_adaptor_state(e._ctx, C.byref(s), io[sda], io[swv]))
            k = nuts_cfg()
            e._call("ahmc_sample_from", C.byref(k), 7, 9, 9, 0, None)   # the adaptor goes on: its state is in use
            out = observe(e, transition=False)
            out["metric"] = e.get_metric()
            return out
        r.probe(lambda: engine(r.lib, D, N, dtype, adaptor=estimator), call, ins={sda: In(da, where), swv: In(wv, where)})


_AS = ["ahmc_get_adaptor_state.da", "ahmc_get_adaptor_state.welford", "ahmc_set_adaptor_state.da", "ahmc_set_adaptor_state.welford"]
for _e in ("welford", "nutpie"):
    for _w in ("device", "host"):
        add(f"adaptor-state-{_e}-{_w}", c_adaptor_state, _AS, estimator=_e, where=_w)


def c_rank_update(r, where):
    D, N, k = 5, 5, 2
    names = ("A", "B", "Dm")
    for dtype in (F64, F32):
        rs = np.random.default_rng(2)
        Av, Bv, Dv = (0.5 + rs.random(D)).astype(dtype), (0.3 * rs.normal(size=D * k)).astype(dtype), np.asfortranarray(np.diag([0.7, 0.4])).ravel().astype(dtype)

        def mk():
            e = engine(r.lib, D, N, dtype, metric="unit")
            e._call("ahmc_set_metric_rank_update", capi.as_ptr(Av), capi.as_ptr(Bv), capi.as_ptr(Dv), k)
            return e

        def call(e, io):
            kk = C.c_int64()
            r.ok(e, r.lib.dll.ahmc_get_metric_rank_update(e._ctx, *[io[f"ahmc_get_metric_rank_update.{n}"] for n in names], C.byref(kk)))
            return {"k": np.array(kk.value)}
        r.probe(mk, call, outs={f"ahmc_get_metric_rank_update.{n}": Out(dtype, m, where) for n, m in zip(names, (D, D * k, k * k))})

        def call(e, io):
            r.ok(e, r.lib.dll.ahmc_set_metric_rank_update(e._ctx, *[io[f"ahmc_set_metric_rank_update.{n}"] for n in names], k))
            e.refresh()
            return observe(e)
        r.probe(lambda: engine(r.lib, D, N, dtype, metric="unit"), call,
                ins={f"ahmc_set_metric_rank_update.{n}": In(v, where) for n, v in zip(names, (Av, Bv, Dv))})


add("rank-update-device", c_rank_update, [f"ahmc_{g}et_metric_rank_update.{n}" for g in "gs" for n in ("A", "B", "Dm")], oracle=False, where="device")
add("rank-update-host", c_rank_update, [f"ahmc_{g}et_metric_rank_update.{n}" for g in "gs" for n in ("A", "B", "Dm")], oracle=False, where="host")


def c_lowrank(r, where):
    D, N, k, over = 6, 5, 2, 2
    names = ("mu", "m2", "Z", "s0", "Omega")

    def mk(run=True):
        e = engine(r.lib, D, N, F64, metric="unit")
        r.ok(e, r.lib.dll.ahmc_lowrank_adaptor_init(e._ctx, capi.ADAPT_STAN, 0.8, 2, 2, 3, k, over, 99))
        if run:
            kc = nuts_cfg()
            e._call("ahmc_sample", C.byref(kc), 4, 12, 0, None)
        return e

    donor = mk()
    st = capi.LowRankState()
    r.ok(donor, r.lib.dll.ahmc_lowrank_get_state(donor._ctx, C.byref(st), None, None, None, None, None))
    ell = int(st.ell)
    sizes = (D, D, D * ell, D, D * ell)
    vals = [np.empty(n) for n in sizes]
    r.ok(donor, r.lib.dll.ahmc_lowrank_get_state(donor._ctx, C.byref(st), *[v.ctypes.data_as(C.c_void_p) for v in vals]))
    donor.close()

    def call(e, io):
        s = capi.LowRankState()
        r.ok(e, r.lib.dll.ahmc_lowrank_get_state(e._ctx, C.byref(s), *[io[f"ahmc_lowrank_get_state.{n}"] for n in names]))
        return {"header": np.frombuffer(bytes(s), dtype=np.uint8)}
    r.probe(mk, call, outs={f"ahmc_lowrank_get_state.{n}": Out(F64, m, where) for n, m in zip(names, sizes)})

    def call(e, io):
        s = capi.LowRankState.from_buffer_copy(st)
        r.ok(e, r.lib.dll.ahmc_lowrank_set_state(e._ctx, C.byref(s), *[io[f"ahmc_lowrank_set_state.{n}"] for n in names]))
        got = [np.empty(n) for n in sizes]
        r.ok(e, r.lib.dll.ahmc_lowrank_get_state(e._ctx, C.byref(s), *[v.ctypes.data_as(C.c_void_p) for v in got]))
        kc = nuts_cfg()
        e._call("ahmc_sample", C.byref(kc), 8, 12, 0, None)   # pushes into the restored window and fits it
        return {**{f"back_{n}": v for n, v in zip(names, got)}, "theta": e.theta()}
    r.probe(lambda: mk(run=False), call, ins={f"ahmc_lowrank_set_state.{n}": In(v, where) for n, v in zip(names, vals)})


_LR = [f"ahmc_lowrank_{g}et_state.{n}" for g in "gs" for n in ("mu", "m2", "Z", "s0", "Omega")]
add("lowrank-state-device", c_lowrank, _LR, oracle=False, where="device")
add("lowrank-state-host", c_lowrank, _LR, oracle=False, where="host")


# ------------------------------------------------------------------------------------------------------------------------------
# GLM targets (HIP engine only)
# ------------------------------------------------------------------------------------------------------------------------------
def glm_data(n_obs, P, dtype, seed=4):
    rs = np.random.default_rng(seed + n_obs)
    return {"X": rs.normal(size=n_obs * P).astype(dtype), "y": rs.normal(size=n_obs).astype(dtype), "offset": (0.1 * rs.normal(size=n_obs)).astype(dtype),
            "prior_prec": np.array([0.5] + [0.0] * (P - 1), dtype=dtype)}


def glm_observe(r, e, n_obs, dtype):
    """what the bound model computes: the phase point at a fixed θ and the pointwise predictor / log-likelihood"""
    rs = np.random.default_rng(12)
    e.set_position(np.asfortranarray(0.3 * rs.normal(size=(e.D, e.N))))
    out = observe(e)
    out["eta"], out["loglik"] = e.glm_pointwise()
    return out


GROUPS = dict(n=1, lo=[1], hi=[3], centered=[0], hyper=[1.5])


def c_glm_set_target(r, entry, n_obs, where):
    """X, y, offset, prior_prec of the four binding entry points, the group table and the factors' level arrays"""
    N, P = 5, 3
    GAUSS, SIGMA = capi.GLM_GAUSSIAN_IDENTITY, capi.GLM_GAUSSIAN_IDENTITY_SIGMA
    i32 = lambda v: np.array(v, dtype=np.int32)  # noqa: E731
    for dtype in (F64, F32):
        d = glm_data(n_obs, P, dtype)
        pre = f"ahmc_{entry}"
        ins = {f"{pre}.{k}": In(v, where) for k, v in d.items()}
        table = {}
        if entry != "set_target_glm":
            table = {"lo": i32(GROUPS["lo"]), "hi": i32(GROUPS["hi"]), "centered": i32(GROUPS["centered"]), "hyper_scale": np.array(GROUPS["hyper"])}
            ins.update({f"{pre}.{k}": In(v, "host") for k, v in table.items()})
        n_lev, lev = i32([2, 3]), None
        if entry == "glm_factor_set_target":
            rs = np.random.default_rng(n_obs)
            lev = np.concatenate([rs.integers(0, 2, n_obs), rs.integers(0, 3, n_obs)]).astype(np.int32)
            ins.update({f"{pre}.n_levels": In(n_lev, "host"), f"{pre}.levels": In(lev, "host")})
        D = {"set_target_glm": P, "hglm_set_target": P + 1, "glm_aux_set_target": P + 2, "glm_factor_set_target": P + 5 + 1 + 1}[entry]
        if entry == "glm_factor_set_target":   # prior_prec covers the P rows of the model: dense columns, then the levels
            ins[f"{pre}.prior_prec"] = In(np.array([0.5, 0, 0] + [1.0] * 5, dtype=dtype), where)

        def call(e, io):
            dll, p = r.lib.dll, lambda k: io[f"{pre}.{k}"]  # noqa: E731
            data = (p("X"), p("y"), p("offset"), p("prior_prec"))
            tab = tuple(C.cast(p(k), C.POINTER(C.c_int32)) for k in ("lo", "hi", "centered")) + (C.cast(p("hyper_scale"), C.POINTER(C.c_double)),) if table else ()
            if entry == "set_target_glm":
                r.ok(e, dll.ahmc_set_target_glm(e._ctx, GAUSS, n_obs, *data, 1.3))
            elif entry == "hglm_set_target":
                r.ok(e, dll.ahmc_hglm_set_target(e._ctx, GAUSS, n_obs, P, *data, 1.3, 1, *tab))
            elif entry == "glm_aux_set_target":
                r.ok(e, dll.ahmc_glm_aux_set_target(e._ctx, SIGMA, n_obs, P, *data, 1, *tab, 0.1, 0.9))
            else:
                r.ok(e, dll.ahmc_glm_factor_set_target(e._ctx, SIGMA, n_obs, P, *data, 1.0, 1, *tab, 2, C.cast(p("n_levels"), C.POINTER(C.c_int32)),
                                                       C.cast(p("levels"), C.POINTER(C.c_int32)), 1, 0.1, 0.9))
            return glm_observe(r, e, n_obs, dtype)
        r.probe(lambda: engine(r.lib, D, N, dtype, metric="unit", position=False), call, ins=ins)


_GLM_IN = ("X", "y", "offset", "prior_prec")
_TAB = ("lo", "hi", "centered", "hyper_scale")
for _n in (1, 70):
    for _w in ("device", "host"):
        add(f"glm-set-target-nobs{_n}-{_w}", c_glm_set_target, [f"ahmc_set_target_glm.{k}" for k in _GLM_IN], oracle=False, entry="set_target_glm", n_obs=_n, where=_w)
        add(f"hglm-set-target-nobs{_n}-{_w}", c_glm_set_target, [f"ahmc_hglm_set_target.{k}" for k in _GLM_IN + _TAB], oracle=False, entry="hglm_set_target", n_obs=_n, where=_w)
        add(f"glm-aux-set-target-nobs{_n}-{_w}", c_glm_set_target, [f"ahmc_glm_aux_set_target.{k}" for k in _GLM_IN + _TAB], oracle=False, entry="glm_aux_set_target",
            n_obs=_n, where=_w)
        add(f"glm-factor-set-target-nobs{_n}-{_w}", c_glm_set_target, [f"ahmc_glm_factor_set_target.{k}" for k in _GLM_IN + _TAB + ("n_levels", "levels")], oracle=False,
            entry="glm_factor_set_target", n_obs=_n, where=_w)


def bound_glm(r, n_obs, dtype, N=5):
    """a context with the factor model bound: coefficient groups, factors and a sampled dispersion, so that every post-processing entry
    point answers.  P_x = 3, two factors of 2 and 3 levels: P = 8, one group, s last: D = 10."""
    rs = np.random.default_rng(n_obs)
    X = rs.normal(size=(n_obs, 3))
    facs = [A.Factor(rs.integers(0, 2, n_obs), 2), A.Factor(rs.integers(0, 3, n_obs), 3)]
    t = A.HierGLMTarget(X, rs.normal(size=n_obs), [A.CoefGroup(1, 3, False, 1.5)], family="gaussian_identity_sigma", aux_prior=(0.1, 0.9), factors=facs)
    e = engine(r.lib, t.D, N, dtype, metric="unit", target=t)
    return e


def c_glm_post(r, n_obs, where):
    """n_cols and the column stride of ahmc_hglm_coefficients and ahmc_glm_dispersion; (n_obs, N) of ahmc_glm_pointwise; the host tables of
    the get_target calls"""
    N, D, P, G = 5, 10, 8, 1
    for dtype in (F64, F32):
        mk = lambda: bound_glm(r, n_obs, dtype)  # noqa: E731
        dll = r.lib.dll
        r.probe(mk, lambda e, io: r.ok(e, dll.ahmc_glm_pointwise(e._ctx, io["ahmc_glm_pointwise.eta_out"], io["ahmc_glm_pointwise.loglik_out"])),
                outs={"ahmc_glm_pointwise.eta_out": Out(dtype, n_obs * N, where), "ahmc_glm_pointwise.loglik_out": Out(dtype, n_obs * N, where)})
        for n_cols in (1, N, 3 * N):
            th = (0.4 * np.random.default_rng(n_cols).normal(size=D * n_cols)).astype(dtype)
            for w_in in ("device", "host"):
                r.probe(mk, lambda e, io: r.ok(e, dll.ahmc_glm_dispersion(e._ctx, io["ahmc_glm_dispersion.theta"], n_cols, io["ahmc_glm_dispersion.out"])),
                        ins={"ahmc_glm_dispersion.theta": In(th, w_in)}, outs={"ahmc_glm_dispersion.out": Out(dtype, n_cols, where)})
                r.probe(mk, lambda e, io: r.ok(e, dll.ahmc_hglm_coefficients(e._ctx, io["ahmc_hglm_coefficients.theta"], n_cols, io["ahmc_hglm_coefficients.beta_out"],
                                                                            io["ahmc_hglm_coefficients.tau_out"])),
                        ins={"ahmc_hglm_coefficients.theta": In(th, w_in)},
                        outs={"ahmc_hglm_coefficients.beta_out": Out(dtype, P * n_cols, where), "ahmc_hglm_coefficients.tau_out": Out(dtype, G * n_cols, where)})
    # the host tables: AHMC_HGLM_MAX_GROUPS / AHMC_GLM_FACTOR_MAX entries suffice, the bound model's entries are meaningful
    MG, MF = capi.HGLM_MAX_GROUPS, capi.GLM_FACTOR_MAX
    pi, pd = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    tab = [f"ahmc_hglm_get_target.{k}" for k in _TAB]

    def call(e, io):
        nc, ng = C.c_int64(), C.c_int32()
        r.ok(e, r.lib.dll.ahmc_hglm_get_target(e._ctx, C.byref(nc), C.byref(ng), *[C.cast(io[k], pi) for k in tab[:3]], C.cast(io[tab[3]], pd)))
        return {"n": np.array([nc.value, ng.value])}
    r.probe(lambda: bound_glm(r, n_obs, F64), call, outs={k: Out(np.float64 if k.endswith("hyper_scale") else np.int32, MG, "host", meaningful=np.arange(MG) < G) for k in tab})

    def call(e, io):
        nc, nf = C.c_int64(), C.c_int32()
        r.ok(e, r.lib.dll.ahmc_glm_factor_get_target(e._ctx, C.byref(nc), C.byref(nf), C.cast(io["ahmc_glm_factor_get_target.n_levels"], pi)))
        return {"n": np.array([nc.value, nf.value])}
    r.probe(lambda: bound_glm(r, n_obs, F64), call, outs={"ahmc_glm_factor_get_target.n_levels": Out(np.int32, MF, "host", meaningful=np.arange(MF) < 2)})


_GP = (["ahmc_glm_pointwise.eta_out", "ahmc_glm_pointwise.loglik_out", "ahmc_glm_dispersion.theta", "ahmc_glm_dispersion.out", "ahmc_hglm_coefficients.theta",
        "ahmc_hglm_coefficients.beta_out", "ahmc_hglm_coefficients.tau_out", "ahmc_glm_factor_get_target.n_levels"] + [f"ahmc_hglm_get_target.{k}" for k in _TAB])
for _n in (1, 70):
    for _w in ("device", "host"):
        add(f"glm-post-nobs{_n}-{_w}", c_glm_post, _GP, oracle=False, n_obs=_n, where=_w)


# ------------------------------------------------------------------------------------------------------------------------------
# ask / tell and the split step
# ------------------------------------------------------------------------------------------------------------------------------
def c_ext(r, where):
    """a two-transition ask / tell NUTS run, D = 3, N = 5: ahmc_ext_pending's chains_out (a set: its order is unspecified) and the listed
    columns of theta_out; ahmc_ext_advance reads the pending chains' entries of lp / grad_neg and ignores the others, which are poisoned"""
    D, N = 3, 5
    ch, th, lp, gn = "ahmc_ext_pending.chains_out", "ahmc_ext_pending.theta_out", "ahmc_ext_advance.lp", "ahmc_ext_advance.grad_neg"
    for dtype in (F64, F32):
        def mk():
            e = engine(r.lib, D, N, dtype, target="external", metric="diag")
            k = nuts_cfg(3)
            e._call("ahmc_ext_begin", C.byref(k), 2)
            return e

        def call(e, io):
            log, trips = [], 0
            while True:
                n = C.c_int64()
                io.refill(ch)
                io.refill(th)
                r.ok(e, r.lib.dll.ahmc_ext_pending(e._ctx, C.byref(n), C.cast(io[ch], C.POINTER(C.c_int32)), io[th]))
                r.ok(e, r.lib.dll.ahmc_sync(e._ctx))
                if n.value == 0:
                    break
                idx = np.sort(io.read(ch)[:n.value])
                assert len(set(idx.tolist())) == n.value and idx.min() >= 0 and idx.max() < N, idx
                theta = io.read(th).reshape(N, D)
                log += [np.array([n.value]), idx.astype(np.float64), theta[idx].ravel().astype(np.float64)]
                pending = np.zeros(N, dtype=bool)
                pending[idx] = True
                lpv = np.where(pending, -0.5 * np.sum(np.square(theta.astype(np.float64)), axis=1), 0.0)
                gv = np.where(pending[:, None], theta, 0.0)
                io.write(lp, lpv.astype(dtype), ignored=~pending)
                io.write(gn, gv.astype(dtype), ignored=np.repeat(~pending, D))
                r.ok(e, r.lib.dll.ahmc_ext_advance(e._ctx, io[lp], io[gn]))
                trips += 1
                assert trips < 200
            out = observe(e, transition=False)
            out["log"] = np.concatenate(log)
            return out

        none = np.zeros(N, dtype=bool)
        r.probe(mk, call, ins={lp: In(np.zeros(N, dtype=dtype), where), gn: In(np.zeros(D * N, dtype=dtype), where)},
                outs={ch: Out(np.int32, N, "host", meaningful=none), th: Out(dtype, D * N, where, meaningful=np.repeat(none, D))})


_EXT = ["ahmc_ext_pending.chains_out", "ahmc_ext_pending.theta_out", "ahmc_ext_advance.lp", "ahmc_ext_advance.grad_neg"]
add("ask-tell-device", c_ext, _EXT, where="device")
add("ask-tell-host", c_ext, _EXT, where="host")


def c_lf_post(r, where):
    D, N = 3, 5
    for dtype in (F64, F32):
        rs = np.random.default_rng(6)
        lpv, gv = rs.normal(size=N).astype(dtype), rs.normal(size=D * N).astype(dtype)

        def mk():
            e = engine(r.lib, D, N, dtype, target="external", metric="diag")
            e._call("ahmc_lf_pre", 1, 1, 1)
            return e

        def call(e, io):
            r.ok(e, r.lib.dll.ahmc_lf_post(e._ctx, 1, 1, 1, io["ahmc_lf_post.lp"], io["ahmc_lf_post.grad_neg"]))
            return observe(e, transition=False)
        r.probe(mk, call, ins={"ahmc_lf_post.lp": In(lpv, where), "ahmc_lf_post.grad_neg": In(gv, where)})


add("lf-post-device", c_lf_post, ["ahmc_lf_post.lp", "ahmc_lf_post.grad_neg"], where="device")
add("lf-post-host", c_lf_post, ["ahmc_lf_post.lp", "ahmc_lf_post.grad_neg"], where="host")


# ------------------------------------------------------------------------------------------------------------------------------
# setters: copy and ingest paths (R and C)
# ------------------------------------------------------------------------------------------------------------------------------
def c_setters(r, where):
    D, N = 3, 5
    dll = r.lib.dll
    for dtype in (F64, F32):
        rs = np.random.default_rng(8)
        v = lambda *s: rs.normal(size=int(np.prod(s))).astype(dtype)  # noqa: E731
        pos = lambda *s: (0.5 + rs.random(int(np.prod(s)))).astype(dtype)  # noqa: E731
        mk = lambda **kw: (lambda: engine(r.lib, D, N, dtype, **kw))  # noqa: E731

        th, rr = v(D, N), v(D, N)
        r.probe(mk(), lambda e, io: (r.ok(e, dll.ahmc_set_position(e._ctx, io["ahmc_set_position.theta"], io["ahmc_set_position.r"])), observe(e))[1],
                ins={"ahmc_set_position.theta": In(th, where), "ahmc_set_position.r": In(rr, where)})
        pp = {f"ahmc_set_phasepoint.{k}": In(x, where) for k, x in zip(("theta", "r", "lp", "grad"), (th, rr, v(N), v(D, N)))}
        r.probe(mk(target="external", metric="diag"), lambda e, io: (r.ok(e, dll.ahmc_set_phasepoint(e._ctx, *[io[k] for k in pp])), observe(e, transition=False))[1], ins=pp)

        for kind, n in ((capi.METRIC_DIAG, D), (capi.METRIC_DIAG, D * N), (capi.METRIC_DENSE, D * D)):
            M = pos(n) if kind == capi.METRIC_DIAG else spd(rs, D).ravel().astype(dtype)

            def call(e, io):
                r.ok(e, dll.ahmc_set_metric(e._ctx, kind, io["ahmc_set_metric.Minv"], n))
                e.refresh()
                return observe(e)
            r.probe(mk(), call, ins={"ahmc_set_metric.Minv": In(M, where)})
        for n in (1, N):
            r.probe(mk(), lambda e, io: (r.ok(e, dll.ahmc_set_stepsize(e._ctx, io["ahmc_set_stepsize.eps"], n)), observe(e))[1], ins={"ahmc_set_stepsize.eps": In(0.1 * pos(n), where)})
        ms = np.concatenate([v(D), pos(D)])
        r.probe(mk(position=False), lambda e, io: (r.ok(e, dll.ahmc_set_target(e._ctx, capi.TARGET_DIAG_GAUSS, io["ahmc_set_target.params"], 2 * D)),
                                                   e.set_position(th.reshape(N, D).T, rr.reshape(N, D).T), observe(e))[2], ins={"ahmc_set_target.params": In(ms, where)})

        def after_adapt(e):
            out = observe(e)
            out["metric"] = e.get_metric()
            return out
        al = (0.2 + 0.6 * rs.random(N)).astype(dtype)
        r.probe(mk(adaptor="welford"), lambda e, io: (r.ok(e, dll.ahmc_adapt(e._ctx, 3, 9, io["ahmc_adapt.theta"], io["ahmc_adapt.alpha"])), after_adapt(e))[1],
                ins={"ahmc_adapt.theta": In(th, where), "ahmc_adapt.alpha": In(al, where)})
        ap = {f"ahmc_adapt_point.{k}": In(x, where) for k, x in zip(("theta", "grad", "alpha"), (th, v(D, N), al))}
        r.probe(mk(adaptor="nutpie"), lambda e, io: (r.ok(e, dll.ahmc_adapt_point(e._ctx, 3, 9, *[io[k] for k in ap])), after_adapt(e))[1], ins=ap)

        acs = {f"ahmc_set_accum_state.{k}": In(x, where) for k, x in zip(("n_steps", "n_divergent", "sum_theta", "sumsq_theta", "energy_sums"),
                                                                         (rs.integers(1, 50, N).astype(np.int64), rs.integers(0, 3, N).astype(np.int64), v(D, N), pos(D, N), v(5, N)))}

        def call(e, io):
            r.ok(e, dll.ahmc_set_accum_state(e._ctx, 7, *[io[k] for k in acs]))
            a = e.accum()
            back = {"n_steps": np.empty(N, dtype=np.int64), "n_div": np.empty(N, dtype=np.int64), "es": np.empty(5 * N, dtype=dtype)}
            n = C.c_int64()
            r.ok(e, dll.ahmc_get_accum_state(e._ctx, C.byref(n), capi.as_ptr(back["n_steps"]), capi.as_ptr(back["n_div"]), None, None, capi.as_ptr(back["es"])))
            return {"counts": np.array([a["total_n_steps"], a["n_transitions"], a["n_divergent"], n.value]), "s1": a["sum_theta"], "s2": a["sumsq_theta"], "ebfmi": e.ebfmi(), **back}
        r.probe(mk(), call, ins=acs)


_SET = (["ahmc_set_position.theta", "ahmc_set_position.r"] + [f"ahmc_set_phasepoint.{k}" for k in ("theta", "r", "lp", "grad")] +
        ["ahmc_set_metric.Minv", "ahmc_set_stepsize.eps", "ahmc_set_target.params", "ahmc_adapt.theta", "ahmc_adapt.alpha"] +
        [f"ahmc_adapt_point.{k}" for k in ("theta", "grad", "alpha")] + [f"ahmc_set_accum_state.{k}" for k in ("n_steps", "n_divergent", "sum_theta", "sumsq_theta", "energy_sums")])
add("setters-device", c_setters, _SET, where="device")
add("setters-host", c_setters, _SET, where="host")


def c_plugin_params(r):
    """the parameters of a target plugin are copied to device memory at the call (tests/user_targets/banana.hpp reads two); the plugin
    is the one tests/test_user_targets.py builds for D = 10, so the object cache serves one of the two"""
    from ahmc_amd.build import build_target_plugin

    D, N = 10, 5
    for where in ("device", "host"):
        def mk():
            e = engine(r.lib, D, N, F64, position=False)
            e._so = build_target_plugin(os.path.join(ROOT, "tests", "user_targets", "banana.hpp"), F64, e.info("group_lanes"), e.info("elems_per_lane"))
            return e

        def call(e, io):
            r.ok(e, r.lib.dll.ahmc_set_target_plugin(e._ctx, e._so.encode(), io["ahmc_set_target_plugin.params"], 2))
            e.set_position(np.asfortranarray(0.5 * np.random.default_rng(1).normal(size=(D, N))))
            return observe(e)
        r.probe(mk, call, ins={"ahmc_set_target_plugin.params": In(np.array([0.5, 0.05]), where)})


add("plugin-params", c_plugin_params, ["ahmc_set_target_plugin.params"], oracle=False)


def c_stan_windows(r):
    """pure host logic: up to `cap` split points, *n_splits of them written"""
    def call(_, io):
        ws, we, ns = C.c_int64(), C.c_int64(), C.c_int32()
        r.ok(None, r.lib.dll.ahmc_stan_windows(9, 6, 15, 60, C.byref(ws), C.byref(we), C.cast(io["ahmc_stan_windows.splits"], C.POINTER(C.c_int64)), cap, C.byref(ns)))
        assert 0 < ns.value <= cap
        seen.append(ns.value)
        return {"n": np.array([ws.value, we.value, ns.value])}

    for cap in (2, 64):
        seen = []
        r.probe(lambda: None, call, outs={"ahmc_stan_windows.splits": Out(np.int64, cap, "host", meaningful=np.arange(cap) < 2)}, sync=False)
        assert set(seen) == {2}


add("stan-windows", c_stan_windows, ["ahmc_stan_windows.splits"])


# ------------------------------------------------------------------------------------------------------------------------------
# the gate
# ------------------------------------------------------------------------------------------------------------------------------
# pointer parameters that are no arrays of the caller's: (function or *, parameter) -> why
NOT_ARRAYS = {
    ("*", "ctx"): "the context",
    ("ahmc_create", "out"): "receives the opaque context handle",
    ("ahmc_create", "stream"): "opaque handle (hipStream_t)",
    ("ahmc_set_target_plugin", "plugin_so"): "C string",
    ("ahmc_set_target_kernel", "handle"): "opaque handle (hipFunction_t / symbol address)",
    ("ahmc_set_target_kernel", "user"): "opaque pointer handed through to the caller's kernel",
    ("ahmc_set_comm", "nccl_comm"): "opaque handle (ncclComm_t)",
    ("ahmc_comm_unique_id", "id_out"): "the 128-byte unique id",
    ("ahmc_comm_init", "id"): "the 128-byte unique id",
    ("*", "cfg"): "pointer to the ABI's struct ahmc_kernel_cfg",
    ("*", "state"): "pointer to the ABI's structs ahmc_adaptor_state / ahmc_lowrank_state",
    ("ahmc_stan_windows", "window_start"): "scalar out-parameter the host code writes",
    ("ahmc_stan_windows", "window_end"): "scalar out-parameter the host code writes",
    ("ahmc_stan_windows", "n_splits"): "scalar out-parameter the host code writes",
    ("ahmc_get_accum", "total_n_steps"): "scalar out-parameter the host code writes",
    ("ahmc_get_accum", "n_transitions"): "scalar out-parameter the host code writes",
    ("ahmc_get_accum", "n_divergent"): "scalar out-parameter the host code writes",
    ("ahmc_get_accum_state", "n_transitions"): "scalar out-parameter the host code writes",
    ("ahmc_ext_pending", "n_pending"): "scalar out-parameter the host code writes",
    ("ahmc_comm_info", "ranks_seen"): "scalar out-parameter the host code writes",
    ("ahmc_comm_info", "chains_total"): "scalar out-parameter the host code writes",
    ("ahmc_comm_info", "chains_min"): "scalar out-parameter the host code writes",
    ("ahmc_comm_info", "chains_max"): "scalar out-parameter the host code writes",
    ("ahmc_gather_moments", "n_draws"): "scalar out-parameter the host code writes",
    ("ahmc_gather_moments", "total_n_steps"): "scalar out-parameter the host code writes",
    ("ahmc_gather_moments", "n_divergent"): "scalar out-parameter the host code writes",
    ("ahmc_get_info", "out"): "scalar out-parameter the host code writes",
    ("ahmc_get_metric_rank_update", "k"): "scalar out-parameter the host code writes",
    ("ahmc_get_target_glm", "family"): "scalar out-parameter the host code writes",
    ("ahmc_get_target_glm", "n_obs"): "scalar out-parameter the host code writes",
    ("ahmc_get_target_glm", "scale"): "scalar out-parameter the host code writes",
    ("ahmc_hglm_get_target", "n_coef"): "scalar out-parameter the host code writes",
    ("ahmc_hglm_get_target", "n_groups"): "scalar out-parameter the host code writes",
    ("ahmc_glm_aux_get_target", "aux_loc"): "scalar out-parameter the host code writes",
    ("ahmc_glm_aux_get_target", "aux_scale"): "scalar out-parameter the host code writes",
    ("ahmc_glm_factor_get_target", "n_coef"): "scalar out-parameter the host code writes",
    ("ahmc_glm_factor_get_target", "n_factors"): "scalar out-parameter the host code writes",
}


def header_pointer_params():
    """{(function, parameter)} of every pointer parameter of every ahmc_* function the library exports, from the prototypes under
    include/ (the regex approach of tests/test_diag_summary.py: diag_header_prototypes).  The two ahmc_user_logdensity_* prototypes of
    ahmc_user_target_object.h carry AHMC_USER_DEVICE: device functions the USER defines and the engine calls — not entry points."""
    found = set()
    for path in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))):
        src = re.sub(r"/\*.*?\*/", "", open(path, encoding="utf-8").read(), flags=re.S)
        src = re.sub(r"//[^\n]*", "", src)
        for m in re.finditer(r"(\bAHMC_USER_DEVICE\s+)?\b(?:int32_t|void\s*\*|const\s+char\s*\*|double|float)\s*(ahmc_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
            if m.group(1):
                continue
            params = " ".join(m.group(3).split())
            for p in ([] if params in ("", "void") else params.split(",")):
                if "*" in p:
                    found.add((m.group(2), re.search(r"([A-Za-z_0-9]+)\s*$", p).group(1)))
    return found


def test_gate_every_array_argument_is_probed():
    params = header_pointer_params()
    assert len(params) > 120 and ("ahmc_sample", "samples_out") in params and ("ahmc_glm_factor_set_target", "levels") in params, len(params)
    probed = {tuple(k.split(".")) for c in CASES.values() for k in c.probes}
    assert probed <= params, f"cases name arguments the headers do not declare: {sorted(probed - params)}"
    excused = {p for p in params if ("*", p[1]) in NOT_ARRAYS or p in NOT_ARRAYS}
    stale = {k for k in NOT_ARRAYS if k[0] != "*" and k not in params} | {k for k in NOT_ARRAYS if k[0] == "*" and not any(p[1] == k[1] for p in params)}
    assert not stale, f"NOT_ARRAYS lists parameters no header declares: {sorted(stale)}"
    assert not (probed & excused), sorted(probed & excused)
    missing = params - probed - excused
    assert not missing, f"array arguments no case probes: {sorted(missing)}"
    # and the ctypes binding table knows every function the gate saw
    bound = set().union(*[set(getattr(capi, n)) for n in dir(capi) if n.endswith("SIGNATURES")])
    assert {f for f, _ in params} <= bound


# ------------------------------------------------------------------------------------------------------------------------------
# the harness itself: a numpy "callee" with planted defects
# ------------------------------------------------------------------------------------------------------------------------------
def np_at(ptr, dtype, n, offset=0):
    """n elements of dtype at address ptr + offset elements, as the callee sees the caller's memory"""
    dt = np.dtype(dtype)
    return np.frombuffer((C.c_char * (n * dt.itemsize)).from_address(ptr.value + offset * dt.itemsize), dtype=dt)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_harness_reports_planted_defects(dtype):
    """out[i] = 2·x[i] over n elements; each defect must be reported as the right property at the right offset, and the clean callee
    must pass"""
    n, item = 37, np.dtype(dtype).itemsize
    x = np.random.default_rng(0).normal(size=n).astype(dtype)

    def run(defect):
        def callee(_, io):
            xi, out = np_at(io["x"], dtype, n), np_at(io["out"], dtype, n)
            keep = out[5].copy()
            out[:] = 2 * xi
            if defect == "unwritten":
                out[5] = keep
            elif defect == "write_before":
                np_at(io["out"], np.uint8, item, -item)[:] ^= 0xFF      # (every byte of the element changes, whatever the band held there)
            elif defect == "write_after":
                np_at(io["out"], np.uint8, item, n * item)[:] ^= 0xFF
            elif defect == "read_past":
                out[n - 1] = 2 * xi[n - 1] + 0 * np_at(io["x"], dtype, 1, n)[0]     # (0·NaN = NaN, 0·1e30 = 0: the NaN pass must catch it)
            elif defect == "read_past_minmax":
                out[3] = max(2 * xi[3], np_at(io["x"], dtype, 2, n).max())          # (max ignores nothing at 1e30; fmax-like code hides NaN)
            elif defect == "scribble":
                np_at(io["x"], dtype, n)[7] = 0.0
        AU.probe(lambda: None, callee, {"x": In(x)}, {"out": Out(dtype, n)})

    run(None)
    for defect, prop, key, first, last in (("write_before", "W", "out", -item, -1), ("write_after", "W", "out", 1, item), ("read_past", "R", "out", n - 1, n - 1),
                                           ("read_past_minmax", "R", "out", 3, 3), ("unwritten", "F", "out", 5, 5), ("scribble", "C", "x", 7, 7)):
        with pytest.raises(AU.BoundsError) as ei:
            run(defect)
        err = ei.value
        assert (err.prop, err.key, err.first, err.last) == (prop, key, first, last), (defect, str(err))


def test_harness_arena_layout_and_patterns():
    for nbytes, band in ((8, 64 * 1024), (100_000, 100_000), (3 * 8 * 1024 * 1024, 8 * 1024 * 1024)):
        assert AU.band_bytes(nbytes) == band
        a = AU.Arena(nbytes, "host", "pattern")
        assert a.ptr % 256 == 0 and a.off >= band and a.image.size - a.off - nbytes >= band and a.band_damage() is None
    a = AU.Arena(64, "host", "pattern")
    a._np[a.off - 3000:a.off - 2000] = a._np[a.off - 3001:a.off - 2001].copy()      # a band shifted by one byte is damage
    assert a.band_damage() is not None
    for dtype in (F64, F32):
        for fill, test in (("nan", np.isnan), ("big", lambda v: np.abs(v) == np.dtype(dtype).type(1e30))):
            a = AU.Arena(24 * np.dtype(dtype).itemsize, "host", fill, dtype)
            item = np.dtype(dtype).itemsize
            front, back = a.image[a.off - 64 * item:a.off].view(dtype), a.image[a.off + a.nbytes:a.off + a.nbytes + 64 * item].view(dtype)
            assert test(front).all() and test(back).all()
            assert fill == "nan" or (np.sign(back[0]) != np.sign(back[1]))
        p = AU.prefill("payload", dtype, 100)
        assert np.isnan(p).all() and len(set(p.view(AU._int_view(dtype)).tolist())) == 100    # recognisable: compared on integer views
    assert not np.array_equal(AU.prefill("A", F64, 10), AU.prefill("B", F64, 10))


# ------------------------------------------------------------------------------------------------------------------------------
# the table against the CPU checker (host arenas) and against the HIP engine
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c for c in CASES if CASES[c].oracle])
def test_oracle_bounds(oracle, monkeypatch, cid):
    run_case(oracle, monkeypatch, cid)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_hip_bounds(hip, monkeypatch, cid):
    if hip.backend != "hip:gfx950" and not CASES[cid].oracle:
        return   # (a dry run on the CPU checker, which does not implement this entry point: nothing to shake out)
    run_case(hip, monkeypatch, cid)
