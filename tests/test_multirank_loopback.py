"""The engine's multi-rank paths (csrc/ahmc_multi_host.hpp: comm_probe, gather_moments, gather_state, the rank merge of the
pooled variance) with R = 2 and R = 3 ranks on ONE GPU: R worker processes share the device and meet through a stand-in for the
six RCCL entry points the engine resolves at run time (tests/host_ref/loopback_rccl.cpp, selected by AHMC_RCCL_LIB in the
workers only; tests/multirank_util.py starts them).  What this covers is everything the engine does AROUND its collectives:
buffer layout, kernels, merge order, refusals, ownership.  What it cannot cover: RCCL itself, xGMI, stream overlap, timing.

CPU part (`-m "not gpu"`): the stand-in's exchange logic in its host-buffer build, driven by a stand-alone program (plain and
under -fsanitize=address,undefined); the exact reference of the pooled estimate, validated on the oracle and on two planted
defects before it judges the engine.

The bound of the pooled estimate, per dimension (u = 2⁻⁵³, u_T the unit roundoff of the element type, γ_k = k·u / (1 − k·u)):

    |est̂ − est| ≤ γ_{n_dbl}(u) · (Σ_c M_c + n·Σ_c (μ_c − μ)² + 10⁻³) + u_T·|est|

`n_dbl` counts the double-precision roundings on one dimension's way through k_pool_var and k_pool_finish; it is read off the
kernels, not fitted.  With c = the longest of k_pool_var's four chain strides (⌈N/4⌉ for the largest partition; N for the
oracle, which sums the chains in sequence) and R partitions:
  * k_pool_var, the M of a partition: (μ_c − mean) 1, its square 1, c additions, the two levels of the four-stride sum 2,
    the product with n 1, the sum with Σ M_c 1 — and Σ M_c itself is c + 2 additions, the shorter path:            c + 6
  * k_pool_finish, each of the R − 1 merges: δ 1, δ² 1, n_a·n_b 1, / n_t 1, the product 1, two additions 2:      7·(R − 1)
  * the estimate: n + 5, n − 1, their product, the quotient, · M, 5 / (n + 5), · 10⁻³, the sum:                       8
  * the means: a partition's mean carries c + 3 roundings (c additions, 2 levels, the division by N), the running mean 4 more
    per merge (δ, n_b / n_t, the product, the sum): k_μ = c + 3 + 4·(R − 1) in all, each relative to values no larger than
    A = √(Σ_c μ_c² / N_tot).  Inside a partition the error of its mean enters M in second order only (Σ_c (μ_c − m) = 0 at the
    exact mean): one more rounding covers it.  In a merge it enters through 2·δ·ε·w with w = n_a·n_b / n_t ≤ n_tot and
    δ²·w ≤ M_tot:  2·|δ|·ε·w ≤ 2·√M_tot·√n_tot·γ_{k_μ}·A, and A² = μ² + Σ_c (μ_c − μ)² / N_tot ≤ 2·M_tot / n_tot for data whose
    pooled mean is no larger than its pooled standard deviation (n_tot·μ² ≤ M_tot — asserted of the exact values, and true of
    `injected_feed` by construction: mean = sd / 4), so ≤ 2·√2·γ_{k_μ}·M_tot per merge:                      3·(R − 1)·k_μ + 1
  n_dbl = c + 6 + 7·(R − 1) + 8 + 3·(R − 1)·(c + 3 + 4·(R − 1)) + 1.
The last term of the bound is the one rounding of the estimate to the element type.

Every error / bound and every bit-for-bit count is recorded in multirank_loopback_margins.json under $AHMC_TEST_OUT (default
test_out/); profiles/multirank_loopback_margins.json is the MI355X run.  On that run the three groups of workers (R = 1, 2, 3)
took 2.3 s, 2.2 s and 2.4 s of wall time, nearly all of it process start-up — no scenario needed more than 0.3 s in a worker (see
"worker_seconds" in the record) — and the eleven GPU test cases 10 s together, the exact reference in rationals included."""
import json
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import ahmc_amd as A
from ahmc_amd import _capi as capi
from ahmc_amd.shard import chain_shard

import multirank_util as MU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53
U_T = {np.dtype(np.float64): 2.0 ** -53, np.dtype(np.float32): 2.0 ** -24}
MARGINS = {}
WORKER_SECONDS = {}


# ------------------------------------------------------------------------------------------------------------------------
# the record
# ------------------------------------------------------------------------------------------------------------------------
def _dump_margins():
    out = os.environ.get("AHMC_TEST_OUT") or os.path.join(ROOT, "test_out")
    try:
        os.makedirs(out, exist_ok=True)
        worst = max([v["error_over_bound"] for v in MARGINS.values() if "error_over_bound" in v and not v.get("planted")], default=0.0)
        bits = {"compared": sum(v.get("bit_compared", 0) for v in MARGINS.values()), "mismatch": sum(v.get("bit_mismatch", 0) for v in MARGINS.values())}
        with open(os.path.join(out, "multirank_loopback_margins.json"), "w") as f:
            json.dump({"worst_error_over_bound": worst, "elements_compared_bit_for_bit": bits, "worker_seconds": WORKER_SECONDS,
                       "cases": dict(sorted(MARGINS.items()))}, f, indent=1)
    except OSError:
        pass


def record_bound(key, err, bound, planted=False):
    """largest err / bound of a comparison, kept under `key`; asserts it is ≤ 1 element by element (a `planted` defect is only
    recorded: its caller asserts the opposite)"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert np.isfinite(err).all() and (bound > 0).all(), f"{key}: non-finite result"
    frac = err / bound
    worst = float(frac.max())
    e = MARGINS.setdefault(key, {})
    e["error_over_bound"] = max(e.get("error_over_bound", 0.0), worst)
    if planted:
        e["planted"] = True
    _dump_margins()
    if worst > 1.0 and not planted:
        i = int(np.argmax(frac))
        raise AssertionError(f"{key}: error {err.ravel()[i]:.3e} is {worst:.3g} × its bound {bound.ravel()[i]:.3e} at element {i}")
    return worst


def record_bits(key, got, want):
    """elements of `got` that differ from `want` (any NaN equals any NaN), counted under `key`; asserts there are none"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (key, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind == "f":
        same = (got == want) | (np.isnan(got) & np.isnan(want))
    else:
        same = got == want
    e = MARGINS.setdefault(key, {})
    e["bit_compared"] = e.get("bit_compared", 0) + int(same.size)
    e["bit_mismatch"] = e.get("bit_mismatch", 0) + int((~same).sum())
    _dump_margins()
    if not same.all():
        bad = np.argwhere(~same)
        raise AssertionError(f"{key}: {len(bad)} of {same.size} elements differ; first at {tuple(bad[0])}: {got[tuple(bad[0])]!r} instead of "
                             f"{want[tuple(bad[0])]!r}")


# ------------------------------------------------------------------------------------------------------------------------
# the exact reference and its bound
# ------------------------------------------------------------------------------------------------------------------------
def welford_push_T(mu, M, x, n):
    """welford_push of csrc/ahmc_kernels.hpp in the element type, operation for operation (no contraction there)"""
    T = mu.dtype.type
    assert M.dtype == mu.dtype == x.dtype
    n = T(n)
    delta = x - mu
    return mu + delta / n, M + delta * delta * ((n - T(1)) / n)


def pooled_reference(mu, M, n, parts):
    """The pooled estimate in exact rational arithmetic from the per-chain Welford states (μ_c, M_c) (N_tot, D) AS STORED, each over
    n draws: per partition (off, cnt) of `parts` the mean, M = Σ M_c + n·Σ (μ_c − mean)² and the count, merged by Chan's update in
    the order given, then est = n_tot / ((n_tot + 5)(n_tot − 1))·M + 10⁻³·5 / (n_tot + 5).  The result does not depend on `parts`.
    Returns (est, M_tot, μ): three lists of D Fractions."""
    n = Fraction(int(n))
    est, Mt, mean = [], [], []
    for d in range(mu.shape[1]):
        fm = [Fraction(float(v)) for v in mu[:, d]]
        fM = [Fraction(float(v)) for v in M[:, d]]
        acc = None
        for off, cnt in parts:
            m_p = sum(fm[off:off + cnt]) / cnt
            M_p = sum(fM[off:off + cnt]) + n * sum((v - m_p) ** 2 for v in fm[off:off + cnt])
            n_p = n * cnt
            if acc is None:
                acc = (n_p, m_p, M_p)
            else:
                na, ma, Ma = acc
                delta, nt = m_p - ma, na + n_p
                acc = (nt, ma + delta * n_p / nt, Ma + M_p + delta * delta * na * n_p / nt)
        nt, m, Mtot = acc
        est.append(nt / ((nt + 5) * (nt - 1)) * Mtot + Fraction(1, 1000) * 5 / (nt + 5))
        Mt.append(Mtot)
        mean.append(m)
    return est, Mt, mean


def n_dbl(c, R):
    """double-precision roundings on one dimension's chain of sums (the module docstring derives it)"""
    return c + 6 + 7 * (R - 1) + 8 + 3 * (R - 1) * (c + 3 + 4 * (R - 1)) + 1


def gamma(k, u=U64):
    assert k * u < 0.5
    return k * u / (1 - k * u)


def pooled_bound(est, Mt, c, R, dtype):
    g = gamma(n_dbl(c, R))
    return np.array([float(g * (Mx + Fraction(1, 1000)) + Fraction(U_T[np.dtype(dtype)]) * abs(ex)) for ex, Mx in zip(est, Mt)])


def pooled_error(got, est):
    return np.array([float(abs(Fraction(float(g)) - ex)) for g, ex in zip(got, est)])


def states_after_last_push(ranks):
    """the ranks' Welford states after i = 99, gathered in rank order, with the 100th push emulated in the element type"""
    mu = np.concatenate([r["mu"] for r in ranks])
    M = np.concatenate([r["M"] for r in ranks])
    x = np.concatenate([np.ascontiguousarray(r["th_last"].T) for r in ranks])
    return welford_push_T(mu, M, x, MU.WINDOW_END - 75)


def check_against_reference(key, metric, ranks, parts, c, dtype):
    mu, M = states_after_last_push(ranks)
    est, Mt, mean = pooled_reference(mu, M, MU.WINDOW_END - 75, parts)
    n_tot = (MU.WINDOW_END - 75) * mu.shape[0]
    assert all(n_tot * m * m <= Mx for m, Mx in zip(mean, Mt)), "the bound is stated for |pooled mean| ≤ pooled sd"
    return record_bound(key, pooled_error(metric, est), pooled_bound(est, Mt, c, len(parts), dtype)), (est, Mt)


# ------------------------------------------------------------------------------------------------------------------------
# CPU: the stand-in's exchange logic, the reference
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_loopback_exchange_logic_on_host_buffers(tmp_path, sanitize):
    """tests/host_ref/loopback_rccl_driver.cpp (its own main, forks 3 ranks on the host-buffer build): sum / max all-reduce and
    all-gather of double / float in and out of place, rank order, count and type mismatches → ncclInvalidArgument on every rank, an
    absent rank with a 1 s deadline → ncclSystemError within seconds and every process reaped, no communicator left alive.  Run as
    a stand-alone binary, once plain and once built with -fsanitize=address,undefined and the sanitizers' runtimes linked statically
    (nothing is loaded into Python)."""
    exe = MU.loopback_driver(sanitize)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([exe, str(tmp_path)], env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), res.stdout[-3000:] + res.stderr[-3000:]
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-3000:]
    for case in ("collectives", "refusals", "absent_at_init", "absent_at_collective", "unique_ids"):
        assert any(line.startswith(case) and " ok " in line for line in res.stdout.splitlines()), res.stdout


@pytest.fixture(scope="module")
def oracle_injected(oracle):
    """the oracle's single-process PooledVar under the injected route, once per element type"""
    out = {}
    for dt in ("float64", "float32"):
        p = {"D": 5, "split": [11], "dtype": dt, "seed": 31}
        out[dt] = (p, MU.injected_part(A, oracle, p, 0, 11))
    return out


@pytest.mark.parametrize("dt", ["float64", "float32"])
def test_reference_is_partition_free_and_holds_the_oracle(oracle_injected, dt):
    """pooled_reference gives the same rationals for every partition of the chains, and the oracle's single-process estimate
    (sequential sums: c = N, R = 1) lies within the bound of it — the reference is judged before it judges the engine"""
    p, r = oracle_injected[dt]
    mu, M = states_after_last_push([r])
    n = MU.WINDOW_END - 75
    whole = pooled_reference(mu, M, n, [(0, 11)])
    for parts in ([(0, 4), (4, 7)], [(0, 1), (1, 3), (4, 7)], [(0, 4), (4, 4), (8, 3)], [(i, 1) for i in range(11)]):
        assert pooled_reference(mu, M, n, parts) == whole
    # against the definition: the variance of all 25·N draws cannot be formed from the states, but the merged M can be checked
    # against the direct two-pass sum over the chain means
    m = sum(Fraction(float(v)) for v in mu[:, 0]) / 11
    assert whole[1][0] == sum(Fraction(float(v)) for v in M[:, 0]) + n * sum((Fraction(float(v)) - m) ** 2 for v in mu[:, 0])
    worst, _ = check_against_reference(f"oracle single-process {dt}", r["metric"], [r], [(0, 11)], 11, dt)
    assert worst <= 1.0


def host_pool(mu, M, n, parts, defect=None):
    """k_pool_var and k_pool_finish in numpy doubles, sum for sum (four chain strides, the pairwise combine, the merge in order);
    `defect` plants a wrong merge: "no_delta_term" drops δ²·n_a·n_b / n_t, "nb_over_na" moves the mean by n_b / n_a"""
    D = mu.shape[1]
    n = float(n)
    blocks = []
    for off, cnt in parts:
        m64, M64 = mu[off:off + cnt].astype(np.float64), M[off:off + cnt].astype(np.float64)
        s_mu, s_M = np.zeros((4, D)), np.zeros((4, D))
        for ch in range(cnt):
            s_mu[ch % 4] += m64[ch]
            s_M[ch % 4] += M64[ch]
        mean = ((s_mu[0] + s_mu[1]) + (s_mu[2] + s_mu[3])) / float(cnt)
        s_d = np.zeros((4, D))
        for ch in range(cnt):
            df = m64[ch] - mean
            s_d[ch % 4] += df * df
        blocks.append((n * cnt, mean, ((s_M[0] + s_M[1]) + (s_M[2] + s_M[3])) + n * ((s_d[0] + s_d[1]) + (s_d[2] + s_d[3]))))
    na, m, Mt = blocks[0]
    for nb, mb, Mb in blocks[1:]:
        delta, nt = mb - m, na + nb
        m = m + delta * (nb / (na if defect == "nb_over_na" else nt))
        Mt = Mt + Mb + (0.0 if defect == "no_delta_term" else delta * delta * (na * nb / nt))
        na = nt
    est = na / ((na + 5) * (na - 1)) * Mt + 1e-3 * (5 / (na + 5))
    return est.astype(mu.dtype)


@pytest.mark.parametrize("dt", ["float64", "float32"])
def test_reference_catches_two_planted_merge_defects(oracle_injected, dt):
    """the faithful host copy of the two kernels passes the check over 2 and 3 partitions; a merge without the δ²·n_a·n_b / n_t
    term, and one that moves the mean by n_b / n_a instead of n_b / n_t, are both caught — by a wide margin"""
    p, r = oracle_injected[dt]
    mu, M = states_after_last_push([r])
    n = MU.WINDOW_END - 75
    for parts in ([(0, 5), (5, 6)], [(0, 4), (4, 4), (8, 3)]):
        c, R = -(-max(cnt for _, cnt in parts) // 4), len(parts)
        est, Mt, _ = pooled_reference(mu, M, n, parts)
        bound = pooled_bound(est, Mt, c, R, dt)
        tag = f"{dt} {R} parts"
        assert record_bound(f"host copy of the kernels {tag}", pooled_error(host_pool(mu, M, n, parts), est), bound) <= 1.0
        for defect in ("no_delta_term", "nb_over_na"):
            if defect == "nb_over_na" and R == 2:
                continue     # (with two partitions the mean of the last merge feeds nothing: the defect needs a third)
            worst = record_bound(f"planted {defect} {tag}", pooled_error(host_pool(mu, M, n, parts, defect), est), bound, planted=True)
            assert worst > 1e3, (defect, tag, worst)


# ------------------------------------------------------------------------------------------------------------------------
# GPU: the worlds
# ------------------------------------------------------------------------------------------------------------------------
def scenarios_of(R):
    """what the R workers run, in order.  Per-rank N from {1, 3, 5, 11, 258} (N < 4 leaves chain strides of k_pool_var and
    k_moments_reduce empty, 258 wraps the 256-thread counter loop once), D from {1, 64, 70} (70: a second, partial block of 64
    dimensions), 23 chains over 3 ranks by chain_shard (8 / 8 / 7), equal splits for gather_state"""
    if R == 1:
        return [{"kind": "one_rank"}]
    if R == 2:
        return [{"kind": "injected", "D": 1, "split": [1, 3], "dtype": "float64", "seed": 11},
                {"kind": "injected", "D": 64, "split": [5, 11], "dtype": "float32", "seed": 12},
                {"kind": "injected", "D": 70, "split": [258, 3], "dtype": "float64", "seed": 13},
                {"kind": "injected", "D": 70, "split": [11, 258], "dtype": "float32", "seed": 14},
                {"kind": "run", "D": 70, "split": [11, 11], "dtype": "float64", "seed": 17},
                {"kind": "run", "D": 1, "split": [3, 5], "dtype": "float64", "seed": 18},
                {"kind": "run", "D": 64, "split": [258, 258], "dtype": "float32", "seed": 19},
                {"kind": "ownership"},
                {"kind": "refusals"}]
    shard23 = [chain_shard(23, r, 3)[1] for r in range(3)]
    assert shard23 == [8, 8, 7]
    return [{"kind": "injected", "D": 70, "split": shard23, "dtype": "float64", "seed": 21},
            {"kind": "injected", "D": 70, "split": shard23, "dtype": "float32", "seed": 22},
            {"kind": "injected", "D": 64, "split": [1, 3, 5], "dtype": "float64", "seed": 23},
            {"kind": "injected", "D": 1, "split": [11, 1, 258], "dtype": "float32", "seed": 24},
            {"kind": "run", "D": 70, "split": shard23, "dtype": "float64", "seed": 27},
            {"kind": "run", "D": 64, "split": [5, 5, 5], "dtype": "float64", "seed": 28},
            {"kind": "run", "D": 1, "split": [3, 3, 3], "dtype": "float32", "seed": 29},
            {"kind": "run", "D": 70, "split": [1, 258, 11], "dtype": "float32", "seed": 30}]


_WORLDS = {}


def world(R, tmp_path_factory):
    """the results of the R-rank world, started once per session: a list of (scenario, [rank results])"""
    if R not in _WORLDS:
        sc = scenarios_of(R)
        try:
            res, seconds = MU.run_world(R, sc, tmp_path_factory.mktemp(f"world{R}"))
        except Exception as ex:          # (kept: every test of this world reports the same failure, and nothing is started again)
            _WORLDS[R] = ex
            raise
        WORKER_SECONDS[f"R={R}"] = {"wall": round(seconds, 2), "scenarios": [round(max(float(r["seconds"]) for r in ranks), 3) for ranks in res]}
        _dump_margins()
        _WORLDS[R] = list(zip(sc, res))
    if isinstance(_WORLDS[R], Exception):
        raise _WORLDS[R]
    return _WORLDS[R]


_SINGLE = {}


def single(hip, p):
    """the single-process HIP engine holding all chains of scenario `p`, run once"""
    key = json.dumps(p, sort_keys=True)
    if key not in _SINGLE:
        fn = MU.injected_part if p["kind"] == "injected" else MU.run_part
        _SINGLE[key] = fn(A, hip, p, 0, sum(p["split"]))
    return _SINGLE[key]


def tag_of(p):
    return f"R={len(p['split'])} D={p['D']} N={'+'.join(map(str, p['split']))} {p['dtype']}"


def of_kind(w, kind):
    got = [(p, ranks) for p, ranks in w if p["kind"] == kind]
    assert got
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("R", [2, 3])
def test_pooled_merge_of_R_ranks_against_the_exact_reference(hip, tmp_path_factory, R):
    """(a) injected (θ_i, α_i), the same for every global chain whatever the partition, window 76 … 100: the (D,) metric after the
    pooled update is bit-identical on every rank, within the bound of the module docstring of `pooled_reference` of the gathered
    per-chain states, within rtol 1e-12 of a single-process engine holding all chains, and cost exactly one all-gather.
    (MI355X: the R workers are started here, once for all tests of this world size — 2.2 s for R = 2, 2.4 s for R = 3; this test
    3.5 s / 2.6 s with them and the rational reference.)"""
    for p, ranks in of_kind(world(R, tmp_path_factory), "injected"):
        tag = "(a) " + tag_of(p)
        dtype = np.dtype(p["dtype"])
        for r in ranks[1:]:
            record_bits(tag + " metric across ranks", r["metric"], ranks[0]["metric"])
        for r in ranks:
            np.testing.assert_array_equal(r["allgathers"], [0, 1], err_msg=tag)
        c = -(-max(p["split"]) // 4)
        check_against_reference(tag + " metric against the exact reference", ranks[0]["metric"], ranks, MU.spans_of(p["split"]), c, dtype)
        one = single(hip, p)
        # the per-chain states do not depend on the partition at all
        record_bits(tag + " welford states against the single process", np.concatenate([r["mu"] for r in ranks]), one["mu"])
        record_bits(tag + " welford states against the single process", np.concatenate([r["M"] for r in ranks]), one["M"])
        check_against_reference(tag + " single-process metric against the exact reference", one["metric"], [one], [(0, sum(p["split"]))],
                                -(-sum(p["split"]) // 4), dtype)
        np.testing.assert_allclose(ranks[0]["metric"], one["metric"], rtol=1e-12, err_msg=tag)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [2, 3])
def test_sharded_warmup_equals_the_single_process_run(hip, tmp_path_factory, R):
    """(b) StanHMCAdaptor(PooledVar, StepSizeAdaptor(0.8)) + NUTS, Philox streams of the global chains, the fused warm-up through the
    first window end: up to and including that transition nothing a chain sees depends on the partition, so θ, the step sizes and
    every statistic are the single-process run's columns bit for bit; the metric after the update is the same bits on every rank
    and within rtol 1e-12 of the single process's; ten further draws leave every rank finite, with one metric"""
    for p, ranks in of_kind(world(R, tmp_path_factory), "run"):
        tag = "(b) " + tag_of(p)
        one = single(hip, p)
        for (off, cnt), r in zip(MU.spans_of(p["split"]), ranks):
            record_bits(tag + " theta", r["theta"], one["theta"][:, off:off + cnt])
            record_bits(tag + " stepsize", r["stepsize"], one["stepsize"][off:off + cnt])
            for key in [k for k in r if k.startswith("stat_")]:
                record_bits(tag + " stats", r[key], one[key][off:off + cnt])
            assert int(r["run_allgathers"]) == 1, tag
            assert np.isfinite(r["theta2"]).all() and np.isfinite(r["metric2"]).all(), tag
            record_bits(tag + " metric across ranks", r["metric"], ranks[0]["metric"])
            record_bits(tag + " metric across ranks after the draws", r["metric2"], ranks[0]["metric2"])
            record_bits(tag + " metric across ranks after the draws", r["metric2"], r["metric"])
        np.testing.assert_allclose(ranks[0]["metric"], one["metric"], rtol=1e-12, err_msg=tag)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [2, 3])
def test_gather_moments_over_R_ranks(hip, tmp_path_factory, R):
    """(c) ahmc_gather_moments (k_moments_reduce, one all-reduce of 2·D + 3 doubles): mean, var and the three counts are the same
    bits on every rank; the counts of the warm-up transitions equal the single-process run's exactly, those of the ten draws the
    sum of the ranks' own; mean / var within rtol 1e-10 / 1e-9 of the values formed from the concatenated accumulators"""
    for p, ranks in of_kind(world(R, tmp_path_factory), "run"):
        one = single(hip, p)
        for phase in ("w_", "d_"):
            tag = f"(c) {tag_of(p)} {'warm-up' if phase == 'w_' else 'draws'}"
            for r in ranks[1:]:
                for key in ("g_mean", "g_var", "g_counts"):
                    record_bits(tag + " across ranks", r[phase + key], ranks[0][phase + key])
            counts = sum(r[phase + "acc_counts"] for r in ranks)
            np.testing.assert_array_equal(ranks[0][phase + "g_counts"], counts, err_msg=tag)
            if phase == "w_":
                np.testing.assert_array_equal(ranks[0]["w_g_counts"], one["w_acc_counts"], err_msg=tag)
                np.testing.assert_array_equal(ranks[0]["w_g_counts"], one["w_g_counts"], err_msg=tag)
                record_bits(tag + " accumulators against the single process", np.concatenate([r["w_acc_sum"] for r in ranks], axis=1), one["w_acc_sum"])
            assert counts[0] == (MU.WINDOW_END if phase == "w_" else 10) * sum(p["split"]) and counts[1] >= counts[0], tag
            s1 = np.concatenate([r[phase + "acc_sum"] for r in ranks], axis=1).astype(np.float64)
            s2 = np.concatenate([r[phase + "acc_sumsq"] for r in ranks], axis=1).astype(np.float64)
            mean = s1.sum(axis=1) / counts[0]
            np.testing.assert_allclose(ranks[0][phase + "g_mean"], mean, rtol=1e-10, atol=1e-12, err_msg=tag)
            np.testing.assert_allclose(ranks[0][phase + "g_var"], s2.sum(axis=1) / counts[0] - mean ** 2, rtol=1e-9, err_msg=tag)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [2, 3])
def test_gather_state_and_comm_info_over_R_ranks(tmp_path_factory, R):
    """(d) with equal shards block r of the (D, N, R) buffer is rank r's θ bit for bit on every rank; with unequal shards (8 / 8 / 7
    among them) every rank is refused with AHMC_ERR_ARGUMENT before the collective (no all-gather is served, nobody waits) and a
    transition afterwards is valid; comm_info reports what the split is"""
    seen = set()
    for p, ranks in of_kind(world(R, tmp_path_factory), "run"):
        tag = "(d) " + tag_of(p)
        split = p["split"]
        equal = min(split) == max(split)
        seen.add(equal)
        for r in ranks:
            np.testing.assert_array_equal(r["comm_info"], [R, sum(split), min(split), max(split)], err_msg=tag)
            assert np.isfinite(r["theta3"]).all() and not np.array_equal(r["theta3"], r["theta2"]), tag
            if equal:
                assert int(r["gather_rc"]) == capi.OK and int(r["gather_allgathers"]) == 1, tag
                for q, src in enumerate(ranks):
                    record_bits(tag + " gathered block", r["gathered"][q], np.ascontiguousarray(src["theta2"].T))
            else:
                assert int(r["gather_rc"]) == capi.ERR_ARGUMENT and int(r["gather_allgathers"]) == 0, tag
                assert "different numbers of chains" in str(r["gather_msg"]) and f"({min(split)} … {max(split)};" in str(r["gather_msg"]), r["gather_msg"]
                assert np.isnan(r["gathered"]).all(), tag     # nothing was written
    assert seen == {True, False}


@pytest.mark.gpu
def test_communicator_attachment_and_ownership(tmp_path_factory):
    """(e) a communicator the caller made (the stand-in's own ncclCommInitRank) and handed to ahmc_set_comm survives the context;
    one made by ahmc_comm_init is destroyed with it; re-attaching releases the previous one; a two-rank communicator announced as
    three is refused with AHMC_ERR_RUNTIME, and the context still makes a valid transition"""
    (p, ranks), = of_kind(world(2, tmp_path_factory), "ownership")
    for r in ranks:
        v = {k: r[k].item() for k in r}
        base = v["live_start"]
        assert base == 0
        assert v["set_comm_seen"] == 2
        assert v["live_attached"] == base + 1 and v["live_after_close_of_borrower"] == base + 1 and v["live_after_own_destroy"] == base
        assert v["live_owned"] == base + 1 and v["live_after_close_of_owner"] == base
        assert v["live_after_reattach"] == base + 1 and v["live_after_detach"] == base and v["finite_after_detach"]
        assert v["announce_rc"] == capi.ERR_RUNTIME and "2 rank(s) answered the all-reduce, 3 were announced" in v["announce_msg"], v["announce_msg"]
        assert v["finite_after_announce"] and v["live_end"] == base


@pytest.mark.gpu
def test_refusals_of_a_context_with_more_than_one_rank(tmp_path_factory):
    """(f) ahmc_diag_summary, ahmc_diag_rank_normalize and ahmc_lowrank_adaptor_init answer AHMC_ERR_UNSUPPORTED on a context whose
    communicator has two ranks; a valid transition follows each refusal"""
    (p, ranks), = of_kind(world(2, tmp_path_factory), "refusals")
    for r in ranks:
        for name, words in (("summary", "communicator of 2 ranks"), ("rank_normalize", "communicator of 2 ranks"), ("lowrank", "not pooled across ranks")):
            assert r[name + "_rc"].item() == capi.ERR_UNSUPPORTED, (name, r[name + "_rc"], r[name + "_msg"])
            assert words in str(r[name + "_msg"]), r[name + "_msg"]
            assert r[name + "_finite_after"].item()


@pytest.mark.gpu
def test_one_rank_through_the_stand_in_gives_the_bits_of_no_communicator(hip, tmp_path_factory):
    """(g) the run of test_hip_pooled_adaptation_through_a_one_rank_communicator in a child whose RCCL is the stand-in: the bits of
    the run without a communicator — which real RCCL gives with one rank too, so the stand-in is tied to it"""
    from test_v3_state_gather import make

    (p, (r,)), = of_kind(world(1, tmp_path_factory), "one_rank")
    e, k, h = make(hip, 24, 300, "stan_pooled", np.random.default_rng(8), shared_metric=True)
    e.run(k, 110, MU.N_ADAPTS)
    for key, want in (("metric", e.get_metric()), ("theta", e.theta()), ("stepsize", e.get_stepsize())):
        record_bits("(g) one rank through the stand-in " + key, r[key], want)
    e.close()
    assert r["ranks_seen"].item() == 1 and r["allgathers"].item() == 1 and r["live_end"].item() == 0
