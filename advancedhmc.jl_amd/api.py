"""Host-side mirror of AdvancedHMC.jl's operator interface for the sampler-vec path.

Julia is absent from the build image, so the host side above the C ABI is written in Python
with the reference's names, argument meaning and error behaviour (so the parity tests read like
test/sampler-vec.jl, test/integrator.jl, test/trajectory.jl).  The Julia package extension that
binds the same ABI with `ccall` is julia/AdvancedHMCMI355XExt.jl.

Every class cites the reference definition it mirrors (paths under the AdvancedHMC.jl checkout).
Arrays are (D, N) column-major like a Julia Matrix: numpy arrays are converted with
`np.asfortranarray`, results come back as F-ordered (D, N) arrays (or (D,) for a single chain).
All compute happens in the C library the `Engine` is bound to — the HIP engine unless a test
injects another `CLib`.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from . import _capi as capi
from . import rank_update as _ru
from . import glm as _glm
from ._capi import ArgumentError


# ------------------------------------------------------------------------------------------------
# RNG handle (replaces `rng::AbstractRNG`)
# ------------------------------------------------------------------------------------------------
@dataclass
class PhiloxRNG:
    """Counter-based Philox4x32-10 stream family.  `chain_offset` is the global index of the
    first local chain (multi-GPU shards), `iteration` the transition counter."""
    seed: int = 0
    chain_offset: int = 0
    iteration: int = 0


def _rng_spec(rng, n_chains):
    """int | PhiloxRNG | sequence of PhiloxRNG (one per chain, src/utilities.jl:12-23)."""
    if rng is None:
        return PhiloxRNG(0), 1
    if isinstance(rng, (int, np.integer)):
        return PhiloxRNG(int(rng)), 1
    if isinstance(rng, PhiloxRNG):
        return rng, 1
    rngs = list(rng)
    if len(rngs) != n_chains:  # @argcheck length(rngs) == n_chains
        raise ArgumentError(capi.ERR_ARGUMENT, f"length(rngs) == n_chains must hold, got {len(rngs)} != {n_chains}")
    first = rngs[0]
    if all(r.seed == first.seed and r.chain_offset == first.chain_offset for r in rngs):
        return first, 0  # identically seeded RNG vector: every chain sees the same variates
    if all(r.seed == first.seed and r.chain_offset == first.chain_offset + k for k, r in enumerate(rngs)):
        return first, 1
    raise ArgumentError(capi.ERR_ARGUMENT, "a vector of RNGs must share one seed (same or consecutive streams)")


# ------------------------------------------------------------------------------------------------
# metrics (src/metric.jl:17-120)
# ------------------------------------------------------------------------------------------------
def _size_tuple(sz):
    if isinstance(sz, (int, np.integer)):
        return (int(sz),)
    return tuple(int(s) for s in sz)


class AbstractMetric:
    kind = None

    @property
    def D(self):
        return self.size[0]


class UnitEuclideanMetric(AbstractMetric):
    """src/metric.jl:17-35.  UnitEuclideanMetric([T,] sz)"""
    kind = capi.METRIC_UNIT

    def __init__(self, *args):
        if len(args) == 2:
            self.eltype, sz = np.dtype(args[0]), args[1]
        else:
            self.eltype, sz = np.dtype(np.float64), args[0]
        self.size = _size_tuple(sz)
        self.Minv = None

    def __repr__(self):
        return f"UnitEuclideanMetric({self.eltype}, {self.size})"


class DiagEuclideanMetric(AbstractMetric):
    """src/metric.jl:52-72.  DiagEuclideanMetric(M⁻¹) | DiagEuclideanMetric([T,] sz)"""
    kind = capi.METRIC_DIAG

    def __init__(self, *args):
        if len(args) == 2:
            T, sz = np.dtype(args[0]), _size_tuple(args[1])
            Minv = np.ones(sz, dtype=T, order="F")
        elif isinstance(args[0], np.ndarray):
            Minv = np.asfortranarray(args[0])
            if Minv.dtype not in (np.float32, np.float64):
                Minv = Minv.astype(np.float64)
        else:
            Minv = np.ones(_size_tuple(args[0]), dtype=np.float64, order="F")
        self.Minv = Minv
        self.eltype = Minv.dtype
        self.size = Minv.shape

    @property
    def sqrtMinv(self):
        return np.sqrt(self.Minv)

    def __repr__(self):
        return f"DiagEuclideanMetric({np.array2string(self.Minv.ravel(order='F')[:6], precision=3)} ...)"


class DenseEuclideanMetric(AbstractMetric):
    """src/metric.jl:89-120.  One (D, D) M⁻¹ shared by all chains (the reference has no batched
    dense metric, :103; sharing it is this engine's extension)."""
    kind = capi.METRIC_DENSE

    def __init__(self, *args):
        if len(args) == 2:
            T, D = np.dtype(args[0]), _size_tuple(args[1])[0]
            Minv = np.eye(D, dtype=T, order="F")
        elif isinstance(args[0], np.ndarray):
            Minv = np.asfortranarray(args[0])
        else:
            Minv = np.eye(_size_tuple(args[0])[0], dtype=np.float64, order="F")
        if Minv.ndim != 2 or Minv.shape[0] != Minv.shape[1]:
            raise ArgumentError(capi.ERR_ARGUMENT, "DenseEuclideanMetric needs a square M⁻¹")
        self.Minv = Minv
        self.eltype = Minv.dtype
        self.size = (Minv.shape[0],)


class RankUpdateEuclideanMetric(AbstractMetric):
    """src/metric.jl:179-245.  M⁻¹ = Diagonal(A) + B·D·Bᵀ, one metric shared by all chains (the reference's is single-chain,
    :322-323; sharing it is this engine's extension, as for DenseEuclideanMetric).  Constructors: RankUpdateEuclideanMetric(n),
    ([T,] n), ([T,] (n,)) — the identity, k = 0 — and (A, B, D) with A the diagonal (a vector, or a 2-D diagonal matrix).
    Fields A (the diagonal, (D,)), B (D, k), D (k, k), factorization (rank_update.WoodburyFactorization); arithmetic:
    advancedhmc.jl_amd/rank_update.py."""
    kind = capi.METRIC_RANK_UPDATE
    D = None  # (the reference's field D, the k×k inner matrix — not AbstractMetric.D, the dimension: that is size[0] here)

    def __init__(self, *args):
        if len(args) == 3:
            A, B, Dm = (np.asarray(x) for x in args)
            if A.ndim == 2:
                if A.shape[0] != A.shape[1] or np.count_nonzero(A - np.diag(np.diag(A))):
                    raise ArgumentError(capi.ERR_ARGUMENT, "RankUpdateEuclideanMetric: A must be a Diagonal")
                A = np.diag(A)
            T = np.result_type(A, B, Dm)
            if T not in (np.float32, np.float64):
                T = np.dtype(np.float64)
            if B.ndim != 2 or B.shape[0] != A.size or Dm.shape != (B.shape[1], B.shape[1]):
                raise ArgumentError(capi.ERR_ARGUMENT, f"DimensionMismatch: A {A.shape}, B {B.shape}, D {Dm.shape}")
            self.A = np.ascontiguousarray(A, dtype=T)
            self.B = np.asfortranarray(B, dtype=T)
            self.D = np.asfortranarray(Dm, dtype=T)
            if not (np.all(np.isfinite(self.A)) and np.all(self.A > 0)):
                raise ArgumentError(capi.ERR_ARGUMENT, "DomainError: A must be a positive definite diagonal")
            try:
                self.factorization = _ru.woodbury_factorize(self.A, self.B, self.D)
            except np.linalg.LinAlgError as e:
                raise ArgumentError(capi.ERR_ARGUMENT, f"PosDefException: I + R·D·Rᵀ is not positive definite ({e})")
        else:
            if len(args) == 2:
                T, n = np.dtype(args[0]), _size_tuple(args[1])[0]
            elif len(args) == 1:
                T, n = np.dtype(np.float64), _size_tuple(args[0])[0]
            else:
                raise ArgumentError(capi.ERR_ARGUMENT, "RankUpdateEuclideanMetric([T,] n), ([T,] (n,)) or (A, B, D)")
            self.A = np.ones(n, dtype=T)
            self.B = np.zeros((n, 0), dtype=T, order="F")
            self.D = np.zeros((0, 0), dtype=T, order="F")
            self.factorization = _ru.woodbury_factorize(self.A, self.B, self.D)
        self.eltype = self.A.dtype
        self.size = (self.A.size,)
        self.Minv = None

    @property
    def rank(self):
        return self.B.shape[1]

    @property
    def _diag_inv_metric(self):
        return _ru.diag_inv_metric(self.A, self.B, self.D)

    def __repr__(self):
        return f"RankUpdateEuclideanMetric({np.array2string(self._diag_inv_metric[:6], precision=3)} ..., rank {self.rank})"


def renew(metric, Minv):
    """src/metric.jl:31,69,117"""
    if isinstance(metric, UnitEuclideanMetric):
        return metric
    if isinstance(metric, RankUpdateEuclideanMetric):
        return RankUpdateEuclideanMetric(*Minv)  # (A, B, D)
    return type(metric)(np.asarray(Minv))


# ------------------------------------------------------------------------------------------------
# targets: the (ℓπ, ∂ℓπ∂θ) pair of Hamiltonian (src/hamiltonian.jl:1-20) as built-in families
# ------------------------------------------------------------------------------------------------
@dataclass
class Target:
    kind: int
    D: int
    params: Optional[np.ndarray] = None


def IsoGaussian(D):
    """ℓπ of test/common.jl:76-77 (`Gaussian(zeros(D), ones(D))`)"""
    return Target(capi.TARGET_ISO_GAUSS, int(D))


def DiagGaussian(m, s):
    """test/common.jl:35-77 `Gaussian(m, s)` with the exact gradient (m-x)/s²"""
    m = np.asarray(m, dtype=np.float64).ravel()
    s = np.asarray(s, dtype=np.float64).ravel()
    if m.shape != s.shape:
        raise ArgumentError(capi.ERR_ARGUMENT, "DiagGaussian: m and s must have the same length")
    return Target(capi.TARGET_DIAG_GAUSS, m.size, np.concatenate([m, s]))


def Funnel(D):
    """Neal's funnel as defined in research/notebooks/geweke_test.ipynb cell 4"""
    return Target(capi.TARGET_FUNNEL, int(D))


def HierGaussian(D):
    """θ = (μ, log τ, x₁..x_{D-2}) hierarchical Gaussian"""
    return Target(capi.TARGET_HIER_GAUSS, int(D))


def DenseGaussian(P):
    """ℓπ = -½ θᵀPθ with P the (D, D) precision matrix"""
    P = np.asfortranarray(np.asarray(P, dtype=np.float64))
    return Target(capi.TARGET_DENSE_GAUSS, P.shape[0], P.ravel(order="F"))


@dataclass
class ExternalTarget:
    """User log-density evaluated by the caller: `fn(θ (D,N)) -> (ℓπ (N,), ∇ℓπ (D,N))`, the
    signature of `∂ℓπ∂θ` at test/common.jl:64-74 (what `Hamiltonian(metric, ℓπ, ∂ℓπ∂θ)` /
    LogDensityProblems hand the reference, src/AdvancedHMC.jl:163-186).  `Engine.step` runs through the
    split-step pair ahmc_lf_pre / ahmc_lf_post around this callback; whole transitions and
    find_good_stepsize run through the ask / tell calls ahmc_ext_* (`Engine._ext_drive`).  `fn` may
    also accept `fn(θ, chains)` — the indices of the columns that need evaluating — when
    `takes_chains` is set; the other columns of its result are ignored."""
    D: int
    fn: object
    kind: int = capi.TARGET_EXTERNAL
    params: Optional[np.ndarray] = None
    takes_chains: bool = False


@dataclass
class PluginTarget:
    """User log-density as a HIP DEVICE FUNCTION compiled INTO the engine's trajectory kernels (include/ahmc_user_target.h
    has the contract; ahmc_set_target_plugin): `source` is the path of a header defining
    `ahmc_user::logdensity<T, G, E>(params, D, theta, grad_neg, lane, d0)`.  The engine compiles it (hipcc, cached by content)
    for the context's element type and thread geometry the first time it is bound; from then on the density runs inside the
    same fused kernels as a built-in family — no host round trip.  HIP engine only (the CPU checker takes the same density
    as an ExternalTarget callback or a host KernelTarget)."""
    D: int
    source: str
    params: Optional[np.ndarray] = None
    kind: int = capi.TARGET_PLUGIN


@dataclass
class ObjectTarget:
    """User log-density as COMPILED device code — a relocatable object of `hipcc -fgpu-rdc -c` or raw amdgcn LLVM bitcode (`.bc`,
    what GPUCompiler.jl / AMDGPU.jl emit for a Julia function) that defines the C symbol of include/ahmc_user_target_object.h.
    `build_target_plugin_from_object` links it with the engine's trajectory kernels (device LTO: a bitcode density is inlined
    into the leaf loop) and the result is bound like a PluginTarget (ahmc_set_target_plugin): the fused kernels incl. the
    in-kernel warm-up, no host round trip, no per-leapfrog launch.  HIP engine only."""
    D: int
    object: str
    params: Optional[np.ndarray] = None
    kind: int = capi.TARGET_PLUGIN


@dataclass
class KernelTarget:
    """User log-density as a device KERNEL the engine launches itself (ahmc_set_target_kernel): `handle` is a hipFunction_t
    (handle_kind = capi.KERNEL_HIP_FUNCTION; what hipModuleGetFunction returns / AMDGPU.jl compiles a Julia kernel to), the
    host address of a __global__ symbol (KERNEL_HIP_SYMBOL), or — CPU checker only — a ctypes callback with the kernel's
    signature (KERNEL_HOST):  f(theta, lp, grad_neg, cols, n_cols, D, N, user)."""
    D: int
    handle: object
    handle_kind: int = capi.KERNEL_HIP_FUNCTION
    block_threads: int = 256
    chains_per_block: int = 1
    user: object = None
    kind: int = capi.TARGET_KERNEL
    params: Optional[np.ndarray] = None


class Factor:
    """A grouping factor of a GLMTarget, index-coded (include/ahmc_glm_factor.h): `index[i]` ∈ [0, n_levels) is the level of observation
    i (an integer array, zero-based); `n_levels` defaults to max + 1.  It stands for n_levels one-hot columns of X — one coefficient
    per level — without storing or multiplying them."""

    def __init__(self, index, n_levels=None):
        try:
            idx = np.asarray(index)
            if idx.ndim != 1 or idx.size < 1:
                raise ValueError(f"DimensionMismatch: a factor's index is one level per observation; got shape {idx.shape}")
            (self.index, self.n_levels), = _glm.check_factors([(idx, n_levels)], idx.size)
        except (ValueError, TypeError) as e:
            raise ArgumentError(capi.ERR_ARGUMENT, str(e))

    def __repr__(self):
        return f"Factor(n_obs={self.index.size}, n_levels={self.n_levels})"


def factor_ranges(P_x, factors):
    """[(start, stop)] of each factor's coefficient rows in a model with P_x dense columns — known before the target is constructed,
    as in `CoefGroup(*A.factor_ranges(1, [fac])[0], centered=False)`"""
    return _glm.factor_ranges(P_x, [f if isinstance(f, Factor) else Factor(*f) for f in factors])


class GLMTarget:
    """A generalised linear model as the target (include/ahmc_glm.h; arithmetic: advancedhmc.jl_amd/glm.py):
        ℓπ(θ) = Σ_i ℓ(y_i, (Xθ + offset)_i) − ½ Σ_d p_d θ_d²,    X (n_obs, D), D = X.shape[1]
    with `family` "bernoulli_logit" (0 <= y <= 1), "poisson_log" (y >= 0) or "gaussian_identity" (scale = 1/σ²); or a family whose
    dispersion is sampled (include/ahmc_glm_aux.h): "gaussian_identity_sigma" (unknown noise σ) or "negbinomial_log" (NB2 counts,
    variance μ + μ²/φ).  θ then has one more row, LAST: s = log σ or log φ, with the prior s ~ Normal(*aux_prior) = (loc, scale),
    default (0, 1), and `.D` counts it; `.dispersion(θ)` gives σ or φ of draws.  The prior of the coefficients is
    N(0, prior_scale²) per coefficient — `prior_scale` a scalar or (D,) — or given as its precision `prior_prec`; neither: flat.
    `factors` (at most 8 `Factor`s) add one coefficient per level after the columns of X: `.P_x` = X.shape[1] dense coefficients,
    `.P` = P_x + Σ n_levels in all, `.factor_ranges` their rows; prior_scale / prior_prec then have P entries.
    `family="ordered_logit"` with `n_categories=C` (include/ahmc_glm_ordinal.h): y holds ordered categories 0 … C − 1 and
    P(y <= k) = σ(c_{k+1} − η).  The model has no intercept — the cutpoints take its place, and a constant column in X is not
    identified.  θ ends with C − 1 rows κ (`.cut_rows`): κ_1 = c_1, κ_j = log(c_j − c_{j−1}), with the prior `cut_prior` =
    (loc_1, scale_1, loc_gap, scale_gap) on κ itself, default (0, 2.5, 0, 1); `.cutpoints(θ)` gives c of draws.
    `family="categorical_logit"` with `n_categories=C` (include/ahmc_glm_categorical.h): y holds UNORDERED classes 0 … C − 1, class 0
    the reference (multinomial / softmax regression).  There are K = C − 1 coefficient blocks of `.P_b` = P_x + Σ n_levels rows
    each, `.P` = K·P_b in all and no further rows: `.class_rows(k)` are the rows of class k = 1 … K, `.n_classes` = C; prior_scale /
    prior_prec have P entries (or broadcast), `offset` is (n_obs, K); `.class_probs(θ)` gives (C, n_obs, n) probabilities of draws.
    The engine evaluates all chains at once, X·Θ and Xᵀ·U on the MFMA units.  HIP engine only (the CPU checker takes the same
    density as `ExternalTarget(D, lambda th: glm.logdensity(...))` or a host KernelTarget)."""
    kind = capi.TARGET_GLM
    params = None
    groups = ()
    factors = ()

    n_categories = 0
    cut_prior = None
    n_classes = 0   # C of family "categorical_logit" (n_categories stays 0: it marks the ordinal family, which adds rows to θ)

    def __init__(self, X, y, family="bernoulli_logit", prior_scale=None, prior_prec=None, offset=None, scale=1.0, aux_prior=None, factors=None,
                 n_categories=None, cut_prior=None):
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64).ravel()
        if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1 or y.size != X.shape[0]:
            raise ArgumentError(capi.ERR_ARGUMENT, f"DimensionMismatch: X {X.shape}, y {y.shape}")
        ordinal = family in _glm.ORDINAL_FAMILIES if isinstance(family, str) else isinstance(family, (int, np.integer)) and family == _glm.ORDERED_LOGIT
        categorical = (family in _glm.CATEGORICAL_FAMILIES if isinstance(family, str)
                       else isinstance(family, (int, np.integer)) and family == _glm.CATEGORICAL_LOGIT)
        try:
            self.family = _glm.ORDERED_LOGIT if ordinal else _glm.CATEGORICAL_LOGIT if categorical else _glm.family_code(family)
        except ValueError as e:
            raise ArgumentError(capi.ERR_ARGUMENT, str(e))
        if categorical:
            if scale != 1.0 or aux_prior is not None or cut_prior is not None:
                raise ArgumentError(capi.ERR_ARGUMENT, "GLMTarget: family \"categorical_logit\" has no scale, no dispersion and no cutpoints; scale, aux_prior "
                                                       "and cut_prior do not apply")
            if n_categories is None:
                raise ArgumentError(capi.ERR_ARGUMENT, "GLMTarget: family \"categorical_logit\" needs n_categories")
            try:
                _, self.n_classes = _glm.check_classes(y, n_categories)
            except (ValueError, TypeError) as e:
                raise ArgumentError(capi.ERR_ARGUMENT, str(e))
        elif not ordinal and (n_categories is not None or cut_prior is not None):
            raise ArgumentError(capi.ERR_ARGUMENT, f"GLMTarget: n_categories and cut_prior belong to family \"ordered_logit\", not to family {self.family}")
        if ordinal:
            if scale != 1.0 or aux_prior is not None:
                raise ArgumentError(capi.ERR_ARGUMENT, "GLMTarget: family \"ordered_logit\" has no scale and no dispersion; scale and aux_prior do not apply")
            if n_categories is None:
                raise ArgumentError(capi.ERR_ARGUMENT, "GLMTarget: family \"ordered_logit\" needs n_categories")
            try:
                _, self.n_categories = _glm.check_categories(y, n_categories)
                self.cut_prior = _glm.check_cut_prior(cut_prior)
            except (ValueError, TypeError) as e:
                raise ArgumentError(capi.ERR_ARGUMENT, str(e))
        if prior_scale is not None and prior_prec is not None:
            raise ArgumentError(capi.ERR_ARGUMENT, "GLMTarget: give prior_scale or prior_prec, not both")
        self.aux = self.family in _glm.AUX_FAMILIES
        if aux_prior is not None and not self.aux:
            raise ArgumentError(capi.ERR_ARGUMENT, f"GLMTarget: aux_prior belongs to the families with a sampled dispersion, not to family {self.family}")
        if self.aux and scale != 1.0:
            raise ArgumentError(capi.ERR_ARGUMENT, f"GLMTarget: family {self.family} samples its dispersion; scale does not apply")
        try:
            self.aux_prior = _glm.check_aux_prior(aux_prior) if self.aux else None
        except (ValueError, TypeError) as e:
            raise ArgumentError(capi.ERR_ARGUMENT, str(e))
        self.X = np.asfortranarray(X)
        self.y = y
        self.n_obs = X.shape[0]
        try:
            facs = [f if isinstance(f, Factor) else Factor(*f) for f in (factors or ())]
            _glm.check_factors(facs, self.n_obs)
        except (ValueError, TypeError) as e:
            raise ArgumentError(capi.ERR_ARGUMENT, str(e))
        self.factors = tuple(facs)
        self.P_x = X.shape[1]
        self.factor_ranges = _glm.factor_ranges(self.P_x, self.factors)
        self.P_b = self.P_x + sum(f.n_levels for f in self.factors)    # (the rows of one block; a categorical model has C − 1 of them)
        self.P = self.P_b * (self.n_classes - 1 if self.n_classes else 1)
        self.D = self.P + (1 if self.aux else 0) + self._n_cut
        if prior_scale is not None:
            prior_prec = 1.0 / np.square(np.asarray(prior_scale, dtype=np.float64))
        try:
            self.prior_prec = None if prior_prec is None else np.ascontiguousarray(np.broadcast_to(np.asarray(prior_prec, dtype=np.float64), (self.P,)))
        except ValueError:
            raise ArgumentError(capi.ERR_ARGUMENT, f"DimensionMismatch: the prior has {np.size(prior_prec)} entries, the model P = {self.P} coefficients")
        if self.n_classes and offset is not None:
            try:
                self.offset = np.asfortranarray(_glm._class_offset(offset, self.n_obs, self.n_classes - 1))
            except (ValueError, TypeError) as e:
                raise ArgumentError(capi.ERR_ARGUMENT, str(e))
        else:
            self.offset = None if offset is None else np.asarray(offset, dtype=np.float64).ravel()
            if self.offset is not None and self.offset.size != self.n_obs:
                raise ArgumentError(capi.ERR_ARGUMENT, f"DimensionMismatch: offset {self.offset.shape}, n_obs {self.n_obs}")
        self.scale = float(scale)

    @property
    def _n_cut(self):
        return self.n_categories - 1 if self.n_categories else 0

    @property
    def cut_rows(self):
        """(start, stop) of the rows κ of θ: (D − C + 1, D)"""
        if not self.n_categories:
            raise ArgumentError(capi.ERR_ARGUMENT, f"cut_rows: family {self.family} has no cutpoints")
        return self.D - self._n_cut, self.D

    def cutpoints(self, theta):
        """c (C − 1, n) of draws θ (D, n) by the numpy mirror (family "ordered_logit")"""
        lo, hi = self.cut_rows
        return _glm.cutpoints(np.asarray(theta, dtype=np.float64)[lo:hi])

    def class_rows(self, k):
        """(start, stop) of the coefficient rows of class k = 1 … C − 1 of a categorical model: ((k − 1)·P_b, k·P_b)"""
        if not self.n_classes:
            raise ArgumentError(capi.ERR_ARGUMENT, f"class_rows: family {self.family} has no class blocks")
        if not 1 <= int(k) < self.n_classes:
            raise ArgumentError(capi.ERR_ARGUMENT, f"class_rows: class {k} is outside [1, {self.n_classes}) (class 0 is the reference: it has no coefficients)")
        return (int(k) - 1) * self.P_b, int(k) * self.P_b

    def class_probs(self, theta):
        """(C, n_obs, n) class probabilities at draws θ (D, n) by the numpy mirror (family "categorical_logit")"""
        if not self.n_classes:
            raise ArgumentError(capi.ERR_ARGUMENT, f"class_probs: family {self.family} has no classes")
        return _glm.categorical_probs(_glm.categorical_pointwise(self.X, self.y, theta, self.n_classes, self.groups, self.offset, self.factors)[0])

    def logdensity(self, theta):
        """(ℓπ (N,), ∇ℓπ (D, N)) by the numpy mirror: the callback of an ExternalTarget for the same model"""
        if self.n_classes:
            return _glm.categorical_logdensity(self.X, self.y, theta, self.n_classes, self.groups, self.offset, self.prior_prec, factors=self.factors)
        if self.n_categories:
            return _glm.ordinal_logdensity(self.X, self.y, theta, self.n_categories, self.groups, self.offset, self.prior_prec, self.cut_prior,
                                           factors=self.factors)
        return _glm.hier_logdensity(self.family, self.X, self.y, theta, self.groups, self.offset, self.prior_prec, self.scale, self.aux_prior,
                                    factors=self.factors)

    def dispersion(self, theta):
        """σ or φ = exp(s) of draws θ (D, n) by the numpy mirror (a family with a sampled dispersion)"""
        if not self.aux:
            raise ArgumentError(capi.ERR_ARGUMENT, f"dispersion: family {self.family} has no sampled dispersion")
        return _glm.dispersion(theta)

    def predict(self, theta, newdata, what="mean"):
        """`what` ("linear" | "mean" | "variance" | "loglik") of the model at the rows of `newdata` (a GLMNewData) and draws θ (D, n) by
        the numpy mirror (glm.predict): what Engine.glm_predict computes on the device"""
        try:
            if len(newdata.factors) != len(self.factors):
                raise ValueError(f"DimensionMismatch: the new data have {len(newdata.factors)} factors, the model {len(self.factors)}")
            facs = [(np.asarray(idx), f.n_levels) for idx, f in zip(newdata.factors, self.factors)]
            family = "categorical_logit" if self.n_classes else "ordered_logit" if self.n_categories else self.family
            return _glm.predict(family, newdata.X, theta, what, factors=facs, offset=newdata.offset, y=newdata.y, groups=self.groups,
                                n_categories=self.n_classes or self.n_categories or None, scale=self.scale)
        except (ValueError, TypeError) as e:
            raise ArgumentError(capi.ERR_ARGUMENT, str(e))

    def __repr__(self):
        return f"GLMTarget(n_obs={self.n_obs}, D={self.D}, family={self.family})"


def glm_yrep_at(engine, family, q, aux=None, row=None, col=None, seed=0, n_categories=0):
    """`engine.glm_yrep_at(...)`: the device's outcome sampler on the caller's planes (include/ahmc_glm_yrep.h)"""
    return engine.glm_yrep_at(family, q, aux=aux, row=row, col=col, seed=seed, n_categories=n_categories)


def glm_summary_dict(summary, K=1, n_categories=0):
    """the rows of a (2Q + 1, n_new) summary (ahmc_glm_predict_summary, glm.predict_summary) by name; K predictors, `n_categories` of an
    ordinal or a categorical model (0: a family with one mean)"""
    s = np.asarray(summary)
    Q = K + (n_categories or 2)
    if s.ndim != 2 or s.shape[0] != 2 * Q + 1:
        raise ArgumentError(capi.ERR_ARGUMENT, f"DimensionMismatch: summary {s.shape}, expected ({2 * Q + 1}, n_new)")
    eta = slice(0, 2 * K, 2) if K > 1 else 0
    out = {"eta_mean": s[eta].copy(), "eta_var": s[slice(1, 2 * K, 2) if K > 1 else 1].copy()}
    if n_categories:
        out["probs"], out["probs_var"] = s[2 * K:2 * Q:2].copy(), s[2 * K + 1:2 * Q:2].copy()
    else:
        out["mean"], out["mean_var"], out["var_within"] = s[2].copy(), s[3].copy(), s[4].copy()
    out["lpd"] = s[2 * Q].copy()
    return out


class GLMNewData:
    """New rows of data for a bound GLMTarget (include/ahmc_glm_predict.h: ahmc_glm_newdata): X (n_new, P_x); `factors`: one integer
    array of zero-based level indices (n_new,) per factor of the model, in its order (levels the model has not seen are refused);
    `offset` (n_new,) — (n_new, C − 1) for a categorical model — or None: zeros; `y` (n_new,) or None: the held-out outcomes, which
    "loglik" and the summary's lpd need."""

    def __init__(self, X, factors=None, offset=None, y=None):
        X = np.asarray(X, dtype=np.float64)
        if X.ndim != 2 or X.shape[1] < 1:
            raise ArgumentError(capi.ERR_ARGUMENT, f"DimensionMismatch: X {X.shape}, expected (n_new, P_x)")
        self.X, self.n_new = np.asfortranarray(X), X.shape[0]
        self.factors = tuple(np.asarray(f.index if isinstance(f, Factor) else f) for f in (factors or ()))
        for k, idx in enumerate(self.factors):
            if idx.shape != (self.n_new,) or not np.issubdtype(idx.dtype, np.integer):
                raise ArgumentError(capi.ERR_ARGUMENT, f"DimensionMismatch: factor {k + 1} of the new data: an integer level per row, ({self.n_new},); got "
                                                       f"{idx.dtype} {idx.shape}")
        self.offset = None if offset is None else np.asfortranarray(np.asarray(offset, dtype=np.float64))
        if self.offset is not None and (self.offset.ndim not in (1, 2) or self.offset.shape[0] != self.n_new):
            raise ArgumentError(capi.ERR_ARGUMENT, f"DimensionMismatch: offset {self.offset.shape}, n_new {self.n_new}")
        self.y = None if y is None else np.asarray(y, dtype=np.float64).ravel()
        if self.y is not None and self.y.size != self.n_new:
            raise ArgumentError(capi.ERR_ARGUMENT, f"DimensionMismatch: y {self.y.shape}, n_new {self.n_new}")

    def __repr__(self):
        return f"GLMNewData(n_new={self.n_new}, factors={len(self.factors)}, offset={self.offset is not None}, y={self.y is not None})"


@dataclass(frozen=True)
class CoefGroup:
    """Coefficients [start, stop) of a HierGLMTarget that share a prior scale τ ~ half-normal(scale), itself sampled (as log τ).
    `centered`: the members are sampled on their own scale, β_d ~ N(0, τ²); otherwise standardised, β_d = τ·z_d with z_d ~ N(0, 1)
    (the non-centred parametrisation: what NUTS needs when the data say little about each member)."""
    start: int
    stop: int
    centered: bool = False
    scale: float = 1.0


class HierGLMTarget(GLMTarget):
    """A GLMTarget whose coefficient `groups` (CoefGroup, ascending and disjoint) each have a sampled prior scale
    (include/ahmc_glm_hier.h; arithmetic: glm.hier_logdensity).  θ has D = P + G entries: the P coefficient parameters (X.shape[1], and
    with `factors` their levels after them: a group may cover a factor's rows, `A.factor_ranges`),
    then log τ of each group.  `prior_scale` / `prior_prec` cover the coefficients in no group; on members they are forced to 0.
    `.coefficients(θ)` gives (β, τ) on the model's own scale.  HIP engine only."""

    def __init__(self, X, y, groups, family="bernoulli_logit", prior_scale=None, prior_prec=None, offset=None, scale=1.0, aux_prior=None, factors=None,
                 n_categories=None, cut_prior=None):
        super().__init__(X, y, family=family, prior_scale=prior_scale, prior_prec=prior_prec, offset=offset, scale=scale, aux_prior=aux_prior,
                         factors=factors, n_categories=n_categories, cut_prior=cut_prior)
        groups = [g if isinstance(g, CoefGroup) else CoefGroup(*g) for g in groups]
        try:
            if self.n_classes:
                _glm.check_class_groups(groups, self.P_b, self.n_classes - 1)
            else:
                _glm.check_groups(groups, self.P)
        except (ValueError, TypeError) as e:
            raise ArgumentError(capi.ERR_ARGUMENT, str(e))
        self.groups = tuple(CoefGroup(int(g.start), int(g.stop), bool(g.centered), float(g.scale)) for g in groups)
        self.D = self.P + len(self.groups) + (1 if self.aux else 0) + self._n_cut
        if self.prior_prec is not None:
            self.prior_prec = self.prior_prec.copy()
            for g in self.groups:
                self.prior_prec[g.start:g.stop] = 0.0

    def coefficients(self, theta):
        """(β (P, n), τ (G, n)) of draws θ (D, n) by the numpy mirror"""
        th = np.asarray(theta, dtype=np.float64)
        return _glm.hier_coefficients(th[:th.shape[0] - self._n_cut - (1 if self.aux else 0)], self.P, self.groups)

    def __repr__(self):
        return f"HierGLMTarget(n_obs={self.n_obs}, P={self.P}, groups={len(self.groups)}, family={self.family})"


@dataclass
class Hamiltonian:
    """src/hamiltonian.jl:1-20 (GaussianKinetic only, :18-20)"""
    metric: AbstractMetric
    target: object

    def __post_init__(self):
        if self.metric.size[0] != self.target.D:
            raise ArgumentError(capi.ERR_ARGUMENT, f"metric dimension {self.metric.size[0]} != target dimension {self.target.D}")


# ------------------------------------------------------------------------------------------------
# integrators (src/integrator.jl:71-209)
# ------------------------------------------------------------------------------------------------
class AbstractLeapfrog:
    kind = capi.INTEGRATOR_LEAPFROG
    param = 0.0

    def nom_step_size(self):
        return self.eps


class Leapfrog(AbstractLeapfrog):
    """src/integrator.jl:71-74; ϵ scalar or per-chain vector"""

    def __init__(self, eps):
        self.eps = np.asarray(eps, dtype=np.float64) if np.ndim(eps) else float(eps)


class JitteredLeapfrog(AbstractLeapfrog):
    """src/integrator.jl:112-156"""
    kind = capi.INTEGRATOR_JITTERED

    def __init__(self, eps0, jitter):
        self.eps = np.asarray(eps0, dtype=np.float64) if np.ndim(eps0) else float(eps0)
        self.param = float(jitter)


class TemperedLeapfrog(AbstractLeapfrog):
    """src/integrator.jl:174-209"""
    kind = capi.INTEGRATOR_TEMPERED

    def __init__(self, eps, alpha):
        self.eps = np.asarray(eps, dtype=np.float64) if np.ndim(eps) else float(eps)
        self.param = float(alpha)


# ------------------------------------------------------------------------------------------------
# trajectories / kernels (src/trajectory.jl:62-254, :414-449)
# ------------------------------------------------------------------------------------------------
class EndPointTS:
    code = capi.TS_ENDPOINT


class MultinomialTS:
    code = capi.TS_MULTINOMIAL


class SliceTS:
    code = capi.TS_SLICE


@dataclass
class FixedNSteps:
    L: int


@dataclass
class FixedIntegrationTime:
    lam: float


@dataclass
class ClassicNoUTurn:
    max_depth: int = 10
    delta_max: float = 1000.0
    code = capi.TC_CLASSIC


@dataclass
class GeneralisedNoUTurn:
    max_depth: int = 10
    delta_max: float = 1000.0
    code = capi.TC_GENERALISED


@dataclass
class StrictGeneralisedNoUTurn:
    max_depth: int = 10
    delta_max: float = 1000.0
    code = capi.TC_STRICT


_DYNAMIC = (ClassicNoUTurn, GeneralisedNoUTurn, StrictGeneralisedNoUTurn)


@dataclass
class Trajectory:
    """`Trajectory{TS}(integrator, termination_criterion)` (src/trajectory.jl:213-224)"""
    TS: type
    integrator: AbstractLeapfrog
    termination_criterion: object


class FullMomentumRefreshment:
    alpha = 0.0


@dataclass
class PartialMomentumRefreshment:
    alpha: float


class HMCKernel:
    """src/trajectory.jl:249-254"""

    def __init__(self, *args):
        if len(args) == 1:
            self.refreshment, self.tau = FullMomentumRefreshment(), args[0]
        else:
            self.refreshment, self.tau = args

    def cfg(self) -> capi.KernelCfg:
        tc = self.tau.termination_criterion
        k = capi.KernelCfg()
        k.sampler = self.tau.TS.code
        k.refresh_alpha = float(self.refreshment.alpha)
        if isinstance(tc, _DYNAMIC):
            k.nuts, k.criterion, k.max_depth, k.delta_max = 1, tc.code, tc.max_depth, tc.delta_max
        elif isinstance(tc, FixedNSteps):
            k.nuts, k.L, k.lambda_ = 0, tc.L, 0.0
        elif isinstance(tc, FixedIntegrationTime):
            k.nuts, k.L, k.lambda_ = 0, 0, tc.lam
        else:
            raise ArgumentError(capi.ERR_ARGUMENT, f"unknown termination criterion {tc!r}")
        return k


# ------------------------------------------------------------------------------------------------
# adaptors (src/adaptation/*.jl)
# ------------------------------------------------------------------------------------------------
class NoAdaptation:
    code = capi.ADAPT_NONE
    delta = 0.8


@dataclass
class StepSizeAdaptor:
    """StepSizeAdaptor(δ, integrator | ϵ) → NesterovDualAveraging (src/AdvancedHMC.jl:105-110)"""
    delta: float
    integrator: object = None
    code = capi.ADAPT_STEPSIZE


@dataclass
class MassMatrixAdaptor:
    """MassMatrixAdaptor(metric) → UnitMassMatrix / WelfordVar (src/AdvancedHMC.jl:112-118)"""
    metric: AbstractMetric
    code = capi.ADAPT_MASSMATRIX
    delta = 0.8
    estimator = 0  # AHMC_VAR_WELFORD


class PooledVar(MassMatrixAdaptor):
    """One (D,) M⁻¹ shared by all chains, estimated from all of them — and from all GPUs once the engine has a
    communicator (include/ahmc_hip.h AHMC_VAR_POOLED).  The reference has no counterpart: in
    matrix mode it resizes WelfordVar to one estimator per chain (src/adaptation/massmatrix.jl:103-121)."""
    estimator = 2  # AHMC_VAR_POOLED


class NutpieVar(MassMatrixAdaptor):
    """NutpieVar(size) (src/adaptation/massmatrix.jl:160-250): the nutpie-style diagonal estimator
    M⁻¹ = sqrt(var θ / var ∇ℓπ); a drop-in for the WelfordVar behind MassMatrixAdaptor(DiagEuclideanMetric),
    e.g. StanHMCAdaptor(NutpieVar(metric), StepSizeAdaptor(δ, lf)) (test/adaptation.jl:141-143)"""
    estimator = 1  # AHMC_VAR_NUTPIE


class LowRankVar(MassMatrixAdaptor):
    """LowRankVar(D | metric, rank, oversample=8, seed=0): the estimator of RankUpdateEuclideanMetric — M⁻¹ = Diagonal(A) + B·Dm·Bᵀ
    of rank `rank`, one for all chains, fitted to the draws of all of them (include/ahmc_lowrank_adapt.h; the arithmetic:
    rank_update.lowrank_*).  The reference has no adaptor for this metric.  Usable alone or as the `pc` of NaiveHMCAdaptor /
    StanHMCAdaptor; the engine's metric may be Unit, a shared (D,) Diag or a rank update of rank <= `rank`, and becomes a rank
    update of rank `rank` when the adaptor is set up."""
    lowrank = True

    def __init__(self, metric, rank, oversample=8, seed=0):
        if not isinstance(metric, AbstractMetric):
            metric = RankUpdateEuclideanMetric(int(metric))
        super().__init__(metric)
        self.rank, self.oversample, self.seed = int(rank), int(oversample), int(seed)


@dataclass
class NaiveHMCAdaptor:
    """src/adaptation/Adaptation.jl:41-64"""
    pc: MassMatrixAdaptor
    ssa: StepSizeAdaptor
    code = capi.ADAPT_NAIVE

    @property
    def delta(self):
        return self.ssa.delta


@dataclass
class StanHMCAdaptor:
    """src/adaptation/stan_adaptor.jl:52-103"""
    pc: MassMatrixAdaptor
    ssa: StepSizeAdaptor
    init_buffer: int = 75
    term_buffer: int = 50
    window_size: int = 25
    code = capi.ADAPT_STAN

    @property
    def delta(self):
        return self.ssa.delta


def stan_windows(n_adapts, init_buffer=75, term_buffer=50, window_size=25, lib: Optional[capi.CLib] = None):
    """initialize!(::StanHMCAdaptorState, ...) (src/adaptation/stan_adaptor.jl:13-50).
    Returns (window_start, window_end, window_splits)."""
    lib = lib or capi.load_hip_library()
    ws, we, ns = C.c_int64(), C.c_int64(), C.c_int32()
    splits = (C.c_int64 * 64)()
    lib.check(lib.dll.ahmc_stan_windows(init_buffer, term_buffer, window_size, n_adapts, C.byref(ws), C.byref(we),
                                        splits, 64, C.byref(ns)))
    return ws.value, we.value, [splits[i] for i in range(ns.value)]


# ------------------------------------------------------------------------------------------------
# phase point / transition carriers (src/hamiltonian.jl:88-107, src/trajectory.jl:18-23)
# ------------------------------------------------------------------------------------------------
@dataclass
class DualValue:
    value: np.ndarray
    gradient: np.ndarray


@dataclass
class PhasePoint:
    theta: np.ndarray
    r: np.ndarray
    lp: DualValue  # ℓπ: value = log density, gradient = -∇ℓπ (src/hamiltonian.jl:45-48)
    lk: DualValue  # ℓκ: value = -K(r); gradient (∂H∂r) is recomputed on demand


@dataclass
class Transition:
    z: PhasePoint
    stat: dict = field(default_factory=dict)


def neg_energy(z: PhasePoint):
    return z.lp.value + z.lk.value


def energy(z: PhasePoint):
    return -neg_energy(z)


# ------------------------------------------------------------------------------------------------
# Engine: one C context
# ------------------------------------------------------------------------------------------------
class Engine:
    """Binds a Hamiltonian and N chains to one `ahmc_ctx`.

    `lib=None` opens the HIP engine (and fails if it is not built).  `stream` is an optional
    hipStream_t (e.g. `torch.cuda.Stream().cuda_stream`) for HIP-event timing."""

    def __init__(self, h: Hamiltonian, n_chains: int, dtype=np.float64, rng=0, lib: Optional[capi.CLib] = None,
                 device: int = 0, stream: int = 0):
        self.lib = lib or capi.load_hip_library()
        self.h = h
        self.D, self.N = int(h.target.D), int(n_chains)
        self.dtype = np.dtype(dtype)
        self._ctx = C.c_void_p()
        self.lib.check(self.lib.dll.ahmc_create(device, capi.dtype_code(self.dtype), self.D, self.N,
                                                C.c_void_p(stream or None), C.byref(self._ctx)))
        self._external = isinstance(h.target, ExternalTarget)
        self.set_target(h.target)
        self.set_metric(h.metric)
        self.seed(rng)

    # -- plumbing --
    def _call(self, name, *args):
        self.lib.check(getattr(self.lib.dll, name)(self._ctx, *args), self._ctx)

    def close(self):
        if self._ctx:
            self.lib.dll.ahmc_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _mat(self, a, name):
        a = np.asarray(a)
        if a.ndim == 1:
            a = a.reshape(-1, 1)
        if a.shape != (self.D, self.N):
            raise ArgumentError(capi.ERR_ARGUMENT, f"{name} has size {a.shape}, expected {(self.D, self.N)}")
        return np.asfortranarray(a, dtype=self.dtype)

    def _out(self, vec=False):
        return np.empty((self.N,) if vec else (self.D, self.N), dtype=self.dtype, order="F")

    def _shape_out(self, a):
        return a[:, 0].copy() if (self.N == 1 and getattr(self, "_vector_mode", False)) else a

    # -- configuration --
    def set_target(self, target):
        p = None if target.params is None else np.ascontiguousarray(target.params, dtype=self.dtype)
        if isinstance(target, (PluginTarget, ObjectTarget)) and self.info("wide"):
            # (refused before anything is compiled: a plugin is built for ONE fused geometry, and a wide context has none)
            self._call("ahmc_set_target_plugin", b"", None, 0)
        if isinstance(target, PluginTarget):
            from .build import build_target_plugin

            so = build_target_plugin(target.source, self.dtype, self.info("group_lanes"), self.info("elems_per_lane"))
            self._call("ahmc_set_target_plugin", so.encode(), capi.as_ptr(p), 0 if p is None else p.size)
            return
        if isinstance(target, ObjectTarget):
            from .build import build_target_plugin_from_object

            so = build_target_plugin_from_object(target.object, self.dtype, self.info("group_lanes"), self.info("elems_per_lane"),
                                                 n_params=-1 if p is None else p.size)
            self._call("ahmc_set_target_plugin", so.encode(), capi.as_ptr(p), 0 if p is None else p.size)
            return
        self._glm_target = None
        if isinstance(target, GLMTarget):
            self._set_glm(target)
            self._glm_target = target   # (glm_yrep(newdata=None): the target's own rows)
            return
        if isinstance(target, KernelTarget):
            h = target.handle
            self._kernel_keepalive = (h, target.user)  # (a ctypes callback must outlive the context's use of it)
            hp = C.cast(h, C.c_void_p) if not isinstance(h, (int, C.c_void_p)) else (C.c_void_p(h) if isinstance(h, int) else h)
            up = target.user if isinstance(target.user, C.c_void_p) else C.c_void_p(target.user)
            self._call("ahmc_set_target_kernel", int(target.handle_kind), hp, int(target.block_threads), int(target.chains_per_block), up)
            return
        self._call("ahmc_set_target", target.kind, capi.as_ptr(p), 0 if p is None else p.size)

    def _need(self, flag, header, what):
        if not getattr(self.lib, flag, False):
            raise capi.UnsupportedError(capi.ERR_UNSUPPORTED, f"{what}: {self.lib.path} does not implement include/{header}")

    def _set_glm(self, t):
        """bind a GLMTarget through the entry point of its kind: a sampled dispersion first, then coefficient groups, then the plain model"""
        hier, G, F = isinstance(t, HierGLMTarget), len(t.groups), len(t.factors)
        if F:
            self._need("has_glm_factor", "ahmc_glm_factor.h", f"{type(t).__name__}(factors=…)")
        if t.n_categories:
            self._need("has_glm_ordinal", "ahmc_glm_ordinal.h", f"{type(t).__name__}(family=\"ordered_logit\")")
            model = f"the model has P + G + (C - 1) = {t.P} + {G} + {t.n_categories - 1} parameters"
        elif t.n_classes:
            self._need("has_glm_categorical", "ahmc_glm_categorical.h", f"{type(t).__name__}(family=\"categorical_logit\")")
            model = f"the model has (C - 1)·P_b + G = {t.n_classes - 1}·{t.P_b} + {G} parameters"
        elif t.aux:
            self._need("has_glm_aux", "ahmc_glm_aux.h", f"GLMTarget(family={t.family})")
            model = f"the model has P + G + 1 = {t.P} + {G} + 1 parameters"
        elif hier:
            self._need("has_hglm", "ahmc_glm_hier.h", "HierGLMTarget")
            model = f"the model has P + G = {t.P} + {G} parameters"
        else:
            self._need("has_glm", "ahmc_glm.h", "GLMTarget")
            model = f"X has {t.D} columns"
        if t.D != self.D:
            raise ArgumentError(capi.ERR_ARGUMENT, f"DimensionMismatch: {model}, the context has D = {self.D}")
        X = np.asfortranarray(t.X, dtype=self.dtype)
        y = np.ascontiguousarray(t.y, dtype=self.dtype)
        off = None if t.offset is None else np.asfortranarray(t.offset, dtype=self.dtype)   # ((n_obs, K) column-major of a categorical model)
        p = None if t.prior_prec is None else np.ascontiguousarray(t.prior_prec, dtype=self.dtype)
        data = (capi.as_ptr(X), capi.as_ptr(y), capi.as_ptr(off), capi.as_ptr(p))
        table = (G, (C.c_int32 * max(G, 1))(*[g.start for g in t.groups]), (C.c_int32 * max(G, 1))(*[g.stop for g in t.groups]),
                 (C.c_int32 * max(G, 1))(*[int(g.centered) for g in t.groups]), (C.c_double * max(G, 1))(*[g.scale for g in t.groups]))
        lev = np.asfortranarray(np.column_stack([f.index for f in t.factors]), dtype=np.int32) if F else None
        factors = (F, (C.c_int32 * F)(*[f.n_levels for f in t.factors]) if F else None, lev.ctypes.data_as(C.POINTER(C.c_int32)) if F else None)
        aux = tuple(float(v) for v in t.aux_prior) if t.aux else (0.0, 1.0)
        n_obs, Px, P = int(t.n_obs), int(t.P_x), int(t.P)
        if t.n_categories:
            call = ("ahmc_glm_ordinal_set_target", n_obs, Px, *data, *table, *factors, int(t.n_categories), (C.c_double * 4)(*t.cut_prior))
        elif t.n_classes:
            call = ("ahmc_glm_categorical_set_target", n_obs, Px, *data, *table, *factors, int(t.n_classes))
        elif F:
            call = ("ahmc_glm_factor_set_target", int(t.family), n_obs, Px, *data, float(t.scale), *table, *factors, int(t.aux), *aux)
        elif t.aux:
            call = ("ahmc_glm_aux_set_target", int(t.family), n_obs, P, *data, *table, *aux)
        elif hier:
            call = ("ahmc_hglm_set_target", int(t.family), n_obs, P, *data, float(t.scale), *table)
        else:
            call = ("ahmc_set_target_glm", int(t.family), n_obs, *data, float(t.scale))
        self._call(*call)

    def _draws(self, who, theta, n_cols):
        """(pointer, n) of draws θ (D, n): an array (default: the context's current θ), or a device pointer (an int) together with `n_cols`"""
        if isinstance(theta, (int, C.c_void_p)):
            if n_cols is None:
                raise ArgumentError(capi.ERR_ARGUMENT, f"{who}: a pointer needs n_cols")
            return (C.c_void_p(theta) if isinstance(theta, int) else theta), int(n_cols)
        th = np.asarray(self.theta() if theta is None else theta)
        if th.ndim == 1:
            th = th.reshape(-1, 1)
        if th.ndim != 2 or th.shape[0] != self.D or (n_cols is not None and n_cols != th.shape[1]):
            raise ArgumentError(capi.ERR_ARGUMENT, f"DimensionMismatch: θ {th.shape}, expected ({self.D}, {n_cols if n_cols is not None else 'n'})")
        return capi.as_ptr(np.asfortranarray(th, dtype=self.dtype)), th.shape[1]   # (the pointer owns the array)

    def _glm_get(self, getter, ctype, pos, n_args):
        """one value of the bound GLM: argument `pos` of the `n_args` outputs of an ahmc_*_get_target call (the others NULL)"""
        v = ctype()
        self._call(getter, *[C.byref(v) if i == pos else None for i in range(n_args)])
        return v.value

    def _on_draws(self, flag, header, entry, draws, n_cols, lead):
        """the post-processing entry points that take draws θ (D, n) — an array (default: the context's current θ), or a device
        pointer (an int) together with `n_cols`: check the feature flag, ask the bound model for the outputs' leading axes
        (`lead()`: one tuple per output), resolve the draws, allocate the outputs (…, n) and call `ahmc_<entry>`"""
        self._need(flag, header, entry)
        shapes = lead()
        ptr, n = self._draws(entry, draws, n_cols)
        outs = [np.empty((*sh, n), dtype=self.dtype, order="F") for sh in shapes]
        self._call("ahmc_" + entry, ptr, n, *[capi.as_ptr(o) if o.size else None for o in outs])
        return outs

    def glm_dispersion(self, theta=None, n_cols=None):
        """σ or φ = exp(s) (n_cols,) of draws θ (D, n_cols) — an array (default: the context's current θ), or a device pointer (an
        int) together with `n_cols`: ahmc_glm_dispersion"""
        return self._on_draws("has_glm_aux", "ahmc_glm_aux.h", "glm_dispersion", theta, n_cols, lambda: [()])[0]

    def _glm_n_obs(self):
        return self._glm_get("ahmc_get_target_glm", C.c_int64, 1, 3)

    def glm_cutpoints(self, draws=None, n_cols=None):
        """the cutpoints c (C − 1, n) of draws θ (D, n) of the bound ordinal model — an array (default: the context's current θ), or a
        device pointer (an int) together with `n_cols`: ahmc_glm_cutpoints"""
        return self._on_draws("has_glm_ordinal", "ahmc_glm_ordinal.h", "glm_cutpoints", draws, n_cols,
                              lambda: [(self._glm_get("ahmc_glm_ordinal_get_target", C.c_int32, 0, 2) - 1,)])[0]

    def glm_class_probs(self, draws=None, n_cols=None):
        """the class probabilities (C, n_obs, n) of every observation at draws θ (D, n) of the bound categorical model — an array
        (default: the context's current θ), or a device pointer (an int) together with `n_cols`: ahmc_glm_class_probs"""
        return self._on_draws("has_glm_categorical", "ahmc_glm_categorical.h", "glm_class_probs", draws, n_cols,
                              lambda: [(self._glm_get("ahmc_glm_categorical_get_target", C.c_int32, 0, 2), self._glm_n_obs())])[0]

    def glm_loglik(self, draws=None, n_cols=None):
        """ℓ(y_i, η_i) (n_obs, n) of every observation at draws θ (D, n) of the bound GLM — an array (default: the context's current θ),
        or a device pointer (an int) together with `n_cols`; the (D, N, K) buffer of `run(samples_out=ptr)` is passed with
        n_cols = N·K: ahmc_glm_loglik"""
        return self._on_draws("has_glm_loo", "ahmc_glm_loo.h", "glm_loglik", draws, n_cols, lambda: [(self._glm_n_obs(),)])[0]

    def glm_loo(self, draws=None, n_cols=None, log_weights=False):
        """PSIS-LOO and WAIC of the bound GLM over draws θ (D, n), passed as to `glm_loglik`: {"elpd_loo", "pareto_k", "lpd", "p_waic"},
        each (n_obs,) float64, and with `log_weights` the normalised "log_weights" (n, n_obs) in the draws' order — what glm.psis_loo
        returns for the same ℓ (glm.loo_summary and glm.loo_compare take either): ahmc_glm_loo"""
        self._need("has_glm_loo", "ahmc_glm_loo.h", "glm_loo")
        n_obs = self._glm_n_obs()
        ptr, n = self._draws("glm_loo", draws, n_cols)
        pw = np.full((4, n_obs), np.nan, order="F")
        lw = np.empty((n, n_obs), order="F") if log_weights else None
        pd = C.POINTER(C.c_double)
        self._call("ahmc_glm_loo", ptr, n, pw.ctypes.data_as(pd) if n else None, lw.ctypes.data_as(pd) if (log_weights and n) else None)
        out = {k: pw[q].copy() for q, k in enumerate(("elpd_loo", "pareto_k", "lpd", "p_waic"))}
        if log_weights:
            out["log_weights"] = lw
        return out

    def _glm_newdata(self, who, nd):
        """(record, keep-alive arrays) of a GLMNewData in the context's element type: struct ahmc_glm_newdata"""
        self._need("has_glm_predict", "ahmc_glm_predict.h", who)
        if not isinstance(nd, GLMNewData):
            raise ArgumentError(capi.ERR_ARGUMENT, f"{who}: newdata must be a GLMNewData, not {type(nd).__name__}")
        X = np.asfortranarray(nd.X, dtype=self.dtype)
        lev = np.asfortranarray(np.column_stack(nd.factors), dtype=np.int32) if nd.factors else None
        off = None if nd.offset is None else np.asfortranarray(nd.offset, dtype=self.dtype)
        y = None if nd.y is None else np.ascontiguousarray(nd.y, dtype=self.dtype)
        rec = capi.GLMNewDataRecord(nd.n_new, capi.as_ptr(X), None if lev is None else lev.ctypes.data_as(C.POINTER(C.c_int32)), capi.as_ptr(off), capi.as_ptr(y))
        return rec, (X, lev, off, y)

    def _glm_quantities(self):
        """(K predictors, C categories or classes — 0 for the families with one mean) of the bound GLM"""
        fam = self._glm_get("ahmc_get_target_glm", C.c_int32, 0, 3)
        if fam == _glm.CATEGORICAL_LOGIT:
            Ccl = self._glm_get("ahmc_glm_categorical_get_target", C.c_int32, 0, 2)
            return Ccl - 1, Ccl
        if fam == _glm.ORDERED_LOGIT:
            return 1, self._glm_get("ahmc_glm_ordinal_get_target", C.c_int32, 0, 2)
        return 1, 0

    def glm_predict(self, newdata, draws=None, n_cols=None, what="mean"):
        """`what` of the bound GLM at the rows of `newdata` (a GLMNewData) and draws θ (D, n), passed as to `glm_loglik`: "linear" η
        (n_new, n) — (K, n_new, n) of a categorical model; "mean" μ (n_new, n), or the probabilities (C, n_new, n) of an ordinal or a
        categorical model; "variance" (n_new, n); "loglik" ℓ(y_new, η) (n_new, n): ahmc_glm_predict.  The matrix is written whole:
        for the S = N·K draws of a run use `glm_predict_summary`."""
        rec, keep = self._glm_newdata("glm_predict", newdata)
        if what not in capi.GLM_PRED_WHAT:
            raise ArgumentError(capi.ERR_ARGUMENT, f"glm_predict: what = {what!r}; one of {sorted(capi.GLM_PRED_WHAT)}")
        K, Ccl = self._glm_quantities()
        planes = {"linear": K, "mean": Ccl or 1}.get(what, 1)
        ptr, n = self._draws("glm_predict", draws, n_cols)
        out = np.empty((planes, newdata.n_new, n), dtype=self.dtype, order="F")
        self._call("ahmc_glm_predict", C.byref(rec), ptr, n, capi.GLM_PRED_WHAT[what], capi.as_ptr(out) if out.size else None)
        del keep
        return out if (what == "linear" and K > 1) or (what == "mean" and Ccl) else out[0]

    def glm_predict_summary(self, newdata, draws=None, n_cols=None):
        """per new observation, over draws θ (D, n) passed as to `glm_loglik` — the (D, N, K) buffer of `run(samples_out=ptr)` with
        n_cols = N·K — the posterior mean and variance of every predicted quantity and the log predictive density at `newdata.y`, with
        the draws reduced on the device (the (n_new, n) matrix is never written): ahmc_glm_predict_summary.  A dict of float64 arrays:
        "eta_mean", "eta_var", "mean", "mean_var", "var_within" (the mean over the draws of Var[y | θ]) and "lpd", each (n_new,), for the
        families with one mean; "eta_mean", "eta_var" ((K, n_new) of a categorical model), "probs", "probs_var" (C, n_new) and "lpd"
        otherwise.  lpd is NaN without `newdata.y`; the variances are NaN for a single draw."""
        rec, keep = self._glm_newdata("glm_predict_summary", newdata)
        K, Ccl = self._glm_quantities()
        Q = K + (Ccl or 2)
        ptr, n = self._draws("glm_predict_summary", draws, n_cols)
        s = np.full((2 * Q + 1, newdata.n_new), np.nan, order="F")
        self._call("ahmc_glm_predict_summary", C.byref(rec), ptr, n, s.ctypes.data_as(C.POINTER(C.c_double)) if (n and s.size) else None)
        del keep
        return glm_summary_dict(s, K, Ccl)

    def _glm_yrep_newdata(self, who, newdata):
        self._need("has_glm_yrep", "ahmc_glm_yrep.h", who)
        if newdata is None:
            t = getattr(self, "_glm_target", None)
            if t is None:
                raise ArgumentError(capi.ERR_ARGUMENT, f"{who}: newdata=None means the rows of the bound GLMTarget, and none was bound through set_target")
            newdata = GLMNewData(t.X, factors=[f.index for f in t.factors], offset=t.offset, y=t.y)
        return newdata, self._glm_newdata(who, newdata)

    def glm_yrep(self, newdata=None, draws=None, n_cols=None, seed=0):
        """posterior-predictive draws y_rep (n_new, n) of the bound GLM: one outcome y ~ p(y | θ_j) per row of `newdata` (a GLMNewData;
        None: the bound target's own rows) and draw θ_j of `draws` (D, n), passed as to `glm_loglik`: ahmc_glm_yrep.  Reproducible:
        element (i, j) depends on its row, its draw, (i, j) and `seed` alone (glm.yrep_at is the sampler's definition).  The matrix is
        written whole: for the S = N·K draws of a run use `glm_yrep_summary`."""
        nd, (rec, keep) = self._glm_yrep_newdata("glm_yrep", newdata)
        ptr, n = self._draws("glm_yrep", draws, n_cols)
        out = np.empty((nd.n_new, n), dtype=self.dtype, order="F")
        self._call("ahmc_glm_yrep", C.byref(rec), ptr, n, int(seed) & (2 ** 64 - 1), capi.as_ptr(out) if out.size else None)
        del keep
        return out

    def glm_yrep_summary(self, newdata=None, draws=None, n_cols=None, seed=0):
        """per row of `newdata` (None: the bound target's own rows), over draws θ (D, n) passed as to `glm_loglik` — the (D, N, K) buffer
        of `run(samples_out=ptr)` with n_cols = N·K — {"mean", "var", "p_less", "p_equal"}, each (n_new,) float64: the mean and the
        variance of the y_rep that `glm_yrep` gives for the same seed, and the shares of them below and at `newdata.y` (NaN without
        it), with the draws reduced on the device: ahmc_glm_yrep_summary"""
        nd, (rec, keep) = self._glm_yrep_newdata("glm_yrep_summary", newdata)
        ptr, n = self._draws("glm_yrep_summary", draws, n_cols)
        s = np.full((4, nd.n_new), np.nan, order="F")
        self._call("ahmc_glm_yrep_summary", C.byref(rec), ptr, n, int(seed) & (2 ** 64 - 1), s.ctypes.data_as(C.POINTER(C.c_double)) if (n and s.size) else None)
        del keep
        return {k: s[i].copy() for i, k in enumerate(("mean", "var", "p_less", "p_equal"))}

    def glm_yrep_at(self, family, q, aux=None, row=None, col=None, seed=0, n_categories=0):
        """y (n,) in the context's element type: one outcome per element from the family's sampler given its planes q (planes, n), the
        log-dispersion `aux` (n,) of a negative binomial and the counters `row`, `col` (n,) (None: 0 … n − 1 and 0): ahmc_glm_yrep_at,
        the device's form of glm.yrep_at.  No GLM need be bound."""
        self._need("has_glm_yrep", "ahmc_glm_yrep.h", "glm_yrep_at")
        fam = _glm._yrep_family(family)
        qa = np.asfortranarray(np.atleast_2d(np.asarray(q)), dtype=self.dtype)
        n = qa.shape[1]
        vec = lambda a, dt: None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a), (n,)), dtype=dt)  # noqa: E731
        au, ro, co = vec(aux, self.dtype), vec(row, np.int32), vec(col, np.int32)
        y = np.empty(n, dtype=self.dtype)
        pi = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
        self._call("ahmc_glm_yrep_at", int(fam), int(n_categories or 0), n, capi.as_ptr(qa) if n else None, capi.as_ptr(au), pi(ro), pi(co), int(seed) & (2 ** 64 - 1),
                   capi.as_ptr(y) if n else None)
        return y

    def hglm_coefficients(self, theta=None, n_cols=None):
        """(β (P, n_cols), τ (G, n_cols)) of draws θ (D, n_cols) — an array (default: the context's current θ), or a device pointer
        (an int) together with `n_cols`: ahmc_hglm_coefficients"""
        return tuple(self._on_draws("has_hglm", "ahmc_glm_hier.h", "hglm_coefficients", theta, n_cols,
                                    lambda: [(self._glm_get("ahmc_hglm_get_target", C.c_int64, 0, 6),), (self._glm_get("ahmc_hglm_get_target", C.c_int32, 1, 6),)]))

    def glm_factors(self):
        """(P_x, [n_levels of each factor]) of the bound GLM: ahmc_glm_factor_get_target"""
        self._need("has_glm_factor", "ahmc_glm_factor.h", "glm_factors")
        Px, F, L = C.c_int64(), C.c_int32(), (C.c_int32 * capi.GLM_FACTOR_MAX)()
        self._call("ahmc_glm_factor_get_target", C.byref(Px), C.byref(F), L)
        return Px.value, [int(L[f]) for f in range(F.value)]

    def glm_pointwise(self):
        """(η, ℓ(y_i, η_i)) at the context's current θ, each (n_obs, N): ahmc_glm_pointwise.  A categorical model has a predictor per
        non-reference class: η is then (K, n_obs, N), η[k − 1] being η_k"""
        self._need("has_glm", "ahmc_glm.h", "glm_pointwise")
        n, fam = C.c_int64(), C.c_int32()
        self._call("ahmc_get_target_glm", C.byref(fam), C.byref(n), None)
        K = 0
        if fam.value == capi.GLM_CATEGORICAL_LOGIT:
            nc = C.c_int32()
            self._call("ahmc_glm_categorical_get_target", C.byref(nc), None)
            K = nc.value - 1
        eta = np.empty((n.value, self.N * max(K, 1)), dtype=self.dtype, order="F")    # (K planes of (n_obs, N), plane after plane)
        ll = np.empty((n.value, self.N), dtype=self.dtype, order="F")
        self._call("ahmc_glm_pointwise", capi.as_ptr(eta), capi.as_ptr(ll))
        return (np.stack([eta[:, k * self.N:(k + 1) * self.N] for k in range(K)]) if K else eta), ll

    def _need_rank_update(self, what):
        if not getattr(self.lib, "has_rank_update", False):
            raise capi.UnsupportedError(capi.ERR_UNSUPPORTED, f"{what}: {self.lib.path} does not implement include/ahmc_rank_update.h")

    def _set_rank_update(self, A, B, Dm):
        self._need_rank_update("RankUpdateEuclideanMetric")
        A = np.ascontiguousarray(A, dtype=self.dtype).ravel()
        B = np.asfortranarray(B, dtype=self.dtype)
        Dm = np.asfortranarray(Dm, dtype=self.dtype)
        if A.size != self.D:
            raise ArgumentError(capi.ERR_ARGUMENT, f"AxesMismatch: A has {A.size} elements but r has first axis {self.D}")
        k = B.shape[1] if B.ndim == 2 else 0
        self._call("ahmc_set_metric_rank_update", capi.as_ptr(A), capi.as_ptr(B) if k else None, capi.as_ptr(Dm) if k else None, k)
        self.metric_kind = capi.METRIC_RANK_UPDATE

    def set_metric(self, metric):
        if metric.kind == capi.METRIC_RANK_UPDATE:
            self._set_rank_update(metric.A, metric.B, metric.D)
            return
        if metric.kind == capi.METRIC_UNIT:
            self._call("ahmc_set_metric", metric.kind, None, 0)
        else:
            M = np.asfortranarray(metric.Minv, dtype=self.dtype)
            if metric.kind == capi.METRIC_DIAG and M.shape[0] != self.D:
                raise ArgumentError(capi.ERR_ARGUMENT, f"AxesMismatch: M⁻¹ has size {M.shape} but r has first axis {self.D}")
            self._call("ahmc_set_metric", metric.kind, capi.as_ptr(M), M.size)
        self.metric_kind = metric.kind

    def get_metric_rank_update(self):
        """(A, B, D) of a RankUpdateEuclideanMetric as the context holds it (ahmc_get_metric_rank_update)"""
        self._need_rank_update("get_metric_rank_update")
        k = C.c_int64()
        self._call("ahmc_get_metric_rank_update", None, None, None, C.byref(k))
        A = np.empty(self.D, dtype=self.dtype)
        B = np.empty((self.D, k.value), dtype=self.dtype, order="F")
        Dm = np.empty((k.value, k.value), dtype=self.dtype, order="F")
        self._call("ahmc_get_metric_rank_update", capi.as_ptr(A), capi.as_ptr(B) if k.value else None, capi.as_ptr(Dm) if k.value else None, None)
        return A, B, Dm

    def get_metric(self):
        if self.metric_kind == capi.METRIC_UNIT:
            return None
        if self.metric_kind == capi.METRIC_RANK_UPDATE:
            return self.get_metric_rank_update()
        # size is whatever was set last (D, D*N or D*D): probe via a D*N then D buffer
        for shape in ((self.D, self.N), (self.D,), (self.D, self.D)):
            out = np.empty(shape, dtype=self.dtype, order="F")
            code = self.lib.dll.ahmc_get_metric(self._ctx, capi.as_ptr(out), out.size)
            if code == capi.OK:
                return out
        self.lib.check(code, self._ctx)

    def set_integrator(self, lf: AbstractLeapfrog):
        eps = np.atleast_1d(np.asarray(lf.eps, dtype=self.dtype))
        if eps.size not in (1, self.N):
            raise ArgumentError(capi.ERR_ARGUMENT, f"step size vector has length {eps.size}, expected 1 or {self.N}")
        self._call("ahmc_set_stepsize", capi.as_ptr(eps), eps.size)
        self._call("ahmc_set_integrator", lf.kind, float(lf.param))

    def get_stepsize(self):
        out = self._out(vec=True)
        self._call("ahmc_get_stepsize", capi.as_ptr(out))
        return out

    def seed(self, rng, iteration=None):
        spec, stride = _rng_spec(rng, self.N)
        self._call("ahmc_seed", spec.seed, spec.chain_offset, stride, spec.iteration if iteration is None else iteration)

    # -- phase point --
    def set_position(self, theta, r=None):
        """phasepoint(h, θ, r) (src/hamiltonian.jl:115-119)"""
        self._vector_mode = np.ndim(theta) == 1
        th = self._mat(theta, "θ")
        if self._external:
            lp, grad = self.h.target.fn(th)
            rr = self._mat(r, "r") if r is not None else np.zeros_like(th)
            # the converted arrays are bound to names: the C call reads them (as_ptr also keeps them alive)
            lp_a = np.ascontiguousarray(lp, dtype=self.dtype).reshape(self.N)
            g_a = self._mat(-np.asarray(grad), "∇ℓπ")
            self._call("ahmc_set_phasepoint", capi.as_ptr(th), capi.as_ptr(rr), capi.as_ptr(lp_a), capi.as_ptr(g_a))
            return
        rr = None if r is None else self._mat(r, "r")
        self._call("ahmc_set_position", capi.as_ptr(th), capi.as_ptr(rr))

    def phasepoint(self) -> PhasePoint:
        th, r, g = self._out(), self._out(), self._out()
        lp, lk = self._out(True), self._out(True)
        self._call("ahmc_get_phasepoint", capi.as_ptr(th), capi.as_ptr(r), capi.as_ptr(lp), capi.as_ptr(g), capi.as_ptr(lk))
        if self.N == 1 and getattr(self, "_vector_mode", False):
            return PhasePoint(th[:, 0], r[:, 0], DualValue(lp[0], g[:, 0]), DualValue(lk[0], None))
        return PhasePoint(th, r, DualValue(lp, g), DualValue(lk, None))

    def theta(self):
        th = self._out()
        self._call("ahmc_get_phasepoint", capi.as_ptr(th), None, None, None, None)
        return self._shape_out(th)

    def set_ref_compat(self, on=True):
        """the reference's matrix-mode early exit (src/integrator.jl:252-258: every chain stops at the first step after which ANY chain is
        non-finite) for `step` and static EndPointTS transitions — off by default (each chain stops at its own first non-finite point)"""
        self._call("ahmc_set_ref_compat", 1 if on else 0)

    def refresh(self, refreshment=None):
        """refresh(rng, refreshment, h, z) (src/hamiltonian.jl:213-254).  Does NOT advance the iteration: the transition that follows
        draws the same (chain, iteration, momentum) normals ξ again.  With FullMomentumRefreshment that merely repeats the draw; a
        transition with PartialMomentumRefreshment(α) after `refresh()` starts from r = (α + √(1 − α²))·ξ, variance 1.78·M at α = 0.9
        instead of M.  A stationary start for such a transition is `set_position(θ, r)` with r ~ N(0, M) drawn by the caller."""
        self._call("ahmc_refresh_momentum", float(getattr(refreshment, "alpha", 0.0)))

    def step(self, n_steps=1):
        """step(lf, h, z, n_steps) (src/integrator.jl:216-265)"""
        if self._external:
            n = abs(int(n_steps))
            fwd = 1 if n_steps > 0 else 0
            theta_view = self._out()
            for i in range(1, n + 1):
                self._call("ahmc_lf_pre", fwd, i, n)
                self._call("ahmc_get_phasepoint", capi.as_ptr(theta_view), None, None, None, None)
                lp, grad = self.h.target.fn(theta_view)
                lp_a = np.ascontiguousarray(lp, dtype=self.dtype).reshape(self.N)
                g_a = self._mat(-np.asarray(grad), "∇ℓπ")
                self._call("ahmc_lf_post", fwd, i, n, capi.as_ptr(lp_a), capi.as_ptr(g_a))
            return
        self._call("ahmc_leapfrog", int(n_steps))

    # -- transitions --
    def transition(self, kernel: HMCKernel):
        """transition(rng, h, κ, z) (src/sampler.jl:48-58)"""
        k = kernel.cfg()
        if self._external:
            self._call("ahmc_ext_begin", C.byref(k), 1)
            self._ext_drive()
            return
        if k.refresh_alpha != 0.0:
            # HMCKernel(PartialMomentumRefreshment(α), τ) (src/trajectory.jl:249-254, src/hamiltonian.jl:243-254): the refreshment is part of
            # the sample loop's kernel configuration at the boundary — ONE iteration of that loop is this transition (the iteration counter,
            # and with it every variate, continues as for the two calls below).  It is issued as iteration 2 of 2, i.e. as a RESUMED loop
            # (ahmc_sample_from with i_first > 1): nothing is reset, and the running accumulators COUNT the draw as a kept one — Σθ, Σθ²,
            # Σ n_steps, the energy sums and n_transitions of an earlier run() go on, +1 transition.  This differs from the full-refresh
            # transition below, which leaves the accumulators alone.  (i_first = 1 would be a loop's first kept iteration and clear them.
            # With n_adapts = 0 no other rule of i_first applies: nothing adapts, and the Stan adaptor's position check needs i_first <= n_adapts.)
            self._call("ahmc_sample_from", C.byref(k), 2, 2, 0, 0, None)
            return
        if k.nuts:
            self._call("ahmc_nuts_transition", k.max_depth, k.delta_max, k.criterion, k.sampler)
        else:
            self._call("ahmc_hmc_transition", k.L, k.lambda_, k.sampler)

    def stats(self, fields: Optional[Sequence[str]] = None) -> dict:
        out = {}
        for name in fields or capi.STAT_FIELDS:
            fid, is_int = capi.STAT_FIELDS[name]
            buf = np.empty(self.N, dtype=np.int32 if is_int else self.dtype)
            self._call("ahmc_get_stat", fid, capi.as_ptr(buf))
            out[name] = buf
        for b in ("is_accept", "numerical_error"):
            if b in out:
                out[b] = out[b].astype(bool)
        return out

    def find_good_stepsize(self, initial_step_size=0.1, max_n_iters=100):
        """find_good_stepsize(rng, h, θ) per chain (src/trajectory.jl:768-837)"""
        if self._external:
            self._call("ahmc_ext_find_good_stepsize_begin", float(initial_step_size), int(max_n_iters))
            self._ext_drive()
        else:
            self._call("ahmc_find_good_stepsize", float(initial_step_size), int(max_n_iters))
        return self.get_stepsize()

    # -- external target: the ask / tell loop (include/ahmc_hip.h, ahmc_ext_*) --
    def _ext_drive(self):
        """Serve the engine's evaluation requests with the user's `fn` until the run started by
        ahmc_ext_begin / ahmc_ext_find_good_stepsize_begin is complete.  Returns the number of
        round trips (= evaluations of `fn`)."""
        n = C.c_int64()
        chains = np.empty(self.N, dtype=np.int32)
        theta = self._out()
        lp_buf = np.zeros(self.N, dtype=self.dtype)
        g_buf = np.zeros((self.D, self.N), dtype=self.dtype, order="F")
        trips = 0
        try:
            while True:
                self._call("ahmc_ext_pending", C.byref(n), capi.as_ptr(chains), capi.as_ptr(theta))
                if n.value == 0:
                    return trips
                idx = chains[:n.value]
                if self.h.target.takes_chains:
                    lp, grad = self.h.target.fn(theta, idx)
                else:
                    lp, grad = self.h.target.fn(theta)
                lp_buf[idx] = np.asarray(lp, dtype=self.dtype).reshape(self.N)[idx]
                g_buf[:, idx] = -np.asarray(grad, dtype=self.dtype).reshape(self.D, self.N)[:, idx]
                self._call("ahmc_ext_advance", capi.as_ptr(lp_buf), capi.as_ptr(g_buf))
                trips += 1
        except BaseException:
            self.lib.dll.ahmc_ext_cancel(self._ctx)
            raise

    # -- adaptation --
    def adaptor_init(self, adaptor):
        ib, tb, ws = (getattr(adaptor, "init_buffer", 75), getattr(adaptor, "term_buffer", 50),
                      getattr(adaptor, "window_size", 25))
        pc = adaptor if isinstance(adaptor, MassMatrixAdaptor) else getattr(adaptor, "pc", None)
        self._call("ahmc_set_var_estimator", int(getattr(pc, "estimator", 0)))
        if getattr(pc, "lowrank", False):
            self._need_lowrank_adapt("LowRankVar")
            self._call("ahmc_lowrank_adaptor_init", adaptor.code, float(adaptor.delta), ib, tb, ws, pc.rank, pc.oversample, pc.seed)
            self.metric_kind = capi.METRIC_RANK_UPDATE
            return
        self._call("ahmc_adaptor_init", adaptor.code, float(adaptor.delta), ib, tb, ws)

    def _need_lowrank_adapt(self, what):
        if not getattr(self.lib, "has_lowrank_adapt", False):
            raise capi.UnsupportedError(capi.ERR_UNSUPPORTED, f"{what}: {self.lib.path} does not implement include/ahmc_lowrank_adapt.h")

    def lowrank_state(self):
        """the low-rank adaptor's state (ahmc_lowrank_get_state) as a dict of the header fields and the float64 arrays mu, m2 (D,),
        Z, Omega (D, ell), s0 (D,); None when the context has no such adaptor"""
        if not getattr(self.lib, "has_lowrank_adapt", False):
            return None
        st = capi.LowRankState()
        if self.lib.dll.ahmc_lowrank_get_state(self._ctx, C.byref(st), None, None, None, None, None) != capi.OK:
            return None
        D, L = self.D, int(st.ell)
        out = {"mu": np.empty(D), "m2": np.empty(D), "Z": np.empty((D, L), order="F"), "s0": np.empty(D), "Omega": np.empty((D, L), order="F")}
        self._call("ahmc_lowrank_get_state", C.byref(st), *(capi.as_ptr(out[k]) for k in ("mu", "m2", "Z", "s0", "Omega")))
        out.update({k: getattr(st, k) for k, _ in capi.LowRankState._fields_})
        return out

    def set_lowrank_state(self, state: dict):
        """ahmc_lowrank_set_state: the adaptor must have been set up with the same rank and oversampling"""
        self._need_lowrank_adapt("set_lowrank_state")
        st = capi.LowRankState(**{k: int(state[k]) for k, _ in capi.LowRankState._fields_})
        arrs = [np.asfortranarray(state[k], dtype=np.float64) for k in ("mu", "m2", "Z", "s0", "Omega")]
        self._call("ahmc_lowrank_set_state", C.byref(st), *(capi.as_ptr(a) for a in arrs))

    def adapt(self, i, n_adapts, theta=None, alpha=None, grad=None):
        """adapt!(h, κ, adaptor, i, n_adapts, z_or_θ, α) (src/sampler.jl:72-90); θ/α default to the
        context's position and the last transition's acceptance_rate; `grad` = z.ℓπ.gradient makes the
        argument a phase point (needed by NutpieVar, src/adaptation/massmatrix.jl:238-243)"""
        th = None if theta is None else self._mat(theta, "θ")
        al = None if alpha is None else np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, dtype=self.dtype), (self.N,)))
        if grad is None:
            self._call("ahmc_adapt", int(i), int(n_adapts), capi.as_ptr(th), capi.as_ptr(al))
        else:
            g = self._mat(grad, "∇")
            self._call("ahmc_adapt_point", int(i), int(n_adapts), capi.as_ptr(th), capi.as_ptr(g), capi.as_ptr(al))

    # -- bulk driver --
    def run(self, kernel: HMCKernel, n_samples, n_adapts=0, drop_warmup=False, samples_out=None, i_first=1):
        """The whole `sample` loop enqueued by one C call (no host synchronisation inside): iterations i_first …
        n_samples (i_first > 1 continues a checkpointed run, ahmc_sample_from).  With an ExternalTarget the loop runs
        here, one ask / tell transition + adapt! per iteration."""
        k = kernel.cfg()
        if self._external:
            if samples_out is not None:
                raise capi.UnsupportedError(capi.ERR_UNSUPPORTED, "samples_out with an ExternalTarget: use sample()")
            for i in range(int(i_first), int(n_samples) + 1):
                self.transition(kernel)
                self.adapt(i, int(n_adapts))
            return
        self._call("ahmc_sample_from", C.byref(k), int(i_first), int(n_samples), int(n_adapts), 1 if drop_warmup else 0,
                   capi.as_ptr(samples_out))

    def sync(self):
        self._call("ahmc_sync")

    # -- checkpoint / resume (HMCState, src/abstractmcmc.jl:11-27) --
    def get_state(self) -> dict:
        """Everything a resumed run needs: the phase point, h's metric, κ's nominal step sizes, the adaptor, the RNG
        counter.  `Engine.set_state` on a fresh engine of the same Hamiltonian continues the run bit for bit."""
        st = capi.AdaptorState()
        self._call("ahmc_get_adaptor_state", C.byref(st), None, None)
        da = np.empty((5, self.N), dtype=self.dtype) if st.has_da else None
        wv = np.empty((st.n_welford, self.N, self.D), dtype=self.dtype) if st.n_welford else None  # C-order view of (n, D, N) column-major
        self._call("ahmc_get_adaptor_state", C.byref(st), capi.as_ptr(da), capi.as_ptr(wv))
        z = self.phasepoint() if not getattr(self, "_vector_mode", False) else None
        if z is None:
            self._vector_mode = False
            z = self.phasepoint()
            self._vector_mode = True
        ntr = C.c_int64()
        acc = {"n_steps": np.empty(self.N, dtype=np.int64), "n_divergent": np.empty(self.N, dtype=np.int64),
               "sum_theta": np.empty((self.N, self.D), dtype=self.dtype), "sumsq_theta": np.empty((self.N, self.D), dtype=self.dtype),
               "energy_sums": np.empty((5, self.N), dtype=self.dtype)}
        self._call("ahmc_get_accum_state", C.byref(ntr), capi.as_ptr(acc["n_steps"]), capi.as_ptr(acc["n_divergent"]), capi.as_ptr(acc["sum_theta"]),
                   capi.as_ptr(acc["sumsq_theta"]), capi.as_ptr(acc["energy_sums"]))
        acc["n_transitions"] = ntr.value
        return {"adaptor": {k: getattr(st, k) for k, _ in capi.AdaptorState._fields_}, "da": da, "welford": wv,
                "theta": z.theta, "r": z.r, "lp": z.lp.value, "grad": z.lp.gradient,
                "metric": self.get_metric(), "metric_kind": self.metric_kind, "stepsize": self.get_stepsize(),
                "stepsize_scalar": bool(self.info("stepsize_scalar")), "accum": acc, "lowrank": self.lowrank_state()}

    def set_state(self, state: dict):
        lr = state.get("lowrank")
        if lr is not None and state["adaptor"]["kind"] in (capi.ADAPT_MASSMATRIX, capi.ADAPT_NAIVE, capi.ADAPT_STAN):  # the low-rank adaptor first: it shapes the metric and the estimator, the saved values then overwrite both
            ad = state["adaptor"]
            self._need_lowrank_adapt("set_state")
            self._call("ahmc_lowrank_adaptor_init", int(ad["kind"]), float(ad["delta"]), int(ad["init_buffer"]), int(ad["term_buffer"]),
                       int(ad["window_size"]), int(lr["k"]), int(lr["ell"]) - int(lr["k"]), int(lr["seed"]))
            self.set_lowrank_state(lr)
        if state.get("metric_kind") == capi.METRIC_RANK_UPDATE:  # (A, B, D)
            self._set_rank_update(*state["metric"])
        elif state["metric"] is not None:
            self._call("ahmc_set_metric", state["metric_kind"], capi.as_ptr(np.asfortranarray(state["metric"], dtype=self.dtype)), state["metric"].size)
        eps = np.ascontiguousarray(state["stepsize"], dtype=self.dtype)
        if state.get("stepsize_scalar"):   # ONE nominal ϵ stays one (κ's integrator is restored as it was: FixedIntegrationTime needs it, Q6)
            eps = eps[:1].copy()
        self._call("ahmc_set_stepsize", capi.as_ptr(eps), eps.size)
        th, r = self._mat(state["theta"], "θ"), self._mat(state["r"], "r")
        lp = np.ascontiguousarray(state["lp"], dtype=self.dtype).reshape(self.N)
        g = self._mat(state["grad"], "∇ℓπ")
        self._call("ahmc_set_phasepoint", capi.as_ptr(th), capi.as_ptr(r), capi.as_ptr(lp), capi.as_ptr(g))
        st = capi.AdaptorState(**state["adaptor"])
        self._call("ahmc_set_adaptor_state", C.byref(st), capi.as_ptr(state["da"]), capi.as_ptr(state["welford"]))
        acc = state.get("accum")
        if acc is not None:  # the running accumulators (Σθ, Σθ², Σ n_steps, the energy sums of EBFMI) are part of the checkpoint
            cont = lambda a, dt: np.ascontiguousarray(a, dtype=dt)  # noqa: E731
            self._call("ahmc_set_accum_state", int(acc["n_transitions"]), capi.as_ptr(cont(acc["n_steps"], np.int64)),
                       capi.as_ptr(cont(acc["n_divergent"], np.int64)), capi.as_ptr(cont(acc["sum_theta"], self.dtype)),
                       capi.as_ptr(cont(acc["sumsq_theta"], self.dtype)), capi.as_ptr(cont(acc["energy_sums"], self.dtype)))

    # -- multi-GPU: the final gather through the C ABI (RCCL inside) --
    def comm_unique_id(self) -> bytes:
        buf = (C.c_char * capi.UNIQUE_ID_BYTES)()
        self.lib.check(self.lib.dll.ahmc_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, unique_id: bytes, n_ranks: int, rank: int):
        buf = (C.c_char * capi.UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        self._call("ahmc_comm_init", buf, int(n_ranks), int(rank))

    def comm_info(self) -> dict:
        """what the communicator's own all-reduces reported when it was attached (ahmc_comm_info)"""
        v = [C.c_int64() for _ in range(4)]
        self._call("ahmc_comm_info", *[C.byref(x) for x in v])
        return dict(zip(("ranks_seen", "chains_total", "chains_min", "chains_max"), (x.value for x in v)))

    def reserve(self, kernel: "HMCKernel", n_samples: int):
        """announce a sampling run of n_samples transitions: its launch buffers are reserved now (ahmc_sample_reserve)"""
        if not self._external:
            k = kernel.cfg()
            self._call("ahmc_sample_reserve", C.byref(k), int(n_samples))

    def gather_moments(self) -> dict:
        mean, var = np.empty(self.D), np.empty(self.D)
        n, tot, ndiv = C.c_int64(), C.c_int64(), C.c_int64()
        self._call("ahmc_gather_moments", capi.as_ptr(mean), capi.as_ptr(var), C.byref(n), C.byref(tot), C.byref(ndiv))
        return {"mean": mean, "var": var, "n_draws": n.value, "total_n_steps": tot.value, "n_divergent": ndiv.value}

    def gather_state(self, theta_all_ptr):
        """ncclAllGather of θ into the caller's DEVICE buffer (D, N, n_ranks)"""
        self._call("ahmc_gather_state", theta_all_ptr if isinstance(theta_all_ptr, C.c_void_p) else capi.as_ptr(theta_all_ptr))

    # -- diagnostics computed where the data is --
    def ebfmi(self):
        """EBFMI (src/diagnosis.jl:1-3) per chain over the kept transitions of the last `run`"""
        out = self._out(vec=True)
        self._call("ahmc_ebfmi", capi.as_ptr(out))
        return out

    def ess(self, draws_ptr, n_draws):
        """ESS of every (dimension, chain) series of the (D, N, n_draws) device buffer `run(samples_out=…)` filled"""
        out = self._out()
        self._call("ahmc_ess", draws_ptr if isinstance(draws_ptr, C.c_void_p) else capi.as_ptr(draws_ptr), int(n_draws), capi.as_ptr(out))
        return out

    # -- convergence diagnostics on the device (include/ahmc_diag.h) --
    def _need_diag(self, what):
        if not getattr(self.lib, "has_diag", False):
            raise capi.UnsupportedError(capi.ERR_UNSUPPORTED, f"{what}: {self.lib.path} does not implement include/ahmc_diag.h")

    def summarystats(self, draws_ptr, n_draws, max_lag=0, out=None):
        """MCMCChains' `summarystats` columns of the (D, N, n_draws) device buffer `run(samples_out=…)` filled, pooled over all N
        chains: a dict name → (D,) array (diagnostics.SUMMARY_NAMES; diagnostics.summarystats is the host mirror).  `out`: optional
        (9, D) float64 buffer, host or device, that receives the rows."""
        self._need_diag("summarystats")
        buf = np.empty((9, self.D), dtype=np.float64) if out is None else out
        self._call("ahmc_diag_summary", draws_ptr if isinstance(draws_ptr, C.c_void_p) else capi.as_ptr(draws_ptr), int(n_draws), int(max_lag),
                   capi.as_ptr(buf))
        if out is not None:
            return out
        from .diagnostics import SUMMARY_NAMES

        return {k: buf[i].copy() for i, k in enumerate(SUMMARY_NAMES)}

    def rank_normalize(self, draws_ptr, n_draws, d, folded=False, out=None):
        """z (or the folded z_f) of dimension d: (n_draws, N) float64, element (k, c) of draw k of chain c; NaN at a dropped middle draw"""
        self._need_diag("rank_normalize")
        buf = np.empty((int(n_draws), self.N), dtype=np.float64) if out is None else out
        self._call("ahmc_diag_rank_normalize", draws_ptr if isinstance(draws_ptr, C.c_void_p) else capi.as_ptr(draws_ptr), int(n_draws), int(d),
                   1 if folded else 0, capi.as_ptr(buf))
        return buf

    @property
    def stream(self):
        return self.lib.dll.ahmc_stream(self._ctx)

    def accum(self, moments=True):
        tot, ntr, ndiv = C.c_int64(), C.c_int64(), C.c_int64()
        s1 = self._out() if moments else None
        s2 = self._out() if moments else None
        self._call("ahmc_get_accum", C.byref(tot), C.byref(ntr), C.byref(ndiv), capi.as_ptr(s1), capi.as_ptr(s2))
        return {"total_n_steps": tot.value, "n_transitions": ntr.value, "n_divergent": ndiv.value,
                "sum_theta": s1, "sumsq_theta": s2}

    def reset_accum(self):
        self._call("ahmc_reset_accum")

    INFO = {"group_lanes": 0, "elems_per_lane": 1, "nuts_launches": 2, "nuts_batch": 3, "iteration": 4, "nuts_kernel_ns": 5,
            "nuts_warm_launches": 6, "nuts_warm_kernel_ns": 7, "dense_gemm_launches": 8, "dense_gemm_small_launches": 9, "dense_pipelines": 10,
            "dense_pool": 11, "nuts_draw_batch": 12, "dense_epoch_launches": 13, "stepsize_scalar": 14, "wide": 15,
            "norm_tail_hits": 16, "norm_prefetch_hits": 17}

    # keys the CPU checker (oracle/) does not answer, and what they mean there: it has no thread geometry, so no wide mode either
    # (nor a launch whose normals could be made ahead of time)
    CHECKER_ONLY_ZERO = ("wide", "norm_tail_hits", "norm_prefetch_hits")

    def info(self, key):
        """engine introspection (ahmc_get_info): thread geometry, NUTS launch count / batch, iteration, wide context"""
        v = C.c_int64()
        code = self.lib.dll.ahmc_get_info(self._ctx, self.INFO[key], C.byref(v))
        if code == capi.ERR_ARGUMENT and key in self.CHECKER_ONLY_ZERO and not self.lib.backend.startswith("hip"):
            return 0
        self.lib.check(code, self._ctx)
        return v.value


# ------------------------------------------------------------------------------------------------
# free functions with the reference's names
# ------------------------------------------------------------------------------------------------
def find_good_stepsize(rng, h: Hamiltonian, theta, initial_step_size=0.1, max_n_iters=100, dtype=np.float64,
                       lib=None):
    """src/trajectory.jl:768-852.  θ (D,) → scalar ϵ; θ (D,N) → per-chain ϵ (N,)"""
    theta = np.asarray(theta)
    N = 1 if theta.ndim == 1 else theta.shape[1]
    eng = Engine(h, N, dtype=dtype, rng=rng, lib=lib)
    try:
        eng.set_position(theta)
        eps = eng.find_good_stepsize(initial_step_size, max_n_iters)
    finally:
        eng.close()
    return float(eps[0]) if theta.ndim == 1 else eps


def sample(rng, h: Hamiltonian, kernel: HMCKernel, theta, n_samples: int, adaptor=None, n_adapts: Optional[int] = None,
           drop_warmup=False, verbose=False, progress=False, dtype=None, lib=None, device=0):
    """sample(rng, h, κ, θ, n_samples, adaptor, n_adapts; drop_warmup) (src/sampler.jl:159-248).

    Returns `(θs, stats)`: a list of (D, N) arrays (or (D,) for vector θ) and a list of stat
    dicts with the reference's field names plus `is_adapt` (:193).  One transition + adapt! per
    iteration is issued through the C ABI, exactly the loop of :182-228."""
    adaptor = adaptor if adaptor is not None else NoAdaptation()
    if n_adapts is None:
        n_adapts = min(n_samples // 10, 1000)
    if drop_warmup and isinstance(adaptor, NoAdaptation):
        raise AssertionError("Cannot drop warmup samples if there is no adaptation phase.")  # :172
    theta = np.asarray(theta)
    dtype = dtype or (theta.dtype if theta.dtype in (np.float32, np.float64) else np.float64)
    N = 1 if theta.ndim == 1 else theta.shape[1]
    eng = Engine(h, N, dtype=dtype, rng=rng, lib=lib, device=device)
    try:
        eng.set_integrator(kernel.tau.integrator)
        eng.set_position(theta)  # sample_init (:36-46)
        eng.adaptor_init(adaptor)
        k = kernel.cfg()
        thetas, stats = [], []
        one = capi.KernelCfg.from_buffer_copy(k)
        for i in range(1, n_samples + 1):
            if eng._external:
                eng.transition(kernel)  # the same transition with the user's ∂ℓπ∂θ served through ahmc_ext_*
            else:
                eng._call("ahmc_sample", C.byref(one), 1, 0, 0, None)  # transition(rng, h, κ, t.z) (:184)
            st = eng.stats()
            isadapted = i <= n_adapts and not isinstance(adaptor, NoAdaptation)
            eng.adapt(i, n_adapts)
            st["is_adapt"] = isadapted
            if not drop_warmup or i > n_adapts:
                thetas.append(eng.theta())
                stats.append(st)
        return thetas, stats
    finally:
        eng.close()


def EBFMI(energies):
    """src/diagnosis.jl:1-3; energies: sequence over iterations of scalars or (N,) arrays"""
    E = np.asarray(energies, dtype=np.float64)
    num = np.mean(np.diff(E, axis=0) ** 2, axis=0)
    return num / np.var(E, axis=0, ddof=1)
