"""ctypes bindings for the C ABI declared in include/ahmc_hip.h.

`CLib(path)` binds every entry point of the header on one shared library.  The product
library is advancedhmc.jl_amd/csrc/libahmc_hip.so (HIP, gfx950) and is the ONLY library this
package ever opens by itself: `load_hip_library()` raises if it has not been built — there is
no CPU fallback.  (tests/ bind the same `CLib` class onto the CPU checker built under oracle/ to obtain the
checker; that path is never taken from inside the package.)
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

# --- enums (mirror include/ahmc_hip.h) --------------------------------------------------------
AHMC_ABI_VERSION = 6
OK, ERR_ARGUMENT, ERR_UNSUPPORTED, ERR_RUNTIME, ERR_STATE = 0, 1, 2, 3, 4
F32, F64 = 0, 1
METRIC_UNIT, METRIC_DIAG, METRIC_DENSE = 0, 1, 2
(TARGET_ISO_GAUSS, TARGET_DIAG_GAUSS, TARGET_FUNNEL, TARGET_HIER_GAUSS, TARGET_DENSE_GAUSS,
 TARGET_EXTERNAL, TARGET_PLUGIN, TARGET_KERNEL) = range(8)
KERNEL_HIP_FUNCTION, KERNEL_HIP_SYMBOL, KERNEL_HOST = 0, 1, 2
INTEGRATOR_LEAPFROG, INTEGRATOR_JITTERED, INTEGRATOR_TEMPERED = 0, 1, 2
TS_ENDPOINT, TS_MULTINOMIAL, TS_SLICE = 0, 1, 2
TC_CLASSIC, TC_GENERALISED, TC_STRICT = 0, 1, 2
ADAPT_NONE, ADAPT_STEPSIZE, ADAPT_MASSMATRIX, ADAPT_NAIVE, ADAPT_STAN = range(5)
VAR_WELFORD, VAR_NUTPIE, VAR_POOLED = 0, 1, 2
UNIQUE_ID_BYTES = 128

# stat fields: name -> (id, is_int)
STAT_FIELDS = {
    "n_steps": (0, True),
    "is_accept": (1, True),
    "acceptance_rate": (2, False),
    "log_density": (3, False),
    "hamiltonian_energy": (4, False),
    "hamiltonian_energy_error": (5, False),
    "max_hamiltonian_energy_error": (6, False),
    "tree_depth": (7, True),
    "numerical_error": (8, True),
    "step_size": (9, False),
    "nom_step_size": (10, False),
}


class KernelCfg(C.Structure):
    """ahmc_kernel_cfg"""
    _fields_ = [
        ("nuts", C.c_int32),
        ("sampler", C.c_int32),
        ("criterion", C.c_int32),
        ("max_depth", C.c_int32),
        ("delta_max", C.c_double),
        ("L", C.c_int64),
        ("lambda_", C.c_double),
        ("refresh_alpha", C.c_double),
    ]


class AdaptorState(C.Structure):
    """ahmc_adaptor_state"""
    _fields_ = [
        ("kind", C.c_int32),
        ("var_estimator", C.c_int32),
        ("init_buffer", C.c_int32),
        ("term_buffer", C.c_int32),
        ("window_size", C.c_int32),
        ("adapting", C.c_int32),
        ("has_da", C.c_int32),
        ("n_welford", C.c_int32),
        ("delta", C.c_double),
        ("stan_i", C.c_int64),
        ("n_adapts", C.c_int64),
        ("wv_n", C.c_int64),
        ("iteration", C.c_int64),
    ]


class AHMCError(RuntimeError):
    """A non-zero status from the C ABI.  `ArgumentError` mirrors Julia's exception of the
    same name (src/hamiltonian.jl:55-57, src/abstractmcmc.jl:64-70)."""

    def __init__(self, code, msg):
        super().__init__(f"[ahmc status {code}] {msg}")
        self.code = code


class ArgumentError(AHMCError, ValueError):
    pass


class UnsupportedError(AHMCError, NotImplementedError):
    pass


_vp, _i32, _i64, _u64, _f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double

# name -> (restype, argtypes); the complete symbol list of include/ahmc_hip.h
SIGNATURES = {
    "ahmc_create": (_i32, [_i32, _i32, _i64, _i64, _vp, C.POINTER(_vp)]),
    "ahmc_destroy": (_i32, [_vp]),
    "ahmc_last_error": (C.c_char_p, [_vp]),
    "ahmc_abi_version": (_i32, []),
    "ahmc_backend": (C.c_char_p, []),
    "ahmc_sync": (_i32, [_vp]),
    "ahmc_stream": (_vp, [_vp]),
    "ahmc_set_target": (_i32, [_vp, _i32, _vp, _i64]),
    "ahmc_set_target_plugin": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "ahmc_set_target_kernel": (_i32, [_vp, _i32, _vp, _i32, _i32, _vp]),
    "ahmc_set_metric": (_i32, [_vp, _i32, _vp, _i64]),
    "ahmc_get_metric": (_i32, [_vp, _vp, _i64]),
    "ahmc_set_stepsize": (_i32, [_vp, _vp, _i64]),
    "ahmc_get_stepsize": (_i32, [_vp, _vp]),
    "ahmc_set_integrator": (_i32, [_vp, _i32, _f64]),
    "ahmc_seed": (_i32, [_vp, _u64, _u64, _u64, _u64]),
    "ahmc_set_position": (_i32, [_vp, _vp, _vp]),
    "ahmc_set_phasepoint": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "ahmc_get_phasepoint": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "ahmc_refresh_momentum": (_i32, [_vp, _f64]),
    "ahmc_leapfrog": (_i32, [_vp, _i64]),
    "ahmc_lf_pre": (_i32, [_vp, _i32, _i64, _i64]),
    "ahmc_lf_post": (_i32, [_vp, _i32, _i64, _i64, _vp, _vp]),
    "ahmc_theta_ptr": (_vp, [_vp]),
    "ahmc_hmc_transition": (_i32, [_vp, _i64, _f64, _i32]),
    "ahmc_nuts_transition": (_i32, [_vp, _i32, _f64, _i32, _i32]),
    "ahmc_get_stat": (_i32, [_vp, _i32, _vp]),
    "ahmc_find_good_stepsize": (_i32, [_vp, _f64, _i32]),
    "ahmc_adaptor_init": (_i32, [_vp, _i32, _f64, _i32, _i32, _i32]),
    "ahmc_adapt": (_i32, [_vp, _i64, _i64, _vp, _vp]),
    "ahmc_adapt_point": (_i32, [_vp, _i64, _i64, _vp, _vp, _vp]),
    "ahmc_set_var_estimator": (_i32, [_vp, _i32]),
    "ahmc_stan_windows": (_i32, [_i32, _i32, _i32, _i64, C.POINTER(_i64), C.POINTER(_i64),
                                 C.POINTER(_i64), _i32, C.POINTER(_i32)]),
    "ahmc_sample": (_i32, [_vp, C.POINTER(KernelCfg), _i64, _i64, _i32, _vp]),
    "ahmc_sample_from": (_i32, [_vp, C.POINTER(KernelCfg), _i64, _i64, _i64, _i32, _vp]),
    "ahmc_sample_reserve": (_i32, [_vp, C.POINTER(KernelCfg), _i64]),
    "ahmc_set_ref_compat": (_i32, [_vp, _i32]),
    "ahmc_get_accum": (_i32, [_vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64), _vp, _vp]),
    "ahmc_reset_accum": (_i32, [_vp]),
    "ahmc_get_accum_state": (_i32, [_vp, C.POINTER(_i64), _vp, _vp, _vp, _vp, _vp]),
    "ahmc_set_accum_state": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "ahmc_get_info": (_i32, [_vp, _i32, C.POINTER(_i64)]),
    "ahmc_ext_begin": (_i32, [_vp, C.POINTER(KernelCfg), _i32]),
    "ahmc_ext_find_good_stepsize_begin": (_i32, [_vp, _f64, _i32]),
    "ahmc_ext_pending": (_i32, [_vp, C.POINTER(_i64), _vp, _vp]),
    "ahmc_ext_advance": (_i32, [_vp, _vp, _vp]),
    "ahmc_ext_cancel": (_i32, [_vp]),
    "ahmc_get_adaptor_state": (_i32, [_vp, C.POINTER(AdaptorState), _vp, _vp]),
    "ahmc_set_adaptor_state": (_i32, [_vp, C.POINTER(AdaptorState), _vp, _vp]),
    "ahmc_comm_unique_id": (_i32, [_vp]),
    "ahmc_comm_init": (_i32, [_vp, _vp, _i32, _i32]),
    "ahmc_set_comm": (_i32, [_vp, _vp, _i32, _i32]),
    "ahmc_comm_info": (_i32, [_vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    "ahmc_gather_moments": (_i32, [_vp, _vp, _vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    "ahmc_gather_state": (_i32, [_vp, _vp]),
    "ahmc_ebfmi": (_i32, [_vp, _vp]),
    "ahmc_ess": (_i32, [_vp, _vp, _i64, _vp]),
}

# include/ahmc_diag.h: optional entry points (the HIP engine exports them, the CPU checker does not); bound when present
AHMC_DIAG_VERSION = 1
DIAG_SIGNATURES = {
    "ahmc_diag_version": (_i32, []),
    "ahmc_diag_summary": (_i32, [_vp, _vp, _i64, _i64, _vp]),
    "ahmc_diag_rank_normalize": (_i32, [_vp, _vp, _i64, _i64, _i32, _vp]),
}

# include/ahmc_rank_update.h: optional entry points of RankUpdateEuclideanMetric (the HIP engine exports them, the CPU checker does not)
AHMC_RANK_UPDATE_VERSION = 1
AHMC_RANK_UPDATE_MAX_K = 32
METRIC_RANK_UPDATE = 3  # (Python side only: the C ABI has no such AHMC_METRIC_* — the metric has entry points of its own)
RU_SIGNATURES = {
    "ahmc_rank_update_version": (_i32, []),
    "ahmc_set_metric_rank_update": (_i32, [_vp, _vp, _vp, _vp, _i64]),
    "ahmc_get_metric_rank_update": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(_i64)]),
}

# include/ahmc_lowrank_adapt.h: the optional mass-matrix adaptor of that metric (likewise: the HIP engine only)
AHMC_LOWRANK_ADAPT_VERSION = 1
AHMC_LOWRANK_MAX_ELL = 40


class LowRankState(C.Structure):
    """ahmc_lowrank_state"""
    _fields_ = [
        ("k", C.c_int64),
        ("ell", C.c_int64),
        ("seed", C.c_uint64),
        ("n", C.c_int64),
        ("n_fits", C.c_int64),
    ]


LR_SIGNATURES = {
    "ahmc_lowrank_adapt_version": (_i32, []),
    "ahmc_lowrank_adaptor_init": (_i32, [_vp, _i32, _f64, _i32, _i32, _i32, _i64, _i64, _u64]),
    "ahmc_lowrank_get_state": (_i32, [_vp, C.POINTER(LowRankState), _vp, _vp, _vp, _vp, _vp]),
    "ahmc_lowrank_set_state": (_i32, [_vp, C.POINTER(LowRankState), _vp, _vp, _vp, _vp, _vp]),
}

# include/ahmc_glm.h: the optional generalised-linear-model target (likewise: the HIP engine only)
AHMC_GLM_VERSION = 1
TARGET_GLM = 8
GLM_BERNOULLI_LOGIT, GLM_POISSON_LOG, GLM_GAUSSIAN_IDENTITY = 0, 1, 2
GLM_SIGNATURES = {
    "ahmc_glm_version": (_i32, []),
    "ahmc_set_target_glm": (_i32, [_vp, _i32, _i64, _vp, _vp, _vp, _vp, _f64]),
    "ahmc_get_target_glm": (_i32, [_vp, C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_f64)]),
    "ahmc_glm_pointwise": (_i32, [_vp, _vp, _vp]),
}

# include/ahmc_glm_hier.h: coefficient groups whose prior scale is sampled (likewise: the HIP engine only)
AHMC_HGLM_VERSION = 1
HGLM_MAX_GROUPS = 32
_pi32 = C.POINTER(_i32)
HGLM_SIGNATURES = {
    "ahmc_hglm_version": (_i32, []),
    "ahmc_hglm_set_target": (_i32, [_vp, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _f64, _i32, _pi32, _pi32, _pi32, C.POINTER(_f64)]),
    "ahmc_hglm_get_target": (_i32, [_vp, C.POINTER(_i64), _pi32, _pi32, _pi32, _pi32, C.POINTER(_f64)]),
    "ahmc_hglm_coefficients": (_i32, [_vp, _vp, _i64, _vp, _vp]),
}

# include/ahmc_glm_aux.h: families of the GLM target whose dispersion is sampled (likewise: the HIP engine only)
AHMC_GLM_AUX_VERSION = 1
GLM_AUX_MAX_GROUPS = 31
GLM_GAUSSIAN_IDENTITY_SIGMA, GLM_NEGBINOMIAL_LOG = 3, 4
GLM_AUX_SIGNATURES = {
    "ahmc_glm_aux_version": (_i32, []),
    "ahmc_glm_aux_set_target": (_i32, [_vp, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _i32, _pi32, _pi32, _pi32, C.POINTER(_f64), _f64, _f64]),
    "ahmc_glm_aux_get_target": (_i32, [_vp, C.POINTER(_f64), C.POINTER(_f64)]),
    "ahmc_glm_dispersion": (_i32, [_vp, _vp, _i64, _vp]),
}

# include/ahmc_glm_factor.h: index-coded factors of the GLM target (likewise: the HIP engine only)
AHMC_GLM_FACTOR_VERSION = 1
GLM_FACTOR_MAX = 8
GLM_FACTOR_SIGNATURES = {
    "ahmc_glm_factor_version": (_i32, []),
    "ahmc_glm_factor_set_target": (_i32, [_vp, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _f64, _i32, _pi32, _pi32, _pi32, C.POINTER(_f64), _i32, _pi32, _pi32, _i32,
                                          _f64, _f64]),
    "ahmc_glm_factor_get_target": (_i32, [_vp, C.POINTER(_i64), _pi32, _pi32]),
}

# include/ahmc_glm_ordinal.h: the ordered-logit family of the GLM target, whose cutpoints are sampled (likewise: the HIP engine only)
AHMC_GLM_ORDINAL_VERSION = 1
GLM_ORDINAL_MAX_CATEGORIES = 16
GLM_ORDERED_LOGIT = 5
GLM_ORDINAL_SIGNATURES = {
    "ahmc_glm_ordinal_version": (_i32, []),
    "ahmc_glm_ordinal_set_target": (_i32, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _i32, _pi32, _pi32, _pi32, C.POINTER(_f64), _i32, _pi32, _pi32, _i32,
                                           C.POINTER(_f64)]),
    "ahmc_glm_ordinal_get_target": (_i32, [_vp, _pi32, C.POINTER(_f64)]),
    "ahmc_glm_cutpoints": (_i32, [_vp, _vp, _i64, _vp]),
}

# include/ahmc_glm_categorical.h: the categorical-logit family of the GLM target, for unordered classes (likewise: the HIP engine only)
AHMC_GLM_CATEGORICAL_VERSION = 1
GLM_CATEGORICAL_MAX_CATEGORIES = 16
GLM_CATEGORICAL_LOGIT = 6
GLM_CATEGORICAL_SIGNATURES = {
    "ahmc_glm_categorical_version": (_i32, []),
    "ahmc_glm_categorical_set_target": (_i32, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _i32, _pi32, _pi32, _pi32, C.POINTER(_f64), _i32, _pi32, _pi32, _i32]),
    "ahmc_glm_categorical_get_target": (_i32, [_vp, _pi32, C.POINTER(_i64)]),
    "ahmc_glm_class_probs": (_i32, [_vp, _vp, _i64, _vp]),
}

# include/ahmc_glm_loo.h: the pointwise log-likelihood of the kept draws, PSIS-LOO and WAIC of a GLM target (likewise: the HIP engine only)
AHMC_GLM_LOO_VERSION = 1
GLM_LOO_MAX_VALUES = 2**31 - 1
GLM_LOO_MAX_TAIL = 4096
GLM_LOO_SIGNATURES = {
    "ahmc_glm_loo_version": (_i32, []),
    "ahmc_glm_loglik": (_i32, [_vp, _vp, _i64, _vp]),
    "ahmc_glm_loo": (_i32, [_vp, _vp, _i64, C.POINTER(_f64), C.POINTER(_f64)]),
}

# include/ahmc_glm_predict.h: predictions of a GLM target at new data, their summaries over the draws and the held-out lpd (likewise)
AHMC_GLM_PREDICT_VERSION = 1
GLM_PRED_LINEAR, GLM_PRED_MEAN, GLM_PRED_VARIANCE, GLM_PRED_LOGLIK = 0, 1, 2, 3
GLM_PRED_WHAT = {"linear": GLM_PRED_LINEAR, "mean": GLM_PRED_MEAN, "variance": GLM_PRED_VARIANCE, "loglik": GLM_PRED_LOGLIK}


class GLMNewDataRecord(C.Structure):
    """struct ahmc_glm_newdata"""
    _fields_ = [("n_new", _i64), ("X", _vp), ("levels", C.POINTER(_i32)), ("offset", _vp), ("y", _vp)]


GLM_PREDICT_SIGNATURES = {
    "ahmc_glm_predict_version": (_i32, []),
    "ahmc_glm_predict": (_i32, [_vp, _vp, _vp, _i64, _i32, _vp]),
    "ahmc_glm_predict_summary": (_i32, [_vp, _vp, _vp, _i64, C.POINTER(_f64)]),
}

# include/ahmc_glm_yrep.h: posterior-predictive draws y_rep of a GLM target and their per-observation summaries (likewise)
AHMC_GLM_YREP_VERSION = 1
GLM_YREP_SIGNATURES = {
    "ahmc_glm_yrep_version": (_i32, []),
    "ahmc_glm_yrep_at": (_i32, [_vp, _i32, _i32, _i64, _vp, _vp, _pi32, _pi32, _u64, _vp]),
    "ahmc_glm_yrep": (_i32, [_vp, _vp, _vp, _i64, _u64, _vp]),
    "ahmc_glm_yrep_summary": (_i32, [_vp, _vp, _vp, _i64, _u64, C.POINTER(_f64)]),
}


class CLib:
    """One loaded implementation of the ABI."""

    def __init__(self, path: str):
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        self.path = os.path.abspath(path)
        self.dll = C.CDLL(self.path, mode=C.RTLD_GLOBAL if hasattr(C, "RTLD_GLOBAL") else 0)
        missing = []
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(self.dll, name)
            except AttributeError:
                missing.append(name)
                continue
            fn.restype = res
            fn.argtypes = args
        if missing:
            raise ImportError(f"{self.path} does not export: {', '.join(missing)}")
        v = self.dll.ahmc_abi_version()
        if v != AHMC_ABI_VERSION:
            raise ImportError(f"{self.path}: ABI version {v}, expected {AHMC_ABI_VERSION}")
        self.backend = self.dll.ahmc_backend().decode()
        # ahmc_diag.h: all of it or none of it
        diag = [getattr(self.dll, name, None) for name in DIAG_SIGNATURES]
        self.has_diag = all(fn is not None for fn in diag)
        if self.has_diag:
            for fn, (res, args) in zip(diag, DIAG_SIGNATURES.values()):
                fn.restype = res
                fn.argtypes = args
            v = self.dll.ahmc_diag_version()
            if v != AHMC_DIAG_VERSION:
                raise ImportError(f"{self.path}: ahmc_diag version {v}, expected {AHMC_DIAG_VERSION}")
        # ahmc_rank_update.h: likewise
        ru = [getattr(self.dll, name, None) for name in RU_SIGNATURES]
        self.has_rank_update = all(fn is not None for fn in ru)
        if self.has_rank_update:
            for fn, (res, args) in zip(ru, RU_SIGNATURES.values()):
                fn.restype = res
                fn.argtypes = args
            v = self.dll.ahmc_rank_update_version()
            if v != AHMC_RANK_UPDATE_VERSION:
                raise ImportError(f"{self.path}: ahmc_rank_update version {v}, expected {AHMC_RANK_UPDATE_VERSION}")
        # ahmc_lowrank_adapt.h: likewise
        lr = [getattr(self.dll, name, None) for name in LR_SIGNATURES]
        self.has_lowrank_adapt = all(fn is not None for fn in lr)
        if self.has_lowrank_adapt:
            for fn, (res, args) in zip(lr, LR_SIGNATURES.values()):
                fn.restype = res
                fn.argtypes = args
            v = self.dll.ahmc_lowrank_adapt_version()
            if v != AHMC_LOWRANK_ADAPT_VERSION:
                raise ImportError(f"{self.path}: ahmc_lowrank_adapt version {v}, expected {AHMC_LOWRANK_ADAPT_VERSION}")
        # ahmc_glm.h: likewise
        glm = [getattr(self.dll, name, None) for name in GLM_SIGNATURES]
        self.has_glm = all(fn is not None for fn in glm)
        if self.has_glm:
            for fn, (res, args) in zip(glm, GLM_SIGNATURES.values()):
                fn.restype = res
                fn.argtypes = args
            v = self.dll.ahmc_glm_version()
            if v != AHMC_GLM_VERSION:
                raise ImportError(f"{self.path}: ahmc_glm version {v}, expected {AHMC_GLM_VERSION}")
        # ahmc_glm_hier.h: likewise
        hglm = [getattr(self.dll, name, None) for name in HGLM_SIGNATURES]
        self.has_hglm = all(fn is not None for fn in hglm)
        if self.has_hglm:
            for fn, (res, args) in zip(hglm, HGLM_SIGNATURES.values()):
                fn.restype = res
                fn.argtypes = args
            v = self.dll.ahmc_hglm_version()
            if v != AHMC_HGLM_VERSION:
                raise ImportError(f"{self.path}: ahmc_glm_hier version {v}, expected {AHMC_HGLM_VERSION}")
        # ahmc_glm_aux.h: likewise
        gaux = [getattr(self.dll, name, None) for name in GLM_AUX_SIGNATURES]
        self.has_glm_aux = all(fn is not None for fn in gaux)
        if self.has_glm_aux:
            for fn, (res, args) in zip(gaux, GLM_AUX_SIGNATURES.values()):
                fn.restype = res
                fn.argtypes = args
            v = self.dll.ahmc_glm_aux_version()
            if v != AHMC_GLM_AUX_VERSION:
                raise ImportError(f"{self.path}: ahmc_glm_aux version {v}, expected {AHMC_GLM_AUX_VERSION}")
        # ahmc_glm_factor.h: likewise
        gfac = [getattr(self.dll, name, None) for name in GLM_FACTOR_SIGNATURES]
        self.has_glm_factor = all(fn is not None for fn in gfac)
        if self.has_glm_factor:
            for fn, (res, args) in zip(gfac, GLM_FACTOR_SIGNATURES.values()):
                fn.restype = res
                fn.argtypes = args
            v = self.dll.ahmc_glm_factor_version()
            if v != AHMC_GLM_FACTOR_VERSION:
                raise ImportError(f"{self.path}: ahmc_glm_factor version {v}, expected {AHMC_GLM_FACTOR_VERSION}")
        # ahmc_glm_ordinal.h: likewise
        gord = [getattr(self.dll, name, None) for name in GLM_ORDINAL_SIGNATURES]
        self.has_glm_ordinal = all(fn is not None for fn in gord)
        if self.has_glm_ordinal:
            for fn, (res, args) in zip(gord, GLM_ORDINAL_SIGNATURES.values()):
                fn.restype, fn.argtypes = res, args
            v = self.dll.ahmc_glm_ordinal_version()
            if v != AHMC_GLM_ORDINAL_VERSION:
                raise ImportError(f"{self.path}: ahmc_glm_ordinal version {v}, expected {AHMC_GLM_ORDINAL_VERSION}")
        # ahmc_glm_categorical.h: likewise
        gcat = [getattr(self.dll, name, None) for name in GLM_CATEGORICAL_SIGNATURES]
        self.has_glm_categorical = all(fn is not None for fn in gcat)
        if self.has_glm_categorical:
            for fn, (res, args) in zip(gcat, GLM_CATEGORICAL_SIGNATURES.values()):
                fn.restype, fn.argtypes = res, args
            v = self.dll.ahmc_glm_categorical_version()
            if v != AHMC_GLM_CATEGORICAL_VERSION:
                raise ImportError(f"{self.path}: ahmc_glm_categorical version {v}, expected {AHMC_GLM_CATEGORICAL_VERSION}")
        # ahmc_glm_loo.h: likewise
        gloo = [getattr(self.dll, name, None) for name in GLM_LOO_SIGNATURES]
        self.has_glm_loo = all(fn is not None for fn in gloo)
        if self.has_glm_loo:
            for fn, (res, args) in zip(gloo, GLM_LOO_SIGNATURES.values()):
                fn.restype, fn.argtypes = res, args
            v = self.dll.ahmc_glm_loo_version()
            if v != AHMC_GLM_LOO_VERSION:
                raise ImportError(f"{self.path}: ahmc_glm_loo version {v}, expected {AHMC_GLM_LOO_VERSION}")
        # ahmc_glm_predict.h: likewise
        gpred = [getattr(self.dll, name, None) for name in GLM_PREDICT_SIGNATURES]
        self.has_glm_predict = all(fn is not None for fn in gpred)
        if self.has_glm_predict:
            for fn, (res, args) in zip(gpred, GLM_PREDICT_SIGNATURES.values()):
                fn.restype, fn.argtypes = res, args
            v = self.dll.ahmc_glm_predict_version()
            if v != AHMC_GLM_PREDICT_VERSION:
                raise ImportError(f"{self.path}: ahmc_glm_predict version {v}, expected {AHMC_GLM_PREDICT_VERSION}")
        # ahmc_glm_yrep.h: likewise
        gyrep = [getattr(self.dll, name, None) for name in GLM_YREP_SIGNATURES]
        self.has_glm_yrep = all(fn is not None for fn in gyrep)
        if self.has_glm_yrep:
            for fn, (res, args) in zip(gyrep, GLM_YREP_SIGNATURES.values()):
                fn.restype, fn.argtypes = res, args
            v = self.dll.ahmc_glm_yrep_version()
            if v != AHMC_GLM_YREP_VERSION:
                raise ImportError(f"{self.path}: ahmc_glm_yrep version {v}, expected {AHMC_GLM_YREP_VERSION}")

    def check(self, code: int, ctx=None):
        if code == OK:
            return
        msg = self.dll.ahmc_last_error(ctx)
        msg = msg.decode("utf-8", "replace") if msg else ""
        if code == ERR_ARGUMENT:
            raise ArgumentError(code, msg)
        if code == ERR_UNSUPPORTED:
            raise UnsupportedError(code, msg)
        raise AHMCError(code, msg)


_HIP_LIB = None


def hip_library_path() -> str:
    # AHMC_HIP_LIB: another build of the SAME HIP engine (kernel-tuning experiments); its
    # backend string is still checked by load_hip_library()
    return os.environ.get("AHMC_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc",
                                                          "libahmc_hip.so")


def load_hip_library() -> CLib:
    """Open the HIP engine.  Fails loudly when it has not been built (no fallback)."""
    global _HIP_LIB
    if _HIP_LIB is None:
        path = hip_library_path()
        if not os.path.exists(path):
            raise ImportError(
                f"{path} is missing: build it with `python __graft_entry__.py` (hipcc, gfx950). "
                "This package has no CPU fallback.")
        # libtorch's bundled libamdhip64 must be the HIP runtime of the process if torch is used
        # at all (bench.py uses torch.distributed/RCCL): import torch first so that our library's
        # NEEDED libamdhip64.so.7 resolves to the copy already mapped.
        try:
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch is optional for single-process use
            pass
        _HIP_LIB = CLib(path)
        if not _HIP_LIB.backend.startswith("hip"):
            raise ImportError(f"{path} reports backend {_HIP_LIB.backend!r}, expected the HIP engine")
    return _HIP_LIB


def np_dtype(dtype_code: int):
    return np.float32 if dtype_code == F32 else np.float64


def dtype_code(dtype) -> int:
    dt = np.dtype(dtype)
    if dt == np.float32:
        return F32
    if dt == np.float64:
        return F64
    raise ArgumentError(ERR_ARGUMENT, f"element type must be float32 or float64, got {dt}")


class _OwningPtr(C.c_void_p):
    """void* that keeps the object it points into alive.  `as_ptr(np.ascontiguousarray(x))` hands the C call the
    address of a TEMPORARY: with a bare c_void_p the temporary is freed as soon as as_ptr returns, i.e. before the
    call runs (round-1 bug: the gradient of a user log-density was read from freed memory once D·N·8 B outgrew
    numpy's small-block cache).  The pointer object lives in the caller's argument tuple until the call returns,
    and so does what it refers to."""
    _keep = None


def as_ptr(a) -> C.c_void_p:
    """host numpy array, torch tensor (host or device) or raw int address -> void* (owning, see _OwningPtr)"""
    if a is None:
        return C.c_void_p(None)
    if isinstance(a, int):
        return C.c_void_p(a)
    if isinstance(a, np.ndarray):
        p = _OwningPtr(a.ctypes.data)
    elif hasattr(a, "data_ptr"):
        p = _OwningPtr(a.data_ptr())
    else:
        raise TypeError(f"cannot take the address of {type(a)}")
    p._keep = a
    return p
