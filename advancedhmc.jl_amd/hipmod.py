"""hipModuleLoad / hipModuleGetFunction through ctypes: a hipFunction_t for `KernelTarget` (ahmc_set_target_kernel) from a
code object file — the Python stand-in for what a host language with its own GPU compiler (AMDGPU.jl) already holds.
The HIP runtime used is the copy already mapped into the process (torch's bundled libamdhip64 when torch is imported, the
one libahmc_hip.so pulled in otherwise), so the handle belongs to the runtime the engine launches with."""
from __future__ import annotations

import ctypes as C
import os

_RUNTIME = None


def hip_runtime() -> C.CDLL:
    global _RUNTIME
    if _RUNTIME is None:
        path = None
        try:
            with open("/proc/self/maps") as f:
                for line in f:
                    if "libamdhip64" in line:
                        path = line.split()[-1]
                        break
        except OSError:
            pass
        _RUNTIME = C.CDLL(path or "libamdhip64.so")
    return _RUNTIME


class Module:
    """a loaded code object; keeps the hipModule_t alive as long as its functions are in use"""

    def __init__(self, path: str):
        rt = hip_runtime()
        self._mod = C.c_void_p()
        self._functions = {}
        rc = rt.hipModuleLoad(C.byref(self._mod), os.fsencode(path))
        if rc != 0:
            raise RuntimeError(f"hipModuleLoad({path}) failed with hipError {rc}")

    def function(self, name: str) -> int:
        rt = hip_runtime()
        fn = C.c_void_p()
        rc = rt.hipModuleGetFunction(C.byref(fn), self._mod, name.encode())
        if rc != 0:
            raise RuntimeError(f"hipModuleGetFunction({name}) failed with hipError {rc}")
        return fn.value

    def launch(self, name: str, grid, block, *args, shared: int = 0):
        """hipModuleLaunchKernel of kernel `name` on the null stream, then hipDeviceSynchronize.  `grid` / `block`: an int or a
        tuple of up to 3.  Arguments: a torch tensor (its data pointer), a ctypes instance (as is), numpy int32 / int64 /
        float32 / float64 scalars, a Python int (int32) or a Python float (double)."""
        import numpy as np

        rt = hip_runtime()
        fn = self._functions.get(name)
        if fn is None:
            fn = self._functions[name] = self.function(name)
        vals = []
        for a in args:
            if hasattr(a, "data_ptr"):
                vals.append(C.c_void_p(a.data_ptr()))
            elif isinstance(a, C._SimpleCData):
                vals.append(a)
            elif isinstance(a, np.int64):
                vals.append(C.c_int64(int(a)))
            elif isinstance(a, np.float32):
                vals.append(C.c_float(float(a)))
            elif isinstance(a, (np.float64, float)):
                vals.append(C.c_double(float(a)))
            elif isinstance(a, (np.int32, int)) and not isinstance(a, bool):
                if not -2**31 <= int(a) < 2**31:
                    raise OverflowError(f"{name}: {a} does not fit an int32 argument (pass np.int64)")
                vals.append(C.c_int32(int(a)))
            else:
                raise TypeError(f"{name}: cannot pass an argument of type {type(a).__name__}")
        params = (C.c_void_p * max(1, len(vals)))(*[C.cast(C.pointer(v), C.c_void_p) for v in vals])
        g = tuple(grid) if isinstance(grid, (tuple, list)) else (grid,)
        b = tuple(block) if isinstance(block, (tuple, list)) else (block,)
        g, b = (g + (1, 1))[:3], (b + (1, 1))[:3]
        rt.hipModuleLaunchKernel.argtypes = [C.c_void_p] + [C.c_uint] * 6 + [C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
        rc = rt.hipModuleLaunchKernel(C.c_void_p(fn), *g, *b, shared, None, params, None)
        if rc != 0:
            raise RuntimeError(f"hipModuleLaunchKernel({name}) failed with hipError {rc}")
        rc = rt.hipDeviceSynchronize()
        if rc != 0:
            raise RuntimeError(f"{name}: hipDeviceSynchronize failed with hipError {rc}")

    def close(self):
        """hipModuleUnload — only once no engine holds a function of this module any more (the engine launches the
        hipFunction_t it was given; it does not own the module)"""
        if self._mod is not None and self._mod.value:
            hip_runtime().hipModuleUnload(self._mod)
        self._mod = None
