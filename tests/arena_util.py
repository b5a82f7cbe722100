"""Guard-band arenas for tests/test_buffer_bounds.py (a helper: no tests in here).

An ARENA is one allocation the test owns; the buffer handed to the library (the EXTENT) is a view in its middle, 256-byte
aligned as torch gives it to callers.  On either side lies a BAND of max(64 KiB, size of the extent) bytes, at most 8 MiB, so a
callee that overruns by up to a whole buffer still lands in memory the test owns: nothing here creates a fault, an overrun that
exists becomes visible without one.  Bands hold a position-dependent byte pattern (a shifted copy of a band is damage too), or —
around INPUTS — a poison of the element type: quiet NaN, or ±1e30 with alternating sign (several kernels sanitise NaN or take
min / max, which would hide it).  Everything is compared as bytes / on integer views, so NaN payloads count.

`probe` runs one call of the library several times, each on a context prepared afresh by the case:
  plain   every array in an arena with small zeroed bands nobody checks, outputs pre-filled with finite pattern A — the reference
  pass 1  inputs inside NaN-poisoned bands, outputs pre-filled with a recognisable NaN payload inside pattern bands
  pass 2  inputs inside ±1e30-poisoned bands, outputs pre-filled with finite pattern B
  pass 3  inputs inside byte-pattern bands, outputs pre-filled with the NaN payload again
and asserts, bit for bit,
  W  no stray write      the bands around every output are intact after the call and ahmc_sync
  F  fully written       the meaningful part of every output extent equals the plain run's (whose pre-fill differs, so an element
                         the call leaves alone shows); a part documented as untouched still holds its pre-fill
  R  no stray read       every output and every extra observable equals the plain run's although the neighbourhood of the inputs
                         (and the part of an input documented as ignored) is poisoned
  C  const               every input extent and its bands are unchanged
A violation raises BoundsError carrying the property, the array's key and the first / last damaged offset: for W and C in BYTES
relative to the extent, with a sign (-1 = the byte just before the extent, +1 = the first byte after its end); for F, R (and C
inside the extent) the first / last differing ELEMENT index of the extent.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

KIB = 1024
MIN_BAND, MAX_BAND, ALIGN = 64 * KIB, 8 * KIB * KIB, 256
PLAIN_BAND = 4 * KIB   # the plain run: zeroed, unchecked slack, so that a callee's stray read there is deterministic


class BoundsError(AssertionError):
    def __init__(self, prop, key, first, last, note=""):
        self.prop, self.key, self.first, self.last = prop, key, first, last
        unit = "byte offsets relative to the extent" if prop in ("W", "C-band") else "element indices"
        super().__init__(f"[{prop}] {key}: damage from {first:+d} to {last:+d} ({unit}){' — ' + note if note else ''}")


def band_bytes(extent_bytes):
    return min(MAX_BAND, max(MIN_BAND, -(-int(extent_bytes) // 8) * 8))


_PATTERN = np.empty(0, dtype=np.uint8)


def byte_pattern(n):
    """position-dependent, with no short period (256·256·256 bytes)"""
    global _PATTERN
    if _PATTERN.size < n:
        i = np.arange(max(n, 1 << 20), dtype=np.int64)
        _PATTERN = ((i * 131 + (i >> 8) * 17 + (i >> 16) * 29 + 0x5A) & 0xFF).astype(np.uint8)
    return _PATTERN[:n].copy()


def _int_view(dt):
    return {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[np.dtype(dt).itemsize]


def poison(kind, dtype, n):
    """n elements of the band / ignored-part poison `kind` ('nan' | 'big' | 'pattern' | 'zero') for element type dtype"""
    dt = np.dtype(dtype)
    if kind == "zero":
        return np.zeros(n, dtype=dt)
    if kind == "pattern":
        return byte_pattern(n * dt.itemsize).view(dt)
    sign = np.where(np.arange(n) % 2 == 0, 1, -1)
    if dt.kind == "f":
        return np.full(n, np.nan, dtype=dt) if kind == "nan" else (sign * 1e30).astype(dt)
    big = np.iinfo(dt).max // 2 + 1   # integers have no NaN: the most negative value, or ±2^(bits-2)
    return np.full(n, np.iinfo(dt).min, dtype=dt) if kind == "nan" else (sign * big).astype(dt)


def prefill(kind, dtype, n):
    """what an output extent holds before the call: 'payload' = quiet NaNs with a recognisable payload (integers: a bit pattern),
    'A' / 'B' = two different finite patterns"""
    dt, i = np.dtype(dtype), np.arange(n, dtype=np.int64)
    if kind == "payload":
        if dt == np.float64:
            return (np.uint64(0x7FF8DEAD00000000) + (i & 0xFFFFFF).astype(np.uint64)).view(np.float64)
        if dt == np.float32:
            return (np.uint32(0x7FC5A000) + (i & 0xFFF).astype(np.uint32)).view(np.float32)
        return (np.int64(0x5A5A5A5A5A5A5A5A) + i).astype(np.uint64).astype(_int_view(dt)).view(dt)
    base, step = (-12345.0, -1.0) if kind == "A" else (777.0, 0.25)
    if dt.kind == "f":
        return (base + step * (i % 65536)).astype(dt)
    return ((-7 if kind == "A" else 1000003) - (i % 1000)).astype(dt)


class Arena:
    """bands + extent in one allocation.  where: 'host' (numpy), 'pinned' (page-locked host memory), 'device' (torch, cuda);
    fill: what the bands hold — 'pattern' | 'nan' | 'big' | 'zero' (the last: the plain run's small unchecked slack)"""

    def __init__(self, nbytes, where="host", fill="pattern", dtype=np.uint8):
        self.nbytes, self.where, self.fill = int(nbytes), where, fill
        band = PLAIN_BAND if fill == "zero" else band_bytes(nbytes)
        total = 2 * band + self.nbytes + ALIGN
        if where == "host":
            self._t, self._np = None, np.empty(total, dtype=np.uint8)
            base = self._np.ctypes.data
        else:
            import torch

            self._t = torch.empty(total, dtype=torch.uint8, device="cuda") if where == "device" else torch.empty(total, dtype=torch.uint8).pin_memory()
            self._np = None if where == "device" else self._t.numpy()
            base = self._t.data_ptr()
        self.off = band + (-(base + band)) % ALIGN
        self.ptr = base + self.off
        assert self.ptr % ALIGN == 0 and self.off >= band and total - self.off - self.nbytes >= band
        img = byte_pattern(total) if fill != "zero" else np.zeros(total, dtype=np.uint8)
        if fill in ("nan", "big"):
            item = np.dtype(dtype).itemsize
            nf = self.off // item
            img[self.off - nf * item:self.off] = poison(fill, dtype, nf).view(np.uint8)
            nb = (total - self.off - self.nbytes) // item
            img[self.off + self.nbytes:self.off + self.nbytes + nb * item] = poison(fill, dtype, nb).view(np.uint8)
        self.image = img
        self._upload()

    def _upload(self):
        if self._np is not None:
            self._np[:] = self.image
        else:
            import torch

            self._t.copy_(torch.from_numpy(self.image))
            torch.cuda.synchronize()

    def _download(self):
        if self._np is not None:
            return self._np.copy()
        import torch

        torch.cuda.synchronize()
        return self._t.cpu().numpy()

    def write(self, arr):
        """set the extent (and remember it as the state before the call)"""
        b = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        assert b.size == self.nbytes, (b.size, self.nbytes)
        self.image[self.off:self.off + self.nbytes] = b
        self._upload()

    def read(self, dtype=np.uint8):
        return self._download()[self.off:self.off + self.nbytes].view(dtype).copy()

    def band_damage(self):
        """None, or (first, last) damaged byte relative to the extent, signed: -1 the byte before it, +1 the first byte after its end"""
        now, lo, hi = self._download(), self.off, self.off + self.nbytes
        bad = np.flatnonzero(now != self.image)
        bad = bad[(bad < lo) | (bad >= hi)]
        if bad.size == 0:
            return None
        rel = np.where(bad < lo, bad - lo, bad - hi + 1)
        return int(rel[0]), int(rel[-1])

    def extent_damage(self, itemsize=1):
        """None, or (first, last) ELEMENT of the extent that no longer holds what `write` put there"""
        now = self._download()[self.off:self.off + self.nbytes]
        bad = np.flatnonzero(now != self.image[self.off:self.off + self.nbytes])
        return None if bad.size == 0 else (int(bad[0]) // itemsize, int(bad[-1]) // itemsize)


class In:
    """an input array: `arr` (any shape, its memory order is what the callee gets), `ignored`: boolean mask over the flattened
    extent of the part the header documents as not read (poisoned in passes 1 and 2), `where`: 'host' | 'pinned' | 'device'"""

    def __init__(self, arr, where="host", ignored=None):
        self.arr = np.ascontiguousarray(np.asarray(arr).reshape(-1, order="A"))
        self.where, self.ignored = where, ignored


class Out:
    """an output array of n elements of dtype.  meaningful: boolean mask over the extent of what the header documents as written
    (None: all of it); untouched: mask of what must keep its pre-fill (None: nothing is claimed)"""

    def __init__(self, dtype, n, where="host", meaningful=None, untouched=None):
        self.dtype, self.n, self.where = np.dtype(dtype), int(n), where
        self.meaningful, self.untouched = meaningful, untouched


class IO:
    """what a case's `call` gets: the addresses of the arrays (io[key], a ctypes void*) and, for calls that go back and forth
    (ask / tell), access to their contents"""

    def __init__(self, mode):
        self.mode = mode           # 'zero' (plain) | 'nan' | 'big' | 'pattern': the poison of this run
        self.arenas, self.specs, self.fills = {}, {}, {}

    def __getitem__(self, key):
        return C.c_void_p(self.arenas[key].ptr)

    def read(self, key):
        return self.arenas[key].read(self.specs[key].dtype if isinstance(self.specs[key], Out) else self.specs[key].arr.dtype)

    def write(self, key, arr, ignored=None):
        """replace an input's extent between two calls; `ignored` is poisoned as the run's mode says"""
        spec = self.specs[key]
        a = np.ascontiguousarray(arr, dtype=spec.arr.dtype).reshape(-1).copy()
        if ignored is not None and self.mode != "zero":
            a[ignored] = poison(self.mode, a.dtype, int(np.count_nonzero(ignored)))
        self.arenas[key].write(a)

    def refill(self, key):
        """put an output's pre-fill back (between two calls that write the same buffer)"""
        spec = self.specs[key]
        self.arenas[key].write(prefill(self.fills[key], spec.dtype, spec.n))


def _place(where, on_device):
    return where if on_device else "host"


def _one_run(setup, call, sync, ins, outs, mode, fill_kind, on_device):
    st = setup()
    io = IO(mode)
    try:
        for key, spec in ins.items():
            a = spec.arr.copy()
            if spec.ignored is not None and mode != "zero":
                a[spec.ignored] = poison(mode, a.dtype, int(np.count_nonzero(spec.ignored)))
            ar = Arena(a.nbytes, _place(spec.where, on_device), mode, a.dtype)
            ar.write(a)
            io.arenas[key], io.specs[key] = ar, spec
        for key, spec in outs.items():
            ar = Arena(spec.n * spec.dtype.itemsize, _place(spec.where, on_device), "zero" if mode == "zero" else "pattern")
            io.arenas[key], io.specs[key], io.fills[key] = ar, spec, fill_kind
            io.refill(key)
        extras = call(st, io) or {}
        if sync is not None:
            sync(st)
        res = {"extras": {k: np.array(v, copy=True) for k, v in extras.items()}, "outs": {}, "io": io}
        for key, spec in outs.items():
            res["outs"][key] = io.arenas[key].read(_int_view(spec.dtype))
        return res
    finally:
        close = getattr(st, "close", None)
        if close is not None:
            close()


def _first_last(mask):
    idx = np.flatnonzero(mask)
    return int(idx[0]), int(idx[-1])


def probe(setup, call, ins, outs, on_device=False, sync=None, passes=(("nan", "payload"), ("big", "B"), ("pattern", "payload"))):
    """see the module docstring.  setup() -> a context prepared identically every time (closed afterwards if it has .close);
    call(st, io) -> None or a dict of extra observables (arrays / scalars) that must not depend on the poison;
    sync(st): called after `call` and before anything is judged (ahmc_sync)."""
    plain = _one_run(setup, call, sync, ins, outs, "zero", "A", on_device)
    for mode, fill_kind in passes:
        run = _one_run(setup, call, sync, ins, outs, mode, fill_kind, on_device)
        io = run["io"]
        for key, spec in outs.items():                                   # W
            d = io.arenas[key].band_damage()
            if d:
                raise BoundsError("W", key, *d, note=f"pass {mode}/{fill_kind}")
        for key, spec in ins.items():                                    # C
            d = io.arenas[key].band_damage()
            if d:
                raise BoundsError("C-band", key, *d, note=f"pass {mode}/{fill_kind}")
            d = io.arenas[key].extent_damage(spec.arr.dtype.itemsize)
            if d:
                raise BoundsError("C", key, *d, note=f"the callee changed an input (pass {mode}/{fill_kind})")
        for key, spec in outs.items():                                   # F (and R: the outputs see the poison through the inputs)
            got, want = run["outs"][key], plain["outs"][key]
            m = np.ones(spec.n, dtype=bool) if spec.meaningful is None else np.asarray(spec.meaningful, dtype=bool)
            bad = (got != want) & m
            if bad.any():
                pre = prefill(fill_kind, spec.dtype, spec.n).view(_int_view(spec.dtype))
                unwritten = bad & (got == pre)
                if unwritten.any():
                    raise BoundsError("F", key, *_first_last(unwritten), note=f"still the pre-fill after the call (pass {mode}/{fill_kind})")
                raise BoundsError("R" if ins else "F", key, *_first_last(bad), note=f"differs from the plain run (pass {mode}/{fill_kind})")
            if spec.untouched is not None:
                pre = prefill(fill_kind, spec.dtype, spec.n).view(_int_view(spec.dtype))
                bad = (got != pre) & np.asarray(spec.untouched, dtype=bool)
                if bad.any():
                    raise BoundsError("W-extent", key, *_first_last(bad), note=f"a part of the extent documented as untouched was written (element indices; pass {mode}/{fill_kind})")
        for k, want in plain["extras"].items():                          # R
            got = run["extras"][k]
            if got.shape != want.shape or got.dtype != want.dtype or got.tobytes() != want.tobytes():
                diff = np.flatnonzero(got.reshape(-1).view(np.uint8) != want.reshape(-1).view(np.uint8)) if got.shape == want.shape else np.array([0])
                raise BoundsError("R", k, int(diff[0]) // max(want.dtype.itemsize, 1), int(diff[-1]) // max(want.dtype.itemsize, 1),
                                  note=f"an observable depends on the poison around the inputs (pass {mode})")
    return plain
