"""Guard bands, poisoned outputs and read-only checks around calls of the C ABI (test helper, imported by test_memory_contract.py).

hipMalloc hands out page-granular, zero-filled memory: with one allocation per operand a stray write lands in slack that is never read
back and a stray read returns zeros.  Here every buffer of a call is carved out of ONE allocation,

    [guard | buf0 | guard | buf1 | ... | guard]

with the guards filled with 0xA5 bytes: a write past either end of a buffer dirties a guard (or the neighbouring buffer, which is then
compared with the oracle or with what was uploaded), and a read past an end picks up 0xA5... or the neighbour's data instead of zeros.
Buffer starts are 32-byte aligned and never 256-byte aligned (an odd multiple of 32 bytes past a 256-byte boundary): the pointer a caller
gets who slices a tensor of containers.  Pure outputs are poisoned with 0x5A bytes: 0x5A5A... is no residue on any width class, so a
form that accumulates into an output, or leaves part of it unwritten, cannot pass.

`pkg` is anything with a lib() that has the fhe_hip_malloc / free / memset / memcpy_h2d / memcpy_d2h / sync entry points."""
import ctypes

import numpy as np

GUARD_BYTE, POISON_BYTE = 0xA5, 0x5A
GUARD_MIN, GUARD_MAX = 64 << 10, 16 << 20


def guard_bytes(unit_bytes):
    """max(64 KiB, 8 batch units), capped at 16 MiB: a grid rounded up to the 8 XCDs writes at most 7 units past the end."""
    return min(GUARD_MAX, max(GUARD_MIN, 8 * int(unit_bytes)))


def _ok(pkg, rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed with status {rc}: {pkg.lib().fhe_hip_last_error().decode(errors='replace')}")


class Slice:
    """One carved buffer: a raw device address (capi._ptr takes it through data_ptr) and its size."""

    def __init__(self, arena, name, offset, nbytes):
        self.arena, self.name, self.offset, self.nbytes = arena, name, offset, nbytes
        self.ptr = arena.base + offset

    def data_ptr(self):
        return self.ptr

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes == self.nbytes, (self.name, arr.nbytes, self.nbytes)
        _ok(self.arena.pkg, self.arena.pkg.lib().fhe_hip_memcpy_h2d(self.ptr, arr.ctypes.data, arr.nbytes), "memcpy_h2d")
        self.arena.uploaded[self.name] = arr.view(np.uint8).reshape(-1).copy()
        return self

    def poison(self):
        poison(self.arena.pkg, self)
        return self

    def download(self, shape, dtype=np.uint64):
        """From the arena image verify() took (one download per call)."""
        img = self.arena.image
        assert img is not None, "verify() first: it takes the one download of the arena"
        return img[self.offset:self.offset + self.nbytes].view(dtype).reshape(shape).copy()


def poison(pkg, buf):
    """0x5A bytes over a pure output (a Slice or a DeviceBuffer) before the call."""
    ptr = buf.data_ptr() if hasattr(buf, "data_ptr") else buf.ptr
    _ok(pkg, pkg.lib().fhe_hip_memset(ptr, POISON_BYTE, buf.nbytes), "memset")


def is_poison(arr):
    return bool((np.ascontiguousarray(arr).view(np.uint8) == POISON_BYTE).all())


class GuardedArena:
    """specs: (name, nbytes) in call order; unit_bytes: one batch unit of the call ([L][n] containers), which sizes the guards."""

    def __init__(self, pkg, specs, unit_bytes):
        self.pkg, self.guard = pkg, guard_bytes(unit_bytes)
        self.uploaded, self.image, self.base = {}, None, None
        self.order, self.slices = [], {}
        cursor = 0
        for i, (name, nbytes) in enumerate(specs):
            assert name not in self.slices and nbytes > 0 and nbytes % 4 == 0, (name, nbytes)
            start = (cursor + self.guard + 255) // 256 * 256 + 32 * (2 * (i % 4) + 1)       # 32, 96, 160, 224 past a 256-byte boundary
            self.order.append((name, start, int(nbytes)))
            cursor = start + int(nbytes)
        self.total = cursor + self.guard
        p = ctypes.c_void_p()
        _ok(pkg, pkg.lib().fhe_hip_malloc(ctypes.byref(p), self.total), "malloc")
        self.base = p.value
        assert self.base % 256 == 0, "allocation bases are 256-byte aligned"
        _ok(pkg, pkg.lib().fhe_hip_memset(self.base, GUARD_BYTE, self.total), "memset")
        for name, start, nbytes in self.order:
            s = Slice(self, name, start, nbytes)
            assert s.ptr % 32 == 0 and s.ptr % 256 != 0
            self.slices[name] = s

    def __getitem__(self, name):
        return self.slices[name]

    def guards(self):
        """(index, start, end, name of the buffer before or None, name of the buffer after or None)"""
        out, prev_end, prev_name = [], 0, None
        for i, (name, start, nbytes) in enumerate(self.order):
            out.append((i, prev_end, start, prev_name, name))
            prev_end, prev_name = start + nbytes, name
        out.append((len(self.order), prev_end, self.total, prev_name, None))
        return out

    def _guard_errors(self, img):
        errs = []
        for i, lo, hi, before, after in self.guards():
            assert hi - lo >= self.guard
            dirty = np.flatnonzero(img[lo:hi] != GUARD_BYTE)
            if dirty.size:
                first, last = int(dirty[0]), int(dirty[-1])
                errs.append(f"guard {i} (after {before!r}, before {after!r}; {hi - lo} bytes) was written: {dirty.size} dirty bytes, first at "
                            f"+{first} ({first} bytes past the end of {before!r}), last at +{last} ({hi - lo - last} bytes before the start of {after!r})")
        return errs

    def _input_errors(self, img, inputs):
        errs = []
        for name in inputs:
            s = self.slices[name]
            assert name in self.uploaded, f"{name!r} is declared an input and was never uploaded"
            diff = np.flatnonzero(img[s.offset:s.offset + s.nbytes] != self.uploaded[name])
            if diff.size:
                errs.append(f"input {name!r} was modified: {diff.size} bytes differ from the upload, first at byte {int(diff[0])}, last at byte {int(diff[-1])}")
        return errs

    def verify(self, inputs=()):
        """After the call: one sync, one download of the whole arena; every guard intact, every declared input as uploaded."""
        lib = self.pkg.lib()
        _ok(self.pkg, lib.fhe_hip_sync(), "sync")
        img = np.empty(self.total, np.uint8)
        _ok(self.pkg, lib.fhe_hip_memcpy_d2h(img.ctypes.data, self.base, self.total), "memcpy_d2h")
        self.image = img
        errs = self._guard_errors(img) + self._input_errors(img, inputs)
        assert not errs, "; ".join(errs)

    def free(self):
        if self.base:
            self.pkg.lib().fhe_hip_free(self.base); self.base = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
