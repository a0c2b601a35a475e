"""tests/memcheck.py on host memory: the guard and read-only checks must trip on a one-byte stray write (no GPU needed: the arena only asks its
`pkg` for malloc / memset / memcpy / sync, served here by ctypes on a host buffer).  The GPU twin is
test_memory_contract.py::test_guard_check_detects_an_overrun."""
import ctypes

import numpy as np
import pytest

from memcheck import GUARD_BYTE, GuardedArena, guard_bytes, is_poison


class _HostLib:
    def __init__(self):
        self.blocks = {}

    def fhe_hip_malloc(self, out, nbytes):
        raw = np.zeros(nbytes + 4096, np.uint8)
        base = (raw.ctypes.data + 4095) // 4096 * 4096
        self.blocks[base] = raw
        out._obj.value = base
        return 0

    def fhe_hip_free(self, p):
        self.blocks.pop(p, None); return 0

    def fhe_hip_memset(self, p, v, n):
        ctypes.memset(p, v, n); return 0

    def fhe_hip_memcpy_h2d(self, d, s, n):
        ctypes.memmove(d, s, n); return 0

    fhe_hip_memcpy_d2h = fhe_hip_memcpy_h2d

    def fhe_hip_sync(self):
        return 0

    def fhe_hip_last_error(self):
        return b""


class _HostPkg:
    def __init__(self):
        self._lib = _HostLib()

    def lib(self):
        return self._lib


def _arena(pkg, data):
    ar = GuardedArena(pkg, [("first", data.nbytes), ("second", data.nbytes), ("third", 4 * 333)], 1024)
    ar["first"].upload(data); ar["second"].upload(data); ar["third"].poison()
    return ar


def test_guard_sizes():
    assert guard_bytes(32) == 64 << 10 and guard_bytes(2 * 2048 * 32) == 1 << 20 and guard_bytes(65536 * 32) == 16 << 20 and guard_bytes(1 << 30) == 16 << 20


def test_layout_and_clean_verify():
    pkg, data = _HostPkg(), np.arange(3 * 1024, dtype=np.uint64)
    ar = _arena(pkg, data)
    assert all(s.ptr % 32 == 0 and s.ptr % 256 != 0 for s in ar.slices.values())
    assert [hi - lo >= ar.guard for _, lo, hi, _, _ in ar.guards()] == [True] * 4
    ar.verify(inputs=["first", "second"])
    assert np.array_equal(ar["second"].download(data.shape), data) and is_poison(ar["third"].download((-1,), np.uint8))
    assert (ar.image[:ar["first"].offset] == GUARD_BYTE).all()


@pytest.mark.parametrize("where,pattern", [
    (lambda ar: ar["first"].ptr + ar["first"].nbytes, r"guard 1 \(after 'first', before 'second'.*first at \+0 .*last at \+0 "),
    (lambda ar: ar["second"].ptr - 1, r"guard 1 .*\(1 bytes before the start of 'second'\)"),
    (lambda ar: ar["first"].ptr - 1, r"guard 0 \(after None, before 'first'"),
    (lambda ar: ar["third"].ptr + 4 * 333, r"guard 3 \(after 'third', before None"),
    (lambda ar: ar["second"].ptr + 777, r"input 'second' was modified: 1 bytes differ from the upload, first at byte 777"),
], ids=["past-first", "before-second", "before-first", "past-last", "inside-input"])
def test_one_stray_byte_is_reported(where, pattern):
    pkg, data = _HostPkg(), np.arange(3 * 1024, dtype=np.uint64)
    ar = _arena(pkg, data)
    ctypes.memset(where(ar), 0xFF, 1)
    with pytest.raises(AssertionError, match=pattern):
        ar.verify(inputs=["first", "second"])
