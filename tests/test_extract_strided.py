"""fhe_rlwe_sample_extract_strided: `count` evenly spaced coefficients of RLWE pairs as LWE samples in one launch, bit for bit against `count`
calls of fhe_rlwe_sample_extract scattered into [batch][count][L][n + 1] through capi (and those against bootstrap_model on the small shapes).

n = 8 is the streaming-size engine and the Limb256 table instance, n = 2048 the word-sized limb tables; count = n makes every row start at
another parity of 8 bytes.  The inputs carry zeros (0 must stay 0 under the negation) and residues q - 1.  Every call runs inside a guarded
arena with the output poisoned."""
import numpy as np
import pytest

import ct_bootstrap_model as cm
import memcheck
import ntt_math as nm
from test_sample_extract import _pair

INVALID, UNSUPPORTED = -1, -5


def _singles(pkg, eng, n, L, batch, count, d0, d1):
    """the definition through capi: one fhe_rlwe_sample_extract per index, scattered on the host"""
    want = np.empty((batch, count, L, n + 1), np.uint64)
    row = pkg.DeviceBuffer(batch * L * (n + 1) * 8)
    for i in range(count):
        eng.sample_extract(row, d0, d1, i * (n // count), batch)
        want[:, i] = row.download((batch, L, n + 1))
    return want


def _check(pkg, n, bits, L, batch, counts, model=False):
    moduli = nm.ntt_primes(bits, n, L)
    eng = pkg.RnsNttEngine(n, moduli)
    c0, c1 = _pair(moduli, n, batch)
    c0[:, :, 0, 0] = [q - 1 for q in moduli]
    d0, d1 = pkg.DeviceBuffer.from_numpy(c0), pkg.DeviceBuffer.from_numpy(c1)
    S = L * n * 32
    for count in counts:
        ar = memcheck.GuardedArena(pkg, [("c0", batch * S), ("out", batch * count * L * (n + 1) * 8), ("c1", batch * S)], S)
        ar["c0"].upload(c0); ar["c1"].upload(c1); ar["out"].poison()
        eng.sample_extract_strided(ar["out"], ar["c0"], ar["c1"], count, batch)
        ar.verify(inputs=("c0", "c1"))
        got = ar["out"].download((batch, count, L, n + 1))
        ar.free()
        want = _singles(pkg, eng, n, L, batch, count, d0, d1)
        assert np.array_equal(got, want), (n, bits, L, batch, count)
        if model:
            assert np.array_equal(got, cm.extract_strided_np(c0[..., 0], c1[..., 0], moduli, count))


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [30, 40, 60])
@pytest.mark.parametrize("L,batch", [(1, 1), (3, 3), (1, 3), (3, 1)])
def test_the_streaming_size_engine_at_n_8(pkg, bits, L, batch):
    _check(pkg, 8, bits, L, batch, (1, 2, 8), model=True)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [30, 40, 60])
@pytest.mark.parametrize("L,batch", [(1, 1), (3, 3), (1, 3), (3, 1)])
def test_the_word_sized_limb_tables_at_n_2048(pkg, bits, L, batch):
    _check(pkg, 2048, bits, L, batch, (1, 2, 64))


@pytest.mark.gpu
@pytest.mark.parametrize("bits,L,batch", [(30, 1, 1), (40, 3, 1), (60, 1, 3)])
def test_every_coefficient_at_n_2048(pkg, bits, L, batch):
    """count = n: the rows of one polynomial are split over several workgroups, and row starts alternate between 16- and 8-byte alignment"""
    _check(pkg, 2048, bits, L, batch, (2048,))


@pytest.mark.gpu
def test_one_limb_output_is_what_the_key_switch_reads(pkg):
    """L = 1: [batch][count][1][n + 1] is [batch count][n + 1], sample b count + i the coefficient i n / count of ciphertext b"""
    n, batch, count = 2048, 2, 4
    moduli = nm.ntt_primes(30, n, 1)
    eng = pkg.RnsNttEngine(n, moduli)
    c0, c1 = _pair(moduli, n, batch)
    d0, d1 = pkg.DeviceBuffer.from_numpy(c0), pkg.DeviceBuffer.from_numpy(c1)
    out = pkg.DeviceBuffer(batch * count * (n + 1) * 8)
    eng.sample_extract_strided(out, d0, d1, count, batch)
    flat = out.download((batch * count, n + 1))
    one = pkg.DeviceBuffer((n + 1) * 8)
    for b in range(batch):
        for i in range(count):
            eng.sample_extract(one, d0.ptr + b * n * 32, d1.ptr + b * n * 32, i * n // count, 1)
            assert np.array_equal(flat[b * count + i], one.download((n + 1,)))


@pytest.mark.gpu
def test_rejections_leave_the_output_poisoned(pkg):
    n, L, batch, count = 2048, 2, 2, 4
    moduli = nm.ntt_primes(30, n, L)
    eng = pkg.RnsNttEngine(n, moduli)
    c0, c1 = _pair(moduli, n, batch)
    d0, d1 = pkg.DeviceBuffer.from_numpy(c0), pkg.DeviceBuffer.from_numpy(c1)
    out = pkg.DeviceBuffer(batch * count * L * (n + 1) * 8)
    memcheck.poison(pkg, out)
    lib, P = pkg.lib(), pkg.capi._ptr

    def call(h=eng.h, o=P(out), a=P(d0), b=P(d1), c=count, bt=batch):
        return lib.fhe_rlwe_sample_extract_strided(h, o, a, b, c, bt)

    bad = {"null handle": call(h=None), "null output": call(o=None), "null c0": call(a=None), "null c1": call(b=None), "batch 0": call(bt=0),
           "count 0": call(c=0), "count 3": call(c=3), "count above n": call(c=2 * n), "count 2^32 - 1": call(c=0xFFFFFFFF),
           "misaligned c0": call(a=P(d0) + 8), "misaligned c1": call(b=P(d1) + 8), "misaligned output": call(o=P(out) + 4),
           "output is c0": call(o=P(d0)), "output inside c1": call(o=P(d1) + 64, bt=1, c=1),
           "batch count overflows 32 bits": call(c=2048, bt=1 << 21), "batch count L above 2^31 - 1": call(c=1024, bt=1 << 20)}
    assert all(rc == INVALID for rc in bad.values()), bad
    # (n < 8 cannot be reached from here: no engine of such a size can be created)
    wide = pkg.RnsNttEngine(n, nm.ntt_primes(120, n, 2))
    assert lib.fhe_rlwe_sample_extract_strided(wide.h, P(out), P(d0), P(d1), count, 1) == UNSUPPORTED
    pkg.capi.sync()
    assert memcheck.is_poison(out.download((out.nbytes // 8,)))
    assert call() == 0
    pkg.capi.sync()
    assert not memcheck.is_poison(out.download((out.nbytes // 8,))[:8])
