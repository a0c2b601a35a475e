"""fhe_rlwe_sample_extract: coefficient idx of RLWE pairs as LWE samples, bit for bit against bootstrap_model (Python integers).

out[b][l][j] = c1[idx - j] (j <= idx), (q_l - c1[n + idx - j]) mod q_l (j > idx), out[b][l][n] = c0[idx], as 8-byte residues.  Every call runs
inside a guarded arena with the output poisoned."""
import numpy as np
import pytest

import bootstrap_model as bm
import memcheck
import ntt_math as nm
from test_lwe_accumulator import _primes
from workload import rns_poly


def _pair(moduli, n, batch, seed=60):
    c0, c1 = rns_poly(seed, moduli, n, batch), rns_poly(seed + 1, moduli, n, batch)
    c1[:, :, 0, 0] = 0; c1[:, :, n - 1, 0] = 0; c1[0, 0, n // 2, 0] = 0          # zeros: the negation must give 0, not q
    for l, q in enumerate(moduli):
        c1[:, l, 1, 0] = q - 1; c1[:, l, n - 2, 0] = 1
    return c0, c1


def _check(pkg, eng, n, moduli, batch, idx, c0, c1):
    L = len(moduli)
    S = L * n * 32
    ar = memcheck.GuardedArena(pkg, [("c0", batch * S), ("out", batch * L * (n + 1) * 8), ("c1", batch * S)], S)
    ar["c0"].upload(c0); ar["c1"].upload(c1); ar["out"].poison()
    eng.sample_extract(ar["out"], ar["c0"], ar["c1"], idx, batch)
    ar.verify(inputs=("c0", "c1"))
    got = ar["out"].download((batch, L, n + 1))
    ar.free()
    assert np.array_equal(got, bm.extract_np(c0[..., 0], c1[..., 0], moduli, idx)), idx


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [30, 40, 60, 64])
def test_every_index_at_n_8(pkg, bits):
    n, L, batch = 8, 3, 3
    moduli = _primes(bits, n, L)
    eng = pkg.RnsNttEngine(n, moduli)
    c0, c1 = _pair(moduli, n, batch)
    for idx in range(n):
        _check(pkg, eng, n, moduli, batch, idx, c0, c1)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2048, 4096])
@pytest.mark.parametrize("bits", [30, 40, 60, 64])
@pytest.mark.parametrize("L,batch", [(1, 1), (3, 3), (1, 3), (3, 1)])
def test_shapes_and_width_classes(pkg, n, bits, L, batch):
    moduli = _primes(bits, n, L)
    eng = pkg.RnsNttEngine(n, moduli)
    c0, c1 = _pair(moduli, n, batch)
    for idx in (0, 1, n // 2, n - 1):
        _check(pkg, eng, n, moduli, batch, idx, c0, c1)


@pytest.mark.gpu
def test_rejections_leave_the_output_untouched(pkg):
    n, L, batch = 2048, 2, 2
    moduli = _primes(30, n, L)
    eng = pkg.RnsNttEngine(n, moduli)
    c0, c1 = _pair(moduli, n, batch)
    d0, d1 = pkg.DeviceBuffer.from_numpy(c0), pkg.DeviceBuffer.from_numpy(c1)
    out = pkg.DeviceBuffer(batch * L * (n + 1) * 8)
    memcheck.poison(pkg, out)
    lib, P = pkg.lib(), pkg.capi._ptr

    def call(h=eng.h, o=P(out), a=P(d0), b=P(d1), idx=0, bt=batch):
        return lib.fhe_rlwe_sample_extract(h, o, a, b, idx, bt)

    bad = [call(h=None), call(o=None), call(a=None), call(b=None), call(bt=0), call(idx=n), call(idx=0xFFFFFFFF), call(a=P(d0) + 8), call(b=P(d1) + 8),
           call(o=P(out) + 4), call(o=P(d0)), call(o=P(d1) + 64, bt=1)]
    assert all(rc == -1 for rc in bad), bad
    pkg.capi.sync()
    assert memcheck.is_poison(out.download((out.nbytes // 8,)))
    assert call(idx=n - 1) == 0
    wide = pkg.RnsNttEngine(n, nm.ntt_primes(120, n, 2))
    assert lib.fhe_rlwe_sample_extract(wide.h, P(out), P(d0), P(d1), 0, 1) == -5
