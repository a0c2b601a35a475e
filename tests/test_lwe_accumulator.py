"""fhe_lwe_prepare_accumulator: an LWE batch into the inputs of fhe_blind_rotate, bit for bit against bootstrap_model (Python integers).

acc0[b] = X^(2n - ms(b_b)) tv, acc1[b] = 0, shifts[i][b] = (2n - ms(a_{b,i})) mod 2n with ms(v) = floor((v 2n + floor(q_lwe / 2)) / q_lwe) mod 2n.
Every call runs inside a guarded arena (memcheck): the three outputs are poisoned first, the guards around them and the inputs must be intact."""
import ctypes

import numpy as np
import pytest

import bootstrap_model as bm
import memcheck
import ntt_math as nm
from workload import rns_poly

NEW_SYMBOLS = ("fhe_rgsw_keys_generate", "fhe_lwe_prepare_accumulator", "fhe_rlwe_sample_extract")


def _primes(bits, n, L):
    return nm.largest_ntt_primes(64, n, L) if bits == 64 else nm.ntt_primes(bits, n, L)


def _tv(moduli, n, seed=40):
    """a canonical test vector with the entries 0 and q - 1 in every limb"""
    tv = rns_poly(seed, moduli, n, 1)[0]
    for l, q in enumerate(moduli):
        tv[l, 0, 0], tv[l, 1, 0], tv[l, n - 1, 0] = 0, q - 1, q - 1
    return tv


def _lwe(rng, q_lwe, n_lwe, batch):
    return np.array([[int(rng.integers(0, min(q_lwe, 1 << 62))) % q_lwe for _ in range(n_lwe + 1)] for _ in range(batch)], dtype=np.uint64)


def _run(pkg, eng, n, moduli, q_lwe, lwe, tv):
    """the call inside a guarded arena; returns (acc0, acc1, shifts) as downloaded"""
    batch, n_lwe, L = lwe.shape[0], lwe.shape[1] - 1, len(moduli)
    S = L * n * 32
    ar = memcheck.GuardedArena(pkg, [("lwe", lwe.nbytes), ("tv", S), ("acc0", batch * S), ("acc1", batch * S), ("shifts", n_lwe * batch * 4)], S)
    ar["lwe"].upload(lwe); ar["tv"].upload(tv)
    for name in ("acc0", "acc1", "shifts"):
        ar[name].poison()
    eng.lwe_prepare_accumulator(q_lwe, n_lwe, ar["lwe"], ar["tv"], ar["acc0"], ar["acc1"], ar["shifts"], batch)
    ar.verify(inputs=("lwe", "tv"))
    out = (ar["acc0"].download((batch, L, n, 4)), ar["acc1"].download((batch, L, n, 4)), ar["shifts"].download((n_lwe, batch), np.uint32))
    ar.free()
    return out


def _check(pkg, n, moduli, q_lwe, lwe, tv=None, eng=None):
    eng = eng or pkg.RnsNttEngine(n, moduli)
    tv = _tv(moduli, n) if tv is None else tv
    acc0, acc1, shifts = _run(pkg, eng, n, moduli, q_lwe, lwe, tv)
    want0, want_sh = bm.prepare_np(lwe, tv[..., 0], moduli, q_lwe)
    assert not acc1.any()
    assert np.array_equal(shifts, want_sh)
    assert not acc0[..., 1:].any()
    assert np.array_equal(acc0[..., 0], want0.astype(np.uint64))
    return acc0, acc1, shifts


# ------------------------------------------------------------------------------------------------ CPU
def test_exports_wrappers_and_rejection_without_device(pkg):
    lib = pkg.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    for method in ("generate_rgsw_keys", "lwe_prepare_accumulator", "sample_extract"):
        assert callable(getattr(pkg.RnsNttEngine, method)), method
    assert lib.fhe_lwe_prepare_accumulator(None, 1 << 32, 1, None, None, None, None, None, 1) == -1
    assert lib.fhe_rlwe_sample_extract(None, None, None, None, 0, 1) == -1
    o0 = (ctypes.c_void_p * 1)(0x1234); o1 = (ctypes.c_void_p * 1)(0x5678)
    mu = (ctypes.c_int32 * 1)(1); seeds = (ctypes.c_uint64 * 2)(1, 2)
    assert lib.fhe_rgsw_keys_generate(None, None, 16, mu, 1, 65537, 3.2, seeds, o0, o1) == -1
    assert (o0[0], o1[0]) == (0x1234, 0x5678)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("bits", [30, 40, 60, 64])
def test_every_rotation_at_n_8(pkg, bits):
    """n = 8, L = 3: b values that land on every b~ in [0, 2n), one ciphertext each (batch 16), and a second value on each"""
    n, L, q_lwe = 8, 3, 1 << 32
    moduli = _primes(bits, n, L)
    rng = np.random.default_rng(1)
    for off in (0, (q_lwe // (2 * n)) // 3):
        lwe = _lwe(rng, q_lwe, 5, 2 * n)
        lwe[:, -1] = [(t * (q_lwe // (2 * n)) + off) % q_lwe for t in range(2 * n)]
        assert sorted(bm.ms(int(v), q_lwe, n) for v in lwe[:, -1]) == list(range(2 * n))
        _check(pkg, n, moduli, q_lwe, lwe)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2048, 4096])
@pytest.mark.parametrize("bits", [30, 40, 60, 64])
@pytest.mark.parametrize("L,batch,n_lwe", [(1, 1, 1), (3, 3, 5), (1, 3, 1), (3, 1, 5)])
def test_shapes_and_width_classes(pkg, n, bits, L, batch, n_lwe):
    moduli = _primes(bits, n, L)
    rng = np.random.default_rng(n + bits + L)
    _check(pkg, n, moduli, 1 << 32, _lwe(rng, 1 << 32, n_lwe, batch))


@pytest.mark.gpu
@pytest.mark.parametrize("q_lwe", [2, 1 << 32, 1 << 48, 1000003])
def test_rounding_edges(pkg, q_lwe):
    """a = 0, a = q_lwe - 1 (ms wraps 2n to 0), and the values on both sides of rounding boundaries: v 2n + floor(q_lwe / 2) crosses a multiple
    of q_lwe between ceil((k q_lwe - floor(q_lwe / 2)) / 2n) - 1 and that value"""
    n, L = 2048, 3
    moduli = _primes(30, n, L)
    edges = [0, q_lwe - 1]
    for k in (1, 2, n, 2 * n - 1, 2 * n):
        v = -(-(k * q_lwe - q_lwe // 2) // (2 * n))
        edges += [x % q_lwe for x in (v - 1, v, v + 1)]
    edges = sorted(set(edges))
    if q_lwe > 2:
        assert len({bm.ms(v, q_lwe, n) for v in edges}) > 4
    n_lwe = len(edges)
    lwe = np.array([edges + [edges[b % len(edges)]] for b in range(3)], dtype=np.uint64)     # b runs over edges too
    lwe[1, -1], lwe[2, -1] = edges[-1], edges[len(edges) // 2]
    _, _, shifts = _check(pkg, n, moduli, q_lwe, lwe)
    assert shifts.shape == (n_lwe, 3) and shifts[0, 0] == 0
    assert shifts[-1, 0] == (n if q_lwe == 2 else 0)               # q_lwe - 1 rounds up to 2n, which wraps to 0 (q_lwe = 2: ms(1) = n)


@pytest.mark.gpu
def test_shift_table_is_steps_by_batch(pkg):
    """distinct a per (ciphertext, index): the table is [n_lwe][batch], as fhe_blind_rotate reads it"""
    n, L, q_lwe, n_lwe, batch = 2048, 1, 1 << 12, 5, 3
    moduli = _primes(30, n, L)
    lwe = np.array([[(b * 7 + i) % (1 << 12) for i in range(n_lwe + 1)] for b in range(batch)], dtype=np.uint64)
    _, _, shifts = _check(pkg, n, moduli, q_lwe, lwe)
    for i in range(n_lwe):
        for b in range(batch):
            assert shifts[i, b] == (2 * n - bm.ms(b * 7 + i, q_lwe, n)) % (2 * n)
    assert not np.array_equal(shifts, shifts.T.reshape(shifts.shape))


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [30, 60])
def test_equals_the_device_composition(pkg, bits):
    """acc0 = tv + (X^shift - 1) tv with shift = (2n - b~) mod 2n: fhe_rns_monomial_mul_sub + fhe_rns_poly_add on a broadcast copy of tv"""
    n, L, batch, q_lwe = 2048, 3, 3, 1 << 32
    moduli = _primes(bits, n, L)
    eng = pkg.RnsNttEngine(n, moduli)
    rng = np.random.default_rng(9)
    lwe = _lwe(rng, q_lwe, 5, batch)
    tv = _tv(moduli, n)
    acc0, _, _ = _check(pkg, n, moduli, q_lwe, lwe, tv=tv, eng=eng)
    sh = np.array([(2 * n - bm.ms(int(v), q_lwe, n)) % (2 * n) for v in lwe[:, -1]], dtype=np.uint32)
    tvb = np.ascontiguousarray(np.broadcast_to(tv[None], (batch,) + tv.shape))
    d_tv, d_sh, d_tmp = pkg.DeviceBuffer.from_numpy(tvb), pkg.DeviceBuffer.from_numpy(sh), pkg.DeviceBuffer(tvb.nbytes)
    eng.monomial_mul_sub(d_tmp, d_tv, d_sh, batch)
    eng.poly_add(d_tmp, d_tmp, d_tv, batch)
    assert np.array_equal(d_tmp.download(tvb.shape), acc0)


@pytest.mark.gpu
def test_rejections_leave_the_outputs_untouched(pkg):
    n, L, batch, n_lwe, q_lwe = 2048, 2, 2, 3, 1 << 32
    moduli = _primes(30, n, L)
    eng = pkg.RnsNttEngine(n, moduli)
    S = L * n * 32
    lwe = _lwe(np.random.default_rng(2), q_lwe, n_lwe, batch)
    d_lwe, d_tv = pkg.DeviceBuffer.from_numpy(lwe), pkg.DeviceBuffer.from_numpy(_tv(moduli, n))
    d0, d1, dsh = pkg.DeviceBuffer(batch * S), pkg.DeviceBuffer(batch * S), pkg.DeviceBuffer(n_lwe * batch * 4)
    for d in (d0, d1, dsh):
        memcheck.poison(pkg, d)
    lib, P = pkg.lib(), pkg.capi._ptr

    def call(h=eng.h, q=q_lwe, k=n_lwe, lw=P(d_lwe), tv=P(d_tv), a0=P(d0), a1=P(d1), sh=P(dsh), b=batch):
        return lib.fhe_lwe_prepare_accumulator(h, q, k, lw, tv, a0, a1, sh, b)

    bad = [call(h=None), call(lw=None), call(tv=None), call(a0=None), call(a1=None), call(sh=None), call(b=0), call(k=0), call(q=0), call(q=1),
           call(q=(1 << 48) + 1), call(tv=P(d_tv) + 8), call(a0=P(d0) + 8), call(a1=P(d1) + 16 + 8), call(lw=P(d_lwe) + 4), call(sh=P(dsh) + 2),
           call(a1=P(d0)), call(a1=P(d0) + 32, b=1), call(a0=P(d_tv)), call(a1=P(d_tv)), call(sh=P(d0)), call(sh=P(d_lwe)), call(a0=P(d_lwe))]
    assert all(rc == -1 for rc in bad), bad
    pkg.capi.sync()
    for d in (d0, d1, dsh):
        assert memcheck.is_poison(d.download((d.nbytes // 4,), np.uint32))
    assert call() == 0
    wide = pkg.RnsNttEngine(n, nm.ntt_primes(120, n, 2))
    assert lib.fhe_lwe_prepare_accumulator(wide.h, q_lwe, n_lwe, P(d_lwe), P(d_tv), P(d0), P(d1), P(dsh), 1) == -5
