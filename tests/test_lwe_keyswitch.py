"""fhe_lwe_keyswitch / fhe_lwe_ksk_generate / create / export on the GPU, bit for bit against lwe_keyswitch_model (Python integers behind numpy).

Apply is tested with IMPORTED tables, so that it does not depend on generation; generation is tested through export.  Every apply runs inside
a guarded arena (memcheck): the output is poisoned first, the guards around it and the input must be intact.  The apply kernel's tile is 64
columns (one per lane) by 16, 4 or 1 ciphertexts (batch > 4, 2 .. 4, 1), its 16 waves split the n_in input coefficients."""
import ctypes
import os

import numpy as np
import pytest

import lwe_keyswitch_model as km
import memcheck
import ntt_math as nm

TOP64 = lambda n: nm.largest_ntt_primes(64, n, 1)[0]
PRIMES = {"top30": lambda n: nm.largest_ntt_primes(30, n, 1)[0], "p43": lambda n: nm.ntt_primes(43, n, 1)[0],
          "p62": lambda n: nm.ntt_primes(62, n, 1)[0], "top64": TOP64}

_engines = {}


def _eng(pkg, n, moduli):
    key = (n, tuple(moduli))
    if key not in _engines:
        _engines[key] = pkg.RnsNttEngine(n, list(moduli))
    return _engines[key]


def _uniform(rng, q, shape):
    return rng.integers(0, q, size=shape, dtype=np.uint64)


def _import(pkg, eng, w, rows):
    d = pkg.DeviceBuffer.from_numpy(rows)
    ksk = eng.import_lwe_ksk(w, rows.shape[1] - 1, d)
    d.free()                                    # the table was copied: the source may go
    return ksk


def _apply(pkg, eng, ksk, lwe, n_out, q_out=0):
    batch = lwe.shape[0]
    ar = memcheck.GuardedArena(pkg, [("in", lwe.nbytes), ("out", batch * (n_out + 1) * 8)], lwe.shape[1] * 8)
    ar["in"].upload(lwe); ar["out"].poison()
    eng.lwe_keyswitch(ksk, ar["out"], ar["in"], q_out, batch)
    ar.verify(inputs=("in",))
    out = ar["out"].download((batch, n_out + 1))
    ar.free()
    return out


def _check(pkg, n_in, q, w, n_out, batch, q_out=0, seed=1, rows=None, lwe=None, eng=None, expect_wide=None):
    eng = eng or _eng(pkg, n_in, [q])
    rng = np.random.default_rng(seed)
    K = km.num_digits(q, w)
    assert eng.lwe_ksk_num_digits(w) == K
    rows = _uniform(rng, q, (n_in * K, n_out + 1)) if rows is None else rows
    lwe = _uniform(rng, q, (batch, n_in + 1)) if lwe is None else lwe
    if expect_wide is not None:
        assert km.u64_form(q, w, n_in * K) == (not expect_wide)
    ksk = _import(pkg, eng, w, rows)
    assert ksk.nbytes() == n_in * K * ((n_out + 1 + 63) // 64 * 64) * 8
    got = _apply(pkg, eng, ksk, lwe, n_out, q_out)
    want = km.keyswitch_np(q, w, rows, lwe, q_out)
    assert np.array_equal(got, want)
    return ksk, rows, lwe, got


# ------------------------------------------------------------------------------------------------ apply
@pytest.mark.gpu
@pytest.mark.parametrize("n_out", [1, 63, 64, 65, 300])
def test_column_tile_edges(pkg, n_out):
    _check(pkg, 8, PRIMES["top30"](8), 8, n_out, 3, seed=n_out)


@pytest.mark.gpu
@pytest.mark.parametrize("n_in,w,K", [(8, 10, 3), (2048, 7, 5), (1024, 8, 4)])
def test_rows_not_divisible_by_the_wave_split(pkg, n_in, w, K):
    """n_in = 8: 8 of the 16 waves have no coefficient; K = 3 and K = 5 rows per coefficient; n = 8 and n = 1024 are engines of the full-width
    class by size (no word-sized kernels below 2^11)"""
    q = PRIMES["top30"](n_in)
    assert km.num_digits(q, w) == K
    _check(pkg, n_in, q, w, 65, 5, seed=n_in)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 2, 3, 4, 5, 15, 16, 17, 33])
def test_batch_tile_edges(pkg, batch):
    _check(pkg, 2048, PRIMES["top30"](2048), 8, 12, batch, seed=batch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PRIMES))
@pytest.mark.parametrize("w", [8, 32])
def test_accumulator_extremes_all_q_minus_one(pkg, name, w):
    """table and input all q - 1, in every word-sized field; at the top 64-bit prime acc + b carries out of 64 bits"""
    n_in = 2048
    q = PRIMES[name](n_in)
    K = km.num_digits(q, w)
    rows = np.full((n_in * K, 66), q - 1, dtype=np.uint64)
    lwe = np.full((5, n_in + 1), q - 1, dtype=np.uint64)
    _check(pkg, n_in, q, w, 65, 5, rows=rows, lwe=lwe)
    _check(pkg, n_in, q, w, 65, 5, seed=w)                  # and random values in the same field


@pytest.mark.gpu
@pytest.mark.parametrize("name,n_in,w,wide", [("p43", 8, 16, False), ("p43", 8, 17, True), ("top30", 8, 31, False), ("top30", 8, 32, True),
                                             ("top30", 2048, 22, False), ("top30", 2048, 23, True)])
def test_u64_and_wide_forms_at_the_boundary(pkg, name, n_in, w, wide):
    """bit_length(q) + w + ceil(log2 R) = 64 on one side and 65 on the other"""
    q = PRIMES[name](n_in)
    K = km.num_digits(q, w)
    total = q.bit_length() + w + (n_in * K - 1).bit_length()
    assert total == (65 if wide else 64), total
    rows = np.full((n_in * K, 3), q - 1, dtype=np.uint64)
    lwe = np.full((2, n_in + 1), q - 1, dtype=np.uint64)
    _check(pkg, n_in, q, w, 2, 2, rows=rows, lwe=lwe, expect_wide=wide)
    _check(pkg, n_in, q, w, 70, 6, seed=w, expect_wide=wide)


@pytest.mark.gpu
def test_forced_wide_form_gives_the_same_bits(pkg):
    n_in, w, q = 2048, 8, PRIMES["top30"](2048)
    _, rows, lwe, got = _check(pkg, n_in, q, w, 65, 17, seed=3, expect_wide=False)
    os.environ["FHE_HIP_LWE_KSK_WIDE"] = "1"
    try:
        ksk = _import(pkg, _eng(pkg, n_in, [q]), w, rows)
    finally:
        del os.environ["FHE_HIP_LWE_KSK_WIDE"]
    assert np.array_equal(_apply(pkg, _eng(pkg, n_in, [q]), ksk, lwe, 65), got)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["p62", "top64", "top30"])
@pytest.mark.parametrize("q_out", [0, 2, 1 << 32, 1 << 48, 1000003])
def test_modulus_switch_epilogue(pkg, name, q_out):
    """random accumulators, and accumulators placed on the rounding steps: with in[0] = 1 and row 0 = the wanted values acc_i is that value
    for i < n_out, and acc_{n_out} = row + b"""
    n_in, w, n_out = 8, 8, 6
    q = PRIMES[name](n_in)
    K = km.num_digits(q, w)
    _check(pkg, n_in, q, w, 65, 5, q_out=q_out, seed=7)
    if q_out:
        exact = (-(q // 2) * pow(q_out, -1, q)) % q          # acc q_out + floor(q / 2) is an exact multiple of q
        targets = [exact, (exact - 1) % q, (exact + 1) % q, 0, q - 1, q // 2]
        rows = np.zeros((n_in * K, n_out + 1), dtype=np.uint64)
        rows[0, :n_out] = targets
        lwe = np.zeros((2, n_in + 1), dtype=np.uint64)
        lwe[:, 0] = 1
        lwe[0, n_in], lwe[1, n_in] = exact, (exact + 1) % q
        _, _, _, got = _check(pkg, n_in, q, w, n_out, 2, q_out=q_out, rows=rows, lwe=lwe)
        assert [int(v) for v in got[0, :n_out]] == [km.round_to(t, q, q_out) for t in targets]
        assert int(got[0, n_out]) == km.round_to(exact, q, q_out)


@pytest.mark.gpu
def test_level_zero_engine_and_one_limb_engine_share_a_key(pkg):
    n, w, n_out, batch = 2048, 8, 12, 5
    moduli = nm.ntt_primes(30, n, 3)
    q = moduli[0]
    e3, e1 = _eng(pkg, n, moduli), _eng(pkg, n, moduli[:1])
    ksk, rows, lwe, got = _check(pkg, n, q, w, n_out, batch, eng=e3)
    assert np.array_equal(_apply(pkg, e1, ksk, lwe, n_out), got)
    other = _eng(pkg, n, moduli[1:2])                        # another first prime: refused
    d_in, d_out = pkg.DeviceBuffer.from_numpy(lwe), pkg.DeviceBuffer(batch * (n_out + 1) * 8)
    with pytest.raises(pkg.FheError) as e:
        other.lwe_keyswitch(ksk, d_out, d_in, 0, batch)
    assert e.value.code == -1


# ------------------------------------------------------------------------------------------------ generation
def _secret(pkg, eng, n, q, rng, L=1, moduli=None):
    s = _uniform(rng, q, n)                                  # residues of limb 0, NOT small
    cont = np.zeros((L, n, 4), dtype=np.uint64)
    cont[0, :, 0] = s
    for l in range(1, L):
        cont[l, :, 0] = _uniform(rng, moduli[l], n)
    ds = pkg.DeviceBuffer.from_numpy(cont)
    return [int(v) for v in s], ds, eng.import_secret_key(ds)


def _z(rng, n_out):
    z = [int(v) for v in rng.integers(-(1 << 15), (1 << 15) + 1, n_out)]
    z[0] = -(1 << 15)
    if n_out > 2:
        z[1], z[2] = 1 << 15, -1
    return z


def _export(pkg, eng, ksk, R, n_out):
    d = pkg.DeviceBuffer(R * (n_out + 1) * 8)
    memcheck.poison(pkg, d)
    eng.export_lwe_ksk(ksk, d)
    return d.download((R, n_out + 1))


@pytest.mark.gpu
@pytest.mark.parametrize("name,w,n_out,noise_scale,sigma", [
    ("top30", 8, 65, 1, 3.2), ("top30", 1, 1, 40961, 3.2), ("p43", 32, 65, 1, 3.2), ("p43", 8, 1, 40961, 90.0), ("p62", 1, 65, 1, 3.2),
    ("p62", 32, 1, 40961, 3.2), ("top64", 8, 65, 40961, 3.2), ("top64", 1, 1, 1, 90.0), ("top64", 32, 65, 1, 3.2)])
def test_generate_equals_the_model(pkg, oracle, name, w, n_out, noise_scale, sigma):
    n = 8
    q = PRIMES[name](n)
    eng = _eng(pkg, n, [q])
    rng = np.random.default_rng(w * 100 + n_out)
    s, ds, sk = _secret(pkg, eng, n, q, rng)
    z = _z(rng, n_out)
    seeds = (1000 + w, (1 << 63) + n_out)
    ksk = eng.generate_lwe_ksk(sk, w, z, noise_scale, sigma, seeds)
    K = km.num_digits(q, w)
    got = _export(pkg, eng, ksk, n * K, n_out)
    want = km.ksk_generate_np(oracle, q, s, z, w, noise_scale, sigma, seeds)
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_generated_and_imported_handles_apply_alike_on_a_three_limb_engine(pkg, oracle):
    """N = 2048, L = 3: s_j is limb 0 of the imported key; generate -> export -> create gives the same apply output, which is the model's"""
    n, w, n_out, batch = 2048, 8, 12, 5
    moduli = nm.ntt_primes(30, n, 3)
    q = moduli[0]
    eng = _eng(pkg, n, moduli)
    rng = np.random.default_rng(11)
    s, ds, sk = _secret(pkg, eng, n, q, rng, L=3, moduli=moduli)
    z = [int(v) for v in rng.integers(0, 2, n_out)]
    ksk = eng.generate_lwe_ksk(sk, w, z, 1, 3.2, (5, 6))
    K = km.num_digits(q, w)
    rows = _export(pkg, eng, ksk, n * K, n_out)
    assert np.array_equal(rows, km.ksk_generate_np(oracle, q, s, z, w, 1, 3.2, (5, 6)))
    lwe = _uniform(rng, q, (batch, n + 1))
    a = _apply(pkg, eng, ksk, lwe, n_out)
    b = _apply(pkg, eng, _import(pkg, eng, w, rows), lwe, n_out)
    assert np.array_equal(a, b) and np.array_equal(a, km.keyswitch_np(q, w, rows, lwe))
    # the phase identity on the device's output: phase_z(out) = phase_s(in) + sum d e
    e = [int(v) for v in km.ksk_noise_np(oracle, n, K, 3.2, (5, 6))]
    for ct, o in zip(lwe, a):
        ct = [int(v) for v in ct]
        want = (ct[-1] + sum(x * y for x, y in zip(ct[:-1], s)) + km.digit_noise(q, w, ct, e, 1)) % q
        assert (int(o[-1]) + sum(int(x) * y for x, y in zip(o[:-1], z))) % q == want


# ------------------------------------------------------------------------------------------------ argument checks
@pytest.mark.gpu
def test_rejections_leave_the_outputs_untouched(pkg):
    n, w, n_out, batch = 2048, 8, 12, 3
    moduli = nm.ntt_primes(30, n, 2)
    q = moduli[0]
    eng, other = _eng(pkg, n, moduli[:1]), _eng(pkg, n, moduli[1:2])
    small = _eng(pkg, 1024, [PRIMES["top30"](1024)])
    wide = pkg.RnsNttEngine(n, nm.ntt_primes(120, n, 1))
    rng = np.random.default_rng(4)
    K = km.num_digits(q, w)
    rows = _uniform(rng, q, (n * K, n_out + 1))
    ksk = _import(pkg, eng, w, rows)
    lwe = _uniform(rng, q, (batch, n + 1))
    d_in, d_out, d_rows = pkg.DeviceBuffer.from_numpy(lwe), pkg.DeviceBuffer(batch * (n_out + 1) * 8 + 64), pkg.DeviceBuffer.from_numpy(rows)
    memcheck.poison(pkg, d_out)
    lib, P = pkg.lib(), pkg.capi._ptr

    def call(h=eng.h, k=ksk.h, qo=0, o=P(d_out), i=P(d_in), b=batch):
        return lib.fhe_lwe_keyswitch(h, k, qo, o, i, b)

    bad = [call(h=None), call(k=None), call(o=None), call(i=None), call(b=0), call(qo=1), call(qo=(1 << 48) + 1), call(o=P(d_out) + 4),
           call(i=P(d_in) + 4), call(o=P(d_in)), call(o=P(d_in) + 8 * n, b=1), call(h=other.h), call(h=small.h)]
    assert bad == [-1] * len(bad)
    assert call(h=wide.h) == -5
    pkg.capi.sync()
    assert memcheck.is_poison(d_out.download((d_out.nbytes // 4,), np.uint32))
    assert call() == 0 and call(qo=2) == 0 and call(qo=1 << 48) == 0

    # create / export
    out = ctypes.c_void_p(0x1234)
    def create(h=eng.h, o=ctypes.byref(out), ww=w, no=n_out, r=P(d_rows)):
        return lib.fhe_lwe_ksk_create(h, o, ww, no, r)
    bad = [create(h=None), create(o=None), create(r=None), create(ww=0), create(ww=33), create(no=0), create(no=65537), create(r=P(d_rows) + 4)]
    assert bad == [-1] * len(bad)
    assert create(h=wide.h) == -5 and out.value == 0x1234
    d_exp = pkg.DeviceBuffer(rows.nbytes)
    memcheck.poison(pkg, d_exp)
    bad = [lib.fhe_lwe_ksk_export(None, ksk.h, P(d_exp)), lib.fhe_lwe_ksk_export(eng.h, None, P(d_exp)), lib.fhe_lwe_ksk_export(eng.h, ksk.h, None),
           lib.fhe_lwe_ksk_export(eng.h, ksk.h, P(d_exp) + 4), lib.fhe_lwe_ksk_export(other.h, ksk.h, P(d_exp))]
    assert bad == [-1] * len(bad)
    assert lib.fhe_lwe_ksk_export(wide.h, ksk.h, P(d_exp)) == -5
    pkg.capi.sync()
    assert memcheck.is_poison(d_exp.download((d_exp.nbytes // 4,), np.uint32))
    assert lib.fhe_lwe_ksk_destroy(None) == 0

    # generate
    s_c = np.zeros((1, n, 4), dtype=np.uint64); s_c[0, :, 0] = _uniform(rng, q, n)
    ds = pkg.DeviceBuffer.from_numpy(s_c)
    sk, sk_other = eng.import_secret_key(ds), other.import_secret_key(ds)
    zs = (ctypes.c_int32 * n_out)(*([1] * n_out)); seeds = (ctypes.c_uint64 * 2)(1, 2)
    z_big = (ctypes.c_int32 * n_out)(*([1] * (n_out - 1) + [(1 << 15) + 1])); z_neg = (ctypes.c_int32 * n_out)(*([-(1 << 15) - 1] + [0] * (n_out - 1)))
    before = eng.workspace_bytes()

    def gen(h=eng.h, k=sk.h, ww=w, no=n_out, z=zs, t=1, sg=3.2, sd=seeds, o=ctypes.byref(out)):
        return lib.fhe_lwe_ksk_generate(h, k, ww, no, z, t, sg, sd, o)
    bad = [gen(h=None), gen(k=None), gen(z=None), gen(sd=None), gen(o=None), gen(k=sk_other.h), gen(no=0), gen(no=65537), gen(ww=0), gen(ww=33),
           gen(z=z_big), gen(z=z_neg), gen(t=0), gen(sg=0.0), gen(sg=-1.0), gen(sg=float("nan")), gen(sg=1e9)]
    assert bad == [-1] * len(bad)
    assert out.value == 0x1234 and eng.workspace_bytes() == before
    # ceil(12 sigma) >= q: a tiny modulus (n = 8, q = 17)
    tiny = _eng(pkg, 8, [17])
    t_c = np.zeros((1, 8, 4), dtype=np.uint64); t_c[0, :, 0] = 3
    dts = pkg.DeviceBuffer.from_numpy(t_c)
    tsk = tiny.import_secret_key(dts)
    assert gen(h=tiny.h, k=tsk.h, sg=3.2) == -1 and out.value == 0x1234           # ceil(38.4) = 39 >= 17
    assert gen(h=tiny.h, k=tsk.h, sg=1.0) == 0 and out.value not in (0, 0x1234)   # 12 < 17
    assert lib.fhe_lwe_ksk_destroy(out) == 0
    wsk_src = pkg.DeviceBuffer(n * 32); wsk_src.zero()
    out2 = ctypes.c_void_p(0x1234)
    assert lib.fhe_lwe_ksk_generate(wide.h, wide.import_secret_key(wsk_src).h, w, n_out, zs, 1, 3.2, seeds, ctypes.byref(out2)) == -5 and out2.value == 0x1234
