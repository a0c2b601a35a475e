"""The CKKS encoder on the device (fhe_ckks_encoder_*, fhe_ckks_encode, fhe_ckks_decode, fhe_ckks_decode_poly) against the long-double
model of ckks_model.py.

Tolerances.  E is the largest error of a plain float64 numpy implementation of the same formula against the model ON THE SAME INPUTS, computed
per case; the device is allowed 4 E (another butterfly order, contracted multiply-adds).  Encode: |c_j - scale m_j| <= 1/2 + 4 scale E.
Decode: (n/2 + 1) / scale for the rounding of the coefficients where the input was rounded, plus 4 E of the decode formula.  The exact cases
have no tolerance: every residue of every limb bit for bit.
The figures measured on an MI355X are in DESIGN.md 4.17."""
import ctypes
import math

import numpy as np
import pytest

import ckks_model as cm
import memcheck
import ntt_math as nm

LD, CLD = cm.LD, cm.CLD
INVALID, UNSUPPORTED = -1, -5
SIZES = [2048, 4096, 8192, 16384]
T63 = 1 << 63


def mixed_moduli(n):
    """A 30-bit, a 40-bit and a 64-bit prime, and a 30-bit, a 60-bit and a 64-bit one: negative coefficients go through every reduction."""
    p30 = nm.ntt_primes(30, n, 2)
    return ([p30[0], nm.ntt_primes(40, n, 1)[0], nm.largest_ntt_primes(64, n, 1)[0]],
            [p30[1], nm.ntt_primes(60, n, 1)[0], nm.largest_ntt_primes(64, n, 2)[1]])


def _engine(pkg, n, moduli):
    e = pkg.RnsNttEngine(n, moduli)
    e.L = len(moduli)
    return e


def _slots_array(z):
    """complex [batch][h] -> float64 [batch][h][2]"""
    z = np.asarray(z, dtype=np.complex128)
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1))


def _encode(pkg, e, enc, z, scale, bits=True):
    batch, h = z.shape
    n = 2 * h
    dz = pkg.DeviceBuffer.from_numpy(_slots_array(z))
    do = pkg.DeviceBuffer(batch * e.L * n * 32)
    db = pkg.DeviceBuffer(batch * 4) if bits else None
    memcheck.poison(pkg, do)
    if bits:
        memcheck.poison(pkg, db)
    enc.encode(do, dz, scale, batch, db)
    got = do.download((batch, e.L, n, 4))
    assert np.array_equal(dz.download((batch, h, 2), np.float64), _slots_array(z))
    return got, (db.download((batch,), np.uint32) if bits else None)


def _decode_words(pkg, enc, words, t, scale):
    batch, n = words.shape
    dm = pkg.DeviceBuffer.from_numpy(words)
    dz = pkg.DeviceBuffer(batch * n * 8)
    memcheck.poison(pkg, dz)
    enc.decode(dz, dm, t, scale, batch)
    out = dz.download((batch, n // 2, 2), np.float64)
    assert np.array_equal(dm.download((batch, n)), words)
    return out[..., 0] + 1j * out[..., 1]


def _signed(containers, q):
    """[..][n] centred Python integers of one limb's low words"""
    w = containers[..., 0].astype(object)
    return np.where(w > q // 2, w - q, w)


def decode_tol(n, scale, want):
    """The decode tolerance for slots `want` ([h] complex) of a plaintext rounded at `scale`: (n/2 + 1) / scale + 4 E, E the error of the
    float64 numpy decode of the model's polynomial against the model."""
    m = cm.encode(want, n)
    return (n / 2 + 1) / scale + 4 * cm.float64_decode_error(m.astype(np.float64), cm.decode(m))


_exact = {}


def exact_case(n, batch=3):
    """Integer polynomials with coefficients uniform in [-2^20, 2^20] (0, +-1, +-2^20 among them) and their slots, rounded to double; the model
    recovers them (asserted here, on the CPU, before the device is asked), computed once."""
    if n not in _exact:
        rng = np.random.default_rng(n)
        m0 = rng.integers(-(1 << 20), (1 << 20) + 1, (batch, n))
        m0[0, :5] = [0, 1, -1, 1 << 20, -(1 << 20)]
        m0[1, -5:] = [-(1 << 20), 1 << 20, -1, 1, 0]
        z = np.stack([cm.decode(m.astype(LD)) for m in m0])
        cm.spot_check(m0[0].astype(LD), z[0], n, 1e-6)                   # |z| ~ sqrt(n) 2^20, compared as doubles
        z = z.astype(np.complex128)
        for b in range(batch):                                           # the reference alone is exact: transform error << 1/2
            for cdtype in (CLD, np.complex128):
                m = cm.encode(z[b], n, cdtype)
                assert float(np.max(np.abs(m.astype(LD) - m0[b].astype(LD)))) < 2.0 ** -10
        _exact[n] = (m0, z)
    return _exact[n]


_generic = {}


def generic_case(n, batch=3):
    """z uniform in the unit square, the model's m, and E (per plaintext), computed once."""
    if n not in _generic:
        rng = np.random.default_rng(1000 + n)
        z = rng.random((batch, n // 2)) + 1j * rng.random((batch, n // 2))
        m = [cm.encode(zb, n) for zb in z]
        cm.spot_check(m[0], z[0].astype(CLD), n, 1e-15)
        E = [cm.float64_error(zb, n, mb) for zb, mb in zip(z, m)]
        _generic[n] = (z, m, E)
    return _generic[n]


# ------------------------------------------------------------------------------------------------ 1. exact cases
@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_integer_polynomials_encode_to_their_residues_bit_for_bit(pkg, n):
    m0, z = exact_case(n)
    for moduli in mixed_moduli(n):
        e = _engine(pkg, n, moduli)
        enc = pkg.capi.CkksEncoder(e)
        got, bits = _encode(pkg, e, enc, z, 1.0)
        want = np.zeros_like(got)
        for l, q in enumerate(moduli):
            want[:, l, :, 0] = np.array([[int(c) % q for c in row] for row in m0], dtype=np.uint64)
        assert np.array_equal(got, want), (n, moduli)
        assert [int(b) for b in bits] == [cm.bit_length(np.max(np.abs(row))) for row in m0]
        e.check_canonical(pkg.DeviceBuffer.from_numpy(got), 3)


# ------------------------------------------------------------------------------------------------ 2. generic cases
@pytest.mark.gpu
@pytest.mark.parametrize("log_scale", [30, 50])
@pytest.mark.parametrize("n", SIZES)
def test_generic_slots_round_within_half_plus_four_times_the_float64_error(pkg, n, log_scale):
    z, m, E = generic_case(n)
    scale = float(2 ** log_scale)
    moduli = [nm.ntt_primes(60, n, 1)[0], nm.ntt_primes(30, n, 1)[0]]     # limb 0 wide enough for the centred value
    e = _engine(pkg, n, moduli)
    enc = pkg.capi.CkksEncoder(e)
    got, bits = _encode(pkg, e, enc, z, scale)
    for b in range(3):
        c = _signed(got[b, 0], moduli[0])
        err = np.abs(np.array([LD(int(x)) for x in c]) - LD(scale) * m[b])
        print(f"n={n} scale=2^{log_scale} b={b}: max |c - scale m| - 1/2 = {float(np.max(err)) - 0.5:.3e}, scale*E(numpy float64) = {scale * E[b]:.3e}, "
              f"device transform error <= {(float(np.max(err)) - 0.5) / scale:.3e} vs E = {E[b]:.3e}")
        assert float(np.max(err)) <= 0.5 + 4 * scale * E[b], (n, log_scale, b)
        assert np.array_equal(got[b, 1, :, 0], np.array([int(x) % moduli[1] for x in c], dtype=np.uint64))
        assert int(bits[b]) == cm.bit_length(max(abs(int(x)) for x in c))


# ------------------------------------------------------------------------------------------------ 3. decode
@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_decode_poly_of_encode_returns_the_slots(pkg, n):
    z, m, E = generic_case(n)
    scale = float(2 ** 40)
    moduli = [nm.ntt_primes(60, n, 1)[0], nm.ntt_primes(30, n, 1)[0]]
    e = _engine(pkg, n, moduli)
    enc = pkg.capi.CkksEncoder(e)
    got, _ = _encode(pkg, e, enc, z, scale)
    dp = pkg.DeviceBuffer.from_numpy(got)
    dz = pkg.DeviceBuffer(3 * n * 8)
    memcheck.poison(pkg, dz)
    enc.decode_poly(dz, dp, scale, 3)
    out = dz.download((3, n // 2, 2), np.float64)
    back = out[..., 0] + 1j * out[..., 1]
    for b in range(3):
        c = _signed(got[b, 0], moduli[0])
        zc = cm.decode(np.array([LD(int(x)) for x in c]) / LD(scale))     # the model's slots of the rounded polynomial
        tol = (n / 2 + 1) / scale + 4 * cm.float64_decode_error(np.array([float(int(x)) for x in c]) / scale, zc)
        d = back[b].astype(CLD) - z[b].astype(CLD)
        print(f"n={n} b={b}: round trip max error {float(np.max(np.abs(d))):.3e}, tolerance {tol:.3e}")
        assert float(max(np.max(np.abs(d.real)), np.max(np.abs(d.imag)))) <= tol


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_decode_of_centred_words_for_three_plaintext_moduli(pkg, n):
    """Hand-made centred words: t = 2^63 (values up to +-2^61), t = 0 (two's complement int64), an odd t (values up to +-(t - 1)/2)."""
    rng = np.random.default_rng(7 + n)
    e = _engine(pkg, n, nm.ntt_primes(30, n, 2))
    enc = pkg.capi.CkksEncoder(e)
    scale = float(2 ** 45)
    t_odd = (1 << 50) + 55
    for t, bound in ((T63, 1 << 61), (0, 1 << 62), (t_odd, (t_odd - 1) // 2)):
        v = rng.integers(-bound, bound + 1, (3, n), dtype=np.int64)
        v[0, :4] = [0, -1, bound, -bound]
        words = (v.astype(object) % (t if t else 1 << 64)).astype(np.uint64)
        got = _decode_words(pkg, enc, words, t, scale)
        for b in range(3):
            mv = np.array([LD(int(x)) for x in v[b]]) / LD(scale)
            zc = cm.decode(mv)
            if b == 0:
                cm.spot_check(mv, zc, n, float(bound) / scale * n * 2.0 ** -50)
            tol = (n / 2 + 1) / scale + 4 * cm.float64_decode_error(mv.astype(np.float64), zc)
            d = got[b].astype(CLD) - zc
            assert float(max(np.max(np.abs(d.real)), np.max(np.abs(d.imag)))) <= tol, (n, t, b)


@pytest.mark.gpu
def test_rotated_and_conjugated_plaintexts_land_where_the_galois_element_says(pkg):
    """fhe_rns_automorphism with fhe_galois_element(n, r) is a cyclic left rotation of the slots by r, the element 2n - 1 conjugates them;
    on plaintexts, no keys."""
    n, scale = 2048, float(2 ** 40)
    z, m, E = generic_case(n)
    moduli = [nm.ntt_primes(60, n, 1)[0], nm.ntt_primes(30, n, 1)[0]]
    e = _engine(pkg, n, moduli)
    enc = pkg.capi.CkksEncoder(e)
    got, _ = _encode(pkg, e, enc, z, scale)
    dp = pkg.DeviceBuffer.from_numpy(got)
    rot = pkg.DeviceBuffer(got.nbytes)
    dz = pkg.DeviceBuffer(3 * n * 8)
    for r, want in ((1, np.roll(z, -1, axis=1)), (5, np.roll(z, -5, axis=1)), (-3, np.roll(z, 3, axis=1)), (None, np.conj(z))):
        g = 2 * n - 1 if r is None else pkg.galois_element(n, r)
        e.automorphism(rot, dp, g, 3)
        enc.decode_poly(dz, rot, scale, 3)
        out = dz.download((3, n // 2, 2), np.float64)
        for b in range(3):
            assert float(np.max(np.abs(out[b, :, 0] + 1j * out[b, :, 1] - want[b]))) <= decode_tol(n, scale, want[b]), (r, b)


# ------------------------------------------------------------------------------------------------ 4. determinism
@pytest.mark.gpu
@pytest.mark.parametrize("n", [2048, 16384])
def test_a_plaintext_does_not_depend_on_its_batch(pkg, n):
    z, m, E = generic_case(n)
    scale = float(2 ** 50)
    moduli = mixed_moduli(n)[0]
    e = _engine(pkg, n, moduli)
    enc = pkg.capi.CkksEncoder(e)
    all3, bits3 = _encode(pkg, e, enc, z, scale)
    words = all3[:, 2, :, 0].copy()                                       # some words: limb 2, the 64-bit prime
    dec3 = _decode_words(pkg, enc, words, moduli[2], scale)
    for b in range(3):
        one, bits1 = _encode(pkg, e, enc, z[b:b + 1], scale)
        assert np.array_equal(one[0], all3[b]) and bits1[0] == bits3[b]
        dec1 = _decode_words(pkg, enc, words[b:b + 1], moduli[2], scale)
        assert dec1[0].tobytes() == dec3[b].tobytes()


# ------------------------------------------------------------------------------------------------ 5. rejections
@pytest.mark.gpu
def test_rejections_leave_poisoned_outputs_alone_and_calls_stay_inside_their_buffers(pkg):
    n, L, batch, scale = 2048, 3, 3, float(2 ** 28)                        # |c| < q_0 / 2 for slots in the unit square: decode_poly is valid
    moduli = nm.ntt_primes(30, n, L)
    e, other = _engine(pkg, n, moduli), _engine(pkg, n, moduli)
    enc = pkg.capi.CkksEncoder(e)
    lib = pkg.lib()
    z, m, E = generic_case(n)
    S = L * n * 32
    arena = memcheck.GuardedArena(pkg, [("slots", batch * n * 8), ("poly", batch * S), ("bits", batch * 4), ("back", batch * n * 8), ("words", batch * n * 8)], S)
    arena["slots"].upload(_slots_array(z))
    arena["words"].upload(np.arange(batch * n, dtype=np.uint64))
    for name in ("poly", "bits", "back"):
        arena[name].poison()
    P = lambda name: arena[name].ptr
    before = e.workspace_bytes()
    enc_call = lambda h=e.h, c=enc.h, o=P("poly"), bt=P("bits"), s=P("slots"), sc=scale, b=batch: lib.fhe_ckks_encode(h, c, o, bt, s, sc, b)
    dec_call = lambda h=e.h, c=enc.h, o=P("back"), s=P("words"), t=T63, sc=scale, b=batch: lib.fhe_ckks_decode(h, c, o, s, t, sc, b)
    pol_call = lambda h=e.h, c=enc.h, o=P("back"), s=P("poly"), sc=scale, b=batch: lib.fhe_ckks_decode_poly(h, c, o, s, sc, b)
    bad_scales = (0.0, -1.0, float("inf"), float("nan"))
    bad = [enc_call(h=None), enc_call(c=None), enc_call(o=None), enc_call(s=None), enc_call(h=other.h), enc_call(b=0), enc_call(o=P("poly") + 8),
           enc_call(s=P("slots") + 4), enc_call(bt=P("bits") + 2), enc_call(o=P("slots")), enc_call(bt=P("slots")), enc_call(bt=P("poly") + 16),
           *[enc_call(sc=s) for s in bad_scales],
           dec_call(h=None), dec_call(c=None), dec_call(o=None), dec_call(s=None), dec_call(h=other.h), dec_call(b=0), dec_call(o=P("back") + 4),
           dec_call(s=P("words") + 4), dec_call(o=P("words")), dec_call(o=P("words") + 8 * n), *[dec_call(sc=s) for s in bad_scales],
           pol_call(h=None), pol_call(c=None), pol_call(o=None), pol_call(s=None), pol_call(h=other.h), pol_call(b=0), pol_call(o=P("back") + 4),
           pol_call(s=P("poly") + 8), pol_call(o=P("poly")), *[pol_call(sc=s) for s in bad_scales]]
    assert bad == [INVALID] * len(bad), bad
    arena.verify(inputs=("slots", "words"))
    for name, shape, dt in (("poly", (batch, L, n, 4), np.uint64), ("bits", (batch,), np.uint32), ("back", (batch, n), np.uint64)):
        assert memcheck.is_poison(arena[name].download(shape, dt)), name
    assert enc_call(bt=None) == 0                                         # d_coeff_bits is optional
    arena.verify(inputs=("slots", "words"))
    assert memcheck.is_poison(arena["bits"].download((batch,), np.uint32))
    first = arena["poly"].download((batch, L, n, 4))
    assert enc_call() == 0 and pol_call() == 0
    arena.verify(inputs=("slots", "words"))
    assert np.array_equal(arena["poly"].download((batch, L, n, 4)), first)
    want, wbits = _encode(pkg, e, enc, z, scale)
    assert np.array_equal(first, want) and np.array_equal(arena["bits"].download((batch,), np.uint32), wbits)
    out = arena["back"].download((batch, n // 2, 2), np.float64)
    for b in range(batch):
        assert float(np.max(np.abs(out[b, :, 0] + 1j * out[b, :, 1] - z[b]))) <= decode_tol(n, scale, z[b]), b
    assert dec_call() == 0
    arena.verify(inputs=("slots", "words"))
    assert np.array_equal(arena["poly"].download((batch, L, n, 4)), first)   # decode left the plaintexts alone
    assert e.workspace_bytes() == before                                  # no workspace, nothing allocated
    arena.free()


@pytest.mark.gpu
def test_creation_supports_n_2048_to_16384_and_word_sized_moduli_only(pkg):
    lib = pkg.lib()
    out = ctypes.c_void_p(0x1234)
    for n in (1024, 32768):
        e = _engine(pkg, n, nm.ntt_primes(30, n, 2))
        assert lib.fhe_ckks_encoder_create(e.h, ctypes.byref(out)) == UNSUPPORTED and out.value == 0x1234, n
    wide = _engine(pkg, 2048, nm.ntt_primes(120, 2048, 2))
    assert lib.fhe_ckks_encoder_create(wide.h, ctypes.byref(out)) == UNSUPPORTED and out.value == 0x1234
    e = _engine(pkg, 2048, nm.ntt_primes(30, 2048, 2))
    assert lib.fhe_ckks_encoder_create(e.h, None) == INVALID


# ------------------------------------------------------------------------------------------------ 6. end to end
def e2e_setup(pkg, oracle, n=2048, L=3, w=16, seed=31):
    """Engines on three and on two 30-bit primes, the keys on both, and the encoder on both (shared with test_ckks_capture.py)."""
    from test_encrypt import _embed, _keygen
    moduli = nm.ntt_primes(30, n, L)
    s, pk0, pk1 = _keygen(oracle, n, moduli, 2, seed)
    e3, e2 = _engine(pkg, n, moduli), _engine(pkg, n, moduli[:-1])
    keep = [pkg.DeviceBuffer.from_numpy(pk0), pkg.DeviceBuffer.from_numpy(pk1), pkg.DeviceBuffer.from_numpy(_embed(s[None], moduli)[0]),
            pkg.DeviceBuffer.from_numpy(_embed(s[None], moduli[:-1])[0])]
    pk = e3.import_public_key(keep[0], keep[1])
    sk3, sk2 = e3.import_secret_key(keep[2]), e2.import_secret_key(keep[3])
    g1 = pkg.galois_element(n, 1)
    rk, gk = e3.generate_keyswitch_keys(sk3, w, [0, g1], 1, 3.2, (101, 202))
    return dict(n=n, moduli=moduli, e3=e3, e2=e2, pk=pk, sk3=sk3, sk2=sk2, rk=rk, gk=gk, g1=g1, keep=keep,
                enc3=pkg.capi.CkksEncoder(e3), enc2=pkg.capi.CkksEncoder(e2))


def check_product(n, v, decoded, z_want, scale_out, what):
    """The two assertions of the end-to-end cases: with e = v - round(scale_out m^model(z_want)), |decoded_k - z_want_k| <= |e|_1 / scale_out +
    the decode tolerance, and max |e| < scale_out 2^-8 (a wrong slot map, a missing conjugate or a missing rescale gives |e| ~ scale_out)."""
    for b in range(len(v)):
        m = cm.encode(z_want[b], n)
        want = np.array([int(np.rint(x)) for x in LD(scale_out) * m], dtype=object)
        err = v[b] - want
        emax, e1 = max(abs(int(x)) for x in err), sum(abs(int(x)) for x in err)
        mv = np.array([LD(int(x)) for x in v[b]]) / LD(scale_out)
        zc = cm.decode(mv)
        tol = (n / 2 + 1) / scale_out + 4 * cm.float64_decode_error(mv.astype(np.float64), zc)
        d = decoded[b].astype(CLD) - np.asarray(z_want[b]).astype(CLD)
        dmax = float(np.max(np.abs(d)))
        print(f"{what} b={b}: max |e| = 2^{math.log2(max(emax, 1)):.1f} (scale_out 2^{math.log2(scale_out):.2f}), |e|_1 / scale_out = {e1 / scale_out:.3e}, "
              f"max slot error = {dmax:.3e} = 2^{math.log2(max(dmax, 1e-300)):.1f}")
        assert emax < scale_out * 2.0 ** -8, (what, b, emax)
        assert dmax <= e1 / scale_out + tol, (what, b, dmax)


@pytest.mark.gpu
def test_encode_encrypt_multiply_rescale_rotate_decrypt_decode(pkg, oracle):
    """n = 2048, three 30-bit primes, w = 16, batch 2, scale 2^30: encode two vectors, fhe_ct_encrypt (t = 2), fhe_ct_multiply_relin,
    fhe_rns_rescale_drop_last on both components, fhe_ct_decrypt on the two-limb engine (t = 2^63, scale 1), decode at 2^60 / q_last; then the
    same with one rotation by 1 through fhe_ct_apply_galois before the rescale."""
    S = e2e_setup(pkg, oracle)
    n, moduli, e3, e2, batch, scale = S["n"], S["moduli"], S["e3"], S["e2"], 2, float(2 ** 30)
    rng = np.random.default_rng(99)
    z1 = rng.random((batch, n // 2)) + 1j * rng.random((batch, n // 2))
    z2 = rng.random((batch, n // 2)) + 1j * rng.random((batch, n // 2))
    nb3, nb2 = batch * 3 * n * 32, batch * 2 * n * 32
    cts = []
    for i, z in enumerate((z1, z2)):
        dm, o0, o1 = pkg.DeviceBuffer(nb3), pkg.DeviceBuffer(nb3), pkg.DeviceBuffer(nb3)
        S["enc3"].encode(dm, pkg.DeviceBuffer.from_numpy(_slots_array(z)), scale, batch)
        e3.encrypt(S["pk"], 2, 3.2, (11 + 10 * i, 12 + 10 * i, 13 + 10 * i), o0, o1, dm, batch)
        cts.append((o0, o1))
    p0, p1 = pkg.DeviceBuffer(nb3), pkg.DeviceBuffer(nb3)
    e3.ct_multiply_relin(S["rk"], p0, p1, cts[0][0], cts[0][1], cts[1][0], cts[1][1], batch)
    q0, q1 = pkg.DeviceBuffer(nb3), pkg.DeviceBuffer(nb3)
    e3.apply_galois(S["gk"], S["g1"], q0, q1, p0, p1, batch)
    scale_out = scale * scale / moduli[-1]
    for what, (c0, c1), want in (("product", (p0, p1), z1 * z2), ("rotated product", (q0, q1), np.roll(z1 * z2, -1, axis=1))):
        r0, r1 = pkg.DeviceBuffer(nb2), pkg.DeviceBuffer(nb2)
        e3.rescale_drop_last(r0, c0, batch); e3.rescale_drop_last(r1, c1, batch)
        dw, dz = pkg.DeviceBuffer(batch * n * 8), pkg.DeviceBuffer(batch * n * 8)
        e2.decrypt(S["sk2"], T63, 1, dw, None, [r0, r1], batch)
        S["enc2"].decode(dz, dw, T63, scale_out, batch)
        words = dw.download((batch, n)).astype(object)
        v = np.where(words > T63 // 2, words - T63, words)
        out = dz.download((batch, n // 2, 2), np.float64)
        check_product(n, v, out[..., 0] + 1j * out[..., 1], want, scale_out, what)
