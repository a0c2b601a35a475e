"""The CKKS encoder at its edges (fhe_ckks_encode, fhe_ckks_decode, fhe_ckks_decode_poly): ties, bit lengths and residues up to the contract's
edge, saturation, decode centring, 8-byte slot alignment, many workgroups.

Most of it is bit for bit, through the exact family of ckks_model.family_slots: z_k = x + i y (x - i y where c(k)) has the plaintext
m = x + y X^(n/2), and neither transform rounds once on it (every butterfly adds two equal values or multiplies a zero; the only twiddles
that meet a non-zero value are omega^0 = zeta^0 = 1; scale / h is a power of two when scale is).  So c_0 = rne(scale x), c_(n/2) = rne(scale y),
every other coefficient is 0, and words that are non-zero at 0 and n/2 only decode to (v_0 +- i v_(n/2)) / scale.  The model reproduces the
family with np.array_equal in both precisions (test_ckks_model.py), so the expectations below are plain Python integers.
The tolerance cases keep the rules of test_ckks_encoder.py: encode 1/2 + 4 scale E, decode 4 E (the inputs here are integers: no rounding
term), E the error of the float64 numpy formula against the long-double reference on the same input."""
import math
from fractions import Fraction

import numpy as np
import pytest

import ckks_model as cm
import memcheck
import ntt_math as nm
from test_ckks_encoder import SIZES, T63, _decode_words, _encode, _engine, _signed, _slots_array, generic_case, mixed_moduli

LD, CLD = cm.LD, cm.CLD
EDGE_SIZES = [2048, 16384]                                       # the smallest and the largest instance
T64 = 1 << 64


def family_batch(n, pairs):
    return np.stack([cm.family_slots(n, x, y) for x, y in pairs])


def family_containers(n, moduli, c0, ch):
    """[batch][L][n][4] containers and [batch] bit lengths of the plaintexts c0[b] + ch[b] X^(n/2) (Python integers)."""
    want = np.zeros((len(c0), len(moduli), n, 4), dtype=np.uint64)
    for l, q in enumerate(moduli):
        want[:, l, 0, 0] = np.array([int(c) % q for c in c0], dtype=np.uint64)
        want[:, l, n // 2, 0] = np.array([int(c) % q for c in ch], dtype=np.uint64)
    return want, np.array([max(abs(int(a)), abs(int(b))).bit_length() for a, b in zip(c0, ch)], dtype=np.uint32)


def rne(value, scale):
    """round-to-nearest-even of the exact rational value * scale: Python's round() of a Fraction."""
    return round(Fraction(value) * Fraction(scale))


def centred(w, t):
    """The header's rule, written from the header: t == 0 two's complement; else w > t/2 (integer t/2) stands for w - t."""
    if t == 0:
        return w - T64 if w >= 1 << 63 else w
    return w - t if w > t // 2 else w


def family_decoded(n, v0, vh, scale):
    """[h] complex128: (v0 + i vh) / scale, conjugated where c(k); float() of a Python integer rounds to nearest even, as the device's
    conversion does, and the division by a power of two is exact."""
    return cm.family_slots(n, float(v0) / scale, float(vh) / scale)


def same_bits(got, want):
    """Bitwise equality of the real and imaginary parts once -0.0 is normalised to +0.0."""
    g, w = np.asarray(got, dtype=np.complex128), np.asarray(want, dtype=np.complex128)
    return (g.real + 0.0).tobytes() == (w.real + 0.0).tobytes() and (g.imag + 0.0).tobytes() == (w.imag + 0.0).tobytes()


# ------------------------------------------------------------------------------------------------ 1. ties and signs
def tie_values():
    """Products scale * x that the rounding has to get right.  Ties k + 1/2 up to the last one a double can hold: doubles in [2^52, 2^53) are
    spaced 1 apart, so the literals 2^52 + 0.5 and 2^52 + 1.5 ARE the integers 2^52 and 2^52 + 2 (kept: an integer must pass unchanged), and the
    largest true ties are 2^51 + 0.5 and 2^52 - 0.5, added here with the odd integers just above 2^52, where floor(v + 0.5) is off by one.
    Near-ties: every representable 0.5 +- k 2^-53, k = 1, 2, and the two neighbours of 0.5."""
    ties = [0.5, 1.5, 2.5, 3.5]
    v = [s * t for t in ties for s in (1.0, -1.0)]
    v += [2.0 ** 52 + 0.5, 2.0 ** 52 + 1.5, -(2.0 ** 52 + 0.5)]
    v += [2.0 ** 51 + 0.5, -(2.0 ** 51 + 0.5), 2.0 ** 51 + 1.5, 2.0 ** 52 - 0.5, -(2.0 ** 52 - 0.5), 2.0 ** 52 - 1.5]
    v += [2.0 ** 52 + 1, -(2.0 ** 52 + 1), 2.0 ** 53 - 1, -(2.0 ** 53 - 1)]
    near = [0.5 - 2.0 ** -54, 0.5 - 2.0 ** -53, 0.5 - 2.0 ** -52, 0.5 + 2.0 ** -53, 0.5 + 2.0 ** -52]
    assert near[0] == math.nextafter(0.5, 0.0) and near[3] == math.nextafter(0.5, 1.0) and all(x != 0.5 for x in near)
    v += [s * x for x in near for s in (1.0, -1.0)]
    v += [1.5 - 2.0 ** -52, -(1.5 - 2.0 ** -52), 2.5 + 2.0 ** -51, -(2.5 + 2.0 ** -51)]
    return v + [0.0, -0.0]


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_ties_round_to_even_in_both_planes_and_both_signs(pkg, n, scale):
    """Plaintext i has x = v_i / scale and y = v_(i+1) / scale (cyclically): every value once in each plane.  Every word of every container is
    compared: a negative coefficient is q - |c|, -0.0 and every other coefficient store 0, and d_coeff_bits follows."""
    v = tie_values()
    xs = [t / scale for t in v]
    assert all(Fraction(x) * Fraction(scale) == Fraction(t) for x, t in zip(xs, v))
    pairs = list(zip(xs, xs[1:] + xs[:1]))
    c0, ch = [rne(x, scale) for x, _ in pairs], [rne(y, scale) for _, y in pairs]
    assert rne(0.5, 1.0) == 0 and rne(1.5, 1.0) == 2 and rne(-2.5, 1.0) == -2 and rne(-3.5, 1.0) == -4 and rne(2.0 ** 52 - 0.5, 1.0) == 1 << 52
    z = family_batch(n, pairs)
    for moduli in mixed_moduli(n):
        e = _engine(pkg, n, moduli)
        got, bits = _encode(pkg, e, pkg.capi.CkksEncoder(e), z, scale)
        want, wbits = family_containers(n, moduli, c0, ch)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (n, scale, moduli, [(int(b), pairs[b], int(got[b, l, j, w]), int(want[b, l, j, w])) for b, l, j, w in bad[:4]])
        assert np.array_equal(bits, wbits), (bits, wbits)


# ------------------------------------------------------------------------------------------------ 2. bit length and residues
def magnitudes():
    m = [0, 1]
    for k in (1, 20, 29, 30, 31, 32, 52):
        m += [(1 << k) - 1, 1 << k]
    return m + [1 << k for k in (53, 59, 60, 61)] + [(1 << 62) - 512]


def magnitude_pairs():
    """Per magnitude four plaintexts: +m and -m in the real plane, +m and -m in the imaginary one; in two of them the other coordinate is the
    larger (2^bit_length(m), one bit more; left out where that would pass 62 bits), in two the smaller (m >> 1, one bit less), with the other
    sign.  Then the two zero plaintexts of either sign."""
    pairs = []
    for m in magnitudes():
        small, big = m >> 1, 1 << m.bit_length()
        if big.bit_length() > 62:
            big = small
        pairs += [(m, -small), (-m, big), (-big, m), (small, -m)]
    pairs = [(float(x), float(y)) for x, y in pairs]
    assert all(float(int(x)) == x and float(int(y)) == y for x, y in pairs)
    return pairs + [(0.0, 0.0), (-0.0, -0.0), (0.0, -0.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_bit_lengths_and_residues_up_to_62_bits(pkg, n):
    """Scale 1: bits 0 (all residues 0) to 62, 2^k - 1 against 2^k, residues int(c) % q in Python under a 30-bit (shift 34), a 40-bit and a
    60-bit prime, and under the two largest 64-bit primes (shift 0) with a 30-bit one."""
    pairs = magnitude_pairs()
    c0, ch = [int(x) for x, _ in pairs], [int(y) for _, y in pairs]
    z = family_batch(n, pairs)
    p30 = nm.ntt_primes(30, n, 2)
    for moduli in ([p30[0], nm.ntt_primes(40, n, 1)[0], nm.ntt_primes(60, n, 1)[0]], nm.largest_ntt_primes(64, n, 2) + [p30[1]]):
        e = _engine(pkg, n, moduli)
        got, bits = _encode(pkg, e, pkg.capi.CkksEncoder(e), z, 1.0)
        want, wbits = family_containers(n, moduli, c0, ch)
        assert {0, 1, 2, 20, 21, 29, 30, 31, 32, 33, 52, 53, 54, 60, 61, 62} <= set(int(b) for b in wbits) and int(wbits.max()) == 62
        assert np.array_equal(bits, wbits), (n, moduli, [(pairs[b], int(bits[b]), int(wbits[b])) for b in np.flatnonzero(bits != wbits)[:6]])
        bad = np.argwhere(got != want)
        assert bad.size == 0, (n, moduli, [(pairs[b], int(l), int(j), int(got[b, l, j, w]), int(want[b, l, j, w])) for b, l, j, w in bad[:4]])
        e.check_canonical(pkg.DeviceBuffer.from_numpy(got), len(pairs))


# ------------------------------------------------------------------------------------------------ 3. saturation and non-finite slots
@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_saturating_and_non_finite_plaintexts_report_63_or_64_bits_and_leave_their_neighbours_alone(pkg, n):
    """Above 62 bits the residues are unspecified, the reported bit length is not, and the containers stay canonical.  Scale 2^30; the odd
    plaintexts of the batch saturate, the even ones are ordinary and must not notice."""
    scale = float(2 ** 30)
    z3, _, _ = generic_case(n)
    h = n // 2

    def poked(part, k, value):
        z = z3[1].copy()
        if part:
            z.imag[k] = value
        else:
            z.real[k] = value
        return z

    def encode(zz):
        """_encode of test_ckks_encoder.py, with the input compared as words afterwards (NaN is not equal to itself)."""
        batch = len(zz)
        dz = pkg.DeviceBuffer.from_numpy(_slots_array(zz))
        do, db = pkg.DeviceBuffer(batch * e.L * n * 32), pkg.DeviceBuffer(batch * 4)
        memcheck.poison(pkg, do); memcheck.poison(pkg, db)
        enc.encode(do, dz, scale, batch, db)                              # raises unless FHE_OK
        out = do.download((batch, e.L, n, 4)), db.download((batch,), np.uint32)
        assert np.array_equal(dz.download((batch, h, 2), np.uint64), _slots_array(zz).view(np.uint64))
        return out

    odd = [(cm.family_slots(n, 2.0 ** 32, 1.0), 63), (cm.family_slots(n, 2.0 ** 33, -1.0), 64), (cm.family_slots(n, -2.0 ** 33, 2.0 ** 20), 64),
           (cm.family_slots(n, 1e300, 0.0), 64), (poked(0, 5, np.inf), 64), (poked(0, h - 1, -np.inf), 64), (poked(1, h // 2 + 1, np.nan), 64),
           (z3[2] * 2.0 ** 40, 64)]
    z = np.empty((2 * len(odd), h), dtype=np.complex128)
    z[0::2] = z3[np.arange(len(odd)) % 3]
    z[1::2] = np.stack([s for s, _ in odd])
    moduli = mixed_moduli(n)[0]
    e = _engine(pkg, n, moduli)
    enc = pkg.capi.CkksEncoder(e)
    got, bits = encode(z)
    assert [int(b) for b in bits[1::2]] == [w for _, w in odd], bits
    e.check_canonical(pkg.DeviceBuffer.from_numpy(got), len(z))
    alone, abits = encode(z[0::2])
    assert np.array_equal(got[0::2], alone) and np.array_equal(bits[0::2], abits)
    assert all(0 < int(b) <= 31 for b in abits), abits                    # ordinary: |c| <= 2^30 (|m_j| <= 1 for slots in the unit square)
    later, lbits = _encode(pkg, e, enc, family_batch(n, [(3.0, -5.0)]), scale)
    want, wbits = family_containers(n, moduli, [3 << 30], [-5 << 30])
    assert np.array_equal(later, want) and np.array_equal(lbits, wbits)


# ------------------------------------------------------------------------------------------------ 4. decode centring
DECODE_WORDS = [(T63, [0, 1, (1 << 62) - 1, 1 << 62, (1 << 62) + 1, (1 << 63) - 1, (1 << 53) + 1]),
                (0, [0, 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, T64 - 1]),
                (2, [0, 1]), (3, [0, 1, 2]),
                ((1 << 50) + 55, [(1 << 49) + 27, (1 << 49) + 28, (1 << 50) + 54])]


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_decode_centres_the_words_around_half_the_modulus_exactly(pkg, n):
    """Words that are non-zero at coefficients 0 and n/2 only: slot k is exactly (v_0 +- i v_(n/2)) / scale with v the centred integers.
    Plaintext i holds word i at 0 and word i + 1 at n/2.  2^53 + 1 (and 2^62 +- 1, 2^63 - 1) round in the conversion to double: float() of the
    Python integer rounds the same way, to nearest even."""
    e = _engine(pkg, n, nm.ntt_primes(30, n, 1))
    enc = pkg.capi.CkksEncoder(e)
    assert centred(1, 2) == 1 and centred(2, 3) == -1 and centred(1 << 62, T63) == 1 << 62 and centred((1 << 62) + 1, T63) == 1 - (1 << 62)
    assert centred(1 << 63, 0) == -(1 << 63) and centred((1 << 63) - 1, 0) == (1 << 63) - 1 and float((1 << 53) + 1) == 2.0 ** 53
    for t, ws in DECODE_WORDS:
        t_odd = (1 << 50) + 55
        assert t != t_odd or ws == [(t - 1) // 2, (t + 1) // 2, t - 1]
        words = np.zeros((len(ws), n), dtype=np.uint64)
        words[:, 0] = np.array(ws, dtype=np.uint64)
        words[:, n // 2] = np.array(ws[1:] + ws[:1], dtype=np.uint64)
        for scale in (1.0, float(2 ** 40)):
            got = _decode_words(pkg, enc, words, t, scale)
            for b, (w0, wh) in enumerate(zip(ws, ws[1:] + ws[:1])):
                want = family_decoded(n, centred(w0, t), centred(wh, t), scale)
                assert same_bits(got[b], want), (n, t, scale, w0, wh, got[b, :2], want[:2])


def _decode_poly(pkg, e, enc, poly, scale):
    batch, L, n, _ = poly.shape
    dp = pkg.DeviceBuffer.from_numpy(poly)
    dz = pkg.DeviceBuffer(batch * n * 8)
    memcheck.poison(pkg, dz)
    e.check_canonical(dp, batch)
    enc.decode_poly(dz, dp, scale, batch)
    out = dz.download((batch, n // 2, 2), np.float64)
    assert np.array_equal(dp.download((batch, L, n, 4)), poly)
    return out[..., 0] + 1j * out[..., 1]


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_decode_poly_reads_limb_0_of_its_own_plaintext_centred_modulo_q0(pkg, n, L):
    """q_0 a 30-bit, a 60-bit and the largest 64-bit prime (there (double)w rounds).  With L = 3 the other limbs hold other residues at every
    coefficient: were one of them read, or limb 0 of another plaintext, the slots would differ.  The upper container words stay zero (the
    containers are canonical)."""
    others = [nm.ntt_primes(30, n, 2)[1], nm.ntt_primes(40, n, 1)[0]][:L - 1]
    rng = np.random.default_rng(n + L)
    for q in (nm.ntt_primes(30, n, 1)[0], nm.ntt_primes(60, n, 1)[0], nm.largest_ntt_primes(64, n, 1)[0]):
        moduli = [q] + others
        ws = [0, 1, (q - 1) // 2, (q + 1) // 2, q - 1]
        poly = np.zeros((len(ws), L, n, 4), dtype=np.uint64)
        poly[:, 0, 0, 0] = np.array(ws, dtype=np.uint64)
        poly[:, 0, n // 2, 0] = np.array(ws[1:] + ws[:1], dtype=np.uint64)
        for l in range(1, L):
            poly[:, l, :, 0] = rng.integers(1, moduli[l], (len(ws), n), dtype=np.uint64)
        e = _engine(pkg, n, moduli)
        enc = pkg.capi.CkksEncoder(e)
        for scale in (1.0, float(2 ** 40)):
            got = _decode_poly(pkg, e, enc, poly, scale)
            for b, (w0, wh) in enumerate(zip(ws, ws[1:] + ws[:1])):
                want = family_decoded(n, centred(w0, q), centred(wh, q), scale)
                assert same_bits(got[b], want), (n, L, q, scale, w0, wh, got[b, :2], want[:2])


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_decode_of_one_large_coefficient_matches_the_closed_form(pkg, n):
    """m = 2^61 X^j: z_k = 2^61 zeta^(j e(k)) / scale, evaluated directly in long double.  Tolerance 4 E, E the float64 model's error on the same
    input against the same closed form; the input is an integer, so the rule's rounding term does not apply."""
    scale, v = float(2 ** 40), 1 << 61
    js = [1, 15, 16, n // 2 - 1, n // 2 + 1, n - 1]
    words = np.zeros((len(js), n), dtype=np.uint64)
    words[np.arange(len(js)), js] = v
    e = _engine(pkg, n, nm.ntt_primes(30, n, 1))
    got = _decode_words(pkg, pkg.capi.CkksEncoder(e), words, T63, scale)
    for b, j in enumerate(js):
        want = cm.impulse_slots(n, j, LD(v) / LD(scale))
        m = np.zeros(n)
        m[j] = v / scale
        E = cm.float64_decode_error(m, want)
        d = got[b].astype(CLD) - want
        err = float(max(np.max(np.abs(d.real)), np.max(np.abs(d.imag))))
        print(f"n={n} j={j}: max slot error {err:.3e}, E(numpy float64) = {E:.3e}, ratio {err / E:.3f} (allowed 4), |z| = 2^21")
        assert err <= 4 * E, (n, j, err, E)


# ------------------------------------------------------------------------------------------------ 5. impulses through encode
_impulse = {}


def impulse_case(n):
    """One unit slot, z = delta_k and i delta_k for k in {0, 1, h/2, h - 1}: the slots, the closed-form m (checked against the model here, on
    the CPU, before the device is asked) and E per plaintext, computed once."""
    if n not in _impulse:
        h = n // 2
        ks = [(k, zk) for k in (0, 1, h // 2, h - 1) for zk in (1.0, 1j)]
        z = np.zeros((len(ks), h), dtype=np.complex128)
        m, E = [], []
        for b, (k, zk) in enumerate(ks):
            z[b, k] = zk
            m.append(cm.impulse_plaintext(n, k, zk))
            model = cm.encode(z[b], n)
            assert float(np.max(np.abs(model - m[b]))) <= 16 * float(np.finfo(LD).eps) * 2 / n, (n, k, zk)
            E.append(cm.float64_error(z[b], n, model))
        _impulse[n] = (ks, z, m, E)
    return _impulse[n]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_unit_slots_encode_to_the_closed_form_of_their_row(pkg, n):
    """c_j against round(scale (2/n) Re(z_k zeta^(-j e(k)))) for every j: the gather table and every twist entry against direct evaluation, not
    against the model's own transform.  1/2 + 4 scale E, scale 2^40."""
    ks, z, m, E = impulse_case(n)
    scale = float(2 ** 40)
    moduli = [nm.ntt_primes(60, n, 1)[0], nm.ntt_primes(30, n, 1)[0]]
    e = _engine(pkg, n, moduli)
    got, bits = _encode(pkg, e, pkg.capi.CkksEncoder(e), z, scale)
    for b, (k, zk) in enumerate(ks):
        c = _signed(got[b, 0], moduli[0])
        err = float(np.max(np.abs(np.array([LD(int(x)) for x in c]) - LD(scale) * m[b])))
        print(f"n={n} k={k} z_k={zk}: max |c - scale m| - 1/2 = {err - 0.5:.3e}, scale*E(numpy float64) = {scale * E[b]:.3e}")
        assert err <= 0.5 + 4 * scale * E[b], (n, k, zk, err)
        assert np.array_equal(got[b, 1, :, 0], np.array([int(x) % moduli[1] for x in c], dtype=np.uint64))
        assert int(bits[b]) == max(abs(int(x)) for x in c).bit_length()


# ------------------------------------------------------------------------------------------------ 6. large generic coefficients
def _generic_body(pkg, n, scale, moduli, what):
    z, m, E = generic_case(n)
    e = _engine(pkg, n, moduli)
    got, bits = _encode(pkg, e, pkg.capi.CkksEncoder(e), z, scale)
    for b in range(3):
        c = _signed(got[b, 0], moduli[0])
        err = float(np.max(np.abs(np.array([LD(int(x)) for x in c]) - LD(scale) * m[b])))
        top = max(abs(int(x)) for x in c)
        print(f"n={n} scale={what} b={b}: max |c - scale m| - 1/2 = {err - 0.5:.3e}, scale*E(numpy float64) = {scale * E[b]:.3e}, "
              f"ratio {(err - 0.5) / (scale * E[b]):.3f} (allowed 4), max |c| = 2^{math.log2(top):.2f}")
        assert err <= 0.5 + 4 * scale * E[b], (n, what, b)
        assert np.array_equal(got[b, 1, :, 0], np.array([int(x) % moduli[1] for x in c], dtype=np.uint64))
        assert int(bits[b]) == top.bit_length()
        assert top < 1 << 62


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_generic_slots_at_scale_2_to_61_round_within_the_rule_and_reduce_exactly(pkg, n):
    """|c| ~ 2^60 under the largest 64-bit prime (limb 0, so that the centred value fits) and a 30-bit prime: limb 1 must be c mod q_1 for the
    c read from limb 0, the bits those of max |c|."""
    _generic_body(pkg, n, float(2 ** 61), [nm.largest_ntt_primes(64, n, 1)[0], nm.ntt_primes(30, n, 1)[0]], "2^61")


@pytest.mark.gpu
def test_a_scale_that_is_no_power_of_two_and_the_smallest_positive_scale(pkg):
    n = 2048
    moduli = [nm.ntt_primes(60, n, 1)[0], nm.ntt_primes(30, n, 1)[0]]
    _generic_body(pkg, n, 1e12 + 0.5, moduli, "1e12+0.5")
    z, _, _ = generic_case(n)
    e = _engine(pkg, n, moduli)
    got, bits = _encode(pkg, e, pkg.capi.CkksEncoder(e), z, 5e-324)       # finite and positive: accepted
    assert not got.any() and not bits.any()


# ------------------------------------------------------------------------------------------------ 7. slots at 8-byte alignment
def _padded(data, fill):
    """8 bytes of `fill`, the bytes of `data` (or that many poison bytes when data is an int), 8 bytes of `fill`, 8 spare: a slice whose
    payload starts 8 bytes past its 32-byte-aligned start."""
    body = np.full(data, memcheck.POISON_BYTE, np.uint8) if isinstance(data, int) else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    pad = np.full(8, fill, np.uint8)
    return np.concatenate([pad, body, pad, pad])


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_slots_and_words_at_8_byte_alignment_give_the_aligned_results(pkg, n):
    """d_slots (in for encode, out for both decoders) and d_m at a 16-byte-aligned address + 8: bit for bit the results of the aligned calls on
    the same data, nothing written outside the buffers (guard bands, and the 8 bytes on either side of each shifted payload)."""
    batch, L, scale = 2, 2, float(2 ** 40)
    moduli = [nm.ntt_primes(60, n, 1)[0], nm.ntt_primes(30, n, 1)[0]]
    e = _engine(pkg, n, moduli)
    enc = pkg.capi.CkksEncoder(e)
    lib = pkg.lib()
    z, _, _ = generic_case(n)
    slots = _slots_array(z[:batch])
    nz, S = batch * n * 8, L * n * 32
    ref, rbits = _encode(pkg, e, enc, z[:batch], scale)
    words = np.ascontiguousarray(ref[:, 0, :, 0])
    ref_poly = _decode_poly(pkg, e, enc, ref, scale)
    ref_words = _decode_words(pkg, enc, words, moduli[0], scale)
    arena = memcheck.GuardedArena(pkg, [("slots8", nz + 24), ("poly", batch * S), ("bits", batch * 4), ("back8_poly", nz + 24), ("back8_words", nz + 24),
                                        ("words", nz), ("words8", nz + 24), ("back_words8", nz)], S)
    arena["slots8"].upload(_padded(slots, 0xC3))
    arena["words"].upload(words)
    arena["words8"].upload(_padded(words, 0xC3))
    for name in ("back8_poly", "back8_words"):
        arena[name].upload(_padded(nz, 0x3C))
    for name in ("poly", "bits", "back_words8"):
        arena[name].poison()
    P = lambda name: arena[name].ptr
    for name in ("slots8", "back8_poly", "back8_words", "words8"):
        assert P(name) % 16 == 0 and (P(name) + 8) % 16 == 8
    assert lib.fhe_ckks_encode(e.h, enc.h, P("poly"), P("bits"), P("slots8") + 8, scale, batch) == 0
    assert lib.fhe_ckks_decode_poly(e.h, enc.h, P("back8_poly") + 8, P("poly"), scale, batch) == 0
    assert lib.fhe_ckks_decode(e.h, enc.h, P("back8_words") + 8, P("words"), moduli[0], scale, batch) == 0
    assert lib.fhe_ckks_decode(e.h, enc.h, P("back_words8"), P("words8") + 8, moduli[0], scale, batch) == 0
    arena.verify(inputs=("slots8", "words", "words8"))
    assert np.array_equal(arena["poly"].download((batch, L, n, 4)), ref)
    assert np.array_equal(arena["bits"].download((batch,), np.uint32), rbits)
    for name, want in (("back8_poly", ref_poly), ("back8_words", ref_words)):
        raw = arena[name].download((nz + 24,), np.uint8)
        assert (raw[:8] == 0x3C).all() and (raw[nz + 8:] == 0x3C).all(), name
        out = raw[8:nz + 8].copy().view(np.float64).reshape(batch, n // 2, 2)
        assert (out[..., 0] + 1j * out[..., 1]).tobytes() == want.tobytes(), name
    out = arena["back_words8"].download((batch, n // 2, 2), np.float64)
    assert (out[..., 0] + 1j * out[..., 1]).tobytes() == ref_words.tobytes()
    arena.free()


# ------------------------------------------------------------------------------------------------ 8. many workgroups
@pytest.mark.gpu
def test_a_batch_of_1031_plaintexts_has_every_coefficient_residue_and_bit_length_in_closed_form(pkg):
    """n = 2048, one 30-bit limb, batch 1031: more workgroups than the CUs hold at once, a multiple of nothing.  Plaintext b is the exact
    family with x = b - 515 and y = b 2^20 + (b & 1) / 2 at scale 1: c_0 = b - 515 (both signs, 0 at b = 515), c_(n/2) = b 2^20 (the tie goes
    to the even side; above q for most b).  Then the same words go through fhe_ckks_decode with t = q."""
    n, batch = 2048, 1031
    q = nm.ntt_primes(30, n, 1)[0]
    e = _engine(pkg, n, [q])
    enc = pkg.capi.CkksEncoder(e)
    b = np.arange(batch, dtype=np.int64)
    x, y = (b - 515).astype(np.float64), (b << 20) + 0.5 * (b & 1)
    assert np.array_equal((y - (b << 20)) * 2, b & 1)                     # the halves are representable
    c = cm.slot_table(n)[1]
    z = x[:, None] + 1j * np.where(c[None, :] == 1, -y[:, None], y[:, None])
    c0, ch = b - 515, b << 20
    got, bits = _encode(pkg, e, enc, z, 1.0)
    want = np.zeros((batch, 1, n, 4), dtype=np.uint64)
    want[:, 0, 0, 0] = (c0 % q).astype(np.uint64)                         # numpy's % of a positive modulus is non-negative
    want[:, 0, n // 2, 0] = (ch % q).astype(np.uint64)
    top = np.maximum(np.abs(c0), ch)
    wbits = np.where(top > 0, np.frexp(top.astype(np.float64))[1], 0).astype(np.uint32)   # frexp's exponent of an integer < 2^53 is its bit length
    assert int(wbits[0]) == 10 and int(wbits[1]) == 21 and int(wbits[1030]) == (1030 << 20).bit_length()
    assert np.array_equal(bits, wbits), np.flatnonzero(bits != wbits)[:8]
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    words = np.ascontiguousarray(got[:, 0, :, 0])
    back = _decode_words(pkg, enc, words, q, 1.0)
    v0, vh = want[:, 0, 0, 0].astype(np.int64), want[:, 0, n // 2, 0].astype(np.int64)
    v0, vh = np.where(v0 > q // 2, v0 - q, v0).astype(np.float64), np.where(vh > q // 2, vh - q, vh).astype(np.float64)
    assert np.array_equal(back.real + 0.0, np.broadcast_to(v0[:, None], back.shape) + 0.0)
    assert np.array_equal(back.imag + 0.0, np.where(c[None, :] == 1, -vh[:, None], vh[:, None]) + 0.0)
