"""Key-switching key generation (fhe_keyswitch_keys_generate, fhe_relin_keys_export) on every instance of ntt_keygen_kernel beyond L = 2, at the
edges of its ranges and tables, and on every route around the kernel.

tests/test_keygen.py runs L = 2, K = 2 (K = 1 and 5 once), bottom-of-class moduli (one pair of largest 64-bit primes), the 39-entry table,
at most two sets and a uniformly random s.  What is added here, test by test (every case is one entry of CASES below; the path it must take is
listed beside it and pinned by test_every_case_takes_the_path_it_was_written_for):

  instances     all sixteen (field, N): test_every_fused_instance_with_three_limbs_span_moduli_three_sets (L = 3, K = 2)
  L and K       L = 1 (every workgroup a gadget workgroup) and L = 5, K = 3: test_one_and_five_limbs_three_digits; L = 3 above; K = 4 and 8:
                test_gadget_factors; K = 40 and 43: test_unpacked_key_sets_on_a_word_sized_class; K = 1 with 27 sets at n = 16384
  moduli        SPAN (L - 1 primes from the top of a class, the smallest one bit below its limit; 64-bit class: 64, 64, 63 bits) in the instance,
                table and noise-scale tests; a top prime beside a narrow one (12289, 31 and 41 bits): test_gadget_factors; the 14- and 16-bit
                pair: test_smallest_moduli
  secret        limb 0 random, limb 1 all q - 1, limb 2 zero (instances, consumers, N >= 2^15); ternary (test_the_default_galois_set); random
  gadget        2^(k w) >= q_j, so that the reduction of the factor does something, on all four fields, and k w = 63 (w = 21, K = 4 and
                w = 9, K = 8): test_gadget_factors
  tables        1, 8, 64, 1024 entries on all four fields (sigma = 85.3 draws magnitudes above 255): test_table_lengths; 1025 entries
                (composed): test_a_table_one_entry_too_long
  noise_scale   1, q_0 (vanishes in limb 0), q_0 + 1 and 2^64 - 59 on the span bases of all four classes: test_noise_scales
  elements      [0, 2n - 1, 5] at every size; [3, 0] (the relinearisation key second); the default Galois set (0, 5^i and 5^-i for i a power of
                two below n / 2, 2n - 1: 21 sets at n = 2048, 27 at n = 16384): test_the_default_galois_set, and its prefixes:
                test_a_prefix_of_the_default_galois_set_gives_the_same_sets
  paths         fused: everything above unless marked; composed by the switch (one child process for every n = 2048 case of the instance,
                limb and gadget tests): test_the_composed_path_gives_the_same_bits_on_every_edge_case; composed by itself at N = 2^15 (4-byte:
                packed afterwards; 8-byte: containers), N = 2^16, the full-width class with L = 3, and a table of 1025 entries:
                test_sizes_and_classes_that_take_the_composed_path; unpacked sets on a word-sized class (digits that do not fit; more than 83
                products on the FP64 field) with their packed neighbour: test_unpacked_key_sets_on_a_word_sized_class
  consumers     relinearize, apply_galois and the hoisted rotation at every size on a 4-byte and an 8-byte field, generated set against imported
                rows, and the export afterwards: test_consumers_at_every_size_and_through_the_hoisted_kernels

Every expected row comes from the CPU oracle (_expected of test_keygen.py: RnsPlan.sample_uniform, inverse, sample_gaussian, polymul) and Python
integers, once per module; every comparison is np.array_equal on whole arrays through fhe_relin_keys_export into poisoned outputs.
test_the_reference_rows_by_hand_for_three_limbs pins _expected itself for L = 3 against schoolbook products.

Not tested: the fallback of the uniform draw after 64 rejections (probability about 2^-64 per draw; no real stream reaches it, and the kernel
offers no way to hand it a crafted one), and hipGraph capture of the call (it allocates)."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

import ntt_math as nm
from test_encrypt import _ints
from test_encrypt_edges import SIGMA_LEN, SMALLEST, T_BIG, _span
from test_keygen import SEEDS, SIGMA, T, _case, _expected, _export, _exports, _generate, _primes
from test_top_of_range import BITS, LOW_BITS, WIDTH
from workload import rns_poly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W2 = {30: 15, 43: 22, 62: 31, 64: 32}                  # K = 2 on a class's widest modulus
W3 = {30: 10, 43: 15, 62: 21, 64: 22}                  # K = 3
MAX_TABLE = 1024                                       # entries of a cumulative table the kernel admits (fhe_dev::ENCRYPT_MAX_CDT)

# n, moduli, decomp_bits, elements, secret ('random': rns_poly(90), as _case of test_keygen.py; 'edges': limb 0 random, limb 1 all q - 1,
# every further limb zero; 'ternary': the oracle's sampler), noise_scale, sigma
Case = collections.namedtuple("Case", "n moduli w elts s noise_scale sigma")


def _mk(n, moduli, w, elts, s="random", noise_scale=T, sigma=SIGMA):
    return Case(n, tuple(moduli), w, tuple(elts), s, noise_scale, sigma)


def _top1(bits, n):
    return nm.largest_ntt_primes(bits, n, 1)


def _galois_set(n):
    """What a user generates: the relinearisation key, the rotations by powers of two in both directions, the row swap."""
    out, i = [0], 1
    while i < n // 2:
        g = pow(5, i, 2 * n)
        out += [g, pow(g, -1, 2 * n)] if i < n // 4 else [g]                                   # 5^(n / 4) is its own inverse
        i *= 2
    return out + [2 * n - 1]


def _scale(name, moduli):
    return {"1": 1, "q0": moduli[0], "q0+1": moduli[0] + 1, "2^64-59": T_BIG}[name]


N0 = 2048
FUSED, COMPOSED = True, False
# Every GPU case of this file: id -> (Case, the path the documented rule must give for it).
CASES = {}
INSTANCE_IDS = [(bits, log_n) for bits in BITS for log_n in (11, 12, 13, 14)]
for bits, log_n in INSTANCE_IDS:
    CASES["instance", bits, log_n] = (_mk(1 << log_n, _span(bits, 1 << log_n, 3), W2[bits], [0, (2 << log_n) - 1, 5], "edges"), FUSED)
LIMB_IDS = [(bits, L) for bits in BITS for L in (1, 5)]
for bits, L in LIMB_IDS:
    CASES["limbs", bits, L] = (_mk(N0, _top1(bits, N0) if L == 1 else _span(bits, N0, L), W3[bits], [3, 0]), FUSED)
# the class's top prime beside a narrow one: (moduli, w).  The last two reach k w = 63.
GADGET = {"30-with-12289": (_top1(30, N0) + [12289], 10), "43-with-31-bit": (_top1(43, N0) + nm.ntt_primes(31, N0, 1), 16),
          "62-with-41-bit": (_top1(62, N0) + nm.ntt_primes(41, N0, 1), 21), "64-with-41-bit": (_top1(64, N0) + nm.ntt_primes(41, N0, 1), 22),
          "64-span-shift-63": (_span(64, N0, 2), 21), "64-with-41-bit-shift-63": (_top1(64, N0) + nm.ntt_primes(41, N0, 1), 9)}
for name, (moduli, w) in GADGET.items():
    CASES["gadget", name] = (_mk(N0, moduli, w, [0, 3]), FUSED)
TABLE_IDS = [(bits, sigma) for bits in BITS for sigma in (0.08, 0.66, 5.3, 85.3)]
for bits, sigma in TABLE_IDS:
    CASES["table", bits, sigma] = (_mk(N0, _span(bits, N0, 2), W2[bits], [0, 3], sigma=sigma), FUSED)
for bits in (30, 64):
    CASES["long-table", bits] = (_mk(N0, _span(bits, N0, 2), W2[bits], [0, 3], sigma=85.4), COMPOSED)
CASES["smallest",] = (_mk(N0, SMALLEST, 4, [0, 3]), FUSED)
SCALE_IDS = [(bits, name) for bits in BITS for name in ("1", "q0", "q0+1", "2^64-59")]
for bits, name in SCALE_IDS:
    CASES["scale", bits, name] = (_mk(N0, _span(bits, N0, 2), W2[bits], [0, 3], noise_scale=_scale(name, _span(bits, N0, 2))), FUSED)
MANY_IDS = [(30, 2048), (30, 16384), (64, 2048)]
for bits, n in MANY_IDS:
    CASES["many", bits, n] = (_mk(n, _span(bits, n, 2), W2[bits] if n == N0 else 30, _galois_set(n), "ternary"), FUSED)      # K = 1 at the large size
BY_ITSELF = {"4-byte-2^15": _mk(1 << 15, _span(30, 1 << 15, 3), W2[30], [0, (1 << 16) - 1, 5], "edges"),
             "lazy-64-bit-2^15": _mk(1 << 15, _span(62, 1 << 15, 3), W2[62], [0, (1 << 16) - 1, 5], "edges"),
             "4-byte-2^16": _mk(1 << 16, _span(30, 1 << 16, 2), W2[30], [(1 << 17) - 1, 0], "edges"),          # L = 2, two sets: the oracle's time
             "full-width-120-bit": _mk(N0, _primes(120, N0, 3), 61, [0, 2 * N0 - 1, 5])}
for name, c in BY_ITSELF.items():
    CASES["by-itself", name] = (c, COMPOSED)
# (Case, packed, fused)
UNPACKED = {"digits-do-not-fit": (_mk(N0, [12289] + _top1(30, N0), 30, [0, 3]), False, COMPOSED),
            "86-products-fp64": (_mk(N0, _span(43, N0, 2), 1, [0, 3]), False, COMPOSED),
            "80-products-fp64": (_mk(N0, nm.ntt_primes(40, N0, 2), 1, [0, 3]), True, FUSED)}
for name, (c, _, fused) in UNPACKED.items():
    CASES["unpacked", name] = (c, fused)
AGAIN = [k for k in CASES if k[0] in ("instance", "limbs", "gadget") and CASES[k][0].n == N0]      # under the switch, in one child process


# ------------------------------------------------------------------------------------------------ the documented rule, mirrored
def _class(c):
    """The class limit of the word-sized field a base runs on, None for the full-width class."""
    if not 11 <= c.n.bit_length() - 1 <= 16:
        return None
    return next((b for b in BITS if max(q.bit_length() for q in c.moduli) <= b), None)


def _digits(c):
    return -(-max(q.bit_length() for q in c.moduli) // c.w)


def _packed(c):
    """keys_get_packed: a word-sized class at a size with one-launch transforms, digits that fit the other limbs' transforms (integer fields) or
    at most 83 products (FP64 field), tables below 4 GiB."""
    cls, log_n, L, K = _class(c), c.n.bit_length() - 1, len(c.moduli), _digits(c)
    if cls is None or log_n > (15 if cls == 30 else 14):
        return False
    if cls == 43:
        fit = L * K <= 83
    else:
        fit = min(1 << c.w, max(c.moduli)) <= (1 if cls == 64 else 4) * min(c.moduli)
    return fit and L * K * L * c.n * (4 if cls == 30 else 8) < 1 << 32


def _fused(oracle, c):
    return _packed(c) and 11 <= c.n.bit_length() - 1 <= 14 and len(oracle.gaussian_cdt(c.sigma)) <= MAX_TABLE


# ------------------------------------------------------------------------------------------------ expectations and runs, once per module
_cache, _got = {}, {}


def _secret(oracle, c):
    if c.s == "ternary":
        return oracle.RnsPlan(c.n, list(c.moduli)).sample_ternary(0.5, 4242, 1)[0]
    s = rns_poly(90, list(c.moduli), c.n, 1)[0]
    if c.s == "edges":
        s[1:] = 0
        s[1, :, 0] = np.uint64(c.moduli[1] - 1)
    return s


def _kw(c):
    return {k: v for k, v, d in (("noise_scale", c.noise_scale, T), ("sigma", c.sigma, SIGMA)) if v != d}


def _want(oracle, c):
    """(s, b, a) of a case; random secrets through _case of test_keygen.py, whose cache the two files share."""
    if c.s == "random":
        return _case(oracle, c.n, list(c.moduli), c.w, list(c.elts), **_kw(c))
    if c not in _cache:
        s = _secret(oracle, c)
        _cache[c] = (s,) + _expected(oracle, c.n, list(c.moduli), c.w, list(c.elts), s, **_kw(c))
    return _cache[c]


def _run(pkg, c, s):
    return _exports(pkg, c.n, list(c.moduli), c.w, list(c.elts), s, **_kw(c))


def _check(pkg, oracle, key):
    c = CASES[key][0]
    s, wb, wa = _want(oracle, c)
    if key not in _got:
        _got[key] = _run(pkg, c, s)
    gb, ga = _got[key]
    assert gb.shape == wb.shape == (len(c.elts), len(c.moduli) * _digits(c), len(c.moduli), c.n, 4)
    assert np.array_equal(ga, wa), key
    assert np.array_equal(gb, wb), key
    return gb, ga


def _noise_magnitudes(oracle, c):
    """|e_P| of the call's Gaussian stream, as Python integers."""
    num = len(c.elts) * len(c.moduli) * _digits(c)
    e = _ints(oracle.RnsPlan(c.n, list(c.moduli)).sample_gaussian(c.sigma, SEEDS[1], num)[:, 0])
    return np.where(e > c.moduli[0] // 2, c.moduli[0] - e, e)


# ------------------------------------------------------------------------------------------------ CPU
def test_the_inputs_sit_on_the_edges_they_are_meant_to_hit(oracle):
    for sigma, length in ((0.08, 1), (0.66, 8), (5.3, 64), (85.3, 1024), (85.4, 1025)):
        assert len(oracle.gaussian_cdt(sigma)) == length == SIGMA_LEN[sigma], sigma
    assert MAX_TABLE == 1024
    for bits in BITS:                                                                          # the streams of the table cases themselves
        assert 255 < int(_noise_magnitudes(oracle, CASES["table", bits, 85.3][0]).max()) <= 1024, bits
        assert int(_noise_magnitudes(oracle, CASES["table", bits, 0.08][0]).max()) == 0, bits
    for name in GADGET:                                                                        # some 2^(k w) >= q_j: the % q of the factor acts
        c = CASES["gadget", name][0]
        assert any(1 << (k * c.w) >= q for q in c.moduli for k in range(_digits(c))), name
        assert (_digits(c) - 1) * c.w < 64, name
    for name in ("64-span-shift-63", "64-with-41-bit-shift-63"):
        c = CASES["gadget", name][0]
        assert (_digits(c) - 1) * c.w == 63 and _packed(c), name
    assert [_digits(CASES["gadget", name][0]) for name in GADGET] == [3, 3, 3, 3, 4, 8]
    for bits in BITS:                                                                          # top, ..., top, bottom of the class's top bit
        for n in (2048, 4096, 8192, 16384):
            q = _span(bits, n, 3)
            assert [x.bit_length() for x in q] == [bits, bits, LOW_BITS[bits]], (bits, n)
            assert q[2] - (1 << (LOW_BITS[bits] - 1)) < 1 << 24 and (1 << bits) - q[0] < 1 << 24, (bits, n)
            assert all(x % (2 * n) == 1 and nm.is_prime(x) for x in q)
    assert [x.bit_length() for x in _span(64, N0, 3)] == [64, 64, 63]
    for bits in BITS:
        q = _span(bits, N0, 2)
        assert CASES["scale", bits, "q0"][0].noise_scale == q[0] and CASES["scale", bits, "q0+1"][0].noise_scale == q[0] + 1 < 1 << 64
        assert CASES["scale", bits, "2^64-59"][0].noise_scale == (1 << 64) - 59 > max(q)
        if bits != 30:                                                                         # the 8-byte fields: wider than every modulus
            assert all(CASES["scale", bits, name][0].noise_scale > max(q) for name in ("q0+1", "2^64-59"))
    assert CASES["smallest",][0].moduli == (12289, 40961) == tuple(nm.ntt_primes(14, N0, 2)) and len(oracle.gaussian_cdt(SIGMA)) == 39 < 12289
    for bits, n in MANY_IDS:
        elts = CASES["many", bits, n][0].elts
        assert len(elts) == 2 * (n.bit_length() - 2) + 1 == len(set(elts)) and elts[0] == 0 and elts[-1] == 2 * n - 1
        assert elts[1] == 5 and elts[-2] == pow(5, n // 4, 2 * n) and elts[-2] ** 2 % (2 * n) == 1
        assert all(g % 2 == 1 and g * elts[i + 1] % (2 * n) == 1 for i, g in enumerate(elts[1:-2], 1) if i % 2)
    s = _secret(oracle, CASES["many", 30, 2048][0])                                            # an actual ternary key: 0, 1, q - 1
    for l, q in enumerate(CASES["many", 30, 2048][0].moduli):
        assert set(_ints(s[l]).tolist()) == {0, 1, q - 1}
    c = CASES["instance", 64, 11][0]
    s = _ints(_secret(oracle, c))
    assert set(s[1].tolist()) == {c.moduli[1] - 1} and set(s[2].tolist()) == {0} and len(set(s[0].tolist())) > 2000


def test_every_case_takes_the_path_it_was_written_for(oracle):
    """The library does not report the path.  This is the documented rule (include/fhe_hip.h; keys_get_packed) in Python, asserted for every GPU
    case of this file, so that a case written for the kernel fails here if a change of parameters moves it to the composition."""
    for key, (c, fused) in CASES.items():
        assert _fused(oracle, c) == fused, key
    assert sum(fused for _, fused in CASES.values()) == 16 + 8 + 6 + 16 + 1 + 16 + 3 + 1 and len(CASES) == 67 + 2 + 4 + 2
    for key in AGAIN:
        assert CASES[key][1] == FUSED
    assert len(AGAIN) == 4 + 8 + 6
    assert {_class(CASES["instance", bits, log_n][0]) for bits, log_n in INSTANCE_IDS} == set(BITS)
    for name, (c, packed, fused) in UNPACKED.items():                                          # word-sized classes, and why they are not packed
        assert _class(c) == (30 if name == "digits-do-not-fit" else 43) and _packed(c) == packed, name
    c = UNPACKED["digits-do-not-fit"][0]
    assert _digits(c) == 1 and min(1 << c.w, max(c.moduli)) > 4 * min(c.moduli)
    assert [len(UNPACKED[k][0].moduli) * _digits(UNPACKED[k][0]) for k in ("86-products-fp64", "80-products-fp64")] == [86, 80]
    # composed by themselves: packed afterwards on the 4-byte class at N = 2^15 (unpack_keys_kernel exports), containers elsewhere
    assert [_packed(c) for c in BY_ITSELF.values()] == [True, False, False, False]
    assert [_class(c) for c in BY_ITSELF.values()] == [30, 62, 30, None]
    assert all(_packed(CASES["long-table", bits][0]) for bits in (30, 64))


def _sigma_by_hand(v, q, g):
    n, out = len(v), [0] * len(v)
    for i, x in enumerate(v):
        k = i * g % (2 * n)
        out[k % n] = x if k < n else (q - x) % q
    return out


def test_the_reference_rows_by_hand_for_three_limbs(oracle):
    """n = 32, L = 3, K = 2, noise_scale = q_0: the noise vanishes from limb 0, where every b row is -a s plus the gadget term alone, here from
    schoolbook products and a loop over the exponents; limbs 1 and 2 differ from that.  a is the inverse transform of the uniform stream."""
    n, w, elts = 32, 15, [0, 3, 2 * 32 - 1]
    moduli = nm.largest_ntt_primes(30, n, 2) + nm.ntt_primes(30, n, 1)
    L, K = 3, 2
    s = rns_poly(90, moduli, n, 1)[0]
    wb, wa = _expected(oracle, n, moduli, w, elts, s, noise_scale=moduli[0])
    rp = oracle.RnsPlan(n, moduli)
    assert rp.num_digits(w) == K and wb.shape == (3, L * K, L, n, 4)
    a = _ints(rp.inverse(rp.sample_uniform(SEEDS[0], len(elts) * L * K), threads=2)).reshape(3, L * K, L, n)
    assert np.array_equal(_ints(wa), a)
    si, b = _ints(s), _ints(wb)
    differ = 0
    for e, g in enumerate(elts):
        for r in range(L * K):
            j, k = divmod(r, K)
            for l, q in enumerate(moduli):
                sl = [int(x) for x in si[l]]
                row = [(q - x) % q for x in nm.negacyclic_mul_direct([int(x) for x in a[e, r, l]], sl, q)]
                if l == j:
                    tgt = nm.negacyclic_mul_direct(sl, sl, q) if g == 0 else _sigma_by_hand(sl, q, g)
                    row = [(x + (1 << (k * w)) % q * y) % q for x, y in zip(row, tgt)]
                if l == 0:
                    assert [int(x) for x in b[e, r, l]] == row, (e, r)
                else:
                    differ += [int(x) for x in b[e, r, l]] != row
    assert differ == 3 * L * K * 2


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("bits,log_n", INSTANCE_IDS)
def test_every_fused_instance_with_three_limbs_span_moduli_three_sets(pkg, oracle, bits, log_n):
    """L = 3, K = 2: the block index splits by 3, 6 and 2, the rows lie (row 3 + l) n apart; elements 0, 2n - 1 and 5; s random, all q - 1, zero."""
    c = CASES["instance", bits, log_n][0]
    assert pkg.RnsNttEngine(c.n, list(c.moduli)).width_class == WIDTH[bits]
    _check(pkg, oracle, ("instance", bits, log_n))


@pytest.mark.gpu
@pytest.mark.parametrize("bits,L", LIMB_IDS)
def test_one_and_five_limbs_three_digits(pkg, oracle, bits, L):
    """L = 1: j = 0 always, every workgroup adds a gadget term.  L = 5, K = 3: fifteen rows of five limbs per set.  Elements [3, 0]."""
    _check(pkg, oracle, ("limbs", bits, L))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GADGET))
def test_gadget_factors(pkg, oracle, name):
    """2^(k w) at or above the narrow modulus of the base (reduced before it is used), and k w = 63 (the shift at its limit, the top bit set)."""
    _check(pkg, oracle, ("gadget", name))


@pytest.mark.gpu
@pytest.mark.parametrize("bits,sigma", TABLE_IDS)
def test_table_lengths(pkg, oracle, bits, sigma):
    _check(pkg, oracle, ("table", bits, sigma))


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [30, 64])
def test_a_table_one_entry_too_long(pkg, oracle, bits):
    _check(pkg, oracle, ("long-table", bits))


@pytest.mark.gpu
def test_smallest_moduli(pkg, oracle):
    """q = 12289 and 40961, w = 4: rejection masks of 14 and 16 bits, noise_scale = 65537 above both moduli."""
    _check(pkg, oracle, ("smallest",))


@pytest.mark.gpu
@pytest.mark.parametrize("bits,name", SCALE_IDS)
def test_noise_scales(pkg, oracle, bits, name):
    gb, _ = _check(pkg, oracle, ("scale", bits, name))
    if name == "q0":                                   # no noise in limb 0: the row without it, from the oracle's polymul
        c = CASES["scale", bits, name][0]
        s, wb, wa = _want(oracle, c)
        clean = _expected(oracle, c.n, list(c.moduli), c.w, list(c.elts), s, noise_scale=c.noise_scale, sigma=0.08)[0]
        assert np.array_equal(gb[:, :, 0], clean[:, :, 0]) and not np.array_equal(gb[:, :, 1], clean[:, :, 1])


@pytest.mark.gpu
@pytest.mark.parametrize("bits,n", MANY_IDS)
def test_the_default_galois_set(pkg, oracle, bits, n):
    """About 2 log2(n) sets from one launch, a ternary secret: every set equals the oracle's, and no two are alike."""
    gb, _ = _check(pkg, oracle, ("many", bits, n))
    assert len({gb[e].tobytes() for e in range(gb.shape[0])}) == gb.shape[0]


@pytest.mark.gpu
@pytest.mark.parametrize("bits,n", MANY_IDS)
def test_a_prefix_of_the_default_galois_set_gives_the_same_sets(pkg, oracle, bits, n):
    """The sets of a call for the first E - 1 elements, and for the first alone, are the bits of the call for all E (the streams are indexed by
    the polynomial, not by the call): test_one_set_equals_the_first_of_two up to the last set."""
    gb, ga = _check(pkg, oracle, ("many", bits, n))
    c = CASES["many", bits, n][0]
    s = _want(oracle, c)[0]
    for count in (len(c.elts) - 1, 1):
        pb, pa = _run(pkg, c._replace(elts=c.elts[:count]), s)
        assert pb.shape[0] == count and np.array_equal(pb, gb[:count]) and np.array_equal(pa, ga[:count]), count


CHILD = """import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import importlib
import numpy as np
pkg = importlib.import_module("gpu-homomorphic-encryption_amd")
import test_keygen_edges as t
out = {{}}
for i, key in enumerate(t.AGAIN):
    c = t.CASES[key][0]
    out[f"b_{{i}}"], out[f"a_{{i}}"] = t._run(pkg, c, t._secret(None, c))
np.savez(sys.argv[1], **out)
"""


@pytest.mark.gpu
def test_the_composed_path_gives_the_same_bits_on_every_edge_case(pkg, oracle, tmp_path):
    """FHE_HIP_NO_FUSED_KEYGEN=1 in ONE child process (the switch is read at engine creation) for every n = 2048 case of the instance, limb and
    gadget tests: the exports equal the oracle's rows and the fused path's."""
    (tmp_path / "child.py").write_text(CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests")))
    env = dict(os.environ, FHE_HIP_NO_FUSED_KEYGEN="1")
    res = subprocess.run([sys.executable, str(tmp_path / "child.py"), str(tmp_path / "out.npz")], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    got = np.load(tmp_path / "out.npz")
    assert len(got.files) == 2 * len(AGAIN)
    for i, key in enumerate(AGAIN):
        fb, fa = _check(pkg, oracle, key)
        _, wb, wa = _want(oracle, CASES[key][0])
        assert np.array_equal(got[f"a_{i}"], wa) and np.array_equal(got[f"b_{i}"], wb), key
        assert np.array_equal(got[f"a_{i}"], fa) and np.array_equal(got[f"b_{i}"], fb), key


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BY_ITSELF))
def test_sizes_and_classes_that_take_the_composed_path(pkg, oracle, name):
    """L = 3 and three sets: sample_uniform_from starts at polynomials 18 and 36 of the stream (N = 2^16: L = 2, two sets, polynomial 8).
    N = 2^15 on the 4-byte class packs the set afterwards (the export unpacks it); the 8-byte class there, N = 2^16 and the full-width class
    keep containers (the export copies them)."""
    _check(pkg, oracle, ("by-itself", name))


def _relinearized(pkg, e, keys, ct):
    d = [pkg.DeviceBuffer.from_numpy(x) for x in ct]
    e.relinearize(keys, d[0], d[1], d[2], 1)
    return [d[0].download(ct[0].shape), d[1].download(ct[0].shape)]


def _imported(pkg, e, w, wb, wa):
    return [e.import_relin_keys(w, [pkg.DeviceBuffer.from_numpy(r) for r in wb[i]], [pkg.DeviceBuffer.from_numpy(r) for r in wa[i]]) for i in range(len(wb))]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(UNPACKED))
def test_unpacked_key_sets_on_a_word_sized_class(pkg, oracle, name):
    """12289 beside a 30-bit prime with w = 30 (a digit of the wide limb does not fit the narrow limb's transform), and the FP64 field with
    L K = 86 products: the sets keep containers, generation composes, the export copies.  L K = 80 is the packed, fused neighbour.  Then
    fhe_ct_relinearize with the generated set against the same call with fhe_relin_keys_create of the oracle's rows."""
    c = CASES["unpacked", name][0]
    moduli = list(c.moduli)
    s, wb, wa = _want(oracle, c)
    e, sets, _keep = _generate(pkg, c.n, moduli, c.w, list(c.elts), s)
    assert e.width_class == WIDTH[_class(c)]
    LK = len(moduli) * e.relin_num_digits(c.w)
    assert LK == len(moduli) * _digits(c)
    ct = [rns_poly(70 + i, moduli, c.n, 1) for i in range(3)]
    mine, theirs = _relinearized(pkg, e, sets[0], ct), _relinearized(pkg, e, _imported(pkg, e, c.w, wb[:1], wa[:1])[0], ct)
    assert np.array_equal(mine[0], theirs[0]) and np.array_equal(mine[1], theirs[1])
    assert not np.array_equal(mine[0], ct[0]) and not np.array_equal(mine[1], ct[1])
    for i, rk in enumerate(sets):
        gb, ga = _export(pkg, e, rk, c.n, len(moduli), LK)
        assert np.array_equal(ga, wa[i]) and np.array_equal(gb, wb[i]), i


@pytest.mark.gpu
@pytest.mark.parametrize("log_n", [11, 12, 13, 14])
@pytest.mark.parametrize("bits", [30, 64])
def test_consumers_at_every_size_and_through_the_hoisted_kernels(pkg, oracle, bits, log_n):
    """The sets of the instance test (elements 0, 2n - 1, 5) against fhe_relin_keys_create of the oracle's rows: relinearize, apply_galois(5),
    one hoist and the hoisted rotations by 2n - 1 and 5 give identical outputs, which differ from their inputs; the export afterwards still
    equals the oracle's rows."""
    c = CASES["instance", bits, log_n][0]
    n, moduli, g = c.n, list(c.moduli), 5
    s, wb, wa = _want(oracle, c)
    e, sets, _keep = _generate(pkg, n, moduli, c.w, list(c.elts), s)
    ct = [rns_poly(70 + i, moduli, n, 1) for i in range(3)]
    res = []
    for keys in (sets, _imported(pkg, e, c.w, wb, wa)):
        out = _relinearized(pkg, e, keys[0], ct)
        d0, d1 = pkg.DeviceBuffer.from_numpy(ct[0]), pkg.DeviceBuffer.from_numpy(ct[1])
        o0, o1 = pkg.DeviceBuffer(ct[0].nbytes), pkg.DeviceBuffer(ct[0].nbytes)
        e.apply_galois(keys[2], g, o0, o1, d0, d1, 1)
        out += [o0.download(ct[0].shape), o1.download(ct[0].shape)]
        e.hoist(c.w, d1, 1)
        for idx in (1, 2):
            e.apply_galois_hoisted(keys[idx], c.elts[idx], o0, o1, d0, 1)
            out += [o0.download(ct[0].shape), o1.download(ct[0].shape)]
        res.append(out)
    assert len(res[0]) == 8
    for i, (x, y) in enumerate(zip(*res)):
        assert np.array_equal(x, y), i
        assert not np.array_equal(x, ct[i % 2]), i
    LK = len(moduli) * _digits(c)
    for i, rk in enumerate(sets):
        gb, ga = _export(pkg, e, rk, n, len(moduli), LK)
        assert np.array_equal(ga, wa[i]) and np.array_equal(gb, wb[i]), i
