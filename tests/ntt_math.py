"""Independent pure-Python big-integer helpers for the tests (neither oracle nor product code).

Closed forms of the reference primitives, a Miller-Rabin prime search, and the
direct O(n^2) definitions of the negacyclic transform / product that both the oracle and the HIP
engine are checked against.
"""
import random

R_BITS = 256
R = 1 << R_BITS
M256 = R - 1
M64 = (1 << 64) - 1


# ---- closed forms of the leaf primitives (include/bigint.cuh:27-140) ---------------------------
def add_mod_ref(a, b, q):
    s = (a + b) & M256
    t = (s - q) & M256
    return s if (t >> 192) > (s >> 192) else t        # top-limb borrow test (D15)


def sub_mod_ref(a, b, q):
    d = (a - b) & M256
    return (d + q) & M256 if (d >> 192) > (a >> 192) else d


def mont_inverse_ref(q):
    inv, n0 = 1, q & M64
    for _ in range(6):
        inv = (inv * (2 - n0 * inv)) & M64
    return (-inv) & M64


def mont_mul_ref(a, b, q, inv0=None):
    """Limb-wise SOS reduction exactly as written (valid for garbage inv0 / unreduced inputs too)."""
    if inv0 is None:
        inv0 = mont_inverse_ref(q)
    t = a * b                                           # < 2^512
    for i in range(4):
        m = (((t >> (64 * i)) & M64) * inv0) & M64
        t = (t + ((m * q) << (64 * i))) & ((1 << 512) - 1)   # carry out of limb 7 is lost
    u = t >> 256
    d = (u - q) & M256
    return u if (d >> 192) > (u >> 192) else d


def ct_ref(a, b, w, q):
    t = mont_mul_ref(b, w, q)
    return add_mod_ref(a, t, q), sub_mod_ref(a, t, q)


def gs_ref(a, b, w, q):
    return add_mod_ref(a, b, q), mont_mul_ref(sub_mod_ref(a, b, q), w, q)


# ---- primes ---------------------------------------------------------------------------------
def is_prime(n, rounds=24):
    if n < 2:
        return False
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for p in small:
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2; s += 1
    rng = random.Random(0xC0FFEE ^ (n & 0xFFFFFFFF))
    bases = list(small) + [rng.randrange(2, n - 1) for _ in range(rounds)]
    for a in bases:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def ntt_primes(bits, n, count):
    """The `count` smallest primes >= 2^(bits-1) with q = 1 (mod 2n)  (SURVEY.md section 8d)."""
    out, step = [], 2 * n
    q = ((1 << (bits - 1)) // step) * step + 1
    while q < (1 << (bits - 1)):
        q += step
    while len(out) < count:
        if is_prime(q):
            out.append(q)
        q += step
    return out


def largest_ntt_primes(bits, n, count):
    """The `count` largest primes below 2^bits with q = 1 (mod 2n): the top of a width class's range."""
    out, step = [], 2 * n
    q = ((1 << bits) // step) * step + 1
    while q >= (1 << bits):
        q -= step
    while len(out) < count:
        if is_prime(q):
            out.append(q)
        q -= step
    return out


def words32(q):
    """q as little-endian 32-bit words, up to and including its top non-zero word."""
    return [(q >> (32 * i)) & 0xFFFFFFFF for i in range((q.bit_length() + 31) // 32)]


def has_generic_words(q):
    """Every 32-bit word of q below its top word is neither 0 nor 0xFFFFFFFF: no term m_i * q_j of a word-wise Montgomery product is
    a product by zero, and no borrow or carry passes a word of q for free."""
    return all(w not in (0, 0xFFFFFFFF) for w in words32(q)[:-1])


def generic_ntt_primes(bits, n, count, seed):
    """`count` distinct primes of exactly `bits` bits with q = 1 (mod 2n) and generic words (has_generic_words), drawn from
    random.Random(seed): deterministic for a seed.  ntt_primes / largest_ntt_primes return 2^(bits-1) + small and 2^bits - small, whose
    middle words are all zeros or all ones; these are the moduli in between."""
    rng = random.Random(seed)
    out, step = [], 2 * n
    while len(out) < count:
        k = rng.getrandbits(bits) | (1 << (bits - 1))
        q = (k // step) * step + 1
        if q.bit_length() == bits and has_generic_words(q) and q not in out and is_prime(q):
            out.append(q)
    return out


GENERIC_BITS = (65, 100, 127, 128, 129, 192, 193, 250, 255)     # see full_width_moduli
_FULL_WIDTH_SETS = {}


def full_width_moduli(name, n):
    """The moduli sets of the full-width class tests (FHE_WIDTH_256), cached per (name, n).
      'g<bits>'  two generic primes of that width.  65 is the first width above the word-sized classes; 127 the top of the two-limb
                 transforms and 128 the bottom of the four-limb ones; 128 / 129 and 192 / 193 put q's top bit at the top of a 64-bit limb
                 or at the bottom of the next; 250 and 255 are the lazy and the canonical tops.
      't<bits>'  the two largest primes below 2^bits (127, 128, 255): sums at the container limit.
      'g85x3'    three generic 85-bit primes whose product has 255 bits, the largest a CRT result may have (the first seed from 85 that gives one).
      'mixed-a'  generic 250-bit + generic 100-bit + the smallest 60-bit prime: a full-width basis that also holds a limb below 2^64.
      'mixed-b'  generic 127-bit + generic 122-bit: a two-limb basis that is not lazy (the widest modulus decides)."""
    key = (name, n)
    if key not in _FULL_WIDTH_SETS:
        if name == "mixed-a":
            qs = generic_ntt_primes(250, n, 1, 250) + generic_ntt_primes(100, n, 1, 100) + ntt_primes(60, n, 1)
        elif name == "mixed-b":
            qs = generic_ntt_primes(127, n, 1, 127) + generic_ntt_primes(122, n, 1, 122)
        elif name == "g85x3":
            seed = 85
            while True:
                qs = generic_ntt_primes(85, n, 3, seed)
                if (qs[0] * qs[1] * qs[2]).bit_length() == 255:
                    break
                seed += 1
        elif name[0] == "g":
            qs = generic_ntt_primes(int(name[1:]), n, 2, int(name[1:]))
        else:
            assert name[0] == "t", name
            qs = largest_ntt_primes(int(name[1:]), n, 2)
            assert all(q.bit_length() == int(name[1:]) for q in qs)
        _FULL_WIDTH_SETS[key] = qs
    return list(_FULL_WIDTH_SETS[key])


def base_conversion_case(case, n):
    """(source moduli, target moduli) of the fast base conversions that involve a full-width basis."""
    if case == "g250->g127+p60":
        return full_width_moduli("g250", n), full_width_moduli("g127", n)[:1] + ntt_primes(60, n, 1)
    if case == "g127x2->g255":
        return full_width_moduli("g127", n), full_width_moduli("g255", n)
    assert case == "p60x3->g250", case
    return ntt_primes(60, n, 3), full_width_moduli("g250", n)


def find_psi(n, q):
    """Same rule as the engine and the oracle: first x^((q-1)/2n), x = 2,3,..., of order exactly 2n."""
    e = (q - 1) // (2 * n)
    x = 2
    while True:
        c = pow(x, e, q)
        if pow(c, n, q) == q - 1:
            return c
        x += 1


def bitrev(x, bits):
    r = 0
    for _ in range(bits):
        r = (r << 1) | (x & 1); x >>= 1
    return r


# ---- direct definitions ------------------------------------------------------------------------
def negacyclic_ntt_direct(x, q, psi):
    """X[k] = sum_j x[j] psi^((2*bitrev(k)+1) j)   -- O(n^2)."""
    n = len(x); bits = n.bit_length() - 1
    out = []
    for k in range(n):
        e = 2 * bitrev(k, bits) + 1
        w = pow(psi, e, q)
        acc, p = 0, 1
        for j in range(n):
            acc = (acc + x[j] * p) % q
            p = p * w % q
        out.append(acc)
    return out


def negacyclic_mul_direct(a, b, q):
    n = len(a)
    r = [0] * n
    for i, ai in enumerate(a):
        if ai == 0:
            continue
        for j, bj in enumerate(b):
            k = i + j
            if k < n:
                r[k] = (r[k] + ai * bj) % q
            else:
                r[k - n] = (r[k - n] - ai * bj) % q
    return r


def splitmix64(seed):
    """SplitMix64 stream (the synthetic-input generator of SURVEY.md 8d)."""
    s = seed & M64
    while True:
        s = (s + 0x9E3779B97F4A7C15) & M64
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        yield z ^ (z >> 31)
