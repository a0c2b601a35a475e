"""High-precision model of the CKKS encoder (test helper; test_ckks_model.py pins it and the host-side table).

With h = n/2, zeta = exp(i pi / n), omega = zeta^4 and e(k) = 3^k mod 2n, the plaintext of z in C^h is the real polynomial m of degree < n with
m(zeta^e(k)) = z_k.  Exactly one of e(k), 2n - e(k) is 4 a + 1: that a is a(k), c(k) says it was the second.  With u_j = m_j + i m_(j+h) and
w_a(k) = z_k (conjugated where c(k)):
    encode  u_j = zeta^-j (1/h) sum_a w_a omega^(-a j)          decode  w_a = sum_j (u_j zeta^j) omega^(a j)
Everything here runs on numpy.clongdouble (64-bit significand on x86) through an own radix-2 transform; `dtype=np.complex128` runs the same
formula in plain float64, which is what the tolerance of the GPU tests is measured from.  Every case is checked against the direct evaluation
m(zeta^e(k)) at 8 random slots (spot_check)."""
import os
import random

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CKKS_SYMBOLS = ("fhe_ckks_encoder_create", "fhe_ckks_encoder_destroy", "fhe_ckks_slot_table", "fhe_ckks_encode", "fhe_ckks_decode", "fhe_ckks_decode_poly")
CKKS_NAMES = CKKS_SYMBOLS + ("fhe_ckks_encoder_t",)              # the seven names of the header block


def exponents(n):
    return [pow(3, k, 2 * n) for k in range(n // 2)]


def slot_table(n):
    """(a(k), c(k)) for k < n/2."""
    a, c = [], []
    for e in exponents(n):
        if e % 4 == 1:
            a.append((e - 1) // 4); c.append(0)
        else:
            a.append((2 * n - e - 1) // 4); c.append(1)
    return np.array(a, dtype=np.int64), np.array(c, dtype=np.uint8)


def _pi(real):
    return real(np.pi) if real is np.float64 else LD("3.14159265358979323846264338327950288")   # (parsed by strtold: full precision)


def _roots(count, den, sign, cdtype):
    """exp(sign i pi j / den), j < count."""
    real = np.float64 if cdtype == np.complex128 else LD
    ang = _pi(real) * np.arange(count, dtype=real) / real(den)
    out = np.empty(count, dtype=cdtype)
    out.real = np.cos(ang); out.imag = sign * np.sin(ang)
    return out


def cyclic(x, sign, cdtype=CLD):
    """out[k] = sum_j x[j] exp(sign 2 pi i j k / len): iterative radix-2, decimation in time."""
    h = len(x)
    bits = h.bit_length() - 1
    rev = np.zeros(h, dtype=np.int64)
    for i in range(bits):
        rev |= ((np.arange(h) >> i) & 1) << (bits - 1 - i)
    a = np.array(x, dtype=cdtype)[rev]
    ln = 2
    while ln <= h:
        half = ln // 2
        w = _roots(half, half, sign, cdtype)                          # exp(sign 2 pi i j / ln)
        a = a.reshape(h // ln, ln)
        u, v = a[:, :half].copy(), a[:, half:] * w
        a[:, :half] = u + v; a[:, half:] = u - v
        a = a.reshape(h)
        ln *= 2
    return a


def encode(z, n, cdtype=CLD):
    """The real polynomial m (length n, the real type of cdtype) of the slots z (length n/2)."""
    h = n // 2
    a, c = slot_table(n)
    z = np.asarray(z, dtype=cdtype)
    w = np.zeros(h, dtype=cdtype)
    w[a] = np.where(c == 1, np.conj(z), z)
    u = cyclic(w, -1, cdtype) * _roots(h, n, -1, cdtype) / h
    return np.concatenate([u.real, u.imag])


def decode(m, cdtype=CLD):
    """The slots of the real polynomial m (any real sequence of length n)."""
    n = len(m)
    h = n // 2
    real = np.float64 if cdtype == np.complex128 else LD
    m = np.asarray(m, dtype=real)
    u = np.empty(h, dtype=cdtype)
    u.real = m[:h]; u.imag = m[h:]
    w = cyclic(u * _roots(h, n, 1, cdtype), 1, cdtype)
    a, c = slot_table(n)
    z = w[a]
    return np.where(c == 1, np.conj(z), z)


def evaluate_at(m, k):
    """m(zeta^e(k)) by direct summation in long double; the angle index is reduced mod 2n exactly first."""
    n = len(m)
    e = pow(3, k, 2 * n)
    idx = (e * np.arange(n, dtype=np.int64)) % (2 * n)
    ang = _pi(LD) * idx.astype(LD) / LD(n)
    m = np.asarray(m, dtype=LD)
    return complex(np.sum(m * np.cos(ang))), complex(np.sum(m * np.sin(ang)))


def family_slots(n, x, y):
    """The exact family: z_k = x + i y where c(k) = 0 and x - i y where c(k) = 1, as complex128.  Its plaintext is m = x + y X^(n/2): every
    w_a is x + i y, so each butterfly of the encode transform adds two equal values or multiplies a zero, and the only twiddles that meet a
    non-zero value are omega^0 = 1 and zeta^0 = 1.  Nothing is rounded in either direction, in any precision."""
    c = slot_table(n)[1]
    z = np.empty(n // 2, dtype=np.complex128)
    z.real = x
    z.imag = np.where(c == 1, -np.float64(y), np.float64(y))
    return z


def impulse_plaintext(n, k, zk):
    """m of the slots z = zk delta_k in closed form: m_j = (2/n) Re(zk zeta^(-j e(k))) (n roots zeta^(+-e(k')), m real), in long double with the
    angle index reduced mod 2n first, as evaluate_at does."""
    e = pow(3, k, 2 * n)
    idx = (e * np.arange(n, dtype=np.int64)) % (2 * n)
    ang = _pi(LD) * idx.astype(LD) / LD(n)
    return (LD(np.real(zk)) * np.cos(ang) + LD(np.imag(zk)) * np.sin(ang)) * LD(2) / LD(n)


def impulse_slots(n, j, v):
    """The slots of m = v X^j in closed form: z_k = v zeta^(j e(k)), in long double, the angle index reduced mod 2n first."""
    idx = np.array([(j * e) % (2 * n) for e in exponents(n)], dtype=np.int64)
    ang = _pi(LD) * idx.astype(LD) / LD(n)
    out = np.empty(n // 2, dtype=CLD)
    out.real = LD(v) * np.cos(ang); out.imag = LD(v) * np.sin(ang)
    return out


def spot_check(m, z, seed, tol):
    """The fast transform against direct evaluation at 8 random slots: |m(zeta^e(k)) - z_k| <= tol."""
    n = len(m)
    for k in random.Random(seed).sample(range(n // 2), 8):
        re, im = evaluate_at(m, k)
        assert abs(re.real - float(np.real(z[k]))) <= tol and abs(im.real - float(np.imag(z[k]))) <= tol, (n, k, re, im, z[k])


def float64_error(z, n, m_model):
    """E of the issue: the largest |m_j| error of the plain float64 implementation of the same formula against the long-double model."""
    m64 = encode(np.asarray(z, dtype=np.complex128), n, np.complex128)
    return float(np.max(np.abs(m64.astype(LD) - m_model)))


def float64_decode_error(m, z_model):
    z64 = decode(np.asarray(m, dtype=np.float64), np.complex128)
    d = z64.astype(CLD) - z_model
    return float(max(np.max(np.abs(d.real)), np.max(np.abs(d.imag))))


def bit_length(v):
    return int(v).bit_length()
