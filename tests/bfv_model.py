"""Python big-integer model of the two RNS steps of a BFV multiplication (include/fhe_hip.h, BFV section), the exact values they
approximate, and the fixed-seed inputs the CPU and GPU tests share.

Polynomial data is [batch][limbs][n] numpy object arrays of Python integers (residues) or [batch][n] (integers); `containers` /
`from_containers` convert to and from the library's [..][4] uint64 layout."""
import numpy as np

import ntt_math as nm

M64 = (1 << 64) - 1


def prod(xs):
    out = 1
    for x in xs:
        out *= int(x)
    return out


def containers(v):
    out = np.zeros(v.shape + (4,), np.uint64)
    for k in range(4):
        out[..., k] = ((v >> (64 * k)) & M64).astype(np.uint64)
    return np.ascontiguousarray(out)


def from_containers(a):
    return sum(a[..., k].astype(object) << (64 * k) for k in range(4))


# ------------------------------------------------------------------------------------------------ the definitions
def lift_tables(B, C):
    Bp = prod(B)
    return {"minv": [pow(Bp // b, -1, b) for b in B], "r": [(1 << 128) // b for b in B],
            "mat": [[(Bp // b) % c for c in C] for b in B], "bmod": [Bp % c for c in C]}


def lift(X, B, C):
    """Centred lift of X ([batch][k][n] residues modulo the primes B) to the primes C: [batch][len(C)][n]."""
    T = lift_tables(B, C)
    y = [(X[:, i, :] * T["minv"][i]) % b for i, b in enumerate(B)]
    V = sum(y[i] * T["r"][i] for i in range(len(B)))
    alpha = (V + (1 << 127)) >> 128
    out = np.empty((X.shape[0], len(C), X.shape[2]), object)
    for j, c in enumerate(C):
        out[:, j, :] = (sum(y[i] * T["mat"][i][j] for i in range(len(B))) - alpha * T["bmod"][j]) % c
    return out


def scale_tables(Q, P, t):
    Qp, Pp = prod(Q), prod(P)
    theta = [t * Pp % q for q in Q]
    return {"yinv": [pow(Qp * Pp // m, -1, m) for m in list(Q) + list(P)], "theta": theta,
            "rho": [((1 << 128) * th) // q for th, q in zip(theta, Q)],
            "omega": [[(-th * pow(q, -1, p)) % p for p in P] for th, q in zip(theta, Q)]}


def scale_round_p(X, Q, P, t):
    """s_j of the definition: X is [batch][L + L'][n] residues modulo Q u P, the result [batch][L'][n] modulo P."""
    T = scale_tables(Q, P, t)
    L, Pp = len(Q), prod(P)
    y = [(X[:, k, :] * T["yinv"][k]) % m for k, m in enumerate(list(Q) + list(P))]
    W = sum(y[i] * T["rho"][i] for i in range(L))
    R = (W + (1 << 127)) >> 128
    out = np.empty((X.shape[0], len(P), X.shape[2]), object)
    for j, p in enumerate(P):
        out[:, j, :] = (R + sum(y[i] * T["omega"][i][j] for i in range(L)) + y[L + j] * t * (Pp // p)) % p
    return out


def scale_round(X, Q, P, t):
    """fhe_bfv_scale_round: s, then its centred lift from base P to base Q: [batch][L][n]."""
    return lift(scale_round_p(X, Q, P, t), P, Q)


# ------------------------------------------------------------------------------------------------ exact values
def crt(X, B):
    """[batch][k][n] residues -> [batch][n] integers in [0, prod B)"""
    Bp = prod(B)
    return sum(X[:, i, :] * ((Bp // b) * pow(Bp // b, -1, b)) for i, b in enumerate(B)) % Bp


def centre(v, B):
    """the representative in (-B/2, B/2] of the integers v modulo the odd B"""
    return np.where((v > (B - 1) // 2).astype(bool), v - B, v)


def residues(v, C):
    """[batch][n] integers -> [batch][len(C)][n] residues"""
    out = np.empty((v.shape[0], len(C), v.shape[1]), object)
    for j, c in enumerate(C):
        out[:, j, :] = v % c
    return out


def exact_lift(X, B, C):
    return residues(centre(crt(X, B), prod(B)), C)


def exact_round(v, Q, t):
    """round(t v / Q) for integers v; Q odd, so no fractional part is 1/2"""
    return (2 * t * v + Q) // (2 * Q)


def negacyclic(a, b):
    """Product of two integer polynomials (lists of Python integers, any sign) modulo x^n + 1, by Kronecker substitution."""
    n = len(a)
    bound = n * max(1, max(abs(int(x)) for x in a)) * max(1, max(abs(int(x)) for x in b))
    w = (bound.bit_length() + 2 + 7) // 8                       # bytes per slot: |c_i| < 2^(8 w - 1)

    def pack(x):
        pos = int.from_bytes(b"".join(max(int(v), 0).to_bytes(w, "little") for v in x), "little")
        neg = int.from_bytes(b"".join(max(-int(v), 0).to_bytes(w, "little") for v in x), "little")
        return pos - neg
    half = 1 << (8 * w - 1)
    off = int.from_bytes((half.to_bytes(w, "little")) * (2 * n), "little")
    raw = (pack(a) * pack(b) + off).to_bytes(2 * n * w + 1, "little")
    c = [int.from_bytes(raw[i * w:(i + 1) * w], "little") - half for i in range(2 * n)]
    return [c[i] - c[i + n] for i in range(n)]


def exact_bfv_product(a0, a1, b0, b1, Q, t):
    """(c0, c1, c2) = round(t / Q (a (x) b)) mod Q for [batch][n] CENTRED integer polynomials: [batch][L][n] residues each."""
    Qp = prod(Q)
    outs = [np.empty(a0.shape, object) for _ in range(3)]
    for b in range(a0.shape[0]):
        t0 = negacyclic(a0[b], b0[b])
        x, y = negacyclic(a0[b], b1[b]), negacyclic(a1[b], b0[b])
        t1 = [u + v for u, v in zip(x, y)]
        t2 = negacyclic(a1[b], b1[b])
        for o, tt in zip(outs, (t0, t1, t2)):
            o[b, :] = [exact_round(v, Qp, t) for v in tt]
    return [residues(o, Q) for o in outs]


# ------------------------------------------------------------------------------------------------ shared fixed-seed inputs
# The word-sized classes at n = 2048 and the prime sizes at the bottom and the top of each one's range.  fhe_bfv_multiplier_create asks for
# P > 32 t n Q, so the shapes with ONE more auxiliary prime than ciphertext primes, (1, 2) and (2, 3), need that prime above 32 t n: 2^17 at
# t = 2, which is what those shapes use (2^32 at t = 65537: out of reach of every prime below 2^33).  The bottom of the 4-byte class is
# therefore 19-bit primes (>= 2^18), the smallest size the bound admits at all; (3, 5) has two primes to spare and uses t = 65537.
N = 2048
CLASSES = {"F32-bottom": (1, 19), "F32-top": (1, 30), "F52-bottom": (3, 31), "F52-top": (3, 43), "F64-bottom": (2, 44), "F64-top": (2, 62),
           "F64X-bottom": (5, 63), "F64X-top": (5, 64)}
SHAPES = [(1, 2, 2), (2, 3, 2), (3, 5, 65537)]               # (L, L', t)
T_PLAIN = 65537
_BASES, _RANDOM = {}, {}


def bases(cls, L, Lp):
    """(Q, P) of a class row: the L + L' largest primes below 2^bits for a "top" row, the smallest from 2^(bits - 1) on for a "bottom" row"""
    key = (cls, L, Lp)
    if key not in _BASES:
        bits = CLASSES[cls][1]
        ps = nm.largest_ntt_primes(bits, N, L + Lp) if cls.endswith("top") else nm.ntt_primes(bits, N, L + Lp)
        _BASES[key] = (ps[:L], ps[L:])
    return _BASES[key]


def cap_bases(cls):
    """L = L' = 16, the cap of both kernels' register arrays: P > 32 t n Q with as many auxiliary primes as ciphertext primes needs SMALLER
    ciphertext primes, so Q is 16 primes from the lower part of the class (22-bit for the 4-byte class, 44-bit for the 8-byte integer class)
    and P the 16 largest of the class."""
    key = (cls, 16, 16)
    if key not in _BASES:
        lo, hi = {"F32": (22, 30), "F64": (44, 62)}[cls]
        _BASES[key] = (nm.ntt_primes(lo, N, 16), nm.largest_ntt_primes(hi, N, 16))
    return _BASES[key]


def bound_holds(Q, P, t, n):
    return prod(P) > 32 * t * n * prod(Q)


def random_residues(seed, moduli, batch, n=N):
    key = (seed, tuple(moduli), batch, n)
    if key not in _RANDOM:
        rng = np.random.default_rng(seed)
        out = np.empty((batch, len(moduli), n), object)
        for l, q in enumerate(moduli):
            words = rng.integers(0, 1 << 63, size=(batch, n, 2), dtype=np.uint64).astype(object)
            out[:, l, :] = (words[..., 0] + (words[..., 1] << 63)) % q
        _RANDOM[key] = out
    return _RANDOM[key]


def lift_inputs(seed, Q, batch, n=N):
    """Random residues with the edge family planted at x = 0 .. 4 of every batch element: the values 0, 1, Q - 1, (Q - 1) / 2, (Q + 1) / 2."""
    X = random_residues(seed, Q, batch, n).copy()
    Qp = prod(Q)
    for x, v in enumerate([0, 1, Qp - 1, (Qp - 1) // 2, (Qp + 1) // 2]):
        for l, q in enumerate(Q):
            X[:, l, x] = v % q
    return X


def scale_inputs(seed, Q, P, t, batch, n=N):
    """Random residues modulo Q u P with planted values at x = 0 .. : 0, 1, QP - 1, (QP -+ 1) / 2 and the neighbours of +-Q / 2t (where t x / Q
    passes 1/2) and of +-3Q / 2t."""
    M = list(Q) + list(P)
    X = random_residues(seed, M, batch, n).copy()
    Qp, QP = prod(Q), prod(M)
    vals = [0, 1, QP - 1, (QP - 1) // 2, (QP + 1) // 2]
    for k in (1, 3):
        c = k * Qp // (2 * t)
        vals += [c - 1, c, c + 1, c + 2, -(c - 1), -c, -(c + 1), -(c + 2)]
    for x, v in enumerate(vals):
        for l, m in enumerate(M):
            X[:, l, x] = v % m
    return X


def ciphertext_sized(seed, Q, batch, n=N):
    """Four dense random polynomials modulo Q (a0, a1, b0, b1) as [batch][L][n] residues"""
    return [random_residues(seed + i, Q, batch, n) for i in range(4)]
