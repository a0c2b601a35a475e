"""Plain-integer model of the LWE -> RLWE ring packing (include/fhe_hip.h, "pack LWE samples into one RLWE ciphertext"), on PHASE
polynomials: a ciphertext is represented by c0 + c1 s modulo q, and a key switch is ideal (it keeps the phase).  Two forms of the same
algorithm: the recursive definition, and the level order the engine runs (all pairs of a level in one step), which the GPU tests also use
to write the composition out through capi.  No device needed."""


def monomial_mul(p, m, q):
    """X^m p in Z_q[X]/(X^n + 1), 0 <= m < n."""
    n = len(p)
    out = [0] * n
    for x in range(n):
        y = x - m
        out[x] = p[y] if y >= 0 else (q - p[y + n]) % q
    return out


def automorphism(p, g, q):
    """p(X^g) in Z_q[X]/(X^n + 1), g odd."""
    n = len(p)
    out = [0] * n
    for i, v in enumerate(p):
        e = (i * g) % (2 * n)
        if e < n:
            out[e] = (out[e] + v) % q
        else:
            out[e - n] = (out[e - n] - v) % q
    return out


def add(a, b, q):
    return [(x + y) % q for x, y in zip(a, b)]


def sub(a, b, q):
    return [(x - y) % q for x, y in zip(a, b)]


def galois_elements(n):
    return [(1 << j) + 1 for j in range(1, n.bit_length())]


def pack_recursive(entries, n, q):
    """The definition: Pack of c = 2^l polynomials, m = n / c."""
    c = len(entries)
    if c == 1:
        return list(entries[0])
    m = n // c
    E = pack_recursive(entries[0::2], n, q)
    O = monomial_mul(pack_recursive(entries[1::2], n, q), m, q)
    return add(add(E, O, q), automorphism(sub(E, O, q), c + 1, q), q)


def merge_levels(count):
    """[(l, half, m_shift_divisor c, g)]: level l pairs entry r with entry r + half, r < half = count / 2^l, among the count / 2^(l-1)
    results of the level before; the monomial is X^(n / 2^l) and the element 2^l + 1."""
    out, l = [], 1
    while (1 << l) <= count:
        out.append((l, count >> l, 1 << l, (1 << l) + 1))
        l += 1
    return out


def pack_levels(entries, n, q):
    """The same result in the engine's order: R_l[r] = merge(R_{l-1}[r], R_{l-1}[r + half])."""
    cur = [list(e) for e in entries]
    for _, half, c, g in merge_levels(len(entries)):
        m = n // c
        nxt = []
        for r in range(half):
            E, O = cur[r], monomial_mul(cur[r + half], m, q)
            nxt.append(add(add(E, O, q), automorphism(sub(E, O, q), g, q), q))
        cur = nxt
    return cur[0]


def trace(p, count, n, q):
    """ct <- ct + sigma_{2^j + 1}(ct), j = log2(count) + 1 .. log2(n), in this order."""
    k, log_n = count.bit_length() - 1, n.bit_length() - 1
    for j in range(k + 1, log_n + 1):
        p = add(p, automorphism(p, (1 << j) + 1, q), q)
    return p


def pack(entries, n, q, with_trace, normalize, levels=False):
    count = len(entries)
    F = n if with_trace else count
    if normalize:
        inv = pow(F, -1, q)
        entries = [[(v * inv) % q for v in e] for e in entries]
    p = (pack_levels if levels else pack_recursive)(entries, n, q)
    return trace(p, count, n, q) if with_trace else p
