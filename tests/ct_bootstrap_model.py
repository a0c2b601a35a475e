"""Plain-integer model of the two joints of FHEContext::bootstrap(Ciphertext&) (test helper; contract: include/fhe_hip.h,
fhe_rlwe_sample_extract_strided and fhe_rlwe_pack) and of the scaled encoding the whole call works in.  Nothing here calls the library."""
import numpy as np

import bootstrap_model as bm


def extract_strided(c0, c1, moduli, count):
    """One RLWE pair ([L][n] each) -> [count][L][n + 1], written the way the kernel works: row i is row 0 rotated by idx_i = i n / count.  The
    lane of position j0 in row 0 holds v = c1[-j0 mod n] and its negation, and stores at j = (j0 + idx_i) mod n the negated value exactly
    where j0 != 0 and j0 + idx_i < n."""
    n = len(c0[0])
    assert count >= 1 and count & (count - 1) == 0 and count <= n
    out = [[[None] * (n + 1) for _ in moduli] for _ in range(count)]
    for l, q in enumerate(moduli):
        for j0 in range(n):
            v = int(c1[l][(n - j0) % n])
            vn = (q - v) % q if j0 else v
            for i in range(count):
                j = j0 + i * (n // count)
                out[i][l][j % n] = vn if j < n else v
        for i in range(count):
            out[i][l][n] = int(c0[l][i * (n // count)])
    return out


def extract_strided_np(c0, c1, moduli, count):
    """c0, c1: [batch][L][n] integer arrays -> uint64 [batch][count][L][n + 1]: `count` calls of bootstrap_model.extract_np, scattered."""
    n = np.asarray(c0).shape[-1]
    return np.stack([bm.extract_np(c0, c1, moduli, i * (n // count)) for i in range(count)], axis=1)


def embed(sample, moduli):
    """[L][n + 1] -> (c0, c1), [L][n] each: c0 = (b, 0, .., 0), c1[0] = a_0, c1[i] = -a_{n-i} (include/fhe_hip.h, "Embedding")."""
    n = len(sample[0]) - 1
    c0 = [[int(row[n])] + [0] * (n - 1) for row in sample]
    c1 = [[int(row[0])] + [(q - int(row[n - i])) % q for i in range(1, n)] for row, q in zip(sample, moduli)]
    return c0, c1


def negacyclic_phase(c0, c1, s, q):
    """c0 + c1 s in Z_q[X] / (X^n + 1) for one limb (lists of integers)."""
    n = len(c0)
    out = [int(v) for v in c0]
    for i, a in enumerate(c1):
        if a:
            for j, sj in enumerate(s):
                if sj:
                    k = i + j
                    if k < n:
                        out[k] = (out[k] + a * sj) % q
                    else:
                        out[k - n] = (out[k - n] - a * sj) % q
    return [v % q for v in out]


def ideal_bootstrap(phases, table, Q, q0, q_lwe, n, p, offset=False):
    """The whole call on noiseless phases: phase modulo Q -> rounded division to the first prime -> modulus switch to q_lwe -> to 2n -> the entry of
    tv[j] = Delta table[floor(j p / n)] (+ Delta / 2) -> the output phase.  A rotation phi >= n reads the negated vector."""
    delta = Q // (2 * p)
    out = []
    for v in phases:
        low = ((v % Q) * q0 + Q // 2) // Q % q0
        lwe = (low * q_lwe + q0 // 2) // q0 % q_lwe
        phi = bm.ms(lwe, q_lwe, n)
        tv = lambda j: delta * table[j * p // n] + (delta // 2 if offset else 0)
        out.append(tv(phi) if phi < n else -tv(phi - n))
    return out
