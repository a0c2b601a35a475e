"""Pure-Python model of what stands around the blind-rotation loop (test helper; contract: include/fhe_hip.h, "programmable
bootstrapping"): the switch of an LWE value to modulus 2n, the accumulator preparation and sample extraction.  Python integers only;
polynomials are [L][n] lists of residues as in bgv_toy.  Nothing here calls the library."""
import numpy as np


def ms(v, q_lwe, n):
    """floor((v 2n + floor(q_lwe / 2)) / q_lwe) mod 2n"""
    return ((int(v) * 2 * n + q_lwe // 2) // q_lwe) % (2 * n)


def rotate(poly, shift, q):
    """X^shift * poly over Z_q[x]/(x^n + 1), shift in [0, 2n), canonical (a negated 0 stays 0)."""
    n = len(poly)
    out = [0] * n
    for i, v in enumerate(poly):
        k = (i + shift) % (2 * n)
        out[k % n] = (q - int(v)) % q if k >= n else int(v)
    return out


def prepare(lwe, tv, moduli, q_lwe):
    """lwe: [batch][n_lwe + 1] values (a_0 .. a_{n_lwe-1}, b); tv: [L][n].  Returns acc0 [batch][L][n] = X^(2n - ms(b)) tv, acc1 (zeros) and
    shifts [n_lwe][batch] = (2n - ms(a_i)) mod 2n."""
    n = len(tv[0])
    n_lwe = len(lwe[0]) - 1
    acc0 = []
    for ct in lwe:
        bt = ms(ct[n_lwe], q_lwe, n)
        # coefficient x comes from index i = (x + b~) mod 2n: tv[i] if i < n, else (q - tv[i - n]) mod q
        acc0.append([[int(tv[l][i]) if (i := (x + bt) % (2 * n)) < n else (q - int(tv[l][i - n])) % q for x in range(n)]
                     for l, q in enumerate(moduli)])
    acc1 = [[[0] * n for _ in moduli] for _ in lwe]
    shifts = [[(2 * n - ms(ct[i], q_lwe, n)) % (2 * n) for ct in lwe] for i in range(n_lwe)]
    return acc0, acc1, shifts


def extract(c0, c1, moduli, idx):
    """One RLWE pair ([L][n] each) -> [L][n + 1]: out[j] = c1[idx - j] (j <= idx), (q - c1[n + idx - j]) mod q (j > idx), out[n] = c0[idx]."""
    n = len(c0[0])
    assert 0 <= idx < n
    out = []
    for l, q in enumerate(moduli):
        row = [int(c1[l][idx - j]) if j <= idx else (q - int(c1[l][n + idx - j])) % q for j in range(n)]
        out.append(row + [int(c0[l][idx])])
    return out


def lwe_phase(sample, s, moduli):
    """out[n] + sum_j out[j] s_j per limb, CRT-centred modulo Q."""
    Q = 1
    for q in moduli:
        Q *= q
    v = 0
    for l, q in enumerate(moduli):
        r = (int(sample[l][-1]) + sum(int(a) * int(sj) for a, sj in zip(sample[l][:-1], s))) % q
        Ql = Q // q
        v += r * Ql * pow(Ql, -1, q)
    v %= Q
    return v - Q if v > Q // 2 else v


# ---- numpy forms of the same definitions for the larger shapes of the GPU tests (word-sized moduli: uint64 / object arithmetic) ----
def prepare_np(lwe, tv, moduli, q_lwe):
    """lwe: uint64 [batch][n_lwe + 1]; tv: [L][n] integers.  Returns (acc0 [batch][L][n] object array, shifts uint32 [n_lwe][batch])."""
    lwe = np.asarray(lwe, dtype=object)
    tv = np.asarray(tv, dtype=object)
    L, n = tv.shape
    t = (lwe * (2 * n) + q_lwe // 2) // q_lwe % (2 * n)
    x = np.arange(n)
    acc0 = np.empty((lwe.shape[0], L, n), dtype=object)
    for b in range(lwe.shape[0]):
        i = (x + int(t[b, -1])) % (2 * n)
        for l, q in enumerate(moduli):
            acc0[b, l] = np.where(i < n, tv[l][i % n], (q - tv[l][i % n]) % q)
    shifts = ((2 * n - t[:, :-1].T) % (2 * n)).astype(np.uint32)
    return acc0, np.ascontiguousarray(shifts)


def extract_np(c0, c1, moduli, idx):
    """c0, c1: [batch][L][n] integer arrays -> uint64 [batch][L][n + 1]."""
    c0 = np.asarray(c0, dtype=object); c1 = np.asarray(c1, dtype=object)
    B, L, n = c0.shape
    j = np.arange(n)
    src = (idx - j) % n
    out = np.empty((B, L, n + 1), dtype=object)
    for l, q in enumerate(moduli):
        g = c1[:, l, :][:, src]
        out[:, l, :n] = np.where(j[None, :] <= idx, g, (q - g) % q)
        out[:, l, n] = c0[:, l, idx]
    return out.astype(np.uint64)
