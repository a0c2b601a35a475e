"""The conventions of programmable bootstrapping (include/fhe_hip.h), pinned without a device: bootstrap_model (ms, prepare, extract)
against bgv_toy.ToyBGV at n = 16 -- prepare, six host blind-rotation steps built from ToyBGV.rgsw and O(n^2) polynomial arithmetic,
extraction, and the LWE phase of the result -- and the extraction identity for every index.  Python integers only."""
import random

import bootstrap_model as bm
import ntt_math as nm
from bgv_toy import ToyBGV

N, W, P_SPACE, Q_LWE, N_LWE = 16, 5, 4, 1 << 10, 6


def _toy(seed=3):
    return ToyBGV(N, nm.ntt_primes(20, N, 2), 1, seed=seed)


def _monomial_mul_sub(toy, poly, shift):
    """(X^shift - 1) * poly, limb-wise"""
    return [[(r - v) % q for r, v in zip(bm.rotate(poly[l], shift, q), poly[l])] for l, q in enumerate(toy.moduli)]


def _external_product(toy, d0, d1, rows0, rows1, K):
    """sum_{j,k} D_jk(d0) (*) rows0[jK + k] + D_jk(d1) (*) rows1[jK + k]: digit k of the limb-j residue, embedded in every limb."""
    o0 = [[0] * N for _ in toy.moduli]; o1 = [[0] * N for _ in toy.moduli]
    for d, (kb, ka) in ((d0, rows0), (d1, rows1)):
        for j in range(toy.L):
            for k in range(K):
                digit = toy.to_rns([(v >> (k * W)) & ((1 << W) - 1) for v in d[j]])
                o0 = toy.add(o0, toy.mul(digit, kb[j * K + k]))
                o1 = toy.add(o1, toy.mul(digit, ka[j * K + k]))
    return o0, o1


def test_ms_rounds_and_wraps():
    n = 8
    assert bm.ms(0, 1 << 32, n) == 0
    assert bm.ms((1 << 32) - 1, 1 << 32, n) == 0                  # rounds up to 2n, which wraps to 0
    assert bm.ms(1 << 27, 1 << 32, n) == 1 and bm.ms((1 << 27) - 1, 1 << 32, n) == 0      # 2^27 = q_lwe / (2 * 2n): the first boundary
    assert [bm.ms(v, 2, n) for v in (0, 1)] == [0, 8]
    assert [bm.ms(v, 7, n) for v in range(7)] == [(v * 16 + 3) // 7 % 16 for v in range(7)]
    assert bm.ms((1 << 48) - 1, 1 << 48, 1 << 15) == 0


def test_prepare_is_the_rotation_by_minus_b():
    toy = _toy()
    rng = random.Random(5)
    tv = toy.uniform()
    tv[0][0], tv[0][1] = 0, toy.moduli[0] - 1
    lwe = [[rng.randrange(Q_LWE) for _ in range(N_LWE + 1)] for _ in range(3)]
    acc0, acc1, shifts = bm.prepare(lwe, tv, toy.moduli, Q_LWE)
    for b, ct in enumerate(lwe):
        bt = bm.ms(ct[-1], Q_LWE, N)
        assert acc0[b] == [bm.rotate(tv[l], (2 * N - bt) % (2 * N), q) for l, q in enumerate(toy.moduli)]
        assert acc1[b] == [[0] * N for _ in toy.moduli]
        for i in range(N_LWE):
            assert shifts[i][b] == (2 * N - bm.ms(ct[i], Q_LWE, N)) % (2 * N)
    a0, sh = bm.prepare_np(lwe, tv, toy.moduli, Q_LWE)
    assert a0.tolist() == acc0 and sh.tolist() == shifts


def test_extraction_identity_for_every_index():
    toy = _toy(seed=7)
    c0, c1 = toy.uniform(), toy.uniform()
    c1[0][3] = 0                                                   # a zero stays zero under the negation
    s_r = toy.to_rns(toy.s)
    full = toy.add(c0, toy.mul(c1, s_r))
    for idx in range(N):
        out = bm.extract(c0, c1, toy.moduli, idx)
        for l, q in enumerate(toy.moduli):
            assert all(0 <= v < q for v in out[l])
            assert (out[l][N] + sum(a * sj for a, sj in zip(out[l][:N], toy.s))) % q == full[l][idx]
        assert bm.extract_np([c0], [c1], toy.moduli, idx)[0].tolist() == out


def test_prepare_rotate_extract_evaluates_the_test_vector():
    """Inputs m q_lwe / (2p) + q_lwe / (4p) + noise; tv[i] = Delta f(floor(i p / n)): the phase of the extracted sample is tv[phi~] or
    -tv[phi~ - n] up to noise below Q / (4p)."""
    toy = _toy(seed=11)
    rng = random.Random(13)
    p, Q = P_SPACE, toy.Q
    delta = Q // (2 * p)
    f = [3, 0, 2, 1]
    tv = toy.to_rns([delta * f[i * p // N] for i in range(N)])
    z = [rng.randrange(2) for _ in range(N_LWE)]
    rgsw = [toy.rgsw(zi, W) for zi in z]
    K = rgsw[0][2]
    batch = []
    for m in range(2 * p):                                         # the upper half of the input range lands in the negacyclic half
        a = [rng.randrange(Q_LWE) for _ in range(N_LWE)]
        phase = (m * Q_LWE // (2 * p) + Q_LWE // (4 * p) + rng.randint(-2, 2)) % Q_LWE
        batch.append(a + [(phase - sum(ai * zi for ai, zi in zip(a, z))) % Q_LWE])
    acc0, acc1, shifts = bm.prepare(batch, tv, toy.moduli, Q_LWE)
    for b, ct in enumerate(batch):
        c0, c1 = acc0[b], acc1[b]
        for i in range(N_LWE):
            d0, d1 = _monomial_mul_sub(toy, c0, shifts[i][b]), _monomial_mul_sub(toy, c1, shifts[i][b])
            e0, e1 = _external_product(toy, d0, d1, rgsw[i][0], rgsw[i][1], K)
            c0, c1 = toy.add(c0, e0), toy.add(c1, e1)
        phi = (bm.ms(ct[-1], Q_LWE, N) + sum(bm.ms(ai, Q_LWE, N) * zi for ai, zi in zip(ct[:-1], z))) % (2 * N)
        tv_int = [delta * f[i * p // N] for i in range(N)]
        want = tv_int[phi] if phi < N else -tv_int[phi - N]
        got = bm.lwe_phase(bm.extract(c0, c1, toy.moduli, 0), toy.s, toy.moduli)
        assert got == toy.phase([c0, c1])[0]
        err = (got - want + Q // 2) % Q - Q // 2
        assert abs(err) < Q // (4 * p), (b, phi, err)
