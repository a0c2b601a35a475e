"""The two joints of FHEContext::bootstrap(Ciphertext&) on plain integers (tests/ct_bootstrap_model.py, tests/bootstrap_model.py,
tests/lwe_pack_model.py): strided extraction is `count` single extractions, extraction at 0 followed by the embedding keeps (c0[0], c1), so
packing from RLWE pairs is packing of their samples, and the parameters of tests/test_ct_bootstrap.py decode on noiseless phases.  No device."""
import random

import pytest

import bootstrap_model as bm
import ct_bootstrap_model as cm
import lwe_pack_model as M

MODULI = (97, 193, 257)


def _pair(n, seed):
    rng = random.Random(seed)
    c0 = [[rng.randrange(q) for _ in range(n)] for q in MODULI]
    c1 = [[rng.randrange(q) for _ in range(n)] for q in MODULI]
    for l, q in enumerate(MODULI):                       # zeros stay zeros under the negation; q - 1 becomes 1
        c1[l][0] = 0; c1[l][n - 1] = 0; c1[l][1] = q - 1; c1[l][n // 2] = 0
    return c0, c1


@pytest.mark.parametrize("n,count", [(8, 1), (8, 2), (8, 8), (32, 4), (32, 32), (64, 1)])
def test_strided_extraction_is_count_single_extractions(n, count):
    c0, c1 = _pair(n, 3 * n + count)
    got = cm.extract_strided(c0, c1, MODULI, count)
    for i in range(count):
        assert got[i] == bm.extract(c0, c1, MODULI, i * n // count), i
    assert all(0 <= v < q for rows in got for row, q in zip(rows, MODULI) for v in row)
    np_form = cm.extract_strided_np([c0], [c1], MODULI, count)
    assert np_form.shape == (1, count, len(MODULI), n + 1) and np_form[0].tolist() == got


@pytest.mark.parametrize("n", [8, 32])
def test_extraction_at_zero_then_the_embedding_keeps_c0_0_and_c1(n):
    c0, c1 = _pair(n, n)
    e0, e1 = cm.embed(bm.extract(c0, c1, MODULI, 0), MODULI)
    assert e1 == c1
    assert e0 == [[row[0]] + [0] * (n - 1) for row in c0]


@pytest.mark.parametrize("count,with_trace,normalize", [(1, True, True), (2, False, True), (4, True, False), (8, True, True)])
def test_packing_from_pairs_is_packing_of_their_samples(count, with_trace, normalize):
    """On phase polynomials, with an ideal key switch: the packer sees c0[0] + c1 s whether it is handed the sample or the pair, so both pack to
    the same polynomial, whose coefficient i n / count is F (or 1) times coefficient 0 of pair i -- whatever the rest of c0 holds."""
    n, q = 8, MODULI[2]
    rng = random.Random(count)
    s = [rng.randrange(-1, 2) for _ in range(n)]
    pairs = [([rng.randrange(q) for _ in range(n)], [rng.randrange(q) for _ in range(n)]) for _ in range(count)]
    from_samples, from_pairs, want = [], [], []
    for c0, c1 in pairs:
        sample = bm.extract([c0], [c1], [q], 0)
        e0, e1 = cm.embed(sample, [q])
        from_samples.append(cm.negacyclic_phase(e0[0], e1[0], s, q))
        from_pairs.append(cm.negacyclic_phase([c0[0]] + [0] * (n - 1), c1, s, q))
        want.append(cm.negacyclic_phase(c0, c1, s, q)[0])
        assert from_samples[-1][0] == want[-1] == bm.lwe_phase(sample, s, [q]) % q
    assert from_samples == from_pairs
    a = M.pack(from_samples, n, q, with_trace, normalize, levels=True)
    assert a == M.pack(from_pairs, n, q, with_trace, normalize)
    F = 1 if normalize else (n if with_trace else count)
    for i in range(count):
        assert a[i * n // count] == (F * want[i]) % q
    if with_trace:
        assert all(v == 0 for x, v in enumerate(a) if x % (n // count))


def test_the_parameters_of_the_gpu_test_decode_without_noise():
    """N = 2048, two 30-bit primes, p = 8, q_lwe = 2^32: every message in the scaled encoding, Delta m + Delta / 2 with an error of up to a
    quarter slot either way, comes out as Delta f(m), and with the half-slot offset in the table the output is the input of a second call."""
    import ntt_math as nm
    n, p, q_lwe = 2048, 8, 1 << 32
    moduli = nm.ntt_primes(30, n, 2)
    Q, q0 = moduli[0] * moduli[1], moduli[0]
    delta = Q // (2 * p)
    f, g = [5, 1, 7, 0, 3, 3, 6, 2], [2, 7, 1, 1, 6, 0, 4, 3]
    for e in (-(delta // 4), 0, delta // 4):
        phases = [delta * m + delta // 2 + e for m in range(p)]
        assert cm.ideal_bootstrap(phases, f, Q, q0, q_lwe, n, p) == [delta * f[m] for m in range(p)]
        mid = cm.ideal_bootstrap(phases, f, Q, q0, q_lwe, n, p, offset=True)
        assert cm.ideal_bootstrap(mid, g, Q, q0, q_lwe, n, p) == [delta * g[f[m]] for m in range(p)]
    # a phase of 0, what every other coefficient carries, would read the table at its edge: those coefficients are not bootstrapped at all
    assert cm.ideal_bootstrap([0], f, Q, q0, q_lwe, n, p) == [delta * f[0]]
