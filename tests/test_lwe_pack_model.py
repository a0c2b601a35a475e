"""The ring packing of LWE samples on plain phase polynomials with an ideal key switch (tests/lwe_pack_model.py): where the phases land,
which factor they carry, what the trace clears, the order of the elements.  Not a GPU test; the last test needs the built library only."""
import random

import pytest

import lwe_pack_model as M

N, Q = 32, 12289 * 65537          # any odd modulus does: the model never divides except by the power of two F


def _entries(count, seed):
    rng = random.Random(seed)
    return [[rng.randrange(Q) for _ in range(N)] for _ in range(count)]   # coefficient 0 is the phase, the rest is "unspecified"


@pytest.mark.parametrize("count", [1, 2, 8, 32])
@pytest.mark.parametrize("with_trace", [False, True])
@pytest.mark.parametrize("normalize", [False, True])
def test_phases_land_at_multiples_of_n_over_count(count, with_trace, normalize):
    ents = _entries(count, 1000 + count)
    out = M.pack(ents, N, Q, with_trace, normalize)
    F = 1 if normalize else (N if with_trace else count)
    step = N // count
    for i in range(count):
        assert out[i * step] == (F * ents[i][0]) % Q, (i, count)
    if with_trace:
        for x in range(N):
            if x % step:
                assert out[x] == 0, x


@pytest.mark.parametrize("count", [1, 2, 8, 32])
def test_level_order_equals_the_recursive_definition(count):
    ents = _entries(count, 7)
    for with_trace in (False, True):
        assert M.pack(ents, N, Q, with_trace, True, levels=True) == M.pack(ents, N, Q, with_trace, True, levels=False)


def test_merge_levels_cover_every_pair_once():
    for count in (2, 8, 32):
        lv = M.merge_levels(count)
        assert [l for l, *_ in lv] == list(range(1, count.bit_length()))
        assert all(half * c == count and g == c + 1 for _, half, c, g in lv)


def test_trace_elements_and_order():
    # with count = 4 the trace runs j = 3, 4, 5: each step doubles the target coefficients and clears the odd multiples of n / 2^j
    ents = _entries(4, 3)
    p = M.pack_recursive(ents, N, Q)
    for j in (3, 4, 5):
        p = M.add(p, M.automorphism(p, (1 << j) + 1, Q), Q)
        stride = N >> j
        assert all(p[x] == 0 for x in range(N) if (x // stride) % 2 == 1 and x % stride == 0)
    assert p == M.pack(ents, N, Q, True, False)


def test_galois_elements_of_the_library(pkg):
    for n in (8, 32, 2048, 1 << 16):
        got = pkg.capi.lwe_pack_galois_elements(n)
        assert got == [(1 << j) + 1 for j in range(1, n.bit_length())] == M.galois_elements(n)
    for bad in (0, 4, 24, 1 << 31):
        with pytest.raises(pkg.capi.FheError):
            pkg.capi.lwe_pack_galois_elements(bad)
