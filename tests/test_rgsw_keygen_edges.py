"""RGSW key generation (fhe_rgsw_keys_generate, fhe_relin_keys_export) on every instance of ntt_rgsw_keygen_kernel beyond the centre of its
ranges, and on every route around the kernel.

tests/test_rgsw_keygen.py runs bottom-of-class moduli (one pair of largest 64-bit primes), L = 3 at N = 2^11 only and L = 1 above, K <= 4, the
39-entry table (sigma = 86 once, composed), noise_scale = 65537, at most three messages and a uniformly random s; the composed path at n = 2048
and 1024.  What is added here, test by test (every case is one entry of CASES below; the path it must take stands beside it and is pinned by
test_every_case_takes_the_path_it_was_written_for):

  instances     all sixteen (field, N) with SPAN moduli (top, top, bottom of the class's top bit: the FP64 field at 43 bits, the lazy field at
                62), L = 3, K = 2, mu = 1, -2^15 and 2^15 together; s: limb 0 random, limb 1 all q - 1, limb 2 zero:
                test_every_fused_instance_with_three_limbs_span_moduli_three_messages
  L and K       L = 1 and L = 5 with K = 3 on all four classes: test_one_and_five_limbs_three_digits
  gadget        2^(k w) >= q_j (a top prime beside 12289, a 31-bit and a 41-bit one: from_u64 of the factor reduces) and k w = 63, with
                mu = -3 and 2^15 (|mu| above 12289: from_u64 of the message reduces too): test_gadget_factors_and_messages
  moduli        the 14- and 16-bit pair, w = 4, mu = 1 and -1: test_smallest_moduli
  tables        1, 8, 64, 1024 entries on all four classes: test_table_lengths; 1025 entries (composed): test_a_table_one_entry_too_long
  noise_scale   1, q_0 (vanishes in limb 0), q_0 + 1, 2^64 - 59 on the span bases of all four classes: test_noise_scales
  messages      40 messages cycling through 0, 1, -1, 2^15, -2^15 at L = K = 1: 80 sets, the stream offsets Pn N and the table lookup
                sets[Pn / LK] at high Pn, against the oracle's rows: test_forty_messages
  paths         composed by the switch, ONE child process for every n = 2048 instance, limb and gadget case, equal to the oracle's rows and to
                the fused bits: test_the_composed_path_gives_the_same_bits_on_every_edge_case; composed by itself at N = 2^15 (4-byte: packed
                afterwards; 8-byte: containers) and N = 2^16, each with mu = 0 (rgsw_target_kernel negates or doubles an accumulator of 0) and a
                negative mu: test_sizes_that_take_the_composed_path; unpacked sets on a word-sized class with their packed neighbour, mu = 0 and
                -1: test_unpacked_key_sets_on_a_word_sized_class
  consumer      fhe_blind_rotate_step with the generated handles at N = 2^12 .. 2^14 on a 4-byte and an 8-byte field and on the FP64 field at
                N = 4096, against the oracle's step on the oracle's rows: test_blind_rotation_step_at_the_larger_sizes

Every expected row comes from the CPU oracle (_expected of test_rgsw_keygen.py) and Python integers, once per module; every comparison is
np.array_equal on whole arrays through fhe_relin_keys_export into poisoned outputs.

Not tested: the fallback of the uniform draw after 64 rejections (about 2^-64 per draw; no real stream reaches it), the kernels' assembly, and
hipGraph capture of the call (it allocates)."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

import ntt_math as nm
from test_encrypt_edges import SIGMA_LEN, SMALLEST, T_BIG, _span
from test_keygen import _export
from test_keygen_edges import FUSED, COMPOSED, GADGET, MAX_TABLE, N0, UNPACKED, W2, W3, _class, _digits, _fused, _kw, _packed, _scale, _secret, _top1
from test_rgsw_keygen import SEEDS, SIGMA, T, _expected, _exports, _generate
from test_top_of_range import BITS, WIDTH
from workload import rns_poly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 15                                          # the largest |mu| the call admits

# n, moduli, decomp_bits, messages, secret ('random': rns_poly(90); 'edges': limb 0 random, limb 1 all q - 1, every further limb zero -- _secret of
# test_keygen_edges.py), noise_scale, sigma
Case = collections.namedtuple("Case", "n moduli w mus s noise_scale sigma")


def _mk(n, moduli, w, mus, s="random", noise_scale=T, sigma=SIGMA):
    return Case(n, tuple(moduli), w, tuple(mus), s, noise_scale, sigma)


# Every GPU case of this file: id -> (Case, the path the documented rule must give for it).
CASES = {}
INSTANCE_IDS = [(bits, log_n) for bits in BITS for log_n in (11, 12, 13, 14)]
for bits, log_n in INSTANCE_IDS:
    CASES["instance", bits, log_n] = (_mk(1 << log_n, _span(bits, 1 << log_n, 3), W2[bits], (1, -BIG, BIG), "edges"), FUSED)
LIMB_IDS = [(bits, L) for bits in BITS for L in (1, 5)]
for bits, L in LIMB_IDS:
    CASES["limbs", bits, L] = (_mk(N0, _top1(bits, N0) if L == 1 else _span(bits, N0, L), W3[bits], (-1, 3)), FUSED)
for name, (moduli, w) in GADGET.items():
    CASES["gadget", name] = (_mk(N0, moduli, w, (-3, BIG)), FUSED)
CASES["smallest",] = (_mk(N0, SMALLEST, 4, (1, -1)), FUSED)
TABLE_IDS = [(bits, sigma) for bits in BITS for sigma in (0.08, 0.66, 5.3, 85.3)]
for bits, sigma in TABLE_IDS:
    CASES["table", bits, sigma] = (_mk(N0, _span(bits, N0, 2), W2[bits], (1, -1), sigma=sigma), FUSED)
for bits in (30, 64):
    CASES["long-table", bits] = (_mk(N0, _span(bits, N0, 2), W2[bits], (1, -1), sigma=85.4), COMPOSED)
SCALE_IDS = [(bits, name) for bits in BITS for name in ("1", "q0", "q0+1", "2^64-59")]
for bits, name in SCALE_IDS:
    CASES["scale", bits, name] = (_mk(N0, _span(bits, N0, 2), W2[bits], (1, -1), noise_scale=_scale(name, _span(bits, N0, 2))), FUSED)
MANY = 40
for bits in (30, 64):                                  # L = 1, K = 1: one row per set, 80 sets
    CASES["many", bits] = (_mk(N0, _top1(bits, N0), bits, [(0, 1, -1, BIG, -BIG)[i % 5] for i in range(MANY)]), FUSED)
BY_ITSELF = {"4-byte-2^15": _mk(1 << 15, _span(30, 1 << 15, 3), W2[30], (0, -3), "edges"),
             "lazy-64-bit-2^15": _mk(1 << 15, _span(62, 1 << 15, 3), W2[62], (0, -3), "edges"),
             "4-byte-2^16": _mk(1 << 16, _span(30, 1 << 16, 2), W2[30], (0, -BIG), "edges")}    # L = 2 for the oracle's time; two messages
for name, c in BY_ITSELF.items():
    CASES["by-itself", name] = (c, COMPOSED)
for name, (c, _, fused) in UNPACKED.items():           # the bases of test_keygen_edges.py: (Case, packed, fused)
    CASES["unpacked", name] = (_mk(c.n, c.moduli, c.w, (0, -1)), fused)
AGAIN = [k for k in CASES if k[0] in ("instance", "limbs", "gadget") and CASES[k][0].n == N0]      # under the switch, in one child process
CONSUMER_IDS = [(bits, log_n) for bits in (30, 64) for log_n in (12, 13, 14)] + [(43, 12)]


# ------------------------------------------------------------------------------------------------ expectations and runs, once per module
_cache, _got = {}, {}


def _want(oracle, c):
    """(s, b, a) of a case: [2 num][L K][L][n][4] each, half 2 i + c the component c of message i"""
    if c not in _cache:
        s = _secret(oracle, c)
        _cache[c] = (s,) + _expected(oracle, c.n, list(c.moduli), c.w, list(c.mus), s, **_kw(c))
    return _cache[c]


def _run(pkg, c, s):
    return _exports(pkg, c.n, list(c.moduli), c.w, list(c.mus), s, **_kw(c))


def _check(pkg, oracle, key):
    c = CASES[key][0]
    s, wb, wa = _want(oracle, c)
    if key not in _got:
        _got[key] = _run(pkg, c, s)
    gb, ga = _got[key]
    assert gb.shape == wb.shape == (2 * len(c.mus), len(c.moduli) * _digits(c), len(c.moduli), c.n, 4)
    assert np.array_equal(ga, wa), key
    assert np.array_equal(gb, wb), key
    return gb, ga


# ------------------------------------------------------------------------------------------------ CPU
def test_every_case_takes_the_path_it_was_written_for(oracle):
    """fhe_rgsw_keys_generate is fused exactly where fhe_keyswitch_keys_generate is (include/fhe_hip.h): packed sets (_packed: keys_get_packed in
    Python), 11 <= log2 n <= 14, a table of at most 1024 entries, a word-sized class -- _fused of test_keygen_edges.py, not restated here."""
    for key, (c, fused) in CASES.items():
        assert _fused(oracle, c) == fused, key
        if fused:
            assert _packed(c) and 11 <= c.n.bit_length() - 1 <= 14 and len(oracle.gaussian_cdt(c.sigma)) <= MAX_TABLE and _class(c) in BITS, key
    assert sum(fused for _, fused in CASES.values()) == 16 + 8 + 6 + 1 + 16 + 16 + 2 + 1 and len(CASES) == 66 + 2 + 3 + 2
    assert len(AGAIN) == 4 + 8 + 6 and all(CASES[key][1] == FUSED for key in AGAIN)
    assert {_class(CASES["instance", bits, log_n][0]) for bits, log_n in INSTANCE_IDS} == set(BITS)
    for name, (_, packed, fused) in UNPACKED.items():                                          # word-sized classes, and why they are not packed
        c = CASES["unpacked", name][0]
        assert _class(c) == (30 if name == "digits-do-not-fit" else 43) and _packed(c) == packed, name
    assert [len(CASES["unpacked", k][0].moduli) * _digits(CASES["unpacked", k][0]) for k in ("86-products-fp64", "80-products-fp64")] == [86, 80]
    # composed by themselves: packed afterwards on the 4-byte class at N = 2^15, containers elsewhere
    assert [_packed(c) for c in BY_ITSELF.values()] == [True, False, False]
    assert [_class(c) for c in BY_ITSELF.values()] == [30, 62, 30]
    assert all(_packed(CASES["long-table", bits][0]) for bits in (30, 64))
    for bits, log_n in CONSUMER_IDS:
        assert CASES["instance", bits, log_n][1] == FUSED


def test_the_inputs_sit_on_the_edges_they_are_meant_to_hit(oracle):
    for sigma, length in ((0.08, 1), (0.66, 8), (5.3, 64), (85.3, 1024), (85.4, 1025)):
        assert len(oracle.gaussian_cdt(sigma)) == length == SIGMA_LEN[sigma], sigma
    assert {c.sigma for k, (c, _) in CASES.items() if k[0] == "table"} == {0.08, 0.66, 5.3, 85.3} and MAX_TABLE == 1024
    for name in GADGET:                                                                        # some 2^(k w) >= q_j: from_u64 of the factor reduces
        c = CASES["gadget", name][0]
        assert any(1 << (k * c.w) >= q for q in c.moduli for k in range(_digits(c))), name
        assert (_digits(c) - 1) * c.w < 64 and c.mus == (-3, BIG), name
    for name in ("64-span-shift-63", "64-with-41-bit-shift-63"):
        c = CASES["gadget", name][0]
        assert (_digits(c) - 1) * c.w == 63 and _packed(c), name
    assert BIG > 12289 in CASES["gadget", "30-with-12289"][0].moduli                           # |mu| above a modulus
    for bits, log_n in INSTANCE_IDS:                                                           # top, top, bottom of the class's top bit
        c = CASES["instance", bits, log_n][0]
        assert [q.bit_length() for q in c.moduli] == [bits, bits, 63 if bits == 64 else bits] and _digits(c) == 2
        assert (1 << bits) - c.moduli[0] < 1 << 24 and c.mus == (1, -BIG, BIG)
    c = CASES["instance", 43, 11][0]
    s = np.stack([x[:, 0] for x in _secret(oracle, c)]).astype(object)
    assert set(s[1].tolist()) == {c.moduli[1] - 1} and set(s[2].tolist()) == {0} and len(set(s[0].tolist())) > 2000
    for bits in BITS:
        q = _span(bits, N0, 2)
        assert [CASES["scale", bits, name][0].noise_scale for name in ("1", "q0", "q0+1", "2^64-59")] == [1, q[0], q[0] + 1, T_BIG]
        assert [len(CASES["limbs", bits, L][0].moduli) for L in (1, 5)] == [1, 5] and _digits(CASES["limbs", bits, 5][0]) == 3
    assert CASES["smallest",][0].moduli == (12289, 40961) == tuple(nm.ntt_primes(14, N0, 2))
    for bits in (30, 64):
        c = CASES["many", bits][0]
        assert len(c.moduli) * _digits(c) == 1 and len(c.mus) == 40 and set(c.mus) == {0, 1, -1, BIG, -BIG}
    for c in BY_ITSELF.values():
        assert 0 in c.mus and min(c.mus) < 0


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("bits,log_n", INSTANCE_IDS)
def test_every_fused_instance_with_three_limbs_span_moduli_three_messages(pkg, oracle, bits, log_n):
    """L = 3, K = 2 at every size: the block index splits by 3, 6 and 2; gm = [mu 2^(k w)] on top-of-class moduli for mu = 1, -2^15 and 2^15, and
    its product with s^ = q - 1 and s^ = 0 in component 1."""
    c = CASES["instance", bits, log_n][0]
    assert pkg.RnsNttEngine(c.n, list(c.moduli)).width_class == WIDTH[bits]
    gb, _ = _check(pkg, oracle, ("instance", bits, log_n))
    assert not np.array_equal(gb[2], gb[4])                        # -2^15 and 2^15 are different keys


@pytest.mark.gpu
@pytest.mark.parametrize("bits,L", LIMB_IDS)
def test_one_and_five_limbs_three_digits(pkg, oracle, bits, L):
    """L = 1: j = 0 always, every workgroup adds a gadget term.  L = 5, K = 3: fifteen rows of five limbs per half.  mu = -1 and 3."""
    _check(pkg, oracle, ("limbs", bits, L))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GADGET))
def test_gadget_factors_and_messages(pkg, oracle, name):
    """2^(k w) at or above the narrow modulus of the base, k w = 63, |mu| = 2^15 above the modulus 12289: both reductions of from_u64 act."""
    _check(pkg, oracle, ("gadget", name))


@pytest.mark.gpu
def test_smallest_moduli(pkg, oracle):
    """q = 12289 and 40961, w = 4: rejection masks of 14 and 16 bits, noise_scale = 65537 above both moduli."""
    _check(pkg, oracle, ("smallest",))


@pytest.mark.gpu
@pytest.mark.parametrize("bits,sigma", TABLE_IDS)
def test_table_lengths(pkg, oracle, bits, sigma):
    """top = 1, 8, 64 and 1024 in the kernel's table search"""
    _check(pkg, oracle, ("table", bits, sigma))


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [30, 64])
def test_a_table_one_entry_too_long(pkg, oracle, bits):
    _check(pkg, oracle, ("long-table", bits))


@pytest.mark.gpu
@pytest.mark.parametrize("bits,name", SCALE_IDS)
def test_noise_scales(pkg, oracle, bits, name):
    gb, _ = _check(pkg, oracle, ("scale", bits, name))
    if name == "q0":                                   # no noise in limb 0: the row without it, from the oracle
        c = CASES["scale", bits, name][0]
        s, wb, wa = _want(oracle, c)
        clean = _expected(oracle, c.n, list(c.moduli), c.w, list(c.mus), s, noise_scale=c.noise_scale, sigma=0.08)[0]
        assert np.array_equal(gb[:, :, 0], clean[:, :, 0]) and not np.array_equal(gb[:, :, 1], clean[:, :, 1])


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [30, 64])
def test_forty_messages(pkg, oracle, bits):
    """80 sets from one launch, every one against the oracle; the halves of equal messages differ (their streams do)."""
    gb, _ = _check(pkg, oracle, ("many", bits))
    assert len({gb[e].tobytes() for e in range(gb.shape[0])}) == gb.shape[0] == 2 * MANY


CHILD = """import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import importlib
import numpy as np
pkg = importlib.import_module("gpu-homomorphic-encryption_amd")
import test_rgsw_keygen_edges as t
out = {{}}
for i, key in enumerate(t.AGAIN):
    c = t.CASES[key][0]
    out[f"b_{{i}}"], out[f"a_{{i}}"] = t._run(pkg, c, t._secret(None, c))
np.savez(sys.argv[1], **out)
"""


@pytest.mark.gpu
def test_the_composed_path_gives_the_same_bits_on_every_edge_case(pkg, oracle, tmp_path):
    """FHE_HIP_NO_FUSED_KEYGEN=1 in ONE child process (the switch is read at engine creation) for every n = 2048 case of the instance, limb and
    gadget tests: rgsw_target_kernel and generate_composed give the oracle's rows and the fused path's."""
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
def test_sizes_that_take_the_composed_path(pkg, oracle, name):
    """N = 2^15: L = 3, K = 2, mu = 0 and -3.  N = 2^16: L = 2, K = 2, mu = 0 and -2^15.  The halves of mu = 0 are encryptions of zero: the target
    rgsw_target_kernel builds is 0 (component 0) or 0 s^ (component 1)."""
    _check(pkg, oracle, ("by-itself", name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(UNPACKED))
def test_unpacked_key_sets_on_a_word_sized_class(pkg, oracle, name):
    """12289 beside a 30-bit prime with w = 30, and the FP64 field with L K = 86 products: the sets keep containers and generation composes on a
    word-sized class.  L K = 80 is the packed, fused neighbour.  mu = 0 and -1."""
    c = CASES["unpacked", name][0]
    assert pkg.RnsNttEngine(c.n, list(c.moduli)).width_class == WIDTH[_class(c)]
    _check(pkg, oracle, ("unpacked", name))


@pytest.mark.gpu
@pytest.mark.parametrize("bits,log_n", CONSUMER_IDS)
def test_blind_rotation_step_at_the_larger_sizes(pkg, oracle, bits, log_n):
    """fhe_blind_rotate_step with the handles of the instance case (message 2: mu = 2^15) equals the oracle's step on the ORACLE's rows"""
    c = CASES["instance", bits, log_n][0]
    n, moduli, batch, i = c.n, list(c.moduli), 2, 2
    s, wb, wa = _want(oracle, c)
    e, r0, r1, _keep = _generate(pkg, n, moduli, c.w, list(c.mus), s)
    acc0, acc1 = rns_poly(70, moduli, n, batch), rns_poly(71, moduli, n, batch)
    shifts = np.array([5, 2 * n - 3], dtype=np.uint32)
    d0, d1 = pkg.DeviceBuffer.from_numpy(acc0), pkg.DeviceBuffer.from_numpy(acc1)
    t0, t1, dsh = pkg.DeviceBuffer(acc0.nbytes), pkg.DeviceBuffer(acc0.nbytes), pkg.DeviceBuffer.from_numpy(shifts)
    e.blind_rotate_step(r0[i], r1[i], d0, d1, dsh, t0, t1, batch)
    rows0, rows1 = (list(wb[2 * i]), list(wa[2 * i])), (list(wb[2 * i + 1]), list(wa[2 * i + 1]))
    w0, w1 = oracle.RnsPlan(n, moduli).blind_rotate_step(c.w, acc0, acc1, shifts, rows0, rows1, threads=8)
    assert np.array_equal(d0.download(acc0.shape), w0) and np.array_equal(d1.download(acc0.shape), w1)
    LK = len(moduli) * _digits(c)
    gb, ga = _export(pkg, e, r1[i], n, len(moduli), LK)                                       # the set is unchanged by its use
    assert np.array_equal(ga, wa[2 * i + 1]) and np.array_equal(gb, wb[2 * i + 1])
