"""CPU tests of the LWE key switch back to the small key: the model (lwe_keyswitch_model) against its own definitions, the q_out rounding
against a rational computation, the noise the bootstrapping chain test relies on, and the header / library / binding surface (the test
that fails before the feature exists)."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import lwe_keyswitch_model as km
import ntt_math as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fhe_lwe_ksk_num_digits", "fhe_lwe_ksk_create", "fhe_lwe_ksk_export", "fhe_lwe_ksk_destroy", "fhe_lwe_ksk_bytes",
               "fhe_lwe_ksk_generate", "fhe_lwe_keyswitch")

# The shape of tests/test_bootstrap_chain.py: the seeds committed there are checked here, on the CPU, to keep the model inside the bound
CHAIN = dict(n=2048, w=8, n_lwe=12, p=8, sigma=3.2, noise_scale=1, seeds=(31, 32), batch=4)


def test_header_library_and_binding_have_the_new_symbols(pkg):
    with open(os.path.join(ROOT, "include", "fhe_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(fhe_[a-z0-9_]+)\s*\(", text))
    lib = pkg.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, f"include/fhe_hip.h does not declare {name}"
        assert hasattr(lib, name), f"libfhe_hip.so does not export {name}"
    assert "fhe_lwe_ksk_t" in text
    for method in ("lwe_ksk_num_digits", "import_lwe_ksk", "generate_lwe_ksk", "export_lwe_ksk", "lwe_keyswitch"):
        assert callable(getattr(pkg.RnsNttEngine, method)), method
    # rejected before a device is needed, outputs untouched
    out = ctypes.c_void_p(0x1234)
    z = (ctypes.c_int32 * 1)(1); seeds = (ctypes.c_uint64 * 2)(1, 2)
    assert lib.fhe_lwe_ksk_generate(None, None, 8, 1, z, 1, 3.2, seeds, ctypes.byref(out)) == -1
    assert lib.fhe_lwe_ksk_create(None, ctypes.byref(out), 8, 1, None) == -1
    assert out.value == 0x1234
    assert lib.fhe_lwe_keyswitch(None, None, 0, None, None, 1) == -1
    assert lib.fhe_lwe_ksk_export(None, None, None) == -1
    assert lib.fhe_lwe_ksk_destroy(None) == 0


def test_vectorised_streams_equal_the_oracle(oracle):
    idx = [0, 1, 2, 12345, (1 << 40) + 7, (1 << 63) + 5]
    for seed in (0, 31, (1 << 64) - 1):
        for draw in (km.DRAW_CDT, km.DRAW_SIGN, km.DRAW_UNIFORM, km.DRAW_UNIFORM + 4 * 63):
            got = km.ctr_rand_np(seed, idx, draw)
            assert [int(v) for v in got] == [oracle.ctr_rand(seed, i, draw) for i in idx]


@pytest.mark.parametrize("q,w,sigma,t", [(nm.ntt_primes(30, 8, 1)[0], 8, 3.2, 1), (nm.largest_ntt_primes(64, 8, 1)[0], 32, 3.2, 65537),
                                         ((1 << 61) - 1, 1, 90.0, 1), (12289, 5, 3.2, 7)])
def test_numpy_generation_equals_the_integer_definition(oracle, q, w, sigma, t):
    rng = np.random.default_rng(q % 1000 + w)
    s = [int(rng.integers(0, min(q, 1 << 62))) % q for _ in range(4)]
    z = [1, -1, -(1 << 15), 1 << 15, 0][:5]
    seeds = (int(rng.integers(1, 1 << 62)), int(rng.integers(1, 1 << 62)))
    want = km.ksk_generate(oracle, q, s, z, w, t, sigma, seeds)
    got = km.ksk_generate_np(oracle, q, s, z, w, t, sigma, seeds)
    assert [[int(v) for v in row] for row in got] == want
    assert list(km.ksk_noise_np(oracle, 4, km.num_digits(q, w), sigma, seeds)) == km.ksk_noise(oracle, 4, km.num_digits(q, w), sigma, seeds)


@pytest.mark.parametrize("q,w", [(nm.ntt_primes(30, 8, 1)[0], 8), (nm.ntt_primes(43, 8, 1)[0], 7), ((1 << 61) - 1, 16),
                                 (nm.largest_ntt_primes(64, 8, 1)[0], 32), (nm.largest_ntt_primes(64, 8, 1)[0], 3)])
@pytest.mark.parametrize("q_out", [0, 2, 1 << 32, 1 << 48, 1000003])
def test_numpy_product_equals_the_integer_definition(q, w, q_out):
    rng = np.random.default_rng(w)
    K, n_in, n_out, batch = km.num_digits(q, w), 5, 3, 3
    rnd = lambda: (int(rng.integers(0, 1 << 62)) << 2 | int(rng.integers(0, 4))) % q
    rows = [[rnd() for _ in range(n_out + 1)] for _ in range(n_in * K)]
    lwe = [[rnd() for _ in range(n_in + 1)] for _ in range(batch)]
    rows[0] = [q - 1] * (n_out + 1); lwe[0] = [q - 1] * (n_in + 1)
    want = km.keyswitch(q, w, rows, lwe, q_out)
    got = km.keyswitch_np(q, w, np.array(rows, dtype=np.uint64), np.array(lwe, dtype=np.uint64), q_out)
    assert [[int(v) for v in r] for r in got] == want


@pytest.mark.parametrize("q,w,t", [(nm.ntt_primes(30, 8, 1)[0], 8, 1), (nm.ntt_primes(43, 8, 1)[0], 11, 65537), ((1 << 61) - 1, 20, 3),
                                   (nm.largest_ntt_primes(64, 8, 1)[0], 32, 1)])
def test_output_phase_is_input_phase_plus_digit_noise(oracle, q, w, t):
    """phase_z(out) = phase_s(in) + noise_scale sum d e, exactly (as integers modulo q), for a general (not small) s and signed z"""
    rng = np.random.default_rng(w + t)
    n_in, n_out = 6, 4
    K = km.num_digits(q, w)
    for trial in range(3):
        s = [(int(rng.integers(0, 1 << 62)) << 2) % q for _ in range(n_in)]
        z = [int(v) for v in rng.integers(-3, 4, n_out)]
        seeds = (100 + trial, 200 + trial)
        rows = km.ksk_generate(oracle, q, s, z, w, t, 3.2, seeds)
        e = km.ksk_noise(oracle, n_in, K, 3.2, seeds)
        lwe = [[(int(rng.integers(0, 1 << 62)) << 2) % q for _ in range(n_in + 1)] for _ in range(2)]
        out = km.keyswitch(q, w, rows, lwe)
        for ct, o in zip(lwe, out):
            want = (ct[-1] + sum(a * sj for a, sj in zip(ct[:-1], s)) + km.digit_noise(q, w, ct, e, t)) % q
            got = (o[-1] + sum(a * zi for a, zi in zip(o[:-1], z))) % q
            assert got == want


@pytest.mark.parametrize("q", [nm.ntt_primes(30, 8, 1)[0], (1 << 61) - 1, nm.largest_ntt_primes(64, 8, 1)[0], 12289])
@pytest.mark.parametrize("q_out", [2, 3, 1 << 32, 1 << 48, 1000003])
def test_rounding_against_rationals(q, q_out):
    """floor((acc q_out + floor(q / 2)) / q) mod q_out is round-half-up of acc q_out / q for odd q (no tie); the cases where the numerator
    is an exact multiple of q are included: acc with acc q_out + floor(q / 2) = m q"""
    rng = np.random.default_rng(5)
    cases = [0, 1, q - 1, q // 2, q // 2 + 1] + [int(rng.integers(0, 1 << 62)) % q for _ in range(50)]
    # the numerator is an exact multiple of q for exactly one acc below q (q_out is invertible modulo the prime q), and its neighbours
    # sit on either side of the step
    exact = (-(q // 2) * pow(q_out, -1, q)) % q
    assert (exact * q_out + q // 2) % q == 0
    cases += [exact, (exact - 1) % q, (exact + 1) % q]
    for acc in cases:
        x = Fraction(acc * q_out, q)
        r = (x + Fraction(q // 2, q)).__floor__()                   # the contract, over the rationals
        assert abs(x - r) <= Fraction(1, 2)                         # it is a nearest integer: q is odd, so x is never half-way
        assert km.round_to(acc, q, q_out) == r % q_out, (acc, q, q_out)
    if q_out <= q:
        assert km.round_to(q - 1, q, q_out) in (0, q_out - 1)      # the top of the range wraps to 0 or stays at q_out - 1


def _chain_setup(oracle):
    """the key and inputs of test_bootstrap_chain.py, from the same constants: ring key, LWE key, key-switching noise"""
    c = CHAIN
    q0 = nm.ntt_primes(30, c["n"], 2)[0]
    K = km.num_digits(q0, c["w"])
    e = km.ksk_noise_np(oracle, c["n"], K, c["sigma"], c["seeds"])
    return q0, K, e


def test_chain_noise_stays_inside_the_bound(oracle, golden_dir):
    """noise_scale sum d e for the key and the inputs of the chain test, through the model, against Delta_1 / 4.  The key noise e_r comes
    from the committed seeds; the inputs are the four samples the chain extracts after its first bootstrap, recorded once in
    tests/golden/bootstrap_chain_extracted.json (the pipeline is exact, so every device gives these bits, and the GPU test asserts that it
    does).  Beside the exact values, the moments for uniform digits (mean (2^w - 1) / 2 sum e, variance (4^w - 1) / 12 sum e^2 for THIS e)
    say how much room other inputs would have."""
    import json
    c = CHAIN
    q0, K, e = _chain_setup(oracle)
    delta1 = q0 // (2 * c["p"])
    with open(os.path.join(golden_dir, "bootstrap_chain_extracted.json")) as f:
        samples = json.load(f)["extracted"]
    assert len(samples) == c["batch"] and all(len(ct) == c["n"] + 1 and max(ct) < q0 for ct in samples)
    e_int = [int(v) for v in e]
    worst = max(abs(km.digit_noise(q0, c["w"], ct, e_int, c["noise_scale"])) for ct in samples)
    print(f"chain key switch: worst |noise_scale sum d e| over the chain's own {len(samples)} samples: {worst.bit_length()} bits, "
          f"Delta_1 / 4 = 2^{np.log2(delta1 / 4):.1f}")
    assert worst < delta1 // 4
    e = np.asarray(e, dtype=np.int64)
    mean = (2 ** c["w"] - 1) / 2 * float(e.sum())
    std = (((4 ** c["w"] - 1) / 12) * float((e * e).sum())) ** 0.5
    print(f"chain key switch: K = {K}, rows = {e.size}, sum e = {int(e.sum())}, |mean| = 2^{np.log2(abs(mean) + 1):.1f}, std = 2^{np.log2(std):.1f}")
    assert abs(mean) + 6 * std < delta1 / 4
