"""Programmable bootstrapping end to end: LWE ciphertexts in, fhe_lwe_prepare_accumulator -> fhe_blind_rotate over generated RGSW rows ->
fhe_rlwe_sample_extract, LWE samples of f(m) under the ring key out.

N = 2048, two 30-bit primes, w = 16, n_lwe = 12 random secret bits, p = 8, q_lwe = 2^32, batch 4.  Inputs have phase m q_lwe / (2p) + q_lwe / (4p) + small
noise; tv[i] = Delta f(floor(i p / N)), Delta = floor(Q / (2p)).  (i) the extracted samples equal model-prepare -> oracle blind rotation on the exported
rows -> model-extract bit for bit; (ii) their phase under s, CRT-centred, is within Delta / 2 of Delta f(m) (the measured noise is printed)."""
import numpy as np
import pytest

import bootstrap_model as bm
from test_encrypt import _containers
from test_keygen import _export, _primes

N, L, W, N_LWE, P_SPACE, Q_LWE, BATCH = 2048, 2, 16, 12, 8, 1 << 32, 4
MSGS = (0, 3, 5, 7)
TABLES = {"identity": list(range(P_SPACE)), "table": [5, 1, 7, 0, 3, 3, 6, 2]}

_state = {}


def _setup(pkg):
    """engine, ring key (ternary), LWE key bits, generated RGSW rows and their exports: once for the module"""
    if not _state:
        moduli = _primes(30, N, L)
        rng = np.random.default_rng(17)
        s = rng.integers(-1, 2, N)
        s_c = _containers(np.stack([np.array([int(v) % q for v in s], dtype=object) for q in moduli]))
        eng = pkg.RnsNttEngine(N, moduli)
        ds = pkg.DeviceBuffer.from_numpy(s_c)
        sk = eng.import_secret_key(ds)
        z = [int(v) for v in rng.integers(0, 2, N_LWE)]
        r0, r1 = eng.generate_rgsw_keys(sk, W, z, 1, 3.2, (21, 22))
        LK = L * eng.relin_num_digits(W)
        rows0 = [_export(pkg, eng, rk, N, L, LK) for rk in r0]
        rows1 = [_export(pkg, eng, rk, N, L, LK) for rk in r1]
        lwe = []
        for m in MSGS:
            a = [int(v) for v in rng.integers(0, Q_LWE, N_LWE)]
            phase = m * Q_LWE // (2 * P_SPACE) + Q_LWE // (4 * P_SPACE) + int(rng.integers(-1000, 1001))
            lwe.append(a + [(phase - sum(ai * zi for ai, zi in zip(a, z))) % Q_LWE])
        _state.update(moduli=moduli, s=[int(v) for v in s], eng=eng, keep=(ds, sk), z=z, r0=r0, r1=r1, rows0=rows0, rows1=rows1,
                      lwe=np.array(lwe, dtype=np.uint64))
    return _state


def _test_vector(moduli, f):
    Q = 1
    for q in moduli:
        Q *= q
    delta = Q // (2 * P_SPACE)
    tv_int = [delta * f[i * P_SPACE // N] for i in range(N)]
    return Q, delta, _containers(np.stack([np.array([v % q for v in tv_int], dtype=object) for q in moduli]))


def _device(pkg, st, tv):
    eng, S = st["eng"], L * N * 32
    d_lwe, d_tv = pkg.DeviceBuffer.from_numpy(st["lwe"]), pkg.DeviceBuffer.from_numpy(tv)
    acc = [pkg.DeviceBuffer(BATCH * S) for _ in range(4)]
    d_sh, d_out = pkg.DeviceBuffer(N_LWE * BATCH * 4), pkg.DeviceBuffer(BATCH * L * (N + 1) * 8)
    eng.lwe_prepare_accumulator(Q_LWE, N_LWE, d_lwe, d_tv, acc[0], acc[1], d_sh, BATCH)
    eng.blind_rotate(st["r0"], st["r1"], acc[0], acc[1], d_sh, acc[2], acc[3], BATCH)
    eng.sample_extract(d_out, acc[0], acc[1], 0, BATCH)
    return d_out.download((BATCH, L, N + 1))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TABLES))
def test_bootstrap_evaluates_the_table(pkg, oracle, name):
    st = _setup(pkg)
    moduli, f = st["moduli"], TABLES[name]
    Q, delta, tv = _test_vector(moduli, f)
    got = _device(pkg, st, tv)
    # (i) the same pipeline from the model and the oracle, on the exported rows
    acc0, shifts = bm.prepare_np(st["lwe"], tv[..., 0], moduli, Q_LWE)
    a0 = _containers(acc0); a1 = np.zeros_like(a0)
    rows0 = [(list(b), list(a)) for b, a in st["rows0"]]; rows1 = [(list(b), list(a)) for b, a in st["rows1"]]
    w0, w1 = oracle.RnsPlan(N, moduli).blind_rotate(W, a0, a1, shifts, rows0, rows1, threads=8)
    want = bm.extract_np(w0[..., 0], w1[..., 0], moduli, 0)
    assert np.array_equal(got, want)
    # (ii) the phase of every sample is Delta f(m) up to noise below Delta / 2
    worst = 0
    for b, m in enumerate(MSGS):
        phi = (bm.ms(int(st["lwe"][b, -1]), Q_LWE, N) + sum(bm.ms(int(a), Q_LWE, N) * zi for a, zi in zip(st["lwe"][b, :-1], st["z"]))) % (2 * N)
        assert phi < N and phi * P_SPACE // N == m
        phase = bm.lwe_phase([[int(v) for v in got[b, l]] for l in range(L)], st["s"], moduli)
        err = abs(phase - delta * f[m])
        worst = max(worst, err)
        assert err < delta // 2, (b, m, err.bit_length(), delta.bit_length())
    print(f"bootstrap {name}: noise {worst.bit_length()} bits, Delta / 2 is {(delta // 2).bit_length()} bits")
