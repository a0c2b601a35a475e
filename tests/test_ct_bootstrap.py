"""FHEContext::bootstrap(Ciphertext&) end to end through capi: a ciphertext in, a refreshed ciphertext of f(m) out.

The shape of test_bootstrap_chain.py: N = 2048, two 30-bit primes, RGSW w = 16, key switch w = 8, n_lwe = 12 secret bits, p = 8, q_lwe = 2^32,
packing keys w = 16, all noise scales 1, sigma 3.2; count = 4.  The pipeline of DESIGN 4.19 on the device, nothing on the host in between:
fhe_rns_rescale_drop_last to one prime -> fhe_rlwe_sample_extract_strided -> fhe_lwe_keyswitch (q_out = q_lwe) -> fhe_lwe_prepare_accumulator ->
fhe_blind_rotate (batch = count) -> fhe_rlwe_pack (trace, normalisation).  Coefficient i n / 4 of the input has phase Delta m_i + Delta / 2 + e,
Delta = floor(Q / (2p)); of the output Delta f(m_i) + e', and every other coefficient e'.  Two ciphertexts carry the 8 messages.  Decryption is
fhe_ct_decrypt with t = 2^63, which returns the centred phase itself (Q < 2^60); its d_noise_bits on the ciphertext minus the ideal plaintext is
the noise, asserted below bit_length(Delta / 2) = 54.

Measured on an MI355X (printed by the tests): 34-35 bits of noise after one bootstrap with either table, 34-35 bits after the second of two."""
import numpy as np
import pytest

from test_bootstrap_end_to_end import TABLES
from test_encrypt import _embed, _keygen
from test_keygen import _primes
from test_lwe_keyswitch_model import CHAIN

N, L, W, W_KS, W_PACK, N_LWE, P_SPACE, Q_LWE, COUNT = CHAIN["n"], 2, 16, CHAIN["w"], 16, CHAIN["n_lwe"], CHAIN["p"], 1 << 32, 4
SIGMA = 3.2
MESSAGES = ((0, 3, 5, 7), (1, 2, 4, 6))                       # all 8, four per ciphertext
F, G = TABLES["table"], [2, 7, 1, 1, 6, 0, 4, 3]
T_RAW = 1 << 63                                               # fhe_ct_decrypt with this t returns v mod 2^63, |v| < Q / 2 < 2^59

_state = {}


def _setup(pkg, oracle):
    if not _state:
        moduli = _primes(30, N, L)
        s, pk0, pk1 = _keygen(oracle, N, moduli, 2, 71)
        eng, eng1 = pkg.RnsNttEngine(N, moduli), pkg.RnsNttEngine(N, moduli[:1])
        src = (pkg.DeviceBuffer.from_numpy(pk0), pkg.DeviceBuffer.from_numpy(pk1))
        pk = eng.import_public_key(*src)
        ds = pkg.DeviceBuffer.from_numpy(_embed(s[None], moduli)[0])
        sk = eng.import_secret_key(ds)
        z = [int(v) for v in np.random.default_rng(17).integers(0, 2, N_LWE)]
        r0, r1 = eng.generate_rgsw_keys(sk, W, z, 1, SIGMA, (21, 22))
        ksk = eng.generate_lwe_ksk(sk, W_KS, z, CHAIN["noise_scale"], CHAIN["sigma"], CHAIN["seeds"])
        pack = eng.generate_keyswitch_keys(sk, W_PACK, pkg.capi.lwe_pack_galois_elements(N), 1, SIGMA, (0x51, 0x52))
        Q = moduli[0] * moduli[1]
        _state.update(moduli=moduli, Q=Q, delta=Q // (2 * P_SPACE), eng=eng, eng1=eng1, pk=pk, sk=sk, keep=(src, ds), r0=r0, r1=r1, ksk=ksk, pack=pack)
    return _state


def _plain(st, values):
    """[L][n] containers of the polynomial with values[i] at coefficient i n / COUNT and 0 elsewhere"""
    v = np.zeros(N, dtype=object)
    v[::N // COUNT] = values
    return _embed(v[None], st["moduli"])


def _tv(st, table, offset):
    delta = st["delta"]
    return _embed(np.array([delta * table[i * P_SPACE // N] + (delta // 2 if offset else 0) for i in range(N)], dtype=object)[None], st["moduli"])


def _encrypt(pkg, st, msgs, seed):
    delta, S = st["delta"], L * N * 32
    c0, c1 = pkg.DeviceBuffer(S), pkg.DeviceBuffer(S)
    st["eng"].encrypt(st["pk"], 2, SIGMA, (seed, seed + 1, seed + 2), c0, c1, pkg.DeviceBuffer.from_numpy(_plain(st, [delta * m + delta // 2 for m in msgs])), 1)
    return c0, c1


def _bootstrap(pkg, st, c0, c1, tv):
    """the six steps; each engine has a stream of its own, so the device is synchronised where the work passes from one to the other"""
    eng, eng1, S = st["eng"], st["eng1"], L * N * 32
    low = [pkg.DeviceBuffer(N * 32) for _ in range(2)]
    eng.rescale_drop_last(low[0], c0, 1); eng.rescale_drop_last(low[1], c1, 1)
    pkg.capi.sync()
    d_ext, d_ks = pkg.DeviceBuffer(COUNT * (N + 1) * 8), pkg.DeviceBuffer(COUNT * (N_LWE + 1) * 8)
    eng1.sample_extract_strided(d_ext, low[0], low[1], COUNT, 1)
    eng1.lwe_keyswitch(st["ksk"], d_ks, d_ext, Q_LWE, COUNT)
    pkg.capi.sync()
    acc = [pkg.DeviceBuffer(COUNT * S) for _ in range(4)]
    d_sh, d_tv = pkg.DeviceBuffer(N_LWE * COUNT * 4), pkg.DeviceBuffer.from_numpy(tv)
    eng.lwe_prepare_accumulator(Q_LWE, N_LWE, d_ks, d_tv, acc[0], acc[1], d_sh, COUNT)
    eng.blind_rotate(st["r0"], st["r1"], acc[0], acc[1], d_sh, acc[2], acc[3], COUNT)
    o0, o1 = pkg.DeviceBuffer(S), pkg.DeviceBuffer(S)
    eng.rlwe_pack(st["pack"], o0, o1, acc[0], acc[1], COUNT, True, True, 1)
    pkg.capi.sync()
    return o0, o1


def _phases(pkg, st, c0, c1):
    """(centred phase of every coefficient as Python integers, d_noise_bits) from fhe_ct_decrypt"""
    dm, dn = pkg.DeviceBuffer(N * 8), pkg.DeviceBuffer(4)
    st["eng"].decrypt(st["sk"], T_RAW, 1, dm, dn, [c0, c1], 1)
    v = dm.download((N,)).astype(object)
    return np.where(v >= T_RAW // 2, v - T_RAW, v), int(dn.download((1,), np.uint32)[0])


def _check_output(pkg, st, o0, o1, want, what):
    """every target coefficient decodes to want[i], every other coefficient to 0, and the noise stays below Delta / 2"""
    delta, step = st["delta"], N // COUNT
    v, _ = _phases(pkg, st, o0, o1)
    decoded = [int((2 * int(x) + delta) // (2 * delta)) % (2 * P_SPACE) for x in v]
    assert [decoded[i * step] for i in range(COUNT)] == list(want), what
    assert all(d == 0 for k, d in enumerate(decoded) if k % step), what
    diff = pkg.DeviceBuffer(L * N * 32)
    st["eng"].poly_sub(diff, o0, pkg.DeviceBuffer.from_numpy(_plain(st, [delta * w for w in want])), 1)
    _, bits = _phases(pkg, st, diff, o1)
    print(f"ciphertext bootstrap, {what}: d_noise_bits {bits}, Delta / 2 has {(delta // 2).bit_length()} bits")
    assert bits < (delta // 2).bit_length(), what
    return bits


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TABLES))
def test_bootstrap_refreshes_the_ciphertext_and_evaluates_the_table(pkg, oracle, name):
    st, f = _setup(pkg, oracle), TABLES[name]
    for k, msgs in enumerate(MESSAGES):
        c0, c1 = _encrypt(pkg, st, msgs, 100 + 10 * k)
        v, bits = _phases(pkg, st, c0, c1)                                       # the input decodes to m, as encrypted
        assert [int(v[i * N // COUNT]) // st["delta"] for i in range(COUNT)] == list(msgs)
        o0, o1 = _bootstrap(pkg, st, c0, c1, _tv(st, f, False))
        _check_output(pkg, st, o0, o1, [f[m] for m in msgs], f"{name} {msgs}")


@pytest.mark.gpu
def test_a_second_bootstrap_of_the_output_decodes_too(pkg, oracle):
    """f with the half-slot offset in the table, so that the first output sits mid-slot, then g: every target coefficient decodes to g(f(m))"""
    st = _setup(pkg, oracle)
    for k, msgs in enumerate(MESSAGES):
        c0, c1 = _encrypt(pkg, st, msgs, 200 + 10 * k)
        m0, m1 = _bootstrap(pkg, st, c0, c1, _tv(st, F, True))
        v, _ = _phases(pkg, st, m0, m1)
        assert [int(v[i * N // COUNT]) // st["delta"] for i in range(COUNT)] == [F[m] for m in msgs]
        o0, o1 = _bootstrap(pkg, st, m0, m1, _tv(st, G, False))
        _check_output(pkg, st, o0, o1, [G[F[m]] for m in msgs], f"g(f(m)) {msgs}")
