"""Two bootstraps in a row, the second fed by the first with nothing on the host in between: the LWE key switch closes the loop.

N = 2048, two 30-bit primes, RGSW w = 16, n_lwe = 12 secret bits, p = 8, batch 4 (the shape of test_bootstrap_end_to_end.py); key switch w = 8,
sigma = 3.2, noise_scale = 1.  LWE(m) under z at q_lwe = 2^32 -> prepare, loop with the table f (test vector Delta f + Delta / 2: the half-slot
offset puts the output mid-slot for the next prepare), rescale to one prime, extract, key switch (q_out = 0) -> prepare with q_lwe = q_0, loop
with the table g, rescale, extract.  (i) the key-switched sample equals the model applied to the device's own extracted sample, bit for bit;
(ii) its phase under z is within Delta_1 / 2 of Delta_1 f(m) + Delta_1 / 2, Delta_1 = floor(q_0 / (2p)); (iii) the final sample's phase under s
decodes to g(f(m)), for every message of the batch.

Measured on an MI355X (printed by the test): 4 bits of noise after rescale + extract, the key switch adds 15 bits, 15 bits after it against
Delta_1 / 2 of 25 bits; 5 bits after the second bootstrap."""
import ctypes
import json
import os

import numpy as np
import pytest

import bootstrap_model as bm
import lwe_keyswitch_model as km
from test_encrypt import _containers
from test_keygen import _primes
from test_lwe_keyswitch_model import CHAIN

N, L, W, N_LWE, P_SPACE, Q_LWE, BATCH = CHAIN["n"], 2, 16, CHAIN["n_lwe"], CHAIN["p"], 1 << 32, CHAIN["batch"]
W_KS = CHAIN["w"]
MSGS = (0, 3, 5, 7)
F = [5, 1, 7, 0, 3, 3, 6, 2]
G = [2, 7, 1, 1, 6, 0, 4, 3]


def _hip_runtime():
    """the HIP runtime this process already holds (the one the library is linked against), for a stream of the test's own"""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(paths) == 1, paths
    return ctypes.CDLL(paths.pop())


def _tv(moduli, values):
    return _containers(np.stack([np.array([v % q for v in values], dtype=object) for q in moduli]))


def run_chain(pkg, oracle):
    """the whole chain on the device; returns what the assertions need (also used to record tests/golden/bootstrap_chain_extracted.json)"""
    moduli = _primes(30, N, L)
    q0 = moduli[0]
    Q = moduli[0] * moduli[1]
    delta, delta1 = Q // (2 * P_SPACE), q0 // (2 * P_SPACE)
    rng = np.random.default_rng(17)
    s = [int(v) for v in rng.integers(-1, 2, N)]
    eng, eng1 = pkg.RnsNttEngine(N, moduli), pkg.RnsNttEngine(N, moduli[:1])
    # the chain alternates between the level-0 engine and the one-limb engine, and every call is enqueued on its engine's stream without a
    # synchronisation: both engines go on ONE stream, which orders them on the device
    hip, side = _hip_runtime(), ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(side)) == 0
    eng.set_stream(side); eng1.set_stream(side)
    ds = pkg.DeviceBuffer.from_numpy(_containers(np.stack([np.array([v % q for v in s], dtype=object) for q in moduli])))
    sk = eng.import_secret_key(ds)
    z = [int(v) for v in rng.integers(0, 2, N_LWE)]
    r0, r1 = eng.generate_rgsw_keys(sk, W, z, 1, 3.2, (21, 22))
    ksk = eng.generate_lwe_ksk(sk, W_KS, z, CHAIN["noise_scale"], CHAIN["sigma"], CHAIN["seeds"])
    K = km.num_digits(q0, W_KS)
    d_rows = pkg.DeviceBuffer(N * K * (N_LWE + 1) * 8)
    eng.export_lwe_ksk(ksk, d_rows)
    rows = d_rows.download((N * K, N_LWE + 1))
    assert np.array_equal(rows, km.ksk_generate_np(oracle, q0, [v % q0 for v in s], z, W_KS, CHAIN["noise_scale"], CHAIN["sigma"], CHAIN["seeds"]))

    lwe = []
    for m in MSGS:
        a = [int(v) for v in rng.integers(0, Q_LWE, N_LWE)]
        phase = m * Q_LWE // (2 * P_SPACE) + Q_LWE // (4 * P_SPACE) + int(rng.integers(-1000, 1001))
        lwe.append(a + [(phase - sum(ai * zi for ai, zi in zip(a, z))) % Q_LWE])
    d_lwe = pkg.DeviceBuffer.from_numpy(np.array(lwe, dtype=np.uint64))
    tv_f = pkg.DeviceBuffer.from_numpy(_tv(moduli, [delta * F[i * P_SPACE // N] + delta // 2 for i in range(N)]))
    tv_g = pkg.DeviceBuffer.from_numpy(_tv(moduli, [delta * G[i * P_SPACE // N] for i in range(N)]))

    S = L * N * 32
    acc = [pkg.DeviceBuffer(BATCH * S) for _ in range(4)]
    low = [pkg.DeviceBuffer(BATCH * N * 32) for _ in range(2)]
    d_sh = pkg.DeviceBuffer(N_LWE * BATCH * 4)
    d_ext, d_ks, d_fin = pkg.DeviceBuffer(BATCH * (N + 1) * 8), pkg.DeviceBuffer(BATCH * (N_LWE + 1) * 8), pkg.DeviceBuffer(BATCH * (N + 1) * 8)

    def bootstrap(q_lwe, d_in, tv, d_out):
        """prepare -> loop -> rescale to one prime -> extract, all on the device"""
        eng.lwe_prepare_accumulator(q_lwe, N_LWE, d_in, tv, acc[0], acc[1], d_sh, BATCH)
        eng.blind_rotate(r0, r1, acc[0], acc[1], d_sh, acc[2], acc[3], BATCH)
        eng.rescale_drop_last(low[0], acc[0], BATCH)
        eng.rescale_drop_last(low[1], acc[1], BATCH)
        eng1.sample_extract(d_out, low[0], low[1], 0, BATCH)

    bootstrap(Q_LWE, d_lwe, tv_f, d_ext)
    eng1.lwe_keyswitch(ksk, d_ks, d_ext, 0, BATCH)
    bootstrap(q0, d_ks, tv_g, d_fin)                      # nothing came back to the host in between

    pkg.capi.sync()
    eng.set_stream(None); eng1.set_stream(None)
    assert hip.hipStreamDestroy(side) == 0
    ext, ks, fin = d_ext.download((BATCH, N + 1)), d_ks.download((BATCH, N_LWE + 1)), d_fin.download((BATCH, N + 1))
    return dict(moduli=moduli, s=s, z=z, rows=rows, K=K, ext=ext, ks=ks, fin=fin)


@pytest.mark.gpu
def test_two_bootstraps_in_a_row(pkg, oracle, golden_dir):
    c = run_chain(pkg, oracle)
    moduli, s, z, rows, K, ext, ks, fin = (c[k] for k in ("moduli", "s", "z", "rows", "K", "ext", "ks", "fin"))
    q0, delta1 = moduli[0], moduli[0] // (2 * P_SPACE)
    # the extracted samples are the ones the CPU test bounds the key-switch noise for (exact arithmetic: the same bits on every device)
    with open(os.path.join(golden_dir, "bootstrap_chain_extracted.json")) as f:
        assert [[int(v) for v in row] for row in ext] == json.load(f)["extracted"]
    # (i) the model on the device's own extracted sample
    assert np.array_equal(ks, km.keyswitch_np(q0, W_KS, rows, ext))
    e = [int(v) for v in km.ksk_noise_np(oracle, N, K, CHAIN["sigma"], CHAIN["seeds"])]
    worst_in = worst_ks = worst_added = worst_fin = 0
    for b, m in enumerate(MSGS):
        target = delta1 * F[m] + delta1 // 2
        err_in = abs(km.lwe_phase(q0, ext[b], s) - target)
        added = km.digit_noise(q0, W_KS, [int(v) for v in ext[b]], e, CHAIN["noise_scale"])
        err = abs(km.lwe_phase(q0, ks[b], z) - target)
        worst_in, worst_ks, worst_added = max(worst_in, err_in), max(worst_ks, err), max(worst_added, abs(added))
        assert (km.lwe_phase(q0, ks[b], z) - km.lwe_phase(q0, ext[b], s) - added) % q0 == 0          # the phase identity, exactly
        assert abs(added) < delta1 // 4, (b, abs(added).bit_length())                                 # what the CPU test bounds for these seeds
        # (ii)
        assert err < delta1 // 2, (b, m, err.bit_length(), (delta1 // 2).bit_length())
        # (iii)
        phase = bm.lwe_phase([[int(v) for v in fin[b]]], s, moduli[:1])
        worst_fin = max(worst_fin, abs(phase - delta1 * G[F[m]]))
        assert (2 * phase + delta1) // (2 * delta1) % (2 * P_SPACE) == G[F[m]], (b, m, F[m], G[F[m]])
    print(f"bootstrap chain: noise after rescale + extract {worst_in.bit_length()} bits, key switch adds {worst_added.bit_length()} bits, "
          f"after the key switch {worst_ks.bit_length()} bits, Delta_1 / 2 is {(delta1 // 2).bit_length()} bits; second bootstrap {worst_fin.bit_length()} bits")
