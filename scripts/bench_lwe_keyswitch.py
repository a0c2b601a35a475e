#!/usr/bin/env python3
"""fhe_lwe_keyswitch against what does the same today, at the same shape, in one process, interleaved in time (every round runs every candidate
once; the MEDIAN of the rounds counts).  Every comparator is checked equal to the new path's output before it is timed.
(a) the call: ONE fhe_lwe_keyswitch on a generated key, in the accumulator form the key picks and, where that is the 64-bit form, also on a key
    created under FHE_HIP_LWE_KSK_WIDE=1 (the 128-bit form on the same shape).
(b) the host path: download of the [batch][N + 1] sample, the digit matrix times the key matrix in numpy (uint64 where it cannot overflow,
    16-bit pieces recombined as Python integers otherwise: lwe_keyswitch_model.keyswitch_np), upload of the result.  The product is timed ONCE
    on the first HOST_BATCH ciphertexts (it takes seconds) and reported per ciphertext; the key is already on the host.
(c) the call's share of an n_out-step fhe_blind_rotate at the level-0 shape (four 30-bit primes at N = 8192, RGSW w = 16), timed in the same run:
    LOOP_STEPS steps are timed and scaled to n_out steps.
Times are wall-clock microseconds per call around ITERS calls and one device synchronisation.  One JSON line per (shape, batch).
usage: bench_lwe_keyswitch.py [out.jsonl]     (default profiles/bench_lwe_keyswitch.jsonl; appends)"""
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
pkg = importlib.import_module("gpu-homomorphic-encryption_amd")
import lwe_keyswitch_model as km  # noqa: E402

ROUNDS, W, N_OUT, LOOP_STEPS = 5, 8, 512, 64
# (name, N, prime bits, q_out, ciphertexts of the host product)
CONFIGS = [("N=8192 1x30-bit", 8192, 30, 0, 16), ("N=16384 1x40-bit", 16384, 40, 0, 8), ("N=8192 1x60-bit q_out=2^32", 8192, 60, 1 << 32, 2)]
BATCHES = (256, 1)


def wall_us(call, iters):
    pkg.capi.sync()
    t0 = time.perf_counter()
    for _ in range(iters):
        call()
    pkg.capi.sync()
    return (time.perf_counter() - t0) * 1e6 / iters


def medians(cands, iters):
    seen = {k: [] for k in cands}
    for call in cands.values():
        call()
    for _ in range(ROUNDS):
        for k, call in cands.items():
            seen[k].append(wall_us(call, iters))
    return {k: statistics.median(v) for k, v in seen.items()}


def secret(eng, n, moduli, rng):
    s = rng.integers(-1, 2, n)
    cont = np.zeros((len(moduli), n, 4), dtype=np.uint64)
    for l, q in enumerate(moduli):
        cont[l, :, 0] = np.where(s < 0, q - 1, s).astype(np.uint64)
    ds = pkg.DeviceBuffer.from_numpy(cont)
    return ds, eng.import_secret_key(ds)


def loop_us(n, batch, rng):
    """LOOP_STEPS steps of fhe_blind_rotate at the level-0 shape, scaled to N_OUT steps"""
    moduli = pkg.find_ntt_primes(30, n, 4)
    eng = pkg.RnsNttEngine(n, moduli)
    ds, sk = secret(eng, n, moduli, rng)
    r0, r1 = eng.generate_rgsw_keys(sk, 16, [int(v) for v in rng.integers(0, 2, LOOP_STEPS)], 1, 3.2, (3, 4))
    S = len(moduli) * n * 32
    acc = [pkg.DeviceBuffer(batch * S) for _ in range(4)]
    for a in acc:
        a.zero()
    d_sh = pkg.DeviceBuffer.from_numpy(rng.integers(0, 2 * n, (LOOP_STEPS, batch)).astype(np.uint32))
    eng.reserve(batch)
    call = lambda: eng.blind_rotate(r0, r1, acc[0], acc[1], d_sh, acc[2], acc[3], batch)
    call()
    return statistics.median(wall_us(call, 2) for _ in range(3)) * N_OUT / LOOP_STEPS


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_lwe_keyswitch.jsonl")
    rng = np.random.default_rng(1)
    loop = {}
    for name, n, bits, q_out, host_batch in CONFIGS:
        q = pkg.find_ntt_primes(bits, n, 1)[0]
        eng = pkg.RnsNttEngine(n, [q])
        ds, sk = secret(eng, n, [q], rng)
        z = [int(v) for v in rng.integers(0, 2, N_OUT)]
        ksk = eng.generate_lwe_ksk(sk, W, z, 1, 3.2, (7, 8))
        K = eng.lwe_ksk_num_digits(W)
        R = n * K
        d_rows = pkg.DeviceBuffer(R * (N_OUT + 1) * 8)
        eng.export_lwe_ksk(ksk, d_rows)
        rows = d_rows.download((R, N_OUT + 1))
        keys = {"auto": ksk}
        if km.u64_form(q, W, R):
            os.environ["FHE_HIP_LWE_KSK_WIDE"] = "1"
            keys["wide"] = eng.import_lwe_ksk(W, N_OUT, d_rows)
            del os.environ["FHE_HIP_LWE_KSK_WIDE"]
        d_rows.free()
        for batch in BATCHES:
            lwe = rng.integers(0, q, (batch, n + 1), dtype=np.uint64)
            d_in, d_out = pkg.DeviceBuffer.from_numpy(lwe), pkg.DeviceBuffer(batch * (N_OUT + 1) * 8)
            hb = min(batch, host_batch)
            # the host path, once, on hb ciphertexts; and the equality checks
            pkg.capi.sync()
            t0 = time.perf_counter()
            down = d_in.download((batch, n + 1))[:hb]
            host = km.keyswitch_np(q, W, rows, down, q_out)
            d_up = pkg.DeviceBuffer.from_numpy(host)
            pkg.capi.sync()
            host_us = (time.perf_counter() - t0) * 1e6
            outs = {}
            for form, k in keys.items():
                eng.lwe_keyswitch(k, d_out, d_in, q_out, batch)
                outs[form] = d_out.download((batch, N_OUT + 1))
                assert np.array_equal(outs[form][:hb], host), (name, batch, form)
            assert all(np.array_equal(o, outs["auto"]) for o in outs.values())
            cands = {form: (lambda k=k: eng.lwe_keyswitch(k, d_out, d_in, q_out, batch)) for form, k in keys.items()}
            us = medians(cands, 20 if batch == 1 else 5)
            if bits == 30 and batch not in loop:
                loop[batch] = loop_us(n, batch, rng)
            macs = batch * R * (N_OUT + 1)
            line = {"bench": "lwe_keyswitch", "shape": name, "n": n, "q_bits": q.bit_length(), "w": W, "K": K, "rows": R, "n_out": N_OUT, "batch": batch,
                    "q_out": q_out, "form": "u64" if km.u64_form(q, W, R) else "wide", "key_bytes": ksk.nbytes(), "us_per_call": round(us["auto"], 1),
                    "mac_per_s": round(macs / (us["auto"] * 1e-6), 1), "key_bytes_per_s_if_read_once_per_batch_tile": round(ksk.nbytes() * -(-batch // 16) / (us["auto"] * 1e-6), 1),
                    "host_batch": hb, "host_us_per_ct": round(host_us / hb, 1), "device_us_per_ct": round(us["auto"] / batch, 2),
                    "host_over_device_per_ct": round((host_us / hb) / (us["auto"] / batch), 1)}
            if "wide" in us:
                line["us_per_call_wide_form"] = round(us["wide"], 1)
            if bits == 30:
                line["loop_us_n_out_steps_level0_4x30bit"] = round(loop[batch], 1)
                line["share_of_loop"] = round(us["auto"] / loop[batch], 5)
            print(json.dumps(line), flush=True)
            with open(out_path, "a") as f:
                f.write(json.dumps(line) + "\n")
            for d in (d_in, d_out, d_up):
                d.free()


if __name__ == "__main__":
    main()
