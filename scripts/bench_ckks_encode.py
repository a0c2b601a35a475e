#!/usr/bin/env python3
"""The CKKS encoder as ONE fhe_ckks_encode / fhe_ckks_decode_poly / fhe_ckks_decode against two comparators, at the same shape, in the same
process, interleaved in time: the calls alternate inside every repetition, the median of REPS repetitions of each counts.
(a) fhe_slots_encode / fhe_slots_decode_poly / fhe_slots_decode of the batch encoder (t = 65537) on the same engine: they write and read the
    same container bytes with an exact transform instead of the FP64 one, so they are the write-bound yardstick.
(b) The host path the encoder replaces: the same formula in numpy float64 (the transform of tests/ckks_model.py), rounding, reduction modulo
    every prime into [L][n] containers, and the upload; decoding: the download of limb 0, centring and the numpy transform.  Wall time per
    plaintext, measured on HOST_PLAINTEXTS plaintexts.
One JSON line per shape and direction: median microseconds per call, the ratios, the bytes the call has to move (encode 8 n + L 32 n per
plaintext; decode_poly 32 n + 8 n as the kernel reads whole 32-byte sectors of limb 0's containers; decode 8 n + 8 n), the rate on those bytes and
its fraction of the HBM roof, and the FP64 work of the transform (10 flops per radix-2 butterfly, n/4 log2(n/2) of them, plus the twist) as a
fraction of the vector FP64 roof, so that the bound the kernel sits at can be read off.
usage: bench_ckks_encode.py [out.jsonl]     (appends, so that a second run lands in the same file)"""
import importlib
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
pkg = importlib.import_module("gpu-homomorphic-encryption_amd")
import ckks_model as cm  # noqa: E402

REPS = 7
T = 65537
SCALE = float(2 ** 24)                                   # slots in the unit square: |c| < q_0 / 2 on 30-bit primes (decode_poly is valid)
HBM_BYTES_PER_S = 8.0e12                                 # MI355X peak
FP64_FLOPS_PER_S = 78.6e12                               # MI355X vector FP64 peak (half the FP32 vector rate)
HOST_PLAINTEXTS = 4
SHAPES = [("N=8192 4x30-bit", 8192, 30, 4, 1024), ("N=16384 6x30-bit", 16384, 30, 6, 1024),
          ("N=8192 4x30-bit, batch 1", 8192, 30, 4, 1), ("N=16384 6x30-bit, batch 1", 16384, 30, 6, 1)]


def once(eng, call, iters):
    t = pkg.Timer(); t.start(eng)
    for _ in range(iters):
        call()
    t.stop(eng)
    return t.elapsed_ms() * 1e3 / iters                  # microseconds per call


def interleaved(eng, calls, iters):
    """{name: median microseconds per call}; inside a repetition the calls alternate"""
    for c in calls.values():
        c()                                              # warm up: code objects, caches
    pkg.capi.sync()
    times = {k: [] for k in calls}
    for _ in range(REPS):
        for k, c in calls.items():
            times[k].append(once(eng, c, iters))
    return {k: statistics.median(v) for k, v in times.items()}


def host_encode(z, n, moduli):
    m = cm.encode(z, n, np.complex128)
    c = np.rint(m * SCALE).astype(np.int64)
    out = np.zeros((len(moduli), n, 4), dtype=np.uint64)
    for l, q in enumerate(moduli):
        out[l, :, 0] = np.mod(c, q).astype(np.uint64)
    return out


def host_decode(limb0, q0):
    w = limb0[:, 0].astype(np.int64)
    return cm.decode(np.where(w > q0 // 2, w - q0, w).astype(np.float64) / SCALE, np.complex128)


def main():
    out = open(sys.argv[1], "a") if len(sys.argv) > 1 else None
    if pkg.device_count() < 1:
        raise SystemExit("bench_ckks_encode.py: no HIP device visible (there is nothing to measure without one)")
    rng = np.random.default_rng(1)
    for name, n, bits, L, batch in SHAPES:
        moduli = pkg.find_ntt_primes(bits, n, L)
        eng = pkg.RnsNttEngine(n, moduli)
        ck, be = pkg.capi.CkksEncoder(eng), pkg.capi.BatchEncoder(eng, T, pkg.capi.SLOTS_ROWS)
        z = rng.random((batch, n // 2)) + 1j * rng.random((batch, n // 2))
        d_z = pkg.DeviceBuffer.from_numpy(np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1)))
        d_vals = pkg.DeviceBuffer.from_numpy(rng.integers(0, T, (batch, n), dtype=np.uint64))
        d_pt, d_pt2 = pkg.DeviceBuffer(batch * L * n * 32), pkg.DeviceBuffer(batch * L * n * 32)
        d_back, d_back2, d_words = pkg.DeviceBuffer(batch * n * 8), pkg.DeviceBuffer(batch * n * 8), pkg.DeviceBuffer(batch * n * 8)
        ck.encode(d_pt, d_z, SCALE, batch); be.encode(d_pt2, d_vals, batch)
        be.decode_poly(d_words, d_pt2, batch)            # some words below t for the word decoders
        iters = 20 if batch > 1 else 200
        med = interleaved(eng, {
            "ckks_encode": lambda: ck.encode(d_pt, d_z, SCALE, batch), "slots_encode": lambda: be.encode(d_pt2, d_vals, batch),
            "ckks_decode_poly": lambda: ck.decode_poly(d_back, d_pt, SCALE, batch), "slots_decode_poly": lambda: be.decode_poly(d_back2, d_pt2, batch),
            "ckks_decode": lambda: ck.decode(d_back, d_words, T, SCALE, batch), "slots_decode": lambda: be.decode(d_back2, d_words, batch)}, iters)
        # (b) the host path, per plaintext
        k = min(batch, HOST_PLAINTEXTS)
        host = pkg.DeviceBuffer(L * n * 32)
        t0 = time.perf_counter()
        for b in range(k):
            host.upload(host_encode(z[b], n, moduli))
        pkg.capi.sync()
        host_enc_us = (time.perf_counter() - t0) * 1e6 / k
        t0 = time.perf_counter()
        for b in range(k):
            host_decode(host.download((L, n, 4))[0], moduli[0])
        host_dec_us = (time.perf_counter() - t0) * 1e6 / k
        flops = batch * (10 * (n // 4) * math.log2(n // 2) + 8 * (n // 2))
        rows = [("encode", "ckks_encode", "slots_encode", batch * (8 * n + L * 32 * n), host_enc_us),
                ("decode_poly", "ckks_decode_poly", "slots_decode_poly", batch * (32 * n + 8 * n), host_dec_us),
                ("decode", "ckks_decode", "slots_decode", batch * (8 * n + 8 * n), None)]
        for direction, mine, theirs, nbytes, host_us in rows:
            us = med[mine]
            hbm_frac, fp64_frac = nbytes / (us * 1e-6) / HBM_BYTES_PER_S, flops / (us * 1e-6) / FP64_FLOPS_PER_S
            rec = {"bench": "ckks_encode", "shape": name, "direction": direction, "n": n, "limbs": L, "batch": batch, "reps": REPS, "iters": iters,
                   "ckks_us": round(us, 2), "batch_encoder_us": round(med[theirs], 2), "ckks_over_batch_encoder": round(us / med[theirs], 3),
                   "per_plaintext_us": round(us / batch, 3), "bytes": nbytes, "GBps": round(nbytes / (us * 1e-6) / 1e9, 1), "hbm_frac": round(hbm_frac, 3),
                   "fp64_flops": int(flops), "fp64_frac": round(fp64_frac, 4),
                   "nearer_bound": "hbm" if hbm_frac >= fp64_frac else "fp64"}
            if host_us is not None:
                rec["host_numpy_us_per_plaintext"] = round(host_us, 1)
                rec["host_over_ckks_per_plaintext"] = round(host_us / (us / batch), 1)
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n"); out.flush()


if __name__ == "__main__":
    main()
