#!/usr/bin/env python3
"""Slot rotations (fhe_ct_apply_galois) against stand-alone relinearisation (fhe_ct_relinearize) at the same shape, in the same process.

A rotation is an automorphism of both components followed by a key switch; on the fused path that is the prologue (sigma(c0), sigma(c1)
and a zero polynomial as compact polynomials) plus the compact-operand key switch of fhe_ct_multiply_relin.  Algorithmic bytes per call
(S = one ciphertext component, L * n * 32 bytes per ciphertext): rotation 4 S (c0, c1 read, two components written; key rows amortised
over the batch), relinearisation 5 S (c0, c1 read and written, c2 read).  The compact round trip of the rotation (3 compact polynomials
written, read back by the key switch) comes on top and is not counted.  HBM fraction against the 8.0 TB/s peak.
usage: bench_rotate.py [out.jsonl]      (one JSON line per shape on stdout)
       bench_rotate.py --trace          (13 rotations at the configs[2] shape and nothing else: the driver of the kernel trace in profiles/)"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
pkg = importlib.import_module("gpu-homomorphic-encryption_amd")
from workload import rns_poly  # noqa: E402

HBM_PEAK_GBS = 8000.0
SHAPES = [("configs[2] N=8192 4x30-bit w=16", 8192, 30, 4, 16, 1024),
          ("configs[3] N=16384 6x30-bit w=16", 16384, 30, 6, 16, 128),
          ("configs[3] N=16384 6x40-bit w=20", 16384, 40, 6, 20, 128),
          ("configs[2] N=8192 4x30-bit w=16, batch 1", 8192, 30, 4, 16, 1),
          ("configs[3] N=16384 6x30-bit w=16, batch 1", 16384, 30, 6, 16, 1)]


def timed(eng, call, iters):
    for _ in range(3):
        call()
    pkg.capi.sync()
    best = None
    for _ in range(3):                                   # best of three timed runs of `iters` calls
        t = pkg.Timer(); t.start(eng)
        for _ in range(iters):
            call()
        t.stop(eng)
        ms = t.elapsed_ms() / iters
        best = ms if best is None else min(best, ms)
    return best


def setup(n, bits, L, w, batch):
    moduli = pkg.find_ntt_primes(bits, n, L)
    eng = pkg.RnsNttEngine(n, moduli)
    K = eng.relin_num_digits(w)
    keys = [pkg.DeviceBuffer.from_numpy(rns_poly(500 + i, moduli, n, 1)[0]) for i in range(L * K)]
    gk = eng.import_relin_keys(w, keys, keys)
    eng.reserve(batch)
    c = [pkg.DeviceBuffer.from_numpy(rns_poly(90 + i, moduli, n, batch)) for i in range(3)]
    return eng, gk, keys, c


def trace():
    eng, gk, keys, c = setup(8192, 30, 4, 16, 1024)
    o0, o1 = pkg.DeviceBuffer(c[0].nbytes), pkg.DeviceBuffer(c[0].nbytes)
    g = pkg.galois_element(8192, 1)
    for _ in range(13):
        eng.apply_galois(gk, g, o0, o1, c[0], c[1], 1024)
    pkg.capi.sync()
    print("13 rotations done")


def main():
    if sys.argv[1:] == ["--trace"]:
        return trace()
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    for name, n, bits, L, w, batch in SHAPES:
        eng, gk, keys, c = setup(n, bits, L, w, batch)
        o0, o1 = pkg.DeviceBuffer(c[0].nbytes), pkg.DeviceBuffer(c[0].nbytes)
        g = pkg.galois_element(n, 1)
        S = L * n * 32 * batch
        iters = 20 if batch > 1 else 200
        rot_ms = timed(eng, lambda: eng.apply_galois(gk, g, o0, o1, c[0], c[1], batch), iters)
        rel_ms = timed(eng, lambda: eng.relinearize(gk, c[0], c[1], c[2], batch), iters)
        rec = {"shape": name, "n": n, "limbs": L, "bits": bits, "decomp_bits": w, "batch": batch, "width_class": eng.width_class,
               "rotations_per_s": batch / (rot_ms * 1e-3), "relinearizations_per_s": batch / (rel_ms * 1e-3),
               "rotation_us_per_call": rot_ms * 1e3, "relinearize_us_per_call": rel_ms * 1e3,
               "rotation_over_relinearize": rel_ms / rot_ms,
               "rotation_hbm_frac": 4 * S / (rot_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
               "relinearize_hbm_frac": 5 * S / (rel_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
               "bytes": {"rotation": "4 S", "relinearize": "5 S", "S_bytes": S}}
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
        del c, o0, o1, gk, keys, eng
    if out:
        out.close()


if __name__ == "__main__":
    main()
