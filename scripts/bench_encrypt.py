#!/usr/bin/env python3
"""Public-key encryption as ONE fhe_ct_encrypt against the composition of existing entry points at the same shape, in the same process,
interleaved in time: the two alternate, the best of REPS repetitions of each counts.  The composition is the call list of
FHEContext::encrypt with device sampling, batched: fhe_rns_sample_ternary, two fhe_rns_ntt_multiply_bcast (pk0, pk1), and per error
polynomial fhe_rns_sample_gaussian, the scale by t (fhe_u256_mont_mul_scalar) and fhe_rns_poly_add, plus the addition of m.  The mirror
scales one limb of one ciphertext per launch; batched, the scale runs here as ONE launch over the whole buffer with limb 0's constants (same
bytes, fewer launches: the composed time is a lower bound, its values are not used).  One JSON line per shape: microseconds per call both
ways, encryptions per second, the ratio, and the fraction of the HBM roof on the 3 S bytes a call has to move (m in, c0 and c1 out).
usage: bench_encrypt.py [out.jsonl]     (appends, so that a second run lands in the same file)"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
pkg = importlib.import_module("gpu-homomorphic-encryption_amd")
from workload import rns_poly  # noqa: E402

REPS = 5
T, SIGMA = 65537, 3.2
HBM_BYTES_PER_S = 8.0e12                                 # MI355X peak
SHAPES = [("N=8192 4x30-bit", 8192, 30, 4, 1024), ("N=16384 6x30-bit", 16384, 30, 6, 1024), ("N=16384 6x40-bit", 16384, 40, 6, 1024),
          ("N=8192 4x30-bit, batch 1", 8192, 30, 4, 1), ("N=16384 6x30-bit, batch 1", 16384, 30, 6, 1), ("N=16384 6x40-bit, batch 1", 16384, 40, 6, 1)]


def once(eng, call, iters):
    t = pkg.Timer(); t.start(eng)
    for _ in range(iters):
        call()
    t.stop(eng)
    return t.elapsed_ms() * 1e3 / iters                  # microseconds per call


def main():
    out = open(sys.argv[1], "a") if len(sys.argv) > 1 else None
    for name, n, bits, L, batch in SHAPES:
        moduli = pkg.find_ntt_primes(bits, n, L)
        eng = pkg.RnsNttEngine(n, moduli)
        pk0, pk1 = (pkg.DeviceBuffer.from_numpy(rns_poly(31 + i, moduli, n, 1)[0]) for i in range(2))
        pk = eng.import_public_key(pk0, pk1)
        eng.reserve(batch); eng.encrypt_reserve(SIGMA, batch)
        m = pkg.DeviceBuffer(batch * L * n * 32); eng.sample_uniform(m, 33, batch)      # drawn on the device: 3 GB at the largest shape
        o = [pkg.DeviceBuffer(m.nbytes) for _ in range(2)]; u = pkg.DeviceBuffer(m.nbytes); e = pkg.DeviceBuffer(m.nbytes)
        q0 = moduli[0]; scalar = (T % q0) * pow(2, 256, q0) % q0; inv0 = pkg.capi.montgomery_inverse(q0) & ((1 << 64) - 1)
        count = batch * L * n
        iters = 2 if batch > 1 else 20

        def composed():
            eng.sample_ternary(u, 0.5, 11, batch)
            eng.multiply_bcast(o[0], u, pk0, batch)
            eng.multiply_bcast(o[1], u, pk1, batch)
            for i, seed in ((0, 12), (1, 13)):
                eng.sample_gaussian(e, SIGMA, seed, batch)
                pkg.capi.u256_mont_mul_scalar(e, e, scalar, q0, inv0, count)
                eng.poly_add(o[i], o[i], e, batch)
            eng.poly_add(o[0], o[0], m, batch)

        def fused():
            eng.encrypt(pk, T, SIGMA, (11, 12, 13), o[0], o[1], m, batch)

        composed(); fused(); pkg.capi.sync()             # warm-up: code objects, workspaces, clocks
        best = {}
        for _ in range(REPS):                            # interleaved: every repetition runs both once
            for kind, fn in (("composed", composed), ("fused", fused)):
                us = once(eng, fn, iters)
                best[kind] = min(best.get(kind, us), us)
        moved = 3 * m.nbytes
        rec = {"shape": name, "n": n, "limbs": L, "bits": bits, "batch": batch, "sigma": SIGMA, "width_class": eng.width_class, "reps": REPS,
               "composed_us": best["composed"], "fused_us": best["fused"], "composed_over_fused": best["composed"] / best["fused"],
               "fused_encryptions_per_s": batch / (best["fused"] * 1e-6), "composed_encryptions_per_s": batch / (best["composed"] * 1e-6),
               "fused_hbm_fraction_of_3S": moved / (best["fused"] * 1e-6) / HBM_BYTES_PER_S}
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n"); out.flush()
        del m, o, u, e, pk, pk0, pk1, eng
    if out:
        out.close()


if __name__ == "__main__":
    main()
