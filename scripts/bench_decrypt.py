#!/usr/bin/env python3
"""Secret-key decryption as ONE fhe_ct_decrypt against the device part of the call list FHEContext::decrypt_values runs, at the same shape, in
the same process, interleaved in time: the two alternate, the best of REPS repetitions of each counts.  The chain, in the mirror's order and
batched: two device-to-device copies (c0 into the accumulator, s into the power buffer -- replicated per ciphertext, the mirror has no
broadcast), fhe_rns_ntt_multiply, fhe_rns_poly_add, fhe_rns_from_rns.  It leaves out what the mirror then does on the host (the download of
n 256-bit integers per ciphertext, centring, % t and the correction, one coefficient at a time), so the composed time is a lower bound.  One
JSON line per shape: microseconds per call both ways, decryptions per second, the ratio, and the fraction of the HBM roof on the bytes the
fused call has to move: 2 S in, the compact round trip 2 L n sizeof(residue), 8 n out, per ciphertext.
usage: bench_decrypt.py [out.jsonl]     (appends, so that a second run lands in the same file)"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
pkg = importlib.import_module("gpu-homomorphic-encryption_amd")
from workload import rns_poly  # noqa: E402

REPS = 5
T = 65537
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
    d2d = pkg.lib().fhe_hip_memcpy_d2d
    for name, n, bits, L, batch in SHAPES:
        moduli = pkg.find_ntt_primes(bits, n, L)
        eng = pkg.RnsNttEngine(n, moduli)
        S = L * n * 32
        s = pkg.DeviceBuffer.from_numpy(rns_poly(31, moduli, n, 1)[0])
        sk = eng.import_secret_key(s)
        eng.reserve(batch); eng.decrypt_reserve(T, 2, batch)
        c = [pkg.DeviceBuffer(batch * S) for _ in range(2)]
        for i in range(2):
            eng.sample_uniform(c[i], 33 + i, batch)      # drawn on the device: 3 GB per buffer at the largest shape
        s_rep, acc, sp, tmp = (pkg.DeviceBuffer(batch * S) for _ in range(4))
        for b in range(batch):
            assert d2d(s_rep.ptr + b * S, s.ptr, S) == 0
        d_int = pkg.DeviceBuffer(batch * n * 32)
        dm, dn = pkg.DeviceBuffer(batch * n * 8), pkg.DeviceBuffer(batch * 4)
        iters = 2 if batch > 1 else 20

        def composed():
            assert d2d(acc.ptr, c[0].ptr, batch * S) == 0
            assert d2d(sp.ptr, s_rep.ptr, batch * S) == 0
            eng.multiply(tmp, c[1], sp, batch)
            eng.poly_add(acc, acc, tmp, batch)
            eng.from_rns(d_int, acc, batch)

        def fused():
            eng.decrypt(sk, T, 1, dm, dn, c, batch)

        composed(); fused(); pkg.capi.sync()             # warm-up: code objects, workspaces, tables, clocks
        best = {}
        for _ in range(REPS):                            # interleaved: every repetition runs both once
            for kind, fn in (("composed", composed), ("fused", fused)):
                us = once(eng, fn, iters)
                best[kind] = min(best.get(kind, us), us)
        eb = 4 if eng.width_class == 1 else 8                      # FHE_WIDTH_32: 4-byte residues
        moved = batch * (2 * S + 2 * L * n * eb + 8 * n)
        rec = {"shape": name, "n": n, "limbs": L, "bits": bits, "batch": batch, "t": T, "components": 2, "width_class": eng.width_class, "reps": REPS,
               "composed_us": best["composed"], "fused_us": best["fused"], "composed_over_fused": best["composed"] / best["fused"],
               "fused_decryptions_per_s": batch / (best["fused"] * 1e-6), "composed_decryptions_per_s": batch / (best["composed"] * 1e-6),
               "fused_bytes_moved": moved, "fused_hbm_fraction": moved / (best["fused"] * 1e-6) / HBM_BYTES_PER_S}
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n"); out.flush()
        del c, s_rep, acc, sp, tmp, d_int, dm, dn, sk, s, eng
    if out:
        out.close()


if __name__ == "__main__":
    main()
