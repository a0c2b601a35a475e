#!/usr/bin/env python3
"""Key-switching key generation as ONE fhe_keyswitch_keys_generate against the device call list that makes the same handles without it, at the
same shape, in the same process, interleaved in time: the two alternate, the best of REPS repetitions of each counts.  The call list, per key
set: fhe_rns_sample_uniform + fhe_rns_sample_gaussian (L K polynomials each), fhe_rns_ntt_multiply_bcast by s, fhe_rns_poly_sub,
fhe_rns_poly_add of a prepared gadget polynomial, fhe_relin_keys_create.  It leaves out the scaling of e by t and the making of the gadget
polynomial (the engine has no call for either; the mirror does both on the host), so the composed time is a lower bound.  Both sides allocate
and free their key sets inside the timed region.  One JSON line per shape: microseconds per call both ways and the ratio.
usage: bench_keygen.py [out.jsonl]     (appends, so that a second run lands in the same file)"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
pkg = importlib.import_module("gpu-homomorphic-encryption_amd")
from workload import rns_poly  # noqa: E402

REPS = 5
T, SIGMA, W = 65537, 3.2, 16
SHAPES = [("N=8192 4x30-bit", 8192, 30, 4), ("N=16384 6x30-bit", 16384, 30, 6), ("N=16384 6x40-bit", 16384, 40, 6)]


def default_elements(eng_n):
    """The set of FHEContext::galoiskey_gen(gal_keys, sk): row steps +-2^i and the column element, 2 log2(n / 2) + 1 elements."""
    elts, s = [], 1
    while s < eng_n // 2:
        elts += [pkg.capi.galois_element(eng_n, s), pkg.capi.galois_element(eng_n, -s)]
        s <<= 1
    return elts + [2 * eng_n - 1]


def once(eng, call, iters):
    t = pkg.Timer(); t.start(eng)
    for _ in range(iters):
        call()
    t.stop(eng)
    return t.elapsed_ms() * 1e3 / iters                  # microseconds per call


def main():
    out = open(sys.argv[1], "a") if len(sys.argv) > 1 else None
    for name, n, bits, L in SHAPES:
        moduli = pkg.find_ntt_primes(bits, n, L)
        eng = pkg.RnsNttEngine(n, moduli)
        S = L * n * 32
        LK = L * eng.relin_num_digits(W)
        s = pkg.DeviceBuffer.from_numpy(rns_poly(31, moduli, n, 1)[0])
        sk = eng.import_secret_key(s)
        a, e, prod, gadget = (pkg.DeviceBuffer(LK * S) for _ in range(4))
        eng.sample_uniform(gadget, 5, LK)
        rows = lambda buf: [buf.ptr + r * S for r in range(LK)]   # raw device addresses of the L K rows
        for kind_name, elts in (("relinearisation key", [0]), ("default Galois set", default_elements(n))):
            def composed():
                for i, _g in enumerate(elts):
                    eng.sample_uniform(a, 100 + i, LK)
                    eng.sample_gaussian(e, SIGMA, 200 + i, LK)
                    eng.multiply_bcast(prod, a, s, LK)
                    eng.poly_sub(e, e, prod, LK)
                    eng.poly_add(e, e, gadget, LK)
                    eng.import_relin_keys(W, rows(e), rows(a)).close()

            def fused():
                for rk in eng.generate_keyswitch_keys(sk, W, elts, T, SIGMA, (11, 22)):
                    rk.close()

            composed(); fused(); pkg.capi.sync()         # warm-up: code objects, workspaces, tables, clocks
            best = {}
            for _ in range(REPS):                        # interleaved: every repetition runs both once
                for kind, fn in (("composed", composed), ("fused", fused)):
                    us = once(eng, fn, 2)
                    best[kind] = min(best.get(kind, us), us)
            rec = {"shape": name, "keys": kind_name, "n": n, "limbs": L, "bits": bits, "decomp_bits": W, "num_sets": len(elts), "rows_per_set": LK,
                   "workgroups": len(elts) * LK * L, "width_class": eng.width_class, "reps": REPS, "composed_us": best["composed"], "fused_us": best["fused"],
                   "composed_over_fused": best["composed"] / best["fused"], "fused_key_sets_per_s": len(elts) / (best["fused"] * 1e-6)}
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n"); out.flush()
        del a, e, prod, gadget, sk, s, eng
    if out:
        out.close()


if __name__ == "__main__":
    main()
