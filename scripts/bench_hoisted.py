#!/usr/bin/env python3
"""Hoisted rotations (one fhe_ct_hoist + G fhe_ct_apply_galois_hoisted) against G calls of fhe_ct_apply_galois at the same shape, in the
same process, interleaved in time: for every G the two sequences alternate, the best of REPS repetitions of each counts.
fhe_ct_apply_galois is the yardstick (unchanged code).  One JSON line per shape: microseconds per rotation both ways, the hoist's own time,
one hoisted rotation's time (first element only), the ratio per G and the break-even: the first measured G at which hoist + G applies take
no longer than G single calls (from the per-G rows, like for like: the same elements both ways).
usage: bench_hoisted.py [out.jsonl]     (appends, so that a second run lands in the same file)"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
pkg = importlib.import_module("gpu-homomorphic-encryption_amd")
from workload import rns_poly  # noqa: E402

REPS = 6
GS = (1, 2, 4, 8, 16)
SHAPES = [("configs[2] N=8192 4x30-bit w=16", 8192, 30, 4, 16, 1024),
          ("configs[3] N=16384 6x30-bit w=16", 16384, 30, 6, 16, 128),
          ("configs[3] N=16384 6x40-bit w=20", 16384, 40, 6, 20, 128),
          ("configs[2] N=8192 4x30-bit w=16, batch 1", 8192, 30, 4, 16, 1),
          ("configs[3] N=16384 6x30-bit w=16, batch 1", 16384, 30, 6, 16, 1)]


def once(eng, call, iters):
    t = pkg.Timer(); t.start(eng)
    for _ in range(iters):
        call()
    t.stop(eng)
    return t.elapsed_ms() * 1e3 / iters                  # microseconds per call


def main():
    out = open(sys.argv[1], "a") if len(sys.argv) > 1 else None
    for name, n, bits, L, w, batch in SHAPES:
        moduli = pkg.find_ntt_primes(bits, n, L)
        eng = pkg.RnsNttEngine(n, moduli)
        K = eng.relin_num_digits(w)
        keys = [pkg.DeviceBuffer.from_numpy(rns_poly(500 + i, moduli, n, 1)[0]) for i in range(L * K)]
        gk = eng.import_relin_keys(w, keys, keys)
        eng.reserve(batch); eng.reserve_hoist(w, batch)
        c = [pkg.DeviceBuffer.from_numpy(rns_poly(90 + i, moduli, n, batch)) for i in range(2)]
        o0, o1 = pkg.DeviceBuffer(c[0].nbytes), pkg.DeviceBuffer(c[0].nbytes)
        elts = [pkg.galois_element(n, r + 1) for r in range(max(GS))]
        iters = 3 if batch > 1 else 30

        def single(G):
            for g in elts[:G]:
                eng.apply_galois(gk, g, o0, o1, c[0], c[1], batch)

        def hoisted(G):
            eng.hoist(w, c[1], batch)
            for g in elts[:G]:
                eng.apply_galois_hoisted(gk, g, o0, o1, c[0], batch)

        def hoist_only():
            eng.hoist(w, c[1], batch)

        def apply_only():
            eng.apply_galois_hoisted(gk, elts[0], o0, o1, c[0], batch)

        single(2); hoisted(2); pkg.capi.sync()           # warm-up: code objects, workspaces, clocks
        best = {}
        for _ in range(REPS):                            # interleaved: every repetition runs every variant once
            for G in GS:
                for kind, fn in (("single", single), ("hoisted", hoisted)):
                    us = once(eng, lambda: fn(G), iters)
                    best[(kind, G)] = min(best.get((kind, G), us), us)
            for kind, fn in (("hoist", hoist_only), ("apply", apply_only)):
                us = once(eng, fn, iters * 4)
                best[kind] = min(best.get(kind, us), us)
        ratio = {G: best[("single", G)] / best[("hoisted", G)] for G in GS}
        rec = {"shape": name, "n": n, "limbs": L, "bits": bits, "decomp_bits": w, "batch": batch, "width_class": eng.width_class,
               "hoist_bytes": eng.hoist_bytes(), "reps": REPS,
               "hoist_us": best["hoist"], "apply_first_element_us": best["apply"],
               "break_even_G": next((G for G in GS if ratio[G] >= 1.0), None),
               "per_G": {str(G): {"single_us_per_rotation": best[("single", G)] / G, "hoisted_us_per_rotation": best[("hoisted", G)] / G,
                                  "single_over_hoisted": ratio[G]} for G in GS}}
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n"); out.flush()
        del c, o0, o1, gk, keys, eng
    if out:
        out.close()


if __name__ == "__main__":
    main()
