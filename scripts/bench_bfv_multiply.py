#!/usr/bin/env python3
"""BFV multiplication per stage and as one call, with its comparators at the same shape, in the same process, interleaved in time: the calls
alternate inside every repetition, the median of REPS repetitions of each counts.
  stages       fhe_bfv_lift (one polynomial), fhe_ct_multiply on the extended engine Q u P, fhe_bfv_scale_round (three components)
  whole call   fhe_bfv_multiply
  comparators  fhe_ct_multiply on hq: the cost of the modular product, which a BFV product cannot use;
               fhe_rns_fast_base_convert Q -> P and fhe_rns_rescale_drop_last on Q u P over the same polynomials: the streaming rate the two new
               kernels are to be read against (they move the same kind of bytes: containers in, containers out, one lane per coefficient).
               The rescale is THREE launches (one per product component) against the one launch of scale-and-round: at batch 1, where a
               launch is most of the time, that favours scale-and-round; at batch 256 it does not matter.
One JSON line per shape: median microseconds per call, the bytes each streaming kernel reads plus writes (whole 32-byte containers: a load of a
residue fetches its sector), TB/s on those bytes, and each new kernel's rate over the slower of the two reference kernels.
usage: bench_bfv_multiply.py [out.jsonl]     (appends; default profiles/bench_bfv_multiply.jsonl)"""
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("gpu-homomorphic-encryption_amd")

REPS = 7
T = 65537
SHAPES = [("N=8192 4+6 x 30-bit", 8192, 30, 4, 6), ("N=16384 6+8 x 40-bit", 16384, 40, 6, 8)]
BATCHES = [1, 256]


def once(eng, call, iters):
    t = pkg.Timer(); t.start(eng)
    for _ in range(iters):
        call()
    t.stop(eng)
    return t.elapsed_ms() * 1e3 / iters                  # microseconds per call


def interleaved(eng, calls, iters):
    for c in calls.values():
        c()                                              # warm up: code objects, caches, workspaces
    pkg.capi.sync()
    times = {k: [] for k in calls}
    for _ in range(REPS):
        for k, c in calls.items():
            times[k].append(once(eng, c, iters))
    return {k: statistics.median(v) for k, v in times.items()}


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_bfv_multiply.jsonl")
    if pkg.device_count() < 1:
        raise SystemExit("bench_bfv_multiply.py: no HIP device visible (there is nothing to measure without one)")
    out = open(path, "a")
    for name, n, bits, L, Lp in SHAPES:
        primes = pkg.find_ntt_primes(bits, n, L + Lp)
        Q, P = primes[:L], primes[L:]
        eng, eng_p = pkg.RnsNttEngine(n, Q), pkg.RnsNttEngine(n, P)
        m = pkg.capi.BfvMultiplier(eng, T, P)
        qp = m.engine
        for batch in BATCHES:
            m.reserve(batch)
            Sq, Sp, Sqp = batch * L * n * 32, batch * Lp * n * 32, batch * (L + Lp) * n * 32
            ins = [pkg.DeviceBuffer(Sq) for _ in range(4)]
            for i, d in enumerate(ins):
                eng.sample_uniform(d, 100 + i, batch)
            outs = [pkg.DeviceBuffer(Sq) for _ in range(3)]
            lifted = [pkg.DeviceBuffer(Sqp) for _ in range(4)]
            prods = [pkg.DeviceBuffer(Sqp) for _ in range(3)]
            conv, resc = pkg.DeviceBuffer(Sp), pkg.DeviceBuffer(batch * (L + Lp - 1) * n * 32)
            for d, s in zip(lifted, ins):
                m.lift(d, s, batch)
            qp.ct_multiply(*prods, *lifted, batch)
            iters = 200 if batch == 1 else 10
            med = interleaved(eng, {
                "lift": lambda: m.lift(lifted[0], ins[0], batch),
                "base_convert": lambda: eng.fast_base_convert(eng_p, conv, ins[0], batch),
                "scale_round": lambda: m.scale_round(outs, prods, batch),
                "rescale": lambda: [qp.rescale_drop_last(resc, p, batch) for p in prods],
                "ct_multiply_qp": lambda: qp.ct_multiply(*prods, *lifted, batch),
                "ct_multiply_q": lambda: eng.ct_multiply(*outs, *ins, batch),
                "bfv_multiply": lambda: m.multiply(*outs, *ins, batch)}, iters)
            nbytes = {"lift": Sq + Sqp, "base_convert": Sq + Sp, "scale_round": 3 * (Sqp + Sq), "rescale": 3 * (Sqp + Sqp - batch * n * 32)}
            tbps = {k: nbytes[k] / (med[k] * 1e-6) / 1e12 for k in nbytes}
            ref = min(tbps["base_convert"], tbps["rescale"])
            rec = {"bench": "bfv_multiply", "shape": name, "n": n, "bits": bits, "L": L, "L_aux": Lp, "t": T, "batch": batch, "reps": REPS, "iters": iters,
                   "us": {k: round(v, 2) for k, v in med.items()}, "bytes": nbytes, "TBps": {k: round(v, 3) for k, v in tbps.items()},
                   "lift_over_slower_reference": round(tbps["lift"] / ref, 3), "scale_round_over_slower_reference": round(tbps["scale_round"] / ref, 3),
                   "stages_sum_us": round(4 * med["lift"] + med["ct_multiply_qp"] + med["scale_round"], 2),
                   "bfv_over_modular_product": round(med["bfv_multiply"] / med["ct_multiply_q"], 2)}
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n"); out.flush()
        m.close()


if __name__ == "__main__":
    main()
