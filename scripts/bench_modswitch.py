#!/usr/bin/env python3
"""Timing of the BGV modulus switch (fhe_ct_mod_switch_drop_last, two components in one launch) against the yardstick that moves the same bytes:
two calls of fhe_rns_rescale_drop_last on the same buffers.  HIP-event timing on the engine stream (fhe_rns_timer_*); the legs are interleaved in one
process, round after round, and the rescale leg runs twice per round so that its own run-to-run spread is on record next to the ratio.
Algorithmic bytes of either leg: 2 components x (2L - 1) x n x 32 per batch element.
usage: bench_modswitch.py [batch] [rounds] [reps]     writes profiles/r06_bench_modswitch.jsonl (one JSON line per shape)"""
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
pkg = importlib.import_module("gpu-homomorphic-encryption_amd")
from workload import rns_poly  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024          # the batch of scripts/bench_n2.py
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 20
T = 65537
SHAPES = [(8192, 4, 30), (16384, 6, 40), (8192, 2, 60)]      # BASELINE config 2; the FP64 field; the 64-bit integer field
OUT = os.path.join(ROOT, "profiles", "r06_bench_modswitch.jsonl")


def filled(block, batch):
    """[batch][L][n] containers on the device: the random block of min(batch, 16) elements, repeated (the kernels' time does not depend on the values)."""
    per = block.nbytes // block.shape[0]
    d = pkg.DeviceBuffer(batch * per)
    for off in range(0, batch, block.shape[0]):
        part = block[:min(block.shape[0], batch - off)]
        pkg.capi._check(pkg.lib().fhe_hip_memcpy_h2d(d.ptr + off * per, part.ctypes.data, part.nbytes))
    return d


def timed(eng, fn):
    t = pkg.Timer(); t.start(eng)
    for _ in range(REPS):
        fn()
    t.stop(eng); pkg.capi.sync()
    return t.elapsed_ms() / REPS


def run(n, L, bits):
    moduli = pkg.find_ntt_primes(bits, n, L)
    eng = pkg.RnsNttEngine(n, moduli)
    S1 = 32 * n
    d_in = [filled(rns_poly(3 + c, moduli, n, min(B, 16)), B) for c in range(2)]
    d_out = [pkg.DeviceBuffer(B * (L - 1) * S1) for _ in range(2)]
    bytes_moved = 2 * B * (2 * L - 1) * S1

    def switch():
        eng.ct_mod_switch(T, d_out, d_in, B)

    def rescale():
        eng.rescale_drop_last(d_out[0], d_in[0], B); eng.rescale_drop_last(d_out[1], d_in[1], B)

    for fn in (switch, rescale, switch, rescale):             # warm-up: code objects, tables, clocks
        timed(eng, fn)
    ms = {"mod_switch": [], "rescale_a": [], "rescale_b": []}
    for _ in range(ROUNDS):
        ms["rescale_a"].append(timed(eng, rescale))
        ms["mod_switch"].append(timed(eng, switch))
        ms["rescale_b"].append(timed(eng, rescale))
    med = {k: statistics.median(v) for k, v in ms.items()}
    rescale_med = statistics.median(ms["rescale_a"] + ms["rescale_b"])
    gbs = lambda x: bytes_moved / x / 1e6
    assert gbs(min(ms["mod_switch"])) <= 8000.0, "above the 8 TB/s HBM peak: the byte count is wrong"
    rec = {
        "n": n, "L": L, "bits": bits, "batch": B, "t": T, "width_class": eng.width_class, "reps": REPS, "rounds": ROUNDS, "bytes": bytes_moved,
        "mod_switch_ms": med["mod_switch"], "rescale_x2_ms": rescale_med,
        "mod_switch_gbs": gbs(med["mod_switch"]), "rescale_x2_gbs": gbs(rescale_med),
        "ratio_mod_switch_over_rescale": med["mod_switch"] / rescale_med,
        "rescale_spread": max(ms["rescale_a"] + ms["rescale_b"]) / min(ms["rescale_a"] + ms["rescale_b"]),
        "rescale_a_over_b": med["rescale_a"] / med["rescale_b"],
        "mod_switch_spread": max(ms["mod_switch"]) / min(ms["mod_switch"]),
        "all_ms": ms,
    }
    print(f"N={n} L={L} {bits}-bit batch={B} class={eng.width_class}: mod_switch {med['mod_switch']:.3f} ms ({rec['mod_switch_gbs']:.0f} GB/s), "
          f"2 x rescale {rescale_med:.3f} ms ({rec['rescale_x2_gbs']:.0f} GB/s), ratio {rec['ratio_mod_switch_over_rescale']:.3f}, "
          f"rescale spread {rec['rescale_spread']:.3f}", flush=True)
    return rec


def main():
    if pkg.device_count() < 1:
        sys.exit("bench_modswitch.py: no HIP device (there is no CPU fallback to time)")
    recs = [run(*shape) for shape in SHAPES]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
