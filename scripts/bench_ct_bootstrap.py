#!/usr/bin/env python3
"""The two joints of FHEContext::bootstrap(Ciphertext&) against the call lists they replace, and the whole pipeline by stage, in one process,
interleaved in time (every round runs every candidate once; the MEDIAN of the rounds counts).  Each new call is checked equal to its call list
before it is timed.  Times are wall-clock microseconds per call around ITERS calls and one device synchronisation.
  extract   fhe_rlwe_sample_extract_strided against `count` calls of fhe_rlwe_sample_extract writing the same layout (batch 1), count = 64 and
            count = n; TB/s on the bytes written
  pack      fhe_rlwe_pack against fhe_rlwe_sample_extract(idx = 0) + fhe_lwe_pack, count = 64, batch 1 and 16, trace and normalisation on
  pipeline  rescale to one prime, strided extraction, LWE key switch (w = 8, q_out = 2^32), accumulator preparation, blind rotation (RGSW w = 16,
            N_LWE steps, batch = count), packing, at count = 64; the blind rotation's share of the sum
One JSON line per measurement.
usage: bench_ct_bootstrap.py [out.jsonl]     (default profiles/bench_ct_bootstrap.jsonl; appends)"""
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

ROUNDS, W, W_KS, N_LWE, Q_LWE, MEM_BUDGET = 3, 16, 8, 64, 1 << 32, 40 << 30
CONFIGS = [("N=8192 4x30-bit", 8192, 30, 4), ("N=16384 6x40-bit", 16384, 40, 6)]


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


def polys(rng, moduli, n, entries):
    out = np.zeros((entries, len(moduli), n, 4), dtype=np.uint64)
    for l, q in enumerate(moduli):
        out[:, l, :, 0] = rng.integers(0, q, (entries, n), dtype=np.uint64)
    return out


def emit(out_path, line):
    print(json.dumps(line), flush=True)
    with open(out_path, "a") as f:
        f.write(json.dumps(line) + "\n")


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_ct_bootstrap.jsonl")
    rng = np.random.default_rng(1)
    for name, n, bits, L in CONFIGS:
        moduli = pkg.find_ntt_primes(bits, n, L)
        eng = pkg.RnsNttEngine(n, moduli)
        s = rng.integers(-1, 2, n)
        cont = np.zeros((L, n, 4), dtype=np.uint64)
        for l, q in enumerate(moduli):
            cont[l, :, 0] = np.where(s < 0, q - 1, s).astype(np.uint64)
        ds = pkg.DeviceBuffer.from_numpy(cont)
        sk = eng.import_secret_key(ds)
        keys = eng.generate_keyswitch_keys(sk, W, pkg.capi.lwe_pack_galois_elements(n), 1, 3.2, (5, 6))
        S, row = L * n * 32, L * (n + 1) * 8
        base = {"shape": name, "n": n, "L": L}

        # ---- 1. strided extraction, batch 1
        ct = [pkg.DeviceBuffer.from_numpy(polys(rng, moduli, n, 1)) for _ in range(2)]
        for count in (64, n):
            line = dict(base, bench="extract_strided", count=count, batch=1, bytes_written=count * row)
            if 2 * count * row > MEM_BUDGET:
                emit(out_path, dict(line, measured=False, reason="the two sample buffers exceed the memory this script allows itself")); continue
            a, b = pkg.DeviceBuffer(count * row), pkg.DeviceBuffer(count * row)

            def singles():
                for i in range(count):
                    eng.sample_extract(b.ptr + i * row, ct[0], ct[1], i * (n // count), 1)
            eng.sample_extract_strided(a, ct[0], ct[1], count, 1); singles()
            assert np.array_equal(a.download((count, L, n + 1)), b.download((count, L, n + 1))), (name, count)
            us = medians({"strided": lambda: eng.sample_extract_strided(a, ct[0], ct[1], count, 1), "singles": singles}, 20 if count <= 64 else 2)
            emit(out_path, dict(line, measured=True, us_strided=round(us["strided"], 1), us_singles=round(us["singles"], 1),
                                singles_over_strided=round(us["singles"] / us["strided"], 2), strided_TB_per_s=round(count * row / us["strided"] / 1e6, 3),
                                singles_TB_per_s=round(count * row / us["singles"] / 1e6, 3)))
            a.free(); b.free()

        # ---- 2. packing from RLWE pairs, count 64
        count = 64
        for batch in (1, 16):
            e = batch * count
            acc = [pkg.DeviceBuffer.from_numpy(polys(rng, moduli, n, e)) for _ in range(2)]
            d_lwe = pkg.DeviceBuffer(e * row)
            o, r = [pkg.DeviceBuffer(batch * S) for _ in range(2)], [pkg.DeviceBuffer(batch * S) for _ in range(2)]
            eng.lwe_pack_reserve(keys, count, True, batch)
            fused = lambda: eng.rlwe_pack(keys, o[0], o[1], acc[0], acc[1], count, True, True, batch)

            def two_calls():
                eng.sample_extract(d_lwe, acc[0], acc[1], 0, e)
                eng.lwe_pack(keys, r[0], r[1], d_lwe, count, True, True, batch)
            fused(); two_calls()
            assert all(np.array_equal(x.download((batch, L, n, 4)), y.download((batch, L, n, 4))) for x, y in zip(o, r)), (name, batch)
            us = medians({"rlwe_pack": fused, "extract_then_lwe_pack": two_calls, "extract_alone": lambda: eng.sample_extract(d_lwe, acc[0], acc[1], 0, e)}, 3)
            emit(out_path, dict(base, bench="rlwe_pack", count=count, batch=batch, w=W, trace=1, normalize=1, measured=True, us_rlwe_pack=round(us["rlwe_pack"], 1),
                                us_extract_then_lwe_pack=round(us["extract_then_lwe_pack"], 1), us_extract_alone=round(us["extract_alone"], 1),
                                composition_over_call=round(us["extract_then_lwe_pack"] / us["rlwe_pack"], 3), sample_bytes_never_written=e * row))
            for d in (*acc, d_lwe, *o, *r):
                d.free()

        # ---- 3. the pipeline by stage, count 64
        z = [int(v) for v in rng.integers(0, 2, N_LWE)]
        r0, r1 = eng.generate_rgsw_keys(sk, W, z, 1, 3.2, (21, 22))
        ksk = eng.generate_lwe_ksk(sk, W_KS, z, 1, 3.2, (31, 32))
        levels = [eng] + [pkg.RnsNttEngine(n, moduli[:k]) for k in range(L - 1, 0, -1)]      # engines of L, L - 1, .., 1 primes
        eng1 = levels[-1]
        lows = [[pkg.DeviceBuffer(k * n * 32) for _ in range(2)] for k in range(L - 1, 0, -1)]
        d_ext, d_ks = pkg.DeviceBuffer(count * (n + 1) * 8), pkg.DeviceBuffer(count * (N_LWE + 1) * 8)
        acc = [pkg.DeviceBuffer(count * S) for _ in range(4)]
        d_sh, tv = pkg.DeviceBuffer(N_LWE * count * 4), pkg.DeviceBuffer.from_numpy(polys(rng, moduli, n, 1))
        o = [pkg.DeviceBuffer(S) for _ in range(2)]
        eng.lwe_pack_reserve(keys, count, True, 1)

        def rescale():
            src = ct
            for e_l, dst in zip(levels[:-1], lows):
                e_l.rescale_drop_last(dst[0], src[0], 1); e_l.rescale_drop_last(dst[1], src[1], 1)
                pkg.capi.sync()                                                           # the next engine has a stream of its own
                src = dst
        stages = {"rescale": rescale,
                  "extract_strided": lambda: eng1.sample_extract_strided(d_ext, lows[-1][0], lows[-1][1], count, 1),
                  "lwe_keyswitch": lambda: eng1.lwe_keyswitch(ksk, d_ks, d_ext, Q_LWE, count),
                  "prepare": lambda: eng.lwe_prepare_accumulator(Q_LWE, N_LWE, d_ks, tv, acc[0], acc[1], d_sh, count),
                  "blind_rotate": lambda: eng.blind_rotate(r0, r1, acc[0], acc[1], d_sh, acc[2], acc[3], count),
                  "rlwe_pack": lambda: eng.rlwe_pack(keys, o[0], o[1], acc[0], acc[1], count, True, True, 1)}
        for call in stages.values():                                                      # in pipeline order once, so that every stage has real inputs
            call(); pkg.capi.sync()
        us = medians(stages, 3)
        total = sum(us.values())
        emit(out_path, dict(base, bench="ct_bootstrap_pipeline", count=count, n_lwe=N_LWE, w=W, w_ks=W_KS, q_lwe=Q_LWE, measured=True,
                            us={k: round(v, 1) for k, v in us.items()}, us_total=round(total, 1), blind_rotate_share=round(us["blind_rotate"] / total, 4),
                            blind_rotate_us_per_step=round(us["blind_rotate"] / N_LWE, 1)))


if __name__ == "__main__":
    main()
