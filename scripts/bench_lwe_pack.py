#!/usr/bin/env python3
"""fhe_lwe_pack against the composed call list (fhe_lwe_to_rlwe, fhe_rns_monomial_mul_sub, fhe_rns_poly_add / sub, fhe_ct_apply_galois through
capi, buffers allocated once), at the same shape, in one process, interleaved in time (every round runs both once; the MEDIAN of the rounds
counts).  The composition is checked equal to the call's output before it is timed.  Trace and normalisation on.  Beside it the streaming
embedding launch (fhe_lwe_to_rlwe: the first-level kernel in its one-sample form) and fhe_lwe_prepare_accumulator at the same batch, as bytes
per second of the bytes each must move (samples in, containers out).  A shape whose samples and scratch exceed MEM_BUDGET is reported as not
measured.  Times are wall-clock microseconds per call around ITERS calls and one device synchronisation.  One JSON line per shape.
usage: bench_lwe_pack.py [out.jsonl]     (default profiles/bench_lwe_pack.jsonl; appends)"""
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
import lwe_pack_model as M  # noqa: E402

ROUNDS, W, MEM_BUDGET = 3, 16, 40 << 30
CONFIGS = [("N=8192 4x30-bit", 8192, 30, 4), ("N=16384 6x40-bit", 16384, 40, 6)]
BATCHES = (1, 16)


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


def composed(eng, keys, moduli, n, count, batch, d_lwe_normalised, out):
    """the call list with every buffer allocated up front; returns the callable"""
    L = len(moduli); S = L * n * 32
    buf = lambda cts: (pkg.DeviceBuffer(cts * S), pkg.DeviceBuffer(cts * S))
    R = buf(batch * count)
    X, P, D, T = buf(max(batch * count // 2, batch)), buf(max(batch * count // 2, 1)), buf(max(batch * count // 2, 1)), buf(batch)
    levels = M.merge_levels(count)
    shifts = [pkg.DeviceBuffer.from_numpy(np.full(half, n // c, np.uint32)) for _, half, c, _ in levels]

    def call():
        eng.lwe_to_rlwe(R[0], R[1], d_lwe_normalised, batch * count)
        cur = count
        for (l, half, c, g), sh in zip(levels, shifts):
            for b in range(batch):
                for k in range(2):
                    E = R[k].ptr + b * cur * S; O = E + half * S; at = b * half * S
                    eng.monomial_mul_sub(X[k].ptr + at, O, sh, half)
                    eng.poly_add(X[k].ptr + at, X[k].ptr + at, O, half)
                    eng.poly_add(P[k].ptr + at, E, X[k].ptr + at, half)
                    eng.poly_sub(D[k].ptr + at, E, X[k].ptr + at, half)
            eng.apply_galois(keys[l - 1], g, X[0], X[1], D[0], D[1], batch * half)
            dst = out if half == 1 else R
            for k in range(2):
                eng.poly_add(dst[k], P[k], X[k], batch * half)
            cur = half
        if count == 1:
            for k in range(2):
                pkg.lib().fhe_hip_memcpy_d2d(out[k].ptr, R[k].ptr, batch * S)
        for j in range(count.bit_length(), n.bit_length()):
            eng.apply_galois(keys[j - 1], (1 << j) + 1, T[0], T[1], out[0], out[1], batch)
            for k in range(2):
                eng.poly_add(out[k], out[k], T[k], batch)
    return call, (R, X, P, D, T, shifts)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_lwe_pack.jsonl")
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
        S = L * n * 32
        for count in (64, n):
            for batch in BATCHES:
                sample_bytes = batch * count * L * (n + 1) * 8
                need = sample_bytes + 3 * batch * count * S                            # the samples and the call's three regions
                if count <= 64:
                    need += sample_bytes + 6 * batch * count * S                       # the normalised samples, R and X / P / D of the list
                line = {"bench": "lwe_pack", "shape": name, "n": n, "L": L, "w": W, "count": count, "batch": batch, "trace": 1, "normalize": 1}
                if need > MEM_BUDGET:
                    line.update(measured=False, reason=f"samples and scratch need {need >> 30} GiB, above the {MEM_BUDGET >> 30} GiB this script allows itself")
                else:
                    lwe = np.stack([rng.integers(0, q, (batch * count, n + 1), dtype=np.uint64) for q in moduli], axis=1)
                    norm = np.stack([((lwe[:, l].astype(object) * pow(n, -1, q)) % q).astype(np.uint64) for l, q in enumerate(moduli)], axis=1) if count <= 64 else None
                    d_lwe = pkg.DeviceBuffer.from_numpy(lwe)
                    o = (pkg.DeviceBuffer(batch * S), pkg.DeviceBuffer(batch * S))
                    eng.lwe_pack_reserve(keys, count, True, batch)
                    fused = lambda: eng.lwe_pack(keys, o[0], o[1], d_lwe, count, True, True, batch)
                    fused()
                    want = [x.download((batch, L, n, 4)) for x in o]
                    cands = {"call": fused}
                    if norm is not None:                                        # F^-1 on the host costs minutes of Python integers at count = n: the list is timed at count = 64
                        d_norm = pkg.DeviceBuffer.from_numpy(norm)
                        c_out = (pkg.DeviceBuffer(batch * S), pkg.DeviceBuffer(batch * S))
                        comp, keep = composed(eng, keys, moduli, n, count, batch, d_norm, c_out)
                        comp()
                        assert all(np.array_equal(x.download((batch, L, n, 4)), w) for x, w in zip(c_out, want)), (name, count, batch)
                        cands["composed"] = comp
                    us = medians(cands, 3 if count <= 64 else 1)
                    # the streaming launches at batch * count samples / accumulators
                    e = batch * min(count, 64)
                    c0, c1, sh, tv = pkg.DeviceBuffer(e * S), pkg.DeviceBuffer(e * S), pkg.DeviceBuffer(e * 4), pkg.DeviceBuffer(S)
                    tv.zero()
                    small = pkg.DeviceBuffer.from_numpy(rng.integers(0, 1 << 32, (e, 2), dtype=np.uint64))
                    st = medians({"embed": lambda: eng.lwe_to_rlwe(c0, c1, d_lwe, e),
                                  "prepare": lambda: eng.lwe_prepare_accumulator(1 << 32, 1, small, tv, c0, c1, sh, e)}, 10)
                    line.update(measured=True, us_call=round(us["call"], 1), levels=count.bit_length() - 1, trace_steps=n.bit_length() - count.bit_length(),
                                embed_us=round(st["embed"], 1), embed_bytes_per_s=round((e * L * (n + 1) * 8 + 2 * e * S) / (st["embed"] * 1e-6), 1),
                                prepare_us=round(st["prepare"], 1), prepare_bytes_per_s=round((2 * e * S) / (st["prepare"] * 1e-6), 1), streaming_entries=e)
                    if "composed" in us:
                        line.update(us_composed=round(us["composed"], 1), composed_over_call=round(us["composed"] / us["call"], 3))
                    for d in (d_lwe, c0, c1, sh, tv, small, *o):
                        d.free()
                print(json.dumps(line), flush=True)
                with open(out_path, "a") as f:
                    f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
