#!/usr/bin/env python3
"""The batch encoder as ONE fhe_slots_encode / fhe_slots_decode_poly against two comparators, at the same shape, in the same process,
interleaved in time: the calls alternate, the best of REPS repetitions of each counts.
(a) What the device can do with the entry points that exist without the encoder, natural order, t <= q: the slot values expanded on the host
    into [batch][1][n] containers of an engine on (n, t) and uploaded (timed once, separately: host_expand_upload_us), then on the device one
    copy into the work buffer, fhe_bit_reverse, fhe_rns_ntt_inverse, and L strided device copies (one hipMemcpy2D per limb over the whole
    batch) into the [batch][L][n] plaintexts; decoding is one strided copy of limb 0, fhe_rns_ntt_forward and fhe_bit_reverse.
(b) The C++ mirror's host encode / decode, upload included, one plaintext per call (scripts/bench_encode_mirror.cpp, built here with g++ and
    run between the shapes; wall time, so it is reported per plaintext and compared with the mirror's own encode_fused / decode_fused).
One JSON line per shape and direction: microseconds per call, the ratios, and the fraction of the HBM roof on the bytes the fused call has to
move (8 n + L 32 n per plaintext for encode, 8 n + 8 n for decode).
usage: bench_encode.py [out.jsonl]     (appends, so that a second run lands in the same file)"""
import ctypes
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
pkg = importlib.import_module("gpu-homomorphic-encryption_amd")

REPS = 5
T = 65537
HBM_BYTES_PER_S = 8.0e12                                 # MI355X peak
SHAPES = [("N=8192 4x30-bit", 8192, 30, 4, 1024), ("N=16384 6x30-bit", 16384, 30, 6, 1024), ("N=16384 6x40-bit", 16384, 40, 6, 1024),
          ("N=8192 4x30-bit, batch 1", 8192, 30, 4, 1), ("N=16384 6x30-bit, batch 1", 16384, 30, 6, 1), ("N=16384 6x40-bit, batch 1", 16384, 40, 6, 1)]
D2D = 3                                                  # hipMemcpyDeviceToDevice


def once(eng, call, iters):
    t = pkg.Timer(); t.start(eng)
    for _ in range(iters):
        call()
    t.stop(eng)
    return t.elapsed_ms() * 1e3 / iters                  # microseconds per call


def build_mirror_harness():
    pkg.build_library()
    lib_dir = os.path.dirname(pkg.library_path())
    exe = os.path.join(tempfile.mkdtemp(prefix="bench_encode_"), "bench_encode_mirror")
    cmd = ["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "scripts", "bench_encode_mirror.cpp"), "-L", lib_dir, "-lfhe_hip",
           f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def main():
    out = open(sys.argv[1], "a") if len(sys.argv) > 1 else None
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy2D.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpy2D.restype = ctypes.c_int
    d2d = pkg.lib().fhe_hip_memcpy_d2d
    harness = build_mirror_harness()
    for name, n, bits, L, batch in SHAPES:
        mirror = subprocess.run([harness, str(n), str(bits), str(L), str(REPS)], capture_output=True, text=True, timeout=300)
        assert mirror.returncode == 0, mirror.stdout + mirror.stderr
        mirror = json.loads(mirror.stdout.strip().splitlines()[-1])
        moduli = pkg.find_ntt_primes(bits, n, L)
        eng = pkg.RnsNttEngine(n, moduli)
        teng = pkg.RnsNttEngine(n, [T])                  # an engine on (n, t): containers only
        enc = pkg.capi.BatchEncoder(eng, T, pkg.capi.SLOTS_NATURAL)
        enc.reserve(batch)
        P, S = n * 32, L * n * 32
        vals = np.random.default_rng(7).integers(0, T, (batch, n), dtype=np.uint64)
        t0 = time.perf_counter()
        cont = np.zeros((batch, n, 4), dtype=np.uint64)
        cont[:, :, 0] = vals                             # slot order; the device bit-reverses
        d_cont = pkg.DeviceBuffer.from_numpy(cont)
        pkg.capi.sync()
        host_us = (time.perf_counter() - t0) * 1e6
        del cont
        d_vals = pkg.DeviceBuffer.from_numpy(vals)
        d_work, d_pt, d_pt2, d_back = pkg.DeviceBuffer(batch * P), pkg.DeviceBuffer(batch * S), pkg.DeviceBuffer(batch * S), pkg.DeviceBuffer(batch * n * 8)
        iters = 2 if batch > 1 else 20

        def composed_encode():
            assert d2d(d_work.ptr, d_cont.ptr, batch * P) == 0
            pkg.bit_reverse(d_work, n, batch)
            teng.inverse(d_work, batch)
            for l in range(L):                           # limb l of every plaintext: rows of P bytes, S bytes apart
                assert hip.hipMemcpy2D(d_pt2.ptr + l * P, S, d_work.ptr, P, P, batch, D2D) == 0

        def composed_decode():
            assert hip.hipMemcpy2D(d_work.ptr, P, d_pt2.ptr, S, P, batch, D2D) == 0
            teng.forward(d_work, batch)
            pkg.bit_reverse(d_work, n, batch)

        def fused_encode():
            enc.encode(d_pt, d_vals, batch)

        def fused_decode():
            enc.decode_poly(d_back, d_pt, batch)

        for fn in (composed_encode, fused_encode, composed_decode, fused_decode):
            fn()                                         # warm-up: code objects, tables, clocks
        pkg.capi.sync()
        if batch == 1:                                   # both ways give the same bits (the large batches would download gigabytes)
            assert np.array_equal(d_pt.download((batch, L, n, 4)), d_pt2.download((batch, L, n, 4)))
            assert np.array_equal(d_work.download((batch, n, 4))[:, :, 0], vals)
        assert np.array_equal(d_back.download((batch, n)), vals)
        best = {}
        for _ in range(REPS):                            # interleaved: every repetition runs all four once
            for kind, fn in (("composed_encode", composed_encode), ("fused_encode", fused_encode), ("composed_decode", composed_decode), ("fused_decode", fused_decode)):
                us = once(eng, fn, iters)
                best[kind] = min(best.get(kind, us), us)
        for what, moved in (("encode", batch * (8 * n + S)), ("decode", batch * 16 * n)):
            f, c = best["fused_" + what], best["composed_" + what]
            rec = {"shape": name, "op": what, "n": n, "limbs": L, "bits": bits, "batch": batch, "t": T, "order": "natural", "reps": REPS, "device_call_list_us": c, "fused_us": f,
                   "device_call_list_over_fused": c / f, "fused_per_s": batch / (f * 1e-6), "host_expand_upload_us": host_us, "fused_bytes_moved": moved,
                   "fused_hbm_fraction": moved / (f * 1e-6) / HBM_BYTES_PER_S, "fused_tb_per_s": moved / (f * 1e-6) / 1e12,
                   "mirror_host_us_per_plaintext": mirror[f"mirror_host_{what}_us"], "mirror_fused_us_per_plaintext": mirror[f"mirror_{what}_fused_us"]}
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n"); out.flush()
        del d_cont, d_vals, d_work, d_pt, d_pt2, d_back, enc, teng, eng
    if out:
        out.close()


if __name__ == "__main__":
    main()
