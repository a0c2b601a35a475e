#!/usr/bin/env python3
"""What stands around the blind-rotation loop, each new call against what does the same today, at the same shape, in one process, interleaved in
time (every round runs every candidate once; the MEDIAN of the rounds counts).  Every comparison is checked equal to the new path's output
before it is timed.
(a) prepare: ONE fhe_lwe_prepare_accumulator against the device call list: upload of the host-computed shift tables, a broadcast copy of tv
    (one device copy per ciphertext), fhe_rns_monomial_mul_sub + fhe_rns_poly_add, and a memset of acc1.
(b) extract: ONE fhe_rlwe_sample_extract against the download of (c0, c1) and a numpy gather on the host.
(c) key generation: fhe_rgsw_keys_generate for 64 RGSW ciphertexts on an engine created as it is (fused) and on one created under
    FHE_HIP_NO_FUSED_KEYGEN=1 (composed); once per (n, primes), it does not depend on the batch.
(d) prepare and extract as a share of a 64-step fhe_blind_rotate over the keys of (c).
Times are wall-clock microseconds per call around ITERS calls and one device synchronisation (the call lists have host parts, so stream events
would not bracket them).  HBM fractions are on the bytes each kernel has to move: prepare 2 S batch written, extract S batch read plus
8 L (n + 1) batch written.  One JSON line per shape.
usage: bench_bootstrap.py [out.jsonl]     (default profiles/bench_bootstrap.jsonl; appends)"""
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

ROUNDS = 5
STEPS = 64                                               # n_lwe = RGSW ciphertexts = steps of the loop
Q_LWE = 1 << 32
HBM_BYTES_PER_S = 8.0e12                                 # MI355X peak
W_OF = {30: 16, 40: 22}                                  # K = 2
CONFIGS = [("N=8192 4x30-bit", 8192, 30, 4), ("N=16384 6x30-bit", 16384, 30, 6), ("N=16384 6x40-bit", 16384, 40, 6)]
BATCHES = (256, 1)


def wall_us(call, iters):
    pkg.capi.sync()
    t0 = time.perf_counter()
    for _ in range(iters):
        call()
    pkg.capi.sync()
    return (time.perf_counter() - t0) * 1e6 / iters


def medians(cands, iters):
    """cands: {name: (call, iters or None)}; one warm-up each, then ROUNDS interleaved rounds"""
    seen = {k: [] for k in cands}
    for call, _ in cands.values():
        call()
    for _ in range(ROUNDS):
        for k, (call, it) in cands.items():
            seen[k].append(wall_us(call, it or iters))
    return {k: statistics.median(v) for k, v in seen.items()}, seen


def ms_host(v, n):
    return ((v.astype(object) * (2 * n) + Q_LWE // 2) // Q_LWE % (2 * n)).astype(np.uint32)


def rand_poly(rng, moduli, n, batch):
    out = np.zeros((batch, len(moduli), n, 4), dtype=np.uint64)
    for l, q in enumerate(moduli):
        out[:, l, :, 0] = rng.integers(0, q, (batch, n), dtype=np.uint64)
    return out


def bench_keys(name, n, bits, L, moduli):
    """(c): returns the record fields and (engine, rows_c0, rows_c1) of the fused engine, kept for (d)"""
    w = W_OF[bits]
    rng = np.random.default_rng(3)
    s = np.zeros((L, n, 4), dtype=np.uint64)
    tern = rng.integers(-1, 2, n)
    for l, q in enumerate(moduli):
        s[l, :, 0] = np.where(tern < 0, q - 1, tern).astype(np.uint64)
    os.environ.pop("FHE_HIP_NO_FUSED_KEYGEN", None)
    eng_f = pkg.RnsNttEngine(n, moduli)
    os.environ["FHE_HIP_NO_FUSED_KEYGEN"] = "1"
    eng_c = pkg.RnsNttEngine(n, moduli)
    os.environ.pop("FHE_HIP_NO_FUSED_KEYGEN")
    ds = pkg.DeviceBuffer.from_numpy(s)
    sk_f, sk_c = eng_f.import_secret_key(ds), eng_c.import_secret_key(ds)
    mu = [int(v) for v in rng.integers(0, 2, STEPS)]
    gen = lambda e, sk: e.generate_rgsw_keys(sk, w, mu, 1, 3.2, (5, 6))
    # equality of the two paths: the first and the last ciphertext, both components, through the export
    LK = L * eng_f.relin_num_digits(w)
    nbytes = LK * L * n * 32
    kf, kc = gen(eng_f, sk_f), gen(eng_c, sk_c)
    for i in (0, STEPS - 1):
        for c in (0, 1):
            got = []
            for e, keys in ((eng_f, kf), (eng_c, kc)):
                db, da = pkg.DeviceBuffer(nbytes), pkg.DeviceBuffer(nbytes)
                e.export_keys(keys[c][i], db, da)
                got.append((db.download(), da.download()))
            assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), (name, i, c)
    del kc
    times = {"fused": [], "composed": []}
    for _ in range(ROUNDS):
        for k, e, sk in (("fused", eng_f, sk_f), ("composed", eng_c, sk_c)):
            pkg.capi.sync(); t0 = time.perf_counter()
            keys = gen(e, sk)                            # the call synchronises before it returns
            times[k].append((time.perf_counter() - t0) * 1e6)
            del keys
    f, c = statistics.median(times["fused"]), statistics.median(times["composed"])
    rec = {"rgsw_ciphertexts": STEPS, "decomp_bits": w, "keygen_fused_us": f, "keygen_composed_us": c, "keygen_composed_over_fused": c / f,
           "keygen_all_us": times}
    return rec, (eng_f, kf, (ds, sk_f))


def bench_shape(name, n, bits, L, moduli, batch, eng, keys):
    rng = np.random.default_rng(11)
    S = L * n * 32
    tv = rand_poly(rng, moduli, n, 1)[0]
    lwe = rng.integers(0, Q_LWE, (batch, STEPS + 1), dtype=np.uint64)
    d_tv, d_lwe = pkg.DeviceBuffer.from_numpy(tv), pkg.DeviceBuffer.from_numpy(lwe)
    acc = [pkg.DeviceBuffer(batch * S) for _ in range(4)]            # acc0, acc1, tmp0, tmp1 of the loop
    ref0, ref1, d_tvb, d_tmp = (pkg.DeviceBuffer(batch * S) for _ in range(4))
    d_sh, ref_sh, d_bsh = pkg.DeviceBuffer(STEPS * batch * 4), pkg.DeviceBuffer(STEPS * batch * 4), pkg.DeviceBuffer(batch * 4)
    d_out = pkg.DeviceBuffer(batch * L * (n + 1) * 8)
    t = ms_host(lwe, n)
    h_sh = np.ascontiguousarray(((2 * n - t[:, :-1].T) % (2 * n)).astype(np.uint32))
    h_bsh = np.ascontiguousarray(((2 * n - t[:, -1]) % (2 * n)).astype(np.uint32))
    d2d, memset = pkg.lib().fhe_hip_memcpy_d2d, pkg.lib().fhe_hip_memset

    def prepare():
        eng.lwe_prepare_accumulator(Q_LWE, STEPS, d_lwe, d_tv, acc[0], acc[1], d_sh, batch)

    def prepare_list():
        ref_sh.upload(h_sh); d_bsh.upload(h_bsh)
        for b in range(batch):
            assert d2d(d_tvb.ptr + b * S, d_tv.ptr, S) == 0
        eng.monomial_mul_sub(d_tmp, d_tvb, d_bsh, batch)
        eng.poly_add(ref0, d_tmp, d_tvb, batch)
        assert memset(ref1.ptr, 0, batch * S) == 0

    prepare(); prepare_list()
    shape = (batch, L, n, 4)
    assert np.array_equal(acc[0].download(shape), ref0.download(shape)) and not acc[1].download(shape).any() and not ref1.download(shape).any()
    assert np.array_equal(d_sh.download((STEPS, batch), np.uint32), h_sh)

    # a pair to extract from: the result of the loop (also (d))
    def loop():
        eng.blind_rotate(keys[0], keys[1], acc[0], acc[1], d_sh, acc[2], acc[3], batch)

    eng.reserve(batch)
    loop()
    idx = n // 3
    host = {}

    def extract():
        eng.sample_extract(d_out, acc[0], acc[1], idx, batch)

    def extract_host():
        c0, c1 = acc[0].download(shape)[..., 0], acc[1].download(shape)[..., 0]
        j = np.arange(n)
        g = c1[:, :, (idx - j) % n]
        q = np.array(moduli, dtype=np.uint64)[None, :, None]
        out = np.empty((batch, L, n + 1), dtype=np.uint64)
        out[:, :, :n] = np.where((j <= idx)[None, None, :] | (g == 0), g, q - g)
        out[:, :, n] = c0[:, :, idx]
        host["out"] = out

    extract(); extract_host()
    assert np.array_equal(d_out.download((batch, L, n + 1)), host["out"])

    iters = 3 if batch > 1 else 20
    med, seen = medians({"prepare": (prepare, None), "prepare_call_list": (prepare_list, None), "extract": (extract, None),
                         "extract_download_host_gather": (extract_host, 1), "blind_rotate_64": (loop, 1)}, iters)
    wrote_p, moved_e = 2 * S * batch, S * batch + 8 * L * (n + 1) * batch
    p, e, lp = med["prepare"], med["extract"], med["blind_rotate_64"]
    return {"shape": name, "n": n, "limbs": L, "bits": bits, "batch": batch, "n_lwe": STEPS, "q_lwe_bits": 32, "rounds": ROUNDS,
            "prepare_us": p, "prepare_call_list_us": med["prepare_call_list"], "prepare_call_list_over_fused": med["prepare_call_list"] / p,
            "prepare_bytes_written": wrote_p, "prepare_tb_per_s": wrote_p / (p * 1e-6) / 1e12, "prepare_hbm_fraction": wrote_p / (p * 1e-6) / HBM_BYTES_PER_S,
            "extract_us": e, "extract_download_host_gather_us": med["extract_download_host_gather"],
            "extract_host_over_fused": med["extract_download_host_gather"] / e,
            "extract_bytes_moved": moved_e, "extract_tb_per_s": moved_e / (e * 1e-6) / 1e12, "extract_hbm_fraction": moved_e / (e * 1e-6) / HBM_BYTES_PER_S,
            "blind_rotate_64_us": lp, "prepare_share_of_loop": p / lp, "extract_share_of_loop": e / lp, "all_us": seen}


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_bootstrap.jsonl")
    with open(path, "a") as out:
        for name, n, bits, L in CONFIGS:
            moduli = pkg.find_ntt_primes(bits, n, L)
            krec, (eng, keys, _keep) = bench_keys(name, n, bits, L, moduli)
            for batch in BATCHES:
                rec = bench_shape(name, n, bits, L, moduli, batch, eng, keys)
                rec.update(krec)
                line = json.dumps(rec)
                print(line, flush=True)
                out.write(line + "\n"); out.flush()
            del keys, eng, _keep


if __name__ == "__main__":
    main()
