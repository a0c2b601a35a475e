"""Galois automorphisms and slot rotations: fhe_galois_element, fhe_rns_automorphism, fhe_ct_apply_galois (include/fhe_hip.h).

The oracle has no automorphism: sigma_g is computed here with numpy / Python integers, and the key switch of a rotation is taken from
the oracle's RnsPlan.relinearize -- apply_galois must equal relinearize(w, sigma(c0), 0, sigma(c1), kb, ka) bit for bit."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

import ntt_math as nm
from workload import rns_poly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpu-homomorphic-encryption_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
MASK64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------ helpers
def _moduli(spec, n):
    if isinstance(spec, tuple) and spec[0] == "mix":
        return [q for bits, cnt in spec[1:] for q in nm.ntt_primes(bits, n, cnt)]
    if isinstance(spec, tuple):
        return nm.ntt_primes(spec[1], n, spec[2])
    return list(spec)


def sigma_np(a, moduli, g):
    """sigma_g on [batch][L][n][4] containers: out[j] = in[i] (i = j g^-1 mod 2n < n), else q - in[i - n] (0 stays 0)."""
    n = a.shape[2]
    i = (np.arange(n, dtype=np.int64) * pow(g, -1, 2 * n)) % (2 * n)
    neg = i >= n
    out = np.ascontiguousarray(a[:, :, i % n, :])
    for l, q in enumerate(moduli):
        sel = out[:, l][:, neg]                                           # [batch][#neg][4]
        if q < (1 << 64):
            v = sel[..., 0]
            sel[..., 0] = np.where(v == 0, np.uint64(0), np.uint64(q) - v)
        else:
            flat = sel.reshape(-1, 4)
            for r in range(flat.shape[0]):
                v = sum(int(flat[r, k]) << (64 * k) for k in range(4))
                v = (q - v) % q
                flat[r] = [(v >> (64 * k)) & MASK64 for k in range(4)]
            sel = flat.reshape(sel.shape)
        out[:, l, neg] = sel
    return out


def _random_keys(moduli, n, count, seed):
    return [rns_poly(seed + 17 * i, moduli, n, 1)[0] for i in range(count)]


def _elements(n, seed):
    rng = random.Random(seed)
    m = 2 * n
    return sorted({1, 3, m - 1, pow(3, rng.randrange(1, n // 2), m), rng.randrange(1, m) | 1})


# ------------------------------------------------------------------------------------------------ CPU
def test_galois_element_matches_python(pkg):
    for n in (8, 16, 1024, 8192, 65536):
        for steps in list(range(-9, 10)) + [n // 2, n // 2 + 1, -n // 2 - 3, 12345, -(1 << 31), (1 << 31) - 1]:
            assert pkg.galois_element(n, steps) == pow(3, steps % (n // 2), 2 * n), (n, steps)
    for bad in (0, 1, 2, 4, 6, 12, 1000, 3 << 10):
        with pytest.raises(pkg.FheError) as e:
            pkg.galois_element(bad, 1)
        assert e.value.code == -1


KERNEL_SRC = """#include "galois.hip.h"
using namespace fhe_dev;
#define INST(F, S) \\
  template __global__ void fhe_dev::galois_kernel<F, S>(F::V16*, F::V16*, F::V16*, const F::V16*, const F::V16*, const Limb<F>*, uint32_t, uint32_t, uint32_t, size_t); \\
  template __global__ void fhe_dev::galois_compact_kernel<F, S>(F::E*, F::E*, F::E*, const F::V16*, const F::V16*, const Limb<F>*, uint32_t, uint32_t, uint32_t, size_t);
INST(F32, true) INST(F32, false) INST(F52, true) INST(F52, false) INST(F64, true) INST(F64, false) INST(F64X, true) INST(F64X, false)
"""


def test_galois_kernels_do_not_spill(tmp_path):
    """Every instantiated automorphism kernel (both forms, every word-sized field, and the full-width one) runs without scratch."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    src = tmp_path / "galois_res.hip"
    src.write_text(KERNEL_SRC)
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-I", CSRC, "-Rpass-analysis=kernel-resource-usage",
           "-c", "-o", str(tmp_path / "galois_res.o"), str(src)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    kernels, cur = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        for key, pat in (("spill", r"VGPRs Spill: (\d+)"), ("sspill", r"SGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    names = [k for k in kernels if "galois" in k]
    assert sum("galois_kernel" in k for k in names) == 8 and sum("galois_compact_kernel" in k for k in names) == 8, names
    assert sum("galois256_kernel" in k for k in names) == 1, names
    for k in names:
        r = kernels[k]
        assert r.get("scratch", 0) == 0 and r.get("spill", 0) == 0 and r.get("sspill", 0) == 0, (k, r)


# ------------------------------------------------------------------------------------------------ GPU: the automorphism
AUTO_CASES = [(256, 30, 2, 3), (2048, 30, 1, 1), (8192, 30, 4, 3), (16384, 30, 6, 2), (32768, 30, 2, 1), (65536, 30, 1, 2),
              (4096, 40, 3, 2), (16384, 40, 2, 1), (32768, 40, 1, 1), (2048, 60, 5, 2), (8192, 60, 2, 1), (16384, 60, 1, 1),
              (4096, 64, 2, 2), (8192, 64, 1, 1), (1024, 120, 2, 2), (4096, 128, 1, 1), (256, 250, 1, 3), (2048, 250, 1, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,bits,L,batch", AUTO_CASES)
def test_automorphism_matches_numpy(pkg, n, bits, L, batch):
    moduli = nm.ntt_primes(bits, n, L)
    e = pkg.RnsNttEngine(n, moduli)
    a = rns_poly(31 + L, moduli, n, batch)
    for l, q in enumerate(moduli):                                         # zeros and q - 1 among the coefficients: 0 -> 0, q - 1 -> 1
        a[:, l, ::97, :] = 0
        a[:, l, 5::101, :] = [((q - 1) >> (64 * k)) & MASK64 for k in range(4)]
    d_in, d_out = pkg.DeviceBuffer.from_numpy(a), pkg.DeviceBuffer(a.nbytes)
    for g in _elements(n, n + bits):
        e.automorphism(d_out, d_in, g, batch)
        assert np.array_equal(d_out.download(a.shape), sigma_np(a, moduli, g)), g
    assert np.array_equal(d_in.download(a.shape), a)


@pytest.mark.gpu
@pytest.mark.parametrize("n,bits,L", [(8192, 30, 3), (4096, 40, 2), (2048, 64, 2), (32768, 30, 1), (1024, 250, 1)])
def test_automorphism_algebra_and_bad_arguments(pkg, n, bits, L):
    moduli = nm.ntt_primes(bits, n, L)
    e = pkg.RnsNttEngine(n, moduli)
    a = rns_poly(5, moduli, n, 2)
    d = [pkg.DeviceBuffer.from_numpy(a), pkg.DeviceBuffer(a.nbytes), pkg.DeviceBuffer(a.nbytes)]
    e.automorphism(d[1], d[0], 1, 2)                                      # sigma_1 is the identity
    assert np.array_equal(d[1].download(a.shape), a)
    rng = random.Random(n)
    for _ in range(3):                                                    # sigma_g o sigma_h = sigma_{gh mod 2n}
        g, h = rng.randrange(1, 2 * n) | 1, rng.randrange(1, 2 * n) | 1
        e.automorphism(d[1], d[0], h, 2); e.automorphism(d[2], d[1], g, 2)
        gh = pkg.DeviceBuffer(a.nbytes); e.automorphism(gh, d[0], g * h % (2 * n), 2)
        assert np.array_equal(d[2].download(a.shape), gh.download(a.shape))
    g = pkg.galois_element(n, 1)                                          # 3^(n/2) = 1: n/2 row steps come back
    cur, nxt = d[0], d[1]
    e.automorphism(nxt, cur, pow(g, n // 4, 2 * n), 2); e.automorphism(d[2], nxt, pow(g, n // 4, 2 * n), 2)
    assert np.array_equal(d[2].download(a.shape), a)
    for bad in (0, 2, 2 * n, 2 * n + 1, 4 * n - 1):
        with pytest.raises(pkg.FheError) as ex:
            e.automorphism(d[1], d[0], bad, 2)
        assert ex.value.code == -1
    with pytest.raises(pkg.FheError):
        e.automorphism(d[0], d[0], 3, 2)                                  # out == in


# ------------------------------------------------------------------------------------------------ GPU: rotation = automorphism + key switch
APPLY_CASES = [(8192, ("bits", 30, 4), 16, 3), (16384, ("bits", 30, 3), 30, 2), (2048, [40961], 8, 9),
               (32768, ("bits", 30, 1), 16, 1), (65536, ("bits", 30, 1), 16, 1),
               (4096, ("bits", 40, 2), 20, 3), (8192, ("bits", 43, 2), 16, 1), (16384, ("bits", 40, 2), 20, 1),
               (2048, ("bits", 60, 2), 32, 2), (8192, ("bits", 64, 1), 32, 1), (256, ("bits", 250, 1), 64, 2),
               (2048, ("bits", 120, 1), 40, 1), (8192, ("bits", 30, 4), 16, 40)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,spec,w,batch", APPLY_CASES)
@pytest.mark.parametrize("variant", ["default", "composed", "no-split-pairs"])
def test_apply_galois_matches_oracle(pkg, oracle, monkeypatch, n, spec, w, batch, variant):
    """fhe_ct_apply_galois == oracle relinearize(sigma(c0), 0, sigma(c1)) bit for bit: the fused path (prologue + compact-operand key
    switch), the composed one (FHE_HIP_NO_FUSED_GALOIS=1) and the fused one without the few-ciphertext key-switch forms."""
    if variant == "composed":
        monkeypatch.setenv("FHE_HIP_NO_FUSED_GALOIS", "1")
    if variant == "no-split-pairs":
        monkeypatch.setenv("FHE_HIP_SPLIT_PAIRS_POLYS", "0")
    moduli = _moduli(spec, n); L = len(moduli)
    e = pkg.RnsNttEngine(n, moduli); rp = oracle.RnsPlan(n, moduli)
    K = e.relin_num_digits(w)
    kb = _random_keys(moduli, n, L * K, 700); ka = _random_keys(moduli, n, L * K, 1300)
    gk = e.import_relin_keys(w, [pkg.DeviceBuffer.from_numpy(k) for k in kb], [pkg.DeviceBuffer.from_numpy(k) for k in ka])
    c0, c1 = rns_poly(81, moduli, n, batch), rns_poly(82, moduli, n, batch)
    d0, d1 = pkg.DeviceBuffer.from_numpy(c0), pkg.DeviceBuffer.from_numpy(c1)
    o0, o1 = pkg.DeviceBuffer(c0.nbytes), pkg.DeviceBuffer(c0.nbytes)
    zero = np.zeros_like(c0)
    for g in (pkg.galois_element(n, 1), 2 * n - 1):
        for _ in range(2):                                               # the second call reuses the workspace
            e.apply_galois(gk, g, o0, o1, d0, d1, batch)
        w0, w1 = rp.relinearize(w, sigma_np(c0, moduli, g), zero, sigma_np(c1, moduli, g), kb, ka, threads=8)
        assert np.array_equal(o0.download(c0.shape), w0), g
        assert np.array_equal(o1.download(c0.shape), w1), g
    assert np.array_equal(d0.download(c0.shape), c0) and np.array_equal(d1.download(c0.shape), c1)   # inputs are read only
    with pytest.raises(pkg.FheError):
        e.apply_galois(gk, 3, d0, o1, d0, d1, batch)                     # an output aliases an input
    with pytest.raises(pkg.FheError):
        e.apply_galois(gk, 3, o0, o0, d0, d1, batch)                     # outputs must be distinct
    with pytest.raises(pkg.FheError):
        e.apply_galois(gk, 2, o0, o1, d0, d1, batch)                     # even element
    other = pkg.RnsNttEngine(n, moduli)
    with pytest.raises(pkg.FheError):
        other.apply_galois(gk, 3, o0, o1, d0, d1, batch)                 # keys imported for another engine


# ------------------------------------------------------------------------------------------------ GPU: slots end to end
def _toy(pkg, oracle):
    import bgv_toy
    n, t = 1024, 65537
    moduli = pkg.find_ntt_primes(30, n, 3)
    rp = oracle.RnsPlan(n, moduli)

    def fast_mul(x, y):
        return bgv_toy.from_limb_array(rp.polymul(bgv_toy.to_limb_array(x), bgv_toy.to_limb_array(y), threads=8))

    return bgv_toy, bgv_toy.ToyBGV(n, moduli, t, seed=23, fast_mul=fast_mul)


def _galois_keys(S, g, w):
    """Key rows of element g in the relinearisation-key layout with sigma_g(s) in place of s^2 (noise times t)."""
    n = S.n
    sg = [0] * n
    for i, c in enumerate(S.s):                                           # x^i -> x^(i g) = +-x^(i g mod n)
        k = i * g % (2 * n)
        sg[k % n] = c if k < n else -c
    K = (max(q.bit_length() for q in S.moduli) + w - 1) // w
    s_r, sg_r = S.to_rns(S.s), S.to_rns(sg)
    kb, ka = [], []
    for j in range(S.L):
        for k in range(K):
            a = S.uniform(); e = S.small()
            b = S.sub(S.to_rns([S.t * x for x in e]), S.mul(a, s_r))
            gj = pow(2, k * w, S.moduli[j])
            b[j] = [(u + gj * v) % S.moduli[j] for u, v in zip(b[j], sg_r[j])]
            kb.append(b); ka.append(a)
    return kb, ka


@pytest.mark.gpu
def test_rotations_move_slots_end_to_end(pkg, oracle):
    """Encrypt slot_encode(v), apply 3^r (rows) or 2n - 1 (columns) on the GPU, decrypt: slot i holds v[pi_g(i)], a cyclic left shift by r
    of both rows in the 3-power order; the column element swaps the rows; two rotations compose."""
    bgv_toy, S = _toy(pkg, oracle)
    n, t, w = S.n, S.t, 16
    half = n // 2
    e = pkg.RnsNttEngine(n, S.moduli)
    shape = (1, S.L, n, 4)

    def up(x):
        return pkg.DeviceBuffer.from_numpy(bgv_toy.to_limb_array(x))

    keys = {}

    def rotate(ct, g):
        if g not in keys:
            kb, ka = _galois_keys(S, g, w)
            keys[g] = e.import_relin_keys(w, [up(k) for k in kb], [up(k) for k in ka])
        o0, o1 = pkg.DeviceBuffer(ct[0].nbytes), pkg.DeviceBuffer(ct[0].nbytes)
        e.apply_galois(keys[g], g, o0, o1, ct[0], ct[1], 1)
        return o0, o1

    def slots(ct):
        return S.slot_decode(S.decrypt([bgv_toy.from_limb_array(x.download(shape)) for x in ct]))

    def perm(vals, g):
        return [vals[(g * (2 * i + 1) % (2 * n) - 1) // 2] for i in range(n)]

    v = [random.Random(5).randrange(t) for _ in range(n)]
    ct = tuple(up(x) for x in S.encrypt(S.slot_encode(v)))
    assert slots(ct) == v
    row0 = [(pow(3, k, 2 * n) - 1) // 2 for k in range(half)]
    row1 = [(2 * n - pow(3, k, 2 * n) - 1) // 2 for k in range(half)]
    for r in (1, 5, -1):
        g = pkg.galois_element(n, r)
        got = slots(rotate(ct, g))
        assert got == perm(v, g)
        assert [got[i] for i in row0] == [v[row0[(k + r) % half]] for k in range(half)]
        assert [got[i] for i in row1] == [v[row1[(k + r) % half]] for k in range(half)]
    got = slots(rotate(ct, 2 * n - 1))
    assert [got[i] for i in row0] == [v[i] for i in row1] and [got[i] for i in row1] == [v[i] for i in row0]
    g1, g2 = pkg.galois_element(n, 1), pkg.galois_element(n, 5)
    assert slots(rotate(rotate(ct, g1), g2)) == perm(v, g1 * g2 % (2 * n)) == slots(rotate(ct, pkg.galois_element(n, 6)))


# ------------------------------------------------------------------------------------------------ GPU: reserve covers both entry points
@pytest.mark.gpu
@pytest.mark.parametrize("n,spec,w,batch", [(8192, ("bits", 30, 4), 16, 1), (8192, ("bits", 30, 4), 16, 24), (4096, ("bits", 30, 4), 16, 300),
                                            (16384, ("bits", 40, 2), 20, 2), (2048, ("bits", 64, 2), 32, 2), (65536, ("bits", 30, 1), 16, 1),
                                            (32768, ("bits", 40, 1), 20, 2), (256, ("bits", 250, 1), 64, 2)])
@pytest.mark.parametrize("form", ["default", "composed"])
def test_reserve_covers_galois_entry_points(pkg, monkeypatch, n, spec, w, batch, form):
    """After fhe_rns_ntt_reserve(h, batch), automorphism and apply_galois of batch, batch/2 and 1 units grow no library workspace."""
    if form == "composed":
        monkeypatch.setenv("FHE_HIP_NO_FUSED_GALOIS", "1"); monkeypatch.setenv("FHE_HIP_NO_FUSED_KEYSWITCH", "1")
    moduli = _moduli(spec, n); L = len(moduli)
    e = pkg.RnsNttEngine(n, moduli)
    K = e.relin_num_digits(w)
    keys = [pkg.DeviceBuffer.from_numpy(k) for k in _random_keys(moduli, n, L * K, 400)]
    gk = e.import_relin_keys(w, keys, keys)
    e.reserve(batch)
    held = e.workspace_bytes()
    for nb in sorted({batch, 1, max(1, batch // 2)}):
        x = rns_poly(78, moduli, n, nb)
        d = [pkg.DeviceBuffer.from_numpy(x) for _ in range(2)]; o = [pkg.DeviceBuffer(x.nbytes) for _ in range(2)]
        e.automorphism(o[0], d[0], 3, nb)
        e.apply_galois(gk, 2 * n - 1, o[0], o[1], d[0], d[1], nb)
        assert e.workspace_bytes() == held, f"a call of {nb} units grew a workspace after reserve({batch})"
