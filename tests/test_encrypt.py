"""Public-key encryption as one engine call (fhe_public_key_create / fhe_ct_encrypt_reserve / fhe_ct_encrypt).

    out0[b][i] = pk0_i (*) u_b + [t e0_b]_{q_i} + m[b][i],      out1[b][i] = pk1_i (*) u_b + [t e1_b]_{q_i}

with u = ternary(seeds[0]), e0 / e1 = gaussian(sigma, seeds[1] / seeds[2]) at sampler index b n + x.  The expected value comes from the CPU
oracle alone: RnsPlan.sample_ternary, sample_gaussian and polymul, plus integer additions in numpy.  Every comparison is bit for bit."""
import concurrent.futures
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import memcheck
import ntt_math as nm
from test_hoisted import CSRC, HIPCC, RES_FIELDS, RES_FLAGS, _resource_remarks
from workload import rns_poly

NEW_SYMBOLS = ("fhe_public_key_create", "fhe_public_key_destroy", "fhe_ct_encrypt_reserve", "fhe_ct_encrypt")
T, SIGMA = 65537, 3.2
SEEDS = (0x1234567, 0x89ABCDEF01, 0xFEDCBA9876543)


# ------------------------------------------------------------------------------------------------ host maths
def _ints(a):
    """[...][4] containers -> Python integers (object array)."""
    a = np.ascontiguousarray(a)
    return sum(a[..., k].astype(object) << (64 * k) for k in range(4))


def _containers(v):
    out = np.zeros(v.shape + (4,), np.uint64)
    for k in range(4):
        out[..., k] = ((v >> (64 * k)) & ((1 << 64) - 1)).astype(np.uint64)
    return out


def _embed(small, moduli):
    """[batch][n] signed Python integers -> [batch][L][n] containers of canonical residues."""
    return _containers(np.stack([small % q for q in moduli], axis=1))


def _expected(oracle, n, moduli, t, sigma, seeds, pk0, pk1, m, batch):
    """The definition, from the oracle's samplers and polymul and integer additions; returns (out0, out1, u) as containers."""
    rp = oracle.RnsPlan(n, moduli)
    u = rp.sample_ternary(0.5, seeds[0], batch)
    outs = []
    for pk, seed, add in ((pk0, seeds[1], m), (pk1, seeds[2], None)):
        e = rp.sample_gaussian(sigma, seed, batch)
        prod = rp.polymul(u, np.ascontiguousarray(np.broadcast_to(pk[None], u.shape)), threads=8)
        out = np.empty_like(prod)
        for l, q in enumerate(moduli):
            if q < (1 << 31):                                             # t |e| and every sum stay far below 2^64
                ev = e[:, l, :, 0]; neg = ev > np.uint64(q // 2)
                k = np.where(neg, np.uint64(q) - ev, ev)
                te = (np.uint64(t % q) * k) % np.uint64(q)
                te = np.where(neg & (te != 0), np.uint64(q) - te, te)
                v = prod[:, l, :, 0] + te + (add[:, l, :, 0] if add is not None else np.uint64(0))
                out[:, l] = 0; out[:, l, :, 0] = v % np.uint64(q)
            else:
                ev = _ints(e[:, l]); signed = np.where(ev > q // 2, ev - q, ev)
                v = _ints(prod[:, l]) + (signed * t) % q + (_ints(add[:, l]) if add is not None else 0)
                out[:, l] = _containers(v % q)
        outs.append(out)
    return outs[0], outs[1], u


def _small_poly(rng, n, batch, bound):
    return np.array([[int(v) for v in rng.integers(-bound, bound + 1, n)] for _ in range(batch)], dtype=object)


def _keygen(oracle, n, moduli, t, seed):
    """s ternary, a uniform, e small: pk = (t e - a s, a).  Returns (s as signed integers [n], pk0, pk1 as [L][n] containers)."""
    rng = np.random.default_rng(seed)
    rp = oracle.RnsPlan(n, moduli)
    s = _small_poly(rng, n, 1, 1); e = _small_poly(rng, n, 1, 6)
    a = rns_poly(seed + 1, moduli, n, 1)
    a_s = _ints(rp.polymul(a, _embed(s, moduli), threads=8))
    pk0 = _containers(np.stack([(t * e[0] - a_s[0, l]) % q for l, q in enumerate(moduli)], axis=0))
    return s[0], pk0, a[0]


def _decrypt(oracle, n, moduli, t, s, c0, c1):
    """(centred c0 + c1 s mod Q) as Python integers [batch][n], by CRT."""
    rp = oracle.RnsPlan(n, moduli)
    sb = np.ascontiguousarray(np.broadcast_to(_embed(s[None], moduli), c1.shape))
    c1s = rp.polymul(np.ascontiguousarray(c1), sb, threads=8)
    Q = math.prod(moduli)
    tot = np.zeros(c0.shape[:1] + (n,), dtype=object)
    for l, q in enumerate(moduli):
        r = (_ints(c0[:, l]) + _ints(c1s[:, l])) % q
        Ml = Q // q
        tot = (tot + r * (Ml * pow(Ml, -1, q))) % Q
    return np.where(tot > Q // 2, tot - Q, tot)


# ------------------------------------------------------------------------------------------------ CPU
def test_exports_wrappers_and_rejection_without_device(pkg):
    lib = pkg.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    for method in ("import_public_key", "encrypt", "encrypt_reserve"):
        assert callable(getattr(pkg.RnsNttEngine, method)), method
    assert callable(pkg.capi.PublicKey)
    out = ctypes.c_void_p(0x1234)
    assert lib.fhe_public_key_create(None, ctypes.byref(out), None, None) == -1 and out.value == 0x1234
    assert lib.fhe_ct_encrypt_reserve(None, 3.2, 1) == -1
    seeds = (ctypes.c_uint64 * 3)(1, 2, 3)
    assert lib.fhe_ct_encrypt(None, None, 65537, 3.2, seeds, None, None, None, 1) == -1
    assert lib.fhe_public_key_destroy(None) == 0


def test_the_definition_decrypts_on_the_oracle(oracle):
    """n = 32, two 30-bit primes, t = 65537, sigma = 3.2, s ternary, pk = (t e - a s, a): c0 + c1 s = m + t (e u + e0 + e1 s), so its centred
    value is m modulo t and at most t B (2n + 1) + t in magnitude, B = ceil(12 sigma) (|u|, |s| <= 1, every error <= B)."""
    n, batch = 32, 3
    moduli = nm.ntt_primes(30, n, 2)
    s, pk0, pk1 = _keygen(oracle, n, moduli, T, 5)
    rng = np.random.default_rng(9)
    msg = np.array([[int(v) for v in rng.integers(0, T, n)] for _ in range(batch)], dtype=object)
    m = _embed(msg, moduli)
    c0, c1, _ = _expected(oracle, n, moduli, T, SIGMA, SEEDS, pk0, pk1, m, batch)
    v = _decrypt(oracle, n, moduli, T, s, c0, c1)
    B = math.ceil(12 * SIGMA)
    assert int(abs(v).max()) <= T * B * (2 * n + 1) + T
    assert np.array_equal(v % T, msg)


RES_SRC = """#include "lds_launch.h"
#include "encrypt.hip.h"
using namespace fhe_dev;
template __global__ void fhe_dev::ntt_encrypt_kernel<RES_FIELD, RES_LOGN, 2>(char*, char*, const char*, const RES_FIELD::E*, const RES_FIELD::E*, const uint64_t*, uint32_t,
    uint64_t, uint64_t, uint64_t, uint64_t, const Limb<RES_FIELD>*, uint32_t, uint32_t);
"""
TABLE_SRC = """#include <cstdio>
#include "lds_launch.h"
int main() {
    for (int eb : {4, 8}) for (int n = 11; n <= 15; n++) std::printf("%d %d %d\\n", eb, n, (int)fhe_dev::lds_encrypt(eb, n));
    return 0;
}
"""
# bytes of scratch per lane the 8-byte instances are allowed (compiled figures, rounded up: F52 600-668, F64 690-850, F64X up to 1060 at N = 2^14)
SCRATCH_8B = {"F52": 700, "F64": 920, "F64X": 1100}


def test_encrypt_kernels_stay_within_their_budgets(tmp_path):
    """Every LDS-resident instance of ntt_encrypt_kernel compiles for gfx950.  Those fhe_dev::lds_encrypt names keep the budgets: at most 256
    VGPRs and two waves per SIMD; 4-byte residues no scratch; 8-byte residues at most the pinned figure of their field (two live 64-register
    arrays and the packed samples around the transforms).  The instance it leaves out (4-byte residues at N = 2^15: 1024-thread workgroups
    cap a thread at 128 VGPRs) is compiled too and must MISS the budget: that is why it takes the composed path."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    (tmp_path / "table.hip").write_text(TABLE_SRC)
    res = subprocess.run([HIPCC, "-std=c++17", "-I", CSRC, "-o", str(tmp_path / "table"), str(tmp_path / "table.hip")], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    table = {}
    for line in subprocess.run([str(tmp_path / "table")], capture_output=True, text=True, timeout=60).stdout.splitlines():
        eb, n, enc = (int(x) for x in line.split())
        table[(eb, n)] = bool(enc)
    named = [(f, n) for f, (eb, sizes) in RES_FIELDS.items() for n in sizes if table[(eb, n)]]
    left_out = [(f, n) for f, (eb, sizes) in RES_FIELDS.items() for n in sizes if not table[(eb, n)]]
    assert left_out == [("F32", 15)] and len(named) == 16, (left_out, named)
    (tmp_path / "enc_res.hip").write_text(RES_SRC)
    jobs = [((f, n), [HIPCC, *RES_FLAGS, f"-DRES_FIELD={f}", f"-DRES_LOGN={n}", "-c", "-o", str(tmp_path / f"e_{f}_{n}.o"), str(tmp_path / "enc_res.hip")])
            for f, n in named + left_out]

    def run(job):
        res = subprocess.run(job[1], capture_output=True, text=True, timeout=1500)
        assert res.returncode == 0, res.stderr[-3000:]
        return job[0], _resource_remarks(res.stderr)

    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
        got = dict(ex.map(run, jobs))
    for (f, n) in named:
        ks = [r for k, r in got[(f, n)].items() if "ntt_encrypt_kernel" in k]
        assert len(ks) == 1, (f, n, list(got[(f, n)]))
        r = ks[0]
        print(f, n, r)
        assert r["vgprs"] <= 256 and r["occupancy"] >= 2, (f, n, r)
        assert r.get("scratch", 0) <= (0 if f == "F32" else SCRATCH_8B[f]), (f, n, r)
    for (f, n) in left_out:
        ks = [r for k, r in got[(f, n)].items() if "ntt_encrypt_kernel" in k]
        print("left out:", f, n, ks)
        assert len(ks) == 1 and ks[0].get("scratch", 0) > 0, (f, n, got[(f, n)])


# ------------------------------------------------------------------------------------------------ GPU
_cache = {}


def _case(oracle, n, moduli, batch, with_m=True):
    key = (n, tuple(moduli), batch, with_m)
    if key not in _cache:
        pk0, pk1 = rns_poly(31, moduli, n, 1)[0], rns_poly(32, moduli, n, 1)[0]
        m = rns_poly(33, moduli, n, batch) if with_m else None
        _cache[key] = (pk0, pk1, m) + _expected(oracle, n, moduli, T, SIGMA, SEEDS, pk0, pk1, m, batch)
    return _cache[key]


def _run(pkg, n, moduli, pk0, pk1, m, batch, seeds=SEEDS, reserve=False, twice=True, t=T, sigma=SIGMA, ws=None):
    """ws: a list that receives workspace_bytes() of the fresh engine before the first call (after the key import and the reserve) and after
    the last one: equal on the one-launch path, apart by at least the composed path's u (batch L n containers) otherwise."""
    e = pkg.RnsNttEngine(n, moduli)
    src = pkg.DeviceBuffer.from_numpy(pk0), pkg.DeviceBuffer.from_numpy(pk1)   # kept alive: an output at a source's address is rejected as aliasing
    pk = e.import_public_key(*src)
    if reserve:
        e.encrypt_reserve(sigma, batch)
    nbytes = batch * len(moduli) * n * 32
    dm = None if m is None else pkg.DeviceBuffer.from_numpy(m)
    o0, o1 = pkg.DeviceBuffer(nbytes), pkg.DeviceBuffer(nbytes)
    shape = (batch, len(moduli), n, 4)
    if ws is not None:
        ws.append(e.workspace_bytes())
    for _ in range(2 if twice else 1):
        memcheck.poison(pkg, o0); memcheck.poison(pkg, o1)
        e.encrypt(pk, t, sigma, seeds, o0, o1, dm, batch)
        got = o0.download(shape), o1.download(shape)
    if ws is not None:
        ws.append(e.workspace_bytes())
    if m is not None:
        assert np.array_equal(dm.download(shape), m)
    return got


def _primes(bits, n, count):
    return nm.largest_ntt_primes(bits, n, count) if bits == 64 else nm.ntt_primes(bits, n, count)


# (n, bits, L, batch): the word-sized classes at n = 2048, the largest LDS-resident size of the 4- and 8-byte residues, both grid forms (the
# planner's default threshold is 256 ciphertexts), and the composed paths: N = 2^15, the full-width class, a small ring
SHAPES = [(2048, 30, 2, 3), (2048, 40, 2, 2), (2048, 60, 2, 2), (2048, 64, 2, 2), (16384, 30, 2, 2), (16384, 60, 2, 2), (2048, 30, 2, 1), (2048, 30, 2, 256),
          (32768, 30, 1, 1), (2048, 250, 2, 1), (64, 30, 2, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,bits,L,batch", SHAPES)
def test_encrypt_matches_the_oracle(pkg, oracle, n, bits, L, batch):
    moduli = _primes(bits, n, L)
    pk0, pk1, m, w0, w1, _ = _case(oracle, n, moduli, batch)
    g0, g1 = _run(pkg, n, moduli, pk0, pk1, m, batch)
    assert np.array_equal(g0, w0) and np.array_equal(g1, w1)


@pytest.mark.gpu
def test_both_grid_forms_and_the_composed_path_give_the_same_bits(pkg, oracle, monkeypatch):
    """n = 2048, L = 2: batch 1 (one workgroup per limb) and batch 256 (one per ciphertext) agree on ciphertext 0; FHE_HIP_NO_FUSED_ENCRYPT=1 and
    a forced grid form equal the default bit for bit."""
    n, L = 2048, 2
    moduli = _primes(30, n, L)
    pk0, pk1, m, w0, w1, _ = _case(oracle, n, moduli, 256)
    one = _run(pkg, n, moduli, pk0, pk1, m[:1], 1, twice=False)
    assert np.array_equal(one[0][0], w0[0]) and np.array_equal(one[1][0], w1[0])
    for name, value in (("FHE_HIP_NO_FUSED_ENCRYPT", "1"), ("FHE_HIP_ENCRYPT_PER_CT_BATCH", "0"), ("FHE_HIP_ENCRYPT_PER_CT_BATCH", "100000")):
        with monkeypatch.context() as mp:
            mp.setenv(name, value)
            g0, g1 = _run(pkg, n, moduli, pk0, pk1, m[:3], 3, twice=False)
        assert np.array_equal(g0, w0[:3]) and np.array_equal(g1, w1[:3]), (name, value)


@pytest.mark.gpu
def test_null_message_seeds_and_stale_workspaces(pkg, oracle):
    n, L, batch = 2048, 2, 2
    moduli = _primes(30, n, L)
    pk0, pk1, m, w0, w1, u = _case(oracle, n, moduli, batch)
    z0, z1 = _run(pkg, n, moduli, pk0, pk1, None, batch)
    y0, y1 = _run(pkg, n, moduli, pk0, pk1, np.zeros_like(m), batch)
    assert np.array_equal(z0, y0) and np.array_equal(z1, y1) and np.array_equal(z1, w1) and not np.array_equal(z0, w0)
    # another u seed changes u, hence both components; another e0 seed changes out0 only
    a0, a1 = _run(pkg, n, moduli, pk0, pk1, m, batch, seeds=(SEEDS[0] + 1, SEEDS[1], SEEDS[2]), twice=False)
    assert not np.array_equal(a0, w0) and not np.array_equal(a1, w1)
    assert not np.array_equal(oracle.RnsPlan(n, moduli).sample_ternary(0.5, SEEDS[0] + 1, batch), u)
    b0, b1 = _run(pkg, n, moduli, pk0, pk1, m, batch, seeds=(SEEDS[0], SEEDS[1] + 1, SEEDS[2]), twice=False)
    assert not np.array_equal(b0, w0) and np.array_equal(b1, w1)
    # equal seeds after an unrelated multiply + relinearise on the same engine
    e = pkg.RnsNttEngine(n, moduli)
    src = pkg.DeviceBuffer.from_numpy(pk0), pkg.DeviceBuffer.from_numpy(pk1)
    pk = e.import_public_key(*src)
    w = 16; K = e.relin_num_digits(w)
    kb = [rns_poly(100 + i, moduli, n, 1)[0] for i in range(L * K)]; ka = [rns_poly(200 + i, moduli, n, 1)[0] for i in range(L * K)]
    rk = e.import_relin_keys(w, [pkg.DeviceBuffer.from_numpy(k) for k in kb], [pkg.DeviceBuffer.from_numpy(k) for k in ka])
    c = [pkg.DeviceBuffer.from_numpy(rns_poly(10 + i, moduli, n, batch)) for i in range(4)]
    dm = pkg.DeviceBuffer.from_numpy(m)
    o0, o1, r0, r1 = (pkg.DeviceBuffer(m.nbytes) for _ in range(4))
    e.encrypt(pk, T, SIGMA, SEEDS, o0, o1, dm, batch)
    assert np.array_equal(o0.download(m.shape), w0)
    e.ct_multiply_relin(rk, r0, r1, c[0], c[1], c[2], c[3], batch)
    memcheck.poison(pkg, o0); memcheck.poison(pkg, o1)
    e.encrypt(pk, T, SIGMA, SEEDS, o0, o1, dm, batch)
    assert np.array_equal(o0.download(m.shape), w0) and np.array_equal(o1.download(m.shape), w1)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["default", "composed"])
def test_guard_bands_rejections_and_reserve(pkg, oracle, monkeypatch, variant):
    """Both outputs inside guard bands, poisoned first: fully overwritten, guards intact, inputs read only.  Every rejected call leaves the
    poisoned outputs untouched.  After fhe_ct_encrypt_reserve a call does not change fhe_rns_ntt_workspace_bytes."""
    if variant == "composed":
        monkeypatch.setenv("FHE_HIP_NO_FUSED_ENCRYPT", "1")
    n, L, batch = 2048, 2, 2
    moduli = _primes(30, n, L)
    pk0, pk1, m, w0, w1, _ = _case(oracle, n, moduli, batch)
    S = L * n * 32
    e = pkg.RnsNttEngine(n, moduli); other = pkg.RnsNttEngine(n, moduli)
    arena = memcheck.GuardedArena(pkg, [("pk0", S), ("out0", batch * S), ("m", batch * S), ("out1", batch * S), ("pk1", S)], S)
    arena["pk0"].upload(pk0); arena["pk1"].upload(pk1); arena["m"].upload(m)
    pk = e.import_public_key(arena["pk0"], arena["pk1"])
    foreign = other.import_public_key(arena["pk0"], arena["pk1"])
    e.encrypt_reserve(SIGMA, batch)
    before = e.workspace_bytes()
    o0, o1 = arena["out0"].poison(), arena["out1"].poison()
    lib = pkg.lib(); P = pkg.capi._ptr
    seeds = (ctypes.c_uint64 * 3)(*SEEDS)
    q_min = min(moduli)

    def call(h=e.h, key=pk.h, t=T, sigma=SIGMA, sd=seeds, a=P(o0), b=P(o1), mm=P(arena["m"]), bt=batch):
        return lib.fhe_ct_encrypt(h, key, t, sigma, sd, a, b, mm, bt)

    bad = [call(h=None), call(key=None), call(sd=None), call(a=None), call(b=None), call(a=P(o0) + 8), call(mm=P(arena["m"]) + 8), call(b=P(o0)),
           call(a=P(arena["m"])), call(b=P(arena["pk0"])), call(a=P(arena["pk1"])), call(key=foreign.h), call(bt=0), call(t=1), call(t=0),
           call(sigma=0.0), call(sigma=-1.0), call(sigma=float("nan")), call(sigma=2e6), call(sigma=q_min / 12.0)]
    assert all(rc == -1 for rc in bad), bad
    arena.verify(inputs=("pk0", "pk1", "m"))
    assert memcheck.is_poison(o0.download((batch, L, n, 4))) and memcheck.is_poison(o1.download((batch, L, n, 4)))
    assert call() == 0
    arena.verify(inputs=("pk0", "pk1", "m"))
    assert np.array_equal(o0.download(w0.shape), w0) and np.array_equal(o1.download(w1.shape), w1)
    assert e.workspace_bytes() == before


@pytest.mark.gpu
def test_round_trip_decrypts_to_the_message(pkg, oracle):
    """A real key pair at n = 2048: the engine's ciphertexts decrypt to m under s with host maths (batch 2)."""
    n, L, batch = 2048, 2, 2
    moduli = _primes(30, n, L)
    s, pk0, pk1 = _keygen(oracle, n, moduli, T, 77)
    rng = np.random.default_rng(3)
    msg = np.array([[int(v) for v in rng.integers(0, T, n)] for _ in range(batch)], dtype=object)
    m = _embed(msg, moduli)
    c0, c1 = _run(pkg, n, moduli, pk0, pk1, m, batch, twice=False)
    v = _decrypt(oracle, n, moduli, T, s, c0, c1)
    assert int(abs(v).max()) <= T * math.ceil(12 * SIGMA) * (2 * n + 1) + T
    assert np.array_equal(v % T, msg)
