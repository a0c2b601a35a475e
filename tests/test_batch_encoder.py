"""The batch encoder on the device (fhe_batch_encoder_*, fhe_slots_encode, fhe_slots_decode, fhe_slots_decode_poly).

Expected values are Python integers: an O(n log n) negacyclic transform over Z_t written here on ntt_math.find_psi / bitrev, itself checked in
every case against the direct evaluation m(psi^e(i)) at 8 random slots.  With psi = find_psi(n, t) slot i has the exponent e(i): 2 i + 1 in the
natural order; 3^k mod 2n for k < n/2 and 2n minus that for n/2 + k in the row order.  Equality is exact everywhere."""
import concurrent.futures
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import memcheck
import ntt_math as nm
from test_hoisted import CSRC, HIPCC, RES_FIELDS, RES_FLAGS, _resource_remarks

NEW_SYMBOLS = ("fhe_batch_encoder_create", "fhe_batch_encoder_destroy", "fhe_batch_encoder_reserve", "fhe_batch_encoder_scratch_bytes",
               "fhe_batch_encoder_slot_table", "fhe_slots_encode", "fhe_slots_decode", "fhe_slots_decode_poly")
NATURAL, ROWS = 0, 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, BAD_MODULUS = -1, -5, -2


# ------------------------------------------------------------------------------------------------ the Python definition
def exponents(n, order):
    if order == NATURAL:
        return [2 * i + 1 for i in range(n)]
    e = [pow(3, k, 2 * n) for k in range(n // 2)]
    return e + [2 * n - x for x in e]


def _cyclic(a, omega, t):
    """Cyclic transform of length n with the root omega: out[k] = sum_j a[j] omega^(j k), iterative Cooley-Tukey on Python integers."""
    n = len(a)
    bits = n.bit_length() - 1
    a = [a[nm.bitrev(i, bits)] for i in range(n)]
    ln = 2
    while ln <= n:
        half, wl = ln // 2, pow(omega, n // ln, t)
        ws = [1] * half
        for j in range(1, half):
            ws[j] = ws[j - 1] * wl % t
        for i in range(0, n, ln):
            for j in range(half):
                u, v = a[i + j], a[i + j + half] * ws[j] % t
                a[i + j], a[i + j + half] = (u + v) % t, (u - v) % t
        ln *= 2
    return a


def evaluate(m, t, order):
    """values[i] = m(psi^e(i)) mod t."""
    n = len(m)
    psi = nm.find_psi(n, t)
    pw, tw = 1, []
    for c in m:
        tw.append(int(c) * pw % t); pw = pw * psi % t
    nat = _cyclic(tw, psi * psi % t, t)                      # nat[j] = m(psi^(2 j + 1))
    return [nat[(e - 1) // 2] for e in exponents(n, order)]


def interpolate(values, t, order):
    """The m of degree < n with m(psi^e(i)) = values[i]."""
    n = len(values)
    psi = nm.find_psi(n, t)
    ipsi, ninv = pow(psi, -1, t), pow(n, -1, t)
    nat = [0] * n
    for v, e in zip(values, exponents(n, order)):
        nat[(e - 1) // 2] = int(v)
    a = _cyclic(nat, ipsi * ipsi % t, t)
    pw, m = ninv, []
    for c in a:
        m.append(c * pw % t); pw = pw * ipsi % t
    return m


def _spot_check(m, values, t, order, seed):
    """The fast transform against Horner at 8 random slots."""
    n = len(m)
    psi, ex = nm.find_psi(n, t), exponents(n, order)
    for i in random.Random(seed).sample(range(n), 8):
        x, acc = pow(psi, ex[i], t), 0
        for c in reversed(m):
            acc = (acc * x + c) % t
        assert acc == values[i], (n, t, order, i)


_cases = {}


def _case(n, t, order, batch=3, seed=1):
    """(values [batch][n] uint64, polynomials as lists of Python integers), computed once."""
    key = (n, t, order, batch, seed)
    if key not in _cases:
        rng = random.Random(hash((n, t, order, seed)) & 0xFFFFFFFF)
        vals = [[rng.randrange(t) for _ in range(n)] for _ in range(batch)]
        ms = [interpolate(v, t, order) for v in vals]
        _spot_check(ms[0], vals[0], t, order, seed)
        _cases[key] = (np.array(vals, dtype=np.uint64), ms)
    return _cases[key]


def _containers(ms, moduli):
    """[batch][L][n] containers of m mod q_l."""
    out = np.zeros((len(ms), len(moduli), len(ms[0]), 4), dtype=np.uint64)
    for b, m in enumerate(ms):
        for l, q in enumerate(moduli):
            out[b, l, :, 0] = np.array([c % q for c in m], dtype=np.uint64)
    return out


def plaintext_moduli(n):
    """65537, the largest 30-bit, a 40-bit, a 60-bit and a 64-bit prime = 1 (mod 2n): every field of the kernels, F64X included."""
    return [65537, nm.largest_ntt_primes(30, n, 1)[0], nm.ntt_primes(40, n, 1)[0], nm.ntt_primes(60, n, 1)[0], nm.largest_ntt_primes(64, n, 1)[0]]


def _encode(pkg, e, enc, vals, check_input=True):
    batch, n = vals.shape
    dv = pkg.DeviceBuffer.from_numpy(vals)
    do = pkg.DeviceBuffer(batch * e.L * n * 32)
    memcheck.poison(pkg, do)
    enc.encode(do, dv, batch)
    got = do.download((batch, e.L, n, 4))
    if check_input:
        assert np.array_equal(dv.download((batch, n)), vals)
    return got


def _decode(pkg, enc, coeffs):
    batch, n = coeffs.shape
    dm = pkg.DeviceBuffer.from_numpy(coeffs)
    dv = pkg.DeviceBuffer(batch * n * 8)
    memcheck.poison(pkg, dv)
    enc.decode(dv, dm, batch)
    assert np.array_equal(dm.download((batch, n)), coeffs)
    return dv.download((batch, n))


def _engine(pkg, n, moduli):
    e = pkg.RnsNttEngine(n, moduli)
    e.L = len(moduli)
    return e


def _both_ways(pkg, n, moduli, t, order, batch=3):
    vals, ms = _case(n, t, order, batch)
    e = _engine(pkg, n, moduli)
    enc = pkg.capi.BatchEncoder(e, t, order)
    assert np.array_equal(_encode(pkg, e, enc, vals), _containers(ms, moduli)), ("encode", n, t, order)
    coeffs = np.array(ms, dtype=np.uint64)
    assert np.array_equal(_decode(pkg, enc, coeffs), vals), ("decode", n, t, order)
    return e, enc, vals, ms


# ------------------------------------------------------------------------------------------------ CPU
def test_exports_wrappers_and_rejection_without_device(pkg):
    lib = pkg.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    for method in ("reserve", "scratch_bytes", "encode", "decode", "decode_poly", "close"):
        assert callable(getattr(pkg.capi.BatchEncoder, method)), method
    out = ctypes.c_void_p(0x1234)
    assert lib.fhe_batch_encoder_create(None, ctypes.byref(out), 65537, 0) == INVALID and out.value == 0x1234
    assert lib.fhe_batch_encoder_create(None, None, 65537, 0) == INVALID
    assert lib.fhe_batch_encoder_destroy(None) == 0
    assert lib.fhe_batch_encoder_reserve(None, None, 1) == INVALID
    assert lib.fhe_slots_encode(None, None, None, None, 1) == INVALID
    assert lib.fhe_slots_decode(None, None, None, None, 1) == INVALID
    assert lib.fhe_slots_decode_poly(None, None, None, None, 1) == INVALID
    b = ctypes.c_uint64(7)
    assert lib.fhe_batch_encoder_scratch_bytes(None, ctypes.byref(b)) == INVALID and b.value == 7
    tab = (ctypes.c_uint32 * 16)()
    assert lib.fhe_batch_encoder_slot_table(16, 2, tab) == INVALID
    assert lib.fhe_batch_encoder_slot_table(12, 0, tab) == INVALID
    assert lib.fhe_batch_encoder_slot_table(16, 0, None) == INVALID
    # (FHE_ERR_NO_DEVICE is out of reach of these entry points: each needs an engine, which does not exist without a device; fhe_hip.h says so)


@pytest.mark.parametrize("n", [16, 2048])
def test_slot_tables_match_the_definition(pkg, n):
    """table[pos] is the slot whose exponent is 2 bitrev(pos) + 1, the point position pos of the NTT domain holds.  The row order is a
    permutation, sigma_3 moves exponent e to 3 e: slot k of a half to slot k + 1 (cyclically), and sigma_{2n-1} swaps the halves."""
    bits = n.bit_length() - 1
    t = 97 if n == 16 else 65537
    for order in (NATURAL, ROWS):
        tab = pkg.capi.slot_table(n, order)
        ex = exponents(n, order)
        vals, ms = _case(n, t, order, batch=1)                   # the Python transform the GPU tests compare with: evaluate inverts interpolate,
        assert evaluate(ms[0], t, order) == [int(v) for v in vals[0]]   # and the library's table is the order both use
        assert sorted(int(x) for x in tab) == list(range(n))
        for pos in range(n):
            assert ex[int(tab[pos])] == 2 * nm.bitrev(pos, bits) + 1, (order, pos)
    ex = exponents(n, ROWS)
    assert sorted(ex) == list(range(1, 2 * n, 2))
    slot_of = {e: i for i, e in enumerate(ex)}
    h = n // 2
    for i in range(n):
        j = slot_of[3 * ex[i] % (2 * n)]
        assert j == (i + 1) % h + (i // h) * h, i                 # the cyclic shift by one inside each half
        assert slot_of[(2 * n - 1) * ex[i] % (2 * n)] == (i + h) % n


RES_SRC = """#include "lds_launch.h"
#include "encode.hip.h"
using namespace fhe_dev;
template __global__ void fhe_dev::ntt_slots_encode_kernel<RES_FIELD, RES_LOGN>(char*, const uint64_t*, const uint32_t*, const fhe_host::ModT*, const Limb<RES_FIELD>*, uint32_t);
template __global__ void fhe_dev::ntt_slots_decode_kernel<RES_FIELD, RES_LOGN, false>(uint64_t*, const char*, const uint32_t*, const Limb<RES_FIELD>*, uint32_t);
template __global__ void fhe_dev::ntt_slots_decode_kernel<RES_FIELD, RES_LOGN, true>(uint64_t*, const char*, const uint32_t*, const Limb<RES_FIELD>*, uint32_t);
"""
TABLE_SRC = """#include <cstdio>
#include "lds_launch.h"
int main() {
    for (int eb : {4, 8}) for (int n = 11; n <= 15; n++) std::printf("%d %d %d\\n", eb, n, (int)fhe_dev::lds_slots(eb, n));
    return 0;
}
"""


def _pinned():
    """The bounds: (VGPRs, waves per SIMD) of every (field, log2 n, kernel) as the compiler gave them when the kernels were written."""
    path = os.path.join(ROOT, "tests", "golden", "batch_encoder_resources.txt")
    out = {}
    for line in open(path).read().splitlines():
        if line and not line.startswith("#"):
            f, n, kernel, vgprs, occ = line.split()
            out[(f, int(n), kernel)] = (int(vgprs), int(occ))
    return out


def _kernel_of(name):
    if "ntt_slots_encode_kernel" in name:
        return "encode"
    if "ntt_slots_decode_kernel" in name:
        return "decode_poly" if "Lb1E" in name else "decode"
    return None


def test_encoder_kernels_compile_without_scratch_and_keep_their_pinned_budgets(tmp_path):
    """fhe_dev::lds_slots is pinned for (4, 8) x (11..15); every instance it names -- four fields x N = 2^11 .. 2^14, three kernels each --
    compiles for gfx950 with no spill, no scratch and an LDS footprint equal to the exchange buffer (n + n / 32 residues).  VGPRs and waves per
    SIMD are BOUNDS: no more registers and no fewer waves than the compiler gave when the kernels were written
    (tests/golden/batch_encoder_resources.txt)."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    (tmp_path / "table.hip").write_text(TABLE_SRC)
    res = subprocess.run([HIPCC, "-std=c++17", "-I", CSRC, "-o", str(tmp_path / "table"), str(tmp_path / "table.hip")], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    table = {}
    for line in subprocess.run([str(tmp_path / "table")], capture_output=True, text=True, timeout=60).stdout.splitlines():
        eb, n, v = (int(x) for x in line.split())
        table[(eb, n)] = bool(v)
    assert table == {(eb, n): n <= 14 for eb in (4, 8) for n in range(11, 16)}, table
    named = [(f, n) for f, (eb, sizes) in RES_FIELDS.items() for n in sizes if table[(eb, n)]]
    assert len(named) == 16
    (tmp_path / "enc_res.hip").write_text(RES_SRC)
    jobs = [((f, n), [HIPCC, *RES_FLAGS, f"-DRES_FIELD={f}", f"-DRES_LOGN={n}", "-c", "-o", str(tmp_path / f"e_{f}_{n}.o"), str(tmp_path / "enc_res.hip")]) for f, n in named]

    def run(job):
        res = subprocess.run(job[1], capture_output=True, text=True, timeout=1500)
        assert res.returncode == 0, res.stderr[-3000:]
        lds = {}
        cur = None
        for line in res.stderr.splitlines():                     # _resource_remarks keeps no LDS size: read it beside it
            if "Function Name: " in line:
                cur = line.split("Function Name: ")[1].split()[0]
            elif "LDS Size [bytes/block]: " in line and cur:
                lds[cur] = int(line.split("LDS Size [bytes/block]: ")[1].split()[0])
        return job[0], (_resource_remarks(res.stderr), lds)

    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
        got = dict(ex.map(run, jobs))
    pinned = _pinned()
    seen = {}
    for (f, n) in named:
        remarks, lds = got[(f, n)]
        eb = RES_FIELDS[f][0]
        for name, r in remarks.items():
            k = _kernel_of(name)
            if k is None:
                continue
            print(f, n, k, r, lds[name])
            assert r.get("spill", 0) == 0 and r.get("scratch", 0) == 0, (f, n, k, r)
            assert lds[name] == ((1 << n) + (1 << n) // 32) * eb, (f, n, k, lds[name])
            seen[(f, n, k)] = (r["vgprs"], r["occupancy"])
    assert len(seen) == 48 and sorted(seen) == sorted(pinned), sorted(seen)
    worse = {k: (seen[k], pinned[k]) for k in seen if seen[k][0] > pinned[k][0] or seen[k][1] < pinned[k][1]}
    assert not worse, worse                                             # no more registers and no fewer waves than pinned


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("order", [NATURAL, ROWS])
@pytest.mark.parametrize("n", [2048, 4096, 8192, 16384])
def test_encode_and_decode_match_python_on_every_instance(pkg, n, order):
    """Every (field, N) instance of both kernels under a 2 x 30-bit engine: t = 65537 and the largest 30-bit prime run the 4-byte field, the
    40-bit one the floating-point field, the 60-bit and the 64-bit one the two 8-byte fields.  Every t but 65537 exceeds the engine's primes, so
    the stored residues are reduced."""
    moduli = nm.ntt_primes(30, n, 2)
    for t in plaintext_moduli(n):
        _both_ways(pkg, n, moduli, t, order)


@pytest.mark.gpu
def test_crafted_inputs(pkg):
    """All zero; the constant vector c, whose polynomial is c x^0; one unit slot, m[j] = n^-1 psi^(-e(i) j); every slot t - 1."""
    n, t = 2048, 65537
    moduli = nm.ntt_primes(30, n, 2)
    e = _engine(pkg, n, moduli)
    psi, ninv = nm.find_psi(n, t), pow(n, -1, t)
    for order in (NATURAL, ROWS):
        enc = pkg.capi.BatchEncoder(e, t, order)
        ex = exponents(n, order)
        c, i = 12345, 777
        vals = np.zeros((4, n), dtype=np.uint64)
        vals[1, :] = c
        vals[2, i] = 1
        vals[3, :] = t - 1
        w = pow(psi, -ex[i], t)
        unit, pw = [], ninv
        for _ in range(n):
            unit.append(pw); pw = pw * w % t
        ms = [[0] * n, [c] + [0] * (n - 1), unit, [t - 1] + [0] * (n - 1)]
        assert np.array_equal(_encode(pkg, e, enc, vals), _containers(ms, moduli)), order
        assert np.array_equal(_decode(pkg, enc, np.array(ms, dtype=np.uint64)), vals), order


@pytest.mark.gpu
def test_a_plaintext_modulus_above_the_primes_is_reduced_and_decode_poly_refuses(pkg):
    n = 2048
    moduli = nm.ntt_primes(30, n, 2)
    t = nm.ntt_primes(60, n, 1)[0]
    e, enc, vals, ms = _both_ways(pkg, n, moduli, t, NATURAL)
    assert any(c >= moduli[0] for c in ms[0])                          # the reduction had something to do
    dp = pkg.DeviceBuffer.from_numpy(_containers(ms, moduli))
    dv = pkg.DeviceBuffer(3 * n * 8)
    memcheck.poison(pkg, dv)
    assert pkg.lib().fhe_slots_decode_poly(e.h, enc.h, dv.ptr, dp.ptr, 3) == UNSUPPORTED
    assert memcheck.is_poison(dv.download((3, n)))


@pytest.mark.gpu
def test_a_full_width_target_gives_the_same_bits(pkg):
    """h only supplies L, the moduli and the stream: 2 x 120-bit primes take the same launch as word-sized ones."""
    n, t = 2048, 65537
    wide = nm.ntt_primes(120, n, 2)
    for order in (NATURAL, ROWS):
        e, enc, vals, ms = _both_ways(pkg, n, wide, t, order)
        assert e.width_class == pkg.WIDTH_256
        narrow = _engine(pkg, n, nm.ntt_primes(30, n, 2))
        got = _encode(pkg, narrow, pkg.capi.BatchEncoder(narrow, t, order), vals)
        assert np.array_equal(got, _containers(ms, wide))              # t below every prime: the containers hold m itself
        dp = pkg.DeviceBuffer.from_numpy(_containers(ms, wide))
        dv = pkg.DeviceBuffer(3 * n * 8)
        enc.decode_poly(dv, dp, 3)
        assert np.array_equal(dv.download((3, n)), vals)


@pytest.mark.gpu
@pytest.mark.parametrize("L,batch", [(1, 1), (6, 1), (1, 257), (6, 257)])
def test_limb_counts_and_batches(pkg, L, batch):
    n, t = 2048, 65537
    _both_ways(pkg, n, nm.ntt_primes(30, n, L), t, ROWS, batch)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [16, 64, 1024, 32768])
def test_sizes_that_take_the_composed_path(pkg, n):
    t = 65537
    moduli = nm.ntt_primes(30, n, 2)
    for order in (NATURAL, ROWS):
        e, enc, vals, ms = _both_ways(pkg, n, moduli, t, order, batch=2)
        assert enc.scratch_bytes() >= 2 * n * 32
        dp = pkg.DeviceBuffer.from_numpy(_containers(ms, moduli))
        dv = pkg.DeviceBuffer(2 * n * 8)
        enc.decode_poly(dv, dp, 2)
        assert np.array_equal(dv.download((2, n)), vals)


CHILD = """import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import importlib
import numpy as np
pkg = importlib.import_module("gpu-homomorphic-encryption_amd")
import ntt_math as nm
from test_batch_encoder import _case, _encode, _decode, _engine, plaintext_moduli
n = 2048
moduli = nm.ntt_primes(30, n, 2)
out = {{}}
for k, t in enumerate(plaintext_moduli(n)):
    for order in (0, 1):
        vals, ms = _case(n, t, order)
        e = _engine(pkg, n, moduli)
        enc = pkg.capi.BatchEncoder(e, t, order)
        out[f"e_{{k}}_{{order}}"] = _encode(pkg, e, enc, vals)
        out[f"d_{{k}}_{{order}}"] = _decode(pkg, enc, np.array(ms, dtype=np.uint64))
        assert enc.scratch_bytes() >= 3 * n * 32, enc.scratch_bytes()      # the composed path's container scratch
np.savez(sys.argv[1], **out)
"""


@pytest.mark.gpu
def test_the_composed_path_gives_the_same_bits(pkg, tmp_path):
    """FHE_HIP_NO_FUSED_ENCODE=1 in a child process (read when the encoder's engine is created) at N = 2048, every field, both orders: the same
    bits as the default path of this process, which are those of Python."""
    (tmp_path / "child.py").write_text(CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests")))
    env = dict(os.environ, FHE_HIP_NO_FUSED_ENCODE="1")
    res = subprocess.run([sys.executable, str(tmp_path / "child.py"), str(tmp_path / "out.npz")], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    got = np.load(tmp_path / "out.npz")
    n = 2048
    moduli = nm.ntt_primes(30, n, 2)
    e = _engine(pkg, n, moduli)
    for k, t in enumerate(plaintext_moduli(n)):
        for order in (NATURAL, ROWS):
            vals, ms = _case(n, t, order)
            enc = pkg.capi.BatchEncoder(e, t, order)
            assert enc.scratch_bytes() == 0
            assert np.array_equal(got[f"e_{k}_{order}"], _encode(pkg, e, enc, vals)), (t, order)
            assert np.array_equal(got[f"e_{k}_{order}"], _containers(ms, moduli)), (t, order)
            assert np.array_equal(got[f"d_{k}_{order}"], vals), (t, order)


@pytest.mark.gpu
def test_round_trips_and_decoding_in_place(pkg):
    n, t, batch = 2048, 65537, 3
    moduli = nm.ntt_primes(30, n, 2)
    e = _engine(pkg, n, moduli)
    for order in (NATURAL, ROWS):
        vals, ms = _case(n, t, order)
        enc = pkg.capi.BatchEncoder(e, t, order)
        dv = pkg.DeviceBuffer.from_numpy(vals)
        dp = pkg.DeviceBuffer(batch * 2 * n * 32)
        back = pkg.DeviceBuffer(batch * n * 8)
        enc.encode(dp, dv, batch)
        enc.decode_poly(back, dp, batch)
        assert np.array_equal(back.download((batch, n)), vals)
        dm = pkg.DeviceBuffer.from_numpy(np.array(ms, dtype=np.uint64))
        enc.decode(dm, dm, batch)                                       # in place
        assert np.array_equal(dm.download((batch, n)), vals)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2048, 8192])
def test_round_trip_through_encryption_and_decryption(pkg, oracle, n):
    """encode -> fhe_ct_encrypt -> fhe_ct_decrypt -> fhe_slots_decode returns the slot values, without leaving the device in between."""
    from test_encrypt import _embed, _keygen
    t, L, batch, sigma = 65537, 3, 2, 3.2
    moduli = nm.ntt_primes(30, n, L)
    s, pk0, pk1 = _keygen(oracle, n, moduli, t, 77)
    e = _engine(pkg, n, moduli)
    enc = pkg.capi.BatchEncoder(e, t, ROWS)
    vals, _ = _case(n, t, ROWS, batch)
    src = pkg.DeviceBuffer.from_numpy(pk0), pkg.DeviceBuffer.from_numpy(pk1)
    pk = e.import_public_key(*src)
    ds = pkg.DeviceBuffer.from_numpy(_embed(s[None], moduli)[0])
    sk = e.import_secret_key(ds)
    nbytes = batch * L * n * 32
    dm, o0, o1 = pkg.DeviceBuffer(nbytes), pkg.DeviceBuffer(nbytes), pkg.DeviceBuffer(nbytes)
    dv = pkg.DeviceBuffer.from_numpy(vals)
    out = pkg.DeviceBuffer(batch * n * 8)
    enc.encode(dm, dv, batch)
    e.encrypt(pk, t, sigma, (11, 22, 33), o0, o1, dm, batch)
    e.decrypt(sk, t, 1, out, None, [o0, o1], batch)
    enc.decode(out, out, batch)
    assert np.array_equal(out.download((batch, n)), vals)


@pytest.mark.gpu
def test_row_order_rotations(pkg):
    """Decoding sigma_3(m) in the row order is the left shift by one of both halves of decoding m; sigma_{2n-1} swaps the halves.  sigma_g is
    computed here, in Python, modulo t: m(x^g) mod (x^n + 1)."""
    n, t = 2048, 65537
    e = _engine(pkg, n, nm.ntt_primes(30, n, 2))
    enc = pkg.capi.BatchEncoder(e, t, ROWS)
    vals, ms = _case(n, t, ROWS, batch=1)
    m, v = ms[0], vals[0]

    def sigma(g):
        out = [0] * n
        for j, c in enumerate(m):
            k = j * g % (2 * n)
            out[k % n] = (t - c) % t if k >= n else c
        return out

    got = _decode(pkg, enc, np.array([sigma(3), sigma(2 * n - 1)], dtype=np.uint64))
    h = n // 2
    assert np.array_equal(got[0], np.concatenate([np.roll(v[:h], -1), np.roll(v[h:], -1)]))
    assert np.array_equal(got[1], np.concatenate([v[h:], v[:h]]))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["default", "composed"])
def test_guard_bands_rejections_and_reserve(pkg, variant):
    """Every buffer of a call between 0xA5 guards, outputs poisoned; rejected calls write nothing; after reserve neither the target's
    workspaces nor the encoder's scratch change across calls.  'composed' is N = 1024, the largest size below the fused range."""
    n = 2048 if variant == "default" else 1024
    t, L, batch = 65537, 3, 5
    moduli = nm.ntt_primes(30, n, L)
    e = _engine(pkg, n, moduli)
    other = _engine(pkg, n, moduli)
    lib = pkg.lib()
    for order in (NATURAL, ROWS):
        vals, ms = _case(n, t, order, batch)
        enc = pkg.capi.BatchEncoder(e, t, order)
        enc.reserve(batch)
        before = (e.workspace_bytes(), enc.scratch_bytes())
        assert (before[1] == 0) == (variant == "default")
        S = L * n * 32
        arena = memcheck.GuardedArena(pkg, [("values", batch * n * 8), ("poly", batch * S), ("back", batch * n * 8), ("back2", batch * n * 8)], S)
        arena["values"].upload(vals)
        for name in ("poly", "back", "back2"):
            arena[name].poison()
        P = lambda name: arena[name].ptr
        bad = [lib.fhe_slots_encode(None, enc.h, P("poly"), P("values"), batch), lib.fhe_slots_encode(e.h, None, P("poly"), P("values"), batch),
               lib.fhe_slots_encode(e.h, enc.h, None, P("values"), batch), lib.fhe_slots_encode(e.h, enc.h, P("poly"), None, batch),
               lib.fhe_slots_encode(other.h, enc.h, P("poly"), P("values"), batch), lib.fhe_slots_encode(e.h, enc.h, P("poly"), P("values"), 0),
               lib.fhe_slots_encode(e.h, enc.h, P("poly") + 8, P("values"), batch), lib.fhe_slots_encode(e.h, enc.h, P("poly"), P("values") + 4, batch),
               lib.fhe_slots_encode(e.h, enc.h, P("values"), P("values"), batch),
               lib.fhe_slots_decode(None, enc.h, P("back"), P("values"), batch), lib.fhe_slots_decode(e.h, None, P("back"), P("values"), batch),
               lib.fhe_slots_decode(e.h, enc.h, None, P("values"), batch), lib.fhe_slots_decode(e.h, enc.h, P("back"), None, batch),
               lib.fhe_slots_decode(other.h, enc.h, P("back"), P("values"), batch), lib.fhe_slots_decode(e.h, enc.h, P("back"), P("values"), 0),
               lib.fhe_slots_decode(e.h, enc.h, P("back") + 4, P("values"), batch), lib.fhe_slots_decode(e.h, enc.h, P("back"), P("values") + 4, batch),
               lib.fhe_slots_decode_poly(e.h, enc.h, P("back"), P("poly") + 8, batch), lib.fhe_slots_decode_poly(e.h, enc.h, None, P("poly"), batch),
               lib.fhe_slots_decode_poly(e.h, enc.h, P("back"), None, batch), lib.fhe_slots_decode_poly(other.h, enc.h, P("back"), P("poly"), batch),
               lib.fhe_batch_encoder_reserve(other.h, enc.h, batch), lib.fhe_batch_encoder_reserve(e.h, enc.h, 0)]
        assert bad == [INVALID] * len(bad), bad
        arena.verify(inputs=("values",))
        for name, shape in (("poly", (batch, L, n, 4)), ("back", (batch, n)), ("back2", (batch, n))):
            assert memcheck.is_poison(arena[name].download(shape)), name
        for _ in range(2):
            enc.encode(arena["poly"], arena["values"], batch)
            enc.decode_poly(arena["back"], arena["poly"], batch)
        arena.verify(inputs=("values",))
        assert np.array_equal(arena["poly"].download((batch, L, n, 4)), _containers(ms, moduli))
        assert np.array_equal(arena["back"].download((batch, n)), vals)
        arena["poly"].upload(_containers(ms, moduli))
        arena["back"].upload(np.array(ms, dtype=np.uint64))
        enc.decode(arena["back2"], arena["back"], batch)
        arena.verify(inputs=("values", "poly", "back"))
        assert np.array_equal(arena["back2"].download((batch, n)), vals)
        assert (e.workspace_bytes(), enc.scratch_bytes()) == before
        arena.free()


@pytest.mark.gpu
def test_creation_rejects_what_is_not_a_plaintext_modulus_for_slots(pkg):
    n = 2048
    e = _engine(pkg, n, nm.ntt_primes(30, n, 2))
    lib = pkg.lib()
    out = ctypes.c_void_p(0x1234)
    for t in (65536, 65539, 18433, 4097, 1, 0):                         # even; prime, not 1 mod n; prime, 1 mod n only; 17 * 241 = 1 mod 2n; trivial
        assert lib.fhe_batch_encoder_create(e.h, ctypes.byref(out), t, 0) == BAD_MODULUS and out.value == 0x1234, t
    for order in (2, -1):
        assert lib.fhe_batch_encoder_create(e.h, ctypes.byref(out), 65537, order) == INVALID and out.value == 0x1234
    assert lib.fhe_batch_encoder_create(e.h, None, 65537, 0) == INVALID
