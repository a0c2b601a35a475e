"""Hoisted linear transform: fhe_linear_transform_create / _destroy / _reserve and fhe_ct_linear_transform_hoisted (include/fhe_hip.h).

    out = sum_t p_t * hoisted_rotation(ct, g_t)          (a keyless term: p_t * (c0, c1))

The expected value comes from what tests/ and oracle/ already offer: sum_t RnsPlan.polymul(p_t, hoisted_t) mod q with hoisted_t from the
identity of test_hoisted.py (_expected), bit for bit on the fused path (hoist_lincomb.hip.h) and on the composed one
(FHE_HIP_NO_FUSED_HOIST=1, N >= 2^15, the full-width class)."""
import concurrent.futures
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import memcheck
import ntt_math as nm
from test_galois import _galois_keys, _moduli, _random_keys, _toy
from test_hoisted import CSRC, HIPCC, RES_FIELDS, RES_FLAGS, _expected, _resource_remarks, _variant
from workload import rns_poly

NEW_SYMBOLS = ("fhe_linear_transform_create", "fhe_linear_transform_destroy", "fhe_linear_transform_reserve", "fhe_ct_linear_transform_hoisted")
MASK64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------ CPU
def test_exports_wrappers_and_rejection_without_device(pkg):
    lib = pkg.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    for method in ("linear_transform_create", "linear_transform_hoisted", "linear_transform_reserve"):
        assert callable(getattr(pkg.RnsNttEngine, method)), method
    assert callable(pkg.capi.LinearTransform)
    # a null handle is an invalid argument, never a crash, and a failed create leaves *out alone
    out = ctypes.c_void_p(0x1234)
    elts = (ctypes.c_uint32 * 1)(1); nul = (ctypes.c_void_p * 1)(None)
    assert lib.fhe_linear_transform_create(None, ctypes.byref(out), 16, elts, nul, nul, 1) == -1 and out.value == 0x1234
    assert lib.fhe_linear_transform_reserve(None, None, 1) == -1
    assert lib.fhe_ct_linear_transform_hoisted(None, None, None, None, None, None, 1) == -1
    assert lib.fhe_linear_transform_destroy(None) == 0


RES_SRC = """#include "lds_launch.h"
#include "hoist_lincomb.hip.h"
using namespace fhe_dev;
template __global__ void fhe_dev::ntt_hoist_fwd_kernel<RES_FIELD, RES_LOGN, 2>(RES_FIELD::E*, const char*, const char*, const Limb<RES_FIELD>*, uint32_t);
template __global__ void fhe_dev::ntt_hoist_lincomb_kernel<RES_FIELD, RES_LOGN, 2, lds_hoist_lincomb_split(sizeof(RES_FIELD::E))>(char*, char*, const RES_FIELD::E*,
    const RES_FIELD::E*, const RES_FIELD::E*, const LincombTerm*, uint32_t, const Limb<RES_FIELD>*, uint32_t, uint32_t);
"""
TABLE_SRC = """#include <cstdio>
#include "lds_launch.h"
int main() {
    for (int eb : {4, 8}) for (int n = 11; n <= 15; n++) std::printf("%d %d %d %d\\n", eb, n, (int)fhe_dev::lds_hoist_lincomb(eb, n), (int)fhe_dev::lds_hoist(eb, n));
    return 0;
}
"""


def test_lincomb_kernels_stay_within_their_budgets(tmp_path):
    """Every LDS-resident instance of the two kernels compiles for gfx950.  Those fhe_dev::lds_hoist_lincomb names keep the project's budgets:
    4-byte residues at most 256 VGPRs, at least two waves per SIMD and no scratch (five live 32-register arrays); 8-byte residues at most 256
    VGPRs, two waves per SIMD and at most 140 bytes of scratch per lane (one workgroup per output component: three live arrays).  The instance
    it leaves out (4-byte residues at N = 2^15: 1024-thread workgroups cap a thread at 128 VGPRs) is compiled too and must MISS the budget:
    that is why it takes the composed path.  The predicate never names an instance that has no hoist kernels."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    (tmp_path / "table.hip").write_text(TABLE_SRC)
    res = subprocess.run([HIPCC, "-std=c++17", "-I", CSRC, "-o", str(tmp_path / "table"), str(tmp_path / "table.hip")], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    table = {}
    for line in subprocess.run([str(tmp_path / "table")], capture_output=True, text=True, timeout=60).stdout.splitlines():
        eb, n, lin, hoist = (int(x) for x in line.split())
        table[(eb, n)] = bool(lin)
        assert not lin or hoist, (eb, n)
    named = [(f, n) for f, (eb, sizes) in RES_FIELDS.items() for n in sizes if table[(eb, n)]]
    left_out = [(f, n) for f, (eb, sizes) in RES_FIELDS.items() for n in sizes if not table[(eb, n)]]
    assert left_out == [("F32", 15)] and len(named) == 16, (left_out, named)
    (tmp_path / "lincomb_res.hip").write_text(RES_SRC)
    jobs = [((f, n), [HIPCC, *RES_FLAGS, f"-DRES_FIELD={f}", f"-DRES_LOGN={n}", "-c", "-o", str(tmp_path / f"l_{f}_{n}.o"), str(tmp_path / "lincomb_res.hip")])
            for f, n in named + left_out]

    def run(job):
        res = subprocess.run(job[1], capture_output=True, text=True, timeout=1500)
        assert res.returncode == 0, res.stderr[-3000:]
        return job[0], _resource_remarks(res.stderr)

    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
        got = dict(ex.map(run, jobs))
    for (f, n) in named:
        ks = {k: v for k, v in got[(f, n)].items() if "ntt_hoist_fwd_kernel" in k or "ntt_hoist_lincomb_kernel" in k}
        assert len(ks) == 2, (f, n, list(got[(f, n)]))
        for name, r in ks.items():
            print(f, n, name[:48], r)
            assert r["vgprs"] <= 256 and r["occupancy"] >= 2, (name, r)
            assert r.get("scratch", 0) <= (0 if f == "F32" else 140), (name, r)
    for (f, n) in left_out:
        lin = [r for k, r in got[(f, n)].items() if "ntt_hoist_lincomb_kernel" in k]
        print("left out:", f, n, got[(f, n)])
        assert len(lin) == 1 and lin[0].get("scratch", 0) > 0, (f, n, got[(f, n)])


# ------------------------------------------------------------------------------------------------ helpers
def _add_mod(a, b, moduli):
    """(a + b) mod q_l on [batch][L][n][4] containers of canonical residues."""
    out = np.zeros_like(a)
    for l, q in enumerate(moduli):
        if q < (1 << 64):
            x, y = a[:, l, :, 0], b[:, l, :, 0]
            s = x + y                                                     # wraps where x + y >= 2^64 (q above 2^63)
            out[:, l, :, 0] = np.where((s < x) | (s >= np.uint64(q)), s - np.uint64(q), s)
        else:
            fa, fb, fo = a[:, l].reshape(-1, 4), b[:, l].reshape(-1, 4), out[:, l].reshape(-1, 4)
            for r in range(fa.shape[0]):
                v = (sum(int(fa[r, k]) << (64 * k) for k in range(4)) + sum(int(fb[r, k]) << (64 * k) for k in range(4))) % q
                fo[r] = [(v >> (64 * k)) & MASK64 for k in range(4)]
            out[:, l] = fo.reshape(out[:, l].shape)
    return out


def _weighted_sum(oracle, n, moduli, w, c0, c1, terms, upto=None):
    """sum_t polymul(p_t, hoisted_t) mod q.  terms: (g, (kb, ka) or None, p) with p one [L][n] polynomial."""
    rp = oracle.RnsPlan(n, moduli)
    tot = None
    for g, keys, p in terms[:upto]:
        r = (c0, c1) if keys is None else _expected(oracle, n, moduli, w, c0, c1, keys[0], keys[1], g)
        pb = np.ascontiguousarray(np.broadcast_to(p[None], c0.shape))
        prod = [rp.polymul(pb, np.ascontiguousarray(x), threads=8) for x in r]
        tot = prod if tot is None else [_add_mod(tot[i], prod[i], moduli) for i in range(2)]
    return tot


def _import(pkg, e, w, keys):
    return e.import_relin_keys(w, [pkg.DeviceBuffer.from_numpy(k) for k in keys[0]], [pkg.DeviceBuffer.from_numpy(k) for k in keys[1]])


def _build(pkg, e, w, terms):
    """Device side of a term list: one imported key set per distinct host key pair, one device plaintext per term."""
    sets = {}
    for g, keys, p in terms:
        if keys is not None and id(keys) not in sets:
            sets[id(keys)] = _import(pkg, e, w, keys)
    plains = [pkg.DeviceBuffer.from_numpy(p) for _, _, p in terms]
    lt = e.linear_transform_create(w, [g for g, _, _ in terms], [None if k is None else sets[id(k)] for _, k, _ in terms], plains)
    return lt, sets


# ------------------------------------------------------------------------------------------------ GPU: bits against the CPU oracle
ORACLE_CASES = [(2048, ("bits", 30, 2), 16, 3, 5), (8192, ("bits", 30, 4), 16, 2, 5), (16384, ("bits", 30, 3), 30, 1, 3), (4096, ("bits", 40, 2), 20, 3, 5),
                (2048, ("bits", 60, 2), 32, 2, 5), (8192, ("bits", 64, 1), 32, 1, 3), (32768, ("bits", 30, 1), 16, 1, 3), (256, ("bits", 250, 1), 64, 2, 3)]
_oracle_cache = {}


def _oracle_terms(n, moduli, w, K, G, fused_shape):
    """Element 1 with a key, a keyless term, 2n - 1, a random odd element and that element again, with two key sets between them.  The G = 3
    rows cannot hold all five: they keep element 1 with a key, the keyless term (element 1 repeated) and a third term that is the random
    element where the shape runs the fused kernel (the general permutation) and 2n - 1 where it runs the composition."""
    L = len(moduli)
    A = (_random_keys(moduli, n, L * K, 700), _random_keys(moduli, n, L * K, 1300))
    B = (_random_keys(moduli, n, L * K, 2100), _random_keys(moduli, n, L * K, 2900))
    rnd = random.Random(n + w).randrange(3, 2 * n - 1) | 1
    elts = [(1, A), (1, None), (2 * n - 1, B), (rnd, A), (rnd, A)] if G == 5 else [(1, A), (1, None), (rnd, B) if fused_shape else (2 * n - 1, B)]
    return [(g, keys, rns_poly(500 + t, moduli, n, 1)[0]) for t, (g, keys) in enumerate(elts)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,spec,w,batch,G", ORACLE_CASES)
@pytest.mark.parametrize("variant", ["default", "composed"])
def test_linear_transform_matches_the_oracle(pkg, oracle, monkeypatch, n, spec, w, batch, G, variant):
    """Outputs poisoned first, the call made twice (the second reuses the workspaces), inputs read only.  The expected value is computed once
    per shape and shared by both variants."""
    _variant(monkeypatch, variant)
    moduli = _moduli(spec, n)
    e = pkg.RnsNttEngine(n, moduli)
    K = e.relin_num_digits(w)
    terms = _oracle_terms(n, moduli, w, K, G, fused_shape=n <= 16384 and spec[1] <= 64)
    c0, c1 = rns_poly(81, moduli, n, batch), rns_poly(82, moduli, n, batch)
    key = (n, str(spec), w, batch, G)
    if key not in _oracle_cache:
        _oracle_cache[key] = _weighted_sum(oracle, n, moduli, w, c0, c1, terms)
    want = _oracle_cache[key]
    lt, sets = _build(pkg, e, w, terms)
    d0, d1 = pkg.DeviceBuffer.from_numpy(c0), pkg.DeviceBuffer.from_numpy(c1)
    o0, o1 = pkg.DeviceBuffer(c0.nbytes), pkg.DeviceBuffer(c0.nbytes)
    e.hoist(w, d1, batch)
    for _ in range(2):
        memcheck.poison(pkg, o0); memcheck.poison(pkg, o1)
        e.linear_transform_hoisted(lt, o0, o1, d0, d1, batch)
        assert np.array_equal(o0.download(c0.shape), want[0])
        assert np.array_equal(o1.download(c0.shape), want[1])
    assert np.array_equal(d0.download(c0.shape), c0) and np.array_equal(d1.download(c0.shape), c1)


# ------------------------------------------------------------------------------------------------ GPU: many terms at the top of each range
@pytest.mark.gpu
@pytest.mark.parametrize("bits,w", [(30, 10), (43, 15), (62, 21), (64, 22)])
@pytest.mark.parametrize("variant", ["default", "composed"])
def test_many_terms_at_the_top_of_each_range(pkg, oracle, monkeypatch, bits, w, variant):
    """n = 2048, the two largest admissible primes below 2^bits, K = ceil(bits / w) = 3, G = 48 random odd elements with one shared key set,
    batch 2: where lazy accumulation over the terms would overflow.  Against the on-device composition apply_galois_hoisted +
    multiply_bcast + poly_add, and against the CPU oracle for the first three terms."""
    _variant(monkeypatch, variant)
    n, batch, G = 2048, 2, 48
    moduli = nm.largest_ntt_primes(bits, n, 2); L = 2
    e = pkg.RnsNttEngine(n, moduli)
    K = e.relin_num_digits(w)
    assert K >= 3
    keys = (_random_keys(moduli, n, L * K, 700), _random_keys(moduli, n, L * K, 1300))
    rng = random.Random(bits)
    terms = [(rng.randrange(1, 2 * n) | 1, keys, rns_poly(900 + t, moduli, n, 1)[0]) for t in range(G)]
    c0, c1 = rns_poly(81, moduli, n, batch), rns_poly(82, moduli, n, batch)
    d0, d1 = pkg.DeviceBuffer.from_numpy(c0), pkg.DeviceBuffer.from_numpy(c1)
    lt, sets = _build(pkg, e, w, terms)
    gk = sets[id(keys)]
    plains = [pkg.DeviceBuffer.from_numpy(p) for _, _, p in terms]
    e.hoist(w, d1, batch)
    o = [pkg.DeviceBuffer(c0.nbytes) for _ in range(2)]
    memcheck.poison(pkg, o[0]); memcheck.poison(pkg, o[1])
    e.linear_transform_hoisted(lt, o[0], o[1], d0, None, batch)           # no keyless term: c1 is not needed
    got = [x.download(c0.shape) for x in o]
    # the composition, folded on the device; its value after three terms is kept for the oracle
    acc = [pkg.DeviceBuffer(c0.nbytes) for _ in range(2)]; tmp = [pkg.DeviceBuffer(c0.nbytes) for _ in range(2)]
    first3 = None
    for t, (g, _, _) in enumerate(terms):
        dst = acc if t == 0 else tmp
        e.apply_galois_hoisted(gk, g, dst[0], dst[1], d0, batch)
        for i in range(2):
            e.multiply_bcast(dst[i], dst[i], plains[t], batch)
            if t:
                e.poly_add(acc[i], acc[i], tmp[i], batch)
        if t == 2:
            first3 = [x.download(c0.shape) for x in acc]
    ref = [x.download(c0.shape) for x in acc]
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    # three terms through the transform itself, against the CPU oracle (and against the composition's prefix)
    lt3, _ = _build(pkg, e, w, terms[:3])
    memcheck.poison(pkg, o[0]); memcheck.poison(pkg, o[1])
    e.linear_transform_hoisted(lt3, o[0], o[1], d0, None, batch)
    want = _weighted_sum(oracle, n, moduli, w, c0, c1, terms, upto=3)
    for i in range(2):
        g3 = o[i].download(c0.shape)
        assert np.array_equal(g3, want[i]) and np.array_equal(first3[i], want[i])


# ------------------------------------------------------------------------------------------------ GPU: state and rejection
@pytest.mark.gpu
@pytest.mark.parametrize("n,spec,w,batch", [(8192, ("bits", 30, 4), 16, 2), (256, ("bits", 250, 1), 64, 2)])
@pytest.mark.parametrize("variant", ["default", "composed"])
def test_linear_transform_state_guards_and_rejections(pkg, oracle, monkeypatch, n, spec, w, batch, variant):
    _variant(monkeypatch, variant)
    moduli = _moduli(spec, n); L = len(moduli)
    e = pkg.RnsNttEngine(n, moduli)
    other = pkg.RnsNttEngine(n, moduli)
    K = e.relin_num_digits(w)
    keys = (_random_keys(moduli, n, L * K, 700), _random_keys(moduli, n, L * K, 1300))
    g = pkg.galois_element(n, 1)
    terms = [(g, keys, rns_poly(500, moduli, n, 1)[0]), (1, None, rns_poly(501, moduli, n, 1)[0]), (2 * n - 1, keys, rns_poly(502, moduli, n, 1)[0])]
    unit = L * n * 32
    c0, c1, c1b = rns_poly(81, moduli, n, batch), rns_poly(82, moduli, n, batch), rns_poly(83, moduli, n, batch)
    ar = memcheck.GuardedArena(pkg, [("c0", c0.nbytes), ("c1", c1.nbytes), ("out0", c0.nbytes), ("out1", c0.nbytes)], unit)
    ar["c0"].upload(c0); ar["c1"].upload(c1)
    lt, sets = _build(pkg, e, w, terms)
    gk = sets[id(keys)]
    plains = [pkg.DeviceBuffer.from_numpy(p) for _, _, p in terms]

    def untouched():
        ar.verify(inputs=("c0", "c1"))
        assert memcheck.is_poison(ar["out0"].download(c0.shape)) and memcheck.is_poison(ar["out1"].download(c0.shape))

    def rejected(eng, obj, out0, out1, in0, in1, nb):
        ar["out0"].poison(); ar["out1"].poison()
        with pytest.raises(pkg.FheError) as ex:
            eng.linear_transform_hoisted(obj, out0, out1, in0, in1, nb)
        assert ex.value.code == -1, str(ex.value)
        untouched()

    def create_rejected(eng, w_, elts, ks, ps):
        ar["out0"].poison(); ar["out1"].poison()
        with pytest.raises(pkg.FheError) as ex:
            eng.linear_transform_create(w_, elts, ks, ps)
        assert ex.value.code == -1, str(ex.value)
        untouched()

    O0, O1, C0, C1 = ar["out0"], ar["out1"], ar["c0"], ar["c1"]
    # ---- create
    create_rejected(e, w, [], [], [])                                           # no terms
    cap = 4096                                                                  # FHE_LINEAR_TRANSFORM_MAX_TERMS
    create_rejected(e, w, [1] * (cap + 1), [gk] * (cap + 1), [plains[0]] * (cap + 1))
    for bad in (2, 2 * n, 2 * n + 1):
        create_rejected(e, w, [bad], [gk], [plains[0]])                         # even, or not below 2n
    create_rejected(e, w, [3], [None], [plains[0]])                             # no key with g != 1
    create_rejected(e, w, [1], [gk], [None])                                    # null plaintext
    both = [pkg.DeviceBuffer.from_numpy(k) for k in keys[0]]
    create_rejected(e, w, [3], [other.import_relin_keys(w, both, both)], [plains[0]])   # keys of another engine
    w2 = w // 2
    k2 = [pkg.DeviceBuffer.from_numpy(k) for k in _random_keys(moduli, n, L * e.relin_num_digits(w2), 90)]
    gk2 = e.import_relin_keys(w2, k2, k2)
    create_rejected(e, w, [3], [gk2], [plains[0]])                              # keys of another decomp_bits

    class Off:                                                                  # 8 bytes past a container boundary
        def __init__(self, s): self.s = s
        def data_ptr(self): return (self.s.data_ptr() if hasattr(self.s, "data_ptr") else self.s.ptr) + 8
    create_rejected(e, w, [1], [gk], [Off(plains[0])])

    class Null:                                                                 # a null object handle
        h = None
    # ---- apply
    rejected(e, lt, O0, O1, C0, C1, batch)                                      # no hoist on this engine yet
    e.hoist(w, C1, batch)
    rejected(e, Null, O0, O1, C0, C1, batch)
    rejected(e, lt, O0, O1, C0, C1, batch + 1)                                  # another batch
    lt2, _ = _build(pkg, e, w2, [(1, None, terms[1][2])])
    rejected(e, lt2, O0, O1, C0, C1, batch)                                     # another decomp_bits than the hoist's
    other.hoist(w, C1, batch)
    rejected(other, lt, O0, O1, C0, C1, batch)                                  # an object of another engine
    rejected(e, lt, O0, O1, C0, None, batch)                                    # a keyless term needs c1
    rejected(e, lt, 0, O1, C0, C1, batch); rejected(e, lt, O0, 0, C0, C1, batch); rejected(e, lt, O0, O1, 0, C1, batch)
    rejected(e, lt, O0, O0, C0, C1, batch)                                      # aliased outputs
    rejected(e, lt, C0, O1, C0, C1, batch); rejected(e, lt, O0, C1, C0, C1, batch)   # an output aliases an input
    rejected(e, lt, Off(O0), O1, C0, C1, batch); rejected(e, lt, O0, O1, Off(C0), C1, batch); rejected(e, lt, O0, O1, C0, Off(C1), batch)

    # ---- the object and the kept decomposition survive other work on the engine
    want = _weighted_sum(oracle, n, moduli, w, c0, c1, terms)
    x = [pkg.DeviceBuffer.from_numpy(rns_poly(60 + i, moduli, n, batch)) for i in range(4)]
    y = [pkg.DeviceBuffer(c0.nbytes) for _ in range(2)]
    e.ct_multiply_relin(gk, y[0], y[1], x[0], x[1], x[2], x[3], batch)
    e.apply_galois(gk, 2 * n - 1, y[0], y[1], x[0], x[1], batch)
    e.forward(x[2], batch)
    O0.poison(); O1.poison()
    e.linear_transform_hoisted(lt, O0, O1, C0, C1, batch)
    ar.verify(inputs=("c0", "c1"))
    assert np.array_equal(O0.download(c0.shape), want[0]) and np.array_equal(O1.download(c0.shape), want[1])
    # ---- a second hoist changes the result accordingly (c1 of the keyless term follows it)
    C1.upload(c1b)
    e.hoist(w, C1, batch)
    want_b = _weighted_sum(oracle, n, moduli, w, c0, c1b, terms)
    O0.poison(); O1.poison()
    e.linear_transform_hoisted(lt, O0, O1, C0, C1, batch)
    ar.verify(inputs=("c0", "c1"))
    assert np.array_equal(O0.download(c0.shape), want_b[0]) and np.array_equal(O1.download(c0.shape), want_b[1])
    assert not np.array_equal(want[1], want_b[1])
    ar.free()


@pytest.mark.gpu
@pytest.mark.parametrize("n,spec,w,batch", [(8192, ("bits", 30, 4), 16, 2), (256, ("bits", 250, 1), 64, 2)])
@pytest.mark.parametrize("variant", ["default", "composed"])
def test_reserve_covers_hoist_and_two_calls(pkg, monkeypatch, n, spec, w, batch, variant):
    _variant(monkeypatch, variant)
    moduli = _moduli(spec, n); L = len(moduli)
    e = pkg.RnsNttEngine(n, moduli)
    K = e.relin_num_digits(w)
    keys = (_random_keys(moduli, n, L * K, 400), _random_keys(moduli, n, L * K, 500))
    terms = [(3, keys, rns_poly(500, moduli, n, 1)[0]), (1, None, rns_poly(501, moduli, n, 1)[0])]
    lt, _ = _build(pkg, e, w, terms)
    e.linear_transform_reserve(lt, batch)
    held, hoisted = e.workspace_bytes(), e.hoist_bytes()
    assert held > 0 and hoisted > 0
    x = rns_poly(78, moduli, n, batch)
    d = [pkg.DeviceBuffer.from_numpy(x) for _ in range(2)]; o = [pkg.DeviceBuffer(x.nbytes) for _ in range(2)]
    e.hoist(w, d[1], batch)
    for _ in range(2):
        e.linear_transform_hoisted(lt, o[0], o[1], d[0], d[1], batch)
    pkg.lib().fhe_hip_sync()
    assert e.hoist_bytes() == hoisted and e.workspace_bytes() == held


# ------------------------------------------------------------------------------------------------ GPU: slots end to end
@pytest.mark.gpu
def test_linear_transform_moves_slots_end_to_end(pkg, oracle):
    """Encrypt slot_encode(v); diagonals slot_encode(d_t) for the steps (0, 1, 5, -1) (step 0: the keyless term), real Galois keys; decrypt:
    slot i holds sum_t d_t[i] * v[pi_{g_t}(i)] mod t, 2 pi_g(i) + 1 = g (2i + 1) mod 2n, which in the 3-power ordering of the rows that the
    header documents is sum_t d_t (.) rot(v, step_t)."""
    bgv_toy, S = _toy(pkg, oracle)
    n, t, w = S.n, S.t, 16
    half = n // 2
    e = pkg.RnsNttEngine(n, S.moduli)
    shape = (1, S.L, n, 4)

    def up(x):
        return pkg.DeviceBuffer.from_numpy(bgv_toy.to_limb_array(x))

    rng = random.Random(11)
    v = [rng.randrange(t) for _ in range(n)]
    steps = (0, 1, 5, -1)
    diags = [[rng.randrange(t) for _ in range(n)] for _ in steps]
    elts = [pkg.galois_element(n, r) for r in steps]
    assert elts[0] == 1
    ct = tuple(up(x) for x in S.encrypt(S.slot_encode(v)))
    key_sets = [None]
    for g in elts[1:]:
        kb, ka = _galois_keys(S, g, w)
        key_sets.append(e.import_relin_keys(w, [up(k) for k in kb], [up(k) for k in ka]))
    plains = [up(S.to_rns(S.slot_encode(d))) for d in diags]
    lt = e.linear_transform_create(w, elts, key_sets, plains)
    o0, o1 = pkg.DeviceBuffer(ct[0].nbytes), pkg.DeviceBuffer(ct[0].nbytes)
    e.hoist(w, ct[1], 1)
    e.linear_transform_hoisted(lt, o0, o1, ct[0], ct[1], 1)
    got = S.slot_decode(S.decrypt([bgv_toy.from_limb_array(x.download(shape)) for x in (o0, o1)]))

    def pi(g, i):
        return (g * (2 * i + 1) % (2 * n) - 1) // 2

    assert got == [sum(d[i] * v[pi(g, i)] for d, g in zip(diags, elts)) % t for i in range(n)]
    # the same statement in the rows' own ordering: position k of row 0 is slot (3^k - 1) / 2, and a step r reads position k + r
    row0 = [(pow(3, k, 2 * n) - 1) // 2 for k in range(half)]
    assert [got[row0[k]] for k in range(half)] == [sum(d[row0[k]] * v[row0[(k + r) % half]] for d, r in zip(diags, steps)) % t for k in range(half)]
