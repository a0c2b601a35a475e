"""Memory behaviour of the C ABI: guard bands around every buffer, poisoned outputs, read-only inputs, stale library workspaces, pointer alignment.

The parity tests compare arithmetic; every operand there is its own zero-filled allocation, every output starts as zeros and almost every engine
is fresh.  Here (tests/memcheck.py) the buffers of a call are carved out of one allocation with 0xA5 guards between them, at 32-byte-aligned
starts that are never 256-byte aligned, pure outputs are poisoned with 0x5A bytes, and after the call the guards must be intact, the declared
inputs byte-identical to what was uploaded and the outputs bit-identical to the CPU oracle (whole arrays, np.array_equal).

Shapes: the smallest at which each kernel form exists (predicates of csrc/lds_launch.h, planners of csrc/transforms.hip).  Rows that differ from a
first guess, each checked against the planner:
  * key switch at N = 2^14, 1 x 30-bit: with w = 16 there is one digit pair (L K = 2), so the stand-alone key switch stays on LDS_PAIRED and only the
    external product takes LDS_PART_PAIRS; w = 8 (two digit pairs) is the row on which the key switch takes LDS_PART_PAIRS as well.
  * FP64 field at N = 2048: the stand-alone relinearisation (container c2) runs LDS_SPLIT, the compact-operand calls (multiply + relinearise, Galois,
    blind rotation) LDS_JOINT3; LDS_JOINT3 reading c2 as containers is reached on the lazy 64-bit field (its own row with FHE_HIP_NO_C2_COMPACTION=1).
  * FHE_HIP_CT_RELIN_CHUNKS: a chunk holds at least 1024 limb polynomials, so batch 3 is one chunk whatever the switch says; batch 1025 at
    N = 2048 x 2 limbs is the smallest call that is cut in two (513 + 512 ciphertexts).
  * bit_reverse and the ref_*_literal kernels take (n, batch), not a count: n stays tiny and batch takes the odd counts."""
import random

import numpy as np
import pytest

import ntt_math as nm
from memcheck import GuardedArena, POISON_BYTE, is_poison, poison
from workload import rns_poly

pytestmark = pytest.mark.gpu

WIDTH = {30: 1, 40: 3, 60: 2, 64: 5, 120: 4, 250: 4}          # bits of the row's primes -> fhe_width_class


@pytest.fixture(scope="module")
def eng(pkg):
    if pkg.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")
    return pkg


def _up(pkg, arr):
    return pkg.DeviceBuffer.from_numpy(arr)


_PRIMES, _REF = {}, {}


def _primes(bits, n, count, skip=0):
    key = (bits, n, count + skip)
    if key not in _PRIMES:
        _PRIMES[key] = nm.ntt_primes(bits, n, count + skip)
    return _PRIMES[key][skip:]


def _cached(key, make):
    """The oracle's answers for one shape, shared by the rows that run it in different kernel forms (consecutive in the tables)."""
    if key not in _REF:
        if len(_REF) >= 2:
            _REF.pop(next(iter(_REF)))
        _REF[key] = make()
    return _REF[key]


def _keys(moduli, n, count, seed):
    return [rns_poly(seed + 17 * i, moduli, n, 1)[0] for i in range(count)]


def _import(pkg, e, w, keys):
    return e.import_relin_keys(w, [_up(pkg, k) for k in keys[0]], [_up(pkg, k) for k in keys[1]])


def _env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def guarded(pkg, unit, bufs, call, want):
    """One call inside a guarded arena.  bufs: (name, role, array or byte count) in call order; roles: 'in' uploaded and read only, 'io' uploaded
    and overwritten, 'out' poisoned and written, 'keep' poisoned and to be found poisoned afterwards, 'scratch' poisoned, contents free.
    want: name -> expected array, compared whole."""
    size = lambda x: int(x) if isinstance(x, (int, np.integer)) else x.nbytes
    ar = GuardedArena(pkg, [(name, size(x)) for name, _, x in bufs], unit)
    try:
        for name, role, x in bufs:
            if role in ("in", "io"):
                ar[name].upload(x)
            else:
                ar[name].poison()
        call(ar)
        ar.verify(inputs=[name for name, role, _ in bufs if role == "in"])
        for name, role, x in bufs:
            if role == "keep":
                assert is_poison(ar[name].download((-1,), np.uint8)), f"{name}: the caller's buffer was to stay untouched"
        for name, arr in want.items():
            got = ar[name].download(arr.shape, arr.dtype)
            assert np.array_equal(got, arr), f"{name} differs from the oracle ({int((got != arr).any(axis=-1).sum())} of {arr.size // 4} containers)"
    finally:
        ar.free()


# ------------------------------------------------------------------------------------ the helper itself
def test_guard_check_detects_an_overrun(eng):
    """One byte past a carved buffer and, separately, one byte inside a declared input (both inside the arena's own allocation): verify fails
    and names the guard / the input.  Without this the rest of the file proves nothing."""
    lib = eng.lib()
    data = np.arange(3 * 1024, dtype=np.uint64)

    def arena():
        ar = GuardedArena(eng, [("first", data.nbytes), ("second", data.nbytes), ("third", 4 * 333)], 1024)
        ar["first"].upload(data); ar["second"].upload(data); ar["third"].poison()
        return ar
    ar = arena()
    assert ar.guard >= 64 << 10 and all(s.ptr % 32 == 0 and s.ptr % 256 for s in ar.slices.values())
    ar.verify(inputs=["first", "second"])                                  # clean
    assert np.array_equal(ar["first"].download(data.shape), data) and is_poison(ar["third"].download((-1,), np.uint8))
    assert lib.fhe_hip_memset(ar["first"].ptr + data.nbytes, 0x00, 1) == 0    # one byte past 'first'
    with pytest.raises(AssertionError, match=r"guard 1 \(after 'first', before 'second'.*first at \+0 .*last at \+0 "):
        ar.verify(inputs=["first", "second"])
    ar.free(); ar = arena()
    assert lib.fhe_hip_memset(ar["second"].ptr - 1, 0x00, 1) == 0             # one byte before 'second': the same guard, its last byte
    with pytest.raises(AssertionError, match=r"guard 1 .*\(1 bytes before the start of 'second'\)"):
        ar.verify()
    ar.free(); ar = arena()
    assert lib.fhe_hip_memset(ar["third"].ptr + 4 * 333, 0x5A, 1) == 0        # past the last buffer, with the poison byte
    with pytest.raises(AssertionError, match=r"guard 3 \(after 'third', before None"):
        ar.verify()
    ar.free(); ar = arena()
    assert lib.fhe_hip_memset(ar["second"].ptr + 777, 0xFF, 1) == 0           # inside a declared input
    with pytest.raises(AssertionError, match=r"input 'second' was modified: 1 bytes differ from the upload, first at byte 777"):
        ar.verify(inputs=["first", "second"])
    ar.verify(inputs=["first"])                                            # ... which an output may be
    ar.free()
    d = eng.DeviceBuffer(640); poison(eng, d)
    assert is_poison(d.download((-1,), np.uint8)) and POISON_BYTE == 0x5A


# ------------------------------------------------------------------------------------ transforms and products
T_ROWS = [
    # id, bits, L, n, batch, environment
    ("f32-n2048x2-b3-small16", 30, 2, 2048, 3, {}),
    ("f32-n2048x2-b3-one-launch", 30, 2, 2048, 3, {"FHE_HIP_SMALL_BATCH_POLYS": "0", "FHE_HIP_COOP_POLYS": "0"}),
    ("f32-n2048x2-b17-xcd-small16", 30, 2, 2048, 17, {}),
    ("f32-n2048x2-b17-xcd-one-launch", 30, 2, 2048, 17, {"FHE_HIP_SMALL_BATCH_POLYS": "0", "FHE_HIP_COOP_POLYS": "0"}),
    ("f32-n8192x1-b3-coop4", 30, 1, 8192, 3, {}),
    ("f32-n16384x1-b1-coop4", 30, 1, 16384, 1, {}),
    ("f32-n32768x1-b1-ct-two-launch", 30, 1, 32768, 1, {}),
    ("f32-n32768x1-b1-ct-three-launch", 30, 1, 32768, 1, {"FHE_HIP_NO_TWO_LAUNCH_CT": "1"}),
    ("f32-n65536x1-b2-two-pass", 30, 1, 65536, 2, {}),
    ("f52-n2048x2-b3-ct-two-launch", 40, 2, 2048, 3, {}),
    ("f52-n16384x1-b1-ct-two-launch", 40, 1, 16384, 1, {}),
    ("f52-n16384x1-b1-ct-three-launch", 40, 1, 16384, 1, {"FHE_HIP_NO_TWO_LAUNCH_CT": "1"}),
    ("f64-n2048x1-b3", 60, 1, 2048, 3, {}),
    ("f64x-n2048x1-b3", 64, 1, 2048, 3, {}),
    ("f64x-n32768x1-b1-two-pass", 64, 1, 32768, 1, {}),
    ("u256-n256x1-b3-general", 250, 1, 256, 3, {}),
    ("u256-n2048x1-b2-tiles", 250, 1, 2048, 2, {}),
    ("u256-n4096x2-b1-two-limb-tiles", 120, 2, 4096, 1, {}),
]


def _per_limb(fn, a, b, L):
    return np.stack([np.stack([fn(np.ascontiguousarray(a[bi, l]), np.ascontiguousarray(b[bi, l]), l) for l in range(L)]) for bi in range(a.shape[0])])


def _transform_ref(oracle, bits, L, n, batch):
    def make():
        moduli = _primes(bits, n, L)
        rp = oracle.RnsPlan(n, moduli)
        A, B, C, D = (rns_poly(s, moduli, n, batch) for s in (1, 2, 3, 4))
        one = np.ascontiguousarray(D[:1])
        return dict(moduli=moduli, A=A, B=B, C=C, D=D, one=one, fwd=rp.forward(A, threads=8), inv=rp.inverse(B, threads=8),
                    mul=rp.polymul(A, B, threads=8), sq=rp.polymul(A, A, threads=8),
                    bc=rp.polymul(A, np.ascontiguousarray(np.broadcast_to(one, A.shape)), threads=8),
                    pw=_per_limb(lambda x, y, l: rp.plans[l].pointwise(x, y), A, B, L),
                    add=_per_limb(lambda x, y, l: oracle.batch_add(x, y, moduli[l]), A, B, L),
                    sub=_per_limb(lambda x, y, l: oracle.batch_sub(x, y, moduli[l]), A, B, L),
                    ct=rp.ct_multiply(A, C, B, D, threads=8), ctsq=rp.ct_multiply(A, C, A, C, threads=8))
    return _cached(("transforms", bits, L, n, batch), make)


@pytest.mark.parametrize("row", T_ROWS, ids=[r[0] for r in T_ROWS])
def test_transforms_and_products_inside_guard_bands(eng, oracle, monkeypatch, row):
    _, bits, L, n, batch, env = row
    _env(monkeypatch, env)
    R = _transform_ref(oracle, bits, L, n, batch)
    e = eng.RnsNttEngine(n, R["moduli"])
    assert e.width_class == WIDTH[bits]
    A, B, C, D = R["A"], R["B"], R["C"], R["D"]
    unit, nb = L * n * 32, A.nbytes
    G = lambda bufs, call, want: guarded(eng, unit, bufs, call, want)
    G([("data", "io", A)], lambda m: e.forward(m["data"], batch), {"data": R["fwd"]})
    G([("data", "io", B)], lambda m: e.inverse(m["data"], batch), {"data": R["inv"]})
    rab = [("r", "out", nb), ("a", "in", A), ("b", "in", B)]
    G(rab, lambda m: e.pointwise(m["r"], m["a"], m["b"], batch), {"r": R["pw"]})
    G(rab, lambda m: e.multiply(m["r"], m["a"], m["b"], batch), {"r": R["mul"]})
    G([("a", "io", A), ("b", "in", B)], lambda m: e.multiply(m["a"], m["a"], m["b"], batch), {"a": R["mul"]})
    G([("a", "in", A), ("b", "io", B)], lambda m: e.multiply(m["b"], m["a"], m["b"], batch), {"b": R["mul"]})
    G([("r", "out", nb), ("a", "in", A)], lambda m: e.multiply(m["r"], m["a"], m["a"], batch), {"r": R["sq"]})
    G([("a", "io", A)], lambda m: e.multiply(m["a"], m["a"], m["a"], batch), {"a": R["sq"]})
    G([("r", "out", nb), ("a", "in", A), ("one", "in", R["one"])], lambda m: e.multiply_bcast(m["r"], m["a"], m["one"], batch), {"r": R["bc"]})
    G([("a", "io", A), ("one", "in", R["one"])], lambda m: e.multiply_bcast(m["a"], m["a"], m["one"], batch), {"a": R["bc"]})
    G(rab, lambda m: e.poly_add(m["r"], m["a"], m["b"], batch), {"r": R["add"]})
    G(rab, lambda m: e.poly_sub(m["r"], m["a"], m["b"], batch), {"r": R["sub"]})
    outs = [("c0", "out", nb), ("c1", "out", nb), ("c2", "out", nb)]
    G(outs + [("a0", "in", A), ("a1", "in", C), ("b0", "in", B), ("b1", "in", D)],
      lambda m: e.ct_multiply(m["c0"], m["c1"], m["c2"], m["a0"], m["a1"], m["b0"], m["b1"], batch), dict(zip(("c0", "c1", "c2"), R["ct"])))
    G(outs + [("a0", "in", A), ("a1", "in", C)],
      lambda m: e.ct_multiply(m["c0"], m["c1"], m["c2"], m["a0"], m["a1"], m["a0"], m["a1"], batch), dict(zip(("c0", "c1", "c2"), R["ctsq"])))


# ------------------------------------------------------------------------------------ key switching
K_ROWS = [
    # id, bits, L, n, w, batch, environment, blind rotation keeps the accumulators compact (the caller's scratch pair stays untouched)
    ("f32-n2048x2-w16-b3-parts16", 30, 2, 2048, 16, 3, {}, True),
    ("f32-n2048x2-w16-b3-paired", 30, 2, 2048, 16, 3, {"FHE_HIP_SPLIT_PAIRS_POLYS": "0"}, True),
    ("f32-n2048x2-w16-b3-single-lds-tw", 30, 2, 2048, 16, 3, {"FHE_HIP_NO_PAIRED_TRANSFORMS": "1"}, False),
    ("f32-n2048x2-w16-b3-single-l2-tw", 30, 2, 2048, 16, 3, {"FHE_HIP_NO_PAIRED_TRANSFORMS": "1", "FHE_HIP_NO_LDS_TWIDDLES": "1"}, False),
    ("f32-n2048x2-w16-b17-paired-xcd", 30, 2, 2048, 16, 17, {"FHE_HIP_SPLIT_PAIRS_POLYS": "0"}, True),
    ("f32-n16384x1-w16-b1-part-pairs-extprod", 30, 1, 16384, 16, 1, {}, True),
    ("f32-n16384x1-w8-b1-part-pairs", 30, 1, 16384, 8, 1, {}, True),
    ("f32-n32768x1-w16-b1-joint3", 30, 1, 32768, 16, 1, {}, True),
    ("f52-n2048x2-w20-b3-joint3", 40, 2, 2048, 20, 3, {}, True),
    ("f52-n2048x2-w20-b3-split", 40, 2, 2048, 20, 3, {"FHE_HIP_SPLIT_KEYSWITCH": "1"}, False),
    ("f52-n2048x2-w20-b3-no-c2-compaction", 40, 2, 2048, 20, 3, {"FHE_HIP_NO_C2_COMPACTION": "1"}, True),
    ("f64-n2048x1-w32-b2-joint3", 60, 1, 2048, 32, 2, {}, True),
    ("f64-n2048x1-w32-b2-joint3-container-c2", 60, 1, 2048, 32, 2, {"FHE_HIP_NO_C2_COMPACTION": "1"}, True),
    ("f64x-n2048x1-w32-b2-split", 64, 1, 2048, 32, 2, {}, False),
    ("f64x-n4096x1-w32-b2-joint3", 64, 1, 4096, 32, 2, {}, True),
    ("u256-n256x1-w64-b2-general", 250, 1, 256, 64, 2, {}, False),
]


def _sigma(a, moduli, g):
    """sigma_g: out[j] = in[i] for i = j g^-1 mod 2n < n, else q - in[i - n] (0 stays 0)."""
    n = a.shape[2]
    i = (np.arange(n, dtype=np.int64) * pow(g, -1, 2 * n)) % (2 * n)
    neg = i >= n
    out = np.ascontiguousarray(a[:, :, i % n, :])
    for l, q in enumerate(moduli):
        if q < 1 << 64:
            v = out[:, l, :, 0]
            out[:, l, :, 0] = np.where(neg[None, :] & (v != 0), np.uint64(q) - v, v)
        else:
            from oracle import pyoracle
            for b in range(a.shape[0]):
                vals = pyoracle.from_limbs(out[b, l])
                out[b, l] = pyoracle.to_limbs([(q - v) % q if s else v for v, s in zip(vals, neg)])
    return out


def _shifts(n, steps, batch):
    edge = [1, n, 2 * n - 1, n - 1, 0, n + 1, 5, n + 77, 2 * n - 2]
    return np.array([[edge[(3 * s + b) % len(edge)] for b in range(batch)] for s in range(steps)], dtype=np.uint32)


def _keyswitch_ref(oracle, bits, L, n, w, batch, g):
    def make():
        moduli = _primes(bits, n, L)
        rp = oracle.RnsPlan(n, moduli); K = rp.num_digits(w)
        sets = [(_keys(moduli, n, L * K, 1000 * s + 100), _keys(moduli, n, L * K, 1000 * s + 600)) for s in range(3)]
        c0, c1, c2, b0, b1 = (rns_poly(s, moduli, n, batch) for s in (51, 52, 53, 54, 55))
        t0, t1, t2 = rp.ct_multiply(c0, c1, b0, b1, threads=8)
        sh = _shifts(n, 3, batch)
        chain, acc = [], (c0, c1)
        for s in range(3):                                                 # step s: rows of component 0 from set s, of component 1 from set s + 1
            acc = rp.blind_rotate_step(w, acc[0], acc[1], sh[s], sets[s], sets[(s + 1) % 3], threads=8)
            chain.append(acc)
        return dict(moduli=moduli, K=K, sets=sets, ops=(c0, c1, c2, b0, b1), sh=sh, chain=chain,
                    relin=rp.relinearize(w, c0, c1, c2, sets[0][0], sets[0][1], threads=8),
                    ctr=rp.relinearize(w, t0, t1, t2, sets[0][0], sets[0][1], threads=8),
                    sigma={x: _sigma(c0, moduli, x) for x in (g, 2 * n - 1)},
                    galois={x: rp.relinearize(w, _sigma(c0, moduli, x), np.zeros_like(c0), _sigma(c1, moduli, x), sets[1][0], sets[1][1], threads=8) for x in (g, 2 * n - 1)},
                    mono=rp.monomial_mul_sub(c2, sh[0]))
    return _cached(("keyswitch", bits, L, n, w, batch), make)


@pytest.mark.parametrize("row", K_ROWS, ids=[r[0] for r in K_ROWS])
def test_key_switching_inside_guard_bands(eng, oracle, monkeypatch, row):
    _, bits, L, n, w, batch, env, compact = row
    _env(monkeypatch, env)
    g = eng.galois_element(n, 5)
    R = _keyswitch_ref(oracle, bits, L, n, w, batch, g)
    e = eng.RnsNttEngine(n, R["moduli"])
    assert e.width_class == WIDTH[bits] and e.relin_num_digits(w) == R["K"]
    ks = [_import(eng, e, w, s) for s in R["sets"]]
    c0, c1, c2, b0, b1 = R["ops"]
    unit, nb = L * n * 32, c0.nbytes
    G = lambda bufs, call, want: guarded(eng, unit, bufs, call, want)
    G([("c0", "io", c0), ("c1", "io", c1), ("c2", "in", c2)], lambda m: e.relinearize(ks[0], m["c0"], m["c1"], m["c2"], batch),
      dict(zip(("c0", "c1"), R["relin"])))
    G([("o0", "out", nb), ("o1", "out", nb), ("a0", "in", c0), ("a1", "in", c1), ("b0", "in", b0), ("b1", "in", b1)],
      lambda m: e.ct_multiply_relin(ks[0], m["o0"], m["o1"], m["a0"], m["a1"], m["b0"], m["b1"], batch), dict(zip(("o0", "o1"), R["ctr"])))
    for x in (g, 2 * n - 1):
        G([("out", "out", nb), ("in", "in", c0)], lambda m: e.automorphism(m["out"], m["in"], x, batch), {"out": R["sigma"][x]})
        G([("o0", "out", nb), ("o1", "out", nb), ("c0", "in", c0), ("c1", "in", c1)],
          lambda m: e.apply_galois(ks[1], x, m["o0"], m["o1"], m["c0"], m["c1"], batch), dict(zip(("o0", "o1"), R["galois"][x])))
    sh = R["sh"]
    G([("out", "out", nb), ("in", "in", c2), ("shifts", "in", sh[0])], lambda m: e.monomial_mul_sub(m["out"], m["in"], m["shifts"], batch), {"out": R["mono"]})
    tmp = "keep" if compact else "scratch"
    for steps in (2, 3):                                                   # even and odd ping-pong
        G([("acc0", "io", c0), ("acc1", "io", c1), ("shifts", "in", np.ascontiguousarray(sh[:steps])), ("tmp0", tmp, nb), ("tmp1", tmp, nb)],
          lambda m: e.blind_rotate([ks[s] for s in range(steps)], [ks[(s + 1) % 3] for s in range(steps)], m["acc0"], m["acc1"], m["shifts"], m["tmp0"], m["tmp1"], batch),
          dict(zip(("acc0", "acc1"), R["chain"][steps - 1])))
    G([("acc0", "io", c0), ("acc1", "io", c1), ("shifts", "in", sh[0]), ("tmp0", tmp, nb), ("tmp1", tmp, nb)],
      lambda m: e.blind_rotate_step(ks[0], ks[1], m["acc0"], m["acc1"], m["shifts"], m["tmp0"], m["tmp1"], batch), dict(zip(("acc0", "acc1"), R["chain"][0])))


def _ctr_call(eng, e, rk, ops, want, L, n, batch):
    nb = ops[0].nbytes
    guarded(eng, L * n * 32, [("o0", "out", nb), ("o1", "out", nb), ("a0", "in", ops[0]), ("a1", "in", ops[1]), ("b0", "in", ops[2]), ("b1", "in", ops[3])],
            lambda m: e.ct_multiply_relin(rk, m["o0"], m["o1"], m["a0"], m["a1"], m["b0"], m["b1"], batch), dict(zip(("o0", "o1"), want)))


@pytest.mark.parametrize("chunks", ["1", "4"])
def test_ct_multiply_relin_chunk_switch_at_batch_3(eng, oracle, monkeypatch, chunks):
    """FHE_HIP_CT_RELIN_CHUNKS = 1 and 4 at a batch the chunk count does not divide (one chunk either way at this size: see the module docstring)."""
    monkeypatch.setenv("FHE_HIP_CT_RELIN_CHUNKS", chunks)
    bits, L, n, w, batch = 30, 2, 2048, 16, 3
    R = _keyswitch_ref(oracle, bits, L, n, w, batch, eng.galois_element(n, 5))
    e = eng.RnsNttEngine(n, R["moduli"])
    c0, c1, _, b0, b1 = R["ops"]
    _ctr_call(eng, e, _import(eng, e, w, R["sets"][0]), (c0, c1, b0, b1), R["ctr"], L, n, batch)


def test_ct_multiply_relin_cut_into_two_chunks(eng, oracle):
    """Batch 1025 at N = 2048, 2 x 30-bit: 2050 limb polynomials, the smallest call the two-stream pipeline cuts (513 + 512 ciphertexts, the
    second chunk's slices of the operands, of the compact workspace and of the outputs start at an odd ciphertext)."""
    bits, L, n, w, batch = 30, 2, 2048, 16, 1025
    moduli = _primes(bits, n, L)
    rp = oracle.RnsPlan(n, moduli); K = rp.num_digits(w)
    keys = (_keys(moduli, n, L * K, 100), _keys(moduli, n, L * K, 600))
    ops = tuple(rns_poly(s, moduli, n, batch) for s in (71, 72, 73, 74))
    t0, t1, t2 = rp.ct_multiply(*ops, threads=8)
    want = rp.relinearize(w, t0, t1, t2, keys[0], keys[1], threads=8)
    e = eng.RnsNttEngine(n, moduli)
    _ctr_call(eng, e, _import(eng, e, w, keys), ops, want, L, n, batch)


# ------------------------------------------------------------------------------------ streaming entry points
def _product(moduli):
    Q = 1
    for q in moduli:
        Q *= q
    return Q


def _random_containers(seed, count, top_bits=64):
    """[count][4] uniform 256-bit values, the top word cut to top_bits bits."""
    a = np.random.default_rng(seed).integers(0, 1 << 64, size=(count, 4), dtype=np.uint64)
    if top_bits < 64:
        a[:, 3] >>= np.uint64(64 - top_bits)
    return a


@pytest.mark.parametrize("word", [True, False], ids=["word-conversions", "container-conversions"])
@pytest.mark.parametrize("n,bits,L", [(1024, 30, 3), (1024, 60, 2), (64, 120, 2), (2048, 30, 3), (2048, 60, 2)],
                         ids=["n1024-3x30", "n1024-2x60", "n64-2x120", "n2048-3x30", "n2048-2x60"])
def test_rns_conversions_inside_guard_bands(eng, oracle, monkeypatch, n, bits, L, word):
    """to_rns, from_rns, rescale_drop_last and fast_base_convert at batch 3.  Rings below 2^11 take the container class whatever the primes; the
    n = 2048 rows are the same bases on the word-sized classes, where FHE_HIP_NO_WORD_CONVERSIONS chooses between two sets of kernels."""
    if not word:
        monkeypatch.setenv("FHE_HIP_NO_WORD_CONVERSIONS", "1")
    batch = 3
    src, dst = _primes(bits, n, L), _primes(bits, n, 2, skip=L)
    assert _product(src) < 1 << 255
    e, t = eng.RnsNttEngine(n, src), eng.RnsNttEngine(n, dst)
    S, D = oracle.RnsPlan(n, src), oracle.RnsPlan(n, dst)
    unit = L * n * 32
    V = _random_containers(n + bits, batch * n).reshape(batch, n, 4)
    X = rns_poly(91, src, n, batch)
    G = lambda bufs, call, want: guarded(eng, unit, bufs, call, want)
    G([("rns", "out", X.nbytes), ("values", "in", V)], lambda m: e.to_rns(m["rns"], m["values"], batch), {"rns": S.to_rns(V)})
    G([("values", "out", V.nbytes), ("rns", "in", X)], lambda m: e.from_rns(m["values"], m["rns"], batch), {"values": S.from_rns(X)})
    G([("out", "out", batch * (L - 1) * n * 32), ("in", "in", X)], lambda m: e.rescale_drop_last(m["out"], m["in"], batch), {"out": S.rescale_drop_last(X)})
    G([("out", "out", batch * 2 * n * 32), ("in", "in", X)], lambda m: e.fast_base_convert(t, m["out"], m["in"], batch), {"out": S.fast_base_convert(D, X)})


def test_rns_conversions_of_a_ringless_base_inside_guard_bands(eng, oracle):
    """fhe_rns_base_create, count 333: buffers [count][L] (a unit is L containers); expected values from Python integers."""
    src, dst = [12289, 40961, (1 << 61) - 1, (1 << 127) - 1], [65537, (1 << 89) - 1]
    e, t = eng.RnsNttEngine(None, src), eng.RnsNttEngine(None, dst)
    count, L, Q = 333, len(src), _product(src)
    rng = random.Random(12)
    vals = [0, 1, Q - 1] + [rng.randrange(Q) for _ in range(count - 3)]
    wide = [rng.getrandbits(256) for _ in range(count)]
    lim = lambda xs, shape: oracle.to_limbs(xs).reshape(shape)
    X = lim([v % q for v in vals for q in src], (count, L, 4))
    G = lambda bufs, call, want: guarded(eng, L * 32, bufs, call, want)
    G([("rns", "out", X.nbytes), ("values", "in", lim(wide, (count, 4)))], lambda m: e.to_rns(m["rns"], m["values"], count),
      {"rns": lim([v % q for v in wide for q in src], (count, L, 4))})
    G([("values", "out", count * 32), ("rns", "in", X)], lambda m: e.from_rns(m["values"], m["rns"], count), {"values": lim(vals, (count, 4))})
    ql = src[-1]
    G([("out", "out", count * (L - 1) * 32), ("in", "in", X)], lambda m: e.rescale_drop_last(m["out"], m["in"], count),
      {"out": lim([((v + ql // 2) // ql) % q for v in vals for q in src[:-1]], (count, L - 1, 4))})
    conv = [sum((v % q) * pow(Q // q, -1, q) % q * (Q // q) for q in src) for v in vals]
    G([("out", "out", count * len(dst) * 32), ("in", "in", X)], lambda m: e.fast_base_convert(t, m["out"], m["in"], count),
      {"out": lim([c % p for c in conv for p in dst], (count, len(dst), 4))})


def test_rns_samplers_inside_guard_bands(eng, oracle):
    n, L, batch = 2048, 2, 3
    moduli = _primes(30, n, L)
    e = eng.RnsNttEngine(n, moduli); rp = oracle.RnsPlan(n, moduli)
    nb = batch * L * n * 32
    G = lambda call, want: guarded(eng, L * n * 32, [("out", "out", nb)], call, {"out": want})
    G(lambda m: e.sample_ternary(m["out"], 0.5, 1234, batch), rp.sample_ternary(0.5, 1234, batch))
    G(lambda m: e.sample_gaussian(m["out"], 3.2, 99, batch), rp.sample_gaussian(3.2, 99, batch))
    G(lambda m: e.sample_uniform(m["out"], 2024, batch), rp.sample_uniform(2024, batch))


@pytest.mark.parametrize("count", [1, 333, 4097])
def test_count_driven_literal_kernels_inside_guard_bands(eng, oracle, count):
    """One thread per container, grids rounded up to 256-thread blocks: counts that are no multiple of the block size.  Guards: 64 KiB (a unit is one container)."""
    q = (1 << 254) + 79
    inv0 = oracle.mont_inverse(q)
    A, B = _random_containers(count, count, 61), _random_containers(count + 1, count, 61)          # below 2^253 < q
    A[0] = oracle.to_limbs([q - 1])[0]
    G = lambda bufs, call, want: guarded(eng, 32, bufs, call, want)
    rab = [("r", "out", A.nbytes), ("a", "in", A), ("b", "in", B)]
    G(rab, lambda m: eng.u256_add_mod(m["r"], m["a"], m["b"], q, count), {"r": oracle.batch_add(A, B, q)})
    G(rab, lambda m: eng.u256_sub_mod(m["r"], m["a"], m["b"], q, count), {"r": oracle.batch_sub(A, B, q)})
    G(rab, lambda m: eng.u256_mont_mul(m["r"], m["a"], m["b"], q, inv0, count), {"r": oracle.batch_mont(A, B, q, inv0)})
    s = 0x1234567 * q // 0x7654321
    G([("r", "out", A.nbytes), ("a", "in", A)], lambda m: eng.u256_mont_mul_scalar(m["r"], m["a"], s, q, inv0, count),
      {"r": oracle.batch_mont(A, oracle.to_limbs([s] * count), q, inv0)})
    for qs in ((1 << 64) - 59, (1 << 200) + 12289):
        G([("out", "out", A.nbytes)], lambda m: eng.sample_uniform_lcg(m["out"], qs, 846930886, count), {"out": oracle.sample_uniform_lcg(qs, 846930886, count)})
        G([("out", "out", A.nbytes)], lambda m: eng.sample_gaussian_placeholder(m["out"], qs, 846930886, count),
          {"out": oracle.sample_gaussian_placeholder(qs, 846930886, count)})
    G([("r", "out", A.nbytes), ("a", "in", A)], lambda m: eng.poly_mod_switch(m["r"], m["a"], q, 65537, count), {"r": oracle.poly_mod_switch(A, q, 65537)})
    F = np.ascontiguousarray(np.concatenate([A, B]))                       # negacyclic fold of 2 * count coefficients: the upper half stays
    G([("data", "io", F)], lambda m: eng.negacyclic_reduce(m["data"], q, count), {"data": oracle.negacyclic_reduce(F, q)})


@pytest.mark.parametrize("n,batch", [(8, 1), (4, 333), (16, 257), (4, 1025)])
def test_batch_driven_literal_kernels_inside_guard_bands(eng, oracle, n, batch):
    """bit_reverse (one thread per container of [batch][n]), the reference's transform kernels as written (one workgroup per polynomial) and its
    Stockham stage (one thread per butterfly): batch * n = 8, 1332, 4112 and 4100 containers."""
    q = nm.ntt_primes(60, 4096, 1)[0]
    inv0 = oracle.mont_inverse(q)
    rng = np.random.default_rng(n * batch)
    cont = lambda count: oracle.small_to_limbs(rng.integers(0, q, size=count, dtype=np.uint64))
    X, tw = cont(batch * n), cont(n)
    polys = lambda fn, src: np.concatenate([fn(np.ascontiguousarray(src[b * n:(b + 1) * n])) for b in range(batch)])
    G = lambda bufs, call, want: guarded(eng, n * 32, bufs, call, want)
    bits = n.bit_length() - 1
    perm = np.array([nm.bitrev(i, bits) for i in range(n)])
    G([("data", "io", X)], lambda m: eng.bit_reverse(m["data"], n, batch), {"data": np.ascontiguousarray(X.reshape(batch, n, 4)[:, perm]).reshape(-1, 4)})
    dt = [("data", "io", X), ("table", "in", tw)]
    G(dt, lambda m: eng.ref_forward_kernel_literal(m["data"], m["table"], q, inv0, n, batch), {"data": polys(lambda p: oracle.ref_forward_kernel(p, tw, q), X)})
    n_inv = int(tw[0, 0]) | 1
    G(dt, lambda m: eng.ref_inverse_kernel_literal(m["data"], m["table"], q, inv0, n_inv, n, batch),
      {"data": polys(lambda p: oracle.ref_inverse_kernel(p, tw, q, n_inv), X)})
    for stage in range(bits):
        G([("out", "out", X.nbytes), ("in", "in", X), ("table", "in", tw)],
          lambda m: eng.ref_stockham_stage_literal(m["out"], m["in"], m["table"], q, inv0, n, stage, batch),
          {"out": polys(lambda p: oracle.ref_stockham_stage(p, tw, q, stage), X)})


# ------------------------------------------------------------------------------------ stale library state
def _poisoned(pkg, nbytes):
    d = pkg.DeviceBuffer(nbytes); poison(pkg, d); return d


def _same(buf, want, what):
    assert np.array_equal(buf.download(want.shape), want), what


@pytest.mark.parametrize("bits,ws,env", [(30, (16, 30), {}), (30, (16, 30), {"FHE_HIP_SPLIT_PAIRS_POLYS": "0"}), (40, (20, 40), {})],
                         ids=["2x30-w16-w30-default", "2x30-w16-w30-paired", "2x40-w20-w40"])
def test_mixed_digit_widths_on_one_engine(eng, oracle, monkeypatch, bits, ws, env):
    """Key sets of different digit counts K on one engine and one stream: relinearize with A, B, A, then the one-call multiply with B, A.  A
    partial-sum workspace laid out for one K and summed with the other, or sized for the first, shows as a mismatch."""
    _env(monkeypatch, env)
    n, L, batch = 2048, 2, 3

    def make():
        moduli = _primes(bits, n, L)
        rp = oracle.RnsPlan(n, moduli)
        keys = {w: (_keys(moduli, n, L * rp.num_digits(w), 100 + w), _keys(moduli, n, L * rp.num_digits(w), 600 + w)) for w in ws}
        c0, c1, c2, b0, b1 = (rns_poly(s, moduli, n, batch) for s in (31, 32, 33, 34, 35))
        t = rp.ct_multiply(c0, c1, b0, b1, threads=8)
        return moduli, keys, (c0, c1, c2, b0, b1), {w: rp.relinearize(w, c0, c1, c2, *keys[w], threads=8) for w in ws}, {w: rp.relinearize(w, *t, *keys[w], threads=8) for w in ws}
    moduli, keys, (c0, c1, c2, b0, b1), relin, ctr = _cached(("mixed", bits), make)
    e = eng.RnsNttEngine(n, moduli)
    rk = {w: _import(eng, e, w, keys[w]) for w in ws}
    assert rk[ws[0]].h and e.relin_num_digits(ws[0]) != e.relin_num_digits(ws[1])
    d2, da = _up(eng, c2), [_up(eng, x) for x in (c0, c1, b0, b1)]
    for i, w in enumerate((ws[0], ws[1], ws[0])):
        d0, d1 = _up(eng, c0), _up(eng, c1)
        e.relinearize(rk[w], d0, d1, d2, batch)
        _same(d0, relin[w][0], ("relinearize", i, w, 0)); _same(d1, relin[w][1], ("relinearize", i, w, 1))
    for i, w in enumerate((ws[1], ws[0])):
        o0, o1 = _poisoned(eng, c0.nbytes), _poisoned(eng, c0.nbytes)
        e.ct_multiply_relin(rk[w], o0, o1, *da, batch)
        _same(o0, ctr[w][0], ("ct_multiply_relin", i, w, 0)); _same(o1, ctr[w][1], ("ct_multiply_relin", i, w, 1))
    _same(d2, c2, "c2 is read only")
    for buf, src in zip(da, (c0, c1, b0, b1)):
        _same(buf, src, "operands are read only")


BR_ENGINES = [("f32-n2048x2-parts16", 30, 2, 2048, {}), ("f32-n2048x2-paired", 30, 2, 2048, {"FHE_HIP_SPLIT_PAIRS_POLYS": "0"}),
              ("f52-n2048x2-joint3", 40, 2, 2048, {}), ("f32-n16384x1-part-pairs", 30, 1, 16384, {}),
              ("f32-n2048x2-composed", 30, 2, 2048, {"FHE_HIP_NO_FUSED_BLIND_ROTATE": "1"})]


@pytest.mark.parametrize("ws", [(8, 16, 8), (16, 8, 16)], ids=["w8-16-8", "w16-8-16"])
@pytest.mark.parametrize("row", BR_ENGINES, ids=[r[0] for r in BR_ENGINES])
def test_mixed_digit_widths_inside_one_blind_rotation_loop(eng, oracle, monkeypatch, row, ws):
    """The loop plans once with the largest K of its row sets and launches every step with that step's own K: the partial sums of a step must be
    laid out and summed with the step's K.  Expected: the oracle's single steps chained, each with its own digit width."""
    _, bits, L, n, env = row
    _env(monkeypatch, env)
    batch, steps = 2, 3

    def make():
        moduli = _primes(bits, n, L)
        rp = oracle.RnsPlan(n, moduli)
        rows = {w: [(_keys(moduli, n, L * rp.num_digits(w), 2000 + 100 * c + w), _keys(moduli, n, L * rp.num_digits(w), 3000 + 100 * c + w)) for c in range(2)] for w in (8, 16)}
        a0, a1 = rns_poly(41, moduli, n, batch), rns_poly(42, moduli, n, batch)
        sh = _shifts(n, steps, batch)
        want = {}
        for order in ((8, 16, 8), (16, 8, 16)):
            acc = (a0, a1)
            for s, w in enumerate(order):
                acc = rp.blind_rotate_step(w, acc[0], acc[1], sh[s], rows[w][0], rows[w][1], threads=8)
            want[order] = acc
        return moduli, rows, a0, a1, sh, want
    moduli, rows, a0, a1, sh, want = _cached(("mixed-br", bits, L, n), make)
    e = eng.RnsNttEngine(n, moduli)
    imp = {w: [_import(eng, e, w, r) for r in rows[w]] for w in (8, 16)}
    dA0, dA1 = _up(eng, a0), _up(eng, a1)
    e.blind_rotate([imp[w][0] for w in ws], [imp[w][1] for w in ws], dA0, dA1, _up(eng, sh), _poisoned(eng, a0.nbytes), _poisoned(eng, a0.nbytes), batch)
    _same(dA0, want[ws][0], "acc0"); _same(dA1, want[ws][1], "acc1")


@pytest.mark.parametrize("reserve", [True, False], ids=["reserved", "grown-on-demand"])
def test_large_then_small_then_other_forms_on_one_engine(eng, oracle, reserve):
    """N = 8192, 4 x 30-bit, w = 16.  The one-call multiply at batch 24 (96 limb polynomials: the throughput forms) dirties the workspaces; batch 1
    then runs the four-workgroup tensor product and the per-digit key switch on them, batch 5 the forms in between; then a product, a rotation and a
    blind-rotation loop.  Every result against the oracle, with and without fhe_rns_ntt_reserve(24) after the key import."""
    n, L, w = 8192, 4, 16

    def make():
        moduli = _primes(30, n, L)
        rp = oracle.RnsPlan(n, moduli); K = rp.num_digits(w)
        sets = [(_keys(moduli, n, L * K, 1000 * s + 100), _keys(moduli, n, L * K, 1000 * s + 600)) for s in range(2)]
        ops = [rns_poly(s, moduli, n, 24) for s in (61, 62, 63, 64)]
        cut = lambda b: [np.ascontiguousarray(x[:b]) for x in ops]
        ctr = {b: rp.relinearize(w, *rp.ct_multiply(*cut(b), threads=8), *sets[0], threads=8) for b in (24, 1, 5)}
        a, b = cut(2)[:2]
        g = 3
        c0, c1 = cut(3)[:2]
        gal = rp.relinearize(w, _sigma(c0, moduli, g), np.zeros_like(c0), _sigma(c1, moduli, g), *sets[1], threads=8)
        sh = _shifts(n, 2, 2)
        br = rp.blind_rotate(w, a, b, sh, [sets[0], sets[1]], [sets[1], sets[0]], threads=8)
        return moduli, sets, ops, ctr, rp.polymul(a, b, threads=8), g, gal, sh, br
    moduli, sets, ops, ctr, mul, g, gal, sh, br = _cached(("large-small",), make)
    e = eng.RnsNttEngine(n, moduli)
    ks = [_import(eng, e, w, s) for s in sets]
    if reserve:
        e.reserve(24)
        held = e.workspace_bytes()
    cut = lambda b: [np.ascontiguousarray(x[:b]) for x in ops]
    for batch in (24, 1, 5):
        host = cut(batch); d = [_up(eng, x) for x in host]
        o0, o1 = _poisoned(eng, host[0].nbytes), _poisoned(eng, host[0].nbytes)
        e.ct_multiply_relin(ks[0], o0, o1, *d, batch)
        _same(o0, ctr[batch][0], ("ct_multiply_relin", batch, 0)); _same(o1, ctr[batch][1], ("ct_multiply_relin", batch, 1))
        for buf, src in zip(d, host):
            _same(buf, src, ("operands are read only", batch))
    a, b = cut(2)[:2]
    dA, dB, dR = _up(eng, a), _up(eng, b), _poisoned(eng, a.nbytes)
    e.multiply(dR, dA, dB, 2); _same(dR, mul, "multiply")
    c0, c1 = cut(3)[:2]
    d0, d1, o0, o1 = _up(eng, c0), _up(eng, c1), _poisoned(eng, c0.nbytes), _poisoned(eng, c0.nbytes)
    e.apply_galois(ks[1], g, o0, o1, d0, d1, 3)
    _same(o0, gal[0], "apply_galois 0"); _same(o1, gal[1], "apply_galois 1"); _same(d0, c0, "c0 is read only"); _same(d1, c1, "c1 is read only")
    t0, t1 = _poisoned(eng, a.nbytes), _poisoned(eng, a.nbytes)
    e.blind_rotate([ks[0], ks[1]], [ks[1], ks[0]], dA, dB, _up(eng, sh), t0, t1, 2)
    _same(dA, br[0], "blind_rotate 0"); _same(dB, br[1], "blind_rotate 1")
    assert is_poison(t0.download((-1,), np.uint8)) and is_poison(t1.download((-1,), np.uint8))       # compact loop: the caller's scratch pair is not touched
    if reserve:
        assert e.workspace_bytes() == held                                 # nothing grew after the reservation


def test_two_pass_transforms_share_one_workspace(eng, oracle):
    """N = 65536: multiply at batch 2 (two compact operands per polynomial in the workspace WS3), then forward at batch 1 and inverse at batch 2 on what it left."""
    n = 65536
    moduli = _primes(30, n, 1)
    R = _transform_ref(oracle, 30, 1, n, 2)
    e = eng.RnsNttEngine(n, moduli)
    A, B = R["A"], R["B"]
    dA, dB, dR = _up(eng, A), _up(eng, B), _poisoned(eng, A.nbytes)
    e.multiply(dR, dA, dB, 2); _same(dR, R["mul"], "multiply")
    dF = _up(eng, np.ascontiguousarray(A[:1]))
    e.forward(dF, 1); _same(dF, R["fwd"][:1], "forward")
    e.inverse(dB, 2); _same(dB, R["inv"], "inverse")
    _same(dA, A, "a is read only")


# ------------------------------------------------------------------------------------ alignment contract
def test_misaligned_pointers_are_rejected(eng):
    """include/fhe_hip.h: container pointers are 16-byte aligned.  base + 8 is refused with FHE_ERR_INVALID_ARG by an entry point of every
    subsystem before anything is launched (the poisoned buffers are still poison); base + 32, the container-granular slice, is what every
    guarded case above passes."""
    n, L = 2048, 2
    moduli = _primes(30, n, L)
    e = eng.RnsNttEngine(n, moduli)
    S = L * n * 32
    bufs = [_poisoned(eng, S + 64) for _ in range(3)]
    r, a, b = (x.ptr for x in bufs)
    sh = _up(eng, np.zeros(1, np.uint32))
    q = moduli[0]
    calls = {
        "transforms: forward": lambda: e.forward(a + 8, 1),
        "transforms: multiply, result": lambda: e.multiply(r + 8, a, b, 1),
        "transforms: multiply, operand": lambda: e.multiply(r, a, b + 8, 1),
        "transforms: ct_multiply": lambda: e.ct_multiply(r, r + S // 2, a, a + 8, b, a + 32, b + 32, 1),
        "keyswitch: automorphism": lambda: e.automorphism(r, a + 8, 3, 1),
        "keyswitch: monomial_mul_sub": lambda: e.monomial_mul_sub(r + 8, a, sh, 1),
        "rns: to_rns": lambda: e.to_rns(r, a + 8, 1),
        "rns: rescale_drop_last": lambda: e.rescale_drop_last(r + 24, a, 1),
        "sampling: rns_sample_uniform": lambda: e.sample_uniform(r + 8, 1, 1),
        "sampling: sample_uniform_lcg": lambda: eng.sample_uniform_lcg(r + 8, q, 1, 16),
        "sampling: poly_mod_switch": lambda: eng.poly_mod_switch(r, a + 8, q, 257, 16),
        "literal: u256_add_mod": lambda: eng.u256_add_mod(r, a, b + 8, q, 16),
        "literal: bit_reverse": lambda: eng.bit_reverse(r + 8, 16, 1),
    }
    for what, call in calls.items():
        with pytest.raises(eng.FheError) as ei:
            call()
        assert ei.value.code == -1 and "16-byte aligned" in str(ei.value), what
    eng.capi.sync()
    for x in bufs:
        assert is_poison(x.download((-1,), np.uint8))
    e.sample_uniform(r + 32, 7, 1)                                         # a whole-container offset is accepted
    eng.capi.sync()
