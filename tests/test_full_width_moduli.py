"""The full-width class (FHE_WIDTH_256) on GENERIC moduli and at the edges of its ranges, on every kernel family, against the CPU oracle and
Python integers.

tests/ntt_math.py::ntt_primes returns 2^(bits-1) + small: six of the eight 32-bit words of such a 250-bit prime are zero, so 48 of the 56
terms m_i * q_j of the hand-scheduled Montgomery product (mont_mul_fips, csrc/u256_dev.h) multiply by zero and no borrow ever travels through
the middle limbs of add_mod / sub_mod with both operands non-trivial; largest_ntt_primes returns 2^bits - small, whose middle words are all
ones.  Here the moduli are (ntt_math.full_width_moduli)
  g<bits>   generic primes: every 32-bit word below the top one is neither 0 nor 0xFFFFFFFF; widths 65 (first above the word-sized classes),
            100, 127 (top of the two-limb transforms), 128 (bottom of the four-limb ones), 129, 192, 193, 250 (lazy top), 255 (canonical top);
  t<bits>   the largest primes below 2^127, 2^128 and 2^255: sums at the container limit;
  mixed-a   generic 250-bit + generic 100-bit + a 60-bit prime: digits of the wide limbs exceed the narrow modulus (d %= q in the digit
            embedding), and the rescale meets a last prime wider or narrower than the others;
  mixed-b   generic 127-bit + generic 122-bit: two-limb transforms that are not lazy,
and the operands are random slots plus slots of all q - 1, of q - 1 / 0 and q - 1 / 1 alternating, and of a random low part under q's own top
word (a comparison with q is decided in the middle limbs).  Integer work: every comparison is np.array_equal on whole arrays.  The oracle
itself is checked on the same kinds of moduli against Python integers in tests/test_oracle.py."""
import random

import numpy as np
import pytest

import ntt_math as nm
from test_galois import sigma_np
from test_hoisted import _expected
from workload import rns_poly

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
N = 2048                                             # one tile of the full-width transforms
GENERIC = ["g%d" % b for b in nm.GENERIC_BITS]
TOP = ["t127", "t128", "t255"]
KEYSWITCH_SETS = ["mixed-a", "mixed-b", "g127", "g128", "g250", "t255"]
A_SLOTS = [None, "top", "alt0", "alt1", "low", None]              # two calls of batch 3; every pattern is carried by one of them
B_SLOTS = [None, "top", "alt1", "top", "low", "alt0"]
BATCH = 3


@pytest.fixture(scope="module")
def eng(pkg):
    if pkg.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")
    return pkg


def _up(pkg, arr):
    return pkg.DeviceBuffer.from_numpy(arr)


# ------------------------------------------------------------------------------------ moduli and operands
def _moduli(name, n=N):
    """Cached in ntt_math.full_width_moduli; every full-width prime of a set has generic words unless the set is a TOP one."""
    qs = nm.full_width_moduli(name, n)
    for q in qs:
        assert q % (2 * n) == 1
        if name[0] != "t" and q.bit_length() > 64:
            assert nm.has_generic_words(q), hex(q)
    return qs


def _engine(eng, n, moduli):
    e = eng.RnsNttEngine(n, moduli)
    assert e.width_class == eng.WIDTH_256
    return e


def _to_limbs(vals):
    vals = list(vals)
    out = np.empty((len(vals), 4), dtype=np.uint64)
    for k in range(4):
        out[:, k] = np.array([(v >> (64 * k)) & M64 for v in vals], dtype=np.uint64)
    return out


def _to_ints(arr):
    a = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, 4)
    c = [a[:, k].tolist() for k in range(4)]
    return [x0 | (x1 << 64) | (x2 << 128) | (x3 << 192) for x0, x1, x2, x3 in zip(*c)]


def _limbs_of(v):
    return np.array([(v >> (64 * k)) & M64 for k in range(4)], dtype=np.uint64)


def _patterns(moduli, n, which, seed=0):
    """[len(which)][L][n][4], all four limbs filled: 'top' every coefficient q - 1; 'alt0' q - 1 and 0 alternating; 'alt1' q - 1 and 1
    alternating; 'low' q's own top 32-bit word over a random lower part below q's."""
    out = np.zeros((len(which), len(moduli), n, 4), np.uint64)
    for s, name in enumerate(which):
        for l, q in enumerate(moduli):
            if name == "low":
                rng = random.Random(seed * 1000 + s * 64 + l)
                sh = 32 * ((q.bit_length() - 1) // 32)
                out[s, l] = _to_limbs((q >> sh << sh) + rng.randrange(q & ((1 << sh) - 1)) for _ in range(n))
            elif name == "top":
                out[s, l, :] = _limbs_of(q - 1)
            else:
                out[s, l, ::2] = _limbs_of(q - 1)
                out[s, l, 1::2] = _limbs_of(0 if name == "alt0" else 1)
    return out


def _mixed(seed, moduli, n, which):
    """One array whose slot s is random (which[s] is None) or a pattern."""
    out = rns_poly(seed, moduli, n, len(which))
    for s, name in enumerate(which):
        if name:
            out[s] = _patterns(moduli, n, [name], seed)[0]
    return out


def _groups(arr, batch=BATCH):
    return [np.ascontiguousarray(arr[g:g + batch]) for g in range(0, arr.shape[0], batch)]


def _keys(moduli, n, count, seed):
    return [rns_poly(seed + 17 * i, moduli, n, 1)[0] for i in range(count)]


_REF = {}


def _cached(key, make):
    """The oracle's answer for one parameter set, shared by the kernel forms that are checked against it (the form varies fastest)."""
    if key not in _REF:
        if len(_REF) >= 2:
            _REF.pop(next(iter(_REF)))
        _REF[key] = make()
    return _REF[key]


def _per_limb_ints(fn, a, b, moduli):
    """fn(x, y, q) on Python integers over [slots][L][n] containers."""
    out = np.empty_like(a)
    for l, q in enumerate(moduli):
        x = _to_ints(a[:, l]); y = _to_ints(b[:, l])
        out[:, l] = _to_limbs(fn(u, v, q) for u, v in zip(x, y)).reshape(a.shape[0], a.shape[2], 4)
    return out


def _per_limb_oracle(fn, a, b, moduli):
    return np.stack([np.stack([fn(np.ascontiguousarray(a[s, l]), np.ascontiguousarray(b[s, l]), l) for l in range(len(moduli))])
                     for s in range(a.shape[0])])


# ------------------------------------------------------------------------------------ element-wise
@pytest.mark.parametrize("name", GENERIC + TOP + ["mixed-a", "mixed-b"])
def test_elementwise_ops_on_generic_moduli(eng, oracle, name):
    """pointwise (mont_mul_fips twice), poly_add / poly_sub (add_mod / sub_mod), the literal Montgomery product (mont_mul) and the handle-free
    kernels, against Python integers and the oracle.  The sums reach 2q - 2, the differences 0 - (q - 1), the products (q - 1)^2."""
    n = N
    moduli = _moduli(name); L = len(moduli)
    e = _engine(eng, n, moduli)
    rp = oracle.RnsPlan(n, moduli)
    A, B = _mixed(1, moduli, n, A_SLOTS), _mixed(2, moduli, n, B_SLOTS)
    want = {"pointwise": _per_limb_ints(lambda x, y, q: x * y % q, A, B, moduli),
            "poly_add": _per_limb_ints(nm.add_mod_ref, A, B, moduli),
            "poly_sub": _per_limb_ints(nm.sub_mod_ref, A, B, moduli),
            "mul_mont_literal": _per_limb_ints(nm.mont_mul_ref, A, B, moduli)}
    assert np.array_equal(want["poly_add"], _per_limb_ints(lambda x, y, q: (x + y) % q, A, B, moduli))
    assert np.array_equal(want["poly_sub"], _per_limb_ints(lambda x, y, q: (x - y) % q, A, B, moduli))
    assert np.array_equal(want["pointwise"], _per_limb_oracle(lambda x, y, l: rp.plans[l].pointwise(x, y), A, B, moduli))
    assert np.array_equal(want["poly_add"], _per_limb_oracle(lambda x, y, l: oracle.batch_add(x, y, moduli[l]), A, B, moduli))
    assert np.array_equal(want["poly_sub"], _per_limb_oracle(lambda x, y, l: oracle.batch_sub(x, y, moduli[l]), A, B, moduli))
    assert np.array_equal(want["mul_mont_literal"], _per_limb_oracle(lambda x, y, l: oracle.batch_mont(x, y, moduli[l]), A, B, moduli))
    shape = (BATCH,) + A.shape[1:]
    for g, (a, b) in enumerate(zip(_groups(A), _groups(B))):
        sl = slice(g * BATCH, (g + 1) * BATCH)
        dA, dB, dR = _up(eng, a), _up(eng, b), eng.DeviceBuffer(a.nbytes)
        for op in ("pointwise", "poly_add", "poly_sub", "mul_mont_literal"):
            getattr(e, op)(dR, dA, dB, BATCH)
            assert np.array_equal(dR.download(shape), want[op][sl]), (op, g)
            e.check_canonical(dR, BATCH)
        dC = _up(eng, a); e.poly_sub(dC, dC, dB, BATCH)                            # in place
        assert np.array_equal(dC.download(shape), want["poly_sub"][sl]), g
        assert np.array_equal(dA.download(shape), a) and np.array_equal(dB.download(shape), b)
    # the handle-free kernels: one modulus, a flat array
    rng = random.Random(7)
    for l, q in enumerate(moduli):
        a, b = np.ascontiguousarray(A[:, l]).reshape(-1, 4), np.ascontiguousarray(B[:, l]).reshape(-1, 4)
        count = a.shape[0]
        dA, dB, dR = _up(eng, a), _up(eng, b), eng.DeviceBuffer(a.nbytes)
        inv0 = nm.mont_inverse_ref(q)
        assert eng.montgomery_inverse(q) & M64 == inv0
        eng.u256_add_mod(dR, dA, dB, q, count); assert np.array_equal(dR.download(), want["poly_add"][:, l].reshape(-1, 4)), q
        eng.u256_sub_mod(dR, dA, dB, q, count); assert np.array_equal(dR.download(), want["poly_sub"][:, l].reshape(-1, 4)), q
        eng.u256_mont_mul(dR, dA, dB, q, inv0, count); assert np.array_equal(dR.download(), want["mul_mont_literal"][:, l].reshape(-1, 4)), q
        for s in (q - 1, rng.randrange(q)):
            eng.u256_mont_mul_scalar(dR, dA, s, q, inv0, count)
            assert np.array_equal(dR.download(), _to_limbs(nm.mont_mul_ref(x, s, q) for x in _to_ints(a))), (q, s)


# ------------------------------------------------------------------------------------ transforms and products
def _tp_case(oracle, name, n):
    def make():
        moduli = _moduli(name, n)
        rp = oracle.RnsPlan(n, moduli)
        A, B = _mixed(11, moduli, n, A_SLOTS), _mixed(12, moduli, n, B_SLOTS)
        one = np.ascontiguousarray(B[4:5])                                          # the shared operand of multiply_bcast: the 'low' slot
        ct = (A, B, np.ascontiguousarray(B[::-1]), np.ascontiguousarray(A[::-1]))
        return dict(moduli=moduli, A=A, B=B, one=one, ct=ct, f=rp.forward(A, threads=8), i=rp.inverse(B, threads=8),
                    m=rp.polymul(A, B, threads=8), sq=rp.polymul(A, A, threads=8),
                    bc=rp.polymul(A, np.ascontiguousarray(np.broadcast_to(one, A.shape)), threads=8), ctw=rp.ct_multiply(*ct, threads=8))
    return _cached(("tp", name, n), make)


SWITCHES = {"default": None, "canonical": "FHE_HIP_NO_WIDE_LAZY", "no-tiles": "FHE_HIP_NO_WIDE_TILES"}
TRANSFORM_CASES = [(name, N, "default") for name in GENERIC + TOP + ["mixed-a", "mixed-b"]]
TRANSFORM_CASES += [("g100", N, "canonical"), ("g100", N, "no-tiles"), ("g127", N, "no-tiles"), ("g128", N, "canonical"), ("g250", N, "canonical"),
                    ("g250", N, "no-tiles"), ("g255", N, "no-tiles"), ("mixed-a", N, "canonical")]
TRANSFORM_CASES += [(name, 4096, sw) for name in ("g127", "g128", "g250", "g255") for sw in (("default", "canonical", "no-tiles") if name == "g250" else ("default",))]
TRANSFORM_CASES += [(name, n, "default") for name in ("g127", "g255") for n in (8, 256)]       # below one tile
TRANSFORM_CASES.sort(key=lambda c: (c[0], c[1]))                                               # the switch varies fastest: one oracle run per (set, n)


@pytest.mark.parametrize("name,n,switch", TRANSFORM_CASES)
def test_transforms_and_products_on_generic_moduli(eng, oracle, monkeypatch, name, n, switch):
    """forward, inverse, multiply, squaring in place, multiply_bcast and ct_multiply.  n = 2048 is one tile, n = 4096 two tiles under a
    global-memory pass, n = 8 and 256 the sub-tile sizes; 'canonical' = the tile kernels that reduce in every butterfly, 'no-tiles' = every
    stage as a global-memory pass."""
    if SWITCHES[switch]:
        monkeypatch.setenv(SWITCHES[switch], "1")
    c = _tp_case(oracle, name, n)
    e = _engine(eng, n, c["moduli"])
    shape = (BATCH,) + c["A"].shape[1:]
    dOne = _up(eng, c["one"])
    for g, (a, b) in enumerate(zip(_groups(c["A"]), _groups(c["B"]))):
        sl = slice(g * BATCH, (g + 1) * BATCH)

        def same(buf, want, what):
            assert np.array_equal(buf.download(shape), want[sl]), (what, g)
            e.check_canonical(buf, BATCH)

        dA, dB, dR = _up(eng, a), _up(eng, b), eng.DeviceBuffer(a.nbytes)
        e.forward(dA, BATCH); same(dA, c["f"], "forward")
        e.inverse(dA, BATCH); same(dA, c["A"], "inverse of forward")
        dT = _up(eng, b); e.inverse(dT, BATCH); same(dT, c["i"], "inverse")
        e.multiply(dR, dA, dB, BATCH); same(dR, c["m"], "multiply")
        assert np.array_equal(dA.download(shape), a) and np.array_equal(dB.download(shape), b)
        dC = _up(eng, a); e.multiply(dC, dC, dC, BATCH); same(dC, c["sq"], "square in place")
        e.multiply_bcast(dR, dA, dOne, BATCH); same(dR, c["bc"], "multiply_bcast")
        d = [_up(eng, np.ascontiguousarray(x[sl])) for x in c["ct"]]
        o = [eng.DeviceBuffer(a.nbytes) for _ in range(3)]
        e.ct_multiply(o[0], o[1], o[2], d[0], d[1], d[2], d[3], BATCH)
        for k in range(3):
            same(o[k], c["ctw"][k], ("ct_multiply", k))


@pytest.mark.parametrize("name", ["g128", "g255"])
def test_single_modulus_engine_on_generic_moduli(eng, oracle, name):
    n = N
    q = _moduli(name)[0]
    e = eng.NttEngine(n, q)
    assert e.width_class == eng.WIDTH_256
    rp = oracle.RnsPlan(n, [q])
    A, B = _mixed(21, [q], n, A_SLOTS[:BATCH + 2]), _mixed(22, [q], n, B_SLOTS[:BATCH + 2])     # batch 5: random, top, alt0, alt1, low
    batch, shape = A.shape[0], A.shape
    dA, dB, dR = _up(eng, A), _up(eng, B), eng.DeviceBuffer(A.nbytes)
    e.forward(dA, batch); assert np.array_equal(dA.download(shape), rp.forward(A, threads=8))
    e.inverse(dA, batch); assert np.array_equal(dA.download(shape), A)
    e.pointwise(dR, dA, dB, batch)
    assert np.array_equal(dR.download(shape), _per_limb_ints(lambda x, y, m: x * y % m, A, B, [q]))
    e.multiply(dR, dA, dB, batch); assert np.array_equal(dR.download(shape), rp.polymul(A, B, threads=8))


@pytest.mark.parametrize("force", [None, "256"])
@pytest.mark.parametrize("name", ["g127", "t127", "g128", "t128"])
def test_forced_four_limb_transforms_agree_on_both_sides_of_127_bits(eng, oracle, monkeypatch, name, force):
    """A basis of at most 127 bits runs the transforms on two 64-bit limbs (a + b approaches 2^128), one of 128 bits on four;
    FHE_HIP_FORCE_WIDTH=256 puts both on four.  Same results either way, bit for bit (the idiom of test_forced_wider_paths_agree)."""
    if force:
        monkeypatch.setenv("FHE_HIP_FORCE_WIDTH", force)
    c = _tp_case(oracle, name, N)
    e = _engine(eng, N, c["moduli"])
    shape = (BATCH,) + c["A"].shape[1:]
    for g, (a, b) in enumerate(zip(_groups(c["A"]), _groups(c["B"]))):
        sl = slice(g * BATCH, (g + 1) * BATCH)
        dA, dB, dR = _up(eng, a), _up(eng, b), eng.DeviceBuffer(a.nbytes)
        e.multiply(dR, dA, dB, BATCH); assert np.array_equal(dR.download(shape), c["m"][sl]), g
        e.forward(dA, BATCH); assert np.array_equal(dA.download(shape), c["f"][sl]), g
        e.inverse(dB, BATCH); assert np.array_equal(dB.download(shape), c["i"][sl]), g


# ------------------------------------------------------------------------------------ key switch
ACC0, ACC1 = [None, "top", "alt1"], ["top", "low", None]                           # accumulators: add_mod runs at q - 1
C2_SLOTS = ([None, "top", "alt0"], ["alt1", "low", "top"])                         # all q - 1: the largest digits


def _ks_case(oracle, name, w):
    def make():
        moduli = _moduli(name); L = len(moduli)
        rp = oracle.RnsPlan(N, moduli); K = rp.num_digits(w)
        assert K == (max(q.bit_length() for q in moduli) + w - 1) // w
        kb = _keys(moduli, N, L * K, 100); ka = _keys(moduli, N, L * K, 900)
        c0, c1 = _mixed(51, moduli, N, ACC0), _mixed(52, moduli, N, ACC1)
        c2s = [_mixed(53 + i, moduli, N, which) for i, which in enumerate(C2_SLOTS)]
        return moduli, K, kb, ka, c0, c1, c2s, [rp.relinearize(w, c0, c1, c2, kb, ka, threads=8) for c2 in c2s]
    return _cached(("ks", name, w), make)


@pytest.mark.parametrize("w", [64, 61, 32])
@pytest.mark.parametrize("name", KEYSWITCH_SETS)
def test_relinearize_on_generic_moduli(eng, oracle, name, w):
    """digit_embed256_kernel + relin_mac256_kernel (mont_mul_fips on every digit x key product) between full-width transforms.  w = 64: a digit
    is a whole limb, top bits set; w = 61: digits straddle the limbs; w = 32: half limbs.  On mixed-a the digits are reduced modulo the 60-bit limb."""
    moduli, K, kb, ka, c0, c1, c2s, want = _ks_case(oracle, name, w)
    e = _engine(eng, N, moduli)
    assert e.relin_num_digits(w) == K
    rk = e.import_relin_keys(w, [_up(eng, k) for k in kb], [_up(eng, k) for k in ka])
    for c2, (w0, w1) in zip(c2s, want):
        d0, d1, d2 = _up(eng, c0), _up(eng, c1), _up(eng, c2)
        e.relinearize(rk, d0, d1, d2, BATCH)
        assert np.array_equal(d0.download(c0.shape), w0) and np.array_equal(d1.download(c0.shape), w1)
        assert np.array_equal(d2.download(c0.shape), c2)
        e.check_canonical(d0, BATCH); e.check_canonical(d1, BATCH)


def _ctr_case(oracle, name, w):
    def make():
        moduli = _moduli(name); L = len(moduli)
        rp = oracle.RnsPlan(N, moduli); K = rp.num_digits(w)
        kb = _keys(moduli, N, L * K, 1100); ka = _keys(moduli, N, L * K, 1900)
        ops = [_mixed(61, moduli, N, ACC0), _mixed(62, moduli, N, ACC1), _mixed(63, moduli, N, C2_SLOTS[1]), _mixed(64, moduli, N, ["top"] * BATCH)]
        t0, t1, t2 = rp.ct_multiply(*ops, threads=8)
        return moduli, kb, ka, ops, rp.relinearize(w, t0, t1, t2, kb, ka, threads=8)
    return _cached(("ctr", name, w), make)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("w", [64, 61])
@pytest.mark.parametrize("name", KEYSWITCH_SETS)
def test_ct_multiply_relin_on_generic_moduli(eng, oracle, monkeypatch, name, w, fused):
    if not fused:
        monkeypatch.setenv("FHE_HIP_NO_FUSED_CT_RELIN", "1")
    moduli, kb, ka, ops, (w0, w1) = _ctr_case(oracle, name, w)
    e = _engine(eng, N, moduli)
    rk = e.import_relin_keys(w, [_up(eng, k) for k in kb], [_up(eng, k) for k in ka])
    d = [_up(eng, x) for x in ops]
    o0, o1 = eng.DeviceBuffer(ops[0].nbytes), eng.DeviceBuffer(ops[0].nbytes)
    e.ct_multiply_relin(rk, o0, o1, d[0], d[1], d[2], d[3], BATCH)
    assert np.array_equal(o0.download(ops[0].shape), w0) and np.array_equal(o1.download(ops[0].shape), w1)
    for buf, src in zip(d, ops):
        assert np.array_equal(buf.download(src.shape), src)
    e.check_canonical(o0, BATCH); e.check_canonical(o1, BATCH)


def _sigma(a, moduli, g):
    """include/fhe_hip.h, gather form: i = j g^-1 mod 2n; out[j] = in[i] if i < n, else (q - in[i - n]) mod q."""
    n = a.shape[2]
    i = (np.arange(n, dtype=np.int64) * pow(g, -1, 2 * n)) % (2 * n)
    neg = (i >= n).tolist()
    out = np.ascontiguousarray(a[:, :, i % n, :])
    for l, q in enumerate(moduli):
        for s in range(a.shape[0]):
            out[s, l] = _to_limbs((q - v) % q if ng else v for v, ng in zip(_to_ints(out[s, l]), neg))
    return out


@pytest.mark.parametrize("name", KEYSWITCH_SETS)
def test_apply_galois_on_generic_moduli(eng, oracle, name):
    """fhe_ct_apply_galois == the oracle's relinearize(sigma(c0), 0, sigma(c1)), sigma written out above; g = 3 and g = 2n - 1, w = 61."""
    w = 61

    def make():
        moduli = _moduli(name); L = len(moduli)
        rp = oracle.RnsPlan(N, moduli); K = rp.num_digits(w)
        kb = _keys(moduli, N, L * K, 700); ka = _keys(moduli, N, L * K, 1300)
        c0, c1 = _mixed(81, moduli, N, ["top", None, "alt0"]), _mixed(82, moduli, N, ["low", "top", "alt1"])
        return moduli, kb, ka, c0, c1, [rp.relinearize(w, _sigma(c0, moduli, x), np.zeros_like(c0), _sigma(c1, moduli, x), kb, ka, threads=8) for x in (3, 2 * N - 1)]
    moduli, kb, ka, c0, c1, want = _cached(("galois", name), make)
    e = _engine(eng, N, moduli)
    gk = e.import_relin_keys(w, [_up(eng, k) for k in kb], [_up(eng, k) for k in ka])
    d0, d1 = _up(eng, c0), _up(eng, c1)
    o0, o1 = eng.DeviceBuffer(c0.nbytes), eng.DeviceBuffer(c0.nbytes)
    for x, (w0, w1) in zip((3, 2 * N - 1), want):
        e.apply_galois(gk, x, o0, o1, d0, d1, BATCH)
        assert np.array_equal(o0.download(c0.shape), w0) and np.array_equal(o1.download(c0.shape), w1), x
        e.check_canonical(o0, BATCH); e.check_canonical(o1, BATCH)
    assert np.array_equal(d0.download(c0.shape), c0) and np.array_equal(d1.download(c0.shape), c1)


@pytest.mark.parametrize("name", KEYSWITCH_SETS)
def test_apply_galois_hoisted_on_generic_moduli(eng, oracle, name):
    """fhe_ct_hoist + fhe_ct_apply_galois_hoisted: digit_embed256_kernel, full-width transforms and relin_mac_perm256_kernel (mont_mul_fips on every
    digit x key product, the digits read at pi_g), on two-limb (mixed-b, g127) and four-limb residues.  w = 64: a digit is a whole limb.  Against
    the identity of tests/test_hoisted.py (pinned to the header's definition by test_hoisted_identity_equals_the_header_definition); its sigma and the
    one written out above are two implementations and must agree.  The full-width class keeps containers: 32 bytes per kept value."""
    n, w, elements = N, 64, (1, 3, 2 * N - 1)

    def make():
        moduli = _moduli(name); L = len(moduli)
        rp = oracle.RnsPlan(n, moduli); K = rp.num_digits(w)
        kb = _keys(moduli, n, L * K, 700); ka = _keys(moduli, n, L * K, 1300)
        c0, c1 = _mixed(81, moduli, n, A_SLOTS), _mixed(82, moduli, n, B_SLOTS)
        for g in elements[1:]:
            assert np.array_equal(sigma_np(c1, moduli, g), _sigma(c1, moduli, g)), g
        return moduli, K, kb, ka, c0, c1, [_expected(oracle, n, moduli, w, c0, c1, kb, ka, g) for g in elements]
    moduli, K, kb, ka, c0, c1, want = _cached(("hoisted", name), make)
    L = len(moduli)
    e = _engine(eng, n, moduli)
    assert e.relin_num_digits(w) == K
    gk = e.import_relin_keys(w, [_up(eng, k) for k in kb], [_up(eng, k) for k in ka])
    shape = (BATCH,) + c0.shape[1:]
    for s, (a0, a1) in enumerate(zip(_groups(c0), _groups(c1))):
        sl = slice(s * BATCH, (s + 1) * BATCH)
        d0, d1 = _up(eng, a0), _up(eng, a1)
        o0, o1 = eng.DeviceBuffer(a0.nbytes), eng.DeviceBuffer(a0.nbytes)
        e.hoist(w, d1, BATCH)
        assert e.hoist_bytes() == BATCH * L * K * L * n * 32
        for g, (w0, w1) in zip(elements, want):
            e.apply_galois_hoisted(gk, g, o0, o1, d0, BATCH)
            assert np.array_equal(o0.download(shape), w0[sl]) and np.array_equal(o1.download(shape), w1[sl]), (g, s)
            e.check_canonical(o0, BATCH); e.check_canonical(o1, BATCH)
        p0, p1 = eng.DeviceBuffer(a0.nbytes), eng.DeviceBuffer(a0.nbytes)         # sigma_1 is the identity: the plain key switch, bit for bit
        e.apply_galois(gk, 1, p0, p1, d0, d1, BATCH)
        assert np.array_equal(p0.download(shape), want[0][0][sl]) and np.array_equal(p1.download(shape), want[0][1][sl]), s
        assert np.array_equal(d0.download(shape), a0) and np.array_equal(d1.download(shape), a1)


@pytest.mark.parametrize("name", KEYSWITCH_SETS)
def test_blind_rotate_on_generic_moduli(eng, oracle, name):
    """Two steps, accumulators random / all q - 1 / alternating / low: (X^a - 1) acc reaches 2q - 2 before it is reduced; w = 61; the six
    shifts are the edges of [0, 2n).  Then one step alone through fhe_blind_rotate_step."""
    n, steps, w = N, 2, 61
    moduli = _moduli(name); L = len(moduli)
    rp = oracle.RnsPlan(n, moduli); K = rp.num_digits(w)
    rows = [[(_keys(moduli, n, L * K, 7000 + 100 * c + 1000 * s), _keys(moduli, n, L * K, 8000 + 100 * c + 1000 * s)) for c in range(2)] for s in range(steps)]
    a0, a1 = _mixed(611, moduli, n, ACC0), _mixed(612, moduli, n, ACC1)
    shifts = np.array([[1, n, 2 * n - 1], [n - 1, 0, n + 1]], dtype=np.uint32)
    w0, w1 = rp.blind_rotate(w, a0, a1, shifts, [r[0] for r in rows], [r[1] for r in rows], threads=8)
    e = _engine(eng, n, moduli)
    imported = [[e.import_relin_keys(w, [_up(eng, k) for k in kb], [_up(eng, k) for k in ka]) for kb, ka in r] for r in rows]
    dA0, dA1 = _up(eng, a0), _up(eng, a1)
    dT0, dT1 = eng.DeviceBuffer(a0.nbytes), eng.DeviceBuffer(a0.nbytes)
    e.blind_rotate([r[0] for r in imported], [r[1] for r in imported], dA0, dA1, eng.DeviceBuffer.from_numpy(shifts), dT0, dT1, BATCH)
    assert np.array_equal(dA0.download(a0.shape), w0) and np.array_equal(dA1.download(a0.shape), w1)
    e.check_canonical(dA0, BATCH); e.check_canonical(dA1, BATCH)
    sh = np.array([n + 1, 2 * n - 1, n], dtype=np.uint32)
    s0, s1 = rp.blind_rotate_step(w, a1, a0, sh, rows[1][0], rows[1][1], threads=8)
    dA0, dA1 = _up(eng, a1), _up(eng, a0)
    e.blind_rotate_step(imported[1][0], imported[1][1], dA0, dA1, eng.DeviceBuffer.from_numpy(sh), dT0, dT1, BATCH)
    assert np.array_equal(dA0.download(a0.shape), s0) and np.array_equal(dA1.download(a0.shape), s1)


# ------------------------------------------------------------------------------------ automorphism and monomial factor
@pytest.mark.parametrize("name", ["g127", "g128", "g255"])
def test_automorphism_and_monomial_factor_on_generic_moduli(eng, name):
    """Negation q - x over all four limbs at x = 0 (stays 0), 1, q - 1 and generic x; (X^a - 1) p: q - 1 minus 0, 0 minus q - 1 and
    -(q - 1) - (q - 1).  Against the definitions of include/fhe_hip.h in Python integers."""
    n = N
    moduli = _moduli(name)
    e = _engine(eng, n, moduli)
    a = _mixed(31, moduli, n, [None, "top", "alt0", "alt1", "low", None])
    a[0, :, ::97, :] = 0
    batch = a.shape[0]
    d_in, d_out = _up(eng, a), eng.DeviceBuffer(a.nbytes)
    for g in (3, 2 * n - 1, eng.galois_element(n, 77)):
        e.automorphism(d_out, d_in, g, batch)
        assert np.array_equal(d_out.download(a.shape), _sigma(a, moduli, g)), g
        e.check_canonical(d_out, batch)
    assert np.array_equal(d_in.download(a.shape), a)
    shifts = [0, 1, n - 1, n, n + 1, 2 * n - 1]
    for rot in (0, 3):
        sh = shifts[rot:] + shifts[:rot]
        want = np.empty_like(a)
        for s in range(batch):
            k = (np.arange(n) - sh[s]) % (2 * n)
            neg = (k >= n).tolist(); k = (k % n).tolist()
            for l, q in enumerate(moduli):
                p = _to_ints(a[s, l])
                want[s, l] = _to_limbs((-p[k[x]] - p[x] if neg[x] else p[k[x]] - p[x]) % q for x in range(n))
        e.monomial_mul_sub(d_out, d_in, eng.DeviceBuffer.from_numpy(np.array(sh, dtype=np.uint32)), batch)
        assert np.array_equal(d_out.download(a.shape), want), rot
        e.check_canonical(d_out, batch)


# ------------------------------------------------------------------------------------ RNS conversions
def _product(moduli):
    Q = 1
    for q in moduli:
        Q *= q
    return Q


def _word_switch(monkeypatch, word):
    if not word:
        monkeypatch.setenv("FHE_HIP_NO_WORD_CONVERSIONS", "1")


@pytest.mark.parametrize("word", [True, False])
@pytest.mark.parametrize("name", ["g127", "g128", "g255", "mixed-a"])
def test_to_rns_of_any_256_bit_value_on_generic_moduli(eng, oracle, monkeypatch, name, word):
    _word_switch(monkeypatch, word)
    n, batch = N, 2
    moduli = _moduli(name); L = len(moduli)
    e = _engine(eng, n, moduli)
    rng = random.Random(len(name))
    edge = [0, 1 << 255, (1 << 256) - 1]
    for q in moduli:
        edge += [q, q - 1, q + 1, (1 << 256) - q, (1 << 256) - q - 1]
    vals = edge + [rng.getrandbits(256) | (1 << 255) for _ in range(batch * n - len(edge))]
    V = _to_limbs(vals).reshape(batch, n, 4)
    dR = eng.DeviceBuffer(batch * L * n * 32)
    e.to_rns(dR, _up(eng, V), batch)
    R = dR.download((batch, L, n, 4))
    want = np.stack([np.stack([_to_limbs(v % q for v in vals[b * n:(b + 1) * n]) for q in moduli]) for b in range(batch)])
    assert np.array_equal(R, want)
    assert np.array_equal(R, oracle.RnsPlan(n, moduli).to_rns(V))
    e.check_canonical(dR, batch)


@pytest.mark.parametrize("word", [True, False])
@pytest.mark.parametrize("name", ["g85x3", "t127"])
def test_from_rns_up_to_255_bits_on_generic_moduli(eng, oracle, monkeypatch, name, word):
    """Q = q_0 q_1 q_2 of 255 bits (three generic 85-bit primes) is the largest product a container holds; two primes at the top of 127 bits give
    254.  Every residue q_l - 1 is Q - 1."""
    _word_switch(monkeypatch, word)
    n, batch = N, 2
    moduli = _moduli(name); L = len(moduli); Q = _product(moduli)
    assert Q.bit_length() == (255 if name == "g85x3" else 254)
    e = _engine(eng, n, moduli)
    rng = random.Random(L)
    vals = [0, 1, Q - 1, Q - 2] + [Q // q for q in moduli] + [Q - Q // q for q in moduli]
    vals += [rng.randrange(Q) for _ in range(batch * n - len(vals))]
    R = np.stack([np.stack([_to_limbs(v % q for v in vals[b * n:(b + 1) * n]) for q in moduli]) for b in range(batch)])
    assert _to_ints(R[0, :, 2]) == [q - 1 for q in moduli]
    dV = eng.DeviceBuffer(batch * n * 32)
    e.from_rns(dV, _up(eng, R), batch)
    got = dV.download((batch, n, 4))
    assert _to_ints(got) == vals                                                     # the CRT inverts Python's %
    assert np.array_equal(got, oracle.RnsPlan(n, moduli).from_rns(R))


@pytest.mark.parametrize("word", [True, False])
@pytest.mark.parametrize("order", ["widest-last", "narrowest-last"])
def test_rescale_drop_last_on_a_mixed_basis(eng, oracle, monkeypatch, order, word):
    """mixed-a in both orders: the centred remainder of the last limb (up to 249 bits, or below 2^59) is reduced modulo the other primes.  Against
    rounded division of the CRT value in Python integers."""
    _word_switch(monkeypatch, word)
    n, batch = N, 2
    moduli = _moduli("mixed-a")
    if order == "widest-last":
        moduli = moduli[::-1]
    L = len(moduli); ql = moduli[-1]; Q = _product(moduli)
    e = _engine(eng, n, moduli)
    c = _mixed(401, moduli, n, [None, "top"])
    edge = [ql // 2, ql // 2 + 1, 0, ql - 1]
    c[0, L - 1, :4] = _to_limbs(edge); c[1, L - 1, :4] = _to_limbs(edge)
    c[1, L - 1, 4::2] = _limbs_of(ql // 2); c[1, L - 1, 5::2] = _limbs_of(ql // 2 + 1)
    dIn = _up(eng, c); dOut = eng.DeviceBuffer(batch * (L - 1) * n * 32)
    e.rescale_drop_last(dOut, dIn, batch)
    got = dOut.download((batch, L - 1, n, 4))
    res = [[_to_ints(c[b, l]) for l in range(L)] for b in range(batch)]
    coef = [pow(Q // q, -1, q) * (Q // q) for q in moduli]
    want = np.empty_like(got)
    for b in range(batch):
        C = [sum(res[b][l][x] * coef[l] for l in range(L)) % Q for x in range(n)]
        rounded = [(2 * v + ql) // (2 * ql) for v in C]                              # round(C / q_last), half up (q_last is odd: no ties)
        for l, q in enumerate(moduli[:-1]):
            want[b, l] = _to_limbs(r % q for r in rounded)
    assert np.array_equal(got, want)
    assert np.array_equal(got, oracle.RnsPlan(n, moduli).rescale_drop_last(c))
    assert np.array_equal(dIn.download(c.shape), c)
    eng.RnsNttEngine(n, moduli[:-1]).check_canonical(dOut, batch)


@pytest.mark.parametrize("word", [True, False])
@pytest.mark.parametrize("case", ["g250->g127+p60", "g127x2->g255", "p60x3->g250"])
def test_fast_base_convert_with_generic_moduli(eng, oracle, monkeypatch, case, word):
    """A scaled residue of up to 250 bits is reduced modulo a 127-bit and a 60-bit prime, and narrow residues are lifted into a 250-bit one.  The
    source of the last case is a word-sized engine: the conversion then runs the container kernel because the target is full-width."""
    _word_switch(monkeypatch, word)
    n, batch = N, 2
    src, dst = nm.base_conversion_case(case, n)
    for q in src + dst:
        assert q.bit_length() <= 64 or nm.has_generic_words(q)
    e, t = eng.RnsNttEngine(n, src), _engine(eng, n, dst)
    assert e.width_class == (eng.WIDTH_64 if case == "p60x3->g250" else eng.WIDTH_256)
    L, Lp = len(src), len(dst); Q = _product(src)
    x = _mixed(501, src, n, [None, "top"])
    dX = _up(eng, x); dY = eng.DeviceBuffer(batch * Lp * n * 32)
    e.fast_base_convert(t, dY, dX, batch)
    got = dY.download((batch, Lp, n, 4))
    coef = [(pow(Q // q, -1, q), Q // q) for q in src]
    want = np.empty_like(got)
    for b in range(batch):
        res = [_to_ints(x[b, l]) for l in range(L)]
        full = [sum(res[l][i] * coef[l][0] % src[l] * coef[l][1] for l in range(L)) for i in range(n)]
        for j, p in enumerate(dst):
            want[b, j] = _to_limbs(f % p for f in full)
    assert np.array_equal(got, want)
    assert np.array_equal(got, oracle.RnsPlan(n, src).fast_base_convert(oracle.RnsPlan(n, dst), x))
    t.check_canonical(dY, batch)


# ------------------------------------------------------------------------------------ samplers and the rest
@pytest.mark.parametrize("name", ["g127", "g255"])
def test_rns_samplers_on_generic_moduli(eng, oracle, name):
    n, batch = N, 3
    moduli = _moduli(name); L = len(moduli)
    e = _engine(eng, n, moduli); rp = oracle.RnsPlan(n, moduli)
    d = eng.DeviceBuffer(batch * L * n * 32); shape = (batch, L, n, 4)
    e.sample_uniform(d, 2024, batch)
    got = d.download(shape)
    assert np.array_equal(got, rp.sample_uniform(2024, batch))
    e.check_canonical(d, batch)
    for l, q in enumerate(moduli):
        v = _to_ints(got[:, l])
        assert max(v) < q and max(v).bit_length() > q.bit_length() - 8              # canonical, and the whole width is used
    e.sample_ternary(d, 0.5, 1234, batch)
    got = d.download(shape)
    assert np.array_equal(got, rp.sample_ternary(0.5, 1234, batch))
    small = []
    for l, q in enumerate(moduli):
        v = _to_ints(got[:, l])
        assert set(v) == {0, 1, q - 1}                                              # -1 is q - 1 over all four limbs
        small.append([x - q if x > 1 else x for x in v])
    assert all(s == small[0] for s in small)                                        # the same small integer in every limb
    assert eng.gaussian_cdt(3.2) == oracle.gaussian_cdt(3.2)
    e.sample_gaussian(d, 3.2, 99, batch)
    got = d.download(shape)
    assert np.array_equal(got, rp.sample_gaussian(3.2, 99, batch))
    small = []
    for l, q in enumerate(moduli):
        v = _to_ints(got[:, l])
        assert all(x < 40 or x > q - 40 for x in v) and any(x > q - 40 for x in v)  # magnitudes stay below ceil(12 sigma) = 39; negative samples are q - m
        small.append([x - q if x >= 40 else x for x in v])
    assert all(s == small[0] for s in small)
    e.check_canonical(d, batch)


def _canonical_edges(q):
    """(accepted, rejected) values next to q: q - 1 and [a smaller top limb over all-ones lower limbs]; q and [q's upper limbs, limb 0 larger by one]."""
    t = (q.bit_length() - 1) // 64
    below = (((q >> (64 * t)) - 1) << (64 * t)) | ((1 << (64 * t)) - 1)
    assert below < q and (q + 1) >> 64 == q >> 64
    return [q - 1, below], [q, q + 1]


@pytest.mark.parametrize("name", GENERIC + ["t255"])
def test_check_canonical_on_generic_moduli(eng, monkeypatch, name):
    """check256_kernel compares over all four limbs; with FHE_HIP_CHECK_INPUTS=1 the compute entry points do the same scan first."""
    n = N
    moduli = _moduli(name); L = len(moduli)
    e = _engine(eng, n, moduli)
    monkeypatch.setenv("FHE_HIP_CHECK_INPUTS", "1")
    e_chk = _engine(eng, n, moduli)
    ok = _patterns(moduli, n, ["top", "alt1"])
    for l, q in enumerate(moduli):
        ok[1, l, 1::2] = _limbs_of(_canonical_edges(q)[0][1])
    dOk = _up(eng, ok)
    e.check_canonical(dOk, 2)
    dB = _up(eng, rns_poly(6, moduli, n, 2)); dR = eng.DeviceBuffer(ok.nbytes)
    e_chk.multiply(dR, dOk, dB, 2)                                                   # clean operands pass
    for l, q in enumerate(moduli):
        for bad in _canonical_edges(q)[1]:
            for pos in (0, n - 1):
                x = ok.copy(); x[1, l, pos] = _limbs_of(bad)
                dBad = _up(eng, x)
                for call in (lambda: e.check_canonical(dBad, 2), lambda: e_chk.multiply(dR, dBad, dB, 2), lambda: e_chk.multiply(dR, dB, dBad, 2),
                             lambda: e_chk.forward(dBad, 2)):
                    with pytest.raises(eng.FheError) as ei:
                        call()
                    assert ei.value.code == -6, (l, bad, pos)


@pytest.mark.parametrize("new_q", [65537, (1 << 64) - 59])
def test_poly_mod_switch_from_a_generic_255_bit_modulus(eng, oracle, new_q):
    old_q = _moduli("g255")[0]
    rng = random.Random(5)
    a = [0, 1, old_q - 1, old_q // 2, old_q // 2 + 1] + _to_ints(_patterns([old_q], 64, ["low"])[0]) + [rng.randrange(old_q) for _ in range(4027)]
    arr = _to_limbs(a)
    dA = _up(eng, arr); dR = eng.DeviceBuffer(arr.nbytes)
    eng.poly_mod_switch(dR, dA, old_q, new_q, len(a))
    got = dR.download(arr.shape)
    assert _to_ints(got) == [((x * new_q + old_q // 2) // old_q) % new_q for x in a]
    assert np.array_equal(got, oracle.poly_mod_switch(arr, old_q, new_q))


def test_negacyclic_reduce_with_a_generic_255_bit_modulus(eng, oracle):
    n = 1024
    q = _moduli("g255")[0]
    d = np.ascontiguousarray(_mixed(4, [q], n, [None, "top", "alt0", "low", None, "alt1", "top", "low"]).reshape(4, 2 * n, 4))   # lower halves minus upper halves
    for poly in d:
        v = _to_ints(poly)
        dD = _up(eng, poly)
        eng.negacyclic_reduce(dD, q, n)
        got = dD.download(poly.shape)
        assert _to_ints(got) == [(v[i] - v[i + n]) % q for i in range(n)] + v[n:]
        assert np.array_equal(got, oracle.negacyclic_reduce(poly, q))
