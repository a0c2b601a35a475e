"""Hoisted rotations (fhe_ct_hoist / fhe_ct_apply_galois_hoisted) at the range edges and on every composed kernel.

tests/test_hoisted.py runs on ntt_math.ntt_primes, the bottom of each width class (see the docstring of test_top_of_range.py), and reaches
relin_mac_perm_kernel only as <F32> with L = 1.  Here:
  0. (CPU) the identity every GPU assertion rests on, test_hoisted._expected, against the definition in include/fhe_hip.h in Python integers;
  1. TOP and SPAN moduli of the four word-sized fields on three paths that must agree bit for bit: the fused LDS kernels (ntt_hoist_kernel /
     ntt_hoist_apply_kernel), the composed path on packed key tables (FHE_HIP_NO_FUSED_HOIST=1: relin_mac_perm_packed_kernel<F>) and the
     composed path on container keys (FHE_HIP_NO_FUSED_KEYSWITCH=1: relin_mac_perm_kernel<F>);
  2. key sets that stay containers by themselves (keys_get_packed in csrc/keyswitch.hip): mixed prime sizes, FP64 above its product limit,
     the two-pass sizes of the 8-byte fields; and L = 2, batch = 2 at N = 2^16 (container kernel) and N = 2^15 (packed kernel, T = 1024);
  3. the full-width class: tests/test_full_width_moduli.py::test_apply_galois_hoisted_on_generic_moduli;
  4. a smaller hoist after a larger one.
fhe_rns_ntt_hoist_bytes tells the path: residues (4 or 8 bytes) on the fused kernels, 32-byte containers on the composed path.  Integer work:
every comparison is np.array_equal on whole arrays."""
import random

import numpy as np
import pytest

import memcheck
import ntt_math as nm
from test_hoisted import _expected
from test_top_of_range import MANY_DIGITS, WIDTH, _cached, _keys, _mixed, _moduli, _patterns, _slots, _w_of
from workload import rns_poly

BITS = (30, 43, 62, 64)
SWITCH = {"default": None, "packed-tables": "FHE_HIP_NO_FUSED_HOIST", "container-keys": "FHE_HIP_NO_FUSED_KEYSWITCH"}
VARIANTS = list(SWITCH)


@pytest.fixture(scope="module")
def eng(pkg):
    if pkg.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")
    return pkg


def _up(pkg, arr):
    return pkg.DeviceBuffer.from_numpy(arr)


def _set_variant(monkeypatch, variant):
    """Before the engine is created: it reads its switches once."""
    if SWITCH[variant]:
        monkeypatch.setenv(SWITCH[variant], "1")


def _hoist_bytes(pkg, e, L, K, n, batch, fused):
    """include/fhe_hip.h: batch * L*K * L * n * sizeof(residue) on the fused kernels, * 32 on the composed path."""
    return batch * L * K * L * n * ((4 if e.width_class == pkg.WIDTH_32 else 8) if fused else 32)


def _odd(n, seed):
    return random.Random(seed).randrange(1, 2 * n) | 1


# ------------------------------------------------------------------------------------------------ 0. CPU: the identity
def _sigma_list(a, q, g):
    """sigma_g on a coefficient list of R_q: x^i -> x^(i g) = +-x^(i g mod n); a negated d becomes q - d and 0 stays 0."""
    n = len(a)
    s = [0] * n
    for i, c in enumerate(a):
        k = i * g % (2 * n)
        s[k % n] = c if k < n else (q - c) % q
    return s


def _header_definition(n, moduli, w, c0, c1, kb, ka, g):
    """out0 = sigma_g(c0) + sum_{j,k} sigma_g(D_{j,k}(c1)) b_{j,k},  out1 = sum_{j,k} sigma_g(D_{j,k}(c1)) a_{j,k}  in R_{q_i}, every limb i;
    D_{j,k} = digit k (w bits) of c1 mod q_j, level j K + k.  Python integers on lists, [batch][L][n]."""
    L = len(moduli)
    K = (max(q.bit_length() for q in moduli) + w - 1) // w
    out0, out1 = [], []
    for b in range(len(c0)):
        r0, r1 = [], []
        for i, q in enumerate(moduli):
            s0, s1 = _sigma_list(c0[b][i], q, g), [0] * n
            for j in range(L):
                for k in range(K):
                    digit = [((v >> (k * w)) & ((1 << w) - 1)) % q for v in c1[b][j]]      # embedded in limb i as a residue of q_i
                    sd = _sigma_list(digit, q, g)
                    s0 = [(x + y) % q for x, y in zip(s0, nm.negacyclic_mul_direct(sd, kb[j * K + k][i], q))]
                    s1 = [(x + y) % q for x, y in zip(s1, nm.negacyclic_mul_direct(sd, ka[j * K + k][i], q))]
            r0.append(s0); r1.append(s1)
        out0.append(r0); out1.append(r1)
    return out0, out1


def _containers(x):
    """Nested lists of integers below 2^256 -> uint64 containers [...][4]."""
    a = np.array(x, dtype=object)
    return np.ascontiguousarray(np.stack([((a >> (64 * k)) & nm.M64).astype(np.uint64) for k in range(4)], axis=-1))


IDENTITY_BASES = ["top30", "top43", "top62", "top64", "span64", "generic100"]


def _identity_moduli(base, n):
    if base == "generic100":
        return nm.generic_ntt_primes(100, n, 2, 100 + n)
    if base == "span64":
        return _moduli("span", 64, n, 2)                     # the largest prime below 2^64 and the smallest above 2^62
    return nm.largest_ntt_primes(int(base[3:]), n, 2)


@pytest.mark.parametrize("n", [16, 32])
@pytest.mark.parametrize("base", IDENTITY_BASES)
def test_hoisted_identity_equals_the_header_definition(oracle, base, n):
    """_expected (sigma_g of the oracle's relinearize with sigma_{g^-1} on the key rows) is what every GPU assertion on hoisted rotations compares
    with; here it is compared with the two formulas of include/fhe_hip.h evaluated literally.  w = 16 and w = the primes' bit length (at most
    64, the widest digit the interface has); batch 2: random, and c1 with every coefficient q - 1 (the largest digits)."""
    moduli = _identity_moduli(base, n); L = len(moduli)
    bits = max(q.bit_length() for q in moduli)
    rng = random.Random(n + bits)

    def poly():
        return [[rng.randrange(q) for _ in range(n)] for q in moduli]

    for w in (16, min(bits, 64)):
        K = (bits + w - 1) // w
        assert oracle.RnsPlan(n, moduli).num_digits(w) == K
        c0 = [poly(), poly()]
        c1 = [poly(), [[q - 1] * n for q in moduli]]
        kb, ka = [poly() for _ in range(L * K)], [poly() for _ in range(L * K)]
        A0, A1 = _containers(c0), _containers(c1)
        KB, KA = [_containers(k) for k in kb], [_containers(k) for k in ka]
        for g in (1, 3, 2 * n - 1, _odd(n, n + w)):
            want0, want1 = _header_definition(n, moduli, w, c0, c1, kb, ka, g)
            got0, got1 = _expected(oracle, n, moduli, w, A0, A1, KB, KA, g)
            assert np.array_equal(got0, _containers(want0)), (w, g)
            assert np.array_equal(got1, _containers(want1)), (w, g)


# ------------------------------------------------------------------------------------------------ 1. top of range, three paths
def _top_case(oracle, bits, kind, n, L, w, batch, elements):
    """Operands in calls of `batch`: c1 = random slots, then all q - 1, q - 1 / 0 and q - 1 / 1 alternating; c0 random with a slot of q - 1.
    The expected values of every element, once for all variants; `got` collects what each variant returned."""
    def make():
        moduli = _moduli(kind, bits, n, L)
        rp = oracle.RnsPlan(n, moduli); K = rp.num_digits(w)
        kb = _keys(moduli, n, L * K, 700); ka = _keys(moduli, n, L * K, 1300)
        c1 = _slots(82, moduli, n, batch, ["top", "alt0", "alt1"])
        c0 = rns_poly(81, moduli, n, c1.shape[0])
        c0[0] = _patterns(moduli, n, ["top"])[0]
        want = {g: _expected(oracle, n, moduli, w, c0, c1, kb, ka, g) for g in elements}
        return dict(moduli=moduli, w=w, K=K, kb=kb, ka=ka, c0=c0, c1=c1, want=want, got={})
    return _cached(("hoist", bits, kind, n, L, w, batch), make)


def _run_top_case(eng, c, n, batch, variant, fused, width):
    moduli, w = c["moduli"], c["w"]; L, K = len(moduli), c["K"]
    e = eng.RnsNttEngine(n, moduli)
    assert e.width_class == width and e.relin_num_digits(w) == K
    gk = e.import_relin_keys(w, [_up(eng, k) for k in c["kb"]], [_up(eng, k) for k in c["ka"]])
    shape = (batch,) + c["c0"].shape[1:]
    got = {}
    for s in range(0, c["c1"].shape[0], batch):
        c0, c1 = np.ascontiguousarray(c["c0"][s:s + batch]), np.ascontiguousarray(c["c1"][s:s + batch])
        d0, d1 = _up(eng, c0), _up(eng, c1)
        o0, o1 = eng.DeviceBuffer(c0.nbytes), eng.DeviceBuffer(c0.nbytes)
        e.hoist(w, d1, batch)
        assert e.hoist_bytes() == _hoist_bytes(eng, e, L, K, n, batch, fused), (variant, "the path this case names did not run")
        for g, (w0, w1) in c["want"].items():
            memcheck.poison(eng, o0); memcheck.poison(eng, o1)
            e.apply_galois_hoisted(gk, g, o0, o1, d0, batch)
            r0, r1 = o0.download(shape), o1.download(shape)
            assert np.array_equal(r0, w0[s:s + batch]), (g, s)
            assert np.array_equal(r1, w1[s:s + batch]), (g, s)
            e.check_canonical(o0, batch); e.check_canonical(o1, batch)
            got[(g, s)] = (r0, r1)
            if g == 1:                                   # sigma_1 is the identity: the plain key switch, bit for bit
                p0, p1 = eng.DeviceBuffer(c0.nbytes), eng.DeviceBuffer(c0.nbytes)
                e.apply_galois(gk, 1, p0, p1, d0, d1, batch)
                assert np.array_equal(p0.download(shape), r0) and np.array_equal(p1.download(shape), r1), s
        assert np.array_equal(d0.download(shape), c0) and np.array_equal(d1.download(shape), c1)     # inputs are read only
    # include/fhe_hip.h: the result never depends on the kernel path
    for other, theirs in c["got"].items():
        for key, (r0, r1) in got.items():
            assert np.array_equal(theirs[key][0], r0) and np.array_equal(theirs[key][1], r1), (variant, other, key)
    c["got"][variant] = got


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("w", ["bits", 16])
@pytest.mark.parametrize("kind", ["top", "span"])
@pytest.mark.parametrize("bits", BITS)
def test_apply_galois_hoisted_at_the_top_primes(eng, oracle, monkeypatch, bits, kind, w, variant):
    """The parameters of test_apply_galois_at_the_top_primes.  The hoist kernel keeps the LAZY forward values ([0, 4q) on the integer fields, up
    to about 12 q as doubles on FP64) and the apply kernel feeds them to pw_mul: with q just under 2^30 / 2^43 / 2^62 / 2^64 about half of them
    have the top bit set.  default = the fused kernels, except w = 64 on the full-range field: its butterflies are canonical, a whole-word
    digit of the larger prime's limb is no residue of the smaller prime (TOP and SPAN alike: q_max > q_min), so the key set stays containers
    by itself and the composed path runs (keys_get_packed)."""
    n, L, batch = 2048, 2, 3
    w = _w_of(bits, w)
    _set_variant(monkeypatch, variant)
    c = _top_case(oracle, bits, kind, n, L, w, batch, (1, eng.galois_element(n, 5), 2 * n - 1))
    fused = variant == "default" and not (bits == 64 and w == 64)
    _run_top_case(eng, c, n, batch, variant, fused, WIDTH[bits])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["default", "container-keys"])
@pytest.mark.parametrize("bits", BITS)
def test_apply_galois_hoisted_with_many_digits_at_the_top_primes(eng, oracle, monkeypatch, bits, variant):
    """MANY_DIGITS of test_top_of_range.py: the longest accumulation chains (FP64: L * K = 44 products as doubles before one reduction)."""
    n, batch = 2048, 1
    w, L = MANY_DIGITS[bits]
    _set_variant(monkeypatch, variant)
    c = _top_case(oracle, bits, "top", n, L, w, batch, (eng.galois_element(n, 5),))
    _run_top_case(eng, c, n, batch, variant, variant == "default", WIDTH[bits])


# ------------------------------------------------------------------------------------------------ 2. keys that stay containers by themselves
def _natural_case(eng, oracle, n, moduli, w, batch, elements, width, fused=False, top_slot=True):
    """No switch.  hoist_bytes in the 32-byte form is the composed path; c1 carries a slot of q - 1 (the largest digits)."""
    L = len(moduli)
    e = eng.RnsNttEngine(n, moduli)
    assert e.width_class == width
    K = e.relin_num_digits(w)
    kb = _keys(moduli, n, L * K, 700); ka = _keys(moduli, n, L * K, 1300)
    gk = e.import_relin_keys(w, [_up(eng, k) for k in kb], [_up(eng, k) for k in ka])
    c0 = rns_poly(81, moduli, n, batch)
    c1 = _mixed(82, moduli, n, ([None] * (batch - 1) + ["top"]) if top_slot else [None] * batch)
    d0, d1 = _up(eng, c0), _up(eng, c1)
    o0, o1 = eng.DeviceBuffer(c0.nbytes), eng.DeviceBuffer(c0.nbytes)
    e.hoist(w, d1, batch)
    assert e.hoist_bytes() == _hoist_bytes(eng, e, L, K, n, batch, fused), "the path this case names did not run"
    for g in elements:
        w0, w1 = _expected(oracle, n, moduli, w, c0, c1, kb, ka, g)
        memcheck.poison(eng, o0); memcheck.poison(eng, o1)
        e.apply_galois_hoisted(gk, g, o0, o1, d0, batch)
        assert np.array_equal(o0.download(c0.shape), w0), g
        assert np.array_equal(o1.download(c0.shape), w1), g
        e.check_canonical(o0, batch); e.check_canonical(o1, batch)
    assert np.array_equal(d0.download(c0.shape), c0) and np.array_equal(d1.download(c0.shape), c1)
    return L, K


def _mixed_bases(n):
    """keys_get_packed: digit_bound = min(2^w, q_max) (q_max for w = 64) must be <= 4 q_min (q_min on the full-range field) for packed tables.
      F32   20-bit + 30-bit + 30-bit, w = 30 (the basis of test_relinearize_mixed_prime_sizes): digit_bound = q_max > 2^29, 4 q_min < 2^22.
      F64   44-bit + 62-bit, w = 62: digit_bound = q_max > 2^61 (q_max < 2^62 = 2^w), 4 q_min < 2^46.
      F64X  63-bit + 64-bit, w = 64: digit_bound = q_max > 2^63, and q_min < 2^63 itself is the limit there.
    Each fails the predicate: the key set keeps its containers and digit_embed_kernel reduces the digits of the wide limb modulo the narrow one."""
    f32 = nm.ntt_primes(20, n, 1) + nm.ntt_primes(30, n, 2)
    f64 = nm.ntt_primes(44, n, 1) + nm.largest_ntt_primes(62, n, 1)
    f64x = nm.ntt_primes(63, n, 1) + nm.largest_ntt_primes(64, n, 1)
    assert max(f32) > 4 * min(f32) and min(1 << 62, max(f64)) > 4 * min(f64) and max(f64x) > min(f64x)
    return {"F32": (f32, 30, 1), "F64": (f64, 62, 2), "F64X": (f64x, 64, 5)}


@pytest.mark.gpu
@pytest.mark.parametrize("field", ["F32", "F64", "F64X"])
def test_apply_galois_hoisted_on_mixed_prime_sizes(eng, oracle, field):
    """relin_mac_perm_kernel<F32 | F64 | F64X> with L > 1 and batch 3, reached without a switch."""
    n, batch = 2048, 3
    moduli, w, width = _mixed_bases(n)[field]
    _natural_case(eng, oracle, n, moduli, w, batch, (3, 2 * n - 1, _odd(n, 7)), width)


@pytest.mark.gpu
@pytest.mark.parametrize("L,w,fused", [(10, 6, True), (12, 7, False)])
def test_fp64_hoisted_rotation_on_both_sides_of_its_product_limit(eng, oracle, L, w, fused):
    """The shapes of test_fp64_key_switch_on_both_sides_of_its_product_limit: L * K = 80 keeps packed tables and the fused kernels (13 MB of
    residues), L * K = 84 keeps containers and runs relin_mac_perm_kernel<F52> (66 MB of containers).  Two elements: the oracle's key switch
    with 84 key rows of 12 limbs is what takes the time."""
    n, batch = 2048, 1
    moduli = _moduli("top", 43, n, L)
    L_, K = _natural_case(eng, oracle, n, moduli, w, batch, (2 * n - 1, _odd(n, L)), WIDTH[43], fused=fused)
    assert L_ * K == (80 if fused else 84)


@pytest.mark.gpu
@pytest.mark.parametrize("n,bits,width", [(32768, 40, 3), (32768, 64, 5), (65536, 62, 2)])
def test_apply_galois_hoisted_at_the_two_pass_sizes_of_the_8_byte_fields(eng, oracle, n, bits, width):
    """The smallest shapes at which relin_mac_perm_kernel<F52 | F64X | F64> meets the two-pass transforms on 8-byte residues (key sets beyond
    the LDS range keep their containers)."""
    _natural_case(eng, oracle, n, nm.largest_ntt_primes(bits, n, 1), 32, 1, (2 * n - 1, _odd(n, bits)), width)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65536, 32768])
def test_apply_galois_hoisted_with_two_limbs_beyond_the_fused_sizes(eng, oracle, n):
    """4-byte residues, L = 2, batch 2.  N = 2^16: container keys, relin_mac_perm_kernel<F32> (kidx = g % per_ct and src = g - 2x + 2 pi_g(x)
    across limb and ciphertext boundaries).  N = 2^15: LDS-resident, so the keys are packed, but lds_hoist leaves the size out:
    relin_mac_perm_packed_kernel<F32> with T = 1024 and the row offset (jk L + i) n for i > 0."""
    _natural_case(eng, oracle, n, nm.largest_ntt_primes(30, n, 2), 16, 2, (3, _odd(n, 11)), 1)


# ------------------------------------------------------------------------------------------------ 4. state across batches
@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["default", "packed-tables"])
def test_a_smaller_hoist_after_a_larger_one(eng, oracle, monkeypatch, variant):
    """Hoist at batch 5, hoist another c1 at batch 2 (the workspace keeps its size: the tail still holds the first decomposition), apply at
    batch 2 inside guard bands; batch 5 is rejected from then on with nothing written."""
    n, L, w, big, batch = 2048, 2, 16, 5, 2
    _set_variant(monkeypatch, variant)
    moduli = _moduli("top", 30, n, L)
    e = eng.RnsNttEngine(n, moduli)
    K = e.relin_num_digits(w)
    kb = _keys(moduli, n, L * K, 700); ka = _keys(moduli, n, L * K, 1300)
    gk = e.import_relin_keys(w, [_up(eng, k) for k in kb], [_up(eng, k) for k in ka])
    first = _mixed(91, moduli, n, [None, "top", "alt0", "alt1", None])
    c0, c1 = _mixed(81, moduli, n, ["top", None]), _mixed(82, moduli, n, [None, "top"])
    g = eng.galois_element(n, 5)
    e.hoist(w, _up(eng, first), big)
    held = e.hoist_bytes()
    assert held == _hoist_bytes(eng, e, L, K, n, big, variant == "default")
    ar = memcheck.GuardedArena(eng, [("c0", c0.nbytes), ("c1", c1.nbytes), ("out0", c0.nbytes), ("out1", c0.nbytes)], L * n * 32)
    ar["c0"].upload(c0); ar["c1"].upload(c1)
    e.hoist(w, ar["c1"], batch)
    assert e.hoist_bytes() == held
    ar["out0"].poison(); ar["out1"].poison()
    e.apply_galois_hoisted(gk, g, ar["out0"], ar["out1"], ar["c0"], batch)
    ar.verify(inputs=("c0", "c1"))
    w0, w1 = _expected(oracle, n, moduli, w, c0, c1, kb, ka, g)
    assert np.array_equal(ar["out0"].download(c0.shape), w0) and np.array_equal(ar["out1"].download(c0.shape), w1)
    assert not np.array_equal(w1, _expected(oracle, n, moduli, w, c0, first[:batch], kb, ka, g)[1])       # the first decomposition would show
    d0, o0, o1 = _up(eng, first), eng.DeviceBuffer(first.nbytes), eng.DeviceBuffer(first.nbytes)
    memcheck.poison(eng, o0); memcheck.poison(eng, o1)
    with pytest.raises(eng.FheError) as ex:
        e.apply_galois_hoisted(gk, g, o0, o1, d0, big)
    assert ex.value.code == -1, str(ex.value)
    assert memcheck.is_poison(o0.download(first.shape)) and memcheck.is_poison(o1.download(first.shape))
    ar.free()
