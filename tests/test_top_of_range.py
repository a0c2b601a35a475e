"""The four word-sized fields at the TOP of their modulus ranges, on every kernel family, against the CPU oracle.

tests/ntt_math.py::ntt_primes returns the smallest primes of a bit width, so the rest of the suite runs every word-sized class at the bottom
of its range, where a lazy value of [0, 4q) almost never has its top bit set and the carry of a full-range 64-bit sum almost never occurs.
Here the moduli are
  TOP  = the largest NTT primes below the class limit (2^30, 2^43, 2^62, 2^64), and
  SPAN = those together with the smallest prime one bit below the limit (2^29+, 2^42+, 2^61+, 2^62+): digits of the wide limb exceed the
         narrow limb's modulus,
and the operands are random (about half of all lazy values now have the top bit set) plus slots of all q - 1, of q - 1 / 0 alternating and of
q - 1 / 1 alternating.  Integer work: every comparison is np.array_equal on whole arrays.

Shapes that differ from a round number one might expect: the word-sized classes exist from n = 2^11 (smaller rings take the 256-bit
container class: test_small_and_degree_one_engines_stay_on_the_container_class), so from_rns runs at n = 2048, not below."""
import numpy as np
import pytest

import ntt_math as nm
from workload import rns_poly

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
BITS = (30, 43, 62, 64)                              # class limits: q < 2^bits
WIDTH = {30: 1, 43: 3, 62: 2, 64: 5}                 # FHE_WIDTH_32 / _52 / _64 / _64X
LOW_BITS = {30: 30, 43: 43, 62: 62, 64: 63}          # ntt_primes(LOW_BITS, ...) = the smallest primes above 2^29, 2^42, 2^61, 2^62
MANY_DIGITS = {30: (4, 2), 43: (4, 4), 62: (8, 2), 64: (8, 2)}     # (w, L) of the many-digit key switch; F52: L * K = 44 products before regroup


@pytest.fixture(scope="module")
def eng(pkg):
    if pkg.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")
    return pkg


def _up(pkg, arr):
    return pkg.DeviceBuffer.from_numpy(arr)


# ------------------------------------------------------------------------------------ moduli and operands
_PRIMES = {}


def _moduli(kind, bits, n, L):
    key = (kind, bits, n, L)
    if key not in _PRIMES:
        if kind == "top":
            _PRIMES[key] = nm.largest_ntt_primes(bits, n, L)
        else:                                        # span: L - 1 primes from the top, one from just below the class limit's top bit
            _PRIMES[key] = nm.largest_ntt_primes(bits, n, L - 1) + nm.ntt_primes(LOW_BITS[bits], n, 1)
        assert all(bits - 1 <= q.bit_length() <= bits for q in _PRIMES[key])
    return _PRIMES[key]


def _patterns(moduli, n, which):
    """[len(which)][L][n][4]: 'top' every coefficient q - 1; 'alt0' q - 1 and 0 alternating; 'alt1' q - 1 and 1 alternating."""
    out = np.zeros((len(which), len(moduli), n, 4), np.uint64)
    for s, name in enumerate(which):
        for l, q in enumerate(moduli):
            if name == "top":
                out[s, l, :, 0] = q - 1
            else:
                out[s, l, ::2, 0] = q - 1
                out[s, l, 1::2, 0] = 0 if name == "alt0" else 1
    return out


def _slots(seed, moduli, n, batch, which):
    """`batch` random slots followed by the pattern slots `which`, padded with random slots to a multiple of `batch`: [groups * batch][L][n][4].
    A call of `batch` units sees group g as slots [g * batch, (g + 1) * batch): the shape of a call stays the one under test, and every pattern
    is carried by one of the calls."""
    pad = (-len(which)) % batch
    parts = [rns_poly(seed, moduli, n, batch), _patterns(moduli, n, which)]
    if pad:
        parts.append(rns_poly(seed + 500, moduli, n, pad))
    return np.ascontiguousarray(np.concatenate(parts))


def _groups(arr, batch):
    return [np.ascontiguousarray(arr[g:g + batch]) for g in range(0, arr.shape[0], batch)]


def _mixed(seed, moduli, n, which):
    """One batch whose slot s is random (which[s] is None) or a pattern."""
    out = rns_poly(seed, moduli, n, len(which))
    for s, name in enumerate(which):
        if name:
            out[s] = _patterns(moduli, n, [name])[0]
    return out


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


def _per_limb(fn, a, b, moduli):
    return np.stack([np.stack([fn(np.ascontiguousarray(a[bi, l]), np.ascontiguousarray(b[bi, l]), l) for l in range(len(moduli))])
                     for bi in range(a.shape[0])])


# ------------------------------------------------------------------------------------ class boundaries
@pytest.mark.parametrize("n", [2048, 16384, 65536])
@pytest.mark.parametrize("bits", BITS)
def test_largest_prime_of_a_class_stays_in_the_class(eng, bits, n):
    """The smallest primes ABOVE 2^30, 2^43 and 2^62 are pinned by CASES in test_gpu_parity.py; this is the other side of each limit."""
    q = nm.largest_ntt_primes(bits, n, 1)[0]
    assert q.bit_length() == bits
    assert eng.RnsNttEngine(n, [q]).width_class == WIDTH[bits]
    assert eng.RnsNttEngine(n, _moduli("span", bits, n, 2)).width_class == WIDTH[bits]


# ------------------------------------------------------------------------------------ transforms and products
TRANSFORM_CASES = [(30, 2048, 3, 3, "throughput"), (30, 2048, 3, 3, "latency"),      # one-workgroup kernels: 32 and 16 coefficients per thread
                   (30, 8192, 2, 1, None),                                            # four workgroups per polynomial (the default for a handful)
                   (30, 32768, 1, 1, None),                                           # 1024-thread workgroups
                   (30, 65536, 1, 1, None)]                                           # two-pass
TRANSFORM_CASES += [(b, n, L, batch, None) for b in (43, 62, 64) for n, L, batch in ((2048, 2, 3), (16384, 1, 1), (32768, 1, 1))]   # LDS, largest LDS size, two-pass


@pytest.mark.parametrize("bits,n,L,batch,form", TRANSFORM_CASES)
def test_transforms_and_products_at_the_top_primes(eng, oracle, monkeypatch, bits, n, L, batch, form):
    moduli = _moduli("top", bits, n, L)
    if form:
        monkeypatch.setenv("FHE_HIP_SMALL_BATCH_POLYS", "0" if form == "throughput" else "1000000")
        monkeypatch.setenv("FHE_HIP_COOP_POLYS", "0")
    e = eng.RnsNttEngine(n, moduli)
    assert e.width_class == WIDTH[bits]
    rp = oracle.RnsPlan(n, moduli)
    A = _slots(1, moduli, n, batch, ["top", "alt0", "alt1"])
    B = _slots(2, moduli, n, batch, ["top", "alt1", "top"])
    want_f, want_i = rp.forward(A, threads=8), rp.inverse(B, threads=8)
    want_m, want_sq = rp.polymul(A, B, threads=8), rp.polymul(A, A, threads=8)
    one = np.ascontiguousarray(B[batch:batch + 1])                                   # the shared operand of multiply_bcast: every coefficient q - 1
    want_bc = rp.polymul(A, np.ascontiguousarray(np.broadcast_to(one, A.shape)), threads=8)
    want_pw = _per_limb(lambda x, y, l: rp.plans[l].pointwise(x, y), A, B, moduli)
    want_add = _per_limb(lambda x, y, l: oracle.batch_add(x, y, moduli[l]), A, B, moduli)
    want_sub = _per_limb(lambda x, y, l: oracle.batch_sub(x, y, moduli[l]), A, B, moduli)
    shape = (batch,) + A.shape[1:]
    dOne = _up(eng, one)
    for g, (a, b) in enumerate(zip(_groups(A, batch), _groups(B, batch))):
        sl = slice(g * batch, (g + 1) * batch)

        def same(buf, want, what):
            assert np.array_equal(buf.download(shape), want[sl]), (what, g)
            e.check_canonical(buf, batch)

        dA, dB, dR = _up(eng, a), _up(eng, b), eng.DeviceBuffer(a.nbytes)
        e.forward(dA, batch); same(dA, want_f, "forward")
        e.inverse(dA, batch); same(dA, A, "inverse of forward")
        dT = _up(eng, b); e.inverse(dT, batch); same(dT, want_i, "inverse")
        e.pointwise(dR, dA, dB, batch); same(dR, want_pw, "pointwise")
        e.multiply(dR, dA, dB, batch); same(dR, want_m, "multiply")
        assert np.array_equal(dA.download(shape), a) and np.array_equal(dB.download(shape), b)
        dC = _up(eng, a); e.multiply(dC, dC, dB, batch); same(dC, want_m, "multiply in place")
        e.multiply(dR, dA, dA, batch); same(dR, want_sq, "square")
        dC = _up(eng, a); e.multiply(dC, dC, dC, batch); same(dC, want_sq, "square in place")
        e.multiply_bcast(dR, dA, dOne, batch); same(dR, want_bc, "multiply_bcast")
        e.poly_add(dR, dA, dB, batch); same(dR, want_add, "poly_add")
        e.poly_sub(dR, dA, dB, batch); same(dR, want_sub, "poly_sub")


# ------------------------------------------------------------------------------------ tensor product
def _ct_case(oracle, bits, kind, n, L, batch):
    def make():
        moduli = _moduli(kind, bits, n, L)
        a0 = _slots(3, moduli, n, batch, ["top", "alt0", "alt1"]); a1 = _slots(4, moduli, n, batch, ["alt1", "top", "alt0"])
        b0 = _slots(5, moduli, n, batch, ["top", "alt1", "top"]); b1 = _slots(6, moduli, n, batch, ["top", "top", "alt0"])
        rp = oracle.RnsPlan(n, moduli)
        return moduli, (a0, a1, b0, b1), rp.ct_multiply(a0, a1, b0, b1, threads=8), rp.ct_multiply(a0, a1, a0, a1, threads=8)
    return _cached(("ct", bits, kind, n, L, batch), make)


def _ct_check(eng, e, ops, want, want_sq, batch):
    shape = (batch,) + ops[0].shape[1:]
    for g in range(ops[0].shape[0] // batch):
        sl = slice(g * batch, (g + 1) * batch)
        host = [np.ascontiguousarray(x[sl]) for x in ops]
        d = [_up(eng, x) for x in host]
        c = [eng.DeviceBuffer(host[0].nbytes) for _ in range(3)]
        e.ct_multiply(c[0], c[1], c[2], d[0], d[1], d[2], d[3], batch)
        for k in range(3):
            assert np.array_equal(c[k].download(shape), want[k][sl]), (k, g)
            e.check_canonical(c[k], batch)
        e.ct_multiply(c[0], c[1], c[2], d[0], d[1], d[0], d[1], batch)               # equal operand pointers: the squaring form where it exists
        for k in range(3):
            assert np.array_equal(c[k].download(shape), want_sq[k][sl]), ("square", k, g)
        for buf, src in zip(d, host):
            assert np.array_equal(buf.download(shape), src)                           # operands preserved


@pytest.mark.parametrize("square_kernels", [True, False])
@pytest.mark.parametrize("kind", ["top", "span"])
@pytest.mark.parametrize("bits", BITS)
def test_tensor_product_at_the_top_primes(eng, oracle, monkeypatch, bits, kind, square_kernels):
    n, L, batch = 2048, 2, 2
    if not square_kernels:
        monkeypatch.setenv("FHE_HIP_NO_SQUARE_KERNELS", "1")
    moduli, ops, want, want_sq = _ct_case(oracle, bits, kind, n, L, batch)
    e = eng.RnsNttEngine(n, moduli)
    assert e.width_class == WIDTH[bits]
    _ct_check(eng, e, ops, want, want_sq, batch)


@pytest.mark.parametrize("forms", ["default", "no-two-launch", "two-launch"])
@pytest.mark.parametrize("bits", [43, 62, 64])
def test_tensor_product_of_the_8_byte_fields_at_the_largest_lds_size(eng, oracle, monkeypatch, bits, forms):
    """N = 2^14, 8-byte residues: no one-launch kernel; two launches, or multiply + multiply + two-product kernel (FHE_HIP_NO_TWO_LAUNCH_CT=1)."""
    n, L, batch = 16384, 1, 1
    if forms == "no-two-launch":
        monkeypatch.setenv("FHE_HIP_NO_TWO_LAUNCH_CT", "1")
    if forms == "two-launch":
        monkeypatch.setenv("FHE_HIP_CT_FORM", "two")
    moduli, ops, want, want_sq = _ct_case(oracle, bits, "top", n, L, batch)
    e = eng.RnsNttEngine(n, moduli)
    _ct_check(eng, e, ops, want, want_sq, batch)


# ------------------------------------------------------------------------------------ key switch
def _w_of(bits, w):
    return bits if w == "bits" else w


def _ks_case(oracle, bits, kind, n, L, w, batch):
    """Keys, accumulators with a slot of q - 1, c2 random and c2 = q - 1 everywhere (the largest digits), and the oracle's results for both."""
    def make():
        moduli = _moduli(kind, bits, n, L)
        rp = oracle.RnsPlan(n, moduli); K = rp.num_digits(w)
        kb = _keys(moduli, n, L * K, 100); ka = _keys(moduli, n, L * K, 900)
        which = [None, "top", "alt1"][:batch]
        c0, c1 = _mixed(51, moduli, n, which), _mixed(52, moduli, n, which[::-1])
        c2s = [rns_poly(53, moduli, n, batch), _patterns(moduli, n, ["top"] * batch)]
        return moduli, K, kb, ka, c0, c1, c2s, [rp.relinearize(w, c0, c1, c2, kb, ka, threads=8) for c2 in c2s]
    return _cached(("ks", bits, kind, n, L, w, batch), make)


def _ks_cases():
    out = []
    for bits in BITS:
        for kind in ("top", "span"):
            out += [(bits, kind, 2048, 2, "bits", 3), (bits, kind, 2048, 2, 16, 3)]
            mw, mL = MANY_DIGITS[bits]
            out.append((bits, kind, 2048, mL, mw, 3 if mL == 2 else 2))               # F52: L * K = 44; batch 2 keeps the oracle short
    out.append((30, "span", 2048, 3, "bits", 3))
    out.append((30, "span", 2048, 3, 16, 3))
    out.append((30, "top", 8192, 2, 16, 1))                                            # few ciphertexts: one workgroup per digit + a combining launch
    out += [(43, "top", 16384, 1, 16, 1), (62, "top", 16384, 1, 16, 1)]               # three-array kernels at the largest LDS size
    return out


RELIN_FORMS = ["default", "single", "containers", "pipeline", "one-launch", "one-launch-containers", "general"]


def _set_relin_form(monkeypatch, form):
    if form == "single":
        monkeypatch.setenv("FHE_HIP_NO_PAIRED_TRANSFORMS", "1")
    elif form == "pipeline":
        monkeypatch.setenv("FHE_HIP_RELIN_PIPELINE", "1")
    elif form in ("one-launch", "one-launch-containers"):
        monkeypatch.setenv("FHE_HIP_SPLIT_PAIRS_POLYS", "0")
        if form == "one-launch-containers":
            monkeypatch.setenv("FHE_HIP_NO_C2_COMPACTION", "1")
    elif form == "containers":
        monkeypatch.setenv("FHE_HIP_NO_C2_COMPACTION", "1")
    elif form == "general":
        monkeypatch.setenv("FHE_HIP_NO_FUSED_KEYSWITCH", "1")


@pytest.mark.parametrize("form", RELIN_FORMS)
@pytest.mark.parametrize("bits,kind,n,L,w,batch", _ks_cases())
def test_relinearize_at_the_top_primes(eng, oracle, monkeypatch, bits, kind, n, L, w, batch, form):
    """default = c2 compacted once; single = digit transforms one at a time; containers / pipeline / one-launch / one-launch-containers = the
    variants of test_relinearize_with_and_without_c2_compaction; general = the unfused composition.  SPAN with w = bits on the full-range field
    takes the general composition by itself (a digit of the wide limb is no residue of the narrow one)."""
    w = _w_of(bits, w)
    _set_relin_form(monkeypatch, form)
    moduli, K, kb, ka, c0, c1, c2s, want = _ks_case(oracle, bits, kind, n, L, w, batch)
    e = eng.RnsNttEngine(n, moduli)
    assert e.width_class == WIDTH[bits] and e.relin_num_digits(w) == K
    rk = e.import_relin_keys(w, [_up(eng, k) for k in kb], [_up(eng, k) for k in ka])
    for c2, (w0, w1) in zip(c2s, want):
        d0, d1, d2 = _up(eng, c0), _up(eng, c1), _up(eng, c2)
        e.relinearize(rk, d0, d1, d2, batch)
        assert np.array_equal(d0.download(c0.shape), w0) and np.array_equal(d1.download(c0.shape), w1)
        assert np.array_equal(d2.download(c0.shape), c2)
        e.check_canonical(d0, batch); e.check_canonical(d1, batch)


def _ctr_case(oracle, bits, kind, n, L, w, batch):
    def make():
        moduli = _moduli(kind, bits, n, L)
        rp = oracle.RnsPlan(n, moduli); K = rp.num_digits(w)
        kb = _keys(moduli, n, L * K, 1100); ka = _keys(moduli, n, L * K, 1900)
        which = [None, "top", "alt1"][:batch]
        ops = [_mixed(61, moduli, n, which), _mixed(62, moduli, n, which[::-1]), _mixed(63, moduli, n, which), _mixed(64, moduli, n, ["top"] * batch)]
        t0, t1, t2 = rp.ct_multiply(*ops, threads=8)
        return moduli, K, kb, ka, ops, rp.relinearize(w, t0, t1, t2, kb, ka, threads=8)
    return _cached(("ctr", bits, kind, n, L, w, batch), make)


@pytest.mark.parametrize("fused", [True, False, "one-launch-keyswitch", "no-four-workgroups", "throughput-kernels"])
@pytest.mark.parametrize("bits,kind,n,L,w,batch", _ks_cases())
def test_ct_multiply_relin_at_the_top_primes(eng, oracle, monkeypatch, bits, kind, n, L, w, batch, fused):
    """The variants of test_ct_multiply_relin_matches_oracle."""
    w = _w_of(bits, w)
    if fused in ("one-launch-keyswitch", "throughput-kernels"):
        monkeypatch.setenv("FHE_HIP_SPLIT_PAIRS_POLYS", "0")
    if fused in ("no-four-workgroups", "throughput-kernels"):
        monkeypatch.setenv("FHE_HIP_COOP_POLYS", "0")
    if fused is False:
        monkeypatch.setenv("FHE_HIP_NO_FUSED_CT_RELIN", "1")
    moduli, K, kb, ka, ops, (w0, w1) = _ctr_case(oracle, bits, kind, n, L, w, batch)
    e = eng.RnsNttEngine(n, moduli)
    rk = e.import_relin_keys(w, [_up(eng, k) for k in kb], [_up(eng, k) for k in ka])
    d = [_up(eng, x) for x in ops]
    o0, o1 = eng.DeviceBuffer(ops[0].nbytes), eng.DeviceBuffer(ops[0].nbytes)
    e.ct_multiply_relin(rk, o0, o1, d[0], d[1], d[2], d[3], batch)
    assert np.array_equal(o0.download(ops[0].shape), w0) and np.array_equal(o1.download(ops[0].shape), w1)
    for buf, src in zip(d, ops):
        assert np.array_equal(buf.download(src.shape), src)
    e.check_canonical(o0, batch); e.check_canonical(o1, batch)


@pytest.mark.parametrize("L,w,fused", [(10, 6, True), (12, 7, False)])
def test_fp64_key_switch_on_both_sides_of_its_product_limit(eng, oracle, L, w, fused):
    """The FP64 field sums its L * K digit x key products as doubles before one reduction: packed tables (the fused kernels) up to L * K = 83,
    the general composition above.  K takes the values ceil(43 / w) only, so the nearest reachable sides are 10 * 8 = 80 and
    12 * 7 = 84.  Both equal the oracle, alone and as one blind-rotation step (whose second component adds to the reduced sum of the first); the
    general composition shows in the digit-polynomial workspace it allocates ((L * K + 2) polynomials of L * n containers)."""
    n, batch, bits = 2048, 1, 43
    moduli = _moduli("top", bits, n, L)
    e = eng.RnsNttEngine(n, moduli); rp = oracle.RnsPlan(n, moduli)
    assert e.width_class == WIDTH[bits]
    K = e.relin_num_digits(w)
    assert L * K == (80 if fused else 84)
    kb = _keys(moduli, n, L * K, 100); ka = _keys(moduli, n, L * K, 900)
    rk = e.import_relin_keys(w, [_up(eng, k) for k in kb], [_up(eng, k) for k in ka])
    c0, c1 = rns_poly(51, moduli, n, batch), _patterns(moduli, n, ["top"])
    for c2 in (rns_poly(53, moduli, n, batch), _patterns(moduli, n, ["top"])):
        d0, d1, d2 = _up(eng, c0), _up(eng, c1), _up(eng, c2)
        e.relinearize(rk, d0, d1, d2, batch)
        w0, w1 = rp.relinearize(w, c0, c1, c2, kb, ka, threads=8)
        assert np.array_equal(d0.download(c0.shape), w0) and np.array_equal(d1.download(c0.shape), w1)
    S = L * n * 32
    assert (e.workspace_bytes() < L * K * S) == fused and (e.workspace_bytes() >= (L * K + 2) * S) == (not fused)
    shifts = np.array([n + 1], dtype=np.uint32)
    dA0, dA1 = _up(eng, c1), _up(eng, c0)
    e.blind_rotate_step(rk, rk, dA0, dA1, eng.DeviceBuffer.from_numpy(shifts), eng.DeviceBuffer(c0.nbytes), eng.DeviceBuffer(c0.nbytes), batch)
    w0, w1 = rp.blind_rotate_step(w, c1, c0, shifts, (kb, ka), (kb, ka), threads=8)
    assert np.array_equal(dA0.download(c0.shape), w0) and np.array_equal(dA1.download(c0.shape), w1)


# ------------------------------------------------------------------------------------ Galois
def _sigma(a, moduli, g):
    """sigma_g on word-sized residues: out[j] = in[i] for i = j g^-1 mod 2n < n, else q - in[i - n], and 0 stays 0."""
    n = a.shape[2]
    i = (np.arange(n, dtype=np.int64) * pow(g, -1, 2 * n)) % (2 * n)
    neg = i >= n
    out = np.ascontiguousarray(a[:, :, i % n, :])
    for l, q in enumerate(moduli):
        v = out[:, l, :, 0]
        out[:, l, :, 0] = np.where(neg[None, :] & (v != 0), np.uint64(q) - v, v)
    return out


@pytest.mark.parametrize("kind", ["top", "span"])
@pytest.mark.parametrize("bits", BITS)
def test_automorphism_at_the_top_primes(eng, bits, kind):
    """Negation q - x at x = 0 (stays 0), x = 1 and x = q - 1 is the edge; elements 3, 2n - 1 and a power of 3."""
    n, L = 2048, 2
    moduli = _moduli(kind, bits, n, L)
    e = eng.RnsNttEngine(n, moduli)
    a = _slots(31, moduli, n, 2, ["top", "alt0", "alt1"])[:5]                         # two random slots and the three patterns: batch 5
    a[0, :, ::97, :] = 0
    d_in, d_out = _up(eng, a), eng.DeviceBuffer(a.nbytes)
    for g in (3, 2 * n - 1, eng.galois_element(n, 77)):
        e.automorphism(d_out, d_in, g, 5)
        assert np.array_equal(d_out.download(a.shape), _sigma(a, moduli, g)), g
        e.check_canonical(d_out, 5)
    assert np.array_equal(d_in.download(a.shape), a)


@pytest.mark.parametrize("variant", ["default", "composed"])
@pytest.mark.parametrize("w", ["bits", 16])
@pytest.mark.parametrize("kind", ["top", "span"])
@pytest.mark.parametrize("bits", BITS)
def test_apply_galois_at_the_top_primes(eng, oracle, monkeypatch, bits, kind, w, variant):
    """fhe_ct_apply_galois == the oracle's relinearize(sigma(c0), 0, sigma(c1)); c1 carries a slot of q - 1: the largest digits after sigma."""
    n, L, batch = 2048, 2, 3
    w = _w_of(bits, w)
    if variant == "composed":
        monkeypatch.setenv("FHE_HIP_NO_FUSED_GALOIS", "1")
    g = eng.galois_element(n, 5)

    def make():
        moduli = _moduli(kind, bits, n, L)
        rp = oracle.RnsPlan(n, moduli); K = rp.num_digits(w)
        kb = _keys(moduli, n, L * K, 700); ka = _keys(moduli, n, L * K, 1300)
        c0, c1 = _mixed(81, moduli, n, ["top", None, "alt0"]), _mixed(82, moduli, n, [None, "top", "alt1"])
        return moduli, kb, ka, c0, c1, [rp.relinearize(w, _sigma(c0, moduli, x), np.zeros_like(c0), _sigma(c1, moduli, x), kb, ka, threads=8) for x in (g, 2 * n - 1)]
    moduli, kb, ka, c0, c1, want = _cached(("galois", bits, kind, w), make)
    e = eng.RnsNttEngine(n, moduli)
    gk = e.import_relin_keys(w, [_up(eng, k) for k in kb], [_up(eng, k) for k in ka])
    d0, d1 = _up(eng, c0), _up(eng, c1)
    o0, o1 = eng.DeviceBuffer(c0.nbytes), eng.DeviceBuffer(c0.nbytes)
    for x, (w0, w1) in zip((g, 2 * n - 1), want):
        e.apply_galois(gk, x, o0, o1, d0, d1, batch)
        assert np.array_equal(o0.download(c0.shape), w0) and np.array_equal(o1.download(c0.shape), w1), x
        e.check_canonical(o0, batch); e.check_canonical(o1, batch)
    assert np.array_equal(d0.download(c0.shape), c0) and np.array_equal(d1.download(c0.shape), c1)


# ------------------------------------------------------------------------------------ blind rotation
@pytest.mark.parametrize("kind", ["top", "span"])
@pytest.mark.parametrize("bits", BITS)
def test_monomial_mul_sub_at_the_top_primes(eng, oracle, bits, kind):
    """(X^a - 1) p: q - 1 minus 0, 0 minus q - 1 and -(q - 1) - (q - 1) all occur on the pattern slots; every shift meets every kind of slot."""
    n, L, batch = 2048, 2, 6
    moduli = _moduli(kind, bits, n, L)
    e = eng.RnsNttEngine(n, moduli); rp = oracle.RnsPlan(n, moduli)
    a = _mixed(601, moduli, n, [None, "top", "alt0", "alt1", None, "top"])
    shifts = [0, 1, n - 1, n, n + 1, 2 * n - 1]
    dA, dT = _up(eng, a), eng.DeviceBuffer(a.nbytes)
    for rot in range(0, 6, 2):
        sh = np.array(shifts[rot:] + shifts[:rot], dtype=np.uint32)
        e.monomial_mul_sub(dT, dA, eng.DeviceBuffer.from_numpy(sh), batch)
        assert np.array_equal(dT.download(a.shape), rp.monomial_mul_sub(a, sh)), rot
        e.check_canonical(dT, batch)


@pytest.mark.parametrize("fused", [True, False, "single", "containers", "split", "no-prerotation", "one-workgroup-per-limb"])
@pytest.mark.parametrize("w", ["bits", 16])
@pytest.mark.parametrize("kind", ["top", "span"])
@pytest.mark.parametrize("bits", BITS)
def test_blind_rotate_at_the_top_primes(eng, oracle, monkeypatch, bits, kind, w, fused):
    """Two steps, three accumulators (random, all q - 1, alternating): (X^a - 1) acc reaches 2q - 2 before it is reduced.  The variants of
    test_blind_rotate_loop_matches_oracle."""
    n, L, batch, steps = 2048, 2, 3, 2
    w = _w_of(bits, w)
    env = {False: "FHE_HIP_NO_FUSED_BLIND_ROTATE", "single": "FHE_HIP_NO_PAIRED_TRANSFORMS", "split": "FHE_HIP_SPLIT_KEYSWITCH",
           "containers": "FHE_HIP_NO_COMPACT_BLIND_ROTATE", "no-prerotation": "FHE_HIP_NO_PREROTATION"}
    if fused in env:
        monkeypatch.setenv(env[fused], "1")
    elif fused == "one-workgroup-per-limb":
        monkeypatch.setenv("FHE_HIP_SPLIT_PAIRS_POLYS", "0")

    def make():
        moduli = _moduli(kind, bits, n, L)
        rp = oracle.RnsPlan(n, moduli); K = rp.num_digits(w)
        rows = [[(_keys(moduli, n, L * K, 7000 + 100 * c + 1000 * s), _keys(moduli, n, L * K, 8000 + 100 * c + 1000 * s)) for c in range(2)] for s in range(steps)]
        a0, a1 = _mixed(611, moduli, n, [None, "top", "alt0"]), _mixed(612, moduli, n, ["top", None, "alt1"])
        shifts = np.array([[1, n, 2 * n - 1], [n - 1, 0, n + 1]], dtype=np.uint32)
        return moduli, rows, a0, a1, shifts, rp.blind_rotate(w, a0, a1, shifts, [r[0] for r in rows], [r[1] for r in rows], threads=8)
    moduli, rows, a0, a1, shifts, (w0, w1) = _cached(("br", bits, kind, w), make)
    e = eng.RnsNttEngine(n, moduli)
    imported = [[e.import_relin_keys(w, [_up(eng, k) for k in kb], [_up(eng, k) for k in ka]) for kb, ka in r] for r in rows]
    dA0, dA1 = _up(eng, a0), _up(eng, a1)
    dT0, dT1 = eng.DeviceBuffer(a0.nbytes), eng.DeviceBuffer(a0.nbytes)
    e.blind_rotate([r[0] for r in imported], [r[1] for r in imported], dA0, dA1, eng.DeviceBuffer.from_numpy(shifts), dT0, dT1, batch)
    assert np.array_equal(dA0.download(a0.shape), w0) and np.array_equal(dA1.download(a0.shape), w1)
    e.check_canonical(dA0, batch); e.check_canonical(dA1, batch)


# ------------------------------------------------------------------------------------ RNS entry and exit
RNS_L = {30: 4, 43: 5, 62: 3, 64: 3}                                                  # the product of the moduli stays below 2^255


@pytest.mark.parametrize("word", [True, False])
@pytest.mark.parametrize("bits", BITS)
def test_to_rns_from_rns_at_the_top_primes(eng, oracle, monkeypatch, bits, word):
    import random
    if not word:
        monkeypatch.setenv("FHE_HIP_NO_WORD_CONVERSIONS", "1")
    n, L, batch = 2048, RNS_L[bits], 1
    moduli = _moduli("top", bits, n, L)
    Q = 1
    for q in moduli:
        Q *= q
    assert Q < 1 << 255
    e = eng.RnsNttEngine(n, moduli); rp = oracle.RnsPlan(n, moduli)
    assert e.width_class == WIDTH[bits]
    rng = random.Random(bits)
    edge = [0, 1, M64, 1 << 64, (1 << 256) - 1]
    for q in moduli:
        k = ((1 << 255) // q)
        edge += [q - 1, q, q + 1, k * q - 1, k * q, k * q + 1, (2 * k - 1) * q - 1, (2 * k - 1) * q + 1]      # multiples of q next to 2^255 and to 2^256
    vals = edge + [rng.getrandbits(256) for _ in range(n - len(edge))]
    V = oracle.to_limbs(vals).reshape(batch, n, 4)
    dR = eng.DeviceBuffer(batch * L * n * 32)
    e.to_rns(dR, _up(eng, V), batch)
    R = dR.download((batch, L, n, 4))
    assert np.array_equal(R, rp.to_rns(V))
    assert oracle.from_limbs(R[0, :, :len(edge)]) == [v % q for q in moduli for v in edge]
    e.check_canonical(dR, batch)
    # exit: values below Q, with 0, 1, Q - 1 (every residue q - 1) and the multiples of Q / q_l next to them
    vals = [0, 1, Q - 1, Q - 2] + [Q // q for q in moduli] + [Q - Q // q for q in moduli]
    vals += [rng.randrange(Q) for _ in range(n - len(vals))]
    V = oracle.to_limbs(vals).reshape(batch, n, 4)
    e.to_rns(dR, _up(eng, V), batch)
    R = dR.download((batch, L, n, 4))
    assert [int(R[0, l, 2, 0]) for l in range(L)] == [q - 1 for q in moduli]
    dBack = eng.DeviceBuffer(V.nbytes)
    e.from_rns(dBack, dR, batch)
    assert np.array_equal(dBack.download(V.shape), V) and np.array_equal(rp.from_rns(R), V)


@pytest.mark.parametrize("word", [True, False])
@pytest.mark.parametrize("bits", BITS)
def test_rescale_drop_last_at_the_top_primes(eng, oracle, monkeypatch, bits, word):
    """Rounded division by the last prime: the centred remainder changes sign between (q_last - 1) / 2 and (q_last + 1) / 2."""
    if not word:
        monkeypatch.setenv("FHE_HIP_NO_WORD_CONVERSIONS", "1")
    n, L, batch = 2048, 3, 3
    moduli = _moduli("top", bits, n, L)
    e = eng.RnsNttEngine(n, moduli); rp = oracle.RnsPlan(n, moduli)
    c = _mixed(401, moduli, n, [None, "top", "alt1"])
    ql = moduli[-1]
    c[0, L - 1, 0:8, 0] = [0, 1, (ql - 1) // 2, (ql + 1) // 2, (ql - 1) // 2 - 1, (ql + 1) // 2 + 1, ql - 1, ql - 2]
    for l, q in enumerate(moduli[:-1]):                                                # the rounding edge against residues 0 and q - 1 as well as random ones
        c[0, l, 0:8:2, 0] = q - 1
        c[0, l, 8:16, 0] = 0
    c[0, L - 1, 8:16, 0] = c[0, L - 1, 0:8, 0]
    c[2, L - 1, :, 0] = np.where(np.arange(n) % 2 == 0, (ql - 1) // 2, (ql + 1) // 2).astype(np.uint64)
    dIn = _up(eng, c); dOut = eng.DeviceBuffer(batch * (L - 1) * n * 32)
    e.rescale_drop_last(dOut, dIn, batch)
    assert np.array_equal(dOut.download((batch, L - 1, n, 4)), rp.rescale_drop_last(c))
    assert np.array_equal(dIn.download(c.shape), c)
    eng.RnsNttEngine(n, moduli[:-1]).check_canonical(dOut, batch)


@pytest.mark.parametrize("word", [True, False])
@pytest.mark.parametrize("bits2", BITS)
@pytest.mark.parametrize("bits", BITS)
def test_fast_base_convert_between_top_primes(eng, oracle, monkeypatch, bits, bits2, word):
    """TOP of one class into TOP of every word-sized class (the same class included: only there does the streaming kernel on the field type run).
    Every residue q - 1 puts the overshoot alpha of the fast conversion at its maximum L - 1."""
    if not word:
        monkeypatch.setenv("FHE_HIP_NO_WORD_CONVERSIONS", "1")
    n, L, Lp, batch = 2048, 3, 2, 2
    src = _moduli("top", bits, n, L)
    dst = [p for p in _moduli("top", bits2, n, L + Lp) if p not in src][:Lp]
    e, t = eng.RnsNttEngine(n, src), eng.RnsNttEngine(n, dst)
    S, D = oracle.RnsPlan(n, src), oracle.RnsPlan(n, dst)
    x = _mixed(501, src, n, [None, "top"])
    for l, q in enumerate(src):
        x[0, l, :4, 0] = [0, q - 1, 1, q - 2]
    dX = _up(eng, x); dY = eng.DeviceBuffer(batch * Lp * n * 32)
    e.fast_base_convert(t, dY, dX, batch)
    assert np.array_equal(dY.download((batch, Lp, n, 4)), S.fast_base_convert(D, x))
    t.check_canonical(dY, batch)


# ------------------------------------------------------------------------------------ samplers and scans
@pytest.mark.parametrize("kind", ["top", "span"])
@pytest.mark.parametrize("bits", BITS)
def test_rns_samplers_at_the_top_primes(eng, oracle, bits, kind):
    """q = 2^64 - delta: the uniform sampler's rejection loop accepts almost every draw (2^63 + delta rejects half of them); -m embeds as q - m."""
    n, L, batch = 2048, 2, 3
    moduli = _moduli(kind, bits, n, L)
    e = eng.RnsNttEngine(n, moduli); rp = oracle.RnsPlan(n, moduli)
    d = eng.DeviceBuffer(batch * L * n * 32); shape = (batch, L, n, 4)
    e.sample_uniform(d, 2024, batch)
    assert np.array_equal(d.download(shape), rp.sample_uniform(2024, batch))
    e.check_canonical(d, batch)
    for p in (0.5, 1.0):
        e.sample_ternary(d, p, 1234, batch)
        got = d.download(shape)
        assert np.array_equal(got, rp.sample_ternary(p, 1234, batch))
        for l, q in enumerate(moduli):
            assert set(np.unique(got[:, l, :, 0]).tolist()) <= {0, 1, q - 1} and (got[:, l, :, 0] == np.uint64(q - 1)).any()
        e.check_canonical(d, batch)
    assert eng.gaussian_cdt(3.2) == oracle.gaussian_cdt(3.2)
    e.sample_gaussian(d, 3.2, 99, batch)
    got = d.download(shape)
    assert np.array_equal(got, rp.sample_gaussian(3.2, 99, batch))
    assert (got[:, 0, :, 0] > np.uint64(moduli[0] - 40)).any()                       # negative samples are there
    e.check_canonical(d, batch)


@pytest.mark.parametrize("kind", ["top", "span"])
@pytest.mark.parametrize("bits", BITS)
def test_check_canonical_at_the_top_primes(eng, bits, kind):
    """q - 1 passes; q, the all-ones residue word and 2^64 - 1 are rejected (on the full-range field q and 2^64 - 1 are both real 64-bit values
    above the modulus; on the 4-byte field 2^32 - 1 is the all-ones residue and 2^64 - 1 has a non-zero upper half besides)."""
    n, L = 2048, 2
    moduli = _moduli(kind, bits, n, L)
    e = eng.RnsNttEngine(n, moduli)
    ok = _patterns(moduli, n, ["top", "alt1"])
    e.check_canonical(_up(eng, ok), 2)
    for l, q in enumerate(moduli):
        for bad in {q, q + 1, M64, (1 << 32) - 1 if bits == 30 else M64 - 1}:
            for pos in (0, n - 1):
                x = ok.copy(); x[1, l, pos, 0] = bad
                with pytest.raises(eng.FheError) as ei:
                    e.check_canonical(_up(eng, x), 2)
                assert ei.value.code == -6, (l, bad, pos)


@pytest.mark.parametrize("bits", BITS)
def test_check_inputs_switch_at_the_top_primes(eng, monkeypatch, bits):
    """FHE_HIP_CHECK_INPUTS=1 as in test_check_inputs_switch_rejects_noncanonical_operands, with a coefficient equal to a top-of-class q."""
    n, L = 2048, 2
    moduli = _moduli("top", bits, n, L)
    monkeypatch.setenv("FHE_HIP_CHECK_INPUTS", "1")
    e = eng.RnsNttEngine(n, moduli)
    a = _patterns(moduli, n, ["top"]); b = rns_poly(6, moduli, n, 1)
    dA, dB, dR = _up(eng, a), _up(eng, b), eng.DeviceBuffer(a.nbytes)
    e.multiply(dR, dA, dB, 1)                                    # every coefficient q - 1 is clean
    bad = a.copy(); bad[0, L - 1, 7, 0] = moduli[L - 1]
    up = a.copy(); up[0, 0, 100, 2] = 1                         # non-zero upper word
    for arr in (bad, up):
        dBad = _up(eng, arr)
        for call in (lambda: e.multiply(dR, dBad, dB, 1), lambda: e.multiply(dR, dA, dBad, 1), lambda: e.forward(dBad, 1),
                     lambda: e.ct_multiply(dR, eng.DeviceBuffer(a.nbytes), eng.DeviceBuffer(a.nbytes), dA, dBad, dB, dA, 1)):
            with pytest.raises(eng.FheError) as ei:
                call()
            assert ei.value.code == -6
