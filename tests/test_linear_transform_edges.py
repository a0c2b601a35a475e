"""Hoisted linear transform (fhe_ct_linear_transform_hoisted) on every fused kernel instance, both halves of block_map, and at the edges.

tests/test_linear_transform.py pins the API contract on ntt_math.ntt_primes (the bottom of each width class), at batch <= 3, on six of the
sixteen instances of ntt_hoist_fwd_kernel / ntt_hoist_lincomb_kernel (csrc/hoist_lincomb.hip.h) and on one of the composed routes.  Here:
  0. (CPU) the two things every GPU assertion rests on: test_linear_transform._weighted_sum (and with it _add_mod) against the definition in
     include/fhe_hip.h in Python integers, and the closed form of part 6 against _weighted_sum;
  1. grids of ntt_hoist_lincomb_kernel that reach the round-robin half of block_map (ntt_lds.hip.h), alone and with a tail, LH = 2, 3, 4, 6;
  2. all sixteen fused instances (F32 / F52 / F64 / F64X at N = 2^11 .. 2^14) on TOP primes, and N = 2^11 on SPAN moduli;
  3. the accumulation length: FP64 on both sides of its product limit (L K = 80 fused, 84 composed by itself) and MANY_DIGITS;
  4. the composed routes on container keys: FHE_HIP_NO_FUSED_KEYSWITCH=1, mixed prime sizes, w = 64 on the full-range field;
  5. term order: keyless first, keyless only, one keyed term, keyless last, two keyless terms;
  6. operands that are constants in the EVALUATION domain (every lane of the kernel sees q - 1 at once), with a closed form;
  7. workspace state: a smaller hoist after a larger one, d_lin growing between two transform objects that alternate on one engine.
fhe_rns_ntt_hoist_bytes tells the hoist's path (residues: fused, 32-byte containers: composed) and fhe_rns_ntt_workspace_bytes after
fhe_linear_transform_reserve the transform's.  Integer work: every comparison is np.array_equal on whole arrays.  Every GPU call has its
outputs poisoned first, both outputs scanned for left-over poison and for non-canonical residues, and its inputs compared afterwards."""
import random

import numpy as np
import pytest

import memcheck
import ntt_math as nm
from test_hoisted_edges import IDENTITY_BASES, SWITCH, _containers, _header_definition, _hoist_bytes, _identity_moduli, _mixed_bases, _odd, _set_variant, _up
from test_hoisted_edges import eng  # noqa: F401  (the module's fixture: fails, not skips, without a device)
from test_linear_transform import _build, _weighted_sum
from test_top_of_range import MANY_DIGITS, WIDTH, _cached, _keys, _mixed, _moduli
from workload import rns_poly

BITS = (30, 43, 62, 64)
NOT_RUN = "the path this case names did not run"


# ------------------------------------------------------------------------------------------------ helpers
def _terms(moduli, n, K, spec, seed=500):
    """spec: (g, 'A' | 'B' | None) per term -> (g, (kb, ka) | None, p) as _weighted_sum and _build take them; one host key pair per name."""
    L, sets = len(moduli), {}
    for _, name in spec:
        if name and name not in sets:
            s = 700 if name == "A" else 2100
            sets[name] = (_keys(moduli, n, L * K, s), _keys(moduli, n, L * K, s + 600))
    return [(g, sets.get(name), rns_poly(seed + t, moduli, n, 1)[0]) for t, (g, name) in enumerate(spec)]


def _keyless(terms):
    return any(keys is None for _, keys, _ in terms)


def _half(bits):
    return (bits + 1) // 2                               # w = ceil(bits / 2): K = 2


def _operands(moduli, n, batch):
    """Random, every batch element different; from batch 2 on c0 opens and c1 closes with the slot of all q - 1 (the largest digits)."""
    if batch == 1:
        return rns_poly(81, moduli, n, 1), rns_poly(82, moduli, n, 1)
    return _mixed(81, moduli, n, ["top"] + [None] * (batch - 1)), _mixed(82, moduli, n, [None] * (batch - 1) + ["top"])


def _poison_left(arr):
    """Some 32-byte container is still the poison of memcheck.poison: a workgroup did not write it."""
    return bool((np.ascontiguousarray(arr).view(np.uint8).reshape(-1, 32) == memcheck.POISON_BYTE).all(axis=1).any())


def _transform(pkg, e, lt, w, c0, c1, keyless, arena=False, hoist=True):
    """One call under the standing checks of this module; hoist=False: the engine already keeps the decomposition of this c1.  arena: all
    four buffers carved out of one allocation between guard bands (memcheck.GuardedArena).  Returns the two outputs."""
    batch = c0.shape[0]
    if arena:
        ar = memcheck.GuardedArena(pkg, [("c0", c0.nbytes), ("c1", c1.nbytes), ("out0", c0.nbytes), ("out1", c0.nbytes)], c0.nbytes // batch)
        d0, d1, o0, o1 = ar["c0"].upload(c0), ar["c1"].upload(c1), ar["out0"], ar["out1"]
    else:
        d0, d1, o0, o1 = _up(pkg, c0), _up(pkg, c1), pkg.DeviceBuffer(c0.nbytes), pkg.DeviceBuffer(c0.nbytes)
    if hoist:
        e.hoist(w, d1, batch)
    memcheck.poison(pkg, o0); memcheck.poison(pkg, o1)
    e.linear_transform_hoisted(lt, o0, o1, d0, d1 if keyless else None, batch)
    if arena:
        ar.verify(inputs=("c0", "c1"))
    else:
        assert np.array_equal(d0.download(c0.shape), c0) and np.array_equal(d1.download(c0.shape), c1)      # inputs are read only
    got = [o0.download(c0.shape), o1.download(c0.shape)]
    assert not _poison_left(got[0]) and not _poison_left(got[1])
    e.check_canonical(o0, batch); e.check_canonical(o1, batch)
    if arena:
        ar.free()
    return got


def _residue_bytes(pkg, e):
    return 4 if e.width_class == pkg.WIDTH_32 else 8


def _fused_sizes(pkg, e, L, n, batch, keyless):
    """What a fresh engine holds after fhe_linear_transform_reserve on the fused path (include/fhe_hip.h): the compact image of c1 that
    fhe_ct_hoist reads (need_hoist in csrc/keyswitch.hip) and c0^ (c1^ too with a keyless term) of ntt_hoist_fwd_kernel (lincomb_scratch)."""
    return batch * L * n * _residue_bytes(pkg, e) * (1 + (2 if keyless else 1))


def _reserve_names_the_path(pkg, e, lt, L, K, n, batch, keyless, fused):
    """On an engine that has only imported keys and built the object.  Fused: both sizes in residue form, as equalities.  Composed: the hoist
    workspace in 32-byte form."""
    assert e.workspace_bytes() == 0 and e.hoist_bytes() == 0
    e.linear_transform_reserve(lt, batch)
    assert e.hoist_bytes() == _hoist_bytes(pkg, e, L, K, n, batch, fused), NOT_RUN
    if fused:
        assert e.workspace_bytes() == _fused_sizes(pkg, e, L, n, batch, keyless), NOT_RUN


def _case(oracle, key, n, moduli, w, batch, spec):
    """Terms, operands and the oracle's answer for one row, computed once for all its variants; `got` collects what each variant returned."""
    def make():
        K = oracle.RnsPlan(n, moduli).num_digits(w)
        terms = _terms(moduli, n, K, spec)
        c0, c1 = _operands(moduli, n, batch)
        return dict(moduli=moduli, w=w, K=K, terms=terms, c0=c0, c1=c1, want=_weighted_sum(oracle, n, moduli, w, c0, c1, terms), got={})
    return _cached(("lincomb",) + key, make)


def _run_case(pkg, c, n, variant, fused, width, arena=False):
    """The engine under `variant` (its switch is set already), the path assertion, one call, the oracle, and every earlier variant of the row
    bit for bit (include/fhe_hip.h: the result never depends on the kernel path)."""
    moduli, w, K, terms, c0, c1 = c["moduli"], c["w"], c["K"], c["terms"], c["c0"], c["c1"]
    L, batch, keyless = len(moduli), c0.shape[0], _keyless(c["terms"])
    e = pkg.RnsNttEngine(n, moduli)
    assert e.width_class == width and e.relin_num_digits(w) == K
    lt, _sets = _build(pkg, e, w, terms)
    _reserve_names_the_path(pkg, e, lt, L, K, n, batch, keyless, fused)
    got = _transform(pkg, e, lt, w, c0, c1, keyless)
    assert e.hoist_bytes() == _hoist_bytes(pkg, e, L, K, n, batch, fused), NOT_RUN
    if fused:
        assert e.workspace_bytes() == _fused_sizes(pkg, e, L, n, batch, keyless), NOT_RUN
    assert np.array_equal(got[0], c["want"][0]) and np.array_equal(got[1], c["want"][1]), variant
    if arena:
        again = _transform(pkg, e, lt, w, c0, c1, keyless, arena=True)
        assert np.array_equal(again[0], c["want"][0]) and np.array_equal(again[1], c["want"][1]), (variant, "arena")
    for other, theirs in c["got"].items():
        assert np.array_equal(theirs[0], got[0]) and np.array_equal(theirs[1], got[1]), (variant, other)
    c["got"][variant] = got


# ------------------------------------------------------------------------------------------------ 0. CPU: what the GPU assertions rest on
def _lincomb_definition(n, moduli, w, c0, c1, terms):
    """include/fhe_hip.h literally: out = sum_t p_t * hoisted_rotation(ct, g_t), a keyless term p_t * (c0, c1).  Python integers on lists
    [batch][L][n]; terms: (g, (kb, ka) | None, p) with p one [L][n] polynomial."""
    tot = None
    for g, keys, p in terms:
        r = (c0, c1) if keys is None else _header_definition(n, moduli, w, c0, c1, keys[0], keys[1], g)
        prod = [[[nm.negacyclic_mul_direct(p[i], x[b][i], q) for i, q in enumerate(moduli)] for b in range(len(c0))] for x in r]
        tot = prod if tot is None else [[[[(u + v) % q for u, v in zip(tot[h][b][i], prod[h][b][i])] for i, q in enumerate(moduli)]
                                         for b in range(len(c0))] for h in range(2)]
    return tot


def _constant(moduli, n):
    """[L][n][4]: the polynomial whose only non-zero coefficient is the constant term q_l - 1.  Its forward transform holds q_l - 1 in every
    evaluation slot, and sigma_g fixes it for every g."""
    out = np.zeros((len(moduli), n, 4), np.uint64)
    for l, q in enumerate(moduli):
        out[l, 0] = [((q - 1) >> (64 * k)) & nm.M64 for k in range(4)]
    return out


def _constant_terms(moduli, n, K, elements):
    """Every key row and every plaintext the constant q_l - 1; elements: g per term, None for the keyless one.  One key pair for all."""
    keys = ([_constant(moduli, n)] * (len(moduli) * K),) * 2
    return [(g or 1, keys if g else None, _constant(moduli, n)) for g in elements]


def _constant_closed_form(moduli, n, w, K, keyed, keyless):
    """c0 = c1 = every key row = every plaintext = -1 (the constant q - 1 of each limb).  In limb i, with D = sum_{j,k} digit k of q_j - 1:
    a keyed term is  -1 * (-1 + D * -1, D * -1) = (1 + D, D),  a keyless one  -1 * (-1, -1) = (1, 1),  so
        out0 = keyed (1 + D) + keyless,   out1 = keyed D + keyless   (mod q_i), constants again: [2][L][n][4] for one batch element."""
    D = sum(((q - 1) >> (k * w)) & ((1 << w) - 1) for q in moduli for k in range(K))
    out = np.zeros((2, len(moduli), n, 4), np.uint64)
    for i, q in enumerate(moduli):
        for h, v in enumerate(((keyed * (1 + D) + keyless) % q, (keyed * D + keyless) % q)):
            out[h, i, 0] = [(v >> (64 * k)) & nm.M64 for k in range(4)]
    return out


@pytest.mark.parametrize("n", [16, 32])
@pytest.mark.parametrize("base", IDENTITY_BASES)
def test_weighted_sum_equals_the_header_definition(oracle, base, n):
    """_weighted_sum is what every GPU assertion on the linear transform compares with.  Its sum over the terms is _add_mod, whose branch for
    q above 2^63 (the 64-bit sum wraps) no CPU test reaches otherwise: top64 and span64 do, generic100 takes its Python-integer branch.
    G = 4: element 1 with a key, the keyless term, 2n - 1 with a second key set and a random element; w = 16 and w = the primes' bit length (at
    most 64); batch 2: random, and c1 with every coefficient q - 1."""
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
        A, B = [([poly() for _ in range(L * K)], [poly() for _ in range(L * K)]) for _ in range(2)]
        terms = [(1, A, poly()), (1, None, poly()), (2 * n - 1, B, poly()), (_odd(n, n + w), A, poly())]
        want = _lincomb_definition(n, moduli, w, c0, c1, terms)
        packed = {id(k): ([_containers(r) for r in k[0]], [_containers(r) for r in k[1]]) for k in (A, B)}
        got = _weighted_sum(oracle, n, moduli, w, _containers(c0), _containers(c1), [(g, k and packed[id(k)], _containers(p)) for g, k, p in terms])
        assert np.array_equal(got[0], _containers(want[0])), w
        assert np.array_equal(got[1], _containers(want[1])), w


@pytest.mark.parametrize("base", IDENTITY_BASES)
def test_constant_closed_form_equals_the_weighted_sum(oracle, base):
    """The closed form that part 6 compares the device with, against _weighted_sum: n = 32, four keyed terms and one keyless."""
    n = 32
    moduli = _identity_moduli(base, n)
    bits = max(q.bit_length() for q in moduli)
    for w in (16, min(bits, 64)):
        K = oracle.RnsPlan(n, moduli).num_digits(w)
        terms = _constant_terms(moduli, n, K, [3, _odd(n, w), None, 2 * n - 1, _odd(n, w + 1)])
        c = np.ascontiguousarray(_constant(moduli, n)[None])
        got = _weighted_sum(oracle, n, moduli, w, c, c.copy(), terms)
        want = _constant_closed_form(moduli, n, w, K, keyed=4, keyless=1)
        assert np.array_equal(got[0][0], want[0]) and np.array_equal(got[1][0], want[1]), w


# ------------------------------------------------------------------------------------------------ 1. both branches of block_map
BLOCK_MAP_ROWS = [(30, 3, 11, True),      # LH = 3, grid 33 = 24 round-robin + 9 linear; once more inside guard bands
                  (30, 2, 17, False),     # grid 34 = 32 + 2
                  (30, 2, 8, False),      # grid 16: all round-robin, no tail
                  (62, 2, 11, False),     # SPLIT, LH = 4, grid 44 = 32 + 12
                  (43, 3, 9, False),      # SPLIT, LH = 6, grid 54 = 48 + 6
                  (64, 1, 9, False)]      # SPLIT, LH = 2, grid 18 = 16 + 2


@pytest.mark.gpu
@pytest.mark.parametrize("bits,L,batch,arena", BLOCK_MAP_ROWS)
def test_lincomb_grids_on_both_branches_of_block_map(eng, oracle, bits, L, batch, arena):
    """block_map(LH) deals the workgroups bid < (grid / 8 LH) 8 LH round-robin over the XCDs and maps the rest linearly; LH = L, or 2 L on the
    SPLIT form (8-byte residues), where the unit also carries the output component.  Batch <= 3 never leaves the linear branch.  Every batch
    element holds different random data, so a map that is no bijection leaves poison or another element's result.  n = 2048, TOP primes,
    K = 2, one keyed term with a random element and one keyless term."""
    n, w = 2048, _half(bits)
    LH = L * (1 if bits == 30 else 2)
    assert (batch * LH) // (8 * LH) >= 1                # the round-robin branch is not empty
    moduli = _moduli("top", bits, n, L)
    c = dict(moduli=moduli, w=w, K=2, c0=rns_poly(81, moduli, n, batch), c1=rns_poly(82, moduli, n, batch), got={})
    c["terms"] = _terms(moduli, n, 2, [(_odd(n, bits + batch), "A"), (1, None)])
    c["want"] = _weighted_sum(oracle, n, moduli, w, c["c0"], c["c1"], c["terms"])
    assert len({c["want"][1][b].tobytes() for b in range(batch)}) == batch       # a swapped pair of batch elements would show
    _run_case(eng, c, n, "default", True, WIDTH[bits], arena=arena)


# ------------------------------------------------------------------------------------------------ 2. every fused instance
INSTANCES = [(bits, "top", n) for bits in BITS for n in (2048, 4096, 8192, 16384)] + [(bits, "span", 2048) for bits in BITS]


@pytest.mark.gpu
@pytest.mark.parametrize("bits,kind,n", INSTANCES)
def test_every_fused_instance_at_the_top_of_its_range(eng, oracle, bits, kind, n):
    """ntt_hoist_fwd_kernel and ntt_hoist_lincomb_kernel<F, LOGN> for all sixteen (F, LOGN): hoist_phys<LOGN>, the t0 = s0 >> (LOGN - 5) split,
    NttCfg<LOGN>::T and the 128 KiB image of the 8-byte fields at 2^14 depend on LOGN.  L = 2, K = 2, batch 2; a random element with key set A,
    the keyless term, 2n - 1 with key set B.  The default path only, and it must be the fused one."""
    L, batch, w = 2, 2, _half(bits)
    moduli = _moduli(kind, bits, n, L)
    c = _case(oracle, (bits, kind, n), n, moduli, w, batch, [(_odd(n, bits + n), "A"), (1, None), (2 * n - 1, "B")])
    assert c["K"] == 2
    _run_case(eng, c, n, "default", True, WIDTH[bits])


# ------------------------------------------------------------------------------------------------ 3. accumulation length
@pytest.mark.gpu
@pytest.mark.parametrize("L,w,fused", [(10, 6, True), (12, 7, False)])
def test_fp64_linear_transform_on_both_sides_of_its_product_limit(eng, oracle, L, w, fused):
    """hoist_lincomb.hip.h: F52 |acc| < L K * 0.76 q < 2^49, the host admits L K <= 83.  K = ceil(43 / w) only, so the nearest sides are
    10 * 8 = 80 (packed tables, the fused kernels) and 12 * 7 = 84, where the key set keeps its containers by itself and the transform takes the
    composed path with no switch set.  One keyed term with a random element and a random plaintext, one keyless term; batch 1."""
    n, batch = 2048, 1
    moduli = _moduli("top", 43, n, L)
    c = _case(oracle, ("fp64-limit", L, w), n, moduli, w, batch, [(_odd(n, L), "A"), (1, None)])
    assert L * c["K"] == (80 if fused else 84)
    _run_case(eng, c, n, "default", fused, WIDTH[43])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["default", "container-keys"])
@pytest.mark.parametrize("bits", BITS)
def test_linear_transform_with_many_digits_at_the_top_primes(eng, oracle, monkeypatch, bits, variant):
    """MANY_DIGITS of test_top_of_range.py: the longest accumulation chains that keep packed tables on every field (FP64: L K = 44)."""
    n, batch = 2048, 1
    w, L = MANY_DIGITS[bits]
    _set_variant(monkeypatch, variant)
    c = _case(oracle, ("many", bits), n, _moduli("top", bits, n, L), w, batch, [(_odd(n, bits), "A"), (1, None)])
    _run_case(eng, c, n, variant, variant == "default", WIDTH[bits])


# ------------------------------------------------------------------------------------------------ 4. the composed routes on container keys
def _route_spec(n, seed):
    """A random element with key set A, the keyless term, 2n - 1 with key set B."""
    return [(_odd(n, seed), "A"), (1, None), (2 * n - 1, "B")]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(SWITCH))
@pytest.mark.parametrize("bits", BITS)
def test_linear_transform_on_container_keys_by_switch(eng, oracle, monkeypatch, bits, variant):
    """FHE_HIP_NO_FUSED_KEYSWITCH=1 keeps every key set as containers: relin_mac_perm_kernel<F> under a linear transform, and the keyless
    term's out-of-place multiply_bcast beside it.  The fused kernels and the packed-table composition must return the same bits."""
    n, L, batch, w = 2048, 2, 2, _half(bits)
    _set_variant(monkeypatch, variant)
    c = _case(oracle, ("route", bits), n, _moduli("top", bits, n, L), w, batch, _route_spec(n, bits))
    assert c["K"] == 2
    _run_case(eng, c, n, variant, variant == "default", WIDTH[bits])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(SWITCH))
@pytest.mark.parametrize("field", ["F32", "F64", "F64X"])
def test_linear_transform_on_mixed_prime_sizes(eng, oracle, monkeypatch, field, variant):
    """test_hoisted_edges._mixed_bases: a digit of the wide limb exceeds the narrow limb's modulus, the key set keeps its containers by itself
    and the transform is composed with no switch set (default); the two switches change nothing about that."""
    n, batch = 2048, 2
    moduli, w, width = _mixed_bases(n)[field]
    _set_variant(monkeypatch, variant)
    c = _case(oracle, ("mixed", field), n, moduli, w, batch, _route_spec(n, width))
    _run_case(eng, c, n, variant, False, width)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(SWITCH))
def test_linear_transform_with_whole_word_digits_on_the_full_range_field(eng, oracle, monkeypatch, variant):
    """F64X, TOP primes, w = 64: keys_get_packed refuses (a whole-word digit of the larger prime's limb is no residue of the smaller prime),
    so the default path is the composed one on container keys."""
    n, L, batch, w = 2048, 2, 2, 64
    _set_variant(monkeypatch, variant)
    c = _case(oracle, ("w64",), n, _moduli("top", 64, n, L), w, batch, _route_spec(n, 64))
    assert c["K"] == 1
    _run_case(eng, c, n, variant, False, WIDTH[64])


# ------------------------------------------------------------------------------------------------ 5. term order
TERM_LISTS = {"keyless": [None], "keyed": ["A"], "keyless-keyed": [None, "A"], "keyed-keyless": ["A", None], "keyless-keyless": [None, None]}


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["default", "packed-tables"])
@pytest.mark.parametrize("order", list(TERM_LISTS))
@pytest.mark.parametrize("bits", [30, 62])
def test_term_order_and_keyless_only_transforms(eng, oracle, monkeypatch, bits, order, variant):
    """The composed path sends its first term straight to the outputs and later ones through d_lin, a keyless one as an out-of-place
    multiply_bcast from c0 / c1; the fused kernel skips its L K loop for a keyless term and still needs the hoist.  c1 is passed where a
    keyless term exists and NULL otherwise.  The two keyless terms carry different plaintexts (_terms seeds them by position)."""
    n, L, batch, w = 2048, 2, 2, _half(bits)
    _set_variant(monkeypatch, variant)
    spec = [(_odd(n, bits) if name else 1, name) for name in TERM_LISTS[order]]
    c = _case(oracle, ("order", bits, order), n, _moduli("top", bits, n, L), w, batch, spec)
    if order == "keyless-keyless":
        assert not np.array_equal(c["terms"][0][2], c["terms"][1][2])
    _run_case(eng, c, n, variant, variant == "default", WIDTH[bits])


# ------------------------------------------------------------------------------------------------ 6. evaluation-domain constants
@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["default", "packed-tables"])
@pytest.mark.parametrize("bits,w", [(30, 10), (43, 15), (62, 21), (64, 22)])
def test_operands_that_are_constants_in_the_evaluation_domain(eng, oracle, monkeypatch, bits, w, variant):
    """The patterns of test_top_of_range.py are extremes of the coefficient domain and look random after the forward transform.  The constant
    polynomial q - 1 is q - 1 in every evaluation slot: with c0, c1, every key row and every plaintext such a constant, every lane of
    ntt_hoist_lincomb_kernel multiplies and adds the largest canonical operands at once (the digits of q - 1 are constants too).  K = 3, four
    keyed terms with random elements and one keyless; batch element 0 has the closed form, element 1 is random and comes from the oracle."""
    n, L, batch = 2048, 2, 2
    _set_variant(monkeypatch, variant)
    moduli = _moduli("top", bits, n, L)

    def make():
        K = oracle.RnsPlan(n, moduli).num_digits(w)
        terms = _constant_terms(moduli, n, K, [_odd(n, bits), _odd(n, bits + 1), None, _odd(n, bits + 2), _odd(n, bits + 3)])
        c0, c1 = rns_poly(81, moduli, n, batch), rns_poly(82, moduli, n, batch)
        c0[0] = c1[0] = _constant(moduli, n)
        return dict(moduli=moduli, w=w, K=K, terms=terms, c0=c0, c1=c1, want=_weighted_sum(oracle, n, moduli, w, c0, c1, terms), got={})
    c = _cached(("lincomb", "constants", bits), make)
    assert c["K"] == 3
    closed = _constant_closed_form(moduli, n, w, 3, keyed=4, keyless=1)
    assert np.array_equal(c["want"][0][0], closed[0]) and np.array_equal(c["want"][1][0], closed[1])
    _run_case(eng, c, n, variant, variant == "default", WIDTH[bits])
    got = c["got"][variant]
    assert np.array_equal(got[0][0], closed[0]) and np.array_equal(got[1][0], closed[1])


# ------------------------------------------------------------------------------------------------ 7. state
@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["default", "packed-tables"])
def test_linear_transform_after_a_smaller_hoist_follows_a_larger_one(eng, oracle, monkeypatch, variant):
    """test_hoisted_edges.test_a_smaller_hoist_after_a_larger_one for the transform: hoist at batch 5, hoist another c1 at batch 2 (the workspace
    keeps its size: its tail still holds the first decomposition), transform at batch 2 inside guard bands; batch 5 is rejected from then on
    with nothing written."""
    n, L, w, big, batch = 2048, 2, 16, 5, 2
    _set_variant(monkeypatch, variant)
    fused = variant == "default"
    moduli = _moduli("top", 30, n, L)
    e = eng.RnsNttEngine(n, moduli)
    K = e.relin_num_digits(w)
    terms = _terms(moduli, n, K, [(eng.galois_element(n, 5), "A"), (1, None)])
    lt, _sets = _build(eng, e, w, terms)
    first = _mixed(91, moduli, n, [None, "top", "alt0", "alt1", None])
    c0, c1 = _mixed(81, moduli, n, ["top", None]), _mixed(82, moduli, n, [None, "top"])
    e.hoist(w, _up(eng, first), big)
    held = e.hoist_bytes()
    assert held == _hoist_bytes(eng, e, L, K, n, big, fused), NOT_RUN
    got = _transform(eng, e, lt, w, c0, c1, True, arena=True)
    assert e.hoist_bytes() == held
    want = _weighted_sum(oracle, n, moduli, w, c0, c1, terms)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not np.array_equal(want[1], _weighted_sum(oracle, n, moduli, w, c0, first[:batch], terms)[1])     # the first decomposition would show
    d0, d1, o0, o1 = _up(eng, first), _up(eng, first), eng.DeviceBuffer(first.nbytes), eng.DeviceBuffer(first.nbytes)
    memcheck.poison(eng, o0); memcheck.poison(eng, o1)
    with pytest.raises(eng.FheError) as ex:
        e.linear_transform_hoisted(lt, o0, o1, d0, d1, big)
    assert ex.value.code == -1, str(ex.value)
    assert memcheck.is_poison(o0.download(first.shape)) and memcheck.is_poison(o1.download(first.shape))
    assert e.hoist_bytes() == held


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["default", "packed-tables"])
def test_two_transforms_alternate_while_the_scratch_grows(eng, oracle, monkeypatch, variant):
    """One engine, one hoist; A has no keyless term, B has one: A, B, A, B.  On the fused path d_lin grows from one residue image (c0^) to two
    (c0^, c1^) at the first B, which frees and reallocates it; the kept decomposition lives in the hoist workspace and must not notice."""
    n, L, batch, bits = 2048, 2, 2, 30
    w = _half(bits)
    _set_variant(monkeypatch, variant)
    fused = variant == "default"
    moduli = _moduli("top", bits, n, L)
    e = eng.RnsNttEngine(n, moduli)
    K = e.relin_num_digits(w)
    both = _terms(moduli, n, K, [(_odd(n, 1), "A"), (2 * n - 1, "B"), (1, None)])
    tA, tB = both[:2], both[1:]
    ltA, _setsA = _build(eng, e, w, tA)
    ltB, _setsB = _build(eng, e, w, tB)
    c0, c1 = _operands(moduli, n, batch)
    want = {"A": _weighted_sum(oracle, n, moduli, w, c0, c1, tA), "B": _weighted_sum(oracle, n, moduli, w, c0, c1, tB)}
    assert not np.array_equal(want["A"][0], want["B"][0])
    e.hoist(w, _up(eng, c1), batch)
    held = e.hoist_bytes()
    assert held == _hoist_bytes(eng, e, L, K, n, batch, fused), NOT_RUN
    for step, name in enumerate("ABAB"):
        got = _transform(eng, e, ltA if name == "A" else ltB, w, c0, c1, name == "B", hoist=False)
        assert np.array_equal(got[0], want[name][0]) and np.array_equal(got[1], want[name][1]), (step, name)
        assert e.hoist_bytes() == held, (step, name)
        if fused:
            assert e.workspace_bytes() == _fused_sizes(eng, e, L, n, batch, keyless=step > 0), (step, name, NOT_RUN)
