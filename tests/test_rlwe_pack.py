"""fhe_rlwe_pack: coefficient 0 of batch * count RLWE pairs packed into one ciphertext per batch element without the samples in between, bit for
bit against fhe_rlwe_sample_extract(idx = 0) + fhe_lwe_pack through capi, on the fused path here and under FHE_HIP_NO_FUSED_PACK=1 in a fresh
child process.  Only c0[.][0] and c1 are read: a second input that differs in every other coefficient of c0 gives the same bits."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import memcheck
from test_lwe_pack import KEY_SEEDS, SIGMA, _context, _primes
from workload import rns_poly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -5
L = 2
# (n, bits, count, trace, normalize, batch): n = 64 with count = 64 runs every merge level and no trace step; count = 1 the plain (embedding) form
# of the first kernel, count >= 2 the pairing form
CASES = ([(64, 30, 64, 0, 1, 2), (64, 30, 64, 0, 0, 1)]
         + [(2048, 30, c, tr, nz, b) for c in (1, 2, 8) for tr in (0, 1) for nz in (0, 1) for b in (1, 3)]
         + [(2048, 40, 8, 1, 1, 3), (2048, 40, 2, 0, 0, 1), (2048, 40, 1, 1, 1, 3), (2048, 40, 1, 0, 0, 1)])
_fused = {}


def _pairs(case, other_c0=False, moduli=None):
    """[batch count][L][n][4] pairs with 0 and q - 1 among the values read; other_c0: the same c0[.][0] and c1, every other coefficient of c0 changed;
    moduli: another basis than the two primes the case's bits name"""
    n, bits, count, trace, normalize, batch = case
    moduli, entries = (list(moduli) if moduli is not None else _primes(bits, n, L)), batch * count
    c0, c1 = rns_poly(300 + count + 7 * batch, moduli, n, entries), rns_poly(301 + count + 7 * batch, moduli, n, entries)
    c1[:, :, 0, 0] = 0; c1[0, :, n // 2, 0] = 0; c0[0, :, 0, 0] = 0
    for l, q in enumerate(moduli):
        c1[:, l, 1, 0] = q - 1; c1[:, l, n - 1, 0] = q - 1; c0[entries - 1, l, 0, 0] = q - 1
    if other_c0:
        keep = c0[:, :, 0].copy()
        c0 = rns_poly(999, moduli, n, entries)
        c0[:, :, 0] = keep
    return c0, c1


def _rlwe_pack(pkg, case, reserve=False, other_c0=False):
    """the one call inside a guarded arena, outputs poisoned first: (out0, out1) as [batch][L][n][4]"""
    n, bits, count, trace, normalize, batch = case
    C = _context(pkg, n, bits)
    eng, S = C["eng"], L * n * 32
    c0, c1 = _pairs(case, other_c0)
    ar = memcheck.GuardedArena(pkg, [("c0", c0.nbytes), ("o0", batch * S), ("c1", c1.nbytes), ("o1", batch * S)], S)
    ar["c0"].upload(c0); ar["c1"].upload(c1); ar["o0"].poison(); ar["o1"].poison()
    if reserve:
        eng.lwe_pack_reserve(C["keys"], count, trace, batch)
    eng.rlwe_pack(C["keys"], ar["o0"], ar["o1"], ar["c0"], ar["c1"], count, trace, normalize, batch)
    ar.verify(inputs=("c0", "c1"))
    out = ar["o0"].download((batch, L, n, 4)), ar["o1"].download((batch, L, n, 4))
    ar.free()
    return out


def _fused_result(pkg, case):
    if case not in _fused:
        _fused[case] = _rlwe_pack(pkg, case)
    return _fused[case]


def _reference(pkg, case):
    """the definition: fhe_rlwe_sample_extract(idx = 0) of every pair, then fhe_lwe_pack of the samples"""
    n, bits, count, trace, normalize, batch = case
    C = _context(pkg, n, bits)
    eng, S = C["eng"], L * n * 32
    c0, c1 = _pairs(case)
    d_lwe = pkg.DeviceBuffer(batch * count * L * (n + 1) * 8)
    eng.sample_extract(d_lwe, pkg.DeviceBuffer.from_numpy(c0), pkg.DeviceBuffer.from_numpy(c1), 0, batch * count)
    o0, o1 = pkg.DeviceBuffer(batch * S), pkg.DeviceBuffer(batch * S)
    eng.lwe_pack(C["keys"], o0, o1, d_lwe, count, trace, normalize, batch)
    return o0.download((batch, L, n, 4)), o1.download((batch, L, n, 4))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_b%d_c%d_t%d_z%d_x%d" % c)
def test_the_call_equals_extraction_at_zero_and_the_packing_of_the_samples(pkg, case):
    got, want = _fused_result(pkg, case), _reference(pkg, case)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not memcheck.is_poison(got[0][..., 0]) and (got[0][..., 1:] == 0).all() and (got[1][..., 1:] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(64, 30, 64, 0, 1, 2), (2048, 30, 1, 1, 1, 3), (2048, 30, 8, 1, 1, 3), (2048, 40, 2, 0, 0, 1)], ids=lambda c: "n%d_b%d_c%d_t%d_z%d_x%d" % c)
def test_c0_away_from_coefficient_0_does_not_influence_the_result(pkg, case):
    a, b = _pairs(case), _pairs(case, other_c0=True)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0][:, :, 0], b[0][:, :, 0]) and not np.array_equal(a[0][:, :, 1:], b[0][:, :, 1:])
    got, want = _rlwe_pack(pkg, case, other_c0=True), _fused_result(pkg, case)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


CHILD = """import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import importlib
import numpy as np
pkg = importlib.import_module("gpu-homomorphic-encryption_amd")
import test_rlwe_pack as T
from test_lwe_pack import _context
out = {{}}
for i, case in enumerate(T.CASES):
    n, bits, count, trace, normalize, batch = case
    eng = _context(pkg, n, bits)["eng"]
    eng.lwe_pack_reserve(_context(pkg, n, bits)["keys"], count, trace, batch)
    reserved = eng.workspace_bytes()
    # the composed path's container scratch (count >= 2) and the samples this entry extracts first
    assert reserved >= (5 * 2 * n * 32 if count >= 2 else 0) * batch * count + batch * count * 2 * (n + 1) * 8, case
    out["a%d" % i], out["b%d" % i] = T._rlwe_pack(pkg, case)
    assert eng.workspace_bytes() == reserved, case
np.savez(sys.argv[1], **out)
"""


@pytest.mark.gpu
def test_the_composed_path_in_a_child_process_gives_the_same_bits(pkg, tmp_path):
    """FHE_HIP_NO_FUSED_PACK=1 for every case, in a fresh process so that the switch stays out of this one; there the reserve also covers the
    sample scratch, so the workspace does not change across the call either."""
    (tmp_path / "child.py").write_text(CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests")))
    env = dict(os.environ, FHE_HIP_NO_FUSED_PACK="1")
    res = subprocess.run([sys.executable, str(tmp_path / "child.py"), str(tmp_path / "out.npz")], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    got = np.load(tmp_path / "out.npz")
    for i, case in enumerate(CASES):
        want = _fused_result(pkg, case)
        assert np.array_equal(got["a%d" % i], want[0]) and np.array_equal(got["b%d" % i], want[1]), case


@pytest.mark.gpu
@pytest.mark.parametrize("count,trace", [(8, True), (1, True), (2, False)])
def test_after_the_reserve_of_lwe_pack_a_call_leaves_the_workspace_alone(pkg, count, trace):
    from test_encrypt import _embed
    n, batch = 2048, 3
    C = _context(pkg, n, 30)
    eng = pkg.RnsNttEngine(n, C["moduli"])                               # a fresh engine: nothing has grown yet
    ds = pkg.DeviceBuffer.from_numpy(_embed(C["s"][None], C["moduli"])[0])
    sk = eng.import_secret_key(ds)
    keys = eng.generate_keyswitch_keys(sk, 16, pkg.capi.lwe_pack_galois_elements(n), 1, SIGMA, KEY_SEEDS)
    eng.lwe_pack_reserve(keys, count, trace, batch)
    reserved = eng.workspace_bytes()
    case = (n, 30, count, int(trace), 1, batch)
    c0, c1 = _pairs(case)
    S = L * n * 32
    o0, o1 = pkg.DeviceBuffer(batch * S), pkg.DeviceBuffer(batch * S)
    eng.rlwe_pack(keys, o0, o1, pkg.DeviceBuffer.from_numpy(c0), pkg.DeviceBuffer.from_numpy(c1), count, trace, True, batch)
    assert eng.workspace_bytes() == reserved
    want = _fused_result(pkg, case)                                      # same keys (seeds) and pairs as the shared context: same bits
    assert np.array_equal(o0.download((batch, L, n, 4)), want[0]) and np.array_equal(o1.download((batch, L, n, 4)), want[1])


@pytest.mark.gpu
def test_rejections_leave_guarded_poisoned_outputs_untouched(pkg):
    n, bits, count, batch = 2048, 30, 4, 2
    case = (n, bits, count, 1, 1, batch)
    C = _context(pkg, n, bits)
    eng, keys, lib = C["eng"], C["keys"], pkg.lib()
    other = _context(pkg, 2048, 40)
    S = L * n * 32
    c0, c1 = _pairs(case)
    arena = memcheck.GuardedArena(pkg, [("o0", batch * S), ("o1", batch * S), ("c0", c0.nbytes), ("c1", c1.nbytes)], S)
    arena["c0"].upload(c0); arena["c1"].upload(c1); arena["o0"].poison(); arena["o1"].poison()
    h, o0, o1, a0, a1 = eng.h, arena["o0"].ptr, arena["o1"].ptr, arena["c0"].ptr, arena["c1"].ptr
    ka = lambda ks: (ctypes.c_void_p * len(ks))(*[None if k is None else k.h for k in ks])
    good = ka(keys)
    w8 = eng.generate_keyswitch_keys(C["keep"][1], 8, [5], 1, SIGMA, KEY_SEEDS)[0]
    bad = {
        "null handle": (None, good, o0, o1, a0, a1, count, 1, 1, batch),
        "null output": (h, good, None, o1, a0, a1, count, 1, 1, batch),
        "null output 1": (h, good, o0, None, a0, a1, count, 1, 1, batch),
        "null c0": (h, good, o0, o1, None, a1, count, 1, 1, batch),
        "null c1": (h, good, o0, o1, a0, None, count, 1, 1, batch),
        "null key array": (h, None, o0, o1, a0, a1, count, 1, 1, batch),
        "null merge key": (h, ka([keys[0], None] + keys[2:]), o0, o1, a0, a1, count, 0, 1, batch),
        "null trace key": (h, ka(keys[:-1] + [None]), o0, o1, a0, a1, count, 1, 1, batch),
        "keys of another engine": (h, ka(other["keys"]), o0, o1, a0, a1, count, 1, 1, batch),
        "differing decomp_bits": (h, ka([keys[0], w8] + keys[2:]), o0, o1, a0, a1, count, 1, 1, batch),
        "count 0": (h, good, o0, o1, a0, a1, 0, 1, 1, batch),
        "count 3": (h, good, o0, o1, a0, a1, 3, 1, 1, batch),
        "count above n": (h, good, o0, o1, a0, a1, 2 * n, 1, 1, batch),
        "batch 0": (h, good, o0, o1, a0, a1, count, 1, 1, 0),
        "batch count overflow": (h, good, o0, o1, a0, a1, 1024, 1, 1, 1 << 22),
        "misaligned output": (h, good, o0 + 8, o1, a0, a1, count, 1, 1, batch),
        "misaligned c0": (h, good, o0, o1, a0 + 8, a1, count, 1, 1, batch),
        "misaligned c1": (h, good, o0, o1, a0, a1 + 8, count, 1, 1, batch),
        "outputs overlap": (h, good, o0, o0 + S, a0, a1, count, 1, 1, batch),
        "output 0 overlaps c0": (h, good, a0 + 32, o1, a0, a1, count, 1, 1, batch),
        "output 1 overlaps c1": (h, good, o0, a1 + (batch * count - 1) * S, a0, a1, count, 1, 1, batch),
        "output 0 is the end of c1": (h, good, a1 + (batch * count - batch) * S, o1, a0, a1, count, 1, 1, batch),
    }
    for name, args in bad.items():
        assert lib.fhe_rlwe_pack(*args) == INVALID, name
    arena.verify(inputs=("c0", "c1"))
    assert memcheck.is_poison(arena["o0"].download((-1,))) and memcheck.is_poison(arena["o1"].download((-1,)))
    # unused key sets may be null: count = 4 without the trace uses keys[0] and keys[1] only
    assert lib.fhe_rlwe_pack(h, ka(keys[:2] + [None] * (len(keys) - 2)), o0, o1, a0, a1, count, 0, 1, batch) == 0
    arena.verify(inputs=("c0", "c1"))
    got = arena["o0"].download((batch, L, n, 4)), arena["o1"].download((batch, L, n, 4))
    want = _reference(pkg, (n, bits, count, 0, 1, batch))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.gpu
def test_a_full_width_engine_is_unsupported(pkg):
    import ntt_math as nm
    n = 2048
    eng = pkg.RnsNttEngine(n, nm.ntt_primes(120, n, 2))
    S = 2 * n * 32
    o0, o1, a0, a1 = (pkg.DeviceBuffer(S) for _ in range(4))
    memcheck.poison(pkg, o0)
    keys = (ctypes.c_void_p * 11)()
    assert pkg.lib().fhe_rlwe_pack(eng.h, keys, o0.ptr, o1.ptr, a0.ptr, a1.ptr, 1, 0, 0, 1) == UNSUPPORTED
    assert memcheck.is_poison(o0.download((-1,)))
