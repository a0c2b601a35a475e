"""fhe_ct_mod_switch_drop_last (BGV modulus switch) against the per-limb formula in Python integers, bit-exact on whole containers.

    r = in[b][L-1][x];  u = (-r t^-1) mod q_last;  u_c = u if u <= (q_last - 1) / 2 else u - q_last
    out[b][l][x] = (in[b][l][x] + t u_c) q_last^-1 mod q_l,   l < L - 1

Rows: the smallest shapes that reach each kernel (the word-sized classes exist from n = 2^11; smaller rings, wider primes and mixed
bases take the container kernel, and so does a word-sized engine under FHE_HIP_NO_WORD_CONVERSIONS=1).  Every input is random canonical
residues with planted coefficients at x = 0 .. 9 of every batch element: the last-limb residue chosen so that u is 0, 1, (q_last - 1) / 2,
(q_last + 1) / 2 and q_last - 1 (both sides of the centring boundary and the range ends), crossed with the other limbs all 0 / all q_l - 1."""
import ctypes

import numpy as np
import pytest

import ntt_math as nm
from memcheck import GuardedArena, is_poison, poison
from workload import rns_poly

M64 = (1 << 64) - 1
BATCH = 3
T_BIG = (1 << 64) - 59
T_ABOVE_30 = (1 << 39) + 7            # between the 30-bit primes and 2^40: the host has to reduce t modulo every limb


def _basis(name):
    n = ROWS[name][0]
    if name == "n2048-2x64top":
        return nm.largest_ntt_primes(64, n, 2)                          # as tests/test_top_of_range.py picks them
    if name == "n64-mixed-wide-last":
        return nm.ntt_primes(60, n, 1) + nm.ntt_primes(30, n, 1) + nm.ntt_primes(250, n, 1)
    if name == "n64-mixed-narrow-last":
        return nm.ntt_primes(250, n, 1) + nm.ntt_primes(60, n, 1) + nm.ntt_primes(30, n, 1)
    bits, L = ROWS[name][2], ROWS[name][3]
    return nm.ntt_primes(bits, n, L)


# name -> (n, width class of the engine, bits, L)
ROWS = {
    "n256-3x30": (256, 4, 30, 3),               # container kernel, by ring size
    "n2048-2x30": (2048, 1, 30, 2),             # F32, the smallest basis
    "n2048-4x30": (2048, 1, 30, 4),
    "n2048-3x40": (2048, 3, 40, 3),             # F52
    "n2048-3x60": (2048, 2, 60, 3),             # F64
    "n2048-2x64top": (2048, 5, 64, 2),          # F64X
    "n64-2x250": (64, 4, 250, 2),               # full width, Q > 2^255: no CRT
    "n64-mixed-wide-last": (64, 4, None, 3),    # last prime wider than the rest
    "n64-mixed-narrow-last": (64, 4, None, 3),  # last prime narrower than the rest
}
CASES = [(name, True) for name in ROWS] + [(name, False) for name, row in ROWS.items() if row[1] != 4]
CASE_IDS = [f"{name}-{'default' if word else 'no-word-conversions'}" for name, word in CASES]
_MODULI, _INPUTS, _REF = {}, {}, {}


def _moduli(name):
    if name not in _MODULI:
        _MODULI[name] = _basis(name)
    return _MODULI[name]


def _t_values(name):
    ts = [2, 65537, T_BIG]
    if ROWS[name][2] == 30:
        ts.append(T_ABOVE_30)
    return ts


def _to_ints(a):
    """[..., 4] uint64 containers -> object array of Python integers"""
    return sum(a[..., k].astype(object) << (64 * k) for k in range(4))


def _to_limbs(v):
    out = np.zeros(v.shape + (4,), np.uint64)
    for k in range(4):
        out[..., k] = ((v >> (64 * k)) & M64).astype(np.uint64)
    return out


def _inputs(name, t):
    """Three components [BATCH][L][n][4] for (row, t), built once."""
    key = (name, t)
    if key not in _INPUTS:
        moduli, n = _moduli(name), ROWS[name][0]
        ql = moduli[-1]
        us = [0, 1, (ql - 1) // 2, (ql + 1) // 2, ql - 1]
        comps = []
        for c in range(3):
            X = _to_ints(rns_poly(700 + c, moduli, n, BATCH))
            for b in range(BATCH):
                for i, u in enumerate(us):
                    for j, top in enumerate((False, True)):
                        x = 2 * i + j
                        X[b, -1, x] = (-t * u) % ql
                        for l, q in enumerate(moduli[:-1]):
                            X[b, l, x] = q - 1 if top else 0
            comps.append(_to_limbs(X))
        _INPUTS[key] = comps
    return _INPUTS[key]


def _formula(X, moduli, t):
    """The issue's per-limb definition on Python integers: X is [batch][L][n][4] containers, the result [batch][L-1][n][4]."""
    V = _to_ints(X)
    ql = moduli[-1]
    u = (-V[:, -1, :] * pow(t, -1, ql)) % ql
    uc = np.where((u <= (ql - 1) // 2).astype(bool), u, u - ql)
    out = np.empty((V.shape[0], len(moduli) - 1, V.shape[2]), object)
    for l, q in enumerate(moduli[:-1]):
        out[:, l, :] = ((V[:, l, :] + t * uc) * pow(ql, -1, q)) % q
    return _to_limbs(out)


def _reference(name, t):
    key = (name, t)
    if key not in _REF:
        _REF[key] = [_formula(X, _moduli(name), t) for X in _inputs(name, t)]
    return _REF[key]


def test_formula_keeps_the_plaintext_up_to_the_known_factor():
    """The oracle itself, on the CPU: the limb-wise formula is the exact integer division C' = (C + t u_c) / q_last with |t u_c| <= t q_last / 2,
    so q_last C' = C (mod t), whereas the plain rounded division (C - [C]_q_last) / q_last is not."""
    moduli, t = nm.ntt_primes(30, 16, 4), 65537
    ql = moduli[-1]
    Q = 1
    for q in moduli:
        Q *= q
    rng = np.random.default_rng(5)
    C = [int.from_bytes(rng.bytes(16), "little") % Q for _ in range(16)]
    X = _to_limbs(np.array([[[c % q for c in C] for q in moduli]], object))
    out = _to_ints(_formula(X, moduli, t))[0]
    plain_kept = 0
    for i, c in enumerate(C):
        u = (-c * pow(t, -1, ql)) % ql
        uc = u if u <= (ql - 1) // 2 else u - ql
        assert (c + t * uc) % ql == 0 and abs(t * uc) <= t * ql // 2
        cp = (c + t * uc) // ql
        assert [cp % q for q in moduli[:-1]] == [int(out[l, i]) for l in range(len(moduli) - 1)]
        assert (cp * ql - c) % t == 0
        r = c % ql
        plain_kept += (((c - (r if r <= ql // 2 else r - ql)) // ql) * ql - c) % t == 0
    assert plain_kept < len(C)


def test_null_handle_is_rejected_without_a_device(pkg):
    lib = pkg.lib()
    assert lib.fhe_ct_mod_switch_drop_last(None, 65537, None, None, 2, 1) == -1
    assert b"null handle" in lib.fhe_hip_last_error()


# ------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def eng(pkg):
    if pkg.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")
    return pkg


def _engine(eng, monkeypatch, name, word):
    if not word:
        monkeypatch.setenv("FHE_HIP_NO_WORD_CONVERSIONS", "1")
    e = eng.RnsNttEngine(ROWS[name][0], _moduli(name))
    assert e.width_class == ROWS[name][1]
    return e


def _out_bytes(name, batch=BATCH):
    return batch * (ROWS[name][3] - 1) * ROWS[name][0] * 32


def _switch(eng, e, name, t, ins, batch=BATCH):
    """One call on fresh poisoned outputs; returns the outputs as [batch][L-1][n][4] arrays."""
    n, L = ROWS[name][0], ROWS[name][3]
    d_in = [eng.DeviceBuffer.from_numpy(np.ascontiguousarray(x)) for x in ins]
    d_out = [eng.DeviceBuffer(_out_bytes(name, batch)) for _ in ins]
    for d in d_out:
        poison(eng, d)
    e.ct_mod_switch(t, d_out, d_in, batch)
    eng.capi.sync()
    return [d.download((batch, L - 1, n, 4)) for d in d_out]


@pytest.mark.gpu
@pytest.mark.parametrize("name,word", CASES, ids=CASE_IDS)
def test_parity_with_the_integer_formula(eng, monkeypatch, name, word):
    """Batch 3, every t of the row, 3 / 2 / 1 components per call: each output equals the formula, hence the calls agree with one another."""
    e = _engine(eng, monkeypatch, name, word)
    for t in _t_values(name):
        assert t % _moduli(name)[-1] != 0
        ins, want = _inputs(name, t), _reference(name, t)
        for k in (3, 2, 1):
            got = _switch(eng, e, name, t, ins[:k])
            for c in range(k):
                bad = int((got[c] != want[c]).any(axis=-1).sum())
                assert bad == 0, f"t = {t}, {k} components, component {c}: {bad} of {want[c].size // 4} containers differ from the formula"


@pytest.mark.gpu
@pytest.mark.parametrize("name,word", CASES, ids=CASE_IDS)
def test_batch_elements_are_independent(eng, monkeypatch, name, word):
    e = _engine(eng, monkeypatch, name, word)
    t = 65537
    ins, want = _inputs(name, t), _reference(name, t)
    for b in range(BATCH):
        got = _switch(eng, e, name, t, [x[b:b + 1] for x in ins[:2]], batch=1)
        for c in range(2):
            assert np.array_equal(got[c][0], want[c][b]), f"batch element {b} alone, component {c}"


@pytest.mark.gpu
@pytest.mark.parametrize("name,word", CASES, ids=CASE_IDS)
def test_memory_contract_at_batch_3(eng, monkeypatch, name, word):
    """Inputs and poisoned outputs carved out of one allocation with guard bands between them: the guards stay intact, the inputs are
    unchanged and every output byte is written (the outputs equal the formula, and no container is left as poison)."""
    e = _engine(eng, monkeypatch, name, word)
    t = T_BIG
    ins, want = _inputs(name, t), _reference(name, t)
    n, L = ROWS[name][0], ROWS[name][3]
    specs = [(f"in{c}", ins[c].nbytes) for c in range(3)] + [(f"out{c}", _out_bytes(name)) for c in range(3)]
    ar = GuardedArena(eng, specs, L * n * 32)
    try:
        for c in range(3):
            ar[f"in{c}"].upload(ins[c])
            ar[f"out{c}"].poison()
        e.ct_mod_switch(t, [ar[f"out{c}"] for c in range(3)], [ar[f"in{c}"] for c in range(3)], BATCH)
        ar.verify(inputs=[f"in{c}" for c in range(3)])
        for c in range(3):
            got = ar[f"out{c}"].download(want[c].shape)
            assert np.array_equal(got, want[c]), f"out{c} differs from the formula"
            assert not (got.reshape(-1, 4) == np.uint64(0x5A5A5A5A5A5A5A5A)).all(axis=-1).any(), f"out{c}: a container was left unwritten"
    finally:
        ar.free()


@pytest.mark.gpu
def test_rejections_launch_nothing(eng):
    n, t = 2048, 65537
    moduli = nm.ntt_primes(30, n, 2)
    ql = moduli[-1]
    e, e1 = eng.RnsNttEngine(n, moduli), eng.RnsNttEngine(n, moduli[:1])
    X = [np.ascontiguousarray(rns_poly(40 + c, moduli, n, 1)) for c in range(4)]
    d_in = [eng.DeviceBuffer.from_numpy(x) for x in X]
    d_out = [eng.DeviceBuffer(n * 32 + 64) for _ in range(4)]
    for d in d_out:
        poison(eng, d)
    i, o = [d.ptr for d in d_in], [d.ptr for d in d_out]
    lib = eng.lib()
    arr = lambda ps: (ctypes.c_void_p * len(ps))(*ps)
    calls = {
        "L = 1": lambda: e1.ct_mod_switch(t, o[:2], i[:2]),
        "t = 0": lambda: e.ct_mod_switch(0, o[:2], i[:2]),
        "t = 1": lambda: e.ct_mod_switch(1, o[:2], i[:2]),
        "t = q_last": lambda: e.ct_mod_switch(ql, o[:2], i[:2]),
        "t = 3 q_last": lambda: e.ct_mod_switch(3 * ql, o[:2], i[:2]),
        "0 components": lambda: e.ct_mod_switch(t, [], []),
        "4 components": lambda: e.ct_mod_switch(t, o, i),
        "null output": lambda: e.ct_mod_switch(t, [o[0], None], i[:2]),
        "null input": lambda: e.ct_mod_switch(t, o[:2], [None, i[1]]),
        "null output array": lambda: eng.capi._check(lib.fhe_ct_mod_switch_drop_last(e.h, t, None, arr(i[:2]), 2, 1)),
        "null input array": lambda: eng.capi._check(lib.fhe_ct_mod_switch_drop_last(e.h, t, arr(o[:2]), None, 2, 1)),
        "output offset by 8 bytes": lambda: e.ct_mod_switch(t, [o[0], o[1] + 8], i[:2]),
        "input offset by 8 bytes": lambda: e.ct_mod_switch(t, o[:2], [i[0] + 8, i[1]]),
        "output aliases an input": lambda: e.ct_mod_switch(t, [o[0], i[0]], i[:2]),
        "output aliases its own input": lambda: e.ct_mod_switch(t, [i[0]], [i[0]]),
        "two equal outputs": lambda: e.ct_mod_switch(t, [o[0], o[0]], i[:2]),
    }
    for what, call in calls.items():
        with pytest.raises(eng.FheError) as ei:
            call()
        assert ei.value.code == -1, what
    eng.capi.sync()
    for d in d_out:
        assert is_poison(d.download((-1,), np.uint8)), "a rejected call wrote to an output"
    for d, x in zip(d_in, X):
        assert np.array_equal(d.download(x.shape), x), "a rejected call wrote to an input"
