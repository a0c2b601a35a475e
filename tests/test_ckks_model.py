"""CPU tests of the CKKS encoder: the long-double model (ckks_model.py) against direct evaluation, the host-side slot table, the seven names of
the header block in header, library and binding, and the compiled kernels' resources (tests/golden/ckks_encoder_resources.txt)."""
import concurrent.futures
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from ckks_model import CKKS_NAMES, CKKS_SYMBOLS, CLD, LD, ROOT, decode, encode, family_slots, impulse_plaintext, impulse_slots, slot_table, spot_check
from test_hoisted import CSRC, HIPCC, RES_FLAGS, _resource_remarks


def test_long_double_is_wider_than_double():
    assert np.finfo(LD).eps < 2.0 ** -60, "the model needs an extended long double"


def test_model_matches_direct_evaluation_and_inverts():
    for n in (16, 2048):
        rng = np.random.default_rng(n)
        z = rng.random(n // 2) + 1j * rng.random(n // 2)
        m = encode(z, n)
        assert m.dtype == LD
        spot_check(m, z.astype(CLD), n, 1e-15)                          # polynomial-evaluation rounding at |m| sum ~ 1
        back = decode(m)
        assert float(np.max(np.abs(back - z.astype(CLD)))) < 1e-16
        # sigma_3 rotates left by one, sigma_(2n-1) conjugates
        def sigma(g):
            out = np.zeros(n, dtype=LD)
            for j in range(n):
                k = j * g % (2 * n)
                out[k % n] = -m[j] if k >= n else m[j]
            return out
        assert float(np.max(np.abs(decode(sigma(3)) - np.roll(z, -1).astype(CLD)))) < 1e-15
        assert float(np.max(np.abs(decode(sigma(2 * n - 1)) - np.conj(z).astype(CLD)))) < 1e-15


def test_integer_polynomials_are_recovered_exactly_by_the_model():
    """The exact cases of the GPU test: coefficients in [-2^20, 2^20]; slots rounded to double; the float64 formula's transform error is far
    below 1/2, so rounding recovers m0 and the reference alone is exact."""
    n = 2048
    rng = np.random.default_rng(5)
    m0 = rng.integers(-(1 << 20), (1 << 20) + 1, n)
    z = decode(m0.astype(LD)).astype(np.complex128)
    for cdtype in (CLD, np.complex128):
        m = encode(z, n, cdtype)
        assert float(np.max(np.abs(m.astype(LD) - m0.astype(LD)))) < 2.0 ** -10
        assert np.array_equal(np.rint(m.astype(np.float64)).astype(np.int64), m0)


FAMILY_XY = ((0.5, -1.5), (-0.0, 0.0), (2.0 ** 53 - 1, 1.0), (2.0 ** 62 - 512, -2.0 ** 61), (2.0 ** 63, -2.0 ** 63), (1e300, -5e-324))


@pytest.mark.parametrize("n", [2048, 4096, 8192, 16384])
def test_the_exact_family_passes_through_the_model_without_one_rounding(n):
    """Premise of test_ckks_edges.py: z_k = x + i y (x - i y where c(k)) encodes to m = x + y X^(n/2) and back with np.array_equal, in long
    double and in float64 alike, so what the device is compared with has no error of its own."""
    for x, y in FAMILY_XY:
        z = family_slots(n, x, y)
        want = np.zeros(n)
        want[0], want[n // 2] = x, y
        for cdtype in (CLD, np.complex128):
            m = encode(z, n, cdtype)
            assert np.array_equal(m, want.astype(m.dtype)), (n, x, y, cdtype)
            assert np.array_equal(decode(want, cdtype), z.astype(cdtype)), (n, x, y, cdtype)


@pytest.mark.parametrize("n", [2048, 16384])
def test_impulse_closed_forms_agree_with_the_model(n):
    """m_j = (2/n) Re(z_k zeta^(-j e(k))) for one unit slot, z_k = v zeta^(j e(k)) for one coefficient: the model's transform has
    log2(n/2) + 1 <= 14 roundings per value on top of its twiddles', so 16 eps of long double times the magnitude bounds the difference."""
    eps = float(np.finfo(LD).eps)
    for k in (0, 1, n // 4, n // 2 - 1):
        for zk in (1.0, 1j):
            z = np.zeros(n // 2, dtype=np.complex128)
            z[k] = zk
            assert float(np.max(np.abs(encode(z, n) - impulse_plaintext(n, k, zk)))) <= 16 * eps * 2 / n, (n, k, zk)
    for j in (1, 15, 16, n // 2 - 1, n // 2 + 1, n - 1):
        m = np.zeros(n, dtype=LD)
        m[j] = LD(2.0 ** 21)
        assert float(np.max(np.abs(decode(m) - impulse_slots(n, j, m[j])))) <= 16 * eps * 2.0 ** 21, (n, j)


@pytest.mark.parametrize("n", [2048, 16384])
def test_generic_slots_at_scale_2_to_61_stay_inside_the_exact_contract(n):
    """Premise of the 2^61 case of test_ckks_edges.py: max |round(scale m)| < 2^62 (about 2^60: m_0 is the mean of the unit square's real parts)."""
    from test_ckks_encoder import generic_case
    z, m, E = generic_case(n)
    for b in range(len(m)):
        top = max(abs(int(x)) for x in np.rint(LD(2.0 ** 61) * m[b]))
        print(f"n={n} b={b}: max |round(2^61 m)| = 2^{np.log2(float(top)):.3f}")
        assert top < 1 << 62, (n, b)


def test_slot_table_of_the_library_matches_python(pkg):
    for n in (2, 4, 16, 2048, 16384):
        a, c = pkg.capi.ckks_slot_table(n)
        wa, wc = slot_table(n)
        assert np.array_equal(a.astype(np.int64), wa) and np.array_equal(c, wc), n
        assert sorted(int(x) for x in wa) == list(range(n // 2))
    lib = pkg.lib()
    a = (ctypes.c_uint32 * 8)(); c = (ctypes.c_uint8 * 8)()
    assert lib.fhe_ckks_slot_table(12, a, c) == -1 and lib.fhe_ckks_slot_table(0, a, c) == -1
    assert lib.fhe_ckks_slot_table(16, None, c) == -1 and lib.fhe_ckks_slot_table(16, a, None) == -1


def test_symbols_in_header_library_and_binding(pkg):
    header = open(os.path.join(ROOT, "include", "fhe_hip.h")).read()
    for name in CKKS_NAMES:
        assert re.search(r"\b" + name + r"\b", header), name
    lib = pkg.lib()
    for name in CKKS_SYMBOLS:
        assert hasattr(lib, name) and name in lib._fhe_symbols, name
    for method in ("encode", "decode", "decode_poly", "close"):
        assert callable(getattr(pkg.capi.CkksEncoder, method)), method
    assert callable(pkg.capi.ckks_slot_table)
    out = ctypes.c_void_p(0x1234)
    assert lib.fhe_ckks_encoder_create(None, ctypes.byref(out)) == -1 and out.value == 0x1234
    assert lib.fhe_ckks_encoder_destroy(None) == 0
    assert lib.fhe_ckks_encode(None, None, None, None, None, 1.0, 1) == -1
    assert lib.fhe_ckks_decode(None, None, None, None, 0, 1.0, 1) == -1
    assert lib.fhe_ckks_decode_poly(None, None, None, None, 1.0, 1) == -1


RES_SRC = """#include "ckks.hip.h"
using namespace fhe_dev;
template __global__ void fhe_dev::ckks_encode_kernel<RES_LOGN>(char*, uint32_t*, const double*, const uint32_t*, const double2*, const double2*, const fhe_host::ModT*, double, uint32_t);
template __global__ void fhe_dev::ckks_decode_kernel<RES_LOGN, 0>(double*, const char*, const uint32_t*, const double2*, const double2*, uint64_t, double, uint32_t);
template __global__ void fhe_dev::ckks_decode_kernel<RES_LOGN, 1>(double*, const char*, const uint32_t*, const double2*, const double2*, uint64_t, double, uint32_t);
"""


def _pinned():
    out = {}
    for line in open(os.path.join(ROOT, "tests", "golden", "ckks_encoder_resources.txt")).read().splitlines():
        if line and not line.startswith("#"):
            n, kernel, vgprs, occ = line.split()
            out[(int(n), kernel)] = (int(vgprs), int(occ))
    return out


def _kernel_of(name):
    if "ckks_encode_kernel" in name:
        return "encode"
    if "ckks_decode_kernel" in name:
        return "decode_poly" if re.search(r"ILi\d+ELi1EE", name) else "decode"
    return None


def test_ckks_kernels_compile_without_scratch_and_keep_their_pinned_budgets(tmp_path):
    """The twelve instances (N = 2^11 .. 2^14, three kernels each) compile for gfx950 with no spill, no scratch and an LDS footprint of two
    padded planes of n/2 doubles (17 n / 2 bytes; encode has one more 8-byte word, the plaintext's maximum): 136 KiB of the 160 KiB at
    N = 2^14.  VGPRs and waves per SIMD are bounds (tests/golden/ckks_encoder_resources.txt)."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    (tmp_path / "ckks_res.hip").write_text(RES_SRC)
    jobs = [(n, [HIPCC, *RES_FLAGS, f"-DRES_LOGN={n}", "-c", "-o", str(tmp_path / f"c_{n}.o"), str(tmp_path / "ckks_res.hip")]) for n in (11, 12, 13, 14)]

    def run(job):
        res = subprocess.run(job[1], capture_output=True, text=True, timeout=1500)
        assert res.returncode == 0, res.stderr[-3000:]
        lds, cur = {}, None
        for line in res.stderr.splitlines():
            if "Function Name: " in line:
                cur = line.split("Function Name: ")[1].split()[0]
            elif "LDS Size [bytes/block]: " in line and cur:
                lds[cur] = int(line.split("LDS Size [bytes/block]: ")[1].split()[0])
        return job[0], (_resource_remarks(res.stderr), lds)

    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as ex:
        got = dict(ex.map(run, jobs))
    pinned, seen = _pinned(), {}
    for n, (remarks, lds) in got.items():
        for name, r in remarks.items():
            k = _kernel_of(name)
            if k is None:
                continue
            print(n, k, r, lds[name])
            assert r.get("spill", 0) == 0 and r.get("scratch", 0) == 0, (n, k, r)
            assert lds[name] == 17 * (1 << n) // 2 + (8 if k == "encode" else 0), (n, k, lds[name])
            assert lds[name] <= 160 * 1024
            seen[(n, k)] = (r["vgprs"], r["occupancy"])
    assert len(seen) == 12 and sorted(seen) == sorted(pinned), sorted(seen)
    worse = {k: (seen[k], pinned[k]) for k in seen if seen[k][0] > pinned[k][0] or seen[k][1] < pinned[k][1]}
    assert not worse, worse
