"""Builds tests/cpp/test_bfv_capture.cpp with hipcc and runs it: after fhe_bfv_multiplier_reserve(m, batch, rk), fhe_bfv_multiply_relin captured into
one hipGraph on a caller-owned stream and replayed twice gives the direct call's bits, on the 4-byte and on an 8-byte field; the multiplier's and
the engine's workspaces do not change from the reserve on."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_bfv_capture.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "test_bfv_capture")


def _build(pkg):
    pkg.build_library()
    lib_dir = os.path.dirname(pkg.library_path())
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "include", "fhe_hip.h")]
    if os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(d) for d in deps):
        return EXE
    cmd = ["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), SRC, "-L", lib_dir, "-lfhe_hip", f"-Wl,-rpath,{lib_dir}", "-o", EXE]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return EXE


def test_bfv_capture_test_compiles(pkg):
    _build(pkg)


# (prime_bits, n, L, L', batch): 30-bit primes need four auxiliary primes for two ciphertext primes (P > 32 t n Q), 60-bit ones three
@pytest.mark.gpu
@pytest.mark.parametrize("args", [("30", "2048", "2", "4", "3"), ("60", "2048", "2", "3", "2")])
def test_a_captured_multiply_relin_replays_the_direct_bits(pkg, args):
    exe = _build(pkg)
    res = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "bfv capture ok" in res.stdout
