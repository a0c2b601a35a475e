"""Builds tests/cpp/test_bootstrap_capture.cpp with hipcc and runs it: after fhe_rns_ntt_reserve the sequence fhe_lwe_prepare_accumulator ->
fhe_blind_rotate -> fhe_rlwe_sample_extract captured into a hipGraph on a caller-owned stream and replayed twice gives the bits of the direct calls."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_bootstrap_capture.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "test_bootstrap_capture")


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


def test_bootstrap_capture_test_compiles(pkg):
    _build(pkg)


# the set-up of test_bootstrap_end_to_end.py (N = 2048, two 30-bit primes, w = 16, n_lwe = 12, batch 4) and an 8-byte field with an odd step count
@pytest.mark.gpu
@pytest.mark.parametrize("args", [("30", "2048", "2", "4", "12", "16"), ("60", "2048", "2", "3", "5", "32")])
def test_a_captured_bootstrap_replays_the_direct_result(pkg, args):
    exe = _build(pkg)
    res = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "bootstrap capture ok" in res.stdout
