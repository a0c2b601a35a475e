"""Builds tests/cpp/test_lwe_keyswitch_capture.cpp with hipcc and runs it: after the reserves the chainable bootstrap, prepare -> loop -> rescale
to one prime -> extract -> fhe_lwe_keyswitch, captured into a hipGraph on a caller-owned stream and replayed twice over fresh inputs gives the
bits of the direct calls, and the workspaces do not change across the key switch."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_lwe_keyswitch_capture.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "test_lwe_keyswitch_capture")


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


def test_lwe_keyswitch_capture_test_compiles(pkg):
    _build(pkg)


# the shape of test_bootstrap_chain.py (N = 2048, two 30-bit primes, RGSW w = 16, n_lwe = 12, batch 4, key switch w = 8, modulus kept), and an
# 8-byte field whose 60-bit first prime needs the modulus switch down to 2^32 in the epilogue (wide accumulators, odd step count)
@pytest.mark.gpu
@pytest.mark.parametrize("args", [("30", "2048", "4", "12", "16", "8", "0"), ("60", "2048", "3", "5", "32", "8", "4294967296")])
def test_a_captured_chainable_bootstrap_replays_the_direct_result(pkg, args):
    exe = _build(pkg)
    res = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "lwe keyswitch capture ok" in res.stdout
