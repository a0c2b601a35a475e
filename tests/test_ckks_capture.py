"""Builds tests/cpp/test_ckks_capture.cpp with hipcc and runs it: fhe_ckks_encode, fhe_ckks_decode_poly and fhe_ckks_decode captured into one
hipGraph on a caller-owned stream and replayed twice with new slots give the bits of the direct calls on the same inputs; the workspace byte
count does not change across the calls."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_ckks_capture.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "test_ckks_capture")


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


def test_ckks_capture_test_compiles(pkg):
    _build(pkg)


@pytest.mark.gpu
@pytest.mark.parametrize("args", [("30", "2048", "2", "3"), ("60", "16384", "3", "2")])
def test_captured_encode_and_decode_replay_with_new_inputs(pkg, args):
    exe = _build(pkg)
    res = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ckks capture ok: 3 nodes" in res.stdout
