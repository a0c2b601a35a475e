"""Builds tests/cpp/test_rlwe_pack_capture.cpp with hipcc and runs it: after fhe_lwe_pack_reserve one fhe_rlwe_sample_extract_strided and one
fhe_rlwe_pack, captured together into a hipGraph on a caller-owned stream and replayed twice over poisoned outputs, give the bits of the eager
calls, and the workspace does not change across them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_rlwe_pack_capture.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "test_rlwe_pack_capture")


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


def test_rlwe_pack_capture_test_compiles(pkg):
    _build(pkg)


@pytest.mark.gpu
def test_captured_extraction_and_packing_replay_the_eager_bits(pkg):
    res = subprocess.run([_build(pkg)], capture_output=True, text=True, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "rlwe pack capture ok" in res.stdout
