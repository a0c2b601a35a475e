"""Builds tests/cpp/test_ct_bootstrap_mirror.cpp against include/fhe/*.hpp + libfhe_hip.so with g++ (as the other mirror tests do) and runs it:
null-handle rejection of the two new entry points on CPU; on the GPU box FHEContext::bootstrap(Ciphertext&) refreshes a ciphertext of four
coefficients in the scaled encoding, twice in a row (f, then g), for all 8 messages, and throws on foreign keys, 3 components and a bad count."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_ct_bootstrap_mirror.cpp")
OUT_DIR = os.path.join(ROOT, "tests", "cpp", "_build")
EXE = os.path.join(OUT_DIR, "test_ct_bootstrap_mirror")


def _build(pkg):
    pkg.build_library()
    lib_dir = os.path.dirname(pkg.library_path())
    os.makedirs(OUT_DIR, exist_ok=True)
    deps = [SRC, pkg.library_path()] + [os.path.join(ROOT, "include", "fhe", f) for f in os.listdir(os.path.join(ROOT, "include", "fhe"))]
    deps.append(os.path.join(ROOT, "include", "fhe_hip.h"))
    if os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(d) for d in deps):
        return EXE
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), SRC, "-L", lib_dir, "-lfhe_hip",
           f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-o", EXE]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return EXE


def test_ct_bootstrap_mirror_compiles_and_rejects_null_handles(pkg):
    exe = _build(pkg)
    res = subprocess.run([exe, "--host-only"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host-only: PASSED" in res.stdout


@pytest.mark.gpu
def test_ct_bootstrap_mirror_on_gpu(pkg):
    exe = _build(pkg)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ALL PASSED" in res.stdout
