"""Builds tests/cpp/test_ckks_mirror.cpp against include/fhe/*.hpp + libfhe_hip.so with g++ (as the other mirror tests do) and runs it: defaults
and rejections on the CPU; on the GPU CKKSEncoder, encrypt_ckks, one multiply + relinearize + rescale_to_next and decrypt_ckks, whose outputs
are held here against z1 z2 under the two assertions of the end-to-end case of test_ckks_encoder.py (check_product, the long-double model)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_ckks_mirror.cpp")
OUT_DIR = os.path.join(ROOT, "tests", "cpp", "_build")
EXE = os.path.join(OUT_DIR, "test_ckks_mirror")


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


def test_ckks_mirror_compiles_and_checks_the_host_side(pkg):
    exe = _build(pkg)
    res = subprocess.run([exe, "--host-only"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host-only: PASSED" in res.stdout


@pytest.mark.gpu
def test_ckks_mirror_product_on_gpu(pkg, tmp_path):
    from test_ckks_encoder import check_product
    exe = _build(pkg)
    out = tmp_path / "mirror.bin"
    res = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=600)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ALL PASSED" in res.stdout
    raw = out.read_bytes()
    n, scale_out = np.frombuffer(raw, np.float64, 2)
    n = int(n); h = n // 2
    assert n == 2048 and 2.0 ** 30.9 < scale_out < 2.0 ** 31.1
    z1, z2, got = (np.frombuffer(raw, np.complex128, h, 16 + 16 * h * i) for i in range(3))
    v = np.frombuffer(raw, np.int64, n, 16 + 48 * h).astype(object)
    check_product(n, v[None], got[None], (z1 * z2)[None], float(scale_out), "mirror product")
