"""Builds tests/cpp/test_decrypt_capture.cpp with hipcc and runs it: after fhe_ct_decrypt_reserve one fhe_ct_decrypt captured into a hipGraph
on a caller-owned stream and replayed twice gives the eager result; the graph is a single chain with no parallel branches and the memset of
d_noise_bits is one of its nodes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_decrypt_capture.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "test_decrypt_capture")


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


def test_decrypt_capture_test_compiles(pkg):
    _build(pkg)


# the fused path is three nodes (ntt_decrypt_kernel, the memset, decrypt_crt_kernel); the composition's count is printed
@pytest.mark.gpu
@pytest.mark.parametrize("args,env,nodes", [
    (("30", "2048", "2", "3", "2"), {}, 3),
    (("30", "2048", "2", "3", "3"), {}, 3),
    (("60", "4096", "2", "2", "3"), {}, 3),
    (("30", "2048", "2", "3", "3"), {"FHE_HIP_NO_FUSED_DECRYPT": "1"}, None),
])
def test_a_captured_decrypt_replays_the_eager_result(pkg, args, env, nodes):
    exe = _build(pkg)
    res = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, env={**os.environ, **env})
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "decrypt capture ok" in res.stdout
    got = int(res.stdout.split("decrypt capture ok: ")[1].split(" nodes")[0])
    assert got >= 3 and (nodes is None or got == nodes), res.stdout
