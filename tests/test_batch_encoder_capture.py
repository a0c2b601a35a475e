"""Builds tests/cpp/test_batch_encoder_capture.cpp with hipcc and runs it: after the reserves, encode -> encrypt -> decrypt -> decode captured into
one hipGraph on a caller-owned stream and replayed twice with new slot values returns those values, on the fused path (N = 2048, two fields of
the target) and on the composed path (N = 1024, and N = 2048 under FHE_HIP_NO_FUSED_ENCODE=1); workspaces and scratch do not change."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_batch_encoder_capture.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "test_batch_encoder_capture")


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


def test_encoder_capture_test_compiles(pkg):
    _build(pkg)


# (prime_bits, n, L, batch), environment, whether the encoder holds scratch (the composed path)
@pytest.mark.gpu
@pytest.mark.parametrize("args,env,scratch", [
    (("30", "2048", "2", "3"), {}, False),
    (("40", "4096", "2", "2"), {}, False),
    (("30", "1024", "2", "3"), {}, True),
    (("30", "2048", "2", "3"), {"FHE_HIP_NO_FUSED_ENCODE": "1"}, True),
])
def test_a_captured_round_trip_replays_with_new_inputs(pkg, args, env, scratch):
    exe = _build(pkg)
    res = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, env={**os.environ, **env})
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "encoder capture ok" in res.stdout
    got = int(res.stdout.split("scratch ")[1].split(" bytes")[0])
    assert (got > 0) == scratch and (not scratch or got >= int(args[3]) * int(args[1]) * 32), res.stdout
