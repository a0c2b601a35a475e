"""GPU test of the engine's workspace table (csrc/engine.h: WsId, Workspace, grow_ws): every reserve that owns a workspace grows
fhe_rns_ntt_workspace_bytes by exactly what it grew it by before the sixteen loose fields became the table, the hoist buffer is reported by
fhe_rns_ntt_hoist_bytes alone, and destroying an engine gives every workspace back.

One engine shape (n = 2048, L = 2, 30-bit primes, batch 2), two engines: the default one, and one created under the switches that put
encryption, decryption, the hoisted rotations and the packing on their composed paths, where WS_ENC and container-sized WS_DEC / WS_HOIST /
WS_LIN / WS_PACK exist at all.  EXPECTED holds (workspace_bytes, hoist_bytes) after each call as the commit before the table reported them
for this script on an MI355X; the sizes are arithmetic on (n, L, batch, K), not measurements, so they hold on any device.

Free memory is read with hipMemGetInfo through torch, so the script runs in a fresh interpreter that imports torch first (one libamdhip64
per process, as in test_torch_interop.py).  After two warm-up cycles (code objects loaded, runtime pools grown) the free memory is read
beside a fresh engine that holds no workspace, before and after CYCLES further create / reserve-everything / destroy cycles of both
engines, and must be where it was.  On the commit before the table free memory moved in steps of 2 MiB (64 KiB allocations one after
another: a step at every 32nd), so the bound is one step: the smallest workspace here is 256 KiB, and CYCLES = 16 cycles that each
forget it hold back 4 MiB."""
import json
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ("keys", "reserve", "reserve_hoist", "linear_transform_reserve", "ct_encrypt_reserve", "ct_decrypt_reserve", "lwe_pack_reserve")
COMPOSED = ("FHE_HIP_NO_FUSED_ENCRYPT", "FHE_HIP_NO_FUSED_DECRYPT", "FHE_HIP_NO_FUSED_HOIST", "FHE_HIP_NO_FUSED_PACK")
CYCLES, GRANULARITY = 16, 2 << 20
EXPECTED = {
    "fused": [[0, 0], [720896, 0], [720896, 131072], [786432, 131072], [786432, 131072], [819200, 131072], [7831552, 131072]],
    "composed": [[0, 0], [720896, 0], [720896, 1048576], [1245184, 1048576], [1507328, 1048576], [2031616, 1048576], [13762848, 1048576]],
}

SCRIPT = textwrap.dedent(r"""
    import importlib, json, os, sys
    import numpy as np
    import torch                                              # first: one HIP runtime per process
    sys.path[:0] = [%(root)r]
    pkg = importlib.import_module("gpu-homomorphic-encryption_amd")
    n, L, batch, w, count, t, sigma = 2048, 2, 2, 16, 8, 65537, 3.2
    moduli = pkg.find_ntt_primes(30, n, L)
    s = np.random.default_rng(9).integers(-1, 2, n)
    s_rns = np.zeros((L, n, 4), np.uint64)
    for l, q in enumerate(moduli):
        s_rns[l, :, 0] = (s %% q).astype(np.uint64)

    def cycle(composed):
        # one engine with its keys, every reserve that owns a workspace, and everything destroyed again
        for name in %(composed)r:
            os.environ.pop(name, None)
            if composed:
                os.environ[name] = "1"
        eng = pkg.RnsNttEngine(n, moduli)
        seen = []
        mark = lambda: seen.append([eng.workspace_bytes(), eng.hoist_bytes()])
        ds = pkg.DeviceBuffer.from_numpy(s_rns)
        sk = eng.import_secret_key(ds)
        keys = eng.generate_keyswitch_keys(sk, w, pkg.capi.lwe_pack_galois_elements(n), 1, sigma, (0x51, 0x52))
        plain = pkg.DeviceBuffer.from_numpy(s_rns)
        lt = eng.linear_transform_create(w, [3, 1], [keys[0], None], [plain, plain])
        mark()
        eng.reserve(batch); mark()
        eng.reserve_hoist(w, batch); mark()
        eng.linear_transform_reserve(lt, batch); mark()
        eng.encrypt_reserve(sigma, batch); mark()
        eng.decrypt_reserve(t, 3, batch); mark()
        eng.lwe_pack_reserve(keys, count, True, batch); mark()
        pkg.capi.sync()
        for obj in [lt, *keys, sk, eng]:
            obj.close()
        ds.free(); plain.free()
        return seen

    def free_bytes():
        pkg.capi.sync()
        return torch.cuda.mem_get_info()[0]

    out = {"fused": cycle(False), "composed": cycle(True)}
    bare = pkg.RnsNttEngine(n, moduli)                        # both readings are taken beside one engine that holds no workspace
    out["free_before"] = free_bytes()
    bare.close()
    for _ in range(%(cycles)d):
        assert cycle(False) == out["fused"] and cycle(True) == out["composed"]
    bare = pkg.RnsNttEngine(n, moduli)
    out["free_after"] = free_bytes()
    bare.close()
    print("RESULT " + json.dumps(out))
""")


def run_script(root=ROOT, cycles=CYCLES):
    """The script's RESULT line as a dict (scripts that measure the numbers on another checkout call this with its root)."""
    env = dict(os.environ); env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    for name in COMPOSED:
        env.pop(name, None)
    res = subprocess.run([sys.executable, "-c", SCRIPT % {"root": root, "composed": COMPOSED, "cycles": cycles}], capture_output=True, text=True, timeout=300, env=env)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")]
    assert res.returncode == 0 and lines, res.stdout[-2000:] + res.stderr[-4000:]
    return json.loads(lines[-1][7:])


@pytest.fixture(scope="module")
def result(pkg):
    return run_script()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fused", "composed"])
def test_every_reserve_grows_the_count_by_what_it_did_before_the_table(result, path):
    got = dict(zip(STEPS, result[path]))
    print(path, got)
    assert result[path] == EXPECTED[path], got
    # the hoist buffer moves for the hoist reserve alone (the linear transform's reserve asks for the same size), and that reserve, coming
    # after reserve(batch), does not move workspace_bytes: the buffer is not counted there
    ws, hoist = zip(*result[path])
    for i, step in enumerate(STEPS[1:], 1):
        if step == "reserve_hoist":
            assert hoist[i] > hoist[i - 1] and ws[i] == ws[i - 1], got
        else:
            assert hoist[i] == hoist[i - 1] and ws[i] >= ws[i - 1], (step, got)


@pytest.mark.gpu
def test_destroying_the_engine_returns_every_workspace(result):
    drift = result["free_before"] - result["free_after"]
    print("free memory before / after %d cycles: %d / %d (drift %d bytes)" % (CYCLES, result["free_before"], result["free_after"], drift))
    assert abs(drift) <= GRANULARITY, drift
