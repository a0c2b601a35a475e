"""CPU test (hipcc cross-compiles without a GPU): the streaming kernels of FHEContext::bootstrap(Ciphertext&) -- the strided sample extraction
and the embedding / first packing level from either source (RLWE pairs, sample rows) -- use no scratch memory and spill nothing, on both
limb-table types.  The remarks are parsed with the helper of test_kernel_resources.py."""
import os
import subprocess

import pytest

from test_kernel_resources import CSRC, FLAGS, HIPCC, _parse

SRC = """#include "lwe_pack.hip.h"
using namespace fhe_dev;
#define INST(T) \\
    template __global__ void fhe_dev::sample_extract_strided_kernel<T>(uint64_t*, const v2u64*, const v2u64*, const T*, uint32_t, uint32_t, uint32_t, uint32_t, size_t); \\
    EMBED(T, false) EMBED(T, true)
#define EMBED(T, PAIR) \\
    template __global__ void fhe_dev::embed_merge_kernel<T, RlwePairs, PAIR, v2u64, v2u64>(v2u64*, v2u64*, v2u64*, v2u64*, const v2u64*, const v2u64*, const T*, uint32_t, uint32_t, uint32_t, uint32_t, size_t); \\
    template __global__ void fhe_dev::embed_merge_kernel<T, SampleRows, PAIR, uint64_t>(v2u64*, v2u64*, v2u64*, v2u64*, const uint64_t*, const T*, uint32_t, uint32_t, uint32_t, uint32_t, size_t);
INST(Limb<F32>) INST(Limb<F64X>) INST(Limb256)
"""


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("ctboot")
    (out / "inst.hip").write_text(SRC)
    res = subprocess.run([HIPCC, *FLAGS, "-I", CSRC, "-c", "-o", str(out / "inst.o"), str(out / "inst.hip")], cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return _parse(res.stderr)[0]


@pytest.mark.parametrize("needle,instances", [("sample_extract_strided_kernel", 3), ("embed_merge_kernel", 12)])
def test_the_new_streaming_kernels_use_no_scratch(kernels, needle, instances):
    hits = {k: v for k, v in kernels.items() if needle in k}
    assert len(hits) == instances, (needle, sorted(kernels))
    for name, k in hits.items():
        assert k["scratch"] == 0 and k["spill"] == 0 and k["lds"] == 0, (name, k)
        assert k["vgprs"] <= 64, (name, k)                       # a streaming kernel: 8 waves per SIMD
