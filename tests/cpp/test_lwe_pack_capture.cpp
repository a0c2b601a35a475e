// test_lwe_pack_capture.cpp -- after fhe_lwe_pack_reserve one fhe_lwe_pack (count = 4, trace, normalisation, batch 2; N = 2048, two 30-bit
// primes, w = 16) is capturable into a hipGraph on a caller-owned stream: the capture is a linear chain (every node has at most one
// predecessor and one successor, nodes - 1 edges), the workspace does not change across the call, and a replay over poisoned outputs gives the
// bits of the eager call.  Every HIP or library error ends the program at once with a non-zero status.  Build: hipcc.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fhe_hip.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "HIP %s at line %d\n", hipGetErrorString(e_), __LINE__); std::exit(1); } } while (0)
#define FHE_OK_(x) do { int rc_ = (x); if (rc_ != 0) { std::fprintf(stderr, "fhe error %d (%s) at line %d\n", rc_, fhe_hip_last_error(), __LINE__); std::exit(1); } } while (0)

int main() {
    const uint32_t n = 2048, L = 2, w = 16, count = 4, batch = 2, log_n = 11;
    const uint64_t seeds[2] = {31, 32};
    std::vector<uint64_t> primes(L); FHE_OK_(fhe_find_ntt_primes(30, n, L, primes.data()));
    std::vector<uint64_t> moduli((size_t)L * 4, 0); for (uint32_t l = 0; l < L; l++) moduli[(size_t)l * 4] = primes[l];
    fhe_rns_ntt_t *h = nullptr; FHE_OK_(fhe_rns_ntt_create(&h, n, (const uint64_t (*)[4])moduli.data(), L));
    hipStream_t s; HIP_OK(hipStreamCreate(&s)); FHE_OK_(fhe_rns_ntt_set_stream(h, s));

    uint64_t seed = 77;
    auto next = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return seed >> 20; };
    const size_t S = (size_t)L * n * 32, out_bytes = batch * S, lwe_words = (size_t)batch * count * L * (n + 1);
    std::vector<uint64_t> host((size_t)L * n * 4, 0), lwe(lwe_words);
    for (uint32_t x = 0; x < n; x++) { const uint64_t r = next() % 3; for (uint32_t l = 0; l < L; l++) host[((size_t)l * n + x) * 4] = r == 2 ? primes[l] - 1 : r; }
    for (size_t i = 0; i < lwe_words; i++) lwe[i] = next() % primes[(i / (n + 1)) % L];
    void *d_s, *d_lwe, *d_out[4];
    HIP_OK(hipMalloc(&d_s, S)); HIP_OK(hipMemcpy(d_s, host.data(), S, hipMemcpyHostToDevice));
    HIP_OK(hipMalloc(&d_lwe, lwe_words * 8)); HIP_OK(hipMemcpy(d_lwe, lwe.data(), lwe_words * 8, hipMemcpyHostToDevice));
    for (void *&p : d_out) HIP_OK(hipMalloc(&p, out_bytes));
    fhe_secret_key_t *sk = nullptr; FHE_OK_(fhe_secret_key_create(h, &sk, d_s));
    std::vector<uint32_t> elts(log_n); FHE_OK_(fhe_lwe_pack_galois_elements(n, elts.data()));
    for (uint32_t j = 1; j <= log_n; j++) if (elts[j - 1] != (1u << j) + 1) { std::fprintf(stderr, "element %u is %u\n", j, elts[j - 1]); return 1; }
    std::vector<fhe_relin_keys_t *> gks(log_n, nullptr);
    FHE_OK_(fhe_keyswitch_keys_generate(h, sk, w, elts.data(), log_n, 1, 3.2, seeds, gks.data()));

    FHE_OK_(fhe_lwe_pack_reserve(h, gks.data(), count, 1, batch));
    uint64_t ws0 = 0, ws1 = 0; FHE_OK_(fhe_rns_ntt_workspace_bytes(h, &ws0));
    if (ws0 < 3ull * batch * count * S) { std::fprintf(stderr, "the reserve left %llu bytes, below 3 batch count S\n", (unsigned long long)ws0); return 1; }
    FHE_OK_(fhe_lwe_pack(h, gks.data(), d_out[0], d_out[1], (const uint64_t *)d_lwe, count, 1, 1, batch));
    HIP_OK(hipStreamSynchronize(s));
    FHE_OK_(fhe_rns_ntt_workspace_bytes(h, &ws1));
    if (ws0 != ws1) { std::fprintf(stderr, "the workspace changed across the call\n"); return 1; }

    hipGraph_t graph; hipGraphExec_t exec;
    HIP_OK(hipStreamBeginCapture(s, hipStreamCaptureModeGlobal));
    FHE_OK_(fhe_lwe_pack(h, gks.data(), d_out[2], d_out[3], (const uint64_t *)d_lwe, count, 1, 1, batch));
    HIP_OK(hipStreamEndCapture(s, &graph));
    size_t nodes = 0, edges = 0;
    HIP_OK(hipGraphGetNodes(graph, nullptr, &nodes)); HIP_OK(hipGraphGetEdges(graph, nullptr, nullptr, &edges));
    // two merge levels (one streaming launch + at least one launch of the key switch each), the last sum, nine trace steps
    if (nodes < 2 * 2 + 1 + 9 * 2) { std::fprintf(stderr, "the captured graph has only %zu nodes\n", nodes); return 1; }
    if (edges != nodes - 1) { std::fprintf(stderr, "%zu nodes and %zu edges: not a chain\n", nodes, edges); return 1; }
    std::vector<hipGraphNode_t> from(edges), to(edges), all(nodes);
    HIP_OK(hipGraphGetEdges(graph, from.data(), to.data(), &edges)); HIP_OK(hipGraphGetNodes(graph, all.data(), &nodes));
    for (hipGraphNode_t v : all) {
        size_t in = 0, out = 0;
        for (size_t i = 0; i < edges; i++) { in += to[i] == v; out += from[i] == v; }
        if (in > 1 || out > 1) { std::fprintf(stderr, "a node has %zu predecessors and %zu successors: parallel branches\n", in, out); return 1; }
    }
    HIP_OK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    std::vector<uint64_t> want(2 * out_bytes / 8), got(2 * out_bytes / 8);
    for (int c = 0; c < 2; c++) HIP_OK(hipMemcpy(want.data() + c * out_bytes / 8, d_out[c], out_bytes, hipMemcpyDeviceToHost));
    for (int c = 2; c < 4; c++) HIP_OK(hipMemsetAsync(d_out[c], 0x5A, out_bytes, s));
    HIP_OK(hipGraphLaunch(exec, s));
    HIP_OK(hipStreamSynchronize(s));
    for (int c = 0; c < 2; c++) HIP_OK(hipMemcpy(got.data() + c * out_bytes / 8, d_out[2 + c], out_bytes, hipMemcpyDeviceToHost));
    if (got != want) { std::fprintf(stderr, "the graph replay differs from the eager call\n"); return 1; }
    std::printf("lwe pack capture ok: %zu nodes in a chain, replay bit-identical to the eager call (n %u count %u batch %u)\n", nodes, n, count, batch);
    HIP_OK(hipGraphExecDestroy(exec)); HIP_OK(hipGraphDestroy(graph));
    for (fhe_relin_keys_t *k : gks) FHE_OK_(fhe_relin_keys_destroy(k));
    FHE_OK_(fhe_secret_key_destroy(sk)); FHE_OK_(fhe_rns_ntt_destroy(h));
    for (void *p : {d_s, d_lwe, d_out[0], d_out[1], d_out[2], d_out[3]}) HIP_OK(hipFree(p));
    HIP_OK(hipStreamDestroy(s));
    return 0;
}
