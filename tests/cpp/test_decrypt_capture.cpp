// test_decrypt_capture.cpp -- after fhe_ct_decrypt_reserve a fhe_ct_decrypt call is capturable into a hipGraph (include/fhe_hip.h): one call
// captured on a caller-owned stream and replayed twice over outputs filled with 0xFF gives the directly launched result.  The graph is a
// single chain (no node with two successors or two predecessors) and holds the memset of d_noise_bits: a replay over 0xFF-filled noise bits
// could not give the eager values without it (the kernel only raises them).  Every HIP or library error ends the program at once with a
// non-zero status.  Build: hipcc (needs the HIP runtime API).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fhe_hip.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "HIP %s at line %d\n", hipGetErrorString(e_), __LINE__); std::exit(1); } } while (0)
#define FHE_OK_(x) do { int rc_ = (x); if (rc_ != 0) { std::fprintf(stderr, "fhe error %d (%s) at line %d\n", rc_, fhe_hip_last_error(), __LINE__); std::exit(1); } } while (0)

// usage: test_decrypt_capture prime_bits n L batch components   (the path -- two launches or the composition -- is the library's choice for the
// shape and for FHE_HIP_NO_FUSED_DECRYPT; the node count printed tells them apart)
int main(int argc, char **argv) {
    if (argc != 6) { std::fprintf(stderr, "usage: %s prime_bits n L batch components\n", argv[0]); return 2; }
    const uint32_t bits = (uint32_t)std::atoi(argv[1]), n = (uint32_t)std::atoi(argv[2]), L = (uint32_t)std::atoi(argv[3]), batch = (uint32_t)std::atoi(argv[4]),
                   nc = (uint32_t)std::atoi(argv[5]);
    if (!bits || !n || !L || L > 16 || !batch || nc < 2 || nc > 3) { std::fprintf(stderr, "bad arguments\n"); return 2; }
    const uint64_t t = 65537, scale = 3;
    std::vector<uint64_t> primes(L); FHE_OK_(fhe_find_ntt_primes(bits, n, L, primes.data()));
    std::vector<uint64_t> moduli((size_t)L * 4, 0); for (uint32_t l = 0; l < L; l++) moduli[(size_t)l * 4] = primes[l];
    fhe_rns_ntt_t *h = nullptr; FHE_OK_(fhe_rns_ntt_create(&h, n, (const uint64_t (*)[4])moduli.data(), L));
    hipStream_t s; HIP_OK(hipStreamCreate(&s));
    FHE_OK_(fhe_rns_ntt_set_stream(h, s));

    const size_t poly = (size_t)L * n * 4, key_bytes = poly * 8, bytes = (size_t)batch * key_bytes;      // u64 words
    const size_t m_bytes = (size_t)batch * n * 8, b_bytes = (size_t)batch * 4;
    std::vector<uint64_t> host((size_t)batch * poly, 0);
    auto fill = [&](uint64_t seed, uint32_t count) { for (uint32_t b = 0; b < count; b++) for (uint32_t l = 0; l < L; l++) for (uint32_t x = 0; x < n; x++) {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull; host[((size_t)(b * L + l) * n + x) * 4] = (seed >> 20) % primes[l]; } };
    void *d_s, *d_c[3] = {nullptr, nullptr, nullptr}, *d_m[2], *d_b[2];
    HIP_OK(hipMalloc(&d_s, key_bytes)); fill(1000, 1); HIP_OK(hipMemcpy(d_s, host.data(), key_bytes, hipMemcpyHostToDevice));
    for (uint32_t i = 0; i < nc; i++) { HIP_OK(hipMalloc(&d_c[i], bytes)); fill(2000 + i, batch); HIP_OK(hipMemcpy(d_c[i], host.data(), bytes, hipMemcpyHostToDevice)); }
    for (int i = 0; i < 2; i++) { HIP_OK(hipMalloc(&d_m[i], m_bytes)); HIP_OK(hipMalloc(&d_b[i], b_bytes)); }
    fhe_secret_key_t *sk = nullptr; FHE_OK_(fhe_secret_key_create(h, &sk, d_s));
    FHE_OK_(fhe_ct_decrypt_reserve(h, t, nc, batch));
    uint64_t ws_before = 0, ws_after = 0; FHE_OK_(fhe_rns_ntt_workspace_bytes(h, &ws_before));

    // reference result by a direct call
    FHE_OK_(fhe_ct_decrypt(h, sk, t, scale, (uint64_t *)d_m[0], (uint32_t *)d_b[0], d_c, nc, batch));
    HIP_OK(hipStreamSynchronize(s));
    std::vector<uint64_t> want_m((size_t)batch * n), got_m(want_m.size());
    std::vector<uint32_t> want_b(batch), got_b(batch);
    HIP_OK(hipMemcpy(want_m.data(), d_m[0], m_bytes, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(want_b.data(), d_b[0], b_bytes, hipMemcpyDeviceToHost));
    for (uint32_t b = 0; b < batch; b++) if (!want_b[b] || want_b[b] > 255) { std::fprintf(stderr, "implausible noise bits %u\n", want_b[b]); return 1; }

    // capture the same call
    hipGraph_t graph; hipGraphExec_t exec;
    HIP_OK(hipStreamBeginCapture(s, hipStreamCaptureModeGlobal));
    FHE_OK_(fhe_ct_decrypt(h, sk, t, scale, (uint64_t *)d_m[1], (uint32_t *)d_b[1], d_c, nc, batch));
    HIP_OK(hipStreamEndCapture(s, &graph));
    size_t nodes = 0, edges = 0; HIP_OK(hipGraphGetNodes(graph, nullptr, &nodes)); HIP_OK(hipGraphGetEdges(graph, nullptr, nullptr, &edges));
    std::vector<hipGraphNode_t> nd(nodes), from(edges), to(edges);
    HIP_OK(hipGraphGetNodes(graph, nd.data(), &nodes));
    if (edges) HIP_OK(hipGraphGetEdges(graph, from.data(), to.data(), &edges));
    size_t memsets = 0;
    for (hipGraphNode_t v : nd) {
        hipGraphNodeType ty; HIP_OK(hipGraphNodeGetType(v, &ty));
        if (ty == hipGraphNodeTypeMemset) memsets++;
        size_t out_deg = 0, in_deg = 0;
        for (size_t e = 0; e < edges; e++) { out_deg += from[e] == v; in_deg += to[e] == v; }
        if (out_deg > 1 || in_deg > 1) { std::fprintf(stderr, "the captured graph branches: a node with %zu successors and %zu predecessors\n", out_deg, in_deg); return 1; }
    }
    if (nodes < 3 || edges != nodes - 1) { std::fprintf(stderr, "the captured graph is no single chain: %zu nodes, %zu edges\n", nodes, edges); return 1; }
    if (memsets != 1) { std::fprintf(stderr, "the memset of d_noise_bits is not part of the capture (%zu memset nodes)\n", memsets); return 1; }
    HIP_OK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    FHE_OK_(fhe_rns_ntt_workspace_bytes(h, &ws_after));
    if (ws_after != ws_before) { std::fprintf(stderr, "the workspace changed across the calls after the reserve: %llu -> %llu bytes\n", (unsigned long long)ws_before, (unsigned long long)ws_after); return 1; }
    for (int rep = 0; rep < 2; rep++) {
        HIP_OK(hipMemsetAsync(d_m[1], 0xFF, m_bytes, s)); HIP_OK(hipMemsetAsync(d_b[1], 0xFF, b_bytes, s));
        HIP_OK(hipGraphLaunch(exec, s));
        HIP_OK(hipStreamSynchronize(s));
        HIP_OK(hipMemcpy(got_m.data(), d_m[1], m_bytes, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(got_b.data(), d_b[1], b_bytes, hipMemcpyDeviceToHost));
        if (got_m != want_m) { std::fprintf(stderr, "graph replay %d differs from the direct call (d_m)\n", rep); return 1; }
        if (got_b != want_b) { std::fprintf(stderr, "graph replay %d differs from the direct call (d_noise_bits)\n", rep); return 1; }
    }
    std::printf("decrypt capture ok: %zu nodes in one chain, 1 memset, 2 replays bit-identical to the direct call (bits %u n %u L %u batch %u components %u)\n", nodes,
                bits, n, L, batch, nc);
    HIP_OK(hipGraphExecDestroy(exec)); HIP_OK(hipGraphDestroy(graph));
    FHE_OK_(fhe_secret_key_destroy(sk)); FHE_OK_(fhe_rns_ntt_destroy(h));
    for (void *p : {d_s, d_c[0], d_c[1], d_c[2], d_m[0], d_m[1], d_b[0], d_b[1]}) if (p) HIP_OK(hipFree(p));
    HIP_OK(hipStreamDestroy(s));
    return 0;
}
