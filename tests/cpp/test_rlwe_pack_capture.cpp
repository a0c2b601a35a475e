// test_rlwe_pack_capture.cpp -- the two joints of FHEContext::bootstrap(Ciphertext&) are capturable: after fhe_lwe_pack_reserve one
// fhe_rlwe_sample_extract_strided (count = 4 coefficients of batch 2 ciphertexts) and one fhe_rlwe_pack (batch count = 8 pairs, trace,
// normalisation; N = 2048, two 30-bit primes, w = 16) go into ONE hipGraph on a caller-owned stream.  The workspace does not change across the
// eager calls, and the graph, replayed twice over poisoned outputs, gives the bits of the eager calls both times.  The runtime's queue settings
// are left alone.  Every HIP or library error ends the program at once with a non-zero status.  Build: hipcc.
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

    uint64_t seed = 79;
    auto next = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return seed >> 20; };
    const size_t S = (size_t)L * n * 32, out_bytes = batch * S, acc_bytes = (size_t)batch * count * S, lwe_bytes = (size_t)batch * count * L * (n + 1) * 8;
    auto random_polys = [&](size_t polys) {                              // [polys / L][L][n] canonical containers
        std::vector<uint64_t> v(polys * n * 4, 0);
        for (size_t p = 0; p < polys; p++) for (uint32_t x = 0; x < n; x++) v[(p * n + x) * 4] = next() % primes[p % L];
        return v;
    };
    std::vector<uint64_t> host_s((size_t)L * n * 4, 0);
    for (uint32_t x = 0; x < n; x++) { const uint64_t r = next() % 3; for (uint32_t l = 0; l < L; l++) host_s[((size_t)l * n + x) * 4] = r == 2 ? primes[l] - 1 : r; }
    void *d_s, *d_ct[2], *d_acc[2], *d_lwe[2], *d_out[4];
    HIP_OK(hipMalloc(&d_s, S)); HIP_OK(hipMemcpy(d_s, host_s.data(), S, hipMemcpyHostToDevice));
    for (void *&p : d_ct) { HIP_OK(hipMalloc(&p, out_bytes)); HIP_OK(hipMemcpy(p, random_polys((size_t)batch * L).data(), out_bytes, hipMemcpyHostToDevice)); }
    for (void *&p : d_acc) { HIP_OK(hipMalloc(&p, acc_bytes)); HIP_OK(hipMemcpy(p, random_polys((size_t)batch * count * L).data(), acc_bytes, hipMemcpyHostToDevice)); }
    for (void *&p : d_lwe) HIP_OK(hipMalloc(&p, lwe_bytes));
    for (void *&p : d_out) HIP_OK(hipMalloc(&p, out_bytes));
    fhe_secret_key_t *sk = nullptr; FHE_OK_(fhe_secret_key_create(h, &sk, d_s));
    std::vector<uint32_t> elts(log_n); FHE_OK_(fhe_lwe_pack_galois_elements(n, elts.data()));
    std::vector<fhe_relin_keys_t *> gks(log_n, nullptr);
    FHE_OK_(fhe_keyswitch_keys_generate(h, sk, w, elts.data(), log_n, 1, 3.2, seeds, gks.data()));

    FHE_OK_(fhe_lwe_pack_reserve(h, gks.data(), count, 1, batch));         // the reserve of fhe_lwe_pack serves fhe_rlwe_pack
    uint64_t ws0 = 0, ws1 = 0; FHE_OK_(fhe_rns_ntt_workspace_bytes(h, &ws0));
    FHE_OK_(fhe_rlwe_sample_extract_strided(h, (uint64_t *)d_lwe[0], d_ct[0], d_ct[1], count, batch));
    FHE_OK_(fhe_rlwe_pack(h, gks.data(), d_out[0], d_out[1], d_acc[0], d_acc[1], count, 1, 1, batch));
    HIP_OK(hipStreamSynchronize(s));
    FHE_OK_(fhe_rns_ntt_workspace_bytes(h, &ws1));
    if (ws0 != ws1) { std::fprintf(stderr, "the workspace changed across the calls\n"); return 1; }

    hipGraph_t graph; hipGraphExec_t exec;
    HIP_OK(hipStreamBeginCapture(s, hipStreamCaptureModeGlobal));
    FHE_OK_(fhe_rlwe_sample_extract_strided(h, (uint64_t *)d_lwe[1], d_ct[0], d_ct[1], count, batch));
    FHE_OK_(fhe_rlwe_pack(h, gks.data(), d_out[2], d_out[3], d_acc[0], d_acc[1], count, 1, 1, batch));
    HIP_OK(hipStreamEndCapture(s, &graph));
    size_t nodes = 0, edges = 0;
    HIP_OK(hipGraphGetNodes(graph, nullptr, &nodes)); HIP_OK(hipGraphGetEdges(graph, nullptr, nullptr, &edges));
    // the extraction, two merge levels (one streaming launch + at least one launch of the key switch each), the last sum, nine trace steps
    if (nodes < 1 + 2 * 2 + 1 + 9 * 2) { std::fprintf(stderr, "the captured graph has only %zu nodes\n", nodes); return 1; }
    if (edges != nodes - 1) { std::fprintf(stderr, "%zu nodes and %zu edges: not a chain\n", nodes, edges); return 1; }
    HIP_OK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    std::vector<uint64_t> want((2 * out_bytes + lwe_bytes) / 8), got(want.size());
    auto fetch = [&](std::vector<uint64_t> &v, void *o0, void *o1, void *lwe) {
        HIP_OK(hipMemcpy(v.data(), o0, out_bytes, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(v.data() + out_bytes / 8, o1, out_bytes, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(v.data() + 2 * out_bytes / 8, lwe, lwe_bytes, hipMemcpyDeviceToHost));
    };
    fetch(want, d_out[0], d_out[1], d_lwe[0]);
    for (int replay = 0; replay < 2; replay++) {
        for (int c = 2; c < 4; c++) HIP_OK(hipMemsetAsync(d_out[c], 0x5A, out_bytes, s));
        HIP_OK(hipMemsetAsync(d_lwe[1], 0x5A, lwe_bytes, s));
        HIP_OK(hipGraphLaunch(exec, s));
        HIP_OK(hipStreamSynchronize(s));
        fetch(got, d_out[2], d_out[3], d_lwe[1]);
        if (got != want) { std::fprintf(stderr, "replay %d of the graph differs from the eager calls\n", replay); return 1; }
    }
    std::printf("rlwe pack capture ok: %zu nodes in a chain, two replays bit-identical to the eager calls (n %u count %u batch %u)\n", nodes, n, count, batch);
    HIP_OK(hipGraphExecDestroy(exec)); HIP_OK(hipGraphDestroy(graph));
    for (fhe_relin_keys_t *k : gks) FHE_OK_(fhe_relin_keys_destroy(k));
    FHE_OK_(fhe_secret_key_destroy(sk)); FHE_OK_(fhe_rns_ntt_destroy(h));
    for (void *p : {d_s, d_ct[0], d_ct[1], d_acc[0], d_acc[1], d_lwe[0], d_lwe[1], d_out[0], d_out[1], d_out[2], d_out[3]}) HIP_OK(hipFree(p));
    HIP_OK(hipStreamDestroy(s));
    return 0;
}
