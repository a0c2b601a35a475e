// test_bootstrap_capture.cpp -- after fhe_rns_ntt_reserve the whole sequence fhe_lwe_prepare_accumulator -> fhe_blind_rotate ->
// fhe_rlwe_sample_extract is capturable into a hipGraph (include/fhe_hip.h): captured once on a caller-owned stream and replayed twice over
// accumulators, shifts and outputs filled with 0xFF it gives the directly launched LWE samples bit for bit, and the workspace does not change
// after the reserve.  Every HIP or library error ends the program at once with a non-zero status.  Build: hipcc (needs the HIP runtime API).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fhe_hip.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "HIP %s at line %d\n", hipGetErrorString(e_), __LINE__); std::exit(1); } } while (0)
#define FHE_OK_(x) do { int rc_ = (x); if (rc_ != 0) { std::fprintf(stderr, "fhe error %d (%s) at line %d\n", rc_, fhe_hip_last_error(), __LINE__); std::exit(1); } } while (0)

// usage: test_bootstrap_capture prime_bits n L batch n_lwe decomp_bits
int main(int argc, char **argv) {
    if (argc != 7) { std::fprintf(stderr, "usage: %s prime_bits n L batch n_lwe decomp_bits\n", argv[0]); return 2; }
    const uint32_t bits = (uint32_t)std::atoi(argv[1]), n = (uint32_t)std::atoi(argv[2]), L = (uint32_t)std::atoi(argv[3]), batch = (uint32_t)std::atoi(argv[4]),
                   n_lwe = (uint32_t)std::atoi(argv[5]), w = (uint32_t)std::atoi(argv[6]);
    if (!bits || !n || !L || L > 16 || !batch || !n_lwe || n_lwe > 64 || !w) { std::fprintf(stderr, "bad arguments\n"); return 2; }
    const uint64_t q_lwe = 1ull << 32, seeds[2] = {11, 12};
    std::vector<uint64_t> primes(L); FHE_OK_(fhe_find_ntt_primes(bits, n, L, primes.data()));
    std::vector<uint64_t> moduli((size_t)L * 4, 0); for (uint32_t l = 0; l < L; l++) moduli[(size_t)l * 4] = primes[l];
    fhe_rns_ntt_t *h = nullptr; FHE_OK_(fhe_rns_ntt_create(&h, n, (const uint64_t (*)[4])moduli.data(), L));
    hipStream_t s; HIP_OK(hipStreamCreate(&s));
    FHE_OK_(fhe_rns_ntt_set_stream(h, s));

    const size_t poly = (size_t)L * n * 4, S = poly * 8, acc_bytes = (size_t)batch * S;                  // u64 words, bytes
    const size_t out_bytes = (size_t)batch * L * (n + 1) * 8, sh_bytes = (size_t)n_lwe * batch * 4, lwe_bytes = (size_t)batch * (n_lwe + 1) * 8;
    uint64_t seed = 1000;
    auto next = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return seed >> 20; };
    std::vector<uint64_t> host(poly, 0), lwe((size_t)batch * (n_lwe + 1));
    void *d_s, *d_tv, *d_acc[4], *d_lwe, *d_sh, *d_out[2];
    for (uint32_t l = 0; l < L; l++) for (uint32_t x = 0; x < n; x++) { const uint64_t r = next() % 3; host[((size_t)l * n + x) * 4] = r == 2 ? primes[l] - 1 : r; }   // not the same
    HIP_OK(hipMalloc(&d_s, S)); HIP_OK(hipMemcpy(d_s, host.data(), S, hipMemcpyHostToDevice));          // polynomial per limb: nothing here decrypts
    for (uint32_t l = 0; l < L; l++) for (uint32_t x = 0; x < n; x++) host[((size_t)l * n + x) * 4] = next() % primes[l];
    HIP_OK(hipMalloc(&d_tv, S)); HIP_OK(hipMemcpy(d_tv, host.data(), S, hipMemcpyHostToDevice));
    for (uint64_t &v : lwe) v = next() % q_lwe;
    HIP_OK(hipMalloc(&d_lwe, lwe_bytes)); HIP_OK(hipMemcpy(d_lwe, lwe.data(), lwe_bytes, hipMemcpyHostToDevice));
    for (int i = 0; i < 4; i++) HIP_OK(hipMalloc(&d_acc[i], acc_bytes));
    HIP_OK(hipMalloc(&d_sh, sh_bytes));
    for (int i = 0; i < 2; i++) HIP_OK(hipMalloc(&d_out[i], out_bytes));

    fhe_secret_key_t *sk = nullptr; FHE_OK_(fhe_secret_key_create(h, &sk, d_s));
    std::vector<int32_t> mu(n_lwe); for (uint32_t i = 0; i < n_lwe; i++) mu[i] = (int32_t)(next() & 1);
    std::vector<fhe_relin_keys_t *> r0(n_lwe, nullptr), r1(n_lwe, nullptr);
    FHE_OK_(fhe_rgsw_keys_generate(h, sk, w, mu.data(), n_lwe, 1, 3.2, seeds, r0.data(), r1.data()));
    FHE_OK_(fhe_rns_ntt_reserve(h, batch));
    uint64_t ws_before = 0, ws_after = 0; FHE_OK_(fhe_rns_ntt_workspace_bytes(h, &ws_before));

    auto sequence = [&](void *out) {
        FHE_OK_(fhe_lwe_prepare_accumulator(h, q_lwe, n_lwe, (const uint64_t *)d_lwe, d_tv, d_acc[0], d_acc[1], (uint32_t *)d_sh, batch));
        FHE_OK_(fhe_blind_rotate(h, r0.data(), r1.data(), n_lwe, d_acc[0], d_acc[1], (const uint32_t *)d_sh, d_acc[2], d_acc[3], batch));
        FHE_OK_(fhe_rlwe_sample_extract(h, (uint64_t *)out, d_acc[0], d_acc[1], 0, batch));
    };
    sequence(d_out[0]);
    HIP_OK(hipStreamSynchronize(s));
    std::vector<uint64_t> want(out_bytes / 8), got(out_bytes / 8);
    HIP_OK(hipMemcpy(want.data(), d_out[0], out_bytes, hipMemcpyDeviceToHost));
    for (uint32_t p = 0; p < batch * L; p++) for (uint32_t j = 0; j <= n; j++)
        if (want[(size_t)p * (n + 1) + j] >= primes[p % L]) { std::fprintf(stderr, "a residue of the direct call is not canonical\n"); return 1; }

    hipGraph_t graph; hipGraphExec_t exec;
    HIP_OK(hipStreamBeginCapture(s, hipStreamCaptureModeGlobal));
    sequence(d_out[1]);
    HIP_OK(hipStreamEndCapture(s, &graph));
    size_t nodes = 0; HIP_OK(hipGraphGetNodes(graph, nullptr, &nodes));
    if (nodes < (size_t)n_lwe + 2) { std::fprintf(stderr, "the captured graph has %zu nodes, fewer than prepare + %u steps + extract\n", nodes, n_lwe); return 1; }
    HIP_OK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    FHE_OK_(fhe_rns_ntt_workspace_bytes(h, &ws_after));
    if (ws_after != ws_before) { std::fprintf(stderr, "the workspace changed across the calls after the reserve: %llu -> %llu bytes\n", (unsigned long long)ws_before, (unsigned long long)ws_after); return 1; }
    for (int rep = 0; rep < 2; rep++) {
        for (int i = 0; i < 4; i++) HIP_OK(hipMemsetAsync(d_acc[i], 0xFF, acc_bytes, s));
        HIP_OK(hipMemsetAsync(d_sh, 0xFF, sh_bytes, s)); HIP_OK(hipMemsetAsync(d_out[1], 0xFF, out_bytes, s));
        HIP_OK(hipGraphLaunch(exec, s));
        HIP_OK(hipStreamSynchronize(s));
        HIP_OK(hipMemcpy(got.data(), d_out[1], out_bytes, hipMemcpyDeviceToHost));
        if (got != want) { std::fprintf(stderr, "graph replay %d differs from the direct calls\n", rep); return 1; }
    }
    std::printf("bootstrap capture ok: %zu nodes, 2 replays bit-identical to the direct calls (bits %u n %u L %u batch %u n_lwe %u w %u)\n", nodes, bits, n, L, batch, n_lwe, w);
    HIP_OK(hipGraphExecDestroy(exec)); HIP_OK(hipGraphDestroy(graph));
    for (uint32_t i = 0; i < n_lwe; i++) { FHE_OK_(fhe_relin_keys_destroy(r0[i])); FHE_OK_(fhe_relin_keys_destroy(r1[i])); }
    FHE_OK_(fhe_secret_key_destroy(sk)); FHE_OK_(fhe_rns_ntt_destroy(h));
    for (void *p : {d_s, d_tv, d_acc[0], d_acc[1], d_acc[2], d_acc[3], d_lwe, d_sh, d_out[0], d_out[1]}) HIP_OK(hipFree(p));
    HIP_OK(hipStreamDestroy(s));
    return 0;
}
