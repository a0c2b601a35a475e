// test_encrypt_capture.cpp -- after fhe_ct_encrypt_reserve a fhe_ct_encrypt call is capturable into a hipGraph (include/fhe_hip.h): one call
// captured on a caller-owned stream, replayed over outputs filled with 0xFF, and compared with the directly launched result.  Every HIP or
// library error ends the program at once with a non-zero status.  Build: hipcc (needs the HIP runtime API).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fhe_hip.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "HIP %s at line %d\n", hipGetErrorString(e_), __LINE__); std::exit(1); } } while (0)
#define FHE_OK_(x) do { int rc_ = (x); if (rc_ != 0) { std::fprintf(stderr, "fhe error %d (%s) at line %d\n", rc_, fhe_hip_last_error(), __LINE__); std::exit(1); } } while (0)

// usage: test_encrypt_capture prime_bits n L batch   (the path -- one launch or the composition -- is the library's choice for the shape and
// for FHE_HIP_NO_FUSED_ENCRYPT; the node count printed tells them apart)
int main(int argc, char **argv) {
    if (argc != 5) { std::fprintf(stderr, "usage: %s prime_bits n L batch\n", argv[0]); return 2; }
    const uint32_t bits = (uint32_t)std::atoi(argv[1]), n = (uint32_t)std::atoi(argv[2]), L = (uint32_t)std::atoi(argv[3]), batch = (uint32_t)std::atoi(argv[4]);
    if (!bits || !n || !L || L > 16 || !batch) { std::fprintf(stderr, "bad arguments\n"); return 2; }
    const uint64_t t = 65537; const double sigma = 3.2;
    const uint64_t seeds[3] = {0x1234567ull, 0x89ABCDEF01ull, 0xFEDCBA9876543ull};
    std::vector<uint64_t> primes(L); FHE_OK_(fhe_find_ntt_primes(bits, n, L, primes.data()));
    std::vector<uint64_t> moduli((size_t)L * 4, 0); for (uint32_t l = 0; l < L; l++) moduli[(size_t)l * 4] = primes[l];
    fhe_rns_ntt_t *h = nullptr; FHE_OK_(fhe_rns_ntt_create(&h, n, (const uint64_t (*)[4])moduli.data(), L));
    hipStream_t s; HIP_OK(hipStreamCreate(&s));
    FHE_OK_(fhe_rns_ntt_set_stream(h, s));

    const size_t poly = (size_t)L * n * 4, key_bytes = poly * 8, bytes = (size_t)batch * key_bytes;      // u64 words
    std::vector<uint64_t> host((size_t)batch * poly, 0);
    auto fill = [&](uint64_t seed, uint32_t count) { for (uint32_t b = 0; b < count; b++) for (uint32_t l = 0; l < L; l++) for (uint32_t x = 0; x < n; x++) {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull; host[((size_t)(b * L + l) * n + x) * 4] = (seed >> 20) % primes[l]; } };
    void *d_pk[2], *d_m, *out[2], *ref[2];
    for (int i = 0; i < 2; i++) { HIP_OK(hipMalloc(&d_pk[i], key_bytes)); fill(1000 + i, 1); HIP_OK(hipMemcpy(d_pk[i], host.data(), key_bytes, hipMemcpyHostToDevice)); }
    HIP_OK(hipMalloc(&d_m, bytes)); fill(2000, batch); HIP_OK(hipMemcpy(d_m, host.data(), bytes, hipMemcpyHostToDevice));
    for (int i = 0; i < 2; i++) { HIP_OK(hipMalloc(&out[i], bytes)); HIP_OK(hipMalloc(&ref[i], bytes)); }
    fhe_public_key_t *pk = nullptr; FHE_OK_(fhe_public_key_create(h, &pk, d_pk[0], d_pk[1]));
    FHE_OK_(fhe_ct_encrypt_reserve(h, sigma, batch));
    uint64_t ws_before = 0, ws_after = 0; FHE_OK_(fhe_rns_ntt_workspace_bytes(h, &ws_before));

    // reference result by a direct call
    FHE_OK_(fhe_ct_encrypt(h, pk, t, sigma, seeds, ref[0], ref[1], d_m, batch));
    HIP_OK(hipStreamSynchronize(s));
    std::vector<uint64_t> want[2] = {std::vector<uint64_t>(host.size()), std::vector<uint64_t>(host.size())}, got(host.size());
    for (int i = 0; i < 2; i++) HIP_OK(hipMemcpy(want[i].data(), ref[i], bytes, hipMemcpyDeviceToHost));

    // capture the same call
    hipGraph_t graph; hipGraphExec_t exec;
    HIP_OK(hipStreamBeginCapture(s, hipStreamCaptureModeGlobal));
    FHE_OK_(fhe_ct_encrypt(h, pk, t, sigma, seeds, out[0], out[1], d_m, batch));
    HIP_OK(hipStreamEndCapture(s, &graph));
    size_t nodes = 0; HIP_OK(hipGraphGetNodes(graph, nullptr, &nodes));
    HIP_OK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    FHE_OK_(fhe_rns_ntt_workspace_bytes(h, &ws_after));
    if (ws_after != ws_before) { std::fprintf(stderr, "the workspace changed across the calls after the reserve: %llu -> %llu bytes\n", (unsigned long long)ws_before, (unsigned long long)ws_after); return 1; }
    for (int rep = 0; rep < 3; rep++) {
        for (int i = 0; i < 2; i++) HIP_OK(hipMemsetAsync(out[i], 0xFF, bytes, s));
        HIP_OK(hipGraphLaunch(exec, s));
        HIP_OK(hipStreamSynchronize(s));
        for (int i = 0; i < 2; i++) {
            HIP_OK(hipMemcpy(got.data(), out[i], bytes, hipMemcpyDeviceToHost));
            if (std::memcmp(got.data(), want[i].data(), bytes) != 0) { std::fprintf(stderr, "graph replay %d differs from the direct call (component %d)\n", rep, i); return 1; }
        }
    }
    std::printf("encrypt capture ok: %zu nodes, 3 replays bit-identical to the direct call (bits %u n %u L %u batch %u)\n", nodes, bits, n, L, batch);
    HIP_OK(hipGraphExecDestroy(exec)); HIP_OK(hipGraphDestroy(graph));
    FHE_OK_(fhe_public_key_destroy(pk)); FHE_OK_(fhe_rns_ntt_destroy(h));
    for (void *p : {d_pk[0], d_pk[1], d_m, out[0], out[1], ref[0], ref[1]}) HIP_OK(hipFree(p));
    HIP_OK(hipStreamDestroy(s));
    return 0;
}
