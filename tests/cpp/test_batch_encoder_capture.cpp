// test_batch_encoder_capture.cpp -- after the reserves, fhe_slots_encode -> fhe_ct_encrypt -> fhe_ct_decrypt -> fhe_slots_decode is capturable
// into ONE hipGraph (include/fhe_hip.h): the chain is run directly (and must return the slot values: a real key pair), captured on a
// caller-owned stream, and replayed twice with NEW slot values each time over outputs filled with 0xFF; every replay must return its own
// values.  Neither the engine's workspaces nor the encoder's scratch may change from the reserves on.  The process keeps the default queue
// count.  Every HIP or library error ends the program at once with a non-zero status.  Build: hipcc (needs the HIP runtime API).
// usage: test_batch_encoder_capture prime_bits n L batch   (fused or composed path: the library's choice for n and FHE_HIP_NO_FUSED_ENCODE;
// the scratch size printed tells them apart)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fhe_hip.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "HIP %s at line %d\n", hipGetErrorString(e_), __LINE__); std::exit(1); } } while (0)
#define FHE_OK_(x) do { int rc_ = (x); if (rc_ != 0) { std::fprintf(stderr, "fhe error %d (%s) at line %d\n", rc_, fhe_hip_last_error(), __LINE__); std::exit(1); } } while (0)

int main(int argc, char **argv) {
    if (argc != 5) { std::fprintf(stderr, "usage: %s prime_bits n L batch\n", argv[0]); return 2; }
    const uint32_t bits = (uint32_t)std::atoi(argv[1]), n = (uint32_t)std::atoi(argv[2]), L = (uint32_t)std::atoi(argv[3]), batch = (uint32_t)std::atoi(argv[4]);
    if (!bits || !n || L < 2 || L > 16 || !batch) { std::fprintf(stderr, "bad arguments\n"); return 2; }
    const uint64_t t = 65537; const double sigma = 3.2;
    std::vector<uint64_t> primes(L); FHE_OK_(fhe_find_ntt_primes(bits, n, L, primes.data()));
    std::vector<uint64_t> moduli((size_t)L * 4, 0); for (uint32_t l = 0; l < L; l++) moduli[(size_t)l * 4] = primes[l];
    fhe_rns_ntt_t *h = nullptr; FHE_OK_(fhe_rns_ntt_create(&h, n, (const uint64_t (*)[4])moduli.data(), L));
    hipStream_t s; HIP_OK(hipStreamCreate(&s));
    FHE_OK_(fhe_rns_ntt_set_stream(h, s));

    // a key pair without noise in the key: s ternary, pk1 = a uniform, pk0 = -(a s), so that c0 + c1 s = m + t (e0 + e1 s)
    const size_t S = (size_t)L * n * 32, vbytes = (size_t)batch * n * 8;
    uint64_t seed = 12345;
    auto next = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return seed >> 20; };
    std::vector<uint64_t> hs((size_t)L * n * 4, 0), ha(hs.size(), 0);
    for (uint32_t x = 0; x < n; x++) {
        const int v = (int)(next() % 3) - 1;
        for (uint32_t l = 0; l < L; l++) hs[((size_t)l * n + x) * 4] = v < 0 ? primes[l] - 1 : (uint64_t)v;
    }
    for (uint32_t l = 0; l < L; l++) for (uint32_t x = 0; x < n; x++) ha[((size_t)l * n + x) * 4] = next() % primes[l];
    void *d_s, *d_a, *d_pk0, *d_zero;
    for (void **p : {&d_s, &d_a, &d_pk0, &d_zero}) HIP_OK(hipMalloc(p, S));
    HIP_OK(hipMemcpy(d_s, hs.data(), S, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(d_a, ha.data(), S, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_zero, 0, S));
    FHE_OK_(fhe_rns_ntt_multiply(h, d_pk0, d_a, d_s, 1));
    FHE_OK_(fhe_rns_poly_sub(h, d_pk0, d_zero, d_pk0, 1));
    HIP_OK(hipStreamSynchronize(s));
    fhe_public_key_t *pk = nullptr; FHE_OK_(fhe_public_key_create(h, &pk, d_pk0, d_a));
    fhe_secret_key_t *sk = nullptr; FHE_OK_(fhe_secret_key_create(h, &sk, d_s));
    fhe_batch_encoder_t *enc = nullptr; FHE_OK_(fhe_batch_encoder_create(h, &enc, t, FHE_SLOTS_ROWS));

    void *d_vals, *d_pt, *d_c0, *d_c1, *d_m, *d_back;
    HIP_OK(hipMalloc(&d_vals, vbytes)); HIP_OK(hipMalloc(&d_m, vbytes)); HIP_OK(hipMalloc(&d_back, vbytes));
    for (void **p : {&d_pt, &d_c0, &d_c1}) HIP_OK(hipMalloc(p, (size_t)batch * S));
    const void *comps[2] = {d_c0, d_c1};
    const uint64_t seeds[3] = {11, 22, 33};

    FHE_OK_(fhe_rns_ntt_reserve(h, batch));
    FHE_OK_(fhe_batch_encoder_reserve(h, enc, batch));
    FHE_OK_(fhe_ct_encrypt_reserve(h, sigma, batch));
    FHE_OK_(fhe_ct_decrypt_reserve(h, t, 2, batch));
    uint64_t ws0 = 0, ws1 = 0, sc0 = 0, sc1 = 0;
    FHE_OK_(fhe_rns_ntt_workspace_bytes(h, &ws0)); FHE_OK_(fhe_batch_encoder_scratch_bytes(enc, &sc0));

    auto chain = [&]() {
        FHE_OK_(fhe_slots_encode(h, enc, d_pt, (const uint64_t *)d_vals, batch));
        FHE_OK_(fhe_ct_encrypt(h, pk, t, sigma, seeds, d_c0, d_c1, d_pt, batch));
        FHE_OK_(fhe_ct_decrypt(h, sk, t, 1, (uint64_t *)d_m, nullptr, comps, 2, batch));
        FHE_OK_(fhe_slots_decode(h, enc, (uint64_t *)d_back, (const uint64_t *)d_m, batch));
    };
    std::vector<uint64_t> vals((size_t)batch * n), got(vals.size());
    auto new_values = [&]() { for (uint64_t &v : vals) v = next() % t; HIP_OK(hipMemcpyAsync(d_vals, vals.data(), vbytes, hipMemcpyHostToDevice, s)); HIP_OK(hipStreamSynchronize(s)); };
    auto check = [&](const char *what) {
        HIP_OK(hipStreamSynchronize(s));
        HIP_OK(hipMemcpy(got.data(), d_back, vbytes, hipMemcpyDeviceToHost));
        if (got != vals) { std::fprintf(stderr, "%s does not return the slot values\n", what); std::exit(1); }
    };
    new_values();
    chain();                                                // direct
    check("the direct chain");

    hipGraph_t graph; hipGraphExec_t exec;
    HIP_OK(hipStreamBeginCapture(s, hipStreamCaptureModeGlobal));
    chain();
    HIP_OK(hipStreamEndCapture(s, &graph));
    size_t nodes = 0; HIP_OK(hipGraphGetNodes(graph, nullptr, &nodes));
    if (nodes < 4) { std::fprintf(stderr, "the captured graph has %zu nodes: four calls cannot be fewer than four\n", nodes); return 1; }
    HIP_OK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    for (int rep = 0; rep < 2; rep++) {
        new_values();
        HIP_OK(hipMemsetAsync(d_back, 0xFF, vbytes, s)); HIP_OK(hipMemsetAsync(d_m, 0xFF, vbytes, s)); HIP_OK(hipMemsetAsync(d_pt, 0xFF, (size_t)batch * S, s));
        HIP_OK(hipGraphLaunch(exec, s));
        check(rep ? "graph replay 2" : "graph replay 1");
    }
    FHE_OK_(fhe_rns_ntt_workspace_bytes(h, &ws1)); FHE_OK_(fhe_batch_encoder_scratch_bytes(enc, &sc1));
    if (ws1 != ws0 || sc1 != sc0) { std::fprintf(stderr, "memory changed after the reserves: workspaces %llu -> %llu, scratch %llu -> %llu bytes\n", (unsigned long long)ws0,
                                                 (unsigned long long)ws1, (unsigned long long)sc0, (unsigned long long)sc1); return 1; }
    std::printf("encoder capture ok: %zu nodes, scratch %llu bytes, 2 replays with new values returned them (bits %u n %u L %u batch %u)\n", nodes, (unsigned long long)sc0, bits, n, L, batch);
    HIP_OK(hipGraphExecDestroy(exec)); HIP_OK(hipGraphDestroy(graph));
    FHE_OK_(fhe_batch_encoder_destroy(enc)); FHE_OK_(fhe_secret_key_destroy(sk)); FHE_OK_(fhe_public_key_destroy(pk)); FHE_OK_(fhe_rns_ntt_destroy(h));
    for (void *p : {d_s, d_a, d_pk0, d_zero, d_vals, d_pt, d_c0, d_c1, d_m, d_back}) HIP_OK(hipFree(p));
    HIP_OK(hipStreamDestroy(s));
    return 0;
}
