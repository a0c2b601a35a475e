// test_bfv_capture.cpp -- after fhe_bfv_multiplier_reserve(m, batch, rk), fhe_bfv_multiply_relin is capturable into ONE hipGraph
// (include/fhe_hip.h): the call is run directly, captured on a caller-owned stream, and replayed twice over outputs filled with 0xFF; every
// replay must give the direct call's bits.  Neither the multiplier's workspaces nor the ciphertext engine's may change from the reserve on.
// The process keeps the default queue count.  Every HIP or library error ends the program at once with a non-zero status.
// Build: hipcc (needs the HIP runtime API).   usage: test_bfv_capture prime_bits n L L' batch
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fhe_hip.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "HIP %s at line %d\n", hipGetErrorString(e_), __LINE__); std::exit(1); } } while (0)
#define FHE_OK_(x) do { int rc_ = (x); if (rc_ != 0) { std::fprintf(stderr, "fhe error %d (%s) at line %d\n", rc_, fhe_hip_last_error(), __LINE__); std::exit(1); } } while (0)

int main(int argc, char **argv) {
    if (argc != 6) { std::fprintf(stderr, "usage: %s prime_bits n L L' batch\n", argv[0]); return 2; }
    const uint32_t bits = (uint32_t)std::atoi(argv[1]), n = (uint32_t)std::atoi(argv[2]), L = (uint32_t)std::atoi(argv[3]), Lp = (uint32_t)std::atoi(argv[4]),
                   batch = (uint32_t)std::atoi(argv[5]);
    if (!bits || !n || !L || L > 16 || !Lp || Lp > 16 || !batch) { std::fprintf(stderr, "bad arguments\n"); return 2; }
    const uint64_t t = 65537;
    std::vector<uint64_t> primes(L + Lp); FHE_OK_(fhe_find_ntt_primes(bits, n, L + Lp, primes.data()));
    std::vector<uint64_t> moduli((size_t)L * 4, 0); for (uint32_t l = 0; l < L; l++) moduli[(size_t)l * 4] = primes[l];
    fhe_rns_ntt_t *h = nullptr; FHE_OK_(fhe_rns_ntt_create(&h, n, (const uint64_t (*)[4])moduli.data(), L));
    hipStream_t s; HIP_OK(hipStreamCreate(&s));
    FHE_OK_(fhe_rns_ntt_set_stream(h, s));
    fhe_bfv_multiplier_t *m = nullptr; FHE_OK_(fhe_bfv_multiplier_create(h, &m, t, primes.data() + L, Lp));

    const size_t S = (size_t)L * n * 32;
    uint64_t seed = 4321;
    auto next = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return seed >> 16; };
    std::vector<uint64_t> hs((size_t)L * n * 4, 0);
    for (uint32_t x = 0; x < n; x++) {
        const int v = (int)(next() % 3) - 1;
        for (uint32_t l = 0; l < L; l++) hs[((size_t)l * n + x) * 4] = v < 0 ? primes[l] - 1 : (uint64_t)v;
    }
    void *d_s; HIP_OK(hipMalloc(&d_s, S)); HIP_OK(hipMemcpy(d_s, hs.data(), S, hipMemcpyHostToDevice));
    fhe_secret_key_t *sk = nullptr; FHE_OK_(fhe_secret_key_create(h, &sk, d_s));
    const uint32_t elts[1] = {0}; const uint64_t key_seeds[2] = {7, 8};
    fhe_relin_keys_t *rk = nullptr; FHE_OK_(fhe_keyswitch_keys_generate(h, sk, 16, elts, 1, 1, 3.2, key_seeds, &rk));

    void *d_in[4], *d_c0, *d_c1;
    std::vector<uint64_t> hin((size_t)batch * L * n * 4, 0);
    for (int i = 0; i < 4; i++) {
        for (uint32_t b = 0; b < batch; b++) for (uint32_t l = 0; l < L; l++) for (uint32_t x = 0; x < n; x++) hin[(((size_t)b * L + l) * n + x) * 4] = next() % primes[l];
        HIP_OK(hipMalloc(&d_in[i], batch * S)); HIP_OK(hipMemcpy(d_in[i], hin.data(), batch * S, hipMemcpyHostToDevice));
    }
    HIP_OK(hipMalloc(&d_c0, batch * S)); HIP_OK(hipMalloc(&d_c1, batch * S));

    FHE_OK_(fhe_bfv_multiplier_reserve(m, batch, rk));
    uint64_t mw0 = 0, mw1 = 0, ew0 = 0, ew1 = 0;
    FHE_OK_(fhe_bfv_multiplier_workspace_bytes(m, &mw0)); FHE_OK_(fhe_rns_ntt_workspace_bytes(h, &ew0));
    if (!mw0) { std::fprintf(stderr, "the reserve sized no workspace\n"); return 1; }

    auto call = [&]() { FHE_OK_(fhe_bfv_multiply_relin(m, rk, d_c0, d_c1, d_in[0], d_in[1], d_in[2], d_in[3], batch)); };
    std::vector<uint64_t> want0(hin.size()), want1(hin.size()), got(hin.size());
    call();                                                 // direct
    HIP_OK(hipStreamSynchronize(s));
    HIP_OK(hipMemcpy(want0.data(), d_c0, batch * S, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(want1.data(), d_c1, batch * S, hipMemcpyDeviceToHost));

    hipGraph_t graph; hipGraphExec_t exec;
    HIP_OK(hipStreamBeginCapture(s, hipStreamCaptureModeGlobal));
    call();
    HIP_OK(hipStreamEndCapture(s, &graph));
    size_t nodes = 0; HIP_OK(hipGraphGetNodes(graph, nullptr, &nodes));
    if (nodes < 4) { std::fprintf(stderr, "the captured graph has %zu nodes: lift, tensor product, scale-and-round and key switch cannot be fewer than four\n", nodes); return 1; }
    HIP_OK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    for (int rep = 0; rep < 2; rep++) {
        HIP_OK(hipMemsetAsync(d_c0, 0xFF, batch * S, s)); HIP_OK(hipMemsetAsync(d_c1, 0xFF, batch * S, s));
        HIP_OK(hipGraphLaunch(exec, s));
        HIP_OK(hipStreamSynchronize(s));
        HIP_OK(hipMemcpy(got.data(), d_c0, batch * S, hipMemcpyDeviceToHost));
        if (got != want0) { std::fprintf(stderr, "graph replay %d: c0 differs from the direct call\n", rep + 1); return 1; }
        HIP_OK(hipMemcpy(got.data(), d_c1, batch * S, hipMemcpyDeviceToHost));
        if (got != want1) { std::fprintf(stderr, "graph replay %d: c1 differs from the direct call\n", rep + 1); return 1; }
    }
    FHE_OK_(fhe_bfv_multiplier_workspace_bytes(m, &mw1)); FHE_OK_(fhe_rns_ntt_workspace_bytes(h, &ew1));
    if (mw1 != mw0 || ew1 != ew0) { std::fprintf(stderr, "memory changed after the reserve: multiplier %llu -> %llu, engine %llu -> %llu bytes\n", (unsigned long long)mw0,
                                                 (unsigned long long)mw1, (unsigned long long)ew0, (unsigned long long)ew1); return 1; }
    std::printf("bfv capture ok: %zu nodes, workspace %llu bytes, 2 replays gave the direct call's bits (bits %u n %u L %u L' %u batch %u)\n", nodes,
                (unsigned long long)mw0, bits, n, L, Lp, batch);
    HIP_OK(hipGraphExecDestroy(exec)); HIP_OK(hipGraphDestroy(graph));
    FHE_OK_(fhe_bfv_multiplier_destroy(m)); FHE_OK_(fhe_relin_keys_destroy(rk)); FHE_OK_(fhe_secret_key_destroy(sk)); FHE_OK_(fhe_rns_ntt_destroy(h));
    for (void *p : {d_s, d_in[0], d_in[1], d_in[2], d_in[3], d_c0, d_c1}) HIP_OK(hipFree(p));
    HIP_OK(hipStreamDestroy(s));
    return 0;
}
