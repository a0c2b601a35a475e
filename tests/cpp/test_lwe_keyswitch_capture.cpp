// test_lwe_keyswitch_capture.cpp -- the whole chainable bootstrap, fhe_lwe_prepare_accumulator -> fhe_blind_rotate -> fhe_rns_rescale_drop_last
// of both accumulators to one prime -> fhe_rlwe_sample_extract on the one-limb engine -> fhe_lwe_keyswitch, is capturable into a hipGraph after
// the reserves (include/fhe_hip.h): captured once on a caller-owned stream and replayed twice over fresh LWE inputs, with every intermediate
// buffer filled with 0xFF first, it gives the directly launched LWE ciphertexts bit for bit, and fhe_rns_ntt_workspace_bytes does not change
// across the key switch.  Every HIP or library error ends the program at once with a non-zero status.  Build: hipcc.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fhe_hip.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "HIP %s at line %d\n", hipGetErrorString(e_), __LINE__); std::exit(1); } } while (0)
#define FHE_OK_(x) do { int rc_ = (x); if (rc_ != 0) { std::fprintf(stderr, "fhe error %d (%s) at line %d\n", rc_, fhe_hip_last_error(), __LINE__); std::exit(1); } } while (0)

// usage: test_lwe_keyswitch_capture prime_bits n batch n_lwe rgsw_bits ks_bits q_out      (two primes; q_out 0 keeps the modulus)
int main(int argc, char **argv) {
    if (argc != 8) { std::fprintf(stderr, "usage: %s prime_bits n batch n_lwe rgsw_bits ks_bits q_out\n", argv[0]); return 2; }
    const uint32_t bits = (uint32_t)std::atoi(argv[1]), n = (uint32_t)std::atoi(argv[2]), batch = (uint32_t)std::atoi(argv[3]),
                   n_lwe = (uint32_t)std::atoi(argv[4]), w = (uint32_t)std::atoi(argv[5]), w_ks = (uint32_t)std::atoi(argv[6]), L = 2;
    const uint64_t q_out = std::strtoull(argv[7], nullptr, 10);
    if (!bits || !n || !batch || !n_lwe || n_lwe > 64 || !w || !w_ks) { std::fprintf(stderr, "bad arguments\n"); return 2; }
    const uint64_t q_lwe = 1ull << 32, seeds[2] = {11, 12}, ks_seeds[2] = {13, 14};
    std::vector<uint64_t> primes(L); FHE_OK_(fhe_find_ntt_primes(bits, n, L, primes.data()));
    std::vector<uint64_t> moduli((size_t)L * 4, 0); for (uint32_t l = 0; l < L; l++) moduli[(size_t)l * 4] = primes[l];
    fhe_rns_ntt_t *h = nullptr, *h1 = nullptr;
    FHE_OK_(fhe_rns_ntt_create(&h, n, (const uint64_t (*)[4])moduli.data(), L));
    FHE_OK_(fhe_rns_ntt_create(&h1, n, (const uint64_t (*)[4])moduli.data(), 1));
    hipStream_t s; HIP_OK(hipStreamCreate(&s));
    FHE_OK_(fhe_rns_ntt_set_stream(h, s)); FHE_OK_(fhe_rns_ntt_set_stream(h1, s));

    const size_t poly = (size_t)L * n * 4, S = poly * 8, acc_bytes = (size_t)batch * S, low_bytes = (size_t)batch * n * 32;   // u64 words, bytes
    const size_t ext_bytes = (size_t)batch * (n + 1) * 8, sh_bytes = (size_t)n_lwe * batch * 4, lwe_bytes = (size_t)batch * (n_lwe + 1) * 8;
    uint64_t seed = 1000;
    auto next = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return seed >> 20; };
    std::vector<uint64_t> host(poly, 0), lwe((size_t)batch * (n_lwe + 1));
    void *d_s, *d_tv, *d_acc[4], *d_low[2], *d_lwe, *d_sh, *d_ext, *d_out[2];
    for (uint32_t x = 0; x < n; x++) { const uint64_t r = next() % 3; for (uint32_t l = 0; l < L; l++) host[((size_t)l * n + x) * 4] = r == 2 ? primes[l] - 1 : r; }
    HIP_OK(hipMalloc(&d_s, S)); HIP_OK(hipMemcpy(d_s, host.data(), S, hipMemcpyHostToDevice));
    for (uint32_t l = 0; l < L; l++) for (uint32_t x = 0; x < n; x++) host[((size_t)l * n + x) * 4] = next() % primes[l];
    HIP_OK(hipMalloc(&d_tv, S)); HIP_OK(hipMemcpy(d_tv, host.data(), S, hipMemcpyHostToDevice));
    HIP_OK(hipMalloc(&d_lwe, lwe_bytes));
    for (int i = 0; i < 4; i++) HIP_OK(hipMalloc(&d_acc[i], acc_bytes));
    for (int i = 0; i < 2; i++) HIP_OK(hipMalloc(&d_low[i], low_bytes));
    HIP_OK(hipMalloc(&d_sh, sh_bytes)); HIP_OK(hipMalloc(&d_ext, ext_bytes));
    for (int i = 0; i < 2; i++) HIP_OK(hipMalloc(&d_out[i], lwe_bytes));

    fhe_secret_key_t *sk = nullptr; FHE_OK_(fhe_secret_key_create(h, &sk, d_s));
    std::vector<int32_t> z(n_lwe); for (uint32_t i = 0; i < n_lwe; i++) z[i] = (int32_t)(next() & 1);
    std::vector<fhe_relin_keys_t *> r0(n_lwe, nullptr), r1(n_lwe, nullptr);
    FHE_OK_(fhe_rgsw_keys_generate(h, sk, w, z.data(), n_lwe, 1, 3.2, seeds, r0.data(), r1.data()));
    fhe_lwe_ksk_t *ksk = nullptr; FHE_OK_(fhe_lwe_ksk_generate(h, sk, w_ks, n_lwe, z.data(), 1, 3.2, ks_seeds, &ksk));
    FHE_OK_(fhe_rns_ntt_reserve(h, batch)); FHE_OK_(fhe_rns_ntt_reserve(h1, batch));

    auto fresh_inputs = [&]() {
        for (uint64_t &v : lwe) v = next() % q_lwe;
        HIP_OK(hipMemcpy(d_lwe, lwe.data(), lwe_bytes, hipMemcpyHostToDevice));
    };
    uint64_t ws[4] = {0, 0, 0, 0};
    auto sequence = [&](void *out, bool measure) {
        FHE_OK_(fhe_lwe_prepare_accumulator(h, q_lwe, n_lwe, (const uint64_t *)d_lwe, d_tv, d_acc[0], d_acc[1], (uint32_t *)d_sh, batch));
        FHE_OK_(fhe_blind_rotate(h, r0.data(), r1.data(), n_lwe, d_acc[0], d_acc[1], (const uint32_t *)d_sh, d_acc[2], d_acc[3], batch));
        FHE_OK_(fhe_rns_rescale_drop_last(h, d_low[0], d_acc[0], batch));
        FHE_OK_(fhe_rns_rescale_drop_last(h, d_low[1], d_acc[1], batch));
        FHE_OK_(fhe_rlwe_sample_extract(h1, (uint64_t *)d_ext, d_low[0], d_low[1], 0, batch));
        if (measure) { FHE_OK_(fhe_rns_ntt_workspace_bytes(h, &ws[0])); FHE_OK_(fhe_rns_ntt_workspace_bytes(h1, &ws[1])); }
        FHE_OK_(fhe_lwe_keyswitch(h1, ksk, q_out, (uint64_t *)out, (const uint64_t *)d_ext, batch));
        if (measure) { FHE_OK_(fhe_rns_ntt_workspace_bytes(h, &ws[2])); FHE_OK_(fhe_rns_ntt_workspace_bytes(h1, &ws[3])); }
    };
    fresh_inputs();
    sequence(d_out[0], true);                       // first use builds the rescale table: before the capture
    HIP_OK(hipStreamSynchronize(s));
    if (ws[0] != ws[2] || ws[1] != ws[3]) { std::fprintf(stderr, "the workspace changed across the key switch\n"); return 1; }

    hipGraph_t graph; hipGraphExec_t exec;
    HIP_OK(hipStreamBeginCapture(s, hipStreamCaptureModeGlobal));
    sequence(d_out[1], false);
    HIP_OK(hipStreamEndCapture(s, &graph));
    size_t nodes = 0; HIP_OK(hipGraphGetNodes(graph, nullptr, &nodes));
    if (nodes < (size_t)n_lwe + 5) { std::fprintf(stderr, "the captured graph has %zu nodes, fewer than prepare + %u steps + 2 rescales + extract + key switch\n", nodes, n_lwe); return 1; }
    HIP_OK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    const uint64_t bound = q_out ? q_out : primes[0];
    std::vector<uint64_t> want(lwe_bytes / 8), got(lwe_bytes / 8);
    for (int rep = 0; rep < 2; rep++) {
        fresh_inputs();                                                       // new LWE ciphertexts for every replay
        sequence(d_out[0], false);
        HIP_OK(hipStreamSynchronize(s));
        HIP_OK(hipMemcpy(want.data(), d_out[0], lwe_bytes, hipMemcpyDeviceToHost));
        for (uint64_t v : want) if (v >= bound) { std::fprintf(stderr, "a value of the direct call is not below the output modulus\n"); return 1; }
        for (int i = 0; i < 4; i++) HIP_OK(hipMemsetAsync(d_acc[i], 0xFF, acc_bytes, s));
        for (int i = 0; i < 2; i++) HIP_OK(hipMemsetAsync(d_low[i], 0xFF, low_bytes, s));
        HIP_OK(hipMemsetAsync(d_sh, 0xFF, sh_bytes, s)); HIP_OK(hipMemsetAsync(d_ext, 0xFF, ext_bytes, s)); HIP_OK(hipMemsetAsync(d_out[1], 0xFF, lwe_bytes, s));
        HIP_OK(hipGraphLaunch(exec, s));
        HIP_OK(hipStreamSynchronize(s));
        HIP_OK(hipMemcpy(got.data(), d_out[1], lwe_bytes, hipMemcpyDeviceToHost));
        if (got != want) { std::fprintf(stderr, "graph replay %d differs from the direct calls\n", rep); return 1; }
    }
    std::printf("lwe keyswitch capture ok: %zu nodes, 2 replays over fresh inputs bit-identical to the direct calls (bits %u n %u batch %u n_lwe %u w %u ks_w %u q_out %llu)\n",
                nodes, bits, n, batch, n_lwe, w, w_ks, (unsigned long long)q_out);
    HIP_OK(hipGraphExecDestroy(exec)); HIP_OK(hipGraphDestroy(graph));
    for (uint32_t i = 0; i < n_lwe; i++) { FHE_OK_(fhe_relin_keys_destroy(r0[i])); FHE_OK_(fhe_relin_keys_destroy(r1[i])); }
    FHE_OK_(fhe_lwe_ksk_destroy(ksk)); FHE_OK_(fhe_secret_key_destroy(sk)); FHE_OK_(fhe_rns_ntt_destroy(h)); FHE_OK_(fhe_rns_ntt_destroy(h1));
    for (void *p : {d_s, d_tv, d_acc[0], d_acc[1], d_acc[2], d_acc[3], d_low[0], d_low[1], d_lwe, d_sh, d_ext, d_out[0], d_out[1]}) HIP_OK(hipFree(p));
    HIP_OK(hipStreamDestroy(s));
    return 0;
}
