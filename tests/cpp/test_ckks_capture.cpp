// test_ckks_capture.cpp -- fhe_ckks_encode -> fhe_ckks_decode_poly, and fhe_ckks_decode of words, are capturable into ONE hipGraph
// (include/fhe_hip.h): the calls run directly, are captured on a caller-owned stream and replayed twice with NEW slots each time over outputs
// filled with 0xFF; every replay must return the direct result for its inputs bit for bit (the result depends on the inputs only) and the
// slots themselves within the rounding of the coefficients.  The engine's workspace byte count may not change across the calls.  Every HIP
// or library error ends the program at once with a non-zero status.  Build: hipcc (needs the HIP runtime API).
// usage: test_ckks_capture prime_bits n L batch
#include <hip/hip_runtime.h>

#include <cmath>
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
    if (!bits || !n || !L || L > 16 || !batch) { std::fprintf(stderr, "bad arguments\n"); return 2; }
    const double scale = std::ldexp(1.0, (int)bits - 4);            // slots in the unit square: |c| < q_0 / 2
    std::vector<uint64_t> primes(L); FHE_OK_(fhe_find_ntt_primes(bits, n, L, primes.data()));
    std::vector<uint64_t> moduli((size_t)L * 4, 0); for (uint32_t l = 0; l < L; l++) moduli[(size_t)l * 4] = primes[l];
    fhe_rns_ntt_t *h = nullptr; FHE_OK_(fhe_rns_ntt_create(&h, n, (const uint64_t (*)[4])moduli.data(), L));
    hipStream_t s; HIP_OK(hipStreamCreate(&s));
    FHE_OK_(fhe_rns_ntt_set_stream(h, s));
    fhe_ckks_encoder_t *enc = nullptr; FHE_OK_(fhe_ckks_encoder_create(h, &enc));

    const size_t S = (size_t)L * n * 32, zbytes = (size_t)batch * n * 8;
    void *d_z, *d_pt, *d_back, *d_words, *d_back2, *d_bits;
    for (void **p : {&d_z, &d_back, &d_words, &d_back2}) HIP_OK(hipMalloc(p, zbytes));
    HIP_OK(hipMalloc(&d_pt, (size_t)batch * S)); HIP_OK(hipMalloc(&d_bits, (size_t)batch * 4));
    FHE_OK_(fhe_rns_ntt_reserve(h, batch));
    uint64_t ws0 = 0, ws1 = 0;
    FHE_OK_(fhe_rns_ntt_workspace_bytes(h, &ws0));

    uint64_t seed = 777;
    auto next = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return seed >> 11; };
    std::vector<double> z((size_t)batch * n), back(z.size()), back2(z.size()), ref(z.size()), ref2(z.size());
    std::vector<uint64_t> words((size_t)batch * n);
    std::vector<uint32_t> cbits(batch), cref(batch);
    auto chain = [&]() {
        FHE_OK_(fhe_ckks_encode(h, enc, d_pt, (uint32_t *)d_bits, (const double *)d_z, scale, batch));
        FHE_OK_(fhe_ckks_decode_poly(h, enc, (double *)d_back, d_pt, scale, batch));
        FHE_OK_(fhe_ckks_decode(h, enc, (double *)d_back2, (const uint64_t *)d_words, 1ull << 63, scale, batch));
    };
    auto new_values = [&]() {
        for (double &v : z) v = (double)next() / 9007199254740992.0;
        for (uint64_t &w : words) w = (next() & 0xFFFFFF) ^ ((next() & 1) ? 0 : 0x7FFFFFFFFF000000ull);   // small positive, or close below 2^63: negative
        HIP_OK(hipMemcpyAsync(d_z, z.data(), zbytes, hipMemcpyHostToDevice, s)); HIP_OK(hipMemcpyAsync(d_words, words.data(), zbytes, hipMemcpyHostToDevice, s));
        HIP_OK(hipStreamSynchronize(s));
    };
    auto fetch = [&](std::vector<double> &a, std::vector<double> &b, std::vector<uint32_t> &c) {
        HIP_OK(hipStreamSynchronize(s));
        HIP_OK(hipMemcpy(a.data(), d_back, zbytes, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(b.data(), d_back2, zbytes, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(c.data(), d_bits, (size_t)batch * 4, hipMemcpyDeviceToHost));
    };
    auto poison = [&]() {
        HIP_OK(hipMemsetAsync(d_back, 0xFF, zbytes, s)); HIP_OK(hipMemsetAsync(d_back2, 0xFF, zbytes, s)); HIP_OK(hipMemsetAsync(d_pt, 0xFF, (size_t)batch * S, s));
        HIP_OK(hipMemsetAsync(d_bits, 0xFF, (size_t)batch * 4, s));
    };
    const double tol = (n / 2 + 1) / scale + 1e-9;
    auto near_slots = [&](const std::vector<double> &a, const char *what) {
        for (size_t i = 0; i < a.size(); i++)
            if (!(std::fabs(a[i] - z[i]) <= tol)) { std::fprintf(stderr, "%s does not return the slots: %g against %g at %zu\n", what, a[i], z[i], i); std::exit(1); }
    };
    new_values(); poison(); chain(); fetch(ref, ref2, cref);          // direct
    near_slots(ref, "the direct chain");

    hipGraph_t graph; hipGraphExec_t exec;
    HIP_OK(hipStreamBeginCapture(s, hipStreamCaptureModeGlobal));
    chain();
    HIP_OK(hipStreamEndCapture(s, &graph));
    size_t nodes = 0; HIP_OK(hipGraphGetNodes(graph, nullptr, &nodes));
    if (nodes != 3) { std::fprintf(stderr, "the captured graph has %zu nodes: three calls are three launches\n", nodes); return 1; }
    HIP_OK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    for (int rep = 0; rep < 2; rep++) {
        new_values();
        poison(); chain(); fetch(ref, ref2, cref);                  // what a direct call gives for these inputs
        poison();
        HIP_OK(hipGraphLaunch(exec, s));
        fetch(back, back2, cbits);
        near_slots(back, rep ? "graph replay 2" : "graph replay 1");
        if (std::memcmp(back.data(), ref.data(), zbytes) || std::memcmp(back2.data(), ref2.data(), zbytes) || cbits != cref) {
            std::fprintf(stderr, "graph replay %d differs from the direct call on the same inputs\n", rep + 1); return 1;
        }
    }
    FHE_OK_(fhe_rns_ntt_workspace_bytes(h, &ws1));
    if (ws1 != ws0) { std::fprintf(stderr, "workspaces changed: %llu -> %llu bytes\n", (unsigned long long)ws0, (unsigned long long)ws1); return 1; }
    std::printf("ckks capture ok: %zu nodes, workspace %llu bytes unchanged, 2 replays with new slots (bits %u n %u L %u batch %u)\n", nodes, (unsigned long long)ws0, bits, n, L, batch);
    HIP_OK(hipGraphExecDestroy(exec)); HIP_OK(hipGraphDestroy(graph));
    FHE_OK_(fhe_ckks_encoder_destroy(enc)); FHE_OK_(fhe_rns_ntt_destroy(h));
    for (void *p : {d_z, d_pt, d_back, d_words, d_back2, d_bits}) HIP_OK(hipFree(p));
    HIP_OK(hipStreamDestroy(s));
    return 0;
}
