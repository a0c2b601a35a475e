// bench_encode_mirror.cpp -- wall time of the C++ mirror's host encode / decode (FHEContext::encode / decode: the host transform over Z_t, the
// expansion into L limbs of 32-byte containers and the upload / download, include/fhe/fhe.hpp) against encode_fused / decode_fused (upload of
// n 8-byte words, one fhe_slots_encode / fhe_slots_decode_poly), one plaintext per call, the four alternating, best of `reps`.  Built and run
// by scripts/bench_encode.py.  usage: bench_encode_mirror n prime_bits L reps  -> one JSON object on stdout
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fhe/fhe.hpp"

using namespace fhe;

int main(int argc, char **argv) {
    if (argc != 5) { std::fprintf(stderr, "usage: %s n prime_bits L reps\n", argv[0]); return 2; }
    const uint32_t n = (uint32_t)std::atoi(argv[1]), bits = (uint32_t)std::atoi(argv[2]), L = (uint32_t)std::atoi(argv[3]);
    const int reps = std::atoi(argv[4]);
    std::vector<uint64_t> primes(L);
    check(fhe_find_ntt_primes(bits, n, L, primes.data()), "prime search");
    std::vector<uint256_t> moduli;
    for (uint64_t p : primes) moduli.emplace_back(p);
    FHEContext ctx(SecurityParams{128, n, bits * L, 3.2f, 64}, moduli);
    const uint64_t t = ctx.params().t;
    std::vector<uint64_t> v(n), out;
    for (uint32_t i = 0; i < n; i++) v[i] = (1234567ull * i + 89) % t;
    Plaintext a, b;
    ctx.encode(a, v); ctx.encode_fused(b, v); ctx.decode(out, a); ctx.decode_fused(out, b);   // warm-up: encoder, code objects
    double best[4] = {1e30, 1e30, 1e30, 1e30};
    for (int r = 0; r < reps; r++)
        for (int k = 0; k < 4; k++) {
            const auto t0 = std::chrono::steady_clock::now();
            if (k == 0) ctx.encode(a, v); else if (k == 1) ctx.encode_fused(b, v); else if (k == 2) ctx.decode(out, a); else ctx.decode_fused(out, b);
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
            if (us < best[k]) best[k] = us;
        }
    if (out != v) { std::fprintf(stderr, "decode_fused does not return the values\n"); return 1; }
    std::printf("{\"mirror_host_encode_us\": %.1f, \"mirror_encode_fused_us\": %.1f, \"mirror_host_decode_us\": %.1f, \"mirror_decode_fused_us\": %.1f}\n", best[0], best[1], best[2], best[3]);
    delete a.poly; delete b.poly;
    return 0;
}
