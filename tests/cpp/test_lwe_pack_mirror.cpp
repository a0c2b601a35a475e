// test_lwe_pack_mirror.cpp -- FHEContext::packing_key_gen / pack_lwes (include/fhe/fhe.hpp: fhe_keyswitch_keys_generate for the elements 2^j + 1,
// fhe_lwe_pack) with decrypt_fused: a ciphertext of a known plaintext, eight of its coefficients extracted with fhe_rlwe_sample_extract, packed
// back with the trace, decrypts to exactly those eight coefficients and zeros elsewhere -- with normalisation (correction 1) and without it
// (correction n mod t, divided out by decrypt_fused).  n = 2048, 2 x 30-bit primes, t = 65537, w = 16.  Foreign keys are refused.
//   ./test_lwe_pack_mirror              the scenario on the GPU
//   ./test_lwe_pack_mirror --host-only  links and checks the new entry points' null-handle rejection (no device)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <vector>

#include "fhe/fhe.hpp"

using namespace fhe;

#define REQUIRE(cond)                                                                       \
    do {                                                                                    \
        if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static void test_host() {
    uint32_t elts[11];
    REQUIRE(fhe_lwe_pack_galois_elements(2048, elts) == FHE_OK);
    for (uint32_t j = 1; j <= 11; j++) REQUIRE(elts[j - 1] == (1u << j) + 1);
    REQUIRE(fhe_lwe_pack_galois_elements(2047, elts) == FHE_ERR_INVALID_ARG && fhe_lwe_pack_galois_elements(4, elts) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_lwe_pack_galois_elements(2048, nullptr) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_lwe_to_rlwe(nullptr, nullptr, nullptr, nullptr, 1) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_lwe_pack(nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, 1, 1) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_lwe_pack_reserve(nullptr, nullptr, 1, 1, 1) == FHE_ERR_INVALID_ARG);
    PackingKeys empty;
    REQUIRE(empty.sets.empty() && empty.made_for == nullptr && empty.decomp_bits == 16);
}

// limb 0 of a plaintext polynomial as integers
static std::vector<uint64_t> limb0(const Polynomial &p, uint32_t n) {
    std::vector<uint256_t> host(n);
    check(fhe_hip_sync(), "sync");
    check(fhe_hip_memcpy_d2h(host.data(), p.coeffs, (size_t)n * sizeof(uint256_t)), "memcpy d2h");
    std::vector<uint64_t> v(n);
    for (uint32_t i = 0; i < n; i++) v[i] = host[i].limbs[0];
    return v;
}

int main(int argc, char **argv) {
    test_host();
    if (argc > 1 && !std::strcmp(argv[1], "--host-only")) { std::cout << "host-only: PASSED" << std::endl; return 0; }
    int devices = 0;
    check(fhe_hip_device_count(&devices), "device count");
    REQUIRE(devices > 0);
    std::cout << "Testing packing_key_gen / pack_lwes..." << std::endl;
    FHEContext ctx(SecurityParams{128, 2048, 60, 3.2f, 64});
    const uint32_t n = ctx.params().n, L = ctx.num_levels(), count = 8, step = n / count;
    const uint64_t t = ctx.params().t;
    REQUIRE(n == 2048 && L == 2 && t == 65537);
    PublicKey pk; SecretKey sk;
    ctx.keygen(pk, sk);
    PackingKeys keys;
    ctx.packing_key_gen(keys, sk, 16);
    REQUIRE(keys.sets.size() == 11 && keys.decomp_bits == 16 && keys.made_for != nullptr);
    for (fhe_relin_keys_t *k : keys.sets) REQUIRE(k != nullptr);

    std::vector<uint64_t> values(n);
    for (uint32_t i = 0; i < n; i++) values[i] = (977ull * i + 13) % t;
    Plaintext pt; ctx.encode(pt, values);
    Ciphertext ct; ctx.encrypt_fused(ct, pt, pk);
    const std::vector<uint64_t> m = limb0(*pt.poly, n);
    for (uint64_t v : m) REQUIRE(v < t);

    // eight coefficients out as LWE samples under the ring key, [count][L][n + 1]
    const size_t sample = (size_t)L * (n + 1);
    std::vector<uint64_t> lwe(count * sample);
    void *d = nullptr; check(fhe_hip_malloc(&d, lwe.size() * 8), "malloc");
    for (uint32_t i = 0; i < count; i++)
        check(fhe_rlwe_sample_extract(ctx.params().rns_ntt->handle(), (uint64_t *)d + i * sample, ct.components[0]->coeffs, ct.components[1]->coeffs, i * step, 1), "extract");
    check(fhe_hip_sync(), "sync");
    check(fhe_hip_memcpy_d2h(lwe.data(), d, lwe.size() * 8), "memcpy d2h");
    check(fhe_hip_free(d), "free");

    for (int normalize = 1; normalize >= 0; normalize--) {
        Ciphertext packed;
        ctx.pack_lwes(packed, keys, lwe, count, true, normalize != 0);
        REQUIRE(packed.level == 0 && packed.components.size() == 2);
        REQUIRE(packed.correction == (normalize ? 1 : n % t));
        Plaintext out; ctx.decrypt_fused(out, packed, sk);
        const std::vector<uint64_t> got = limb0(*out.poly, n);
        for (uint32_t x = 0; x < n; x++) REQUIRE(got[x] == (x % step ? 0 : m[x]));
        std::cout << "  normalize " << normalize << ": correction " << packed.correction << ", budget " << ctx.noise_budget_fused(packed, sk) << std::endl;
        delete out.poly;
    }
    {   // keys made by another context are refused before anything runs
        FHEContext other(SecurityParams{128, 2048, 60, 3.2f, 64});
        Ciphertext o; bool threw = false;
        try { other.pack_lwes(o, keys, lwe, count); } catch (const std::exception &) { threw = true; }
        REQUIRE(threw && o.components.empty());
        try { threw = false; ctx.pack_lwes(o, keys, lwe, count + 1); } catch (const std::exception &) { threw = true; }
        REQUIRE(threw);
    }
    delete pt.poly; delete sk.sk; delete pk.pk0; delete pk.pk1;
    std::cout << "ALL PASSED" << std::endl;
    return 0;
}
