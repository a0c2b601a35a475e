// test_encrypt_mirror.cpp -- public-key encryption as one engine call through the C++ mirror (include/fhe/fhe.hpp):
// FHEContext::encrypt_fused imports the public key once and makes one fhe_ct_encrypt with three seeds of the context generator.
//   ./test_encrypt_mirror              the scenarios on the GPU
//   ./test_encrypt_mirror --host-only  links and checks the new entry points' argument validation (no device)
#include <cmath>
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

static std::vector<uint64_t> decrypt_slots(FHEContext &ctx, const Ciphertext &ct, const SecretKey &sk) {
    Plaintext pt; std::vector<uint64_t> out;
    ctx.decrypt(pt, ct, sk);
    ctx.decode(out, pt);
    delete pt.poly;
    return out;
}
static void free_ct(Ciphertext &ct) { for (Polynomial *p : ct.components) delete p; ct.components.clear(); }

static void test_host() {
    fhe_public_key_t *pk = reinterpret_cast<fhe_public_key_t *>(0x10);
    REQUIRE(fhe_public_key_create(nullptr, &pk, nullptr, nullptr) == FHE_ERR_INVALID_ARG);
    REQUIRE(pk == reinterpret_cast<fhe_public_key_t *>(0x10));          // a failed create leaves *out alone
    const uint64_t seeds[3] = {1, 2, 3};
    REQUIRE(fhe_ct_encrypt_reserve(nullptr, 3.2, 1) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_ct_encrypt(nullptr, nullptr, 65537, 3.2, seeds, nullptr, nullptr, nullptr, 1) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_public_key_destroy(nullptr) == FHE_OK);
}

// encode, encrypt_fused, decrypt, decode: the slots come back; the estimated noise budget is within 2 bits of encrypt's (the same noise terms;
// the 2 bits cover the different host and device draw ranges)
static void test_round_trip() {
    std::cout << "Testing encrypt_fused round trip..." << std::endl;
    SecurityParams sp{128, 2048, 120, 3.2f, 64};                        // n = 2048, 4 x 30-bit primes
    FHEContext ctx(sp);
    ctx.seed(77);
    const uint32_t n = ctx.params().n;
    const uint64_t t = ctx.params().t;
    PublicKey pk; SecretKey sk;
    ctx.keygen(pk, sk);
    std::vector<uint64_t> v(n);
    for (uint32_t i = 0; i < n; i++) v[i] = (11 * i + 3) % t;
    Plaintext pt; ctx.encode(pt, v);
    Ciphertext fused, plain;
    ctx.encrypt_fused(fused, pt, pk);
    REQUIRE(fused.components.size() == 2 && fused.level == 0 && fused.correction == 1);
    REQUIRE(pk.imported);                                               // the imported handle is kept ...
    fhe_public_key_t *first = pk.imported.get();
    REQUIRE(decrypt_slots(ctx, fused, sk) == v);
    Ciphertext again;
    ctx.encrypt_fused(again, pt, pk);
    REQUIRE(pk.imported.get() == first);                                // ... and reused
    REQUIRE(decrypt_slots(ctx, again, sk) == v);
    ctx.encrypt(plain, pt, pk);
    const float bf = ctx.estimate_noise_budget(fused, sk), bp = ctx.estimate_noise_budget(plain, sk);
    std::cout << "  noise budget: encrypt_fused " << bf << " bits, encrypt " << bp << " bits" << std::endl;
    REQUIRE(bf > 0 && std::fabs(bf - bp) <= 2.0f);
    free_ct(fused); free_ct(again); free_ct(plain);
    delete pt.poly; delete sk.sk; delete pk.pk0; delete pk.pk1;
}

// the reference scenario of test_fhe_mirror.cpp with both inputs encrypted by encrypt_fused
static void test_reference_scenario() {
    std::cout << "Testing the reference scenario on encrypt_fused ciphertexts..." << std::endl;
    SecurityParams sp{128, 4096, 120, 3.2f, 64};
    FHEContext ctx(sp);
    ctx.seed(2026);
    PublicKey pk; SecretKey sk; RelinKeys rlk;
    ctx.keygen(pk, sk);
    ctx.relinkey_gen(rlk, sk, 16);
    Plaintext pa, pb, pr;
    ctx.encode(pa, {5, 10, 15, 20});
    ctx.encode(pb, {3, 6, 9, 12});
    Ciphertext ca, cb, csum, cprod;
    ctx.encrypt_fused(ca, pa, pk); ctx.encrypt_fused(cb, pb, pk);
    std::vector<uint64_t> out;
    ctx.decrypt(pr, ca, sk); ctx.decode(out, pr);
    REQUIRE(out[0] == 5 && out[1] == 10 && out[2] == 15 && out[3] == 20);
    ctx.add(csum, ca, cb);
    ctx.decrypt(pr, csum, sk); ctx.decode(out, pr);
    std::cout << "  Addition result: " << out[0] << " " << out[1] << " " << out[2] << " " << out[3] << " (expected: 8 16 24 32)" << std::endl;
    REQUIRE(out[0] == 8 && out[1] == 16 && out[2] == 24 && out[3] == 32);
    ctx.multiply(cprod, ca, cb, rlk);
    REQUIRE(cprod.components.size() == 2);
    ctx.decrypt(pr, cprod, sk); ctx.decode(out, pr);
    std::cout << "  Multiplication result: " << out[0] << " " << out[1] << " " << out[2] << " " << out[3] << " (expected: 15 60 135 240)" << std::endl;
    REQUIRE(out[0] == 15 && out[1] == 60 && out[2] == 135 && out[3] == 240);
    for (Ciphertext *c : {&ca, &cb, &csum, &cprod}) free_ct(*c);
    delete pa.poly; delete pb.poly; delete pr.poly;
    delete sk.sk; delete pk.pk0; delete pk.pk1;
}

int main(int argc, char **argv) {
    test_host();
    if (argc > 1 && !std::strcmp(argv[1], "--host-only")) { std::cout << "host-only: PASSED" << std::endl; return 0; }
    int count = 0;
    check(fhe_hip_device_count(&count), "device count");
    REQUIRE(count > 0);
    test_round_trip();
    test_reference_scenario();
    std::cout << "ALL PASSED" << std::endl;
    return 0;
}
