// test_hoisted_mirror.cpp -- hoisted rotations through the C++ mirror (include/fhe/fhe.hpp): FHEContext::rotate_rows_hoisted decomposes the
// ciphertext once and applies one Galois element per step; the results decrypt to the slots of rotate_rows (ciphertext bits differ).
//   ./test_hoisted_mirror              the scenario on the GPU
//   ./test_hoisted_mirror --host-only  links and checks the new entry points' argument validation (no device)
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
    uint64_t bytes = 5;
    REQUIRE(fhe_ct_hoist(nullptr, 16, nullptr, 1) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_ct_apply_galois_hoisted(nullptr, nullptr, 3, nullptr, nullptr, nullptr, 1) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_rns_ntt_reserve_hoist(nullptr, 16, 1) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_rns_ntt_hoist_bytes(nullptr, &bytes) == FHE_ERR_INVALID_ARG && bytes == 5);
}

static void test_hoisted_rotations() {
    std::cout << "Testing rotate_rows_hoisted..." << std::endl;
    SecurityParams sp{128, 4096, 120, 3.2f, 64};
    FHEContext ctx(sp);
    const uint32_t n = ctx.params().n;
    const uint64_t t = ctx.params().t;
    PublicKey pk; SecretKey sk;
    ctx.keygen(pk, sk);
    GaloisKeys gk;
    const std::vector<int> steps = {1, 2, -3};
    ctx.galoiskey_gen(gk, sk, steps, false, 16);
    std::vector<uint64_t> v(n);
    for (uint32_t i = 0; i < n; i++) v[i] = (7 * i + 1) % t;
    Plaintext pt; ctx.encode(pt, v);
    Ciphertext ct; ctx.encrypt(ct, pt, pk);
    std::vector<Ciphertext> hoisted = ctx.rotate_rows_hoisted(ct, steps, gk);
    REQUIRE(hoisted.size() == steps.size());
    for (size_t s = 0; s < steps.size(); s++) {
        Ciphertext r;
        ctx.rotate_rows(r, ct, steps[s], gk);
        const std::vector<uint64_t> want = decrypt_slots(ctx, r, sk), got = decrypt_slots(ctx, hoisted[s], sk);
        REQUIRE(want != v && got == want);
        free_ct(r);
        std::cout << "  step " << steps[s] << " decrypts to the slots of rotate_rows" << std::endl;
    }
    REQUIRE(decrypt_slots(ctx, ct, sk) == v);                           // the input is read only
    bool threw = false;                                                 // a step without its own key is an error, as in rotate_rows
    try { ctx.rotate_rows_hoisted(ct, {1, 5}, gk); } catch (const std::runtime_error &) { threw = true; }
    REQUIRE(threw);
    for (Ciphertext &c : hoisted) free_ct(c);
    free_ct(ct); delete pt.poly;
    delete sk.sk; delete pk.pk0; delete pk.pk1;
}

int main(int argc, char **argv) {
    test_host();
    if (argc > 1 && !std::strcmp(argv[1], "--host-only")) { std::cout << "host-only: PASSED" << std::endl; return 0; }
    int count = 0;
    check(fhe_hip_device_count(&count), "device count");
    REQUIRE(count > 0);
    test_hoisted_rotations();
    std::cout << "ALL PASSED" << std::endl;
    return 0;
}
