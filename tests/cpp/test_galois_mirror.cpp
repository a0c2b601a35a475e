// test_galois_mirror.cpp -- slot rotations through the C++ mirror (include/fhe/fhe.hpp): GaloisKeys, FHEContext::galoiskey_gen,
// rotate_rows, rotate_columns (include/fhe.cuh:58-61, 86, 112-116).
//   ./test_galois_mirror              host maths + the rotation scenarios on the GPU
//   ./test_galois_mirror --host-only  the Galois-element helper only (no device)
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

static uint32_t pow_mod(uint64_t b, uint64_t e, uint64_t m) {
    uint64_t r = 1 % m;
    for (b %= m; e; e >>= 1) { if (e & 1) r = r * b % m; b = b * b % m; }
    return (uint32_t)r;
}

static void test_galois_element_host() {
    std::cout << "Testing fhe_galois_element (host)..." << std::endl;
    for (uint32_t n : {8u, 1024u, 4096u, 65536u}) {
        const uint32_t m = 2 * n, half = n / 2;
        for (int steps : {0, 1, 2, 3, -1, -2, (int)half, (int)half + 1, -(int)half - 5, 1000}) {
            uint32_t g = 0;
            REQUIRE(fhe_galois_element(n, steps, &g) == FHE_OK);
            const uint32_t e = (uint32_t)(((long long)steps % half + half) % half);
            REQUIRE(g == pow_mod(3, e, m) && (g & 1));
        }
        uint32_t a = 0, b = 0;                                          // opposite steps are inverse elements
        REQUIRE(fhe_galois_element(n, 5, &a) == FHE_OK && fhe_galois_element(n, -5, &b) == FHE_OK);
        REQUIRE((uint64_t)a * b % m == 1);
    }
    uint32_t g = 0;
    for (uint32_t bad : {0u, 4u, 6u, 12u, 1000u}) REQUIRE(fhe_galois_element(bad, 1, &g) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_galois_element(1024, 1, nullptr) == FHE_ERR_INVALID_ARG);
    std::cout << "  3^(steps mod n/2) mod 2n; bad n rejected" << std::endl;
}

// slot i of sigma_g(m) holds slot pi_g(i) of m, 2 pi_g(i) + 1 = g (2i + 1) (mod 2n)
static std::vector<uint64_t> permuted(const std::vector<uint64_t> &v, uint32_t g, uint32_t n) {
    std::vector<uint64_t> out(n);
    for (uint32_t i = 0; i < n; i++) out[i] = v[(uint32_t)(((uint64_t)g * (2 * i + 1) % (2 * n) - 1) / 2)];
    return out;
}

static std::vector<uint64_t> decrypt_slots(FHEContext &ctx, const Ciphertext &ct, const SecretKey &sk) {
    Plaintext pt; std::vector<uint64_t> out;
    ctx.decrypt(pt, ct, sk);
    ctx.decode(out, pt);
    delete pt.poly;
    return out;
}

static void free_ct(Ciphertext &ct) { for (Polynomial *p : ct.components) delete p; ct.components.clear(); }

static void test_rotations() {
    std::cout << "Testing galoiskey_gen / rotate_rows / rotate_columns..." << std::endl;
    SecurityParams sp{128, 4096, 120, 3.2f, 64};
    FHEContext ctx(sp);
    const uint32_t n = ctx.params().n, half = n / 2;
    const uint64_t t = ctx.params().t;
    PublicKey pk; SecretKey sk;
    ctx.keygen(pk, sk);
    GaloisKeys gk;
    ctx.galoiskey_gen(gk, sk);
    const uint32_t levels = ctx.relin_levels(gk.decomp_bits);
    // +-2^i for i < log2(n/2) = 11 and 2n - 1; +2^10 and -2^10 are the same element (3 has order n/2 = 2048), so 22 distinct elements
    REQUIRE(gk.elements.size() == 2 * 11 - 1 + 1 && gk.gal_keys.size() == gk.elements.size() * levels);

    std::vector<uint64_t> v(n);
    for (uint32_t i = 0; i < n; i++) v[i] = (i + 1) % t;
    Plaintext pt; ctx.encode(pt, v);
    Ciphertext ct; ctx.encrypt(ct, pt, pk);
    REQUIRE(decrypt_slots(ctx, ct, sk) == v);

    // row order: row 0 holds the slots with 2i+1 = 3^k, row 1 those with 2i+1 = -3^k (mod 2n)
    std::vector<uint32_t> row0(half), row1(half);
    for (uint32_t k = 0; k < half; k++) {
        const uint32_t p = pow_mod(3, k, 2 * n);
        row0[k] = (p - 1) / 2; row1[k] = (2 * n - p - 1) / 2;
    }
    for (int steps : {1, -1, 3}) {                                      // 3 is not in the set: composed from 1 and 2
        Ciphertext r;
        ctx.rotate_rows(r, ct, steps, gk);
        const std::vector<uint64_t> got = decrypt_slots(ctx, r, sk);
        REQUIRE(got == permuted(v, ctx.galois_element(steps), n));
        const uint32_t sh = (uint32_t)((steps % (int)half + (int)half) % (int)half);
        for (uint32_t k = 0; k < half; k++) {                           // cyclic left shift by `steps` of both rows
            REQUIRE(got[row0[k]] == v[row0[(k + sh) % half]]);
            REQUIRE(got[row1[k]] == v[row1[(k + sh) % half]]);
        }
        free_ct(r);
        std::cout << "  rotate_rows(" << steps << ") ok" << std::endl;
    }
    {
        Ciphertext r;
        ctx.rotate_columns(r, ct, gk);
        const std::vector<uint64_t> got = decrypt_slots(ctx, r, sk);
        REQUIRE(got == permuted(v, 2 * n - 1, n));
        for (uint32_t k = 0; k < half; k++) REQUIRE(got[row0[k]] == v[row1[k]] && got[row1[k]] == v[row0[k]]);
        free_ct(r);
        std::cout << "  rotate_columns swaps the rows" << std::endl;
    }
    {                                                                   // in place: result aliases ct
        Ciphertext r;
        ctx.rotate_rows(r, ct, 2, gk);
        ctx.rotate_rows(r, r, -2, gk);
        REQUIRE(decrypt_slots(ctx, r, sk) == v);
        free_ct(r);
    }
    {                                                                   // multiply, then rotate, then decrypt
        RelinKeys rlk;
        ctx.relinkey_gen(rlk, sk, 16);
        std::vector<uint64_t> w(n);
        for (uint32_t i = 0; i < n; i++) w[i] = (3 * i + 7) % t;
        Plaintext pw; ctx.encode(pw, w);
        Ciphertext cw; ctx.encrypt(cw, pw, pk);
        Ciphertext prod, r;
        ctx.multiply(prod, ct, cw, rlk);
        ctx.rotate_rows(r, prod, 1, gk);
        std::vector<uint64_t> vw(n);
        for (uint32_t i = 0; i < n; i++) vw[i] = v[i] * w[i] % t;
        REQUIRE(decrypt_slots(ctx, r, sk) == permuted(vw, ctx.galois_element(1), n));
        Ciphertext three;                                               // a 3-component ciphertext is rejected
        RelinKeys none;
        ctx.multiply(three, ct, cw, none);
        bool threw = false;
        try { ctx.rotate_rows(r, three, 1, gk); } catch (const std::runtime_error &) { threw = true; }
        REQUIRE(threw);
        GaloisKeys only_one;                                            // a step no composition of the set reaches
        ctx.galoiskey_gen(only_one, sk, {1}, false, 16);
        threw = false;
        try { ctx.rotate_rows(r, ct, 2, only_one); } catch (const std::runtime_error &) { threw = true; }
        REQUIRE(threw);
        for (Ciphertext *c : {&cw, &prod, &r, &three}) free_ct(*c);
        delete pw.poly;
        std::cout << "  multiply then rotate decrypts to the rotated slot-wise product" << std::endl;
    }
    free_ct(ct); delete pt.poly;
    delete sk.sk; delete pk.pk0; delete pk.pk1;
}

int main(int argc, char **argv) {
    test_galois_element_host();
    if (argc > 1 && !std::strcmp(argv[1], "--host-only")) { std::cout << "host-only: PASSED" << std::endl; return 0; }
    int count = 0;
    check(fhe_hip_device_count(&count), "device count");
    REQUIRE(count > 0);
    test_rotations();
    std::cout << "ALL PASSED" << std::endl;
    return 0;
}
