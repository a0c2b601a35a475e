// test_batch_encoder_mirror.cpp -- the device encoder through the C++ mirror (include/fhe/fhe.hpp): FHEContext::encode_fused / decode_fused /
// decrypt_decode_fused (natural slot order, equal to encode / decode) and class BatchEncoder (row order: rotate_rows shifts both rows).
//   ./test_batch_encoder_mirror              the scenarios on the GPU
//   ./test_batch_encoder_mirror --host-only  links and checks the new entry points' rejections and the host slot table (no device)
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

static void free_ct(Ciphertext &ct) { for (Polynomial *p : ct.components) delete p; ct.components.clear(); }

static void test_host() {
    fhe_batch_encoder_t *out = reinterpret_cast<fhe_batch_encoder_t *>(0x1234);
    REQUIRE(fhe_batch_encoder_create(nullptr, &out, 65537, FHE_SLOTS_NATURAL) == FHE_ERR_INVALID_ARG && out == reinterpret_cast<fhe_batch_encoder_t *>(0x1234));
    REQUIRE(fhe_batch_encoder_reserve(nullptr, nullptr, 1) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_slots_encode(nullptr, nullptr, nullptr, nullptr, 1) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_slots_decode(nullptr, nullptr, nullptr, nullptr, 1) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_slots_decode_poly(nullptr, nullptr, nullptr, nullptr, 1) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_batch_encoder_destroy(nullptr) == FHE_OK);
    uint32_t tab[8];
    REQUIRE(fhe_batch_encoder_slot_table(8, FHE_SLOTS_NATURAL, tab) == FHE_OK);
    const uint32_t natural[8] = {0, 4, 2, 6, 1, 5, 3, 7};               // position x holds the exponent 2 bitrev(x) + 1 = 2 i + 1
    REQUIRE(!std::memcmp(tab, natural, sizeof tab));
    REQUIRE(fhe_batch_encoder_slot_table(8, FHE_SLOTS_ROWS, tab) == FHE_OK);
    const uint32_t exps[8] = {1, 3, 9, 11, 15, 13, 7, 5};                // 3^k mod 16, then 16 minus those
    for (uint32_t x = 0; x < 8; x++) REQUIRE(exps[tab[x]] == 2 * natural[x] + 1);
}

static std::vector<uint256_t> containers(const Plaintext &pt) {
    std::vector<uint256_t> h(pt.poly->count());
    device_synchronize(); copy_to_host(h.data(), pt.poly->coeffs, h.size());
    return h;
}

// encode_fused against encode container for container, decode_fused against decode, on full and short value vectors
static void test_natural_order_equals_the_host_encoder() {
    std::cout << "Testing encode_fused / decode_fused against encode / decode..." << std::endl;
    SecurityParams sp{128, 2048, 120, 3.2f, 64};
    FHEContext ctx(sp);
    const uint32_t n = ctx.params().n; const uint64_t t = ctx.params().t;
    for (size_t len : {(size_t)n, (size_t)4, (size_t)0}) {
        std::vector<uint64_t> v(len);
        for (size_t i = 0; i < len; i++) v[i] = (1234567ull * i + 89) % (2 * t);   // above t too: both reduce
        Plaintext a, b;
        ctx.encode(a, v); ctx.encode_fused(b, v);
        const std::vector<uint256_t> ha = containers(a), hb = containers(b);
        REQUIRE(ha.size() == hb.size() && !std::memcmp(ha.data(), hb.data(), ha.size() * sizeof(uint256_t)));
        std::vector<uint64_t> da, db;
        ctx.decode(da, a); ctx.decode_fused(db, a);
        REQUIRE(da == db && da.size() == n);
        for (size_t i = 0; i < n; i++) REQUIRE(da[i] == (i < len ? v[i] % t : 0));
        delete a.poly; delete b.poly;
    }
}

// the reference scenario of test_fhe_mirror.cpp with the device encoder at both ends
static void test_reference_scenario() {
    std::cout << "Testing the reference scenario on encode_fused / decrypt_decode_fused..." << std::endl;
    SecurityParams sp{128, 4096, 120, 3.2f, 64};
    FHEContext ctx(sp);
    ctx.seed(2026);
    PublicKey pk; SecretKey sk; RelinKeys rlk;
    ctx.keygen(pk, sk);
    ctx.relinkey_gen(rlk, sk, 16);
    Plaintext pa, pb;
    ctx.encode_fused(pa, {5, 10, 15, 20});
    ctx.encode_fused(pb, {3, 6, 9, 12});
    Ciphertext ca, cb, csum, cprod;
    ctx.encrypt(ca, pa, pk); ctx.encrypt_fused(cb, pb, pk);
    std::vector<uint64_t> out;
    ctx.decrypt_decode_fused(out, ca, sk);
    REQUIRE(out.size() == 4096 && out[0] == 5 && out[1] == 10 && out[2] == 15 && out[3] == 20 && out[4] == 0);
    ctx.add(csum, ca, cb);
    ctx.decrypt_decode_fused(out, csum, sk);
    std::cout << "  Addition result: " << out[0] << " " << out[1] << " " << out[2] << " " << out[3] << " (expected: 8 16 24 32)" << std::endl;
    REQUIRE(out[0] == 8 && out[1] == 16 && out[2] == 24 && out[3] == 32);
    ctx.multiply(cprod, ca, cb, rlk);
    ctx.decrypt_decode_fused(out, cprod, sk);
    std::cout << "  Multiplication result: " << out[0] << " " << out[1] << " " << out[2] << " " << out[3] << " (expected: 15 60 135 240)" << std::endl;
    REQUIRE(out[0] == 15 && out[1] == 60 && out[2] == 135 && out[3] == 240);
    ctx.mod_switch_to_level(cprod, 1);                                    // a lower level: its own engine, its own encoder, correction != 1
    ctx.decrypt_decode_fused(out, cprod, sk);
    REQUIRE(out[0] == 15 && out[1] == 60 && out[2] == 135 && out[3] == 240 && out[5] == 0);
    for (Ciphertext *c : {&ca, &cb, &csum, &cprod}) free_ct(*c);
    delete pa.poly; delete pb.poly;
    delete sk.sk; delete pk.pk0; delete pk.pk1;
}

// BatchEncoder is the row order: rotate_rows(1) is the cyclic left shift of both rows, rotate_columns the swap
static void test_rows() {
    std::cout << "Testing BatchEncoder with rotate_rows / rotate_columns..." << std::endl;
    SecurityParams sp{128, 2048, 120, 3.2f, 64};
    FHEContext ctx(sp);
    BatchEncoder enc(ctx);
    const uint32_t n = enc.slot_count(), half = n / 2;
    REQUIRE(n == 2048);
    PublicKey pk; SecretKey sk; GaloisKeys gk;
    ctx.keygen(pk, sk);
    ctx.galoiskey_gen(gk, sk);
    std::vector<uint64_t> v(n), got;
    for (uint32_t i = 0; i < n; i++) v[i] = (7 * i + 1) % ctx.params().t;
    Plaintext pt; enc.encode(pt, v);
    enc.decode(got, pt);
    REQUIRE(got == v);
    Ciphertext ct, r;
    Plaintext dec;
    auto slots = [&](const Ciphertext &c) { ctx.decrypt_fused(dec, c, sk); enc.decode(got, dec); };
    ctx.encrypt(ct, pt, pk);
    slots(ct);
    REQUIRE(got == v);
    ctx.rotate_rows(r, ct, 1, gk);
    slots(r);
    for (uint32_t k = 0; k < half; k++) REQUIRE(got[k] == v[(k + 1) % half] && got[half + k] == v[half + (k + 1) % half]);
    ctx.rotate_columns(r, ct, gk);
    slots(r);
    for (uint32_t k = 0; k < half; k++) REQUIRE(got[k] == v[half + k] && got[half + k] == v[k]);
    free_ct(ct); free_ct(r);
    delete pt.poly; delete dec.poly; delete sk.sk; delete pk.pk0; delete pk.pk1;
}

int main(int argc, char **argv) {
    test_host();
    if (argc > 1 && !std::strcmp(argv[1], "--host-only")) { std::cout << "host-only: PASSED" << std::endl; return 0; }
    int count = 0;
    check(fhe_hip_device_count(&count), "device count");
    REQUIRE(count > 0);
    test_natural_order_equals_the_host_encoder();
    test_reference_scenario();
    test_rows();
    std::cout << "ALL PASSED" << std::endl;
    return 0;
}
