// test_ckks_mirror.cpp -- the CKKS part of the mirror (include/fhe/fhe.hpp): CKKSEncoder, FHEContext::encrypt_ckks, one multiply +
// relinearize + rescale_to_next, decrypt_ckks.  n = 2048, 3 x 30-bit primes, plaintext modulus 2 (key noise 2 e), digit width 16, scale 2^30.
//   ./test_ckks_mirror out.bin       the scenario on the GPU; writes n, scale_out, z1, z2, the decoded slots and the decrypted integers for
//                                    tests/test_ckks_mirror.py, which applies the assertions of the end-to-end case against the long-double model
//   ./test_ckks_mirror --host-only   links, checks the defaults and the null-handle rejections (no device)
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <vector>

#include "fhe/fhe.hpp"

using namespace fhe;
typedef std::complex<double> cd;

#define REQUIRE(cond)                                                                       \
    do {                                                                                    \
        if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static void free_ct(Ciphertext &ct) { for (Polynomial *p : ct.components) delete p; ct.components.clear(); }

static void test_host() {
    Ciphertext ct;
    REQUIRE(ct.scale == 1.0 && ct.level == 0 && ct.correction == 1);
    fhe_ckks_encoder_t *out = reinterpret_cast<fhe_ckks_encoder_t *>(0x1234);
    REQUIRE(fhe_ckks_encoder_create(nullptr, &out) == FHE_ERR_INVALID_ARG && out == reinterpret_cast<fhe_ckks_encoder_t *>(0x1234));
    REQUIRE(fhe_ckks_encoder_destroy(nullptr) == FHE_OK);
    REQUIRE(fhe_ckks_encode(nullptr, nullptr, nullptr, nullptr, nullptr, 1.0, 1) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_ckks_decode(nullptr, nullptr, nullptr, nullptr, 0, 1.0, 1) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_ckks_decode_poly(nullptr, nullptr, nullptr, nullptr, 1.0, 1) == FHE_ERR_INVALID_ARG);
    uint32_t a[8]; uint8_t c[8];
    REQUIRE(fhe_ckks_slot_table(16, a, c) == FHE_OK && a[0] == 0 && c[0] == 0 && a[1] == 7 && c[1] == 1);   // e(1) = 3: 32 - 3 = 4 * 7 + 1
    void (CKKSEncoder::*enc)(Plaintext &, const std::vector<cd> &, double, uint32_t) = &CKKSEncoder::encode;
    void (CKKSEncoder::*dec)(std::vector<cd> &, const Plaintext &, double) = &CKKSEncoder::decode;
    REQUIRE(enc && dec);
    std::cout << "host-only: PASSED" << std::endl;
}

template <class T> static void put(std::FILE *f, const std::vector<T> &v) { REQUIRE(std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size()); }

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--host-only")) { test_host(); return 0; }
    if (argc != 2) { std::fprintf(stderr, "usage: %s out.bin | --host-only\n", argv[0]); return 2; }
    const SecurityParams sp{128, 2048, 90, 3.2f, 64};
    FHEContext ctx(sp);
    REQUIRE(ctx.num_levels() == 3);
    ctx.set_plain_modulus(2);
    PublicKey pk; SecretKey sk; RelinKeys rlk;
    ctx.keygen(pk, sk);
    ctx.relinkey_gen(rlk, sk, 16);
    const uint32_t n = ctx.params().n, h = n / 2;
    const double scale = 1073741824.0;                               // 2^30
    CKKSEncoder encoder(ctx);
    REQUIRE(encoder.slot_count() == h);
    uint64_t seed = 2024;
    auto unit = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (double)(seed >> 11) / 9007199254740992.0; };
    std::vector<cd> z1(h), z2(h), back, got;
    for (uint32_t k = 0; k < h; k++) { z1[k] = cd(unit(), unit()); z2[k] = cd(unit(), unit()); }

    Plaintext p1, p2;
    encoder.encode(p1, z1, scale); encoder.encode(p2, z2, scale);
    // (round trip through decode needs |c| < q_0 / 2: a plaintext at a smaller scale, on the one-limb level too)
    Plaintext small;
    for (uint32_t level : {0u, 2u}) {
        encoder.encode(small, z1, 16777216.0, level);                // 2^24
        REQUIRE(small.poly->num_limbs == 3 - level);
        encoder.decode(back, small, 16777216.0);
        double worst = 0;
        for (uint32_t k = 0; k < h; k++) worst = std::max(worst, std::abs(back[k] - z1[k]));
        std::cout << "  round trip at level " << level << ": max error " << worst << std::endl;
        REQUIRE(worst <= (h + 1) / 16777216.0 + 1e-12);
    }
    Ciphertext c1, c2, prod;
    ctx.encrypt_ckks(c1, p1, scale, pk); ctx.encrypt_ckks(c2, p2, scale, pk);
    REQUIRE(c1.scale == scale && c1.level == 0 && c1.components.size() == 2);
    ctx.multiply(prod, c1, c2, rlk);                                  // tensor product + relinearisation
    ctx.relinearize(prod, rlk);
    REQUIRE(prod.components.size() == 2);
    prod.scale = c1.scale * c2.scale;
    ctx.rescale_to_next(prod);
    const double q_last = (double)ctx.params().rns_moduli[2].limbs[0];
    REQUIRE(prod.level == 1 && prod.components[0]->num_limbs == 2 && prod.scale == scale * scale / q_last);
    std::vector<int64_t> v;
    ctx.decrypt_ckks(got, prod, sk, &v);
    REQUIRE(got.size() == h && v.size() == n);
    double worst = 0;
    for (uint32_t k = 0; k < h; k++) worst = std::max(worst, std::abs(got[k] - z1[k] * z2[k]));
    std::cout << "  product: scale_out " << prod.scale << ", max slot error " << worst << std::endl;
    REQUIRE(worst < 1.0 / 256);                                      // the two assertions proper: tests/test_ckks_mirror.py
    Ciphertext last = {};
    bool threw = false;
    ctx.rescale_to_next(prod);
    try { ctx.rescale_to_next(prod); } catch (const std::runtime_error &) { threw = true; }
    REQUIRE(threw && prod.level == 2);

    std::FILE *f = std::fopen(argv[1], "wb");
    REQUIRE(f);
    const std::vector<double> head = {(double)n, scale * scale / q_last};
    put(f, head); put(f, z1); put(f, z2); put(f, got); put(f, v);
    REQUIRE(std::fclose(f) == 0);
    free_ct(c1); free_ct(c2); free_ct(prod); free_ct(last);
    delete p1.poly; delete p2.poly; delete small.poly;
    delete sk.sk; delete pk.pk0; delete pk.pk1;
    std::cout << "ALL PASSED" << std::endl;
    return 0;
}
