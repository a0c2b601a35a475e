// test_bfv_mirror.cpp -- BFV through the C++ mirror (include/fhe/fhe.hpp): a context with noise scale 1, encrypt_bfv (Delta m + e),
// multiply_bfv (one fhe_bfv_multiply_relin; three components without keys) and decrypt_bfv (round(t v / Q) mod t), on the slot values
// 1 2 3 4 x 5 6 7 8 and a depth-2 product, ASSERTED.  The same ciphertexts through the modular FHEContext::multiply must not decrypt to the product.
//   ./test_bfv_mirror             full run (needs the MI355X)
//   ./test_bfv_mirror --host-only defaults and rejections that need no device
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "fhe/fhe.hpp"

using namespace fhe;

#define REQUIRE(cond)                                                                       \
    do {                                                                                    \
        if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static bool slots_are(const std::vector<uint64_t> &out, const std::vector<uint64_t> &want) {
    for (size_t i = 0; i < out.size(); i++) if (out[i] != (i < want.size() ? want[i] : 0)) return false;
    return true;
}
template <class Fn> static bool throws(Fn &&fn) { try { fn(); } catch (const std::exception &) { return true; } return false; }

int main(int argc, char **argv) {
    {
        BFVMultiplier bm;
        REQUIRE(!bm.handle && bm.aux_moduli.empty() && !bm.made_for && bm.t == 0);
        bm.clear();                                                              // destroying nothing is fine
        fhe_bfv_multiplier_t *out = reinterpret_cast<fhe_bfv_multiplier_t *>(0x1234);
        const uint64_t aux[2] = {12289, 40961};
        REQUIRE(fhe_bfv_multiplier_create(nullptr, &out, 65537, aux, 2) == FHE_ERR_INVALID_ARG && out == reinterpret_cast<fhe_bfv_multiplier_t *>(0x1234));
        REQUIRE(fhe_bfv_multiplier_destroy(nullptr) == FHE_OK);
        REQUIRE(fhe_bfv_multiply_relin(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1) == FHE_ERR_INVALID_ARG);
    }
    if (argc > 1 && !std::strcmp(argv[1], "--host-only")) { std::cout << "host-only: PASSED" << std::endl; return 0; }

    SecurityParams sp{128, 4096, 120, 3.2f, 64};                                // 4 limbs of 30 bits, t = 65537
    FHEContext ctx(sp);
    ctx.seed(2026);
    REQUIRE(ctx.noise_scale() == ctx.params().t);                               // the default stays BGV-style
    REQUIRE(throws([&] { ctx.set_noise_scale(0); }));
    ctx.set_noise_scale(1);                                                     // BFV: before key generation
    PublicKey pk; SecretKey sk; RelinKeys rlk, none;
    ctx.keygen(pk, sk);
    ctx.relinkey_gen(rlk, sk, 16);
    Plaintext pa, pb, pr;
    ctx.encode(pa, {1, 2, 3, 4});
    ctx.encode(pb, {5, 6, 7, 8});
    Ciphertext ca, cb, cprod, c3, cdeep, cmod;
    ctx.encrypt_bfv(ca, pa, pk); ctx.encrypt_bfv(cb, pb, pk);
    std::vector<uint64_t> out;
    ctx.decrypt_bfv(pr, ca, sk); ctx.decode(out, pr);
    REQUIRE(slots_are(out, {1, 2, 3, 4}));
    ctx.decrypt_bfv(pr, cb, sk); ctx.decode(out, pr);
    REQUIRE(slots_are(out, {5, 6, 7, 8}));
    ctx.decrypt(pr, ca, sk); ctx.decode(out, pr);                               // the BGV-flavoured decrypt reads the low bits: not the message
    REQUIRE(!slots_are(out, {1, 2, 3, 4}));

    ctx.multiply_bfv(cprod, ca, cb, rlk);
    REQUIRE(cprod.components.size() == 2 && cprod.level == 0 && cprod.correction == 1);
    ctx.decrypt_bfv(pr, cprod, sk); ctx.decode(out, pr);
    std::cout << "  BFV product: " << out[0] << " " << out[1] << " " << out[2] << " " << out[3] << " (expected: 5 12 21 32)" << std::endl;
    REQUIRE(slots_are(out, {5, 12, 21, 32}));

    ctx.multiply_bfv(c3, ca, cb, none);                                         // no keys: the three components stay, decrypt_bfv takes c2 s^2
    REQUIRE(c3.components.size() == 3);
    ctx.decrypt_bfv(pr, c3, sk); ctx.decode(out, pr);
    REQUIRE(slots_are(out, {5, 12, 21, 32}));

    ctx.multiply_bfv(cdeep, cprod, ca, rlk);                                    // depth 2: (a b) a
    ctx.decrypt_bfv(pr, cdeep, sk); ctx.decode(out, pr);
    std::cout << "  depth 2: " << out[0] << " " << out[1] << " " << out[2] << " " << out[3] << " (expected: 5 24 63 128)" << std::endl;
    REQUIRE(slots_are(out, {5, 24, 63, 128}));

    ctx.multiply(cmod, ca, cb, rlk);                                            // the product modulo Q is not a BFV product
    ctx.decrypt_bfv(pr, cmod, sk); ctx.decode(out, pr);
    REQUIRE(!slots_are(out, {5, 12, 21, 32}));

    {   // a multiplier of the caller's: chosen primes are of the ciphertext primes' size, outside the basis, and satisfy the bound with room for no fewer
        BFVMultiplier own;
        ctx.bfv_multiplier_gen(own);
        REQUIRE(own.handle && own.t == ctx.params().t && own.aux_moduli.size() == 6);   // 2^33 < 32 t n < 2^58: two primes more than the basis
        for (uint64_t p : own.aux_moduli) {
            REQUIRE((p >> 29) == 1 && p % (2 * 4096) == 1);
            for (const uint256_t &q : ctx.params().rns_moduli) REQUIRE(q.limbs[0] != p);
        }
        Ciphertext c;
        ctx.multiply_bfv(c, ca, cb, rlk, own);
        ctx.decrypt_bfv(pr, c, sk); ctx.decode(out, pr);
        REQUIRE(slots_are(out, {5, 12, 21, 32}));
        BFVMultiplier few;
        REQUIRE(throws([&] { ctx.bfv_multiplier_gen(few, {own.aux_moduli[0]}); }) && !few.handle);   // P <= 32 t n Q
        REQUIRE(throws([&] { ctx.multiply_bfv(c, ca, cb, rlk, few); }));                             // an empty multiplier
        FHEContext other(sp);
        BFVMultiplier theirs;
        other.bfv_multiplier_gen(theirs);
        REQUIRE(throws([&] { ctx.multiply_bfv(c, ca, cb, rlk, theirs); }));                          // another context's
        Ciphertext odd = {};
        REQUIRE(throws([&] { ctx.multiply_bfv(c, odd, cb, rlk); }));                                 // not two components
    }
    delete pk.pk0; delete pk.pk1; delete sk.sk; delete pa.poly; delete pb.poly; delete pr.poly;
    std::cout << "ALL PASSED" << std::endl;
    return 0;
}
