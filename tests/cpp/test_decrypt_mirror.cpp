// test_decrypt_mirror.cpp -- FHEContext::decrypt_fused / noise_budget_fused (include/fhe/fhe.hpp: one fhe_ct_decrypt on the engine of the
// ciphertext's level) against FHEContext::decrypt / estimate_noise_budget.  n = 2048, t = 65537, 6 x 30-bit primes, digit width 16.
//   ./test_decrypt_mirror              the scenarios on the GPU
//   ./test_decrypt_mirror --host-only  links and checks the new entry points' null-handle rejection (no device)
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
static uint64_t mulm(uint64_t a, uint64_t b, uint64_t t) { return (uint64_t)((unsigned __int128)a * b % t); }

struct Fixture {
    FHEContext ctx;
    PublicKey pk; SecretKey sk;
    RelinKeys rlk;
    uint32_t n; uint64_t t;
    explicit Fixture(const SecurityParams &sp) : ctx(sp) {
        n = ctx.params().n; t = ctx.params().t;
        ctx.keygen(pk, sk);
        ctx.relinkey_gen(rlk, sk, 16);
    }
    ~Fixture() { delete sk.sk; delete pk.pk0; delete pk.pk1; }
    std::vector<uint64_t> values(uint64_t a, uint64_t b) const {
        std::vector<uint64_t> v(n);
        for (uint32_t i = 0; i < n; i++) v[i] = (a * i + b) % t;
        return v;
    }
    void encrypt(Ciphertext &ct, const std::vector<uint64_t> &v) {
        Plaintext pt; ctx.encode(pt, v);
        ctx.encrypt(ct, pt, pk);
        delete pt.poly;
    }
    // both decryptions of ct, slot for slot; the fused budget equals the mirror's or is one bit lower (a maximum that is a power of two)
    std::vector<uint64_t> both(const Ciphertext &ct, const char *what) {
        Plaintext a, b; std::vector<uint64_t> sa, sb;
        ctx.decrypt(a, ct, sk); ctx.decode(sa, a);
        ctx.decrypt_fused(b, ct, sk); ctx.decode(sb, b);
        delete a.poly; delete b.poly;
        REQUIRE(sa == sb);
        const float want = ctx.estimate_noise_budget(ct, sk), got = ctx.noise_budget_fused(ct, sk);
        std::cout << "  " << what << ": level " << ct.level << ", " << ct.components.size() << " components, correction " << ct.correction << ", budget " << want
                  << " (mirror) / " << got << " (fused)" << std::endl;
        REQUIRE(got == want || (want > 0 && got == want - 1));
        return sb;
    }
};

static void test_host() {
    fhe_secret_key_t *out = reinterpret_cast<fhe_secret_key_t *>(0x1234);
    REQUIRE(fhe_secret_key_create(nullptr, &out, nullptr) == FHE_ERR_INVALID_ARG && out == reinterpret_cast<fhe_secret_key_t *>(0x1234));
    REQUIRE(fhe_ct_decrypt_reserve(nullptr, 65537, 2, 1) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_ct_decrypt(nullptr, nullptr, 65537, 1, nullptr, nullptr, nullptr, 2, 1) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_secret_key_destroy(nullptr) == FHE_OK);
}

int main(int argc, char **argv) {
    test_host();
    if (argc > 1 && !std::strcmp(argv[1], "--host-only")) { std::cout << "host-only: PASSED" << std::endl; return 0; }
    int count = 0;
    check(fhe_hip_device_count(&count), "device count");
    REQUIRE(count > 0);
    Fixture F(SecurityParams{128, 2048, 180, 3.2f, 64});
    REQUIRE(F.t == 65537 && F.ctx.num_levels() == 6);
    const std::vector<uint64_t> x = F.values(7, 1), y = F.values(13, 5);
    std::vector<uint64_t> xy(F.n);
    for (uint32_t i = 0; i < F.n; i++) xy[i] = mulm(x[i], y[i], F.t);

    std::cout << "Testing decrypt_fused against decrypt..." << std::endl;
    Ciphertext a, b, p, p3, low;
    F.encrypt(a, x); F.encrypt(b, y);
    REQUIRE(F.both(a, "fresh") == x);
    F.ctx.multiply(p, a, b, F.rlk);
    REQUIRE(p.components.size() == 2 && F.both(p, "multiply + relinearize") == xy);
    {   // three components, before relinearisation: the tensor product through the engine, as FHEContext::multiply runs it
        RNS_NTTEngine &E = F.ctx.engine(0);
        for (int i = 0; i < 3; i++) p3.components.push_back(F.ctx.new_polynomial());
        check(fhe_ct_multiply(E.handle(), p3.components[0]->coeffs, p3.components[1]->coeffs, p3.components[2]->coeffs, a.components[0]->coeffs,
                              a.components[1]->coeffs, b.components[0]->coeffs, b.components[1]->coeffs, 1), "ct_multiply");
        device_synchronize();
        REQUIRE(F.both(p3, "three components") == xy);
    }
    F.encrypt(low, x);
    F.ctx.mod_switch_to_level(low, 2);
    REQUIRE(low.level == 2 && low.correction != 1 && F.both(low, "after mod_switch_to_level(2)") == x);
    F.ctx.mod_switch_to_level(p, 1);
    REQUIRE(F.both(p, "product at level 1") == xy);
    REQUIRE(F.sk.imported.size() == 6 && F.sk.imported[0] && F.sk.imported[1] && F.sk.imported[2] && !F.sk.imported[3]);   // one import per level used
    free_ct(a); free_ct(b); free_ct(p); free_ct(p3); free_ct(low);
    std::cout << "ALL PASSED" << std::endl;
    return 0;
}
