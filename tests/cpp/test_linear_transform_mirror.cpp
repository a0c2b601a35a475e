// test_linear_transform_mirror.cpp -- the hoisted linear transform through the C++ mirror (include/fhe/fhe.hpp):
// FHEContext::linear_transform_hoisted makes one hoist and one fhe_ct_linear_transform_hoisted for sum_s diagonal_s * rotate_rows(ct, step_s).
//   ./test_linear_transform_mirror              the scenario on the GPU
//   ./test_linear_transform_mirror --host-only  links and checks the new entry points' argument validation (no device)
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
    fhe_linear_transform_t *lt = reinterpret_cast<fhe_linear_transform_t *>(0x10);
    const uint32_t g = 1; const fhe_relin_keys_t *gk = nullptr; const void *p = nullptr;
    REQUIRE(fhe_linear_transform_create(nullptr, &lt, 16, &g, &gk, &p, 1) == FHE_ERR_INVALID_ARG);
    REQUIRE(lt == reinterpret_cast<fhe_linear_transform_t *>(0x10));   // a failed create leaves *out alone
    REQUIRE(fhe_linear_transform_reserve(nullptr, nullptr, 1) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_ct_linear_transform_hoisted(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_linear_transform_destroy(nullptr) == FHE_OK);
}

// four diagonals on `ct`: the result decrypts to sum_s d_s (.) rot(v, step_s), equals the composition rotate_rows_hoisted + multiply_plain + add
// when decrypted, and loses at most one bit of estimated noise budget against it (the ring elements are identical: slack for the estimator only)
static void check_transform(FHEContext &ctx, const Ciphertext &ct, const SecretKey &sk, const GaloisKeys &gk, const std::vector<int> &steps,
                            const std::vector<std::vector<uint64_t>> &diag, const std::vector<Plaintext> &pts, const char *what) {
    const uint32_t n = ctx.params().n;
    const uint64_t t = ctx.params().t;
    std::vector<const Plaintext *> pp;
    for (const Plaintext &p : pts) pp.push_back(&p);
    Ciphertext fused = ctx.linear_transform_hoisted(ct, steps, pp, gk);
    REQUIRE(fused.level == ct.level && fused.correction == ct.correction && fused.components.size() == 2);
    std::vector<Ciphertext> rot = ctx.rotate_rows_hoisted(ct, steps, gk);
    std::vector<uint64_t> want(n, 0);
    Ciphertext sum;
    for (size_t s = 0; s < steps.size(); s++) {
        const std::vector<uint64_t> r = decrypt_slots(ctx, rot[s], sk);
        for (uint32_t i = 0; i < n; i++) want[i] = (want[i] + (unsigned __int128)diag[s][i] * r[i] % t) % t;
        Ciphertext prod;
        ctx.multiply_plain(prod, rot[s], pts[s]);
        if (s == 0) { ctx.multiply_plain(sum, rot[s], pts[s]); } else ctx.add(sum, sum, prod);
        free_ct(prod);
    }
    const std::vector<uint64_t> got = decrypt_slots(ctx, fused, sk), comp = decrypt_slots(ctx, sum, sk);
    REQUIRE(got == want);
    REQUIRE(got == comp);
    const float bf = ctx.estimate_noise_budget(fused, sk), bc = ctx.estimate_noise_budget(sum, sk);
    std::cout << "  " << what << ": decrypts to the expected slots; noise budget fused " << bf << " bits, composition " << bc << " bits" << std::endl;
    REQUIRE(bf > 0 && bf >= bc - 1.0f);
    for (Ciphertext &c : rot) free_ct(c);
    free_ct(sum); free_ct(fused);
}

static void test_linear_transform() {
    std::cout << "Testing linear_transform_hoisted..." << std::endl;
    SecurityParams sp{128, 2048, 180, 3.2f, 64};                        // n = 2048, 6 x 30-bit primes
    FHEContext ctx(sp);
    const uint32_t n = ctx.params().n;
    const uint64_t t = ctx.params().t;
    REQUIRE(n == 2048 && ctx.params().rns_moduli.size() == 6);
    PublicKey pk; SecretKey sk;
    ctx.keygen(pk, sk);
    GaloisKeys gk;
    const std::vector<int> steps = {0, 1, 5, -1};
    ctx.galoiskey_gen(gk, sk, {1, 5, -1}, false, 16);
    std::vector<uint64_t> v(n);
    for (uint32_t i = 0; i < n; i++) v[i] = (7 * i + 1) % t;
    std::vector<std::vector<uint64_t>> diag(steps.size(), std::vector<uint64_t>(n));
    std::vector<Plaintext> pts(steps.size());
    for (size_t s = 0; s < steps.size(); s++) {
        for (uint32_t i = 0; i < n; i++) diag[s][i] = (uint64_t)((s + 2) * 1000003ull * (i + 1) + 17 * s) % t;
        ctx.encode(pts[s], diag[s]);
    }
    Plaintext pt; ctx.encode(pt, v);
    Ciphertext ct; ctx.encrypt(ct, pt, pk);
    check_transform(ctx, ct, sk, gk, steps, diag, pts, "level 0");
    REQUIRE(decrypt_slots(ctx, ct, sk) == v);                           // the input is read only
    ctx.mod_switch_to_next(ct);
    REQUIRE(ct.level == 1);
    check_transform(ctx, ct, sk, gk, steps, diag, pts, "level 1");
    bool threw = false;                                                 // a step without its own key is an error
    try { ctx.linear_transform_hoisted(ct, {1, 7}, {&pts[0], &pts[1]}, gk); } catch (const std::runtime_error &) { threw = true; }
    REQUIRE(threw);
    for (Plaintext &p : pts) delete p.poly;
    free_ct(ct); delete pt.poly;
    delete sk.sk; delete pk.pk0; delete pk.pk1;
}

int main(int argc, char **argv) {
    test_host();
    if (argc > 1 && !std::strcmp(argv[1], "--host-only")) { std::cout << "host-only: PASSED" << std::endl; return 0; }
    int count = 0;
    check(fhe_hip_device_count(&count), "device count");
    REQUIRE(count > 0);
    test_linear_transform();
    std::cout << "ALL PASSED" << std::endl;
    return 0;
}
