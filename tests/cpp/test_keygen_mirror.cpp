// test_keygen_mirror.cpp -- FHEContext::relinkey_gen_fused / galoiskey_gen_fused (include/fhe/fhe.hpp: one fhe_keyswitch_keys_generate each,
// rows read back with fhe_relin_keys_export) against the host-made keys of relinkey_gen / galoiskey_gen: everything a key does must decrypt
// to the same slots with either.  n = 2048, t = 65537, 6 x 30-bit primes, digit width 16.
//   ./test_keygen_mirror              the scenarios on the GPU
//   ./test_keygen_mirror --host-only  links and checks the new entry points' null-handle rejection (no device)
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

static std::vector<uint64_t> slots(FHEContext &ctx, const Ciphertext &ct, const SecretKey &sk) {
    Plaintext pt; std::vector<uint64_t> out;
    ctx.decrypt(pt, ct, sk);
    ctx.decode(out, pt);
    delete pt.poly;
    REQUIRE(ctx.noise_budget_fused(ct, sk) > 0);
    return out;
}

static void test_host() {
    fhe_relin_keys_t *outs[2] = {reinterpret_cast<fhe_relin_keys_t *>(0x1234), reinterpret_cast<fhe_relin_keys_t *>(0x5678)};
    const uint32_t elts[2] = {0, 3}; const uint64_t seeds[2] = {1, 2};
    REQUIRE(fhe_keyswitch_keys_generate(nullptr, nullptr, 16, elts, 2, 65537, 3.2, seeds, outs) == FHE_ERR_INVALID_ARG);
    REQUIRE(outs[0] == reinterpret_cast<fhe_relin_keys_t *>(0x1234) && outs[1] == reinterpret_cast<fhe_relin_keys_t *>(0x5678));
    REQUIRE(fhe_relin_keys_export(nullptr, nullptr, nullptr, nullptr) == FHE_ERR_INVALID_ARG);
}

// everything the keys do, on `a` (slots x) and `b` (slots y) at their level: the fused keys and the host-made ones decrypt to the same slots
static void check_level(FHEContext &ctx, const SecretKey &sk, const RelinKeys &rlk, const RelinKeys &rlk_f, const GaloisKeys &gk, const GaloisKeys &gk_f,
                        const Ciphertext &a, const Ciphertext &b, const std::vector<uint64_t> &xy, const std::vector<Plaintext> &diag, const char *what) {
    const std::vector<int> steps = {1, 5, -1};
    Ciphertext p, pf, r, rf;
    ctx.multiply(p, a, b, rlk); ctx.multiply(pf, a, b, rlk_f);
    REQUIRE(pf.components.size() == 2 && slots(ctx, pf, sk) == xy && slots(ctx, p, sk) == xy);
    for (int st : steps) {
        ctx.rotate_rows(r, a, st, gk); ctx.rotate_rows(rf, a, st, gk_f);
        REQUIRE(slots(ctx, rf, sk) == slots(ctx, r, sk));
    }
    ctx.rotate_columns(r, a, gk); ctx.rotate_columns(rf, a, gk_f);
    const std::vector<uint64_t> col = slots(ctx, rf, sk), x = slots(ctx, a, sk);
    REQUIRE(col == slots(ctx, r, sk) && col != x);
    std::vector<Ciphertext> h = ctx.rotate_rows_hoisted(a, steps, gk), hf = ctx.rotate_rows_hoisted(a, steps, gk_f);
    for (size_t s = 0; s < steps.size(); s++) REQUIRE(slots(ctx, hf[s], sk) == slots(ctx, h[s], sk));
    std::vector<const Plaintext *> pp;
    for (const Plaintext &d : diag) pp.push_back(&d);
    Ciphertext lt = ctx.linear_transform_hoisted(a, steps, pp, gk), ltf = ctx.linear_transform_hoisted(a, steps, pp, gk_f);
    REQUIRE(slots(ctx, ltf, sk) == slots(ctx, lt, sk));
    std::cout << "  " << what << ": multiply + relinearise, rotate_rows, rotate_columns, rotate_rows_hoisted and linear_transform_hoisted agree; budget of the product "
              << ctx.noise_budget_fused(pf, sk) << " bits (fused keys) / " << ctx.noise_budget_fused(p, sk) << " bits (host keys)" << std::endl;
    for (Ciphertext &c : h) free_ct(c);
    for (Ciphertext &c : hf) free_ct(c);
    free_ct(p); free_ct(pf); free_ct(r); free_ct(rf); free_ct(lt); free_ct(ltf);
}

int main(int argc, char **argv) {
    test_host();
    if (argc > 1 && !std::strcmp(argv[1], "--host-only")) { std::cout << "host-only: PASSED" << std::endl; return 0; }
    int count = 0;
    check(fhe_hip_device_count(&count), "device count");
    REQUIRE(count > 0);
    std::cout << "Testing relinkey_gen_fused / galoiskey_gen_fused..." << std::endl;
    FHEContext ctx(SecurityParams{128, 2048, 180, 3.2f, 64});
    const uint32_t n = ctx.params().n; const uint64_t t = ctx.params().t;
    REQUIRE(n == 2048 && t == 65537 && ctx.num_levels() == 6);
    PublicKey pk; SecretKey sk;
    ctx.keygen(pk, sk);
    RelinKeys rlk, rlk_f;
    GaloisKeys gk, gk_f;
    ctx.relinkey_gen(rlk, sk, 16);
    ctx.galoiskey_gen(gk, sk, {1, 5, -1}, true, 16);
    ctx.relinkey_gen_fused(rlk_f, sk, 16);
    ctx.galoiskey_gen_fused(gk_f, sk, {1, 5}, false, 16);
    REQUIRE(gk_f.elements.size() == 2 && gk_f.imported.size() == 2);
    ctx.galoiskey_gen_fused(gk_f, sk, {1, 5, -1}, true, 16);            // only the missing elements are generated, in one call
    REQUIRE(gk_f.elements.size() == 4 && gk_f.imported.size() == 4 && gk_f.elements == gk.elements);
    REQUIRE(rlk_f.imported && rlk_f.rlk_keys.size() == rlk.rlk_keys.size() && gk_f.gal_keys.size() == gk.gal_keys.size());
    fhe_relin_keys_t *kept = rlk_f.imported;

    std::vector<uint64_t> x(n), y(n), xy(n);
    for (uint32_t i = 0; i < n; i++) { x[i] = (7 * i + 1) % t; y[i] = (13 * i + 5) % t; xy[i] = mulm(x[i], y[i], t); }
    std::vector<Plaintext> diag(3);
    for (size_t s = 0; s < diag.size(); s++) {
        std::vector<uint64_t> d(n);
        for (uint32_t i = 0; i < n; i++) d[i] = (uint64_t)((s + 2) * 1000003ull * (i + 1) + 17 * s) % t;
        ctx.encode(diag[s], d);
    }
    Plaintext px, py; ctx.encode(px, x); ctx.encode(py, y);
    Ciphertext a, b;
    ctx.encrypt(a, px, pk); ctx.encrypt(b, py, pk);
    REQUIRE(slots(ctx, a, sk) == x);
    check_level(ctx, sk, rlk, rlk_f, gk, gk_f, a, b, xy, diag, "level 0");
    REQUIRE(rlk_f.imported == kept);                                   // level 0 runs on the generated handles: nothing was imported again
    ctx.mod_switch_to_next(a); ctx.mod_switch_to_next(b);
    REQUIRE(a.level == 1);
    check_level(ctx, sk, rlk, rlk_f, gk, gk_f, a, b, xy, diag, "level 1 (keys sliced from the exported rows)");
    for (Plaintext &p : diag) delete p.poly;
    free_ct(a); free_ct(b); delete px.poly; delete py.poly;
    delete sk.sk; delete pk.pk0; delete pk.pk1;
    std::cout << "ALL PASSED" << std::endl;
    return 0;
}
