// test_modswitch_mirror.cpp -- leveled ciphertexts through the C++ mirror (include/fhe/fhe.hpp): FHEContext::mod_switch_to_next / mod_switch_to_level
// drop primes from a ciphertext, the correction factor keeps track of the plaintext, keys of lower levels are sliced from the level-0 keys, and
// estimate_noise_budget says how far a ciphertext is from failing.  n = 2048, t = 65537, 6 x 30-bit primes, digit width 16.
//   ./test_modswitch_mirror              the scenarios on the GPU
//   ./test_modswitch_mirror --host-only  links and checks the new entry point's null-handle rejection (no device)
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
static uint64_t mulm(uint64_t a, uint64_t b, uint64_t t) { return (uint64_t)((unsigned __int128)a * b % t); }
template <class Fn> static bool throws(Fn &&fn) {
    try { fn(); } catch (const std::runtime_error &) { return true; }
    return false;
}
// log2 of the modulus of a level: the noise of a ciphertext is log2(Q_l / 2) - budget bits
static double log2_q(const FHEContext &ctx, uint32_t level) {
    double s = 0;
    for (size_t l = 0; l + level < ctx.params().rns_moduli.size(); l++) s += std::log2((double)ctx.params().rns_moduli[l].limbs[0]);
    return s;
}
static double noise_bits(FHEContext &ctx, const Ciphertext &ct, const SecretKey &sk) { return log2_q(ctx, ct.level) - 1 - ctx.estimate_noise_budget(ct, sk); }

struct Fixture {
    FHEContext ctx;
    PublicKey pk; SecretKey sk;
    RelinKeys rlk;
    uint32_t n; uint64_t t;
    explicit Fixture(const SecurityParams &sp) : ctx(sp) { init(); }
    Fixture(const SecurityParams &sp, const std::vector<uint256_t> &moduli) : ctx(sp, moduli) { init(); }
    void init() {
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
};

static void test_host() {
    REQUIRE(fhe_ct_mod_switch_drop_last(nullptr, 65537, nullptr, nullptr, 2, 1) == FHE_ERR_INVALID_ARG);
}

static void test_every_level(Fixture &F) {
    std::cout << "Testing mod_switch_to_level at every level..." << std::endl;
    const std::vector<uint64_t> v = F.values(7, 1);
    const uint32_t L = F.ctx.num_levels();
    REQUIRE(L == 6);
    for (uint32_t l = 1; l < L; l++) {
        Ciphertext ct; F.encrypt(ct, v);
        const float fresh = F.ctx.estimate_noise_budget(ct, F.sk);
        F.ctx.mod_switch_to_level(ct, l);
        REQUIRE(ct.level == l && ct.components.size() == 2 && ct.components[0]->num_limbs == L - l && ct.correction != 1);
        const float budget = F.ctx.estimate_noise_budget(ct, F.sk);
        std::cout << "  level " << l << ": budget " << budget << " bits (fresh at level 0: " << fresh << ")" << std::endl;
        REQUIRE(budget > 0);
        REQUIRE(decrypt_slots(F.ctx, ct, F.sk) == v);
        if (l + 1 == L) {
            REQUIRE(throws([&] { F.ctx.mod_switch_to_next(ct); }));                 // the last level
            REQUIRE(throws([&] { F.ctx.mod_switch_to_level(ct, 2); }));             // a target above the current level
        }
        free_ct(ct);
    }
}

// (x y)^4 in three multiplications, each of two equally noisy operands: the noise squares at every step (measured: 53, 112, 173 bits without
// switching against Q of 174 bits).  A chain ((x y) z) w with fresh operands adds only about 30 bits per multiplication at these parameters and
// decrypts with or without switching, so it would not tell the two legs apart.  Returns the slots; last_budget is the budget at the end.
static std::vector<uint64_t> depth3(Fixture &F, bool switching, const std::vector<uint64_t> &x, const std::vector<uint64_t> &y, float &last_budget) {
    Ciphertext a, b, p;
    F.encrypt(a, x); F.encrypt(b, y);
    F.ctx.multiply(p, a, b, F.rlk);                                                 // relinearised with the keys of p's level
    for (int depth = 1;; depth++) {
        std::cout << "  depth " << depth << ": level " << p.level << ", budget " << F.ctx.estimate_noise_budget(p, F.sk) << ", noise "
                  << noise_bits(F.ctx, p, F.sk) << " bits";
        if (switching) {
            // as many levels as the measured budget suggests: one prime takes about 29 bits of noise away, down to the floor of about 22 bits that the
            // switch itself adds; stop once the noise is within a prime and a half of that floor
            while (noise_bits(F.ctx, p, F.sk) > 45 && p.level + 1 < F.ctx.num_levels()) F.ctx.mod_switch_to_next(p);
            std::cout << " -> level " << p.level << ", budget " << F.ctx.estimate_noise_budget(p, F.sk) << ", noise " << noise_bits(F.ctx, p, F.sk) << " bits";
        }
        std::cout << std::endl;
        if (depth == 3) break;
        Ciphertext sq;
        F.ctx.multiply(sq, p, p, F.rlk);
        free_ct(p);
        p = sq;
    }
    last_budget = F.ctx.estimate_noise_budget(p, F.sk);
    const std::vector<uint64_t> out = decrypt_slots(F.ctx, p, F.sk);
    free_ct(a); free_ct(b); free_ct(p);
    return out;
}

static void test_depth3(Fixture &F) {
    const std::vector<uint64_t> x = F.values(7, 1), y = F.values(13, 5);
    std::vector<uint64_t> want(F.n);
    for (uint32_t i = 0; i < F.n; i++) { const uint64_t p = mulm(x[i], y[i], F.t), p2 = mulm(p, p, F.t); want[i] = mulm(p2, p2, F.t); }
    float budget = 0;
    std::cout << "Testing a depth-3 chain with modulus switching..." << std::endl;
    REQUIRE(depth3(F, true, x, y, budget) == want);
    REQUIRE(budget > 0);
    std::cout << "Testing the same chain without switching (must fail)..." << std::endl;
    REQUIRE(depth3(F, false, x, y, budget) != want);
    REQUIRE(budget == 0);
}

static void test_rotations_at_level_2(Fixture &F) {
    std::cout << "Testing rotations at level 2 with keys generated at level 0..." << std::endl;
    GaloisKeys gk;
    F.ctx.galoiskey_gen(gk, F.sk, {1, -2}, true, 16);
    const std::vector<uint64_t> v = F.values(5, 3);
    Ciphertext ct, low;
    F.encrypt(ct, v); F.encrypt(low, v);
    F.ctx.mod_switch_to_level(low, 2);
    Ciphertext r0, r2, c0, c2;
    F.ctx.rotate_rows(r0, ct, 1, gk); F.ctx.rotate_rows(r2, low, 1, gk);
    REQUIRE(r2.level == 2 && r2.correction == low.correction && r2.components[0]->num_limbs == 4);
    const std::vector<uint64_t> rows0 = decrypt_slots(F.ctx, r0, F.sk);
    REQUIRE(rows0 != v && decrypt_slots(F.ctx, r2, F.sk) == rows0);
    F.ctx.rotate_columns(c0, ct, gk); F.ctx.rotate_columns(c2, low, gk);
    const std::vector<uint64_t> cols0 = decrypt_slots(F.ctx, c0, F.sk);
    REQUIRE(cols0 != v && decrypt_slots(F.ctx, c2, F.sk) == cols0);
    std::vector<Ciphertext> h0 = F.ctx.rotate_rows_hoisted(ct, {1, -2}, gk), h2 = F.ctx.rotate_rows_hoisted(low, {1, -2}, gk);
    for (size_t s = 0; s < h0.size(); s++) {
        const std::vector<uint64_t> want = decrypt_slots(F.ctx, h0[s], F.sk);
        REQUIRE(h2[s].level == 2 && want != v && decrypt_slots(F.ctx, h2[s], F.sk) == want);
    }
    REQUIRE(decrypt_slots(F.ctx, h0[0], F.sk) == rows0);
    REQUIRE(F.ctx.estimate_noise_budget(r2, F.sk) > 0);
    for (Ciphertext &c : h0) free_ct(c);
    for (Ciphertext &c : h2) free_ct(c);
    free_ct(ct); free_ct(low); free_ct(r0); free_ct(r2); free_ct(c0); free_ct(c2);
}

static void test_corrections_and_levels(Fixture &F) {
    std::cout << "Testing corrections and level checks..." << std::endl;
    const std::vector<uint64_t> x = F.values(7, 1), y = F.values(13, 5), z = F.values(3, 11), p = F.values(2, 9);
    Ciphertext cx, cy, a, b;
    F.encrypt(cx, x); F.encrypt(cy, y); F.encrypt(b, z);
    F.ctx.mod_switch_to_next(cx); F.ctx.mod_switch_to_next(cy);
    F.ctx.multiply(a, cx, cy, F.rlk);                                  // at level 1: correction q_5^-2
    F.ctx.mod_switch_to_next(a);                                       // level 2, switched after a multiplication
    F.ctx.mod_switch_to_level(b, 2);                                   // level 2, switched twice fresh
    REQUIRE(a.level == 2 && b.level == 2 && a.correction != b.correction && a.correction != 1 && b.correction != 1);
    std::vector<uint64_t> want(F.n);
    Ciphertext s;
    F.ctx.add(s, a, b);
    for (uint32_t i = 0; i < F.n; i++) want[i] = (mulm(x[i], y[i], F.t) + z[i]) % F.t;
    REQUIRE(s.level == 2 && s.correction == 1 && decrypt_slots(F.ctx, s, F.sk) == want);
    F.ctx.sub(s, a, b);
    for (uint32_t i = 0; i < F.n; i++) want[i] = (mulm(x[i], y[i], F.t) + F.t - z[i]) % F.t;
    REQUIRE(decrypt_slots(F.ctx, s, F.sk) == want);
    F.ctx.add(s, b, b);                                                // equal corrections are kept
    for (uint32_t i = 0; i < F.n; i++) want[i] = 2 * z[i] % F.t;
    REQUIRE(s.correction == b.correction && decrypt_slots(F.ctx, s, F.sk) == want);
    std::cout << "  budgets at level 2: product " << F.ctx.estimate_noise_budget(a, F.sk) << ", fresh " << F.ctx.estimate_noise_budget(b, F.sk) << std::endl;

    Plaintext pt; F.ctx.encode(pt, p);
    Ciphertext r;
    F.ctx.add_plain(r, b, pt);
    for (uint32_t i = 0; i < F.n; i++) want[i] = (z[i] + p[i]) % F.t;
    REQUIRE(r.level == 2 && r.correction == 1 && decrypt_slots(F.ctx, r, F.sk) == want);
    F.ctx.sub_plain(r, b, pt);
    for (uint32_t i = 0; i < F.n; i++) want[i] = (z[i] + F.t - p[i]) % F.t;
    REQUIRE(decrypt_slots(F.ctx, r, F.sk) == want);
    F.ctx.multiply_plain(r, b, pt);
    for (uint32_t i = 0; i < F.n; i++) want[i] = mulm(z[i], p[i], F.t);
    REQUIRE(r.level == 2 && r.correction == b.correction && decrypt_slots(F.ctx, r, F.sk) == want);
    REQUIRE(decrypt_slots(F.ctx, b, F.sk) == z);                       // the operands are read only

    Ciphertext top; F.encrypt(top, x);
    REQUIRE(throws([&] { F.ctx.add(s, top, b); }));
    REQUIRE(throws([&] { F.ctx.sub(s, top, b); }));
    REQUIRE(throws([&] { F.ctx.multiply(s, top, b, F.rlk); }));
    delete pt.poly;
    free_ct(cx); free_ct(cy); free_ct(a); free_ct(b); free_ct(s); free_ct(r); free_ct(top);
}

static void test_second_field() {
    std::cout << "Testing multiply -> switch -> decrypt on 4 x 40-bit primes..." << std::endl;
    const uint32_t n = 2048;
    uint64_t primes[4];
    check(fhe_find_ntt_primes(40, n, 4, primes), "prime search");
    std::vector<uint256_t> moduli;
    for (uint64_t q : primes) moduli.emplace_back(q);
    Fixture F(SecurityParams{128, n, 160, 3.2f, 64}, moduli);
    REQUIRE(F.ctx.params().rns_ntt->width_class() == FHE_WIDTH_52);
    const std::vector<uint64_t> x = F.values(7, 1), y = F.values(13, 5);
    Ciphertext a, b, p;
    F.encrypt(a, x); F.encrypt(b, y);
    F.ctx.multiply(p, a, b, F.rlk);
    const float before = F.ctx.estimate_noise_budget(p, F.sk);
    F.ctx.mod_switch_to_next(p);
    const float after = F.ctx.estimate_noise_budget(p, F.sk);
    std::cout << "  budget " << before << " at level 0, " << after << " at level 1" << std::endl;
    REQUIRE(p.level == 1 && after > 0);
    std::vector<uint64_t> want(n);
    for (uint32_t i = 0; i < n; i++) want[i] = mulm(x[i], y[i], F.t);
    REQUIRE(decrypt_slots(F.ctx, p, F.sk) == want);
    Ciphertext sq;                                                     // and the level-1 keys (3 limbs x 3 digits of the 4 x 3 rows)
    F.ctx.multiply(sq, p, p, F.rlk);
    for (uint32_t i = 0; i < n; i++) want[i] = mulm(want[i], want[i], F.t);
    REQUIRE(sq.level == 1 && decrypt_slots(F.ctx, sq, F.sk) == want);
    free_ct(a); free_ct(b); free_ct(p); free_ct(sq);
}

int main(int argc, char **argv) {
    test_host();
    if (argc > 1 && !std::strcmp(argv[1], "--host-only")) { std::cout << "host-only: PASSED" << std::endl; return 0; }
    int count = 0;
    check(fhe_hip_device_count(&count), "device count");
    REQUIRE(count > 0);
    {
        Fixture F(SecurityParams{128, 2048, 180, 3.2f, 64});
        REQUIRE(F.t == 65537);
        test_every_level(F);
        test_depth3(F);
        test_rotations_at_level_2(F);
        test_corrections_and_levels(F);
    }
    test_second_field();
    std::cout << "ALL PASSED" << std::endl;
    return 0;
}
