// test_ct_bootstrap_mirror.cpp -- FHEContext::bootstrap(Ciphertext&) (include/fhe/fhe.hpp: fhe_rns_rescale_drop_last down to one prime ->
// fhe_rlwe_sample_extract_strided -> fhe_lwe_keyswitch -> fhe_lwe_prepare_accumulator -> fhe_blind_rotate -> fhe_rlwe_pack) on a ciphertext whose
// four coefficients i n / 4 carry Delta m_i + Delta / 2: it comes back at level 0 with correction 1, those coefficients decode to f(m_i) and every
// other one to 0; bootstrapped again with g, to g(f(m_i)).  n = 2048, 2 x 30-bit primes, plaintext modulus 2 (the keys then carry noise 2 e),
// RGSW w = 16, key switch w = 8, packing keys w = 16, n_lwe = 12, p = 8, q_lwe = 2^32; both ciphertexts together cover all 8 messages.  The raw
// phase comes from fhe_ct_decrypt with t = 2^63.  A foreign key, a 3-component ciphertext and a bad count throw and leave the ciphertext alone.
//   ./test_ct_bootstrap_mirror              the scenario on the GPU
//   ./test_ct_bootstrap_mirror --host-only  links and checks the new entry points' null-handle rejection (no device)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <vector>

#include "fhe/fhe.hpp"

using namespace fhe;
typedef unsigned __int128 u128;

#define REQUIRE(cond)                                                                       \
    do {                                                                                    \
        if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static void test_host() {
    REQUIRE(fhe_rlwe_sample_extract_strided(nullptr, nullptr, nullptr, nullptr, 1, 1) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_rlwe_pack(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, 1, 1) == FHE_ERR_INVALID_ARG);
}

// the centred phase of every coefficient of a level-0 ciphertext: fhe_ct_decrypt with t = 2^63 returns v mod 2^63, and |v| < Q / 2 < 2^59
static std::vector<int64_t> phases(FHEContext &ctx, const fhe_secret_key_t *key, const Ciphertext &ct) {
    const uint32_t n = ctx.params().n;
    void *d = nullptr; check(fhe_hip_malloc(&d, (size_t)n * 8), "malloc");
    const void *comps[2] = {ct.components[0]->coeffs, ct.components[1]->coeffs};
    check(fhe_ct_decrypt(ctx.params().rns_ntt->handle(), key, 1ull << 63, 1, (uint64_t *)d, nullptr, comps, 2, 1), "decrypt");
    check(fhe_hip_sync(), "sync");
    std::vector<uint64_t> raw(n);
    check(fhe_hip_memcpy_d2h(raw.data(), d, (size_t)n * 8), "memcpy d2h");
    check(fhe_hip_free(d), "free");
    std::vector<int64_t> v(n);
    for (uint32_t i = 0; i < n; i++) v[i] = raw[i] >= (1ull << 62) ? (int64_t)(raw[i] - (1ull << 63)) : (int64_t)raw[i];
    return v;
}

int main(int argc, char **argv) {
    test_host();
    if (argc > 1 && !std::strcmp(argv[1], "--host-only")) { std::cout << "host-only: PASSED" << std::endl; return 0; }
    int devices = 0;
    check(fhe_hip_device_count(&devices), "device count");
    REQUIRE(devices > 0);
    std::cout << "Testing FHEContext::bootstrap(Ciphertext&)..." << std::endl;
    FHEContext ctx(SecurityParams{128, 2048, 60, 3.2f, 64});
    ctx.set_plain_modulus(2);                                            // before key generation: every key carries noise 2 e
    const uint32_t n = ctx.params().n, L = ctx.num_levels(), n_lwe = 12, p = 8, count = 4, step = n / count;
    REQUIRE(n == 2048 && L == 2);
    const uint64_t q_lwe = 1ull << 32, q[2] = {ctx.params().rns_moduli[0].limbs[0], ctx.params().rns_moduli[1].limbs[0]};
    const u128 Q = (u128)q[0] * q[1];
    const int64_t delta = (int64_t)(Q / (2 * p));
    PublicKey pk; SecretKey sk;
    ctx.keygen(pk, sk);
    fhe_secret_key_t *key = nullptr;
    check(fhe_secret_key_create(ctx.params().rns_ntt->handle(), &key, sk.sk->coeffs), "secret key import");

    uint64_t seed = 123;
    auto next = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return seed >> 20; };
    std::vector<int32_t> z(n_lwe);
    for (int32_t &b : z) b = (int32_t)(next() & 1);
    BootstrapKey bk; PackingKeys keys;
    ctx.bootstrap_key_gen(bk, sk, z, 16, 8);
    ctx.packing_key_gen(keys, sk, 16);
    REQUIRE(bk.lwe_ksk && keys.sets.size() == 11);

    const uint32_t f[8] = {5, 1, 7, 0, 3, 3, 6, 2}, g[8] = {2, 7, 1, 1, 6, 0, 4, 3};
    auto upload = [&](const std::vector<int64_t> &values) {              // non-negative integers below Q -> one level-0 polynomial
        std::vector<uint256_t> host((size_t)L * n);
        for (uint32_t l = 0; l < L; l++) for (uint32_t i = 0; i < n; i++) host[(size_t)l * n + i] = uint256_t((uint64_t)values[i] % q[l]);
        Polynomial *poly = ctx.new_polynomial();
        copy_to_device(poly->coeffs, host.data(), host.size());
        return poly;
    };
    auto test_vector = [&](const uint32_t *table, bool offset) {
        std::vector<int64_t> tv(n);
        for (uint32_t i = 0; i < n; i++) tv[i] = delta * table[(size_t)i * p / n] + (offset ? delta / 2 : 0);
        return upload(tv);
    };
    Polynomial *tv_f = test_vector(f, true), *tv_g = test_vector(g, false);
    auto decode = [&](int64_t v) { return (uint32_t)((((2 * v + delta) / (2 * delta)) % (2 * p) + 2 * p) % (2 * p)); };

    const uint32_t msgs[2][4] = {{0, 3, 5, 7}, {1, 2, 4, 6}};
    for (int k = 0; k < 2; k++) {
        std::vector<int64_t> m(n, 0);
        for (uint32_t i = 0; i < count; i++) m[(size_t)i * step] = delta * msgs[k][i] + delta / 2;
        Plaintext pt; pt.poly = upload(m);
        Ciphertext ct; ctx.encrypt_ckks(ct, pt, 1.0, pk);
        ctx.bootstrap(ct, *tv_f, bk, keys, count, q_lwe);
        REQUIRE(ct.level == 0 && ct.correction == 1 && ct.components.size() == 2 && ct.components[0]->num_limbs == L);
        std::vector<int64_t> v = phases(ctx, key, ct);
        int64_t worst = 0;
        for (uint32_t x = 0; x < n; x++) {
            const int64_t want = x % step ? 0 : delta * f[msgs[k][x / step]] + delta / 2, err = v[x] > want ? v[x] - want : want - v[x];
            REQUIRE(err < delta / 2);                                    // the target coefficients sit mid-slot of f(m), the others decode to 0
            if (err > worst) worst = err;
        }
        for (uint32_t i = 0; i < count; i++) REQUIRE(v[(size_t)i * step] / delta == (int64_t)f[msgs[k][i]]);
        ctx.bootstrap(ct, *tv_g, bk, keys, count, q_lwe);                // the output is the input of the next call
        v = phases(ctx, key, ct);
        for (uint32_t x = 0; x < n; x++) REQUIRE(decode(v[x]) == (x % step ? 0 : g[f[msgs[k][x / step]]]));
        int bits = 0; for (int64_t e = worst; e; e >>= 1) bits++;
        std::cout << "  messages " << msgs[k][0] << msgs[k][1] << msgs[k][2] << msgs[k][3] << ": f(m), then g(f(m)); noise after the first call " << bits << " bits" << std::endl;

        // what must throw, with the ciphertext left alone
        const Polynomial *before0 = ct.components[0], *before1 = ct.components[1];
        auto throws = [&](auto &&fn) { try { fn(); } catch (const std::runtime_error &) { return true; } return false; };
        for (uint32_t bad : {0u, 3u, 2 * n}) REQUIRE(throws([&] { ctx.bootstrap(ct, *tv_g, bk, keys, bad, q_lwe); }));
        REQUIRE(throws([&] { ctx.bootstrap(ct, *tv_g, bk, keys, count, 0); }));                  // q_lwe outside [2, 2^48]
        BootstrapKey none; PackingKeys no_keys;
        REQUIRE(throws([&] { ctx.bootstrap(ct, *tv_g, none, keys, count, q_lwe); }));
        REQUIRE(throws([&] { ctx.bootstrap(ct, *tv_g, bk, no_keys, count, q_lwe); }));
        ct.components.push_back(ctx.new_polynomial());
        REQUIRE(throws([&] { ctx.bootstrap(ct, *tv_g, bk, keys, count, q_lwe); }));              // 3 components
        delete ct.components.back(); ct.components.pop_back();
        REQUIRE(ct.components[0] == before0 && ct.components[1] == before1 && ct.level == 0);
        if (k == 0) {                                                    // keys in a context that did not make them
            FHEContext other(SecurityParams{128, 2048, 60, 3.2f, 64});
            Ciphertext o; other.encrypt_ckks(o, pt, 1.0, pk);
            Polynomial *tv = other.new_polynomial();
            REQUIRE(throws([&] { other.bootstrap(o, *tv, bk, keys, count, q_lwe); }));
            delete tv; for (Polynomial *c : o.components) delete c;
        }
        delete pt.poly; for (Polynomial *c : ct.components) delete c;
    }
    delete tv_f; delete tv_g;
    check(fhe_secret_key_destroy(key), "secret key destroy");
    delete sk.sk; delete pk.pk0; delete pk.pk1;
    std::cout << "ALL PASSED" << std::endl;
    return 0;
}
