// test_bootstrap_mirror.cpp -- FHEContext::bootstrap_key_gen + blind_rotate_lwe (include/fhe/fhe.hpp: fhe_rgsw_keys_generate, then
// fhe_lwe_prepare_accumulator -> fhe_blind_rotate -> fhe_rlwe_sample_extract): LWE ciphertexts of m in, LWE samples of f(m) under the ring key
// out.  n = 2048, 2 x 30-bit primes, w = 16, n_lwe = 12, p = 8, q_lwe = 2^32, batch 4; tv[i] = Delta f(floor(i p / n)), Delta = floor(Q / (2p)); the
// phase of every output, CRT-centred, is within Delta / 2 of Delta f(m), for f = identity and for a table.
//   ./test_bootstrap_mirror              the scenario on the GPU
//   ./test_bootstrap_mirror --host-only  links and checks the new entry points' null-handle rejection (no device)
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
    fhe_relin_keys_t *o0[1] = {reinterpret_cast<fhe_relin_keys_t *>(0x1234)}, *o1[1] = {reinterpret_cast<fhe_relin_keys_t *>(0x5678)};
    const int32_t mu[1] = {1}; const uint64_t seeds[2] = {1, 2};
    REQUIRE(fhe_rgsw_keys_generate(nullptr, nullptr, 16, mu, 1, 1, 3.2, seeds, o0, o1) == FHE_ERR_INVALID_ARG);
    REQUIRE(o0[0] == reinterpret_cast<fhe_relin_keys_t *>(0x1234) && o1[0] == reinterpret_cast<fhe_relin_keys_t *>(0x5678));
    REQUIRE(fhe_lwe_prepare_accumulator(nullptr, 1ull << 32, 1, nullptr, nullptr, nullptr, nullptr, nullptr, 1) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_rlwe_sample_extract(nullptr, nullptr, nullptr, nullptr, 0, 1) == FHE_ERR_INVALID_ARG);
}

static uint64_t pow_mod_u64(uint64_t b, uint64_t e, uint64_t m) { uint64_t r = 1; b %= m; for (; e; e >>= 1) { if (e & 1) r = (uint64_t)((u128)r * b % m); b = (uint64_t)((u128)b * b % m); } return r; }

int main(int argc, char **argv) {
    test_host();
    if (argc > 1 && !std::strcmp(argv[1], "--host-only")) { std::cout << "host-only: PASSED" << std::endl; return 0; }
    int count = 0;
    check(fhe_hip_device_count(&count), "device count");
    REQUIRE(count > 0);
    std::cout << "Testing bootstrap_key_gen / blind_rotate_lwe..." << std::endl;
    FHEContext ctx(SecurityParams{128, 2048, 60, 3.2f, 64});
    const uint32_t n = ctx.params().n, L = ctx.num_levels(), n_lwe = 12, p = 8, batch = 4;
    REQUIRE(n == 2048 && L == 2);
    const uint64_t q_lwe = 1ull << 32, q[2] = {ctx.params().rns_moduli[0].limbs[0], ctx.params().rns_moduli[1].limbs[0]};
    const u128 Q = (u128)q[0] * q[1], delta = Q / (2 * p);
    PublicKey pk; SecretKey sk;
    ctx.keygen(pk, sk);
    std::vector<uint256_t> hs((size_t)L * n);
    copy_to_host(hs.data(), sk.sk->coeffs, hs.size());
    std::vector<int> s(n);
    for (uint32_t i = 0; i < n; i++) { const uint64_t v = hs[i].limbs[0]; REQUIRE(v <= 1 || v == q[0] - 1); s[i] = v == q[0] - 1 ? -1 : (int)v; }

    uint64_t seed = 77;
    auto next = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return seed >> 20; };
    std::vector<int32_t> z(n_lwe);
    for (int32_t &b : z) b = (int32_t)(next() & 1);
    BootstrapKey bk;
    ctx.bootstrap_key_gen(bk, sk, z, 16);
    REQUIRE(bk.rows_c0.size() == n_lwe && bk.rows_c1.size() == n_lwe && bk.decomp_bits == 16);
    {   // a ternary secret is refused; so is a key in a context that did not make it
        BootstrapKey bad; bool threw = false;
        try { ctx.bootstrap_key_gen(bad, sk, std::vector<int32_t>{1, -1, 0}, 16); } catch (const std::runtime_error &) { threw = true; }
        REQUIRE(threw && bad.rows_c0.empty());
        FHEContext other(SecurityParams{128, 2048, 60, 3.2f, 64});
        Polynomial *p = other.new_polynomial(); std::vector<uint64_t> o, in(n_lwe + 1, 0);
        threw = false;
        try { other.blind_rotate_lwe(o, in, 1ull << 32, *p, bk, 0); } catch (const std::runtime_error &) { threw = true; }
        REQUIRE(threw && o.empty());
        delete p;
    }

    const uint32_t msgs[batch] = {0, 3, 5, 7};
    std::vector<uint64_t> lwe((size_t)batch * (n_lwe + 1));
    for (uint32_t b = 0; b < batch; b++) {
        uint64_t acc = 0;
        for (uint32_t i = 0; i < n_lwe; i++) { const uint64_t a = next() % q_lwe; lwe[(size_t)b * (n_lwe + 1) + i] = a; if (z[i]) acc = (acc + a) % q_lwe; }
        const uint64_t phase = msgs[b] * (q_lwe / (2 * p)) + q_lwe / (4 * p) + next() % 1000;
        lwe[(size_t)b * (n_lwe + 1) + n_lwe] = (phase + q_lwe - acc) % q_lwe;
    }
    const uint32_t tables[2][8] = {{0, 1, 2, 3, 4, 5, 6, 7}, {5, 1, 7, 0, 3, 3, 6, 2}};
    for (const auto &f : tables) {
        std::vector<uint256_t> htv((size_t)L * n);
        for (uint32_t l = 0; l < L; l++) for (uint32_t i = 0; i < n; i++) htv[(size_t)l * n + i] = uint256_t((uint64_t)(delta * f[(size_t)i * p / n] % q[l]));
        Polynomial *tv = ctx.new_polynomial();
        copy_to_device(tv->coeffs, htv.data(), htv.size());
        std::vector<uint64_t> out;
        ctx.blind_rotate_lwe(out, lwe, q_lwe, *tv, bk, 0);
        REQUIRE(out.size() == (size_t)batch * L * (n + 1));
        u128 worst = 0;
        for (uint32_t b = 0; b < batch; b++) {
            u128 v = 0;
            for (uint32_t l = 0; l < L; l++) {
                const uint64_t *row = out.data() + ((size_t)b * L + l) * (n + 1);
                uint64_t r = row[n] % q[l];
                for (uint32_t j = 0; j < n; j++) { REQUIRE(row[j] < q[l]); if (s[j] == 1) r = (r + row[j]) % q[l]; else if (s[j] == -1) r = (r + q[l] - row[j]) % q[l]; }
                const uint64_t Ql = q[1 - l], inv = pow_mod_u64(Ql % q[l], q[l] - 2, q[l]);
                v = (v + (u128)((u128)r * inv % q[l]) * Ql) % Q;
            }
            const u128 want = delta * f[msgs[b]], d = v > want ? v - want : want - v, err = d < Q - d ? d : Q - d;      // centred modulo Q
            if (err > worst) worst = err;
            REQUIRE(err < delta / 2);
        }
        int bits = 0; for (u128 e = worst; e; e >>= 1) bits++;
        std::cout << "  f(0..7) = " << f[0] << f[1] << f[2] << f[3] << f[4] << f[5] << f[6] << f[7] << ": every phase within Delta / 2 of Delta f(m); noise " << bits << " bits" << std::endl;
        delete tv;
    }
    delete sk.sk; delete pk.pk0; delete pk.pk1;
    std::cout << "ALL PASSED" << std::endl;
    return 0;
}
