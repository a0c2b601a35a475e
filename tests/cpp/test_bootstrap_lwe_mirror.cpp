// test_bootstrap_lwe_mirror.cpp -- FHEContext::bootstrap_lwe (include/fhe/fhe.hpp: fhe_lwe_prepare_accumulator -> fhe_blind_rotate ->
// fhe_rns_rescale_drop_last down to one prime -> fhe_rlwe_sample_extract -> fhe_lwe_keyswitch) called twice in a row on the same ciphertexts:
// LWE ciphertexts of m under z in, LWE ciphertexts of f(m) under z out, those in again, LWE ciphertexts of g(f(m)) under z out.  n = 2048,
// 2 x 30-bit primes, RGSW w = 16, key switch w = 8, n_lwe = 12, p = 8, batch 4; both test vectors carry the half-slot offset,
// tv[i] = Delta f(floor(i p / n)) + Delta / 2, so the phase of an output under z sits in the middle of slot f(m) of width Delta_1 = floor(q_0 / (2p)).
// Also with the modulus switch in the key-switch launch (q_out = 2^32 between the two calls), and a foreign BootstrapKey is refused.
//   ./test_bootstrap_lwe_mirror              the scenario on the GPU
//   ./test_bootstrap_lwe_mirror --host-only  links and checks the new entry points' null-handle rejection (no device)
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
    fhe_lwe_ksk_t *out = reinterpret_cast<fhe_lwe_ksk_t *>(0x1234);
    const int32_t z[1] = {1}; const uint64_t seeds[2] = {1, 2};
    REQUIRE(fhe_lwe_ksk_generate(nullptr, nullptr, 8, 1, z, 1, 3.2, seeds, &out) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_lwe_ksk_create(nullptr, &out, 8, 1, nullptr) == FHE_ERR_INVALID_ARG);
    REQUIRE(out == reinterpret_cast<fhe_lwe_ksk_t *>(0x1234));
    REQUIRE(fhe_lwe_ksk_export(nullptr, nullptr, nullptr) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_lwe_keyswitch(nullptr, nullptr, 0, nullptr, nullptr, 1) == FHE_ERR_INVALID_ARG);
    REQUIRE(fhe_lwe_ksk_destroy(nullptr) == FHE_OK);
    BootstrapKey empty;
    REQUIRE(empty.lwe_ksk == nullptr && empty.ks_decomp_bits == 8);
}

// the slot of an LWE ciphertext (a_0 .. a_{n_lwe-1}, b) under z modulo q: floor(((b + sum a_i z_i) mod q) / slot_width) mod 2p, and how far
// the phase is from the middle of its slot
static uint32_t slot_of(const uint64_t *ct, const std::vector<int32_t> &z, uint64_t q, uint64_t width, uint32_t p, uint64_t *off_centre) {
    uint64_t phase = ct[z.size()] % q;
    for (size_t i = 0; i < z.size(); i++) { REQUIRE(ct[i] < q); if (z[i]) phase = (phase + ct[i]) % q; }
    const uint64_t slot = phase / width, mid = slot * width + width / 2;
    *off_centre = phase > mid ? phase - mid : mid - phase;
    return (uint32_t)(slot % (2 * p));
}

int main(int argc, char **argv) {
    test_host();
    if (argc > 1 && !std::strcmp(argv[1], "--host-only")) { std::cout << "host-only: PASSED" << std::endl; return 0; }
    int count = 0;
    check(fhe_hip_device_count(&count), "device count");
    REQUIRE(count > 0);
    std::cout << "Testing bootstrap_key_gen / bootstrap_lwe..." << std::endl;
    FHEContext ctx(SecurityParams{128, 2048, 60, 3.2f, 64});
    const uint32_t n = ctx.params().n, L = ctx.num_levels(), n_lwe = 12, p = 8, batch = 4;
    REQUIRE(n == 2048 && L == 2);
    const uint64_t q_lwe = 1ull << 32, q[2] = {ctx.params().rns_moduli[0].limbs[0], ctx.params().rns_moduli[1].limbs[0]};
    const u128 Q = (u128)q[0] * q[1], delta = Q / (2 * p);
    PublicKey pk; SecretKey sk;
    ctx.keygen(pk, sk);

    uint64_t seed = 91;
    auto next = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return seed >> 20; };
    std::vector<int32_t> z(n_lwe);
    for (int32_t &b : z) b = (int32_t)(next() & 1);
    BootstrapKey bk;
    ctx.bootstrap_key_gen(bk, sk, z, 16, 8);
    REQUIRE(bk.rows_c0.size() == n_lwe && bk.rows_c1.size() == n_lwe && bk.decomp_bits == 16 && bk.lwe_ksk && bk.ks_decomp_bits == 8);
    uint64_t key_bytes = 0;
    check(fhe_lwe_ksk_bytes(bk.lwe_ksk, &key_bytes), "lwe_ksk_bytes");
    REQUIRE(key_bytes == (uint64_t)n * 4 * 64 * 8);                      // K = ceil(30 / 8) = 4 rows per coefficient, 13 columns padded to 64
    {   // a key in a context that did not make it is refused, and nothing is written
        FHEContext other(SecurityParams{128, 2048, 60, 3.2f, 64});
        Polynomial *tv = other.new_polynomial(); std::vector<uint64_t> o, in(n_lwe + 1, 0);
        bool threw = false;
        try { other.bootstrap_lwe(o, in, q_lwe, *tv, bk); } catch (const std::runtime_error &) { threw = true; }
        REQUIRE(threw && o.empty());
        BootstrapKey none; threw = false;
        try { ctx.bootstrap_lwe(o, in, q_lwe, *tv, none); } catch (const std::runtime_error &) { threw = true; }
        REQUIRE(threw && o.empty());
        delete tv;
    }

    const uint32_t msgs[batch] = {0, 3, 5, 7};
    std::vector<uint64_t> lwe((size_t)batch * (n_lwe + 1));
    for (uint32_t b = 0; b < batch; b++) {
        uint64_t acc = 0;
        for (uint32_t i = 0; i < n_lwe; i++) { const uint64_t a = next() % q_lwe; lwe[(size_t)b * (n_lwe + 1) + i] = a; if (z[i]) acc = (acc + a) % q_lwe; }
        const uint64_t phase = msgs[b] * (q_lwe / (2 * p)) + q_lwe / (4 * p) + next() % 1000;
        lwe[(size_t)b * (n_lwe + 1) + n_lwe] = (phase + q_lwe - acc) % q_lwe;
    }
    const uint32_t f[8] = {5, 1, 7, 0, 3, 3, 6, 2}, g[8] = {2, 7, 1, 1, 6, 0, 4, 3};
    auto test_vector = [&](const uint32_t *table) {
        std::vector<uint256_t> htv((size_t)L * n);
        for (uint32_t l = 0; l < L; l++) for (uint32_t i = 0; i < n; i++) htv[(size_t)l * n + i] = uint256_t((uint64_t)((delta * table[(size_t)i * p / n] + delta / 2) % q[l]));
        Polynomial *tv = ctx.new_polynomial();
        copy_to_device(tv->coeffs, htv.data(), htv.size());
        return tv;
    };
    Polynomial *tv_f = test_vector(f), *tv_g = test_vector(g);
    // q_mid: the modulus between the two calls -- q_0 itself (q_out = 0) or 2^32 by the fused modulus switch
    for (uint64_t q_out : {(uint64_t)0, (uint64_t)1 << 32}) {
        const uint64_t q_mid = q_out ? q_out : q[0];
        std::vector<uint64_t> mid, fin;
        ctx.bootstrap_lwe(mid, lwe, q_lwe, *tv_f, bk, q_out);
        REQUIRE(mid.size() == lwe.size());
        ctx.bootstrap_lwe(fin, mid, q_mid, *tv_g, bk);                   // the first call's output is the second call's input
        REQUIRE(fin.size() == lwe.size());
        uint64_t worst_mid = 0, worst_fin = 0;
        for (uint32_t b = 0; b < batch; b++) {
            uint64_t off = 0;
            REQUIRE(slot_of(mid.data() + (size_t)b * (n_lwe + 1), z, q_mid, q_mid / (2 * p), p, &off) == f[msgs[b]]);
            REQUIRE(off < q_mid / (8 * p));                              // within a quarter slot of the middle
            if (off > worst_mid) worst_mid = off;
            REQUIRE(slot_of(fin.data() + (size_t)b * (n_lwe + 1), z, q[0], q[0] / (2 * p), p, &off) == g[f[msgs[b]]]);
            REQUIRE(off < q[0] / (8 * p));
            if (off > worst_fin) worst_fin = off;
        }
        int bm = 0, bf = 0; for (uint64_t e = worst_mid; e; e >>= 1) bm++; for (uint64_t e = worst_fin; e; e >>= 1) bf++;
        std::cout << "  between the calls modulo " << (q_out ? "2^32" : "q_0") << ": every output decrypts to f(m), then to g(f(m)); off-centre " << bm << " and " << bf
                  << " bits" << std::endl;
    }
    delete tv_f; delete tv_g;
    delete sk.sk; delete pk.pk0; delete pk.pk1;
    std::cout << "ALL PASSED" << std::endl;
    return 0;
}
