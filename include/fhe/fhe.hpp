// fhe/fhe.hpp -- mirror of the parts of fhe::FHEContext on the multiply path (include/fhe.cuh:15-148,
// src/fhe.cu:7-52,187-235): SecurityParams, SchemeParams, Ciphertext, RelinKeys, GaloisKeys, FHEContext::add /
// multiply / relinearize / rotate_rows / rotate_columns, and the scheme plumbing around them (key generation, slot encoding,
// encryption).  Bootstrapping is out of scope of this engine.
#pragma once
#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <complex>
#include <memory>
#include <random>
#include <vector>

#include "polynomial.hpp"

namespace fhe {

struct SecurityParams {          // include/fhe.cuh:15-21
    uint32_t lambda;
    uint32_t poly_degree;
    uint32_t log_q;
    float sigma;
    uint32_t hamming_weight;
};

struct PublicKey {                                            // include/fhe.cuh:41-44
    Polynomial *pk0; Polynomial *pk1;
    // engine-side copy for FHEContext::encrypt_fused (fhe_public_key_create), built on first use; shared, so that copies of the struct stay valid
    mutable std::shared_ptr<fhe_public_key_t> imported;
    mutable const void *imported_for = nullptr;
};
struct SecretKey {                                            // include/fhe.cuh:47-49
    Polynomial *sk;
    // engine-side copies for FHEContext::decrypt_fused / noise_budget_fused (fhe_secret_key_create), one per level (index = level), built on
    // first use: a level's key is the first L - level limbs of sk, imported through the same pointer; shared, so that copies of the struct stay valid
    mutable std::vector<std::shared_ptr<fhe_secret_key_t>> imported;
    mutable const void *imported_for = nullptr;
};
struct RelinKeys {                                            // include/fhe.cuh:52-55
    std::vector<PublicKey *> rlk_keys;     // level j*K + k: (b, a) with b = -a*s + e + g*s^2, g = 2^(k*w) in limb j, 0 elsewhere
    uint32_t decomp_bits = 16;
    // engine-side copy (NTT domain, packed for the fused key-switch kernel); built on first use
    mutable fhe_relin_keys_t *imported = nullptr;
    mutable const void *imported_for = nullptr;
    // the same rows imported on the engines of lower levels (index = level, entry 0 unused): derived by slicing, never regenerated
    mutable std::vector<fhe_relin_keys_t *> imported_levels;
    RelinKeys() = default;
    RelinKeys(const RelinKeys &) = delete;
    RelinKeys &operator=(const RelinKeys &) = delete;
    void drop_levels() const { for (fhe_relin_keys_t *k : imported_levels) fhe_relin_keys_destroy(k); imported_levels.clear(); }
    ~RelinKeys() { drop_levels(); fhe_relin_keys_destroy(imported); for (PublicKey *k : rlk_keys) { if (k) { delete k->pk0; delete k->pk1; delete k; } } }
};

struct GaloisKeys {                                           // include/fhe.cuh:58-61
    std::vector<PublicKey *> gal_keys;     // one block of L*K key rows per Galois element, in the order of `elements`: row j*K + k of the block for g
                                           // is (b, a) with b = -a*s + e + g_{j,k} * sigma_g(s) (the relinearisation-key layout with sigma_g(s) for s^2)
    std::vector<uint32_t> elements;        // the Galois elements the blocks were made for (odd, below 2n)
    uint32_t decomp_bits = 16;
    // engine-side copies (one imported key set per element, NTT domain, packed for the fused key switch); built on first use
    mutable std::vector<fhe_relin_keys_t *> imported;
    mutable const void *imported_for = nullptr;
    mutable std::vector<std::vector<fhe_relin_keys_t *>> imported_levels;   // [level][element], entry 0 unused: sliced from the same rows
    GaloisKeys() = default;
    GaloisKeys(const GaloisKeys &) = delete;
    GaloisKeys &operator=(const GaloisKeys &) = delete;
    void drop_levels() const { for (auto &lv : imported_levels) for (fhe_relin_keys_t *k : lv) fhe_relin_keys_destroy(k); imported_levels.clear(); }
    ~GaloisKeys() {
        drop_levels();
        for (fhe_relin_keys_t *k : imported) fhe_relin_keys_destroy(k);
        for (PublicKey *k : gal_keys) { if (k) { delete k->pk0; delete k->pk1; delete k; } }
    }
};

// The key of FHEContext::bootstrap / blind_rotate (include/fhe.cuh:119, 139, declared only): one RGSW encryption under the ring key per
// element of the LWE secret, each two engine-side row sets (fhe_rgsw_keys_generate), in the order fhe_blind_rotate takes them, and the LWE
// key-switching key from the ring key (first prime) back to the LWE secret (fhe_lwe_ksk_generate), which has a digit width of its own
struct BootstrapKey {
    std::vector<fhe_relin_keys_t *> rows_c0, rows_c1;
    uint32_t decomp_bits = 16;
    fhe_lwe_ksk_t *lwe_ksk = nullptr;      // n K rows of n_lwe + 1 residues modulo the first prime (FHEContext::bootstrap_lwe)
    uint32_t ks_decomp_bits = 8;
    const void *made_for = nullptr;        // the engine whose handles these are (FHEContext::blind_rotate_lwe / bootstrap_lwe refuse another context's key)
    BootstrapKey() = default;
    BootstrapKey(const BootstrapKey &) = delete;
    BootstrapKey &operator=(const BootstrapKey &) = delete;
    void clear() {
        for (auto *v : {&rows_c0, &rows_c1}) { for (fhe_relin_keys_t *k : *v) fhe_relin_keys_destroy(k); v->clear(); }
        fhe_lwe_ksk_destroy(lwe_ksk); lwe_ksk = nullptr;
    }
    ~BootstrapKey() { clear(); }
};

// The Galois keys of 2^j + 1, j = 1 .. log2 n, that pack LWE samples back into one ciphertext (FHEContext::packing_key_gen / pack_lwes)
struct PackingKeys {
    std::vector<fhe_relin_keys_t *> sets;  // sets[j - 1]: the keys of 2^j + 1
    uint32_t decomp_bits = 16;
    const void *made_for = nullptr;        // the engine whose handles these are (FHEContext::pack_lwes refuses another context's keys)
    PackingKeys() = default;
    PackingKeys(const PackingKeys &) = delete;
    PackingKeys &operator=(const PackingKeys &) = delete;
    void clear() { for (fhe_relin_keys_t *k : sets) fhe_relin_keys_destroy(k); sets.clear(); }
    ~PackingKeys() { clear(); }
};

// The engine-side object of FHEContext::multiply_bfv (fhe_bfv_multiplier_create): the extended engine on Q u P and the tables of the exact
// lift and scale-and-round, for the context's level-0 basis and plaintext modulus.  FHEContext::bfv_multiplier_gen fills it; the context keeps
// one of its own for multiply_bfv.  Destroy it before the context.
struct BFVMultiplier {
    fhe_bfv_multiplier_t *handle = nullptr;
    std::vector<uint64_t> aux_moduli;      // the auxiliary primes P it was made with
    uint64_t t = 0;
    const void *made_for = nullptr;        // the engine whose multiplier this is
    BFVMultiplier() = default;
    BFVMultiplier(const BFVMultiplier &) = delete;
    BFVMultiplier &operator=(const BFVMultiplier &) = delete;
    void clear() { fhe_bfv_multiplier_destroy(handle); handle = nullptr; aux_moduli.clear(); made_for = nullptr; }
    ~BFVMultiplier() { clear(); }
};

struct Plaintext {                                            // include/fhe.cuh:72-75
    Polynomial *poly = nullptr;
    bool is_ntt_form = false;
};

// Levels.  Level l means the first L - l primes of the basis: a ciphertext at level l has components of L - l limbs and lives on the
// context's engine for those primes.  mod_switch_to_next moves it one level down and divides its noise by the dropped prime; the
// plaintext picks up the factor q_last^-1 mod t, which `correction` keeps: the ciphertext decrypts to correction * m mod t.
struct Ciphertext {                                           // include/fhe.cuh:63-69
    std::vector<Polynomial *> components;
    uint32_t level = 0;
    uint64_t correction = 1;
    float noise_budget = 0.f;
    bool is_ntt_form = false;
    double scale = 1.0;                    // CKKS (encrypt_ckks, rescale_to_next, decrypt_ckks): the plaintext is scale * m; the exact calls leave it alone
};

struct SchemeParams {                                         // include/fhe.cuh:24-38 (the parts that are used)
    SecurityParams security;
    uint32_t n;
    std::vector<uint256_t> rns_moduli;     // q = prod(rns_moduli); the reference hard-codes the even q = 2^60 (src/fhe.cu:13)
    uint64_t t = 65537;                    // plaintext modulus (src/fhe.cu:14); t = 1 (mod 2n) gives n SIMD slots
    RNS_NTTEngine *rns_ntt;
};

class FHEContext {
public:
    // Honours poly_degree and log_q (the reference ignores log_q): L = ceil(log_q / 30) NTT primes of
    // ceil(log_q / L) bits each, the smallest ones >= 2^(bits-1) with q = 1 (mod 2n).
    explicit FHEContext(const SecurityParams &params) {
        uint32_t L = std::max(1u, (params.log_q + 29) / 30);
        uint32_t bits = std::max(20u, (params.log_q + L - 1) / L);
        std::vector<uint64_t> primes(L);
        check(fhe_find_ntt_primes(bits, params.poly_degree, L, primes.data()), "FHEContext: prime search");
        std::vector<uint256_t> moduli;
        for (uint64_t p : primes) moduli.emplace_back(p);
        init(params, moduli);
    }
    // Explicit RNS basis (e.g. BASELINE config 4: N = 16384, 6 limbs).
    FHEContext(const SecurityParams &params, const std::vector<uint256_t> &rns_moduli) { init(params, rns_moduli); }
    ~FHEContext() { bfv_.clear(); delete params_.rns_ntt; }
    FHEContext(const FHEContext &) = delete;
    FHEContext &operator=(const FHEContext &) = delete;

    // a zeroed polynomial of level `level`: L - level limbs
    Polynomial *new_polynomial(uint32_t level = 0) const {
        return new Polynomial(params_.n, params_.rns_moduli[0], (uint32_t)params_.rns_moduli.size() - level);
    }
    uint32_t num_levels() const { return (uint32_t)params_.rns_moduli.size(); }               // levels 0 .. L - 1
    // the engine of a level (the first L - level primes), created on first use; level 0 is params().rns_ntt
    RNS_NTTEngine &engine(uint32_t level) {
        if (level >= num_levels()) throw std::runtime_error("FHEContext: no such level");
        if (!level) return *params_.rns_ntt;
        if (level_engines_.size() < num_levels()) level_engines_.resize(num_levels());
        if (!level_engines_[level])
            level_engines_[level].reset(new RNS_NTTEngine(params_.n, params_.rns_moduli.data(), num_levels() - level));
        return *level_engines_[level];
    }

    // src/fhe.cu:187-197
    // Operands must be at the same level (no automatic alignment).  With unequal corrections both operands are first brought to correction 1
    // on a copy (normalized()), which costs up to log2(t / 2) bits of noise; equal corrections are kept.
    void add(Ciphertext &result, const Ciphertext &a, const Ciphertext &b) {
        same_level(a, b, "FHEContext::add");
        if (a.correction != b.correction) {
            Ciphertext na, nb;
            const Ciphertext &x = normalized(na, a), &y = normalized(nb, b);
            add(result, x, y);
            device_synchronize();
            free_components(na); free_components(nb);
            return;
        }
        RNS_NTTEngine &E = engine(a.level);
        size_t num = std::max(a.components.size(), b.components.size());
        ensure_components(result, num, a.level);
        for (size_t i = 0; i < num; i++) {
            if (i < a.components.size() && i < b.components.size())
                E.add_rns(result.components[i]->coeffs, a.components[i]->coeffs, b.components[i]->coeffs);
            else {
                const Polynomial *src = i < a.components.size() ? a.components[i] : b.components[i];
                if (src != result.components[i])
                    check(fhe_hip_memcpy_d2d(result.components[i]->coeffs, src->coeffs, src->count() * sizeof(uint256_t)), "add copy");
            }
        }
        result.noise_budget = std::min(a.noise_budget, b.noise_budget);
        result.level = a.level; result.correction = a.correction;
    }
    // sub / add_plain / sub_plain / multiply_plain (include/fhe.cuh:98-104, declared only in the reference).  Plaintexts are the
    // encode()d polynomials (reduced mod t in every limb); with the mirror's BGV-style encryption c0 + c1*s = m + t*e they act
    // on the message directly: component-wise subtraction, +-pt on c0, every component times pt.
    void sub(Ciphertext &result, const Ciphertext &a, const Ciphertext &b) {
        if (a.components.size() != b.components.size()) throw std::runtime_error("FHEContext::sub: ciphertexts of different size");
        same_level(a, b, "FHEContext::sub");
        if (a.correction != b.correction) {
            Ciphertext na, nb;
            const Ciphertext &x = normalized(na, a), &y = normalized(nb, b);
            sub(result, x, y);
            device_synchronize();
            free_components(na); free_components(nb);
            return;
        }
        RNS_NTTEngine &E = engine(a.level);
        ensure_components(result, a.components.size(), a.level);
        for (size_t i = 0; i < a.components.size(); i++)
            E.sub_rns(result.components[i]->coeffs, a.components[i]->coeffs, b.components[i]->coeffs);
        result.noise_budget = std::min(a.noise_budget, b.noise_budget);
        result.level = a.level; result.correction = a.correction;
    }
    void add_plain(Ciphertext &result, const Ciphertext &ct, const Plaintext &pt) { plain_addsub(result, ct, pt, true); }
    void sub_plain(Ciphertext &result, const Ciphertext &ct, const Plaintext &pt) { plain_addsub(result, ct, pt, false); }
    // A level-l plaintext is the first L - l limbs of the encoded one: a contiguous prefix of its [L][n] buffer, used in place.  The product
    // keeps the correction of ct (correction * m * p); add_plain / sub_plain need correction 1 and normalise a copy of ct first (up to
    // log2(t / 2) bits of noise).
    void multiply_plain(Ciphertext &result, const Ciphertext &ct, const Plaintext &pt) {
        RNS_NTTEngine &E = engine(ct.level);
        ensure_components(result, ct.components.size(), ct.level);
        for (size_t i = 0; i < ct.components.size(); i++)
            E.multiply_rns(result.components[i]->coeffs, ct.components[i]->coeffs, pt.poly->coeffs);
        result.noise_budget = ct.noise_budget; result.level = ct.level; result.correction = ct.correction;
    }

    // src/fhe.cu:199-224: tensor product (4 forward + 3 inverse transforms instead of the reference's 8 + 4), then relinearisation.
    // With keys the two steps are ONE ABI call (fhe_ct_multiply_relin: c2 never leaves the library's workspace); with an empty
    // RelinKeys the result keeps its three components, as relinearize() does.
    void multiply(Ciphertext &result, const Ciphertext &a, const Ciphertext &b, const RelinKeys &rlk) {
        if (a.components.size() != 2 || b.components.size() != 2) throw std::runtime_error("FHEContext::multiply: 2-component ciphertexts expected");
        same_level(a, b, "FHEContext::multiply");
        const uint32_t level = a.level;
        const uint64_t corr = mul_mod_t(a.correction, b.correction);
        const float nb = a.noise_budget + b.noise_budget + 10;        // the reference's rough estimate (src/fhe.cu:222)
        RNS_NTTEngine &E = engine(level);
        if (rlk.rlk_keys.empty()) {
            ensure_components(result, 3, level);
            E.tensor_multiply(result.components[0]->coeffs, result.components[1]->coeffs, result.components[2]->coeffs,
                              a.components[0]->coeffs, a.components[1]->coeffs, b.components[0]->coeffs, b.components[1]->coeffs);
            device_synchronize();
        } else {
            fhe_relin_keys_t *keys = relin_keys_at(rlk, level);
            ensure_components(result, 2, level);
            while (result.components.size() > 2) { delete result.components.back(); result.components.pop_back(); }
            check(fhe_ct_multiply_relin(E.handle(), keys, result.components[0]->coeffs, result.components[1]->coeffs,
                                        a.components[0]->coeffs, a.components[1]->coeffs, b.components[0]->coeffs, b.components[1]->coeffs, 1),
                  "FHEContext::multiply");
            device_synchronize();
        }
        result.noise_budget = nb; result.level = level; result.correction = corr;
    }

    // src/fhe.cu:226-235 is a stub that drops c2 (which breaks decryption); docs/ARCHITECTURE.md:319-326 gives the
    // intended algorithm, implemented here as RNS digit decomposition + key switching (fhe_ct_relinearize).
    // With no keys (an empty RelinKeys) the ciphertext keeps its three components, so no information is lost.
    void relinearize(Ciphertext &ct, const RelinKeys &rlk) {
        if (ct.components.size() <= 2) return;                                              // src/fhe.cu:227
        if (rlk.rlk_keys.empty()) return;
        if (ct.components.size() != 3) throw std::runtime_error("FHEContext::relinearize: 3-component ciphertext expected");
        check(fhe_ct_relinearize(engine(ct.level).handle(), relin_keys_at(rlk, ct.level), ct.components[0]->coeffs, ct.components[1]->coeffs,
                                 ct.components[2]->coeffs, 1), "FHEContext::relinearize");
        device_synchronize();
        delete ct.components[2];
        ct.components.resize(2);                                                            // src/fhe.cu:234
    }

    // hands the key polynomials to the engine once (transformed and packed inside the library), cached in the RelinKeys object
    void import_relin_keys(const RelinKeys &rlk) {
        if (rlk.imported && rlk.imported_for == params_.rns_ntt) return;
        fhe_relin_keys_destroy(rlk.imported); rlk.imported = nullptr; rlk.drop_levels();
        std::vector<const void *> kb, ka;
        for (const PublicKey *k : rlk.rlk_keys) { kb.push_back(k->pk0->coeffs); ka.push_back(k->pk1->coeffs); }
        check(fhe_relin_keys_create(params_.rns_ntt->handle(), &rlk.imported, rlk.decomp_bits, kb.data(), ka.data(), (uint32_t)kb.size()),
              "FHEContext: relinearisation key import");
        rlk.imported_for = params_.rns_ntt;
    }

    // The imported key set for ciphertexts at `level`.  Level 0 is import_relin_keys.  Lower levels are DERIVED from the same rows: top-level
    // row j*K + k is (b, a) with the gadget 2^(kw) in limb j only, and the first L' = L - level limbs of a row are the level's row, so the
    // level's key set is rows j*K + k for j < L', k < K' (K' = digits per limb of the level's engine, K' <= K) through the same device pointers.
    fhe_relin_keys_t *relin_keys_at(const RelinKeys &rlk, uint32_t level) {
        import_relin_keys(rlk);
        if (!level) return rlk.imported;
        if (rlk.imported_levels.size() < num_levels()) rlk.imported_levels.resize(num_levels(), nullptr);
        if (!rlk.imported_levels[level]) {
            std::vector<const PublicKey *> rows(rlk.rlk_keys.begin(), rlk.rlk_keys.end());
            rlk.imported_levels[level] = import_sliced(rows.data(), rows.size(), rlk.decomp_bits, level);
        }
        return rlk.imported_levels[level];
    }

    // number of key levels relinkey_gen must produce for this context: L limbs x ceil(bits(q_max) / decomp_bits) digits
    uint32_t relin_levels(uint32_t decomp_bits) const {
        uint32_t K = 0;
        check(fhe_relin_num_digits(params_.rns_ntt->handle(), decomp_bits, &K), "relin_levels");
        return K * (uint32_t)params_.rns_moduli.size();
    }

    // FHEContext::relinkey_gen (src/fhe.cu:76-111): rlk[level] = (-a*s + e + g*s^2, a).  `a` uniform and `e` small are drawn
    // on the host from `rng` (a std::mt19937_64-like generator; the reference's device samplers are toys and out of
    // scope); the polynomial products run on the engine.  `noise_scale` multiplies e (1 = the reference's BFV-style
    // keys; t for BGV-style keys whose noise must vanish mod t).
    template <class Rng>
    void relinkey_gen(RelinKeys &rlk, const SecretKey &sk, uint32_t decomp_bits, Rng &rng, uint64_t noise_scale = 1, int noise_bound = 3) {
        rlk.decomp_bits = decomp_bits;
        std::unique_ptr<Polynomial> s2(new_polynomial());
        params_.rns_ntt->multiply_rns(s2->coeffs, sk.sk->coeffs, sk.sk->coeffs);             // s^2 (src/fhe.cu:80-81)
        keyswitch_rows(rlk.rlk_keys, *s2, sk, decomp_bits, rng, noise_scale, noise_bound);
    }

    // The L*K key rows that switch `target` (s^2, sigma_g(s)) to s: row j*K + k = (-a*s + e + g_{j,k} * target, a), g_{j,k} = 2^(k*w) in limb j.
    template <class Rng>
    void keyswitch_rows(std::vector<PublicKey *> &rows, const Polynomial &target, const SecretKey &sk, uint32_t decomp_bits, Rng &rng,
                        uint64_t noise_scale = 1, int noise_bound = 3) {
        const uint32_t L = (uint32_t)params_.rns_moduli.size(), n = params_.n, levels = relin_levels(decomp_bits), K = levels / L;
        RNS_NTTEngine &E = *params_.rns_ntt;
        std::unique_ptr<Polynomial> tmp(new_polynomial());
        std::vector<uint256_t> h_s2((size_t)L * n), h_a((size_t)L * n), h_e((size_t)L * n), h_g((size_t)L * n);
        device_synchronize();
        copy_to_host(h_s2.data(), target.coeffs, h_s2.size());
        for (uint32_t j = 0; j < L; j++)
            for (uint32_t k = 0; k < K; k++) {
                PublicKey *key = new PublicKey{new_polynomial(), new_polynomial()};
                std::fill(h_g.begin(), h_g.end(), uint256_t());
                const uint64_t qj = params_.rns_moduli[j].limbs[0];
                uint64_t g = 1;
                for (uint32_t i = 0; i < k * decomp_bits; i++) g = (g << 1) % qj;           // 2^(k*w) mod q_j  (src/fhe.cu:98)
                std::vector<int> e(n);
                for (uint32_t x = 0; x < n; x++) e[x] = (int)(rng() % (2 * noise_bound + 1)) - noise_bound;
                for (uint32_t l = 0; l < L; l++) {
                    const uint64_t q = params_.rns_moduli[l].limbs[0];
                    for (uint32_t x = 0; x < n; x++) {
                        h_a[(size_t)l * n + x] = uint256_t(rng() % q);
                        const uint64_t mag = (uint64_t)(e[x] < 0 ? -e[x] : e[x]) * (noise_scale % q) % q;
                        h_e[(size_t)l * n + x] = uint256_t(e[x] < 0 ? (q - mag) % q : mag);
                    }
                }
                for (uint32_t x = 0; x < n; x++)
                    h_g[(size_t)j * n + x] = uint256_t((uint64_t)((unsigned __int128)h_s2[(size_t)j * n + x].limbs[0] * g % qj));
                copy_to_device(key->pk1->coeffs, h_a.data(), h_a.size());
                E.multiply_rns(tmp->coeffs, key->pk1->coeffs, sk.sk->coeffs);                 // a*s (src/fhe.cu:104)
                copy_to_device(key->pk0->coeffs, h_e.data(), h_e.size());
                E.sub_rns(key->pk0->coeffs, key->pk0->coeffs, tmp->coeffs);                   // e - a*s (:105)
                copy_to_device(tmp->coeffs, h_g.data(), h_g.size());
                E.add_rns(key->pk0->coeffs, key->pk0->coeffs, tmp->coeffs);                   // + g*s^2 (:106) / + g*sigma_g(s)
                device_synchronize();
                rows.push_back(key);
            }
    }

    // ---- scheme plumbing: BGV-flavoured so that tensor product + relinearisation decrypt correctly --------
    // (the reference's keygen / encrypt / decrypt, src/fhe.cu:54-185, mix BFV scaling with an even modulus and call
    // undefined kernels; here noise is a multiple of t and plaintexts sit in the low bits: c0 + c1*s = m + t*e).
    // Sampling is done on the host with a seeded std::mt19937_64 (the reference's device samplers are toys, out of scope).
    void seed(uint64_t s) { rng_.seed(s); }
    // true: keygen / encrypt draw their polynomials with the DEVICE samplers below (seeds taken from the context's generator)
    void device_sampling(bool on) { device_sampling_ = on; }

    // FHEContext::sample_error_polynomial / sample_uniform_polynomial / sample_ternary_polynomial (src/fhe.cu:237-257) on the
    // device: discrete Gaussian of parameter security.sigma, uniform residues, ternary with P(nonzero) = 0.5 -- the
    // distributions the reference names (its kernels are placeholders or undefined; the literal placeholders are
    // fhe_sample_uniform_lcg / fhe_sample_gaussian_placeholder).  Seeds come from the context generator where the reference calls rand().
    void sample_error_polynomial(Polynomial &p) {
        check(fhe_rns_sample_gaussian(params_.rns_ntt->handle(), p.coeffs, (double)params_.security.sigma, rng_(), 1), "sample_error_polynomial");
    }
    void sample_uniform_polynomial(Polynomial &p) { check(fhe_rns_sample_uniform(params_.rns_ntt->handle(), p.coeffs, rng_(), 1), "sample_uniform_polynomial"); }
    void sample_ternary_polynomial(Polynomial &p) { check(fhe_rns_sample_ternary(params_.rns_ntt->handle(), p.coeffs, 0.5, rng_(), 1), "sample_ternary_polynomial"); }

    void keygen(PublicKey &pk, SecretKey &sk) {                                            // src/fhe.cu:54-74
        sk.sk = new_polynomial(); pk.pk0 = new_polynomial(); pk.pk1 = new_polynomial();
        sk.imported.clear();                                                                // engine-side copies of an earlier key
        draw_ternary(*sk.sk);                                                               // ternary secret (:57)
        draw_uniform(*pk.pk1);                                                              // :64
        std::unique_ptr<Polynomial> as(new_polynomial());
        params_.rns_ntt->multiply_rns(as->coeffs, pk.pk1->coeffs, sk.sk->coeffs);           // :71
        draw_scaled_error(*pk.pk0);                                                         // t*e (:67-68)
        params_.rns_ntt->sub_rns(pk.pk0->coeffs, pk.pk0->coeffs, as->coeffs);               // pk0 = t*e - pk1*sk (:72)
        device_synchronize();
    }

    void relinkey_gen(RelinKeys &rlk, const SecretKey &sk, uint32_t decomp_bits = 16) {    // src/fhe.cu:76 signature
        relinkey_gen(rlk, sk, decomp_bits, rng_, noise_scale());
    }

    // ---- Galois keys and slot rotations (include/fhe.cuh:58-61, 86, 112-116; declared, never defined in the reference) ------------------
    // Slot i of the encoding holds m(zeta_i), zeta_i = psi^(2i+1); sigma_g moves slot pi_g(i) to slot i, 2 pi_g(i) + 1 = g (2i + 1) (mod 2n).
    // Ordered as row 0: 2i+1 = 3^k, row 1: 2i+1 = -3^k (mod 2n), k = 0 .. n/2 - 1, rotate_rows(r) is a cyclic left shift by r of both rows
    // (g = 3^r) and rotate_columns swaps them (g = 2n - 1), as in SEAL; the natural slot order of encode() is a permutation of that order.

    // the Galois element of a row rotation by `steps` (mod n/2; negative steps: the inverse power)
    uint32_t galois_element(int steps) const {
        uint32_t g = 0;
        check(fhe_galois_element(params_.n, (int32_t)steps, &g), "FHEContext::galois_element");
        return g;
    }
    uint32_t column_element() const { return 2 * params_.n - 1; }

    // FHEContext::galoiskey_gen (include/fhe.cuh:86): the SEAL-style default set, row steps +-2^i for i = 0 .. log2(n/2) - 1 and the column element.
    void galoiskey_gen(GaloisKeys &gal_keys, const SecretKey &sk) {
        std::vector<int> steps;
        for (uint32_t s = 1; s < params_.n / 2; s <<= 1) { steps.push_back((int)s); steps.push_back(-(int)s); }
        galoiskey_gen(gal_keys, sk, steps, true, 16);
    }
    // Keys for the given row steps (and the column element when `columns`), digit width decomp_bits.  sigma_g(s) is computed on the engine
    // (fhe_rns_automorphism); noise as in relinkey_gen (times t).
    void galoiskey_gen(GaloisKeys &gal_keys, const SecretKey &sk, const std::vector<int> &steps, bool columns, uint32_t decomp_bits) {
        if (!gal_keys.gal_keys.empty() && gal_keys.decomp_bits != decomp_bits)
            throw std::runtime_error("FHEContext::galoiskey_gen: the key set already holds keys of another digit width");
        gal_keys.decomp_bits = decomp_bits;
        std::vector<uint32_t> elts;
        for (int st : steps) elts.push_back(galois_element(st));
        if (columns) elts.push_back(column_element());
        std::unique_ptr<Polynomial> sg(new_polynomial());
        for (uint32_t g : elts) {
            if (std::find(gal_keys.elements.begin(), gal_keys.elements.end(), g) != gal_keys.elements.end()) continue;
            check(fhe_rns_automorphism(params_.rns_ntt->handle(), sg->coeffs, sk.sk->coeffs, g, 1), "galoiskey_gen: sigma_g(s)");
            keyswitch_rows(gal_keys.gal_keys, *sg, sk, decomp_bits, rng_, params_.t);
            gal_keys.elements.push_back(g);
        }
    }

    // relinkey_gen / galoiskey_gen in ONE engine call each (fhe_keyswitch_keys_generate): a, e are drawn on the device with seeds from the
    // context generator, noise scale t, sigma = security.sigma.  The generated handles ARE the level-0 import (nothing is imported again); the
    // rows are read back with fhe_relin_keys_export, so that relin_keys_at / galois_keys_at slice lower levels as they do for host-made keys.
    // relinkey_gen / galoiskey_gen themselves stay as they are.
    void relinkey_gen_fused(RelinKeys &rlk, const SecretKey &sk, uint32_t decomp_bits = 16) {
        const uint32_t zero = 0;
        fhe_relin_keys_t *set = nullptr;
        generate_key_sets(sk, decomp_bits, &zero, 1, &set);
        for (PublicKey *k : rlk.rlk_keys) { if (k) { delete k->pk0; delete k->pk1; delete k; } }
        rlk.rlk_keys.clear(); rlk.drop_levels(); fhe_relin_keys_destroy(rlk.imported);
        rlk.decomp_bits = decomp_bits; rlk.imported = set; rlk.imported_for = params_.rns_ntt;
        rows_from_export(rlk.rlk_keys, set, relin_levels(decomp_bits));
    }
    // every element of (steps, columns) that gal_keys does not hold yet, ALL in one call
    void galoiskey_gen_fused(GaloisKeys &gal_keys, const SecretKey &sk, const std::vector<int> &steps, bool columns, uint32_t decomp_bits) {
        if (!gal_keys.gal_keys.empty() && gal_keys.decomp_bits != decomp_bits)
            throw std::runtime_error("FHEContext::galoiskey_gen_fused: the key set already holds keys of another digit width");
        std::vector<uint32_t> want, elts;
        for (int st : steps) want.push_back(galois_element(st));
        if (columns) want.push_back(column_element());
        for (uint32_t g : want)
            if (std::find(gal_keys.elements.begin(), gal_keys.elements.end(), g) == gal_keys.elements.end() && std::find(elts.begin(), elts.end(), g) == elts.end())
                elts.push_back(g);
        gal_keys.decomp_bits = decomp_bits;
        if (elts.empty()) return;
        import_galois_keys(gal_keys);                                                       // what it already holds (host-made rows), before the new handles join
        std::vector<fhe_relin_keys_t *> sets(elts.size(), nullptr);
        generate_key_sets(sk, decomp_bits, elts.data(), (uint32_t)elts.size(), sets.data());
        std::vector<PublicKey *> rows;
        try {
            for (fhe_relin_keys_t *set : sets) rows_from_export(rows, set, relin_levels(decomp_bits));
        } catch (...) {
            for (fhe_relin_keys_t *set : sets) fhe_relin_keys_destroy(set);
            for (PublicKey *k : rows) { delete k->pk0; delete k->pk1; delete k; }
            throw;
        }
        gal_keys.drop_levels();
        gal_keys.gal_keys.insert(gal_keys.gal_keys.end(), rows.begin(), rows.end());
        gal_keys.imported.insert(gal_keys.imported.end(), sets.begin(), sets.end());
        gal_keys.elements.insert(gal_keys.elements.end(), elts.begin(), elts.end());
        gal_keys.imported_for = params_.rns_ntt;
    }
    // Programmable bootstrapping around fhe_blind_rotate (FHEContext::bootstrap / blind_rotate, include/fhe.cuh:119, 139, declared only).
    // bootstrap_key_gen: RGSW encryptions of the LWE secret's bits under sk in ONE engine call; noise scale 1 (the blind rotation reads the
    // phase modulo Q: there is no plaintext modulus for the noise to be a multiple of), sigma = security.sigma, seeds from the context generator.
    // The LWE key-switching key back to the LWE secret comes from the same call, with its own digit width ks_decomp_bits (the RGSW width does
    // not fit its noise: DESIGN 4.16) and its own pair of seeds, drawn after the RGSW pair.
    void bootstrap_key_gen(BootstrapKey &bk, const SecretKey &sk, const std::vector<int32_t> &lwe_secret_bits, uint32_t decomp_bits = 16,
                           uint32_t ks_decomp_bits = 8) {
        if (lwe_secret_bits.empty()) throw std::runtime_error("FHEContext::bootstrap_key_gen: the LWE secret is empty");
        for (int32_t b : lwe_secret_bits)
            if (b != 0 && b != 1) throw std::runtime_error("FHEContext::bootstrap_key_gen: the LWE secret must be binary (a ternary secret needs two RGSW ciphertexts per element)");
        const uint64_t seeds[2] = {rng_(), rng_()}, ks_seeds[2] = {rng_(), rng_()};
        const uint32_t n_lwe = (uint32_t)lwe_secret_bits.size();
        std::vector<fhe_relin_keys_t *> r0(n_lwe, nullptr), r1(n_lwe, nullptr);
        check(fhe_rgsw_keys_generate(params_.rns_ntt->handle(), secret_key_at(sk, 0), decomp_bits, lwe_secret_bits.data(), n_lwe, 1,
                                     (double)params_.security.sigma, seeds, r0.data(), r1.data()), "FHEContext::bootstrap_key_gen");
        bk.clear();
        bk.rows_c0 = std::move(r0); bk.rows_c1 = std::move(r1); bk.decomp_bits = decomp_bits; bk.made_for = params_.rns_ntt;
        const int rc = fhe_lwe_ksk_generate(params_.rns_ntt->handle(), secret_key_at(sk, 0), ks_decomp_bits, n_lwe, lwe_secret_bits.data(), 1,
                                            (double)params_.security.sigma, ks_seeds, &bk.lwe_ksk);
        if (rc) { bk.clear(); bk.made_for = nullptr; check(rc, "FHEContext::bootstrap_key_gen: LWE key-switching key"); }
        bk.ks_decomp_bits = ks_decomp_bits;
    }
    // lwe: [batch][n_lwe + 1] values below q_lwe, (a_0 .. a_{n_lwe-1}, b) with phase b + sum a_i z_i, n_lwe = the size of the key; test_vector: one
    // top-level polynomial.  out_lwe: [batch][L][n + 1] residues, coefficient idx of X^(-phase~) test_vector as an LWE sample under the ring key
    // (fhe_lwe_prepare_accumulator -> fhe_blind_rotate -> fhe_rlwe_sample_extract on buffers owned by the call).
    void blind_rotate_lwe(std::vector<uint64_t> &out_lwe, const std::vector<uint64_t> &lwe, uint64_t q_lwe, const Polynomial &test_vector, const BootstrapKey &bk,
                          uint32_t idx = 0) {
        const uint32_t n_lwe = (uint32_t)bk.rows_c0.size(), n = params_.n, L = num_levels();
        if (!n_lwe || bk.rows_c1.size() != n_lwe) throw std::runtime_error("FHEContext::blind_rotate_lwe: the bootstrapping key is empty");
        if (bk.made_for != params_.rns_ntt) throw std::runtime_error("FHEContext::blind_rotate_lwe: the bootstrapping key was generated by another context");
        if (lwe.empty() || lwe.size() % (n_lwe + 1)) throw std::runtime_error("FHEContext::blind_rotate_lwe: lwe must hold batch x (n_lwe + 1) values");
        const uint32_t batch = (uint32_t)(lwe.size() / (n_lwe + 1));
        const size_t poly = (size_t)L * n, acc = poly * batch;                             // containers
        auto containers = [](size_t bytes) { return (bytes + sizeof(uint256_t) - 1) / sizeof(uint256_t); };
        const size_t lwe_c = containers(lwe.size() * 8), sh_c = containers((size_t)n_lwe * batch * 4), out_c = containers((size_t)batch * L * (n + 1) * 8);
        uint256_t *d = device_alloc(4 * acc + lwe_c + sh_c + out_c);
        try {
            uint256_t *a0 = d, *a1 = d + acc, *t0 = d + 2 * acc, *t1 = d + 3 * acc, *d_lwe = d + 4 * acc, *d_sh = d_lwe + lwe_c, *d_out = d_sh + sh_c;
            fhe_rns_ntt_t *h = params_.rns_ntt->handle();
            check(fhe_hip_memcpy_h2d(d_lwe, lwe.data(), lwe.size() * 8), "memcpy h2d");
            check(fhe_lwe_prepare_accumulator(h, q_lwe, n_lwe, (const uint64_t *)d_lwe, test_vector.coeffs, a0, a1, (uint32_t *)d_sh, batch), "blind_rotate_lwe: prepare");
            check(fhe_blind_rotate(h, bk.rows_c0.data(), bk.rows_c1.data(), n_lwe, a0, a1, (const uint32_t *)d_sh, t0, t1, batch), "blind_rotate_lwe: blind rotation");
            check(fhe_rlwe_sample_extract(h, (uint64_t *)d_out, a0, a1, idx, batch), "blind_rotate_lwe: sample extraction");
            device_synchronize();
            out_lwe.resize((size_t)batch * L * (n + 1));
            check(fhe_hip_memcpy_d2h(out_lwe.data(), d_out, out_lwe.size() * 8), "memcpy d2h");
        } catch (...) { device_free(d); throw; }
        device_free(d);
    }

    // The way back from LWE samples to a ciphertext (fhe_lwe_pack; the last step of FHEContext::bootstrap(Ciphertext&) below, which packs
    // straight from the accumulators).  packing_key_gen: the log2(n) Galois key sets of 2^j + 1 in ONE engine call, noise scale t like every key of the context.
    void packing_key_gen(PackingKeys &pk, const SecretKey &sk, uint32_t decomp_bits = 16) {
        uint32_t log_n = 0; while ((1u << log_n) < params_.n) log_n++;
        std::vector<uint32_t> elts(log_n);
        check(fhe_lwe_pack_galois_elements(params_.n, elts.data()), "FHEContext::packing_key_gen");
        std::vector<fhe_relin_keys_t *> sets(log_n, nullptr);
        generate_key_sets(sk, decomp_bits, elts.data(), log_n, sets.data());
        pk.clear();
        pk.sets = std::move(sets); pk.decomp_bits = decomp_bits; pk.made_for = params_.rns_ntt;
    }
    // lwe: [count][L][n + 1] residues, samples under the ring key at level 0 (what blind_rotate_lwe or fhe_rlwe_sample_extract leaves).  out is a
    // level-0 ciphertext whose coefficient i (n / count) carries the phase of sample i: exactly with normalize (correction 1), times F = n (trace) or
    // count (no trace) without, which out.correction records as F mod t, so that decrypt_fused divides it out.  With the trace every other
    // coefficient is 0.
    void pack_lwes(Ciphertext &out, const PackingKeys &pk, const std::vector<uint64_t> &lwe, uint32_t count, bool trace = true, bool normalize = true) {
        const uint32_t n = params_.n, L = num_levels();
        if (pk.made_for != params_.rns_ntt) throw std::runtime_error("FHEContext::pack_lwes: the packing keys were generated by another context");
        if (!count || lwe.size() != (size_t)count * L * (n + 1)) throw std::runtime_error("FHEContext::pack_lwes: lwe must hold count x L x (n + 1) values");
        const uint64_t F = normalize ? 1 : (trace ? n : count);
        if (F % params_.t == 0) throw std::runtime_error("FHEContext::pack_lwes: the factor F is 0 modulo t; pack with normalize");
        ensure_components(out, 2, 0);
        const size_t lwe_c = (lwe.size() * 8 + sizeof(uint256_t) - 1) / sizeof(uint256_t);
        uint256_t *d = device_alloc(lwe_c);
        try {
            check(fhe_hip_memcpy_h2d(d, lwe.data(), lwe.size() * 8), "memcpy h2d");
            check(fhe_lwe_pack(params_.rns_ntt->handle(), pk.sets.data(), out.components[0]->coeffs, out.components[1]->coeffs, (const uint64_t *)d, count,
                               trace ? 1 : 0, normalize ? 1 : 0, 1), "FHEContext::pack_lwes");
            device_synchronize();
        } catch (...) { device_free(d); throw; }
        device_free(d);
        out.level = 0; out.correction = F % params_.t; out.noise_budget = 0; out.is_ntt_form = false;
    }

    // FHEContext::bootstrap (include/fhe.cuh:119, declared only) as one chainable call: lwe is [batch][n_lwe + 1] values below q_lwe under the
    // LWE secret of bk; out_lwe is [batch][n_lwe + 1] under the SAME secret, an LWE ciphertext of the test vector's entry at the input's phase,
    // modulo the first prime q_0 (q_out == 0) or modulo q_out (2 <= q_out <= 2^48, rounded in the key-switch launch).  It can be the `lwe` of the
    // next call (q_lwe = q_0 or q_out): give the test vector the half-slot offset Delta f + Delta / 2 so that the output sits mid-slot.  On
    // buffers owned by the call: fhe_lwe_prepare_accumulator -> fhe_blind_rotate -> fhe_rns_rescale_drop_last of both accumulators down the level
    // engines to one prime -> fhe_rlwe_sample_extract on the one-limb engine -> fhe_lwe_keyswitch.  Every engine of the context has a stream of
    // its own, so the call synchronises the device where the work passes from one engine to the next.
    void bootstrap_lwe(std::vector<uint64_t> &out_lwe, const std::vector<uint64_t> &lwe, uint64_t q_lwe, const Polynomial &test_vector, const BootstrapKey &bk,
                       uint64_t q_out = 0, uint32_t idx = 0) {
        const uint32_t n_lwe = (uint32_t)bk.rows_c0.size(), n = params_.n, L = num_levels();
        if (!n_lwe || bk.rows_c1.size() != n_lwe || !bk.lwe_ksk) throw std::runtime_error("FHEContext::bootstrap_lwe: the bootstrapping key is empty");
        if (bk.made_for != params_.rns_ntt) throw std::runtime_error("FHEContext::bootstrap_lwe: the bootstrapping key was generated by another context");
        if (lwe.empty() || lwe.size() % (n_lwe + 1)) throw std::runtime_error("FHEContext::bootstrap_lwe: lwe must hold batch x (n_lwe + 1) values");
        const uint32_t batch = (uint32_t)(lwe.size() / (n_lwe + 1));
        const size_t poly = (size_t)L * n, acc = poly * batch;                             // containers
        auto containers = [](size_t bytes) { return (bytes + sizeof(uint256_t) - 1) / sizeof(uint256_t); };
        const size_t lwe_c = containers(lwe.size() * 8), sh_c = containers((size_t)n_lwe * batch * 4), ext_c = containers((size_t)batch * (n + 1) * 8);
        uint256_t *d = device_alloc(4 * acc + 2 * lwe_c + sh_c + ext_c);
        try {
            uint256_t *cur0 = d, *cur1 = d + acc, *oth0 = d + 2 * acc, *oth1 = d + 3 * acc, *d_lwe = d + 4 * acc, *d_out = d_lwe + lwe_c, *d_sh = d_out + lwe_c,
                      *d_ext = d_sh + sh_c;
            fhe_rns_ntt_t *h = params_.rns_ntt->handle();
            check(fhe_hip_memcpy_h2d(d_lwe, lwe.data(), lwe.size() * 8), "memcpy h2d");
            check(fhe_lwe_prepare_accumulator(h, q_lwe, n_lwe, (const uint64_t *)d_lwe, test_vector.coeffs, cur0, cur1, (uint32_t *)d_sh, batch), "bootstrap_lwe: prepare");
            check(fhe_blind_rotate(h, bk.rows_c0.data(), bk.rows_c1.data(), n_lwe, cur0, cur1, (const uint32_t *)d_sh, oth0, oth1, batch), "bootstrap_lwe: blind rotation");
            for (uint32_t level = 0; level + 1 < L; level++) {                            // [batch][L - level][n] -> [batch][L - level - 1][n]
                fhe_rns_ntt_t *hl = engine(level).handle();
                if (level) device_synchronize();                                          // the previous level's engine wrote cur0 / cur1
                check(fhe_rns_rescale_drop_last(hl, oth0, cur0, batch), "bootstrap_lwe: rescale");
                check(fhe_rns_rescale_drop_last(hl, oth1, cur1, batch), "bootstrap_lwe: rescale");
                std::swap(cur0, oth0); std::swap(cur1, oth1);
            }
            fhe_rns_ntt_t *h1 = engine(L - 1).handle();                                   // the one-limb engine (the context's own when L == 1)
            if (L > 1) device_synchronize();
            check(fhe_rlwe_sample_extract(h1, (uint64_t *)d_ext, cur0, cur1, idx, batch), "bootstrap_lwe: sample extraction");
            check(fhe_lwe_keyswitch(h1, bk.lwe_ksk, q_out, (uint64_t *)d_out, (const uint64_t *)d_ext, batch), "bootstrap_lwe: key switch");
            device_synchronize();
            out_lwe.resize(lwe.size());
            check(fhe_hip_memcpy_d2h(out_lwe.data(), d_out, out_lwe.size() * 8), "memcpy d2h");
        } catch (...) { device_free(d); throw; }
        device_free(d);
    }

    // FHEContext::bootstrap(Ciphertext&) (include/fhe.cuh:119, declared only): refresh `count` evenly spaced coefficients of a ciphertext and apply
    // a table to them.  The reference declares bootstrap(Ciphertext&, const SecretKey&) with no keys: a refresh that reads the secret key is a
    // decryption, so the evaluation keys made FROM it are the arguments instead (bootstrap_key_gen, packing_key_gen), as pack_lwes did for the last
    // step.  Scaled (MSB) encoding, that of bootstrap_lwe: with Q_level the product of the primes of ct's level and Delta = floor(Q_level / (2p)),
    // coefficient i n / count of ct has phase Delta m_i + Delta / 2 + e; the other coefficients are ignored.  test_vector is one top-level
    // polynomial, tv[j] the value for a phase in slice j of the n slices of [0, Q / 2).  On buffers owned by the call, ct untouched until the end:
    // fhe_rns_rescale_drop_last of both components down the level engines to the one-limb engine -> fhe_rlwe_sample_extract_strided ->
    // fhe_lwe_keyswitch with q_out = q_lwe (2 <= q_lwe <= 2^48) -> fhe_lwe_prepare_accumulator -> fhe_blind_rotate at level 0 with batch = count
    // -> fhe_rlwe_pack with the trace and the normalisation.  The result replaces ct: level 0, correction 1, coefficient i n / count of phase
    // tv[phase~_i] plus noise and every other coefficient of phase 0 plus noise.  Keys: the packing keys carry noise t e like every key of the
    // context, which the scaled encoding sees in full: a context that bootstraps sets the plaintext modulus to 2 before key generation, as a CKKS
    // context does.  Every engine of the context has a stream of its own, so the call synchronises the device where the work passes from one
    // engine to the next, as bootstrap_lwe does.
    void bootstrap(Ciphertext &ct, const Polynomial &test_vector, const BootstrapKey &bk, const PackingKeys &pk, uint32_t count, uint64_t q_lwe) {
        const uint32_t n_lwe = (uint32_t)bk.rows_c0.size(), n = params_.n, L = num_levels();
        if (!n_lwe || bk.rows_c1.size() != n_lwe || !bk.lwe_ksk) throw std::runtime_error("FHEContext::bootstrap: the bootstrapping key is empty");
        if (bk.made_for != params_.rns_ntt) throw std::runtime_error("FHEContext::bootstrap: the bootstrapping key was generated by another context");
        if (pk.made_for != params_.rns_ntt || pk.sets.empty()) throw std::runtime_error("FHEContext::bootstrap: the packing keys were generated by another context");
        if (ct.components.size() != 2) throw std::runtime_error("FHEContext::bootstrap: 2-component ciphertext expected (relinearize first)");
        if (ct.level >= L) throw std::runtime_error("FHEContext::bootstrap: no such level");
        if (!count || (count & (count - 1)) || count > n) throw std::runtime_error("FHEContext::bootstrap: count must be a power of two in [1, n]");
        if (test_vector.num_limbs != L) throw std::runtime_error("FHEContext::bootstrap: a top-level test vector is needed");
        const size_t poly = (size_t)L * n, acc = poly * count;                              // containers
        auto containers = [](size_t bytes) { return (bytes + sizeof(uint256_t) - 1) / sizeof(uint256_t); };
        const size_t low_c = (size_t)(L - ct.level) * n, ext_c = containers((size_t)count * (n + 1) * 8), ks_c = containers((size_t)count * (n_lwe + 1) * 8),
                     sh_c = containers((size_t)n_lwe * count * 4);
        std::unique_ptr<Polynomial> o0(new_polynomial()), o1(new_polynomial());
        uint256_t *d = device_alloc(4 * acc + 4 * low_c + ext_c + ks_c + sh_c);
        try {
            uint256_t *a0 = d, *a1 = d + acc, *t0 = d + 2 * acc, *t1 = d + 3 * acc, *r0 = d + 4 * acc, *r1 = r0 + low_c, *u0 = r1 + low_c, *u1 = u0 + low_c,
                      *d_ext = u1 + low_c, *d_ks = d_ext + ext_c, *d_sh = d_ks + ks_c;
            const uint256_t *cur0 = ct.components[0]->coeffs, *cur1 = ct.components[1]->coeffs;
            for (uint32_t level = ct.level; level + 1 < L; level++) {                       // [L - level][n] -> [L - level - 1][n]; ct itself is only read
                fhe_rns_ntt_t *hl = engine(level).handle();
                if (level > ct.level) device_synchronize();                                // the previous level's engine wrote cur0 / cur1
                check(fhe_rns_rescale_drop_last(hl, r0, cur0, 1), "bootstrap: rescale");
                check(fhe_rns_rescale_drop_last(hl, r1, cur1, 1), "bootstrap: rescale");
                cur0 = r0; cur1 = r1; std::swap(r0, u0); std::swap(r1, u1);
            }
            fhe_rns_ntt_t *h1 = engine(L - 1).handle(), *h = params_.rns_ntt->handle();     // the one-limb engine (the context's own when L == 1)
            device_synchronize();
            check(fhe_rlwe_sample_extract_strided(h1, (uint64_t *)d_ext, cur0, cur1, count, 1), "bootstrap: sample extraction");
            check(fhe_lwe_keyswitch(h1, bk.lwe_ksk, q_lwe, (uint64_t *)d_ks, (const uint64_t *)d_ext, count), "bootstrap: LWE key switch");
            if (L > 1) device_synchronize();
            check(fhe_lwe_prepare_accumulator(h, q_lwe, n_lwe, (const uint64_t *)d_ks, test_vector.coeffs, a0, a1, (uint32_t *)d_sh, count), "bootstrap: prepare");
            check(fhe_blind_rotate(h, bk.rows_c0.data(), bk.rows_c1.data(), n_lwe, a0, a1, (const uint32_t *)d_sh, t0, t1, count), "bootstrap: blind rotation");
            check(fhe_rlwe_pack(h, pk.sets.data(), o0->coeffs, o1->coeffs, a0, a1, count, 1, 1, 1), "bootstrap: packing");
            device_synchronize();
        } catch (...) { device_free(d); throw; }
        device_free(d);
        free_components(ct);
        ct.components.push_back(o0.release()); ct.components.push_back(o1.release());
        ct.level = 0; ct.correction = 1; ct.noise_budget = 0; ct.is_ntt_form = false;
    }

    void galoiskey_gen_fused(GaloisKeys &gal_keys, const SecretKey &sk) {                   // the default set of galoiskey_gen
        std::vector<int> steps;
        for (uint32_t s = 1; s < params_.n / 2; s <<= 1) { steps.push_back((int)s); steps.push_back(-(int)s); }
        galoiskey_gen_fused(gal_keys, sk, steps, true, 16);
    }

    // result = sigma_g(ct), key-switched back to s (one fhe_ct_apply_galois call); `result` may be `ct`.
    void apply_galois(Ciphertext &result, const Ciphertext &ct, uint32_t galois_elt, const GaloisKeys &gal_keys) {
        if (ct.components.size() != 2) throw std::runtime_error("FHEContext::apply_galois: 2-component ciphertext expected (relinearize first)");
        const size_t idx = galois_key_index(gal_keys, galois_elt);
        if (idx == (size_t)-1) throw std::runtime_error("FHEContext::apply_galois: no Galois key for this element");
        const float nb = ct.noise_budget; const uint32_t lv = ct.level; const uint64_t corr = ct.correction;   // sigma_g(correction * m) = correction * sigma_g(m)
        const std::vector<fhe_relin_keys_t *> &keys = galois_keys_at(gal_keys, lv);
        std::unique_ptr<Polynomial> o0(new_polynomial(lv)), o1(new_polynomial(lv));     // the ABI call is out of place
        check(fhe_ct_apply_galois(engine(lv).handle(), keys[idx], galois_elt, o0->coeffs, o1->coeffs, ct.components[0]->coeffs,
                                  ct.components[1]->coeffs, 1), "FHEContext::apply_galois");
        ensure_components(result, 2, lv);
        while (result.components.size() > 2) { delete result.components.back(); result.components.pop_back(); }
        const size_t bytes = o0->count() * sizeof(uint256_t);
        check(fhe_hip_memcpy_d2d(result.components[0]->coeffs, o0->coeffs, bytes), "apply_galois copy");
        check(fhe_hip_memcpy_d2d(result.components[1]->coeffs, o1->coeffs, bytes), "apply_galois copy");
        device_synchronize();
        result.noise_budget = nb; result.level = lv; result.correction = corr; result.is_ntt_form = false;
    }
    // FHEContext::rotate_rows (include/fhe.cuh:112-113): cyclic left shift by `steps` of both rows.  One call when the key set holds 3^steps,
    // else a composition of the power-of-two steps it holds (either direction); throws when the step cannot be reached.
    void rotate_rows(Ciphertext &result, const Ciphertext &ct, int steps, const GaloisKeys &gal_keys) {
        const uint32_t half = params_.n / 2, r = (uint32_t)(((long long)steps % half + half) % half);
        const uint32_t g = galois_element((int)r);
        if (galois_key_index(gal_keys, g) != (size_t)-1) { apply_galois(result, ct, g, gal_keys); return; }
        auto compose = [&](int dir, std::vector<uint32_t> &out) {  // r as a sum of +2^i, or n/2 - r as a sum of -2^i
            const uint32_t m = dir > 0 ? r : half - r;
            out.clear();
            for (uint32_t b = 0; (1u << b) < half; b++) {
                if (!((m >> b) & 1)) continue;
                const uint32_t e = galois_element(dir * (int)(1u << b));
                if (galois_key_index(gal_keys, e) == (size_t)-1) return false;
                out.push_back(e);
            }
            return true;
        };
        std::vector<uint32_t> path;
        if (!compose(1, path) && !compose(-1, path)) throw std::runtime_error("FHEContext::rotate_rows: no composition of the Galois keys reaches this step");
        if (path.empty()) {                                         // r = 0: the identity
            if (&result != &ct) { ensure_components(result, ct.components.size(), ct.level); copy_ciphertext(result, ct); }
            return;
        }
        apply_galois(result, ct, path[0], gal_keys);
        for (size_t i = 1; i < path.size(); i++) apply_galois(result, result, path[i], gal_keys);
    }
    // Hoisted rotations: ct is decomposed and transformed once (fhe_ct_hoist), every step is then one fhe_ct_apply_galois_hoisted with the key of
    // 3^step.  UNLIKE rotate_rows, a missing step is not composed from power-of-two keys: each step needs its own key in the set (a composed
    // rotation is not a rotation of the hoisted ciphertext; generate keys with galoiskey_gen(gal_keys, sk, steps, ...)), else it throws; step 0
    // is a copy.  The results decrypt like rotate_rows' but are not bit-identical to them.
    std::vector<Ciphertext> rotate_rows_hoisted(const Ciphertext &ct, const std::vector<int> &steps, const GaloisKeys &gal_keys) {
        if (ct.components.size() != 2) throw std::runtime_error("FHEContext::rotate_rows_hoisted: 2-component ciphertext expected (relinearize first)");
        const uint32_t half = params_.n / 2;
        std::vector<uint32_t> elts;
        for (int st : steps) {
            const uint32_t r = (uint32_t)(((long long)st % half + half) % half), g = galois_element((int)r);
            if (r && galois_key_index(gal_keys, g) == (size_t)-1) throw std::runtime_error("FHEContext::rotate_rows_hoisted: no Galois key for a step");
            elts.push_back(r ? g : 1);
        }
        const std::vector<fhe_relin_keys_t *> &keys = galois_keys_at(gal_keys, ct.level);
        fhe_rns_ntt_t *h = engine(ct.level).handle();
        std::vector<Ciphertext> out(steps.size());
        if (!elts.empty())
            check(fhe_ct_hoist(h, gal_keys.decomp_bits, ct.components[1]->coeffs, 1), "FHEContext::rotate_rows_hoisted: hoist");
        for (size_t s = 0; s < elts.size(); s++) {
            ensure_components(out[s], 2, ct.level);
            if (elts[s] == 1) copy_ciphertext(out[s], ct);
            else check(fhe_ct_apply_galois_hoisted(h, keys[galois_key_index(gal_keys, elts[s])], elts[s],
                                                   out[s].components[0]->coeffs, out[s].components[1]->coeffs, ct.components[0]->coeffs, 1),
                       "FHEContext::rotate_rows_hoisted");
            out[s].noise_budget = ct.noise_budget; out[s].level = ct.level; out[s].correction = ct.correction; out[s].is_ntt_form = false;
        }
        device_synchronize();
        return out;
    }
    // Hoisted linear transform (plaintext matrix-vector product by diagonals): sum_s diagonals[s] * rotate_rows(ct, steps[s]) from ONE hoist and
    // ONE fhe_ct_linear_transform_hoisted at the ciphertext's level.  Step 0 is the keyless term; every other step needs its own key in the
    // set, else it throws (as rotate_rows_hoisted).  A level-l plaintext is the prefix of its buffer (as multiply_plain); correction and level
    // are carried from ct.  The ring elements are those of rotate_rows_hoisted + multiply_plain + add.
    Ciphertext linear_transform_hoisted(const Ciphertext &ct, const std::vector<int> &steps, const std::vector<const Plaintext *> &diagonals,
                                        const GaloisKeys &gal_keys) {
        if (ct.components.size() != 2) throw std::runtime_error("FHEContext::linear_transform_hoisted: 2-component ciphertext expected (relinearize first)");
        if (steps.empty() || steps.size() != diagonals.size()) throw std::runtime_error("FHEContext::linear_transform_hoisted: one diagonal per step, at least one");
        const uint32_t half = params_.n / 2;
        std::vector<uint32_t> elts;
        for (int st : steps) {
            const uint32_t r = (uint32_t)(((long long)st % half + half) % half), g = galois_element((int)r);
            if (r && galois_key_index(gal_keys, g) == (size_t)-1) throw std::runtime_error("FHEContext::linear_transform_hoisted: no Galois key for a step");
            elts.push_back(r ? g : 1);
        }
        const std::vector<fhe_relin_keys_t *> &keys = galois_keys_at(gal_keys, ct.level);
        fhe_rns_ntt_t *h = engine(ct.level).handle();
        std::vector<const fhe_relin_keys_t *> gks;
        std::vector<const void *> plains;
        for (size_t s = 0; s < elts.size(); s++) {
            if (!diagonals[s] || !diagonals[s]->poly) throw std::runtime_error("FHEContext::linear_transform_hoisted: null diagonal");
            gks.push_back(elts[s] == 1 ? nullptr : keys[galois_key_index(gal_keys, elts[s])]);
            plains.push_back(diagonals[s]->poly->coeffs);
        }
        fhe_linear_transform_t *lt = nullptr;
        check(fhe_linear_transform_create(h, &lt, gal_keys.decomp_bits, elts.data(), gks.data(), plains.data(), (uint32_t)elts.size()),
              "FHEContext::linear_transform_hoisted: create");
        Ciphertext out;
        ensure_components(out, 2, ct.level);
        int rc = fhe_ct_hoist(h, gal_keys.decomp_bits, ct.components[1]->coeffs, 1);
        if (!rc) rc = fhe_ct_linear_transform_hoisted(h, lt, out.components[0]->coeffs, out.components[1]->coeffs, ct.components[0]->coeffs,
                                                      ct.components[1]->coeffs, 1);
        if (!rc) device_synchronize();
        fhe_linear_transform_destroy(lt);
        check(rc, "FHEContext::linear_transform_hoisted");
        out.noise_budget = ct.noise_budget; out.level = ct.level; out.correction = ct.correction; out.is_ntt_form = false;
        return out;
    }
    // FHEContext::rotate_columns (include/fhe.cuh:114-115): swaps the two rows (g = 2n - 1).
    void rotate_columns(Ciphertext &result, const Ciphertext &ct, const GaloisKeys &gal_keys) { apply_galois(result, ct, column_element(), gal_keys); }

    // hands every element's key rows to the engine once, cached in the GaloisKeys object
    void import_galois_keys(const GaloisKeys &gk) {
        if (gk.imported_for == params_.rns_ntt && gk.imported.size() == gk.elements.size()) return;
        for (fhe_relin_keys_t *k : gk.imported) fhe_relin_keys_destroy(k);
        gk.imported.clear(); gk.drop_levels();
        const uint32_t levels = relin_levels(gk.decomp_bits);
        if (gk.gal_keys.size() != (size_t)levels * gk.elements.size()) throw std::runtime_error("FHEContext: Galois key set of the wrong size");
        for (size_t e = 0; e < gk.elements.size(); e++) {
            std::vector<const void *> kb, ka;
            for (uint32_t r = 0; r < levels; r++) { const PublicKey *k = gk.gal_keys[e * levels + r]; kb.push_back(k->pk0->coeffs); ka.push_back(k->pk1->coeffs); }
            fhe_relin_keys_t *h = nullptr;
            check(fhe_relin_keys_create(params_.rns_ntt->handle(), &h, gk.decomp_bits, kb.data(), ka.data(), levels), "FHEContext: Galois key import");
            gk.imported.push_back(h);
        }
        gk.imported_for = params_.rns_ntt;
    }

    // every element's key set for ciphertexts at `level`: level 0 is import_galois_keys, lower levels are sliced from the same rows (relin_keys_at)
    const std::vector<fhe_relin_keys_t *> &galois_keys_at(const GaloisKeys &gk, uint32_t level) {
        import_galois_keys(gk);
        if (!level) return gk.imported;
        if (gk.imported_levels.size() < num_levels()) gk.imported_levels.resize(num_levels());
        std::vector<fhe_relin_keys_t *> &sets = gk.imported_levels[level];
        if (sets.size() != gk.elements.size()) {
            for (fhe_relin_keys_t *k : sets) fhe_relin_keys_destroy(k);
            sets.clear();
            const size_t rows = gk.gal_keys.size() / gk.elements.size();
            for (size_t e = 0; e < gk.elements.size(); e++) sets.push_back(import_sliced(gk.gal_keys.data() + e * rows, rows, gk.decomp_bits, level));
        }
        return sets;
    }

    // ---- levels: BGV modulus switching down the prime chain (include/fhe.cuh:109-110, 122; declared only in the reference) -------------------
    // Drops the last prime of ct's level from all its components (2 or 3) in one fhe_ct_mod_switch_drop_last call: the noise shrinks by about
    // the dropped prime (plus a rounding term of the size of a fresh ciphertext's noise), the plaintext picks up q_last^-1 mod t (correction).
    void mod_switch_to_next(Ciphertext &ct) {
        const uint32_t L = num_levels(), k = (uint32_t)ct.components.size();
        if (ct.level + 1 >= L) throw std::runtime_error("FHEContext::mod_switch_to_next: the ciphertext is at the last level");
        if (k < 1 || k > 3) throw std::runtime_error("FHEContext::mod_switch_to_next: 1 to 3 components expected");
        const uint256_t &q_last = params_.rns_moduli[L - 1 - ct.level];
        const uint64_t t = params_.t;
        std::vector<Polynomial *> outs;
        std::vector<uint256_t *> d_out; std::vector<const uint256_t *> d_in;
        for (uint32_t i = 0; i < k; i++) { outs.push_back(new_polynomial(ct.level + 1)); d_out.push_back(outs[i]->coeffs); d_in.push_back(ct.components[i]->coeffs); }
        engine(ct.level).mod_switch_drop_last(t, d_out.data(), d_in.data(), k);
        device_synchronize();
        for (uint32_t i = 0; i < k; i++) { delete ct.components[i]; ct.components[i] = outs[i]; }
        ct.level += 1;
        ct.correction = mul_mod_t(ct.correction, inv_mod_t(mod_small(q_last.limbs, t)));
    }
    void mod_switch_to_level(Ciphertext &ct, uint32_t target) {
        if (target < ct.level) throw std::runtime_error("FHEContext::mod_switch_to_level: the target is above the ciphertext's level");
        if (target >= num_levels()) throw std::runtime_error("FHEContext::mod_switch_to_level: no such level");
        while (ct.level < target) mod_switch_to_next(ct);
    }
    // floor(log2(Q_l / 2)) - ceil(log2(max_i |v_i|)), clipped at 0: v the centred value of c0 + c1 s (+ c2 s^2) modulo Q_l, i.e. the bits left
    // before the noise wraps around Q_l and decryption fails.
    float estimate_noise_budget(const Ciphertext &ct, const SecretKey &sk) {
        uint64_t Q[4], half[4];
        const std::vector<uint256_t> v = decrypt_values(ct, sk, Q, half);
        uint64_t mx[4] = {0, 0, 0, 0};
        for (const uint256_t &x : v) {
            uint64_t a[4];
            if (greater(x.limbs, half)) sub4(a, Q, x.limbs); else std::copy(x.limbs, x.limbs + 4, a);
            if (greater(a, mx)) std::copy(a, a + 4, mx);
        }
        const int qb = bit_length(Q), mb = bit_length(mx);
        const bool pow2 = __builtin_popcountll(mx[0]) + __builtin_popcountll(mx[1]) + __builtin_popcountll(mx[2]) + __builtin_popcountll(mx[3]) == 1;
        const int budget = (qb - 2) - (pow2 ? mb - 1 : mb);             // floor(log2(Q / 2)) - ceil(log2 max); max = 0 counts as 1
        return (float)std::max(0, budget);
    }

    // SIMD-slot encoding (the reference's encode scales by delta, src/fhe.cu:113-136, and its BatchEncoder is a passthrough,
    // :267-279; the expectations of its test -- element-wise products -- need real slots): m(zeta_i) = values[i].
    void encode(Plaintext &pt, const std::vector<uint64_t> &values) {
        const uint32_t n = params_.n; const uint64_t t = params_.t;
        if ((t - 1) % (2ull * n)) throw std::runtime_error("FHEContext::encode: t must be 1 (mod 2n) for slot encoding");
        std::vector<uint64_t> m(n, 0);
        for (size_t i = 0; i < values.size() && i < n; i++) m[i] = values[i] % t;
        slot_transform(m, true);
        std::vector<long long> sm(m.begin(), m.end());
        if (!pt.poly) pt.poly = new_polynomial();
        upload_signed(*pt.poly, sm);
        pt.is_ntt_form = false;
    }
    void decode(std::vector<uint64_t> &values, const Plaintext &pt) {
        const uint32_t n = params_.n, L = (uint32_t)params_.rns_moduli.size();
        std::vector<uint256_t> h((size_t)L * n);
        device_synchronize(); copy_to_host(h.data(), pt.poly->coeffs, h.size());
        values.assign(n, 0);
        for (uint32_t i = 0; i < n; i++) values[i] = h[i].limbs[0] % params_.t;              // plaintexts are stored reduced mod t in every limb
        slot_transform(values, false);
    }

    // encode / decode on the device (fhe_slots_encode / fhe_slots_decode_poly): the n values go up as 8-byte words and the [L][n] plaintext is
    // written there once.  Natural slot order: equal to encode / decode value for value; encode and decode themselves stay as they are.
    void encode_fused(Plaintext &pt, const std::vector<uint64_t> &values) { encode_slots(pt, values, FHE_SLOTS_NATURAL); }
    void decode_fused(std::vector<uint64_t> &values, const Plaintext &pt) { decode_slots(values, pt, FHE_SLOTS_NATURAL); }
    // decrypt_fused and decode_fused chained on the device: fhe_ct_decrypt writes the n coefficients, fhe_slots_decode turns them into the
    // slot values in place, n 8-byte words come back
    void decrypt_decode_fused(std::vector<uint64_t> &values, const Ciphertext &ct, const SecretKey &sk) { decrypt_decode_slots(values, ct, sk, FHE_SLOTS_NATURAL); }

private:
    friend class BatchEncoder;                               // the row order of the same three
    // the three above in either slot order (fhe_slot_order)
    void encode_slots(Plaintext &pt, const std::vector<uint64_t> &values, int order) {
        const uint32_t n = params_.n; const uint64_t t = params_.t;
        std::vector<uint64_t> v(n, 0);
        for (size_t i = 0; i < values.size() && i < n; i++) v[i] = values[i] % t;
        if (!pt.poly) pt.poly = new_polynomial();
        const uint32_t level = num_levels() - pt.poly->num_limbs;
        uint256_t *d_v = device_alloc(slot_words());
        try {
            check(fhe_hip_memcpy_h2d(d_v, v.data(), (size_t)n * sizeof(uint64_t)), "encode_fused: upload");
            check(fhe_slots_encode(engine(level).handle(), encoder_at(level, order), pt.poly->coeffs, reinterpret_cast<const uint64_t *>(d_v), 1), "encode_fused");
            device_synchronize();
        } catch (...) { device_free(d_v); throw; }
        device_free(d_v);
        pt.is_ntt_form = false;
    }
    void decode_slots(std::vector<uint64_t> &values, const Plaintext &pt, int order) {
        const uint32_t n = params_.n, level = num_levels() - pt.poly->num_limbs;
        uint256_t *d_v = device_alloc(slot_words());
        values.assign(n, 0);
        try {
            check(fhe_slots_decode_poly(engine(level).handle(), encoder_at(level, order), reinterpret_cast<uint64_t *>(d_v), pt.poly->coeffs, 1), "decode_fused");
            device_synchronize();
            check(fhe_hip_memcpy_d2h(values.data(), d_v, (size_t)n * sizeof(uint64_t)), "decode_fused: download");
        } catch (...) { device_free(d_v); throw; }
        device_free(d_v);
    }
    void decrypt_decode_slots(std::vector<uint64_t> &values, const Ciphertext &ct, const SecretKey &sk, int order) {
        const uint32_t n = params_.n, Ll = num_levels() - ct.level;
        if (ct.components.size() != 2 && ct.components.size() != 3) throw std::runtime_error("FHEContext: a ciphertext of 2 or 3 components is needed");
        for (const Polynomial *c : ct.components)
            if (c->num_limbs != Ll) throw std::runtime_error("FHEContext: ciphertext components do not have the limbs of its level");
        const fhe_secret_key_t *key = secret_key_at(sk, ct.level);
        std::vector<const uint256_t *> comps;
        for (const Polynomial *c : ct.components) comps.push_back(c->coeffs);
        uint256_t *d_v = device_alloc(slot_words());
        uint64_t *d_m = reinterpret_cast<uint64_t *>(d_v);
        values.assign(n, 0);
        try {
            engine(ct.level).decrypt(key, params_.t, inv_mod_t(ct.correction), d_m, nullptr, comps.data(), (uint32_t)comps.size());
            check(fhe_slots_decode(engine(ct.level).handle(), encoder_at(ct.level, order), d_m, d_m, 1), "decrypt_decode_fused");
            device_synchronize();
            check(fhe_hip_memcpy_d2h(values.data(), d_v, (size_t)n * sizeof(uint64_t)), "decrypt_decode_fused: download");
        } catch (...) { device_free(d_v); throw; }
        device_free(d_v);
    }
    // the encoder of (level, order), created on first use and kept
    const fhe_batch_encoder_t *encoder_at(uint32_t level, int order) {
        if (order != FHE_SLOTS_NATURAL && order != FHE_SLOTS_ROWS) throw std::runtime_error("FHEContext: unknown slot order");
        if (encoders_.size() < 2 * (size_t)num_levels()) encoders_.resize(2 * (size_t)num_levels());
        std::shared_ptr<fhe_batch_encoder_t> &e = encoders_[2 * (size_t)level + (size_t)order];
        if (!e) {
            fhe_batch_encoder_t *p = nullptr;
            check(fhe_batch_encoder_create(engine(level).handle(), &p, params_.t, order), "FHEContext: batch encoder (t must be a prime = 1 mod 2n)");
            e.reset(p, [](fhe_batch_encoder_t *q) { fhe_batch_encoder_destroy(q); });
        }
        return e.get();
    }

public:
    void encrypt(Ciphertext &ct, const Plaintext &pt, const PublicKey &pk) {               // src/fhe.cu:138-169
        ensure_components(ct, 2, 0);
        RNS_NTTEngine &E = *params_.rns_ntt;
        std::unique_ptr<Polynomial> u(new_polynomial()), e(new_polynomial());
        draw_ternary(*u);
        E.multiply_rns(ct.components[0]->coeffs, pk.pk0->coeffs, u->coeffs);                 // pk0*u (:160)
        E.multiply_rns(ct.components[1]->coeffs, pk.pk1->coeffs, u->coeffs);                 // pk1*u (:165)
        draw_scaled_error(*e);
        E.add_rns(ct.components[0]->coeffs, ct.components[0]->coeffs, e->coeffs);            // + t*e1
        E.add_rns(ct.components[0]->coeffs, ct.components[0]->coeffs, pt.poly->coeffs);      // + m  (:161-162)
        device_synchronize();
        draw_scaled_error(*e);
        E.add_rns(ct.components[1]->coeffs, ct.components[1]->coeffs, e->coeffs);            // + t*e2 (:166)
        device_synchronize();
        ct.level = 0; ct.correction = 1; ct.noise_budget = 0; ct.is_ntt_form = false;
    }

    // The same ciphertext distribution as encrypt in ONE engine call (fhe_ct_encrypt): u, e1, e2 are drawn inside the kernel from three seeds of
    // the context generator with security.sigma, the public key is imported once and kept.  Level 0.  encrypt itself stays as the reference has it.
    void encrypt_fused(Ciphertext &ct, const Plaintext &pt, const PublicKey &pk) {
        ensure_components(ct, 2, 0);
        fhe_rns_ntt_t *h = params_.rns_ntt->handle();
        if (!pk.imported || pk.imported_for != params_.rns_ntt) {
            fhe_public_key_t *k = nullptr;
            check(fhe_public_key_create(h, &k, pk.pk0->coeffs, pk.pk1->coeffs), "encrypt_fused: public key import");
            pk.imported.reset(k, [](fhe_public_key_t *p) { fhe_public_key_destroy(p); });
            pk.imported_for = params_.rns_ntt;
        }
        const uint64_t seeds[3] = {rng_(), rng_(), rng_()};
        check(fhe_ct_encrypt(h, pk.imported.get(), params_.t, (double)params_.security.sigma, seeds, ct.components[0]->coeffs, ct.components[1]->coeffs,
                             pt.poly->coeffs, 1), "encrypt_fused");
        ct.level = 0; ct.correction = 1; ct.noise_budget = 0; ct.is_ntt_form = false;
    }

    // c0 + c1*s (+ c2*s^2) on the engine of ct's level, CRT to the centred integer modulo Q_l through fhe_rns_from_rns, reduced mod t and divided
    // by ct.correction  (src/fhe.cu:171-185).  The secret key of a level is the first L - level limbs of sk, used in place.
    void decrypt(Plaintext &pt, const Ciphertext &ct, const SecretKey &sk) {
        const uint32_t n = params_.n;
        uint64_t Q[4], half[4];
        const std::vector<uint256_t> v = decrypt_values(ct, sk, Q, half);
        const uint64_t t = params_.t, q_mod_t = mod_small(Q, t), cinv = inv_mod_t(ct.correction % t);
        std::vector<long long> m(n);
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t r = mod_small(v[i].limbs, t);
            const uint64_t c = greater(v[i].limbs, half) ? (r + t - q_mod_t) % t : r;           // value - Q when above Q/2
            m[i] = (long long)(cinv == 1 ? c : mul_mod_t(c, cinv));
        }
        if (!pt.poly) pt.poly = new_polynomial();
        upload_signed(*pt.poly, m);
        pt.is_ntt_form = false;
    }

    // decrypt in ONE engine call (fhe_ct_decrypt) on the engine of ct's level: the n plaintext coefficients come back as 8-byte integers, already
    // reduced mod t and divided by ct.correction (scale = correction^-1 mod t).  The secret key is imported once per level and kept.  Equals
    // decrypt slot for slot; decrypt itself stays as it is.
    void decrypt_fused(Plaintext &pt, const Ciphertext &ct, const SecretKey &sk) {
        const uint32_t n = params_.n;
        std::vector<uint64_t> m(n);
        run_decrypt(ct, sk, m.data(), nullptr);
        std::vector<long long> sm(m.begin(), m.end());
        if (!pt.poly) pt.poly = new_polynomial();
        upload_signed(*pt.poly, sm);
        pt.is_ntt_form = false;
    }
    // estimate_noise_budget from the same call: max(0, bit_length(Q_l) - 2 - bit_length(max |v|)).  The engine reports the bit length of the
    // maximum, which cannot tell 2^k from 2^k + 1, so this is the bound that is never optimistic: equal to estimate_noise_budget, except one bit
    // lower when the maximum is an exact power of two (and the budget is not already 0).
    float noise_budget_fused(const Ciphertext &ct, const SecretKey &sk) {
        uint32_t bits = 0;
        run_decrypt(ct, sk, nullptr, &bits);
        uint64_t Q[4] = {1, 0, 0, 0};
        for (uint32_t l = 0; l < num_levels() - ct.level; l++) mul_small(Q, params_.rns_moduli[l].limbs[0]);
        return (float)std::max(0, bit_length(Q) - 2 - (int)bits);
    }

    // ---- BFV: the scale-invariant encoding Delta m + e, Delta = floor(Q / t), of the reference's keygen / encrypt / decrypt (src/fhe.cu:54-185) ----
    // multiply, encrypt and decrypt above are the BGV-flavoured ones and stay as they are.  A BFV context calls set_noise_scale(1) BEFORE key
    // generation: keygen, relinkey_gen(rlk, sk, w) and encrypt then draw e instead of t e (as a CKKS context sets the plaintext modulus first).
    // Level 0 only, correction 1.
    void set_noise_scale(uint64_t s) {
        if (!s) throw std::runtime_error("FHEContext::set_noise_scale: the scale must be at least 1");
        noise_scale_ = s;
    }
    uint64_t noise_scale() const { return noise_scale_ ? noise_scale_ : params_.t; }
    // The multiplier for this context's basis and t.  With no auxiliary primes given they are chosen: NTT primes of the ciphertext primes' size
    // outside the basis, as few as P > 32 t n Q takes (fhe_bfv_multiplier_create checks that bound).
    void bfv_multiplier_gen(BFVMultiplier &bm, const std::vector<uint64_t> &aux_moduli = {}) {
        bm.clear();
        fhe_rns_ntt_t *h = params_.rns_ntt->handle();
        const uint32_t L = num_levels();
        int rc = FHE_ERR_INVALID_ARG;
        if (!aux_moduli.empty()) {
            rc = fhe_bfv_multiplier_create(h, &bm.handle, params_.t, aux_moduli.data(), (uint32_t)aux_moduli.size());
            bm.aux_moduli = aux_moduli;
        } else {
            for (const uint256_t &q : params_.rns_moduli)
                if (q.limbs[1] | q.limbs[2] | q.limbs[3]) throw std::runtime_error("FHEContext::bfv_multiplier_gen: word-sized RNS primes are needed");
            const uint32_t bits = 64 - (uint32_t)__builtin_clzll(params_.rns_moduli[0].limbs[0]);
            for (uint32_t Lp = 1; Lp <= 16 && rc == FHE_ERR_INVALID_ARG; Lp++) {          // INVALID_ARG here: the bound needs one more prime
                std::vector<uint64_t> cand(L + Lp), aux;
                check(fhe_find_ntt_primes(bits, params_.n, L + Lp, cand.data()), "FHEContext::bfv_multiplier_gen: prime search");
                for (uint64_t p : cand) {
                    bool in_basis = false;
                    for (const uint256_t &q : params_.rns_moduli) in_basis |= q.limbs[0] == p;
                    if (!in_basis && aux.size() < Lp) aux.push_back(p);
                }
                rc = fhe_bfv_multiplier_create(h, &bm.handle, params_.t, aux.data(), (uint32_t)aux.size());
                bm.aux_moduli = aux;
            }
        }
        if (rc) bm.aux_moduli.clear();
        check(rc, "FHEContext::bfv_multiplier_gen");
        bm.t = params_.t; bm.made_for = params_.rns_ntt;
    }
    // (c0, c1) = relin(round(t / Q (a (x) b))) with the tensor product over the integers: ONE fhe_bfv_multiply_relin; with an empty RelinKeys
    // the three components of fhe_bfv_multiply.  The context's own multiplier is made on first use (and again after set_plain_modulus).
    void multiply_bfv(Ciphertext &result, const Ciphertext &a, const Ciphertext &b, const RelinKeys &rlk) {
        if (!bfv_.handle || bfv_.t != params_.t || bfv_.made_for != params_.rns_ntt) bfv_multiplier_gen(bfv_);
        multiply_bfv(result, a, b, rlk, bfv_);
    }
    void multiply_bfv(Ciphertext &result, const Ciphertext &a, const Ciphertext &b, const RelinKeys &rlk, const BFVMultiplier &bm) {
        if (a.components.size() != 2 || b.components.size() != 2) throw std::runtime_error("FHEContext::multiply_bfv: 2-component ciphertexts expected");
        if (a.level || b.level || a.correction != 1 || b.correction != 1) throw std::runtime_error("FHEContext::multiply_bfv: level-0 ciphertexts with correction 1 expected");
        if (!bm.handle || bm.made_for != params_.rns_ntt || bm.t != params_.t) throw std::runtime_error("FHEContext::multiply_bfv: the multiplier was made for another context or plaintext modulus");
        const float nb = a.noise_budget + b.noise_budget + 10;
        if (rlk.rlk_keys.empty()) {
            ensure_components(result, 3, 0);
            check(fhe_bfv_multiply(bm.handle, result.components[0]->coeffs, result.components[1]->coeffs, result.components[2]->coeffs, a.components[0]->coeffs,
                                   a.components[1]->coeffs, b.components[0]->coeffs, b.components[1]->coeffs, 1), "FHEContext::multiply_bfv");
        } else {
            fhe_relin_keys_t *keys = relin_keys_at(rlk, 0);
            ensure_components(result, 2, 0);
            while (result.components.size() > 2) { delete result.components.back(); result.components.pop_back(); }
            check(fhe_bfv_multiply_relin(bm.handle, keys, result.components[0]->coeffs, result.components[1]->coeffs, a.components[0]->coeffs,
                                         a.components[1]->coeffs, b.components[0]->coeffs, b.components[1]->coeffs, 1), "FHEContext::multiply_bfv");
        }
        device_synchronize();
        result.noise_budget = nb; result.level = 0; result.correction = 1;
    }
    // encrypt of Delta pt: the constant Delta mod q_l times the encoded plaintext in every limb (fhe_rns_ntt_multiply_bcast), then the
    // existing encryption, whose errors carry noise_scale() (1 in a BFV context)
    void encrypt_bfv(Ciphertext &ct, const Plaintext &pt, const PublicKey &pk) {
        if (!pt.poly || pt.poly->num_limbs != num_levels()) throw std::runtime_error("FHEContext::encrypt_bfv: a level-0 plaintext is needed");
        const uint32_t n = params_.n, L = num_levels();
        uint64_t Q[4] = {1, 0, 0, 0}, delta[4];
        for (uint32_t l = 0; l < L; l++) mul_small(Q, params_.rns_moduli[l].limbs[0]);
        div_small(delta, Q, params_.t);
        std::vector<uint256_t> h((size_t)L * n);
        for (uint32_t l = 0; l < L; l++) h[(size_t)l * n] = uint256_t(mod_small(delta, params_.rns_moduli[l].limbs[0]));
        std::unique_ptr<Polynomial> dpoly(new_polynomial());
        Plaintext scaled; scaled.poly = new_polynomial();
        copy_to_device(dpoly->coeffs, h.data(), h.size());
        params_.rns_ntt->multiply_rns_bcast(scaled.poly->coeffs, pt.poly->coeffs, dpoly->coeffs, 1);
        try { encrypt(ct, scaled, pk); } catch (...) { delete scaled.poly; throw; }
        device_synchronize();
        delete scaled.poly;
    }
    // v = c0 + c1 s (+ c2 s^2) centred modulo Q through fhe_rns_from_rns, then m = round(t v / Q) mod t on the host, exactly
    void decrypt_bfv(Plaintext &pt, const Ciphertext &ct, const SecretKey &sk) {
        if (ct.level || ct.correction != 1) throw std::runtime_error("FHEContext::decrypt_bfv: a level-0 ciphertext with correction 1 is needed");
        const uint32_t n = params_.n;
        uint64_t Q[4], half[4];
        const std::vector<uint256_t> v = decrypt_values(ct, sk, Q, half);
        const uint64_t t = params_.t;
        std::vector<long long> m(n);
        for (uint32_t i = 0; i < n; i++) {
            const bool neg = greater(v[i].limbs, half);
            uint64_t mag[4];
            if (neg) sub4(mag, Q, v[i].limbs); else std::memcpy(mag, v[i].limbs, 32);
            const uint64_t r = round_scaled(mag, t, Q) % t;
            m[i] = (long long)(neg ? (t - r) % t : r);
        }
        if (!pt.poly) pt.poly = new_polynomial();
        upload_signed(*pt.poly, m);
        pt.is_ntt_form = false;
    }

    // ---- CKKS: approximate arithmetic on the same ciphertexts (fhe_ckks_encode / fhe_ckks_decode; class CKKSEncoder below) -------------------
    // multiply, relinearize, rotate_rows and the level engines are used as they are; they do not look at `scale`, so after a multiply the
    // caller sets result.scale = a.scale * b.scale.  Keys carry noise t e (keygen, relinkey_gen): a CKKS context sets the plaintext modulus to 2
    // BEFORE key generation, the smallest the engine calls accept.
    void set_plain_modulus(uint64_t t) {
        if (t < 2) throw std::runtime_error("FHEContext::set_plain_modulus: t must be at least 2");
        params_.t = t; encoders_.clear();
    }
    // One fhe_ct_encrypt with t = 2 (its contract is t >= 2): c0 + c1 s = pt + 2 e, one bit more noise than e alone.  pt is a level-0 plaintext
    // of CKKSEncoder::encode at `scale`, which the ciphertext records.
    void encrypt_ckks(Ciphertext &ct, const Plaintext &pt, double scale, const PublicKey &pk) {
        if (!pt.poly || pt.poly->num_limbs != num_levels()) throw std::runtime_error("FHEContext::encrypt_ckks: a level-0 plaintext is needed");
        ensure_components(ct, 2, 0);
        fhe_rns_ntt_t *h = params_.rns_ntt->handle();
        if (!pk.imported || pk.imported_for != params_.rns_ntt) {
            fhe_public_key_t *k = nullptr;
            check(fhe_public_key_create(h, &k, pk.pk0->coeffs, pk.pk1->coeffs), "encrypt_ckks: public key import");
            pk.imported.reset(k, [](fhe_public_key_t *p) { fhe_public_key_destroy(p); });
            pk.imported_for = params_.rns_ntt;
        }
        const uint64_t seeds[3] = {rng_(), rng_(), rng_()};
        check(fhe_ct_encrypt(h, pk.imported.get(), 2, (double)params_.security.sigma, seeds, ct.components[0]->coeffs, ct.components[1]->coeffs,
                             pt.poly->coeffs, 1), "encrypt_ckks");
        device_synchronize();
        ct.level = 0; ct.correction = 1; ct.noise_budget = 0; ct.is_ntt_form = false; ct.scale = scale;
    }
    // The CKKS rescale: fhe_rns_rescale_drop_last (the rounded division by the last prime of ct's level) on every component onto the next
    // level's engine; scale /= q_last.
    void rescale_to_next(Ciphertext &ct) {
        const uint32_t L = num_levels();
        if (ct.level + 1 >= L) throw std::runtime_error("FHEContext::rescale_to_next: the ciphertext is at the last level");
        const uint64_t q_last = params_.rns_moduli[L - 1 - ct.level].limbs[0];
        for (Polynomial *&c : ct.components) {
            Polynomial *out = new_polynomial(ct.level + 1);
            try { engine(ct.level).rescale_drop_last(out->coeffs, c->coeffs); device_synchronize(); } catch (...) { delete out; throw; }
            delete c; c = out;
        }
        ct.level += 1;
        ct.scale /= (double)q_last;
    }
    // fhe_ct_decrypt on the engine of ct's level with t = 2^63 and scale 1 (no |v| < 2^62 wraps), then fhe_ckks_decode at ct.scale: the n/2
    // slots.  `coeffs` (optional) receives the n centred integers v of c0 + c1 s (+ c2 s^2) that were decoded.
    void decrypt_ckks(std::vector<std::complex<double>> &values, const Ciphertext &ct, const SecretKey &sk, std::vector<int64_t> *coeffs = nullptr) {
        const uint32_t n = params_.n, Ll = num_levels() - ct.level;
        const uint64_t t63 = 1ull << 63;
        if (ct.components.size() != 2 && ct.components.size() != 3) throw std::runtime_error("FHEContext::decrypt_ckks: a ciphertext of 2 or 3 components is needed");
        for (const Polynomial *c : ct.components)
            if (c->num_limbs != Ll) throw std::runtime_error("FHEContext::decrypt_ckks: ciphertext components do not have the limbs of its level");
        const fhe_secret_key_t *key = secret_key_at(sk, ct.level);
        std::vector<const uint256_t *> comps;
        for (const Polynomial *c : ct.components) comps.push_back(c->coeffs);
        uint256_t *d_m = device_alloc(slot_words()), *d_z = nullptr;
        values.assign(n / 2, std::complex<double>());
        try {
            d_z = device_alloc(slot_words());
            engine(ct.level).decrypt(key, t63, 1, reinterpret_cast<uint64_t *>(d_m), nullptr, comps.data(), (uint32_t)comps.size());
            check(fhe_ckks_decode(engine(ct.level).handle(), ckks_encoder_at(ct.level), reinterpret_cast<double *>(d_z), reinterpret_cast<const uint64_t *>(d_m), t63,
                                  ct.scale, 1), "decrypt_ckks: decode");
            device_synchronize();
            check(fhe_hip_memcpy_d2h(values.data(), d_z, (size_t)n * sizeof(double)), "decrypt_ckks: download");
            if (coeffs) {
                std::vector<uint64_t> w(n);
                check(fhe_hip_memcpy_d2h(w.data(), d_m, (size_t)n * sizeof(uint64_t)), "decrypt_ckks: download");
                coeffs->resize(n);
                for (uint32_t i = 0; i < n; i++) (*coeffs)[i] = w[i] > (t63 >> 1) ? -(int64_t)(t63 - w[i]) : (int64_t)w[i];
            }
        } catch (...) { device_free(d_m); device_free(d_z); throw; }
        device_free(d_m); device_free(d_z);
    }

private:
    friend class CKKSEncoder;
    // the CKKS encoder of a level, created on first use and kept (n = 2^11 .. 2^14, primes below 2^64; the library refuses anything else)
    const fhe_ckks_encoder_t *ckks_encoder_at(uint32_t level) {
        if (ckks_encoders_.size() < num_levels()) ckks_encoders_.resize(num_levels());
        std::shared_ptr<fhe_ckks_encoder_t> &e = ckks_encoders_[level];
        if (!e) {
            fhe_ckks_encoder_t *p = nullptr;
            check(fhe_ckks_encoder_create(engine(level).handle(), &p), "FHEContext: CKKS encoder");
            e.reset(p, [](fhe_ckks_encoder_t *q) { fhe_ckks_encoder_destroy(q); });
        }
        return e.get();
    }
    void ckks_encode(Plaintext &pt, const std::vector<std::complex<double>> &values, double scale, uint32_t level) {
        const uint32_t n = params_.n;
        if (values.size() > n / 2) throw std::runtime_error("CKKSEncoder::encode: more values than slots");
        std::vector<std::complex<double>> v(n / 2);
        std::copy(values.begin(), values.end(), v.begin());
        if (pt.poly && pt.poly->num_limbs != num_levels() - level) { delete pt.poly; pt.poly = nullptr; }
        if (!pt.poly) pt.poly = new_polynomial(level);
        uint256_t *d_v = device_alloc(slot_words());
        try {
            check(fhe_hip_memcpy_h2d(d_v, v.data(), (size_t)n * sizeof(double)), "CKKSEncoder::encode: upload");
            check(fhe_ckks_encode(engine(level).handle(), ckks_encoder_at(level), pt.poly->coeffs, nullptr, reinterpret_cast<const double *>(d_v), scale, 1),
                  "CKKSEncoder::encode");
            device_synchronize();
        } catch (...) { device_free(d_v); throw; }
        device_free(d_v);
        pt.is_ntt_form = false;
    }
    void ckks_decode(std::vector<std::complex<double>> &values, const Plaintext &pt, double scale) {
        const uint32_t n = params_.n;
        if (!pt.poly) throw std::runtime_error("CKKSEncoder::decode: empty plaintext");
        const uint32_t level = num_levels() - pt.poly->num_limbs;
        uint256_t *d_v = device_alloc(slot_words());
        values.assign(n / 2, std::complex<double>());
        try {
            check(fhe_ckks_decode_poly(engine(level).handle(), ckks_encoder_at(level), reinterpret_cast<double *>(d_v), pt.poly->coeffs, scale, 1), "CKKSEncoder::decode");
            device_synchronize();
            check(fhe_hip_memcpy_d2h(values.data(), d_v, (size_t)n * sizeof(double)), "CKKSEncoder::decode: download");
        } catch (...) { device_free(d_v); throw; }
        device_free(d_v);
    }

public:
    const SchemeParams &params() const { return params_; }

private:
    SchemeParams params_;
    std::mt19937_64 rng_{0x5EED0000ull};
    bool device_sampling_ = false;
    std::vector<std::unique_ptr<RNS_NTTEngine>> level_engines_;   // index = level; entry 0 unused (params_.rns_ntt)
    BFVMultiplier bfv_;                    // multiply_bfv's own multiplier, made on first use
    uint64_t noise_scale_ = 0;             // 0: the plaintext modulus t (BGV-style noise); set_noise_scale
    std::vector<std::shared_ptr<fhe_batch_encoder_t>> encoders_;  // index = 2 level + slot order (encoder_at)
    std::vector<std::shared_ptr<fhe_ckks_encoder_t>> ckks_encoders_;   // index = level (ckks_encoder_at)
    size_t slot_words() const { return ((size_t)params_.n * sizeof(uint64_t) + sizeof(uint256_t) - 1) / sizeof(uint256_t); }   // n 8-byte words in containers

    // c0 + c1*s (+ c2*s^2) of a ciphertext at its level as integers in [0, Q_l); Q = Q_l and half = floor(Q_l / 2) as 256-bit integers
    std::vector<uint256_t> decrypt_values(const Ciphertext &ct, const SecretKey &sk, uint64_t Q[4], uint64_t half[4]) {
        const uint32_t n = params_.n, Ll = num_levels() - ct.level, lv = ct.level;
        RNS_NTTEngine &E = engine(lv);
        for (const Polynomial *c : ct.components)
            if (c->num_limbs != Ll) throw std::runtime_error("FHEContext: ciphertext components do not have the limbs of its level");
        std::unique_ptr<Polynomial> acc(new_polynomial(lv)), sp(new_polynomial(lv)), tmp(new_polynomial(lv));
        check(fhe_hip_memcpy_d2d(acc->coeffs, ct.components[0]->coeffs, acc->count() * sizeof(uint256_t)), "decrypt copy");
        check(fhe_hip_memcpy_d2d(sp->coeffs, sk.sk->coeffs, sp->count() * sizeof(uint256_t)), "decrypt copy");
        for (size_t k = 1; k < ct.components.size(); k++) {
            E.multiply_rns(tmp->coeffs, ct.components[k]->coeffs, sp->coeffs);
            E.add_rns(acc->coeffs, acc->coeffs, tmp->coeffs);
            if (k + 1 < ct.components.size()) E.multiply_rns(sp->coeffs, sp->coeffs, sk.sk->coeffs);   // s^(k+1), in place
        }
        uint256_t *d_int = device_alloc(n);
        E.from_rns(d_int, acc->coeffs);
        std::vector<uint256_t> v(n);
        device_synchronize(); copy_to_host(v.data(), d_int, n); device_free(d_int);
        Q[0] = 1; Q[1] = Q[2] = Q[3] = 0;
        for (uint32_t l = 0; l < Ll; l++) mul_small(Q, params_.rns_moduli[l].limbs[0]);
        for (int i = 0; i < 4; i++) half[i] = (Q[i] >> 1) | (i < 3 ? Q[i + 1] << 63 : 0);
        return v;
    }
    // the secret key on the engine of `level`, imported on first use (SecretKey::imported)
    const fhe_secret_key_t *secret_key_at(const SecretKey &sk, uint32_t level) {
        if (sk.imported_for != params_.rns_ntt) { sk.imported.clear(); sk.imported_for = params_.rns_ntt; }
        if (sk.imported.size() < num_levels()) sk.imported.resize(num_levels());
        if (!sk.imported[level]) {
            fhe_secret_key_t *k = nullptr;
            check(fhe_secret_key_create(engine(level).handle(), &k, sk.sk->coeffs), "decrypt_fused: secret key import");
            sk.imported[level].reset(k, [](fhe_secret_key_t *p) { fhe_secret_key_destroy(p); });
        }
        return sk.imported[level].get();
    }
    // one fhe_keyswitch_keys_generate on the top-level engine: noise scale t, sigma = security.sigma, seeds from the context generator
    void generate_key_sets(const SecretKey &sk, uint32_t decomp_bits, const uint32_t *elts, uint32_t num_sets, fhe_relin_keys_t **sets) {
        const uint64_t seeds[2] = {rng_(), rng_()};
        check(fhe_keyswitch_keys_generate(params_.rns_ntt->handle(), secret_key_at(sk, 0), decomp_bits, elts, num_sets, noise_scale(), (double)params_.security.sigma,
                                          seeds, sets), "FHEContext: key-switching key generation");
    }
    // appends the `levels` rows of a key set to `rows` as coefficient-form polynomials (fhe_relin_keys_export)
    void rows_from_export(std::vector<PublicKey *> &rows, const fhe_relin_keys_t *set, uint32_t levels) {
        const size_t poly = (size_t)num_levels() * params_.n;
        uint256_t *d = device_alloc(2 * poly * levels);
        try {
            check(fhe_relin_keys_export(params_.rns_ntt->handle(), set, d, d + poly * levels), "FHEContext: key export");
            for (uint32_t r = 0; r < levels; r++) {
                PublicKey *key = new PublicKey{new_polynomial(), new_polynomial()};
                rows.push_back(key);
                check(fhe_hip_memcpy_d2d(key->pk0->coeffs, d + poly * r, poly * sizeof(uint256_t)), "memcpy d2d");
                check(fhe_hip_memcpy_d2d(key->pk1->coeffs, d + poly * (levels + r), poly * sizeof(uint256_t)), "memcpy d2d");
            }
            device_synchronize();
        } catch (...) { device_free(d); throw; }
        device_free(d);
    }
    // one fhe_ct_decrypt of ct at its level; m (n values) and / or noise_bits may be null
    void run_decrypt(const Ciphertext &ct, const SecretKey &sk, uint64_t *m, uint32_t *noise_bits) {
        const uint32_t n = params_.n, Ll = num_levels() - ct.level;
        if (ct.components.size() != 2 && ct.components.size() != 3) throw std::runtime_error("FHEContext: a ciphertext of 2 or 3 components is needed");
        for (const Polynomial *c : ct.components)
            if (c->num_limbs != Ll) throw std::runtime_error("FHEContext: ciphertext components do not have the limbs of its level");
        const fhe_secret_key_t *key = secret_key_at(sk, ct.level);
        const size_t m_bytes = (size_t)n * sizeof(uint64_t), words = (m_bytes + sizeof(uint32_t) + sizeof(uint256_t) - 1) / sizeof(uint256_t);
        uint256_t *d_out = device_alloc(words);                     // [n] plaintext coefficients, then the noise bits
        uint64_t *d_m = reinterpret_cast<uint64_t *>(d_out);
        uint32_t *d_bits = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(d_out) + m_bytes);
        std::vector<const uint256_t *> comps;
        for (const Polynomial *c : ct.components) comps.push_back(c->coeffs);
        std::vector<uint256_t> host(words);
        try {
            engine(ct.level).decrypt(key, params_.t, inv_mod_t(ct.correction), d_m, noise_bits ? d_bits : nullptr, comps.data(), (uint32_t)comps.size());
            device_synchronize(); copy_to_host(host.data(), d_out, words);
        } catch (...) { device_free(d_out); throw; }
        device_free(d_out);
        if (m) std::memcpy(m, host.data(), m_bytes);
        if (noise_bits) std::memcpy(noise_bits, reinterpret_cast<const char *>(host.data()) + m_bytes, sizeof(uint32_t));
    }
    static void same_level(const Ciphertext &a, const Ciphertext &b, const char *what) {
        if (a.level != b.level) throw std::runtime_error(std::string(what) + ": operands at different levels (mod_switch_to_level first)");
    }
    uint64_t mul_mod_t(uint64_t a, uint64_t b) const { return (uint64_t)((unsigned __int128)(a % params_.t) * (b % params_.t) % params_.t); }
    uint64_t inv_mod_t(uint64_t a) const {                           // extended Euclid: t need not be prime, a must be a unit
        __int128 r0 = params_.t, r1 = a % params_.t, s0 = 0, s1 = 1;
        while (r1) { const __int128 q = r0 / r1, r2 = r0 - q * r1, s2 = s0 - q * s1; r0 = r1; r1 = r2; s0 = s1; s1 = s2; }
        if (r0 != 1) throw std::runtime_error("FHEContext: not invertible modulo t");
        return (uint64_t)(s0 < 0 ? s0 + params_.t : s0);
    }
    // `ct` itself when its correction is 1, else `tmp` = a copy of ct times the centred representative of correction^-1 mod t (a constant
    // polynomial through fhe_rns_ntt_multiply_bcast): the same plaintext with correction 1, at up to log2(t / 2) more bits of noise.
    const Ciphertext &normalized(Ciphertext &tmp, const Ciphertext &ct) {
        if (ct.correction == 1) return ct;
        const uint64_t t = params_.t, c = inv_mod_t(ct.correction);
        std::vector<long long> cpoly(params_.n, 0);
        cpoly[0] = c > t / 2 ? -(long long)(t - c) : (long long)c;
        std::unique_ptr<Polynomial> cp(new_polynomial());            // [L][n]: its first L - level limbs are the level's constant
        upload_signed(*cp, cpoly);
        ensure_components(tmp, ct.components.size(), ct.level);
        for (size_t i = 0; i < ct.components.size(); i++)
            engine(ct.level).multiply_rns_bcast(tmp.components[i]->coeffs, ct.components[i]->coeffs, cp->coeffs, 1);
        device_synchronize();
        tmp.level = ct.level; tmp.correction = 1; tmp.noise_budget = ct.noise_budget; tmp.is_ntt_form = false;
        return tmp;
    }
    static void free_components(Ciphertext &ct) { for (Polynomial *p : ct.components) delete p; ct.components.clear(); }
    // rows j*K + k (j < L', k < K') of a top-level key-switch key, imported on the engine of `level` through the same device pointers
    fhe_relin_keys_t *import_sliced(const PublicKey *const *rows, size_t num_rows, uint32_t decomp_bits, uint32_t level) {
        const uint32_t L = num_levels(), Ll = L - level;
        if (num_rows % L) throw std::runtime_error("FHEContext: key set of the wrong size");
        const uint32_t K = (uint32_t)(num_rows / L);
        uint32_t Kl = 0;
        check(fhe_relin_num_digits(engine(level).handle(), decomp_bits, &Kl), "FHEContext: digits of a level");
        if (Kl > K) throw std::runtime_error("FHEContext: a level needs more digits than the key set has");
        std::vector<const void *> kb, ka;
        for (uint32_t j = 0; j < Ll; j++)
            for (uint32_t k = 0; k < Kl; k++) { const PublicKey *r = rows[(size_t)j * K + k]; kb.push_back(r->pk0->coeffs); ka.push_back(r->pk1->coeffs); }
        fhe_relin_keys_t *h = nullptr;
        check(fhe_relin_keys_create(engine(level).handle(), &h, decomp_bits, kb.data(), ka.data(), (uint32_t)kb.size()), "FHEContext: key import at a level");
        return h;
    }
    static void sub4(uint64_t r[4], const uint64_t a[4], const uint64_t b[4]) {
        unsigned __int128 br = 0;
        for (int i = 0; i < 4; i++) { const unsigned __int128 d = (unsigned __int128)a[i] - b[i] - br; r[i] = (uint64_t)d; br = (d >> 64) & 1; }
    }
    static int bit_length(const uint64_t a[4]) {
        for (int i = 3; i >= 0; i--) if (a[i]) return 64 * i + 64 - __builtin_clzll(a[i]);
        return 0;
    }

    void plain_addsub(Ciphertext &result, const Ciphertext &ct_in, const Plaintext &pt, bool add_it) {
        Ciphertext norm;
        const Ciphertext &ct = normalized(norm, ct_in);
        ensure_components(result, ct.components.size(), ct.level);
        RNS_NTTEngine &E = engine(ct.level);
        if (add_it) E.add_rns(result.components[0]->coeffs, ct.components[0]->coeffs, pt.poly->coeffs);
        else E.sub_rns(result.components[0]->coeffs, ct.components[0]->coeffs, pt.poly->coeffs);
        for (size_t i = 1; i < ct.components.size(); i++)
            if (result.components[i] != ct.components[i])
                check(fhe_hip_memcpy_d2d(result.components[i]->coeffs, ct.components[i]->coeffs, ct.components[i]->count() * sizeof(uint256_t)), "plain op copy");
        result.noise_budget = ct.noise_budget; result.level = ct.level; result.correction = 1;
        if (!norm.components.empty()) { device_synchronize(); free_components(norm); }
    }

    // ---- where keygen / encrypt get their random polynomials: host generator (default) or the device samplers --------------
    void draw_ternary(Polynomial &p) { if (device_sampling_) sample_ternary_polynomial(p); else upload_signed(p, sample_small(1)); }
    void draw_uniform(Polynomial &p) { if (device_sampling_) sample_uniform_polynomial(p); else upload_uniform(p); }
    // noise_scale() * e, e small: t e by default, BGV-style noise (a multiple of the plaintext modulus); e itself in a BFV context
    void draw_scaled_error(Polynomial &p) {
        if (!device_sampling_) { upload_signed(p, sample_small(3), noise_scale()); return; }
        sample_error_polynomial(p);
        const uint32_t n = params_.n, L = (uint32_t)params_.rns_moduli.size();
        for (uint32_t l = 0; l < L; l++) {   // limb l *= t: literal Montgomery product with the scalar t * 2^256 mod q_l (poly_mul_scalar_kernel)
            const uint256_t &q = params_.rns_moduli[l];
            if (q.limbs[1] | q.limbs[2] | q.limbs[3]) throw std::runtime_error("FHEContext: device sampling expects word-sized RNS primes");
            const uint64_t q0 = q.limbs[0], tr = (uint64_t)((unsigned __int128)(noise_scale() % q0) * pow_mod(2, 256, q0) % q0);
            uint64_t inv[4]; check(fhe_montgomery_inverse(q.limbs, inv), "montgomery inverse");
            const uint256_t scalar(tr);
            check(fhe_u256_mont_mul_scalar(p.coeffs + (size_t)l * n, p.coeffs + (size_t)l * n, scalar.limbs, q.limbs, inv[0], n, nullptr),   // legacy default stream: ordered with the engine's blocking stream
                  "FHEContext: scale error by t");
        }
    }

    // ---- host-side helpers of the plumbing above --------------------------------------------------------------------------
    std::vector<long long> sample_small(int bound) {
        std::vector<long long> v(params_.n);
        for (auto &x : v) x = (long long)(rng_() % (2 * bound + 1)) - bound;
        return v;
    }
    // signed integers (times `scale`) -> residues in every limb -> device
    void upload_signed(Polynomial &p, const std::vector<long long> &v, uint64_t scale = 1) {
        const uint32_t n = params_.n, L = (uint32_t)params_.rns_moduli.size();
        std::vector<uint256_t> h((size_t)L * n);
        for (uint32_t l = 0; l < L; l++) {
            const uint64_t q = params_.rns_moduli[l].limbs[0];
            for (uint32_t i = 0; i < n; i++) {
                const uint64_t mag = (uint64_t)((unsigned __int128)(uint64_t)(v[i] < 0 ? -v[i] : v[i]) % q * (scale % q) % q);
                h[(size_t)l * n + i] = uint256_t(v[i] < 0 ? (q - mag) % q : mag);
            }
        }
        copy_to_device(p.coeffs, h.data(), h.size());
    }
    void upload_uniform(Polynomial &p) {
        const uint32_t n = params_.n, L = (uint32_t)params_.rns_moduli.size();
        std::vector<uint256_t> h((size_t)L * n);
        for (uint32_t l = 0; l < L; l++) for (uint32_t i = 0; i < n; i++) h[(size_t)l * n + i] = uint256_t(rng_() % params_.rns_moduli[l].limbs[0]);
        copy_to_device(p.coeffs, h.data(), h.size());
    }
    static uint64_t pow_mod(uint64_t b, uint64_t e, uint64_t m) {
        unsigned __int128 acc = 1, bb = b % m;
        for (; e; e >>= 1) { if (e & 1) acc = acc * bb % m; bb = bb * bb % m; }
        return (uint64_t)acc;
    }
    // forward = false: coefficients -> values at the odd powers of a primitive 2n-th root mod t; forward = true: the inverse map.
    // O(n^2 / 64)-free: a plain O(n log n) negacyclic NTT over Z_t on the host.
    void slot_transform(std::vector<uint64_t> &a, bool inverse) const {
        const uint32_t n = params_.n; const uint64_t t = params_.t;
        uint64_t g = 2;                                           // find a generator-derived primitive 2n-th root of unity mod t
        uint64_t psi = 0;
        for (;; g++) { psi = pow_mod(g, (t - 1) / (2ull * n), t); if (pow_mod(psi, n, t) == t - 1) break; }
        const uint64_t ipsi = pow_mod(psi, 2ull * n - 1, t), ninv = pow_mod(n, t - 2, t);
        auto mulm = [t](uint64_t x, uint64_t y) { return (uint64_t)((unsigned __int128)x * y % t); };
        if (!inverse) { uint64_t pw = 1; for (uint32_t i = 0; i < n; i++) { a[i] = mulm(a[i], pw); pw = mulm(pw, psi); } }   // twist
        // cyclic NTT with omega = psi^2 (or its inverse), bit-reversal + iterative Cooley-Tukey
        const uint64_t omega = inverse ? mulm(ipsi, ipsi) : mulm(psi, psi);
        uint32_t lg = 0; while ((1u << lg) < n) lg++;
        for (uint32_t i = 0; i < n; i++) { uint32_t r = 0; for (uint32_t b = 0; b < lg; b++) r |= ((i >> b) & 1) << (lg - 1 - b); if (i < r) std::swap(a[i], a[r]); }
        for (uint32_t len = 2; len <= n; len <<= 1) {
            const uint64_t wl = pow_mod(omega, n / len, t);
            for (uint32_t i = 0; i < n; i += len) {
                uint64_t w = 1;
                for (uint32_t j = 0; j < len / 2; j++) {
                    const uint64_t u = a[i + j], v = mulm(a[i + j + len / 2], w);
                    a[i + j] = (u + v) % t; a[i + j + len / 2] = (u + t - v) % t; w = mulm(w, wl);
                }
            }
        }
        if (inverse) { uint64_t pw = 1; for (uint32_t i = 0; i < n; i++) { a[i] = mulm(mulm(a[i], ninv), pw); pw = mulm(pw, ipsi); } }   // untwist, scale
    }
    static void div_small(uint64_t q[4], const uint64_t x[4], uint64_t m) {         // q = floor(x / m)
        unsigned __int128 r = 0;
        for (int i = 3; i >= 0; i--) { const unsigned __int128 cur = (r << 64) | x[i]; q[i] = (uint64_t)(cur / m); r = cur % m; }
    }
    static void mul5(uint64_t out[5], const uint64_t x[4], uint64_t m) {             // the 320-bit product x m
        unsigned __int128 c = 0;
        for (int i = 0; i < 4; i++) { c += (unsigned __int128)x[i] * m; out[i] = (uint64_t)c; c >>= 64; }
        out[4] = (uint64_t)c;
    }
    // round(t mag / Q) = floor((2 t mag + Q) / (2 Q)) for mag <= Q / 2 < 2^254: at most t / 2 + 1, found bit by bit (Q is odd: no tie)
    static uint64_t round_scaled(const uint64_t mag[4], uint64_t t, const uint64_t Q[4]) {
        uint64_t num[5], Q2[4];
        mul5(num, mag, t);
        for (int i = 4; i > 0; i--) num[i] = (num[i] << 1) | (num[i - 1] >> 63);
        num[0] <<= 1;
        unsigned __int128 c = 0;
        for (int i = 0; i < 5; i++) { c += (unsigned __int128)num[i] + (i < 4 ? Q[i] : 0); num[i] = (uint64_t)c; c >>= 64; }
        for (int i = 3; i > 0; i--) Q2[i] = (Q[i] << 1) | (Q[i - 1] >> 63);
        Q2[0] = Q[0] << 1;
        uint64_t r = 0;
        for (int b = 63; b >= 0; b--) {
            uint64_t p[5];
            mul5(p, Q2, r | (1ull << b));
            bool above = false;
            for (int i = 4; i >= 0; i--) if (p[i] != num[i]) { above = p[i] > num[i]; break; }
            if (!above) r |= 1ull << b;
        }
        return r;
    }
    static void mul_small(uint64_t x[4], uint64_t m) {
        unsigned __int128 c = 0;
        for (int i = 0; i < 4; i++) { c += (unsigned __int128)x[i] * m; x[i] = (uint64_t)c; c >>= 64; }
    }
    static uint64_t mod_small(const uint64_t x[4], uint64_t m) {
        unsigned __int128 r = 0;
        for (int i = 3; i >= 0; i--) r = ((r << 64) | x[i]) % m;
        return (uint64_t)r;
    }
    static bool greater(const uint64_t a[4], const uint64_t b[4]) {
        for (int i = 3; i >= 0; i--) if (a[i] != b[i]) return a[i] > b[i];
        return false;
    }

    void init(const SecurityParams &params, const std::vector<uint256_t> &moduli) {
        params_.security = params;
        params_.n = params.poly_degree;
        params_.rns_moduli = moduli;
        params_.rns_ntt = new RNS_NTTEngine(params_.n, params_.rns_moduli.data(), (uint32_t)moduli.size());
    }
    static size_t galois_key_index(const GaloisKeys &gk, uint32_t g) {
        for (size_t i = 0; i < gk.elements.size(); i++) if (gk.elements[i] == g) return i;
        return (size_t)-1;
    }
    void copy_ciphertext(Ciphertext &dst, const Ciphertext &src) {
        for (size_t i = 0; i < src.components.size(); i++)
            check(fhe_hip_memcpy_d2d(dst.components[i]->coeffs, src.components[i]->coeffs, src.components[i]->count() * sizeof(uint256_t)), "ciphertext copy");
        dst.noise_budget = src.noise_budget; dst.level = src.level; dst.correction = src.correction;
    }
    // at least `num` components of the limbs of `level` (a component left over from another level is replaced)
    void ensure_components(Ciphertext &ct, size_t num, uint32_t level) {
        const uint32_t limbs = num_levels() - level;
        for (Polynomial *&p : ct.components) if (p->num_limbs != limbs) { delete p; p = new_polynomial(level); }
        while (ct.components.size() < num) ct.components.push_back(new_polynomial(level));   // the reference `new`s and never frees (src/fhe.cu:202-205)
    }
};

// include/fhe.cuh:150-157 (the reference's is a passthrough, src/fhe.cu:267-279): slots in the ROW order of the Galois section -- two rows of
// n / 2, rotate_rows shifts both cyclically, rotate_columns swaps them -- encoded and decoded on the device (fhe_slots_encode /
// fhe_slots_decode_poly).  The context is not const: it keeps the encoders.
class BatchEncoder {
public:
    explicit BatchEncoder(FHEContext &context) : ctx_(context), slot_count_(context.params().n) {}
    void encode(Plaintext &pt, const std::vector<uint64_t> &values) { ctx_.encode_slots(pt, values, FHE_SLOTS_ROWS); }
    void decode(std::vector<uint64_t> &values, const Plaintext &pt) { ctx_.decode_slots(values, pt, FHE_SLOTS_ROWS); }
    uint32_t slot_count() const { return slot_count_; }

private:
    FHEContext &ctx_;
    uint32_t slot_count_;
};

// CKKS encoder: n / 2 complex slots in the order of rotate_rows (a rotation by r is a cyclic left shift, the Galois element 2n - 1 conjugates),
// encoded and decoded on the device (fhe_ckks_encode / fhe_ckks_decode_poly).  encode writes round(scale m) mod q_l at `level`; decode reads limb 0
// centred modulo q_0, so it is the round trip of a plaintext whose coefficients stay below q_0 / 2.  The context is not const: it keeps the encoders.
class CKKSEncoder {
public:
    explicit CKKSEncoder(FHEContext &context) : ctx_(context), slot_count_(context.params().n / 2) {}
    void encode(Plaintext &pt, const std::vector<std::complex<double>> &values, double scale, uint32_t level = 0) { ctx_.ckks_encode(pt, values, scale, level); }
    void decode(std::vector<std::complex<double>> &values, const Plaintext &pt, double scale) { ctx_.ckks_decode(values, pt, scale); }
    uint32_t slot_count() const { return slot_count_; }

private:
    FHEContext &ctx_;
    uint32_t slot_count_;
};

}  // namespace fhe
