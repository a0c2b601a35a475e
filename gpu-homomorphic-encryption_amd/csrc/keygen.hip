// keygen.hip -- key-switching key generation (fhe_keyswitch_keys_generate; the key sets themselves: keys.hip) and, at the end, RGSW rows on the
// same two paths (fhe_rgsw_keys_generate).
// Fused path (plan_fused_keygen, a secret key with packed transforms, a cumulative table that fits the kernel; kernel: keygen.hip.h): the
// packed tables of every set are allocated, a table of (tables, Galois element) per set is uploaded and ONE launch fills them all; the
// Galois targets are gathered in the kernel from the packed transform of s.
// Composed path (everything else), one key set at a time: the uniform residues go straight into the set's `a` containers, which are
// NTT-domain by definition (sample_uniform_from); keygen_noise_kernel writes [noise_scale e] into the `b` containers, which are transformed;
// a^ . s^ row by row (do_ew) into scratch and one subtraction; keygen_gadget_kernel adds 2^(k w) target^ in limb j; then finish_key_set, as
// for an imported set.  Scratch: s^, target^ and the L K products, (L K + 2) S bytes.
#include "engine.h"

#include "ctr_rand.hip.h"

namespace fhe_dev {

// out[r][l][x] = [noise_scale e_P[x]]_{q_l}, P = first + r, on containers of any width class; one lane per (row, coefficient), the same small
// integer in every limb.  e is the Gaussian draw (gaussian_draw) of element P n + x.
__global__ void __launch_bounds__(256)
keygen_noise_kernel(u256 *__restrict__ out, const CrtLimb *__restrict__ limbs, uint32_t L, uint32_t log_n, uint64_t seed, uint64_t noise_scale,
                    const uint64_t *__restrict__ cdt, uint32_t cdt_len, size_t first /* polynomial */, size_t count /* rows * n */) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, n = (size_t)1 << log_n;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < count; o += stride) {
        const size_t r = o >> log_n, x = o & (n - 1);
        const GaussianDraw e = gaussian_draw(seed, ((first + r) << log_n) + x, cdt, cdt_len);
        for (uint32_t l = 0; l < L; l++) {
            const u256 q = limbs[l].q;
            store_u256(out + ((r * L + l) << log_n) + x, scaled_small_mod(e.mag, e.neg, noise_scale, q));
        }
    }
}

// kb[r][j][x] += (2^(k w) mod q_j) tgt[j][x] for row r = j K + k, NTT domain, containers of any width class: k w doublings modulo q_j;
// one lane per (row, position)
__global__ void __launch_bounds__(256)
keygen_gadget_kernel(u256 *__restrict__ kb, const u256 *__restrict__ tgt, const CrtLimb *__restrict__ limbs, uint32_t L, uint32_t log_n,
                     uint32_t K, uint32_t w, size_t count /* L K n */) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, n = (size_t)1 << log_n;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < count; o += stride) {
        const size_t r = o >> log_n, x = o & (n - 1);
        const uint32_t j = (uint32_t)(r / K), k = (uint32_t)(r % K);
        const u256 q = limbs[j].q;
        u256 v = load_u256(tgt + ((size_t)j << log_n) + x);
        for (uint32_t d = 0; d < k * w; d++) v = add_mod(v, v, q);
        u256 *at = kb + ((r * L + j) << log_n) + x;
        store_u256(at, add_mod(load_u256(at), v, q));
    }
}

// tgt[l][x] = [mu]_{q_l} (by_s == 0: the constant polynomial mu, the same value at every NTT position) or [mu]_{q_l} sh[l][x] (by_s: mu s^), the
// target of an RGSW component (fhe_rgsw_keys_generate, composed path); |mu| = mag by double-and-add, then the sign.  One lane per (limb, position)
__global__ void __launch_bounds__(256)
rgsw_target_kernel(u256 *__restrict__ tgt, const u256 *__restrict__ sh, const CrtLimb *__restrict__ limbs, uint32_t log_n, uint32_t mag, uint32_t neg,
                   uint32_t by_s, size_t count /* L n */) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < count; o += stride) {
        const u256 q = limbs[o >> log_n].q;
        u256 v = by_s ? load_u256(sh + o) : u256_small(1), acc = u256_small(0);
        for (uint32_t k = mag; k; k >>= 1) { if (k & 1) acc = add_mod(acc, v, q); v = add_mod(v, v, q); }
        store_u256(tgt + o, neg ? sub_mod(u256_small(0), acc, q) : acc);
    }
}

}  // namespace fhe_dev

// one set on the composed path: rows first .. first + L K - 1 of the call's streams; sh = s^ as containers, tgt = the set's target^
static int generate_composed(fhe_rns_ntt *h, fhe_relin_keys *rk, const void *sh, const void *tgt, char *prod, size_t first, uint64_t noise_scale,
                             const uint64_t seeds[2], bool packed) {
    const uint32_t LK = rk->num_keys;
    const size_t S = (size_t)h->L * h->n * 32, count = (size_t)LK * h->n;
    int rc;
    HIP_TRY(hipMalloc(&rk->d_kb, S * LK));
    HIP_TRY(hipMalloc(&rk->d_ka, S * LK));
    if ((rc = sample_uniform_from(h, rk->d_ka, seeds[0], first * h->L, (size_t)LK * h->L))) return rc;
    hipLaunchKernelGGL(fhe_dev::keygen_noise_kernel, dim3(ew_grid(count)), dim3(256), 0, h->stream, (fhe_dev::u256 *)rk->d_kb, (const fhe_dev::CrtLimb *)h->d_crt,
                       h->L, h->log_n, seeds[1], noise_scale, (const uint64_t *)h->d_cdt, h->cdt_len, first, count);
    if ((rc = post_launch(h->stream, "keygen_noise_kernel"))) return rc;
    if ((rc = do_forward(h, rk->d_kb, LK))) return rc;
    for (uint32_t r = 0; r < LK; r++)
        if ((rc = do_ew<0>(h, prod + r * S, (const char *)rk->d_ka + r * S, sh, 1, "keygen a . s"))) return rc;
    if ((rc = do_ew<2>(h, rk->d_kb, rk->d_kb, prod, LK, "keygen e - a . s"))) return rc;
    hipLaunchKernelGGL(fhe_dev::keygen_gadget_kernel, dim3(ew_grid(count)), dim3(256), 0, h->stream, (fhe_dev::u256 *)rk->d_kb, (const fhe_dev::u256 *)tgt,
                       (const fhe_dev::CrtLimb *)h->d_crt, h->L, h->log_n, rk->K, rk->decomp_bits, count);
    if ((rc = post_launch(h->stream, "keygen_gadget_kernel"))) return rc;
    return finish_key_set(h, rk, packed);
}

extern "C" int fhe_keyswitch_keys_generate(fhe_rns_ntt_t *h, const fhe_secret_key_t *sk, uint32_t decomp_bits, const uint32_t *galois_elts,
                                           uint32_t num_sets, uint64_t noise_scale, double sigma, const uint64_t seeds[2], fhe_relin_keys_t **out_sets) {
    int rc = check_call(h, 1, "keyswitch_keys_generate"); if (rc) return rc;
    if (!sk || !galois_elts || !seeds || !out_sets) return fail(FHE_ERR_INVALID_ARG, "keyswitch_keys_generate: null argument");
    if (sk->owner != h) return fail(FHE_ERR_INVALID_ARG, "keyswitch_keys_generate: the key was imported for a different engine");
    if (!num_sets) return fail(FHE_ERR_INVALID_ARG, "keyswitch_keys_generate: num_sets must be at least 1");
    if (decomp_bits < 1 || decomp_bits > 64) return fail(FHE_ERR_INVALID_ARG, "keyswitch_keys_generate: decomp_bits must be in [1, 64]");
    for (uint32_t e = 0; e < num_sets; e++)
        if (galois_elts[e] && (rc = check_galois_element(h, galois_elts[e], "keyswitch_keys_generate"))) return rc;
    if (!noise_scale) return fail(FHE_ERR_INVALID_ARG, "keyswitch_keys_generate: noise_scale must not be 0");
    const uint32_t K = relin_digits(h, decomp_bits), LK = h->L * K;
    if ((uint64_t)num_sets * LK * h->L > 0x7fffffffull) return fail(FHE_ERR_INVALID_ARG, "keyswitch_keys_generate: num_sets * num_primes^2 * digits too large");
    if ((rc = ensure_cdt(h, sigma, "keyswitch_keys_generate"))) return rc;      // rejects 12 sigma >= the smallest modulus before it allocates
    (void)hipGetLastError();

    const bool packed = keys_get_packed(h, decomp_bits, K);
    const bool fused = plan_fused_keygen(h, packed) && sk->d_packed && h->cdt_len <= fhe_dev::ENCRYPT_MAX_CDT;
    const size_t S = (size_t)h->L * h->n * 32, table = LK * packed_row_bytes(h);
    std::vector<fhe_relin_keys *> sets(num_sets, nullptr);
    Scratch scratch;
    auto body = [&]() -> int {
        for (uint32_t e = 0; e < num_sets; e++)
            if (!(sets[e] = new_key_set(h, decomp_bits, K))) return fail(FHE_ERR_INVALID_ARG, "out of host memory");
        if (fused) {
            std::vector<fhe_dev::KeygenSet> tab(num_sets);
            for (uint32_t e = 0; e < num_sets; e++) {
                HIP_TRY(hipMalloc(&sets[e]->d_pkb, table));
                HIP_TRY(hipMalloc(&sets[e]->d_pka, table));
                tab[e] = {sets[e]->d_pkb, sets[e]->d_pka, galois_elts[e], 0u};
            }
            void *d_tab = nullptr;
            if (int r = scratch.get(&d_tab, num_sets * sizeof(fhe_dev::KeygenSet))) return r;
            HIP_TRY(hipMemcpy(d_tab, tab.data(), num_sets * sizeof(fhe_dev::KeygenSet), hipMemcpyHostToDevice));
            fhe_dev::LdsArgs A = lds_args(h, fhe_dev::LDS_KEYGEN, {}, num_sets * LK * h->L);
            A.a0 = d_tab; A.kb = sk->d_packed; A.ka = (const char *)sk->d_packed + packed_row_bytes(h);
            A.cdt = h->d_cdt; A.cdt_len = h->cdt_len; A.seeds[0] = seeds[0]; A.seeds[1] = seeds[1]; A.t = noise_scale; A.K = K; A.w = decomp_bits;
            if (int r = lds_launch(h, A, "ntt_keygen_kernel")) return r;
            for (fhe_relin_keys *rk : sets) (void)finish_key_set(h, rk, packed);     // the kernel wrote the packed tables: K for fhe_rns_ntt_reserve only
        } else {
            if (int r = ensure_crt(h)) return r;
            void *sh = nullptr, *tgt = nullptr, *prod = nullptr;
            int r;
            if ((r = scratch.get(&sh, S)) || (r = scratch.get(&tgt, S)) || (r = scratch.get(&prod, S * LK))) return r;
            HIP_TRY(hipMemcpyAsync(sh, sk->d_s, S, hipMemcpyDeviceToDevice, h->stream));
            if ((r = do_forward(h, sh, 1))) return r;
            for (uint32_t e = 0; e < num_sets; e++) {
                if (!galois_elts[e]) HIP_TRY(hipMemcpyAsync(tgt, (const char *)sk->d_s + S, S, hipMemcpyDeviceToDevice, h->stream));
                else if ((r = do_galois(h, tgt, nullptr, nullptr, sk->d_s, nullptr, galois_elts[e], h->L, false))) return r;
                if ((r = do_forward(h, tgt, 1))) return r;
                if ((r = generate_composed(h, sets[e], sh, tgt, (char *)prod, (size_t)e * LK, noise_scale, seeds, packed))) return r;
            }
        }
        HIP_TRY(hipStreamSynchronize(h->stream));     // the scratch is freed when the call returns; the keys are complete then
        return FHE_OK;
    };
    rc = body();
    if (rc) {
        (void)hipStreamSynchronize(h->stream);
        for (fhe_relin_keys *rk : sets) fhe_relin_keys_destroy(rk);
        for (uint32_t e = 0; e < num_sets; e++) out_sets[e] = nullptr;
        return rc;
    }
    for (uint32_t e = 0; e < num_sets; e++) out_sets[e] = sets[e];
    return FHE_OK;
}

// RGSW ciphertexts of small messages (the bootstrapping key of a blind rotation): the same rows with the gadget term mu (component 0) or
// mu s (component 1); half e = 2 i + c of the call is "set" e of the streams.  Fused where fhe_keyswitch_keys_generate is (ONE launch of the
// sibling kernel, which reads s^ only); else generate_composed with target^ = mu at every position, or mu s^ (rgsw_target_kernel).
extern "C" int fhe_rgsw_keys_generate(fhe_rns_ntt_t *h, const fhe_secret_key_t *sk, uint32_t decomp_bits, const int32_t *mu, uint32_t num,
                                      uint64_t noise_scale, double sigma, const uint64_t seeds[2], fhe_relin_keys_t **out_rows_c0,
                                      fhe_relin_keys_t **out_rows_c1) {
    int rc = check_call(h, 1, "rgsw_keys_generate"); if (rc) return rc;
    if (!word_sized_moduli(h)) return fail(FHE_ERR_UNSUPPORTED, "rgsw_keys_generate: every modulus must be below 2^64");
    if (!sk || !mu || !seeds || !out_rows_c0 || !out_rows_c1) return fail(FHE_ERR_INVALID_ARG, "rgsw_keys_generate: null argument");
    if (out_rows_c0 == out_rows_c1) return fail(FHE_ERR_INVALID_ARG, "rgsw_keys_generate: the two output arrays must be distinct");
    if (sk->owner != h) return fail(FHE_ERR_INVALID_ARG, "rgsw_keys_generate: the key was imported for a different engine");
    if (!num) return fail(FHE_ERR_INVALID_ARG, "rgsw_keys_generate: num must be at least 1");
    if (decomp_bits < 1 || decomp_bits > 64) return fail(FHE_ERR_INVALID_ARG, "rgsw_keys_generate: decomp_bits must be in [1, 64]");
    for (uint32_t i = 0; i < num; i++)
        if (mu[i] > (1 << 15) || mu[i] < -(1 << 15)) return fail(FHE_ERR_INVALID_ARG, "rgsw_keys_generate: |mu| must not exceed 2^15");
    if (!noise_scale) return fail(FHE_ERR_INVALID_ARG, "rgsw_keys_generate: noise_scale must not be 0");
    const uint32_t K = relin_digits(h, decomp_bits), LK = h->L * K;
    if (2ull * num * LK * h->L > 0x7fffffffull) return fail(FHE_ERR_INVALID_ARG, "rgsw_keys_generate: num * num_primes^2 * digits too large");
    if ((rc = ensure_cdt(h, sigma, "rgsw_keys_generate"))) return rc;
    (void)hipGetLastError();

    const bool packed = keys_get_packed(h, decomp_bits, K);
    const bool fused = plan_fused_keygen(h, packed) && sk->d_packed && h->cdt_len <= fhe_dev::ENCRYPT_MAX_CDT;
    const size_t S = (size_t)h->L * h->n * 32, table = LK * packed_row_bytes(h);
    const uint32_t halves = 2 * num;
    std::vector<fhe_relin_keys *> sets(halves, nullptr);          // [2 i + c]
    Scratch scratch;
    auto body = [&]() -> int {
        for (uint32_t e = 0; e < halves; e++)
            if (!(sets[e] = new_key_set(h, decomp_bits, K))) return fail(FHE_ERR_INVALID_ARG, "out of host memory");
        if (fused) {
            std::vector<fhe_dev::RgswSet> tab(halves);
            for (uint32_t e = 0; e < halves; e++) {
                HIP_TRY(hipMalloc(&sets[e]->d_pkb, table));
                HIP_TRY(hipMalloc(&sets[e]->d_pka, table));
                tab[e] = {sets[e]->d_pkb, sets[e]->d_pka, mu[e / 2], e & 1u};
            }
            void *d_tab = nullptr;
            if (int r = scratch.get(&d_tab, halves * sizeof(fhe_dev::RgswSet))) return r;
            HIP_TRY(hipMemcpy(d_tab, tab.data(), halves * sizeof(fhe_dev::RgswSet), hipMemcpyHostToDevice));
            fhe_dev::LdsArgs A = lds_args(h, fhe_dev::LDS_RGSW_KEYGEN, {}, halves * LK * h->L);
            A.a0 = d_tab; A.kb = sk->d_packed;
            A.cdt = h->d_cdt; A.cdt_len = h->cdt_len; A.seeds[0] = seeds[0]; A.seeds[1] = seeds[1]; A.t = noise_scale; A.K = K; A.w = decomp_bits;
            if (int r = lds_launch(h, A, "ntt_rgsw_keygen_kernel")) return r;
            for (fhe_relin_keys *rk : sets) (void)finish_key_set(h, rk, packed);     // the kernel wrote the packed tables: K for fhe_rns_ntt_reserve only
        } else {
            if (int r = ensure_crt(h)) return r;
            void *sh = nullptr, *tgt = nullptr, *prod = nullptr;
            int r;
            if ((r = scratch.get(&sh, S)) || (r = scratch.get(&tgt, S)) || (r = scratch.get(&prod, S * LK))) return r;
            HIP_TRY(hipMemcpyAsync(sh, sk->d_s, S, hipMemcpyDeviceToDevice, h->stream));
            if ((r = do_forward(h, sh, 1))) return r;
            const size_t count = (size_t)h->L * h->n;
            for (uint32_t e = 0; e < halves; e++) {
                const int32_t m = mu[e / 2];
                hipLaunchKernelGGL(fhe_dev::rgsw_target_kernel, dim3(ew_grid(count)), dim3(256), 0, h->stream, (fhe_dev::u256 *)tgt, (const fhe_dev::u256 *)sh,
                                   (const fhe_dev::CrtLimb *)h->d_crt, h->log_n, m < 0 ? 0u - (uint32_t)m : (uint32_t)m, m < 0 ? 1u : 0u, e & 1u, count);
                if ((r = post_launch(h->stream, "rgsw_target_kernel"))) return r;
                if ((r = generate_composed(h, sets[e], sh, tgt, (char *)prod, (size_t)e * LK, noise_scale, seeds, packed))) return r;
            }
        }
        HIP_TRY(hipStreamSynchronize(h->stream));     // the scratch is freed when the call returns; the keys are complete then
        return FHE_OK;
    };
    rc = body();
    if (rc) {
        (void)hipStreamSynchronize(h->stream);
        for (fhe_relin_keys *rk : sets) fhe_relin_keys_destroy(rk);
        for (uint32_t i = 0; i < num; i++) out_rows_c0[i] = out_rows_c1[i] = nullptr;
        return rc;
    }
    for (uint32_t i = 0; i < num; i++) { out_rows_c0[i] = sets[2 * i]; out_rows_c1[i] = sets[2 * i + 1]; }
    return FHE_OK;
}
