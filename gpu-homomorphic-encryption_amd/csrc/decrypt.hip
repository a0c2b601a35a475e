// decrypt.hip -- secret-key decryption (fhe_ct_decrypt*; the keys: keys.hip).
// Fused path (plan_fused_decrypt; kernels: decrypt.hip.h): the key is kept transformed, with its pointwise square, packed like one key row each;
// a call is two launches, ntt_decrypt_kernel into the compact decryption workspace WS_DEC and decrypt_crt_kernel from it.  Composed path
// (full-width class, sizes outside the LDS-resident range, FHE_HIP_NO_FUSED_DECRYPT=1): fhe_rns_ntt_multiply_bcast against s (and against the
// s^2 built at import), fhe_rns_poly_add into container scratch in WS_DEC, then the CRT kernel on containers.
#include "engine.h"

#include "ntt_word.hip.h"
#define FHE_DECRYPT_CRT_KERNELS
#include "decrypt.hip.h"

static int decrypt_q_fits(fhe_rns_ntt *h, const char *what) {
    if (int rc = ensure_crt(h)) return rc;
    if (h->crt_state < 0) return fail(FHE_ERR_UNSUPPORTED, std::string(what) + ": the product of the moduli must be below 2^255 (the noise bits need the integer itself, which has to fit a 256-bit container)");
    return FHE_OK;
}
// everything a call with `num_components` components and `batch` ciphertexts needs: the CRT tables and WS_DEC (compact residues on the fused
// path; containers for c1 s and, with c2, c2 s^2 on the composed path, whose products also need the multiply workspaces)
static int ensure_decrypt(fhe_rns_ntt *h, uint32_t num_components, uint32_t batch) {
    int rc;
    if (h->width != FHE_WIDTH_256 && (rc = ensure_from_rns_word(h))) return rc;
    const size_t polys = (size_t)batch * h->L;
    if (plan_fused_decrypt(h)) return grow_ws(h, h->ws[WS_DEC], polys * h->n * residue_bytes(h));
    if ((rc = ensure_need(h, need_multiply(h, batch) | need_multiply(h, 1) | need_transform(h, polys)))) return rc;
    return grow_ws(h, h->ws[WS_DEC], (num_components - 1) * polys * h->n * 32);
}
extern "C" int fhe_ct_decrypt_reserve(fhe_rns_ntt_t *h, uint64_t t, uint32_t num_components, uint32_t batch) {
    int rc = check_call(h, batch, "ct_decrypt_reserve"); if (rc) return rc;
    if (num_components != 2 && num_components != 3) return fail(FHE_ERR_INVALID_ARG, "ct_decrypt_reserve: 2 or 3 components");
    if (t < 2) return fail(FHE_ERR_INVALID_ARG, "ct_decrypt_reserve: the plaintext modulus t must be at least 2");
    if ((rc = decrypt_q_fits(h, "ct_decrypt_reserve"))) return rc;
    return ensure_decrypt(h, num_components, batch);       // (the constants of t are kernel arguments: nothing to keep per t)
}
extern "C" int fhe_ct_decrypt(fhe_rns_ntt_t *h, const fhe_secret_key_t *sk, uint64_t t, uint64_t scale, uint64_t *d_m, uint32_t *d_noise_bits,
                              const void *const *d_components, uint32_t num_components, uint32_t batch) {
    int rc = check_call(h, batch, "ct_decrypt"); if (rc) return rc;
    if (!sk || !d_m || !d_components) return fail(FHE_ERR_INVALID_ARG, "ct_decrypt: null argument");
    if (num_components != 2 && num_components != 3) return fail(FHE_ERR_INVALID_ARG, "ct_decrypt: 2 or 3 components");
    if (sk->owner != h) return fail(FHE_ERR_INVALID_ARG, "ct_decrypt: the key was imported for a different engine");
    const void *c[3] = {nullptr, nullptr, nullptr};
    for (uint32_t k = 0; k < num_components; k++) {
        if (!(c[k] = d_components[k])) return fail(FHE_ERR_INVALID_ARG, "ct_decrypt: null component pointer");
        if ((rc = check_aligned({c[k]}, "ct_decrypt"))) return rc;
    }
    if ((rc = check_aligned({d_m}, "ct_decrypt"))) return rc;
    if ((uintptr_t)d_noise_bits & 3) return fail(FHE_ERR_INVALID_ARG, "ct_decrypt: d_noise_bits must be 4-byte aligned");
    if ((const void *)d_m == (const void *)d_noise_bits) return fail(FHE_ERR_INVALID_ARG, "ct_decrypt: outputs must be distinct");
    for (const void *i : {c[0], c[1], c[2], sk->src, (const void *)sk->d_s})
        if (i && ((const void *)d_m == i || (d_noise_bits && (const void *)d_noise_bits == i)))
            return fail(FHE_ERR_INVALID_ARG, "ct_decrypt: outputs must not alias the components or the key");
    if (t < 2) return fail(FHE_ERR_INVALID_ARG, "ct_decrypt: the plaintext modulus t must be at least 2");
    if (!scale || scale >= t) return fail(FHE_ERR_INVALID_ARG, "ct_decrypt: scale must be in [1, t)");
    if ((rc = decrypt_q_fits(h, "ct_decrypt"))) return rc;
    if ((rc = check_inputs(h, {c[0], c[1]}, batch)) || (c[2] && (rc = check_inputs(h, {c[2]}, batch)))) return rc;
    if ((rc = ensure_decrypt(h, num_components, batch))) return rc;             // (no-op after fhe_ct_decrypt_reserve)
    fhe_host::ModT M; fhe_host::modt_init(M, t);
    const size_t S = (size_t)h->L * h->n * 32, count = (size_t)batch * h->n;
    const bool fused = sk->d_packed && plan_fused_decrypt(h);
    const void *res = h->ws[WS_DEC].p;
    if (fused) {
        fhe_dev::LdsArgs A = lds_args(h, fhe_dev::LDS_DECRYPT, {}, batch * h->L);
        A.r0 = h->ws[WS_DEC].p; A.a0 = c[0]; A.a1 = c[1]; A.c2 = c[2]; A.kb = sk->d_packed; A.ka = (const char *)sk->d_packed + packed_row_bytes(h); A.out_compact = true;
        if ((rc = lds_launch(h, A, "ntt_decrypt_kernel"))) return rc;
    } else {
        char *p0 = (char *)h->ws[WS_DEC].p, *p1 = p0 + (size_t)batch * S;
        if ((rc = fhe_rns_ntt_multiply_bcast(h, p0, c[1], sk->d_s, batch))) return rc;
        if (c[2]) {
            if ((rc = fhe_rns_ntt_multiply_bcast(h, p1, c[2], (const char *)sk->d_s + S, batch))) return rc;
            if ((rc = fhe_rns_poly_add(h, p0, p0, p1, batch))) return rc;
        }
        if ((rc = fhe_rns_poly_add(h, p0, p0, c[0], batch))) return rc;
    }
    if (d_noise_bits) HIP_TRY(hipMemsetAsync(d_noise_bits, 0, (size_t)batch * sizeof(uint32_t), h->stream));
    if (h->width == FHE_WIDTH_256) {
        hipLaunchKernelGGL(fhe_dev::decrypt_crt256_kernel, dim3(ew_grid(count)), dim3(256), 0, h->stream, d_m, d_noise_bits, (const fhe_dev::u256 *)res,
                           (const fhe_dev::CrtLimb *)h->d_crt, h->crt_big, M, scale, h->L, h->log_n, count);
        return post_launch(h->stream, "decrypt_crt256_kernel");
    }
    return with_word_field(h, [&](auto f) {
        using F = decltype(f); using E = typename F::E;
        auto launch = [&](auto COMPACT) {
            hipLaunchKernelGGL((fhe_dev::decrypt_crt_kernel<F, decltype(COMPACT)::value>), dim3(ew_grid(count)), dim3(256), 0, h->stream, d_m, d_noise_bits, res,
                               (const fhe_dev::Limb<F> *)h->d_limbs, (const E *)h->d_from_rns_w_minv, (const fhe_dev::u256 *)h->d_from_rns_w_M, h->crt_big.Q, M, scale,
                               h->L, h->log_n, count);
        };
        if (fused) launch(std::true_type{}); else launch(std::false_type{});
        return post_launch(h->stream, "decrypt_crt_kernel");
    });
}
