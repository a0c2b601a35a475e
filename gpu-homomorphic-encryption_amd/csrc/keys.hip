// keys.hip -- the lifetime of every key object (fhe_relin_keys_*, fhe_secret_key_*, fhe_public_key_*) and the packing they share: rows of
// NTT-domain containers into the register order of the fused kernels and back (pack_keys_kernel / unpack_keys_kernel, launched here only).
// A key is kept as given (containers) for the composed paths and, where the fused kernels run, transformed and packed like one key row each.
#include "engine.h"

#include "ntt_word.hip.h"

int pack_rows(fhe_rns_ntt *h, void *dst, const void *src, uint32_t rows, const char *what) {
    return with_word_field(h, [&](auto f) {
        using F = decltype(f);
        hipLaunchKernelGGL((fhe_dev::pack_keys_kernel<F>), dim3(ew_grid((size_t)rows * h->L * h->n)), dim3(256), 0, h->stream, (typename F::E *)dst,
                           (const typename F::V16 *)src, (const fhe_dev::Limb<F> *)h->d_limbs, h->L, h->log_n, rows);
        return post_launch(h->stream, what);
    });
}
int unpack_rows(fhe_rns_ntt *h, void *dst, const void *src, uint32_t rows, const char *what) {
    return with_word_field(h, [&](auto f) {
        using F = decltype(f);
        hipLaunchKernelGGL((fhe_dev::unpack_keys_kernel<F>), dim3(ew_grid((size_t)rows * h->L * h->n * 2)), dim3(256), 0, h->stream, (typename F::V16 *)dst,
                           (const typename F::E *)src, (const fhe_dev::Limb<F> *)h->d_limbs, h->L, h->log_n, rows);
        return post_launch(h->stream, what);
    });
}

// ---- key-switching key sets -----------------------------------------------------------------------------------------------------
fhe_relin_keys *new_key_set(fhe_rns_ntt *h, uint32_t decomp_bits, uint32_t K) {
    fhe_relin_keys *rk = new (std::nothrow) fhe_relin_keys();
    if (rk) { rk->owner = h; rk->decomp_bits = decomp_bits; rk->K = K; rk->num_keys = h->L * K; }
    return rk;
}
int finish_key_set(fhe_rns_ntt *h, fhe_relin_keys *rk, bool packed) {
    if (packed && rk->d_kb) {
        const size_t table = rk->num_keys * packed_row_bytes(h);
        HIP_TRY(hipMalloc(&rk->d_pkb, table));
        HIP_TRY(hipMalloc(&rk->d_pka, table));
        if (int rc = pack_rows(h, rk->d_pkb, rk->d_kb, rk->num_keys, "pack_keys_kernel")) return rc;
        if (int rc = pack_rows(h, rk->d_pka, rk->d_ka, rk->num_keys, "pack_keys_kernel")) return rc;
        // the fused kernels read only the packed tables (n * sizeof(E) bytes per key polynomial instead of n * 32): drop the container
        // copy, so that a bootstrapping key of several hundred RGSW ciphertexts fits (hipFree waits for the packing)
        (void)hipFree(rk->d_kb); (void)hipFree(rk->d_ka);
        rk->d_kb = rk->d_ka = nullptr;
    }
    if (rk->K > h->max_digits) h->max_digits = rk->K;                              // fhe_rns_ntt_reserve sizes the key-switch workspaces for it
    if (!packed && rk->K > h->max_composed_digits) h->max_composed_digits = rk->K;  // this set runs the composed key switch (digit polynomials in the workspace)
    return FHE_OK;
}
extern "C" int fhe_relin_keys_destroy(fhe_relin_keys_t *rk) {
    if (rk) {
        for (void *p : {rk->d_kb, rk->d_ka, rk->d_pkb, rk->d_pka}) if (p) (void)hipFree(p);
        delete rk;
    }
    return FHE_OK;
}
extern "C" int fhe_relin_keys_create(fhe_rns_ntt_t *h, fhe_relin_keys_t **out, uint32_t decomp_bits,
                                     const void *const *d_keys_b, const void *const *d_keys_a, uint32_t num_keys) {
    if (!h || !out || !d_keys_b || !d_keys_a) return fail(FHE_ERR_INVALID_ARG, "relin_keys_create: null argument");
    *out = nullptr;
    if (decomp_bits < 1 || decomp_bits > 64) return fail(FHE_ERR_INVALID_ARG, "decomp_bits must be in [1, 64]");
    const uint32_t K = relin_digits(h, decomp_bits);
    if (num_keys != h->L * K) {
        char buf[128]; snprintf(buf, sizeof buf, "relin_keys_create: expected %u keys (L = %u limbs x K = %u digits), got %u", h->L * K, h->L, K, num_keys);
        return fail(FHE_ERR_INVALID_ARG, buf);
    }
    for (uint32_t i = 0; i < num_keys; i++) if (!d_keys_b[i] || !d_keys_a[i]) return fail(FHE_ERR_INVALID_ARG, "relin_keys_create: null key pointer");
    for (uint32_t i = 0; i < num_keys; i++) if (int rc = check_aligned({d_keys_b[i], d_keys_a[i]}, "relin_keys_create")) return rc;
    (void)hipGetLastError();
    fhe_relin_keys *rk = new_key_set(h, decomp_bits, K);
    if (!rk) return fail(FHE_ERR_INVALID_ARG, "out of host memory");
    const size_t S = (size_t)h->L * h->n * 32;
    auto body = [&]() -> int {
        auto hip = [](hipError_t e, const char *what) { return e == hipSuccess ? FHE_OK : fail(FHE_ERR_HIP, std::string(what) + hipGetErrorString(e)); };   // HIP_TRY with this entry point's own prefixes
        int rc;
        if ((rc = hip(hipMalloc(&rk->d_kb, S * num_keys), "relin_keys_create: ")) || (rc = hip(hipMalloc(&rk->d_ka, S * num_keys), "relin_keys_create: "))) return rc;
        for (uint32_t i = 0; i < num_keys; i++)
            if ((rc = hip(hipMemcpyAsync((char *)rk->d_kb + i * S, d_keys_b[i], S, hipMemcpyDeviceToDevice, h->stream), "relin_keys_create copy: ")) ||
                (rc = hip(hipMemcpyAsync((char *)rk->d_ka + i * S, d_keys_a[i], S, hipMemcpyDeviceToDevice, h->stream), "relin_keys_create copy: "))) return rc;
        if ((rc = do_forward(h, rk->d_kb, num_keys)) || (rc = do_forward(h, rk->d_ka, num_keys))) return rc;
        return finish_key_set(h, rk, keys_get_packed(h, decomp_bits, K));
    };
    if (int rc = body()) { fhe_relin_keys_destroy(rk); return rc; }
    *out = rk;
    return FHE_OK;
}
extern "C" int fhe_relin_keys_export(fhe_rns_ntt_t *h, const fhe_relin_keys_t *rk, void *d_keys_b, void *d_keys_a) {
    int rc = check_call(h, 1, "relin_keys_export"); if (rc) return rc;
    if (!rk || !d_keys_b || !d_keys_a) return fail(FHE_ERR_INVALID_ARG, "relin_keys_export: null argument");
    if ((rc = check_aligned({d_keys_b, d_keys_a}, "relin_keys_export"))) return rc;
    if (rk->owner != h) return fail(FHE_ERR_INVALID_ARG, "relin_keys_export: keys were imported for a different engine");
    if (d_keys_b == d_keys_a) return fail(FHE_ERR_INVALID_ARG, "relin_keys_export: outputs must be distinct");
    void *outs[2] = {d_keys_b, d_keys_a};
    const void *cont[2] = {rk->d_kb, rk->d_ka}, *pk[2] = {rk->d_pkb, rk->d_pka};
    for (int c = 0; c < 2; c++) {
        if (cont[c]) HIP_TRY(hipMemcpyAsync(outs[c], cont[c], (size_t)rk->num_keys * h->L * h->n * 32, hipMemcpyDeviceToDevice, h->stream));
        else if (pk[c]) { if ((rc = unpack_rows(h, outs[c], pk[c], rk->num_keys, "unpack_keys_kernel"))) return rc; }
        else return fail(FHE_ERR_INVALID_ARG, "relin_keys_export: the key set holds no tables");
        if ((rc = do_inverse(h, outs[c], rk->num_keys))) return rc;
    }
    return FHE_OK;
}

// ---- secret and public keys -----------------------------------------------------------------------------------------------------
extern "C" int fhe_secret_key_destroy(fhe_secret_key_t *sk) {
    if (sk) {
        for (void *p : {sk->d_s, sk->d_packed}) if (p) (void)hipFree(p);
        delete sk;
    }
    return FHE_OK;
}
extern "C" int fhe_secret_key_create(fhe_rns_ntt_t *h, fhe_secret_key_t **out, const void *d_s) {
    if (!h || !out || !d_s) return fail(FHE_ERR_INVALID_ARG, "secret_key_create: null argument");
    int rc = check_aligned({d_s}, "secret_key_create"); if (rc) return rc;
    (void)hipGetLastError();
    fhe_secret_key *sk = new (std::nothrow) fhe_secret_key();
    if (!sk) return fail(FHE_ERR_INVALID_ARG, "out of host memory");
    sk->owner = h; sk->src = d_s;
    const size_t S = (size_t)h->L * h->n * 32;
    Scratch scratch;
    auto body = [&]() -> int {
        HIP_TRY(hipMalloc(&sk->d_s, 2 * S));
        HIP_TRY(hipMemcpyAsync(sk->d_s, d_s, S, hipMemcpyDeviceToDevice, h->stream));
        if (int r = fhe_rns_ntt_multiply(h, (char *)sk->d_s + S, sk->d_s, sk->d_s, 1)) return r;
        if (plan_fused_decrypt(h)) {
            void *d_tr = nullptr;                    // (s^, s^ . s^), containers
            if (int r = scratch.get(&d_tr, 2 * S)) return r;
            HIP_TRY(hipMemcpyAsync(d_tr, sk->d_s, S, hipMemcpyDeviceToDevice, h->stream));
            if (int r = do_forward(h, d_tr, 1)) return r;
            if (int r = fhe_rns_ntt_pointwise(h, (char *)d_tr + S, d_tr, d_tr, 1)) return r;
            HIP_TRY(hipMalloc(&sk->d_packed, 2 * packed_row_bytes(h)));
            if (int r = pack_rows(h, sk->d_packed, d_tr, 2, "pack_keys_kernel (secret key)")) return r;
        }
        HIP_TRY(hipStreamSynchronize(h->stream));     // the scratch is freed when the call returns; the import is complete then
        return FHE_OK;
    };
    if ((rc = body())) { fhe_secret_key_destroy(sk); return rc; }
    *out = sk;
    return FHE_OK;
}

extern "C" int fhe_public_key_destroy(fhe_public_key_t *pk) {
    if (pk) {
        for (void *p : {pk->d_pk, pk->d_packed}) if (p) (void)hipFree(p);
        delete pk;
    }
    return FHE_OK;
}
extern "C" int fhe_public_key_create(fhe_rns_ntt_t *h, fhe_public_key_t **out, const void *d_pk0, const void *d_pk1) {
    if (!h || !out || !d_pk0 || !d_pk1) return fail(FHE_ERR_INVALID_ARG, "public_key_create: null argument");
    int rc = check_aligned({d_pk0, d_pk1}, "public_key_create"); if (rc) return rc;
    (void)hipGetLastError();
    fhe_public_key *pk = new (std::nothrow) fhe_public_key();
    if (!pk) return fail(FHE_ERR_INVALID_ARG, "out of host memory");
    pk->owner = h; pk->src0 = d_pk0; pk->src1 = d_pk1;
    const size_t S = (size_t)h->L * h->n * 32;
    Scratch scratch;
    auto body = [&]() -> int {
        HIP_TRY(hipMalloc(&pk->d_pk, 2 * S));
        HIP_TRY(hipMemcpyAsync(pk->d_pk, d_pk0, S, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync((char *)pk->d_pk + S, d_pk1, S, hipMemcpyDeviceToDevice, h->stream));
        if (!plan_fused_encrypt(h)) return post_launch(h->stream, "public_key_create copy");
        void *d_tr = nullptr;                        // the transformed copy, containers
        if (int r = scratch.get(&d_tr, 2 * S)) return r;
        HIP_TRY(hipMemcpyAsync(d_tr, pk->d_pk, 2 * S, hipMemcpyDeviceToDevice, h->stream));
        if (int r = do_forward(h, d_tr, 2)) return r;
        HIP_TRY(hipMalloc(&pk->d_packed, 2 * packed_row_bytes(h)));
        if (int r = pack_rows(h, pk->d_packed, d_tr, 2, "pack_keys_kernel (public key)")) return r;
        HIP_TRY(hipStreamSynchronize(h->stream));     // the scratch is freed when the call returns
        return FHE_OK;
    };
    if ((rc = body())) { fhe_public_key_destroy(pk); return rc; }
    *out = pk;
    return FHE_OK;
}
