// lwe_keyswitch.hip -- the LWE key switch that closes the bootstrapping loop: an LWE sample under the ring key (fhe_rlwe_sample_extract on a
// one-limb engine) becomes an LWE ciphertext under the small key z, optionally switched to another modulus in the same launch, ready for the
// next fhe_lwe_prepare_accumulator.  Owns the key object fhe_lwe_ksk_t (import, export, generation on the device) and the apply call.
// fhe_lwe_keyswitch is one launch, no workspace, nothing allocated: it can be captured into a hipGraph with the rest of the pipeline.
// Kernels: lwe_keyswitch.hip.h.
#include "engine.h"

#include "lwe_keyswitch.hip.h"

struct fhe_lwe_ksk {
    int device = 0;
    uint32_t n_in = 0, n_out = 0, ncp = 0, w = 0, K = 0;   // ncp: columns of an internal row, n_out + 1 rounded up to 64
    uint64_t q = 0;
    size_t R = 0;                                          // n_in K rows
    bool wide = false;                                     // the apply kernel's accumulator form, chosen at creation
    uint64_t *d_rows = nullptr;                            // [R][ncp], padding columns zero
};

static uint32_t bit_length(uint64_t v) { return v ? 64 - (uint32_t)__builtin_clzll(v) : 0; }
static uint32_t ksk_digits(uint64_t q, uint32_t w) { return (bit_length(q) + w - 1) / w; }

// the checks every entry point that names a digit width shares; `what` prefixes the message
static int check_shape(uint32_t decomp_bits, uint32_t n_out, const char *what) {
    if (decomp_bits < 1 || decomp_bits > 32) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": decomp_bits must be in [1, 32]");
    if (!n_out || n_out > 65536) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": n_out must be in [1, 65536]");
    return FHE_OK;
}
static bool key_matches(const fhe_rns_ntt *h, const fhe_lwe_ksk *k) { return h->n == k->n_in && h->moduli[0].w[0] == k->q && h->device == k->device; }

// an empty key for (h, w, n_out) with its table allocated; the accumulator form is decided here (FHE_HIP_LWE_KSK_WIDE=1 forces the wide form)
static int new_ksk(const fhe_rns_ntt *h, uint32_t w, uint32_t n_out, fhe_lwe_ksk **out) {
    fhe_lwe_ksk *k = new (std::nothrow) fhe_lwe_ksk();
    if (!k) return fail(FHE_ERR_INVALID_ARG, "out of host memory");
    k->device = h->device; k->n_in = h->n; k->n_out = n_out; k->w = w; k->q = h->moduli[0].w[0];
    k->K = ksk_digits(k->q, w); k->R = (size_t)k->n_in * k->K;
    k->ncp = (n_out + 1 + fhe_dev::LWE_KS_COLS - 1) / fhe_dev::LWE_KS_COLS * fhe_dev::LWE_KS_COLS;
    const char *force = std::getenv("FHE_HIP_LWE_KSK_WIDE");
    k->wide = bit_length(k->q) + w + bit_length(k->R - 1) > 64 || (force && force[0] == '1');
    hipError_t e = hipMalloc((void **)&k->d_rows, k->R * k->ncp * sizeof(uint64_t));
    if (e != hipSuccess) { delete k; return fail(FHE_ERR_HIP, std::string("lwe_ksk: hipMalloc of the key table: ") + hipGetErrorString(e)); }
    *out = k;
    return FHE_OK;
}

extern "C" int fhe_lwe_ksk_destroy(fhe_lwe_ksk_t *ksk) {
    if (ksk) {
        if (ksk->d_rows) (void)hipFree(ksk->d_rows);
        delete ksk;
    }
    return FHE_OK;
}

extern "C" int fhe_lwe_ksk_num_digits(const fhe_rns_ntt_t *h, uint32_t decomp_bits, uint32_t *digits) {
    if (!h || !digits) return fail(FHE_ERR_INVALID_ARG, "lwe_ksk_num_digits: null argument");
    if (int rc = check_word_call(h, 1, "lwe_ksk_num_digits")) return rc;
    if (decomp_bits < 1 || decomp_bits > 32) return fail(FHE_ERR_INVALID_ARG, "lwe_ksk_num_digits: decomp_bits must be in [1, 32]");
    *digits = ksk_digits(h->moduli[0].w[0], decomp_bits);
    return FHE_OK;
}

extern "C" int fhe_lwe_ksk_bytes(const fhe_lwe_ksk_t *ksk, uint64_t *bytes) {
    if (!ksk || !bytes) return fail(FHE_ERR_INVALID_ARG, "lwe_ksk_bytes: null argument");
    *bytes = (uint64_t)ksk->R * ksk->ncp * sizeof(uint64_t);
    return FHE_OK;
}

static int repack(hipStream_t stream, uint64_t *dst, const uint64_t *src, const fhe_lwe_ksk *k, int to_internal) {
    const size_t count = k->R * k->ncp;
    hipLaunchKernelGGL(fhe_dev::lwe_ksk_repack_kernel, dim3(ew_grid(count)), dim3(256), 0, stream, dst, src, k->n_out, k->ncp, count, to_internal);
    return post_launch(stream, "lwe_ksk_repack_kernel");
}

extern "C" int fhe_lwe_ksk_create(fhe_rns_ntt_t *h, fhe_lwe_ksk_t **out, uint32_t decomp_bits, uint32_t n_out, const uint64_t *d_rows) {
    int rc = check_word_call(h, 1, "lwe_ksk_create"); if (rc) return rc;
    if (!out || !d_rows) return fail(FHE_ERR_INVALID_ARG, "lwe_ksk_create: null argument");
    if ((uintptr_t)d_rows & 7) return fail(FHE_ERR_INVALID_ARG, "lwe_ksk_create: d_rows must be 8-byte aligned");
    if ((rc = check_shape(decomp_bits, n_out, "lwe_ksk_create"))) return rc;
    fhe_lwe_ksk *k = nullptr;
    if ((rc = new_ksk(h, decomp_bits, n_out, &k))) return rc;
    rc = repack(h->stream, k->d_rows, d_rows, k, 1);
    if (!rc && hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(FHE_ERR_HIP, "lwe_ksk_create: the copy of the table failed");   // the source is not read again
    if (rc) { fhe_lwe_ksk_destroy(k); return rc; }
    *out = k;
    return FHE_OK;
}

extern "C" int fhe_lwe_ksk_export(fhe_rns_ntt_t *h, const fhe_lwe_ksk_t *ksk, uint64_t *d_rows) {
    int rc = check_word_call(h, 1, "lwe_ksk_export"); if (rc) return rc;
    if (!ksk || !d_rows) return fail(FHE_ERR_INVALID_ARG, "lwe_ksk_export: null argument");
    if ((uintptr_t)d_rows & 7) return fail(FHE_ERR_INVALID_ARG, "lwe_ksk_export: d_rows must be 8-byte aligned");
    if (!key_matches(h, ksk)) return fail(FHE_ERR_INVALID_ARG, "lwe_ksk_export: the engine does not match the key (degree, limb-0 modulus, device)");
    return repack(h->stream, d_rows, ksk->d_rows, ksk, 0);
}

extern "C" int fhe_lwe_ksk_generate(fhe_rns_ntt_t *h, const fhe_secret_key_t *sk, uint32_t decomp_bits, uint32_t n_out, const int32_t *z,
                                    uint64_t noise_scale, double sigma, const uint64_t seeds[2], fhe_lwe_ksk_t **out) {
    int rc = check_word_call(h, 1, "lwe_ksk_generate"); if (rc) return rc;
    if (!sk || !z || !seeds || !out) return fail(FHE_ERR_INVALID_ARG, "lwe_ksk_generate: null argument");
    if (sk->owner != h) return fail(FHE_ERR_INVALID_ARG, "lwe_ksk_generate: the key was imported for a different engine");
    if ((rc = check_shape(decomp_bits, n_out, "lwe_ksk_generate"))) return rc;
    for (uint32_t i = 0; i < n_out; i++)
        if (z[i] > (1 << 15) || z[i] < -(1 << 15)) return fail(FHE_ERR_INVALID_ARG, "lwe_ksk_generate: |z| must not exceed 2^15");
    if (!noise_scale) return fail(FHE_ERR_INVALID_ARG, "lwe_ksk_generate: noise_scale must not be 0");
    uint32_t len = 0;
    if ((rc = fhe_gaussian_cdt(sigma, nullptr, 0, &len))) return rc;
    const uint64_t q = h->moduli[0].w[0];
    if (len >= q) return fail(FHE_ERR_INVALID_ARG, "lwe_ksk_generate: 12 sigma does not fit below the modulus");
    if ((rc = ensure_cdt(h, sigma, "lwe_ksk_generate"))) return rc;
    (void)hipGetLastError();

    fhe_lwe_ksk *k = nullptr;
    Scratch scratch;
    auto body = [&]() -> int {
        if (int r = new_ksk(h, decomp_bits, n_out, &k)) return r;
        void *d_z = nullptr;
        if (int r = scratch.get(&d_z, (size_t)n_out * sizeof(int32_t))) return r;
        HIP_TRY(hipMemcpy(d_z, z, (size_t)n_out * sizeof(int32_t), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(fhe_dev::lwe_ksk_keygen_kernel, dim3((unsigned)k->R), dim3(fhe_dev::LWE_KEYGEN_THREADS), 0, h->stream, k->d_rows,
                           (const uint64_t *)sk->d_s, (const int32_t *)d_z, (const uint64_t *)h->d_cdt, h->cdt_len, q, noise_scale, seeds[0], seeds[1], n_out,
                           k->ncp, k->K, decomp_bits, (uint32_t)k->R);
        if (int r = post_launch(h->stream, "lwe_ksk_keygen_kernel")) return r;
        HIP_TRY(hipStreamSynchronize(h->stream));     // z is freed when the call returns; the key is complete then
        return FHE_OK;
    };
    if ((rc = body())) {
        (void)hipStreamSynchronize(h->stream);
        fhe_lwe_ksk_destroy(k);
        return rc;
    }
    *out = k;
    return FHE_OK;
}

template <bool WIDE>
static void launch_keyswitch(hipStream_t stream, const fhe_lwe_ksk *k, uint64_t q_out, uint64_t *d_out, const uint64_t *d_in, uint32_t batch) {
    auto go = [&](auto tb) {
        constexpr uint32_t TB = decltype(tb)::value;
        const uint32_t tiles = (batch + TB - 1) / TB;
        hipLaunchKernelGGL((fhe_dev::lwe_keyswitch_kernel<TB, WIDE>), dim3(k->ncp / fhe_dev::LWE_KS_COLS, std::min<uint32_t>(tiles, 65535)),
                           dim3(fhe_dev::LWE_KS_THREADS), 0, stream, d_out, d_in, (const uint64_t *)k->d_rows, k->q, q_out, k->n_in, k->n_out, k->ncp, k->K,
                           k->w, batch);
    };
    // the batch tile: 16 ciphertexts per workgroup re-read the key 16 times less often than one; small batches take the smaller tiles
    if (batch == 1) go(std::integral_constant<uint32_t, 1>{});
    else if (batch <= 4) go(std::integral_constant<uint32_t, 4>{});
    else go(std::integral_constant<uint32_t, 16>{});
}

extern "C" int fhe_lwe_keyswitch(fhe_rns_ntt_t *h, const fhe_lwe_ksk_t *ksk, uint64_t q_out, uint64_t *d_out, const uint64_t *d_in, uint32_t batch) {
    int rc = check_word_call(h, batch, "lwe_keyswitch"); if (rc) return rc;
    if (!ksk || !d_out || !d_in) return fail(FHE_ERR_INVALID_ARG, "lwe_keyswitch: null argument");
    if (((uintptr_t)d_out | (uintptr_t)d_in) & 7) return fail(FHE_ERR_INVALID_ARG, "lwe_keyswitch: d_out and d_in must be 8-byte aligned");
    if (q_out == 1 || q_out > (1ull << 48)) return fail(FHE_ERR_INVALID_ARG, "lwe_keyswitch: q_out must be 0 or in [2, 2^48]");
    if (!key_matches(h, ksk)) return fail(FHE_ERR_INVALID_ARG, "lwe_keyswitch: the engine does not match the key (degree, limb-0 modulus, device)");
    const size_t in = (size_t)batch * ((size_t)ksk->n_in + 1) * 8, out = (size_t)batch * ((size_t)ksk->n_out + 1) * 8;
    if (overlaps(d_out, out, d_in, in)) return fail(FHE_ERR_INVALID_ARG, "lwe_keyswitch: the output overlaps the input");
    if (ksk->wide) launch_keyswitch<true>(h->stream, ksk, q_out, d_out, d_in, batch);
    else launch_keyswitch<false>(h->stream, ksk, q_out, d_out, d_in, batch);
    return post_launch(h->stream, "lwe_keyswitch_kernel");
}
