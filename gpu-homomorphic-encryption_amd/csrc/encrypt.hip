// encrypt.hip -- public keys and public-key encryption (fhe_public_key_*, fhe_ct_encrypt*).
// Fused path (plan_fused_encrypt; kernel: encrypt.hip.h): the key is kept transformed and packed like one key row, a call is one launch that
// draws u, e0, e1 in registers.  Composed path (full-width class, sizes outside the LDS-resident range, N = 2^15, sigma > 85,
// FHE_HIP_NO_FUSED_ENCRYPT=1): u by fhe_rns_sample_ternary into d_enc, two fhe_rns_ntt_multiply_bcast against the key as given, then
// encrypt_add_kernel below, which draws e0, e1 and adds t e0 + m and t e1 to the two products.
#include "engine.h"

#include <cmath>

#include "ctr_rand.hip.h"
#include "ntt_word.hip.h"

namespace fhe_dev {

__device__ __forceinline__ u256 small256(uint64_t v) { u256 r; r.l[0] = v; r.l[1] = r.l[2] = r.l[3] = 0; return r; }

// out0 += [t e0] + m, out1 += [t e1] on containers of any width class; one lane per (ciphertext, coefficient), the same small integers in
// every limb.  e0, e1 are the draws of sample_small_kernel<1> for element g of their seeds; t |e| mod q_l by double-and-add (|e| < 2^24, no division).
__global__ void __launch_bounds__(256)
encrypt_add_kernel(u256 *__restrict__ out0, u256 *__restrict__ out1, const u256 *__restrict__ m, const CrtLimb *__restrict__ limbs, uint32_t L, uint32_t log_n,
                   uint64_t seed_e0, uint64_t seed_e1, uint64_t t, const uint64_t *__restrict__ cdt, uint32_t cdt_len, size_t count /* batch * n */) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, n = (size_t)1 << log_n;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count; g += stride) {
        uint32_t mag[2]; bool neg[2];
        for (int c = 0; c < 2; c++) {
            const uint64_t base = ctr_base(c ? seed_e1 : seed_e0, g), r = sm64(base + DRAW_CDT);
            uint32_t k = 0;
            for (uint32_t j = 0; j < cdt_len; j++) k += r >= cdt[j] ? 1u : 0u;
            mag[c] = k; neg[c] = (sm64(base + DRAW_SIGN) >> 63) != 0;
        }
        const size_t b = g >> log_n, x = g & (n - 1);
        for (uint32_t l = 0; l < L; l++) {
            const u256 q = limbs[l].q;
            const u256 tq = small256((q.l[1] | q.l[2] | q.l[3]) ? t : t % q.l[0]);     // t mod q_l
            const size_t at = ((b * L + l) << log_n) + x;
            for (int c = 0; c < 2; c++) {
                u256 te = small256(0), pw = tq;
                for (uint32_t k = mag[c]; k; k >>= 1) { if (k & 1) te = add_mod(te, pw, q); pw = add_mod(pw, pw, q); }
                u256 *out = c ? out1 : out0;
                u256 v = load_u256(out + at);
                v = neg[c] ? sub_mod(v, te, q) : add_mod(v, te, q);
                if (!c && m) v = add_mod(v, load_u256(m + at), q);
                store_u256(out + at, v);
            }
        }
    }
}

}  // namespace fhe_dev

struct fhe_public_key {
    fhe_rns_ntt *owner = nullptr;
    const void *src0 = nullptr, *src1 = nullptr;    // what the key was imported from (outputs must not alias them)
    void *d_pk = nullptr;                           // (pk0, pk1) as given: 2 x [L][n] containers, coefficient form (the composed path multiplies by these)
    void *d_packed = nullptr;                       // fused path: (pk0^, pk1^), 2 x [L][n] residues, transformed and packed like one key row each
};
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
    void *d_tr = nullptr;                            // the transformed copy, containers
    auto body = [&]() -> int {
        HIP_TRY(hipMalloc(&pk->d_pk, 2 * S));
        HIP_TRY(hipMemcpyAsync(pk->d_pk, d_pk0, S, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync((char *)pk->d_pk + S, d_pk1, S, hipMemcpyDeviceToDevice, h->stream));
        if (!plan_fused_encrypt(h)) return post_launch(h->stream, "public_key_create copy");
        HIP_TRY(hipMalloc(&d_tr, 2 * S));
        HIP_TRY(hipMemcpyAsync(d_tr, pk->d_pk, 2 * S, hipMemcpyDeviceToDevice, h->stream));
        if (int r = do_forward(h, d_tr, 2)) return r;
        HIP_TRY(hipMalloc(&pk->d_packed, 2 * (size_t)h->L * h->n * residue_bytes(h)));
        if (int r = with_word_field(h, [&](auto f) {
                using F = decltype(f);
                hipLaunchKernelGGL((fhe_dev::pack_keys_kernel<F>), dim3(ew_grid(2 * (size_t)h->L * h->n)), dim3(256), 0, h->stream, (typename F::E *)pk->d_packed,
                                   (const typename F::V16 *)d_tr, (const fhe_dev::Limb<F> *)h->d_limbs, h->L, h->log_n, 2u);
                return post_launch(h->stream, "pack_keys_kernel (public key)");
            })) return r;
        HIP_TRY(hipStreamSynchronize(h->stream));     // the transformed copy is freed below
        return FHE_OK;
    };
    rc = body();
    if (d_tr) (void)hipFree(d_tr);
    if (rc) { fhe_public_key_destroy(pk); return rc; }
    *out = pk;
    return FHE_OK;
}

// Whether a call with the table now in h->d_cdt runs the one-launch kernel
static bool encrypt_fused(const fhe_rns_ntt *h, const fhe_public_key *pk) {
    return pk->d_packed && plan_fused_encrypt(h) && h->cdt_len <= fhe_dev::ENCRYPT_MAX_CDT;
}
// sigma as fhe_gaussian_cdt admits it and 12 sigma below every modulus; uploads the table when sigma changed
static int encrypt_table(fhe_rns_ntt *h, double sigma, const char *what) {
    uint32_t len = 0;
    if (int rc = fhe_gaussian_cdt(sigma, nullptr, 0, &len)) return rc;
    return ensure_cdt(h, sigma, what);
}
// everything the composed path needs for `batch` ciphertexts: u as containers, the workspaces of the broadcast product, the CRT limb table
static int ensure_encrypt_composed(fhe_rns_ntt *h, uint32_t batch) {
    int rc = ensure_need(h, need_multiply(h, batch) | need_transform(h, (size_t)batch * h->L)); if (rc) return rc;
    if ((rc = ensure_crt(h))) return rc;
    return grow_ws(h, &h->d_enc, &h->enc_bytes, (size_t)batch * h->L * h->n * 32);
}
extern "C" int fhe_ct_encrypt_reserve(fhe_rns_ntt_t *h, double sigma, uint32_t batch) {
    int rc = check_call(h, batch, "ct_encrypt_reserve"); if (rc) return rc;
    if ((rc = encrypt_table(h, sigma, "ct_encrypt_reserve"))) return rc;
    // a key may be imported later, and a table too long for the kernel takes the composed path: size that path wherever a call can reach it
    if (plan_fused_encrypt(h) && h->cdt_len <= fhe_dev::ENCRYPT_MAX_CDT) return FHE_OK;
    return ensure_encrypt_composed(h, batch);
}
extern "C" int fhe_ct_encrypt(fhe_rns_ntt_t *h, const fhe_public_key_t *pk, uint64_t t, double sigma, const uint64_t seeds[3], void *d_out0, void *d_out1,
                              const void *d_m, uint32_t batch) {
    int rc = check_call(h, batch, "ct_encrypt"); if (rc) return rc;
    if (!pk || !seeds || !d_out0 || !d_out1) return fail(FHE_ERR_INVALID_ARG, "ct_encrypt: null argument");
    if (pk->owner != h) return fail(FHE_ERR_INVALID_ARG, "ct_encrypt: the key was imported for a different engine");
    if ((rc = check_aligned({d_out0, d_out1, d_m}, "ct_encrypt"))) return rc;
    if (d_out0 == d_out1) return fail(FHE_ERR_INVALID_ARG, "ct_encrypt: outputs must be distinct");
    for (const void *i : {d_m, pk->src0, pk->src1, (const void *)pk->d_pk})
        if (i && (d_out0 == i || d_out1 == i)) return fail(FHE_ERR_INVALID_ARG, "ct_encrypt: outputs must not alias the message or the key");
    if (t < 2) return fail(FHE_ERR_INVALID_ARG, "ct_encrypt: the plaintext modulus t must be at least 2");
    if ((rc = encrypt_table(h, sigma, "ct_encrypt"))) return rc;
    if (d_m && (rc = check_inputs(h, {d_m}, batch))) return rc;
    if (encrypt_fused(h, pk)) {
        const size_t half = (size_t)h->L * h->n * residue_bytes(h);
        fhe_dev::LdsArgs A = lds_args(h, fhe_dev::LDS_ENCRYPT, {}, batch * h->L);
        A.r0 = d_out0; A.r1 = d_out1; A.a0 = d_m; A.kb = pk->d_packed; A.ka = (const char *)pk->d_packed + half;
        A.cdt = h->d_cdt; A.cdt_len = h->cdt_len; A.t = t; A.per_ct = plan_encrypt_per_ct(h, batch);
        for (int s = 0; s < 3; s++) A.seeds[s] = seeds[s];
        return lds_launch(h, A, "ntt_encrypt_kernel");
    }
    if ((rc = ensure_encrypt_composed(h, batch))) return rc;                   // (no-op after fhe_ct_encrypt_reserve)
    const size_t S = (size_t)h->L * h->n * 32;
    if ((rc = fhe_rns_sample_ternary(h, h->d_enc, 0.5, seeds[0], batch))) return rc;
    if ((rc = fhe_rns_ntt_multiply_bcast(h, d_out0, h->d_enc, pk->d_pk, batch))) return rc;
    if ((rc = fhe_rns_ntt_multiply_bcast(h, d_out1, h->d_enc, (const char *)pk->d_pk + S, batch))) return rc;
    const size_t count = (size_t)batch * h->n;
    hipLaunchKernelGGL(fhe_dev::encrypt_add_kernel, dim3(ew_grid(count)), dim3(256), 0, h->stream, (fhe_dev::u256 *)d_out0, (fhe_dev::u256 *)d_out1,
                       (const fhe_dev::u256 *)d_m, (const fhe_dev::CrtLimb *)h->d_crt, h->L, h->log_n, seeds[1], seeds[2], t, (const uint64_t *)h->d_cdt, h->cdt_len, count);
    return post_launch(h->stream, "encrypt_add_kernel");
}
