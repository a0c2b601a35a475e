// encrypt.hip -- public-key encryption (fhe_ct_encrypt*; the keys: keys.hip).
// Fused path (plan_fused_encrypt; kernel: encrypt.hip.h): the key is kept transformed and packed like one key row, a call is one launch that
// draws u, e0, e1 in registers.  Composed path (full-width class, sizes outside the LDS-resident range, N = 2^15, sigma > 85,
// FHE_HIP_NO_FUSED_ENCRYPT=1): u by fhe_rns_sample_ternary into WS_ENC, two fhe_rns_ntt_multiply_bcast against the key as given, then
// encrypt_add_kernel below, which draws e0, e1 and adds t e0 + m and t e1 to the two products.
#include "engine.h"

#include "ctr_rand.hip.h"

namespace fhe_dev {

// out0 += [t e0] + m, out1 += [t e1] on containers of any width class; one lane per (ciphertext, coefficient), the same small integers in
// every limb.  e0, e1 are the Gaussian draws (gaussian_draw) of element g of their seeds.
__global__ void __launch_bounds__(256)
encrypt_add_kernel(u256 *__restrict__ out0, u256 *__restrict__ out1, const u256 *__restrict__ m, const CrtLimb *__restrict__ limbs, uint32_t L, uint32_t log_n,
                   uint64_t seed_e0, uint64_t seed_e1, uint64_t t, const uint64_t *__restrict__ cdt, uint32_t cdt_len, size_t count /* batch * n */) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, n = (size_t)1 << log_n;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count; g += stride) {
        const GaussianDraw e[2] = {gaussian_draw(seed_e0, g, cdt, cdt_len), gaussian_draw(seed_e1, g, cdt, cdt_len)};
        const size_t b = g >> log_n, x = g & (n - 1);
        for (uint32_t l = 0; l < L; l++) {
            const u256 q = limbs[l].q;
            const size_t at = ((b * L + l) << log_n) + x;
            for (int c = 0; c < 2; c++) {
                u256 *out = c ? out1 : out0;
                u256 v = add_mod(load_u256(out + at), scaled_small_mod(e[c].mag, e[c].neg, t, q), q);
                if (!c && m) v = add_mod(v, load_u256(m + at), q);
                store_u256(out + at, v);
            }
        }
    }
}

}  // namespace fhe_dev

// Whether a call with the table now in h->d_cdt runs the one-launch kernel
static bool encrypt_fused(const fhe_rns_ntt *h, const fhe_public_key *pk) {
    return pk->d_packed && plan_fused_encrypt(h) && h->cdt_len <= fhe_dev::ENCRYPT_MAX_CDT;
}
// everything the composed path needs for `batch` ciphertexts: u as containers, the workspaces of the broadcast product, the CRT limb table
static int ensure_encrypt_composed(fhe_rns_ntt *h, uint32_t batch) {
    int rc = ensure_need(h, need_multiply(h, batch) | need_transform(h, (size_t)batch * h->L)); if (rc) return rc;
    if ((rc = ensure_crt(h))) return rc;
    return grow_ws(h, h->ws[WS_ENC], (size_t)batch * h->L * h->n * 32);
}
extern "C" int fhe_ct_encrypt_reserve(fhe_rns_ntt_t *h, double sigma, uint32_t batch) {
    int rc = check_call(h, batch, "ct_encrypt_reserve"); if (rc) return rc;
    if ((rc = ensure_cdt(h, sigma, "ct_encrypt_reserve"))) return rc;       // sigma as fhe_gaussian_cdt admits it and 12 sigma below every modulus
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
    if ((rc = ensure_cdt(h, sigma, "ct_encrypt"))) return rc;
    if (d_m && (rc = check_inputs(h, {d_m}, batch))) return rc;
    if (encrypt_fused(h, pk)) {
        fhe_dev::LdsArgs A = lds_args(h, fhe_dev::LDS_ENCRYPT, {}, batch * h->L);
        A.r0 = d_out0; A.r1 = d_out1; A.a0 = d_m; A.kb = pk->d_packed; A.ka = (const char *)pk->d_packed + packed_row_bytes(h);
        A.cdt = h->d_cdt; A.cdt_len = h->cdt_len; A.t = t; A.per_ct = plan_encrypt_per_ct(h, batch);
        for (int s = 0; s < 3; s++) A.seeds[s] = seeds[s];
        return lds_launch(h, A, "ntt_encrypt_kernel");
    }
    if ((rc = ensure_encrypt_composed(h, batch))) return rc;                   // (no-op after fhe_ct_encrypt_reserve)
    const size_t S = (size_t)h->L * h->n * 32;
    if ((rc = fhe_rns_sample_ternary(h, h->ws[WS_ENC].p, 0.5, seeds[0], batch))) return rc;
    if ((rc = fhe_rns_ntt_multiply_bcast(h, d_out0, h->ws[WS_ENC].p, pk->d_pk, batch))) return rc;
    if ((rc = fhe_rns_ntt_multiply_bcast(h, d_out1, h->ws[WS_ENC].p, (const char *)pk->d_pk + S, batch))) return rc;
    const size_t count = (size_t)batch * h->n;
    hipLaunchKernelGGL(fhe_dev::encrypt_add_kernel, dim3(ew_grid(count)), dim3(256), 0, h->stream, (fhe_dev::u256 *)d_out0, (fhe_dev::u256 *)d_out1,
                       (const fhe_dev::u256 *)d_m, (const fhe_dev::CrtLimb *)h->d_crt, h->L, h->log_n, seeds[1], seeds[2], t, (const uint64_t *)h->d_cdt, h->cdt_len, count);
    return post_launch(h->stream, "encrypt_add_kernel");
}
