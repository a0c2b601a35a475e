// bootstrap.hip -- what stands around the blind-rotation loop (fhe_blind_rotate, keyswitch.hip): an LWE ciphertext into the loop's inputs
// (fhe_lwe_prepare_accumulator), one coefficient of the result out as an LWE sample (fhe_rlwe_sample_extract), and `count` evenly spaced
// coefficients of a ciphertext out in the layout the key switch and the packer read (fhe_rlwe_sample_extract_strided).  One launch each, no
// workspace, nothing allocated: all can be captured into a hipGraph with the loop.  Kernels: bootstrap.hip.h.  (The RGSW rows the loop
// consumes: fhe_rgsw_keys_generate, keygen.hip.)
#include "engine.h"

#include "bootstrap.hip.h"

extern "C" int fhe_lwe_prepare_accumulator(fhe_rns_ntt_t *h, uint64_t q_lwe, uint32_t n_lwe, const uint64_t *d_lwe, const void *d_tv, void *d_acc0,
                                           void *d_acc1, uint32_t *d_shifts, uint32_t batch) {
    int rc = check_word_call(h, batch, "lwe_prepare_accumulator", true); if (rc) return rc;
    if (!d_lwe || !d_tv || !d_acc0 || !d_acc1 || !d_shifts) return fail(FHE_ERR_INVALID_ARG, "lwe_prepare_accumulator: null argument");
    if ((rc = check_aligned({d_tv, d_acc0, d_acc1}, "lwe_prepare_accumulator"))) return rc;
    if (((uintptr_t)d_lwe & 7) || ((uintptr_t)d_shifts & 3)) return fail(FHE_ERR_INVALID_ARG, "lwe_prepare_accumulator: d_lwe must be 8-byte, d_shifts 4-byte aligned");
    if (!n_lwe) return fail(FHE_ERR_INVALID_ARG, "lwe_prepare_accumulator: n_lwe must be at least 1");
    if (q_lwe < 2 || q_lwe > (1ull << 48)) return fail(FHE_ERR_INVALID_ARG, "lwe_prepare_accumulator: q_lwe must be in [2, 2^48]");
    const size_t S = (size_t)h->L * h->n * 32, acc = S * batch, sh = (size_t)n_lwe * batch * 4, lw = ((size_t)n_lwe + 1) * batch * 8;
    if (overlaps(d_acc0, acc, d_acc1, acc) || overlaps(d_acc0, acc, d_shifts, sh) || overlaps(d_acc1, acc, d_shifts, sh))
        return fail(FHE_ERR_INVALID_ARG, "lwe_prepare_accumulator: the outputs must not overlap");
    for (const void *o : {(const void *)d_acc0, (const void *)d_acc1})
        if (overlaps(o, acc, d_lwe, lw) || overlaps(o, acc, d_tv, S)) return fail(FHE_ERR_INVALID_ARG, "lwe_prepare_accumulator: an output overlaps an input");
    if (overlaps(d_shifts, sh, d_lwe, lw) || overlaps(d_shifts, sh, d_tv, S)) return fail(FHE_ERR_INVALID_ARG, "lwe_prepare_accumulator: an output overlaps an input");
    if ((rc = check_inputs(h, {d_tv}, 1))) return rc;
    using V = fhe_dev::v2u64;
    const size_t halves = (size_t)batch * h->L * h->n * 2;
    return with_limbs(h, [&](auto *limbs) {
        hipLaunchKernelGGL((fhe_dev::lwe_prepare_kernel<limb_of<decltype(limbs)>>), dim3(ew_grid(halves)), dim3(256), 0, h->stream, (V *)d_acc0, (V *)d_acc1, d_shifts, d_lwe, (const V *)d_tv, limbs,
                           q_lwe, n_lwe, batch, h->L, h->log_n, halves);
        return post_launch(h->stream, "lwe_prepare_kernel");
    });
}

extern "C" int fhe_rlwe_sample_extract(fhe_rns_ntt_t *h, uint64_t *d_out, const void *d_c0, const void *d_c1, uint32_t idx, uint32_t batch) {
    int rc = check_word_call(h, batch, "rlwe_sample_extract", true); if (rc) return rc;
    if (!d_out || !d_c0 || !d_c1) return fail(FHE_ERR_INVALID_ARG, "rlwe_sample_extract: null argument");
    if ((rc = check_aligned({d_c0, d_c1}, "rlwe_sample_extract"))) return rc;
    if ((uintptr_t)d_out & 7) return fail(FHE_ERR_INVALID_ARG, "rlwe_sample_extract: d_out must be 8-byte aligned");
    if (idx >= h->n) return fail(FHE_ERR_INVALID_ARG, "rlwe_sample_extract: idx must be below n");
    const size_t polys = (size_t)batch * h->L, in = polys * h->n * 32, out = polys * ((size_t)h->n + 1) * 8;
    if (overlaps(d_out, out, d_c0, in) || overlaps(d_out, out, d_c1, in)) return fail(FHE_ERR_INVALID_ARG, "rlwe_sample_extract: the output overlaps an input");
    if ((rc = check_inputs(h, {d_c0, d_c1}, batch))) return rc;
    using V = fhe_dev::v2u64;
    const unsigned bx = (unsigned)std::min<size_t>(((size_t)h->n + 1 + 255) / 256, 64), by = (unsigned)std::min<size_t>(polys, 65535);
    return with_limbs(h, [&](auto *limbs) {
        hipLaunchKernelGGL((fhe_dev::sample_extract_kernel<limb_of<decltype(limbs)>>), dim3(bx, by), dim3(256), 0, h->stream, d_out, (const V *)d_c0, (const V *)d_c1, limbs, idx, h->L, h->log_n, polys);
        return post_launch(h->stream, "sample_extract_kernel");
    });
}

extern "C" int fhe_rlwe_sample_extract_strided(fhe_rns_ntt_t *h, uint64_t *d_out, const void *d_c0, const void *d_c1, uint32_t count, uint32_t batch) {
    int rc = check_word_call(h, batch, "rlwe_sample_extract_strided", true); if (rc) return rc;
    if (!d_out || !d_c0 || !d_c1) return fail(FHE_ERR_INVALID_ARG, "rlwe_sample_extract_strided: null argument");
    if ((rc = check_aligned({d_c0, d_c1}, "rlwe_sample_extract_strided"))) return rc;
    if ((uintptr_t)d_out & 7) return fail(FHE_ERR_INVALID_ARG, "rlwe_sample_extract_strided: d_out must be 8-byte aligned");
    if ((rc = check_count(h, count, batch, "rlwe_sample_extract_strided"))) return rc;   // what fhe_lwe_pack accepts
    const size_t polys = (size_t)batch * h->L, in = polys * h->n * 32, out = polys * count * ((size_t)h->n + 1) * 8;
    if (overlaps(d_out, out, d_c0, in) || overlaps(d_out, out, d_c1, in)) return fail(FHE_ERR_INVALID_ARG, "rlwe_sample_extract_strided: the output overlaps an input");
    if ((rc = check_inputs(h, {d_c0, d_c1}, batch))) return rc;
    using V = fhe_dev::v2u64;
    uint32_t log_count = 0; while ((1u << log_count) < count) log_count++;
    // x: the positions of a row; y: the polynomials; z: runs of rows, as many as it takes to reach ~4096 workgroups (16 per CU) where x and y
    // alone give fewer, each run at least 8 rows long so that a loaded coefficient is stored 8 times or more
    const unsigned bx = (unsigned)std::min<size_t>(((size_t)h->n + 255) / 256, 64), by = (unsigned)std::min<size_t>(polys, 65535);
    const size_t want = (4096 + (size_t)bx * by - 1) / ((size_t)bx * by);
    const uint32_t runs = (uint32_t)std::max<size_t>(1, std::min<size_t>(want, std::max<uint32_t>(1, count / 8)));
    const uint32_t rows_per_block = (count + runs - 1) / runs, bz = (count + rows_per_block - 1) / rows_per_block;
    return with_limbs(h, [&](auto *limbs) {
        hipLaunchKernelGGL((fhe_dev::sample_extract_strided_kernel<limb_of<decltype(limbs)>>), dim3(bx, by, bz), dim3(256), 0, h->stream, d_out, (const V *)d_c0, (const V *)d_c1, limbs, log_count,
                           rows_per_block, h->L, h->log_n, polys);
        return post_launch(h->stream, "sample_extract_strided_kernel");
    });
}
