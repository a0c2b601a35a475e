// lwe_pack.hip -- the way back from bootstrapping: LWE samples under the ring key (what fhe_rlwe_sample_extract writes) into one RLWE ciphertext
// (fhe_lwe_to_rlwe, fhe_lwe_pack*; contract and algorithm: include/fhe_hip.h), and the same from coefficient 0 of RLWE pairs, the blind rotation's
// accumulators, without the samples in between (fhe_rlwe_pack).  The ring packing of Chen, Dai, Kim and Song: log2(count) merge
// levels and, with the trace, log2(n / count) more automorphisms, every one a batched fhe_ct_apply_galois.
// Fused path (kernels: lwe_pack.hip.h): per level one streaming launch and one key switch.  The first level reads the samples (or the pairs) themselves, a later
// one forms the "P + G" of the level before in registers; three regions of the packing workspace WS_PACK rotate as (P, G, free).
// Composed path (FHE_HIP_NO_FUSED_PACK=1, read per call): the literal composition of entry points through container scratch in WS_PACK -- the
// embedding, fhe_rns_monomial_mul_sub, fhe_rns_poly_add / sub, fhe_ct_apply_galois -- one batch element at a time where the pairs are strided;
// fhe_rlwe_pack runs fhe_rlwe_sample_extract(idx = 0) into sample scratch at the end of WS_PACK first.
#include "engine.h"

#include "lwe_pack.hip.h"

static bool pack_composed_env() { const char *e = std::getenv("FHE_HIP_NO_FUSED_PACK"); return e && e[0] == '1'; }

extern "C" int fhe_lwe_pack_galois_elements(uint32_t n, uint32_t *elts) {
    if (!elts) return fail(FHE_ERR_INVALID_ARG, "lwe_pack_galois_elements: null argument");
    if (n < 8 || n > (1u << 30) || (n & (n - 1))) return fail(FHE_ERR_INVALID_ARG, "lwe_pack_galois_elements: n must be a power of two in [8, 2^30]");
    for (uint32_t j = 1; (1u << j) <= n; j++) elts[j - 1] = (1u << j) + 1;
    return FHE_OK;
}

// what a packing call packs: LWE samples (fhe_lwe_pack), or coefficient 0 of RLWE pairs (fhe_rlwe_pack; lwe == nullptr)
struct PackSource { const uint64_t *lwe; const void *c0, *c1; };

// the embedding (PAIR = false) or the first merge level (PAIR = true) of `entries` output ciphertexts
template <bool PAIR>
static int launch_embed(fhe_rns_ntt *h, void *o0, void *o1, void *d0, void *d1, const PackSource &src, uint32_t half, uint32_t halvings, size_t entries) {
    using V = fhe_dev::v2u64;
    const size_t halves = entries * h->L * h->n * 2;
    auto launch = [&](auto source, const char *what, auto... in) {           // in: the arrays the source reads
        return with_limbs(h, [&](auto *limbs) {
            hipLaunchKernelGGL((fhe_dev::embed_merge_kernel<limb_of<decltype(limbs)>, decltype(source), PAIR, limb_of<decltype(in)>...>), dim3(ew_grid(halves)), dim3(256), 0,
                               h->stream, (V *)o0, (V *)o1, (V *)d0, (V *)d1, in..., limbs, half, halvings, h->L, h->log_n, halves);
            return post_launch(h->stream, what);
        });
    };
    if (src.lwe) return launch(fhe_dev::SampleRows{}, PAIR ? "embed_merge_kernel (samples, first level)" : "embed_merge_kernel (samples, embedding)", src.lwe);
    return launch(fhe_dev::RlwePairs{}, PAIR ? "embed_merge_kernel (pairs, first level)" : "embed_merge_kernel (pairs, embedding)", (const V *)src.c0, (const V *)src.c1);
}
static int launch_merge(fhe_rns_ntt *h, char *np0, char *np1, char *nd0, char *nd1, const char *p0, const char *p1, const char *g0, const char *g1, uint32_t half,
                        uint32_t m, size_t entries) {
    using V = fhe_dev::v2u64;
    const size_t halves = entries * h->L * h->n * 2;
    return with_limbs(h, [&](auto *limbs) {
        hipLaunchKernelGGL((fhe_dev::lwe_merge_kernel<limb_of<decltype(limbs)>>), dim3(ew_grid(halves)), dim3(256), 0, h->stream, (V *)np0, (V *)np1, (V *)nd0, (V *)nd1, (const V *)p0,
                           (const V *)p1, (const V *)g0, (const V *)g1, limbs, half, m, h->L, h->log_n, halves);
        return post_launch(h->stream, "lwe_merge_kernel");
    });
}
static int launch_sum(fhe_rns_ntt *h, void *o0, void *o1, const void *a0, const void *a1, const void *b0, const void *b1, size_t entries) {
    using V = fhe_dev::v2u64;
    const size_t halves = entries * h->L * h->n * 2;
    return with_limbs(h, [&](auto *limbs) {
        hipLaunchKernelGGL((fhe_dev::lwe_pack_sum_kernel<limb_of<decltype(limbs)>>), dim3(ew_grid(halves)), dim3(256), 0, h->stream, (V *)o0, (V *)o1, (const V *)a0, (const V *)a1,
                           (const V *)b0, (const V *)b1, limbs, h->L, h->log_n, halves);
        return post_launch(h->stream, "lwe_pack_sum_kernel");
    });
}

extern "C" int fhe_lwe_to_rlwe(fhe_rns_ntt_t *h, void *d_c0, void *d_c1, const uint64_t *d_lwe, uint32_t batch) {
    int rc = check_word_call(h, batch, "lwe_to_rlwe", true); if (rc) return rc;
    if (!d_c0 || !d_c1 || !d_lwe) return fail(FHE_ERR_INVALID_ARG, "lwe_to_rlwe: null argument");
    if ((rc = check_aligned({d_c0, d_c1}, "lwe_to_rlwe"))) return rc;
    if ((uintptr_t)d_lwe & 7) return fail(FHE_ERR_INVALID_ARG, "lwe_to_rlwe: d_lwe must be 8-byte aligned");
    const size_t polys = (size_t)batch * h->L, out = polys * h->n * 32, in = polys * ((size_t)h->n + 1) * 8;
    if (overlaps(d_c0, out, d_c1, out)) return fail(FHE_ERR_INVALID_ARG, "lwe_to_rlwe: the outputs must not overlap");
    if (overlaps(d_c0, out, d_lwe, in) || overlaps(d_c1, out, d_lwe, in)) return fail(FHE_ERR_INVALID_ARG, "lwe_to_rlwe: an output overlaps the input");
    return launch_embed<false>(h, d_c0, d_c1, nullptr, nullptr, PackSource{d_lwe, nullptr, nullptr}, 0, 0, batch);
}

// ---- the packing call ----------------------------------------------------------------------------------------------------------------
namespace {
struct PackShape {
    uint32_t k = 0;            // log2 count: merge levels
    uint32_t first_trace = 0, last_trace = 0;   // trace steps j = first .. last (none when first > last)
    uint32_t K = 0; bool packed = false;        // of the key sets the call uses (0: it uses none)
    uint32_t galois_batch = 0; // the largest batch of an fhe_ct_apply_galois of the call
};
}
// count, batch and the key sets of a call: everything fhe_lwe_pack and fhe_lwe_pack_reserve check alike
static int check_pack_shape(fhe_rns_ntt *h, const fhe_relin_keys_t *const *gks, uint32_t count, int trace, uint32_t batch, const char *what, PackShape *S) {
    const std::string w(what);
    if (int rc = check_count(h, count, batch, what)) return rc;
    while ((1u << S->k) < count) S->k++;
    S->first_trace = S->k + 1; S->last_trace = trace ? h->log_n : S->k;
    if (S->last_trace >= 1 && !gks) return fail(FHE_ERR_INVALID_ARG, w + ": null key-set array");
    for (uint32_t j = 1; j <= S->last_trace; j++) {
        const fhe_relin_keys_t *gk = gks[j - 1];
        if (!gk) return fail(FHE_ERR_INVALID_ARG, w + ": the key set of 2^" + std::to_string(j) + " + 1 is needed and null");
        if (gk->owner != h) return fail(FHE_ERR_INVALID_ARG, w + ": keys were imported for a different engine");
        if (S->K && gk->decomp_bits != gks[0]->decomp_bits) return fail(FHE_ERR_INVALID_ARG, w + ": the key sets differ in decomp_bits");
        S->K = gk->K; S->packed = gk->d_pkb != nullptr;
    }
    S->galois_batch = S->k ? batch * (count / 2) : (S->last_trace ? batch : 0);
    return FHE_OK;
}
// bytes of WS_PACK for a call.  Fused: three regions of batch count S (S = L n 32; a region holds both components of batch count / 2
// ciphertexts), or the trace's pair alone for count = 1.  Composed: R (batch count ciphertexts), X, P, D (half as many each) and the shift words,
// then, from a 16-byte boundary (composed_samples_at), the batch count samples that fhe_rlwe_pack extracts first: fhe_lwe_pack_reserve cannot know
// which of the two entries follows, so the composed size covers both.
static size_t composed_samples_at(const fhe_rns_ntt *h, const PackShape &S, uint32_t count, uint32_t batch) {
    const size_t poly = (size_t)h->L * h->n * 32, bc = (size_t)batch * count;
    const size_t own = S.k ? 5 * bc * poly + 2 * bc : (S.last_trace ? 2 * batch * poly : 0);
    return (own + 15) & ~(size_t)15;
}
static size_t pack_bytes(const fhe_rns_ntt *h, const PackShape &S, uint32_t count, uint32_t batch, bool composed) {
    const size_t poly = (size_t)h->L * h->n * 32, bc = (size_t)batch * count;
    if (composed) return composed_samples_at(h, S, count, batch) + bc * h->L * ((size_t)h->n + 1) * 8;
    if (!S.k) return S.last_trace ? 2 * batch * poly : 0;
    return 3 * bc * poly;
}
static int ensure_pack(fhe_rns_ntt *h, const PackShape &S, uint32_t count, uint32_t batch, bool composed) {
    int rc = grow_ws(h, h->ws[WS_PACK], pack_bytes(h, S, count, batch, composed)); if (rc) return rc;
    return S.galois_batch ? ensure_need(h, need_apply_galois(h, S.galois_batch, S.K, S.packed)) : FHE_OK;
}

extern "C" int fhe_lwe_pack_reserve(fhe_rns_ntt_t *h, const fhe_relin_keys_t *const *gks, uint32_t count, int trace, uint32_t batch) {
    int rc = check_word_call(h, batch, "lwe_pack_reserve", true); if (rc) return rc;
    PackShape S;
    if ((rc = check_pack_shape(h, gks, count, trace, batch, "lwe_pack_reserve", &S))) return rc;
    return ensure_pack(h, S, count, batch, pack_composed_env());
}

// ct <- ct + sigma_{2^j + 1}(ct) on the outputs, j = first_trace .. last_trace; (t0, t1): scratch for `batch` ciphertexts
static int pack_trace(fhe_rns_ntt *h, const fhe_relin_keys_t *const *gks, const PackShape &S, void *d_out0, void *d_out1, char *t0, char *t1, uint32_t batch, bool composed) {
    int rc;
    for (uint32_t j = S.first_trace; j <= S.last_trace; j++) {
        if ((rc = fhe_ct_apply_galois(h, gks[j - 1], (1u << j) + 1, t0, t1, d_out0, d_out1, batch))) return rc;
        if (!composed) { if ((rc = launch_sum(h, d_out0, d_out1, d_out0, d_out1, t0, t1, batch))) return rc; continue; }
        if ((rc = fhe_rns_poly_add(h, d_out0, d_out0, t0, batch)) || (rc = fhe_rns_poly_add(h, d_out1, d_out1, t1, batch))) return rc;
    }
    return FHE_OK;
}

static int pack_fused(fhe_rns_ntt *h, const fhe_relin_keys_t *const *gks, const PackShape &S, void *d_out0, void *d_out1, const PackSource &src, uint32_t count,
                      uint32_t halvings, uint32_t batch) {
    const size_t poly = (size_t)h->L * h->n * 32, region = (size_t)batch * count * poly;
    char *base = (char *)h->ws[WS_PACK].p;
    int rc;
    if (!S.k) {
        if ((rc = launch_embed<false>(h, d_out0, d_out1, nullptr, nullptr, src, 0, halvings, batch))) return rc;
        return pack_trace(h, gks, S, d_out0, d_out1, base, base + batch * poly, batch, false);
    }
    char *reg_p = base, *reg_g = base + 2 * region, *reg_free = base + region;
    size_t e = (size_t)batch * (count / 2);                                   // ciphertexts the level writes
    // level 1: P -> reg_p, D -> reg_free, G = key-switched sigma_3(D) -> reg_g
    if ((rc = launch_embed<true>(h, reg_p, reg_p + e * poly, reg_free, reg_free + e * poly, src, count / 2, halvings, e))) return rc;
    if ((rc = fhe_ct_apply_galois(h, gks[0], 3, reg_g, reg_g + e * poly, reg_free, reg_free + e * poly, (uint32_t)e))) return rc;
    const char *p0 = reg_p, *p1 = reg_p + e * poly, *g0 = reg_g, *g1 = reg_g + e * poly;
    for (uint32_t l = 2; l <= S.k; l++) {
        const uint32_t half = count >> l;
        e = (size_t)batch * half;
        char *np0 = reg_free, *np1 = np0 + e * poly, *nd0 = np1 + e * poly, *nd1 = nd0 + e * poly;   // 4 e <= batch count: inside the region
        if ((rc = launch_merge(h, np0, np1, nd0, nd1, p0, p1, g0, g1, half, h->n >> l, e))) return rc;
        char *ng0 = reg_p, *ng1 = reg_p + e * poly;                           // the P of the level before is consumed: its region takes the new G
        if ((rc = fhe_ct_apply_galois(h, gks[l - 1], (1u << l) + 1, ng0, ng1, nd0, nd1, (uint32_t)e))) return rc;
        char *old_g = reg_g;
        reg_g = reg_p; reg_p = reg_free; reg_free = old_g;
        p0 = np0; p1 = np1; g0 = ng0; g1 = ng1;
    }
    if ((rc = launch_sum(h, d_out0, d_out1, p0, p1, g0, g1, batch))) return rc;      // e == batch here
    return pack_trace(h, gks, S, d_out0, d_out1, reg_free, reg_free + batch * poly, batch, false);
}

static int pack_composed(fhe_rns_ntt *h, const fhe_relin_keys_t *const *gks, const PackShape &S, void *d_out0, void *d_out1, PackSource src, uint32_t count,
                         uint32_t halvings, uint32_t batch) {
    const size_t poly = (size_t)h->L * h->n * 32, bc = (size_t)batch * count, hb = bc / 2 * poly;
    char *base = (char *)h->ws[WS_PACK].p;
    int rc;
    if (!src.lwe) {                                                             // fhe_rlwe_pack: the literal extraction at idx = 0 of every pair first
        uint64_t *samples = (uint64_t *)(base + composed_samples_at(h, S, count, batch));
        if ((rc = fhe_rlwe_sample_extract(h, samples, src.c0, src.c1, 0, (uint32_t)bc))) return rc;
        src = PackSource{samples, nullptr, nullptr};
    }
    if (!S.k) {
        if ((rc = launch_embed<false>(h, d_out0, d_out1, nullptr, nullptr, src, 0, halvings, batch))) return rc;
        return pack_trace(h, gks, S, d_out0, d_out1, base, base + batch * poly, batch, true);
    }
    char *R[2] = {base, base + bc * poly}, *X[2] = {base + 2 * bc * poly, base + 2 * bc * poly + hb}, *P[2] = {X[1] + hb, X[1] + 2 * hb}, *D[2] = {P[1] + hb, P[1] + 2 * hb};
    uint32_t *shifts = (uint32_t *)(D[1] + hb);
    if ((rc = launch_embed<false>(h, R[0], R[1], nullptr, nullptr, src, 0, halvings, bc))) return rc;       // fhe_lwe_to_rlwe of F^-1 times the samples
    for (uint32_t l = 1, cur = count; l <= S.k; l++, cur /= 2) {
        const uint32_t half = cur / 2, e = batch * half;
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)shifts, (int)(h->n >> l), half, h->stream));
        for (uint32_t b = 0; b < batch; b++)
            for (int c = 0; c < 2; c++) {
                const char *E = R[c] + (size_t)b * cur * poly, *O = E + (size_t)half * poly;
                char *x = X[c] + (size_t)b * half * poly;
                if ((rc = fhe_rns_monomial_mul_sub(h, x, O, shifts, half))) return rc;                        // (X^m - 1) O
                if ((rc = fhe_rns_poly_add(h, x, x, O, half))) return rc;                                     // X^m O
                if ((rc = fhe_rns_poly_add(h, P[c] + (size_t)b * half * poly, E, x, half))) return rc;
                if ((rc = fhe_rns_poly_sub(h, D[c] + (size_t)b * half * poly, E, x, half))) return rc;
            }
        if ((rc = fhe_ct_apply_galois(h, gks[l - 1], (1u << l) + 1, X[0], X[1], D[0], D[1], e))) return rc;   // G over X^m O, which is consumed
        void *dst[2] = {l == S.k ? d_out0 : (void *)R[0], l == S.k ? d_out1 : (void *)R[1]};
        for (int c = 0; c < 2; c++) if ((rc = fhe_rns_poly_add(h, dst[c], P[c], X[c], e))) return rc;
    }
    return pack_trace(h, gks, S, d_out0, d_out1, X[0], X[1], batch, true);
}

extern "C" int fhe_lwe_pack(fhe_rns_ntt_t *h, const fhe_relin_keys_t *const *gks, void *d_out0, void *d_out1, const uint64_t *d_lwe, uint32_t count, int trace,
                            int normalize, uint32_t batch) {
    int rc = check_word_call(h, batch, "lwe_pack", true); if (rc) return rc;
    if (!d_out0 || !d_out1 || !d_lwe) return fail(FHE_ERR_INVALID_ARG, "lwe_pack: null argument");
    if ((rc = check_aligned({d_out0, d_out1}, "lwe_pack"))) return rc;
    if ((uintptr_t)d_lwe & 7) return fail(FHE_ERR_INVALID_ARG, "lwe_pack: d_lwe must be 8-byte aligned");
    PackShape S;
    if ((rc = check_pack_shape(h, gks, count, trace, batch, "lwe_pack", &S))) return rc;
    const size_t out = (size_t)batch * h->L * h->n * 32, in = (size_t)batch * count * h->L * ((size_t)h->n + 1) * 8;
    if (overlaps(d_out0, out, d_out1, out)) return fail(FHE_ERR_INVALID_ARG, "lwe_pack: the outputs must not overlap");
    if (overlaps(d_out0, out, d_lwe, in) || overlaps(d_out1, out, d_lwe, in)) return fail(FHE_ERR_INVALID_ARG, "lwe_pack: an output overlaps the input");
    const bool composed = pack_composed_env();
    if ((rc = ensure_pack(h, S, count, batch, composed))) return rc;              // (no-op after fhe_lwe_pack_reserve)
    const uint32_t halvings = normalize ? (trace ? h->log_n : S.k) : 0;           // F = n with the trace, count without
    const PackSource src{d_lwe, nullptr, nullptr};
    return composed ? pack_composed(h, gks, S, d_out0, d_out1, src, count, halvings, batch) : pack_fused(h, gks, S, d_out0, d_out1, src, count, halvings, batch);
}

extern "C" int fhe_rlwe_pack(fhe_rns_ntt_t *h, const fhe_relin_keys_t *const *gks, void *d_out0, void *d_out1, const void *d_c0, const void *d_c1, uint32_t count,
                             int trace, int normalize, uint32_t batch) {
    int rc = check_word_call(h, batch, "rlwe_pack", true); if (rc) return rc;
    if (!d_out0 || !d_out1 || !d_c0 || !d_c1) return fail(FHE_ERR_INVALID_ARG, "rlwe_pack: null argument");
    if ((rc = check_aligned({d_out0, d_out1, d_c0, d_c1}, "rlwe_pack"))) return rc;
    PackShape S;
    if ((rc = check_pack_shape(h, gks, count, trace, batch, "rlwe_pack", &S))) return rc;
    const size_t out = (size_t)batch * h->L * h->n * 32, in = out * count;
    if (overlaps(d_out0, out, d_out1, out)) return fail(FHE_ERR_INVALID_ARG, "rlwe_pack: the outputs must not overlap");
    for (const void *o : {(const void *)d_out0, (const void *)d_out1})
        if (overlaps(o, out, d_c0, in) || overlaps(o, out, d_c1, in)) return fail(FHE_ERR_INVALID_ARG, "rlwe_pack: an output overlaps an input");
    const bool composed = pack_composed_env();
    if ((rc = ensure_pack(h, S, count, batch, composed))) return rc;              // (no-op after fhe_lwe_pack_reserve: the scratch is fhe_lwe_pack's)
    if ((rc = check_inputs(h, {d_c1}, batch * count))) return rc;
    const uint32_t halvings = normalize ? (trace ? h->log_n : S.k) : 0;
    const PackSource src{nullptr, d_c0, d_c1};
    return composed ? pack_composed(h, gks, S, d_out0, d_out1, src, count, halvings, batch) : pack_fused(h, gks, S, d_out0, d_out1, src, count, halvings, batch);
}
