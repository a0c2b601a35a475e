// keyswitch.hip -- relinearisation, multiply + relinearise, Galois automorphisms, hoisted rotations and linear transform, blind rotation.
#include "engine.h"

#include <algorithm>
#include <utility>

#include "galois.hip.h"
#include "ntt256_keyswitch.hip.h"
#include "ntt_word.hip.h"

// ------------------------------------------------------------------------------------------------------
// relinearisation / key switching (general path: digit embedding -> batched forward NTT -> MAC -> inverse)
// ------------------------------------------------------------------------------------------------------
uint32_t relin_digits(const fhe_rns_ntt *h, uint32_t w) {
    int mx = 0;
    for (const U256 &q : h->moduli) mx = q.bit_length() > mx ? q.bit_length() : mx;
    return ((uint32_t)mx + w - 1) / w;
}
extern "C" int fhe_relin_num_digits(const fhe_rns_ntt_t *h, uint32_t decomp_bits, uint32_t *digits) {
    if (!h || !digits) return fail(FHE_ERR_INVALID_ARG, "null argument");
    if (decomp_bits < 1 || decomp_bits > 64) return fail(FHE_ERR_INVALID_ARG, "decomp_bits must be in [1, 64]");
    *digits = relin_digits(h, decomp_bits);
    return FHE_OK;
}
// Whether a key set of K digits of decomp_bits bits gets packed tables, i.e. runs the fused kernels (fhe_ct_hoist asks before any key set is seen)
bool keys_get_packed(const fhe_rns_ntt *h, uint32_t decomp_bits, uint32_t K) {
    const size_t num_keys = (size_t)h->L * K;
    // The fused kernels feed a digit of limb j (< min(2^w, q_j)) straight into limb i's lazy forward transform, whose
    // integer butterflies accept inputs below 4*q_i; bases mixing very different prime sizes go through the general
    // composition, which reduces every digit modulo q_i first.
    bool digits_fit = true;
    if (h->width == FHE_WIDTH_32 || h->width == FHE_WIDTH_64 || h->width == FHE_WIDTH_64X) {
        fhe_host::u128 q_min = ~(fhe_host::u128)0, q_max = 0;
        for (const U256 &q : h->moduli) { fhe_host::u128 v = q.w[0]; q_min = v < q_min ? v : q_min; q_max = v > q_max ? v : q_max; }
        const fhe_host::u128 digit_bound = decomp_bits < 64 ? std::min((fhe_host::u128)1 << decomp_bits, q_max) : q_max;
        // the full-range field's butterflies are canonical: there a digit must be a residue of q_i as it stands
        digits_fit = digit_bound <= (h->width == FHE_WIDTH_64X ? q_min : 4 * q_min);
    } else if (h->width == FHE_WIDTH_52) {
        // floating-point field: the fused kernels add the L*K digit-times-key products of a limb as doubles and reduce the sum once
        // (F52::regroup, stated for |x| < 2^49).  A product is below 0.76 q in magnitude, and the external product adds the second
        // component's L*K products to the reduced sum of the first: (L*K + 1) * 0.76 * 2^43 < 2^49 holds up to L*K = 83 (DESIGN.md
        // section 4.3).  More digits than that take the general composition, which reduces after every product.
        digits_fit = (uint64_t)h->L * K <= 83;
    }
    // the fused kernels address a packed table through a buffer descriptor with 32-bit offsets (fhe_dev::TableBuf): a table of 4 GiB or
    // more (L*K*L*n residues: not reached by any parameter set of the reference) stays on the general composition
    const bool table_fits = (size_t)num_keys * h->L * h->n * (h->width == FHE_WIDTH_32 ? 4 : 8) < ((size_t)1 << 32);
    return h->width != FHE_WIDTH_256 && !h->sub_top && digits_fit && table_fits && !h->env.no_fused_keyswitch;
}

// D[jk][b][i] = digit jk of src[b] embedded in limb i, as containers (K digits of w bits per limb)
static int embed_digits(fhe_rns_ntt *h, char *D, const void *src, uint32_t K, uint32_t w, uint32_t chunk) {
    const size_t total = (size_t)h->L * K * chunk * h->L * h->n;
    if (h->width != FHE_WIDTH_256) return with_word_field(h, [&](auto f) {
        using F = decltype(f); using V = typename F::V16;
        hipLaunchKernelGGL((fhe_dev::digit_embed_kernel<F>), dim3(ew_grid(total * 2)), dim3(256), 0, h->stream, (V *)D, (const V *)src,
                           (const fhe_dev::Limb<F> *)h->d_limbs, h->L, h->log_n, K, w, chunk);
        return post_launch(h->stream, "digit_embed_kernel");
    });
    hipLaunchKernelGGL(fhe_dev::digit_embed256_kernel, dim3(ew_grid(total)), dim3(256), 0, h->stream, (fhe_dev::u256 *)D, (const fhe_dev::u256 *)src,
                       (const fhe_dev::Limb256 *)h->d_limbs, h->L, h->log_n, K, w, chunk);
    return post_launch(h->stream, "digit_embed256_kernel");
}
template <class F>
static int relin_embed_mac_lds(fhe_rns_ntt *h, const fhe_relin_keys *rk, char *D, char *acc0, char *acc1, const void *c2, uint32_t chunk, int phase) {
    using V = typename F::V16;
    const uint32_t LK = h->L * rk->K;
    size_t halves = (size_t)chunk * h->L * h->n * 2;
    hipLaunchKernelGGL((fhe_dev::relin_mac_kernel<F>), dim3(ew_grid(halves)), dim3(256), 0, h->stream, (V *)acc0, (V *)acc1, (const V *)D,
                       (const V *)rk->d_kb, (const V *)rk->d_ka, (const fhe_dev::Limb<F> *)h->d_limbs, h->L, h->log_n, LK, chunk);
    return post_launch(h->stream, "relin_mac_kernel");
}
static int relin_embed_mac(fhe_rns_ntt *h, const fhe_relin_keys *rk, char *D, char *acc0, char *acc1, const void *c2, uint32_t chunk, int phase) {
    if (phase == 0) return embed_digits(h, D, c2, rk->K, rk->decomp_bits, chunk);
    if (h->width != FHE_WIDTH_256) return with_word_field(h, [&](auto f) { return relin_embed_mac_lds<decltype(f)>(h, rk, D, acc0, acc1, c2, chunk, phase); });
    const uint32_t LK = h->L * rk->K;
    size_t count = (size_t)chunk * h->L * h->n;
    hipLaunchKernelGGL(fhe_dev::relin_mac256_kernel, dim3(ew_grid(count)), dim3(256), 0, h->stream, (fhe_dev::u256 *)acc0, (fhe_dev::u256 *)acc1,
                       (const fhe_dev::u256 *)D, (const fhe_dev::u256 *)rk->d_kb, (const fhe_dev::u256 *)rk->d_ka,
                       (const fhe_dev::Limb256 *)h->d_limbs, h->L, h->log_n, LK, chunk);
    return post_launch(h->stream, "relin_mac256_kernel");
}

// The key-switch call of a plan: digit source c2 (compact where the plan says so), results r0 / r1, compact addends add0 / add1 (nullptr: in place)
static fhe_dev::LdsArgs keyswitch_args(fhe_rns_ntt *h, const fhe_relin_keys *rk, const LdsPlan &P, void *r0, void *r1, const void *c2, const void *add0,
                                       const void *add1, uint32_t polys, hipStream_t s) {
    fhe_dev::LdsArgs B = lds_args(h, fhe_dev::LDS_KEYSWITCH, P, polys);
    B.r0 = r0; B.r1 = r1; B.c2 = c2; B.add0 = add0; B.add1 = add1; B.stream = s; B.in_compact = P.compact; B.add_compact = P.add_compact;
    B.kb = rk->d_pkb; B.ka = rk->d_pka; B.K = rk->K; B.w = rk->decomp_bits;
    return B;
}
// The two chunked pipelines (stand-alone relinearisation, one-call multiply + relinearise) cut the batch into chunks of whole ciphertexts: as many
// as wanted, fewer while a chunk would not fill the chip (1024 limb polynomials: 256 CUs x 4 workgroups) or hold one ciphertext
struct Pipeline {
    uint32_t chunks = 1;
    struct { LdsPlan first, ks; } c[16]; // per chunk: tensor product (the relinearisation's first stage, the compaction, has no plan), key switch
    WsNeed need;                         // of the whole call
    void add(const LdsPlan &p) { const size_t ws2 = need.ws2 + p.ws2; need |= p.need(); need.ws2 = ws2; }   // every chunk has its own slice of WS2
};
static uint32_t pipeline_chunks(const fhe_rns_ntt *h, uint32_t batch, uint32_t want) { while (want > 1 && ((size_t)batch * h->L / want < 1024 || batch < want)) want--; return want; }
static uint32_t chunk_begin(uint32_t batch, uint32_t chunks, uint32_t c) { return c * (batch / chunks) + std::min(c, batch % chunks); }   // first ciphertext of chunk c
// Chunks of whole ciphertexts on two streams: the compaction of chunk i+1 (HBM-bound) runs beside the key switch of chunk i.
// (measured, N = 8192 x 4 x 30-bit, batch 1024: compaction alone 773 K -> 805 K relin/s at w = 16, 948 K -> 1007 K at w = 30; with the key switch of
//  chunk i beside the compaction of chunk i+1 on a second stream 807 K / 953 K at two chunks, 772 K / 948 K at four: one stream unless asked)
static Pipeline relin_pipeline(const fhe_rns_ntt *h, uint32_t batch, uint32_t K, KsSource src) {
    Pipeline pl;
    const LdsPlan P = plan_keyswitch(h, (size_t)batch * h->L, K, src, true);
    if (P.compact && h->width == FHE_WIDTH_32 && h->env.relin_chunks_forced) pl.chunks = pipeline_chunks(h, batch, h->env.overlap_chunks);
    for (uint32_t c = 0; c < pl.chunks; c++)
        pl.add(pl.c[c].ks = pl.chunks == 1 ? P : plan_keyswitch(h, (size_t)(chunk_begin(batch, pl.chunks, c + 1) - chunk_begin(batch, pl.chunks, c)) * h->L, K, KS_C2, false));
    return pl;
}
// The composed key switch (no packed tables): digit polynomials D[L K][chunk] + two accumulators in WS1, bounded to ~1 GiB: ciphertexts per chunk
static uint32_t composed_chunk(const fhe_rns_ntt *h, uint32_t batch, uint32_t K) {
    return (uint32_t)std::min<size_t>(std::max<size_t>(((size_t)1 << 30) / (((size_t)h->L * K + 2) * h->L * h->n * 32), 1), batch);
}
WsNeed need_relinearize(const fhe_rns_ntt *h, uint32_t batch, uint32_t K, bool packed, KsSource src) {
    const size_t LK = (size_t)h->L * K, chunk = composed_chunk(h, batch, K);
    if (packed) return relin_pipeline(h, batch, K, src).need;
    return {(LK + 2) * chunk * h->L * h->n * 32, 0, 0};   // (the transforms of the digit polynomials and accumulators ensure their own WS3, as before)
}
// Two-stream chunk pipeline: what the engine's stream has queued for chunk c is done -> the second stream may start on it; at the end the
// engine's stream joins the second one, so the call stays ordered on the engine's stream (and can be captured: fork / join through events).
static int fork_chunk(fhe_rns_ntt *h, uint32_t c) {
    HIP_TRY(hipEventRecord(h->ev_chunk[c], h->stream));
    HIP_TRY(hipStreamWaitEvent(h->aux_stream, h->ev_chunk[c], 0));
    return FHE_OK;
}
static int join_chunks(fhe_rns_ntt *h) {
    HIP_TRY(hipEventRecord(h->ev_join, h->aux_stream));
    HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_join, 0));
    return FHE_OK;
}

extern "C" int fhe_ct_relinearize(fhe_rns_ntt_t *h, const fhe_relin_keys_t *rk, void *d_c0, void *d_c1, const void *d_c2, uint32_t batch) {
    int rc = check_call(h, batch, "ct_relinearize"); if (rc) return rc;
    if (!rk || !d_c0 || !d_c1 || !d_c2) return fail(FHE_ERR_INVALID_ARG, "ct_relinearize: null argument");
    if ((rc = check_aligned({d_c0, d_c1, d_c2}, "ct_relinearize"))) return rc;
    if (rk->owner != h) return fail(FHE_ERR_INVALID_ARG, "ct_relinearize: keys were imported for a different engine");
    if (d_c0 == d_c1 || d_c0 == d_c2 || d_c1 == d_c2) return fail(FHE_ERR_INVALID_ARG, "ct_relinearize: components must be distinct buffers");
    if ((rc = check_inputs(h, {d_c0, d_c1, d_c2}, batch))) return rc;
    if (rk->d_pkb) {   // word-sized paths: fused launches
        // (c2 already in the workspace: the composed multiply + relinearise under a testing switch -- it stays where it is)
        const bool c2_in_ws2 = h->ws[WS2].p && (const char *)d_c2 >= (const char *)h->ws[WS2].p && (const char *)d_c2 < (const char *)h->ws[WS2].p + h->ws[WS2].bytes;
        const Pipeline pl = relin_pipeline(h, batch, rk->K, c2_in_ws2 ? KS_C2_AS_IS : KS_C2);
        const size_t S = (size_t)h->L * h->n * 32, Sc = (size_t)h->L * h->n * residue_bytes(h);
        if ((rc = ensure_need(h, pl.need)) || (pl.chunks > 1 && (rc = ensure_aux_stream(h)))) return rc;
        for (uint32_t c = 0; c < pl.chunks; c++) {
            const uint32_t b0 = chunk_begin(batch, pl.chunks, c), nb = chunk_begin(batch, pl.chunks, c + 1) - b0;
            const LdsPlan &Q = pl.c[c].ks;
            const void *c2 = (const char *)d_c2 + (size_t)b0 * S;
            if (Q.compact) {
                char *c2c = (char *)h->ws[WS2].p + (size_t)b0 * Sc;
                if ((rc = compact_poly(h, c2c, c2, (size_t)nb * h->L * h->n))) return rc;
                c2 = c2c;
            }
            if (pl.chunks > 1 && (rc = fork_chunk(h, c))) return rc;
            if ((rc = lds_launch(h, keyswitch_args(h, rk, Q, (char *)d_c0 + (size_t)b0 * S, (char *)d_c1 + (size_t)b0 * S, c2, nullptr, nullptr, nb * h->L,
                                                   pl.chunks > 1 ? h->aux_stream : h->stream), "ntt_keyswitch_kernel"))) return rc;
        }
        return pl.chunks > 1 ? join_chunks(h) : FHE_OK;
    }
    const uint32_t LK = h->L * rk->K, chunk = composed_chunk(h, batch, rk->K);
    const size_t S = (size_t)h->L * h->n * 32;
    if ((rc = ensure_need(h, need_relinearize(h, batch, rk->K, false, KS_C2)))) return rc;
    char *D = (char *)h->ws[WS1].p, *acc0 = D + (size_t)LK * chunk * S, *acc1 = acc0 + (size_t)chunk * S;
    for (uint32_t done = 0; done < batch; done += chunk) {
        const uint32_t nb = batch - done < chunk ? batch - done : chunk;
        const char *c2 = (const char *)d_c2 + (size_t)done * S;
        char *c0 = (char *)d_c0 + (size_t)done * S, *c1 = (char *)d_c1 + (size_t)done * S;
        if ((rc = relin_embed_mac(h, rk, D, acc0, acc1, c2, nb, 0))) return rc;
        if ((rc = do_forward(h, D, LK * nb))) return rc;
        if ((rc = relin_embed_mac(h, rk, D, acc0, acc1, c2, nb, 1))) return rc;
        if ((rc = do_inverse(h, acc0, nb))) return rc;
        if ((rc = do_inverse(h, acc1, nb))) return rc;
        if ((rc = do_ew<1>(h, c0, c0, acc0, nb, "relin add"))) return rc;
        if ((rc = do_ew<1>(h, c1, c1, acc1, nb, "relin add"))) return rc;
    }
    return FHE_OK;
}

static Pipeline ct_relin_pipeline(const fhe_rns_ntt *h, uint32_t batch, uint32_t K) {
    Pipeline pl;
    const LdsPlan T = plan_ct_multiply(h, (size_t)batch * h->L, false, true, true);
    const bool two = T.form == fhe_dev::LDS_TWO_LAUNCH;                  // at N >= 2^14: 128+ KiB of LDS per workgroup, the two stages cannot share a CU anyway
    pl.chunks = pipeline_chunks(h, batch, two && h->log_n >= 14 ? 1 : h->env.overlap_chunks);
    pl.add(T);                           // the two-launch form's workspace is sized for the whole batch, every chunk has its slice
    for (uint32_t c = 0; c < pl.chunks; c++) {
        const size_t polys = (size_t)(chunk_begin(batch, pl.chunks, c + 1) - chunk_begin(batch, pl.chunks, c)) * h->L;
        pl.add(pl.c[c].first = pl.chunks == 1 ? T : plan_ct_multiply(h, polys, false, true, false));
        pl.add(pl.c[c].ks = plan_keyswitch(h, polys, K, KS_FUSED, pl.chunks == 1 && !two));   // (the few-ciphertext parts take WS1: never beside the two-launch form)
    }
    return pl;
}
WsNeed need_ct_multiply_relin(const fhe_rns_ntt *h, uint32_t batch, uint32_t K, bool packed) {   // composed: the tensor product's c2 as containers in WS2
    return plan_fused_ct_relin(h, packed) ? ct_relin_pipeline(h, batch, K).need
                                          : WsNeed{0, (size_t)batch * h->L * h->n * 32, 0} | need_ct_multiply(h, batch, false) | need_relinearize(h, batch, K, packed, KS_C2_AS_IS);
}
// FHEContext::multiply as the reference declares it (src/fhe.cu:199-224: tensor product, then relinearize): (c0, c1) = relin(a (x) b).
// On the LDS-resident sizes of the word-sized classes the three components of the tensor product never take the 32-byte container
// form: the tensor-product kernel(s) write c0, c1, c2 to a compact workspace (sizeof(residue) bytes per coefficient) and the
// key-switch kernel reads its digit source (c2) and its addends (c0, c1) from there -- HBM traffic 4 S in + 2 S out + 3 compact
// components written once and read back (c2 by every limb workgroup) instead of 12 S.  Elsewhere: fhe_ct_multiply into a container
// workspace followed by fhe_ct_relinearize.  Same bits either way (tests compare both with the oracle).
extern "C" int fhe_ct_multiply_relin(fhe_rns_ntt_t *h, const fhe_relin_keys_t *rk, void *d_c0, void *d_c1, const void *d_a0, const void *d_a1,
                                     const void *d_b0, const void *d_b1, uint32_t batch) {
    int rc = check_call(h, batch, "ct_multiply_relin"); if (rc) return rc;
    if (!rk || !d_c0 || !d_c1 || !d_a0 || !d_a1 || !d_b0 || !d_b1) return fail(FHE_ERR_INVALID_ARG, "ct_multiply_relin: null argument");
    if ((rc = check_aligned({d_c0, d_c1, d_a0, d_a1, d_b0, d_b1}, "ct_multiply_relin"))) return rc;
    if (rk->owner != h) return fail(FHE_ERR_INVALID_ARG, "ct_multiply_relin: keys were imported for a different engine");
    const void *ins[4] = {d_a0, d_a1, d_b0, d_b1};
    for (const void *i : ins) if (d_c0 == i || d_c1 == i) return fail(FHE_ERR_INVALID_ARG, "ct_multiply_relin: outputs must not alias inputs");
    if (d_c0 == d_c1) return fail(FHE_ERR_INVALID_ARG, "ct_multiply_relin: outputs must be distinct");
    if ((rc = check_inputs(h, {d_a0, d_a1, d_b0, d_b1}, batch))) return rc;
    if (plan_fused_ct_relin(h, rk->d_pkb != nullptr)) {
        // The two kernels of the call sit on different roofs: the tensor product streams 4 S in at the HBM rate, the key switch (compact
        // operands) is bound by instruction issue.  The call is therefore a two-stage pipeline over chunks of whole ciphertexts: every
        // tensor product runs on the engine's stream, back to back; the key switch of chunk i runs on a second stream as soon as
        // tensor product i is done (event), i.e. beside tensor product i+1 on the same CUs.  The engine's stream joins the second one
        // at the end, so the call stays ordered on the engine's stream (and can be captured into a graph: fork / join through events).
        // Every chunk has its own slice of the compact workspace (and of the two-launch form's, sized for the whole batch).
        const Pipeline pl = ct_relin_pipeline(h, batch, rk->K);             // (its need is need_ct_multiply_relin's)
        if ((rc = ensure_need(h, pl.need)) || (pl.chunks > 1 && (rc = ensure_aux_stream(h)))) return rc;
        const size_t eb = residue_bytes(h), cbytes = (size_t)batch * h->L * h->n * eb;       // one compact component
        char *c0c = (char *)h->ws[WS2].p, *c1c = c0c + cbytes, *c2c = c1c + cbytes;
        const size_t S = (size_t)h->L * h->n * 32, Sc = (size_t)h->L * h->n * eb;   // bytes of one ciphertext component: containers / compact
        for (uint32_t c = 0; c < pl.chunks; c++) {
            const uint32_t b0 = chunk_begin(batch, pl.chunks, c), nb = chunk_begin(batch, pl.chunks, c + 1) - b0;
            const size_t o = (size_t)b0 * S, oc = (size_t)b0 * Sc;
            fhe_dev::LdsArgs A = lds_args(h, fhe_dev::LDS_CT_MULTIPLY, pl.c[c].first, nb * h->L);
            A.r0 = c0c + oc; A.r1 = c1c + oc; A.r2 = c2c + oc; A.out_compact = true;
            A.a0 = (const char *)d_a0 + o; A.a1 = (const char *)d_a1 + o; A.b0 = (const char *)d_b0 + o; A.b1 = (const char *)d_b1 + o;
            if (A.ws && A.form == fhe_dev::LDS_TWO_LAUNCH) A.ws = (char *)A.ws + 2 * oc;   // two compact polynomials per limb polynomial of the chunk
            if ((rc = lds_launch(h, A, "tensor product (compact outputs)"))) return rc;
            if (pl.chunks > 1 && (rc = fork_chunk(h, c))) return rc;
            if ((rc = lds_launch(h, keyswitch_args(h, rk, pl.c[c].ks, (char *)d_c0 + o, (char *)d_c1 + o, c2c + oc, c0c + oc, c1c + oc, nb * h->L,
                                                   pl.chunks > 1 ? h->aux_stream : h->stream), "key switch (compact operands)"))) return rc;
        }
        return pl.chunks > 1 ? join_chunks(h) : FHE_OK;
    }
    if ((rc = ensure_need(h, need_ct_multiply_relin(h, batch, rk->K, rk->d_pkb != nullptr)))) return rc;
    if ((rc = do_ct_multiply(h, d_c0, d_c1, h->ws[WS2].p, d_a0, d_a1, d_b0, d_b1, batch))) return rc;
    return fhe_ct_relinearize(h, rk, d_c0, d_c1, h->ws[WS2].p, batch);
}


// ------------------------------------------------------------------------------------------------------
// Galois automorphisms and slot rotations (FHEContext::rotate_rows / rotate_columns, include/fhe.cuh:112-116)
// ------------------------------------------------------------------------------------------------------
extern "C" int fhe_galois_element(uint32_t n, int32_t steps, uint32_t *elt) {
    if (!elt) return fail(FHE_ERR_INVALID_ARG, "galois_element: elt is null");
    if (n < 8 || n > (1u << 30) || (n & (n - 1))) return fail(FHE_ERR_INVALID_ARG, "galois_element: n must be a power of two in [8, 2^30]");
    const uint32_t half = n / 2, m = 2 * n;                          // 3 generates a cyclic subgroup of order n/2 of (Z/2n)^*
    const uint32_t e = (uint32_t)(((int64_t)steps % half + half) % half);
    uint64_t r = 1, b = 3;
    for (uint32_t k = e; k; k >>= 1) { if (k & 1) r = r * b % m; b = b * b % m; }
    *elt = (uint32_t)r;
    return FHE_OK;
}
int check_galois_element(const fhe_rns_ntt *h, uint32_t g, const char *what) {
    if (!(g & 1) || g >= 2 * h->n)
        return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": the Galois element must be odd and below 2n");
    return FHE_OK;
}
static uint32_t galois_inverse(const fhe_rns_ntt *h, uint32_t g) {    // g^-1 mod 2n (g odd): Newton iteration modulo 2^32, then reduced
    uint32_t x = g;
    for (int i = 0; i < 5; i++) x *= 2 - g * x;
    return x & (2 * h->n - 1);
}
// sigma_g of one or two components (in1 == nullptr: one) into out0 / out1, zero_out (optional) cleared beside them; compact: E per coefficient out.
// The staged form up to 32 KiB per limb polynomial (4-byte residues up to N = 8192, 8-byte ones up to 4096), the L2 gather above: the interleaved
// A/B of scratch/galois_ab.hip had the staged form 13 % faster at 32 KiB and 8-14 % slower at 64 KiB (two workgroups per CU).
template <class F>
static int galois_word(fhe_rns_ntt *h, void *out0, void *out1, void *zero_out, const void *in0, const void *in1, uint32_t g_inv, size_t polys, bool compact) {
    using V = typename F::V16; using E = typename F::E;
    const uint32_t comps = in1 ? 2 : 1;
    const size_t lds = (size_t)h->n * sizeof(E);
    const bool staged = lds <= fhe_dev::GALOIS_STAGE_BYTES;
    const dim3 block(fhe_dev::GALOIS_T), grid(staged ? (unsigned)std::min<size_t>(polys, 1u << 20) : ew_grid(polys * h->n), comps);
    const fhe_dev::Limb<F> *limbs = (const fhe_dev::Limb<F> *)h->d_limbs;
    if (compact) {
        if (staged) hipLaunchKernelGGL((fhe_dev::galois_compact_kernel<F, true>), grid, block, lds, h->stream, (E *)out0, (E *)out1, (E *)zero_out, (const V *)in0, (const V *)in1, limbs, h->L, h->log_n, g_inv, polys);
        else hipLaunchKernelGGL((fhe_dev::galois_compact_kernel<F, false>), grid, block, 0, h->stream, (E *)out0, (E *)out1, (E *)zero_out, (const V *)in0, (const V *)in1, limbs, h->L, h->log_n, g_inv, polys);
        return post_launch(h->stream, "galois_compact_kernel");
    }
    if (staged) hipLaunchKernelGGL((fhe_dev::galois_kernel<F, true>), grid, block, lds, h->stream, (V *)out0, (V *)out1, (V *)zero_out, (const V *)in0, (const V *)in1, limbs, h->L, h->log_n, g_inv, polys);
    else hipLaunchKernelGGL((fhe_dev::galois_kernel<F, false>), grid, block, 0, h->stream, (V *)out0, (V *)out1, (V *)zero_out, (const V *)in0, (const V *)in1, limbs, h->L, h->log_n, g_inv, polys);
    return post_launch(h->stream, "galois_kernel");
}
int do_galois(fhe_rns_ntt *h, void *out0, void *out1, void *zero_out, const void *in0, const void *in1, uint32_t g, size_t polys, bool compact) {
    const uint32_t g_inv = galois_inverse(h, g);
    if (h->width != FHE_WIDTH_256) return with_word_field(h, [&](auto f) { return galois_word<decltype(f)>(h, out0, out1, zero_out, in0, in1, g_inv, polys, compact); });
    if (compact) return fail(FHE_ERR_UNSUPPORTED, "compact polynomials exist on the word-sized classes only");
    const size_t count = polys * h->n;
    hipLaunchKernelGGL(fhe_dev::galois256_kernel, dim3(ew_grid(count), in1 ? 2 : 1), dim3(fhe_dev::GALOIS_T), 0, h->stream, (fhe_dev::u256 *)out0,
                       (fhe_dev::u256 *)out1, (fhe_dev::u256 *)zero_out, (const fhe_dev::u256 *)in0, (const fhe_dev::u256 *)in1,
                       (const fhe_dev::Limb256 *)h->d_limbs, h->L, h->log_n, g_inv, count);
    return post_launch(h->stream, "galois256_kernel");
}
extern "C" int fhe_rns_automorphism(fhe_rns_ntt_t *h, void *d_out, const void *d_in, uint32_t galois_elt, uint32_t batch) {
    int rc = check_call(h, batch, "automorphism"); if (rc) return rc;
    if (!d_out || !d_in) return fail(FHE_ERR_INVALID_ARG, "automorphism: null argument");
    if ((rc = check_aligned({d_out, d_in}, "automorphism"))) return rc;
    if (d_out == d_in) return fail(FHE_ERR_INVALID_ARG, "automorphism: the permutation is out of place (out must differ from in)");
    if ((rc = check_galois_element(h, galois_elt, "automorphism"))) return rc;
    if ((rc = check_inputs(h, {d_in}, batch))) return rc;
    return do_galois(h, d_out, nullptr, nullptr, d_in, nullptr, galois_elt, (size_t)batch * h->L, false);
}
// (c0, c1) -> (sigma(c0) + sum D(sigma(c1)) b, sum D(sigma(c1)) a): bit for bit fhe_ct_relinearize applied to (sigma(c0), 0, sigma(c1)).
// Fused path (the LDS-resident word-sized sizes with packed keys, as plan_fused_ct_relin): the prologue writes sigma(c0), sigma(c1) and a zero
// polynomial as compact polynomials into the three slices of WS2 that fhe_ct_multiply_relin uses, then ONE compact-operand key switch
// (KS_FUSED) reads them -- HBM traffic 2 S in + 2 S out plus the compact round trip.  Elsewhere: sigma(c0) -> out0, zero -> out1 and
// sigma(c1) -> WS2 as containers in one launch, then fhe_ct_relinearize.
WsNeed need_apply_galois(const fhe_rns_ntt *h, uint32_t batch, uint32_t K, bool packed) {
    if (plan_fused_ct_relin(h, packed) && !h->env.no_fused_galois) return plan_keyswitch(h, (size_t)batch * h->L, K, KS_FUSED, true).need();
    return WsNeed{0, (size_t)batch * h->L * h->n * 32, 0} | need_relinearize(h, batch, K, packed, KS_C2_AS_IS);
}
extern "C" int fhe_ct_apply_galois(fhe_rns_ntt_t *h, const fhe_relin_keys_t *gk, uint32_t galois_elt, void *d_out0, void *d_out1, const void *d_c0,
                                   const void *d_c1, uint32_t batch) {
    int rc = check_call(h, batch, "ct_apply_galois"); if (rc) return rc;
    if (!gk || !d_out0 || !d_out1 || !d_c0 || !d_c1) return fail(FHE_ERR_INVALID_ARG, "ct_apply_galois: null argument");
    if ((rc = check_aligned({d_out0, d_out1, d_c0, d_c1}, "ct_apply_galois"))) return rc;
    if (gk->owner != h) return fail(FHE_ERR_INVALID_ARG, "ct_apply_galois: keys were imported for a different engine");
    if (d_out0 == d_out1) return fail(FHE_ERR_INVALID_ARG, "ct_apply_galois: outputs must be distinct");
    for (const void *i : {d_c0, d_c1}) if (d_out0 == i || d_out1 == i) return fail(FHE_ERR_INVALID_ARG, "ct_apply_galois: outputs must not alias inputs");
    if ((rc = check_galois_element(h, galois_elt, "ct_apply_galois"))) return rc;
    if ((rc = check_inputs(h, {d_c0, d_c1}, batch))) return rc;
    const size_t polys = (size_t)batch * h->L;
    if ((rc = ensure_need(h, need_apply_galois(h, batch, gk->K, gk->d_pkb != nullptr)))) return rc;
    if (plan_fused_ct_relin(h, gk->d_pkb != nullptr) && !h->env.no_fused_galois) {
        const size_t cbytes = polys * h->n * residue_bytes(h);
        char *s0 = (char *)h->ws[WS2].p, *s1 = s0 + cbytes, *zero = s1 + cbytes;      // sigma(c0): addend of c0'; sigma(c1): digit source; 0: addend of c1'
        const LdsPlan P = plan_keyswitch(h, polys, gk->K, KS_FUSED, true);
        if ((rc = do_galois(h, s0, s1, zero, d_c0, d_c1, galois_elt, polys, true))) return rc;
        return lds_launch(h, keyswitch_args(h, gk, P, d_out0, d_out1, s1, s0, zero, (uint32_t)polys, h->stream), "key switch (rotation)");
    }
    if ((rc = do_galois(h, d_out0, h->ws[WS2].p, d_out1, d_c0, d_c1, galois_elt, polys, false))) return rc;
    return fhe_ct_relinearize(h, gk, d_out0, d_out1, h->ws[WS2].p, batch);
}

// ------------------------------------------------------------------------------------------------------
// Hoisted rotations (Halevi-Shoup): fhe_ct_hoist decomposes and transforms c1 once, every fhe_ct_apply_galois_hoisted is a permuted
// multiply-accumulate with the key rows, two inverse transforms and sigma_g(c0)   (semantics and pi_g: include/fhe_hip.h)
// ------------------------------------------------------------------------------------------------------
// Fused path (plan_fused_hoist; kernels: hoist.hip.h): c1 compacted into WS2, ntt_hoist_kernel writes the L K L kept polynomials as
// residues; a rotation is the one-component automorphism of c0 into WS2 (compact) and ntt_hoist_apply_kernel.  Composed path: the
// digit polynomials as containers [jk][b][i] (digit_embed + forward transform); a rotation is relin_mac_perm (first sum into WS1, second
// into out1), two inverse transforms, sigma_g(c0) into out0 and an addition.  A key set that kept only its packed tables (N = 2^15,
// FHE_HIP_NO_FUSED_HOIST=1) is read from those (relin_mac_perm_packed_kernel): key import is the same with and without hoisting.
static bool hoist_fused(const fhe_rns_ntt *h, uint32_t w, uint32_t K) { return plan_fused_hoist(h, keys_get_packed(h, w, K)); }
static size_t hoist_size(const fhe_rns_ntt *h, uint32_t batch, uint32_t K, bool fused) {
    return (size_t)batch * h->L * K * h->L * h->n * (fused ? residue_bytes(h) : 32);
}
static WsNeed need_hoist(const fhe_rns_ntt *h, uint32_t batch, uint32_t K, bool fused) {   // of fhe_ct_hoist and fhe_ct_apply_galois_hoisted together
    const size_t polys = (size_t)batch * h->L;
    if (fused) return {0, polys * h->n * residue_bytes(h), 0};                 // compact c1, then compact sigma_g(c0)
    return WsNeed{polys * h->n * 32, 0, 0} | need_transform(h, polys * h->L * K) | need_transform(h, polys);
}
static int ensure_hoist(fhe_rns_ntt *h, uint32_t batch, uint32_t K, bool fused) {
    int rc = ensure_need(h, need_hoist(h, batch, K, fused)); if (rc) return rc;
    const size_t bytes = hoist_size(h, batch, K, fused);
    if (h->ws[WS_HOIST].bytes < bytes) h->hoist.valid = false;                       // growing drops what was kept
    return grow_ws(h, h->ws[WS_HOIST], bytes);
}
static int check_hoist_call(const fhe_rns_ntt *h, uint32_t decomp_bits, uint32_t batch, const char *what) {
    int rc = check_call(h, batch, what); if (rc) return rc;
    if (decomp_bits < 1 || decomp_bits > 64) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": decomp_bits must be in [1, 64]");
    if ((uint64_t)batch * h->L * h->L > 0x7fffffffull) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": batch * num_primes^2 too large");
    return FHE_OK;
}
extern "C" int fhe_rns_ntt_reserve_hoist(fhe_rns_ntt_t *h, uint32_t decomp_bits, uint32_t batch) {
    int rc = check_hoist_call(h, decomp_bits, batch, "reserve_hoist"); if (rc) return rc;
    const uint32_t K = relin_digits(h, decomp_bits);
    return ensure_hoist(h, batch, K, hoist_fused(h, decomp_bits, K));
}
extern "C" int fhe_rns_ntt_hoist_bytes(const fhe_rns_ntt_t *h, uint64_t *bytes) {
    if (!h || !bytes) return fail(FHE_ERR_INVALID_ARG, "hoist_bytes: null argument");
    *bytes = (uint64_t)h->ws[WS_HOIST].bytes;
    return FHE_OK;
}
extern "C" int fhe_ct_hoist(fhe_rns_ntt_t *h, uint32_t decomp_bits, const void *d_c1, uint32_t batch) {
    int rc = check_hoist_call(h, decomp_bits, batch, "ct_hoist"); if (rc) return rc;
    if (!d_c1) return fail(FHE_ERR_INVALID_ARG, "ct_hoist: null argument");
    if ((rc = check_aligned({d_c1}, "ct_hoist"))) return rc;
    if ((rc = check_inputs(h, {d_c1}, batch))) return rc;
    const uint32_t K = relin_digits(h, decomp_bits);
    const bool fused = hoist_fused(h, decomp_bits, K);
    h->hoist.valid = false;
    if ((rc = ensure_hoist(h, batch, K, fused))) return rc;
    if (fused) {
        if ((rc = compact_poly(h, h->ws[WS2].p, d_c1, (size_t)batch * h->L * h->n))) return rc;
        fhe_dev::LdsArgs A = lds_args(h, fhe_dev::LDS_HOIST, {}, batch * h->L * h->L);
        A.r0 = h->ws[WS_HOIST].p; A.c2 = h->ws[WS2].p; A.in_compact = true; A.K = K; A.w = decomp_bits;
        if ((rc = lds_launch(h, A, "ntt_hoist_kernel"))) return rc;
    } else {
        if ((rc = embed_digits(h, (char *)h->ws[WS_HOIST].p, d_c1, K, decomp_bits, batch))) return rc;
        if ((rc = do_forward(h, h->ws[WS_HOIST].p, h->L * K * batch))) return rc;
    }
    h->hoist.valid = true; h->hoist.fused = fused; h->hoist.w = decomp_bits; h->hoist.K = K; h->hoist.batch = batch;
    return FHE_OK;
}
static int relin_mac_perm(fhe_rns_ntt *h, const fhe_relin_keys *gk, void *acc0, void *acc1, uint32_t g, uint32_t batch) {
    const uint32_t LK = h->L * gk->K;
    const size_t count = (size_t)batch * h->L * h->n;
    if (h->width != FHE_WIDTH_256) return with_word_field(h, [&](auto f) {
        using F = decltype(f); using V = typename F::V16;
        if (!gk->d_kb) {
            hipLaunchKernelGGL((fhe_dev::relin_mac_perm_packed_kernel<F>), dim3(ew_grid(count * 2)), dim3(256), 0, h->stream, (V *)acc0, (V *)acc1, (const V *)h->ws[WS_HOIST].p,
                               (const typename F::E *)gk->d_pkb, (const typename F::E *)gk->d_pka, (const fhe_dev::Limb<F> *)h->d_limbs, h->L, h->log_n, LK, batch, g);
            return post_launch(h->stream, "relin_mac_perm_packed_kernel");
        }
        hipLaunchKernelGGL((fhe_dev::relin_mac_perm_kernel<F>), dim3(ew_grid(count * 2)), dim3(256), 0, h->stream, (V *)acc0, (V *)acc1, (const V *)h->ws[WS_HOIST].p,
                           (const V *)gk->d_kb, (const V *)gk->d_ka, (const fhe_dev::Limb<F> *)h->d_limbs, h->L, h->log_n, LK, batch, g);
        return post_launch(h->stream, "relin_mac_perm_kernel");
    });
    hipLaunchKernelGGL(fhe_dev::relin_mac_perm256_kernel, dim3(ew_grid(count)), dim3(256), 0, h->stream, (fhe_dev::u256 *)acc0, (fhe_dev::u256 *)acc1,
                       (const fhe_dev::u256 *)h->ws[WS_HOIST].p, (const fhe_dev::u256 *)gk->d_kb, (const fhe_dev::u256 *)gk->d_ka,
                       (const fhe_dev::Limb256 *)h->d_limbs, h->L, h->log_n, LK, batch, g);
    return post_launch(h->stream, "relin_mac_perm256_kernel");
}
extern "C" int fhe_ct_apply_galois_hoisted(fhe_rns_ntt_t *h, const fhe_relin_keys_t *gk, uint32_t galois_elt, void *d_out0, void *d_out1,
                                           const void *d_c0, uint32_t batch) {
    int rc = check_call(h, batch, "ct_apply_galois_hoisted"); if (rc) return rc;
    if (!gk || !d_out0 || !d_out1 || !d_c0) return fail(FHE_ERR_INVALID_ARG, "ct_apply_galois_hoisted: null argument");
    if ((rc = check_aligned({d_out0, d_out1, d_c0}, "ct_apply_galois_hoisted"))) return rc;
    if (gk->owner != h) return fail(FHE_ERR_INVALID_ARG, "ct_apply_galois_hoisted: keys were imported for a different engine");
    if (d_out0 == d_out1 || d_out0 == d_c0 || d_out1 == d_c0) return fail(FHE_ERR_INVALID_ARG, "ct_apply_galois_hoisted: outputs must be distinct from each other and from c0");
    if ((rc = check_galois_element(h, galois_elt, "ct_apply_galois_hoisted"))) return rc;
    if (!h->hoist.valid) return fail(FHE_ERR_INVALID_ARG, "ct_apply_galois_hoisted: no fhe_ct_hoist on this engine yet (or its workspace was re-sized since)");
    if (batch != h->hoist.batch) return fail(FHE_ERR_INVALID_ARG, "ct_apply_galois_hoisted: batch differs from the hoisted one");
    if (gk->decomp_bits != h->hoist.w) return fail(FHE_ERR_INVALID_ARG, "ct_apply_galois_hoisted: the keys' decomp_bits differ from the hoisted ones");
    if (h->hoist.fused ? !gk->d_pkb : (!gk->d_kb && !gk->d_pkb)) return fail(FHE_ERR_INVALID_ARG, "ct_apply_galois_hoisted: the key set does not have the tables this engine's hoist path reads");
    if ((rc = check_inputs(h, {d_c0}, batch))) return rc;
    if ((rc = ensure_hoist(h, batch, gk->K, h->hoist.fused))) return rc;       // (no-op after fhe_ct_hoist: the workspaces only ever grow)
    const size_t polys = (size_t)batch * h->L;
    if (h->hoist.fused) {
        if ((rc = do_galois(h, h->ws[WS2].p, nullptr, nullptr, d_c0, nullptr, galois_elt, polys, true))) return rc;
        fhe_dev::LdsArgs A = lds_args(h, fhe_dev::LDS_HOIST_APPLY, {}, (uint32_t)polys);
        A.r0 = d_out0; A.r1 = d_out1; A.c2 = h->ws[WS_HOIST].p; A.add0 = h->ws[WS2].p; A.in_compact = A.add_compact = true;
        A.kb = gk->d_pkb; A.ka = gk->d_pka; A.K = gk->K; A.galois = galois_elt;
        return lds_launch(h, A, "ntt_hoist_apply_kernel");
    }
    if ((rc = relin_mac_perm(h, gk, h->ws[WS1].p, d_out1, galois_elt, batch))) return rc;
    if ((rc = do_inverse(h, h->ws[WS1].p, batch))) return rc;
    if ((rc = do_inverse(h, d_out1, batch))) return rc;
    if ((rc = do_galois(h, d_out0, nullptr, nullptr, d_c0, nullptr, galois_elt, polys, false))) return rc;
    return do_ew<1>(h, d_out0, d_out0, h->ws[WS1].p, batch, "hoisted rotation add");
}

// ------------------------------------------------------------------------------------------------------
// Hoisted linear transform: out = sum_t p_t * hoisted_rotation(ct, g_t) from one kept decomposition   (semantics: include/fhe_hip.h)
// ------------------------------------------------------------------------------------------------------
// Fused path (plan_fused_lincomb, every keyed term with packed tables; kernels: hoist_lincomb.hip.h): the plaintexts are kept transformed and
// packed like key rows, the terms sit in a device table, and a call is two launches whatever G is: c0 (and c1, where a term has no key)
// forward into WS_LIN in the hoist layout, then ntt_hoist_lincomb_kernel.  Composed path: the plaintexts are kept as given, and every term is
// fhe_ct_apply_galois_hoisted into WS_LIN (the first term: into the outputs), fhe_rns_ntt_multiply_bcast and fhe_rns_poly_add.
struct fhe_linear_transform {
    fhe_rns_ntt *owner = nullptr;
    uint32_t decomp_bits = 0, K = 0;
    bool fused = false, keyless = false;            // fused: the LDS kernels run it; keyless: some term has no key (the call needs c1)
    std::vector<uint32_t> g;
    std::vector<const fhe_relin_keys *> gk;         // referenced, not owned
    void *d_plain = nullptr;                        // fused: [G][L][n] residues, transformed and packed; composed: [G][L][n] containers, coefficient form
    void *d_terms = nullptr;                        // fused: LincombTerm[G]
};
extern "C" int fhe_linear_transform_destroy(fhe_linear_transform_t *lt) {
    if (lt) {
        for (void *p : {lt->d_plain, lt->d_terms}) if (p) (void)hipFree(p);
        delete lt;
    }
    return FHE_OK;
}
extern "C" int fhe_linear_transform_create(fhe_rns_ntt_t *h, fhe_linear_transform_t **out, uint32_t decomp_bits, const uint32_t *galois_elts,
                                           const fhe_relin_keys_t *const *gks, const void *const *d_plain, uint32_t num_terms) {
    if (!h || !out || !galois_elts || !gks || !d_plain) return fail(FHE_ERR_INVALID_ARG, "linear_transform_create: null argument");
    int rc = check_hoist_call(h, decomp_bits, 1, "linear_transform_create"); if (rc) return rc;
    if (num_terms < 1 || num_terms > FHE_LINEAR_TRANSFORM_MAX_TERMS) return fail(FHE_ERR_INVALID_ARG, "linear_transform_create: num_terms must be in [1, FHE_LINEAR_TRANSFORM_MAX_TERMS]");
    const uint32_t K = relin_digits(h, decomp_bits);
    bool fused = plan_fused_lincomb(h, keys_get_packed(h, decomp_bits, K)), keyless = false;
    for (uint32_t t = 0; t < num_terms; t++) {
        if ((rc = check_galois_element(h, galois_elts[t], "linear_transform_create"))) return rc;
        if (!d_plain[t]) return fail(FHE_ERR_INVALID_ARG, "linear_transform_create: null plaintext pointer");
        if ((rc = check_aligned({d_plain[t]}, "linear_transform_create"))) return rc;
        const fhe_relin_keys *gk = gks[t];
        if (!gk) {
            if (galois_elts[t] != 1) return fail(FHE_ERR_INVALID_ARG, "linear_transform_create: a term without a key set must have Galois element 1");
            keyless = true;
            continue;
        }
        if (gk->owner != h) return fail(FHE_ERR_INVALID_ARG, "linear_transform_create: keys were imported for a different engine");
        if (gk->decomp_bits != decomp_bits) return fail(FHE_ERR_INVALID_ARG, "linear_transform_create: a key set's decomp_bits differ from the transform's");
        fused = fused && gk->d_pkb;
        if (!gk->d_pkb && !gk->d_kb) return fail(FHE_ERR_INVALID_ARG, "linear_transform_create: a key set has no tables");
    }
    fhe_linear_transform *lt = new (std::nothrow) fhe_linear_transform();
    if (!lt) return fail(FHE_ERR_INVALID_ARG, "out of host memory");
    lt->owner = h; lt->decomp_bits = decomp_bits; lt->K = K; lt->fused = fused; lt->keyless = keyless;
    lt->g.assign(galois_elts, galois_elts + num_terms); lt->gk.assign(gks, gks + num_terms);
    const size_t S = (size_t)h->L * h->n * 32;
    Scratch scratch;
    auto body = [&]() -> int {
        void *d_copy = nullptr;                      // the plaintexts as containers: scratch of the fused path, the transform's own copy otherwise
        if (fused) { if (int r = scratch.get(&d_copy, S * num_terms)) return r; }
        else { HIP_TRY(hipMalloc(&lt->d_plain, S * num_terms)); d_copy = lt->d_plain; }
        for (uint32_t t = 0; t < num_terms; t++) HIP_TRY(hipMemcpyAsync((char *)d_copy + t * S, d_plain[t], S, hipMemcpyDeviceToDevice, h->stream));
        if (!fused) return post_launch(h->stream, "linear_transform_create copy");
        if (int r = do_forward(h, d_copy, num_terms)) return r;
        std::vector<fhe_dev::LincombTerm> terms(num_terms);
        HIP_TRY(hipMalloc(&lt->d_plain, num_terms * packed_row_bytes(h)));
        HIP_TRY(hipMalloc(&lt->d_terms, num_terms * sizeof(fhe_dev::LincombTerm)));
        if (int r = pack_rows(h, lt->d_plain, d_copy, num_terms, "pack_keys_kernel (plaintexts)")) return r;
        for (uint32_t t = 0; t < num_terms; t++)
            terms[t] = {gks[t] ? gks[t]->d_pkb : nullptr, gks[t] ? gks[t]->d_pka : nullptr, (const char *)lt->d_plain + t * packed_row_bytes(h), galois_elts[t], 0};
        HIP_TRY(hipMemcpyAsync(lt->d_terms, terms.data(), num_terms * sizeof(fhe_dev::LincombTerm), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));     // `terms` leaves scope; the scratch is freed when the call returns
        return FHE_OK;
    };
    if ((rc = body())) { fhe_linear_transform_destroy(lt); return rc; }
    *out = lt;
    return FHE_OK;
}
// bytes of WS_LIN for `batch` ciphertexts: c0^ and c1^ as residues, or two container components
static size_t lincomb_scratch(const fhe_rns_ntt *h, const fhe_linear_transform *lt, uint32_t batch) {
    return (size_t)batch * h->L * h->n * (lt->fused ? (lt->keyless ? 2 : 1) * residue_bytes(h) : 2 * 32);
}
static int ensure_lincomb(fhe_rns_ntt *h, const fhe_linear_transform *lt, uint32_t batch) {
    int rc = ensure_hoist(h, batch, lt->K, hoist_fused(h, lt->decomp_bits, lt->K)); if (rc) return rc;
    if (!lt->fused && (rc = ensure_need(h, need_multiply(h, batch)))) return rc;
    return grow_ws(h, h->ws[WS_LIN], lincomb_scratch(h, lt, batch));
}
extern "C" int fhe_linear_transform_reserve(fhe_rns_ntt_t *h, const fhe_linear_transform_t *lt, uint32_t batch) {
    if (!h || !lt) return fail(FHE_ERR_INVALID_ARG, "linear_transform_reserve: null argument");
    int rc = check_hoist_call(h, lt->decomp_bits, batch, "linear_transform_reserve"); if (rc) return rc;
    if (lt->owner != h) return fail(FHE_ERR_INVALID_ARG, "linear_transform_reserve: the transform was created for a different engine");
    return ensure_lincomb(h, lt, batch);
}
extern "C" int fhe_ct_linear_transform_hoisted(fhe_rns_ntt_t *h, const fhe_linear_transform_t *lt, void *d_out0, void *d_out1, const void *d_c0,
                                               const void *d_c1, uint32_t batch) {
    int rc = check_call(h, batch, "ct_linear_transform_hoisted"); if (rc) return rc;
    if (!lt || !d_out0 || !d_out1 || !d_c0) return fail(FHE_ERR_INVALID_ARG, "ct_linear_transform_hoisted: null argument");
    if (lt->owner != h) return fail(FHE_ERR_INVALID_ARG, "ct_linear_transform_hoisted: the transform was created for a different engine");
    if (lt->keyless && !d_c1) return fail(FHE_ERR_INVALID_ARG, "ct_linear_transform_hoisted: a term without a key set needs c1");
    if ((rc = check_aligned({d_out0, d_out1, d_c0, d_c1}, "ct_linear_transform_hoisted"))) return rc;
    if (d_out0 == d_out1) return fail(FHE_ERR_INVALID_ARG, "ct_linear_transform_hoisted: outputs must be distinct");
    for (const void *i : {d_c0, d_c1}) if (d_out0 == i || d_out1 == i) return fail(FHE_ERR_INVALID_ARG, "ct_linear_transform_hoisted: outputs must not alias inputs");
    if (!h->hoist.valid) return fail(FHE_ERR_INVALID_ARG, "ct_linear_transform_hoisted: no fhe_ct_hoist on this engine yet (or its workspace was re-sized since)");
    if (batch != h->hoist.batch) return fail(FHE_ERR_INVALID_ARG, "ct_linear_transform_hoisted: batch differs from the hoisted one");
    if (lt->decomp_bits != h->hoist.w) return fail(FHE_ERR_INVALID_ARG, "ct_linear_transform_hoisted: the transform's decomp_bits differ from the hoisted ones");
    if (lt->fused && !h->hoist.fused) return fail(FHE_ERR_INVALID_ARG, "ct_linear_transform_hoisted: the kept decomposition is not in the layout this transform reads");
    if ((rc = check_inputs(h, {d_c0}, batch)) || (lt->keyless && (rc = check_inputs(h, {d_c1}, batch)))) return rc;
    if ((rc = ensure_lincomb(h, lt, batch))) return rc;                       // (no-op after fhe_linear_transform_reserve)
    if (!h->hoist.valid) return fail(FHE_ERR_INVALID_ARG, "ct_linear_transform_hoisted: the hoist workspace had to grow, which drops the kept decomposition: hoist again");
    const uint32_t polys = batch * h->L, G = (uint32_t)lt->g.size();
    if (lt->fused) {
        fhe_dev::LdsArgs A = lds_args(h, fhe_dev::LDS_HOIST_FWD, {}, polys);
        A.r0 = h->ws[WS_LIN].p; A.a0 = d_c0; A.a1 = lt->keyless ? d_c1 : nullptr; A.out_compact = true;
        if ((rc = lds_launch(h, A, "ntt_hoist_fwd_kernel"))) return rc;
        fhe_dev::LdsArgs B = lds_args(h, fhe_dev::LDS_HOIST_LINCOMB, {}, polys);
        B.r0 = d_out0; B.r1 = d_out1; B.c2 = h->ws[WS_HOIST].p; B.add0 = h->ws[WS_LIN].p; B.in_compact = B.add_compact = true;
        B.add1 = lt->keyless ? (const char *)h->ws[WS_LIN].p + (size_t)polys * h->n * residue_bytes(h) : nullptr;
        B.terms = lt->d_terms; B.num_terms = G; B.K = lt->K;
        return lds_launch(h, B, "ntt_hoist_lincomb_kernel");
    }
    const size_t S = (size_t)h->L * h->n * 32;
    char *s0 = (char *)h->ws[WS_LIN].p, *s1 = s0 + (size_t)batch * S;
    for (uint32_t t = 0; t < G; t++) {
        void *t0 = t ? (void *)s0 : d_out0, *t1 = t ? (void *)s1 : d_out1;    // the first term goes straight to the outputs
        const void *pt = (const char *)lt->d_plain + (size_t)t * S;
        if (lt->gk[t]) {
            if ((rc = fhe_ct_apply_galois_hoisted(h, lt->gk[t], lt->g[t], t0, t1, d_c0, batch))) return rc;
            if ((rc = fhe_rns_ntt_multiply_bcast(h, t0, t0, pt, batch)) || (rc = fhe_rns_ntt_multiply_bcast(h, t1, t1, pt, batch))) return rc;
        } else if ((rc = fhe_rns_ntt_multiply_bcast(h, t0, d_c0, pt, batch)) || (rc = fhe_rns_ntt_multiply_bcast(h, t1, d_c1, pt, batch))) return rc;
        if (t && ((rc = fhe_rns_poly_add(h, d_out0, d_out0, s0, batch)) || (rc = fhe_rns_poly_add(h, d_out1, d_out1, s1, batch)))) return rc;
    }
    return FHE_OK;
}

// ------------------------------------------------------------------------------------------------------
// blind-rotation inner loop
// ------------------------------------------------------------------------------------------------------
static int monomial_compact(fhe_rns_ntt *h, void *out, const void *in, const uint32_t *shifts, size_t count) {   // (X^shift - 1) * p on compact polynomials
    return with_word_field(h, [&](auto f) {
        using F = decltype(f);
        hipLaunchKernelGGL((fhe_dev::monomial_compact_kernel<F>), dim3(ew_grid(count)), dim3(256), 0, h->stream, (typename F::E *)out, (const typename F::E *)in, shifts,
                           (const fhe_dev::Limb<F> *)h->d_limbs, h->L, h->log_n, count);
        return post_launch(h->stream, "monomial_compact_kernel");
    });
}

template <class F>
static int monomial_lds(fhe_rns_ntt *h, void *out, const void *in, const uint32_t *shifts, uint32_t batch) {
    using V = typename F::V16;
    size_t halves = (size_t)batch * h->L * h->n * 2;
    hipLaunchKernelGGL((fhe_dev::monomial_mul_sub_kernel<F>), dim3(ew_grid(halves)), dim3(256), 0, h->stream, (V *)out, (const V *)in, shifts,
                       (const fhe_dev::Limb<F> *)h->d_limbs, h->L, h->log_n, halves);
    return post_launch(h->stream, "monomial_mul_sub_kernel");
}
extern "C" int fhe_rns_monomial_mul_sub(fhe_rns_ntt_t *h, void *d_out, const void *d_in, const uint32_t *d_shifts, uint32_t batch) {
    int rc = check_call(h, batch, "monomial_mul_sub"); if (rc) return rc;
    if (!d_out || !d_in || !d_shifts || d_out == d_in) return fail(FHE_ERR_INVALID_ARG, "monomial_mul_sub: null or aliased argument");
    if ((rc = check_aligned({d_out, d_in}, "monomial_mul_sub"))) return rc;
    if (h->width != FHE_WIDTH_256) return with_word_field(h, [&](auto f) { return monomial_lds<decltype(f)>(h, d_out, d_in, d_shifts, batch); });
    size_t count = (size_t)batch * h->L * h->n;
    hipLaunchKernelGGL(fhe_dev::monomial_mul_sub256_kernel, dim3(ew_grid(count)), dim3(256), 0, h->stream, (fhe_dev::u256 *)d_out,
                       (const fhe_dev::u256 *)d_in, d_shifts, (const fhe_dev::Limb256 *)h->d_limbs, h->L, h->log_n, count);
    return post_launch(h->stream, "monomial_mul_sub256_kernel");
}
// One step on the general composition (any width class): d = (X^a - 1) * acc, then two key switches accumulate into acc in place.
static int blind_rotate_step_general(fhe_rns_ntt_t *h, const fhe_relin_keys_t *rows_c0, const fhe_relin_keys_t *rows_c1, void *d_acc0, void *d_acc1,
                                     const uint32_t *d_shifts, void *d_tmp0, void *d_tmp1, uint32_t batch) {
    int rc;
    if ((rc = fhe_rns_monomial_mul_sub(h, d_tmp0, d_acc0, d_shifts, batch))) return rc;       // d0 = (X^a - 1) * acc0
    if ((rc = fhe_rns_monomial_mul_sub(h, d_tmp1, d_acc1, d_shifts, batch))) return rc;       // d1 = (X^a - 1) * acc1
    if ((rc = fhe_ct_relinearize(h, rows_c0, d_acc0, d_acc1, d_tmp0, batch))) return rc;      // acc += sum D(d0) * rows_c0
    return fhe_ct_relinearize(h, rows_c1, d_acc0, d_acc1, d_tmp1, batch);                     // acc += sum D(d1) * rows_c1
}
// One step as ONE launch (word-sized classes with packed rows): (out0, out1) = (in0, in1) + ExtProd((X^a - 1) * in, RGSW).
// rot0, rot1: (X^a - 1) * (in0, in1), pre-rotated by the loop (compact), or nullptr
static int blind_rotate_step_fused(fhe_rns_ntt_t *h, const LdsPlan &P, const fhe_relin_keys_t *r0, const fhe_relin_keys_t *r1, void *out0, void *out1,
                                   const void *in0, const void *in1, const uint32_t *d_shifts, uint32_t batch, bool in_compact, bool out_compact,
                                   const void *rot0, const void *rot1) {
    fhe_dev::LdsArgs A = lds_args(h, fhe_dev::LDS_EXTPROD, P, batch * h->L);
    A.r0 = out0; A.r1 = out1; A.a0 = in0; A.a1 = in1; A.rot0 = rot0; A.rot1 = rot1;
    A.kb = r0->d_pkb; A.ka = r0->d_pka; A.kb1 = r1->d_pkb; A.ka1 = r1->d_pka; A.K = r0->K; A.w = r0->decomp_bits; A.shifts = d_shifts;
    A.in_compact = in_compact; A.out_compact = out_compact;
    return lds_launch(h, A, "ntt_extprod_kernel");
}
static int check_rows(const fhe_rns_ntt_t *h, const fhe_relin_keys_t *r0, const fhe_relin_keys_t *r1) {
    if (!r0 || !r1) return fail(FHE_ERR_INVALID_ARG, "blind_rotate: null RGSW rows");
    if (r0->owner != h || r1->owner != h) return fail(FHE_ERR_INVALID_ARG, "blind_rotate: rows were imported for a different engine");
    if (r0->decomp_bits != r1->decomp_bits || r0->K != r1->K) return fail(FHE_ERR_INVALID_ARG, "blind_rotate: the two row sets use different digit widths");
    return FHE_OK;
}
static bool blind_rotate_fused(const fhe_rns_ntt *h, bool packed) { return packed && h->width != FHE_WIDTH_256 && !h->env.no_fused_blind_rotate; }
WsNeed need_blind_rotate(const fhe_rns_ntt *h, uint32_t batch, uint32_t K, bool packed) {   // fused loop: the plan's; else every step is two stand-alone key switches
    return blind_rotate_fused(h, packed) ? plan_extprod(h, (size_t)batch * h->L, K).need() : need_relinearize(h, batch, K, packed, KS_C2);
}
extern "C" int fhe_blind_rotate(fhe_rns_ntt_t *h, const fhe_relin_keys_t *const *rows_c0, const fhe_relin_keys_t *const *rows_c1, uint32_t steps,
                                void *d_acc0, void *d_acc1, const uint32_t *d_shifts, void *d_tmp0, void *d_tmp1, uint32_t batch) {
    int rc = check_call(h, batch, "blind_rotate"); if (rc) return rc;
    if (!d_acc0 || !d_acc1 || !d_tmp0 || !d_tmp1 || !d_shifts || (steps && (!rows_c0 || !rows_c1))) return fail(FHE_ERR_INVALID_ARG, "blind_rotate: null argument");
    if ((rc = check_aligned({d_acc0, d_acc1, d_tmp0, d_tmp1}, "blind_rotate"))) return rc;
    {   // the four buffers must be pairwise distinct
        const void *bufs[4] = {d_acc0, d_acc1, d_tmp0, d_tmp1};
        for (int x = 0; x < 4; x++) for (int y = x + 1; y < 4; y++)
            if (bufs[x] == bufs[y]) return fail(FHE_ERR_INVALID_ARG, "blind_rotate: accumulators and scratch must be distinct buffers");
    }
    if ((rc = check_inputs(h, {d_acc0, d_acc1}, batch))) return rc;
    bool packed = true; uint32_t kmax = 0;
    for (uint32_t s = 0; s < steps; s++) {
        if ((rc = check_rows(h, rows_c0[s], rows_c1[s]))) return rc;
        packed = packed && rows_c0[s]->d_pkb && rows_c1[s]->d_pkb;
        kmax = rows_c0[s]->K > kmax ? rows_c0[s]->K : kmax;
    }
    if (!blind_rotate_fused(h, packed)) {
        for (uint32_t s = 0; s < steps; s++)
            if ((rc = blind_rotate_step_general(h, rows_c0[s], rows_c1[s], d_acc0, d_acc1, d_shifts + (size_t)s * batch, d_tmp0, d_tmp1, batch))) return rc;
        return FHE_OK;
    }
    if (!steps) return FHE_OK;
    const LdsPlan P = plan_extprod(h, batch * h->L, kmax);
    if ((rc = ensure_need(h, P.need()))) return rc;
    if (P.compact) {
        // The accumulator pair is compacted first (one streaming pass), every step reads compact input from a workspace ping-pong (4 compact
        // polynomials; 2 more hold the pre-rotated pair of the current step), all but the last write compact output, the last one writes the
        // caller's containers.  The caller's scratch pair is not touched.
        const size_t cbytes = (size_t)batch * h->L * h->n * residue_bytes(h), count = (size_t)batch * h->L * h->n;
        char *w0 = (char *)h->ws[WS2].p;
        char *pp[2][2] = {{w0, w0 + cbytes}, {w0 + 2 * cbytes, w0 + 3 * cbytes}};
        char *rot0 = w0 + 4 * cbytes, *rot1 = w0 + 5 * cbytes;       // (X^a - 1) * acc of the current step
        if ((rc = compact_poly(h, pp[1][0], d_acc0, count))) return rc;
        if ((rc = compact_poly(h, pp[1][1], d_acc1, count))) return rc;
        for (uint32_t s = 0; s < steps; s++) {
            const bool last = s + 1 == steps;
            const void *i0 = pp[(s + 1) & 1][0], *i1 = pp[(s + 1) & 1][1];
            void *o0 = last ? d_acc0 : pp[s & 1][0], *o1 = last ? d_acc1 : pp[s & 1][1];
            const uint32_t *sh = d_shifts + (size_t)s * batch;
            if (P.prerot && ((rc = monomial_compact(h, rot0, i0, sh, count)) || (rc = monomial_compact(h, rot1, i1, sh, count)))) return rc;
            if ((rc = blind_rotate_step_fused(h, P, rows_c0[s], rows_c1[s], o0, o1, i0, i1, sh, batch, true, !last, P.prerot ? rot0 : nullptr,
                                              P.prerot ? rot1 : nullptr))) return rc;
        }
        return FHE_OK;
    }
    // ping-pong between (acc0, acc1) and (tmp0, tmp1): one launch per step, 4*S bytes of HBM traffic per accumulator and step
    void *cur0 = d_acc0, *cur1 = d_acc1, *nxt0 = d_tmp0, *nxt1 = d_tmp1;
    for (uint32_t s = 0; s < steps; s++) {
        if ((rc = blind_rotate_step_fused(h, P, rows_c0[s], rows_c1[s], nxt0, nxt1, cur0, cur1, d_shifts + (size_t)s * batch, batch, false, false, nullptr, nullptr))) return rc;
        std::swap(cur0, nxt0); std::swap(cur1, nxt1);
    }
    if (cur0 != d_acc0) {   // odd number of steps: the result sits in the scratch pair
        const size_t bytes = (size_t)batch * h->L * h->n * 32;
        HIP_TRY(hipMemcpyAsync(d_acc0, cur0, bytes, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(d_acc1, cur1, bytes, hipMemcpyDeviceToDevice, h->stream));
    }
    return FHE_OK;
}
extern "C" int fhe_blind_rotate_step(fhe_rns_ntt_t *h, const fhe_relin_keys_t *rows_c0, const fhe_relin_keys_t *rows_c1, void *d_acc0, void *d_acc1,
                                     const uint32_t *d_shifts, void *d_tmp0, void *d_tmp1, uint32_t batch) {
    return fhe_blind_rotate(h, &rows_c0, &rows_c1, 1, d_acc0, d_acc1, d_shifts, d_tmp0, d_tmp1, batch);
}
