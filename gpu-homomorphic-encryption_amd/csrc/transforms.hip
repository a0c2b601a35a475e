// transforms.hip -- launchers of the full-width and the LDS-resident kernels, the planners, and the transform / element-wise / multiply /
// tensor-product entry points.
#include "engine.h"

#include "ntt256_transforms.hip.h"
#include "ntt_wide.hip.h"
#include "ntt_word.hip.h"

// ---- full-width launchers (kernels: ntt_wide.hip.h; container-level element-wise ops: ntt256_transforms.hip.h) ---------------------------------
// One radix-2^R (R = 1 .. 3) global-memory pass over `polys` polynomials (src -> dst).  forward: stages s0 .. s0+R-1; inverse: index bits s0 .. s0+R-1.
template <int NL, bool FWD>
static void wide_pass(fhe_rns_ntt *h, fhe_dev::u256 *dst, const fhe_dev::u256 *src, uint32_t polys, uint32_t s0, uint32_t R, uint32_t scale) {
    const uint32_t chunk_max = (65535u / h->L) * h->L;      // grid.y limit; chunks keep the limb phase (polynomial index mod L)
    decltype(&fhe_dev::wide_pass_kernel<NL, 3, FWD>) const kernels[3] = {fhe_dev::wide_pass_kernel<NL, 3, FWD>, fhe_dev::wide_pass_kernel<NL, 2, FWD>, fhe_dev::wide_pass_kernel<NL, 1, FWD>};
    for (uint32_t done = 0; done < polys;) {
        const uint32_t chunk = polys - done < chunk_max ? polys - done : chunk_max;
        const size_t o = (size_t)done * h->n;
        hipLaunchKernelGGL(kernels[3 - R], dim3(((h->n >> R) + 255) / 256, chunk), dim3(256), 0, h->stream, dst + o, src + o, (const fhe_dev::WLimb<NL> *)h->d_wlimbs, h->L, h->log_n, s0, scale);
        done += chunk;
    }
}
template <int NL, int MODE>
static void wide_tile(fhe_rns_ntt *h, fhe_dev::u256 *dst, const fhe_dev::u256 *src, const fhe_dev::u256 *src2, uint32_t polys, uint32_t scale) {
    const uint32_t tiles_log = h->log_n - fhe_dev::WT_LOG;
    const uint32_t chunk_max = (0x7fffffffu >> tiles_log) / h->L * h->L;
    const auto kernel = h->wide_lazy ? fhe_dev::wide_tile_kernel<NL, MODE, true> : fhe_dev::wide_tile_kernel<NL, MODE, false>;
    for (uint32_t done = 0; done < polys;) {
        const uint32_t chunk = polys - done < chunk_max ? polys - done : chunk_max;
        const size_t o = (size_t)done * h->n;
        hipLaunchKernelGGL(kernel, dim3(chunk << tiles_log), dim3(fhe_dev::WT_T), 0, h->stream, dst + o, src + o, src2 ? src2 + o : nullptr,
                           (const fhe_dev::WLimb<NL> *)h->d_wlimbs, h->L, h->log_n, scale);
        done += chunk;
    }
}
// Number of leading (forward) / trailing (inverse) stages that run as global passes: everything above the 2^11-coefficient LDS tile.
static uint32_t wide_top_stages(const fhe_rns_ntt *h) {
    return (!h->env.no_wide_tiles && h->log_n >= (uint32_t)fhe_dev::WT_LOG) ? h->log_n - fhe_dev::WT_LOG : h->log_n;
}
// The top stages of a forward transform, src -> dst (src == dst allowed): R <= 3 stages per launch.
template <int NL>
static void wide_forward_top(fhe_rns_ntt *h, fhe_dev::u256 *dst, const fhe_dev::u256 *src, uint32_t polys) {
    const uint32_t top = wide_top_stages(h);
    for (uint32_t s = 0; s < top;) {
        const uint32_t R = top - s >= 3 ? 3 : top - s;
        wide_pass<NL, true>(h, dst, s ? dst : src, polys, s, R, 0);
        s += R;
    }
}
// The trailing stages of an inverse transform, in place on data, with the final scaling (1: n^-1, 2: n^-1 R for the fused products).
template <int NL>
static void wide_inverse_top(fhe_rns_ntt *h, fhe_dev::u256 *data, uint32_t polys, uint32_t scale) {
    const uint32_t top = wide_top_stages(h), b_first = h->log_n - top;
    if (!h->log_n && scale) {                               // degree-1 engine: no butterflies, only the scaling (n^-1 = 1)
        const size_t count = (size_t)polys;
        hipLaunchKernelGGL((fhe_dev::wide_scale_kernel<NL>), dim3(ew_grid(count)), dim3(256), 0, h->stream, data, data,
                           (const fhe_dev::WLimb<NL> *)h->d_wlimbs, h->L, 0u, scale, count);
    }
    for (uint32_t s = 0; s < top;) {
        const uint32_t R = top - s >= 3 ? 3 : top - s;
        wide_pass<NL, false>(h, data, data, polys, b_first + s, R, s + R == top ? scale : 0);
        s += R;
    }
}
template <int NL>
static int wide_transform_t(fhe_rns_ntt *h, fhe_dev::u256 *dst, const fhe_dev::u256 *src, uint32_t polys, bool forward, uint32_t scale) {
    const uint32_t top = wide_top_stages(h);
    const bool tiled = top < h->log_n;
    if (!h->log_n) {                                        // degree 1: the transforms are the identity (stand-alone inverse: n^-1 = 1)
        if (dst != src) HIP_TRY(hipMemcpyAsync(dst, src, (size_t)polys * 32, hipMemcpyDeviceToDevice, h->stream));
        if (!forward && scale == 2) wide_inverse_top<NL>(h, dst, polys, 2);
        return post_launch(h->stream, "wide identity");
    }
    if (forward) {
        wide_forward_top<NL>(h, dst, src, polys);
        if (tiled) wide_tile<NL, fhe_dev::TILE_FWD>(h, dst, top ? dst : src, nullptr, polys, 0);
    } else {
        if (tiled) wide_tile<NL, fhe_dev::TILE_INV>(h, dst, src, nullptr, polys, top ? 0 : scale);
        else if (dst != src) HIP_TRY(hipMemcpyAsync(dst, src, (size_t)polys * h->n * 32, hipMemcpyDeviceToDevice, h->stream));
        wide_inverse_top<NL>(h, dst, polys, scale);
    }
    return post_launch(h->stream, forward ? "wide forward" : "wide inverse");
}
// src -> dst (in place when equal); inverse: scale 1 = n^-1 (stand-alone), 2 = n^-1 R (inputs carry the R^-1 of a fused pointwise product)
static int run256_transform(fhe_rns_ntt *h, fhe_dev::u256 *dst, const fhe_dev::u256 *src, uint32_t polys, bool forward, uint32_t scale = 1) {
    return h->wide_nl == 2 ? wide_transform_t<2>(h, dst, src, polys, forward, scale) : wide_transform_t<4>(h, dst, src, polys, forward, scale);
}
static int run256_transform(fhe_rns_ntt *h, fhe_dev::u256 *data, uint32_t polys, bool forward) { return run256_transform(h, data, data, polys, forward, 1); }

template <int OP>
static int run256_ew(fhe_rns_ntt *h, void *r, const void *a, const void *b, uint32_t polys, const char *what) {
    size_t count = (size_t)polys * h->n;
    hipLaunchKernelGGL(fhe_dev::ew256_rns_kernel<OP>, dim3(ew_grid(count)), dim3(256), 0, h->stream, (fhe_dev::u256 *)r,
                       (const fhe_dev::u256 *)a, (const fhe_dev::u256 *)b, (const fhe_dev::Limb256 *)h->d_limbs, h->L, h->log_n, count);
    return post_launch(h->stream, what);
}

// ---- LDS-resident path launchers (kernels live in lds_inst.hip, one object per (field, log2 n)) ---------
// Two-pass transforms of the word-sized classes (log2 n = 13 + sub_top): one launch of the LOGN = 13 instance per pass.  Between the
// two launches the polynomials are COMPACT (sizeof(residue) bytes per coefficient, WS3); *_compact tell which pointers are.
int lds_launch(fhe_rns_ntt *h, const fhe_dev::LdsArgs &A, const char *what, int log_n) {
    if (!log_n) log_n = (int)h->log_n;
    fhe_dev::lds_launch_fn fn = fhe_dev::lds_lookup(lds_width_id(h), log_n);
    if (!fn) return fail(FHE_ERR_UNSUPPORTED, "transform size outside the LDS-resident range");
    if (!fn(A)) {
        char buf[256];
        snprintf(buf, sizeof buf, "no LDS kernel for the %s in the %s form (%s inputs, %s outputs) at width %d, log2 N = %d", fhe_dev::lds_op_name(A.op), fhe_dev::lds_form_name(A.form),
                 A.in_compact ? "compact" : "container", A.out_compact ? "compact" : "container", lds_width_id(h), log_n);
        return fail(FHE_ERR_UNSUPPORTED, buf);
    }
    return post_launch(A.stream, what);
}
static int lds_big(fhe_rns_ntt *h, int op, void *dst, bool dst_compact, const void *src, bool src_compact, const void *src2, uint32_t polys, bool rconst,
                   const char *what) {
    const uint32_t chunk_max = (65535u / h->L) * h->L;      // grid.y of the pass kernel; chunks keep the limb phase
    const size_t dstep = (size_t)h->n * (dst_compact ? residue_bytes(h) : 32), sstep = (size_t)h->n * (src_compact ? residue_bytes(h) : 32);
    for (uint32_t done = 0; done < polys;) {
        const uint32_t chunk = polys - done < chunk_max ? polys - done : chunk_max;
        fhe_dev::LdsArgs A = lds_args(h, op, {}, chunk);
        A.r0 = (char *)dst + done * dstep; A.a0 = (const char *)src + done * sstep; A.b0 = src2 ? (const char *)src2 + done * sstep : nullptr;
        A.in_compact = src_compact; A.out_compact = dst_compact; A.top = h->sub_top; A.rconst = rconst;
        int rc = lds_launch(h, A, what, 13); if (rc) return rc;
        done += chunk;
    }
    return FHE_OK;
}
// forward / inverse: at the two-pass sizes the compact polynomials between the two launches
WsNeed need_transform(const fhe_rns_ntt *h, size_t polys) { return {0, 0, h->sub_top ? polys * h->n * residue_bytes(h) : 0}; }
static int big_forward(fhe_rns_ntt *h, void *dst, const void *src, uint32_t polys) {
    int rc = ensure_need(h, need_transform(h, polys)); if (rc) return rc;
    if ((rc = lds_big(h, fhe_dev::LDS_PASS_FWD, h->ws[WS3].p, true, src, false, nullptr, polys, false, "word_pass_kernel"))) return rc;
    return lds_big(h, fhe_dev::LDS_SUB_FORWARD, dst, false, h->ws[WS3].p, true, nullptr, polys, false, "ntt_sub_kernel");
}
static int big_inverse(fhe_rns_ntt *h, void *data, uint32_t polys) {
    int rc = ensure_need(h, need_transform(h, polys)); if (rc) return rc;
    if ((rc = lds_big(h, fhe_dev::LDS_SUB_INVERSE, h->ws[WS3].p, true, data, false, nullptr, polys, false, "ntt_sub_kernel"))) return rc;
    return lds_big(h, fhe_dev::LDS_PASS_INV, data, false, h->ws[WS3].p, true, nullptr, polys, false, "word_pass_kernel");
}

// ---- kernel forms of the LDS-resident ops (LdsPlan: engine.h) ---------------------------------------------------------------
// r = a * b of `polys` limb polynomials; same_operands: b == a (not broadcast)
LdsPlan plan_multiply(const fhe_rns_ntt *h, size_t polys, bool same_operands) {
    const int eb = (int)residue_bytes(h), ln = (int)h->log_n;
    // a handful of polynomials: four workgroups each (in place is fine: every operand container is read by the first launch, the result containers
    // are written by the third)
    if (polys <= h->env.coop_polys && fhe_dev::lds_coop4_multiply(eb, ln)) return {fhe_dev::LDS_COOP4, 3, 3 * polys * h->n * 4};
    if (polys <= h->env.small_batch_polys && fhe_dev::lds_small_multiply(eb, ln)) return {fhe_dev::LDS_SMALL16};   // few: one workgroup's latency is what counts
    return {same_operands && !h->env.no_square ? fhe_dev::LDS_SQUARE : fhe_dev::LDS_ONE_LAUNCH};
}
// Tensor product of `polys` limb polynomials per component; compact_out: c0, c1, c2 as compact polynomials (the fused multiply + relinearise);
// alone: no other chunk of the call runs beside it.
// Two launches (ntt_forward_compact_kernel + ntt_ct_a_kernel, workspace for the transformed b-side) instead of the one-launch kernel: always
// where that kernel does not exist (8-byte residues at N = 2^14, N = 2^15), and for the 8-byte residues where the interleaved A/B favoured it
// (scripts/ab_ct_form.sh, one MI355X, batch 1024, N = 8192 / 4096 / 2048): the FP64 field (tensor product +32 / +35 / +26 %, full multiply
// +11 / +10 / +2 %) and the stand-alone tensor product of the full-range 64-bit field (+13 / +11 / +12 %; inside the full multiply
// 0 / -9 / -2 %); the lazy 64-bit field keeps its one-launch kernel (-1 / +6 / -4 %).  The squaring forms stay on the one-launch kernel
// (5 transforms).  FHE_HIP_CT_FORM=one|two forces a form where both exist.
LdsPlan plan_ct_multiply(const fhe_rns_ntt *h, size_t polys, bool same_operands, bool compact_out, bool alone) {
    const int eb = (int)residue_bytes(h), ln = (int)h->log_n;
    const bool square = same_operands && !compact_out && !h->env.no_square;
    bool two = !h->env.no_two_launch_ct && fhe_dev::lds_ct_two_launch(eb, ln);
    if (two && fhe_dev::lds_ct_fused(eb, ln)) {
        bool want = h->width == FHE_WIDTH_52 || (h->width == FHE_WIDTH_64X && !compact_out);
        if (h->env.ct_form_force) want = h->env.ct_form_force == 2;       // FHE_HIP_CT_FORM=one|two (A/B, cross-check)
        two = want && !square;
    }
    if (two) return {fhe_dev::LDS_TWO_LAUNCH, 1, 2 * polys * h->n * eb};
    if (compact_out && alone && polys <= h->env.coop_polys && fhe_dev::lds_coop4_multiply(eb, ln))     // a handful of ciphertexts: four workgroups per limb polynomial
        return {fhe_dev::LDS_COOP4, 3, 7 * polys * h->n * 4};
    if (compact_out && polys <= h->env.split_pairs_polys && fhe_dev::lds_small_multiply(eb, ln))      // few ciphertexts: the 16-per-thread tensor product (and the split key switch)
        return {fhe_dev::LDS_SMALL16};
    if (fhe_dev::lds_ct_fused(eb, ln)) return {square ? fhe_dev::LDS_SQUARE : fhe_dev::LDS_ONE_LAUNCH};
    return {fhe_dev::LDS_THREE_LAUNCH};
}
// Key switch / external product of the 8-byte residues (and of the 4-byte residues at N = 2^15): ONE workgroup per (ciphertext, limb)
// with three live arrays (ntt_keyswitch3_kernel / ntt_extprod3_kernel) instead of the split form -- everywhere it was faster in the
// interleaved A/B (scripts/ab_keyswitch3.sh, ab_extprod3.sh, ab_joint3_small.sh; with the descriptor loads of round 2): every size for
// the lazy 64-bit field (+4...+60 %) and for the FP64 field's external product and compact-operand key switch (+10...+46 %); the FP64
// field's stand-alone key switch (container operands) from N = 2^13 (3-6 % behind at N <= 4096); the full-range 64-bit field from
// N = 2^12 (at N = 2048: key switch -3 %, external product -16 %).  Never under FHE_HIP_SPLIT_KEYSWITCH=1 (a testing aid).
static bool use_joint3(const fhe_rns_ntt *h, bool extprod, bool compact) {
    if (h->env.split_keyswitch || !fhe_dev::lds_keyswitch_joint3((int)residue_bytes(h), (int)h->log_n)) return false;
    if (h->width == FHE_WIDTH_52) return extprod || compact || h->log_n >= 13;
    if (h->width == FHE_WIDTH_64X) return h->log_n >= 12;
    return true;
}
// The fused FHEContext::multiply (tensor product with compact outputs straight into the key switch) on every LDS-resident size with packed keys
bool plan_fused_ct_relin(const fhe_rns_ntt *h, bool packed_keys) {
    return packed_keys && h->width != FHE_WIDTH_256 && !h->sub_top && !h->env.single_transforms && !h->env.no_fused_ct_relin;
}
// Hoisted rotations as the two LDS ops of hoist.hip.h: where the fused multiply + relinearise runs and the instance has the kernels
bool plan_fused_hoist(const fhe_rns_ntt *h, bool packed_keys) {
    return plan_fused_ct_relin(h, packed_keys) && fhe_dev::lds_hoist((int)residue_bytes(h), (int)h->log_n) && !h->env.no_fused_hoist;
}
bool plan_fused_lincomb(const fhe_rns_ntt *h, bool packed_keys) {
    return plan_fused_hoist(h, packed_keys) && fhe_dev::lds_hoist_lincomb((int)residue_bytes(h), (int)h->log_n);
}
// Public-key encryption as the one launch of encrypt.hip.h: every LDS-resident word-sized size whose instance has the kernel
bool plan_fused_encrypt(const fhe_rns_ntt *h) {
    return h->width != FHE_WIDTH_256 && !h->sub_top && h->log_n >= 11 && fhe_dev::lds_encrypt((int)residue_bytes(h), (int)h->log_n) && !h->env.no_fused_encrypt;
}
// Secret-key decryption as the two launches of decrypt.hip.h: every LDS-resident word-sized size whose instance has the kernel
bool plan_fused_decrypt(const fhe_rns_ntt *h) {
    return h->width != FHE_WIDTH_256 && !h->sub_top && h->log_n >= 11 && fhe_dev::lds_decrypt((int)residue_bytes(h), (int)h->log_n) && !h->env.no_fused_decrypt;
}
// Key-switching key generation as the one launch of keygen.hip.h: every LDS-resident word-sized size whose instance has the kernel, for key
// sets that get packed tables (the kernel writes nothing else)
bool plan_fused_keygen(const fhe_rns_ntt *h, bool packed_keys) {
    return packed_keys && h->width != FHE_WIDTH_256 && !h->sub_top && h->log_n >= 11 && fhe_dev::lds_keygen((int)residue_bytes(h), (int)h->log_n) && !h->env.no_fused_keygen;
}
// The batch encoder as one launch of encode.hip.h: te is the encoder's one-limb engine on (n, t), whose field the kernels run on
bool plan_fused_slots(const fhe_rns_ntt *te) {
    return te->width != FHE_WIDTH_256 && !te->sub_top && te->log_n >= 11 && fhe_dev::lds_slots((int)residue_bytes(te), (int)te->log_n) && !te->env.no_fused_encode;
}
// ... one workgroup per ciphertext (draws once, loops over the limbs) from FHE_HIP_ENCRYPT_PER_CT_BATCH ciphertexts, below that one per
// (ciphertext, limb): L times the workgroups for a device that the ciphertexts alone do not fill.  Same kernel, same bits.
bool plan_encrypt_per_ct(const fhe_rns_ntt *h, uint32_t batch) { return h->L > 1 && batch >= h->env.encrypt_per_ct_batch; }
// Key switch of `polys` limb polynomials with K digits (KsSource: engine.h).  alone: no other chunk of the call runs beside it (the
// few-ciphertext parts take WS1).
LdsPlan plan_keyswitch(const fhe_rns_ntt *h, size_t polys, uint32_t K, KsSource src, bool alone) {
    const int eb = (int)residue_bytes(h), ln = (int)h->log_n;
    const bool joint3 = use_joint3(h, false, src == KS_FUSED);
    const bool paired32 = h->width == FHE_WIDTH_32 && !h->env.single_transforms && fhe_dev::lds_paired_keyswitch(4, ln);
    LdsPlan p{fhe_dev::LDS_ONE_LAUNCH};
    // Every limb workgroup re-reads all of c2 (the three-array kernels once per DIGIT): compact it once (a streaming pass: S read, S/4 or S/8
    // written) so that those re-reads move compact polynomials instead of 32-byte containers -- round 2 counters at N = 2^14, 6 x 40-bit:
    // 2.6 x the algorithmic bytes; on the 4-byte residues the container loads kept the address FIFO full 12 % of the time (round 3 SQ counters).
    p.compact = src == KS_FUSED || (src == KS_C2 && ((joint3 && h->width != FHE_WIDTH_32) || paired32) && !h->env.no_c2_compaction);
    // Few ciphertexts on the paired key-switch kernel: one workgroup per digit pair and a combining launch (ntt_lds_small.hip.h); partial
    // accumulators: one pair per digit PAIR, or (N <= 2^13: the 16-per-thread form, one workgroup per digit) one pair per digit
    const uint32_t NP = (h->L * K + 1) / 2;
    if (alone && paired32 && NP >= 2 && polys <= h->env.split_pairs_polys) {
        const bool d16 = fhe_dev::lds_small_multiply(4, ln);
        p.form = d16 ? fhe_dev::LDS_PARTS16 : fhe_dev::LDS_PART_PAIRS;
        p.ws = 1; p.bytes = 2 * polys * (d16 ? h->L * K : NP) * h->n * 4;
    } else if (fhe_dev::lds_keyswitch_split(eb, ln)) {
        p.form = joint3 ? fhe_dev::LDS_JOINT3 : fhe_dev::LDS_SPLIT;
    } else if (fhe_dev::lds_paired_keyswitch(eb, ln) && !h->env.single_transforms) {
        p.form = fhe_dev::LDS_PAIRED;
    } else {
        p.form = fhe_dev::lds_twiddles_in_lds(eb, ln) && !h->env.global_twiddles ? fhe_dev::LDS_SINGLE_LDS_TW : fhe_dev::LDS_SINGLE_L2_TW;
    }
    p.add_compact = src == KS_FUSED;
    if (p.compact) p.ws2 = (src == KS_FUSED ? 3 : 1) * polys * h->n * eb;   // c0, c1, c2 of the fused tensor product (rotation: sigma(c0), sigma(c1), 0) / the compacted c2
    return p;
}
// External product of a blind-rotation loop over `polys` limb polynomials per accumulator component, K digits (the largest of the loop's rows).
LdsPlan plan_extprod(const fhe_rns_ntt *h, size_t polys, uint32_t K) {
    const int eb = (int)residue_bytes(h), ln = (int)h->log_n;
    const bool w32 = h->width == FHE_WIDTH_32 && !h->env.single_transforms && !h->env.no_compact_blind_rotate;
    LdsPlan p{fhe_dev::LDS_ONE_LAUNCH};
    // Few accumulators (4-byte residues, N <= 2^13; what a bootstrapping of one or a few ciphertexts looks like): with one workgroup per (accumulator, limb)
    // a step lasts as long as that workgroup's 2 L K / 2 paired transforms back to back (103 us per external product at N = 8192, L = 4, w = 16, batch 1).
    // Here a step is three launches: the monomial factor (X^a - 1) once per step (a streaming pass), one workgroup per (accumulator, limb, component, DIGIT) on the
    // 16-per-thread forward transform with that digit's two key products, and one workgroup per (accumulator, limb, output component) that sums the 2 L K partials,
    // runs one inverse transform and adds the accumulator (ntt_keyswitch16_{part,comb}_kernel); two partial accumulators per (limb polynomial, component, digit).
    // (N = 2^14: the same three launches on the paired 32-per-thread transforms, one workgroup per digit PAIR of a component)
    if (w32 && !h->env.no_prerotation && fhe_dev::lds_paired_keyswitch(4, ln) && polys <= h->env.split_pairs_polys) {
        const bool d16 = fhe_dev::lds_small_multiply(4, ln);
        p.form = d16 ? fhe_dev::LDS_PARTS16 : fhe_dev::LDS_PART_PAIRS;
        p.ws = 1; p.bytes = 2 * polys * h->n * (d16 ? 2 * (size_t)h->L * K : 2 * (((size_t)h->L * K + 1) / 2)) * 4;
        p.compact = p.prerot = true;
    // Paired kernel (4-byte residues up to N = 2^14): the accumulator pair lives in COMPACT form for the whole loop: the L limb workgroups of an
    // accumulator each read all of it, which in container form is 3x the algorithmic traffic (profiles/r02_blindrotate_*) and made the first step
    // of a loop 40 % slower than the others (1114 vs 785 us at N = 16384 x 6, profiles/r03_blindrotate_n16384_summary.txt).
    } else if (w32 && fhe_dev::lds_paired_extprod(4, ln)) {
        p.form = fhe_dev::LDS_PAIRED; p.compact = true;
    // Three-array kernel (8-byte residues; 4-byte residues at N = 2^15): every limb workgroup re-reads each limb of the accumulator pair once per
    // DIGIT (rotated), L * K * 2 reads per workgroup -- as containers that was several times the algorithmic traffic: compact pair, and the
    // monomial factor once per step (a streaming pass over two compact polynomials) instead of once per digit inside the kernel.
    } else if (use_joint3(h, true, false) && !h->env.no_compact_blind_rotate) {
        p.form = fhe_dev::LDS_JOINT3; p.compact = true; p.prerot = !h->env.no_prerotation;
    // container accumulators
    } else if (fhe_dev::lds_keyswitch_split(eb, ln)) {
        p.form = use_joint3(h, true, false) ? fhe_dev::LDS_JOINT3 : fhe_dev::LDS_SPLIT;
    } else if (fhe_dev::lds_paired_extprod(eb, ln) && !h->env.single_transforms) {
        p.form = fhe_dev::LDS_PAIRED;
    } else {
        p.form = fhe_dev::lds_twiddles_in_lds(eb, ln) && !h->env.global_twiddles ? fhe_dev::LDS_SINGLE_LDS_TW : fhe_dev::LDS_SINGLE_L2_TW;
    }
    if (p.compact) p.ws2 = (p.prerot ? 6 : 4) * polys * h->n * eb;   // the ping-pong of compact accumulator pairs, and the pre-rotated pair of the current step
    return p;
}

// r = a * b on the LDS-resident sizes (the caller has ensured need_multiply); b_polys: polynomials behind b (0 = as many as the batch, L = one RNS polynomial broadcast over the batch)
static int lds_multiply(fhe_rns_ntt *h, void *r, const void *a, const void *b, uint32_t polys, uint32_t b_polys) {
    fhe_dev::LdsArgs A = lds_args(h, fhe_dev::LDS_MULTIPLY, plan_multiply(h, polys, a == b && !b_polys), polys);
    A.r0 = r; A.a0 = a; A.b0 = b; A.b_polys = b_polys;
    return lds_launch(h, A, "ntt_multiply_kernel");
}
template <class F, int OP>
static int lds_ew(fhe_rns_ntt *h, void *r, const void *a, const void *b, uint32_t polys, const char *what) {
    using V = typename F::V16;
    size_t halves = (size_t)polys * h->n * 2;
    hipLaunchKernelGGL((fhe_dev::ew_kernel<F, OP>), dim3(ew_grid(halves)), dim3(256), 0, h->stream, (V *)r, (const V *)a,
                       (const V *)b, (const fhe_dev::Limb<F> *)h->d_limbs, h->L, h->log_n, halves);
    return post_launch(h->stream, what);
}
template <class F>
static int lds_check(fhe_rns_ntt *h, const void *d, uint32_t polys) {
    using V = typename F::V16;
    size_t halves = (size_t)polys * h->n * 2;
    hipLaunchKernelGGL((fhe_dev::check_kernel<F>), dim3(ew_grid(halves)), dim3(256), 0, h->stream, (const V *)d,
                       (const fhe_dev::Limb<F> *)h->d_limbs, h->L, h->log_n, halves, h->d_flag);
    return post_launch(h->stream, "check_kernel");
}

int compact_poly(fhe_rns_ntt *h, void *out, const void *in, size_t containers) {
    return with_word_field(h, [&](auto f) {
        using F = decltype(f);
        hipLaunchKernelGGL((fhe_dev::compact_kernel<F>), dim3(ew_grid(containers)), dim3(256), 0, h->stream, (typename F::E *)out, (const typename F::V16 *)in, containers);
        return post_launch(h->stream, "compact_kernel");
    });
}


static int do_transform(fhe_rns_ntt *h, void *d_data, uint32_t batch, bool fwd) {
    const uint32_t polys = batch * h->L;
    if (h->sub_top) return fwd ? big_forward(h, d_data, d_data, polys) : big_inverse(h, d_data, polys);
    if (h->width == FHE_WIDTH_256) return run256_transform(h, (fhe_dev::u256 *)d_data, polys, fwd);
    fhe_dev::LdsArgs A = lds_args(h, fwd ? fhe_dev::LDS_FORWARD : fhe_dev::LDS_INVERSE, {}, polys); A.r0 = d_data;
    return lds_launch(h, A, fwd ? "ntt_forward_kernel" : "ntt_inverse_kernel");
}
int do_forward(fhe_rns_ntt *h, void *d_data, uint32_t batch) { return do_transform(h, d_data, batch, true); }
int do_inverse(fhe_rns_ntt *h, void *d_data, uint32_t batch) { return do_transform(h, d_data, batch, false); }
template <int OP>
int do_ew(fhe_rns_ntt *h, void *r, const void *a, const void *b, uint32_t batch, const char *what) {
    const uint32_t polys = batch * h->L;
    if (h->width == FHE_WIDTH_256) return run256_ew<OP>(h, r, a, b, polys, what);
    return with_word_field(h, [&](auto f) { return lds_ew<decltype(f), OP>(h, r, a, b, polys, what); });
}
template int do_ew<0>(fhe_rns_ntt *, void *, const void *, const void *, uint32_t, const char *);   // the other sources call these
template int do_ew<1>(fhe_rns_ntt *, void *, const void *, const void *, uint32_t, const char *);
template int do_ew<2>(fhe_rns_ntt *, void *, const void *, const void *, uint32_t, const char *);
// Full-width multiply without operand copies (the reference copies both operands first, src/ntt.cu:50-58): the top forward stages
// write the transformed operands into the workspace, one fused tile launch does the remaining forward stages of both operands, the
// pointwise product and the low inverse stages, the trailing inverse stages finish in place on the result.
template <int NL>
static int wide_multiply_t(fhe_rns_ntt *h, void *d_r, const void *d_a, const void *d_b, uint32_t polys) {
    using fhe_dev::u256;
    const uint32_t top = wide_top_stages(h);
    const bool tiled = top < h->log_n;
    const size_t bytes = (size_t)polys * h->n * 32;
    const u256 *A = (const u256 *)d_a, *B = (const u256 *)d_b;
    if (!h->log_n) return run256_ew<0>(h, d_r, d_a, d_b, polys, "pointwise");     // degree 1: the product in Z_q
    if (top) {
        u256 *wa = (u256 *)h->ws[WS1].p, *wb = (u256 *)((char *)h->ws[WS1].p + bytes);
        wide_forward_top<NL>(h, wa, A, polys);
        if (d_b != d_a) wide_forward_top<NL>(h, wb, B, polys);
        B = d_b != d_a ? wb : wa; A = wa;
    }
    if (tiled) {
        wide_tile<NL, fhe_dev::TILE_MUL>(h, (u256 *)d_r, A, B, polys, top ? 0 : 2);
    } else {                                                // n < 2^11 (or FHE_HIP_NO_WIDE_TILES): pointwise product of the transformed copies
        const size_t count = (size_t)polys * h->n;
        hipLaunchKernelGGL((fhe_dev::wide_pointwise_kernel<NL>), dim3(ew_grid(count)), dim3(256), 0, h->stream, (u256 *)d_r, A, B,
                           (const fhe_dev::WLimb<NL> *)h->d_wlimbs, h->L, h->log_n, count);
    }
    wide_inverse_top<NL>(h, (u256 *)d_r, polys, 2);
    return post_launch(h->stream, "wide multiply");
}
template <int NL>
static int wide_ct_multiply_t(fhe_rns_ntt *h, void *c0, void *c1, void *c2, const void *a0, const void *a1, const void *b0, const void *b1, uint32_t polys) {
    using fhe_dev::u256;
    // 4 forward transforms into the workspace (no copies), one pass for the three NTT-domain products, 3 inverse transforms
    const size_t bytes = (size_t)polys * h->n * 32;
    char *ws = (char *)h->ws[WS1].p;
    const void *src[4] = {a0, a1, b0, b1};
    int rc;
    for (int i = 0; i < 4; i++)
        if ((rc = run256_transform(h, (u256 *)(ws + i * bytes), (const u256 *)src[i], polys, true, 0))) return rc;
    const size_t count = (size_t)polys * h->n;
    hipLaunchKernelGGL((fhe_dev::wide_ct_pointwise_kernel<NL>), dim3(ew_grid(count)), dim3(256), 0, h->stream, (u256 *)c0, (u256 *)c1, (u256 *)c2,
                       (const u256 *)ws, (const u256 *)(ws + bytes), (const u256 *)(ws + 2 * bytes), (const u256 *)(ws + 3 * bytes),
                       (const fhe_dev::WLimb<NL> *)h->d_wlimbs, h->L, h->log_n, count);
    for (void *c : {c0, c1, c2})
        if ((rc = run256_transform(h, (u256 *)c, (const u256 *)c, polys, false, 2))) return rc;
    return FHE_OK;
}
WsNeed need_multiply(const fhe_rns_ntt *h, uint32_t batch) {   // (no form's workspace depends on b == a)
    const size_t polys = (size_t)batch * h->L;
    if (h->sub_top) return {0, 0, 2 * polys * h->n * residue_bytes(h)};              // two compact operands
    if (h->width != FHE_WIDTH_256) return plan_multiply(h, polys, false).need();
    return {h->log_n && wide_top_stages(h) ? 2 * polys * h->n * 32 : 0, 0, 0};       // full width: both operands after their top forward stages
}
WsNeed need_ct_multiply(const fhe_rns_ntt *h, uint32_t batch, bool same_operands) {
    const size_t polys = (size_t)batch * h->L;
    if (h->sub_top) return WsNeed{5 * polys * h->n * 32, 0, 0} | need_transform(h, polys);   // 4 transformed operands + one product as containers
    if (h->width != FHE_WIDTH_256) return plan_ct_multiply(h, polys, same_operands, false, true).need();
    return {4 * polys * h->n * 32, 0, 0};                                            // full width: 4 transformed operands
}
static int do_multiply(fhe_rns_ntt *h, void *d_r, const void *d_a, const void *d_b, uint32_t batch) {
    const uint32_t polys = batch * h->L;
    int rc = ensure_need(h, need_multiply(h, batch)); if (rc) return rc;
    // d_r may alias d_a and/or d_b, as in the reference (which copies its operands first, src/ntt.cu:50-58): every
    // workgroup loads both of its operand polynomials completely before its first store, and the general path works on copies.
    if (h->sub_top) {   // two-pass: the top stages of both operands go to the COMPACT workspace, one fused launch over the 2^13 blocks (compact in and out), last pass into the result
        const size_t cbytes = (size_t)polys * h->n * residue_bytes(h);
        char *wa = (char *)h->ws[WS3].p, *wb = d_b != d_a ? wa + cbytes : wa;
        if ((rc = lds_big(h, fhe_dev::LDS_PASS_FWD, wa, true, d_a, false, nullptr, polys, false, "word_pass_kernel"))) return rc;
        if (d_b != d_a && (rc = lds_big(h, fhe_dev::LDS_PASS_FWD, wb, true, d_b, false, nullptr, polys, false, "word_pass_kernel"))) return rc;
        if ((rc = lds_big(h, fhe_dev::LDS_SUB_MULTIPLY, wa, true, wa, true, wb, polys, false, "ntt_sub_kernel"))) return rc;
        return lds_big(h, fhe_dev::LDS_PASS_INV, d_r, false, wa, true, nullptr, polys, true, "word_pass_kernel");
    }
    if (h->width != FHE_WIDTH_256) return lds_multiply(h, d_r, d_a, d_b, polys, 0);
    return h->wide_nl == 2 ? wide_multiply_t<2>(h, d_r, d_a, d_b, polys) : wide_multiply_t<4>(h, d_r, d_a, d_b, polys);
}
int do_ct_multiply(fhe_rns_ntt *h, void *c0, void *c1, void *c2, const void *a0, const void *a1, const void *b0,
                          const void *b1, uint32_t batch) {
    const uint32_t polys = batch * h->L;
    int rc = ensure_need(h, need_ct_multiply(h, batch, a0 == b0 && a1 == b1)); if (rc) return rc;
    if (h->sub_top) {   // 4 forward transforms into the workspace, NTT-domain products on the field type, 3 inverse transforms
        const size_t bytes = (size_t)polys * h->n * 32;
        char *ws = (char *)h->ws[WS1].p, *T = ws + 4 * bytes;
        const void *src[4] = {a0, a1, b0, b1};
        for (int i = 0; i < 4; i++) if ((rc = big_forward(h, ws + i * bytes, src[i], polys))) return rc;
        if ((rc = do_ew<0>(h, c0, ws, ws + 2 * bytes, batch, "ct pointwise"))) return rc;
        if ((rc = do_ew<0>(h, c1, ws, ws + 3 * bytes, batch, "ct pointwise"))) return rc;
        if ((rc = do_ew<0>(h, T, ws + bytes, ws + 2 * bytes, batch, "ct pointwise"))) return rc;
        if ((rc = do_ew<1>(h, c1, c1, T, batch, "ct add"))) return rc;
        if ((rc = do_ew<0>(h, c2, ws + bytes, ws + 3 * bytes, batch, "ct pointwise"))) return rc;
        for (void *c : {c0, c1, c2}) if ((rc = big_inverse(h, c, polys))) return rc;
        return FHE_OK;
    }
    if (h->width != FHE_WIDTH_256) {
        fhe_dev::LdsArgs A = lds_args(h, fhe_dev::LDS_CT_MULTIPLY, plan_ct_multiply(h, polys, a0 == b0 && a1 == b1, false, true), polys);
        A.r0 = c0; A.r1 = c1; A.r2 = c2; A.a0 = a0; A.a1 = a1; A.b0 = b0; A.b1 = b1;
        return lds_launch(h, A, "ntt_ct_multiply_kernel");
    }
    return h->wide_nl == 2 ? wide_ct_multiply_t<2>(h, c0, c1, c2, a0, a1, b0, b1, polys) : wide_ct_multiply_t<4>(h, c0, c1, c2, a0, a1, b0, b1, polys);
}

static int transform_call(fhe_rns_ntt *h, void *d_data, uint32_t batch, bool fwd, const char *what) {
    int rc = check_call(h, batch, what); if (rc) return rc;
    if (!d_data) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": null data");
    if ((rc = check_aligned({d_data}, what))) return rc;
    if ((rc = check_inputs(h, {d_data}, batch))) return rc;
    return do_transform(h, d_data, batch, fwd);
}
extern "C" int fhe_rns_ntt_forward(fhe_rns_ntt_t *h, void *d_data, uint32_t batch) { return transform_call(h, d_data, batch, true, "forward"); }
extern "C" int fhe_rns_ntt_inverse(fhe_rns_ntt_t *h, void *d_data, uint32_t batch) { return transform_call(h, d_data, batch, false, "inverse"); }
template <int OP>
static int ew_call(fhe_rns_ntt *h, void *r, const void *a, const void *b, uint32_t batch, const char *what) {
    int rc = check_call(h, batch, what); if (rc) return rc;
    if (!r || !a || !b) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": null argument");
    if ((rc = check_aligned({r, a, b}, what))) return rc;
    return do_ew<OP>(h, r, a, b, batch, what);
}
extern "C" int fhe_rns_ntt_pointwise(fhe_rns_ntt_t *h, void *r, const void *a, const void *b, uint32_t batch) { return ew_call<0>(h, r, a, b, batch, "pointwise"); }
extern "C" int fhe_rns_ntt_multiply(fhe_rns_ntt_t *h, void *r, const void *a, const void *b, uint32_t batch) {
    int rc = check_call(h, batch, "multiply"); if (rc) return rc;
    if (!r || !a || !b) return fail(FHE_ERR_INVALID_ARG, "multiply: null argument");
    if ((rc = check_aligned({r, a, b}, "multiply"))) return rc;
    if ((rc = check_inputs(h, {a, b}, batch))) return rc;
    return do_multiply(h, r, a, b, batch);
}
extern "C" int fhe_rns_ntt_multiply_bcast(fhe_rns_ntt_t *h, void *r, const void *a, const void *b_one, uint32_t batch) {
    int rc = check_call(h, batch, "multiply_bcast"); if (rc) return rc;
    if (!r || !a || !b_one) return fail(FHE_ERR_INVALID_ARG, "multiply_bcast: null argument");
    if ((rc = check_aligned({r, a, b_one}, "multiply_bcast"))) return rc;
    if (r == b_one) return fail(FHE_ERR_INVALID_ARG, "multiply_bcast: the result must not overwrite the shared operand");
    if (h->width != FHE_WIDTH_256 && !h->sub_top) { // every workgroup reads limb (p % L) of the one shared polynomial: L2 hits after the first use
        if ((rc = ensure_need(h, need_multiply(h, batch)))) return rc;
        return lds_multiply(h, r, a, b_one, batch * h->L, h->L);
    }
    const size_t S = (size_t)h->L * h->n * 32;
    for (uint32_t i = 0; i < batch; i++)
        if ((rc = do_multiply(h, (char *)r + i * S, (const char *)a + i * S, b_one, 1))) return rc;
    return FHE_OK;
}
extern "C" int fhe_rns_poly_add(fhe_rns_ntt_t *h, void *r, const void *a, const void *b, uint32_t batch) { return ew_call<1>(h, r, a, b, batch, "poly_add"); }
extern "C" int fhe_rns_mul_mont_literal(fhe_rns_ntt_t *h, void *r, const void *a, const void *b, uint32_t batch) {
    int rc = check_call(h, batch, "mul_mont_literal"); if (rc) return rc;
    if (!r || !a || !b) return fail(FHE_ERR_INVALID_ARG, "mul_mont_literal: null argument");
    if ((rc = check_aligned({r, a, b}, "mul_mont_literal"))) return rc;
    if (h->width != FHE_WIDTH_256) return fail(FHE_ERR_UNSUPPORTED, "mul_mont_literal: R = 2^256 Montgomery products exist on full-width handles only "
                                                                    "(an RNS base from fhe_rns_base_create, or FHE_HIP_FORCE_WIDTH=256)");
    return run256_ew<3>(h, r, a, b, batch * h->L, "mul_mont_literal");
}
extern "C" int fhe_rns_poly_sub(fhe_rns_ntt_t *h, void *r, const void *a, const void *b, uint32_t batch) { return ew_call<2>(h, r, a, b, batch, "poly_sub"); }
extern "C" int fhe_ct_multiply(fhe_rns_ntt_t *h, void *c0, void *c1, void *c2, const void *a0, const void *a1,
                               const void *b0, const void *b1, uint32_t batch) {
    int rc = check_call(h, batch, "ct_multiply"); if (rc) return rc;
    if (!c0 || !c1 || !c2 || !a0 || !a1 || !b0 || !b1) return fail(FHE_ERR_INVALID_ARG, "ct_multiply: null argument");
    if ((rc = check_aligned({c0, c1, c2, a0, a1, b0, b1}, "ct_multiply"))) return rc;
    const void *ins[4] = {a0, a1, b0, b1}; void *outs[3] = {c0, c1, c2};
    for (void *o : outs) for (const void *i : ins) if (o == i) return fail(FHE_ERR_INVALID_ARG, "ct_multiply: outputs must not alias inputs");
    if (c0 == c1 || c0 == c2 || c1 == c2) return fail(FHE_ERR_INVALID_ARG, "ct_multiply: outputs must be distinct");
    if ((rc = check_inputs(h, {a0, a1, b0, b1}, batch))) return rc;
    return do_ct_multiply(h, c0, c1, c2, a0, a1, b0, b1, batch);
}
extern "C" int fhe_rns_check_canonical(fhe_rns_ntt_t *h, const void *d_data, uint32_t batch) {
    int rc = check_call(h, batch, "check_canonical"); if (rc) return rc;
    if (!d_data) return fail(FHE_ERR_INVALID_ARG, "check_canonical: null data");
    if ((rc = check_aligned({d_data}, "check_canonical"))) return rc;
    const uint32_t polys = batch * h->L;
    HIP_TRY(hipMemsetAsync(h->d_flag, 0, sizeof(uint32_t), h->stream));
    if (h->width != FHE_WIDTH_256) rc = with_word_field(h, [&](auto f) { return lds_check<decltype(f)>(h, d_data, polys); });
    else {
        size_t count = (size_t)polys * h->n;
        hipLaunchKernelGGL(fhe_dev::check256_kernel, dim3(ew_grid(count)), dim3(256), 0, h->stream, (const fhe_dev::u256 *)d_data,
                           (const fhe_dev::Limb256 *)h->d_limbs, h->L, h->log_n, count, h->d_flag);
        rc = post_launch(h->stream, "check256_kernel");
    }
    if (rc) return rc;
    uint32_t flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, h->d_flag, sizeof flag, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return flag ? fail(FHE_ERR_NONCANONICAL, "buffer holds coefficients that are not canonical residues of their limb modulus") : FHE_OK;
}

extern "C" int fhe_ntt_forward(fhe_ntt_t *h, void *d, uint32_t batch) { return h ? fhe_rns_ntt_forward(h->impl, d, batch) : fail(FHE_ERR_INVALID_ARG, "null handle"); }
extern "C" int fhe_ntt_inverse(fhe_ntt_t *h, void *d, uint32_t batch) { return h ? fhe_rns_ntt_inverse(h->impl, d, batch) : fail(FHE_ERR_INVALID_ARG, "null handle"); }
extern "C" int fhe_ntt_pointwise(fhe_ntt_t *h, void *r, const void *a, const void *b, uint32_t batch) {
    return h ? fhe_rns_ntt_pointwise(h->impl, r, a, b, batch) : fail(FHE_ERR_INVALID_ARG, "null handle");
}
extern "C" int fhe_ntt_multiply(fhe_ntt_t *h, void *r, const void *a, const void *b, uint32_t batch) {
    return h ? fhe_rns_ntt_multiply(h->impl, r, a, b, batch) : fail(FHE_ERR_INVALID_ARG, "null handle");
}
