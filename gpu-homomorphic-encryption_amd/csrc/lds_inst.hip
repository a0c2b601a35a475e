// lds_inst.hip -- one (field, LOGN) instance of the LDS-resident kernels.
// Compile with -DFHE_FIELD=F32|F52|F64|F64X -DFHE_LOGN=11..15 (the Makefile lists the instances).
#include <cstdlib>
#include "lds_launch.h"
#include "ntt_lds.hip.h"
#include "ntt_lds_small.hip.h"

#define CAT_(a, b, c) a##b##_##c
#define CAT(a, b, c) CAT_(a, b, c)

namespace fhe_dev {

#define OP_FORM(op, form) ((op) * 32 + (form))

// a template, so that the forms this instance lacks are not instantiated at all
template <class F, int LOGN>
static bool launch(const LdsArgs &A) {
    using E = typename F::E;
    constexpr int EB = sizeof(E);
    constexpr int MULT_MINW = F::MULT_MINW;
    const dim3 grid(A.polys), block(NttCfg<LOGN>::T);
    const Limb<F> *limbs = (const Limb<F> *)A.limbs;
    const bool in = A.in_compact, out = A.out_compact;
    if constexpr (LOGN == 13) {          // this instance also serves N = 2^14 .. 2^16 in two passes (ntt_sub_kernel / word_pass_kernel)
        // pass: one lane per column of a 2^13-column block (forward: containers -> compact), two per column (inverse: compact -> containers)
        const dim3 fgrid((1u << 13) >> 8, A.polys), igrid((2u << 13) >> 8, A.polys), sgrid(A.polys << A.top);
        switch (A.op) {
            case LDS_PASS_FWD:
                if (A.top == 3) hipLaunchKernelGGL((word_pass_kernel<F, 3, true>), fgrid, dim3(256), 0, A.stream, A.r0, A.a0, limbs, A.L, 16u, 0u);
                else if (A.top == 2) hipLaunchKernelGGL((word_pass_kernel<F, 2, true>), fgrid, dim3(256), 0, A.stream, A.r0, A.a0, limbs, A.L, 15u, 0u);
                else hipLaunchKernelGGL((word_pass_kernel<F, 1, true>), fgrid, dim3(256), 0, A.stream, A.r0, A.a0, limbs, A.L, 14u, 0u);
                return true;
            case LDS_PASS_INV:
                if (A.top == 3) hipLaunchKernelGGL((word_pass_kernel<F, 3, false>), igrid, dim3(256), 0, A.stream, A.r0, A.a0, limbs, A.L, 16u, A.rconst ? 1u : 0u);
                else if (A.top == 2) hipLaunchKernelGGL((word_pass_kernel<F, 2, false>), igrid, dim3(256), 0, A.stream, A.r0, A.a0, limbs, A.L, 15u, A.rconst ? 1u : 0u);
                else hipLaunchKernelGGL((word_pass_kernel<F, 1, false>), igrid, dim3(256), 0, A.stream, A.r0, A.a0, limbs, A.L, 14u, A.rconst ? 1u : 0u);
                return true;
            case LDS_SUB_FORWARD:
                hipLaunchKernelGGL((ntt_sub_kernel<F, 13, SUB_FORWARD, MULT_MINW>), sgrid, block, 0, A.stream, (char *)A.r0, (const char *)A.a0, (const char *)nullptr, limbs, A.L, A.top);
                return true;
            case LDS_SUB_INVERSE:
                hipLaunchKernelGGL((ntt_sub_kernel<F, 13, SUB_INVERSE, MULT_MINW>), sgrid, block, 0, A.stream, (char *)A.r0, (const char *)A.a0, (const char *)nullptr, limbs, A.L, A.top);
                return true;
            case LDS_SUB_MULTIPLY:
                hipLaunchKernelGGL((ntt_sub_kernel<F, 13, SUB_MULTIPLY, MULT_MINW>), sgrid, block, 0, A.stream, (char *)A.r0, (const char *)A.a0, (const char *)A.b0, limbs, A.L, A.top);
                return true;
            default: break;
        }
    }
    if (A.op == LDS_FORWARD) {
        hipLaunchKernelGGL((ntt_forward_kernel<F, LOGN>), grid, block, 0, A.stream, (char *)A.r0, limbs, A.L);
        return true;
    }
    if (A.op == LDS_INVERSE) {
        hipLaunchKernelGGL((ntt_inverse_kernel<F, LOGN>), grid, block, 0, A.stream, (char *)A.r0, limbs, A.L);
        return true;
    }
    // LDS_KEYSWITCH: the addends of r0, r1 are a1, b0 (compact, from the fused multiply + relinearise) or r0, r1 themselves (in place, containers);
    // the digit source c2 = a0 is compact whenever in_compact is set
    const bool add_in = A.a1 != nullptr;
    const char *add0 = add_in ? (const char *)A.a1 : (const char *)A.r0, *add1 = add_in ? (const char *)A.b0 : (const char *)A.r1;
    if (A.op == LDS_KEYSWITCH && (out || (add_in && !in))) return false;
    if ((A.op == LDS_MULTIPLY && (in || out)) || (A.op == LDS_CT_MULTIPLY && in)) return false;
    switch (OP_FORM(A.op, A.form)) {
        // ---- multiply: containers in and out --------------------------------------------------------------------------------------
        case OP_FORM(LDS_MULTIPLY, LDS_ONE_LAUNCH):
            hipLaunchKernelGGL((ntt_multiply_kernel<F, LOGN, MULT_MINW>), grid, block, 0, A.stream, (char *)A.r0, (const char *)A.a0,
                               (const char *)A.b0, limbs, A.L, A.b_polys ? 1u : 0u);
            return true;
        case OP_FORM(LDS_MULTIPLY, LDS_SQUARE):
            hipLaunchKernelGGL((ntt_multiply_kernel<F, LOGN, MULT_MINW, true>), grid, block, 0, A.stream, (char *)A.r0, (const char *)A.a0,
                               (const char *)A.b0, limbs, A.L, 0u);
            return true;
        case OP_FORM(LDS_MULTIPLY, LDS_SMALL16):     // one workgroup's latency is what counts (ntt_lds_small.hip.h); b == a simply loads twice
            if constexpr (lds_small_multiply(EB, LOGN)) {
                hipLaunchKernelGGL((ntt16_multiply_kernel<F, LOGN>), dim3(A.polys), dim3(Cfg16<LOGN>::T), 0, A.stream, (char *)A.r0, (const char *)A.a0,
                                   (const char *)A.b0, limbs, A.L, A.b_polys ? 1u : 0u);
                return true;
            }
            break;
        case OP_FORM(LDS_MULTIPLY, LDS_COOP4):       // each polynomial over four workgroups, three dependent launches (ntt_lds_small.hip.h)
            if constexpr (lds_coop4_multiply(EB, LOGN)) {
                const dim3 grid4(A.polys * 4), cgrid(A.polys * Coop4<F, LOGN>::CWG), block4(Coop4<F, LOGN>::T);      // blocks: four per limb polynomial; columns: CWG
                hipLaunchKernelGGL((ntt_multiply4_top_kernel<F, LOGN>), cgrid, block4, 0, A.stream, (const char *)A.a0, (const char *)A.b0, (E *)A.ws, limbs, A.L, A.b_polys ? 1u : 0u);
                hipLaunchKernelGGL((ntt_multiply4_block_kernel<F, LOGN>), grid4, dim3(2 * Coop4<F, LOGN>::T), 0, A.stream, (E *)A.ws, limbs, A.L);   // two groups: the forward transforms side by side
                hipLaunchKernelGGL((ntt_multiply4_last_kernel<F, LOGN>), cgrid, block4, 0, A.stream, (char *)A.r0, (const E *)A.ws, limbs, A.L);
                return true;
            }
            break;
        // ---- tensor product: containers in; out_compact: r0, r1, r2 compact (the first half of the fused multiply + relinearise) ------
        case OP_FORM(LDS_CT_MULTIPLY, LDS_ONE_LAUNCH):
            if constexpr (lds_ct_fused(EB, LOGN)) {
                if (out)
                    hipLaunchKernelGGL((ntt_ct_multiply_kernel<F, LOGN, false, true>), grid, block, 0, A.stream, (char *)A.r0, (char *)A.r1,
                                       (char *)A.r2, (const char *)A.a0, (const char *)A.a1, (const char *)A.b0, (const char *)A.b1, limbs, A.L);
                else
                    hipLaunchKernelGGL((ntt_ct_multiply_kernel<F, LOGN>), grid, block, 0, A.stream, (char *)A.r0, (char *)A.r1,
                                       (char *)A.r2, (const char *)A.a0, (const char *)A.a1, (const char *)A.b0, (const char *)A.b1, limbs, A.L);
                return true;
            }
            break;
        case OP_FORM(LDS_CT_MULTIPLY, LDS_SQUARE):
            if constexpr (lds_ct_fused(EB, LOGN)) {
                if (out) break;
                hipLaunchKernelGGL((ntt_ct_multiply_kernel<F, LOGN, true>), grid, block, 0, A.stream, (char *)A.r0, (char *)A.r1,
                                   (char *)A.r2, (const char *)A.a0, (const char *)A.a1, (const char *)A.b0, (const char *)A.b1, limbs, A.L);
                return true;
            }
            break;
        case OP_FORM(LDS_CT_MULTIPLY, LDS_SMALL16):
            if constexpr (lds_small_multiply(EB, LOGN)) {
                if (!out) break;
                hipLaunchKernelGGL((ntt16_ct_multiply_kernel<F, LOGN>), dim3(A.polys), dim3(Cfg16<LOGN>::T), 0, A.stream, (E *)A.r0, (E *)A.r1, (E *)A.r2,
                                   (const char *)A.a0, (const char *)A.a1, (const char *)A.b0, (const char *)A.b1, limbs, A.L);
                return true;
            }
            break;
        case OP_FORM(LDS_CT_MULTIPLY, LDS_COOP4):    // four workgroups per (ciphertext, limb), three launches
            if constexpr (lds_coop4_multiply(EB, LOGN)) {
                if (!out) break;
                const dim3 block4(Coop4<F, LOGN>::T);
                hipLaunchKernelGGL((ntt_ct4_top_kernel<F, LOGN>), dim3(A.polys * Coop4<F, LOGN>::CWG, 4), block4, 0, A.stream, (const char *)A.a0, (const char *)A.a1, (const char *)A.b0,
                                   (const char *)A.b1, (E *)A.ws, limbs, A.L);
                if constexpr (LOGN == 13)      // four groups of threads: the four forward transforms side by side, three inverses side by side
                    hipLaunchKernelGGL((ntt_ct4_block_kernel<F, LOGN>), dim3(A.polys * 4), dim3(4 * Coop4<F, LOGN>::T), 0, A.stream, (E *)A.ws, limbs, A.L);
                else
                    hipLaunchKernelGGL((ntt_ct4_block1_kernel<F, LOGN>), dim3(A.polys * 4), block4, 0, A.stream, (E *)A.ws, limbs, A.L);
                hipLaunchKernelGGL((ntt_ct4_last_kernel<F, LOGN>), dim3(A.polys * Coop4<F, LOGN>::CWG, 3), block4, 0, A.stream, (E *)A.r0, (E *)A.r1, (E *)A.r2, (const E *)A.ws, limbs, A.L);
                return true;
            }
            break;
        case OP_FORM(LDS_CT_MULTIPLY, LDS_TWO_LAUNCH):   // the b-side transforms into the workspace, then one workgroup per (ciphertext, limb) does the rest
            if constexpr (lds_ct_two_launch(EB, LOGN)) {
                E *w0 = (E *)A.ws, *w1 = w0 + (size_t)A.polys * (1u << LOGN);
                hipLaunchKernelGGL((ntt_forward_compact_kernel<F, LOGN, MULT_MINW>), dim3(A.polys, 2), block, 0, A.stream, w0, w1,
                                   (const char *)A.b0, (const char *)A.b1, limbs, A.L);
                if (out)
                    hipLaunchKernelGGL((ntt_ct_a_kernel<F, LOGN, MULT_MINW, true>), grid, block, 0, A.stream, (char *)A.r0, (char *)A.r1, (char *)A.r2,
                                       (const char *)A.a0, (const char *)A.a1, (const E *)w0, (const E *)w1, limbs, A.L);
                else
                    hipLaunchKernelGGL((ntt_ct_a_kernel<F, LOGN, MULT_MINW, false>), grid, block, 0, A.stream, (char *)A.r0, (char *)A.r1, (char *)A.r2,
                                       (const char *)A.a0, (const char *)A.a1, (const E *)w0, (const E *)w1, limbs, A.L);
                return true;
            }
            break;
        case OP_FORM(LDS_CT_MULTIPLY, LDS_THREE_LAUNCH):   // four transformed operands exceed the register file: c0, c2 by the fused multiply, c1 by the two-product kernel
            if constexpr (!lds_ct_fused(EB, LOGN)) {
                if (out) {
                    hipLaunchKernelGGL((ntt_multiply_kernel<F, LOGN, MULT_MINW, false, true>), grid, block, 0, A.stream, (char *)A.r0,
                                       (const char *)A.a0, (const char *)A.b0, limbs, A.L, 0u);
                    hipLaunchKernelGGL((ntt_multiply_kernel<F, LOGN, MULT_MINW, false, true>), grid, block, 0, A.stream, (char *)A.r2,
                                       (const char *)A.a1, (const char *)A.b1, limbs, A.L, 0u);
                    hipLaunchKernelGGL((ntt_mac2_kernel<F, LOGN, MULT_MINW, true>), grid, block, 0, A.stream, (char *)A.r1, (const char *)A.a0,
                                       (const char *)A.b1, (const char *)A.a1, (const char *)A.b0, limbs, A.L);
                } else {
                    hipLaunchKernelGGL((ntt_multiply_kernel<F, LOGN, MULT_MINW>), grid, block, 0, A.stream, (char *)A.r0,
                                       (const char *)A.a0, (const char *)A.b0, limbs, A.L, 0u);
                    hipLaunchKernelGGL((ntt_multiply_kernel<F, LOGN, MULT_MINW>), grid, block, 0, A.stream, (char *)A.r2,
                                       (const char *)A.a1, (const char *)A.b1, limbs, A.L, 0u);
                    hipLaunchKernelGGL((ntt_mac2_kernel<F, LOGN, MULT_MINW>), grid, block, 0, A.stream, (char *)A.r1, (const char *)A.a0,
                                       (const char *)A.b1, (const char *)A.a1, (const char *)A.b0, limbs, A.L);
                }
                return true;
            }
            break;
        // ---- key switch: r0, r1 containers ------------------------------------------------------------------------------------------
        case OP_FORM(LDS_KEYSWITCH, LDS_SPLIT):
            if constexpr (lds_keyswitch_split(EB, LOGN)) {
                if (add_in)
                    hipLaunchKernelGGL((ntt_keyswitch_kernel<F, LOGN, 2, true, false, true>), dim3(A.polys * 2), block, 0, A.stream, (char *)A.r0, (char *)A.r1,
                                       (const char *)A.a0, add0, add1, (const E *)A.kb, (const E *)A.ka, limbs, A.L, A.K, A.w);
                else if (!in)
                    hipLaunchKernelGGL((ntt_keyswitch_kernel<F, LOGN, 2, true>), dim3(A.polys * 2), block, 0, A.stream, (char *)A.r0, (char *)A.r1,
                                       (const char *)A.a0, add0, add1, (const E *)A.kb, (const E *)A.ka, limbs, A.L, A.K, A.w);
                else
                    break;
                return true;
            }
            break;
        case OP_FORM(LDS_KEYSWITCH, LDS_JOINT3):
            if constexpr (lds_keyswitch_joint3(EB, LOGN)) {
                if (add_in)
                    hipLaunchKernelGGL((ntt_keyswitch3_kernel<F, LOGN, 2, true>), grid, block, 0, A.stream, (char *)A.r0, (char *)A.r1,
                                       (const char *)A.a0, add0, add1, (const E *)A.kb, (const E *)A.ka, limbs, A.L, A.K, A.w);
                else if (in)
                    hipLaunchKernelGGL((ntt_keyswitch3_kernel<F, LOGN, 2, true, false>), grid, block, 0, A.stream, (char *)A.r0, (char *)A.r1,
                                       (const char *)A.a0, add0, add1, (const E *)A.kb, (const E *)A.ka, limbs, A.L, A.K, A.w);
                else
                    hipLaunchKernelGGL((ntt_keyswitch3_kernel<F, LOGN, 2, false>), grid, block, 0, A.stream, (char *)A.r0, (char *)A.r1,
                                       (const char *)A.a0, add0, add1, (const E *)A.kb, (const E *)A.ka, limbs, A.L, A.K, A.w);
                return true;
            }
            break;
        case OP_FORM(LDS_KEYSWITCH, LDS_PAIRED):
            if constexpr (lds_paired_keyswitch(EB, LOGN)) {
                if (add_in)
                    hipLaunchKernelGGL((ntt_keyswitch2_kernel<F, LOGN, 2, true>), grid, block, 0, A.stream, (char *)A.r0, (char *)A.r1,
                                       (const char *)A.a0, add0, add1, (const E *)A.kb, (const E *)A.ka, limbs, A.L, A.K, A.w);
                else if (in)
                    hipLaunchKernelGGL((ntt_keyswitch2_kernel<F, LOGN, 2, true, false>), grid, block, 0, A.stream, (char *)A.r0, (char *)A.r1,
                                       (const char *)A.a0, add0, add1, (const E *)A.kb, (const E *)A.ka, limbs, A.L, A.K, A.w);
                else
                    hipLaunchKernelGGL((ntt_keyswitch2_kernel<F, LOGN, 2>), grid, block, 0, A.stream, (char *)A.r0, (char *)A.r1,
                                       (const char *)A.a0, add0, add1, (const E *)A.kb, (const E *)A.ka, limbs, A.L, A.K, A.w);
                return true;
            }
            break;
        case OP_FORM(LDS_KEYSWITCH, LDS_SINGLE_LDS_TW):
            if constexpr (lds_twiddles_in_lds(EB, LOGN)) {
                if (in) break;
                hipLaunchKernelGGL((ntt_keyswitch_kernel<F, LOGN, 2, false, true>), grid, block, 0, A.stream, (char *)A.r0, (char *)A.r1,
                                   (const char *)A.a0, add0, add1, (const E *)A.kb, (const E *)A.ka, limbs, A.L, A.K, A.w);
                return true;
            }
            break;
        case OP_FORM(LDS_KEYSWITCH, LDS_SINGLE_L2_TW):
            if constexpr (!lds_keyswitch_split(EB, LOGN)) {
                if (in) break;
                hipLaunchKernelGGL((ntt_keyswitch_kernel<F, LOGN, 2, false>), grid, block, 0, A.stream, (char *)A.r0, (char *)A.r1,
                                   (const char *)A.a0, add0, add1, (const E *)A.kb, (const E *)A.ka, limbs, A.L, A.K, A.w);
                return true;
            }
            break;
        case OP_FORM(LDS_KEYSWITCH, LDS_PARTS16):    // few ciphertexts: one workgroup per DIGIT, then one per (ciphertext, limb, component) sums the partials
            if constexpr (lds_small_multiply(EB, LOGN)) {
                const uint32_t LK = A.L * A.K;
                const dim3 b16(Cfg16<LOGN>::T), pgrid(A.polys * LK), cgrid(A.polys, 2);
                E *part0 = (E *)A.ws, *part1 = part0 + (size_t)A.polys * LK * (1u << LOGN);
                if (in)
                    hipLaunchKernelGGL((ntt_keyswitch16_part_kernel<F, LOGN, true>), pgrid, b16, 0, A.stream, part0, part1, (const char *)A.a0, (const char *)nullptr, (const E *)A.kb, (const E *)A.ka,
                                       (const E *)nullptr, (const E *)nullptr, limbs, A.L, A.K, A.w);
                else
                    hipLaunchKernelGGL((ntt_keyswitch16_part_kernel<F, LOGN, false>), pgrid, b16, 0, A.stream, part0, part1, (const char *)A.a0, (const char *)nullptr, (const E *)A.kb, (const E *)A.ka,
                                       (const E *)nullptr, (const E *)nullptr, limbs, A.L, A.K, A.w);
                if (add_in)
                    hipLaunchKernelGGL((ntt_keyswitch16_comb_kernel<F, LOGN, true>), cgrid, b16, 0, A.stream, (char *)A.r0, (char *)A.r1, (const E *)part0, (const E *)part1,
                                       add0, add1, limbs, A.L, LK);
                else
                    hipLaunchKernelGGL((ntt_keyswitch16_comb_kernel<F, LOGN, false>), cgrid, b16, 0, A.stream, (char *)A.r0, (char *)A.r1, (const E *)part0, (const E *)part1,
                                       add0, add1, limbs, A.L, LK);
                return true;
            }
            break;
        case OP_FORM(LDS_KEYSWITCH, LDS_PART_PAIRS):   // few ciphertexts: one workgroup per digit PAIR, then one per (ciphertext, limb) sums the partials
            if constexpr (lds_paired_keyswitch(EB, LOGN)) {
                const uint32_t NP = (A.L * A.K + 1) / 2;
                const dim3 pgrid(A.polys * NP), cgrid(A.polys);
                E *part0 = (E *)A.ws, *part1 = part0 + (size_t)A.polys * NP * (1u << LOGN);
                if (in)
                    hipLaunchKernelGGL((ntt_keyswitch2_part_kernel<F, LOGN, true>), pgrid, block, 0, A.stream, part0, part1, (const char *)A.a0, (const char *)nullptr, (const E *)A.kb, (const E *)A.ka,
                                       (const E *)nullptr, (const E *)nullptr, limbs, A.L, A.K, A.w);
                else
                    hipLaunchKernelGGL((ntt_keyswitch2_part_kernel<F, LOGN, false>), pgrid, block, 0, A.stream, part0, part1, (const char *)A.a0, (const char *)nullptr, (const E *)A.kb, (const E *)A.ka,
                                       (const E *)nullptr, (const E *)nullptr, limbs, A.L, A.K, A.w);
                if (add_in)
                    hipLaunchKernelGGL((ntt_keyswitch2_comb_kernel<F, LOGN, true>), cgrid, block, 0, A.stream, (char *)A.r0, (char *)A.r1, (const E *)part0, (const E *)part1,
                                       add0, add1, limbs, A.L, NP);
                else
                    hipLaunchKernelGGL((ntt_keyswitch2_comb_kernel<F, LOGN, false>), cgrid, block, 0, A.stream, (char *)A.r0, (char *)A.r1, (const E *)part0, (const E *)part1,
                                       add0, add1, limbs, A.L, NP);
                return true;
            }
            break;
        // ---- external product: b0, b1 = pre-rotated digit sources where given ---------------------------------------------------------
        case OP_FORM(LDS_EXTPROD, LDS_SPLIT):
            if constexpr (lds_keyswitch_split(EB, LOGN)) {
                if (in || out || A.b0) break;
                hipLaunchKernelGGL((ntt_extprod_kernel<F, LOGN, 2, true>), dim3(A.polys * 2), block, 0, A.stream, (char *)A.r0, (char *)A.r1,
                                   (const char *)A.a0, (const char *)A.a1, A.shifts, (const E *)A.kb, (const E *)A.ka, (const E *)A.kb1,
                                   (const E *)A.ka1, limbs, A.L, A.K, A.w);
                return true;
            }
            break;
        case OP_FORM(LDS_EXTPROD, LDS_JOINT3):
            if constexpr (lds_keyswitch_joint3(EB, LOGN)) {
#define EXTPROD3(IC, OC, PR) hipLaunchKernelGGL((ntt_extprod3_kernel<F, LOGN, 2, IC, OC, PR>), grid, block, 0, A.stream, (char *)A.r0, (char *)A.r1, \
                                       (const char *)A.a0, (const char *)A.a1, (const char *)A.b0, (const char *)A.b1, A.shifts, (const E *)A.kb, (const E *)A.ka, \
                                       (const E *)A.kb1, (const E *)A.ka1, limbs, A.L, A.K, A.w)
                if (!in && (out || A.b0)) break;     // container input with compact output, or pre-rotated sources beside container input: never asked for
                if (A.b0) { if (out) EXTPROD3(true, true, true); else EXTPROD3(true, false, true); }
                else if (in && out) EXTPROD3(true, true, false);
                else if (in) EXTPROD3(true, false, false);
                else EXTPROD3(false, false, false);
#undef EXTPROD3
                return true;
            }
            break;
        case OP_FORM(LDS_EXTPROD, LDS_PAIRED):
            if constexpr (lds_paired_extprod(EB, LOGN)) {
                if (A.b0) break;
#define EXTPROD2(IC, OC) hipLaunchKernelGGL((ntt_extprod2_kernel<F, LOGN, 2, IC, OC>), grid, block, 0, A.stream, (char *)A.r0, (char *)A.r1, \
                                       (const char *)A.a0, (const char *)A.a1, A.shifts, (const E *)A.kb, (const E *)A.ka, (const E *)A.kb1, \
                                       (const E *)A.ka1, limbs, A.L, A.K, A.w)
                if (in && out) EXTPROD2(true, true);
                else if (in) EXTPROD2(true, false);
                else if (out) EXTPROD2(false, true);
                else EXTPROD2(false, false);
#undef EXTPROD2
                return true;
            }
            break;
        case OP_FORM(LDS_EXTPROD, LDS_SINGLE_LDS_TW):
            if constexpr (lds_twiddles_in_lds(EB, LOGN)) {
                if (in || out || A.b0) break;
                hipLaunchKernelGGL((ntt_extprod_kernel<F, LOGN, 2, false, true>), grid, block, 0, A.stream, (char *)A.r0, (char *)A.r1,
                                   (const char *)A.a0, (const char *)A.a1, A.shifts, (const E *)A.kb, (const E *)A.ka, (const E *)A.kb1,
                                   (const E *)A.ka1, limbs, A.L, A.K, A.w);
                return true;
            }
            break;
        case OP_FORM(LDS_EXTPROD, LDS_SINGLE_L2_TW):
            if constexpr (!lds_keyswitch_split(EB, LOGN)) {
                if (in || out || A.b0) break;
                hipLaunchKernelGGL((ntt_extprod_kernel<F, LOGN, 2, false>), grid, block, 0, A.stream, (char *)A.r0, (char *)A.r1,
                                   (const char *)A.a0, (const char *)A.a1, A.shifts, (const E *)A.kb, (const E *)A.ka, (const E *)A.kb1,
                                   (const E *)A.ka1, limbs, A.L, A.K, A.w);
                return true;
            }
            break;
        // few accumulators: the key-switch launches above with two digit sources -- the pre-rotated components b0, b1 with their RGSW rows --
        // and the accumulator pair a0, a1 as addends; r0, r1 compact or containers
        case OP_FORM(LDS_EXTPROD, LDS_PARTS16):
            if constexpr (lds_small_multiply(EB, LOGN)) {
                if (!in || !A.b0) break;
                const uint32_t LK = A.L * A.K;
                const dim3 b16(Cfg16<LOGN>::T), pgrid(A.polys * LK, 2), cgrid(A.polys, 2);
                E *part0 = (E *)A.ws, *part1 = part0 + (size_t)A.polys * 2 * LK * (1u << LOGN);
                hipLaunchKernelGGL((ntt_keyswitch16_part_kernel<F, LOGN, true>), pgrid, b16, 0, A.stream, part0, part1, (const char *)A.b0, (const char *)A.b1, (const E *)A.kb, (const E *)A.ka,
                                   (const E *)A.kb1, (const E *)A.ka1, limbs, A.L, A.K, A.w);
                if (out)
                    hipLaunchKernelGGL((ntt_keyswitch16_comb_kernel<F, LOGN, true, true>), cgrid, b16, 0, A.stream, (char *)A.r0, (char *)A.r1, (const E *)part0, (const E *)part1,
                                       (const char *)A.a0, (const char *)A.a1, limbs, A.L, 2 * LK);
                else
                    hipLaunchKernelGGL((ntt_keyswitch16_comb_kernel<F, LOGN, true, false>), cgrid, b16, 0, A.stream, (char *)A.r0, (char *)A.r1, (const E *)part0, (const E *)part1,
                                       (const char *)A.a0, (const char *)A.a1, limbs, A.L, 2 * LK);
                return true;
            }
            break;
        case OP_FORM(LDS_EXTPROD, LDS_PART_PAIRS):   // one workgroup per digit PAIR of a component (paired 32-per-thread transform), paired combining launch
            if constexpr (lds_paired_extprod(EB, LOGN) && !lds_small_multiply(EB, LOGN)) {
                if (!in || !A.b0) break;
                const uint32_t NP = (A.L * A.K + 1) / 2;
                const dim3 pgrid(A.polys * NP, 2), cgrid(A.polys);
                E *part0 = (E *)A.ws, *part1 = part0 + (size_t)A.polys * 2 * NP * (1u << LOGN);
                hipLaunchKernelGGL((ntt_keyswitch2_part_kernel<F, LOGN, true>), pgrid, block, 0, A.stream, part0, part1, (const char *)A.b0, (const char *)A.b1, (const E *)A.kb, (const E *)A.ka,
                                   (const E *)A.kb1, (const E *)A.ka1, limbs, A.L, A.K, A.w);
                if (out)
                    hipLaunchKernelGGL((ntt_keyswitch2_comb_kernel<F, LOGN, true, true>), cgrid, block, 0, A.stream, (char *)A.r0, (char *)A.r1, (const E *)part0, (const E *)part1,
                                       (const char *)A.a0, (const char *)A.a1, limbs, A.L, 2 * NP);
                else
                    hipLaunchKernelGGL((ntt_keyswitch2_comb_kernel<F, LOGN, true, false>), cgrid, block, 0, A.stream, (char *)A.r0, (char *)A.r1, (const E *)part0, (const E *)part1,
                                       (const char *)A.a0, (const char *)A.a1, limbs, A.L, 2 * NP);
                return true;
            }
            break;
        default: break;
    }
    return false;
}

bool CAT(lds_launch_, FHE_FIELD, FHE_LOGN)(const LdsArgs &A) { return launch<FHE_FIELD, FHE_LOGN>(A); }

}  // namespace fhe_dev
