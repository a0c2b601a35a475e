// lds_inst.hip -- one (field, LOGN) instance of the LDS-resident kernels.
// Compile with -DFHE_FIELD=F32|F52|F64|F64X -DFHE_LOGN=11..15 (the Makefile lists the instances).
#include <cstdlib>
#include <type_traits>
#include "lds_launch.h"
#include "decrypt.hip.h"
#include "encode.hip.h"
#include "encrypt.hip.h"
#include "hoist.hip.h"
#include "hoist_lincomb.hip.h"
#include "keygen.hip.h"
#include "ntt_lds.hip.h"
#include "ntt_lds_small.hip.h"

#define CAT_(a, b, c) a##b##_##c
#define CAT(a, b, c) CAT_(a, b, c)

namespace fhe_dev {

#define OP_FORM(op, form) ((op) * 32 + (form))

// Runtime bools -> std::bool_constant arguments of a generic lambda, so that a kernel call whose template arguments depend on them is
// written once.  The lambda is instantiated for EVERY combination: one that must not exist is excluded with `if constexpr` inside it.
template <class Fn> static void with_bools(Fn &&fn) { fn(); }
template <class Fn, class... Bs> static void with_bools(Fn &&fn, bool b, Bs... rest) {
    if (b) with_bools([&](auto... c) { fn(std::true_type{}, c...); }, rest...);
    else with_bools([&](auto... c) { fn(std::false_type{}, c...); }, rest...);
}
// ... and the number of pass stages, 1..3, as an std::integral_constant
template <class Fn> static void with_top(uint32_t top, Fn &&fn) {
    if (top == 3) fn(std::integral_constant<int, 3>{});
    else if (top == 2) fn(std::integral_constant<int, 2>{});
    else fn(std::integral_constant<int, 1>{});
}

// a template, so that the forms this instance lacks are not instantiated at all
template <class F, int LOGN>
static bool launch(const LdsArgs &A) {
    using E = typename F::E;
    constexpr int EB = sizeof(E);
    constexpr int MULT_MINW = F::MULT_MINW;
    const dim3 grid(A.polys), block(NttCfg<LOGN>::T);
    const Limb<F> *limbs = (const Limb<F> *)A.limbs;
    const bool in = A.in_compact, ac = A.add_compact, out = A.out_compact;
    if constexpr (LOGN == 13) {          // this instance also serves N = 2^14 .. 2^16 in two passes (ntt_sub_kernel / word_pass_kernel)
        // pass: one lane per column of a 2^13-column block (forward: containers -> compact), two per column (inverse: compact -> containers);
        // sub-transforms: forward compact -> containers, inverse containers -> compact, multiply compact -> compact
        const dim3 fgrid((1u << 13) >> 8, A.polys), igrid((2u << 13) >> 8, A.polys), sgrid(A.polys << A.top);
        auto pass = [&](auto FWD) {
            constexpr bool fwd = decltype(FWD)::value;
            if (in == fwd || out != fwd) return false;
            with_top(A.top, [&](auto R) {
                hipLaunchKernelGGL((word_pass_kernel<F, decltype(R)::value, fwd>), fwd ? fgrid : igrid, dim3(256), 0, A.stream, A.r0, A.a0, limbs, A.L, 13u + R, !fwd && A.rconst ? 1u : 0u);
            });
            return true;
        };
        auto sub = [&](auto MODE, bool want_in, bool want_out) {
            if (in != want_in || out != want_out) return false;
            hipLaunchKernelGGL((ntt_sub_kernel<F, 13, decltype(MODE)::value, MULT_MINW>), sgrid, block, 0, A.stream, (char *)A.r0, (const char *)A.a0, (const char *)A.b0, limbs, A.L, A.top);
            return true;
        };
        switch (A.op) {
            case LDS_PASS_FWD: return pass(std::true_type{});
            case LDS_PASS_INV: return pass(std::false_type{});
            case LDS_SUB_FORWARD: return sub(std::integral_constant<int, SUB_FORWARD>{}, true, false);
            case LDS_SUB_INVERSE: return sub(std::integral_constant<int, SUB_INVERSE>{}, false, true);
            case LDS_SUB_MULTIPLY: return sub(std::integral_constant<int, SUB_MULTIPLY>{}, true, true);
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
    // Hoisted rotations: compact c1 in, kept polynomials out; kept polynomials and a compact addend in, containers out
    if (A.op == LDS_HOIST || A.op == LDS_HOIST_APPLY) {
        if constexpr (lds_hoist(EB, LOGN)) {
            if (A.op == LDS_HOIST) {
                if (!in || out) return false;
                hipLaunchKernelGGL((ntt_hoist_kernel<F, LOGN, 2>), grid, block, 0, A.stream, (E *)A.r0, (const char *)A.c2, limbs, A.L, A.K, A.w);
            } else {
                if (!in || !ac || out || !A.add0) return false;
                hipLaunchKernelGGL((ntt_hoist_apply_kernel<F, LOGN, 2>), grid, block, 0, A.stream, (char *)A.r0, (char *)A.r1, (const E *)A.c2, (const char *)A.add0,
                                   (const E *)A.kb, (const E *)A.ka, limbs, A.L, A.K, A.galois);
            }
            return true;
        }
        return false;
    }
    // Hoisted linear transform: containers in, canonical hoist-layout residues out; those, the kept polynomials and the term table in, containers out
    if (A.op == LDS_HOIST_FWD || A.op == LDS_HOIST_LINCOMB) {
        if constexpr (lds_hoist_lincomb(EB, LOGN)) {
            if (A.op == LDS_HOIST_FWD) {
                if (in || !out || !A.a0) return false;
                hipLaunchKernelGGL((ntt_hoist_fwd_kernel<F, LOGN, 2>), dim3(A.polys, A.a1 ? 2 : 1), block, 0, A.stream, (E *)A.r0, (const char *)A.a0, (const char *)A.a1, limbs, A.L);
            } else {
                constexpr bool split = lds_hoist_lincomb_split(EB);
                if (!in || !ac || out || !A.add0 || !A.terms || !A.num_terms) return false;
                hipLaunchKernelGGL((ntt_hoist_lincomb_kernel<F, LOGN, 2, split>), dim3(A.polys * (split ? 2 : 1)), block, 0, A.stream, (char *)A.r0, (char *)A.r1, (const E *)A.c2,
                                   (const E *)A.add0, (const E *)A.add1, (const LincombTerm *)A.terms, A.num_terms, limbs, A.L, A.K);
            }
            return true;
        }
        return false;
    }
    // Public-key encryption: m in containers (or none), containers out, nothing else
    if (A.op == LDS_ENCRYPT) {
        if constexpr (lds_encrypt(EB, LOGN)) {
            if (in || out || !A.r0 || !A.r1 || !A.kb || !A.ka || !A.cdt || !A.cdt_len || A.cdt_len > ENCRYPT_MAX_CDT || A.polys % A.L) return false;
            hipLaunchKernelGGL((ntt_encrypt_kernel<F, LOGN, 2>), dim3(A.per_ct ? A.polys / A.L : A.polys), block, 0, A.stream, (char *)A.r0, (char *)A.r1, (const char *)A.a0,
                               (const E *)A.kb, (const E *)A.ka, A.cdt, A.cdt_len, A.seeds[0], A.seeds[1], A.seeds[2], A.t, limbs, A.L, A.per_ct ? 1u : 0u);
            return true;
        }
        return false;
    }
    // Secret-key decryption, first launch: containers in, the compact decryption workspace out
    if (A.op == LDS_DECRYPT) {
        if constexpr (lds_decrypt(EB, LOGN)) {
            if (in || !out || !A.r0 || !A.a0 || !A.a1 || !A.kb || (A.c2 && !A.ka) || A.polys % A.L) return false;
            hipLaunchKernelGGL((ntt_decrypt_kernel<F, LOGN, 2>), grid, block, 0, A.stream, (E *)A.r0, (const char *)A.a0, (const char *)A.a1, (const char *)A.c2,
                               (const E *)A.kb, (const E *)A.ka, limbs, A.L);
            return true;
        }
        return false;
    }
    // Key-switching key generation: nothing in but the kept secret key, the packed tables of every set out
    if (A.op == LDS_KEYGEN) {
        if constexpr (lds_keygen(EB, LOGN)) {
            if (in || out || !A.a0 || !A.kb || !A.ka || !A.cdt || !A.cdt_len || A.cdt_len > ENCRYPT_MAX_CDT || !A.K || !A.w || A.polys % (A.L * A.K * A.L)) return false;
            hipLaunchKernelGGL((ntt_keygen_kernel<F, LOGN, 2>), grid, block, 0, A.stream, (const KeygenSet *)A.a0, (const E *)A.kb, (const E *)A.ka, A.cdt, A.cdt_len,
                               A.seeds[0], A.seeds[1], A.t, limbs, A.L, A.K, A.w);
            return true;
        }
        return false;
    }
    // RGSW key generation: the same, with the table of (tables, message, component) and the packed transformed s alone
    if (A.op == LDS_RGSW_KEYGEN) {
        if constexpr (lds_keygen(EB, LOGN)) {
            if (in || out || !A.a0 || !A.kb || !A.cdt || !A.cdt_len || A.cdt_len > ENCRYPT_MAX_CDT || !A.K || !A.w || A.polys % (A.L * A.K * A.L)) return false;
            hipLaunchKernelGGL((ntt_rgsw_keygen_kernel<F, LOGN, 2>), grid, block, 0, A.stream, (const RgswSet *)A.a0, (const E *)A.kb, A.cdt, A.cdt_len,
                               A.seeds[0], A.seeds[1], A.t, limbs, A.L, A.K, A.w);
            return true;
        }
        return false;
    }
    // Batch encoder: this instance is the field of the plaintext modulus; slot words in, containers out / words or containers in, slot words out
    if (A.op == LDS_SLOTS_ENCODE || A.op == LDS_SLOTS_DECODE) {
        if constexpr (lds_slots(EB, LOGN)) {
            if (!A.r0 || !A.a0 || !A.kb || !A.L) return false;
            if (A.op == LDS_SLOTS_ENCODE) {
                if (!in || out || !A.ka) return false;
                hipLaunchKernelGGL((ntt_slots_encode_kernel<F, LOGN>), grid, block, 0, A.stream, (char *)A.r0, (const uint64_t *)A.a0, (const uint32_t *)A.kb,
                                   (const fhe_host::ModT *)A.ka, limbs, A.L);
            } else {
                if (!out) return false;
                with_bools([&](auto IN) {
                    hipLaunchKernelGGL((ntt_slots_decode_kernel<F, LOGN, !decltype(IN)::value>), grid, block, 0, A.stream, (uint64_t *)A.r0, (const char *)A.a0,
                                       (const uint32_t *)A.kb, limbs, A.L);
                }, in);
            }
            return true;
        }
        return false;
    }
    // What no form has a kernel for.  Multiply: containers in and out.  Tensor product: containers in.  Key switch: r0, r1 containers; the addends
    // are given, compact and beside a compact digit source (the fused multiply + relinearise), or not given: r0, r1 are accumulated in place.
    // External product: the pair a0, a1 is its own addend (in_compact says it all).
    const bool prerot = A.rot0 != nullptr;
    if (A.op == LDS_KEYSWITCH && (out || ac != (A.add0 != nullptr) || (ac && !in))) return false;
    if ((A.op == LDS_MULTIPLY && (in || out)) || (A.op == LDS_CT_MULTIPLY && in)) return false;
    if (A.op == LDS_EXTPROD && ac) return false;
    const char *add0 = A.add0 ? (const char *)A.add0 : (const char *)A.r0, *add1 = A.add0 ? (const char *)A.add1 : (const char *)A.r1;
    // One digit transform at a time: two workgroups per (ciphertext, limb), one per key half (SPLIT), or one with the twiddles in LDS (TWL) or read through L2
    auto keyswitch1 = [&](auto SPLIT, auto TWL, auto AC) {
        hipLaunchKernelGGL((ntt_keyswitch_kernel<F, LOGN, 2, decltype(SPLIT)::value, decltype(TWL)::value, decltype(AC)::value>), dim3(A.polys * (decltype(SPLIT)::value ? 2 : 1)), block, 0,
                           A.stream, (char *)A.r0, (char *)A.r1, (const char *)A.c2, add0, add1, (const E *)A.kb, (const E *)A.ka, limbs, A.L, A.K, A.w);
    };
    auto extprod1 = [&](auto SPLIT, auto TWL) {
        hipLaunchKernelGGL((ntt_extprod_kernel<F, LOGN, 2, decltype(SPLIT)::value, decltype(TWL)::value>), dim3(A.polys * (decltype(SPLIT)::value ? 2 : 1)), block, 0, A.stream,
                           (char *)A.r0, (char *)A.r1, (const char *)A.a0, (const char *)A.a1, A.shifts, (const E *)A.kb, (const E *)A.ka, (const E *)A.kb1,
                           (const E *)A.ka1, limbs, A.L, A.K, A.w);
    };
    // Few ciphertexts, shared by the key switch (SRCS = 1: digit source c2, addends add0 / add1) and the external product (SRCS = 2: the pre-rotated
    // pair with the rows kb / ka and kb1 / ka1, addends = the compact accumulator pair): one workgroup per digit (16-per-thread transforms) or
    // per digit PAIR (WIDE: paired 32-per-thread transforms) of each source, then a combining launch that sums the partials per limb polynomial,
    // runs the inverse transform(s) and adds the addends.  Generic, so that an instance compiles them where a case calls them and not before.
    auto parts = [&](auto SRCS, auto WIDE, const dim3 pblock, uint32_t np, const dim3 cgrid) {   // np: partials per source and limb polynomial
        constexpr uint32_t srcs = decltype(SRCS)::value;
        constexpr bool wide = decltype(WIDE)::value;
        const void *s0 = srcs == 1 ? A.c2 : A.rot0, *s1 = srcs == 1 ? nullptr : A.rot1;
        const char *t0 = srcs == 1 ? add0 : (const char *)A.a0, *t1 = srcs == 1 ? add1 : (const char *)A.a1;
        const dim3 pgrid(A.polys * np, srcs);
        E *part0 = (E *)A.ws, *part1 = part0 + (size_t)A.polys * srcs * np * (1u << LOGN);
        with_bools([&](auto IN) {
            if constexpr (wide)
                hipLaunchKernelGGL((ntt_keyswitch2_part_kernel<F, LOGN, decltype(IN)::value>), pgrid, pblock, 0, A.stream, part0, part1, (const char *)s0, (const char *)s1,
                                   (const E *)A.kb, (const E *)A.ka, (const E *)A.kb1, (const E *)A.ka1, limbs, A.L, A.K, A.w);
            else
                hipLaunchKernelGGL((ntt_keyswitch16_part_kernel<F, LOGN, decltype(IN)::value>), pgrid, pblock, 0, A.stream, part0, part1, (const char *)s0, (const char *)s1,
                                   (const E *)A.kb, (const E *)A.ka, (const E *)A.kb1, (const E *)A.ka1, limbs, A.L, A.K, A.w);
        }, in);
        auto comb = [&](auto AC, auto OC) {
            if constexpr (wide)
                hipLaunchKernelGGL((ntt_keyswitch2_comb_kernel<F, LOGN, decltype(AC)::value, decltype(OC)::value>), cgrid, pblock, 0, A.stream, (char *)A.r0, (char *)A.r1,
                                   (const E *)part0, (const E *)part1, t0, t1, limbs, A.L, srcs * np);
            else
                hipLaunchKernelGGL((ntt_keyswitch16_comb_kernel<F, LOGN, decltype(AC)::value, decltype(OC)::value>), cgrid, pblock, 0, A.stream, (char *)A.r0, (char *)A.r1,
                                   (const E *)part0, (const E *)part1, t0, t1, limbs, A.L, srcs * np);
        };
        if constexpr (srcs == 1) with_bools([&](auto AC) { comb(AC, std::false_type{}); }, ac);
        else with_bools([&](auto OC) { comb(std::true_type{}, OC); }, out);
        return true;
    };
    const uint32_t LK = A.L * A.K, NP = (LK + 1) / 2;
    constexpr std::integral_constant<uint32_t, 1> ONE{};
    constexpr std::integral_constant<uint32_t, 2> TWO{};
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
                with_bools([&](auto OC) {
                    hipLaunchKernelGGL((ntt_ct_multiply_kernel<F, LOGN, false, decltype(OC)::value>), grid, block, 0, A.stream, (char *)A.r0, (char *)A.r1,
                                       (char *)A.r2, (const char *)A.a0, (const char *)A.a1, (const char *)A.b0, (const char *)A.b1, limbs, A.L);
                }, out);
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
                with_bools([&](auto OC) {
                    hipLaunchKernelGGL((ntt_ct_a_kernel<F, LOGN, MULT_MINW, decltype(OC)::value>), grid, block, 0, A.stream, (char *)A.r0, (char *)A.r1, (char *)A.r2,
                                       (const char *)A.a0, (const char *)A.a1, (const E *)w0, (const E *)w1, limbs, A.L);
                }, out);
                return true;
            }
            break;
        case OP_FORM(LDS_CT_MULTIPLY, LDS_THREE_LAUNCH):   // four transformed operands exceed the register file: c0, c2 by the fused multiply, c1 by the two-product kernel
            if constexpr (!lds_ct_fused(EB, LOGN)) {
                with_bools([&](auto OC) {
                    constexpr bool oc = decltype(OC)::value;
                    hipLaunchKernelGGL((ntt_multiply_kernel<F, LOGN, MULT_MINW, false, oc>), grid, block, 0, A.stream, (char *)A.r0,
                                       (const char *)A.a0, (const char *)A.b0, limbs, A.L, 0u);
                    hipLaunchKernelGGL((ntt_multiply_kernel<F, LOGN, MULT_MINW, false, oc>), grid, block, 0, A.stream, (char *)A.r2,
                                       (const char *)A.a1, (const char *)A.b1, limbs, A.L, 0u);
                    hipLaunchKernelGGL((ntt_mac2_kernel<F, LOGN, MULT_MINW, oc>), grid, block, 0, A.stream, (char *)A.r1, (const char *)A.a0,
                                       (const char *)A.b1, (const char *)A.a1, (const char *)A.b0, limbs, A.L);
                }, out);
                return true;
            }
            break;
        // ---- key switch: r0, r1 containers ------------------------------------------------------------------------------------------
        case OP_FORM(LDS_KEYSWITCH, LDS_SPLIT):
            if constexpr (lds_keyswitch_split(EB, LOGN)) {
                if (in && !ac) break;
                with_bools([&](auto AC) { keyswitch1(std::true_type{}, std::false_type{}, AC); }, ac);
                return true;
            }
            break;
        case OP_FORM(LDS_KEYSWITCH, LDS_JOINT3):
            if constexpr (lds_keyswitch_joint3(EB, LOGN)) {
                with_bools([&](auto IN, auto AC) {
                    if constexpr (decltype(IN)::value || !decltype(AC)::value)
                        hipLaunchKernelGGL((ntt_keyswitch3_kernel<F, LOGN, 2, decltype(IN)::value, decltype(AC)::value>), grid, block, 0, A.stream, (char *)A.r0, (char *)A.r1,
                                           (const char *)A.c2, add0, add1, (const E *)A.kb, (const E *)A.ka, limbs, A.L, A.K, A.w);
                }, in, ac);
                return true;
            }
            break;
        case OP_FORM(LDS_KEYSWITCH, LDS_PAIRED):
            if constexpr (lds_paired_keyswitch(EB, LOGN)) {
                with_bools([&](auto IN, auto AC) {
                    if constexpr (decltype(IN)::value || !decltype(AC)::value)
                        hipLaunchKernelGGL((ntt_keyswitch2_kernel<F, LOGN, 2, decltype(IN)::value, decltype(AC)::value>), grid, block, 0, A.stream, (char *)A.r0, (char *)A.r1,
                                           (const char *)A.c2, add0, add1, (const E *)A.kb, (const E *)A.ka, limbs, A.L, A.K, A.w);
                }, in, ac);
                return true;
            }
            break;
        case OP_FORM(LDS_KEYSWITCH, LDS_SINGLE_LDS_TW):
            if constexpr (lds_twiddles_in_lds(EB, LOGN)) {
                if (in) break;
                keyswitch1(std::false_type{}, std::true_type{}, std::false_type{});
                return true;
            }
            break;
        case OP_FORM(LDS_KEYSWITCH, LDS_SINGLE_L2_TW):
            if constexpr (!lds_keyswitch_split(EB, LOGN)) {
                if (in) break;
                keyswitch1(std::false_type{}, std::false_type{}, std::false_type{});
                return true;
            }
            break;
        case OP_FORM(LDS_KEYSWITCH, LDS_PARTS16):    // few ciphertexts: one workgroup per DIGIT, then one per (ciphertext, limb, component) sums the partials
            if constexpr (lds_small_multiply(EB, LOGN)) return parts(ONE, std::false_type{}, dim3(Cfg16<LOGN>::T), LK, dim3(A.polys, 2));
            break;
        case OP_FORM(LDS_KEYSWITCH, LDS_PART_PAIRS):   // few ciphertexts: one workgroup per digit PAIR, then one per (ciphertext, limb) sums the partials
            if constexpr (lds_paired_keyswitch(EB, LOGN)) return parts(ONE, std::true_type{}, block, NP, grid);
            break;
        // ---- external product: rot0, rot1 = pre-rotated digit sources where given ---------------------------------------------------------
        case OP_FORM(LDS_EXTPROD, LDS_SPLIT):
            if constexpr (lds_keyswitch_split(EB, LOGN)) {
                if (in || out || prerot) break;
                extprod1(std::true_type{}, std::false_type{});
                return true;
            }
            break;
        case OP_FORM(LDS_EXTPROD, LDS_JOINT3):
            if constexpr (lds_keyswitch_joint3(EB, LOGN)) {
                if (!in && (out || prerot)) break;     // container input with compact output, or pre-rotated sources beside container input: never asked for
                with_bools([&](auto PR, auto IC, auto OC) {
                    if constexpr (decltype(IC)::value || !(decltype(OC)::value || decltype(PR)::value))
                        hipLaunchKernelGGL((ntt_extprod3_kernel<F, LOGN, 2, decltype(IC)::value, decltype(OC)::value, decltype(PR)::value>), grid, block, 0, A.stream, (char *)A.r0,
                                           (char *)A.r1, (const char *)A.a0, (const char *)A.a1, (const char *)A.rot0, (const char *)A.rot1, A.shifts, (const E *)A.kb,
                                           (const E *)A.ka, (const E *)A.kb1, (const E *)A.ka1, limbs, A.L, A.K, A.w);
                }, prerot, in, out);
                return true;
            }
            break;
        case OP_FORM(LDS_EXTPROD, LDS_PAIRED):
            if constexpr (lds_paired_extprod(EB, LOGN)) {
                if (prerot) break;
                with_bools([&](auto IC, auto OC) {
                    hipLaunchKernelGGL((ntt_extprod2_kernel<F, LOGN, 2, decltype(IC)::value, decltype(OC)::value>), grid, block, 0, A.stream, (char *)A.r0, (char *)A.r1,
                                       (const char *)A.a0, (const char *)A.a1, A.shifts, (const E *)A.kb, (const E *)A.ka, (const E *)A.kb1,
                                       (const E *)A.ka1, limbs, A.L, A.K, A.w);
                }, in, out);
                return true;
            }
            break;
        case OP_FORM(LDS_EXTPROD, LDS_SINGLE_LDS_TW):
            if constexpr (lds_twiddles_in_lds(EB, LOGN)) {
                if (in || out || prerot) break;
                extprod1(std::false_type{}, std::true_type{});
                return true;
            }
            break;
        case OP_FORM(LDS_EXTPROD, LDS_SINGLE_L2_TW):
            if constexpr (!lds_keyswitch_split(EB, LOGN)) {
                if (in || out || prerot) break;
                extprod1(std::false_type{}, std::false_type{});
                return true;
            }
            break;
        // few accumulators: the key-switch launches above with two digit sources -- the pre-rotated components rot0, rot1 with their RGSW rows --
        // and the accumulator pair a0, a1 as addends; r0, r1 compact or containers
        case OP_FORM(LDS_EXTPROD, LDS_PARTS16):
            if constexpr (lds_small_multiply(EB, LOGN)) {
                if (in && prerot) return parts(TWO, std::false_type{}, dim3(Cfg16<LOGN>::T), LK, dim3(A.polys, 2));
            }
            break;
        case OP_FORM(LDS_EXTPROD, LDS_PART_PAIRS):   // one workgroup per digit PAIR of a component (paired 32-per-thread transform), paired combining launch
            if constexpr (lds_paired_extprod(EB, LOGN) && !lds_small_multiply(EB, LOGN)) {
                if (in && prerot) return parts(TWO, std::true_type{}, block, NP, grid);
            }
            break;
        default: break;
    }
    return false;
}

bool CAT(lds_launch_, FHE_FIELD, FHE_LOGN)(const LdsArgs &A) { return launch<FHE_FIELD, FHE_LOGN>(A); }

}  // namespace fhe_dev
