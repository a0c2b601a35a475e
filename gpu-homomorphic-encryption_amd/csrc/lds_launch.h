// lds_launch.h -- host-side launch table for the LDS-resident kernels (one translation unit per
// (field, log2 n) instance so the instances compile in parallel).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fhe_dev {

enum LdsOp { LDS_FORWARD = 0, LDS_INVERSE = 1, LDS_MULTIPLY = 2, LDS_CT_MULTIPLY = 3, LDS_KEYSWITCH = 4, LDS_EXTPROD = 5,
             // transforms beyond the LDS range (N = 2^(13 + top), top = 1..3; served by the LOGN = 13 instances): the register-only pass over
             // the top stages (r0 = dst, a0 = src) and the sub-transforms of the 2^top blocks (r0 = dst, a0 = src, b0 = second operand)
             LDS_PASS_FWD = 6, LDS_PASS_INV = 7, LDS_SUB_FORWARD = 8, LDS_SUB_INVERSE = 9, LDS_SUB_MULTIPLY = 10 };

// Which kernel form runs an op is decided on the host, once, by the planner of transforms.hip (plan_*), which also says which library workspace
// the form needs; the instance launches exactly that form or returns false.  The predicates below say where a form exists.

// the tensor product as one fused launch (LDS_ONE_LAUNCH / LDS_SQUARE); elsewhere the two-launch form (NTT(b0), NTT(b1) into the compact
// workspace, then everything else; 7 transforms) or, without a workspace (testing aid FHE_HIP_NO_TWO_LAUNCH_CT=1), the three-launch form:
// multiply(c0), multiply(c2) and the two-product kernel for c1 (11 transforms)
constexpr bool lds_ct_fused(int elem_bytes, int log_n) { return elem_bytes == 4 ? log_n <= 14 : log_n <= 13; }   // 1024-thread blocks cap a thread at 128 VGPRs
// the two-launch form exists wherever the one-launch kernel does not, and for every size of the 8-byte residues (whose one-launch
// kernel holds four 64-register arrays and parks 1.1-1.3 KB per lane in scratch when it writes containers)
constexpr bool lds_ct_two_launch(int elem_bytes, int log_n) { return elem_bytes == 8 || !lds_ct_fused(elem_bytes, log_n); }
// key switching: 4-byte residues run one workgroup per (ciphertext, limb); 8-byte residues and 1024-thread blocks (N = 2^15)
// two, one per key half (three live arrays instead of four)
constexpr bool lds_keyswitch_split(int elem_bytes, int log_n) { return elem_bytes == 8 || log_n >= 15; }
// ... or ONE workgroup per limb with both accumulators and the digit polynomial live (LDS_JOINT3: ntt_keyswitch3_kernel / ntt_extprod3_kernel:
// half the transforms, ~450-660 bytes per lane parked in scratch at N = 2^14), which exists for every LDS-resident size of the 8-byte residues
// and for 4-byte residues at N = 2^15 (1024-thread workgroups capped at 128 VGPRs: relinearisation +38 %, blind rotation +48 % over the split form)
constexpr bool lds_keyswitch_joint3(int elem_bytes, int log_n) { return (elem_bytes == 8 && log_n <= 14) || (elem_bytes == 4 && log_n == 15); }
// key switching / external product in the one-workgroup-per-limb form: twiddle tables copied into LDS for 4-byte residues up
// to N = 2^13 (exchange buffer + table = 65 KiB per workgroup, still two workgroups per CU).  Interleaved A/B on one MI355X
// (scripts/bench_ab_twiddles.sh): external product N = 8192 +7 %, relinearisation N = 8192 +-0 %; at N = 2^14 (130 KiB, one
// workgroup per CU) it was 1-6 % slower, so that size keeps reading twiddles through L2.
constexpr bool lds_twiddles_in_lds(int elem_bytes, int log_n) { return elem_bytes == 4 && log_n <= 13; }

// key switching / external product with the digit transforms done two at a time (ntt_keyswitch2_kernel / ntt_extprod2_kernel;
// two exchange buffers: 66 KiB at N = 2^13, 132 KiB at N = 2^14) and the two products of a pair sharing one Montgomery reduction.
// Interleaved A/B on one MI355X (scripts/bench_ab_paired.sh) against the one-at-a-time kernels (with LDS twiddles up to N = 2^13):
// relinearisation +7.5 % at N = 8192 and +17 % at N = 16384; external product +7 % at N = 8192, +13 % at N = 16384, +3.5 % at N = 4096.
constexpr bool lds_paired_keyswitch(int elem_bytes, int log_n) { return elem_bytes == 4 && log_n <= 14; }
constexpr bool lds_paired_extprod(int elem_bytes, int log_n) { return elem_bytes == 4 && log_n <= 14; }

// LDS_SMALL16 (few polynomials: batch x limbs below the CU count): the 16-per-thread latency kernels of ntt_lds_small.hip.h --
// multiply, tensor product, and the key-switch parts (LDS_PARTS16); 4-byte residues only (its 90 preloaded 4-byte twiddles fit the register file, 8-byte ones do not)
// (N = 2^14 would be 1024 threads under the 128-VGPR cap: the preloaded twiddles spill 51-163 VGPRs there, so that size keeps the 32-per-thread kernels)
constexpr bool lds_small_multiply(int elem_bytes, int log_n) { return elem_bytes == 4 && log_n <= 13; }
// ... and for a handful of polynomials one polynomial over four workgroups (LDS_COOP4: ntt_multiply4_* / ntt_ct4_* kernels)
constexpr bool lds_coop4_multiply(int elem_bytes, int log_n) { return elem_bytes == 4 && (log_n == 13 || log_n == 14); }

// The kernel form of LDS_MULTIPLY / LDS_CT_MULTIPLY / LDS_KEYSWITCH / LDS_EXTPROD (the other ops have one form each).
enum LdsForm {
    // LDS_MULTIPLY, LDS_CT_MULTIPLY
    LDS_ONE_LAUNCH = 0,                  // one workgroup per limb polynomial, one launch
    LDS_SQUARE,                          // the same with b == a: the squaring kernels (container outputs)
    LDS_SMALL16,                         // few polynomials: the 16-per-thread latency kernels (tensor product: compact outputs)
    LDS_COOP4,                           // a handful: four workgroups per limb polynomial, three launches, ws = 3 (multiply) / 7 (tensor product) compact polynomials per limb polynomial
    LDS_TWO_LAUNCH,                      // tensor product: NTT(b0), NTT(b1) into ws (2 compact polynomials per limb polynomial), then the rest
    LDS_THREE_LAUNCH,                    // tensor product where the one-launch kernel does not exist and no workspace is wanted
    // LDS_KEYSWITCH, LDS_EXTPROD
    LDS_SPLIT,                           // two workgroups per (ciphertext, limb), one per key half
    LDS_JOINT3,                          // one workgroup per limb, three live arrays
    LDS_PAIRED,                          // one workgroup per (ciphertext, limb), digit transforms two at a time
    LDS_SINGLE_LDS_TW,                   // one workgroup per (ciphertext, limb), one digit transform at a time, twiddles in LDS
    LDS_SINGLE_L2_TW,                    // ... twiddles read through L2
    LDS_PARTS16,                         // one workgroup per digit (16-per-thread transforms) + a combining launch, ws = partial sums
    LDS_PART_PAIRS,                      // one workgroup per digit PAIR (paired transforms) + a combining launch, ws = partial sums
};

struct LdsArgs {
    int op, form;
    void *r0, *r1, *r2;                  // outputs (forward / inverse: r0 is the in-place buffer)
    const void *a0, *a1, *b0, *b1;       // inputs
    const void *limbs;                   // device array of Limb<F>
    uint32_t L, polys;
    hipStream_t stream;
    // layout: compact polynomials (sizeof(residue) bytes per coefficient) instead of 32-byte containers
    bool in_compact = false;             // every input a0, a1, b0, b1 is compact
    bool out_compact = false;            // every output r0, r1, r2 is compact
    void *ws = nullptr;                  // the form's workspace (LdsForm)
    // LDS_KEYSWITCH: r0 += c2 x kb, r1 += c2 x ka with c2 = a0; a1, b0 = addends of r0, r1 (nullptr: r0, r1 are accumulated in place)
    // LDS_EXTPROD (fused blind-rotation step): (r0, r1) = (a0, a1) + ExtProd((X^shift - 1) (a0, a1)); kb / ka = rows of component 0,
    // kb1 / ka1 = rows of component 1, shifts = device array of per-ciphertext monomial exponents; b0, b1 = (X^shift - 1) (a0, a1) when the
    // host pre-rotated them (compact), else nullptr
    const void *kb = nullptr, *ka = nullptr, *kb1 = nullptr, *ka1 = nullptr;
    const uint32_t *shifts = nullptr;
    uint32_t K = 0, w = 0;
    uint32_t b_polys = 0;                // LDS_MULTIPLY: polynomials behind b0 (0 = as many as the batch; L = one RNS polynomial broadcast over the batch)
    uint32_t top = 0;                    // LDS_PASS_* / LDS_SUB_*: number of stages above the 2^13 blocks (log2 n = 13 + top)
    bool rconst = false;                 // LDS_PASS_INV: scale with the constants that also absorb the 2^-W of a fused pointwise product
};

// false (and nothing launched) when this instance has no such (op, form, layout)
typedef bool (*lds_launch_fn)(const LdsArgs &);

// width: 32, 52, 64 or 65 (= F64X, full-range 64-bit).  nullptr when the instance does not exist.
lds_launch_fn lds_lookup(int width, int log_n);

}  // namespace fhe_dev
