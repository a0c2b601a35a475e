// lds_launch.h -- host-side launch table for the LDS-resident kernels (one translation unit per (field, log2 n) instance so the
// instances compile in parallel): the ops and forms with their names, where each form exists, and LdsArgs, the one launch request --
// operands named by role, one layout flag per role.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fhe_dev {

// One list per enum: the enumerators and the names that the "no LDS kernel for ..." error prints come out of the same lines.
// LDS_HOIST / LDS_HOIST_APPLY: hoisted rotations (hoist.hip.h), one form each.  LDS_HOIST_FWD / LDS_HOIST_LINCOMB: the two launches of the
// hoisted linear transform (hoist_lincomb.hip.h), one form each.  LDS_ENCRYPT: public-key encryption with in-kernel sampling (encrypt.hip.h),
// one kernel on two grids (LdsArgs::per_ct).  LDS_DECRYPT: the first launch of secret-key decryption (decrypt.hip.h), one form.
// LDS_KEYGEN: key-switching key generation with in-kernel sampling (keygen.hip.h), one form.  LDS_RGSW_KEYGEN: its sibling for RGSW rows
// (the gadget term is mu or mu s instead of a Galois target), one form, wherever LDS_KEYGEN exists.
// LDS_SLOTS_ENCODE / LDS_SLOTS_DECODE: the batch encoder (encode.hip.h), one form each, on the instance of the PLAINTEXT modulus' field.
// The last five: transforms beyond the LDS range (N = 2^(13 + top), top = 1..3; served by the LOGN = 13 instances): the register-only pass
// over the top stages and the sub-transforms of the 2^top blocks
#define LDS_OPS(X) X(LDS_FORWARD, "forward") X(LDS_INVERSE, "inverse") X(LDS_MULTIPLY, "multiply") X(LDS_CT_MULTIPLY, "tensor product") \
    X(LDS_KEYSWITCH, "key switch") X(LDS_EXTPROD, "external product") X(LDS_HOIST, "hoist") X(LDS_HOIST_APPLY, "hoisted rotation") \
    X(LDS_HOIST_FWD, "hoist-order forward") X(LDS_HOIST_LINCOMB, "hoisted linear transform") X(LDS_ENCRYPT, "encryption") X(LDS_DECRYPT, "decryption") X(LDS_KEYGEN, "key generation") X(LDS_RGSW_KEYGEN, "RGSW key generation") \
    X(LDS_SLOTS_ENCODE, "slot encoding") X(LDS_SLOTS_DECODE, "slot decoding") \
    X(LDS_PASS_FWD, "pass forward") X(LDS_PASS_INV, "pass inverse") X(LDS_SUB_FORWARD, "sub forward") X(LDS_SUB_INVERSE, "sub inverse") X(LDS_SUB_MULTIPLY, "sub multiply")
#define LDS_ENUMERATOR(id, name) id,
#define LDS_NAME_CASE(id, name) case id: return name;
enum LdsOp { LDS_OPS(LDS_ENUMERATOR) };
constexpr const char *lds_op_name(int op) { switch (op) { LDS_OPS(LDS_NAME_CASE) } return "unknown"; }

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

// hoisted rotations (ntt_hoist_kernel / ntt_hoist_apply_kernel: two and three live arrays): every LDS-resident size but N = 2^15, whose
// 1024-thread workgroups cap a thread at 128 VGPRs (the apply kernel parks 84 bytes per lane in scratch there): that size takes the composed path
constexpr bool lds_hoist(int elem_bytes, int log_n) { (void)elem_bytes; return log_n <= 14; }
// hoisted linear transform (ntt_hoist_fwd_kernel / ntt_hoist_lincomb_kernel): 4-byte residues one workgroup per (ciphertext, limb) with five live
// arrays, 8-byte residues one per (ciphertext, limb, output component) with three; wherever the hoist kernels exist and the instance keeps
// the budget of its field (tests/test_linear_transform.py compiles every LDS-resident instance and pins it)
constexpr bool lds_hoist_lincomb(int elem_bytes, int log_n) { return lds_hoist(elem_bytes, log_n); }
constexpr bool lds_hoist_lincomb_split(int elem_bytes) { return elem_bytes == 8; }
// public-key encryption with in-kernel sampling (ntt_encrypt_kernel: two live arrays and 34 registers of packed samples): every LDS-resident
// size but N = 2^15, whose 1024-thread workgroups cap a thread at 128 VGPRs (tests/test_encrypt.py compiles every instance and pins the
// budgets; that size takes the composed path)
constexpr bool lds_encrypt(int elem_bytes, int log_n) { (void)elem_bytes; return log_n <= 14; }
// secret-key decryption, first launch (ntt_decrypt_kernel: two live arrays): every LDS-resident size but N = 2^15, whose 1024-thread
// workgroups cap a thread at 128 VGPRs (the kernel parks 176 bytes per lane in scratch there): that size takes the composed path
// (tests/test_decrypt.py compiles every instance and pins the budgets: no scratch anywhere)
constexpr bool lds_decrypt(int elem_bytes, int log_n) { (void)elem_bytes; return log_n <= 14; }
// key-switching key generation (ntt_keygen_kernel: one live array, every draw in registers): the sizes of the encryption and decryption
// kernels; N = 2^15 takes the composed path like them (tests/test_keygen.py compiles every instance and pins the budgets: no scratch anywhere)
constexpr bool lds_keygen(int elem_bytes, int log_n) { (void)elem_bytes; return log_n <= 14; }
// batch encoder (ntt_slots_encode_kernel / ntt_slots_decode_kernel: one live array, no scratch anywhere): the sizes of the encryption,
// decryption and key-generation kernels, which it feeds and drains; N = 2^15 takes the composed path like them (tests/test_batch_encoder.py
// compiles every instance and pins the budgets)
constexpr bool lds_slots(int elem_bytes, int log_n) { (void)elem_bytes; return log_n <= 14; }
// entries of a cumulative Gaussian table the kernel stages in its exchange buffer (8 KiB: the buffer of the smallest instance; searched with cdt_count, ctr_rand.hip.h); larger
// tables (sigma > 85) take the composed path
constexpr uint32_t ENCRYPT_MAX_CDT = 1024;

// The kernel form of LDS_MULTIPLY / LDS_CT_MULTIPLY / LDS_KEYSWITCH / LDS_EXTPROD (the other ops have one form each).
#define LDS_FORMS(X) /* LDS_MULTIPLY, LDS_CT_MULTIPLY */ \
    X(LDS_ONE_LAUNCH, "one-launch")              /* one workgroup per limb polynomial, one launch */ \
    X(LDS_SQUARE, "square")                      /* the same with b == a: the squaring kernels (container outputs) */ \
    X(LDS_SMALL16, "16-per-thread")              /* few polynomials: the 16-per-thread latency kernels (tensor product: compact outputs) */ \
    X(LDS_COOP4, "four-workgroup")               /* a handful: four workgroups per limb polynomial, three launches, ws = 3 (multiply) / 7 (tensor product) compact polynomials per limb polynomial */ \
    X(LDS_TWO_LAUNCH, "two-launch")              /* tensor product: NTT(b0), NTT(b1) into ws (2 compact polynomials per limb polynomial), then the rest */ \
    X(LDS_THREE_LAUNCH, "three-launch")          /* tensor product where the one-launch kernel does not exist and no workspace is wanted */ \
    /* LDS_KEYSWITCH, LDS_EXTPROD */ \
    X(LDS_SPLIT, "split")                        /* two workgroups per (ciphertext, limb), one per key half */ \
    X(LDS_JOINT3, "three-array")                 /* one workgroup per limb, three live arrays */ \
    X(LDS_PAIRED, "paired")                      /* one workgroup per (ciphertext, limb), digit transforms two at a time */ \
    X(LDS_SINGLE_LDS_TW, "single (LDS twiddles)")   /* one workgroup per (ciphertext, limb), one digit transform at a time, twiddles in LDS */ \
    X(LDS_SINGLE_L2_TW, "single (L2 twiddles)")  /* ... twiddles read through L2 */ \
    X(LDS_PARTS16, "per-digit parts")            /* one workgroup per digit (16-per-thread transforms) + a combining launch, ws = partial sums */ \
    X(LDS_PART_PAIRS, "per-digit-pair parts")    /* one workgroup per digit PAIR (paired transforms) + a combining launch, ws = partial sums */
enum LdsForm { LDS_FORMS(LDS_ENUMERATOR) };
constexpr const char *lds_form_name(int form) { switch (form) { LDS_FORMS(LDS_NAME_CASE) } return "unknown"; }

// One term of a hoisted linear transform (device table owned by the fhe_linear_transform object, read by ntt_hoist_lincomb_kernel).
// kb == nullptr: no key switch, the term is p * (c0, c1)
struct LincombTerm {
    const void *kb, *ka;                 // packed key tables of the term's key set (pack_rows, keys.hip)
    const void *pt;                      // the term's plaintext, transformed and packed like one key row: [L][n] residues
    uint32_t g, _pad;                    // Galois element (1 for a keyless term)
};

// One key set of a key-generation call (device table read by ntt_keygen_kernel): the set's packed tables and its Galois element
// (0: the relinearisation key, target s^2)
struct KeygenSet {
    void *kb, *ka;
    uint32_t g, _pad;
};

// One half of an RGSW ciphertext of an RGSW key-generation call (device table read by ntt_rgsw_keygen_kernel): the packed tables of the
// component's rows, the message and the component (0: gadget term mu, 1: mu s)
struct RgswSet {
    void *kb, *ka;
    int32_t mu; uint32_t comp;
};

// One launch request.  The host fills the members that are operands of ITS op, by name (lds_args of engine.h sets the common ones from the
// engine and the plan); everything else keeps its default.
struct LdsArgs {
    int op = LDS_FORWARD, form = LDS_ONE_LAUNCH;
    void *r0 = nullptr, *r1 = nullptr, *r2 = nullptr;   // outputs (forward / inverse: r0 is the in-place buffer; pass / sub: r0 = dst)
    const void *a0 = nullptr, *a1 = nullptr, *b0 = nullptr, *b1 = nullptr;   // inputs of multiply / tensor product (pass / sub: a0 = src, b0 = second operand)
    // LDS_KEYSWITCH: r0 = add0 + c2 x kb, r1 = add1 + c2 x ka (no addends given: r0, r1 are accumulated in place)
    const void *c2 = nullptr, *add0 = nullptr, *add1 = nullptr;
    // LDS_EXTPROD (fused blind-rotation step): (r0, r1) = (a0, a1) + ExtProd((X^shift - 1) (a0, a1)); kb / ka = rows of component 0, kb1 / ka1 = rows
    // of component 1; rot0, rot1 = (X^shift - 1) (a0, a1) where the loop pre-rotated them (always compact), else nullptr
    const void *rot0 = nullptr, *rot1 = nullptr;
    const void *limbs = nullptr;         // device array of Limb<F>
    uint32_t L = 0, polys = 0;
    hipStream_t stream = nullptr;
    // Layout: compact polynomials (sizeof(residue) bytes per coefficient) instead of 32-byte containers.  Set by the host, from the plan,
    // for every op; the instance never derives a layout from a pointer and refuses a combination it has no kernel for.
    bool in_compact = false;             // what the workgroups transform: a0, a1, b0, b1 (LDS_EXTPROD: the accumulator pair a0, a1, which is its own
                                         // addend; pass / sub: the source a0, b0); LDS_KEYSWITCH: the digit source c2
    bool add_compact = false;            // LDS_KEYSWITCH: the addends add0, add1 (given, and beside a compact digit source only)
    bool out_compact = false;            // every output r0, r1, r2
    void *ws = nullptr;                  // the form's workspace (LdsForm)
    const void *kb = nullptr, *ka = nullptr, *kb1 = nullptr, *ka1 = nullptr;   // packed key tables / RGSW rows
    // LDS_HOIST: r0 = the hoist workspace, c2 = c1 (compact).  LDS_HOIST_APPLY: (r0, r1) = (add0, 0) + the kept polynomials of c2 = the hoist
    // workspace, read at pi_galois, times kb / ka; add0 = sigma_galois(c0), compact
    uint32_t galois = 0;
    // LDS_HOIST_FWD: r0 = [a1 ? 2 : 1][polys][n] residues = the forward transforms of a0 (and a1), containers in, canonical, hoist layout.
    // LDS_HOIST_LINCOMB: (r0, r1) = sum over the num_terms entries of `terms` (device array of LincombTerm) of plaintext * rotation; c2 = the
    // hoist workspace, add0 / add1 = the two halves LDS_HOIST_FWD wrote (add1 only where a term has no key); polys = ciphertexts x limbs
    const void *terms = nullptr;
    uint32_t num_terms = 0;
    // LDS_ENCRYPT: (r0, r1) = (kb, ka) (*) u + t (e0, e1) + (a0, 0): kb / ka = the packed transformed public key ([L][n] residues each), a0 = m
    // (containers) or nullptr, polys = ciphertexts x limbs; per_ct: one workgroup per ciphertext looping over its limbs, else one per (ciphertext, limb)
    const uint64_t *cdt = nullptr;       // device cumulative table of the Gaussian (cdt_len <= ENCRYPT_MAX_CDT entries)
    uint32_t cdt_len = 0;
    uint64_t seeds[3] = {0, 0, 0}, t = 0;
    bool per_ct = false;
    // LDS_DECRYPT: r0 = the decryption workspace ([polys][n] residues, compact) = a0 + a1 (*) s + c2 (*) s^2 limb-wise; a0, a1 = c0, c1 and c2 = c2 or
    // nullptr (containers); kb / ka = the packed transformed s and s^2 ([L][n] residues each); polys = ciphertexts x limbs, out_compact set
    // LDS_KEYGEN: a0 = KeygenSet[polys / (L K L)] (device): both packed tables of every set are written; kb / ka = the packed transformed s and s^2;
    // cdt / cdt_len as LDS_ENCRYPT; seeds[0], seeds[1] = the streams of a and e; t = the noise scale; polys = sets x rows x limbs
    // LDS_RGSW_KEYGEN: as LDS_KEYGEN with a0 = RgswSet[polys / (L K L)] (device) and kb = the packed transformed s alone
    // LDS_SLOTS_ENCODE: r0 = [polys][L][n] containers = the plaintexts of a0 = [polys][n] slot values (8-byte words: in_compact set); kb = the
    // position -> slot table (uint32_t[n]), ka = ModT[L], the reduction modulo the target's q_l (t == 0: none); limbs = the ONE limb of the
    // encoder's engine on (n, t); L = limbs of the TARGET engine; polys = plaintexts
    // LDS_SLOTS_DECODE: r0 = [polys][n] slot values (8-byte words: out_compact set) of a0 = [polys][n] 8-byte words (in_compact) or limb 0 of
    // [polys][L][n] containers; kb, limbs, L, polys as for LDS_SLOTS_ENCODE.  r0 == a0 is allowed for 8-byte words
    const uint32_t *shifts = nullptr;    // LDS_EXTPROD: device array of per-ciphertext monomial exponents
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
