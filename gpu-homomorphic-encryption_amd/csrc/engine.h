// engine.h -- what the host sources of the C ABI (include/fhe_hip.h) share: the engine and key-set structs, error plumbing, the
// width-class -> field-type and limb-table dispatch, the shared argument checks, the workspace table, and the few entry points one subsystem
// offers the others.  Internal: nothing declared here is exported from the library.  Which source owns what:
//   core.hip        last error, device / memory entry points, host number theory, timers
//   literal.hip     the reference's single-modulus kernels as written (ntt256_literal.hip.h)
//   sampling.hip    samplers, modulus switch, negacyclic fold (sampling.hip.h)
//   keys.hip        the lifetime of every key object: import, export and destruction of key sets, secret keys, public keys; packing rows into
//                   the register order of the fused kernels and back (the pack / unpack kernels of ntt_word.hip.h)
//   encrypt.hip     public-key encryption (composed path: the entry points of sampling.hip and transforms.hip with the small kernel of encrypt.hip; fused: encrypt.hip.h)
//   decrypt.hip     secret-key decryption (fused: decrypt.hip.h; composed path: the entry points of transforms.hip; the CRT kernels of decrypt.hip.h either way)
//   engine.hip      engine lifetime, width-class choice, environment switches, limb tables, workspaces, reserve (= the merge of need_* below)
//   transforms.hip  wide and LDS launchers, the planners, forward / inverse / element-wise / multiply / tensor product (ntt_wide.hip.h,
//                   ntt256_transforms.hip.h; ew / compact / check kernels of ntt_word.hip.h)
//   keyswitch.hip   relinearisation, multiply + relinearise, Galois, hoisting, linear transform, blind rotation (galois.hip.h, ntt256_keyswitch.hip.h;
//                   digit / monomial kernels of ntt_word.hip.h)
//   keygen.hip      key-switching key generation (fused: keygen.hip.h; composed path: the entry points of transforms.hip, sampling.hip, keyswitch.hip
//                   and keys.hip with the small kernels of keygen.hip)
//   encode.hip      batch encoder: slots <-> plaintexts (fused: encode.hip.h on the engine of the plaintext modulus; composed path: the small
//                   kernels of encode.hip.h around do_inverse / do_forward)
//   bootstrap.hip   around the blind-rotation loop: LWE ciphertexts -> accumulators and shift table, sample extraction (bootstrap.hip.h); the RGSW
//                   rows of the loop come from keygen.hip (fhe_rgsw_keys_generate)
//   lwe_keyswitch.hip  after the loop: the LWE key-switching key (its one key object, import / export / generation) and the key switch of an
//                   extracted sample back to the small LWE key, with the optional modulus switch (lwe_keyswitch.hip.h)
//   lwe_pack.hip    the way back: LWE samples under the ring key into one RLWE ciphertext, merge levels and trace around fhe_ct_apply_galois
//                   (lwe_pack.hip.h)
//   rns.hip         CRT tables, to / from RNS, rescale, BGV modulus switch, base conversion (ntt256_rns.hip.h; conversion kernels of ntt_word.hip.h)
//   bfv.hip         BFV multiplication: the multiplier object (an owned engine on Q u P, the conversion tables, one workspace), centred lift,
//                   scale-and-round, the one-call product around do_ct_multiply and fhe_ct_relinearize (bfv.hip.h)
// Every kernel (template instantiations included) is launched, and therefore compiled, by its owning source only.
// What they share is written once, here: overlaps (the byte-range test), with_word_field / with_limbs (width class -> field type / typed limb
// table), word_operand / inv_mod_u64 (the constants of the streaming conversion kernels), check_word_call and check_count (the engine and (count, batch) rules of the entry points around the blind rotation), and the
// workspace table (WsId, Workspace, grow_ws).
#pragma once
#include "../../include/fhe_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "host_math.hpp"
#include "lds_launch.h"
#include "ntt256.hip.h"
#include "ntt_field.hip.h"

#pragma GCC visibility push(hidden)

using fhe_host::U256;

// ---- error plumbing (core.hip) ------------------------------------------------------------------------------------------------
int fail(int code, const std::string &msg);              // records the thread's last error, returns code
int ensure_device();
int post_launch(hipStream_t s, const char *what);        // launch error of the call (FHE_HIP_SYNC=1: and of the kernel, after a stream sync)

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(FHE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));           \
    } while (0)

// Every d_* container pointer of the ABI: 16-byte aligned (the kernels load and store containers as 16-byte halves; include/fhe_hip.h,
// Conventions).  Null pointers pass: the null checks beside each call of this report those.
inline int check_aligned(std::initializer_list<const void *> ptrs, const char *what) {
    for (const void *p : ptrs)
        if ((uintptr_t)p & 15) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": container pointers must be 16-byte aligned");
    return FHE_OK;
}

// whether the byte ranges [a, a + na) and [b, b + nb) share a byte: the range test of the entry points that take one
inline bool overlaps(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

inline fhe_dev::u256 to_dev(const uint64_t q[4]) { fhe_dev::u256 r; std::memcpy(r.l, q, 32); return r; }

inline unsigned ew_grid(size_t items) {
    size_t blocks = (items + 255) / 256;
    return (unsigned)(blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks));   // grid-stride above 8192 blocks
}

// ---- engine handle ------------------------------------------------------------------------------------------------------------
// Environment switches, read once at engine creation (read_env, engine.hip)
struct EngineEnv {
    int force_width = 0;
    bool no_wide_lazy = false, no_wide_tiles = false;
    bool no_fused_keygen = false;
    bool no_square = false, single_transforms = false, global_twiddles = false, no_fused_keyswitch = false, no_word_conversions = false,
         no_fused_blind_rotate = false, no_fused_ct_relin = false, no_compact_blind_rotate = false, no_two_launch_ct = false, no_fused_galois = false, no_fused_hoist = false, no_fused_encrypt = false, no_fused_decrypt = false, no_fused_encode = false,
         split_keyswitch = false, relin_chunks_forced = false, no_prerotation = false, no_c2_compaction = false, check_inputs = false;
    uint32_t small_batch_polys = 256, coop_polys = 64, split_pairs_polys = 128, overlap_chunks = 4;
    uint32_t encrypt_per_ct_batch = 256; // fhe_ct_encrypt of at least this many ciphertexts runs one workgroup per ciphertext (plan_encrypt)
    int ct_form_force = 0;
};

// Library-owned workspaces, per engine, grown on demand by grow_ws (never while the engine's stream is capturing) and freed with the engine.
// This table is the one place that names them: destroy_impl and fhe_rns_ntt_workspace_bytes loop over it.
enum WsId {
    WS1,        // general paths (the reference mallocs/frees per multiply, src/ntt.cu:51-74) and the transformed b-side of the two-launch tensor product
    WS2,        // c0, c1, c2 of the fused multiply + relinearise (compact or containers) and the compact accumulators of a blind-rotation loop;
                // separate from WS1, which the general paths use
    WS3,        // compact polynomials between the two launches of a two-pass transform (sub_top != 0: N beyond the LDS range)
    WS_HOIST,   // hoisted rotations: the transformed digit polynomials of the c1 of the last fhe_ct_hoist; no other entry point touches it
    WS_LIN,     // hoisted linear transform.  Fused path: c0^ (and c1^) of the call in the hoist layout; composed path: the two components of
                // one weighted rotation before they are added to the outputs
    WS_ENC,     // fhe_ct_encrypt, composed path: u of the call as containers
    WS_DEC,     // fhe_ct_decrypt.  Fused path: the residues of c0 + c1 s + c2 s^2 as compact polynomials between the two launches; composed
                // path: c1 s (and c2 s^2) as containers
    WS_PACK,    // fhe_lwe_pack.  Fused path: three regions that rotate as (P, G, free) over the merge levels; composed path: the embedded
                // ciphertexts and the operands of one level as containers
    WS_COUNT
};
// whether fhe_rns_ntt_workspace_bytes counts it: all but the hoist buffer, which fhe_rns_ntt_hoist_bytes reports on its own
constexpr bool ws_in_workspace_bytes(int id) { return id != WS_HOIST; }
struct Workspace { void *p = nullptr; size_t bytes = 0; };   // one grow-on-demand device allocation (the encoder objects' scratch too)

struct fhe_rns_ntt {
    int device = 0;
    uint32_t n = 0, log_n = 0, L = 0;
    int width = 0;
    size_t residue_bytes = 8; int lds_id = 65;   // of the word-sized class's field (set at creation through with_word_field): bytes of a compact residue, id of its instances in lds_table.cpp
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipStream_t aux_stream = nullptr;   // second stream of the overlapped one-call multiply (fork / join with events around it)
    hipEvent_t ev_chunk[16] = {}, ev_join = nullptr;   // tensor product of chunk i done (engine stream) -> key switch of chunk i may start (second stream)
    EngineEnv env;
    uint32_t max_digits = 0, max_composed_digits = 0;   // largest digit count K of the key sets imported on this engine / of those without packed tables (fhe_rns_ntt_reserve)
    void *d_limbs = nullptr;            // owned by d_tables
    void *d_wlimbs = nullptr;           // FHE_WIDTH_256: WLimb<wide_nl>[L] for the NTT kernels of ntt_wide.hip.h (owned by d_tables)
    uint32_t sub_top = 0;               // word-sized classes beyond the LDS range: log2 n = 13 + sub_top (two-pass transforms), else 0
    int wide_nl = 0;                    // FHE_WIDTH_256: 64-bit limbs per residue in those kernels (2: q < 2^127, 4: q < 2^255)
    bool wide_lazy = false;             // FHE_WIDTH_256: every modulus below 2^(64 wide_nl - 6): the lazy tile kernels (unless FHE_HIP_NO_WIDE_LAZY)
    std::vector<void *> d_tables;
    Workspace ws[WS_COUNT];             // the library-owned workspaces (the table above)
    struct { bool valid = false, fused = false; uint32_t w = 0, K = 0, batch = 0; } hoist;   // what WS_HOIST holds: digit width, digits per limb, ciphertexts
    uint32_t *d_flag = nullptr;
    std::vector<U256> moduli;
    void *d_crt = nullptr;               // CrtLimb[L], built on first use of to_rns / from_rns (owned by d_tables)
    void *d_rescale = nullptr;           // RescaleLimb[L-1], built on first use of rescale_drop_last (owned by d_tables)
    void *d_bconv = nullptr;             // ((Q/q_i) mod p_j) * R_j for the most recent base-conversion target (owned by d_tables)
    const void *bconv_target = nullptr;
    void *d_rescale_w = nullptr;         // word-sized classes: (q_last^-1 mod q_l) as pw operands, E[L-1] (owned by d_tables)
    void *d_bconv_w_minv = nullptr, *d_bconv_w_mat = nullptr;   // word-sized classes: base-conversion operands for bconv_w_target
    const void *bconv_w_target = nullptr;
    std::vector<U256> bconv_moduli, bconv_w_moduli;   // the target bases the cached matrices were built for (a handle address can be re-used)
    // fhe_ct_mod_switch_drop_last: the constant tables depend on t; one entry per t seen (ModSwitchLimb[L], or E[2L - 1] on the word-sized
    // kernels; owned by d_tables).  A call with a t that has an entry allocates nothing.
    std::vector<std::pair<uint64_t, void *>> mod_switch_tables;
    void *d_from_rns_w_minv = nullptr, *d_from_rns_w_M = nullptr;   // integer word classes: CRT operands and Q / q_l (owned by d_tables)
    void *d_to_rns_w = nullptr;          // integer word classes: 2^(W k) mod q_l as pw operands, E[L][256 / W] (owned by d_tables)
    fhe_dev::CrtBig crt_big;
    int crt_state = 0;                   // 0 = not built, 1 = ready, -1 = Q too large for from_rns (to_rns still fine)
    double cdt_sigma = 0; uint64_t *d_cdt = nullptr; uint32_t cdt_len = 0;   // cumulative table of the last Gaussian sampler call
};
struct fhe_ntt { fhe_rns_ntt *impl; };

struct fhe_relin_keys {
    fhe_rns_ntt *owner = nullptr;
    uint32_t decomp_bits = 0, K = 0, num_keys = 0;
    void *d_kb = nullptr, *d_ka = nullptr;      // [num_keys][L][n] containers, NTT domain, canonical
    void *d_pkb = nullptr, *d_pka = nullptr;    // packed tables for the fused key-switch kernel (word-sized paths)
};

struct fhe_secret_key {                             // keys.hip; decrypt.hip and keygen.hip read it
    fhe_rns_ntt *owner = nullptr;
    const void *src = nullptr;                      // what the key was imported from (outputs must not alias it)
    void *d_s = nullptr;                            // s as given followed by s^2 = s (*) s: 2 x [L][n] containers, coefficient form (the composed paths multiply by these)
    void *d_packed = nullptr;                       // fused paths: (s^, s^ . s^), 2 x [L][n] residues, transformed and packed like one key row each
};
struct fhe_public_key {                             // keys.hip; encrypt.hip reads it
    fhe_rns_ntt *owner = nullptr;
    const void *src0 = nullptr, *src1 = nullptr;    // what the key was imported from (outputs must not alias them)
    void *d_pk = nullptr;                           // (pk0, pk1) as given: 2 x [L][n] containers, coefficient form (the composed path multiplies by these)
    void *d_packed = nullptr;                       // fused path: (pk0^, pk1^), 2 x [L][n] residues, transformed and packed like one key row each
};

// The one place that maps a word-sized width class to its field type: fn(F32{}) / fn(F52{}) / fn(F64{}) / fn(F64X{}), in the body
// `using F = decltype(f);`.  The FHE_WIDTH_256 branch stays with the caller.
template <class Fn>
int with_word_field(const fhe_rns_ntt *h, Fn &&fn) {
    switch (h->width) {
        case FHE_WIDTH_32: return fn(fhe_dev::F32{});
        case FHE_WIDTH_52: return fn(fhe_dev::F52{});
        case FHE_WIDTH_64: return fn(fhe_dev::F64{});
        case FHE_WIDTH_64X: return fn(fhe_dev::F64X{});
        default: return fail(FHE_ERR_UNSUPPORTED, "width class " + std::to_string(h->width) + " has no word-sized field (compact polynomials and the field kernels exist on the word-sized classes only)");
    }
}
// The one place that types the engine's limb table for the kernels that are templated on the limb-table type and not on the field (bootstrap.hip.h,
// lwe_pack.hip.h): fn(const Limb<F> *) on the word-sized classes, fn(const Limb256 *) on FHE_WIDTH_256; in the body, limb_of<decltype(limbs)>.
template <class P> using limb_of = std::remove_const_t<std::remove_pointer_t<P>>;
template <class Fn>
int with_limbs(const fhe_rns_ntt *h, Fn &&fn) {
    if (h->width == FHE_WIDTH_256) return fn((const fhe_dev::Limb256 *)h->d_limbs);
    return with_word_field(h, [&](auto f) { return fn((const fhe_dev::Limb<decltype(f)> *)h->d_limbs); });
}
// "pw operand" of the constant c for limb modulus q of a word-sized class: c * 2^W mod q for the integer fields (so that the
// Montgomery product with it is the plain product), c itself for the FP64 field
template <class F> inline typename F::E word_operand(uint64_t c, uint64_t q) {
    using E = typename F::E;
    if (std::is_same<F, fhe_dev::F52>::value) return (E)c;
    const unsigned W = 8 * sizeof(E);
    fhe_host::u128 v = (fhe_host::u128)(c % q);
    for (unsigned k = 0; k < W; k++) v = (v << 1) % q;
    return (E)(uint64_t)v;
}
inline uint64_t inv_mod_u64(uint64_t a, uint64_t q) {       // a^(q-2) mod q, q prime
    fhe_host::u128 acc = 1, b = a % q; uint64_t e = q - 2;
    for (; e; e >>= 1) { if (e & 1) acc = acc * b % q; b = b * b % q; }
    return (uint64_t)acc;
}
// every modulus below 2^64: a word-sized class, or FHE_WIDTH_256 chosen for the SIZE (n < 2^11 has no word-sized kernels), not for a wide modulus
inline bool word_sized_moduli(const fhe_rns_ntt *h) {
    for (const U256 &q : h->moduli) if (q.w[1] | q.w[2] | q.w[3]) return false;
    return true;
}
inline size_t residue_bytes(const fhe_rns_ntt *h) { return h->residue_bytes; }   // of a compact polynomial's coefficient
inline int lds_width_id(const fhe_rns_ntt *h) { return h->lds_id; }
inline size_t packed_row_bytes(const fhe_rns_ntt *h) { return (size_t)h->L * h->n * residue_bytes(h); }   // of one packed row: [L][n] residues

struct Scratch {                                     // device allocations of one call, freed when it ends
    std::vector<void *> p;
    ~Scratch() { for (void *d : p) if (d) (void)hipFree(d); }
    int get(void **out, size_t bytes) {
        HIP_TRY(hipMalloc(out, bytes));
        p.push_back(*out);
        return FHE_OK;
    }
};

// ---- engine.hip -----------------------------------------------------------------------------------------------------------------
int create_impl(fhe_rns_ntt **out, uint32_t n, const uint64_t (*moduli)[4], uint32_t L, bool base_only = false);
void destroy_impl(fhe_rns_ntt *h);
int check_call(const fhe_rns_ntt *h, uint32_t batch, const char *what);
int check_inputs(fhe_rns_ntt *h, std::initializer_list<const void *> operands, uint32_t batch);   // FHE_HIP_CHECK_INPUTS=1
// check_call, then what the entry points around the blind rotation ask of the engine: every modulus below 2^64 (FHE_ERR_UNSUPPORTED, ahead of
// the caller's null and alignment tests) and, with min_n8, n >= 8
inline int check_word_call(const fhe_rns_ntt *h, uint32_t batch, const char *what, bool min_n8 = false) {
    int rc = check_call(h, batch, what); if (rc) return rc;
    if (!word_sized_moduli(h)) return fail(FHE_ERR_UNSUPPORTED, std::string(what) + ": every modulus must be below 2^64");
    if (min_n8 && h->n < 8) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": n must be at least 8");
    return FHE_OK;
}
// `count` samples per batch element (fhe_lwe_pack, fhe_rlwe_sample_extract_strided): a power of two in [1, n], and the sample rows are indexed in 32 bits
inline int check_count(const fhe_rns_ntt *h, uint32_t count, uint32_t batch, const char *what) {
    if (!count || (count & (count - 1)) || count > h->n) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": count must be a power of two in [1, n]");
    if ((uint64_t)batch * count > 0xffffffffull) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": batch * count overflows 32 bits");
    if ((uint64_t)batch * count * h->L > 0x7fffffffull) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": batch * count * num_primes too large");
    return FHE_OK;
}
int grow_ws(fhe_rns_ntt *h, Workspace &w, size_t bytes);   // at least `bytes` in w (refused while h's stream is capturing)
struct WsNeed {
    size_t ws = 0, ws2 = 0, ws3 = 0;     // bytes of WS1, WS2, WS3
    WsNeed &operator|=(const WsNeed &o) { ws = std::max(ws, o.ws); ws2 = std::max(ws2, o.ws2); ws3 = std::max(ws3, o.ws3); return *this; }
    friend WsNeed operator|(WsNeed a, const WsNeed &b) { return a |= b; }
};
inline int ensure_need(fhe_rns_ntt *h, const WsNeed &n) {
    int rc = grow_ws(h, h->ws[WS1], n.ws); if (!rc) rc = grow_ws(h, h->ws[WS2], n.ws2);
    return rc ? rc : grow_ws(h, h->ws[WS3], n.ws3);
}
int ensure_aux_stream(fhe_rns_ntt *h);   // second stream + events of the chunked two-stage pipelines, created on first use

template <class T>
int upload(fhe_rns_ntt *h, const std::vector<T> &v, void **out) {    // a table owned by the engine (d_tables)
    void *d = nullptr;
    HIP_TRY(hipMalloc(&d, v.size() * sizeof(T)));
    h->d_tables.push_back(d);
    HIP_TRY(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = d;
    return FHE_OK;
}

// ---- transforms.hip -------------------------------------------------------------------------------------------------------------
// Which form runs a multiply, tensor product, key switch or external product is decided by the planners and nowhere else.  A plan also says what the
// form needs of the workspaces; need_* merges the plans of an entry point's calls, the entry point ensures that, and so does fhe_rns_ntt_reserve.
struct LdsPlan {
    fhe_dev::LdsForm form = fhe_dev::LDS_ONE_LAUNCH;
    int ws = 0;                          // the form's own workspace (LdsArgs::ws): 0 none, 1 WS1, 3 WS3
    size_t bytes = 0;
    bool compact = false;                // key switch: c2 is read compact (compacted first, or from the fused tensor product); external product: the
                                         // blind-rotation loop keeps the accumulator pair compact
    bool add_compact = false;            // key switch: separate compact addends (KS_FUSED) instead of accumulating in place
    bool prerot = false;                 // external product: the loop applies the monomial factor once per step (rotated digit sources rot0, rot1)
    size_t ws2 = 0;                      // compact polynomials in WS2: 3 components (KS_FUSED), 1 (compacted KS_C2), 4 or 6 (compact external-product loop)
    WsNeed need() const { return {ws == 1 ? bytes : 0, ws2, ws == 3 ? bytes : 0}; }
};
// Key switch source.  KS_C2: c2 in containers, compacted first where that pays; KS_C2_AS_IS: containers that must stay where they are (c2 already
// in WS2: the composed multiply + relinearise under a testing switch); KS_FUSED: c2 and the addends are compact polynomials
enum KsSource { KS_C2, KS_C2_AS_IS, KS_FUSED };
LdsPlan plan_multiply(const fhe_rns_ntt *h, size_t polys, bool same_operands);
LdsPlan plan_ct_multiply(const fhe_rns_ntt *h, size_t polys, bool same_operands, bool compact_out, bool alone);
bool plan_fused_ct_relin(const fhe_rns_ntt *h, bool packed_keys);
LdsPlan plan_keyswitch(const fhe_rns_ntt *h, size_t polys, uint32_t K, KsSource src, bool alone);
LdsPlan plan_extprod(const fhe_rns_ntt *h, size_t polys, uint32_t K);
bool plan_fused_hoist(const fhe_rns_ntt *h, bool packed_keys);   // hoisted rotations on the LDS kernels of hoist.hip.h (else the composed path)
bool plan_fused_lincomb(const fhe_rns_ntt *h, bool packed_keys); // hoisted linear transform on the LDS kernels of hoist_lincomb.hip.h (else the composed path)
bool plan_fused_encrypt(const fhe_rns_ntt *h);                   // public-key encryption on the LDS kernel of encrypt.hip.h (else the composed path)
bool plan_fused_decrypt(const fhe_rns_ntt *h);                   // secret-key decryption on the LDS kernel of decrypt.hip.h (else the composed path)
bool plan_fused_keygen(const fhe_rns_ntt *h, bool packed_keys);  // key-switching key generation on the LDS kernel of keygen.hip.h (else the composed path)
bool plan_fused_slots(const fhe_rns_ntt *te);                    // batch encoder on the LDS kernels of encode.hip.h; te = the encoder's engine on (n, t) (else the composed path)
bool plan_encrypt_per_ct(const fhe_rns_ntt *h, uint32_t batch);  // ... on the one-workgroup-per-ciphertext grid (else one per (ciphertext, limb))
// What a call of `batch` units needs (K digits; packed: the key set has packed tables, i.e. runs the fused kernels); the last four: keyswitch.hip
WsNeed need_transform(const fhe_rns_ntt *h, size_t polys);                       // forward / inverse of `polys` limb polynomials
WsNeed need_multiply(const fhe_rns_ntt *h, uint32_t batch);
WsNeed need_ct_multiply(const fhe_rns_ntt *h, uint32_t batch, bool same_operands);
WsNeed need_relinearize(const fhe_rns_ntt *h, uint32_t batch, uint32_t K, bool packed, KsSource src);
WsNeed need_ct_multiply_relin(const fhe_rns_ntt *h, uint32_t batch, uint32_t K, bool packed);
WsNeed need_apply_galois(const fhe_rns_ntt *h, uint32_t batch, uint32_t K, bool packed);
WsNeed need_blind_rotate(const fhe_rns_ntt *h, uint32_t batch, uint32_t K, bool packed);
inline fhe_dev::LdsArgs lds_args(fhe_rns_ntt *h, int op, const LdsPlan &p, uint32_t polys) {   // everything but the operands and layouts of the op
    fhe_dev::LdsArgs A;
    A.op = op; A.form = p.form; A.ws = p.ws == 1 ? h->ws[WS1].p : p.ws == 3 ? h->ws[WS3].p : nullptr;
    A.limbs = h->d_limbs; A.L = h->L; A.polys = polys; A.stream = h->stream;
    return A;
}
// one call of the (field, log_n) instance: the instance launches exactly the form A asks for, or nothing and says so
int lds_launch(fhe_rns_ntt *h, const fhe_dev::LdsArgs &A, const char *what, int log_n = 0);
int do_forward(fhe_rns_ntt *h, void *d_data, uint32_t batch);
int do_inverse(fhe_rns_ntt *h, void *d_data, uint32_t batch);
template <int OP> int do_ew(fhe_rns_ntt *h, void *r, const void *a, const void *b, uint32_t batch, const char *what);   // OP 0: product, 1: add, 2: sub
int do_ct_multiply(fhe_rns_ntt *h, void *c0, void *c1, void *c2, const void *a0, const void *a1, const void *b0, const void *b1, uint32_t batch);
int compact_poly(fhe_rns_ntt *h, void *out, const void *in, size_t containers);   // containers -> compact polynomials (word-sized classes)

// ---- keys.hip -------------------------------------------------------------------------------------------------------------------
// `rows` polynomials of [L][n] NTT-domain containers -> packed residues (times 2^W, register order of the fused kernels), and back; `what` names the launch
int pack_rows(fhe_rns_ntt *h, void *dst, const void *src, uint32_t rows, const char *what);
int unpack_rows(fhe_rns_ntt *h, void *dst, const void *src, uint32_t rows, const char *what);
fhe_relin_keys *new_key_set(fhe_rns_ntt *h, uint32_t decomp_bits, uint32_t K);   // an empty set of L K rows (nullptr: out of host memory)
// A generated or imported set whose tables are complete (NTT domain): packed = what keys_get_packed says of it.  Packs d_kb / d_ka into
// d_pkb / d_pka and drops the containers where the set has them, and records K for fhe_rns_ntt_reserve.
int finish_key_set(fhe_rns_ntt *h, fhe_relin_keys *rk, bool packed);

// ---- keyswitch.hip --------------------------------------------------------------------------------------------------------------
uint32_t relin_digits(const fhe_rns_ntt *h, uint32_t decomp_bits);               // K of fhe_relin_num_digits
bool keys_get_packed(const fhe_rns_ntt *h, uint32_t decomp_bits, uint32_t K);   // whether such a key set gets packed tables, i.e. runs the fused kernels
int check_galois_element(const fhe_rns_ntt *h, uint32_t g, const char *what);   // odd and below 2n
// sigma_g of one or two components (in1 == nullptr: one) into out0 / out1, zero_out (optional) cleared beside them; compact: residues out
int do_galois(fhe_rns_ntt *h, void *out0, void *out1, void *zero_out, const void *in0, const void *in1, uint32_t g, size_t polys, bool compact);

// ---- sampling.hip ---------------------------------------------------------------------------------------------------------------
int ensure_cdt(fhe_rns_ntt *h, double sigma, const char *what);   // h->d_cdt / cdt_len = the cumulative table of sigma (uploaded when sigma changes)
// fhe_rns_sample_uniform for the polynomials first_poly .. first_poly + polys - 1 of a stream (first_poly a multiple of L), into d_out[0 .. polys)
int sample_uniform_from(fhe_rns_ntt *h, void *d_out, uint64_t seed, size_t first_poly, size_t polys);

// ---- rns.hip --------------------------------------------------------------------------------------------------------------------
int ensure_crt(fhe_rns_ntt *h);          // CrtLimb[L] (and Q, where it fits 255 bits) on first use
int ensure_from_rns_word(fhe_rns_ntt *h);   // word-sized classes: d_from_rns_w_minv / d_from_rns_w_M on first use (from_rns, decrypt)

#pragma GCC visibility pop
