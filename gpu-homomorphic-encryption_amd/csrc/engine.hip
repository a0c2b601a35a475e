// engine.hip -- the engine handle: lifetime, width-class choice, environment switches, limb tables, workspaces, reserve.
#include "engine.h"

#include <algorithm>
#include <climits>

#include "ntt_wide.hip.h"

void destroy_impl(fhe_rns_ntt *h) {
    if (!h) return;
    for (void *p : h->d_tables) (void)hipFree(p);
    for (Workspace &w : h->ws) if (w.p) (void)hipFree(w.p);
    if (h->d_cdt) (void)hipFree(h->d_cdt);
    if (h->d_flag) (void)hipFree(h->d_flag);
    if (h->aux_stream) (void)hipStreamDestroy(h->aux_stream);
    for (hipEvent_t e : h->ev_chunk) if (e) (void)hipEventDestroy(e);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
}

static uint32_t shoup32(uint64_t w, uint64_t q) { return (uint32_t)((w << 32) / q); }
static uint64_t shoup64(uint64_t w, uint64_t q) { return (uint64_t)((((fhe_host::u128)w) << 64) / q); }

// One limb table: for every limb, fill(c, P, tw, itw) sets the constants of P (zeroed first) and the two n-entry twiddle tables; the tables
// are uploaded, their device pointers stored in P, and the limb array is uploaded to *out.  The fields below keep only their arithmetic.
using Consts = fhe_host::NttConstants;
template <class LimbT, class TW, class Fill>
static int build_limb_table(fhe_rns_ntt *h, const std::vector<Consts> &cs, void **out, const TW *LimbT::*tw_p, const TW *LimbT::*itw_p, Fill &&fill) {
    std::vector<LimbT> limbs(h->L);
    std::vector<TW> tw(h->n), itw(h->n);
    for (uint32_t l = 0; l < h->L; l++) {
        LimbT &P = limbs[l];
        std::memset(&P, 0, sizeof(P));
        fill(cs[l], P, tw, itw);
        void *d = nullptr; int rc;
        if ((rc = upload(h, tw, &d))) return rc; P.*tw_p = (const TW *)d;
        if ((rc = upload(h, itw, &d))) return rc; P.*itw_p = (const TW *)d;
    }
    return upload(h, limbs, out);
}
// ... and a limb table without twiddle tables: fill(c, P) sets the constants of P (zeroed first)
template <class LimbT, class Fill>
static int build_limb_table(fhe_rns_ntt *h, const std::vector<Consts> &cs, void **out, Fill &&fill) {
    std::vector<LimbT> limbs(h->L);
    for (uint32_t l = 0; l < h->L; l++) {
        std::memset(&limbs[l], 0, sizeof(LimbT));
        fill(cs[l], limbs[l]);
    }
    return upload(h, limbs, out);
}

static int build_limbs(fhe_rns_ntt *h, const std::vector<Consts> &cs, fhe_dev::F32) {
    using Lm = fhe_dev::Limb32;
    return build_limb_table<Lm>(h, cs, &h->d_limbs, &Lm::tw, &Lm::itw, [](const Consts &c, Lm &P, auto &tw, auto &itw) {
        const uint64_t q = c.q.w[0];
        for (size_t k = 0; k < tw.size(); k++) {           // Montgomery form: w * 2^32 mod q
            tw[k] = (uint32_t)((c.tw[k].w[0] << 32) % q);
            itw[k] = (uint32_t)((c.itw[k].w[0] << 32) % q);
        }
        P.q = (uint32_t)q; P.q2 = (uint32_t)(2 * q);
        uint32_t x = 1; for (int i = 0; i < 5; i++) x *= 2 - (uint32_t)q * x;     // q^-1 mod 2^32
        P.qinv = 0u - x;                                                           // negated: F32::mont_mul adds m*q instead of subtracting
        const uint64_t two32 = (1ull << 32) % q, ninv = c.n_inv.w[0], w1 = c.itw[1].w[0];
        auto mulq = [q](uint64_t a, uint64_t b) { return (uint64_t)(((fhe_host::u128)a * b) % q); };
        P.r1 = (uint32_t)two32; P.r1_s = shoup32(two32, q);
        P.ninv = (uint32_t)ninv; P.ninv_s = shoup32(ninv, q);
        uint64_t nw = mulq(ninv, w1);
        P.ninvw = (uint32_t)nw; P.ninvw_s = shoup32(nw, q);
        uint64_t nr = mulq(ninv, two32), nwr = mulq(nw, two32);
        P.ninv_r = (uint32_t)nr; P.ninv_r_s = shoup32(nr, q);
        P.ninvw_r = (uint32_t)nwr; P.ninvw_r_s = shoup32(nwr, q);
    });
}

static int build_limbs(fhe_rns_ntt *h, const std::vector<Consts> &cs, fhe_dev::F64) {
    using Lm = fhe_dev::Limb64;
    return build_limb_table<Lm>(h, cs, &h->d_limbs, &Lm::tw, &Lm::itw, [](const Consts &c, Lm &P, auto &tw, auto &itw) {
        const uint64_t q = c.q.w[0];
        for (size_t k = 0; k < tw.size(); k++) {
            tw[k] = make_ulonglong2(c.tw[k].w[0], shoup64(c.tw[k].w[0], q));
            itw[k] = make_ulonglong2(c.itw[k].w[0], shoup64(c.itw[k].w[0], q));
        }
        P.q = q; P.q2 = 2 * q;
        uint64_t x = 1; for (int i = 0; i < 6; i++) x *= 2 - q * x;               // q^-1 mod 2^64
        P.qinv = x;
        auto mulq = [q](uint64_t a, uint64_t b) { return (uint64_t)(((fhe_host::u128)a * b) % q); };
        const uint64_t two64 = (uint64_t)((((fhe_host::u128)1) << 64) % q), ninv = c.n_inv.w[0], w1 = c.itw[1].w[0];
        P.r1 = two64; P.r1_s = shoup64(two64, q);
        P.ninv = ninv; P.ninv_s = shoup64(ninv, q);
        uint64_t nw = mulq(ninv, w1);
        P.ninvw = nw; P.ninvw_s = shoup64(nw, q);
        uint64_t nr = mulq(ninv, two64), nwr = mulq(nw, two64);
        P.ninv_r = nr; P.ninv_r_s = shoup64(nr, q);
        P.ninvw_r = nwr; P.ninvw_r_s = shoup64(nwr, q);
    });
}

static int build_limbs(fhe_rns_ntt *h, const std::vector<Consts> &cs, fhe_dev::F64X) {
    using Lm = fhe_dev::Limb64X;
    return build_limb_table<Lm>(h, cs, &h->d_limbs, &Lm::tw, &Lm::itw, [](const Consts &c, Lm &P, auto &tw, auto &itw) {
        const uint64_t q = c.q.w[0];
        auto mulq = [q](uint64_t a, uint64_t b) { return (uint64_t)(((fhe_host::u128)a * b) % q); };
        const uint64_t two64 = (uint64_t)((((fhe_host::u128)1) << 64) % q), two128 = mulq(two64, two64);
        for (size_t k = 0; k < tw.size(); k++) { tw[k] = mulq(c.tw[k].w[0], two64); itw[k] = mulq(c.itw[k].w[0], two64); }   // Montgomery form: w * 2^64 mod q
        P.q = q; P.q2 = 0;                                 // 2q does not fit; nothing on this field reads it
        uint64_t x = 1; for (int i = 0; i < 6; i++) x *= 2 - q * x;               // q^-1 mod 2^64
        P.qinv = x;
        const uint64_t ninv = c.n_inv.w[0], nw = mulq(ninv, c.itw[1].w[0]);
        P.r1 = two128;
        P.ninv = mulq(ninv, two64); P.ninvw = mulq(nw, two64);
        P.ninv_r = mulq(ninv, two128); P.ninvw_r = mulq(nw, two128);
        P.r1_s = P.ninv_s = P.ninvw_s = P.ninv_r_s = P.ninvw_r_s = x;              // the companion slots carry q^-1 (F64X::inv_last)
    });
}

static int build_limbs(fhe_rns_ntt *h, const std::vector<Consts> &cs, fhe_dev::F52) {
    using Lm = fhe_dev::Limb52;
    return build_limb_table<Lm>(h, cs, &h->d_limbs, &Lm::tw, &Lm::itw, [](const Consts &c, Lm &P, auto &tw, auto &itw) {
        const double q = (double)c.q.w[0];                 // q < 2^43: exact
        const uint64_t qi = c.q.w[0];
        // companions fl(w * fl(1/q)) are recomputed in the butterflies
        for (size_t k = 0; k < tw.size(); k++) { tw[k] = (double)c.tw[k].w[0]; itw[k] = (double)c.itw[k].w[0]; }
        auto mulq = [qi](uint64_t a, uint64_t b) { return (uint64_t)(((fhe_host::u128)a * b) % qi); };
        const uint64_t ninv = c.n_inv.w[0], nw = mulq(ninv, c.itw[1].w[0]);
        P.q = q; P.q2 = 2 * q; P.qinv = 1.0 / q;
        P.r1 = 1.0; P.r1_s = 1.0 / q;                       // no Montgomery factor on this path
        P.ninv = (double)ninv; P.ninv_s = (double)ninv / q;
        P.ninvw = (double)nw; P.ninvw_s = (double)nw / q;
        P.ninv_r = P.ninv; P.ninv_r_s = P.ninv_s; P.ninvw_r = P.ninvw; P.ninvw_r_s = P.ninvw_s;
    });
}

// Constants of the container-level kernels of a full-width handle (ntt256.hip.h): radix R = 2^256, no twiddle tables
static int build_limbs256(fhe_rns_ntt *h, const std::vector<Consts> &cs) {
    using Lm = fhe_dev::Limb256;
    return build_limb_table<Lm>(h, cs, &h->d_limbs, [](const Consts &c, Lm &P) {
        fhe_host::Mod M(c.q);
        std::memcpy(P.q.l, c.q.w, 32);
        std::memcpy(P.r2.l, M.r2.w, 32);
        U256 nm = M.to_mont(c.n_inv);
        std::memcpy(P.ninv_m.l, nm.w, 32);
        P.inv0 = M.inv0;
    });
}

// Constants and twiddle tables of the full-width transforms (ntt_wide.hip.h): Montgomery radix R = 2^(64 NL).
template <int NL>
static int build_wlimbs(fhe_rns_ntt *h, const std::vector<Consts> &cs) {
    using W = fhe_dev::wint<NL>; using Lm = fhe_dev::WLimb<NL>;
    return build_limb_table<Lm>(h, cs, &h->d_wlimbs, &Lm::tw, &Lm::itw, [](const Consts &c, Lm &P, auto &tw, auto &itw) {
        fhe_host::Mod M(c.q);
        U256 Rn = M.r1;                                   // 2^256 mod q
        if (NL == 2) { U256 t; t.w[2] = 1; Rn = M.reduce(t); }   // 2^128 mod q
        auto put = [](W &dst, const U256 &v) { for (int i = 0; i < NL; i++) { dst.w[2 * i] = (uint32_t)v.w[i]; dst.w[2 * i + 1] = (uint32_t)(v.w[i] >> 32); } };
        for (size_t k = 0; k < tw.size(); k++) { put(tw[k], M.mul(c.tw[k], Rn)); put(itw[k], M.mul(c.itw[k], Rn)); }
        const U256 R2 = M.mul(Rn, Rn), nR = M.mul(c.n_inv, Rn);
        put(P.q, c.q); put(P.ninv_m, nR); put(P.ninv_r2, M.mul(nR, Rn)); put(P.r2, R2);
        P.qinv32 = (uint32_t)M.inv0;
    });
}
// id of a field's LDS instances in lds_table.cpp
static int lds_id(fhe_dev::F32) { return 32; }
static int lds_id(fhe_dev::F52) { return 52; }
static int lds_id(fhe_dev::F64) { return 64; }
static int lds_id(fhe_dev::F64X) { return 65; }

// base_only: an RNS base without a ring (RNSContext, include/rns.cuh:27-66): the handle is an engine of degree n = 1, whose
// buffers [batch][L][1] are exactly RNSContext's interleaved [count][num_primes] layout (src/rns.cu:103-104) and whose
// transforms are the identity (Z_q[x]/(x + 1) = Z_q), so every container-level entry point works on it unchanged.
static fhe_host::BuildStatus base_constants(const U256 &q, fhe_host::NttConstants &out) {
    if (!(q.w[0] & 1) || (q.w[3] >> 63) || q.bit_length() < 2 || !fhe_host::is_prime(q)) return fhe_host::BUILD_BAD_MODULUS;
    out.n = 1; out.log_n = 0; out.q = q;
    fhe_host::sub_to(out.psi, q, U256(1)); out.psi_inv = out.psi;     // the primitive 2nd root of unity, -1
    out.n_inv = U256(1);
    out.tw.assign(1, U256(1)); out.itw.assign(1, U256(1));
    return fhe_host::BUILD_OK;
}
// One line per switch; all of them are read here, once, when an engine is created.
static EngineEnv read_env() {
    auto set = [](const char *name) { return getenv(name) != nullptr; };
    auto is1 = [](const char *name) { const char *e = getenv(name); return e && e[0] == '1'; };
    auto num = [](const char *name, long dflt, long lo, long hi) { const char *e = getenv(name); const long v = e ? atol(e) : dflt; return (uint32_t)(v < lo ? lo : v > hi ? hi : v); };
    EngineEnv e;
    if (const char *f = getenv("FHE_HIP_FORCE_WIDTH")) e.force_width = atoi(f);        // testing aid: "52" / "64" / "65" / "128" / "256" force a wider path than needed
    e.no_wide_lazy = set("FHE_HIP_NO_WIDE_LAZY");                                      // full-width class: the canonical tile kernels (cross-check / A-B)
    e.no_wide_tiles = set("FHE_HIP_NO_WIDE_TILES");                                    // full-width class: every stage as a global-memory pass (cross-check / A-B)
    e.no_square = set("FHE_HIP_NO_SQUARE_KERNELS");
    e.single_transforms = set("FHE_HIP_NO_PAIRED_TRANSFORMS");
    e.global_twiddles = set("FHE_HIP_NO_LDS_TWIDDLES");
    e.no_fused_keyswitch = set("FHE_HIP_NO_FUSED_KEYSWITCH");
    e.no_word_conversions = set("FHE_HIP_NO_WORD_CONVERSIONS");
    e.no_fused_blind_rotate = set("FHE_HIP_NO_FUSED_BLIND_ROTATE");
    e.no_fused_ct_relin = set("FHE_HIP_NO_FUSED_CT_RELIN");
    e.no_compact_blind_rotate = set("FHE_HIP_NO_COMPACT_BLIND_ROTATE");
    e.no_two_launch_ct = set("FHE_HIP_NO_TWO_LAUNCH_CT");
    e.no_fused_galois = set("FHE_HIP_NO_FUSED_GALOIS");                                // fhe_ct_apply_galois on the composed path everywhere (cross-check)
    e.no_fused_hoist = set("FHE_HIP_NO_FUSED_HOIST");                                  // hoisted rotations on the composed path everywhere (cross-check); key import is unchanged
    e.no_fused_encrypt = set("FHE_HIP_NO_FUSED_ENCRYPT");                              // fhe_ct_encrypt on the composed path everywhere (cross-check); read when a public key is imported too
    e.no_fused_decrypt = set("FHE_HIP_NO_FUSED_DECRYPT");                              // fhe_ct_decrypt on the composed path everywhere (cross-check); read when a secret key is imported too
    e.no_fused_encode = set("FHE_HIP_NO_FUSED_ENCODE");                                // fhe_slots_encode / fhe_slots_decode on the composed path everywhere (cross-check); read when an encoder is created
    e.no_fused_keygen = set("FHE_HIP_NO_FUSED_KEYGEN");                                // fhe_keyswitch_keys_generate on the composed path everywhere (cross-check)
    e.encrypt_per_ct_batch = num("FHE_HIP_ENCRYPT_PER_CT_BATCH", 256, 0, LONG_MAX); // fused fhe_ct_encrypt of at least this many ciphertexts: one workgroup per ciphertext, sampling once (0 = always)
    e.split_keyswitch = set("FHE_HIP_SPLIT_KEYSWITCH");
    e.small_batch_polys = num("FHE_HIP_SMALL_BATCH_POLYS", 256, 0, LONG_MAX);       // fused multiply of at most this many limb polynomials runs the 16-per-thread latency kernel (0 = never)
    e.coop_polys = num("FHE_HIP_COOP_POLYS", 64, 0, 64);                               // ... (N = 2^13 / 2^14, 4-byte residues) spreads each over four workgroups in three launches (0 = never)
    e.split_pairs_polys = num("FHE_HIP_SPLIT_PAIRS_POLYS", 128, 0, LONG_MAX);       // key switch (paired kernel) of at most this many limb polynomials runs one workgroup per digit pair + a combining launch (0 = never)
    e.relin_chunks_forced = set("FHE_HIP_RELIN_PIPELINE");                             // the stand-alone relinearisation also runs as a two-stream pipeline (A/B)
    e.overlap_chunks = num("FHE_HIP_CT_RELIN_CHUNKS", 4, 1, 16);                       // pieces the one-call multiply is cut into (1 = one stream)
    e.no_prerotation = set("FHE_HIP_NO_PREROTATION");                                  // blind-rotation loop of the three-array kernels: monomial factor inside the kernel, per digit (A/B, cross-check)
    e.no_c2_compaction = set("FHE_HIP_NO_C2_COMPACTION");                              // stand-alone relinearisation of the 8-byte fields: c2 read as containers (A/B, cross-check)
    if (const char *m = getenv("FHE_HIP_CT_FORM")) e.ct_form_force = !strcmp(m, "two") ? 2 : !strcmp(m, "one") ? 1 : 0;   // 0 = by field and size, 1 / 2 = one- / two-launch tensor product where it exists
    e.check_inputs = is1("FHE_HIP_CHECK_INPUTS");                                      // every compute entry point first scans its operands (check_inputs below)
    return e;
}

int create_impl(fhe_rns_ntt **out, uint32_t n, const uint64_t (*moduli)[4], uint32_t L, bool base_only) {
    if (!out || !moduli) return fail(FHE_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (base_only) n = 1;
    else if (n < 8 || n > 65536 || (n & (n - 1))) return fail(FHE_ERR_INVALID_ARG, "polynomial degree must be a power of two in [8, 65536]");
    if (L < 1 || L > 64) return fail(FHE_ERR_INVALID_ARG, "num_primes must be in [1, 64]");
    std::vector<Consts> cs(L);
    int max_bits = 0;
    for (uint32_t l = 0; l < L; l++) {
        U256 q = U256::from(moduli[l]);
        for (uint32_t k = 0; k < l; k++) if (q == cs[k].q) return fail(FHE_ERR_BAD_MODULUS, "the RNS primes must be pairwise distinct");
        fhe_host::BuildStatus st = base_only ? base_constants(q, cs[l]) : fhe_host::build_constants(n, q, cs[l]);
        if (st != fhe_host::BUILD_OK) {
            char buf[160];
            snprintf(buf, sizeof buf, "modulus %u (low limb 0x%llx) rejected: need an odd prime < 2^255 with q = 1 (mod 2n)", l,
                     (unsigned long long)q.w[0]);
            return fail(FHE_ERR_BAD_MODULUS, buf);
        }
        if (q.bit_length() > max_bits) max_bits = q.bit_length();
    }
    int rc = ensure_device(); if (rc) return rc;
    fhe_rns_ntt *h = new (std::nothrow) fhe_rns_ntt();
    if (!h) return fail(FHE_ERR_INVALID_ARG, "out of host memory");
    h->n = n; h->L = L; while ((1u << h->log_n) < n) h->log_n++;
    for (uint32_t l = 0; l < L; l++) h->moduli.push_back(cs[l].q);
    h->env = read_env();
    // word-sized classes: one LDS-resident kernel per transform for 2^11 .. 2^15 (4-byte residues) / 2^14 (8-byte residues), two passes
    // (top stages over global memory + 2^13-coefficient LDS blocks) up to 2^16
    const bool lds_size = h->log_n >= 11 && h->log_n <= 16;
    const int floor_w = h->env.force_width;
    if (floor_w >= 128) h->width = FHE_WIDTH_256;      // 128: the full-width class on two 64-bit limbs (needs q < 2^127), 256: on four
    else if (lds_size && max_bits <= 30 && floor_w < 52) h->width = FHE_WIDTH_32;
    else if (lds_size && max_bits <= 43 && floor_w < 64) h->width = FHE_WIDTH_52;
    else if (lds_size && max_bits <= 62 && floor_w < 65) h->width = FHE_WIDTH_64;
    else if (lds_size && max_bits <= 64) h->width = FHE_WIDTH_64X;      // FHE_HIP_FORCE_WIDTH=65 forces it
    else h->width = FHE_WIDTH_256;
#define TRY_OR_DESTROY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { destroy_impl(h); return fail(FHE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } } while (0)
    TRY_OR_DESTROY(hipGetDevice(&h->device));
    TRY_OR_DESTROY(hipStreamCreate(&h->own_stream));   // blocking stream, like the reference's cudaStreamCreate (src/ntt.cu:18):
                                                       // a later hipMemcpy on the null stream is ordered after our kernels
    h->stream = h->own_stream;
    TRY_OR_DESTROY(hipMalloc((void **)&h->d_flag, sizeof(uint32_t)));
    TRY_OR_DESTROY(hipMemset(h->d_flag, 0, sizeof(uint32_t)));
#undef TRY_OR_DESTROY
    if (h->width != FHE_WIDTH_256) {
        rc = with_word_field(h, [&](auto f) {
            h->residue_bytes = sizeof(typename decltype(f)::E); h->lds_id = lds_id(f);
            return build_limbs(h, cs, f);
        });
        if (h->log_n > (h->width == FHE_WIDTH_32 ? 15u : 14u)) h->sub_top = h->log_n - 13;
    } else if (!(rc = build_limbs256(h, cs))) {
        h->wide_nl = (max_bits <= 127 && floor_w != 256) ? 2 : 4;
        // six spare bits above the largest modulus: the tile kernels run their butterflies without full reductions (ntt_wide.hip.h: wbfly)
        h->wide_lazy = max_bits + 6 <= 64 * h->wide_nl && !h->env.no_wide_lazy;
        rc = h->wide_nl == 2 ? build_wlimbs<2>(h, cs) : build_wlimbs<4>(h, cs);
    }
    if (rc) { destroy_impl(h); return rc; }
    *out = h;
    return FHE_OK;
}

int check_call(const fhe_rns_ntt *h, uint32_t batch, const char *what) {
    if (!h) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": null handle");
    if (!batch) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": batch must be >= 1");
    if ((uint64_t)batch * h->L > 0x7fffffffull) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": batch * num_primes too large");
    (void)hipGetLastError();            // drop any stale sticky error so post_launch reports only this call's
    return FHE_OK;
}

// Library-owned workspaces are per ENGINE and grow on demand; calls on one engine must be ordered on one stream (they share them).
// A hipGraph captured from a call has the workspace addresses baked in, so growing (free + malloc) later would make every replay
// touch freed memory: growth is refused while the engine's stream is capturing (call fhe_rns_ntt_reserve(h, max_batch) before the
// capture; after it nothing here allocates), and a larger batch after a capture needs a re-capture -- see INTEGRATION.md.
int grow_ws(fhe_rns_ntt *h, Workspace &w, size_t bytes) {
    if (w.bytes >= bytes) return FHE_OK;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(h->stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone)
        return fail(FHE_ERR_INVALID_ARG, "a library workspace would have to grow while the engine's stream is being captured into a graph: "
                                         "call fhe_rns_ntt_reserve(h, batch) for the largest batch before the capture");
    (void)hipGetLastError();
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (w.p) { HIP_TRY(hipFree(w.p)); w = Workspace{}; }
    HIP_TRY(hipMalloc(&w.p, bytes));
    w.bytes = bytes;
    return FHE_OK;
}
// second stream + events of the chunked two-stage pipelines (fhe_ct_multiply_relin, stand-alone relinearisation): created on first use
int ensure_aux_stream(fhe_rns_ntt *h) {
    if (h->aux_stream) return FHE_OK;
    HIP_TRY(hipStreamCreateWithFlags(&h->aux_stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
    for (hipEvent_t &e : h->ev_chunk) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return FHE_OK;
}

// FHE_HIP_CHECK_INPUTS=1 (read at engine creation): every compute entry point first scans its operands for coefficients that are not
// canonical residues (value >= q_l or non-zero upper words) and returns FHE_ERR_NONCANONICAL instead of computing on them -- the
// word-sized classes read only the low word(s) of a container, so such an operand would otherwise give a silently different
// product than the reference's full 256-bit arithmetic.  Debugging aid: one extra read of every operand and a stream sync per call.
extern "C" int fhe_rns_check_canonical(fhe_rns_ntt_t *h, const void *d_data, uint32_t batch);
int check_inputs(fhe_rns_ntt *h, std::initializer_list<const void *> operands, uint32_t batch) {
    if (!h->env.check_inputs) return FHE_OK;
    for (const void *p : operands) { int rc = fhe_rns_check_canonical(h, p, batch); if (rc) return rc; }
    return FHE_OK;
}

extern "C" int fhe_rns_ntt_create(fhe_rns_ntt_t **out, uint32_t n, const uint64_t (*moduli)[4], uint32_t num_primes) {
    return create_impl(out, n, moduli, num_primes);
}
extern "C" int fhe_rns_base_create(fhe_rns_ntt_t **out, const uint64_t (*primes)[4], uint32_t num_primes) {
    return create_impl(out, 1, primes, num_primes, true);
}
extern "C" int fhe_rns_ntt_destroy(fhe_rns_ntt_t *h) { destroy_impl(h); return FHE_OK; }
extern "C" int fhe_rns_ntt_set_stream(fhe_rns_ntt_t *h, void *stream) {
    if (!h) return fail(FHE_ERR_INVALID_ARG, "null handle");
    h->stream = stream ? (hipStream_t)stream : h->own_stream;
    return FHE_OK;
}
// Pre-sizes the library-owned workspaces for calls of up to `batch` units, so that no later call allocates (hipMalloc synchronises and cannot be captured into a hipGraph):
// the merge of every entry point's need_* (engine.h), for the largest K of the key sets imported so far, with and without packed tables (import keys first).
extern "C" int fhe_rns_ntt_reserve(fhe_rns_ntt_t *h, uint32_t batch) {
    int rc = check_call(h, batch, "reserve"); if (rc) return rc;
    WsNeed n;
    // the few-polynomial forms are taken by every call of at most split_pairs_polys / coop_polys limb polynomials: the largest batch below each threshold as well
    for (uint32_t b : {batch, std::min(batch, h->env.split_pairs_polys / h->L), std::min(batch, h->env.coop_polys / h->L)}) {
        if (!b) continue;
        n |= need_transform(h, (size_t)b * h->L) | need_multiply(h, b) | need_ct_multiply(h, b, false);
        const bool lds_class = h->width != FHE_WIDTH_256 && !h->sub_top;             // where packed key tables exist
        for (bool packed : {true, false}) {
            const uint32_t K = packed ? (lds_class ? std::max(h->max_digits, 1u) : 0) : h->max_composed_digits;
            if (K) n |= need_relinearize(h, b, K, packed, KS_C2) | need_ct_multiply_relin(h, b, K, packed) | need_apply_galois(h, b, K, packed) | need_blind_rotate(h, b, K, packed);
        }
    }
    if ((rc = ensure_need(h, n))) return rc;
    return ensure_aux_stream(h);                                       // second stream + events of the chunked pipelines
}
extern "C" int fhe_rns_ntt_workspace_bytes(const fhe_rns_ntt_t *h, uint64_t *bytes) {
    if (!h || !bytes) return fail(FHE_ERR_INVALID_ARG, "workspace_bytes: null argument");
    *bytes = 0;
    for (int id = 0; id < WS_COUNT; id++) if (ws_in_workspace_bytes(id)) *bytes += h->ws[id].bytes;
    return FHE_OK;
}
extern "C" int fhe_rns_ntt_width_class(const fhe_rns_ntt_t *h) { return h ? h->width : fail(FHE_ERR_INVALID_ARG, "null handle"); }

// ------------------------------------------------------------------------------------------------------
// single-modulus engine ABI = RNS engine with one limb
// ------------------------------------------------------------------------------------------------------
extern "C" int fhe_ntt_create(fhe_ntt_t **out, uint32_t n, const uint64_t q[4]) {
    if (!out || !q) return fail(FHE_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    uint64_t m[1][4]; std::memcpy(m[0], q, 32);
    fhe_rns_ntt *impl = nullptr;
    int rc = create_impl(&impl, n, m, 1); if (rc) return rc;
    fhe_ntt *h = new (std::nothrow) fhe_ntt{impl};
    if (!h) { destroy_impl(impl); return fail(FHE_ERR_INVALID_ARG, "out of host memory"); }
    *out = h;
    return FHE_OK;
}
extern "C" int fhe_ntt_destroy(fhe_ntt_t *h) { if (h) { destroy_impl(h->impl); delete h; } return FHE_OK; }
extern "C" int fhe_ntt_set_stream(fhe_ntt_t *h, void *stream) { return h ? fhe_rns_ntt_set_stream(h->impl, stream) : fail(FHE_ERR_INVALID_ARG, "null handle"); }
extern "C" int fhe_ntt_width_class(const fhe_ntt_t *h) { return h ? h->impl->width : fail(FHE_ERR_INVALID_ARG, "null handle"); }
