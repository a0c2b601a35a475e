// encode.hip -- the batch encoder (fhe_batch_encoder_*, fhe_slots_encode, fhe_slots_decode, fhe_slots_decode_poly): slot values <-> plaintext
// polynomials on the device.  An encoder owns a one-limb engine on (n, t) -- the existing table construction, the existing transforms -- plus the
// position -> slot table of its order and one reduction entry per limb of the target engine.
// Fused path (plan_fused_slots; kernels: encode.hip.h): one launch per call on the LDS instance of t's field, no workspace.  Composed path (sizes
// outside N = 2^11 .. 2^14, FHE_HIP_NO_FUSED_ENCODE=1): a gather into [batch][1][n] containers of the encoder's scratch, do_inverse on the
// encoder's engine, one streaming kernel into the L limbs; decoding is the mirror image with do_forward.  Same bits either way.
#include "engine.h"

#define FHE_ENCODE_STREAM_KERNELS
#include "encode.hip.h"

struct fhe_batch_encoder {
    fhe_rns_ntt *owner = nullptr;                   // the target engine: L, the moduli, the stream
    fhe_rns_ntt *te = nullptr;                      // owned: one limb on (n, t); owns the two tables below
    uint64_t t = 0;
    int order = 0;
    void *d_table = nullptr;                        // uint32_t[n]: position of the NTT domain -> slot index
    void *d_red = nullptr;                          // ModT[L]: reduction modulo q_l where t > q_l, t == 0 elsewhere
    bool reduces_limb0 = false;                     // t > q_0: limb 0 of a plaintext is not m (fhe_slots_decode_poly refuses)
    Workspace scratch;                              // composed path: [batch][1][n] containers
};

// table[pos] = the slot i whose exponent e(i) is 2 bitrev(pos) + 1, the point position pos of the NTT domain holds
static int slot_table(uint32_t n, int order, uint32_t *table) {
    if (n < 2 || (n & (n - 1)) || n > (1u << 30)) return fail(FHE_ERR_INVALID_ARG, "slot table: n must be a power of two in [2, 2^30]");
    if (order != FHE_SLOTS_NATURAL && order != FHE_SLOTS_ROWS) return fail(FHE_ERR_INVALID_ARG, "slot table: unknown slot order");
    uint32_t log_n = 0; while ((1u << log_n) < n) log_n++;
    const uint32_t mask = 2 * n - 1;
    uint32_t e = 1;                                 // 3^k mod 2n
    for (uint32_t i = 0; i < (order == FHE_SLOTS_ROWS ? n / 2 : n); i++) {
        if (order == FHE_SLOTS_NATURAL) table[fhe_host::bitrev(i, log_n)] = i;
        else {
            table[fhe_host::bitrev((e - 1) / 2, log_n)] = i;
            table[fhe_host::bitrev((2 * n - e - 1) / 2, log_n)] = n / 2 + i;
            e = (uint32_t)(((uint64_t)e * 3) & mask);
        }
    }
    return FHE_OK;
}
extern "C" int fhe_batch_encoder_slot_table(uint32_t n, int slot_order, uint32_t *table) {
    if (!table) return fail(FHE_ERR_INVALID_ARG, "slot table: null argument");
    return slot_table(n, slot_order, table);
}

extern "C" int fhe_batch_encoder_destroy(fhe_batch_encoder_t *enc) {
    if (enc) {
        if (enc->scratch.p) (void)hipFree(enc->scratch.p);
        destroy_impl(enc->te);
        delete enc;
    }
    return FHE_OK;
}
extern "C" int fhe_batch_encoder_create(fhe_rns_ntt_t *h, fhe_batch_encoder_t **out, uint64_t t, int slot_order) {
    if (!h || !out) return fail(FHE_ERR_INVALID_ARG, "batch_encoder_create: null argument");
    if (slot_order != FHE_SLOTS_NATURAL && slot_order != FHE_SLOTS_ROWS) return fail(FHE_ERR_INVALID_ARG, "batch_encoder_create: unknown slot order");
    const uint64_t mod[1][4] = {{t, 0, 0, 0}};
    fhe_rns_ntt *te = nullptr;
    int rc = create_impl(&te, h->n, mod, 1);        // FHE_ERR_BAD_MODULUS unless t is a prime = 1 (mod 2n)
    if (rc) return rc;
    fhe_batch_encoder *enc = new (std::nothrow) fhe_batch_encoder();
    if (!enc) { destroy_impl(te); return fail(FHE_ERR_INVALID_ARG, "out of host memory"); }
    enc->owner = h; enc->te = te; enc->t = t; enc->order = slot_order;
    std::vector<uint32_t> table(h->n);
    std::vector<fhe_host::ModT> red(h->L);
    if (!(rc = slot_table(h->n, slot_order, table.data()))) {
        for (uint32_t l = 0; l < h->L; l++) {
            const U256 &q = h->moduli[l];
            std::memset(&red[l], 0, sizeof(fhe_host::ModT));
            if (!(q.w[1] | q.w[2] | q.w[3]) && t > q.w[0]) { fhe_host::modt_init(red[l], q.w[0]); if (!l) enc->reduces_limb0 = true; }
        }
        if (!(rc = upload(te, table, &enc->d_table))) rc = upload(te, red, &enc->d_red);
    }
    if (rc) { fhe_batch_encoder_destroy(enc); return rc; }
    *out = enc;
    return FHE_OK;
}
extern "C" int fhe_batch_encoder_scratch_bytes(const fhe_batch_encoder_t *enc, uint64_t *bytes) {
    if (!enc || !bytes) return fail(FHE_ERR_INVALID_ARG, "batch_encoder_scratch_bytes: null argument");
    *bytes = (uint64_t)enc->scratch.bytes + enc->te->ws[WS1].bytes + enc->te->ws[WS2].bytes + enc->te->ws[WS3].bytes;
    return FHE_OK;
}

static int check_encoder(fhe_rns_ntt *h, const fhe_batch_encoder *enc, uint32_t batch, const char *what) {
    int rc = check_call(h, batch, what); if (rc) return rc;
    if (!enc) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": null encoder");
    if (enc->owner != h) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": the encoder was created for a different engine");
    return FHE_OK;
}
// the composed path's scratch and the workspaces of its transforms (nothing on the fused path)
static int ensure_slots(fhe_rns_ntt *h, fhe_batch_encoder *enc, uint32_t batch) {
    enc->te->stream = h->stream;
    if (plan_fused_slots(enc->te)) return FHE_OK;
    int rc = ensure_need(enc->te, need_transform(enc->te, batch)); if (rc) return rc;
    return grow_ws(enc->te, enc->scratch, (size_t)batch * h->n * 32);
}
extern "C" int fhe_batch_encoder_reserve(fhe_rns_ntt_t *h, fhe_batch_encoder_t *enc, uint32_t batch) {
    int rc = check_encoder(h, enc, batch, "batch_encoder_reserve"); if (rc) return rc;
    return ensure_slots(h, enc, batch);
}


extern "C" int fhe_slots_encode(fhe_rns_ntt_t *h, const fhe_batch_encoder_t *enc_c, void *d_out, const uint64_t *d_values, uint32_t batch) {
    fhe_batch_encoder *enc = const_cast<fhe_batch_encoder *>(enc_c);      // the scratch of the composed path is the encoder's
    int rc = check_encoder(h, enc, batch, "slots_encode"); if (rc) return rc;
    if (!d_out || !d_values) return fail(FHE_ERR_INVALID_ARG, "slots_encode: null argument");
    if ((rc = check_aligned({d_out}, "slots_encode"))) return rc;
    if ((uintptr_t)d_values & 7) return fail(FHE_ERR_INVALID_ARG, "slots_encode: d_values must be 8-byte aligned");
    const size_t count = (size_t)batch * h->n;
    if (overlaps(d_out, count * h->L * 32, d_values, count * 8)) return fail(FHE_ERR_INVALID_ARG, "slots_encode: the output must not alias the input");
    if ((rc = ensure_slots(h, enc, batch))) return rc;                   // (no-op after fhe_batch_encoder_reserve)
    fhe_rns_ntt *te = enc->te;
    if (plan_fused_slots(te)) {
        fhe_dev::LdsArgs A = lds_args(te, fhe_dev::LDS_SLOTS_ENCODE, {}, batch);
        A.r0 = d_out; A.a0 = d_values; A.kb = enc->d_table; A.ka = enc->d_red; A.L = h->L; A.in_compact = true;
        return lds_launch(te, A, "ntt_slots_encode_kernel");
    }
    hipLaunchKernelGGL(fhe_dev::slots_gather_kernel, dim3(ew_grid(count)), dim3(256), 0, h->stream, (fhe_dev::v2u64 *)enc->scratch.p, d_values,
                       (const uint32_t *)enc->d_table, h->log_n, count);
    if ((rc = post_launch(h->stream, "slots_gather_kernel"))) return rc;
    if ((rc = do_inverse(te, enc->scratch.p, batch))) return rc;
    hipLaunchKernelGGL(fhe_dev::slots_spread_kernel, dim3(ew_grid(count)), dim3(256), 0, h->stream, (fhe_dev::v2u64 *)d_out, (const fhe_dev::v2u64 *)enc->scratch.p,
                       (const fhe_host::ModT *)enc->d_red, h->L, h->log_n, count);
    return post_launch(h->stream, "slots_spread_kernel");
}

static int slots_decode(fhe_rns_ntt *h, fhe_batch_encoder *enc, uint64_t *d_values, const void *d_src, bool containers, uint32_t batch, const char *what) {
    int rc = check_encoder(h, enc, batch, what); if (rc) return rc;
    if (!d_values || !d_src) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": null argument");
    if ((uintptr_t)d_values & 7) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": d_values must be 8-byte aligned");
    if (containers) { if ((rc = check_aligned({d_src}, what))) return rc; }
    else if ((uintptr_t)d_src & 7) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": d_m must be 8-byte aligned");
    const size_t count = (size_t)batch * h->n;
    if (containers) {
        if (enc->reduces_limb0) return fail(FHE_ERR_UNSUPPORTED, std::string(what) + ": t exceeds the first modulus, so limb 0 holds m mod q_0 and not m");
        if (overlaps(d_values, count * 8, d_src, count * h->L * 32)) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": the output must not alias the plaintexts");
    } else if ((const void *)d_values != d_src && overlaps(d_values, count * 8, d_src, count * 8))
        return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": the output must be d_m itself (in place) or not overlap it");
    if ((rc = ensure_slots(h, enc, batch))) return rc;
    fhe_rns_ntt *te = enc->te;
    if (plan_fused_slots(te)) {
        fhe_dev::LdsArgs A = lds_args(te, fhe_dev::LDS_SLOTS_DECODE, {}, batch);
        A.r0 = d_values; A.a0 = d_src; A.kb = enc->d_table; A.L = h->L; A.in_compact = !containers; A.out_compact = true;
        return lds_launch(te, A, "ntt_slots_decode_kernel");
    }
    hipLaunchKernelGGL(fhe_dev::slots_lift_kernel, dim3(ew_grid(count)), dim3(256), 0, h->stream, (fhe_dev::v2u64 *)enc->scratch.p, d_src, containers ? 1u : 0u, h->L,
                       h->log_n, count);
    if ((rc = post_launch(h->stream, "slots_lift_kernel"))) return rc;
    if ((rc = do_forward(te, enc->scratch.p, batch))) return rc;
    hipLaunchKernelGGL(fhe_dev::slots_scatter_kernel, dim3(ew_grid(count)), dim3(256), 0, h->stream, d_values, (const fhe_dev::v2u64 *)enc->scratch.p,
                       (const uint32_t *)enc->d_table, h->log_n, count);
    return post_launch(h->stream, "slots_scatter_kernel");
}
extern "C" int fhe_slots_decode(fhe_rns_ntt_t *h, const fhe_batch_encoder_t *enc, uint64_t *d_values, const uint64_t *d_m, uint32_t batch) {
    return slots_decode(h, const_cast<fhe_batch_encoder *>(enc), d_values, d_m, false, batch, "slots_decode");
}
extern "C" int fhe_slots_decode_poly(fhe_rns_ntt_t *h, const fhe_batch_encoder_t *enc, uint64_t *d_values, const void *d_poly, uint32_t batch) {
    return slots_decode(h, const_cast<fhe_batch_encoder *>(enc), d_values, d_poly, true, batch, "slots_decode_poly");
}
