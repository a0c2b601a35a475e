// bfv.hip -- BFV multiplication (fhe_bfv_*): the multiplier object, the centred lift Q -> Q u P, scale-and-round by t / Q back to Q, and the
// one-call product around do_ct_multiply on the extended engine (kernels and the layout of the tables: bfv.hip.h; definitions:
// include/fhe_hip.h).  A multiplier owns an engine on (q_0 .. q_{L-1}, p_0 .. p_{L'-1}), whose d_tables hold the conversion tables, and one
// workspace: the lifted operands, the three components of the tensor product over Q u P and c2 of the one-call multiply + relinearise.
// Every table entry is word-sized host arithmetic, built once at creation; no call allocates after fhe_bfv_multiplier_reserve.
#include "engine.h"

#include <array>

#include "bfv.hip.h"

struct fhe_bfv_multiplier {
    fhe_rns_ntt *owner = nullptr;                   // hq: the ciphertext engine (L, the stream)
    fhe_rns_ntt *qp = nullptr;                      // owned: the engine on Q u P (Q first); owns the tables below
    uint64_t t = 0;
    uint32_t L = 0, Lp = 0;
    fhe_dev::BfvLift up = {}, down = {};            // centred lifts Q -> P and P -> Q
    fhe_dev::BfvScale scale = {};
    Workspace ws;                                   // 4 lifted operands + 3 products, [batch][L + L'][n] each, then c2 [batch][L][n]
};

using fhe_host::u128;
typedef std::vector<uint64_t> Big;                  // little-endian words, no length limit: the bound P > 32 t n Q is checked exactly
static void big_mul(Big &a, uint64_t m) {
    uint64_t carry = 0;
    for (uint64_t &w : a) { const u128 p = (u128)w * m + carry; w = (uint64_t)p; carry = (uint64_t)(p >> 64); }
    if (carry) a.push_back(carry);
}
static bool big_greater(Big a, Big b) {
    const size_t len = std::max(a.size(), b.size());
    a.resize(len, 0); b.resize(len, 0);
    for (size_t i = len; i-- > 0;) if (a[i] != b[i]) return a[i] > b[i];
    return false;
}
static uint64_t mulm(uint64_t a, uint64_t b, uint64_t m) { return (uint64_t)((u128)(a % m) * (b % m) % m); }
static uint64_t prod_mod(const std::vector<uint64_t> &base, size_t skip, uint64_t m) {          // prod_{k != skip} base[k] mod m (skip = size: all)
    uint64_t acc = 1 % m;
    for (size_t k = 0; k < base.size(); k++) if (k != skip) acc = mulm(acc, base[k], m);
    return acc;
}
static void fixed_128(uint64_t num, uint64_t q, uint64_t out[2]) {                               // floor(2^128 num / q) for num < q: two steps of a long division
    const u128 hi = ((u128)num << 64) / q, rem = ((u128)num << 64) % q;
    out[1] = (uint64_t)hi; out[0] = (uint64_t)((rem << 64) / q);
}

template <class F>
static int build_lift(fhe_rns_ntt *qp, const std::vector<uint64_t> &B, const std::vector<uint64_t> &C, fhe_dev::BfvLift &T) {
    using E = typename F::E;
    const size_t k = B.size(), kc = C.size();
    std::vector<E> minv(k), mat(k * kc), bmod(kc);
    std::vector<uint64_t> r(2 * k);
    for (size_t i = 0; i < k; i++) {
        minv[i] = word_operand<F>(inv_mod_u64(prod_mod(B, i, B[i]), B[i]), B[i]);
        fixed_128(1, B[i], &r[2 * i]);
        for (size_t j = 0; j < kc; j++) mat[i * kc + j] = word_operand<F>(prod_mod(B, i, C[j]), C[j]);
    }
    for (size_t j = 0; j < kc; j++) bmod[j] = word_operand<F>(prod_mod(B, k, C[j]), C[j]);
    void *d_minv = nullptr, *d_mat = nullptr, *d_bmod = nullptr, *d_r = nullptr;
    int rc;
    if ((rc = upload(qp, minv, &d_minv)) || (rc = upload(qp, mat, &d_mat)) || (rc = upload(qp, bmod, &d_bmod)) || (rc = upload(qp, r, &d_r))) return rc;
    T.minv = d_minv; T.mat = d_mat; T.bmod = d_bmod; T.r = (const uint64_t *)d_r;
    return FHE_OK;
}
template <class F>
static int build_tables(fhe_bfv_multiplier *m, const std::vector<uint64_t> &Q, const std::vector<uint64_t> &P) {
    using E = typename F::E;
    const size_t L = Q.size(), Lp = P.size();
    constexpr unsigned W = (sizeof(E) == 8 && !std::is_same<E, double>::value) ? 64 : 32;       // the words reduce_words cuts R into
    std::vector<E> yinv(L), omega(L * Lp), tq(Lp), pow(3 * Lp);
    std::vector<uint64_t> rho(2 * L);
    for (size_t i = 0; i < L; i++) {
        const uint64_t q = Q[i], P_q = prod_mod(P, Lp, q), theta = mulm(m->t, P_q, q);
        yinv[i] = word_operand<F>(inv_mod_u64(mulm(prod_mod(Q, i, q), P_q, q), q), q);
        fixed_128(theta, q, &rho[2 * i]);
        for (size_t j = 0; j < Lp; j++) {
            const uint64_t p = P[j], v = mulm(theta, inv_mod_u64(q % p, p), p);                  // floor(t P / q_i) = (t P - theta_i) / q_i = -theta_i q_i^-1 (mod p_j)
            omega[i * Lp + j] = word_operand<F>(v ? p - v : 0, p);
        }
    }
    for (size_t j = 0; j < Lp; j++) {
        const uint64_t p = P[j];
        tq[j] = word_operand<F>(mulm(m->t, inv_mod_u64(prod_mod(Q, L, p), p), p), p);
        u128 w = 1;
        for (int k = 0; k < 3; k++) { pow[3 * j + k] = word_operand<F>((uint64_t)(w % p), p); w = ((w % p) << W) % p; }
    }
    void *d_yinv = nullptr, *d_omega = nullptr, *d_tq = nullptr, *d_pow = nullptr, *d_rho = nullptr;
    int rc;
    if ((rc = upload(m->qp, yinv, &d_yinv)) || (rc = upload(m->qp, omega, &d_omega)) || (rc = upload(m->qp, tq, &d_tq)) || (rc = upload(m->qp, pow, &d_pow)) ||
        (rc = upload(m->qp, rho, &d_rho))) return rc;
    m->scale.yinv = d_yinv; m->scale.omega = d_omega; m->scale.tq = d_tq; m->scale.pow = d_pow; m->scale.rho = (const uint64_t *)d_rho;
    if ((rc = build_lift<F>(m->qp, Q, P, m->up))) return rc;
    return build_lift<F>(m->qp, P, Q, m->down);
}

extern "C" int fhe_bfv_multiplier_destroy(fhe_bfv_multiplier_t *m) {
    if (m) {
        if (m->ws.p) (void)hipFree(m->ws.p);
        destroy_impl(m->qp);
        delete m;
    }
    return FHE_OK;
}
extern "C" int fhe_bfv_multiplier_create(fhe_rns_ntt_t *hq, fhe_bfv_multiplier_t **out, uint64_t t, const uint64_t *aux_moduli, uint32_t num_aux) {
    if (!hq || !out || !aux_moduli) return fail(FHE_ERR_INVALID_ARG, "bfv_multiplier_create: null argument");
    if (t < 2) return fail(FHE_ERR_INVALID_ARG, "bfv_multiplier_create: t must be >= 2");
    if (!num_aux) return fail(FHE_ERR_INVALID_ARG, "bfv_multiplier_create: needs at least one auxiliary prime");
    if (!word_sized_moduli(hq)) return fail(FHE_ERR_UNSUPPORTED, "bfv_multiplier_create: every modulus must be below 2^64");
    if (hq->L > (uint32_t)fhe_dev::BFV_MAX_LIMBS || num_aux > (uint32_t)fhe_dev::BFV_MAX_LIMBS)
        return fail(FHE_ERR_UNSUPPORTED, "bfv_multiplier_create: at most 16 ciphertext primes and 16 auxiliary primes");
    if (hq->width == FHE_WIDTH_256) return fail(FHE_ERR_UNSUPPORTED, "bfv_multiplier_create: the ciphertext engine must be of a word-sized width class (n >= 2^11)");
    std::vector<uint64_t> Q(hq->L), P(aux_moduli, aux_moduli + num_aux);
    for (uint32_t i = 0; i < hq->L; i++) Q[i] = hq->moduli[i].w[0];
    for (uint32_t j = 0; j < num_aux; j++) {
        for (uint64_t q : Q) if (P[j] == q) return fail(FHE_ERR_INVALID_ARG, "bfv_multiplier_create: an auxiliary prime equals a ciphertext prime");
        for (uint32_t k = 0; k < j; k++) if (P[j] == P[k]) return fail(FHE_ERR_INVALID_ARG, "bfv_multiplier_create: the auxiliary primes must be pairwise distinct");
        if (P[j] < 2 || (P[j] - 1) % (2 * (uint64_t)hq->n)) return fail(FHE_ERR_INVALID_ARG, "bfv_multiplier_create: an auxiliary prime is not 1 modulo 2n");
    }
    // P > 32 t n Q: the tensor product of two lifted operands (each within Q of its centred value) stays below Q P / 2 in magnitude with room
    // for the rounding, so its residues modulo Q u P determine it
    Big lhs(1, 1), rhs(1, 32);
    for (uint64_t p : P) big_mul(lhs, p);
    big_mul(rhs, t); big_mul(rhs, hq->n);
    for (uint64_t q : Q) big_mul(rhs, q);
    if (!big_greater(lhs, rhs)) return fail(FHE_ERR_INVALID_ARG, "bfv_multiplier_create: the auxiliary primes must multiply to more than 32 t n Q");
    std::vector<std::array<uint64_t, 4>> mods;
    for (uint64_t q : Q) mods.push_back({q, 0, 0, 0});
    for (uint64_t p : P) mods.push_back({p, 0, 0, 0});
    fhe_rns_ntt *qp = nullptr;
    int rc = create_impl(&qp, hq->n, reinterpret_cast<const uint64_t (*)[4]>(mods.data()), (uint32_t)mods.size());   // FHE_ERR_BAD_MODULUS: an auxiliary modulus is not prime
    if (rc) return rc;
    if (qp->width != hq->width) {
        destroy_impl(qp);
        return fail(FHE_ERR_UNSUPPORTED, "bfv_multiplier_create: the auxiliary primes must be of the ciphertext primes' width class (pick them of the same size)");
    }
    fhe_bfv_multiplier *m = new (std::nothrow) fhe_bfv_multiplier();
    if (!m) { destroy_impl(qp); return fail(FHE_ERR_INVALID_ARG, "out of host memory"); }
    m->owner = hq; m->qp = qp; m->t = t; m->L = hq->L; m->Lp = num_aux;
    rc = with_word_field(qp, [&](auto f) { return build_tables<decltype(f)>(m, Q, P); });
    if (rc) { fhe_bfv_multiplier_destroy(m); return rc; }
    *out = m;
    return FHE_OK;
}
extern "C" int fhe_bfv_multiplier_engine(const fhe_bfv_multiplier_t *m, fhe_rns_ntt_t **engine) {
    if (!m || !engine) return fail(FHE_ERR_INVALID_ARG, "bfv_multiplier_engine: null argument");
    *engine = m->qp;
    return FHE_OK;
}
extern "C" int fhe_bfv_multiplier_workspace_bytes(const fhe_bfv_multiplier_t *m, uint64_t *bytes) {
    if (!m || !bytes) return fail(FHE_ERR_INVALID_ARG, "bfv_multiplier_workspace_bytes: null argument");
    *bytes = (uint64_t)m->ws.bytes + m->qp->ws[WS1].bytes + m->qp->ws[WS2].bytes + m->qp->ws[WS3].bytes;
    return FHE_OK;
}

// every call: the handle, the batch rules of both engines, and the extended engine on hq's current stream
static int check_bfv(fhe_bfv_multiplier *m, uint32_t batch, const char *what) {
    if (!m) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": null multiplier");
    int rc = check_call(m->owner, batch, what); if (rc) return rc;
    if ((rc = check_call(m->qp, batch, what))) return rc;
    m->qp->stream = m->owner->stream;
    return FHE_OK;
}
static size_t bytes_q(const fhe_bfv_multiplier *m, uint32_t batch) { return (size_t)batch * m->L * m->owner->n * 32; }
static size_t bytes_qp(const fhe_bfv_multiplier *m, uint32_t batch) { return (size_t)batch * (m->L + m->Lp) * m->owner->n * 32; }
static int ensure_bfv(fhe_bfv_multiplier *m, uint32_t batch) {           // the multiplier's workspace and the tensor product's (both operand forms)
    int rc = ensure_need(m->qp, need_ct_multiply(m->qp, batch, false) | need_ct_multiply(m->qp, batch, true)); if (rc) return rc;
    return grow_ws(m->qp, m->ws, 7 * bytes_qp(m, batch) + bytes_q(m, batch));
}
extern "C" int fhe_bfv_multiplier_reserve(fhe_bfv_multiplier_t *m, uint32_t batch, const fhe_relin_keys_t *rk) {
    int rc = check_bfv(m, batch, "bfv_multiplier_reserve"); if (rc) return rc;
    if (rk && rk->owner != m->owner) return fail(FHE_ERR_INVALID_ARG, "bfv_multiplier_reserve: keys were imported for a different engine");
    if ((rc = ensure_bfv(m, batch))) return rc;
    return rk ? fhe_rns_ntt_reserve(m->owner, batch) : FHE_OK;          // the relinearisation runs on hq's own workspaces
}

static int launch_lift(fhe_bfv_multiplier *m, const fhe_dev::BfvPtrs &ptrs, uint32_t comps, uint32_t batch) {
    fhe_rns_ntt *h = m->qp;
    const size_t per_comp = (size_t)batch * h->n, count = per_comp * comps;
    return with_word_field(h, [&](auto f) {
        using F = decltype(f);
        hipLaunchKernelGGL((fhe_dev::bfv_lift_kernel<F>), dim3(ew_grid(count)), dim3(256), 0, h->stream, ptrs, (const fhe_dev::Limb<F> *)h->d_limbs, m->up, m->L,
                           m->Lp, h->log_n, per_comp, count);
        return post_launch(h->stream, "bfv_lift_kernel");
    });
}
static int launch_scale_round(fhe_bfv_multiplier *m, const fhe_dev::BfvPtrs &ptrs, uint32_t comps, uint32_t batch) {
    fhe_rns_ntt *h = m->qp;
    const size_t per_comp = (size_t)batch * h->n, count = per_comp * comps;
    return with_word_field(h, [&](auto f) {
        using F = decltype(f);
        hipLaunchKernelGGL((fhe_dev::bfv_scale_round_kernel<F>), dim3(ew_grid(count)), dim3(256), 0, h->stream, ptrs, (const fhe_dev::Limb<F> *)h->d_limbs,
                           m->scale, m->down, m->L, m->Lp, h->log_n, per_comp, count);
        return post_launch(h->stream, "bfv_scale_round_kernel");
    });
}

extern "C" int fhe_bfv_lift(fhe_bfv_multiplier_t *m, void *d_out, const void *d_in, uint32_t batch) {
    int rc = check_bfv(m, batch, "bfv_lift"); if (rc) return rc;
    if (!d_out || !d_in) return fail(FHE_ERR_INVALID_ARG, "bfv_lift: null argument");
    if ((rc = check_aligned({d_out, d_in}, "bfv_lift"))) return rc;
    if (overlaps(d_out, bytes_qp(m, batch), d_in, bytes_q(m, batch))) return fail(FHE_ERR_INVALID_ARG, "bfv_lift: the output must not alias the input");
    fhe_dev::BfvPtrs ptrs = {};
    ptrs.in[0] = d_in; ptrs.out[0] = d_out;
    return launch_lift(m, ptrs, 1, batch);
}
extern "C" int fhe_bfv_scale_round(fhe_bfv_multiplier_t *m, void *const *d_out, const void *const *d_in, uint32_t num_components, uint32_t batch) {
    int rc = check_bfv(m, batch, "bfv_scale_round"); if (rc) return rc;
    if (num_components < 1 || num_components > 3) return fail(FHE_ERR_INVALID_ARG, "bfv_scale_round: 1 to 3 components");
    if (!d_out || !d_in) return fail(FHE_ERR_INVALID_ARG, "bfv_scale_round: null argument");
    fhe_dev::BfvPtrs ptrs = {};
    for (uint32_t c = 0; c < num_components; c++) {
        if (!d_out[c] || !d_in[c]) return fail(FHE_ERR_INVALID_ARG, "bfv_scale_round: null component pointer");
        if ((rc = check_aligned({d_out[c], d_in[c]}, "bfv_scale_round"))) return rc;
        ptrs.in[c] = d_in[c]; ptrs.out[c] = d_out[c];
    }
    const size_t ob = bytes_q(m, batch), ib = bytes_qp(m, batch);
    for (uint32_t c = 0; c < num_components; c++) {
        for (uint32_t k = 0; k < num_components; k++)
            if (overlaps(d_out[c], ob, d_in[k], ib)) return fail(FHE_ERR_INVALID_ARG, "bfv_scale_round: an output aliases an input");
        for (uint32_t k = c + 1; k < num_components; k++)
            if (overlaps(d_out[c], ob, d_out[k], ob)) return fail(FHE_ERR_INVALID_ARG, "bfv_scale_round: two outputs overlap");
    }
    return launch_scale_round(m, ptrs, num_components, batch);
}

// lift (one launch for the four operands, two when squaring) -> tensor product over Q u P -> scale and round (one launch) into outs[0 .. 2]
static int bfv_product(fhe_bfv_multiplier *m, void *const outs[3], const void *a0, const void *a1, const void *b0, const void *b1, uint32_t batch) {
    int rc = ensure_bfv(m, batch); if (rc) return rc;                    // (no-op after fhe_bfv_multiplier_reserve)
    const size_t S = bytes_qp(m, batch);
    char *w = (char *)m->ws.p;
    const bool square = a0 == b0 && a1 == b1;                            // same buffers: the tensor product's squaring path
    fhe_dev::BfvPtrs up = {};
    const void *ins[4] = {a0, a1, b0, b1};
    for (int i = 0; i < 4; i++) { up.in[i] = ins[i]; up.out[i] = w + i * S; }
    if ((rc = launch_lift(m, up, square ? 2 : 4, batch))) return rc;
    char *la0 = w, *la1 = w + S, *lb0 = square ? la0 : w + 2 * S, *lb1 = square ? la1 : w + 3 * S, *t0 = w + 4 * S;
    if ((rc = do_ct_multiply(m->qp, t0, t0 + S, t0 + 2 * S, la0, la1, lb0, lb1, batch))) return rc;
    fhe_dev::BfvPtrs down = {};
    for (int c = 0; c < 3; c++) { down.in[c] = t0 + c * S; down.out[c] = outs[c]; }
    return launch_scale_round(m, down, 3, batch);
}
static int check_product_args(std::initializer_list<void *> outs, std::initializer_list<const void *> ins, const char *what) {
    for (void *o : outs) if (!o) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": null argument");
    for (const void *i : ins) if (!i) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": null argument");
    for (void *o : outs) { int rc = check_aligned({o}, what); if (rc) return rc; }
    for (const void *i : ins) { int rc = check_aligned({i}, what); if (rc) return rc; }
    for (void *o : outs) for (const void *i : ins) if (o == i) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": outputs must not alias inputs");
    for (auto a = outs.begin(); a != outs.end(); ++a) for (auto b = a + 1; b != outs.end(); ++b)
        if (*a == *b) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": outputs must be distinct");
    return FHE_OK;
}
extern "C" int fhe_bfv_multiply(fhe_bfv_multiplier_t *m, void *d_c0, void *d_c1, void *d_c2, const void *d_a0, const void *d_a1, const void *d_b0,
                                const void *d_b1, uint32_t batch) {
    int rc = check_bfv(m, batch, "bfv_multiply"); if (rc) return rc;
    if ((rc = check_product_args({d_c0, d_c1, d_c2}, {d_a0, d_a1, d_b0, d_b1}, "bfv_multiply"))) return rc;
    if ((rc = check_inputs(m->owner, {d_a0, d_a1, d_b0, d_b1}, batch))) return rc;
    void *const outs[3] = {d_c0, d_c1, d_c2};
    return bfv_product(m, outs, d_a0, d_a1, d_b0, d_b1, batch);
}
extern "C" int fhe_bfv_multiply_relin(fhe_bfv_multiplier_t *m, const fhe_relin_keys_t *rk, void *d_c0, void *d_c1, const void *d_a0, const void *d_a1,
                                      const void *d_b0, const void *d_b1, uint32_t batch) {
    int rc = check_bfv(m, batch, "bfv_multiply_relin"); if (rc) return rc;
    if (!rk) return fail(FHE_ERR_INVALID_ARG, "bfv_multiply_relin: null argument");
    if ((rc = check_product_args({d_c0, d_c1}, {d_a0, d_a1, d_b0, d_b1}, "bfv_multiply_relin"))) return rc;
    if (rk->owner != m->owner) return fail(FHE_ERR_INVALID_ARG, "bfv_multiply_relin: keys were imported for a different engine");
    if ((rc = check_inputs(m->owner, {d_a0, d_a1, d_b0, d_b1}, batch))) return rc;
    if ((rc = ensure_bfv(m, batch))) return rc;                          // before c2's address is taken
    void *const c2 = (char *)m->ws.p + 7 * bytes_qp(m, batch);
    void *const outs[3] = {d_c0, d_c1, c2};
    if ((rc = bfv_product(m, outs, d_a0, d_a1, d_b0, d_b1, batch))) return rc;
    return fhe_ct_relinearize(m->owner, rk, d_c0, d_c1, c2, batch);
}
