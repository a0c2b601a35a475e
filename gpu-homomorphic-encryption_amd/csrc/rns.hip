// rns.hip -- RNS entry / exit: CRT tables, to / from RNS, rescale, BGV modulus switch, fast base conversion.
#include "engine.h"

#include <type_traits>

#include "ntt256_rns.hip.h"
#include "ntt_word.hip.h"

static bool mul_checked(U256 &r, const U256 &a, const U256 &b) {      // r = a*b, false on overflow beyond 256 bits
    uint64_t t[8] = {0};
    for (int i = 0; i < 4; i++) {
        uint64_t carry = 0;
        for (int j = 0; j < 4; j++) {
            fhe_host::u128 acc = (fhe_host::u128)a.w[i] * b.w[j] + t[i + j] + carry;
            t[i + j] = (uint64_t)acc; carry = (uint64_t)(acc >> 64);
        }
        t[i + 4] = carry;
    }
    std::memcpy(r.w, t, 32);
    return !(t[4] | t[5] | t[6] | t[7]);
}
int ensure_crt(fhe_rns_ntt *h) {
    if (h->crt_state) return FHE_OK;
    const uint32_t L = h->L;
    U256 Q(1); bool fits = true;
    for (uint32_t l = 0; l < L && fits; l++) { U256 t; fits = mul_checked(t, Q, h->moduli[l]); Q = t; }
    fits = fits && !(Q.w[3] >> 63);
    std::vector<fhe_dev::CrtLimb> limbs(L);
    std::memset(limbs.data(), 0, L * sizeof(fhe_dev::CrtLimb));
    for (uint32_t l = 0; l < L; l++) {
        fhe_host::Mod M(h->moduli[l]);
        std::memcpy(limbs[l].q.l, M.q.w, 32); std::memcpy(limbs[l].r2.l, M.r2.w, 32); limbs[l].inv0 = M.inv0;
        // ((Q/q)^-1 mod q) * R from the other primes modulo q: the fast base conversion needs it for ANY basis, also one whose product Q
        // does not fit a container (only from_rns needs Q itself)
        U256 Mi_m = M.r1;
        for (uint32_t k = 0; k < L; k++) if (k != l) Mi_m = M.mont(Mi_m, M.to_mont(M.reduce(h->moduli[k])));
        U256 qm2; fhe_host::sub_to(qm2, M.q, U256(2));
        const U256 minv_m = M.pow_m(Mi_m, qm2);
        std::memcpy(limbs[l].minv_m.l, minv_m.w, 32);
    }
    if (fits) {
        fhe_host::Mod MQ(Q);
        for (uint32_t l = 0; l < L; l++) {
            U256 Mi(1);
            for (uint32_t k = 0; k < L; k++) if (k != l) { U256 t; mul_checked(t, Mi, h->moduli[k]); Mi = t; }
            const U256 Mi_mQ = MQ.to_mont(Mi);
            std::memcpy(limbs[l].Mi_mQ.l, Mi_mQ.w, 32);
        }
        std::memcpy(h->crt_big.Q.l, Q.w, 32); h->crt_big.inv0 = MQ.inv0; h->crt_big._pad = 0;
    }
    int rc = upload(h, limbs, &h->d_crt); if (rc) return rc;
    h->crt_state = fits ? 1 : -1;
    return FHE_OK;
}
template <class F>
static int to_rns_word(fhe_rns_ntt *h, void *d_rns, const void *d_values, uint32_t batch) {
    using E = typename F::E; using V = typename F::V16;
    using WT = typename std::conditional<std::is_same<E, uint64_t>::value, uint64_t, uint32_t>::type;   // the word the value is cut into (FP64 field: 32-bit words)
    constexpr uint32_t NW = 32 / sizeof(WT), W = 8 * sizeof(WT);
    if (!h->d_to_rns_w) {
        std::vector<E> ops((size_t)h->L * NW);
        for (uint32_t l = 0; l < h->L; l++) {
            const uint64_t q = h->moduli[l].w[0];
            fhe_host::u128 p = 1 % q;
            for (uint32_t k = 0; k < NW; k++) {
                ops[(size_t)l * NW + k] = word_operand<F>((uint64_t)p, q);
                for (uint32_t t = 0; t < W; t++) p = (p << 1) % q;              // 2^(W (k+1)) mod q
            }
        }
        int rc = upload(h, ops, &h->d_to_rns_w); if (rc) return rc;
    }
    const size_t containers = (size_t)batch * h->L * h->n;
    hipLaunchKernelGGL((fhe_dev::to_rns_word_kernel<F, WT>), dim3(ew_grid(containers)), dim3(256), 0, h->stream, (V *)d_rns, (const V *)d_values,
                       (const fhe_dev::Limb<F> *)h->d_limbs, (const E *)h->d_to_rns_w, h->L, h->log_n, containers);
    return post_launch(h->stream, "to_rns_word_kernel");
}
extern "C" int fhe_rns_to_rns(fhe_rns_ntt_t *h, void *d_rns, const void *d_values, uint32_t batch) {
    int rc = check_call(h, batch, "to_rns"); if (rc) return rc;
    if (!d_rns || !d_values || d_rns == d_values) return fail(FHE_ERR_INVALID_ARG, "to_rns: null or aliased argument");
    if ((rc = check_aligned({d_rns, d_values}, "to_rns"))) return rc;
    // (to_rns_word_kernel stores through lane pairs of WHOLE waves, store_wave_containers: every wave must cover 64 consecutive containers
    //  of one polynomial, i.e. n a multiple of 256.  Word-sized classes exist from n = 2^11, the guard keeps that an explicit condition.)
    if (h->width != FHE_WIDTH_256 && !h->env.no_word_conversions && h->log_n >= 8)       // word-sized classes: a streaming kernel on the field type
        return with_word_field(h, [&](auto f) { return to_rns_word<decltype(f)>(h, d_rns, d_values, batch); });
    if ((rc = ensure_crt(h))) return rc;
    const size_t count = (size_t)batch * h->n;
    hipLaunchKernelGGL(fhe_dev::to_rns_kernel, dim3(ew_grid(count)), dim3(256), 0, h->stream, (fhe_dev::u256 *)d_rns, (const fhe_dev::u256 *)d_values,
                       (const fhe_dev::CrtLimb *)h->d_crt, h->L, h->log_n, count);
    return post_launch(h->stream, "to_rns_kernel");
}
// The CRT operands of the word-sized classes: ((Q / q_l)^-1 mod q_l) as pw operands and Q / q_l as plain integers (Q < 2^255: the callers check)
int ensure_from_rns_word(fhe_rns_ntt *h) {
    if (h->d_from_rns_w_minv) return FHE_OK;
    return with_word_field(h, [&](auto f) {
        using F = decltype(f); using E = typename F::E;
        const uint32_t L = h->L;
        std::vector<E> minv(L); std::vector<fhe_dev::u256> Ms(L);
        for (uint32_t l = 0; l < L; l++) {
            const uint64_t q = h->moduli[l].w[0];
            U256 Mi(1); fhe_host::u128 Mi_mod_q = 1;
            for (uint32_t k = 0; k < L; k++) if (k != l) { U256 t; mul_checked(t, Mi, h->moduli[k]); Mi = t; Mi_mod_q = Mi_mod_q * (h->moduli[k].w[0] % q) % q; }
            minv[l] = word_operand<F>(inv_mod_u64((uint64_t)Mi_mod_q, q), q);
            std::memcpy(Ms[l].l, Mi.w, 32);
        }
        void *d_minv = nullptr;
        int rc;
        if ((rc = upload(h, minv, &d_minv)) || (rc = upload(h, Ms, &h->d_from_rns_w_M))) return rc;
        h->d_from_rns_w_minv = d_minv;                 // set last: the pair is there or neither is
        return (int)FHE_OK;
    });
}
template <class F>
static int from_rns_word(fhe_rns_ntt *h, void *d_values, const void *d_rns, uint32_t batch) {
    using E = typename F::E; using V = typename F::V16;
    if (int rc = ensure_from_rns_word(h)) return rc;
    const size_t count = (size_t)batch * h->n;
    hipLaunchKernelGGL((fhe_dev::from_rns_word_kernel<F>), dim3(ew_grid(count)), dim3(256), 0, h->stream, (fhe_dev::u256 *)d_values, (const V *)d_rns,
                       (const fhe_dev::Limb<F> *)h->d_limbs, (const E *)h->d_from_rns_w_minv, (const fhe_dev::u256 *)h->d_from_rns_w_M, h->crt_big.Q,
                       h->L, h->log_n, count);
    return post_launch(h->stream, "from_rns_word_kernel");
}
extern "C" int fhe_rns_from_rns(fhe_rns_ntt_t *h, void *d_values, const void *d_rns, uint32_t batch) {
    int rc = check_call(h, batch, "from_rns"); if (rc) return rc;
    if (!d_rns || !d_values || d_rns == d_values) return fail(FHE_ERR_INVALID_ARG, "from_rns: null or aliased argument");
    if ((rc = check_aligned({d_rns, d_values}, "from_rns"))) return rc;
    if ((rc = ensure_crt(h))) return rc;
    if (h->crt_state < 0) return fail(FHE_ERR_UNSUPPORTED, "from_rns: the product of the moduli must be below 2^255 to fit a 256-bit container");
    if (h->width != FHE_WIDTH_256 && !h->env.no_word_conversions)       // word-sized classes: word x 256-bit accumulation instead of 256-bit Montgomery products
        return with_word_field(h, [&](auto f) { return from_rns_word<decltype(f)>(h, d_values, d_rns, batch); });
    const size_t count = (size_t)batch * h->n;
    hipLaunchKernelGGL(fhe_dev::from_rns_kernel, dim3(ew_grid(count)), dim3(256), 0, h->stream, (fhe_dev::u256 *)d_values, (const fhe_dev::u256 *)d_rns,
                       (const fhe_dev::CrtLimb *)h->d_crt, h->crt_big, h->L, h->log_n, count);
    return post_launch(h->stream, "from_rns_kernel");
}


template <class F>
static int rescale_word(fhe_rns_ntt *h, void *d_out, const void *d_in, uint32_t batch) {
    using E = typename F::E; using V = typename F::V16;
    if (!h->d_rescale_w) {
        std::vector<E> ops(h->L - 1);
        const uint64_t ql = h->moduli[h->L - 1].w[0];
        for (uint32_t l = 0; l + 1 < h->L; l++) { const uint64_t q = h->moduli[l].w[0]; ops[l] = word_operand<F>(inv_mod_u64(ql % q, q), q); }
        int rc = upload(h, ops, &h->d_rescale_w); if (rc) return rc;
    }
    const size_t count = (size_t)batch * h->n;
    hipLaunchKernelGGL((fhe_dev::rescale_word_kernel<F>), dim3(ew_grid(count)), dim3(256), 0, h->stream, (V *)d_out, (const V *)d_in,
                       (const fhe_dev::Limb<F> *)h->d_limbs, (const E *)h->d_rescale_w, h->L, h->log_n, count);
    return post_launch(h->stream, "rescale_word_kernel");
}
template <class F>
static int base_convert_word(fhe_rns_ntt *h, fhe_rns_ntt *t, void *d_out, const void *d_in, uint32_t batch) {
    using E = typename F::E; using V = typename F::V16;
    if (h->bconv_w_target != t || !(h->bconv_w_moduli == t->moduli)) {
        const uint32_t L = h->L, Lp = t->L;
        std::vector<E> minv(L), mat((size_t)L * Lp);
        for (uint32_t i = 0; i < L; i++) {
            const uint64_t qi = h->moduli[i].w[0];
            fhe_host::u128 Mi = 1;
            for (uint32_t k = 0; k < L; k++) if (k != i) Mi = Mi * (h->moduli[k].w[0] % qi) % qi;
            minv[i] = word_operand<F>(inv_mod_u64((uint64_t)Mi, qi), qi);
            for (uint32_t j = 0; j < Lp; j++) {
                const uint64_t pj = t->moduli[j].w[0];
                fhe_host::u128 m = 1;
                for (uint32_t k = 0; k < L; k++) if (k != i) m = m * (h->moduli[k].w[0] % pj) % pj;
                mat[(size_t)i * Lp + j] = word_operand<F>((uint64_t)m, pj);
            }
        }
        int rc;
        if ((rc = upload(h, minv, &h->d_bconv_w_minv)) || (rc = upload(h, mat, &h->d_bconv_w_mat))) return rc;   // earlier tables stay owned by d_tables
        h->bconv_w_target = t; h->bconv_w_moduli = t->moduli;
    }
    constexpr bool all_lanes = std::is_same<F, fhe_dev::F64>::value || std::is_same<F, fhe_dev::F64X>::value;
    const size_t work = (size_t)batch * t->L * h->n * (all_lanes ? 1 : 2);
    hipLaunchKernelGGL((fhe_dev::base_convert_word_kernel<F, all_lanes>), dim3(ew_grid(work)), dim3(256), 0, h->stream, (V *)d_out, (const V *)d_in,
                       (const fhe_dev::Limb<F> *)h->d_limbs, h->L, (const fhe_dev::Limb<F> *)t->d_limbs, t->L, (const E *)h->d_bconv_w_minv,
                       (const E *)h->d_bconv_w_mat, h->log_n, work);
    return post_launch(h->stream, "base_convert_word_kernel");
}

extern "C" int fhe_rns_rescale_drop_last(fhe_rns_ntt_t *h, void *d_out, const void *d_in, uint32_t batch) {
    int rc = check_call(h, batch, "rescale_drop_last"); if (rc) return rc;
    if (!d_out || !d_in || d_out == d_in) return fail(FHE_ERR_INVALID_ARG, "rescale_drop_last: null or aliased argument");
    if ((rc = check_aligned({d_out, d_in}, "rescale_drop_last"))) return rc;
    if (h->L < 2) return fail(FHE_ERR_INVALID_ARG, "rescale_drop_last: needs at least two primes");
    if (h->width != FHE_WIDTH_256 && !h->env.no_word_conversions)       // word-sized classes: streaming kernels on the field type
        return with_word_field(h, [&](auto f) { return rescale_word<decltype(f)>(h, d_out, d_in, batch); });
    if ((rc = ensure_crt(h))) return rc;
    if (!h->d_rescale) {
        std::vector<fhe_dev::RescaleLimb> rs(h->L - 1);
        const U256 &ql = h->moduli[h->L - 1];
        for (uint32_t l = 0; l + 1 < h->L; l++) {
            fhe_host::Mod M(h->moduli[l]);
            U256 qm2; fhe_host::sub_to(qm2, M.q, U256(2));
            U256 inv_m = M.pow_m(M.to_mont(M.reduce(ql)), qm2);                    // (q_last^-1 mod q_l) * R
            std::memcpy(rs[l].qlast_inv_m.l, inv_m.w, 32);
        }
        if ((rc = upload(h, rs, &h->d_rescale))) return rc;
    }
    const size_t count = (size_t)batch * h->n;
    hipLaunchKernelGGL(fhe_dev::rescale_drop_last_kernel, dim3(ew_grid(count)), dim3(256), 0, h->stream, (fhe_dev::u256 *)d_out,
                       (const fhe_dev::u256 *)d_in, (const fhe_dev::CrtLimb *)h->d_crt, (const fhe_dev::RescaleLimb *)h->d_rescale, h->L, h->log_n, count);
    return post_launch(h->stream, "rescale_drop_last_kernel");
}


// ---- BGV modulus switch ---------------------------------------------------------------------------------------------------------
static void *find_mod_switch_table(const fhe_rns_ntt *h, uint64_t t) {
    for (const auto &e : h->mod_switch_tables) if (e.first == t) return e.second;
    return nullptr;
}
template <class F>
static int mod_switch_word(fhe_rns_ntt *h, uint64_t t, const fhe_dev::ModSwitchPtrs &ptrs, uint32_t comps, uint32_t batch) {
    using E = typename F::E;
    void *d_ops = find_mod_switch_table(h, t);
    if (!d_ops) {
        const uint32_t L = h->L;
        std::vector<E> ops(2 * (size_t)L - 1);
        const uint64_t ql = h->moduli[L - 1].w[0];
        ops[0] = word_operand<F>(ql - inv_mod_u64(t % ql, ql), ql);                          // -t^-1 mod q_last (t != 0 mod q_last: checked by the caller)
        for (uint32_t l = 0; l + 1 < L; l++) {
            const uint64_t q = h->moduli[l].w[0], inv = inv_mod_u64(ql % q, q);
            ops[1 + 2 * l] = word_operand<F>(inv, q);
            ops[2 + 2 * l] = word_operand<F>((uint64_t)((fhe_host::u128)(t % q) * inv % q), q);   // t reduced here: it may exceed q_l
        }
        int rc = upload(h, ops, &d_ops); if (rc) return rc;
        h->mod_switch_tables.emplace_back(t, d_ops);
    }
    const size_t per_comp = (size_t)batch * h->n, count = per_comp * comps;
    hipLaunchKernelGGL((fhe_dev::mod_switch_word_kernel<F>), dim3(ew_grid(count)), dim3(256), 0, h->stream, ptrs, (const fhe_dev::Limb<F> *)h->d_limbs,
                       (const E *)d_ops, h->L, h->log_n, per_comp, count);
    return post_launch(h->stream, "mod_switch_word_kernel");
}
extern "C" int fhe_ct_mod_switch_drop_last(fhe_rns_ntt_t *h, uint64_t t, void *const *d_out, const void *const *d_in, uint32_t num_components,
                                           uint32_t batch) {
    int rc = check_call(h, batch, "ct_mod_switch_drop_last"); if (rc) return rc;
    if (num_components < 1 || num_components > 3) return fail(FHE_ERR_INVALID_ARG, "ct_mod_switch_drop_last: 1 to 3 components");
    if (!d_out || !d_in) return fail(FHE_ERR_INVALID_ARG, "ct_mod_switch_drop_last: null argument");
    fhe_dev::ModSwitchPtrs ptrs = {};
    for (uint32_t c = 0; c < num_components; c++) {
        if (!d_out[c] || !d_in[c]) return fail(FHE_ERR_INVALID_ARG, "ct_mod_switch_drop_last: null component pointer");
        if ((rc = check_aligned({d_out[c], d_in[c]}, "ct_mod_switch_drop_last"))) return rc;
        ptrs.in[c] = d_in[c]; ptrs.out[c] = d_out[c];
    }
    for (uint32_t c = 0; c < num_components; c++) {
        for (uint32_t k = 0; k < num_components; k++)
            if (d_out[c] == d_in[k]) return fail(FHE_ERR_INVALID_ARG, "ct_mod_switch_drop_last: an output aliases an input");
        for (uint32_t k = c + 1; k < num_components; k++)
            if (d_out[c] == d_out[k]) return fail(FHE_ERR_INVALID_ARG, "ct_mod_switch_drop_last: two outputs are the same buffer");
    }
    if (h->L < 2) return fail(FHE_ERR_INVALID_ARG, "ct_mod_switch_drop_last: needs at least two primes");
    if (t < 2) return fail(FHE_ERR_INVALID_ARG, "ct_mod_switch_drop_last: t must be >= 2");
    const U256 &ql = h->moduli[h->L - 1];
    if (!(ql.w[1] | ql.w[2] | ql.w[3]) && t % ql.w[0] == 0)                                   // a wider q_last exceeds any 64-bit t
        return fail(FHE_ERR_INVALID_ARG, "ct_mod_switch_drop_last: t must be invertible modulo the last prime");
    if (h->width != FHE_WIDTH_256 && !h->env.no_word_conversions)       // word-sized classes: a streaming kernel on the field type
        return with_word_field(h, [&](auto f) { return mod_switch_word<decltype(f)>(h, t, ptrs, num_components, batch); });
    if ((rc = ensure_crt(h))) return rc;
    void *d_ms = find_mod_switch_table(h, t);
    if (!d_ms) {
        const uint32_t L = h->L;
        std::vector<fhe_dev::ModSwitchLimb> ms(L);
        std::memset(ms.data(), 0, L * sizeof(fhe_dev::ModSwitchLimb));
        {
            fhe_host::Mod M(ql);
            U256 qm2; fhe_host::sub_to(qm2, M.q, U256(2));
            const U256 tinv_m = M.pow_m(M.to_mont(M.reduce(U256(t))), qm2);                  // (t^-1 mod q_last) * R
            const U256 neg_m = M.sub(U256(), tinv_m);
            std::memcpy(ms[L - 1].qlast_inv_m.l, neg_m.w, 32);
        }
        for (uint32_t l = 0; l + 1 < L; l++) {
            fhe_host::Mod M(h->moduli[l]);
            U256 qm2; fhe_host::sub_to(qm2, M.q, U256(2));
            const U256 inv_m = M.pow_m(M.to_mont(M.reduce(ql)), qm2);                        // (q_last^-1 mod q_l) * R
            const U256 t_inv = M.mont(M.reduce(U256(t)), inv_m);                             // t * q_last^-1 mod q_l, plain
            std::memcpy(ms[l].qlast_inv_m.l, inv_m.w, 32); std::memcpy(ms[l].t_qlast_inv.l, t_inv.w, 32);
        }
        if ((rc = upload(h, ms, &d_ms))) return rc;
        h->mod_switch_tables.emplace_back(t, d_ms);
    }
    const size_t per_comp = (size_t)batch * h->n, count = per_comp * num_components;
    hipLaunchKernelGGL(fhe_dev::mod_switch_drop_last_kernel, dim3(ew_grid(count)), dim3(256), 0, h->stream, ptrs, (const fhe_dev::CrtLimb *)h->d_crt,
                       (const fhe_dev::ModSwitchLimb *)d_ms, h->L, h->log_n, per_comp, count);
    return post_launch(h->stream, "mod_switch_drop_last_kernel");
}

extern "C" int fhe_rns_fast_base_convert(fhe_rns_ntt_t *h, fhe_rns_ntt_t *target, void *d_out, const void *d_in, uint32_t batch) {
    int rc = check_call(h, batch, "fast_base_convert"); if (rc) return rc;
    if (!target || !d_out || !d_in || d_out == d_in) return fail(FHE_ERR_INVALID_ARG, "fast_base_convert: null or aliased argument");
    if ((rc = check_aligned({d_out, d_in}, "fast_base_convert"))) return rc;
    if (target->n != h->n) return fail(FHE_ERR_INVALID_ARG, "fast_base_convert: source and target engines differ in degree");
    if (h->width == target->width && h->width != FHE_WIDTH_256 && !h->env.no_word_conversions && h->log_n >= 8)   // whole waves per polynomial, as in to_rns
        return with_word_field(h, [&](auto f) { return base_convert_word<decltype(f)>(h, target, d_out, d_in, batch); });
    if ((rc = ensure_crt(h)) || (rc = ensure_crt(target))) return rc;
    if (h->bconv_target != target || !(h->bconv_moduli == target->moduli)) {
        std::vector<fhe_dev::u256> mat((size_t)h->L * target->L);
        for (uint32_t j = 0; j < target->L; j++) {
            fhe_host::Mod M(target->moduli[j]);
            for (uint32_t i = 0; i < h->L; i++) {
                U256 acc = M.r1;                                              // prod_{k != i} q_k mod p_j, Montgomery form
                for (uint32_t k = 0; k < h->L; k++) if (k != i) acc = M.mont(acc, M.to_mont(M.reduce(h->moduli[k])));
                std::memcpy(mat[(size_t)i * target->L + j].l, acc.w, 32);
            }
        }
        if ((rc = upload(h, mat, &h->d_bconv))) return rc;                    // earlier matrices stay owned by d_tables until destroy
        h->bconv_target = target; h->bconv_moduli = target->moduli;
    }
    const size_t count = (size_t)batch * h->n;
    hipLaunchKernelGGL(fhe_dev::fast_base_convert_kernel, dim3(ew_grid(count)), dim3(256), 0, h->stream, (fhe_dev::u256 *)d_out,
                       (const fhe_dev::u256 *)d_in, (const fhe_dev::CrtLimb *)h->d_crt, h->L, (const fhe_dev::CrtLimb *)target->d_crt, target->L,
                       (const fhe_dev::u256 *)h->d_bconv, h->log_n, count);
    return post_launch(h->stream, "fast_base_convert_kernel");
}
