// ckks.hip -- the CKKS encoder (fhe_ckks_encoder_*, fhe_ckks_slot_table, fhe_ckks_encode, fhe_ckks_decode, fhe_ckks_decode_poly): complex slots <->
// real plaintext polynomials on the device (kernels and the definition: ckks.hip.h).  An encoder owns four tables: the slot -> position table
// of the transform, the two twiddle tables (built here in long double, rounded once to double) and one division-free reduction per limb of the
// engine.  Every call is ONE launch without workspace; nothing is allocated after create.
#include "engine.h"

#include <cmath>
#include <type_traits>

#include "ckks.hip.h"

struct fhe_ckks_encoder {
    fhe_rns_ntt *owner = nullptr;
    void *d_gather = nullptr;                       // uint32_t[n/2]: bitrev(a(k)) | c(k) << 31
    void *d_twist = nullptr;                        // double2[n/2]: zeta^j
    void *d_omega = nullptr;                        // double2[n/4]: omega^i
    void *d_red = nullptr;                          // ModT[L] of q_l
    uint64_t q0 = 0;
};

// a(k), c(k) of slot k: e(k) = 3^k mod 2n is 4 a + 1 (c = 0), or 2n - e(k) is (c = 1)
static int ckks_slot_table(uint32_t n, uint32_t *a_of_slot, uint8_t *conj_of_slot) {
    if (n < 2 || (n & (n - 1)) || n > (1u << 30)) return fail(FHE_ERR_INVALID_ARG, "ckks slot table: n must be a power of two in [2, 2^30]");
    const uint32_t mask = 2 * n - 1;
    uint32_t e = 1;
    for (uint32_t k = 0; k < n / 2; k++) {
        const bool c = (e & 3) != 1;
        a_of_slot[k] = ((c ? 2 * n - e : e) - 1) / 4;
        conj_of_slot[k] = c ? 1 : 0;
        e = (uint32_t)(((uint64_t)e * 3) & mask);
    }
    return FHE_OK;
}
extern "C" int fhe_ckks_slot_table(uint32_t n, uint32_t *a_of_slot, uint8_t *conj_of_slot) {
    if (!a_of_slot || !conj_of_slot) return fail(FHE_ERR_INVALID_ARG, "ckks slot table: null argument");
    return ckks_slot_table(n, a_of_slot, conj_of_slot);
}

extern "C" int fhe_ckks_encoder_destroy(fhe_ckks_encoder_t *enc) {
    if (enc) {
        for (void *d : {enc->d_gather, enc->d_twist, enc->d_omega, enc->d_red}) if (d) (void)hipFree(d);
        delete enc;
    }
    return FHE_OK;
}

template <class T>
static int own_table(const std::vector<T> &v, void **out) {
    HIP_TRY(hipMalloc(out, v.size() * sizeof(T)));
    HIP_TRY(hipMemcpy(*out, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return FHE_OK;
}
// exp(i pi num / den) for 0 <= num <= den, den a power of two: the angle is folded into [0, pi/4] first, where cosl / sinl are at their best
static double2 unit_root(uint32_t num, uint32_t den) {
    const long double pi = 3.14159265358979323846264338327950288L;
    const bool reflect = num > den / 2;                                  // pi - x
    uint32_t x = reflect ? den - num : num;                              // [0, pi/2]
    const bool swap = x > den / 4;                                       // pi/2 - x
    if (swap) x = den / 2 - x;
    long double c = cosl(pi * x / den), s = sinl(pi * x / den);
    if (swap) std::swap(c, s);
    if (reflect) c = -c;
    return double2{(double)c, (double)s};
}

extern "C" int fhe_ckks_encoder_create(fhe_rns_ntt_t *h, fhe_ckks_encoder_t **out) {
    if (!h || !out) return fail(FHE_ERR_INVALID_ARG, "ckks_encoder_create: null argument");
    if (h->log_n < 11 || h->log_n > 14) return fail(FHE_ERR_UNSUPPORTED, "ckks_encoder_create: supported for n = 2^11 .. 2^14 (one workgroup holds the transform)");
    if (!word_sized_moduli(h)) return fail(FHE_ERR_UNSUPPORTED, "ckks_encoder_create: every modulus must be below 2^64");
    const uint32_t n = h->n, half = n / 2;
    std::vector<uint32_t> a(half), gather(half);
    std::vector<uint8_t> c(half);
    int rc = ckks_slot_table(n, a.data(), c.data()); if (rc) return rc;
    for (uint32_t k = 0; k < half; k++) gather[k] = fhe_host::bitrev(a[k], h->log_n - 1) | (c[k] ? fhe_dev::CKKS_CONJ : 0u);
    std::vector<double2> twist(half), omega(half / 2);
    for (uint32_t j = 0; j < half; j++) twist[j] = unit_root(j, n);                       // zeta^j = exp(i pi j / n)
    for (uint32_t i = 0; i < half / 2; i++) omega[i] = unit_root(4 * i, n);               // omega^i = zeta^(4 i)
    std::vector<fhe_host::ModT> red(h->L);
    for (uint32_t l = 0; l < h->L; l++)
        if (!fhe_host::modt_init(red[l], h->moduli[l].w[0])) return fail(FHE_ERR_BAD_MODULUS, "ckks_encoder_create: modulus below 2");
    fhe_ckks_encoder *enc = new (std::nothrow) fhe_ckks_encoder();
    if (!enc) return fail(FHE_ERR_INVALID_ARG, "out of host memory");
    enc->owner = h; enc->q0 = h->moduli[0].w[0];
    if (!(rc = own_table(gather, &enc->d_gather)) && !(rc = own_table(twist, &enc->d_twist)) && !(rc = own_table(omega, &enc->d_omega)))
        rc = own_table(red, &enc->d_red);
    if (rc) { fhe_ckks_encoder_destroy(enc); return rc; }
    *out = enc;
    return FHE_OK;
}

static int check_ckks(const fhe_rns_ntt *h, const fhe_ckks_encoder *enc, double scale, uint32_t batch, const char *what) {
    int rc = check_call(h, batch, what); if (rc) return rc;
    if (!enc) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": null encoder");
    if (enc->owner != h) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": the encoder was created for a different engine");
    if (!std::isfinite(scale) || !(scale > 0)) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": scale must be finite and positive");
    return FHE_OK;
}
// fn(std::integral_constant<int, log_n>) for the encoder's size
template <class Fn>
static int with_ckks_size(const fhe_rns_ntt *h, Fn &&fn) {
    switch (h->log_n) {
        case 11: return fn(std::integral_constant<int, 11>{});
        case 12: return fn(std::integral_constant<int, 12>{});
        case 13: return fn(std::integral_constant<int, 13>{});
        case 14: return fn(std::integral_constant<int, 14>{});
        default: return fail(FHE_ERR_UNSUPPORTED, "ckks: n outside 2^11 .. 2^14");
    }
}

extern "C" int fhe_ckks_encode(fhe_rns_ntt_t *h, const fhe_ckks_encoder_t *enc, void *d_out, uint32_t *d_coeff_bits, const double *d_slots, double scale,
                               uint32_t batch) {
    int rc = check_ckks(h, enc, scale, batch, "ckks_encode"); if (rc) return rc;
    if (!d_out || !d_slots) return fail(FHE_ERR_INVALID_ARG, "ckks_encode: null argument");
    if ((rc = check_aligned({d_out}, "ckks_encode"))) return rc;
    if ((uintptr_t)d_slots & 7) return fail(FHE_ERR_INVALID_ARG, "ckks_encode: d_slots must be 8-byte aligned");
    if ((uintptr_t)d_coeff_bits & 3) return fail(FHE_ERR_INVALID_ARG, "ckks_encode: d_coeff_bits must be 4-byte aligned");
    const size_t count = (size_t)batch * h->n, out_bytes = count * h->L * 32;
    if (overlaps(d_out, out_bytes, d_slots, count * 8)) return fail(FHE_ERR_INVALID_ARG, "ckks_encode: the output must not alias the input");
    if (d_coeff_bits && (overlaps(d_coeff_bits, (size_t)batch * 4, d_slots, count * 8) || overlaps(d_coeff_bits, (size_t)batch * 4, d_out, out_bytes)))
        return fail(FHE_ERR_INVALID_ARG, "ckks_encode: d_coeff_bits must not alias the slots or the output");
    const double scale_over_h = scale / (double)(h->n / 2);               // exact: h is a power of two
    return with_ckks_size(h, [&](auto logn) {
        using C = fhe_dev::CkksCfg<decltype(logn)::value>;
        hipLaunchKernelGGL(fhe_dev::ckks_encode_kernel<decltype(logn)::value>, dim3(batch), dim3(C::T), 0, h->stream, (char *)d_out, d_coeff_bits, d_slots,
                           (const uint32_t *)enc->d_gather, (const double2 *)enc->d_twist, (const double2 *)enc->d_omega, (const fhe_host::ModT *)enc->d_red,
                           scale_over_h, h->L);
        return post_launch(h->stream, "ckks_encode_kernel");
    });
}

static int ckks_decode(fhe_rns_ntt *h, const fhe_ckks_encoder *enc, double *d_slots, const void *d_src, bool containers, uint64_t t, double scale, uint32_t batch,
                       const char *what) {
    int rc = check_ckks(h, enc, scale, batch, what); if (rc) return rc;
    if (!d_slots || !d_src) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": null argument");
    if ((uintptr_t)d_slots & 7) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": d_slots must be 8-byte aligned");
    if (containers) { if ((rc = check_aligned({d_src}, what))) return rc; }
    else if ((uintptr_t)d_src & 7) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": d_m must be 8-byte aligned");
    const size_t count = (size_t)batch * h->n;
    if (overlaps(d_slots, count * 8, d_src, containers ? count * h->L * 32 : count * 8)) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": the output must not alias the input");
    const double inv_scale = 1.0 / scale;
    return with_ckks_size(h, [&](auto logn) {
        constexpr int LOGN = decltype(logn)::value;
        using C = fhe_dev::CkksCfg<LOGN>;
        if (containers)
            hipLaunchKernelGGL((fhe_dev::ckks_decode_kernel<LOGN, 1>), dim3(batch), dim3(C::T), 0, h->stream, d_slots, (const char *)d_src, (const uint32_t *)enc->d_gather,
                               (const double2 *)enc->d_twist, (const double2 *)enc->d_omega, enc->q0, inv_scale, h->L);
        else
            hipLaunchKernelGGL((fhe_dev::ckks_decode_kernel<LOGN, 0>), dim3(batch), dim3(C::T), 0, h->stream, d_slots, (const char *)d_src, (const uint32_t *)enc->d_gather,
                               (const double2 *)enc->d_twist, (const double2 *)enc->d_omega, t, inv_scale, h->L);
        return post_launch(h->stream, "ckks_decode_kernel");
    });
}
extern "C" int fhe_ckks_decode(fhe_rns_ntt_t *h, const fhe_ckks_encoder_t *enc, double *d_slots, const uint64_t *d_m, uint64_t t, double scale, uint32_t batch) {
    return ckks_decode(h, enc, d_slots, d_m, false, t, scale, batch, "ckks_decode");
}
extern "C" int fhe_ckks_decode_poly(fhe_rns_ntt_t *h, const fhe_ckks_encoder_t *enc, double *d_slots, const void *d_poly, double scale, uint32_t batch) {
    return ckks_decode(h, enc, d_slots, d_poly, true, 0, scale, batch, "ckks_decode_poly");
}
