// keygen.hip -- key-switching key generation and key export (fhe_keyswitch_keys_generate, fhe_relin_keys_export).
// Fused path (plan_fused_keygen, a secret key with packed transforms, a cumulative table that fits the kernel; kernel: keygen.hip.h): the
// packed tables of every set are allocated, a table of (tables, Galois element) per set is uploaded and ONE launch fills them all; the
// Galois targets are gathered in the kernel from the packed transform of s.
// Composed path (everything else), one key set at a time: the uniform residues go straight into the set's `a` containers, which are
// NTT-domain by definition (sample_uniform_from); keygen_noise_kernel writes [noise_scale e] into the `b` containers, which are transformed;
// a^ . s^ row by row (do_ew) into scratch and one subtraction; keygen_gadget_kernel adds 2^(k w) target^ in limb j; then the set is packed
// where keys_get_packed says so, exactly as fhe_relin_keys_create does.  Scratch: s^, target^ and the L K products, (L K + 2) S bytes.
#include "engine.h"

#include <cmath>

#include "ctr_rand.hip.h"
#include "ntt_word.hip.h"

namespace fhe_dev {

// out[r][l][x] = [noise_scale e_P[x]]_{q_l}, P = first + r, on containers of any width class; one lane per (row, coefficient), the same small
// integer in every limb.  e is the draw of sample_small_kernel<1> for element P n + x; noise_scale |e| mod q_l by double-and-add (no division).
__global__ void __launch_bounds__(256)
keygen_noise_kernel(u256 *__restrict__ out, const CrtLimb *__restrict__ limbs, uint32_t L, uint32_t log_n, uint64_t seed, uint64_t noise_scale,
                    const uint64_t *__restrict__ cdt, uint32_t cdt_len, size_t first /* polynomial */, size_t count /* rows * n */) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, n = (size_t)1 << log_n;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < count; o += stride) {
        const size_t r = o >> log_n, x = o & (n - 1);
        const uint64_t base = ctr_base(seed, ((first + r) << log_n) + x), rnd = sm64(base + DRAW_CDT);
        uint32_t mag = 0;
        for (uint32_t j = 0; j < cdt_len; j++) mag += rnd >= cdt[j] ? 1u : 0u;
        const bool neg = (sm64(base + DRAW_SIGN) >> 63) != 0;
        for (uint32_t l = 0; l < L; l++) {
            const u256 q = limbs[l].q;
            u256 te, pw;
            te.l[0] = te.l[1] = te.l[2] = te.l[3] = 0;
            pw.l[0] = (q.l[1] | q.l[2] | q.l[3]) ? noise_scale : noise_scale % q.l[0]; pw.l[1] = pw.l[2] = pw.l[3] = 0;
            for (uint32_t k = mag; k; k >>= 1) { if (k & 1) te = add_mod(te, pw, q); pw = add_mod(pw, pw, q); }
            if (neg) { u256 z; z.l[0] = z.l[1] = z.l[2] = z.l[3] = 0; te = sub_mod(z, te, q); }
            store_u256(out + ((r * L + l) << log_n) + x, te);
        }
    }
}

// kb[r][j][x] += (2^(k w) mod q_j) tgt[j][x] for row r = j K + k, NTT domain, containers of any width class: k w doublings modulo q_j;
// one lane per (row, position)
__global__ void __launch_bounds__(256)
keygen_gadget_kernel(u256 *__restrict__ kb, const u256 *__restrict__ tgt, const CrtLimb *__restrict__ limbs, uint32_t L, uint32_t log_n,
                     uint32_t K, uint32_t w, size_t count /* L K n */) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, n = (size_t)1 << log_n;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < count; o += stride) {
        const size_t r = o >> log_n, x = o & (n - 1);
        const uint32_t j = (uint32_t)(r / K), k = (uint32_t)(r % K);
        const u256 q = limbs[j].q;
        u256 v = load_u256(tgt + ((size_t)j << log_n) + x);
        for (uint32_t d = 0; d < k * w; d++) v = add_mod(v, v, q);
        u256 *at = kb + ((r * L + j) << log_n) + x;
        store_u256(at, add_mod(load_u256(at), v, q));
    }
}

}  // namespace fhe_dev

namespace {

struct Scratch {                                     // device allocations of one call, freed when it ends
    std::vector<void *> p;
    ~Scratch() { for (void *d : p) if (d) (void)hipFree(d); }
    int get(void **out, size_t bytes) {
        HIP_TRY(hipMalloc(out, bytes));
        p.push_back(*out);
        return FHE_OK;
    }
};

fhe_relin_keys *new_key_set(fhe_rns_ntt *h, uint32_t decomp_bits, uint32_t K) {
    fhe_relin_keys *rk = new (std::nothrow) fhe_relin_keys();
    if (rk) { rk->owner = h; rk->decomp_bits = decomp_bits; rk->K = K; rk->num_keys = h->L * K; }
    return rk;
}

// one set on the composed path: rows first .. first + L K - 1 of the call's streams; sh = s^ as containers, tgt = the set's target^
int generate_composed(fhe_rns_ntt *h, fhe_relin_keys *rk, const void *sh, const void *tgt, char *prod, size_t first, uint64_t noise_scale,
                      const uint64_t seeds[2], bool packed) {
    const uint32_t LK = rk->num_keys;
    const size_t S = (size_t)h->L * h->n * 32, count = (size_t)LK * h->n;
    int rc;
    HIP_TRY(hipMalloc(&rk->d_kb, S * LK));
    HIP_TRY(hipMalloc(&rk->d_ka, S * LK));
    if ((rc = sample_uniform_from(h, rk->d_ka, seeds[0], first * h->L, (size_t)LK * h->L))) return rc;
    hipLaunchKernelGGL(fhe_dev::keygen_noise_kernel, dim3(ew_grid(count)), dim3(256), 0, h->stream, (fhe_dev::u256 *)rk->d_kb, (const fhe_dev::CrtLimb *)h->d_crt,
                       h->L, h->log_n, seeds[1], noise_scale, (const uint64_t *)h->d_cdt, h->cdt_len, first, count);
    if ((rc = post_launch(h->stream, "keygen_noise_kernel"))) return rc;
    if ((rc = do_forward(h, rk->d_kb, LK))) return rc;
    for (uint32_t r = 0; r < LK; r++)
        if ((rc = do_ew<0>(h, prod + r * S, (const char *)rk->d_ka + r * S, sh, 1, "keygen a . s"))) return rc;
    if ((rc = do_ew<2>(h, rk->d_kb, rk->d_kb, prod, LK, "keygen e - a . s"))) return rc;
    hipLaunchKernelGGL(fhe_dev::keygen_gadget_kernel, dim3(ew_grid(count)), dim3(256), 0, h->stream, (fhe_dev::u256 *)rk->d_kb, (const fhe_dev::u256 *)tgt,
                       (const fhe_dev::CrtLimb *)h->d_crt, h->L, h->log_n, rk->K, rk->decomp_bits, count);
    if ((rc = post_launch(h->stream, "keygen_gadget_kernel"))) return rc;
    if (packed) {
        if ((rc = pack_relin_keys(h, rk))) return rc;
        (void)hipFree(rk->d_kb); (void)hipFree(rk->d_ka);     // as fhe_relin_keys_create: a packed set keeps its tables only (hipFree waits for the packing)
        rk->d_kb = rk->d_ka = nullptr;
    }
    return FHE_OK;
}

}  // namespace

extern "C" int fhe_keyswitch_keys_generate(fhe_rns_ntt_t *h, const fhe_secret_key_t *sk, uint32_t decomp_bits, const uint32_t *galois_elts,
                                           uint32_t num_sets, uint64_t noise_scale, double sigma, const uint64_t seeds[2], fhe_relin_keys_t **out_sets) {
    int rc = check_call(h, 1, "keyswitch_keys_generate"); if (rc) return rc;
    if (!sk || !galois_elts || !seeds || !out_sets) return fail(FHE_ERR_INVALID_ARG, "keyswitch_keys_generate: null argument");
    if (sk->owner != h) return fail(FHE_ERR_INVALID_ARG, "keyswitch_keys_generate: the key was imported for a different engine");
    if (!num_sets) return fail(FHE_ERR_INVALID_ARG, "keyswitch_keys_generate: num_sets must be at least 1");
    if (decomp_bits < 1 || decomp_bits > 64) return fail(FHE_ERR_INVALID_ARG, "keyswitch_keys_generate: decomp_bits must be in [1, 64]");
    for (uint32_t e = 0; e < num_sets; e++)
        if (galois_elts[e] && (rc = check_galois_element(h, galois_elts[e], "keyswitch_keys_generate"))) return rc;
    if (!noise_scale) return fail(FHE_ERR_INVALID_ARG, "keyswitch_keys_generate: noise_scale must not be 0");
    const uint32_t K = relin_digits(h, decomp_bits), LK = h->L * K;
    if ((uint64_t)num_sets * LK * h->L > 0x7fffffffull) return fail(FHE_ERR_INVALID_ARG, "keyswitch_keys_generate: num_sets * num_primes^2 * digits too large");
    uint32_t len = 0;
    if ((rc = fhe_gaussian_cdt(sigma, nullptr, 0, &len))) return rc;
    if ((rc = ensure_cdt(h, sigma, "keyswitch_keys_generate"))) return rc;      // rejects 12 sigma >= the smallest modulus before it allocates
    (void)hipGetLastError();

    const bool packed = keys_get_packed(h, decomp_bits, K);
    const bool fused = plan_fused_keygen(h, packed) && sk->d_packed && h->cdt_len <= fhe_dev::ENCRYPT_MAX_CDT;
    const size_t S = (size_t)h->L * h->n * 32, table = (size_t)LK * h->L * h->n * residue_bytes(h);
    std::vector<fhe_relin_keys *> sets(num_sets, nullptr);
    Scratch scratch;
    auto body = [&]() -> int {
        for (uint32_t e = 0; e < num_sets; e++)
            if (!(sets[e] = new_key_set(h, decomp_bits, K))) return fail(FHE_ERR_INVALID_ARG, "out of host memory");
        if (fused) {
            std::vector<fhe_dev::KeygenSet> tab(num_sets);
            for (uint32_t e = 0; e < num_sets; e++) {
                HIP_TRY(hipMalloc(&sets[e]->d_pkb, table));
                HIP_TRY(hipMalloc(&sets[e]->d_pka, table));
                tab[e] = {sets[e]->d_pkb, sets[e]->d_pka, galois_elts[e], 0u};
            }
            void *d_tab = nullptr;
            if (int r = scratch.get(&d_tab, num_sets * sizeof(fhe_dev::KeygenSet))) return r;
            HIP_TRY(hipMemcpy(d_tab, tab.data(), num_sets * sizeof(fhe_dev::KeygenSet), hipMemcpyHostToDevice));
            const size_t half = (size_t)h->L * h->n * residue_bytes(h);
            fhe_dev::LdsArgs A = lds_args(h, fhe_dev::LDS_KEYGEN, {}, num_sets * LK * h->L);
            A.a0 = d_tab; A.kb = sk->d_packed; A.ka = (const char *)sk->d_packed + half;
            A.cdt = h->d_cdt; A.cdt_len = h->cdt_len; A.seeds[0] = seeds[0]; A.seeds[1] = seeds[1]; A.t = noise_scale; A.K = K; A.w = decomp_bits;
            if (int r = lds_launch(h, A, "ntt_keygen_kernel")) return r;
        } else {
            if (int r = ensure_crt(h)) return r;
            void *sh = nullptr, *tgt = nullptr, *prod = nullptr;
            int r;
            if ((r = scratch.get(&sh, S)) || (r = scratch.get(&tgt, S)) || (r = scratch.get(&prod, S * LK))) return r;
            HIP_TRY(hipMemcpyAsync(sh, sk->d_s, S, hipMemcpyDeviceToDevice, h->stream));
            if ((r = do_forward(h, sh, 1))) return r;
            for (uint32_t e = 0; e < num_sets; e++) {
                if (!galois_elts[e]) HIP_TRY(hipMemcpyAsync(tgt, (const char *)sk->d_s + S, S, hipMemcpyDeviceToDevice, h->stream));
                else if ((r = do_galois(h, tgt, nullptr, nullptr, sk->d_s, nullptr, galois_elts[e], h->L, false))) return r;
                if ((r = do_forward(h, tgt, 1))) return r;
                if ((r = generate_composed(h, sets[e], sh, tgt, (char *)prod, (size_t)e * LK, noise_scale, seeds, packed))) return r;
            }
        }
        HIP_TRY(hipStreamSynchronize(h->stream));     // the scratch is freed when the call returns; the keys are complete then
        return FHE_OK;
    };
    rc = body();
    if (rc) {
        (void)hipStreamSynchronize(h->stream);
        for (fhe_relin_keys *rk : sets) fhe_relin_keys_destroy(rk);
        for (uint32_t e = 0; e < num_sets; e++) out_sets[e] = nullptr;
        return rc;
    }
    if (K > h->max_digits) h->max_digits = K;                                   // as the import: fhe_rns_ntt_reserve sizes the key-switch workspaces for it
    if (!packed && K > h->max_composed_digits) h->max_composed_digits = K;
    for (uint32_t e = 0; e < num_sets; e++) out_sets[e] = sets[e];
    return FHE_OK;
}

extern "C" int fhe_relin_keys_export(fhe_rns_ntt_t *h, const fhe_relin_keys_t *rk, void *d_keys_b, void *d_keys_a) {
    int rc = check_call(h, 1, "relin_keys_export"); if (rc) return rc;
    if (!rk || !d_keys_b || !d_keys_a) return fail(FHE_ERR_INVALID_ARG, "relin_keys_export: null argument");
    if ((rc = check_aligned({d_keys_b, d_keys_a}, "relin_keys_export"))) return rc;
    if (rk->owner != h) return fail(FHE_ERR_INVALID_ARG, "relin_keys_export: keys were imported for a different engine");
    if (d_keys_b == d_keys_a) return fail(FHE_ERR_INVALID_ARG, "relin_keys_export: outputs must be distinct");
    const size_t bytes = (size_t)rk->num_keys * h->L * h->n * 32;
    void *outs[2] = {d_keys_b, d_keys_a};
    const void *cont[2] = {rk->d_kb, rk->d_ka}, *pk[2] = {rk->d_pkb, rk->d_pka};
    for (int c = 0; c < 2; c++) {
        if (cont[c]) HIP_TRY(hipMemcpyAsync(outs[c], cont[c], bytes, hipMemcpyDeviceToDevice, h->stream));
        else if (pk[c]) {
            if ((rc = with_word_field(h, [&](auto f) {
                    using F = decltype(f);
                    hipLaunchKernelGGL((fhe_dev::unpack_keys_kernel<F>), dim3(ew_grid(bytes / 16)), dim3(256), 0, h->stream, (typename F::V16 *)outs[c],
                                       (const typename F::E *)pk[c], (const fhe_dev::Limb<F> *)h->d_limbs, h->L, h->log_n, rk->num_keys);
                    return post_launch(h->stream, "unpack_keys_kernel");
                }))) return rc;
        } else return fail(FHE_ERR_INVALID_ARG, "relin_keys_export: the key set holds no tables");
        if ((rc = do_inverse(h, outs[c], rk->num_keys))) return rc;
    }
    return FHE_OK;
}
