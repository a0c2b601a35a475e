// keygen.hip.h -- key-switching key generation on the LDS-resident sizes in ONE launch (fhe_keyswitch_keys_generate, include/fhe_hip.h).
// For set e, row r = j K + k (polynomial P = e L K + r of the call) and limb l, in the NTT domain:
//     a^_P[l] = U_P[l]                                                    the uniform residues themselves
//     b^_P[l] = NTT_l([noise_scale e_P]_{q_l}) - a^_P[l] . s^[l] + (l == j ? (2^(k w) mod q_j) . target^[j] : 0)
// with U and e drawn IN the kernel from the counter-based generator of the samplers (ctr_rand.hip.h): U_P[l][y] is what
// sample_uniform_rns_kernel writes at element (P L + l) n + y, e_P[x] what sample_small_kernel<1> writes at element P n + x, so the rows equal
// the composition of the container-level entry points bit for bit.  Both rows go straight into the set's packed tables (the layout of
// pack_keys_kernel: times 2^W, register order of pattern Z), which is all a packed key set keeps: no inverse transform, no workspace.
//
// One workgroup per (set, row, limb), ONE live 32-register array:
//   1. the cumulative table is staged in the exchange buffer and inverted with cdt_count, as ntt_encrypt_kernel does; e is drawn at the
//      coefficients of the forward transform's input (pattern A: thread tid, register r <-> coefficient tid + r T), scaled and signed;
//   2. one forward transform: register r now holds position y = tid 32 + r (pattern Z), the order of the packed tables;
//   3. per 16-byte chunk of that order: a^ is drawn (rejection on masked 64-bit words, trial t at draw DRAW_UNIFORM + 4 t; after 64 rejections
//      the top bit is cleared: sample_uniform_rns_kernel for a word-sized q) and written times 2^W; s^ comes through a descriptor; in limb j
//      target^ = s^ . s^ (element 0) or the NTT-domain permutation of s^ (Galois element g: position y holds s^[pi_g(y)], the index map of
//      galois.hip.h and hoist.hip.h), GATHERED from the packed table of the secret key -- [L][n] residues, L2-resident, read by the L K
//      workgroups of limb j only: no target table is built and the call stays one launch.
// Ranges: [noise_scale e] canonical -> fwd_core -> [0, 4q) lazy (F52: |.| <= 12 q) -> canon_fwd -> [0, q); a^ canonical by the rejection;
// pw_mul(canonical s^ 2^W, canonical a^) -> [0, 2q) (F52: |.| < 0.76 q) with no 2^-W left -> canon_inv -> [0, q); the gadget product
// likewise (pw_mul(canonical target^ 2^W, canonical 2^(k w) mod q_j)); subtraction and addition are canonical (ew_sub / ew_add);
// to_pw_operand takes and gives canonical values.  F64X is canonical throughout.
#pragma once
#include "ctr_rand.hip.h"                  // the generator and cdt_count
#include "lds_launch.h"
#include "ntt_lds.hip.h"

namespace fhe_dev {

// pi_g(y): the position of NTT(a) that position y of NTT(sigma_g a) equals (position y holds a(psi^(2 bitrev(y) + 1)))
template <int LOGN>
__device__ __forceinline__ uint32_t keygen_ntt_src(uint32_t y, uint32_t g) {
    const uint32_t e = __brev(y) >> (32 - LOGN);
    return __brev(((g * (2 * e + 1)) & ((2u << LOGN) - 1)) >> 1) >> (32 - LOGN);
}

template <class F, int LOGN, int MINW = 1>
__global__ void __launch_bounds__(NttCfg<LOGN>::T, MINW)
ntt_keygen_kernel(const KeygenSet *__restrict__ sets, const typename F::E *__restrict__ sh, const typename F::E *__restrict__ sh2,
                  const uint64_t *__restrict__ cdt, uint32_t cdt_len, uint64_t seed_a, uint64_t seed_e, uint64_t noise_scale,
                  const Limb<F> *__restrict__ limbs, uint32_t L, uint32_t K, uint32_t w) {
    using C = NttCfg<LOGN>;
    using E = typename F::E;
    constexpr int VPL = 16 / sizeof(E), NCH = 32 / VPL;
    typedef E VecE __attribute__((ext_vector_type(VPL)));
    static_assert(ENCRYPT_MAX_CDT * sizeof(uint64_t) <= C::LDS_ELEMS * sizeof(E), "the cumulative table is staged in the exchange buffer");
    __shared__ __attribute__((aligned(16))) E lds[C::LDS_ELEMS];
    const uint32_t tid = threadIdx.x, LK = L * K;
    const uint32_t pl = blockIdx.x, Pn = pl / L, l = pl % L;          // polynomial of the call, limb
    const uint32_t set = Pn / LK, row = Pn % LK, j = row / K, k = row % K;
    const Limb<F> P = limbs[l];
    const KeygenSet S = sets[set];

    // ---- [noise_scale e_P]_{q_l} at coefficients tid + r T ----
    uint64_t *tab = reinterpret_cast<uint64_t *>(lds);
    for (uint32_t i = tid; i < cdt_len; i += C::T) tab[i] = cdt[i];
    __syncthreads();
    const uint32_t top = 1u << (31 - __builtin_clz(cdt_len));
    const E sW = F::to_pw_operand(F::from_u64(noise_scale, P.q), P);   // (noise_scale mod q) 2^W: pw_mul(sW, m) = noise_scale m mod q, in [0, 2q)
    const uint64_t g0 = (uint64_t)Pn * C::N + tid;
    E x[32];
#pragma unroll
    for (int r = 0; r < 32; r++) {
        const uint64_t h = ctr_base(seed_e, g0 + (uint64_t)r * C::T);
        const uint32_t m = cdt_count(tab, cdt_len, top, sm64(h + DRAW_CDT));
        const E te = F::canon_inv(F::pw_mul(sW, (E)m, P.q, P.qinv), P.q);
        x[r] = (sm64(h + DRAW_SIGN) >> 63) ? F::ew_sub((E)0, te, P.q) : te;
        if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);          // four coefficients' 64-bit temporaries at a time
    }
    fwd_core<F, LOGN, false, true>(x, lds, tid, P);                    // PRESYNC: the table reads are done before this exchange
    __builtin_amdgcn_sched_barrier(0);

    // ---- the two rows, chunk by chunk of the packed order ----
    const uint64_t qw = (uint64_t)P.q;
    const uint64_t mask = ~0ull >> __builtin_clzll(qw);               // bit_length(q) ones
    const uint64_t u0 = ((uint64_t)Pn * L + l) * C::N + (uint64_t)tid * 32;
    const TableBuf SH(sh);
    const uint32_t voff = tid * 16, srow = (uint32_t)(((size_t)l * C::N) * sizeof(E));   // byte offset of limb l's row of s^ (L n residues: far below 4 GiB)
    const size_t out = ((size_t)row * L + l) * C::N;                   // the row's place in the set's tables
    VecE *ob = reinterpret_cast<VecE *>(reinterpret_cast<E *>(S.kb) + out) + tid;
    VecE *oa = reinterpret_cast<VecE *>(reinterpret_cast<E *>(S.ka) + out) + tid;
    const bool gadget = l == j;                                        // uniform over the workgroup
    const E *tgt = (S.g ? sh : sh2) + (size_t)l * C::N;
    const uint32_t g = S.g ? S.g : 1u;
    const E gk = F::from_u64(1ull << (k * w), P.q);                    // 2^(k w) mod q_j, canonical (k w < the widest modulus' bits <= 64)
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const VecE sv = SH.template load16<VecE>(voff, srow + c * C::T * 16);
        VecE vb, va;
#pragma unroll
        for (int e = 0; e < VPL; e++) {
            const int r = c * VPL + e;
            const uint64_t h = ctr_base(seed_a, u0 + r);
            uint64_t v;
            for (uint32_t t = 0;; t++) {
                v = sm64(h + DRAW_UNIFORM + 4 * t) & mask;
                if (v < qw) break;
                if (t == 63) { v &= mask >> 1; break; }
            }
            const E a = (E)v;
            E b = F::ew_sub(F::canon_fwd(x[r], P.q, P.q2, P.qinv), F::canon_inv(F::pw_mul(sv[e], a, P.q, P.qinv), P.q), P.q);
            if (gadget) {
                const uint32_t y = keygen_ntt_src<LOGN>(tid * 32 + r, g), ry = y & 31;
                const E tv = tgt[((size_t)(ry / VPL) * C::T + (y >> 5)) * VPL + ry % VPL];
                b = F::ew_add(b, F::canon_inv(F::pw_mul(tv, gk, P.q, P.qinv), P.q), P.q);
            }
            vb[e] = F::to_pw_operand(b, P);
            va[e] = F::to_pw_operand(a, P);
        }
        ob[c * C::T] = vb;
        oa[c * C::T] = va;
        if ((c & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
}

// The sibling for RGSW rows (fhe_rgsw_keys_generate): set e = 2 i + c is component c of RGSW ciphertext i with message mu_i, and the rows are
// those above with the gadget term  (2^(k w) mod q_j) . T^,  T = mu_i (c = 0: the constant polynomial, mu_i at EVERY position of the NTT
// domain, nothing read) or T = mu_i s (c = 1: mu_i s^[y] at position y -- the Galois-element-1 case of the gather above, whose index map is the
// identity, i.e. the chunk of s^ that the a^ . s^ product of this position has loaded already).  mu == 0 adds nothing.  Same draws (polynomial
// P = e L K + r of the call's streams), same forward transform, same packed stores; one workgroup per (set, row, limb), ONE live array.
// Ranges as above; gm = [mu 2^(k w)]_{q_j} is canonical (pw_mul(canonical |mu| 2^W, canonical 2^(k w)) -> canon_inv, negated by ew_sub).
template <class F, int LOGN, int MINW = 1>
__global__ void __launch_bounds__(NttCfg<LOGN>::T, MINW)
ntt_rgsw_keygen_kernel(const RgswSet *__restrict__ sets, const typename F::E *__restrict__ sh, const uint64_t *__restrict__ cdt, uint32_t cdt_len,
                       uint64_t seed_a, uint64_t seed_e, uint64_t noise_scale, const Limb<F> *__restrict__ limbs, uint32_t L, uint32_t K, uint32_t w) {
    using C = NttCfg<LOGN>;
    using E = typename F::E;
    constexpr int VPL = 16 / sizeof(E), NCH = 32 / VPL;
    typedef E VecE __attribute__((ext_vector_type(VPL)));
    static_assert(ENCRYPT_MAX_CDT * sizeof(uint64_t) <= C::LDS_ELEMS * sizeof(E), "the cumulative table is staged in the exchange buffer");
    __shared__ __attribute__((aligned(16))) E lds[C::LDS_ELEMS];
    const uint32_t tid = threadIdx.x, LK = L * K;
    const uint32_t pl = blockIdx.x, Pn = pl / L, l = pl % L;          // polynomial of the call, limb
    const uint32_t set = Pn / LK, row = Pn % LK, j = row / K, k = row % K;
    const Limb<F> P = limbs[l];
    const RgswSet S = sets[set];

    // ---- [noise_scale e_P]_{q_l} at coefficients tid + r T ----
    uint64_t *tab = reinterpret_cast<uint64_t *>(lds);
    for (uint32_t i = tid; i < cdt_len; i += C::T) tab[i] = cdt[i];
    __syncthreads();
    const uint32_t top = 1u << (31 - __builtin_clz(cdt_len));
    const E sW = F::to_pw_operand(F::from_u64(noise_scale, P.q), P);
    const uint64_t g0 = (uint64_t)Pn * C::N + tid;
    E x[32];
#pragma unroll
    for (int r = 0; r < 32; r++) {
        const uint64_t h = ctr_base(seed_e, g0 + (uint64_t)r * C::T);
        const uint32_t m = cdt_count(tab, cdt_len, top, sm64(h + DRAW_CDT));
        const E te = F::canon_inv(F::pw_mul(sW, (E)m, P.q, P.qinv), P.q);
        x[r] = (sm64(h + DRAW_SIGN) >> 63) ? F::ew_sub((E)0, te, P.q) : te;
        if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
    fwd_core<F, LOGN, false, true>(x, lds, tid, P);
    __builtin_amdgcn_sched_barrier(0);

    // ---- the two rows, chunk by chunk of the packed order ----
    const uint64_t qw = (uint64_t)P.q;
    const uint64_t mask = ~0ull >> __builtin_clzll(qw);
    const uint64_t u0 = ((uint64_t)Pn * L + l) * C::N + (uint64_t)tid * 32;
    const TableBuf SH(sh);
    const uint32_t voff = tid * 16, srow = (uint32_t)(((size_t)l * C::N) * sizeof(E));
    const size_t out = ((size_t)row * L + l) * C::N;
    VecE *ob = reinterpret_cast<VecE *>(reinterpret_cast<E *>(S.kb) + out) + tid;
    VecE *oa = reinterpret_cast<VecE *>(reinterpret_cast<E *>(S.ka) + out) + tid;
    const bool gadget = l == j && S.mu != 0;                           // uniform over the workgroup
    const bool by_s = S.comp != 0;
    const uint32_t mag = S.mu < 0 ? 0u - (uint32_t)S.mu : (uint32_t)S.mu;
    const E gk = F::from_u64(1ull << (k * w), P.q);                    // 2^(k w) mod q_j, canonical
    E gm = F::canon_inv(F::pw_mul(F::to_pw_operand(F::from_u64(mag, P.q), P), gk, P.q, P.qinv), P.q);
    if (S.mu < 0) gm = F::ew_sub((E)0, gm, P.q);                       // [mu 2^(k w)]_{q_j}
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const VecE sv = SH.template load16<VecE>(voff, srow + c * C::T * 16);
        VecE vb, va;
#pragma unroll
        for (int e = 0; e < VPL; e++) {
            const int r = c * VPL + e;
            const uint64_t h = ctr_base(seed_a, u0 + r);
            uint64_t v;
            for (uint32_t t = 0;; t++) {
                v = sm64(h + DRAW_UNIFORM + 4 * t) & mask;
                if (v < qw) break;
                if (t == 63) { v &= mask >> 1; break; }
            }
            const E a = (E)v;
            E b = F::ew_sub(F::canon_fwd(x[r], P.q, P.q2, P.qinv), F::canon_inv(F::pw_mul(sv[e], a, P.q, P.qinv), P.q), P.q);
            if (gadget) b = F::ew_add(b, by_s ? F::canon_inv(F::pw_mul(sv[e], gm, P.q, P.qinv), P.q) : gm, P.q);
            vb[e] = F::to_pw_operand(b, P);
            va[e] = F::to_pw_operand(a, P);
        }
        ob[c * C::T] = vb;
        oa[c * C::T] = va;
        if ((c & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
}

}  // namespace fhe_dev
