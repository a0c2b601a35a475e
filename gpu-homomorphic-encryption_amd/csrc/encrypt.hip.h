// encrypt.hip.h -- public-key encryption on the LDS-resident sizes in ONE launch (fhe_ct_encrypt, include/fhe_hip.h):
//     out0[b][i] = pk0_i (*) u_b + [t e0_b]_{q_i} + m[b][i],      out1[b][i] = pk1_i (*) u_b + [t e1_b]_{q_i}
// with u ternary and e0, e1 discrete Gaussians drawn IN the kernel from the counter-based generator of the samplers (ctr_rand.hip.h): element
// g = b n + x of stream seeds[0..2] is exactly what sample_small_kernel (sampling.hip.h) writes for that element, so the result equals the
// composition of the container-level entry points bit for bit.
//
// A workgroup first draws its ciphertext's u, e0, e1 at the coefficients of the forward transform's input layout (pattern A: thread tid,
// register r <-> coefficient tid + r T) and keeps them as PACKED SMALL INTEGERS: u as two 32-bit masks (non-zero, negative), every error as
// 16 bits (15 of magnitude, one of sign), 34 VGPRs in all.  The cumulative table is staged in the exchange buffer, which nothing else uses yet,
// and inverted by a branch-free binary search (cdt_count, ctr_rand.hip.h; the host admits tables that fit: ENCRYPT_MAX_CDT entries, i.e. sigma <= 85): ceil(log2 len)
// LDS reads per coefficient instead of the linear scan's len 64-bit compares, same count because the table is non-decreasing.
// Then, for every limb i of its range, with TWO live arrays:
//     u^ = NTT_i(u);  x = pk0^_i . u^ -> INTT -> + t e0 + m -> containers;  x = pk1^_i . u^ -> INTT -> + t e1 -> containers
// i.e. one forward and two inverse transforms per limb polynomial, no workspace, 3 S bytes of HBM traffic (m in, c0 and c1 out).  pk^ are the
// packed tables of pack_keys_kernel (transformed, times 2^W, in the register order of pattern Z), read through a descriptor.
// The limb range is the grid form: one workgroup per (ciphertext, limb) (per_ct = 0; few ciphertexts: L times the workgroups) or one per
// ciphertext looping over the L limbs (per_ct = 1; the draws, ~8 SplitMix64 finalisers per coefficient, are paid once instead of L times).
// The same code runs both, so the bits cannot differ.
// Ranges: u in {0, 1, q - 1} canonical -> fwd_core -> [0, 4q) lazy (F52: |u^| < 12 q); pw_mul(canonical pk^ 2^W, lazy u^) -> [0, 2q)
// (F52: < 0.76 q) with no 2^-W left, which is what inv_core takes; canon_inv -> [0, q); the additions are canonical (ew_add / ew_sub).
#pragma once
#include "ctr_rand.hip.h"
#include "lds_launch.h"
#include "ntt_lds.hip.h"

namespace fhe_dev {

template <class F, int LOGN, int MINW = 1>
__global__ void __launch_bounds__(NttCfg<LOGN>::T, MINW)
ntt_encrypt_kernel(char *__restrict__ out0, char *__restrict__ out1, const char *__restrict__ m, const typename F::E *__restrict__ pk0,
                   const typename F::E *__restrict__ pk1, const uint64_t *__restrict__ cdt, uint32_t cdt_len, uint64_t seed_u, uint64_t seed_e0,
                   uint64_t seed_e1, uint64_t t, const Limb<F> *__restrict__ limbs, uint32_t L, uint32_t per_ct) {
    using C = NttCfg<LOGN>;
    using E = typename F::E;
    constexpr int VPL = 16 / sizeof(E), NCH = 32 / VPL;
    typedef E VecE __attribute__((ext_vector_type(VPL)));
    static_assert(ENCRYPT_MAX_CDT * sizeof(uint64_t) <= C::LDS_ELEMS * sizeof(E), "the cumulative table is staged in the exchange buffer");
    __shared__ __attribute__((aligned(16))) E lds[C::LDS_ELEMS];
    const uint32_t tid = threadIdx.x;
    uint32_t b, i0, i1;
    if (per_ct) { b = blockIdx.x; i0 = 0; i1 = L; }
    else { const auto [bb, i] = block_map(L); b = bb; i0 = i; i1 = i + 1; }

    // ---- the ciphertext's u, e0, e1 at coefficients tid + r T, packed ----
    uint64_t *tab = reinterpret_cast<uint64_t *>(lds);
    for (uint32_t j = tid; j < cdt_len; j += C::T) tab[j] = cdt[j];
    __syncthreads();
    const uint32_t top = 1u << (31 - __builtin_clz(cdt_len));
    uint32_t u_nz = 0, u_neg = 0, pe0[16], pe1[16];
#pragma unroll
    for (int r = 0; r < 16; r++) { pe0[r] = 0; pe1[r] = 0; }
    const uint64_t g0 = (uint64_t)b * C::N + tid;
    // A ROLLED loop of 16 trips, two coefficients (four table searches) each: fully unrolled, the 64-bit temporaries of 32 x 8 finalisers
    // push the kernel over its register budget.  The packed word of trip `it` goes to its register by 16 selects, not by a dynamic index
    // (which would move the arrays to scratch).
#pragma unroll 1
    for (uint32_t it = 0; it < 16; it++) {
        uint32_t w0 = 0, w1 = 0;
#pragma unroll
        for (uint32_t k = 0; k < 2; k++) {
            const uint32_t r = 2 * it + k;
            const uint64_t g = g0 + (uint64_t)r * C::T;
            const uint64_t ru = ctr_rand(seed_u, g, DRAW_TERNARY);
            u_nz |= ((uint32_t)ru < 0x80000000u ? 1u : 0u) << r;       // threshold 2^31: probability 0.5
            u_neg |= (uint32_t)(ru >> 63) << r;
            const uint64_t h0 = ctr_base(seed_e0, g), h1 = ctr_base(seed_e1, g);
            const uint32_t m0 = cdt_count(tab, cdt_len, top, sm64(h0 + DRAW_CDT)), m1 = cdt_count(tab, cdt_len, top, sm64(h1 + DRAW_CDT));
            const uint32_t s0 = (uint32_t)(sm64(h0 + DRAW_SIGN) >> 63), s1 = (uint32_t)(sm64(h1 + DRAW_SIGN) >> 63);
            w0 |= (m0 | (s0 << 15)) << (16 * k);
            w1 |= (m1 | (s1 << 15)) << (16 * k);
        }
#pragma unroll
        for (uint32_t j = 0; j < 16; j++) { pe0[j] = j == it ? w0 : pe0[j]; pe1[j] = j == it ? w1 : pe1[j]; }
    }

    const TableBuf PK0(pk0), PK1(pk1);
    const uint32_t voff = tid * 16;
    for (uint32_t i = i0; i < i1; i++) {
        const Limb<F> P = limbs[i];
        const uint32_t p = b * L + i;
        const uint32_t row = (uint32_t)(((size_t)i * C::N) * sizeof(E));   // byte offset of limb i's row (the tables hold L n residues: far below 4 GiB)
        const E tW = F::to_pw_operand(F::from_u64(t, P.q), P);              // (t mod q) 2^W: pw_mul(tW, k) = t k mod q, in [0, 2q)
        const E qm1 = F::ew_sub((E)0, (E)1, P.q);
        E uh[32], x[32];
#pragma unroll
        for (int r = 0; r < 32; r++) uh[r] = ((u_nz >> r) & 1) ? (((u_neg >> r) & 1) ? qm1 : (E)1) : (E)0;
        fwd_core<F, LOGN, false, true>(uh, lds, tid, P);       // PRESYNC: the table reads / the previous limb's store are done before this exchange
        __builtin_amdgcn_sched_barrier(0);
        // one half: x = pk^ . u^ -> coefficient domain, canonical, + or - t |e| (+ m), through the exchange buffer into containers
        auto half = [&](const TableBuf &PK, const uint32_t (&pe)[16], const char *add, char *out) __attribute__((always_inline)) {
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const VecE v = PK.template load16<VecE>(voff, row + c * C::T * 16);
#pragma unroll
                for (int e = 0; e < VPL; e++) x[c * VPL + e] = F::pw_mul(v[e], uh[c * VPL + e], P.q, P.qinv);
                if ((c & 3) == 3) __builtin_amdgcn_sched_barrier(0);       // four chunks of table loads in flight at a time
            }
            inv_core<F, LOGN>(x, lds, tid, P, P.ninv, P.ninv_s, P.ninvw, P.ninvw_s);   // the slots this thread read last: no barrier needed before
            __builtin_amdgcn_sched_barrier(0);
            const TableBuf M(add ? add + (size_t)p * (C::N * 32) : nullptr);
#pragma unroll
            for (int r = 0; r < 32; r++) {
                const uint32_t w = pe[r >> 1] >> (16 * (r & 1));
                const E te = F::canon_inv(F::pw_mul(tW, (E)(w & 0x7fffu), P.q, P.qinv), P.q);
                E v = F::canon_inv(x[r], P.q);
                v = (w & 0x8000u) ? F::ew_sub(v, te, P.q) : F::ew_add(v, te, P.q);
                if (add) v = F::ew_add(v, M.template load_residue<F, false>(tid * 32, r * (C::T * 32)), P.q);
                x[r] = v;
                if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);       // four loads of m in flight at a time
            }
            lds_put<PatA<LOGN>>(lds, tid, x);
            __syncthreads();
            store_from_lds_rolled<F, LOGN>(out + (size_t)p * (C::N * 32), lds, tid);   // rolled: u^ or the packed samples are live across it
            __builtin_amdgcn_sched_barrier(0);
        };
        half(PK0, pe0, m, out0);
        __syncthreads();                                       // the store's reads of the exchange buffer are done
        half(PK1, pe1, nullptr, out1);
    }
}

}  // namespace fhe_dev
