// hoist_lincomb.hip.h -- hoisted linear transform on the LDS-resident sizes: out = sum_t p_t * hoisted_rotation(ct, g_t) in ONE launch over all
// G terms ("double hoisting": fhe_ct_linear_transform_hoisted, include/fhe_hip.h).  ntt_hoist_apply_kernel (hoist.hip.h) has each rotated
// key-switch result in registers, in the NTT domain, before its inverse transforms; there a plaintext product is a pointwise multiply and
// the sum over the terms an addition, so G terms cost two inverse transforms and two container stores in all instead of 6 G of each.
//
// Everything sits in the layout of hoist.hip.h (natural evaluation order, slot e at word hoist_phys(e)): the kept digit polynomials, and
// c0^ (c1^ when a term has no key) written once per call by ntt_hoist_fwd_kernel, CANONICAL.  Every image goes through the exchange buffer
// and is read at pi_g with the odd lane stride that header derives, so the permuted reads stay conflict-free for every g.
// Ranges, per term (acc = the term's key products, tot = the running totals):
//   acc  after L K pw_mul / pw_add: integer fields [0, 2q) (F64X: canonical), F52 |acc| < L K * 0.76 q < 2^49 (the host admits L K <= 83)
//   acc  = pw_add(regroup1(acc), c^):  regroup1 brings F52 below 0.76 q first, c^ < q: integer fields csub(a + b, 2q) with a + b < 3q -> [0, 2q);
//          F52 |acc| < 1.76 q, inside the |b| < 2^48 that pw_mul states
//   prod = pw_mul(p^ 2^W, acc): p^ canonical operand, acc lazy (< 4q) -> [0, 2q) (F52 |prod| < 0.76 q); the 2^-W cancels as for key rows
//   tot  = regroup1(pw_add(tot, prod)): [0, 2q) + [0, 2q) -> [0, 2q); F52 < 0.76 q again after every term, so G is not bounded by a range
// and tot enters inv_core exactly as the accumulators of ntt_hoist_apply_kernel do.
#pragma once
#include "hoist.hip.h"
#include "lds_launch.h"

namespace fhe_dev {

// c0 (blockIdx.y == 0) or c1 (1) of the call: containers in, forward transform, canonical values in the hoist layout out ([comp][polys][n]
// residues).  ntt_hoist_kernel with the whole residue as its single digit and j = i.
template <class F, int LOGN, int MINW = 1>
__global__ void __launch_bounds__(NttCfg<LOGN>::T, MINW)
ntt_hoist_fwd_kernel(typename F::E *__restrict__ dst0, const char *__restrict__ c0, const char *__restrict__ c1, const Limb<F> *__restrict__ limbs, uint32_t L) {
    using C = NttCfg<LOGN>;
    using E = typename F::E;
    constexpr int VPL = 16 / sizeof(E), NCH = 32 / VPL;
    typedef E VecE __attribute__((ext_vector_type(VPL)));
    __shared__ __attribute__((aligned(16))) E lds[C::LDS_ELEMS];
    const uint32_t tid = threadIdx.x, p = blockIdx.x, comp = blockIdx.y;
    const Limb<F> P = limbs[p % L];
    E x[32];
    load_src<F, LOGN, false>(comp ? c1 : c0, p, tid, x);
    fwd_core<F, LOGN>(x, lds, tid, P);
#pragma unroll
    for (int r = 0; r < 32; r++) x[r] = F::canon_fwd(x[r], P.q, P.q2, P.qinv);
    __syncthreads();                                       // every Z-pattern read of the transform is done
    E *put = lds + hoist_phys<LOGN>(__brev(tid << 5) >> (32 - LOGN));
#pragma unroll
    for (int r = 0; r < 32; r++) put[bitrev5(r) << 6] = x[r];
    __syncthreads();
    VecE *dst = reinterpret_cast<VecE *>(dst0 + ((size_t)comp * gridDim.x + p) * C::N) + tid;
    const VecE *img = reinterpret_cast<const VecE *>(lds) + tid;
#pragma unroll
    for (int c = 0; c < NCH; c++) dst[c * C::T] = img[c * C::T];
}

// SPLIT = false: one workgroup per (ciphertext b, limb i), five live arrays (both accumulators, both totals, the image read; 4-byte residues).
// SPLIT = true : one workgroup per (b, i, output component), three live arrays (8-byte residues).
// cw0 / cw1: c0^ / c1^ of ntt_hoist_fwd_kernel ([polys][n] residues each; cw1 is read for keyless terms only).
template <class F, int LOGN, int MINW = 1, bool SPLIT = false>
__global__ void __launch_bounds__(NttCfg<LOGN>::T, MINW)
ntt_hoist_lincomb_kernel(char *__restrict__ out0, char *__restrict__ out1, const typename F::E *__restrict__ hoist, const typename F::E *__restrict__ cw0,
                         const typename F::E *__restrict__ cw1, const LincombTerm *__restrict__ terms, uint32_t G,
                         const Limb<F> *__restrict__ limbs, uint32_t L, uint32_t K) {
    using C = NttCfg<LOGN>;
    using E = typename F::E;
    constexpr int VPL = 16 / sizeof(E), NCH = 32 / VPL, NC = SPLIT ? 1 : 2;
    constexpr int FLIGHT = SPLIT ? 2 : 1;                  // chunks of table loads in flight at a time: 8 VGPRs (half of what ntt_hoist_apply_kernel allows itself)
    typedef E VecE __attribute__((ext_vector_type(VPL)));
    __shared__ __attribute__((aligned(16))) E lds[C::LDS_ELEMS];
    const uint32_t tid = threadIdx.x;
    const auto [b, u] = block_map(L * (SPLIT ? 2 : 1));
    const uint32_t i = SPLIT ? u >> 1 : u, comp = SPLIT ? u & 1 : 0;      // comp: the one component a SPLIT workgroup produces
    const uint32_t p = b * L + i, LK = L * K;
    const Limb<F> P = limbs[i];
    E tot[NC][32], acc[NC][32], d[32];
#pragma unroll
    for (int r = 0; r < 32; r++)
#pragma unroll
        for (int h = 0; h < NC; h++) tot[h][r] = 0;
    const uint32_t voff = tid * 16;
    const uint32_t slot = __brev(tid << 5) >> (32 - LOGN);
    VecE *img = reinterpret_cast<VecE *>(lds) + tid;
    // the workgroup's kept polynomials and its c0^ / c1^ through descriptors (one shared VGPR offset, scalar strides: no 64-bit VGPR addresses);
    // L K n residues per workgroup stay below the 4 GiB that the host already demands of a packed key table
    const TableBuf KEPT(hoist + (size_t)p * LK * C::N), CW0(cw0 + (size_t)p * C::N), CW1(cw1 + (size_t)p * C::N);
    for (uint32_t t = 0; t < G; t++) {
        const LincombTerm term = terms[t];
        const uint32_t g = term.g;
        const bool keyed = term.kb != nullptr;
        // source slot of register r as in ntt_hoist_apply_kernel: g * slot + (g - 1) / 2 mod n; the register index moves its top five bits only
        const uint32_t s0 = (g * slot + (g >> 1)) & (C::N - 1), t0 = s0 >> (LOGN - 5);
        const E *get = lds + hoist_phys<LOGN>(s0 & ((1u << (LOGN - 5)) - 1));
        // one polynomial of the hoist layout into the exchange buffer (coalesced 16-byte loads), read back at pi_g
        auto read_permuted = [&](const TableBuf &B, uint32_t soff) {
            // 8-byte residues: the 32 word offsets are formed anew for every image (three instructions each beside a 64-bit modular product)
            // instead of living in 32 VGPRs across the level loop: the element is passed through an empty asm statement that the compiler cannot see through
            uint32_t gs = g;
            if constexpr (SPLIT) asm volatile("" : "+s"(gs));
            VecE v[NCH];
#pragma unroll
            for (int c = 0; c < NCH; c++) v[c] = B.template load16<VecE>(voff, soff + c * C::T * 16);
            __syncthreads();                               // the previous image's permuted reads are done
#pragma unroll
            for (int c = 0; c < NCH; c++) img[c * C::T] = v[c];
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 32; r++) d[r] = get[((t0 + gs * bitrev5(r)) & 31) << 6];
        };
#pragma unroll
        for (int r = 0; r < 32; r++)
#pragma unroll
            for (int h = 0; h < NC; h++) acc[h][r] = 0;
        if (keyed) {
            const TableBuf KB(SPLIT && comp ? term.ka : term.kb), KA(term.ka);
            for (uint32_t jk = 0; jk < LK; jk++) {
                read_permuted(KEPT, jk * (uint32_t)(C::N * sizeof(E)));
                __builtin_amdgcn_sched_barrier(0);
                const uint32_t tbl = (uint32_t)((((size_t)jk * L + i) * C::N) * sizeof(E));   // byte offset of the row (< 4 GiB: host)
#pragma unroll
                for (int c = 0; c < NCH; c++) {
                    const VecE vb = KB.template load16<VecE>(voff, tbl + c * C::T * 16);
                    VecE va;
                    if constexpr (!SPLIT) va = KA.template load16<VecE>(voff, tbl + c * C::T * 16);
#pragma unroll
                    for (int e = 0; e < VPL; e++) {
                        const int r = c * VPL + e;
                        acc[0][r] = F::pw_add(acc[0][r], F::pw_mul(vb[e], d[r], P.q, P.qinv), P.q, P.q2);
                        if constexpr (!SPLIT) acc[1][r] = F::pw_add(acc[1][r], F::pw_mul(va[e], d[r], P.q, P.qinv), P.q, P.q2);
                    }
                    if ((c & (FLIGHT - 1)) == FLIGHT - 1) __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        // + pi_g(c0^) on component 0; a keyless term (g = 1) is (c0^, c1^) itself
        if (!SPLIT || !comp || !keyed) {
            read_permuted(SPLIT && comp ? CW1 : CW0, 0);
#pragma unroll
            for (int r = 0; r < 32; r++) acc[0][r] = F::pw_add(F::regroup1(acc[0][r], P.q, P.qinv), d[r], P.q, P.q2);
        } else {
#pragma unroll
            for (int r = 0; r < 32; r++) acc[0][r] = F::regroup1(acc[0][r], P.q, P.qinv);
        }
        if constexpr (!SPLIT) {
            if (!keyed) {
                read_permuted(CW1, 0);
#pragma unroll
                for (int r = 0; r < 32; r++) acc[1][r] = d[r];
            } else {
#pragma unroll
                for (int r = 0; r < 32; r++) acc[1][r] = F::regroup1(acc[1][r], P.q, P.qinv);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // times the term's plaintext, into the totals
        const TableBuf PT(term.pt);
        const uint32_t row = (uint32_t)(((size_t)i * C::N) * sizeof(E));
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            const VecE vp = PT.template load16<VecE>(voff, row + c * C::T * 16);
#pragma unroll
            for (int e = 0; e < VPL; e++) {
                const int r = c * VPL + e;
#pragma unroll
                for (int h = 0; h < NC; h++)
                    tot[h][r] = F::regroup1(F::pw_add(tot[h][r], F::pw_mul(vp[e], acc[h][r], P.q, P.qinv), P.q, P.q2), P.q, P.qinv);
            }
            if ((c & (FLIGHT - 1)) == FLIGHT - 1) __builtin_amdgcn_sched_barrier(0);
        }
    }
    // the totals leave as the accumulators of ntt_hoist_apply_kernel do (sigma_g(c0) is already inside)
    inv_core<F, LOGN, false, true>(tot[0], lds, tid, P, P.ninv, P.ninv_s, P.ninvw, P.ninvw_s);   // PRESYNC: the last permuted reads are done
#pragma unroll
    for (int r = 0; r < 32; r++) tot[0][r] = F::canon_inv(tot[0][r], P.q);
    lds_put<PatA<LOGN>>(lds, tid, tot[0]);
    __syncthreads();
    if constexpr (SPLIT) {
        store_from_lds<F, LOGN>((comp ? out1 : out0) + (size_t)p * (C::N * 32), lds, tid);
    } else {
        store_from_lds_rolled<F, LOGN>(out0 + (size_t)p * (C::N * 32), lds, tid);
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        inv_core<F, LOGN>(tot[1], lds, tid, P, P.ninv, P.ninv_s, P.ninvw, P.ninvw_s);
#pragma unroll
        for (int r = 0; r < 32; r++) tot[1][r] = F::canon_inv(tot[1][r], P.q);
        lds_put<PatA<LOGN>>(lds, tid, tot[1]);
        __syncthreads();
        store_from_lds<F, LOGN>(out1 + (size_t)p * (C::N * 32), lds, tid);
    }
}

}  // namespace fhe_dev
