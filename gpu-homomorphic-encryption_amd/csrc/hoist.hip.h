// hoist.hip.h -- hoisted rotations on the LDS-resident sizes (Halevi-Shoup): the digit polynomials of c1 are formed and transformed ONCE
// (ntt_hoist_kernel) and kept; every Galois element then costs a permuted multiply-accumulate with its key rows and two inverse
// transforms (ntt_hoist_apply_kernel), because sigma_g of a polynomial is a pure permutation of its NTT values:
//     NTT(sigma_g a)[x] = NTT(a)[pi_g(x)],   pi_g(x) = bitrev(((g (2 bitrev(x) + 1)) mod 2n - 1) / 2)       (include/fhe_hip.h, Galois section)
// since position x of a transformed limb holds a(psi^(2 bitrev(x) + 1)) and (sigma_g a)(z) = a(z^g).
//
// Layout of a kept polynomial (internal).  Values sit in NATURAL EVALUATION ORDER -- slot e holds a(psi^(2e + 1)) -- so that pi_g becomes
// the affine map e -> g e + (g - 1) / 2 mod n, and slot e sits at word hoist_phys(e): the top 11 bits of e moved to the bottom.  Thread
// `tid`, register r of the transforms owns position tid * 32 + r, i.e. slot bitrev5(r) << (LOGN - 5) | bitrev(tid): the 64 lanes of a wave
// differ in slot bits [LOGN - 11, LOGN - 5), so their words differ by m, and after the map by g m mod 2^11, m = 0 .. 63 -- an odd stride, 64
// distinct banks for 4-byte residues, for the store of the hoist kernel and for the permuted read of the apply kernel alike.  The apply
// kernel brings a kept polynomial into the exchange buffer with coalesced 16-byte loads and takes the permuted reads from there: a gather
// from device memory would touch one cache line per lane.
// Workspace: [batch][L target limbs i][L K levels jk][n] residues, so that the L K polynomials a workgroup of the apply kernel reads are contiguous.
#pragma once
#include "ntt_lds.hip.h"

namespace fhe_dev {

template <int LOGN>
__device__ __forceinline__ uint32_t hoist_phys(uint32_t e) {
    static_assert(LOGN >= 11 && LOGN <= 15, "the LDS-resident sizes: the top 11 slot bits move down by S = LOGN - 11");
    constexpr uint32_t S = LOGN - 11;
    return S ? (e >> S) | ((e & ((1u << S) - 1)) << 11) : e;
}
constexpr uint32_t bitrev5(int r) { return (uint32_t)(((r & 1) << 4) | ((r & 2) << 2) | (r & 4) | ((r & 8) >> 2) | ((r & 16) >> 4)); }

// One workgroup per (ciphertext b, target limb i, source limb j): limb j of c1 (compact) is loaded once; for every digit k the digit
// polynomial is formed in registers and transformed under q_i -- the loop body of ntt_keyswitch_kernel without the keys -- and stored, as
// the lazy values the key products take, to level j K + k of (b, i).
template <class F, int LOGN, int MINW = 1>
__global__ void __launch_bounds__(NttCfg<LOGN>::T, MINW)
ntt_hoist_kernel(typename F::E *__restrict__ hoist, const char *__restrict__ c1, const Limb<F> *__restrict__ limbs, uint32_t L, uint32_t K, uint32_t w) {
    using C = NttCfg<LOGN>;
    using E = typename F::E;
    constexpr int VPL = 16 / sizeof(E), NCH = 32 / VPL;
    typedef E VecE __attribute__((ext_vector_type(VPL)));
    __shared__ __attribute__((aligned(16))) E lds[C::LDS_ELEMS];
    const uint32_t tid = threadIdx.x;
    const auto [b, u] = block_map(L * L);                 // the L * L workgroups of a ciphertext re-read its c1: one XCD's L2
    const uint32_t i = u / L, j = u % L;
    const Limb<F> P = limbs[i];
    E x[32], d[32];
    load_src<F, LOGN, true>(c1, (size_t)b * L + j, tid, x);
    // register r goes to slot bitrev5(r) << (LOGN - 5) | bitrev(tid), i.e. to word hoist_phys(bitrev(tid)) + (bitrev5(r) << 6)
    E *put = lds + hoist_phys<LOGN>(__brev(tid << 5) >> (32 - LOGN));
    VecE *dst = reinterpret_cast<VecE *>(hoist + (((size_t)b * L + i) * L + j) * K * C::N) + tid;
    const VecE *img = reinterpret_cast<const VecE *>(lds) + tid;
    for (uint32_t k = 0; k < K; k++) {
#pragma unroll
        for (int r = 0; r < 32; r++) d[r] = F::digit(x[r], k * w, w);
        fwd_core<F, LOGN, false, true>(d, lds, tid, P);    // PRESYNC: the previous digit's image has been copied out
        __syncthreads();                                   // every Z-pattern read of the transform is done
#pragma unroll
        for (int r = 0; r < 32; r++) put[bitrev5(r) << 6] = d[r];
        __syncthreads();
#pragma unroll
        for (int c = 0; c < NCH; c++) dst[c * C::T] = img[c * C::T];
        dst += C::N / VPL;
    }
}

// One workgroup per (ciphertext b, limb i), three live arrays: for every level jk the kept polynomial is copied into the exchange buffer,
// read back at pi_g and multiplied into both accumulators with the packed key rows (as ntt_keyswitch3_kernel); two inverse transforms;
// out0 = sigma_g(c0) (compact addend, written by the automorphism kernel) + the first, out1 = the second.
template <class F, int LOGN, int MINW = 1>
__global__ void __launch_bounds__(NttCfg<LOGN>::T, MINW)
ntt_hoist_apply_kernel(char *__restrict__ out0, char *__restrict__ out1, const typename F::E *__restrict__ hoist, const char *__restrict__ add0,
                       const typename F::E *__restrict__ kb, const typename F::E *__restrict__ ka, const Limb<F> *__restrict__ limbs,
                       uint32_t L, uint32_t K, uint32_t g) {
    using C = NttCfg<LOGN>;
    using E = typename F::E;
    constexpr int VPL = 16 / sizeof(E), NCH = 32 / VPL;
    typedef E VecE __attribute__((ext_vector_type(VPL)));
    __shared__ __attribute__((aligned(16))) E lds[C::LDS_ELEMS];
    const uint32_t tid = threadIdx.x;
    const auto [b, i] = block_map(L);
    const uint32_t p = b * L + i, LK = L * K;
    const Limb<F> P = limbs[i];
    E acc0[32], acc1[32], d[32];
#pragma unroll
    for (int r = 0; r < 32; r++) { acc0[r] = 0; acc1[r] = 0; }
    const TableBuf KB(kb), KA(ka);
    const uint32_t voff = tid * 16;
    // source slot of register r: g * slot + (g - 1) / 2 mod n, slot = bitrev5(r) << (LOGN - 5) | bitrev(tid).  The register index moves the top
    // five bits of the source slot only: word get + (((t0 + g * bitrev5(r)) & 31) << 6), three instructions per element
    const uint32_t s0 = (g * (__brev(tid << 5) >> (32 - LOGN)) + (g >> 1)) & (C::N - 1), t0 = s0 >> (LOGN - 5);
    const E *get = lds + hoist_phys<LOGN>(s0 & ((1u << (LOGN - 5)) - 1));
    const VecE *src = reinterpret_cast<const VecE *>(hoist + (size_t)p * LK * C::N) + tid;
    VecE *img = reinterpret_cast<VecE *>(lds) + tid;
    for (uint32_t jk = 0; jk < LK; jk++) {
        VecE v[NCH];
#pragma unroll
        for (int c = 0; c < NCH; c++) v[c] = src[c * C::T];
        src += C::N / VPL;
        __syncthreads();                                   // the previous level's permuted reads are done
#pragma unroll
        for (int c = 0; c < NCH; c++) img[c * C::T] = v[c];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 32; r++) d[r] = get[((t0 + g * bitrev5(r)) & 31) << 6];
        __builtin_amdgcn_sched_barrier(0);
        const uint32_t tbl = (uint32_t)((((size_t)jk * L + i) * C::N) * sizeof(E));   // byte offset of the row (< 4 GiB: host)
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            const VecE vb = KB.template load16<VecE>(voff, tbl + c * C::T * 16), va = KA.template load16<VecE>(voff, tbl + c * C::T * 16);
#pragma unroll
            for (int e = 0; e < VPL; e++) {
                const int r = c * VPL + e;
                acc0[r] = F::pw_add(acc0[r], F::pw_mul(vb[e], d[r], P.q, P.qinv), P.q, P.q2);
                acc1[r] = F::pw_add(acc1[r], F::pw_mul(va[e], d[r], P.q, P.qinv), P.q, P.q2);
            }
            if ((c & (NCH / 4 - 1)) == NCH / 4 - 1) __builtin_amdgcn_sched_barrier(0);   // a quarter of the key loads (16 VGPRs) in flight at a time
        }
    }
    F::regroup(acc0, P.q, P.qinv);
    inv_core<F, LOGN, false, true>(acc0, lds, tid, P, P.ninv, P.ninv_s, P.ninvw, P.ninvw_s);   // PRESYNC: the last permuted reads are done
    __builtin_amdgcn_sched_barrier(0);
    load_poly_buf<F, LOGN, true>(add0 + (size_t)p * (C::N * sizeof(E)), tid, d);
#pragma unroll
    for (int r = 0; r < 32; r++) acc0[r] = F::ew_add(F::canon_inv(acc0[r], P.q), d[r], P.q);
    lds_put<PatA<LOGN>>(lds, tid, acc0);
    __syncthreads();
    store_from_lds_rolled<F, LOGN>(out0 + (size_t)p * (C::N * 32), lds, tid);
    __builtin_amdgcn_sched_barrier(0);
    F::regroup(acc1, P.q, P.qinv);
    __syncthreads();
    inv_core<F, LOGN>(acc1, lds, tid, P, P.ninv, P.ninv_s, P.ninvw, P.ninvw_s);
#pragma unroll
    for (int r = 0; r < 32; r++) acc1[r] = F::canon_inv(acc1[r], P.q);
    lds_put<PatA<LOGN>>(lds, tid, acc1);
    __syncthreads();
    store_from_lds<F, LOGN>(out1 + (size_t)p * (C::N * 32), lds, tid);
}

}  // namespace fhe_dev
