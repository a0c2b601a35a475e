// decrypt.hip.h -- secret-key decryption (fhe_ct_decrypt, include/fhe_hip.h): with v[b][x] the centred representative in (-Q/2, Q/2] of
//     (c0 + c1 s + c2 s^2)[b][x] mod Q,         m[b][x] = ((v mod t) scale) mod t,      noise_bits[b] = bit_length(max_x |v[b][x]|)
// in TWO launches on the LDS-resident sizes:
//   1. ntt_decrypt_kernel: one workgroup per (ciphertext, limb) forms the limb's residue polynomial of c0 + c1 s + c2 s^2 with TWO live arrays
//          x = NTT(c1) . s^;   [y = NTT(c2);  x += s2^ . y;]   x -> INTT -> canonical, + c0 -> compact workspace
//      s^, s2^ = NTT(s), NTT(s)^2 are the packed tables of pack_keys_kernel (times 2^W, in the register order of pattern Z), read through a
//      descriptor; c0 is read through a descriptor as ntt_encrypt_kernel reads m.  HBM: 2 S (3 S) in, L n sizeof(E) out.
//   2. decrypt_crt_kernel: one lane per (ciphertext, coefficient) reads the L residues, forms the CRT sum in the 320-bit accumulator of
//      from_rns_word_kernel, brings it into [0, Q), centres it (negative exactly when it exceeds floor(Q / 2)), reduces |v| modulo t with the
//      division-free reduction of host_math.hpp (ModT), negates modulo t for a negative v, multiplies by scale and stores 8 bytes; the
//      bit length of |v| is reduced over the wave and one atomicMax per wave goes to noise_bits[b] (zeroed by the host before the launch).
// The composed path (decrypt.hip) runs launch 2 on containers; the full-width class has decrypt_crt256_kernel with the tables of from_rns_kernel.
// Ranges of launch 1: c1, c2 canonical -> fwd_core -> [0, 4q) lazy (F52: |.| <= 12 q < 2^47); pw_mul(canonical s^ 2^W, lazy) -> [0, 2q)
// (F52: |.| < 0.76 q) with no 2^-W left; the sum of the two products goes through pw_add -> [0, 2q) (F52: |.| < 1.52 q, then regroup -> < 0.76 q),
// which is what inv_core takes; canon_inv -> [0, q); the addition of c0 is canonical (ew_add).  F64X is canonical throughout.
#pragma once
#include "host_math.hpp"
#include "lds_launch.h"
#include "ntt_lds.hip.h"

namespace fhe_dev {

template <class F, int LOGN, int MINW = 1>
__global__ void __launch_bounds__(NttCfg<LOGN>::T, MINW)
ntt_decrypt_kernel(typename F::E *__restrict__ dec, const char *__restrict__ c0, const char *__restrict__ c1, const char *__restrict__ c2,
                   const typename F::E *__restrict__ sh, const typename F::E *__restrict__ sh2, const Limb<F> *__restrict__ limbs, uint32_t L) {
    using C = NttCfg<LOGN>;
    using E = typename F::E;
    constexpr int VPL = 16 / sizeof(E), NCH = 32 / VPL;
    typedef E VecE __attribute__((ext_vector_type(VPL)));
    __shared__ __attribute__((aligned(16))) E lds[C::LDS_ELEMS];
    const uint32_t tid = threadIdx.x;
    const auto [b, i] = block_map(L);
    const uint32_t p = b * L + i;
    const Limb<F> P = limbs[i];
    const size_t off = (size_t)p * (C::N * 32);
    const uint32_t voff = tid * 16, row = (uint32_t)(((size_t)i * C::N) * sizeof(E));   // byte offset of limb i's row (the tables hold L n residues: far below 4 GiB)
    // c2 is loaded before c1's butterflies, so that its HBM latency hides under them, where the register file allows it: the 512-thread instances
    // of the 8-byte residues (N = 2^14: 256 VGPRs for two 64-register arrays and 16-byte twiddles) would park 12-68 bytes per lane in scratch for it
    constexpr bool EARLY_C2 = !(sizeof(E) == 8 && LOGN >= 14);
    E x[32], y[32];
    load_A<F, LOGN>(c1 + off, tid, x);
    if (EARLY_C2 && c2) load_A<F, LOGN>(c2 + off, tid, y);
    fwd_core<F, LOGN>(x, lds, tid, P);
    __builtin_amdgcn_sched_barrier(0);
    {
        const TableBuf S1(sh);
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            const VecE v = S1.template load16<VecE>(voff, row + c * C::T * 16);
#pragma unroll
            for (int e = 0; e < VPL; e++) x[c * VPL + e] = F::pw_mul(v[e], x[c * VPL + e], P.q, P.qinv);
            if ((c & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // four chunks of table loads in flight at a time
        }
    }
    if (c2) {
        if (!EARLY_C2) load_A<F, LOGN>(c2 + off, tid, y);
        fwd_core<F, LOGN, false, true>(y, lds, tid, P);        // PRESYNC: the Z-pattern reads of c1's transform are done before this exchange
        __builtin_amdgcn_sched_barrier(0);
        const TableBuf S2(sh2);
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            const VecE v = S2.template load16<VecE>(voff, row + c * C::T * 16);
#pragma unroll
            for (int e = 0; e < VPL; e++) x[c * VPL + e] = F::pw_add(x[c * VPL + e], F::pw_mul(v[e], y[c * VPL + e], P.q, P.qinv), P.q, P.q2);
            if ((c & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        F::regroup(x, P.q, P.qinv);
    }
    const TableBuf C0(c0 + (size_t)b * L * (C::N * 32));
    load_src_buf<F, LOGN, false>(C0, i, tid, y);                 // in flight under the inverse transform
    inv_core<F, LOGN>(x, lds, tid, P, P.ninv, P.ninv_s, P.ninvw, P.ninvw_s);   // the slots this thread read last: no barrier needed before
#pragma unroll
    for (int r = 0; r < 32; r++) x[r] = F::ew_add(F::canon_inv(x[r], P.q), y[r], P.q);
    store_A_compact<F, LOGN>(dec + (size_t)p * C::N, tid, x);  // pattern A: consecutive lanes, consecutive words
}

// ---- the CRT launch: streaming kernels, compiled by decrypt.hip alone (it defines FHE_DECRYPT_CRT_KERNELS and includes ntt_word.hip.h first) ----
#ifdef FHE_DECRYPT_CRT_KERNELS
__device__ __forceinline__ uint32_t bit_length256(const uint64_t (&a)[4]) {
    for (int i = 3; i >= 0; i--) if (a[i]) return (uint32_t)(64 * i + 64 - __builtin_clzll(a[i]));
    return 0;
}
// w in [0, Q) -> m and bit_length(|v|), v = w centred.  Q is odd: floor(Q / 2) = (Q - 1) / 2, and w is negative exactly when it exceeds that
__device__ __forceinline__ uint64_t decrypt_finish(uint64_t (&w)[4], const u256 &Q, const fhe_host::ModT &M, uint64_t scale, uint32_t &bits) {
    uint64_t half[4];
#pragma unroll
    for (int i = 0; i < 4; i++) half[i] = (Q.l[i] >> 1) | (i < 3 ? Q.l[i + 1] << 63 : 0);
    bool neg = false;
#pragma unroll
    for (int i = 3; i >= 0; i--) { if (w[i] != half[i]) { neg = w[i] > half[i]; break; } }
    if (neg) {
        uint64_t borrow = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) { const u128_t d = (u128_t)Q.l[i] - w[i] - borrow; w[i] = (uint64_t)d; borrow = (uint64_t)(d >> 64) & 1; }
    }
    bits = bit_length256(w);
    uint64_t r = fhe_host::modt_reduce<4>(w, M);
    if (neg && r) r = M.t - r;
    return fhe_host::modt_mul(r, scale, M);
}
// one atomicMax per wave where a wave's 64 lanes share a ciphertext (n a multiple of 64; the grid-stride loop keeps whole waves together)
__device__ __forceinline__ void decrypt_noise(uint32_t *noise_bits, size_t b, uint32_t bits, uint32_t log_n) {
    if (!noise_bits) return;
    if (log_n >= 6) {
#pragma unroll
        for (int o = 32; o; o >>= 1) { const uint32_t other = (uint32_t)__shfl_xor((int)bits, o, 64); bits = other > bits ? other : bits; }
        if (!(threadIdx.x & 63)) atomicMax(noise_bits + b, bits);
    } else atomicMax(noise_bits + b, bits);
}

// Word-sized classes.  COMPACT: the residues are the compact polynomials ntt_decrypt_kernel wrote ([batch][L][n] of E; F52: exact integers in
// doubles); else [batch][L][n] containers (the composed path).  minv_ops / Mi: the tables of from_rns_word_kernel.
template <class F, bool COMPACT>
__global__ void __launch_bounds__(256)
decrypt_crt_kernel(uint64_t *__restrict__ m, uint32_t *__restrict__ noise_bits, const void *__restrict__ res, const Limb<F> *__restrict__ limbs,
                   const typename F::E *__restrict__ minv_ops, const u256 *__restrict__ Mi, u256 Q, fhe_host::ModT M, uint64_t scale, uint32_t L,
                   uint32_t log_n, size_t count /* batch * n */) {
    using E = typename F::E;
    const size_t stride = (size_t)gridDim.x * blockDim.x, n = (size_t)1 << log_n;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count; g += stride) {
        const size_t b = g >> log_n, x = g & (n - 1);
        uint64_t acc[5] = {0, 0, 0, 0, 0};
        for (uint32_t l = 0; l < L; l++) {
            const size_t at = ((b * L + l) << log_n) + x;
            E r;
            if constexpr (COMPACT) r = reinterpret_cast<const E *>(res)[at];
            else r = F::load_low(reinterpret_cast<const typename F::V16 *>(res) + at * 2);
            const uint64_t tl = (uint64_t)mul_const<F>(minv_ops[l], r, limbs[l]);
            const u256 Ml = Mi[l];
            u128_t c = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) { c += (u128_t)tl * Ml.l[i] + acc[i]; acc[i] = (uint64_t)c; c >>= 64; }
            acc[4] += (uint64_t)c;
        }
        for (uint32_t it = 0; it < L; it++) {                          // acc < L * Q
            bool ge = acc[4] != 0;
            if (!ge) {
                ge = true;
#pragma unroll
                for (int i = 3; i >= 0; i--) { if (acc[i] != Q.l[i]) { ge = acc[i] > Q.l[i]; break; } }
            }
            if (!ge) break;
            uint64_t borrow = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) { const u128_t d = (u128_t)acc[i] - Q.l[i] - borrow; acc[i] = (uint64_t)d; borrow = (uint64_t)(d >> 64) & 1; }
            acc[4] -= borrow;
        }
        uint64_t w[4] = {acc[0], acc[1], acc[2], acc[3]};
        uint32_t bits;
        m[g] = decrypt_finish(w, Q, M, scale, bits);
        decrypt_noise(noise_bits, b, bits, log_n);
    }
}

// Full-width class: the CRT sum of from_rns_kernel (256-bit Montgomery products modulo Q) on containers
__global__ void __launch_bounds__(256)
decrypt_crt256_kernel(uint64_t *__restrict__ m, uint32_t *__restrict__ noise_bits, const u256 *__restrict__ res, const CrtLimb *__restrict__ limbs,
                      const CrtBig big, fhe_host::ModT M, uint64_t scale, uint32_t L, uint32_t log_n, size_t count) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, n = (size_t)1 << log_n;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count; g += stride) {
        const size_t b = g >> log_n, x = g & (n - 1);
        u256 acc; acc.l[0] = acc.l[1] = acc.l[2] = acc.l[3] = 0;
        for (uint32_t l = 0; l < L; l++) {
            const CrtLimb &P = limbs[l];
            const u256 tl = mont_mul(load_u256(res + (b * L + l) * n + x), P.minv_m, P.q, P.inv0);
            acc = add_mod(acc, mont_mul(tl, P.Mi_mQ, big.Q, big.inv0), big.Q);
        }
        uint64_t w[4] = {acc.l[0], acc.l[1], acc.l[2], acc.l[3]};
        uint32_t bits;
        m[g] = decrypt_finish(w, big.Q, M, scale, bits);
        decrypt_noise(noise_bits, b, bits, log_n);
    }
}

#endif  // FHE_DECRYPT_CRT_KERNELS

}  // namespace fhe_dev
