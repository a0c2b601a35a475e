// bootstrap.hip.h -- the streaming kernels around the blind-rotation loop (fhe_lwe_prepare_accumulator, fhe_rlwe_sample_extract and its
// strided form fhe_rlwe_sample_extract_strided; contract: include/fhe_hip.h), for moduli below 2^64.  No transform, no workspace: one pass
// over HBM each, launched by bootstrap.hip only.
// No kernel here multiplies: a residue below 2^64 is the low 8 bytes of its container in every width class (the upper 24 bytes are zero), so
// one instance per limb-table type serves every field -- LimbT = Limb<F> of the word-sized classes, Limb256 of an engine whose size has no
// word-sized kernels (n < 2^11) but whose moduli fit a word.
#pragma once
#include "ntt256.hip.h"
#include "ntt_field.hip.h"

namespace fhe_dev {

template <class F> __device__ __forceinline__ uint64_t limb_q64(const Limb<F> &P) { return (uint64_t)P.q; }
__device__ __forceinline__ uint64_t limb_q64(const Limb256 &P) { return P.q.l[0]; }

// ms(v) = floor((v 2n + floor(q_lwe / 2)) / q_lwe) mod 2n for v < q_lwe <= 2^48, n <= 2^16.  v n < 2^64; with v n = A q_lwe + B the value is
// 2 A + floor((2 B + floor(q_lwe / 2)) / q_lwe), and the second quotient is 0, 1 or 2: one division.
__device__ __forceinline__ uint32_t lwe_mod_switch(uint64_t v, uint64_t q_lwe, uint32_t log_n) {
    const uint64_t t = v << log_n, A = t / q_lwe, B = 2 * (t - A * q_lwe) + (q_lwe >> 1);
    const uint64_t r = 2 * A + (B >= q_lwe) + (B >= 2 * q_lwe);
    return (uint32_t)r & ((2u << log_n) - 1);
}

// acc0[b] = X^(2n - ms(b_b)) tv (negacyclic, canonical), acc1[b] = 0, shifts[i][b] = (2n - ms(a_{b,i})) mod 2n.  One 16-byte half container of
// BOTH accumulators per lane (the odd halves and all of acc1 are zero); the rotated read of tv is a shifted contiguous run, so it stays
// coalesced.  tv is read with a TEMPORAL load: it is one [L][n] polynomial that every accumulator of the batch reads, served from L2 after its
// first use (the streaming kernels' own operands use non-temporal loads).  The first n_lwe batch lanes of the grid also write the transposed
// shift table.
template <class LimbT>
__global__ void __launch_bounds__(256)
lwe_prepare_kernel(v2u64 *__restrict__ acc0, v2u64 *__restrict__ acc1, uint32_t *__restrict__ shifts, const uint64_t *__restrict__ lwe,
                   const v2u64 *__restrict__ tv, const LimbT *__restrict__ limbs, uint64_t q_lwe, uint32_t n_lwe, uint32_t batch, uint32_t L,
                   uint32_t log_n, size_t halves) {
    const uint32_t n = 1u << log_n, two_n = 2 * n;
    const size_t stride = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t entries = (size_t)n_lwe * batch;
    for (size_t g = first; g < entries; g += stride) {
        const size_t i = g / batch, b = g - i * batch;
        shifts[g] = (two_n - lwe_mod_switch(lwe[b * (n_lwe + 1) + i], q_lwe, log_n)) & (two_n - 1);
    }
    for (size_t g = first; g < halves; g += stride) {
        uint64_t o = 0;
        if (!(g & 1)) {
            const size_t c = g >> 1, poly = c >> log_n;                   // container index, polynomial index b L + l
            const uint32_t x = (uint32_t)(c & (n - 1)), l = (uint32_t)(poly % L);
            const uint32_t bt = lwe_mod_switch(lwe[(poly / L) * (n_lwe + 1) + n_lwe], q_lwe, log_n);
            uint32_t k = (x + bt) & (two_n - 1);
            const bool neg = k >= n; k &= n - 1;
            o = *reinterpret_cast<const uint64_t *>(tv + (((size_t)l << log_n) + k) * 2);
            if (neg && o) o = limb_q64(limbs[l]) - o;
        }
        const v2u64 v = {o, 0ull}, zero = {0ull, 0ull};
        __builtin_nontemporal_store(v, acc0 + g);
        __builtin_nontemporal_store(zero, acc1 + g);
    }
}

// Sample extraction at coefficient idx: out[p][j] = c1[p][idx - j] (j <= idx), q_l - c1[p][n + idx - j] (idx < j < n, 0 stays 0),
// out[p][n] = c0[p][idx], p = b L + l, as 8-byte residues.  blockIdx.y strides over the polynomials, the lanes of the x dimension over
// j = 0 .. n: the STORES run in lane order (dense 8-byte residues, 512 consecutive bytes per wave instruction) and the index reversal is on the
// LOAD side, where a wave reads the low words of 64 consecutive containers in descending order -- the same 2 KiB of whole cache lines that the
// ascending order touches.  c1 is read once (non-temporal), one container of c0 per polynomial.
template <class LimbT>
__global__ void __launch_bounds__(256)
sample_extract_kernel(uint64_t *__restrict__ out, const v2u64 *__restrict__ c0, const v2u64 *__restrict__ c1, const LimbT *__restrict__ limbs,
                      uint32_t idx, uint32_t L, uint32_t log_n, size_t polys) {
    const uint32_t n = 1u << log_n;
    for (size_t p = blockIdx.y; p < polys; p += gridDim.y) {
        const uint64_t q = limb_q64(limbs[(uint32_t)(p % L)]);
        uint64_t *row = out + p * ((size_t)n + 1);
        for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j <= n; j += gridDim.x * blockDim.x) {
            uint64_t v;
            if (j == n) v = __builtin_nontemporal_load(reinterpret_cast<const uint64_t *>(c0 + ((p << log_n) + idx) * 2));
            else {
                v = __builtin_nontemporal_load(reinterpret_cast<const uint64_t *>(c1 + ((p << log_n) + ((idx - j) & (n - 1))) * 2));
                if (j > idx && v) v = q - v;
            }
            __builtin_nontemporal_store(v, row + j);
        }
    }
}

// Sample extraction at the `count` coefficients idx_i = i n / count of every pair in ONE launch: row (b, i, l) of out, [batch][count][L][n + 1],
// is what sample_extract_kernel writes for polynomial p = b L + l at idx_i.  Row i is row 0 rotated by idx_i, so a lane is bound to ONE source
// coefficient, x = -j0 mod n, j0 its position in row 0: it loads c1[p][x] once, keeps v and q_l - v in registers, and stores one of the two at
// j = (j0 + idx_i) mod n of every row of its block -- the negated value where j0 != 0 and j0 + idx_i < n (then j > idx_i: the source index
// wrapped).  The discipline of the kernel above holds: for one row a wave stores 64 consecutive 8-byte words in lane order (non-temporal; rows
// are n + 1 words long, so their starts alternate between 16- and 8-byte alignment and nothing wider than a word is stored), and the reversal
// is on the load side.  blockIdx.y strides over the polynomials, blockIdx.z splits the rows of one polynomial into runs of `rows_per_block`
// (more workgroups where batch L n alone cannot fill the device): c1 comes from HBM once per ciphertext and is re-read by the gridDim.z - 1
// other blocks of the polynomial through L2, hence the TEMPORAL load.  Lane j0 = i also writes b of row i, c0[p][idx_i].
template <class LimbT>
__global__ void __launch_bounds__(256)
sample_extract_strided_kernel(uint64_t *__restrict__ out, const v2u64 *__restrict__ c0, const v2u64 *__restrict__ c1, const LimbT *__restrict__ limbs,
                              uint32_t log_count, uint32_t rows_per_block, uint32_t L, uint32_t log_n, size_t polys) {
    const uint32_t n = 1u << log_n, count = 1u << log_count, sh = log_n - log_count;
    const size_t row_len = (size_t)n + 1;
    const uint32_t i_lo = blockIdx.z * rows_per_block, i_hi = min(count, i_lo + rows_per_block);
    for (size_t p = blockIdx.y; p < polys; p += gridDim.y) {
        const size_t b = p / L;
        const uint32_t l = (uint32_t)(p - b * L);
        const uint64_t q = limb_q64(limbs[l]);
        uint64_t *rows = out + ((b << log_count) * L + l) * row_len;            // row (b, 0, l); row (b, i, l) is i L row_len words further
        for (uint32_t j0 = blockIdx.x * blockDim.x + threadIdx.x; j0 < n; j0 += gridDim.x * blockDim.x) {
            const uint64_t v = *reinterpret_cast<const uint64_t *>(c1 + ((p << log_n) + ((n - j0) & (n - 1))) * 2);
            const uint64_t vn = (j0 && v) ? q - v : v;
            for (uint32_t i = i_lo; i < i_hi; i++) {
                const uint32_t j = j0 + (i << sh);
                __builtin_nontemporal_store(j < n ? vn : v, rows + (size_t)i * L * row_len + (j & (n - 1)));
            }
            if (j0 >= i_lo && j0 < i_hi)
                __builtin_nontemporal_store(__builtin_nontemporal_load(reinterpret_cast<const uint64_t *>(c0 + ((p << log_n) + ((size_t)j0 << sh)) * 2)),
                                            rows + (size_t)j0 * L * row_len + n);
        }
    }
}

}  // namespace fhe_dev
