// lwe_pack.hip.h -- the streaming kernels of the LWE -> RLWE ring packing (fhe_lwe_to_rlwe, fhe_lwe_pack, fhe_rlwe_pack; contract:
// include/fhe_hip.h), for moduli below 2^64.  No transform, one pass over HBM each, launched by lwe_pack.hip only.  As in bootstrap.hip.h no kernel multiplies by a
// table entry: a residue below 2^64 is the low 8 bytes of its container in every width class (the upper 24 bytes are zero), so one instance
// per limb-table type serves every field, and the one product of the algorithm -- by F^-1, F a power of two, q odd -- is log2 F exact halvings.
// One 16-byte half container of every output per lane: the even halves carry the residue, the odd halves are zero and read nothing.
#pragma once
#include "bootstrap.hip.h"

namespace fhe_dev {

// canonical arithmetic modulo any odd q < 2^64 (a + b may carry out of the word)
__device__ __forceinline__ uint64_t pk_add(uint64_t a, uint64_t b, uint64_t q) { const uint64_t s = a + b; return (s < a || s >= q) ? s - q : s; }
__device__ __forceinline__ uint64_t pk_sub(uint64_t a, uint64_t b, uint64_t q) { return a >= b ? a - b : a - b + q; }
__device__ __forceinline__ uint64_t pk_neg(uint64_t a, uint64_t q) { return a ? q - a : 0; }
// a 2^-k mod q: an odd a becomes (a + q) / 2 = (a >> 1) + (q >> 1) + 1, which is below q
__device__ __forceinline__ uint64_t pk_halve(uint64_t a, uint64_t q, uint32_t k) {
    for (uint32_t i = 0; i < k; i++) a = (a >> 1) + ((a & 1) ? (q >> 1) + 1 : 0);
    return a;
}
// What the embedding reads.  A source gives, of input entry se and limb l -- at(se L + l, ...) says where that is -- c1 of the embedded
// ciphertext at coefficient x, and the constant b that is its c0; each source keeps its own load flavour.
// SampleRows: LWE samples, lwe is [entries][L][n + 1], a row (a_0 .. a_{n-1}, b).  c1 is a_0 at x = 0 and -a_{n-x} elsewhere: a reversed
// contiguous run of the row (descending 8-byte loads: the same whole cache lines as ascending ones).
struct SampleRows {
    const uint64_t *lwe;
    __device__ __forceinline__ const uint64_t *at(size_t poly, uint32_t n, uint32_t) const { return lwe + poly * ((size_t)n + 1); }
    __device__ __forceinline__ uint64_t c1(const uint64_t *row, uint32_t x, uint32_t n, uint64_t q) const {
        const uint64_t v = __builtin_nontemporal_load(row + ((n - x) & (n - 1)));
        return x ? pk_neg(v, q) : v;
    }
    __device__ __forceinline__ uint64_t b(const uint64_t *row, uint32_t n) const { return __builtin_nontemporal_load(row + n); }
};
// RlwePairs: coefficient 0 of RLWE pairs (fhe_rlwe_pack), in0, in1 are [entries][L][n] containers.  Extraction at idx = 0 followed by the embedding
// is the identity on c1 and keeps c0[0] alone, so c1 is read in place, ascending and not negated, and c0 contributes its container 0: the bits
// of SampleRows on the extracted samples, which are never written.  The rest of c0 is not read.
struct RlwePairs {
    const v2u64 *in0, *in1;
    __device__ __forceinline__ size_t at(size_t poly, uint32_t, uint32_t log_n) const { return (poly << log_n) * 2; }   // container 0 of the polynomial, in halves
    __device__ __forceinline__ uint64_t c1(size_t at, uint32_t x, uint32_t, uint64_t) const { return __builtin_nontemporal_load(reinterpret_cast<const uint64_t *>(in1 + at + (size_t)(2 * x))); }   // x < n <= 2^31
    __device__ __forceinline__ uint64_t b(size_t at, uint32_t) const { return __builtin_nontemporal_load(reinterpret_cast<const uint64_t *>(in0 + at)); }
};

// PAIR = false: the embedding of `entries` inputs of the source, (o0, o1) = (c0, c1), times 2^-halvings.
// PAIR = true : the first merge level straight from the source.  Output entry e = b half + r (r < half) pairs input b 2 half + r (E)
//   with input b 2 half + r + half (O); with m = n / 2:  (o0, o1) = P = E + X^m O,  (d0, d1) = D = E - X^m O, all [entries][L][n]
//   containers.  c0 of an embedding is the constant b, so P0 / D0 are zero except at x = 0 (b_E) and x = m (+- b_O).
template <class LimbT, class Source, bool PAIR, class... In>
__global__ void __launch_bounds__(256)
embed_merge_kernel(v2u64 *__restrict__ o0, v2u64 *__restrict__ o1, v2u64 *__restrict__ d0, v2u64 *__restrict__ d1, const In *__restrict__... in,
                   const LimbT *__restrict__ limbs, uint32_t half, uint32_t halvings, uint32_t L, uint32_t log_n, size_t halves /* entries L n 2 */) {
    const uint32_t n = 1u << log_n, m = n >> 1;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const Source src{in...};
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < halves; g += stride) {
        uint64_t p0 = 0, p1 = 0, q0 = 0, q1 = 0;
        if (!(g & 1)) {
            const size_t c = g >> 1, poly = c >> log_n, e = poly / L;            // container, polynomial e L + l, output entry
            const uint32_t x = (uint32_t)(c & (n - 1)), l = (uint32_t)(poly - e * L);
            const uint64_t q = limb_q64(limbs[l]);
            const size_t se = PAIR ? (e / half) * 2 * half + e % half : e;      // input entry of E
            const auto E = src.at(se * L + l, n, log_n);
            const uint64_t e1 = pk_halve(src.c1(E, x, n, q), q, halvings);
            const uint64_t e0 = x ? 0 : pk_halve(src.b(E, n), q, halvings);
            if (PAIR) {
                const auto O = src.at((se + half) * L + l, n, log_n);
                const uint32_t y = (x - m) & (n - 1);                            // (X^m O)[x] = O[x - m], negated where x < m
                uint64_t r1 = pk_halve(src.c1(O, y, n, q), q, halvings);
                uint64_t r0 = y ? 0 : pk_halve(src.b(O, n), q, halvings);
                if (x < m) { r1 = pk_neg(r1, q); r0 = pk_neg(r0, q); }
                p0 = pk_add(e0, r0, q); p1 = pk_add(e1, r1, q);
                q0 = pk_sub(e0, r0, q); q1 = pk_sub(e1, r1, q);
            } else { p0 = e0; p1 = e1; }
        }
        const v2u64 a = {p0, 0ull}, b = {p1, 0ull};
        __builtin_nontemporal_store(a, o0 + g);
        __builtin_nontemporal_store(b, o1 + g);
        if (PAIR) {
            const v2u64 c = {q0, 0ull}, d = {q1, 0ull};
            __builtin_nontemporal_store(c, d0 + g);
            __builtin_nontemporal_store(d, d1 + g);
        }
    }
}

// A later merge level.  The level before left P and G = the key-switched sigma(D) of 2 half results per batch element; its "P + G" is formed here,
// in registers: E = P[b][r] + G[b][r], O = P[b][r + half] + G[b][r + half], and the next P = E + X^m O, D = E - X^m O go out, entry b half + r.
// Both components in one launch (c = 0, 1).  The monomial is a rotated read with a conditional negation, as in lwe_prepare_kernel.
template <class LimbT>
__global__ void __launch_bounds__(256)
lwe_merge_kernel(v2u64 *__restrict__ np0, v2u64 *__restrict__ np1, v2u64 *__restrict__ nd0, v2u64 *__restrict__ nd1, const v2u64 *__restrict__ p0,
                 const v2u64 *__restrict__ p1, const v2u64 *__restrict__ g0, const v2u64 *__restrict__ g1, const LimbT *__restrict__ limbs, uint32_t half,
                 uint32_t m, uint32_t L, uint32_t log_n, size_t halves /* (batch half) L n 2, per component */) {
    const uint32_t n = 1u << log_n;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < halves; g += stride) {
        uint64_t P[2] = {0, 0}, D[2] = {0, 0};
        if (!(g & 1)) {
            const size_t c = g >> 1, poly = c >> log_n, e = poly / L;
            const uint32_t x = (uint32_t)(c & (n - 1)), l = (uint32_t)(poly - e * L);
            const uint64_t q = limb_q64(limbs[l]);
            const size_t ie = (e / half) * 2 * half + e % half;                                    // entry of E in the level before
            const size_t atE = (((ie * L + l) << log_n) + x) * 2, atO = ((((ie + half) * L + l) << log_n) + ((x - m) & (n - 1))) * 2;
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const v2u64 *p = k ? p1 : p0, *gg = k ? g1 : g0;
                const uint64_t E = pk_add(__builtin_nontemporal_load(reinterpret_cast<const uint64_t *>(p + atE)),
                                          __builtin_nontemporal_load(reinterpret_cast<const uint64_t *>(gg + atE)), q);
                uint64_t O = pk_add(__builtin_nontemporal_load(reinterpret_cast<const uint64_t *>(p + atO)),
                                    __builtin_nontemporal_load(reinterpret_cast<const uint64_t *>(gg + atO)), q);
                if (x < m) O = pk_neg(O, q);
                P[k] = pk_add(E, O, q); D[k] = pk_sub(E, O, q);
            }
        }
        const v2u64 a = {P[0], 0ull}, b = {P[1], 0ull}, c = {D[0], 0ull}, d = {D[1], 0ull};
        __builtin_nontemporal_store(a, np0 + g);
        __builtin_nontemporal_store(b, np1 + g);
        __builtin_nontemporal_store(c, nd0 + g);
        __builtin_nontemporal_store(d, nd1 + g);
    }
}

// (o0, o1) = (a0 + b0, a1 + b1): the last "P + G" and every sum of the trace, into the outputs.  o may be a (the trace adds in place): the lane
// that stores a half is the lane that loaded it.  No __restrict__ on those.
template <class LimbT>
__global__ void __launch_bounds__(256)
lwe_pack_sum_kernel(v2u64 *o0, v2u64 *o1, const v2u64 *a0, const v2u64 *a1, const v2u64 *__restrict__ b0, const v2u64 *__restrict__ b1,
                    const LimbT *__restrict__ limbs, uint32_t L, uint32_t log_n, size_t halves) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < halves; g += stride) {
        uint64_t s0 = 0, s1 = 0;
        if (!(g & 1)) {
            const uint64_t q = limb_q64(limbs[(uint32_t)(((g >> 1) >> log_n) % L)]);
            s0 = pk_add(*reinterpret_cast<const uint64_t *>(a0 + g), __builtin_nontemporal_load(reinterpret_cast<const uint64_t *>(b0 + g)), q);
            s1 = pk_add(*reinterpret_cast<const uint64_t *>(a1 + g), __builtin_nontemporal_load(reinterpret_cast<const uint64_t *>(b1 + g)), q);
        }
        const v2u64 u = {s0, 0ull}, v = {s1, 0ull};
        __builtin_nontemporal_store(u, o0 + g);
        __builtin_nontemporal_store(v, o1 + g);
    }
}

}  // namespace fhe_dev
