// bfv.hip.h -- the two RNS steps of a BFV multiplication on word-sized residues (Halevi, Polyakov and Shoup's "simple scaling" with the
// floating-point sums replaced by 128-bit fixed point, so that both are exact integer functions of their inputs): the centred lift of a
// base B = prod b_i (k primes) to a base C, and the division by Q with rounding from base Q u P (Q = prod q_i, i < L; P = prod p_j, j < L')
// back to base Q.  Definitions: include/fhe_hip.h, BFV section; bfv.hip builds the tables and launches the kernels.
//
// Both are streaming kernels without LDS: ONE lane per coefficient (of one ciphertext component), a grid-stride loop, whole containers
// stored as two nontemporal 16-byte halves by the lane that produced them (as rescale_word_kernel).  Constants are "pw operands"
// (mul_const, ntt_word.hip.h): a residue of one prime of the width class is a valid second operand modulo another as it stands.
// The residues y_i a lane carries from one loop to the next live in a 16-entry register array.  Every loop that READS the array is
// unrolled over its 16 static positions and leaves at the limb count; a loop over the OTHER base stays rolled (its results go straight to
// memory, or into the array through a select over the static positions: set_at), so the code is O(16) products long, not O(16^2), and no
// array is ever indexed dynamically, which would move it to scratch.  BFV_MAX_LIMBS = 16 is therefore the cap on L and on L'.
#pragma once
#include <type_traits>

#include "ntt_word.hip.h"

namespace fhe_dev {

constexpr int BFV_MAX_LIMBS = 16;
constexpr uint32_t BFV_MAX_COMPONENTS = 4;
struct BfvPtrs { const void *in[BFV_MAX_COMPONENTS]; void *out[BFV_MAX_COMPONENTS]; };
// The centred lift B -> C.  E-typed entries are pw operands: minv[i] of (B / b_i)^-1 modulo b_i; mat[i * kc + j] of (B / b_i) mod c_j and
// bmod[j] of B mod c_j, modulo c_j.  r[2 i], r[2 i + 1] = the low and high word of floor(2^128 / b_i).
struct BfvLift { const void *minv, *mat, *bmod; const uint64_t *r; };
// Scale and round.  yinv[i]: operand of (Q P / q_i)^-1 modulo q_i.  Modulo p_j: omega[i * L' + j] of floor(t P / q_i) mod p_j, tq[j] of
// t Q^-1 mod p_j (= (Q P / p_j)^-1 t (P / p_j): the p_j term of the sum, straight from the residue), pow[3 j + k] of 2^(W k) mod p_j
// (W = 32 on the 4-byte and FP64 fields, 64 on the 8-byte integer fields).  rho[2 i], rho[2 i + 1] = floor(2^128 (t P mod q_i) / q_i).
struct BfvScale { const void *yinv, *omega, *tq, *pow; const uint64_t *rho; };

// acc += y * (c_hi 2^64 + c_lo): the exact fixed-point sums (3 words: below 16 * 2^128; 4 words: below 16 * 2^192)
template <int NW>
__device__ __forceinline__ void mac_64x128(uint64_t (&acc)[NW], uint64_t y, uint64_t c_lo, uint64_t c_hi) {
    const u128_t p0 = (u128_t)y * c_lo, p1 = (u128_t)y * c_hi + (uint64_t)(p0 >> 64);
    u128_t s = (u128_t)acc[0] + (uint64_t)p0; acc[0] = (uint64_t)s;
    s = (s >> 64) + acc[1] + (uint64_t)p1; acc[1] = (uint64_t)s;
    s = (s >> 64) + acc[2] + (uint64_t)(p1 >> 64); acc[2] = (uint64_t)s;
    if constexpr (NW == 4) acc[3] += (uint64_t)(s >> 64);
}
template <class E>
__device__ __forceinline__ void set_at(E (&a)[BFV_MAX_LIMBS], uint32_t j, E v) {     // a[j] = v for a wave-uniform j, positions static
#pragma unroll
    for (int k = 0; k < BFV_MAX_LIMBS; k++) a[k] = (uint32_t)k == j ? v : a[k];
}
// (hi 2^64 + lo) mod p for hi < 2^32, as words of W bits times 2^(W k) mod p: no word needs a reduction of its own (to_rns_word_kernel)
template <class F>
__device__ __forceinline__ typename F::E reduce_words(uint64_t lo, uint64_t hi, const typename F::E *pow, const Limb<F> &P) {
    using E = typename F::E;
    if constexpr (sizeof(E) == 8 && !std::is_same<E, double>::value)
        return F::ew_add(mul_const<F>(pow[0], (E)lo, P), mul_const<F>(pow[1], (E)hi, P), P.q);
    else {
        const E o = F::ew_add(mul_const<F>(pow[0], (E)(uint32_t)lo, P), mul_const<F>(pow[1], (E)(uint32_t)(lo >> 32), P), P.q);
        return F::ew_add(o, mul_const<F>(pow[2], (E)(uint32_t)hi, P), P.q);
    }
}
// alpha = floor((sum_i y_i r_i + 2^127) / 2^128) of the k residues y
template <class F>
__device__ __forceinline__ uint32_t lift_alpha(const typename F::E (&y)[BFV_MAX_LIMBS], uint32_t k, const uint64_t *__restrict__ r) {
    uint64_t v[3] = {0, 0, 0};
#pragma unroll
    for (int i = 0; i < BFV_MAX_LIMBS; i++) {
        if ((uint32_t)i >= k) break;
        mac_64x128<3>(v, (uint64_t)y[i], r[2 * i], r[2 * i + 1]);
    }
    return (uint32_t)(v[2] + (v[1] >> 63));
}
// (sum_i y_i ((B / b_i) mod c) - alpha (B mod c)) mod c for the target prime c = D.q; mat points at its column (stride kc)
template <class F>
__device__ __forceinline__ typename F::E lift_residue(const typename F::E (&y)[BFV_MAX_LIMBS], uint32_t k, uint32_t alpha,
                                                      const typename F::E *__restrict__ mat, uint32_t kc, typename F::E bmod, const Limb<F> &D) {
    using E = typename F::E;
    E o = 0;
#pragma unroll
    for (int i = 0; i < BFV_MAX_LIMBS; i++) {
        if ((uint32_t)i >= k) break;
        o = F::ew_add(o, mul_const<F>(mat[(size_t)i * kc], y[i], D), D.q);
    }
    return F::ew_sub(o, mul_const<F>(bmod, (E)alpha, D), D.q);
}
template <class F>
__device__ __forceinline__ void store_container(typename F::V16 *dst, typename F::E o) {
    __builtin_nontemporal_store(F::pack(o), dst);
    __builtin_nontemporal_store(F::pack((typename F::E)0), dst + 1);
}
template <class P>
__device__ __forceinline__ P pick4(P const (&p)[BFV_MAX_COMPONENTS], uint32_t c) {   // (a lane-dependent index into a kernel argument would go through scratch)
    return c == 0 ? p[0] : c == 1 ? p[1] : c == 2 ? p[2] : p[3];
}

// out[b][i][x] = in[b][i][x] for i < L; out[b][L + j][x] = the centred lift of the L residues modulo p_j.  [batch][L][n] -> [batch][L + L'][n]
// for up to four polynomials in one launch.  limbs: the table of the engine on Q u P (Q first).
template <class F>
__global__ void __launch_bounds__(256)
bfv_lift_kernel(BfvPtrs ptrs, const Limb<F> *__restrict__ limbs, BfvLift T, uint32_t L, uint32_t Lp, uint32_t log_n, size_t per_comp /* batch * n */,
                size_t count /* components * batch * n */) {
    using E = typename F::E; using V = typename F::V16;
    const size_t stride = (size_t)gridDim.x * blockDim.x, n = (size_t)1 << log_n;
    const E *__restrict__ minv = (const E *)T.minv, *__restrict__ mat = (const E *)T.mat, *__restrict__ bmod = (const E *)T.bmod;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count; g += stride) {
        const uint32_t c = (g >= per_comp) + (g >= 2 * per_comp) + (g >= 3 * per_comp);
        const size_t r = g - c * per_comp, b = r >> log_n, x = r & (n - 1);
        const V *__restrict__ in = (const V *)pick4(ptrs.in, c) + ((b * L) << log_n) * 2 + x * 2;
        V *__restrict__ out = (V *)pick4(ptrs.out, c) + ((b * (L + Lp)) << log_n) * 2 + x * 2;
        E y[BFV_MAX_LIMBS] = {};
#pragma unroll
        for (int i = 0; i < BFV_MAX_LIMBS; i++) {
            if ((uint32_t)i >= L) break;
            const E xi = F::load_low(in + ((size_t)i << log_n) * 2);
            store_container<F>(out + ((size_t)i << log_n) * 2, xi);
            y[i] = mul_const<F>(minv[i], xi, limbs[i]);
        }
        const uint32_t alpha = lift_alpha<F>(y, L, T.r);
        for (uint32_t j = 0; j < Lp; j++)
            store_container<F>(out + ((size_t)(L + j) << log_n) * 2, lift_residue<F>(y, L, alpha, mat + j, Lp, bmod[j], limbs[L + j]));
    }
}

// [batch][L + L'][n] -> [batch][L][n] for up to three components in one launch: s_j = round(t x / Q) mod p_j from the L + L' residues of x
// (R = the rounded fixed-point sum of the fractional parts, then the integer parts), then the centred lift of s from base P to base Q.  s
// never touches memory.  T lifts P -> Q: its minv / r are indexed by j, its mat is [L'][L], its bmod [L].
template <class F>
__global__ void __launch_bounds__(256)
bfv_scale_round_kernel(BfvPtrs ptrs, const Limb<F> *__restrict__ limbs, BfvScale S, BfvLift T, uint32_t L, uint32_t Lp, uint32_t log_n, size_t per_comp,
                       size_t count) {
    using E = typename F::E; using V = typename F::V16;
    const size_t stride = (size_t)gridDim.x * blockDim.x, n = (size_t)1 << log_n;
    const E *__restrict__ yinv = (const E *)S.yinv, *__restrict__ omega = (const E *)S.omega, *__restrict__ tq = (const E *)S.tq, *__restrict__ pow = (const E *)S.pow;
    const E *__restrict__ pinv = (const E *)T.minv, *__restrict__ mat = (const E *)T.mat, *__restrict__ bmod = (const E *)T.bmod;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count; g += stride) {
        const uint32_t c = (g >= per_comp) + (g >= 2 * per_comp);
        const size_t r = g - c * per_comp, b = r >> log_n, x = r & (n - 1);
        const V *__restrict__ in = (const V *)pick4(ptrs.in, c) + ((b * (L + Lp)) << log_n) * 2 + x * 2;
        V *__restrict__ out = (V *)pick4(ptrs.out, c) + ((b * L) << log_n) * 2 + x * 2;
        E y[BFV_MAX_LIMBS] = {};
        uint64_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < BFV_MAX_LIMBS; i++) {
            if ((uint32_t)i >= L) break;
            y[i] = mul_const<F>(yinv[i], F::load_low(in + ((size_t)i << log_n) * 2), limbs[i]);
            mac_64x128<4>(w, (uint64_t)y[i], S.rho[2 * i], S.rho[2 * i + 1]);
        }
        const uint64_t carry = w[1] >> 63, r_lo = w[2] + carry, r_hi = w[3] + (r_lo < carry);     // R = floor((W + 2^127) / 2^128) < 16 * 2^64
        E yp[BFV_MAX_LIMBS] = {};
        uint64_t v[3] = {0, 0, 0};
        for (uint32_t j = 0; j < Lp; j++) {
            const Limb<F> &D = limbs[L + j];
            E s = reduce_words<F>(r_lo, r_hi, pow + 3 * j, D);
#pragma unroll
            for (int i = 0; i < BFV_MAX_LIMBS; i++) {
                if ((uint32_t)i >= L) break;
                s = F::ew_add(s, mul_const<F>(omega[(size_t)i * Lp + j], y[i], D), D.q);
            }
            s = F::ew_add(s, mul_const<F>(tq[j], F::load_low(in + ((size_t)(L + j) << log_n) * 2), D), D.q);
            const E ypj = mul_const<F>(pinv[j], s, D);
            mac_64x128<3>(v, (uint64_t)ypj, T.r[2 * j], T.r[2 * j + 1]);
            set_at(yp, j, ypj);
        }
        const uint32_t alpha = (uint32_t)(v[2] + (v[1] >> 63));
        for (uint32_t i = 0; i < L; i++)
            store_container<F>(out + ((size_t)i << log_n) * 2, lift_residue<F>(yp, Lp, alpha, mat + i, L, bmod[i], limbs[i]));
    }
}

}  // namespace fhe_dev
