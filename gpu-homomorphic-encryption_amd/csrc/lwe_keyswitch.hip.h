// lwe_keyswitch.hip.h -- LWE key switching from the ring key back to the small LWE key (fhe_lwe_keyswitch, fhe_lwe_ksk_generate; contract:
// include/fhe_hip.h), for one modulus q below 2^64.  Launched by lwe_keyswitch.hip only.
//
// Key table.  [R][ncp] uint64_t, R = n_in K rows, ncp = n_out + 1 rounded up to the wave width (64); the padding columns are zero.  Row
// r = j K + k is (a_{r,0} .. a_{r,n_out-1}, b_r, 0 ..): a wave instruction of the apply kernel reads 512 consecutive bytes of one row.
//
// Apply.  out = D [batch][R] x KSK [R][n_out + 1] mod q with the digits D taken from the input on the fly.  A workgroup owns TB ciphertexts
// times 64 columns, one column per lane; its waves split the input coefficients j (all K digits of a coefficient stay in one wave) and fold
// their partial sums through LDS, one wave after the other, at the end.  The input values of the tile are wave-uniform: they are read through
// the scalar cache and the digit is a scalar shift and mask, so the inner loop is one 8-byte key load per lane and row and TB
// multiply-adds.  A ciphertext index past the batch is clamped on the load side and skipped on the store side; a column past n_out reads
// the zero padding and is not stored.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ctr_rand.hip.h"
#include "u256_dev.h"

namespace fhe_dev {

constexpr uint32_t LWE_KS_COLS = 64;      // columns of a workgroup's tile: one per lane
constexpr uint32_t LWE_KS_THREADS = 1024; // 16 waves split the rows
constexpr uint32_t LWE_KEYGEN_THREADS = 256;

// (hi 2^64 + lo) mod q by restoring division, q < 2^64: 64 steps, once per output value
__device__ __forceinline__ uint64_t lwe_mod128(uint64_t hi, uint64_t lo, uint64_t q) {
    uint64_t r = hi % q;
    for (int i = 63; i >= 0; i--) {
        const uint64_t top = r >> 63;
        r = (r << 1) | ((lo >> i) & 1);
        if (top || r >= q) r -= q;
    }
    return r;
}
__device__ __forceinline__ uint64_t lwe_mul_mod(uint64_t a, uint64_t b, uint64_t q) {
    const u128_t p = (u128_t)a * b;
    return lwe_mod128((uint64_t)(p >> 64), (uint64_t)p, q);
}
__device__ __forceinline__ uint64_t lwe_add_mod(uint64_t a, uint64_t b, uint64_t q) {      // a, b < q < 2^64: the sum may carry out of 64 bits
    const uint64_t s = a + b;
    return (s < a || s >= q) ? s - q : s;
}
// floor((v q_out + floor(q / 2)) / q) mod q_out for v < q, 2 <= q_out <= 2^48: the numerator is below q (q_out + 1), so its upper word is
// below q and the quotient is at most q_out
__device__ __forceinline__ uint64_t lwe_round_to(uint64_t v, uint64_t q, uint64_t q_out) {
    const u128_t num = (u128_t)v * q_out + (q >> 1);
    uint64_t r = (uint64_t)(num >> 64), quo = 0;
    const uint64_t lo = (uint64_t)num;
    for (int i = 63; i >= 0; i--) {
        const uint64_t top = r >> 63;
        r = (r << 1) | ((lo >> i) & 1);
        quo <<= 1;
        if (top || r >= q) { r -= q; quo |= 1; }
    }
    return quo >= q_out ? quo - q_out : quo;
}

// WIDE = false: bit_length(q) + w + ceil(log2 R) <= 64, the whole sum fits 64 bits; WIDE = true: 128-bit accumulators (a term is below
// 2^96 and R <= 2^22).  Both are reduced once per wave at the end.
template <bool WIDE> struct LweAcc;
template <> struct LweAcc<false> {
    uint64_t v = 0;
    __device__ __forceinline__ void mad(uint32_t d, uint64_t k) { v += (uint64_t)d * k; }
    __device__ __forceinline__ uint64_t reduce(uint64_t q) const { return v % q; }
};
template <> struct LweAcc<true> {
    u128_t v = 0;
    __device__ __forceinline__ void mad(uint32_t d, uint64_t k) { v += (u128_t)k * d; }
    __device__ __forceinline__ uint64_t reduce(uint64_t q) const { return lwe_mod128((uint64_t)(v >> 64), (uint64_t)v, q); }
};

template <uint32_t TB, bool WIDE>
__global__ void __launch_bounds__(LWE_KS_THREADS)
lwe_keyswitch_kernel(uint64_t *__restrict__ out, const uint64_t *__restrict__ in, const uint64_t *__restrict__ ksk, uint64_t q, uint64_t q_out,
                     uint32_t n_in, uint32_t n_out, uint32_t ncp, uint32_t K, uint32_t w, uint32_t batch) {
    __shared__ uint64_t fold[TB][LWE_KS_COLS];
    constexpr uint32_t WAVES = LWE_KS_THREADS / 64;
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t col = blockIdx.x * LWE_KS_COLS + lane;                       // < ncp: the grid covers exactly ncp / 64 column tiles
    const uint32_t per = (n_in + WAVES - 1) / WAVES, j0 = min(wave * per, n_in), j1 = min(j0 + per, n_in);
    const uint64_t mask = w == 32 ? 0xffffffffull : (1ull << w) - 1;
    const size_t row_in = (size_t)n_in + 1, row_out = (size_t)n_out + 1;
    const uint32_t tiles = (batch + TB - 1) / TB;
    for (uint32_t tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
        const uint32_t b0 = tile * TB;
        LweAcc<WIDE> acc[TB];
        const uint64_t *src[TB];
#pragma unroll
        for (uint32_t t = 0; t < TB; t++) src[t] = in + (size_t)min(b0 + t, batch - 1) * row_in;
        for (uint32_t j = j0; j < j1; j++) {
            uint64_t v[TB];
#pragma unroll
            for (uint32_t t = 0; t < TB; t++) v[t] = src[t][j];
            const uint64_t *kp = ksk + (size_t)j * K * ncp + col;
#pragma unroll 4
            for (uint32_t k = 0; k < K; k++) {
                const uint64_t kv = kp[(size_t)k * ncp];
                const uint32_t sh = k * w;
#pragma unroll
                for (uint32_t t = 0; t < TB; t++) acc[t].mad((uint32_t)((v[t] >> sh) & mask), kv);
            }
        }
        // every wave reduces its partial sums below q, then the waves fold them, one after the other
        uint64_t red[TB];
#pragma unroll
        for (uint32_t t = 0; t < TB; t++) red[t] = acc[t].reduce(q);
        for (uint32_t turn = 0; turn < WAVES; turn++) {
            if (wave == turn) {
#pragma unroll
                for (uint32_t t = 0; t < TB; t++) fold[t][lane] = turn ? lwe_add_mod(fold[t][lane], red[t], q) : red[t];
            }
            __syncthreads();
        }
        // epilogue, every thread of the workgroup: TB * 64 values
        for (uint32_t o = threadIdx.x; o < TB * LWE_KS_COLS; o += LWE_KS_THREADS) {
            const uint32_t t = o >> 6, b = b0 + t, c = blockIdx.x * LWE_KS_COLS + (o & 63);
            if (b < batch && c <= n_out) {
                uint64_t r = fold[t][o & 63];
                if (c == n_out) r = lwe_add_mod(r, __builtin_nontemporal_load(in + (size_t)b * row_in + n_in), q);
                if (q_out) r = lwe_round_to(r, q, q_out);
                __builtin_nontemporal_store(r, out + (size_t)b * row_out + c);
            }
        }
        __syncthreads();            // the next tile's first turn overwrites fold
    }
}

// Key generation: one workgroup per row r = j K + k.  A lane draws the uniform a_{r,i} of its columns in registers, writes them and sums
// a_{r,i} |z_i| apart for the two signs of z_i (a term is below 2^79, at most 256 per lane); the workgroup folds sum a z mod q through LDS and
// lane 0 adds the gadget term s_j 2^(k w) and the noise.  The padding columns of the row are written as zeros.
__global__ void __launch_bounds__(LWE_KEYGEN_THREADS)
lwe_ksk_keygen_kernel(uint64_t *__restrict__ ksk, const uint64_t *__restrict__ s /* containers of limb 0: 4 words per coefficient */,
                      const int32_t *__restrict__ z, const uint64_t *__restrict__ cdt, uint32_t cdt_len, uint64_t q, uint64_t noise_scale,
                      uint64_t seed_a, uint64_t seed_e, uint32_t n_out, uint32_t ncp, uint32_t K, uint32_t w, uint32_t R) {
    __shared__ uint64_t part[LWE_KEYGEN_THREADS];
    const int bits = 64 - __builtin_clzll(q);
    const uint64_t mask = bits == 64 ? ~0ull : ((1ull << bits) - 1);
    for (uint32_t r = blockIdx.x; r < R; r += gridDim.x) {
        uint64_t *row = ksk + (size_t)r * ncp;
        u128_t pos = 0, neg = 0;
        for (uint32_t i = threadIdx.x; i < n_out; i += LWE_KEYGEN_THREADS) {
            const uint64_t g = (uint64_t)r * n_out + i;
            uint64_t a;
            for (uint32_t t = 0;; t++) {
                a = ctr_rand(seed_a, g, DRAW_UNIFORM + 4 * t) & mask;
                if (a < q) break;
                if (t == 63) { a &= mask >> 1; break; }
            }
            row[i] = a;
            const int32_t zi = z[i];
            if (zi >= 0) pos += (u128_t)a * (uint32_t)zi; else neg += (u128_t)a * (uint32_t)(-zi);
        }
        for (uint32_t i = n_out + 1 + threadIdx.x; i < ncp; i += LWE_KEYGEN_THREADS) row[i] = 0;
        const uint64_t p = lwe_mod128((uint64_t)(pos >> 64), (uint64_t)pos, q), m = lwe_mod128((uint64_t)(neg >> 64), (uint64_t)neg, q);
        part[threadIdx.x] = p >= m ? p - m : p + (q - m);                       // (p - m) mod q without leaving 64 bits
        __syncthreads();
        for (uint32_t h = LWE_KEYGEN_THREADS / 2; h; h >>= 1) {
            if (threadIdx.x < h) part[threadIdx.x] = lwe_add_mod(part[threadIdx.x], part[threadIdx.x + h], q);
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const uint32_t j = r / K, k = r - j * K;
            const uint64_t gadget = lwe_mul_mod(s[(size_t)j * 4], (1ull << (k * w)) % q, q);
            const GaussianDraw e = gaussian_draw(seed_e, r, cdt, cdt_len);
            uint64_t noise = lwe_mul_mod(noise_scale % q, e.mag, q);
            if (e.neg && noise) noise = q - noise;
            const uint64_t az = part[0], t = lwe_add_mod(gadget, noise, q);
            row[n_out] = t >= az ? t - az : t + (q - az);
        }
        __syncthreads();            // part is rewritten by the next row
    }
}

// canonical [R][n_out + 1] <-> internal [R][ncp]; to_internal writes the zero padding too.  One lane per internal element.
__global__ void __launch_bounds__(256)
lwe_ksk_repack_kernel(uint64_t *__restrict__ dst, const uint64_t *__restrict__ src, uint32_t n_out, uint32_t ncp, size_t count /* R ncp */, int to_internal) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count; g += stride) {
        const size_t r = g / ncp; const uint32_t c = (uint32_t)(g - r * ncp);
        if (to_internal) dst[g] = c <= n_out ? src[r * ((size_t)n_out + 1) + c] : 0;
        else if (c <= n_out) dst[r * ((size_t)n_out + 1) + c] = src[g];
    }
}

}  // namespace fhe_dev
