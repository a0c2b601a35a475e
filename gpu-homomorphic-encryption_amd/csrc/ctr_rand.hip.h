// ctr_rand.hip.h -- the counter-based generator of the samplers (SplitMix64 finaliser over (seed, index, draw)) and the Gaussian draw on it, on
// their own so that the container-level kernels (sampling.hip.h, encrypt.hip, keygen.hip) and the kernels that draw the same values in registers
// (encrypt.hip.h, keygen.hip.h) share one definition.  No kernel is defined here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fhe_dev {

__device__ __host__ inline uint64_t sm64(uint64_t z) {          // SplitMix64 output function
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// the part of ctr_rand that the draws of one (seed, element) share
__device__ __host__ inline uint64_t ctr_base(uint64_t seed, uint64_t index) { return sm64(seed ^ (index * 0xD1342543DE82EF95ull)); }
// 64 random bits for (seed, element index, draw number)
__device__ __host__ inline uint64_t ctr_rand(uint64_t seed, uint64_t index, uint64_t draw) { return sm64(ctr_base(seed, index) + draw); }
enum : uint64_t { DRAW_TERNARY = 0, DRAW_CDT = 1, DRAW_SIGN = 2, DRAW_UNIFORM = 16 };

// The discrete Gaussian of element `index` of stream `seed` by inversion of a cumulative table: magnitude #{ j < len : r >= cdt[j] } for the
// 64 bits r of one draw, sign from a second.  The container-level kernels scan the table (constant work per coefficient); the fused
// kernels take the same two draws and count with cdt_count below.
struct GaussianDraw { uint32_t mag; bool neg; };
__device__ __forceinline__ GaussianDraw gaussian_draw(uint64_t seed, uint64_t index, const uint64_t *cdt, uint32_t len) {
    const uint64_t base = ctr_base(seed, index), r = sm64(base + DRAW_CDT);
    uint32_t mag = 0;
    for (uint32_t j = 0; j < len; j++) mag += r >= cdt[j] ? 1u : 0u;
    return {mag, (sm64(base + DRAW_SIGN) >> 63) != 0};
}
// count = #{ j < len : r >= cdt[j] } of a non-decreasing table: the largest pos <= len with cdt[pos - 1] <= r, by binary lifting from
// top = the largest power of two <= len.  Constant trip count, no divergence.
__device__ __forceinline__ uint32_t cdt_count(const uint64_t *cdt, uint32_t len, uint32_t top, uint64_t r) {
    uint32_t pos = 0;
    for (uint32_t s = top; s; s >>= 1) {
        const uint32_t idx = pos + s, at = (idx <= len ? idx : len) - 1;
        pos = (idx <= len && cdt[at] <= r) ? idx : pos;
    }
    return pos;
}

}  // namespace fhe_dev
