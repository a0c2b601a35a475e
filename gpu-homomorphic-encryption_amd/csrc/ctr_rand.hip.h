// ctr_rand.hip.h -- the counter-based generator of the samplers (SplitMix64 finaliser over (seed, index, draw)), on its own so that the
// container-level samplers (sampling.hip.h) and the kernels that draw the same values in registers (encrypt.hip.h) share one definition.
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

}  // namespace fhe_dev
