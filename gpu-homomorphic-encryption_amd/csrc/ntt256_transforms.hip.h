// ntt256_transforms.hip.h -- container-level kernels of the transform subsystem (transforms.hip) on full-width handles: the per-limb
// element-wise ops (product, add, sub, the literal R = 2^256 Montgomery product) and the canonical-residue check.  They work on u256
// containers with Limb256 constants and mont_mul_fips / mont_mul of u256_dev.h.  The full-width TRANSFORMS are not here: the global-memory
// passes, the LDS tiles and the NTT-domain products are the kernels of ntt_wide.hip.h.  (Shared types: ntt256.hip.h.)
#pragma once
#include "ntt256.hip.h"

namespace fhe_dev {

// Element-wise over [batch][L][n] with per-limb moduli.  OP 0: plain product a*b mod q
// (= mont(mont(a,b), R^2)); 1: add_mod; 2: sub_mod; 3: literal mul_mod_montgomery(a, b) (rns_mul_kernel).
template <int OP>
__global__ void __launch_bounds__(256)
ew256_rns_kernel(u256 *r, const u256 *a, const u256 *b,              // no __restrict__: r may be a or b (in-place add / sub / product)
                 const Limb256 *__restrict__ limbs, uint32_t L, uint32_t log_n, size_t count) {
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count; g += stride) {
        const Limb256 &P = limbs[(uint32_t)((g >> log_n) % L)];
        u256 x = load_u256(a + g), y = load_u256(b + g), o;
        if (OP == 0) o = mont_mul_fips(mont_mul_fips(x, y, P.q, (uint32_t)P.inv0), P.r2, P.q, (uint32_t)P.inv0);
        else if (OP == 1) o = add_mod(x, y, P.q);
        else if (OP == 2) o = sub_mod(x, y, P.q);
        else o = mont_mul(x, y, P.q, P.inv0);          // 3: rns_mul_kernel, literal (src/rns.cu:160-181): carries R^-1
        store_u256(r + g, o);
    }
}

__global__ void __launch_bounds__(256)
check256_kernel(const u256 *__restrict__ a, const Limb256 *__restrict__ limbs, uint32_t L, uint32_t log_n,
                size_t count, uint32_t *__restrict__ flag) {
    size_t stride = (size_t)gridDim.x * blockDim.x;
    uint32_t bad = 0;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count; g += stride) {
        const u256 q = limbs[(uint32_t)((g >> log_n) % L)].q;
        u256 x = load_u256(a + g), d;
        // x >= q  <=>  x - q does not borrow
        uint64_t borrow = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            u128_t t = (u128_t)x.l[i] - q.l[i] - borrow;
            d.l[i] = (uint64_t)t; borrow = (uint64_t)(t >> 64) & 1;
        }
        bad |= (borrow == 0);
    }
    if (bad) atomicOr(flag, 1u);
}

}  // namespace fhe_dev
