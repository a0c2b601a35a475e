// galois.hip.h -- Galois automorphisms sigma_g: a(x) -> a(x^g) over Z_q[x]/(x^n + 1), g odd, 1 <= g < 2n (slot rotations,
// FHEContext::rotate_rows / rotate_columns, include/fhe.cuh:112-116).  Streaming kernels, compiled into keyswitch.o.
//
// Gather form: output coefficient j reads input coefficient i = j * g^-1 mod 2n and negates it when i >= n (x^n = -1).  Consecutive
// outputs read at stride g^-1 across a limb polynomial.  The STAGED form loads a limb polynomial coalesced into LDS, takes the permuted
// reads from LDS (an odd stride over 4-byte words is bank-conflict-free) and stores coalesced: one workgroup per limb polynomial, up to
// 64 KiB of LDS.  The plain form gathers through L2, one lane per output coefficient.  The host stages a limb polynomial of at most
// GALOIS_STAGE_BYTES: measured faster at 32 KiB (4-byte residues, N = 8192), slower at 64 KiB, where only two workgroups fit a CU
// (DESIGN.md 4.9).
#pragma once
#include "ntt256.hip.h"
#include "ntt_field.hip.h"

namespace fhe_dev {

constexpr uint32_t GALOIS_LDS_BYTES = 64 * 1024;       // largest limb polynomial the staged form holds
constexpr uint32_t GALOIS_STAGE_BYTES = 32 * 1024;     // largest limb polynomial the host runs the staged form on
constexpr uint32_t GALOIS_T = 256;                     // threads per workgroup of every form

// -v mod q for a canonical residue, 0 -> 0 (also exact on the FP64 field: no -0.0)
template <class F>
__device__ __forceinline__ typename F::E galois_neg(typename F::E v, typename F::E q) { return v != (typename F::E)0 ? q - v : (typename F::E)0; }

// where output j of a limb polynomial reads from: index into the input (bits below log_n) and the sign (x^n = -1); 2n divides 2^32,
// so the wrapped 32-bit product is exact modulo 2n
__device__ __forceinline__ uint32_t galois_src(uint32_t j, uint32_t g_inv, uint32_t log_n) { return (j * g_inv) & ((2u << log_n) - 1); }

// One output of the word-sized kernels: COMPACT writes E, else a 32-byte container with zero upper words.  `o` belongs to coefficient g of
// a buffer; every lane of the wave holds one of 64 consecutive coefficients (n is a multiple of 256 on the word-sized classes).
template <class F, bool COMPACT>
__device__ __forceinline__ void galois_put(void *dst, size_t g, typename F::E o) {
    if constexpr (COMPACT) ((typename F::E *)dst)[g] = o;
    else store_wave_containers<F>((typename F::V16 *)dst + 2 * (g - (threadIdx.x & 63)), o);
}

// Work item (component c, limb polynomial p) of a call: sigma_g of in_c[p] into out_c[p]; the component-0 items also clear zero_out[p].
// STAGED: one workgroup per item, the limb polynomial in LDS.  Plain: the workgroups of blockIdx.y = c stride over that component.
template <class F, bool STAGED, bool COMPACT>
__device__ __forceinline__ void galois_body(void *out0, void *out1, void *zero_out, const typename F::V16 *in0, const typename F::V16 *in1,
                                            const Limb<F> *limbs, uint32_t L, uint32_t log_n, uint32_t g_inv, size_t polys) {
    using E = typename F::E;
    const uint32_t n = 1u << log_n, c = blockIdx.y;
    const typename F::V16 *in = c ? in1 : in0;
    void *out = c ? out1 : out0;
    if constexpr (STAGED) {
        extern __shared__ __align__(16) unsigned char galois_lds[];
        E *buf = (E *)galois_lds;
        for (size_t p = blockIdx.x; p < polys; p += gridDim.x) {
            const E q = limbs[(uint32_t)(p % L)].q;
            const size_t base = p << log_n;
            for (uint32_t x = threadIdx.x; x < n; x += GALOIS_T) buf[x] = F::load_low(in + 2 * (base + x));
            __syncthreads();
            for (uint32_t j = threadIdx.x; j < n; j += GALOIS_T) {
                const uint32_t i = galois_src(j, g_inv, log_n);
                const E v = buf[i & (n - 1)];
                galois_put<F, COMPACT>(out, base + j, i >= n ? galois_neg<F>(v, q) : v);
                if (zero_out && !c) galois_put<F, COMPACT>(zero_out, base + j, (E)0);
            }
            __syncthreads();                                            // the next item overwrites buf
        }
    } else {
        const size_t count = polys << log_n, stride = (size_t)gridDim.x * blockDim.x;
        for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count; g += stride) {   // whole waves: count is a multiple of 256
            const size_t p = g >> log_n;
            const uint32_t i = galois_src((uint32_t)(g & (n - 1)), g_inv, log_n);
            const E v = F::load_low(in + 2 * ((p << log_n) + (i & (n - 1))));
            galois_put<F, COMPACT>(out, g, i >= n ? galois_neg<F>(v, limbs[(uint32_t)(p % L)].q) : v);
            if (zero_out && !c) galois_put<F, COMPACT>(zero_out, g, (E)0);
        }
    }
}

// containers in, canonical containers out (fhe_rns_automorphism; the composed rotation: sigma(c0) -> out0, sigma(c1) -> out1, out1 of the
// call cleared through zero_out).  gridDim.y = number of components (1 or 2).
template <class F, bool STAGED>
__global__ void __launch_bounds__(GALOIS_T)
galois_kernel(typename F::V16 *out0, typename F::V16 *out1, typename F::V16 *zero_out, const typename F::V16 *__restrict__ in0,
              const typename F::V16 *__restrict__ in1, const Limb<F> *__restrict__ limbs, uint32_t L, uint32_t log_n, uint32_t g_inv, size_t polys) {
    galois_body<F, STAGED, false>(out0, out1, zero_out, in0, in1, limbs, L, log_n, g_inv, polys);
}

// The rotation prologue of the fused path: ONE launch over both components writes sigma(c0), sigma(c1) and a zero polynomial as compact
// polynomials -- the addend of c0', the digit source and the addend of c1' of the compact-operand key switch (fhe_ct_apply_galois).
template <class F, bool STAGED>
__global__ void __launch_bounds__(GALOIS_T)
galois_compact_kernel(typename F::E *out0, typename F::E *out1, typename F::E *zero_out, const typename F::V16 *__restrict__ in0,
                      const typename F::V16 *__restrict__ in1, const Limb<F> *__restrict__ limbs, uint32_t L, uint32_t log_n, uint32_t g_inv, size_t polys) {
    galois_body<F, STAGED, true>(out0, out1, zero_out, in0, in1, limbs, L, log_n, g_inv, polys);
}

// Full-width class: one lane per output container, the gather through L2 (a 32-byte container per coefficient: n * 32 bytes exceed the
// staged form's LDS from N = 2^11); negation through the borrow chain of u256_dev.h.
__global__ void __launch_bounds__(GALOIS_T)
galois256_kernel(u256 *out0, u256 *out1, u256 *zero_out, const u256 *__restrict__ in0, const u256 *__restrict__ in1, const Limb256 *__restrict__ limbs,
                 uint32_t L, uint32_t log_n, uint32_t g_inv, size_t count /* polys * n */) {
    const uint32_t n = 1u << log_n, c = blockIdx.y;
    const u256 *in = c ? in1 : in0;
    u256 *out = c ? out1 : out0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count; g += stride) {
        const size_t p = g >> log_n;
        const uint32_t i = galois_src((uint32_t)(g & (n - 1)), g_inv, log_n);
        u256 v = load_u256(in + (p << log_n) + (i & (n - 1)));
        if (i >= n && (v.l[0] | v.l[1] | v.l[2] | v.l[3])) { u256 r; sub256(r, limbs[(uint32_t)(p % L)].q, v); v = r; }
        store_u256(out + g, v);
        if (zero_out && !c) { u256 z; z.l[0] = z.l[1] = z.l[2] = z.l[3] = 0; store_u256(zero_out + g, z); }
    }
}

}  // namespace fhe_dev
