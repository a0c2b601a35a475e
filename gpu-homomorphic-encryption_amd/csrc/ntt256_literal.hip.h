// ntt256_literal.hip.h -- the reference's single-modulus kernels as written (literal.hip): element-wise primitives, transform kernels, bit reversal
// (one of the per-subsystem parts of the FHE_WIDTH_256 kernels; the shared types and the design note are in ntt256.hip.h)
#pragma once
#include "ntt256.hip.h"

namespace fhe_dev {

// Literal element-wise primitives with one modulus passed by value:
// batch_mod_add_kernel / batch_mod_sub_kernel / batch_mod_mul_kernel (src/bigint.cu:171-214),
// poly_add_kernel / poly_sub_kernel / poly_mul_scalar_kernel (src/polynomial.cu:70-111),
// ntt_pointwise_mul_kernel (kernels/ntt_kernels.cu:124-137).
// OP 0: mont(a,b); 1: add; 2: sub; 3: mont(a, scalar)
template <int OP>
__global__ void __launch_bounds__(256)
ew256_kernel(u256 *r, const u256 *a, const u256 *b,                  // no __restrict__: callers pass r == a (in-place mul_scalar, add_rns(acc, acc, tmp))
             const u256 q, const u256 scalar, uint64_t inv0, size_t count) {
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count; g += stride) {
        u256 x = load_u256(a + g), o;
        if (OP == 3) o = mont_mul(x, scalar, q, inv0);
        else {
            u256 y = load_u256(b + g);
            if (OP == 0) o = mont_mul(x, y, q, inv0);
            else if (OP == 1) o = add_mod(x, y, q);
            else o = sub_mod(x, y, q);
        }
        store_u256(r + g, o);
    }
}

// ---- the reference's transform kernels AS WRITTEN (L1 parity) ---------------------------------------------------------
// ntt_forward_optimized_kernel / ntt_inverse_optimized_kernel (kernels/ntt_kernels.cu:7-62, :65-121), launched by
// NTTEngine::forward / inverse as ONE block of n threads (src/ntt.cu:30-47): stage schedule with log_n = popc(n-1)+1 (sic),
// butterfly pairs (k*2m + j, k*2m + j + m) only where the second index < block size (= n), twiddle index j << (log_n-stage-1),
// caller-supplied tables (the reference fills them with placeholders, src/ntt.cu:86-97), literal mul_mod_montgomery /
// add_mod / sub_mod.  The n "threads" of the reference's block are walked by the lanes of one workgroup (within a stage every
// thread owns a private pair, so the order inside a stage is irrelevant); the data stay in device memory instead of the
// reference's dynamic shared memory (n * 32 bytes: beyond any LDS for n > 4096), which changes nothing observable.
// One workgroup per polynomial of a [batch][n] buffer.  bit_reverse_kernel is not applied (out-of-bounds accesses there make
// its result undefined); these kernels are what the reference's own source computes on the data it is given.
__global__ void __launch_bounds__(256)
ref_forward_literal_kernel(u256 *__restrict__ data, const u256 *__restrict__ tw, u256 q, uint64_t inv0, uint32_t n) {
    u256 *d = data + (size_t)blockIdx.x * n;
    const uint32_t log_n = (uint32_t)__popc(n - 1) + 1;
    for (uint32_t stage = 0; stage < log_n; stage++) {
        const uint32_t m = 1u << stage, m2 = m << 1;
        for (uint32_t tid = threadIdx.x; tid < n; tid += blockDim.x) {
            const uint32_t k = tid / m, j = tid % m;
            if ((uint64_t)k * m2 + j + m < n) {
                const uint32_t idx1 = k * m2 + j, idx2 = idx1 + m;
                const u256 u = load_u256(d + idx1);
                const u256 v = mont_mul(load_u256(d + idx2), load_u256(tw + (j << (log_n - stage - 1))), q, inv0);
                store_u256(d + idx1, add_mod(u, v, q));
                store_u256(d + idx2, sub_mod(u, v, q));
            }
        }
        __syncthreads();
    }
}
__global__ void __launch_bounds__(256)
ref_inverse_literal_kernel(u256 *__restrict__ data, const u256 *__restrict__ itw, u256 q, uint64_t inv0, u256 n_inv, uint32_t n) {
    u256 *d = data + (size_t)blockIdx.x * n;
    const uint32_t log_n = (uint32_t)__popc(n - 1) + 1;
    for (int stage = (int)log_n - 1; stage >= 0; stage--) {
        const uint32_t m = 1u << stage, m2 = m << 1;
        for (uint32_t tid = threadIdx.x; tid < n; tid += blockDim.x) {
            const uint32_t k = tid / m, j = tid % m;
            if ((uint64_t)k * m2 + j + m < n) {
                const uint32_t idx1 = k * m2 + j, idx2 = idx1 + m;
                const u256 u = load_u256(d + idx1), v = load_u256(d + idx2);
                store_u256(d + idx1, add_mod(u, v, q));
                store_u256(d + idx2, mont_mul(sub_mod(u, v, q), load_u256(itw + (j << (log_n - (uint32_t)stage - 1))), q, inv0));
            }
        }
        __syncthreads();
    }
    for (uint32_t tid = threadIdx.x; tid < n; tid += blockDim.x) store_u256(d + tid, mont_mul(load_u256(d + tid), n_inv, q, inv0));
}

// ntt_stockham_kernel (kernels/ntt_kernels.cu:213-243; never launched by the reference): ONE out-of-place butterfly stage,
// output[idx1] = input[idx1] + mont(input[idx2], tw[j * (n / 2m)]), output[idx2] = input[idx1] - ..., idx1 = k*2m + j, idx2 = idx1 + m.
// As written the kernel runs idx over [0, n) and indexes past the arrays for idx >= n/2 (undefined); this restatement runs the
// n/2 in-bounds butterflies, which are all of a stage.  One lane per butterfly, [batch][n] polynomials.
__global__ void __launch_bounds__(256)
ref_stockham_stage_kernel(u256 *__restrict__ output, const u256 *__restrict__ input, const u256 *__restrict__ tw, u256 q, uint64_t inv0,
                          uint32_t n, uint32_t stage, size_t count /* batch * n/2 */) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const uint32_t m = 1u << stage, m2 = m << 1, half = n >> 1;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count; g += stride) {
        const size_t b = g / half; const uint32_t idx = (uint32_t)(g % half);
        const uint32_t k = idx / m, j = idx % m, idx1 = k * m2 + j, idx2 = idx1 + m;
        const u256 *in = input + b * n; u256 *out = output + b * n;
        const u256 u = load_u256(in + idx1);
        const u256 v = mont_mul(load_u256(in + idx2), load_u256(tw + j * (n / m2)), q, inv0);
        store_u256(out + idx1, add_mod(u, v, q));
        store_u256(out + idx2, sub_mod(u, v, q));
    }
}

// bit_reverse_kernel's intent (kernels/ntt_kernels.cu:140-161): in-place bit-reversal permutation of each polynomial, swapping
// only where idx < rev(idx).  The reference reverses over popc(n-1)+1 = log2(n)+1 bits, which sends half of the indices past
// the array (undefined); this kernel reverses over log2(n) bits.  It converts between natural order and the order
// fhe_ntt_forward leaves its values in (X[k] sits at position bitrev(k)).
__global__ void __launch_bounds__(256)
bit_reverse_kernel(u256 *__restrict__ data, uint32_t log_n, size_t count /* batch * n */) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const uint32_t n = 1u << log_n;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count; g += stride) {
        const uint32_t idx = (uint32_t)(g & (n - 1));
        const uint32_t rev = __brev(idx) >> (32 - log_n);
        if (idx < rev) {
            u256 *d = data + (g - idx);
            const u256 a = load_u256(d + idx), b = load_u256(d + rev);
            store_u256(d + idx, b);
            store_u256(d + rev, a);
        }
    }
}

}  // namespace fhe_dev
