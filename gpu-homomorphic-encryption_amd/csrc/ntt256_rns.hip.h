// ntt256_rns.hip.h -- full-width kernels of the RNS conversions (rns.hip): to / from RNS, rescale, fast base conversion
// (one of the per-subsystem parts of the FHE_WIDTH_256 kernels; the shared types and the design note are in ntt256.hip.h)
#pragma once
#include "ntt256.hip.h"

namespace fhe_dev {

// rns[b][l][x] = values[b][x] mod q_l : mont(mont(v, R^2), 1) is exact for ANY 256-bit v (the sum before the final
// subtraction is below 2q).  One lane per (b, x); the L residues are produced from one load of the value.
__global__ void __launch_bounds__(256)
to_rns_kernel(u256 *__restrict__ rns, const u256 *__restrict__ values, const CrtLimb *__restrict__ limbs, uint32_t L, uint32_t log_n, size_t count) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, n = (size_t)1 << log_n;
    u256 one; one.l[0] = 1; one.l[1] = one.l[2] = one.l[3] = 0;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count; g += stride) {
        const u256 v = load_u256(values + g);
        const size_t b = g >> log_n, x = g & (n - 1);
        for (uint32_t l = 0; l < L; l++) {
            const CrtLimb &P = limbs[l];
            store_u256(rns + (b * L + l) * n + x, mont_mul(mont_mul(v, P.r2, P.q, P.inv0), one, P.q, P.inv0));
        }
    }
}
// values[b][x] = sum_l [r_l * (Q/q_l)^-1]_{q_l} * (Q/q_l) mod Q, accumulated with the 256-bit Montgomery primitives modulo Q.
__global__ void __launch_bounds__(256)
from_rns_kernel(u256 *__restrict__ values, const u256 *__restrict__ rns, const CrtLimb *__restrict__ limbs, const CrtBig big, uint32_t L,
                uint32_t log_n, size_t count) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, n = (size_t)1 << log_n;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count; g += stride) {
        const size_t b = g >> log_n, x = g & (n - 1);
        u256 acc; acc.l[0] = acc.l[1] = acc.l[2] = acc.l[3] = 0;
        for (uint32_t l = 0; l < L; l++) {
            const CrtLimb &P = limbs[l];
            const u256 t = mont_mul(load_u256(rns + (b * L + l) * n + x), P.minv_m, P.q, P.inv0);
            acc = add_mod(acc, mont_mul(t, P.Mi_mQ, big.Q, big.inv0), big.Q);
        }
        store_u256(values + g, acc);
    }
}

// Modulus switching by dropping the last prime (rns_mod_switch_kernel, include/rns.cuh:128-136, undefined in the reference):
// out[b][l][x] = (c[b][l][x] - r) * q_last^-1 mod q_l with r the centred residue modulo q_last, i.e. round(C / q_last) limb-wise.
// One lane per (b, x): the last limb is read once and all L-1 outputs are produced from it.
__global__ void __launch_bounds__(256)
rescale_drop_last_kernel(u256 *__restrict__ out, const u256 *__restrict__ in, const CrtLimb *__restrict__ limbs,
                         const RescaleLimb *__restrict__ rs, uint32_t L, uint32_t log_n, size_t count) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, n = (size_t)1 << log_n;
    u256 one; one.l[0] = 1; one.l[1] = one.l[2] = one.l[3] = 0;
    const u256 ql = limbs[L - 1].q;
    u256 half;                                                       // floor(q_last / 2)
#pragma unroll
    for (int i = 0; i < 4; i++) half.l[i] = (ql.l[i] >> 1) | (i < 3 ? ql.l[i + 1] << 63 : 0);
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count; g += stride) {
        const size_t b = g >> log_n, x = g & (n - 1);
        const u256 cl = load_u256(in + (b * L + (L - 1)) * n + x);
        u256 d; sub256(d, half, cl);                                 // borrow <=> cl > half
        bool neg = false;
#pragma unroll
        for (int i = 3; i >= 0; i--) { if (cl.l[i] != half.l[i]) { neg = cl.l[i] > half.l[i]; break; } }
        u256 mag;
        if (neg) sub256(mag, ql, cl); else mag = cl;
        for (uint32_t l = 0; l + 1 < L; l++) {
            const CrtLimb &P = limbs[l];
            u256 r = mont_mul(mont_mul(mag, P.r2, P.q, P.inv0), one, P.q, P.inv0);          // |r| mod q_l
            if (neg && (r.l[0] | r.l[1] | r.l[2] | r.l[3])) { u256 z; sub256(z, P.q, r); r = z; }
            const u256 diff = sub_mod(load_u256(in + (b * L + l) * n + x), r, P.q);
            store_u256(out + (b * (L - 1) + l) * n + x, mont_mul(diff, rs[l].qlast_inv_m, P.q, P.inv0));
        }
    }
}

// BGV modulus switch (FHEContext::mod_switch_to_next, include/fhe.cuh:109, undefined in the reference): the rescale above with a rounding term
// that is a multiple of t.  u = [-r t^-1]_{q_last} centred, out[b][l][x] = (c[b][l][x] + t u) * q_last^-1 mod q_l, for up to three components in
// one launch.  No CRT constant is read (only q, r2, inv0 of CrtLimb), so the product of the primes may exceed a container.  The magnitude of u
// may exceed q_l (a wider last prime): mont(mag, R^2) is its residue times R for ANY 256-bit value (to_rns_kernel), and the second product with the
// PLAIN constant t q_last^-1 takes the R out again.  One lane per (component, b, x).
__global__ void __launch_bounds__(256)
mod_switch_drop_last_kernel(ModSwitchPtrs ptrs, const CrtLimb *__restrict__ limbs, const ModSwitchLimb *__restrict__ ms, uint32_t L, uint32_t log_n,
                            size_t per_comp /* batch * n */, size_t count /* components * batch * n */) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, n = (size_t)1 << log_n;
    const u256 ql = limbs[L - 1].q;
    const uint64_t ql_inv0 = limbs[L - 1].inv0;
    const u256 u_m = ms[L - 1].qlast_inv_m;
    u256 half;                                                       // floor(q_last / 2)
#pragma unroll
    for (int i = 0; i < 4; i++) half.l[i] = (ql.l[i] >> 1) | (i < 3 ? ql.l[i + 1] << 63 : 0);
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count; g += stride) {
        const uint32_t c = g >= 2 * per_comp ? 2 : g >= per_comp ? 1 : 0;
        const size_t r = g - c * per_comp, b = r >> log_n, x = r & (n - 1);
        const u256 *__restrict__ in = (const u256 *)(c == 0 ? ptrs.in[0] : c == 1 ? ptrs.in[1] : ptrs.in[2]);
        u256 *__restrict__ out = (u256 *)(c == 0 ? ptrs.out[0] : c == 1 ? ptrs.out[1] : ptrs.out[2]);
        const u256 u = mont_mul(load_u256(in + (b * L + (L - 1)) * n + x), u_m, ql, ql_inv0);
        bool neg = false;
#pragma unroll
        for (int i = 3; i >= 0; i--) { if (u.l[i] != half.l[i]) { neg = u.l[i] > half.l[i]; break; } }
        u256 mag;
        if (neg) sub256(mag, ql, u); else mag = u;
        for (uint32_t l = 0; l + 1 < L; l++) {
            const CrtLimb &P = limbs[l];
            const u256 a = mont_mul(load_u256(in + (b * L + l) * n + x), ms[l].qlast_inv_m, P.q, P.inv0);
            const u256 m = mont_mul(mont_mul(mag, P.r2, P.q, P.inv0), ms[l].t_qlast_inv, P.q, P.inv0);
            store_u256(out + (b * (L - 1) + l) * n + x, neg ? sub_mod(a, m, P.q) : add_mod(a, m, P.q));
        }
    }
}

// Fast base conversion (Bajard et al.; fast_base_conversion_kernel, include/rns.cuh:116-125, undefined in the reference):
// out[b][j][x] = sum_i [x_i * (Q/q_i)^-1]_{q_i} * (Q/q_i) mod p_j.  `mat` holds ((Q/q_i) mod p_j) * R_j, row-major [L][Lp].
// One lane per (b, x): the L scaled residues t_i are formed once and reused for every target prime.
constexpr int BASE_CONV_MAX_L = 16;
__global__ void __launch_bounds__(256)
fast_base_convert_kernel(u256 *__restrict__ out, const u256 *__restrict__ in, const CrtLimb *__restrict__ src, uint32_t L,
                         const CrtLimb *__restrict__ dst, uint32_t Lp, const u256 *__restrict__ mat, uint32_t log_n, size_t count) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, n = (size_t)1 << log_n;
    u256 one; one.l[0] = 1; one.l[1] = one.l[2] = one.l[3] = 0;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count; g += stride) {
        const size_t b = g >> log_n, x = g & (n - 1);
        for (uint32_t j = 0; j < Lp; j++) {
            const CrtLimb &D = dst[j];
            u256 acc; acc.l[0] = acc.l[1] = acc.l[2] = acc.l[3] = 0;
            for (uint32_t i = 0; i < L; i++) {
                const CrtLimb &S = src[i];
                const u256 ti = mont_mul(load_u256(in + (b * L + i) * n + x), S.minv_m, S.q, S.inv0);      // [x_i * M_i^-1]_{q_i}
                const u256 ti_m = mont_mul(ti, D.r2, D.q, D.inv0);                                       // (t_i mod p_j) * R_j
                const u256 term = mont_mul(mont_mul(ti_m, load_u256(mat + (size_t)i * Lp + j), D.q, D.inv0), one, D.q, D.inv0);
                acc = add_mod(acc, term, D.q);
            }
            store_u256(out + (b * Lp + j) * n + x, acc);
        }
    }
}

}  // namespace fhe_dev
