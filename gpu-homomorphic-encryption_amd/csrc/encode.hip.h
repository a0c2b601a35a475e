// encode.hip.h -- the batch encoder (fhe_slots_encode / fhe_slots_decode / fhe_slots_decode_poly, include/fhe_hip.h): with psi = fhe_find_psi(n, t)
// and e(i) the exponent of slot i (fhe_slot_order),
//     encode:  m_b = the polynomial of degree < n over Z_t with m_b(psi^e(i)) = values[b][i];   out[b][l][x] = m_b[x] mod q_l  (containers)
//     decode:  values[b][i] = m_b(psi^e(i)) mod t
// The field F is that of the PLAINTEXT modulus t: the kernels run on the limb table of the one-limb engine on (n, t) that the encoder owns; the
// target engine supplies L and its moduli only.  Position x of the NTT domain holds a(psi^(2 bitrev(x) + 1)), so both slot orders are ONE
// n-entry table, position -> slot index (slot_table, encode.hip), and both orders run the same kernels.
// Global memory is moved COALESCED in slot order and the permutation runs through the exchange buffer (one more LDS round trip per plaintext).
// The other form -- permuted 8-byte global accesses inside the plaintext's window -- is scratch/experiments/slots_global.hip.h: interleaved A/B
// on one MI355X (scratch/experiments/slots_ab.hip, profiles/slots_ab.jsonl): the permuted stores of decode cost 1.3-3.4 x, the permuted loads of
// encode 0-9 % from N = 8192 up (DESIGN 4.14 has the rows).
//   ntt_slots_encode_kernel: one workgroup per plaintext, ONE live array: the slot values are loaded in pattern A and put into the exchange
//      buffer; the thread that owns positions tid 32 .. tid 32 + 31 (pattern Z, what inv_core takes) reads its 32 table entries as eight
//      16-byte loads and picks lds[table[pos]]; one inverse transform with the n^-1 constants; canonical; the coefficients go through the
//      exchange buffer once more and are stored L times as containers by lane pairs (store_from_lds's pattern).  Where t > q_l the residue is
//      reduced with the division-free reduction of host_math.hpp (ModT of q_l; an entry with t == 0 says "no reduction": m < t <= q_l).
//      HBM: 8 n bytes in, L 32 n bytes out; no workspace.
//   ntt_slots_decode_kernel: one workgroup per plaintext: coalesced pattern-A load of 8-byte words (CONTAINERS: of limb 0's low words), one
//      forward transform, canonical, lds[table[pos]] = the value at pos, and the buffer is stored in pattern A.  In place is fine: the
//      workgroup has consumed every load before the transform's first barrier and stores after its last.
// Ranges: values canonical below t -> inv_core takes [0, 2q) (F52: |.| < 0.76 q; canonical inputs are what ntt_inverse_kernel feeds it) -> canon_inv
// -> [0, q).  Decode: canonical -> fwd_core -> [0, 4q) lazy (F52: |.| <= 12 q) -> canon_fwd -> [0, q).  F64X is canonical throughout.
// The streaming kernels of the composed path (sizes outside the LDS-resident range, FHE_HIP_NO_FUSED_ENCODE=1) are at the end, compiled by
// encode.hip alone (it defines FHE_ENCODE_STREAM_KERNELS); they move 8-byte words and containers and know no field.
#pragma once
#include "host_math.hpp"
#include "lds_launch.h"
#include "ntt_lds.hip.h"

namespace fhe_dev {

__device__ __forceinline__ uint32_t slots_phys(uint32_t i) { return i + (i >> 5); }   // slot of the padded exchange buffer

template <class F, int LOGN>
__global__ void __launch_bounds__(NttCfg<LOGN>::T)
ntt_slots_encode_kernel(char *__restrict__ out, const uint64_t *__restrict__ values, const uint32_t *__restrict__ table,
                        const fhe_host::ModT *__restrict__ red, const Limb<F> *__restrict__ limbs, uint32_t L) {
    using C = NttCfg<LOGN>;
    using E = typename F::E;
    __shared__ __attribute__((aligned(16))) E lds[C::LDS_ELEMS];
    const uint32_t tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const Limb<F> P = limbs[0];
    const uint64_t *v = values + b * C::N + tid;
    const v4u32 *tp = reinterpret_cast<const v4u32 *>(table) + tid * 8;
    E x[32];
#pragma unroll
    for (int r = 0; r < 32; r++) x[r] = (E)v[r * C::T];                  // coalesced, slot order
    lds_put<PatA<LOGN>>(lds, tid, x);
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 8; c++) {                                          // the gather, out of the exchange buffer
        const v4u32 i = tp[c];
        x[4 * c + 0] = lds[slots_phys(i.x)]; x[4 * c + 1] = lds[slots_phys(i.y)]; x[4 * c + 2] = lds[slots_phys(i.z)]; x[4 * c + 3] = lds[slots_phys(i.w)];
    }
    inv_core<F, LOGN, false, true>(x, lds, tid, P, P.ninv, P.ninv_s, P.ninvw, P.ninvw_s);   // PRESYNC: the permuted reads are done before the first exchange
#pragma unroll
    for (int r = 0; r < 32; r++) x[r] = F::canon_inv(x[r], P.q);
    lds_put<PatA<LOGN>>(lds, tid, x);      // the slots this thread read last: no barrier needed before
    __syncthreads();
    // consecutive lanes write consecutive 16-byte halves (even lane: the value, odd lane: zeros): 1 KiB contiguous per wave instruction
    const uint32_t half = tid & 1, c0 = tid >> 1;
    const E *p = lds + c0 + (c0 >> 5);
    char *ob = out + b * L * ((size_t)C::N * 32);
    for (uint32_t l = 0; l < L; l++) {
        const fhe_host::ModT M = red[l];
        v2u64 *dst = reinterpret_cast<v2u64 *>(ob + (size_t)l * (C::N * 32)) + tid;
        if (M.t) {                           // t > q_l (uniform over the workgroup)
#pragma unroll 8
            for (int s = 0; s < 64; s++) {
                const uint64_t w[1] = {(uint64_t)p[s * (C::T / 2 + C::T / 64)]};
                const v2u64 o = {half ? 0ull : fhe_host::modt_reduce<1>(w, M), 0ull};
                __builtin_nontemporal_store(o, dst + (size_t)s * C::T);
            }
        } else {
#pragma unroll 16
            for (int s = 0; s < 64; s++) {
                const v2u64 o = {half ? 0ull : (uint64_t)p[s * (C::T / 2 + C::T / 64)], 0ull};
                __builtin_nontemporal_store(o, dst + (size_t)s * C::T);
            }
        }
    }
}

// no __restrict__ on values / src: decoding in place (values == src) is allowed
template <class F, int LOGN, bool CONTAINERS>
__global__ void __launch_bounds__(NttCfg<LOGN>::T)
ntt_slots_decode_kernel(uint64_t *values, const char *src, const uint32_t *__restrict__ table, const Limb<F> *__restrict__ limbs, uint32_t L) {
    using C = NttCfg<LOGN>;
    using E = typename F::E;
    __shared__ __attribute__((aligned(16))) E lds[C::LDS_ELEMS];
    const uint32_t tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const Limb<F> P = limbs[0];
    E x[32];
    if constexpr (CONTAINERS) {
        load_A<F, LOGN>(src + b * L * ((size_t)C::N * 32), tid, x);            // limb 0 of plaintext b
    } else {
        const uint64_t *m = reinterpret_cast<const uint64_t *>(src) + b * C::N + tid;
#pragma unroll
        for (int r = 0; r < 32; r++) x[r] = (E)m[r * C::T];
    }
    fwd_core<F, LOGN>(x, lds, tid, P);
    const v4u32 *tp = reinterpret_cast<const v4u32 *>(table) + tid * 8;
    __syncthreads();                        // every pattern-Z read of the transform is done before the buffer is overwritten
#pragma unroll
    for (int c = 0; c < 8; c++) {           // the scatter, into the exchange buffer
        const v4u32 i = tp[c];
        lds[slots_phys(i.x)] = F::canon_fwd(x[4 * c + 0], P.q, P.q2, P.qinv);
        lds[slots_phys(i.y)] = F::canon_fwd(x[4 * c + 1], P.q, P.q2, P.qinv);
        lds[slots_phys(i.z)] = F::canon_fwd(x[4 * c + 2], P.q, P.q2, P.qinv);
        lds[slots_phys(i.w)] = F::canon_fwd(x[4 * c + 3], P.q, P.q2, P.qinv);
    }
    __syncthreads();
    lds_get<PatA<LOGN>>(lds, tid, x);
    uint64_t *v = values + b * C::N + tid;
#pragma unroll
    for (int r = 0; r < 32; r++) v[r * C::T] = (uint64_t)x[r];             // coalesced, slot order
}

// ---- the composed path: streaming kernels around fhe_rns_ntt_inverse / fhe_rns_ntt_forward of the encoder's engine -------------------------
#ifdef FHE_ENCODE_STREAM_KERNELS
// scratch[b][pos] = values[b][table[pos]] as a container; one lane per container (count = batch n)
__global__ void __launch_bounds__(256)
slots_gather_kernel(v2u64 *__restrict__ scratch, const uint64_t *__restrict__ values, const uint32_t *__restrict__ table, uint32_t log_n, size_t count) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, n = (size_t)1 << log_n;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count; g += stride) {
        const v2u64 lo = {values[(g & ~(n - 1)) + table[g & (n - 1)]], 0ull}, hi = {0ull, 0ull};
        scratch[2 * g] = lo; scratch[2 * g + 1] = hi;
    }
}
// out[b][l][x] = scratch[b][x] mod q_l; one lane per coefficient of a plaintext, L containers each
__global__ void __launch_bounds__(256)
slots_spread_kernel(v2u64 *__restrict__ out, const v2u64 *__restrict__ scratch, const fhe_host::ModT *__restrict__ red, uint32_t L, uint32_t log_n, size_t count) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, n = (size_t)1 << log_n;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count; g += stride) {
        const size_t b = g >> log_n, x = g & (n - 1);
        const uint64_t w[1] = {scratch[2 * g].x};
        for (uint32_t l = 0; l < L; l++) {
            const fhe_host::ModT M = red[l];
            const v2u64 lo = {M.t ? fhe_host::modt_reduce<1>(w, M) : w[0], 0ull}, hi = {0ull, 0ull};
            v2u64 *o = out + 2 * (((b * L + l) << log_n) + x);
            __builtin_nontemporal_store(lo, o); __builtin_nontemporal_store(hi, o + 1);
        }
    }
}
// scratch[b][x] = m[b][x] as a container, from 8-byte words or from the low word of limb 0 of [batch][L][n] containers
__global__ void __launch_bounds__(256)
slots_lift_kernel(v2u64 *__restrict__ scratch, const void *__restrict__ src, uint32_t containers, uint32_t L, uint32_t log_n, size_t count) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, n = (size_t)1 << log_n;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count; g += stride) {
        const size_t b = g >> log_n, x = g & (n - 1);
        const uint64_t w = containers ? reinterpret_cast<const v2u64 *>(src)[2 * (((b * L) << log_n) + x)].x : reinterpret_cast<const uint64_t *>(src)[g];
        const v2u64 lo = {w, 0ull}, hi = {0ull, 0ull};
        scratch[2 * g] = lo; scratch[2 * g + 1] = hi;
    }
}
// values[b][table[pos]] = scratch[b][pos]
__global__ void __launch_bounds__(256)
slots_scatter_kernel(uint64_t *__restrict__ values, const v2u64 *__restrict__ scratch, const uint32_t *__restrict__ table, uint32_t log_n, size_t count) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, n = (size_t)1 << log_n;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count; g += stride)
        values[(g & ~(n - 1)) + table[g & (n - 1)]] = scratch[2 * g].x;
}
#endif  // FHE_ENCODE_STREAM_KERNELS

}  // namespace fhe_dev
