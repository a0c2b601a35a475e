// slots_global.hip.h -- the batch encoder's gather / scatter by PERMUTED GLOBAL ACCESSES instead of through the exchange buffer (the adopted
// form: csrc/encode.hip.h).  Same arguments, same results.  Encode gathers values[b][table[pos]] with 8-byte loads, decode stores
// values[b][table[pos]] with 8-byte stores, both inside the 16-128 KiB window of one plaintext, which the workgroup touches completely.  One
// LDS round trip and one (encode) or two (decode) barriers fewer per plaintext -- and slower: a wave's permuted stores write partial lines
// (decode 1.3-3.4 x the time of the adopted form), the permuted loads cost 0-9 % from N = 8192 up and win 1-5 % at N = 2048 only.
// Measured by scratch/experiments/slots_ab.hip (profiles/slots_ab.jsonl).  Not adopted.
#pragma once
#include "../../gpu-homomorphic-encryption_amd/csrc/encode.hip.h"

namespace fhe_dev {

template <class F, int LOGN>
__global__ void __launch_bounds__(NttCfg<LOGN>::T)
ntt_slots_encode_global_kernel(char *__restrict__ out, const uint64_t *__restrict__ values, const uint32_t *__restrict__ table,
                               const fhe_host::ModT *__restrict__ red, const Limb<F> *__restrict__ limbs, uint32_t L) {
    using C = NttCfg<LOGN>;
    using E = typename F::E;
    __shared__ __attribute__((aligned(16))) E lds[C::LDS_ELEMS];
    const uint32_t tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const Limb<F> P = limbs[0];
    const uint64_t *v = values + b * C::N;
    const v4u32 *tp = reinterpret_cast<const v4u32 *>(table) + tid * 8;
    E x[32];
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const v4u32 i = tp[c];
        x[4 * c + 0] = (E)v[i.x]; x[4 * c + 1] = (E)v[i.y]; x[4 * c + 2] = (E)v[i.z]; x[4 * c + 3] = (E)v[i.w];
    }
    inv_core<F, LOGN>(x, lds, tid, P, P.ninv, P.ninv_s, P.ninvw, P.ninvw_s);
#pragma unroll
    for (int r = 0; r < 32; r++) x[r] = F::canon_inv(x[r], P.q);
    lds_put<PatA<LOGN>>(lds, tid, x);
    __syncthreads();
    const uint32_t half = tid & 1, c0 = tid >> 1;
    const E *p = lds + c0 + (c0 >> 5);
    char *ob = out + b * L * ((size_t)C::N * 32);
    for (uint32_t l = 0; l < L; l++) {
        const fhe_host::ModT M = red[l];
        v2u64 *dst = reinterpret_cast<v2u64 *>(ob + (size_t)l * (C::N * 32)) + tid;
        if (M.t) {
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

template <class F, int LOGN, bool CONTAINERS>
__global__ void __launch_bounds__(NttCfg<LOGN>::T)
ntt_slots_decode_global_kernel(uint64_t *values, const char *src, const uint32_t *__restrict__ table, const Limb<F> *__restrict__ limbs, uint32_t L) {
    using C = NttCfg<LOGN>;
    using E = typename F::E;
    __shared__ __attribute__((aligned(16))) E lds[C::LDS_ELEMS];
    const uint32_t tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const Limb<F> P = limbs[0];
    E x[32];
    if constexpr (CONTAINERS) {
        load_A<F, LOGN>(src + b * L * ((size_t)C::N * 32), tid, x);
    } else {
        const uint64_t *m = reinterpret_cast<const uint64_t *>(src) + b * C::N + tid;
#pragma unroll
        for (int r = 0; r < 32; r++) x[r] = (E)m[r * C::T];
    }
    fwd_core<F, LOGN>(x, lds, tid, P);
    uint64_t *v = values + b * C::N;
    const v4u32 *tp = reinterpret_cast<const v4u32 *>(table) + tid * 8;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const v4u32 i = tp[c];
        v[i.x] = (uint64_t)F::canon_fwd(x[4 * c + 0], P.q, P.q2, P.qinv);
        v[i.y] = (uint64_t)F::canon_fwd(x[4 * c + 1], P.q, P.q2, P.qinv);
        v[i.z] = (uint64_t)F::canon_fwd(x[4 * c + 2], P.q, P.q2, P.qinv);
        v[i.w] = (uint64_t)F::canon_fwd(x[4 * c + 3], P.q, P.q2, P.qinv);
    }
}

}  // namespace fhe_dev
