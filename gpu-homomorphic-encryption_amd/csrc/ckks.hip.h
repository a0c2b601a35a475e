// ckks.hip.h -- the CKKS encoder (fhe_ckks_encode / fhe_ckks_decode / fhe_ckks_decode_poly, include/fhe_hip.h): complex slots <-> real
// polynomials through the canonical embedding, in FP64.  With h = n/2, zeta = exp(i pi / n), omega = zeta^4 = exp(2 pi i / h) and
// e(k) = 3^k mod 2n, the plaintext of z in C^h is the real m of degree < n with m(zeta^e(k)) = z_k.  Exactly one of e(k), 2n - e(k) is 4 a + 1:
// that a is a(k), and c(k) says it was the second (the slot is then stored conjugated).  With u_j = m_j + i m_(j+h) and w_a(k) = z_k or conj(z_k):
//     encode:  u_j = zeta^-j (1/h) sum_a w_a omega^(-a j);    out[b][l][j] = rne(scale m_j) mod q_l   (containers; negative c as q_l - (|c| mod q_l))
//     decode:  w_a = sum_j (u_j zeta^j) omega^(a j);          z_k = w_a(k), conjugated if c(k)
// One workgroup of T = n/32 threads per plaintext, one cyclic complex transform of length h WHOLLY IN LDS: the vector lives there as two planes
// of doubles (real, imaginary; one padding double after every 16, so the 16-element groups of the first pass and the strided groups of the
// later ones both spread over the banks), 17 n / 2 bytes: 17 KiB at n = 2^11, 136 KiB at n = 2^14 (one workgroup per CU there).  A pass takes
// up to four radix-2 stages: a thread reads the 16 elements of its group into registers, runs the stages, writes them back; barriers between
// passes only.  The encode transform is decimation in time from bit-reversed positions, the decode transform decimation in frequency into
// bit-reversed positions, so ONE table serves both: gather[k] = bitrev(a(k)) | c(k) << 31.  Global memory is moved coalesced in slot order and
// the permutation runs through LDS (permuted global accesses lose).
// Twiddles are read, never computed: omega[i] = exp(2 pi i i / h), i < h/2, and twist[j] = zeta^j, j < h, built on the host in long double and
// rounded once (ckks.hip); the inverse direction conjugates them.  No sincos on the device, so the result is a function of (inputs, n, scale,
// moduli) for a given build: nothing depends on the batch, the position in it or the grid.
//   ckks_encode_kernel: slots -> LDS at gather[k] (conjugated where c(k)) -> inverse transform -> per element: times conj(twist), times
//      scale / h, round to nearest even, to int64, back into the same LDS cell as an integer; the largest |c| of the plaintext goes through one
//      LDS atomic to d_coeff_bits[b] -> the coefficients are reduced per limb (ModT of q_l, division-free; host_math.hpp) and stored L times as
//      containers by lane pairs.  HBM: 8 n bytes in, L 32 n bytes out; no workspace.
//   ckks_decode_kernel: 8-byte words (t == 0: two's complement; else centred modulo t) or limb 0 of containers (centred modulo q_0) -> double,
//      times 1 / scale, times twist -> LDS -> forward transform -> slot k reads position gather[k] -> coalesced store.
// d_slots is 8-byte aligned only (an ABI promise), so slots move as pairs of doubles and the compiler picks the access width.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "host_math.hpp"
#include "ntt_field.hip.h"

namespace fhe_dev {

template <int LOGN>
struct CkksCfg {
    static constexpr int LOGH = LOGN - 1;
    static constexpr uint32_t N = 1u << LOGN, H = N / 2, T = N / 32;
    static constexpr uint32_t PLANE = H + H / 16;             // doubles of one padded plane
    static constexpr uint32_t LDS_DOUBLES = 2 * PLANE;
};

FHE_HD uint32_t ckks_phys(uint32_t i) { return i + (i >> 4); }
constexpr uint32_t CKKS_CONJ = 1u << 31;                      // bit of a gather entry: the slot is stored conjugated

// Stages S .. S + K - 1 of the length-2^LOGH transform on the 2^K elements of group g (index bits [S, S + K) vary, the others are g's).
// FWD: decimation in frequency, exponent +, stages in descending order; else decimation in time, exponent -, ascending.
template <int LOGH, int S, int K, bool FWD>
FHE_HD void ckks_pass(double *re, double *im, const double2 *__restrict__ omega, uint32_t g) {
    constexpr uint32_t R = 1u << K;
    const uint32_t lo = g & ((1u << S) - 1);
    const uint32_t base = ((g >> S) << (S + K)) | lo;
    double xr[R], xi[R];
#pragma unroll
    for (uint32_t r = 0; r < R; r++) {
        const uint32_t p = ckks_phys(base + (r << S));
        xr[r] = re[p]; xi[r] = im[p];
    }
#pragma unroll
    for (int tt = 0; tt < K; tt++) {
        const int t = FWD ? K - 1 - tt : tt;                  // stage S + t: partners 2^t apart in r
#pragma unroll
        for (uint32_t jj = 0; jj < (1u << t); jj++) {
            const double2 w = omega[(lo + (jj << S)) << (LOGH - 1 - S - t)];   // exp(2 pi i (index mod 2^(S+t)) / 2^(S+t+1))
#pragma unroll
            for (uint32_t blk = 0; blk < (R >> (t + 1)); blk++) {
                const uint32_t r0 = (blk << (t + 1)) | jj, r1 = r0 | (1u << t);
                if constexpr (FWD) {
                    const double dr = xr[r0] - xr[r1], di = xi[r0] - xi[r1];
                    xr[r0] += xr[r1]; xi[r0] += xi[r1];
                    xr[r1] = dr * w.x - di * w.y; xi[r1] = dr * w.y + di * w.x;
                } else {
                    const double br = xr[r1] * w.x + xi[r1] * w.y, bi = xi[r1] * w.x - xr[r1] * w.y;   // times conj(w)
                    xr[r1] = xr[r0] - br; xi[r1] = xi[r0] - bi;
                    xr[r0] += br; xi[r0] += bi;
                }
            }
        }
    }
#pragma unroll
    for (uint32_t r = 0; r < R; r++) {
        const uint32_t p = ckks_phys(base + (r << S));
        re[p] = xr[r]; im[p] = xi[r];
    }
}

// Centred value of a word: t == 0 two's complement, else w in [0, t) and w > t/2 stands for w - t
FHE_HD double ckks_centre(uint64_t w, uint64_t t) {
    if (!t) return (double)(int64_t)w;
    return w > (t >> 1) ? -(double)(t - w) : (double)w;
}
// rne(v) as a signed 64-bit integer; |v| >= 2^63 saturates (the caller is told by the reported bit length, 64 then)
FHE_HD int64_t ckks_round(double v, uint64_t &mag) {
    const double r = __builtin_rint(v);
    if (!(__builtin_fabs(r) < 9223372036854775808.0)) { mag = ~0ull; return r < 0 ? INT64_MIN : INT64_MAX; }
    const int64_t c = (int64_t)r;
    mag = c < 0 ? (uint64_t)0 - (uint64_t)c : (uint64_t)c;
    return c;
}
// c mod q in [0, q) for the signed c, M = ModT of q
FHE_HD uint64_t ckks_residue(int64_t c, const fhe_host::ModT &M) {
    const uint64_t mag[1] = {c < 0 ? (uint64_t)0 - (uint64_t)c : (uint64_t)c};
    const uint64_t r = fhe_host::modt_reduce<1>(mag, M);
    return (c < 0 && r) ? M.t - r : r;
}

#if defined(__HIPCC__)
// every pass of the transform, a barrier after each; the caller has synchronised before
template <int LOGH, int S, bool FWD>
__device__ __forceinline__ void ckks_transform(double *re, double *im, const double2 *__restrict__ omega, uint32_t tid) {
    if constexpr (S < LOGH) {
        constexpr int K = LOGH - S < 4 ? LOGH - S : 4;
        constexpr uint32_t T = 1u << (LOGH - 4);
        if constexpr (FWD) ckks_transform<LOGH, S + K, FWD>(re, im, omega, tid);
        for (uint32_t g = tid; g < (1u << (LOGH - K)); g += T) ckks_pass<LOGH, S, K, FWD>(re, im, omega, g);
        __syncthreads();
        if constexpr (!FWD) ckks_transform<LOGH, S + K, FWD>(re, im, omega, tid);
    }
}

template <int LOGN>
__global__ void __launch_bounds__(CkksCfg<LOGN>::T)
ckks_encode_kernel(char *__restrict__ out, uint32_t *__restrict__ coeff_bits, const double *__restrict__ slots, const uint32_t *__restrict__ gather,
                   const double2 *__restrict__ twist, const double2 *__restrict__ omega, const fhe_host::ModT *__restrict__ red, double scale_over_h,
                   uint32_t L) {
    using C = CkksCfg<LOGN>;
    __shared__ __attribute__((aligned(16))) double lds[C::LDS_DOUBLES];
    __shared__ unsigned long long lds_max;
    double *re = lds, *im = lds + C::PLANE;
    const uint32_t tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const double *z = slots + b * C::N;
    if (!tid) lds_max = 0;
#pragma unroll
    for (uint32_t r = 0; r < 16; r++) {                       // coalesced, slot order; placed by the gather table
        const uint32_t k = r * C::T + tid;
        const double vr = z[2 * k], vi = z[2 * k + 1];
        const uint32_t gk = gather[k], p = ckks_phys(gk & ~CKKS_CONJ);
        re[p] = vr; im[p] = (gk & CKKS_CONJ) ? -vi : vi;
    }
    __syncthreads();
    ckks_transform<C::LOGH, 0, false>(re, im, omega, tid);
    uint64_t top = 0;
#pragma unroll
    for (uint32_t r = 0; r < 16; r++) {                       // twist, scale, round: the cell keeps the integer
        const uint32_t j = r * C::T + tid, p = ckks_phys(j);
        const double2 w = twist[j];
        const double yr = re[p], yi = im[p];
        uint64_t m0, m1;
        const int64_t c0 = ckks_round((yr * w.x + yi * w.y) * scale_over_h, m0);   // y conj(zeta^j)
        const int64_t c1 = ckks_round((yi * w.x - yr * w.y) * scale_over_h, m1);
        reinterpret_cast<int64_t *>(re)[p] = c0; reinterpret_cast<int64_t *>(im)[p] = c1;
        top = m0 > top ? m0 : top; top = m1 > top ? m1 : top;
    }
    atomicMax(&lds_max, (unsigned long long)top);
    __syncthreads();
    if (!tid && coeff_bits) coeff_bits[b] = lds_max ? 64u - (uint32_t)__clzll((long long)lds_max) : 0u;
    // consecutive lanes write consecutive 16-byte halves (even lane: the residue, odd lane: zeros): 1 KiB contiguous per wave instruction
    const uint32_t half = tid & 1, c0 = tid >> 1;
    char *ob = out + b * L * ((size_t)C::N * 32);
    for (uint32_t l = 0; l < L; l++) {
        const fhe_host::ModT M = red[l];
        v2u64 *dst = reinterpret_cast<v2u64 *>(ob + (size_t)l * (C::N * 32)) + tid;
#pragma unroll 8
        for (uint32_t s = 0; s < 64; s++) {
            const uint32_t x = c0 + (s & 31) * (C::T / 2);
            const int64_t c = reinterpret_cast<const int64_t *>(s < 32 ? re : im)[ckks_phys(x)];
            const v2u64 o = {half ? 0ull : ckks_residue(c, M), 0ull};
            __builtin_nontemporal_store(o, dst + (size_t)s * C::T);
        }
    }
}

// SRC 0: [batch][n] 8-byte words centred modulo t (t == 0: two's complement); SRC 1: limb 0 of [batch][L][n] containers, t = q_0
template <int LOGN, int SRC>
__global__ void __launch_bounds__(CkksCfg<LOGN>::T)
ckks_decode_kernel(double *__restrict__ slots, const char *__restrict__ src, const uint32_t *__restrict__ gather, const double2 *__restrict__ twist,
                   const double2 *__restrict__ omega, uint64_t t, double inv_scale, uint32_t L) {
    using C = CkksCfg<LOGN>;
    __shared__ __attribute__((aligned(16))) double lds[C::LDS_DOUBLES];
    double *re = lds, *im = lds + C::PLANE;
    const uint32_t tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const size_t stride = SRC ? 4 : 1;                        // 8-byte words between coefficients
    const uint64_t *m = reinterpret_cast<const uint64_t *>(src) + (SRC ? b * L * ((size_t)C::N * 4) : b * C::N);
#pragma unroll
    for (uint32_t r = 0; r < 16; r++) {                       // u_j = m_j + i m_(j+h), twisted on the way in
        const uint32_t j = r * C::T + tid, p = ckks_phys(j);
        const double ur = ckks_centre(m[(size_t)j * stride], t) * inv_scale, ui = ckks_centre(m[(size_t)(j + C::H) * stride], t) * inv_scale;
        const double2 w = twist[j];
        re[p] = ur * w.x - ui * w.y; im[p] = ur * w.y + ui * w.x;
    }
    __syncthreads();
    ckks_transform<C::LOGH, 0, true>(re, im, omega, tid);
    double *z = slots + b * C::N;
#pragma unroll
    for (uint32_t r = 0; r < 16; r++) {                       // coalesced, slot order
        const uint32_t k = r * C::T + tid;
        const uint32_t gk = gather[k], p = ckks_phys(gk & ~CKKS_CONJ);
        z[2 * k] = re[p]; z[2 * k + 1] = (gk & CKKS_CONJ) ? -im[p] : im[p];
    }
}
#endif  // __HIPCC__

}  // namespace fhe_dev
