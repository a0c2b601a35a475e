// literal.hip -- the reference's single-modulus kernels as written: 256-bit element-wise primitives, its transform kernels, bit reversal.
#include "engine.h"
#include "ntt256_literal.hip.h"

template <int OP>
static int launch_ew256(void *d_r, const void *d_a, const void *d_b, const uint64_t q[4], const uint64_t *scalar,
                        uint64_t inv0, size_t count, void *stream, const char *what) {
    if (!d_r || !d_a || (OP != 3 && !d_b) || !q) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": null argument");
    if (int rc = check_aligned({d_r, d_a, d_b}, what)) return rc;
    int rc = ensure_device(); if (rc) return rc;
    if (!count) return FHE_OK;
    hipStream_t s = (hipStream_t)stream;
    fhe_dev::u256 Q = to_dev(q), S = scalar ? to_dev(scalar) : Q;
    hipLaunchKernelGGL(fhe_dev::ew256_kernel<OP>, dim3(ew_grid(count)), dim3(256), 0, s, (fhe_dev::u256 *)d_r,
                       (const fhe_dev::u256 *)d_a, (const fhe_dev::u256 *)d_b, Q, S, inv0, count);
    return post_launch(s, what);
}
extern "C" int fhe_u256_add_mod(void *r, const void *a, const void *b, const uint64_t q[4], size_t count, void *stream) {
    return launch_ew256<1>(r, a, b, q, nullptr, 0, count, stream, "fhe_u256_add_mod");
}
extern "C" int fhe_u256_sub_mod(void *r, const void *a, const void *b, const uint64_t q[4], size_t count, void *stream) {
    return launch_ew256<2>(r, a, b, q, nullptr, 0, count, stream, "fhe_u256_sub_mod");
}
extern "C" int fhe_u256_mont_mul(void *r, const void *a, const void *b, const uint64_t q[4], uint64_t inv0, size_t count, void *stream) {
    return launch_ew256<0>(r, a, b, q, nullptr, inv0, count, stream, "fhe_u256_mont_mul");
}
extern "C" int fhe_u256_mont_mul_scalar(void *r, const void *a, const uint64_t scalar[4], const uint64_t q[4], uint64_t inv0, size_t count, void *stream) {
    if (!scalar) return fail(FHE_ERR_INVALID_ARG, "scalar is null");
    return launch_ew256<3>(r, a, nullptr, q, scalar, inv0, count, stream, "fhe_u256_mont_mul_scalar");
}

// the reference's transform kernels as written (L1 parity; see ntt256.hip.h)
static int ref_literal_check(const void *d_data, const void *d_table, const uint64_t q[4], uint32_t n, uint32_t batch, const char *what) {
    if (!d_data || !d_table || !q) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": null argument");
    if (int rc = check_aligned({d_data, d_table}, what)) return rc;
    if (n < 2 || (n & (n - 1)) || n > 65536) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": n must be a power of two in [2, 65536]");
    if (!batch) return fail(FHE_ERR_INVALID_ARG, std::string(what) + ": batch must be >= 1");
    return ensure_device();
}
extern "C" int fhe_ref_forward_kernel_literal(void *d_data, const void *d_twiddles, const uint64_t q[4], uint64_t inv0, uint32_t n, uint32_t batch, void *stream) {
    int rc = ref_literal_check(d_data, d_twiddles, q, n, batch, "fhe_ref_forward_kernel_literal"); if (rc) return rc;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fhe_dev::ref_forward_literal_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, (fhe_dev::u256 *)d_data,
                       (const fhe_dev::u256 *)d_twiddles, to_dev(q), inv0, n);
    return post_launch((hipStream_t)stream, "ref_forward_literal_kernel");
}
extern "C" int fhe_ref_inverse_kernel_literal(void *d_data, const void *d_inv_twiddles, const uint64_t q[4], uint64_t inv0, const uint64_t n_inv[4],
                                              uint32_t n, uint32_t batch, void *stream) {
    int rc = ref_literal_check(d_data, d_inv_twiddles, q, n, batch, "fhe_ref_inverse_kernel_literal"); if (rc) return rc;
    if (!n_inv) return fail(FHE_ERR_INVALID_ARG, "fhe_ref_inverse_kernel_literal: n_inv is null");
    (void)hipGetLastError();
    hipLaunchKernelGGL(fhe_dev::ref_inverse_literal_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, (fhe_dev::u256 *)d_data,
                       (const fhe_dev::u256 *)d_inv_twiddles, to_dev(q), inv0, to_dev(n_inv), n);
    return post_launch((hipStream_t)stream, "ref_inverse_literal_kernel");
}

extern "C" int fhe_ref_stockham_stage_literal(void *d_output, const void *d_input, const void *d_twiddles, const uint64_t q[4], uint64_t inv0, uint32_t n,
                                             uint32_t stage, uint32_t batch, void *stream) {
    int rc = ref_literal_check(d_output, d_twiddles, q, n, batch, "fhe_ref_stockham_stage_literal"); if (rc) return rc;
    if (!d_input || d_input == d_output) return fail(FHE_ERR_INVALID_ARG, "fhe_ref_stockham_stage_literal: the stage is out of place");
    if ((rc = check_aligned({d_input}, "fhe_ref_stockham_stage_literal"))) return rc;
    if ((2u << stage) > n) return fail(FHE_ERR_INVALID_ARG, "fhe_ref_stockham_stage_literal: stage must satisfy 2^(stage+1) <= n");
    (void)hipGetLastError();
    const size_t count = (size_t)batch * (n / 2);
    hipLaunchKernelGGL(fhe_dev::ref_stockham_stage_kernel, dim3(ew_grid(count)), dim3(256), 0, (hipStream_t)stream, (fhe_dev::u256 *)d_output,
                       (const fhe_dev::u256 *)d_input, (const fhe_dev::u256 *)d_twiddles, to_dev(q), inv0, n, stage, count);
    return post_launch((hipStream_t)stream, "ref_stockham_stage_kernel");
}

extern "C" int fhe_bit_reverse(void *d_data, uint32_t n, uint32_t batch, void *stream) {
    if (!d_data) return fail(FHE_ERR_INVALID_ARG, "fhe_bit_reverse: null argument");
    if (int rc = check_aligned({d_data}, "fhe_bit_reverse")) return rc;
    if (n < 2 || (n & (n - 1))) return fail(FHE_ERR_INVALID_ARG, "fhe_bit_reverse: n must be a power of two >= 2");
    if (!batch) return fail(FHE_ERR_INVALID_ARG, "fhe_bit_reverse: batch must be >= 1");
    int rc = ensure_device(); if (rc) return rc;
    (void)hipGetLastError();
    uint32_t log_n = 0; while ((1u << log_n) < n) log_n++;
    const size_t count = (size_t)batch * n;
    hipLaunchKernelGGL(fhe_dev::bit_reverse_kernel, dim3(ew_grid(count)), dim3(256), 0, (hipStream_t)stream, (fhe_dev::u256 *)d_data, log_n, count);
    return post_launch((hipStream_t)stream, "bit_reverse_kernel");
}
