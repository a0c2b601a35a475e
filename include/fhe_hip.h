/*
 * fhe_hip.h -- C ABI of the MI355X (gfx950) RNS-NTT polynomial-multiply engine.
 *
 * This is the drop-in boundary for the reference's hot path.  The reference
 * (codebasecomprehension987/gpu-homomorphic-encryption) has no FFI layer of its own: its boundary is
 * the C++ class surface fhe::NTTEngine / RNS_NTTEngine / PolynomialOps / FHEContext::multiply.
 * Every entry point below names the reference interface it replaces (file:line, relative to the
 * reference root).  The C++ mirror of those classes lives in include/fhe/ and is a header-only
 * wrapper over this ABI; INTEGRATION.md shows the binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - 256-bit values are the reference's `uint256_t` (include/bigint.cuh:9-11): 4 x uint64_t,
 *     little-endian limbs, 32 bytes.  Host-side moduli are passed as `const uint64_t[4]` (8-byte aligned).
 *   - `d_*` arguments are raw DEVICE pointers owned by the caller (hipMalloc / fhe_hip_malloc /
 *     torch tensor storage), exactly as the reference takes cudaMalloc'd pointers (src/ntt.cu:30-75).
 *   - Every `d_*` pointer to containers must be 16-byte aligned: the kernels move a container as two 16-byte
 *     halves.  An allocation base is, and so is any whole-container slice of a buffer that is (offsets are
 *     multiples of 32 bytes).  A pointer that is not is rejected with FHE_ERR_INVALID_ARG before anything is
 *     launched.  (`d_shifts` arrays hold uint32_t and need 4-byte alignment only.)
 *   - Polynomial data is limb-major `[batch][L][n]` containers (src/ntt.cu:161).
 *   - Coefficients handed to the NTT entry points must be canonical residues (< q_limb).
 *   - Work is enqueued on the handle's stream and NOT synchronised (callers sync, as the
 *     reference's callers do: tests/test_fhe.cu:88,97,155), unless env FHE_HIP_SYNC=1.
 *   - Every function returns 0 on success or a negative fhe_status; fhe_hip_last_error() gives the
 *     message of the calling thread's last failure.  (The reference reports no errors at all.)
 *   - A handle is bound to the device that was current at creation and is not thread-safe; distinct
 *     handles may be used from distinct threads (docs/API_REFERENCE.md:600-606).
 *   - There is NO CPU fallback: without a usable HIP device every compute entry point fails with
 *     FHE_ERR_NO_DEVICE.
 */
#ifndef FHE_HIP_H
#define FHE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FHE_HIP_ABI_VERSION 1

typedef enum fhe_status {
    FHE_OK = 0,
    FHE_ERR_INVALID_ARG = -1,   /* null pointer, n not a power of two, batch == 0 ... */
    FHE_ERR_BAD_MODULUS = -2,   /* even, >= 2^255, not prime, or q != 1 (mod 2n) */
    FHE_ERR_NO_DEVICE = -3,     /* no HIP device / HIP runtime failure at init */
    FHE_ERR_HIP = -4,           /* a HIP call failed; message holds hipGetErrorString */
    FHE_ERR_UNSUPPORTED = -5,   /* size outside what the kernels were built for */
    FHE_ERR_NONCANONICAL = -6   /* fhe_*_check found coefficients >= q in a fast-path buffer */
} fhe_status;

/* Which kernel family a modulus set selected (reported, never chosen by the caller). */
typedef enum fhe_width_class {
    FHE_WIDTH_32 = 1,    /* every q < 2^30 : 32-bit lazy Shoup butterflies, whole NTT in LDS */
    FHE_WIDTH_64 = 2,    /* every q < 2^62 : 64-bit lazy butterflies, whole NTT in LDS */
    FHE_WIDTH_52 = 3,    /* every q < 2^43 : residues as exact integers in doubles, FP64 FMA butterflies, whole NTT in LDS */
    FHE_WIDTH_256 = 4,   /* anything else < 2^255 : full 4x64-bit Montgomery (R = 2^256), multi-pass */
    FHE_WIDTH_64X = 5    /* every q < 2^64 (some q >= 2^62): 64-bit canonical butterflies (carry-aware add / sub, one-word
                            Montgomery twiddles), whole NTT in LDS */
} fhe_width_class;

typedef struct fhe_ntt fhe_ntt_t;          /* replaces fhe::NTTEngine      (include/ntt.cuh:72-103)  */
typedef struct fhe_rns_ntt fhe_rns_ntt_t;  /* replaces fhe::RNS_NTTEngine  (include/ntt.cuh:106-137) */

/* ---- library / device plumbing (the reference calls the CUDA runtime directly) ------------- */
int fhe_hip_abi_version(void);
const char *fhe_hip_last_error(void);
int fhe_hip_device_count(int *count);
int fhe_hip_set_device(int device);
int fhe_hip_get_device(int *device);
int fhe_hip_device_name(char *buf, size_t buflen);            /* gcnArchName + marketing name */
int fhe_hip_malloc(void **d_ptr, size_t bytes);               /* cudaMalloc   (src/polynomial.cu:8) */
int fhe_hip_free(void *d_ptr);                                /* cudaFree     (src/polynomial.cu:13) */
int fhe_hip_memset(void *d_ptr, int value, size_t bytes);     /* cudaMemset   (src/polynomial.cu:9) */
int fhe_hip_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes);
int fhe_hip_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes);
int fhe_hip_memcpy_d2d(void *d_dst, const void *d_src, size_t bytes);
int fhe_hip_sync(void);                                       /* cudaDeviceSynchronize (tests/test_fhe.cu:88) */

/* ---- host-side parameter maths ------------------------------------------------------------ */
/* compute_montgomery_inverse (src/bigint.cu:23-40): inv[0] = -q^-1 mod 2^64 by 6 Newton steps,
 * inv[1..3] = 0.  Literal, including the deterministic garbage for even q. */
int fhe_montgomery_inverse(const uint64_t q[4], uint64_t inv[4]);
/* compute_montgomery_params (src/bigint.cu:42-55) with r_squared actually computed. */
int fhe_montgomery_params(const uint64_t q[4], uint64_t r_squared[4], uint64_t inv[4]);
/* find_ntt_prime / generate_rns_primes (include/rns.cuh:139-149; src/rns.cu:183-209 are stubs):
 * the `count` smallest primes >= 2^(bits-1) with q = 1 (mod 2n); bits <= 64. */
int fhe_find_ntt_primes(uint32_t bits, uint32_t n, uint32_t count, uint64_t *primes_out);
/* the same search for moduli of any width the engine accepts (bits <= 255), as 4 x u64 little-endian containers */
int fhe_find_ntt_primes_wide(uint32_t bits, uint32_t n, uint32_t count, uint64_t (*primes_out)[4]);
/* find_primitive_root (src/ntt.cu:110-114 is a stub): primitive 2n-th root of unity psi, chosen as
 * the first x^((q-1)/2n), x = 2,3,..., whose n-th power is q-1. */
int fhe_find_psi(uint32_t n, const uint64_t q[4], uint64_t psi[4]);

/* ---- element-wise 256-bit modular kernels, literal reference semantics ---------------------- */
/* batch_mod_add_kernel (src/bigint.cu:171-184) / poly_add_kernel (src/polynomial.cu:70-82):
 * r[i] = add_mod(a[i], b[i], q)  (include/bigint.cuh:27-48).  stream may be NULL (default stream). */
int fhe_u256_add_mod(void *d_r, const void *d_a, const void *d_b, const uint64_t q[4], size_t count, void *stream);
/* batch_mod_sub_kernel (src/bigint.cu:186-199) / poly_sub_kernel (src/polynomial.cu:84-96). */
int fhe_u256_sub_mod(void *d_r, const void *d_a, const void *d_b, const uint64_t q[4], size_t count, void *stream);
/* batch_mod_mul_kernel (src/bigint.cu:201-214) / ntt_pointwise_mul_kernel (kernels/ntt_kernels.cu:124-137):
 * r[i] = mul_mod_montgomery(a[i], b[i], q, inv)  (include/bigint.cuh:76-140); only inv0 = inv.limbs[0] is used. */
int fhe_u256_mont_mul(void *d_r, const void *d_a, const void *d_b, const uint64_t q[4], uint64_t inv0, size_t count, void *stream);
/* poly_mul_scalar_kernel (src/polynomial.cu:98-111): r[i] = mul_mod_montgomery(a[i], scalar, q, inv). */
int fhe_u256_mont_mul_scalar(void *d_r, const void *d_a, const uint64_t scalar[4], const uint64_t q[4], uint64_t inv0, size_t count, void *stream);

/* ---- the reference's transform kernels AS WRITTEN (L1 parity) ---------------------------------------------- */
/* ntt_forward_optimized_kernel (kernels/ntt_kernels.cu:7-62) exactly as NTTEngine::forward launches it (one block of n threads,
 * src/ntt.cu:30-40, WITHOUT the out-of-bounds bit_reverse_kernel): stage schedule log_n = popc(n-1)+1, pairs
 * (k*2m + j, k*2m + j + m) where the second index < n, twiddle index j << (log_n - stage - 1), caller-supplied table of n
 * containers (the reference fills it with the placeholders [1, 1, 2, 3, ...], src/ntt.cu:86-97), literal primitives.  This is
 * what the reference's source computes on the data it is given -- not an NTT with those tables; fhe_ntt_forward is the real
 * transform.  [batch][n] polynomials, one workgroup each; n a power of two up to 65536 (the reference itself cannot launch n > 1024). */
int fhe_ref_forward_kernel_literal(void *d_data, const void *d_twiddles, const uint64_t q[4], uint64_t inv0, uint32_t n, uint32_t batch, void *stream);
/* ntt_inverse_optimized_kernel (kernels/ntt_kernels.cu:65-121): the same pairs in reverse stage order, Gentleman-Sande form,
 * then every element mont(x, n_inv). */
int fhe_ref_inverse_kernel_literal(void *d_data, const void *d_inv_twiddles, const uint64_t q[4], uint64_t inv0, const uint64_t n_inv[4],
                                   uint32_t n, uint32_t batch, void *stream);

/* ntt_stockham_kernel (kernels/ntt_kernels.cu:213-243, never launched by the reference): one out-of-place butterfly stage,
 * out[i1] = in[i1] + mont(in[i2], tw[j * n / 2m]), out[i2] = in[i1] - ..., i1 = k*2m + j, i2 = i1 + m, m = 2^stage.  The n/2
 * in-bounds butterflies are run (as written the kernel also indexes past the arrays for idx >= n/2: undefined). */
int fhe_ref_stockham_stage_literal(void *d_output, const void *d_input, const void *d_twiddles, const uint64_t q[4], uint64_t inv0, uint32_t n,
                                   uint32_t stage, uint32_t batch, void *stream);

/* bit_reverse_kernel's intent (kernels/ntt_kernels.cu:140-161): in-place bit-reversal permutation of every polynomial of a
 * [batch][n] buffer over log2(n) bits (the reference's popc(n-1)+1 bits index out of bounds).  The engine's transforms need no
 * such pass (DIF/DIT pairing); this entry converts between natural order and the order fhe_ntt_forward leaves its values in. */
int fhe_bit_reverse(void *d_data, uint32_t n, uint32_t batch, void *stream);

/* ---- single-modulus engine: fhe::NTTEngine -------------------------------------------------- */
/* NTTEngine::NTTEngine(n, modulus) (src/ntt.cu:7-22) + precompute_twiddle_factors (:77-107), with the
 * root / inverse / table placeholders replaced by real values.  q prime, q = 1 (mod 2n), q < 2^255,
 * 8 <= n <= 65536 a power of two. */
int fhe_ntt_create(fhe_ntt_t **out, uint32_t n, const uint64_t q[4]);
int fhe_ntt_destroy(fhe_ntt_t *h);                                            /* ~NTTEngine (src/ntt.cu:24-28) */
int fhe_ntt_set_stream(fhe_ntt_t *h, void *stream);   /* adopt a caller stream (e.g. torch's); NULL = back to the private one */
int fhe_ntt_width_class(const fhe_ntt_t *h);
/* NTTEngine::forward (src/ntt.cu:30-40) / forward_batch (include/ntt.cuh:87): in place, `batch`
 * polynomials contiguous [batch][n]; natural order in, merged-CT (bit-reversed) order out. */
int fhe_ntt_forward(fhe_ntt_t *h, void *d_data, uint32_t batch);
/* NTTEngine::inverse (src/ntt.cu:42-47) / inverse_batch (include/ntt.cuh:88): exact inverse of
 * forward including the n^-1 scaling (kernels/ntt_kernels.cu:117-120). */
int fhe_ntt_inverse(fhe_ntt_t *h, void *d_data, uint32_t batch);
/* ntt_pointwise_mul_kernel's intent (kernels/ntt_kernels.cu:124-137): r = a .* b mod q, plain product. */
int fhe_ntt_pointwise(fhe_ntt_t *h, void *d_r, const void *d_a, const void *d_b, uint32_t batch);
/* NTTEngine::multiply (src/ntt.cu:49-75): r = a (*) b mod (x^n + 1, q); d_a, d_b are not modified unless d_r aliases
 * one of them, which is allowed (in-place product, squaring with d_a == d_b).  One fused launch on the word-sized paths; with
 * d_a == d_b the squaring form of the kernel runs (one load, one forward transform: 2*S bytes of traffic instead of 3*S). */
int fhe_ntt_multiply(fhe_ntt_t *h, void *d_r, const void *d_a, const void *d_b, uint32_t batch);

/* ---- RNS engine: fhe::RNS_NTTEngine ---------------------------------------------------------- */
/* RNS_NTTEngine::RNS_NTTEngine(n, rns_moduli, num_primes) (src/ntt.cu:122-145): moduli are copied. */
int fhe_rns_ntt_create(fhe_rns_ntt_t **out, uint32_t n, const uint64_t (*moduli)[4], uint32_t num_primes);
/* RNSContext::RNSContext(primes) (include/rns.cuh:27-66, src/rns.cu:6-29): an RNS base WITHOUT a ring.  The handle is an engine of
 * degree n = 1: its buffers [batch][L][1] are exactly RNSContext's interleaved [count][num_primes] layout (src/rns.cu:103-104),
 * `batch` is the reference's `count`, and every container-level entry point (fhe_rns_to_rns, fhe_rns_from_rns, fhe_rns_poly_add /
 * sub, fhe_rns_ntt_pointwise, fhe_rns_mul_mont_literal, fhe_rns_rescale_drop_last, fhe_ct_mod_switch_drop_last, fhe_rns_fast_base_convert, the samplers) works on
 * it.  Primes: pairwise distinct odd primes < 2^255 (no congruence condition). */
int fhe_rns_base_create(fhe_rns_ntt_t **out, const uint64_t (*primes)[4], uint32_t num_primes);
int fhe_rns_ntt_destroy(fhe_rns_ntt_t *h);                                    /* src/ntt.cu:147-156 */
int fhe_rns_ntt_set_stream(fhe_rns_ntt_t *h, void *stream);
int fhe_rns_ntt_width_class(const fhe_rns_ntt_t *h);
/* Pre-sizes the library-owned workspaces for calls of up to `batch` units of every entry point that uses one -- fhe_rns_ntt_forward /
 * inverse (two-pass sizes), fhe_rns_ntt_multiply, fhe_rns_ntt_multiply_bcast, fhe_ct_multiply, fhe_ct_relinearize, fhe_ct_multiply_relin,
 * fhe_rns_automorphism, fhe_ct_apply_galois, fhe_blind_rotate and fhe_blind_rotate_step -- so that later calls never allocate: required before capturing such calls into a hipGraph,
 * optional otherwise (the workspaces grow on first use).  No counterpart in the reference, which mallocs and frees inside every multiply (src/ntt.cu:51-74).
 * The key-switch workspaces depend on the digit count: import the key sets BEFORE reserving.  fhe_rns_ntt_workspace_bytes reports what
 * the engine holds at the moment (device bytes in its three workspaces; tables and key sets are not counted). */
int fhe_rns_ntt_reserve(fhe_rns_ntt_t *h, uint32_t batch);
int fhe_rns_ntt_workspace_bytes(const fhe_rns_ntt_t *h, uint64_t *bytes);
/* forward_rns / inverse_rns (src/ntt.cu:158-171): data [batch][L][n]; one launch for all limbs. */
int fhe_rns_ntt_forward(fhe_rns_ntt_t *h, void *d_data, uint32_t batch);
int fhe_rns_ntt_inverse(fhe_rns_ntt_t *h, void *d_data, uint32_t batch);
int fhe_rns_ntt_pointwise(fhe_rns_ntt_t *h, void *d_r, const void *d_a, const void *d_b, uint32_t batch);
/* multiply_rns (include/ntt.cuh:124-126; declared, never defined in the reference). */
int fhe_rns_ntt_multiply(fhe_rns_ntt_t *h, void *d_r, const void *d_a, const void *d_b, uint32_t batch);
/* The same product with ONE polynomial d_b_one ([L][n]) multiplied into every element of a batch d_a ([batch][L][n]) -- what
 * FHEContext does with a key or a plaintext (pk0 * u, c_i * pt: src/fhe.cu:160-166, include/fhe.cuh:104).  The shared operand is served
 * from L2 after its first use: 2*S bytes of HBM traffic per product instead of 3*S.  d_r may alias d_a, not d_b_one. */
int fhe_rns_ntt_multiply_bcast(fhe_rns_ntt_t *h, void *d_r, const void *d_a, const void *d_b_one, uint32_t batch);
/* PolynomialOps::add / sub over RNS polynomials (src/polynomial.cu:36-52), per-limb moduli. */
int fhe_rns_poly_add(fhe_rns_ntt_t *h, void *d_r, const void *d_a, const void *d_b, uint32_t batch);
int fhe_rns_poly_sub(fhe_rns_ntt_t *h, void *d_r, const void *d_a, const void *d_b, uint32_t batch);
/* rns_mul_kernel / RNSContext::mul_rns (src/rns.cu:84-91, :160-181), LITERAL: r = mul_mod_montgomery(a, b, q_l, inv_l) per limb, i.e. the
 * product carries R^-1 = 2^-256 exactly as in the reference (fhe_rns_ntt_pointwise is the plain product).  Full-width handles only. */
int fhe_rns_mul_mont_literal(fhe_rns_ntt_t *h, void *d_r, const void *d_a, const void *d_b, uint32_t batch);
/* FHEContext::multiply tensor product (src/fhe.cu:199-218), relinearisation excluded (:220 is a stub):
 * c0 = a0*b0, c1 = a0*b1 + a1*b0, c2 = a1*b1.  4 forward + 3 inverse transforms instead of the
 * reference's 8 + 4 (results identical: modular arithmetic is exact). */
int fhe_ct_multiply(fhe_rns_ntt_t *h, void *d_c0, void *d_c1, void *d_c2,
                    const void *d_a0, const void *d_a1, const void *d_b0, const void *d_b1, uint32_t batch);
/* ---- RNS entry / exit ------------------------------------------------------------------------------ */
/* RNS_NTTEngine::to_rns (include/ntt.cuh:114; RNSContext::to_rns src/rns.cu:56-61, kernel :93-115 is a placeholder that
 * copies the value): d_rns[b][l][x] = d_values[b][x] mod q_l for ANY 256-bit value; d_values is [batch][n], d_rns is
 * [batch][L][n] (limb-major like every other buffer of this engine). */
int fhe_rns_to_rns(fhe_rns_ntt_t *h, void *d_rns, const void *d_values, uint32_t batch);
/* RNS_NTTEngine::from_rns (include/ntt.cuh:117; from_rns_crt_kernel src/rns.cu:117-141 writes zero): Chinese remainder
 * reconstruction into [0, Q), Q = prod q_l.  Needs Q < 2^255 (FHE_ERR_UNSUPPORTED otherwise). */
int fhe_rns_from_rns(fhe_rns_ntt_t *h, void *d_values, const void *d_rns, uint32_t batch);

/* RNSContext::mod_switch_rns / rns_mod_switch_kernel (include/rns.cuh:44,128-136), poly_mod_switch_kernel
 * (include/polynomial.cuh:96-103) -- undefined in the reference: drop the last prime with rounding,
 * d_out[b][l][x] = round(C / q_last) mod q_l for l < L-1.  d_in is [batch][L][n], d_out is [batch][L-1][n] (the layout of an
 * engine built on the first L-1 primes).  Needs L >= 2.  The rounding term is arbitrary modulo a plaintext modulus t: this is NOT the
 * modulus switch of a BGV ciphertext (FHEContext::mod_switch_to_next), which is fhe_ct_mod_switch_drop_last below. */
int fhe_rns_rescale_drop_last(fhe_rns_ntt_t *h, void *d_out, const void *d_in, uint32_t batch);

/* FHEContext::mod_switch_to_next / mod_switch_to_level (include/fhe.cuh:109-110, declared only): BGV modulus switch.  Drops the last
 * prime of the basis from up to three ciphertext components in ONE launch, keeping the plaintext modulo t up to the known factor
 * q_last^-1 mod t.  d_in and d_out are HOST arrays of num_components (1..3) device pointers; inputs are [batch][L][n], outputs
 * [batch][L-1][n] (the layout of an engine on the first L-1 primes).  For every component, b and x, with r = in[b][L-1][x]:
 *     u   = (-r * t^-1) mod q_last,   u_c = u if u <= (q_last - 1) / 2, else u - q_last       (q_last is odd: no tie)
 *     out[b][l][x] = (in[b][l][x] + t * u_c) * q_last^-1 mod q_l,  canonical,  l < L-1
 * i.e. C' = (C + t * u_c) / q_last exactly: the added term is 0 modulo t, cancels C modulo q_last and is at most t * q_last / 2 in
 * magnitude.  If (c0, c1) decrypts to m + t*e under s modulo Q, the outputs decrypt modulo Q / q_last to q_last^-1 * (m + t*e) + small,
 * which is q_last^-1 * m modulo t: the caller keeps that factor (Ciphertext::correction in include/fhe/fhe.hpp).
 * FHE_ERR_INVALID_ARG, with nothing launched, unless L >= 2, t >= 2, t != 0 (mod q_last), num_components in 1..3, every pointer is
 * non-null and 16-byte aligned, and the outputs are distinct from each other and from every input.  No condition on Q = prod q_l: no
 * CRT is involved (two 250-bit primes work).  The constant tables depend on t: they are built and uploaded on the first call with a
 * given t and kept, one set per t, until fhe_rns_ntt_destroy.  After that first call a call with the same t allocates nothing and can
 * be captured into a hipGraph. */
int fhe_ct_mod_switch_drop_last(fhe_rns_ntt_t *h, uint64_t t, void *const *d_out, const void *const *d_in, uint32_t num_components,
                                uint32_t batch);

/* ---- public-key encryption as one call -------------------------------------------------------------------------------------------
 * FHEContext::encrypt (src/fhe.cu:138-169; batched by examples/batch_processing.cu): c = (pk0 * u + t e0 + m, pk1 * u + t e1) with u
 * ternary and e0, e1 discrete Gaussians.  For ciphertext b, limb i and coefficient x, with sampler index g = b * n + x:
 *     u  = ternary(seeds[0], g), P(u != 0) = 1/2           exactly what fhe_rns_sample_ternary(h, ., 0.5, seeds[0], batch) writes
 *     e0 = gaussian(sigma, seeds[1], g),  e1 = gaussian(sigma, seeds[2], g)       exactly fhe_rns_sample_gaussian (table of fhe_gaussian_cdt)
 *     out0[b][i] = pk0_i (*) u_b + [t e0_b]_{q_i} + m[b][i],     out1[b][i] = pk1_i (*) u_b + [t e1_b]_{q_i}
 * in Z_{q_i}[x] / (x^n + 1), canonical; a negative small integer -k embeds as q_i - (t k mod q_i) (0 stays 0).  All arithmetic is exact, so
 * the result is bit-identical on every path to fhe_rns_sample_* + fhe_rns_ntt_multiply_bcast + a multiplication by the constant t +
 * fhe_rns_poly_add, and depends only on (pk, t, sigma, seeds, m, b): never on the kernel form or the launch shape.  Because the sampler
 * index is b * n + x, ciphertext b of a batch call differs from a batch-1 call with the same seeds unless b = 0: give every call its own seeds.
 *
 * On the LDS-resident word-sized sizes up to N = 2^14 (and sigma <= 85, so that the cumulative table fits the kernel's staging buffer) a
 * call is ONE launch: a workgroup draws u, e0, e1 in registers, runs one forward transform of u, multiplies by the kept transforms of pk0
 * and pk1 and finishes with two inverse transforms: 3 S bytes of HBM traffic (m in, c0 and c1 out), no workspace.  Elsewhere (full-width
 * class, N >= 2^15, sizes below 2^11, sigma > 85, FHE_HIP_NO_FUSED_ENCRYPT=1) the library runs the composition itself through scratch of
 * its own (u as containers), which fhe_rns_ntt_workspace_bytes counts.
 *
 * fhe_public_key_create: d_pk0, d_pk1 are [L][n] containers in coefficient form, canonical.  They are copied (the sources are not read
 * again; their addresses are remembered only for the aliasing check of fhe_ct_encrypt, so an output placed where a freed source was is
 * rejected), and for the one-launch path transformed once and kept in the order the kernel reads, as key rows are kept.  FHE_ERR_INVALID_ARG with
 * *out untouched: a null or misaligned argument.  fhe_public_key_destroy(NULL) is FHE_OK. */
typedef struct fhe_public_key fhe_public_key_t;
int fhe_public_key_create(fhe_rns_ntt_t *h, fhe_public_key_t **out, const void *d_pk0, const void *d_pk1);
int fhe_public_key_destroy(fhe_public_key_t *pk);
/* Sizes everything a later fhe_ct_encrypt with this sigma and up to `batch` ciphertexts needs: the upload of the cumulative table (one
 * table is kept per engine, shared with fhe_rns_sample_gaussian: a call with another sigma replaces it) and the composed path's scratch.
 * After it fhe_ct_encrypt allocates nothing, fhe_rns_ntt_workspace_bytes does not change across the call, and the call can be captured
 * into a hipGraph (re-capture after the table was replaced). */
int fhe_ct_encrypt_reserve(fhe_rns_ntt_t *h, double sigma, uint32_t batch);
/* (d_out0, d_out1) = the ciphertexts above, [batch][L][n] each; d_m is [batch][L][n] canonical containers (the encoded plaintext in every
 * limb), NULL encrypts zero; seeds = {u, e0, e1}.  FHE_ERR_INVALID_ARG, with nothing launched and nothing written: a null handle, key,
 * seeds or output; a misaligned pointer; outputs aliasing each other, d_m or the key's sources; a key of another engine; batch == 0;
 * t < 2; a sigma that fhe_gaussian_cdt rejects; ceil(12 sigma) >= the smallest modulus. */
int fhe_ct_encrypt(fhe_rns_ntt_t *h, const fhe_public_key_t *pk, uint64_t t, double sigma, const uint64_t seeds[3], void *d_out0, void *d_out1,
                   const void *d_m, uint32_t batch);

/* ---- secret-key decryption as one call ------------------------------------------------------------------------------------------
 * FHEContext::decrypt (src/fhe.cu:171-195) and FHEContext::estimate_noise_budget in one call, the inverse of fhe_ct_encrypt.  d_components
 * is a HOST array of num_components (2 or 3) device pointers to [batch][L][n] canonical containers: c0, c1 and optionally c2 (the convention
 * of fhe_ct_mod_switch_drop_last).  With Q the product of the engine's moduli and, for ciphertext b and coefficient x,
 *     w = (c0 + c1 (*) s + c2 (*) s (*) s)[b][x] mod Q in [0, Q)       (products in Z_Q[x] / (x^n + 1), by CRT over the limbs)
 *     v = w if w <= floor(Q / 2), else w - Q                            the centred representative, in (-Q/2, Q/2]; Q is odd: no tie
 * the outputs are
 *     d_m[b][x]        = ((v mod t) * scale) mod t                      a plain uint64_t in [0, t); d_m is [batch][n]
 *     d_noise_bits[b]  = bit_length(max_x |v[b][x]|)                     0 when every v is 0; d_noise_bits is [batch] and may be NULL
 * where v mod t is the non-negative residue.  scale is what include/fhe/fhe.hpp calls correction^-1 mod t (1: no correction).  The result is an
 * exact function of (components, s, t, scale): every path gives the same bits, whatever the batch, the grid or the kernel form.  Any t with
 * 2 <= t < 2^64 is accepted; the reduction modulo t is division-free (a reciprocal prepared on the host per call, passed as a kernel argument).
 *
 * Q must be below 2^255, the limit of fhe_rns_from_rns, because the noise bits need the integer itself: FHE_ERR_UNSUPPORTED otherwise
 * (from fhe_ct_decrypt_reserve too).
 *
 * On the LDS-resident word-sized sizes, N = 2^11 .. 2^14, a call is TWO launches: one workgroup per (ciphertext, limb) transforms c1 (and c2),
 * multiplies by the kept transforms of s (and s^2), inverts, adds c0 and writes the limb's residues compactly into a library workspace; a
 * second launch, one lane per coefficient, does the CRT, the centring, the reduction modulo t and the per-ciphertext maximum.  2 S (3 S)
 * bytes of containers are read.  Elsewhere (full-width class, N >= 2^15, sizes below 2^11, FHE_HIP_NO_FUSED_DECRYPT=1) the library composes
 * fhe_rns_ntt_multiply_bcast and fhe_rns_poly_add through container scratch of its own and runs the second launch on that.
 * fhe_rns_ntt_workspace_bytes counts the workspace either way.
 *
 * fhe_secret_key_create: d_s is [L][n] canonical containers in coefficient form.  It is copied (its address is remembered only for the aliasing
 * check of fhe_ct_decrypt); s (*) s and, for the two-launch path, the transforms of both are built at import, which is complete when the call
 * returns.  FHE_ERR_INVALID_ARG with *out untouched: a null or misaligned argument.  fhe_secret_key_destroy(NULL) is FHE_OK. */
typedef struct fhe_secret_key fhe_secret_key_t;
int fhe_secret_key_create(fhe_rns_ntt_t *h, fhe_secret_key_t **out, const void *d_s);
int fhe_secret_key_destroy(fhe_secret_key_t *sk);
/* Sizes everything a later fhe_ct_decrypt with up to `num_components` components and up to `batch` ciphertexts needs (CRT tables, the
 * decryption workspace, the composed path's product workspaces).  After it such a call allocates nothing, fhe_rns_ntt_workspace_bytes does
 * not change across it, and it can be captured into a hipGraph (the zeroing of d_noise_bits is part of the capture).  t is checked only:
 * its constants travel with every call. */
int fhe_ct_decrypt_reserve(fhe_rns_ntt_t *h, uint64_t t, uint32_t num_components, uint32_t batch);
/* FHE_ERR_INVALID_ARG, with nothing launched and nothing written: a null handle, key, d_m, d_components or component; num_components outside
 * {2, 3}; a key of another engine; a component or d_m that is not 16-byte aligned (d_noise_bits: 4-byte); d_m or d_noise_bits equal to each
 * other, to a component, or to the key's source; batch == 0; t < 2; scale == 0 or scale >= t. */
int fhe_ct_decrypt(fhe_rns_ntt_t *h, const fhe_secret_key_t *sk, uint64_t t, uint64_t scale, uint64_t *d_m, uint32_t *d_noise_bits,
                   const void *const *d_components, uint32_t num_components, uint32_t batch);

/* Fast base conversion (Bajard et al.) -- RNSContext::base_extend / fast_base_conversion_kernel (include/rns.cuh:47-48,
 * 116-125, undefined in the reference): d_out[b][j][x] = sum_i [x_i (Q/q_i)^-1]_{q_i} (Q/q_i) mod p_j for the primes p_j of
 * `target` (an engine of the same degree).  The value is that of X + alpha*Q, 0 <= alpha < L (inexact by design of the
 * method; the computation itself is deterministic).  d_in: [batch][L][n] in src's basis, d_out: [batch][L'][n] in target's. */
int fhe_rns_fast_base_convert(fhe_rns_ntt_t *src, fhe_rns_ntt_t *target, void *d_out, const void *d_in, uint32_t batch);

/* ---- relinearisation / key switching ------------------------------------------ */
/* RelinKeys (include/fhe.cuh:52-55) as produced by FHEContext::relinkey_gen (src/fhe.cu:76-111):
 * key pairs (b, a) with b = -a*s + e + g*s^2, one per decomposition level.  In the RNS representation every residue
 * polynomial c2 mod q_j is decomposed into K = ceil(bits(q_max) / decomp_bits) base-2^w digit polynomials, so there are
 * L*K levels; level j*K + k carries g = 2^(k*w) in limb j and g = 0 in the other limbs.  For L = 1 this is the
 * reference's decomposition of a single-modulus ciphertext. */
typedef struct fhe_relin_keys fhe_relin_keys_t;
int fhe_relin_num_digits(const fhe_rns_ntt_t *h, uint32_t decomp_bits, uint32_t *digits_per_limb);
/* d_keys_b / d_keys_a: host arrays of num_keys (= L*K) device pointers to [L][n] polynomials in coefficient form.
 * The keys are copied, transformed to the NTT domain once and kept inside the returned object. */
int fhe_relin_keys_create(fhe_rns_ntt_t *h, fhe_relin_keys_t **out, uint32_t decomp_bits,
                          const void *const *d_keys_b, const void *const *d_keys_a, uint32_t num_keys);
int fhe_relin_keys_destroy(fhe_relin_keys_t *rk);
/* FHEContext::relinearize (src/fhe.cu:226-235 is a stub that drops c2; algorithm: docs/ARCHITECTURE.md:319-326):
 * c0 += sum_{j,k} D_{j,k} * b_{j,k},  c1 += sum_{j,k} D_{j,k} * a_{j,k}  with D_{j,k} the digit polynomials of c2.
 * c0, c1 are [batch][L][n] and updated in place; c2 is read only. */
int fhe_ct_relinearize(fhe_rns_ntt_t *h, const fhe_relin_keys_t *rk, void *d_c0, void *d_c1, const void *d_c2, uint32_t batch);
/* FHEContext::multiply as declared (include/fhe.cuh:101-103, src/fhe.cu:199-224): tensor product followed by relinearisation,
 * (c0, c1) = relin(a (x) b), two components out.  Same result as fhe_ct_multiply + fhe_ct_relinearize; c2 stays in an internal
 * workspace (compact form on the word-sized classes), so the call moves about half the bytes of the two-call sequence.
 * Outputs must be distinct and must not alias the inputs. */
int fhe_ct_multiply_relin(fhe_rns_ntt_t *h, const fhe_relin_keys_t *rk, void *d_c0, void *d_c1, const void *d_a0, const void *d_a1,
                          const void *d_b0, const void *d_b1, uint32_t batch);

/* ---- Galois automorphisms / slot rotations ------------------------------------------------------------------------ */
/* The reference declares GaloisKeys (include/fhe.cuh:58-61), FHEContext::galoiskey_gen (:86) and rotate_rows / rotate_columns (:112-116;
 * docs/API_REFERENCE.md:143-144, 220-236) and defines none of them.
 *   Automorphism.  For an odd Galois element g, 1 <= g < 2n, sigma_g maps a(x) to a(x^g) in Z_q[x]/(x^n + 1), coefficient by coefficient
 *     and limb by limb.  Gather form, output index j: i = j * g^-1 mod 2n; out[j] = in[i] if i < n, else (q - in[i - n]) mod q.
 *     sigma_g o sigma_h = sigma_{gh mod 2n}; sigma_1 is the identity.
 *   Galois key for g.  The layout of a relinearisation key with sigma_g(s) in place of s^2: L*K rows, row j*K + k is (b, a) with
 *     b = -a*s + e + g_{j,k} * sigma_g(s).  Imported with fhe_relin_keys_create (no key type of its own); the engine cannot tell which
 *     element a key set was made for, so the caller passes g with the keys.
 *   Applying g to a ciphertext.  (c0, c1) -> (sigma(c0) + sum_{j,k} D_{j,k}(sigma(c1)) b_{j,k}, sum_{j,k} D_{j,k}(sigma(c1)) a_{j,k}): bit for
 *     bit fhe_ct_relinearize applied to (sigma(c0), 0, sigma(c1)).  The result decrypts under s to sigma_g(m).
 *   Slots (slot i holds m(zeta_i), zeta_i = psi^(2i+1), t = 1 mod 2n).  Decrypting sigma_g(ct) gives slot i = v[pi_g(i)] with
 *     2 pi_g(i) + 1 = g (2i + 1) (mod 2n).  rotate_rows(steps) uses g = 3^steps mod 2n (steps taken mod n/2, negative steps the inverse
 *     power); rotate_columns uses g = 2n - 1.  With the slots of row 0 ordered by 2i+1 = 3^k and those of row 1 by 2i+1 = -3^k (mod 2n),
 *     rotate_rows(r) is a cyclic left shift by r of both rows, as in SEAL, and rotate_columns swaps the rows.  The natural slot order of
 *     the encoding is a permutation of this one.
 *   NTT-domain order.  Position x of a forward-transformed limb holds a(psi^(2 bitrev(x) + 1)), bitrev over log2 n bits (fhe_ntt_forward:
 *     "X[k] sits at position bitrev(k)"; in the LDS kernels thread tid, register r holds position tid * 32 + r).  An automorphism is
 *     therefore a pure permutation of the transformed values, with no negation: NTT(sigma_g a)[x] = NTT(a)[pi_g(x)] with
 *         pi_g(x) = bitrev( ((g * (2 * bitrev(x) + 1)) mod 2n - 1) / 2 ).
 *     Every size and width class leaves this order (two-pass sizes and the full-width tile kernels included); hoisted rotations rest on it. */
/* Host only: *elt = 3^(steps mod n/2) mod 2n, the row-rotation element.  n a power of two, 8 <= n <= 2^30. */
int fhe_galois_element(uint32_t n, int32_t steps, uint32_t *elt);
/* d_out[b][l] = sigma_g(d_in[b][l]) on [batch][L][n]; out of place (d_out != d_in).  FHE_ERR_INVALID_ARG for an even g or g >= 2n. */
int fhe_rns_automorphism(fhe_rns_ntt_t *h, void *d_out, const void *d_in, uint32_t galois_elt, uint32_t batch);
/* (d_out0, d_out1) = the ciphertext (d_c0, d_c1) under sigma_g, key-switched back to s with the Galois keys gk of g (see above).  Inputs are
 * read only; outputs distinct from each other and from the inputs; keys imported for another engine are rejected.  On the LDS-resident
 * word-sized sizes with packed keys: two launches (the automorphism of both components into the compact workspace, then the compact-operand
 * key switch of fhe_ct_multiply_relin); elsewhere the automorphism followed by fhe_ct_relinearize. */
int fhe_ct_apply_galois(fhe_rns_ntt_t *h, const fhe_relin_keys_t *gk, uint32_t galois_elt, void *d_out0, void *d_out1, const void *d_c0,
                        const void *d_c1, uint32_t batch);

/* ---- hoisted rotations: decompose a ciphertext once, rotate it many times (Halevi and Shoup) ------------------------------------
 * sigma_g is a ring automorphism, so it can be applied to the digit polynomials instead of to c1.  With D_{j,k}(c1) the base-2^w digit
 * polynomials of c1 mod q_j (the digits fhe_ct_relinearize takes of c2, same level order j*K + k), each embedded in every limb i as a
 * residue of q_i:
 *     out0 = sigma_g(c0) + sum_{j,k} sigma_g(D_{j,k}(c1)) * b_{j,k}
 *     out1 =               sum_{j,k} sigma_g(D_{j,k}(c1)) * a_{j,k}          in Z_{q_i}[x]/(x^n + 1), every limb i
 * sigma_g acts on a digit polynomial as on any element of R_{q_i} (a negated digit d becomes q_i - d).  sum sigma_g(D_{j,k}) g_{j,k} =
 * sigma_g(c1) and sigma_g(D) has the coefficient magnitudes of D, so the result decrypts under s to sigma_g(m) with the noise bound of
 * fhe_ct_apply_galois, from the same Galois keys.  It is NOT bit-identical to fhe_ct_apply_galois for g != 1 (the digits of sigma(c1) are
 * not sigma of the digits of c1); for g = 1 it is.  Equivalently, with sigma_{g^-1} applied to every key row:
 *     hoisted(c0, c1; kb, ka, g) = sigma_g( relinearize(c0, 0, c1; sigma_{g^-1}(kb), sigma_{g^-1}(ka)) ).
 * The result depends only on (c0, c1, keys, g, w): never on how many elements are applied, on the kernel path or on the batch.
 *
 * fhe_ct_hoist decomposes c1 ([batch][L][n], read only) into its L*K digit polynomials for decomp_bits, transforms each under every limb
 * and keeps them in the engine's hoist workspace until the next fhe_ct_hoist or fhe_rns_ntt_destroy.  The hoist workspace is a fourth
 * allocation of its own: no other entry point touches it, and fhe_rns_ntt_reserve / fhe_rns_ntt_workspace_bytes neither size nor count
 * it.  Its size is batch * L*K * L * n * sizeof(residue) bytes (4 or 8) on the LDS-resident word-sized sizes up to N = 2^14 whose key
 * sets get packed tables, and batch * L*K * L * n * 32 bytes elsewhere (full-width class, N >= 2^15, FHE_HIP_NO_FUSED_HOIST=1).  A failed
 * allocation is FHE_ERR_HIP with nothing launched. */
int fhe_ct_hoist(fhe_rns_ntt_t *h, uint32_t decomp_bits, const void *d_c1, uint32_t batch);
/* One rotation from the kept decomposition.  gk: Galois keys of galois_elt, imported with fhe_relin_keys_create.  d_c0 is the c0 that
 * belongs to the hoisted c1 (read only); outputs distinct from each other and from d_c0.  FHE_ERR_INVALID_ARG, with nothing launched, when
 * there is no prior fhe_ct_hoist on this engine, batch or gk's decomp_bits differ from the hoist's, the keys belong to another engine, g is
 * even or >= 2n, or a pointer is null, misaligned or aliased. */
int fhe_ct_apply_galois_hoisted(fhe_rns_ntt_t *h, const fhe_relin_keys_t *gk, uint32_t galois_elt, void *d_out0, void *d_out1,
                                const void *d_c0, uint32_t batch);
/* Pre-sizes the hoist workspace (and what fhe_ct_hoist / fhe_ct_apply_galois_hoisted need of the three other workspaces) for `batch`
 * ciphertexts at decomp_bits, so that neither call allocates afterwards; growing the hoist workspace drops a kept decomposition.
 * fhe_rns_ntt_hoist_bytes reports the hoist workspace's size in bytes (0 until the first hoist or reserve_hoist). */
int fhe_rns_ntt_reserve_hoist(fhe_rns_ntt_t *h, uint32_t decomp_bits, uint32_t batch);
int fhe_rns_ntt_hoist_bytes(const fhe_rns_ntt_t *h, uint64_t *bytes);

/* ---- hoisted linear transform: a sum of plaintext-weighted rotations in one call ("double hoisting") -------------------------------
 * The plaintext matrix-vector product over slots (Halevi and Shoup, diagonal method):  out = sum_t p_t * rotate(ct, step_t), t = 0 .. G-1.
 * Term t has a Galois element g_t (odd, below 2n), the Galois keys of g_t (imported with fhe_relin_keys_create on h for decomp_bits) and a
 * plaintext p_t: ONE [L][n] polynomial in coefficient form, canonical, shared by the whole batch.  gks[t] == NULL is allowed only with
 * galois_elts[t] == 1 and means "no key switch": the term is p_t * (c0, c1).  Elements may repeat.  From the decomposition kept by the last
 * fhe_ct_hoist on h (same decomp_bits, same batch), with D_{j,k}(c1) and the level order of the hoisted rotation above:
 *     out0 = sum_t p_t * ( sigma_{g_t}(c0) + sum_{j,k} sigma_{g_t}(D_{j,k}(c1)) * b_{t,j,k} )
 *     out1 = sum_t p_t * (                   sum_{j,k} sigma_{g_t}(D_{j,k}(c1)) * a_{t,j,k} )      in Z_{q_i}[x]/(x^n + 1), every limb i, canonical
 * and for a keyless term  p_t * c0  and  p_t * c1.  All arithmetic is exact modular arithmetic: the result is bit-identical to
 *     sum_t fhe_rns_ntt_multiply_bcast( fhe_ct_apply_galois_hoisted(gk_t, g_t), p_t )   folded with fhe_rns_poly_add
 * on every path, and depends only on the inputs: never on the batch, the kernel path or the order of the terms.  It decrypts under s to
 * sum_t p_t * sigma_{g_t}(m); in slots, sum_t d_t (.) rot(v, step_t) with the row ordering of the Galois section above when p_t encodes d_t.
 *
 * On the LDS-resident word-sized sizes up to N = 2^14 whose key sets have packed tables a call is two launches whatever G is: c0 (and c1,
 * if a term has no key) forward-transformed once, then one kernel that runs every term's permuted multiply-accumulate, multiplies by the
 * transformed plaintext and adds in the NTT domain: two inverse transforms and two container stores per ciphertext limb in all, instead
 * of 6 G of each for the composition.  Elsewhere (full-width class, N >= 2^15, FHE_HIP_NO_FUSED_HOIST=1) the library runs that composition
 * itself, per term, through a scratch pair of its own.
 *
 * fhe_linear_transform_create copies the plaintexts (and, for the fused path, transforms them once and keeps them in the order the kernel
 * reads, as key rows are kept); the key sets are referenced, not copied, and must outlive the object.  FHE_ERR_INVALID_ARG, with nothing
 * launched and *out untouched: a null argument, plaintext or (with g != 1) key set; num_terms == 0 or above
 * FHE_LINEAR_TRANSFORM_MAX_TERMS; an even element or one >= 2n; keys of another engine or of another decomp_bits; a misaligned plaintext. */
#define FHE_LINEAR_TRANSFORM_MAX_TERMS 4096u
typedef struct fhe_linear_transform fhe_linear_transform_t;
int fhe_linear_transform_create(fhe_rns_ntt_t *h, fhe_linear_transform_t **out, uint32_t decomp_bits, const uint32_t *galois_elts,
                                const fhe_relin_keys_t *const *gks, const void *const *d_plain, uint32_t num_terms);
int fhe_linear_transform_destroy(fhe_linear_transform_t *lt);
/* Sizes whatever fhe_ct_linear_transform_hoisted (and the fhe_ct_hoist before it) needs for `batch` ciphertexts, so that neither allocates
 * afterwards (hipGraph capture).  The call's scratch is a fifth allocation of the engine, counted by fhe_rns_ntt_workspace_bytes; like
 * fhe_rns_ntt_reserve_hoist, growing the hoist workspace drops a kept decomposition, so reserve before hoisting.  On the fused path
 * (where fhe_rns_ntt_hoist_bytes is in residue form and every keyed term has packed tables) a fresh engine then holds
 * batch * L * n * sizeof(residue) bytes for the compact c1 that fhe_ct_hoist reads plus the scratch of once (twice with a keyless term)
 * that size; on the composed path the scratch is 2 * batch * L * n * 32 bytes beside what fhe_ct_apply_galois_hoisted needs. */
int fhe_linear_transform_reserve(fhe_rns_ntt_t *h, const fhe_linear_transform_t *lt, uint32_t batch);
/* (d_out0, d_out1) = the sum above, [batch][L][n] each.  d_c0 is the c0 that belongs to the hoisted c1; d_c1 is required (and must be the
 * hoisted c1) iff lt has a keyless term, else may be NULL.  Inputs are read only.  FHE_ERR_INVALID_ARG, with nothing launched and nothing
 * written: a null handle, object or output; an object created for another engine; no valid fhe_ct_hoist on h, or a batch or decomp_bits
 * that differs from the hoist's; d_c1 missing when a term has no key; a misaligned pointer; outputs aliasing each other or an input. */
int fhe_ct_linear_transform_hoisted(fhe_rns_ntt_t *h, const fhe_linear_transform_t *lt, void *d_out0, void *d_out1,
                                    const void *d_c0, const void *d_c1, uint32_t batch);

/* ---- blind-rotation inner loop ------------------------------------------------------ */
/* FHEContext::blind_rotate is only declared in the reference (include/fhe.cuh:139; pipeline prose README.md:146-159).  Its
 * inner loop is  acc <- acc + ExternalProduct((X^a - 1) * acc, RGSW(s)),  and the external product of an RLWE pair (d0, d1)
 * with an RGSW ciphertext is two key switches accumulated into one pair.  An RGSW ciphertext is therefore imported as two
 * fhe_relin_keys_t objects (rows for component 0 and for component 1, level order j*K + k as for relinearisation keys).
 *
 * d_out[b][l] = (X^shift[b] - 1) * d_in[b][l] over Z_q[x]/(x^n + 1); d_shifts is a DEVICE array of `batch` values in [0, 2n). */
int fhe_rns_monomial_mul_sub(fhe_rns_ntt_t *h, void *d_out, const void *d_in, const uint32_t *d_shifts, uint32_t batch);
/* One blind-rotation step for `batch` independent accumulators: (acc0, acc1) += ExtProd((X^a - 1) * (acc0, acc1), RGSW) with
 * per-accumulator shifts.  d_tmp0 / d_tmp1 are caller-provided scratch polynomials ([batch][L][n] each, distinct from the
 * accumulators).  Same as fhe_blind_rotate with steps = 1. */
int fhe_blind_rotate_step(fhe_rns_ntt_t *h, const fhe_relin_keys_t *rows_c0, const fhe_relin_keys_t *rows_c1, void *d_acc0, void *d_acc1,
                          const uint32_t *d_shifts, void *d_tmp0, void *d_tmp1, uint32_t batch);
/* The loop itself: for s = 0 .. steps-1:  acc <- acc + ExtProd((X^shift[s][b] - 1) * acc, RGSW_s), RGSW_s = (rows_c0[s], rows_c1[s]);
 * d_shifts is a DEVICE array [steps][batch].  On the word-sized width classes every step is ONE kernel launch that reads the
 * accumulator pair and writes the other buffer pair (ping-pong between acc and tmp; the result always ends in d_acc0 / d_acc1),
 * 4 * S bytes of HBM traffic per accumulator and step; the full-width class composes the monomial kernel and two key switches.
 * Nothing is allocated on the word-sized path, so the whole loop can be captured into a hipGraph. */
int fhe_blind_rotate(fhe_rns_ntt_t *h, const fhe_relin_keys_t *const *rows_c0, const fhe_relin_keys_t *const *rows_c1, uint32_t steps,
                     void *d_acc0, void *d_acc1, const uint32_t *d_shifts, void *d_tmp0, void *d_tmp1, uint32_t batch);

/* ---- scheme plumbing around the hot path ------------------------------------------------ */
/* sample_uniform_kernel (src/polynomial.cu:130-143), LITERAL: out[i] = ((seed + i) * 1103515245 + 12345) % q.limbs[0] in 64-bit
 * wrap-around arithmetic ("Simple LCG for demonstration"); called by FHEContext::sample_uniform_polynomial (src/fhe.cu:245-250).
 * count <= 2^32 (the reference's index is a uint32_t); stream may be NULL. */
int fhe_sample_uniform_lcg(void *d_out, const uint64_t q[4], uint64_t seed, size_t count, void *stream);
/* sample_gaussian_kernel (src/polynomial.cu:113-128), LITERAL placeholder: out[i] = (seed + i) % q.limbs[0] (sigma is ignored
 * there); called by FHEContext::sample_error_polynomial (src/fhe.cu:238-243).  Not a Gaussian: see fhe_rns_sample_gaussian. */
int fhe_sample_gaussian_placeholder(void *d_out, const uint64_t q[4], uint64_t seed, size_t count, void *stream);
/* The samplers the reference declares or leaves as placeholders, on the RNS layout [batch][L][n] (a small signed integer is
 * embedded identically in every limb: -m -> q_l - m).  Counter-based generator over (seed, coefficient index): results do not
 * depend on the launch shape and equal the CPU oracle's bit for bit.
 *   ternary : sample_ternary_kernel(result, modulus, probability, seed, n) (include/polynomial.cuh:129-135, declared only; called
 *             with probability 0.5 by src/fhe.cu:252-257): P(coefficient != 0) = probability, sign uniform.
 *   gaussian: discrete Gaussian of parameter sigma over the integers, cut at 12 sigma, by inversion of the cumulative table
 *             fhe_gaussian_cdt builds (what sample_gaussian_kernel's comment asks for, src/polynomial.cu:122-123).
 *   uniform : residues uniform in [0, q_l) per limb, rejection sampling (no modulo bias), any modulus width. */
int fhe_rns_sample_ternary(fhe_rns_ntt_t *h, void *d_out, double probability, uint64_t seed, uint32_t batch);
int fhe_rns_sample_gaussian(fhe_rns_ntt_t *h, void *d_out, double sigma, uint64_t seed, uint32_t batch);
int fhe_rns_sample_uniform(fhe_rns_ntt_t *h, void *d_out, uint64_t seed, uint32_t batch);
/* Host helper: table[k] = floor(2^64 * P(|X| <= k)), k = 0 .. len-1, len = ceil(12 sigma); table == NULL queries len. */
int fhe_gaussian_cdt(double sigma, uint64_t *table, uint32_t capacity, uint32_t *len);
/* poly_mod_switch_kernel(result, a, old_modulus, new_modulus, n) (include/polynomial.cuh:96-103, declared; launched by
 * FHEContext::decrypt, src/fhe.cu:181-184: "scale down by delta and reduce mod t"):
 * r[i] = round(a[i] * new_q / old_q) mod new_q (round half up) on single-modulus containers; a < old_q < 2^255, new_q < 2^64. */
int fhe_poly_mod_switch(void *d_r, const void *d_a, const uint64_t old_q[4], const uint64_t new_q[4], size_t count, void *stream);
/* negacyclic_reduce_kernel(data, modulus, n) (include/polynomial.cuh:105-110, declared): fold 2n coefficients modulo x^n + 1,
 * data[i] = sub_mod(data[i], data[i + n]) for i < n (the upper half is left unchanged). */
int fhe_negacyclic_reduce(void *d_data, const uint64_t q[4], size_t n, void *stream);

/* ---- key-switching key generation as one call; key export ---------------------------------------------------------------------------
 * FHEContext::relinkey_gen (src/fhe.cu:76-111) and galoiskey_gen (include/fhe.cuh:86) on the device: num_sets key sets from one call.
 * galois_elts[e] == 0 asks for a relinearisation key (target s (*) s, what fhe_secret_key_create keeps); an odd g in [1, 2n) for the Galois
 * key of g (target sigma_g(s), what fhe_rns_automorphism gives).  With K = fhe_relin_num_digits, row r = j K + k of set e, polynomial index
 * P = e L K + r, limb l, position x:
 *     U_P[l][x]  the uniform residue that fhe_rns_sample_uniform(h, ., seeds[0], num_sets L K) writes at element (P L + l) n + x, taken AS THE
 *                NTT-DOMAIN VALUE of a: a^_P = U_P, a_P = fhe_rns_ntt_inverse(U_P)  (a uniform polynomial is uniform in either domain; one
 *                forward transform per limb polynomial is saved)
 *     e_P[x]     what fhe_rns_sample_gaussian(h, ., sigma, seeds[1], num_sets L K) writes at element P n + x, the same small integer in every limb
 *     b_P[l]     = -a_P[l] (*) s[l] + [noise_scale e_P]_{q_l} + (l == j ? (2^(k w) mod q_j) target[j] : 0), canonical
 * out_sets[e] is the handle fhe_relin_keys_create would return for the rows (b_P, a_P) of set e: the same bits in the same tables (packed
 * tables where the import packs, NTT-domain containers otherwise), accepted unchanged by every consumer.  All arithmetic is exact: the result
 * is a function of (s, decomp_bits, elements, noise_scale, sigma, seeds) only, never of the path or the launch shape.  The same element may
 * appear more than once (different rows of the streams: different keys for the same target).
 *
 * On the LDS-resident word-sized sizes, N = 2^11 .. 2^14, with key sets that get packed tables, a secret key that has its packed transforms
 * and sigma <= 85, the call is ONE launch, one workgroup per (set, row, limb), which draws e and U in registers and writes both packed rows;
 * Galois targets are gathered in the kernel from the transform of s.  Elsewhere (full-width class, N >= 2^15, sizes below 2^11, unpacked
 * key sets, sigma > 85, FHE_HIP_NO_FUSED_KEYGEN=1) the library composes the samplers, the transforms and element-wise kernels, one key set
 * at a time, through scratch of (L K + 2) S bytes that it frees before it returns.  The keys are complete when the call returns.
 *
 * FHE_ERR_INVALID_ARG with nothing launched, nothing allocated and every out_sets[i] untouched: a null argument; a key of another engine;
 * num_sets == 0; an even element or one not below 2n; decomp_bits outside [1, 64]; noise_scale == 0; a sigma fhe_gaussian_cdt rejects;
 * ceil(12 sigma) not below the smallest modulus.  On a failure after that every handle made so far is destroyed and every out_sets[i] is NULL. */
int fhe_keyswitch_keys_generate(fhe_rns_ntt_t *h, const fhe_secret_key_t *sk, uint32_t decomp_bits, const uint32_t *galois_elts, uint32_t num_sets,
                                uint64_t noise_scale, double sigma, const uint64_t seeds[2], fhe_relin_keys_t **out_sets);
/* The inverse of fhe_relin_keys_create for ANY key set of h, however it was made: d_keys_b / d_keys_a receive its rows as
 * [num_keys][L][n] canonical containers in coefficient form (num_keys = L K; packed sets are unpacked first).  Outputs must be distinct. */
int fhe_relin_keys_export(fhe_rns_ntt_t *h, const fhe_relin_keys_t *rk, void *d_keys_b, void *d_keys_a);

/* ---- programmable bootstrapping around the blind-rotation loop -----------------------------------------------------------------------
 * FHEContext::bootstrap / blind_rotate / extract_lsb (include/fhe.cuh:119, 138-140, declared only; pipeline prose README.md:146-159): an LWE
 * ciphertext in, fhe_blind_rotate over RGSW encryptions of the LWE secret's bits, one coefficient of the accumulator out as an LWE sample of
 * f(m) under the ring key.  For moduli below 2^64 only: the word-sized width classes, and the sizes n < 2^11 that have no word-sized kernels (such
 * an engine reports FHE_WIDTH_256 for its size; the streaming kernels and the composed key generation serve it).  An engine with a modulus of
 * 2^64 or more gets FHE_ERR_UNSUPPORTED from all three calls, nothing launched.
 *
 * Phase.  Everything uses the library's phase c0 + c1 s.  An LWE ciphertext is n_lwe + 1 values (a_0 .. a_{n_lwe-1}, b), phase b + sum a_i z_i.
 * Input LWE.  d_lwe is [batch][n_lwe + 1] uint64_t, every value below q_lwe, 2 <= q_lwe <= 2^48 (so v 2n + q_lwe/2 < 2^64).  The switch to
 *   modulus 2n is ms(v) = floor((v 2n + floor(q_lwe / 2)) / q_lwe) mod 2n; b~ = ms(b), a~_i = ms(a_i).  A value >= q_lwe is the CALLER'S error,
 *   as a non-canonical coefficient is everywhere else: the result is then unspecified (nothing is read or written out of bounds).
 * Accumulator.  d_tv is ONE [L][n] canonical container polynomial shared by the batch, the test vector.  acc0[b] = X^(2n - b~_b) tv, negacyclic
 *   and canonical: coefficient x comes from index i = (x + b~) mod 2n and is tv[i] if i < n, else (q - tv[i - n]) mod q.  acc1[b] = 0.
 *   shifts[i][b] = (2n - a~_i) mod 2n, laid out [n_lwe][batch] as fhe_blind_rotate reads it.
 * Result of the loop.  After fhe_blind_rotate with RGSW encryptions of z_i in {0, 1} the accumulator has phase X^(-phi~) tv + noise,
 *   phi~ = (b~ + sum a~_i z_i) mod 2n: its constant coefficient is tv[phi~] for phi~ < n and -tv[phi~ - n] otherwise.
 * Extraction at idx < n.  The output is [batch][L][n + 1] uint64_t residues, limb l modulo q_l: out[n] = c0[idx]; out[j] = c1[idx - j] for
 *   j <= idx; out[j] = (q_l - c1[n + idx - j]) mod q_l for j > idx.  Hence out[n] + sum out[j] s_j = (c0 + c1 s)[idx] in every limb.
 * RGSW rows.  The layout of fhe_blind_rotate's rows, with K, U_P, e_P and the "uniform taken as the NTT-domain value of a" convention of
 *   fhe_keyswitch_keys_generate: message mu_i, component c in {0, 1}, polynomial index P = (2 i + c) L K + r, row r = j K + k,
 *       b_P[l] = -a_P[l] (*) s[l] + [noise_scale e_P]_{q_l} + (l == j ? (2^(k w) mod q_j) T : 0),   T = mu_i (the constant polynomial) for c = 0,
 *   T = mu_i s for c = 1 -- with a' = a + g mu this is exactly RLWE(0) + (0, g mu).  mu_i is a host int32_t, |mu_i| <= 2^15; a negative value
 *   embeds as q - |mu|.
 *
 * fhe_rgsw_keys_generate: `num` RGSW ciphertexts, each two handles (out_rows_c0[i], out_rows_c1[i]) that are bit for bit what
 * fhe_relin_keys_create returns for the rows above: fhe_blind_rotate, fhe_relin_keys_export and fhe_relin_keys_destroy take them unchanged.
 * Where fhe_keyswitch_keys_generate is one launch (N = 2^11 .. 2^14, packed key sets, a secret key with packed transforms, sigma <= 85) this
 * call is ONE launch too (for c = 0 the gadget term is a constant at every NTT position, for c = 1 it is mu 2^(k w) s^[y] read from the packed
 * transform of s); everywhere else and under FHE_HIP_NO_FUSED_KEYGEN=1 it composes the samplers, transforms and element-wise kernels like
 * fhe_keyswitch_keys_generate, through scratch of (L K + 2) S bytes freed before it returns.  Same bits on either path.
 * FHE_ERR_INVALID_ARG with nothing launched, nothing allocated and the outputs untouched: a null argument; out_rows_c0 == out_rows_c1; a key
 * of another engine; num == 0; decomp_bits outside [1, 64]; |mu_i| > 2^15; noise_scale == 0; a sigma fhe_gaussian_cdt rejects; ceil(12 sigma)
 * not below the smallest modulus.  On a failure after that every handle made so far is destroyed and every output is NULL. */
int fhe_rgsw_keys_generate(fhe_rns_ntt_t *h, const fhe_secret_key_t *sk, uint32_t decomp_bits, const int32_t *mu, uint32_t num,
                           uint64_t noise_scale, double sigma, const uint64_t seeds[2], fhe_relin_keys_t **out_rows_c0, fhe_relin_keys_t **out_rows_c1);
/* The loop's inputs from `batch` LWE ciphertexts: d_acc0, d_acc1 ([batch][L][n] containers each) and d_shifts ([n_lwe][batch] uint32_t) as
 * above.  ONE launch for any n >= 8, no workspace, nothing allocated (capturable into a hipGraph); tv is read through L2.  FHE_ERR_INVALID_ARG
 * with nothing launched: a null pointer; d_tv / d_acc0 / d_acc1 not 16-byte, d_lwe not 8-byte or d_shifts not 4-byte aligned; outputs that
 * overlap each other or an input; batch == 0; n_lwe == 0; q_lwe outside [2, 2^48]. */
int fhe_lwe_prepare_accumulator(fhe_rns_ntt_t *h, uint64_t q_lwe, uint32_t n_lwe, const uint64_t *d_lwe, const void *d_tv, void *d_acc0, void *d_acc1,
                                uint32_t *d_shifts, uint32_t batch);
/* Coefficient idx of `batch` RLWE pairs (d_c0, d_c1: [batch][L][n] containers) as LWE samples, d_out = [batch][L][n + 1] uint64_t as above.
 * ONE launch for any n >= 8, no workspace.  FHE_ERR_INVALID_ARG with nothing launched: a null pointer; misaligned d_c0 / d_c1 (16 bytes) or
 * d_out (8 bytes); an output that overlaps an input; batch == 0; idx >= n. */
int fhe_rlwe_sample_extract(fhe_rns_ntt_t *h, uint64_t *d_out, const void *d_c0, const void *d_c1, uint32_t idx, uint32_t batch);
/* The `count` evenly spaced coefficients i n / count, i < count, of `batch` RLWE pairs at once: the way INTO the LWE side of
 * FHEContext::bootstrap(Ciphertext&).  d_c0, d_c1: [batch][L][n] containers; d_out: [batch][count][L][n + 1] uint64_t, row (b, i, l) exactly what
 * fhe_rlwe_sample_extract(h, ., d_c0, d_c1, idx = i n / count, .) writes for polynomial (b, l): bit-identical to `count` single calls scattered
 * into that layout, which is the d_lwe of fhe_lwe_pack and, on a one-limb engine, the [batch count][n + 1] d_in of fhe_lwe_keyswitch.
 * count is a power of two, 1 <= count <= n.  ONE launch for any n >= 8, no workspace, nothing allocated: capturable.  Row i is row 0 rotated
 * by i n / count, so every coefficient of c1 is loaded once and stored `count` times (from HBM once per ciphertext, not once per row).
 * FHE_ERR_INVALID_ARG with nothing launched: a null pointer; misaligned d_c0 / d_c1 (16 bytes) or d_out (8 bytes); an output that overlaps an
 * input; batch == 0; n < 8; a count that is zero, not a power of two, or above n; batch count overflowing uint32_t or batch count L above
 * 2^31 - 1 (the range of fhe_lwe_pack). */
int fhe_rlwe_sample_extract_strided(fhe_rns_ntt_t *h, uint64_t *d_out, const void *d_c0, const void *d_c1, uint32_t count, uint32_t batch);

/* ---- LWE key switch back to the small key: chainable bootstrapping -------------------------------------------------------------------
 * The last step of FHEContext::bootstrap (include/fhe.cuh:119, declared only; README.md:146-159): the sample that fhe_rlwe_sample_extract
 * leaves is under the RING key s (dimension n, modulus q); the next fhe_lwe_prepare_accumulator wants dimension n_lwe, the small key z and one
 * modulus of at most 2^48.  This block switches the key, and optionally the modulus, in one launch.  Phase b + sum a_i z_i as above.  For
 * moduli below 2^64: an engine with a wider modulus gets FHE_ERR_UNSUPPORTED from every call that takes one, nothing launched.
 *
 * Definitions.  q = the modulus of LIMB 0 of the engine (the level-0 engine and the one-limb level engine on the same first prime both do);
 *   n_in = h->n; w = decomp_bits in [1, 32]; K = ceil(bit_length(q) / w) (fhe_lwe_ksk_num_digits); R = n_in K.  Row r = j K + k (j < n_in,
 *   k < K) encrypts s_j 2^(k w) under z, an array of n_out small integers.
 * Key object.  Canonical form: a row-major table [R][n_out + 1] of uint64_t below q, row r = (a_{r,0} .. a_{r,n_out-1}, b_r).  Inside the
 *   object a row is padded with zeros to a multiple of 64 columns, so that one wave instruction of the apply kernel reads 512 consecutive
 *   bytes of a row (fhe_lwe_ksk_bytes reports the padded size).  A key is bound to (n_in, q, device), not to one engine handle.
 *
 * fhe_lwe_ksk_create imports the canonical table from a device pointer, 8-byte aligned, and copies it (complete when the call returns);
 *   values >= q are the caller's error, as non-canonical coefficients are everywhere else.  fhe_lwe_ksk_export is its inverse for a key
 *   however it was made (enqueued on h's stream).  fhe_lwe_ksk_destroy(NULL) is FHE_OK.  FHE_ERR_INVALID_ARG with *out untouched: a null
 *   argument, a misaligned pointer, decomp_bits outside [1, 32], n_out == 0 or n_out > 65536, (export) an engine that does not match the key.
 *
 * fhe_lwe_ksk_generate.  z is a HOST array of n_out int32_t, |z_i| <= 2^15; a negative value embeds as q - |z_i|.  s_j is coefficient j of
 *   limb 0 of the secret key as imported, taken as a residue (nothing assumes it is small).  With the stream conventions of
 *   fhe_keyswitch_keys_generate:
 *       a_{r,i}  the uniform residue below q of element r n_out + i of stream seeds[0], drawn as fhe_rns_sample_uniform draws a one-word
 *                modulus: word DRAW_UNIFORM + 4 t of the element, masked to bit_length(q), rejected until below q, top bit cleared after 64
 *                rejections
 *       e_r      the discrete Gaussian of element r of stream seeds[1] from the table of fhe_gaussian_cdt(sigma)
 *       b_r      = (s_j (2^(k w) mod q) + [noise_scale e_r]_q - sum_i a_{r,i} z_i) mod q
 *   The result is the handle fhe_lwe_ksk_create would return for that table, bit for bit: a function of (s, z, w, n_out, noise_scale, sigma,
 *   seeds) only.  ONE launch after z is uploaded: one workgroup per row draws the row in registers, forms the inner product with z and writes
 *   the row in the internal layout.  The key is complete when the call returns.  FHE_ERR_INVALID_ARG, with nothing launched or allocated and
 *   *out untouched: a null argument; a key of another engine; n_out == 0 or n_out > 65536; decomp_bits outside [1, 32]; |z_i| > 2^15;
 *   noise_scale == 0; a sigma fhe_gaussian_cdt rejects; ceil(12 sigma) >= q.  The noise comes from the engine's one cumulative table (shared with
 *   fhe_rns_sample_gaussian, uploaded when sigma changes), which is kept for every limb: on an engine of several primes ceil(12 sigma) must
 *   also be below the smallest of them.
 *
 * fhe_lwe_keyswitch.  d_in is [batch][n_in + 1] uint64_t below q (what fhe_rlwe_sample_extract writes on a one-limb engine), d_out is
 *   [batch][n_out + 1].  With d_{j,k} = (in[b][j] >> (k w)) & (2^w - 1):
 *       acc_i = sum_{j,k} d_{j,k} ksk[j K + k][i] mod q  for i <= n_out;     acc_{n_out} = (acc_{n_out} + in[b][n_in]) mod q
 *   q_out == 0: out[b][i] = acc_i.  Otherwise 2 <= q_out <= 2^48 and out[b][i] = floor((acc_i q_out + floor(q / 2)) / q) mod q_out, the modulus
 *   switch of the sample fused as the epilogue (needed when q > 2^48; q_out need not be prime).  The output phase under z equals the input
 *   phase under s plus noise_scale sum d_{j,k} e_{j K + k}.  All arithmetic is exact: the same bits whatever the batch, the grid or the
 *   accumulator form (a 64-bit accumulator where bit_length(q) + w + ceil(log2 R) <= 64, a 128-bit one elsewhere; chosen at key creation,
 *   FHE_HIP_LWE_KSK_WIDE=1 read there forces the second).  Accepted engines: any h with h->n == n_in, limb-0 modulus q and the key's device;
 *   the work runs on h's stream.  ONE launch, no workspace, nothing allocated: capturable into a hipGraph.  FHE_ERR_INVALID_ARG, with nothing
 *   launched and nothing written: a null argument; a pointer not 8-byte aligned; an output overlapping the input; batch == 0; q_out outside
 *   {0} u [2, 2^48]; an engine that does not match the key. */
typedef struct fhe_lwe_ksk fhe_lwe_ksk_t;
int fhe_lwe_ksk_num_digits(const fhe_rns_ntt_t *h, uint32_t decomp_bits, uint32_t *digits);   /* K for h's limb-0 modulus */
int fhe_lwe_ksk_create(fhe_rns_ntt_t *h, fhe_lwe_ksk_t **out, uint32_t decomp_bits, uint32_t n_out, const uint64_t *d_rows);
int fhe_lwe_ksk_export(fhe_rns_ntt_t *h, const fhe_lwe_ksk_t *ksk, uint64_t *d_rows);
int fhe_lwe_ksk_destroy(fhe_lwe_ksk_t *ksk);
int fhe_lwe_ksk_bytes(const fhe_lwe_ksk_t *ksk, uint64_t *bytes);                              /* device bytes of the key table */
int fhe_lwe_ksk_generate(fhe_rns_ntt_t *h, const fhe_secret_key_t *sk, uint32_t decomp_bits, uint32_t n_out, const int32_t *z,
                         uint64_t noise_scale, double sigma, const uint64_t seeds[2], fhe_lwe_ksk_t **out);
int fhe_lwe_keyswitch(fhe_rns_ntt_t *h, const fhe_lwe_ksk_t *ksk, uint64_t q_out, uint64_t *d_out, const uint64_t *d_in, uint32_t batch);

/* ---- pack LWE samples into one RLWE ciphertext: the way back from bootstrapping -------------------------------------------------------
 * The last step of FHEContext::bootstrap(Ciphertext&) (include/fhe.cuh:119, declared only; README.md:146-159): the refreshed coefficients are LWE
 * samples under the RING key, and the ring operations want one RLWE ciphertext.  The ring packing of Chen, Dai, Kim and Song ("Efficient
 * homomorphic conversion between (ring) LWE ciphertexts": PackLWEs and the field trace): log2(n) automorphism key switches and streaming merges.
 * Phase c0 + c1 s.  For moduli below 2^64, the rule of the bootstrapping block: an engine with a modulus of 2^64 or more gets
 * FHE_ERR_UNSUPPORTED from every call that takes one, nothing launched.  Any n >= 8 the engine accepts.
 *
 * Embedding.  An LWE sample under the ring key is [L][n + 1] uint64_t, limb l holding (a_0 .. a_{n-1}, b) below q_l: what fhe_rlwe_sample_extract
 *   writes.  Its RLWE embedding is the inverse of extraction at idx = 0: c0 = (b, 0, .., 0), c1[0] = a_0, c1[i] = (q_l - a_{n-i}) mod q_l for i >= 1.
 *   Coefficient 0 of c0 + c1 s is b + sum a_j s_j; the other coefficients are unspecified.
 * Merge.  For a list of c = 2^l RLWE ciphertexts, c >= 2, m = n / c:  E = Pack(entries 0, 2, 4, ..), O = Pack(entries 1, 3, 5, ..),
 *   P = E + X^m O, D = E - X^m O (negacyclic, per component, per limb, canonical), Pack = P + fhe_ct_apply_galois(D, g = c + 1).  Pack of one
 *   entry is the entry.  Unrolled by level l = 1 .. log2(count): the count / 2^(l-1) results R of the level before merge in pairs,
 *   R_l[r] = merge(R_(l-1)[r], R_(l-1)[r + count / 2^l]) with m = n / 2^l and g = 2^l + 1, all batch count / 2^l pairs in one step.
 * Trace.  With k = log2(count): for j = k+1, k+2, .., log2(n) in this order, ct <- ct + fhe_ct_apply_galois(ct, g = 2^j + 1).
 * Normalisation.  F = n with the trace, F = count without.  With normalize != 0 every embedded value is multiplied by F^-1 mod q_l before the
 *   first merge: exact, F is a power of two and q_l is odd (log2 F halvings in the kernel, no table).
 * Result.  Coefficient i (n / count) of the output has phase F phi_i without normalisation, phi_i exactly with it, plus key-switch noise, phi_i the
 *   phase of sample i.  With the trace every other coefficient has phase 0 plus noise; without it the others are unspecified.
 * All arithmetic is exact and fhe_ct_apply_galois is deterministic: the output is a function of (samples, keys, count, trace, normalize) only, and
 * every path gives the bits of the composition above written out with fhe_lwe_to_rlwe, fhe_rns_monomial_mul_sub, fhe_rns_poly_add / sub and
 * fhe_ct_apply_galois.  Values >= q_l are the caller's error, as everywhere else.
 *
 * Per level the library runs ONE streaming launch and one batched fhe_ct_apply_galois.  The first level reads the pair of samples as 8-byte
 * words and writes P and D of both components (the batch count embedded ciphertexts, 4 x the bytes of the samples, are never written); a later
 * level reads (P_E, G_E, P_O, G_O), G the key-switched D of the level before, forms E = P_E + G_E and O = P_O + G_O in registers and writes the next
 * P and D; the last sum and the sums of the trace go straight into the outputs.  FHE_HIP_NO_FUSED_PACK=1, read per call, runs the literal
 * composition through container scratch instead (same bits).  Work goes on h's stream.
 * Workspace.  The call's scratch is an allocation of the engine's own, which fhe_rns_ntt_workspace_bytes counts.  With S = L n 32 bytes:
 *     3 batch count S                      count >= 2  (three regions, each both components of batch count / 2 ciphertexts)
 *     2 batch S                            count == 1 with the trace;  nothing for count == 1 without
 *     5 batch count S + 2 batch count      count >= 2 under FHE_HIP_NO_FUSED_PACK=1; under that switch every shape also holds, from the next
 *                                          16-byte boundary, batch count L (n + 1) 8 bytes of sample scratch for fhe_rlwe_pack
 *   beside what fhe_ct_apply_galois needs at the largest level batch, batch count / 2 (batch for count == 1).  fhe_lwe_pack_reserve sizes both (for
 *   the path the environment selects when it is called); after it a call allocates nothing and can be captured into a hipGraph. */
/* host only: elts[j-1] = 2^j + 1, j = 1 .. log2 n.  n a power of two, 8 <= n <= 2^30. */
int fhe_lwe_pack_galois_elements(uint32_t n, uint32_t *elts);
/* the embedding above for `batch` samples: d_lwe [batch][L][n+1] uint64_t -> d_c0, d_c1 [batch][L][n] containers.  fhe_rlwe_sample_extract(idx = 0)
 * of the result gives d_lwe back bit for bit.  ONE launch, no workspace. */
int fhe_lwe_to_rlwe(fhe_rns_ntt_t *h, void *d_c0, void *d_c1, const uint64_t *d_lwe, uint32_t batch);
/* d_lwe [batch][count][L][n+1] -> (d_out0, d_out1) [batch][L][n].  gks: HOST array of log2(n) key-set handles, gks[j-1] the Galois keys of 2^j + 1
 * (from fhe_keyswitch_keys_generate or fhe_relin_keys_create on h, one decomp_bits for all); an entry the call does not use (j > log2(count)
 * without the trace) may be NULL.  fhe_lwe_pack and fhe_lwe_to_rlwe return FHE_ERR_INVALID_ARG, with nothing launched and nothing written: a null
 * handle, output, input or needed key set; keys of another engine, or key sets of differing decomp_bits; a count that is zero, not a power of
 * two, or above n; batch == 0, or batch count overflowing uint32_t (or batch count L above 2^31 - 1); a container pointer not 16-byte aligned, or
 * d_lwe not 8-byte aligned; outputs overlapping each other or the input. */
int fhe_lwe_pack(fhe_rns_ntt_t *h, const fhe_relin_keys_t *const *gks, void *d_out0, void *d_out1, const uint64_t *d_lwe, uint32_t count, int trace,
                 int normalize, uint32_t batch);
int fhe_lwe_pack_reserve(fhe_rns_ntt_t *h, const fhe_relin_keys_t *const *gks, uint32_t count, int trace, uint32_t batch);
/* The same packing straight from RLWE pairs: the way OUT of the LWE side of FHEContext::bootstrap(Ciphertext&).  d_c0, d_c1: [batch][count][L][n]
 * containers, batch count accumulators in the order fhe_blind_rotate leaves them, whose coefficient 0 carries the refreshed value.  The
 * result is fhe_lwe_pack applied to fhe_rlwe_sample_extract(idx = 0) of every input pair, the same bits on every path.  Extraction at 0
 * followed by the embedding is the identity on c1 and keeps c0[0] alone, so the first merge level (for count == 1 the embedding) reads c1 and
 * container 0 of c0 in place: the batch count L (n + 1) 8 bytes of samples are neither written nor read back, and their buffer never
 * exists.  Nothing else of c0 is read.  Every later level, the trace, the normalisation and the scratch are fhe_lwe_pack's: the SAME
 * fhe_lwe_pack_reserve(h, gks, count, trace, batch) serves both entries, after which a call allocates nothing and can be captured.
 * FHE_HIP_NO_FUSED_PACK=1, read per call, runs fhe_rlwe_sample_extract(idx = 0) into the sample scratch of the table above and then the
 * composed path of fhe_lwe_pack.  FHE_ERR_INVALID_ARG as fhe_lwe_pack (every container pointer 16-byte aligned), and for an output that
 * overlaps an input. */
int fhe_rlwe_pack(fhe_rns_ntt_t *h, const fhe_relin_keys_t *const *gks, void *d_out0, void *d_out1, const void *d_c0, const void *d_c1, uint32_t count,
                  int trace, int normalize, uint32_t batch);

/* ---- batch encoder: slot values <-> plaintext polynomials on the device --------------------------------------------------------------
 * FHEContext::encode / decode and BatchEncoder (include/fhe.cuh:89-90, 150-157).  With psi = fhe_find_psi(n, t) and e(i) the exponent of slot i:
 *   FHE_SLOTS_NATURAL  e(i) = 2 i + 1                                          (what the mirror's host encode / decode evaluate)
 *   FHE_SLOTS_ROWS     e(k) = 3^k mod 2n, e(n/2 + k) = 2n - e(k), k < n/2      (the order of the Galois section above: rotate_rows(r) is a
 *                      cyclic left shift by r of both halves, rotate_columns swaps the halves)
 * encode       d_values is [batch][n] uint64_t, each below t (canonical, like every data input).  m_b is the polynomial of degree < n over Z_t
 *              with m_b(psi^e(i)) = values[b][i]; d_out[b][l][x] = m_b[x] mod q_l as canonical containers, [batch][L][n]: the d_m of
 *              fhe_ct_encrypt, and one [L][n] slice is a plaintext of fhe_linear_transform_create.  Where t <= q_l the residue is m itself,
 *              where t > q_l it is reduced (division-free, one table entry per limb prepared at creation).
 * decode       d_m is [batch][n] uint64_t below t, what fhe_ct_decrypt writes; values[b][i] = m_b(psi^e(i)) mod t.  d_values == d_m is allowed.
 * decode_poly  the same from [batch][L][n] containers, reading limb 0; FHE_ERR_UNSUPPORTED when t > q_0 (the residue is then not m).
 * All arithmetic is exact: the result is a function of (t, n, order, inputs) only, never of the path, the batch or h's width class.
 *
 * fhe_batch_encoder_create builds and owns a one-limb engine on (n, t), so t must be a prime = 1 (mod 2n): FHE_ERR_BAD_MODULUS with *out
 * untouched otherwise; an order outside the enum is FHE_ERR_INVALID_ARG.  It uploads one n-entry table, position of the NTT domain -> slot
 * (fhe_batch_encoder_slot_table builds the same table on the host, no device needed), and the per-limb reductions.  For N = 2^11 .. 2^14 a
 * call is ONE launch on the kernels of t's field (t = 65537 runs the 4-byte field whatever h's primes are; a full-width h too) and allocates
 * nothing.  Elsewhere (and under FHE_HIP_NO_FUSED_ENCODE=1, read at creation) the library composes a gather, a transform of the owned engine and a
 * streaming kernel through scratch of batch n 32 bytes that the ENCODER owns: fhe_batch_encoder_reserve sizes it, after which no call
 * allocates and a call can be captured into a hipGraph; fhe_batch_encoder_scratch_bytes reports it.  Work is enqueued on h's stream.
 * FHE_ERR_INVALID_ARG, with nothing launched and nothing written: a null handle, encoder or buffer; an encoder of another engine; batch == 0;
 * a container pointer not 16-byte aligned or a uint64_t pointer not 8-byte aligned; an encode output overlapping its input (a decode output
 * may be d_m itself, not overlap it otherwise).  fhe_batch_encoder_destroy(NULL) is FHE_OK.  None of these returns FHE_ERR_NO_DEVICE: every
 * one needs an engine, which cannot exist without a device (fhe_rns_ntt_create reports that); fhe_batch_encoder_slot_table needs neither.
 * The `const` of the encoder argument says that a call changes nothing a caller can observe, NOT that calls may run concurrently: like the
 * workspaces of an engine, the scratch and the owned engine belong to one call at a time, so all calls on one encoder must be ordered on
 * one stream, and a composed-path call that has to grow the scratch (no reserve before it) synchronises that stream first. */
typedef enum fhe_slot_order { FHE_SLOTS_NATURAL = 0, FHE_SLOTS_ROWS = 1 } fhe_slot_order;
typedef struct fhe_batch_encoder fhe_batch_encoder_t;
int fhe_batch_encoder_create(fhe_rns_ntt_t *h, fhe_batch_encoder_t **out, uint64_t t, int slot_order);
int fhe_batch_encoder_destroy(fhe_batch_encoder_t *enc);
int fhe_batch_encoder_reserve(fhe_rns_ntt_t *h, fhe_batch_encoder_t *enc, uint32_t batch);
int fhe_batch_encoder_scratch_bytes(const fhe_batch_encoder_t *enc, uint64_t *bytes);
int fhe_batch_encoder_slot_table(uint32_t n, int slot_order, uint32_t *table);   /* host: table[n], position -> slot index */
int fhe_slots_encode(fhe_rns_ntt_t *h, const fhe_batch_encoder_t *enc, void *d_out, const uint64_t *d_values, uint32_t batch);
int fhe_slots_decode(fhe_rns_ntt_t *h, const fhe_batch_encoder_t *enc, uint64_t *d_values, const uint64_t *d_m, uint32_t batch);
int fhe_slots_decode_poly(fhe_rns_ntt_t *h, const fhe_batch_encoder_t *enc, uint64_t *d_values, const void *d_poly, uint32_t batch);

/* ---- CKKS encoder: complex slots <-> RNS plaintexts on the device ------------------------------------------------------------------------
 * Approximate arithmetic on the scheme-agnostic calls above (fhe_ct_encrypt, fhe_ct_multiply_relin, fhe_rns_rescale_drop_last = the CKKS
 * rescale, fhe_ct_apply_galois, fhe_ct_decrypt): the canonical embedding in FP64.  With h = n/2, zeta = exp(i pi / n), omega = zeta^4:
 *   slot k < h has the exponent e(k) = 3^k mod 2n (the generator of fhe_galois_element): fhe_galois_element(n, r) is a cyclic LEFT rotation of
 *   the h complex slots by r, the element 2n - 1 conjugates them.  The plaintext of z in C^h is the REAL polynomial m of degree < n with
 *   m(zeta^e(k)) = z_k (and so m(zeta^-e(k)) = conj(z_k)).  Exactly one of e(k), 2n - e(k) is 4 a + 1: that a is a(k), and c(k) = 1 says it was
 *   the second (fhe_ckks_slot_table, host only).  With u_j = m_j + i m_(j+h) and w_a(k) = z_k, or conj(z_k) where c(k):
 *       encode  u_j = zeta^-j (1/h) sum_a w_a omega^(-a j)           decode  w_a = sum_j (u_j zeta^j) omega^(a j)
 * encode       d_slots is [batch][n/2][2] doubles (re, im).  c_j = round-to-nearest-even(scale m_j) as a signed 64-bit integer;
 *              d_out[b][l][j] = c_j mod q_l in [0, q_l) (a negative c as q_l - (|c| mod q_l), 0 stays 0) as canonical containers, [batch][L][n]:
 *              the d_m of fhe_ct_encrypt, and one [L][n] slice is a plaintext of fhe_linear_transform_create.  The reduction is division-free,
 *              one table entry per limb prepared at creation.  d_coeff_bits ([batch], may be NULL) receives bit_length(max_j |c_j|), written
 *              by the same launch (nothing to zero first, the call stays capturable).  The contract is exact for d_coeff_bits[b] <= 62; above
 *              that the residues are unspecified and the reported value says so (as d_noise_bits of fhe_ct_decrypt does), and the containers
 *              stay canonical, each in [0, q_l): 63 for 2^62 <= max |c| < 2^63; 64 where a |scale m_j| reaches 2^63 or is not finite (an
 *              infinite or NaN slot makes every coefficient of its plaintext so), saturated and not an error.  Other plaintexts of the batch
 *              are not affected.
 * decode       d_m is [batch][n] uint64_t in [0, t), what fhe_ct_decrypt(.., t, scale = 1, ..) writes: each word is centred (w > t/2 -> w - t),
 *              converted to double and multiplied by 1/scale, then transformed; d_slots is [batch][n/2][2].  t == 0: the words already are
 *              two's-complement int64.  Take t = 2^63, so that no |v| < 2^62 wraps.  "Does not wrap" is not "exact": the centred integer is
 *              converted to double first, so a magnitude above 2^53 is rounded to 53 bits (relative error 2^-53) before the transform.
 * decode_poly  the same from [batch][L][n] containers, reading limb 0 centred modulo q_0: valid for |c| < q_0 / 2 (the round trip without keys).
 * The twiddles come from tables built on the host in long double and rounded once; the device evaluates no sine or cosine.  For a given build
 * the result is a function of (inputs, n, scale, moduli) only, never of the batch size, the position in the batch or the grid.
 *
 * fhe_ckks_encoder_create: n = 2^11 .. 2^14 and every modulus below 2^64; another n or a full-width engine is FHE_ERR_UNSUPPORTED with *out
 * untouched (a two-pass form for n >= 2^15 does not exist).  Every call is ONE launch, one workgroup per plaintext, no workspace, nothing
 * allocated after create: capturable into a hipGraph.  Work is enqueued on h's stream.  FHE_ERR_INVALID_ARG, with nothing launched and nothing
 * written: a null handle, encoder or buffer (d_coeff_bits excepted); an encoder of another engine; batch == 0; a container pointer not 16-byte
 * aligned, a double or uint64_t pointer not 8-byte aligned, d_coeff_bits not 4-byte aligned; an output overlapping an input; a scale that is
 * not finite and > 0.  fhe_ckks_encoder_destroy(NULL) is FHE_OK.  An encoder refers to its engine (every call reads h's stream and limb count) and
 * owns only its tables: destroy it BEFORE the engine, and order all calls that use it on the engine's stream, as for the batch encoder.  fhe_ckks_slot_table needs no device: n a power of two in [2, 2^30]. */
typedef struct fhe_ckks_encoder fhe_ckks_encoder_t;
int fhe_ckks_encoder_create(fhe_rns_ntt_t *h, fhe_ckks_encoder_t **out);
int fhe_ckks_encoder_destroy(fhe_ckks_encoder_t *enc);
int fhe_ckks_slot_table(uint32_t n, uint32_t *a_of_slot, uint8_t *conj_of_slot);   /* host: a(k), c(k), k < n/2 */
int fhe_ckks_encode(fhe_rns_ntt_t *h, const fhe_ckks_encoder_t *enc, void *d_out, uint32_t *d_coeff_bits, const double *d_slots, double scale,
                    uint32_t batch);
int fhe_ckks_decode(fhe_rns_ntt_t *h, const fhe_ckks_encoder_t *enc, double *d_slots, const uint64_t *d_m, uint64_t t, double scale, uint32_t batch);
int fhe_ckks_decode_poly(fhe_rns_ntt_t *h, const fhe_ckks_encoder_t *enc, double *d_slots, const void *d_poly, double scale, uint32_t batch);

/* ---- BFV multiplication: exact RNS lift, scale-and-round by t / Q, one call ------------------------------------------------------------------
 * The scale-invariant encoding Delta m + e, Delta = floor(Q / t), of the reference's keygen / encrypt / decrypt (include/fhe/fhe.hpp:302, 353)
 * cannot be multiplied by fhe_ct_multiply, the tensor product modulo Q: a BFV product is the tensor product over the integers, scaled by t / Q
 * and rounded.  Halevi, Polyakov and Shoup's "simple scaling", with the floating-point sums replaced by 128-bit fixed point so that every call
 * is a deterministic integer function of its inputs.  Q = prod q_i (i < L) the primes of the ciphertext engine hq, P = prod p_j (j < L') the
 * auxiliary NTT primes for the same n, t the plaintext modulus; every modulus below 2^64; containers and layouts as everywhere else.
 *   centred lift of a base B = prod b_i (k primes) to a base C, for residues x_i:
 *       y_i = [x_i (B / b_i)^-1]_{b_i},  r_i = floor(2^128 / b_i),  V = sum y_i r_i,  alpha = floor((V + 2^127) / 2^128)
 *       out_j = (sum_i y_i ((B / b_i) mod c_j) - alpha (B mod c_j)) mod c_j
 *     the centred representative of x, or that +- B for a coefficient with x / B within k 2^-64 of 1/2 modulo 1; the definition decides.
 *   scale and round, base Q u P -> base P: y_m = [x_m (Q P / m)^-1]_m for every prime m; theta_i = t P mod q_i,
 *       rho_i = floor(2^128 theta_i / q_i),  W = sum_i y_i rho_i,  R = floor((W + 2^127) / 2^128)
 *       s_j = (R + sum_i y_i (floor(t P / q_i) mod p_j) + y_{p_j} t (P / p_j)) mod p_j
 *     round(t x / Q) mod p_j for the centred x, up to +-1 where the fractional part is within L 2^-64 of 1/2.
 * fhe_bfv_multiplier_create  the object owns an engine on (q_0 .. q_{L-1}, p_0 .. p_{L'-1}) and the tables above (word-sized host arithmetic, built
 *     once).  FHE_ERR_INVALID_ARG: a null argument; t < 2; num_aux == 0; an auxiliary prime that equals a q_i or another p_j, or is not 1 modulo 2n;
 *     P <= 32 t n Q (checked exactly: the factor 32 covers operands the lift left at +- Q and costs at most one auxiliary prime).
 *     FHE_ERR_UNSUPPORTED: a modulus of 2^64 or more or an hq without a word-sized width class (n < 2^11); L or L' above 16; an extended engine of
 *     another width class than hq (pick auxiliary primes of the ciphertext primes' size).  FHE_ERR_BAD_MODULUS: an auxiliary modulus that is
 *     not prime.  *out stays untouched on failure; fhe_bfv_multiplier_destroy(NULL) is FHE_OK.  Destroy the multiplier BEFORE hq.
 * fhe_bfv_multiplier_engine  the borrowed engine on Q u P: run tensor products of your own there and scale a sum of products once.  Every call
 *     below sets that engine's stream to hq's current stream before it launches.
 * fhe_bfv_lift         [batch][L][n] -> [batch][L + L'][n]: the Q limbs copied, the P limbs from the centred lift.  One launch.
 * fhe_bfv_scale_round  host arrays of 1 to 3 device pointers, inputs [batch][L + L'][n], outputs [batch][L][n]: s as above, then its centred
 *     lift from base P to base Q in the same kernel (s never touches memory).  One launch for all components.
 * fhe_bfv_multiply     lift of the four inputs into the workspace, the tensor product on the extended engine, scale-and-round into c0, c1, c2:
 *     bit for bit that composition through the public calls.  a and b the same buffers: the squaring path of the tensor product.
 * fhe_bfv_multiply_relin  the same with c2 kept in the workspace, then fhe_ct_relinearize on hq: bit for bit fhe_bfv_multiply + fhe_ct_relinearize.
 * fhe_bfv_multiplier_reserve  sizes the multiplier's workspace (7 [batch][L + L'][n] + 1 [batch][L][n] polynomials) and the extended engine's
 *     for `batch`; with a key set also fhe_rns_ntt_reserve(hq, batch).  Afterwards the calls above allocate nothing and can be captured into a
 *     hipGraph.  fhe_bfv_multiplier_workspace_bytes reports the multiplier's and the extended engine's workspaces.
 * FHE_ERR_INVALID_ARG with nothing launched: a null handle or buffer, batch == 0, a container pointer not 16-byte aligned, an output that
 * aliases an input or another output, keys of another engine.  All calls on one multiplier must be ordered on one stream. */
typedef struct fhe_bfv_multiplier fhe_bfv_multiplier_t;
int fhe_bfv_multiplier_create(fhe_rns_ntt_t *hq, fhe_bfv_multiplier_t **out, uint64_t t, const uint64_t *aux_moduli, uint32_t num_aux);
int fhe_bfv_multiplier_destroy(fhe_bfv_multiplier_t *m);
int fhe_bfv_multiplier_engine(const fhe_bfv_multiplier_t *m, fhe_rns_ntt_t **engine);
int fhe_bfv_multiplier_reserve(fhe_bfv_multiplier_t *m, uint32_t batch, const fhe_relin_keys_t *rk_or_null);
int fhe_bfv_multiplier_workspace_bytes(const fhe_bfv_multiplier_t *m, uint64_t *bytes);
int fhe_bfv_lift(fhe_bfv_multiplier_t *m, void *d_out, const void *d_in, uint32_t batch);
int fhe_bfv_scale_round(fhe_bfv_multiplier_t *m, void *const *d_out, const void *const *d_in, uint32_t num_components, uint32_t batch);
int fhe_bfv_multiply(fhe_bfv_multiplier_t *m, void *d_c0, void *d_c1, void *d_c2, const void *d_a0, const void *d_a1, const void *d_b0,
                     const void *d_b1, uint32_t batch);
int fhe_bfv_multiply_relin(fhe_bfv_multiplier_t *m, const fhe_relin_keys_t *rk, void *d_c0, void *d_c1, const void *d_a0, const void *d_a1,
                           const void *d_b0, const void *d_b1, uint32_t batch);

/* Scan a [batch][L][n] buffer for coefficients that are not canonical (>= q_limb, or non-zero
 * upper limbs on the narrow paths).  Synchronises.  FHE_OK or FHE_ERR_NONCANONICAL. */
int fhe_rns_check_canonical(fhe_rns_ntt_t *h, const void *d_data, uint32_t batch);

/* ---- timing on the handle's stream (hipEvent pair; what bench.py uses for the roofline) ------ */
typedef struct fhe_timer fhe_timer_t;
int fhe_timer_create(fhe_timer_t **out);
int fhe_timer_destroy(fhe_timer_t *t);
int fhe_rns_timer_start(fhe_rns_ntt_t *h, fhe_timer_t *t);   /* hipEventRecord(start, h->stream) */
int fhe_rns_timer_stop(fhe_rns_ntt_t *h, fhe_timer_t *t);    /* hipEventRecord(stop,  h->stream) */
int fhe_timer_elapsed_ms(fhe_timer_t *t, float *ms);         /* synchronises on stop */

#ifdef __cplusplus
}
#endif
#endif /* FHE_HIP_H */
