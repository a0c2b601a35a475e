// core.hip -- last error, device and memory entry points, host number theory, timers (no kernels).
#include "engine.h"

// ------------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

int fail(int code, const std::string &msg) { g_last_error = msg; return code; }

static bool env_sync() {
    static int v = -1;
    if (v < 0) { const char *e = getenv("FHE_HIP_SYNC"); v = (e && e[0] == '1') ? 1 : 0; }
    return v == 1;
}

int ensure_device() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(FHE_ERR_NO_DEVICE, std::string("no usable HIP device (hipGetDeviceCount: ") +
                                           (e == hipSuccess ? "0 devices" : hipGetErrorString(e)) +
                                           "); this library has no CPU fallback");
    }
    return FHE_OK;
}

int post_launch(hipStream_t s, const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FHE_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
    if (env_sync()) {
        e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(FHE_ERR_HIP, std::string(what) + " sync: " + hipGetErrorString(e));
    }
    return FHE_OK;
}

// ------------------------------------------------------------------------------------------------------
// plumbing entry points
// ------------------------------------------------------------------------------------------------------
extern "C" int fhe_hip_abi_version(void) { return FHE_HIP_ABI_VERSION; }
extern "C" const char *fhe_hip_last_error(void) { return g_last_error.c_str(); }

extern "C" int fhe_hip_device_count(int *count) {
    if (!count) return fail(FHE_ERR_INVALID_ARG, "count is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { (void)hipGetLastError(); *count = 0; return fail(FHE_ERR_NO_DEVICE, hipGetErrorString(e)); }
    *count = n;
    return FHE_OK;
}
extern "C" int fhe_hip_set_device(int device) {
    int rc = ensure_device(); if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    return FHE_OK;
}
extern "C" int fhe_hip_get_device(int *device) {
    if (!device) return fail(FHE_ERR_INVALID_ARG, "device is null");
    int rc = ensure_device(); if (rc) return rc;
    HIP_TRY(hipGetDevice(device));
    return FHE_OK;
}
extern "C" int fhe_hip_device_name(char *buf, size_t buflen) {
    if (!buf || !buflen) return fail(FHE_ERR_INVALID_ARG, "buf is null");
    int rc = ensure_device(); if (rc) return rc;
    int dev = 0; HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t prop; HIP_TRY(hipGetDeviceProperties(&prop, dev));
    snprintf(buf, buflen, "%s %s (%d CUs)", prop.gcnArchName, prop.name, prop.multiProcessorCount);
    return FHE_OK;
}
extern "C" int fhe_hip_malloc(void **d_ptr, size_t bytes) {
    if (!d_ptr) return fail(FHE_ERR_INVALID_ARG, "d_ptr is null");
    int rc = ensure_device(); if (rc) return rc;
    HIP_TRY(hipMalloc(d_ptr, bytes ? bytes : 1));
    return FHE_OK;
}
extern "C" int fhe_hip_free(void *d_ptr) { if (d_ptr) HIP_TRY(hipFree(d_ptr)); return FHE_OK; }
extern "C" int fhe_hip_memset(void *d_ptr, int value, size_t bytes) { HIP_TRY(hipMemset(d_ptr, value, bytes)); return FHE_OK; }
extern "C" int fhe_hip_memcpy_h2d(void *d, const void *h, size_t bytes) { HIP_TRY(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice)); return FHE_OK; }
extern "C" int fhe_hip_memcpy_d2h(void *h, const void *d, size_t bytes) { HIP_TRY(hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost)); return FHE_OK; }
extern "C" int fhe_hip_memcpy_d2d(void *d, const void *s, size_t bytes) { HIP_TRY(hipMemcpy(d, s, bytes, hipMemcpyDeviceToDevice)); return FHE_OK; }
extern "C" int fhe_hip_sync(void) { int rc = ensure_device(); if (rc) return rc; HIP_TRY(hipDeviceSynchronize()); return FHE_OK; }

// ------------------------------------------------------------------------------------------------------
// host parameter maths (no device needed)
// ------------------------------------------------------------------------------------------------------
extern "C" int fhe_montgomery_inverse(const uint64_t q[4], uint64_t inv[4]) {
    if (!q || !inv) return fail(FHE_ERR_INVALID_ARG, "null argument");
    // literal: 6 Newton steps on the low limb from x = 1, negated (src/bigint.cu:27-37); garbage for even q
    inv[0] = fhe_host::neg_inv64(q[0]); inv[1] = inv[2] = inv[3] = 0;
    return FHE_OK;
}
extern "C" int fhe_montgomery_params(const uint64_t q[4], uint64_t r_squared[4], uint64_t inv[4]) {
    if (!q || !r_squared || !inv) return fail(FHE_ERR_INVALID_ARG, "null argument");
    U256 Q = U256::from(q);
    if (!(Q.w[0] & 1) || (Q.w[3] >> 63) || Q.bit_length() < 2) return fail(FHE_ERR_BAD_MODULUS, "modulus must be odd, > 1 and < 2^255");
    fhe_host::Mod M(Q);
    std::memcpy(r_squared, M.r2.w, 32);
    return fhe_montgomery_inverse(q, inv);
}
extern "C" int fhe_find_ntt_primes(uint32_t bits, uint32_t n, uint32_t count, uint64_t *primes_out) {
    if (!primes_out || !count) return fail(FHE_ERR_INVALID_ARG, "null output / zero count");
    if (!fhe_host::find_ntt_primes(bits, n, count, primes_out))
        return fail(FHE_ERR_INVALID_ARG, "no such primes (need 4 <= bits <= 64, n a power of two, 2n < 2^(bits-1))");
    return FHE_OK;
}
extern "C" int fhe_find_ntt_primes_wide(uint32_t bits, uint32_t n, uint32_t count, uint64_t (*primes_out)[4]) {
    if (!primes_out || !count) return fail(FHE_ERR_INVALID_ARG, "null output / zero count");
    std::vector<U256> ps(count);
    if (!fhe_host::find_ntt_primes_wide(bits, n, count, ps.data()))
        return fail(FHE_ERR_INVALID_ARG, "no such primes (need 4 <= bits <= 255, n a power of two, 2n < 2^(bits-2))");
    for (uint32_t i = 0; i < count; i++) std::memcpy(primes_out[i], ps[i].w, 32);
    return FHE_OK;
}
extern "C" int fhe_find_psi(uint32_t n, const uint64_t q[4], uint64_t psi[4]) {
    if (!q || !psi) return fail(FHE_ERR_INVALID_ARG, "null argument");
    if (n < 2 || (n & (n - 1))) return fail(FHE_ERR_INVALID_ARG, "n must be a power of two");
    U256 Q = U256::from(q);
    if (!(Q.w[0] & 1) || (Q.w[3] >> 63) || !fhe_host::is_prime(Q)) return fail(FHE_ERR_BAD_MODULUS, "modulus must be an odd prime < 2^255");
    fhe_host::Mod M(Q); U256 p;
    if (fhe_host::find_psi(n, M, p) != fhe_host::BUILD_OK) return fail(FHE_ERR_BAD_MODULUS, "q != 1 (mod 2n): no primitive 2n-th root");
    std::memcpy(psi, p.w, 32);
    return FHE_OK;
}

// ------------------------------------------------------------------------------------------------------
// timers
// ------------------------------------------------------------------------------------------------------
struct fhe_timer { hipEvent_t start, stop; };
extern "C" int fhe_timer_create(fhe_timer_t **out) {
    if (!out) return fail(FHE_ERR_INVALID_ARG, "null argument");
    int rc = ensure_device(); if (rc) return rc;
    fhe_timer *t = new (std::nothrow) fhe_timer();
    if (!t) return fail(FHE_ERR_INVALID_ARG, "out of host memory");
    HIP_TRY(hipEventCreate(&t->start)); HIP_TRY(hipEventCreate(&t->stop));
    *out = t;
    return FHE_OK;
}
extern "C" int fhe_timer_destroy(fhe_timer_t *t) {
    if (t) { (void)hipEventDestroy(t->start); (void)hipEventDestroy(t->stop); delete t; }
    return FHE_OK;
}
extern "C" int fhe_rns_timer_start(fhe_rns_ntt_t *h, fhe_timer_t *t) {
    if (!h || !t) return fail(FHE_ERR_INVALID_ARG, "null argument");
    HIP_TRY(hipEventRecord(t->start, h->stream)); return FHE_OK;
}
extern "C" int fhe_rns_timer_stop(fhe_rns_ntt_t *h, fhe_timer_t *t) {
    if (!h || !t) return fail(FHE_ERR_INVALID_ARG, "null argument");
    HIP_TRY(hipEventRecord(t->stop, h->stream)); return FHE_OK;
}
extern "C" int fhe_timer_elapsed_ms(fhe_timer_t *t, float *ms) {
    if (!t || !ms) return fail(FHE_ERR_INVALID_ARG, "null argument");
    HIP_TRY(hipEventSynchronize(t->stop));
    HIP_TRY(hipEventElapsedTime(ms, t->start, t->stop));
    return FHE_OK;
}
