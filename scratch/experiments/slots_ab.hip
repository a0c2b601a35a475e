// slots_ab.hip -- interleaved A/B of the batch encoder's two gather / scatter forms on one GPU: permuted global accesses (slots_global.hip.h,
// "global") against the permutation through the exchange buffer (csrc/encode.hip.h, the adopted form, "lds").  Stand-alone: the limb constants and twiddle
// tables are arbitrary words below q (the time of a butterfly does not depend on its operands), the position -> slot tables are the real ones,
// and the two forms must give the same bytes.  One JSON line per (field, N, L, order, op); best of REPS, the forms alternating.
// build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -mllvm -pragma-unroll-threshold=1000000 -o slots_ab slots_ab.hip
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "slots_global.hip.h"

using namespace fhe_dev;

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "HIP %s at line %d\n", hipGetErrorString(e_), __LINE__); std::exit(1); } } while (0)

static uint64_t rnd_state = 88172645463325252ull;
static uint64_t rnd() { rnd_state ^= rnd_state << 13; rnd_state ^= rnd_state >> 7; rnd_state ^= rnd_state << 17; return rnd_state; }
static uint32_t brev(uint32_t x, uint32_t bits) { uint32_t r = 0; for (uint32_t i = 0; i < bits; i++) { r = (r << 1) | (x & 1); x >>= 1; } return r; }

static std::vector<uint32_t> slot_table(uint32_t n, uint32_t log_n, int rows) {
    std::vector<uint32_t> t(n);
    uint32_t e = 1;
    for (uint32_t i = 0; i < (rows ? n / 2 : n); i++) {
        if (!rows) t[brev(i, log_n)] = i;
        else { t[brev((e - 1) / 2, log_n)] = i; t[brev((2 * n - e - 1) / 2, log_n)] = n / 2 + i; e = (uint32_t)(((uint64_t)e * 3) & (2 * n - 1)); }
    }
    return t;
}

template <class F> static void set_modulus(Limb<F> &P);
template <> void set_modulus<F32>(Limb<F32> &P) {
    const uint32_t q = 1073479681u;                       // odd, below 2^30
    uint32_t x = 1; for (int i = 0; i < 5; i++) x *= 2 - q * x;
    P.q = q; P.q2 = 2 * q; P.qinv = 0u - x;
}
template <> void set_modulus<F64>(Limb<F64> &P) {
    const uint64_t q = (1ull << 59) + 163841;             // odd, below 2^62
    uint64_t x = 1; for (int i = 0; i < 6; i++) x *= 2 - q * x;
    P.q = q; P.q2 = 2 * q; P.qinv = x;
}

template <class F, int LOGN>
static void run(const char *field, uint32_t L, uint32_t batch, int reps) {
    using E = typename F::E; using TW = typename F::TW;
    constexpr uint32_t n = 1u << LOGN, T = NttCfg<LOGN>::T;
    Limb<F> P; std::memset(&P, 0, sizeof P);
    set_modulus<F>(P);
    const uint64_t q = (uint64_t)P.q;
    for (E *f : {&P.r1, &P.r1_s, &P.ninv, &P.ninv_s, &P.ninvw, &P.ninvw_s}) *f = (E)(rnd() % q);
    std::vector<TW> tw(n);
    for (uint32_t k = 0; k < n; k++) { uint64_t w[2] = {rnd() % q, rnd()}; std::memcpy(&tw[k], w, sizeof(TW)); }
    TW *d_tw, *d_itw; Limb<F> *d_limb;
    HIP_OK(hipMalloc(&d_tw, n * sizeof(TW))); HIP_OK(hipMalloc(&d_itw, n * sizeof(TW))); HIP_OK(hipMalloc(&d_limb, sizeof P));
    HIP_OK(hipMemcpy(d_tw, tw.data(), n * sizeof(TW), hipMemcpyHostToDevice));
    for (uint32_t k = 0; k < n; k++) { uint64_t w[2] = {rnd() % q, rnd()}; std::memcpy(&tw[k], w, sizeof(TW)); }
    HIP_OK(hipMemcpy(d_itw, tw.data(), n * sizeof(TW), hipMemcpyHostToDevice));
    P.tw = d_tw; P.itw = d_itw;
    HIP_OK(hipMemcpy(d_limb, &P, sizeof P, hipMemcpyHostToDevice));
    std::vector<fhe_host::ModT> red(L); std::memset(red.data(), 0, L * sizeof(fhe_host::ModT));
    fhe_host::ModT *d_red; HIP_OK(hipMalloc(&d_red, L * sizeof(fhe_host::ModT)));
    HIP_OK(hipMemcpy(d_red, red.data(), L * sizeof(fhe_host::ModT), hipMemcpyHostToDevice));
    const size_t words = (size_t)batch * n, out_bytes = words * L * 32;
    std::vector<uint64_t> vals(words);
    for (uint64_t &v : vals) v = rnd() % q;
    uint64_t *d_vals, *d_back[2]; char *d_out[2]; uint32_t *d_table;
    HIP_OK(hipMalloc(&d_vals, words * 8)); HIP_OK(hipMalloc(&d_table, n * 4));
    for (int i = 0; i < 2; i++) { HIP_OK(hipMalloc(&d_out[i], out_bytes)); HIP_OK(hipMalloc(&d_back[i], words * 8)); }
    HIP_OK(hipMemcpy(d_vals, vals.data(), words * 8, hipMemcpyHostToDevice));
    hipEvent_t e0, e1; HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1));
    for (int rows = 0; rows < 2; rows++) {
        const std::vector<uint32_t> table = slot_table(n, LOGN, rows);
        HIP_OK(hipMemcpy(d_table, table.data(), n * 4, hipMemcpyHostToDevice));
        auto enc = [&](int form) {
            if (form) hipLaunchKernelGGL((ntt_slots_encode_kernel<F, LOGN>), dim3(batch), dim3(T), 0, 0, d_out[1], d_vals, d_table, d_red, d_limb, L);
            else hipLaunchKernelGGL((ntt_slots_encode_global_kernel<F, LOGN>), dim3(batch), dim3(T), 0, 0, d_out[0], d_vals, d_table, d_red, d_limb, L);
        };
        auto dec = [&](int form) {                        // from the 8-byte words, the layout fhe_ct_decrypt writes
            if (form) hipLaunchKernelGGL((ntt_slots_decode_kernel<F, LOGN, false>), dim3(batch), dim3(T), 0, 0, d_back[1], (const char *)d_vals, d_table, d_limb, L);
            else hipLaunchKernelGGL((ntt_slots_decode_global_kernel<F, LOGN, false>), dim3(batch), dim3(T), 0, 0, d_back[0], (const char *)d_vals, d_table, d_limb, L);
        };
        for (int op = 0; op < 2; op++) {
            auto launch = [&](int form) { if (op) dec(form); else enc(form); };
            launch(0); launch(1);
            HIP_OK(hipDeviceSynchronize());
            {   // same bytes
                const size_t bytes = op ? words * 8 : out_bytes, chunk = std::min(bytes, (size_t)64 << 20);
                std::vector<char> a(chunk), c(chunk);
                HIP_OK(hipMemcpy(a.data(), op ? (char *)d_back[0] : d_out[0], chunk, hipMemcpyDeviceToHost));
                HIP_OK(hipMemcpy(c.data(), op ? (char *)d_back[1] : d_out[1], chunk, hipMemcpyDeviceToHost));
                if (std::memcmp(a.data(), c.data(), chunk)) { std::fprintf(stderr, "the two forms differ (%s N=%u %s %s)\n", field, n, rows ? "rows" : "natural", op ? "decode" : "encode"); std::exit(1); }
            }
            float best[2] = {1e30f, 1e30f};
            for (int r = 0; r < reps; r++)
                for (int form = 0; form < 2; form++) {
                    HIP_OK(hipEventRecord(e0, 0));
                    for (int i = 0; i < 3; i++) launch(form);
                    HIP_OK(hipEventRecord(e1, 0));
                    HIP_OK(hipEventSynchronize(e1));
                    float ms; HIP_OK(hipEventElapsedTime(&ms, e0, e1));
                    if (ms / 3 < best[form]) best[form] = ms / 3;
                }
            const double moved = op ? (double)words * 16 : (double)words * 8 + (double)out_bytes;
            std::printf("{\"field\": \"%s\", \"n\": %u, \"limbs\": %u, \"batch\": %u, \"order\": \"%s\", \"op\": \"%s\", \"global_us\": %.2f, \"lds_us\": %.2f, "
                        "\"global_tb_per_s\": %.3f, \"lds_tb_per_s\": %.3f, \"lds_over_global\": %.3f}\n", field, n, L, batch, rows ? "rows" : "natural", op ? "decode" : "encode",
                        best[0] * 1e3, best[1] * 1e3, moved / (best[0] * 1e-3) / 1e12, moved / (best[1] * 1e-3) / 1e12, best[1] / best[0]);
            std::fflush(stdout);
        }
    }
    for (void *p : {(void *)d_tw, (void *)d_itw, (void *)d_limb, (void *)d_red, (void *)d_vals, (void *)d_table, (void *)d_out[0], (void *)d_out[1], (void *)d_back[0], (void *)d_back[1]}) HIP_OK(hipFree(p));
    HIP_OK(hipEventDestroy(e0)); HIP_OK(hipEventDestroy(e1));
}

int main() {
    const int reps = 7;
    run<F32, 11>("F32", 2, 4096, reps);
    run<F32, 13>("F32", 4, 1024, reps);
    run<F32, 14>("F32", 6, 1024, reps);
    run<F64, 13>("F64", 4, 1024, reps);
    run<F64, 14>("F64", 6, 1024, reps);
    return 0;
}
