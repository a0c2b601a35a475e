// galois_ab.hip -- interleaved A/B of the two forms of the rotation prologue (csrc/galois.hip.h): galois_compact_kernel<F, true> (limb
// polynomial staged in LDS, permuted reads from LDS) against <F, false> (plain gather through L2), both components of a ciphertext batch
// in one launch, containers in, compact out (+ the zero slice).  DESIGN.md 4.9 records the numbers.
// build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -I ../gpu-homomorphic-encryption_amd/csrc -o galois_ab galois_ab.hip
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "galois.hip.h"

using namespace fhe_dev;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("%s: %s\n", #x, hipGetErrorString(e_)); std::exit(1); } } while (0)

template <class F>
static void run(const char *field, uint32_t log_n, uint32_t L, uint32_t batch, uint64_t q) {
    using E = typename F::E; using V = typename F::V16;
    const uint32_t n = 1u << log_n;
    const size_t polys = (size_t)batch * L, cont = polys * n;
    std::vector<uint64_t> h(cont * 4, 0);
    uint64_t s = 88172645463325252ull;
    for (size_t i = 0; i < cont; i++) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; h[4 * i] = s % q; }
    std::vector<Limb<F>> limbs(L);
    for (auto &P : limbs) { std::memset(&P, 0, sizeof P); P.q = (E)q; }
    void *c0, *c1, *ws, *dl;
    CK(hipMalloc(&c0, cont * 32)); CK(hipMalloc(&c1, cont * 32)); CK(hipMalloc(&ws, 3 * cont * sizeof(E))); CK(hipMalloc(&dl, L * sizeof(Limb<F>)));
    CK(hipMemcpy(c0, h.data(), cont * 32, hipMemcpyHostToDevice)); CK(hipMemcpy(c1, h.data(), cont * 32, hipMemcpyHostToDevice));
    CK(hipMemcpy(dl, limbs.data(), L * sizeof(Limb<F>), hipMemcpyHostToDevice));
    E *s0 = (E *)ws, *s1 = s0 + cont, *z = s1 + cont;
    const uint32_t g = 3, m = 2 * n;
    uint32_t g_inv = g; for (int i = 0; i < 5; i++) g_inv *= 2 - g * g_inv; g_inv &= m - 1;
    const size_t lds = (size_t)n * sizeof(E);
    const bool can_stage = lds <= GALOIS_LDS_BYTES;
    size_t gb = (cont + 255) / 256; if (gb > 8192) gb = 8192;
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    auto launch = [&](bool staged) {
        if (staged) hipLaunchKernelGGL((galois_compact_kernel<F, true>), dim3((unsigned)polys, 2), dim3(GALOIS_T), lds, 0, s0, s1, z, (const V *)c0, (const V *)c1, (const Limb<F> *)dl, L, log_n, g_inv, polys);
        else hipLaunchKernelGGL((galois_compact_kernel<F, false>), dim3((unsigned)gb, 2), dim3(GALOIS_T), 0, 0, s0, s1, z, (const V *)c0, (const V *)c1, (const Limb<F> *)dl, L, log_n, g_inv, polys);
    };
    double best[2] = {1e30, 1e30};
    for (int rep = 0; rep < 6; rep++)
        for (int f = can_stage ? 0 : 1; f < 2; f++) {                  // interleaved: staged, gather, staged, gather, ...
            launch(f == 0); launch(f == 0); CK(hipDeviceSynchronize());
            const int iters = 20;
            CK(hipEventRecord(a, 0));
            for (int i = 0; i < iters; i++) launch(f == 0);
            CK(hipEventRecord(b, 0)); CK(hipEventSynchronize(b));
            float ms = 0; CK(hipEventElapsedTime(&ms, a, b));
            if (ms / iters < best[f]) best[f] = ms / iters;
        }
    const double bytes = 2.0 * cont * 32 + 3.0 * cont * sizeof(E);      // two container components read, three compact polynomials written
    for (int f = can_stage ? 0 : 1; f < 2; f++)
        std::printf("%s N=%u L=%u batch=%u %-7s %9.1f us  %6.2f TB/s (2 S in + 3 compact out)\n", field, n, L, batch, f ? "gather" : "staged", best[f] * 1e3,
                    bytes / (best[f] * 1e-3) / 1e12);
    CK(hipFree(c0)); CK(hipFree(c1)); CK(hipFree(ws)); CK(hipFree(dl));
}

int main() {
    run<F32>("F32", 13, 4, 1024, 1073692673ull);       // configs[2] shape (a 30-bit prime = 1 mod 2^14)
    run<F32>("F32", 14, 6, 128, 1073692673ull);        // configs[3] shape
    run<F52>("F52", 13, 4, 256, 549755731969ull);      // 40-bit residues as doubles
    run<F64>("F64", 13, 4, 256, 1152921504606584833ull);
    return 0;
}
