// ntt256.hip.h -- FHE_WIDTH_256 kernels: full-width (q < 2^255) negacyclic NTT and element-wise ops.
//
// The general path behind NTTEngine / RNS_NTTEngine for moduli that do not fit the word-sized fast
// paths (and for transform sizes outside 2^11..2^15).  It is built only from the reference's own
// primitives (u256_dev.h: add_mod / sub_mod / mul_mod_montgomery / ct_butterfly / gs_butterfly,
// include/bigint.cuh:27-140, include/ntt.cuh:147-167) with Montgomery-form twiddles, so data stays in
// plain form exactly as in the reference.
//
// Roofline note: one 256-bit Montgomery product is 128 v_mad_u64_u32 + 128 v_addc_co_u32 (hand-scheduled
// mont_mul_fips, u256_dev.h); at ~14 integer MADs per byte of compulsory traffic this path is bound by
// integer issue, not by HBM, so it runs as plain
// multi-pass radix-2^R register kernels over global memory (R <= 3 stages per launch, every access a
// whole 32-byte container, consecutive lanes on consecutive containers) without LDS staging.
//
// This file holds the types every part shares; the kernels are in ntt256_{transforms,literal,keyswitch,rns}.hip.h, one part per host
// source, so that each kernel is compiled into exactly one object.
#pragma once
#include "u256_dev.h"

namespace fhe_dev {

struct Limb256 {
    u256 q;
    u256 r2;          // R^2 mod q
    u256 ninv_m;      // n^-1 * R mod q
    uint64_t inv0;    // -q^-1 mod 2^64  (MontgomeryParams::inv.limbs[0], include/bigint.cuh:167-173)
    uint64_t _pad;
    const u256 *tw_m;   // [n] psi^bitrev(k) * R mod q
    const u256 *itw_m;  // [n] psi^-bitrev(k) * R mod q
};

// ---- RNS entry / exit (RNS_NTTEngine::to_rns / from_rns, include/ntt.cuh:114-117; src/rns.cu:93-141 are placeholders) ---
// Container-level operations, independent of the width class of the transforms.
struct CrtLimb {
    u256 q, r2;          // modulus, R^2 mod q
    u256 minv_m;         // ((Q/q)^-1 mod q) * R mod q
    u256 Mi_mQ;          // (Q/q) * R mod Q          (Montgomery form with respect to Q)
    uint64_t inv0, _pad;
};
struct CrtBig { u256 Q; uint64_t inv0, _pad; };
struct RescaleLimb { u256 qlast_inv_m; };   // (q_last^-1 mod q_l) * R mod q_l

}  // namespace fhe_dev
