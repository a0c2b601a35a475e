// ntt256.hip.h -- FHE_WIDTH_256: the types shared by the container-level kernels of a full-width handle (q < 2^255, or any handle
// where an entry point works on whole 32-byte containers: RNS entry / exit, mixed-class conversions).
//
// A full-width engine keeps TWO limb tables.  Limb256 (here, h->d_limbs) holds the constants of the container-level kernels --
// element-wise ops, canonical check, composed key switch, conversions -- which compute with mont_mul_fips / mont_mul of u256_dev.h at
// the reference's radix R = 2^256 and leave data in plain form exactly as the reference does.  WLimb<NL> (ntt_wide.hip.h,
// h->d_wlimbs) holds the constants and the twiddle tables of the transforms: global-memory passes over the top stages, LDS tiles of 2^11
// coefficients below them, on the one-block products of wide_asm.inc at radix 2^(64 NL).  Limb256 has no twiddle tables of its own.
//
// The kernels are in ntt256_{transforms,literal,keyswitch,rns}.hip.h, one part per host source, so that each kernel is compiled into
// exactly one object.
#pragma once
#include "u256_dev.h"

namespace fhe_dev {

struct Limb256 {
    u256 q;
    u256 r2;          // R^2 mod q
    u256 ninv_m;      // n^-1 * R mod q
    uint64_t inv0;    // -q^-1 mod 2^64  (MontgomeryParams::inv.limbs[0], include/bigint.cuh:167-173)
    uint64_t _pad;
    const void *_pad_tw[2];   // where two twiddle-table pointers were: sizeof(Limb256) and every offset stay as the kernels index them
};
static_assert(sizeof(Limb256) == 128 && alignof(Limb256) == 16, "the kernels index limbs[p % L] with this layout");

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
// BGV modulus switch (fhe_ct_mod_switch_drop_last): entry l < L-1 holds the constants of output limb l, entry L-1 (qlast_inv_m only) -t^-1 mod q_last
struct ModSwitchLimb {
    u256 qlast_inv_m;    // (q_last^-1 mod q_l) * R mod q_l          entry L-1: (-t^-1 mod q_last) * R mod q_last
    u256 t_qlast_inv;    // t * q_last^-1 mod q_l, PLAIN: multiplied into a value that already carries R
};
struct ModSwitchPtrs { const void *in[3]; void *out[3]; };   // the components of one call, by value in the kernel arguments

}  // namespace fhe_dev
