// gf61_limbs.hpp — a GF((2^61-1)^2) product with a wave-uniform factor as plain 64-bit multiply-adds: the weight tables of the decoder's direct
// path (gf61_decode.hip: k_direct_coef, k_direct_accumulate) and of the small writes (gf61_update.hip).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf61.hpp"

namespace fastecc {
namespace p61 {

// ---- lazy accumulation: no reduction per term ----
// A weight component c < 2^61 is wave-uniform.  With c' = c * 2^32 mod p (a rotation of its 61 bits) a data component a = a1 2^32 + a0 (ANY 64-bit
// word) gives a * c = a0 * c + a1 * c' (mod p), and with c = l0 + l1 2^21 + l2 2^42 (limbs of 21, 21, 19 bits) every partial product is below 2^53:
// a sum of 4 products per row over DIRECT_ROWS = 512 rows stays below 2^64 in a plain 64-bit accumulator — one v_mad_u64_u32 per product, no carry,
// no fold.  re = a c + b (p - d), im = a d + b c: 24 multiply-adds per term (the reducing form: 16 + limb splits + three folds = 58 instructions).
// The 18 limbs of a weight — of c, c', d, d', e = p - d, e' — are what the table holds (COEF_WORDS 32-bit words per entry, all zero for a zero weight):
// splitting them in the kernel costs 35 scalar instructions per term, and the scalar unit, shared by the four SIMDs of a CU, then limits the kernel
// (measured: 16 lost blocks 3.0 ms against 3.6 for the reducing form).  The three sums of a component are put together once per chunk.
constexpr int COEF_WORDS = 18;
struct Limbs {
    uint32_t l0, l1, l2;
};
__device__ __forceinline__ Limbs limbs_of(uint64_t v) { return Limbs{(uint32_t)v & 0x1FFFFFu, (uint32_t)(v >> 21) & 0x1FFFFFu, (uint32_t)(v >> 42)}; }
__device__ __forceinline__ uint64_t times_2_32(uint64_t v) { return ((v << 32) & gf61::P) | (v >> 29); }  // v <= p: v 2^32 mod p (or p for v = p)
struct Acc3 {
    uint64_t t0, t1, t2;
};
__device__ __forceinline__ void mac3(Acc3& s, uint32_t x, const Limbs& w)
{
    s.t0 += (uint64_t)x * w.l0;
    s.t1 += (uint64_t)x * w.l1;
    s.t2 += (uint64_t)x * w.l2;
}
// t0 + t1 2^21 + t2 2^42 (mod p) as a lazy value (< 2^61 + 4)
__device__ __forceinline__ uint64_t gather3(const Acc3& s)
{
    auto fold = [](uint64_t t) { return (t & gf61::P) + (t >> 61); };                                       // < 2^61 + 8
    auto shl = [](uint64_t y, int sh) { return ((y << sh) & gf61::P) + (y >> (61 - sh)); };                // y < 2^62: y 2^sh mod p, < 2^61 + 2^(sh + 1)
    return fold(fold(s.t0) + shl(fold(s.t1), 21) + shl(fold(s.t2), 42));                                    // the sum is below 2^63
}

__device__ __forceinline__ void store_weight(uint32_t* __restrict__ o, gf61::Elem v)
{
    if ((v.re | v.im) == 0) {
        for (int i = 0; i < COEF_WORDS; ++i) o[i] = 0;
        return;
    }
    const uint64_t nim = gf61::P - v.im;
    const uint64_t parts[6] = {v.re, times_2_32(v.re), v.im, times_2_32(v.im), nim, times_2_32(nim)};
    for (int i = 0; i < 6; ++i) {
        const Limbs l = limbs_of(parts[i]);
        o[3 * i] = l.l0;
        o[3 * i + 1] = l.l1;
        o[3 * i + 2] = l.l2;
    }
}

}  // namespace p61
}  // namespace fastecc
