// lazy96.hpp — exact sums of products x * w mod p = 0xFFF00001 in 96-bit accumulators, reduced once per run of terms (direct.hip: the
// few-loss decoder and the direct encoder; update.hip: the parity update).  w is wave-uniform and in Montgomery form (gf.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf.hpp"

namespace fastecc {

// (hi:lo) += x * w, w wave-uniform: the 64-bit multiply-add delivers its carry in an SGPR pair, the add-with-carry consumes it
__device__ __forceinline__ void mac96(uint64_t& lo, uint32_t& hi, uint32_t x, uint32_t w)
{
    uint64_t c;
    asm("v_mad_u64_u32 %0, %1, %2, %3, %0" : "+v"(lo), "=s"(c) : "v"(x), "s"(w));
    asm("v_addc_co_u32_e64 %0, %1, 0, %0, %1" : "+v"(hi), "+s"(c));
}
// (hi * 2^64 + lo) / 2^32 mod p: the sum of products with Montgomery-form weights, as a plain representative
__device__ __forceinline__ uint32_t reduce96(uint64_t lo, uint32_t hi)
{
    const uint32_t l0 = (uint32_t)lo, l1 = (uint32_t)(lo >> 32);
    uint32_t r = gf::mul_mont(l0, 1u);                            // l0 / 2^32
    r = gf::add(r, l1 >= gf::P ? l1 - gf::P : l1);                // l1
    r = gf::add(r, gf::mul(hi >= gf::P ? hi - gf::P : hi, gf::MONT_ONE));  // hi * 2^32
    return r;
}

}  // namespace fastecc
