// mfma_digits.hpp — what the matrix-core kernels of direct.hip and pool_encode.hip share: the signed base-256 digits of a field element (the i8
// operands of v_mfma_i32_32x32x32_i8), the way back from four i32 digit sums to a canonical word, and a wave-uniform buffer descriptor.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf.hpp"

namespace fastecc {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));

// Signed base-256 digits, packed: x = sum_a s_a 256^a (mod p) with s_a in [-128, 127], s_a = byte a of the result as int8.
// y = x + 0x80808080 biases every digit by 128; where that would carry out of 32 bits (x >= 0x7F7F7F80) the value is taken as x - p
// instead (2^32 = 2^20 - 1 mod p: y + 0xFFFFF, which cannot carry again).  Bytes of y are the biased digits; flipping bit 7 un-biases.
__device__ __forceinline__ uint32_t balanced_digits(uint32_t x)
{
    const uint32_t bias = x >= 0x7F7F7F80u ? 0x8090807Fu : 0x80808080u;
    return (x + bias) ^ 0x80808080u;
}

// The canonical word of sum_b d_b 256^b for four i32 digit sums, |d_b| < 2^28: |sum| < 2^53, + p * 2^24 makes it positive.
__device__ __forceinline__ uint32_t digit_sums_to_word(int d0, int d1, int d2, int d3)
{
    const int64_t v = (int64_t)d0 + ((int64_t)d1 << 8) + ((int64_t)d2 << 16) + ((int64_t)d3 << 24);
    const uint64_t t = (uint64_t)(v + ((int64_t)gf::P << 24));
    const uint32_t tl = (uint32_t)t, th = (uint32_t)(t >> 32);  // th < 2^26
    return gf::add(gf::mul(th, gf::MONT_ONE), tl >= gf::P ? tl - gf::P : tl);
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t direct_desc(const void* p, uint32_t bytes)
{
    // the pointer is wave-uniform; readfirstlane makes that provable (no waterfall loop around the buffer ops)
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), 0, __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}

}  // namespace fastecc
