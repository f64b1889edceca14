// scrub_device.hpp — device code of the scrub path, included by scrub.hip only (its head comment says what every pass computes): the block
// fingerprint and its four kernels, the locator tables, the syndrome checks and gathers, the root searches.  The kernels are tuned one by one
// (79/80/82 VGPRs, five or six waves per SIMD: DESIGN.md sections 14, 17, 19 and 27) and are not merged or re-templated.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fastecc.h"
#include "gf.hpp"

namespace fastecc {

namespace {

constexpr int R = 3;   // fingerprint columns (the transform stripe has 4 words per position; the 4th stays zero)
constexpr int RW = 4;  // words per position of the fingerprint stripe

// x mod p for any 64-bit x (2^32 = 2^20 - 1 mod p); three folds leave < 2^33 < 3p
__device__ __forceinline__ uint64_t fold64(uint64_t x)
{
    x = (x >> 32) * 0xFFFFFull + (x & 0xFFFFFFFFull);
    x = (x >> 32) * 0xFFFFFull + (x & 0xFFFFFFFFull);
    x = (x >> 32) * 0xFFFFFull + (x & 0xFFFFFFFFull);
    return x;
}
__device__ __forceinline__ uint32_t reduce64(uint64_t x)
{
    x = fold64(x);
    if (x >= gf::P) x -= gf::P;
    if (x >= gf::P) x -= gf::P;
    return (uint32_t)x;
}

__device__ __forceinline__ void mad3(uint64_t& a0, uint64_t& a1, uint64_t& a2, uint32_t v, uint32_t wx, uint32_t wy)
{
    // packed weights of one word: wx = rho0 | (rho2 & 0xFFF) << 20, wy = rho1 | (rho2 >> 12) << 20
    const uint32_t r0 = wx & 0xFFFFFu, r1 = wy & 0xFFFFFu, r2 = (wx >> 20) | ((wy >> 20) << 12);
    a0 += (uint64_t)v * r0;
    a1 += (uint64_t)v * r1;
    a2 += (uint64_t)v * r2;
}

// One wave's fingerprint of one block of S words.  VEC: S % 4 == 0 and a 16-byte aligned block — lane l reads words 4l + 256 i as
// dwordx4, four loads in flight per batch; else one word per lane and step.  Sums: products < 2^52, folded every 4096 of them.
// Every lane gets the three fingerprints (mod p) and whether some word of the block is >= p.
template <bool VEC>
__device__ __forceinline__ void block_fingerprint(const uint32_t* __restrict__ blk, uint32_t S, const uint2* __restrict__ wt, uint32_t lane, uint32_t f[R],
                                                  bool& any_big)
{
    uint64_t a0 = 0, a1 = 0, a2 = 0;
    uint32_t big = 0;
    if (VEC) {
        const uint4* wt4 = reinterpret_cast<const uint4*>(wt);
        uint32_t batches = 0;
        for (uint32_t base = lane * 4u; base < S; base += 1024u) {
            uint4 v[4], wa[4], wb[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t w = base + 256u * u;
                if (w < S) {
                    v[u] = *reinterpret_cast<const uint4*>(blk + w);
                    wa[u] = wt4[w >> 1];
                    wb[u] = wt4[(w >> 1) + 1];
                } else {
                    v[u] = wa[u] = wb[u] = make_uint4(0, 0, 0, 0);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                big |= (uint32_t)(v[u].x >= gf::P) | (uint32_t)(v[u].y >= gf::P) | (uint32_t)(v[u].z >= gf::P) | (uint32_t)(v[u].w >= gf::P);
                mad3(a0, a1, a2, v[u].x, wa[u].x, wa[u].y);
                mad3(a0, a1, a2, v[u].y, wa[u].z, wa[u].w);
                mad3(a0, a1, a2, v[u].z, wb[u].x, wb[u].y);
                mad3(a0, a1, a2, v[u].w, wb[u].z, wb[u].w);
            }
            if ((++batches & 255u) == 0) {  // 16 products per batch: 4096 since the last fold
                a0 = fold64(a0);
                a1 = fold64(a1);
                a2 = fold64(a2);
            }
        }
    } else {
        uint32_t steps = 0;
        for (uint32_t w = lane; w < S; w += 64u) {
            const uint32_t v = blk[w];
            const uint2 q = wt[w];
            big |= (uint32_t)(v >= gf::P);
            mad3(a0, a1, a2, v, q.x, q.y);
            if ((++steps & 4095u) == 0) {
                a0 = fold64(a0);
                a1 = fold64(a1);
                a2 = fold64(a2);
            }
        }
    }
    // lane sums < p, wave sums < 2^38
    a0 = reduce64(a0);
    a1 = reduce64(a1);
    a2 = reduce64(a2);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a0 += __shfl_xor(a0, o, 64);
        a1 += __shfl_xor(a1, o, 64);
        a2 += __shfl_xor(a2, o, 64);
    }
    any_big = __any(big != 0);
    f[0] = reduce64(a0);
    f[1] = reduce64(a1);
    f[2] = reduce64(a2);
}

// pos[j] of a block the caller named absent (fastecc_scrub_erasures) carries this mark: the block is not read
constexpr uint32_t ABSENT = 0x80000000u;

// One wave per block (blocks wave, wave + waves, ...).  F[pos[j] * 4 + c] receives the block's fingerprint c; a block with a word >= p
// is appended to bad[1 ..] (bad[0] counts them).  An absent block is skipped (j and pos[j] are wave-uniform: no lane diverges) and its
// F keeps whatever an earlier call left: the weigh pass multiplies it by a locator that is zero there.
template <bool VEC>
__global__ __launch_bounds__(256) void fingerprint_kernel(const uint32_t* __restrict__ data, const uint32_t* __restrict__ parity, uint32_t k_blocks,
                                                          uint32_t n_blocks, uint32_t S, const uint2* __restrict__ wt, const uint32_t* __restrict__ pos,
                                                          uint32_t* __restrict__ F, uint32_t* __restrict__ bad, uint32_t bad_cap)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t j = wave; j < n_blocks; j += waves) {
        const uint32_t u = pos[j];
        if (u & ABSENT) continue;
        const uint32_t* blk = j < k_blocks ? data + (size_t)j * S : parity + (size_t)(j - k_blocks) * S;
        uint32_t fp[R];
        bool any_big;
        block_fingerprint<VEC>(blk, S, wt, lane, fp, any_big);
        if (lane == 0) {
            uint32_t* f = F + (size_t)u * RW;
            f[0] = fp[0];
            f[1] = fp[1];
            f[2] = fp[2];
            if (any_big) {
                const uint32_t slot = atomicAdd(bad, 1u);
                if (slot < bad_cap) bad[1 + slot] = j;
            }
        }
    }
}

// fastecc_verify_batch: the same per block over the B stripes [b0, b0 + B) of a batch, global block g = b * n + j (stripe b - b0 of the chunk, block j;
// both wave-uniform).  Fingerprint c of that block, times the locator of the fixed and the named erasures at its position (lfix, null: 1), lands in
// F[pos[j] * row + (b - b0) * 4 + c] — the chunk's stripes are word columns of one fingerprint stripe of NC rows.  A block with a word >= p
// sets flag[b] (a plain store of 1: idempotent, no atomics).  An absent block (pos[j] marked; wave-uniform) is not read and its entry is stored
// as zero: nothing multiplies F by the locator afterwards, and the entry may hold another call's or another pattern's value.
// At most 80 VGPRs: six waves per SIMD, the grid the host launches all resident.
// LIST (batched location and the closing verify of fastecc_correct_batch): the chunk is B entries of a list of stripes of the
// pool — list[bl] names the stripe whose blocks are read (wave-uniform like b), while the fingerprint columns, flag[] and big[] are addressed by the
// position bl in the chunk (the host passes all three arrays from the chunk's first entry on; b0 is not used).  big[bl] = 1 records that a present
// block of the entry held a word >= p (flag[bl] is set as well).  The list form needs two registers more than 80 in its vector form: five waves per
// SIMD there (82 VGPRs, no scratch) instead of a spilled pointer; its grid is sized to match (chunk_pass).
template <bool VEC, bool LIST = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(LIST ? 5 : 6))) void fingerprint_batch_kernel(const uint32_t* __restrict__ data, const uint32_t* __restrict__ parity, uint32_t k_blocks,
                                                                uint32_t n_blocks, uint32_t S, uint64_t b0, uint64_t B, const uint2* __restrict__ wt,
                                                                const uint32_t* __restrict__ pos, const uint32_t* __restrict__ lfix, uint32_t* __restrict__ F,
                                                                uint64_t row, uint8_t* __restrict__ flag, const uint64_t* __restrict__ list,
                                                                uint8_t* __restrict__ big)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint64_t waves = (gridDim.x * blockDim.x) >> 6;
    const uint64_t total = B * n_blocks;
    const uint64_t m_blocks = n_blocks - k_blocks;
    for (uint64_t g = wave; g < total; g += waves) {
        const uint64_t bl = g / n_blocks;
        const uint32_t j = (uint32_t)(g - bl * n_blocks);
        const uint32_t entry = __builtin_amdgcn_readfirstlane((uint32_t)bl);  // (LIST: a chunk has at most 2^16 entries)
        const uint64_t b = LIST ? list[entry] : b0 + bl;
        const uint32_t u = pos[j];
        if (u & ABSENT) {
            if (lane == 0) *reinterpret_cast<uint4*>(F + (uint64_t)(u & ~ABSENT) * row + bl * RW) = make_uint4(0, 0, 0, 0);
            continue;
        }
        const uint32_t* blk = j < k_blocks ? data + (b * k_blocks + j) * S : parity + (b * m_blocks + (j - k_blocks)) * S;
        uint32_t fp[R];
        bool any_big;
        block_fingerprint<VEC>(blk, S, wt, lane, fp, any_big);
        if (lane == 0) {
            const uint32_t l = lfix ? lfix[u] : 1u;
            uint32_t* f = F + (uint64_t)u * row + bl * RW;
            f[0] = gf::mul(fp[0], l);
            f[1] = gf::mul(fp[1], l);
            f[2] = gf::mul(fp[2], l);
            if (any_big) {
                if (LIST) {
                    flag[entry] = 1;
                    big[entry] = 1;
                } else {
                    flag[b] = 1;
                }
            }
        }
    }
}

// fastecc_verify_batch_set: fingerprint_batch_kernel's pass with a pattern PER STRIPE.  q = pattern_of[b] is read once per wave and
// made uniform by readfirstlane, so q, pos_set[q * n + j] and the absent test are scalar loads and one scalar branch, as above.  A stripe with
// q = FASTECC_PATTERN_NONE reads nothing and stores a zero entry at every one of its n positions (through pattern 0's position table: a set has at least
// one pattern, and the mark is masked off); an absent block stores its zero entry; a present one F * lset[q * NC + u], the fixed and the pattern's own
// erasures' locator at its position.  Every (stripe, block) entry of the chunk is stored by every call: nothing an earlier call, set or pattern left in F
// is read.  Six waves per SIMD (at most 80 VGPRs), the grid all resident, as for the batch kernel.
template <bool VEC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6))) void fingerprint_set_kernel(const uint32_t* __restrict__ data, const uint32_t* __restrict__ parity, uint32_t k_blocks,
                                                              uint32_t n_blocks, uint32_t S, uint64_t b0, uint64_t B, const uint2* __restrict__ wt,
                                                              const uint32_t* __restrict__ pattern_of, const uint32_t* __restrict__ pos_set,
                                                              const uint32_t* __restrict__ lset, uint32_t NC, uint32_t* __restrict__ F, uint64_t row,
                                                              uint8_t* __restrict__ flag)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint64_t waves = (gridDim.x * blockDim.x) >> 6;
    const uint64_t total = B * n_blocks;
    const uint64_t m_blocks = n_blocks - k_blocks;
    for (uint64_t g = wave; g < total; g += waves) {
        const uint64_t bl = g / n_blocks;
        const uint32_t j = (uint32_t)(g - bl * n_blocks);
        const uint64_t b = b0 + bl;
        const uint32_t q = __builtin_amdgcn_readfirstlane(pattern_of[b]);
        const bool none = q == FASTECC_PATTERN_NONE;
        const uint32_t u = pos_set[(none ? 0u : q) * n_blocks + j];
        if (none || (u & ABSENT)) {
            if (lane == 0) *reinterpret_cast<uint4*>(F + (uint64_t)(u & ~ABSENT) * row + bl * RW) = make_uint4(0, 0, 0, 0);
            continue;
        }
        const uint32_t* blk = j < k_blocks ? data + (b * k_blocks + j) * S : parity + (b * m_blocks + (j - k_blocks)) * S;
        uint32_t fp[R];
        bool any_big;
        block_fingerprint<VEC>(blk, S, wt, lane, fp, any_big);
        if (lane == 0) {
            const uint32_t l = lset[q * NC + u];
            uint32_t* f = F + (uint64_t)u * row + bl * RW;
            f[0] = gf::mul(fp[0], l);
            f[1] = gf::mul(fp[1], l);
            f[2] = gf::mul(fp[2], l);
            if (any_big) flag[b] = 1;
        }
    }
}

// Batched location under a pattern per stripe: fingerprint_set_kernel's body with the LIST form's addressing.  The chunk is B
// entries of a list of stripes of the pool: list[entry] names the stripe whose blocks are read and whose pattern q = pattern_of[stripe] holds (both
// wave-uniform: scalar loads, q through readfirstlane; pattern_of is the whole call's array, indexed by stripe), while the fingerprint columns, flag[]
// and big[] are addressed by the position in the chunk (the host passes the three from the chunk's first entry on).  The host lists only stripes with
// a pattern (q < P).  A present block stores F * lset[q * NC + u] and an absent one its zero entry, so every (entry, block) of the chunk is stored by
// every launch and nothing an earlier call left in F is read; big[entry] = 1 when a present block held a word >= p (flag[entry] as well).
// Five waves per SIMD with the grid to match, as for the list kernel: the vector form needs more than 80 VGPRs.
template <bool VEC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void fingerprint_set_list_kernel(const uint32_t* __restrict__ data, const uint32_t* __restrict__ parity, uint32_t k_blocks,
                                                                   uint32_t n_blocks, uint32_t S, uint64_t B, const uint2* __restrict__ wt,
                                                                   const uint32_t* __restrict__ pattern_of, const uint32_t* __restrict__ pos_set,
                                                                   const uint32_t* __restrict__ lset, uint32_t NC, uint32_t* __restrict__ F, uint64_t row,
                                                                   uint8_t* __restrict__ flag, const uint64_t* __restrict__ list, uint8_t* __restrict__ big)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint64_t waves = (gridDim.x * blockDim.x) >> 6;
    const uint64_t total = B * n_blocks;
    const uint64_t m_blocks = n_blocks - k_blocks;
    for (uint64_t g = wave; g < total; g += waves) {
        const uint64_t bl = g / n_blocks;
        const uint32_t j = (uint32_t)(g - bl * n_blocks);
        const uint32_t entry = __builtin_amdgcn_readfirstlane((uint32_t)bl);  // (a chunk has at most 2^16 entries)
        const uint64_t b = list[entry];
        const uint32_t q = __builtin_amdgcn_readfirstlane(pattern_of[b]);
        const uint32_t u = pos_set[q * n_blocks + j];
        if (u & ABSENT) {
            if (lane == 0) *reinterpret_cast<uint4*>(F + (uint64_t)(u & ~ABSENT) * row + bl * RW) = make_uint4(0, 0, 0, 0);
            continue;
        }
        const uint32_t* blk = j < k_blocks ? data + (b * k_blocks + j) * S : parity + (b * m_blocks + (j - k_blocks)) * S;
        uint32_t fp[R];
        bool any_big;
        block_fingerprint<VEC>(blk, S, wt, lane, fp, any_big);
        if (lane == 0) {
            const uint32_t l = lset[q * NC + u];
            uint32_t* f = F + (uint64_t)u * row + bl * RW;
            f[0] = gf::mul(fp[0], l);
            f[1] = gf::mul(fp[1], l);
            f[2] = gf::mul(fp[2], l);
            if (any_big) {
                flag[entry] = 1;
                big[entry] = 1;
            }
        }
    }
}

// out[u] = base[u] (or 1) * prod_i (w^u - roots[i]); WITH_F: G[u][c] = F[u][c] * that instead (all plain representatives)
template <bool WITH_F>
__global__ __launch_bounds__(256) void locator_kernel(const uint32_t* __restrict__ base, const uint32_t* __restrict__ roots, uint32_t nroots,
                                                      const uint32_t* __restrict__ wpow, uint32_t NC, const uint32_t* __restrict__ F, uint32_t* __restrict__ out)
{
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= NC) return;
    const uint32_t x = wpow[u];
    uint32_t v = base ? base[u] : 1u;
    for (uint32_t i = 0; i < nroots; i++) v = gf::mul(v, gf::sub(x, roots[i]));
    if (!WITH_F) {
        out[u] = v;
        return;
    }
    const uint4 f = reinterpret_cast<const uint4*>(F)[u];
    reinterpret_cast<uint4*>(out)[u] = make_uint4(gf::mul(f.x, v), gf::mul(f.y, v), gf::mul(f.z, v), 0u);
}

// fastecc_scrub_erasures_set: locator_kernel<false> for every pattern of a set at once, one grid row per pattern q:
// out[q * NC + u] = base[u] (or 1) * prod (w^u - roots[i]), i in [off[q], off[q + 1])
__global__ __launch_bounds__(256) void locator_set_kernel(const uint32_t* __restrict__ base, const uint32_t* __restrict__ roots, const uint32_t* __restrict__ off,
                                                          const uint32_t* __restrict__ wpow, uint32_t NC, uint32_t* __restrict__ out)
{
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x, q = blockIdx.y;
    if (u >= NC) return;
    const uint32_t x = wpow[u];
    uint32_t v = base ? base[u] : 1u;
    for (uint32_t i = off[q], e = off[q + 1]; i < e; i++) v = gf::mul(v, gf::sub(x, roots[i]));
    out[(uint64_t)q * NC + u] = v;
}

// G holds the inverse transform in bit-reversed order (G[bitrev(m)] = NC * coefficient m).  Every coefficient m >= m_lo must vanish:
// flag[0] |= 1 otherwise; the first `gather` of them per column go to syn[c * gather + (m - m_lo)].
__global__ __launch_bounds__(256) void syndrome_kernel(const uint32_t* __restrict__ G, int lgc, uint32_t NC, uint32_t m_lo, uint32_t gather,
                                                       uint32_t* __restrict__ syn, uint32_t* __restrict__ flag)
{
    const uint32_t m = m_lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= NC) return;
    const uint32_t slot = __brev(m) >> (32 - lgc);
    const uint4 g = reinterpret_cast<const uint4*>(G)[slot];
    if ((g.x | g.y | g.z) != 0) atomicOr(flag, 1u);
    const uint32_t i = m - m_lo;
    if (i < gather) {
        syn[i] = g.x;
        syn[gather + i] = g.y;
        syn[2 * gather + i] = g.z;
    }
}

// fastecc_verify_batch: G as above with the chunk's B stripes as word columns (row words per position); item i <-> stripe b = i % B of the chunk,
// coefficient m = m_lo + i / B.  Any non-zero coefficient m >= m_lo in one of stripe b's three columns sets flag[b0 + b].
__global__ __launch_bounds__(256) void syndrome_batch_kernel(const uint32_t* __restrict__ G, int lgc, uint32_t NC, uint32_t m_lo, uint64_t row, uint32_t B,
                                                             uint64_t b0, uint8_t* __restrict__ flag)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (NC - m_lo) * B) return;
    const uint32_t b = i % B, m = m_lo + i / B;
    const uint32_t slot = __brev(m) >> (32 - lgc);
    const uint4 g = *reinterpret_cast<const uint4*>(G + (uint64_t)slot * row + (uint64_t)b * RW);
    if ((g.x | g.y | g.z) != 0) flag[b0 + b] = 1;
}

// fastecc_verify_batch_set: syndrome_batch_kernel's item mapping from m_lo = the smallest bound of the set on; stripe b0 + b checks the coefficients from its
// own pattern's bound mlo_set[pattern_of[b0 + b]] = N + fixed + w on (the w below it are legitimately non-zero), a FASTECC_PATTERN_NONE stripe none
__global__ __launch_bounds__(256) void syndrome_set_kernel(const uint32_t* __restrict__ G, int lgc, uint32_t NC, uint32_t m_lo, uint64_t row, uint32_t B,
                                                           uint64_t b0, const uint32_t* __restrict__ pattern_of, const uint32_t* __restrict__ mlo_set,
                                                           uint8_t* __restrict__ flag)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (NC - m_lo) * B) return;
    const uint32_t b = i % B, m = m_lo + i / B;
    const uint32_t q = pattern_of[b0 + b];
    if (q == FASTECC_PATTERN_NONE || m < mlo_set[q]) return;
    const uint32_t slot = __brev(m) >> (32 - lgc);
    const uint4 g = *reinterpret_cast<const uint4*>(G + (uint64_t)slot * row + (uint64_t)b * RW);
    if ((g.x | g.y | g.z) != 0) flag[b0 + b] = 1;
}

// Batched location: all avail = NC - m_lo coefficients from m_lo on of the chunk's B entries, by entry and column:
// syn[(b * 3 + c) * avail + i] = NC * coefficient m_lo + i of column c of entry b (item = i * B + b, as above)
__global__ __launch_bounds__(256) void syndrome_gather_kernel(const uint32_t* __restrict__ G, int lgc, uint32_t m_lo, uint32_t avail, uint64_t row, uint32_t B,
                                                              uint32_t* __restrict__ syn)
{
    const uint32_t item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= avail * B) return;
    const uint32_t b = item % B, i = item / B;
    const uint32_t slot = __brev(m_lo + i) >> (32 - lgc);
    const uint4 g = *reinterpret_cast<const uint4*>(G + (uint64_t)slot * row + (uint64_t)b * RW);
    uint32_t* o = syn + (uint64_t)b * R * avail + i;
    o[0] = g.x;
    o[avail] = g.y;
    o[2 * (uint64_t)avail] = g.z;
}

// Batched location under a pattern per stripe: syndrome_set_kernel's item mapping from m_lo = the set's smallest bound on, over the
// chunk's B list entries.  Entry b (stripe list[b], pattern q = pattern_of[list[b]]) keeps the coefficients from its own bound mlo_set[q] on:
// syn[(b * 3 + c) * stride + (m - mlo_set[q])]; the ones below it are legitimately non-zero and are not stored, and an entry with more than `stride`
// coefficients (the host lists none) stores only the first `stride`.
__global__ __launch_bounds__(256) void syndrome_gather_set_kernel(const uint32_t* __restrict__ G, int lgc, uint32_t NC, uint32_t m_lo, uint64_t row, uint32_t B,
                                                                  const uint64_t* __restrict__ list, const uint32_t* __restrict__ pattern_of,
                                                                  const uint32_t* __restrict__ mlo_set, uint32_t stride, uint32_t* __restrict__ syn)
{
    const uint32_t item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= (NC - m_lo) * B) return;
    const uint32_t b = item % B, m = m_lo + item / B;
    const uint32_t lo = mlo_set[pattern_of[list[b]]];
    if (m < lo || m - lo >= stride) return;
    const uint32_t slot = __brev(m) >> (32 - lgc);
    const uint4 g = *reinterpret_cast<const uint4*>(G + (uint64_t)slot * row + (uint64_t)b * RW);
    uint32_t* o = syn + (uint64_t)b * R * stride + (m - lo);
    o[0] = g.x;
    o[stride] = g.y;
    o[2 * (uint64_t)stride] = g.z;
}

// Batched location: thread (e, u) evaluates the locator of entry e — lambda[e * stride + 0 .. L[e]] — at w^u; a root is appended to entry e's own list
// found[e * (cap + 1) + 1 ..] (found[e * (cap + 1)] counts all of them, the list keeps the first cap)
__global__ __launch_bounds__(256) void root_search_batch_kernel(const uint32_t* __restrict__ lambda, const uint32_t* __restrict__ Ls, uint32_t stride,
                                                                const uint32_t* __restrict__ wpow, uint32_t NC, uint32_t entries, uint32_t* __restrict__ found,
                                                                uint32_t cap)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= entries * NC) return;
    const uint32_t e = t / NC, u = t - e * NC;
    const uint32_t* l = lambda + (uint64_t)e * stride;
    const uint32_t L = Ls[e];
    const uint32_t x = wpow[u];
    uint32_t acc = l[L];
    for (int i = (int)L - 1; i >= 0; i--) acc = gf::add(gf::mul(acc, x), l[i]);
    if (acc == 0) {
        uint32_t* f = found + (uint64_t)e * (cap + 1);
        const uint32_t slot = atomicAdd(f, 1u);
        if (slot < cap) f[1 + slot] = u;
    }
}

// Lambda(w^u) == 0 -> u appended to found[1 ..] (found[0] counts)
__global__ __launch_bounds__(256) void root_search_kernel(const uint32_t* __restrict__ lambda, uint32_t L, const uint32_t* __restrict__ wpow, uint32_t NC,
                                                          uint32_t* __restrict__ found, uint32_t cap)
{
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= NC) return;
    const uint32_t x = wpow[u];
    uint32_t acc = lambda[L];
    for (int i = (int)L - 1; i >= 0; i--) acc = gf::add(gf::mul(acc, x), lambda[i]);
    if (acc == 0) {
        const uint32_t slot = atomicAdd(found, 1u);
        if (slot < cap) found[1 + slot] = u;
    }
}

__global__ __launch_bounds__(256) void powers_kernel(uint32_t* __restrict__ wpow, uint32_t w, uint32_t count)
{
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= count) return;
    uint32_t r = 1, b = w;
    for (uint32_t e = u; e; e >>= 1) {
        if (e & 1u) r = gf::mul(r, b);
        b = gf::mul(b, b);
    }
    wpow[u] = r;
}

}  // namespace

}  // namespace fastecc
