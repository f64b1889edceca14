// scrub.hip — error detection and location: fastecc_verify, fastecc_locate_errors, fastecc_correct and the batched fastecc_verify_batch,
// fastecc_correct_batch, fastecc_locate_errors_batch (include/fastecc.h).
//
// The erasure decoder (decode.hip) acts on losses the caller names.  Here the corrupted blocks are found first.  Every code of the
// library is f (degree < N) on a subset of the NC-th roots of unity, NC = N << e, position u <-> w^u: data block i at i << e, parity at
// the positions code_parity_position (internal.hpp) gives, zero-extended data blocks are known zeros, positions that hold no block are
// fixed erasures.  With l the locator of the erased positions, p = f * l has degree < N + |erased| (the decoder's identity), so the
// coefficients of the inverse transform of c[u] l(w^u) (0 at erased positions) above that vanish for a codeword.  For a received word
// c + e they are S_m = sum_u e_u l(w^u) w^(-um) / NC: power sums in the locators X_u = w^(-u) — the syndromes of classic RS decoding,
// n - k - b of them with b further erasures.
//
// Blocks are long (kilobytes), so the decoding runs on a FINGERPRINT of the codeword: per block j and column c, F_c[j] = sum_w
// rho_c[w] r_j[w] mod p with small random weights (rho < 2^20, splitmix64 of the seed), R = 3 columns.  F is linear, so the
// fingerprints of a codeword are a codeword of the same code (of the polynomial sum_w rho_c[w] f_w) and the fingerprints of a corrupted
// block differ from the clean ones except with probability <= 2^-20 per column.  The pass that reads the codeword once is the only
// part that scales with the stripe; the rest works on NC x 4 words:
//   fingerprint_kernel  : one wave per block, dwordx4 loads, v_mad_u64_u32 into 64-bit sums (a product is < 2^52), a per-block
//                         "word >= p" flag (those blocks are certainly corrupt: known erasures), F written in position order;
//   syndromes           : F times l(w^u) (the fixed erasures' values, cached per context, times the further erasures' factors),
//                         the library's stand-alone inverse transform of NC points (transform_bitrev), and a pass that checks
//                         every coefficient above the degree bound for zero and gathers the first 2 locate_max of each column;
//   Berlekamp-Massey    : on the host, per column; the longest LFSR is the locator Lambda(x) = prod (1 - X_u x);
//   root search         : Lambda(w^u) by Horner at every position on the device;
//   confirmation        : the syndromes once more with the located positions erased must all vanish, in every column.
// fastecc_correct then hands the located blocks to fastecc_decode_prepare + fastecc_repair.
// fastecc_scrub_erasures names blocks that are absent: the fingerprint kernels skip them, their locator joins the
// fixed erasures' in a table cached per pattern, w fewer syndromes are checked, and fastecc_correct rebuilds them with the located blocks.
// fastecc_verify_batch / _correct_batch run the verify over many stripes at once: the stripe index becomes extra word columns of
// the fingerprint stripe, so one transform serves a whole chunk of stripes (fingerprint_batch_kernel, syndrome_batch_kernel, verify_batch_locked).
// fastecc_locate_errors_batch and the grouped path of fastecc_correct_batch run the same passes over a LIST of stripes of the pool:
// all syndromes of the flagged stripes gathered at once (syndrome_gather_kernel), Berlekamp-Massey per stripe on the host, one root search for all
// locators (root_search_batch_kernel), then one fastecc_decode_prepare and one list-form repair (decode.hip repair_list) per distinct set of lost blocks.
#include <algorithm>
#include <map>
#include <memory>
#include <vector>

#include "drivers.hpp"

namespace fastecc {

namespace {

constexpr int R = 3;   // fingerprint columns (the transform stripe has 4 words per position; the 4th stays zero)
constexpr int RW = 4;  // words per position of the fingerprint stripe

uint64_t splitmix64(uint64_t& s)
{
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

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
// SIMD there (82 VGPRs, no scratch) instead of a spilled pointer; its grid is sized to match (list_chunk).
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

// fastecc_scrub_erasures_set: P patterns of absent blocks, their tables side by side
struct ScrubSet {
    uint64_t P = 0;
    std::vector<std::vector<uint32_t>> absent;    // per pattern: the absent blocks' codeword indices, increasing
    std::vector<std::vector<uint8_t>> is_absent;  // per pattern: n flags
    std::vector<uint32_t> mlo;                    // per pattern: N + fixed + w, the first coefficient that must vanish
    uint32_t mlo_min = 0;
    uint32_t* d_pos = nullptr;                    // P x n words: d_pos with ABSENT set at the pattern's absent blocks
    uint32_t* d_l = nullptr;                      // P x NC words: d_lfix (or 1) times the locator of the pattern's absent positions at w^u
    uint32_t* d_mlo = nullptr;                    // P words: mlo
    ~ScrubSet()
    {
        for (void* p : {(void*)d_pos, (void*)d_l, (void*)d_mlo})
            if (p) (void)hipFree(p);
    }
};

struct ScrubState {
    uint64_t N = 0, NC = 0, n = 0, k = 0;  // transform length of the code, positions, blocks (user k + user m), data blocks
    int lgc = 0;
    uint64_t fixed = 0;                     // positions that hold no block (fixed erasures)
    std::vector<uint32_t> pos;              // block -> position
    std::vector<uint32_t> block_at;         // position -> block, ~0u if none (fixed erasure or known-zero data block)
    fastecc_ctx* ntt = nullptr;             // stand-alone transform of NC points, 4 words per position
    uint32_t* d_pos = nullptr;              // n words
    uint32_t* d_wpow = nullptr;             // NC words: w^u
    uint32_t* d_lfix = nullptr;             // NC words: the fixed erasures' locator at w^u (null: none)
    uint32_t* d_F = nullptr;                // NC x 4 words: fingerprints by position (zero where no block is read)
    uint32_t* d_G = nullptr;                // NC x 4 words: weighted fingerprints, transformed in place
    uint32_t* d_small = nullptr;            // counters and lists: [bad: 1 + n], [flag: 1], [found: 1 + cap_found], syndromes, lambda, roots
    uint64_t small_words = 0;
    uint2* d_weights = nullptr;             // S packed weights of the current seed
    uint64_t weights_seed = 0;
    bool weights_valid = false;
    // fastecc_verify_batch (built at its first call): a chunk of up to batch_cap stripes as word columns of one fingerprint stripe
    fastecc_ctx* ntt_batch = nullptr;       // stand-alone transform of NC points over rows of 4 x batch_cap words
    uint64_t batch_cap = 0;
    uint32_t* d_FB = nullptr;               // NC x 4 batch_cap words: weighted fingerprints by position (zero where no block is read)
    uint32_t* d_GB = nullptr;               // their transform
    uint8_t* d_flag = nullptr;              // one byte per stripe of the call: 1 = inconsistent
    uint64_t flag_cap = 0;
    // fastecc_scrub_erasures: the blocks the caller named absent (none: empty / null)
    std::vector<uint32_t> absent;           // their codeword indices, increasing
    std::vector<uint8_t> is_absent;         // n flags
    uint32_t* d_pos_named = nullptr;        // n words: d_pos with ABSENT set at those blocks
    uint32_t* d_lnamed = nullptr;           // NC words: d_lfix (or 1) times the locator of their positions at w^u
    // batched location and the list forms, all grow-only
    uint64_t* d_list = nullptr;             // the stripes a list pass runs over
    uint8_t* d_lflag = nullptr;             // per list entry: [0, list_cap) inconsistent, [list_cap, 2 list_cap) a present block held a word >= p
    uint64_t list_cap = 0;
    uint32_t* d_loc = nullptr;              // one chunk's syndromes, then its locators, their lengths and the found lists
    uint64_t loc_words = 0;
    // fastecc_scrub_erasures_set: the pattern set (null: none) and the device copy of a call's pattern_of (grow-only)
    ScrubSet* set = nullptr;
    uint32_t* d_pattern_of = nullptr;
    uint64_t pattern_cap = 0;
};

void destroy_scrub_state(ScrubState* s)
{
    if (!s) return;
    if (s->ntt) fastecc_destroy(s->ntt);
    if (s->ntt_batch) fastecc_destroy(s->ntt_batch);
    for (void* p : {(void*)s->d_pos, (void*)s->d_wpow, (void*)s->d_lfix, (void*)s->d_F, (void*)s->d_G, (void*)s->d_small, (void*)s->d_weights, (void*)s->d_FB,
                    (void*)s->d_GB, (void*)s->d_flag, (void*)s->d_pos_named, (void*)s->d_lnamed, (void*)s->d_list, (void*)s->d_lflag, (void*)s->d_loc, (void*)s->d_pattern_of})
        if (p) (void)hipFree(p);
    delete s->set;
    delete s;
}

namespace {

// What a scrub call erases up front besides the known-bad blocks: the position table its fingerprint pass reads, the locator of
// those erasures at every position (null: 1), the number of named ones (the fixed ones are counted by ScrubState::fixed), their
// codeword indices and the n flags (both null when w == 0).  A view of the single fastecc_scrub_erasures pattern (erasures) or of one
// pattern of the set (set_view); it points into the scrub state and lives as long as the context's lock is held.
struct Erasures {
    const uint32_t* d_pos;
    const uint32_t* d_loc;
    uint64_t w;
    const std::vector<uint32_t>* absent;
    const std::vector<uint8_t>* is_absent;
};

Erasures erasures(const ScrubState* s, bool named)
{
    if (named && !s->absent.empty()) return {s->d_pos_named, s->d_lnamed, s->absent.size(), &s->absent, &s->is_absent};
    return {s->d_pos, s->d_lfix, 0, nullptr, nullptr};
}

// pattern q of the set: its rows of the set's tables (the locator row is lfix, or 1, for a pattern that names nothing)
Erasures set_view(const ScrubState* s, uint32_t q)
{
    const ScrubSet* t = s->set;
    const uint64_t w = t->absent[q].size();
    return {t->d_pos + (uint64_t)q * s->n, t->d_l + (uint64_t)q * s->NC, w, w ? &t->absent[q] : nullptr, w ? &t->is_absent[q] : nullptr};
}

int scrub_args(fastecc_ctx* c, const void* data, const void* parity, int mem_kind)
{
    if (!c || !data || !parity || (((uintptr_t)data | (uintptr_t)parity) & 3u)) return FASTECC_E_INVAL;
    if (mem_kind != FASTECC_MEM_HOST && mem_kind != FASTECC_MEM_DEVICE && mem_kind != FASTECC_MEM_HOST_PINNED) return FASTECC_E_INVAL;
    if (c->sharded || c->p61 || c->field != FASTECC_FIELD_GF_FFF00001) return FASTECC_E_UNSUPPORTED;
    if (c->q > 1) return FASTECC_E_UNSUPPORTED;  // mixed radix: the syndromes would need the decoder's mixed transforms in natural order
    if (c->ld != c->S) return FASTECC_E_UNSUPPORTED;
    if (mem_kind != FASTECC_MEM_DEVICE) return FASTECC_E_UNSUPPORTED;
    return FASTECC_OK;
}

// The context's geometry, position map, w^u table and fixed-erasure locator (once per context; synchronous).
int scrub_state(fastecc_ctx* c, ScrubState** out)
{
    if (c->scrub) {
        *out = c->scrub;
        return FASTECC_OK;
    }
    ScrubState* s = new (std::nothrow) ScrubState();
    if (!s) return FASTECC_E_NOMEM;
    c->scrub = s;  // (partially built state is freed with the context; a failed build is retried from scratch)
    auto fail = [&](int rc) {
        destroy_scrub_state(s);
        c->scrub = nullptr;
        return rc;
    };
    int e = 1;
    while ((1 << e) < c->cosets + 1) e++;
    s->N = c->N;
    s->NC = c->N << e;
    s->lgc = c->n + e;
    s->k = c->K;
    s->n = c->K + c->Mu;
    if (s->NC > (1ull << 20) || s->NC < 4) return fail(FASTECC_E_UNSUPPORTED);
    auto parity_position = [&](uint64_t q) -> uint64_t { return code_parity_position(c->N, e, c->fold, c->cosets, q); };
    s->pos.resize(s->n);
    s->block_at.assign(s->NC, ~0u);
    std::vector<uint8_t> held(s->NC, 0);
    for (uint64_t i = 0; i < s->N; i++) held[i << e] = 1;  // data positions, the zero-extended ones included (known zeros)
    for (uint64_t i = 0; i < s->k; i++) s->pos[i] = (uint32_t)(i << e);
    for (uint64_t q = 0; q < c->Mu; q++) s->pos[s->k + q] = (uint32_t)parity_position(q);
    for (uint64_t j = 0; j < s->n; j++) {
        held[s->pos[j]] = 1;
        s->block_at[s->pos[j]] = (uint32_t)j;
    }
    std::vector<uint32_t> fixed_roots;
    const uint32_t w = gf::h_root((uint32_t)s->NC);
    for (uint64_t u = 0; u < s->NC; u++)
        if (!held[u]) fixed_roots.push_back(gf::h_pow(w, u));
    s->fixed = fixed_roots.size();
    if (s->N + s->fixed + (s->n - s->k) != s->NC) return fail(FASTECC_E_DEVICE);  // (the layout is inconsistent: cannot happen)

    const int rc = create_ntt_ctx(&s->ntt, s->lgc, 4 * RW, c->device);
    if (rc != FASTECC_OK) return fail(rc);
    const uint64_t NC = s->NC;
    hipError_t he = hipSuccess;
    auto grid = [](uint64_t items) { return dim3((unsigned)((items + 255) / 256)); };
    if ((he = hipMalloc((void**)&s->d_pos, s->n * 4)) != hipSuccess || (he = hipMalloc((void**)&s->d_wpow, NC * 4)) != hipSuccess ||
        (he = hipMalloc((void**)&s->d_F, NC * RW * 4)) != hipSuccess || (he = hipMalloc((void**)&s->d_G, NC * RW * 4)) != hipSuccess)
        return fail(hip_fail(he, "hipMalloc"));
    if ((he = hipMemcpy(s->d_pos, s->pos.data(), s->n * 4, hipMemcpyHostToDevice)) != hipSuccess) return fail(hip_fail(he, "hipMemcpy"));
    // positions no block is read from (fixed erasures, known-zero data blocks) keep fingerprint 0 for good
    if ((he = hipMemset(s->d_F, 0, NC * RW * 4)) != hipSuccess) return fail(hip_fail(he, "hipMemset"));
    hipLaunchKernelGGL(powers_kernel, grid(NC), dim3(256), 0, nullptr, s->d_wpow, w, (uint32_t)NC);
    if ((he = hipGetLastError()) != hipSuccess) return fail(hip_fail(he, "powers_kernel"));
    if (!fixed_roots.empty()) {
        uint32_t* d_roots = nullptr;
        if ((he = hipMalloc((void**)&s->d_lfix, NC * 4)) != hipSuccess || (he = hipMalloc((void**)&d_roots, fixed_roots.size() * 4)) != hipSuccess)
            return fail(hip_fail(he, "hipMalloc"));
        he = hipMemcpy(d_roots, fixed_roots.data(), fixed_roots.size() * 4, hipMemcpyHostToDevice);
        if (he == hipSuccess) {
            hipLaunchKernelGGL(locator_kernel<false>, grid(NC), dim3(256), 0, nullptr, nullptr, d_roots, (uint32_t)fixed_roots.size(), s->d_wpow,
                               (uint32_t)NC, nullptr, s->d_lfix);
            he = hipGetLastError();
        }
        if (he == hipSuccess) he = hipDeviceSynchronize();
        (void)hipFree(d_roots);
        if (he != hipSuccess) return fail(hip_fail(he, "locator_kernel"));
    }
    if ((he = hipDeviceSynchronize()) != hipSuccess) return fail(hip_fail(he, "hipDeviceSynchronize"));
    *out = s;
    return FASTECC_OK;
}

// The small buffer's layout for this call: bad list, flag, found list, gathered syndromes, lambda, extra roots
struct Small {
    uint32_t *bad, *flag, *found, *syn, *lambda, *roots;
    uint64_t bad_cap, found_cap, gather, roots_cap;
};

int small_buffers(ScrubState* s, uint32_t locate_max, Small* sm)
{
    const uint64_t m = s->n - s->k;
    sm->bad_cap = m + 1;
    sm->found_cap = (uint64_t)locate_max + 1;
    sm->gather = std::min<uint64_t>(2ull * locate_max, m);
    sm->roots_cap = m + 1;
    const uint64_t words = (1 + sm->bad_cap) + 1 + (1 + sm->found_cap) + R * std::max<uint64_t>(sm->gather, 1) + (locate_max + 1) + sm->roots_cap;
    if (words > s->small_words) {
        if (s->d_small) (void)hipFree(s->d_small);
        s->d_small = nullptr;
        s->small_words = 0;
        HIP_TRY(hipMalloc((void**)&s->d_small, words * 4));
        s->small_words = words;
    }
    uint32_t* p = s->d_small;
    sm->bad = p;
    p += 1 + sm->bad_cap;
    sm->flag = p;
    p += 1;
    sm->found = p;
    p += 1 + sm->found_cap;
    sm->syn = p;
    p += R * std::max<uint64_t>(sm->gather, 1);
    sm->lambda = p;
    p += locate_max + 1;
    sm->roots = p;
    return FASTECC_OK;
}

int upload_weights(fastecc_ctx* c, ScrubState* s, uint64_t seed, hipStream_t st)
{
    if (s->weights_valid && s->weights_seed == seed) return FASTECC_OK;
    std::vector<uint32_t> h(2 * c->S);
    uint64_t state = seed;
    for (uint64_t w = 0; w < c->S; w++) {
        const uint64_t x = splitmix64(state);
        const uint32_t r0 = (uint32_t)(x & 0xFFFFF), r1 = (uint32_t)((x >> 20) & 0xFFFFF), r2 = (uint32_t)((x >> 40) & 0xFFFFF);
        h[2 * w] = r0 | ((r2 & 0xFFFu) << 20);
        h[2 * w + 1] = r1 | ((r2 >> 12) << 20);
    }
    s->weights_valid = false;
    if (!s->d_weights) HIP_TRY(hipMalloc((void**)&s->d_weights, 2 * c->S * 4 + 16));
    HIP_TRY(hipStreamSynchronize(st));  // (the previous call's kernels are done: calls end with a synchronise; this one has enqueued nothing yet)
    HIP_TRY(hipMemcpy(s->d_weights, h.data(), 2 * c->S * 4, hipMemcpyHostToDevice));
    s->weights_seed = seed;
    s->weights_valid = true;
    return FASTECC_OK;
}

// The fingerprint pass over the blocks `er` does not name absent; those holding a word >= p come back sorted in `bad` (b > bad_cap - 1: *overflow).
int fingerprints(fastecc_ctx* c, ScrubState* s, const Small& sm, const Erasures& er, const uint32_t* data, const uint32_t* parity, uint64_t seed,
                 hipStream_t st, std::vector<uint32_t>& bad)
{
    int rc = upload_weights(c, s, seed, st);
    if (rc != FASTECC_OK) return rc;
    HIP_TRY(hipMemsetAsync(sm.bad, 0, 4, st));
    const bool vec = (c->S % 4) == 0 && (((uintptr_t)data | (uintptr_t)parity) & 15u) == 0;
    // every workgroup resident at once (6 waves per SIMD; its 72 VGPRs would fit a seventh): a grid-stride loop over the blocks without a tail wave of late groups
    const uint64_t groups = std::min<uint64_t>((s->n + 3) / 4, (uint64_t)c->cus * 6);
    {
        ProfScope ps(c, st, "fingerprint", (s->n - er.w) * c->S * 4);
        if (vec)
            hipLaunchKernelGGL(fingerprint_kernel<true>, dim3((unsigned)groups), dim3(256), 0, st, data, parity, (uint32_t)s->k, (uint32_t)s->n, (uint32_t)c->S,
                               s->d_weights, er.d_pos, s->d_F, sm.bad, (uint32_t)sm.bad_cap);
        else
            hipLaunchKernelGGL(fingerprint_kernel<false>, dim3((unsigned)groups), dim3(256), 0, st, data, parity, (uint32_t)s->k, (uint32_t)s->n, (uint32_t)c->S,
                               s->d_weights, er.d_pos, s->d_F, sm.bad, (uint32_t)sm.bad_cap);
        HIP_TRY(hipGetLastError());
    }
    uint32_t nb = 0;
    HIP_TRY(hipMemcpyAsync(&nb, sm.bad, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    bad.assign(std::min<uint64_t>(nb, sm.bad_cap), 0);
    if (!bad.empty()) HIP_TRY(hipMemcpy(bad.data(), sm.bad + 1, bad.size() * 4, hipMemcpyDeviceToHost));
    if (nb > bad.size()) bad.push_back(~0u);  // more than n - k: marks the overflow
    std::sort(bad.begin(), bad.end());
    return FASTECC_OK;
}

// Syndromes of the fingerprints with the fixed positions, the named ones of `er` (both through er.d_loc, the cached locator the product
// starts from) and then the positions `erased` erased: *nonzero = some coefficient above the degree bound is not zero in some column; the
// first `gather` of each column land in syn (host) if gather > 0.
int syndromes(fastecc_ctx* c, ScrubState* s, const Small& sm, const Erasures& er, const std::vector<uint32_t>& erased, uint64_t gather, hipStream_t st,
              bool* nonzero, std::vector<uint32_t>* syn)
{
    const uint64_t NC = s->NC;
    const uint64_t m_lo = s->N + s->fixed + er.w + erased.size();
    *nonzero = false;
    if (m_lo >= NC) return FASTECC_OK;  // nothing left to check: every set of n - k erasures explains any word
    if (erased.size() > sm.roots_cap) return FASTECC_E_INVAL;
    std::vector<uint32_t> pts(erased.size());
    const uint32_t w = gf::h_root((uint32_t)NC);
    for (size_t i = 0; i < erased.size(); i++) pts[i] = gf::h_pow(w, erased[i]);
    if (!pts.empty()) HIP_TRY(hipMemcpyAsync(sm.roots, pts.data(), pts.size() * 4, hipMemcpyHostToDevice, st));
    auto grid = [](uint64_t items) { return dim3((unsigned)((items + 255) / 256)); };
    {
        ProfScope ps(c, st, "scrub_weigh");
        hipLaunchKernelGGL(locator_kernel<true>, grid(NC), dim3(256), 0, st, er.d_loc, sm.roots, (uint32_t)pts.size(), s->d_wpow, (uint32_t)NC, s->d_F, s->d_G);
        HIP_TRY(hipGetLastError());
    }
    {
        ProfScope ps(c, st, "scrub_transform");
        const int rc = transform_bitrev(s->ntt, s->d_G, s->d_G, false, true, RW, st);
        if (rc != FASTECC_OK) return rc;
    }
    gather = std::min<uint64_t>(gather, NC - m_lo);
    HIP_TRY(hipMemsetAsync(sm.flag, 0, 4, st));
    {
        ProfScope ps(c, st, "scrub_syndromes");
        hipLaunchKernelGGL(syndrome_kernel, grid(NC - m_lo), dim3(256), 0, st, s->d_G, s->lgc, (uint32_t)NC, (uint32_t)m_lo, (uint32_t)gather, sm.syn, sm.flag);
        HIP_TRY(hipGetLastError());
    }
    uint32_t flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, sm.flag, 4, hipMemcpyDeviceToHost, st));
    if (syn) {
        syn->assign(R * gather, 0);
        if (gather) HIP_TRY(hipMemcpyAsync(syn->data(), sm.syn, R * gather * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    *nonzero = flag != 0;
    return FASTECC_OK;
}

// Berlekamp-Massey over GF(p): lambda = connection polynomial (lambda[0] = 1), returns its length L
int berlekamp_massey(const uint32_t* s, uint32_t count, std::vector<uint32_t>& C)
{
    C.assign(count + 1, 0);
    std::vector<uint32_t> B(count + 1, 0), T;
    C[0] = B[0] = 1;
    uint32_t L = 0, m = 1, b = 1;
    for (uint32_t n = 0; n < count; n++) {
        uint64_t d = s[n] % gf::P;
        for (uint32_t i = 1; i <= L; i++) d = (d + (uint64_t)C[i] * (s[n - i] % gf::P)) % gf::P;
        if (d == 0) {
            m++;
            continue;
        }
        const uint32_t coef = gf::h_mul((uint32_t)d, gf::h_inv(b));
        const bool grow = 2 * L <= n;
        if (grow) T = C;
        for (uint32_t i = 0; i + m <= count; i++) {
            if (!B[i]) continue;
            C[i + m] = (uint32_t)((C[i + m] + (uint64_t)(gf::P - gf::h_mul(coef, B[i]))) % gf::P);
        }
        if (grow) {
            L = n + 1 - L;
            B = T;
            b = (uint32_t)d;
            m = 1;
        } else {
            m++;
        }
    }
    C.resize(L + 1);
    return (int)L;
}

// fastecc_locate_errors on a locked context: the sorted codeword indices of the corrupted blocks, or FASTECC_E_UNCORRECTABLE.  The blocks
// `er` names absent are erased and not read; with the view of no pattern every block is read.
int locate(fastecc_ctx* c, ScrubState* s, const Erasures& er, const uint32_t* data, const uint32_t* parity, uint64_t seed, hipStream_t st,
           std::vector<uint32_t>& result, bool verify_only)
{
    int rc;
    const uint32_t tmax = (uint32_t)c->locate_max;
    Small sm;
    rc = small_buffers(s, tmax, &sm);
    if (rc != FASTECC_OK) return rc;
    std::vector<uint32_t> bad;
    rc = fingerprints(c, s, sm, er, data, parity, seed, st, bad);
    if (rc != FASTECC_OK) return rc;
    const uint64_t m = s->n - s->k;
    result.clear();
    if (verify_only) {  // fastecc_verify: any out-of-range word or any non-zero syndrome is an inconsistency
        if (!bad.empty()) {
            result.push_back(bad[0]);
            return FASTECC_OK;
        }
        bool nonzero = false;
        rc = syndromes(c, s, sm, er, {}, 0, st, &nonzero, nullptr);
        if (rc != FASTECC_OK) return rc;
        if (nonzero) result.push_back(~0u);
        return FASTECC_OK;
    }
    if (bad.size() + er.w > m) return FASTECC_E_UNCORRECTABLE;  // more known erasures than parity blocks
    std::vector<uint32_t> erased(bad.size());
    for (size_t i = 0; i < bad.size(); i++) erased[i] = s->pos[bad[i]];
    const uint64_t avail = m - er.w - bad.size();  // syndromes left after the known erasures
    bool nonzero = false;
    std::vector<uint32_t> syn;
    const uint64_t gather = std::min<uint64_t>(2ull * tmax, avail);
    rc = syndromes(c, s, sm, er, erased, gather, st, &nonzero, &syn);
    if (rc != FASTECC_OK) return rc;
    if (nonzero) {
        // the locator: the longest of the columns' LFSRs (a column may miss an error with probability <= 2^-20; the check below covers all)
        std::vector<uint32_t> lambda, cand;
        int L = 0;
        for (int col = 0; col < R; col++) {
            const int Lc = berlekamp_massey(syn.data() + col * gather, (uint32_t)gather, cand);
            if (Lc > L) {
                L = Lc;
                lambda = cand;
            }
        }
        if (L == 0 || (uint32_t)L > tmax || 2ull * (uint64_t)L > gather) return FASTECC_E_UNCORRECTABLE;
        HIP_TRY(hipMemcpyAsync(sm.lambda, lambda.data(), (L + 1) * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(sm.found, 0, 4, st));
        {
            ProfScope ps(c, st, "scrub_root_search");
            hipLaunchKernelGGL(root_search_kernel, dim3((unsigned)((s->NC + 255) / 256)), dim3(256), 0, st, sm.lambda, (uint32_t)L, s->d_wpow, (uint32_t)s->NC, sm.found,
                               (uint32_t)sm.found_cap);
            HIP_TRY(hipGetLastError());
        }
        uint32_t nf = 0;
        HIP_TRY(hipMemcpyAsync(&nf, sm.found, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (nf != (uint32_t)L) return FASTECC_E_UNCORRECTABLE;  // a locator splits into distinct roots at the code's positions, or it is no locator
        std::vector<uint32_t> roots(nf);
        HIP_TRY(hipMemcpy(roots.data(), sm.found + 1, nf * 4, hipMemcpyDeviceToHost));
        for (uint32_t u : roots) {
            const uint32_t j = s->block_at[u];
            if (j == ~0u || std::binary_search(bad.begin(), bad.end(), j) || (er.w && (*er.is_absent)[j])) return FASTECC_E_UNCORRECTABLE;  // no block there, or one already erased
            erased.push_back(u);
            result.push_back(j);
        }
        // confirmation: with the located blocks erased too, every syndrome of every column vanishes
        rc = syndromes(c, s, sm, er, erased, 0, st, &nonzero, nullptr);
        if (rc != FASTECC_OK) return rc;
        if (nonzero) return FASTECC_E_UNCORRECTABLE;
    }
    result.insert(result.end(), bad.begin(), bad.end());
    std::sort(result.begin(), result.end());
    return FASTECC_OK;
}

// MANY STRIPES (fastecc_verify_batch / _correct_batch).  Stripes back to back as for fastecc_decode_batch; the same refusals as one stripe, and
// count == 0 or a batch whose byte extent overflows 64 bits is FASTECC_E_INVAL.
int batch_args(fastecc_ctx* c, const void* data, const void* parity, uint64_t count)
{
    if (count == 0) return FASTECC_E_INVAL;
    const int rc = scrub_args(c, data, parity, FASTECC_MEM_DEVICE);
    if (rc != FASTECC_OK) return rc;
    const uint64_t block = c->S * 4, data_bytes = c->K * block, parity_bytes = c->Mu * block;
    if (count > UINT64_MAX / data_bytes || count > UINT64_MAX / parity_bytes) return FASTECC_E_INVAL;
    if ((uint64_t)(uintptr_t)data > UINT64_MAX - count * data_bytes || (uint64_t)(uintptr_t)parity > UINT64_MAX - count * parity_bytes) return FASTECC_E_INVAL;
    return FASTECC_OK;
}

// The chunk buffers (once per context): the largest power-of-two chunk whose fingerprint stripe holds at most 32 MiB with rows of at most 1 MiB.
// The chunk does not depend on the call's count, so one transform context serves every call.  F is zeroed here once: the positions that hold
// no block are the same for every stripe, and the transform reads F and writes G, so they stay zero.
int batch_state(fastecc_ctx* c, ScrubState* s)
{
    if (s->ntt_batch) return FASTECC_OK;
    uint64_t cap = 1;
    while (cap < (1ull << 16) && s->NC * 16 * (2 * cap) <= (32ull << 20)) cap *= 2;
    const uint64_t bytes = s->NC * RW * cap * 4;
    fastecc_ctx* t = nullptr;
    uint32_t *F = nullptr, *G = nullptr;
    int rc = create_ntt_ctx(&t, s->lgc, RW * 4 * cap, c->device);
    if (rc != FASTECC_OK) return rc;
    hipError_t he = hipMalloc((void**)&F, bytes);
    if (he == hipSuccess) he = hipMalloc((void**)&G, bytes);
    if (he == hipSuccess) he = hipMemset(F, 0, bytes);
    if (he == hipSuccess) he = hipDeviceSynchronize();  // (the call's stream may not order after the null stream)
    if (he != hipSuccess) {
        fastecc_destroy(t);
        if (F) (void)hipFree(F);
        if (G) (void)hipFree(G);
        return hip_fail(he, "scrub batch buffers");
    }
    s->ntt_batch = t;
    s->batch_cap = cap;
    s->d_FB = F;
    s->d_GB = G;
    return FASTECC_OK;
}

// fastecc_scrub_fingerprints (tests): a batched pass given one of these stops each chunk after its fingerprint launch and copies the chunk's
// fingerprints out instead of transforming them.  out: host, 3 words per block and entry, the entry's blocks in codeword order.
struct Probe {
    uint32_t* out;
};

// the B entries of the chunk d_FB holds -> out[(i * n + j) * 3 + c], read by pos[j]; waits for the stream
int probe_chunk(ScrubState* s, uint64_t B, hipStream_t st, uint32_t* out)
{
    std::vector<uint32_t> h(s->NC * B * RW);
    HIP_TRY(hipMemcpy2DAsync(h.data(), B * RW * 4, s->d_FB, RW * s->batch_cap * 4, B * RW * 4, s->NC, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (uint64_t i = 0; i < B; i++)
        for (uint64_t j = 0; j < s->n; j++)
            for (int col = 0; col < R; col++) out[(i * s->n + j) * R + col] = h[((uint64_t)s->pos[j] * B + i) * RW + col];
    return FASTECC_OK;
}

// What the batched verify passes share.  batch_begin: the chunk buffers, the seed's weights and `count` cleared flag bytes in d_flag (grow-only), enqueued on
// st.  batch_end: the call's one copy of the flags and its one synchronisation.
int batch_begin(fastecc_ctx* c, ScrubState* s, uint64_t count, uint64_t seed, hipStream_t st)
{
    int rc = batch_state(c, s);
    if (rc != FASTECC_OK) return rc;
    if (s->flag_cap < count) {
        if (s->d_flag) (void)hipFree(s->d_flag);
        s->d_flag = nullptr;
        s->flag_cap = 0;
        HIP_TRY(hipMalloc((void**)&s->d_flag, count));
        s->flag_cap = count;
    }
    if ((rc = upload_weights(c, s, seed, st)) != FASTECC_OK) return rc;
    HIP_TRY(hipMemsetAsync(s->d_flag, 0, count, st));
    return FASTECC_OK;
}

int batch_end(ScrubState* s, uint64_t count, hipStream_t st, std::vector<uint8_t>& flag)
{
    flag.assign(count, 0);
    HIP_TRY(hipMemcpyAsync(flag.data(), s->d_flag, count, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return FASTECC_OK;
}

// fastecc_verify_batch on a locked context: flag[b] = 1 iff fastecc_verify with this seed would find stripe b inconsistent.  Per chunk of B
// stripes: the fingerprints (weighed by the locator of the fixed and the named erasures as they are stored; absent blocks are not read and
// store zero), one transform of NC points over 4B word columns, the syndrome check of every stripe from coefficient N + fixed + w on; then
// one copy of the flags and one synchronisation for the whole call.
// probe: the chunks end after their fingerprint pass (nothing else sets a flag then: flag[b] = 1 iff a block of stripe b holds a word >= p).
int verify_batch_locked(fastecc_ctx* c, const uint32_t* data, const uint32_t* parity, uint64_t count, uint64_t seed, hipStream_t st, std::vector<uint8_t>& flag,
                        const Probe* probe = nullptr)
{
    ScrubState* s = nullptr;
    int rc = scrub_state(c, &s);
    if (rc != FASTECC_OK) return rc;
    if ((rc = batch_begin(c, s, count, seed, st)) != FASTECC_OK) return rc;
    const uint64_t chunk = c->scrub_batch_chunk > 0 ? std::min<uint64_t>(s->batch_cap, (uint64_t)c->scrub_batch_chunk) : s->batch_cap;
    const Erasures er = erasures(s, true);
    const uint64_t row = RW * s->batch_cap, NC = s->NC, m_lo = s->N + s->fixed + er.w, S = c->S;
    const bool vec = (S % 4) == 0 && (((uintptr_t)data | (uintptr_t)parity) & 15u) == 0;
    for (uint64_t b0 = 0; b0 < count; b0 += chunk) {
        const uint64_t B = std::min(chunk, count - b0);
        // every workgroup resident at once, as for one stripe
        const uint64_t groups = std::min<uint64_t>((B * s->n + 3) / 4, (uint64_t)c->cus * 6);
        {
            ProfScope ps(c, st, "fingerprint_batch", B * (s->n - er.w) * S * 4);
            if (vec)
                hipLaunchKernelGGL(fingerprint_batch_kernel<true>, dim3((unsigned)groups), dim3(256), 0, st, data, parity, (uint32_t)s->k, (uint32_t)s->n, (uint32_t)S,
                                   b0, B, s->d_weights, er.d_pos, er.d_loc, s->d_FB, row, s->d_flag, nullptr, nullptr);
            else
                hipLaunchKernelGGL(fingerprint_batch_kernel<false>, dim3((unsigned)groups), dim3(256), 0, st, data, parity, (uint32_t)s->k, (uint32_t)s->n, (uint32_t)S,
                                   b0, B, s->d_weights, er.d_pos, er.d_loc, s->d_FB, row, s->d_flag, nullptr, nullptr);
            HIP_TRY(hipGetLastError());
        }
        if (probe) {
            if ((rc = probe_chunk(s, B, st, probe->out + b0 * s->n * R)) != FASTECC_OK) return rc;
            continue;
        }
        if (m_lo >= NC) continue;  // n - k blocks named absent: no coefficient is left to check, only the words >= p count
        {
            ProfScope ps(c, st, "scrub_transform_batch");
            if ((rc = transform_bitrev(s->ntt_batch, s->d_FB, s->d_GB, false, true, (uint32_t)(RW * B), st)) != FASTECC_OK) return rc;
        }
        {
            ProfScope ps(c, st, "scrub_syndromes_batch");
            const uint64_t items = (NC - m_lo) * B;  // <= NC * batch_cap <= 2^21
            hipLaunchKernelGGL(syndrome_batch_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, s->d_GB, s->lgc, (uint32_t)NC, (uint32_t)m_lo, row,
                               (uint32_t)B, b0, s->d_flag);
            HIP_TRY(hipGetLastError());
        }
    }
    return batch_end(s, count, st, flag);
}

// ---- list forms: the same passes over the stripes list[0 .. L) of the pool ----

// the device copy of a list and its cleared per-entry flags; enqueued on st (the host list must live until the next synchronise)
int upload_list(ScrubState* s, const std::vector<uint64_t>& list, hipStream_t st)
{
    const uint64_t L = list.size();
    if (s->list_cap < L) {
        if (s->d_list) (void)hipFree(s->d_list);
        if (s->d_lflag) (void)hipFree(s->d_lflag);
        s->d_list = nullptr;
        s->d_lflag = nullptr;
        s->list_cap = 0;
        HIP_TRY(hipMalloc((void**)&s->d_list, L * 8));
        HIP_TRY(hipMalloc((void**)&s->d_lflag, 2 * L));
        s->list_cap = L;
    }
    HIP_TRY(hipMemcpyAsync(s->d_list, list.data(), L * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(s->d_lflag, 0, 2 * s->list_cap, st));
    return FASTECC_OK;
}

// One chunk of verify_batch_locked over the list entries [l0, l0 + B) of s->d_list: fingerprints, transform and either the flags of those entries
// (syn == null) or all their `avail` = NC - m_lo syndromes gathered to syn.  Nothing is copied back and nothing waits — unless probe_out is
// given (fastecc_scrub_fingerprints): then the chunk ends after the fingerprint pass with its fingerprints copied there (probe_chunk).
int list_chunk(fastecc_ctx* c, ScrubState* s, const Erasures& er, const uint32_t* data, const uint32_t* parity, uint64_t l0, uint64_t B, hipStream_t st,
               uint32_t* syn, uint32_t* probe_out = nullptr)
{
    const uint64_t row = RW * s->batch_cap, NC = s->NC, m_lo = s->N + s->fixed + er.w, S = c->S;
    const bool vec = (S % 4) == 0 && (((uintptr_t)data | (uintptr_t)parity) & 15u) == 0;
    const uint64_t groups = std::min<uint64_t>((B * s->n + 3) / 4, (uint64_t)c->cus * 5);  // every workgroup resident at once: five waves per SIMD
    uint8_t *flag = s->d_lflag, *big = s->d_lflag + s->list_cap;
    {
        ProfScope ps(c, st, "fingerprint_batch_list", B * (s->n - er.w) * S * 4);
        if (vec)
            hipLaunchKernelGGL((fingerprint_batch_kernel<true, true>), dim3((unsigned)groups), dim3(256), 0, st, data, parity, (uint32_t)s->k, (uint32_t)s->n,
                               (uint32_t)S, (uint64_t)0, B, s->d_weights, er.d_pos, er.d_loc, s->d_FB, row, flag + l0, s->d_list + l0, big + l0);
        else
            hipLaunchKernelGGL((fingerprint_batch_kernel<false, true>), dim3((unsigned)groups), dim3(256), 0, st, data, parity, (uint32_t)s->k, (uint32_t)s->n,
                               (uint32_t)S, (uint64_t)0, B, s->d_weights, er.d_pos, er.d_loc, s->d_FB, row, flag + l0, s->d_list + l0, big + l0);
        HIP_TRY(hipGetLastError());
    }
    if (probe_out) return probe_chunk(s, B, st, probe_out);
    if (m_lo >= NC) return FASTECC_OK;
    {
        ProfScope ps(c, st, "scrub_transform_batch");
        const int rc = transform_bitrev(s->ntt_batch, s->d_FB, s->d_GB, false, true, (uint32_t)(RW * B), st);
        if (rc != FASTECC_OK) return rc;
    }
    const uint64_t items = (NC - m_lo) * B;  // <= NC * batch_cap <= 2^21
    if (syn) {
        ProfScope ps(c, st, "scrub_syndromes_gather");
        hipLaunchKernelGGL(syndrome_gather_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, s->d_GB, s->lgc, (uint32_t)m_lo, (uint32_t)(NC - m_lo), row,
                           (uint32_t)B, syn);
        HIP_TRY(hipGetLastError());
    } else {
        ProfScope ps(c, st, "scrub_syndromes_batch");
        hipLaunchKernelGGL(syndrome_batch_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, s->d_GB, s->lgc, (uint32_t)NC, (uint32_t)m_lo, row,
                           (uint32_t)B, l0, flag);
        HIP_TRY(hipGetLastError());
    }
    return FASTECC_OK;
}

uint64_t chunk_of(const fastecc_ctx* c, const ScrubState* s)
{
    return c->scrub_batch_chunk > 0 ? std::min<uint64_t>(s->batch_cap, (uint64_t)c->scrub_batch_chunk) : s->batch_cap;
}

// verify_batch_locked over the stripes `list` of the pool: flag[i] = 1 iff fastecc_verify with this seed would find stripe list[i] inconsistent
// (named: under the named erasures).  One copy of the flags and one synchronisation for the call.  probe: as for verify_batch_locked, and
// flag[i] = 1 iff a block of stripe list[i] holds a word >= p.
int verify_list_locked(fastecc_ctx* c, const uint32_t* data, const uint32_t* parity, const std::vector<uint64_t>& list, uint64_t seed, hipStream_t st, bool named,
                       std::vector<uint8_t>& flag, const Probe* probe = nullptr)
{
    ScrubState* s = nullptr;
    int rc = scrub_state(c, &s);
    if (rc != FASTECC_OK) return rc;
    if ((rc = batch_state(c, s)) != FASTECC_OK) return rc;
    if ((rc = upload_weights(c, s, seed, st)) != FASTECC_OK) return rc;
    if ((rc = upload_list(s, list, st)) != FASTECC_OK) return rc;
    const Erasures er = erasures(s, named);
    const uint64_t chunk = chunk_of(c, s), L = list.size();
    for (uint64_t l0 = 0; l0 < L; l0 += chunk)
        if ((rc = list_chunk(c, s, er, data, parity, l0, std::min(chunk, L - l0), st, nullptr, probe ? probe->out + l0 * s->n * R : nullptr)) != FASTECC_OK) return rc;
    flag.assign(L, 0);
    HIP_TRY(hipMemcpyAsync(flag.data(), s->d_lflag + (probe ? s->list_cap : 0), L, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return FASTECC_OK;
}

// whether every s[i], L <= i < count, obeys the recurrence of lambda (lambda[0] = 1, length L)
bool obeys_recurrence(const uint32_t* s, uint64_t count, const std::vector<uint32_t>& lambda)
{
    const uint64_t L = lambda.size() - 1;
    for (uint64_t i = L; i < count; i++) {
        uint64_t d = s[i] % gf::P;
        for (uint64_t j = 1; j <= L; j++) d = (d + (uint64_t)lambda[j] * (s[i - j] % gf::P)) % gf::P;
        if (d != 0) return false;
    }
    return true;
}

enum : uint8_t { LOC_FALLBACK = 0, LOC_FOUND = 1, LOC_UNCORRECTABLE = 2 };

// Batched location on a locked context: for the stripes `list` of the pool — all of them inconsistent under `seed` and the
// named erasures — state[i] = LOC_FOUND with blocks[i] the located blocks (increasing; what fastecc_locate_errors returns for that stripe),
// LOC_UNCORRECTABLE where it would refuse, or LOC_FALLBACK for a stripe this path does not take: a present block holds a word >= p, or the code
// has more than 512 syndromes.  Per chunk: one list pass that gathers every syndrome, Berlekamp-Massey and the recurrence check on the host,
// one root search over all locators; two synchronisations.
int locate_list(fastecc_ctx* c, const uint32_t* data, const uint32_t* parity, const std::vector<uint64_t>& list, uint64_t seed, hipStream_t st,
                std::vector<uint8_t>& state, std::vector<std::vector<uint32_t>>& blocks)
{
    constexpr uint64_t GATHER_MAX = 512;
    ScrubState* s = nullptr;
    int rc = scrub_state(c, &s);
    if (rc != FASTECC_OK) return rc;
    const uint64_t L = list.size();
    state.assign(L, LOC_FALLBACK);
    blocks.assign(L, {});
    const Erasures er = erasures(s, true);
    const uint64_t m = s->n - s->k, avail = m > er.w ? m - er.w : 0, tmax = (uint64_t)c->locate_max;
    if (L == 0 || avail == 0 || avail > GATHER_MAX) return FASTECC_OK;
    if ((rc = batch_state(c, s)) != FASTECC_OK) return rc;
    if ((rc = upload_weights(c, s, seed, st)) != FASTECC_OK) return rc;
    if ((rc = upload_list(s, list, st)) != FASTECC_OK) return rc;
    const uint64_t chunk = std::min(chunk_of(c, s), L), gather = std::min<uint64_t>(2 * tmax, avail);
    const uint64_t lmax = std::min<uint64_t>(tmax, gather / 2), stride = lmax + 1, cap = lmax + 1;
    // the chunk's buffer: syndromes | locators | their lengths | found lists
    const uint64_t syn_words = chunk * R * avail, lam_words = chunk * stride, found_words = chunk * (cap + 1);
    const uint64_t words = syn_words + lam_words + chunk + found_words;
    if (s->loc_words < words) {
        if (s->d_loc) (void)hipFree(s->d_loc);
        s->d_loc = nullptr;
        s->loc_words = 0;
        HIP_TRY(hipMalloc((void**)&s->d_loc, words * 4));
        s->loc_words = words;
    }
    uint32_t *d_syn = s->d_loc, *d_lam = d_syn + syn_words, *d_len = d_lam + lam_words, *d_found = d_len + chunk;
    std::vector<uint32_t> syn(syn_words), lam, len, found, cand;
    std::vector<uint8_t> big(chunk);
    std::vector<uint64_t> who;                   // list entries with a locator, in table order
    std::vector<std::vector<uint32_t>> lambdas;  // their locators
    for (uint64_t l0 = 0; l0 < L; l0 += chunk) {
        const uint64_t B = std::min(chunk, L - l0);
        if ((rc = list_chunk(c, s, er, data, parity, l0, B, st, d_syn)) != FASTECC_OK) return rc;
        HIP_TRY(hipMemcpyAsync(syn.data(), d_syn, B * R * avail * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(big.data(), s->d_lflag + s->list_cap + l0, B, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        who.clear();
        lambdas.clear();
        for (uint64_t b = 0; b < B; b++) {
            if (big[b]) continue;  // known erasures besides the named ones: the single-stripe code
            const uint32_t* sy = syn.data() + b * R * avail;
            bool nonzero = false;
            for (uint64_t i = 0; i < R * avail && !nonzero; i++) nonzero = sy[i] != 0;
            if (!nonzero) continue;  // (consistent after all: cannot happen for a stripe the same seed flagged)
            // locate()'s decisions: the longest of the columns' LFSRs, the first column on ties
            std::vector<uint32_t> lambda;
            int len_best = 0;
            for (int col = 0; col < R; col++) {
                const int Lc = berlekamp_massey(sy + col * avail, (uint32_t)gather, cand);
                if (Lc > len_best) {
                    len_best = Lc;
                    lambda = cand;
                }
            }
            state[l0 + b] = LOC_UNCORRECTABLE;
            if (len_best == 0 || (uint64_t)len_best > tmax || 2ull * (uint64_t)len_best > gather) continue;
            // confirmation: every syndrome of every column obeys the locator's recurrence
            bool ok = true;
            for (int col = 0; col < R && ok; col++) ok = obeys_recurrence(sy + col * avail, avail, lambda);
            if (!ok) continue;
            who.push_back(l0 + b);
            lambdas.push_back(std::move(lambda));
        }
        if (who.empty()) continue;
        const uint64_t E = who.size();
        lam.assign(E * stride, 0);
        len.resize(E);
        for (uint64_t e = 0; e < E; e++) {
            std::copy(lambdas[e].begin(), lambdas[e].end(), lam.begin() + e * stride);
            len[e] = (uint32_t)(lambdas[e].size() - 1);
        }
        HIP_TRY(hipMemcpyAsync(d_lam, lam.data(), E * stride * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_len, len.data(), E * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(d_found, 0, E * (cap + 1) * 4, st));
        {
            ProfScope ps(c, st, "scrub_root_search_batch");
            hipLaunchKernelGGL(root_search_batch_kernel, dim3((unsigned)((E * s->NC + 255) / 256)), dim3(256), 0, st, d_lam, d_len, (uint32_t)stride, s->d_wpow,
                               (uint32_t)s->NC, (uint32_t)E, d_found, (uint32_t)cap);
            HIP_TRY(hipGetLastError());
        }
        found.resize(E * (cap + 1));
        HIP_TRY(hipMemcpyAsync(found.data(), d_found, E * (cap + 1) * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint64_t e = 0; e < E; e++) {
            const uint32_t* f = found.data() + e * (cap + 1);
            if (f[0] != len[e]) continue;  // a locator splits into distinct roots at the code's positions, or it is no locator
            std::vector<uint32_t> js;
            bool ok = true;
            for (uint32_t i = 0; i < f[0] && ok; i++) {
                const uint32_t j = s->block_at[f[1 + i]];
                ok = j != ~0u && !(er.w && (*er.is_absent)[j]);  // a block is there, and not one already erased
                js.push_back(j);
            }
            if (!ok) continue;
            std::sort(js.begin(), js.end());
            blocks[who[e]] = std::move(js);
            state[who[e]] = LOC_FOUND;
        }
    }
    return FASTECC_OK;
}

// fastecc_scrub_erasures on a locked context: `absent` (codeword indices, increasing, at most n - k) replaces the named pattern.  The marked
// position table and the locator table lfix * prod (x - w^pos) are built aside and swapped in, so a failure leaves the previous pattern in
// force.  Synchronous; every scrub call ends with a synchronise, so nothing in flight reads the tables that are freed here.
int set_erasures(fastecc_ctx* c, const std::vector<uint32_t>& absent)
{
    ScrubState* s = c->scrub;
    uint32_t *d_pos = nullptr, *d_loc = nullptr, *d_roots = nullptr;
    std::vector<uint8_t> is_absent;
    if (!absent.empty()) {
        const int rc = scrub_state(c, &s);
        if (rc != FASTECC_OK) return rc;
        std::vector<uint32_t> pos(s->pos), roots(absent.size());
        is_absent.assign(s->n, 0);
        const uint32_t w = gf::h_root((uint32_t)s->NC);
        for (size_t i = 0; i < absent.size(); i++) {
            roots[i] = gf::h_pow(w, s->pos[absent[i]]);
            pos[absent[i]] |= ABSENT;
            is_absent[absent[i]] = 1;
        }
        hipError_t he = hipMalloc((void**)&d_pos, s->n * 4);
        if (he == hipSuccess) he = hipMalloc((void**)&d_loc, s->NC * 4);
        if (he == hipSuccess) he = hipMalloc((void**)&d_roots, roots.size() * 4);
        if (he == hipSuccess) he = hipMemcpy(d_pos, pos.data(), s->n * 4, hipMemcpyHostToDevice);
        if (he == hipSuccess) he = hipMemcpy(d_roots, roots.data(), roots.size() * 4, hipMemcpyHostToDevice);
        if (he == hipSuccess) {
            hipLaunchKernelGGL(locator_kernel<false>, dim3((unsigned)((s->NC + 255) / 256)), dim3(256), 0, nullptr, s->d_lfix, d_roots, (uint32_t)roots.size(),
                               s->d_wpow, (uint32_t)s->NC, nullptr, d_loc);
            he = hipGetLastError();
        }
        if (he == hipSuccess) he = hipDeviceSynchronize();
        if (d_roots) (void)hipFree(d_roots);
        if (he != hipSuccess) {
            if (d_pos) (void)hipFree(d_pos);
            if (d_loc) (void)hipFree(d_loc);
            return hip_fail(he, "scrub erasure tables");
        }
    }
    if (!s) return FASTECC_OK;  // no scrub state yet and nothing to name
    if (s->d_pos_named) (void)hipFree(s->d_pos_named);
    if (s->d_lnamed) (void)hipFree(s->d_lnamed);
    s->d_pos_named = d_pos;
    s->d_lnamed = d_loc;
    s->absent = absent;
    s->is_absent.swap(is_absent);
    return FASTECC_OK;
}

// ---- a pattern per stripe ----

// fastecc_scrub_erasures_set on a locked context: `absent` (per pattern: codeword indices, increasing, at most n - k) replaces the set; none clears
// it.  All tables are built aside — one 2-D locator launch and one synchronisation for the whole set — and swapped in, so a refusal or a failure
// leaves the previous set in force.  Every scrub call ends with a synchronise, so nothing in flight reads the tables that are freed here.
int set_erasures_set(fastecc_ctx* c, std::vector<std::vector<uint32_t>>& absent)
{
    ScrubState* s = c->scrub;
    const uint64_t P = absent.size();
    if (P == 0) {
        if (s) {
            delete s->set;
            s->set = nullptr;
        }
        return FASTECC_OK;
    }
    const int rc = scrub_state(c, &s);
    if (rc != FASTECC_OK) return rc;
    const uint64_t n = s->n, NC = s->NC;
    if (P * NC > (1ull << 24)) return FASTECC_E_UNSUPPORTED;  // the locator tables stay at most 64 MiB
    std::unique_ptr<ScrubSet> t(new (std::nothrow) ScrubSet());
    if (!t) return FASTECC_E_NOMEM;
    t->P = P;
    t->is_absent.resize(P);
    t->mlo.resize(P);
    std::vector<uint32_t> pos(P * n), roots, off(P + 1, 0);
    const uint32_t w = gf::h_root((uint32_t)NC);
    for (uint64_t q = 0; q < P; q++) {
        std::copy(s->pos.begin(), s->pos.end(), pos.begin() + q * n);
        t->is_absent[q].assign(n, 0);
        for (uint32_t j : absent[q]) {
            roots.push_back(gf::h_pow(w, s->pos[j]));
            pos[q * n + j] |= ABSENT;
            t->is_absent[q][j] = 1;
        }
        off[q + 1] = (uint32_t)roots.size();  // at most P (n - k) <= P NC <= 2^24
        t->mlo[q] = (uint32_t)(s->N + s->fixed + absent[q].size());
    }
    t->mlo_min = *std::min_element(t->mlo.begin(), t->mlo.end());
    t->absent.swap(absent);
    uint32_t *d_roots = nullptr, *d_off = nullptr;
    hipError_t he = hipMalloc((void**)&t->d_pos, P * n * 4);
    if (he == hipSuccess) he = hipMalloc((void**)&t->d_l, P * NC * 4);
    if (he == hipSuccess) he = hipMalloc((void**)&t->d_mlo, P * 4);
    if (he == hipSuccess) he = hipMalloc((void**)&d_roots, std::max<size_t>(roots.size(), 1) * 4);
    if (he == hipSuccess) he = hipMalloc((void**)&d_off, (P + 1) * 4);
    if (he == hipSuccess) he = hipMemcpy(t->d_pos, pos.data(), P * n * 4, hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(t->d_mlo, t->mlo.data(), P * 4, hipMemcpyHostToDevice);
    if (he == hipSuccess && !roots.empty()) he = hipMemcpy(d_roots, roots.data(), roots.size() * 4, hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(d_off, off.data(), (P + 1) * 4, hipMemcpyHostToDevice);
    if (he == hipSuccess) {
        hipLaunchKernelGGL(locator_set_kernel, dim3((unsigned)((NC + 255) / 256), (unsigned)P), dim3(256), 0, nullptr, s->d_lfix, d_roots, d_off, s->d_wpow, (uint32_t)NC,
                           t->d_l);
        he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipDeviceSynchronize();
    if (d_roots) (void)hipFree(d_roots);
    if (d_off) (void)hipFree(d_off);
    if (he != hipSuccess) return hip_fail(he, "scrub erasure set tables");
    delete s->set;
    s->set = t.release();
    return FASTECC_OK;
}

// fastecc_verify_batch_set's own argument check on a locked context: a set is prepared and every entry names one of its patterns or none
int set_args(const fastecc_ctx* c, const uint32_t* pattern_of, uint64_t count)
{
    const ScrubState* s = c->scrub;
    if (!s || !s->set) return FASTECC_E_INVAL;
    for (uint64_t b = 0; b < count; b++)
        if (pattern_of[b] >= s->set->P && pattern_of[b] != FASTECC_PATTERN_NONE) return FASTECC_E_INVAL;
    return FASTECC_OK;
}

// fastecc_verify_batch_set on a locked context (set_args passed): verify_batch_locked with stripe b under pattern pattern_of[b] of the set.
// flag[b] = 1 iff fastecc_scrub_erasures(that pattern) + fastecc_verify with this seed would find stripe b inconsistent; 0 for FASTECC_PATTERN_NONE.
// Per chunk: the fingerprints (fingerprint_set_kernel), one transform, the syndrome check of every stripe from its own pattern's bound on.  A chunk
// in which no block is read is skipped; one in which no stripe has a coefficient left skips transform and check.  pattern_of is copied synchronously
// (every scrub call, a failed one included, leaves nothing in flight that reads the device copy), so the caller's array is free on every return.
int verify_batch_set_chunks(fastecc_ctx* c, const uint32_t* data, const uint32_t* parity, uint64_t count, const uint32_t* pattern_of, uint64_t seed, hipStream_t st,
                            std::vector<uint8_t>& flag)
{
    ScrubState* s = c->scrub;
    const ScrubSet* t = s->set;
    int rc;
    if (s->pattern_cap < count) {
        if (s->d_pattern_of) (void)hipFree(s->d_pattern_of);
        s->d_pattern_of = nullptr;
        s->pattern_cap = 0;
        HIP_TRY(hipMalloc((void**)&s->d_pattern_of, count * 4));
        s->pattern_cap = count;
    }
    HIP_TRY(hipMemcpy(s->d_pattern_of, pattern_of, count * 4, hipMemcpyHostToDevice));
    if ((rc = batch_begin(c, s, count, seed, st)) != FASTECC_OK) return rc;
    const uint64_t chunk = chunk_of(c, s);
    const uint64_t row = RW * s->batch_cap, NC = s->NC, S = c->S, m_lo = t->mlo_min;
    const bool vec = (S % 4) == 0 && (((uintptr_t)data | (uintptr_t)parity) & 15u) == 0;
    for (uint64_t b0 = 0; b0 < count; b0 += chunk) {
        const uint64_t B = std::min(chunk, count - b0);
        uint64_t blocks_read = 0;
        bool to_check = false;
        for (uint64_t b = b0; b < b0 + B; b++) {
            if (pattern_of[b] == FASTECC_PATTERN_NONE) continue;
            blocks_read += s->n - t->absent[pattern_of[b]].size();
            to_check = to_check || t->mlo[pattern_of[b]] < NC;
        }
        if (blocks_read == 0) continue;  // every stripe of the chunk is FASTECC_PATTERN_NONE (a stripe with a pattern reads at least k blocks)
        // every workgroup resident at once, as for fastecc_verify_batch
        const uint64_t groups = std::min<uint64_t>((B * s->n + 3) / 4, (uint64_t)c->cus * 6);
        {
            ProfScope ps(c, st, "fingerprint_set", blocks_read * S * 4);
            if (vec)
                hipLaunchKernelGGL(fingerprint_set_kernel<true>, dim3((unsigned)groups), dim3(256), 0, st, data, parity, (uint32_t)s->k, (uint32_t)s->n, (uint32_t)S, b0,
                                   B, s->d_weights, s->d_pattern_of, t->d_pos, t->d_l, (uint32_t)NC, s->d_FB, row, s->d_flag);
            else
                hipLaunchKernelGGL(fingerprint_set_kernel<false>, dim3((unsigned)groups), dim3(256), 0, st, data, parity, (uint32_t)s->k, (uint32_t)s->n, (uint32_t)S, b0,
                                   B, s->d_weights, s->d_pattern_of, t->d_pos, t->d_l, (uint32_t)NC, s->d_FB, row, s->d_flag);
            HIP_TRY(hipGetLastError());
        }
        if (!to_check) continue;  // every stripe of the chunk has n - k blocks absent (or none named): only the words >= p count
        {
            ProfScope ps(c, st, "scrub_transform_batch");
            if ((rc = transform_bitrev(s->ntt_batch, s->d_FB, s->d_GB, false, true, (uint32_t)(RW * B), st)) != FASTECC_OK) return rc;
        }
        {
            ProfScope ps(c, st, "scrub_syndromes_set");
            const uint64_t items = (NC - m_lo) * B;  // <= NC * batch_cap <= 2^21
            hipLaunchKernelGGL(syndrome_set_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, s->d_GB, s->lgc, (uint32_t)NC, (uint32_t)m_lo, row,
                               (uint32_t)B, b0, s->d_pattern_of, t->d_mlo, s->d_flag);
            HIP_TRY(hipGetLastError());
        }
    }
    return batch_end(s, count, st, flag);
}

// a failed pass waits for what it enqueued: the next call may free or overwrite the buffers its kernels read
int verify_batch_set_locked(fastecc_ctx* c, const uint32_t* data, const uint32_t* parity, uint64_t count, const uint32_t* pattern_of, uint64_t seed, hipStream_t st,
                            std::vector<uint8_t>& flag)
{
    const int rc = verify_batch_set_chunks(c, data, parity, count, pattern_of, seed, st, flag);
    if (rc != FASTECC_OK) (void)hipStreamSynchronize(st);
    return rc;
}

// fastecc_verify; named = false: over all blocks whatever fastecc_scrub_erasures named (the closing check of fastecc_correct)
int verify_impl(fastecc_ctx* c, const void* data, const void* parity, int mem_kind, void* stream, uint64_t seed, int* consistent, bool named)
{
    if (!consistent) return FASTECC_E_INVAL;
    int rc = scrub_args(c, data, parity, mem_kind);
    if (rc != FASTECC_OK) return rc;
    DeviceGuard dg(c->device);
    if (!dg.ok) return FASTECC_E_DEVICE;
    CallLock lk(c->mu);
    return guarded([&]() -> int {
        std::vector<uint32_t> found;
        ScrubState* s = nullptr;
        int r = scrub_state(c, &s);
        if (r != FASTECC_OK) return r;
        r = locate(c, s, erasures(s, named), (const uint32_t*)data, (const uint32_t*)parity, seed, (hipStream_t)stream, found, true);
        if (r == FASTECC_OK) *consistent = found.empty() ? 1 : 0;
        return r;
    });
}

// fastecc_correct on one stripe (DEVICE memory, arguments checked): locate under the single fastecc_scrub_erasures pattern, or under pattern q of
// the set (from_set), then rebuild located and absent blocks and verify the whole codeword with the derived seed.  found: the located blocks.
int correct_stripe(fastecc_ctx* c, void* data, void* parity, void* stream, uint64_t seed, bool from_set, uint32_t q, std::vector<uint32_t>& found)
{
    std::vector<uint32_t> absent;
    {
        CallLock lk(c->mu);
        ScrubState* s = nullptr;
        int r = scrub_state(c, &s);
        if (r != FASTECC_OK) return r;
        if (from_set && (!s->set || q >= s->set->P)) return FASTECC_E_INVAL;  // (the set was replaced while the call ran)
        const Erasures er = from_set ? set_view(s, q) : erasures(s, true);
        if (er.w) absent = *er.absent;
        r = locate(c, s, er, (const uint32_t*)data, (const uint32_t*)parity, seed, (hipStream_t)stream, found, false);
        if (r != FASTECC_OK) return r;
    }
    if (found.empty()) return FASTECC_OK;  // consistent: untouched, the absent blocks included
    // the erasure decoder rebuilds the located blocks and, in the same repair, the ones named absent (prepare and repair take the
    // context's lock themselves); the codeword is whole then, so the closing verify reads every block
    std::vector<uint8_t> dp(c->K, 1), pp(c->Mu, 1);
    for (uint32_t j : found) (j < c->K ? dp[j] : pp[j - c->K]) = 0;
    for (uint32_t j : absent) (j < c->K ? dp[j] : pp[j - c->K]) = 0;
    int r = fastecc_decode_prepare(c, dp.data(), pp.data());
    if (r != FASTECC_OK) return r;
    r = fastecc_repair(c, data, parity, FASTECC_MEM_DEVICE, stream);
    if (r != FASTECC_OK) return r;
    uint64_t seed2 = seed ^ 0x5C7B5C7B5C7B5C7Bull;
    seed2 = splitmix64(seed2);
    int ok = 0;
    r = verify_impl(c, data, parity, FASTECC_MEM_DEVICE, stream, seed2, &ok, false);
    if (r != FASTECC_OK) return r;
    return ok ? FASTECC_OK : FASTECC_E_UNCORRECTABLE;
}

int report(const std::vector<uint32_t>& found, uint64_t* blocks, uint64_t cap, uint64_t* count)
{
    for (uint64_t i = 0; i < found.size() && i < cap; i++) blocks[i] = found[i];
    *count = found.size();
    return FASTECC_OK;
}

}  // namespace

}  // namespace fastecc

using namespace fastecc;

extern "C" {

int fastecc_gf_berlekamp_massey(const uint32_t* s, uint32_t count, uint32_t* lambda, uint32_t cap)
{
    if ((!s && count) || !lambda) return FASTECC_E_INVAL;
    return guarded([&]() -> int {
        std::vector<uint32_t> C;
        const int L = berlekamp_massey(s, count, C);
        if ((uint64_t)cap < (uint64_t)L + 1) return FASTECC_E_INVAL;
        std::copy(C.begin(), C.end(), lambda);
        return L;
    });
}

int fastecc_scrub_fingerprints(fastecc_ctx* c, const void* data, const void* parity, uint64_t count, const uint64_t* list, int form, void* stream, uint64_t seed,
                               uint32_t* out, uint8_t* big)
{
    if (!out || !big || form < 0 || form > 2 || (form == 0 && count != 1) || (form == 2) != (list != nullptr)) return FASTECC_E_INVAL;
    const int rc = batch_args(c, data, parity, count);
    if (rc != FASTECC_OK) return rc;
    DeviceGuard dg(c->device);
    if (!dg.ok) return FASTECC_E_DEVICE;
    CallLock lk(c->mu);
    return guarded([&]() -> int {
        hipStream_t st = (hipStream_t)stream;
        const uint32_t *d = (const uint32_t*)data, *p = (const uint32_t*)parity;
        ScrubState* s = nullptr;
        int r = scrub_state(c, &s);
        if (r != FASTECC_OK) return r;
        if (!s->absent.empty()) return FASTECC_E_UNSUPPORTED;
        if (form == 0) {  // fingerprint_kernel stores F unweighed, by position
            Small sm;
            if ((r = small_buffers(s, (uint32_t)c->locate_max, &sm)) != FASTECC_OK) return r;
            std::vector<uint32_t> bad;
            if ((r = fingerprints(c, s, sm, erasures(s, false), d, p, seed, st, bad)) != FASTECC_OK) return r;
            std::vector<uint32_t> F(s->NC * RW);
            HIP_TRY(hipMemcpy(F.data(), s->d_F, F.size() * 4, hipMemcpyDeviceToHost));  // (fingerprints() has waited for the stream)
            for (uint64_t j = 0; j < s->n; j++)
                for (int col = 0; col < R; col++) out[j * R + col] = F[(uint64_t)s->pos[j] * RW + col];
            big[0] = bad.empty() ? 0 : 1;
            return FASTECC_OK;
        }
        if (s->d_lfix) return FASTECC_E_UNSUPPORTED;  // the batched passes store F times the fixed erasures' locator
        const Probe probe{out};
        std::vector<uint8_t> flag;
        if (form == 1)
            r = verify_batch_locked(c, d, p, count, seed, st, flag, &probe);
        else
            r = verify_list_locked(c, d, p, std::vector<uint64_t>(list, list + count), seed, st, false, flag, &probe);
        if (r != FASTECC_OK) return r;
        std::copy(flag.begin(), flag.end(), big);
        return FASTECC_OK;
    });
}

int fastecc_scrub_erasures(fastecc_ctx* c, const uint8_t* data_present, const uint8_t* parity_present)
{
    if (!c) return FASTECC_E_INVAL;
    if (c->sharded || c->p61 || c->field != FASTECC_FIELD_GF_FFF00001 || c->q > 1) return FASTECC_E_UNSUPPORTED;  // fastecc_verify's refusals by kind
    return guarded([&]() -> int {
        std::vector<uint32_t> absent;
        for (uint64_t i = 0; data_present && i < c->K; i++)
            if (!data_present[i]) absent.push_back((uint32_t)i);
        for (uint64_t q = 0; parity_present && q < c->Mu; q++)
            if (!parity_present[q]) absent.push_back((uint32_t)(c->K + q));
        if (absent.size() > c->Mu) return FASTECC_E_INVAL;
        DeviceGuard dg(c->device);
        if (!dg.ok) return FASTECC_E_DEVICE;
        CallLock lk(c->mu);
        return set_erasures(c, absent);
    });
}

int fastecc_verify(fastecc_ctx* c, const void* data, const void* parity, int mem_kind, void* stream, uint64_t seed, int* consistent)
{
    return verify_impl(c, data, parity, mem_kind, stream, seed, consistent, true);
}

int fastecc_locate_errors(fastecc_ctx* c, const void* data, const void* parity, int mem_kind, void* stream, uint64_t seed, uint64_t* blocks, uint64_t cap,
                          uint64_t* count)
{
    if (!count || (!blocks && cap)) return FASTECC_E_INVAL;
    int rc = scrub_args(c, data, parity, mem_kind);
    if (rc != FASTECC_OK) return rc;
    DeviceGuard dg(c->device);
    if (!dg.ok) return FASTECC_E_DEVICE;
    CallLock lk(c->mu);
    return guarded([&]() -> int {
        std::vector<uint32_t> found;
        ScrubState* s = nullptr;
        int r = scrub_state(c, &s);
        if (r != FASTECC_OK) return r;
        r = locate(c, s, erasures(s, true), (const uint32_t*)data, (const uint32_t*)parity, seed, (hipStream_t)stream, found, false);
        return r == FASTECC_OK ? report(found, blocks, cap, count) : r;
    });
}

int fastecc_correct(fastecc_ctx* c, void* data, void* parity, int mem_kind, void* stream, uint64_t seed, uint64_t* blocks, uint64_t cap, uint64_t* count)
{
    if (!count || (!blocks && cap)) return FASTECC_E_INVAL;
    int rc = scrub_args(c, data, parity, mem_kind);
    if (rc != FASTECC_OK) return rc;
    DeviceGuard dg(c->device);
    if (!dg.ok) return FASTECC_E_DEVICE;
    return guarded([&]() -> int {
        std::vector<uint32_t> found;
        const int r = correct_stripe(c, data, parity, stream, seed, false, 0, found);
        return r == FASTECC_OK ? report(found, blocks, cap, count) : r;
    });
}

int fastecc_verify_batch(fastecc_ctx* c, const void* data, const void* parity, uint64_t count, void* stream, uint64_t seed, uint8_t* consistent,
                         uint64_t* inconsistent)
{
    if (!consistent || !inconsistent) return FASTECC_E_INVAL;
    const int rc = batch_args(c, data, parity, count);
    if (rc != FASTECC_OK) return rc;
    DeviceGuard dg(c->device);
    if (!dg.ok) return FASTECC_E_DEVICE;
    CallLock lk(c->mu);
    return guarded([&]() -> int {
        std::vector<uint8_t> flag;
        const int r = verify_batch_locked(c, (const uint32_t*)data, (const uint32_t*)parity, count, seed, (hipStream_t)stream, flag);
        if (r != FASTECC_OK) return r;
        uint64_t bad = 0;
        for (uint64_t b = 0; b < count; b++) {
            consistent[b] = flag[b] ? 0 : 1;
            bad += flag[b] ? 1 : 0;
        }
        *inconsistent = bad;
        return FASTECC_OK;
    });
}

int fastecc_locate_errors_batch(fastecc_ctx* c, const void* data, const void* parity, uint64_t count, void* stream, uint64_t seed, uint8_t* status,
                                uint64_t* blocks, uint64_t cap, uint32_t* counts, uint64_t* inconsistent)
{
    if (!status || !inconsistent || (cap && (!blocks || !counts))) return FASTECC_E_INVAL;
    const int rc = batch_args(c, data, parity, count);
    if (rc != FASTECC_OK) return rc;
    if (cap && count > UINT64_MAX / 8 / cap) return FASTECC_E_INVAL;
    DeviceGuard dg(c->device);
    if (!dg.ok) return FASTECC_E_DEVICE;
    CallLock lk(c->mu);
    return guarded([&]() -> int {
        hipStream_t st = (hipStream_t)stream;
        std::vector<uint8_t> flag, state;
        int r = verify_batch_locked(c, (const uint32_t*)data, (const uint32_t*)parity, count, seed, st, flag);
        if (r != FASTECC_OK) return r;
        std::vector<uint64_t> list;
        for (uint64_t b = 0; b < count; b++)
            if (flag[b]) list.push_back(b);
        std::vector<std::vector<uint32_t>> found;
        if ((r = locate_list(c, (const uint32_t*)data, (const uint32_t*)parity, list, seed, st, state, found)) != FASTECC_OK) return r;
        const uint64_t data_words = c->K * c->S, parity_words = c->Mu * c->S;
        for (size_t i = 0; i < list.size(); i++) {
            if (state[i] != LOC_FALLBACK) continue;
            // a word >= p in a present block, or more syndromes than the batched pass gathers: the single-stripe code through the stripe's own pointers
            r = locate(c, c->scrub, erasures(c->scrub, true), (const uint32_t*)data + list[i] * data_words, (const uint32_t*)parity + list[i] * parity_words, seed, st,
                       found[i], false);
            if (r == FASTECC_E_UNCORRECTABLE) state[i] = LOC_UNCORRECTABLE;
            else if (r != FASTECC_OK) return r;
            else state[i] = LOC_FOUND;
        }
        // every output is written only now: a failed call leaves them alone
        bool uncorrectable = false;
        uint64_t bad = 0;
        std::fill(status, status + count, (uint8_t)0);
        if (counts) std::fill(counts, counts + count, 0u);
        for (size_t i = 0; i < list.size(); i++) {
            const uint64_t b = list[i];
            if (state[i] == LOC_UNCORRECTABLE) {
                status[b] = 2;
                uncorrectable = true;
                bad++;
                continue;
            }
            if (found[i].empty()) continue;  // (consistent after all)
            status[b] = 1;
            bad++;
            if (counts) counts[b] = (uint32_t)found[i].size();
            for (uint64_t q = 0; q < found[i].size() && q < cap; q++) blocks[b * cap + q] = found[i][q];
        }
        *inconsistent = bad;
        return uncorrectable ? FASTECC_E_UNCORRECTABLE : FASTECC_OK;
    });
}

int fastecc_correct_batch(fastecc_ctx* c, void* data, void* parity, uint64_t count, void* stream, uint64_t seed, uint8_t* status, uint64_t* inconsistent)
{
    if (!status || !inconsistent) return FASTECC_E_INVAL;
    const int rc = batch_args(c, data, parity, count);
    if (rc != FASTECC_OK) return rc;
    DeviceGuard dg(c->device);
    if (!dg.ok) return FASTECC_E_DEVICE;
    return guarded([&]() -> int {
        hipStream_t hst = (hipStream_t)stream;
        const int mode = c->correct_batch_mode;
        std::vector<uint8_t> flag, state;
        std::vector<uint64_t> list;
        std::vector<std::vector<uint32_t>> found;
        std::vector<uint32_t> absent;
        bool grouped = false;
        {
            CallLock lk(c->mu);
            int r = verify_batch_locked(c, (const uint32_t*)data, (const uint32_t*)parity, count, seed, hst, flag);
            if (r != FASTECC_OK) return r;
            for (uint64_t b = 0; b < count; b++)
                if (flag[b]) list.push_back(b);
            // one stripe has nothing to share; mode 0 groups from two qualifying stripes on
            if (mode != 2 && list.size() >= (mode == 1 ? 1u : 2u)) {
                if ((r = locate_list(c, (const uint32_t*)data, (const uint32_t*)parity, list, seed, hst, state, found)) != FASTECC_OK) return r;
                const uint64_t qualify = (uint64_t)(list.size() - std::count(state.begin(), state.end(), (uint8_t)LOC_FALLBACK));
                grouped = qualify >= (mode == 1 ? 1u : 2u);
                if (grouped) absent = c->scrub->absent;
            }
        }
        const uint64_t block = c->S * 4, data_bytes = c->K * block, parity_bytes = c->Mu * block;
        std::vector<uint8_t> st(count, 0);
        bool uncorrectable = false;
        // fastecc_correct on one inconsistent stripe through its own pointers (it takes the lock itself)
        auto correct_one = [&](uint64_t b) -> int {
            uint64_t n_found = 0;
            const int r = fastecc_correct(c, (char*)data + b * data_bytes, (char*)parity + b * parity_bytes, FASTECC_MEM_DEVICE, stream, seed, nullptr, 0, &n_found);
            if (r == FASTECC_E_UNCORRECTABLE) {
                st[b] = 2;
                uncorrectable = true;
            } else if (r != FASTECC_OK) {
                return r;
            } else {
                st[b] = n_found ? 1 : 0;
            }
            return FASTECC_OK;
        };
        if (!grouped) {
            for (uint64_t b : list) {
                const int r = correct_one(b);
                if (r != FASTECC_OK) return r;
            }
        } else {
            // the located stripes by their lost set — located blocks and blocks named absent — in the order the first stripe of each set appears
            std::map<std::vector<uint32_t>, size_t> group_of;
            std::vector<std::vector<uint32_t>> lost_sets;
            std::vector<std::vector<uint64_t>> members;
            uint64_t repaired = 0;
            for (size_t i = 0; i < list.size(); i++) {
                if (state[i] == LOC_UNCORRECTABLE) {
                    st[list[i]] = 2;
                    uncorrectable = true;
                }
                if (state[i] != LOC_FOUND || found[i].empty()) continue;
                std::vector<uint32_t> lost(found[i]);
                lost.insert(lost.end(), absent.begin(), absent.end());
                std::sort(lost.begin(), lost.end());
                auto it = group_of.find(lost);
                if (it == group_of.end()) {
                    it = group_of.emplace(lost, lost_sets.size()).first;
                    lost_sets.push_back(lost);
                    members.emplace_back();
                }
                members[it->second].push_back(list[i]);
                repaired++;
            }
            if (repaired) {
                std::vector<uint64_t> order;  // the groups' stripes back to back: group g at its offset
                for (const auto& mb : members) order.insert(order.end(), mb.begin(), mb.end());
                // the lists the repair launches read live on the device for this call only (the repair runs outside the scrub state's lock)
                struct DeviceList {
                    uint64_t* p = nullptr;
                    ~DeviceList()
                    {
                        if (p) (void)hipFree(p);
                    }
                } dl;
                HIP_TRY(hipMalloc((void**)&dl.p, order.size() * 8));
                HIP_TRY(hipMemcpy(dl.p, order.data(), order.size() * 8, hipMemcpyHostToDevice));
                uint64_t at = 0;
                for (size_t g = 0; g < members.size(); g++) {
                    std::vector<uint8_t> dp(c->K, 1), pp(c->Mu, 1);
                    for (uint32_t j : lost_sets[g]) (j < c->K ? dp[j] : pp[j - c->K]) = 0;
                    int r = fastecc_decode_prepare(c, dp.data(), pp.data());
                    if (r != FASTECC_OK) return r;
                    if ((r = repair_list(c, data, parity, order.data() + at, dl.p + at, members[g].size(), stream)) != FASTECC_OK) return r;
                    at += members[g].size();
                }
                // the closing verify of fastecc_correct for all of them at once: its second seed, every block read (the stripes are whole now)
                uint64_t seed2 = seed ^ 0x5C7B5C7B5C7B5C7Bull;
                seed2 = splitmix64(seed2);
                std::vector<uint8_t> still;
                {
                    CallLock lk(c->mu);
                    const int r = verify_list_locked(c, (const uint32_t*)data, (const uint32_t*)parity, order, seed2, hst, false, still);
                    if (r != FASTECC_OK) return r;
                }
                for (size_t i = 0; i < order.size(); i++) {
                    st[order[i]] = still[i] ? 2 : 1;
                    uncorrectable = uncorrectable || still[i];
                }
            }
            for (size_t i = 0; i < list.size(); i++) {
                if (state[i] != LOC_FALLBACK) continue;
                const int r = correct_one(list[i]);
                if (r != FASTECC_OK) return r;
            }
        }
        std::copy(st.begin(), st.end(), status);
        *inconsistent = list.size();
        return uncorrectable ? FASTECC_E_UNCORRECTABLE : FASTECC_OK;
    });
}

int fastecc_scrub_erasures_set(fastecc_ctx* c, const uint8_t* data_present, const uint8_t* parity_present, uint64_t n_patterns)
{
    if (!c || (n_patterns && (!data_present || !parity_present)) || n_patterns > 4096) return FASTECC_E_INVAL;
    if (c->sharded || c->p61 || c->field != FASTECC_FIELD_GF_FFF00001 || c->q > 1) return FASTECC_E_UNSUPPORTED;  // fastecc_scrub_erasures' refusals by kind
    return guarded([&]() -> int {
        std::vector<std::vector<uint32_t>> absent(n_patterns);
        for (uint64_t q = 0; q < n_patterns; q++) {
            for (uint64_t i = 0; i < c->K; i++)
                if (!data_present[q * c->K + i]) absent[q].push_back((uint32_t)i);
            for (uint64_t i = 0; i < c->Mu; i++)
                if (!parity_present[q * c->Mu + i]) absent[q].push_back((uint32_t)(c->K + i));
            if (absent[q].size() > c->Mu) return FASTECC_E_INVAL;
        }
        DeviceGuard dg(c->device);
        if (!dg.ok) return FASTECC_E_DEVICE;
        CallLock lk(c->mu);
        return set_erasures_set(c, absent);
    });
}

int fastecc_verify_batch_set(fastecc_ctx* c, const void* data, const void* parity, uint64_t count, const uint32_t* pattern_of, void* stream, uint64_t seed,
                             uint8_t* consistent, uint64_t* inconsistent)
{
    if (!consistent || !inconsistent || !pattern_of) return FASTECC_E_INVAL;
    int rc = batch_args(c, data, parity, count);
    if (rc != FASTECC_OK) return rc;
    DeviceGuard dg(c->device);
    if (!dg.ok) return FASTECC_E_DEVICE;
    CallLock lk(c->mu);
    if ((rc = set_args(c, pattern_of, count)) != FASTECC_OK) return rc;
    return guarded([&]() -> int {
        std::vector<uint8_t> flag;
        const int r = verify_batch_set_locked(c, (const uint32_t*)data, (const uint32_t*)parity, count, pattern_of, seed, (hipStream_t)stream, flag);
        if (r != FASTECC_OK) return r;
        uint64_t bad = 0;
        for (uint64_t b = 0; b < count; b++) {
            consistent[b] = flag[b] ? 0 : 1;
            bad += flag[b] ? 1 : 0;
        }
        *inconsistent = bad;
        return FASTECC_OK;
    });
}

int fastecc_correct_batch_set(fastecc_ctx* c, void* data, void* parity, uint64_t count, const uint32_t* pattern_of, void* stream, uint64_t seed, uint8_t* status,
                              uint64_t* inconsistent)
{
    if (!status || !inconsistent || !pattern_of) return FASTECC_E_INVAL;
    int rc = batch_args(c, data, parity, count);
    if (rc != FASTECC_OK) return rc;
    DeviceGuard dg(c->device);
    if (!dg.ok) return FASTECC_E_DEVICE;
    return guarded([&]() -> int {
        std::vector<uint8_t> flag;
        {
            CallLock lk(c->mu);
            int r = set_args(c, pattern_of, count);
            if (r != FASTECC_OK) return r;
            if ((r = verify_batch_set_locked(c, (const uint32_t*)data, (const uint32_t*)parity, count, pattern_of, seed, (hipStream_t)stream, flag)) != FASTECC_OK) return r;
        }
        // fastecc_correct under the stripe's own pattern on each inconsistent stripe, one after the other (it takes the lock itself)
        const uint64_t block = c->S * 4, data_bytes = c->K * block, parity_bytes = c->Mu * block;
        std::vector<uint8_t> st(count, 0);
        std::vector<uint32_t> found;
        bool uncorrectable = false;
        uint64_t bad = 0;
        for (uint64_t b = 0; b < count; b++) {
            if (!flag[b]) continue;
            bad++;
            const int r = correct_stripe(c, (char*)data + b * data_bytes, (char*)parity + b * parity_bytes, stream, seed, true, pattern_of[b], found);
            if (r == FASTECC_E_UNCORRECTABLE) {
                st[b] = 2;
                uncorrectable = true;
            } else if (r != FASTECC_OK) {
                return r;
            } else {
                st[b] = found.empty() ? 0 : 1;
            }
        }
        std::copy(st.begin(), st.end(), status);
        *inconsistent = bad;
        return uncorrectable ? FASTECC_E_UNCORRECTABLE : FASTECC_OK;
    });
}

}  // extern "C"
