// decode_prepare.hip — fastecc_decode_prepare of the GF(0xFFF00001) codes: everything that depends only on the erasure PATTERN, done once, on the
// device (the algorithm and the even / odd split: the head of decode.hip; the state it fills: decode_state.hpp).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "decode_state.hpp"
#include "ntt_device.hpp"

namespace fastecc {

namespace {

// ------------------------------------------------------------------------------------------------
// fastecc_decode_prepare on the device.  All values are plain representatives unless a table is consumed by
// gf::mul_mont, in which case it is stored in Montgomery form (x * 2^32 mod p = gf::mul(x, MONT_ONE)).
// ------------------------------------------------------------------------------------------------
constexpr int LEAF_LOG = 4, LEAF = 1 << LEAF_LOG;
constexpr int TREE_LOW = 10;  // tall trees: the polynomials of 2^TREE_LOW roots come from one kernel (schoolbook products in LDS) instead of six more levels  // the lowest levels of the tree are one schoolbook kernel: 16 roots per thread

__device__ __forceinline__ uint32_t dev_pow(uint32_t x, uint32_t e)
{
    uint32_t r = 1;
    for (; e; e >>= 1) {
        if (e & 1u) r = gf::mul(r, x);
        x = gf::mul(x, x);
    }
    return r;
}

// wpow[u] = w^u
__global__ __launch_bounds__(256) void wpow_kernel(uint32_t* __restrict__ wpow, uint32_t w, uint32_t count)
{
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u < count) wpow[u] = dev_pow(w, u);
}

// (2k,k) layout: position u is data block u / 2 (u even) or parity block u / 2 (bit 31) — the block map of the table-driven gather, which
// serves the plans whose first pass cannot read the two stripes itself
__global__ __launch_bounds__(256) void standard_srcmap_kernel(const uint8_t* __restrict__ state, uint32_t NC, uint32_t* __restrict__ srcmap)
{
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u < NC) srcmap[u] = state[u] == ST_HELD ? ((u >> 1) | ((u & 1u) << 31)) : 0u;
}

// erased[] = the positions whose state is LOST or UNUSED, in any order; *counter (zero on entry) ends as their number.  A thread takes 16
// positions (one 16-byte load of the state), a workgroup 4096: ONE atomic per workgroup (one per wave measured 187 us at NC = 2^20 — 16384
// atomics on one address).
__global__ __launch_bounds__(256) void erased_list_kernel(const uint8_t* __restrict__ state, uint32_t NC, uint32_t* __restrict__ erased, uint32_t* __restrict__ counter)
{
    __shared__ uint32_t wave_sum[4], block_base;
    const uint32_t u0 = (blockIdx.x * blockDim.x + threadIdx.x) * 16u;
    uint32_t bits = 0;
    if (u0 + 16u <= NC) {
        const uint4 v = *reinterpret_cast<const uint4*>(state + u0);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t st = (w[i >> 2] >> (8 * (i & 3))) & 0xFFu;
            bits |= (uint32_t)(st == ST_LOST || st == ST_UNUSED) << i;
        }
    } else {
        for (uint32_t i = 0; i < 16u && u0 + i < NC; ++i) bits |= (uint32_t)(state[u0 + i] == ST_LOST || state[u0 + i] == ST_UNUSED) << i;
    }
    const uint32_t mine = (uint32_t)__builtin_popcount(bits), lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = mine;  // inclusive prefix sum over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d);
        if (lane >= (uint32_t)d) incl += t;
    }
    if (lane == 63u) wave_sum[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t total = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
        block_base = total ? atomicAdd(counter, total) : 0u;
    }
    __syncthreads();
    uint32_t at = block_base + incl - mine;
    for (uint32_t w = 0; w < wave; ++w) at += wave_sum[w];
    for (uint32_t b = bits; b; b &= b - 1u) erased[at++] = u0 + (uint32_t)__builtin_ctz(b);
}

// The reference's (2k,k) layout, pattern scan on the device: counts[0] = lost data blocks, [1] = lost parity blocks, [2 + h] = surviving parity
// blocks at multiples of 2^h of the parity half (h = 1..5: the split transform's "small form" reads those alone).
__global__ __launch_bounds__(256) void presence_counts_kernel(const uint8_t* __restrict__ pd, const uint8_t* __restrict__ pp, uint32_t N, uint32_t* __restrict__ counts)
{
    __shared__ uint32_t acc[7];
    if (threadIdx.x < 7) acc[threadIdx.x] = 0;
    __syncthreads();
    uint32_t c[7] = {};
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        const uint32_t held_p = pp[i] != 0;
        c[0] += pd[i] == 0;
        c[1] += 1u - held_p;
        const int tz = __builtin_ctz(i | 32u);
#pragma unroll
        for (int h = 1; h <= 5; ++h) c[1 + h] += held_p & (uint32_t)(tz >= h);
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        uint32_t v = c[j];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
        if ((threadIdx.x & 63u) == 0 && v) atomicAdd(&acc[j], v);
    }
    __syncthreads();
    if (threadIdx.x < 7 && acc[threadIdx.x]) atomicAdd(&counts[threadIdx.x], acc[threadIdx.x]);
}

// ... and the per-position state from the two presence arrays: position 2i = data block i, 2i + 1 = parity block i; surviving parity blocks
// off the multiples of `unused_mask` + 1 are UNUSED (roots of the locator like lost ones).  parity_lost[i] = 1 for a lost parity block.
__global__ __launch_bounds__(256) void standard_state_kernel(const uint8_t* __restrict__ pd, const uint8_t* __restrict__ pp, uint32_t N, uint32_t unused_mask,
                                                             uint8_t* __restrict__ state, uint32_t* __restrict__ parity_lost)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const uint32_t held_p = pp[i] != 0;
    const uint32_t sd = pd[i] != 0 ? ST_HELD : ST_LOST;
    const uint32_t sp = !held_p ? ST_LOST : (i & unused_mask) ? ST_UNUSED : ST_HELD;
    reinterpret_cast<uint16_t*>(state)[i] = (uint16_t)(sd | (sp << 8));
    parity_lost[i] = 1u - held_p;
}

// roots[i] = w^erased[i] for i < n_erased, 0 for the padding up to T (a factor x: it only shifts the locator)
__global__ __launch_bounds__(256) void roots_kernel(uint32_t* __restrict__ roots, const uint32_t* __restrict__ erased,
                                                    const uint32_t* __restrict__ wpow, uint32_t n_erased, uint32_t T)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < T) roots[i] = i < n_erased ? wpow[erased[i]] : 0u;
}

// Leaves: polynomial p = prod_{j < leaf} (x - roots[p*leaf + j]), monic of degree `leaf`; its other coefficients go to
// x[i * m + p], i < leaf (m = T / leaf polynomials side by side).
__global__ __launch_bounds__(256) void leaf_products_kernel(const uint32_t* __restrict__ roots, uint32_t* __restrict__ x, uint32_t leaf, uint32_t m)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    uint32_t c[LEAF + 1];
#pragma unroll
    for (int i = 0; i <= LEAF; ++i) c[i] = i == 0 ? 1u : 0u;
    for (uint32_t j = 0; j < leaf; ++j) {
        const uint32_t r = roots[p * leaf + j];
#pragma unroll
        for (int i = LEAF; i >= 1; --i) c[i] = gf::sub(c[i - 1], gf::mul(r, c[i]));  // c <- c * (x - r)
        c[0] = gf::sub(0u, gf::mul(r, c[0]));
    }
    for (uint32_t i = 0; i < leaf; ++i) x[i * m + p] = c[i];
}

// The lowest LOW levels of the product tree in ONE kernel (the per-level form costs six launches of 5-9 us per level whatever the size):
// a workgroup takes 2^LOW roots and multiplies the monic polynomials pairwise in LDS by the schoolbook rule, degree 1 -> 2 -> ... -> 2^LOW
// ((x^d + a)(x^d + b) = x^2d + x^d (a + b) + a b; 2^(LOW-1) (2^LOW - 1) products per workgroup, 524 K at LOW = 10), and writes the result where
// level LOW of the tree expects it: coefficient i of polynomial p at x[i * m + p], m = T >> LOW (the upper half of the 2 * 2^LOW rows is zero).
template <int LOW>
__global__ __launch_bounds__(1 << LOW) void tree_low_levels_kernel(const uint32_t* __restrict__ roots, uint32_t* __restrict__ x, uint32_t m)
{
    constexpr uint32_t R = 1u << LOW;  // one thread per coefficient
    __shared__ uint32_t buf[2][R];
    const uint32_t p = blockIdx.x, o = threadIdx.x;
    buf[0][o] = gf::sub(0u, roots[p * R + o]);  // x - r
    __syncthreads();
    int cur = 0;
    for (uint32_t d = 1; d < R; d <<= 1) {
        const uint32_t t = o & (2u * d - 1u);
        const uint32_t* a = buf[cur] + (o - t);
        const uint32_t* b = a + d;
        const uint32_t lo_i = t >= d ? t - d + 1u : 0u, hi_i = t < d ? t : d - 1u;
        // the products are summed as exact integers (96 bits: at most 2^(LOW-1) terms below 2^64) and reduced once per coefficient
        uint64_t lo = t >= d ? (uint64_t)a[t - d] + b[t - d] : 0ull;
        uint32_t hi = 0;
        uint32_t i = lo_i;
        for (; i + 3u <= hi_i; i += 4u) {  // four products per turn: the LDS reads of a turn are in flight together
            const uint32_t a0 = a[i], a1 = a[i + 1], a2 = a[i + 2], a3 = a[i + 3];
            const uint32_t b0 = b[t - i], b1 = b[t - i - 1], b2 = b[t - i - 2], b3 = b[t - i - 3];
            uint64_t pr = (uint64_t)a0 * b0;
            lo += pr, hi += lo < pr;
            pr = (uint64_t)a1 * b1;
            lo += pr, hi += lo < pr;
            pr = (uint64_t)a2 * b2;
            lo += pr, hi += lo < pr;
            pr = (uint64_t)a3 * b3;
            lo += pr, hi += lo < pr;
        }
        for (; i <= hi_i; ++i) {  // (t = 2d - 1: lo_i > hi_i, no product)
            const uint64_t pr = (uint64_t)a[i] * b[t - i];
            lo += pr, hi += lo < pr;
        }
        const uint32_t l0 = (uint32_t)lo, l1 = (uint32_t)(lo >> 32);
        uint32_t acc = gf::add(l0 >= gf::P ? l0 - gf::P : l0, gf::mul(l1 >= gf::P ? l1 - gf::P : l1, gf::MONT_ONE));  // 2^32 mod p
        acc = gf::add(acc, gf::mul(hi, gf::MONT_R2));                                                              // 2^64 mod p
        buf[cur ^ 1][o] = acc;
        __syncthreads();
        cur ^= 1;
    }
    x[(size_t)o * m + p] = buf[cur][o];
}

// y[i][q] = f[i][2q] * f[i][2q+1] * scale (rows of pitch m, m/2 results per row); scale = 1 / (2d) in Montgomery form
__global__ __launch_bounds__(256) void pointwise_pairs_kernel(const uint32_t* __restrict__ f, uint32_t* __restrict__ y, uint32_t m, uint64_t total,
                                                              uint32_t scale_mont)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const uint32_t half = m >> 1;
    const uint64_t i = t / half;
    const uint32_t q = (uint32_t)(t - i * half);
    const uint2 v = *reinterpret_cast<const uint2*>(f + i * m + 2 * q);
    y[i * m + q] = gf::mul_mont(gf::mul(v.x, v.y), scale_mont);
}

// (x^d + a)(x^d + b) = x^2d + x^d (a + b) + a b: the next level's polynomials from the cyclic products a b (y, rows of
// pitch m) and this level's a, b (xold, [d][m]); xnew is [4d][m/2] with the upper 2d rows zero (room for the next product)
__global__ __launch_bounds__(256) void combine_kernel(const uint32_t* __restrict__ y, const uint32_t* __restrict__ xold, uint32_t* __restrict__ xnew,
                                                      uint32_t d, uint32_t m, uint64_t total, bool top)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const uint32_t half = m >> 1;
    const uint64_t i = t / half;
    const uint32_t q = (uint32_t)(t - i * half);
    uint32_t v = 0;
    if (i < 2ull * d) {
        v = y[i * m + q];
        if (i >= d) v = gf::add(v, gf::add(xold[(i - d) * m + 2 * q], xold[(i - d) * m + 2 * q + 1]));
    } else if (top) {
        return;  // the last level has no upper half
    }
    xnew[i * half + q] = v;
}

// ---- transforms of FEW columns (the locator's own: 2; the tree's top levels: 2, 4, 8 polynomials side by side) ----
// The stripe kernels give a wave 64 or more words of one row; with E words per row most lanes idle and a row is a 4 E-byte access.  The rows x E
// array is taken as N1 x (N2 E), N2 E = CHUNK words, as in the four-step method: the N1-point transform over the upper row bits is the stripe kernels'
// (a chunk's words are its columns: uniform twiddles, wide accesses); this kernel, one workgroup per chunk c = bitrev(k1), does the rest inside LDS with
// per-lane twiddles from the decoder's w^u table: DIF (natural rows in, bit-reversed out; runs AFTER the stripe kernels): times w_N^(i2 k1), then
// the N2-point DIF over i2; DIT with the inverse roots (bit-reversed in, natural out; runs BEFORE them): the N2-point DIT, then times w_N^(-i2 k1).
// Either way rows end up where the stripe kernels' passes alone would leave them.
constexpr int CHUNK_LOG = 12, CHUNK = 1 << CHUNK_LOG;
constexpr uint64_t NARROW_COLUMNS = 4;  // tree levels of at most this many polynomials go this way
template <bool DIT>
__global__ __launch_bounds__(256) void chunk_transform_kernel(uint32_t* __restrict__ data, const uint32_t* __restrict__ wpow, int logE, int logN1, uint32_t step_n,
                                                              uint32_t step_n2, uint32_t nc_mask)
{
    __shared__ uint32_t lds[CHUNK], tw[CHUNK / 2];  // the chunk; w_N2^(+-j) for j < N2 / 2 in Montgomery form
    const uint32_t tid = threadIdx.x, k1 = __brev(blockIdx.x) >> (32 - logN1);
    uint32_t* base = data + (size_t)CHUNK * blockIdx.x;
    auto root = [&](uint32_t ex) { return gf::mul_mont(wpow[DIT ? (0u - ex) & nc_mask : ex], gf::MONT_R2); };
    const int levels = CHUNK_LOG - logE;
    const uint32_t half_rows = 1u << (levels - 1);
    for (uint32_t j = tid; j < half_rows; j += 256u) tw[j] = root(j * step_n2);
#pragma unroll
    for (int r = 0; r < CHUNK / 256; ++r) {
        const uint32_t i = r * 256u + tid;
        uint32_t v = base[i];
        if (!DIT) v = gf::mul_mont(v, root((i >> logE) * k1 * step_n));
        lds[i] = v;
    }
    __syncthreads();
    for (int s = 0; s < levels; ++s) {
        // rows r and r + h, h = 2^s (DIT, bottom up) or N2 >> (s + 1) (DIF, top down); twiddle w_2h^(r mod h) = w_N2^((r mod h) N2 / 2h)
        const int hb = DIT ? logE + s : CHUNK_LOG - 1 - s, sh = DIT ? levels - 1 - s : s;
        const uint32_t low = (1u << hb) - 1u;
#pragma unroll
        for (int r = 0; r < CHUNK / 512; ++r) {
            const uint32_t b = r * 256u + tid, i = ((b >> hb) << (hb + 1)) | (b & low), j = i + low + 1u;
            const uint32_t x = lds[i], y = lds[j], w = tw[((i & low) >> logE) << sh];
            if (DIT) {
                const uint32_t t = gf::mul_mont(y, w);
                lds[i] = gf::add(x, t);
                lds[j] = gf::sub(x, t);
            } else {
                lds[i] = gf::add(x, y);
                lds[j] = gf::mul_mont(gf::sub(x, y), w);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < CHUNK / 256; ++r) {
        const uint32_t i = r * 256u + tid;
        uint32_t v = lds[i];
        if (DIT) v = gf::mul_mont(v, root((i >> logE) * k1 * step_n));
        base[i] = v;
    }
}

// lv[m][0] = c_m, lv[m][1] = m c_m for the locator L = x^T + sum_{m<T} c_m x^m taken modulo x^NC - 1 (exact on the NC-th
// roots of unity): the two columns whose transforms are L(w^u) and (x L')(w^u)
__global__ __launch_bounds__(256) void locator_columns_kernel(const uint32_t* __restrict__ c, uint32_t* __restrict__ lv, uint32_t T, uint32_t NC)
{
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= NC) return;
    uint32_t v0 = m < T ? c[m] : 0u;
    uint32_t v1 = gf::mul(m, v0);
    if (m == T % NC) {  // the monic term x^T (T == NC wraps onto x^0)
        v0 = gf::add(v0, 1u);
        v1 = gf::add(v1, T % gf::P);
    }
    lv[2 * m] = v0;
    lv[2 * m + 1] = v1;
}

// From the values L(w^u), (x L')(w^u) of the padded locator L = x^pad l to the decoder's tables:
//   fin[u]  = l(w^u) (Montgomery) on surviving positions, 0 elsewhere           l(w^u) = L(w^u) w^(-u pad)
//   gout[i] = 1 / (w^u l'(w^u)) (Montgomery) for erased data block i at u = i << e   (x l')(w^u) = (x L')(w^u) w^(-u pad) there
__global__ __launch_bounds__(256) void finish_tables_kernel(const uint32_t* __restrict__ lv, const uint32_t* __restrict__ state,
                                                            const uint32_t* __restrict__ wpow, uint32_t* __restrict__ fin, uint32_t* __restrict__ gout,
                                                            uint32_t NC, uint32_t pad, int e, uint32_t user_k, uint32_t q, int lg2,
                                                            uint32_t* __restrict__ gout_par = nullptr, bool lv_bitrev = false)
{
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= NC) return;
    const uint32_t st = (state[u >> 2] >> (8 * (u & 3u))) & 0xFFu;
    const uint32_t back = (uint32_t)(((uint64_t)u * pad) % NC);
    const uint32_t corr = wpow[back == 0 ? 0 : NC - back];  // w^(-u pad)
    // where the two values for w^u sit in lv: position u for the power-of-two transform (natural order out); the way down
    // of a mixed-radix context (mixed_dif) leaves the value at w^(-v), v = q * bitrev(r) + j1, in block j1 * 2^lg2 + r
    uint32_t at = lv_bitrev ? (__brev(u) >> (32 - lg2)) : u;  // (power of two, transform_bitrev: the value for w^u sits at the bit-reversed position)
    if (q > 1) {
        const uint32_t v = u == 0 ? 0u : NC - u;
        at = (v % q << lg2) + (__brev(v / q) >> (32 - lg2));
    }
    fin[u] = st == ST_HELD ? gf::mul(gf::mul(lv[2 * at], corr), gf::MONT_ONE) : 0u;
    if ((u & ((1u << e) - 1u)) == 0) {
        const uint32_t i = u >> e;
        uint32_t g = 0;
        if (st == ST_LOST && i < user_k) g = gf::mul(dev_pow(gf::mul(lv[2 * at + 1], corr), gf::P - 2u), gf::MONT_ONE);
        gout[i] = g;
    } else if (gout_par) {  // (2k,k) layout: odd u is parity block u >> 1
        gout_par[u >> 1] = st == ST_LOST ? gf::mul(dev_pow(gf::mul(lv[2 * at + 1], corr), gf::P - 2u), gf::MONT_ONE) : 0u;
    }
}

// split transform: the per-block factors of the two half stripes in the order the first pass reads them, from fin (by codeword position)
__global__ __launch_bounds__(256) void split_rows_kernel(const uint32_t* __restrict__ fin, const uint32_t* __restrict__ gout, const uint32_t* __restrict__ order,
                                                         uint32_t* __restrict__ rows_data, uint32_t* __restrict__ rows_parity, uint32_t* __restrict__ rows_out,
                                                         uint32_t k, const uint32_t* __restrict__ gout_par = nullptr, uint32_t* __restrict__ rows_out_parity = nullptr)
{
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= k) return;
    const uint32_t i = order[slot];
    rows_data[slot] = fin[2u * i];
    rows_parity[slot] = fin[2u * i + 1u];
    rows_out[slot] = gout[i];  // the last pass has the first one's tile shape, so its blocks come in the same order
    if (rows_out_parity) rows_out_parity[slot] = gout_par[i];
}
// ... and the factor of the parity half's coefficients, by position: -w^(-m) / 2 (Montgomery) at position bitrev(m); wpow[u] = w^u, w of order 2k
// (forward: w^m instead — the factor of the data half's coefficients in the parity chain of fastecc_repair)
__global__ __launch_bounds__(256) void split_pos_kernel(const uint32_t* __restrict__ wpow, uint32_t* __restrict__ pos, uint32_t k, int lg, uint32_t neg_half,
                                                        bool forward)
{
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= k) return;
    const uint32_t w = wpow[forward ? m : (m == 0 ? 0 : 2u * k - m)];
    pos[__brev(m) >> (32 - lg)] = gf::mul(gf::mul(w, neg_half), gf::MONT_ONE);
}

__global__ __launch_bounds__(256) void permute_kernel(const uint32_t* __restrict__ src, const uint32_t* __restrict__ order, uint32_t* __restrict__ dst,
                                                      uint32_t count)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) dst[i] = src[order[i]];
}

// ---- fastecc_decode_prepare ----
// The 64-bit field has its own decoder (gf61_decode.hip); its contexts are (2k,k), (4k,k) or (8k,k) with k a power of two (and their zero-extended
// relatives), n = 4k / 8k the same decoder on the (k << e)-th roots of unity
int prepare_p61(fastecc_ctx* c, const uint8_t* data_present, const uint8_t* parity_present)
{
    DeviceGuard dg(c->device);
    if (!dg.ok) return FASTECC_E_DEVICE;
    CallLock lk(c->mu);
    const int rc0 = wait_idle(c);  // a decode still using the previous pattern
    if (rc0 != FASTECC_OK) return rc0;
    char detail[160] = "";
    // codes other than (2N,N): the decoder sees the (2N,N) codeword — data blocks beyond the caller's k are surviving zero blocks,
    // parity positions the code does not use are lost (which is what limits the losses to n - k)
    std::vector<uint8_t> dfull, pfull;
    if (zero_extended(c)) {
        dfull.assign(c->N, 1);
        pfull.assign(c->N, 0);
        for (uint64_t i = 0; i < c->K; i++) dfull[i] = data_present[i] ? 1 : 0;
        for (uint64_t q = 0; q < c->Mu; q++) pfull[q * (uint64_t)c->p61_stride] = parity_present[q] ? 1 : 0;
        data_present = dfull.data();
        parity_present = pfull.data();
    }
    const int rc = p61::decode_prepare(&c->decoder61, c->n, c->S / 4, data_present, parity_present, c->decode_direct_max, detail, sizeof detail,
                                       c->decode_split, code_coset_shift(c->cosets));
    if (rc != FASTECC_OK && detail[0]) (void)hip_fail(hipErrorUnknown, detail);  // (the message of a failed p61::create*; the code stays p61's)
    return rc;
}

// The parity half's low levels when few block groups are in use (run_split_decode): what the DIF levels with strides 512 ... 16 make of a
// 1024-block tile in which block q0 alone is 1 — simulated here exactly as the tile does them, (a, b) -> (a + b, (a - b) w_2s^i) with the inverse
// roots; entry [t][g][c] = block g + 16 c for q0 = g + 16 t (Montgomery form).  w: of order 2N.
std::vector<uint32_t> split_impulse_table(uint32_t w, uint64_t N)
{
    const uint32_t w1024_inv = gf::h_pow(gf::h_inv(gf::h_mul(w, w)), N / 1024);
    const uint32_t tables = (uint32_t)split_impulse_max();
    std::vector<uint32_t> table((size_t)tables * 16 * 64), v(1024), tw(512);
    for (uint32_t q0 = 0; q0 < 16u * tables; q0++) {
        std::fill(v.begin(), v.end(), 0u);
        v[q0] = 1;
        for (uint32_t sdist = 512; sdist >= 16; sdist >>= 1) {
            const uint32_t root = gf::h_pow(w1024_inv, 512 / sdist);  // order 2 * sdist
            tw[0] = 1;
            for (uint32_t i = 1; i < sdist; i++) tw[i] = gf::h_mul(tw[i - 1], root);
            for (uint32_t base = 0; base < 1024; base += 2 * sdist)
                for (uint32_t i = 0; i < sdist; i++) {
                    const uint32_t lo = v[base + i], hi = v[base + i + sdist];
                    if ((lo | hi) == 0) continue;
                    v[base + i] = (uint32_t)(((uint64_t)lo + hi) % gf::P);
                    v[base + i + sdist] = gf::h_mul((uint32_t)(((uint64_t)lo + gf::P - hi) % gf::P), tw[i]);
                }
        }
        const uint32_t t = q0 / 16, g0 = q0 % 16;
        for (uint32_t cc = 0; cc < 64; cc++) table[(t * 16 + g0) * 64 + cc] = gf::h_to_mont(v[g0 + 16 * cc]);
    }
    return table;
}

// What the pattern scan of the transform path found
struct PatternScan {
    bool device_scan = false;      // the (2k,k) layout's scan ran on the device: the state and the lost-parity flags are written there
    std::vector<uint8_t> state;    // host scan: ST_* per position
    std::vector<uint32_t> srcmap;  // host scan, layouts other than (2k,k): the block at each position (the table-driven gather's map)
    uint64_t erased_data = 0, erased_parity = 0;  // lost blocks
    uint64_t erased_count = 0;                    // roots of the locator: lost or unused positions and those that hold no block of the code
    uint32_t split_groups = 0;  // non-zero: the pattern goes through the split transform — parity block groups in use (1 for the small form)
    uint32_t split_shift = 0;   // the small form's shift (0: the group form)
};

// One fastecc_decode_prepare of a GF(0xFFF00001) code.  Every code is f on a subset of the NC-th roots of unity, NC = N << e (position u <->
// w_NC^u): data block i at i << e (blocks k..N-1 of a zero-extended code are known zero blocks), parity at the positions fastecc_create documents —
// odd multiples of 2^fold for the codes inside (2N,N), the cosets' offsets for n = 4k / 8k.  Positions that hold no block of the code count as
// erased, which is exactly what limits the losses to n - k.  Mixed-radix codes (fastecc_create_ex): the same scheme on the (2 q 2^m)-th roots of
// unity; the decoder's transform is a mixed-radix context one size up, the locator's values come from the way down of another one (mixed_dif).
struct Prepare {
    fastecc_ctx* c;
    const uint8_t* data_present;
    const uint8_t* parity_present;
    bool mixed;     // mixed radix
    uint64_t N;     // the transform order
    int e;          // data block i at position i << e
    uint64_t NC;    // positions
    int lgc;        // log2k + e
    bool standard;  // the reference's (2k,k) layout
    bool narrow;    // NC is a power of two: the w^u table holds every root the chunks of chunk_transform_kernel need
    DecodeState* d = nullptr;
    PatternScan s;
    // The locator's product tree.  T = padded root count: the smallest power of two that holds the most losses the code tolerates, NC - N (the
    // top of the tree is a cyclic product of length T, so w_T must exist: T <= 2^20.  Orders above 2^20 — mixed radix — tolerate more losses than
    // that; there T = 2^20 and patterns with more erasures than T are refused.)  The levels below 2^TREE_LOW roots per polynomial are one kernel
    // (tree_low_levels_kernel) when the tree is tall enough to have them.
    uint64_t T = 1;
    int lgT = 0, leaf_log = 0;
    // parity block j at position 2j + 1 (the (2k,k) layout and its zero-extended relatives with fold 0): a pattern that loses data AND parity
    // gets the factors of its lost parity blocks too — fastecc_repair then needs no second encode
    bool parity_factors = false;
    PhaseTimer pt;

    Prepare(fastecc_ctx* ctx, const uint8_t* dp, const uint8_t* pp)
        : c(ctx), data_present(dp), parity_present(pp), mixed(c->q > 1), N(transform_order(c)), e(code_coset_shift(c->cosets)), NC(N << e), lgc(c->n + e),
          standard(!mixed && c->cosets == 1 && c->fold == 0 && !zero_extended(c)),
          narrow(!mixed && (1ull << lgc) == NC)
    {
    }
    uint64_t parity_position(uint64_t q) const { return code_parity_position(N, e, c->fold, c->cosets, q); }
    void new_pattern(uint64_t erased_data)  // (the previous pattern is dropped)
    {
        d->pattern.ready = false;
        d->pattern.erased_data = erased_data;
        d->pattern.positions = NC;
        d->pattern.standard = standard;
        d->pattern.mixed = mixed;
    }

    // ---- few losses: interpolation on the surviving data points + a few parity points (direct.hip) ----
    // The most lost blocks for the direct path.  The matrix-core kernel recomputes 256 blocks in a third of the transform path's time, the VALU
    // kernel breaks even near 128 (profiles/r03/direct_bench.jsonl); stripes the MFMA kernel cannot take (odd or short rows) stop at 96 unless a
    // kernel was asked for — at 80 where the split transform (4.3 ms instead of 7.2 at k = 2^19 x 4 KB) is the alternative.
    int direct_limit() const
    {
        int limit = std::min(c->decode_direct_max, direct_cap());
        const bool split_applies = c->decode_split && c->q <= 1 && c->cosets == 1 && c->n >= 17;
        if (c->direct_kernel == 0 && !direct_mfma_applies(nullptr, nullptr, c->S)) limit = std::min(limit, split_applies ? 80 : 96);
        // orders above 2^20 (mixed radix): the locator tree is padded to 2^20 roots whatever the pattern
        uint64_t T20 = 1;
        while (T20 < NC - N) T20 <<= 1;
        // their tree costs a 2^20-point product: the direct path first, up to the caller's "decode_direct_max" (the 80 / 96 cap of rows the
        // matrix-core kernel cannot take is a speed trade-off against a transform path that is much dearer here, so it does not apply)
        if (T20 > (1ull << 20) && c->decode_direct_max > 0) limit = std::max(limit, std::min(c->decode_direct_max, direct_cap()));
        return limit;
    }

    // Every lost data block is a fixed linear combination of the surviving data blocks and as many surviving parity blocks, the lost parity blocks
    // one of the data; decided before any per-position table is built.  *done = false: too many losses, or no memory for the weight tables —
    // the transform path needs none of them.
    int direct(bool* done)
    {
        *done = false;
        const int limit = direct_limit();
        if (limit <= 0 || c->K >= 0xFFFFFFF0ull) return FASTECC_OK;
        PhaseTimer ptd;
        std::vector<uint32_t> R, Pl, A;  // lost data blocks, lost parity blocks, the surviving parity blocks that serve as nodes
        bool over = false;
        each_lost(data_present, c->K, [&](uint64_t i) { R.push_back((uint32_t)i); return !(over = (int)R.size() > limit); });
        if (!over) each_lost(parity_present, c->Mu, [&](uint64_t q) { Pl.push_back((uint32_t)q); return !(over = (int)(R.size() + Pl.size()) > limit); });
        for (uint64_t q = 0; q < c->Mu && !over && A.size() < R.size(); q++)
            if (parity_present[q]) A.push_back((uint32_t)q);
        if (over || R.size() + Pl.size() < 1 || A.size() != R.size()) return FASTECC_OK;
        const int ed = (int)R.size(), ep = (int)Pl.size();
        ptd.mark("few losses: pattern scan");
        DeviceGuard dg(c->device);
        if (!dg.ok) return FASTECC_E_DEVICE;
        CallLock lk(c->mu);
        if (!(d = state_of(c))) return FASTECC_E_NOMEM;
        new_pattern(ed);
        d->pattern.direct_path = false;
        d->pattern.erased_parity = ep;
        d->pattern.direct_kernel = c->direct_kernel;
        int rc = wait_idle(c);  // a decode still using the previous pattern
        if (rc != FASTECC_OK) return rc;
        ptd.mark("few losses: lock, idle");
        rc = direct_tables(CodeGeometry(c), R, Pl, A, d->few.direct, ptd);
        if (rc == FASTECC_E_NOMEM && !d->few.direct.host_nomem) return FASTECC_OK;  // no memory for the weight tables: the transform path
        if (rc != FASTECC_OK) return rc;
        d->pattern.direct_path = true;  // (from here on the calls read d->few.direct: the passes, both_built, only_both, ed, ep)
        d->host.lost_data = R;  // (FASTECC_MEM_HOST calls: the rows that travel back)
        d->host.lost_parity = Pl;
        d->host.parity_used = A;
        d->host.lists_of = ++d->pattern.serial;
        d->pattern.ready = true;
        *done = true;
        return FASTECC_OK;
    }

    // ---- the transform path ----
    int transform_path()
    {
        pt = PhaseTimer();
        DeviceGuard dg(c->device);
        if (!dg.ok) return FASTECC_E_DEVICE;
        CallLock lk(c->mu);  // (held from here on: the device scan already writes the context's pattern state)
        if (!(d = state_of(c))) return FASTECC_E_NOMEM;
        int rc;
        if (standard && N <= 0x7FFFFFFFull && (rc = scan_device()) != FASTECC_OK) return rc;
        if (!s.device_scan) scan_host();
        if (s.erased_count > NC - N) return FASTECC_E_INVAL;  // fewer than k blocks survive: not decodable
        pt.mark(s.device_scan ? "pattern scan (device)" : "pattern scan (host)");
        if ((rc = set_pattern()) != FASTECC_OK) return rc;
        if (s.erased_data == 0) {  // no data block to recover
            // standard_state_kernel's writes of the lost-parity flags are still pending on the null stream: a repair on a non-blocking
            // stream is not ordered after them (the full path below ends with the same synchronise)
            if (s.device_scan) HIP_TRY(hipStreamSynchronize(nullptr));
            d->pattern.ready = true;
            return FASTECC_OK;
        }
        while (T < NC - N && T < (1ull << 20)) T <<= 1;
        while ((1ull << lgT) < T) lgT++;
        if (s.erased_count > T) return FASTECC_E_UNSUPPORTED;
        leaf_log = lgT >= TREE_LOW + 2 ? TREE_LOW : std::min(LEAF_LOG, lgT);
        parity_factors = d->pattern.erased_parity != 0 && (d->pattern.standard || (s.split_groups != 0 && c->fold == 0));
        if ((rc = build_shape()) != FASTECC_OK) return rc;
        if ((rc = wait_idle(c)) != FASTECC_OK) return rc;  // a decode still using the previous pattern
        pt.mark("tables, tile order");
        uint32_t* coeffs = nullptr;
        if ((rc = locator_tree(&coeffs)) != FASTECC_OK || (rc = locator_tables(coeffs)) != FASTECC_OK) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        pt.mark("this pattern (device)");
        d->pattern.ready = true;
        return FASTECC_OK;
    }

    // The reference's (2k,k) layout: the pattern is scanned on the DEVICE (the host loops of scan_host took 1.2-1.4 ms of a 2.6 ms call at k = 2^19:
    // four passes over a million byte-sized coin flips).  Two 512 KB uploads, one counting kernel, 32 bytes back; the per-position state and the
    // lost-parity flags are then written by a kernel.  Patterns the "small form" of the split transform does not take (too few surviving parity
    // blocks at multiples of 2^h) leave s as it is: the host scan.
    int scan_device()
    {
        RC_TRY(d->tables.dev_present.alloc(2 * N));
        RC_TRY(d->tables.dev_counts.alloc(8));
        RC_TRY(d->tables.dev_state.alloc(NC));
        RC_TRY(d->tables.parity_lost.alloc(c->Mu));
        RC_TRY(wait_idle(c));  // a decode or repair still reading the previous pattern's state
        d->pattern.ready = false;
        HIP_TRY(hipMemcpyAsync(d->tables.dev_present, data_present, N, hipMemcpyHostToDevice, nullptr));
        HIP_TRY(hipMemcpyAsync(d->tables.dev_present + N, parity_present, N, hipMemcpyHostToDevice, nullptr));
        HIP_TRY(hipMemsetAsync(d->tables.dev_counts, 0, 8 * 4, nullptr));
        hipLaunchKernelGGL(presence_counts_kernel, dim3(128), dim3(256), 0, nullptr, d->tables.dev_present, d->tables.dev_present + N, (uint32_t)N, d->tables.dev_counts);
        HIP_TRY(hipGetLastError());
        uint32_t counts[8] = {};
        HIP_TRY(hipMemcpy(counts, d->tables.dev_counts, sizeof counts, hipMemcpyDeviceToHost));
        const uint64_t erased_data = counts[0], erased_parity = counts[1];
        uint32_t shift = 0;
        const bool want_split = c->decode_split && c->n >= 17 && erased_data != 0;
        if (want_split && c->decode_split != 2)
            for (int h = 5; h >= 1 && shift == 0; h--)
                if (counts[1 + h] >= erased_data) shift = (uint32_t)h;
        if (want_split && shift == 0) return FASTECC_OK;  // the host path counts again
        s.device_scan = true;
        s.erased_data = erased_data;
        s.erased_parity = erased_parity;
        s.erased_count = erased_data + erased_parity + (shift ? (N - erased_parity) - counts[1 + shift] : 0);
        s.split_shift = shift;
        s.split_groups = shift ? 1u : 0u;
        hipLaunchKernelGGL(standard_state_kernel, grid_of(N), dim3(256), 0, nullptr, d->tables.dev_present, d->tables.dev_present + N, (uint32_t)N,
                           shift ? (1u << shift) - 1u : 0u, d->tables.dev_state, d->tables.parity_lost);
        HIP_TRY(hipGetLastError());
        return FASTECC_OK;
    }

    // The pattern scanned on the host.  (Branch-free loops: on a random pattern every "if (present)" is a coin flip — 2^20 mispredictions were
    // most of this call's time at 50 % loss.)
    void scan_host()
    {
        std::vector<uint8_t>& state = s.state;
        state.assign(NC, ST_LOST);
        if (standard) {  // (the (2k,k) layout reads its two stripes by position: no block map)
            for (uint64_t i = 0; i < N; i++) {
                const uint32_t held_d = data_present[i] != 0, held_p = parity_present[i] != 0;
                state[2 * i] = held_d ? ST_HELD : ST_LOST;
                state[2 * i + 1] = held_p ? ST_HELD : ST_LOST;
                s.erased_data += 1u - held_d;
                s.erased_parity += 1u - held_p;
            }
        } else {
            std::vector<uint32_t>& srcmap = s.srcmap;
            srcmap.assign(NC, 0);
            for (uint64_t i = 0; i < c->K; i++) {
                const uint64_t u = i << e;
                const uint32_t held = data_present[i] != 0;
                state[u] = held ? ST_HELD : ST_LOST;
                srcmap[u] = (uint32_t)i & (0u - held);
                s.erased_data += 1u - held;
            }
            for (uint64_t i = c->K; i < N; i++) state[i << e] = ST_ZERO;
            for (uint64_t q = 0; q < c->Mu; q++) {
                const uint64_t u = parity_position(q);
                const uint32_t held = parity_present[q] != 0;
                state[u] = held ? ST_HELD : ST_LOST;
                srcmap[u] = ((uint32_t)q | 0x80000000u) & (0u - held);
                s.erased_parity += 1u - held;
            }
        }
        if (c->decode_split && !mixed && c->cosets == 1 && c->n >= 17 && s.erased_data != 0) choose_split();
        if (s.split_groups != 0 && !s.srcmap.empty())
            for (uint64_t u = 1; u < NC; u += 2) s.srcmap[u] &= 0u - (uint32_t)(state[u] != ST_UNUSED);
        // the erased positions themselves are listed on the device (erased_list_kernel): the host needs their number only
        for (uint64_t u = 0; u < NC; u++) s.erased_count += (unsigned)(state[u] == ST_LOST) + (unsigned)(state[u] == ST_UNUSED);
    }

    // (2k,k) layout, split transform: recovering e lost data blocks takes e parity blocks, not all of them — the surviving parity blocks of the
    // first few block groups of the parity stripe (group g = blocks g + (t << 10): what one tile of the first pass reads).  The others are left
    // unread: roots of the locator like the lost ones.  (Also the zero-extended codes inside (2N,N): data block i at position 2i, parity block j at
    // 2j + 1, fewer blocks than N in either stripe; and the codes with fewer parity blocks: parity block j at position 2 (j << fold) + 1, i.e.
    // block j << fold of the parity half.)
    void choose_split()
    {
        std::vector<uint8_t>& state = s.state;
        // first choice: the surviving parity blocks at multiples of 2^h of the parity half, the largest h <= 5 that still leaves as many as there
        // are lost data blocks (2 % of the codeword lost: h = 5) — r~ is then the transform of k >> h rows (see DecodeState::split_shift)
        uint64_t at_multiple[6] = {};
        for (uint64_t q = 0; q < c->Mu; q++) {
            if (!parity_present[q]) continue;
            const uint64_t hpos = q << c->fold;
            for (int h = 1; h <= 5 && (hpos & ((1ull << h) - 1ull)) == 0; h++) at_multiple[h]++;
        }
        for (int h = 5; h >= 1 && s.split_shift == 0; h--)
            if (at_multiple[h] >= s.erased_data && c->decode_split != 2) s.split_shift = (uint32_t)h;
        if (s.split_shift != 0) {
            const uint64_t mask = (1ull << s.split_shift) - 1ull;
            for (uint64_t q = 0; q < N; q++)
                if ((q & mask) != 0 && state[2 * q + 1] == ST_HELD) state[2 * q + 1] = (uint8_t)ST_UNUSED;
            s.split_groups = 1;
            return;
        }
        constexpr uint32_t GROUPS = 1024;
        uint32_t held_in[GROUPS] = {};
        for (uint64_t q = 0; q < c->Mu; q++) held_in[(q << c->fold) & (GROUPS - 1u)] += parity_present[q] != 0;
        uint64_t have = 0;
        while (s.split_groups < GROUPS && have < s.erased_data) have += held_in[s.split_groups++];
        if (have < s.erased_data) {
            s.split_groups = 0;  // not decodable: refused by the caller
            return;
        }
        for (uint64_t q0 = 0; q0 < N; q0 += GROUPS)  // (the blocks of the groups in use keep their state)
            for (uint64_t q = q0 + s.split_groups; q < q0 + GROUPS; q++) state[2 * q + 1] = state[2 * q + 1] == ST_HELD ? (uint8_t)ST_UNUSED : state[2 * q + 1];
    }

    // the pattern's counts into the decoder's state (the previous pattern is dropped) and the lost-parity flags of a host scan to the device
    int set_pattern()
    {
        new_pattern(s.erased_data);
        pt.mark("lock, state");
        d->pattern.erased_parity = s.erased_parity;
        if (!s.device_scan) {
            std::vector<uint32_t> plost(c->Mu);
            for (uint64_t q = 0; q < c->Mu; q++) plost[q] = parity_present[q] ? 0u : 1u;
            RC_TRY(d->tables.parity_lost.alloc(c->Mu));
            RC_TRY(wait_idle(c));  // a repair still reading the previous pattern
            HIP_TRY(hipMemcpy(d->tables.parity_lost, plost.data(), c->Mu * 4, hipMemcpyHostToDevice));
        }
        pt.mark("lost-parity flags");
        d->pattern.direct_path = false;
        ++d->pattern.serial;  // (the lists of rebuilt rows for FASTECC_MEM_HOST calls are made when such a call comes: StripeDecode::stage_host)
        return FASTECC_OK;
    }

    // Everything that outlives a pattern, built once per context or shape: contexts, tree buffers, tables, the split transform and its buffers,
    // the one-transform repair's context, the tile order.  May clear s.split_groups (split_buffers).
    int build_shape()
    {
        int rc = build_transforms();
        if (rc != FASTECC_OK) return rc;
        if ((d->tree.T != T || d->tree.low != leaf_log) && (rc = build_tree()) != FASTECC_OK) return rc;
        pt.mark("tree contexts + buffers");
        if ((rc = build_tables()) != FASTECC_OK) return rc;
        d->split.ready = false;
        d->split.repair_ready = false;
        if (s.split_groups != 0 && !d->split.unavailable && !d->split.ctx && (rc = build_split()) != FASTECC_OK) return rc;
        if (s.split_groups != 0 && d->split.ctx && (rc = split_buffers()) != FASTECC_OK) return rc;
        if (d->pattern.standard && d->pattern.erased_parity != 0 && !(s.split_groups != 0 && d->split.ctx) && !d->tables.transform_full) {
            // repair in one transform (see DecodeState::transform_full): the form for patterns or plans the split transform does not take
            rc = create_ramp_transform_ctx(d->tables.transform_full.fill(), lgc, c->S * 4, 0, gf::h_inv((uint32_t)NC), c->device);
            if (rc != FASTECC_OK && rc != FASTECC_E_NOMEM) return rc;
            d->tables.full_ok = d->tables.transform_full && same_tile_order(d->tables.transform, d->tables.transform_full);
            if (getenv("FASTECC_TRACE_PREPARE"))
                fprintf(stderr, "[fastecc prepare] one-transform repair: context %s, same first-pass order %d (%s | %s)\n", d->tables.transform_full ? "built" : "none",
                        (int)d->tables.full_ok, fastecc_plan_string(d->tables.transform), d->tables.transform_full ? fastecc_plan_string(d->tables.transform_full) : "");
        }
        if (d->pattern.standard && !d->tables.tile_order_valid) {
            if (same_tile_order(d->tables.transform, d->tables.transform)) {  // (a tile first pass: the order exists)
                RC_TRY(d->tables.tile_order.alloc(NC));
                if (!gather_tile_order_device(d->tables.transform, d->tables.tile_order, nullptr)) return FASTECC_E_DEVICE;
                RC_TRY(d->tables.fin_tiled.alloc(NC));
                d->tables.fin_first_pass = d->tables.fin_tiled;
            } else {
                d->tables.fin_first_pass = d->tables.fin;
            }
            d->tables.tile_order_valid = true;
        }
        if (!d->pattern.standard) d->tables.fin_first_pass = d->tables.fin;
        return FASTECC_OK;
    }

    // the pattern's transform (two columns: l and l') and the decoder's own
    int build_transforms()
    {
        if (!d->tables.pattern_ntt) {
            int rc;
            if (mixed) {
                const std::vector<uint32_t> ones(NC, 1u);
                rc = create_mixed_transform_ctx(d->tables.pattern_ntt.fill(), c->q, lgc, 8, ones.data(), c->device);
            } else {
                // only its stand-alone transform is used; long ones as the upper row bits of a four-step transform (chunk_transform_kernel)
                d->tables.pattern_narrow = narrow && lgc + 1 - CHUNK_LOG >= 1;
                rc = d->tables.pattern_narrow ? create_ntt_ctx(d->tables.pattern_ntt.fill(), lgc + 1 - CHUNK_LOG, 4 * CHUNK, c->device) : create_ntt_ctx(d->tables.pattern_ntt.fill(), lgc, 8, c->device);
            }
            if (rc != FASTECC_OK) return rc;
        }
        pt.mark("pattern_ntt context");
        RC_TRY(d->tables.pattern_buf.alloc(2 * NC));
        if (!d->tables.transform) {
            // x p'(x): coefficient m times m, and the 1/NC of the inverse transform.  fold e: only the data positions (multiples of 2^e) are
            // evaluated (mixed radix: all positions, the even ones are used)
            const uint32_t inv_nc = gf::h_inv((uint32_t)NC);
            int rc;
            if (mixed) {
                std::vector<uint32_t> factor(NC);
                const uint32_t inv_nc_m = gf::h_to_mont(inv_nc);
                for (uint64_t m = 0; m < NC; m++) factor[m] = gf::h_mont_mul((uint32_t)m, inv_nc_m);
                rc = create_mixed_transform_ctx(d->tables.transform.fill(), c->q, lgc, c->S * 4, factor.data(), c->device);
            } else {
                rc = create_ramp_transform_ctx(d->tables.transform.fill(), lgc, c->S * 4, e, inv_nc, c->device);
            }
            if (rc != FASTECC_OK) return rc;
        }
        pt.mark("transform context");
        return FASTECC_OK;
    }

    // the tree's contexts and buffers: level k >= leaf_log multiplies pairs of degree-2^k polynomials — transforms of length 2^(k+1) on T / 2^k columns
    int build_tree()
    {
        d->tree.ctx.clear();
        d->tree.top.reset();
        d->tree.ctx.resize(lgT);
        const bool narrow_tree = narrow && lgT + 1 - CHUNK_LOG >= 1 && lgT > leaf_log;
        for (int lv = leaf_log; lv < lgT; lv++) {
            if (narrow_tree && (T >> lv) <= NARROW_COLUMNS) continue;  // tree_top + chunk_transform_kernel
            const int rc = create_ntt_ctx(d->tree.ctx[lv].fill(), lv + 1, 4 * (T >> lv), c->device);
            if (rc != FASTECC_OK) return rc;
        }
        if (narrow_tree) {
            const int rc = create_ntt_ctx(d->tree.top.fill(), lgT + 1 - CHUNK_LOG, 4 * CHUNK, c->device);
            if (rc != FASTECC_OK) return rc;
        }
        for (DeviceBuf<uint32_t>* b : {&d->tree.x, &d->tree.f, &d->tree.y, &d->tree.p, &d->tree.roots, &d->tree.dev_erased}) b->reset();
        for (DeviceBuf<uint32_t>* b : {&d->tree.x, &d->tree.f, &d->tree.y, &d->tree.p}) RC_TRY(b->alloc(2 * T));
        RC_TRY(d->tree.roots.alloc(T));
        RC_TRY(d->tree.dev_erased.alloc(T + 1));  // + the counter of erased_list_kernel
        d->tree.T = T;
        d->tree.low = leaf_log;
        return FASTECC_OK;
    }

    // the tables by position and block, and the stripe of the recovered blocks
    int build_tables()
    {
        if (!d->tree.wpow) {
            // the table becomes visible to later calls only once the kernel that fills it has been launched without error
            // (an unfilled table behind a non-null pointer would give silently wrong weights on the next prepare)
            DeviceBuf<uint32_t> fresh;
            RC_TRY(fresh.alloc(NC));
            hipLaunchKernelGGL(wpow_kernel, grid_of(NC), dim3(256), 0, nullptr, fresh.get(), gf::h_root((uint32_t)NC), (uint32_t)NC);
            HIP_TRY(hipGetLastError());
            d->tree.wpow = std::move(fresh);
        }
        RC_TRY(d->tables.dev_state.alloc(NC));
        RC_TRY(d->tables.fin.alloc(NC));
        RC_TRY(d->tables.srcmap.alloc(NC));
        RC_TRY(d->tables.gout.alloc(N));
        if (parity_factors) RC_TRY(d->tables.gout_par.alloc(N));
        // mixed radix: the work stripe of all NC positions, transformed in place; else the N recovered data positions
        return d->tables.recovered.alloc((mixed ? NC : N) * c->S);
    }

    // The split transform's context and tables (once).  Anything missing — a plan without the tile shapes, no memory for the two extra stripes —
    // leaves the 2k-point transform in charge for good (split_unavailable); the pattern's unused parity blocks are unused there as well.
    int build_split()
    {
        const int rc = [&]() -> int {
            // per-block factor (2m + k) / 2k = m / k + 1 / 2
            const int rc = create_ramp_transform_ctx(d->split.ctx.fill(), c->n, c->S * 4, 0, gf::h_inv((uint32_t)N), c->device, gf::h_inv(2u));
            if (rc != FASTECC_OK) return rc;
            if (!split_decode_supported(d->split.ctx) || split_decode_groups(d->split.ctx) != 1024u) return FASTECC_E_UNSUPPORTED;
            for (DeviceBuf<uint32_t>* b : {&d->split.order, &d->split.rows_data, &d->split.rows_parity, &d->split.rows_out, &d->split.pos_parity,
                                           &d->split.pos_data_odd, &d->split.rows_out_parity})
                RC_TRY(b->alloc(N));
            if (!gather_tile_order_device(d->split.ctx, d->split.order, nullptr)) return FASTECC_E_UNSUPPORTED;
            const std::vector<uint32_t> table = split_impulse_table(gf::h_root((uint32_t)NC), N);
            RC_TRY(d->split.impulse.alloc(table.size()));
            HIP_TRY(hipMemcpy(d->split.impulse, table.data(), table.size() * 4, hipMemcpyHostToDevice));
            const uint32_t neg_half = (uint32_t)(gf::P - gf::h_inv(2u));
            hipLaunchKernelGGL(split_pos_kernel, grid_of(N), dim3(256), 0, nullptr, d->tree.wpow, d->split.pos_parity, (uint32_t)N, c->n, neg_half, false);
            hipLaunchKernelGGL(split_pos_kernel, grid_of(N), dim3(256), 0, nullptr, d->tree.wpow, d->split.pos_data_odd, (uint32_t)N, c->n, neg_half, true);
            HIP_TRY(hipGetLastError());
            return FASTECC_OK;
        }();
        if (rc == FASTECC_OK) {
            d->split.dirty = 0;
            return FASTECC_OK;
        }
        // nothing half-built stays behind: a later call either builds all of it or none
        (void)hipGetLastError();
        d->split.reset();
        if (rc != FASTECC_E_NOMEM && rc != FASTECC_E_UNSUPPORTED) return rc;
        d->split.unavailable = true;
        return FASTECC_OK;
    }

    // The split transform's work buffers for the parity half, by form.  No memory for them: the 2k-point transform serves this pattern (as for a
    // missing tile shape) and s.split_groups / split_shift are cleared — the pattern's unused parity blocks stay unused, the 2k-point transform
    // reads the same factors.
    int split_buffers()
    {
        hipError_t err = hipSuccess;
        if (s.split_shift != 0) {
            const uint64_t rows = N >> s.split_shift;
            if (!d->split.small[s.split_shift]) {
                const int rc = create_ntt_ctx(d->split.small[s.split_shift].fill(), c->n - (int)s.split_shift, c->S * 4, c->device);
                if (rc != FASTECC_OK && rc != FASTECC_E_NOMEM && rc != FASTECC_E_UNSUPPORTED) return rc;
                if (rc != FASTECC_OK) err = hipErrorOutOfMemory;
            }
            if (err == hipSuccess) err = d->split.small_buf.try_grow(rows * c->S);
        } else if (!d->split.r1 || !d->split.r2) {
            err = d->split.r1.try_alloc(N * c->S);
            if (err == hipSuccess) err = d->split.r2.try_alloc(N * c->S);
            if (err == hipSuccess) err = hipMemsetAsync(d->split.r1, 0, N * c->S * 4, nullptr);
            d->split.dirty = 0;
            if (err != hipSuccess) {
                d->split.r1.reset();
                d->split.r2.reset();
            }
        }
        if (err != hipSuccess) {
            (void)hipGetLastError();
            s.split_groups = 0;
            s.split_shift = 0;
        }
        return FASTECC_OK;
    }

    // ---- this pattern on the device ----
    // 2^log_rows rows of 2^logE words (2^log_rows divides NC): DIF with the forward roots (natural -> bit-reversed rows) or DIT with the inverse
    // roots (bit-reversed -> natural); `top` has 2^(log_rows + logE) / CHUNK rows of CHUNK words
    int narrow_transform(fastecc_ctx* top, int log_rows, int logE, const uint32_t* in, uint32_t* out, bool dit)
    {
        const int logN1 = log_rows + logE - CHUNK_LOG;
        const uint32_t step_n = (uint32_t)(NC >> log_rows), step_n2 = (uint32_t)(NC >> (CHUNK_LOG - logE));
        if (!dit) {
            const int rc = transform_bitrev(top, in, out, false, false, CHUNK, nullptr);
            if (rc != FASTECC_OK) return rc;
            hipLaunchKernelGGL(chunk_transform_kernel<false>, dim3(1u << logN1), dim3(256), 0, nullptr, out, d->tree.wpow, logE, logN1, step_n, step_n2, (uint32_t)(NC - 1));
            return hipGetLastError() == hipSuccess ? FASTECC_OK : FASTECC_E_DEVICE;
        }
        if (in != out) return FASTECC_E_INVAL;
        hipLaunchKernelGGL(chunk_transform_kernel<true>, dim3(1u << logN1), dim3(256), 0, nullptr, out, d->tree.wpow, logE, logN1, step_n, step_n2, (uint32_t)(NC - 1));
        if (hipGetLastError() != hipSuccess) return FASTECC_E_DEVICE;
        return transform_bitrev(top, out, out, true, true, CHUNK, nullptr);
    }

    // The locator's product tree: the erased positions' roots, the leaves (T / leaf polynomials of degree `leaf` side by side, [coefficient]
    // [polynomial]; the upper half of the 2 leaf rows the first product needs is zero), then level by level up.  *coeffs: the buffer that ends
    // with the T lower coefficients of L = x^pad * l (monic of degree T), pad = T - |E|.
    int locator_tree(uint32_t** coeffs)
    {
        hipStream_t st = nullptr;
        if (!s.device_scan) HIP_TRY(hipMemcpyAsync(d->tables.dev_state, s.state.data(), NC, hipMemcpyHostToDevice, st));
        if (!s.srcmap.empty()) HIP_TRY(hipMemcpyAsync(d->tables.srcmap, s.srcmap.data(), NC * 4, hipMemcpyHostToDevice, st));
        else hipLaunchKernelGGL(standard_srcmap_kernel, grid_of(NC), dim3(256), 0, st, d->tables.dev_state, (uint32_t)NC, d->tables.srcmap);
        // the list of erased positions (any order: the locator is their product); its counter sits behind the list
        HIP_TRY(hipMemsetAsync(d->tree.dev_erased + T, 0, 4, st));
        hipLaunchKernelGGL(erased_list_kernel, grid_of((NC + 15) / 16), dim3(256), 0, st, d->tables.dev_state, (uint32_t)NC, d->tree.dev_erased, d->tree.dev_erased + T);
        hipLaunchKernelGGL(roots_kernel, grid_of(T), dim3(256), 0, st, d->tree.roots, d->tree.dev_erased, d->tree.wpow, (uint32_t)s.erased_count, (uint32_t)T);
        HIP_TRY(hipMemsetAsync(d->tree.x, 0, 2 * T * 4, st));
        const uint32_t leaves = (uint32_t)(T >> leaf_log);
        if (leaf_log == TREE_LOW) hipLaunchKernelGGL(tree_low_levels_kernel<TREE_LOW>, dim3(leaves), dim3(1 << TREE_LOW), 0, st, d->tree.roots, d->tree.x, leaves);
        else hipLaunchKernelGGL(leaf_products_kernel, grid_of(leaves), dim3(256), 0, st, d->tree.roots, d->tree.x, (uint32_t)(1 << leaf_log), leaves);
        HIP_TRY(hipGetLastError());
        uint32_t* x = d->tree.x;
        uint32_t* spare = d->tree.y;  // x / spare swap roles level by level; tree_f always holds the transforms
        for (int lv = leaf_log; lv < lgT; lv++) {
            const uint64_t deg = 1ull << lv, m = T >> lv;  // m polynomials of degree deg in x: [2 deg][m], rows deg.. are zero
            fastecc_ctx* t = d->tree.ctx[lv];            // (none: few columns, narrow_transform)
            int rc = t ? transform_bitrev(t, x, d->tree.f, false, false, (uint32_t)m, st)  // all of them at once
                       : narrow_transform(d->tree.top, lv + 1, lgT - lv, x, d->tree.f, false);
            if (rc != FASTECC_OK) return rc;
            const uint32_t scale = gf::h_to_mont(gf::h_inv((uint32_t)(2 * deg)));
            hipLaunchKernelGGL(pointwise_pairs_kernel, grid_of(2 * deg * (m / 2)), dim3(256), 0, st, d->tree.f, d->tree.p, (uint32_t)m, 2 * deg * (m / 2), scale);
            HIP_TRY(hipGetLastError());
            rc = t ? transform_bitrev(t, d->tree.p, d->tree.p, true, true, (uint32_t)(m / 2), st)      // the products, back in natural order
                   : narrow_transform(d->tree.top, lv + 1, lgT - lv, d->tree.p, d->tree.p, true);  // (the unused columns ride along)
            if (rc != FASTECC_OK) return rc;
            const bool top = lv + 1 == lgT;
            const uint64_t rows = top ? 2 * deg : 4 * deg;
            hipLaunchKernelGGL(combine_kernel, grid_of(rows * (m / 2)), dim3(256), 0, st, d->tree.p, x, spare, (uint32_t)deg, (uint32_t)m, rows * (m / 2), top);
            HIP_TRY(hipGetLastError());
            std::swap(x, spare);
        }
        *coeffs = x;
        return FASTECC_OK;
    }

    // From the locator's coefficients to the decoder's tables: its values and its derivative's by one transform of a two-column stripe, fin and
    // gout (gout_par) by finish_tables_kernel, fin in the first pass's order, and the split transform's rows
    int locator_tables(const uint32_t* coeffs)
    {
        hipStream_t st = nullptr;
        hipLaunchKernelGGL(locator_columns_kernel, grid_of(NC), dim3(256), 0, st, coeffs, d->tables.pattern_buf, (uint32_t)T, (uint32_t)NC);
        HIP_TRY(hipGetLastError());
        // (power of two: the values stay in bit-reversed order, finish_tables_kernel reads them there — the reordering pass of fastecc_ntt was 87 us)
        const int rc = mixed               ? mixed_dif(d->tables.pattern_ntt, d->tables.pattern_buf, d->tables.pattern_buf, st)
                       : d->tables.pattern_narrow ? narrow_transform(d->tables.pattern_ntt, lgc, 1, d->tables.pattern_buf, d->tables.pattern_buf, false)
                                           : transform_bitrev(d->tables.pattern_ntt, d->tables.pattern_buf, d->tables.pattern_buf, false, false, 2, st);
        if (rc != FASTECC_OK) return rc;
        hipLaunchKernelGGL(finish_tables_kernel, grid_of(NC), dim3(256), 0, st, d->tables.pattern_buf, (const uint32_t*)d->tables.dev_state.get(), d->tree.wpow, d->tables.fin, d->tables.gout, (uint32_t)NC,
                           (uint32_t)(T - s.erased_count), e, (uint32_t)c->K, (uint32_t)(mixed ? c->q : 1), lgc, parity_factors ? d->tables.gout_par.get() : nullptr,
                           !mixed);
        HIP_TRY(hipGetLastError());
        if (d->tables.fin_first_pass != d->tables.fin) {
            hipLaunchKernelGGL(permute_kernel, grid_of(NC), dim3(256), 0, st, d->tables.fin, d->tables.tile_order, d->tables.fin_first_pass, (uint32_t)NC);
            HIP_TRY(hipGetLastError());
        }
        if (s.split_groups == 0 || !d->split.ctx) return FASTECC_OK;
        // (fastecc_repair in the (2k,k) layout: the lost parity blocks' factors too — gout_par is filled above for such patterns)
        const bool with_parity = parity_factors && d->tables.gout_par != nullptr;
        hipLaunchKernelGGL(split_rows_kernel, grid_of(N), dim3(256), 0, st, d->tables.fin, d->tables.gout, d->split.order, d->split.rows_data, d->split.rows_parity,
                           d->split.rows_out, (uint32_t)N, with_parity ? d->tables.gout_par.get() : nullptr, with_parity ? d->split.rows_out_parity.get() : nullptr);
        d->split.repair_ready = with_parity;
        HIP_TRY(hipGetLastError());
        d->split.shift = s.split_shift;
        if (s.split_shift == 0 && d->split.dirty > s.split_groups) {
            // rows of groups this pattern does not write any more: group g = blocks g + (t << 10)
            const size_t row = c->S * 4;
            HIP_TRY(hipMemset2DAsync(d->split.r1 + (size_t)s.split_groups * c->S, 1024 * row, 0, (d->split.dirty - s.split_groups) * row,
                                     split_decode_group_rows(d->split.ctx), st));
            d->split.dirty = s.split_groups;
        }
        d->split.groups = s.split_shift == 0 ? s.split_groups : 0;
        d->split.ready = true;
        return FASTECC_OK;
    }
};

int decode_prepare_impl(fastecc_ctx* c, const uint8_t* data_present, const uint8_t* parity_present)
{
    if (!c || !data_present || !parity_present) return FASTECC_E_INVAL;
    if (c->sharded) return sharded_decode_prepare(c, data_present, parity_present);
    if (c->field == FASTECC_FIELD_GF_P61_SQUARED) return prepare_p61(c, data_present, parity_present);
    if (c->field != FASTECC_FIELD_GF_FFF00001) return FASTECC_E_UNSUPPORTED;
    if (c->ld != c->S) return FASTECC_E_UNSUPPORTED;
    Prepare p(c, data_present, parity_present);
    bool done = false;
    const int rc = p.direct(&done);
    return rc != FASTECC_OK || done ? rc : p.transform_path();
}

}  // namespace

// (documented in decode_state.hpp: pattern_set.hip builds its sets' tables through here too)
int direct_tables(const CodeGeometry& g, const std::vector<uint32_t>& R, const std::vector<uint32_t>& Pl, const std::vector<uint32_t>& A, PatternTables& t, PhaseTimer& ptd)
{
    const int ed = (int)R.size(), ep = (int)Pl.size();
    int rc = FASTECC_OK;
    auto have = [&](DirectPassPtr& p) {  // a pass object where t holds none yet
        if (!p) p.reset(direct_pass_new());
        t.host_nomem = !p;
        return !t.host_nomem;
    };
    t.host_nomem = false;
    t.ed = ed;
    t.ep = ep;
    const uint32_t K = (uint32_t)g.c->K;
    const uint32_t w = gf::h_root((uint32_t)g.NC), wd = gf::h_pow(w, 1ull << g.e);  // data row i sits at wd^i
    std::vector<uint32_t> xr(ed), ya(ed);  // the points of the lost data blocks and of their parity nodes
    for (int r = 0; r < ed; r++) xr[r] = gf::h_pow(w, (uint64_t)R[r] << g.e);
    for (int a = 0; a < ed; a++) ya[a] = gf::h_pow(w, g.parity_position(A[a]));
    // (up to 32 outputs a pass costs the read of the survivors whatever it computes, profiles/r03/direct_bench.jsonl: one table then serves decode and repair)
    t.only_both = ed > 0 && ep > 0 && ed + ep <= 32;
    if (ed > 0 && !t.only_both) {
        if (!have(t.data)) return FASTECC_E_NOMEM;
        rc = direct_build_interp(t.data, wd, g.N, K, R, xr, A, ya, nullptr);
    }
    ptd.mark("few losses: data table");
    t.both_built = false;
    if (rc == FASTECC_OK && ep > 0) {
        std::vector<uint32_t> yt(ep), ct(ep), pos(ep);
        const uint32_t inv_N = gf::h_inv((uint32_t)(g.N % gf::P));
        for (int i = 0; i < ep; i++) {
            yt[i] = gf::h_pow(w, g.parity_position(Pl[i]));
            ct[i] = gf::h_mul((uint32_t)(((uint64_t)gf::h_pow(yt[i], g.N) + gf::P - 1u) % gf::P), inv_N);  // (y_t^N - 1) / N
            pos[i] = 2u * Pl[i] + 1u;
        }
        if (t.only_both) {
            // data lost as well, few outputs: fastecc_repair reads the survivors ONCE — the lost parity blocks are further outputs on the data
            // pass's nodes (the surviving data and as many parity blocks), not a second pass over the repaired data.  (Above 32 outputs the
            // matrix cores bound the pass, not the read: 128 + 128 lost take 2.40 ms in one pass, 2.48 in two, and the set-up of the second
            // 256-output table costs 0.9 ms.)
            if (!have(t.both)) return FASTECC_E_NOMEM;
            rc = direct_build_interp(t.both, wd, g.N, K, R, xr, A, ya, nullptr, &yt, &pos);
            t.both_built = rc == FASTECC_OK;
        } else {
            if (!have(t.parity)) return FASTECC_E_NOMEM;
            rc = direct_build_lagrange(t.parity, wd, K, yt, ct, pos, nullptr);
        }
    }
    ptd.mark("few losses: parity table");
    return rc;
}

}  // namespace fastecc

using namespace fastecc;

extern "C" {

int fastecc_decode_prepare(fastecc_ctx* c, const uint8_t* data_present, const uint8_t* parity_present)
{
    return guarded([&]() -> int { return decode_prepare_impl(c, data_present, parity_present); });
}

}  // extern "C"
