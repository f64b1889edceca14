// decode.hip — erasure decoding, the "fastest" scheme of README.md:102-119 / RS.md:42-79, for every code of this library.
//
// The reference documents this algorithm and does not implement it.  For the reference's (2k,k) code the codeword is f
// on the 2k-th roots of unity: position u <-> point w^u (w = w_2k), even positions are the data blocks (u = 2i), odd
// ones the parity blocks (u = 2j+1, RS.cpp:51-54).  With E the erased positions (|E| <= k) and
// l(x) = prod_{e in E} (x - w^e):
//
//   p = f * l has degree < 2k and KNOWN values everywhere: c[u] * l(w^u) at surviving positions, 0 at erased ones;
//   p'(w^e) = f(w^e) * l'(w^e) at an erased position, so  f(w^e) = [x p'(x)](w^e) / (w^e * l'(w^e)).
//
// x p'(x) = sum m p_m x^m needs no coefficient shift, which makes the data-parallel part the SAME pipeline as the
// encoder one size up: inverse transform of size 2k, block holding coefficient m times m / 2k, forward transform —
// i.e. create_transform_ctx(2k, factor[m] = m / 2k) with fold = 1, because only the even (data) positions are wanted.
// Around it: a gather (codeword blocks times l(w^u), zeros at erasures; fused into the transform's first pass for the
// (2k,k) layout) and one pass that multiplies the recovered rows by 1 / (w^e l'(w^e)).
//
// Even / odd split (codes with n <= 2k on power-of-two orders, k >= 2^18; option "decode_split"): recovering e data blocks takes e parity
// blocks, so the other surviving parity blocks may count as erased too (ST_UNUSED: roots of l like the lost ones).  With q~ = DIF_k(data * l)
// and r~ = DIF_k(parity * l), unnormalised inverse transforms of k points over the even and the odd positions, the 2k coefficients are
// P[m] = (q~[m] + w^-m r~[m]) / 2k and P[m+k] = (q~[m] - w^-m r~[m]) / 2k, and because w^(2j(m+k)) = w^(2jm) the values of x p'(x) at the data
// positions are the k-point forward transform of  g[m] = m P[m] + (m+k) P[m+k] = (2m+k)/2k q~[m] - 1/2 w^-m r~[m].  So the 2k-point
// pipeline becomes: the encoder's own three passes over the data half (blocks times l(w^2i) on the way in, g's second term added between
// the halves of MID, only the rebuilt blocks stored on the way out) plus r~ — the first pass over the few parity block groups in use, and
// the low levels over a stripe that is zero elsewhere (run_split_decode in encode.hip; tile modes in tile_kernels.hip).
//
// The other codes are the same thing on the (k << e)-th roots of unity (fastecc_decode_prepare): positions that hold no
// block of the code count as erased, zero-extended data blocks as known zeros, the transform has fold = e.
//
// Everything that depends only on the erasure PATTERN is done once in fastecc_decode_prepare, on the device: the locator by
// a product tree whose every level is ONE batch of cyclic products through the library's own transforms (all polynomials
// of a level side by side as the word columns of a stripe), its values and its derivative's values by one transform of a
// two-column stripe, the inverses by Fermat powers.  The host only classifies the positions (one pass over the flags).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <vector>

#include "drivers.hpp"
#include "ntt_device.hpp"

namespace fastecc {

// The direct path's tables of one erasure pattern (Prepare::direct_tables): which passes it takes and their weights
struct PatternTables {
    DirectPassPtr data;    // the lost data blocks (only data lost, or more than 32 blocks lost in all)
    DirectPassPtr parity;  // the lost parity blocks from the complete data (only parity lost, or more than 32 in all)
    DirectPassPtr both;    // data AND parity lost, at most 32 in all: the single pass
    bool both_built = false;       // `both` holds this pattern
    bool only_both = false;        // ... and is its only pass
    int ed = 0, ep = 0;    // lost data / parity blocks
    bool host_nomem = false;       // direct_tables' FASTECC_E_NOMEM is the host's (no DirectPass object), not the device's (no room for a table)
};

struct DecodeState {
    CtxPtr transform;                       // size-2k transform context, fold 1
    CtxPtr pattern_ntt;                     // same length, 2 words per block: l and l' are evaluated on the device
    DeviceBuf<uint32_t> pattern_buf;        // its stripe
    DeviceBuf<uint32_t> fin;                // 2k factors by codeword position: l(w^u) (Montgomery) or 0 if erased
    uint32_t* fin_first_pass = nullptr;     // the same in the order the transform's first pass reads them: a view of fin, or of fin_tiled
    DeviceBuf<uint32_t> fin_tiled;          // ... where that order is not the order of the positions (permuted from fin for every pattern)
    DeviceBuf<uint32_t> srcmap;             // per codeword position: the block that sits there (row, bit 31 = parity stripe)
    DeviceBuf<uint32_t> gout;               // k factors by data block: 1 / (w^2i l'(w^2i)) (Montgomery) if erased, else 0
    // fastecc_repair of the (2k,k) layout in ONE transform: the same x p'(x) evaluated at ALL 2k positions (fold 0) gives the lost parity
    // blocks as well, f(w^u) = (x p')(w^u) / (w^u l'(w^u)) at odd u — instead of decoding the data and encoding it once more
    CtxPtr transform_full;
    DeviceBuf<uint32_t> gout_par;           // k factors by parity block: 1 / (w^(2q+1) l'(w^(2q+1))) (Montgomery) if erased, else 0
    DeviceBuf<uint32_t> recovered_full;     // 2k blocks: x p'(x) at every position (lazy: 4 GiB at the headline size)
    bool full_ok = false;                   // transform_full's first pass reads the factors in the same order as transform's
    DeviceBuf<uint32_t> recovered;          // k blocks: x p'(x) at the data positions
    // (2k,k) layout, the transform as two half-size ones ("even / odd split" below)
    CtxPtr split;                           // k blocks, per-block factor (2m + k) / 2k
    DeviceBuf<uint32_t> split_order;        // k words: the block each slot of its first pass holds (gather_tile_order)
    DeviceBuf<uint32_t> split_rows_data;    // k words, that order: l(w^2i) of the surviving data blocks (0: lost)
    DeviceBuf<uint32_t> split_rows_parity;  // k words, that order: l(w^(2i+1)) of the parity blocks in use (0: lost or unused)
    DeviceBuf<uint32_t> split_rows_out;     // k words, that order: gout of the block (0: not lost)
    DeviceBuf<uint32_t> split_pos_parity;   // k words by position: -w^(-m) / 2 at position bitrev(m)
    DeviceBuf<uint32_t> split_impulse;      // [IMPULSE_MAX][16][64]: what six DIF levels make of a lone block of a 1024-block tile (run_split_decode)
    DeviceBuf<uint32_t> split_r1;           // k blocks: the parity half after its first pass (zero outside the groups in use)
    DeviceBuf<uint32_t> split_r2;           // k blocks: ... after all DIF levels
    DeviceBuf<uint32_t> split_q2;           // fastecc_repair: k blocks, the data chain's MID output while the top-level result serves the parity chain (lazy)
    DeviceBuf<uint32_t> split_pos_data_odd; // k words by position: -w^m / 2 at position bitrev(m) (the parity chain's factor of the data half)
    DeviceBuf<uint32_t> split_rows_out_parity;  // k words, first-pass order: gout_par of the block (0: not lost)
    bool split_repair_ready = false;        // this pattern's lost parity blocks can come from the split transform too
    DeviceBuf<uint32_t> split_r0;           // codes with fewer parity blocks (fold > 0): parity block j copied to its place j << fold of a k-block stripe (lazy)
    uint32_t split_groups = 0;              // block groups of the parity stripe this pattern reads
    // "small" form of the parity half: the parity blocks in use are those at multiples of 2^split_shift of the parity half (1 <= shift <= 5), so r~
    // is the transform of (k >> shift) rows, each result block standing for 2^shift positions: no k-block stripes r1 / r2, no impulse pass
    uint32_t split_shift = 0;
    CtxPtr split_small[6];                  // stand-alone transform contexts of k >> shift blocks (lazy, by shift)
    DeviceBuf<uint32_t> split_small_buf;    // (k >> shift) blocks: those rows times l, then transformed in place
    uint32_t split_dirty = 0;               // groups of split_r1 that may hold non-zero rows
    bool split_ready = false;               // this pattern decodes through the split transform
    bool split_unavailable = false;         // it could not be built on this context (plan shape, memory): the 2k-point transform serves
    DeviceBuf<uint32_t> parity_dev;         // staging for FASTECC_MEM_HOST calls (lazy)
    // FASTECC_MEM_HOST: only the rebuilt blocks travel back — their row numbers (host, and a device copy), valid for pattern `host_lists_of`
    std::vector<uint32_t> host_lost_data, host_lost_parity;
    std::vector<uint32_t> host_parity_used; // few losses: the parity blocks the direct path reads (all it needs staged of a host parity stripe)
    uint64_t pattern_serial = 0, host_lists_of = ~0ull;
    DeviceBuf<uint32_t> lost_rows_dev;      // the two lists back to back
    DeviceBuf<uint32_t> pack_dev;           // the rebuilt blocks, packed
    PinnedBuf<uint32_t> pack_host;          // pinned landing buffer of that copy (kept between calls; the blocks go to their places from here)
    // fastecc_decode_prepare's device state (lazy): the product tree of the locator
    uint64_t tree_T = 0;                    // padded number of roots: the smallest power of two >= the most losses a code tolerates
    std::vector<CtxPtr> tree_ctx;           // level k (polynomials of degree d = 2^k): transforms of length 2d, T/d columns
    CtxPtr tree_top;                        // few-column levels (chunk_transform_kernel): the upper row bits, 2T / CHUNK rows of CHUNK words
    bool pattern_narrow = false;            // pattern_ntt is such a context too (2 NC / CHUNK rows)
    DeviceBuf<uint32_t> tree_x;             // 2T words: the level's polynomials, [coefficient][polynomial]
    DeviceBuf<uint32_t> tree_f;             // 2T words: their transforms
    DeviceBuf<uint32_t> tree_y;             // 2T words: the next level's polynomials (swaps roles with tree_x)
    DeviceBuf<uint32_t> tree_p;             // 2T words: pairwise products
    DeviceBuf<uint32_t> wpow;               // NC words: w^u (plain)
    DeviceBuf<uint32_t> roots;              // T words: the erased points, zero-padded
    DeviceBuf<uint8_t> dev_state;           // NC bytes: LOST / HELD / ZERO per position
    DeviceBuf<uint32_t> dev_erased;         // T words: erased positions
    DeviceBuf<uint8_t> dev_present;         // (2k,k) layout: the caller's two presence arrays, k bytes each (the pattern is scanned on the device)
    DeviceBuf<uint32_t> dev_counts;         // ... and what presence_counts_kernel counts in them (8 words)
    int tree_low = 0;                       // levels below this one are done by tree_low_levels_kernel (0: the per-thread leaves of degree 2^LEAF_LOG)
    DeviceBuf<uint32_t> tile_order;         // NC words: first-pass order of the factors (only for the (2k,k) layout)
    bool tile_order_valid = false;
    // fastecc_repair: which parity blocks are lost (one word each), and the stripe the re-encode writes to
    DeviceBuf<uint32_t> parity_lost;
    DeviceBuf<uint32_t> parity_again;
    uint64_t erased_parity = 0;
    uint64_t erased_data = 0, erased_total = 0;
    // few losses (any layout: the reference's, zero extension, sub-/extra cosets, mixed radix): every lost data block is a fixed linear
    // combination of the surviving data blocks and as many surviving parity blocks (interpolation on N nodes); for repair the lost parity
    // blocks follow from the complete data (direct.hip)
    PatternTables direct;                   // the passes of the current pattern: built over from pattern to pattern
    bool sub_both = false;                  // direct.both (data AND parity lost: fastecc_repair's single pass) is built for this pattern
    bool sub_only_both = false;             // ... and is the only pass (few outputs: the pass is bound by the read of the survivors, fastecc_decode runs it too and drops the parity outputs)
    int sub_lost_data = 0, sub_lost_parity = 0;
    bool sub = false;
    int direct_kernel = 0;                  // 0 choose, 1 VALU, 2 MFMA (option "direct_kernel")
    DeviceBuf<DirectSetPass> read_desc;     // fastecc_read_batch: the descriptor of the pass that rebuilds the lost data, valid for pattern `read_desc_of` (lazy)
    uint64_t read_desc_of = ~0ull;
    uint64_t positions = 0;                 // code length on the roots of unity: k << log2(n / k) rounded up to powers of two
    bool mixed = false;                     // mixed-radix code: `recovered` is the whole work stripe (all positions), transformed in place
    bool standard = false;                  // the reference's (2k,k) layout: position u = data u/2 or parity u/2, every block in memory
    bool ready = false;
};

void destroy_decode_state(DecodeState* d) { delete d; }

// A pattern set (fastecc_decode_prepare_set): P patterns of at most 16 lost blocks, each exactly one direct pass, for pools in which the pattern
// differs from stripe to stripe (fastecc_decode_batch_set / _repair_batch_set).  Independent of the DecodeState's single pattern.
struct PatternSet {
    enum : uint8_t { NOTHING = 0, DATA = 1, PARITY = 2, BOTH = 3 };  // which pass a pattern takes (NOTHING: no block lost)
    std::vector<PatternTables> tables;  // per pattern
    std::vector<uint8_t> kind;          // ... its pass
    std::vector<uint8_t> cls;           // ... log2 of that pass's pad (1, 2, 4, 8, 16): the class a launch is templated on
    std::vector<uint32_t> rows;         // ... the rows it reads
    std::vector<std::vector<uint32_t>> lost_data;  // ... its lost data blocks, in the order of the pass's outputs (fastecc_read_batch_set)
    std::vector<std::vector<uint32_t>> lost_parity;  // ... its lost parity blocks, increasing (fastecc_update_batch_set)
    DeviceBuf<DirectSetPass> d_passes;  // device: the descriptor table, entry q = pattern q's pass
    DeviceBuf<uint32_t> d_lost_parity;  // device: P + 1 rows of SET_LOST_ROW words, row q = lost_parity[q] padded with SET_LOST_END; row P loses nothing
    // one call's entries, sorted by class (list.dev is an internal buffer: ordered between streams by the context's buf_event).  Outlives the set.
    StagedList<DirectSetEntry> list;
    DirectPass* pass(uint64_t q) const { return kind[q] == DATA ? tables[q].data.get() : kind[q] == PARITY ? tables[q].parity.get() : tables[q].both.get(); }
};

void destroy_pattern_set(PatternSet* s) { delete s; }

namespace {

// ------------------------------------------------------------------------------------------------
// fastecc_decode_prepare on the device.  All values are plain representatives unless a table is consumed by
// gf::mul_mont, in which case it is stored in Montgomery form (x * 2^32 mod p = gf::mul(x, MONT_ONE)).
// ------------------------------------------------------------------------------------------------
// ST_UNUSED: a surviving parity block the split transform does not read — a root of the locator like a lost one, but nothing to rebuild
enum : uint32_t { ST_LOST = 0, ST_HELD = 1, ST_ZERO = 2, ST_UNUSED = 3 };
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

// ------------------------------------------------------------------------------------------------
// kernels: one wave per (block row, 64*V-word column chunk); the row's factor is a scalar
// ------------------------------------------------------------------------------------------------
// work[u] = block at codeword position u, times fin[u].  srcmap[u] names the block: row index, bit 31 set = parity
// stripe.  Positions without a surviving block have fin == 0: they are written as zeros and nothing is read for them.
template <int V>
__global__ __launch_bounds__(256) void decode_gather_kernel(const uint32_t* __restrict__ data, const uint32_t* __restrict__ parity,
                                                            uint32_t* __restrict__ work, const uint32_t* __restrict__ fin,
                                                            const uint32_t* __restrict__ srcmap, uint32_t S, uint32_t ld, uint32_t ld_work,
                                                            uint32_t col_chunks, uint64_t items)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t item = (uint64_t)blockIdx.x * 4u + wave;
    if (item >= items) return;
    const uint32_t cc = (uint32_t)(item % col_chunks);
    const uint32_t u = (uint32_t)(item / col_chunks);
    const uint32_t col = (cc * 64u + lane) * V;
    if (col >= S) return;
    const uint32_t f = as_constant(fin)[u];
    uint32_t x[V];
    if (f != 0) {
        const uint32_t m = as_constant(srcmap)[u];
        const uint32_t* src = ((m >> 31) ? parity : data) + (size_t)(m & 0x7FFFFFFFu) * ld + col;
        load_vec<V>(x, src);
#pragma unroll
        for (int v = 0; v < V; ++v) x[v] = gf::mul_mont(x[v], f);
    } else {
#pragma unroll
        for (int v = 0; v < V; ++v) x[v] = 0;
    }
    store_vec<V>(work + (size_t)u * ld_work + col, x);
}

// data[i] = recovered[i] * gout[i] for the erased data blocks (gout != 0); surviving blocks are not touched
template <int V>
__global__ __launch_bounds__(256) void decode_scatter_kernel(const uint32_t* __restrict__ recovered, uint32_t* __restrict__ data,
                                                             const uint32_t* __restrict__ gout, uint32_t S, uint32_t ld_rec, uint32_t ld,
                                                             uint32_t col_chunks, uint64_t items)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t item = (uint64_t)blockIdx.x * 4u + wave;
    if (item >= items) return;
    const uint32_t cc = (uint32_t)(item % col_chunks);
    const uint32_t i = (uint32_t)(item / col_chunks);
    const uint32_t f = as_constant(gout)[i];
    if (f == 0) return;  // wave-uniform
    const uint32_t col = (cc * 64u + lane) * V;
    if (col >= S) return;
    uint32_t x[V];
    load_vec<V>(x, recovered + (size_t)i * ld_rec + col);
#pragma unroll
    for (int v = 0; v < V; ++v) x[v] = gf::mul_mont(x[v], f);
    store_vec<V>(data + (size_t)i * ld + col, x);
}

// split transform of a code with fewer parity blocks: stage[q << fold] = parity[q] for the parity blocks in use (fin != 0 at their position); the
// rest of the stage is never read with a non-zero factor
template <int V>
__global__ __launch_bounds__(256) void split_stage_kernel(const uint32_t* __restrict__ parity, uint32_t* __restrict__ stage, const uint32_t* __restrict__ fin,
                                                          uint32_t S, int fold, uint32_t col_chunks, uint64_t items)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t item = (uint64_t)blockIdx.x * 4u + wave;
    if (item >= items) return;
    const uint32_t cc = (uint32_t)(item % col_chunks);
    const uint32_t q = (uint32_t)(item / col_chunks);
    if (as_constant(fin)[2u * (q << fold) + 1u] == 0) return;  // wave-uniform
    const uint32_t col = (cc * 64u + lane) * V;
    if (col >= S) return;
    uint32_t x[V];
    load_vec<V>(x, parity + (size_t)q * S + col);
    store_vec<V>(stage + (size_t)(q << fold) * S + col, x);
}

// split transform, small form: row m of the work stripe = parity block at position m << shift of the parity half (block (m << shift) >> fold of
// the parity stripe) times l at its codeword position — zero where that block is lost, not in use, or does not exist
template <int V>
__global__ __launch_bounds__(256) void split_small_gather_kernel(const uint32_t* __restrict__ parity, uint32_t* __restrict__ work, const uint32_t* __restrict__ fin,
                                                                 uint32_t S, int shift, int fold, uint32_t parity_blocks, uint32_t col_chunks, uint64_t items)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t item = (uint64_t)blockIdx.x * 4u + wave;
    if (item >= items) return;
    const uint32_t cc = (uint32_t)(item % col_chunks);
    const uint32_t m = (uint32_t)(item / col_chunks);
    const uint32_t h = m << shift, q = h >> fold;
    const uint32_t f = ((h & ((1u << fold) - 1u)) == 0 && q < parity_blocks) ? as_constant(fin)[2u * h + 1u] : 0u;  // wave-uniform
    const uint32_t col = (cc * 64u + lane) * V;
    if (col >= S) return;
    uint32_t x[V];
#pragma unroll
    for (int v = 0; v < V; ++v) x[v] = 0;
    if (f != 0) {
        load_vec<V>(x, parity + (size_t)q * S + col);
#pragma unroll
        for (int v = 0; v < V; ++v) x[v] = gf::mul_mont(x[v], f);
    }
    store_vec<V>(work + (size_t)m * S + col, x);
}

// packed[r] = stripe[rows[r]]: the rebuilt blocks side by side, for one copy to the host
template <int V>
__global__ __launch_bounds__(256) void pack_rows_kernel(const uint32_t* __restrict__ stripe, const uint32_t* __restrict__ rows, uint32_t* __restrict__ packed,
                                                        uint32_t S, uint32_t col_chunks, uint64_t items)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t item = (uint64_t)blockIdx.x * 4u + wave;
    if (item >= items) return;
    const uint32_t cc = (uint32_t)(item % col_chunks);
    const uint32_t r = (uint32_t)(item / col_chunks);
    const uint32_t col = (cc * 64u + lane) * V;
    if (col >= S) return;
    uint32_t x[V];
    load_vec<V>(x, stripe + (size_t)as_constant(rows)[r] * S + col);
    store_vec<V>(packed + (size_t)r * S + col, x);
}

// parity[q] = again[q] for the parity blocks that were lost (lost[q] != 0); the others are not touched
template <int V>
__global__ __launch_bounds__(256) void restore_parity_kernel(const uint32_t* __restrict__ again, uint32_t* __restrict__ parity,
                                                             const uint32_t* __restrict__ lost, uint32_t S, uint32_t col_chunks, uint64_t items)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t item = (uint64_t)blockIdx.x * 4u + wave;
    if (item >= items) return;
    const uint32_t cc = (uint32_t)(item % col_chunks);
    const uint32_t q = (uint32_t)(item / col_chunks);
    if (as_constant(lost)[q] == 0) return;  // wave-uniform
    const uint32_t col = (cc * 64u + lane) * V;
    if (col >= S) return;
    uint32_t x[V];
    load_vec<V>(x, again + (size_t)q * S + col);
    store_vec<V>(parity + (size_t)q * S + col, x);
}

dim3 grid_of(uint64_t items) { return dim3((unsigned)((items + 255) / 256)); }  // one thread per item, 256 per workgroup

// The row kernels above over `rows` rows of S words: one wave per (row, column chunk of 64 V words), V = 4 when S is a multiple of 4 and every
// pointer in `ptrs` is 16-byte aligned, else 1.  `args` are the kernel's arguments but the last two (chunks per row, waves in all).
template <class... K, class... A>
void launch_rows(void (*k4)(K...), void (*k1)(K...), uint64_t rows, uint32_t S, std::initializer_list<const void*> ptrs, hipStream_t st, const A&... args)
{
    uintptr_t bits = 0;
    for (const void* p : ptrs) bits |= (uintptr_t)p;
    const bool v4 = (S % 4) == 0 && (bits & 15u) == 0;
    const uint32_t col_chunks = (S + (v4 ? 256 : 64) - 1) / (v4 ? 256 : 64);
    const uint64_t items = rows * col_chunks;
    hipLaunchKernelGGL(v4 ? k4 : k1, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, st, args..., col_chunks, items);
}

// the context's decoder state, made at its first use (nullptr: no memory)
DecodeState* state_of(fastecc_ctx* c)
{
    if (!c->decoder) c->decoder = new (std::nothrow) DecodeState();
    return c->decoder;
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

// lost(i) for each flag i < count that is zero, until lost returns false.  (Eight flags per step: a word without a zero byte holds no lost
// block — byte by byte the two scans took 0.2-0.4 ms of a 0.3-0.5 ms call at k = 2^19.)
template <class F> void each_lost(const uint8_t* flags, uint64_t count, F&& lost)
{
    uint64_t i = 0;
    for (; i + 8 <= count; i += 8) {
        uint64_t v;
        memcpy(&v, flags + i, 8);
        if (((v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull) == 0) continue;
        for (uint64_t j = i; j < i + 8; j++)
            if (!flags[j] && !lost(j)) return;
    }
    for (; i < count; i++)
        if (!flags[i] && !lost(i)) return;
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
    void new_pattern(uint64_t erased_data, uint64_t erased_total)  // (the previous pattern is dropped)
    {
        d->ready = false;
        d->erased_data = erased_data;
        d->erased_total = erased_total;
        d->positions = NC;
        d->standard = standard;
        d->mixed = mixed;
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

    // The direct path's tables of one pattern: the lost data blocks R (each a fixed linear combination of the surviving data blocks and of the
    // surviving parity blocks A, one per lost data block), the lost parity blocks Pl.  Data AND parity lost, at most 32 in all: one pass, `both`
    // (the lost parity blocks as further outputs on the data pass's nodes); else `data` for the lost data and `parity` (from the complete data)
    // for the lost parity.  Passes are allocated where t holds none yet.  Takes no lock and touches no context state: the single pattern's
    // fastecc_decode_prepare (direct) and every pattern of a set (prepare_set_impl) come through here.
    int direct_tables(const std::vector<uint32_t>& R, const std::vector<uint32_t>& Pl, const std::vector<uint32_t>& A, PatternTables& t, PhaseTimer& ptd)
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
        const uint32_t K = (uint32_t)c->K;
        const uint32_t w = gf::h_root((uint32_t)NC), wd = gf::h_pow(w, 1ull << e);  // data row i sits at wd^i
        std::vector<uint32_t> xr(ed), ya(ed);  // the points of the lost data blocks and of their parity nodes
        for (int r = 0; r < ed; r++) xr[r] = gf::h_pow(w, (uint64_t)R[r] << e);
        for (int a = 0; a < ed; a++) ya[a] = gf::h_pow(w, parity_position(A[a]));
        // (up to 32 outputs a pass costs the read of the survivors whatever it computes, profiles/r03/direct_bench.jsonl: one table then serves decode and repair)
        t.only_both = ed > 0 && ep > 0 && ed + ep <= 32;
        if (ed > 0 && !t.only_both) {
            if (!have(t.data)) return FASTECC_E_NOMEM;
            rc = direct_build_interp(t.data, wd, N, K, R, xr, A, ya, nullptr);
        }
        ptd.mark("few losses: data table");
        t.both_built = false;
        if (rc == FASTECC_OK && ep > 0) {
            std::vector<uint32_t> yt(ep), ct(ep), pos(ep);
            const uint32_t inv_N = gf::h_inv((uint32_t)(N % gf::P));
            for (int i = 0; i < ep; i++) {
                yt[i] = gf::h_pow(w, parity_position(Pl[i]));
                ct[i] = gf::h_mul((uint32_t)(((uint64_t)gf::h_pow(yt[i], N) + gf::P - 1u) % gf::P), inv_N);  // (y_t^N - 1) / N
                pos[i] = 2u * Pl[i] + 1u;
            }
            if (t.only_both) {
                // data lost as well, few outputs: fastecc_repair reads the survivors ONCE — the lost parity blocks are further outputs on the data
                // pass's nodes (the surviving data and as many parity blocks), not a second pass over the repaired data.  (Above 32 outputs the
                // matrix cores bound the pass, not the read: 128 + 128 lost take 2.40 ms in one pass, 2.48 in two, and the set-up of the second
                // 256-output table costs 0.9 ms.)
                if (!have(t.both)) return FASTECC_E_NOMEM;
                rc = direct_build_interp(t.both, wd, N, K, R, xr, A, ya, nullptr, &yt, &pos);
                t.both_built = rc == FASTECC_OK;
            } else {
                if (!have(t.parity)) return FASTECC_E_NOMEM;
                rc = direct_build_lagrange(t.parity, wd, K, yt, ct, pos, nullptr);
            }
        }
        ptd.mark("few losses: parity table");
        return rc;
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
        new_pattern(ed, ed + ep);
        d->sub = false;
        d->erased_parity = ep;
        d->direct_kernel = c->direct_kernel;
        int rc = wait_idle(c);  // a decode still using the previous pattern
        if (rc != FASTECC_OK) return rc;
        ptd.mark("few losses: lock, idle");
        const PatternTables& t = d->direct;
        rc = direct_tables(R, Pl, A, d->direct, ptd);
        d->sub_only_both = t.only_both;
        d->sub_both = t.both_built;
        if (rc == FASTECC_E_NOMEM && !t.host_nomem) return FASTECC_OK;  // no memory for the weight tables: the transform path
        if (rc != FASTECC_OK) return rc;
        d->sub = true;
        d->sub_lost_data = ed;
        d->sub_lost_parity = ep;
        d->host_lost_data = R;  // (FASTECC_MEM_HOST calls: the rows that travel back)
        d->host_lost_parity = Pl;
        d->host_parity_used = A;
        d->host_lists_of = ++d->pattern_serial;
        d->ready = true;
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
            d->ready = true;
            return FASTECC_OK;
        }
        while (T < NC - N && T < (1ull << 20)) T <<= 1;
        while ((1ull << lgT) < T) lgT++;
        if (s.erased_count > T) return FASTECC_E_UNSUPPORTED;
        leaf_log = lgT >= TREE_LOW + 2 ? TREE_LOW : std::min(LEAF_LOG, lgT);
        parity_factors = d->erased_parity != 0 && (d->standard || (s.split_groups != 0 && c->fold == 0));
        if ((rc = build_shape()) != FASTECC_OK) return rc;
        if ((rc = wait_idle(c)) != FASTECC_OK) return rc;  // a decode still using the previous pattern
        pt.mark("tables, tile order");
        uint32_t* coeffs = nullptr;
        if ((rc = locator_tree(&coeffs)) != FASTECC_OK || (rc = locator_tables(coeffs)) != FASTECC_OK) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        pt.mark("this pattern (device)");
        d->ready = true;
        return FASTECC_OK;
    }

    // The reference's (2k,k) layout: the pattern is scanned on the DEVICE (the host loops of scan_host took 1.2-1.4 ms of a 2.6 ms call at k = 2^19:
    // four passes over a million byte-sized coin flips).  Two 512 KB uploads, one counting kernel, 32 bytes back; the per-position state and the
    // lost-parity flags are then written by a kernel.  Patterns the "small form" of the split transform does not take (too few surviving parity
    // blocks at multiples of 2^h) leave s as it is: the host scan.
    int scan_device()
    {
        RC_TRY(d->dev_present.alloc(2 * N));
        RC_TRY(d->dev_counts.alloc(8));
        RC_TRY(d->dev_state.alloc(NC));
        RC_TRY(d->parity_lost.alloc(c->Mu));
        RC_TRY(wait_idle(c));  // a decode or repair still reading the previous pattern's state
        d->ready = false;
        HIP_TRY(hipMemcpyAsync(d->dev_present, data_present, N, hipMemcpyHostToDevice, nullptr));
        HIP_TRY(hipMemcpyAsync(d->dev_present + N, parity_present, N, hipMemcpyHostToDevice, nullptr));
        HIP_TRY(hipMemsetAsync(d->dev_counts, 0, 8 * 4, nullptr));
        hipLaunchKernelGGL(presence_counts_kernel, dim3(128), dim3(256), 0, nullptr, d->dev_present, d->dev_present + N, (uint32_t)N, d->dev_counts);
        HIP_TRY(hipGetLastError());
        uint32_t counts[8] = {};
        HIP_TRY(hipMemcpy(counts, d->dev_counts, sizeof counts, hipMemcpyDeviceToHost));
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
        hipLaunchKernelGGL(standard_state_kernel, grid_of(N), dim3(256), 0, nullptr, d->dev_present, d->dev_present + N, (uint32_t)N,
                           shift ? (1u << shift) - 1u : 0u, d->dev_state, d->parity_lost);
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
        new_pattern(s.erased_data, s.erased_count);
        pt.mark("lock, state");
        d->erased_parity = s.erased_parity;
        if (!s.device_scan) {
            std::vector<uint32_t> plost(c->Mu);
            for (uint64_t q = 0; q < c->Mu; q++) plost[q] = parity_present[q] ? 0u : 1u;
            RC_TRY(d->parity_lost.alloc(c->Mu));
            RC_TRY(wait_idle(c));  // a repair still reading the previous pattern
            HIP_TRY(hipMemcpy(d->parity_lost, plost.data(), c->Mu * 4, hipMemcpyHostToDevice));
        }
        pt.mark("lost-parity flags");
        d->sub = false;
        ++d->pattern_serial;  // (the lists of rebuilt rows for FASTECC_MEM_HOST calls are made when such a call comes: StripeDecode::stage_host)
        return FASTECC_OK;
    }

    // Everything that outlives a pattern, built once per context or shape: contexts, tree buffers, tables, the split transform and its buffers,
    // the one-transform repair's context, the tile order.  May clear s.split_groups (split_buffers).
    int build_shape()
    {
        int rc = build_transforms();
        if (rc != FASTECC_OK) return rc;
        if ((d->tree_T != T || d->tree_low != leaf_log) && (rc = build_tree()) != FASTECC_OK) return rc;
        pt.mark("tree contexts + buffers");
        if ((rc = build_tables()) != FASTECC_OK) return rc;
        d->split_ready = false;
        d->split_repair_ready = false;
        if (s.split_groups != 0 && !d->split_unavailable && !d->split && (rc = build_split()) != FASTECC_OK) return rc;
        if (s.split_groups != 0 && d->split && (rc = split_buffers()) != FASTECC_OK) return rc;
        if (d->standard && d->erased_parity != 0 && !(s.split_groups != 0 && d->split) && !d->transform_full) {
            // repair in one transform (see DecodeState::transform_full): the form for patterns or plans the split transform does not take
            rc = create_ramp_transform_ctx(d->transform_full.fill(), lgc, c->S * 4, 0, gf::h_inv((uint32_t)NC), c->device);
            if (rc != FASTECC_OK && rc != FASTECC_E_NOMEM) return rc;
            d->full_ok = d->transform_full && same_tile_order(d->transform, d->transform_full);
            if (getenv("FASTECC_TRACE_PREPARE"))
                fprintf(stderr, "[fastecc prepare] one-transform repair: context %s, same first-pass order %d (%s | %s)\n", d->transform_full ? "built" : "none",
                        (int)d->full_ok, fastecc_plan_string(d->transform), d->transform_full ? fastecc_plan_string(d->transform_full) : "");
        }
        if (d->standard && !d->tile_order_valid) {
            if (same_tile_order(d->transform, d->transform)) {  // (a tile first pass: the order exists)
                RC_TRY(d->tile_order.alloc(NC));
                if (!gather_tile_order_device(d->transform, d->tile_order, nullptr)) return FASTECC_E_DEVICE;
                RC_TRY(d->fin_tiled.alloc(NC));
                d->fin_first_pass = d->fin_tiled;
            } else {
                d->fin_first_pass = d->fin;
            }
            d->tile_order_valid = true;
        }
        if (!d->standard) d->fin_first_pass = d->fin;
        return FASTECC_OK;
    }

    // the pattern's transform (two columns: l and l') and the decoder's own
    int build_transforms()
    {
        if (!d->pattern_ntt) {
            int rc;
            if (mixed) {
                const std::vector<uint32_t> ones(NC, 1u);
                rc = create_mixed_transform_ctx(d->pattern_ntt.fill(), c->q, lgc, 8, ones.data(), c->device);
            } else {
                // only its stand-alone transform is used; long ones as the upper row bits of a four-step transform (chunk_transform_kernel)
                d->pattern_narrow = narrow && lgc + 1 - CHUNK_LOG >= 1;
                rc = d->pattern_narrow ? create_ntt_ctx(d->pattern_ntt.fill(), lgc + 1 - CHUNK_LOG, 4 * CHUNK, c->device) : create_ntt_ctx(d->pattern_ntt.fill(), lgc, 8, c->device);
            }
            if (rc != FASTECC_OK) return rc;
        }
        pt.mark("pattern_ntt context");
        RC_TRY(d->pattern_buf.alloc(2 * NC));
        if (!d->transform) {
            // x p'(x): coefficient m times m, and the 1/NC of the inverse transform.  fold e: only the data positions (multiples of 2^e) are
            // evaluated (mixed radix: all positions, the even ones are used)
            const uint32_t inv_nc = gf::h_inv((uint32_t)NC);
            int rc;
            if (mixed) {
                std::vector<uint32_t> factor(NC);
                const uint32_t inv_nc_m = gf::h_to_mont(inv_nc);
                for (uint64_t m = 0; m < NC; m++) factor[m] = gf::h_mont_mul((uint32_t)m, inv_nc_m);
                rc = create_mixed_transform_ctx(d->transform.fill(), c->q, lgc, c->S * 4, factor.data(), c->device);
            } else {
                rc = create_ramp_transform_ctx(d->transform.fill(), lgc, c->S * 4, e, inv_nc, c->device);
            }
            if (rc != FASTECC_OK) return rc;
        }
        pt.mark("transform context");
        return FASTECC_OK;
    }

    // the tree's contexts and buffers: level k >= leaf_log multiplies pairs of degree-2^k polynomials — transforms of length 2^(k+1) on T / 2^k columns
    int build_tree()
    {
        d->tree_ctx.clear();
        d->tree_top.reset();
        d->tree_ctx.resize(lgT);
        const bool narrow_tree = narrow && lgT + 1 - CHUNK_LOG >= 1 && lgT > leaf_log;
        for (int lv = leaf_log; lv < lgT; lv++) {
            if (narrow_tree && (T >> lv) <= NARROW_COLUMNS) continue;  // tree_top + chunk_transform_kernel
            const int rc = create_ntt_ctx(d->tree_ctx[lv].fill(), lv + 1, 4 * (T >> lv), c->device);
            if (rc != FASTECC_OK) return rc;
        }
        if (narrow_tree) {
            const int rc = create_ntt_ctx(d->tree_top.fill(), lgT + 1 - CHUNK_LOG, 4 * CHUNK, c->device);
            if (rc != FASTECC_OK) return rc;
        }
        for (DeviceBuf<uint32_t>* b : {&d->tree_x, &d->tree_f, &d->tree_y, &d->tree_p, &d->roots, &d->dev_erased}) b->reset();
        for (DeviceBuf<uint32_t>* b : {&d->tree_x, &d->tree_f, &d->tree_y, &d->tree_p}) RC_TRY(b->alloc(2 * T));
        RC_TRY(d->roots.alloc(T));
        RC_TRY(d->dev_erased.alloc(T + 1));  // + the counter of erased_list_kernel
        d->tree_T = T;
        d->tree_low = leaf_log;
        return FASTECC_OK;
    }

    // the tables by position and block, and the stripe of the recovered blocks
    int build_tables()
    {
        if (!d->wpow) {
            // the table becomes visible to later calls only once the kernel that fills it has been launched without error
            // (an unfilled table behind a non-null pointer would give silently wrong weights on the next prepare)
            DeviceBuf<uint32_t> fresh;
            RC_TRY(fresh.alloc(NC));
            hipLaunchKernelGGL(wpow_kernel, grid_of(NC), dim3(256), 0, nullptr, fresh.get(), gf::h_root((uint32_t)NC), (uint32_t)NC);
            HIP_TRY(hipGetLastError());
            d->wpow = std::move(fresh);
        }
        RC_TRY(d->dev_state.alloc(NC));
        RC_TRY(d->fin.alloc(NC));
        RC_TRY(d->srcmap.alloc(NC));
        RC_TRY(d->gout.alloc(N));
        if (parity_factors) RC_TRY(d->gout_par.alloc(N));
        // mixed radix: the work stripe of all NC positions, transformed in place; else the N recovered data positions
        return d->recovered.alloc((mixed ? NC : N) * c->S);
    }

    // The split transform's context and tables (once).  Anything missing — a plan without the tile shapes, no memory for the two extra stripes —
    // leaves the 2k-point transform in charge for good (split_unavailable); the pattern's unused parity blocks are unused there as well.
    int build_split()
    {
        const int rc = [&]() -> int {
            // per-block factor (2m + k) / 2k = m / k + 1 / 2
            const int rc = create_ramp_transform_ctx(d->split.fill(), c->n, c->S * 4, 0, gf::h_inv((uint32_t)N), c->device, gf::h_inv(2u));
            if (rc != FASTECC_OK) return rc;
            if (!split_decode_supported(d->split) || split_decode_groups(d->split) != 1024u) return FASTECC_E_UNSUPPORTED;
            for (DeviceBuf<uint32_t>* b : {&d->split_order, &d->split_rows_data, &d->split_rows_parity, &d->split_rows_out, &d->split_pos_parity,
                                           &d->split_pos_data_odd, &d->split_rows_out_parity})
                RC_TRY(b->alloc(N));
            if (!gather_tile_order_device(d->split, d->split_order, nullptr)) return FASTECC_E_UNSUPPORTED;
            const std::vector<uint32_t> table = split_impulse_table(gf::h_root((uint32_t)NC), N);
            RC_TRY(d->split_impulse.alloc(table.size()));
            HIP_TRY(hipMemcpy(d->split_impulse, table.data(), table.size() * 4, hipMemcpyHostToDevice));
            const uint32_t neg_half = (uint32_t)(gf::P - gf::h_inv(2u));
            hipLaunchKernelGGL(split_pos_kernel, grid_of(N), dim3(256), 0, nullptr, d->wpow, d->split_pos_parity, (uint32_t)N, c->n, neg_half, false);
            hipLaunchKernelGGL(split_pos_kernel, grid_of(N), dim3(256), 0, nullptr, d->wpow, d->split_pos_data_odd, (uint32_t)N, c->n, neg_half, true);
            HIP_TRY(hipGetLastError());
            return FASTECC_OK;
        }();
        if (rc == FASTECC_OK) {
            d->split_dirty = 0;
            return FASTECC_OK;
        }
        // nothing half-built stays behind: a later call either builds all of it or none
        (void)hipGetLastError();
        d->split.reset();
        for (DeviceBuf<uint32_t>* b : {&d->split_order, &d->split_rows_data, &d->split_rows_parity, &d->split_rows_out, &d->split_pos_parity, &d->split_impulse,
                                       &d->split_r1, &d->split_r2, &d->split_pos_data_odd, &d->split_rows_out_parity})
            b->reset();
        if (rc != FASTECC_E_NOMEM && rc != FASTECC_E_UNSUPPORTED) return rc;
        d->split_unavailable = true;
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
            if (!d->split_small[s.split_shift]) {
                const int rc = create_ntt_ctx(d->split_small[s.split_shift].fill(), c->n - (int)s.split_shift, c->S * 4, c->device);
                if (rc != FASTECC_OK && rc != FASTECC_E_NOMEM && rc != FASTECC_E_UNSUPPORTED) return rc;
                if (rc != FASTECC_OK) err = hipErrorOutOfMemory;
            }
            if (err == hipSuccess) err = d->split_small_buf.try_grow(rows * c->S);
        } else if (!d->split_r1 || !d->split_r2) {
            err = d->split_r1.try_alloc(N * c->S);
            if (err == hipSuccess) err = d->split_r2.try_alloc(N * c->S);
            if (err == hipSuccess) err = hipMemsetAsync(d->split_r1, 0, N * c->S * 4, nullptr);
            d->split_dirty = 0;
            if (err != hipSuccess) {
                d->split_r1.reset();
                d->split_r2.reset();
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
            hipLaunchKernelGGL(chunk_transform_kernel<false>, dim3(1u << logN1), dim3(256), 0, nullptr, out, d->wpow, logE, logN1, step_n, step_n2, (uint32_t)(NC - 1));
            return hipGetLastError() == hipSuccess ? FASTECC_OK : FASTECC_E_DEVICE;
        }
        if (in != out) return FASTECC_E_INVAL;
        hipLaunchKernelGGL(chunk_transform_kernel<true>, dim3(1u << logN1), dim3(256), 0, nullptr, out, d->wpow, logE, logN1, step_n, step_n2, (uint32_t)(NC - 1));
        if (hipGetLastError() != hipSuccess) return FASTECC_E_DEVICE;
        return transform_bitrev(top, out, out, true, true, CHUNK, nullptr);
    }

    // The locator's product tree: the erased positions' roots, the leaves (T / leaf polynomials of degree `leaf` side by side, [coefficient]
    // [polynomial]; the upper half of the 2 leaf rows the first product needs is zero), then level by level up.  *coeffs: the buffer that ends
    // with the T lower coefficients of L = x^pad * l (monic of degree T), pad = T - |E|.
    int locator_tree(uint32_t** coeffs)
    {
        hipStream_t st = nullptr;
        if (!s.device_scan) HIP_TRY(hipMemcpyAsync(d->dev_state, s.state.data(), NC, hipMemcpyHostToDevice, st));
        if (!s.srcmap.empty()) HIP_TRY(hipMemcpyAsync(d->srcmap, s.srcmap.data(), NC * 4, hipMemcpyHostToDevice, st));
        else hipLaunchKernelGGL(standard_srcmap_kernel, grid_of(NC), dim3(256), 0, st, d->dev_state, (uint32_t)NC, d->srcmap);
        // the list of erased positions (any order: the locator is their product); its counter sits behind the list
        HIP_TRY(hipMemsetAsync(d->dev_erased + T, 0, 4, st));
        hipLaunchKernelGGL(erased_list_kernel, grid_of((NC + 15) / 16), dim3(256), 0, st, d->dev_state, (uint32_t)NC, d->dev_erased, d->dev_erased + T);
        hipLaunchKernelGGL(roots_kernel, grid_of(T), dim3(256), 0, st, d->roots, d->dev_erased, d->wpow, (uint32_t)s.erased_count, (uint32_t)T);
        HIP_TRY(hipMemsetAsync(d->tree_x, 0, 2 * T * 4, st));
        const uint32_t leaves = (uint32_t)(T >> leaf_log);
        if (leaf_log == TREE_LOW) hipLaunchKernelGGL(tree_low_levels_kernel<TREE_LOW>, dim3(leaves), dim3(1 << TREE_LOW), 0, st, d->roots, d->tree_x, leaves);
        else hipLaunchKernelGGL(leaf_products_kernel, grid_of(leaves), dim3(256), 0, st, d->roots, d->tree_x, (uint32_t)(1 << leaf_log), leaves);
        HIP_TRY(hipGetLastError());
        uint32_t* x = d->tree_x;
        uint32_t* spare = d->tree_y;  // x / spare swap roles level by level; tree_f always holds the transforms
        for (int lv = leaf_log; lv < lgT; lv++) {
            const uint64_t deg = 1ull << lv, m = T >> lv;  // m polynomials of degree deg in x: [2 deg][m], rows deg.. are zero
            fastecc_ctx* t = d->tree_ctx[lv];            // (none: few columns, narrow_transform)
            int rc = t ? transform_bitrev(t, x, d->tree_f, false, false, (uint32_t)m, st)  // all of them at once
                       : narrow_transform(d->tree_top, lv + 1, lgT - lv, x, d->tree_f, false);
            if (rc != FASTECC_OK) return rc;
            const uint32_t scale = gf::h_to_mont(gf::h_inv((uint32_t)(2 * deg)));
            hipLaunchKernelGGL(pointwise_pairs_kernel, grid_of(2 * deg * (m / 2)), dim3(256), 0, st, d->tree_f, d->tree_p, (uint32_t)m, 2 * deg * (m / 2), scale);
            HIP_TRY(hipGetLastError());
            rc = t ? transform_bitrev(t, d->tree_p, d->tree_p, true, true, (uint32_t)(m / 2), st)      // the products, back in natural order
                   : narrow_transform(d->tree_top, lv + 1, lgT - lv, d->tree_p, d->tree_p, true);  // (the unused columns ride along)
            if (rc != FASTECC_OK) return rc;
            const bool top = lv + 1 == lgT;
            const uint64_t rows = top ? 2 * deg : 4 * deg;
            hipLaunchKernelGGL(combine_kernel, grid_of(rows * (m / 2)), dim3(256), 0, st, d->tree_p, x, spare, (uint32_t)deg, (uint32_t)m, rows * (m / 2), top);
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
        hipLaunchKernelGGL(locator_columns_kernel, grid_of(NC), dim3(256), 0, st, coeffs, d->pattern_buf, (uint32_t)T, (uint32_t)NC);
        HIP_TRY(hipGetLastError());
        // (power of two: the values stay in bit-reversed order, finish_tables_kernel reads them there — the reordering pass of fastecc_ntt was 87 us)
        const int rc = mixed               ? mixed_dif(d->pattern_ntt, d->pattern_buf, d->pattern_buf, st)
                       : d->pattern_narrow ? narrow_transform(d->pattern_ntt, lgc, 1, d->pattern_buf, d->pattern_buf, false)
                                           : transform_bitrev(d->pattern_ntt, d->pattern_buf, d->pattern_buf, false, false, 2, st);
        if (rc != FASTECC_OK) return rc;
        hipLaunchKernelGGL(finish_tables_kernel, grid_of(NC), dim3(256), 0, st, d->pattern_buf, (const uint32_t*)d->dev_state.get(), d->wpow, d->fin, d->gout, (uint32_t)NC,
                           (uint32_t)(T - s.erased_count), e, (uint32_t)c->K, (uint32_t)(mixed ? c->q : 1), lgc, parity_factors ? d->gout_par.get() : nullptr,
                           !mixed);
        HIP_TRY(hipGetLastError());
        if (d->fin_first_pass != d->fin) {
            hipLaunchKernelGGL(permute_kernel, grid_of(NC), dim3(256), 0, st, d->fin, d->tile_order, d->fin_first_pass, (uint32_t)NC);
            HIP_TRY(hipGetLastError());
        }
        if (s.split_groups == 0 || !d->split) return FASTECC_OK;
        // (fastecc_repair in the (2k,k) layout: the lost parity blocks' factors too — gout_par is filled above for such patterns)
        const bool with_parity = parity_factors && d->gout_par != nullptr;
        hipLaunchKernelGGL(split_rows_kernel, grid_of(N), dim3(256), 0, st, d->fin, d->gout, d->split_order, d->split_rows_data, d->split_rows_parity,
                           d->split_rows_out, (uint32_t)N, with_parity ? d->gout_par.get() : nullptr, with_parity ? d->split_rows_out_parity.get() : nullptr);
        d->split_repair_ready = with_parity;
        HIP_TRY(hipGetLastError());
        d->split_shift = s.split_shift;
        if (s.split_shift == 0 && d->split_dirty > s.split_groups) {
            // rows of groups this pattern does not write any more: group g = blocks g + (t << 10)
            const size_t row = c->S * 4;
            HIP_TRY(hipMemset2DAsync(d->split_r1 + (size_t)s.split_groups * c->S, 1024 * row, 0, (d->split_dirty - s.split_groups) * row,
                                     split_decode_group_rows(d->split), st));
            d->split_dirty = s.split_groups;
        }
        d->split_groups = s.split_shift == 0 ? s.split_groups : 0;
        d->split_ready = true;
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

// ---- fastecc_decode / fastecc_repair ----
// The 64-bit field's decode (gf61_decode.hip).  Codes other than (2N,N): the padded (2N,N) codeword is decoded in the context's two work stripes
// and the caller's blocks are copied back.  The caller holds c->mu.
int decode_p61(fastecc_ctx* c, void* data, const void* parity, int mem_kind, hipStream_t st, void* parity_out)
{
    if ((((uintptr_t)data | (uintptr_t)parity) & 15u)) return FASTECC_E_INVAL;
    p61::Decoder* d61 = c->decoder61;
    if (!p61::decoder_ready(d61)) return FASTECC_E_INVAL;
    DeviceGuard dg(c->device);
    if (!dg.ok) return FASTECC_E_DEVICE;
    return with_internal_buffers(c, st, [&]() -> int {  // the decoder's work stripe and tables are internal buffers
        P61Hooks hk(c);
        const p61::LaunchHooks* hooks = c->profiling ? &hk.h : nullptr;
        p61::Path* encoder = parity_out ? c->p61.get() : nullptr;
        if (!zero_extended(c))
            return mem_kind == FASTECC_MEM_DEVICE ? p61::decode(d61, (uint64_t*)data, (uint64_t*)const_cast<void*>(parity), encoder, st, hooks)
                                                  : p61::decode_host(d61, data, const_cast<void*>(parity), encoder, st, hooks);
        if (mem_kind != FASTECC_MEM_DEVICE) return FASTECC_E_UNSUPPORTED;
        const size_t row = c->S * 4, prow = row * (size_t)c->p61_stride;
        uint64_t *wd = nullptr, *wp = nullptr;
        int rc = p61_work_stripes(c, &wd, &wp);
        auto step = [&](hipError_t e, const char* what) {
            if (rc == FASTECC_OK && e != hipSuccess) rc = hip_fail(e, what);
        };
        if (rc == FASTECC_OK) {
            step(hipMemcpyAsync(wd, data, c->K * row, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync(data)");
            step(hipMemsetAsync((char*)wd + c->K * row, 0, (c->N - c->K) * row, st), "hipMemsetAsync");
            step(hipMemcpy2DAsync(wp, prow, parity, row, row, c->Mu, hipMemcpyDeviceToDevice, st), "hipMemcpy2DAsync(parity)");
        }
        if (rc == FASTECC_OK) rc = p61::decode(d61, wd, wp, encoder, st, hooks);
        if (rc == FASTECC_OK) {
            step(hipMemcpyAsync(data, wd, c->K * row, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync(data back)");
            if (parity_out) step(hipMemcpy2DAsync(parity_out, row, wp, prow, row, c->Mu, hipMemcpyDeviceToDevice, st), "hipMemcpy2DAsync(parity back)");
        }
        return rc;
    });
}

// The direct path's passes over a stripe or a batch: run(p, parity_in, data_out, parity_out) runs one of them.  Data and parity lost with a table
// for both: one pass over the survivors writes both (fastecc_decode: the data only); else the lost data, then (rebuild) the lost parity from it.
template <class Run> int direct_passes(const DecodeState* d, bool rebuild, uint32_t* data, const uint32_t* parity, uint32_t* parity_out, Run&& pass)
{
    if (d->sub_both && (rebuild || d->sub_only_both)) return pass(d->direct.both, parity, data, rebuild ? parity_out : nullptr);
    if (d->sub_lost_data > 0) {
        const int rc = pass(d->direct.data, parity, data, nullptr);
        if (rc != FASTECC_OK) return rc;
    }
    return rebuild ? pass(d->direct.parity, nullptr, nullptr, parity_out) : FASTECC_OK;
}

// One stripe's decode of a GF(0xFFF00001) code, the call lock held and the internal buffers ordered on `st`
struct StripeDecode {
    fastecc_ctx* c;
    DecodeState* d;
    hipStream_t st;
    bool rebuild;            // fastecc_repair of a pattern that lost parity blocks
    uint32_t* data;          // the data stripe on the device (FASTECC_MEM_HOST: the staging copy)
    const uint32_t* parity;  // the parity stripe ...
    uint32_t* parity_out;    // where the rebuilt parity blocks go
    uint64_t N;              // the transform order
    size_t block;            // bytes per block
    uint32_t S;              // words per block

    // FASTECC_MEM_HOST: the codeword staged in the decoder's stripe (parity, then data) — of the parity stripe only what the decoder will read where
    // that is known to be a few blocks or block groups.  *rows_only: only the rebuilt blocks will travel back (few enough of them, their rows known).
    int stage_host(const void* host_data, const void* host_parity, bool* rows_only)
    {
        const size_t data_bytes = c->K * block, parity_bytes = c->Mu * block;
        RC_TRY(d->parity_dev.alloc((c->Mu + c->K) * S));
        if (d->host_lists_of != d->pattern_serial) {
            // the rows that travel back: known from the set-up (few losses), else read off the decoder's tables once per pattern
            d->host_lost_data.clear();
            d->host_lost_parity.clear();
            if (d->erased_data + d->erased_parity <= (c->K + c->Mu) / 8 && d->parity_lost && (d->erased_data == 0 || d->gout)) {
                std::vector<uint32_t> flags(std::max(c->K, c->Mu));
                if (d->erased_data != 0) {
                    HIP_TRY(hipMemcpy(flags.data(), d->gout, c->K * 4, hipMemcpyDeviceToHost));
                    for (uint64_t i = 0; i < c->K; i++)
                        if (flags[i] != 0) d->host_lost_data.push_back((uint32_t)i);
                }
                HIP_TRY(hipMemcpy(flags.data(), d->parity_lost, c->Mu * 4, hipMemcpyDeviceToHost));
                for (uint64_t q = 0; q < c->Mu; q++)
                    if (flags[q] != 0) d->host_lost_parity.push_back((uint32_t)q);
                if (d->host_lost_data.size() != d->erased_data) d->host_lost_data.clear(), d->host_lost_parity.clear();  // (tables of another shape: whole stripes back)
            }
            d->host_lists_of = d->pattern_serial;
        }
        const uint64_t back = (d->erased_data != 0 ? d->host_lost_data.size() : 0) + (rebuild ? d->host_lost_parity.size() : 0);
        *rows_only = back != 0 && (d->erased_data == 0 || d->host_lost_data.size() == d->erased_data) &&
                     (!rebuild || d->host_lost_parity.size() == d->erased_parity) && back <= (c->K + c->Mu) / 8;
        const bool partial = !rebuild || *rows_only;  // (a repair that copies the whole parity stripe back must have staged all of it)
        const bool split = !d->sub && d->split_ready && d->standard && d->erased_data != 0 && partial;
        if (split && d->split_shift != 0) {
            // split transform, small form: the parity blocks at multiples of 2^shift are all it reads — one strided copy of every 2^shift-th block
            const size_t pitch = block << d->split_shift;
            HIP_TRY(hipMemcpy2DAsync(d->parity_dev, pitch, host_parity, pitch, block, (c->Mu + (1ull << d->split_shift) - 1) >> d->split_shift, hipMemcpyHostToDevice, st));
        } else if (split && d->split_groups < 512) {
            // group form: groups g < split_groups = blocks g + 1024 t, one strided copy
            HIP_TRY(hipMemcpy2DAsync(d->parity_dev, 1024 * block, host_parity, 1024 * block, (size_t)d->split_groups * block, c->Mu / 1024, hipMemcpyHostToDevice, st));
        } else if (d->sub && partial) {
            // few losses: the direct path reads as many parity blocks as data blocks are lost (at most 256 copies of a block)
            for (uint32_t q : d->host_parity_used)
                HIP_TRY(hipMemcpyAsync(d->parity_dev + (size_t)q * S, (const char*)host_parity + (size_t)q * block, block, hipMemcpyHostToDevice, st));
        } else {
            HIP_TRY(hipMemcpyAsync(d->parity_dev, host_parity, parity_bytes, hipMemcpyHostToDevice, st));
        }
        HIP_TRY(hipMemcpyAsync(d->parity_dev + c->Mu * S, host_data, data_bytes, hipMemcpyHostToDevice, st));
        parity = parity_out = d->parity_dev;
        data = d->parity_dev + c->Mu * S;
        return FASTECC_OK;
    }

    // any layout, few losses (profile: one "direct_pass" per read of the stripe)
    int direct()
    {
        return direct_passes(d, rebuild, data, parity, parity_out, [&](DirectPass* p, const uint32_t* par_in, uint32_t* data_to, uint32_t* par_to) {
            ProfScope ps(c, st, "direct_pass", (c->K + (uint64_t)d->sub_lost_data) * block);
            return direct_run(p, data, par_in, data_to, par_to, S, d->direct_kernel, st);
        });
    }

    // The transform path: fastecc_repair in one transform where the pattern's tables allow it, else the lost data and then the lost parity from
    // one more encode
    int transform()
    {
        if (rebuild && d->erased_data != 0) {
            bool done = false;
            int rc = d->split_ready && d->split_repair_ready ? repair_split(&done) : FASTECC_OK;
            if (rc == FASTECC_OK && !done && d->standard && d->transform_full && d->full_ok && d->gout_par) rc = repair_full(&done);
            if (rc != FASTECC_OK || done) return rc;
        }
        if (d->erased_data != 0) {
            const int rc = decode_data();
            if (rc != FASTECC_OK) return rc;
        }
        return rebuild ? reencode_parity() : FASTECC_OK;
    }

    // split transform, small form: the rows of the parity half in use (multiples of 2^shift), times l, and their stand-alone DIF in place; then
    // the split transform over the data stripe and that addend, whose last pass writes the rebuilt blocks into the data stripe (odd: fastecc_repair's
    // second chain too).  (The gather reads parity block (h >> fold) for position h itself: no staging stripe for codes with fewer parity blocks.)
    int split_small(const SplitRepair* odd)
    {
        launch_rows(split_small_gather_kernel<4>, split_small_gather_kernel<1>, N >> d->split_shift, S, {parity, d->split_small_buf}, st, parity, d->split_small_buf,
                    d->fin, S, (int)d->split_shift, c->fold, (uint32_t)c->Mu);
        HIP_TRY(hipGetLastError());
        const int rc = transform_bitrev(d->split_small[d->split_shift], d->split_small_buf, d->split_small_buf, false, true, S, st);
        if (rc != FASTECC_OK) return rc;
        return run_split_decode(d->split, data, nullptr, d->split_rows_data, nullptr, 0, d->split_pos_parity, d->recovered, nullptr, nullptr, d->split_rows_out,
                                data, nullptr, (uint32_t)c->K, (uint32_t)c->Mu, st, odd, d->split_small_buf, d->split_shift);
    }

    // fastecc_repair through the split transform: the data chain as in fastecc_decode, and a second MID + DIT over the same two halves for x p'(x)
    // at the odd positions — the lost parity blocks, written straight into the parity stripe.  No room for the extra k-block stripe, or a plan the
    // form does not take: *done stays false.
    int repair_split(bool* done)
    {
        if (d->split_q2.try_alloc(N * S) != hipSuccess) {
            (void)hipGetLastError();
            return FASTECC_OK;
        }
        const SplitRepair odd{d->split_q2, d->split_pos_data_odd, d->split_rows_out_parity, parity_out};
        d->split_dirty = std::max(d->split_dirty, d->split_groups);  // (before the launches: a failure half way must not hide written groups)
        ProfScope ps(c, st, "repair_split_transform", (5 * N + (uint64_t)d->split_groups * split_decode_group_rows(d->split)) * block);
        const int rc = d->split_shift != 0 ? split_small(&odd)
                                           : run_split_decode(d->split, data, parity, d->split_rows_data, d->split_rows_parity, d->split_groups, d->split_pos_parity,
                                                              d->recovered, d->split_r1, d->split_r2, d->split_rows_out, data, d->split_impulse,
                                                              (uint32_t)c->K, (uint32_t)c->Mu, st, &odd);
        if (rc == FASTECC_E_UNSUPPORTED) return FASTECC_OK;
        *done = rc == FASTECC_OK;
        return rc;
    }

    // fastecc_repair, (2k,k) layout: x p'(x) at all 2k positions — the even rows give the lost data, the odd rows the lost parity.  No room for
    // the 2k-block stripe, or a plan whose first pass cannot read the codeword: *done stays false.
    int repair_full(bool* done)
    {
        if (d->recovered_full.try_alloc(d->positions * S) != hipSuccess) {
            (void)hipGetLastError();
            return FASTECC_OK;
        }
        const int rc = run_gathered(d->transform_full, data, parity, d->fin_first_pass, d->recovered_full, st);
        if (rc != FASTECC_OK) return rc == FASTECC_E_UNSUPPORTED ? FASTECC_OK : rc;
        launch_rows(decode_scatter_kernel<4>, decode_scatter_kernel<1>, N, S, {data, parity_out, d->recovered_full}, st, d->recovered_full, data, d->gout, S, 2u * S, S);
        launch_rows(decode_scatter_kernel<4>, decode_scatter_kernel<1>, N, S, {data, parity_out, d->recovered_full}, st, d->recovered_full + S, parity_out, d->gout_par,
                    S, 2u * S, S);
        HIP_TRY(hipGetLastError());
        *done = true;
        return FASTECC_OK;
    }

    // The lost data through the split transform (two half-size transforms instead of one of size 2k, see "even / odd split"), whose last pass
    // writes the rebuilt blocks straight into the data stripe.  FASTECC_E_UNSUPPORTED: not on this plan, or no room for the staging stripe.
    int decode_split()
    {
        if (d->split_shift != 0) {
            ProfScope ps(c, st, "decode_split_transform", (3 * N + 3 * (N >> d->split_shift)) * block);
            return split_small(nullptr);
        }
        if (c->fold > 0 && d->split_r0.try_alloc(N * S) != hipSuccess) {
            (void)hipGetLastError();
            return FASTECC_E_UNSUPPORTED;
        }
        ProfScope ps(c, st, "decode_split_transform", (3 * N + (uint64_t)d->split_groups * split_decode_group_rows(d->split)) * block);
        const uint32_t* parity_half = parity;
        uint32_t parity_half_blocks = (uint32_t)c->Mu;
        if (c->fold > 0) {
            // fewer parity blocks than data blocks: block j belongs at j << fold of the parity half — the blocks in use are copied there
            launch_rows(split_stage_kernel<4>, split_stage_kernel<1>, c->Mu, S, {parity, d->split_r0}, st, parity, d->split_r0, d->fin, S, c->fold);
            parity_half = d->split_r0;
            parity_half_blocks = (uint32_t)N;
        }
        d->split_dirty = std::max(d->split_dirty, d->split_groups);  // (before the launches, as in repair_split)
        return run_split_decode(d->split, data, parity_half, d->split_rows_data, d->split_rows_parity, d->split_groups, d->split_pos_parity, d->recovered,
                                d->split_r1, d->split_r2, d->split_rows_out, data, d->split_impulse, (uint32_t)c->K, parity_half_blocks, st);
    }

    // The lost data blocks: the split transform, else the 2k-point one.  The (2k,k) layout lets the transform's first pass read the two halves of
    // the codeword itself (no gather pass).  The other codes do not hold every position in memory: they take the table-driven gather, which never
    // touches a position whose factor is zero, instead of a tile that reads first and multiplies by zero afterwards.
    int decode_data()
    {
        int rc = d->split_ready ? decode_split() : FASTECC_E_UNSUPPORTED;
        if (rc == FASTECC_OK) return FASTECC_OK;
        if (rc == FASTECC_E_UNSUPPORTED && d->standard) {
            ProfScope ps(c, st, "decode_transform_2k", 3 * N * block);
            rc = run_gathered(d->transform, data, parity, d->fin_first_pass, d->recovered, st);
        }
        const bool fused = rc == FASTECC_OK;
        if (!fused && rc != FASTECC_E_UNSUPPORTED) return rc;
        uint32_t* work = d->recovered;
        if (!d->mixed && !fused && (rc = scratch_of(d->transform, &work)) != FASTECC_OK) return rc;  // (only the unfused form gathers into it)
        if (!fused) {
            launch_rows(decode_gather_kernel<4>, decode_gather_kernel<1>, d->positions, S, {data, parity, work, d->recovered}, st, data, parity, work, d->fin,
                        d->srcmap, S, S, S);
            HIP_TRY(hipGetLastError());
            rc = fastecc_encode(d->transform, work, d->mixed ? work : d->recovered, FASTECC_MEM_DEVICE, st);
            if (rc != FASTECC_OK) return rc;
        }
        // (mixed radix: data position i is row 2i of the transformed work stripe)
        launch_rows(decode_scatter_kernel<4>, decode_scatter_kernel<1>, N, S, {data, parity, work, d->recovered}, st, d->recovered, data, d->gout, S,
                    d->mixed ? 2u * S : S, S);
        HIP_TRY(hipGetLastError());
        return FASTECC_OK;
    }

    // The lost parity blocks are whatever the encoder makes of the (now complete) data: one more encode into a stripe of the decoder's, from which
    // only the lost blocks are copied — the surviving ones are left as they are
    int reencode_parity()
    {
        RC_TRY(d->parity_again.alloc(c->Mu * S));
        const int rc = encode_device(c, data, d->parity_again, st);
        if (rc != FASTECC_OK) return rc;
        launch_rows(restore_parity_kernel<4>, restore_parity_kernel<1>, c->Mu, S, {parity_out, d->parity_again}, st, d->parity_again, parity_out, d->parity_lost, S);
        HIP_TRY(hipGetLastError());
        return FASTECC_OK;
    }

    // FASTECC_MEM_HOST: the rebuilt blocks back to the caller's stripes.  rows_only: packed side by side on the device, one copy into a pinned
    // landing buffer, and a memcpy per block on the host — the repair has already run, so if one of the buffers of this shortcut cannot be had the
    // whole stripes go back instead.
    int copy_back(void* host_data, void* host_parity, bool rows_only)
    {
        const uint64_t nd = d->erased_data != 0 ? d->host_lost_data.size() : 0, np = rebuild ? d->host_lost_parity.size() : 0;
        if (rows_only && d->lost_rows_dev.try_grow(nd + np) == hipSuccess && d->pack_dev.try_grow((nd + np) * S) == hipSuccess &&
            d->pack_host.try_grow((nd + np) * S) == hipSuccess) {
            if (nd) HIP_TRY(hipMemcpyAsync(d->lost_rows_dev, d->host_lost_data.data(), nd * 4, hipMemcpyHostToDevice, st));
            if (np) HIP_TRY(hipMemcpyAsync(d->lost_rows_dev + nd, d->host_lost_parity.data(), np * 4, hipMemcpyHostToDevice, st));
            if (nd)
                launch_rows(pack_rows_kernel<4>, pack_rows_kernel<1>, nd, S, {data, d->parity_dev, d->pack_dev}, st, (const uint32_t*)data, d->lost_rows_dev,
                            d->pack_dev, S);
            if (np)
                launch_rows(pack_rows_kernel<4>, pack_rows_kernel<1>, np, S, {data, d->parity_dev, d->pack_dev}, st, (const uint32_t*)d->parity_dev,
                            d->lost_rows_dev + nd, d->pack_dev + nd * S, S);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(d->pack_host, d->pack_dev, (nd + np) * (size_t)S * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            for (uint64_t r = 0; r < nd; r++) memcpy((char*)host_data + (size_t)d->host_lost_data[r] * block, d->pack_host + r * S, block);
            for (uint64_t r = 0; r < np; r++) memcpy((char*)host_parity + (size_t)d->host_lost_parity[r] * block, d->pack_host + (nd + r) * S, block);
            return FASTECC_OK;
        }
        if (rows_only) (void)hipGetLastError();  // out of memory for the shortcut only
        if (d->erased_data != 0) {
            const int rc = stage_download(c, host_data, data, c->K * block, st);
            if (rc != FASTECC_OK) return rc;
        }
        if (rebuild) {
            const int rc = stage_download(c, host_parity, d->parity_dev, c->Mu * block, st);
            if (rc != FASTECC_OK) return rc;
        }
        HIP_TRY(hipStreamSynchronize(st));
        return FASTECC_OK;
    }
};

// one stripe (fastecc_decode_batch runs the transform path through this, stripe by stripe).  parity_out != null (== parity): also rebuild the lost
// parity blocks.  The caller holds c->mu.
int decode_locked(fastecc_ctx* c, void* data, const void* parity, int mem_kind, void* stream, void* parity_out)
{
    if (c->field == FASTECC_FIELD_GF_P61_SQUARED) return decode_p61(c, data, parity, mem_kind, (hipStream_t)stream, parity_out);
    DecodeState* d = c->decoder;
    if (!d || !d->ready) return FASTECC_E_INVAL;  // fastecc_decode_prepare first
    const bool rebuild = parity_out != nullptr && d->erased_parity != 0;
    if (d->erased_data == 0 && !rebuild) return FASTECC_OK;
    if (c->ld != c->S) return FASTECC_E_UNSUPPORTED;  // the gather / scatter passes address contiguous stripes
    DeviceGuard dg(c->device);
    if (!dg.ok) return FASTECC_E_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    return with_internal_buffers(c, st, [&]() -> int {  // the decoder's work stripes and tables are internal buffers
        StripeDecode j{c, d, st, rebuild, (uint32_t*)data, (const uint32_t*)parity, (uint32_t*)parity_out, transform_order(c), c->S * 4, (uint32_t)c->S};
        const bool host = mem_kind == FASTECC_MEM_HOST;
        bool rows_only = false;
        if (host) RC_TRY(j.stage_host(data, parity, &rows_only));
        RC_TRY(d->sub ? j.direct() : j.transform());
        return host ? j.copy_back(data, parity_out, rows_only) : FASTECC_OK;
    });
}

int decode_impl(fastecc_ctx* c, void* data, const void* parity, int mem_kind, void* stream, void* parity_out)
{
    if (!c || !data || !parity || (((uintptr_t)data | (uintptr_t)parity) & 3u)) return FASTECC_E_INVAL;
    if (c->sharded) return sharded_decode_stripe(c, data, const_cast<void*>(parity), mem_kind, parity_out != nullptr, (hipStream_t)stream);
    if (mem_kind == FASTECC_MEM_HOST_PINNED) mem_kind = FASTECC_MEM_HOST;  // the same staging; the copies are simply faster from pinned memory
    if (mem_kind != FASTECC_MEM_HOST && mem_kind != FASTECC_MEM_DEVICE) return FASTECC_E_INVAL;
    CallLock lk(c->mu);
    return decode_locked(c, data, parity, mem_kind, stream, parity_out);
}

// `count` stripes back to back in device memory, all with the prepared pattern.  The direct path runs each of its passes over the whole batch in
// one launch (direct_run_batch) when the pass has fewer than 4096 rows (from 4096 data rows on, the single-stripe path takes the matrix cores) and
// the batch gives at least one wave per SIMD; otherwise (option "decode_batch_kernel" decides when set) direct_run stripe by stripe.  Patterns of
// the transform path: the single-stripe decode, stripe by stripe.
// host_list / dev_list (the scrubber's repair_list; both or neither): the batch is the stripes list[0 .. count) of a pool whose extent the caller has
// checked.  The same choice between one launch and stripe by stripe; the batched launch reads the device copy, the loops the host copy.
int decode_batch_impl(fastecc_ctx* c, void* data, void* parity, uint64_t count, void* stream, bool repair, const uint64_t* host_list = nullptr,
                      const uint64_t* dev_list = nullptr)
{
    if (!c || !data || !parity || count == 0 || (((uintptr_t)data | (uintptr_t)parity) & 3u)) return FASTECC_E_INVAL;
    if (c->sharded) return FASTECC_E_UNSUPPORTED;
    CallLock lk(c->mu);
    if (c->field != FASTECC_FIELD_GF_FFF00001) return FASTECC_E_UNSUPPORTED;
    if (c->ld != c->S) return FASTECC_E_UNSUPPORTED;  // stripes of a batch are contiguous
    PoolExtent x;
    RC_TRY(pool_extent(c, data, parity, count, &x, !host_list));
    const uint64_t block = x.block;
    if ((host_list != nullptr) != (dev_list != nullptr)) return FASTECC_E_INVAL;
    auto stripe_of = [&](uint64_t b) { return host_list ? host_list[b] : b; };
    DecodeState* d = c->decoder;
    if (!d || !d->ready) return FASTECC_E_INVAL;  // fastecc_decode_prepare first
    const bool rebuild = repair && d->erased_parity != 0;
    if (d->erased_data == 0 && !rebuild) return FASTECC_OK;
    DeviceGuard dg(c->device);
    if (!dg.ok) return FASTECC_E_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    if (!d->sub) {
        // more losses than the direct path takes: correct, not faster than the caller's own loop
        for (uint64_t b = 0; b < count; b++) {
            char* pb = (char*)parity + stripe_of(b) * x.parity_bytes;
            RC_TRY(decode_locked(c, (char*)data + stripe_of(b) * x.data_bytes, pb, FASTECC_MEM_DEVICE, stream, repair ? pb : nullptr));
        }
        return FASTECC_OK;
    }
    const uint64_t S = c->S, data_words = c->K * S, parity_words = c->Mu * S;
    uint32_t* ddata = (uint32_t*)data;
    uint32_t* dparity = (uint32_t*)parity;
    auto run = [&](DirectPass* p, const uint32_t* par_in, uint32_t* data_to, uint32_t* par_to) -> int {
        const uint64_t rows = (uint64_t)direct_pass_rows(p);
        const int mode = c->decode_batch_kernel;
        const bool batched = mode == 1 || (mode == 0 && d->direct_kernel != 2 && rows < 4096 && direct_batch_waves(p, ddata, dparity, S, count) >= 1024);
        if (batched) {
            const uint64_t outputs = (data_to ? (uint64_t)d->sub_lost_data : 0) + (par_to ? (uint64_t)d->sub_lost_parity : 0);
            ProfScope ps(c, st, dev_list ? "direct_pass_list" : "direct_pass_batch", count * (rows + outputs) * block);
            return direct_run_batch(p, ddata, par_in, data_to, par_to, S, count, data_words, parity_words, st, dev_list);
        }
        ProfScope ps(c, st, "direct_pass", count * (c->K + (uint64_t)d->sub_lost_data) * block);
        for (uint64_t b = 0; b < count; b++) {
            const uint64_t sb = stripe_of(b);
            RC_TRY(direct_run(p, ddata + sb * data_words, par_in ? par_in + sb * parity_words : nullptr, data_to ? data_to + sb * data_words : nullptr,
                              par_to ? par_to + sb * parity_words : nullptr, (uint32_t)S, d->direct_kernel, st));
        }
        return FASTECC_OK;
    };
    return with_internal_buffers(c, st, [&] { return direct_passes(d, rebuild, ddata, dparity, dparity, run); });
}

// ---- fastecc_decode_prepare_set / _decode_batch_set / _repair_batch_set: a pattern per stripe ----

// one pattern on the host: lost data blocks, lost parity blocks, the surviving parity blocks that serve as nodes (one per lost data block)
struct LostLists {
    std::vector<uint32_t> R, Pl, A;
};

// The table-building part of fastecc_decode_prepare_set: the tables, kinds, classes and the device descriptor table of the patterns `lists` (each at
// most SET_MAX_LOST blocks) into the empty set `fresh`.  The context's device is current; touches no context state (the context's own set comes through
// here, and the scrubber's private one: repair_lost_sets).
int fill_pattern_set(fastecc_ctx* c, const std::vector<LostLists>& lists, PatternSet* fresh)
{
    const uint64_t P = lists.size();
    fresh->tables.resize(P);
    fresh->kind.assign(P, PatternSet::NOTHING);
    fresh->cls.assign(P, 0);
    fresh->rows.assign(P, 0);
    fresh->lost_data.assign(P, {});
    fresh->lost_parity.assign(P, {});
    std::vector<DirectSetPass> desc(P, DirectSetPass{});
    std::vector<uint32_t> lost_rows((P + 1) * SET_LOST_ROW, SET_LOST_END);
    Prepare geometry(c, nullptr, nullptr);
    PhaseTimer quiet;  // one line per set, not two per pattern
    quiet.on = false;
    for (uint64_t q = 0; q < P; q++) {
        const LostLists& l = lists[q];
        if (l.R.empty() && l.Pl.empty()) continue;  // nothing lost: its stripes are not touched
        int rc = geometry.direct_tables(l.R, l.Pl, l.A, fresh->tables[q], quiet);
        if (rc != FASTECC_OK) return rc;
        fresh->kind[q] = !l.R.empty() && !l.Pl.empty() ? PatternSet::BOTH : !l.R.empty() ? PatternSet::DATA : PatternSet::PARITY;
        if ((rc = direct_set_describe(fresh->pass(q), &desc[q])) != FASTECC_OK) return rc;
        while ((1u << fresh->cls[q]) < desc[q].cstride) fresh->cls[q]++;
        fresh->rows[q] = desc[q].rows;
        fresh->lost_data[q] = l.R;
        fresh->lost_parity[q] = l.Pl;
        std::sort(fresh->lost_parity[q].begin(), fresh->lost_parity[q].end());
        std::copy(fresh->lost_parity[q].begin(), fresh->lost_parity[q].end(), lost_rows.begin() + q * SET_LOST_ROW);  // (at most SET_MAX_LOST < SET_LOST_ROW)
    }
    RC_TRY(fresh->d_passes.alloc(P));
    HIP_TRY(hipMemcpy(fresh->d_passes, desc.data(), P * sizeof(DirectSetPass), hipMemcpyHostToDevice));
    RC_TRY(fresh->d_lost_parity.alloc(lost_rows.size()));
    HIP_TRY(hipMemcpy(fresh->d_lost_parity, lost_rows.data(), lost_rows.size() * 4, hipMemcpyHostToDevice));
    return FASTECC_OK;
}

// The new set is built aside and swapped in at the end: a refused or failed call leaves the previous one in force.
int prepare_set_impl(fastecc_ctx* c, const uint8_t* data_present, const uint8_t* parity_present, uint64_t P)
{
    if (!c || P > SET_MAX_PATTERNS || (P > 0 && (!data_present || !parity_present))) return FASTECC_E_INVAL;
    if (c->sharded) return FASTECC_E_UNSUPPORTED;
    if (c->field != FASTECC_FIELD_GF_FFF00001 || c->ld != c->S || c->K >= 0xFFFFFFF0ull) return FASTECC_E_UNSUPPORTED;
    // every pattern's lists first, on the host
    std::vector<LostLists> lists(P);
    bool too_many = false;
    for (uint64_t q = 0; q < P; q++) {
        const uint8_t* dp = data_present + q * c->K;
        const uint8_t* pp = parity_present + q * c->Mu;
        LostLists& l = lists[q];
        uint64_t lost = 0;
        each_lost(dp, c->K, [&](uint64_t i) {
            if (++lost <= SET_MAX_LOST) l.R.push_back((uint32_t)i);
            return true;
        });
        each_lost(pp, c->Mu, [&](uint64_t j) {
            if (++lost <= SET_MAX_LOST) l.Pl.push_back((uint32_t)j);
            return true;
        });
        if (lost > c->Mu) return FASTECC_E_INVAL;  // fewer than k blocks survive: not decodable
        too_many |= lost > SET_MAX_LOST;
        for (uint64_t j = 0; j < c->Mu && !too_many && l.A.size() < l.R.size(); j++)
            if (pp[j]) l.A.push_back((uint32_t)j);
    }
    if (too_many) return FASTECC_E_UNSUPPORTED;
    DeviceGuard dg(c->device);
    if (!dg.ok) return FASTECC_E_DEVICE;
    CallLock lk(c->mu);
    PatternSet* fresh = nullptr;
    struct DropFresh {  // (whatever was built goes unless it became the context's set)
        PatternSet*& f;
        ~DropFresh() { destroy_pattern_set(f); }
    } drop{fresh};
    if (P > 0) {
        if (!(fresh = new (std::nothrow) PatternSet())) return FASTECC_E_NOMEM;
        PhaseTimer pt("[fastecc prepare_set]");
        RC_TRY(fill_pattern_set(c, lists, fresh));
        pt.mark("tables of the set");
    }
    RC_TRY(wait_idle(c));  // device work that still uses the previous set (its tables, its list buffer)
    if (fresh && c->pattern_set) {  // the list buffers outlive a set
        fresh->list = std::move(c->pattern_set->list);
        fresh->list.pending = false;  // (the wait above outlasted the last copy out of the pinned side)
    }
    std::swap(c->pattern_set, fresh);  // (DropFresh frees the previous set)
    return FASTECC_OK;
}

// The launch part of fastecc_decode_batch_set / _repair_batch_set, on a locked context: `count` stripes of the pool, item i = stripe stripe_of(i) with
// pattern pattern_at(i) of the set s (FASTECC_PATTERN_NONE: not touched) — the pool's stripes under the caller's pattern_of (decode_batch_set_impl), or a
// list of stripes each with its pass (repair_lost_sets).
// The stripes that have work are sorted by the pad class of their pattern's pass; a class is ONE launch of direct_set_kernel when all its passes
// read fewer than 4096 rows (from 4096 data rows on, the single-stripe path takes the matrix cores), else direct_run stripe by stripe with each
// stripe's own table; option "decode_batch_kernel" decides when set.
template <class StripeOf, class PatternAt>
int run_pattern_set(fastecc_ctx* c, PatternSet* s, void* data, void* parity, uint64_t block, uint64_t count, StripeOf stripe_of, PatternAt pattern_at, void* stream,
                    bool repair)
{
    const uint64_t P = s->tables.size();
    constexpr int CLASSES = 5;
    // the pass stripe b takes in this call: none for FASTECC_PATTERN_NONE, a pattern that lost nothing, and (decode) one that lost only parity
    auto work_of = [&](uint32_t q) { return q != FASTECC_PATTERN_NONE && s->kind[q] != PatternSet::NOTHING && (repair || s->kind[q] != PatternSet::PARITY); };
    uint64_t per_class[CLASSES] = {}, total = 0;
    uint32_t rows_max[CLASSES] = {};
    for (uint64_t b = 0; b < count; b++) {
        const uint32_t q = pattern_at(b);
        if (q != FASTECC_PATTERN_NONE && q >= P) return FASTECC_E_INVAL;
        if (!work_of(q)) continue;
        per_class[s->cls[q]]++;
        rows_max[s->cls[q]] = std::max(rows_max[s->cls[q]], s->rows[q]);
        total++;
    }
    if (total == 0) return FASTECC_OK;
    DeviceGuard dg(c->device);
    if (!dg.ok) return FASTECC_E_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    RC_TRY(s->list.reserve(total, [&] { return wait_idle(c); }));  // (growing waits for the kernels that read the device list)
    uint64_t first[CLASSES], at[CLASSES], moved[CLASSES] = {};  // a class's entries: [first, first + per_class); blocks its passes read and write
    for (int k = 0; k < CLASSES; k++) first[k] = at[k] = k ? first[k - 1] + per_class[k - 1] : 0;
    for (uint64_t b = 0; b < count; b++) {
        const uint32_t q = pattern_at(b);
        if (q != FASTECC_PATTERN_NONE && q >= P) return FASTECC_E_INVAL;  // (the caller's array changed under the call)
        if (!work_of(q)) continue;
        const int k = s->cls[q];
        if (at[k] >= first[k] + per_class[k]) return FASTECC_E_INVAL;
        s->list.host[at[k]++] = DirectSetEntry{stripe_of(b), q, 0};
        moved[k] += (uint64_t)s->rows[q] + (uint64_t)s->tables[q].ed + (repair ? (uint64_t)s->tables[q].ep : 0);
    }
    const uint64_t S = c->S, data_words = c->K * S, parity_words = c->Mu * S;
    uint32_t* ddata = (uint32_t*)data;
    uint32_t* dparity = (uint32_t*)parity;
    const int mode = c->decode_batch_kernel;
    bool kernel[CLASSES], any_kernel = false;
    for (int k = 0; k < CLASSES; k++) {
        kernel[k] = at[k] > first[k] && (mode == 1 || (mode == 0 && rows_max[k] < 4096)) && direct_set_waves_per_entry(1 << k, data, parity, S) <= (1ull << 24);
        any_kernel |= kernel[k];
    }
    return with_internal_buffers(c, st, [&]() -> int {  // the set's tables and the list are internal buffers
        if (any_kernel) RC_TRY(s->list.publish(total, st));
        for (int k = 0; k < CLASSES; k++) {
            const uint64_t n = at[k] - first[k];
            if (n == 0) continue;
            if (kernel[k]) {
                ProfScope ps(c, st, "direct_pass_set", moved[k] * block);
                RC_TRY(direct_run_set(1 << k, s->d_passes, s->list.dev + first[k], n, ddata, dparity, ddata, repair ? dparity : nullptr, S, data_words, parity_words, st));
                continue;
            }
            ProfScope ps(c, st, "direct_pass", moved[k] * block);
            for (uint64_t i = first[k]; i < at[k]; i++) {
                const uint64_t b = s->list.host[i].stripe;
                const uint32_t q = s->list.host[i].pass;
                uint32_t* db = ddata + b * data_words;
                uint32_t* pb = dparity + b * parity_words;
                const bool reads_parity = s->kind[q] != PatternSet::PARITY, writes_data = reads_parity, writes_parity = repair && s->kind[q] != PatternSet::DATA;
                RC_TRY(direct_run(s->pass(q), db, reads_parity ? pb : nullptr, writes_data ? db : nullptr, writes_parity ? pb : nullptr, (uint32_t)S, c->direct_kernel, st));
            }
        }
        return FASTECC_OK;
    });
}

// `count` stripes back to back in device memory, stripe b with pattern pattern_of[b] of the prepared set: the argument checks, then run_pattern_set
int decode_batch_set_impl(fastecc_ctx* c, void* data, void* parity, uint64_t count, const uint32_t* pattern_of, void* stream, bool repair)
{
    if (!c || !data || !parity || !pattern_of || count == 0 || (((uintptr_t)data | (uintptr_t)parity) & 3u)) return FASTECC_E_INVAL;
    if (c->sharded) return FASTECC_E_UNSUPPORTED;
    CallLock lk(c->mu);
    if (c->field != FASTECC_FIELD_GF_FFF00001) return FASTECC_E_UNSUPPORTED;
    if (c->ld != c->S) return FASTECC_E_UNSUPPORTED;  // stripes of a pool are contiguous
    PoolExtent x;
    RC_TRY(pool_extent(c, data, parity, count, &x));
    PatternSet* s = c->pattern_set;
    if (!s) return FASTECC_E_INVAL;  // fastecc_decode_prepare_set first
    return run_pattern_set(c, s, data, parity, x.block, count, [](uint64_t b) { return b; }, [&](uint64_t b) { return pattern_of[b]; }, stream, repair);
}

// ---- fastecc_read_batch / _read_batch_set: degraded reads ----
// The requested data blocks reads[0 .. n_reads) of a pool, words [col0, col0 + width) of each, into row u of `out`; the pool is only read.
// set_form: stripe b under pattern pattern_of[b] of the prepared set; else every stripe under the single prepared pattern (direct path only).
// The argument checks, the pool's extent, then every request on the host — (stripe, pattern, present or the block's output index in the pass that
// fastecc_decode_batch[_set] takes for the lost data) — and only when all of them are valid ONE launch of direct_read_kernel over the staged list.
int read_batch_impl(fastecc_ctx* c, const void* data, const void* parity, uint64_t count, const uint32_t* pattern_of, bool set_form, const uint64_t* reads,
                    uint64_t n_reads, uint64_t col0, uint64_t width, void* out, void* stream)
{
    if (!c || count == 0 || width == 0 || (set_form && !pattern_of)) return FASTECC_E_INVAL;
    if (n_reads > 0 && (!data || !parity || !reads || !out)) return FASTECC_E_INVAL;
    if (((uintptr_t)data | (uintptr_t)parity | (uintptr_t)out) & 3u) return FASTECC_E_INVAL;
    if (c->sharded) return FASTECC_E_UNSUPPORTED;
    CallLock lk(c->mu);
    if (c->field != FASTECC_FIELD_GF_FFF00001) return FASTECC_E_UNSUPPORTED;
    if (c->ld != c->S) return FASTECC_E_UNSUPPORTED;  // stripes of a pool are contiguous
    const uint64_t S = c->S, K = c->K;
    if (col0 > S || width > S - col0) return FASTECC_E_INVAL;
    PoolExtent x;
    RC_TRY(pool_extent(c, data, parity, count, &x));
    if (n_reads > UINT64_MAX / (width * 4u)) return FASTECC_E_INVAL;
    const uint64_t out_bytes = n_reads * width * 4u;
    const uint64_t o0 = (uint64_t)(uintptr_t)out, d0 = (uint64_t)(uintptr_t)data, p0 = (uint64_t)(uintptr_t)parity;
    if (o0 > UINT64_MAX - out_bytes) return FASTECC_E_INVAL;
    auto overlaps = [&](uint64_t base, uint64_t bytes) { return o0 < base + bytes && base < o0 + out_bytes; };
    if (n_reads > 0 && (overlaps(d0, count * x.data_bytes) || overlaps(p0, count * x.parity_bytes))) return FASTECC_E_INVAL;
    // the tables: the set's descriptor table, or the single pattern's pass for the lost data
    PatternSet* s = nullptr;
    DecodeState* d = nullptr;
    DirectPass* single = nullptr;  // (null: the single pattern lost no data block — every request is a copy)
    if (set_form) {
        if (!(s = c->pattern_set)) return FASTECC_E_INVAL;  // fastecc_decode_prepare_set first
    } else {
        d = c->decoder;
        if (!d || !d->ready) return FASTECC_E_INVAL;  // fastecc_decode_prepare first
        // a pattern of the transform path is not served — but a pattern that lost NOTHING has no tables on either path (Prepare::direct leaves it to
        // transform_path, which finds nothing to build): it has no lost data block, so every request is a copy.  (erased_total is no measure of
        // that: on the transform path it counts the positions of a folded or zero-extended code that hold no block.)
        if (!d->sub && (d->erased_data != 0 || d->erased_parity != 0)) return FASTECC_E_UNSUPPORTED;
        if (d->sub && d->sub_lost_data > 0) {
            single = d->sub_both && d->sub_only_both ? d->direct.both.get() : d->direct.data.get();
            if (!single || d->host_lost_data.size() != (size_t)d->sub_lost_data) return FASTECC_E_DEVICE;
        }
    }
    if (n_reads == 0) return FASTECC_OK;
    const uint64_t P = s ? s->tables.size() : 0, blocks = count * K;  // (count * K * block fits 64 bits: pool_extent)
    const uint32_t single_rows = single ? (uint32_t)direct_pass_rows(single) : 0;
    const bool small = blocks <= 0xFFFFFFFFull;
    // request u -> its entry and the rows its wave reads
    auto translate = [&](uint64_t u, DirectReadEntry* ent, uint64_t* rows_read) -> int {
        const uint64_t idx = reads[u];
        if (idx >= blocks) return FASTECC_E_INVAL;
        const uint64_t b = small ? (uint64_t)((uint32_t)idx / (uint32_t)K) : idx / K;  // (the common case: a 32-bit division)
        const uint32_t i = (uint32_t)(idx - b * K);
        *ent = DirectReadEntry{b, 0, i, DIRECT_READ_PRESENT, 0};
        *rows_read = 1;
        if (set_form) {
            const uint32_t q = pattern_of[b];
            if (q == FASTECC_PATTERN_NONE) return FASTECC_OK;
            if (q >= P) return FASTECC_E_INVAL;
            if (s->kind[q] != PatternSet::DATA && s->kind[q] != PatternSet::BOTH) return FASTECC_OK;
            const std::vector<uint32_t>& R = s->lost_data[q];
            for (size_t j = 0; j < R.size(); j++)
                if (R[j] == i) {
                    ent->pass = q;
                    ent->out = (uint32_t)j;
                    *rows_read = s->rows[q];
                    break;
                }
            return FASTECC_OK;
        }
        if (single) {
            const std::vector<uint32_t>& R = d->host_lost_data;  // increasing (Prepare::direct)
            const auto it = std::lower_bound(R.begin(), R.end(), i);
            if (it != R.end() && *it == i) {
                ent->out = (uint32_t)(it - R.begin());
                *rows_read = single_rows;
            }
        }
        return FASTECC_OK;
    };
    const uint32_t* ddata = (const uint32_t*)data;
    const uint32_t* dparity = (const uint32_t*)parity;
    if (direct_read_waves_per_entry(data, parity, out, S, col0, width) > (1ull << 24)) return FASTECC_E_UNSUPPORTED;
    DeviceGuard dg(c->device);
    if (!dg.ok) return FASTECC_E_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    // ONE pass over the requests, straight into the pinned side of the list (reserve allocates, and waits for the previous call's copy; it enqueues
    // nothing): a request that is refused leaves a half-written list that no device work ever sees
    StagedList<DirectReadEntry>& list = c->read_list;
    RC_TRY(list.reserve(n_reads, [&] { return wait_idle(c); }));  // (growing waits for the kernels that read the device list)
    uint64_t rows_total = 0;
    for (uint64_t u = 0; u < n_reads; u++) {
        uint64_t rows_read;
        RC_TRY(translate(u, &list.host[u], &rows_read));
        rows_total += rows_read + 1;
    }
    const DirectSetPass* passes = s ? s->d_passes.get() : nullptr;
    if (!set_form) {
        if (single && d->read_desc_of != d->pattern_serial) {
            // (no read that used the previous descriptor is in flight: fastecc_decode_prepare waited for them before it rebuilt the tables)
            DirectSetPass desc;
            RC_TRY(direct_read_describe(single, &desc));
            RC_TRY(d->read_desc.alloc(1));
            HIP_TRY(hipMemcpy(d->read_desc, &desc, sizeof(desc), hipMemcpyHostToDevice));
            d->read_desc_of = d->pattern_serial;
        }
        RC_TRY(d->read_desc.alloc(1));  // (a pattern that lost no data: the table is never read, but the launch takes a pointer)
        passes = d->read_desc.get();
    }
    return with_internal_buffers(c, st, [&]() -> int {  // the tables and the list are internal buffers
        RC_TRY(list.publish(n_reads, st));
        ProfScope ps(c, st, set_form ? "direct_read_set" : "direct_read", rows_total * width * 4u);
        return direct_run_read(passes, list.dev, n_reads, ddata, dparity, (uint32_t*)out, S, col0, width, K * S, c->Mu * S, st);
    });
}

}  // namespace

// The context's pattern set as the degraded writes see it (drivers.hpp; update.hip)
bool pattern_set_view(const fastecc_ctx* c, PatternSetView* out)
{
    const PatternSet* s = c->pattern_set;
    if (!s) return false;
    *out = PatternSetView{s->tables.size(), s->d_passes.get(), s->d_lost_parity.get()};
    return true;
}
const std::vector<uint32_t>& pattern_lost_data(const fastecc_ctx* c, uint64_t q) { return c->pattern_set->lost_data[q]; }
const std::vector<uint32_t>& pattern_lost_parity(const fastecc_ctx* c, uint64_t q) { return c->pattern_set->lost_parity[q]; }
uint32_t pattern_rows(const fastecc_ctx* c, uint64_t q) { return c->pattern_set->rows[q]; }

// The scrubber's grouped repair (drivers.hpp): a pattern set of the lost sets, private to the call — fill_pattern_set, run_pattern_set
// over the (stripe, set) list, and the set freed once the stream's work is done
int repair_lost_sets(fastecc_ctx* c, void* data, void* parity, const std::vector<std::vector<uint32_t>>& lost_sets, const std::vector<uint64_t>& stripes,
                     const std::vector<uint32_t>& set_of, void* stream)
{
    if (lost_sets.empty() || lost_sets.size() > SET_MAX_PATTERNS || stripes.empty() || stripes.size() != set_of.size()) return FASTECC_E_INVAL;
    std::vector<LostLists> lists(lost_sets.size());
    for (size_t q = 0; q < lost_sets.size(); q++) {
        LostLists& l = lists[q];
        if (lost_sets[q].size() > SET_MAX_LOST) return FASTECC_E_INVAL;
        std::vector<uint8_t> parity_lost(c->Mu, 0);
        for (uint32_t j : lost_sets[q]) {
            if (j >= c->K + c->Mu) return FASTECC_E_INVAL;
            if (j < c->K) {
                l.R.push_back(j);
            } else {
                l.Pl.push_back((uint32_t)(j - c->K));
                parity_lost[j - c->K] = 1;
            }
        }
        for (uint64_t j = 0; j < c->Mu && l.A.size() < l.R.size(); j++)
            if (!parity_lost[j]) l.A.push_back((uint32_t)j);
        if (l.A.size() != l.R.size()) return FASTECC_E_INVAL;  // fewer than k blocks survive
    }
    DeviceGuard dg(c->device);
    if (!dg.ok) return FASTECC_E_DEVICE;
    CallLock lk(c->mu);
    PatternSetPtr set;
    struct Settle {  // (declared after the set: the stream's work, which reads the set's tables and list, is over before the set goes, on every path)
        hipStream_t st;
        ~Settle() { (void)hipStreamSynchronize(st); }
    } settle{(hipStream_t)stream};
    set.reset(new (std::nothrow) PatternSet());
    if (!set) return FASTECC_E_NOMEM;
    PhaseTimer pt("[fastecc correct_batch_set]");
    RC_TRY(fill_pattern_set(c, lists, set));
    pt.mark("  private set: tables");
    return run_pattern_set(c, set, data, parity, c->S * 4, stripes.size(), [&](uint64_t i) { return stripes[i]; }, [&](uint64_t i) { return set_of[i]; }, stream, true);
}

int repair_list(fastecc_ctx* c, void* data, void* parity, const uint64_t* host_list, const uint64_t* dev_list, uint64_t count, void* stream)
{
    if (!host_list || !dev_list) return FASTECC_E_INVAL;
    return decode_batch_impl(c, data, parity, count, stream, true, host_list, dev_list);
}

}  // namespace fastecc

using namespace fastecc;

extern "C" {

int fastecc_decode_prepare(fastecc_ctx* c, const uint8_t* data_present, const uint8_t* parity_present)
{
    return guarded([&]() -> int { return decode_prepare_impl(c, data_present, parity_present); });
}

int fastecc_decode(fastecc_ctx* c, void* data, const void* parity, int mem_kind, void* stream)
{
    return guarded([&]() -> int { return decode_impl(c, data, parity, mem_kind, stream, nullptr); });
}

int fastecc_repair(fastecc_ctx* c, void* data, void* parity, int mem_kind, void* stream)
{
    return guarded([&]() -> int { return decode_impl(c, data, parity, mem_kind, stream, parity); });
}

int fastecc_decode_batch(fastecc_ctx* c, void* data, const void* parity, uint64_t count, void* stream)
{
    return guarded([&]() -> int { return decode_batch_impl(c, data, const_cast<void*>(parity), count, stream, false); });
}

int fastecc_repair_batch(fastecc_ctx* c, void* data, void* parity, uint64_t count, void* stream)
{
    return guarded([&]() -> int { return decode_batch_impl(c, data, parity, count, stream, true); });
}

int fastecc_decode_prepare_set(fastecc_ctx* c, const uint8_t* data_present, const uint8_t* parity_present, uint64_t n_patterns)
{
    return guarded([&]() -> int { return prepare_set_impl(c, data_present, parity_present, n_patterns); });
}

int fastecc_decode_batch_set(fastecc_ctx* c, void* data, const void* parity, uint64_t count, const uint32_t* pattern_of, void* stream)
{
    return guarded([&]() -> int { return decode_batch_set_impl(c, data, const_cast<void*>(parity), count, pattern_of, stream, false); });
}

int fastecc_repair_batch_set(fastecc_ctx* c, void* data, void* parity, uint64_t count, const uint32_t* pattern_of, void* stream)
{
    return guarded([&]() -> int { return decode_batch_set_impl(c, data, parity, count, pattern_of, stream, true); });
}

int fastecc_read_batch_set(fastecc_ctx* c, const void* data, const void* parity, uint64_t count, const uint32_t* pattern_of, const uint64_t* reads, uint64_t n_reads,
                           uint64_t col0_words, uint64_t width_words, void* out, void* stream)
{
    return guarded([&]() -> int { return read_batch_impl(c, data, parity, count, pattern_of, true, reads, n_reads, col0_words, width_words, out, stream); });
}

int fastecc_read_batch(fastecc_ctx* c, const void* data, const void* parity, uint64_t count, const uint64_t* reads, uint64_t n_reads, uint64_t col0_words,
                       uint64_t width_words, void* out, void* stream)
{
    return guarded([&]() -> int { return read_batch_impl(c, data, parity, count, nullptr, false, reads, n_reads, col0_words, width_words, out, stream); });
}

}  // extern "C"
