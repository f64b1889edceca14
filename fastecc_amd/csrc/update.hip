// update.hip — small writes: fastecc_update, fastecc_update_parity, their pool forms fastecc_update_batch, fastecc_update_parity_batch, the pool forms for
// stripes that miss blocks fastecc_update_batch_set, fastecc_update_parity_batch_set, and
// fastecc_code_coefficient (include/fastecc.h).
//
// The code is linear, so after data blocks i_u change by D_u = new_u - old_u the parity changes by
//     parity[q][w] += sum_u L_{i_u}(y_q) * D_u[w]   (mod p),
// L_i the Lagrange basis on the data points.  Every code of the library sits on the NC-th roots of unity (internal.hpp:
// code_parity_position): data block i at position i << e, parity block q at pos(q).  With x_i = w^(i << e), y = w^pos and
// L_i(y) = (y^N - 1) x_i / (N (y - x_i)) (direct.hip) the weight depends on the difference of positions only:
//     L_i(y_q) = G[(pos(q) - (i << e)) mod NC],   G[u] = (w^(uN) - 1) / (N (w^u - 1))   (u not a multiple of 2^e),
// so ONE table of NC words serves every data block, every parity block and every call.  For e = 1 only odd u occur and the table holds
// G[2v + 1] at v (NC / 2 words).
//
// A call runs in passes of up to ROWS changed blocks:
//   update_table_kernel : G in Montgomery form, one thread per entry, once per context (on the stream of the first call);
//   update_delta_kernel : D_u into the context's delta rows; fastecc_update also stores new_u into the stripe, after reading old_u;
//   update_parity_kernel: a wave owns a column slice of 64 V words and a run of parity blocks.  It loads the pass's T <= ROWS delta
//                         rows of its slice into VGPRs once, then streams its parity blocks: T wave-uniform weights from G (scalar
//                         loads behind one wait), T x V mac96 into 96-bit sums (lazy96.hpp), + the old parity word, one reduction, a
//                         non-temporal store.  The next block's parity load is in flight during the current block's arithmetic.
// The three parity kernels (this one and the two below) differ in how a wave finds its rows and forms the deltas.  From there on the two pool
// kernels call stream_parity with the position of row i and the next block to visit as callables; this one keeps the same loop written out, for
// a measured reason.  The host picks the instantiation <T, V> through with_class and V through lane_words.
//
// A pool of stripes stored back to back (fastecc_update_batch): G does not depend on the stripe, so nothing per stripe is
// built.  The host sorts the writes by (stripe, block), cuts each stripe's writes into segments of at most ROWS, and uploads the sorted list and
// the segment tables; the r-th segment of every stripe runs in round r (segments of one stripe read-modify-write the same parity blocks), one
// launch per padded segment length T in {1, 2, 4, 8, 16}:
//   update_batch_kernel  : a wave owns one segment, one column slice and one run of that stripe's parity blocks.  It forms D = new - old of its
//                          <= T rows in VGPRs (no delta buffer) and streams its parity blocks through stream_parity;
//   update_scatter_kernel: after the last round, fastecc_update_batch only: new_blocks row u into its data block (several waves of the parity
//                          kernel need the same old row, so the store waits for a later kernel on the same stream: no race, no flag).
//
// A pool whose stripes miss blocks (fastecc_update_batch_set / _update_parity_batch_set): stripe b under pattern pattern_of[b] of the
// set of fastecc_decode_prepare_set.  The same host code (update_batch_run with a SetForm; build_update_list, update_list.hpp, with its arrays), and on the stream
//   direct_run_read      : the old rows of the written data blocks that are absent, rebuilt into UpdateState::d_recon before any parity launch;
//   update_set_kernel    : update_batch_kernel with each old row at an offset the host chose (the pool, or d_recon) and the stripe's absent parity
//                          blocks skipped — neither loaded nor stored: stream_parity's next block is the next PRESENT one;
//   update_scatter_kernel: only the writes whose data block is present.
//
// One window of word columns [col0, col0 + width) of every written block (the four fastecc_update_*_window calls): the same host code
// once more (update_batch_run with a Window), rows of `width` words, and on the stream
//   direct_run_read             : the old WINDOWS of the absent written blocks, into d_recon at pitch width;
//   update_window_kernel        : update_set_kernel with the lane's columns counted from the window, for the set forms and the plain ones alike (a call
//                                 without a pattern set gives every stripe a row that loses nothing); no word outside the window is loaded or stored;
//   update_window_scatter_kernel: row u into the window of its present data block.
//
// The write list in device memory (fastecc_update_batch_device / _update_parity_batch_device): no host code looks at the list.
// update_device_run enqueues the reset of the per-stripe counters and the caller's status word, three kernels that build the records and the
// segment tables in the window form's formats (device_count_kernel, device_fill_kernel, device_segments_kernel), update_window_device_kernel per
// admitted length class — update_window_kernel's wave behind a look at the status and at the class's real segment count — and
// update_device_scatter_kernel straight from the caller's list.
//
// ... for a pool whose stripes miss blocks (fastecc_update_batch_set_device / _update_parity_batch_set_device): pattern_of is a
// device array as well.  The same driver with the set forms of the three build kernels — the lane that opens a stripe's segment reads and checks
// pattern_of[b]; a write to an absent data block draws a row of d_recon and its DirectReadEntry, the segment points at its pattern's lost parity blocks —
// then direct_run_read_device over those entries, the same update_window_device_kernel launches with the set's lost-parity table, and
// update_device_set_scatter_kernel, which leaves the absent blocks alone.
//
// The host side of the pool calls: the formats of the list and of the segment tables, sort_writes and build_update_list are in
// update_list.hpp, which needs no HIP; update_batch_run and update_device_run are written out of the same stages (pool_lanes, grow_behind_wait,
// pool_kernel_args, split_runs, launch_split).
#include <algorithm>
#include <atomic>
#include <vector>

#include "devmem.hpp"
#include "drivers.hpp"
#include "lazy96.hpp"
#include "ntt_device.hpp"
#include "update_list.hpp"

namespace fastecc {

namespace {

struct CodeGeom {
    uint64_t N = 0;  // transform order (q * 2^m for the mixed-radix codes)
    int e = 1, fold = 0, cosets = 1;
    uint64_t K = 0, Mu = 0;  // data and parity blocks of the caller's stripes
};

uint32_t geom_weight(const CodeGeom& g, uint64_t i, uint64_t q)
{
    const uint64_t NC = g.N << g.e;
    const uint64_t u = (code_parity_position(g.N, g.e, g.fold, g.cosets, q) + NC - (i << g.e)) % NC;
    const uint32_t w = gf::h_root((uint32_t)NC), wu = gf::h_pow(w, u);
    const uint32_t num = (uint32_t)(((uint64_t)gf::h_pow(wu, g.N) + gf::P - 1u) % gf::P);
    const uint32_t den = gf::h_mul((uint32_t)(g.N % gf::P), (uint32_t)(((uint64_t)wu + gf::P - 1u) % gf::P));
    return gf::h_mul(num, gf::h_inv(den));
}

// The geometry fastecc_create / fastecc_create_ex give (n, k, flags) over GF(0xFFF00001), without a device.
int geom_of_code(uint64_t n, uint64_t k, unsigned flags, CodeGeom* g)
{
    if (flags & ~(unsigned)(FASTECC_CODE_MIXED_RADIX | FASTECC_CODE_TOP_RADIX2 | FASTECC_CODE_MIXED_RADIX_PFA)) return FASTECC_E_INVAL;
    if (k < 1 || n <= k) return FASTECC_E_INVAL;
    g->K = k;
    g->Mu = n - k;
    if (flags & FASTECC_CODE_TOP_RADIX2) {  // the (2k,k) code through another kernel
        int lg = 0;
        while ((1ull << lg) < k) lg++;
        if (flags != FASTECC_CODE_TOP_RADIX2 || n != 2 * k || (1ull << lg) != k || lg < 12 || lg > 19) return FASTECC_E_UNSUPPORTED;
        g->N = k;
        return FASTECC_OK;
    }
    if (flags & (FASTECC_CODE_MIXED_RADIX | FASTECC_CODE_MIXED_RADIX_PFA)) {  // create.hip: the same choice as fastecc_create_ex
        int bq = 1, bm = 0;
        const uint64_t best = mixed_radix_order(k, flags, &bq, &bm);
        if (best == 0 || n - k > best) return FASTECC_E_UNSUPPORTED;
        if (bq > 1) {
            g->N = best;
            return FASTECC_OK;
        }
    }
    int lg = 0;
    const int rc = pow2_code_shape(n, k, &lg, &g->fold, &g->cosets);  // create.hip: the same rule as fastecc_create
    if (rc != FASTECC_OK) return rc;
    const uint64_t N1 = 1ull << lg;
    if (lg > 19 || (g->cosets > 1 && n > (1ull << 20))) return FASTECC_E_UNSUPPORTED;
    g->N = N1;
    g->e = code_coset_shift(g->cosets);
    return FASTECC_OK;
}

CodeGeom geom_of_ctx(const fastecc_ctx* c)
{
    CodeGeom g;
    g.N = (uint64_t)c->q * c->N;
    g.cosets = c->cosets;
    g.fold = c->fold;
    g.e = code_coset_shift(c->cosets);
    g.K = c->K;
    g.Mu = c->Mu;
    return g;
}

__device__ __forceinline__ uint32_t dev_pow(uint32_t x, uint64_t e)
{
    uint32_t r = 1;
    for (; e; e >>= 1) {
        if (e & 1u) r = gf::mul(r, x);
        x = gf::mul(x, x);
    }
    return r;
}

// G[v], u = (v << tshift) | tshift; Montgomery form; 0 where u is a multiple of 2^e (no weight has that index)
__global__ __launch_bounds__(256) void update_table_kernel(uint32_t* __restrict__ G, uint32_t words, uint32_t w, uint32_t N_mod_p, uint64_t N, uint32_t tshift,
                                                           uint32_t emask)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= words) return;
    const uint32_t u = (v << tshift) | tshift;
    uint32_t r = 0;
    if (u & emask) {
        const uint32_t wu = dev_pow(w, u);
        const uint32_t num = gf::sub(dev_pow(wu, N), 1u);
        const uint32_t den = gf::mul(N_mod_p, gf::sub(wu, 1u));
        r = gf::mul(gf::mul(num, dev_pow(den, gf::P - 2u)), gf::MONT_ONE);
    }
    G[v] = r;
}

struct DeltaArgs {
    uint32_t* data;              // fastecc_update: the stripe (old blocks read, new ones stored); else null
    const uint32_t* old_blocks;  // fastecc_update_parity: the pass's old blocks, contiguous (null: zero)
    const uint32_t* new_blocks;  // the pass's new blocks, contiguous
    uint32_t* delta;             // [rows][S]
    uint64_t S;
    uint32_t rows;               // rows of the pass; rows [rows, gridDim.y) of delta are zeroed (the parity kernel reads T rows)
    uint32_t idx[ROWS];          // data block of each row
};

// thread (word w, row r): delta[r][w] = new - old; the stripe gets new after old was read
__global__ __launch_bounds__(256) void update_delta_kernel(const DeltaArgs a)
{
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t r = blockIdx.y;
    if (w >= a.S) return;
    if (r >= a.rows) {
        a.delta[(uint64_t)r * a.S + w] = 0;
        return;
    }
    const uint32_t nv = a.new_blocks[(uint64_t)r * a.S + w];
    uint32_t ov = 0;
    if (a.data) {
        uint32_t* p = a.data + (uint64_t)a.idx[r] * a.S + w;
        ov = *p;
        *p = nv;
    } else if (a.old_blocks) {
        ov = a.old_blocks[(uint64_t)r * a.S + w];
    }
    a.delta[(uint64_t)r * a.S + w] = gf::sub(nv, ov);
}

// pos(q) of the code, and where the weight of a data block at position d (i << e) for parity block q stands in G
struct Positions {
    uint32_t NC, tshift;     // weight index = ((pos(q) - d) mod NC) >> tshift
    uint32_t qs, qmask, ps;  // pos(q) = off[q >> qs] + ((q & qmask) << ps)
    uint32_t off[8];
    __device__ __forceinline__ uint32_t pos(uint32_t q) const { return off[q >> qs] + ((q & qmask) << ps); }
};

struct ParityArgs {
    uint32_t* parity;       // Mu blocks of S words
    const uint32_t* delta;  // [T][S]
    const uint32_t* G;      // weight table (Montgomery form)
    uint64_t S;
    uint32_t M;             // parity blocks
    uint32_t slices;        // column slices of 64 V words
    uint32_t run;           // parity blocks per wave
    uint32_t waves;
    Positions p;
    uint32_t d[ROWS];       // position of each row's data block (i << e)
};

// Parity blocks through buffer descriptors: the descriptor (base = the block, range = its S words) is scalar and the lane offset is one
// VGPR fixed for the whole loop, so no address register is rewritten between a block's load and the next one.  A lane past the end of
// the row gets an offset outside the range: its loads return 0 and its stores are dropped by the hardware.  aux 2: non-temporal.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t block_desc(const uint32_t* p, uint32_t bytes)
{
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), 0, bytes, 0x00020000);
}
template <int V> __device__ __forceinline__ void load_nt(uint32_t (&dst)[V], __amdgpu_buffer_rsrc_t d, uint32_t voff)
{
    if constexpr (V == 1) {
        dst[0] = __builtin_amdgcn_raw_buffer_load_b32(d, voff, 0, 2);
    } else if constexpr (V == 2) {
        typedef unsigned v2 __attribute__((ext_vector_type(2)));
        const v2 t = __builtin_amdgcn_raw_buffer_load_b64(d, voff, 0, 2);
        dst[0] = t[0], dst[1] = t[1];
    } else {
        typedef unsigned v4 __attribute__((ext_vector_type(4)));
        const v4 t = __builtin_amdgcn_raw_buffer_load_b128(d, voff, 0, 2);
        dst[0] = t[0], dst[1] = t[1], dst[2] = t[2], dst[3] = t[3];
    }
}
template <int V> __device__ __forceinline__ void store_nt(const uint32_t (&src)[V], __amdgpu_buffer_rsrc_t d, uint32_t voff)
{
    if constexpr (V == 1) {
        __builtin_amdgcn_raw_buffer_store_b32(src[0], d, voff, 0, 2);
    } else if constexpr (V == 2) {
        typedef unsigned v2 __attribute__((ext_vector_type(2)));
        __builtin_amdgcn_raw_buffer_store_b64(v2{src[0], src[1]}, d, voff, 0, 2);
    } else {
        typedef unsigned v4 __attribute__((ext_vector_type(4)));
        __builtin_amdgcn_raw_buffer_store_b128(v4{src[0], src[1], src[2], src[3]}, d, voff, 0, 2);
    }
}

// The V words of a block of S words that a lane of column slice `slice` owns (V > 1 only when S % V == 0: a live lane's V words all exist;
// S * 4 < 2^32: update_pass, update_batch_args).  A dead lane — one past the end of the row — reads column 0 and stores nothing.
struct LaneColumns {
    uint64_t lcol;   // the lane's first word for plain loads (a dead lane: 0)
    uint32_t bytes;  // of a block: the range of its descriptor
    uint32_t voff;   // the lane's byte offset in a block for load_nt / store_nt (a dead lane: outside the range)
};
template <int V> __device__ __forceinline__ LaneColumns lane_columns(uint32_t slice, uint32_t lane, uint64_t S)
{
    const uint64_t col = ((uint64_t)slice * 64u + lane) * V;
    const bool live = col < S;
    const uint32_t bytes = (uint32_t)(S * 4u);
    return LaneColumns{live ? col : 0, bytes, live ? (uint32_t)col * 4u : bytes};
}

// The tail of update_batch_kernel and update_set_kernel (update_parity_kernel has the same loop written out): the wave adds
// sum_i weight(row i, q) * x[i] to its column slice of the parity blocks q, next(q + 1), next(next(q + 1) + 1), ... < q1 of the stripe at
// pbase; q < q1 is the first of them.  next(q') is the first block >= q' the wave is to visit
// (the identity where every block is there; it may lie past q1) and row_pos(i) the position of row i's data block, both wave-uniform.
// A block costs T weights from G (T scalar loads behind one wait), T x V mac96 into 96-bit sums, + the old word, one reduction, a non-temporal
// store.  The loop has no branch on the row count or the lane: rows past the count are zero and point at a valid weight, dead lanes only have
// their stores dropped, and past the last block the next load asks for the current block once more (never used).  So the next block's parity
// load stays in flight under the current block's arithmetic (two register sets, the loop unrolled by two: no copy between them).
template <int T, int V, class RowPos, class Next>
__device__ __forceinline__ void stream_parity(const uint32_t (&x)[T][V], const uint32_t* pbase, uint64_t S, const LaneColumns& c, const uint32_t* weights,
                                              const Positions& p, uint32_t q, uint32_t q1, RowPos row_pos, Next next)
{
    const_u32_ptr G = as_constant(weights);
    auto desc = [&](uint32_t qq) { return block_desc(pbase + (uint64_t)qq * S, c.bytes); };
    auto step = [&](uint32_t qq, const uint32_t (&old)[V]) {
        const uint32_t pos = p.pos(qq);
        uint32_t w[T];
#pragma unroll
        for (int i = 0; i < T; ++i) {
            int32_t u = (int32_t)(pos - row_pos(i));
            if (u < 0) u += (int32_t)p.NC;
            w[i] = G[(uint32_t)u >> p.tshift];
        }
        uint64_t lo[V];
        uint32_t hi[V];
#pragma unroll
        for (int v = 0; v < V; ++v) lo[v] = 0, hi[v] = 0;
#pragma unroll
        for (int i = 0; i < T; ++i)
#pragma unroll
            for (int v = 0; v < V; ++v) mac96(lo[v], hi[v], x[i][v], w[i]);
        uint32_t r[V];
#pragma unroll
        for (int v = 0; v < V; ++v) r[v] = gf::add(reduce96(lo[v], hi[v]), old[v]);
        store_nt<V>(r, desc(qq), c.voff);
    };
    uint32_t pa[V], pb[V];
    load_nt<V>(pa, desc(q), c.voff);
    for (;;) {
        uint32_t n = next(q + 1);
        load_nt<V>(pb, desc(n < q1 ? n : q), c.voff);
        step(q, pa);
        if (n >= q1) break;
        q = n;
        n = next(q + 1);
        load_nt<V>(pa, desc(n < q1 ? n : q), c.voff);
        step(q, pb);
        if (n >= q1) break;
        q = n;
    }
}

// Every one of the T delta rows is loaded: rows past the pass's count are zero in d_delta.  This kernel keeps stream_parity's loop written out, in
// the form it had before there was a helper (the next block at a clamped index): through the helper its T = 16, V = 4 instance, which is bound by
// its instruction stream, measured 0.3-0.7 % slower (HISTORY.md).  A change to the weight index, the descriptor or the pipeline goes into both.
template <int T, int V>
__global__ __launch_bounds__(256) void update_parity_kernel(const ParityArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (wave >= a.waves) return;
    const uint32_t slice = wave % a.slices;
    const uint32_t q0 = (wave / a.slices) * a.run, q1 = min(q0 + a.run, a.M);
    const LaneColumns c = lane_columns<V>(slice, lane, a.S);
    uint32_t x[T][V];
#pragma unroll
    for (int i = 0; i < T; ++i) load_vec<V>(x[i], a.delta + (uint64_t)i * a.S + c.lcol);
    const_u32_ptr G = as_constant(a.G);
    auto desc = [&](uint32_t q) { return block_desc(a.parity + (uint64_t)q * a.S, c.bytes); };
    auto step = [&](uint32_t q, const uint32_t (&old)[V]) {
        const uint32_t pos = a.p.pos(q);
        uint32_t w[T];
#pragma unroll
        for (int i = 0; i < T; ++i) {
            int32_t u = (int32_t)(pos - a.d[i]);
            if (u < 0) u += (int32_t)a.p.NC;
            w[i] = G[(uint32_t)u >> a.p.tshift];
        }
        uint64_t lo[V];
        uint32_t hi[V];
#pragma unroll
        for (int v = 0; v < V; ++v) lo[v] = 0, hi[v] = 0;
#pragma unroll
        for (int i = 0; i < T; ++i)
#pragma unroll
            for (int v = 0; v < V; ++v) mac96(lo[v], hi[v], x[i][v], w[i]);
        uint32_t r[V];
#pragma unroll
        for (int v = 0; v < V; ++v) r[v] = gf::add(reduce96(lo[v], hi[v]), old[v]);
        store_nt<V>(r, desc(q), c.voff);
    };
    if (q0 >= q1) return;
    const uint32_t last = q1 - 1;
    uint32_t pa[V], pb[V];
    load_nt<V>(pa, desc(q0), c.voff);
    for (uint32_t q = q0; q < q1; q += 2) {
        load_nt<V>(pb, desc(min(q + 1, last)), c.voff);
        step(q, pa);
        if (q + 1 > last) break;
        load_nt<V>(pa, desc(min(q + 2, last)), c.voff);
        step(q + 1, pb);
    }
}

// ---- a pool of stripes (fastecc_update_batch / _update_parity_batch) ----
// (the formats of the sorted list and of the segment tables: update_list.hpp)
struct BatchArgs {
    uint32_t* parity;            // the pool's parity: stripe b's M blocks at parity + b * M * S
    const uint32_t* data;        // fastecc_update_batch: the pool's data (old rows), stripe b's K blocks at data + b * K * S; else null
    const uint32_t* old_blocks;  // fastecc_update_parity_batch: old rows by row of the caller's list (null: zero)
    const uint32_t* new_blocks;  // new rows by row of the caller's list
    const uint32_t* G;           // weight table (Montgomery form)
    const uint32_t* list;        // the call's sorted writes, LIST_WORDS each
    const uint32_t* segs;        // this launch's segments, SEG_HEAD + T words each
    uint64_t S, K;
    uint32_t M;                  // parity blocks per stripe
    uint32_t slices;             // column slices of 64 V words
    uint32_t run, runs;          // parity blocks per wave, runs per segment
    uint32_t waves;              // segments of the launch x runs x slices
    uint32_t e;                  // data block = position >> e
    Positions p;
};

// update_parity_kernel with the delta rows formed in registers and everything about the stripe read from the segment table and the write list
// (wave-uniform: scalar loads).  Rows past the segment's length are zero and take the weight of row 0; they and dead lanes load from valid
// addresses (row 0 of the segment, column 0), so the T row loads go out together without a branch.  All stripe offsets are 64-bit.
template <int T, int V>
__global__ __launch_bounds__(256) void update_batch_kernel(const BatchArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (wave >= a.waves) return;
    const uint32_t slice = wave % a.slices, rest = wave / a.slices;
    const uint32_t q0 = (rest % a.runs) * a.run, q1 = min(q0 + a.run, a.M);
    const_u32_ptr seg = as_constant(a.segs) + (size_t)(rest / a.runs) * (SEG_HEAD + T);
    const uint32_t len = seg[1];
    const_u32_ptr list = as_constant(a.list) + (size_t)seg[0] * LIST_WORDS;
    const uint64_t stripe = ((uint64_t)list[3] << 32) | list[2];
    const LaneColumns c = lane_columns<V>(slice, lane, a.S);
    // One form of the loop for the three sources of the old rows (no old rows: the new row once more, masked away), and masks instead of
    // conditions: the row loads go out together, with no branch or wait between them.
    const uint32_t omask = (a.data || a.old_blocks) ? 0xFFFFFFFFu : 0u;
    const uint32_t* obase = a.data ? a.data : a.old_blocks ? a.old_blocks : a.new_blocks;
    const uint64_t first_block = a.data ? stripe * a.K : 0;  // old row = block first_block + (data block | list row) of obase
    const uint32_t dmask = a.data ? 0xFFFFFFFFu : 0u;
    uint32_t x[T][V];
    constexpr int H = T * V > 32 ? T / 2 : T;  // rows in flight together (both halves at once would hold 2 T V words beside x)
#pragma unroll
    for (int h = 0; h < T; h += H) {
        uint32_t nv[H][V], ov[H][V];
#pragma unroll
        for (int i = 0; i < H; ++i) {
            const_u32_ptr wr = list + ((uint32_t)(h + i) < len ? h + i : 0) * LIST_WORDS;
            const uint64_t nrow = (uint64_t)wr[1] * a.S;
            const uint64_t orow = (first_block + (((wr[0] >> a.e) & dmask) | (wr[1] & ~dmask))) * a.S;
            load_vec<V>(nv[i], a.new_blocks + nrow + c.lcol);
            load_vec<V>(ov[i], obase + orow + c.lcol);
        }
#pragma unroll
        for (int i = 0; i < H; ++i) {
            const uint32_t imask = (uint32_t)(h + i) < len ? 0xFFFFFFFFu : 0u;
#pragma unroll
            for (int v = 0; v < V; ++v) x[h + i][v] = gf::sub(nv[i][v], ov[i][v] & omask) & imask;
        }
    }
    if (q0 >= q1) return;
    stream_parity<T, V>(x, a.parity + stripe * a.M * a.S, a.S, c, a.G, a.p, q0, q1, [&](int i) { return seg[SEG_HEAD + i]; }, [](uint32_t q) { return q; });
}

// ---- a pool of stripes with absent blocks (fastecc_update_batch_set / _update_parity_batch_set) ----
// (the longer records, SET_LIST_WORDS and SET_SEG_HEAD + T words: update_list.hpp)
struct SetArgs {
    BatchArgs b;               // list and segs in the two formats above
    const uint32_t* old_base;  // what the old rows' offsets count from: the pool's data, else old_blocks, else new_blocks (no old rows: masked away)
    const uint32_t* lost;      // the pattern set's lost parity blocks (drivers.hpp: PatternSetView::lost_parity)
};

// update_batch_kernel for stripes that miss blocks.  The old row of a write comes from the pool or from the reconstruction buffer — the host has put its
// offset into the list, so the kernel chooses nothing and the 2T row loads still go out together — and the wave walks only the PRESENT parity blocks of
// its run: its stripe's lost parity blocks are a sorted list ending in SET_LOST_END, read by scalar loads behind a cursor (q and the cursor are
// wave-uniform: scalar control flow, no lane-divergent branch).  An absent parity block is neither loaded nor stored.  The pipeline is the same: the
// next PRESENT block's load is in flight during the current block's arithmetic.
template <int T, int V>
__global__ __launch_bounds__(256) void update_set_kernel(const SetArgs s)
{
    const BatchArgs& a = s.b;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (wave >= a.waves) return;
    const uint32_t slice = wave % a.slices, rest = wave / a.slices;
    const uint32_t q0 = (rest % a.runs) * a.run, q1 = min(q0 + a.run, a.M);
    const_u32_ptr seg = as_constant(a.segs) + (size_t)(rest / a.runs) * (SET_SEG_HEAD + T);
    const uint32_t len = seg[1];
    const_u32_ptr lost = as_constant(s.lost) + seg[2];
    const_u32_ptr list = as_constant(a.list) + (size_t)seg[0] * SET_LIST_WORDS;
    const uint64_t stripe = ((uint64_t)list[3] << 32) | list[2];
    const LaneColumns c = lane_columns<V>(slice, lane, a.S);
    const uint32_t omask = (a.data || a.old_blocks) ? 0xFFFFFFFFu : 0u;
    const uint32_t* obase = s.old_base + c.lcol;  // (pointer arithmetic, not integers: the loads stay global loads)
    uint32_t x[T][V];
    constexpr int H = T * V > 32 ? T / 2 : T;
#pragma unroll
    for (int h = 0; h < T; h += H) {
        uint32_t nv[H][V], ov[H][V];
#pragma unroll
        for (int i = 0; i < H; ++i) {
            const_u32_ptr wr = list + ((uint32_t)(h + i) < len ? h + i : 0) * SET_LIST_WORDS;
            const uint64_t nrow = (uint64_t)(wr[1] & ~ROW_ABSENT) * a.S;
            const int64_t orow = (int64_t)(((uint64_t)wr[LIST_WORDS + 1] << 32) | wr[LIST_WORDS]);
            load_vec<V>(nv[i], a.new_blocks + nrow + c.lcol);
            load_vec<V>(ov[i], obase + orow);
        }
#pragma unroll
        for (int i = 0; i < H; ++i) {
            const uint32_t imask = (uint32_t)(h + i) < len ? 0xFFFFFFFFu : 0u;
#pragma unroll
            for (int v = 0; v < V; ++v) x[h + i][v] = gf::sub(nv[i][v], ov[i][v] & omask) & imask;
        }
        // (nothing but registers ties the halves together here: unless the first half's differences are pinned where they are formed, the scheduler lifts
        // the second half's loads above the first half's subtractions and the kernel holds 2 T V words beside x after all — 156 VGPRs instead of 104 at
        // T = 16, V = 4)
        if constexpr (H < T) {
#pragma unroll
            for (int i = 0; i < H; ++i)
#pragma unroll
                for (int v = 0; v < V; ++v) asm volatile("" : "+v"(x[h + i][v]));  // (the differences exist here, not where the loop first uses them)
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // the first present parity block at or after q (it may lie past the run: the caller compares with q1); the cursor only moves forward
    uint32_t cur = 0;
    auto present_from = [&](uint32_t q) {
        for (;;) {
            const uint32_t l = lost[cur];
            if (l > q) return q;  // (SET_LOST_END ends every row)
            cur++;
            if (l == q) q++;
        }
    };
    const uint32_t q = present_from(q0);
    if (q >= q1) return;  // an empty run, or every parity block of the run is absent
    stream_parity<T, V>(x, a.parity + stripe * a.M * a.S, a.S, c, a.G, a.p, q, q1, [&](int i) { return seg[SET_SEG_HEAD + i]; }, present_from);
}

// ---- a column window of the pool's blocks (the four fastecc_update_*_window calls) ----
// One kernel for the four calls: the list and the segments in update_set_kernel's formats (a call without a pattern set points every segment at
// UpdateState::d_lost_none, a row that loses nothing).  b.parity is the pool's parity shifted by col0 words, b.S the pool's block (the stride of the
// parity blocks), b.slices the slices of `width` words; an old row's offset from old_base already holds col0 (a pool block) or counts rows of `width`
// words (the reconstruction buffer, old_blocks).
struct WindowArgs {
    SetArgs s;
    uint64_t width;  // words of a row of new_blocks, old_blocks and the reconstruction buffer, and of the window in a pool block
};

// update_set_kernel over the word columns [col0, col0 + width) of every block.  The lane's columns count from the window (a lane past `width` is dead),
// the new rows and the old rows outside the pool sit at pitch `width`, and the parity blocks are addressed through descriptors of width * 4 bytes
// whose bases are S words apart: no word outside the window is loaded or stored.  Rows past the segment's length and dead lanes load from valid
// addresses inside the window (row 0, column 0 of the window) without a branch.  All stripe offsets are 64-bit.
// The kernel's body is update_window_wave, shared with update_window_device_kernel (below), which learns on the device how many of its launch's
// segments exist: admit(wave) says whether the wave has work (update_window_kernel: always).
template <int T, int V, class Admit>
__device__ __forceinline__ void update_window_wave(const WindowArgs& w, Admit admit)
{
    const BatchArgs& a = w.s.b;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (wave >= a.waves) return;
    if (!admit(wave)) return;  // (wave-uniform)
    const uint32_t slice = wave % a.slices, rest = wave / a.slices;
    const uint32_t q0 = (rest % a.runs) * a.run, q1 = min(q0 + a.run, a.M);
    const_u32_ptr seg = as_constant(a.segs) + (size_t)(rest / a.runs) * (SET_SEG_HEAD + T);
    const uint32_t len = seg[1];
    const_u32_ptr lost = as_constant(w.s.lost) + seg[2];
    const_u32_ptr list = as_constant(a.list) + (size_t)seg[0] * SET_LIST_WORDS;
    const uint64_t stripe = ((uint64_t)list[3] << 32) | list[2];
    const LaneColumns c = lane_columns<V>(slice, lane, w.width);
    const uint32_t omask = (a.data || a.old_blocks) ? 0xFFFFFFFFu : 0u;
    const uint32_t* obase = w.s.old_base + c.lcol;
    const uint32_t* nbase = a.new_blocks + c.lcol;
    uint32_t x[T][V];
    constexpr int H = T * V > 32 ? T / 2 : T;
#pragma unroll
    for (int h = 0; h < T; h += H) {
        uint32_t nv[H][V], ov[H][V];
#pragma unroll
        for (int i = 0; i < H; ++i) {
            const_u32_ptr wr = list + ((uint32_t)(h + i) < len ? h + i : 0) * SET_LIST_WORDS;
            const uint64_t nrow = (uint64_t)(wr[1] & ~ROW_ABSENT) * w.width;
            const int64_t orow = (int64_t)(((uint64_t)wr[LIST_WORDS + 1] << 32) | wr[LIST_WORDS]);
            load_vec<V>(nv[i], nbase + nrow);
            load_vec<V>(ov[i], obase + orow);
        }
#pragma unroll
        for (int i = 0; i < H; ++i) {
            const uint32_t imask = (uint32_t)(h + i) < len ? 0xFFFFFFFFu : 0u;
#pragma unroll
            for (int v = 0; v < V; ++v) x[h + i][v] = gf::sub(nv[i][v], ov[i][v] & omask) & imask;
        }
        if constexpr (H < T) {  // (as in update_set_kernel: the first half's differences are formed before the second half's loads go out)
#pragma unroll
            for (int i = 0; i < H; ++i)
#pragma unroll
                for (int v = 0; v < V; ++v) asm volatile("" : "+v"(x[h + i][v]));
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    uint32_t cur = 0;
    auto present_from = [&](uint32_t q) {
        for (;;) {
            const uint32_t l = lost[cur];
            if (l > q) return q;  // (SET_LOST_END ends every row)
            cur++;
            if (l == q) q++;
        }
    };
    const uint32_t q = present_from(q0);
    if (q >= q1) return;
    stream_parity<T, V>(x, a.parity + stripe * a.M * a.S, a.S, c, a.G, a.p, q, q1, [&](int i) { return seg[SET_SEG_HEAD + i]; }, present_from);
}

template <int T, int V>
__global__ __launch_bounds__(256) void update_window_kernel(const WindowArgs w)
{
    update_window_wave<T, V>(w, [](uint32_t) { return true; });
}

struct WindowScatterArgs {
    uint32_t* data;  // the pool's data shifted by col0 words
    const uint32_t* new_blocks;
    const uint32_t* list;  // the launch's first write (SET_LIST_WORDS each)
    uint64_t S, K, width;
    uint32_t slices, waves, e;
};

// update_scatter_kernel for a window: row u of new_blocks (pitch width) into columns [col0, col0 + width) of its present data block
template <int V>
__global__ __launch_bounds__(256) void update_window_scatter_kernel(const WindowScatterArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (wave >= a.waves) return;
    const_u32_ptr wr = as_constant(a.list) + (size_t)(wave / a.slices) * SET_LIST_WORDS;
    if (wr[1] & ROW_ABSENT) return;  // (wave-uniform)
    const uint64_t stripe = ((uint64_t)wr[3] << 32) | wr[2];
    const uint64_t col = ((uint64_t)(wave % a.slices) * 64u + lane) * V;
    if (col >= a.width) return;
    uint32_t t[V];
    load_vec<V>(t, a.new_blocks + (uint64_t)wr[1] * a.width + col);
    store_vec<V>(a.data + (stripe * a.K + (wr[0] >> a.e)) * a.S + col, t);
}

struct ScatterArgs {
    uint32_t* data;
    const uint32_t* new_blocks;
    const uint32_t* list;  // the launch's first write
    uint64_t S, K;
    uint32_t slices, waves, e;
    uint32_t list_words;   // LIST_WORDS, or SET_LIST_WORDS: a write whose data block is absent (ROW_ABSENT) is not stored
};

// wave (write, column slice): row u of new_blocks into data block (stripe, position >> e)
template <int V>
__global__ __launch_bounds__(256) void update_scatter_kernel(const ScatterArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (wave >= a.waves) return;
    const_u32_ptr wr = as_constant(a.list) + (size_t)(wave / a.slices) * a.list_words;
    if (wr[1] & ROW_ABSENT) return;  // (wave-uniform; never set in a list of fastecc_update_batch)
    const uint64_t stripe = ((uint64_t)wr[3] << 32) | wr[2];
    const uint64_t col = ((uint64_t)(wave % a.slices) * 64u + lane) * V;
    if (col >= a.S) return;
    uint32_t t[V];
    load_vec<V>(t, a.new_blocks + (uint64_t)wr[1] * a.S + col);
    store_vec<V>(a.data + (stripe * a.K + (wr[0] >> a.e)) * a.S + col, t);
}

// ---- the write list in device memory (fastecc_update_batch_device / _update_parity_batch_device) ----
// The host never reads the list, so what build_update_list builds on the host — the list's records and the segment tables of update_window_kernel — is
// built by three kernels on the stream, without a sort:
//   device_count_kernel   : lane u takes slot = cnt[stripe]++ of its write (cnt is zeroed by the call); the lane that draws slot 0 gives the stripe its
//                           segment number, from one counter;
//   device_fill_kernel    : lane u writes its record (SET_LIST_WORDS) at seg_of[stripe] * max_per_stripe + slot;
//   device_segments_kernel: lane per segment: its length cnt[stripe], the pairwise duplicate check, and its record (SET_SEG_HEAD + T) in the table of
//                           its length class, at a slot from that class's counter.
// Kernel boundaries order the three and the parity launches behind them; nothing waits inside a kernel.  The counters that many lanes draw from (one
// for the segments, five for the classes) take ONE atomic per workgroup: ballot and mbcnt inside a wave, LDS between the four waves.  A fault of the
// list goes into the caller's status word — the first compare-and-swap from 0 wins — and every later kernel of the call returns when it is non-zero,
// so a refused list writes no word of the pool.  The order of a stripe's records depends on atomic arrival; the parity does not (exact 96-bit sums).
constexpr uint32_t DEVICE_COUNTERS = 8;             // behind cnt[count]: [0] segments, [1 + c] segments of class c (T = 1 << c); zeroed with cnt
constexpr uint32_t DEVICE_ABSENT = 6;               // ... [6] rows of the reconstruction buffer handed out (the set forms)
constexpr uint64_t DEVICE_MAX = 1ull << 24;         // stripes of a pool and entries of a list the device form takes
constexpr uint64_t WRITE_NONE = FASTECC_WRITE_NONE;

struct DeviceListArgs {
    const uint64_t* writes;
    unsigned long long* status;
    uint32_t* cnt;        // [count] writes per stripe, then the DEVICE_COUNTERS
    uint32_t* counters;   // cnt + count
    uint32_t* seg_of;     // [count] the stripe's segment (stripes with a write)
    uint32_t* stripe_of;  // [segments] and back
    uint32_t* slot_of;    // [n] the slot lane u drew (>= mps: no record)
    uint32_t* records;    // [segments][mps] x SET_LIST_WORDS
    uint32_t* tables;     // the five class tables, class c at table_off[c], SET_SEG_HEAD + (1 << c) words a segment
    uint64_t n, limit, K;  // entries of the list; count * K
    uint64_t S, col0, W;
    uint32_t mps, e, with_data, small;  // small: count * K fits 32 bits
    uint32_t table_off[5];
};

__device__ __forceinline__ void device_list_fail(unsigned long long* status, int code, uint64_t u)
{
    atomicCAS(status, 0ull, ((unsigned long long)(uint32_t)code << 32) | (uint32_t)u);
}
__device__ __forceinline__ uint32_t lanes_before(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
__device__ __forceinline__ uint64_t stripe_of_index(const DeviceListArgs& a, uint64_t idx)
{
    return a.small ? (uint64_t)((uint32_t)idx / (uint32_t)a.K) : idx / a.K;
}

// What the set forms (fastecc_update_batch_set_device / _update_parity_batch_set_device) add to DeviceListArgs; NoSet: the plain forms,
// whose kernels are the bodies below with every `if constexpr (SET)` gone.
struct DeviceSetArgs {
    const uint32_t* pattern_of;  // the caller's `count` entries (device); only touched stripes' entries are read, once each, by device_count_set_kernel
    const uint32_t* lost_data;   // PatternSetView::lost_data
    uint32_t* pattern_seg;       // [segments] the stripe's pattern, FASTECC_PATTERN_NONE and a bad entry as `patterns` (the row that loses nothing)
    DirectReadEntry* entries;    // [cap] how to rebuild row r of the reconstruction buffer; device_count_set_kernel fills them with skip entries
    uint32_t* absent;            // the counter the reconstruction rows are drawn from (zeroed with cnt)
    uint64_t recon_offset;       // the reconstruction buffer's offset from old_base, in words (two's complement where it lies below)
    uint32_t patterns, cap;      // P; rows of the reconstruction buffer: min(max_absent, n), 0 for the parity form
};
struct NoSet {};
template <class Set> constexpr bool is_set_form = std::is_same<Set, DeviceSetArgs>::value;

template <class Set>
__device__ __forceinline__ void device_count_body(const DeviceListArgs& a, const Set& s)
{
    constexpr bool SET = is_set_form<Set>;
    __shared__ uint32_t wave_sum[4], block_base;
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    bool first = false;
    uint32_t b = 0;
    if (u < a.n) {
        uint32_t slot = 0xFFFFFFFFu;
        const uint64_t idx = a.writes[u];
        if (idx != WRITE_NONE) {
            if (idx >= a.limit) {
                device_list_fail(a.status, FASTECC_E_INVAL, u);
            } else {
                b = (uint32_t)stripe_of_index(a, idx);
                slot = atomicAdd(&a.cnt[b], 1u);
                if (slot >= a.mps) device_list_fail(a.status, FASTECC_E_UNSUPPORTED, u);
                first = slot == 0;
            }
        }
        a.slot_of[u] = slot;
        if constexpr (SET) {  // (cap <= n) the rebuild launch is sized by cap: a row that device_fill_set_kernel does not hand out is skipped
            if (u < s.cap) s.entries[u] = DirectReadEntry{0, 0, 0, DIRECT_READ_SKIP, 0};
        }
    }
    const uint64_t firsts = __ballot(first);
    if (lane == 0) wave_sum[wave] = (uint32_t)__popcll(firsts);
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t total = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
        block_base = total ? atomicAdd(&a.counters[0], total) : 0u;
    }
    __syncthreads();
    if (!first) return;
    uint32_t seg = block_base + lanes_before(firsts);
    for (uint32_t w = 0; w < wave; ++w) seg += wave_sum[w];
    a.seg_of[b] = seg;  // (seg < min(count, n): one per stripe with a write)
    a.stripe_of[seg] = b;
    if constexpr (SET) {  // the one look at pattern_of[b] (a stripe that no write names: none)
        uint32_t q = s.pattern_of[b];
        if (q == FASTECC_PATTERN_NONE) {
            q = s.patterns;
        } else if (q >= s.patterns) {
            device_list_fail(a.status, FASTECC_E_INVAL, u);
            q = s.patterns;  // (the later build kernels run whatever the status: they find a valid row)
        }
        s.pattern_seg[seg] = q;
    }
}
__global__ __launch_bounds__(256) void device_count_kernel(const DeviceListArgs a) { device_count_body(a, NoSet{}); }
__global__ __launch_bounds__(256) void device_count_set_kernel(const DeviceListArgs a, const DeviceSetArgs s) { device_count_body(a, s); }

// The set form: a write whose data block is absent under its stripe's pattern (the data form only) draws row r of the reconstruction buffer — one atomic
// per workgroup, as the segment counter is drawn — and gets the record of build_update_list's long form: ROW_ABSENT, the old row at r, and
// DirectReadEntry r for the rebuild.  ROW_ABSENT also goes into slot_of[u], where the scatter finds it.  (Every lane of the set form reaches the barriers.)
template <class Set>
__device__ __forceinline__ void device_fill_body(const DeviceListArgs& a, const Set& s)
{
    constexpr bool SET = is_set_form<Set>;
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t slot = 0xFFFFFFFFu;
    if constexpr (SET) {
        if (u < a.n) slot = a.slot_of[u];
    } else {
        if (u >= a.n) return;
        slot = a.slot_of[u];
        if (slot >= a.mps) return;  // FASTECC_WRITE_NONE, an index out of range, or one write too many for its stripe: no record (the status is set)
    }
    const bool record = slot < a.mps;
    const uint64_t idx = !SET || record ? a.writes[u] : 0;
    const uint64_t b = stripe_of_index(a, idx);
    uint64_t off = a.with_data ? idx * a.S + a.col0 : u * a.W;  // the old row from old_base, as build_update_list's long form
    uint32_t row = (uint32_t)u;
    uint32_t seg = 0;
    if constexpr (!SET) seg = a.seg_of[b];
    if constexpr (SET) {
        if (record) seg = a.seg_of[b];
        __shared__ uint32_t wave_sum[4], block_base;
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        const uint32_t i = (uint32_t)(idx - b * a.K);
        uint32_t q = 0, j = 0;
        bool absent = false;
        if (record && a.with_data) {  // (the parity form: only the parity flags matter)
            q = s.pattern_seg[seg];
            if (q < s.patterns) {
                const uint32_t* lost = s.lost_data + (size_t)q * DIRECT_READ_LOST_ROW;  // (the padding matches no block: i < K < 0xFFFFFFF0)
                for (uint32_t t = 0; t < DIRECT_READ_LOST_ROW; ++t)
                    if (lost[t] == i) absent = true, j = t;
            }
        }
        const uint64_t absents = __ballot(absent);
        if (lane == 0) wave_sum[wave] = (uint32_t)__popcll(absents);
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t total = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
            block_base = total ? atomicAdd(s.absent, total) : 0u;
        }
        __syncthreads();
        if (!record) return;
        if (absent) {
            uint32_t r = block_base + lanes_before(absents);
            for (uint32_t w = 0; w < wave; ++w) r += wave_sum[w];
            if (r >= s.cap) {
                device_list_fail(a.status, FASTECC_E_NOMEM, u);  // (no row for it: the record below stays the present block's, and nothing reads it)
            } else {
                s.entries[r] = DirectReadEntry{b, q, i, j, 0};
                off = s.recon_offset + (uint64_t)r * a.W;
                row |= ROW_ABSENT;
                a.slot_of[u] = slot | ROW_ABSENT;
            }
        }
    }
    uint32_t* wr = a.records + ((uint64_t)seg * a.mps + slot) * SET_LIST_WORDS;
    wr[0] = (uint32_t)((idx - b * a.K) << a.e);
    wr[1] = row;
    wr[2] = (uint32_t)b;
    wr[3] = 0;  // (b < DEVICE_MAX)
    wr[LIST_WORDS] = (uint32_t)off;
    wr[LIST_WORDS + 1] = (uint32_t)(off >> 32);
}
__global__ __launch_bounds__(256) void device_fill_kernel(const DeviceListArgs a) { device_fill_body(a, NoSet{}); }
__global__ __launch_bounds__(256) void device_fill_set_kernel(const DeviceListArgs a, const DeviceSetArgs s) { device_fill_body(a, s); }

// The set form: the segment points at its stripe's row of the set's lost parity blocks (PatternSetView::lost_parity; row P loses nothing)
template <class Set>
__device__ __forceinline__ void device_segments_body(const DeviceListArgs& a, const Set& s)
{
    constexpr bool SET = is_set_form<Set>;
    __shared__ uint32_t wave_sum[5][4], block_base[5];
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    bool live = *a.status == 0ull && g < a.counters[0];  // (a list refused by device_count_kernel: nothing to build)
    uint32_t len = 0, cls = 0;
    const uint32_t* rec = a.records + (uint64_t)g * a.mps * SET_LIST_WORDS;
    if (live) {
        len = a.cnt[a.stripe_of[g]];  // (1 .. mps: the status is 0)
        for (uint32_t j = 1; j < len && live; ++j)
            for (uint32_t i = 0; i < j; ++i)
                if (rec[i * SET_LIST_WORDS] == rec[j * SET_LIST_WORDS]) {  // two writes to one block
                    device_list_fail(a.status, FASTECC_E_INVAL, rec[j * SET_LIST_WORDS + 1] & (SET ? ~ROW_ABSENT : 0xFFFFFFFFu));
                    live = false;
                    break;
                }
        while ((1u << cls) < len) cls++;
    }
    uint32_t before = 0;
#pragma unroll
    for (uint32_t c = 0; c < 5; ++c) {
        const uint64_t m = __ballot(live && cls == c);
        if (lane == 0) wave_sum[c][wave] = (uint32_t)__popcll(m);
        if (cls == c) before = lanes_before(m);
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const uint32_t c = threadIdx.x, total = wave_sum[c][0] + wave_sum[c][1] + wave_sum[c][2] + wave_sum[c][3];
        block_base[c] = total ? atomicAdd(&a.counters[1 + c], total) : 0u;
    }
    __syncthreads();
    if (!live) return;
    uint32_t slot = block_base[cls] + before;
    for (uint32_t w = 0; w < wave; ++w) slot += wave_sum[cls][w];
    const uint32_t T = 1u << cls;
    const uint32_t off = cls == 0 ? a.table_off[0] : cls == 1 ? a.table_off[1] : cls == 2 ? a.table_off[2] : cls == 3 ? a.table_off[3] : a.table_off[4];
    uint32_t* seg = a.tables + off + (uint64_t)slot * (SET_SEG_HEAD + T);  // (slot < the class's bound: segments of class T > 1 hold more than T / 2 writes)
    seg[0] = g * a.mps;
    seg[1] = len;
    if constexpr (SET) seg[SEG_HEAD] = s.pattern_seg[g] * (uint32_t)SET_LOST_ROW;
    else seg[SEG_HEAD] = 0;  // the one row of UpdateState::d_lost_none
    for (uint32_t r = 0; r < T; ++r) seg[SET_SEG_HEAD + r] = rec[(r < len ? r : 0) * SET_LIST_WORDS];
}
__global__ __launch_bounds__(256) void device_segments_kernel(const DeviceListArgs a) { device_segments_body(a, NoSet{}); }
__global__ __launch_bounds__(256) void device_segments_set_kernel(const DeviceListArgs a, const DeviceSetArgs s) { device_segments_body(a, s); }

// update_window_kernel for segment tables built on the device: the launch is sized from the host's upper bound on its class's segments, and the wave
// reads the status and the class's real count (scalar loads) before anything else.  seg0: the launch's first segment in the class's table.
template <int T, int V>
__global__ __launch_bounds__(256) void update_window_device_kernel(const WindowArgs w, const uint32_t* status, const uint32_t* built, const uint32_t seg0)
{
    update_window_wave<T, V>(w, [&](uint32_t wave) {
        const_u32_ptr st = as_constant(status);
        if ((st[0] | st[1]) != 0) return false;  // a refused list: all or nothing
        return seg0 + wave / w.s.b.slices / w.s.b.runs < as_constant(built)[0];
    });
}

struct DeviceScatterArgs {
    uint32_t* data;  // the pool's data shifted by col0 words
    const uint32_t* new_blocks;
    const uint32_t* writes;  // the launch's first entry (two words each)
    const uint32_t* status;
    uint64_t S, width;
    uint32_t slices, waves, row0;  // row0: the row of the launch's first entry
};

// update_window_scatter_kernel straight from the caller's list: wave (entry u, column slice)
// present(row): false = the write's data block is absent and nothing is stored (the set form; wave-uniform)
template <int V, class Present>
__device__ __forceinline__ void update_device_scatter_wave(const DeviceScatterArgs& a, Present present)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (wave >= a.waves) return;
    const_u32_ptr st = as_constant(a.status);
    if ((st[0] | st[1]) != 0) return;
    const uint32_t u = wave / a.slices;
    if (!present(a.row0 + u)) return;
    const_u32_ptr wr = as_constant(a.writes) + (size_t)u * 2;
    const uint64_t idx = ((uint64_t)wr[1] << 32) | wr[0];
    if (idx == WRITE_NONE) return;  // (every other entry is < count * K: the status is 0)
    const uint64_t col = ((uint64_t)(wave % a.slices) * 64u + lane) * V;
    if (col >= a.width) return;
    uint32_t t[V];
    load_vec<V>(t, a.new_blocks + (uint64_t)(a.row0 + u) * a.width + col);
    store_vec<V>(a.data + idx * a.S + col, t);
}
template <int V>
__global__ __launch_bounds__(256) void update_device_scatter_kernel(const DeviceScatterArgs a)
{
    update_device_scatter_wave<V>(a, [](uint32_t) { return true; });
}
// ... of the set form: device_fill_set_kernel has put ROW_ABSENT into slot_of[row] of a write whose data block is absent
template <int V>
__global__ __launch_bounds__(256) void update_device_set_scatter_kernel(const DeviceScatterArgs a, const uint32_t* slot_of)
{
    update_device_scatter_wave<V>(a, [&](uint32_t row) { return (as_constant(slot_of)[row] & ROW_ABSENT) == 0; });
}

}  // namespace

struct UpdateState {
    CodeGeom g;
    uint64_t NC = 0;
    uint32_t tshift = 0;
    DeviceBuf<uint32_t> d_G;  // weight table, (NC >> tshift) words
    bool table_ready = false, table_pending = false;
    Event table_event;  // end of the table kernel (on table_stream)
    hipStream_t table_stream = nullptr;
    DeviceBuf<uint32_t> d_delta;  // ROWS x S words (an internal buffer: ordered between streams by buf_event)
    // fastecc_update_batch: one call's sorted write list and segment tables, in words (list.dev is an internal buffer like d_delta)
    StagedList<uint32_t> list;
    // fastecc_update_batch_set: the old rows of one call's absent written blocks, S words each, rebuilt by direct_run_read (an internal buffer)
    DeviceBuf<uint32_t> d_recon;
    // the window calls: such rows at `width` words each; and one row of SET_LOST_ROW words that loses nothing, for the calls without a pattern set
    // (written once, by a synchronous copy at the first window or device-list call of the context: lost_none_row)
    DeviceBuf<uint32_t> d_lost_none;
    // the device-list calls (DeviceListArgs): what the three build kernels write and the parity launches read, grown on demand (internal buffers)
    DeviceBuf<uint32_t> dl_cnt, dl_seg_of, dl_stripe_of, dl_slot_of, dl_records, dl_tables;
    // their set forms (DeviceSetArgs): the pattern of each segment, and the DirectReadEntry of each row of d_recon, ENTRY_WORDS words each
    DeviceBuf<uint32_t> dl_pattern_seg, dl_entries;
};
constexpr uint64_t ENTRY_WORDS = sizeof(DirectReadEntry) / 4;
static_assert(sizeof(DirectReadEntry) % 8 == 0, "entries in a buffer of words: an allocation is aligned for them");

void destroy_update_state(UpdateState* s) { delete s; }

namespace {

// The weight table for stream st: built by a kernel on st at the first call (no host synchronisation); a use on another stream waits
// for that kernel on the device until it is seen complete.
int update_table(fastecc_ctx* c, UpdateState* s, hipStream_t st)
{
    if (s->table_ready) {
        if (s->table_pending && st != s->table_stream) {
            if (hipEventQuery(s->table_event) == hipSuccess) s->table_pending = false;
            else HIP_TRY(hipStreamWaitEvent(st, s->table_event, 0));
            (void)hipGetLastError();  // hipErrorNotReady of the query is not an error
        }
        return FASTECC_OK;
    }
    const uint64_t words = s->NC >> s->tshift;
    RC_TRY(s->d_G.alloc(words));
    RC_TRY(s->table_event.create());
    {
        ProfScope ps(c, st, "update_table", words * 4);
        hipLaunchKernelGGL(update_table_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, s->d_G, (uint32_t)words, gf::h_root((uint32_t)s->NC),
                           (uint32_t)(s->g.N % gf::P), (uint64_t)s->g.N, s->tshift, (uint32_t)((1u << s->g.e) - 1u));
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(s->table_event, st));
    s->table_stream = st;
    s->table_ready = s->table_pending = true;
    return FASTECC_OK;
}

int update_state(fastecc_ctx* c, UpdateState** out)
{
    if (!c->update) {
        UpdateState* s = new (std::nothrow) UpdateState();
        if (!s) return FASTECC_E_NOMEM;
        s->g = geom_of_ctx(c);
        s->NC = s->g.N << s->g.e;
        s->tshift = s->g.e == 1 ? 1u : 0u;
        if (s->NC > 0xFFFFFFFFull / 2) {
            delete s;
            return FASTECC_E_UNSUPPORTED;
        }
        c->update = s;
    }
    *out = c->update;
    return FASTECC_OK;
}

// The instantiated kernels: T rows (the padded length of a pass or segment: 1, 2, 4, 8, ROWS) x V words per lane (4, 2, 1).  launch(T, V) gets
// the pair as constants.
template <int N> using Int = std::integral_constant<int, N>;
template <int T, class Launch>
void with_words(int V, Launch&& launch)
{
    switch (V) {
        case 4: launch(Int<T>(), Int<4>()); break;
        case 2: launch(Int<T>(), Int<2>()); break;
        default: launch(Int<T>(), Int<1>()); break;
    }
}
template <class Launch>
void with_class(int T, int V, Launch&& launch)
{
    switch (T) {
        case 1: with_words<1>(V, launch); break;
        case 2: with_words<2>(V, launch); break;
        case 4: with_words<4>(V, launch); break;
        case 8: with_words<8>(V, launch); break;
        default: with_words<ROWS>(V, launch); break;
    }
}

// Words per lane: the widest V that divides the block's S words and leaves every pointer in `pointers` (ORed) on a V-word boundary —
// everything a lane touches through it, read or written
int lane_words(uint64_t S, uintptr_t pointers)
{
    int V = 4;
    while (V > 1 && ((S % V) != 0 || (pointers & (4u * V - 1u)) != 0)) V >>= 1;
    return V;
}
// ... for the word columns [col0, col0 + width) of such blocks, with rows of `width` words beside them: V also divides col0 and width, so a
// window's first word in a block and every row of `width` words lie on a V-word boundary where the pointers do (V a power of two: one test)
int lane_words(uint64_t S, uint64_t col0, uint64_t width, uintptr_t pointers) { return lane_words(S | col0 | width, pointers); }

// update_parity_kernel, update_batch_kernel, update_set_kernel, update_window_kernel
enum KernelKind { KERNEL_PARITY = 0, KERNEL_BATCH = 1, KERNEL_SET = 2, KERNEL_WINDOW = 3 };

// waves of that kernel<T, V> one SIMD holds: 512 VGPRs in granules of 8, at most 8 (queried once per shape)
int resident_waves_per_simd(KernelKind kind, int T, int V)
{
    static std::atomic<int> cache[4][3][5];  // zero-initialised (static storage)
    int ti = 0;
    while ((1 << ti) < T) ti++;
    std::atomic<int>& slot = cache[kind][V >> 1][ti];  // (V in {1, 2, 4}: entries 0, 1, 2; nothing else indexes the cache)
    if (!slot.load()) {
        hipFuncAttributes attr{};
        const void* fn = nullptr;
        with_class(T, V, [&](auto t_c, auto v_c) {
            constexpr int Tc = t_c, Vc = v_c;
            fn = kind == KERNEL_WINDOW  ? (const void*)update_window_kernel<Tc, Vc>
                 : kind == KERNEL_SET   ? (const void*)update_set_kernel<Tc, Vc>
                 : kind == KERNEL_BATCH ? (const void*)update_batch_kernel<Tc, Vc>
                                        : (const void*)update_parity_kernel<Tc, Vc>;
        });
        int waves = 4;  // (if the query fails: a safe middle)
        if (hipFuncGetAttributes(&attr, fn) == hipSuccess && attr.numRegs > 0) waves = std::max(1, std::min(8, 512 / ((attr.numRegs + 7) / 8 * 8)));
        (void)hipGetLastError();
        slot.store(waves);
    }
    return slot.load();
}

// pos(q) of the code, in the form the parity kernels evaluate it
void set_positions(const UpdateState* s, Positions& p)
{
    const CodeGeom& g = s->g;
    p.NC = (uint32_t)s->NC;
    p.tshift = s->tshift;
    if (g.cosets > 1) {  // N a power of two: coset t = q >> log2 N
        int lgN = 0;
        while ((1ull << lgN) < g.N) lgN++;
        p.qs = (uint32_t)lgN;
        p.qmask = (uint32_t)(g.N - 1);
        p.ps = (uint32_t)g.e;
        for (int t = 0; t < g.cosets && t < 8; t++) p.off[t] = (uint32_t)code_parity_position(g.N, g.e, g.fold, g.cosets, (uint64_t)t * g.N);
    } else {
        p.qs = 31;  // q < 2^31: always entry 0
        p.qmask = 0xFFFFFFFFu;
        p.ps = (uint32_t)g.fold + 1u;
        p.off[0] = 1;
    }
}

// One pass: rows [r0, r0 + rows) of the call
int update_pass(fastecc_ctx* c, UpdateState* s, uint32_t* data, uint32_t* parity, const uint64_t* blocks, uint32_t rows, const uint32_t* old_blocks,
                const uint32_t* new_blocks, hipStream_t st)
{
    const uint64_t S = c->S;
    DeltaArgs da{};
    da.data = data;
    da.old_blocks = old_blocks;
    da.new_blocks = new_blocks;
    da.delta = s->d_delta;
    da.S = S;
    da.rows = rows;
    int T = 1;
    while (T < (int)rows) T <<= 1;
    ParityArgs pa{};
    for (int r = 0; r < T; r++) {  // rows past the count: zero delta rows, any valid weight
        const uint64_t b = blocks[(uint32_t)r < rows ? r : 0];
        if ((uint32_t)r < rows) da.idx[r] = (uint32_t)b;
        pa.d[r] = (uint32_t)(b << s->g.e);
    }
    {
        ProfScope ps(c, st, "update_delta", (uint64_t)rows * S * 4 * (data || old_blocks ? 3 : 2) + (data ? rows * S * 4 : 0));
        hipLaunchKernelGGL(update_delta_kernel, dim3((unsigned)((S + 255) / 256), (unsigned)T), dim3(256), 0, st, da);
        HIP_TRY(hipGetLastError());
    }
    const CodeGeom& g = s->g;
    pa.parity = parity;
    pa.delta = s->d_delta;
    pa.G = s->d_G;
    pa.S = S;
    pa.M = (uint32_t)g.Mu;
    set_positions(s, pa.p);
    if (S * 4 + 64 * 16 > 0xFFFFFFFFull) return FASTECC_E_UNSUPPORTED;  // (blocks of 4 GiB: the kernel addresses a block through one buffer descriptor)
    const int V = lane_words(S, (uintptr_t)parity);  // (the delta rows are the context's own: aligned)
    pa.slices = (uint32_t)((S + 64u * V - 1) / (64u * V));
    // every wave resident at once (the kernel's waves per SIMD from its register count), each with an equal run of parity blocks
    const uint64_t target = (uint64_t)c->cus * 4u * (uint64_t)resident_waves_per_simd(KERNEL_PARITY, T, V);
    const uint64_t runs = std::max<uint64_t>(1, std::min<uint64_t>(g.Mu, target / pa.slices));
    pa.run = (uint32_t)((g.Mu + runs - 1) / runs);
    const uint64_t waves = (uint64_t)pa.slices * ((g.Mu + pa.run - 1) / pa.run);
    if (waves > 0xFFFFFFFFull / 64) return FASTECC_E_UNSUPPORTED;
    pa.waves = (uint32_t)waves;
    const dim3 grid((unsigned)((waves + 3) / 4));
    {
        ProfScope ps(c, st, "update_parity", g.Mu * S * 8);
        with_class(T, V, [&](auto t_c, auto v_c) {
            constexpr int Tc = t_c, Vc = v_c;
            hipLaunchKernelGGL((update_parity_kernel<Tc, Vc>), grid, dim3(256), 0, st, pa);
        });
        HIP_TRY(hipGetLastError());
    }
    return FASTECC_OK;
}

int update_args(fastecc_ctx* c, const void* data, const void* parity, const uint64_t* blocks, uint64_t count, const void* old_blocks, const void* new_blocks,
                int mem_kind, bool with_data)
{
    if (!c) return FASTECC_E_INVAL;
    if (count > 0 && (!parity || !blocks || !new_blocks || (with_data && !data))) return FASTECC_E_INVAL;
    if ((((uintptr_t)data | (uintptr_t)parity | (uintptr_t)old_blocks | (uintptr_t)new_blocks) & 3u) != 0) return FASTECC_E_INVAL;
    if (mem_kind != FASTECC_MEM_HOST && mem_kind != FASTECC_MEM_DEVICE && mem_kind != FASTECC_MEM_HOST_PINNED) return FASTECC_E_INVAL;
    if (c->sharded || c->p61 || c->field != FASTECC_FIELD_GF_FFF00001) return FASTECC_E_UNSUPPORTED;
    if (c->ld != c->S) return FASTECC_E_UNSUPPORTED;
    if (mem_kind != FASTECC_MEM_DEVICE) return FASTECC_E_UNSUPPORTED;
    if (count == 0) return FASTECC_OK;
    std::vector<uint64_t> sorted(blocks, blocks + count);
    std::sort(sorted.begin(), sorted.end());
    if (sorted.back() >= c->K) return FASTECC_E_INVAL;
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return FASTECC_E_INVAL;  // a duplicate index
    return FASTECC_OK;
}

int update_run(fastecc_ctx* c, uint32_t* data, uint32_t* parity, const uint64_t* blocks, uint64_t count, const uint32_t* old_blocks, const uint32_t* new_blocks,
               hipStream_t st)
{
    UpdateState* s = nullptr;
    int rc = update_state(c, &s);
    if (rc != FASTECC_OK) return rc;
    RC_TRY(s->d_delta.alloc((uint64_t)ROWS * c->S));
    rc = update_table(c, s, st);
    if (rc != FASTECC_OK) return rc;
    return with_internal_buffers(c, st, [&]() -> int {
        for (uint64_t r0 = 0; r0 < count; r0 += ROWS) {
            const uint32_t rows = (uint32_t)std::min<uint64_t>(ROWS, count - r0);
            const size_t off = (size_t)r0 * c->S;
            const int r = update_pass(c, s, data, parity, blocks + r0, rows, old_blocks ? old_blocks + off : nullptr, new_blocks + off, st);
            if (r != FASTECC_OK) return r;
        }
        return FASTECC_OK;
    });
}


// ---- a pool of stripes ----
// What can be refused without the write list.  n_writes == 0 is decided by the caller (FASTECC_OK after these checks).
int update_batch_args(fastecc_ctx* c, const void* data, const void* parity, uint64_t count, const uint64_t* writes, uint64_t n_writes, const void* old_blocks,
                      const void* new_blocks, bool with_data)
{
    if (!c || count == 0) return FASTECC_E_INVAL;
    if (n_writes > 0 && (!parity || !writes || !new_blocks || (with_data && !data))) return FASTECC_E_INVAL;
    if ((((uintptr_t)data | (uintptr_t)parity | (uintptr_t)old_blocks | (uintptr_t)new_blocks) & 3u) != 0) return FASTECC_E_INVAL;
    if (c->sharded || c->p61 || c->field != FASTECC_FIELD_GF_FFF00001) return FASTECC_E_UNSUPPORTED;
    if (c->ld != c->S) return FASTECC_E_UNSUPPORTED;  // stripes of a pool are contiguous
    PoolExtent x;
    RC_TRY(pool_extent(c, with_data ? data : nullptr, parity, count, &x));
    const uint64_t block = x.block;
    if (n_writes > UINT64_MAX / block) return FASTECC_E_INVAL;
    if (n_writes > 0xFFFFFFFFull / (LIST_WORDS + SEG_HEAD + 1)) return FASTECC_E_UNSUPPORTED;  // (rows and list offsets are 32-bit: over 700 million writes in one call)
    if (block + 64 * 16 > 0xFFFFFFFFull) return FASTECC_E_UNSUPPORTED;  // (blocks of 4 GiB: the kernel addresses a block through one buffer descriptor)
    return FASTECC_OK;
}

constexpr uint64_t LAUNCH_WAVES = 1ull << 24;  // a dispatch holds fewer than 2^32 work-items per dimension: at most 2^22 workgroups of 4 waves

// What fastecc_update_batch_set / _update_parity_batch_set add to a call (update_batch_set_impl fills it): every array is by write of the SORTED list.
struct SetForm {
    PatternSetView view;
    std::vector<uint32_t> lost_row;        // its stripe's row of view.lost_parity (view.patterns: a whole stripe)
    std::vector<uint32_t> present_parity;  // its stripe's present parity blocks
    std::vector<uint32_t> old_row;         // OLD_IN_POOL, or its row of the reconstruction buffer (its data block is absent)
    uint64_t rebuilt = 0;                  // rows of the reconstruction buffer: the first `rebuilt` entries of c->read_list.host say how to rebuild them
    uint64_t rebuilt_rows_read = 0;        // rows those passes read, and the ones they write
};

// The word columns [col0, col0 + width) of every block that a window call works on (checked against S by the caller); width == 0: the whole block.
struct Window {
    uint64_t col0 = 0, width = 0;
};

// UpdateState::d_lost_none, written once by a synchronous copy at the first call of the context that needs it
int lost_none_row(UpdateState* s)
{
    if (s->d_lost_none) return FASTECC_OK;
    const std::vector<uint32_t> none(SET_LOST_ROW, SET_LOST_END);
    RC_TRY(s->d_lost_none.alloc(none.size()));
    const hipError_t e = hipMemcpy(s->d_lost_none, none.data(), none.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        s->d_lost_none.reset();  // (the next call tries again)
        return hip_fail(e, "hipMemcpy");
    }
    return FASTECC_OK;
}

// ---- the stages the two pool drivers are written out of ----
// How a call's waves cut its rows: V words per lane, `slices` column slices of 64 V words over the W words of a row (the window's width, else the block),
// the window's first column.  FASTECC_E_UNSUPPORTED where one segment's waves do not fit a launch.
struct PoolLanes {
    int V;
    uint64_t slices, W, col0;
};
int pool_lanes(const fastecc_ctx* c, const Window win, uintptr_t pointers, PoolLanes* l)
{
    l->W = win.width ? win.width : c->S;
    l->col0 = win.width ? win.col0 : 0;
    l->V = lane_words(c->S, l->col0, l->W, pointers);  // (the whole block: lane_words(S, pointers))
    l->slices = (l->W + 64u * l->V - 1) / (64u * l->V);
    return l->slices * c->Mu > LAUNCH_WAVES ? FASTECC_E_UNSUPPORTED : FASTECC_OK;
}

// Room for `words` in an internal buffer: replacing it waits, on the host, for the kernels that read it (FASTECC_E_NOMEM: it does not fit)
int grow_behind_wait(fastecc_ctx* c, DeviceBuf<uint32_t>& buf, uint64_t words)
{
    if (words <= buf.capacity()) return FASTECC_OK;
    RC_TRY(wait_idle(c));
    return buf.grow(std::max<uint64_t>(words, 2 * buf.capacity()));
}

// What the old rows' offsets of the long records count from
const uint32_t* old_rows_base(const uint32_t* data, const uint32_t* old_blocks, const uint32_t* new_blocks) { return data ? data : old_blocks ? old_blocks : new_blocks; }

// What every parity launch of a call is told, in the nested form the three kernel families read (update_batch_kernel: wa.s.b, update_set_kernel: wa.s);
// segs, waves, run and runs belong to a launch (split_runs, launch_split).  col0 is folded into the parity pointer.
void pool_kernel_args(const fastecc_ctx* c, const UpdateState* s, const uint32_t* data, uint32_t* parity, const uint32_t* old_blocks, const uint32_t* new_blocks,
                      const PoolLanes& l, const uint32_t* list, const uint32_t* lost, WindowArgs& wa)
{
    BatchArgs& a = wa.s.b;
    a.parity = parity + l.col0;
    a.data = data;
    a.old_blocks = old_blocks;
    a.new_blocks = new_blocks;
    a.G = s->d_G;
    a.list = list;
    a.S = c->S;
    a.K = c->K;
    a.M = (uint32_t)c->Mu;
    a.slices = (uint32_t)l.slices;
    a.e = (uint32_t)s->g.e;
    set_positions(s, a.p);
    wa.s.old_base = old_rows_base(data, old_blocks, new_blocks);
    wa.s.lost = lost;  // (read by update_set_kernel and the window kernels only)
    wa.width = l.W;
}

// a.run and a.runs of a launch of `segs` segments of class T: at least every resident wave of the device, where the parity count allows it, in runs of
// parity blocks per segment.  Returns the waves of one segment.
uint64_t split_runs(const fastecc_ctx* c, KernelKind kind, int T, int V, uint64_t segs, uint64_t slices, uint64_t M, BatchArgs& a)
{
    const uint64_t target = (uint64_t)c->cus * 4u * (uint64_t)resident_waves_per_simd(kind, T, V);
    const uint64_t per_run = segs * slices;
    const uint64_t want = std::max<uint64_t>(1, std::min<uint64_t>(M, (target + per_run - 1) / per_run));
    a.run = (uint32_t)((M + want - 1) / want);
    a.runs = (uint32_t)((M + a.run - 1) / a.run);
    return slices * a.runs;
}

// `items` (segments of a parity launch, writes of a scatter) of item_waves waves each, LAUNCH_WAVES waves at a time: launch_one(first item, waves, grid)
// enqueues one launch.  The one place where a pool write call is cut into launches.
template <class LaunchOne>
int launch_split(uint64_t items, uint64_t item_waves, LaunchOne&& launch_one)
{
    const uint64_t launch_items = LAUNCH_WAVES / item_waves;
    for (uint64_t i0 = 0; i0 < items; i0 += launch_items) {
        const uint64_t waves = std::min<uint64_t>(launch_items, items - i0) * item_waves;
        launch_one(i0, (uint32_t)waves, dim3((unsigned)((waves + 3) / 4)));
        HIP_TRY(hipGetLastError());
    }
    return FASTECC_OK;
}

// The host-list driver: checks, the list and the segment tables (build_update_list, into the pinned side of the staged list), the reconstruction reads,
// the parity launches round by round, the scatter.
// sw: the call's writes, sorted and checked.  data == null: the parity form.  set != null: stripes with absent blocks (update_set_kernel; with data, first
// the old rows of the absent written blocks into the reconstruction buffer, and at the end only present blocks are stored).  A window (win.width != 0):
// update_window_kernel and update_window_scatter_kernel for either form, with the list and the segments in the set form's formats, the caller's rows and
// the reconstruction buffer at pitch W = width, and col0 folded into the parity pointer, the scatter's data pointer and the old rows' pool offsets.
int update_batch_run(fastecc_ctx* c, uint32_t* data, uint32_t* parity, const std::vector<SortedWrite>& sw, const uint32_t* old_blocks, const uint32_t* new_blocks,
                     hipStream_t st, const SetForm* set, const Window win)
{
    UpdateState* s = nullptr;
    RC_TRY(update_state(c, &s));
    const uint64_t S = c->S, K = c->K, M = c->Mu, n = sw.size();
    const bool window = win.width != 0, long_form = set || window;
    const int list_words = long_form ? SET_LIST_WORDS : LIST_WORDS, seg_head = long_form ? SET_SEG_HEAD : SEG_HEAD;
    PoolLanes l;
    RC_TRY(pool_lanes(c, win, (uintptr_t)data | (uintptr_t)parity | (uintptr_t)old_blocks | (uintptr_t)new_blocks, &l));
    if (window && !set) RC_TRY(lost_none_row(s));  // (the whole-block calls never read it)
    RC_TRY(s->list.reserve(n * (list_words + seg_head + 1), [&] { return wait_idle(c); }));  // (build_update_list's bound; growing waits for the kernels that read the list)
    if (set && set->rebuilt) {
        if (direct_read_waves_per_entry(data, parity, nullptr, S, l.col0, l.W) > LAUNCH_WAVES) return FASTECC_E_UNSUPPORTED;
        RC_TRY(grow_behind_wait(c, s->d_recon, set->rebuilt * l.W));  // (rebuilt * W words fit 64 bits: the call's new blocks are more)
    }

    const ListShape shape{K, s->g.e, S, l.W, l.col0, M, data != nullptr, long_form};
    ListSet ls{};
    if (set)  // (the reconstruction buffer and old_base both lie on word boundaries)
        ls = ListSet{set->old_row.data(), set->lost_row.data(), set->present_parity.data(), (uint32_t)SET_LOST_ROW,
                     (uint64_t)(((intptr_t)s->d_recon.get() - (intptr_t)old_rows_base(data, old_blocks, new_blocks)) / 4)};
    std::vector<BatchLaunch> launches;
    const BuiltList built = build_update_list(sw, shape, set ? &ls : nullptr, s->list.host.get(), launches);

    RC_TRY(update_table(c, s, st));
    return with_internal_buffers(c, st, [&]() -> int {
        const size_t words = (size_t)n * list_words + built.seg_words;
        {
            ProfScope ps(c, st, "update_batch_list", words * 4);
            RC_TRY(s->list.publish(words, st));
        }
        if (set && set->rebuilt) {
            // The old rows of the absent written blocks, before ANY parity launch of the call: the passes read parity blocks that those launches
            // rewrite (and present data blocks, which only the scatter at the very end overwrites).
            RC_TRY(c->read_list.publish(set->rebuilt, st));
            ProfScope ps(c, st, window ? "update_window_recon" : "update_set_recon", set->rebuilt_rows_read * l.W * 4);
            RC_TRY(direct_run_read(set->view.passes, c->read_list.dev, set->rebuilt, data, parity, s->d_recon, S, l.col0, l.W, K * S, M * S, st));
        }
        WindowArgs wa{};
        pool_kernel_args(c, s, data, parity, old_blocks, new_blocks, l, s->list.dev, set ? set->view.lost_parity : s->d_lost_none.get(), wa);
        BatchArgs& a = wa.s.b;
        for (const BatchLaunch& bl : launches) {
            const uint64_t seg_waves = split_runs(c, window ? KERNEL_WINDOW : set ? KERNEL_SET : KERNEL_BATCH, bl.T, l.V, bl.segs, l.slices, M, a);
            const uint32_t* table = s->list.dev + n * list_words + bl.seg0;
            ProfScope ps(c, st, window ? "update_window" : set ? "update_set" : "update_batch", bl.parity_blocks * l.W * 8);
            RC_TRY(launch_split(bl.segs, seg_waves, [&](uint64_t s0, uint32_t waves, dim3 grid) {
                a.segs = table + (size_t)s0 * (seg_head + bl.T);
                a.waves = waves;
                with_class(bl.T, l.V, [&](auto t_c, auto v_c) {
                    constexpr int Tc = t_c, Vc = v_c;
                    if (window) hipLaunchKernelGGL((update_window_kernel<Tc, Vc>), grid, dim3(256), 0, st, wa);
                    else if (set) hipLaunchKernelGGL((update_set_kernel<Tc, Vc>), grid, dim3(256), 0, st, wa.s);
                    else hipLaunchKernelGGL((update_batch_kernel<Tc, Vc>), grid, dim3(256), 0, st, a);
                });
            }));
        }
        if (!data || !built.stored) return FASTECC_OK;
        ProfScope ps(c, st, window ? "update_window_scatter" : "update_scatter", built.stored * l.W * 8);
        if (window) {
            WindowScatterArgs ca{data + l.col0, new_blocks, nullptr, S, K, l.W, (uint32_t)l.slices, 0, (uint32_t)s->g.e};
            return launch_split(n, l.slices, [&](uint64_t w0, uint32_t waves, dim3 grid) {
                ca.list = s->list.dev + w0 * list_words;
                ca.waves = waves;
                with_words<1>(l.V, [&](auto, auto v_c) { hipLaunchKernelGGL(update_window_scatter_kernel<decltype(v_c)::value>, grid, dim3(256), 0, st, ca); });
            });
        }
        ScatterArgs ca{data, new_blocks, nullptr, S, K, (uint32_t)l.slices, 0, (uint32_t)s->g.e, (uint32_t)list_words};
        return launch_split(n, l.slices, [&](uint64_t w0, uint32_t waves, dim3 grid) {
            ca.list = s->list.dev + w0 * list_words;
            ca.waves = waves;
            with_words<1>(l.V, [&](auto, auto v_c) { hipLaunchKernelGGL(update_scatter_kernel<decltype(v_c)::value>, grid, dim3(256), 0, st, ca); });
        });
    });
}

// True where the pbytes bytes at p and the qbytes bytes at q share a byte (neither range wraps; a null pointer or an empty range shares nothing)
bool ranges_overlap(const void* p, uint64_t pbytes, const void* q, uint64_t qbytes)
{
    const uint64_t p0 = (uint64_t)(uintptr_t)p, q0 = (uint64_t)(uintptr_t)q;
    return p && q && pbytes && qbytes && p0 < q0 + qbytes && q0 < p0 + pbytes;
}

// True where n_writes rows of row_bytes bytes at `rows` touch the pool (or wrap the address space).  The pool's extent has been checked (pool_extent).
bool rows_overlap_pool(const fastecc_ctx* c, const void* data, const void* parity, uint64_t count, bool with_data, const void* rows, uint64_t n_writes,
                       uint64_t row_bytes)
{
    PoolExtent x;
    (void)pool_extent(c, with_data ? data : nullptr, parity, count, &x, false);
    const uint64_t rows_bytes = n_writes * row_bytes;  // (fits 64 bits: update_batch_args, row_bytes <= x.block)
    if ((uint64_t)(uintptr_t)rows > UINT64_MAX - rows_bytes) return rows && n_writes > 0;
    return (with_data && ranges_overlap(rows, rows_bytes, data, count * x.data_bytes)) || ranges_overlap(rows, rows_bytes, parity, count * x.parity_bytes);
}

// A window call's own refusals, after update_batch_args: the window {col0_words, width_words} against the block, and the caller's rows of width words
// against the pool.  *win is the window to run.
int window_args(const fastecc_ctx* c, const void* data, const void* parity, uint64_t count, uint64_t n_writes, const void* old_blocks, const void* new_blocks,
                bool with_data, const uint64_t* col0_width, Window* win)
{
    const uint64_t col0 = col0_width[0], width = col0_width[1];
    if (width == 0 || col0 > c->S || width > c->S - col0) return FASTECC_E_INVAL;  // (no sum: nothing to overflow)
    if (rows_overlap_pool(c, data, parity, count, with_data, new_blocks, n_writes, width * 4) ||
        rows_overlap_pool(c, data, parity, count, with_data, old_blocks, n_writes, width * 4))
        return FASTECC_E_INVAL;
    *win = Window{col0, width};
    return FASTECC_OK;
}

// col0_width: null (the whole-block forms), or the window {col0_words, width_words} of a window call
int update_batch_impl(fastecc_ctx* c, void* data, void* parity, uint64_t count, const uint64_t* writes, uint64_t n_writes, const void* old_blocks,
                      const void* new_blocks, void* stream, bool with_data, const uint64_t* col0_width = nullptr)
{
    int rc = update_batch_args(c, data, parity, count, writes, n_writes, old_blocks, new_blocks, with_data);
    Window win;
    if (rc == FASTECC_OK && col0_width) rc = window_args(c, data, parity, count, n_writes, old_blocks, new_blocks, with_data, col0_width, &win);
    if (rc != FASTECC_OK || n_writes == 0) return rc;
    std::vector<SortedWrite> sw;
    if (!sort_writes(c->K, count, writes, n_writes, sw)) return FASTECC_E_INVAL;
    DeviceGuard dg(c->device);
    if (!dg.ok) return FASTECC_E_DEVICE;
    CallLock lk(c->mu);
    return update_batch_run(c, with_data ? (uint32_t*)data : nullptr, (uint32_t*)parity, sw, (const uint32_t*)old_blocks, (const uint32_t*)new_blocks,
                            (hipStream_t)stream, nullptr, win);
}

// fastecc_update_batch_set / _update_parity_batch_set: stripe b under pattern pattern_of[b] of the prepared set.  Everything is decided on the host before any
// device work: the checks of update_batch_impl, the rows against the pool, the set, and per touched stripe its pattern — which of its written data blocks are
// absent (their old rows are rebuilt: one DirectReadEntry each, as read_batch_impl's translate makes them) and which parity blocks update_set_kernel skips.
int update_batch_set_impl(fastecc_ctx* c, void* data, void* parity, uint64_t count, const uint32_t* pattern_of, const uint64_t* writes, uint64_t n_writes,
                          const void* old_blocks, const void* new_blocks, void* stream, bool with_data, const uint64_t* col0_width = nullptr)
{
    RC_TRY(update_batch_args(c, data, parity, count, writes, n_writes, old_blocks, new_blocks, with_data));
    if (!pattern_of) return FASTECC_E_INVAL;
    if (n_writes > 0xFFFFFFFFull / (SET_LIST_WORDS + SET_SEG_HEAD + 1)) return FASTECC_E_UNSUPPORTED;  // (the limit of update_batch_args for the longer records)
    Window win;
    if (col0_width) {
        RC_TRY(window_args(c, data, parity, count, n_writes, old_blocks, new_blocks, with_data, col0_width, &win));
    } else if (rows_overlap_pool(c, data, parity, count, with_data, new_blocks, n_writes, c->S * 4) ||
               rows_overlap_pool(c, data, parity, count, with_data, old_blocks, n_writes, c->S * 4)) {
        return FASTECC_E_INVAL;
    }
    CallLock lk(c->mu);
    SetForm set;
    if (!pattern_set_view(c, &set.view)) return FASTECC_E_INVAL;  // fastecc_decode_prepare_set first
    if (n_writes == 0) return FASTECC_OK;
    std::vector<SortedWrite> sw;
    if (!sort_writes(c->K, count, writes, n_writes, sw)) return FASTECC_E_INVAL;
    const uint64_t K = c->K, P = set.view.patterns, n = sw.size();
    set.lost_row.resize(n);
    set.present_parity.resize(n);
    set.old_row.assign(n, OLD_IN_POOL);
    std::vector<DirectReadEntry> rebuild;
    const bool small = count * K <= 0xFFFFFFFFull;  // (count * K fits 64 bits: update_batch_args)
    for (uint64_t f = 0; f < n;) {
        const uint64_t b = small ? (uint64_t)((uint32_t)sw[f].index / (uint32_t)K) : sw[f].index / K;  // (the common case: a 32-bit division, as read_batch_impl)
        const uint32_t q = pattern_of[b];  // (only touched stripes' entries are looked at)
        if (q != FASTECC_PATTERN_NONE && q >= P) return FASTECC_E_INVAL;
        const bool whole = q == FASTECC_PATTERN_NONE;
        const std::vector<uint32_t>* R = whole || !with_data ? nullptr : &pattern_lost_data(c, q);  // (the parity form: only the parity flags matter)
        const uint32_t present = (uint32_t)(c->Mu - (whole ? 0 : pattern_lost_parity(c, q).size()));
        for (; f < n && sw[f].index < (b + 1) * K; f++) {
            set.lost_row[f] = whole ? (uint32_t)P : q;
            set.present_parity[f] = present;
            if (!R) continue;
            const uint32_t i = (uint32_t)(sw[f].index - b * K);
            for (size_t j = 0; j < R->size(); j++)
                if ((*R)[j] == i) {
                    set.old_row[f] = (uint32_t)rebuild.size();
                    rebuild.push_back(DirectReadEntry{b, q, i, (uint32_t)j, 0});
                    set.rebuilt_rows_read += (uint64_t)pattern_rows(c, q) + 1;
                    break;
                }
        }
    }
    DeviceGuard dg(c->device);
    if (!dg.ok) return FASTECC_E_DEVICE;
    if (!rebuild.empty()) {  // (reserve allocates, and waits for the previous call's copy out of the pinned side; it enqueues nothing)
        RC_TRY(c->read_list.reserve(rebuild.size(), [&] { return wait_idle(c); }));
        std::copy(rebuild.begin(), rebuild.end(), c->read_list.host.get());
        set.rebuilt = rebuild.size();
    }
    return update_batch_run(c, with_data ? (uint32_t*)data : nullptr, (uint32_t*)parity, sw, (const uint32_t*)old_blocks, (const uint32_t*)new_blocks,
                            (hipStream_t)stream, &set, win);
}

// ---- the write list in device memory (fastecc_update_batch_device / _update_parity_batch_device) ----
// Everything on `st`, nothing read back: the reset of the per-stripe counters and of *status, the three build kernels, one launch of
// update_window_device_kernel per admitted length class — sized from the host's upper bound on that class's segments: a segment of class T > 1 holds
// more than T / 2 of the list's n entries — and, with a data pool, the scatter after the last of them (section 15: waves of the parity launches
// read the old rows).  The scratch grows on demand behind the host-side wait for the kernels that read it; a steady-state call allocates nothing,
// copies nothing and waits for nothing.
// The stages are update_batch_run's, with the three build kernels where that one calls build_update_list.
// set != null (fastecc_update_batch_set_device / _update_parity_batch_set_device): stripe b under pattern set->pattern_of[b].  The
// build kernels are their set forms; with a data pool the old rows of the absent written blocks are rebuilt into d_recon from entries made on the device,
// after the build (the status is final) and before ANY parity launch (update_batch_run's hazard: the rebuild reads parity that those launches rewrite and
// data that the scatter overwrites); the parity launches skip the stripes' absent parity blocks and the scatter the absent data blocks.  Steps 2 to 5 write
// scratch alone; the parity launches and the scatter write the pool, each wave behind a look at the status.
struct DeviceSetForm {
    PatternSetView view;
    const uint32_t* pattern_of;  // device
    uint64_t max_absent;         // the caller's bound on the absent written data blocks
};
int update_device_run(fastecc_ctx* c, uint32_t* data, uint32_t* parity, uint64_t count, const uint64_t* writes, uint64_t n, uint32_t mps, const Window win,
                      const uint32_t* old_blocks, const uint32_t* new_blocks, uint64_t* status, hipStream_t st, const DeviceSetForm* set = nullptr)
{
    UpdateState* s = nullptr;
    RC_TRY(update_state(c, &s));
    const uint64_t S = c->S, K = c->K, M = c->Mu;
    PoolLanes l;
    RC_TRY(pool_lanes(c, win, (uintptr_t)data | (uintptr_t)parity | (uintptr_t)old_blocks | (uintptr_t)new_blocks, &l));
    if (!set) RC_TRY(lost_none_row(s));  // (the set forms never read it)
    // upper bounds: segments in all (one per touched stripe), and per admitted class
    const uint64_t segs_max = std::min(count, n);
    uint64_t bound[5] = {}, table_words = 0;
    DeviceListArgs la{};
    for (int cl = 0; cl < 5 && (cl == 0 || (1u << (cl - 1)) < mps); cl++) {
        const uint64_t T = 1ull << cl;
        bound[cl] = cl == 0 ? segs_max : std::min(count, n / (T / 2 + 1));
        la.table_off[cl] = (uint32_t)table_words;
        table_words += bound[cl] * (SET_SEG_HEAD + T);  // (n <= DEVICE_MAX: under 14 n words)
    }
    RC_TRY(grow_behind_wait(c, s->dl_cnt, count + DEVICE_COUNTERS));
    RC_TRY(grow_behind_wait(c, s->dl_seg_of, count));
    RC_TRY(grow_behind_wait(c, s->dl_stripe_of, segs_max));
    RC_TRY(grow_behind_wait(c, s->dl_slot_of, n));
    RC_TRY(grow_behind_wait(c, s->dl_records, segs_max * mps * SET_LIST_WORDS));  // (under 2^32 words: DEVICE_MAX x ROWS x SET_LIST_WORDS)
    RC_TRY(grow_behind_wait(c, s->dl_tables, table_words));
    const uint64_t cap = set && data ? std::min(set->max_absent, n) : 0;  // rows of the reconstruction buffer
    if (set) RC_TRY(grow_behind_wait(c, s->dl_pattern_seg, segs_max));
    if (cap) {
        if (direct_read_waves_per_entry(data, parity, nullptr, S, l.col0, l.W) > LAUNCH_WAVES) return FASTECC_E_UNSUPPORTED;
        RC_TRY(grow_behind_wait(c, s->d_recon, cap * l.W));  // (cap <= DEVICE_MAX and W < 2^30: no wrap)
        RC_TRY(grow_behind_wait(c, s->dl_entries, cap * ENTRY_WORDS));
    }
    RC_TRY(update_table(c, s, st));
    return with_internal_buffers(c, st, [&]() -> int {
        DeviceSetArgs sa{};
        if (set) {
            sa.pattern_of = set->pattern_of;
            sa.lost_data = set->view.lost_data;
            sa.pattern_seg = s->dl_pattern_seg;
            sa.entries = (DirectReadEntry*)s->dl_entries.get();
            sa.absent = s->dl_cnt + count + DEVICE_ABSENT;
            sa.recon_offset = cap ? (uint64_t)(((intptr_t)s->d_recon.get() - (intptr_t)data) / 4) : 0;  // (both on word boundaries)
            sa.patterns = (uint32_t)set->view.patterns;
            sa.cap = (uint32_t)cap;
        }
        la.writes = writes;
        la.status = (unsigned long long*)status;
        la.cnt = s->dl_cnt;
        la.counters = s->dl_cnt + count;
        la.seg_of = s->dl_seg_of;
        la.stripe_of = s->dl_stripe_of;
        la.slot_of = s->dl_slot_of;
        la.records = s->dl_records;
        la.tables = s->dl_tables;
        la.n = n;
        la.limit = count * K;  // (fits: update_batch_args)
        la.K = K;
        la.S = S;
        la.col0 = l.col0;
        la.W = l.W;
        la.mps = mps;
        la.e = (uint32_t)s->g.e;
        la.with_data = data ? 1u : 0u;
        la.small = la.limit <= 0xFFFFFFFFull ? 1u : 0u;
        {
            ProfScope ps(c, st, set ? "update_set_device_build" : "update_device_build", (count + DEVICE_COUNTERS) * 4 + n * (8 + 8 + SET_LIST_WORDS * 4));
            HIP_TRY(hipMemsetAsync(s->dl_cnt, 0, (count + DEVICE_COUNTERS) * 4, st));
            HIP_TRY(hipMemsetAsync(status, 0, 8, st));
            const dim3 per_entry((unsigned)((n + 255) / 256)), per_segment((unsigned)((segs_max + 255) / 256));
            if (set) {
                hipLaunchKernelGGL(device_count_set_kernel, per_entry, dim3(256), 0, st, la, sa);
                hipLaunchKernelGGL(device_fill_set_kernel, per_entry, dim3(256), 0, st, la, sa);
                hipLaunchKernelGGL(device_segments_set_kernel, per_segment, dim3(256), 0, st, la, sa);
            } else {
                hipLaunchKernelGGL(device_count_kernel, per_entry, dim3(256), 0, st, la);
                hipLaunchKernelGGL(device_fill_kernel, per_entry, dim3(256), 0, st, la);
                hipLaunchKernelGGL(device_segments_kernel, per_segment, dim3(256), 0, st, la);
            }
            HIP_TRY(hipGetLastError());
        }
        if (cap) {  // (the bytes: a bound, every row taken and rebuilt from K rows — how many are absent is known on the device only)
            ProfScope ps(c, st, "update_set_device_recon", cap * (K + 1) * l.W * 4);
            RC_TRY(direct_run_read_device(set->view.passes, sa.entries, cap, data, parity, s->d_recon, S, l.col0, l.W, K * S, M * S, status, st));
        }
        WindowArgs wa{};
        pool_kernel_args(c, s, data, parity, old_blocks, new_blocks, l, s->dl_records, set ? set->view.lost_parity : s->d_lost_none.get(), wa);
        BatchArgs& a = wa.s.b;
        {
            ProfScope ps(c, st, set ? "update_set_device" : "update_device", n * M * l.W * 8);  // (every entry a write, every parity block present)
            for (int cl = 0; cl < 5; cl++) {
                if (!bound[cl]) continue;
                const int T = 1 << cl;
                const uint64_t seg_waves = split_runs(c, KERNEL_WINDOW, T, l.V, bound[cl], l.slices, M, a);
                RC_TRY(launch_split(bound[cl], seg_waves, [&](uint64_t s0, uint32_t waves, dim3 grid) {
                    a.segs = s->dl_tables + la.table_off[cl] + (size_t)s0 * (SET_SEG_HEAD + T);
                    a.waves = waves;
                    with_class(T, l.V, [&](auto t_c, auto v_c) {
                        constexpr int Tc = t_c, Vc = v_c;
                        hipLaunchKernelGGL((update_window_device_kernel<Tc, Vc>), grid, dim3(256), 0, st, wa, (const uint32_t*)status,
                                           (const uint32_t*)(la.counters + 1 + cl), (uint32_t)s0);
                    });
                }));
            }
        }
        if (!data) return FASTECC_OK;
        DeviceScatterArgs ca{data + l.col0, new_blocks, nullptr, (const uint32_t*)status, S, l.W, (uint32_t)l.slices, 0, 0};
        ProfScope ps(c, st, set ? "update_set_device_scatter" : "update_device_scatter", n * l.W * 8);
        return launch_split(n, l.slices, [&](uint64_t w0, uint32_t waves, dim3 grid) {
            ca.writes = (const uint32_t*)(writes + w0);
            ca.row0 = (uint32_t)w0;
            ca.waves = waves;
            with_words<1>(l.V, [&](auto, auto v_c) {
                constexpr int Vc = decltype(v_c)::value;
                if (set) hipLaunchKernelGGL(update_device_set_scatter_kernel<Vc>, grid, dim3(256), 0, st, ca, (const uint32_t*)s->dl_slot_of.get());
                else hipLaunchKernelGGL(update_device_scatter_kernel<Vc>, grid, dim3(256), 0, st, ca);
            });
        });
    });
}

// What the host can decide without the list; then update_device_run.  col0_width: the window {col0_words, width_words}.
// set_args != null: the set forms, {pattern_of, max_absent} — pattern_of against the pool as well, and the prepared set (none: FASTECC_E_INVAL, as
// fastecc_update_batch_set says it, and before an empty list is accepted).
struct DeviceSetCall {
    const uint32_t* pattern_of;
    uint64_t max_absent;
};
int update_batch_device_impl(fastecc_ctx* c, void* data, void* parity, uint64_t count, const uint64_t* writes, uint64_t n_writes, uint32_t max_per_stripe,
                             const uint64_t* col0_width, const void* old_blocks, const void* new_blocks, uint64_t* status, void* stream, bool with_data,
                             const DeviceSetCall* set_args = nullptr)
{
    RC_TRY(update_batch_args(c, data, parity, count, writes, n_writes, old_blocks, new_blocks, with_data));
    if (!status || max_per_stripe < 1 || max_per_stripe > (uint32_t)ROWS) return FASTECC_E_INVAL;
    if ((((uintptr_t)writes | (uintptr_t)status) & 7u) != 0) return FASTECC_E_INVAL;
    if (count > DEVICE_MAX || n_writes > DEVICE_MAX) return FASTECC_E_UNSUPPORTED;  // (the counters reset by every call: 4 bytes per stripe)
    Window win;
    RC_TRY(window_args(c, data, parity, count, n_writes, old_blocks, new_blocks, with_data, col0_width, &win));
    // the list and the status word against the pool, the rows and each other (n_writes <= DEVICE_MAX: no product wraps)
    const uint64_t rows_bytes = n_writes * win.width * 4;  // (fits: window_args has walked them)
    if (rows_overlap_pool(c, data, parity, count, with_data, writes, n_writes, 8) || rows_overlap_pool(c, data, parity, count, with_data, status, 1, 8) ||
        ranges_overlap(writes, n_writes * 8, new_blocks, rows_bytes) || ranges_overlap(writes, n_writes * 8, old_blocks, rows_bytes) ||
        ranges_overlap(status, 8, new_blocks, rows_bytes) || ranges_overlap(status, 8, old_blocks, rows_bytes) || ranges_overlap(status, 8, writes, n_writes * 8))
        return FASTECC_E_INVAL;
    if (set_args && rows_overlap_pool(c, data, parity, count, with_data, set_args->pattern_of, count, 4)) return FASTECC_E_INVAL;
    DeviceGuard dg(c->device);
    if (!dg.ok) return FASTECC_E_DEVICE;
    CallLock lk(c->mu);
    DeviceSetForm set{};
    if (set_args) {
        if (!pattern_set_view(c, &set.view)) return FASTECC_E_INVAL;  // fastecc_decode_prepare_set first
        set.pattern_of = set_args->pattern_of;
        set.max_absent = set_args->max_absent;
    }
    if (n_writes == 0) {
        HIP_TRY(hipMemsetAsync(status, 0, 8, (hipStream_t)stream));
        return FASTECC_OK;
    }
    return update_device_run(c, with_data ? (uint32_t*)data : nullptr, (uint32_t*)parity, count, writes, n_writes, max_per_stripe, win,
                             (const uint32_t*)old_blocks, (const uint32_t*)new_blocks, status, (hipStream_t)stream, set_args ? &set : nullptr);
}

// The set forms: first what can be refused without reading the context — the pointers, the promise, the bounds of 2^24 and pattern_of against the
// list, the status word and the rows — then everything update_batch_device_impl refuses.
int update_batch_set_device_impl(fastecc_ctx* c, void* data, void* parity, uint64_t count, const uint32_t* pattern_of, const uint64_t* writes, uint64_t n_writes,
                                 uint32_t max_per_stripe, uint64_t max_absent, const uint64_t* col0_width, const void* old_blocks, const void* new_blocks,
                                 uint64_t* status, void* stream, bool with_data)
{
    if (!c || count == 0 || !pattern_of || !status) return FASTECC_E_INVAL;
    if (n_writes > 0 && (!parity || !writes || !new_blocks || (with_data && !data))) return FASTECC_E_INVAL;
    if (((uintptr_t)pattern_of & 3u) != 0 || (((uintptr_t)writes | (uintptr_t)status) & 7u) != 0) return FASTECC_E_INVAL;
    if ((((uintptr_t)data | (uintptr_t)parity | (uintptr_t)old_blocks | (uintptr_t)new_blocks) & 3u) != 0) return FASTECC_E_INVAL;
    if (max_per_stripe < 1 || max_per_stripe > (uint32_t)ROWS || col0_width[1] == 0) return FASTECC_E_INVAL;
    if (count > DEVICE_MAX || n_writes > DEVICE_MAX) return FASTECC_E_UNSUPPORTED;
    // (no product wraps: count and n_writes <= 2^24; a width that no block of under 4 GiB holds is refused with the window)
    const uint64_t rows_bytes = col0_width[1] < (1ull << 30) ? n_writes * col0_width[1] * 4 : 0, pattern_bytes = count * 4, writes_bytes = n_writes * 8;
    if (ranges_overlap(pattern_of, pattern_bytes, writes, writes_bytes) || ranges_overlap(pattern_of, pattern_bytes, status, 8) ||
        ranges_overlap(pattern_of, pattern_bytes, new_blocks, rows_bytes) || ranges_overlap(pattern_of, pattern_bytes, old_blocks, rows_bytes) ||
        ranges_overlap(status, 8, writes, writes_bytes) || ranges_overlap(writes, writes_bytes, new_blocks, rows_bytes) ||
        ranges_overlap(writes, writes_bytes, old_blocks, rows_bytes) || ranges_overlap(status, 8, new_blocks, rows_bytes) ||
        ranges_overlap(status, 8, old_blocks, rows_bytes))
        return FASTECC_E_INVAL;
    const DeviceSetCall set_args{pattern_of, max_absent};
    return update_batch_device_impl(c, data, parity, count, writes, n_writes, max_per_stripe, col0_width, old_blocks, new_blocks, status, stream, with_data,
                                    &set_args);
}

}  // namespace

}  // namespace fastecc

using namespace fastecc;

extern "C" {

int fastecc_update(fastecc_ctx* c, void* data, void* parity, const uint64_t* blocks, uint64_t count, const void* new_blocks, int mem_kind, void* stream)
{
    return guarded([&]() -> int {
        int rc = update_args(c, data, parity, blocks, count, nullptr, new_blocks, mem_kind, true);
        if (rc != FASTECC_OK || count == 0) return rc;
        DeviceGuard dg(c->device);
        if (!dg.ok) return FASTECC_E_DEVICE;
        CallLock lk(c->mu);
        return update_run(c, (uint32_t*)data, (uint32_t*)parity, blocks, count, nullptr, (const uint32_t*)new_blocks, (hipStream_t)stream);
    });
}

int fastecc_update_parity(fastecc_ctx* c, void* parity, const uint64_t* blocks, uint64_t count, const void* old_blocks, const void* new_blocks, int mem_kind,
                          void* stream)
{
    return guarded([&]() -> int {
        int rc = update_args(c, nullptr, parity, blocks, count, old_blocks, new_blocks, mem_kind, false);
        if (rc != FASTECC_OK || count == 0) return rc;
        DeviceGuard dg(c->device);
        if (!dg.ok) return FASTECC_E_DEVICE;
        CallLock lk(c->mu);
        return update_run(c, nullptr, (uint32_t*)parity, blocks, count, (const uint32_t*)old_blocks, (const uint32_t*)new_blocks, (hipStream_t)stream);
    });
}

int fastecc_update_batch(fastecc_ctx* c, void* data, void* parity, uint64_t count, const uint64_t* writes, uint64_t n_writes, const void* new_blocks, void* stream)
{
    return guarded([&]() -> int { return update_batch_impl(c, data, parity, count, writes, n_writes, nullptr, new_blocks, stream, true); });
}

int fastecc_update_parity_batch(fastecc_ctx* c, void* parity, uint64_t count, const uint64_t* writes, uint64_t n_writes, const void* old_blocks,
                                const void* new_blocks, void* stream)
{
    return guarded([&]() -> int { return update_batch_impl(c, nullptr, parity, count, writes, n_writes, old_blocks, new_blocks, stream, false); });
}

int fastecc_update_batch_set(fastecc_ctx* c, void* data, void* parity, uint64_t count, const uint32_t* pattern_of, const uint64_t* writes, uint64_t n_writes,
                             const void* new_blocks, void* stream)
{
    return guarded([&]() -> int { return update_batch_set_impl(c, data, parity, count, pattern_of, writes, n_writes, nullptr, new_blocks, stream, true); });
}

int fastecc_update_parity_batch_set(fastecc_ctx* c, void* parity, uint64_t count, const uint32_t* pattern_of, const uint64_t* writes, uint64_t n_writes,
                                    const void* old_blocks, const void* new_blocks, void* stream)
{
    return guarded([&]() -> int { return update_batch_set_impl(c, nullptr, parity, count, pattern_of, writes, n_writes, old_blocks, new_blocks, stream, false); });
}

int fastecc_update_batch_window(fastecc_ctx* c, void* data, void* parity, uint64_t count, const uint64_t* writes, uint64_t n_writes, uint64_t col0_words,
                                uint64_t width_words, const void* new_blocks, void* stream)
{
    const uint64_t win[2] = {col0_words, width_words};
    return guarded([&]() -> int { return update_batch_impl(c, data, parity, count, writes, n_writes, nullptr, new_blocks, stream, true, win); });
}

int fastecc_update_parity_batch_window(fastecc_ctx* c, void* parity, uint64_t count, const uint64_t* writes, uint64_t n_writes, uint64_t col0_words,
                                       uint64_t width_words, const void* old_blocks, const void* new_blocks, void* stream)
{
    const uint64_t win[2] = {col0_words, width_words};
    return guarded([&]() -> int { return update_batch_impl(c, nullptr, parity, count, writes, n_writes, old_blocks, new_blocks, stream, false, win); });
}

int fastecc_update_batch_set_window(fastecc_ctx* c, void* data, void* parity, uint64_t count, const uint32_t* pattern_of, const uint64_t* writes,
                                    uint64_t n_writes, uint64_t col0_words, uint64_t width_words, const void* new_blocks, void* stream)
{
    const uint64_t win[2] = {col0_words, width_words};
    return guarded([&]() -> int { return update_batch_set_impl(c, data, parity, count, pattern_of, writes, n_writes, nullptr, new_blocks, stream, true, win); });
}

int fastecc_update_parity_batch_set_window(fastecc_ctx* c, void* parity, uint64_t count, const uint32_t* pattern_of, const uint64_t* writes, uint64_t n_writes,
                                           uint64_t col0_words, uint64_t width_words, const void* old_blocks, const void* new_blocks, void* stream)
{
    const uint64_t win[2] = {col0_words, width_words};
    return guarded(
        [&]() -> int { return update_batch_set_impl(c, nullptr, parity, count, pattern_of, writes, n_writes, old_blocks, new_blocks, stream, false, win); });
}

int fastecc_update_batch_device(fastecc_ctx* c, void* data, void* parity, uint64_t count, const uint64_t* writes, uint64_t n_writes, uint32_t max_per_stripe,
                                uint64_t col0_words, uint64_t width_words, const void* new_blocks, uint64_t* status, void* stream)
{
    const uint64_t win[2] = {col0_words, width_words};
    return guarded([&]() -> int {
        return update_batch_device_impl(c, data, parity, count, writes, n_writes, max_per_stripe, win, nullptr, new_blocks, status, stream, true);
    });
}

int fastecc_update_parity_batch_device(fastecc_ctx* c, void* parity, uint64_t count, const uint64_t* writes, uint64_t n_writes, uint32_t max_per_stripe,
                                       uint64_t col0_words, uint64_t width_words, const void* old_blocks, const void* new_blocks, uint64_t* status,
                                       void* stream)
{
    const uint64_t win[2] = {col0_words, width_words};
    return guarded([&]() -> int {
        return update_batch_device_impl(c, nullptr, parity, count, writes, n_writes, max_per_stripe, win, old_blocks, new_blocks, status, stream, false);
    });
}

int fastecc_update_batch_set_device(fastecc_ctx* c, void* data, void* parity, uint64_t count, const uint32_t* pattern_of, const uint64_t* writes, uint64_t n_writes,
                                    uint32_t max_per_stripe, uint64_t max_absent, uint64_t col0_words, uint64_t width_words, const void* new_blocks,
                                    uint64_t* status, void* stream)
{
    const uint64_t win[2] = {col0_words, width_words};
    return guarded([&]() -> int {
        return update_batch_set_device_impl(c, data, parity, count, pattern_of, writes, n_writes, max_per_stripe, max_absent, win, nullptr, new_blocks, status,
                                            stream, true);
    });
}

int fastecc_update_parity_batch_set_device(fastecc_ctx* c, void* parity, uint64_t count, const uint32_t* pattern_of, const uint64_t* writes, uint64_t n_writes,
                                           uint32_t max_per_stripe, uint64_t col0_words, uint64_t width_words, const void* old_blocks, const void* new_blocks,
                                           uint64_t* status, void* stream)
{
    const uint64_t win[2] = {col0_words, width_words};
    return guarded([&]() -> int {
        return update_batch_set_device_impl(c, nullptr, parity, count, pattern_of, writes, n_writes, max_per_stripe, 0, win, old_blocks, new_blocks, status,
                                            stream, false);
    });
}

int fastecc_code_coefficient(uint64_t n, uint64_t k, unsigned flags, uint64_t data_block, uint64_t parity_block, uint32_t* out)
{
    if (!out) return FASTECC_E_INVAL;
    CodeGeom g;
    const int rc = geom_of_code(n, k, flags, &g);
    if (rc != FASTECC_OK) return rc;
    if (data_block >= g.K || parity_block >= g.Mu) return FASTECC_E_INVAL;
    *out = geom_weight(g, data_block, parity_block);
    return FASTECC_OK;
}

}  // extern "C"
