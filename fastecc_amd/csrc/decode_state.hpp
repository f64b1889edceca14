// decode_state.hpp — what the three files of the GF(0xFFF00001) erasure decoder share: decode_prepare.hip (a pattern's tables), decode.hip (a stripe or
// a batch under it) and pattern_set.hip (a pattern per stripe, degraded reads).  Private to those three: everyone else sees DecodeState and PatternSet
// as the forward declarations of internal.hpp.  The algorithm is described at the head of decode.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <initializer_list>
#include <new>
#include <vector>

#include "drivers.hpp"

namespace fastecc {

// The direct path's tables of one erasure pattern (direct_tables): which passes it takes and their weights
struct PatternTables {
    DirectPassPtr data;    // the lost data blocks (only data lost, or more than 32 blocks lost in all)
    DirectPassPtr parity;  // the lost parity blocks from the complete data (only parity lost, or more than 32 in all)
    DirectPassPtr both;    // data AND parity lost, at most 32 in all: the single pass
    bool both_built = false;       // `both` holds this pattern
    bool only_both = false;        // ... and is its only pass (few outputs: the pass is bound by the read of the survivors, fastecc_decode runs it too and drops the parity outputs)
    int ed = 0, ep = 0;    // lost data / parity blocks
    bool host_nomem = false;       // direct_tables' FASTECC_E_NOMEM is the host's (no DirectPass object), not the device's (no room for a table)
};

// ---- the parts of DecodeState, by owner.  Each says when it is built and what invalidates it. ----

// The prepared pattern as the calls see it.  Written by every fastecc_decode_prepare (Prepare::new_pattern, direct, set_pattern) under the call lock;
// `ready` is false from the moment a new pattern starts to overwrite anything until all of it stands.
struct DecodePattern {
    bool ready = false;
    uint64_t erased_data = 0, erased_parity = 0;  // lost blocks
    uint64_t positions = 0;      // code length on the roots of unity: k << log2(n / k) rounded up to powers of two
    bool standard = false;       // the reference's (2k,k) layout: position u = data u/2 or parity u/2, every block in memory
    bool mixed = false;          // mixed-radix code: `recovered` is the whole work stripe (all positions), transformed in place
    uint64_t serial = 0;         // counts the patterns: what HostStaging's lists and FewLosses' read descriptor are valid for
    bool direct_path = false;    // few losses: FewLosses::direct serves this pattern; else the transform path's tables do
    int direct_kernel = 0;       // 0 choose, 1 VALU, 2 MFMA (option "direct_kernel"), as it stood at the prepare
};

// Few losses (any layout: the reference's, zero extension, sub-/extra cosets, mixed radix): every lost data block is a fixed linear combination of the
// surviving data blocks and as many surviving parity blocks (interpolation on N nodes); for repair the lost parity blocks follow from the complete
// data (direct.hip).  `direct` is built over by every prepare that tries the direct path (its pass objects are kept and refilled), also by one that
// then falls through to the transform path: it describes the pattern only while DecodePattern::direct_path is set.
struct FewLosses {
    PatternTables direct;
    DeviceBuf<DirectSetPass> read_desc;  // fastecc_read_batch: the descriptor of the pass that rebuilds the lost data, valid for pattern `read_desc_of` (lazy)
    uint64_t read_desc_of = ~0ull;
    DeviceBuf<uint32_t> read_lost;       // fastecc_read_batch_device: HostStaging::lost_data (increasing, at most 256) of pattern `read_lost_of` (lazy)
    uint64_t read_lost_of = ~0ull;
};

// The transform path's contexts and per-position tables.  The contexts, `recovered`, the tile order and the table buffers are built once per context by
// the first pattern that needs them (Prepare::build_shape) and kept; the contents of fin, fin_tiled, srcmap, gout, gout_par, parity_lost, dev_state,
// dev_present and dev_counts are this pattern's, rewritten by every prepare of the transform path.  recovered_full and parity_again are made by the
// first repair that needs them.
struct TransformTables {
    CtxPtr transform;                       // size-2k transform context, fold 1
    CtxPtr pattern_ntt;                     // same length, 2 words per block: l and l' are evaluated on the device
    DeviceBuf<uint32_t> pattern_buf;        // its stripe
    bool pattern_narrow = false;            // pattern_ntt holds the upper row bits of a few-column transform (chunk_transform_kernel): 2 NC / CHUNK rows
    DeviceBuf<uint32_t> fin;                // 2k factors by codeword position: l(w^u) (Montgomery) or 0 if erased
    uint32_t* fin_first_pass = nullptr;     // the same in the order the transform's first pass reads them: a view of fin, or of fin_tiled
    DeviceBuf<uint32_t> fin_tiled;          // ... where that order is not the order of the positions (permuted from fin for every pattern)
    DeviceBuf<uint32_t> tile_order;         // NC words: first-pass order of the factors (only for the (2k,k) layout)
    bool tile_order_valid = false;
    DeviceBuf<uint32_t> srcmap;             // per codeword position: the block that sits there (row, bit 31 = parity stripe)
    DeviceBuf<uint32_t> gout;               // k factors by data block: 1 / (w^2i l'(w^2i)) (Montgomery) if erased, else 0
    DeviceBuf<uint32_t> gout_par;           // k factors by parity block: 1 / (w^(2q+1) l'(w^(2q+1))) (Montgomery) if erased, else 0
    DeviceBuf<uint32_t> recovered;          // k blocks: x p'(x) at the data positions
    // fastecc_repair of the (2k,k) layout in ONE transform: the same x p'(x) evaluated at ALL 2k positions (fold 0) gives the lost parity
    // blocks as well, f(w^u) = (x p')(w^u) / (w^u l'(w^u)) at odd u — instead of decoding the data and encoding it once more
    CtxPtr transform_full;
    DeviceBuf<uint32_t> recovered_full;     // 2k blocks: x p'(x) at every position (lazy: 4 GiB at the headline size)
    bool full_ok = false;                   // transform_full's first pass reads the factors in the same order as transform's
    // fastecc_repair: which parity blocks are lost (one word each), and the stripe the re-encode writes to
    DeviceBuf<uint32_t> parity_lost;
    DeviceBuf<uint32_t> parity_again;
    DeviceBuf<uint8_t> dev_state;           // NC bytes: LOST / HELD / ZERO per position
    DeviceBuf<uint8_t> dev_present;         // (2k,k) layout: the caller's two presence arrays, k bytes each (the pattern is scanned on the device)
    DeviceBuf<uint32_t> dev_counts;         // ... and what presence_counts_kernel counts in them (8 words)
};

// fastecc_decode_prepare's device state: the product tree of the locator.  wpow is filled once per context (Prepare::build_tables) and serves the split
// transform's tables too; everything else is rebuilt when the padded root count or the leaf size changes (Prepare::build_tree) and is scratch between
// prepares: no decode reads it.
struct LocatorTree {
    uint64_t T = 0;                         // padded number of roots: the smallest power of two >= the most losses a code tolerates
    int low = 0;                            // levels below this one are done by tree_low_levels_kernel (0: the per-thread leaves of degree 2^LEAF_LOG)
    std::vector<CtxPtr> ctx;                // level k (polynomials of degree d = 2^k): transforms of length 2d, T/d columns
    CtxPtr top;                             // few-column levels (chunk_transform_kernel): the upper row bits, 2T / CHUNK rows of CHUNK words
    DeviceBuf<uint32_t> x;                  // 2T words: the level's polynomials, [coefficient][polynomial]
    DeviceBuf<uint32_t> f;                  // 2T words: their transforms
    DeviceBuf<uint32_t> y;                  // 2T words: the next level's polynomials (swaps roles with x)
    DeviceBuf<uint32_t> p;                  // 2T words: pairwise products
    DeviceBuf<uint32_t> wpow;               // NC words: w^u (plain)
    DeviceBuf<uint32_t> roots;              // T words: the erased points, zero-padded
    DeviceBuf<uint32_t> dev_erased;         // T words: erased positions
};

// (2k,k) layout, the transform as two half-size ones ("even / odd split", decode.hip).  ctx, the seven k-word tables and the impulse table are built
// together by the first pattern that wants the split (Prepare::build_split) — all or nothing, see reset() — and kept; the work stripes come lazily
// (split_buffers, StripeDecode::repair_split / decode_split) and are kept.  rows_*, ready, repair_ready, groups and shift are this pattern's
// (Prepare::build_shape clears the two flags, locator_tables sets all of them); dirty follows r1's contents across patterns.
struct SplitTransform {
    CtxPtr ctx;                             // k blocks, per-block factor (2m + k) / 2k
    DeviceBuf<uint32_t> order;              // k words: the block each slot of its first pass holds (gather_tile_order)
    DeviceBuf<uint32_t> rows_data;          // k words, that order: l(w^2i) of the surviving data blocks (0: lost)
    DeviceBuf<uint32_t> rows_parity;        // k words, that order: l(w^(2i+1)) of the parity blocks in use (0: lost or unused)
    DeviceBuf<uint32_t> rows_out;           // k words, that order: gout of the block (0: not lost)
    DeviceBuf<uint32_t> pos_parity;         // k words by position: -w^(-m) / 2 at position bitrev(m)
    DeviceBuf<uint32_t> impulse;            // [IMPULSE_MAX][16][64]: what six DIF levels make of a lone block of a 1024-block tile (run_split_decode)
    DeviceBuf<uint32_t> r1;                 // k blocks: the parity half after its first pass (zero outside the groups in use)
    DeviceBuf<uint32_t> r2;                 // k blocks: ... after all DIF levels
    DeviceBuf<uint32_t> q2;                 // fastecc_repair: k blocks, the data chain's MID output while the top-level result serves the parity chain (lazy)
    DeviceBuf<uint32_t> pos_data_odd;       // k words by position: -w^m / 2 at position bitrev(m) (the parity chain's factor of the data half)
    DeviceBuf<uint32_t> rows_out_parity;    // k words, first-pass order: gout_par of the block (0: not lost)
    bool repair_ready = false;              // this pattern's lost parity blocks can come from the split transform too
    DeviceBuf<uint32_t> r0;                 // codes with fewer parity blocks (fold > 0): parity block j copied to its place j << fold of a k-block stripe (lazy)
    uint32_t groups = 0;                    // block groups of the parity stripe this pattern reads
    // "small" form of the parity half: the parity blocks in use are those at multiples of 2^shift of the parity half (1 <= shift <= 5), so r~
    // is the transform of (k >> shift) rows, each result block standing for 2^shift positions: no k-block stripes r1 / r2, no impulse pass
    uint32_t shift = 0;
    CtxPtr small[6];                        // stand-alone transform contexts of k >> shift blocks (lazy, by shift)
    DeviceBuf<uint32_t> small_buf;          // (k >> shift) blocks: those rows times l, then transformed in place
    uint32_t dirty = 0;                     // groups of r1 that may hold non-zero rows
    bool ready = false;                     // this pattern decodes through the split transform
    bool unavailable = false;               // it could not be built on this context (plan shape, memory): the 2k-point transform serves

    // A build that failed half way leaves nothing behind: a later call builds all of it or none.  Drops the context and what is built with it or
    // under it; q2, r0 and the small form exist only under a built context, and `unavailable` is the caller's to decide.
    void reset()
    {
        ctx.reset();
        for (DeviceBuf<uint32_t>* b : {&order, &rows_data, &rows_parity, &rows_out, &pos_parity, &impulse, &r1, &r2, &pos_data_odd, &rows_out_parity}) b->reset();
    }
};

// Staging of FASTECC_MEM_HOST calls.  Every buffer is made (or grown) by the first call that needs it and kept; the lists name the rows of pattern
// `lists_of` — written by Prepare::direct, else by the first host call under a pattern (StripeDecode::stage_host).
struct HostStaging {
    DeviceBuf<uint32_t> parity_dev;         // the staged codeword: parity stripe, then data stripe
    // only the rebuilt blocks travel back — their row numbers (host, and a device copy)
    std::vector<uint32_t> lost_data, lost_parity;
    std::vector<uint32_t> parity_used;      // few losses: the parity blocks the direct path reads (all it needs staged of a host parity stripe)
    uint64_t lists_of = ~0ull;
    DeviceBuf<uint32_t> lost_rows_dev;      // the two lists back to back
    DeviceBuf<uint32_t> pack_dev;           // the rebuilt blocks, packed
    PinnedBuf<uint32_t> pack_host;          // pinned landing buffer of that copy (kept between calls; the blocks go to their places from here)
};

// One per context (fastecc_ctx::decoder), made at the first fastecc_decode_prepare, freed by destroy_decode_state
struct DecodeState {
    DecodePattern pattern;
    FewLosses few;
    TransformTables tables;
    LocatorTree tree;
    SplitTransform split;
    HostStaging host;
};

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
    // device, behind those rows in the same buffer (one upload): P rows of DIRECT_READ_LOST_ROW words, row q = lost_data[q] padded with SET_LOST_END —
    // an empty row for a pattern that lost no data (fastecc_read_batch_set_device: read_translate_kernel)
    const uint32_t* d_lost_data = nullptr;
    uint32_t rows_max = 0;              // the most rows any of its passes reads
    // one call's entries, sorted by class (list.dev is an internal buffer: ordered between streams by the context's buf_event).  Outlives the set.
    StagedList<DirectSetEntry> list;
    DirectPass* pass(uint64_t q) const { return kind[q] == DATA ? tables[q].data.get() : kind[q] == PARITY ? tables[q].parity.get() : tables[q].both.get(); }
};

// The state of a codeword position in a pattern.  ST_UNUSED: a surviving parity block the split transform does not read — a root of the locator like
// a lost one, but nothing to rebuild
enum : uint32_t { ST_LOST = 0, ST_HELD = 1, ST_ZERO = 2, ST_UNUSED = 3 };

namespace {  // (helpers of the three files, each with its own copy as before the split: the library exports nothing for them)

dim3 grid_of(uint64_t items) { return dim3((unsigned)((items + 255) / 256)); }  // one thread per item, 256 per workgroup

// A row kernel (one wave per (block row, 64*V-word column chunk)) over `rows` rows of S words: V = 4 when S is a multiple of 4 and every pointer in
// `ptrs` is 16-byte aligned, else 1.  `args` are the kernel's arguments but the last two (chunks per row, waves in all).
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

// the context's decoder state, made at its first use (nullptr: no memory)
DecodeState* state_of(fastecc_ctx* c)
{
    if (!c->decoder) c->decoder = new (std::nothrow) DecodeState();
    return c->decoder;
}

}  // namespace

// ---- decode_prepare.hip, for pattern_set.hip ----
// What direct_tables needs of a code: the transform order N, data block i at position i << e of the NC = N << e positions, and the context for K,
// fold and cosets
struct CodeGeometry {
    const fastecc_ctx* c;
    uint64_t N;
    int e;
    uint64_t NC;
    explicit CodeGeometry(const fastecc_ctx* ctx) : c(ctx), N(transform_order(ctx)), e(code_coset_shift(ctx->cosets)), NC(N << e) {}
    uint64_t parity_position(uint64_t q) const { return code_parity_position(N, e, c->fold, c->cosets, q); }
};
// The direct path's tables of one pattern: the lost data blocks R (each a fixed linear combination of the surviving data blocks and of the
// surviving parity blocks A, one per lost data block), the lost parity blocks Pl.  Data AND parity lost, at most 32 in all: one pass, `both`
// (the lost parity blocks as further outputs on the data pass's nodes); else `data` for the lost data and `parity` (from the complete data)
// for the lost parity.  Passes are allocated where t holds none yet.  Takes no lock and touches no context state: the single pattern's
// fastecc_decode_prepare (Prepare::direct) and every pattern of a set (fill_pattern_set) come through here.
int direct_tables(const CodeGeometry& g, const std::vector<uint32_t>& R, const std::vector<uint32_t>& Pl, const std::vector<uint32_t>& A, PatternTables& t,
                  PhaseTimer& ptd);

}  // namespace fastecc
