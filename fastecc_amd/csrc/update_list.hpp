// update_list.hpp — what a pool write call hands its parity kernels (update.hip, DESIGN.md sections 15, 33, 36 and 40): the sorted write list and the
// segment tables, their formats, and the host code that builds them.  Nothing here needs HIP: the kernels read the constants, the drivers call
// sort_writes and build_update_list, and tests/test_update_list_host.py compiles both with the host compiler alone.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace fastecc {

constexpr int ROWS = 16;  // changed blocks per pass: delta rows held in VGPRs (32 spills SGPRs: the 32 row positions and their weights)

constexpr int LIST_WORDS = 4;  // one write of the sorted list: position of its data block (i << e), its row of new_blocks, its stripe (low, high word)
constexpr int SEG_HEAD = 2;    // one segment of a launch of class T: its first write in the sorted list, its number of writes (1 .. T), then the T
                               // positions of its rows (rows past its length: that of row 0) — SEG_HEAD + T words

constexpr int SET_LIST_WORDS = LIST_WORDS + 2;  // ... and where the write's old row is: its offset in words from SetArgs::old_base (low, high word; negative where the
                                                // row lies below the base) — the pool's data block, or for an ABSENT data block its row of the reconstruction
                                                // buffer; the parity form: its row of old_blocks.  An absent block's write has ROW_ABSENT set in its row word.
constexpr int SET_SEG_HEAD = SEG_HEAD + 1;      // ... and the offset (words) of its stripe's row of the pattern set's lost parity blocks
constexpr uint32_t ROW_ABSENT = 0x80000000u;    // (a call has fewer than 2^31 rows: update_batch_args)
constexpr uint32_t OLD_IN_POOL = 0xFFFFFFFFu;   // host: ListSet::old_row of a write whose data block is present

struct SortedWrite {
    uint64_t index;  // b * k + i
    uint32_t row;    // its row of new_blocks / old_blocks
};

// The writes by (stripe, block), each with its row of the caller's blocks; false for an index >= count * K or a duplicate (n_writes > 0)
inline bool sort_writes(uint64_t K, uint64_t count, const uint64_t* writes, uint64_t n_writes, std::vector<SortedWrite>& out)
{
    out.resize(n_writes);
    for (uint64_t u = 0; u < n_writes; u++) out[u] = SortedWrite{writes[u], (uint32_t)u};
    std::sort(out.begin(), out.end(), [](const SortedWrite& x, const SortedWrite& y) { return x.index < y.index; });
    if (out.back().index >= count * K) return false;  // (count * K fits: update_batch_args)
    for (uint64_t u = 1; u < n_writes; u++)
        if (out[u].index == out[u - 1].index) return false;
    return true;
}

struct BatchLaunch {
    int T;
    uint32_t seg0, segs;     // its segment table: first word after the list, number of segments
    uint64_t parity_blocks;  // parity blocks its segments read and write (the profile's byte count)
};

// The pool and the form of the records
struct ListShape {
    uint64_t K;
    int e;                       // position of data block i: i << e
    uint64_t S, W, col0, M;      // words of a block, of a row of the caller's blocks and of the reconstruction buffer; the window's first column; parity blocks
    bool with_data, long_form;   // the old rows come from the data pool (else: by row of the caller's list); SET_LIST_WORDS and SET_SEG_HEAD
};
// What a pattern set adds, every array by write of the SORTED list (a long-form call without one: null).  A set always has the long records, whatever
// ListShape::long_form says: only they hold where an absent block's old row is.
struct ListSet {
    const uint32_t* old_row;         // OLD_IN_POOL, or its row of the reconstruction buffer (its data block is absent)
    const uint32_t* lost_row;        // its stripe's row of the set's lost parity blocks, rows of lost_pitch words
    const uint32_t* present_parity;  // its stripe's present parity blocks
    uint32_t lost_pitch;
    uint64_t recon_offset;           // the reconstruction buffer's offset from old_base, in words (two's complement where it lies below)
};
struct BuiltList {
    uint32_t seg_words;  // words of all segment tables, which follow the sw.size() records at `list`
    uint64_t stored;     // writes whose data block is there to be stored
};

// The records of sw into `list` and behind them the segment tables, one BatchLaunch each (room for sw.size() * (record + head + 1) words: a segment of len
// writes takes head + T <= (head + 1) len words).  Each stripe's writes are cut into segments of at most ROWS; segment r of a stripe runs in round r
// (segments of one stripe read-modify-write the same parity blocks), a round's segments are grouped by their length padded to a power of two, T, and the
// tables stand by round, then T, a table's segments in the order of the list.
// LONG = (f.long_form or a set) and SET = (set != null) are template parameters so that the record size and the source of the old row are constants in the per-write
// loop: with the size read at run time the calls with long records measured 3 to 4 % more host time at 32768 writes (HISTORY.md).  build_update_list,
// below, is the call.
template <bool LONG, bool SET>
BuiltList build_update_list_form(const std::vector<SortedWrite>& sw, const ListShape& f, const ListSet* set, uint32_t* list, std::vector<BatchLaunch>& launches)
{
    const uint64_t n = sw.size(), K = f.K, S = f.S, W = f.W, col0 = f.col0, recon = SET ? set->recon_offset : 0;  // (locals: the per-write loop reads no struct)
    const uint32_t* old_row = SET ? set->old_row : nullptr;
    const int e = f.e;
    const bool with_data = f.with_data;
    constexpr int list_words = LONG ? SET_LIST_WORDS : LIST_WORDS, seg_head = LONG ? SET_SEG_HEAD : SEG_HEAD;
    std::vector<std::vector<uint32_t>> bucket;  // [round * 5 + class]: first write of each segment (its length: to the stripe's end, at most ROWS)
    std::vector<uint32_t> stripe_end(n);        // per write: one past the last write of its stripe
    uint64_t stored = n;
    for (uint64_t first = 0; first < n;) {
        const uint64_t b = sw[first].index / K;
        uint64_t g = first;
        for (; g < n && sw[g].index < (b + 1) * K; g++) {
            uint32_t* wr = list + g * list_words;
            wr[0] = (uint32_t)((sw[g].index - b * K) << e);
            wr[1] = sw[g].row;
            wr[2] = (uint32_t)b;
            wr[3] = (uint32_t)(b >> 32);
            if constexpr (LONG) {  // its old row, from old_base (a window: its columns of the pool's block, or a row of W words)
                const uint32_t r = SET ? old_row[g] : OLD_IN_POOL;
                const uint64_t off = r != OLD_IN_POOL ? recon + (uint64_t)r * W : with_data ? sw[g].index * S + col0 : (uint64_t)sw[g].row * W;
                wr[LIST_WORDS] = (uint32_t)off;
                wr[LIST_WORDS + 1] = (uint32_t)(off >> 32);
                if (r != OLD_IN_POOL) wr[1] |= ROW_ABSENT, stored--;
            }
        }
        for (uint64_t a0 = first, r = 0; a0 < g; a0 += ROWS, r++) {
            int cls = 0;
            while ((1u << cls) < std::min<uint64_t>(ROWS, g - a0)) cls++;
            if (bucket.size() < (r + 1) * 5) bucket.resize((r + 1) * 5);
            bucket[r * 5 + cls].push_back((uint32_t)a0);
            stripe_end[a0] = (uint32_t)g;
        }
        first = g;
    }
    uint32_t* segs = list + n * list_words;
    uint32_t seg_words = 0;
    for (size_t i = 0; i < bucket.size(); i++) {
        if (bucket[i].empty()) continue;
        const int T = 1 << (int)(i % 5);
        launches.push_back(BatchLaunch{T, seg_words, (uint32_t)bucket[i].size(), 0});
        for (uint32_t first : bucket[i]) {
            const uint32_t len = std::min<uint32_t>(ROWS, stripe_end[first] - first);
            uint32_t* seg = segs + seg_words;
            seg[0] = first;
            seg[1] = len;
            if constexpr (LONG) seg[SEG_HEAD] = SET ? set->lost_row[first] * set->lost_pitch : 0;  // (no set: the one row that loses nothing)
            for (int r = 0; r < T; r++) seg[seg_head + r] = list[(size_t)(first + ((uint32_t)r < len ? r : 0)) * list_words];
            seg_words += seg_head + T;
            launches.back().parity_blocks += SET ? set->present_parity[first] : f.M;
        }
    }
    return BuiltList{seg_words, stored};
}
inline BuiltList build_update_list(const std::vector<SortedWrite>& sw, const ListShape& f, const ListSet* set, uint32_t* list, std::vector<BatchLaunch>& launches)
{
    if (set) return build_update_list_form<true, true>(sw, f, set, list, launches);
    return f.long_form ? build_update_list_form<true, false>(sw, f, set, list, launches) : build_update_list_form<false, false>(sw, f, set, list, launches);
}

}  // namespace fastecc
