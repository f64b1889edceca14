// internal.hpp — what the translation units share that needs no fastecc_ctx member: the error helpers (HIP_TRY / hip_fail), DeviceGuard, guarded,
// PhaseTimer, the code positions, the sub-states' forward declarations and destroy functions, and the interfaces of direct.hip, pool_encode.hip,
// the transform contexts and the split transform (which take a context as an opaque pointer).  Whoever reads or writes the context itself includes
// context.hpp (the struct) or drivers.hpp (the drivers, the call lock, buffer ordering, profiling).  Nothing here is part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <vector>

#include "../../include/fastecc.h"

namespace fastecc {

// ---- the helpers of every entry point ----
// The failed HIP call `what` becomes this thread's fastecc_last_error_detail and the error is cleared: FASTECC_E_NOMEM for an out-of-memory error,
// else FASTECC_E_DEVICE (api.hip)
int hip_fail(hipError_t e, const char* what);
#define HIP_TRY(expr)                                     \
    do {                                                  \
        hipError_t e_ = (expr);                           \
        if (e_ != hipSuccess) return hip_fail(e_, #expr); \
    } while (0)

// FASTECC_TRACE_PREPARE=1: wall-clock of the phases of a decode_prepare on stderr (where does a first call spend its time), one line per mark():
// the prefix, the label padded to `width`, the time since the previous mark
struct PhaseTimer {
    const char* prefix;
    int width;
    bool on = getenv("FASTECC_TRACE_PREPARE") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit PhaseTimer(const char* prefix_ = "[fastecc prepare]", int width_ = 28) : prefix(prefix_), width(width_) {}
    void mark(const char* what)
    {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "%s %-*s %8.3f ms\n", prefix, width, what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};

// the current device is `dev` for the scope, the previous one again after it
struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// No exception crosses the ABI: an entry point's body runs through this, and an allocation failure of the host code (std::vector) is
// FASTECC_E_NOMEM (the call locks of the context are scoped objects, so they are released on the way out)
template <class F> int guarded(F body)
{
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return FASTECC_E_NOMEM;
    } catch (...) {
        return FASTECC_E_DEVICE;
    }
}

struct DecodeState;                        // decode_state.hpp: tables of one erasure pattern + the size-2k transform context
void destroy_decode_state(DecodeState*);   // decode.hip, called by fastecc_destroy
struct PatternSet;                         // decode_state.hpp: the tables of a pattern set (fastecc_decode_prepare_set) and the set calls' list buffers
void destroy_pattern_set(PatternSet*);     // pattern_set.hip, called by fastecc_destroy
struct ScrubState;                         // scrub.hip: error detection and location (fastecc_verify, _locate_errors, _correct)
void destroy_scrub_state(ScrubState*);     // scrub.hip, called by fastecc_destroy
struct UpdateState;                        // update.hip: the parity update's weight table and delta rows (fastecc_update, _update_parity)
void destroy_update_state(UpdateState*);   // update.hip, called by fastecc_destroy
struct Gf61UpdateState;                    // gf61_update.hip: the same for the 64-bit field (fastecc_gf61_update, _gf61_update_parity)
void destroy_gf61_update_state(Gf61UpdateState*);  // gf61_update.hip, called by fastecc_destroy

// Every GF(0xFFF00001) code is f (degree < N, the transform order: a power of two, or q * 2^m for the mixed-radix codes) on a subset of
// the NC-th roots of unity, NC = N << e, position u <-> w_NC^u: data block i at i << e, parity block q at code_parity_position — odd
// multiples of 2^fold for the codes inside (2N,N), the cosets' offsets for n = 4k / 8k (fastecc_create).  decode_prepare.hip, scrub.hip, update.hip.
inline int code_coset_shift(int cosets)
{
    int e = 1;
    while ((1 << e) < cosets + 1) e++;
    return e;
}
inline uint64_t code_parity_position(uint64_t N, int e, int fold, int cosets, uint64_t q)
{
    if (cosets > 1) {
        const uint64_t t = q / N, j = q % N;  // coset t = generator w_(N << jj)^c, see fastecc_create
        int jj = 1;
        while ((1ull << jj) - 1 <= t) jj++;
        const uint64_t odd = 2 * (t + 1 - (1ull << (jj - 1))) + 1;
        return (odd << (e - jj)) + (j << e);
    }
    return ((q << fold) << 1) + 1;
}

struct Sharded;                            // sharded.hip: one stripe in column slabs on several devices (fastecc_create_sharded; its calls: context.hpp)
void destroy_sharded(Sharded*);            // sharded.hip, called by fastecc_destroy

// ---- direct.hip: blocks as fixed linear combinations of other blocks (few lost blocks / few parity blocks) ----
struct DirectPass;                 // the weights of one pattern (or code) and the work buffers of its pass
DirectPass* direct_pass_new();
void direct_pass_free(DirectPass*);
int direct_cap();                  // most outputs (lost or parity blocks) of one pass
// Output t = f(y[t]) from ALL K data rows (row i at the point wd^i, wd of order N): weight c[t] x_i / (y[t] - x_i), c[t] = (y[t]^N - 1) / N;
// written to data row pos >> 1 (pos even) or parity row pos >> 1 (pos odd).  Synchronises `st`.
int direct_build_lagrange(DirectPass* p, uint32_t wd, uint32_t K, const std::vector<uint32_t>& y, const std::vector<uint32_t>& c, const std::vector<uint32_t>& out_pos,
                          hipStream_t st);
// The lost data rows (points lost_points) from the surviving data rows and as many surviving parity rows (node_rows at node_points).
// more_points / more_pos: further outputs on the same nodes — f at those points, written to row pos >> 1 of the parity (pos odd) or data stripe: the lost
// parity blocks, for fastecc_repair in one pass.
int direct_build_interp(DirectPass* p, uint32_t wd, uint64_t N, uint32_t K, const std::vector<uint32_t>& lost_rows, const std::vector<uint32_t>& lost_points,
                        const std::vector<uint32_t>& node_rows, const std::vector<uint32_t>& node_points, hipStream_t st,
                        const std::vector<uint32_t>* more_points = nullptr, const std::vector<uint32_t>* more_pos = nullptr);
// kernel: 0 = choose, 1 = VALU (96-bit lazy accumulation), 2 = MFMA (i8 digits) when the stripes allow it
int direct_run(DirectPass* p, const uint32_t* data, const uint32_t* parity, uint32_t* data_out, uint32_t* parity_out, uint32_t S, int kernel, hipStream_t st);
// The same pass over `count` stripes in ONE launch (VALU, no partial sums): stripe b's rows at data + b * data_stride and parity + b * parity_stride
// (words), its outputs at the same places of data_out / parity_out (each either the input stripe or null: that kind of output is skipped).
// list != null (device, `count` entries): the stripes list[0 .. count) of the pool instead of its stripes 0 .. count
int direct_run_batch(DirectPass* p, const uint32_t* data, const uint32_t* parity, uint32_t* data_out, uint32_t* parity_out, uint64_t S, uint64_t count,
                     uint64_t data_stride, uint64_t parity_stride, hipStream_t st, const uint64_t* list = nullptr);
uint64_t direct_batch_waves(const DirectPass* p, const void* data, const void* parity, uint64_t S, uint64_t count);  // waves of that launch, all sweeps
int direct_pass_rows(const DirectPass* p);  // rows a pass reads (lost data rows included, at weight 0)
// Many stripes, a pattern per stripe, in ONE launch (direct_set_kernel): the stripes entries[0 .. n) of a pool, each with the pass passes[entry.pass].
// Both arrays in DEVICE memory.  Every pass of a launch has at most 16 outputs and the same pad `eb` (1, 2, 4, 8, 16).
struct DirectSetPass {  // what the kernel takes from one built DirectPass
    const uint32_t* coef;   // [rows][cstride], Montgomery form
    const uint32_t* extra;  // rows data_rows.. of the pass are parity rows extra[u - data_rows]
    const uint32_t* pos;    // outputs: data row pos >> 1 (even) or parity row pos >> 1 (odd)
    uint32_t rows, data_rows, outputs;
    uint32_t cstride;       // == the pass's pad: the class a launch is templated on (the kernel strides by that constant)
};
struct DirectSetEntry {
    uint64_t stripe;  // of the pool
    uint32_t pass;    // index into the descriptor table
    uint32_t reserved;
};
int direct_set_describe(const DirectPass* p, DirectSetPass* out);  // FASTECC_E_INVAL: not built, or more than 16 outputs
// waves one entry takes (V chosen for the class, the pointers' alignment and S); more than 2^24: direct_run_set refuses (FASTECC_E_UNSUPPORTED)
uint64_t direct_set_waves_per_entry(int eb, const void* data, const void* parity, uint64_t S);
int direct_run_set(int eb, const DirectSetPass* passes, const DirectSetEntry* entries, uint64_t n_entries, const uint32_t* data, const uint32_t* parity,
                   uint32_t* data_out, uint32_t* parity_out, uint64_t S, uint64_t data_stride, uint64_t parity_stride, hipStream_t st);
// Degraded reads (fastecc_read_batch / _read_batch_set; direct_read_kernel): a list of requests, each ONE data block of a pool over the word
// columns [col0, col0 + width), stored to row `entry index` of a compact buffer `out` of `width` words per row.  The pool is only read.
// A present block is a copy of its window; a lost one is output `out` of the pass passes[entry.pass] over its stripe's survivors — one column
// of that pass's weight table.  The table's row stride comes from the descriptor, so one launch serves every pad class of a set and, with
// direct_read_describe, the sweep-major tables of passes with more than 16 outputs.  Both arrays in DEVICE memory.
constexpr uint32_t DIRECT_READ_PRESENT = 0xFFFFFFFFu;
struct DirectReadEntry {
    uint64_t stripe;  // of the pool
    uint32_t pass;    // index into the descriptor table (not looked at for a present block)
    uint32_t block;   // the data block of the stripe
    uint32_t out;     // its output index in the pass, or DIRECT_READ_PRESENT
    uint32_t reserved;
};
// direct_set_describe for a pass of any pad: cstride = min(pad, 16), the row stride inside a sweep of the table (coef_index).  For direct_run_read only.
int direct_read_describe(const DirectPass* p, DirectSetPass* out);
// waves one request takes (V chosen for the pointers' alignment, S, col0 and width); more than 2^24: direct_run_read refuses (FASTECC_E_UNSUPPORTED)
uint64_t direct_read_waves_per_entry(const void* data, const void* parity, const void* out, uint64_t S, uint64_t col0, uint64_t width);
// The caller guarantees col0 + width <= S, entry.block < data rows, entry.out < the pass's outputs and room for n_entries * width words at `out`.
int direct_run_read(const DirectSetPass* passes, const DirectReadEntry* entries, uint64_t n_entries, const uint32_t* data, const uint32_t* parity, uint32_t* out,
                    uint64_t S, uint64_t col0, uint64_t width, uint64_t data_stride, uint64_t parity_stride, hipStream_t st);
// The request list in device memory (fastecc_read_batch_device / _read_batch_set_device): read_translate_kernel, one lane per
// request, makes entry u of `entries` from reads[u] on the stream — what read_batch_impl's translate makes on the host — and direct_run_read_device
// is direct_run_read behind a look at the status word.  A FASTECC_READ_NONE request becomes an entry with out = DIRECT_READ_SKIP: no wave touches
// its row.  A request at fault (an index >= blocks, in the set form a pattern_of entry that is neither FASTECC_PATTERN_NONE nor < patterns) sets
// *status to (uint32_t)FASTECC_E_INVAL << 32 | u unless it is non-zero already; every wave of the read launches returns on a non-zero status.
constexpr uint32_t DIRECT_READ_SKIP = 0xFFFFFFFEu;
constexpr uint32_t DIRECT_READ_LOST_ROW = 16;  // words per pattern of ReadTranslate::lost in the set form
struct ReadTranslate {
    const uint64_t* reads;       // device: n requests b * K + i, or FASTECC_READ_NONE
    const uint32_t* pattern_of;  // device: the pool's `count` entries (set form); null: the single pattern
    // device.  Set form: `patterns` rows of DIRECT_READ_LOST_ROW words, row q = pattern q's lost data blocks in the order of its pass's outputs, then
    // 0xFFFFFFFF to the end.  Single pattern: its n_lost lost data blocks, increasing (not read when n_lost == 0).
    const uint32_t* lost;
    uint64_t* status;            // device
    DirectReadEntry* entries;    // device: room for n entries
    uint64_t n, blocks, K;       // requests; count * K
    uint32_t patterns, n_lost;
};
int direct_run_read_translate(const ReadTranslate& t, hipStream_t st);
int direct_run_read_device(const DirectSetPass* passes, const DirectReadEntry* entries, uint64_t n_entries, const uint32_t* data, const uint32_t* parity,
                           uint32_t* out, uint64_t S, uint64_t col0, uint64_t width, uint64_t data_stride, uint64_t parity_stride, const uint64_t* status,
                           hipStream_t st);
bool direct_mfma_applies(const void* data, const void* parity, uint64_t words);
// encoding straight from the Lagrange basis for codes with few parity blocks (n - k <= direct_encode_max())
struct DirectEncode;
int direct_encode_max();
int direct_encode_build(DirectEncode** out, uint64_t N, uint64_t K, uint64_t m, int fold, uint64_t words);  // current device = the context's
int direct_encode_run(DirectEncode* de, const uint32_t* data, uint32_t* parity, int kernel, hipStream_t st);
void direct_encode_destroy(DirectEncode* de);
DirectPass* direct_encode_pass(DirectEncode* de);  // its one pass: rows == data_rows == k, every output a parity row (for direct_run_batch)
// The weight fragments of pool_encode.hip's kernel for sweeps of `mt` M-tiles (1, 2 or 4: 8 mt outputs): [ceil(k / 8)][*mt_total][64] uint4 in
// mfma_weights_kernel's layout, zero for rows >= k and outputs >= n - k.  Built by a kernel on `st` at the first call and never rewritten; a later
// call on another stream is ordered behind that kernel on the device.  No host synchronisation.
int direct_encode_pool_fragments(DirectEncode* de, int mt, hipStream_t st, const uint4** frag, uint32_t* mt_total);

// ---- pool_encode.hip: the parity of a pool of stripes on the matrix cores, one launch (fastecc_encode_pool, option "encode_pool_kernel" = 2) ----
bool pool_encode_mfma_applies(const void* data, const void* parity, uint64_t k, uint64_t words, uint64_t count);
int pool_encode_mfma_tiles(uint64_t outputs);  // M-tiles per wave and sweep: 1, 2 or 4
int pool_encode_mfma_run(const uint4* frag, uint32_t mt_total, int mt, const uint32_t* data, uint32_t* parity, uint32_t k, uint32_t outputs, uint32_t words,
                         uint64_t count, hipStream_t st);

// ---- api.hip, host_copy.hip ----
void set_error_text(const char* text);  // this thread's fastecc_last_error_detail, verbatim (a worker thread's text republished on the caller's)
// host_copy.hip: `rows` pieces of `width` bytes between two pitched host buffers (software prefetch + streaming stores)
void host_copy_rows(char* dst, size_t dst_pitch, const char* src, size_t src_pitch, size_t width, size_t rows);

// ---- create.hip, encode.hip: the transform contexts ----
// A transform context (GF(0xFFF00001)): DIF over all log2k levels with inverse roots, the block holding coefficient m
// multiplied by factor[m] (plain representatives, k entries), DIT back with forward roots keeping every 2^fold-th
// output block.  fastecc_encode(ctx, in, out, FASTECC_MEM_DEVICE, stream) runs it; k may be 2^20 (no root of order 2k
// is needed).  The encoder of RS.cpp:40-63 is the case factor[m] = w_2k^m / k.
int create_transform_ctx(fastecc_ctx** out, int log2k, uint64_t block_bytes, int fold, const uint32_t* factor, int device);
// create_transform_ctx with factor[m] = m * scale, the table written by a kernel (the decoder's x p'(x) transform: scale = 1 / 2^log2k)
int create_ramp_transform_ctx(fastecc_ctx** out, int log2k, uint64_t block_bytes, int fold, uint32_t scale, int device, uint32_t offset = 0);  // factor m * scale + offset
// A context for stand-alone transforms only (fastecc_ntt, transform_bitrev): no per-block factor table is built, fastecc_encode is unsupported.
int create_ntt_ctx(fastecc_ctx** out, int log2k, uint64_t block_bytes, int device);
// The same for a transform of order q * 2^log2m (q an odd radix of mixed_kernels.hip): factor has q << log2m entries by
// coefficient index; fastecc_encode(ctx, in, out, DEVICE, stream) maps all q << log2m blocks, in place if in == out.
int create_mixed_transform_ctx(fastecc_ctx** out, int q, int log2m, uint64_t block_bytes, const uint32_t* factor, int device);
// The way down of such a context alone (inverse roots, unscaled): block j1 * 2^log2m + r of `out` holds
// Y[q * bitrev(r) + j1],  Y[v] = sum_i in[i] w^(-i v),  w of order q << log2m.
int mixed_dif(fastecc_ctx* c, const uint32_t* in, uint32_t* out, hipStream_t st);
// Decoder: when the transform's first pass is a register DIF pass it can read the codeword straight from its two
// halves (PassArgs::in_odd / row_factor) and the separate gather pass disappears.  run_gathered does that and returns
// FASTECC_E_UNSUPPORTED (nothing enqueued) when the plan starts with another kind of pass.
int run_gathered(fastecc_ctx* c, const uint32_t* even_blocks, const uint32_t* odd_blocks, const uint32_t* row_factor, uint32_t* out,
                 hipStream_t st);
// Half a stand-alone transform of a transform context, on the word columns [0, width) of every block: dit = false runs the
// DIF passes (natural order in, bit-reversed order out), dit = true the mirrored DIT passes (bit-reversed in, natural out);
// unscaled, forward roots or (inverse_roots) their inverses.  A product of transforms does not care about the order, so
// polynomial products on the device need no permutation pass (decode_prepare.hip: the erasure locator's product tree).
int transform_bitrev(fastecc_ctx* c, const uint32_t* in, uint32_t* out, bool dit, bool inverse_roots, uint32_t width, hipStream_t st);
// The order in which that first pass wants row_factor: returns false when it is the natural order (register pass),
// else fills `order` with order[i] = codeword position whose factor is entry i of the table (two-window DIF tile:
// the factors of one wave are contiguous).
bool gather_tile_order(const fastecc_ctx* c, std::vector<uint32_t>& order);
bool gather_tile_order_device(const fastecc_ctx* c, uint32_t* order, hipStream_t st);  // the same N words, written on the device
bool same_tile_order(const fastecc_ctx* a, const fastecc_ctx* b);
// The decoder's split transform (decode.hip, "even / odd split") on a context of k blocks created by create_ramp_transform_ctx with the factor
// (2m + k) / 2k: data and parity stripes each through the plan's first DIF tile with per-block factors (tile order: gather_tile_order; a zero
// factor = block not used), the parity half only in its first `parity_groups` block groups (group g = blocks g + (t << s), t < group_rows; the
// rest of r1 must be zero and stays zero), its low levels as a DIF tile of their own (r1 -> r2), then MID on q with + r2[p] * parity_pos_factor[p]
// and the plan's DIT tile.  q, r1, r2: k blocks each; the result, x p'(x) at the data positions, is left in q.
bool split_decode_supported(const fastecc_ctx* c);
uint32_t split_decode_groups(const fastecc_ctx* c);
uint32_t split_decode_group_rows(const fastecc_ctx* c);
int split_impulse_max();  // IMPULSE_MAX of kernels.hpp
// odd != null (fastecc_repair, (2k,k) layout): x p'(x) at the odd positions as well — MID's second half and a DIT once more over the same two halves.
struct SplitRepair {
    uint32_t* q2;                      // k blocks: the data half after ALL its DIF levels, stored by the first chain's MID on its way; the second chain works there
    const uint32_t* data_pos_factor;   // k words by position: -w^m / 2 at position bitrev(m)
    const uint32_t* out_rows_factor;   // k words, tile order: 1 / (w^(2j+1) l'(w^(2j+1))) of the lost parity blocks, 0 elsewhere
    uint32_t* out;                     // the parity stripe
};
// out_rows_factor != null: the DIT tile stores only the blocks with a non-zero factor (tile order), times it, to out[] (the decoder's scatter).
int run_split_decode(fastecc_ctx* c, const uint32_t* data, const uint32_t* parity, const uint32_t* data_rows_factor, const uint32_t* parity_rows_factor,
                     uint32_t parity_groups, const uint32_t* parity_pos_factor, uint32_t* q, uint32_t* r1, uint32_t* r2, const uint32_t* out_rows_factor,
                     uint32_t* out, const uint32_t* impulse_table, uint32_t data_blocks, uint32_t parity_blocks, hipStream_t st,
                     const SplitRepair* odd = nullptr, const uint32_t* small_addend = nullptr, uint32_t addend_shift = 0);
// small_addend != null (1 <= addend_shift <= 5): the parity blocks in use sit at multiples of 2^shift of the parity half only.  The DIF of such a
// stripe is the DIF of its (k >> shift) non-zero rows with every result block repeated 2^shift times (the last `shift` levels pair a value with a
// zero under the twiddle 1), so the caller has transformed those rows alone — small_addend, (k >> shift) blocks in that transform's own bit-
// reversed order — and parity, parity_rows_factor, parity_groups, r1, r2 and impulse_table are not used.
// data_blocks / parity_blocks: the blocks the two stripes really hold (<= k: zero-extended codes; the rest counts as zero blocks)
// impulse_table (optional): [IMPULSE_MAX][16][64] words (Montgomery form), entry [t][g][c] = block g + 16 c of a 1024-block tile after the DIF
// levels with strides 512 ... 16 when block g + 16 t alone was 1 — with at most 16 IMPULSE_MAX parity groups in use those six of the parity
// half's low levels are a multiply-add per word and block in use (MODE_DIF_IMPULSE)

}  // namespace fastecc
