// drivers.hpp — what the translation units behind the C ABI share beyond context.hpp: the encode drivers (encode.hip), the host staging
// paths (host_stage.hip) and context creation (create.hip), called from the entry points in api.hip, the decoder's three files (decode_prepare.hip,
// decode.hip, pattern_set.hip), scrub.hip, update.hip and sharded.hip; and the one mechanism each for profiling (ProfScope, P61Hooks), for ordering the internal buffers between streams
// (with_internal_buffers, wait_idle) and for the extent of a pool (pool_extent).  Nothing here is part of the ABI.
#pragma once
#include <condition_variable>
#include <thread>

#include "context.hpp"
#include "launch_limits.hpp"

namespace fastecc {

// widest lane vector that the block size and the pointers allow
inline int pick_vec(const fastecc_ctx* c, const void* a, const void* b)
{
    int v = c->vec;
    const uintptr_t bits = (uintptr_t)a | (uintptr_t)b;
    while (v > 1 && ((c->S % v) != 0 || (c->ld % v) != 0 || (bits % (4u * v)) != 0)) v >>= 1;
    return v;
}

struct ProfScope {
    fastecc_ctx* c;
    hipStream_t st;
    ProfileRec* rec = nullptr;
    ProfScope(fastecc_ctx* c_, hipStream_t st_, const char* name, uint64_t bytes = 0) : c(c_), st(st_)
    {
        if (!c->profiling) return;
        if (c->prof_used == c->prof.size()) {
            ProfileRec r;
            if (r.start.try_create() != hipSuccess || r.stop.try_create() != hipSuccess) return;
            c->prof.push_back(std::move(r));
        }
        rec = &c->prof[c->prof_used++];
        rec->name = name;
        rec->bytes = bytes;
        (void)hipEventRecord(rec->start, st);
    }
    void finish()
    {
        if (rec) (void)hipEventRecord(rec->stop, st);
        rec = nullptr;
    }
    ~ProfScope() { finish(); }
};

// fastecc_profile_* for the launches of gf61_kernels.hip: one ProfScope per launch (launches of a context are serial)
struct P61Hooks {
    fastecc_ctx* c;
    ProfScope* open = nullptr;
    p61::LaunchHooks h;
    explicit P61Hooks(fastecc_ctx* c_) : c(c_)
    {
        h.user = this;
        h.begin = [](void* u, hipStream_t st, const char* name, uint64_t bytes) {
            P61Hooks* self = (P61Hooks*)u;
            self->open = new (std::nothrow) ProfScope(self->c, st, name, bytes);
        };
        h.end = [](void* u, hipStream_t) {
            P61Hooks* self = (P61Hooks*)u;
            delete self->open;
            self->open = nullptr;
        };
    }
    ~P61Hooks() { delete open; }
};

// ---- encode.hip: the device drivers ----
int run_passes(fastecc_ctx* c, const std::vector<Pass>& plan, const uint32_t* in, uint32_t* out, const uint32_t* tw_dif,
               const uint32_t* tw_dit, hipStream_t st, uint32_t col0 = 0, uint32_t width = 0, hipEvent_t first_done = nullptr,
               uint32_t batch = 1, const CallBounds& cb = CallBounds());
// The encode plan of a (2k,k) power-of-two code over `count` stripes back to back (k blocks apart in both buffers), cut into runs of stripes so that
// no pass of a run takes more than MAX_LAUNCH_WAVES waves (a stripe of more waves than that is a run of its own).  FASTECC_E_UNSUPPORTED, before any
// device work, when a pass of one stripe does not fit a dispatch (run_passes).
int encode_batch_passes(fastecc_ctx* c, const uint32_t* data, uint32_t* parity, uint64_t count, hipStream_t st);
int ensure_slab_streams(fastecc_ctx* c);
bool plan_is_all_tiles(const std::vector<Pass>& plan);
int encode_pow2(fastecc_ctx* c, const uint32_t* data, uint32_t* parity, hipStream_t st, const CallBounds& cb = CallBounds());
int encode_mixed(fastecc_ctx* c, const uint32_t* data, uint32_t* parity, hipStream_t st);
bool direct_encode_applies(const fastecc_ctx* c, const void* data = nullptr, const void* parity = nullptr);
int encode_device(fastecc_ctx* c, const uint32_t* data, uint32_t* parity, hipStream_t st);
// `count` stripes back to back (stripe b's k data blocks at data + b * k * S words, its n - k parity blocks at parity + b * (n - k) * S): fastecc_encode_pool
int encode_pool_device(fastecc_ctx* c, const uint32_t* data, uint32_t* parity, uint64_t count, hipStream_t st);
int ntt_device(fastecc_ctx* c, uint32_t* data, bool inverse, hipStream_t st);
// Work that uses the context's internal device buffers is ordered between streams (fastecc_ctx::buf_event); the caller holds c->mu for all three:
// order makes `st` wait for the previous such work, mark records this one, wait_idle is the host-side wait for the last recorded one (instead of a
// device-wide synchronise: before tables that device work may still read are rebuilt).
int order_internal_buffers(fastecc_ctx* c, hipStream_t st);
int mark_internal_buffers(fastecc_ctx* c, hipStream_t st);
int wait_idle(fastecc_ctx* c);
// Runs `body` (which enqueues work on `st` that uses internal buffers) between the two.
template <class F> int with_internal_buffers(fastecc_ctx* c, hipStream_t st, F body)
{
    int rc = order_internal_buffers(c, st);
    if (rc != FASTECC_OK) return rc;
    rc = body();
    const int rc2 = mark_internal_buffers(c, st);  // also after a failure: part of the work may have been enqueued
    return rc != FASTECC_OK ? rc : rc2;
}
// The k-block work stripe of a fold > 0 / multi-coset context (allocated on first use); a caller may build its input
// there and pass it as `data` to fastecc_encode, which then runs the DIF half in place.
int scratch_of(fastecc_ctx* c, uint32_t** out);
// GF((2^61-1)^2) codes other than (2N,N) work on padded copies of the caller's stripes: the context's two N-block work stripes
int p61_work_stripes(fastecc_ctx* c, uint64_t** data_full, uint64_t** parity_full);

// `count` stripes back to back (a pool): bytes per block, per data stripe and per parity stripe.  FASTECC_E_INVAL when count is 0, when the pool's
// byte extent overflows 64 bits, or (wraps) when either pointer plus its extent wraps; a null `data` has nothing to wrap (fastecc_update_parity_batch
// has no data pool).  wraps = false: the caller of a list form has already checked the pool.  *out is filled either way.
struct PoolExtent {
    uint64_t block, data_bytes, parity_bytes;
};
inline int pool_extent(const fastecc_ctx* c, const void* data, const void* parity, uint64_t count, PoolExtent* out, bool wraps = true)
{
    const uint64_t block = c->S * 4, data_bytes = c->K * block, parity_bytes = c->Mu * block;
    *out = PoolExtent{block, data_bytes, parity_bytes};
    if (count == 0 || count > UINT64_MAX / data_bytes || count > UINT64_MAX / parity_bytes) return FASTECC_E_INVAL;
    if (!wraps) return FASTECC_OK;
    if ((uint64_t)(uintptr_t)data > UINT64_MAX - count * data_bytes || (uint64_t)(uintptr_t)parity > UINT64_MAX - count * parity_bytes) return FASTECC_E_INVAL;
    return FASTECC_OK;
}

// ---- decode.hip, for the scrubber (fastecc_correct_batch) ----
// fastecc_repair_batch's work on the `count` stripes list[0 .. count) of a pool of back-to-back stripes, with the prepared pattern.  The list is
// given twice: on the host (the stripe-by-stripe forms) and on the device (the batched launch).  The caller has checked the pool's pointers and
// extent; takes the context's call lock itself.
int repair_list(fastecc_ctx* c, void* data, void* parity, const uint64_t* host_list, const uint64_t* dev_list, uint64_t count, void* stream);
// ---- pattern_set.hip, for the scrubber ----
// What a pattern set takes (fastecc_decode_prepare_set, and the private set below)
constexpr uint64_t SET_MAX_PATTERNS = 4096;
constexpr size_t SET_MAX_LOST = 16;  // one direct pass of a single sweep: pad <= 16
// fastecc_repair_batch_set's work through a pattern set PRIVATE to the call (fastecc_correct_batch_set): stripe stripes[i] of the
// pool loses exactly the blocks lost_sets[set_of[i]] (codeword indices; at most 16 per set, at most 4096 sets).  One direct_set_kernel launch per size
// class, as for the context's own set, which is neither read nor changed.  The caller has checked the pool's pointers and extent; takes the context's
// call lock itself and returns only when the stream's work is done and the private set is freed.
int repair_lost_sets(fastecc_ctx* c, void* data, void* parity, const std::vector<std::vector<uint32_t>>& lost_sets, const std::vector<uint64_t>& stripes,
                     const std::vector<uint32_t>& set_of, void* stream);
// ---- pattern_set.hip, for the degraded writes (update.hip: fastecc_update_batch_set) ----
// What a write under the context's pattern set (fastecc_decode_prepare_set) needs of it; PatternSet itself stays private to the decoder's files
// (decode_state.hpp).  The caller
// holds c->mu, and everything is valid until the lock is released (a later fastecc_decode_prepare_set waits for the enqueued work: wait_idle).
constexpr int SET_LOST_ROW = (int)SET_MAX_LOST + 1;  // words per pattern of lost_parity: its lost parity blocks, increasing, then SET_LOST_END to the end
constexpr uint32_t SET_LOST_END = 0xFFFFFFFFu;       // (a pattern loses at most SET_MAX_LOST blocks: every row ends with at least one)
struct PatternSetView {
    uint64_t patterns;            // P
    const DirectSetPass* passes;  // device: the descriptor table of direct_run_read, entry q = pattern q's pass
    const uint32_t* lost_parity;  // device: P + 1 rows of SET_LOST_ROW words; row P loses nothing (a whole stripe)
    const uint32_t* lost_data;    // device: P rows of DIRECT_READ_LOST_ROW words, row q = pattern q's lost data blocks in the order of its pass's
                                  // outputs (DirectReadEntry::out), then SET_LOST_END to the end — what the device-list forms scan (section 41)
};
bool pattern_set_view(const fastecc_ctx* c, PatternSetView* out);  // false: no set prepared
// pattern q < P of that set: its lost data blocks in the order of its pass's outputs (DirectReadEntry::out), its lost parity blocks (increasing),
// the rows its pass reads
const std::vector<uint32_t>& pattern_lost_data(const fastecc_ctx* c, uint64_t q);
const std::vector<uint32_t>& pattern_lost_parity(const fastecc_ctx* c, uint64_t q);
uint32_t pattern_rows(const fastecc_ctx* c, uint64_t q);
// ---- host_stage.hip: stripes in host memory ----
// PAGEABLE host memory (what RS.cpp's malloc'ed buffers are) <-> device.  The runtime's own pageable download stages through pinned memory
// with one copying host thread: 2 GiB took 89 ms (24 GB/s) on a link that moves them in 37 ms.  Here a ring of pinned slots sits between the
// two: the copy engine fills (or empties) a slot with one hipMemcpy2DAsync on `st`, an event per slot, and a few helper threads move the
// slot's rows from / to the caller's buffer side by side; a slot is reused once all of them (download) or the copy engine (upload) are done
// with it.  The transfer is a `rows x width` rectangle on both sides (pitches may differ: a column slab of a stripe), packed in the slots.
// Synchronous on the host: returns when the caller's memory is complete (download) or every copy is on the stream (upload).  Any failure to
// set this up — no pinned memory, no threads — falls back to the plain copy.
struct StageJob {
    bool to_device;
    char* host;           // pageable
    size_t host_pitch;
    char* dev;
    size_t dev_pitch;
    size_t width, rows;   // bytes per row, rows
    void* const* host_rows = nullptr;  // optional: row r lives at host_rows[r] (host, host_pitch unused): the reference's T** block table
};
int stage_transfer(fastecc_ctx* c, const StageJob& j, hipStream_t st, int threads = 0);
int stage_download(fastecc_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t st);
int ensure_dbuf(fastecc_ctx* c);
int encode_host_pinned(fastecc_ctx* c, const uint32_t* data, uint32_t* parity, hipStream_t st);
int encode_host_pageable(fastecc_ctx* c, const uint32_t* data, uint32_t* parity, hipStream_t st);

// ---- create.hip ----
int create_impl(fastecc_ctx** out, uint64_t n, uint64_t k, int lg, uint64_t block_bytes, int field, int device, int fold, int cosets,
                const uint32_t* custom_factor);
extern const uint32_t* const NTT_ONLY;  // custom_factor value: see create_ntt_ctx
int setup_mixed(fastecc_ctx* c, int q, uint64_t k_user, uint64_t m_user, const uint32_t* custom_factor = nullptr);
// the code geometry fastecc_create / fastecc_create_ex choose (also read by fastecc_code_coefficient, update.hip)
int pow2_code_shape(uint64_t n, uint64_t k, int* lg, int* fold, int* cosets);
uint64_t mixed_radix_order(uint64_t k, unsigned flags, int* q, int* m);

}  // namespace fastecc
