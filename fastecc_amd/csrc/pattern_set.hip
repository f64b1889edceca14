// pattern_set.hip — a pattern per stripe (fastecc_decode_prepare_set and the calls under it), the set's two other clients (the scrubber's private set,
// the view for degraded writes) and degraded reads.  Every pass here is one of direct.hip's; the tables come from decode_prepare.hip (direct_tables).
#include <algorithm>
#include <new>
#include <vector>

#include "decode_state.hpp"

namespace fastecc {

void destroy_pattern_set(PatternSet* s) { delete s; }

namespace {

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
    // the lost parity blocks (P + 1 rows of SET_LOST_ROW words), then the lost data blocks (P rows of DIRECT_READ_LOST_ROW words): one buffer, one upload
    static_assert(DIRECT_READ_LOST_ROW == SET_MAX_LOST, "a row of the read table holds a pattern's lost data blocks");
    const size_t lost_data_at = (P + 1) * SET_LOST_ROW;
    std::vector<uint32_t> lost_rows(lost_data_at + P * DIRECT_READ_LOST_ROW, SET_LOST_END);
    const CodeGeometry geometry(c);
    PhaseTimer quiet;  // one line per set, not two per pattern
    quiet.on = false;
    for (uint64_t q = 0; q < P; q++) {
        const LostLists& l = lists[q];
        if (l.R.empty() && l.Pl.empty()) continue;  // nothing lost: its stripes are not touched
        int rc = direct_tables(geometry, l.R, l.Pl, l.A, fresh->tables[q], quiet);
        if (rc != FASTECC_OK) return rc;
        fresh->kind[q] = !l.R.empty() && !l.Pl.empty() ? PatternSet::BOTH : !l.R.empty() ? PatternSet::DATA : PatternSet::PARITY;
        if ((rc = direct_set_describe(fresh->pass(q), &desc[q])) != FASTECC_OK) return rc;
        while ((1u << fresh->cls[q]) < desc[q].cstride) fresh->cls[q]++;
        fresh->rows[q] = desc[q].rows;
        fresh->rows_max = std::max(fresh->rows_max, desc[q].rows);
        fresh->lost_data[q] = l.R;
        std::copy(l.R.begin(), l.R.end(), lost_rows.begin() + lost_data_at + q * DIRECT_READ_LOST_ROW);  // (at most SET_MAX_LOST)
        fresh->lost_parity[q] = l.Pl;
        std::sort(fresh->lost_parity[q].begin(), fresh->lost_parity[q].end());
        std::copy(fresh->lost_parity[q].begin(), fresh->lost_parity[q].end(), lost_rows.begin() + q * SET_LOST_ROW);  // (at most SET_MAX_LOST < SET_LOST_ROW)
    }
    RC_TRY(fresh->d_passes.alloc(P));
    HIP_TRY(hipMemcpy(fresh->d_passes, desc.data(), P * sizeof(DirectSetPass), hipMemcpyHostToDevice));
    RC_TRY(fresh->d_lost_parity.alloc(lost_rows.size()));
    HIP_TRY(hipMemcpy(fresh->d_lost_parity, lost_rows.data(), lost_rows.size() * 4, hipMemcpyHostToDevice));
    fresh->d_lost_data = fresh->d_lost_parity.get() + lost_data_at;
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

// ---- fastecc_read_batch / _read_batch_set and their device-list forms: degraded reads ----
// The tables a read call works under: the set, or the single pattern's pass for the lost data
struct ReadTables {
    PatternSet* s = nullptr;
    DecodeState* d = nullptr;
    DirectPass* single = nullptr;  // (null: the single pattern lost no data block — every request is a copy)
};

// What the host decides without looking at the request list, for the host-list and the device-list forms alike (`reads` is tested for null only):
// the arguments, the context's kind — from there on under the call lock, which `lk` holds when this returns FASTECC_OK —, the window, the pool's
// extent, `out` against the pool, and the prepared set or pattern.
int read_batch_checks(fastecc_ctx* c, const void* data, const void* parity, uint64_t count, const uint32_t* pattern_of, bool set_form, const uint64_t* reads,
                      uint64_t n_reads, uint64_t col0, uint64_t width, const void* out, std::unique_lock<std::mutex>& lk, ReadTables* tables)
{
    if (!c || count == 0 || width == 0 || (set_form && !pattern_of)) return FASTECC_E_INVAL;
    if (n_reads > 0 && (!data || !parity || !reads || !out)) return FASTECC_E_INVAL;
    if (((uintptr_t)data | (uintptr_t)parity | (uintptr_t)out) & 3u) return FASTECC_E_INVAL;
    if (c->sharded) return FASTECC_E_UNSUPPORTED;
    lk = std::unique_lock<std::mutex>(c->mu);
    if (c->field != FASTECC_FIELD_GF_FFF00001) return FASTECC_E_UNSUPPORTED;
    if (c->ld != c->S) return FASTECC_E_UNSUPPORTED;  // stripes of a pool are contiguous
    const uint64_t S = c->S;
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
    PatternSet*& s = tables->s;
    DecodeState*& d = tables->d;
    DirectPass*& single = tables->single;
    if (set_form) {
        if (!(s = c->pattern_set)) return FASTECC_E_INVAL;  // fastecc_decode_prepare_set first
    } else {
        d = c->decoder;
        if (!d || !d->pattern.ready) return FASTECC_E_INVAL;  // fastecc_decode_prepare first
        // a pattern of the transform path is not served — but a pattern that lost NOTHING has no tables on either path (Prepare::direct leaves it to
        // transform_path, which finds nothing to build): it has no lost data block, so every request is a copy.  (The locator's root count is no
        // measure of that: on the transform path it also counts the positions of a folded or zero-extended code that hold no block.)
        if (!d->pattern.direct_path && (d->pattern.erased_data != 0 || d->pattern.erased_parity != 0)) return FASTECC_E_UNSUPPORTED;
        if (d->pattern.direct_path && d->few.direct.ed > 0) {
            single = d->few.direct.both_built && d->few.direct.only_both ? d->few.direct.both.get() : d->few.direct.data.get();
            if (!single || d->host.lost_data.size() != (size_t)d->few.direct.ed) return FASTECC_E_DEVICE;
        }
    }
    return FASTECC_OK;
}

// The single pattern's descriptor table on the device, uploaded once per prepared pattern.  (No read that used the previous one is in flight:
// fastecc_decode_prepare waited for them before it rebuilt the tables.)
int single_read_desc(DecodeState* d, DirectPass* single, const DirectSetPass** passes)
{
    if (single && d->few.read_desc_of != d->pattern.serial) {
        DirectSetPass desc;
        RC_TRY(direct_read_describe(single, &desc));
        RC_TRY(d->few.read_desc.alloc(1));
        HIP_TRY(hipMemcpy(d->few.read_desc, &desc, sizeof(desc), hipMemcpyHostToDevice));
        d->few.read_desc_of = d->pattern.serial;
    }
    RC_TRY(d->few.read_desc.alloc(1));  // (a pattern that lost no data: the table is never read, but the launch takes a pointer)
    *passes = d->few.read_desc.get();
    return FASTECC_OK;
}

// The requested data blocks reads[0 .. n_reads) of a pool, words [col0, col0 + width) of each, into row u of `out`; the pool is only read.
// set_form: stripe b under pattern pattern_of[b] of the prepared set; else every stripe under the single prepared pattern (direct path only).
// read_batch_checks, then every request on the host — (stripe, pattern, present or the block's output index in the pass that
// fastecc_decode_batch[_set] takes for the lost data) — and only when all of them are valid ONE launch of direct_read_kernel over the staged list.
int read_batch_impl(fastecc_ctx* c, const void* data, const void* parity, uint64_t count, const uint32_t* pattern_of, bool set_form, const uint64_t* reads,
                    uint64_t n_reads, uint64_t col0, uint64_t width, void* out, void* stream)
{
    std::unique_lock<std::mutex> lk;
    ReadTables tables;
    RC_TRY(read_batch_checks(c, data, parity, count, pattern_of, set_form, reads, n_reads, col0, width, out, lk, &tables));
    PatternSet* const s = tables.s;
    DecodeState* const d = tables.d;
    DirectPass* const single = tables.single;
    if (n_reads == 0) return FASTECC_OK;
    const uint64_t S = c->S, K = c->K;
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
            const std::vector<uint32_t>& R = d->host.lost_data;  // increasing (Prepare::direct)
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
    if (!set_form) RC_TRY(single_read_desc(d, single, &passes));
    return with_internal_buffers(c, st, [&]() -> int {  // the tables and the list are internal buffers
        RC_TRY(list.publish(n_reads, st));
        ProfScope ps(c, st, set_form ? "direct_read_set" : "direct_read", rows_total * width * 4u);
        return direct_run_read(passes, list.dev, n_reads, ddata, dparity, (uint32_t*)out, S, col0, width, K * S, c->Mu * S, st);
    });
}

// fastecc_read_batch_device / _read_batch_set_device: read_batch_impl with `reads`, `pattern_of` (set form) and `status` in
// DEVICE memory, never dereferenced here.  What the host decides without the lists, then on the stream: *status = 0, read_translate_kernel into the
// context's own entry list (not read_list.dev, which the degraded writes use too) and direct_read_device_kernel over it.  A steady-state call
// allocates nothing, copies nothing and waits for nothing; the entry list grows behind the host-side wait for the kernels that read it, and the
// single pattern's two small tables are uploaded once per prepared pattern.
constexpr uint64_t READ_DEVICE_MAX = 1ull << 24;  // requests of one list: the row field of the status word is 32 bits, a launch holds 2^24 waves

int read_batch_device_impl(fastecc_ctx* c, const void* data, const void* parity, uint64_t count, const uint32_t* pattern_of, bool set_form,
                           const uint64_t* reads, uint64_t n_reads, uint64_t col0, uint64_t width, void* out, uint64_t* status, void* stream)
{
    if (!c || !status) return FASTECC_E_INVAL;
    if ((((uintptr_t)reads | (uintptr_t)status) & 7u) != 0 || (set_form && ((uintptr_t)pattern_of & 3u) != 0)) return FASTECC_E_INVAL;
    if (n_reads > READ_DEVICE_MAX) return FASTECC_E_UNSUPPORTED;
    std::unique_lock<std::mutex> lk;
    ReadTables tables;
    RC_TRY(read_batch_checks(c, data, parity, count, pattern_of, set_form, reads, n_reads, col0, width, out, lk, &tables));
    // the lists and the status word against `out`, the status word against the lists (count * 4 and n_reads * width * 4 fit: read_batch_checks)
    const auto hits = [](const void* p, uint64_t pbytes, const void* q, uint64_t qbytes) {
        const uint64_t p0 = (uint64_t)(uintptr_t)p, q0 = (uint64_t)(uintptr_t)q;
        return p && q && pbytes && qbytes && p0 < q0 + qbytes && q0 < p0 + pbytes;
    };
    const uint64_t out_bytes = n_reads * width * 4u, reads_bytes = n_reads * 8u, pattern_bytes = set_form ? count * 4u : 0;
    if (hits(reads, reads_bytes, out, out_bytes) || hits(pattern_of, pattern_bytes, out, out_bytes) || hits(status, 8, out, out_bytes) ||
        hits(status, 8, reads, reads_bytes) || hits(status, 8, pattern_of, pattern_bytes))
        return FASTECC_E_INVAL;
    const uint64_t S = c->S, K = c->K;
    if (n_reads > 0 && direct_read_waves_per_entry(data, parity, out, S, col0, width) > (1ull << 24)) return FASTECC_E_UNSUPPORTED;
    DeviceGuard dg(c->device);
    if (!dg.ok) return FASTECC_E_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    if (n_reads == 0) {
        HIP_TRY(hipMemsetAsync(status, 0, 8, st));
        return FASTECC_OK;
    }
    ReadTranslate t{};
    t.reads = reads;
    t.pattern_of = set_form ? pattern_of : nullptr;
    t.status = status;
    t.n = n_reads;
    t.blocks = count * K;  // (fits: pool_extent)
    t.K = K;
    const DirectSetPass* passes = nullptr;
    uint64_t rows_max = 0;
    if (set_form) {
        PatternSet* s = tables.s;
        passes = s->d_passes.get();
        t.lost = s->d_lost_data;
        t.patterns = (uint32_t)s->tables.size();
        rows_max = s->rows_max;
    } else {
        DecodeState* d = tables.d;
        RC_TRY(single_read_desc(d, tables.single, &passes));
        if (tables.single) {
            const std::vector<uint32_t>& R = d->host.lost_data;  // increasing (Prepare::direct)
            if (d->few.read_lost_of != d->pattern.serial) {  // (as for the descriptor: no read under the previous pattern is in flight)
                RC_TRY(d->few.read_lost.alloc((uint64_t)direct_cap()));
                if (R.size() > d->few.read_lost.capacity()) return FASTECC_E_DEVICE;
                HIP_TRY(hipMemcpy(d->few.read_lost, R.data(), R.size() * 4, hipMemcpyHostToDevice));
                d->few.read_lost_of = d->pattern.serial;
            }
            t.lost = d->few.read_lost.get();
            t.n_lost = (uint32_t)R.size();
            rows_max = (uint64_t)direct_pass_rows(tables.single);
        }
    }
    if (n_reads > c->read_entries.capacity()) {
        RC_TRY(wait_idle(c));  // the kernels that read the list about to be replaced
        RC_TRY(c->read_entries.grow(std::max<uint64_t>(std::max<uint64_t>(n_reads, 2 * c->read_entries.capacity()), 4096)));
    }
    t.entries = c->read_entries.get();
    return with_internal_buffers(c, st, [&]() -> int {  // the tables and the entry list are internal buffers
        HIP_TRY(hipMemsetAsync(status, 0, 8, st));
        {
            ProfScope ps(c, st, "direct_read_device_translate", n_reads * (8 + sizeof(DirectReadEntry) + (set_form ? 4 : 0)));
            RC_TRY(direct_run_read_translate(t, st));
        }
        // (the bytes: a BOUND, every request taken for a lost block of the pattern with the most rows — what the requests are is known on the device only)
        ProfScope ps(c, st, set_form ? "direct_read_device_set" : "direct_read_device", n_reads * (rows_max + 1) * width * 4u);
        return direct_run_read_device(passes, t.entries, n_reads, (const uint32_t*)data, (const uint32_t*)parity, (uint32_t*)out, S, col0, width, K * S,
                                      c->Mu * S, status, st);
    });
}

}  // namespace

// The context's pattern set as the degraded writes see it (drivers.hpp; update.hip)
bool pattern_set_view(const fastecc_ctx* c, PatternSetView* out)
{
    const PatternSet* s = c->pattern_set;
    if (!s) return false;
    *out = PatternSetView{s->tables.size(), s->d_passes.get(), s->d_lost_parity.get(), s->d_lost_data};
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

}  // namespace fastecc

using namespace fastecc;

extern "C" {

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

int fastecc_read_batch_set_device(fastecc_ctx* c, const void* data, const void* parity, uint64_t count, const uint32_t* pattern_of, const uint64_t* reads,
                                  uint64_t n_reads, uint64_t col0_words, uint64_t width_words, void* out, uint64_t* status, void* stream)
{
    return guarded(
        [&]() -> int { return read_batch_device_impl(c, data, parity, count, pattern_of, true, reads, n_reads, col0_words, width_words, out, status, stream); });
}

int fastecc_read_batch_device(fastecc_ctx* c, const void* data, const void* parity, uint64_t count, const uint64_t* reads, uint64_t n_reads,
                              uint64_t col0_words, uint64_t width_words, void* out, uint64_t* status, void* stream)
{
    return guarded(
        [&]() -> int { return read_batch_device_impl(c, data, parity, count, nullptr, false, reads, n_reads, col0_words, width_words, out, status, stream); });
}

}  // extern "C"
