// scrub.hip — error detection and location: fastecc_verify, fastecc_locate_errors, fastecc_correct, their batched, list and per-stripe-pattern forms
// and degraded scrubbing (include/fastecc.h).  The kernels are in scrub_device.hpp.
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
// part that scales with the stripe; the rest works on NC x 4 words.
//
// The stages, in the order of this file:
//   state        per context (scrub_state): geometry, position map, w^u, the fixed erasures' locator; the blocks named absent — one pattern
//                (set_erasures) or a set with a pattern per stripe (set_erasures_set, section 19) — seen through Erasures: the
//                fingerprint kernels skip them, their locator joins the fixed erasures', w fewer syndromes are checked.  Buffers only grow (DeviceBuf::grow).
//   one stripe   locate: fingerprints (one wave per block, dwordx4 loads; a block with a word >= p is certainly corrupt: a known erasure), syndromes
//                (F times the erasures' locator, the stand-alone inverse transform of NC points, every coefficient above the degree bound checked
//                for zero and the first 2 locate_max of each column gathered), Berlekamp-Massey on the host per column and the longest LFSR as the
//                locator Lambda(x) = prod (1 - X_u x) (longest_lfsr), Lambda(w^u) by Horner at every position on the device, the roots' blocks
//                (accept_root), and the confirmation: the syndromes once more with the located positions erased must all vanish, in every column.
//   chunk pass   many stripes (section 14): the stripe index becomes extra word columns of the fingerprint stripe, so one transform serves a whole
//                chunk of stripes.  chunk_pass runs one chunk — fingerprints, transform, syndrome launch — in the form a ChunkForm names, for
//                verify_batch_locked (the stripes of a batch), verify_list_locked and LocateList (a LIST of stripes of the pool, section 17),
//                verify_batch_set_locked (a pattern per stripe) and LocateList under the set (a list, a pattern per entry: section 27).  A pass that
//                fails part-way waits for what it enqueued (settled).
//   location     LocateList, per chunk of the flagged stripes: gather_chunk (all syndromes at once), solve_chunk (Berlekamp-Massey and the recurrence
//                check per stripe on the host), search_chunk (one root search for all locators), accept_chunk.
//   pool calls   StripePatterns holds what the single-pattern and the per-stripe-pattern form of a pool call differ in (section 30): the form's own
//                argument check, its verify pass, the erasure view and the absent blocks of a stripe, the room in the call-private pattern set.  Written
//                once on top of it: flagged (the verify pass's inconsistent stripes), locate_list (LocateList over those of them the batched pass takes),
//                verify_pool_impl, locate_pool_impl and CorrectPool.
//   correction   correct_stripe: locate, fastecc_decode_prepare + fastecc_repair of the located and the absent blocks, the closing verify.
//                CorrectPool: flag_and_locate, group_by_lost_set, repair_groups (the lost sets of at most 16 blocks through ONE pattern set private to
//                the call, pattern_set.hip repair_lost_sets, where the form has one: section 27; every other distinct lost set one prepare and one list-form
//                repair, decode.hip repair_list), closing_verify, fallbacks (correct_stripe on what the grouped path does not take).
//   entry points argument checks, then the stage inside on_device.
#include <algorithm>
#include <map>
#include <memory>
#include <vector>

#include "devmem.hpp"
#include "drivers.hpp"
#include "scrub_device.hpp"

namespace fastecc {

namespace {

uint64_t splitmix64(uint64_t& s)
{
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

}  // namespace

// fastecc_scrub_erasures_set: P patterns of absent blocks, their tables side by side
struct ScrubSet {
    uint64_t P = 0;
    std::vector<std::vector<uint32_t>> absent;    // per pattern: the absent blocks' codeword indices, increasing
    std::vector<std::vector<uint8_t>> is_absent;  // per pattern: n flags
    std::vector<uint32_t> mlo;                    // per pattern: N + fixed + w, the first coefficient that must vanish
    uint32_t mlo_min = 0;
    DeviceBuf<uint32_t> d_pos;                    // P x n words: d_pos with ABSENT set at the pattern's absent blocks
    DeviceBuf<uint32_t> d_l;                      // P x NC words: d_lfix (or 1) times the locator of the pattern's absent positions at w^u
    DeviceBuf<uint32_t> d_mlo;                    // P words: mlo
};

struct ScrubState {
    uint64_t N = 0, NC = 0, n = 0, k = 0;  // transform length of the code, positions, blocks (user k + user m), data blocks
    int lgc = 0;
    uint64_t fixed = 0;                     // positions that hold no block (fixed erasures)
    std::vector<uint32_t> pos;              // block -> position
    std::vector<uint32_t> block_at;         // position -> block, ~0u if none (fixed erasure or known-zero data block)
    CtxPtr ntt;                             // stand-alone transform of NC points, 4 words per position
    DeviceBuf<uint32_t> d_pos;              // n words
    DeviceBuf<uint32_t> d_wpow;             // NC words: w^u
    DeviceBuf<uint32_t> d_lfix;             // NC words: the fixed erasures' locator at w^u (null: none)
    DeviceBuf<uint32_t> d_F;                // NC x 4 words: fingerprints by position (zero where no block is read)
    DeviceBuf<uint32_t> d_G;                // NC x 4 words: weighted fingerprints, transformed in place
    DeviceBuf<uint32_t> d_small;            // counters and lists: [bad: 1 + n], [flag: 1], [found: 1 + cap_found], syndromes, lambda, roots
    DeviceBuf<uint2> d_weights;             // S packed weights of the current seed
    uint64_t weights_seed = 0;
    bool weights_valid = false;
    // fastecc_verify_batch (built at its first call): a chunk of up to batch_cap stripes as word columns of one fingerprint stripe
    CtxPtr ntt_batch;                       // stand-alone transform of NC points over rows of 4 x batch_cap words
    uint64_t batch_cap = 0;
    DeviceBuf<uint32_t> d_FB;               // NC x 4 batch_cap words: weighted fingerprints by position (zero where no block is read)
    DeviceBuf<uint32_t> d_GB;               // their transform
    DeviceBuf<uint8_t> d_flag;              // one byte per stripe of the call: 1 = inconsistent
    // fastecc_scrub_erasures: the blocks the caller named absent (none: empty / null)
    std::vector<uint32_t> absent;           // their codeword indices, increasing
    std::vector<uint8_t> is_absent;         // n flags
    DeviceBuf<uint32_t> d_pos_named;        // n words: d_pos with ABSENT set at those blocks
    DeviceBuf<uint32_t> d_lnamed;           // NC words: d_lfix (or 1) times the locator of their positions at w^u
    // batched location and the list forms, all grow-only
    DeviceBuf<uint64_t> d_list;             // the stripes a list pass runs over
    DeviceBuf<uint8_t> d_lflag;             // per list entry: [0, lflag_cap) inconsistent, [lflag_cap, 2 lflag_cap) a present block held a word >= p
    uint64_t lflag_cap() const { return d_lflag.capacity() / 2; }  // (grows with d_list)
    DeviceBuf<uint32_t> d_loc;              // one chunk's syndromes, then its locators, their lengths and the found lists
    // fastecc_scrub_erasures_set: the pattern set (null: none) and the device copy of a call's pattern_of (grow-only)
    std::unique_ptr<ScrubSet> set;
    DeviceBuf<uint32_t> d_pattern_of;
};

void destroy_scrub_state(ScrubState* s) { delete s; }

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
    const ScrubSet* t = s->set.get();
    const uint64_t w = t->absent[q].size();
    return {t->d_pos + (uint64_t)q * s->n, t->d_l + (uint64_t)q * s->NC, w, w ? &t->absent[q] : nullptr, w ? &t->is_absent[q] : nullptr};
}

// the fingerprint kernels' vector form: whole dwordx4 loads, 16-byte aligned stripes
bool vec_form(const fastecc_ctx* c, const void* data, const void* parity)
{
    return (c->S % 4) == 0 && (((uintptr_t)data | (uintptr_t)parity) & 15u) == 0;
}

// a fingerprint kernel in its vector (kv) or scalar (ks) form over `groups` workgroups of four waves
template <class... K, class... A> void launch_fp(void (*kv)(K...), void (*ks)(K...), bool vec, uint64_t groups, hipStream_t st, const A&... args)
{
    hipLaunchKernelGGL(vec ? kv : ks, dim3((unsigned)groups), dim3(256), 0, st, args...);
}

// the frame of an entry point whose arguments are checked: the context's device current, exceptions turned into return codes (a body that touches the
// scrub state takes the call lock first)
template <class F> int on_device(fastecc_ctx* c, F body)
{
    DeviceGuard dg(c->device);
    if (!dg.ok) return FASTECC_E_DEVICE;
    return guarded(body);
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

// The context's geometry, position map, w^u table and fixed-erasure locator (synchronous).
int build_scrub_state(fastecc_ctx* c, ScrubState* s)
{
    int e = 1;
    while ((1 << e) < c->cosets + 1) e++;
    s->N = c->N;
    s->NC = c->N << e;
    s->lgc = c->n + e;
    s->k = c->K;
    s->n = c->K + c->Mu;
    if (s->NC > (1ull << 20) || s->NC < 4) return FASTECC_E_UNSUPPORTED;
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
    if (s->N + s->fixed + (s->n - s->k) != s->NC) return FASTECC_E_DEVICE;  // (the layout is inconsistent: cannot happen)

    RC_TRY(create_ntt_ctx(s->ntt.fill(), s->lgc, 4 * RW, c->device));
    const uint64_t NC = s->NC;
    auto grid = [](uint64_t items) { return dim3((unsigned)((items + 255) / 256)); };
    RC_TRY(s->d_pos.alloc(s->n));
    RC_TRY(s->d_wpow.alloc(NC));
    RC_TRY(s->d_F.alloc(NC * RW));
    RC_TRY(s->d_G.alloc(NC * RW));
    HIP_TRY(hipMemcpy(s->d_pos, s->pos.data(), s->n * 4, hipMemcpyHostToDevice));
    // positions no block is read from (fixed erasures, known-zero data blocks) keep fingerprint 0 for good
    HIP_TRY(hipMemset(s->d_F, 0, NC * RW * 4));
    hipLaunchKernelGGL(powers_kernel, grid(NC), dim3(256), 0, nullptr, s->d_wpow, w, (uint32_t)NC);
    HIP_TRY(hipGetLastError());
    if (!fixed_roots.empty()) {
        DeviceBuf<uint32_t> d_roots;
        RC_TRY(s->d_lfix.alloc(NC));
        RC_TRY(d_roots.alloc(fixed_roots.size()));
        HIP_TRY(hipMemcpy(d_roots, fixed_roots.data(), fixed_roots.size() * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(locator_kernel<false>, grid(NC), dim3(256), 0, nullptr, nullptr, d_roots, (uint32_t)fixed_roots.size(), s->d_wpow,
                           (uint32_t)NC, nullptr, s->d_lfix);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());  // (d_roots goes here)
    }
    HIP_TRY(hipDeviceSynchronize());
    return FASTECC_OK;
}

// ... once per context; a failed build leaves none and is retried from scratch
int scrub_state(fastecc_ctx* c, ScrubState** out)
{
    if (!c->scrub) {
        std::unique_ptr<ScrubState> s(new (std::nothrow) ScrubState());
        if (!s) return FASTECC_E_NOMEM;
        const int rc = build_scrub_state(c, s.get());
        if (rc != FASTECC_OK) return rc;
        c->scrub = s.release();
    }
    *out = c->scrub;
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
    const int rc = s->d_small.grow(words);
    if (rc != FASTECC_OK) return rc;
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
    RC_TRY(s->d_weights.alloc(c->S + 2));  // (16 bytes past the last weight)
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
    // every workgroup resident at once (6 waves per SIMD; its 72 VGPRs would fit a seventh): a grid-stride loop over the blocks without a tail wave of late groups
    const uint64_t groups = std::min<uint64_t>((s->n + 3) / 4, (uint64_t)c->cus * 6);
    {
        ProfScope ps(c, st, "fingerprint", (s->n - er.w) * c->S * 4);
        launch_fp(fingerprint_kernel<true>, fingerprint_kernel<false>, vec_form(c, data, parity), groups, st, data, parity, (uint32_t)s->k, (uint32_t)s->n,
                  (uint32_t)c->S, s->d_weights, er.d_pos, s->d_F, sm.bad, (uint32_t)sm.bad_cap);
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

// The decisions of location, shared by one stripe (locate) and the list form (LocateList).  The locator of a stripe's syndromes — `gather` per column,
// column c at syn + c * column_stride: the longest of the columns' LFSRs, the first column on ties (a column may miss an error with probability
// <= 2^-20; the caller's confirmation covers all).  Returns its length L with lambda[0 .. L], or 0 where location refuses: no LFSR, more than tmax
// errors, or fewer than 2L syndromes.  cand: scratch (a caller with many stripes keeps it).
int longest_lfsr(const uint32_t* syn, uint64_t column_stride, uint64_t gather, uint64_t tmax, std::vector<uint32_t>& lambda, std::vector<uint32_t>& cand)
{
    int L = 0;
    for (int col = 0; col < R; col++) {
        const int Lc = berlekamp_massey(syn + col * column_stride, (uint32_t)gather, cand);
        if (Lc > L) {
            L = Lc;
            lambda = cand;
        }
    }
    return (L == 0 || (uint64_t)L > tmax || 2ull * (uint64_t)L > gather) ? 0 : L;
}

// The locator's root at position u names the block there: appended to `blocks`, or false where no block is there or the block is already erased —
// named absent by `er`, or one of `bad` (sorted; null: none)
bool accept_root(uint32_t u, const std::vector<uint32_t>& block_at, const Erasures& er, const std::vector<uint32_t>* bad, std::vector<uint32_t>& blocks)
{
    const uint32_t j = block_at[u];
    if (j == ~0u || (bad && std::binary_search(bad->begin(), bad->end(), j)) || (er.w && (*er.is_absent)[j])) return false;
    blocks.push_back(j);
    return true;
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
        std::vector<uint32_t> lambda, cand;
        const int L = longest_lfsr(syn.data(), gather, gather, tmax, lambda, cand);
        if (L == 0) return FASTECC_E_UNCORRECTABLE;
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
            if (!accept_root(u, s->block_at, er, &bad, result)) return FASTECC_E_UNCORRECTABLE;
            erased.push_back(u);
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
    PoolExtent x;
    return pool_extent(c, data, parity, count, &x);
}

// The chunk buffers (once per context): the largest power-of-two chunk whose fingerprint stripe holds at most 32 MiB with rows of at most 1 MiB.
// The chunk does not depend on the call's count, so one transform context serves every call.  F is zeroed here once: the positions that hold
// no block are the same for every stripe, and the transform reads F and writes G, so they stay zero.
int batch_state(fastecc_ctx* c, ScrubState* s)
{
    if (s->ntt_batch) return FASTECC_OK;
    uint64_t cap = 1;
    while (cap < (1ull << 16) && s->NC * 16 * (2 * cap) <= (32ull << 20)) cap *= 2;
    const uint64_t words = s->NC * RW * cap;
    CtxPtr t;
    DeviceBuf<uint32_t> F, G;
    RC_TRY(create_ntt_ctx(t.fill(), s->lgc, RW * 4 * cap, c->device));
    RC_TRY(F.alloc(words));
    RC_TRY(G.alloc(words));
    HIP_TRY(hipMemset(F, 0, words * 4));
    HIP_TRY(hipDeviceSynchronize());  // (the call's stream may not order after the null stream)
    s->ntt_batch = std::move(t);
    s->batch_cap = cap;
    s->d_FB = std::move(F);
    s->d_GB = std::move(G);
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
    if ((rc = s->d_flag.grow(count)) != FASTECC_OK) return rc;
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

uint64_t chunk_of(const fastecc_ctx* c, const ScrubState* s)
{
    return c->scrub_batch_chunk > 0 ? std::min<uint64_t>(s->batch_cap, (uint64_t)c->scrub_batch_chunk) : s->batch_cap;
}

// A batched pass that fails part-way waits for what it enqueued: the next call may free or overwrite the buffers its kernels read
template <class F> int settled(hipStream_t st, F pass)
{
    const int rc = pass();
    if (rc != FASTECC_OK) (void)hipStreamSynchronize(st);
    return rc;
}

// ---- the chunk pass: every batched verify and the batched location run their chunks through chunk_pass, in the form a ChunkForm names ----
// Fp, the fingerprint launch: BATCH stripes [b0, b0 + B) of the call under `er`, flags in d_flag; LIST entries [b0, b0 + B) of d_list under `er`, flags
// and big marks in d_lflag; SET stripes [b0, b0 + B) under d_pattern_of and the set's tables, flags in d_flag.  Syn, the syndrome launch: FLAGS a non-zero
// coefficient from m_lo on sets the entry's flag; GATHER all of them are copied to syn_out; SET they are checked from the stripe's own bound on.
// SET_LIST (section 27): LIST entries, each under the pattern d_pattern_of gives its stripe; GATHER_SET: each entry's coefficients from its own pattern's
// bound on are copied to syn_out, `stride` words per column.
enum class Fp { BATCH, LIST, SET, SET_LIST };
enum class Syn { FLAGS, GATHER, SET, GATHER_SET };
constexpr const char* FP_SCOPE[] = {"fingerprint_batch", "fingerprint_batch_list", "fingerprint_set", "fingerprint_set_list"};
constexpr const char* SYN_SCOPE[] = {"scrub_syndromes_batch", "scrub_syndromes_gather", "scrub_syndromes_set", "scrub_syndromes_gather_set"};

struct ChunkForm {
    Fp fp;
    Syn syn;
    uint64_t m_lo;         // the first coefficient the syndrome launch looks at
    bool check;            // some coefficient is left to check (else the chunk ends after its fingerprints: only the words >= p count)
    Erasures er;           // BATCH, LIST: the pattern
    uint32_t* syn_out;     // GATHER: device, B x R x (NC - m_lo) words; GATHER_SET: B x R x stride words
    uint64_t blocks_read;  // SET, SET_LIST: the blocks the chunk reads (the others read B (n - er.w))
    uint64_t stride = 0;   // GATHER_SET: words per column of syn_out
};

// One chunk of B entries from b0 on: the fingerprints (weighed by the erasures' locator as they are stored; absent blocks are not read and store
// zero), one transform of NC points over 4B word columns, the syndrome launch.  Nothing is copied back and nothing waits — unless `probe` is
// given (fastecc_scrub_fingerprints): then the chunk ends after its fingerprint launch with its fingerprints copied out (probe_chunk).
int chunk_pass(fastecc_ctx* c, ScrubState* s, const ChunkForm& f, const uint32_t* data, const uint32_t* parity, uint64_t b0, uint64_t B, hipStream_t st,
               const Probe* probe = nullptr)
{
    const ScrubSet* t = s->set.get();
    const uint64_t row = RW * s->batch_cap;
    const uint32_t k = (uint32_t)s->k, n = (uint32_t)s->n, S = (uint32_t)c->S, NC = (uint32_t)s->NC, m_lo = (uint32_t)f.m_lo;
    const bool vec = vec_form(c, data, parity), list = f.fp == Fp::LIST || f.fp == Fp::SET_LIST, per_stripe = f.fp == Fp::SET || f.fp == Fp::SET_LIST;
    // every workgroup resident at once, as for one stripe: six waves per SIMD, five for the list kernels
    const uint64_t groups = std::min<uint64_t>((B * n + 3) / 4, (uint64_t)c->cus * (list ? 5 : 6));
    uint8_t* flag = list ? s->d_lflag : s->d_flag;
    {
        ProfScope ps(c, st, FP_SCOPE[(int)f.fp], (per_stripe ? f.blocks_read : B * (n - f.er.w)) * S * 4);
        switch (f.fp) {
        case Fp::BATCH:
            launch_fp(fingerprint_batch_kernel<true>, fingerprint_batch_kernel<false>, vec, groups, st, data, parity, k, n, S, b0, B, s->d_weights, f.er.d_pos,
                      f.er.d_loc, s->d_FB, row, flag, nullptr, nullptr);
            break;
        case Fp::LIST:  // flags, list and big marks from the chunk's first entry on; b0 is not used
            launch_fp(fingerprint_batch_kernel<true, true>, fingerprint_batch_kernel<false, true>, vec, groups, st, data, parity, k, n, S, (uint64_t)0, B,
                      s->d_weights, f.er.d_pos, f.er.d_loc, s->d_FB, row, flag + b0, s->d_list + b0, flag + s->lflag_cap() + b0);
            break;
        case Fp::SET:
            launch_fp(fingerprint_set_kernel<true>, fingerprint_set_kernel<false>, vec, groups, st, data, parity, k, n, S, b0, B, s->d_weights, s->d_pattern_of,
                      t->d_pos, t->d_l, NC, s->d_FB, row, flag);
            break;
        case Fp::SET_LIST:  // as LIST; d_pattern_of is indexed by stripe
            launch_fp(fingerprint_set_list_kernel<true>, fingerprint_set_list_kernel<false>, vec, groups, st, data, parity, k, n, S, B, s->d_weights,
                      s->d_pattern_of, t->d_pos, t->d_l, NC, s->d_FB, row, flag + b0, s->d_list + b0, flag + s->lflag_cap() + b0);
            break;
        }
        HIP_TRY(hipGetLastError());
    }
    if (probe) return probe_chunk(s, B, st, probe->out + b0 * n * R);
    if (!f.check) return FASTECC_OK;
    {
        ProfScope ps(c, st, "scrub_transform_batch");
        const int rc = transform_bitrev(s->ntt_batch, s->d_FB, s->d_GB, false, true, (uint32_t)(RW * B), st);
        if (rc != FASTECC_OK) return rc;
    }
    {
        ProfScope ps(c, st, SYN_SCOPE[(int)f.syn]);
        const uint64_t items = (uint64_t)(NC - m_lo) * B;  // <= NC * batch_cap <= 2^21
        const dim3 grid((unsigned)((items + 255) / 256));
        switch (f.syn) {
        case Syn::FLAGS:
            hipLaunchKernelGGL(syndrome_batch_kernel, grid, dim3(256), 0, st, s->d_GB, s->lgc, NC, m_lo, row, (uint32_t)B, b0, flag);
            break;
        case Syn::GATHER:
            hipLaunchKernelGGL(syndrome_gather_kernel, grid, dim3(256), 0, st, s->d_GB, s->lgc, m_lo, NC - m_lo, row, (uint32_t)B, f.syn_out);
            break;
        case Syn::SET:
            hipLaunchKernelGGL(syndrome_set_kernel, grid, dim3(256), 0, st, s->d_GB, s->lgc, NC, m_lo, row, (uint32_t)B, b0, s->d_pattern_of, t->d_mlo, flag);
            break;
        case Syn::GATHER_SET:
            hipLaunchKernelGGL(syndrome_gather_set_kernel, grid, dim3(256), 0, st, s->d_GB, s->lgc, NC, m_lo, row, (uint32_t)B, s->d_list + b0, s->d_pattern_of, t->d_mlo,
                               (uint32_t)f.stride, f.syn_out);
            break;
        }
        HIP_TRY(hipGetLastError());
    }
    return FASTECC_OK;
}

// the form of the single named pattern (`named`), or of no pattern: flags, or every syndrome gathered to syn_out
ChunkForm pattern_form(const ScrubState* s, Fp fp, bool named, uint32_t* syn_out = nullptr)
{
    const Erasures er = erasures(s, named);
    const uint64_t m_lo = s->N + s->fixed + er.w;  // m_lo >= NC: n - k blocks named absent, no coefficient is left to check
    return {fp, syn_out ? Syn::GATHER : Syn::FLAGS, m_lo, m_lo < s->NC, er, syn_out, 0};
}

// fastecc_verify_batch on a locked context: flag[b] = 1 iff fastecc_verify with this seed would find stripe b inconsistent.  The chunks of
// B stripes in the BATCH form, then one copy of the flags and one synchronisation for the whole call.
// probe: the chunks end after their fingerprint pass (nothing else sets a flag then: flag[b] = 1 iff a block of stripe b holds a word >= p).
int verify_batch_locked(fastecc_ctx* c, const uint32_t* data, const uint32_t* parity, uint64_t count, uint64_t seed, hipStream_t st, std::vector<uint8_t>& flag,
                        const Probe* probe = nullptr)
{
    return settled(st, [&]() -> int {
        ScrubState* s = nullptr;
        int rc = scrub_state(c, &s);
        if (rc != FASTECC_OK) return rc;
        if ((rc = batch_begin(c, s, count, seed, st)) != FASTECC_OK) return rc;
        const ChunkForm f = pattern_form(s, Fp::BATCH, true);
        const uint64_t chunk = chunk_of(c, s);
        for (uint64_t b0 = 0; b0 < count; b0 += chunk)
            if ((rc = chunk_pass(c, s, f, data, parity, b0, std::min(chunk, count - b0), st, probe)) != FASTECC_OK) return rc;
        return batch_end(s, count, st, flag);
    });
}

// ---- list forms: the same passes over the stripes list[0 .. L) of the pool ----

// What a list pass needs before its first chunk: the chunk buffers, the seed's weights, the device copy of the list and its cleared per-entry flags;
// enqueued on st (the host list must live until the next synchronise)
int list_begin(fastecc_ctx* c, ScrubState* s, const std::vector<uint64_t>& list, uint64_t seed, hipStream_t st)
{
    const uint64_t L = list.size();
    int rc = batch_state(c, s);
    if (rc == FASTECC_OK) rc = upload_weights(c, s, seed, st);
    if (rc == FASTECC_OK) rc = s->d_list.grow(L);
    if (rc == FASTECC_OK) rc = s->d_lflag.grow(2 * L);
    if (rc != FASTECC_OK) return rc;
    HIP_TRY(hipMemcpyAsync(s->d_list, list.data(), L * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(s->d_lflag, 0, 2 * s->lflag_cap(), st));
    return FASTECC_OK;
}

// verify_batch_locked over the stripes `list` of the pool: flag[i] = 1 iff fastecc_verify with this seed would find stripe list[i] inconsistent
// (named: under the named erasures).  One copy of the flags and one synchronisation for the call.  probe: as for verify_batch_locked, and
// flag[i] = 1 iff a block of stripe list[i] holds a word >= p.
int verify_list_locked(fastecc_ctx* c, const uint32_t* data, const uint32_t* parity, const std::vector<uint64_t>& list, uint64_t seed, hipStream_t st, bool named,
                       std::vector<uint8_t>& flag, const Probe* probe = nullptr)
{
    return settled(st, [&]() -> int {
        ScrubState* s = nullptr;
        int rc = scrub_state(c, &s);
        if (rc != FASTECC_OK) return rc;
        if ((rc = list_begin(c, s, list, seed, st)) != FASTECC_OK) return rc;
        const ChunkForm f = pattern_form(s, Fp::LIST, named);
        const uint64_t chunk = chunk_of(c, s), L = list.size();
        for (uint64_t l0 = 0; l0 < L; l0 += chunk)
            if ((rc = chunk_pass(c, s, f, data, parity, l0, std::min(chunk, L - l0), st, probe)) != FASTECC_OK) return rc;
        flag.assign(L, 0);
        HIP_TRY(hipMemcpyAsync(flag.data(), s->d_lflag + (probe ? s->lflag_cap() : 0), L, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return FASTECC_OK;
    });
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
// has more than 512 syndromes.  Per chunk: one list pass that gathers every syndrome (gather_chunk), Berlekamp-Massey and the recurrence check on
// the host (solve_chunk), one root search over all locators (search_chunk), the roots' blocks (accept_chunk); two synchronisations.
// pattern_of (host, by stripe): every entry under its own pattern of the set instead — the SET_LIST pass, avail per entry
// (each in [1, GATHER_MAX]: locate_list lists no others), the device copy d_pattern_of that the call's verify pass made.
struct LocateList {
    static constexpr uint64_t GATHER_MAX = 512;
    fastecc_ctx* c;
    ScrubState* s;
    const uint32_t *data, *parity;
    const std::vector<uint64_t>& list;
    uint64_t seed;
    hipStream_t st;
    std::vector<uint8_t>& state;
    std::vector<std::vector<uint32_t>>& blocks;
    const uint32_t* pattern_of = nullptr;
    ChunkForm form{};                                                  // the list pass that gathers; form.syn_out: the chunk's syndromes
    uint64_t avail = 0, tmax = 0, gather = 0, stride = 0, cap = 0;     // syndromes per column (the most of any entry), locate_max, those Berlekamp-Massey reads, words per locator, roots kept
    uint32_t *d_lam = nullptr, *d_len = nullptr, *d_found = nullptr;   // the chunk's locators, their lengths, the found lists
    std::vector<uint32_t> syn, len, found, cand;                       // host copies; Berlekamp-Massey's scratch
    std::vector<uint8_t> big;
    std::vector<uint64_t> who;                                         // list entries with a locator, in table order
    std::vector<std::vector<uint32_t>> lambdas;                        // their locators

    // the chunk's buffer (d_loc, grow-only): syndromes | locators | their lengths | found lists
    int layout(uint64_t chunk)
    {
        gather = std::min<uint64_t>(2 * tmax, avail);
        stride = cap = std::min<uint64_t>(tmax, gather / 2) + 1;
        const uint64_t syn_words = chunk * R * avail, lam_words = chunk * stride, found_words = chunk * (cap + 1);
        const int rc = s->d_loc.grow(syn_words + lam_words + chunk + found_words);
        if (rc != FASTECC_OK) return rc;
        if (pattern_of)
            form = ChunkForm{Fp::SET_LIST, Syn::GATHER_SET, s->set->mlo_min, true, {}, s->d_loc, 0, avail};
        else
            form = pattern_form(s, Fp::LIST, true, s->d_loc);
        d_lam = s->d_loc + syn_words;
        d_len = d_lam + lam_words;
        d_found = d_len + chunk;
        syn.resize(syn_words);
        big.resize(chunk);
        return FASTECC_OK;
    }

    // the list pass over entries [l0, l0 + B), every syndrome and the big marks copied back; the chunk's first synchronisation
    int gather_chunk(uint64_t l0, uint64_t B)
    {
        form.blocks_read = 0;
        for (uint64_t i = l0; pattern_of && i < l0 + B; i++) form.blocks_read += s->n - view_of(i).w;
        const int rc = chunk_pass(c, s, form, data, parity, l0, B, st);
        if (rc != FASTECC_OK) return rc;
        HIP_TRY(hipMemcpyAsync(syn.data(), form.syn_out, B * R * avail * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(big.data(), s->d_lflag + s->lflag_cap() + l0, B, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return FASTECC_OK;
    }

    // the erasures entry i is located under, and the syndromes it has per column
    Erasures view_of(uint64_t i) const { return pattern_of ? set_view(s, pattern_of[list[i]]) : form.er; }
    uint64_t avail_of(uint64_t i) const { return pattern_of ? s->n - s->k - view_of(i).w : avail; }

    // host only: who and lambdas, the entries with a locator that every syndrome confirms; the others keep LOC_FALLBACK or become LOC_UNCORRECTABLE
    void solve_chunk(uint64_t l0, uint64_t B)
    {
        who.clear();
        lambdas.clear();
        for (uint64_t b = 0; b < B; b++) {
            if (big[b]) continue;  // known erasures besides the named ones: the single-stripe code
            const uint32_t* sy = syn.data() + b * R * avail;
            const uint64_t have = avail_of(l0 + b);  // (the entry's columns are `avail` words apart and hold `have`)
            bool zero = true;
            for (int col = 0; col < R && zero; col++) zero = std::all_of(sy + col * avail, sy + col * avail + have, [](uint32_t v) { return v == 0; });
            if (zero) continue;  // (consistent after all: cannot happen for a stripe the same seed flagged)
            state[l0 + b] = LOC_UNCORRECTABLE;
            std::vector<uint32_t> lambda;
            if (longest_lfsr(sy, avail, std::min<uint64_t>(2 * tmax, have), tmax, lambda, cand) == 0) continue;
            // confirmation: every syndrome of every column obeys the locator's recurrence
            bool ok = true;
            for (int col = 0; col < R && ok; col++) ok = obeys_recurrence(sy + col * avail, have, lambda);
            if (!ok) continue;
            who.push_back(l0 + b);
            lambdas.push_back(std::move(lambda));
        }
    }

    // the locators uploaded, one root search over all of them, the found lists copied back; the chunk's second synchronisation
    int search_chunk()
    {
        const uint64_t E = who.size();
        std::vector<uint32_t> lam(E * stride, 0);
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
        return FASTECC_OK;
    }

    // an entry whose locator splits into as many distinct roots as its length, each at a block that is there and not erased, is LOC_FOUND
    void accept_chunk()
    {
        for (uint64_t e = 0; e < who.size(); e++) {
            const uint32_t* f = found.data() + e * (cap + 1);
            if (f[0] != len[e]) continue;  // a locator splits into distinct roots at the code's positions, or it is no locator
            std::vector<uint32_t> js;
            bool ok = true;
            const Erasures er = view_of(who[e]);
            for (uint32_t i = 0; i < f[0] && ok; i++) ok = accept_root(f[1 + i], s->block_at, er, nullptr, js);
            if (!ok) continue;
            std::sort(js.begin(), js.end());
            blocks[who[e]] = std::move(js);
            state[who[e]] = LOC_FOUND;
        }
    }

    int run()
    {
        const uint64_t L = list.size(), m = s->n - s->k, w = erasures(s, true).w;
        state.assign(L, LOC_FALLBACK);
        blocks.assign(L, {});
        avail = m > w ? m - w : 0;
        if (pattern_of) avail = 0;
        for (uint64_t i = 0; pattern_of && i < L; i++) avail = std::max(avail, avail_of(i));
        tmax = (uint64_t)c->locate_max;
        if (L == 0 || avail == 0 || avail > GATHER_MAX) return FASTECC_OK;
        int rc = list_begin(c, s, list, seed, st);
        if (rc != FASTECC_OK) return rc;
        const uint64_t chunk = std::min(chunk_of(c, s), L);
        if ((rc = layout(chunk)) != FASTECC_OK) return rc;
        for (uint64_t l0 = 0; l0 < L; l0 += chunk) {
            const uint64_t B = std::min(chunk, L - l0);
            if ((rc = gather_chunk(l0, B)) != FASTECC_OK) return rc;
            solve_chunk(l0, B);
            if (who.empty()) continue;
            if ((rc = search_chunk()) != FASTECC_OK) return rc;
            accept_chunk();
        }
        return FASTECC_OK;
    }
};

// fastecc_scrub_erasures on a locked context: `absent` (codeword indices, increasing, at most n - k) replaces the named pattern.  The marked
// position table and the locator table lfix * prod (x - w^pos) are built aside and swapped in, so a failure leaves the previous pattern in
// force.  Synchronous; every scrub call ends with a synchronise, so nothing in flight reads the tables that are freed here.
int set_erasures(fastecc_ctx* c, const std::vector<uint32_t>& absent)
{
    ScrubState* s = c->scrub;
    DeviceBuf<uint32_t> d_pos, d_loc;
    std::vector<uint8_t> is_absent;
    if (!absent.empty()) {
        RC_TRY(scrub_state(c, &s));
        std::vector<uint32_t> pos(s->pos), roots(absent.size());
        is_absent.assign(s->n, 0);
        const uint32_t w = gf::h_root((uint32_t)s->NC);
        for (size_t i = 0; i < absent.size(); i++) {
            roots[i] = gf::h_pow(w, s->pos[absent[i]]);
            pos[absent[i]] |= ABSENT;
            is_absent[absent[i]] = 1;
        }
        DeviceBuf<uint32_t> d_roots;
        RC_TRY(d_pos.alloc(s->n));
        RC_TRY(d_loc.alloc(s->NC));
        RC_TRY(d_roots.alloc(roots.size()));
        HIP_TRY(hipMemcpy(d_pos, pos.data(), s->n * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_roots, roots.data(), roots.size() * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(locator_kernel<false>, dim3((unsigned)((s->NC + 255) / 256)), dim3(256), 0, nullptr, s->d_lfix, d_roots, (uint32_t)roots.size(),
                           s->d_wpow, (uint32_t)s->NC, nullptr, d_loc);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
    }
    if (!s) return FASTECC_OK;  // no scrub state yet and nothing to name
    s->d_pos_named = std::move(d_pos);
    s->d_lnamed = std::move(d_loc);
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
        if (s) s->set.reset();
        return FASTECC_OK;
    }
    RC_TRY(scrub_state(c, &s));
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
    DeviceBuf<uint32_t> d_roots, d_off;
    RC_TRY(t->d_pos.alloc(P * n));
    RC_TRY(t->d_l.alloc(P * NC));
    RC_TRY(t->d_mlo.alloc(P));
    RC_TRY(d_roots.alloc(std::max<size_t>(roots.size(), 1)));
    RC_TRY(d_off.alloc(P + 1));
    HIP_TRY(hipMemcpy(t->d_pos, pos.data(), P * n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(t->d_mlo, t->mlo.data(), P * 4, hipMemcpyHostToDevice));
    if (!roots.empty()) HIP_TRY(hipMemcpy(d_roots, roots.data(), roots.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_off, off.data(), (P + 1) * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(locator_set_kernel, dim3((unsigned)((NC + 255) / 256), (unsigned)P), dim3(256), 0, nullptr, s->d_lfix, d_roots, d_off,
                       s->d_wpow, (uint32_t)NC, t->d_l);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    s->set = std::move(t);
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
// The chunks in the SET form, the syndrome check of every stripe from its own pattern's bound on.  A chunk in which no block is read is skipped; one
// in which no stripe has a coefficient left (n - k blocks absent, or none named) skips transform and check.  pattern_of is copied synchronously
// (every scrub call, a failed one included, leaves nothing in flight that reads the device copy), so the caller's array is free on every return.
int verify_batch_set_locked(fastecc_ctx* c, const uint32_t* data, const uint32_t* parity, uint64_t count, const uint32_t* pattern_of, uint64_t seed, hipStream_t st,
                            std::vector<uint8_t>& flag)
{
    return settled(st, [&]() -> int {
        ScrubState* s = c->scrub;
        const ScrubSet* t = s->set.get();
        int rc = s->d_pattern_of.grow(count);
        if (rc != FASTECC_OK) return rc;
        HIP_TRY(hipMemcpy(s->d_pattern_of, pattern_of, count * 4, hipMemcpyHostToDevice));
        if ((rc = batch_begin(c, s, count, seed, st)) != FASTECC_OK) return rc;
        const uint64_t chunk = chunk_of(c, s);
        ChunkForm f{Fp::SET, Syn::SET, t->mlo_min, false, {}, nullptr, 0};
        for (uint64_t b0 = 0; b0 < count; b0 += chunk) {
            const uint64_t B = std::min(chunk, count - b0);
            f.blocks_read = 0;
            f.check = false;
            for (uint64_t b = b0; b < b0 + B; b++) {
                if (pattern_of[b] == FASTECC_PATTERN_NONE) continue;
                f.blocks_read += s->n - t->absent[pattern_of[b]].size();
                f.check = f.check || t->mlo[pattern_of[b]] < s->NC;
            }
            if (f.blocks_read == 0) continue;  // every stripe of the chunk is FASTECC_PATTERN_NONE (a stripe with a pattern reads at least k blocks)
            if ((rc = chunk_pass(c, s, f, data, parity, b0, B, st)) != FASTECC_OK) return rc;
        }
        return batch_end(s, count, st, flag);
    });
}

// ---- the pool calls, written once for both forms ----

// What the two forms of a pool call differ in: every stripe under the single fastecc_scrub_erasures pattern (pattern_of null), or stripe b under pattern
// pattern_of[b] of the set (host, by stripe).  Every member is evaluated under the context's lock.
struct StripePatterns {
    const uint32_t* pattern_of;

    // the form's own argument check
    int args(const fastecc_ctx* c, uint64_t count) const { return pattern_of ? set_args(c, pattern_of, count) : FASTECC_OK; }

    // its verify pass over the pool
    int verify(fastecc_ctx* c, const uint32_t* data, const uint32_t* parity, uint64_t count, uint64_t seed, hipStream_t st, std::vector<uint8_t>& flag) const
    {
        if (pattern_of) return verify_batch_set_locked(c, data, parity, count, pattern_of, seed, st, flag);
        return verify_batch_locked(c, data, parity, count, seed, st, flag);
    }

    // the erasures `stripe` is scrubbed under; no view (d_pos null) where the set has no such pattern: args passed under this lock, or the set was
    // replaced since (correct_stripe)
    Erasures view(const ScrubState* s, uint64_t stripe) const
    {
        if (!pattern_of) return erasures(s, true);
        const uint32_t q = pattern_of[stripe];
        return s->set && q < s->set->P ? set_view(s, q) : Erasures{};
    }

    // the blocks absent under that view (the scrub state's own list: another call may replace the pattern or the set once the lock is released)
    const std::vector<uint32_t>& absent(const ScrubState* s, uint64_t stripe) const
    {
        static const std::vector<uint32_t> none;
        const Erasures er = view(s, stripe);
        return er.w ? *er.absent : none;
    }

    // whether the pattern set private to a correcting call (section 27) takes one more distinct lost set, of `blocks` blocks, after `sets`: the
    // single form has no such set, every lost set goes set by set there
    bool private_set_takes(size_t sets, size_t blocks) const { return pattern_of && blocks <= SET_MAX_LOST && sets < SET_MAX_PATTERNS; }
};

// the form's verify pass on a locked context (args passed): the inconsistent stripes, increasing
int flagged(fastecc_ctx* c, const uint32_t* data, const uint32_t* parity, uint64_t count, const StripePatterns& pats, uint64_t seed, hipStream_t st,
            std::vector<uint64_t>& list)
{
    std::vector<uint8_t> flag;
    const int r = pats.verify(c, data, parity, count, seed, st, flag);
    if (r != FASTECC_OK) return r;
    for (uint64_t b = 0; b < count; b++)
        if (flag[b]) list.push_back(b);
    return FASTECC_OK;
}

// LocateList over the flagged stripes `list`, stripe list[i] under pats.view (DESIGN.md sections 17 and 27).  Called under the same lock as the verify pass
// whose flags made the list: the scrub state is there, and under the set the pass's device copy of pattern_of serves the list pass.  Entries whose view
// leaves no syndrome or more than the batched pass gathers are not passed on and keep LOC_FALLBACK, so stripes of both kinds may share a call (under the
// single pattern every entry is of one kind).
int locate_list(fastecc_ctx* c, const uint32_t* data, const uint32_t* parity, const std::vector<uint64_t>& list, const StripePatterns& pats, uint64_t seed,
                hipStream_t st, std::vector<uint8_t>& state, std::vector<std::vector<uint32_t>>& blocks)
{
    std::vector<uint64_t> taken, at;  // the entries the batched pass takes: their stripes (the list pass copies them from here), their places in `list`
    return settled(st, [&]() -> int {
        ScrubState* s = c->scrub;
        const uint64_t m = s->n - s->k;
        for (size_t i = 0; i < list.size(); i++) {
            const uint64_t w = pats.view(s, list[i]).w;
            if (w >= m || m - w > LocateList::GATHER_MAX) continue;
            taken.push_back(list[i]);
            at.push_back(i);
        }
        state.assign(list.size(), LOC_FALLBACK);
        blocks.assign(list.size(), {});
        std::vector<uint8_t> st_taken;
        std::vector<std::vector<uint32_t>> bl_taken;
        LocateList ll{c, s, data, parity, taken, seed, st, st_taken, bl_taken, pats.pattern_of};
        const int rc = ll.run();
        if (rc != FASTECC_OK) return rc;
        for (size_t e = 0; e < at.size(); e++) {
            state[at[e]] = st_taken[e];
            blocks[at[e]] = std::move(bl_taken[e]);
        }
        return FASTECC_OK;
    });
}

// the seed of the closing verify of fastecc_correct and fastecc_correct_batch
uint64_t closing_seed(uint64_t seed)
{
    uint64_t state = seed ^ 0x5C7B5C7B5C7B5C7Bull;
    return splitmix64(state);
}

// fastecc_decode_prepare for exactly the blocks `lost` (codeword indices); it takes the context's lock itself
int prepare_lost(fastecc_ctx* c, const std::vector<uint32_t>& lost)
{
    std::vector<uint8_t> dp(c->K, 1), pp(c->Mu, 1);
    for (uint32_t j : lost) (j < c->K ? dp[j] : pp[j - c->K]) = 0;
    return fastecc_decode_prepare(c, dp.data(), pp.data());
}

// a verify pass's flags as the entry points report them
void report_flags(const std::vector<uint8_t>& flag, uint8_t* consistent, uint64_t* inconsistent)
{
    for (size_t b = 0; b < flag.size(); b++) consistent[b] = flag[b] ? 0 : 1;
    *inconsistent = (uint64_t)(flag.size() - std::count(flag.begin(), flag.end(), (uint8_t)0));
}

// One stripe's return code rc of fastecc_correct (or of locate) in a batch's terms: FASTECC_E_UNCORRECTABLE is *status = 2 and *uncorrectable, success
// is 1 where blocks were found (0: consistent after all); any other failure ends the call
int record_status(int rc, bool found, uint8_t* status, bool* uncorrectable)
{
    if (rc != FASTECC_OK && rc != FASTECC_E_UNCORRECTABLE) return rc;
    *status = rc != FASTECC_OK ? 2 : found ? 1 : 0;
    *uncorrectable = *uncorrectable || rc != FASTECC_OK;
    return FASTECC_OK;
}

// fastecc_verify; named = false: over all blocks whatever fastecc_scrub_erasures named (the closing check of fastecc_correct)
int verify_impl(fastecc_ctx* c, const void* data, const void* parity, int mem_kind, void* stream, uint64_t seed, int* consistent, bool named)
{
    if (!consistent) return FASTECC_E_INVAL;
    int rc = scrub_args(c, data, parity, mem_kind);
    if (rc != FASTECC_OK) return rc;
    return on_device(c, [&]() -> int {
        CallLock lk(c->mu);
        std::vector<uint32_t> found;
        ScrubState* s = nullptr;
        int r = scrub_state(c, &s);
        if (r != FASTECC_OK) return r;
        r = locate(c, s, erasures(s, named), (const uint32_t*)data, (const uint32_t*)parity, seed, (hipStream_t)stream, found, true);
        if (r == FASTECC_OK) *consistent = found.empty() ? 1 : 0;
        return r;
    });
}

// fastecc_correct on one stripe (DEVICE memory, arguments checked; data and parity are the stripe's own): locate under the view pats gives stripe
// `stripe` — the single fastecc_scrub_erasures pattern, or the stripe's pattern of the set — then rebuild located and absent blocks and verify the whole
// codeword with the derived seed.  found: the located blocks.
int correct_stripe(fastecc_ctx* c, void* data, void* parity, void* stream, uint64_t seed, const StripePatterns& pats, uint64_t stripe, std::vector<uint32_t>& found)
{
    std::vector<uint32_t> absent;
    {
        CallLock lk(c->mu);
        ScrubState* s = nullptr;
        int r = scrub_state(c, &s);
        if (r != FASTECC_OK) return r;
        const Erasures er = pats.view(s, stripe);
        if (!er.d_pos) return FASTECC_E_INVAL;  // (the set was replaced while the call ran)
        if (er.w) absent = *er.absent;
        r = locate(c, s, er, (const uint32_t*)data, (const uint32_t*)parity, seed, (hipStream_t)stream, found, false);
        if (r != FASTECC_OK) return r;
    }
    if (found.empty()) return FASTECC_OK;  // consistent: untouched, the absent blocks included
    // the erasure decoder rebuilds the located blocks and, in the same repair, the ones named absent (prepare and repair take the
    // context's lock themselves); the codeword is whole then, so the closing verify reads every block
    absent.insert(absent.end(), found.begin(), found.end());
    int r = prepare_lost(c, absent);
    if (r != FASTECC_OK) return r;
    r = fastecc_repair(c, data, parity, FASTECC_MEM_DEVICE, stream);
    if (r != FASTECC_OK) return r;
    int ok = 0;
    r = verify_impl(c, data, parity, FASTECC_MEM_DEVICE, stream, closing_seed(seed), &ok, false);
    if (r != FASTECC_OK) return r;
    return ok ? FASTECC_OK : FASTECC_E_UNCORRECTABLE;
}

// A batched location's outputs as its entry points report them — state[i] (LOC_FOUND / LOC_UNCORRECTABLE, no LOC_FALLBACK left) and found[i] of stripe
// list[i], every other stripe consistent — and its return code.  Every output is written only here, at the end: a failed call leaves them alone.
int report_located(const std::vector<uint64_t>& list, const std::vector<uint8_t>& state, const std::vector<std::vector<uint32_t>>& found, uint64_t count,
                   uint8_t* status, uint64_t* blocks, uint64_t cap, uint32_t* counts, uint64_t* inconsistent)
{
    uint64_t bad = 0;
    bool uncorrectable = false;
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
}

int report(const std::vector<uint32_t>& found, uint64_t* blocks, uint64_t cap, uint64_t* count)
{
    for (uint64_t i = 0; i < found.size() && i < cap; i++) blocks[i] = found[i];
    *count = found.size();
    return FASTECC_OK;
}

// fastecc_verify_batch / _verify_batch_set (null pointers refused): flags of the form's verify pass
int verify_pool_impl(fastecc_ctx* c, const void* data, const void* parity, uint64_t count, const StripePatterns& pats, void* stream, uint64_t seed,
                     uint8_t* consistent, uint64_t* inconsistent)
{
    const int rc = batch_args(c, data, parity, count);
    if (rc != FASTECC_OK) return rc;
    return on_device(c, [&]() -> int {
        CallLock lk(c->mu);
        int r = pats.args(c, count);
        if (r != FASTECC_OK) return r;
        std::vector<uint8_t> flag;
        r = pats.verify(c, (const uint32_t*)data, (const uint32_t*)parity, count, seed, (hipStream_t)stream, flag);
        if (r == FASTECC_OK) report_flags(flag, consistent, inconsistent);
        return r;
    });
}

// fastecc_locate_errors_batch / _locate_errors_batch_set (null pointers refused): the verify pass, the batched location of the flagged stripes, the
// single-stripe code for what that leaves, all under one lock
int locate_pool_impl(fastecc_ctx* c, const void* data, const void* parity, uint64_t count, const StripePatterns& pats, void* stream, uint64_t seed,
                     uint8_t* status, uint64_t* blocks, uint64_t cap, uint32_t* counts, uint64_t* inconsistent)
{
    const int rc = batch_args(c, data, parity, count);
    if (rc != FASTECC_OK) return rc;
    if (cap && count > UINT64_MAX / 8 / cap) return FASTECC_E_INVAL;
    return on_device(c, [&]() -> int {
        CallLock lk(c->mu);
        hipStream_t st = (hipStream_t)stream;
        const uint32_t *d = (const uint32_t*)data, *p = (const uint32_t*)parity;
        int r = pats.args(c, count);
        if (r != FASTECC_OK) return r;
        std::vector<uint64_t> list;
        std::vector<uint8_t> state;
        std::vector<std::vector<uint32_t>> found;
        bool uncorrectable = false;
        if ((r = flagged(c, d, p, count, pats, seed, st, list)) != FASTECC_OK) return r;
        if ((r = locate_list(c, d, p, list, pats, seed, st, state, found)) != FASTECC_OK) return r;
        const uint64_t data_words = c->K * c->S, parity_words = c->Mu * c->S;
        for (size_t i = 0; i < list.size(); i++) {
            if (state[i] != LOC_FALLBACK) continue;
            // a word >= p in a present block, no syndrome left or more than the batched pass gathers: the single-stripe code through the stripe's own
            // pointers, under the stripe's view
            r = locate(c, c->scrub, pats.view(c->scrub, list[i]), d + list[i] * data_words, p + list[i] * parity_words, seed, st, found[i], false);
            if ((r = record_status(r, !found[i].empty(), &state[i], &uncorrectable)) != FASTECC_OK) return r;  // (the status codes 1 and 2 are LOC_FOUND and LOC_UNCORRECTABLE)
        }
        return report_located(list, state, found, count, status, blocks, cap, counts, inconsistent);
    });
}

// fastecc_correct_batch / _correct_batch_set (arguments checked; DESIGN.md sections 17 and 27): the locked verify and location, then — grouped — the located
// stripes by lost set: located blocks and the blocks absent under the stripe's view.  The lost sets of at most 16 blocks, up to the 4096th distinct one, are
// repaired through ONE pattern set private to the call where the form has one (repair_lost_sets: one launch per size class); every other lost set takes one
// prepare and one list-form repair.  One closing verify for all of them, and correct_stripe under the stripe's view for whatever that leaves.
struct CorrectPool {
    fastecc_ctx* c;
    void *data, *parity;
    uint64_t count;
    StripePatterns pats;
    void* stream;
    uint64_t seed;
    const char* trace_label;                       // of the phase lines under FASTECC_TRACE_PREPARE
    std::vector<uint64_t> list;                    // the inconsistent stripes
    std::vector<uint8_t> state;                    // grouped: LOC_* per list entry
    std::vector<std::vector<uint32_t>> found;      // grouped: the located blocks per list entry
    bool grouped = false;
    std::vector<std::vector<uint32_t>> lost_sets;  // per distinct lost set of the private set: located and absent blocks, sorted
    std::vector<uint64_t> stripes;                 // the private set's stripes ...
    std::vector<uint32_t> set_of;                  // ... and the lost set of each
    std::vector<std::vector<uint32_t>> wide_sets;  // the lost sets that go set by set, in the order the first stripe of each appears
    std::vector<std::vector<uint64_t>> wide_members;
    std::vector<uint64_t> order;                   // every repaired stripe: the private set's, then the wide sets' members back to back
    DeviceBuf<uint64_t> dev_order;                 // the wide sets' part of it on the device, for this call only (the repair runs outside the scrub state's lock)
    std::vector<uint8_t> status;
    bool uncorrectable = false;
    PhaseTimer pt{trace_label};                    // (where a call's wall time goes, host work included)

    // under the lock: the inconsistent stripes and, where the mode and their number allow grouping, their located blocks and lost sets
    int flag_and_locate()
    {
        const int mode = c->correct_batch_mode;
        const uint32_t *d = (const uint32_t*)data, *p = (const uint32_t*)parity;
        CallLock lk(c->mu);
        int r = pats.args(c, count);
        if (r != FASTECC_OK) return r;
        if ((r = flagged(c, d, p, count, pats, seed, (hipStream_t)stream, list)) != FASTECC_OK) return r;
        status.assign(count, 0);
        pt.mark("verify pass");
        // one stripe has nothing to share; mode 0 groups from two qualifying stripes on
        const size_t least = mode == 1 ? 1 : 2;
        if (mode == 2 || list.size() < least) return FASTECC_OK;
        if ((r = locate_list(c, d, p, list, pats, seed, (hipStream_t)stream, state, found)) != FASTECC_OK) return r;
        pt.mark("batched location");
        grouped = list.size() - (size_t)std::count(state.begin(), state.end(), (uint8_t)LOC_FALLBACK) >= least;
        if (grouped) group_by_lost_set();
        return FASTECC_OK;
    }

    // the located stripes by their lost set — located blocks and the blocks absent under the stripe's view — into the private set while it takes them,
    // else set by set.  Under flag_and_locate's lock: the scrub state's lists of absent blocks are read here, and another call may replace the pattern
    // or the set once the lock is released.
    void group_by_lost_set()
    {
        std::map<std::vector<uint32_t>, size_t> narrow_of, wide_of;
        for (size_t i = 0; i < list.size(); i++) {
            if (state[i] == LOC_UNCORRECTABLE) {
                status[list[i]] = 2;
                uncorrectable = true;
            }
            if (state[i] != LOC_FOUND || found[i].empty()) continue;
            std::vector<uint32_t> lost(found[i]);
            const std::vector<uint32_t>& absent = pats.absent(c->scrub, list[i]);
            lost.insert(lost.end(), absent.begin(), absent.end());
            std::sort(lost.begin(), lost.end());
            auto it = narrow_of.find(lost);
            if (it == narrow_of.end() && pats.private_set_takes(lost_sets.size(), lost.size())) {
                it = narrow_of.emplace(lost, lost_sets.size()).first;
                lost_sets.push_back(lost);
            }
            if (it != narrow_of.end()) {
                stripes.push_back(list[i]);
                set_of.push_back((uint32_t)it->second);
                continue;
            }
            auto wt = wide_of.find(lost);
            if (wt == wide_of.end()) {
                wt = wide_of.emplace(lost, wide_sets.size()).first;
                wide_sets.push_back(lost);
                wide_members.emplace_back();
            }
            wide_members[wt->second].push_back(list[i]);
        }
        order = stripes;
        for (const auto& mb : wide_members) order.insert(order.end(), mb.begin(), mb.end());
        pt.mark("lost sets");
    }

    // the private set's stripes in one call, then one prepare and one list-form repair per wide set (all take the lock themselves)
    int repair_groups()
    {
        if (!stripes.empty()) RC_TRY(repair_lost_sets(c, data, parity, lost_sets, stripes, set_of, stream));
        if (wide_sets.empty()) return FASTECC_OK;
        const uint64_t first = stripes.size();
        RC_TRY(dev_order.alloc(order.size() - first));
        HIP_TRY(hipMemcpy(dev_order, order.data() + first, (order.size() - first) * 8, hipMemcpyHostToDevice));
        return settled((hipStream_t)stream, [&]() -> int {  // (dev_order goes with this object: a failure waits for the repairs that read it)
            uint64_t at = 0;
            for (size_t g = 0; g < wide_sets.size(); g++) {
                RC_TRY(prepare_lost(c, wide_sets[g]));
                RC_TRY(repair_list(c, data, parity, order.data() + first + at, dev_order + at, wide_members[g].size(), stream));
                at += wide_members[g].size();
            }
            return FASTECC_OK;
        });
    }

    // the closing verify of fastecc_correct for all repaired stripes at once: its second seed, every block read whatever pattern is named (the
    // stripes are whole now)
    int closing_verify()
    {
        std::vector<uint8_t> still;
        {
            CallLock lk(c->mu);
            RC_TRY(verify_list_locked(c, (const uint32_t*)data, (const uint32_t*)parity, order, closing_seed(seed), (hipStream_t)stream, false, still));
        }
        for (size_t i = 0; i < order.size(); i++) {
            status[order[i]] = still[i] ? 2 : 1;
            uncorrectable = uncorrectable || still[i];
        }
        return FASTECC_OK;
    }

    // fastecc_correct under the stripe's view, through the stripe's own pointers (correct_stripe takes the lock itself), on what the grouped path left:
    // every inconsistent stripe, or the LOC_FALLBACK ones
    int fallbacks()
    {
        const uint64_t block = c->S * 4, data_bytes = c->K * block, parity_bytes = c->Mu * block;
        std::vector<uint32_t> located;
        for (size_t i = 0; i < list.size(); i++) {
            if (grouped && state[i] != LOC_FALLBACK) continue;
            const uint64_t b = list[i];
            int r = correct_stripe(c, (char*)data + b * data_bytes, (char*)parity + b * parity_bytes, stream, seed, pats, b, located);
            if ((r = record_status(r, !located.empty(), &status[b], &uncorrectable)) != FASTECC_OK) return r;
        }
        return FASTECC_OK;
    }

    int run(uint8_t* status_out, uint64_t* inconsistent)
    {
        int r = flag_and_locate();
        if (r != FASTECC_OK) return r;
        if (!order.empty()) {
            if ((r = repair_groups()) != FASTECC_OK) return r;
            pt.mark("private set and repair");
            if ((r = closing_verify()) != FASTECC_OK) return r;
            pt.mark("closing verify");
        }
        if ((r = fallbacks()) != FASTECC_OK) return r;
        pt.mark("stripe by stripe");
        std::copy(status.begin(), status.end(), status_out);
        *inconsistent = list.size();
        return uncorrectable ? FASTECC_E_UNCORRECTABLE : FASTECC_OK;
    }
};

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
    return on_device(c, [&]() -> int {
        CallLock lk(c->mu);
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
    return on_device(c, [&]() -> int {
        CallLock lk(c->mu);
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
    return on_device(c, [&]() -> int {
        std::vector<uint32_t> found;
        const int r = correct_stripe(c, data, parity, stream, seed, StripePatterns{nullptr}, 0, found);
        return r == FASTECC_OK ? report(found, blocks, cap, count) : r;
    });
}

int fastecc_verify_batch(fastecc_ctx* c, const void* data, const void* parity, uint64_t count, void* stream, uint64_t seed, uint8_t* consistent,
                         uint64_t* inconsistent)
{
    if (!consistent || !inconsistent) return FASTECC_E_INVAL;
    return verify_pool_impl(c, data, parity, count, {nullptr}, stream, seed, consistent, inconsistent);
}

int fastecc_locate_errors_batch(fastecc_ctx* c, const void* data, const void* parity, uint64_t count, void* stream, uint64_t seed, uint8_t* status,
                                uint64_t* blocks, uint64_t cap, uint32_t* counts, uint64_t* inconsistent)
{
    if (!status || !inconsistent || (cap && (!blocks || !counts))) return FASTECC_E_INVAL;
    return locate_pool_impl(c, data, parity, count, {nullptr}, stream, seed, status, blocks, cap, counts, inconsistent);
}

int fastecc_correct_batch(fastecc_ctx* c, void* data, void* parity, uint64_t count, void* stream, uint64_t seed, uint8_t* status, uint64_t* inconsistent)
{
    if (!status || !inconsistent) return FASTECC_E_INVAL;
    const int rc = batch_args(c, data, parity, count);
    if (rc != FASTECC_OK) return rc;
    return on_device(c, [&]() -> int {
        CorrectPool cp{c, data, parity, count, {nullptr}, stream, seed, "[fastecc correct_batch]"};
        return cp.run(status, inconsistent);
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
    return verify_pool_impl(c, data, parity, count, {pattern_of}, stream, seed, consistent, inconsistent);
}

int fastecc_correct_batch_set(fastecc_ctx* c, void* data, void* parity, uint64_t count, const uint32_t* pattern_of, void* stream, uint64_t seed, uint8_t* status,
                              uint64_t* inconsistent)
{
    if (!status || !inconsistent || !pattern_of) return FASTECC_E_INVAL;
    const int rc = batch_args(c, data, parity, count);
    if (rc != FASTECC_OK) return rc;
    return on_device(c, [&]() -> int {
        CorrectPool cp{c, data, parity, count, {pattern_of}, stream, seed, "[fastecc correct_batch_set]"};
        return cp.run(status, inconsistent);
    });
}

int fastecc_locate_errors_batch_set(fastecc_ctx* c, const void* data, const void* parity, uint64_t count, const uint32_t* pattern_of, void* stream, uint64_t seed,
                                    uint8_t* status, uint64_t* blocks, uint64_t cap, uint32_t* counts, uint64_t* inconsistent)
{
    if (!status || !inconsistent || !pattern_of || (cap && (!blocks || !counts))) return FASTECC_E_INVAL;
    return locate_pool_impl(c, data, parity, count, {pattern_of}, stream, seed, status, blocks, cap, counts, inconsistent);
}

}  // extern "C"
