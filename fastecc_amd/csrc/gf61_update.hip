// gf61_update.hip — small writes over GF((2^61-1)^2): fastecc_gf61_update, fastecc_gf61_update_parity and fastecc_gf61_code_coefficient
// (include/fastecc.h).  The scheme is update.hip's, on 16-byte elements.
//
// The code is linear, so after data blocks i_u change by D_u = new_u - old_u the parity changes by
//     parity[q][col] += sum_u L_{i_u}(y_q) * D_u[col]   (in GF(p^2)),
// L_i the Lagrange basis on the data points.  The field's codes sit on the positions of the 32-bit ones (internal.hpp: code_parity_position): on the
// NC-th roots of unity, NC = N << e, data block i at i << e, parity block q at pos(q) — for the codes inside (2N,N) the odd positions
// ((q * stride) << 1) + 1 with the context's p61_stride, for n = 4k / 8k the cosets' offsets.  With w = w_NC the weight depends on the difference of
// positions only:
//     L_i(y_q) = G[(pos(q) - (i << e)) mod NC],   G[u] = (w^(uN) - 1) / (N (w^u - 1))   (u not a multiple of 2^e),
// so ONE table serves every data block, every parity block and every call — and the zero-extended codes need no padded copies of the stripes: the
// caller's k data and n - k parity blocks are read and written where they are.  The table holds only the u that occur, u at u - (u >> e) - 1
// (N (2^e - 1) entries), each as the COEF_WORDS limb words of gf61_limbs.hpp: 72 bytes, 38 MB at k = 2^19.
//
// A call runs in passes of up to ROWS changed blocks:
//   k_update_table : one thread per entry (three exponentiations, one inversion), once per context, on the stream of the first call;
//   k_update_delta : D_u, canonical, into the context's delta rows; fastecc_gf61_update also stores new_u into the stripe, in the thread that
//                    has read old_u.  Of the two forms update.hip has (delta rows / differences formed in the parity kernel's registers with a scatter
//                    kernel behind it) this is the single-stripe one: the parity kernel runs several waves per column slice, each of which would
//                    read old and new again, and the delta rows are the context's own — 16-byte aligned whatever the caller's pointers are;
//   k_update_parity: a wave owns 64 element columns and a run of parity blocks.  It loads the pass's T <= ROWS delta elements of its lanes into
//                    VGPRs once (4 per row), then streams its parity blocks: the T wave-uniform weights by scalar loads (18 words each, two rows
//                    in one fetch: 36 SGPRs — with four, 72, the kernels spill scalar registers), 8 mac3 per row into two Acc3 sums, gather3,
//                    + the old element, canonical, a non-temporal store.  The next block's load is in flight during the current block's arithmetic.
#include <algorithm>
#include <atomic>
#include <vector>

#include "devmem.hpp"
#include "drivers.hpp"
#include "gf61_limbs.hpp"

namespace fastecc {

namespace {

using gf61::Elem;
using gf61::P;
using namespace p61;  // the limb arithmetic

constexpr int ROWS = 16;  // changed blocks per pass: delta rows held in VGPRs, 4 each

// Rows in a pass, 4 partial products below 2^53 per row and sum: 16 x 4 x 2^53 = 2^59 < 2^64, so an Acc3 takes a whole pass without a fold.
static_assert(ROWS * 4 <= (1 << 11), "an Acc3 sum of a pass stays below 2^64");

struct CodeGeom {
    uint64_t N = 0;  // transform order, a power of two
    int e = 1, fold = 0, cosets = 1;  // fold: log2 of the stride of the code's parity blocks in the (2N,N) parity
    uint64_t K = 0, Mu = 0;           // data and parity blocks of the caller's stripes
};

Elem geom_weight(const CodeGeom& g, uint64_t i, uint64_t q)
{
    const uint64_t NC = g.N << g.e;
    const uint64_t u = (code_parity_position(g.N, g.e, g.fold, g.cosets, q) + NC - (i << g.e)) % NC;
    const Elem wu = gf61::h_pow(gf61::h_root(NC), u);
    Elem num = gf61::h_pow(wu, g.N);
    num.re = gf61::h_subp(num.re, 1);
    const Elem den = gf61::h_mul(Elem{g.N % P, 0}, Elem{gf61::h_subp(wu.re, 1), wu.im});
    return gf61::h_mul(num, gf61::h_inv(den));
}

// The geometry fastecc_create gives (n, k) over this field, without a device
int geom_of_code(uint64_t n, uint64_t k, CodeGeom* g)
{
    if (k < 1 || n <= k) return FASTECC_E_INVAL;
    int lg = 0;
    RC_TRY(pow2_code_shape(n, k, &lg, &g->fold, &g->cosets));  // create.hip: the same rule as fastecc_create
    if (lg > p61::MAX_LOG2_K) return FASTECC_E_UNSUPPORTED;
    g->N = 1ull << lg;
    g->e = code_coset_shift(g->cosets);
    g->K = k;
    g->Mu = n - k;
    return FASTECC_OK;
}

CodeGeom geom_of_ctx(const fastecc_ctx* c)
{
    CodeGeom g;
    g.N = c->N;
    g.cosets = c->cosets;
    g.e = code_coset_shift(c->cosets);
    while ((1 << g.fold) < c->p61_stride) g.fold++;  // (the context keeps fold = 0 for this field and the code's fold in p61_stride: create.hip)
    g.K = c->K;
    g.Mu = c->Mu;
    return g;
}

// ---- device code ----
// A 16-byte element as four dwords: re low, re high, im low, im high — the 32-bit halves mac3 takes.  The caller's blocks are 8-byte aligned.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));
__device__ __forceinline__ Elem ld8(const uint64_t* p)
{
    const u32x4 t = *reinterpret_cast<const u32x4_a8*>(p);
    return Elem{gf61::join(t[0], t[1]), gf61::join(t[2], t[3])};
}
__device__ __forceinline__ void st8(uint64_t* p, Elem v)
{
    *reinterpret_cast<u32x4_a8*>(p) = u32x4{(uint32_t)v.re, (uint32_t)(v.re >> 32), (uint32_t)v.im, (uint32_t)(v.im >> 32)};
}
__device__ __forceinline__ uint64_t subc(uint64_t x, uint64_t y) { return x >= y ? x - y : x + P - y; }  // canonical - canonical -> canonical

// 1 / x = conj(x) / (re^2 + im^2); the norm lies in GF(p) and is inverted by norm^(p-2)
__device__ __forceinline__ Elem invc(Elem x, const gf61::Opaque& k)
{
    const Elem re2 = gf61::mul_canon(Elem{x.re, 0}, Elem{x.re, 0}, k), im2 = gf61::mul_canon(Elem{x.im, 0}, Elem{x.im, 0}, k);
    const uint64_t norm = re2.re + im2.re;
    const Elem ninv = gf61::pow_canon(Elem{norm >= P ? norm - P : norm, 0}, P - 2, k);
    return gf61::mul_canon(Elem{x.re, subc(0, x.im)}, ninv, k);
}

// entry v holds G[u], u = v + v / (2^e - 1) + 1: the v-th index that is no multiple of 2^e
__global__ __launch_bounds__(256) void k_update_table(uint32_t* __restrict__ G, uint32_t entries, uint64_t wre, uint64_t wim, uint64_t N, uint32_t emask)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= entries) return;
    const gf61::Opaque k = gf61::make_opaque();
    const uint32_t u = v + v / emask + 1u;
    const Elem wu = gf61::pow_canon(Elem{wre, wim}, u, k);
    Elem num = gf61::pow_canon(wu, N, k);
    num.re = subc(num.re, 1);
    const Elem den = gf61::mul_canon(Elem{N, 0}, Elem{subc(wu.re, 1), wu.im}, k);  // (N <= 2^24 < p; w^u != 1: u < NC is no multiple of NC)
    store_weight(G + (uint64_t)v * COEF_WORDS, gf61::mul_canon(num, invc(den, k), k));
}

struct DeltaArgs {
    uint64_t* data;              // fastecc_gf61_update: the stripe (old blocks read, new ones stored); else null
    const uint64_t* old_blocks;  // fastecc_gf61_update_parity: the pass's old blocks, contiguous (null: zero)
    const uint64_t* new_blocks;  // the pass's new blocks, contiguous
    uint64_t* delta;             // [rows][elems] elements
    uint64_t elems;
    uint32_t rows;               // rows of the pass; rows [rows, gridDim.y) of delta are zeroed (the parity kernel reads T rows)
    uint32_t idx[ROWS];          // data block of each row
};

// thread (element col, row r): delta[r][col] = new - old; the stripe gets new after old was read
__global__ __launch_bounds__(256) void k_update_delta(const DeltaArgs a)
{
    const uint64_t col = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t r = blockIdx.y;
    if (col >= a.elems) return;
    uint64_t* out = a.delta + 2 * ((uint64_t)r * a.elems + col);
    if (r >= a.rows) {
        st8(out, Elem{0, 0});
        return;
    }
    const Elem nv = ld8(a.new_blocks + 2 * ((uint64_t)r * a.elems + col));
    Elem ov{0, 0};
    if (a.data) {
        uint64_t* p = a.data + 2 * ((uint64_t)a.idx[r] * a.elems + col);
        ov = ld8(p);
        st8(p, nv);
    } else if (a.old_blocks) {
        ov = ld8(a.old_blocks + 2 * ((uint64_t)r * a.elems + col));
    }
    st8(out, Elem{subc(nv.re, ov.re), subc(nv.im, ov.im)});
}

// pos(q) of the code, and where the weight of a data block at position d (i << e) for parity block q stands in G
struct Positions {
    uint32_t NC, e;          // weight index = u - (u >> e) - 1, u = (pos(q) - d) mod NC
    uint32_t qs, qmask, ps;  // pos(q) = off[q >> qs] + ((q & qmask) << ps)
    uint32_t off[8];
    __device__ __forceinline__ uint32_t pos(uint32_t q) const { return off[q >> qs] + ((q & qmask) << ps); }
};

struct ParityArgs {
    uint64_t* parity;       // Mu blocks of elems elements
    const uint64_t* delta;  // [T][elems]
    const uint32_t* G;      // weight table, COEF_WORDS words per entry
    uint64_t elems;
    uint32_t M;             // parity blocks
    uint32_t slices;        // column slices of 64 elements
    uint32_t run;           // parity blocks per wave
    uint32_t waves;
    Positions p;
    uint32_t d[ROWS];       // position of each row's data block (i << e)
};

using const_u32_ptr = const uint32_t __attribute__((address_space(4)))*;

// Parity blocks through buffer descriptors, as in update.hip: the descriptor (base = the block, range = its bytes) is scalar and the lane offset is one
// VGPR fixed for the whole loop.  A lane past the end of the block gets an offset outside the range: its loads return 0 and its stores are dropped
// by the hardware.  aux 2: non-temporal.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t block_desc(const uint64_t* p, uint32_t bytes)
{
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), 0, bytes, 0x00020000);
}

// Every one of the T delta rows is loaded: rows past the pass's count are zero in the delta rows and point at a valid weight.  The loop has no branch
// on the row count or the lane; past the last block of the run the next load asks for the last block once more (never used).
template <int T>
__global__ __launch_bounds__(256) void k_update_parity(const ParityArgs a)
{
    constexpr int GRP = T >= 2 ? 2 : T;  // rows whose limbs come in one scalar fetch: 36 SGPRs
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (wave >= a.waves) return;
    const uint32_t slice = wave % a.slices;
    const uint32_t q0 = (wave / a.slices) * a.run, q1 = min(q0 + a.run, a.M);
    if (q0 >= q1) return;
    // elems * 16 < 2^32 (gf61_update_args): the lane's byte offset in a block fits 32 bits
    const uint64_t col = (uint64_t)slice * 64u + lane;
    const bool live = col < a.elems;
    const uint32_t bytes = (uint32_t)(a.elems * 16u);
    const uint32_t voff = live ? (uint32_t)col * 16u : bytes;  // (a dead lane: outside the range)
    const uint64_t lcol = live ? col : 0;                      // (a dead lane reads column 0 of the delta rows)
    u32x4 x[T];
#pragma unroll
    for (int i = 0; i < T; ++i) x[i] = *reinterpret_cast<const u32x4*>(a.delta + 2 * ((uint64_t)i * a.elems + lcol));  // (the context's own rows: 16-byte aligned)
    // The rows' positions live in the lanes of one VGPR and are read back one at a time (v_readlane): as 16 SGPRs beside the 72 of a fetch they do
    // not fit the scalar file
    const uint32_t dv = a.d[lane & (ROWS - 1)];
    const_u32_ptr G = (const_u32_ptr)(reinterpret_cast<uintptr_t>(a.G));
    auto desc = [&](uint32_t q) { return block_desc(a.parity + 2 * (uint64_t)q * a.elems, bytes); };
    auto step = [&](uint32_t q, const u32x4 old) {
        const uint32_t pos = a.p.pos(q);
        // Bound: a row adds 4 products below 2^53 to each of the six sums; T <= 16 rows: below 2^59.  No fold inside the loop.
        Acc3 re{0, 0, 0}, im{0, 0, 0};
#pragma unroll
        for (int g = 0; g < T; g += GRP) {
            uint32_t w[GRP * COEF_WORDS];  // pinned, so that a group's loads go out together and are not sunk between the multiply-adds
            // (and the group's addresses are formed behind the previous group's pins: formed for all groups at the head of the block they do not
            // fit the scalar file beside a fetch)
            uint32_t pg = pos;
            asm volatile("" : "+s"(pg));
#pragma unroll
            for (int i = 0; i < GRP; ++i) {
                int32_t u = (int32_t)(pg - __builtin_amdgcn_readlane(dv, g + i));
                if (u < 0) u += (int32_t)a.p.NC;
                const_u32_ptr cf = G + (uint64_t)((uint32_t)u - ((uint32_t)u >> a.p.e) - 1u) * COEF_WORDS;
#pragma unroll
                for (int t = 0; t < COEF_WORDS; ++t) w[i * COEF_WORDS + t] = cf[t];
            }
#pragma unroll
            for (int t = 0; t < GRP * COEF_WORDS; ++t) asm volatile("" : "+s"(w[t]));
#pragma unroll
            for (int i = 0; i < GRP; ++i) {
                const uint32_t* s = w + i * COEF_WORDS;
                const Limbs C{s[0], s[1], s[2]}, C2{s[3], s[4], s[5]}, D{s[6], s[7], s[8]}, D2{s[9], s[10], s[11]}, E{s[12], s[13], s[14]},
                    E2{s[15], s[16], s[17]};
                const u32x4 v = x[g + i];  // a0, a1, b0, b1
                mac3(re, v[0], C);
                mac3(re, v[1], C2);
                mac3(re, v[2], E);
                mac3(re, v[3], E2);
                mac3(im, v[0], D);
                mac3(im, v[1], D2);
                mac3(im, v[2], C);
                mac3(im, v[3], C2);
            }
        }
        // gather3 < 2^61 + 4, the old word < p: the sum is below 2^62 + 4, one fold leaves at most p + 2 < 2p, which canon takes
        auto finish = [](uint64_t sum, uint64_t o) {
            const uint64_t t = sum + o;
            return gf61::canon((t & P) + (t >> 61));
        };
        const uint64_t r0 = finish(gather3(re), gf61::join(old[0], old[1])), r1 = finish(gather3(im), gf61::join(old[2], old[3]));
        __builtin_amdgcn_raw_buffer_store_b128(u32x4{(uint32_t)r0, (uint32_t)(r0 >> 32), (uint32_t)r1, (uint32_t)(r1 >> 32)}, desc(q), voff, 0, 2);
    };
    auto load = [&](uint32_t q) -> u32x4 { return __builtin_amdgcn_raw_buffer_load_b128(desc(q), voff, 0, 2); };
    const uint32_t last = q1 - 1;
    u32x4 pa = load(q0), pb;
    for (uint32_t q = q0; q < q1; q += 2) {
        pb = load(min(q + 1, last));
        step(q, pa);
        if (q + 1 > last) break;
        pa = load(min(q + 2, last));
        step(q + 1, pb);
    }
}

}  // namespace

struct Gf61UpdateState {
    CodeGeom g;
    uint64_t NC = 0, entries = 0;
    DeviceBuf<uint32_t> d_G;  // weight table, entries x COEF_WORDS words
    bool table_ready = false, table_pending = false;
    Event table_event;  // end of the table kernel (on table_stream)
    hipStream_t table_stream = nullptr;
    DeviceBuf<uint64_t> d_delta;  // ROWS x elems elements (an internal buffer: ordered between streams by buf_event)
};

void destroy_gf61_update_state(Gf61UpdateState* s) { delete s; }

namespace {

// fastecc_profile_* through the field's launch hooks (drivers.hpp: P61Hooks), one scope per launch
struct HookScope {
    const p61::LaunchHooks* h;
    hipStream_t st;
    HookScope(const p61::LaunchHooks* h_, hipStream_t st_, const char* name, uint64_t bytes) : h(h_), st(st_)
    {
        if (h) h->begin(h->user, st, name, bytes);
    }
    ~HookScope()
    {
        if (h) h->end(h->user, st);
    }
};

// The weight table for stream st: built by a kernel on st at the first call (no host synchronisation); a use on another stream waits
// for that kernel on the device until it is seen complete.
int update_table(Gf61UpdateState* s, hipStream_t st, const p61::LaunchHooks* hooks)
{
    if (s->table_ready) {
        if (s->table_pending && st != s->table_stream) {
            if (hipEventQuery(s->table_event) == hipSuccess) s->table_pending = false;
            else HIP_TRY(hipStreamWaitEvent(st, s->table_event, 0));
            (void)hipGetLastError();  // hipErrorNotReady of the query is not an error
        }
        return FASTECC_OK;
    }
    RC_TRY(s->d_G.alloc(s->entries * COEF_WORDS));  // (FASTECC_E_NOMEM: the table does not fit)
    RC_TRY(s->table_event.create());
    {
        const Elem w = gf61::h_root(s->NC);
        HookScope ps(hooks, st, "gf61_update_table", s->entries * COEF_WORDS * 4);
        hipLaunchKernelGGL(k_update_table, dim3((unsigned)((s->entries + 255) / 256)), dim3(256), 0, st, s->d_G.get(), (uint32_t)s->entries, w.re, w.im,
                           (uint64_t)s->g.N, (uint32_t)((1u << s->g.e) - 1u));
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(s->table_event, st));
    s->table_stream = st;
    s->table_ready = s->table_pending = true;
    return FASTECC_OK;
}

int update_state(fastecc_ctx* c, Gf61UpdateState** out)
{
    if (!c->update61) {
        Gf61UpdateState* s = new (std::nothrow) Gf61UpdateState();
        if (!s) return FASTECC_E_NOMEM;
        s->g = geom_of_ctx(c);
        s->NC = s->g.N << s->g.e;  // <= 2^27 (k <= 2^24, e <= 3): positions and table indices are 32-bit
        s->entries = s->NC - s->g.N;
        c->update61 = s;
    }
    *out = c->update61;
    return FASTECC_OK;
}

template <class Launch>
void with_rows(int T, Launch&& launch)
{
    switch (T) {
        case 1: launch(std::integral_constant<int, 1>()); break;
        case 2: launch(std::integral_constant<int, 2>()); break;
        case 4: launch(std::integral_constant<int, 4>()); break;
        case 8: launch(std::integral_constant<int, 8>()); break;
        default: launch(std::integral_constant<int, ROWS>()); break;
    }
}

// waves of k_update_parity<T> one SIMD holds: 512 VGPRs in granules of 8, at most 8 (queried once per T)
int resident_waves_per_simd(int T)
{
    static std::atomic<int> cache[5];  // zero-initialised (static storage)
    int ti = 0;
    while ((1 << ti) < T) ti++;
    std::atomic<int>& slot = cache[ti];
    if (!slot.load()) {
        hipFuncAttributes attr{};
        const void* fn = nullptr;
        with_rows(T, [&](auto t_c) {
            constexpr int Tc = t_c;
            fn = (const void*)k_update_parity<Tc>;
        });
        int waves = 4;  // (if the query fails: a safe middle)
        if (hipFuncGetAttributes(&attr, fn) == hipSuccess && attr.numRegs > 0) waves = std::max(1, std::min(8, 512 / ((attr.numRegs + 7) / 8 * 8)));
        (void)hipGetLastError();
        slot.store(waves);
    }
    return slot.load();
}

// pos(q) of the code, in the form the parity kernel evaluates it
void set_positions(const Gf61UpdateState* s, Positions& p)
{
    const CodeGeom& g = s->g;
    p.NC = (uint32_t)s->NC;
    p.e = (uint32_t)g.e;
    if (g.cosets > 1) {  // coset t = q >> log2 N
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

// One pass: `rows` changed blocks
int update_pass(fastecc_ctx* c, Gf61UpdateState* s, uint64_t* data, uint64_t* parity, const uint64_t* blocks, uint32_t rows, const uint64_t* old_blocks,
                const uint64_t* new_blocks, hipStream_t st, const p61::LaunchHooks* hooks)
{
    const uint64_t elems = c->S / 4;
    DeltaArgs da{};
    da.data = data;
    da.old_blocks = old_blocks;
    da.new_blocks = new_blocks;
    da.delta = s->d_delta;
    da.elems = elems;
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
        HookScope ps(hooks, st, "gf61_update_delta", (uint64_t)rows * elems * 16 * (data || old_blocks ? 3 : 2) + (data ? rows * elems * 16 : 0));
        hipLaunchKernelGGL(k_update_delta, dim3((unsigned)((elems + 255) / 256), (unsigned)T), dim3(256), 0, st, da);
        HIP_TRY(hipGetLastError());
    }
    const CodeGeom& g = s->g;
    pa.parity = parity;
    pa.delta = s->d_delta;
    pa.G = s->d_G;
    pa.elems = elems;
    pa.M = (uint32_t)g.Mu;
    set_positions(s, pa.p);
    pa.slices = (uint32_t)((elems + 63) / 64);
    // every wave resident at once (the kernel's waves per SIMD from its register count), each with an equal run of parity blocks
    const uint64_t target = (uint64_t)c->cus * 4u * (uint64_t)resident_waves_per_simd(T);
    const uint64_t runs = std::max<uint64_t>(1, std::min<uint64_t>(g.Mu, target / pa.slices));
    pa.run = (uint32_t)((g.Mu + runs - 1) / runs);
    const uint64_t waves = (uint64_t)pa.slices * ((g.Mu + pa.run - 1) / pa.run);
    if (waves > 0xFFFFFFFFull / 64) return FASTECC_E_UNSUPPORTED;
    pa.waves = (uint32_t)waves;
    const dim3 grid((unsigned)((waves + 3) / 4));
    {
        HookScope ps(hooks, st, "gf61_update_parity", g.Mu * elems * 32);
        with_rows(T, [&](auto t_c) {
            constexpr int Tc = t_c;
            hipLaunchKernelGGL((k_update_parity<Tc>), grid, dim3(256), 0, st, pa);
        });
        HIP_TRY(hipGetLastError());
    }
    return FASTECC_OK;
}

// Everything that refuses a call, before any device work
int update_args(fastecc_ctx* c, const void* data, const void* parity, const uint64_t* blocks, uint64_t count, const void* old_blocks, const void* new_blocks,
                bool with_data)
{
    if (!c) return FASTECC_E_INVAL;
    if (count > 0 && (!parity || !blocks || !new_blocks || (with_data && !data))) return FASTECC_E_INVAL;
    if ((((uintptr_t)data | (uintptr_t)parity | (uintptr_t)old_blocks | (uintptr_t)new_blocks) & 7u) != 0) return FASTECC_E_INVAL;
    if (c->sharded || !c->p61 || c->field != FASTECC_FIELD_GF_P61_SQUARED) return FASTECC_E_UNSUPPORTED;
    if (c->ld != c->S) return FASTECC_E_UNSUPPORTED;
    // (blocks of 4 GiB: the kernel addresses a block through one buffer descriptor, whose range and lane offsets are 32-bit byte counts; a dead lane's
    // offset is the block's size itself)
    if (c->S * 4 + 64 * 16 > 0xFFFFFFFFull) return FASTECC_E_UNSUPPORTED;
    if (count == 0) return FASTECC_OK;
    std::vector<uint64_t> sorted(blocks, blocks + count);
    std::sort(sorted.begin(), sorted.end());
    if (sorted.back() >= c->K) return FASTECC_E_INVAL;
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return FASTECC_E_INVAL;  // a duplicate index
    return FASTECC_OK;
}

int update_run(fastecc_ctx* c, uint64_t* data, uint64_t* parity, const uint64_t* blocks, uint64_t count, const uint64_t* old_blocks, const uint64_t* new_blocks,
               hipStream_t st)
{
    Gf61UpdateState* s = nullptr;
    RC_TRY(update_state(c, &s));
    const uint64_t elems = c->S / 4;
    RC_TRY(s->d_delta.alloc((uint64_t)ROWS * elems * 2));
    P61Hooks hk(c);
    const p61::LaunchHooks* hooks = c->profiling ? &hk.h : nullptr;
    RC_TRY(update_table(s, st, hooks));
    return with_internal_buffers(c, st, [&]() -> int {
        for (uint64_t r0 = 0; r0 < count; r0 += ROWS) {
            const uint32_t rows = (uint32_t)std::min<uint64_t>(ROWS, count - r0);
            const size_t off = (size_t)r0 * elems * 2;
            RC_TRY(update_pass(c, s, data, parity, blocks + r0, rows, old_blocks ? old_blocks + off : nullptr, new_blocks + off, st, hooks));
        }
        return FASTECC_OK;
    });
}

}  // namespace

}  // namespace fastecc

using namespace fastecc;

extern "C" {

int fastecc_gf61_update(fastecc_ctx* c, void* data, void* parity, const uint64_t* blocks, uint64_t count, const void* new_blocks, void* stream)
{
    return guarded([&]() -> int {
        const int rc = update_args(c, data, parity, blocks, count, nullptr, new_blocks, true);
        if (rc != FASTECC_OK || count == 0) return rc;
        DeviceGuard dg(c->device);
        if (!dg.ok) return FASTECC_E_DEVICE;
        CallLock lk(c->mu);
        return update_run(c, (uint64_t*)data, (uint64_t*)parity, blocks, count, nullptr, (const uint64_t*)new_blocks, (hipStream_t)stream);
    });
}

int fastecc_gf61_update_parity(fastecc_ctx* c, void* parity, const uint64_t* blocks, uint64_t count, const void* old_blocks, const void* new_blocks, void* stream)
{
    return guarded([&]() -> int {
        const int rc = update_args(c, nullptr, parity, blocks, count, old_blocks, new_blocks, false);
        if (rc != FASTECC_OK || count == 0) return rc;
        DeviceGuard dg(c->device);
        if (!dg.ok) return FASTECC_E_DEVICE;
        CallLock lk(c->mu);
        return update_run(c, nullptr, (uint64_t*)parity, blocks, count, (const uint64_t*)old_blocks, (const uint64_t*)new_blocks, (hipStream_t)stream);
    });
}

int fastecc_gf61_code_coefficient(uint64_t n, uint64_t k, uint64_t data_block, uint64_t parity_block, uint64_t out[2])
{
    if (!out || k < 1 || n <= k || data_block >= k || parity_block >= n - k) return FASTECC_E_INVAL;
    CodeGeom g;
    const int rc = geom_of_code(n, k, &g);
    if (rc != FASTECC_OK) return rc;
    const Elem v = geom_weight(g, data_block, parity_block);
    out[0] = v.re;
    out[1] = v.im;
    return FASTECC_OK;
}

}  // extern "C"
