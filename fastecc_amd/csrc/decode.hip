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
#include <algorithm>
#include <cstring>
#include <vector>

#include "decode_state.hpp"
#include "ntt_device.hpp"

namespace fastecc {

void destroy_decode_state(DecodeState* d) { delete d; }

namespace {

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
    if (d->few.direct.both_built && (rebuild || d->few.direct.only_both)) return pass(d->few.direct.both, parity, data, rebuild ? parity_out : nullptr);
    if (d->few.direct.ed > 0) {
        const int rc = pass(d->few.direct.data, parity, data, nullptr);
        if (rc != FASTECC_OK) return rc;
    }
    return rebuild ? pass(d->few.direct.parity, nullptr, nullptr, parity_out) : FASTECC_OK;
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
        RC_TRY(d->host.parity_dev.alloc((c->Mu + c->K) * S));
        if (d->host.lists_of != d->pattern.serial) {
            // the rows that travel back: known from the set-up (few losses), else read off the decoder's tables once per pattern
            d->host.lost_data.clear();
            d->host.lost_parity.clear();
            if (d->pattern.erased_data + d->pattern.erased_parity <= (c->K + c->Mu) / 8 && d->tables.parity_lost && (d->pattern.erased_data == 0 || d->tables.gout)) {
                std::vector<uint32_t> flags(std::max(c->K, c->Mu));
                if (d->pattern.erased_data != 0) {
                    HIP_TRY(hipMemcpy(flags.data(), d->tables.gout, c->K * 4, hipMemcpyDeviceToHost));
                    for (uint64_t i = 0; i < c->K; i++)
                        if (flags[i] != 0) d->host.lost_data.push_back((uint32_t)i);
                }
                HIP_TRY(hipMemcpy(flags.data(), d->tables.parity_lost, c->Mu * 4, hipMemcpyDeviceToHost));
                for (uint64_t q = 0; q < c->Mu; q++)
                    if (flags[q] != 0) d->host.lost_parity.push_back((uint32_t)q);
                if (d->host.lost_data.size() != d->pattern.erased_data) d->host.lost_data.clear(), d->host.lost_parity.clear();  // (tables of another shape: whole stripes back)
            }
            d->host.lists_of = d->pattern.serial;
        }
        const uint64_t back = (d->pattern.erased_data != 0 ? d->host.lost_data.size() : 0) + (rebuild ? d->host.lost_parity.size() : 0);
        *rows_only = back != 0 && (d->pattern.erased_data == 0 || d->host.lost_data.size() == d->pattern.erased_data) &&
                     (!rebuild || d->host.lost_parity.size() == d->pattern.erased_parity) && back <= (c->K + c->Mu) / 8;
        const bool partial = !rebuild || *rows_only;  // (a repair that copies the whole parity stripe back must have staged all of it)
        const bool split = !d->pattern.direct_path && d->split.ready && d->pattern.standard && d->pattern.erased_data != 0 && partial;
        if (split && d->split.shift != 0) {
            // split transform, small form: the parity blocks at multiples of 2^shift are all it reads — one strided copy of every 2^shift-th block
            const size_t pitch = block << d->split.shift;
            HIP_TRY(hipMemcpy2DAsync(d->host.parity_dev, pitch, host_parity, pitch, block, (c->Mu + (1ull << d->split.shift) - 1) >> d->split.shift, hipMemcpyHostToDevice, st));
        } else if (split && d->split.groups < 512) {
            // group form: groups g < split_groups = blocks g + 1024 t, one strided copy
            HIP_TRY(hipMemcpy2DAsync(d->host.parity_dev, 1024 * block, host_parity, 1024 * block, (size_t)d->split.groups * block, c->Mu / 1024, hipMemcpyHostToDevice, st));
        } else if (d->pattern.direct_path && partial) {
            // few losses: the direct path reads as many parity blocks as data blocks are lost (at most 256 copies of a block)
            for (uint32_t q : d->host.parity_used)
                HIP_TRY(hipMemcpyAsync(d->host.parity_dev + (size_t)q * S, (const char*)host_parity + (size_t)q * block, block, hipMemcpyHostToDevice, st));
        } else {
            HIP_TRY(hipMemcpyAsync(d->host.parity_dev, host_parity, parity_bytes, hipMemcpyHostToDevice, st));
        }
        HIP_TRY(hipMemcpyAsync(d->host.parity_dev + c->Mu * S, host_data, data_bytes, hipMemcpyHostToDevice, st));
        parity = parity_out = d->host.parity_dev;
        data = d->host.parity_dev + c->Mu * S;
        return FASTECC_OK;
    }

    // any layout, few losses (profile: one "direct_pass" per read of the stripe)
    int direct()
    {
        return direct_passes(d, rebuild, data, parity, parity_out, [&](DirectPass* p, const uint32_t* par_in, uint32_t* data_to, uint32_t* par_to) {
            ProfScope ps(c, st, "direct_pass", (c->K + (uint64_t)d->few.direct.ed) * block);
            return direct_run(p, data, par_in, data_to, par_to, S, d->pattern.direct_kernel, st);
        });
    }

    // The transform path: fastecc_repair in one transform where the pattern's tables allow it, else the lost data and then the lost parity from
    // one more encode
    int transform()
    {
        if (rebuild && d->pattern.erased_data != 0) {
            bool done = false;
            int rc = d->split.ready && d->split.repair_ready ? repair_split(&done) : FASTECC_OK;
            if (rc == FASTECC_OK && !done && d->pattern.standard && d->tables.transform_full && d->tables.full_ok && d->tables.gout_par) rc = repair_full(&done);
            if (rc != FASTECC_OK || done) return rc;
        }
        if (d->pattern.erased_data != 0) {
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
        launch_rows(split_small_gather_kernel<4>, split_small_gather_kernel<1>, N >> d->split.shift, S, {parity, d->split.small_buf}, st, parity, d->split.small_buf,
                    d->tables.fin, S, (int)d->split.shift, c->fold, (uint32_t)c->Mu);
        HIP_TRY(hipGetLastError());
        const int rc = transform_bitrev(d->split.small[d->split.shift], d->split.small_buf, d->split.small_buf, false, true, S, st);
        if (rc != FASTECC_OK) return rc;
        return run_split_decode(d->split.ctx, data, nullptr, d->split.rows_data, nullptr, 0, d->split.pos_parity, d->tables.recovered, nullptr, nullptr, d->split.rows_out,
                                data, nullptr, (uint32_t)c->K, (uint32_t)c->Mu, st, odd, d->split.small_buf, d->split.shift);
    }

    // fastecc_repair through the split transform: the data chain as in fastecc_decode, and a second MID + DIT over the same two halves for x p'(x)
    // at the odd positions — the lost parity blocks, written straight into the parity stripe.  No room for the extra k-block stripe, or a plan the
    // form does not take: *done stays false.
    int repair_split(bool* done)
    {
        if (d->split.q2.try_alloc(N * S) != hipSuccess) {
            (void)hipGetLastError();
            return FASTECC_OK;
        }
        const SplitRepair odd{d->split.q2, d->split.pos_data_odd, d->split.rows_out_parity, parity_out};
        d->split.dirty = std::max(d->split.dirty, d->split.groups);  // (before the launches: a failure half way must not hide written groups)
        ProfScope ps(c, st, "repair_split_transform", (5 * N + (uint64_t)d->split.groups * split_decode_group_rows(d->split.ctx)) * block);
        const int rc = d->split.shift != 0 ? split_small(&odd)
                                           : run_split_decode(d->split.ctx, data, parity, d->split.rows_data, d->split.rows_parity, d->split.groups, d->split.pos_parity,
                                                              d->tables.recovered, d->split.r1, d->split.r2, d->split.rows_out, data, d->split.impulse,
                                                              (uint32_t)c->K, (uint32_t)c->Mu, st, &odd);
        if (rc == FASTECC_E_UNSUPPORTED) return FASTECC_OK;
        *done = rc == FASTECC_OK;
        return rc;
    }

    // fastecc_repair, (2k,k) layout: x p'(x) at all 2k positions — the even rows give the lost data, the odd rows the lost parity.  No room for
    // the 2k-block stripe, or a plan whose first pass cannot read the codeword: *done stays false.
    int repair_full(bool* done)
    {
        if (d->tables.recovered_full.try_alloc(d->pattern.positions * S) != hipSuccess) {
            (void)hipGetLastError();
            return FASTECC_OK;
        }
        const int rc = run_gathered(d->tables.transform_full, data, parity, d->tables.fin_first_pass, d->tables.recovered_full, st);
        if (rc != FASTECC_OK) return rc == FASTECC_E_UNSUPPORTED ? FASTECC_OK : rc;
        launch_rows(decode_scatter_kernel<4>, decode_scatter_kernel<1>, N, S, {data, parity_out, d->tables.recovered_full}, st, d->tables.recovered_full, data, d->tables.gout, S, 2u * S, S);
        launch_rows(decode_scatter_kernel<4>, decode_scatter_kernel<1>, N, S, {data, parity_out, d->tables.recovered_full}, st, d->tables.recovered_full + S, parity_out, d->tables.gout_par,
                    S, 2u * S, S);
        HIP_TRY(hipGetLastError());
        *done = true;
        return FASTECC_OK;
    }

    // The lost data through the split transform (two half-size transforms instead of one of size 2k, see "even / odd split"), whose last pass
    // writes the rebuilt blocks straight into the data stripe.  FASTECC_E_UNSUPPORTED: not on this plan, or no room for the staging stripe.
    int decode_split()
    {
        if (d->split.shift != 0) {
            ProfScope ps(c, st, "decode_split_transform", (3 * N + 3 * (N >> d->split.shift)) * block);
            return split_small(nullptr);
        }
        if (c->fold > 0 && d->split.r0.try_alloc(N * S) != hipSuccess) {
            (void)hipGetLastError();
            return FASTECC_E_UNSUPPORTED;
        }
        ProfScope ps(c, st, "decode_split_transform", (3 * N + (uint64_t)d->split.groups * split_decode_group_rows(d->split.ctx)) * block);
        const uint32_t* parity_half = parity;
        uint32_t parity_half_blocks = (uint32_t)c->Mu;
        if (c->fold > 0) {
            // fewer parity blocks than data blocks: block j belongs at j << fold of the parity half — the blocks in use are copied there
            launch_rows(split_stage_kernel<4>, split_stage_kernel<1>, c->Mu, S, {parity, d->split.r0}, st, parity, d->split.r0, d->tables.fin, S, c->fold);
            parity_half = d->split.r0;
            parity_half_blocks = (uint32_t)N;
        }
        d->split.dirty = std::max(d->split.dirty, d->split.groups);  // (before the launches, as in repair_split)
        return run_split_decode(d->split.ctx, data, parity_half, d->split.rows_data, d->split.rows_parity, d->split.groups, d->split.pos_parity, d->tables.recovered,
                                d->split.r1, d->split.r2, d->split.rows_out, data, d->split.impulse, (uint32_t)c->K, parity_half_blocks, st);
    }

    // The lost data blocks: the split transform, else the 2k-point one.  The (2k,k) layout lets the transform's first pass read the two halves of
    // the codeword itself (no gather pass).  The other codes do not hold every position in memory: they take the table-driven gather, which never
    // touches a position whose factor is zero, instead of a tile that reads first and multiplies by zero afterwards.
    int decode_data()
    {
        int rc = d->split.ready ? decode_split() : FASTECC_E_UNSUPPORTED;
        if (rc == FASTECC_OK) return FASTECC_OK;
        if (rc == FASTECC_E_UNSUPPORTED && d->pattern.standard) {
            ProfScope ps(c, st, "decode_transform_2k", 3 * N * block);
            rc = run_gathered(d->tables.transform, data, parity, d->tables.fin_first_pass, d->tables.recovered, st);
        }
        const bool fused = rc == FASTECC_OK;
        if (!fused && rc != FASTECC_E_UNSUPPORTED) return rc;
        uint32_t* work = d->tables.recovered;
        if (!d->pattern.mixed && !fused && (rc = scratch_of(d->tables.transform, &work)) != FASTECC_OK) return rc;  // (only the unfused form gathers into it)
        if (!fused) {
            launch_rows(decode_gather_kernel<4>, decode_gather_kernel<1>, d->pattern.positions, S, {data, parity, work, d->tables.recovered}, st, data, parity, work, d->tables.fin,
                        d->tables.srcmap, S, S, S);
            HIP_TRY(hipGetLastError());
            rc = fastecc_encode(d->tables.transform, work, d->pattern.mixed ? work : d->tables.recovered, FASTECC_MEM_DEVICE, st);
            if (rc != FASTECC_OK) return rc;
        }
        // (mixed radix: data position i is row 2i of the transformed work stripe)
        launch_rows(decode_scatter_kernel<4>, decode_scatter_kernel<1>, N, S, {data, parity, work, d->tables.recovered}, st, d->tables.recovered, data, d->tables.gout, S,
                    d->pattern.mixed ? 2u * S : S, S);
        HIP_TRY(hipGetLastError());
        return FASTECC_OK;
    }

    // The lost parity blocks are whatever the encoder makes of the (now complete) data: one more encode into a stripe of the decoder's, from which
    // only the lost blocks are copied — the surviving ones are left as they are
    int reencode_parity()
    {
        RC_TRY(d->tables.parity_again.alloc(c->Mu * S));
        const int rc = encode_device(c, data, d->tables.parity_again, st);
        if (rc != FASTECC_OK) return rc;
        launch_rows(restore_parity_kernel<4>, restore_parity_kernel<1>, c->Mu, S, {parity_out, d->tables.parity_again}, st, d->tables.parity_again, parity_out, d->tables.parity_lost, S);
        HIP_TRY(hipGetLastError());
        return FASTECC_OK;
    }

    // FASTECC_MEM_HOST: the rebuilt blocks back to the caller's stripes.  rows_only: packed side by side on the device, one copy into a pinned
    // landing buffer, and a memcpy per block on the host — the repair has already run, so if one of the buffers of this shortcut cannot be had the
    // whole stripes go back instead.
    int copy_back(void* host_data, void* host_parity, bool rows_only)
    {
        const uint64_t nd = d->pattern.erased_data != 0 ? d->host.lost_data.size() : 0, np = rebuild ? d->host.lost_parity.size() : 0;
        if (rows_only && d->host.lost_rows_dev.try_grow(nd + np) == hipSuccess && d->host.pack_dev.try_grow((nd + np) * S) == hipSuccess &&
            d->host.pack_host.try_grow((nd + np) * S) == hipSuccess) {
            if (nd) HIP_TRY(hipMemcpyAsync(d->host.lost_rows_dev, d->host.lost_data.data(), nd * 4, hipMemcpyHostToDevice, st));
            if (np) HIP_TRY(hipMemcpyAsync(d->host.lost_rows_dev + nd, d->host.lost_parity.data(), np * 4, hipMemcpyHostToDevice, st));
            if (nd)
                launch_rows(pack_rows_kernel<4>, pack_rows_kernel<1>, nd, S, {data, d->host.parity_dev, d->host.pack_dev}, st, (const uint32_t*)data, d->host.lost_rows_dev,
                            d->host.pack_dev, S);
            if (np)
                launch_rows(pack_rows_kernel<4>, pack_rows_kernel<1>, np, S, {data, d->host.parity_dev, d->host.pack_dev}, st, (const uint32_t*)d->host.parity_dev,
                            d->host.lost_rows_dev + nd, d->host.pack_dev + nd * S, S);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(d->host.pack_host, d->host.pack_dev, (nd + np) * (size_t)S * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            for (uint64_t r = 0; r < nd; r++) memcpy((char*)host_data + (size_t)d->host.lost_data[r] * block, d->host.pack_host + r * S, block);
            for (uint64_t r = 0; r < np; r++) memcpy((char*)host_parity + (size_t)d->host.lost_parity[r] * block, d->host.pack_host + (nd + r) * S, block);
            return FASTECC_OK;
        }
        if (rows_only) (void)hipGetLastError();  // out of memory for the shortcut only
        if (d->pattern.erased_data != 0) {
            const int rc = stage_download(c, host_data, data, c->K * block, st);
            if (rc != FASTECC_OK) return rc;
        }
        if (rebuild) {
            const int rc = stage_download(c, host_parity, d->host.parity_dev, c->Mu * block, st);
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
    if (!d || !d->pattern.ready) return FASTECC_E_INVAL;  // fastecc_decode_prepare first
    const bool rebuild = parity_out != nullptr && d->pattern.erased_parity != 0;
    if (d->pattern.erased_data == 0 && !rebuild) return FASTECC_OK;
    if (c->ld != c->S) return FASTECC_E_UNSUPPORTED;  // the gather / scatter passes address contiguous stripes
    DeviceGuard dg(c->device);
    if (!dg.ok) return FASTECC_E_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    return with_internal_buffers(c, st, [&]() -> int {  // the decoder's work stripes and tables are internal buffers
        StripeDecode j{c, d, st, rebuild, (uint32_t*)data, (const uint32_t*)parity, (uint32_t*)parity_out, transform_order(c), c->S * 4, (uint32_t)c->S};
        const bool host = mem_kind == FASTECC_MEM_HOST;
        bool rows_only = false;
        if (host) RC_TRY(j.stage_host(data, parity, &rows_only));
        RC_TRY(d->pattern.direct_path ? j.direct() : j.transform());
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
    if (!d || !d->pattern.ready) return FASTECC_E_INVAL;  // fastecc_decode_prepare first
    const bool rebuild = repair && d->pattern.erased_parity != 0;
    if (d->pattern.erased_data == 0 && !rebuild) return FASTECC_OK;
    DeviceGuard dg(c->device);
    if (!dg.ok) return FASTECC_E_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    if (!d->pattern.direct_path) {
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
        const bool batched = mode == 1 || (mode == 0 && d->pattern.direct_kernel != 2 && rows < 4096 && direct_batch_waves(p, ddata, dparity, S, count) >= 1024);
        if (batched) {
            const uint64_t outputs = (data_to ? (uint64_t)d->few.direct.ed : 0) + (par_to ? (uint64_t)d->few.direct.ep : 0);
            ProfScope ps(c, st, dev_list ? "direct_pass_list" : "direct_pass_batch", count * (rows + outputs) * block);
            return direct_run_batch(p, ddata, par_in, data_to, par_to, S, count, data_words, parity_words, st, dev_list);
        }
        ProfScope ps(c, st, "direct_pass", count * (c->K + (uint64_t)d->few.direct.ed) * block);
        for (uint64_t b = 0; b < count; b++) {
            const uint64_t sb = stripe_of(b);
            RC_TRY(direct_run(p, ddata + sb * data_words, par_in ? par_in + sb * parity_words : nullptr, data_to ? data_to + sb * data_words : nullptr,
                              par_to ? par_to + sb * parity_words : nullptr, (uint32_t)S, d->pattern.direct_kernel, st));
        }
        return FASTECC_OK;
    };
    return with_internal_buffers(c, st, [&] { return direct_passes(d, rebuild, ddata, dparity, dparity, run); });
}

}  // namespace

int repair_list(fastecc_ctx* c, void* data, void* parity, const uint64_t* host_list, const uint64_t* dev_list, uint64_t count, void* stream)
{
    if (!host_list || !dev_list) return FASTECC_E_INVAL;
    return decode_batch_impl(c, data, parity, count, stream, true, host_list, dev_list);
}

}  // namespace fastecc

using namespace fastecc;

extern "C" {

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

}  // extern "C"
