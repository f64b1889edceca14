// pool_encode.hip — the parity of a POOL of stripes on the matrix cores, one launch per sweep of outputs (fastecc_encode_pool, option
// "encode_pool_kernel" = 2; the routing is encode.hip's encode_pool_device).
//
//   parity[b][j][col] = sum_i  w[i][j] * data[b][i][col]   (mod p = 0xFFF00001),   b < count stripes,  i < k,  j < n - k,  col < S
//
// The arithmetic is direct.hip's MFMA form: data words and weights cut into signed base-256 digits, k' = (row, digit of the word) the contraction
// index and (output, digit of 256^a w) the M index of v_mfma_i32_32x32x32_i8, exact i32 digit sums, one reduction mod p at the end.  What differs
// is the shape.  direct_mfma_kernel cuts ONE long stripe into chunks of rows with partial sums, two reduce kernels and LDS-staged fragments; a pool
// has many short stripes (k = 16: two 8-row steps), so here a wave owns (stripe, 64 word columns), walks ALL rows of its stripe and stores canonical
// words straight into the parity blocks: no partial sums, no reduce kernels, no LDS, no barriers.  The weight fragments ((k / 8) * MT KiB per sweep,
// the same for every stripe) come straight from global memory and stay in L2.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "internal.hpp"
#include "mfma_digits.hpp"

namespace fastecc {

namespace {

constexpr uint64_t POOL_LAUNCH_WAVES = 1ull << 24;  // 2^30 work-items: a dispatch holds fewer than 2^32 per dimension (as direct_run_batch)
// Rows per stripe the i32 digit sums take: a product of two digits is at most 2^14 in magnitude, an accumulator receives 4 of them per row (the
// four digits of the row's word), so after k rows it holds at most k * 2^16 — below the 2^28 digit_sums_to_word takes for k < 4096.
constexpr uint64_t POOL_MAX_ROWS = 4096;

struct PoolArgs {
    const uint32_t* data;  // stripe b's k rows at data + b * k * S
    uint32_t* parity;      // its n - k outputs at parity + b * outputs * S
    const uint4* frag;     // [steps][mt_total][64]: mfma_weights_kernel's fragments, zero for rows >= k and outputs >= `outputs`
    uint32_t S, k, outputs, mt_total, steps, waves_per_stripe;
    uint32_t waves;        // count * waves_per_stripe
};

// A wave = (stripe b, columns [64 cc, 64 cc + 64)) as two 32-column N-tiles in direct_mfma_kernel's operand layout: lane n = l & 31 holds columns
// 2n, 2n + 1 (one dwordx2 per row; N-tile 0 the even, N-tile 1 the odd columns), lanes 32-63 the rows 4 further down.  Rows are read through one
// raw buffer descriptor per stripe of exactly k * S * 4 bytes, every byte of the offset in the VGPR: the rows 8 ks + 4 half + i >= k of the last
// step lie at or beyond the descriptor's end and read as zero instead of reaching into the next stripe (or past the pool).  Lanes whose columns
// are >= S read column 0 and store nothing.  A sweep (blockIdx.y) is MT M-tiles = 8 MT outputs; step ks + 1 is requested before step ks is used.
// Waves per SIMD asked of the register allocator: 6 / 3 / 2 for 32 / 64 / 128 accumulator registers — a stripe of k = 16 is two steps, so it is
// the other waves of the SIMD, not the one-step prefetch, that cover the latency of the rows.
template <int MT>
__global__ __launch_bounds__(256, (MT == 1 ? 6 : MT == 2 ? 3 : 2)) void pool_encode_mfma_kernel(const PoolArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (w >= a.waves) return;
    const uint32_t b = w / a.waves_per_stripe, cc = w - b * a.waves_per_stripe;
    const uint32_t sweep = blockIdx.y;
    const uint32_t n = lane & 31u, half = lane >> 5;
    const uint32_t col = cc * 64u + 2u * n;
    const bool live = col < a.S;  // (S is even: col + 1 < S as well)
    const uint32_t row_bytes = a.S * 4u;
    const uint32_t voff = 4u * half * row_bytes + 4u * (live ? col : 0u);
    const __amdgpu_buffer_rsrc_t rows_desc = direct_desc(a.data + (size_t)b * a.k * a.S, a.k * row_bytes);
    const uint4* frag = a.frag + ((size_t)sweep * MT) * 64u + lane;
    const size_t step_frags = (size_t)a.mt_total * 64u;
    v16i acc[MT][2];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][c][r] = 0;
    v2u x[4];
    uint4 af[MT];
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = __builtin_amdgcn_raw_buffer_load_b64(rows_desc, voff + (uint32_t)i * row_bytes, 0, 0);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) af[mt] = frag[mt * 64];
    for (uint32_t ks = 0; ks < a.steps; ++ks) {
        v2u xn[4];
        uint4 afn[MT];
#pragma unroll
        for (int i = 0; i < 4; ++i) xn[i] = x[i];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) afn[mt] = af[mt];
        if (ks + 1 < a.steps) {  // wave-uniform
#pragma unroll
            for (int i = 0; i < 4; ++i) xn[i] = __builtin_amdgcn_raw_buffer_load_b64(rows_desc, voff + (8u * (ks + 1) + (uint32_t)i) * row_bytes, 0, 0);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) afn[mt] = frag[(size_t)(ks + 1) * step_frags + mt * 64];
        }
        v4i bf[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bf[0][i] = (int)balanced_digits(x[i][0]);
            bf[1][i] = (int)balanced_digits(x[i][1]);
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            v4i av;
            av[0] = (int)af[mt].x; av[1] = (int)af[mt].y; av[2] = (int)af[mt].z; av[3] = (int)af[mt].w;
            acc[mt][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bf[0], acc[mt][0], 0, 0, 0);
            acc[mt][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bf[1], acc[mt][1], 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = xn[i];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) af[mt] = afn[mt];
    }
    // D: column n = lane & 31, row m = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) = 4 j' + digit: registers 4 q .. 4 q + 3 of a lane are the four
    // digit sums of output j' = 2 q + half of the M-tile
    uint32_t* prow = a.parity + (size_t)b * a.outputs * a.S + col;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t r[2];
#pragma unroll
            for (int c = 0; c < 2; ++c)
                r[c] = digit_sums_to_word(acc[mt][c][4 * q], acc[mt][c][4 * q + 1], acc[mt][c][4 * q + 2], acc[mt][c][4 * q + 3]);
            const uint32_t out = (sweep * MT + mt) * 8u + 2u * q + half;
            if (live && out < a.outputs) *reinterpret_cast<uint2*>(prow + (size_t)out * a.S) = make_uint2(r[0], r[1]);
            __builtin_amdgcn_sched_barrier(0);  // one output at a time: the accumulators are not all read out before the first store
        }
}

}  // namespace

// 8 / 16 / 32 outputs per wave and sweep: the fewest M-tiles that hold the code's n - k outputs, at most 4 (128 accumulator registers)
int pool_encode_mfma_tiles(uint64_t outputs) { return outputs <= 8 ? 1 : outputs <= 16 ? 2 : 4; }

// What the kernel needs: rows of whole dwordx2 (S even, both pools 8-byte aligned; a stripe is k * S words, so every stripe then is), at least one
// full wave of columns, k within the digit bound, a stripe — with the up to 7 rows the last step addresses beyond it — within the 32-bit offset of
// one buffer descriptor, and the pool's waves within one dispatch.
bool pool_encode_mfma_applies(const void* data, const void* parity, uint64_t k, uint64_t words, uint64_t count)
{
    if ((words % 2) != 0 || words < 64 || ((((uintptr_t)data | (uintptr_t)parity) & 7u) != 0)) return false;
    if (k < 1 || k >= POOL_MAX_ROWS || (k + 8) * words * 4 >= (1ull << 32)) return false;
    return count <= POOL_LAUNCH_WAVES / ((words + 63) / 64);
}

int pool_encode_mfma_run(const uint4* frag, uint32_t mt_total, int mt, const uint32_t* data, uint32_t* parity, uint32_t k, uint32_t outputs, uint32_t words,
                         uint64_t count, hipStream_t st)
{
    if (!frag || !pool_encode_mfma_applies(data, parity, k, words, count) || outputs < 1 || mt_total < 1 || (mt_total % mt) != 0 ||
        (uint64_t)mt_total * 8u < outputs)
        return FASTECC_E_INVAL;
    const uint32_t wps = (words + 63u) / 64u;
    const PoolArgs a{data, parity, frag, words, k, outputs, mt_total, (k + 7u) / 8u, wps, (uint32_t)(count * wps)};
    const dim3 grid((a.waves + 3u) / 4u, mt_total / (uint32_t)mt);
    switch (mt) {
        case 1: hipLaunchKernelGGL(pool_encode_mfma_kernel<1>, grid, dim3(256), 0, st, a); break;
        case 2: hipLaunchKernelGGL(pool_encode_mfma_kernel<2>, grid, dim3(256), 0, st, a); break;
        case 4: hipLaunchKernelGGL(pool_encode_mfma_kernel<4>, grid, dim3(256), 0, st, a); break;
        default: return FASTECC_E_INVAL;
    }
    HIP_TRY(hipGetLastError());
    return FASTECC_OK;
}

}  // namespace fastecc
