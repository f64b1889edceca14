// launch_limits.hpp — how large one launch of the transform path may be.  Plain C++ (no HIP): tests/test_launch_seams_host.py compiles it on the host.
#pragma once
#include <stdint.h>

namespace fastecc {

// The batched entry points (encode.hip: encode_batch_passes) cut a batch into runs of stripes whose passes take at most this many waves each
// (2^30 work-items: 2^22 workgroups of 256 threads) — the run size of direct.hip, update.hip and pool_encode.hip.  A size to split at, not a limit:
// a single stripe cannot be cut, and a launch of one may be as large as a dispatch allows (below).
constexpr uint64_t MAX_LAUNCH_WAVES = 1ull << 24;

// A dispatch holds fewer than 2^32 work-items per dimension.  What does not fit is refused with FASTECC_E_UNSUPPORTED before any device work
// (run_passes, ntt_device, fastecc_scale_blocks); the launchers of kernels.hip check again.
constexpr uint64_t MAX_DISPATCH_THREADS = (1ull << 32) - 1;
inline bool dispatch_fits(uint64_t workgroups, uint64_t threads) { return workgroups > 0 && threads > 0 && workgroups <= MAX_DISPATCH_THREADS / threads; }
// the launchers of kernels.hip: one wave per item, workgroups of four waves
inline bool wave_launch_fits(uint64_t waves) { return dispatch_fits((waves + 3u) / 4u, 256u); }

// waves of launch_bitrev_rows / launch_scale_rows over `rows` blocks of S words
inline uint64_t rows_waves(uint32_t S, int vec, uint64_t rows) { return (uint64_t)((S + 64u * vec - 1u) / (64u * vec)) * rows; }
// waves one stripe of 2^n blocks of S words takes in a register pass of 2^logr blocks per wave (launch_pass multiplies by the batch)
inline uint64_t pass_stripe_waves(int logr, int vec, uint32_t S, int n) { return n < logr ? 0 : rows_waves(S, vec, 1) << (n - logr); }

// A tile pass (tile_kernels.hip: TileCfg): one workgroup of 2^(logt - logr - pair) waves per tile of 2^logt blocks x (pair ? 32 : 64) words
inline uint64_t tile_stripe_tiles(int logt, bool pair, uint32_t S, int n)
{
    const uint32_t W = pair ? 32u : 64u;
    return n < logt ? 0 : (uint64_t)((S + W - 1u) / W) << (n - logt);
}
inline int tile_workgroup_waves(int logt, bool pair, int logr) { return 1 << (logt - logr - (pair ? 1 : 0)); }
inline uint64_t tile_stripe_waves(int logt, bool pair, int logr, uint32_t S, int n)
{
    return tile_stripe_tiles(logt, pair, S, n) * (uint64_t)tile_workgroup_waves(logt, pair, logr);
}
// Tiles of more than 80 KiB of LDS run as persistent workgroups when the context asks for them: their grid is sized to the machine, whatever the
// number of tiles.  Those are the 128 KiB shapes of launch_mode: 1024 x 32 words, and 512 x 64 words, unless the pass takes the split exchange
// (split2; outer = a DIF or DIT pass) or address windows (wide).
inline bool tile_grid_is_capped(int logt, bool pair, int logr, bool outer, bool split2, int wide, int persistent_cus)
{
    if (persistent_cus <= 0 || logr != 5 || wide) return false;
    if (logt == 10 && pair) return !split2;
    if (logt == 9 && !pair) return !(split2 && outer);
    return false;
}
inline bool tile_launch_fits(uint64_t tiles, int logt, bool pair, int logr, bool outer, bool split2, int wide, int persistent_cus)
{
    if (tiles == 0 || tiles > 0x7FFFFFFFull) return false;  // (launch_one's own check: 32-bit tile indices)
    return tile_grid_is_capped(logt, pair, logr, outer, split2, wide, persistent_cus) || dispatch_fits(tiles, 64u * (uint64_t)tile_workgroup_waves(logt, pair, logr));
}

}  // namespace fastecc
