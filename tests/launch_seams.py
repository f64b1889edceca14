"""Pools that make one pool call take several launches, and the arithmetic that says where the launches meet.

A dispatch holds fewer than 2^32 work-items per dimension, so the batched launchers cut one call into launches of at most 2^24 waves (2^30 lane
groups) and hand every launch after the first a base index.  The limits are restated here (LIMITS: name -> (file, value));
tests/test_launch_seams_host.py finds each constexpr by its name in that file, so whoever changes a limit is told that the seam tests
(tests/test_gpu_launch_seams.py) no longer cross it.

  limit                    launcher                                        what only a later launch uses
  LAUNCH_GROUPS            direct_run_batch (decode_batch, repair_batch,   a.group_base
                           encode_pool's VALU kernel)
  SET_LAUNCH_WAVES         direct_run_set (decode_batch_set,               a.entries = entries + e0
                           repair_batch_set, grouped repair)
  SET_LAUNCH_WAVES         direct_run_read (read_batch, read_batch_set)    a.entries, a.row_base = e0
  LAUNCH_WAVES             launch_split, for update_batch_run              a.segs + s0 * (SEG_HEAD + T), ca.list + w0 * LIST_WORDS
                           (update_batch, update_parity_batch)
  POOL_LAUNCH_WAVES        pool_encode_mfma_applies (encode_pool's         no second launch: past the limit the call takes the VALU kernel
                           matrix-core kernel)
  MAX_LAUNCH_WAVES         encode_batch_passes (encode_batch, the (2k,k)   data + b0 * stride, parity + b0 * stride, batch = b1 - b0
                           branch of encode_pool)

THE POOL is periodic with a prime period of T = 4099 stripes.  Word columns of a stripe are independent codewords, so the parity of a TILE of T
stripes is ONE call of pool_model.Codec.parity on a (k, T * S) array — column t * S + c is word c of stripe t — and the device pool is the tile
repeated and cut at `count` stripes.  4099 divides no launch size, so every seam falls inside a tile: a stripe computed from a neighbour's rows,
or written one entry off, or a launch that starts over at entry 0, gives a pool that differs from the tile's repetition.  The expected words are
the oracle's; the library's own per-stripe calls are no reference here.

Plain numpy / torch helpers (no fixtures, no tests), like tests/p32_edges.py; torch is handed in by the caller."""
import math

import numpy as np

from pool_model import Codec

P = 0xFFF00001
T = 4099                     # stripes per tile: prime, coprime to every launch size
LOST = 0xA5A5A5A5 - (1 << 32)    # what a block named lost holds before the call, as the int32 the device tensors hold (>= p: no word of the truth)
CANARY = 0xFFFA5A5A - (1 << 32)  # the row beyond the end of every buffer a call writes
NONE_EVERY = 97              # the set cases name every 97th stripe FASTECC_PATTERN_NONE

# name -> (file under fastecc_amd/csrc, value)
LIMITS = {
    "LAUNCH_GROUPS": ("direct.hip", 1 << 30),         # lane groups per launch of direct_batch_kernel (in direct_run_batch)
    "SET_LAUNCH_WAVES": ("direct.hip", 1 << 24),      # waves per launch of direct_set_kernel and direct_read_kernel
    "LAUNCH_WAVES": ("update.hip", 1 << 24),          # waves per launch of update_batch_kernel and update_scatter_kernel
    "POOL_LAUNCH_WAVES": ("pool_encode.hip", 1 << 24),   # waves of the one launch of pool_encode_mfma_kernel
    "MAX_LAUNCH_WAVES": ("launch_limits.hpp", 1 << 24),  # waves per pass of one run of stripes on the transform path
}
LAUNCH_GROUPS, SET_LAUNCH_WAVES, LAUNCH_WAVES, POOL_LAUNCH_WAVES, MAX_LAUNCH_WAVES = (LIMITS[name][1] for name in LIMITS)


# ---- the launchers' own arithmetic (device pools are at least 16-byte aligned) ----
def set_waves_per_entry(eb, S):
    """direct.hip: lane_words and direct_set_waves_per_entry for pad class eb"""
    v = 4 if eb <= 4 else 2 if eb == 8 else 1
    while v > 1 and S % v:
        v >>= 1
    while v > 1 and S < 64 * v:
        v >>= 1
    return -(-S // (64 * v))


def read_waves_per_entry(S, col0, width):
    """direct.hip: lane_words and direct_read_waves_per_entry"""
    v = 4
    while v > 1 and (S % v or col0 % v or width % v):
        v >>= 1
    while v > 1 and width < 64 * v:
        v >>= 1
    return -(-width // (64 * v))


def batch_groups(eb, S, count):
    """direct.hip: lane_words and BatchArgs::groups"""
    v = 4 if eb <= 4 else 2 if eb == 8 else 1
    while v > 1 and S % v:
        v >>= 1
    return count * S // v


# ---- the shapes of the cases: each crosses its seam by more than 1000 entries unless it says otherwise ----
# The set cases skip every 97th stripe (FASTECC_PATTERN_NONE), and only stripes with work become entries: 2^24 + 2^16 stripes would leave
# 16 669 115 entries, fewer than the 2^24 a launch holds.  The counts are therefore the next powers of two that put the ENTRIES past the seam:
# 2^24 + 2^18 stripes (16 863 696 entries) and floor(2^24 / 3) + 2^16 stripes (5 599 611 entries, the seam at 5 592 405).
SET_A = dict(n=6, k=4, S=1, count=(1 << 24) + (1 << 18))     # one wave per entry: 2^24 entries per launch
SET_B = dict(n=3, k=2, S=129, count=(1 << 24) // 3 + (1 << 16))  # three waves per entry: floor(2^24 / 3) entries per launch
READ = dict(n=20, k=16, S=192, count=64, down=7, stride=389, extra=37)
READ_WINDOWS = ((1, 1), (1, 129))                          # (col0, width): one wave and three waves per request
WRITES = dict(n=6, k=4, S=1, count=(1 << 24) + (1 << 13))
GROUPS = dict(n=3, k=2, S=1, count=(1 << 30) + T + 3)
MFMA = dict(n=3, k=2, S=64, count=1 << 24)
# the plan of each, the profile scope of its one pass and the waves that pass takes per stripe (a register pass of one wave; a 64-block tile of two)
TRANSFORM = (dict(n=4, k=2, S=1, count=(1 << 26) + T, plan="mid1@0 v1", scope="mid1v1", stripe_waves=1),
             dict(n=128, k=64, S=1, count=(1 << 24) + T, plan="T64:mid6@0 v1", scope="tile_mid6_w64", stripe_waves=2))

# ---- one launch (launch_limits.hpp): a dispatch holds fewer than 2^32 work-items; a single stripe cannot be cut, so this is where it is refused ----
MAX_DISPATCH_THREADS = (1 << 32) - 1


def dispatch_fits(workgroups, threads):
    return 0 < workgroups <= MAX_DISPATCH_THREADS // threads


def wave_launch_fits(waves):
    """the register passes and the row kernels: one wave per item, workgroups of four waves"""
    return dispatch_fits(-(-waves // 4), 256)


def rows_waves(S, vec, rows):
    return -(-S // (64 * vec)) * rows


def with_work(count):
    """stripes of a set case that are not named FASTECC_PATTERN_NONE"""
    return count - -(-count // NONE_EVERY)


def launch_sizes():
    """every number of entries (stripes, requests, writes) after which some case's launcher starts a new launch"""
    sizes = {LAUNCH_GROUPS, SET_LAUNCH_WAVES, SET_LAUNCH_WAVES // 3, LAUNCH_WAVES, POOL_LAUNCH_WAVES}
    sizes |= {MAX_LAUNCH_WAVES // w for w in (1, 2)}  # (4,2): one wave per stripe; (128,64): a tile of two waves per stripe
    return sorted(sizes)


# ---- tiles ----
def draw_tile(seed, k, S, period=T):
    """(k, period * S) words below p; the first columns hold the field's edges"""
    x = np.random.default_rng(seed).integers(0, P, size=(k, period * S), dtype=np.uint64).astype(np.uint32)
    x[0, :4] = [0, 1, P - 1, 0x000FFFFF]
    return x


def tile_parity(oracle, n, k, x):
    """the oracle's parity of every stripe of the tile, in ONE call: (n - k, period * S)"""
    return Codec(oracle, n, k).parity(x)


def tile_to_stripes(a, S):
    """(rows, period * S) -> (period, rows, S): the pool layout of the tile's stripes"""
    rows, cols = a.shape
    assert cols % S == 0
    return np.ascontiguousarray(a.reshape(rows, cols // S, S).transpose(1, 0, 2))


def to_device(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to("cuda:0")


def periodic_pool(torch, tile, count, guard=CANARY):
    """device (count + 1, rows, S): the tile (period, rows, S) repeated and cut at `count` stripes, then one guard stripe"""
    period, shape = tile.shape[0], tuple(tile.shape[1:])
    out = torch.empty((count + 1,) + shape, dtype=tile.dtype, device=tile.device)
    full = count // period
    if full:
        out[:full * period].view((full, period) + shape).copy_(tile.unsqueeze(0).expand((full, period) + shape))
    if count > full * period:
        out[full * period:count] = tile[:count - full * period]
    out[count:] = guard
    return out


def equal_periodic(torch, pool, tile, count, guard=CANARY, chunk_words=1 << 27):
    """pool (at least count + 1 stripes) == periodic_pool(tile, count) followed by guard words only — every word compared on the device, a run
    of whole tiles at a time, without building the expected pool (the 8 GiB pools)"""
    period, shape = tile.shape[0], tuple(tile.shape[1:])
    full = count // period
    step = max(1, chunk_words // max(1, tile.numel()))
    for r0 in range(0, full, step):
        r = min(step, full - r0)
        if not bool((pool[r0 * period:(r0 + r) * period].view((r, period) + shape) == tile).all()):
            return False
    rest = count - full * period
    if rest and not torch.equal(pool[full * period:count], tile[:rest]):
        return False
    return bool((pool[count:] == guard).all())


def flag_rows(k, m, patterns):
    """(P x k, P x m) presence flags of patterns given as (lost data blocks, lost parity blocks)"""
    dp, pp = np.ones((len(patterns), k), np.uint8), np.ones((len(patterns), m), np.uint8)
    for q, (ld, lp) in enumerate(patterns):
        dp[q, list(ld)] = 0
        pp[q, list(lp)] = 0
    return dp, pp


# ---- case d: the writes and the tiles of the truth after each burst ----
def burst1(x0, new_words, k):
    """every stripe b gets block b % k rewritten with new_words[b % T] (S = 1): the truth's tile of period k * T and the write list of `count` stripes"""
    x1 = np.tile(x0, (1, k))
    t = np.arange(k * T)
    x1[t % k, t] = new_words[t % T]
    return x1


def burst1_writes(count, k):
    b = np.arange(count, dtype=np.uint64)
    return b * np.uint64(k) + b % np.uint64(k)


def burst2(x1, words_a, words_b, k):
    """the stripes with b % 3 == 0 get blocks (b + 1) % k and (b + 2) % k rewritten (words_a[b % T], words_b[b % T]): period 3 * k * T"""
    x2 = np.tile(x1, (1, 3))
    t = np.arange(0, 3 * k * T, 3)
    x2[(t + 1) % k, t] = words_a[t % T]
    x2[(t + 2) % k, t] = words_b[t % T]
    return x2


def burst2_writes(count, k):
    """(writes, stripe of each write, 0 / 1 = first or second block), last stripe first: any order is allowed"""
    b = np.arange(0, count, 3, dtype=np.uint64)[::-1]
    w = np.stack([b * np.uint64(k) + (b + np.uint64(1)) % np.uint64(k), b * np.uint64(k) + (b + np.uint64(2)) % np.uint64(k)], axis=1).reshape(-1)
    return np.ascontiguousarray(w), np.repeat(b, 2), np.tile(np.array([0, 1]), len(b))


def coprime_to_launch_sizes(period=T):
    return all(math.gcd(period, s) == 1 for s in launch_sizes())
