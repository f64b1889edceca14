"""An exact model of the scrub fingerprint pass (block_fingerprint in fastecc_amd/csrc/scrub.hip), for the tests that read its numbers.

The pass computes, per block r of S 32-bit words and column c < 3, F_c = sum_w rho_c[w] * r[w] mod p, p = 0xFFF00001.  The weights are
the contract fastecc_scrub_fingerprints states (include/fastecc.h): weight word w comes from the w-th splitmix64 output x of the state
started at `seed`, rho_0 = x & 0xFFFFF, rho_1 = (x >> 20) & 0xFFFFF, rho_2 = (x >> 40) & 0xFFFFF; r[w] is the word as stored, words >= p
included.  The device keeps 64-bit sums per lane and folds them every 4096 products; lane_sums gives those sums WITHOUT the folds, as
Python integers, so that a test can prove that an input overflows 64 bits unless the fold happens.

Everything here is exact integer arithmetic (numpy uint64 where the bound is written next to it, Python integers else); nothing of the
library is used.  Plain helper module (no fixtures, no tests), like tests/p32_edges.py."""
import numpy as np

P = 0xFFF00001
MASK20 = 0xFFFFF
VECTOR, SCALAR = "vector", "scalar"
LANES = 64


def weights(seed, S):
    """[S, 3] uint64: rho_c[w].  State w of splitmix64 is seed + (w + 1) * 0x9E3779B97F4A7C15 mod 2^64 (uint64 arrays wrap), so the
    weights of a shorter block are a prefix of those of a longer one."""
    z = np.arange(1, S + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.full(S, seed % (1 << 64), dtype=np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    x = z ^ (z >> np.uint64(31))
    m = np.uint64(MASK20)
    return np.stack([x & m, (x >> np.uint64(20)) & m, (x >> np.uint64(40)) & m], axis=1)


def fingerprints(blocks, seed, w=None):
    """[..., 3] uint32: F_c of every block of `blocks` ([..., S] uint32), canonical.  w: weights(seed, S) if the caller has them already.
    A product is < 2^20 * 2^32 = 2^52 and is reduced at once; a sum of S < 2^20 residues is < 2^52."""
    blocks = np.asarray(blocks)
    assert blocks.dtype == np.uint32
    S = blocks.shape[-1]
    assert S < (1 << 20)
    if w is None:
        w = weights(seed, S)
    assert w.shape == (S, 3) and w.dtype == np.uint64
    r = blocks.astype(np.uint64)
    out = np.empty(blocks.shape[:-1] + (3,), np.uint32)
    for c in range(3):
        out[..., c] = (((r * w[:, c]) % np.uint64(P)).sum(axis=-1, dtype=np.uint64) % np.uint64(P)).astype(np.uint32)
    return out


def lane_of(word, form):
    """The lane whose sums word `word` of a block joins: the vector form reads 4 words per lane and 256 per wave and load, the scalar one."""
    if form == VECTOR:
        return (word % 256) // 4
    assert form == SCALAR
    return word % LANES


def lane_sums(block, w, form):
    """[64][3] Python integers: the sums of rho_c[word] * block[word] over the words of each lane, unfolded and unreduced.  w = weights(seed, S)."""
    block = np.asarray(block)
    assert block.dtype == np.uint32 and block.ndim == 1 and w.shape == (block.shape[0], 3)
    S = block.shape[0]
    per_row = 256 if form == VECTOR else LANES
    rows = -(-S // per_row)
    sums = [[0, 0, 0] for _ in range(LANES)]
    for c in range(3):
        prod = np.zeros(rows * per_row, np.uint64)
        prod[:S] = block.astype(np.uint64) * w[:, c]  # < 2^52
        # the 32-bit halves apart: each column sum is < 2^20 rows * 4 * 2^32 = 2^54
        lo = (prod & np.uint64(0xFFFFFFFF)).reshape(rows, per_row).sum(axis=0, dtype=np.uint64)
        hi = (prod >> np.uint64(32)).reshape(rows, per_row).sum(axis=0, dtype=np.uint64)
        for i in range(per_row):
            sums[lane_of(i, form)][c] += (int(hi[i]) << 32) + int(lo[i])
    return sums
