"""GPU tests (-m gpu) of the degraded reads: fastecc_read_batch_set and fastecc_read_batch.

A pool of stripes is encoded with the library (fastecc_encode_pool), every block its stripe's pattern loses is overwritten with garbage that
includes 0xFFFFFFFF words, and a list of requested data blocks — healthy and degraded mixed, any order, duplicates — is read into a compact
buffer with canary rows before and after it.  Every row must equal the same words of the ORIGINAL data (a FASTECC_PATTERN_NONE stripe: of what
the pool holds, garbage >= p verbatim), and of what fastecc_repair_batch_set / fastecc_repair_batch rebuilds on a clone of the damaged pool; the
pool itself must equal its pre-call clone byte for byte and the canaries must be intact."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 0xFFF00001
CANARY = 0x3C3C3C3C


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def fe(hip_lib):
    import fastecc_amd
    return fastecc_amd


def flag_rows(k, m, patterns):
    dp, pp = np.ones((len(patterns), k), np.uint8), np.ones((len(patterns), m), np.uint8)
    for q, (ld, lp) in enumerate(patterns):
        dp[q, list(ld)] = 0
        pp[q, list(lp)] = 0
    return dp, pp


def garbage(torch, shape, seed):
    """arbitrary 32-bit words, every third one 0xFFFFFFFF (not a field element)"""
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    w = torch.randint(0, 1 << 32, shape, dtype=torch.int64, device="cuda:0", generator=g)
    w.view(-1)[::3] = 0xFFFFFFFF
    return (w - ((w >> 31) << 32)).to(torch.int32)  # the same 32 bits as an int32


class Pool:
    """`count` codewords [count, k, S] / [count, m, S] on the device (fastecc_encode_pool), then damaged: stripe b loses the blocks of
    patterns[pattern_of[b]] (overwritten with garbage), a PATTERN_NONE stripe holds nothing but garbage.
    want: what a read of each data block returns — the original, and for PATTERN_NONE stripes what the pool holds."""

    def __init__(self, torch, fe, enc, count, S, patterns, pattern_of, seed):
        self.torch, self.enc, self.count, self.S, self.k, self.m = torch, enc, count, S, enc.k, enc.n - enc.k
        self.patterns, self.pattern_of = patterns, list(pattern_of)
        g = torch.Generator(device="cuda:0").manual_seed(seed)
        data = torch.randint(0, P, (count, self.k, S), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32)
        parity = torch.zeros((count, self.m, S), dtype=torch.int32, device="cuda:0")
        enc.encode_pool(data, parity, count)
        torch.cuda.synchronize()
        self.D, self.Q, self.want = data.clone(), parity.clone(), data.clone()
        for b, q in enumerate(self.pattern_of):
            if q == fe.PATTERN_NONE:
                self.D[b] = garbage(torch, (self.k, S), seed * 1000 + b)
                self.Q[b] = garbage(torch, (self.m, S), seed * 1000 + b + 500)
                self.want[b] = self.D[b]
                continue
            ld, lp = patterns[q]
            if ld:
                self.D[b, list(ld)] = garbage(torch, (len(ld), S), seed * 1000 + b)
            if lp:
                self.Q[b, list(lp)] = garbage(torch, (len(lp), S), seed * 1000 + b + 500)
        torch.cuda.synchronize()
        self.D0, self.Q0 = self.D.clone(), self.Q.clone()

    def lost_data_blocks(self):
        return [b * self.k + i for b, q in enumerate(self.pattern_of) if q != 0xFFFFFFFF for i in self.patterns[q][0]]

    def check_repair(self, set_form=True):
        """the second expectation: repair on a clone of the damaged pool gives the same blocks as the original data"""
        Dr, Qr = self.D.clone(), self.Q.clone()
        if set_form:
            self.enc.repair_batch_set(Dr, Qr, self.count, np.array(self.pattern_of, np.uint32))
        else:
            self.enc.repair_batch(Dr, Qr, self.count)
        self.torch.cuda.synchronize()
        assert self.torch.equal(Dr, self.want), "repair of the damaged clone gives back the original data"
        self.repaired = Dr

    def read(self, reads, col0=0, width=None, set_form=True, out_offset=0, stream=0):
        """one read call, everything checked: rows against both expectations, the canaries, the pool"""
        torch, enc = self.torch, self.enc
        w = self.S - col0 if width is None else width
        n = len(reads)
        buf = torch.full(((n + 2) * w + 2,), CANARY, dtype=torch.int32, device="cuda:0")
        first = w + out_offset  # a canary row (and out_offset words) before the output, a canary row (and the rest) after it
        out = buf.data_ptr() + 4 * first
        if set_form:
            enc.read_batch_set(self.D, self.Q, self.count, np.array(self.pattern_of, np.uint32), reads, out, col0=col0, width=width, stream=stream)
        else:
            enc.read_batch(self.D, self.Q, self.count, reads, out, col0=col0, width=width, stream=stream)
        torch.cuda.synchronize()
        idx = torch.tensor(np.asarray(reads, dtype=np.int64), device="cuda:0")
        got = buf[first:first + n * w].view(n, w)
        what = "window (%d, %d), out offset %d" % (col0, w, out_offset)
        assert torch.equal(got, self.want.view(-1, self.S)[idx, col0:col0 + w]), what
        if hasattr(self, "repaired"):
            assert torch.equal(got, self.repaired.view(-1, self.S)[idx, col0:col0 + w]), what
        assert bool((buf[:first] == CANARY).all()) and bool((buf[first + n * w:] == CANARY).all()), "canaries, " + what
        assert torch.equal(self.D, self.D0) and torch.equal(self.Q, self.Q0), "the pool is not written, " + what
        return got


def shuffled_reads(count, k, seed, extra=64):
    """every data block of every stripe in a seeded random order, with duplicates"""
    rng = np.random.default_rng(seed)
    reads = np.concatenate([rng.permutation(count * k), rng.integers(0, count * k, extra)]).astype(np.uint64)
    rng.shuffle(reads)
    return reads


def codeword_block(k, u):
    return ([u], []) if u < k else ([], [u - k])


def two_blocks(k, n, u):
    """codeword blocks u and u + 1 (mod n): data + data, data + parity and parity + parity over the rotation"""
    a, b = codeword_block(k, u), codeword_block(k, (u + 1) % n)
    return (sorted(a[0] + b[0]), sorted(a[1] + b[1]))


# ---- 1. rotated (20,16), one and two devices down ----
WINDOWS = [(0, 1024), (0, 1), (1023, 1), (3, 5), (64, 128), (0, 255), (0, 256), (0, 257), (4, 68)]


@pytest.mark.parametrize("down", [1, 2])
def test_rotated_20_16(torch_cuda, fe, down):
    n, k, S, count = 20, 16, 1024, 40
    patterns = [codeword_block(k, u) if down == 1 else two_blocks(k, n, u) for u in range(n)]
    if down == 2:
        kinds = {(len(ld), len(lp)) for ld, lp in patterns}
        assert kinds == {(2, 0), (1, 1), (0, 2)}
    pattern_of = [fe.PATTERN_NONE if b in (7, 23, 39) else b % n for b in range(count)]
    reads = shuffled_reads(count, k, seed=down)
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        pool = Pool(torch_cuda, fe, enc, count, S, patterns, pattern_of, seed=10 + down)
        pool.check_repair()
        for col0, width in WINDOWS:
            pool.read(reads, col0, width)
        pool.read(reads, 0, None)                     # width=None: the whole block
        pool.read(reads, 0, S, out_offset=1)          # `out` 4 bytes past a 16-byte boundary: V = 1
        pool.read(reads, 64, 128, out_offset=1)
        pool.read(list(reads[:5]) + [int(reads[0])] * 3, 8, 16)  # a short list of Python ints


# ---- 2. blocks shorter than a wave ----
def test_short_blocks(torch_cuda, fe):
    n, k, S, count = 20, 16, 6, 40
    patterns = [codeword_block(k, u) for u in range(n)]
    pattern_of = [fe.PATTERN_NONE if b == 11 else (3 * b + 1) % n for b in range(count)]
    reads = shuffled_reads(count, k, seed=2)
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        pool = Pool(torch_cuda, fe, enc, count, S, patterns, pattern_of, seed=20)
        pool.check_repair()
        for col0, width in [(0, 6), (2, 3)]:
            pool.read(reads, col0, width)
            pool.read(reads, col0, width, out_offset=1)


# ---- 3. sixteen losses per pattern ----
def test_sixteen_losses(torch_cuda, fe):
    n, k, S, count = 256, 128, 64, 8
    rng = np.random.default_rng(3)
    pick = lambda total, cnt: sorted(int(x) for x in rng.permutation(total)[:cnt])  # noqa: E731
    patterns = [(pick(k, ld), pick(n - k, 16 - ld)) for ld in (8, 15, 1, 16)]
    pattern_of = [b % 4 for b in range(count)]
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        pool = Pool(torch_cuda, fe, enc, count, S, patterns, pattern_of, seed=30)
        pool.check_repair()
        reads = pool.lost_data_blocks()
        present = [b * k + i for b in range(count) for i in range(k) if i not in patterns[pattern_of[b]][0]][::97]
        reads = np.array(reads + present + reads[::5], dtype=np.uint64)
        np.random.default_rng(4).shuffle(reads)
        for col0, width in [(0, 64), (0, 63), (17, 30), (60, 4)]:
            pool.read(reads, col0, width)


# ---- 4. row counts that are no multiple of the rows in flight; every code family ----
FAMILIES = [(13, 10, 0), (80, 64, 0), (64, 16, 0), (96, 48, 1)]


@pytest.mark.parametrize("n,k,fl", FAMILIES, ids=["%d_%d" % (c[0], c[1]) for c in FAMILIES])
def test_code_families(torch_cuda, fe, n, k, fl):
    S, count = 64, 6
    patterns = [([1], []), ([0, k - 1], []), ([2], [1]), ([3, 5, 6], []), ([4], [0, 2]), ([], [1])]
    pattern_of = list(range(count))
    reads = shuffled_reads(count, k, seed=n, extra=9)
    with fe.Encoder(n, k, 4 * S, flags=fl) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        pool = Pool(torch_cuda, fe, enc, count, S, patterns, pattern_of, seed=40 + n)
        pool.check_repair()
        for col0, width in [(0, 64), (5, 7), (32, 32)]:
            pool.read(reads, col0, width)


# ---- 5. fastecc_read_batch: the single prepared pattern ----
@pytest.mark.parametrize("lost", [(18, 2), (20, 0), (0, 5)], ids=["both_pad32", "data_pad32", "parity_only"])
def test_read_batch_single_pattern(torch_cuda, fe, lost):
    """20 lost blocks: a table of pad 32 (two sweeps of outputs in the other kernels), here a column index >= 16"""
    n, k, S, count = 64, 32, 64, 16
    rng = np.random.default_rng(5)
    pattern = (sorted(int(x) for x in rng.permutation(k)[:lost[0]]), sorted(int(x) for x in rng.permutation(n - k)[:lost[1]]))
    reads = shuffled_reads(count, k, seed=5)
    with fe.Encoder(n, k, 4 * S) as enc:
        dp, pp = flag_rows(k, n - k, [pattern])
        enc.decode_prepare(dp[0], pp[0])
        pool = Pool(torch_cuda, fe, enc, count, S, [pattern], [0] * count, seed=50)
        pool.check_repair(set_form=False)
        for col0, width in [(0, 64), (3, 5), (16, 48)]:
            pool.read(reads, col0, width, set_form=False)
        pool.read(reads, 0, 64, set_form=False, out_offset=1)


def test_read_batch_k_4096(torch_cuda, fe):
    """(8192,4096): a pass of 4099 rows — the loop bound is the pass's rows"""
    n, k, S, count = 8192, 4096, 16, 2
    pattern = ([5, 2049, 4095], [])
    with fe.Encoder(n, k, 4 * S) as enc:
        dp, pp = flag_rows(k, n - k, [pattern])
        enc.decode_prepare(dp[0], pp[0])
        pool = Pool(torch_cuda, fe, enc, count, S, [pattern], [0] * count, seed=51)
        pool.check_repair(set_form=False)
        reads = np.array(pool.lost_data_blocks() + [0, 4096 + 7, 2 * 4096 - 2, 5], dtype=np.uint64)
        pool.read(reads, 0, 16, set_form=False)
        pool.read(reads, 3, 6, set_form=False)


def raw(fe, enc, set_form, data, parity, count, po, reads, n_reads, col0, width, out, stream=None):
    """the C entry point itself: its return code"""
    addr = lambda t: None if t is None else t if isinstance(t, int) else t.data_ptr()  # noqa: E731
    pr = None if reads is None else reads.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    if set_form:
        pp = None if po is None else po.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        return fe.lib().fastecc_read_batch_set(enc._h, addr(data), addr(parity), count, pp, pr, n_reads, col0, width, addr(out), stream)
    return fe.lib().fastecc_read_batch(enc._h, addr(data), addr(parity), count, pr, n_reads, col0, width, addr(out), stream)


def test_read_batch_unprepared_and_transform_path(torch_cuda, fe):
    torch = torch_cuda
    n, k, S, count = 64, 32, 64, 2
    reads = np.array([3, 35], dtype=np.uint64)  # the lost block of stripe 0 and of stripe 1
    with fe.Encoder(n, k, 4 * S) as enc:
        D = torch.zeros((count, k, S), dtype=torch.int32, device="cuda:0")
        Q = torch.zeros((count, n - k, S), dtype=torch.int32, device="cuda:0")
        out = torch.full((2, S), CANARY, dtype=torch.int32, device="cuda:0")
        assert raw(fe, enc, False, D, Q, count, None, reads, 2, 0, S, out) == fe.E_INVAL  # nothing prepared
        dp, pp = flag_rows(k, n - k, [([3], [])])
        enc.set_option("decode_direct_max", 0)  # every pattern takes the transform path
        enc.decode_prepare(dp[0], pp[0])
        assert raw(fe, enc, False, D, Q, count, None, reads, 2, 0, S, out) == fe.E_UNSUPPORTED
        torch.cuda.synchronize()
        assert bool((out == CANARY).all()), "a refused call writes nothing"
        enc.set_option("decode_direct_max", 256)
        enc.decode_prepare(dp[0], pp[0])
        assert raw(fe, enc, False, D, Q, count, None, reads, 2, 0, S, out) == fe.OK
        torch.cuda.synchronize()
        assert bool((out == 0).all())  # (the all-zero codeword)


@pytest.mark.parametrize("n,k,flags", [(20, 16, 0), (64, 32, 0), (72, 48, 1)], ids=["20_16", "64_32", "72_48_mixed"])
def test_read_batch_under_a_pattern_that_lost_nothing(torch_cuda, fe, n, k, flags):
    """A healthy pool with fixed placement: decode_prepare with every block present, then fastecc_read_batch.  "A pattern with no lost data block
    is valid: every request is then a copy" (include/fastecc.h) — also the pattern that lost nothing at all, which has tables on neither path,
    so whatever "decode_direct_max" was when it was prepared.  (Found by the pool sequences of tests/pool_model.py: the call was refused
    FASTECC_E_UNSUPPORTED.)  The words are copied as stored, words >= p included."""
    torch = torch_cuda
    S, count = 20, 5
    with fe.Encoder(n, k, 4 * S, flags=flags) as enc:
        D = garbage(torch, (count, k, S), 7)
        Q = garbage(torch, (count, n - k, S), 8)
        D0, Q0 = D.clone(), Q.clone()
        reads = np.array([0, count * k - 1, k + 3, k + 3, 2], dtype=np.uint64)
        idx = torch.tensor(reads.astype(np.int64), device="cuda:0")
        for direct_max in (256, 0):
            enc.set_option("decode_direct_max", direct_max)
            enc.decode_prepare(np.ones(k, np.uint8), np.ones(n - k, np.uint8))
            for col0, width in ((0, S), (3, 5), (S - 1, 1)):
                out = torch.full((len(reads) + 1, width), CANARY, dtype=torch.int32, device="cuda:0")
                assert raw(fe, enc, False, D, Q, count, None, reads, len(reads), col0, width, out) == fe.OK, (direct_max, col0, width)
                torch.cuda.synchronize()
                assert torch.equal(out[:-1], D0.view(-1, S)[idx, col0:col0 + width]), (direct_max, col0, width)
                assert bool((out[-1] == CANARY).all())
        assert torch.equal(D, D0) and torch.equal(Q, Q0), "the pool is not written"


# ---- 6. one launch, whatever the classes ----
def test_one_launch_and_bytes(torch_cuda, fe):
    torch = torch_cuda
    n, k, S, count = 64, 32, 64, 12
    rng = np.random.default_rng(6)
    sizes = [1, 2, 3, 5, 9, 16]  # pads 1, 2, 4, 8, 16, 16
    patterns = [(sorted(int(x) for x in rng.permutation(k)[:ld]), []) for ld in sizes]
    pattern_of = [b % len(sizes) for b in range(count)]
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        pool = Pool(torch, fe, enc, count, S, patterns, pattern_of, seed=60)
        lost = pool.lost_data_blocks()
        present = [b * k + i for b in range(count) for i in range(k) if i not in patterns[pattern_of[b]][0]][::13]
        reads = np.array(lost + present, dtype=np.uint64)
        np.random.default_rng(7).shuffle(reads)
        enc.profile(True)
        for col0, width in [(0, S), (8, 24)]:
            enc.profile_reset()
            pool.read(reads, col0, width)
            seen = enc.profile_read()
            assert sorted(seen) == ["direct_read_set"], sorted(seen)
            # a lost block: the pass's rows (k + its pattern's lost data blocks) read + 1 written; a present one: 1 + 1
            rows = sum(k + sizes[pattern_of[r // k]] + 1 for r in lost) + 2 * len(present)
            assert seen["direct_read_set"][1] == 1, "one launch"
            assert seen["direct_read_set"][2] == rows * width * 4


# ---- 7. state ----
def test_state_is_left_alone(torch_cuda, fe):
    torch = torch_cuda
    n, k, S, count = 20, 16, 64, 10
    m = n - k
    rotate = lambda shift: [codeword_block(k, (u + shift) % n) for u in range(n)]  # noqa: E731
    pattern_of = [(3 * b + 1) % n for b in range(count)]
    single = ([2, 9], [1])
    reads = shuffled_reads(count, k, seed=8, extra=5)
    with fe.Encoder(n, k, 4 * S) as enc:
        dp, pp = flag_rows(k, m, [single])
        enc.decode_prepare(dp[0], pp[0])
        enc.decode_prepare_set(*flag_rows(k, m, rotate(0)))
        pool = Pool(torch, fe, enc, count, S, rotate(0), pattern_of, seed=70)
        one = Pool(torch, fe, enc, count, S, [single], [0] * count, seed=71)
        pool.read(reads, 0, S)
        one.read(reads, 4, 9, set_form=False)
        pool.read(reads, 1, 33)
        pool.check_repair()                 # repair_batch_set with the same set still repairs a clone
        one.check_repair(set_form=False)    # ... and the single prepared pattern still decodes
        Dd = one.D.clone()
        enc.decode_batch(Dd, one.Q, count)
        torch.cuda.synchronize()
        assert torch.equal(Dd, one.want)
        # a read on a second stream after decode_prepare_set with other patterns uses the new set
        s2 = torch.cuda.Stream()
        pool.read(reads, 0, S, stream=s2.cuda_stream)
        enc.decode_prepare_set(*flag_rows(k, m, rotate(5)))
        moved = Pool(torch, fe, enc, count, S, rotate(5), pattern_of, seed=72)
        moved.read(reads, 0, S, stream=s2.cuda_stream)
        moved.read(reads, 2, 6)
        one.read(reads, 0, S, set_form=False)


# ---- 8. refusals on a live context ----
def test_refusals(torch_cuda, fe):
    torch = torch_cuda
    n, k, S, count = 20, 16, 64, 4
    m = n - k
    patterns = [codeword_block(k, u) for u in (0, 17, 9)]
    g = torch.Generator(device="cuda:0").manual_seed(9)
    rnd = lambda words: torch.randint(0, 1 << 31, (words,), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32)  # noqa: E731
    reads = np.array([0, 17, 63], dtype=np.uint64)

    def refused(enc, rc_want, forms=(True, False), watch=None, **kw):
        """the call (the valid arguments, with `kw` replacing some) returns rc_want; the pool and `out` stay byte for byte as they were"""
        D, Q, buf = watch or (rnd((count + 1) * k * S), rnd((count + 1) * m * S), rnd(8 * S))
        keep = [t.clone() for t in (D, Q, buf)]
        a = dict(data=D, parity=Q, count=count, po=np.array([0, 1, 2, fe.PATTERN_NONE], np.uint32), reads=reads, n_reads=3, col0=0, width=S, out=buf)
        a.update(kw)
        torch.cuda.synchronize()
        for set_form in forms:
            rc = raw(fe, enc, set_form, **a)
            assert rc == rc_want, (set_form, rc, sorted(kw))
        torch.cuda.synchronize()
        assert all(torch.equal(t, t0) for t, t0 in zip((D, Q, buf), keep)), sorted(kw)

    with fe.Encoder(n, k, 4 * S) as enc:
        refused(enc, fe.E_INVAL)  # no set prepared, no pattern prepared
        enc.decode_prepare_set(*flag_rows(k, m, patterns))
        dp, pp = flag_rows(k, m, [patterns[0]])
        enc.decode_prepare(dp[0], pp[0])
        refused(enc, fe.OK, forms=(True,), po=np.array([0, 1, 2, 7], np.uint32), reads=np.array([0, 17, 40], np.uint64), width=S, out=rnd(3 * S))  # (7: a stripe no read names)
        refused(enc, fe.OK, data=None, parity=None, reads=None, out=None, n_reads=0)  # an empty list does nothing
        refused(enc, fe.OK, n_reads=0)
        refused(enc, fe.E_INVAL, data=None)
        refused(enc, fe.E_INVAL, parity=None)
        refused(enc, fe.E_INVAL, reads=None)
        refused(enc, fe.E_INVAL, out=None)
        refused(enc, fe.E_INVAL, forms=(True,), po=None)
        refused(enc, fe.E_INVAL, count=0)
        D, Q, out = rnd((count + 1) * k * S), rnd((count + 1) * m * S), rnd(8 * S)
        refused(enc, fe.E_INVAL, watch=(D, Q, out), data=D.data_ptr() + 2)
        refused(enc, fe.E_INVAL, watch=(D, Q, out), parity=Q.data_ptr() + 1)
        refused(enc, fe.E_INVAL, watch=(D, Q, out), out=out.data_ptr() + 2)
        refused(enc, fe.E_INVAL, width=0)
        refused(enc, fe.E_INVAL, col0=1, width=S)                  # the window ends beyond the block
        refused(enc, fe.E_INVAL, col0=S, width=1)
        refused(enc, fe.E_INVAL, col0=(1 << 64) - 1, width=2)      # ... also where the sum wraps
        refused(enc, fe.E_INVAL, reads=np.array([0, count * k, 1], np.uint64))          # a read index = count * k
        refused(enc, fe.E_INVAL, reads=np.array([0, (1 << 64) - 1, 1], np.uint64))
        refused(enc, fe.E_INVAL, count=(1 << 64) - 1)              # byte sizes beyond 64 bits
        refused(enc, fe.E_INVAL, n_reads=1 << 62)
        refused(enc, fe.E_INVAL, forms=(True,), po=np.array([0, len(patterns), 0, 0], np.uint32))  # an entry = P of a named stripe
        refused(enc, fe.E_INVAL, forms=(True,), po=np.array([0xFFFFFFFE, 0, 0, 0], np.uint32))
        # `out` inside the data range and the parity range, at the start, in the middle and with only its first word inside
        for t, words in ((D, count * k * S), (Q, count * m * S)):
            for at in (0, 4 * S, words - 1):
                refused(enc, fe.E_INVAL, watch=(D, Q, out), out=t.data_ptr() + 4 * at)
        refused(enc, fe.E_INVAL, watch=(D, Q, out), out=D.data_ptr() - 4 * (3 * S - 1))  # ... and with only its last word inside
        enc.set_option("row_pitch_words", S + 32)
        refused(enc, fe.E_UNSUPPORTED, watch=(rnd((count + 1) * k * (S + 32)), rnd((count + 1) * m * (S + 32)), out))
    N = 16
    with fe.Encoder(2 * N, N, 16 * 8, field=fe.FIELD_GF_P61_SQUARED) as enc:
        refused(enc, fe.E_UNSUPPORTED)
    with fe.ShardedEncoder(2 * N, N, 4 * S, [0, 0]) as enc:
        refused(enc, fe.E_UNSUPPORTED)
