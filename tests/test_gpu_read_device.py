"""GPU tests (-m gpu) of the degraded reads from a request list in device memory: fastecc_read_batch_set_device, fastecc_read_batch_device.

The pools are those of tests/test_gpu_read_batch.py (encoded by the library, the lost blocks overwritten with garbage that includes 0xFFFFFFFF
words).  The reference of every case is the host-list call (fastecc_read_batch_set / fastecc_read_batch) on the same pool, set and list, the list
copied to the host for it: the whole output buffer of the device-list call — a canary row before the rows, the rows, a canary row after them,
all pre-filled with the canary word — must equal byte for byte the buffer that holds the host-list call's rows at the rows of the requests and
the canary word everywhere else (FASTECC_READ_NONE rows included).  The pool must equal its pre-call clone and the status word must be 0.  A
list at fault leaves the whole buffer as it was, and the status word names the code and a row that is truly at fault."""
import ctypes

import numpy as np
import pytest

from test_gpu_read_batch import CANARY, Pool, codeword_block, flag_rows, garbage, shuffled_reads, two_blocks

pytestmark = pytest.mark.gpu

NONE = (1 << 64) - 1
MASK = (1 << 64) - 1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def fe(hip_lib):
    import fastecc_amd
    return fastecc_amd


def fault(fe, u):
    return ((fe.E_INVAL & 0xFFFFFFFF) << 32) | u


class Call:
    """One device-list read of a Pool: reference() runs the host-list call on the requests that are not FASTECC_READ_NONE and builds the buffer
    the device-list call has to leave; launch() enqueues the device-list call (the lists go to the device first); check() synchronises and
    compares the buffer, the status word and the pool.  pattern_of: the device call's array when it differs from the pool's (status cases)."""

    def __init__(self, pool, reads, col0=0, width=None, set_form=True, out_offset=0, stream=0, pattern_of=None):
        torch = pool.torch
        self.pool, self.set_form, self.stream, self.col0, self.width = pool, set_form, stream, col0, width
        self.w = pool.S - col0 if width is None else width
        self.reads = np.asarray(reads, dtype=np.uint64)
        self.n = len(self.reads)
        self.first = self.w + out_offset  # a canary row (and out_offset words) before the output, a canary row (and the rest) after it
        self.buf = torch.full(((self.n + 2) * self.w + 2,), CANARY, dtype=torch.int32, device="cuda:0")
        self.expect = self.buf.clone()
        self.po_host = np.array(pool.pattern_of, np.uint32)
        po = self.po_host if pattern_of is None else np.array(pattern_of, np.uint32)
        self.d_po = torch.from_numpy(po.view(np.int32).copy()).to("cuda:0")
        self.d_reads = torch.from_numpy(self.reads.view(np.int64).copy()).to("cuda:0") if self.n else torch.zeros(1, dtype=torch.int64, device="cuda:0")
        self.status = torch.full((1,), 0x5151515151515151, dtype=torch.int64, device="cuda:0")
        self.what = "window (%d, %d), out offset %d, %d requests" % (col0, self.w, out_offset, self.n)
        torch.cuda.synchronize()

    def reference(self):
        torch, pool = self.pool.torch, self.pool
        live = np.nonzero(self.reads != np.uint64(NONE))[0]
        if len(live) == 0:
            return self
        rows = torch.full((len(live), self.w), 0x77777777, dtype=torch.int32, device="cuda:0")
        if self.set_form:
            pool.enc.read_batch_set(pool.D, pool.Q, pool.count, self.po_host, self.reads[live], rows, col0=self.col0, width=self.width)
        else:
            pool.enc.read_batch(pool.D, pool.Q, pool.count, self.reads[live], rows, col0=self.col0, width=self.width)
        torch.cuda.synchronize()
        self.expect[self.first:self.first + self.n * self.w].view(self.n, self.w)[torch.from_numpy(live).to("cuda:0")] = rows
        torch.cuda.synchronize()
        return self

    def launch(self, n_reads=None):
        pool, out = self.pool, self.buf.data_ptr() + 4 * self.first
        n = self.n if n_reads is None else n_reads
        if self.set_form:
            pool.enc.read_batch_set_device(pool.D, pool.Q, pool.count, self.d_po, self.d_reads, n, out, self.status, col0=self.col0, width=self.width,
                                           stream=self.stream)
        else:
            pool.enc.read_batch_device(pool.D, pool.Q, pool.count, self.d_reads, n, out, self.status, col0=self.col0, width=self.width, stream=self.stream)
        return self

    def rows(self):
        return self.buf[self.first:self.first + self.n * self.w].view(self.n, self.w)

    def check(self, status=(0,)):
        torch, pool = self.pool.torch, self.pool
        torch.cuda.synchronize()
        got = self.status.item() & MASK
        print("%s: status %#x" % (self.what, got))
        assert got in status, "%s: status %#x" % (self.what, got)
        assert torch.equal(self.buf, self.expect), "rows, skipped rows and canaries, " + self.what
        assert torch.equal(pool.D, pool.D0) and torch.equal(pool.Q, pool.Q0), "the pool is not written, " + self.what
        return self


def device_read(pool, reads, *a, **kw):
    return Call(pool, reads, *a, **kw).reference().launch().check()


def original(pool, call):
    """the rows of the requests also equal the original data (FASTECC_PATTERN_NONE stripes: what the pool holds)"""
    idx = pool.torch.from_numpy(call.reads.astype(np.int64)).to("cuda:0")
    assert pool.torch.equal(call.rows(), pool.want.view(-1, pool.S)[idx, call.col0:call.col0 + call.w]), call.what


# ---- 1. rotated (20,16), one and two devices down; windows; V = 1 ----
def windows(S):
    return [(0, S), (0, 1), (S - 1, 1), (3, 5), (64, 128), (0, 257), (4, 68)]


@pytest.mark.parametrize("down", [1, 2])
def test_rotated_20_16(torch_cuda, fe, down):
    n, k, S, count = 20, 16, 1024, 40
    patterns = [codeword_block(k, u) if down == 1 else two_blocks(k, n, u) for u in range(n)]
    pattern_of = [fe.PATTERN_NONE if b in (7, 23, 39) else b % n for b in range(count)]
    reads = shuffled_reads(count, k, seed=down)
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        pool = Pool(torch_cuda, fe, enc, count, S, patterns, pattern_of, seed=10 + down)
        for col0, width in windows(S):
            original(pool, device_read(pool, reads, col0, width))
        original(pool, device_read(pool, reads, 0, None))            # width=None: the whole block
        original(pool, device_read(pool, reads, 0, S, out_offset=1))  # `out` 4 bytes past a 16-byte boundary: V = 1
        original(pool, device_read(pool, reads, 64, 128, out_offset=1))
        original(pool, device_read(pool, reads, 4, 68, out_offset=3))


def test_24_byte_blocks(torch_cuda, fe):
    n, k, S, count = 20, 16, 6, 40
    patterns = [codeword_block(k, u) for u in range(n)]
    pattern_of = [fe.PATTERN_NONE if b == 11 else (3 * b + 1) % n for b in range(count)]
    reads = shuffled_reads(count, k, seed=2)
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        pool = Pool(torch_cuda, fe, enc, count, S, patterns, pattern_of, seed=20)
        for col0, width in [(0, 6), (2, 3), (5, 1)]:
            original(pool, device_read(pool, reads, col0, width))
            original(pool, device_read(pool, reads, col0, width, out_offset=1))


# ---- 2. FASTECC_READ_NONE ----
def test_read_none(torch_cuda, fe):
    torch = torch_cuda
    n, k, S, count = 20, 16, 64, 40
    patterns = [codeword_block(k, u) for u in range(n)]
    pattern_of = [fe.PATTERN_NONE if b == 5 else b % n for b in range(count)]
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        dp, pp = flag_rows(k, n - k, [patterns[3]])
        enc.decode_prepare(dp[0], pp[0])
        pool = Pool(torch, fe, enc, count, S, patterns, pattern_of, seed=21)
        one = Pool(torch, fe, enc, count, S, [patterns[3]], [0] * count, seed=22)
        reads = shuffled_reads(count, k, seed=3)
        rng = np.random.default_rng(4)
        holes = reads.copy()
        holes[rng.permutation(len(reads))[:len(reads) // 3]] = np.uint64(NONE)
        holes[0] = holes[-1] = np.uint64(NONE)  # (the first and the last row among them)
        for p, set_form in ((pool, True), (one, False)):
            for col0, width in [(0, S), (3, 5)]:
                c = device_read(p, holes, col0, width, set_form=set_form)
                skipped = torch.from_numpy(np.nonzero(holes == np.uint64(NONE))[0]).to("cuda:0")
                assert len(skipped) > 200 and bool((c.rows()[skipped] == CANARY).all()), "skipped rows keep the fill word for word"
                device_read(p, holes, col0, width, set_form=set_form, out_offset=1)
            device_read(p, np.full(300, NONE, np.uint64), 0, S, set_form=set_form)  # nothing but FASTECC_READ_NONE
            # n_reads = 0: the status word is set to 0 on the stream and nothing else happens (the list given holds requests)
            Call(p, reads[:4], 0, S, set_form=set_form).launch(n_reads=0).check()


# ---- 3. sixteen losses per pattern; every code family ----
def test_sixteen_losses(torch_cuda, fe):
    n, k, S, count = 256, 128, 64, 8
    rng = np.random.default_rng(3)
    pick = lambda total, cnt: sorted(int(x) for x in rng.permutation(total)[:cnt])  # noqa: E731
    patterns = [(pick(k, ld), pick(n - k, 16 - ld)) for ld in (8, 15, 1, 16)]
    pattern_of = [b % 4 for b in range(count)]
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        pool = Pool(torch_cuda, fe, enc, count, S, patterns, pattern_of, seed=30)
        lost = pool.lost_data_blocks()
        present = [b * k + i for b in range(count) for i in range(k) if i not in patterns[pattern_of[b]][0]][::97]
        reads = np.array(lost + present + lost[::5], dtype=np.uint64)
        np.random.default_rng(4).shuffle(reads)
        for col0, width in [(0, 64), (0, 63), (17, 30), (60, 4)]:
            original(pool, device_read(pool, reads, col0, width))
        original(pool, device_read(pool, shuffled_reads(count, k, seed=31), 0, 64))  # every block: the neighbours of every lost one


FAMILIES = [(13, 10, 0), (96, 48, 1)]


@pytest.mark.parametrize("n,k,fl", FAMILIES, ids=["%d_%d" % (c[0], c[1]) for c in FAMILIES])
def test_code_families(torch_cuda, fe, n, k, fl):
    """(13,10): odd sizes, V = 1 (S = 63, windows of odd widths); (96,48): mixed radix"""
    S, count = (63 if n == 13 else 64), 6
    patterns = [([1], []), ([0, k - 1], []), ([2], [1]), ([3, 5, 6], []), ([4], [0, 2]), ([], [1])]
    pattern_of = list(range(count))
    reads = shuffled_reads(count, k, seed=n, extra=9)
    with fe.Encoder(n, k, 4 * S, flags=fl) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        pool = Pool(torch_cuda, fe, enc, count, S, patterns, pattern_of, seed=40 + n)
        for col0, width in [(0, S), (5, 7), (32, S - 32)]:
            original(pool, device_read(pool, reads, col0, width))


# ---- 4. the single prepared pattern ----
# 20 lost data blocks of 32: each of the first, a middle and the last of them has a present block on either side
LOST20 = [2] + list(range(4, 13)) + [14] + list(range(16, 24)) + [29]


def test_single_pattern_binary_search(torch_cuda, fe):
    """a table of pad 32 (a column index >= 16) and a search over 20 entries: the first, the last and a middle lost block and their present
    neighbours, alone and inside every block of the pool in a random order"""
    n, k, S, count = 64, 32, 64, 16
    assert len(LOST20) == 20 and LOST20 == sorted(set(LOST20))
    pattern = (LOST20, [3, 30])
    with fe.Encoder(n, k, 4 * S) as enc:
        dp, pp = flag_rows(k, n - k, [pattern])
        enc.decode_prepare(dp[0], pp[0])
        pool = Pool(torch_cuda, fe, enc, count, S, [pattern], [0] * count, seed=50)
        picks = []
        for b in (0, 7, count - 1):
            for i in (LOST20[0], LOST20[10], LOST20[-1]):
                assert i - 1 not in LOST20 and i + 1 not in LOST20
                picks += [b * k + i - 1, b * k + i, b * k + i + 1]
        picks += [b * k + i for b in (3,) for i in LOST20[15:]]  # output indices 15 .. 19
        picks = np.array(picks, dtype=np.uint64)
        for col0, width in [(0, 64), (3, 5)]:
            original(pool, device_read(pool, picks, col0, width, set_form=False))
        reads = shuffled_reads(count, k, seed=5)
        for col0, width in [(0, 64), (16, 48)]:
            original(pool, device_read(pool, reads, col0, width, set_form=False))
        original(pool, device_read(pool, reads, 0, 64, set_form=False, out_offset=1))


@pytest.mark.parametrize("lost", [(0, 5), (0, 0)], ids=["parity_only", "nothing_lost"])
def test_single_pattern_without_lost_data(torch_cuda, fe, lost):
    n, k, S, count = 64, 32, 64, 16
    rng = np.random.default_rng(5)
    pattern = ([], sorted(int(x) for x in rng.permutation(n - k)[:lost[1]]))
    reads = shuffled_reads(count, k, seed=6)
    with fe.Encoder(n, k, 4 * S) as enc:
        dp, pp = flag_rows(k, n - k, [pattern])
        enc.decode_prepare(dp[0], pp[0])
        pool = Pool(torch_cuda, fe, enc, count, S, [pattern], [0] * count, seed=51)
        for col0, width in [(0, 64), (3, 5)]:
            original(pool, device_read(pool, reads, col0, width, set_form=False))


def raw(fe, enc, set_form, data, parity, count, po, reads, n_reads, col0, width, out, status, stream=None):
    """the C entry point itself: its return code"""
    addr = lambda t: None if t is None else t if isinstance(t, int) else t.data_ptr()  # noqa: E731
    if set_form:
        return fe.lib().fastecc_read_batch_set_device(enc._h, addr(data), addr(parity), count, addr(po), addr(reads), n_reads, col0, width, addr(out),
                                                      addr(status), stream)
    return fe.lib().fastecc_read_batch_device(enc._h, addr(data), addr(parity), count, addr(reads), n_reads, col0, width, addr(out), addr(status), stream)


def test_unprepared_and_transform_path(torch_cuda, fe):
    """the return codes of the host form, with `out` and the status word untouched"""
    torch = torch_cuda
    n, k, S, count = 64, 32, 64, 2
    with fe.Encoder(n, k, 4 * S) as enc:
        D = torch.zeros((count, k, S), dtype=torch.int32, device="cuda:0")
        Q = torch.zeros((count, n - k, S), dtype=torch.int32, device="cuda:0")
        out = torch.full((2, S), CANARY, dtype=torch.int32, device="cuda:0")
        reads = torch.tensor([3, 35], dtype=torch.int64, device="cuda:0")  # the lost block of stripe 0 and of stripe 1
        status = torch.full((1,), 0x51, dtype=torch.int64, device="cuda:0")
        assert raw(fe, enc, False, D, Q, count, None, reads, 2, 0, S, out, status) == fe.E_INVAL  # nothing prepared
        dp, pp = flag_rows(k, n - k, [([3], [])])
        enc.set_option("decode_direct_max", 0)  # every pattern takes the transform path
        enc.decode_prepare(dp[0], pp[0])
        assert raw(fe, enc, False, D, Q, count, None, reads, 2, 0, S, out, status) == fe.E_UNSUPPORTED
        torch.cuda.synchronize()
        assert bool((out == CANARY).all()) and status.item() == 0x51, "a refused call writes nothing"
        enc.set_option("decode_direct_max", 256)
        enc.decode_prepare(dp[0], pp[0])
        assert raw(fe, enc, False, D, Q, count, None, reads, 2, 0, S, out, status) == fe.OK
        torch.cuda.synchronize()
        assert bool((out == 0).all()) and status.item() == 0  # (the all-zero codeword)


# ---- 5. the status word; several workgroups of the translate kernel; a growing scratch list ----
def test_status_and_many_requests(torch_cuda, fe):
    torch = torch_cuda
    n, k, S, count = 20, 16, 64, 300
    patterns = [codeword_block(k, u) for u in range(n)]
    nP = len(patterns)
    pattern_of = [fe.PATTERN_NONE if b % 37 == 5 else b % n for b in range(count)]
    rng = np.random.default_rng(8)
    reads = rng.integers(0, count * k, 1025).astype(np.uint64)  # 1025 requests: five workgroups of the translate kernel, the last with one lane
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        dp, pp = flag_rows(k, n - k, [patterns[2]])
        enc.decode_prepare(dp[0], pp[0])
        pool = Pool(torch, fe, enc, count, S, patterns, pattern_of, seed=60)
        one = Pool(torch, fe, enc, count, S, [patterns[2]], [0] * count, seed=61)
        for p, set_form in ((pool, True), (one, False)):
            original(p, device_read(p, reads[:7], 0, S, set_form=set_form))  # the context's scratch list: 7 requests, then 1025
            original(p, device_read(p, reads, 0, S, set_form=set_form))
            original(p, device_read(p, reads, 3, 5, set_form=set_form))
            # an index = count * k: the status names the row, `out` keeps its fill (the expected buffer holds no row: no reference() here)
            for at in (0, 512, 1024):
                bad = reads.copy()
                bad[at] = count * k
                Call(p, bad, 0, S, set_form=set_form).launch().check(status=(fault(fe, at),))
            bad = reads.copy()
            bad[[0, 512, 1024]] = np.array([count * k, NONE - 1, count * k + 1], dtype=np.uint64)  # several: any one of them is reported
            Call(p, bad, 3, 5, set_form=set_form).launch().check(status=tuple(fault(fe, at) for at in (0, 512, 1024)))
            device_read(p, reads, 0, S, set_form=set_form)  # a valid call straight after a fault: status 0, every row
        # a pattern_of entry = P of a requested stripe; an entry of FASTECC_PATTERN_NONE - 1
        for value in (nP, 0xFFFFFFFE):
            b = int(reads[700]) // k
            po = list(pattern_of)
            po[b] = value
            rows_at_fault = tuple(fault(fe, int(u)) for u in np.nonzero(reads // np.uint64(k) == np.uint64(b))[0])
            assert fault(fe, 700) in rows_at_fault
            Call(pool, reads, 0, S, pattern_of=po).launch().check(status=rows_at_fault)
        # ... of a stripe nobody requests: no fault
        free = sorted(set(range(count)) - set(int(r) // k for r in reads))
        assert free
        po = list(pattern_of)
        po[free[0]] = nP
        po[free[-1]] = 0xFFFFFFFE
        original(pool, Call(pool, reads, 0, S, pattern_of=po).reference().launch().check())


# ---- 6. a list made on the device ----
def test_list_made_on_the_device(torch_cuda, fe):
    """reads and pattern_of come from torch ops on a side stream; two calls back to back on that stream, the list buffer rewritten by a device op
    between them; one synchronise at the end"""
    torch = torch_cuda
    n, k, S, count, nr = 20, 16, 256, 40, 500
    patterns = [codeword_block(k, u) for u in range(n)]
    pattern_of = [b % n for b in range(count)]
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        pool = Pool(torch, fe, enc, count, S, patterns, pattern_of, seed=70)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            outs = [torch.full((nr + 2, S), CANARY, dtype=torch.int32, device="cuda:0") for _ in range(2)]
            status = torch.full((2,), 0x51, dtype=torch.int64, device="cuda:0")
            d_po = (torch.arange(count, device="cuda:0") % n).to(torch.int32)
            d_reads = (torch.arange(nr, device="cuda:0", dtype=torch.int64) * 7 + 3) % (count * k)
            d_reads[::9] = -1  # FASTECC_READ_NONE
            enc.read_batch_set_device(pool.D, pool.Q, count, d_po, d_reads, nr, outs[0][1:], status[0:], stream=side.cuda_stream)
            d_reads.mul_(5).add_(11).remainder_(count * k)  # (the NONE rows become requests: -5 + 11 = 6)
            enc.read_batch_set_device(pool.D, pool.Q, count, d_po, d_reads, nr, outs[1][1:], status[1:], stream=side.cuda_stream)
        side.synchronize()
        torch.cuda.synchronize()
        assert status.tolist() == [0, 0]
        first = (np.arange(nr, dtype=np.int64) * 7 + 3) % (count * k)
        first[::9] = -1
        second = (first * 5 + 11) % (count * k)
        assert np.array_equal(second, d_reads.cpu().numpy())
        for out, lst in zip(outs, (first, second)):
            live = np.nonzero(lst >= 0)[0]
            want = torch.full((nr + 2, S), CANARY, dtype=torch.int32, device="cuda:0")
            rows = torch.empty((len(live), S), dtype=torch.int32, device="cuda:0")
            enc.read_batch_set(pool.D, pool.Q, count, np.array(pattern_of, np.uint32), lst[live].astype(np.uint64), rows)
            torch.cuda.synchronize()
            want[1 + torch.from_numpy(live).to("cuda:0")] = rows
            assert torch.equal(out, want)
            assert torch.equal(rows, pool.want.view(-1, S)[torch.from_numpy(lst[live]).to("cuda:0")])
        assert torch.equal(pool.D, pool.D0) and torch.equal(pool.Q, pool.Q0)


# ---- 7. a replaced set on a second stream ----
def test_replaced_set_on_a_second_stream(torch_cuda, fe):
    torch = torch_cuda
    n, k, S, count = 20, 16, 64, 10
    m = n - k
    rotate = lambda shift: [codeword_block(k, (u + shift) % n) for u in range(n)]  # noqa: E731
    pattern_of = [(3 * b + 1) % n for b in range(count)]
    reads = shuffled_reads(count, k, seed=8, extra=5)
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, m, rotate(0)))
        pool = Pool(torch, fe, enc, count, S, rotate(0), pattern_of, seed=72)
        moved = Pool(torch, fe, enc, count, S, rotate(5), pattern_of, seed=73)
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        before = Call(pool, reads, 0, S, stream=a.cuda_stream).reference()
        after = Call(moved, reads, 0, S, stream=b.cuda_stream)
        before.launch()
        enc.decode_prepare_set(*flag_rows(k, m, rotate(5)))  # (waits for the read in flight before it replaces the tables)
        after.launch()
        before.check()
        original(pool, before)
        original(moved, after.reference().check())  # (the reference under the new set; the device call's rows are already there)
        original(moved, device_read(moved, reads, 2, 6))


# ---- 8. host refusals on a live context ----
def test_refusals(torch_cuda, fe):
    torch = torch_cuda
    n, k, S, count = 20, 16, 64, 4
    m = n - k
    patterns = [codeword_block(k, u) for u in (0, 17, 9)]
    g = torch.Generator(device="cuda:0").manual_seed(9)
    rnd = lambda words: torch.randint(0, 1 << 31, (words,), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32)  # noqa: E731
    reads = torch.tensor([0, 17, 63, 5], dtype=torch.int64, device="cuda:0")
    po = torch.tensor([0, 1, 2, -1], dtype=torch.int32, device="cuda:0")
    status = torch.full((2,), 0x51, dtype=torch.int64, device="cuda:0")

    def refused(enc, rc_want, forms=(True, False), watch=None, status_after=0x51, **kw):
        """the call (the valid arguments, with `kw` replacing some) returns rc_want; the pool, `out`, the lists and the status stay as they were"""
        D, Q, buf = watch or (rnd((count + 1) * k * S), rnd((count + 1) * m * S), rnd(8 * S))
        watched = (D, Q, buf, reads, po)
        keep = [t.clone() for t in watched]
        a = dict(data=D, parity=Q, count=count, po=po, reads=reads, n_reads=3, col0=0, width=S, out=buf, status=status)
        a.update(kw)
        for set_form in forms:
            status.fill_(0x51)
            torch.cuda.synchronize()
            rc = raw(fe, enc, set_form, **a)
            torch.cuda.synchronize()
            assert rc == rc_want, (set_form, rc, sorted(kw))
            assert status.tolist() == [status_after, 0x51], (set_form, sorted(kw))
        assert all(torch.equal(t, t0) for t, t0 in zip(watched, keep)), sorted(kw)

    with fe.Encoder(n, k, 4 * S) as enc:
        refused(enc, fe.E_INVAL)  # no set prepared, no pattern prepared
        enc.decode_prepare_set(*flag_rows(k, m, patterns))
        dp, pp = flag_rows(k, m, [patterns[0]])
        enc.decode_prepare(dp[0], pp[0])
        refused(enc, fe.OK, n_reads=0, status_after=0)  # an empty list: *status = 0 on the stream and nothing else
        refused(enc, fe.OK, data=None, parity=None, out=None, n_reads=0, status_after=0)
        refused(enc, fe.E_INVAL, status=None)
        refused(enc, fe.E_INVAL, status=None, n_reads=0)
        refused(enc, fe.E_INVAL, status=status.data_ptr() + 4)
        refused(enc, fe.E_INVAL, reads=reads.data_ptr() + 4)
        refused(enc, fe.E_INVAL, forms=(True,), po=po.data_ptr() + 2)
        refused(enc, fe.E_INVAL, forms=(True,), po=None)
        refused(enc, fe.E_INVAL, data=None)
        refused(enc, fe.E_INVAL, parity=None)
        refused(enc, fe.E_INVAL, reads=None)
        refused(enc, fe.E_INVAL, out=None)
        refused(enc, fe.E_INVAL, count=0)
        D, Q, out = rnd((count + 1) * k * S), rnd((count + 1) * m * S), rnd(8 * S)
        refused(enc, fe.E_INVAL, watch=(D, Q, out), data=D.data_ptr() + 2)
        refused(enc, fe.E_INVAL, watch=(D, Q, out), parity=Q.data_ptr() + 1)
        refused(enc, fe.E_INVAL, watch=(D, Q, out), out=out.data_ptr() + 2)
        refused(enc, fe.E_INVAL, width=0)
        refused(enc, fe.E_INVAL, col0=1, width=S)                  # the window ends beyond the block
        refused(enc, fe.E_INVAL, col0=S, width=1)
        refused(enc, fe.E_INVAL, col0=(1 << 64) - 1, width=2)      # ... also where the sum wraps
        refused(enc, fe.E_INVAL, count=(1 << 64) - 1)              # byte sizes beyond 64 bits
        refused(enc, fe.E_UNSUPPORTED, n_reads=(1 << 24) + 1)      # a list above 2^24 entries
        refused(enc, fe.E_UNSUPPORTED, n_reads=1 << 62)
        # `out` inside the data range and the parity range, at the start, in the middle and with only its first word inside
        for t, words in ((D, count * k * S), (Q, count * m * S)):
            for at in (0, 4 * S, words - 1):
                refused(enc, fe.E_INVAL, watch=(D, Q, out), out=t.data_ptr() + 4 * at)
        refused(enc, fe.E_INVAL, watch=(D, Q, out), out=D.data_ptr() - 4 * (3 * S - 1))  # ... and with only its last word inside
        # the lists and the status word inside `out`: at its start, and with only the last word of `out` on them
        # (`out` is the first 3 S words of `big`)
        big = rnd(8 * S)
        for name in ("reads", "status"):
            refused(enc, fe.E_INVAL, watch=(D, Q, big), **{name: big.data_ptr()})
            refused(enc, fe.E_INVAL, watch=(D, Q, big), **{name: big.data_ptr() + 4 * (3 * S - 2)})
        refused(enc, fe.E_INVAL, watch=(D, Q, big), reads=big.data_ptr() + 16 * S, out=big.data_ptr() + 16 * S + 8)  # `out` begins inside the list
        refused(enc, fe.E_INVAL, watch=(D, Q, big), forms=(True,), po=big.data_ptr() + 4 * S)
        refused(enc, fe.E_INVAL, watch=(D, Q, big), forms=(True,), po=big.data_ptr() + 4 * (3 * S - 1))
        refused(enc, fe.E_INVAL, status=reads.data_ptr() + 8)      # the status word inside the list
        refused(enc, fe.E_INVAL, forms=(True,), status=po.data_ptr() + 8)
        enc.set_option("row_pitch_words", S + 32)
        refused(enc, fe.E_UNSUPPORTED, watch=(rnd((count + 1) * k * (S + 32)), rnd((count + 1) * m * (S + 32)), out))
    N = 16
    with fe.Encoder(2 * N, N, 16 * 8, field=fe.FIELD_GF_P61_SQUARED) as enc:
        refused(enc, fe.E_UNSUPPORTED)
    with fe.ShardedEncoder(2 * N, N, 4 * S, [0, 0]) as enc:
        refused(enc, fe.E_UNSUPPORTED)
