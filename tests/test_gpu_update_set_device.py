"""GPU tests (-m gpu) of the degraded pool writes from a write list in device memory: fastecc_update_batch_set_device and
fastecc_update_parity_batch_set_device.

The yardstick in every case is the HOST-list call of the same build: a clone of the pool after fastecc_update_batch_set_window /
fastecc_update_parity_batch_set_window with the list copied to the host, its FASTECC_WRITE_NONE entries removed and the rows renumbered.  The
comparison is word for word over the whole tensors: absent blocks and untouched stripes (seeded garbage with words >= p), and a guard stripe of
sentinels behind each pool.  A refused list (a non-zero status word) must leave the pool word for word as it was."""
import numpy as np
import pytest

from pool_model import MIXED_RADIX
from test_gpu_update_batch_set import aimed_writes, codeword_block, flag_rows, garbage, rand_words, random_writes, rotated, two_blocks

pytestmark = pytest.mark.gpu

P = 0xFFF00001
NONE = -1                # FASTECC_WRITE_NONE in an int64 tensor
PATTERN_NONE = 0xFFFFFFFF
STATUS_GARBAGE = 0x5151515151515151
INVAL, NOMEM, UNSUPPORTED = -1, -2, -4


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def fe(hip_lib):
    import fastecc_amd
    return fastecc_amd


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1).view(np.int32)).to("cuda:0")


def host(t):
    return t.cpu().numpy().view(np.uint32).copy()


def decode_status(v):
    """(code, row) of a status word"""
    v = int(v) & ((1 << 64) - 1)
    hi = v >> 32
    return (hi - (1 << 32) if hi >= 1 << 31 else hi), v & 0xFFFFFFFF


def above_p(rng, shape):
    return (P + rng.integers(0, (1 << 32) - P, size=shape, dtype=np.uint64)).astype(np.uint32)


class SetPool:
    """The truth X of `count` stripes (device), and the damaged image handed to the library: every block that its stripe's pattern loses, and every
    block of a stripe outside `live`, holds garbage; a guard stripe of sentinels stands behind each of the two tensors.  outside: a window
    (col0, width) — every word of the image outside it is >= p, in every block."""

    def __init__(self, torch, enc, n, k, S, count, patterns, pattern_of, live, seed, outside=None):
        self.torch, self.enc, self.n, self.k, self.m, self.S, self.count = torch, enc, n, k, n - k, S, count
        self.patterns, self.pattern_of = patterns, np.array(pattern_of, dtype=np.uint32)
        self.rng = rng = np.random.default_rng(seed)
        m = self.m
        self.live = np.zeros(count, bool)
        self.live[list(live)] = True
        self.absent_d, self.absent_p = np.zeros((count, k), bool), np.zeros((count, m), bool)
        for b in np.flatnonzero(self.live):
            q = int(self.pattern_of[b])
            if q != PATTERN_NONE:
                self.absent_d[b, list(patterns[q][0])] = True
                self.absent_p[b, list(patterns[q][1])] = True
        self.X = rand_words(rng, (count, k, S))
        xd = to_dev(torch, self.X)
        par = torch.zeros(count * m * S, dtype=torch.int32, device="cuda:0")
        enc.encode_pool(xd, par, count)
        torch.cuda.synchronize()
        img_d, img_p = self.X.copy(), host(par).reshape(count, m, S)
        dead_d, dead_p = self.absent_d | ~self.live[:, None], self.absent_p | ~self.live[:, None]
        img_d[dead_d] = garbage(rng, (int(dead_d.sum()), S))
        img_p[dead_p] = garbage(rng, (int(dead_p.sum()), S))
        if outside:
            cols = np.ones(S, bool)
            cols[outside[0]:outside[0] + outside[1]] = False
            img_d[:, :, cols] = above_p(rng, (count, k, int(cols.sum())))
            img_p[:, :, cols] = above_p(rng, (count, m, int(cols.sum())))
        self.dd = to_dev(torch, np.concatenate([img_d.reshape(-1), np.full(k * S, 0xFEEDFACE, np.uint32)]))
        self.dp = to_dev(torch, np.concatenate([img_p.reshape(-1), np.full(m * S, 0xDEADBEEF, np.uint32)]))
        self.po = to_dev(torch, self.pattern_of)
        self.touched = np.zeros(count, bool)

    def n_absent(self, writes):
        return sum(1 for w in writes if w != NONE and self.absent_d[w // self.k, w % self.k])

    def rows(self, n_rows, width):
        return to_dev(self.torch, rand_words(self.rng, (max(n_rows, 1), width)))

    def old_rows(self, writes, col0, width):
        """the TRUE old words of the written windows, one row per entry (FASTECC_WRITE_NONE or an index past the pool: block 0's)"""
        X = self.X.reshape(self.count * self.k, self.S)
        return to_dev(self.torch, np.stack([X[w if 0 <= w < len(X) else 0, col0:col0 + width] for w in writes]))

    def reference(self, writes, new, window, form, old, po=None):
        """(data, parity) clones after the host-list call with the list's real writes and their rows"""
        torch, enc = self.torch, self.enc
        col0, width = window
        real = [u for u, w in enumerate(writes) if w != NONE]
        sel = torch.tensor(real, dtype=torch.int64, device="cuda:0")
        pick = lambda rows: None if rows is None else rows.view(-1, width)[sel].contiguous().view(-1)
        cd, cp = self.dd.clone(), self.dp.clone()
        po = self.pattern_of if po is None else po
        if real and form == "batch":
            enc.update_batch_set(cd, cp, self.count, po, [writes[u] for u in real], pick(new), col0=col0, width=width)
        elif real:
            enc.update_parity_batch_set(cp, self.count, po, [writes[u] for u in real], pick(new), old=pick(old), col0=col0, width=width)
        torch.cuda.synchronize()
        return cd, cp

    def device_call(self, writes, new, window, form, old, mps, max_absent=None, stream=0, po=None):
        """the device-list call on the pool itself; returns the status word read back after a synchronise"""
        torch, enc = self.torch, self.enc
        col0, width = window
        dw = torch.tensor(writes, dtype=torch.int64, device="cuda:0") if writes else torch.zeros(1, dtype=torch.int64, device="cuda:0")
        status = torch.full((1,), STATUS_GARBAGE, dtype=torch.int64, device="cuda:0")
        po = self.po if po is None else po
        keep_po = po.clone()
        torch.cuda.synchronize()
        if form == "batch":
            enc.update_batch_set_device(self.dd, self.dp, self.count, po, dw, len(writes), new, status, max_per_stripe=mps, max_absent=max_absent,
                                        stream=stream, col0=col0, width=width)
        else:
            enc.update_parity_batch_set_device(self.dp, self.count, po, dw, len(writes), new, status, old=old, max_per_stripe=mps, stream=stream,
                                               col0=col0, width=width)
        torch.cuda.synchronize()
        assert dw.tolist()[:len(writes)] == list(writes) and torch.equal(po, keep_po), "the lists are only read"
        return int(status.item())

    def apply(self, writes, mps, window=None, form="batch", with_old=True, new=None, max_absent=None, what=""):
        """one device-list call checked against the host-list call on a clone"""
        torch = self.torch
        window = window or (0, self.S)
        new = self.rows(len(writes), window[1]) if new is None else new
        old = self.old_rows(writes, *window) if form == "parity" and with_old and writes else None
        keep = new.clone()
        want_d, want_p = self.reference(writes, new, window, form, old)
        status = self.device_call(writes, new, window, form, old, mps, max_absent)
        assert status == 0, "%s: status %r" % (what, decode_status(status))
        assert torch.equal(self.dd, want_d), what + ": the data pool (guard stripe included) differs from the host-list call's"
        assert torch.equal(self.dp, want_p), what + ": the parity pool (guard stripe included) differs from the host-list call's"
        assert torch.equal(new, keep), what + ": the rows are only read"
        real = [(u, w) for u, w in enumerate(writes) if w != NONE]
        self.touched[[w // self.k for _, w in real]] = True
        if form == "batch":
            rows = host(new).reshape(-1, window[1])
            for u, w in real:
                self.X.reshape(-1, self.S)[w, window[0]:window[0] + window[1]] = rows[u]
        return new

    def refused(self, writes, mps, code, rows, window=None, form="batch", max_absent=None, po=None, what=""):
        """a list the device refuses: the status word's code, its row among `rows`, and the pool word for word as before"""
        torch = self.torch
        window = window or (0, self.S)
        new = self.rows(len(writes), window[1])
        old = self.old_rows(writes, *window) if form == "parity" else None
        before_d, before_p = self.dd.clone(), self.dp.clone()
        got = decode_status(self.device_call(writes, new, window, form, old, mps, max_absent, po=po))
        assert got[0] == code and got[1] in rows, "%s: status %r, expected code %d and a row of %r" % (what, got, code, sorted(rows))
        assert torch.equal(self.dd, before_d) and torch.equal(self.dp, before_p), what + ": a refused list wrote to the pool"

    def check_repair_and_reads(self, what=""):
        """after whole-block data calls: repair_batch_set of a clone gives encode_pool of the true X', and read_batch_set of every absent block of
        the touched stripes — the written ones among them — returns its row of X'"""
        torch, enc, count, k, m, S = self.torch, self.enc, self.count, self.k, self.m, self.S
        t = self.touched
        reads = [int(b) * k + int(i) for b, i in np.argwhere(self.absent_d & t[:, None])]
        if reads:
            out = torch.full((len(reads) * S,), 0x3C3C3C3C, dtype=torch.int32, device="cuda:0")
            enc.read_batch_set(self.dd, self.dp, count, self.pattern_of, reads, out)
            torch.cuda.synchronize()
            assert np.array_equal(host(out).reshape(len(reads), S), self.X.reshape(-1, S)[reads]), what + ": read_batch_set of the absent blocks"
        cd, cp = self.dd.clone(), self.dp.clone()
        enc.repair_batch_set(cd, cp, count, np.where(t, self.pattern_of, PATTERN_NONE).astype(np.uint32))
        true_p = torch.zeros(count * m * S, dtype=torch.int32, device="cuda:0")
        enc.encode_pool(to_dev(torch, self.X), true_p, count)
        torch.cuda.synchronize()
        got_d, got_p = host(cd)[:count * k * S].reshape(count, k, S), host(cp)[:count * m * S].reshape(count, m, S)
        assert np.array_equal(got_d[t], self.X[t]), what + ": the repaired data is not X'"
        assert np.array_equal(got_p[t], host(true_p).reshape(count, m, S)[t]), what + ": the repaired parity is not encode_pool of X'"


def prepared(fe, n, k, S, patterns, flags=0):
    enc = fe.Encoder(n, k, 4 * S, flags=flags)
    enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
    return enc


# ---- 1. rotated placement, one and two devices down ----
@pytest.mark.parametrize("which", ["aimed", "random"])
@pytest.mark.parametrize("down", [1, 2], ids=["one_down", "two_down"])
@pytest.mark.parametrize("S", [1, 63, 65, 130, 260])
def test_rotated_placement(torch_cuda, fe, S, down, which):
    n, k, count = 20, 16, 40
    patterns = [codeword_block(k, u) if down == 1 else two_blocks(k, n, u) for u in range(n)]
    pattern_of = rotated(n, count)
    rng = np.random.default_rng(100 * down + S)
    with prepared(fe, n, k, S, patterns) as enc:
        pool = SetPool(torch_cuda, enc, n, k, S, count, patterns, pattern_of, range(count), seed=S + down)
        if which == "aimed":
            writes = aimed_writes(rng, k, count, patterns, pattern_of)
            assert pool.n_absent(writes) >= count * (k // 2) // n
        else:
            writes = [b * k + int(rng.integers(k)) for b in range(count)]
        writes = [writes[u] for u in rng.permutation(count)]
        what = "S = %d, %d down, %s" % (S, down, which)
        pool.apply(writes, 1, what=what)
        pool.check_repair_and_reads(what)


# ---- 2. every class in one call; the list's order does not matter ----
@pytest.mark.parametrize("mps", [16, 9])
def test_classes_in_any_order(torch_cuda, fe, mps):
    """stripes with 1, 2, 3, 5, 9 and 16 writes under the promise 16; without the stripe of 16 under the promise 9, the exact maximum"""
    n, k, S, count = 48, 32, 8, 7
    per_stripe = [1, 2, 3, 5, 9, 16 if mps == 16 else 7, 4]
    patterns = [([3, 17, 20], [5]), ([0], []), ([], [15, 0]), ([1, 2, 4, 8], [])]
    pattern_of = [1, 0, 2, 3, 0, 3, PATTERN_NONE]
    rng = np.random.default_rng(2)
    writes = []
    for b, t in enumerate(per_stripe):  # the stripe's absent data blocks first: several absent written blocks, mixed with present ones
        ld = list(patterns[pattern_of[b]][0]) if pattern_of[b] != PATTERN_NONE else []
        others = [int(i) for i in rng.permutation(k) if i not in ld]
        writes += [b * k + i for i in (ld + others)[:t]]
    rows = rand_words(rng, (len(writes), S))
    orders = {"as built": list(range(len(writes))), "reversed": list(range(len(writes)))[::-1], "permuted": [int(u) for u in rng.permutation(len(writes))]}
    results = {}
    with prepared(fe, n, k, S, patterns) as enc:
        for name, order in orders.items():
            pool = SetPool(torch_cuda, enc, n, k, S, count, patterns, pattern_of, range(count), seed=22)
            ws = [writes[u] for u in order]
            absent = pool.n_absent(ws)
            assert absent >= 8 and any(pool.absent_d[w // k].sum() > 1 for w in ws)
            pool.apply(ws, mps, new=to_dev(torch_cuda, rows[order]), max_absent=absent, what="the list " + name)
            pool.check_repair_and_reads("the list " + name)
            results[name] = (pool.dd.clone(), pool.dp.clone())
    for name in ("reversed", "permuted"):
        assert torch_cuda.equal(results[name][0], results["as built"][0]) and torch_cuda.equal(results[name][1], results["as built"][1]), name


# ---- 3. windows ----
@pytest.mark.parametrize("form,with_old", [("batch", True), ("parity", True), ("parity", False)], ids=["batch", "parity_old_rows", "parity_from_zero"])
@pytest.mark.parametrize("window", ["whole", (4, 8), (2, 6), (1, 5), "last"], ids=str)
def test_windows(torch_cuda, fe, window, form, with_old):
    n, k, S, count = 20, 16, 68, 6
    window = (0, S) if window == "whole" else (S - 1, 1) if window == "last" else window
    patterns = [([2, 9], [1]), ([], [0, 3]), ([5], [])]
    pattern_of = [0, 1, 2, PATTERN_NONE, 0, 7]  # (stripe 5 is not touched)
    rng = np.random.default_rng(window[0] + window[1])
    writes = [2, 9, 4, k + 1, 2 * k + 5, 2 * k + 6, 3 * k, 4 * k + 9, 4 * k + 10, 4 * k + 11]
    writes = [writes[u] for u in rng.permutation(len(writes))] + [NONE]
    with prepared(fe, n, k, S, patterns) as enc:
        pool = SetPool(torch_cuda, enc, n, k, S, count, patterns, pattern_of, range(5), seed=33, outside=window)
        before_d, before_p = host(pool.dd), host(pool.dp)
        pool.apply(writes, 4, window=window, form=form, with_old=with_old, what="window %r" % (window,))
        cols = np.ones(S, bool)
        cols[window[0]:window[0] + window[1]] = False
        for got, was, blocks in ((host(pool.dd), before_d, count * k), (host(pool.dp), before_p, count * (n - k))):
            assert np.array_equal(got.reshape(-1, S)[:, cols], was.reshape(-1, S)[:, cols]), "words outside the window changed"
            assert (was.reshape(-1, S)[:blocks, cols] >= P).all(), "the test's own pool: every word outside the window is >= p"


# ---- 4. the cursor through the lost parity blocks ----
def test_sixteen_losses_and_the_edges_of_a_run(torch_cuda, fe):
    n, k, S, count = 256, 128, 8, 3
    rng = np.random.default_rng(4)
    ld = sorted(int(i) for i in rng.permutation(k)[:8])
    lp = sorted(int(i) for i in rng.permutation(n - k)[:8])
    patterns = [(ld, lp), ([], [0, 1, 127]), ([5], []), ([], [0, 63, 64, 126, 127])]
    present = [i for i in range(k) if i not in ld]
    with prepared(fe, n, k, S, patterns) as enc:
        pool = SetPool(torch_cuda, enc, n, k, S, count, patterns, [2, 0, 1], range(3), seed=44)
        pool.apply([k + i for i in ld[:3] + present[:5]] + [5, 6], 8, what="8 data + 8 parity blocks lost")
        pool.apply([2 * k + 40, 2 * k + 41, NONE, 7], 2, what="the stripe that lost parity blocks 0, 1 and 127")
        pool.check_repair_and_reads()
        pool = SetPool(torch_cuda, enc, n, k, S, count, patterns, [3, 3, 1], range(3), seed=45)
        pool.apply([1, k + 2, k + 3, 2 * k + 4], 2, form="parity", what="lost parity at the start, the middle and the end")


def test_several_parity_blocks_per_wave(torch_cuda, fe):
    """8192 touched stripes of (20,16): a wave walks the whole parity of its stripe (tests/test_gpu_update_batch_set.py), 3000: half of it"""
    n, k, S, count = 20, 16, 4, 8192
    patterns = [two_blocks(k, n, u) for u in range(n)] + [([], [0, 3]), ([], [1, 2]), ([2], [0, 1, 2])]
    pattern_of = [b % len(patterns) for b in range(count)]
    rng = np.random.default_rng(5)
    with prepared(fe, n, k, S, patterns) as enc:
        pool = SetPool(torch_cuda, enc, n, k, S, count, patterns, pattern_of, range(count), seed=55)
        pool.apply(aimed_writes(rng, k, count, patterns, pattern_of), 1, what="8192 stripes")
        some = [int(b) for b in rng.permutation(count)[:3000]]
        pool.apply([b * k + int(rng.integers(k)) for b in some], 1, what="3000 stripes")
        pool.check_repair_and_reads()


# ---- 5. whole stripes; other code families ----
def test_whole_stripes_equal_update_batch_device(torch_cuda, fe):
    torch = torch_cuda
    n, k, S, count = 20, 16, 65, 9
    patterns = [([], []), ([1], [2])]  # pattern 0 loses nothing
    pattern_of = [PATTERN_NONE, 0, PATTERN_NONE, 0, 5, 99, 0, PATTERN_NONE, 1 << 20]  # stripes 4, 5 and 8: not touched, so not looked at
    live = [0, 1, 2, 3, 6, 7]
    rng = np.random.default_rng(6)
    writes = random_writes(rng, k, live, 30)
    with prepared(fe, n, k, S, patterns) as enc:
        pool = SetPool(torch, enc, n, k, S, count, patterns, pattern_of, live, seed=66)
        cd, cp = pool.dd.clone(), pool.dp.clone()
        new = pool.apply(writes, 16, max_absent=0, what="patterns that lose nothing")
        status = torch.full((1,), STATUS_GARBAGE, dtype=torch.int64, device="cuda:0")
        enc.update_batch_device(cd, cp, count, torch.tensor(writes, dtype=torch.int64, device="cuda:0"), len(writes), new, status, max_per_stripe=16)
        torch.cuda.synchronize()
        assert status.item() == 0 and torch.equal(cd, pool.dd) and torch.equal(cp, pool.dp)


@pytest.mark.parametrize("n,k,S,flags", [(32, 8, 32, 0), (72, 48, 64, MIXED_RADIX)], ids=["32_8", "72_48_mixed"])
def test_code_families(torch_cuda, fe, n, k, S, flags):
    count = n + 3
    patterns = [codeword_block(k, u) for u in range(n)]
    pattern_of = rotated(n, count, down=1)
    rng = np.random.default_rng(n)
    with prepared(fe, n, k, S, patterns, flags) as enc:
        pool = SetPool(torch_cuda, enc, n, k, S, count, patterns, pattern_of, range(count), seed=n)
        pool.apply(aimed_writes(rng, k, count, patterns, pattern_of), 1)
        pool.check_repair_and_reads()


# ---- 6. max_absent ----
def test_max_absent(torch_cuda, fe):
    n, k, S, count = 20, 16, 16, 40
    patterns = [codeword_block(k, u) for u in range(n)]
    pattern_of = rotated(n, count)
    rng = np.random.default_rng(6)
    with prepared(fe, n, k, S, patterns) as enc:
        pool = SetPool(torch_cuda, enc, n, k, S, count, patterns, pattern_of, range(count), seed=61)
        writes = aimed_writes(rng, k, count, patterns, pattern_of)
        absent = pool.n_absent(writes)
        absent_rows = {u for u, w in enumerate(writes) if pool.absent_d[w // k, w % k]}
        assert absent == len(absent_rows) >= 2
        pool.refused(writes, 1, NOMEM, absent_rows, max_absent=absent - 1, what="one slot fewer than absent writes")
        pool.refused(writes, 1, NOMEM, absent_rows, max_absent=0, what="max_absent = 0 with absent writes")
        one = [w for u, w in enumerate(writes) if u not in absent_rows] + [writes[min(absent_rows)]]
        pool.refused(one, 1, NOMEM, {len(one) - 1}, max_absent=0, what="max_absent = 0 with one absent write")
        pool.apply(writes, 1, max_absent=absent, what="exactly the number of absent writes")
        pool.apply(one[:-1], 1, max_absent=0, what="max_absent = 0 with no absent write")
        pool.apply(writes, 1, max_absent=None, what="max_absent = None")
        pool.apply(writes, 1, max_absent=1 << 40, what="a bound far above n_writes")
        pool.check_repair_and_reads()


# ---- 7. lists the device refuses ----
def test_status_faults_leave_the_pool_unchanged(torch_cuda, fe):
    n, k, S, count = 6, 4, 4, 1025
    patterns = [codeword_block(k, u) for u in range(n)]
    pattern_of = rotated(n, count)
    rng = np.random.default_rng(7)
    with prepared(fe, n, k, S, patterns) as enc:
        pool = SetPool(torch_cuda, enc, n, k, S, count, patterns, pattern_of, range(count), seed=71)
        good = aimed_writes(rng, k, count, patterns, pattern_of)
        present = next(u for u, w in enumerate(good) if not pool.absent_d[w // k, w % k])
        absent = next(u for u, w in enumerate(good) if pool.absent_d[w // k, w % k])
        bad_po = {}
        for value in (len(patterns), 0xFFFFFFFE):
            po = pool.pattern_of.copy()
            po[300] = value
            bad_po[value] = to_dev(torch_cuda, po)
        for form in ("batch", "parity"):
            for row in (0, 512, 1024):
                pool.refused(good[:row] + [count * k] + good[row + 1:], 1, INVAL, {row}, form=form, what="an index == count * k at row %d" % row)
            pool.refused(good + [good[present]], 2, INVAL, {present, count}, form=form, what="a duplicate on a present block")
            pool.refused(good + [good[absent]], 2, INVAL, {absent, count}, form=form, what="a duplicate on an absent block")
            other = good[7] - good[7] % k + (good[7] + 1) % k
            pool.refused(good + [other], 1, UNSUPPORTED, {7, count}, form=form, what="2 writes to one stripe under max_per_stripe = 1")
            for value, po in bad_po.items():
                row = next(u for u, w in enumerate(good) if w // k == 300)
                pool.refused(good, 1, INVAL, {row}, form=form, po=po, what="pattern_of[b] = %#x of a touched stripe" % value)
            pool.refused([count * k] + good[1:512] + [good[5]] + good[513:], 2, INVAL, {0, 5, 300, 512}, form=form, po=bad_po[len(patterns)],
                         what="several faults at once")
            # the same entries on stripes that nobody writes: no fault; and a valid call straight after the refused ones
            for po in bad_po.values():
                quiet = [w for w in good if w // k != 300]
                rows, old = pool.rows(len(quiet), S), pool.old_rows(quiet, 0, S)
                want = pool.reference(quiet, rows, (0, S), form, old)
                assert pool.device_call(quiet, rows, (0, S), form, old, 1, po=po) == 0
                assert torch_cuda.equal(pool.dd, want[0]) and torch_cuda.equal(pool.dp, want[1])
            pool.apply(good, 1, form=form, what="a valid call after the refused ones (%s)" % form)


# ---- 8. empty lists ----
def test_write_none_entries_and_empty_lists(torch_cuda, fe):
    n, k, S, count = 20, 16, 64, 7
    patterns = [([3], [1]), ([], [0])]
    pattern_of = [0, 1, 0, PATTERN_NONE, 0, 1, 0]
    with prepared(fe, n, k, S, patterns) as enc:
        pool = SetPool(torch_cuda, enc, n, k, S, count, patterns, pattern_of, range(count), seed=88)
        real = aimed_writes(pool.rng, k, count, patterns, pattern_of)
        writes = [w for pair in zip(real, [NONE] * len(real)) for w in pair]  # every second entry
        pool.apply(writes, 1, what="every second entry NONE")
        before = pool.dd.clone(), pool.dp.clone()
        pool.apply([NONE] * 9, 1, what="a list of NONE only")
        pool.apply([NONE] * 300, 16, form="parity", what="a long list of NONE only")
        pool.apply([], 1, what="n_writes = 0")
        pool.apply([], 16, form="parity", what="n_writes = 0, the parity form")
        assert torch_cuda.equal(pool.dd, before[0]) and torch_cuda.equal(pool.dp, before[1])
        pool.check_repair_and_reads()
        pool.apply(writes[::-1], 1, form="parity", what="every second entry NONE, the parity form")


# ---- 9. more than one workgroup of the build kernels; growth ----
@pytest.mark.parametrize("count", [300, 1025])
def test_many_stripes_cross_the_workgroups_of_the_build_kernels(torch_cuda, fe, count):
    n, k, S = 6, 4, 4
    patterns = [two_blocks(k, n, u) for u in range(n)]
    pattern_of = rotated(n, count)
    with prepared(fe, n, k, S, patterns) as enc:
        pool = SetPool(torch_cuda, enc, n, k, S, count, patterns, pattern_of, range(count), seed=count)
        pool.apply(aimed_writes(pool.rng, k, count, patterns, pattern_of), 1, what="%d stripes, one write each" % count)
        two = [int(b) * k + int(i) for b in range(count) for i in pool.rng.permutation(k)[:2]]
        pool.apply([two[u] for u in pool.rng.permutation(len(two))], 2, what="%d stripes, two writes each" % count)
        pool.check_repair_and_reads()
        pool.apply(aimed_writes(pool.rng, k, count, patterns, pattern_of), 1, form="parity", what="%d stripes, the parity form" % count)


def test_a_context_that_grows(torch_cuda, fe):
    n, k, S = 6, 4, 4
    patterns = [codeword_block(k, u) for u in range(n)]
    with prepared(fe, n, k, S, patterns) as enc:
        small = SetPool(torch_cuda, enc, n, k, S, 7, patterns, rotated(n, 7), range(7), seed=7)
        writes = aimed_writes(small.rng, k, 7, patterns, small.pattern_of)
        keep = [w for w in writes if not small.absent_d[w // k, w % k]] + [next(w for w in writes if small.absent_d[w // k, w % k])]
        small.apply(keep, 1, max_absent=1, what="7 stripes, max_absent = 1")
        large = SetPool(torch_cuda, enc, n, k, S, 1025, patterns, [0] * 1025, range(1025), seed=1025)
        every = [b * k for b in range(1025)]  # pattern 0 loses data block 0: every write is to an absent block
        assert large.n_absent(every) == 1025
        large.apply(every, 1, max_absent=1025, what="1025 stripes and 1025 absent writes on the context that served 7 and 1")
        large.check_repair_and_reads()
        small.apply(keep, 1, max_absent=1, what="7 stripes again")


# ---- 10. streams ----
def test_lists_made_on_the_device_and_back_to_back_calls(torch_cuda, fe):
    """writes and pattern_of are computed by torch ops on a side stream and are never on the host before the calls.  Two calls back to back on that
    stream: both write every stripe's absent data block, so the second one rebuilds old rows from the parity that the first one has just rewritten;
    the list, the status word and pattern_of are rewritten by device ops in between; one synchronise at the end."""
    torch = torch_cuda
    n, k, S, count = 20, 16, 64, 40
    patterns = [codeword_block(k, u) for u in range(n)]
    with prepared(fe, n, k, S, patterns) as enc:
        pool = SetPool(torch, enc, n, k, S, count, patterns, rotated(n, count), range(count), seed=77)
        start_d, start_p = pool.dd.clone(), pool.dp.clone()
        rows1, rows2 = pool.rows(count, S), pool.rows(count, S)
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            b = torch.randperm(count, device="cuda:0")
            lost = (n - b % n) % n                                   # rotated(n, count): stripe b loses codeword block (0 - b) mod n
            po = lost.to(torch.int32)
            writes = b * k + torch.where(lost < k, lost, (b * 5 + 3) % k)  # the absent data block where the stripe has one
            status = torch.full((1,), STATUS_GARBAGE, dtype=torch.int64, device="cuda:0")
            po_by_stripe = torch.empty(count, dtype=torch.int32, device="cuda:0")
            po_by_stripe[b] = po
            enc.update_batch_set_device(pool.dd, pool.dp, count, po_by_stripe, writes, count, rows1, status, stream=st.cuda_stream)
            list1, status1 = writes.clone(), status.clone()
            writes.copy_(torch.where(b % 3 == 0, torch.full_like(b, NONE), writes))  # every third stripe: skipped
            po_by_stripe.copy_(po_by_stripe.clone())
            status.fill_(STATUS_GARBAGE)
            enc.update_batch_set_device(pool.dd, pool.dp, count, po_by_stripe, writes, count, rows2, status, stream=st.cuda_stream)
        torch.cuda.synchronize()
        assert status1.item() == 0 and status.item() == 0
        assert po_by_stripe.tolist() == [int(q) for q in pool.pattern_of]
        list1, list2 = list1.tolist(), writes.tolist()
        assert pool.n_absent(list1) >= 30 and pool.n_absent(list2) >= 15 and NONE in list2
        got_d, got_p = pool.dd.clone(), pool.dp.clone()
        pool.dd.copy_(start_d)
        pool.dp.copy_(start_p)
        for ws, rows in ((list1, rows1), (list2, rows2)):  # the same two lists through the host-list call
            pool.dd, pool.dp = pool.reference(ws, rows, (0, S), "batch", None)
        assert torch.equal(got_d, pool.dd) and torch.equal(got_p, pool.dp)


def test_prepare_set_between_calls_on_two_streams(torch_cuda, fe):
    torch = torch_cuda
    n, k, S, count = 20, 16, 260, 40
    first = [codeword_block(k, u) for u in range(n)]
    second = [two_blocks(k, n, u) for u in range(n)]
    with prepared(fe, n, k, S, first) as enc:
        a = SetPool(torch, enc, n, k, S, count, first, rotated(n, count), range(count), seed=5)
        enc.decode_prepare_set(*flag_rows(k, n - k, second))
        b = SetPool(torch, enc, n, k, S, count, second, rotated(n, count), range(count), seed=6)
        wa, wb = aimed_writes(a.rng, k, count, first, a.pattern_of), aimed_writes(b.rng, k, count, second, b.pattern_of)
        rows_a, rows_b = a.rows(count, S), b.rows(count, S)
        want_b = b.reference(wb, rows_b, (0, S), "batch", None)
        enc.decode_prepare_set(*flag_rows(k, n - k, first))
        want_a = a.reference(wa, rows_a, (0, S), "batch", None)
        dwa, dwb = (torch.tensor(w, dtype=torch.int64, device="cuda:0") for w in (wa, wb))
        status = torch.full((2,), STATUS_GARBAGE, dtype=torch.int64, device="cuda:0")
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        enc.update_batch_set_device(a.dd, a.dp, count, a.po, dwa, count, rows_a, status[0:], stream=sa.cuda_stream)
        enc.decode_prepare_set(*flag_rows(k, n - k, second))  # waits for the call in flight before it swaps the tables
        enc.update_batch_set_device(b.dd, b.dp, count, b.po, dwb, count, rows_b, status[1:], stream=sb.cuda_stream)
        torch.cuda.synchronize()
        assert status.tolist() == [0, 0]
        assert torch.equal(a.dd, want_a[0]) and torch.equal(a.dp, want_a[1]), "the write before the new set"
        assert torch.equal(b.dd, want_b[0]) and torch.equal(b.dp, want_b[1]), "the write under the new set"


def test_a_device_read_while_a_device_write_is_in_flight(torch_cuda, fe):
    torch = torch_cuda
    n, k, S, count = 20, 16, 260, 40
    patterns = [codeword_block(k, u) for u in range(n)]
    with prepared(fe, n, k, S, patterns) as enc:
        w = SetPool(torch, enc, n, k, S, count, patterns, rotated(n, count), range(count), seed=8)
        r = SetPool(torch, enc, n, k, S, count, patterns, rotated(n, count, down=3), range(count), seed=9)
        writes = aimed_writes(w.rng, k, count, patterns, w.pattern_of)
        rows = w.rows(count, S)
        want = w.reference(writes, rows, (0, S), "batch", None)
        reads = aimed_writes(r.rng, k, count, patterns, r.pattern_of)
        dwrites, dreads = (torch.tensor(x, dtype=torch.int64, device="cuda:0") for x in (writes, reads))
        out = torch.full((count * S,), 0x3C3C3C3C, dtype=torch.int32, device="cuda:0")
        status = torch.full((2,), STATUS_GARBAGE, dtype=torch.int64, device="cuda:0")
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        enc.update_batch_set_device(w.dd, w.dp, count, w.po, dwrites, count, rows, status[0:], stream=sa.cuda_stream)
        enc.read_batch_set_device(r.dd, r.dp, count, r.po, dreads, count, out, status[1:], stream=sb.cuda_stream)
        torch.cuda.synchronize()
        assert status.tolist() == [0, 0]
        assert torch.equal(w.dd, want[0]) and torch.equal(w.dp, want[1])
        assert np.array_equal(host(out).reshape(count, S), r.X.reshape(-1, S)[reads])


# ---- 11. what the return value covers, with a live context ----
def test_host_refusals_with_a_live_context(torch_cuda, fe):
    torch = torch_cuda
    n, k, S, count = 20, 16, 16, 3
    patterns = [([2], [1])]
    lib = fe.lib()
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        pool = SetPool(torch, enc, n, k, S, count, patterns, [0, 0, PATTERN_NONE], range(count), seed=66)
        enc.decode_prepare_set([], [])
        before = pool.dd.clone(), pool.dp.clone()
        rows = pool.rows(4, S)
        dw = torch.tensor([1, 2, NONE, 0, 0], dtype=torch.int64, device="cuda:0")
        status = torch.full((2,), STATUS_GARBAGE, dtype=torch.int64, device="cuda:0")
        d, p, w, r, s, po = pool.dd.data_ptr(), pool.dp.data_ptr(), dw.data_ptr(), rows.data_ptr(), status.data_ptr(), pool.po.data_ptr()

        def both(code, h=enc._h, writes=w, n_writes=3, mps=1, col0=0, width=S, new=r, st=s, cnt=count, pattern_of=po, parity=p):
            assert lib.fastecc_update_batch_set_device(h, d, parity, cnt, pattern_of, writes, n_writes, mps, n_writes, col0, width, new, st, None) == code
            assert lib.fastecc_update_parity_batch_set_device(h, parity, cnt, pattern_of, writes, n_writes, mps, col0, width, None, new, st, None) == code

        both(fe.E_INVAL)                                          # no set prepared
        both(fe.E_INVAL, n_writes=0)                              # ... with nothing to write, too
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        both(fe.E_INVAL, mps=17)
        both(fe.E_INVAL, pattern_of=None)
        both(fe.E_INVAL, pattern_of=po + 2)
        both(fe.E_INVAL, pattern_of=p + 4 * (count * (n - k) * S - 1))  # pattern_of reaching the pool's last word
        both(fe.E_INVAL, pattern_of=r)                            # ... on the rows
        both(fe.E_INVAL, pattern_of=w + 8)                        # ... inside the list
        both(fe.E_INVAL, pattern_of=s)                            # ... on the status word
        both(fe.E_INVAL, col0=1, width=S)
        both(fe.E_INVAL, writes=p + 8)                            # what fastecc_update_batch_device refuses: the list inside the parity pool
        both(fe.E_INVAL, new=p)
        both(fe.E_UNSUPPORTED, cnt=(1 << 24) + 1)
        with fe.Encoder(n, k, 4 * S) as pitched:
            pitched.set_option("row_pitch_words", S + 4)
            both(fe.E_UNSUPPORTED, h=pitched._h)
        with fe.Encoder(64, 32, 4 * S, field=fe.FIELD_GF_P61_SQUARED) as e61:
            both(fe.E_UNSUPPORTED, h=e61._h, cnt=1)
        torch.cuda.synchronize()
        assert status.tolist() == [STATUS_GARBAGE] * 2 and torch.equal(pool.dd, before[0]) and torch.equal(pool.dp, before[1])
        pool.apply([2, 2 * k + 3], 1, what="a valid call after the refusals")
