"""GPU tests (-m gpu) of the sub-block pool writes: the window forms of update_batch, update_parity_batch, update_batch_set and
update_parity_batch_set (fastecc_update_*_window).

The truth is kept on the host: the data X of every stripe and its parity from the ORACLE (tests/pool_model.Codec.parity; never the library's own
encode or update).  The pool image handed to the library is the truth with seeded garbage — every third word >= p — in every word that must
not matter: all columns outside the columns a test's calls may touch in every block of the touched stripes, all absent blocks, all untouched stripes.
After a call with writes W, window (col0, width) and rows N, X' = X with words [col0, col0 + width) of the written blocks replaced, and the WHOLE
pool image is compared: the window columns of present blocks of touched stripes hold X' and the oracle's parity of X' there, every other word is
byte-identical to before.  The rows handed in (new, old) sit between guard bands and are unchanged as well.
The oracle works column by column, so the parity of all stripes of a pool is ONE oracle call on the stripes laid side by side."""
import ctypes

import numpy as np
import pytest

from footprint import Banded
from pool_model import MIXED_RADIX, Codec

pytestmark = pytest.mark.gpu

P = 0xFFF00001
NONE = 0xFFFFFFFF  # FASTECC_PATTERN_NONE


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


def rand_words(rng, shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64).astype(np.uint32)


def garbage(rng, shape):
    """arbitrary 32-bit words, every third one >= p (not a field element)"""
    g = rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
    flat = g.reshape(-1)
    flat[::3] = (P + rng.integers(0, (1 << 32) - P, size=len(flat[::3]), dtype=np.uint64)).astype(np.uint32)
    return g


def flag_rows(k, m, patterns):
    dp, pp = np.ones((len(patterns), k), np.uint8), np.ones((len(patterns), m), np.uint8)
    for q, (ld, lp) in enumerate(patterns):
        dp[q, list(ld)] = 0
        pp[q, list(lp)] = 0
    return dp, pp


def codeword_block(k, u):
    return ([u], []) if u < k else ([], [u - k])


def two_blocks(k, n, u):
    """codeword blocks u and u + 1 (mod n)"""
    a, b = codeword_block(k, u), codeword_block(k, (u + 1) % n)
    return (sorted(a[0] + b[0]), sorted(a[1] + b[1]))


def rotated(n, count, down=0):
    """placement (i + b) mod n with device `down` lost: stripe b loses codeword block (down - b) mod n — the pattern of that index"""
    return [(down - b) % n for b in range(count)]


def parity_of_pool(codec, X):
    """the oracle's parity [count, m, S] of the stripes X [count, k, S]: one call on the stripes side by side"""
    count, k, S = X.shape
    side = np.ascontiguousarray(X.transpose(1, 0, 2)).reshape(k, count * S)
    return np.ascontiguousarray(codec.parity(side).reshape(codec.m, count, S).transpose(1, 0, 2))


_TRUTH = {}


def truth(oracle, n, k, S, count, flags=0, order=0, seed=0):
    """(X, parity) of a pool, computed once per shape and shared (read-only: callers copy)"""
    key = (n, k, S, count, flags, order, seed)
    if key not in _TRUTH:
        X = rand_words(np.random.default_rng(1000 + seed + S), (count, k, S))
        Par = parity_of_pool(Codec(oracle, n, k, flags, order), X)
        X.setflags(write=False)
        Par.setflags(write=False)
        _TRUTH[key] = (X, Par)
    return _TRUTH[key]


class Pool:
    """The truth of a pool, its image on the device, and one checked call after another.
    live: {stripe: [(col0, width), ...]} — the stripes some call will touch, each with the columns its calls may touch (None: every column); every
    other word of the pool holds garbage, as do the absent blocks (the blocks the stripe's pattern loses).  parity_only: the data lives elsewhere (the
    truth X) and only the parity flags of a pattern matter."""

    def __init__(self, torch, enc, codec, base, S, count, live, seed, patterns=(), pattern_of=None, parity_only=False):
        self.torch, self.enc, self.codec = torch, enc, codec
        self.S, self.count, self.k, self.m = S, count, codec.k, codec.m
        self.patterns = list(patterns)
        self.pattern_of = np.array([NONE] * count if pattern_of is None else pattern_of, dtype=np.uint32)
        self.rng = rng = np.random.default_rng(seed)
        self.live = np.zeros(count, bool)
        self.cols = np.zeros((count, S), bool)  # the columns of each stripe that hold the truth
        for b, windows in live.items():
            self.live[b] = True
            for c0, w in ([(0, S)] if windows is None else windows):
                self.cols[b, c0:c0 + w] = True
        self.absent_d, self.absent_p = np.zeros((count, self.k), bool), np.zeros((count, self.m), bool)
        for b in np.flatnonzero(self.live):
            q = int(self.pattern_of[b])
            if q != NONE:
                if not parity_only:
                    self.absent_d[b, list(self.patterns[q][0])] = True
                self.absent_p[b, list(self.patterns[q][1])] = True
        self.X, self.Par = base[0].copy(), base[1].copy()
        self.img_d, self.img_p = self.X.copy(), self.Par.copy()
        for img, absent in ((self.img_d, self.absent_d), (self.img_p, self.absent_p)):
            dead = absent[:, :, None] | ~self.cols[:, None, :]
            img[dead] = garbage(rng, int(dead.sum()))
        self.dd, self.dp = to_dev(torch, self.img_d), to_dev(torch, self.img_p)
        self.touched = np.zeros(count, bool)
        self.parity_only = parity_only

    def new_rows(self, writes, width):
        return rand_words(self.rng, (len(writes), width))

    def expect(self, writes, window, values, data=True):
        """the truth and the image after a call that makes words [col0, col0 + width) of the written blocks `values`"""
        c0, w = window
        touched = np.zeros(self.count, bool)
        touched[[x // self.k for x in writes]] = True
        assert self.live[touched].all() and self.cols[touched, c0:c0 + w].all(), "the test's own bookkeeping: a call stays inside what it declared"
        self.touched |= touched
        self.X.reshape(self.count * self.k, self.S)[writes, c0:c0 + w] = values
        self.Par[touched] = parity_of_pool(self.codec, self.X[touched])
        if data:
            b, j = np.nonzero(touched[:, None] & ~self.absent_d)
            self.img_d[b, j, c0:c0 + w] = self.X[b, j, c0:c0 + w]
        b, j = np.nonzero(touched[:, None] & ~self.absent_p)
        self.img_p[b, j, c0:c0 + w] = self.Par[b, j, c0:c0 + w]

    def check_image(self, what=""):
        """the WHOLE pool image: window columns of present blocks of touched stripes hold the new truth, every other word what it held"""
        self.torch.cuda.synchronize()
        got_d, got_p = host(self.dd).reshape(self.img_d.shape), host(self.dp).reshape(self.img_p.shape)
        for name, got, want in (("data", got_d, self.img_d), ("parity", got_p, self.img_p)):
            bad = got != want
            assert not bad.any(), "%s: wrong %s words (stripe, block, column), first ones %r" % (what, name, np.argwhere(bad)[:8].tolist())

    def call(self, form, writes, window=None, new=None, with_old=True, skew=0, stream=0, what="", check=True):
        """one call of `form` (batch, parity, batch_set, parity_set) with the window (None: the whole-block entry point), its rows between guard
        bands (`skew` words off a 16-byte boundary), the expectation moved on and everything checked"""
        torch, enc = self.torch, self.enc
        c0, w = window or (0, self.S)
        kw = {} if window is None else dict(col0=c0, width=w)
        new = self.new_rows(writes, w) if new is None else new
        rows = self.X.reshape(self.count * self.k, self.S)
        old = rows[writes, c0:c0 + w].copy()
        bn = Banded(torch, new, 2, w, 71, skew_words=skew)
        bands = [(bn, new)]
        assert bn.ptr % 16 == 4 * skew
        arr = np.array(writes, dtype=np.uint64)
        if form in ("parity", "parity_set"):
            assert self.parity_only
            bo = None
            if with_old:
                bo = Banded(torch, old, 2, w, 72)
                bands.append((bo, old))
            if form == "parity":
                enc.update_parity_batch(self.dp, self.count, arr, bn.view, old=bo.view if bo else None, stream=stream, **kw)
            else:
                enc.update_parity_batch_set(self.dp, self.count, self.pattern_of, arr, bn.view, old=bo.view if bo else None, stream=stream, **kw)
            # old rows given: the windows become `new`; from zero: the parity moves as if `new` had been ADDED to them (the code is linear)
            values = new if with_old else ((old.astype(np.uint64) + new) % P).astype(np.uint32)
            self.expect(writes, (c0, w), values, data=False)
        else:
            assert not self.parity_only
            if form == "batch":
                enc.update_batch(self.dd, self.dp, self.count, arr, bn.view, stream=stream, **kw)
            else:
                enc.update_batch_set(self.dd, self.dp, self.count, self.pattern_of, arr, bn.view, stream=stream, **kw)
            self.expect(writes, (c0, w), new)
        arr[:] = 0xFFFFFFFFFFFFFFFF  # the list may be reused as soon as the call returns
        if check:
            self.check_image(what)
            self.check_rows(bands, what)
        return bands

    def check_rows(self, bands, what=""):
        for band, want in bands:
            assert np.array_equal(band.host(), want), what + ": the rows are only read"
            band.check(what + " (rows)")

    def check_reads(self, window):
        """before any repair: the window of every absent WRITTEN-stripe data block reads as its row of the truth (the new row where it was written)"""
        c0, w = window
        reads = [int(b) * self.k + int(i) for b, i in np.argwhere(self.absent_d & self.touched[:, None])]
        assert reads
        out = self.torch.full((len(reads) * w,), 0x3C3C3C3C, dtype=self.torch.int32, device="cuda:0")
        self.enc.read_batch_set(self.dd, self.dp, self.count, self.pattern_of, reads, out, col0=c0, width=w)
        self.torch.cuda.synchronize()
        assert np.array_equal(host(out).reshape(len(reads), w), self.X.reshape(-1, self.S)[reads, c0:c0 + w])

    def check_repair(self):
        """repair of a clone under the same patterns, the garbage columns of the touched stripes' present blocks first replaced by the truth there,
        gives the oracle's full stripes (stripes never touched: not repaired, byte-identical)"""
        t = self.touched
        fixed_d, fixed_p = self.img_d.copy(), self.img_p.copy()
        for fixed, true, absent in ((fixed_d, self.X, self.absent_d), (fixed_p, self.Par, self.absent_p)):
            sel = (t[:, None] & ~absent)[:, :, None] & ~self.cols[:, None, :]
            fixed[sel] = true[sel]
        cd, cp = to_dev(self.torch, fixed_d), to_dev(self.torch, fixed_p)
        po = np.where(t, self.pattern_of, NONE).astype(np.uint32)
        self.enc.repair_batch_set(cd, cp, self.count, po)
        self.torch.cuda.synchronize()
        got_d, got_p = host(cd).reshape(self.X.shape), host(cp).reshape(self.Par.shape)
        assert np.array_equal(got_d[t], self.X[t]) and np.array_equal(got_p[t], self.Par[t])
        assert np.array_equal(got_d[~t], self.img_d[~t]) and np.array_equal(got_p[~t], self.img_p[~t])


# ---- 1. windows at the edges of the width rule ----
def lane_words(S, col0, width, skew):
    """the width rule: the widest of 4, 2, 1 that divides S, col0 and width and leaves the rows' pointer on a V-word boundary"""
    v = 4
    while v > 1 and ((S | col0 | width) % v or (4 * skew) % (4 * v)):
        v //= 2
    return v


EDGE_WINDOWS = ([(260, c, w, 4) for c, w in [(0, 260), (4, 256), (4, 128), (8, 252)]] + [(260, c, w, 2) for c, w in [(2, 66), (6, 254)]]
                + [(260, c, w, 1) for c, w in [(0, 1), (259, 1), (3, 1), (1, 130), (5, 255), (1, 64), (1, 65)]]
                + [(65, c, w, 1) for c, w in [(0, 65), (1, 64), (64, 1)]] + [(1025, c, w, 1) for c, w in [(1, 1024), (513, 512)]])


@pytest.mark.parametrize("skew", [0, 1], ids=["aligned", "new_rows_off_by_4_bytes"])
@pytest.mark.parametrize("S,col0,width,V", EDGE_WINDOWS, ids=["S%d_c%d_w%d" % c[:3] for c in EDGE_WINDOWS])
def test_windows_at_the_edges_of_the_width_rule(torch_cuda, fe, oracle, S, col0, width, V, skew):
    n, k, count = 20, 16, 12
    assert lane_words(S, col0, width, 0) == V and lane_words(S, col0, width, 1) == 1  # what the case is named for
    rng = np.random.default_rng(S * 1000 + col0 + width)
    stripes = sorted(int(b) for b in rng.permutation(count)[:8])
    writes = [b * k + int(rng.integers(k)) for b in stripes]
    writes = [writes[i] for i in rng.permutation(len(writes))]
    assert len({x // k for x in writes}) == 8
    with fe.Encoder(n, k, 4 * S) as enc:
        pool = Pool(torch_cuda, enc, Codec(oracle, n, k), truth(oracle, n, k, S, count), S, count, {b: [(col0, width)] for b in stripes}, seed=col0 + width)
        pool.call("batch", writes, (col0, width), skew=skew, what="S = %d, window (%d, %d)" % (S, col0, width))


# ---- 2. row classes and rounds ----
def test_row_classes_and_rounds(torch_cuda, fe, oracle):
    n, k, S, count, window = 48, 32, 64, 10, (5, 40)
    per_stripe = [1, 2, 3, 5, 9, 16, 17, 20]
    rng = np.random.default_rng(2)
    stripes = sorted(int(b) for b in rng.permutation(count)[:len(per_stripe)])
    writes = [b * k + int(i) for b, t in zip(stripes, per_stripe) for i in rng.permutation(k)[:t]]
    writes = [writes[i] for i in rng.permutation(len(writes))]
    assert sorted(np.bincount([x // k for x in writes], minlength=count)) == [0, 0] + per_stripe  # classes 1, 2, 4, 8, 16 and a second round
    with fe.Encoder(n, k, 4 * S) as enc:
        pool = Pool(torch_cuda, enc, Codec(oracle, n, k), truth(oracle, n, k, S, count), S, count, {b: [window] for b in stripes}, seed=22)
        pool.call("batch", writes, window)


# ---- 3. code families ----
@pytest.mark.parametrize("n,k,S,flags,order", [(32, 8, 32, 0, 0), (72, 48, 64, MIXED_RADIX, 48), (100, 70, 20, 0, 0)],
                         ids=["32_8", "72_48_mixed", "100_70"])
def test_code_families(torch_cuda, fe, oracle, n, k, S, flags, order):
    count = 7
    window = (3, min(21, S - 3))  # (S = 20: the window ends with the block)
    rng = np.random.default_rng(n)
    stripes = [0, 2, 3, 5, 6]
    writes = [b * k + int(i) for b in stripes for i in rng.permutation(k)[:3]]
    writes = [writes[i] for i in rng.permutation(len(writes))]
    with fe.Encoder(n, k, 4 * S, flags=flags) as enc:
        pool = Pool(torch_cuda, enc, Codec(oracle, n, k, flags, order), truth(oracle, n, k, S, count, flags, order), S, count,
                    {b: [window] for b in stripes}, seed=n)
        pool.call("batch", writes, window)


# ---- 4. degraded, the set form ----
def degraded_writes(rng, k, count, patterns, pattern_of):
    """per stripe: the absent data block where the stripe has one (every other such stripe also a present one), else a random block"""
    writes = []
    for b in range(count):
        ld = patterns[pattern_of[b]][0]
        if ld:
            writes.append(b * k + int(ld[0]))
            if b % 2:
                writes.append(b * k + int(next(i for i in rng.permutation(k) if i not in ld)))
        else:
            writes.append(b * k + int(rng.integers(k)))
    return [writes[i] for i in rng.permutation(len(writes))]


def kinds_of(writes, k, patterns, pattern_of):
    kinds = set()
    for x in writes:
        ld, lp = patterns[pattern_of[x // k]]
        kinds.add("absent" if x % k in ld else "present")
        if lp:
            kinds.add("parity_absent")
    return kinds


@pytest.mark.parametrize("window", [(0, 130), (7, 64), (129, 1)], ids=lambda w: "c%d_w%d" % w)
def test_one_device_down(torch_cuda, fe, oracle, window):
    n, k, S, count = 20, 16, 130, 40
    patterns = [codeword_block(k, u) for u in range(n)]
    pattern_of = rotated(n, count)
    rng = np.random.default_rng(4)
    writes = degraded_writes(rng, k, count, patterns, pattern_of)
    assert kinds_of(writes, k, patterns, pattern_of) == {"present", "absent", "parity_absent"} and len(set(writes)) == len(writes)
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        pool = Pool(torch_cuda, enc, Codec(oracle, n, k), truth(oracle, n, k, S, count), S, count, {b: [window] for b in range(count)}, seed=44,
                    patterns=patterns, pattern_of=pattern_of)
        pool.call("batch_set", writes, window)
        pool.check_reads(window)
        pool.check_repair()


def test_two_devices_down(torch_cuda, fe, oracle):
    n, k, S, count, window = 20, 16, 130, 40, (7, 64)
    patterns = [two_blocks(k, n, u) for u in range(n)]
    assert {(len(ld), len(lp)) for ld, lp in patterns} == {(2, 0), (1, 1), (0, 2)}
    pattern_of = rotated(n, count)
    rng = np.random.default_rng(5)
    writes = degraded_writes(rng, k, count, patterns, pattern_of)
    both = next(b for b in range(count) if len(patterns[pattern_of[b]][0]) == 2)  # data + data lost: both written
    writes = sorted(set(writes) | {both * k + int(i) for i in patterns[pattern_of[both]][0]})
    assert kinds_of(writes, k, patterns, pattern_of) == {"present", "absent", "parity_absent"}
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        pool = Pool(torch_cuda, enc, Codec(oracle, n, k), truth(oracle, n, k, S, count), S, count, {b: [window] for b in range(count)}, seed=55,
                    patterns=patterns, pattern_of=pattern_of)
        pool.call("batch_set", writes, window)
        pool.check_reads(window)
        pool.check_repair()


# ---- 5. the parity forms ----
@pytest.mark.parametrize("with_old", [True, False], ids=["old_rows", "from_zero"])
@pytest.mark.parametrize("form", ["parity", "parity_set"])
def test_parity_forms(torch_cuda, fe, oracle, form, with_old):
    n, k, S, count, window = 20, 16, 130, 40, (6, 50)
    patterns = [codeword_block(k, u) for u in range(n)]
    pattern_of = rotated(n, count) if form == "parity_set" else None
    rng = np.random.default_rng(6)
    blocks = rng.permutation(count * k)[:60]
    writes = [int(x) for x in blocks]
    live = sorted({x // k for x in writes})
    with fe.Encoder(n, k, 4 * S) as enc:
        if form == "parity_set":
            enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
            assert any(patterns[pattern_of[b]][1] for b in live)  # some touched stripe misses a parity block: it must stay byte-identical
        pool = Pool(torch_cuda, enc, Codec(oracle, n, k), truth(oracle, n, k, S, count), S, count, {b: [window] for b in live}, seed=66,
                    patterns=patterns, pattern_of=pattern_of, parity_only=True)
        pool.call(form, writes, window, with_old=with_old)


# ---- 6. equivalences with the whole-block calls ----
@pytest.mark.parametrize("form", ["batch", "parity", "batch_set", "parity_set"])
def test_equivalence_with_the_whole_block_call(torch_cuda, fe, oracle, form):
    torch = torch_cuda
    n, k, S, count = 20, 16, 260, 12
    m = n - k
    patterns = [codeword_block(k, u) for u in range(n)]
    po = np.array(rotated(n, count), dtype=np.uint32)
    X, Par = truth(oracle, n, k, S, count)  # a clean pool: every word < p
    rng = np.random.default_rng(7)
    writes = [int(x) for x in rng.permutation(count * k)[:40]]
    old = X.reshape(-1, S)[writes].copy()
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, m, patterns))

        def run(dd, dp, new, old_rows, **kw):
            dn, do = to_dev(torch, new), to_dev(torch, old_rows)
            if form == "batch":
                enc.update_batch(dd, dp, count, writes, dn, **kw)
            elif form == "parity":
                enc.update_parity_batch(dp, count, writes, dn, old=do, **kw)
            elif form == "batch_set":
                enc.update_batch_set(dd, dp, count, po, writes, dn, **kw)
            else:
                enc.update_parity_batch_set(dp, count, po, writes, dn, old=do, **kw)
            torch.cuda.synchronize()
            return host(dd), host(dp)

        def pools():
            return to_dev(torch, X.copy()), to_dev(torch, Par.copy())

        whole_new = rand_words(rng, (len(writes), S))
        want = run(*pools(), whole_new, old)
        got = run(*pools(), whole_new, old, col0=0, width=S)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "window (0, S) against the whole-block form"
        assert not np.array_equal(want[1], Par.reshape(-1))
        c0, w = 4, 128
        patched = old.copy()
        patched[:, c0:c0 + w] = rand_words(rng, (len(writes), w))
        want = run(*pools(), patched, old)
        got = run(*pools(), patched[:, c0:c0 + w], old[:, c0:c0 + w], col0=c0, width=w)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "window (4, 128) against the old block with the window replaced"
        assert not np.array_equal(want[1], Par.reshape(-1))


# ---- 7. several calls on one context ----
def test_several_calls_on_one_context(torch_cuda, fe, oracle):
    """Three window calls back to back on one stream with different windows and list lengths (the staged lists are reused, the reconstruction buffer
    changes its pitch), a whole-block update_batch_set and a whole-block update_batch, then a window call again; checked after each step."""
    torch = torch_cuda
    n, k, S, count = 20, 16, 130, 40
    patterns = [codeword_block(k, u) for u in range(n)]
    pattern_of = rotated(n, count)
    rng = np.random.default_rng(8)
    live = {b: None for b in range(34)}
    po = list(pattern_of)
    for b in (30, 31, 32, 33):
        po[b] = NONE  # (every stripe of the rotated pool misses a block: whole stripes, for update_batch)
    lists = [degraded_writes(rng, k, 30, patterns, po), degraded_writes(rng, k, 12, patterns, po)[:9], degraded_writes(rng, k, 25, patterns, po)]
    assert len({len(x) for x in lists}) == 3
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        pool = Pool(torch, enc, Codec(oracle, n, k), truth(oracle, n, k, S, count), S, count, live, seed=88, patterns=patterns, pattern_of=po)
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        for step, (writes, window) in enumerate(zip(lists, [(7, 64), (0, 130), (129, 1)])):
            pool.call("batch_set", writes, window, stream=st.cuda_stream, what="window call %d" % step)
        pool.call("batch_set", lists[1], None, stream=st.cuda_stream, what="whole-block update_batch_set")
        pool.call("batch", [30 * k + 1, 31 * k, 31 * k + 15, 33 * k + 7], None, stream=st.cuda_stream, what="whole-block update_batch")
        pool.call("batch_set", lists[0], (2, 66), stream=st.cuda_stream, what="a window call after the whole-block calls")
        pool.call("batch", [30 * k + 1, 32 * k + 3], (100, 30), stream=st.cuda_stream, what="a window update_batch on whole stripes")
        pool.check_reads((0, S))
        pool.check_repair()


def test_calls_without_a_synchronise_between_them(torch_cuda, fe, oracle):
    """The same three window calls enqueued on one stream with no host synchronisation between them: the second and third rewrite blocks the first
    wrote, absent ones among them, so their reconstruction must see the earlier calls' parity."""
    torch = torch_cuda
    n, k, S, count = 20, 16, 130, 40
    patterns = [codeword_block(k, u) for u in range(n)]
    pattern_of = rotated(n, count)
    rng = np.random.default_rng(9)
    lists = [degraded_writes(rng, k, 40, patterns, pattern_of), degraded_writes(rng, k, 15, patterns, pattern_of), degraded_writes(rng, k, 33, patterns, pattern_of)]
    windows = [(4, 64), (0, 130), (60, 9)]
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        pool = Pool(torch, enc, Codec(oracle, n, k), truth(oracle, n, k, S, count), S, count, {b: None for b in range(count)}, seed=99,
                    patterns=patterns, pattern_of=pattern_of)
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        bands = []
        for writes, window in zip(lists, windows):
            bands += pool.call("batch_set", writes, window, stream=st.cuda_stream, check=False)
        pool.check_image("three calls on one stream")
        pool.check_rows(bands)
        pool.check_repair()


# ---- 8. refusals with a live context ----
def test_refusals_leave_the_pool_and_the_rows_unchanged(torch_cuda, fe, oracle):
    torch = torch_cuda
    n, k, S, count = 20, 16, 16, 6
    m = n - k
    patterns = [([2], []), ([], [1])]
    pattern_of = [0, 1, NONE, 0, 1, 0]
    rng = np.random.default_rng(10)
    with fe.Encoder(n, k, 4 * S) as enc:
        pool = Pool(torch, enc, Codec(oracle, n, k), truth(oracle, n, k, S, count), S, count, {b: None for b in range(count)}, seed=100,
                    patterns=patterns, pattern_of=pattern_of)
        rows = to_dev(torch, rand_words(rng, (4, S)))
        r0 = rows.clone()
        po = pool.pattern_of

        def calls(writes, new, old, **kw):
            return [lambda: enc.update_batch(pool.dd, pool.dp, count, writes, new, **kw),
                    lambda: enc.update_parity_batch(pool.dp, count, writes, new, old=old, **kw),
                    lambda: enc.update_batch_set(pool.dd, pool.dp, count, po, writes, new, **kw),
                    lambda: enc.update_parity_batch_set(pool.dp, count, po, writes, new, old=old, **kw)]

        def refused(code, fns):
            for fn in fns:
                with pytest.raises(fe.FastEccError) as ei:
                    fn()
                assert ei.value.code == code
            pool.check_image("after a refusal")
            assert torch.equal(rows, r0)

        refused(fe.E_INVAL, calls([1, 2], rows, rows, col0=2, width=4)[2:])            # the set forms with no set prepared
        refused(fe.E_INVAL, calls([], rows, rows, col0=2, width=4)[2:])                # ... with nothing to write, too
        enc.decode_prepare_set(*flag_rows(k, m, patterns))
        refused(fe.E_INVAL, calls([1, 2], rows, rows, col0=1, width=S))                # col0 + width = S + 1
        refused(fe.E_INVAL, calls([1, 2], rows, rows, col0=S, width=1))
        lib = fe.lib()
        one = (ctypes.c_uint64 * 1)(1)
        for c0, w in ((S + 1, (1 << 64) - 1), (1, (1 << 64) - 1), (0, 0), (0, S + 1)):  # (past what the Python methods let through)
            assert lib.fastecc_update_batch_window(enc._h, pool.dd.data_ptr(), pool.dp.data_ptr(), count, one, 1, c0, w, rows.data_ptr(), None) == fe.E_INVAL
            assert lib.fastecc_update_parity_batch_set_window(enc._h, pool.dp.data_ptr(), count, po.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), one, 1, c0, w,
                                                              None, rows.data_ptr(), None) == fe.E_INVAL
        refused(fe.E_INVAL, [])  # (nothing more to call: the image and the rows after the calls above)
        # rows overlapping the pool, as n_writes * width words: the last 8 words of the parity pool are 2 rows of 4 — inside — and 2 rows of 4 that
        # start 4 words before the pool reach into it
        refused(fe.E_INVAL, calls([1, 2], pool.dp[count * m * S - 8:], rows, col0=2, width=4))       # new inside the parity pool
        refused(fe.E_INVAL, calls([1, 2], rows, pool.dp[S:], col0=2, width=4)[1::2])                 # old inside the parity pool
        refused(fe.E_INVAL, calls([1, 2], pool.dd[5 * S:], rows, col0=2, width=4)[0::2])             # new inside the data pool (the forms that have one)
        refused(fe.E_INVAL, calls([1, 1], rows, rows, col0=0, width=4))                              # what the whole-block forms refuse: a duplicate
        refused(fe.E_INVAL, calls([1, count * k], rows, rows, col0=0, width=4))                      # ... an index >= count * k
        with fe.Encoder(n, k, 4 * S) as pitched:
            pitched.set_option("row_pitch_words", S + 4)
            fns = [lambda: pitched.update_batch(pool.dd, pool.dp, 1, [1], rows, col0=2, width=4),
                   lambda: pitched.update_parity_batch(pool.dp, 1, [1], rows, col0=2, width=4),
                   lambda: pitched.update_batch_set(pool.dd, pool.dp, 1, [NONE], [1], rows, col0=2, width=4),
                   lambda: pitched.update_parity_batch_set(pool.dp, 1, [NONE], [1], rows, col0=2, width=4)]
            refused(fe.E_UNSUPPORTED, fns)                                                            # a row_pitch_words context
        # n_writes == 0 is a no-op
        for fn in calls([], rows[:0], rows[:0], col0=2, width=4):
            fn()
        pool.check_image("no writes")
        # after the refusals a valid call still gives the right pool
        pool.call("batch_set", [2, 5, k + 2, 2 * k, 5 * k + 2, 4 * k + 7], (2, 4), what="a valid call after the refusals")
        pool.check_repair()
