"""GPU tests (-m gpu) of the degraded writes: fastecc_update_batch_set and fastecc_update_parity_batch_set.

The truth is kept on the host: the data X of every stripe and its parity from the ORACLE (tests/pool_model.Codec.parity; never the library's own
encode or update).  The pool handed to the library is the truth with every ABSENT block — the blocks its stripe's pattern loses — and every
stripe that no call will touch overwritten by seeded garbage that includes words >= p.  After a call with writes W and rows N, X' = X with the
written blocks replaced, and all of this is checked:
  (a) every present block of every touched stripe equals X' / the oracle's parity of X';
  (b) every absent block, every untouched stripe and the new rows are byte-identical to before ((a) and (b) together: the whole pool image);
  (c) fastecc_repair_batch_set on a clone makes the touched stripes equal the oracle's full stripe;
  (d) fastecc_read_batch_set of every absent data block of the touched stripes, issued before the repair, returns its row of X' — the new row
      where the block was written, the true old one where it was not.
The oracle works column by column, so the parity of all stripes of a pool is ONE oracle call on the stripes laid side by side."""
import ctypes

import numpy as np
import pytest

from footprint import Banded, BandedHost
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


class Degraded:
    """The truth of a pool, its damaged image on the device, and one checked call after another.  `live`: the stripes some call will touch
    (every other stripe holds garbage in all its blocks).  pattern_of may name patterns the set does not have on stripes outside `live`."""

    def __init__(self, torch, fe, enc, codec, S, count, patterns, pattern_of, live, seed, banded=False):
        self.torch, self.fe, self.enc, self.codec = torch, fe, enc, codec
        self.S, self.count, self.k, self.m = S, count, codec.k, codec.m
        self.patterns, self.pattern_of = patterns, np.array(pattern_of, dtype=np.uint32)
        self.rng = rng = np.random.default_rng(seed)
        self.live = np.zeros(count, bool)
        self.live[list(live)] = True
        self.absent_d, self.absent_p = np.zeros((count, self.k), bool), np.zeros((count, self.m), bool)
        for b in np.flatnonzero(self.live):
            q = int(self.pattern_of[b])
            if q != NONE:
                self.absent_d[b, list(patterns[q][0])] = True
                self.absent_p[b, list(patterns[q][1])] = True
        self.X = rand_words(rng, (count, self.k, S))
        self.Par = parity_of_pool(codec, self.X)
        dead_d = self.absent_d | ~self.live[:, None]
        dead_p = self.absent_p | ~self.live[:, None]
        self.img_d, self.img_p = self.X.copy(), self.Par.copy()
        self.img_d[dead_d] = garbage(rng, (int(dead_d.sum()), S))
        self.img_p[dead_p] = garbage(rng, (int(dead_p.sum()), S))
        self.bands = []
        if banded:
            bd, bp = Banded(torch, self.img_d.reshape(-1, S), 2, S, seed + 1), Banded(torch, self.img_p.reshape(-1, S), 2, S, seed + 2)
            self.dd, self.dp, self.bands = bd.view, bp.view, [bd, bp]
            self.po_band = BandedHost(self.pattern_of.reshape(1, count), 2, count, seed + 3)
            self.bands.append(self.po_band)
            self.po = self.po_band.view  # (a contiguous uint32 numpy view: Encoder passes it through as it is)
        else:
            self.dd, self.dp, self.po = to_dev(torch, self.img_d), to_dev(torch, self.img_p), self.pattern_of
        self.touched = np.zeros(count, bool)

    def new_rows(self, writes):
        return rand_words(self.rng, (len(writes), self.S))

    def expect(self, writes, new):
        """the truth and the image after update_batch_set(writes, new)"""
        self.X.reshape(self.count * self.k, self.S)[writes] = new
        self._expect_touched(writes, data=True)

    def _expect_touched(self, writes, data):
        touched = np.zeros(self.count, bool)
        touched[[w // self.k for w in writes]] = True
        assert self.live[touched].all(), "the test's own bookkeeping: a call touches live stripes only"
        self.touched |= touched
        self.Par = parity_of_pool(self.codec, self.X)
        if data:
            sel = touched[:, None] & ~self.absent_d
            self.img_d[sel] = self.X[sel]
        sel = touched[:, None] & ~self.absent_p
        self.img_p[sel] = self.Par[sel]

    def check_image(self, what=""):
        """(a) and (b): present blocks of touched stripes hold the new truth, everything else what it held"""
        self.torch.cuda.synchronize()
        got_d, got_p = host(self.dd).reshape(self.img_d.shape), host(self.dp).reshape(self.img_p.shape)
        for name, got, want in (("data", got_d, self.img_d), ("parity", got_p, self.img_p)):
            bad = (got != want).any(axis=2)
            assert not bad.any(), "%s: wrong %s blocks (stripe, block), first ones %r" % (what, name, np.argwhere(bad)[:8].tolist())
        for band in self.bands:
            band.check(what)

    def update(self, writes, new=None, stream=0, what=""):
        """one fastecc_update_batch_set, with (a) and (b) checked"""
        new = self.new_rows(writes) if new is None else new
        if self.bands:
            bn = Banded(self.torch, new, 2, self.S, 77)
            dn, extra = bn.view, [bn]
        else:
            dn, extra = to_dev(self.torch, new), []
        self.enc.update_batch_set(self.dd, self.dp, self.count, self.po, writes, dn, stream=stream)
        self.expect(writes, new)
        self.check_image(what)
        assert np.array_equal(host(dn).reshape(new.shape), new), "the new rows are only read"
        for band in extra:
            band.check(what + " (new rows)")

    def check_reads(self):
        """(d): every absent data block of the touched stripes reads as its row of the truth"""
        reads = [int(b) * self.k + int(i) for b, i in np.argwhere(self.absent_d & self.touched[:, None])]
        if not reads:
            return
        out = self.torch.full((len(reads) * self.S,), 0x3C3C3C3C, dtype=self.torch.int32, device="cuda:0")
        self.enc.read_batch_set(self.dd, self.dp, self.count, self.po, reads, out)
        self.torch.cuda.synchronize()
        assert np.array_equal(host(out).reshape(len(reads), self.S), self.X.reshape(-1, self.S)[reads])

    def check_repair(self):
        """(c): repair of a clone under the same patterns (stripes never touched: not repaired) gives the oracle's full stripes"""
        cd, cp = self.dd.clone(), self.dp.clone()
        po = np.where(self.touched, self.pattern_of, NONE).astype(np.uint32)
        self.enc.repair_batch_set(cd, cp, self.count, po)
        self.torch.cuda.synchronize()
        got_d, got_p = host(cd).reshape(self.X.shape), host(cp).reshape(self.Par.shape)
        t = self.touched
        assert np.array_equal(got_d[t], self.X[t]) and np.array_equal(got_p[t], self.Par[t])
        assert np.array_equal(got_d[~t], self.img_d[~t]) and np.array_equal(got_p[~t], self.img_p[~t])

    def check_all(self):
        self.check_reads()
        self.check_repair()


def aimed_writes(rng, k, count, patterns, pattern_of, stripes=None):
    """one write per stripe, aimed at the absent data block where the stripe has one, else at a random block"""
    out = []
    for b in (range(count) if stripes is None else stripes):
        ld = patterns[pattern_of[b]][0] if pattern_of[b] != NONE else []
        out.append(b * k + (int(ld[0]) if ld else int(rng.integers(k))))
    return out


def random_writes(rng, k, stripes, t):
    """t distinct pool blocks among the stripes' data blocks"""
    blocks = np.array([b * k + i for b in stripes for i in range(k)])
    return [int(w) for w in rng.permutation(blocks)[:t]]


# ---- 1. one device of a rotated pool down; 7. the same with guard bands ----
def one_device_down(torch, fe, oracle, S, which, banded=False):
    n, k, count = 20, 16, 41
    patterns = [codeword_block(k, u) for u in range(n)]
    pattern_of = rotated(n, count)
    assert min(np.bincount(pattern_of, minlength=n)) >= 2
    rng = np.random.default_rng(100 + S)
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        if which == "aimed":
            live, writes = range(count), aimed_writes(rng, k, count, patterns, pattern_of)
        else:
            writes = random_writes(rng, k, range(count), 60)
            live = sorted({w // k for w in writes})
        pool = Degraded(torch, fe, enc, Codec(oracle, n, k), S, count, patterns, pattern_of, live, seed=S, banded=banded)
        pool.update(writes, what="S = %d, %s" % (S, which))
        pool.check_all()


@pytest.mark.parametrize("which", ["aimed", "random"])
@pytest.mark.parametrize("S", [1, 63, 65, 130, 260])
def test_one_device_down(torch_cuda, fe, oracle, S, which):
    one_device_down(torch_cuda, fe, oracle, S, which)


@pytest.mark.parametrize("which", ["aimed", "random"])
def test_guard_bands(torch_cuda, fe, oracle, which):
    one_device_down(torch_cuda, fe, oracle, 63, which, banded=True)


# ---- 2. two devices down ----
def test_two_devices_down(torch_cuda, fe, oracle):
    n, k, S, count = 20, 16, 65, 41
    patterns = [two_blocks(k, n, u) for u in range(n)]
    assert {(len(ld), len(lp)) for ld, lp in patterns} == {(2, 0), (1, 1), (0, 2)}
    pattern_of = rotated(n, count)
    rng = np.random.default_rng(2)
    both = next(b for b in range(count) if len(patterns[pattern_of[b]][0]) == 2)       # data + data lost
    stay = next(b for b in range(count) if b != both and patterns[pattern_of[b]][0])   # a data block stays absent
    ld = patterns[pattern_of[both]][0]
    present = [i for i in range(k) if i not in ld]
    writes = [both * k + i for i in list(ld) + present[:3]]
    writes += [stay * k + i for i in range(k) if i not in patterns[pattern_of[stay]][0]][:4]
    writes += aimed_writes(rng, k, count, patterns, pattern_of, [b for b in range(count) if b not in (both, stay)])
    writes = [writes[i] for i in rng.permutation(len(writes))]
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        pool = Degraded(torch_cuda, fe, enc, Codec(oracle, n, k), S, count, patterns, pattern_of, range(count), seed=22)
        pool.update(writes)
        pool.check_all()


# ---- 3. more than one round and more than one run ----
def test_twenty_writes_in_one_stripe(torch_cuda, fe, oracle):
    n, k, S, count = 48, 32, 64, 5
    patterns = [([3, 17], [5]), ([0], []), ([], [15])]
    pattern_of = [1, 0, NONE, 2, 7]     # (stripe 4 is not touched: its entry is not looked at)
    rng = np.random.default_rng(3)
    others = [i for i in rng.permutation(k) if i not in (3, 17)][:18]
    writes = [k + int(i) for i in [3, 17] + others] + [0, 2 * k + 9, 3 * k + 31, 3 * k]
    writes = [writes[i] for i in rng.permutation(len(writes))]
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        pool = Degraded(torch_cuda, fe, enc, Codec(oracle, n, k), S, count, patterns, pattern_of, range(4), seed=33)
        pool.update(writes)
        pool.check_all()


def test_sixteen_losses_and_the_edges_of_a_run(torch_cuda, fe, oracle):
    n, k, S, count = 256, 128, 64, 3
    rng = np.random.default_rng(4)
    ld = sorted(int(i) for i in rng.permutation(k)[:8])
    lp = sorted(int(i) for i in rng.permutation(n - k)[:8])
    patterns = [(ld, lp), ([], [0, 1, 127]), ([5], [])]
    present = [i for i in range(k) if i not in ld]
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        pool = Degraded(torch_cuda, fe, enc, Codec(oracle, n, k), S, count, patterns, [2, 0, 1], range(3), seed=44)
        pool.update([k + i for i in ld[:3] + present[:5]] + [5, 6], what="8 data + 8 parity blocks lost")
        pool.check_all()
        pool.update([2 * k + 40, 2 * k + 41], what="the stripe alone that lost parity blocks 0, 1 and 127")
        pool.check_all()


# Runs per segment: the small pools above have so few segments that every wave gets ONE parity block (run = 1; tests/test_gpu_update_batch.py,
# RUN_POOLS).  With 8192 touched stripes of (20,16) a wave walks the whole parity of its stripe (run = 4 on 256 CUs), with 3000 half of it
# (run = 2): the cursor through the lost list, the prefetch of the next PRESENT block, absent blocks at the start, in the middle and at the end of a run.
def test_several_parity_blocks_per_wave(torch_cuda, fe, oracle):
    n, k, S, count = 20, 16, 4, 8192
    patterns = [two_blocks(k, n, u) for u in range(n)] + [([], [0, 3]), ([], [1, 2]), ([2], [0, 1, 2])]
    pattern_of = [b % len(patterns) for b in range(count)]
    rng = np.random.default_rng(5)
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        pool = Degraded(torch_cuda, fe, enc, Codec(oracle, n, k), S, count, patterns, pattern_of, range(count), seed=55)
        pool.update(aimed_writes(rng, k, count, patterns, pattern_of), what="8192 stripes")
        some = [int(b) for b in rng.permutation(count)[:3000]]
        pool.update([b * k + int(rng.integers(k)) for b in some], what="3000 stripes")
        pool.check_all()


# ---- 4. other code families, once each ----
@pytest.mark.parametrize("n,k,S,flags,order", [(32, 8, 32, 0, 0), (72, 48, 64, MIXED_RADIX, 48)], ids=["32_8", "72_48_mixed"])
def test_code_families(torch_cuda, fe, oracle, n, k, S, flags, order):
    count = n + 3
    patterns = [codeword_block(k, u) for u in range(n)]
    pattern_of = rotated(n, count, down=1)
    rng = np.random.default_rng(n)
    with fe.Encoder(n, k, 4 * S, flags=flags) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        pool = Degraded(torch_cuda, fe, enc, Codec(oracle, n, k, flags, order), S, count, patterns, pattern_of, range(count), seed=n)
        pool.update(aimed_writes(rng, k, count, patterns, pattern_of))
        pool.check_all()


# ---- 5. whole stripes ----
def test_whole_stripes_equal_update_batch(torch_cuda, fe, oracle):
    torch = torch_cuda
    n, k, S, count = 20, 16, 65, 9
    patterns = [([], []), ([1], [2])]           # pattern 0 loses nothing
    pattern_of = [NONE, 0, NONE, 0, 5, 99, 0, NONE, 1 << 20]   # entries >= n_patterns on stripes 4, 5 and 8: not touched, so not looked at
    live = [0, 1, 2, 3, 6, 7]
    rng = np.random.default_rng(6)
    writes = random_writes(rng, k, live, 30)
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        pool = Degraded(torch, fe, enc, Codec(oracle, n, k), S, count, patterns, pattern_of, live, seed=66)
        cd, cp = pool.dd.clone(), pool.dp.clone()
        new = pool.new_rows(writes)
        pool.update(writes, new)
        enc.update_batch(cd, cp, count, writes, to_dev(torch, new))
        torch.cuda.synchronize()
        assert torch.equal(cd, pool.dd) and torch.equal(cp, pool.dp)


# ---- 6. the parity form ----
@pytest.mark.parametrize("with_old", [True, False])
@pytest.mark.parametrize("which", ["aimed", "random"])
def test_parity_form(torch_cuda, fe, oracle, which, with_old):
    torch = torch_cuda
    n, k, S, count = 20, 16, 65, 41
    patterns = [codeword_block(k, u) for u in range(n)]
    pattern_of = rotated(n, count)
    rng = np.random.default_rng(7)
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        if which == "aimed":
            live, writes = range(count), aimed_writes(rng, k, count, patterns, pattern_of)
        else:
            writes = random_writes(rng, k, range(count), 60)
            live = sorted({w // k for w in writes})
        pool = Degraded(torch, fe, enc, Codec(oracle, n, k), S, count, patterns, pattern_of, live, seed=77)
        pool.absent_d[:] = False    # the data lives elsewhere (the truth X): only the parity flags of a pattern matter
        rows = pool.X.reshape(count * k, S)
        new, old = pool.new_rows(writes), rows[writes].copy()
        dn, do = to_dev(torch, new), to_dev(torch, old)
        enc.update_parity_batch_set(pool.dp, count, pool.po, writes, dn, old=do if with_old else None)
        # old rows given: the blocks become `new`; from zero: the parity moves as if `new` had been ADDED to them (the code is linear)
        rows[writes] = new if with_old else ((old.astype(np.uint64) + new) % P).astype(np.uint32)
        pool._expect_touched(writes, data=False)
        torch.cuda.synchronize()
        got_p = host(pool.dp).reshape(pool.img_p.shape)
        bad = (got_p != pool.img_p).any(axis=2)
        assert not bad.any(), "wrong parity blocks (stripe, block), first ones %r" % np.argwhere(bad)[:8].tolist()
        assert np.array_equal(host(dn).reshape(new.shape), new) and np.array_equal(host(do).reshape(old.shape), old)


# ---- 8. back-to-back calls ----
def test_back_to_back_calls_reuse_the_staged_lists(torch_cuda, fe, oracle):
    """Two calls with different lists of different lengths on one non-default stream, no synchronise between them (the second rewrites blocks
    the first wrote, absent ones among them, so its reconstruction must see the first call's parity), then one on a second stream over other
    stripes; the host list is overwritten as soon as a call returns."""
    torch = torch_cuda
    n, k, S, count = 20, 16, 65, 41
    patterns = [codeword_block(k, u) for u in range(n)]
    pattern_of = rotated(n, count)
    rng = np.random.default_rng(8)
    first = aimed_writes(rng, k, count, patterns, pattern_of, range(0, 30))
    second = aimed_writes(rng, k, count, patterns, pattern_of, range(0, 30, 2)) + random_writes(rng, k, range(5, 25), 45)
    second = sorted(set(second))
    third = aimed_writes(rng, k, count, patterns, pattern_of, range(30, count)) + [30 * k + 1, 30 * k + 2]
    third = sorted(set(third))
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        pool = Degraded(torch, fe, enc, Codec(oracle, n, k), S, count, patterns, pattern_of, range(count), seed=88)
        calls = [(w, pool.new_rows(w)) for w in (first, second, third)]
        news = [to_dev(torch, new) for _, new in calls]
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        for (w, _), dn, st in zip(calls, news, (s1, s1, s2)):
            arr = np.array(w, dtype=np.uint64)
            enc.update_batch_set(pool.dd, pool.dp, count, pool.po, arr, dn, stream=st.cuda_stream)
            arr[:] = 0xFFFFFFFFFFFFFFFF  # the list may be reused as soon as the call returns
        torch.cuda.synchronize()
        for w, new in calls:
            pool.expect(w, new)
        pool.check_image()
        pool.check_all()


# ---- 9. refusals on a live context ----
def test_refusals_leave_the_pool_unchanged(torch_cuda, fe, oracle):
    torch = torch_cuda
    n, k, S, count = 20, 16, 16, 6
    m = n - k
    patterns = [([2], []), ([], [1])]
    pattern_of = [0, 1, NONE, 0, 1, 0]
    rng = np.random.default_rng(9)
    lib = fe.lib()
    with fe.Encoder(n, k, 4 * S) as enc:
        pool = Degraded(torch, fe, enc, Codec(oracle, n, k), S, count, patterns, pattern_of, range(count), seed=99)
        new = to_dev(torch, rand_words(rng, (4, S)))
        n0 = new.clone()

        def refused(code, writes, po=None, rows=None, parity_form=True):
            rows = new if rows is None else rows
            po = pool.po if po is None else po
            with pytest.raises(fe.FastEccError) as ei:
                enc.update_batch_set(pool.dd, pool.dp, count, po, writes, rows)
            assert ei.value.code == code
            if parity_form:
                for old in (None, new):
                    with pytest.raises(fe.FastEccError) as ei:
                        enc.update_parity_batch_set(pool.dp, count, po, writes, rows, old=old)
                    assert ei.value.code == code
            pool.check_image("after a refusal")
            assert torch.equal(new, n0)

        refused(fe.E_INVAL, [1, 2])                                   # no set prepared
        refused(fe.E_INVAL, [])                                       # ... with nothing to write, too
        enc.decode_prepare_set(*flag_rows(k, m, patterns))
        refused(fe.E_INVAL, [1, count * k])                           # an index >= count * k
        refused(fe.E_INVAL, [3, 40, 3])                               # a duplicate
        bad = pool.pattern_of.copy()
        bad[3] = 2
        refused(fe.E_INVAL, [1, 3 * k + 4], po=bad)                   # a touched stripe's entry >= n_patterns
        refused(fe.E_INVAL, [1, 2], rows=pool.dd[5 * S:], parity_form=False)  # new_blocks inside the data pool (the parity form has none)
        refused(fe.E_INVAL, [1, 2], rows=pool.dp[count * m * S - S:])  # ... reaching into the parity pool's last block
        with pytest.raises(fe.FastEccError) as ei:                    # old_blocks inside the parity pool
            enc.update_parity_batch_set(pool.dp, count, pool.po, [1, 2], new, old=pool.dp[S:])
        assert ei.value.code == fe.E_INVAL
        pool.check_image("after a refusal")
        assert lib.fastecc_update_batch_set(enc._h, pool.dd.data_ptr(), pool.dp.data_ptr(), count, None, (ctypes.c_uint64 * 1)(1), 1, new.data_ptr(),
                                            None) == fe.E_INVAL       # a null pattern_of
        pool.check_image("after a refusal")
        with fe.Encoder(64, 32, 4 * S, field=fe.FIELD_GF_P61_SQUARED) as e61:
            for call in (lambda: e61.update_batch_set(pool.dd, pool.dp, 1, [NONE], [1], new),
                         lambda: e61.update_parity_batch_set(pool.dp, 1, [NONE], [1], new)):
                with pytest.raises(fe.FastEccError) as ei:
                    call()
                assert ei.value.code == fe.E_UNSUPPORTED              # the 64-bit field
        pool.check_image("after a refusal")
        # after the refusals a valid call still gives the right pool; an entry >= n_patterns on an untouched stripe is accepted
        writes = [2, 5, k + 2, 2 * k, 5 * k + 2, 4 * k + 7]
        new6 = rand_words(rng, (len(writes), S))
        enc.update_batch_set(pool.dd, pool.dp, count, bad, writes, to_dev(torch, new6))
        pool.expect(writes, new6)
        pool.check_image("a valid call after the refusals")
        pool.check_all()


def test_no_writes_is_a_no_op(torch_cuda, fe, oracle):
    n, k, S, count = 20, 16, 16, 3
    patterns = [([2], [0])]
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        pool = Degraded(torch_cuda, fe, enc, Codec(oracle, n, k), S, count, patterns, [0, 0, NONE], range(count), seed=10)
        enc.update_batch_set(pool.dd, pool.dp, count, pool.po, [], pool.dd[:0])
        enc.update_parity_batch_set(pool.dp, count, pool.po, [], pool.dd[:0])
        pool.check_image("no writes")
