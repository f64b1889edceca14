"""GPU tests (-m gpu) of the scrub of degraded pools with absent blocks PER STRIPE: fastecc_scrub_erasures_set names a set of patterns,
fastecc_verify_batch_set and fastecc_correct_batch_set treat stripe b under pattern pattern_of[b] (rotated placement with a device down).

The expected answers come from the corruption the tests inject themselves, from the original codewords (the library's encoder, pinned to
the reference by the other suites) and from the per-stripe loop of the calls that existed before: fastecc_scrub_erasures(pattern) +
fastecc_verify / fastecc_correct on the stripe alone.  Absent blocks and FASTECC_PATTERN_NONE stripes are filled with random words, words
>= p included: they must never be read.  Every comparison is bit-exact."""
import ctypes
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 0xFFF00001
SEED = 0x5E75


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def fe(hip_lib):
    import fastecc_amd
    return fastecc_amd


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to("cuda:0")


def host(t):
    return t.cpu().numpy().view(np.uint32).copy()


def presence(n, k, absent):
    dp, pp = np.ones(k, np.uint8), np.ones(n - k, np.uint8)
    for j in absent:
        if j < k:
            dp[j] = 0
        else:
            pp[j - k] = 0
    return dp, pp


def flag_rows(n, k, patterns):
    """the two arrays of fastecc_scrub_erasures_set / fastecc_decode_prepare_set: one row of flags per pattern (a list of absent blocks)"""
    rows = [presence(n, k, a) for a in patterns]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def pick_absent(rng, n, k, w, avoid=()):
    """w distinct blocks, sorted, outside `avoid`, spread over data and parity when w >= 2."""
    free_d = [j for j in range(k) if j not in avoid]
    free_p = [j for j in range(k, n) if j not in avoid]
    if w >= 2 and free_d and free_p:
        first = [int(rng.choice(free_d)), int(rng.choice(free_p))]
        rest = [j for j in free_d + free_p if j not in first]
        return sorted(first + [int(x) for x in rng.choice(rest, size=w - 2, replace=False)])
    return sorted(int(x) for x in rng.choice(free_d + free_p, size=w, replace=False))


def garbage(row, rng):
    row[:] = rng.integers(0, 1 << 32, size=row.shape[0], dtype=np.uint64).astype(np.uint32)
    row[0] = np.uint32(P + int(rng.integers(0, (1 << 32) - P)))


def one_word(row, rng):
    w = int(rng.integers(row.shape[0]))
    row[w] = np.uint32((int(row[w]) + 1 + int(rng.integers(P - 1))) % P)


class Pool:
    """`count` stripes back to back: host copies d (count, k, S), p (count, n - k, S) of the clean codewords, device buffers D, Q
    (offset_words = 1: their base addresses miss 16-byte alignment)."""

    def __init__(self, torch, enc, count, S, rng, offset_words=0):
        n, k = enc.n, enc.k
        self.torch, self.enc, self.count, self.S, self.n, self.k = torch, enc, count, S, n, k
        self.d = rng.integers(0, P, size=(count, k, S), dtype=np.uint64).astype(np.uint32)
        self.D = torch.zeros(offset_words + count * k * S, dtype=torch.int32, device="cuda:0")[offset_words:]
        self.Q = torch.zeros(offset_words + count * (n - k) * S, dtype=torch.int32, device="cuda:0")[offset_words:]
        assert self.D.data_ptr() % 16 == 4 * offset_words and self.Q.data_ptr() % 16 == 4 * offset_words
        self.D.copy_(to_dev(torch, self.d.reshape(-1)))
        for b in range(count):
            enc.encode(*self.stripe(b))
        torch.cuda.synchronize()
        self.p = host(self.Q).reshape(count, n - k, S)

    def stripe(self, b, D=None, Q=None):
        dw, pw = self.k * self.S, (self.n - self.k) * self.S
        D, Q = (self.D, self.Q) if D is None else (D, Q)
        return D[b * dw:(b + 1) * dw], Q[b * pw:(b + 1) * pw]

    def upload(self, d, p):
        self.D.copy_(to_dev(self.torch, d.reshape(-1)))
        self.Q.copy_(to_dev(self.torch, p.reshape(-1)))
        self.torch.cuda.synchronize()

    def contents(self, D=None, Q=None):
        D, Q = (self.D, self.Q) if D is None else (D, Q)
        return host(D).reshape(self.d.shape), host(Q).reshape(self.p.shape)

    def block(self, d, p, b, j):
        return d[b, j] if j < self.k else p[b, j - self.k]

    def degraded(self, fe, patterns, pattern_of, rng):
        """Copies of the clean pool with garbage (word 0 >= p) in every stripe's absent blocks and in all of a FASTECC_PATTERN_NONE stripe."""
        d, p = self.d.copy(), self.p.copy()
        for b, q in enumerate(pattern_of):
            for j in (range(self.n) if q == fe.PATTERN_NONE else patterns[q]):
                garbage(self.block(d, p, b, j), rng)
        return d, p

    def verify_loop(self, fe, patterns, pattern_of, seed):
        """the per-stripe route: fastecc_scrub_erasures(the stripe's pattern) + fastecc_verify; a FASTECC_PATTERN_NONE stripe is consistent"""
        out = []
        for b, q in enumerate(pattern_of):
            if q == fe.PATTERN_NONE:
                out.append(True)
                continue
            self.enc.scrub_erasures(*presence(self.n, self.k, patterns[q]))
            out.append(self.enc.verify(*self.stripe(b), seed=seed))
        self.enc.scrub_erasures()
        return np.array(out)


def raw_set_call(fe, name, enc, D, Q, count, pattern_of, seed, fill=7):
    """the C entry point itself: (return code, the count bytes of consistent / status, *inconsistent), both outputs preset to sentinels"""
    out = np.full(count, fill, np.uint8)
    bad = ctypes.c_uint64(0xABCD)
    po = np.ascontiguousarray(pattern_of, dtype=np.uint32)
    code = getattr(fe.lib(), name)(enc._h, D.data_ptr(), Q.data_ptr(), count, po.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), None, seed,
                                   out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(bad))
    return code, out, int(bad.value)


def uncorrectable(fe, call, *args, **kw):
    with pytest.raises(fe.FastEccError) as ei:
        call(*args, **kw)
    assert ei.value.code == fe.E_UNCORRECTABLE
    return ei.value


def test_rotated_pool(torch_cuda, fe):
    """One device of a rotated pool down: stripe b lacks block b mod n.  More than 2n stripes with a ragged tail, chunks of 8, so the
    patterns mix inside every chunk."""
    torch, rng = torch_cuda, _rng("rotated")
    n, k, S, count = 20, 16, 16, 45
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.set_option("scrub_batch_chunk", 8)
        pool = Pool(torch, enc, count, S, rng)
        patterns = [[q] for q in range(n)]
        po = np.arange(count, dtype=np.uint32) % n
        enc.scrub_erasures_set(*flag_rows(n, k, patterns))
        d, p = pool.degraded(fe, patterns, po, rng)
        pool.upload(d, p)
        assert enc.verify_batch_set(pool.D, pool.Q, count, po, seed=SEED).all()
        corrupted = [3, 8, 21, 40, 44]
        for b in corrupted:
            one_word(pool.block(d, p, b, int(rng.choice([j for j in range(n) if j != b % n]))), rng)
        pool.upload(d, p)
        for seed in (SEED, SEED + 1):
            got = enc.verify_batch_set(pool.D, pool.Q, count, po, seed=seed)
            assert np.array_equal(got, pool.verify_loop(fe, patterns, po, seed))
            assert np.nonzero(~got)[0].tolist() == corrupted
        hd, hq = pool.contents()
        assert np.array_equal(hd, d) and np.array_equal(hq, p)  # reads only
        # negative control: stripe 10's garbage sits in block 11, not in the block 10 its pattern names — with a word >= p and without one
        for big in (True, False):
            d, p = pool.degraded(fe, patterns, po, rng)
            pool.block(d, p, 10, 10)[:] = pool.block(pool.d, pool.p, 10, 10)
            garbage(pool.block(d, p, 10, 11), rng)
            if not big:
                pool.block(d, p, 10, 11)[:] %= np.uint32(P)
            pool.upload(d, p)
            code, out, bad = raw_set_call(fe, "fastecc_verify_batch_set", enc, pool.D, pool.Q, count, po, SEED)
            assert code == fe.OK and out.tolist() == [int(b != 10) for b in range(count)] and bad == 1


def test_different_w_in_one_chunk(torch_cuda, fe):
    """Patterns with 0, 1, 3 and n - k absent blocks and FASTECC_PATTERN_NONE stripes in one chunk: every stripe is checked from its own
    pattern's first coefficient on (a chunk-wide bound is wrong in one direction or the other)."""
    torch, rng = torch_cuda, _rng("w")
    n, k, S = 32, 16, 64
    m, NONE = n - k, fe.PATTERN_NONE
    with fe.Encoder(n, k, 4 * S) as enc:
        patterns = [[], pick_absent(rng, n, k, 1), pick_absent(rng, n, k, 3), pick_absent(rng, n, k, m)]
        po = np.array([0, 1, 2, 3, NONE, 0, 1, 2, 3, NONE, 2, 1, 3, 0], dtype=np.uint32)
        count = len(po)
        pool = Pool(torch, enc, count, S, rng)
        enc.scrub_erasures_set(*flag_rows(n, k, patterns))
        d, p = pool.degraded(fe, patterns, po, rng)
        pool.upload(d, p)
        code, out, bad = raw_set_call(fe, "fastecc_verify_batch_set", enc, pool.D, pool.Q, count, po, SEED)
        assert code == fe.OK and out.all() and bad == 0  # clean w = 0, 1, 3, 16 stripes and the garbage-only stripes

        def present(b):
            return int(rng.choice([j for j in range(n) if j not in patterns[po[b]]]))
        one_word(pool.block(d, p, 5, present(5)), rng)        # w = 0
        one_word(pool.block(d, p, 7, present(7)), rng)        # w = 3
        one_word(pool.block(d, p, 3, present(3)), rng)        # w = 16, a changed word < p: nothing can be checked
        pool.block(d, p, 8, present(8))[9] = np.uint32(P + 3)  # w = 16, a word >= p in a present block
        pool.upload(d, p)
        for seed in (SEED, SEED + 1):
            code, out, bad = raw_set_call(fe, "fastecc_verify_batch_set", enc, pool.D, pool.Q, count, po, seed)
            assert code == fe.OK
            assert np.nonzero(out == 0)[0].tolist() == [5, 7, 8] and set(out.tolist()) <= {0, 1}
            assert bad == 3  # the FASTECC_PATTERN_NONE stripes are not counted
            assert np.array_equal(out.astype(bool), pool.verify_loop(fe, patterns, po, seed))
        hd, hq = pool.contents()
        assert np.array_equal(hd, d) and np.array_equal(hq, p)


@pytest.mark.parametrize("n,k,S", [(8, 4, 32), (72, 64, 33), (64, 16, 16), (64, 8, 32), (130, 100, 16), (1100, 1000, 8)])
def test_code_families(torch_cuda, fe, n, k, S):
    """(2k,k), an odd block length (the kernel without vector loads), fixed erasures, n = 4k / 8k, zero-extended codes: the per-stripe loop's
    answer; once more from base addresses that miss 16-byte alignment (the kernel without vector loads on a vectorisable length)."""
    torch, m = torch_cuda, n - k
    for offset in ((0, 1) if S % 4 == 0 else (0,)):
        rng = _rng("families", n, k, S, offset)
        with fe.Encoder(n, k, 4 * S) as enc:
            patterns = [pick_absent(rng, n, k, 1), pick_absent(rng, n, k, 2), pick_absent(rng, n, k, min(3, m))]
            po = np.array([0, 1, 2, 2, 1, 0, 1], dtype=np.uint32)
            count = len(po)
            pool = Pool(torch, enc, count, S, rng, offset_words=offset)
            enc.scrub_erasures_set(*flag_rows(n, k, patterns))
            d, p = pool.degraded(fe, patterns, po, rng)
            pool.upload(d, p)
            assert enc.verify_batch_set(pool.D, pool.Q, count, po, seed=SEED).all()
            for b in (1, 4):
                one_word(pool.block(d, p, b, int(rng.choice([j for j in range(n) if j not in patterns[po[b]]]))), rng)
            pool.upload(d, p)
            got = enc.verify_batch_set(pool.D, pool.Q, count, po, seed=SEED)
            assert np.array_equal(got, pool.verify_loop(fe, patterns, po, SEED))
            assert np.nonzero(~got)[0].tolist() == [1, 4]


def test_stale_state_and_independence(torch_cuda, fe):
    """One context through: verify_batch with no pattern, set A, a disjoint set B, the single pattern changed in between, a refused set,
    the set cleared.  No answer may depend on what an earlier call, set or pattern left behind."""
    torch, rng = torch_cuda, _rng("stale")
    n, k, S, count = 32, 16, 64, 11
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.set_option("scrub_batch_chunk", 8)
        pool = Pool(torch, enc, count, S, rng)
        blocks = [int(x) for x in rng.permutation(n)]
        A = [sorted(blocks[0:2]), sorted(blocks[2:4]), sorted(blocks[4:6])]
        B = [sorted(blocks[6:8]), sorted(blocks[8:10]), sorted(blocks[10:12])]
        C = [blocks[12]]
        po = np.arange(count, dtype=np.uint32) % 3
        in_a, in_b = pool.degraded(fe, A, po, rng), pool.degraded(fe, B, po, rng)
        in_c = pool.degraded(fe, [C], np.zeros(count, np.uint32), rng)
        for g in (in_a, in_b, in_c):  # garbage without a word >= p: only the syndromes can tell
            g[0][:] %= np.uint32(P)
            g[1][:] %= np.uint32(P)

        def answers(stripes, call, *args):
            pool.upload(*stripes)
            return call(pool.D, pool.Q, count, *args, seed=SEED).tolist()
        yes, no = [True] * count, [False] * count
        # 1. no pattern, one corrupted stripe: every position of the batch's fingerprint stripe gets written
        d, p = pool.d.copy(), pool.p.copy()
        one_word(pool.block(d, p, 5, 2), rng)
        assert answers((d, p), enc.verify_batch) == [b != 5 for b in range(count)]
        # 2. set A
        enc.scrub_erasures_set(*flag_rows(n, k, A))
        assert answers(in_a, enc.verify_batch_set, po) == yes
        assert answers(in_b, enc.verify_batch_set, po) == no
        assert answers(in_a, enc.verify_batch) == no  # the single pattern (none) does not see the set
        # 3. a disjoint set B
        enc.scrub_erasures_set(*flag_rows(n, k, B))
        assert answers(in_b, enc.verify_batch_set, po) == yes
        assert answers(in_a, enc.verify_batch_set, po) == no
        assert answers((pool.d, pool.p), enc.verify_batch_set, po) == yes
        # 4. the single pattern set to something else in between: each call answers with its own state
        enc.scrub_erasures(*presence(n, k, C))
        assert answers(in_b, enc.verify_batch_set, po) == yes
        assert answers(in_b, enc.verify_batch) == no
        assert answers(in_c, enc.verify_batch) == yes
        assert answers(in_c, enc.verify_batch_set, po) == no
        assert answers(in_b, enc.verify_batch_set, po) == yes
        # 5. n - k + 1 absent blocks in one pattern: refused, set B stays in force
        with pytest.raises(fe.FastEccError) as ei:
            enc.scrub_erasures_set(*flag_rows(n, k, [A[0], sorted(blocks[:n - k + 1])]))
        assert ei.value.code == fe.E_INVAL
        assert answers(in_b, enc.verify_batch_set, po) == yes
        assert answers(in_a, enc.verify_batch_set, po) == no
        # 6. cleared: no set to answer with, while verify_batch still answers with the single pattern
        enc.scrub_erasures_set([], [])
        with pytest.raises(fe.FastEccError) as ei:
            enc.verify_batch_set(pool.D, pool.Q, count, po, seed=SEED)
        assert ei.value.code == fe.E_INVAL
        assert answers(in_c, enc.verify_batch) == yes
        assert answers(in_b, enc.verify_batch) == no


@pytest.mark.parametrize("n,k,S,count", [(20, 16, 16, 27), (32, 16, 64, 37)])
def test_correct(torch_cuda, fe, n, k, S, count):
    torch, rng, m = torch_cuda, _rng("correct", n, k, S), n - k
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.set_option("scrub_batch_chunk", 8)
        enc.set_option("locate_max", 1)
        pool = Pool(torch, enc, count, S, rng)
        patterns = [[q] for q in range(n)]
        po = np.arange(count, dtype=np.uint32) % n
        dp, pp = flag_rows(n, k, patterns)
        enc.decode_prepare_set(dp, pp)  # before correct_batch_set: it must still work afterwards
        enc.scrub_erasures_set(dp, pp)
        d, p = pool.degraded(fe, patterns, po, rng)
        # t = 2 > locate_max = 1, and t + locate_max = 3 < n - k - w + 1 (the distance left), so no codeword is within reach
        assert 3 < m - 1 + 1
        fixable, big_stripe, hopeless = [1, 8, 15, count - 1], 11, 9

        def present(b, size=1):
            return [int(j) for j in rng.choice([j for j in range(n) if j != b % n], size=size, replace=False)]
        for b in fixable:
            one_word(pool.block(d, p, b, present(b)[0]), rng)
        pool.block(d, p, big_stripe, present(big_stripe)[0])[3] = np.uint32(P + 7)
        for j in present(hopeless, 2):
            one_word(pool.block(d, p, hopeless, j), rng)
        pool.upload(d, p)
        want = np.zeros(count, np.uint8)
        want[fixable + [big_stripe]] = 1
        want[hopeless] = 2
        # the per-stripe loop on a clone: fastecc_scrub_erasures(pattern) + fastecc_correct
        D2, Q2 = pool.D.clone(), pool.Q.clone()
        loop = np.zeros(count, np.uint8)
        for b in range(count):
            enc.scrub_erasures(*presence(n, k, patterns[po[b]]))
            try:
                loop[b] = 1 if enc.correct(*pool.stripe(b, D2, Q2), seed=SEED) else 0
            except fe.FastEccError as e:
                assert e.code == fe.E_UNCORRECTABLE
                loop[b] = 2
        enc.scrub_erasures()
        torch.cuda.synchronize()
        assert np.array_equal(loop, want)
        code, status, bad = raw_set_call(fe, "fastecc_correct_batch_set", enc, pool.D, pool.Q, count, po, SEED)
        torch.cuda.synchronize()
        assert code == fe.E_UNCORRECTABLE and np.array_equal(status, want) and bad == len(fixable) + 2
        assert torch.equal(pool.D, D2) and torch.equal(pool.Q, Q2)  # the pool's bytes of the loop
        hd, hq = pool.contents()
        for b in range(count):
            if want[b] == 1:  # the original codeword in every block, the absent one included
                assert np.array_equal(hd[b], pool.d[b]) and np.array_equal(hq[b], pool.p[b]), b
            else:             # untouched: consistent (garbage and all) or uncorrectable
                assert np.array_equal(hd[b], d[b]) and np.array_equal(hq[b], p[b]), b
        # the Python method: the same status on its error, nothing left to correct but the stripe out of reach
        err = uncorrectable(fe, enc.correct_batch_set, pool.D, pool.Q, count, po, seed=SEED)
        assert err.status.tolist() == [2 if b == hopeless else 0 for b in range(count)]
        # the workflow's second step: the decode pattern set prepared before brings back the absent blocks of all the others
        enc.repair_batch_set(pool.D, pool.Q, count, po)
        torch.cuda.synchronize()
        hd, hq = pool.contents()
        keep = [b for b in range(count) if b != hopeless]
        assert np.array_equal(hd[keep], pool.d[keep]) and np.array_equal(hq[keep], pool.p[keep])
        nothing = np.full(count, fe.PATTERN_NONE, np.uint32)
        assert enc.correct_batch_set(pool.D, pool.Q, count, np.where(np.arange(count) == hopeless, nothing, po), seed=SEED).tolist() == [0] * count


def test_refused_contexts(torch_cuda, fe):
    torch = torch_cuda
    for make in (lambda: fe.Encoder(64, 32, 64, field=fe.FIELD_GF_P61_SQUARED), lambda: fe.ShardedEncoder(64, 32, 256, [0, 0]),
                 lambda: fe.Encoder(2 * 48, 48, 64, flags=fe.CODE_MIXED_RADIX)):
        with make() as enc:
            n, k = enc.n, enc.k
            buf = torch.zeros(2 * n * enc.block_bytes // 4, dtype=torch.int32, device="cuda:0")
            po = np.zeros(2, np.uint32)
            for call in (lambda: enc.scrub_erasures_set(*flag_rows(n, k, [[1], [k]])), lambda: enc.scrub_erasures_set([], []),
                         lambda: enc.verify_batch_set(buf, buf, 2, po), lambda: enc.correct_batch_set(buf, buf, 2, po)):
                with pytest.raises(fe.FastEccError) as ei:
                    call()
                assert ei.value.code == fe.E_UNSUPPORTED


def test_refused_arguments(torch_cuda, fe):
    torch, rng = torch_cuda, _rng("refused")
    n, k, S, count = 8, 4, 32, 5
    with fe.Encoder(n, k, 4 * S) as enc:
        pool = Pool(torch, enc, count, S, rng)
        patterns = [[0], [5], [2, 7]]
        d, p = pool.degraded(fe, patterns, [0, 1, 2, 0, 1], rng)
        one_word(pool.block(d, p, 3, 1), rng)
        pool.upload(d, p)
        for name in ("fastecc_verify_batch_set", "fastecc_correct_batch_set"):  # no set prepared
            code, out, bad = raw_set_call(fe, name, enc, pool.D, pool.Q, count, [0, 1, 2, 0, 1], SEED)
            assert code == fe.E_INVAL and out.tolist() == [7] * count and bad == 0xABCD
        enc.scrub_erasures_set(*flag_rows(n, k, patterns))
        for name in ("fastecc_verify_batch_set", "fastecc_correct_batch_set"):
            for po in ([0, 1, 3, 0, 1], [0, 1, 2, 0, fe.PATTERN_NONE - 1]):  # an entry >= P that is not FASTECC_PATTERN_NONE
                code, out, bad = raw_set_call(fe, name, enc, pool.D, pool.Q, count, po, SEED)
                assert code == fe.E_INVAL and out.tolist() == [7] * count and bad == 0xABCD
        hd, hq = pool.contents()
        assert np.array_equal(hd, d) and np.array_equal(hq, p)
        assert enc.verify_batch_set(pool.D, pool.Q, count, [0, 1, 2, 0, 1], seed=SEED).tolist() == [True, True, True, False, True]
        with pytest.raises(fe.FastEccError) as ei:  # more than 4096 patterns
            enc.scrub_erasures_set(np.ones((4097, k), np.uint8), np.ones((4097, n - k), np.uint8))
        assert ei.value.code == fe.E_INVAL
        assert enc.verify_batch_set(pool.D, pool.Q, count, [0, 1, 2, 0, 1], seed=SEED).tolist() == [True, True, True, False, True]
    # P * NC > 2^24: (8192,4096) has NC = 8192, so P = 4096 patterns are one table too many
    with fe.Encoder(8192, 4096, 4) as enc:
        with pytest.raises(fe.FastEccError) as ei:
            enc.scrub_erasures_set(np.ones((4096, 4096), np.uint8), np.ones((4096, 4096), np.uint8))
        assert ei.value.code == fe.E_UNSUPPORTED
        enc.scrub_erasures_set(np.ones((2048, 4096), np.uint8), np.ones((2048, 4096), np.uint8))  # 2^24 exactly
