"""GPU tests (-m gpu) of the scrub of degraded stripes: fastecc_scrub_erasures names the absent blocks, and fastecc_verify,
fastecc_locate_errors, fastecc_correct, fastecc_verify_batch and fastecc_correct_batch work around them.

The expected answers come from the corruption the tests inject themselves and from the original codeword, which the library's encoder
produces (the encoder is pinned to the reference by the other suites).  Absent blocks are filled with random words, words >= p
included: they must never be read.  Every comparison is bit-exact."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 0xFFF00001
SEED = 0x5EED

# the small codes of tests/test_gpu_scrub.py: (2k,k), n = k + N/2^d, an odd block length, 4k / 8k, zero-extended; NC from 4 to 2048
CODES = [(4, 2, 64), (8, 4, 32), (32, 16, 64), (64 + 16, 64, 32), (64 + 8, 64, 33), (4 * 16, 16, 16), (8 * 8, 8, 32), (130, 100, 16), (1100, 1000, 8)]


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


def codeword(torch, enc, S, rng):
    """(data, parity) of a random codeword on the device, every word < p."""
    n, k = enc.n, enc.k
    data = to_dev(torch, rng.integers(0, P, size=k * S, dtype=np.uint64))
    parity = torch.zeros((n - k) * S, dtype=torch.int32, device="cuda:0")
    enc.encode(data, parity)
    torch.cuda.synchronize()
    return data, parity


def pick_absent(rng, n, k, w, avoid=()):
    """w distinct blocks, sorted, outside `avoid`, spread over data and parity when w >= 2."""
    free_d = [j for j in range(k) if j not in avoid]
    free_p = [j for j in range(k, n) if j not in avoid]
    if w >= 2 and free_d and free_p:
        first = [int(rng.choice(free_d)), int(rng.choice(free_p))]
        rest = [j for j in free_d + free_p if j not in first]
        return sorted(first + [int(x) for x in rng.choice(rest, size=w - 2, replace=False)])
    return sorted(int(x) for x in rng.choice(free_d + free_p, size=w, replace=False))


def presence(n, k, absent):
    dp, pp = np.ones(k, np.uint8), np.ones(n - k, np.uint8)
    for j in absent:
        if j < k:
            dp[j] = 0
        else:
            pp[j - k] = 0
    return dp, pp


def set_pattern(enc, absent):
    enc.scrub_erasures(*presence(enc.n, enc.k, absent))


def edit(torch, data, parity, k, S, blocks, kind, rng):
    """Change the given codeword blocks in place (numpy round trip of the whole stripe).  garbage: random 32-bit words, word 0 >= p;
    one_word / random: a different block with every word < p; bitflip: one flipped bit (may leave [0, p)); big: one word >= p."""
    d, p = host(data).reshape(k, S), host(parity).reshape(-1, S)
    for j in blocks:
        row = d[j] if j < k else p[j - k]
        w = int(rng.integers(S))
        if kind == "garbage":
            row[:] = rng.integers(0, 1 << 32, size=S, dtype=np.uint64).astype(np.uint32)
            row[0] = np.uint32(P + int(rng.integers(0, (1 << 32) - P)))
        elif kind == "one_word":
            row[w] = np.uint32((int(row[w]) + 1 + int(rng.integers(P - 1))) % P)
        elif kind == "random":
            new = rng.integers(0, P, size=S, dtype=np.uint64).astype(np.uint32)
            new[0] = np.uint32((int(row[0]) + 1) % P)  # certainly different
            row[:] = new
        elif kind == "bitflip":
            bit = int(rng.integers(32)) if row[w] < (1 << 31) else int(rng.integers(20))
            row[w] ^= np.uint32(1 << bit)
        elif kind == "big":
            row[w] = np.uint32(P + int(rng.integers(0, (1 << 32) - P)))
        else:
            raise ValueError(kind)
    data.copy_(to_dev(torch, d.reshape(-1)))
    parity.copy_(to_dev(torch, p.reshape(-1)))
    torch.cuda.synchronize()


def uncorrectable(fe, call, *args, **kw):
    with pytest.raises(fe.FastEccError) as ei:
        call(*args, **kw)
    assert ei.value.code == fe.E_UNCORRECTABLE
    return ei.value


@pytest.mark.parametrize("n,k,S", CODES)
def test_clean_but_degraded(torch_cuda, fe, n, k, S):
    torch, rng, m = torch_cuda, _rng("clean", n, k, S), n - k
    with fe.Encoder(n, k, 4 * S) as enc:
        data, parity = codeword(torch, enc, S, rng)
        d0, p0 = data.clone(), parity.clone()
        for w in sorted({1, m // 2, m - 1, m} - {0}):
            data.copy_(d0)
            parity.copy_(p0)
            absent = pick_absent(rng, n, k, w)
            edit(torch, data, parity, k, S, absent, "garbage", rng)
            dg, pg = data.clone(), parity.clone()
            set_pattern(enc, absent)
            assert enc.verify(data, parity, seed=SEED), (w, absent)
            assert enc.locate_errors(data, parity, seed=SEED + 1) == []
            assert enc.correct(data, parity, seed=SEED + 2) == []
            torch.cuda.synchronize()
            assert torch.equal(dg, data) and torch.equal(pg, parity)  # untouched, the garbage included
            enc.scrub_erasures()  # cleared: the old behaviour
            assert not enc.verify(data, parity, seed=SEED)


def _budgets(m, tmax):
    """(t, w) with t >= 1, w >= 1: the equality 2t + w = n - k and a pattern half that size."""
    out = set()
    for t in (1, 2, tmax):
        for w in (m - 2 * t, (m - 2 * t) // 2):
            if w >= 1:
                out.add((t, w))
    return sorted(out)


@pytest.mark.parametrize("kind", ["one_word", "random", "bitflip"])
@pytest.mark.parametrize("n,k,S", [c for c in CODES if c[0] - c[1] >= 3])
def test_errors_plus_erasures(torch_cuda, fe, n, k, S, kind):
    torch, rng, m, tmax = torch_cuda, _rng("errors", n, k, S, kind), n - k, 4
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.set_option("locate_max", tmax)
        data, parity = codeword(torch, enc, S, rng)
        d0, p0 = data.clone(), parity.clone()
        for t, w in _budgets(m, tmax):
            data.copy_(d0)
            parity.copy_(p0)
            absent = pick_absent(rng, n, k, w)
            wrong = pick_absent(rng, n, k, t, avoid=absent)
            edit(torch, data, parity, k, S, absent, "garbage", rng)
            edit(torch, data, parity, k, S, wrong, kind, rng)
            dc, pc = data.clone(), parity.clone()
            set_pattern(enc, absent)
            assert not enc.verify(data, parity, seed=SEED), (t, w)
            assert enc.locate_errors(data, parity, seed=SEED) == wrong, (t, w)
            assert torch.equal(dc, data) and torch.equal(pc, parity)  # locate reads only
            assert enc.correct(data, parity, seed=SEED) == wrong, (t, w)
            torch.cuda.synchronize()
            assert torch.equal(d0, data) and torch.equal(p0, parity)  # every block, the absent ones included
            assert enc.verify(data, parity, seed=SEED + 9)
            enc.scrub_erasures()
            assert enc.verify(data, parity, seed=SEED + 10)


@pytest.mark.parametrize("n,k,S,b,w", [(32, 16, 64, 4, 4), (32, 16, 64, 1, 13), (80, 64, 32, 6, 2), (72, 64, 33, 2, 2), (130, 100, 16, 10, 8)])
def test_known_bad_blocks_plus_errors_plus_erasures(torch_cuda, fe, n, k, S, b, w):
    """b present blocks with a word >= p, w absent blocks and t other corrupted blocks, 2t + b + w = n - k."""
    torch, rng, m = torch_cuda, _rng("bad", n, k, S, b, w), n - k
    t = (m - b - w) // 2
    assert 2 * t + b + w == m and t >= 1
    with fe.Encoder(n, k, 4 * S) as enc:
        data, parity = codeword(torch, enc, S, rng)
        d0, p0 = data.clone(), parity.clone()
        absent = pick_absent(rng, n, k, w)
        chosen = pick_absent(rng, n, k, b + t, avoid=absent)
        big = sorted(int(x) for x in rng.choice(chosen, size=b, replace=False))
        edit(torch, data, parity, k, S, absent, "garbage", rng)
        edit(torch, data, parity, k, S, big, "big", rng)
        edit(torch, data, parity, k, S, [j for j in chosen if j not in big], "random", rng)
        set_pattern(enc, absent)
        assert not enc.verify(data, parity, seed=SEED)
        assert enc.locate_errors(data, parity, seed=SEED) == chosen
        assert enc.correct(data, parity, seed=SEED) == chosen
        torch.cuda.synchronize()
        assert torch.equal(d0, data) and torch.equal(p0, parity)


@pytest.mark.parametrize("n,k,S,t,w", [(8, 4, 32, 2, 1), (32, 16, 64, 4, 9), (80, 64, 32, 3, 11), (72, 64, 33, 1, 7), (130, 100, 16, 8, 15)])
def test_over_budget(torch_cuda, fe, n, k, S, t, w):
    """2t + w = n - k + 1: either FASTECC_E_UNCORRECTABLE with nothing written, or a set whose repair verifies — never asserted which."""
    torch, rng, m = torch_cuda, _rng("over", n, k, S, t, w), n - k
    assert 2 * t + w == m + 1
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.set_option("locate_max", 8)
        data, parity = codeword(torch, enc, S, rng)
        absent = pick_absent(rng, n, k, w)
        wrong = pick_absent(rng, n, k, t, avoid=absent)
        edit(torch, data, parity, k, S, absent, "garbage", rng)
        edit(torch, data, parity, k, S, wrong, "one_word", rng)
        dc, pc = data.clone(), parity.clone()
        set_pattern(enc, absent)
        try:
            got = enc.correct(data, parity, seed=SEED)
        except fe.FastEccError as e:
            assert e.code == fe.E_UNCORRECTABLE
            torch.cuda.synchronize()
            assert torch.equal(dc, data) and torch.equal(pc, parity)
        else:
            assert got == sorted(got) and not set(got) & set(absent)
            enc.scrub_erasures()
            assert enc.verify(data, parity, seed=SEED + 5)  # the closing state is a codeword


@pytest.mark.parametrize("n,k,S", [(8, 4, 32), (72, 64, 33), (130, 100, 16)])
def test_every_parity_worth_absent(torch_cuda, fe, n, k, S):
    """w = n - k: nothing can be checked, so verify answers 1 even with a corrupted present block; one more absent block is refused
    and leaves the pattern in force."""
    torch, rng, m = torch_cuda, _rng("all", n, k, S), n - k
    with fe.Encoder(n, k, 4 * S) as enc:
        data, parity = codeword(torch, enc, S, rng)
        absent = pick_absent(rng, n, k, m)
        wrong = pick_absent(rng, n, k, 1, avoid=absent)
        edit(torch, data, parity, k, S, absent, "garbage", rng)
        edit(torch, data, parity, k, S, wrong, "one_word", rng)
        set_pattern(enc, absent)
        assert enc.verify(data, parity, seed=SEED)
        assert enc.locate_errors(data, parity, seed=SEED) == []
        with pytest.raises(fe.FastEccError) as ei:
            set_pattern(enc, sorted(absent + wrong))
        assert ei.value.code == fe.E_INVAL
        assert enc.verify(data, parity, seed=SEED)  # the previous pattern still holds
        enc.scrub_erasures()
        assert not enc.verify(data, parity, seed=SEED)
        # a present word >= p is an inconsistency whatever the pattern
        set_pattern(enc, absent)
        edit(torch, data, parity, k, S, wrong, "big", rng)
        assert not enc.verify(data, parity, seed=SEED)


@pytest.mark.parametrize("n,k,S", [(32, 16, 64), (72, 64, 33), (130, 100, 16)])
def test_stale_state_single_stripe(torch_cuda, fe, n, k, S):
    """One context through: no pattern, pattern A, a disjoint pattern B, cleared.  No answer may depend on what earlier calls left."""
    torch, rng = torch_cuda, _rng("stale", n, k, S)
    with fe.Encoder(n, k, 4 * S) as enc, fe.Encoder(n, k, 4 * S) as fresh:
        data, parity = codeword(torch, enc, S, rng)
        A = pick_absent(rng, n, k, 3)
        B = pick_absent(rng, n, k, 3, avoid=A)

        def variant(blocks, kind):
            d, p = data.clone(), parity.clone()
            edit(torch, d, p, k, S, blocks, kind, rng)
            return d, p
        clean, corrupted = (data, parity), variant(pick_absent(rng, n, k, 2, avoid=A + B), "one_word")
        in_a, in_b = variant(A, "garbage"), variant(B, "garbage")
        assert not enc.verify(*corrupted, seed=SEED)  # 1. no pattern: F is written at every position
        set_pattern(enc, A)                           # 2.
        assert enc.verify(*in_a, seed=SEED)
        assert not enc.verify(*corrupted, seed=SEED)
        set_pattern(enc, B)                           # 3.
        assert enc.verify(*in_b, seed=SEED)
        assert not enc.verify(*in_a, seed=SEED)
        assert enc.verify(*clean, seed=SEED)
        enc.scrub_erasures()                          # 4. cleared: a fresh context's answers
        for stripe, want in ((clean, True), (in_a, False), (in_b, False), (corrupted, False)):
            assert enc.verify(*stripe, seed=SEED) == fresh.verify(*stripe, seed=SEED) == want
            assert enc.locate_errors(*stripe, seed=SEED) == fresh.locate_errors(*stripe, seed=SEED)
        assert enc.locate_errors(*in_a, seed=SEED) == A


class Pool:
    """`count` stripes back to back: host copies d (count, k, S), p (count, n - k, S) of the clean codewords, device buffers D, Q."""

    def __init__(self, torch, enc, count, S, rng):
        n, k = enc.n, enc.k
        self.torch, self.enc, self.count, self.S, self.n, self.k = torch, enc, count, S, n, k
        self.d = rng.integers(0, P, size=(count, k, S), dtype=np.uint64).astype(np.uint32)
        self.D = to_dev(torch, self.d.reshape(-1))
        self.Q = torch.zeros(count * (n - k) * S, dtype=torch.int32, device="cuda:0")
        for b in range(count):
            enc.encode(*self.stripe(b))
        torch.cuda.synchronize()
        self.p = host(self.Q).reshape(count, n - k, S)

    def stripe(self, b):
        dw, pw = self.k * self.S, (self.n - self.k) * self.S
        return self.D[b * dw:(b + 1) * dw], self.Q[b * pw:(b + 1) * pw]

    def upload(self, d, p):
        self.D.copy_(to_dev(self.torch, d.reshape(-1)))
        self.Q.copy_(to_dev(self.torch, p.reshape(-1)))
        self.torch.cuda.synchronize()

    def contents(self):
        return host(self.D).reshape(self.d.shape), host(self.Q).reshape(self.p.shape)

    def block(self, d, p, b, j):
        return d[b, j] if j < self.k else p[b, j - self.k]

    def with_garbage(self, blocks, rng):
        """Copies of the clean pool with different garbage (word 0 >= p) in `blocks` of every stripe."""
        d, p = self.d.copy(), self.p.copy()
        for b in range(self.count):
            for j in blocks:
                row = self.block(d, p, b, j)
                row[:] = rng.integers(0, 1 << 32, size=self.S, dtype=np.uint64).astype(np.uint32)
                row[0] = np.uint32(P + int(rng.integers(0, (1 << 32) - P)))
        return d, p

    def verify_loop(self, seed):
        return np.array([self.enc.verify(*self.stripe(b), seed=seed) for b in range(self.count)])


def one_word(row, rng):
    w = int(rng.integers(row.shape[0]))
    row[w] = np.uint32((int(row[w]) + 1 + int(rng.integers(P - 1))) % P)


@pytest.mark.parametrize("n,k,S,count,wa", [(20, 16, 16, 37, 1), (32, 16, 64, 19, 3)])
def test_batch(torch_cuda, fe, n, k, S, count, wa):
    torch, rng, m = torch_cuda, _rng("batch", n, k, S, count), n - k
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.set_option("scrub_batch_chunk", 8)  # chunks are crossed, the last one is ragged
        enc.set_option("locate_max", 1)
        pool = Pool(torch, enc, count, S, rng)
        A = pick_absent(rng, n, k, wa)
        B = pick_absent(rng, n, k, wa, avoid=A)
        # 1. no pattern, one corrupted stripe: every position of the batch's fingerprint stripe gets written
        d, p = pool.d.copy(), pool.p.copy()
        one_word(pool.block(d, p, 5, 2), rng)
        pool.upload(d, p)
        assert enc.verify_batch(pool.D, pool.Q, count, seed=SEED).tolist() == [b != 5 for b in range(count)]
        # 2. pattern A, garbage in A
        ga, gb = pool.with_garbage(A, rng), pool.with_garbage(B, rng)
        set_pattern(enc, A)
        pool.upload(*ga)
        assert enc.verify_batch(pool.D, pool.Q, count, seed=SEED).all()
        # 3. pattern B: garbage in B is fine, garbage in A is not
        set_pattern(enc, B)
        pool.upload(*gb)
        assert enc.verify_batch(pool.D, pool.Q, count, seed=SEED).all()
        pool.upload(*ga)
        assert not enc.verify_batch(pool.D, pool.Q, count, seed=SEED).any()
        # pattern B, garbage in B; errors in a few stripes, a present word >= p in one, one stripe beyond reach:
        # t = 2 > locate_max = 1, and t + locate_max = 3 < n - k - w + 1 (the distance left), so no codeword is within reach
        assert 3 < m - wa + 1
        d, p = gb[0].copy(), gb[1].copy()
        present = [j for j in range(n) if j not in B]
        fixable, big_stripe, hopeless = [1, 8, 15, count - 1], 11, 9
        for b in fixable:
            one_word(pool.block(d, p, b, int(rng.choice(present))), rng)
        pool.block(d, p, big_stripe, int(rng.choice(present)))[3] = np.uint32(P + 7)
        for j in rng.choice(present, size=2, replace=False):
            one_word(pool.block(d, p, hopeless, int(j)), rng)
        pool.upload(d, p)
        bad = sorted(fixable + [big_stripe, hopeless])
        for seed in (SEED, SEED + 1):
            got = enc.verify_batch(pool.D, pool.Q, count, seed=seed)
            assert np.array_equal(got, pool.verify_loop(seed))  # the single-stripe answer under the same pattern and seed
            assert sorted(np.nonzero(~got)[0].tolist()) == bad
        hd, hq = pool.contents()
        assert np.array_equal(hd, d) and np.array_equal(hq, p)  # reads only
        err = uncorrectable(fe, enc.correct_batch, pool.D, pool.Q, count, seed=SEED)
        want = np.zeros(count, np.uint8)
        want[fixable + [big_stripe]] = 1
        want[hopeless] = 2
        assert np.array_equal(err.status, want)
        hd, hq = pool.contents()
        for b in range(count):
            if want[b] == 1:  # the original codeword in every block, the absent ones included
                assert np.array_equal(hd[b], pool.d[b]) and np.array_equal(hq[b], pool.p[b]), b
            else:             # untouched: consistent (garbage and all) or uncorrectable
                assert np.array_equal(hd[b], d[b]) and np.array_equal(hq[b], p[b]), b
        # 4. cleared: the old answers — garbage in B makes every stripe but the repaired ones inconsistent
        enc.scrub_erasures()
        assert enc.verify_batch(pool.D, pool.Q, count, seed=SEED).tolist() == [bool(want[b] == 1) for b in range(count)]


def test_refused_contexts(torch_cuda, fe):
    for make in (lambda: fe.Encoder(64, 32, 64, field=fe.FIELD_GF_P61_SQUARED), lambda: fe.ShardedEncoder(64, 32, 256, [0, 0]),
                 lambda: fe.Encoder(2 * 48, 48, 64, flags=fe.CODE_MIXED_RADIX)):
        with make() as enc:
            for args in ((), presence(enc.n, enc.k, [1, enc.k])):
                with pytest.raises(fe.FastEccError) as ei:
                    enc.scrub_erasures(*args)
                assert ei.value.code == fe.E_UNSUPPORTED


def test_pattern_is_independent_of_the_decoder(torch_cuda, fe):
    torch, rng = torch_cuda, _rng("independent")
    n, k, S = 64, 32, 32
    with fe.Encoder(n, k, 4 * S) as enc:
        data, parity = codeword(torch, enc, S, rng)
        d0, p0 = data.clone(), parity.clone()
        absent = [2, k + 1]
        set_pattern(enc, absent)
        # decode and repair with another loss pattern while the scrub pattern is set
        lost = [0, 5, 9, k + 7]
        dp, pp = presence(n, k, lost)
        for j in lost:
            (data if j < k else parity)[(j % k) * S:(j % k + 1) * S].zero_()
        enc.decode_prepare(dp, pp)
        enc.decode(data, parity)
        torch.cuda.synchronize()
        assert torch.equal(d0, data)
        enc.repair(data, parity)
        torch.cuda.synchronize()
        assert torch.equal(d0, data) and torch.equal(p0, parity)
        # decode_prepare left the scrub pattern alone
        edit(torch, data, parity, k, S, absent, "garbage", rng)
        assert enc.verify(data, parity, seed=SEED)
        # correct (it replaces the DECODE pattern) leaves it alone too
        edit(torch, data, parity, k, S, [7, k + 20], "one_word", rng)
        assert enc.correct(data, parity, seed=SEED) == [7, k + 20]
        torch.cuda.synchronize()
        assert torch.equal(d0, data) and torch.equal(p0, parity)
        edit(torch, data, parity, k, S, absent, "garbage", rng)
        assert enc.verify(data, parity, seed=SEED + 1)
        assert enc.correct(data, parity, seed=SEED + 1) == []
        enc.scrub_erasures()
        assert not enc.verify(data, parity, seed=SEED + 1)
