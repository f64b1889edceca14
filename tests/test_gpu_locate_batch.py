"""GPU tests (-m gpu) of batched error location (fastecc_locate_errors_batch) and of the grouped path of fastecc_correct_batch
(option "correct_batch_mode").

The expected answers are the corruption the tests inject, a loop of the single-stripe fastecc_locate_errors with the same seed and
named erasures (which the batch must equal stripe for stripe, refusals included), and fastecc_correct_batch stripe by stripe
(mode 2), which the grouped path (mode 1) must equal byte for byte.  A guard region after the last stripe of both buffers must never
change.  Pool, corrupt_block and the guard words follow tests/test_gpu_scrub_batch.py."""
import ctypes
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 0xFFF00001
SEED = 0x5EED
GUARD = 1024  # words after the last stripe of data and of parity
GUARD_WORD = 0xA5A5A5A5
SENTINEL = 0xFEEDFACECAFEBEEF


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
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to("cuda:0")


def host(t):
    return t.cpu().numpy().view(np.uint32).copy()


class Pool:
    """`count` stripes of an (n, k) code with S-word blocks: host copies d (count, k, S), p (count, n - k, S) of the clean codewords,
    device buffers D, Q holding the stripes plus GUARD words each.  skew: D starts that many words into its allocation (a data pointer
    that is 4-byte but not 16-byte aligned), with guard words in front as well."""

    def __init__(self, torch, enc, count, S, rng, skew=0):
        n, k = enc.n, enc.k
        self.torch, self.enc, self.count, self.S, self.n, self.k, self.skew = torch, enc, count, S, n, k, skew
        d = rng.integers(0, P, size=(count, k, S), dtype=np.uint64).astype(np.uint32)
        guard = np.full(GUARD, GUARD_WORD, np.uint32)
        self.Dall = to_dev(torch, np.concatenate([guard[:skew], d.reshape(-1), guard]))
        self.D = self.Dall[skew:]
        self.Q = to_dev(torch, np.concatenate([np.zeros(count * (n - k) * S, np.uint32), guard]))
        dw, pw = k * S, (n - k) * S
        aligned = to_dev(torch, d.reshape(-1)) if skew else self.D
        for b in range(count):  # the single-stripe encoder, stripe by stripe
            enc.encode(aligned[b * dw:(b + 1) * dw], self.Q[b * pw:(b + 1) * pw])
        torch.cuda.synchronize()
        self.d = d
        self.p = host(self.Q)[:count * pw].reshape(count, n - k, S)

    def stripe(self, b):
        dw, pw = self.k * self.S, (self.n - self.k) * self.S
        return self.D[b * dw:(b + 1) * dw], self.Q[b * pw:(b + 1) * pw]

    def upload(self, d, p):
        guard = np.full(GUARD, GUARD_WORD, np.uint32)
        self.Dall.copy_(to_dev(self.torch, np.concatenate([guard[:self.skew], d.reshape(-1), guard])))
        self.Q.copy_(to_dev(self.torch, np.concatenate([p.reshape(-1), guard])))
        self.torch.cuda.synchronize()

    def contents(self):
        """(data, parity, guards intact)"""
        hd, hq = host(self.Dall), host(self.Q)
        nd, nq = self.count * self.k * self.S, self.count * (self.n - self.k) * self.S
        guards = (hd[:self.skew] == GUARD_WORD).all() and (hd[self.skew + nd:] == GUARD_WORD).all() and (hq[nq:] == GUARD_WORD).all()
        return hd[self.skew:self.skew + nd].reshape(self.d.shape), hq[:nq].reshape(self.p.shape), guards

    def locate_loop(self, fe, seed):
        """(status, lists) of a loop of the single-stripe locate_errors, E_UNCORRECTABLE mapped to status 2"""
        status, lists = np.zeros(self.count, np.uint8), []
        for b in range(self.count):
            try:
                found = self.enc.locate_errors(*self.stripe(b), seed=seed)
            except fe.FastEccError as e:
                assert e.code == fe.E_UNCORRECTABLE
                status[b], found = 2, []
            else:
                status[b] = 1 if found else 0
            lists.append(found)
        return status, lists


def corrupt_block(d, p, k, b, j, kind, rng, donor=None):
    """Corrupt block j of stripe b of the host copies in place."""
    row = d[b, j] if j < k else p[b, j - k]
    S = row.shape[0]
    w = int(rng.integers(S))
    if kind == "big":
        row[w] = np.uint32(P + int(rng.integers(0, (1 << 32) - P)))
    elif kind == "misdirected":  # the same block of another stripe: a write that landed in the wrong place
        src = d[donor, j] if j < k else p[donor, j - k]
        assert not np.array_equal(src, row)
        row[:] = src
    elif kind == "one_word":
        row[w] = np.uint32((int(row[w]) + 1 + int(rng.integers(P - 1))) % P)
    else:
        raise ValueError(kind)


# (n, k, S): (2k,k), n = k + N/2^d, zero-extended, n = k + N/2^d with zero extension, 4k, 8k
CODES = [(256, 128, 16), (20, 16, 32), (130, 100, 8), (80, 64, 12), (64, 16, 16), (64, 8, 8)]
COUNTS = [1, 7, 300]


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def locate_batch_raw(fe, enc, pool, seed, cap):
    """the C call: (return code, status, counts, blocks — count * cap entries and 16 more, prefilled with SENTINEL —, inconsistent)"""
    count = pool.count
    status = np.full(count, 0xAB, np.uint8)
    counts = np.full(count, 0xC0C0, np.uint32)
    blocks = np.full(count * cap + 16, SENTINEL, np.uint64)
    inc = ctypes.c_uint64(12345)
    rc = fe.lib().fastecc_locate_errors_batch(enc._h, pool.D.data_ptr(), pool.Q.data_ptr(), count, None, seed,
                                             status.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), blocks.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                             cap, counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(inc))
    return rc, status, counts, blocks, inc.value


def locate_batch(fe, enc, pool, seed):
    """the Python method, E_UNCORRECTABLE folded in: (status, lists)"""
    try:
        return enc.locate_errors_batch(pool.D, pool.Q, pool.count, seed=seed)
    except fe.FastEccError as e:
        assert e.code == fe.E_UNCORRECTABLE and (e.status == 2).any()
        return e.status, e.lists


def location_case(torch, fe, n, k, S, count, chunk=0):
    rng = _rng("locate", n, k, S, count, chunk)
    m = n - k
    with fe.Encoder(n, k, 4 * S) as enc:
        if chunk:
            enc.set_option("scrub_batch_chunk", chunk)
        pool = Pool(torch, enc, count, S, rng)
        d, p = pool.d.copy(), pool.p.copy()
        kinds = ["one_word", "clean", "misdirected", "big", "clean", "one_word", "clean"] + (["over"] if (n, k) == (20, 16) else [])
        injected = {}  # stripe -> the corrupted blocks, where location is guaranteed
        for b in range(count):
            kind = kinds[(b + count) % len(kinds)] if count > 1 else "one_word"
            if kind == "clean":
                continue
            if kind == "one_word":
                t = int(rng.integers(1, min(3, m // 2) + 1))
                blocks = sorted(int(x) for x in rng.choice(n, size=t, replace=False))
                for j in blocks:
                    corrupt_block(d, p, k, b, j, "one_word", rng)
                injected[b] = blocks
            elif kind == "over":  # three errors in (20,16): beyond the guarantee, whatever the single-stripe call says
                for j in rng.choice(n, size=3, replace=False):
                    corrupt_block(d, p, k, b, int(j), "one_word", rng)
            else:
                j = int(rng.integers(n))
                corrupt_block(d, p, k, b, j, kind, rng, donor=(b + 1) % count)
                injected[b] = [j]
        pool.upload(d, p)
        for seed in (SEED, SEED + 1):
            want_status, want_lists = pool.locate_loop(fe, seed)
            status, lists = locate_batch(fe, enc, pool, seed)
            assert np.array_equal(status, want_status)
            assert lists == want_lists
            for b, blocks in injected.items():
                assert status[b] == 1 and lists[b] == blocks, b
            # the C call with cap = 1: full counts, one entry per located stripe, nothing written behind them
            rc, st1, counts, blk, inc = locate_batch_raw(fe, enc, pool, seed, 1)
            assert rc == (fe.E_UNCORRECTABLE if (want_status == 2).any() else fe.OK)
            assert np.array_equal(st1, want_status) and inc == int(np.count_nonzero(want_status))
            assert counts.tolist() == [len(x) for x in want_lists]
            assert blk[:count].tolist() == [x[0] if x else SENTINEL for x in want_lists] and (blk[count:] == SENTINEL).all()
        hd, hq, guards = pool.contents()
        assert np.array_equal(hd, d) and np.array_equal(hq, p) and guards  # reads only


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("n,k,S", CODES)
def test_location_equals_single_stripe(torch_cuda, fe, n, k, S, count):
    location_case(torch_cuda, fe, n, k, S, count)


@pytest.mark.parametrize("n,k,S,count,chunk", [(256, 128, 16, 150, 64), (20, 16, 32, 333, 100), (64, 8, 8, 70, 7)])
def test_location_across_forced_chunks(torch_cuda, fe, n, k, S, count, chunk):
    location_case(torch_cuda, fe, n, k, S, count, chunk)


@pytest.mark.parametrize("n,k,S,count,absent", [(20, 16, 32, 60, 5), (20, 16, 32, 60, 18), (256, 128, 16, 40, 200)])
def test_location_degraded(torch_cuda, fe, n, k, S, count, absent):
    torch = torch_cuda
    rng = _rng("degraded", n, k, S, absent)
    with fe.Encoder(n, k, 4 * S) as enc:
        pool = Pool(torch, enc, count, S, rng)
        d, p = pool.d.copy(), pool.p.copy()
        (d[:, absent] if absent < k else p[:, absent - k])[...] = 0xFFFFFFFF  # the absent block holds garbage in every stripe
        present = [j != absent for j in range(n)]
        enc.scrub_erasures(present[:k], present[k:])
        injected = {}
        for b in range(0, count, 3):
            j = int(rng.choice([x for x in range(n) if x != absent]))
            corrupt_block(d, p, k, b, j, "one_word", rng)
            injected[b] = [j]
        pool.upload(d, p)
        for seed in (SEED, SEED + 1):
            want_status, want_lists = pool.locate_loop(fe, seed)
            status, lists = locate_batch(fe, enc, pool, seed)
            assert np.array_equal(status, want_status) and lists == want_lists
            for b in range(count):
                assert lists[b] == injected.get(b, [])  # the absent block is not listed
        hd, hq, guards = pool.contents()
        assert np.array_equal(hd, d) and np.array_equal(hq, p) and guards


def correct_with_mode(fe, enc, pool, d, p, mode):
    """the corrupted pool corrected under correct_batch_mode `mode`: (status, data, parity, guards intact)"""
    pool.upload(d, p)
    enc.set_option("correct_batch_mode", mode)
    try:
        status = enc.correct_batch(pool.D, pool.Q, pool.count, seed=SEED)
    except fe.FastEccError as e:
        assert e.code == fe.E_UNCORRECTABLE and (e.status == 2).any()
        status = e.status
    return (status,) + pool.contents()


def grouped_equals_loop(fe, enc, pool, d, p, want):
    """mode 1 against mode 2 on identical pools; where the status is 1 the stripe is the clean one, elsewhere it is untouched"""
    s1, d1, p1, g1 = correct_with_mode(fe, enc, pool, d, p, 1)
    s2, d2, p2, g2 = correct_with_mode(fe, enc, pool, d, p, 2)
    assert g1 and g2
    assert np.array_equal(s1, s2) and np.array_equal(d1, d2) and np.array_equal(p1, p2)
    assert np.array_equal(s1, want)
    for b in range(pool.count):
        if s1[b] == 1:
            assert np.array_equal(d1[b], pool.d[b]) and np.array_equal(p1[b], pool.p[b]), b
        else:
            assert np.array_equal(d1[b], d[b]) and np.array_equal(p1[b], p[b]), b
    return s1


def small_pool(torch, fe, n, k, S, count, rng, **kw):
    enc = fe.Encoder(n, k, 4 * S)
    enc.set_option("locate_max", 8)
    enc.set_option("decode_batch_kernel", 1)
    return enc, Pool(torch, enc, count, S, rng, **kw)


def test_grouped_same_block_in_every_stripe(torch_cuda, fe):
    n, k, S, count = 20, 16, 32, 300
    rng = _rng("grouped a")
    enc, pool = small_pool(torch_cuda, fe, n, k, S, count, rng)
    with enc:
        d, p = pool.d.copy(), pool.p.copy()
        for b in range(count):
            corrupt_block(d, p, k, b, 3, "one_word", rng)
        grouped_equals_loop(fe, enc, pool, d, p, np.ones(count, np.uint8))


@pytest.mark.parametrize("n,k,S,count,chunk", [(256, 128, 16, 40, 0), (20, 16, 32, 300, 64), (130, 100, 8, 25, 0), (64, 16, 16, 30, 0)])
def test_grouped_random_patterns(torch_cuda, fe, n, k, S, count, chunk):
    rng = _rng("grouped b", n, k, S, count)
    m = n - k
    enc, pool = small_pool(torch_cuda, fe, n, k, S, count, rng)
    with enc:
        if chunk:
            enc.set_option("scrub_batch_chunk", chunk)
        d, p = pool.d.copy(), pool.p.copy()
        bad = sorted(set(int(x) for x in rng.choice(count, size=max(1, count // 4), replace=False)))
        for b in bad:  # 2t + b_big <= n - k, t <= locate_max
            nb = int(rng.integers(0, min(2, m) + 1))
            t = int(rng.integers(1 if nb == 0 else 0, min(8, (m - nb) // 2) + 1))
            blocks = [int(x) for x in rng.choice(n, size=nb + t, replace=False)]
            for j in blocks[:nb]:
                corrupt_block(d, p, k, b, j, "big", rng)
            for j in blocks[nb:]:
                corrupt_block(d, p, k, b, j, "one_word", rng)
        want = np.zeros(count, np.uint8)
        want[bad] = 1
        grouped_equals_loop(fe, enc, pool, d, p, want)
        assert enc.verify_batch(pool.D, pool.Q, count, seed=SEED + 3).all()


def test_grouped_uncorrectable_stripe_is_untouched(torch_cuda, fe):
    n, k, S, count = 20, 16, 32, 12
    rng = _rng("grouped c")
    enc, pool = small_pool(torch_cuda, fe, n, k, S, count, rng)
    with enc:
        d, p = pool.d.copy(), pool.p.copy()
        for j in (0, 5, 17):  # 3 unknown errors > (n - k) / 2
            corrupt_block(d, p, k, 4, j, "one_word", rng)
        for b, j in ((1, 3), (9, 18), (10, 3)):  # one each: correctable
            corrupt_block(d, p, k, b, j, "one_word", rng)
        want = np.zeros(count, np.uint8)
        want[[1, 9, 10]] = 1
        want[4] = 2
        grouped_equals_loop(fe, enc, pool, d, p, want)


@pytest.mark.parametrize("absent", [7, 17])
def test_grouped_degraded(torch_cuda, fe, absent):
    n, k, S, count = 20, 16, 32, 50
    rng = _rng("grouped d", absent)
    enc, pool = small_pool(torch_cuda, fe, n, k, S, count, rng)
    with enc:
        d, p = pool.d.copy(), pool.p.copy()
        (d[:, absent] if absent < k else p[:, absent - k])[...] = 0xFFFFFFFF
        present = [j != absent for j in range(n)]
        enc.scrub_erasures(present[:k], present[k:])
        want = np.zeros(count, np.uint8)
        for b in range(0, count, 4):
            corrupt_block(d, p, k, b, int(rng.choice([x for x in range(n) if x != absent])), "one_word", rng)
            want[b] = 1
        # located stripes come back whole, the absent block rebuilt too; consistent stripes keep their garbage (grouped_equals_loop checks both)
        grouped_equals_loop(fe, enc, pool, d, p, want)


def test_grouped_path_runs(torch_cuda, fe):
    """block 3 wrong in every stripe, mode 1: one list repair where fastecc_repair_batch has one batched pass, no single-stripe work"""
    n, k, S, count = 20, 16, 32, 300
    rng = _rng("grouped runs")
    enc, pool = small_pool(torch_cuda, fe, n, k, S, count, rng)
    with enc:
        d, p = pool.d.copy(), pool.p.copy()
        for b in range(count):
            corrupt_block(d, p, k, b, 3, "one_word", rng)
        pool.upload(d, p)
        enc.set_option("correct_batch_mode", 1)
        enc.profile(True)
        enc.profile_reset()
        status = enc.correct_batch(pool.D, pool.Q, count, seed=SEED)
        grouped = enc.profile_read()
        assert (status == 1).all()
        hd, hq, guards = pool.contents()
        assert np.array_equal(hd, pool.d) and np.array_equal(hq, pool.p) and guards
        pool.upload(d, p)
        present = [j != 3 for j in range(n)]
        enc.decode_prepare(present[:k], present[k:])
        enc.profile_reset()
        enc.repair_batch(pool.D, pool.Q, count)
        whole = enc.profile_read()
        enc.profile(False)
        assert whole["direct_pass_batch"][1] >= 1
        assert grouped["direct_pass_list"][1] == whole["direct_pass_batch"][1]
        assert "fingerprint" not in grouped and "direct_pass" not in grouped and "direct_pass_batch" not in grouped
        for scope in ("fingerprint_batch_list", "scrub_syndromes_gather", "scrub_root_search_batch"):
            assert grouped[scope][1] >= 1, scope


@pytest.mark.parametrize("S,skew", [(8, 0), (9, 0), (12, 0), (8, 1), (12, 1)])
def test_list_kernel_edges(torch_cuda, fe, S, skew):
    """blocks far below a wave's 64 V words, a flagged list of the first, the last and scattered stripes, a pattern of a single stripe, and a
    data pointer that is only 4-byte aligned"""
    n, k, count = 20, 16, 70
    rng = _rng("edges", S, skew)
    enc, pool = small_pool(torch_cuda, fe, n, k, S, count, rng, skew=skew)
    with enc:
        assert pool.D.data_ptr() % 16 == (4 * skew) % 16
        d, p = pool.d.copy(), pool.p.copy()
        want = np.zeros(count, np.uint8)
        for b in (0, 13, 14, 37, 64, count - 1):  # one pattern in several stripes
            corrupt_block(d, p, k, b, 2, "one_word", rng)
            want[b] = 1
        for b, blocks in ((5, (2, 19)), (41, (17,)), (66, (0, 15))):  # patterns of a single stripe each
            for j in blocks:
                corrupt_block(d, p, k, b, j, "one_word", rng)
            want[b] = 1
        pool.upload(d, p)
        status, lists = enc.locate_errors_batch(pool.D, pool.Q, count, seed=SEED)
        assert np.array_equal(status, want) and lists[5] == [2, 19] and lists[count - 1] == [2] and lists[66] == [0, 15]
        grouped_equals_loop(fe, enc, pool, d, p, want)


def test_grouped_transform_path_patterns(torch_cuda, fe):
    """decode_direct_max = 0: every pattern takes the decoder's transform path, which the list repair runs stripe by stripe"""
    n, k, S, count = 256, 128, 16, 40
    rng = _rng("transform path")
    enc, pool = small_pool(torch_cuda, fe, n, k, S, count, rng)
    with enc:
        enc.set_option("decode_direct_max", 0)
        d, p = pool.d.copy(), pool.p.copy()
        want = np.zeros(count, np.uint8)
        for b in rng.choice(count, size=10, replace=False):
            for j in rng.choice(n, size=int(rng.integers(1, 4)), replace=False):
                corrupt_block(d, p, k, int(b), int(j), "one_word", rng)
            want[int(b)] = 1
        grouped_equals_loop(fe, enc, pool, d, p, want)


def test_offsets_beyond_32_bits(torch_cuda, fe):
    """(20,16) x 4 KB x 66000 stripes, all zero (a pool of codewords): the data alone is over 4 GiB.  One word changes in a stripe past
    the 4 GiB mark and one in the last stripe; location names exactly those blocks and the grouped correction returns the pool to zero."""
    torch = torch_cuda
    n, k, S, B = 20, 16, 1024, 66000
    M = n - k
    hits = {65600: 4, B - 1: 18}
    assert 65600 * k * S * 4 > 1 << 32
    with fe.Encoder(n, k, 4 * S) as enc:
        data = torch.zeros(B * k * S, dtype=torch.int32, device="cuda:0")
        parity = torch.zeros(B * M * S, dtype=torch.int32, device="cuda:0")
        for b, j in hits.items():
            (data if j < k else parity)[(b * k + j if j < k else b * M + j - k) * S + 77] = 123456
        status, lists = enc.locate_errors_batch(data, parity, B, seed=SEED)
        assert np.flatnonzero(status).tolist() == sorted(hits) and (status[sorted(hits)] == 1).all()
        for b, j in hits.items():
            assert lists[b] == [j]
        assert int(torch.count_nonzero(data)) == 1 and int(torch.count_nonzero(parity)) == 1  # reads only
        enc.set_option("correct_batch_mode", 1)
        status = enc.correct_batch(data, parity, B, seed=SEED)
        assert np.flatnonzero(status).tolist() == sorted(hits) and (status[sorted(hits)] == 1).all()
        assert int(torch.count_nonzero(data)) == 0 and int(torch.count_nonzero(parity)) == 0


def _refused(fe, enc, D, Q, count, want):
    status = (ctypes.c_uint8 * count)(*([7] * count))
    counts = (ctypes.c_uint32 * count)(*([9] * count))
    blocks = (ctypes.c_uint64 * (2 * count))(*([11] * (2 * count)))
    inc = ctypes.c_uint64(12345)
    rc = fe.lib().fastecc_locate_errors_batch(enc._h, D.data_ptr(), Q.data_ptr(), count, None, SEED, status, blocks, 2, counts, ctypes.byref(inc))
    assert rc == want
    assert list(status) == [7] * count and list(counts) == [9] * count and list(blocks) == [11] * (2 * count) and inc.value == 12345


def test_refusals(torch_cuda, fe):
    torch = torch_cuda
    rng = _rng("refusals")
    count = 3
    with fe.Encoder(128, 96, 64, flags=fe.CODE_MIXED_RADIX) as enc:  # mixed radix
        D, Q = to_dev(torch, rng.integers(0, P, size=count * 96 * 16, dtype=np.uint64)), torch.zeros(count * 32 * 16, dtype=torch.int32, device="cuda:0")
        d0, q0 = D.clone(), Q.clone()
        _refused(fe, enc, D, Q, count, fe.E_UNSUPPORTED)
        torch.cuda.synchronize()
        assert torch.equal(D, d0) and torch.equal(Q, q0)
    with fe.Encoder(64, 32, 16 * 8, field=fe.FIELD_GF_P61_SQUARED) as enc:  # the 64-bit field
        D, Q = torch.ones(count * 32 * 32, dtype=torch.int32, device="cuda:0"), torch.ones(count * 32 * 32, dtype=torch.int32, device="cuda:0")
        _refused(fe, enc, D, Q, count, fe.E_UNSUPPORTED)
        torch.cuda.synchronize()
        assert (D == 1).all() and (Q == 1).all()
    with fe.Encoder(32, 16, 60) as enc:  # a set row pitch
        enc.set_option("row_pitch_words", 16)
        D, Q = torch.ones(count * 16 * 16, dtype=torch.int32, device="cuda:0"), torch.ones(count * 16 * 16, dtype=torch.int32, device="cuda:0")
        _refused(fe, enc, D, Q, count, fe.E_UNSUPPORTED)
        torch.cuda.synchronize()
        assert (D == 1).all() and (Q == 1).all()


def test_stream_order(torch_cuda, fe):
    """encode and locate_errors_batch on one non-blocking stream: the batch sees the encoded parity."""
    torch = torch_cuda
    n, k, S, count = 256, 128, 64, 16
    rng = _rng("stream")
    s = torch.cuda.Stream(device=0)  # non-blocking with respect to the null stream
    with fe.Encoder(n, k, 4 * S) as enc:
        d = rng.integers(0, P, size=count * k * S, dtype=np.uint64).astype(np.uint32)
        D = to_dev(torch, d)
        Q = torch.full((count * (n - k) * S,), 7, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            h = s.cuda_stream
            for b in range(count):
                enc.encode(D[b * k * S:(b + 1) * k * S], Q[b * (n - k) * S:(b + 1) * (n - k) * S], stream=h)
            status, lists = enc.locate_errors_batch(D, Q, count, seed=SEED, stream=h)
        assert (status == 0).all() and lists == [[]] * count
