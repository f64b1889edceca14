"""GPU tests (-m gpu) of the batched scrub: fastecc_verify_batch and fastecc_correct_batch.

Stripes lie back to back (the layout of fastecc_decode_batch); the codewords come from the single-stripe encoder.  The expected answers
are the corruption the tests inject and a loop of the single-stripe fastecc_verify with the same seed, which must agree stripe for
stripe.  A guard region after the last stripe of both buffers must never change."""
import ctypes
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 0xFFF00001
SEED = 0x5EED
GUARD = 1024  # words after the last stripe of data and of parity
GUARD_WORD = 0xA5A5A5A5


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
    device buffers D, Q holding the stripes plus GUARD words each."""

    def __init__(self, torch, enc, count, S, rng):
        n, k = enc.n, enc.k
        self.torch, self.enc, self.count, self.S, self.n, self.k = torch, enc, count, S, n, k
        d = rng.integers(0, P, size=(count, k, S), dtype=np.uint64).astype(np.uint32)
        guard = np.full(GUARD, GUARD_WORD, np.uint32)
        self.D = to_dev(torch, np.concatenate([d.reshape(-1), guard]))
        self.Q = to_dev(torch, np.concatenate([np.zeros(count * (n - k) * S, np.uint32), guard]))
        dw, pw = k * S, (n - k) * S
        for b in range(count):  # the single-stripe encoder, stripe by stripe
            enc.encode(self.D[b * dw:(b + 1) * dw], self.Q[b * pw:(b + 1) * pw])
        torch.cuda.synchronize()
        self.d = d
        self.p = host(self.Q)[:count * pw].reshape(count, n - k, S)

    def stripe(self, b):
        dw, pw = self.k * self.S, (self.n - self.k) * self.S
        return self.D[b * dw:(b + 1) * dw], self.Q[b * pw:(b + 1) * pw]

    def upload(self, d, p):
        guard = np.full(GUARD, GUARD_WORD, np.uint32)
        self.D.copy_(to_dev(self.torch, np.concatenate([d.reshape(-1), guard])))
        self.Q.copy_(to_dev(self.torch, np.concatenate([p.reshape(-1), guard])))
        self.torch.cuda.synchronize()

    def contents(self):
        """(data, parity, guards intact)"""
        hd, hq = host(self.D), host(self.Q)
        nd, nq = self.count * self.k * self.S, self.count * (self.n - self.k) * self.S
        guards = (hd[nd:] == GUARD_WORD).all() and (hq[nq:] == GUARD_WORD).all()
        return hd[:nd].reshape(self.d.shape), hq[:nq].reshape(self.p.shape), guards

    def verify_loop(self, seed):
        return np.array([self.enc.verify(*self.stripe(b), seed=seed) for b in range(self.count)])


def corrupt_block(d, p, k, b, j, kind, rng, donor=None):
    """Corrupt block j of stripe b of the host copies in place."""
    row = d[b, j] if j < k else p[b, j - k]
    S = row.shape[0]
    w = int(rng.integers(S))
    if kind == "flip":
        row[w] ^= np.uint32(1 << int(rng.integers(20)))  # stays < 2^32; a changed word (it may leave [0, p): also a corruption)
    elif kind == "big":
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


def detection_case(torch, fe, n, k, S, count, chunk=0):
    rng = _rng(n, k, S, count, chunk)
    with fe.Encoder(n, k, 4 * S) as enc:
        if chunk:
            enc.set_option("scrub_batch_chunk", chunk)
        pool = Pool(torch, enc, count, S, rng)
        # clean pool: every stripe consistent, nothing written
        ok = enc.verify_batch(pool.D, pool.Q, count, seed=SEED)
        assert ok.dtype == bool and ok.shape == (count,) and ok.all()
        d, p = pool.d.copy(), pool.p.copy()
        bad = sorted(set(int(x) for x in rng.choice(count, size=max(1, count // 5), replace=False)))
        kinds = ["flip", "flip_parity", "big", "misdirected"]
        for i, b in enumerate(bad):
            kind = kinds[i % 4]
            if kind == "misdirected" and count == 1:
                kind = "flip"
            if kind == "flip_parity":
                corrupt_block(d, p, k, b, int(k + rng.integers(n - k)), "flip", rng)
            elif kind == "flip":
                corrupt_block(d, p, k, b, int(rng.integers(k)), "flip", rng)
            elif kind == "big":
                corrupt_block(d, p, k, b, int(rng.integers(n)), "big", rng)
            else:
                corrupt_block(d, p, k, b, int(rng.integers(n)), "misdirected", rng, donor=(b + 1) % count)
        pool.upload(d, p)
        for seed in (SEED, SEED + 1):
            cons = (ctypes.c_uint8 * count)()
            inc = ctypes.c_uint64()
            rc = fe.lib().fastecc_verify_batch(enc._h, pool.D.data_ptr(), pool.Q.data_ptr(), count, None, seed, cons, ctypes.byref(inc))
            assert rc == fe.OK
            got = np.frombuffer(cons, np.uint8)
            assert set(got.tolist()) <= {0, 1}
            want = pool.verify_loop(seed)
            assert np.array_equal(got.astype(bool), want)  # bit for bit the single-stripe answer
            assert sorted(np.nonzero(got == 0)[0].tolist()) == bad  # and exactly the corrupted stripes
            assert inc.value == len(bad)
        hd, hq, guards = pool.contents()
        assert np.array_equal(hd, d) and np.array_equal(hq, p) and guards  # reads only


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("n,k,S", CODES)
def test_verify_batch_detects_and_matches_single(torch_cuda, fe, n, k, S, count):
    detection_case(torch_cuda, fe, n, k, S, count)


@pytest.mark.parametrize("n,k,S,count,chunk", [(256, 128, 16, 150, 64), (20, 16, 32, 333, 100), (64, 8, 8, 70, 7)])
def test_verify_batch_across_forced_chunks(torch_cuda, fe, n, k, S, count, chunk):
    detection_case(torch_cuda, fe, n, k, S, count, chunk)


@pytest.mark.parametrize("n,k,S,count,chunk", [(256, 128, 16, 40, 0), (20, 16, 32, 300, 64), (130, 100, 8, 25, 0), (64, 16, 16, 30, 0)])
def test_correct_batch_restores(torch_cuda, fe, n, k, S, count, chunk):
    torch = torch_cuda
    rng = _rng("correct", n, k, S, count)
    m = n - k
    with fe.Encoder(n, k, 4 * S) as enc:
        if chunk:
            enc.set_option("scrub_batch_chunk", chunk)
        enc.set_option("locate_max", 8)
        pool = Pool(torch, enc, count, S, rng)
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
        pool.upload(d, p)
        status = enc.correct_batch(pool.D, pool.Q, count, seed=SEED)
        want = np.zeros(count, np.uint8)
        want[bad] = 1
        assert np.array_equal(status, want)
        hd, hq, guards = pool.contents()
        assert np.array_equal(hd, pool.d) and np.array_equal(hq, pool.p) and guards
        assert enc.verify_batch(pool.D, pool.Q, count, seed=SEED + 3).all()


def test_correct_batch_too_many_errors(torch_cuda, fe):
    torch = torch_cuda
    n, k, S, count = 20, 16, 32, 12
    rng = _rng("too many")
    with fe.Encoder(n, k, 4 * S) as enc:
        pool = Pool(torch, enc, count, S, rng)
        d, p = pool.d.copy(), pool.p.copy()
        for j in (0, 5, 17):  # 3 unknown errors > (n - k) / 2
            corrupt_block(d, p, k, 4, j, "one_word", rng)
        for b, j in ((1, 3), (9, 18)):  # one each: correctable
            corrupt_block(d, p, k, b, j, "one_word", rng)
        pool.upload(d, p)
        with pytest.raises(fe.FastEccError) as ei:
            enc.correct_batch(pool.D, pool.Q, count, seed=SEED)
        assert ei.value.code == fe.E_UNCORRECTABLE
        want = np.zeros(count, np.uint8)
        want[[1, 9]] = 1
        want[4] = 2
        assert np.array_equal(ei.value.status, want)
        hd, hq, guards = pool.contents()
        assert guards
        for b in range(count):
            if b == 4:  # fastecc_correct leaves an uncorrectable stripe untouched
                assert np.array_equal(hd[b], d[b]) and np.array_equal(hq[b], p[b])
            else:
                assert np.array_equal(hd[b], pool.d[b]) and np.array_equal(hq[b], pool.p[b])
        ok = enc.verify_batch(pool.D, pool.Q, count, seed=SEED)
        assert ok.tolist() == [b != 4 for b in range(count)]


def _refused(fe, enc, D, Q, count, want):
    for fn in (fe.lib().fastecc_verify_batch, fe.lib().fastecc_correct_batch):
        out = (ctypes.c_uint8 * count)(*([7] * count))
        inc = ctypes.c_uint64(12345)
        assert fn(enc._h, D.data_ptr(), Q.data_ptr(), count, None, SEED, out, ctypes.byref(inc)) == want, fn.__name__
        assert list(out) == [7] * count and inc.value == 12345


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
    with fe.Encoder(32, 16, 64) as enc:  # invalid arguments on a real context
        D, Q = torch.zeros(count * 16 * 16 + 4, dtype=torch.int32, device="cuda:0"), torch.zeros(count * 16 * 16 + 4, dtype=torch.int32, device="cuda:0")
        for fn in (fe.lib().fastecc_verify_batch, fe.lib().fastecc_correct_batch):
            out = (ctypes.c_uint8 * 4)(*([7] * 4))
            inc = ctypes.c_uint64(12345)
            for dp, qp, c in ((D.data_ptr() + 2, Q.data_ptr(), count), (D.data_ptr(), Q.data_ptr(), 0), (D.data_ptr(), Q.data_ptr(), (1 << 64) - 1)):
                assert fn(enc._h, dp, qp, c, None, SEED, out, ctypes.byref(inc)) == fe.E_INVAL
            assert list(out) == [7] * 4 and inc.value == 12345


def test_stream_order(torch_cuda, fe):
    """encode and verify_batch on one non-blocking stream: the batch sees the encoded parity."""
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
            ok = enc.verify_batch(D, Q, count, seed=SEED, stream=h)
        assert ok.all()
