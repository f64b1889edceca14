"""GPU test (-m gpu): ONE context carried through erasure patterns that change which part of its decoder state serves them.

The direct path's facts (which passes a pattern takes, how many blocks it lost) are read from tables that an earlier pattern also wrote, and
the transform path's tables sit next to them: a (128,64) code goes through patterns that use only the table for both, only the data table,
only the parity table, a data pass followed by a parity pass, the transform path (decode_direct_max = 0) with data and parity lost, nothing
lost, only parity lost, and the direct path again.  After every decode_prepare each call form runs on freshly damaged copies — lost blocks
hold words >= p — inside canary rows: decode and repair on device and on host memory, decode_batch and repair_batch over three stripes with
both values of decode_batch_kernel, and read_batch of a lost and a present data block of every stripe.  Every result is the original data
(repairs: and the original parity), everything a call must not write is what it was, and a read under a transform-path pattern that lost
blocks is refused with E_UNSUPPORTED.  Blocks of 33 words take the one-word form of the row kernels, blocks of 64 words the four-word form."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 0xFFF00001
CANARY = 0x5A5A5A5A
N, K, M, COUNT = 128, 64, 64, 3


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def fe(hip_lib):
    import fastecc_amd
    return fastecc_amd


PATTERN_A = ([5, 40], [7])
STEPS = [  # (name, decode_direct_max to set first or None, lost data blocks, lost parity blocks)
    ("a: table for both", None, *PATTERN_A),
    ("b: data table", None, [0, 31, 63], []),
    ("c: parity table", None, [], [0, 63]),
    ("d: data pass, parity pass", None, list(range(2, 62, 3)), list(range(1, 61, 3))),
    ("e: transform path, data and parity", 0, *PATTERN_A),
    ("f: nothing lost", None, [], []),
    ("g: transform path, parity only", None, [], [3, 50]),
    ("h: direct path again", 256, *PATTERN_A),
]


def codewords(oracle, S):
    """COUNT codewords [COUNT, K, S] / [COUNT, M, S]: seeded data, parity from the oracle"""
    rng = np.random.default_rng(1000 + S)
    data = rng.integers(0, P, size=(COUNT, K, S), dtype=np.uint64).astype(np.uint32)
    parity = np.stack([oracle.encode_fast(data[b]) for b in range(COUNT)]).astype(np.uint32)
    return data, parity


def framed(stripes):
    """the stripes back to back with a canary row before and after: (the whole buffer, the view of the stripes)"""
    count, rows, S = stripes.shape
    buf = np.full((count * rows + 2, S), CANARY, np.uint32)
    buf[1:-1] = stripes.reshape(count * rows, S)
    return buf, buf[1:-1].reshape(count, rows, S)


def damaged(orig, lost, seed):
    """a copy of the stripes whose lost blocks hold words >= p"""
    out = orig.copy()
    if lost:
        rng = np.random.default_rng(seed)
        out[:, lost] = rng.integers(P, 1 << 32, size=(orig.shape[0], len(lost), orig.shape[2]), dtype=np.uint64).astype(np.uint32)
    return out


class Case:
    """one call's buffers: damaged copies of the first `count` codewords inside canary rows, on the device or on the host"""

    def __init__(self, torch, data, parity, ld, lp, count, seed, host=False):
        self.torch, self.host, self.count = torch, host, count
        self.data0, self.parity0 = data[:count], parity[:count]
        self.bad_d, self.bad_p = damaged(self.data0, ld, seed), damaged(self.parity0, lp, seed + 1)
        bufs = [framed(self.bad_d), framed(self.bad_p)]
        if host:
            (self.dbuf, self.d), (self.pbuf, self.p) = bufs
        else:
            up = [torch.from_numpy(b.view(np.int32)).to("cuda:0") for b, _ in bufs]
            self.dbuf, self.pbuf = up
            self.d, self.p = up[0][1:-1], up[1][1:-1]
            torch.cuda.synchronize()

    def _host(self, buf):
        if self.host:
            return buf
        self.torch.cuda.synchronize()
        return buf.cpu().numpy().view(np.uint32)

    def check(self, what, parity_rebuilt):
        dbuf, pbuf = self._host(self.dbuf), self._host(self.pbuf)
        S = dbuf.shape[1]
        assert np.array_equal(dbuf[1:-1], self.data0.reshape(-1, S)), what + ": the data is the original"
        want_p = self.parity0 if parity_rebuilt else self.bad_p
        assert np.array_equal(pbuf[1:-1], want_p.reshape(-1, S)), what + (": the parity is the original" if parity_rebuilt else ": the parity is not written")
        for buf in (dbuf, pbuf):
            assert (buf[0] == CANARY).all() and (buf[-1] == CANARY).all(), what + ": canary rows"


@pytest.mark.parametrize("S", [33, 64])
def test_one_context_through_every_part(torch_cuda, fe, oracle, S):
    torch = torch_cuda
    data, parity = codewords(oracle, S)
    with fe.Encoder(N, K, 4 * S, device=0) as enc:
        direct_max = 256  # the library's default: every pattern below goes the direct path until step e
        for step, (name, set_max, ld, lp) in enumerate(STEPS):
            if set_max is not None:
                enc.set_option("decode_direct_max", set_max)
                direct_max = set_max
            transform_path = direct_max == 0
            dp, pp = np.ones(K, np.uint8), np.ones(M, np.uint8)
            dp[ld] = 0
            pp[lp] = 0
            enc.decode_prepare(dp, pp)
            seed = 100 * step + S

            for host in (False, True):
                mem = fe.MEM_HOST if host else fe.MEM_DEVICE
                where = "%s, %s memory" % (name, "host" if host else "device")
                c = Case(torch, data, parity, ld, lp, 1, seed, host)
                enc.decode(c.d[0], c.p[0], mem=mem)
                c.check(where + ", decode", parity_rebuilt=False)
                c = Case(torch, data, parity, ld, lp, 1, seed + 2, host)
                enc.repair(c.d[0], c.p[0], mem=mem)
                c.check(where + ", repair", parity_rebuilt=True)

            for kernel in (1, 2):
                enc.set_option("decode_batch_kernel", kernel)
                where = "%s, decode_batch_kernel %d" % (name, kernel)
                c = Case(torch, data, parity, ld, lp, COUNT, seed + 4)
                enc.decode_batch(c.d, c.p, COUNT)
                c.check(where + ", decode_batch", parity_rebuilt=False)
                c = Case(torch, data, parity, ld, lp, COUNT, seed + 6)
                enc.repair_batch(c.d, c.p, COUNT)
                c.check(where + ", repair_batch", parity_rebuilt=True)
            enc.set_option("decode_batch_kernel", 0)

            # one lost (where the pattern lost data) and one present data block of each stripe
            present = next(i for i in range(K) if i not in ld)
            blocks = ([ld[-1]] if ld else [K - 1 - present]) + [present]
            reads = np.array([b * K + i for b in range(COUNT) for i in blocks], np.uint64)
            c = Case(torch, data, parity, ld, lp, COUNT, seed + 8)
            out = torch.full((len(reads) + 2, S), CANARY, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            if transform_path and (ld or lp):
                with pytest.raises(fe.FastEccError) as refused:
                    enc.read_batch(c.d, c.p, COUNT, reads, out[1:].data_ptr())
                assert refused.value.code == fe.E_UNSUPPORTED, name + ", read_batch"
                got_rows = 0
            else:
                enc.read_batch(c.d, c.p, COUNT, reads, out[1:].data_ptr())
                got_rows = len(reads)
            torch.cuda.synchronize()
            got = out.cpu().numpy().view(np.uint32)
            assert np.array_equal(got[1:1 + got_rows], data.reshape(-1, S)[reads.astype(np.int64)][:got_rows]), name + ", read_batch: the original blocks"
            assert (got[0] == CANARY).all() and (got[1 + got_rows:] == CANARY).all(), name + ", read_batch: canary rows"
            dbuf, pbuf = c._host(c.dbuf), c._host(c.pbuf)
            assert np.array_equal(dbuf[1:-1], c.bad_d.reshape(-1, S)) and np.array_equal(pbuf[1:-1], c.bad_p.reshape(-1, S)), name + ", read_batch: the pool is not written"
