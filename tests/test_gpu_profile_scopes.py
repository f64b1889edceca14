"""GPU tests (-m gpu) that pin who opens and closes the profile records and the buffer-ordering scopes of the decoder's entry points:
per call {scope name: (launches, algorithmic bytes)} as Encoder.profile_read() reports it after profile() / profile_reset().

The expected values were read from a run of the library as it stood BEFORE the decoder and the sharded code reached the context
directly (FASTECC_HIP_LIB pointed this file at that build); where the code states a formula it is written as one.  The file passes
unchanged on that build and on the current one: a scope that opens late, closes early, is counted twice or carries other bytes fails it.
Every case runs twice, with profiling on and off: off leaves profile_read() empty, and the results are the same bits either way (and
the right ones: the stripes are the library's own encode, damaged by the test)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 0xFFF00001
P61 = (1 << 61) - 1
NONE = 0xFFFFFFFF
BLOCK = 256  # bytes per block unless noted
TRANSFORM = ", decode_direct_max = 0"  # label of the 64-bit cases that take the transform path


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def fe(hip_lib):
    import fastecc_amd
    return fastecc_amd


class Pool:
    """`count` stripes of an (k + m, k) code back to back in device memory, encoded by `enc` itself; words of `dtype` (uint32, or uint64
    for the 64-bit field), `width` of them per block"""

    def __init__(self, torch, enc, k, m, width, dtype, seed, count=1, mem_host=False):
        self.torch, self.k, self.m, self.count = torch, k, m, count
        self.signed = np.int32 if dtype == np.uint32 else np.int64
        self.dtype = dtype
        rng = np.random.default_rng(seed)
        self.data = rng.integers(0, P if dtype == np.uint32 else P61, size=(count, k, width), dtype=np.uint64).astype(dtype)
        D = self.dev(self.data)
        Q = torch.zeros((count, m * width), dtype=D.dtype, device="cuda:0")
        for b in range(count):
            enc.encode(D[b], Q[b])
        torch.cuda.synchronize()
        self.parity = Q.cpu().numpy().view(dtype).reshape(count, m, width)

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).reshape(a.shape[0], -1).view(self.signed)).to("cuda:0")

    def damaged(self, lost_of):
        """device copies of the pool with the blocks lost_of(b) = (data blocks, parity blocks) of stripe b overwritten"""
        d, p = self.data.copy(), self.parity.copy()
        for b in range(self.count):
            ld, lp = lost_of(b)
            d[b, list(ld)] = self.dtype(~self.dtype(0))
            p[b, list(lp)] = self.dtype(~self.dtype(0))
        return self.dev(d), self.dev(p), p

    def host(self, t, like):
        self.torch.cuda.synchronize()
        return t.cpu().numpy().view(self.dtype).reshape(like.shape)


def aligned_copy(a):
    """a host copy of `a` on a 64-byte boundary (the 64-bit field's stripes are 16-byte aligned)"""
    buf = np.empty(a.nbytes + 64, np.uint8)
    off = (-buf.ctypes.data) % 64
    out = buf[off:off + a.nbytes].view(a.dtype).reshape(a.shape)
    out[...] = a
    return out


def presence(k, m, lost_data, lost_parity):
    return [i not in lost_data for i in range(k)], [j not in lost_parity for j in range(m)]


class Recorder:
    """runs the calls of a scenario with profiling on or off: records[label] = {scope: (launches, bytes)} of that call alone,
    results = what the scenario handed over for the bit-for-bit comparison of the two runs"""

    def __init__(self, on):
        self.on, self.records, self.results = on, {}, []

    def call(self, enc, label, fn):
        enc.profile(self.on)
        enc.profile_reset()
        try:
            fn()
        finally:
            prof = enc.profile_read(cap=128)
            enc.profile(False)
        self.records[label] = {name: (v[1], v[2]) for name, v in prof.items()}

    def keep(self, *arrays):
        self.results += [np.array(a) for a in arrays]


def run_both_ways(scenario, expected):
    on, off = Recorder(True), Recorder(False)
    scenario(on)
    scenario(off)
    for label, rec in on.records.items():
        print("%s: %r" % (label, rec))  # (the figures before they are judged: pytest -s)
    assert on.records == expected
    assert off.records == {label: {} for label in expected}
    assert len(on.results) == len(off.results) and all(np.array_equal(a, b) for a, b in zip(on.results, off.results))


def test_direct_path(torch_cuda, fe):
    """(16,8), data block 3 and parity block 5 lost: one pass over the survivors serves decode and repair alike (at most 32 outputs:
    the table for both), and the record's bytes are the k rows read and the lost data block written"""
    k, m = 8, 8

    def scenario(r):
        with fe.Encoder(k + m, k, BLOCK) as enc:
            pool = Pool(torch_cuda, enc, k, m, BLOCK // 4, np.uint32, 1)
            enc.decode_prepare(*presence(k, m, {3}, {5}))
            d, q, bad_p = pool.damaged(lambda b: ({3}, {5}))
            r.call(enc, "decode", lambda: enc.decode(d[0], q[0]))
            got_d, got_q = pool.host(d, pool.data), pool.host(q, pool.parity)
            assert np.array_equal(got_d, pool.data) and np.array_equal(got_q, bad_p)
            r.keep(got_d, got_q)
            d, q, _ = pool.damaged(lambda b: ({3}, {5}))
            r.call(enc, "repair", lambda: enc.repair(d[0], q[0]))
            got_d, got_q = pool.host(d, pool.data), pool.host(q, pool.parity)
            assert np.array_equal(got_d, pool.data) and np.array_equal(got_q, pool.parity)
            r.keep(got_d, got_q)

    one_pass = {"direct_pass": (1, (k + 1) * BLOCK)}
    run_both_ways(scenario, {"decode": one_pass, "repair": one_pass})


def test_transform_path(torch_cuda, fe):
    """(256,128) with "decode_direct_max" = 0, 40 data and 40 parity blocks lost, repair: the 2k-point transform under one record of
    3 N blocks, then the lost parity from one more encode, whose passes are the context's own records.  k = 2^7 is below the split
    transform's sizes, so "decode_split" = 0 and the default take the same form."""
    k = m = 128
    rng = np.random.default_rng(2)
    lost = rng.permutation(k)[:40]
    lost_d, lost_p = set(lost.tolist()), set(rng.permutation(m)[:40].tolist())

    def scenario(r):
        for label, split in (("repair", None), ("repair, decode_split = 0", 0)):
            with fe.Encoder(k + m, k, BLOCK) as enc:
                pool = Pool(torch_cuda, enc, k, m, BLOCK // 4, np.uint32, 3)
                enc.set_option("decode_direct_max", 0)
                if split is not None:
                    enc.set_option("decode_split", split)
                enc.decode_prepare(*presence(k, m, lost_d, lost_p))
                d, q, _ = pool.damaged(lambda b: (lost_d, lost_p))
                r.call(enc, label, lambda: enc.repair(d[0], q[0]))
                got_d, got_q = pool.host(d, pool.data), pool.host(q, pool.parity)
                assert np.array_equal(got_d, pool.data) and np.array_equal(got_q, pool.parity)
                r.keep(got_d, got_q)

    form = {"decode_transform_2k": (1, 3 * k * BLOCK), "direct_encode": (1, (k + m) * BLOCK)}  # (n - k <= 160: the encode is the direct one)
    run_both_ways(scenario, {"repair": form, "repair, decode_split = 0": form})


def test_batch_paths(torch_cuda, fe):
    """(20,16) x 8 stripes, data block 5 lost, repair_batch: "decode_batch_kernel" = 1 is one launch over the batch (per stripe the
    rows the pass reads and its one output), 2 is direct_run stripe by stripe under ONE record (per stripe k rows and the lost block)"""
    k, m, count = 16, 4, 8

    def scenario(r):
        with fe.Encoder(k + m, k, BLOCK) as enc:
            pool = Pool(torch_cuda, enc, k, m, BLOCK // 4, np.uint32, 4, count)
            enc.decode_prepare(*presence(k, m, {5}, set()))
            for mode in (1, 2):
                enc.set_option("decode_batch_kernel", mode)
                d, q, _ = pool.damaged(lambda b: ({5}, set()))
                r.call(enc, "decode_batch_kernel = %d" % mode, lambda: enc.repair_batch(d, q, count))
                got_d, got_q = pool.host(d, pool.data), pool.host(q, pool.parity)
                assert np.array_equal(got_d, pool.data) and np.array_equal(got_q, pool.parity)
                r.keep(got_d, got_q)

    rows = k + 1  # the k data rows (the lost one at weight 0) and the one parity row that stands in for it
    run_both_ways(scenario, {"decode_batch_kernel = 1": {"direct_pass_batch": (1, count * (rows + 1) * BLOCK)},
                             "decode_batch_kernel = 2": {"direct_pass": (1, count * (k + 1) * BLOCK)}})


def test_set_path(torch_cuda, fe):
    """(20,16) x 8 stripes, pattern 0 (data block 2 lost) and pattern 1 (data block 7 and parity block 1 lost) in turn and one stripe
    PATTERN_NONE, repair_batch_set: a record per pad class that has work; per stripe the rows its pass reads and the blocks it writes"""
    k, m, count = 16, 4, 8
    patterns = [({2}, set()), ({7}, {1})]
    pattern_of = [0, 1, 0, 1, NONE, 0, 1, 0]

    def lost_of(b):
        return patterns[pattern_of[b]] if pattern_of[b] != NONE else (set(), set())

    def scenario(r):
        with fe.Encoder(k + m, k, BLOCK) as enc:
            pool = Pool(torch_cuda, enc, k, m, BLOCK // 4, np.uint32, 5, count)
            flags = [presence(k, m, *p) for p in patterns]
            enc.decode_prepare_set([f[0] for f in flags], [f[1] for f in flags])
            for mode in (1, 2):
                enc.set_option("decode_batch_kernel", mode)
                d, q, _ = pool.damaged(lost_of)
                r.call(enc, "decode_batch_kernel = %d" % mode, lambda: enc.repair_batch_set(d, q, count, pattern_of))
                got_d, got_q = pool.host(d, pool.data), pool.host(q, pool.parity)
                assert np.array_equal(got_d, pool.data) and np.array_equal(got_q, pool.parity)
                r.keep(got_d, got_q)

    # pattern 0: k + 1 rows read, 1 block written (pad 1); pattern 1: k + 1 rows read, 2 written (pad 2): two classes, a record each
    moved = 4 * (k + 1 + 1) * BLOCK, 3 * (k + 1 + 2) * BLOCK
    run_both_ways(scenario, {"decode_batch_kernel = 1": {"direct_pass_set": (2, sum(moved))},
                             "decode_batch_kernel = 2": {"direct_pass": (2, sum(moved))}})


def p61_scenario(torch, fe, r, k, m, elems, lost_d, lost_p, seed):
    with fe.Encoder(k + m, k, 16 * elems, field=fe.FIELD_GF_P61_SQUARED) as enc:
        pool = Pool(torch, enc, k, m, 2 * elems, np.uint64, seed)
        for suffix in ("", TRANSFORM):
            if suffix:
                enc.set_option("decode_direct_max", 0)
            enc.decode_prepare(*presence(k, m, lost_d, lost_p))
            for label, call in (("decode", enc.decode), ("repair", enc.repair)):
                d, q, bad_p = pool.damaged(lambda b: (lost_d, lost_p))
                r.call(enc, label + suffix, lambda: call(d[0], q[0]))
                got_d, got_q = pool.host(d, pool.data), pool.host(q, pool.parity)
                assert np.array_equal(got_d, pool.data) and np.array_equal(got_q, pool.parity if label == "repair" else bad_p)
                r.keep(got_d, got_q)


def test_64_bit_field(torch_cuda, fe):
    """(32,16) over GF((2^61-1)^2) with 64-byte blocks, data block 9 lost.  The 64-bit field's few-loss path launches outside the
    launch hooks and records nothing; with "decode_direct_max" = 0 the same pattern takes the transform path, whose launches are one
    record each through the hooks"""
    run_both_ways(lambda r: p61_scenario(torch_cuda, fe, r, 16, 16, 4, {9}, set(), 6), EXPECTED_P61)


def test_64_bit_field_zero_extended(torch_cuda, fe):
    """(6,5) with 48-byte blocks, the smallest zero-extended 64-bit code the suite builds, in device memory, data block 2 lost: the same
    decoder on the padded (16,8) codeword in the context's work stripes (the copies in and out are not launches)"""
    run_both_ways(lambda r: p61_scenario(torch_cuda, fe, r, 5, 1, 3, {2}, set(), 7), EXPECTED_P61_ZERO_EXTENDED)


def test_64_bit_field_unsupported_host_call_leaves_the_context_in_order(torch_cuda, fe):
    """The same zero-extended code: a decode from host memory is FASTECC_E_UNSUPPORTED after the call has ordered the internal
    buffers, and must leave them marked: a decode on a second stream directly after it (the work stripes still in use by the decode
    before, on the first stream) gives the right data.  Both forms of the decoder; the refused call records nothing."""
    torch = torch_cuda
    k, m, elems = 5, 1, 3
    sequence = "decode, refused host decode, decode on a second stream"

    def scenario(r):
        with fe.Encoder(k + m, k, 16 * elems, field=fe.FIELD_GF_P61_SQUARED) as enc:
            pool = Pool(torch, enc, k, m, 2 * elems, np.uint64, 8)
            second = torch.cuda.Stream()
            for suffix in ("", TRANSFORM):
                if suffix:
                    enc.set_option("decode_direct_max", 0)
                enc.decode_prepare(*presence(k, m, {2}, set()))
                first_d, first_q, _ = pool.damaged(lambda b: ({2}, set()))
                d, q, _ = pool.damaged(lambda b: ({2}, set()))
                host_d, host_q = aligned_copy(pool.data[0]), aligned_copy(pool.parity[0])
                torch.cuda.synchronize()

                def calls():
                    enc.decode(first_d[0], first_q[0])
                    with pytest.raises(fe.FastEccError) as refused:
                        enc.decode(host_d, host_q, mem=fe.MEM_HOST)
                    assert refused.value.code == fe.E_UNSUPPORTED
                    enc.decode(d[0], q[0], stream=second.cuda_stream)

                r.call(enc, sequence + suffix, calls)
                got_first, got = pool.host(first_d, pool.data), pool.host(d, pool.data)
                assert np.array_equal(got_first, pool.data) and np.array_equal(got, pool.data)
                r.keep(got_first, got)

    def twice(rec):
        return {name: (2 * launches, 2 * nbytes) for name, (launches, nbytes) in rec.items()}

    run_both_ways(scenario, {sequence + suffix: twice(EXPECTED_P61_ZERO_EXTENDED["decode" + suffix]) for suffix in ("", TRANSFORM)})


def test_sharded_context(torch_cuda, fe):
    """A sharded context of two slabs on one device, (32,16), data block 4 and parity block 11 lost: encode, decode_prepare, repair;
    profile_read() through the shell reads the first slab's context, whose blocks are half as long"""
    k = m = 16
    slab = BLOCK // 2

    def scenario(r):
        with fe.ShardedEncoder(k + m, k, BLOCK, [0, 0]) as enc:
            rng = np.random.default_rng(9)
            data = rng.integers(0, P, size=(k, BLOCK // 4), dtype=np.uint64).astype(np.uint32)
            D = torch_cuda.from_numpy(data.reshape(-1).view(np.int32)).to("cuda:0")
            Q = torch_cuda.zeros(m * BLOCK // 4, dtype=torch_cuda.int32, device="cuda:0")
            r.call(enc, "encode", lambda: enc.encode(D, Q))
            torch_cuda.cuda.synchronize()
            parity = Q.cpu().numpy().view(np.uint32).reshape(m, -1)
            with fe.Encoder(k + m, k, BLOCK) as whole:  # (the slabs' parity is the column ranges of the one-device parity)
                Q1 = torch_cuda.zeros_like(Q)
                whole.encode(D, Q1)
                torch_cuda.cuda.synchronize()
                assert np.array_equal(Q1.cpu().numpy().view(np.uint32).reshape(m, -1), parity)
            enc.decode_prepare(*presence(k, m, {4}, {11}))
            bad_d, bad_p = data.copy(), parity.copy()
            bad_d[4] = 0xFFFFFFFF
            bad_p[11] = 0xFFFFFFFF
            d = torch_cuda.from_numpy(bad_d.reshape(-1).view(np.int32)).to("cuda:0")
            q = torch_cuda.from_numpy(bad_p.reshape(-1).view(np.int32)).to("cuda:0")
            r.call(enc, "repair", lambda: enc.repair(d, q))
            torch_cuda.cuda.synchronize()
            got_d, got_q = d.cpu().numpy().view(np.uint32).reshape(k, -1), q.cpu().numpy().view(np.uint32).reshape(m, -1)
            assert np.array_equal(got_d, data) and np.array_equal(got_q, parity)
            r.keep(parity, got_d, got_q)

    run_both_ways(scenario, {"encode": {"direct_encode": (1, (k + m) * slab)}, "repair": {"direct_pass": (1, (k + 1) * slab)}})


# The records of the 64-bit field's decoder are its kernels' own names and byte counts (gf61_decode.hip, gf61_kernels.hip), which this file
# does not restate as formulas: literals from the run named in the head comment.
EXPECTED_P61 = {"decode": {}, "repair": {}, "decode" + TRANSFORM: {"p61_tile_mid5": (1, 4096)}, "repair" + TRANSFORM: {"p61_tile_mid5": (1, 4096)}}
EXPECTED_P61_ZERO_EXTENDED = {"decode": {}, "repair": {}, "decode" + TRANSFORM: {"p61_mid4": (1, 1536)},
                              "repair" + TRANSFORM: {"p61_mid4": (1, 1536), "p61_mid3": (1, 768)}}
