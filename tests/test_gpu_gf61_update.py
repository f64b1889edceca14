"""GPU tests (-m gpu) of the small writes over GF((2^61-1)^2): fastecc_gf61_update and fastecc_gf61_update_parity.

After an update the stripe and the parity must be bit-identical to what fastecc_encode gives for the new stripe (the encoder is pinned to the
oracle by tests/test_gpu_p61.py); for (2k,k) at few elements the parity is also checked against the oracle itself."""
import numpy as np
import pytest

from footprint import Banded

pytestmark = pytest.mark.gpu

P = (1 << 61) - 1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def fe(hip_lib):
    import fastecc_amd
    return fastecc_amd


@pytest.fixture(scope="module")
def orc61():
    import oracle
    return oracle.OracleP61()


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to("cuda:0")


def host(t):
    return t.cpu().numpy().view(np.uint64).copy()


def rand_words(rng, shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64)


def encoder(fe, n, k, elems):
    return fe.Encoder(n, k, 16 * elems, field=fe.FIELD_GF_P61_SQUARED)


def encoded(torch, enc, d):
    """(data, parity) on the device: the stripe d (numpy [k, 2 * elems]) and its parity by fastecc_encode"""
    data = to_dev(torch, d.reshape(-1))
    parity = torch.zeros((enc.n - enc.k) * (enc.block_bytes // 8), dtype=torch.int64, device="cuda:0")
    enc.encode(data, parity)
    torch.cuda.synchronize()
    return data, parity


# (2k,k); n = 4k / 8k; zero-extended and fewer parity blocks
CODES = [(4, 2), (16, 8), (128, 64), (16, 4), (32, 4), (64, 16), (7, 5), (20, 16), (37, 20), (1100, 1000)]
ELEMS = [1, 3, 64, 65, 4096]  # 3: ragged; 65: one past a wave's columns; 4096: 64 KB blocks (k <= 16 only)
SHAPES = [(n, k, e) for n, k in CODES for e in ELEMS if e < 4096 or k <= 16]


def counts_for(k):
    """one row, two, a full pass, two passes, three passes — where they fit"""
    return sorted(set(t for t in (1, 2, 16, 17, min(k, 40)) if t <= k))


@pytest.mark.parametrize("n,k,elems", SHAPES)
def test_update_equals_encode_of_the_new_stripe(torch_cuda, fe, orc61, n, k, elems):
    torch = torch_cuda
    W = 2 * elems
    rng = np.random.default_rng(n * 7 + k * 3 + elems)
    with encoder(fe, n, k, elems) as enc:
        d = rand_words(rng, (k, W))
        data, parity = encoded(torch, enc, d)
        for t in counts_for(k):
            blocks = [int(b) for b in rng.permutation(k)[:t]]
            new = rand_words(rng, (t, W))
            old_rows = d[blocks].copy()
            enc.gf61_update(data, parity, blocks, to_dev(torch, new.reshape(-1)))
            torch.cuda.synchronize()
            d[blocks] = new
            assert np.array_equal(host(data).reshape(k, W), d), t
            _, want = encoded(torch, enc, d)
            assert torch.equal(parity, want), "update t=%d" % t
            if n == 2 * k and elems <= 3:
                assert np.array_equal(host(parity).reshape(k, W), orc61.encode(d)), t
            # back to the old rows, from data held elsewhere
            enc.gf61_update_parity(parity, blocks, to_dev(torch, old_rows.reshape(-1)), old=to_dev(torch, new.reshape(-1)))
            d[blocks] = old_rows
            data.copy_(to_dev(torch, d.reshape(-1)))
            torch.cuda.synchronize()
            _, want = encoded(torch, enc, d)
            assert torch.equal(parity, want), "update_parity t=%d" % t


@pytest.mark.parametrize("n,k,elems", [(128, 64, 64), (37, 20, 3), (1100, 1000, 65), (64, 16, 1), (32, 4, 4096)])
def test_incremental_encode_from_zero(torch_cuda, fe, n, k, elems):
    """Zero parity, then gf61_update_parity(old=None) over all k blocks in uneven batches: the encode of the stripe."""
    torch = torch_cuda
    rng = np.random.default_rng(k + elems)
    with encoder(fe, n, k, elems) as enc:
        d = rand_words(rng, (k, 2 * elems))
        _, want = encoded(torch, enc, d)
        parity = torch.zeros_like(want)
        order = [int(b) for b in rng.permutation(k)]
        cuts = sorted(set([0, k] + [int(c) for c in rng.integers(1, k, size=5)]))
        for a, b in zip(cuts, cuts[1:]):
            batch = order[a:b]
            enc.gf61_update_parity(parity, batch, to_dev(torch, d[batch].reshape(-1)))
        torch.cuda.synchronize()
        assert torch.equal(parity, want)


@pytest.mark.parametrize("n,k,elems", [(128, 64, 65), (64, 16, 64), (1100, 1000, 3)])
def test_edge_words(torch_cuda, fe, n, k, elems):
    """t = 16, so that the six sums of an element see 16 maximal rows: every re and im word p - 1 in old and new; p - 1 / 0 alternating
    replaced by zeros; new == old."""
    torch = torch_cuda
    W = 2 * elems
    rng = np.random.default_rng(elems)
    t = 16
    blocks = [int(b) for b in rng.permutation(k)[:t]]
    with encoder(fe, n, k, elems) as enc:
        # every word p - 1: the differences of the rows that stay p - 1 are 0, those of the others anything
        d = np.full((k, W), P - 1, np.uint64)
        data, parity = encoded(torch, enc, d)
        new = rand_words(rng, (t, W))
        new[: t // 2] = P - 1
        enc.gf61_update(data, parity, blocks, to_dev(torch, new.reshape(-1)))
        d[blocks] = new
        _, want = encoded(torch, enc, d)
        assert torch.equal(parity, want) and np.array_equal(host(data).reshape(k, W), d)
        # zeros become p - 1 in all 16 rows: every difference is p - 1, the largest canonical word
        d = np.zeros((k, W), np.uint64)
        data, parity = encoded(torch, enc, d)
        new = np.full((t, W), P - 1, np.uint64)
        enc.gf61_update(data, parity, blocks, to_dev(torch, new.reshape(-1)))
        d[blocks] = new
        _, want = encoded(torch, enc, d)
        assert torch.equal(parity, want) and np.array_equal(host(data).reshape(k, W), d)
        # p - 1 / 0 alternating, replaced by zeros: differences 1 and 0
        d = np.zeros((k, W), np.uint64)
        d.reshape(-1)[::2] = P - 1
        data, parity = encoded(torch, enc, d)
        enc.gf61_update(data, parity, blocks, torch.zeros(t * W, dtype=torch.int64, device="cuda:0"))
        d[blocks] = 0
        _, want = encoded(torch, enc, d)
        assert torch.equal(parity, want) and np.array_equal(host(data).reshape(k, W), d)
        # new == old leaves the parity bit-unchanged
        before = parity.clone()
        enc.gf61_update(data, parity, blocks, to_dev(torch, d[blocks].reshape(-1)))
        enc.gf61_update_parity(parity, blocks, to_dev(torch, d[blocks].reshape(-1)), old=to_dev(torch, d[blocks].reshape(-1)))
        torch.cuda.synchronize()
        assert torch.equal(parity, before)


def test_two_streams_on_one_context(torch_cuda, fe):
    """Two non-blocking streams update different blocks of one stripe back to back; the library orders them (the table is built on the first)."""
    torch = torch_cuda
    n, k, elems = 2048, 1024, 256
    W = 2 * elems
    rng = np.random.default_rng(2)
    with encoder(fe, n, k, elems) as enc:
        d = rand_words(rng, (k, W))
        data, parity = encoded(torch, enc, d)
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        ba, bb = [3, 500, 1000], [7, 8, 900, 1023]
        keep = []
        for _ in range(2):  # (fresh new blocks every round; the tensors live until the streams are done)
            na, nb = rand_words(rng, (3, W)), rand_words(rng, (4, W))
            ta, tb = to_dev(torch, na.reshape(-1)), to_dev(torch, nb.reshape(-1))
            keep += [ta, tb]
            torch.cuda.synchronize()
            enc.gf61_update(data, parity, ba, ta, stream=sa.cuda_stream)
            enc.gf61_update(data, parity, bb, tb, stream=sb.cuda_stream)
        torch.cuda.synchronize()
        d[ba], d[bb] = na, nb
        _, want = encoded(torch, enc, d)
        assert torch.equal(parity, want) and np.array_equal(host(data).reshape(k, W), d)


# 64 elements: the issue's case (one column slice, 4096 parity blocks).  130 and 300 elements (3 and 5 slices): with 4096 parity blocks a wave's
# run is longer than one block on any device of up to 8192 resident waves — runs of 4 or 2, and of 6 or 3 blocks: the loop's even and odd exits.
@pytest.mark.parametrize("elems", [64, 130, 300])
def test_several_runs_per_column_slice(torch_cuda, fe, elems):
    torch = torch_cuda
    k = 1 << 12
    W = 2 * elems
    rng = np.random.default_rng(elems)
    with encoder(fe, 2 * k, k, elems) as enc:
        d = rand_words(rng, (k, W))
        data, parity = encoded(torch, enc, d)
        for t in (1, 33):
            blocks = [k - 1] + [int(b) for b in rng.permutation(k - 1)[: t - 1]]
            new = rand_words(rng, (t, W))
            enc.gf61_update(data, parity, blocks, to_dev(torch, new.reshape(-1)))
            d[blocks] = new
            _, want = encoded(torch, enc, d)
            assert torch.equal(parity, want) and np.array_equal(host(data).reshape(k, W), d), t


def test_refusals_leave_the_buffers_unchanged(torch_cuda, fe):
    torch = torch_cuda
    elems = 4
    W = 2 * elems
    rng = np.random.default_rng(5)

    def refused(enc, data, parity, blocks, code, new=None, shift=None):
        """shift = (argument, bytes): that pointer moved"""
        new = torch.zeros(max(len(blocks), 1) * W + 2, dtype=torch.int64, device="cuda:0") if new is None else new
        d0, p0 = data.clone(), parity.clone()
        ptr = {"data": data.data_ptr(), "parity": parity.data_ptr(), "new": new.data_ptr(), "old": new.data_ptr()}
        if shift:
            ptr[shift[0]] += shift[1]
        with pytest.raises(fe.FastEccError) as ei:
            enc.gf61_update(ptr["data"], ptr["parity"], blocks, ptr["new"])
        assert ei.value.code == code
        with pytest.raises(fe.FastEccError) as ei:
            enc.gf61_update_parity(ptr["parity"], blocks, ptr["new"], old=ptr["old"])
        assert ei.value.code == code
        torch.cuda.synchronize()
        assert torch.equal(data, d0) and torch.equal(parity, p0)

    with encoder(fe, 64, 32, elems) as enc:
        data, parity = encoded(torch, enc, rand_words(rng, (32, W)))
        refused(enc, data, parity, [3, 5, 3], fe.E_INVAL)   # duplicate
        refused(enc, data, parity, [1, 32], fe.E_INVAL)     # index >= k
        for which in ("parity", "new"):                     # not 8-byte aligned (data and old: one call each)
            refused(enc, data, parity, [1], fe.E_INVAL, shift=(which, 4))
        with pytest.raises(fe.FastEccError) as ei:
            enc.gf61_update(data.data_ptr() + 4, parity, [1], torch.zeros(W, dtype=torch.int64, device="cuda:0"))
        assert ei.value.code == fe.E_INVAL
        with pytest.raises(fe.FastEccError) as ei:
            enc.gf61_update_parity(parity, [1], torch.zeros(W, dtype=torch.int64, device="cuda:0"), old=data.data_ptr() + 4)
        assert ei.value.code == fe.E_INVAL
        # the 32-bit calls keep refusing this field
        d0, p0 = data.clone(), parity.clone()
        new = torch.zeros(W, dtype=torch.int64, device="cuda:0")
        with pytest.raises(fe.FastEccError) as ei:
            enc.update(data, parity, [1], new)
        assert ei.value.code == fe.E_UNSUPPORTED
        with pytest.raises(fe.FastEccError) as ei:
            enc.update_parity(parity, [1], new, old=new)
        assert ei.value.code == fe.E_UNSUPPORTED
        torch.cuda.synchronize()
        assert torch.equal(data, d0) and torch.equal(parity, p0)
    with fe.Encoder(64, 32, 16 * elems) as enc:  # a GF(0xFFF00001) context
        data, parity = to_dev(torch, rand_words(rng, 32 * W) % (1 << 31)), to_dev(torch, rand_words(rng, 32 * W) % (1 << 31))
        refused(enc, data, parity, [1], fe.E_UNSUPPORTED)


def test_count_zero_is_a_no_op(torch_cuda, fe):
    torch = torch_cuda
    with encoder(fe, 16, 8, 4) as enc:
        data, parity = encoded(torch, enc, rand_words(np.random.default_rng(0), (8, 8)))
        p0 = parity.clone()
        enc.gf61_update(data, parity, [], parity[:0])
        enc.gf61_update_parity(parity, [], parity[:0])
        torch.cuda.synchronize()
        assert torch.equal(parity, p0)


def test_the_profile_names_the_three_kernels(torch_cuda, fe):
    torch = torch_cuda
    rng = np.random.default_rng(9)
    with encoder(fe, 16, 8, 4) as enc:
        d = rand_words(rng, (8, 8))
        data, parity = encoded(torch, enc, d)
        enc.profile(True)
        enc.profile_reset()
        enc.gf61_update(data, parity, [1, 5], to_dev(torch, rand_words(rng, 16)))
        enc.gf61_update(data, parity, [2], to_dev(torch, rand_words(rng, 8)))
        torch.cuda.synchronize()
        prof = enc.profile_read()
        assert {name: v[1] for name, v in prof.items()} == {"gf61_update_table": 1, "gf61_update_delta": 2, "gf61_update_parity": 2}, prof


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("n,k,elems,t", [(37, 20, 3, 17), (16, 4, 65, 3), (128, 64, 64, 16)])
def test_guard_bands(torch_cuda, fe, n, k, elems, t, skew):
    """data, parity and the rows each as [front band | payload | back band], the payloads on a 16-byte boundary plus `skew` words: only the named
    data blocks and the parity payload change, nothing outside any payload does, and the rows are only read."""
    torch = torch_cuda
    W, m = 2 * elems, n - k
    rng = np.random.default_rng(n + elems + skew)
    d = rand_words(rng, (k, W))
    new, old_elsewhere = rand_words(rng, (t, W)), rand_words(rng, (t, W))
    blocks = [int(b) for b in rng.permutation(k)[:t]]
    with encoder(fe, n, k, elems) as enc:
        _, par0 = encoded(torch, enc, d)  # (fastecc_encode wants 16-byte alignment: the expectations come from aligned copies)
        after = d.copy()
        after[blocks] = new
        _, par1 = encoded(torch, enc, after)
        data = Banded(torch, d, 2, W, 11, skew_words=skew)
        parity = Banded(torch, host(par0).reshape(m, W), 2, W, 12, skew_words=skew)
        rows = Banded(torch, new, 2, W, 13, skew_words=skew).frozen()
        enc.gf61_update(data.ptr, parity.ptr, blocks, rows.ptr)
        torch.cuda.synchronize()
        for b, what in ((data, "data"), (parity, "parity"), (rows, "new rows")):
            b.check("gf61_update: " + what)
        rows.check_unchanged("gf61_update: new rows")
        assert np.array_equal(data.host(), after) and np.array_equal(parity.host(), host(par1).reshape(m, W))
        # the parity form, back to a stripe whose blocks `blocks` hold old_elsewhere
        olds = Banded(torch, new, 2, W, 14, skew_words=skew).frozen()
        news = Banded(torch, old_elsewhere, 2, W, 15, skew_words=skew).frozen()
        enc.gf61_update_parity(parity.ptr, blocks, news.ptr, old=olds.ptr)
        torch.cuda.synchronize()
        for b, what in ((parity, "parity"), (olds, "old rows"), (news, "new rows")):
            b.check("gf61_update_parity: " + what)
        olds.check_unchanged("gf61_update_parity: old rows")
        news.check_unchanged("gf61_update_parity: new rows")
        after[blocks] = old_elsewhere
        _, par2 = encoded(torch, enc, after)
        assert np.array_equal(parity.host(), host(par2).reshape(m, W))
