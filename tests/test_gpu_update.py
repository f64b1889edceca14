"""GPU tests (-m gpu) of the parity update for small writes: fastecc_update and fastecc_update_parity.

After an update the stripe and the parity must be bit-identical to what fastecc_encode gives for the new stripe (the encoder is pinned to
the reference by the other suites); for (2k,k) the parity is also checked against the oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 0xFFF00001


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


def rand_words(rng, shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64).astype(np.uint32)


def encoded(torch, enc, d):
    """parity of the stripe d (numpy [k, S]) by fastecc_encode"""
    data = to_dev(torch, d.reshape(-1))
    parity = torch.zeros((enc.n - enc.k) * (enc.block_bytes // 4), dtype=torch.int32, device="cuda:0")
    enc.encode(data, parity)
    torch.cuda.synchronize()
    return data, parity


# (n, k, flags): (2k,k); n = k + N/4; 4k; 8k; zero-extended; mixed radix 3 * 2^5; PFA 21 * 2^3; the top-radix-2 form of (2k,k)
CODES = [(16, 8, 0), (128, 64, 0), (64 + 16, 64, 0), (4 * 16, 16, 0), (8 * 8, 8, 0), (37, 20, 0), (1100, 1000, 0), (96 + 40, 96, 1), (168 + 50, 168, 4),
         (1 << 13, 1 << 12, 2)]
BLOCK_BYTES = [4, 8, 12, 24, 4096, 4100]  # 8 and 24: S = 2 mod 4, the two-word kernels


def counts_for(k):
    return [t for t in (1, 2, 17, 40) if t <= k]  # 40: more than one pass of 16 rows


@pytest.mark.parametrize("block_bytes", BLOCK_BYTES)
@pytest.mark.parametrize("n,k,flags", CODES)
def test_update_equals_encode_of_the_new_stripe(torch_cuda, fe, oracle, n, k, flags, block_bytes):
    torch = torch_cuda
    S = block_bytes // 4
    rng = np.random.default_rng(n * 7 + k * 3 + S)
    with fe.Encoder(n, k, block_bytes, flags=flags) as enc:
        d = rand_words(rng, (k, S))
        data, parity = encoded(torch, enc, d)
        for t in counts_for(k):
            blocks = [int(b) for b in rng.permutation(k)[:t]]
            new = rand_words(rng, (t, S))
            # fastecc_update: the stripe takes the new blocks, the parity follows
            old_rows = d[blocks].copy()
            enc.update(data, parity, blocks, to_dev(torch, new.reshape(-1)))
            torch.cuda.synchronize()
            d[blocks] = new
            assert np.array_equal(host(data).reshape(k, S), d), t
            _, want = encoded(torch, enc, d)
            assert torch.equal(parity, want), "update t=%d" % t
            if flags == 0 and n == 2 * k:
                assert np.array_equal(host(parity).reshape(k, S), oracle.encode(d)), t
            # fastecc_update_parity: back to the old blocks, from data held elsewhere
            enc.update_parity(parity, blocks, to_dev(torch, old_rows.reshape(-1)), old=to_dev(torch, new.reshape(-1)))
            d[blocks] = old_rows
            data.copy_(to_dev(torch, d.reshape(-1)))
            torch.cuda.synchronize()
            _, want = encoded(torch, enc, d)
            assert torch.equal(parity, want), "update_parity t=%d" % t


@pytest.mark.parametrize("n,k,flags,block_bytes", [(128, 64, 0, 4096), (37, 20, 0, 12), (96 + 40, 96, 1, 4100), (4 * 16, 16, 0, 4)])
def test_incremental_encode_from_zero(torch_cuda, fe, n, k, flags, block_bytes):
    """Zero parity, then update_parity(old=None) over all k blocks in uneven batches: the encode of the stripe."""
    torch = torch_cuda
    S = block_bytes // 4
    rng = np.random.default_rng(k + S)
    with fe.Encoder(n, k, block_bytes, flags=flags) as enc:
        d = rand_words(rng, (k, S))
        _, want = encoded(torch, enc, d)
        parity = torch.zeros_like(want)
        order = [int(b) for b in rng.permutation(k)]
        cuts = sorted(set([0, k] + [int(c) for c in rng.integers(1, k, size=5)]))
        for a, b in zip(cuts, cuts[1:]):
            batch = order[a:b]
            enc.update_parity(parity, batch, to_dev(torch, d[batch].reshape(-1)))
        torch.cuda.synchronize()
        assert torch.equal(parity, want)


@pytest.mark.parametrize("n,k,block_bytes", [(128, 64, 4096), (8 * 8, 8, 4100), (1100, 1000, 12)])
def test_adversarial_words(torch_cuda, fe, n, k, block_bytes):
    """The 96-bit lazy sums at their extremes: every word p - 1, p - 1 / 0 alternating replaced by zeros, and new == old."""
    torch = torch_cuda
    S = block_bytes // 4
    rng = np.random.default_rng(S)
    t = min(k, 40)
    blocks = [int(b) for b in rng.permutation(k)[:t]]
    with fe.Encoder(n, k, block_bytes) as enc:
        # every word p - 1, old and new
        d = np.full((k, S), P - 1, np.uint32)
        data, parity = encoded(torch, enc, d)
        new = rand_words(rng, (t, S))
        new[: t // 2] = P - 1
        enc.update(data, parity, blocks, to_dev(torch, new.reshape(-1)))
        d[blocks] = new
        _, want = encoded(torch, enc, d)
        assert torch.equal(parity, want) and np.array_equal(host(data).reshape(k, S), d)
        # p - 1 / 0 alternating, replaced by zeros
        d = np.zeros((k, S), np.uint32)
        d.reshape(-1)[::2] = P - 1
        data, parity = encoded(torch, enc, d)
        enc.update(data, parity, blocks, torch.zeros(t * S, dtype=torch.int32, device="cuda:0"))
        d[blocks] = 0
        _, want = encoded(torch, enc, d)
        assert torch.equal(parity, want) and np.array_equal(host(data).reshape(k, S), d)
        # new == old leaves the parity bit-unchanged
        before = parity.clone()
        enc.update(data, parity, blocks, to_dev(torch, d[blocks].reshape(-1)))
        enc.update_parity(parity, blocks, to_dev(torch, d[blocks].reshape(-1)), old=to_dev(torch, d[blocks].reshape(-1)))
        torch.cuda.synchronize()
        assert torch.equal(parity, before)


def test_two_streams_on_one_context(torch_cuda, fe):
    """Two non-blocking streams update different blocks of one stripe back to back; the library orders them."""
    torch = torch_cuda
    n, k, S = 2048, 1024, 1024
    rng = np.random.default_rng(2)
    with fe.Encoder(n, k, 4 * S) as enc:
        d = rand_words(rng, (k, S))
        data, parity = encoded(torch, enc, d)
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        ba, bb = [3, 500, 1000], [7, 8, 900, 1023]
        keep = []
        for _ in range(2):  # (fresh new blocks every round; the tensors live until the streams are done)
            na, nb = rand_words(rng, (3, S)), rand_words(rng, (4, S))
            ta, tb = to_dev(torch, na.reshape(-1)), to_dev(torch, nb.reshape(-1))
            keep += [ta, tb]
            torch.cuda.synchronize()
            enc.update(data, parity, ba, ta, stream=sa.cuda_stream)
            enc.update(data, parity, bb, tb, stream=sb.cuda_stream)
        torch.cuda.synchronize()
        d[ba], d[bb] = na, nb
        _, want = encoded(torch, enc, d)
        assert torch.equal(parity, want) and np.array_equal(host(data).reshape(k, S), d)


def test_refusals_leave_the_buffers_unchanged(torch_cuda, fe):
    torch = torch_cuda
    S = 16
    rng = np.random.default_rng(5)

    def refused(enc, data, parity, blocks, code, mem=fe.MEM_DEVICE, new=None):
        new = torch.zeros(max(len(blocks), 1) * S, dtype=torch.int32, device="cuda:0") if new is None else new
        d0 = data.clone() if hasattr(data, "clone") else data.copy()
        p0 = parity.clone() if hasattr(parity, "clone") else parity.copy()
        with pytest.raises(fe.FastEccError) as ei:
            enc.update(data, parity, blocks, new, mem=mem)
        assert ei.value.code == code
        with pytest.raises(fe.FastEccError) as ei:
            enc.update_parity(parity, blocks, new, old=new, mem=mem)
        assert ei.value.code == code
        if hasattr(data, "clone"):
            torch.cuda.synchronize()
            assert torch.equal(data, d0) and torch.equal(parity, p0)
        else:
            assert np.array_equal(data, d0) and np.array_equal(parity, p0)

    with fe.Encoder(64, 32, 4 * S) as enc:
        data, parity = encoded(torch, enc, rand_words(rng, (32, S)))
        refused(enc, data, parity, [3, 5, 3], fe.E_INVAL)   # duplicate
        refused(enc, data, parity, [1, 32], fe.E_INVAL)     # index >= k
        h = rand_words(rng, 32 * S)
        refused(enc, h, h.copy(), [1], fe.E_UNSUPPORTED, mem=fe.MEM_HOST, new=np.zeros(S, np.uint32))
    with fe.Encoder(64, 32, 64, field=fe.FIELD_GF_P61_SQUARED) as enc:
        buf = to_dev(torch, rand_words(rng, 32 * 16) % (1 << 31))
        refused(enc, buf, buf.clone(), [1], fe.E_UNSUPPORTED)
    with fe.ShardedEncoder(64, 32, 4 * S, [0, 0]) as enc:
        data, par = to_dev(torch, rand_words(rng, 32 * S)), to_dev(torch, rand_words(rng, 32 * S))
        refused(enc, data, par, [1], fe.E_UNSUPPORTED)
    with fe.Encoder(64, 32, 60) as enc:
        enc.set_option("row_pitch_words", 16)
        data, par = to_dev(torch, rand_words(rng, 32 * S)), to_dev(torch, rand_words(rng, 32 * S))
        refused(enc, data, par, [1], fe.E_UNSUPPORTED)


def test_count_zero_is_a_no_op(torch_cuda, fe):
    torch = torch_cuda
    with fe.Encoder(16, 8, 64) as enc:
        data, parity = encoded(torch, enc, rand_words(np.random.default_rng(0), (8, 16)))
        p0 = parity.clone()
        enc.update(data, parity, [], parity[:0])
        enc.update_parity(parity, [], parity[:0])
        torch.cuda.synchronize()
        assert torch.equal(parity, p0)
