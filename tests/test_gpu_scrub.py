"""GPU tests (-m gpu) of error detection and location: fastecc_verify, fastecc_locate_errors, fastecc_correct.

The expected answers come from the corruption the tests inject themselves and from the original codeword, which the library's
encoder produces (the encoder is pinned to the reference by the other suites).  Every comparison is bit-exact."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 0xFFF00001
SEED = 0x5EED


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
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")


def host(t):
    return t.cpu().numpy().view(np.uint32).copy()


def codeword(torch, fe, n, k, S, rng, fill=None, flags=0):
    """(encoder, data, parity) on the device; data words random < p with word 0 of every block < 2^20 (room for +p)."""
    enc = fe.Encoder(n, k, 4 * S, flags=flags)
    if fill is None:
        d = rng.integers(0, P, size=(k, S), dtype=np.uint64).astype(np.uint32)
        d[:, 0] = rng.integers(0, 1 << 20, size=k, dtype=np.uint32)
    else:
        d = np.full((k, S), fill, np.uint32)
    data = to_dev(torch, d.reshape(-1))
    parity = torch.zeros((n - k) * S, dtype=torch.int32, device="cuda:0")
    enc.encode(data, parity)
    torch.cuda.synchronize()
    return enc, data, parity


def corrupt(torch, data, parity, k, S, blocks, kind, rng):
    """Corrupt the given codeword blocks in place (numpy round trip of the whole stripes)."""
    d, p = host(data).reshape(k, S), host(parity).reshape(-1, S)
    for j in blocks:
        row = d[j] if j < k else p[j - k]
        w = int(rng.integers(S))
        if kind == "bitflip":
            bit = int(rng.integers(32)) if row[w] < (1 << 31) else int(rng.integers(20))  # stays a different word; may leave [0,p) (fine)
            row[w] ^= np.uint32(1 << bit)
        elif kind == "random":
            new = rng.integers(0, P, size=S, dtype=np.uint64).astype(np.uint32)
            new[0] = np.uint32((int(row[0]) + 1) % P)  # certainly different
            row[:] = new
        elif kind == "big":
            row[w] = np.uint32(P + int(rng.integers(0, (1 << 32) - P)))
        elif kind == "plus_p":
            small = np.nonzero(row < (1 << 20))[0]
            assert len(small), "no word < 2^20 in block %d" % j
            row[small[0]] += np.uint32(P)
        elif kind == "one_word":
            row[w] = np.uint32((int(row[w]) + 1 + int(rng.integers(P - 1))) % P)
        else:
            raise ValueError(kind)
    data.copy_(to_dev(torch, d.reshape(-1)))
    parity.copy_(to_dev(torch, p.reshape(-1)))
    torch.cuda.synchronize()


# (n, k, S): (2k,k), n = k + N/2^d, 4k / 8k, zero-extended
CODES = [(4, 2, 64), (8, 4, 32), (32, 16, 64), (64 + 16, 64, 32), (64 + 8, 64, 33), (4 * 16, 16, 16), (8 * 8, 8, 32), (130, 100, 16), (1100, 1000, 8)]


@pytest.mark.parametrize("logk", range(1, 17))
def test_clean_reference_code(torch_cuda, fe, logk):
    torch, rng = torch_cuda, np.random.default_rng(logk)
    k = 1 << logk
    S = 64 if logk <= 10 else 4
    enc, data, parity = codeword(torch, fe, 2 * k, k, S, rng)
    d0, p0 = data.clone(), parity.clone()
    assert enc.verify(data, parity, seed=SEED)
    assert enc.locate_errors(data, parity, seed=SEED) == []
    assert torch.equal(d0, data) and torch.equal(p0, parity)
    enc.close()


@pytest.mark.parametrize("n,k,S", CODES + [(1024 + 512, 1024, 16), (1024 + 64, 1024, 16), (1500, 1000, 8), (150, 100, 16), (4 * 256, 256, 8), (8 * 64, 64, 8)])
def test_clean_other_codes(torch_cuda, fe, n, k, S):
    torch, rng = torch_cuda, np.random.default_rng(n + k)
    enc, data, parity = codeword(torch, fe, n, k, S, rng)
    d0, p0 = data.clone(), parity.clone()
    assert enc.verify(data, parity, seed=SEED)
    assert enc.locate_errors(data, parity, seed=SEED + 1) == []
    assert enc.correct(data, parity, seed=SEED + 2) == []
    assert torch.equal(d0, data) and torch.equal(p0, parity)
    enc.close()


def _t_values(n, k, tmax):
    m = n - k
    ts = {1, 2, tmax}
    if m // 2 <= tmax:
        ts.add(m // 2)
    return sorted(t for t in ts if 1 <= t and 2 * t <= m)


# a constant stripe is a codeword of the codes without zero extension: the saturated case runs on those
CASES = [(n, k, S, kind) for (n, k, S) in CODES for kind in ("bitflip", "random", "big", "plus_p")] + \
        [(n, k, S, "one_word_saturated") for (n, k, S) in CODES if k & (k - 1) == 0]


@pytest.mark.parametrize("n,k,S,kind", CASES)
def test_locate_and_correct(torch_cuda, fe, n, k, S, kind):
    torch, rng = torch_cuda, np.random.default_rng(zlib.crc32(repr((n, k, S, kind)).encode()))
    tmax = 4
    saturated = kind == "one_word_saturated"
    for t in _t_values(n, k, tmax):
        enc, data, parity = codeword(torch, fe, n, k, S, rng, fill=P - 1 if saturated else None)
        enc.set_option("locate_max", tmax)
        d0, p0 = data.clone(), parity.clone()
        pool = np.arange(k) if kind == "plus_p" else np.arange(n)
        blocks = sorted(int(b) for b in rng.choice(pool, size=t, replace=False))
        if kind != "plus_p" and t >= 2 and not any(b >= k for b in blocks):
            blocks[-1] = int(k + rng.integers(n - k))  # mix data and parity
            blocks = sorted(set(blocks))
        corrupt(torch, data, parity, k, S, blocks, "one_word" if saturated else kind, rng)
        dc, pc = data.clone(), parity.clone()
        assert not enc.verify(data, parity, seed=SEED)
        assert enc.locate_errors(data, parity, seed=SEED) == blocks
        assert torch.equal(dc, data) and torch.equal(pc, parity)  # locate reads only
        assert enc.correct(data, parity, seed=SEED) == blocks
        torch.cuda.synchronize()
        assert torch.equal(d0, data) and torch.equal(p0, parity)
        assert enc.verify(data, parity, seed=SEED + 9)
        enc.close()


def test_saturated_reference_code_is_a_codeword(torch_cuda, fe):
    torch, rng = torch_cuda, np.random.default_rng(3)
    enc, data, parity = codeword(torch, fe, 64, 32, 16, rng, fill=P - 1)
    assert (host(parity) == P - 1).all()
    assert enc.verify(data, parity, seed=SEED)
    enc.close()


@pytest.mark.parametrize("n,k,S,b", [(32, 16, 64, 4), (32, 16, 64, 8), (80, 64, 32, 6), (130, 100, 16, 10)])
def test_known_erasures_plus_errors(torch_cuda, fe, n, k, S, b):
    """b blocks with a word >= p plus t other corrupted blocks, 2t + b = n - k."""
    torch, rng = torch_cuda, np.random.default_rng(b + n)
    t = (n - k - b) // 2
    enc, data, parity = codeword(torch, fe, n, k, S, rng)
    d0, p0 = data.clone(), parity.clone()
    chosen = [int(x) for x in rng.choice(n, size=b + t, replace=False)]
    corrupt(torch, data, parity, k, S, chosen[:b], "big", rng)
    corrupt(torch, data, parity, k, S, chosen[b:], "random", rng)
    assert not enc.verify(data, parity, seed=SEED)
    assert enc.locate_errors(data, parity, seed=SEED) == sorted(chosen)
    assert enc.correct(data, parity, seed=SEED) == sorted(chosen)
    torch.cuda.synchronize()
    assert torch.equal(d0, data) and torch.equal(p0, parity)
    enc.close()


def test_too_many_errors_uncorrectable_and_untouched(torch_cuda, fe):
    torch, rng = torch_cuda, np.random.default_rng(9)
    k, S = 1 << 12, 8
    enc, data, parity = codeword(torch, fe, 2 * k, k, S, rng)
    enc.set_option("locate_max", 8)
    blocks = sorted(int(x) for x in rng.choice(2 * k, size=9, replace=False))
    corrupt(torch, data, parity, k, S, blocks, "random", rng)
    dc, pc = data.clone(), parity.clone()
    for call in (enc.locate_errors, enc.correct):
        with pytest.raises(fe.FastEccError) as ei:
            call(data, parity, seed=SEED)
        assert ei.value.code == fe.E_UNCORRECTABLE
        torch.cuda.synchronize()
        assert torch.equal(dc, data) and torch.equal(pc, parity)
    enc.set_option("locate_max", 9)  # within reach now
    assert enc.locate_errors(data, parity, seed=SEED) == blocks
    enc.close()


def test_locate_max_option_range(fe):
    with fe.Encoder(16, 8, 64) as enc:
        enc.set_option("locate_max", 0)
        enc.set_option("locate_max", 4096)
        for bad in (-1, 4097):
            with pytest.raises(fe.FastEccError) as ei:
                enc.set_option("locate_max", bad)
            assert ei.value.code == fe.E_INVAL


def test_correct_parity_only_on_nonblocking_stream(torch_cuda, fe):
    """Only parity blocks corrupted, the transform path (device scan of the pattern), a torch stream: the lost-parity flags written by
    decode_prepare must be visible to the repair on that stream."""
    torch, rng = torch_cuda, np.random.default_rng(11)
    k, S = 1 << 10, 64
    enc, data, parity = codeword(torch, fe, 2 * k, k, S, rng)
    enc.set_option("decode_direct_max", 0)
    d0, p0 = data.clone(), parity.clone()
    for round_ in range(2):  # a second pattern: stale flags of the first would leave blocks unrepaired
        blocks = sorted(int(k + x) for x in rng.choice(k, size=3 + 2 * round_, replace=False))
        corrupt(torch, data, parity, k, S, blocks, "random", rng)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            got = enc.correct(data, parity, seed=SEED + round_, stream=s.cuda_stream)
        s.synchronize()
        assert got == blocks
        assert torch.equal(d0, data) and torch.equal(p0, parity)
    enc.close()


def test_same_seed_same_answer_and_decoder_still_works(torch_cuda, fe):
    torch, rng = torch_cuda, np.random.default_rng(12)
    n, k, S = 64, 32, 32
    enc, data, parity = codeword(torch, fe, n, k, S, rng)
    d0, p0 = data.clone(), parity.clone()
    blocks = [3, 40]
    corrupt(torch, data, parity, k, S, blocks, "bitflip", rng)
    a = enc.locate_errors(data, parity, seed=77)
    assert a == enc.locate_errors(data, parity, seed=77) == blocks
    assert enc.correct(data, parity, seed=77) == blocks
    torch.cuda.synchronize()
    assert torch.equal(d0, data) and torch.equal(p0, parity)
    # the context's decoder after correct replaced its pattern: a fresh prepare + decode
    dp, pp = np.ones(k, np.uint8), np.ones(n - k, np.uint8)
    dp[[0, 5, 9]] = 0
    for b in (0, 5, 9):
        data[b * S:(b + 1) * S].zero_()
    enc.decode_prepare(dp, pp)
    enc.decode(data, parity)
    torch.cuda.synchronize()
    assert torch.equal(d0, data)
    enc.close()


def test_headline_size_three_blocks(torch_cuda, fe):
    torch = torch_cuda
    k, S = 1 << 19, 1024
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(5)
    data = torch.randint(0, (1 << 31) - 1, (k * S,), dtype=torch.int32, device="cuda:0", generator=gen)
    parity = torch.empty_like(data)
    with fe.Encoder(2 * k, k, 4 * S) as enc:
        enc.encode(data, parity)
        torch.cuda.synchronize()
        assert enc.verify(data, parity, seed=SEED)
        blocks = [12345, k - 1, k + 777]
        saved = [(data if b < k else parity)[(b % k) * S:(b % k + 1) * S].clone() for b in blocks]
        data[12345 * S + 17] += 1
        data[(k - 1) * S: k * S] = 7
        parity[777 * S + 1000] ^= 1 << 30
        assert not enc.verify(data, parity, seed=SEED)
        assert enc.locate_errors(data, parity, seed=SEED) == blocks
        assert enc.correct(data, parity, seed=SEED) == blocks
        torch.cuda.synchronize()
        for b, want in zip(blocks, saved):
            assert torch.equal((data if b < k else parity)[(b % k) * S:(b % k + 1) * S], want)
        assert enc.verify(data, parity, seed=SEED + 1)


def test_unsupported_contexts(torch_cuda, fe):
    torch = torch_cuda
    buf = torch.zeros(64 * 64 * 4, dtype=torch.int32, device="cuda:0")
    def refused(enc, d, p, mem=fe.MEM_DEVICE):
        for call in (enc.verify, enc.locate_errors, enc.correct):
            with pytest.raises(fe.FastEccError) as ei:
                call(d, p, mem=mem)
            assert ei.value.code == fe.E_UNSUPPORTED
    with fe.Encoder(64, 32, 64, field=fe.FIELD_GF_P61_SQUARED) as enc:
        refused(enc, buf, buf)
    with fe.ShardedEncoder(64, 32, 256, [0, 0]) as enc:
        refused(enc, buf, buf)
    with fe.Encoder(64, 32, 60) as enc:
        enc.set_option("row_pitch_words", 16)
        refused(enc, buf, buf)
    with fe.Encoder(64, 32, 64) as enc:
        h = np.zeros(64 * 16, np.uint32)
        refused(enc, h, h, mem=fe.MEM_HOST)
        refused(enc, h, h, mem=fe.MEM_HOST_PINNED)
    with fe.Encoder(2 * 48, 48, 64, flags=fe.CODE_MIXED_RADIX) as enc:  # mixed radix: documented as unsupported
        refused(enc, buf, buf)
