"""GPU tests (-m gpu) of batched erasure decoding: fastecc_decode_batch and fastecc_repair_batch.

The codewords come from the library's own single-stripe encode (pinned to the reference by the other suites).  A batch must give back the
original stripes bit for bit, and exactly what a loop of fastecc_decode / fastecc_repair over the same erased stripes gives, through both
the one-launch kernel (option decode_batch_kernel = 1) and the stripe-by-stripe form (= 2).  Nothing outside the erased blocks is written:
not the survivors, not (decode_batch) the erased parity blocks, not the guard stripe after the last one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 0xFFF00001
GARBAGE = 0xFFFFFFFF  # what an erased block holds before the call (not even a field element)
GUARD = 0x5A5A5A5A    # the stripe after the last one of a batch


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


def codewords(torch, enc, d):
    """parity [count, n - k, S] of the stripes d [count, k, S], one fastecc_encode per stripe"""
    count, k, S = d.shape
    m = enc.n - enc.k
    data = to_dev(torch, d)
    parity = torch.zeros(count * m * S, dtype=torch.int32, device="cuda:0")
    for b in range(count):
        enc.encode(data.data_ptr() + b * k * S * 4, parity.data_ptr() + b * m * S * 4)
    torch.cuda.synchronize()
    return host(parity).reshape(count, m, S)


def flags(k, m, lost_data, lost_parity):
    dp, pp = np.ones(k, np.uint8), np.ones(m, np.uint8)
    dp[list(lost_data)] = 0
    pp[list(lost_parity)] = 0
    return dp, pp


def run(torch, enc, d, p, dp, pp, op, how, stream=0):
    """Erase (GARBAGE), run `op` ("decode" / "repair") as one batch or as a loop of single-stripe calls; -> data, parity on the host.
    The buffers hold one guard stripe more, which must come back unchanged."""
    count, k, S = d.shape
    m = p.shape[1]
    dbuf = np.full((count + 1, k, S), GUARD, np.uint32)
    pbuf = np.full((count + 1, m, S), GUARD, np.uint32)
    dbuf[:count], pbuf[:count] = d, p
    dbuf[:count, dp == 0] = GARBAGE
    pbuf[:count, pp == 0] = GARBAGE
    D, Q = to_dev(torch, dbuf), to_dev(torch, pbuf)
    torch.cuda.synchronize()
    if how == "batch":
        getattr(enc, op + "_batch")(D, Q, count, stream=stream)
    else:
        for b in range(count):
            getattr(enc, op)(D.data_ptr() + b * k * S * 4, Q.data_ptr() + b * m * S * 4, stream=stream)
    torch.cuda.synchronize()
    gd, gp = host(D).reshape(count + 1, k, S), host(Q).reshape(count + 1, m, S)
    assert (gd[count] == GUARD).all() and (gp[count] == GUARD).all(), "guard stripe written"
    return gd[:count], gp[:count]


def check(torch, enc, d, p, dp, pp, modes=(1, 2)):
    """decode_batch and repair_batch == the single-stripe loop == the original, for each decode_batch_kernel mode"""
    for op in ("decode", "repair"):
        want_d, want_p = run(torch, enc, d, p, dp, pp, op, "loop")
        assert np.array_equal(want_d, d), "single-stripe %s" % op
        expect_p = p.copy()
        if op == "decode":
            expect_p[:, pp == 0] = GARBAGE  # decode leaves erased parity alone
        assert np.array_equal(want_p, expect_p), "single-stripe %s parity" % op
        for mode in modes:
            enc.set_option("decode_batch_kernel", mode)
            got_d, got_p = run(torch, enc, d, p, dp, pp, op, "batch")
            assert np.array_equal(got_d, want_d), "%s_batch data, mode %d" % (op, mode)
            assert np.array_equal(got_p, want_p), "%s_batch parity, mode %d" % (op, mode)
    enc.set_option("decode_batch_kernel", 0)


# (n, k, flags): (2k,k) at k = 2, 16, 128, 1024; n = k + N/2; zero extension (14,10), (20,16); n = 4k; mixed radix k = 96
CODES = [(4, 2, 0), (32, 16, 0), (256, 128, 0), (2048, 1024, 0), (24, 16, 0), (14, 10, 0), (20, 16, 0), (64, 16, 0), (128, 96, 1)]
WORDS = [1, 8, 33, 64, 1024]
COUNTS = [1, 3, 257]
MAX_WORDS = 1 << 23  # data words of one case (32 MiB): the largest combinations are left out


def matrix():
    for n, k, fl in CODES:
        for S in WORDS:
            for count in COUNTS:
                if count * k * S <= MAX_WORDS:
                    yield n, k, fl, S, count


@pytest.mark.parametrize("n,k,fl,S,count", list(matrix()))
def test_batch_equals_loop_equals_original(torch_cuda, fe, n, k, fl, S, count):
    torch = torch_cuda
    m = n - k
    rng = np.random.default_rng(n * 1000 + S * 7 + count)
    with fe.Encoder(n, k, 4 * S, flags=fl) as enc:
        d = rand_words(rng, (count, k, S))
        p = codewords(torch, enc, d)
        dp, pp = flags(k, m, rng.permutation(k)[:min(2, m - 1)], rng.permutation(m)[:1])  # data and parity lost
        enc.decode_prepare(dp, pp)
        check(torch, enc, d, p, dp, pp)


# every pass shape of the direct path: (n, k, lost data, lost parity)
SHAPES = {
    "data_only": (256, 128, 3, 0),           # direct_data
    "parity_only": (256, 128, 0, 3),         # decode: nothing to do; repair: direct_parity
    "both_one_pass": (256, 128, 5, 4),       # direct_both (<= 32 lost in all)
    "two_passes": (256, 128, 20, 20),        # direct_data, then direct_parity on the repaired data
    "sweeps_256": (512, 256, 200, 56),       # 200 outputs: 13 sweeps of 16
    "sweeps_both": (256, 128, 17, 9),        # 26 outputs in the single pass: 2 sweeps
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_pass_shapes(torch_cuda, fe, shape):
    torch = torch_cuda
    n, k, ld, lp = SHAPES[shape]
    m, S, count = n - k, 64, 5
    rng = np.random.default_rng(len(shape) * 31 + ld)
    with fe.Encoder(n, k, 4 * S) as enc:
        d = rand_words(rng, (count, k, S))
        p = codewords(torch, enc, d)
        dp, pp = flags(k, m, rng.permutation(k)[:ld], rng.permutation(m)[:lp])
        enc.decode_prepare(dp, pp)
        check(torch, enc, d, p, dp, pp, modes=(0, 1, 2))


def test_transform_path_runs_stripe_by_stripe(torch_cuda, fe):
    torch = torch_cuda
    n, k, S, count = 256, 128, 64, 6
    rng = np.random.default_rng(5)
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.set_option("decode_direct_max", 0)
        d = rand_words(rng, (count, k, S))
        p = codewords(torch, enc, d)
        dp, pp = flags(k, k, rng.permutation(k)[:40], rng.permutation(k)[:30])
        enc.decode_prepare(dp, pp)
        check(torch, enc, d, p, dp, pp, modes=(0, 1, 2))


@pytest.mark.parametrize("kind", ["all_p_minus_1", "alternating"])
def test_adversarial_words(torch_cuda, fe, kind):
    """128 data rows, 16 outputs: the 96-bit accumulators near their largest sums"""
    torch = torch_cuda
    n, k, S, count = 256, 128, 64, 4
    with fe.Encoder(n, k, 4 * S) as enc:
        if kind == "all_p_minus_1":
            d = np.full((count, k, S), P - 1, np.uint32)
        else:
            d = np.zeros((count, k, S), np.uint32)
            d.reshape(-1)[::2] = P - 1
        p = codewords(torch, enc, d)
        # lost parity only: repair's pass reads exactly the 128 data rows and writes 16 outputs
        dp, pp = flags(k, k, [], range(3, 3 + 16 * 7, 7))
        enc.decode_prepare(dp, pp)
        check(torch, enc, d, p, dp, pp)
        # 16 lost data rows: 144 rows (128 data, 16 parity nodes), 16 outputs
        dp, pp = flags(k, k, range(1, 1 + 16 * 5, 5), [])
        enc.decode_prepare(dp, pp)
        check(torch, enc, d, p, dp, pp)


def test_two_streams(torch_cuda, fe):
    torch = torch_cuda
    n, k, S, count = 64, 32, 256, 40
    rng = np.random.default_rng(11)
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.set_option("decode_batch_kernel", 1)
        dp, pp = flags(k, k, [0, 9, 31], [4])
        bufs = []
        for _ in range(2):
            d = rand_words(rng, (count, k, S))
            p = codewords(torch, enc, d)
            D, Q = d.copy(), p.copy()
            D[:, dp == 0] = GARBAGE
            Q[:, pp == 0] = GARBAGE
            bufs.append((d, p, to_dev(torch, D), to_dev(torch, Q)))
        enc.decode_prepare(dp, pp)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        enc.repair_batch(bufs[0][2], bufs[0][3], count, stream=s1.cuda_stream)
        enc.decode_batch(bufs[1][2], bufs[1][3], count, stream=s2.cuda_stream)
        torch.cuda.synchronize()
        d, p, D, Q = bufs[0]
        assert np.array_equal(host(D).reshape(count, k, S), d)
        assert np.array_equal(host(Q).reshape(count, k, S), p)
        d, p, D, Q = bufs[1]
        assert np.array_equal(host(D).reshape(count, k, S), d)
        want = p.copy()
        want[:, pp == 0] = GARBAGE
        assert np.array_equal(host(Q).reshape(count, k, S), want)


def refused(torch, fe, enc, rc_want, words_d, words_p, count=2, prepare=None, offset=0, raw_count=None):
    """the call returns rc_want and leaves both buffers as they were"""
    rng = np.random.default_rng(3)
    d, p = rand_words(rng, words_d), rand_words(rng, words_p)
    D, Q = to_dev(torch, d), to_dev(torch, p)
    torch.cuda.synchronize()
    for fn in (fe.lib().fastecc_decode_batch, fe.lib().fastecc_repair_batch):
        rc = fn(enc._h, D.data_ptr() + offset, Q.data_ptr(), count if raw_count is None else raw_count, None)
        assert rc == rc_want, (fn.__name__, rc)
    torch.cuda.synchronize()
    assert np.array_equal(host(D), d.reshape(-1)) and np.array_equal(host(Q), p.reshape(-1))


def test_refusals(torch_cuda, fe):
    torch = torch_cuda
    N, S = 16, 64
    # GF((2^61-1)^2): unsupported, with a prepared pattern
    with fe.Encoder(2 * N, N, 16 * 8, field=fe.FIELD_GF_P61_SQUARED) as enc:
        enc.decode_prepare([0] + [1] * (N - 1), [1] * N)
        refused(torch, fe, enc, fe.E_UNSUPPORTED, 2 * N * 32, 2 * N * 32)
    # sharded: unsupported
    with fe.ShardedEncoder(2 * N, N, 4 * S, [0, 0]) as enc:
        enc.decode_prepare([0] + [1] * (N - 1), [1] * N)
        refused(torch, fe, enc, fe.E_UNSUPPORTED, 2 * N * S, 2 * N * S)
    with fe.Encoder(2 * N, N, 4 * S) as enc:
        refused(torch, fe, enc, fe.E_INVAL, 2 * N * S, 2 * N * S)  # no prepared pattern
        enc.decode_prepare([0] + [1] * (N - 1), [1] * N)
        refused(torch, fe, enc, fe.E_INVAL, 2 * N * S, 2 * N * S, raw_count=0)  # count 0
        refused(torch, fe, enc, fe.E_INVAL, 2 * N * S, 2 * N * S, offset=2)     # misaligned
        refused(torch, fe, enc, fe.E_INVAL, 2 * N * S, 2 * N * S, raw_count=(1 << 64) - 1)  # byte sizes beyond 64 bits
        enc.set_option("row_pitch_words", S + 32)  # (drops the prepared pattern; the pitch is checked first)
        refused(torch, fe, enc, fe.E_UNSUPPORTED, 2 * N * (S + 32), 2 * N * (S + 32))


# random configurations: code, block size, count, pattern, kernel option
RANDOM_CODES = [(8, 4, 0), (64, 32, 0), (512, 256, 0), (24, 16, 0), (40, 32, 0), (14, 10, 0), (37, 20, 0), (64, 16, 0), (64, 8, 0), (128, 96, 1)]


@pytest.mark.parametrize("seed", range(20))
def test_random_configurations(torch_cuda, fe, seed):
    torch = torch_cuda
    rng = np.random.default_rng(1000 + seed)
    n, k, fl = RANDOM_CODES[int(rng.integers(len(RANDOM_CODES)))]
    m = n - k
    S, count, mode = int(rng.integers(1, 80)), int(rng.integers(1, 40)), int(rng.integers(0, 3))
    t = int(rng.integers(1, m + 1))
    ld = int(rng.integers(0, t + 1))
    ld, lp = min(ld, k), t - min(ld, k)
    with fe.Encoder(n, k, 4 * S, flags=fl) as enc:
        if seed % 5 == 4:
            enc.set_option("decode_direct_max", 0)  # the transform path
        d = rand_words(rng, (count, k, S))
        p = codewords(torch, enc, d)
        dp, pp = flags(k, m, rng.permutation(k)[:ld], rng.permutation(m)[:lp])
        enc.decode_prepare(dp, pp)
        check(torch, enc, d, p, dp, pp, modes=(mode,))
