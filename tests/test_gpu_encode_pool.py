"""GPU tests (-m gpu) of fastecc_encode_pool: the parity of a pool of stripes, in every mode of option "encode_pool_kernel".

Every comparison is bit-exact.  The expected parity of a pool is fastecc_encode of each stripe on the same context (computed once per
configuration and shared by the modes); stripes 0 and count - 1 are also compared with the oracle's parity (tests/pool_model.Codec), so
the check is not only self-referential.  The pools are the smallest at which each mechanism can go wrong: a full and a partial last wave
per stripe, odd and short blocks and a misaligned pool (the matrix-core kernel must fall back), k no multiple of 8 (rows past the stripe's
end), 8 / 16 / 32 outputs per wave, more outputs than one sweep, a mixed-radix order, and the codes that leave the direct path."""
import numpy as np
import pytest

from pool_model import Codec

pytestmark = pytest.mark.gpu

P = 0xFFF00001
MIXED_RADIX = 1  # FASTECC_CODE_MIXED_RADIX
CANARY = 0xC0FFEE11
PAD = 16  # canary words on either side of the parity pool (64 bytes: the pool itself stays 8-byte aligned)
MODES = (0, 1, 2, 3)


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


# name: (n, k, S words, count, flags, transform order for the oracle, options set on the context)
POOLS = {
    "20_16_s64": (20, 16, 64, 67, 0, 0, {}),                 # one full wave per stripe
    "20_16_s100": (20, 16, 100, 67, 0, 0, {}),               # partial last wave
    "20_16_s99": (20, 16, 99, 5, 0, 0, {}),                  # odd S: the matrix-core kernel falls back
    "14_10": (14, 10, 64, 33, 0, 0, {}),                     # k not a multiple of 8
    "100_70": (100, 70, 20, 11, 0, 0, {}),                   # S < 64: falls back
    "100_60": (100, 60, 64, 9, 0, 0, {}),                    # 40 outputs: sweeps
    "48_32": (48, 32, 64, 40, 0, 0, {}),                     # 16 outputs
    "96_64": (96, 64, 128, 5, 0, 0, {}),                     # 32 outputs
    "72_48_mixed": (72, 48, 64, 16, MIXED_RADIX, 48, {}),    # mixed radix
    "64_32": (64, 32, 16, 33, 0, 0, {}),                     # (2k,k) with short blocks
    "32_8": (32, 8, 32, 24, 0, 0, {}),                       # n = 4k: stripe by stripe
    "20_16_transform": (20, 16, 64, 5, 0, 0, {"encode_direct_max": 0}),  # the transform path forced: stripe by stripe
    "64_32_transform": (64, 32, 16, 33, 0, 0, {"encode_direct_max": 0}),  # ... for (2k,k): the passes once over the whole pool
}


class Pool:
    """An encoder, a pool of stripes on the host and on the device, and its parity by fastecc_encode stripe by stripe (computed once)."""

    def __init__(self, torch, fe, n, k, S, count, flags=0, order=0, options=None, data=None, seed=0):
        self.torch, self.n, self.k, self.S, self.count, self.m = torch, n, k, S, count, n - k
        self.flags, self.order = flags, order
        self.enc = fe.Encoder(n, k, 4 * S, flags=flags)
        for name, value in (options or {}).items():
            self.enc.set_option(name, value)
        self.data = rand_words(np.random.default_rng(seed), (count, k, S)) if data is None else data
        self.dev = to_dev(torch, self.data.reshape(-1))
        self.want = self.loop_parity(self.dev)

    def loop_parity(self, dev):
        """[count, m, S]: fastecc_encode of each stripe of the device pool `dev`"""
        torch, ks, ms = self.torch, self.k * self.S, self.m * self.S
        out = torch.zeros(self.count * ms, dtype=torch.int32, device="cuda:0")
        for b in range(self.count):
            self.enc.encode(dev[b * ks:(b + 1) * ks], out[b * ms:(b + 1) * ms])
        torch.cuda.synchronize()
        return host(out).reshape(self.count, self.m, self.S)

    def parity_buffer(self, shift=0):
        """(whole tensor, view of the parity pool inside it): canaries all over, the pool `shift` words past an 8-byte aligned address"""
        torch, words = self.torch, self.count * self.m * self.S
        whole = to_dev(torch, np.full(PAD + shift + words + PAD, CANARY, np.uint32))
        return whole, whole[PAD + shift:PAD + shift + words]

    def check(self, whole, shift=0):
        """the parity pool inside `whole` is the expected one, the canaries and the data are as they were"""
        got = host(whole)
        words = self.count * self.m * self.S
        assert (got[:PAD + shift] == CANARY).all() and (got[PAD + shift + words:] == CANARY).all(), "canary words were written"
        assert np.array_equal(got[PAD + shift:PAD + shift + words].reshape(self.count, self.m, self.S), self.want)
        assert np.array_equal(host(self.dev), self.data.reshape(-1)), "the data pool was written"

    def profiled(self, mode, whole_view):
        """encode_pool under `mode` with profiling on: {scope: launches}"""
        self.enc.set_option("encode_pool_kernel", mode)
        self.enc.profile(True)
        self.enc.profile_reset()
        self.enc.encode_pool(self.dev, whole_view, self.count)
        self.torch.cuda.synchronize()
        prof = self.enc.profile_read()
        self.enc.profile(False)
        return prof

    def close(self):
        self.enc.close()


@pytest.fixture(scope="module")
def pools(torch_cuda, fe):
    made = {}

    def get(name):
        if name not in made:
            n, k, S, count, flags, order, options = POOLS[name]
            made[name] = Pool(torch_cuda, fe, n, k, S, count, flags, order, options, seed=sum(map(ord, name)))
        return made[name]

    yield get
    for p in made.values():
        p.close()


# ---- 1. equality ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(POOLS))
def test_pool_equals_loop_of_encode(torch_cuda, pools, name, mode):
    pool = pools(name)
    pool.enc.set_option("encode_pool_kernel", mode)
    whole, view = pool.parity_buffer()
    pool.enc.encode_pool(pool.dev, view, pool.count)
    torch_cuda.cuda.synchronize()
    pool.check(whole)


@pytest.mark.parametrize("name", list(POOLS))
def test_loop_of_encode_is_the_oracles_parity(pools, oracle, name):
    pool = pools(name)
    codec = Codec(oracle, pool.n, pool.k, pool.flags, pool.order)
    for b in (0, pool.count - 1):
        assert np.array_equal(pool.want[b], codec.parity(pool.data[b])), "stripe %d" % b


# ---- 2. which kernel ran ----
def scopes(prof):
    return {name: v[1] for name, v in prof.items() if name.startswith("encode_pool_")}


@pytest.mark.parametrize("name", ["20_16_s64", "48_32"])
def test_mode_2_runs_the_matrix_core_kernel_once(pools, name):
    pool = pools(name)
    whole, view = pool.parity_buffer()
    prof = pool.profiled(2, view)
    assert scopes(prof) == {"encode_pool_mfma": 1}, prof
    assert prof["encode_pool_mfma"][2] == pool.count * pool.n * pool.S * 4
    pool.check(whole)


@pytest.mark.parametrize("name", ["20_16_s64", "48_32"])
def test_mode_1_runs_the_valu_kernel_once(pools, name):
    pool = pools(name)
    whole, view = pool.parity_buffer()
    prof = pool.profiled(1, view)
    assert scopes(prof) == {"encode_pool_valu": 1}, prof
    assert prof["encode_pool_valu"][2] == pool.count * pool.n * pool.S * 4
    pool.check(whole)


def test_mode_2_on_odd_blocks_falls_back_to_the_valu_kernel(pools):
    pool = pools("20_16_s99")
    whole, view = pool.parity_buffer()
    assert scopes(pool.profiled(2, view)) == {"encode_pool_valu": 1}
    pool.check(whole)


def test_mode_3_keeps_the_single_stripe_scope(pools):
    pool = pools("20_16_s64")
    whole, view = pool.parity_buffer()
    prof = pool.profiled(3, view)
    assert scopes(prof) == {} and prof["direct_encode"][1] == pool.count, prof
    pool.check(whole)


@pytest.mark.parametrize("n,k,S,count", [(20, 16, 64, 4096), (24, 16, 64, 2048)])
def test_mode_0_takes_one_launch_from_1024_waves_on(torch_cuda, fe, oracle, n, k, S, count):
    """the VALU launch of these pools has exactly 1024 waves (4 resp. 2 words per lane): mode 0 runs one batched launch, whichever kernel"""
    pool = Pool(torch_cuda, fe, n, k, S, count, seed=n)
    try:
        codec = Codec(oracle, n, k)
        for b in (0, count - 1):
            assert np.array_equal(pool.want[b], codec.parity(pool.data[b])), "stripe %d" % b
        whole, view = pool.parity_buffer()
        prof = pool.profiled(0, view)
        assert sorted(scopes(prof).values()) == [1] and "direct_encode" not in prof, prof
        pool.check(whole)
    finally:
        pool.close()


def test_mode_0_below_1024_waves_goes_stripe_by_stripe(pools):
    pool = pools("20_16_s64")
    whole, view = pool.parity_buffer()
    prof = pool.profiled(0, view)
    assert scopes(prof) == {} and prof["direct_encode"][1] == pool.count, prof
    pool.check(whole)


# ---- 3. saturated inputs ----
@pytest.fixture(scope="module")
def saturated(torch_cuda, fe):
    made = {}

    def get(n, k, S):
        if (n, k) not in made:
            data = np.full((3, k, S), P - 1, np.uint32)
            if k > 16:  # the edge of the k < 4096 digit bound: all p - 1, alternating 0 / p - 1, random
                data[1].reshape(-1)[::2] = 0
                data[2] = rand_words(np.random.default_rng(4090), (k, S))
            made[(n, k)] = Pool(torch_cuda, fe, n, k, S, 3, data=data)
        return made[(n, k)]

    yield get
    for p in made.values():
        p.close()


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("n,k,S", [(4094, 4090, 64), (20, 16, 64)])
def test_saturated_inputs(saturated, oracle, n, k, S, mode):
    pool = saturated(n, k, S)
    codec = Codec(oracle, n, k)
    for b in range(3):
        assert np.array_equal(pool.want[b], codec.parity(pool.data[b])), "stripe %d" % b
    whole, view = pool.parity_buffer()
    assert scopes(pool.profiled(mode, view)) == {"encode_pool_mfma" if mode == 2 else "encode_pool_valu": 1}
    pool.check(whole)


# ---- 4. alignment ----
def test_misaligned_parity_falls_back(pools):
    pool = pools("20_16_s64")
    whole, view = pool.parity_buffer(shift=1)  # 4 bytes past an 8-byte aligned address
    assert view.data_ptr() % 8 == 4
    assert scopes(pool.profiled(2, view)) == {"encode_pool_valu": 1}
    pool.check(whole, shift=1)


# ---- 5. refusals with a device ----
def refused(torch, fe, enc, rc_want, words_d, words_p, count=2, parity_at=None):
    """the call returns rc_want and leaves both buffers as they were; parity_at: the parity pointer as a word offset into the data buffer"""
    rng = np.random.default_rng(3)
    d, p = rand_words(rng, words_d), rand_words(rng, words_p)
    D, Q = to_dev(torch, d), to_dev(torch, p)
    torch.cuda.synchronize()
    parity = Q.data_ptr() if parity_at is None else D.data_ptr() + 4 * parity_at
    rc = fe.lib().fastecc_encode_pool(enc._h, D.data_ptr(), parity, count, None)
    assert rc == rc_want, rc
    torch.cuda.synchronize()
    assert np.array_equal(host(D), d) and np.array_equal(host(Q), p)


def test_refusals(torch_cuda, fe):
    torch = torch_cuda
    N, S = 16, 64
    with fe.Encoder(2 * N, N, 16 * 8, field=fe.FIELD_GF_P61_SQUARED) as enc:  # GF((2^61-1)^2)
        refused(torch, fe, enc, fe.E_UNSUPPORTED, 2 * N * 32, 2 * N * 32)
    with fe.ShardedEncoder(2 * N, N, 4 * S, [0, 0]) as enc:  # sharded, both slabs on device 0
        refused(torch, fe, enc, fe.E_UNSUPPORTED, 2 * N * S, 2 * N * S)
    with fe.Encoder(20, 16, 4 * S) as enc:
        dw, pw = 2 * 16 * S, 2 * 4 * S
        refused(torch, fe, enc, fe.E_INVAL, dw, pw, count=0)
        refused(torch, fe, enc, fe.E_INVAL, dw, pw, count=(1 << 64) - 1)  # byte sizes beyond 64 bits
        refused(torch, fe, enc, fe.E_INVAL, dw, pw, parity_at=0)          # in place
        refused(torch, fe, enc, fe.E_INVAL, dw, pw, parity_at=dw - S)     # the parity pool begins in the last data block
        refused(torch, fe, enc, fe.E_INVAL, dw, pw, parity_at=dw // 2)    # ... and where the data pool's second stripe begins
        for bad in (-1, 4):
            with pytest.raises(fe.FastEccError) as e:
                enc.set_option("encode_pool_kernel", bad)
            assert e.value.code == fe.E_INVAL
        enc.set_option("row_pitch_words", S + 32)
        refused(torch, fe, enc, fe.E_UNSUPPORTED, 2 * 16 * (S + 32), 2 * 4 * (S + 32))


def test_parity_pool_may_end_where_the_data_pool_begins(torch_cuda, fe):
    """adjacent is not overlapping: one buffer, parity pool first, data pool right behind it"""
    torch = torch_cuda
    n, k, S, count = 20, 16, 64, 3
    pw = count * (n - k) * S
    with fe.Encoder(n, k, 4 * S) as enc:
        data = rand_words(np.random.default_rng(8), (count, k, S))
        buf = to_dev(torch, np.concatenate([np.zeros(pw, np.uint32), data.reshape(-1)]))
        enc.set_option("encode_pool_kernel", 2)
        enc.encode_pool(buf[pw:], buf[:pw], count)
        want = torch.zeros(pw, dtype=torch.int32, device="cuda:0")
        for b in range(count):
            enc.encode(buf[pw + b * k * S:pw + (b + 1) * k * S], want[b * (n - k) * S:(b + 1) * (n - k) * S])
        torch.cuda.synchronize()
        got = host(buf)
        assert np.array_equal(got[:pw], host(want)) and np.array_equal(got[pw:], data.reshape(-1))


# ---- 6. lifecycle ----
@pytest.mark.parametrize("mode", [1, 2])
def test_pool_verifies_and_follows_updates(torch_cuda, pools, mode):
    torch, pool = torch_cuda, pools("20_16_s64")
    enc, k, S, count = pool.enc, pool.k, pool.S, pool.count
    enc.set_option("encode_pool_kernel", mode)
    D = pool.dev.clone()
    _, Q = pool.parity_buffer()
    enc.encode_pool(D, Q, count)
    assert enc.verify_batch(D, Q, count).all()
    rng = np.random.default_rng(17)
    writes = [0, 5 * k + 3, 5 * k + 9, (count - 1) * k + (k - 1)]
    new = to_dev(torch, rand_words(rng, (len(writes), S)))
    enc.update_batch(D, Q, count, writes, new)
    _, Q2 = pool.parity_buffer()
    enc.encode_pool(D, Q2, count)
    torch.cuda.synchronize()
    data = pool.data.copy().reshape(count * k, S)
    data[writes] = host(new).reshape(len(writes), S)
    assert np.array_equal(host(D), data.reshape(-1))
    assert np.array_equal(host(Q), host(Q2))
    assert enc.verify_batch(D, Q, count).all()


# ---- 7. streams ----
def test_two_streams_first_call_builds_the_tables(torch_cuda, fe):
    """the first call (it builds the weight fragments) on stream A, a second call with other data on stream B with nothing in between"""
    torch = torch_cuda
    n, k, S, count = 48, 32, 64, 40
    rng = np.random.default_rng(23)
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.set_option("encode_pool_kernel", 2)
        d = [rand_words(rng, (count, k, S)) for _ in range(2)]
        D = [to_dev(torch, x.reshape(-1)) for x in d]
        Q = [torch.zeros(count * (n - k) * S, dtype=torch.int32, device="cuda:0") for _ in range(2)]
        torch.cuda.synchronize()  # the buffers are the caller's business
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        enc.encode_pool(D[0], Q[0], count, stream=sa.cuda_stream)
        enc.encode_pool(D[1], Q[1], count, stream=sb.cuda_stream)
        torch.cuda.synchronize()
        for x, dev, q in zip(d, D, Q):
            want = torch.zeros_like(q)
            for b in range(count):
                enc.encode(dev[b * k * S:(b + 1) * k * S], want[b * (n - k) * S:(b + 1) * (n - k) * S])
            torch.cuda.synchronize()
            assert np.array_equal(host(q), host(want))
            assert np.array_equal(host(dev), x.reshape(-1))
