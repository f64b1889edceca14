"""GPU tests (-m gpu) of the batched small writes: fastecc_update_batch and fastecc_update_parity_batch on a pool of stripes.

Every comparison is bit-exact.  The expected data is the new pool built on the host; the expected parity of a touched stripe is
fastecc_encode of its new data (the single-stripe encoder is pinned to the reference by the other suites); an untouched stripe must
come back as it was, whatever it held.  The pools are the smallest at which each mechanism can fail: every code family, row lengths
below a wave, every vector width, more rounds than one, every segment length class."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 0xFFF00001
MIXED_RADIX, MIXED_RADIX_PFA = 1, 4  # FASTECC_CODE_MIXED_RADIX, FASTECC_CODE_MIXED_RADIX_PFA


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


def update_batch_from(fe, enc, data, parity, count, arr, new, stream):
    """fastecc_update_batch reading the caller's own host list (a numpy uint64 array; Encoder.update_batch copies its list)"""
    code = fe.lib().fastecc_update_batch(enc._h, data.data_ptr(), parity.data_ptr(), count, arr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(arr),
                                         new.data_ptr(), stream)
    assert code == 0, code


def rand_words(rng, shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64).astype(np.uint32)


# (n, k, S words, stripes, flags, one-word offset of the pool tensors)
POOLS = {
    "k+N/4": (20, 16, 64, 7, 0, 0),
    "zero-extended": (14, 10, 32, 5, 0, 0),
    "2k,k short rows": (32, 16, 16, 9, 0, 0),
    "odd S": (72, 64, 33, 3, 0, 0),
    "V=2": (24, 16, 6, 4, 0, 0),
    "4k": (64, 16, 16, 3, 0, 0),
    "8k": (64, 8, 32, 3, 0, 0),
    "zero-extended k>16": (130, 100, 16, 3, 0, 0),
    "mixed radix": (96, 48, 16, 3, MIXED_RADIX, 0),
    "PFA": (84, 42, 8, 2, MIXED_RADIX_PFA, 0),
    "misaligned base": (20, 16, 64, 4, 0, 1),
    "six stripes k=32": (40, 32, 8, 6, 0, 0),  # holds the segment lengths 1, 2, 3, 5, 16 and 17 in one call
}


class Pool:
    """An encoder, a random pool of stripes on the host and its parity (fastecc_encode stripe by stripe, computed once per module)."""

    def __init__(self, torch, fe, name):
        self.torch, self.name = torch, name
        self.n, self.k, self.S, self.B, flags, self.shift = POOLS[name]
        self.M = self.n - self.k
        self.enc = fe.Encoder(self.n, self.k, 4 * self.S, flags=flags)
        rng = np.random.default_rng(sum(map(ord, name)))
        self.data = rand_words(rng, (self.B, self.k, self.S))
        self.parity = np.stack([self.encode(self.data[b]) for b in range(self.B)])

    def encode(self, stripe):
        """parity [M, S] of one stripe [k, S] by fastecc_encode"""
        torch = self.torch
        out = torch.zeros(self.M * self.S, dtype=torch.int32, device="cuda:0")
        self.enc.encode(to_dev(torch, stripe.reshape(-1)), out)
        torch.cuda.synchronize()
        return host(out).reshape(self.M, self.S)

    def device(self, a):
        """the words of `a` in device memory, `shift` words past an aligned address"""
        t = self.torch.zeros(a.size + self.shift, dtype=self.torch.int32, device="cuda:0")
        t[self.shift:] = to_dev(self.torch, a.reshape(-1))
        return t[self.shift:]

    def close(self):
        self.enc.close()


@pytest.fixture(scope="module")
def pools(torch_cuda, fe):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Pool(torch_cuda, fe, name)
        return made[name]

    yield get
    for p in made.values():
        p.close()


def pattern(name, B, k, rng):
    """pool block indices b * k + i of a write pattern, sorted; None where the pool does not allow it"""
    def blocks(b, t):
        return [b * k + int(i) for i in rng.permutation(k)[:t]]
    if name == "one per stripe":
        w = [b * k + int(rng.integers(k)) for b in range(B)]
    elif name == "first and last stripe":
        w = blocks(0, min(k, 3)) + blocks(B - 1, 1)
    elif name == "every block of one stripe":  # k = 16: exactly one full pass; k >= 17: more than one round
        w = blocks(B // 2, k)
    elif name == "17 blocks in one stripe":    # crosses the pass boundary
        if k < 17:
            return None
        w = blocks(B - 1, 17)
    elif name == "every length class":         # 1, 2, 3, 5, 16, 17 writes in different stripes: every T and a second round in one call
        lens = [t for t in (17, 16, 5, 3, 2, 1) if t <= k][:B]
        w = sum([blocks(b, t) for b, t in enumerate(lens)], [])
    return sorted(w)


PATTERNS = ["one per stripe", "first and last stripe", "every block of one stripe", "17 blocks in one stripe", "every length class"]


def expect(pool, data, parity, writes, new):
    """(data, parity) of the pool after the writes: the host's scatter, and fastecc_encode of every touched stripe"""
    d, p = data.copy(), parity.copy()
    flat = d.reshape(pool.B * pool.k, pool.S)
    flat[writes] = new
    for b in sorted({w // pool.k for w in writes}):
        p[b] = pool.encode(d[b])
    return d, p


# every pattern on every pool whose k allows it
CASES = [(name, pat) for name in POOLS for pat in PATTERNS if pat != "17 blocks in one stripe" or POOLS[name][1] >= 17]


@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("name,pat", CASES)
def test_update_batch_equals_encode_of_the_touched_stripes(torch_cuda, pools, name, pat, order):
    torch = torch_cuda
    pool = pools(name)
    rng = np.random.default_rng(len(pat) * 131 + len(name))
    writes = pattern(pat, pool.B, pool.k, rng)
    if order == "shuffled":
        writes = [writes[i] for i in rng.permutation(len(writes))]
    data, parity = pool.data.copy(), pool.parity.copy()
    if pat == "first and last stripe":  # the stripes between hold no field elements at all: they must be neither read nor written
        data[1:-1] = 0xFFFFFFFF
        parity[1:-1] = 0xFFFFFFFF
    new = rand_words(rng, (len(writes), pool.S))
    want_d, want_p = expect(pool, data, parity, writes, new)
    dd, dp, dn = pool.device(data), pool.device(parity), to_dev(torch, new.reshape(-1))
    pool.enc.update_batch(dd, dp, pool.B, writes, dn)
    torch.cuda.synchronize()
    assert np.array_equal(host(dd).reshape(data.shape), want_d)
    got_p = host(dp).reshape(parity.shape)
    for b in range(pool.B):
        assert np.array_equal(got_p[b], want_p[b]), "parity of stripe %d" % b
    # the parity form, back to the old blocks from rows held elsewhere: the old parity again
    old_rows = data.reshape(pool.B * pool.k, pool.S)[writes]
    pool.enc.update_parity_batch(dp, pool.B, writes, to_dev(torch, old_rows.reshape(-1)), old=dn)
    torch.cuda.synchronize()
    assert np.array_equal(host(dp).reshape(parity.shape), parity)


@pytest.mark.parametrize("name", ["k+N/4", "odd S", "8k"])
def test_edge_values(torch_cuda, pools, name):
    """The edges of gf::sub / gf::add: old = p - 1 with new = 0 and the reverse, new == old, a stripe of all p - 1."""
    torch = torch_cuda
    pool = pools(name)
    B, k, S = pool.B, pool.k, pool.S
    rng = np.random.default_rng(B + k + S)
    writes = pattern("every length class", B, k, rng)
    t = len(writes)
    for old_word, new_word in ((P - 1, 0), (0, P - 1), (P - 1, P - 1)):
        data = pool.data.copy()
        data.reshape(B * k, S)[writes] = old_word
        data[0] = old_word  # a whole stripe of the edge value (all p - 1: the largest sums the lazy accumulators see)
        parity = np.stack([pool.encode(data[b]) for b in range(B)])
        new = np.full((t, S), new_word, np.uint32)
        want_d, want_p = expect(pool, data, parity, writes, new)
        dd, dp = pool.device(data), pool.device(parity)
        pool.enc.update_batch(dd, dp, B, writes, to_dev(torch, new.reshape(-1)))
        torch.cuda.synchronize()
        assert np.array_equal(host(dd).reshape(data.shape), want_d), (old_word, new_word)
        assert np.array_equal(host(dp).reshape(parity.shape), want_p), (old_word, new_word)
    # new == old (random words): not one bit of the parity changes
    same = pool.data.reshape(B * k, S)[writes]
    dd, dp = pool.device(pool.data), pool.device(pool.parity)
    pool.enc.update_batch(dd, dp, B, writes, to_dev(torch, same.reshape(-1)))
    pool.enc.update_parity_batch(dp, B, writes, to_dev(torch, same.reshape(-1)), old=to_dev(torch, same.reshape(-1)))
    torch.cuda.synchronize()
    assert np.array_equal(host(dd).reshape(pool.data.shape), pool.data)
    assert np.array_equal(host(dp).reshape(pool.parity.shape), pool.parity)


@pytest.mark.parametrize("name", ["zero-extended", "six stripes k=32", "mixed radix", "4k"])
def test_incremental_encode_from_zero(torch_cuda, pools, name):
    """A zeroed parity pool, then update_parity_batch(old=None) over all blocks of the pool in two calls, half each: the encode."""
    torch = torch_cuda
    pool = pools(name)
    B, k, S = pool.B, pool.k, pool.S
    rng = np.random.default_rng(k)
    order = [int(i) for i in rng.permutation(B * k)]
    dp = pool.device(np.zeros_like(pool.parity))
    rows = pool.data.reshape(B * k, S)
    for part in (order[: B * k // 2], order[B * k // 2:]):
        pool.enc.update_parity_batch(dp, B, part, to_dev(torch, rows[part].reshape(-1)))
    torch.cuda.synchronize()
    assert np.array_equal(host(dp).reshape(pool.parity.shape), pool.parity)


def test_parity_form_with_explicit_old_blocks(torch_cuda, pools):
    torch = torch_cuda
    pool = pools("zero-extended k>16")
    B, k, S = pool.B, pool.k, pool.S
    rng = np.random.default_rng(11)
    writes = [int(i) for i in rng.permutation(B * k)[:40]]
    new = rand_words(rng, (len(writes), S))
    _, want_p = expect(pool, pool.data, pool.parity, writes, new)
    dp = pool.device(pool.parity)
    pool.enc.update_parity_batch(dp, B, writes, to_dev(torch, new.reshape(-1)), old=to_dev(torch, pool.data.reshape(B * k, S)[writes].reshape(-1)))
    torch.cuda.synchronize()
    assert np.array_equal(host(dp).reshape(pool.parity.shape), want_p)


def test_equals_a_loop_of_update_per_stripe(torch_cuda, pools):
    torch = torch_cuda
    pool = pools("k+N/4")
    B, k, S, M = pool.B, pool.k, pool.S, pool.M
    rng = np.random.default_rng(12)
    writes = [int(i) for i in rng.permutation(B * k)[:30]]
    new = rand_words(rng, (len(writes), S))
    dd, dp = pool.device(pool.data), pool.device(pool.parity)
    pool.enc.update_batch(dd, dp, B, writes, to_dev(torch, new.reshape(-1)))
    ld, lp = pool.device(pool.data), pool.device(pool.parity)
    for b in range(B):
        mine = [u for u, w in enumerate(writes) if w // k == b]
        if mine:
            pool.enc.update(ld[b * k * S:(b + 1) * k * S], lp[b * M * S:(b + 1) * M * S], [writes[u] % k for u in mine], to_dev(torch, new[mine].reshape(-1)))
    torch.cuda.synchronize()
    assert torch.equal(dd, ld) and torch.equal(dp, lp)


def test_back_to_back_calls_on_a_stream_reuse_the_staging_buffer(torch_cuda, fe, pools):
    """Three calls on a non-blocking stream without a synchronise between them: the second rewrites blocks the first wrote and writes
    others in the same stripes, the third carries a longer list (the buffers grow); the host list is overwritten as soon as a call
    returns.  After one synchronise the pool equals the sequential result."""
    torch = torch_cuda
    pool = pools("k+N/4")
    B, k, S = pool.B, pool.k, pool.S
    rng = np.random.default_rng(13)
    first = [b * k + 3 for b in range(B)] + [5]
    second = [b * k + 3 for b in range(0, B, 2)] + [b * k + 7 for b in range(B)] + [6]
    # (the longest list of the three; this small pool cannot outgrow the buffers' first size: the next test does)
    third = [int(i) for i in rng.permutation(B * k)[: B * k - 5]]
    calls = [(w, rand_words(rng, (len(w), S))) for w in (first, second, third)]
    want_d, want_p = pool.data, pool.parity
    for w, new in calls:
        want_d, want_p = expect(pool, want_d, want_p, w, new)
    st = torch.cuda.Stream()
    dd, dp = pool.device(pool.data), pool.device(pool.parity)
    news = [to_dev(torch, new.reshape(-1)) for _, new in calls]
    torch.cuda.synchronize()
    for (w, _), dn in zip(calls, news):
        arr = np.array(w, dtype=np.uint64)
        update_batch_from(fe, pool.enc, dd, dp, B, arr, dn, st.cuda_stream)
        arr[:] = 0xFFFFFFFFFFFFFFFF  # the list may be reused as soon as the call returns
    torch.cuda.synchronize()
    assert np.array_equal(host(dd).reshape(pool.data.shape), want_d)
    assert np.array_equal(host(dp).reshape(pool.parity.shape), want_p)


def test_staging_buffers_grow_between_calls_on_a_stream(torch_cuda, fe):
    """(20,16) x 16 B x 1024 stripes: a call with 8 writes, then — no synchronise — one with 1024 (more than the buffers' first size holds)
    that rewrites the blocks of the first, then a short one again."""
    torch = torch_cuda
    n, k, S, B = 20, 16, 4, 1024
    rng = np.random.default_rng(14)
    st = torch.cuda.Stream()
    with fe.Encoder(n, k, 4 * S) as enc:
        data = torch.zeros(B * k * S, dtype=torch.int32, device="cuda:0")   # an all-zero pool is a pool of codewords
        parity = torch.zeros(B * (n - k) * S, dtype=torch.int32, device="cuda:0")
        lists = [[b * k + 2 for b in range(8)], [b * k + 2 for b in range(B)], [b * k + 9 for b in range(5)]]
        rows = np.zeros((B * k, S), np.uint32)
        news = []
        for w in lists:
            new = rand_words(rng, (len(w), S))
            rows[w] = new
            news.append(to_dev(torch, new.reshape(-1)))
        torch.cuda.synchronize()
        for w, dn in zip(lists, news):
            arr = np.array(w, dtype=np.uint64)
            update_batch_from(fe, enc, data, parity, B, arr, dn, st.cuda_stream)
            arr[:] = 0xFFFFFFFFFFFFFFFF
        torch.cuda.synchronize()
        assert np.array_equal(host(data).reshape(B * k, S), rows)
        want = torch.zeros_like(parity)
        for b in range(B):
            enc.encode(data[b * k * S:(b + 1) * k * S], want[b * (n - k) * S:(b + 1) * (n - k) * S])
        torch.cuda.synchronize()
        assert torch.equal(parity, want)


# Runs per segment.  The host gives a launch at least the device's resident waves where the parity count M allows it: with `segs` segments and
# `slices` column slices it asks for want = min(M, ceil(target / (segs * slices))) runs, target = 4 SIMDs x CUs x waves per SIMD (256 x 4 x 8 =
# 8192 on an MI355X for T <= 4), and a wave then walks run = ceil(M / want) parity blocks.  The small pools above always get run = 1; these
# pools have enough segments for run > 1 — the loop's second block, its prefetch, an odd run, a short last run, several slices.
# (n, k, S words, stripes, [(touched stripes, writes per touched stripe)]); the run expected on 256 CUs is in the comment.
RUN_POOLS = [
    (20, 16, 4, 8192, [(8192, 1), (3000, 1)]),      # M = 4: run = 4 (one wave, the whole parity), then run = 2
    (130, 100, 4, 2048, [(2048, 1), (1200, 1)]),    # M = 30: run = 8 with a last run of 6, then run = 5 (odd)
    (20, 16, 320, 4096, [(2500, 2), (4096, 1)]),    # two slices, the second with 16 live lanes: T = 2 with run = 2, then T = 1 with run = 4
]


@pytest.mark.parametrize("n,k,S,B,calls", RUN_POOLS)
def test_several_parity_blocks_per_wave(torch_cuda, fe, n, k, S, B, calls):
    torch = torch_cuda
    M = n - k
    rng = np.random.default_rng(n + S + B)
    g = torch.Generator(device="cuda:0").manual_seed(B + S)

    def words(count):
        return torch.randint(0, P, (count,), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32)

    with fe.Encoder(n, k, 4 * S) as enc:
        def encode_pool(data):
            out = torch.empty(B * M * S, dtype=torch.int32, device="cuda:0")
            for b in range(B):
                enc.encode(data[b * k * S:(b + 1) * k * S], out[b * M * S:(b + 1) * M * S])
            torch.cuda.synchronize()
            return out

        data = words(B * k * S)
        parity = encode_pool(data)
        for touched, per in calls:
            stripes = rng.permutation(B)[:touched]
            writes = np.concatenate([b * k + rng.permutation(k)[:per] for b in stripes]).astype(np.int64)
            writes = writes[rng.permutation(len(writes))]
            new = words(len(writes) * S)
            want_d = data.clone()
            want_d.view(B * k, S)[torch.from_numpy(writes).to("cuda:0")] = new.view(len(writes), S)
            enc.update_batch(data, parity, B, writes.tolist(), new)
            torch.cuda.synchronize()
            assert torch.equal(data, want_d), (touched, per)
            want_p = encode_pool(want_d)
            bad = (parity.view(B, M, S) != want_p.view(B, M, S)).any(dim=2)
            assert not bool(bad.any()), "calls %r: wrong (stripe, parity block) pairs, first ones %r" % ((touched, per), bad.nonzero()[:8].tolist())


def test_offsets_beyond_32_bits(torch_cuda, fe):
    """(20,16) x 4 KB x 66000 stripes: the data alone is over 4 GiB.  The pool is all zero (a pool of codewords); one write goes into the
    last stripe and one into a stripe past the 4 GiB mark.  The touched stripes equal their encode; nothing else is non-zero."""
    torch = torch_cuda
    n, k, S, B = 20, 16, 1024, 66000
    M = n - k
    rng = np.random.default_rng(15)
    touched = [65600, B - 1]
    assert touched[0] * k * S * 4 > 1 << 32
    writes = [touched[1] * k + 11, touched[0] * k + 4]
    new = rand_words(rng, (2, S))
    with fe.Encoder(n, k, 4 * S) as enc:
        data = torch.zeros(B * k * S, dtype=torch.int32, device="cuda:0")
        parity = torch.zeros(B * M * S, dtype=torch.int32, device="cuda:0")
        enc.update_batch(data, parity, B, writes, to_dev(torch, new.reshape(-1)))
        torch.cuda.synchronize()
        for b, w, row in zip((touched[1], touched[0]), writes, new):
            stripe = np.zeros((k, S), np.uint32)
            stripe[w % k] = row
            d = data[b * k * S:(b + 1) * k * S]
            p = parity[b * M * S:(b + 1) * M * S]
            assert np.array_equal(host(d).reshape(k, S), stripe), b
            one = torch.zeros(M * S, dtype=torch.int32, device="cuda:0")
            enc.encode(to_dev(torch, stripe.reshape(-1)), one)
            torch.cuda.synchronize()
            assert torch.equal(p, one), b
            assert int(torch.count_nonzero(p)) > 0
            d.zero_()
            p.zero_()
        assert int(torch.count_nonzero(data)) == 0 and int(torch.count_nonzero(parity)) == 0


def test_refusals_leave_the_pool_unchanged(torch_cuda, fe):
    torch = torch_cuda
    S, B = 16, 3
    rng = np.random.default_rng(16)

    def refused(enc, k, m, writes, code):
        data, parity = to_dev(torch, rand_words(rng, B * k * S)), to_dev(torch, rand_words(rng, B * m * S))
        new = to_dev(torch, rand_words(rng, max(len(writes), 1) * S))
        d0, p0, n0 = data.clone(), parity.clone(), new.clone()
        with pytest.raises(fe.FastEccError) as ei:
            enc.update_batch(data, parity, B, writes, new)
        assert ei.value.code == code
        for old in (None, new):
            with pytest.raises(fe.FastEccError) as ei:
                enc.update_parity_batch(parity, B, writes, new, old=old)
            assert ei.value.code == code
        torch.cuda.synchronize()
        assert torch.equal(data, d0) and torch.equal(parity, p0) and torch.equal(new, n0)

    with fe.Encoder(48, 32, 4 * S) as enc:
        refused(enc, 32, 16, [3, 40, 3], fe.E_INVAL)             # a duplicate index
        refused(enc, 32, 16, [40, 70, 41, 70], fe.E_INVAL)       # ... not next to each other in the list
        refused(enc, 32, 16, [1, B * 32], fe.E_INVAL)            # an index >= count * k
        refused(enc, 32, 16, [(1 << 64) - 1], fe.E_INVAL)
    with fe.Encoder(64, 32, 4 * S, field=fe.FIELD_GF_P61_SQUARED) as enc:
        refused(enc, 32, 32, [1], fe.E_UNSUPPORTED)              # the 64-bit field
    with fe.ShardedEncoder(64, 32, 4 * S, [0, 0]) as enc:
        refused(enc, 32, 32, [1], fe.E_UNSUPPORTED)              # a sharded context
    with fe.Encoder(64, 32, 60) as enc:
        enc.set_option("row_pitch_words", 16)
        refused(enc, 32, 32, [1], fe.E_UNSUPPORTED)              # a set row pitch


def test_invalid_arguments_with_a_real_context(torch_cuda, fe):
    """What tests/test_update_batch_host.py can only ask of a null context: count == 0, a null pointer with writes to do and pointers off
    a 4-byte boundary are FASTECC_E_INVAL on a live context too, and nothing is written."""
    torch = torch_cuda
    k, m, S, B = 16, 4, 16, 3
    rng = np.random.default_rng(17)
    lib = fe.lib()
    with fe.Encoder(k + m, k, 4 * S) as enc:
        data, parity = to_dev(torch, rand_words(rng, B * k * S + 1)), to_dev(torch, rand_words(rng, B * m * S + 1))
        new, old = to_dev(torch, rand_words(rng, 2 * S + 1)), to_dev(torch, rand_words(rng, 2 * S + 1))
        keep = [t.clone() for t in (data, parity, new, old)]
        w = (ctypes.c_uint64 * 2)(5, k + 1)
        d, p, nw, ol = (t.data_ptr() for t in (data, parity, new, old))

        def both(dd, pp, count, ww, n_writes, oo, nn):
            """the two entry points with the same arguments (the parity form has no data, the data form no old blocks)"""
            return (lib.fastecc_update_batch(enc._h, dd, pp, count, ww, n_writes, nn, None),
                    lib.fastecc_update_parity_batch(enc._h, pp, count, ww, n_writes, oo, nn, None))

        inval = (fe.E_INVAL, fe.E_INVAL)
        assert both(d, p, 0, w, 2, ol, nw) == inval            # count 0
        assert both(d, p, 0, w, 0, ol, nw) == inval            # ... with nothing to write
        assert both(d, None, B, w, 2, ol, nw) == inval         # no parity
        assert both(d, p, B, None, 2, ol, nw) == inval         # no list
        assert both(d, p, B, w, 2, ol, None) == inval          # no new blocks
        assert lib.fastecc_update_batch(enc._h, None, p, B, w, 2, nw, None) == fe.E_INVAL   # no data
        for off in (1, 2, 3):
            assert both(d, p + off, B, w, 2, ol, nw) == inval  # parity off a word boundary
            assert both(d, p, B, w, 2, ol, nw + off) == inval  # new blocks
            assert lib.fastecc_update_batch(enc._h, d + off, p, B, w, 2, nw, None) == fe.E_INVAL          # data
            assert lib.fastecc_update_parity_batch(enc._h, p, B, w, 2, ol + off, nw, None) == fe.E_INVAL  # old blocks
        assert both(d, p, (1 << 64) - 1, w, 2, ol, nw) == inval  # byte sizes beyond 64 bits
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip((data, parity, new, old), keep))
        # the same arguments, valid: accepted (the refusals above are not the list's or the context's doing)
        assert both(d, p, B, w, 2, ol, nw) == (0, 0)
        assert both(d, p, B, None, 0, None, None) == (0, 0)    # nothing to write: a no-op, null list and blocks included
        torch.cuda.synchronize()


def test_no_writes_is_a_no_op(torch_cuda, pools):
    torch = torch_cuda
    pool = pools("V=2")
    dd, dp = pool.device(pool.data), pool.device(pool.parity)
    pool.enc.update_batch(dd, dp, pool.B, [], dd[:0])
    pool.enc.update_parity_batch(dp, pool.B, [], dd[:0])
    torch.cuda.synchronize()
    assert np.array_equal(host(dd).reshape(pool.data.shape), pool.data) and np.array_equal(host(dp).reshape(pool.parity.shape), pool.parity)
