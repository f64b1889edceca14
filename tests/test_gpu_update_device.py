"""GPU tests (-m gpu) of the pool writes from a write list in device memory: fastecc_update_batch_device, fastecc_update_parity_batch_device.

Expected bytes are bit-exact.  The primary check is a clone of the pool after the HOST-list call with the same writes (update_batch /
update_parity_batch and their window forms, pinned by their own tests); for whole blocks the parity is also encode_pool of the new data.  Every
pool carries a guard stripe of sentinel words behind it, outside `count`: untouched stripes and the sentinels must keep their bytes, so the whole
tensors are compared.  A refused list (a non-zero status word) must leave the pool word for word as it was."""
import numpy as np
import pytest

from test_gpu_update_batch import POOLS

pytestmark = pytest.mark.gpu

P = 0xFFF00001
NONE = -1  # FASTECC_WRITE_NONE in an int64 tensor
STATUS_GARBAGE = 0x5151515151515151
INVAL, UNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def fe(hip_lib):
    import fastecc_amd
    return fastecc_amd


def rand_words(rng, shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64).astype(np.uint32)


def to_dev(torch, a, shift=0):
    """the words of `a` in device memory, `shift` words past an aligned address"""
    t = torch.zeros(a.size + shift, dtype=torch.int32, device="cuda:0")
    t[shift:] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1).view(np.int32)).to("cuda:0")
    return t[shift:]


def decode_status(v):
    """(code, row) of a status word"""
    v = int(v) & ((1 << 64) - 1)
    hi = v >> 32
    return (hi - (1 << 32) if hi >= 1 << 31 else hi), v & 0xFFFFFFFF


class Pool:
    """`count` random stripes and their parity (encode_pool) in device memory, a guard stripe of sentinel words behind each of the two tensors"""

    def __init__(self, torch, enc, n, k, S, count, seed, shift=0):
        self.torch, self.enc, self.n, self.k, self.S, self.count, self.m = torch, enc, n, k, S, count, n - k
        self.rng = np.random.default_rng(seed)
        data = np.concatenate([rand_words(self.rng, count * k * S), np.full(k * S, 0xFEEDFACE, np.uint32)])
        self.dd = to_dev(torch, data, shift)
        self.dp = to_dev(torch, np.full((count + 1) * self.m * S, 0xDEADBEEF, np.uint32), shift)
        enc.encode_pool(self.dd, self.dp, count)
        torch.cuda.synchronize()

    def rows(self, n_rows, width):
        return to_dev(self.torch, rand_words(self.rng, (n_rows, width)))

    def old_rows(self, writes, col0, width):
        """the pool's present words of the written windows, one row per list entry (FASTECC_WRITE_NONE or an index past the pool: block 0's)"""
        idx = self.torch.tensor([w if 0 <= w < self.count * self.k else 0 for w in writes], dtype=self.torch.int64, device="cuda:0")
        blocks = self.dd[:self.count * self.k * self.S].view(self.count * self.k, self.S)
        return blocks[idx, col0:col0 + width].contiguous().view(-1)

    def reference(self, writes, new, window, form, old):
        """(data, parity) clones after the host-list call with the list's real writes and their rows"""
        torch, enc = self.torch, self.enc
        col0, width = window
        real = [u for u, w in enumerate(writes) if w != NONE]
        sel = torch.tensor(real, dtype=torch.int64, device="cuda:0")
        pick = lambda rows: None if rows is None else rows.view(len(writes), width)[sel].contiguous().view(-1)
        cd, cp = self.dd.clone(), self.dp.clone()
        kw = {} if window == (0, self.S) else dict(col0=col0, width=width)
        if real and form == "batch":
            enc.update_batch(cd, cp, self.count, [writes[u] for u in real], pick(new), **kw)
        elif real:
            enc.update_parity_batch(cp, self.count, [writes[u] for u in real], pick(new), old=pick(old), **kw)
        torch.cuda.synchronize()
        return cd, cp

    def device_call(self, writes, new, window, form, old, mps, stream=0):
        """the device-list call on the pool itself; returns the status word read back after a synchronise"""
        torch, enc = self.torch, self.enc
        col0, width = window
        dw = torch.tensor(writes, dtype=torch.int64, device="cuda:0") if writes else torch.zeros(1, dtype=torch.int64, device="cuda:0")
        status = torch.full((1,), STATUS_GARBAGE, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        if form == "batch":
            enc.update_batch_device(self.dd, self.dp, self.count, dw, len(writes), new, status, max_per_stripe=mps, stream=stream, col0=col0, width=width)
        else:
            enc.update_parity_batch_device(self.dp, self.count, dw, len(writes), new, status, old=old, max_per_stripe=mps, stream=stream, col0=col0,
                                           width=width)
        torch.cuda.synchronize()
        assert dw.tolist()[:len(writes)] == list(writes), "the list is only read"
        return int(status.item())

    def apply(self, writes, mps, window=None, form="batch", with_old=True, new=None, what=""):
        """one device-list call checked against the host-list call on a clone; whole blocks of the data form: against encode_pool as well"""
        torch = self.torch
        window = window or (0, self.S)
        new = self.rows(max(len(writes), 1), window[1]) if new is None else new
        old = self.old_rows(writes, *window) if form == "parity" and with_old and writes else None
        keep = new.clone()
        want_d, want_p = self.reference(writes, new, window, form, old)
        status = self.device_call(writes, new, window, form, old, mps)
        assert status == 0, "%s: status %r" % (what, decode_status(status))
        assert torch.equal(self.dd, want_d), what + ": the data pool (guard stripe included) differs from the host-list call's"
        assert torch.equal(self.dp, want_p), what + ": the parity pool (guard stripe included) differs from the host-list call's"
        assert torch.equal(new, keep), what + ": the rows are only read"
        if form == "batch" and window == (0, self.S):
            fresh = self.dp.clone()
            self.enc.encode_pool(self.dd, fresh, self.count)
            torch.cuda.synchronize()
            assert torch.equal(fresh, self.dp), what + ": the parity is not encode_pool of the new data"
        return new

    def refused(self, writes, mps, code, rows, window=None, form="batch", what=""):
        """a list the device refuses: the status word's code, its row among `rows`, and the pool word for word as before"""
        torch = self.torch
        window = window or (0, self.S)
        new = self.rows(len(writes), window[1])
        old = self.old_rows(writes, *window) if form == "parity" else None
        before_d, before_p = self.dd.clone(), self.dp.clone()
        got = decode_status(self.device_call(writes, new, window, form, old, mps))
        assert got[0] == code and got[1] in rows, "%s: status %r, expected code %d and a row of %r" % (what, got, code, sorted(rows))
        assert torch.equal(self.dd, before_d) and torch.equal(self.dp, before_p), what + ": a refused list wrote to the pool"


def one_write_per_stripe(rng, k, count):
    stripes = rng.permutation(count)
    return [int(b) * k + int(rng.integers(k)) for b in stripes]


# ---- 1. one write per stripe, max_per_stripe = 1, whole block ----
ONE_WRITE = ["k+N/4", "zero-extended", "V=2", "odd S", "misaligned base", "mixed radix", "PFA"]


@pytest.mark.parametrize("name", ONE_WRITE)
def test_one_write_per_stripe(torch_cuda, fe, name):
    n, k, S, count, flags, shift = POOLS[name]
    with fe.Encoder(n, k, 4 * S, flags=flags) as enc:
        pool = Pool(torch_cuda, enc, n, k, S, count, seed=len(name) + S, shift=shift)
        writes = one_write_per_stripe(pool.rng, k, count)
        before = pool.dp.clone()
        pool.apply(writes, 1, what=name)
        assert not torch_cuda.equal(pool.dp, before)  # (the call did something)
        pool.apply(writes[:max(1, count // 2)], 1, form="parity", what=name + ", the parity form")


# ---- 2. every class in one call; the list's order does not matter ----
def test_every_class_in_one_call_in_any_order(torch_cuda, fe):
    n, k, S, count = 40, 32, 8, 6
    per_stripe = [1, 2, 3, 5, 9, 16]
    rng = np.random.default_rng(2)
    writes = [b * k + int(i) for b, t in enumerate(per_stripe) for i in rng.permutation(k)[:t]]
    rows = rand_words(rng, (len(writes), S))
    orders = {"as built": list(range(len(writes))), "reversed": list(range(len(writes)))[::-1], "permuted": [int(u) for u in rng.permutation(len(writes))]}
    results = {}
    with fe.Encoder(n, k, 4 * S) as enc:
        for name, order in orders.items():
            pool = Pool(torch_cuda, enc, n, k, S, count, seed=22)
            pool.apply([writes[u] for u in order], 16, new=to_dev(torch_cuda, rows[order]), what="the list " + name)
            results[name] = (pool.dd.clone(), pool.dp.clone())
    for name in ("reversed", "permuted"):
        assert torch_cuda.equal(results[name][0], results["as built"][0]) and torch_cuda.equal(results[name][1], results["as built"][1]), name


@pytest.mark.parametrize("mps", [2, 3, 4, 5, 8, 9])
def test_promises_between_the_classes(torch_cuda, fe, mps):
    """max_per_stripe admits the classes up to its power of two: stripes with 1 .. mps writes under every kind of promise"""
    n, k, S, count = 40, 32, 8, 6
    rng = np.random.default_rng(mps)
    per_stripe = [1 + (b * (mps - 1)) // (count - 1) for b in range(count)]
    assert per_stripe[0] == 1 and per_stripe[-1] == mps
    writes = [b * k + int(i) for b, t in enumerate(per_stripe) for i in rng.permutation(k)[:t]]
    writes = [writes[u] for u in rng.permutation(len(writes))]
    with fe.Encoder(n, k, 4 * S) as enc:
        Pool(torch_cuda, enc, n, k, S, count, seed=23).apply(writes, mps, what="max_per_stripe = %d" % mps)


# ---- 3. windows ----
@pytest.mark.parametrize("form,with_old", [("batch", True), ("parity", True), ("parity", False)], ids=["batch", "parity_old_rows", "parity_from_zero"])
@pytest.mark.parametrize("window", [(4, 128), (259, 1), (0, 260), (130, 2)], ids=lambda w: "c%d_w%d" % w)
def test_windows(torch_cuda, fe, window, form, with_old):
    n, k, S, count = 20, 16, 260, 5
    rng = np.random.default_rng(window[0] + window[1])
    writes = [b * k + int(i) for b, t in enumerate([1, 3, 0, 2, 4]) for i in rng.permutation(k)[:t]]
    writes = [writes[u] for u in rng.permutation(len(writes))]
    with fe.Encoder(n, k, 4 * S) as enc:
        pool = Pool(torch_cuda, enc, n, k, S, count, seed=33)
        pool.apply(writes, 4, window=window, form=form, with_old=with_old, what="window %r" % (window,))


# ---- 4. FASTECC_WRITE_NONE ----
def test_write_none_entries(torch_cuda, fe):
    n, k, S, count = 20, 16, 64, 7
    with fe.Encoder(n, k, 4 * S) as enc:
        pool = Pool(torch_cuda, enc, n, k, S, count, seed=44)
        real = one_write_per_stripe(pool.rng, k, count)
        writes = [w for pair in zip(real, [NONE] * len(real)) for w in pair]  # every second entry
        pool.apply(writes, 1, what="every second entry NONE")
        before = pool.dd.clone(), pool.dp.clone()
        pool.apply([NONE] * 9, 1, what="a list of NONE only")
        pool.apply([NONE] * 300, 16, form="parity", what="a long list of NONE only")
        pool.apply([], 1, what="n_writes = 0")
        pool.apply([], 16, form="parity", what="n_writes = 0, the parity form")
        assert torch_cuda.equal(pool.dd, before[0]) and torch_cuda.equal(pool.dp, before[1])
        pool.apply(writes[::-1], 1, form="parity", what="every second entry NONE, the parity form")  # (last: the parity leaves the data behind)


# ---- 5. lists the device refuses ----
def test_status_refusals_leave_the_pool_unchanged(torch_cuda, fe):
    n, k, S, count = 40, 32, 8, 6
    rng = np.random.default_rng(5)
    with fe.Encoder(n, k, 4 * S) as enc:
        pool = Pool(torch_cuda, enc, n, k, S, count, seed=55)
        good = [b * k + int(i) for b in range(count) for i in rng.permutation(k)[:3]]
        for form in ("batch", "parity"):
            pool.refused(good[:7] + [count * k] + good[7:], 16, INVAL, {7}, form=form, what="an index == count * k")
            pool.refused([count * k + 5], 1, INVAL, {0}, form=form, what="only an index past the pool")
            pool.refused(good[:4] + [good[4], good[4]] + good[5:], 16, INVAL, {4, 5}, form=form, what="a duplicate, adjacent")
            pool.refused(good + [good[0]], 16, INVAL, {0, len(good)}, form=form, what="a duplicate, far apart")
            seventeen = [2 * k + int(i) for i in rng.permutation(k)[:17]]
            pool.refused(good[:3] + seventeen, 16, UNSUPPORTED, set(range(3, 20)), form=form, what="17 writes to one stripe")
            pool.refused([5, k + 1, 2 * k + 7, k + 9], 1, UNSUPPORTED, {1, 3}, form=form, what="2 writes to one stripe under max_per_stripe = 1")
            pool.refused(good[:5] + [good[1], 1 << 40], 16, INVAL, {1, 5, 6}, form=form, what="a duplicate and an index out of range")
            # straight after a refused call, on the same context
            pool.apply(good, 16, form=form, what="a valid call after the refused ones (%s)" % form)
        pool.refused(good + [good[2]], 16, INVAL, {2, len(good)}, window=(3, 4), what="a duplicate, a window call")


def test_host_refusals_with_a_live_context(torch_cuda, fe):
    """what the return value covers, here with a context and device memory: nothing is enqueued, the status word is not written"""
    torch = torch_cuda
    n, k, S, count = 20, 16, 16, 3
    with fe.Encoder(n, k, 4 * S) as enc:
        pool = Pool(torch, enc, n, k, S, count, seed=66)
        before = pool.dd.clone(), pool.dp.clone()
        rows = pool.rows(4, S)
        dw = torch.tensor([1, 2, NONE, 0, 0], dtype=torch.int64, device="cuda:0")
        status = torch.full((2,), STATUS_GARBAGE, dtype=torch.int64, device="cuda:0")
        lib, h = fe.lib(), enc._h
        d, p, w, r, s = pool.dd.data_ptr(), pool.dp.data_ptr(), dw.data_ptr(), rows.data_ptr(), status.data_ptr()

        def both(code, writes=w, n_writes=3, mps=1, col0=0, width=S, new=r, st=s, cnt=count):
            assert lib.fastecc_update_batch_device(h, d, p, cnt, writes, n_writes, mps, col0, width, new, st, None) == code
            assert lib.fastecc_update_parity_batch_device(h, p, cnt, writes, n_writes, mps, col0, width, None, new, st, None) == code

        both(fe.E_INVAL, mps=0)
        both(fe.E_INVAL, mps=17)
        both(fe.E_INVAL, st=None)
        both(fe.E_INVAL, st=None, n_writes=0)
        both(fe.E_INVAL, writes=w + 4)
        both(fe.E_INVAL, st=s + 4)
        both(fe.E_INVAL, col0=1, width=S)
        both(fe.E_INVAL, col0=0, width=0)
        both(fe.E_INVAL, writes=p + 8)                      # the list inside the parity pool
        both(fe.E_INVAL, st=p + 4 * (count * (n - k) * S - 2))  # the status word on the pool's last words
        both(fe.E_INVAL, writes=r)                          # the list on the rows
        both(fe.E_INVAL, st=r + 8)                          # the status word inside the rows
        both(fe.E_INVAL, st=w + 8)                          # the status word inside the list
        both(fe.E_INVAL, new=p)                             # what the window calls refuse: rows inside the pool
        both(fe.E_UNSUPPORTED, cnt=(1 << 24) + 1)
        both(fe.E_UNSUPPORTED, n_writes=(1 << 24) + 1)
        with fe.Encoder(n, k, 4 * S) as pitched:
            pitched.set_option("row_pitch_words", S + 4)
            assert lib.fastecc_update_batch_device(pitched._h, d, p, count, w, 3, 1, 0, S, r, s, None) == fe.E_UNSUPPORTED
        torch.cuda.synchronize()
        assert status.tolist() == [STATUS_GARBAGE] * 2 and torch.equal(pool.dd, before[0]) and torch.equal(pool.dp, before[1])
        pool.apply([1, 2 * k + 3], 1, what="a valid call after the refusals")


# ---- 6. more than one workgroup of the build kernels; growth ----
@pytest.mark.parametrize("count", [300, 1025])
def test_many_stripes_cross_the_workgroups_of_the_build_kernels(torch_cuda, fe, count):
    n, k, S = 6, 4, 4
    with fe.Encoder(n, k, 4 * S) as enc:
        pool = Pool(torch_cuda, enc, n, k, S, count, seed=count)
        pool.apply(one_write_per_stripe(pool.rng, k, count), 1, what="%d stripes, one write each" % count)
        two = [int(b) * k + int(i) for b in range(count) for i in pool.rng.permutation(k)[:2]]
        pool.apply([two[u] for u in pool.rng.permutation(len(two))], 2, what="%d stripes, two writes each" % count)
        pool.apply(one_write_per_stripe(pool.rng, k, count), 1, form="parity", what="%d stripes, the parity form" % count)


def test_a_context_that_grows(torch_cuda, fe):
    n, k, S = 6, 4, 4
    with fe.Encoder(n, k, 4 * S) as enc:
        small = Pool(torch_cuda, enc, n, k, S, 7, seed=7)
        small.apply(one_write_per_stripe(small.rng, k, 7), 1, what="7 stripes")
        large = Pool(torch_cuda, enc, n, k, S, 1025, seed=1025)
        large.apply(one_write_per_stripe(large.rng, k, 1025), 1, what="1025 stripes on the context that served 7")
        small.apply(one_write_per_stripe(small.rng, k, 7), 1, what="7 stripes again")


# ---- 7. a list made on the device ----
def test_a_list_made_on_the_device(torch_cuda, fe):
    """The list is computed by torch ops on a side stream from a seeded device tensor and is never on the host before the calls: two calls back to
    back on that stream with the same `writes` and `status` buffers, rewritten on the stream between them; one synchronise at the end."""
    torch = torch_cuda
    n, k, S, count = 20, 16, 64, 40
    with fe.Encoder(n, k, 4 * S) as enc:
        pool = Pool(torch, enc, n, k, S, count, seed=77)
        start_d, start_p = pool.dd.clone(), pool.dp.clone()
        rows1, rows2 = pool.rows(count, S), pool.rows(count, S)
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(7)
        seed = torch.randperm(count, generator=gen, device="cuda:0")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            writes = seed * k + (seed * 5 + 3) % k                       # one write per stripe, in a permuted order
            status = torch.full((1,), STATUS_GARBAGE, dtype=torch.int64, device="cuda:0")
            enc.update_batch_device(pool.dd, pool.dp, count, writes, count, rows1, status, stream=st.cuda_stream)
            list1, status1 = writes.clone(), status.clone()
            writes.copy_(torch.where(seed % 3 == 0, torch.full_like(seed, NONE), seed.flip(0) * k + (seed + 11) % k))  # every third stripe of the order: skipped
            status.fill_(STATUS_GARBAGE)
            enc.update_batch_device(pool.dd, pool.dp, count, writes, count, rows2, status, stream=st.cuda_stream)
        torch.cuda.synchronize()
        assert status1.item() == 0 and status.item() == 0
        list1, list2 = list1.tolist(), writes.tolist()
        assert len(set(list1)) == count and NONE in list2 and len({w for w in list2 if w != NONE}) > count // 2
        got_d, got_p = pool.dd.clone(), pool.dp.clone()
        pool.dd.copy_(start_d)
        pool.dp.copy_(start_p)
        for writes_host, rows in ((list1, rows1), (list2, rows2)):  # the same two lists through the host-list call
            real = [u for u, w in enumerate(writes_host) if w != NONE]
            enc.update_batch(pool.dd, pool.dp, count, [writes_host[u] for u in real], rows.view(count, S)[torch.tensor(real, device="cuda:0")].contiguous().view(-1))
        torch.cuda.synchronize()
        assert torch.equal(got_d, pool.dd) and torch.equal(got_p, pool.dp)
        fresh = got_p.clone()
        enc.encode_pool(got_d, fresh, count)
        torch.cuda.synchronize()
        assert torch.equal(fresh, got_p)
