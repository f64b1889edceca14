"""GPU tests (-m gpu): every (T, V) instance of the update path's parity kernels, through each call that has them.

update.hip instantiates its parity stream for T delta rows x V words per lane — (1, 2, 4, 8, 16) x (4, 2, 1) — in three kernels:
update_parity_kernel (fastecc_update, _update_parity), update_batch_kernel (_update_batch, _update_parity_batch) and update_set_kernel (the
_set forms).  The small shapes are the smallest at which that stream can still go wrong:

  * code (32,16), three stripes and a guard stripe of sentinel words behind them; M = 16 parity blocks, so every wave gets ONE parity block;
  * 1, 2, 3, 5, 9, 16 and 17 changed blocks per stripe: classes T = 1, 2, 4, 8, 16, 16 and 16 + 1 (a second pass / round of T = 1); 3, 5 and 9
    leave padded rows that must contribute nothing.  (32,16) has only 16 data blocks, so the 17 run on (48,32): the same M = 16;
  * S = 260 words (65 lane groups of 4: a second wave with one live lane; V = 4), 130 (V = 2), 33 (V = 1), and 260 with the pool 8 bytes
    (V = 2) and 4 bytes (V = 1) past a 16-byte boundary.

Every case goes through update and update_parity stripe by stripe, update_batch, update_parity_batch with and without old rows, the two set
forms with FASTECC_PATTERN_NONE on every stripe, and the two set forms under a set of two patterns that between them lose a written data block,
an unwritten one (where the stripe has one), the first parity block, the last one and two adjacent ones in the middle.  Whole stripes must equal
encode_pool of the new stripes bit for bit (the library's encode is pinned to the reference elsewhere); of degraded stripes the present blocks
equal that encode, the absent blocks and every sentinel word keep their bytes, and repair_batch_set of a clone gives the whole new stripes.

The large shapes at the end are the smallest where a wave walks more than one parity block (the second half of the kernels' pipeline)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 0xFFF00001
NONE = 0xFFFFFFFF  # FASTECC_PATTERN_NONE
COUNT = 3
SENTINEL = 0x5A5A5A5A
CHANGED = [1, 2, 3, 5, 9, 16, 17]
# (words per block, the pool's offset from a 16-byte boundary in words)
POOLS = [(260, 0), (130, 0), (33, 0), (260, 2), (260, 1)]
LOST_PARITY = ([0, 7, 8], [15])  # pattern 0: the first block and two adjacent ones in the middle; pattern 1: the last block
PATTERN_OF = [0, 1, 0]


def code_for(t):
    return (32, 16) if t <= 16 else (48, 32)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def fe(hip_lib):
    import fastecc_amd
    return fastecc_amd


def rand_words(torch, shape, seed):
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    return torch.randint(0, P, shape, dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32)


class Case:
    """One (code, S, t): the old stripes, the writes in every form the calls take, and the stripes afterwards; computed once, never written"""

    def __init__(self, torch, enc, n, k, S, t):
        self.enc, self.n, self.k, self.m, self.S, self.t = enc, n, k, n - k, S, t
        rng = np.random.default_rng(1000 * S + t)
        self.blocks = [int(i) for i in rng.permutation(k)[:t]]  # the same blocks of every stripe, in the order of the rows
        unwritten = [i for i in range(k) if i not in self.blocks]
        # (pattern 1 loses an unwritten data block; at t = k there is none and it loses a second written one)
        self.patterns = [([self.blocks[0]], LOST_PARITY[0]), ([unwritten[0] if unwritten else self.blocks[-1]], LOST_PARITY[1])]
        self.data = rand_words(torch, (COUNT, k, S), S + t)
        self.new = rand_words(torch, (COUNT, t, S), S + t + 1)    # row j of stripe b: its block blocks[j]
        self.old = self.data[:, self.blocks].contiguous()
        self.new_data = self.data.clone()
        self.new_data[:, self.blocks] = self.new
        zeroed = self.new_data.clone()
        zeroed[:, self.blocks] = 0
        self.parity, self.new_parity, self.zeroed_parity = (self.encode(x) for x in (self.data, self.new_data, zeroed))
        # the pool forms: the writes of all stripes in one shuffled list
        perm = rng.permutation(COUNT * t)
        self.writes = [int(w) for w in np.array([b * k + i for b in range(COUNT) for i in self.blocks])[perm]]
        at = torch.from_numpy(perm).to("cuda:0")
        self.new_rows, self.old_rows = self.new.view(-1, S)[at].contiguous(), self.old.view(-1, S)[at].contiguous()
        self.absent_d, self.absent_p = torch.zeros((COUNT, k), dtype=torch.bool), torch.zeros((COUNT, self.m), dtype=torch.bool)
        for b, q in enumerate(PATTERN_OF):
            self.absent_d[b, self.patterns[q][0]] = True
            self.absent_p[b, self.patterns[q][1]] = True
        self.absent_d, self.absent_p = self.absent_d.to("cuda:0"), self.absent_p.to("cuda:0")
        torch.cuda.synchronize()

    def encode(self, data):
        parity = data.new_zeros((COUNT, self.m, self.S))
        self.enc.encode_pool(data, parity, COUNT)
        return parity

    def prepare_set(self):
        dp, pp = np.ones((2, self.k), np.uint8), np.ones((2, self.m), np.uint8)
        for q, (ld, lp) in enumerate(self.patterns):
            dp[q, ld] = 0
            pp[q, lp] = 0
        self.enc.decode_prepare_set(dp, pp)


@pytest.fixture(scope="module")
def cases(torch_cuda, fe):
    encoders, made = {}, {}

    def get(S, t):
        n, k = code_for(t)
        if (S, t) not in made:
            if (n, k, S) not in encoders:
                encoders[n, k, S] = fe.Encoder(n, k, 4 * S)
            made[S, t] = Case(torch_cuda, encoders[n, k, S], n, k, S, t)
        return made[S, t]
    yield get
    for enc in encoders.values():
        enc.close()


class Pool:
    """Stripes [COUNT, rows, S] with the blocks `absent` ([COUNT, rows] bool, or None) overwritten by 0xFFFFFFFF, `off` words past a 16-byte
    boundary, inside sentinel words: `off` words before, the guard stripe and the rest of a 16-byte unit after."""

    def __init__(self, torch, content, off, absent=None):
        self.torch, self.off, self.absent = torch, off, absent
        self.shape = content.shape
        self.buf = self.image(content)
        assert self.buf.data_ptr() % 16 == 0
        self.addr = self.buf.data_ptr() + 4 * off  # a raw address

    def image(self, content):
        rows, S = self.shape[1], self.shape[2]
        words = COUNT * rows * S
        buf = self.torch.full((self.off + words + rows * S + 4,), SENTINEL, dtype=self.torch.int32, device="cuda:0")
        view = buf[self.off:self.off + words].view(self.shape)
        view.copy_(content)
        if self.absent is not None:
            view[self.absent] = -1
        return buf

    def stripe(self, b):
        return self.addr + 4 * b * self.shape[1] * self.shape[2]

    def holds(self, content):
        """these stripes in the present blocks; every absent block and every sentinel word as it was"""
        return self.torch.equal(self.buf, self.image(content))

    def clone(self):
        return Pool(self.torch, self.buf[self.off:self.off + COUNT * self.shape[1] * self.shape[2]].view(self.shape), self.off)


@pytest.mark.parametrize("S,off", POOLS, ids=["S%d_off%d" % p for p in POOLS])
@pytest.mark.parametrize("t", CHANGED)
def test_every_instance(torch_cuda, cases, t, S, off):
    torch = torch_cuda
    c = cases(S, t)
    enc = c.enc
    what = "S %d, offset %d words, %d changed blocks per stripe" % (S, off, t)

    def done(name, D, Q, repair=False):
        torch.cuda.synchronize()
        assert D is None or D.holds(c.new_data), "%s, data, %s" % (name, what)
        assert Q.holds(c.new_parity), "%s, parity, %s" % (name, what)
        if repair:  # a clone under the same patterns becomes the whole new stripes
            D = D.clone() if D is not None else Pool(torch, c.new_data, off, c.absent_d)
            Q = Q.clone()
            whole_d, whole_q = Pool(torch, c.new_data, off), Pool(torch, c.new_parity, off)
            enc.repair_batch_set(D.addr, Q.addr, COUNT, PATTERN_OF)
            torch.cuda.synchronize()
            assert torch.equal(D.buf, whole_d.buf) and torch.equal(Q.buf, whole_q.buf), "%s, then repair_batch_set, %s" % (name, what)

    # update_parity_kernel: stripe by stripe
    D, Q = Pool(torch, c.data, off), Pool(torch, c.parity, off)
    for b in range(COUNT):
        enc.update(D.stripe(b), Q.stripe(b), c.blocks, c.new[b])
    done("update", D, Q)
    Q = Pool(torch, c.parity, off)
    for b in range(COUNT):
        enc.update_parity(Q.stripe(b), c.blocks, c.new[b], old=c.old[b])
    done("update_parity", None, Q)
    # update_batch_kernel: the pool, the parity alone from old rows, and from zero (the parity of the stripes with zeros in the written blocks)
    D, Q = Pool(torch, c.data, off), Pool(torch, c.parity, off)
    enc.update_batch(D.addr, Q.addr, COUNT, c.writes, c.new_rows)
    done("update_batch", D, Q)
    Q = Pool(torch, c.parity, off)
    enc.update_parity_batch(Q.addr, COUNT, c.writes, c.new_rows, old=c.old_rows)
    done("update_parity_batch", None, Q)
    Q = Pool(torch, c.zeroed_parity, off)
    enc.update_parity_batch(Q.addr, COUNT, c.writes, c.new_rows)
    done("update_parity_batch from zero", None, Q)
    # update_set_kernel: whole stripes, then the set of two patterns
    c.prepare_set()
    whole = [NONE] * COUNT
    D, Q = Pool(torch, c.data, off), Pool(torch, c.parity, off)
    enc.update_batch_set(D.addr, Q.addr, COUNT, whole, c.writes, c.new_rows)
    done("update_batch_set, whole", D, Q)
    Q = Pool(torch, c.parity, off)
    enc.update_parity_batch_set(Q.addr, COUNT, whole, c.writes, c.new_rows, old=c.old_rows)
    done("update_parity_batch_set, whole", None, Q)
    D, Q = Pool(torch, c.data, off, c.absent_d), Pool(torch, c.parity, off, c.absent_p)
    enc.update_batch_set(D.addr, Q.addr, COUNT, PATTERN_OF, c.writes, c.new_rows)
    done("update_batch_set", D, Q, repair=True)
    Q = Pool(torch, c.parity, off, c.absent_p)
    enc.update_parity_batch_set(Q.addr, COUNT, PATTERN_OF, c.writes, c.new_rows, old=c.old_rows)
    done("update_parity_batch_set", None, Q, repair=True)


# ---- a wave that walks more than one parity block ----
# The host gives a launch every resident wave of the device where the parity count allows it (tests/test_gpu_update_batch.py, RUN_POOLS):
# target = 4 SIMDs x CUs x waves per SIMD, 8192 on 256 CUs for T <= 4.  A single stripe of (8192,4096) x 768 words has 3 column slices, so a
# wave walks run = ceil(4096 / (8192 / 3)) = 2 parity blocks at T = 1, and at T = 16, V = 4 (5 waves per SIMD: target 5120) run = 3 with a
# last run of 1 — an odd run with a short last run.  (Expected on 256 CUs; it depends on the CU count, so nothing here asserts it.)
@pytest.mark.parametrize("t", [1, 16])
def test_single_stripe_runs(torch_cuda, fe, t):
    torch = torch_cuda
    n, k, S = 8192, 4096, 768
    rng = np.random.default_rng(t)
    blocks = [int(i) for i in rng.permutation(k)[:t]]
    with fe.Encoder(n, k, 4 * S) as enc:
        data = rand_words(torch, (k, S), 10 + t)
        new = rand_words(torch, (t, S), 20 + t)
        parity, want = torch.zeros((n - k, S), dtype=torch.int32, device="cuda:0"), torch.zeros((n - k, S), dtype=torch.int32, device="cuda:0")
        enc.encode(data, parity)
        old_parity = parity.clone()
        new_data = data.clone()
        new_data[blocks] = new
        enc.encode(new_data, want)
        old = data[blocks].contiguous()
        enc.update(data, parity, blocks, new)
        torch.cuda.synchronize()
        assert torch.equal(data, new_data) and torch.equal(parity, want), "update"
        enc.update_parity(parity, blocks, old, old=new)  # and back to the old blocks
        torch.cuda.synchronize()
        assert torch.equal(parity, old_parity), "update_parity"


# (n, k, S words, stripes, touched stripes (one write each), lost parity block or None); the run expected on 256 CUs is in the comment
RUN_POOLS = [
    (20, 16, 4, 8192, 8192, None),   # M = 4: run = 4, one wave walks the whole parity of its stripe
    (20, 16, 4, 8192, 8192, 2),      # ... and steps over a middle block that every stripe has lost
    (130, 100, 4, 2048, 2048, None),  # M = 30: run = 8 with a last run of 6 (short)
    (130, 100, 4, 2048, 1200, None),  # run = 5 (odd); M = 30 cannot give an odd run AND a short last run, so:
    (23, 16, 4, 4096, 2731, None),    # M = 7: run = 3 with a last run of 1, in update_batch_kernel
    (23, 16, 4, 4096, 2731, 3),       # ... and in update_set_kernel, the middle block of the middle run lost
]


@pytest.mark.parametrize("n,k,S,B,touched,lost", RUN_POOLS)
def test_pool_runs(torch_cuda, fe, n, k, S, B, touched, lost):
    torch = torch_cuda
    M = n - k
    rng = np.random.default_rng(n + B + touched)
    stripes = rng.permutation(B)[:touched]
    writes = (stripes * k + rng.integers(0, k, size=touched)).astype(np.int64)
    with fe.Encoder(n, k, 4 * S) as enc:
        data = rand_words(torch, (B, k, S), n)
        new = rand_words(torch, (touched, S), n + 1)
        parity, want = torch.zeros((B, M, S), dtype=torch.int32, device="cuda:0"), torch.zeros((B, M, S), dtype=torch.int32, device="cuda:0")
        enc.encode_pool(data, parity, B)
        new_data = data.clone()
        new_data.view(B * k, S)[torch.from_numpy(writes).to("cuda:0")] = new
        enc.encode_pool(new_data, want, B)
        if lost is None:
            enc.update_batch(data, parity, B, writes.tolist(), new)
        else:
            pp = np.ones((1, M), np.uint8)
            pp[0, lost] = 0
            enc.decode_prepare_set(np.ones((1, k), np.uint8), pp)
            parity[:, lost] = -1
            want[:, lost] = -1  # an absent block keeps its bytes
            enc.update_batch_set(data, parity, B, np.zeros(B, np.uint32), writes.tolist(), new)
        torch.cuda.synchronize()
        assert torch.equal(data, new_data)
        bad = (parity != want).any(dim=2)
        assert not bool(bad.any()), "wrong (stripe, parity block) pairs, first ones %r" % bad.nonzero()[:8].tolist()
