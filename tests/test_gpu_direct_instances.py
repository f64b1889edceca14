"""GPU tests (-m gpu): every (EB, V) instance of the direct path's VALU kernels, through each kernel that has them.

direct.hip instantiates its row loop for EB outputs x V words per lane — (1, 2, 4) x (4, 2, 1), 8 x (2, 1), 16 x 1 — in four kernels:
direct_accumulate_kernel (its own copy), direct_batch_kernel, direct_set_kernel and, as EB = 1, direct_read_kernel (weigh_rows).  The shapes
here are the smallest at which that loop can still go wrong:

  * code (32,16), three stripes and a guard stripe of sentinel words behind them;
  * 1, 2, 3, 5, 9 and 16 lost data blocks: classes EB = 1, 2, 4, 8, 16, 16 and 17, 18, 19, 21, 25, 32 rows to sum — the last group of
    U = 8, 4 or 2 rows in flight is partial, and at 32 rows exact;
  * S = 260 words (65 lane groups of 4: a second wave with one live lane; V = 4 / 2 / 1 for EB <= 4 / 8 / 16), 130 (V = 2 / 2 / 1), 33 (V = 1),
    and 260 with the pool 8 bytes (V <= 2) and 4 bytes (V = 1) past a 16-byte boundary.

Lost blocks hold 0xFFFFFFFF.  Every case goes through single-stripe repair on the VALU kernel, repair_batch and repair_batch_set as one launch,
read_batch_set and read_batch of every data block; all five give back the original stripes bit for bit (the library's encode is pinned to the
reference elsewhere) and write nothing else."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 0xFFF00001
N, K, M, COUNT = 32, 16, 16, 3
SENTINEL = 0x5A5A5A5A
LOST = [1, 2, 3, 5, 9, 16]
# (words per block, the pool's offset from a 16-byte boundary in words)
POOLS = [(260, 0), (130, 0), (33, 0), (260, 2), (260, 1)]
ORDER = [int(x) for x in np.random.default_rng(1).permutation(K)]       # which data blocks go first
PARITY_ORDER = [int(x) for x in np.random.default_rng(2).permutation(M)]


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
def codes(torch_cuda, fe):
    """S -> (encoder with both kernel choices forced, the original data [COUNT, K, S] and parity [COUNT, M, S]); computed once, never written"""
    torch, made = torch_cuda, {}

    def get(S):
        if S not in made:
            enc = fe.Encoder(N, K, 4 * S)
            enc.set_option("direct_kernel", 1)        # single stripes: the VALU kernel (direct_accumulate_kernel)
            enc.set_option("decode_batch_kernel", 1)  # batches and sets: one launch (direct_batch_kernel, direct_set_kernel)
            g = torch.Generator(device="cuda:0").manual_seed(S)
            data = torch.randint(0, P, (COUNT, K, S), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32)
            parity = torch.zeros((COUNT, M, S), dtype=torch.int32, device="cuda:0")
            enc.encode_pool(data, parity, COUNT)
            torch.cuda.synchronize()
            made[S] = (enc, data, parity)
        return made[S]
    yield get
    for enc, _, _ in made.values():
        enc.close()


class Damaged:
    """The original stripes with the lost blocks overwritten by 0xFFFFFFFF, `off` words past a 16-byte boundary, inside sentinel words: `off`
    words before, the guard stripe and the rest of a 16-byte unit after."""

    def __init__(self, torch, orig, lost, off):
        self.torch, self.orig = torch, orig
        rows, S = orig.shape[1], orig.shape[2]
        words = COUNT * rows * S
        self.buf = torch.full((off + words + rows * S + 4,), SENTINEL, dtype=torch.int32, device="cuda:0")
        assert self.buf.data_ptr() % 16 == 0
        self.stripes = self.buf[off:off + words].view(COUNT, rows, S)
        self.stripes.copy_(orig)
        if lost:
            self.stripes[:, lost] = -1
        self.before = self.buf.clone()
        self.whole = self.before.clone()
        self.whole[off:off + words] = orig.reshape(-1)
        self.addr = self.buf.data_ptr() + 4 * off  # a raw address

    def stripe(self, b):
        return self.addr + 4 * b * self.stripes[0].numel()

    def restored(self):
        """the original stripes, and every sentinel word as it was"""
        return self.torch.equal(self.buf, self.whole)

    def untouched(self):
        return self.torch.equal(self.buf, self.before)


def flags(lost_data, lost_parity):
    dp, pp = np.ones(K, np.uint8), np.ones(M, np.uint8)
    dp[lost_data] = 0
    pp[lost_parity] = 0
    return dp, pp


def five_paths(torch, codes, S, off, lost_data, lost_parity, windows=((0, None),)):
    enc, data, parity = codes(S)
    dp, pp = flags(lost_data, lost_parity)
    enc.decode_prepare(dp, pp)
    enc.decode_prepare_set(dp[None, :], pp[None, :])
    pattern_of = np.zeros(COUNT, np.uint32)
    what = "S %d, offset %d words, lost data %s parity %s" % (S, off, lost_data, lost_parity)

    def pools():
        return Damaged(torch, data, lost_data, off), Damaged(torch, parity, lost_parity, off)

    # 1. direct_accumulate_kernel: stripe by stripe
    D, Q = pools()
    for b in range(COUNT):
        enc.repair(D.stripe(b), Q.stripe(b))
    torch.cuda.synchronize()
    assert D.restored() and Q.restored(), "repair, " + what
    # 2. direct_batch_kernel
    D, Q = pools()
    enc.repair_batch(D.addr, Q.addr, COUNT)
    torch.cuda.synchronize()
    assert D.restored() and Q.restored(), "repair_batch, " + what
    # 3. direct_set_kernel: the same pattern as a set of one
    D, Q = pools()
    enc.repair_batch_set(D.addr, Q.addr, COUNT, pattern_of)
    torch.cuda.synchronize()
    assert D.restored() and Q.restored(), "repair_batch_set, " + what
    # 4, 5. direct_read_kernel: every data block of every stripe, from the set and from the single pattern
    D, Q = pools()
    reads = np.arange(COUNT * K, dtype=np.uint64)
    for col0, width in windows:
        w = S - col0 if width is None else width
        want = data.view(-1, S)[:, col0:col0 + w]
        for set_form in (True, False):
            out = torch.full((COUNT * K + 2, w), SENTINEL, dtype=torch.int32, device="cuda:0")
            if set_form:
                enc.read_batch_set(D.addr, Q.addr, COUNT, pattern_of, reads, out[1:], col0=col0, width=width)
            else:
                enc.read_batch(D.addr, Q.addr, COUNT, reads, out[1:], col0=col0, width=width)
            torch.cuda.synchronize()
            form = "read_batch_set" if set_form else "read_batch"
            assert torch.equal(out[1:-1], want), "%s window (%d, %d), %s" % (form, col0, w, what)
            assert bool((out[0] == SENTINEL).all()) and bool((out[-1] == SENTINEL).all()), "%s writes its rows only, %s" % (form, what)
            assert D.untouched() and Q.untouched(), "%s does not write the pool, %s" % (form, what)


@pytest.mark.parametrize("S,off", POOLS, ids=["S%d_off%d" % p for p in POOLS])
@pytest.mark.parametrize("lost", LOST)
def test_every_instance(torch_cuda, codes, lost, S, off):
    five_paths(torch_cuda, codes, S, off, sorted(ORDER[:lost]), [])


def test_lost_parity_beside_lost_data(torch_cuda, codes):
    """outputs on both stripes: three data blocks by pos even, one parity block by pos odd (class EB = 4)"""
    five_paths(torch_cuda, codes, 260, 0, sorted(ORDER[:3]), PARITY_ORDER[:1])


def test_read_window(torch_cuda, codes):
    """the window form of the reads: columns [4, 136) of 260"""
    five_paths(torch_cuda, codes, 260, 0, sorted(ORDER[:5]), [], windows=((4, 132),))
