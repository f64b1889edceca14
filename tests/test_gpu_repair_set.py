"""GPU tests (-m gpu) of the pattern-set calls: fastecc_decode_prepare_set, fastecc_repair_batch_set, fastecc_decode_batch_set.

A pool of stripes stored back to back, every stripe with its own erasure pattern out of a prepared set (rotated placement: one lost device
costs stripe b a different block).  The codewords come from the library's own single-stripe encode (pinned to the reference by the other
suites).  A set call must give back the original pool bit for bit, and exactly what a loop of fastecc_decode_prepare + fastecc_repair over
the same erased stripes gives, through the one-launch kernel (option decode_batch_kernel = 1) and the stripe-by-stripe form (= 2).  Nothing
but the erased blocks is written: not the survivors, not (decode_batch_set) the erased parity blocks, not a FASTECC_PATTERN_NONE stripe that
holds garbage only, not the guard stripe after the pool.  Pools live on the device and are compared there."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 0xFFF00001
GARBAGE = -1          # 0xFFFFFFFF as the int32 the device tensors hold: what an erased block holds before the call (not even a field element)
GUARD = 0x5A5A5A5A    # the stripe after the last one of a pool


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
    """count codewords [count + 1, k, S] / [count + 1, m, S] on the device (one fastecc_encode per stripe) and a guard stripe after them"""

    def __init__(self, torch, enc, count, S, seed, fill=None):
        self.torch, self.enc, self.count, self.S = torch, enc, count, S
        self.k, self.m = enc.k, enc.n - enc.k
        g = torch.Generator(device="cuda:0").manual_seed(seed)
        self.data = torch.full((count + 1, self.k, S), GUARD, dtype=torch.int32, device="cuda:0")
        self.parity = torch.full((count + 1, self.m, S), GUARD, dtype=torch.int32, device="cuda:0")
        if fill is None:
            self.data[:count] = torch.randint(0, P, (count, self.k, S), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32)
        else:
            self.data[:count] = fill if fill < 1 << 31 else fill - (1 << 32)
        for b in range(count):
            enc.encode(self.data[b].data_ptr(), self.parity[b].data_ptr())
        torch.cuda.synchronize()

    def erased(self, patterns, pattern_of, fe, wipe_none=False):
        """copies of the pool with every stripe's lost blocks (and, wipe_none, the whole FASTECC_PATTERN_NONE stripes) set to GARBAGE"""
        torch = self.torch
        D, Q = self.data.clone(), self.parity.clone()
        db, dr, pb, pr = [], [], [], []
        for b, q in enumerate(pattern_of):
            if q == fe.PATTERN_NONE:
                if wipe_none:
                    D[b], Q[b] = GARBAGE, GARBAGE
                continue
            ld, lp = patterns[q]
            db += [b] * len(ld)
            dr += list(ld)
            pb += [b] * len(lp)
            pr += list(lp)
        if db:
            D[torch.tensor(db, device="cuda:0"), torch.tensor(dr, device="cuda:0")] = GARBAGE
        if pb:
            Q[torch.tensor(pb, device="cuda:0"), torch.tensor(pr, device="cuda:0")] = GARBAGE
        torch.cuda.synchronize()
        return D, Q

    def stripe(self, D, Q, b):
        return D[b].data_ptr(), Q[b].data_ptr()


def flag_rows(k, m, patterns):
    dp, pp = np.ones((len(patterns), k), np.uint8), np.ones((len(patterns), m), np.uint8)
    for q, (ld, lp) in enumerate(patterns):
        dp[q, list(ld)] = 0
        pp[q, list(lp)] = 0
    return dp, pp


def loop_repair(pool, patterns, pattern_of, fe):
    """the per-stripe route: fastecc_decode_prepare + fastecc_repair for every stripe whose pattern lost something"""
    enc = pool.enc
    D, Q = pool.erased(patterns, pattern_of, fe, wipe_none=True)
    dp, pp = flag_rows(pool.k, pool.m, patterns)
    for b, q in enumerate(pattern_of):
        if q == fe.PATTERN_NONE or not (patterns[q][0] or patterns[q][1]):
            continue
        enc.decode_prepare(dp[q], pp[q])
        enc.repair(*pool.stripe(D, Q, b))
    pool.torch.cuda.synchronize()
    return D, Q


def expectation(pool, patterns, pattern_of, fe, op):
    """the original pool; FASTECC_PATTERN_NONE stripes stay GARBAGE; decode leaves the erased parity blocks GARBAGE"""
    left = [([], lp if op == "decode" else []) for ld, lp in patterns]
    return pool.erased(left, pattern_of, fe, wipe_none=True)


def check_set(pool, patterns, pattern_of, fe, modes, loop=None, stream=0):
    """repair_batch_set and decode_batch_set of the erased pool == the expectation (== the per-stripe loop), for each decode_batch_kernel mode"""
    torch, enc = pool.torch, pool.enc
    po = np.array(pattern_of, dtype=np.uint32)
    if loop is not None:
        want_d, want_p = expectation(pool, patterns, pattern_of, fe, "repair")
        assert torch.equal(loop[0], want_d) and torch.equal(loop[1], want_p), "the per-stripe loop gives back the original"
    for op in ("repair", "decode"):
        want_d, want_p = expectation(pool, patterns, pattern_of, fe, op)
        for mode in modes:
            enc.set_option("decode_batch_kernel", mode)
            D, Q = pool.erased(patterns, pattern_of, fe, wipe_none=True)
            getattr(enc, op + "_batch_set")(D, Q, pool.count, po, stream=stream)
            torch.cuda.synchronize()
            assert torch.equal(D, want_d), "%s_batch_set data, mode %d" % (op, mode)
            assert torch.equal(Q, want_p), "%s_batch_set parity, mode %d" % (op, mode)
    enc.set_option("decode_batch_kernel", 0)


def codeword_block(k, u):
    """pattern that loses codeword block u: data block u, or parity block u - k"""
    return ([u], []) if u < k else ([], [u - k])


# ---- 1. rotated single failure ----
# (n, k, flags, the codeword blocks the patterns lose): every rotation, 16 of 2048 for the largest code
ROTATED = [(20, 16, 0, None), (14, 10, 0, None), (24, 16, 0, None), (64, 16, 0, None), (256, 128, 0, None), (128, 96, 1, None),
           (2048, 1024, 0, [(137 * q + 5) % 2048 for q in range(16)])]
WORDS = [1, 33, 64, 256, 1025]  # a lone live lane; odd with a masked tail; one wave at V = 1; one wave at V = 4; several waves, a tail, V = 1


@pytest.mark.parametrize("S", WORDS)
@pytest.mark.parametrize("n,k,fl,lose", ROTATED, ids=["%d_%d" % (c[0], c[1]) for c in ROTATED])
def test_rotated_single_failure(torch_cuda, fe, n, k, fl, lose, S):
    count = 67
    lose = list(range(n)) if lose is None else lose
    patterns = [codeword_block(k, u) for u in lose]
    pattern_of = [(7 * b + 3) % len(patterns) for b in range(count)]
    with fe.Encoder(n, k, 4 * S, flags=fl) as enc:
        pool = Pool(torch_cuda, enc, count, S, seed=n * 1000 + S)
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        loop = loop_repair(pool, patterns, pattern_of, fe)
        check_set(pool, patterns, pattern_of, fe, modes=(1, 2), loop=loop)


# ---- 2. mixed classes in one call ----
def mixed_patterns(k, m, rng):
    """0, 1, 2, 3, 5, 9 and 16 lost blocks: data only, parity only and both"""
    shapes = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (0, 2), (3, 0), (1, 2), (0, 3), (5, 0), (0, 5), (3, 2), (9, 0), (0, 9), (4, 5), (16, 0), (0, 16), (9, 7)]
    return [(sorted(int(x) for x in rng.permutation(k)[:ld]), sorted(int(x) for x in rng.permutation(m)[:lp])) for ld, lp in shapes]


@pytest.mark.parametrize("S", [33, 256])
def test_mixed_classes_in_one_call(torch_cuda, fe, S):
    n, k, count = 64, 32, 59
    rng = np.random.default_rng(S)
    patterns = mixed_patterns(k, n - k, rng)
    # every pattern several times, and FASTECC_PATTERN_NONE stripes (all GARBAGE) in between
    pattern_of = [fe.PATTERN_NONE if b % 7 == 3 else (5 * b + 1) % len(patterns) for b in range(count)]
    assert set(pattern_of) == set(range(len(patterns))) | {fe.PATTERN_NONE}
    with fe.Encoder(n, k, 4 * S) as enc:
        pool = Pool(torch_cuda, enc, count, S, seed=S)
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        loop = loop_repair(pool, patterns, pattern_of, fe)
        check_set(pool, patterns, pattern_of, fe, modes=(0, 1, 2), loop=loop)


# ---- 3. the lazy sums' worst case ----
def test_lazy_sum_worst_case(torch_cuda, fe):
    """(2048,1024), every data word p - 1, 16 lost blocks: 1040 rows, the longest row loop the kernel takes by default at its largest terms"""
    n, k, S, count = 2048, 1024, 64, 4
    patterns = [(list(range(3, 3 + 16 * 61, 61)), []), (list(range(1, 1 + 8 * 97, 97)), list(range(2, 2 + 8 * 113, 113))), ([], list(range(5, 5 + 16 * 59, 59)))]
    pattern_of = [0, 1, 2, 0]
    with fe.Encoder(n, k, 4 * S) as enc:
        pool = Pool(torch_cuda, enc, count, S, seed=0, fill=P - 1)
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        loop = loop_repair(pool, patterns, pattern_of, fe)
        check_set(pool, patterns, pattern_of, fe, modes=(0, 1, 2), loop=loop)


# ---- 4. the branch rule ----
def test_branch_rule(torch_cuda, fe):
    """k = 8192: a pass reads more than 4096 rows, so mode 0 goes stripe by stripe and mode 1 takes the kernel; the same bits"""
    torch = torch_cuda
    n, k, S, count = 8192 + 16, 8192, 64, 3
    patterns = [([5], []), ([100], [3]), ([], [7])]
    pattern_of = [0, 1, 2]
    po = np.array(pattern_of, dtype=np.uint32)
    with fe.Encoder(n, k, 4 * S) as enc:
        pool = Pool(torch, enc, count, S, seed=4)
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        want_d, want_p = expectation(pool, patterns, pattern_of, fe, "repair")
        enc.profile(True)
        results = []
        for mode, scope, other in ((0, "direct_pass", "direct_pass_set"), (1, "direct_pass_set", "direct_pass")):
            enc.set_option("decode_batch_kernel", mode)
            D, Q = pool.erased(patterns, pattern_of, fe)
            enc.profile_reset()
            enc.repair_batch_set(D, Q, count, po)
            torch.cuda.synchronize()
            seen = enc.profile_read()
            assert scope in seen and other not in seen, (mode, sorted(seen))
            assert torch.equal(D, want_d) and torch.equal(Q, want_p), "mode %d" % mode
            results.append((D, Q))
        assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])


# ---- 5. independence of the single prepared pattern ----
def test_set_and_single_pattern_are_independent(torch_cuda, fe):
    torch = torch_cuda
    n, k, S, count = 20, 16, 64, 9
    m = n - k
    rotate = lambda shift: [codeword_block(k, (u + shift) % n) for u in range(n)]  # noqa: E731
    pattern_of = [(3 * b + 1) % n for b in range(count)]
    po = np.array(pattern_of, dtype=np.uint32)
    A, B = ([2], []), ([7], [1])
    with fe.Encoder(n, k, 4 * S) as enc:
        pool = Pool(torch, enc, count, S, seed=5)
        enc.set_option("decode_batch_kernel", 1)
        dpA, ppA = flag_rows(k, m, [A])
        enc.decode_prepare(dpA[0], ppA[0])
        enc.decode_prepare_set(*flag_rows(k, m, rotate(0)))
        # repair_batch still applies A
        D, Q = pool.erased([A], [0] * count, fe)
        enc.repair_batch(D, Q, count)
        torch.cuda.synchronize()
        assert torch.equal(D, pool.data) and torch.equal(Q, pool.parity), "the single pattern survives decode_prepare_set"
        # another single pattern does not change what the set does
        dpB, ppB = flag_rows(k, m, [B])
        enc.decode_prepare(dpB[0], ppB[0])
        D, Q = pool.erased(rotate(0), pattern_of, fe)
        enc.repair_batch_set(D, Q, count, po)
        torch.cuda.synchronize()
        assert torch.equal(D, pool.data) and torch.equal(Q, pool.parity), "the set survives decode_prepare"
        # ... and the set call did not change the single pattern
        D, Q = pool.erased([B], [0] * count, fe)
        enc.repair_batch(D, Q, count)
        torch.cuda.synchronize()
        assert torch.equal(D, pool.data) and torch.equal(Q, pool.parity), "the single pattern survives repair_batch_set"
        # replacing the set takes effect: the old set would rebuild other blocks
        enc.decode_prepare_set(*flag_rows(k, m, rotate(5)))
        D, Q = pool.erased(rotate(5), pattern_of, fe)
        enc.repair_batch_set(D, Q, count, po)
        torch.cuda.synchronize()
        assert torch.equal(D, pool.data) and torch.equal(Q, pool.parity), "the replaced set"
        # clearing it: the set calls are refused and write nothing
        enc.decode_prepare_set([], [])
        D, Q = pool.erased(rotate(5), pattern_of, fe)
        D0, Q0 = D.clone(), Q.clone()
        for fn in (fe.lib().fastecc_decode_batch_set, fe.lib().fastecc_repair_batch_set):
            assert fn(enc._h, D.data_ptr(), Q.data_ptr(), count, po.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), None) == fe.E_INVAL
        torch.cuda.synchronize()
        assert torch.equal(D, D0) and torch.equal(Q, Q0)


# ---- 6. refusals on a live context ----
def refused(torch, fe, enc, rc_want, words_d, words_p, pattern_of, count=2):
    """both set calls return rc_want and leave the pool byte for byte as it was"""
    g = torch.Generator(device="cuda:0").manual_seed(3)
    D = torch.randint(0, 1 << 31, (words_d,), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32)
    Q = torch.randint(0, 1 << 31, (words_p,), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32)
    D0, Q0 = D.clone(), Q.clone()
    po = np.array(pattern_of, dtype=np.uint32)
    torch.cuda.synchronize()
    for fn in (fe.lib().fastecc_decode_batch_set, fe.lib().fastecc_repair_batch_set):
        rc = fn(enc._h, D.data_ptr(), Q.data_ptr(), count, po.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), None)
        assert rc == rc_want, (fn.__name__, rc)
    torch.cuda.synchronize()
    assert torch.equal(D, D0) and torch.equal(Q, Q0)


def prepare_set_rc(fe, enc, dp, pp):
    u8p = ctypes.POINTER(ctypes.c_uint8)
    return fe.lib().fastecc_decode_prepare_set(enc._h, dp.ctypes.data_as(u8p), pp.ctypes.data_as(u8p), len(dp))


def test_refusals(torch_cuda, fe):
    torch = torch_cuda
    n, k, S, count = 64, 32, 64, 5
    m = n - k
    patterns = [codeword_block(k, u) for u in (0, 40, 9)]
    pattern_of = [0, 1, 2, 1, 0]
    with fe.Encoder(n, k, 4 * S) as enc:
        pool = Pool(torch, enc, count, S, seed=6)
        refused(torch, fe, enc, fe.E_INVAL, 2 * k * S, 2 * m * S, [0, 0])  # no set prepared
        enc.decode_prepare_set(*flag_rows(k, m, patterns))
        # 17 losses: unsupported; more than n - k: not decodable; too many patterns; and the previous set is still in force
        assert prepare_set_rc(fe, enc, *flag_rows(k, m, [patterns[0], (list(range(10)), list(range(7)))])) == fe.E_UNSUPPORTED
        assert prepare_set_rc(fe, enc, *flag_rows(k, m, [(list(range(20)), list(range(13)))])) == fe.E_INVAL
        assert prepare_set_rc(fe, enc, *flag_rows(k, m, [patterns[0]] * 4097)) == fe.E_INVAL
        u8p = ctypes.POINTER(ctypes.c_uint8)
        assert fe.lib().fastecc_decode_prepare_set(enc._h, None, np.ones(m, np.uint8).ctypes.data_as(u8p), 1) == fe.E_INVAL
        check_set(pool, patterns, pattern_of, fe, modes=(1,))
        refused(torch, fe, enc, fe.E_INVAL, 2 * k * S, 2 * m * S, [0, len(patterns)])       # an entry = P
        refused(torch, fe, enc, fe.E_INVAL, 2 * k * S, 2 * m * S, [0, 0xFFFFFFFE])
        refused(torch, fe, enc, fe.E_INVAL, 2 * k * S, 2 * m * S, [0, 0], count=(1 << 64) - 1)  # byte sizes beyond 64 bits
        enc.set_option("row_pitch_words", S + 32)
        refused(torch, fe, enc, fe.E_UNSUPPORTED, 2 * k * (S + 32), 2 * m * (S + 32), [0, 0])
        assert prepare_set_rc(fe, enc, *flag_rows(k, m, patterns)) == fe.E_UNSUPPORTED
    with fe.Encoder(20, 16, 4 * S) as enc:
        assert prepare_set_rc(fe, enc, *flag_rows(16, 4, [([1, 2, 3], [0, 1])])) == fe.E_INVAL  # fewer than k survivors
        refused(torch, fe, enc, fe.E_INVAL, 2 * 16 * S, 2 * 4 * S, [0, 0])                       # ... and no set came of it
    N = 16
    with fe.Encoder(2 * N, N, 16 * 8, field=fe.FIELD_GF_P61_SQUARED) as enc:
        assert prepare_set_rc(fe, enc, *flag_rows(N, N, [([0], [])])) == fe.E_UNSUPPORTED
        refused(torch, fe, enc, fe.E_UNSUPPORTED, 2 * N * 32, 2 * N * 32, [0, 0])
    with fe.ShardedEncoder(2 * N, N, 4 * S, [0, 0]) as enc:
        assert prepare_set_rc(fe, enc, *flag_rows(N, N, [([0], [])])) == fe.E_UNSUPPORTED
        refused(torch, fe, enc, fe.E_UNSUPPORTED, 2 * N * S, 2 * N * S, [0, 0])


# ---- 7. staging of the per-call list ----
def test_list_staging_on_a_stream(torch_cuda, fe):
    """two calls back to back on a non-default stream with different pattern_of arrays, each overwritten as soon as its call returns"""
    torch = torch_cuda
    n, k, S, count = 24, 16, 256, 300
    patterns = [codeword_block(k, u) for u in range(n)]
    rot = [(5 * b + 2) % n for b in range(count)]
    first = [q if b % 2 == 0 else fe.PATTERN_NONE for b, q in enumerate(rot)]
    second = [q if b % 2 == 1 else fe.PATTERN_NONE for b, q in enumerate(rot)]
    with fe.Encoder(n, k, 4 * S) as enc:
        pool = Pool(torch, enc, count, S, seed=7)
        enc.decode_prepare_set(*flag_rows(k, n - k, patterns))
        D, Q = pool.erased(patterns, rot, fe)
        s1 = torch.cuda.Stream()
        po = np.array(first, dtype=np.uint32)
        enc.repair_batch_set(D, Q, count, po, stream=s1.cuda_stream)
        po[:] = 0  # (pattern 0 loses data block 0: a list read late would rebuild that block everywhere)
        po2 = np.array(second, dtype=np.uint32)
        enc.repair_batch_set(D, Q, count, po2, stream=s1.cuda_stream)
        po2[:] = 1
        torch.cuda.synchronize()
        assert torch.equal(D, pool.data) and torch.equal(Q, pool.parity)
