"""GPU tests (-m gpu) that pin the dispatch structure of the batched scrub calls: how many launches every profile scope records, chunk
by chunk, for fastecc_verify_batch, fastecc_verify_batch_set, fastecc_locate_errors_batch, fastecc_correct_batch and the last two with a
pattern per stripe, fastecc_locate_errors_batch_set and fastecc_correct_batch_set.

The expected counts are formulas of the documented algorithm (the head comment of fastecc_amd/csrc/scrub.hip, DESIGN.md sections 14, 16,
17, 19 and 27), never numbers read back from a run.  With "scrub_batch_chunk" = CHUNK a pass over X stripes takes ceil(X / CHUNK) chunks, and
per chunk
  a verify chunk is one fingerprint launch, one transform and one syndrome check; with n - k blocks named absent no coefficient is left
      to check and the chunk ends after its fingerprints; a chunk of a set call whose stripes are all PATTERN_NONE is skipped;
  batched location runs one list pass per chunk of the FLAGGED stripes (list fingerprints, transform, syndrome gather) and one root search
      per chunk that holds a locator; a stripe with a word >= p in a present block is left to the single-stripe code;
  with a pattern per stripe the same passes run in their set forms, over the flagged stripes whose pattern leaves 1 .. 512 syndromes, and the
      grouped repair is one launch per size class of the lost sets;
  the grouped correction closes with one list verify (list fingerprints, transform, syndrome check) over the repaired stripes;
  fastecc_correct on one stripe reads the stripe twice: the fingerprints of its location and of its closing verify.
Every case also checks the call's result: the pool's parity is the oracle's (tests/pool_model.py Codec), the corruption is the test's own."""
import numpy as np
import pytest

from pool_model import Codec

pytestmark = pytest.mark.gpu

P = 0xFFF00001
NONE = 0xFFFFFFFF
SEED = 0x57A6E5
N, K, COUNT, CHUNK = 20, 16, 5, 2
M = N - K
# words per block, words the data pointer is offset by: the vector form, the scalar form, the scalar form of blocks of whole dwordx4
SHAPES = [(64, 0), (37, 0), (64, 1)]
BAD = {0: 3, 2: 17, 3: 9}  # stripe -> its corrupted block (chunks of the pool: {0, 1} {2, 3} {4}; of the flagged list: {0, 2} {3})


def chunks(x):
    return -(-x // CHUNK)


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
def codewords(oracle):
    """(data, parity) of COUNT clean stripes per block size, computed once; the tests copy them"""
    codec, out = Codec(oracle, N, K), {}
    for S in sorted({S for S, _ in SHAPES}):
        d = np.random.default_rng(S).integers(0, P, size=(COUNT, K, S), dtype=np.uint64).astype(np.uint32)
        out[S] = (d, np.stack([codec.parity(d[b]) for b in range(COUNT)]))
        out[S][0].setflags(write=False)
        out[S][1].setflags(write=False)
    return out


class Pool:
    """the stripes d, p in device memory, the data `skew` words into its allocation"""

    def __init__(self, torch, d, p, skew):
        self.torch, self.shape_d, self.shape_p = torch, d.shape, p.shape
        flat = np.concatenate([np.zeros(skew, np.uint32), d.reshape(-1)])
        self.D = torch.from_numpy(flat.view(np.int32)).to("cuda:0")[skew:]
        self.Q = torch.from_numpy(p.reshape(-1).copy().view(np.int32)).to("cuda:0")
        assert self.D.data_ptr() % 16 == 4 * skew and self.Q.data_ptr() % 16 == 0

    def read(self):
        self.torch.cuda.synchronize()
        return (self.D.cpu().numpy().view(np.uint32).reshape(self.shape_d), self.Q.cpu().numpy().view(np.uint32).reshape(self.shape_p))


def block(d, p, b, j):
    return d[b, j] if j < K else p[b, j - K]


def garbage(d, p, b, blocks):
    for j in blocks:
        block(d, p, b, j)[:] = 0xFFFFFFFF


def launches(enc, call):
    """(the call's result, {scope: launches} of that call alone)"""
    enc.profile(True)
    enc.profile_reset()
    try:
        result = call()
    finally:
        prof = enc.profile_read(cap=128)
        enc.profile(False)
    return result, {name: v[1] for name, v in prof.items()}


def open_encoder(fe, S):
    enc = fe.Encoder(N, K, 4 * S)
    enc.set_option("scrub_batch_chunk", CHUNK)
    return enc


def presence(absent):
    return [j not in absent for j in range(K)], [j not in absent for j in range(K, N)]


@pytest.mark.parametrize("S,skew", SHAPES)
def test_verify_batch_clean(torch_cuda, fe, codewords, S, skew):
    d, p = codewords[S]
    with open_encoder(fe, S) as enc:
        pool = Pool(torch_cuda, d, p, skew)
        ok, got = launches(enc, lambda: enc.verify_batch(pool.D, pool.Q, COUNT, seed=SEED))
        assert ok.all()
        for scope in ("fingerprint_batch", "scrub_transform_batch", "scrub_syndromes_batch"):
            assert got.get(scope, 0) == chunks(COUNT), (scope, got)
        assert "fingerprint" not in got and "fingerprint_batch_list" not in got


@pytest.mark.parametrize("S,skew", SHAPES)
def test_verify_batch_all_parity_budget_absent(torch_cuda, fe, codewords, S, skew):
    absent = [1, 6, 16, 19]  # n - k blocks: no coefficient is left, only a word >= p in a present block counts
    assert len(absent) == M
    d, p = codewords[S][0].copy(), codewords[S][1].copy()
    for b in range(COUNT):
        garbage(d, p, b, absent)
    block(d, p, 1, 4)[S // 2] = P + 5           # a present block with a word >= p
    block(d, p, 3, 5)[0] = (int(d[3, 5, 0]) + 1) % P  # any word < p is explained by the n - k erasures
    with open_encoder(fe, S) as enc:
        enc.scrub_erasures(*presence(absent))
        pool = Pool(torch_cuda, d, p, skew)
        ok, got = launches(enc, lambda: enc.verify_batch(pool.D, pool.Q, COUNT, seed=SEED))
        assert ok.tolist() == [True, False, True, True, True]
        assert got.get("fingerprint_batch", 0) == chunks(COUNT), got
        assert got.get("scrub_transform_batch", 0) == 0 and got.get("scrub_syndromes_batch", 0) == 0, got


PATTERN_OF = [0, NONE, NONE, NONE, 1]  # the chunk {2, 3} is all PATTERN_NONE: skipped
SET_CHUNKS = len({b // CHUNK for b, q in enumerate(PATTERN_OF) if q != NONE})


@pytest.mark.parametrize("S,skew", SHAPES)
def test_verify_batch_set_two_patterns(torch_cuda, fe, codewords, S, skew):
    patterns = [[2], [18, 5]]
    d, p = codewords[S][0].copy(), codewords[S][1].copy()
    for b, q in enumerate(PATTERN_OF):
        garbage(d, p, b, range(N) if q == NONE else patterns[q])
    block(d, p, 4, 7)[S - 1] = (int(d[4, 7, S - 1]) + 1) % P  # a present block of stripe 4
    with open_encoder(fe, S) as enc:
        enc.scrub_erasures_set([presence(q)[0] for q in patterns], [presence(q)[1] for q in patterns])
        pool = Pool(torch_cuda, d, p, skew)
        ok, got = launches(enc, lambda: enc.verify_batch_set(pool.D, pool.Q, COUNT, PATTERN_OF, seed=SEED))
        assert ok.tolist() == [True, True, True, True, False]
        assert SET_CHUNKS == 2
        for scope in ("fingerprint_set", "scrub_transform_batch", "scrub_syndromes_set"):
            assert got.get(scope, 0) == SET_CHUNKS, (scope, got)
        assert "fingerprint_batch" not in got and "scrub_syndromes_batch" not in got


@pytest.mark.parametrize("S,skew", SHAPES)
def test_verify_batch_set_nothing_left_to_check(torch_cuda, fe, codewords, S, skew):
    patterns = [[0, 1, 2, 3], [8, 17, 18, 19]]  # n - k blocks each
    d, p = codewords[S][0].copy(), codewords[S][1].copy()
    for b, q in enumerate(PATTERN_OF):
        garbage(d, p, b, range(N) if q == NONE else patterns[q])
    block(d, p, 0, 9)[1] = (int(d[0, 9, 1]) + 1) % P  # below p: explained by the erasures
    block(d, p, 4, 16)[S - 1] = 0xFFF00001           # a present block with a word >= p
    with open_encoder(fe, S) as enc:
        enc.scrub_erasures_set([presence(q)[0] for q in patterns], [presence(q)[1] for q in patterns])
        pool = Pool(torch_cuda, d, p, skew)
        ok, got = launches(enc, lambda: enc.verify_batch_set(pool.D, pool.Q, COUNT, PATTERN_OF, seed=SEED))
        assert ok.tolist() == [True, True, True, True, False]
        assert got.get("fingerprint_set", 0) == SET_CHUNKS, got
        assert got.get("scrub_transform_batch", 0) == 0 and got.get("scrub_syndromes_set", 0) == 0, got


def corrupted(codewords, S, big=None):
    """the pool with block BAD[b] of stripe b wrong in one word: another value below p, or (stripe `big`) a word >= p"""
    d, p = codewords[S][0].copy(), codewords[S][1].copy()
    for b, j in BAD.items():
        row = block(d, p, b, j)
        row[S // 3] = P + 1 + b if b == big else (int(row[S // 3]) + 1 + b) % P
    return d, p


L = len(BAD)  # the flagged stripes


@pytest.mark.parametrize("S,skew", SHAPES)
def test_locate_errors_batch(torch_cuda, fe, codewords, S, skew):
    d, p = corrupted(codewords, S)
    with open_encoder(fe, S) as enc:
        pool = Pool(torch_cuda, d, p, skew)
        (status, lists), got = launches(enc, lambda: enc.locate_errors_batch(pool.D, pool.Q, COUNT, seed=SEED))
        assert status.tolist() == [1 if b in BAD else 0 for b in range(COUNT)]
        assert lists == [[BAD[b]] if b in BAD else [] for b in range(COUNT)]
        assert got.get("fingerprint_batch", 0) == chunks(COUNT) and got.get("scrub_syndromes_batch", 0) == chunks(COUNT), got
        for scope in ("fingerprint_batch_list", "scrub_syndromes_gather", "scrub_root_search_batch"):
            assert got.get(scope, 0) == chunks(L), (scope, got)
        assert got.get("scrub_transform_batch", 0) == chunks(COUNT) + chunks(L), got
        assert got.get("fingerprint", 0) == 0, got
        hd, hp = pool.read()
        assert np.array_equal(hd, d) and np.array_equal(hp, p)  # reads only


@pytest.mark.parametrize("S,skew", SHAPES)
def test_correct_batch_grouped(torch_cuda, fe, codewords, S, skew):
    d, p = corrupted(codewords, S)
    with open_encoder(fe, S) as enc:
        enc.set_option("correct_batch_mode", 1)
        pool = Pool(torch_cuda, d, p, skew)
        status, got = launches(enc, lambda: enc.correct_batch(pool.D, pool.Q, COUNT, seed=SEED))
        assert status.tolist() == [1 if b in BAD else 0 for b in range(COUNT)]
        # the verify, the list pass of the location, the closing list verify over the L repaired stripes
        assert got.get("fingerprint_batch", 0) == chunks(COUNT), got
        assert got.get("fingerprint_batch_list", 0) == chunks(L) + chunks(L), got
        assert got.get("scrub_syndromes_gather", 0) == chunks(L) and got.get("scrub_root_search_batch", 0) == chunks(L), got
        assert got.get("scrub_syndromes_batch", 0) == chunks(COUNT) + chunks(L), got
        assert got.get("scrub_transform_batch", 0) == chunks(COUNT) + 2 * chunks(L), got
        assert got.get("fingerprint", 0) == 0, got
        hd, hp = pool.read()
        assert np.array_equal(hd, codewords[S][0]) and np.array_equal(hp, codewords[S][1])


@pytest.mark.parametrize("S,skew", SHAPES)
def test_correct_batch_grouped_with_a_word_above_p(torch_cuda, fe, codewords, S, skew):
    big = 3  # the flagged list's second chunk is this stripe alone: no locator there, no root search
    d, p = corrupted(codewords, S, big=big)
    batched = L - 1  # the stripes the grouped path repairs
    with open_encoder(fe, S) as enc:
        enc.set_option("correct_batch_mode", 1)
        pool = Pool(torch_cuda, d, p, skew)
        status, got = launches(enc, lambda: enc.correct_batch(pool.D, pool.Q, COUNT, seed=SEED))
        assert status.tolist() == [1 if b in BAD else 0 for b in range(COUNT)]
        assert got.get("fingerprint_batch", 0) == chunks(COUNT), got
        assert got.get("fingerprint_batch_list", 0) == chunks(L) + chunks(batched), got
        assert got.get("scrub_syndromes_gather", 0) == chunks(L), got
        flagged = sorted(BAD)
        with_locator = len({i // CHUNK for i, b in enumerate(flagged) if b != big})
        assert with_locator == 1 and got.get("scrub_root_search_batch", 0) == with_locator, got
        assert got.get("scrub_syndromes_batch", 0) == chunks(COUNT) + chunks(batched), got
        assert got.get("scrub_transform_batch", 0) == chunks(COUNT) + chunks(L) + chunks(batched), got
        assert got.get("fingerprint", 0) == 2, got  # fastecc_correct on the one stripe: its location and its closing verify
        hd, hp = pool.read()
        assert np.array_equal(hd, codewords[S][0]) and np.array_equal(hp, codewords[S][1])


# ---- the same two calls with a pattern per stripe ----
SET_PATTERNS = [[2], [18, 5]]  # n - k - w = 3 and 2 syndromes: one wrong block is within reach under either
LOCATE_PATTERN_OF = [0, 1, 1, 0, NONE]  # every stripe of BAD has a pattern that leaves its corrupted block present; the chunk {4} is all PATTERN_NONE
LOCATE_SET_CHUNKS = len({b // CHUNK for b, q in enumerate(LOCATE_PATTERN_OF) if q != NONE})
assert all(BAD[b] not in SET_PATTERNS[LOCATE_PATTERN_OF[b]] for b in BAD) and LOCATE_SET_CHUNKS == 2


def degraded(codewords, S, big=None):
    """corrupted() with the absent blocks of every stripe, and every block of the PATTERN_NONE stripe, overwritten: (d, p, d and p as a correction
    must leave them: the clean codewords, whole, for the corrected stripes; a consistent stripe and the PATTERN_NONE stripe as they were)"""
    d, p = corrupted(codewords, S, big=big)
    want_d, want_p = codewords[S][0].copy(), codewords[S][1].copy()
    for b, q in enumerate(LOCATE_PATTERN_OF):
        garbage(d, p, b, range(N) if q == NONE else SET_PATTERNS[q])
        if b not in BAD:
            garbage(want_d, want_p, b, range(N) if q == NONE else SET_PATTERNS[q])
    return d, p, want_d, want_p


def open_set_encoder(fe, S):
    enc = open_encoder(fe, S)
    enc.scrub_erasures_set([presence(q)[0] for q in SET_PATTERNS], [presence(q)[1] for q in SET_PATTERNS])
    return enc


def lost_set_classes(stripes):
    """the launches of the grouped repair through the call's private pattern set: one per size class of the lost sets (located and absent blocks;
    the class of a pass: its outputs rounded up to a power of two) — the rule of test_gpu_locate_batch_set.py::test_correct_batch_set_modes"""
    return len({1 << (1 + len(SET_PATTERNS[LOCATE_PATTERN_OF[b]]) - 1).bit_length() for b in stripes})


@pytest.mark.parametrize("S,skew", SHAPES)
def test_locate_errors_batch_set(torch_cuda, fe, codewords, S, skew):
    d, p, _, _ = degraded(codewords, S)
    with open_set_encoder(fe, S) as enc:
        pool = Pool(torch_cuda, d, p, skew)
        (status, lists), got = launches(enc, lambda: enc.locate_errors_batch_set(pool.D, pool.Q, COUNT, LOCATE_PATTERN_OF, seed=SEED))
        assert status.tolist() == [1 if b in BAD else 0 for b in range(COUNT)]
        assert lists == [[BAD[b]] if b in BAD else [] for b in range(COUNT)]
        # the verify pass: the chunks that hold a stripe with a pattern; the list pass: every flagged stripe has 1 .. 512 syndromes left
        assert got.get("fingerprint_set", 0) == LOCATE_SET_CHUNKS and got.get("scrub_syndromes_set", 0) == LOCATE_SET_CHUNKS, got
        for scope in ("fingerprint_set_list", "scrub_syndromes_gather_set", "scrub_root_search_batch"):
            assert got.get(scope, 0) == chunks(L), (scope, got)
        assert got.get("scrub_transform_batch", 0) == LOCATE_SET_CHUNKS + chunks(L), got
        assert got.get("fingerprint", 0) == 0, got
        assert not [x for x in ("fingerprint_batch", "fingerprint_batch_list", "scrub_syndromes_batch", "scrub_syndromes_gather") if x in got], got
        hd, hp = pool.read()
        assert np.array_equal(hd, d) and np.array_equal(hp, p)  # reads only


@pytest.mark.parametrize("S,skew", SHAPES)
def test_correct_batch_set_grouped(torch_cuda, fe, codewords, S, skew):
    d, p, want_d, want_p = degraded(codewords, S)
    with open_set_encoder(fe, S) as enc:
        enc.set_option("correct_batch_mode", 1)
        pool = Pool(torch_cuda, d, p, skew)
        status, got = launches(enc, lambda: enc.correct_batch_set(pool.D, pool.Q, COUNT, LOCATE_PATTERN_OF, seed=SEED))
        assert status.tolist() == [1 if b in BAD else 0 for b in range(COUNT)]
        assert got.get("fingerprint_set", 0) == LOCATE_SET_CHUNKS and got.get("scrub_syndromes_set", 0) == LOCATE_SET_CHUNKS, got
        for scope in ("fingerprint_set_list", "scrub_syndromes_gather_set", "scrub_root_search_batch"):
            assert got.get(scope, 0) == chunks(L), (scope, got)
        assert lost_set_classes(BAD) == 2 and got.get("direct_pass_set", 0) == lost_set_classes(BAD), got
        # the closing list verify over the L repaired stripes: every block is read, whatever pattern is named
        assert got.get("fingerprint_batch_list", 0) == chunks(L) and got.get("scrub_syndromes_batch", 0) == chunks(L), got
        assert got.get("scrub_transform_batch", 0) == LOCATE_SET_CHUNKS + 2 * chunks(L), got
        assert got.get("fingerprint", 0) == 0, got
        hd, hp = pool.read()
        assert np.array_equal(hd, want_d) and np.array_equal(hp, want_p)  # the clean codewords, absent blocks included; the other stripes untouched


@pytest.mark.parametrize("S,skew", SHAPES)
def test_correct_batch_set_grouped_with_a_word_above_p(torch_cuda, fe, codewords, S, skew):
    big = 3  # the flagged list's second chunk is this stripe alone: no locator there, no root search; the stripe is left to the single-stripe code
    d, p, want_d, want_p = degraded(codewords, S, big=big)
    batched = L - 1  # the stripes the grouped path repairs
    with open_set_encoder(fe, S) as enc:
        enc.set_option("correct_batch_mode", 1)
        pool = Pool(torch_cuda, d, p, skew)
        status, got = launches(enc, lambda: enc.correct_batch_set(pool.D, pool.Q, COUNT, LOCATE_PATTERN_OF, seed=SEED))
        assert status.tolist() == [1 if b in BAD else 0 for b in range(COUNT)]
        assert got.get("fingerprint_set", 0) == LOCATE_SET_CHUNKS and got.get("scrub_syndromes_set", 0) == LOCATE_SET_CHUNKS, got
        assert got.get("fingerprint_set_list", 0) == chunks(L) and got.get("scrub_syndromes_gather_set", 0) == chunks(L), got
        flagged = sorted(BAD)
        with_locator = len({i // CHUNK for i, b in enumerate(flagged) if b != big})
        assert with_locator == 1 and got.get("scrub_root_search_batch", 0) == with_locator, got
        assert got.get("direct_pass_set", 0) == lost_set_classes(b for b in BAD if b != big), got
        # the stripe is missing from the closing list
        assert got.get("fingerprint_batch_list", 0) == chunks(batched) and got.get("scrub_syndromes_batch", 0) == chunks(batched), got
        assert got.get("scrub_transform_batch", 0) == LOCATE_SET_CHUNKS + chunks(L) + chunks(batched), got
        assert got.get("fingerprint", 0) == 2, got  # correct_stripe on the one stripe: its location and its closing verify
        hd, hp = pool.read()
        assert np.array_equal(hd, want_d) and np.array_equal(hp, want_p)
