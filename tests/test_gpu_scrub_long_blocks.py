"""GPU tests (-m gpu) of the scrub fingerprint pass on long blocks, against the exact model of tests/scrub_model.py.

Every scrub call starts with one pass over the codeword (block_fingerprint, fastecc_amd/csrc/scrub.hip); the other suites run it on
blocks of 8 to 64 words (once 1024) and see it through one boolean per stripe.  Here the probe fastecc_scrub_fingerprints returns the
numbers and they must equal the model's, at the lengths where the pass takes another path: a second trip of the vector form's loop
(256 words per load, 1024 per trip), a ragged last trip, the periodic fold of the 64-bit lane sums (4096 products per lane: blocks of
2^18 words), the scalar form (a length that is no multiple of 4, or a pointer that misses 16-byte alignment) beyond one step per lane,
more blocks than resident waves, and the batch and list kernels.  The end-to-end tests then corrupt words at positions above 1023.

Codewords come from the CPU oracle (or are the constant stripe all p - 1, a codeword of the (2k,k) codes), never from the library's
encoder: a failure here is a scrub failure.  Every comparison is equality of integers.  fastecc_create refuses none of the block
lengths used, so none is left out."""
import numpy as np
import pytest

import scrub_model as sm

pytestmark = pytest.mark.gpu

P = sm.P
SEED = 0x5EED
LONG = 786437  # the longest block; the weights of every shorter one are a prefix of its weights
FOLD_VECTOR, FOLD_SCALAR = 786436, 786437  # the all-(p - 1) block overflows a 64-bit lane sum without the fold (asserted below)

WEIGHTS = {}


def weights(S, seed=SEED):
    if seed not in WEIGHTS:
        w = sm.weights(seed, LONG)
        w.setflags(write=False)
        WEIGHTS[seed] = w
    return WEIGHTS[seed][:S]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def fe(hip_lib):
    import fastecc_amd
    return fastecc_amd


def to_dev(torch, a, offset_words=0):
    """The words of `a` on the device; offset_words = 1: in a slice that starts 4 bytes into an allocation (not 16-byte aligned)."""
    flat = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
    t = torch.empty(flat.size + offset_words, dtype=torch.int32, device="cuda:0")[offset_words:]
    t.copy_(torch.from_numpy(flat.view(np.int32)))
    assert t.data_ptr() % 16 == 4 * offset_words
    return t


def host(t):
    return t.cpu().numpy().view(np.uint32).copy()


def i32(v):
    return v - (1 << 32) if v >= (1 << 31) else v


def assert_needs_fold(S, form):
    sums = sm.lane_sums(np.full(S, P - 1, np.uint32), weights(S), form)
    assert max(max(lane) for lane in sums) >= 1 << 64, (S, form)


# ---- a. the probe against the model, one stripe of the (4,2) code ----

LENGTHS = [1, 3, 4, 63, 64, 65, 252, 256, 260, 1020, 1024, 1028, 1029, 2052, 4099, 262144, 262148, 786436, 786437]


def four_blocks(S, rng):
    """random words below p; all p - 1; p - 1 and 0 alternating; random words below p (the block that later gets words >= p)"""
    b = np.empty((4, S), np.uint32)
    b[0] = rng.integers(0, P, size=S, dtype=np.uint64)
    b[1] = P - 1
    b[2] = np.where(np.arange(S) % 2 == 0, P - 1, 0)
    b[3] = rng.integers(0, P, size=S, dtype=np.uint64)
    return b


def plant_big(blocks, rng):
    out = blocks.copy()
    S = out.shape[1]
    for w in (0, S // 2, S - 1):
        out[3, w] = P + int(rng.integers(0, (1 << 32) - P))
    out[3, S - 1] = 0xFFFFFFFF
    return out


def probe_single(torch, fe, S, rng, data_offset=0, parity_offset=0):
    with fe.Encoder(4, 2, 4 * S) as enc:
        clean = four_blocks(S, rng)
        for blocks, want_big in ((clean, False), (plant_big(clean, rng), True)):
            data, parity = to_dev(torch, blocks[:2], data_offset), to_dev(torch, blocks[2:], parity_offset)
            got, big = enc.scrub_fingerprints(data, parity, seed=SEED)
            want = sm.fingerprints(blocks, SEED, weights(S))
            assert got.shape == (1, 4, 3) and got.dtype == np.uint32
            assert got[0].tolist() == want.tolist(), "S = %d, words >= p planted: %s" % (S, want_big)
            assert big.tolist() == [want_big]


@pytest.mark.parametrize("S", LENGTHS)
def test_probe_matches_model(torch_cuda, fe, S):
    if S == FOLD_VECTOR:
        assert_needs_fold(S, sm.VECTOR)
    if S == FOLD_SCALAR:
        assert_needs_fold(S, sm.SCALAR)
    probe_single(torch_cuda, fe, S, np.random.default_rng(S))


@pytest.mark.parametrize("which", ["data", "parity"])
@pytest.mark.parametrize("S", [1028, 2052, 786436])
def test_probe_matches_model_misaligned_pointer(torch_cuda, fe, S, which):
    """A multiple-of-4 length behind a pointer that is 4 bytes off 16-byte alignment: the scalar form, which torch allocations never select."""
    if S == 786436:
        assert_needs_fold(S, sm.SCALAR)  # 786436 = 64 * 12288 + 4: a lane's share is that of S = 786437 up to one product
    probe_single(torch_cuda, fe, S, np.random.default_rng(S + 1), data_offset=int(which == "data"), parity_offset=int(which == "parity"))


# ---- b. every word position of a block ----

@pytest.mark.parametrize("S", [2052, 2051])
def test_position_sweep(torch_cuda, fe, S):
    """Block j of the (4096,2048) code is zero except word j % S = v_j: its fingerprints are rho_c[j % S] * v_j mod p, so a word that the
    pass reads with the wrong weight, twice or not at all shows by its position."""
    torch, rng = torch_cuda, np.random.default_rng(S)
    n, k = 4096, 2048
    j = np.arange(n)
    pos = j % S
    v = np.array([1, P - 1, 1 << 31, 0], np.uint64)[j % 4]
    v[j % 4 == 3] = rng.integers(1, P, size=n // 4, dtype=np.uint64)
    blocks = np.zeros((n, S), np.uint32)
    blocks[j, pos] = v
    assert set(pos.tolist()) == set(range(S))  # every position is hit
    want = ((weights(S)[pos] * v[:, None]) % np.uint64(P)).astype(np.uint32)  # < 2^20 * 2^32
    with fe.Encoder(n, k, 4 * S) as enc:
        got, big = enc.scrub_fingerprints(to_dev(torch, blocks[:k]), to_dev(torch, blocks[k:]), seed=SEED)
    wrong = sorted(set(pos[(got[0] != want).any(axis=1)].tolist()))
    assert not wrong, "S = %d: %d word positions with a wrong fingerprint, the first at %s" % (S, len(wrong), wrong[:16])
    assert big.tolist() == [False]


# ---- c. more blocks than resident waves ----

def test_more_blocks_than_waves(torch_cuda, fe):
    """(16384,8192): 16384 blocks for at most 6 waves per SIMD of every compute unit, so each wave's loop over blocks takes several trips."""
    torch, rng = torch_cuda, np.random.default_rng(3)
    n, k, S = 16384, 8192, 4
    blocks = rng.integers(0, P, size=(n, S), dtype=np.uint64).astype(np.uint32)
    with fe.Encoder(n, k, 4 * S) as enc:
        got, big = enc.scrub_fingerprints(to_dev(torch, blocks[:k]), to_dev(torch, blocks[k:]), seed=SEED)
    want = sm.fingerprints(blocks, SEED, weights(S))
    wrong = np.nonzero((got[0] != want).any(axis=1))[0]
    assert wrong.size == 0, "%d blocks with a wrong fingerprint, the first %s" % (wrong.size, wrong[:16].tolist())
    assert big.tolist() == [False]


# ---- d. the batch and list forms ----

def batch_case(torch, fe, n, k, S, count, chunk=0, offset=0):
    rng = np.random.default_rng([n, S, count, chunk, offset])
    pool = rng.integers(0, P, size=(count, n, S), dtype=np.uint64).astype(np.uint32)
    pool[0, 0] = P - 1  # a saturated block: at the long length these kernels' own fold is needed too (assert_needs_fold's input)
    with_big = sorted(set([1, count - 1]))  # stripes in which one block holds a word >= p
    for b in with_big:
        pool[b, (3 * b + 1) % n, (S // 2 + b) % S] = 0xFFFFFFFF - b
    want = sm.fingerprints(pool, SEED, weights(S))
    want_big = [b in with_big for b in range(count)]
    D, Q = to_dev(torch, pool[:, :k], offset), to_dev(torch, pool[:, k:], offset)
    dw, pw = k * S, (n - k) * S
    with fe.Encoder(n, k, 4 * S) as enc:
        if chunk:
            enc.set_option("scrub_batch_chunk", chunk)
        got, big = enc.scrub_fingerprints(D, Q, count=count, form=1, seed=SEED)
        assert got.shape == (count, n, 3)
        assert np.array_equal(got, want), "batch form: stripes %s differ from the model" % np.nonzero((got != want).any(axis=(1, 2)))[0][:16].tolist()
        assert big.tolist() == want_big
        order = [int(b) for b in rng.permutation(count)]
        order.insert(len(order) // 2, order[0])  # one stripe named twice
        got, big = enc.scrub_fingerprints(D, Q, form=2, stripes=order, seed=SEED)
        assert got.shape == (count + 1, n, 3)
        assert np.array_equal(got, want[order]), "list form: entries %s differ from the model" % np.nonzero((got != want[order]).any(axis=(1, 2)))[0][:16].tolist()
        assert big.tolist() == [want_big[b] for b in order]
        for b in range(count):  # the single-stripe pass on each stripe alone (the slices of a misaligned pool stay misaligned: S is even)
            one, one_big = enc.scrub_fingerprints(D[b * dw:(b + 1) * dw], Q[b * pw:(b + 1) * pw], seed=SEED)
            assert np.array_equal(one[0], want[b]), "form 0, stripe %d" % b
            assert one_big.tolist() == [want_big[b]]


@pytest.mark.parametrize("n,k,S,count", [(4, 2, 2052, 5), (4, 2, 2051, 5), (4, 2, 786436, 3), (256, 128, 16, 300)])
def test_batch_and_list_forms(torch_cuda, fe, n, k, S, count):
    batch_case(torch_cuda, fe, n, k, S, count)


def test_batch_and_list_forms_in_chunks_of_two(torch_cuda, fe):
    batch_case(torch_cuda, fe, 4, 2, 2052, 5, chunk=2)


def test_batch_and_list_forms_misaligned_pointers(torch_cuda, fe):
    batch_case(torch_cuda, fe, 4, 2, 2052, 5, offset=1)


# ---- e. end to end on long blocks ----

POSITIONS = [0, 3, 255, 256, 1023, 1024, 1027, 2047, 2048]
LONG_POSITIONS = [262143, 262144, 524288, 786431, 786432]
N8, K8 = 8, 4


def positions_for(S):
    return POSITIONS + [S - 1] + (LONG_POSITIONS if S > 786432 else [])


def block_for(i):
    """The block the i-th position's corruption goes to: data and parity blocks in turn."""
    return (i // 2) % K8 if i % 2 == 0 else K8 + (i // 2) % (N8 - K8)


@pytest.fixture(scope="module")
def codewords(oracle):
    """(data, parity) host arrays of the (8,4) code per (kind, S), made once by the CPU oracle."""
    made = {}

    def get(kind, S):
        if (kind, S) not in made:
            if kind == "saturated":
                d = np.full((K8, S), P - 1, np.uint32)
            else:
                d = np.random.default_rng(S).integers(0, P, size=(K8, S), dtype=np.uint64).astype(np.uint32)
            p = oracle.encode_fast(d)
            if kind == "saturated":
                assert (p == P - 1).all()  # the constant stripe is a codeword
            made[(kind, S)] = (d, p)
        return made[(kind, S)]
    return get


def changed(old, i):
    """Another word below p."""
    new = (int(old) + 1 + (0x9E3779B1 * (i + 1)) % (P - 1)) % P
    assert new != int(old) and new < P
    return new


@pytest.mark.parametrize("kind", ["random", "saturated"])
@pytest.mark.parametrize("S", [2052, 2051, 786436, 786437])
def test_end_to_end_single_stripe(torch_cuda, fe, codewords, S, kind):
    """One changed word at a time, at the edges of the loads, trips and folds of the pass: detected, located in its block, corrected."""
    torch = torch_cuda
    positions = positions_for(S)
    w = weights(S)
    assert all(w[pos].any() for pos in positions)  # a word whose three weights are all zero cannot be detected: none of these is one
    if kind == "saturated" and S in (FOLD_VECTOR, FOLD_SCALAR):
        assert_needs_fold(S, sm.VECTOR if S % 4 == 0 else sm.SCALAR)
    d, p = codewords(kind, S)
    data, parity = to_dev(torch, d), to_dev(torch, p)
    d0, p0 = data.clone(), parity.clone()
    with fe.Encoder(N8, K8, 4 * S) as enc:
        assert enc.verify(data, parity, seed=SEED)
        assert enc.locate_errors(data, parity, seed=SEED) == []
        for i, pos in enumerate(positions):
            j = block_for(i)
            buf, at = (data, j * S + pos) if j < K8 else (parity, (j - K8) * S + pos)
            old = int(buf[at].item()) & 0xFFFFFFFF
            buf[at] = i32(changed(old, i))
            torch.cuda.synchronize()
            assert not enc.verify(data, parity, seed=SEED), "word %d of block %d" % (pos, j)
            assert enc.locate_errors(data, parity, seed=SEED) == [j], "word %d of block %d" % (pos, j)
            if i in (0, len(positions) - 1):
                assert enc.correct(data, parity, seed=SEED) == [j], "word %d of block %d" % (pos, j)
                torch.cuda.synchronize()
            else:
                buf[at] = i32(old)
            assert torch.equal(d0, data) and torch.equal(p0, parity), "word %d of block %d" % (pos, j)
        assert enc.verify(data, parity, seed=SEED + 1)


@pytest.mark.parametrize("kind", ["random", "saturated"])
def test_end_to_end_pool(torch_cuda, fe, codewords, kind):
    """One pool at S = 2052 whose stripe b carries the b-th position's corruption: the batched calls."""
    torch, S = torch_cuda, 2052
    positions = positions_for(S)
    count = len(positions)
    assert all(weights(S)[pos].any() for pos in positions)
    d, p = codewords(kind, S)
    pd, pp = np.tile(d, (count, 1, 1)), np.tile(p, (count, 1, 1))
    D0, Q0 = to_dev(torch, pd), to_dev(torch, pp)
    for b, pos in enumerate(positions):
        j = block_for(b)
        row = pd[b, j] if j < K8 else pp[b, j - K8]
        row[pos] = changed(row[pos], b)
    D, Q = to_dev(torch, pd), to_dev(torch, pp)
    with fe.Encoder(N8, K8, 4 * S) as enc:
        assert enc.verify_batch(D0, Q0, count, seed=SEED).all()
        assert not enc.verify_batch(D, Q, count, seed=SEED).any()
        status, lists = enc.locate_errors_batch(D, Q, count, seed=SEED)
        assert status.tolist() == [1] * count
        assert lists == [[block_for(b)] for b in range(count)]
        assert enc.correct_batch(D, Q, count, seed=SEED).tolist() == [1] * count
        torch.cuda.synchronize()
        assert torch.equal(D, D0) and torch.equal(Q, Q0)
