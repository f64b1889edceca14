"""GPU tests (-m gpu) of GF(0xFFF00001) on stripes whose butterflies sit where add, sub and mul_mont flip their decisions.

gf.hpp is canonical everywhere; add takes the wrapped value when x + y carried out of 32 bits or x + y + (2^20 - 1) carried, sub adds p when it
borrowed, mul_mont adds p when hi - q borrowed.  Each decision flips at an exact equality (x + y in {p - 1, p, p + 1, 2^32 - 1, 2^32, 2^32 + 1},
x - y in {-1, 0, 1}, hi == q) that uniformly random stripes — all the other GPU tests of this field feed — meet with probability 2^-29 per
butterfly.  Here
  * the element-wise probe fastecc_gf_binary runs add, sub, mul and mul_mont on the full grid of tests/p32_edges.py's BOUNDARY_PAIRS, and
    mul_mont on non-canonical x, against Python integers;
  * encode under every plan, the stand-alone transform, scale_blocks, the other code layouts, the mixed-radix orders, the decoders, scrub and
    update run on the stripes of tests/p32_edges.py — structured columns whose butterflies are (a, a), (a, p - a), (1, 0), (p - 1, 0), and
    targeted columns in which the pairs of one level are drawn from BOUNDARY_PAIRS — against the oracle.
Every comparison is equality of integers, every result canonical (< p); failures name the columns."""
import functools
import random

import numpy as np
import pytest

import p32_edges as pe
from p32_edges import P
from test_gpu_cosets import oracle_parity
from test_gpu_general import expected as zero_extended_parity
from test_gpu_parity import test_every_plan_is_bit_exact as _plans_test

pytestmark = pytest.mark.gpu

S = 70   # words per block: one full 64-lane chunk and a ragged one
ERASED = 0xFFFFFFFF
# every plan id of test_every_plan_is_bit_exact, and the default
PLANS = [0] + [m.args[1] for m in _plans_test.pytestmark if m.name == "parametrize"][0]
ENCODE_LOGN = (4, 7, 11, 13)
# 16-word-per-lane ("slim") outer tiles exist for 8- and 9-level chunks only: k = 2^16 is the smallest size that plans them (ids 2080, 3080,
# 4080); narrower blocks there so that the stripe is built within the model's budget
SLIM_LOGN, SLIM_S, SLIM_PLANS = 16, 40, (2080, 3080, 4080)
MIXED_Q = (3, 5, 7, 9, 13, 15, 21, 35, 39, 45, 63, 65, 91, 105, 117)


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
    return torch.from_numpy(np.array(a, dtype=np.uint32).view(np.int32)).to("cuda:0")   # a copy: the cached stripes are read-only


def to_host(t):
    return t.cpu().numpy().view(np.uint32)


@functools.lru_cache(maxsize=None)
def edge_stripe(logn, words=S):
    """(stripe, column names): built once per size and shared, never written to.  From 2^12 blocks on the targeted columns are capped so
    that the backward model stays near 10^6 butterflies; the structured columns are always all there."""
    columns, names = pe.edge_stripe(1 << logn, words, budget=10**6 if logn >= 12 else None)
    x = pe.stripe_array(columns)
    x.setflags(write=False)
    return x, names


@functools.lru_cache(maxsize=None)
def edge_parity(logn, words=S):
    import oracle
    par = oracle.Oracle().encode_fast(edge_stripe(logn, words)[0])
    par.setflags(write=False)
    return par


@functools.lru_cache(maxsize=None)
def structured_stripe(N, words=S):
    """structured_columns(N) for any order N | p - 1 (tones of the full order), then random fill: (stripe, names)."""
    cols = pe.structured_columns(N)
    names = [name for name, _ in cols] + ["random %d" % c for c in range(words - len(cols))]
    x = np.empty((N, words), dtype=np.uint32)
    x[:, :len(cols)] = pe.stripe_array([col for _, col in cols])
    x[:, len(cols):] = np.random.default_rng(N).integers(0, P, size=(N, words - len(cols)), dtype=np.uint64).astype(np.uint32)
    x.setflags(write=False)
    return x, names


def assert_same(got, want, names, what):
    """Bit-exact and canonical; a failure names the columns."""
    got = np.asarray(got).reshape(want.shape)
    if not (got == want).all():
        bad = sorted(int(c) for c in np.flatnonzero((got != want).any(axis=0)))
        raise AssertionError("%s: %d words differ, in columns %s" % (what, int((got != want).sum()), [names[c] if c < len(names) else c for c in bad][:12]))
    assert (got < np.uint32(P)).all(), what + ": not canonical"


# ------------------------------------------------------------------------------------------------
# the probe: add, sub, mul, mul_mont on the grid of boundary pairs
# ------------------------------------------------------------------------------------------------
def probe(torch, enc, op, xs, ys):
    dx, dy = to_dev(torch, np.array(xs, dtype=np.uint32)), to_dev(torch, np.array(ys, dtype=np.uint32))
    out = torch.full_like(dx, -1)
    enc.gf_binary(op, dx, dy, out, len(xs))
    torch.cuda.synchronize()
    return [int(v) for v in to_host(out)]


@pytest.mark.parametrize("op", ["add", "sub", "mul", "mul_mont"])
def test_probe_on_boundary_pairs(torch_cuda, fe, op):
    """Every pair of BOUNDARY_PAIRS both ways round (each of the six sums and three differences at least four times), then 2^16 random
    pairs: the result is the Python integers' and < p."""
    rng = random.Random(len(op))
    pairs = pe.BOUNDARY_PAIRS + [(b, a) for a, b in pe.BOUNDARY_PAIRS] + [(rng.randrange(P), rng.randrange(P)) for _ in range(1 << 16)]
    fn = {"add": lambda a, b: (a + b) % P, "sub": lambda a, b: (a - b) % P, "mul": lambda a, b: a * b % P, "mul_mont": lambda a, b: a * b % P}[op]
    with fe.Encoder(4, 2, 4) as enc:
        got = probe(torch_cuda, enc, op, [a for a, _ in pairs], [b for _, b in pairs])
    wrong = [(hex(a), hex(b), hex(g), hex(fn(a, b))) for (a, b), g in zip(pairs, got) if g != fn(a, b)]
    assert not wrong, (op, len(wrong), wrong[:6])


def test_probe_mul_mont_takes_any_32_bit_word(torch_cuda, fe):
    """gf.hpp: "x may be any uint32".  x over p, p + 1, 2^32 - 2, 2^32 - 1 and the canonical edge words, y over 0, 1, p - 1, 2^20 - 1 (2^32 mod
    p) and the roots of order 2, 4, 8, 16 with their inverses: x y mod p, canonical.  x = p and x = 0 are the products with hi == q."""
    xs = [P, P + 1, 0xFFFFFFFE, 0xFFFFFFFF] + pe.EDGE_A
    ys = [0, 1, P - 1, (1 << 20) - 1]
    for order in (2, 4, 8, 16):
        ys += [pe.root(order), pe.inv(pe.root(order))]
    pairs = [(x, y) for x in xs for y in ys]
    with fe.Encoder(4, 2, 4) as enc:
        got = probe(torch_cuda, enc, "mul_mont", [x for x, _ in pairs], [y for _, y in pairs])
    wrong = [(hex(x), hex(y), hex(g), hex(x * y % P)) for (x, y), g in zip(pairs, got) if g != x * y % P]
    assert not wrong, (len(wrong), wrong[:6])
    assert all(g < P for g in got)


# ------------------------------------------------------------------------------------------------
# encode under every plan
# ------------------------------------------------------------------------------------------------
def encode_both_ways(torch, enc, x, want, names, what):
    d = to_dev(torch, x)
    out = torch.full_like(d, -1)
    enc.encode(d, out)
    torch.cuda.synchronize()
    assert_same(to_host(out), want, names, "encode %s %s" % (what, enc.plan()))
    assert (to_host(d).reshape(x.shape) == x).all(), "out-of-place encode must not touch its input"
    enc.encode(d)   # in place
    torch.cuda.synchronize()
    assert_same(to_host(d), want, names, "encode in place %s %s" % (what, enc.plan()))


@pytest.mark.parametrize("plan", PLANS)
def test_encode_of_edge_stripes(torch_cuda, fe, plan):
    """The default plan and every id of test_every_plan_is_bit_exact at k = 2^4, 2^7, 2^11, 2^13 (what they select:
    test_the_encode_cases_reach_every_kernel_family): the parity of the structured and targeted columns is the oracle's, word for word and
    canonical, out of place and in place."""
    for logn in ENCODE_LOGN:
        x, names = edge_stripe(logn)
        with fe.Encoder(2 << logn, 1 << logn, 4 * S) as enc:
            enc.set_plan(plan)
            enc.set_option("encode_direct_max", 0)   # up to 160 parity blocks (k = 2^4, 2^7) the default is the direct encode, whatever the plan
            encode_both_ways(torch_cuda, enc, x, edge_parity(logn), names, "k=2^%d plan %d" % (logn, plan))


@pytest.mark.parametrize("plan", SLIM_PLANS)
def test_encode_of_edge_stripes_through_slim_outer_tiles(torch_cuda, fe, plan):
    x, names = edge_stripe(SLIM_LOGN, SLIM_S)
    with fe.Encoder(2 << SLIM_LOGN, 1 << SLIM_LOGN, 4 * SLIM_S) as enc:
        enc.set_plan(plan)
        assert "S32:dif8@8" in enc.plan() and "S32:dit8@8" in enc.plan(), enc.plan()
        encode_both_ways(torch_cuda, enc, x, edge_parity(SLIM_LOGN, SLIM_S), names, "k=2^16 plan %d" % plan)


def test_the_encode_cases_reach_every_kernel_family(torch_cuda, fe):
    """What the plans of the two tests above select, read from the contexts themselves (fastecc_plan_string): register passes of 1..5 levels
    with 1, 2 and 4 words per lane; the MID tile with 32-word rows (a pair tile: v_permlane32_swap levels) of 7..10 levels and with 64-word rows
    (the plan ids' wide flag; a plain tile, no swap) of 6..9; outer pair tiles (T32, and S32 with 16 words per lane) and outer plain tiles
    (T64).  (The tiles of several address windows need blocks of 16 KiB at k = 2^18: test_windowed_tiles_for_blocks_spanning_4_to_32_gib.)"""
    passes = set()
    for logn, words, plans in [(logn, S, PLANS) for logn in ENCODE_LOGN] + [(SLIM_LOGN, SLIM_S, SLIM_PLANS)]:
        with fe.Encoder(2 << logn, 1 << logn, 4 * words) as enc:
            for plan in plans:
                enc.set_plan(plan)
                text, vec = enc.plan().split(" v")
                passes |= {(p.split("@")[0], int(vec)) for p in text.split(",")}
    kinds = {name for name, _ in passes}
    for levels in range(1, 6):
        assert {"dif%d" % levels, "dit%d" % levels, "mid%d" % levels} <= kinds, (levels, sorted(kinds))            # register passes
    assert {vec for name, vec in passes if ":" not in name} == {1, 2, 4}
    assert {"T32:mid%d" % m for m in (7, 8, 9, 10)} | {"T64:mid%d" % m for m in (6, 7, 8, 9)} <= kinds, sorted(kinds)   # pair and wide MID tiles
    assert {"T32:dif7", "T32:dit7", "S32:dif8", "S32:dit8"} <= kinds, sorted(kinds)                                # outer pair tiles
    assert {"T64:dif6", "T64:dit6"} <= kinds, sorted(kinds)                                                        # outer plain tiles


# ------------------------------------------------------------------------------------------------
# stand-alone transform and scale_blocks
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", [4, 9])
def test_ntt_and_scale_blocks_of_edge_stripes(torch_cuda, fe, oracle, logn):
    torch = torch_cuda
    N = 1 << logn
    x, names = edge_stripe(logn)
    with fe.Encoder(2 * N, N, 4 * S) as enc:
        for inverse in (False, True):
            d = to_dev(torch, x)
            enc.ntt(d, inverse)
            torch.cuda.synchronize()
            assert_same(to_host(d), oracle.ntt_fast(x, inverse), names, "ntt k=2^%d inverse=%s" % (logn, inverse))
        # the encoder's factors w_2N^i / N, and factors that are boundary words themselves: -1^i, and 2^32 mod p times the powers of w_4
        for scale, base in ((pe.inv(N), pe.root(2 * N)), (P - 1, P - 1), ((1 << 20) - 1, pe.root(4)), (1, 1)):
            d = to_dev(torch, x)
            enc.scale_blocks(d, scale, base)
            torch.cuda.synchronize()
            assert_same(to_host(d), oracle.scale_blocks(x, scale, base), names, "scale_blocks k=2^%d (%#x, %#x)" % (logn, scale, base))


# ------------------------------------------------------------------------------------------------
# other code layouts
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [2, 3])
def test_coset_parity_of_edge_stripes(torch_cuda, fe, oracle, e):
    """n = 4k and n = 8k at k = 64."""
    torch = torch_cuda
    N, rows = 64, ((1 << e) - 1) * 64
    x, names = edge_stripe(6)
    with fe.Encoder(N << e, N, 4 * S) as enc:
        out = torch.full((rows * S,), -1, dtype=torch.int32, device="cuda:0")
        enc.encode(to_dev(torch, x), out)
        torch.cuda.synchronize()
        assert_same(to_host(out), oracle_parity(oracle, x, e), names, "n = %dk %s" % (1 << e, enc.plan()))


def profiled(torch, enc, call):
    enc.profile(True)
    enc.profile_reset()
    call()
    torch.cuda.synchronize()
    prof = enc.profile_read()
    enc.profile(False)
    return prof


@pytest.mark.parametrize("k,m,logn", [(64, 16, 6), (128, 32, 7), (100, 30, 7), (1000, 300, 10), (1024, 64, 10), (1024, 160, 10)])
def test_fewer_parity_blocks_and_zero_extension(torch_cuda, fe, oracle, k, m, logn):
    """n = k + k / 2^d, zero-extended (n, k) with k no power of two (the first k blocks of the edge stripe), and codes with at most 160 parity
    blocks: through the transform pipeline (encode_direct_max = 0) and, where the code has at most 160 parity blocks, through the single-pass
    direct encode by the matrix-core kernel and by the VALU kernel — all the oracle's parity of the zero-padded stripe."""
    torch = torch_cuda
    full, names = edge_stripe(logn)
    x = np.ascontiguousarray(full[:k])
    want = zero_extended_parity(oracle, x, m)
    with fe.Encoder(k + m, k, 4 * S) as enc:
        for direct_max, kernel in ((0, 0), (160, 2), (160, 1), (160, 0)):
            enc.set_option("encode_direct_max", direct_max)
            enc.set_option("direct_kernel", kernel)
            d = to_dev(torch, x)
            out = torch.full((m * S,), -1, dtype=torch.int32, device="cuda:0")
            prof = profiled(torch, enc, lambda: enc.encode(d, out))
            assert ("direct_encode" in prof) == (direct_max != 0 and m <= 160), (direct_max, kernel, prof)
            assert_same(to_host(out), want, names, "(%d, %d) encode_direct_max %d kernel %d %s" % (k + m, k, direct_max, kernel, enc.plan()))
            assert (to_host(d).reshape(x.shape) == x).all()


# ------------------------------------------------------------------------------------------------
# mixed radix
# ------------------------------------------------------------------------------------------------
def mixed_case(torch, fe, oracle, q, m, fused, words=S):
    k = q << m
    pfa = q not in fe.MIXED_RADIX_Q
    assert fe.mixed_radix_order(k, pfa=pfa) == k
    x, names = structured_stripe(k, words)
    want = oracle.encode_mixed(x)
    with fe.Encoder(2 * k, k, 4 * words, flags=fe.CODE_MIXED_RADIX_PFA if pfa else fe.CODE_MIXED_RADIX) as enc:
        # the kernel kind, so that a planner change cannot silently drop coverage: R<q>+ is the odd-radix level fused into the outer tile,
        # R<q>: the stand-alone radix kernel around the power-of-two pipeline
        assert (("R%d+dif" % q) in enc.plan()) == fused and (("R%d:dif1" % q) in enc.plan()) == (not fused), enc.plan()
        enc.set_option("encode_direct_max", 0)   # (the orders up to 160 would be encoded directly, without the radix kernels)
        encode_both_ways(torch, enc, x, want, names, "order %d * 2^%d" % (q, m))


@pytest.mark.parametrize("q", MIXED_Q)
def test_mixed_radix_stand_alone_radix_kernel(torch_cuda, fe, oracle, q):
    """Order q 2^3: sym_dft and the vmadd chains of the odd-radix kernels on columns whose partial sums cancel (constants, impulses, tones of
    the full order q 2^m, periodic patterns)."""
    mixed_case(torch_cuda, fe, oracle, q, 3, fused=False)


@pytest.mark.parametrize("q", [q for q in MIXED_Q if q <= 63])
def test_mixed_radix_fused_kernel(torch_cuda, fe, oracle, q):
    """Order q 2^11, the smallest with an outer chunk above the 10-level MID tile and so the smallest at which the fused kernel is planned
    (q = 65, 91, 105, 117 have no fused shape).  34 words per block (the structured columns and a few random ones, a ragged row): the oracle's
    q-point transforms by definition are what takes the time here."""
    mixed_case(torch_cuda, fe, oracle, q, 11, fused=True, words=34)


# ------------------------------------------------------------------------------------------------
# decoders
# ------------------------------------------------------------------------------------------------
def flags_of(lost, k, m):
    lost = np.asarray(lost)
    dp, pp = np.ones(k, np.uint8), np.ones(m, np.uint8)
    dp[lost[lost < k]] = 0
    pp[lost[lost >= k] - k] = 0
    return dp, pp


def decode_and_repair(torch, enc, x, par, dp, pp, names, what):
    """Erased blocks hold 0xFFFFFFFF.  decode restores the data and leaves the parity alone, repair restores both."""
    bad_x, bad_p = x.copy(), par.copy()
    bad_x[dp == 0] = ERASED
    bad_p[pp == 0] = ERASED
    enc.decode_prepare(dp, pp)
    d, q = to_dev(torch, bad_x), to_dev(torch, bad_p)
    prof = profiled(torch, enc, lambda: enc.decode(d, q))
    assert_same(to_host(d), x, names, what + " decode")
    assert (to_host(q).reshape(par.shape) == bad_p).all(), what + ": decode wrote to the parity"
    d = to_dev(torch, bad_x)
    enc.repair(d, q)
    torch.cuda.synchronize()
    assert_same(to_host(d), x, names, what + " repair, data")
    assert_same(to_host(q), par, names, what + " repair, parity")
    return prof


def test_decoder_with_k_blocks_lost(torch_cuda, fe):
    """(2k,k) at k = 2^7 with k blocks lost, data and parity mixed, and with all data lost."""
    N = 128
    x, names = edge_stripe(7)
    par = edge_parity(7)
    rng = np.random.default_rng(71)
    with fe.Encoder(2 * N, N, 4 * S) as enc:
        for trial in range(2):
            dp, pp = flags_of(rng.permutation(2 * N)[:N], N, N)
            decode_and_repair(torch_cuda, enc, x, par, dp, pp, names, "k blocks lost, trial %d" % trial)
        decode_and_repair(torch_cuda, enc, x, par, np.zeros(N, np.uint8), np.ones(N, np.uint8), names, "all data lost")


def test_decoder_with_two_percent_lost(torch_cuda, fe):
    """k = 2^11, 2 % of the codeword lost (81 blocks): as the library decodes it by default, with decode_split = 0, and through the
    transforms (decode_direct_max = 0), with and without the split.  (In this field the split transform is planned from k = 2^17:
    test_split_decoder_at_its_smallest_size.)"""
    N = 1 << 11
    x, names = edge_stripe(11)
    par = edge_parity(11)
    dp, pp = flags_of(np.random.default_rng(111).permutation(2 * N)[: 2 * N // 50], N, N)
    assert (dp == 0).any() and (pp == 0).any()
    with fe.Encoder(2 * N, N, 4 * S) as enc:
        for split, direct_max in ((1, 256), (0, 256), (1, 0), (0, 0)):
            enc.set_option("decode_split", split)
            enc.set_option("decode_direct_max", direct_max)
            prof = decode_and_repair(torch_cuda, enc, x, par, dp, pp, names, "2 %% lost, decode_split %d, decode_direct_max %d" % (split, direct_max))
            assert ("direct_pass" in prof) == (direct_max != 0), prof


def test_split_decoder_at_its_smallest_size(torch_cuda, fe):
    """k = 2^17 (the smallest k whose decoder runs the two half-size transforms), 2 % lost, 32-word blocks: the split path, then again with
    decode_split = 0."""
    logn, words = 17, 32
    N = 1 << logn
    x, names = edge_stripe(logn, words)
    par = edge_parity(logn, words)
    dp, pp = flags_of(np.random.default_rng(17).permutation(2 * N)[: 2 * N // 50], N, N)
    with fe.Encoder(2 * N, N, 4 * words) as enc:
        for split in (1, 0):
            enc.set_option("decode_split", split)
            prof = decode_and_repair(torch_cuda, enc, x, par, dp, pp, names, "k = 2^17, decode_split %d" % split)
            assert ("decode_split_transform" in prof) == (split == 1) and ("decode_transform_2k" in prof) == (split == 0), prof


@pytest.mark.parametrize("nlost", [1, 16, 32])
def test_direct_path_under_both_kernels(torch_cuda, fe, nlost):
    """k = 2^11: 1, 16 and 32 lost blocks, data and parity mixed, by the VALU kernel (96-bit lazy sums) and the MFMA kernel (signed base-256
    digits), against the original stripes and the transform path (decode_direct_max = 0)."""
    N = 1 << 11
    x, names = edge_stripe(11)
    par = edge_parity(11)
    rng = np.random.default_rng(nlost)
    lost = rng.permutation(2 * N)[:nlost]
    if nlost > 1:
        lost[0], lost[1] = int(rng.integers(N)), N + int(rng.integers(N))
        lost = np.unique(lost)
    else:
        lost[0] = int(rng.integers(N))
    dp, pp = flags_of(lost, N, N)
    with fe.Encoder(2 * N, N, 4 * S) as enc:
        for kernel, direct_max in ((1, 256), (2, 256), (0, 0)):
            enc.set_option("direct_kernel", kernel)
            enc.set_option("decode_direct_max", direct_max)
            prof = decode_and_repair(torch_cuda, enc, x, par, dp, pp, names, "%d lost, direct_kernel %d, decode_direct_max %d" % (nlost, kernel, direct_max))
            assert ("direct_pass" in prof) == (direct_max != 0), prof


def test_n_equals_4k_decoder(torch_cuda, fe, oracle):
    """n = 4k at k = 64 with 3k blocks lost."""
    N, e = 64, 2
    x, names = edge_stripe(6)
    par = oracle_parity(oracle, x, e)
    dp, pp = flags_of(np.random.default_rng(64).permutation(4 * N)[: 3 * N], N, 3 * N)
    assert (dp == 0).any()
    with fe.Encoder(N << e, N, 4 * S) as enc:
        decode_and_repair(torch_cuda, enc, x, par, dp, pp, names, "n = 4k decoder")


# ------------------------------------------------------------------------------------------------
# scrub on sparse codewords
# ------------------------------------------------------------------------------------------------
SEED = 0x5EED


def test_scrub_on_sparse_codewords(torch_cuda, fe):
    """verify finds the all-zero stripe and the edge stripe consistent; one corrupted word in a block of the all-zero codeword, of a tone
    column and of the all-(p - 1) column is located and corrected (syndromes of a single non-zero term; the fingerprints of the zero
    codeword are all zero); verify_batch / correct_batch on one stripe give the same answers."""
    torch = torch_cuda
    N = 128
    x, names = edge_stripe(7)
    par = edge_parity(7)
    tone, ones = names.index("tone f=1"), names.index("all p-1")
    zero = np.zeros_like(x)
    with fe.Encoder(2 * N, N, 4 * S) as enc:
        for what, cx, cp in (("zero stripe", zero, zero), ("edge stripe", x, par)):
            d, q = to_dev(torch, cx), to_dev(torch, cp)
            assert enc.verify(d, q, seed=SEED), what
            assert enc.locate_errors(d, q, seed=SEED) == [], what
            assert enc.verify_batch(d, q, 1, seed=SEED).tolist() == [True], what
            assert enc.correct_batch(d, q, 1, seed=SEED).tolist() == [0], what
            assert (to_host(d).reshape(cx.shape) == cx).all() and (to_host(q).reshape(cp.shape) == cp).all(), what
        cases = [("zero codeword, data", zero, zero, 5, 3, 1), ("zero codeword, parity", zero, zero, N + 77, 69, P - 1),
                 ("tone column, data", x, par, 100, tone, None), ("tone column, parity", x, par, N + 1, tone, None),
                 ("all p-1 column, data", x, par, 0, ones, 0), ("all p-1 column, parity", x, par, 2 * N - 1, ones, P - 2)]
        for what, cx, cp, block, col, value in cases:
            bx, bp = cx.copy(), cp.copy()
            row = bx[block] if block < N else bp[block - N]
            row[col] = (int(row[col]) + 1) % P if value is None else value
            assert row[col] != (cx[block] if block < N else cp[block - N])[col]
            for batched in (False, True):
                d, q = to_dev(torch, bx), to_dev(torch, bp)
                if batched:
                    assert enc.verify_batch(d, q, 1, seed=SEED).tolist() == [False], what
                    assert enc.correct_batch(d, q, 1, seed=SEED).tolist() == [1], what
                else:
                    assert not enc.verify(d, q, seed=SEED), what
                    assert enc.locate_errors(d, q, seed=SEED) == [block], what
                    assert enc.correct(d, q, seed=SEED) == [block], what
                torch.cuda.synchronize()
                assert_same(to_host(d), cx, names, what + ", data, batched=%s" % batched)
                assert_same(to_host(q), cp, names, what + ", parity, batched=%s" % batched)


# ------------------------------------------------------------------------------------------------
# update
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 16])
def test_update_equals_a_reencode(torch_cuda, fe, oracle, t):
    """fastecc_update after replacing t blocks of the edge stripe — by the blocks half a stripe away (the periodic columns do not change: differences
    of exactly zero), the first of them by zeros — equals the encode of the new stripe."""
    torch = torch_cuda
    N = 128
    x, names = edge_stripe(7)
    blocks = [int(b) for b in np.random.default_rng(t).permutation(N)[:t]]
    new = np.stack([x[(b + N // 2) % N] for b in blocks])
    new[0] = 0
    after = x.copy()
    after[blocks] = new
    with fe.Encoder(2 * N, N, 4 * S) as enc:
        d, q = to_dev(torch, x), to_dev(torch, edge_parity(7))
        enc.update(d, q, blocks, to_dev(torch, new))
        torch.cuda.synchronize()
        assert_same(to_host(d), after, names, "update t=%d, data" % t)
        assert_same(to_host(q), oracle.encode_fast(after), names, "update t=%d, parity" % t)
