"""GPU tests (-m gpu) of the 64-bit field's LAZY arithmetic at the edges of its ranges.

The transform code over GF((2^61-1)^2) keeps words lazy (in [0, 2^61 + 2^33)), uses unfolded "loose" sums and differences inside a run of
levels and plain 64-bit accumulators in the few-loss decoder; each step is right only while a bound holds.  Random stripes
(tests/test_gpu_p61.py) never come near those bounds.  Here
  * the device probe fastecc_gf61_binary runs every primitive and every register run on grids of edge words, lazy and raw, and the result
    is checked for its residue AND for the bound include/fastecc.h states;
  * encode, the stand-alone transform, the n = 4k / 8k codes and the decoders run on the stripes of tests/p61_edges.py, whose intermediate
    words are zeros, small values and values just below p, against the oracle.
Everything is bit-exact."""
import functools
import random

import numpy as np
import pytest

import p61_edges as pe
from p61_edges import P
from test_gpu_p61 import p61_oracle_coset_parity, to_dev, to_host

pytestmark = pytest.mark.gpu

ELEMS = 70   # one full 64-lane chunk and a ragged one


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
def orc61():
    import oracle
    return oracle.OracleP61()


@functools.lru_cache(maxsize=None)
def edge_stripe(logn):
    """(stripe, column names): built once per size and shared, never written to.  From 2^12 blocks on the targeted columns are capped so
    that the backward model stays near 10^6 butterflies."""
    columns, names = pe.edge_stripe(1 << logn, ELEMS, budget=10**6 if logn >= 12 else None)
    return pe.stripe_array(columns), names


@functools.lru_cache(maxsize=None)
def edge_parity(logn):
    import oracle
    return oracle.OracleP61().encode(edge_stripe(logn)[0])


def assert_same(got, want, names, what):
    got = got.reshape(want.shape)
    if (got == want).all():
        return
    bad = sorted({int(c) // 2 for c in np.flatnonzero((got != want).any(axis=0))})
    raise AssertionError("%s: %d words differ, in columns %s" % (what, int((got != want).sum()), [names[c] if c < len(names) else c for c in bad][:12]))


def encoder(fe, N, elems=ELEMS):
    return fe.Encoder(2 * N, N, 16 * elems, field=fe.FIELD_GF_P61_SQUARED)


# ------------------------------------------------------------------------------------------------
# the probe: every primitive on the full grid of edge words
# ------------------------------------------------------------------------------------------------
def twiddle_operands():
    """Canonical elements: 0, 1, i, p - 1, w_8, the four w_16 roots, their conjugates, and a grid of canonical edge words."""
    w16 = pe.root(16)
    special = [(0, 0), (1, 0), (0, 1), (P - 1, 0), (0, P - 1), (P - 1, P - 1), pe.root(8), pe.conj(pe.root(8))]
    special += [pe.powc(w16, m) for m in (1, 3, 5, 7)] + [pe.conj(pe.powc(w16, m)) for m in (1, 3, 5, 7)]
    words = [0, 1, (1 << 31) - 1, 1 << 31, (1 << 60) - 1, 1 << 60, P - 2, P - 1]
    return special + [(a, b) for a in words for b in words]


def probe_operands(op):
    """(x, y): lists of elements.  The full grid of edge words in both components of x — and of y for add / sub, y running over the canonical
    twiddles for the products — then 2^16 random operands."""
    rng = random.Random(sum(map(ord, op)))
    raw = op in pe.RAW_INPUT_OPS
    words = pe.LAZY_EDGE_WORDS + (pe.RAW_EDGE_WORDS if raw else [])
    grid = [(a, b) for a in words for b in words]
    rnd_x = (lambda: rng.randrange(1 << 64)) if raw else (lambda: rng.randrange(pe.LAZY_LIMIT))
    if op in ("add", "sub"):
        xs = [x for x in grid for _ in grid]
        ys = [y for _ in grid for y in grid]
        rnd_y = lambda: rng.randrange(pe.LAZY_LIMIT)
    elif op in ("mul", "mul_raw"):
        tw = twiddle_operands()
        xs = [x for x in grid for _ in tw]
        ys = [y for _ in grid for y in tw]
        rnd_y = lambda: rng.randrange(P)
    else:
        xs, ys, rnd_y = list(grid), None, None
    xs += [(rnd_x(), rnd_x()) for _ in range(1 << 16)]
    if ys is not None:
        ys += [(rnd_y(), rnd_y()) for _ in range(1 << 16)]
    return xs, ys


def elems_array(vs):
    return np.array([w for v in vs for w in v], dtype=np.uint64)


@pytest.mark.parametrize("op", pe.ELEMENT_OPS)
def test_probe_primitives_on_edge_words(torch_cuda, fe, op):
    """out = exact (mod p), out below the bound the header states for the op, canon of a lazy word below p."""
    xs, ys = probe_operands(op)
    want = elems_array([pe.probe_expected(op, x, ys[i] if ys else None) for i, x in enumerate(xs)])
    with encoder(fe, 4, 4) as enc:
        dx = to_dev(torch_cuda, elems_array(xs))
        dy = to_dev(torch_cuda, elems_array(ys)) if ys else None
        out = torch_cuda.full_like(dx, -1)
        enc.gf61_binary(op, dx, dy, out, len(xs))
        torch_cuda.cuda.synchronize()
        got = to_host(out)
    wrong = np.flatnonzero(got % np.uint64(P) != want)
    assert wrong.size == 0, (op, wrong.size, [(xs[i // 2], ys[i // 2] if ys else None, int(got[i]), int(want[i])) for i in wrong[:4]])
    bound = pe.PROBE_BOUNDS[op]
    over = np.flatnonzero(got >= np.uint64(bound))
    assert over.size == 0, (op, "bound 2^61 + %d" % (bound - (1 << 61)), [(xs[i // 2], ys[i // 2] if ys else None, int(got[i])) for i in over[:4]])
    if op == "canon":
        assert (got < np.uint64(P)).all() and (got == want).all()


@pytest.mark.parametrize("levels", [1, 2, 3, 4])
@pytest.mark.parametrize("op", pe.RUN_OPS)
def test_probe_register_runs_on_edge_words(torch_cuda, fe, op, levels):
    """dif_levels / dit_levels of 1..4 levels as the passes call them (loose outputs every other level, w_4 / w_8 / w_16 specialised) on 2^14 runs
    whose registers are lazy edge words and random lazy words: element for element against the 2^L-point model."""
    R, items = 1 << levels, 1 << 14
    rng = random.Random(levels * 10 + len(op))

    def word(kind):
        return rng.choice(pe.LAZY_EDGE_WORDS) if kind == 0 or (kind == 2 and rng.random() < 0.5) else rng.randrange(pe.LAZY_LIMIT)

    # a third of the runs: edge words only; a third: random lazy words only; the rest: mixed word by word
    xs = [(word(it % 3), word(it % 3)) for it in range(items) for _ in range(R)]
    want = []
    for it in range(items):
        want += pe.run_expected(op, xs[it * R:(it + 1) * R])
    want = elems_array(want)
    with encoder(fe, 4, 4) as enc:
        dx = to_dev(torch_cuda, elems_array(xs))
        out = torch_cuda.full_like(dx, -1)
        enc.gf61_binary(op, dx, None, out, len(xs), levels=levels)
        torch_cuda.cuda.synchronize()
        got = to_host(out)
    wrong = np.flatnonzero(got % np.uint64(P) != want)
    assert wrong.size == 0, (op, levels, wrong.size, [("run", int(i) // (2 * R), "register", int(i) // 2 % R, xs[(i // (2 * R)) * R:(i // (2 * R) + 1) * R]) for i in wrong[:2]])
    assert (got < np.uint64(pe.PROBE_BOUNDS[op])).all(), (op, levels, int(got.max()) - (1 << 61))


def test_probe_argument_checks(torch_cuda, fe):
    torch = torch_cuda
    d = torch.zeros(64, dtype=torch.int64, device="cuda:0")
    out = torch.zeros_like(d)
    with encoder(fe, 4, 4) as enc:
        for bad_op in (-1, 10, 15, 28, 1000):
            with pytest.raises(fe.FastEccError) as ei:
                enc.gf61_binary(bad_op, d, d, out, 32)
            assert ei.value.code == fe.E_INVAL, bad_op
        for x, y, o in ((None, d, out), (d, None, out), (d, d, None)):
            with pytest.raises(fe.FastEccError) as ei:
                enc.gf61_binary("mul", x, y, o, 32)
            assert ei.value.code == fe.E_INVAL
        with pytest.raises(fe.FastEccError) as ei:
            enc.gf61_binary("run_dif", d, None, out, 24, levels=4)   # 24 is no multiple of 16
        assert ei.value.code == fe.E_INVAL
        enc.gf61_binary("fold", d, None, out, 0)                      # nothing to do
    with fe.Encoder(8, 4, 64) as enc32:
        with pytest.raises(fe.FastEccError) as ei:
            enc32.gf61_binary("add", d, d, out, 32)
        assert ei.value.code == fe.E_UNSUPPORTED


# ------------------------------------------------------------------------------------------------
# transforms on the edge stripes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,plan", [(4, 0), (4, 4), (7, 0), (7, 4)] + [(logn, plan) for logn in (12, 13) for plan in (0, 4, 13, 24)])
def test_encode_of_edge_stripes(torch_cuda, fe, logn, plan):
    """MID-only plans (4: registers, 7: the tile), one and two tile chunks around MID (12, 13), register passes, tiles with a 64 and a 128 KiB
    exchange buffer: the parity of the structured and targeted columns is the oracle's, word for word, and canonical."""
    x, names = edge_stripe(logn)
    want = edge_parity(logn)
    with encoder(fe, 1 << logn) as enc:
        enc.set_plan(plan)
        d = to_dev(torch_cuda, x)
        out = torch_cuda.full_like(d, -1)
        enc.encode(d, out)
        got = to_host(out)
        assert (got < np.uint64(P)).all(), "parity words must be canonical"
        assert_same(got, want, names, "encode %s" % enc.plan())
        enc.encode(d)   # in place
        assert_same(to_host(d), want, names, "encode in place %s" % enc.plan())


@pytest.mark.parametrize("logn", [4, 9])
@pytest.mark.parametrize("inverse", [False, True])
def test_ntt_of_edge_stripes(torch_cuda, fe, orc61, logn, inverse):
    x, names = edge_stripe(logn)
    want = orc61.ntt(x, inverse)
    with encoder(fe, 1 << logn) as enc:
        d = to_dev(torch_cuda, x)
        enc.ntt(d, inverse=inverse)
        got = to_host(d)
        assert (got < np.uint64(P)).all()
        assert_same(got, want, names, "ntt inverse=%s" % inverse)


@pytest.mark.parametrize("e", [2, 3])
def test_coset_parity_of_edge_stripes(torch_cuda, fe, orc61, e):
    logn = 6
    N, rows = 1 << logn, ((1 << e) - 1) << logn
    x, names = edge_stripe(logn)
    want = p61_oracle_coset_parity(orc61, x, e)
    with fe.Encoder(N << e, N, 16 * ELEMS, field=fe.FIELD_GF_P61_SQUARED) as enc:
        out = torch_cuda.full((rows * 2 * ELEMS,), -1, dtype=torch_cuda.int64, device="cuda:0")
        enc.encode(to_dev(torch_cuda, x), out)
        got = to_host(out)
        assert (got < np.uint64(P)).all()
        assert_same(got, want, names, "n = %dk" % (1 << e))


# ------------------------------------------------------------------------------------------------
# decoders on the edge stripes
# ------------------------------------------------------------------------------------------------
def erase(x, par, dp, pp):
    bad_x, bad_p = x.copy(), par.copy()
    bad_x[dp == 0] = np.uint64(0xFFFFFFFFFFFFFFFF)   # erased blocks hold garbage
    bad_p[pp == 0] = np.uint64(0xDEADBEEFDEADBEEF)
    return bad_x, bad_p


def decode_and_repair(torch, enc, x, par, dp, pp, names, what):
    bad_x, bad_p = erase(x, par, dp, pp)
    enc.decode_prepare(dp, pp)
    d, q = to_dev(torch, bad_x), to_dev(torch, bad_p)
    enc.decode(d, q)
    torch.cuda.synchronize()
    assert_same(to_host(d), x, names, what + " decode")
    assert (to_host(q).reshape(par.shape) == bad_p).all()   # decode leaves the parity alone
    d = to_dev(torch, bad_x)
    enc.repair(d, q)
    torch.cuda.synchronize()
    assert_same(to_host(d), x, names, what + " repair, data")
    assert_same(to_host(q), par, names, what + " repair, parity")


def test_folded_decoder_on_edge_stripes(torch_cuda, fe):
    """(2k,k) at k = 2^7 with k blocks lost, data and parity mixed: the folded 2k-point transform, decode and repair."""
    logn = 7
    N = 1 << logn
    x, names = edge_stripe(logn)
    par = edge_parity(logn)
    rng = np.random.default_rng(71)
    for trial in range(2):
        lost = rng.permutation(2 * N)[:N]
        dp, pp = np.ones(N, np.uint8), np.ones(N, np.uint8)
        dp[lost[lost < N]] = 0
        pp[lost[lost >= N] - N] = 0
        with encoder(fe, N) as enc:
            decode_and_repair(torch_cuda, enc, x, par, dp, pp, names, "folded decoder, trial %d" % trial)
    dp, pp = np.zeros(N, np.uint8), np.ones(N, np.uint8)   # all data lost
    with encoder(fe, N) as enc:
        decode_and_repair(torch_cuda, enc, x, par, dp, pp, names, "folded decoder, all data lost")


def test_split_decoder_on_edge_stripes(torch_cuda, fe):
    """k = 2^11, 2 % of the blocks lost: the even / odd split (the profile shows its kernels) — and the folded transform on the same pattern."""
    logn = 11
    N = 1 << logn
    x, names = edge_stripe(logn)
    par = edge_parity(logn)
    rng = np.random.default_rng(111)
    for parity_too in (False, True):
        dp, pp = np.ones(N, np.uint8), np.ones(N, np.uint8)
        dp[rng.permutation(N)[: N // 50]] = 0
        if parity_too:
            pp[rng.permutation(N)[: N // 50]] = 0
        with encoder(fe, N) as enc:
            bad_x, bad_p = erase(x, par, dp, pp)
            enc.decode_prepare(dp, pp)
            enc.profile(True)
            enc.profile_reset()
            d = to_dev(torch_cuda, bad_x)
            enc.decode(d, to_dev(torch_cuda, bad_p))
            torch_cuda.cuda.synchronize()
            kernels = set(enc.profile_read())
            enc.profile(False)
            assert any(name.endswith("_add") for name in kernels), kernels   # the split's MID with the addend
            assert_same(to_host(d), x, names, "split decoder")
            decode_and_repair(torch_cuda, enc, x, par, dp, pp, names, "split decoder")
            enc.set_option("decode_split", 0)
            decode_and_repair(torch_cuda, enc, x, par, dp, pp, names, "folded transform at 2^11")


def test_n_equals_4k_decoder_on_edge_stripes(torch_cuda, fe, orc61):
    logn, e = 6, 2
    N, rows = 1 << logn, 3 << logn
    x, names = edge_stripe(logn)
    par = p61_oracle_coset_parity(orc61, x, e)
    rng = np.random.default_rng(64)
    lost = rng.permutation(4 * N)[: 3 * N]
    dp, pp = np.ones(N, np.uint8), np.ones(rows, np.uint8)
    dp[lost[lost < N]] = 0
    pp[lost[lost >= N] - N] = 0
    assert (dp == 0).any()
    with fe.Encoder(N << e, N, 16 * ELEMS, field=fe.FIELD_GF_P61_SQUARED) as enc:
        decode_and_repair(torch_cuda, enc, x, par, dp, pp, names, "n = 4k decoder")


@pytest.mark.parametrize("pattern", ["all p-1", "alternating"])
def test_few_loss_direct_path_at_the_top_of_its_accumulators(torch_cuda, fe, orc61, pattern):
    """N = 1024 (two full 512-row accumulation chunks), 9 elements: every data word p - 1, and p - 1 / 0 alternating over the blocks (the other way
    round in every second column) — the largest sums the 64-bit accumulators of the direct path meet.  1, 16 and 32 lost blocks, data and parity
    mixed, against the original stripes and against the transform path (decode_direct_max = 0)."""
    torch = torch_cuda
    N, elems = 1024, 9
    if pattern == "all p-1":
        x = np.full((N, 2 * elems), P - 1, dtype=np.uint64)
    else:
        x = np.zeros((N, 2 * elems), dtype=np.uint64)
        x[0::2, 0::4] = P - 1
        x[0::2, 1::4] = P - 1
        x[1::2, 2::4] = P - 1
        x[1::2, 3::4] = P - 1
    par = orc61.encode(x)
    names = ["column %d" % c for c in range(elems)]
    rng = np.random.default_rng(1024)
    with encoder(fe, N, elems) as enc:
        for nlost in (1, 16, 32):
            lost = rng.permutation(2 * N)[:nlost]
            if nlost > 1:
                lost[0], lost[1] = int(rng.integers(N)), N + int(rng.integers(N))   # data and parity mixed
                lost = np.unique(lost)
            dp, pp = np.ones(N, np.uint8), np.ones(N, np.uint8)
            dp[lost[lost < N]] = 0
            pp[lost[lost >= N] - N] = 0
            bad_x, bad_p = erase(x, par, dp, pp)
            got = {}
            for direct_max in (32, 0):
                enc.set_option("decode_direct_max", direct_max)
                enc.decode_prepare(dp, pp)
                d, q = to_dev(torch, bad_x), to_dev(torch, bad_p)
                enc.decode(d, q)
                torch.cuda.synchronize()
                got[direct_max] = to_host(d).reshape(x.shape).copy()
                assert_same(got[direct_max], x, names, "decode, %d lost, direct_max %d" % (nlost, direct_max))
                d = to_dev(torch, bad_x)
                enc.repair(d, q)
                torch.cuda.synchronize()
                assert_same(to_host(d), x, names, "repair data, %d lost, direct_max %d" % (nlost, direct_max))
                assert_same(to_host(q), par, names, "repair parity, %d lost, direct_max %d" % (nlost, direct_max))
            assert (got[32] == got[0]).all()
        enc.set_option("decode_direct_max", 32)
