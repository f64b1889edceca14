"""CPU tests of tests/p61_edges.py — the generators of the edge-of-range inputs for the 64-bit field and the expected values of its
device probe.  They check the generators, not the library: the exact model against the oracle, backwards against forwards, the
targeted columns against their targets, and the condition that keeps the structured inputs honest (most of their intermediate words
lie where a lazy word is not canonical, while a random column's never do)."""
import os
import random
import re

import numpy as np
import pytest

import p61_edges as pe
from p61_edges import P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1 << n for n in range(1, 8)]
# every stripe size tests/test_gpu_p61_edges.py uses
GPU_SIZES = [16, 64, 128, 512, 1024, 2048, 4096, 8192]


@pytest.fixture(scope="module")
def orc61():
    import oracle
    return oracle.OracleP61()


def columns_for(N):
    return [col for _, col in pe.structured_columns(N)] + [pe.random_column(N, s) for s in range(2)]


def test_roots_are_the_headers(orc61):
    assert pe.root(4) == (0, 1) and pe.root(8) == (1 << 30, 1 << 30)   # include/fastecc.h: w_4 = i, w_8 = 2^30 (1 + i)
    for t in (1, 2, 3, 4, 10, 20, 62):
        assert pe.root(1 << t) == orc61.root(1 << t)
    x, y = (123456789012345678, P - 1), (5, 77)
    assert pe.mulc(x, y) == orc61.cmul(x, y) and pe.invc(x) == orc61.cinv(x) and pe.powc(x, 12345) == orc61.cpow(x, 12345)


@pytest.mark.parametrize("N", SIZES)
def test_model_ends_where_the_oracle_does(orc61, N):
    cols = columns_for(N)
    x = pe.stripe_array(cols)
    enc, fwd, inv = orc61.encode(x), orc61.ntt(x), orc61.ntt(x, True)
    for c, col in enumerate(cols):
        states = pe.run_forward(col, pe.encode_plan(N))
        assert len(states) == 2 * pe.ilog2(N) + 1
        assert states[-1] == pe.column_of(enc, c), (N, c)
        assert pe.run_forward(col, pe.ntt_plan(N))[-1] == pe.column_of(fwd, c), (N, c)
        assert pe.run_forward(col, pe.ntt_plan(N, True))[-1] == pe.column_of(inv, c), (N, c)


@pytest.mark.parametrize("N", [2, 16, 64])
@pytest.mark.parametrize("e", [2, 3])
def test_coset_model_is_the_oracles_composition(orc61, N, e):
    from test_gpu_p61 import p61_coset_generators, p61_oracle_coset_parity
    gens = pe.coset_generators(N, e)
    assert gens == p61_coset_generators(orc61, N, e)
    cols = columns_for(N)
    want = p61_oracle_coset_parity(orc61, pe.stripe_array(cols), e)
    for c, col in enumerate(cols):
        got = [v for g in gens for v in pe.run_forward(col, pe.encode_plan(N, g))[-1]]
        assert got == pe.column_of(want, c), (N, e, c)


@pytest.mark.parametrize("N", SIZES)
def test_backward_then_forward_is_the_identity(N):
    plans = [pe.encode_plan(N), pe.ntt_plan(N), pe.ntt_plan(N, True), pe.encode_plan(N, pe.coset_generators(N, 3)[-1])]
    for col in columns_for(N)[-4:]:   # period 4, small words, two random columns: nothing the zero short cut hides
        for plan in plans:
            states = pe.run_forward(col, plan)
            for stop in range(1, len(plan) + 1):
                assert pe.run_backward(states[stop - 1], plan, stop) == col, (N, stop)
            assert pe.run_forward(pe.run_backward(col, plan, len(plan)), plan)[-1] == col


@pytest.mark.parametrize("N", [2, 16, 64, 128])
def test_targeted_columns_meet_their_targets(N):
    n = pe.ilog2(N)
    cols = pe.targeted_columns(N)
    assert [(hf, T) for hf, T, _, _ in cols] == [("dif", T) for T in range(n - 1, -1, -1)] + [("dit", T) for T in range(n)]
    plan = pe.encode_plan(N)
    for hf, T, col, target in cols:
        assert all(0 <= w < P for v in col for w in v)                      # a canonical input
        assert all(w in pe.EDGE_WORDS for v in target for w in v)
        idx = pe.stage_index(N, T, hf)
        assert plan[idx][:2] == (hf, T)
        entering = col if idx == 0 else pe.run_forward(col, plan)[idx - 1]
        assert entering == target, (N, hf, T)                                # word for word
        assert pe.targeted_columns(N, T, hf)[0][2] == col                    # the single-column form builds the same column
    # a budget drops whole columns, DIT levels of the largest strides first, and keeps the others as they are
    few = pe.targeted_columns(N, budget=pe.targeted_cost(N, 0, "dit") + sum(pe.targeted_cost(N, T, "dif") for T in range(n)))
    assert [c[:2] for c in few] == [("dif", T) for T in range(n - 1, -1, -1)] + [("dit", 0)]
    assert all(a[2] == b[2] for a, b in zip(few, cols))


def test_edge_words_cover_both_zones():
    assert all(w < pe.ZONE or w >= P - pe.ZONE or w in (1 << 33, 1 << 60) for w in pe.EDGE_WORDS)
    assert all(w < pe.LAZY_LIMIT for w in pe.LAZY_EDGE_WORDS) and max(pe.LAZY_EDGE_WORDS) == pe.LAZY_LIMIT - 1
    assert sum(w >= P for w in pe.LAZY_EDGE_WORDS) >= 5 and all((1 << 62) <= w < (1 << 64) for w in pe.RAW_EDGE_WORDS)
    assert 7 * (1 << 61) + (1 << 34) in pe.RAW_EDGE_WORDS   # 3.5 * 2^62 + 2^34: the largest loose difference mul_raw is handed


@pytest.mark.parametrize("N", GPU_SIZES)
def test_structured_columns_live_in_the_edge_zone(N):
    """The condition that keeps the inputs honest.  Measured over the words the DIF half computes (n levels x N elements x 2):
    every family but 'constant' and 'small words' puts at least half of them in [0, 2^33) or [p - 2^33, p) — at N = 64: tones 642 / 768,
    unit impulses at odd positions 550 / 768, all p - 1 768 / 768 — and a random column none at all."""
    cols = pe.structured_columns(N)
    names = [name for name, _ in cols]
    assert len(names) == len(set(names)) >= 20
    for name, col in cols:
        assert len(col) == N and all(0 <= w < P for v in col for w in v), name
        if name in ("constant", "small words"):
            continue
        assert pe.edge_share(pe.dif_half_states(col)) >= 0.5, (N, name)
    if N == 64:
        share = {name: pe.edge_share(pe.dif_half_states(col)) for name, col in cols}
        assert share["all p-1"] == 1.0 and share["zero"] == 1.0
        assert share["impulse 1 at 1"] == 550 / 768
        assert all(share[name] == 642 / 768 for name in names if name.startswith("tone"))
        assert pe.edge_share(pe.dif_half_states(pe.random_column(64))) == 0.0


def test_edge_stripe_layout():
    N, elems = 16, 70
    columns, names = pe.edge_stripe(N, elems)
    assert len(columns) == len(names) == elems
    nstruct = len(pe.structured_columns(N))
    assert names[nstruct:nstruct + 8] == ["target dif %d" % T for T in (3, 2, 1, 0)] + ["target dit %d" % T for T in range(4)]
    assert names[nstruct + 8] == "random 0" and names[-1].startswith("random")
    x = pe.stripe_array(columns)
    assert x.shape == (N, 2 * elems) and x.dtype == np.uint64 and (x < P).all()
    assert pe.column_of(x, 3) == columns[3]


# ---- the device probe's expected values ----
def naive_dft(xs, inverse):
    R = len(xs)
    w = pe.root(R)
    if inverse:
        w = pe.invc(w)
    out = []
    for j in range(R):
        acc = (0, 0)
        for c, v in enumerate(xs):
            acc = pe.addc(acc, pe.mulc(v, pe.powc(w, j * c)))
        out.append(acc)
    return out


def test_probe_formulas():
    rng = random.Random(3)
    words = pe.LAZY_EDGE_WORDS + pe.RAW_EDGE_WORDS + [rng.randrange(1 << 64) for _ in range(20)]
    for _ in range(200):
        x, y = (rng.choice(words), rng.choice(words)), (rng.randrange(P), rng.randrange(P))
        a, b = x[0] % P, x[1] % P
        assert pe.probe_expected("add", x, y) == ((x[0] + y[0]) % P, (x[1] + y[1]) % P)
        assert pe.probe_expected("sub", x, y) == ((x[0] - y[0]) % P, (x[1] - y[1]) % P)
        assert pe.probe_expected("mul", x, y) == pe.probe_expected("mul_raw", x, y) == ((a * y[0] - b * y[1]) % P, (a * y[1] + b * y[0]) % P)
        # w_8 = 2^30 (1 + i): x w_8 = 2^30 ((a - b) + (a + b) i); w_8^3 = i w_8; the inverse roots are the conjugates
        w8 = ((a - b) << 30) % P, ((a + b) << 30) % P
        assert pe.probe_expected("mul_w8", x) == w8
        assert pe.probe_expected("mul_w8i", x) == (-w8[1] % P, w8[0])
        assert pe.mulc(pe.probe_expected("mul_w8_inv", x), pe.root(8)) == (a, b)
        assert pe.mulc(pe.probe_expected("mul_w8i_inv", x), pe.powc(pe.root(8), 3)) == (a, b)
        assert pe.probe_expected("fold", x) == pe.probe_expected("canon", x) == (a, b)


@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_run_model_is_the_small_transform(L):
    R = 1 << L
    rng = random.Random(L)
    xs = [(rng.choice(pe.LAZY_EDGE_WORDS), rng.randrange(pe.LAZY_LIMIT)) for _ in range(R)]
    canon = [(v[0] % P, v[1] % P) for v in xs]
    rev = [pe.bitrev(j, L) for j in range(R)]
    for op, inverse in (("run_dif", False), ("run_dif_inv", True)):
        want = naive_dft(canon, inverse)
        assert pe.run_expected(op, xs) == [want[rev[j]] for j in range(R)]           # result in bit-reversed order
    assert pe.run_expected("run_dit", [xs[rev[j]] for j in range(R)]) == naive_dft(canon, False)   # input in bit-reversed order


def test_bound_table_and_op_codes():
    """Every result of the probe is lazy again (what any lazy-input op accepts), canon's is canonical; the names are those of the
    wrapper and their codes those of include/fastecc.h."""
    import fastecc_amd
    assert set(pe.PROBE_BOUNDS) == set(pe.ELEMENT_OPS) | set(pe.RUN_OPS) == set(fastecc_amd.Encoder.GF61_OPS)
    assert all(b <= pe.LAZY_LIMIT for b in pe.PROBE_BOUNDS.values()) and pe.PROBE_BOUNDS["canon"] == P
    # the folds: a 64-bit t gives (t mod 2^61) + (t >> 61) <= 2^61 - 1 + 7; lazy + lazy and lazy + 2p - lazy have t >> 61 <= 2 and <= 3
    assert pe.FOLDED == (1 << 61) - 1 + ((1 << 64) - 1 >> 61) + 2
    assert pe.PROBE_BOUNDS["add"] == (1 << 61) - 1 + (2 * (pe.LAZY_LIMIT - 1) >> 61) + 1 == (1 << 61) + 2
    assert pe.PROBE_BOUNDS["sub"] == (1 << 61) - 1 + (pe.LAZY_LIMIT - 1 + 2 * P >> 61) + 1 == (1 << 61) + 3
    # rot30 of x < 2^63: (x mod 2^31) 2^30 + (x >> 31) < 2^61 + 2^32
    assert pe.PROBE_BOUNDS["mul_w8"] == ((1 << 31) - 1 << 30) + ((1 << 63) - 1 >> 31) + 1 + (1 << 30)
    text = open(os.path.join(ROOT, "include", "fastecc.h")).read()
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"FASTECC_GF61_OP_([A-Z0-9_]+) = (\d+)", text)}
    assert codes == fastecc_amd.Encoder.GF61_OPS
