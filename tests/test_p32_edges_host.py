"""CPU tests of tests/p32_edges.py — the generators of the boundary-event inputs for GF(0xFFF00001).  They check the generators, not the
library: the exact model against the oracle, backwards against forwards, the targeted columns against their targets, and the condition that
keeps the structured inputs honest (at least half of the butterflies of their DIF half are boundary events, while a random column has none)."""
from fractions import Fraction

import numpy as np
import pytest

import p32_edges as pe
from p32_edges import P

SIZES = [1 << n for n in range(1, 8)]
# every power-of-two stripe size tests/test_gpu_p32_edges.py builds structured columns at
GPU_SIZES = [16, 64, 128, 512, 1024, 2048, 4096, 8192, 1 << 16, 1 << 17]
# ... and the mixed-radix orders (no radix-2 DIF half to measure: the columns are only checked for shape and range)
MIXED_SIZES = [q << 3 for q in (3, 5, 7, 9, 13, 15, 21, 35, 39, 45, 63, 65, 91, 105, 117)] + [3 << 11, 63 << 11]


def columns_for(N):
    return [col for _, col in pe.structured_columns(N)] + [pe.random_column(N, s) for s in range(2)]


def test_roots_are_the_oracles(oracle):
    assert pe.root(2) == P - 1 and pe.root(1) == 1
    for order in (2, 4, 8, 16, 1 << 10, 1 << 20, 3, 9, 5, 7, 13, 3 << 4, 117 << 11, 4095 << 20):
        assert pe.root(order) == oracle.gf_root(order) and pow(pe.root(order), order, P) == 1
    x = 0xFEDCBA98
    assert pe.inv(x) == oracle.gf_inv(x) and pe.HALF * 2 % P == 1


@pytest.mark.parametrize("N", SIZES)
def test_model_ends_where_the_oracle_does(oracle, N):
    cols = columns_for(N)
    x = pe.stripe_array(cols)
    enc, fwd, inv = oracle.encode_fast(x), oracle.ntt_fast(x), oracle.ntt_fast(x, True)
    for c, col in enumerate(cols):
        states = pe.run_forward(col, pe.encode_plan(N))
        assert len(states) == 2 * pe.ilog2(N) + 1
        assert states[-1] == pe.column_of(enc, c), (N, c)
        assert pe.run_forward(col, pe.ntt_plan(N))[-1] == pe.column_of(fwd, c), (N, c)
        assert pe.run_forward(col, pe.ntt_plan(N, True))[-1] == pe.column_of(inv, c), (N, c)


@pytest.mark.parametrize("N", [2, 16, 64])
@pytest.mark.parametrize("e", [2, 3])
def test_coset_model_is_the_oracles_composition(oracle, N, e):
    from test_gpu_cosets import coset_generators, oracle_parity
    gens = pe.coset_generators(N, e)
    assert gens == coset_generators(oracle, N, e)
    cols = columns_for(N)
    want = oracle_parity(oracle, pe.stripe_array(cols), e)
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


@pytest.mark.parametrize("N", [2, 16, 64, 128, 512])
def test_targeted_columns_meet_their_targets(N):
    n = pe.ilog2(N)
    cols = pe.targeted_columns(N)
    assert [(hf, T) for hf, T, _, _ in cols] == [("dif", T) for T in range(n - 1, -1, -1)] + [("dit", T) for T in range(n)]
    plan = pe.encode_plan(N)
    for hf, T, col, target in cols:
        assert all(0 <= w < P for w in col)                                  # a canonical input
        idx = pe.stage_index(N, T, hf)
        assert plan[idx][:2] == (hf, T)
        entering = col if idx == 0 else pe.run_forward(col, plan)[idx - 1]
        assert entering == target, (N, hf, T)                                # word for word
        pairs = pe.level_pairs(entering, plan[idx])                          # what that level's add and sub see
        assert len(pairs) == N // 2 and all(pr in pe.BOUNDARY_PAIRS and pe.boundary_event(*pr) for pr in pairs), (N, hf, T)   # share 1.0
        if N // 2 >= len(pe.EVENT_PAIRS):   # every pair is dealt out: each equality is met in every column, and the DIT level's products
            assert set(pairs) == set(pe.EVENT_PAIRS)   # are 0, 1 and p - 1 among others
            assert {a + b for a, b in pairs} >= set(pe.EVENT_SUMS) and {a - b for a, b in pairs} >= set(pe.EVENT_DIFFS)
            assert {0, 1, P - 1} <= {b for _, b in pairs}
        assert pe.targeted_columns(N, T, hf)[0][2] == col                    # the single-column form builds the same column
    # a budget drops whole columns, DIT levels of the largest strides first, and keeps the others as they are
    few = pe.targeted_columns(N, budget=pe.targeted_cost(N, 0, "dit") + sum(pe.targeted_cost(N, T, "dif") for T in range(n)))
    assert [c[:2] for c in few] == [("dif", T) for T in range(n - 1, -1, -1)] + [("dit", 0)]
    assert all(a[2] == b[2] for a, b in zip(few, cols))


def test_boundary_pairs_cover_every_equality():
    pairs = pe.BOUNDARY_PAIRS
    assert len(pairs) == len(set(pairs)) and all(0 <= a < P and 0 <= b < P for a, b in pairs)
    for s in pe.EVENT_SUMS:
        assert sum(a + b == s for a, b in pairs) >= 4, hex(s)
    for d in pe.EVENT_DIFFS:
        assert sum(a - b == d for a, b in pairs) >= 4, d
    assert (P - 1, P - 1) in pairs and (0, 0) in pairs and (1, P - 1) in pairs and (1 << 31, 1 << 31) in pairs
    assert sum(a == 0 for a, _ in pairs) >= 12 and sum(b == 0 for _, b in pairs) >= 12
    assert pe.EVENT_PAIRS == [pr for pr in pairs if pe.boundary_event(*pr)] and len(pe.EVENT_PAIRS) >= 100
    # the definition itself, on its borders
    assert pe.boundary_event(5, P - 5) and pe.boundary_event(5, P - 6) and pe.boundary_event(5, P - 4) and not pe.boundary_event(5, P - 7)
    assert pe.boundary_event(1 << 31, 1 << 31) and pe.boundary_event((1 << 31) + 1, 1 << 31) and not pe.boundary_event((1 << 31) + 2, 1 << 31)
    assert pe.boundary_event(7, 7) and pe.boundary_event(7, 8) and pe.boundary_event(8, 7) and not pe.boundary_event(7, 9)
    assert pe.boundary_event(P - 1, P - 1) and pe.boundary_event(0, 0) and not pe.boundary_event((1 << 20) - 1, 0)


@pytest.mark.parametrize("N", [16, 64, 128])
def test_the_two_counters_agree(N):
    for col in columns_for(N) + [c[2] for c in pe.targeted_columns(N)]:
        assert pe.event_counts_np(col) == pe.event_counts(col)
        events, total = pe.event_counts(col)
        assert pe.event_share(col) == (events / total if total else 1.0)


@pytest.mark.parametrize("N", GPU_SIZES)
def test_structured_columns_are_made_of_boundary_events(N):
    """The condition that keeps the inputs honest.  Measured over the butterflies of the encode's DIF half that have a non-zero operand: in
    every family but the impulses at odd positions and 'small words' (kept as plain cases) at least half are boundary events, and in a
    random column none.  At N = 64, of 63 live butterflies: constants, all p - 1, tones, 'a, -a alternating' and the impulses at 0 and N/2
    63 / 63; period 2 31 / 32; period 4 46 / 49; impulses of 1 and p - 1 at odd positions 6 / 63, of 2^20 - 1 none; small words 17 / 192.
    (The impulses of 2^20 - 1 at EVEN positions measured 0 / 63 — paired with zeros that word is no boundary event — so that family gave way
    to the constant columns of 2^31 and 2^20 - 1: 2 * 2^31 is the carry out of 32 bits, and both walk through 2^k (2^20 - 1).)"""
    cols = pe.structured_columns(N)
    names = [name for name, _ in cols]
    assert len(names) == len(set(names)) >= 20
    for name, col in cols:
        assert len(col) == N and all(0 <= w < P for w in col), name
        if pe.is_plain_case(name, N):
            continue
        events, total = pe.event_counts_np(col)
        assert total == 0 or Fraction(events, total) >= Fraction(1, 2), (N, name, events, total)
    for s in range(3):
        assert pe.event_counts_np(pe.random_column(N, s))[0] == 0
    if N == 64:
        share = {name: Fraction(*pe.event_counts(col)) if any(col) else None for name, col in cols}
        assert share["zero"] is None and pe.event_share(cols[0][1]) == 1.0
        ones = ["all p-1", "constant", "constant 2^31", "constant 2^20-1", "a, -a alternating", "impulse 1 at 0", "impulse 1 at 32",
                "impulse p-1 at 0", "impulse p-1 at 32"] + [name for name in names if name.startswith("tone")]
        assert len(ones) == 14 and all(share[name] == 1 and pe.event_counts(dict(cols)[name]) == (63, 63) for name in ones)
        assert share["period 2"] == Fraction(31, 32) and share["period 4"] == Fraction(46, 49)
        assert share["impulse 1 at 1"] == share["impulse p-1 at 63"] == Fraction(6, 63)
        assert share["impulse 2^20-1 at 1"] == share["impulse 2^20-1 at 63"] == 0
        assert share["small words"] == Fraction(17, 192)
        assert pe.event_share(pe.random_column(64)) == 0.0
    if N == 16:
        assert pe.event_counts(dict(cols)["period 2"]) == (7, 8) and pe.event_counts(dict(cols)["period 4"]) == (10, 13)


@pytest.mark.parametrize("N", MIXED_SIZES)
def test_structured_columns_of_mixed_radix_orders(N):
    cols = pe.structured_columns(N)
    names = [name for name, _ in cols]
    assert len(names) == len(set(names)) >= 20 and "tone f=%d" % (N - 1) in names and "tone f=%d" % (N // 2) in names
    w = pe.root(N)
    assert pow(w, N, P) == 1 and pow(w, N // 2, P) == P - 1
    for name, col in cols:
        assert len(col) == N and all(0 <= v < P for v in col), name
        if name.startswith("tone"):
            f = int(name.split("=")[1])
            assert col[1] == col[0] * pow(w, f, P) % P and col[N - 1] * pow(w, f, P) % P == col[0]   # a tone of the full order


def test_edge_stripe_layout():
    N, S = 16, 70
    columns, names = pe.edge_stripe(N, S)
    assert len(columns) == len(names) == S
    nstruct = len(pe.structured_columns(N))
    assert names[nstruct:nstruct + 8] == ["target dif %d" % T for T in (3, 2, 1, 0)] + ["target dit %d" % T for T in range(4)]
    assert names[nstruct + 8] == "random 0" and names[-1].startswith("random")
    x = pe.stripe_array(columns)
    assert x.shape == (N, S) and x.dtype == np.uint32 and (x < P).all() and x.flags["C_CONTIGUOUS"]
    assert pe.column_of(x, 3) == columns[3]
    # the largest stripes of the GPU file fit their 70 columns under the budget rule, the structured columns all kept
    for n in (11, 13):
        cost = sum(pe.targeted_cost(1 << n, T, hf) for hf in ("dif", "dit") for T in range(n))
        assert (cost > 10**6) == (n == 13)
