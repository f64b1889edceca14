"""Inputs that put the 32-bit field's add / sub / mul_mont at the equalities where their decisions flip, and an exact model to build them with.

The device code over GF(p), p = 0xFFF00001 (gf.hpp), is canonical everywhere; its correctness rests on three decisions: add takes the wrapped
value when x + y carried out of 32 bits or x + y + (2^20 - 1) carried, sub adds p when it borrowed, mul_mont adds p when hi - q borrowed.  Each
flips at an exact equality — x + y in {p - 1, p, p + 1, 2^32 - 1, 2^32, 2^32 + 1}, x - y in {-1, 0, 1} — and a butterfly on uniformly random
words meets one of them with probability about 2^-29.  A BOUNDARY EVENT is a butterfly whose add and sub see such a pair.  The columns built
here make the butterflies of a transform boundary events:

  structured_columns(N)             constants, impulses, tones, periodic patterns: their transforms are sparse, so a level's pairs are (a, a),
                                    (a, p - a), (1, 0) or (p - 1, 0) almost everywhere
  targeted_columns(N, level, half)  the pairs the add and sub of ONE radix-2 level see are drawn from BOUNDARY_PAIRS and the input that
                                    produces them is found by running the model backwards

Everything here is exact arithmetic on Python integers; nothing of the library is used.  Plain helper module (no fixtures, no tests); it reads
like tests/p61_edges.py, the 64-bit field's counterpart."""
import functools
import random

P = 0xFFF00001
GENERATOR = 19
HALF = (P + 1) // 2     # 1 / 2 mod p
W32 = 1 << 32

# a butterfly is a boundary event when the sum or the difference of the pair its add and sub see is one of these
EVENT_SUMS = (P - 1, P, P + 1, W32 - 1, W32, W32 + 1)
EVENT_DIFFS = (-1, 0, 1)


def inv(x):
    return pow(x, P - 2, P)


@functools.lru_cache(maxsize=None)
def root(order):
    """The root of unity of order `order` (any divisor of p - 1 = 2^20 * 3^2 * 5 * 7 * 13): 19^((p-1)/order)."""
    assert order >= 1 and (P - 1) % order == 0, order
    return pow(GENERATOR, (P - 1) // order, P)


def bitrev(v, bits):
    r = 0
    for _ in range(bits):
        r = (r << 1) | (v & 1)
        v >>= 1
    return r


def ilog2(N):
    n = N.bit_length() - 1
    assert N == 1 << n and n >= 1
    return n


@functools.lru_cache(maxsize=None)
def level_twiddles(T, inverse):
    """w^m for m < 2^T, w the root of order 2^(T+1) (inverse: its inverse) — the twiddles of the radix-2 level of stride 2^T."""
    w = root(2 << T)
    if inverse:
        w = inv(w)
    out, cur = [], 1
    for _ in range(1 << T):
        out.append(cur)
        cur = cur * w % P
    return out


# ---- radix-2 levels on one column (a list of N words), forwards and backwards ----
def dif_level(x, T, inverse, backward=False):
    """Decimation in frequency, stride 2^T: (a, b) -> (a + b, (a - b) w^m).  backward: the level undone."""
    h = 1 << T
    tw = level_twiddles(T, not inverse if backward else inverse)
    y = list(x)
    for base in range(0, len(x), 2 * h):
        for m in range(h):
            a, b = x[base + m], x[base + m + h]
            if a == 0 and b == 0:
                continue
            if backward:
                t = b * tw[m] % P
                y[base + m], y[base + m + h] = (a + t) * HALF % P, (a - t) * HALF % P
            else:
                y[base + m], y[base + m + h] = (a + b) % P, (a - b) * tw[m] % P
    return y


def dit_level(x, T, inverse=False, backward=False):
    """Decimation in time, stride 2^T: (a, b) -> (a + b w^m, a - b w^m).  backward: the level undone."""
    h = 1 << T
    tw = level_twiddles(T, not inverse if backward else inverse)
    y = list(x)
    for base in range(0, len(x), 2 * h):
        for m in range(h):
            a, b = x[base + m], x[base + m + h]
            if a == 0 and b == 0:
                continue
            if backward:
                y[base + m], y[base + m + h] = (a + b) * HALF % P, (a - b) * HALF % P * tw[m] % P
            else:
                t = b * tw[m] % P
                y[base + m], y[base + m + h] = (a + t) % P, (a - t) % P
    return y


@functools.lru_cache(maxsize=None)
def block_factors(N, gen):
    """Position q holds coefficient c = bitrev(q) after the DIF half; its factor is gen^c / N (the encoder: gen = w_2N)."""
    n = ilog2(N)
    powers, cur = [], inv(N)
    for _ in range(N):
        powers.append(cur)
        cur = cur * gen % P
    return [powers[bitrev(q, n)] for q in range(N)]


@functools.lru_cache(maxsize=None)
def block_factors_inverse(N, gen):
    n = ilog2(N)
    ginv, powers, cur = inv(gen), [], N % P
    for _ in range(N):
        powers.append(cur)
        cur = cur * ginv % P
    return [powers[bitrev(q, n)] for q in range(N)]


def factor_stage(x, N, gen, backward=False):
    f = block_factors_inverse(N, gen) if backward else block_factors(N, gen)
    return [v * w % P for v, w in zip(x, f)]


def bitrev_stage(x):
    n = ilog2(len(x))
    return [x[bitrev(q, n)] for q in range(len(x))]


# ---- staged pipelines: a plan is a list of stages, every stage can run forwards and backwards ----
def encode_plan(N, gen=None):
    """The encode in the position order the kernels use: DIF levels with the inverse roots from stride N/2 down to 1 (natural order in,
    bit-reversed out), the factor gen^c / N on the position that holds coefficient c (gen = w_2N: the (2k,k) code; the coset
    generators of n = 4k / 8k otherwise), DIT levels with the forward roots from stride 1 up to N/2 (natural order out)."""
    n = ilog2(N)
    gen = gen or root(2 * N)
    return [("dif", T, True) for T in range(n - 1, -1, -1)] + [("factor", gen)] + [("dit", T) for T in range(n)]


def ntt_plan(N, inverse=False):
    """The stand-alone transform: DIF levels over all strides, then the block permutation (natural order in and out)."""
    n = ilog2(N)
    return [("dif", T, inverse) for T in range(n - 1, -1, -1)] + [("bitrev",)]


def run_stage(x, stage, backward=False):
    if stage[0] == "dif":
        return dif_level(x, stage[1], stage[2], backward)
    if stage[0] == "dit":
        return dit_level(x, stage[1], False, backward)
    if stage[0] == "factor":
        return factor_stage(x, len(x), stage[1], backward)
    return bitrev_stage(x)   # its own inverse


def run_forward(column, plan, start=0):
    """The states after stage start, start + 1, ... of `plan`, `column` being the state that enters stage `start`."""
    states, x = [], list(column)
    for stage in plan[start:]:
        x = run_stage(x, stage)
        states.append(x)
    return states


def run_backward(state, plan, stop):
    """The input of the pipeline whose state ENTERING stage `stop` is `state` (stages stop - 1 .. 0 undone)."""
    x = list(state)
    for stage in reversed(plan[:stop]):
        x = run_stage(x, stage, backward=True)
    return x


def coset_generators(N, e):
    """w_2N; w_4N, w_4N^3; w_8N, w_8N^3, w_8N^5, w_8N^7 — the nesting order of include/fastecc.h."""
    gens = []
    for j in range(1, e + 1):
        w = root(N << j)
        gens += [pow(w, c, P) for c in range(1, 1 << j, 2)]
    return gens


def stage_index(N, level, half):
    """Index in encode_plan(N) of the radix-2 level of stride 2^level of the DIF half ('dif') or the DIT half ('dit')."""
    n = ilog2(N)
    assert 0 <= level < n and half in ("dif", "dit")
    return n - 1 - level if half == "dif" else n + 1 + level


# ---- boundary events ----
def boundary_event(a, b):
    """The pair (a, b) an add and a sub see sits where one of their decisions flips."""
    return a + b in EVENT_SUMS or a - b in EVENT_DIFFS or (a == P - 1 and b == P - 1)


def level_pairs(state, stage):
    """The pairs (a, b) the add and the sub of one radix-2 level of an encode plan see, `state` entering it: the two words of a DIF
    butterfly as they are, the first word and the PRODUCT of the second with its twiddle in a DIT butterfly."""
    h = 1 << stage[1]
    tw = level_twiddles(stage[1], False) if stage[0] == "dit" else None
    out = []
    for base in range(0, len(state), 2 * h):
        for m in range(h):
            a, b = state[base + m], state[base + m + h]
            out.append((a, b * tw[m] % P) if tw else (a, b))
    return out


def event_counts(column):
    """(boundary events, butterflies with a non-zero operand) over the levels of the encode's DIF half."""
    N = len(column)
    total = events = 0
    x = list(column)
    for stage in encode_plan(N)[:ilog2(N)]:
        for a, b in level_pairs(x, stage):
            if a or b:
                total += 1
                events += boundary_event(a, b)
        x = run_stage(x, stage)
    return events, total


def event_counts_np(column):
    """event_counts on numpy uint64 words (every product is below 2^64, so it is as exact): for the sizes the loop above is too slow at."""
    import numpy as np
    N = len(column)
    x = np.array(column, dtype=np.uint64)
    total = events = 0
    for T in range(ilog2(N) - 1, -1, -1):
        h = 1 << T
        v = x.reshape(-1, 2, h)
        a, b = v[:, 0, :].copy(), v[:, 1, :].copy()
        s, d = a + b, a.astype(np.int64) - b.astype(np.int64)
        live = (a | b) != 0
        ev = np.isin(s, np.array(EVENT_SUMS, dtype=np.uint64)) | (np.abs(d) <= 1)   # a = b = p - 1 is a difference of 0
        total += int(live.sum())
        events += int((ev & live).sum())
        tw = np.array(level_twiddles(T, True), dtype=np.uint64)
        v[:, 0, :] = s % np.uint64(P)
        v[:, 1, :] = (a + np.uint64(P) - b) % np.uint64(P) * tw % np.uint64(P)
    return events, total


def event_share(column):
    """Share of boundary events among the butterflies of the encode's DIF half that have a non-zero operand (1.0 when there is none: the
    zero column).  Where the condition on the structured columns is measured."""
    events, total = event_counts(column)
    return events / total if total else 1.0


EDGE_A = [0, 1, 2, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 31) - 1, 1 << 31, P - (1 << 20), 0xFFEFFFFF, P - 1, P - 2]


def _boundary_pairs():
    rng = random.Random(32)
    firsts = EDGE_A + [rng.randrange(P) for _ in range(6)]
    pairs = []
    for a in firsts:
        for s in EVENT_SUMS:
            if 0 <= s - a < P:
                pairs.append((a, s - a))
        for d in EVENT_DIFFS:
            if 0 <= a - d < P:
                pairs.append((a, a - d))
    pairs += [(0, 0)] + [(0, x) for x in firsts if x] + [(x, 0) for x in firsts if x]
    seen, out = set(), []
    for pr in pairs:
        if pr not in seen:
            seen.add(pr)
            out.append(pr)
    return out


# canonical (a, b): every sum of EVENT_SUMS and every difference of EVENT_DIFFS that a word of EDGE_A (or one of six seeded random words) can
# reach with a canonical partner, then (0, 0), (0, x) and (x, 0).  All but the (0, x) / (x, 0) with x not 1 or p - 1 are boundary events.
BOUNDARY_PAIRS = _boundary_pairs()
EVENT_PAIRS = [pr for pr in BOUNDARY_PAIRS if boundary_event(*pr)]   # what the targeted columns draw from


# ---- columns ----
def structured_columns(N, seed=0):
    """[(name, column)]: one column of N words per family, N any divisor of p - 1 that is even.  At a power of two all but the impulses at
    odd positions and 'small words' (kept as plain cases) make at least half of the DIF half's butterflies boundary events."""
    assert (P - 1) % N == 0 and N % 2 == 0, N
    rng = random.Random(1000 + seed + N)
    rnd = lambda: rng.randrange(1 << 21, P - (1 << 21))
    small = lambda: rng.choice([rng.randrange(8), P - 1 - rng.randrange(8)])
    cols = [("zero", [0] * N), ("all p-1", [P - 1] * N), ("constant", [rnd()] * N)]
    # 2 * 2^31 = 2^32 exactly (the carry out of 32 bits) = 2^20 - 1 (mod p), so both constants walk through 2^k (2^20 - 1)
    cols += [("constant 2^31", [1 << 31] * N), ("constant 2^20-1", [(1 << 20) - 1] * N)]
    positions = sorted({0, 1, N // 2, N - 1})
    for name, v in (("1", 1), ("p-1", P - 1), ("2^20-1", (1 << 20) - 1)):
        for pos in positions:
            if v == (1 << 20) - 1 and pos % 2 == 0:
                continue   # paired with zeros this word is no boundary event: only its plain cases (odd positions) are kept
            col = [0] * N
            col[pos] = v
            cols.append(("impulse %s at %d" % (name, pos), col))
    others = [f for f in range(3, N - 1, 2) if f != N // 2]     # one more odd frequency, where there is one
    for f in positions + ([rng.choice(others)] if others else []):
        w, cur, col = pow(root(N), f, P), rnd(), []
        for _ in range(N):
            col.append(cur)
            cur = cur * w % P
        cols.append(("tone f=%d" % f, col))
    a = rnd()
    cols.append(("a, -a alternating", [(a, P - a)[j & 1] for j in range(N)]))
    cols.append(("period 2", [(P - 1, 0)[j & 1] for j in range(N)]))
    cols.append(("period 4", [(P - 1, 0, 1, P - 2)[j & 3] for j in range(N)]))
    cols.append(("small words", [small() for _ in range(N)]))
    return cols


PLAIN_CASES = ("small words",)


def is_plain_case(name, N):
    """The families the share condition does not bind: 'small words' and the impulses at odd positions."""
    if name in PLAIN_CASES:
        return True
    return name.startswith("impulse") and int(name.rsplit(" ", 1)[1]) % 2 == 1


def targeted_cost(N, level, half):
    """Butterflies the backward model runs for one targeted column."""
    n = ilog2(N)
    return (N // 2) * (n - 1 - level if half == "dif" else n + level)


def targeted_columns(N, level=None, half=None, seed=0, budget=None):
    """[(half, level, column, target)]: the pairs the add and sub of the level of stride 2^level of that half of the encode see are drawn from
    EVENT_PAIRS (the boundary events of BOUNDARY_PAIRS); `target` is the state ENTERING that level — the pair itself for a DIF level,
    (a, t w^-m) for a DIT level, whose product b w^m is then t — and `column` the canonical input that produces it.  With level and half: that
    one column; else one per level of each half — budget: at most about that many model butterflies in all (the DIF levels first, then the
    DIT levels from stride 1 up)."""
    n = ilog2(N)
    plan = encode_plan(N)
    wanted = [(half, level)] if level is not None else [("dif", T) for T in range(n - 1, -1, -1)] + [("dit", T) for T in range(n)]
    out, spent = [], 0
    for hf, T in wanted:
        cost = targeted_cost(N, T, hf)
        if budget is not None and spent + cost > budget:
            continue
        spent += cost
        rng = random.Random((seed * 64 + T) * 2 + (hf == "dit") + 977 * N)
        h = 1 << T
        itw = level_twiddles(T, True)   # w^-m
        order = list(EVENT_PAIRS)   # dealt out in a shuffled order: from N / 2 >= len(EVENT_PAIRS) on every pair is met in every column
        rng.shuffle(order)
        target, dealt = [0] * N, 0
        for base in range(0, N, 2 * h):
            for m in range(h):
                a, b = order[dealt % len(order)]
                dealt += 1
                target[base + m], target[base + m + h] = a, (b * itw[m] % P if hf == "dit" else b)
        out.append((hf, T, run_backward(target, plan, stage_index(N, T, hf)), target))
    return out


def random_column(N, seed=0):
    rng = random.Random(5000 + seed + N)
    return [rng.randrange(P) for _ in range(N)]


def edge_stripe(N, S=70, seed=0, budget=None):
    """The columns of one stripe of S words per block: the structured columns, then the targeted columns of every level of both halves
    (within `budget`), then random fill.  -> (columns, names); stripe_array(columns) is the stripe."""
    cols = structured_columns(N, seed)
    names = [name for name, _ in cols]
    columns = [col for _, col in cols]
    for hf, T, col, _ in targeted_columns(N, seed=seed, budget=budget):
        names.append("target %s %d" % (hf, T))
        columns.append(col)
    assert len(columns) <= S, (len(columns), S)
    k = 0
    while len(columns) < S:
        names.append("random %d" % k)
        columns.append(random_column(N, seed * 100 + k))
        k += 1
    return columns, names


def stripe_array(columns):
    """columns[c][block]  ->  numpy uint32 [N, S], the library's stripe layout."""
    import numpy as np
    return np.ascontiguousarray(np.array(columns, dtype=np.uint32).T)


def column_of(stripe, c):
    return [int(v) for v in stripe[:, c]]
