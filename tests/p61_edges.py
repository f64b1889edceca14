"""Inputs that put the 64-bit field's LAZY arithmetic at the edges of its ranges, and an exact model to build them with.

The device code over GF((2^61-1)^2) (gf61.hpp, gf61_kernels.hip) keeps words lazy — in [0, 2^61 + 2^33), congruent to the value —
and only the last pass of a transform makes them canonical.  A lazy word is non-canonical only when its value lies in
[0, 2^33) (held as v or v + p) — the zone where canon() has work to do and where an offset of 2p or 4p is needed — and the butterflies of
a transform turn uniformly random inputs into uniformly random intermediates, which meet that zone with probability 2^-27.
The columns built here make the INTERMEDIATE words of a transform small, zero or just below p:

  structured_columns(N)             tones, impulses, constants, periodic patterns: their transforms are sparse (zeros everywhere)
  targeted_columns(N, level, half)  the state ENTERING one radix-2 level is chosen word by word from EDGE_WORDS and the input that
                                    produces it is found by running the model backwards

Everything here is exact arithmetic on Python integers; nothing of the library is used.  Plain helper module (no fixtures, no tests).
"""
import functools
import random

P = (1 << 61) - 1
LAZY_LIMIT = (1 << 61) + (1 << 33)   # lazy words are below this
ZONE = 1 << 33                       # edge zone: [0, ZONE) and [P - ZONE, P)
ZERO = (0, 0)
HALF = 1 << 60                       # 1 / 2 mod p  (2 * 2^60 = 2^61 = 1)

# the state entering a level is drawn from these (re and im independently): targeted_columns
EDGE_WORDS = [0, 1, 2, 1 << 30, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, (1 << 33) - 1, 1 << 33, 1 << 60, P - (1 << 33), P - 2, P - 1]
# operands of the device probe (fastecc_gf61_binary): lazy words, canonical or not
LAZY_EDGE_WORDS = [0, 1, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 33, 1 << 60, P - 1, P, P + 1, (1 << 61) + 7, (1 << 61) + (1 << 32),
                   (1 << 61) + (1 << 33) - 1]
# ... and for the ops that take any 64-bit word
RAW_EDGE_WORDS = [1 << 62, (1 << 63) - 1, 1 << 63, 7 * (1 << 61) + (1 << 34), (1 << 64) - 1]   # 3.5 * 2^62 = 7 * 2^61


# ---- GF(p^2), elements are tuples (re, im), i^2 = -1 ----
def addc(x, y):
    return ((x[0] + y[0]) % P, (x[1] + y[1]) % P)


def subc(x, y):
    return ((x[0] - y[0]) % P, (x[1] - y[1]) % P)


def mulc(x, y):
    return ((x[0] * y[0] - x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


def scalec(x, s):
    return (x[0] * s % P, x[1] * s % P)


def conj(x):
    return (x[0], -x[1] % P)


def powc(x, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = mulc(r, x)
        x = mulc(x, x)
        e >>= 1
    return r


def invc(x):
    return scalec(conj(x), pow((x[0] * x[0] + x[1] * x[1]) % P, P - 2, P))


@functools.lru_cache(maxsize=None)
def root(order):
    """The root of unity of order `order` (a power of two <= 2^62) of include/fastecc.h: w_(2^62) = (4 + i)^(2^60 - 1)."""
    assert order >= 1 and order & (order - 1) == 0 and order <= 1 << 62
    return powc(powc((4, 1), (1 << 60) - 1), (1 << 62) // order)


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
        w = conj(w)   # |w| = 1: the inverse of a root of unity is its conjugate (w * conj(w) = norm = 1)
    out, cur = [], (1, 0)
    for _ in range(1 << T):
        out.append(cur)
        cur = mulc(cur, w)
    return out


# ---- radix-2 levels on one column (a list of N elements), forwards and backwards ----
def dif_level(x, T, inverse, backward=False):
    """Decimation in frequency, stride 2^T: (a, b) -> (a + b, (a - b) w^m).  backward: the level undone."""
    h = 1 << T
    tw = level_twiddles(T, not inverse if backward else inverse)
    y = list(x)
    for base in range(0, len(x), 2 * h):
        for m in range(h):
            a, b = x[base + m], x[base + m + h]
            if a == ZERO and b == ZERO:
                continue
            if backward:
                t = mulc(b, tw[m])
                y[base + m], y[base + m + h] = scalec(addc(a, t), HALF), scalec(subc(a, t), HALF)
            else:
                y[base + m], y[base + m + h] = addc(a, b), mulc(subc(a, b), tw[m])
    return y


def dit_level(x, T, inverse=False, backward=False):
    """Decimation in time, stride 2^T: (a, b) -> (a + b w^m, a - b w^m).  backward: the level undone."""
    h = 1 << T
    tw = level_twiddles(T, not inverse if backward else inverse)
    y = list(x)
    for base in range(0, len(x), 2 * h):
        for m in range(h):
            a, b = x[base + m], x[base + m + h]
            if a == ZERO and b == ZERO:
                continue
            if backward:
                y[base + m], y[base + m + h] = scalec(addc(a, b), HALF), mulc(scalec(subc(a, b), HALF), tw[m])
            else:
                t = mulc(b, tw[m])
                y[base + m], y[base + m + h] = addc(a, t), subc(a, t)
    return y


@functools.lru_cache(maxsize=None)
def block_factors(N, gen):
    """Position q holds coefficient c = bitrev(q) after the DIF half; its factor is gen^c / N (the encoder: gen = w_2N)."""
    n = ilog2(N)
    inv_n = pow(N, P - 2, P)
    powers, cur = [], (inv_n, 0)
    for _ in range(N):
        powers.append(cur)
        cur = mulc(cur, gen)
    return [powers[bitrev(q, n)] for q in range(N)]


def factor_stage(x, N, gen, backward=False):
    f = block_factors(N, gen)
    if backward:
        return [mulc(v, invc(w)) if v != ZERO else v for v, w in zip(x, f)]
    return [mulc(v, w) if v != ZERO else v for v, w in zip(x, f)]


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
        gens += [powc(w, c) for c in range(1, 1 << j, 2)]
    return gens


def stage_index(N, level, half):
    """Index in encode_plan(N) of the radix-2 level of stride 2^level of the DIF half ('dif') or the DIT half ('dit')."""
    n = ilog2(N)
    assert 0 <= level < n and half in ("dif", "dit")
    return n - 1 - level if half == "dif" else n + 1 + level


# ---- columns ----
def edge_share(states):
    """Share of the words (re and im of every element of every state) that lie in [0, 2^33) or [p - 2^33, p)."""
    total = edge = 0
    for st in states:
        for v in st:
            for w in v:
                total += 1
                edge += w < ZONE or w >= P - ZONE
    return edge / total if total else 0.0


def dif_half_states(column):
    """The states after each level of the encode's DIF half: where the condition on edge_share is measured."""
    N = len(column)
    return run_forward(column, encode_plan(N)[:ilog2(N)])


def structured_columns(N, seed=0):
    """[(name, column)]: one column of N elements per family.  The transforms of all but 'constant' (kept as the plain case) and 'small
    words' are sparse — at least half of the words the DIF half computes are in the edge zone."""
    rng = random.Random(1000 + seed + N)
    rnd = lambda: rng.randrange(1 << 33, P - (1 << 33))
    small = lambda: rng.choice([rng.randrange(8), P - 1 - rng.randrange(8)])
    ilog2(N)
    cols = [("zero", [ZERO] * N), ("all p-1", [(P - 1, P - 1)] * N)]
    c = (rnd(), rnd())
    cols += [("constant", [c] * N), ("re only", [(c[0], 0)] * N), ("im only", [(0, c[1])] * N)]
    for name, v in (("1", (1, 0)), ("p-1", (P - 1, 0)), ("i", (0, 1))):
        for pos in sorted({0, 1, N // 2, N - 1}):
            col = [ZERO] * N
            col[pos] = v
            cols.append(("impulse %s at %d" % (name, pos), col))
    fixed = sorted({0, 1, N // 2, N - 1})
    others = [f for f in range(3, N - 1, 2)]                      # one more odd frequency, where there is one
    for f in fixed + ([rng.choice(others)] if others else []):
        w, cur, col = powc(root(N), f), (rnd(), rnd()), []
        for _ in range(N):
            col.append(cur)
            cur = mulc(cur, w)
        cols.append(("tone f=%d" % f, col))
    cols.append(("period 2", [((P - 1, P - 1), ZERO)[j & 1] for j in range(N)]))
    cols.append(("period 4", [((P - 1, 0), ZERO, (0, P - 1), (P - 1, P - 1))[j & 3] for j in range(N)]))
    cols.append(("small words", [(small(), small()) for _ in range(N)]))
    return cols


def targeted_cost(N, level, half):
    """Butterflies the backward model runs for one targeted column."""
    n = ilog2(N)
    return (N // 2) * (n - 1 - level if half == "dif" else n + level)


def targeted_columns(N, level=None, half=None, seed=0, budget=None):
    """[(half, level, column, target)]: `target`, the state ENTERING the level of stride 2^level of that half of the encode, is drawn word by
    word from EDGE_WORDS; `column` is the canonical input that produces it.  With level and half: that one column; else one per level of each
    half — budget: at most about that many model butterflies in all (the DIF levels first, then the DIT levels from stride 1 up)."""
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
        target = [(rng.choice(EDGE_WORDS), rng.choice(EDGE_WORDS)) for _ in range(N)]
        out.append((hf, T, run_backward(target, plan, stage_index(N, T, hf)), target))
    return out


def random_column(N, seed=0):
    rng = random.Random(5000 + seed + N)
    return [(rng.randrange(P), rng.randrange(P)) for _ in range(N)]


def edge_stripe(N, elems=70, seed=0, budget=None):
    """The columns of one stripe of `elems` elements per block: the structured columns, then the targeted columns of every level of both
    halves (within `budget`), then random fill.  -> (columns, names); stripe_array(columns) is the stripe."""
    cols = structured_columns(N, seed)
    names = [name for name, _ in cols]
    columns = [col for _, col in cols]
    for hf, T, col, _ in targeted_columns(N, seed=seed, budget=budget):
        names.append("target %s %d" % (hf, T))
        columns.append(col)
    assert len(columns) <= elems, (len(columns), elems)
    k = 0
    while len(columns) < elems:
        names.append("random %d" % k)
        columns.append(random_column(N, seed * 100 + k))
        k += 1
    return columns, names


def stripe_array(columns):
    """columns[c][block] = (re, im)  ->  numpy uint64 [N, 2 * elems], the library's stripe layout."""
    import numpy as np
    N, elems = len(columns[0]), len(columns)
    a = np.empty((N, 2 * elems), dtype=np.uint64)
    for c, col in enumerate(columns):
        a[:, 2 * c] = np.array([v[0] for v in col], dtype=np.uint64)
        a[:, 2 * c + 1] = np.array([v[1] for v in col], dtype=np.uint64)
    return a


def column_of(stripe, c):
    return [(int(r), int(i)) for r, i in zip(stripe[:, 2 * c], stripe[:, 2 * c + 1])]


# ---- the device probe (fastecc_gf61_binary, include/fastecc.h): exact results and the stated output bounds ----
FOLDED = (1 << 61) + 8
PROBE_BOUNDS = {
    "add": (1 << 61) + 2,        # lazy + lazy < 2^62 + 2^34: the fold adds at most 2 to a 61-bit word  (any inputs: FOLDED)
    "sub": (1 << 61) + 3,        # lazy + 2p - lazy < 3 * 2^61 + 2^33: at most 3
    "mul": FOLDED,
    "mul_raw": FOLDED,
    "mul_w8": (1 << 61) + (1 << 32),
    "mul_w8i": (1 << 61) + (1 << 32),
    "mul_w8_inv": (1 << 61) + (1 << 32),
    "mul_w8i_inv": (1 << 61) + (1 << 32),
    "fold": FOLDED,
    "canon": P,
    "run_dif": FOLDED,
    "run_dif_inv": FOLDED,
    "run_dit": FOLDED,
}
ELEMENT_OPS = ["add", "sub", "mul", "mul_raw", "mul_w8", "mul_w8i", "mul_w8_inv", "mul_w8i_inv", "fold", "canon"]
BINARY_OPS = ("add", "sub", "mul", "mul_raw")
RAW_INPUT_OPS = ("mul_raw", "fold")    # x: any 64-bit word
RUN_OPS = ("run_dif", "run_dif_inv", "run_dit")


def probe_expected(op, x, y=None):
    """The residue (canonical element) the probe's `op` must return for x (and y): operands are any integers, reduced here."""
    x = (x[0] % P, x[1] % P)
    if op in BINARY_OPS:
        y = (y[0] % P, y[1] % P)
    if op == "add":
        return addc(x, y)
    if op == "sub":
        return subc(x, y)
    if op in ("mul", "mul_raw"):
        return mulc(x, y)
    w8 = root(8)
    if op == "mul_w8":
        return mulc(x, w8)
    if op == "mul_w8i":
        return mulc(x, powc(w8, 3))
    if op == "mul_w8_inv":
        return mulc(x, conj(w8))
    if op == "mul_w8i_inv":
        return mulc(x, conj(powc(w8, 3)))
    assert op in ("fold", "canon"), op
    return x


def run_expected(op, xs):
    """A run op on 2^L elements (any integers): all L levels of a 2^L-point transform, no twiddle outside the run."""
    L = ilog2(len(xs))
    x = [(v[0] % P, v[1] % P) for v in xs]
    if op == "run_dit":
        for T in range(L):
            x = dit_level(x, T)
    else:
        for T in range(L - 1, -1, -1):
            x = dif_level(x, T, op == "run_dif_inv")
    return x
