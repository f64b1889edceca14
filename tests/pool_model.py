"""A CPU model of a small pool of stripes, a seeded generator of pool-operation sequences and the driver that applies one sequence to the
model and to a backend, comparing after every step (tests/test_pool_model_host.py on the numpy backend, tests/test_gpu_pool_sequences.py on
the library).  Exact integer arithmetic and numpy only; nothing here calls the library: the parity comes from the oracle (oracle/), the GPU
backend is handed the package by its test module.

The model (PoolModel) holds
  truth   the codewords: the data last written and the oracle's parity of it (Codec.parity: the one place the tests' code forms live);
  mirror  what the device pool must hold now: truth except for blocks the model corrupted or marked absent (garbage);
  per stripe the silently corrupted blocks ("small": all words < p, "big": a word >= p) and the absent blocks;
  the devices that are down or replaced (their blocks are named absent until every one is rebuilt);
  the context state include/fastecc.h defines: the prepared pattern (a value, None or UNSPECIFIED), the prepared pattern set, the scrub pattern,
  the scrub pattern set, the options, the stream.

Placement: "fixed" keeps block j of every stripe on device j (one pattern, the single-pattern calls); "rotated" keeps block j of stripe b on
device (j + b) mod n (stripe b uses pattern b mod n of a set, the _set calls).  A rotated pool has QUARANTINED stripes: garbage that every
_set call names FASTECC_PATTERN_NONE and no write targets; they are compared like every other stripe after every step.

Budget: with t small-corrupted blocks, b big ones and w blocks named absent, every stripe keeps 2t + b + w <= n - k and t <= locate_max at
all times (include/fastecc.h:438-444, 470-471), so every answer is unique.

State probes (each a short scripted run of operations that ends in a check on a scratch stripe; the header lines are include/fastecc.h's):
  prepared_after_prepare_set        decode_prepare's pattern survives fastecc_decode_prepare_set            (385-387)
  prepared_after_scrub_pattern      ... fastecc_scrub_erasures                                              (458-460)
  prepared_after_scrub_pattern_set  ... fastecc_scrub_erasures_set                                          (548-550)
  prepared_after_write              ... fastecc_update_batch (the update state is its own: 631)             (631-639)
  prepared_after_verify             ... fastecc_verify_batch / _verify_batch_set ("Reads only")             (489-490, 554)
  prepared_after_locate             ... fastecc_locate_errors_batch ("Reads only")                          (504-509)
  set_after_prepare                 the pattern set survives fastecc_decode_prepare                         (385-387)
  set_after_single                  ... fastecc_decode / fastecc_repair                                     (385-387)
  set_after_batch                   ... fastecc_decode_batch / fastecc_repair_batch                         (385-387)
  set_after_correct                 ... fastecc_correct_batch / _correct_batch_set                          (386, 563-564)
  scrub_after_prepare               the scrub pattern survives fastecc_decode_prepare                       (458-460)
  scrub_after_single                ... fastecc_decode / fastecc_repair                                     (458-460)
  scrub_after_correct               ... fastecc_correct_batch / _correct_batch_set                          (458-460, 472-476)
  unspecified_after_correct         fastecc_correct* REPLACES the prepared pattern (436, 491-492, 563): the model makes it UNSPECIFIED and
                                    raises ModelError if an operation uses it before a new decode_prepare (checked on the host)
  refused_bad_write                 an index >= count*k in writes: FASTECC_E_INVAL, nothing written         (627-630)
  refused_bad_pattern               pattern_of[b] == n_patterns: FASTECC_E_INVAL, nothing written           (413-416)
  refused_count0                    count == 0: FASTECC_E_INVAL                                             (375-377)
Extended sequences (EXT_SEEDS) run these instead, and prepared_after_locate on rotated pools too (fastecc_locate_errors_batch_set, 643-647):
  prepared_after_read               decode_prepare's pattern survives fastecc_read_batch / _read_batch_set  (477-478)
  set_after_read                    the pattern set survives ...                                            (477-478)
  scrub_after_read                  the scrub pattern survives ...                                          (477-478)
  read_after_prepare                decode_prepare(A), read, decode_prepare(B), read on a scratch stripe: the second read rebuilds B's lost
                                    blocks and copies A's (459-468).  B loses as many data blocks as A and differs in one; variant "transform":
                                    A is prepared under decode_direct_max = 0 and its read is refused FASTECC_E_UNSUPPORTED with nothing
                                    written (459-461, 484), B is direct; variant "parity": B loses parity only, every request a copy (461)
  read_after_prepare_set            decode_prepare_set, a read on the side stream, a second decode_prepare_set with other patterns and nothing
                                    synchronised in between (it waits for the read itself: 476-477), a read: it follows the new set (456-458)
  refused_bad_read                  a read index >= count*k; pattern_of[b] == n_patterns for a requested stripe: FASTECC_E_INVAL, the output
                                    all canary, the context unchanged                                        (480-483)

Degraded sequences (DEG_SEEDS) run these instead (the lines are those of "Degraded writes" and "Sub-block writes" in include/fastecc.h):
  prepared_after_degraded_write     decode_prepare's pattern survives fastecc_update_batch_set / _update_parity_batch_set, whole-block or window,
                                    into a scratch stripe under a set of its own                                (765-766)
  set_after_degraded_write          the pattern set survives ...                                                (765-766)
  scrub_after_degraded_write        the scrub pattern survives ...                                              (765-766)
  write_after_prepare_set           decode_prepare_set(A), a degraded write on the side stream, decode_prepare_set(B) with nothing synchronised
                                    in between (it waits for the write itself: 766), a degraded write: the first result is A's, the second B's
  read_after_degraded_write         a degraded write of absent blocks on one stream, fastecc_read_batch_set of them on the other, ordered by an
                                    event only: the read returns the new rows                                   (759-760)
  repair_after_degraded_write       a degraded window write, then fastecc_repair_batch_set under the same pattern: every block of the scratch
                                    stripe is the oracle's encode of X'                                         (758-760, 792-795)
  untouched_pattern_ignored         pattern_of[b] == n_patterns for a stripe that no write names: the call succeeds (752-753, 764)
  refused_bad_degraded_write        one variant per draw: such an entry for a TOUCHED stripe, a null pattern_of (767-769); width 0, col0 + width =
                                    S + 1, col0 = 2^64 - 1 with width 2 (the sum overflows), rows that overlap the pool (802-804):
                                    FASTECC_E_INVAL, the pool, the caller's rows and the context unchanged.  The operation is a write the model
                                    allows (the pool's own set in force, legal stripes, a window inside the block) with that one argument
                                    spoiled, so nothing else can be the reason; the first two and the last through both kinds of entry point
  refused_no_set                    a _set write before any fastecc_decode_prepare_set: FASTECC_E_INVAL (768); step 0 of the seed DEG_SEEDS[0]
(An option cannot be read back from a context: that no option changes shows only in the calls that follow.)

Writes: the forms "batch", "parity", "single" (fastecc_update_batch, _update_parity_batch, fastecc_update), "pool" (extended: whole stripes and
fastecc_encode_pool) and, in degraded sequences, "batch_set" and "parity_set" (fastecc_update_batch_set, _update_parity_batch_set) and an optional
window {"col0", "width", "shape"} on the four pool forms (the fastecc_update_*_window calls; rows compact at pitch width).  One rule, the header's:
no touched stripe is quarantined; inside the window's columns every PRESENT block of a touched stripe equals the truth (so a window may lie beside
a single wrong word, and the corruption mark stays: 796-797); absent blocks only under a _set form.  The truth takes the rows in the window and the
oracle's whole re-encode; the mirror's present blocks take the truth in the window's columns; its other columns and every absent block stay as
they are.  The parity forms store no data: the backend, as the caller, stores the window into the present data blocks itself, and hands
"parity_set" the truth as the old row of an absent block.  Both placements use the set needed_set() with pattern_of[b] = b mod n.

Reads ("read", extended sequences): fastecc_read_batch on fixed placement, fastecc_read_batch_set on rotated, over the whole pool: a present
block gives the mirror's words (a corrupted block reads back corrupted, a quarantined stripe's garbage is copied), a block lost under its
stripe's pattern gives the truth; lost blocks are requested only in stripes without a corrupted survivor (which survivors a pass reads is
left open by the header).  The backend presets n_reads + 1 output rows to CANARY and returns the rows and the extra row ("guard").

Bursts: a "burst" operation enqueues 2 to 4 calls (writes of every form, at most one rebuild; in extended sequences reads too, their output
read back only after the burst) back to back on the null and the side stream
with nothing read in between, so a call meets the previous call's staged list and buffers still in flight; its prediction is the calls
applied in order.  In degraded sequences a burst's middle is read, write, write, read on alternating streams where absent data blocks can be
written: both writes rebuild old rows (through the staged list the reads use), one a window call and one a whole-block call.

Determinism: the generator reads the model only, never a backend's answer, so (config, seed) fixes the sequence.  Every operation is one JSON
line (its arrays come from the "dseed" it names); run_sequence(backend, config, seed, steps=N) replays a prefix.
"""
import collections
import json
import zlib

import numpy as np

P = 0xFFF00001
PATTERN_NONE = 0xFFFFFFFF
OK, E_INVAL, E_UNSUPPORTED = 0, -1, -4
UNSPECIFIED = "UNSPECIFIED"
MIXED_RADIX = 1  # FASTECC_CODE_MIXED_RADIX
CANARY = 0xFFFA5A5A  # what the output rows of a read hold before the call (>= p: no word of the truth)


# ---- the code forms (shared with test_gpu_fuzz.py and test_gpu_cosets.py) ----
def expected_pow2(oracle, x, m):
    """fastecc_create's code for any (k, m <= N): the (N + M, N) sub-code of the zero-extended stripe (RS.md:23-33)."""
    k, S = x.shape
    lg = max(1, int(np.ceil(np.log2(k))))
    N = 1 << lg
    lgm = int(np.ceil(np.log2(m))) if m > 1 else 0
    fold = min(lg - lgm, 4)
    padded = np.zeros((N, S), dtype=np.uint32)
    padded[:k] = x
    return oracle.encode_fast(padded)[:: 1 << fold][:m]


def coset_generators(oracle, N, e):
    """w_2N; w_4N, w_4N^3; w_8N, w_8N^3, w_8N^5, w_8N^7 — the nesting order of include/fastecc.h."""
    gens = []
    for j in range(1, e + 1):
        w = oracle.gf_root(N << j)
        gens += [oracle.gf_pow(w, c) for c in range(1, 1 << j, 2)]
    return gens


def oracle_parity(oracle, x, e):
    """n = k << e: the parity one coset at a time (iNTT, block i *= g^i / N, NTT)."""
    N = x.shape[0]
    coef = oracle.ntt_fast(x, inverse=True)
    inv_n = oracle.gf_inv(N)
    return np.concatenate([oracle.ntt_fast(oracle.scale_blocks(coef, inv_n, g)) for g in coset_generators(oracle, N, e)])


class Codec:
    """The oracle's parity of one stripe for every kind of code the pool tests use."""

    def __init__(self, oracle, n, k, flags=0, order=0):
        self.oracle, self.n, self.k, self.m, self.flags, self.order = oracle, n, k, n - k, flags, order

    def parity(self, x):
        x = np.ascontiguousarray(x, dtype=np.uint32)
        n, k = self.n, self.k
        if self.flags & MIXED_RADIX and self.order & (self.order - 1):
            return self.oracle.encode_mixed_code(x, n, self.order)
        if not k & (k - 1) and n in (4 * k, 8 * k):
            return oracle_parity(self.oracle, x, 2 if n == 4 * k else 3)
        return expected_pow2(self.oracle, x, n - k)


Config = collections.namedtuple("Config", "name n k S count flags order placement steps")


def _configs():
    rows = [("20_16_s64", 20, 16, 64, 67, 0, 0), ("20_16_s100", 20, 16, 100, 67, 0, 0), ("64_32", 64, 32, 16, 33, 0, 0),
            ("48_32", 48, 32, 64, 40, 0, 0), ("32_8", 32, 8, 32, 24, 0, 0), ("100_70", 100, 70, 20, 11, 0, 0),
            ("256_128", 256, 128, 1024, 9, 0, 0), ("72_48_mixed", 72, 48, 64, 16, MIXED_RADIX, 48)]
    return [Config(name + "_" + pl, n, k, S, count, flags, order, pl, 40) for name, n, k, S, count, flags, order in rows
            for pl in ("fixed", "rotated")]


CONFIGS = _configs()
SEEDS = (1, 2, 3, 4)
EXT_SEEDS = (5, 6)  # the extended sequences: reads, set location, whole-stripe writes (Generator(extended=True))
DEG_SEEDS = (7, 8)  # the degraded sequences: degraded writes and column-window writes as well (Generator(degraded=True))
SET_FORMS = ("batch_set", "parity_set")  # fastecc_update_batch_set, fastecc_update_parity_batch_set: stripes may miss blocks
WINDOW_FORMS = ("batch", "parity") + SET_FORMS  # the four pool forms that take a column window ("single" and "pool" keep none)


def config_named(name):
    return next(c for c in CONFIGS if c.name == name)


def writes_of(op, k):
    """the pool block indices a write names: its list, or every data block of the stripes [b0, b1) of a whole-stripe write"""
    return list(range(op["b0"] * k, op["b1"] * k)) if op["form"] == "pool" else op["writes"]


def window(row, op):
    return row[op["col0"]:op["col0"] + op["width"]]


def canary_rows(n, width):
    return np.full((n, width), CANARY, dtype=np.uint32)


class ModelError(Exception):
    """The generator produced an operation the model's state does not allow (a bug of the generator, never of a backend)."""


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _below_p(rng, shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64).astype(np.uint32)


def _garbage(rng, S, big):
    row = rng.integers(0, 1 << 32, size=S, dtype=np.uint64).astype(np.uint32)
    if big:
        row[int(rng.integers(S))] = np.uint32(P + int(rng.integers(0, (1 << 32) - P)))
    return row


class Ctx:
    """The context state include/fastecc.h defines."""

    def __init__(self):
        self.prepared = None      # None, a sorted tuple of lost blocks, or UNSPECIFIED
        self.prepared_set = None  # None or a tuple of such tuples
        self.scrub = ()           # the absent blocks fastecc_scrub_erasures named
        self.scrub_set = None
        self.prepared_limit = 256  # "decode_direct_max" when the pattern was prepared: it chose the pattern's path
        self.options = {"scrub_batch_chunk": 0, "direct_kernel": 0, "decode_direct_max": 256, "locate_max": 256, "encode_pool_kernel": 0}
        self.stream = 0

    def snapshot(self):
        return (self.prepared, self.prepared_limit, self.prepared_set, self.scrub, self.scrub_set, tuple(sorted(self.options.items())), self.stream)


class PoolModel:
    def __init__(self, cfg, seed, oracle):
        self.cfg, self.seed = cfg, seed
        self.n, self.k, self.m, self.S, self.count = cfg.n, cfg.k, cfg.n - cfg.k, cfg.S, cfg.count
        self.mixed = bool(cfg.flags & MIXED_RADIX)
        self.rotated = cfg.placement == "rotated"
        self.codec = Codec(oracle, cfg.n, cfg.k, cfg.flags, cfg.order)
        rng = _rng("pool", cfg.name, seed)
        self.truth_d = _below_p(rng, (self.count, self.k, self.S))
        self.truth_d[0, 0, :4] = [0, 1, P - 1, 0x000FFFFF][: min(4, self.S)]
        self.truth_p = np.stack([self.codec.parity(self.truth_d[b]) for b in range(self.count)])
        self.quarantined = set()
        if self.rotated:
            self.quarantined = {int(b) for b in rng.choice(self.count, size=2, replace=False)}
            for b in self.quarantined:
                for j in range(self.n):
                    self.block(self.truth_d, self.truth_p, b, j)[:] = _garbage(rng, self.S, j % 3 == 0)
        self.mirror_d, self.mirror_p = self.truth_d.copy(), self.truth_p.copy()
        self.corrupt = [dict() for _ in range(self.count)]
        self.absent = [set() for _ in range(self.count)]
        self.devs = {}  # device -> "down" | "replaced"
        self.ctx = Ctx()
        self.npat = min(self.n, self.count)

    # -- geometry
    def block(self, d, p, b, j):
        return d[b, j] if j < self.k else p[b, j - self.k]

    def dev_of(self, b, j):
        return (j + b) % self.n if self.rotated else j

    def blocks_on(self, b, devs):
        return tuple(sorted((d - b) % self.n if self.rotated else d for d in devs))

    def needed_single(self):
        return self.blocks_on(0, self.devs)

    def needed_set(self):
        return tuple(self.blocks_on(q, self.devs) for q in range(self.npat))

    def live(self):
        return [b for b in range(self.count) if b not in self.quarantined]

    def whole(self, b):
        return b not in self.quarantined and not self.corrupt[b] and not self.absent[b]

    def budget(self, b, extra_t=0, extra_b=0, extra_w=0):
        """(2t + b + w <= n - k and t <= locate_max) for stripe b after the named additions"""
        t = sum(1 for v in self.corrupt[b].values() if v == "small") + extra_t
        big = sum(1 for v in self.corrupt[b].values() if v == "big") + extra_b
        return 2 * t + big + len(self.devs) + extra_w <= self.m and t <= self.ctx.options["locate_max"]

    def pattern_of(self, b0, b1, treat):
        return [b % self.n if treat(b) else PATTERN_NONE for b in range(b0, b1)]

    def _settle(self):
        """a replaced device whose blocks are all back is up again"""
        for dev in [d for d, s in self.devs.items() if s == "replaced"]:
            if not any(j in self.absent[b] for b in self.live() for j in self.blocks_on(b, [dev])):
                del self.devs[dev]

    def _scrub_ready(self, use_set):
        if self.mixed:
            return
        if use_set:
            if self.ctx.scrub_set != self.needed_set():
                raise ModelError("the scrub pattern set is stale")
        elif self.ctx.scrub != self.needed_single():
            raise ModelError("the scrub pattern is stale")

    def _prepared(self):
        if self.ctx.prepared is None or self.ctx.prepared == UNSPECIFIED:
            raise ModelError("the single prepared pattern is %s: decode_prepare first" % (self.ctx.prepared,))
        return self.ctx.prepared

    def _set_pattern(self, q):
        if self.ctx.prepared_set is None:
            raise ModelError("no pattern set")
        return self.ctx.prepared_set[q]

    def _served(self):
        """fastecc_read_batch serves the single prepared pattern: one of the direct path (at most "decode_direct_max" lost blocks when it was
        prepared), or one that lost nothing"""
        return len(self._prepared()) <= self.ctx.prepared_limit

    def _scratch_stripe(self, rng, b, lost):
        """stripe b's truth with the blocks of `lost` overwritten with garbage"""
        d, p = self.truth_d[b].copy(), self.truth_p[b].copy()
        for j in lost:
            (d[j] if j < self.k else p[j - self.k])[:] = _garbage(rng, self.S, j % 2 == 0)
        return d, p

    # -- the arrays an operation carries (a function of the model and the operation's dseed)
    def payload(self, op):
        kind, rng = op["op"], _rng("data", self.cfg.name, self.seed, op.get("dseed", 0))
        pay = {}
        if kind == "corrupt":
            pokes = []
            for j in op["blocks"]:
                row = self.block(self.mirror_d, self.mirror_p, op["b"], j).copy()
                w = int(rng.integers(self.S))
                if op["how"] == "big":
                    row[w] = np.uint32(P + int(rng.integers(0, (1 << 32) - P)))
                elif op["how"] == "word":
                    row[w] = np.uint32((int(row[w]) + 1 + int(rng.integers(P - 1))) % P)
                else:
                    row = _below_p(rng, self.S)
                    row[w] = np.uint32((int(self.block(self.mirror_d, self.mirror_p, op["b"], j)[w]) + 1) % P)
                pokes.append((op["b"], j, row))
            pay["pokes"] = pokes
        elif kind == "device_down":
            pay["pokes"] = [(b, j, _garbage(rng, self.S, b % 2 == 0)) for b in self.live() for j in self.blocks_on(b, [op["dev"]])]
        elif kind == "write":
            writes = writes_of(op, self.k)
            col0, width = op.get("col0", 0), op.get("width", self.S)  # a window: rows of `width` words
            new = _below_p(rng, (len(writes), width))
            new.reshape(-1)[:3] = [P - 1, 0, 1][: min(3, new.size)]
            pay["new"] = new
            if op["form"] != "pool":  # the old rows: the caller's own copy (the truth) where the block is absent, what the pool holds elsewhere
                pay["old"] = np.stack([(self.truth_d if w % self.k in self.lost_for_write(w // self.k, op["form"]) else self.mirror_d)
                                       [w // self.k, w % self.k, col0:col0 + width] for w in writes])
        elif kind == "probe_write":
            lost = self._set_pattern(op["q"])
            pay["scratch_d"], pay["scratch_p"] = self._scratch_stripe(rng, op["b"], lost)
            pay["src"] = op["b"]
            pay["new"] = _below_p(rng, (len(op["writes"]), op["width"]))
            pay["old"] = np.stack([window(self.truth_d[op["b"], i], op) for i in op["writes"]])
        elif kind == "probe_write_swap":
            pay["src"], pay["scratch"], pay["new"], pay["old"] = op["b"], [], [], []
            for half in op["halves"]:
                pay["scratch"].append(self._scratch_stripe(rng, op["b"], half["patterns"][half["q"]]))
                pay["new"].append(_below_p(rng, (len(half["writes"]), half["width"])))
                pay["old"].append(np.stack([window(self.truth_d[op["b"], i], half) for i in half["writes"]]))
        elif kind == "refused" and op["which"] in ("bad_degraded_write", "no_set"):
            pay["new"] = _below_p(rng, (len(op["writes"]), self.S))  # (rows of S words: what the whole-block entry point takes)
        elif kind == "probe_read":
            lost = self._prepared() if not op["set"] else self._set_pattern(op["q"])
            pay["scratch_d"], pay["scratch_p"] = self._scratch_stripe(rng, op["b"], lost)
            pay["src"] = op["b"]
        elif kind == "probe_read_swap":
            pay["src"], pay["scratch"] = op["b"], [self._scratch_stripe(rng, op["b"], half["patterns"][half["q"]]) for half in op["halves"]]
        elif kind in ("probe_repair", "probe_repair_set"):
            lost = self._prepared() if kind == "probe_repair" else self.ctx.prepared_set[op["q"]]
            d, p = self.truth_d[op["b"]].copy(), self.truth_p[op["b"]].copy()
            for j in lost:
                (d[j] if j < self.k else p[j - self.k])[:] = _garbage(rng, self.S, j % 2 == 0)
            pay["scratch_d"], pay["scratch_p"], pay["src"] = d, p, op["b"]
        elif kind == "probe_verify":
            d, p = self.truth_d[op["b"]].copy(), self.truth_p[op["b"]].copy()
            for j in self.ctx.scrub:
                (d[j] if j < self.k else p[j - self.k])[:] = _garbage(rng, self.S, True)
            d2, p2 = d.copy(), p.copy()
            row = d2[op["j"]] if op["j"] < self.k else p2[op["j"] - self.k]
            row[int(rng.integers(self.S))] ^= np.uint32(1 + int(rng.integers(0xFFFF)))
            pay["scratch"], pay["src"] = [(d, p), (d2, p2)], op["b"]
        return pay

    # -- one operation: the new state and the exact prediction of every host output
    def apply(self, op, pay):
        out = getattr(self, "_" + op["op"])(op, pay)
        return {"code": OK} if out is None else out

    def _poke(self, pay):
        for b, j, row in pay["pokes"]:
            self.block(self.mirror_d, self.mirror_p, b, j)[:] = row

    def _corrupt(self, op, pay):
        b = op["b"]
        small = op["how"] != "big"
        if b in self.quarantined or self.mixed:
            raise ModelError("no corruption there")
        for j in op["blocks"]:
            if self.dev_of(b, j) in self.devs or j in self.corrupt[b]:
                raise ModelError("block %d of stripe %d cannot be corrupted" % (j, b))
        if not self.budget(b, extra_t=len(op["blocks"]) if small else 0, extra_b=0 if small else len(op["blocks"])):
            raise ModelError("beyond the correction guarantee")
        for j in op["blocks"]:
            self.corrupt[b][j] = "small" if small else "big"
        self._poke(pay)
        return {}

    def _device_down(self, op, pay):
        dev = op["dev"]
        if dev in self.devs or len(self.devs) >= min(self.m, 2) or not all(self.budget(b, extra_w=1) for b in self.live()):
            raise ModelError("device %d cannot go down" % dev)
        self.devs[dev] = "down"
        for b in self.live():
            for j in self.blocks_on(b, [dev]):
                self.corrupt[b].pop(j, None)
                self.absent[b].add(j)
        self._poke(pay)
        return {}

    def _device_replaced(self, op, pay):
        if self.devs.get(op["dev"]) != "down":
            raise ModelError("device %d is not down" % op["dev"])
        self.devs[op["dev"]] = "replaced"
        self._settle()
        return {}

    def _write(self, op, pay):
        writes = writes_of(op, self.k)
        if len(set(writes)) != len(writes):
            raise ModelError("duplicate write")
        touched = sorted({w // self.k for w in writes})
        if op["form"] in SET_FORMS or "width" in op:
            return self._write_degraded(op, pay, writes, touched)
        if op["form"] == "pool":  # every data block is new and every parity block is encoded: what was corrupted is gone
            if not touched or any(b in self.quarantined or self.absent[b] for b in touched):
                raise ModelError("a whole-stripe write into a stripe that is quarantined or has an absent block")
            for b in touched:
                self.corrupt[b].clear()
        if not all(self.whole(b) for b in touched):
            raise ModelError("a write into a stripe that is not whole")
        for u, w in enumerate(writes):
            self.truth_d[w // self.k, w % self.k] = pay["new"][u]
        for b in touched:
            self.truth_p[b] = self.codec.parity(self.truth_d[b])
            self.mirror_d[b], self.mirror_p[b] = self.truth_d[b], self.truth_p[b]

    def lost_for_write(self, b, form):
        """the blocks of stripe b that a write of this form takes as absent: those its pattern loses (_set forms), none (plain forms)"""
        return self.blocks_on(b, self.devs) if form in SET_FORMS and b not in self.quarantined else ()

    def wrong_columns(self, b):
        """the word columns in which a PRESENT block of stripe b differs from the truth (blocks on a device that is down or replaced aside)"""
        lost = self.blocks_on(b, self.devs)
        bad = np.zeros(self.S, dtype=bool)
        for j in range(self.n):
            if j not in lost:
                bad |= self.block(self.mirror_d, self.mirror_p, b, j) != self.block(self.truth_d, self.truth_p, b, j)
        return np.nonzero(bad)[0]

    def write_legal(self, b, form, col0, width):
        """include/fastecc.h, "Inside the window the inputs of touched stripes' present blocks must be < p" and what makes the answer unique: the
        stripe is not quarantined and inside the window's columns every PRESENT block equals the truth; absent blocks only under a _set form"""
        if b in self.quarantined or (form not in SET_FORMS and self.absent[b]):
            return False
        if not self.corrupt[b]:
            return True
        lost = self.lost_for_write(b, form)
        return all(np.array_equal(self.block(self.mirror_d, self.mirror_p, b, j)[col0:col0 + width], self.block(self.truth_d, self.truth_p, b, j)[col0:col0 + width])
                   for j in range(self.n) if j not in lost)

    def _write_degraded(self, op, pay, writes, touched):
        """the _set forms and the window forms (include/fastecc.h: "Degraded writes", "Sub-block writes"): the truth takes the rows in the window and
        the oracle's whole re-encode; every PRESENT block of a touched stripe takes the truth in the window's columns; nothing else changes"""
        form, S = op["form"], self.S
        col0, width = op.get("col0", 0), op.get("width", S)
        if form not in WINDOW_FORMS:
            raise ModelError("the forms single and pool keep no window")
        if not writes or width < 1 or col0 < 0 or col0 + width > S:
            raise ModelError("no such write")
        if form in SET_FORMS:
            if self.ctx.prepared_set != self.needed_set():
                raise ModelError("the prepared pattern set is stale")
            if op["pattern_of"] != self.pattern_of(0, self.count, lambda b: b not in self.quarantined):
                raise ModelError("pattern_of does not skip what it must")
            if op.get("ignored") is not None and op["ignored"] in touched:
                raise ModelError("the entry to ignore belongs to a touched stripe")
        for b in touched:
            if not self.write_legal(b, form, col0, width):
                raise ModelError("a %s write into stripe %d: quarantined, an absent block under a plain form, or a wrong word in the window" % (form, b))
        for u, w in enumerate(writes):
            self.truth_d[w // self.k, w % self.k, col0:col0 + width] = pay["new"][u]
        for b in touched:
            self.truth_p[b] = self.codec.parity(self.truth_d[b])
            lost = self.lost_for_write(b, form)
            for j in range(self.n):
                src, dst = self.block(self.truth_d, self.truth_p, b, j), self.block(self.mirror_d, self.mirror_p, b, j)
                if j not in lost:
                    dst[col0:col0 + width] = src[col0:col0 + width]
                elif not np.array_equal(src, dst):  # (a block rebuilt on a replaced device goes stale again: its pattern still calls it lost)
                    self.absent[b].add(j)

    def _probe_write(self, op, pay):
        """a degraded write into a scratch stripe (stripe b's truth, garbage where pattern q of the set lost a block); "after": a repair under the
        same pattern (every block is then the oracle's encode of X'), or a read of the written blocks on the other stream (the new rows)"""
        lost = self._set_pattern(op["q"])
        if op["form"] not in SET_FORMS or len(set(op["writes"])) != len(op["writes"]):
            raise ModelError("no such scratch write")
        return self._scratch_write(op, pay["scratch_d"], pay["scratch_p"], pay["new"], lost, op.get("after"))

    def _scratch_write(self, half, d, p, new, lost, after=None):
        """X' = stripe half["b"]'s true data with the rows in the window, its parity the oracle's: the present blocks take it in the window"""
        d, p, x = d.copy(), p.copy(), self.truth_d[half["b"]].copy()
        win = slice(half["col0"], half["col0"] + half["width"])
        for u, i in enumerate(half["writes"]):
            x[i, win] = new[u]
        xp = self.codec.parity(x)
        for j in range(self.n):
            src, dst = (x[j], d[j]) if j < self.k else (xp[j - self.k], p[j - self.k])
            if j not in lost:
                dst[win] = src[win]
            elif after == "repair":
                dst[:] = src
        out = {"code": OK, "scratch_d": d, "scratch_p": p}
        if after == "repair":
            out["codes"] = [OK, OK]
        if after == "read":
            out["codes"] = [OK, OK]
            out["rows"] = np.stack([x[i, win] for i in half["reads"]])
            out["guard"] = np.full(half["width"], CANARY, dtype=np.uint32)
        return out

    def _probe_write_swap(self, op, pay):
        """decode_prepare_set(first patterns), a degraded write on the side stream, decode_prepare_set(second patterns) with nothing synchronised, a
        degraded write: the first write's result is the first set's, the second follows the second set"""
        ds, ps = [], []
        for half, (d, p), new in zip(op["halves"], pay["scratch"], pay["new"]):
            self.ctx.prepared_set = tuple(tuple(q) for q in half["patterns"])
            out = self._scratch_write(dict(half, b=op["b"]), d, p, new, self.ctx.prepared_set[half["q"]])
            ds.append(out["scratch_d"])
            ps.append(out["scratch_p"])
        return {"code": OK, "codes": [OK] * 4, "scratch_d": np.stack(ds), "scratch_p": np.stack(ps)}

    def _prepare(self, op, pay):
        self.ctx.prepared = tuple(op["lost"])
        self.ctx.prepared_limit = self.ctx.options["decode_direct_max"]

    def _prepare_set(self, op, pay):
        self.ctx.prepared_set = tuple(tuple(q) for q in op["patterns"])

    def _scrub_pattern(self, op, pay):
        if self.mixed:
            return {"code": E_UNSUPPORTED}
        self.ctx.scrub = tuple(op["absent"])

    def _scrub_pattern_set(self, op, pay):
        if self.mixed:
            return {"code": E_UNSUPPORTED}
        self.ctx.scrub_set = tuple(tuple(q) for q in op["patterns"])

    def _check_budget(self, b0, b1):
        for b in range(b0, b1):
            if b not in self.quarantined and not self.budget(b):
                raise ModelError("stripe %d is beyond the correction guarantee" % b)

    def _verify(self, op, pay):
        if self.mixed:
            return {"code": E_UNSUPPORTED}
        self._scrub_ready(op["set"])
        self._check_budget(op["b0"], op["b1"])
        if op["set"] != self.rotated:
            raise ModelError("the pool's placement needs the other form")
        ok = [0 if self.corrupt[b] else 1 for b in range(op["b0"], op["b1"])]
        out = {"code": OK, "consistent": ok, "inconsistent": ok.count(0)}
        if op.get("single") is not None:
            b = op["single"]
            if b in self.quarantined or self.ctx.scrub != self.blocks_on(b, self.devs):
                raise ModelError("fastecc_verify of stripe %d needs its own pattern" % b)
            out["single"] = 0 if self.corrupt[b] else 1
        return out

    def _locate(self, op, pay):
        if self.mixed:
            return {"code": E_UNSUPPORTED}
        use_set = bool(op.get("set"))
        if use_set != self.rotated:
            raise ModelError("locate is a fixed-placement operation, locate under the set a rotated one")
        if use_set and op["pattern_of"] != self.pattern_of(op["b0"], op["b1"], lambda b: b not in self.quarantined):
            raise ModelError("pattern_of does not skip what it must")
        self._scrub_ready(use_set)
        self._check_budget(op["b0"], op["b1"])
        # stripe b's absent blocks (under the set those of its own pattern) are never read and never listed
        lists = [[] if b in self.quarantined else [j for j in sorted(self.corrupt[b]) if j not in self.blocks_on(b, self.devs)]
                 for b in range(op["b0"], op["b1"])]
        status = [1 if x else 0 for x in lists]
        return {"code": OK, "status": status, "lists": lists, "inconsistent": sum(status)}

    def _correct(self, op, pay):
        if self.mixed:
            return {"code": E_UNSUPPORTED}
        self._scrub_ready(op["set"])
        self._check_budget(op["b0"], op["b1"])
        if op["set"] != self.rotated:
            raise ModelError("the pool's placement needs the other form")
        status = []
        for b in range(op["b0"], op["b1"]):
            status.append(1 if self.corrupt[b] else 0)
            if self.corrupt[b]:
                self.mirror_d[b], self.mirror_p[b] = self.truth_d[b], self.truth_p[b]
                self.corrupt[b].clear()
                self.absent[b].clear()
        self.ctx.prepared = UNSPECIFIED
        self._settle()
        return {"code": OK, "status": status, "inconsistent": sum(status)}

    def _rebuild(self, op, data_only):
        if op["set"] != self.rotated:
            raise ModelError("the pool's placement needs the other form")
        if op["set"]:
            if self.ctx.prepared_set != self.needed_set():
                raise ModelError("the prepared pattern set is stale")
            want = self.pattern_of(op["b0"], op["b1"], lambda b: b not in self.quarantined and not self.corrupt[b])
            if op["pattern_of"] != want:
                raise ModelError("pattern_of does not skip what it must")
        elif self._prepared() != self.needed_single():
            raise ModelError("the prepared pattern is not the pool's")
        for b in range(op["b0"], op["b1"]):
            if b in self.quarantined or (op["set"] and self.corrupt[b]):
                continue
            if self.corrupt[b]:
                raise ModelError("stripe %d has a corrupted block: no repair" % b)
            for j in self.blocks_on(b, self.devs):
                if data_only and j >= self.k:
                    continue
                self.block(self.mirror_d, self.mirror_p, b, j)[:] = self.block(self.truth_d, self.truth_p, b, j)
                self.absent[b].discard(j)
        self._settle()

    def _repair(self, op, pay):
        self._rebuild(op, False)

    def _decode(self, op, pay):
        self._rebuild(op, True)

    def _reencode(self, op, pay):
        for b in range(op["b0"], op["b1"]):
            if b in self.quarantined or any(j < self.k for j in list(self.corrupt[b]) + list(self.absent[b])):
                raise ModelError("stripe %d has no clean data to encode" % b)
        return {"code": OK, "parity": self.truth_p[op["b0"]:op["b1"]].copy()}

    def _option(self, op, pay):
        if op["name"] == "locate_max" and not all(
                sum(1 for v in self.corrupt[b].values() if v == "small") <= op["value"] for b in self.live()):
            raise ModelError("locate_max below a stripe's t")
        self.ctx.options[op["name"]] = op["value"]
        return {}

    def _stream(self, op, pay):
        self.ctx.stream = op["stream"]
        return {}

    def _burst(self, op, pay):
        """several enqueued calls back to back, nothing read in between: the prediction is the calls applied in order"""
        pay["subs"], codes, reads = [], [], []
        for sub in op["ops"]:  # a read is drawn against the patterns as the burst meets them (a rebuild of the burst may bring a device back:
            if sub["op"] == "read":  # its blocks are then present and whole, and lost under the pattern in force — the truth either way)
                self._read_check(sub)
        for sub in op["ops"]:
            if sub["op"] not in ("write", "repair", "decode", "read"):
                raise ModelError("a burst holds enqueued calls only")
            pay["subs"].append(dict(self.payload(sub), in_burst=True))
            out = self.apply(sub, pay["subs"][-1])
            codes.append(out["code"])
            if sub["op"] == "read":
                reads.append(out)
        out = {"code": OK, "codes": codes}
        if reads:  # every read's rows, then every read's guard row, as the backend reads them back after the burst
            out["rows"] = np.concatenate([r["rows"].reshape(-1) for r in reads])
            out["guard"] = np.concatenate([r["guard"] for r in reads])
        return out

    def _read_check(self, op):
        if op["set"] != self.rotated:
            raise ModelError("the pool's placement needs the other form")
        if not op["reads"] or op["width"] < 1 or op["col0"] + op["width"] > self.S:
            raise ModelError("no such read")
        if op["set"]:
            if self.ctx.prepared_set != self.needed_set():
                raise ModelError("the prepared pattern set is stale")
            if op["pattern_of"] != self.pattern_of(0, self.count, lambda b: b not in self.quarantined):
                raise ModelError("pattern_of does not skip what it must")
        elif self._prepared() != self.needed_single():
            raise ModelError("the prepared pattern is not the pool's")

    def _read(self, op, pay):
        """fastecc_read_batch / _read_batch_set over the whole pool: a present block is a copy of the mirror, a lost one the truth"""
        if not pay.get("in_burst"):
            self._read_check(op)
        n, guard = len(op["reads"]), np.full(op["width"], CANARY, dtype=np.uint32)
        if not op["set"] and not self._served():
            return {"code": E_UNSUPPORTED, "rows": canary_rows(n, op["width"]), "guard": guard}
        rows = []
        for idx in op["reads"]:
            b, i = divmod(idx, self.k)
            if not 0 <= b < self.count:
                raise ModelError("no such block")
            if b not in self.quarantined and self.dev_of(b, i) in self.devs:  # lost under its stripe's pattern
                if self.corrupt[b]:
                    raise ModelError("a lost block of stripe %d, which has a corrupted survivor" % b)
                rows.append(window(self.truth_d[b, i], op))
            else:
                rows.append(window(self.mirror_d[b, i], op))
        return {"code": OK, "rows": np.stack(rows), "guard": guard}

    def _probe_read(self, op, pay):
        """a read of a scratch stripe (stripe b's truth, garbage where the pattern in force lost a block): the truth, whatever is asked for"""
        n, guard = len(op["reads"]), np.full(op["width"], CANARY, dtype=np.uint32)
        if op["set"]:
            self._set_pattern(op["q"])
        elif not self._served():
            return {"code": E_UNSUPPORTED, "rows": canary_rows(n, op["width"]), "guard": guard}
        return {"code": OK, "rows": np.stack([window(self.truth_d[op["b"], i], op) for i in op["reads"]]), "guard": guard}

    def _probe_read_swap(self, op, pay):
        """decode_prepare_set(first patterns), a read on the side stream, decode_prepare_set(second patterns) with nothing synchronised, a read"""
        rows = []
        for half in op["halves"]:
            self.ctx.prepared_set = tuple(tuple(q) for q in half["patterns"])
            rows.append(np.stack([window(self.truth_d[op["b"], i], half) for i in half["reads"]]).reshape(-1))
        return {"code": OK, "codes": [OK] * 4, "rows": np.concatenate(rows),
                "guard": np.concatenate([np.full(half["width"], CANARY, dtype=np.uint32) for half in op["halves"]])}

    def _probe_repair(self, op, pay):
        lost = self._prepared()
        d, p = pay["scratch_d"].copy(), pay["scratch_p"].copy()
        for j in lost:
            if j < self.k:
                d[j] = self.truth_d[op["b"], j]
            elif op["form"].startswith("repair"):
                p[j - self.k] = self.truth_p[op["b"], j - self.k]
        return {"code": OK, "scratch_d": d, "scratch_p": p}

    def _probe_repair_set(self, op, pay):
        if self.ctx.prepared_set is None:
            raise ModelError("no pattern set")
        d, p = pay["scratch_d"].copy(), pay["scratch_p"].copy()
        for j in self.ctx.prepared_set[op["q"]]:
            if j < self.k:
                d[j] = self.truth_d[op["b"], j]
            elif op["form"] == "repair":
                p[j - self.k] = self.truth_p[op["b"], j - self.k]
        return {"code": OK, "scratch_d": d, "scratch_p": p}

    def _probe_verify(self, op, pay):
        if self.mixed or op["j"] in self.ctx.scrub:
            raise ModelError("no scrub probe here")
        return {"code": OK, "ok": [1, 0]}

    def _refused(self, op, pay):
        if op["which"] == "bad_read":  # two refused reads, (n_reads + 1) rows each: all canary
            return {"code": E_INVAL, "codes": [E_INVAL, E_INVAL], "rows": canary_rows(2 * (len(op["reads"]) + 1), op["width"]).reshape(-1)}
        if op["which"] in ("bad_degraded_write", "no_set"):  # refused with nothing written: the pool (compared after every step) and the caller's rows
            if (op["which"] == "no_set") != (self.ctx.prepared_set is None):
                raise ModelError("refused_no_set needs a context without a set, every other refusal one with a set")
            # but for the argument that the variant spoils the call is a write the model allows: nothing else can be the reason to refuse it
            if op["which"] == "bad_degraded_write" and (self.ctx.prepared_set != self.needed_set() or op["entry"] != len(self.ctx.prepared_set)):
                raise ModelError("the pool's own set is not the one in force, or the entry is not its number of patterns")
            if op["pattern_of"] != self.pattern_of(0, self.count, lambda b: b not in self.quarantined) or len(set(op["writes"])) != len(op["writes"]):
                raise ModelError("pattern_of or the write list would be refused by itself")
            if op["width"] < 1 or op["col0"] + op["width"] > self.S or not op["writes"] or not all(
                    0 <= w < self.count * self.k and self.write_legal(w // self.k, op["form"], op["col0"], op["width"]) for w in op["writes"]):
                raise ModelError("the write would not be legal without the variant's own argument")
            call = (op["call_col0"], op["call_width"])
            want = {"width0": (op["col0"], 0), "past_end": (self.S + 1 - op["width"], op["width"]), "overflow": ((1 << 64) - 1, 2)}
            if call != want.get(op.get("variant"), (op["col0"], op["width"])):
                raise ModelError("the window of the call is not what the variant says")
            codes = [E_INVAL] * len(op["entries"])
            return {"code": E_INVAL, "codes": codes, "rows": pay["new"].reshape(-1)}
        return {"code": E_INVAL}


# ---- the generator: reads the model only ----
KINDS = ("write", "corrupt", "device_down", "device_replaced", "verify", "locate", "correct", "repair", "decode", "reencode", "option",
         "stream", "burst")
# the state probes, met in turn: a sequence runs PROBES_PER_SEQUENCE of them at fixed steps, starting where its seed and placement say, so
# that the four seeds and two placements of a configuration meet every probe at least twice
PROBES = [("prepared", "prepare_set"), ("set", "prepare"), ("scrub", "prepare"), ("refused", "bad_write"), ("prepared", "scrub_pattern"),
          ("set", "single"), ("prepared", "locate"), ("scrub", "single"), ("refused", "bad_pattern"), ("prepared", "scrub_pattern_set"),
          ("set", "batch"), ("prepared", "write"), ("scrub", "correct"), ("refused", "count0"), ("prepared", "verify"), ("set", "correct")]
PROBES_PER_SEQUENCE = 5
WEIGHTS = {"write": 12, "corrupt": 12, "device_down": 6, "device_replaced": 9, "verify": 7, "locate": 6, "correct": 7, "repair": 7,
           "decode": 5, "reencode": 5, "option": 6, "stream": 4, "burst": 8}


# Extended sequences (the seeds EXT_SEEDS): the kinds above and "read"; "locate" on rotated pools too (fastecc_locate_errors_batch_set); writes
# and re-encodes have the form "pool" (fastecc_encode_pool); option "encode_pool_kernel" is flipped; bursts hold reads.  Their probes are
# EXT_PROBES, met in turn like PROBES: the two seeds and two placements of a configuration start 5 apart, so every probe is met at least twice.
EXT_KINDS = KINDS + ("read",)
EXT_WEIGHTS = dict(WEIGHTS, read=16, write=20, reencode=18, locate=9)
EXT_PROBES = [("read", "prepare"), ("prepared", "read"), ("set", "read"), ("scrub", "read"), ("read", "prepare_transform"),
              ("read", "prepare_set"), ("refused", "bad_read"), ("read", "prepare_parity"), ("prepared", "locate")]
WINDOWS = ("whole", "word", "narrow", "tail")

# Degraded sequences (the seeds DEG_SEEDS): the extended kinds, with writes of the forms "batch_set" and "parity_set" (fastecc_update_batch_set,
# _update_parity_batch_set) that go on while devices are down, and a column window on the four pool forms (the fastecc_update_*_window calls).  A
# window has one of the shapes of WINDOWS or, for the vector-width rule, "quad" (col0 and width multiples of 4: every configuration's S is one,
# so 4 words per lane) or "pair" (both even, not both multiples of 4).  Their probes are DEG_PROBES, met in turn like EXT_PROBES; step 0 of the
# seed DEG_SEEDS[0] is refused_no_set (no later step can meet a context without a set).
WRITE_WINDOWS = WINDOWS + ("quad", "pair")
DEG_WEIGHTS = {"write": 40, "burst": 24, "corrupt": 12, "device_down": 10, "device_replaced": 8, "verify": 2, "locate": 2, "correct": 4, "repair": 8,
               "decode": 3, "reencode": 3, "option": 3, "stream": 4, "read": 10}
DEG_PROBES = [("prepared", "degraded_write"), ("write", "prepare_set"), ("set", "degraded_write"), ("write", "read"), ("scrub", "degraded_write"),
              ("write", "repair"), ("refused", "bad_degraded_write"), ("write", "ignored")]
BAD_DEGRADED_WRITES = ("entry", "null_pattern_of", "width0", "past_end", "overflow", "overlap")


class Generator:
    def __init__(self, model, seed, extended=False, degraded=False):
        self.m, self.rng = model, _rng("gen", model.cfg.name, seed)
        self.degraded, extended = degraded, extended or degraded
        self.bad_writes, self.absent_written = 0, []
        self.queue = collections.deque()
        self.drawn = self.skipped = 0
        self.dseed = 0
        self.verifies = 0
        m = model
        self.extended, self.seed, self.pool_encodes, self.used_form = extended, seed, 0, collections.Counter()
        self.weights, self.probe_list = (DEG_WEIGHTS, DEG_PROBES) if degraded else (EXT_WEIGHTS, EXT_PROBES) if extended else (WEIGHTS, PROBES)
        kinds = [k for k in (EXT_KINDS if extended else KINDS)
                 if not (m.mixed and k == "corrupt") and not (m.rotated and k == "locate" and not extended)]
        self.emitted = self.probes_started = 0
        self.probe_at = 5 * (seed - EXT_SEEDS[0] + (2 if m.rotated else 0)) if extended else 2 * (seed + (4 if model.rotated else 0))
        if degraded:
            self.probe_at = 5 * (seed - DEG_SEEDS[0] + (2 if m.rotated else 0))
        self.kinds = kinds
        self.used = collections.Counter()

    def _ds(self):
        self.dseed += 1
        return self.dseed

    def _pick(self, seq):
        seq = list(seq)
        return seq[int(self.rng.integers(len(seq)))]

    def _next_probe(self):
        m = self.m
        for _ in range(len(self.probe_list)):
            family, variant = self.probe_list[self.probe_at % len(self.probe_list)]
            skip = ((m.mixed and (family == "scrub" or variant in ("correct", "locate")))
                    or (m.rotated and variant == "locate" and not self.extended))
            if not skip:
                ops = getattr(self, "make_probe_" + family)(variant)
                if ops is None:
                    return None  # not now: the same probe at the next draw
            self.probe_at += 1
            if not skip:
                self.probes_started += 1
                return ops

    def _draw_kind(self):
        """by weight, a kind this sequence has not run yet three times as likely"""
        m = self.m
        idle = {"device_replaced": "down" not in m.devs.values(),
                "device_down": len(m.devs) >= min(m.m, 2) or not all(m.budget(b, extra_w=1) for b in m.live()),
                "write": not any(m.whole(b) for b in m.live())}
        idle["burst"] = idle["write"]
        if self.extended:
            if any(not m.absent[b] for b in m.live()):  # a whole-stripe write takes corrupted stripes too
                idle["write"] = False
            idle["reencode"] = not any(not any(j < m.k for j in list(m.corrupt[b]) + list(m.absent[b])) for b in m.live())
        if self.degraded:  # the _set forms go on writing while devices are down
            idle["write"] = idle["burst"] = False
            # (first the plain forms, which need stripes without absent blocks)
            idle["device_down"] = idle["device_down"] or (self.emitted <= 26 and self._plain_forms_due())
        w = np.array([self.weights[k] * (0.25 if idle.get(k) else 3.0 if not self.used[k] else 1.0) for k in self.kinds])
        if self.degraded and m.devs and not self.used_form["burst_pair"]:  # a device is down: the burst with a pair of rebuilding calls, soon
            w[self.kinds.index("burst")] *= 3
        if self.degraded and self._forms_due():
            w[self.kinds.index("write")] *= 2.5
        if self.degraded and not m.devs:  # bursts are for the time a device is down; the plain forms, and one directly after a prepare_set, for now
            w[self.kinds.index("burst")] *= 0.4
            w[self.kinds.index("write")] *= 1.6
            if not self._plain_forms_due():
                w[self.kinds.index("device_down")] *= 3
        return self.kinds[int(self.rng.choice(len(self.kinds), p=w / w.sum()))]

    def _range(self, ok=None):
        """the whole pool, or with probability 1/3 a sub-range; with `ok` a run of stripes that all satisfy it (None if there is none)"""
        m, rng = self.m, self.rng
        if ok is None:
            if rng.random() < 0.35 and m.count > 2:
                b0 = int(rng.integers(0, m.count - 1))
                return b0, int(rng.integers(b0 + 1, m.count + 1))
            return 0, m.count
        runs, b = [], 0
        while b < m.count:
            if ok(b):
                e = b
                while e < m.count and ok(e):
                    e += 1
                runs.append((b, e))
                b = e
            else:
                b += 1
        if not runs:
            return None
        b0, b1 = max(runs, key=lambda r: r[1] - r[0]) if rng.random() < 0.6 else self._pick(runs)
        if rng.random() < 0.3 and b1 - b0 > 1:
            b0 = int(rng.integers(b0, b1 - 1))
            b1 = int(rng.integers(b0 + 1, b1 + 1))
        return b0, b1

    # state operations
    def _state_prepare(self, lost=None):
        return {"op": "prepare", "lost": list(self.m.needed_single() if lost is None else lost)}

    def _random_pattern(self, most):
        m = self.m
        r = int(self.rng.integers(1, max(1, min(m.m, most)) + 1))
        return sorted(int(x) for x in self.rng.choice(m.n, size=r, replace=False))

    def _any_set(self):
        m = self.m
        if m.rotated:
            return [list(q) for q in m.needed_set()]
        return [self._random_pattern(4) for _ in range(3)]

    def _state_prepare_set(self):
        return {"op": "prepare_set", "patterns": self._any_set()}

    def _state_scrub(self):
        m = self.m
        absent = m.blocks_on(self._pick(m.live()), m.devs) if m.rotated else m.needed_single()
        return {"op": "scrub_pattern", "absent": list(absent)}

    def _state_scrub_set(self):
        return {"op": "scrub_pattern_set", "patterns": self._any_set()}

    def _scrub_prereq(self):
        m = self.m
        if m.mixed:
            return None
        if m.rotated:
            return self._state_scrub_set() if m.ctx.scrub_set != m.needed_set() else None
        return self._state_scrub() if m.ctx.scrub != m.needed_single() else None

    def _rebuild_prereq(self):
        m = self.m
        if m.rotated:
            return self._state_prepare_set() if m.ctx.prepared_set != m.needed_set() else None
        return self._state_prepare() if m.ctx.prepared != m.needed_single() else None

    # operations: each returns a list of operations (prerequisites first) or None when the state does not allow it
    def make_write(self, in_burst=False):
        m, rng = self.m, self.rng
        if self.degraded:
            return self._make_degraded_write(in_burst)
        # extended: whole stripes — new data and fastecc_encode_pool over the run — two times in five, and outside bursts a sequence's first two
        # writes and every write while no stripe is whole.  Corrupted stripes qualify (the write makes them whole), but not inside a burst, whose
        # other calls were drawn against the marks as they are
        pool = self.extended and rng.random() < 0.4
        if self.extended and not in_burst and (self.used_form["write_pool"] < 2 or not any(m.whole(b) for b in m.live())):
            pool = True
        if pool:
            self.used_form["write_pool"] += 1
            r = self._range((lambda b: m.whole(b)) if in_burst else (lambda b: b not in m.quarantined and not m.absent[b]))
            return None if r is None else [{"op": "write", "form": "pool", "b0": r[0], "b1": r[1], "dseed": self._ds()}]
        whole = [b for b in range(m.count) if m.whole(b)]
        if not whole:
            return None
        form = self._pick(["batch", "batch", "batch", "parity", "parity", "single"])
        if form == "single":
            b = self._pick(whole)
            blocks = rng.choice(m.k, size=int(rng.integers(1, min(m.k, 20) + 1)), replace=False)
            writes = [b * m.k + int(i) for i in blocks]
        else:
            total = int(rng.integers(1, 41))
            writes = []
            if m.k > 16 and rng.random() < 0.4:  # more than 16 writes in one stripe: a second round
                b = self._pick(whole)
                writes = [b * m.k + int(i) for i in rng.choice(m.k, size=int(rng.integers(17, min(m.k, 36) + 1)), replace=False)]
            taken = set(writes)
            free = [b * m.k + i for b in whole for i in range(m.k) if b * m.k + i not in taken]
            more = max(0, min(total - len(writes), len(free))) if writes else min(total, len(free))
            writes += [int(x) for x in rng.choice(free, size=more, replace=False)]
            writes = [writes[i] for i in rng.permutation(len(writes))]
        return [{"op": "write", "form": form, "writes": writes, "dseed": self._ds()}]

    # -- degraded sequences: writes of the _set forms and column windows
    def _write_window(self, shape=None):
        """(shape, col0, width) of a write: _window()'s four shapes, "quad" (col0 and width multiples of 4) and "pair" (both even, col0 = 2 mod 4)"""
        S, rng = self.m.S, self.rng
        shape = shape or self._pick(WRITE_WINDOWS)
        if shape == "quad":
            col0 = 4 * int(rng.integers(S // 4))
            return shape, col0, 4 * int(rng.integers(1, (S - col0) // 4 + 1))
        if shape == "pair":
            col0 = 2 + 4 * int(rng.integers((S - 4) // 4 + 1))
            return shape, col0, 2 * int(rng.integers(1, (S - col0) // 2 + 1))
        return self._window(shape)

    def _forms_due(self):
        """a (form, window or not) of the four pool forms has not run twice in this sequence yet"""
        return any(self.used_form[f, w] < 2 for f in WINDOW_FORMS for w in (True, False))

    def _plain_forms_due(self):
        return any(self.used_form[f, w] < 2 for f in ("batch", "parity") for w in (True, False))

    def _needed_set_op(self):
        return {"op": "prepare_set", "patterns": [list(q) for q in self.m.needed_set()]}

    def _set_prereq(self):
        """what makes the pool's own patterns the set in force ([] when they are); a fixed pool uses the same set, every pattern needed_single()"""
        return [self._needed_set_op()] if self.m.ctx.prepared_set != self.m.needed_set() else []

    def _beside_corruption(self):
        """(stripe, shape, col0, width): a stripe whose present blocks are wrong in a few word columns only, and a window that misses them all"""
        m = self.m
        for b in [b for b in m.live() if m.corrupt[b]]:
            cols = m.wrong_columns(b)
            if 1 <= len(cols) <= 24:
                for _ in range(8):
                    shape, col0, width = self._write_window(self._pick(WRITE_WINDOWS[1:]))
                    if not ((cols >= col0) & (cols < col0 + width)).any():
                        return b, shape, col0, width
        return None

    def _degraded_write(self, want_rebuilt=False, whole_block=None, form=None, in_burst=False):
        """(prerequisites, a write of one of the four pool forms) or None.  One list holds absent data blocks, present data blocks of degraded stripes
        and stripes that lose parity only or nothing, whichever the pool has; where k > 16 a stripe with more than 16 writes two times in five.
        want_rebuilt: form "batch_set" with at least two absent data blocks written (their old rows are rebuilt).  whole_block: True the whole-block
        entry point, False a window narrower than the block, None either.  in_burst: a plain form keeps to stripes with no block on a device that is
        down or replaced (a _set write earlier in the burst leaves such a block, rebuilt since, stale again: the stripe then has an absent block)."""
        m, rng = self.m, self.rng
        if want_rebuilt:
            form = "batch_set"
        if form is None or whole_block is None:  # the (form, window or not) that this sequence has used least, among those the pool allows now: the
            # plain forms need stripes without absent blocks, so while no device is down or replaced they come first, until each has run twice
            forms = [form] if form else list(SET_FORMS) if m.devs or (not self._plain_forms_due() and rng.random() < 0.75) else ["batch", "parity"]
            combos = [(f, w) for f in forms for w in ([True, False] if whole_block is None else [whole_block])]
            least = min(self.used_form[c] for c in combos)
            form, whole_block = self._pick([c for c in combos if self.used_form[c] == least])
        target = None
        shape, col0, width = None, 0, m.S  # (shape None: the whole-block entry point)
        if not whole_block:
            shape, col0, width = self._write_window(self._pick(WRITE_WINDOWS[1:]) if want_rebuilt else None)
            if not m.mixed and (rng.random() < 0.6 or not self.used_form["beside"]):
                beside = self._beside_corruption()
                if beside:
                    target, shape, col0, width = beside
                    self.used_form["beside"] += 1
        legal = [b for b in m.live() if m.write_legal(b, form, col0, width) and not (in_burst and form not in SET_FORMS and m.blocks_on(b, m.devs))]
        if not legal:
            return None
        absent_d = [b * m.k + i for b in legal for i in m.lost_for_write(b, form) if i < m.k]
        if want_rebuilt and len(absent_d) < 2:
            return None
        writes = []
        if m.k > 16 and rng.random() < 0.4:  # more than 16 writes in one stripe, its absent data blocks among them: a second round
            with_absent = [b for b in legal if any(i < m.k for i in m.lost_for_write(b, form))]
            b = self._pick(with_absent if with_absent and rng.random() < 0.7 else legal)
            first = [i for i in m.lost_for_write(b, form) if i < m.k]
            rest = [int(i) for i in rng.permutation(m.k) if int(i) not in first]
            writes = [b * m.k + i for i in (first + rest)[: int(rng.integers(17, min(m.k, 36) + 1))]]
        if target is not None and target in legal and not any(w // m.k == target for w in writes):
            writes.append(target * m.k + int(rng.integers(m.k)))
        if absent_d and (want_rebuilt or rng.random() < 0.7):
            more = [int(x) for x in rng.choice(absent_d, size=min(len(absent_d), int(rng.integers(2, 5))), replace=False)]
            writes += [w for w in more if w not in writes]
        parity_only = [b for b in legal if m.lost_for_write(b, form) and min(m.lost_for_write(b, form)) >= m.k]
        if parity_only and rng.random() < 0.8:  # a stripe that loses parity only
            w = self._pick(parity_only) * m.k + int(rng.integers(m.k))
            writes += [w] if w not in writes else []
        taken = set(writes)
        free = [b * m.k + i for b in legal for i in range(m.k) if b * m.k + i not in taken]
        more = min(max(0 if writes else 1, int(rng.integers(1, 41)) - len(writes)), len(free))
        writes += [int(x) for x in rng.choice(free, size=more, replace=False)]
        writes = [writes[i] for i in rng.permutation(len(writes))]
        self.used_form[form, whole_block] += 1
        op = {"op": "write", "form": form, "writes": writes, "dseed": self._ds()}
        if shape is not None:
            op.update(col0=col0, width=width, shape=shape)
        if form in SET_FORMS:
            op["pattern_of"] = m.pattern_of(0, m.count, lambda b: b not in m.quarantined)
            self.absent_written += [w for w in writes if w in absent_d]
        return (self._set_prereq() if form in SET_FORMS else []), op

    def _make_degraded_write(self, in_burst=False):
        m, rng = self.m, self.rng
        if not in_burst and rng.random() < 0.12:  # whole stripes, as in the extended sequences
            r = self._range(lambda b: b not in m.quarantined and not m.absent[b])
            if r is not None:
                self.used_form["write_pool"] += 1
                return [{"op": "write", "form": "pool", "b0": r[0], "b1": r[1], "dseed": self._ds()}]
        if not in_burst and rng.random() < 0.08 and any(m.whole(b) for b in m.live()):  # fastecc_update on one whole stripe
            b = self._pick([b for b in m.live() if m.whole(b)])
            blocks = rng.choice(m.k, size=int(rng.integers(1, min(m.k, 20) + 1)), replace=False)
            return [{"op": "write", "form": "single", "writes": [b * m.k + int(i) for i in blocks], "dseed": self._ds()}]
        r = self._degraded_write(in_burst=in_burst)
        if r is None:
            return None
        pre, op = r
        # a plain window write directly after a decode_prepare_set of other patterns: the "loses nothing" row survives the swap of tables
        if not in_burst and op["form"] in ("batch", "parity") and "width" in op and (rng.random() < 0.5 or not self.used_form["window_after_set"]):
            self.used_form["window_after_set"] += 1
            return [{"op": "prepare_set", "patterns": self._write_patterns()}, op]
        if not in_burst and rng.random() < 0.6:  # a second write as the next step (drawn like a burst's: the first may leave a rebuilt block stale)
            second = self._degraded_write(in_burst=True)
            if second:
                return pre + [op] + [x for x in second[0] if x not in pre] + [second[1]]
        return pre + [op]

    def _write_patterns(self):
        """three patterns for a scratch write, each losing at least one data block"""
        m, out = self.m, []
        for _ in range(3):
            q = self._random_pattern(4)
            if q[0] >= m.k:
                q = sorted([int(self.rng.integers(m.k))] + q[1:])
            out.append(q)
        return out

    def _probe_write(self, patterns, q, probe=None, after=None):
        """a degraded write into a scratch stripe under pattern q: absent data blocks and present ones in one list, usually a window"""
        m, rng = self.m, self.rng
        lost_d = [j for j in patterns[q] if j < m.k]
        n = int(rng.integers(17, min(m.k, 30) + 1)) if m.k > 16 and rng.random() < 0.3 else int(rng.integers(1, min(m.k - len(lost_d), 5) + 1))
        writes = lost_d + [int(i) for i in rng.permutation(m.k) if int(i) not in lost_d][:n]
        writes = [writes[i] for i in rng.permutation(len(writes))]
        if after is None and (self.used_form["probe_write"] + self.seed) % 2 == 0:  # every other one through the whole-block entry point
            shape, col0, width = "whole_block", 0, m.S
        else:
            shape, col0, width = self._write_window(self._pick(WRITE_WINDOWS[1:]) if after == "repair" else None)
        self.used_form["probe_write"] += after is None
        op = {"op": "probe_write", "b": self._pick(m.live()), "q": q, "form": self._pick(["batch_set", "batch_set", "parity_set"]), "writes": writes,
              "col0": col0, "width": width, "shape": shape, "dseed": self._ds(), "probe": probe}
        if after:
            op["after"] = after
        if after == "read":  # the written blocks, the absent ones first, a duplicate
            op["reads"] = lost_d + writes[:2] + lost_d[:1]
        return op

    def _scratch_set_write(self, probe=None, after=None):
        sp = {"op": "prepare_set", "patterns": self._write_patterns()}
        return [sp, self._probe_write(sp["patterns"], int(self.rng.integers(3)), probe, after)]

    def make_probe_write(self, x):
        """write_after_prepare_set, read_after_degraded_write, repair_after_degraded_write, untouched_pattern_ignored"""
        m, rng = self.m, self.rng
        if x == "prepare_set":
            halves = []
            for _ in range(2):
                patterns = self._write_patterns()
                w = self._probe_write(patterns, int(rng.integers(3)))
                halves.append({"patterns": patterns, "q": w["q"], "form": w["form"], "writes": w["writes"], "col0": w["col0"], "width": w["width"],
                               "shape": w["shape"]})
            return [{"op": "probe_write_swap", "halves": halves, "b": self._pick(m.live()), "dseed": self._ds(), "probe": "write_after_prepare_set"}]
        if x == "read":
            return self._scratch_set_write("read_after_degraded_write", "read")
        if x == "repair":
            return self._scratch_set_write("repair_after_degraded_write", "repair")
        r = self._degraded_write(form=self._pick(SET_FORMS))  # "ignored": the entry of a stripe that no write names is the number of patterns
        if r is None:
            return None
        pre, op = r
        others = [b for b in range(m.count) if b not in {w // m.k for w in op["writes"]}]
        if not others:
            return None
        op.update(ignored=self._pick(others), entry=m.npat, probe="untouched_pattern_ignored")
        return pre + [op]

    def _refused_degraded_write(self, which):
        """A degraded write that must be refused: `which` "no_set" (no set was ever prepared) or "bad_degraded_write", one variant per draw.  The
        operation is a write that the model would allow — the pool's own set in force, legal stripes, a window inside the block — so that the one
        argument the backend then spoils is the only reason to refuse it; "call_col0" / "call_width" are the window as the call gets it.  The
        variants that are no matter of the window go through the whole-block entry point and the window entry point, one call each."""
        m, rng = self.m, self.rng
        used, absent_written = self.used_form.copy(), list(self.absent_written)
        r = self._degraded_write(form=self._pick(SET_FORMS), whole_block=False)
        self.used_form, self.absent_written = used, absent_written  # (nothing is written)
        if r is None:
            return None
        pre, w = r
        op = {"op": "refused", "which": which, "form": w["form"], "writes": w["writes"][:5], "pattern_of": w["pattern_of"], "col0": w["col0"],
              "width": w["width"], "shape": w["shape"], "call_col0": w["col0"], "call_width": w["width"], "entries": ["window"],
              "dseed": w["dseed"], "probe": "refused_" + which}
        if which == "no_set":
            return [op]
        variant = BAD_DEGRADED_WRITES[(self.bad_writes + self.seed + CONFIGS.index(m.cfg) // 2 + (3 if m.rotated else 0)) % len(BAD_DEGRADED_WRITES)]
        self.bad_writes += 1
        op.update(variant=variant, entry=m.npat)
        if variant in ("entry", "null_pattern_of", "overlap"):
            op["entries"] = ["whole_block", "window"]
        elif variant == "width0":
            op["call_width"] = 0
        elif variant == "past_end":
            op["call_col0"] = m.S + 1 - op["width"]
        elif variant == "overflow":
            op.update(call_col0=(1 << 64) - 1, call_width=2)
        return pre + [op]

    def _make_degraded_burst(self):
        """Enqueued calls back to back.  Where absent data blocks can be written, its middle is read, write, write, read on alternating streams:
        both writes rebuild old rows, one a window call and one a whole-block call (in either order: different widths of the one reconstruction
        buffer), and each read asks for absent blocks that the write beside it replaces."""
        m, rng = self.m, self.rng
        pre, mid = [], []

        def add(to, made):
            if made:
                for x in made[:-1]:
                    if x not in pre:
                        pre.append(x)
                to.append(made[-1])

        def absent_of(w):
            return [x for x in w["writes"] if (x % m.k) in m.lost_for_write(x // m.k, "batch_set") and not m.corrupt[x // m.k]]
        if m.devs and (rng.random() < 0.8 or not self.used_form["burst_pair"]):
            window_first = (self.used_form["burst_pair"] + self.seed) % 2 == 0
            first = self._degraded_write(want_rebuilt=True, whole_block=not window_first, in_burst=True)
            second = self._degraded_write(want_rebuilt=True, whole_block=window_first, in_burst=True) if first else None
            if first:
                self.used_form["burst_pair"] += 1
                add(mid, self.make_read(prefer=absent_of(first[1])))
                add(mid, list(first[0]) + [first[1]])
                if second and second[1].get("width", m.S) != first[1].get("width", m.S):
                    add(mid, list(second[0]) + [second[1]])
                add(mid, self.make_read(prefer=absent_of(mid[-1])))
        before, after = [], []
        for _ in range(int(rng.integers(1, 3) if mid else rng.integers(2, 4))):
            add(before if rng.random() < 0.5 else after, self.make_write(in_burst=True))
        if not mid and rng.random() < 0.5:
            add(after if rng.random() < 0.5 else before, self.make_read())
        ops = before + mid + after
        if self._rebuild_prereq() is None and rng.random() < 0.3:  # a rebuild, last: the calls before it were drawn against the patterns as they are
            r = self._make_rebuild(self._pick(["repair", "decode"]))
            if r:
                ops.append(r[-1])
        if len(ops) < 2:
            return None
        for sub in ops:
            sub["stream"] = int(rng.integers(2))
        for i, sub in enumerate(mid):
            sub["stream"] = (mid[0]["stream"] + i) % 2
        return pre + [{"op": "burst", "ops": ops}]

    def make_corrupt(self):
        m, rng = self.m, self.rng
        how = self._pick(["word", "word", "block", "big"])
        if self.degraded and how == "block" and rng.random() < 0.6:  # a single wrong word leaves room for a window beside it
            how = "word"
        for _ in range(16):
            b = self._pick(m.live())
            free = [j for j in range(m.n) if m.dev_of(b, j) not in m.devs and j not in m.corrupt[b]]
            r, u = 1, rng.random()
            if m.m >= 40 and u < 0.2:  # more than 16 blocks to rebuild in one repair
                r, how = int(rng.integers(17, 21)), "word"
            elif u < 0.35:
                r = int(rng.integers(2, 9))
            small = how != "big"
            while r > 0 and not m.budget(b, extra_t=r if small else 0, extra_b=0 if small else r):
                r = r // 2 if r > 2 else r - 1
            if r > 0 and len(free) >= r:
                return [{"op": "corrupt", "b": b, "blocks": sorted(int(x) for x in rng.choice(free, size=r, replace=False)), "how": how,
                         "dseed": self._ds()}]
        return None

    def make_device_down(self):
        m = self.m
        if len(m.devs) >= min(m.m, 2) or not all(m.budget(b, extra_w=1) for b in m.live()):
            return None
        up = [d for d in range(m.n) if d not in m.devs]
        if self.degraded:  # a device whose loss costs some stripes a data block and others parity only; on a fixed pool first a data block's device
            live = m.live()
            both = [d for d in up if len({j < m.k for b in live for j in m.blocks_on(b, [d])}) == 2]
            up = both if both and self.rng.random() < 0.8 else [d for d in up if (d < m.k) != bool(m.devs)] if not m.rotated else up
        return [{"op": "device_down", "dev": self._pick(up), "dseed": self._ds()}]

    def make_device_replaced(self):
        down = [d for d, s in self.m.devs.items() if s == "down"]
        return [{"op": "device_replaced", "dev": self._pick(down)}] if down else None

    def make_verify(self):
        m = self.m
        pre = self._scrub_prereq()
        b0, b1 = self._range()
        op = {"op": "verify", "set": m.rotated, "b0": b0, "b1": b1, "seed": int(self.rng.integers(1 << 40)), "single": None}
        if m.rotated:
            op["pattern_of"] = m.pattern_of(b0, b1, lambda b: b not in m.quarantined)
        self.verifies += 1
        ops = [pre] if pre else []
        if not m.mixed and self.verifies % 2 == 0:  # fastecc_verify of one stripe as well, under the single pattern
            if m.rotated:
                op["single"] = self._pick(m.live())
                if m.ctx.scrub != m.blocks_on(op["single"], m.devs):
                    ops.append({"op": "scrub_pattern", "absent": list(m.blocks_on(op["single"], m.devs))})
            elif pre is not None or m.ctx.scrub == m.needed_single():
                op["single"] = self._pick(m.live())
        return ops + [op]

    def make_locate(self):
        pre = self._scrub_prereq()
        b0, b1 = self._range()
        op = {"op": "locate", "b0": b0, "b1": b1, "seed": int(self.rng.integers(1 << 40))}
        if self.extended:  # fastecc_locate_errors_batch_set on rotated pools, pattern_of as for verify
            op["set"] = self.m.rotated
            if self.m.rotated:
                op["pattern_of"] = self.m.pattern_of(b0, b1, lambda b: b not in self.m.quarantined)
        return ([pre] if pre else []) + [op]

    def make_correct(self):
        m = self.m
        pre = self._scrub_prereq()
        b0, b1 = self._range()
        op = {"op": "correct", "set": m.rotated, "b0": b0, "b1": b1, "seed": int(self.rng.integers(1 << 40)),
              "mode": int(self.rng.integers(3))}
        if m.rotated:
            op["pattern_of"] = m.pattern_of(b0, b1, lambda b: b not in m.quarantined)
        return ([pre] if pre else []) + [op]

    def _make_rebuild(self, kind):
        m = self.m
        if m.rotated:
            b0, b1 = self._range()
        else:
            r = self._range(lambda b: not m.corrupt[b])
            if r is None:
                return None
            b0, b1 = r
        pre = self._rebuild_prereq()
        op = {"op": kind, "set": m.rotated, "b0": b0, "b1": b1, "kernel": int(self.rng.integers(3))}
        if m.rotated:
            op["pattern_of"] = m.pattern_of(b0, b1, lambda b: b not in m.quarantined and not m.corrupt[b])
        return ([pre] if pre else []) + [op]

    def make_repair(self):
        return self._make_rebuild("repair")

    def make_decode(self):
        return self._make_rebuild("decode")

    def make_reencode(self):
        m = self.m

        def clean(b):
            return b not in m.quarantined and not any(j < m.k for j in list(m.corrupt[b]) + list(m.absent[b]))
        good = [b for b in range(m.count) if clean(b)]
        if not good:
            return None
        if self.extended and (self.rng.random() < 0.6 or self.pool_encodes < 2):  # fastecc_encode_pool into the scratch parity, the kernel choice flipped first
            b0, b1 = self._range(clean)
            # under each kernel choice in turn (0 = choose, 1 = VALU, 2 = matrix cores), starting where the seed and the placement say
            want = (self.pool_encodes + self.seed + (1 if m.rotated else 0)) % 3
            self.pool_encodes += 1
            pre = [{"op": "option", "name": "encode_pool_kernel", "value": want}] if m.ctx.options["encode_pool_kernel"] != want else []
            return pre + [{"op": "reencode", "form": "pool", "b0": b0, "b1": b1}]
        if m.n == 2 * m.k and not m.mixed and self.rng.random() < 0.5:
            b0, b1 = self._range(clean)
            return [{"op": "reencode", "form": "batch", "b0": b0, "b1": b1}]
        b = self._pick(good)
        return [{"op": "reencode", "form": "one", "b0": b, "b1": b + 1}]

    def make_option(self):
        m = self.m
        name = self._pick(["scrub_batch_chunk", "scrub_batch_chunk", "direct_kernel", "decode_direct_max", "locate_max"]
                          + (["encode_pool_kernel"] * 3 if self.extended else []))
        if not m.mixed and self.used["option"] == 0:  # a sequence's first flip makes its scrub calls take several chunks
            return [{"op": "option", "name": "scrub_batch_chunk", "value": int(self._pick([3, 4]))}]
        if name == "encode_pool_kernel":  # 0 = choose, 1 = VALU, 2 = matrix cores (VALU where they cannot run): always another value
            return [{"op": "option", "name": name, "value": (m.ctx.options[name] + 1 + int(self.rng.integers(2))) % 3}]
        if name == "locate_max":
            t = max([sum(1 for v in m.corrupt[b].values() if v == "small") for b in m.live()] + [1])
            value = self._pick([v for v in (1, 2, 8, 256) if v >= t])
        else:
            value = self._pick({"scrub_batch_chunk": [0, 3, 4, 8], "direct_kernel": [0, 1, 2], "decode_direct_max": [0, 1, 256]}[name])
        return [{"op": "option", "name": name, "value": int(value)}]

    def make_stream(self):
        return [{"op": "stream", "stream": 1 - self.m.ctx.stream}]

    def _window(self, shape=None):
        """(shape, col0, width): the whole block, one word, a narrow window with odd col0 and odd width, a window that ends at S"""
        S, rng = self.m.S, self.rng
        shape = shape or self._pick(WINDOWS)
        if shape == "whole":
            return shape, 0, S
        if shape == "word":
            return shape, int(rng.integers(S)), 1
        if shape == "narrow":
            col0 = 1 + 2 * int(rng.integers((S - 3) // 2))
            return shape, col0, 1 + 2 * int(rng.integers(1, min(6, (S - col0 - 1) // 2 + 1)))
        width = int(rng.integers(2, S // 2 + 1))
        return shape, S - width, width

    def _read_prereq(self):
        """what makes the pool's own patterns the ones in force for a read ([] when they are): on fixed placement a pattern of the direct path"""
        m = self.m
        if m.rotated:
            return [self._state_prepare_set()] if m.ctx.prepared_set != m.needed_set() else []
        need, pre = m.needed_single(), []
        if len(need) > m.ctx.options["decode_direct_max"]:
            pre.append({"op": "option", "name": "decode_direct_max", "value": 256})
        if pre or m.ctx.prepared != need or len(need) > m.ctx.prepared_limit:
            pre.append(self._state_prepare())
        return pre

    def make_read(self, prefer=()):
        """1 to about 3k requests over the whole pool: present and lost blocks, duplicates, quarantined stripes, corrupted blocks, shuffled"""
        m, rng = self.m, self.rng
        if self.degraded:  # an absent block that a degraded write replaced, read before any rebuild: the new row must come back
            prefer = [w for w in (list(prefer) or self.absent_written[-4:]) if m.dev_of(w // m.k, w % m.k) in m.devs and not m.corrupt[w // m.k]]
        lost = [b * m.k + i for b in m.live() if not m.corrupt[b] for i in m.blocks_on(b, m.devs) if i < m.k]
        barred = {b * m.k + i for b in m.live() if m.corrupt[b] for i in m.blocks_on(b, m.devs) if i < m.k}
        special = [b * m.k + i for b in sorted(m.quarantined) for i in range(m.k)]
        special += [b * m.k + j for b in m.live() for j in m.corrupt[b] if j < m.k]
        n = int(rng.integers(1, 3 * m.k + 1)) if rng.random() < 0.5 else int(rng.integers(1, 9))
        reads = [int(x) for x in prefer][: max(1, n // 2)]
        if lost and n >= 3:  # the mix of one list: a lost block, a present one, a duplicate
            x = self._pick(lost)
            reads += [x, x]
        while len(reads) < n:
            u = rng.random()
            if u < 0.3 and lost:
                reads.append(self._pick(lost))
            elif u < 0.45 and special:
                reads.append(self._pick(special))
            elif u < 0.55 and reads:
                reads.append(self._pick(reads))
            else:
                x = int(rng.integers(m.count * m.k))
                if x not in barred:
                    reads.append(x)
        reads = [reads[i] for i in rng.permutation(len(reads))]
        shape, col0, width = self._window()
        op = {"op": "read", "set": m.rotated, "reads": reads, "col0": col0, "width": width, "shape": shape}
        if m.rotated:
            op["pattern_of"] = m.pattern_of(0, m.count, lambda b: b not in m.quarantined)
        return self._read_prereq() + [op]

    def _probe_read(self, use_set, lost, probe=None, q=0, variant=None):
        """a read of a scratch stripe under the single pattern or pattern q of the set: the blocks of `lost` (those the pattern in force then
        has lost, and whatever else the probe wants to see), some others, a duplicate"""
        m, rng = self.m, self.rng
        reads = [j for j in lost if j < m.k] + [int(x) for x in rng.integers(m.k, size=int(rng.integers(1, 4)))]
        reads.append(reads[0])
        reads = [int(reads[i]) for i in rng.permutation(len(reads))]
        shape, col0, width = self._window()
        op = {"op": "probe_read", "set": use_set, "q": q, "b": self._pick(m.live()), "reads": reads, "col0": col0, "width": width, "shape": shape,
              "dseed": self._ds(), "probe": probe}
        if variant:
            op["variant"] = variant
        return op

    def _mid_read(self):
        """[a state operation, a scratch read]: the read whose effect on other state a probe looks for, in either form"""
        m = self.m
        if self.rng.random() < 0.5:
            lost = self._probe_lost()
            pre = [] if m.ctx.options["decode_direct_max"] >= len(lost) else [{"op": "option", "name": "decode_direct_max", "value": 256}]
            return pre + [self._state_prepare(lost), self._probe_read(False, lost)]
        sp = self._state_prepare_set()
        q = int(self.rng.integers(len(sp["patterns"])))
        return [sp, self._probe_read(True, sp["patterns"][q], q=q)]

    def make_probe_read(self, x):
        """read_after_prepare (plain: B loses as many data blocks as A and differs in one; "transform": A on the transform path, its read
        refused; "parity": B loses parity only) and read_after_prepare_set"""
        m, rng = self.m, self.rng
        if x == "prepare_set":
            halves = []
            for _ in range(2):
                patterns = [self._random_pattern(4) for _ in range(3)]
                q = int(rng.integers(3))
                r = self._probe_read(True, patterns[q] + (halves[0]["patterns"][halves[0]["q"]] if halves else []), q=q)
                halves.append({"patterns": patterns, "q": q, "reads": r["reads"], "col0": r["col0"], "width": r["width"], "shape": r["shape"]})
            return [{"op": "probe_read_swap", "halves": halves, "b": self._pick(m.live()), "dseed": self._ds(), "probe": "read_after_prepare_set"}]
        # A: r lost data blocks (more than 16 where the code allows: the single form serves up to 256, a set 16 per pattern) and some parity
        r = int(rng.integers(17, 21)) if m.m >= 40 and x == "prepare" else int(rng.integers(1, min(m.m, m.k - 1, 6) + 1))
        a_data = sorted(int(i) for i in rng.choice(m.k, size=r, replace=False))
        a_par = sorted(m.k + int(i) for i in rng.choice(m.m, size=int(rng.integers(0, min(m.m - r, 2) + 1)), replace=False))
        if x == "prepare_parity":
            b_lost = sorted(m.k + int(i) for i in rng.choice(m.m, size=int(rng.integers(1, min(m.m, 3) + 1)), replace=False))
        else:
            b_data = list(a_data)
            b_data[int(rng.integers(r))] = self._pick([i for i in range(m.k) if i not in a_data])
            b_lost = sorted(b_data) + a_par
        a_lost = a_data + a_par
        ops = []
        limit = m.ctx.options["decode_direct_max"]
        if x == "prepare_transform":
            ops.append({"op": "option", "name": "decode_direct_max", "value": 0})
        elif limit < max(len(a_lost), len(b_lost)):
            ops.append({"op": "option", "name": "decode_direct_max", "value": 256})
        ops += [self._state_prepare(a_lost), self._probe_read(False, a_lost)]
        if x == "prepare_transform":
            ops.append({"op": "option", "name": "decode_direct_max", "value": 256})
        ops += [self._state_prepare(b_lost), self._probe_read(False, b_lost + a_lost, "read_after_prepare", variant=x[8:] or "plain")]
        return ops

    def make_burst(self):
        """2 to 4 enqueued calls back to back (writes of every form, at most one rebuild), each on the null or the side stream"""
        m, rng = self.m, self.rng
        if self.degraded:
            return self._make_degraded_burst()
        ops = []
        for _ in range(int(rng.integers(2, 5))):
            w = self.make_write(in_burst=True) if self.extended else self.make_write()
            if w:
                ops += w
        if self._rebuild_prereq() is None and rng.random() < 0.6:
            r = self._make_rebuild(self._pick(["repair", "decode"]))
            if r:
                ops.insert(int(rng.integers(len(ops) + 1)), r[-1])
        pre = []
        if self.extended and ops and (rng.random() < 0.7 or not self.used_form["burst_read"]):
            self.used_form["burst_read"] += 1
            pre = self._read_prereq()  # (the pool's own patterns, made the ones in force before the burst)
            # a read behind one of the calls, asking for blocks that the write before it has just replaced
            at = int(rng.integers(1, len(ops) + 1))
            before = [x for x in ops[:at] if x["op"] == "write"]
            ops.insert(at, self.make_read(prefer=writes_of(before[-1], m.k) if before else ())[-1])
        if len(ops) < 2:
            return None
        for sub in ops:
            sub["stream"] = int(rng.integers(2))
        if self.extended and len({sub["stream"] for sub in ops}) == 1:  # a read of a burst runs beside a call on the other stream
            for sub in ops:
                if sub["op"] == "read":
                    sub["stream"] = 1 - sub["stream"]
        return pre + [{"op": "burst", "ops": ops}]

    def _probe_lost(self):
        return self._random_pattern(20)

    def _probe_repair(self, probe):
        return {"op": "probe_repair", "b": self._pick(self.m.live()), "form": self._pick(["decode", "repair", "decode_batch", "repair_batch"]),
                "dseed": self._ds(), "probe": probe}

    def make_probe_prepared(self, x):
        m = self.m
        if x == "prepare_set":
            mid = [self._state_prepare_set()]
        elif x == "scrub_pattern":
            mid = [self._state_scrub()]
        elif x == "scrub_pattern_set":
            mid = [self._state_scrub_set()]
        elif x == "write":
            mid = self.make_write()
            if mid is None:
                return None
            mid[0]["form"] = "batch"
        elif x == "degraded_write":  # a degraded write into a scratch stripe, under a set of its own
            mid = self._scratch_set_write()
        elif x == "read":  # a scratch read under the probe's own pattern, or one under the set
            lost = self._probe_lost()
            if self.rng.random() < 0.5:
                mid = [self._probe_read(False, lost)]
                if m.ctx.options["decode_direct_max"] < len(lost):
                    mid.insert(0, {"op": "option", "name": "decode_direct_max", "value": 256})
            else:
                sp = self._state_prepare_set()
                q = int(self.rng.integers(len(sp["patterns"])))
                mid = [sp, self._probe_read(True, sp["patterns"][q], q=q)]
            return mid[:-1] + [self._state_prepare(lost)] + mid[-1:] + [self._probe_repair("prepared_after_read")]
        else:
            mid = self.make_verify() if x == "verify" else self.make_locate()
        pre, mid = mid[:-1], mid[-1:]
        return pre + [self._state_prepare(self._probe_lost())] + mid + [self._probe_repair("prepared_after_" + x)]

    def make_probe_set(self, y):
        m = self.m
        ops = []
        if y == "degraded_write":  # a set of its own, a scratch write under one of its patterns, a scratch repair under another
            ops = self._scratch_set_write()
            patterns = ops[0]["patterns"]
        elif m.ctx.prepared_set is None or (m.rotated and m.ctx.prepared_set != m.needed_set()):
            ops.append(self._state_prepare_set())
            patterns = ops[0]["patterns"]
        else:
            patterns = m.ctx.prepared_set
        if y == "degraded_write":
            pass
        elif y == "prepare":
            ops.append(self._state_prepare(self._probe_lost()))
        elif y in ("single", "batch"):
            ops.append(self._state_prepare(self._probe_lost()))
            pr = self._probe_repair(None)
            pr["form"] = self._pick(["decode", "repair"]) + ("_batch" if y == "batch" else "")
            ops.append(pr)
        elif y == "read":  # a scratch read under a single pattern of its own, or one under the set itself
            if self.rng.random() < 0.5:
                lost = self._probe_lost()
                if m.ctx.options["decode_direct_max"] < len(lost):
                    ops.append({"op": "option", "name": "decode_direct_max", "value": 256})
                ops += [self._state_prepare(lost), self._probe_read(False, lost)]
            else:
                q = int(self.rng.integers(len(patterns)))
                ops.append(self._probe_read(True, list(patterns[q]), q=q))
        else:
            ops = self.make_correct()[:-1] + ops + self.make_correct()[-1:]
        q = int(self.rng.integers(len(patterns)))
        ops.append({"op": "probe_repair_set", "q": q, "b": self._pick(m.live()), "form": self._pick(["decode", "repair"]),
                    "kernel": int(self.rng.integers(3)), "dseed": self._ds(), "probe": "set_after_" + y})
        return ops

    def make_probe_scrub(self, z):
        m = self.m
        ops = []
        pre = self._scrub_prereq()
        if pre:
            ops.append(pre)
        scrub = tuple(pre["absent"]) if pre and pre["op"] == "scrub_pattern" else m.ctx.scrub
        if z == "prepare":
            ops.append(self._state_prepare(self._probe_lost()))
        elif z == "single":
            ops.append(self._state_prepare(self._probe_lost()))
            pr = self._probe_repair(None)
            pr["form"] = self._pick(["decode", "repair"])
            ops.append(pr)
        elif z == "read":
            ops += self._mid_read()
        elif z == "degraded_write":
            ops += self._scratch_set_write()
        else:
            ops.append(self.make_correct()[-1])
        j = self._pick([j for j in range(m.n) if j not in scrub])
        ops.append({"op": "probe_verify", "b": self._pick(m.live()), "j": j, "seed": int(self.rng.integers(1 << 40)), "dseed": self._ds(),
                    "probe": "scrub_after_" + z})
        return ops

    def make_probe_refused(self, which):
        if which == "bad_degraded_write":
            return self._refused_degraded_write(which)
        if which == "bad_read":  # among valid requests an index count*k; for a requested stripe a pattern_of entry equal to the number of patterns
            m = self.m
            reads = [int(x) for x in self.rng.integers(m.count * m.k, size=int(self.rng.integers(2, 6)))]
            shape, col0, width = self._window()
            return [{"op": "refused", "which": which, "entry": len(m.ctx.prepared_set or ()), "reads": reads, "at": int(self.rng.integers(len(reads))),
                     "col0": col0, "width": width, "shape": shape, "probe": "refused_" + which}]
        return [{"op": "refused", "which": which, "entry": len(self.m.ctx.prepared_set or ()), "probe": "refused_" + which}]

    def next_op(self):
        self.emitted += 1
        if self.degraded and self.emitted == 1 and self.seed == DEG_SEEDS[0]:  # refused_no_set: no later step meets a context without a set
            return self._refused_degraded_write("no_set")[0]
        if self.queue:
            return self.queue.popleft()
        if self.probes_started < PROBES_PER_SEQUENCE and self.emitted > 2 + 7 * self.probes_started:
            ops = self._next_probe()
            if ops:
                self.queue.extend(ops)
                return self.queue.popleft()
        for _ in range(64):
            kind = self._draw_kind()
            self.drawn += 1
            ops = getattr(self, "make_" + kind)()
            if ops is None:
                self.skipped += 1
                continue
            self.used[kind] += 1
            self.queue.extend(ops)
            return self.queue.popleft()
        raise ModelError("no legal operation")


# ---- the driver ----
class SequenceFailure(AssertionError):
    def __init__(self, cfg, seed, step, what, log, extended=False, degraded=False):
        self.cfg, self.seed, self.step, self.what, self.log = cfg, seed, step, what, log
        flag = ", degraded=True" if degraded else ", extended=True" if extended else ""
        super().__init__("config %s seed %d step %d: %s\nreplay: run_sequence(backend, config_named(%r), %d, steps=%d%s)\noperations:\n%s"
                         % (cfg.name, seed, step, what, cfg.name, seed, step + 1, flag, "\n".join(log)))


def _same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    return a == b


def run_sequence(backend, cfg, seed, steps=None, oracle=None, on_step=None, extended=False, log=None, degraded=False):
    """Apply the sequence of (cfg, seed) to a fresh model and to `backend`; after every step compare every host output and the whole pool.
    Returns the model's Coverage.  Raises SequenceFailure (config, seed, step, the operation log) at the first difference.  `extended`: the
    generator draws the extended kinds as well (the seeds EXT_SEEDS; off, a sequence is what it always was).  `degraded`: degraded and column-window
    writes as well (the seeds DEG_SEEDS; it implies the extended kinds).  `log`: a list that receives the
    operation log, one JSON line per step."""
    if oracle is None:
        from oracle import Oracle
        oracle = Oracle()
    model = PoolModel(cfg, seed, oracle)
    gen = Generator(model, seed, extended, degraded)
    cov = Coverage(model)
    backend.start(model.mirror_d, model.mirror_p, sorted(model.quarantined))
    log = [] if log is None else log
    for step in range(cfg.steps if steps is None else steps):
        op = gen.next_op()
        log.append("%3d %s" % (step, json.dumps(op, separators=(",", ":"))))
        pay = model.payload(op)
        before = model.ctx.snapshot() if op["op"] == "refused" else None
        cov.before(op)
        want = model.apply(op, pay)
        if before is not None and before != model.ctx.snapshot():
            raise ModelError("a refused call changed the model's state")
        backend.step = step
        got = backend.run(op, pay)
        for key in want:
            if key not in got or not _same(want[key], got[key]):
                raise SequenceFailure(cfg, seed, step, "output %r is %r, the model says %r" % (key, got.get(key), want[key]), log, extended, degraded)
        d, p = backend.read_pool()
        if not np.array_equal(d, model.mirror_d) or not np.array_equal(p, model.mirror_p):
            bad = sorted({int(b) for b in np.nonzero((d != model.mirror_d).any(axis=(1, 2)) | (p != model.mirror_p).any(axis=(1, 2)))[0]})
            blocks = [j for j in range(model.n) if not np.array_equal(model.block(d, p, bad[0], j), model.block(model.mirror_d, model.mirror_p, bad[0], j))]
            raise SequenceFailure(cfg, seed, step, "the pool differs from the model in stripes %s (quarantined: %s); stripe %d blocks %s"
                                  % (bad, sorted(model.quarantined), bad[0], blocks), log, extended, degraded)
        cov.after(op)
        if on_step:
            on_step(step, op)
    cov.drawn, cov.skipped = gen.drawn, gen.skipped
    return cov


class Coverage:
    """What a sequence exercised (counted on the model, so it is the same on every backend)."""

    def __init__(self, model):
        self.m = model
        self.kinds = collections.Counter()
        self.variants = collections.Counter()
        self.probes = collections.Counter()
        self.drawn = self.skipped = 0
        self.prev = None            # the kind of the step before
        self.written_absent = set()  # absent data blocks that a degraded write replaced and no rebuild has visited since

    def _rebuilt(self, op):
        """the absent data blocks whose old rows a write rebuilds (fastecc_update_batch_set alone: the parity form is handed its old rows)"""
        m = self.m
        if op["op"] != "write" or op["form"] != "batch_set":
            return []
        return [w for w in op["writes"] if w % m.k in m.lost_for_write(w // m.k, "batch_set")]

    def _degraded_write(self, op, v):
        """the variants of a write of the four pool forms (against the model as the call, or its burst, meets it)"""
        m, form = self.m, op["form"]
        v["write_%s_%s" % (form, "window" if "width" in op else "whole_block")] += 1
        if "width" in op:
            v["write_window_" + op["shape"]] += 1
            if self.prev == "prepare_set" and form not in SET_FORMS:
                v["window_after_prepare_set"] += 1
        touched = sorted({w // m.k for w in op["writes"]})
        if any(m.corrupt[b] for b in touched) and "width" in op:
            v["window_beside_corruption"] += 1
        if form not in SET_FORMS:
            return
        if PATTERN_NONE in op["pattern_of"]:
            v["write_pattern_none"] += 1
        absent = [w for w in op["writes"] if w % m.k in m.lost_for_write(w // m.k, form)]
        if absent:
            v["write_absent_data"] += 1
            self.written_absent |= set(absent)
        if any(w not in absent and m.lost_for_write(w // m.k, form) for w in op["writes"]):
            v["write_present_of_degraded"] += 1
        if absent and len(absent) < len(op["writes"]):
            v["write_mixed_list"] += 1
        if any(m.lost_for_write(b, form) and min(m.lost_for_write(b, form)) >= m.k for b in touched):
            v["write_parity_only_stripe"] += 1
        if self._rebuilt(op):
            v["write_rebuilt_rows"] += 1
            if max(collections.Counter(w // m.k for w in op["writes"]).values()) > 16:
                v["segment_over_16_rebuilt"] += 1

    def before(self, op):
        m, kind = self.m, op["op"]
        self.kinds[kind] += 1
        if kind == "burst":
            self.prev = "burst"  # (no call of a burst counts as the step after the operation before the burst)
            for sub in op["ops"]:
                self.before(sub)
            for x, y in zip(op["ops"], op["ops"][1:]):  # neighbours on different streams: a read beside a rebuilding write, two rebuilding writes
                if x["stream"] != y["stream"]:
                    if x["op"] == "read" and self._rebuilt(y):
                        self.variants["burst_read_then_rebuilding_write"] += 1
                    if self._rebuilt(x) and y["op"] == "read":
                        self.variants["burst_rebuilding_write_then_read"] += 1
                    if self._rebuilt(x) and self._rebuilt(y) and x.get("width", m.S) != y.get("width", m.S):
                        self.variants["burst_rebuilding_writes_two_widths"] += 1
            if len({sub["stream"] for sub in op["ops"]}) > 1:
                self.variants["burst_two_streams"] += 1
                if any(sub["op"] == "read" for sub in op["ops"]):
                    self.variants["read_in_two_stream_burst"] += 1
            if any(sub["op"] == "read" and sub["stream"] == 1 for sub in op["ops"]):
                self.variants["read_side_stream"] += 1
            return
        v = self.variants
        if kind in ("read", "probe_read"):
            self._read(op, v)
        if kind == "probe_read_swap":
            v["read_side_stream"] += 1
            for half in op["halves"]:
                v["window_" + half["shape"]] += 1
        if kind == "refused" and op["which"] == "bad_read":
            v["window_" + op["shape"]] += 1
        if kind == "locate" and op.get("set"):
            self.kinds["locate_set"] += 1
            v["locate_set"] += 1
        if kind in ("write", "reencode") and op["form"] == "pool":
            self.kinds[kind + "_pool"] += 1
            v["%s_pool_kernel_%d" % (kind, m.ctx.options["encode_pool_kernel"])] += 1
            if kind == "write" and (op["b0"], op["b1"]) != (0, m.count):
                v["write_pool_subrange"] += 1
        if "b0" in op and (op["b0"], op["b1"]) != (0, m.count) and kind != "reencode":
            self.kinds["subrange"] += 1
            v["subrange"] += 1
        if kind in ("verify", "locate", "correct", "repair", "decode"):
            v["set" if op.get("set") else "single"] += 1
        if kind in ("verify", "locate", "correct") and not m.mixed:
            for b in range(op["b0"], op["b1"]):
                if b not in m.quarantined and not m.budget(b):
                    raise ModelError("budget")
            chunk = m.ctx.options["scrub_batch_chunk"]
            if chunk and op["b1"] - op["b0"] > chunk:
                v["multi_chunk"] += 1
        if kind == "correct":
            v["correct_mode_%d" % op["mode"]] += 1
        if kind in ("repair", "decode"):
            v["kernel_%d" % op["kernel"]] += 1
        if kind == "write" and op["form"] in WINDOW_FORMS:
            self._degraded_write(op, v)
        if kind in ("repair", "decode", "correct") or (kind == "write" and op["form"] == "pool"):
            self.written_absent.clear()
        if kind == "read" and any(w in self.written_absent and m.dev_of(w // m.k, w % m.k) in m.devs for w in op["reads"]):
            v["read_of_written_absent_block"] += 1
        if kind in ("probe_write", "probe_write_swap"):  # scratch writes: counted apart from the pool's
            for half in (op["halves"] if kind == "probe_write_swap" else [op]):
                v["probe_write_" + ("whole_block" if half["shape"] == "whole_block" else "window")] += 1
                if kind == "probe_write" and not op.get("after"):
                    v["state_probe_write_" + ("whole_block" if half["shape"] == "whole_block" else "window")] += 1
            if kind == "probe_write_swap":
                v["side_stream_scratch_write"] += 1
        if kind == "write":
            v["write_" + op["form"]] += 1
            per = collections.Counter(w // m.k for w in writes_of(op, m.k))
            if op["form"] not in ("single", "pool") and max(per.values()) > 16:
                v["segment_over_16"] += 1
        if kind == "corrupt" and len(op["blocks"]) + len(m.devs) > 16:
            v["over_16_lost"] += 1
        if m.ctx.stream == 1 and kind not in ("stream", "option", "device_replaced", "corrupt", "device_down"):
            v["side_stream"] += 1

    def _read(self, op, v):
        """the variants of one read (a pool read or a probe's scratch read), against the patterns in force as the call meets them"""
        m = self.m
        if not op["set"]:
            m._prepared()
        if m.ctx.stream == 1:
            v["read_side_stream"] += 1
        v["read_set" if op["set"] else "read_single"] += 1
        v["window_" + op["shape"]] += 1
        if op["op"] == "probe_read":
            lost = m.ctx.prepared_set[op["q"]] if op["set"] else m.ctx.prepared
            kinds = {"lost" if i in lost else "present" for i in op["reads"]}
            patterns = [lost]
        else:
            stripes = sorted({idx // m.k for idx in op["reads"]})
            if any(b in m.quarantined for b in stripes):
                v["read_pattern_none"] += 1
            kinds = {"lost" if b not in m.quarantined and m.dev_of(b, i) in m.devs else "present" for b, i in (divmod(idx, m.k) for idx in op["reads"])}
            patterns = [m.blocks_on(b, m.devs) for b in stripes if b not in m.quarantined] if op["set"] else [m.ctx.prepared]
        if kinds == {"lost", "present"} and len(set(op["reads"])) < len(op["reads"]):
            v["read_mixed_list"] += 1
        if any(q and min(q) >= m.k for q in patterns):
            v["read_parity_only"] += 1
        if not op["set"] and len(m.ctx.prepared) > 16 and len(m.ctx.prepared) <= m.ctx.prepared_limit:
            v["read_single_over_16_lost"] += 1
        if op.get("probe") == "read_after_prepare":
            v["read_after_prepare_" + op["variant"]] += 1

    def after(self, op):
        if op.get("probe"):
            self.probes[op["probe"]] += 1
            if op["op"] == "refused" and op.get("variant"):  # (the model has checked that the variant's argument is the only thing wrong)
                self.variants["refused_" + op["variant"]] += 1
                for entry in op["entries"]:
                    self.variants["refused_%s_%s" % (op["variant"], entry)] += 1
        self.prev = op["op"]

    def merge(self, other):
        self.kinds.update(other.kinds)
        self.variants.update(other.variants)
        self.probes.update(other.probes)
        return self


# ---- backends: one method per operation, returning the host outputs, plus read_pool ----
class ModelBackend:
    """The interface in numpy from the definitions: repair is the truth, update is a re-encode.  It keeps its own pool, its own truth and its
    own context state, so that the harness can be tested (and defects injected) without a GPU."""

    def __init__(self, cfg, oracle):
        self.cfg, self.n, self.k, self.m, self.S, self.count = cfg, cfg.n, cfg.k, cfg.n - cfg.k, cfg.S, cfg.count
        self.mixed = bool(cfg.flags & MIXED_RADIX)
        self.codec = Codec(oracle, cfg.n, cfg.k, cfg.flags, cfg.order)
        self.step = 0

    def start(self, d, p, quarantined):
        self.d, self.p = d.copy(), p.copy()
        self.td, self.tp = d.copy(), p.copy()
        self.prepared, self.prepared_set, self.scrub, self.scrub_set = None, None, (), None
        self.prepared_limit = 256
        self.options = {}

    def read_pool(self):
        return self.d.copy(), self.p.copy()

    def run(self, op, pay):
        return getattr(self, "op_" + op["op"])(op, pay) or {"code": OK}

    def blk(self, d, p, b, j):
        return d[b, j] if j < self.k else p[b, j - self.k]

    def _poke(self, pay):
        for b, j, row in pay["pokes"]:
            self.blk(self.d, self.p, b, j)[:] = row

    def op_corrupt(self, op, pay):
        self._poke(pay)

    def op_device_down(self, op, pay):
        self._poke(pay)

    def op_device_replaced(self, op, pay):
        pass

    def op_write(self, op, pay):
        """fastecc_update_batch, fastecc_update on one stripe, or fastecc_update_parity_batch + the caller's own store of the data blocks"""
        writes = writes_of(op, self.k)  # (form "pool": the harness stores every data block of the run, fastecc_encode_pool encodes it)
        if op["form"] in SET_FORMS or "width" in op:
            def lost_of(b):
                q = op["pattern_of"][b] if op["form"] in SET_FORMS else PATTERN_NONE
                return () if q == PATTERN_NONE else self.prepared_set[q]
            return self.write_rows(self.d, self.p, self.td, self.tp, [divmod(w, self.k) for w in writes], pay["new"], lost_of, op["form"],
                                   op.get("col0", 0), op.get("width", self.S))
        for u, w in enumerate(writes):
            self.d[w // self.k, w % self.k] = pay["new"][u]
        touched = sorted({w // self.k for w in writes})
        encoded = self.encoded_stripes(op, touched)
        for b in touched:
            self.td[b], self.tp[b] = self.d[b], self.codec.parity(self.d[b])
            if b in encoded:
                self.p[b] = self.tp[b]

    def encoded_stripes(self, op, stripes):
        return stripes

    # -- degraded and window writes, from the definition: the truth takes the rows, the parity is the oracle's re-encode of the truth, the present
    # blocks take both in the window's columns.  The library updates the parity from the CHANGE of each written block, so an old row it gets wrong
    # shows in the parity as the re-encode of a stripe that is off by that much: write_rows keeps this form, so that defects in the old rows can be
    # injected (the exact backend's old rows are the truth, and the term is zero).
    def write_rows(self, d, p, td, tp, writes, new, lost_of, form, col0, width):
        """d, p: a pool (stripes, k or n - k, S) and td, tp its truth; writes: (stripe, block) pairs, row u of `new` for writes[u]"""
        win = slice(col0, col0 + width)
        rebuilt = [u for u, (b, i) in enumerate(writes) if form == "batch_set" and i in lost_of(b)]
        recon = dict(zip(rebuilt, self.rebuilt_rows(d, td, [writes[u] for u in rebuilt], col0, width)))
        off = {}
        for u, (b, i) in enumerate(writes):
            absent = i in lost_of(b)
            if u in recon and not np.array_equal(recon[u], td[b, i, win]):  # (what the parity will be wrong by)
                off[b, i] = (td[b, i, win].astype(np.int64) - recon[u].astype(np.int64) % P) % P
            td[b, i, win] = new[u]
            if self.stores_data(form, absent):  # (the parity forms: the harness, as the caller, stores the window into present data blocks)
                self.store_data(d, b, i, col0, width, new[u], form)
        for b in sorted({b for b, _ in writes}):
            tp[b] = self.codec.parity(td[b])
            rows = tp[b]
            if any(x == b for x, _ in off):
                x = td[b].copy()
                for (bb, i), e in off.items():
                    if bb == b:
                        x[i, win] = ((x[i, win].astype(np.int64) + e) % P).astype(np.uint32)
                rows = self.codec.parity(x)
            self.store_parity(p, b, rows, [q - self.k for q in lost_of(b) if q >= self.k], col0, width)

    def rebuilt_rows(self, d, td, blocks, col0, width):
        """the old rows of the absent written blocks, as a rebuild from the survivors gives them"""
        return [td[b, i, col0:col0 + width].copy() for b, i in blocks]

    def stores_data(self, form, absent):
        return not absent

    def store_data(self, d, b, i, col0, width, row, form):
        d[b, i, col0:col0 + width] = row

    def store_parity(self, p, b, rows, lost, col0, width):
        for q in range(self.m):
            if q not in lost:
                p[b, q, col0:col0 + width] = rows[q, col0:col0 + width]

    def _scratch_write(self, half, pay_d, pay_p, new, src, lost):
        """one degraded write into a scratch stripe whose truth is stripe src's: (d, p, its new truth)"""
        d, p, td, tp = pay_d.copy()[None], pay_p.copy()[None], self.td[src].copy()[None], self.tp[src].copy()[None]
        self.write_rows(d, p, td, tp, [(0, i) for i in half["writes"]], new, lambda b: lost, half["form"], half["col0"], half["width"])
        return d[0], p[0], td[0], tp[0]

    def op_probe_write(self, op, pay):
        lost = self.prepared_set[op["q"]]
        d, p, td, tp = self._scratch_write(op, pay["scratch_d"], pay["scratch_p"], pay["new"], pay["src"], lost)
        out = {"code": OK}
        if op.get("after") == "repair":
            for j in lost:
                (d if j < self.k else p)[j if j < self.k else j - self.k] = (td if j < self.k else tp)[j if j < self.k else j - self.k]
            out["codes"] = [OK, OK]
        if op.get("after") == "read":
            rows = self.read_rows(d[None], td[None], [(0, i) for i in op["reads"]], lambda b: lost, op["col0"], op["width"])
            out.update(codes=[OK, OK], rows=rows[:-1], guard=rows[-1])
        return dict(out, scratch_d=d, scratch_p=p)

    def op_probe_write_swap(self, op, pay):
        ds, ps = [], []
        for half, (d, p), new in zip(op["halves"], pay["scratch"], pay["new"]):
            self.prepared_set = tuple(tuple(q) for q in half["patterns"])
            d, p, _, _ = self._scratch_write(half, d, p, new, pay["src"], self.swap_pattern(op, half))
            ds.append(d)
            ps.append(p)
        return {"code": OK, "codes": [OK] * 4, "scratch_d": np.stack(ds), "scratch_p": np.stack(ps)}

    def swap_pattern(self, op, half):
        return self.prepared_set[half["q"]]

    def op_prepare(self, op, pay):
        self.prepared = tuple(op["lost"])
        self.prepared_limit = self.options.get("decode_direct_max", 256)

    def op_prepare_set(self, op, pay):
        self.prepared_set = tuple(tuple(q) for q in op["patterns"])

    def op_scrub_pattern(self, op, pay):
        if self.mixed:
            return {"code": E_UNSUPPORTED}
        self.scrub = tuple(op["absent"])

    def op_scrub_pattern_set(self, op, pay):
        if self.mixed:
            return {"code": E_UNSUPPORTED}
        self.scrub_set = tuple(tuple(q) for q in op["patterns"])

    def _wrong(self, b, absent):
        return [j for j in range(self.n) if j not in absent and not np.array_equal(self.blk(self.d, self.p, b, j), self.blk(self.td, self.tp, b, j))]

    def _absent_of(self, op, b):
        """the absent blocks a scrub call applies to stripe b, or None for FASTECC_PATTERN_NONE"""
        if not op.get("set"):
            return self.scrub
        q = op["pattern_of"][b - op["b0"]]
        return None if q == PATTERN_NONE else self.scrub_set[q]

    def _verify_one(self, b, absent):
        return 0 if self._wrong(b, absent) else 1

    def op_verify(self, op, pay):
        if self.mixed:
            return {"code": E_UNSUPPORTED}
        ok = []
        for b in range(op["b0"], op["b1"]):
            absent = self._absent_of(op, b)
            ok.append(1 if absent is None else self._verify_one(b, absent))
        out = {"code": OK, "consistent": ok, "inconsistent": ok.count(0)}
        if op.get("single") is not None:
            out["single"] = self._verify_one(op["single"], self.scrub)
        return out

    def op_locate(self, op, pay):
        if self.mixed:
            return {"code": E_UNSUPPORTED}
        absent = [self._absent_of(op, b) for b in range(op["b0"], op["b1"])]
        lists = [[] if a is None else self._wrong(b, a) for b, a in zip(range(op["b0"], op["b1"]), absent)]
        status = [1 if x else 0 for x in lists]
        return {"code": OK, "status": status, "lists": lists, "inconsistent": sum(status)}

    def op_correct(self, op, pay):
        if self.mixed:
            return {"code": E_UNSUPPORTED}
        status = []
        for b in range(op["b0"], op["b1"]):
            absent = self._absent_of(op, b)
            bad = [] if absent is None else self._wrong(b, absent)
            status.append(1 if bad else 0)
            if bad:
                self.d[b], self.p[b] = self.td[b], self.tp[b]
                self.prepared = tuple(sorted(set(bad) | set(absent)))
        return {"code": OK, "status": status, "inconsistent": sum(status)}

    def _lost_of(self, op, b):
        if not op["set"]:
            return self.prepared
        q = op["pattern_of"][b - op["b0"]]
        return () if q == PATTERN_NONE else self.prepared_set[q]

    def _rebuild(self, op, data_only):
        for b in range(op["b0"], op["b1"]):
            for j in self._lost_of(op, b):
                if not (data_only and j >= self.k):
                    self.blk(self.d, self.p, b, j)[:] = self.blk(self.td, self.tp, b, j)

    def op_repair(self, op, pay):
        self._rebuild(op, False)

    def op_decode(self, op, pay):
        self._rebuild(op, True)

    def op_reencode(self, op, pay):
        return {"code": OK, "parity": np.stack([self.codec.parity(self.d[b]) for b in range(op["b0"], op["b1"])])}

    def op_option(self, op, pay):
        self.options[op["name"]] = op["value"]

    def op_stream(self, op, pay):
        pass

    def op_burst(self, op, pay):
        outs = [self.run(sub, pz) for sub, pz in zip(op["ops"], pay["subs"])]
        out = {"code": OK, "codes": [o["code"] for o in outs]}
        reads = [o for sub, o in zip(op["ops"], outs) if sub["op"] == "read"]
        if reads:
            out["rows"] = np.concatenate([r["rows"].reshape(-1) for r in reads])
            out["guard"] = np.concatenate([r["guard"] for r in reads])
        return out

    # -- degraded reads: (n_reads + 1) rows of canary, row u the window of the requested block — as stored where the block is present under the
    # pattern in force, the truth where it is lost
    def single_pattern(self):
        return self.prepared

    def read_rows(self, d, td, reads, lost_of, col0, width):
        out = canary_rows(len(reads) + 1, width)
        for u, (b, i) in enumerate(reads):
            out[u] = (td if i in lost_of(b) else d)[b, i, col0:col0 + width]
        return out

    def read_out(self, code, out):
        return {"code": code, "rows": out[:-1], "guard": out[-1]}

    def op_read(self, op, pay):
        reads = [divmod(idx, self.k) for idx in op["reads"]]
        if op["set"]:
            def lost_of(b):
                return () if op["pattern_of"][b] == PATTERN_NONE else self.prepared_set[op["pattern_of"][b]]
        else:
            if len(self.prepared) > self.prepared_limit:
                return self.read_out(E_UNSUPPORTED, canary_rows(len(reads) + 1, op["width"]))
            lost = self.single_pattern()

            def lost_of(b):
                return lost
        return self.read_out(OK, self.read_rows(self.d, self.td, reads, lost_of, op["col0"], op["width"]))

    def _scratch_read(self, d, src, lost, half):
        """one read of a scratch stripe `d` whose truth is stripe src's"""
        return self.read_rows(d[None], self.td[src][None], [(0, i) for i in half["reads"]], lambda b: lost, half["col0"], half["width"])

    def op_probe_read(self, op, pay):
        if not op["set"] and len(self.prepared) > self.prepared_limit:
            return self.read_out(E_UNSUPPORTED, canary_rows(len(op["reads"]) + 1, op["width"]))
        lost = self.prepared_set[op["q"]] if op["set"] else self.single_pattern()
        return self.read_out(OK, self._scratch_read(pay["scratch_d"], pay["src"], lost, op))

    def op_probe_read_swap(self, op, pay):
        outs = []
        for half, (d, p) in zip(op["halves"], pay["scratch"]):
            self.prepared_set = tuple(tuple(q) for q in half["patterns"])
            outs.append(self._scratch_read(d, pay["src"], self.prepared_set[half["q"]], half))
        return {"code": OK, "codes": [OK] * 4, "rows": np.concatenate([o[:-1].reshape(-1) for o in outs]), "guard": np.concatenate([o[-1] for o in outs])}

    def _scratch_rebuild(self, pay, lost, repair):
        d, p = pay["scratch_d"].copy(), pay["scratch_p"].copy()
        for j in lost:
            if j < self.k:
                d[j] = self.td[pay["src"], j]
            elif repair:
                p[j - self.k] = self.tp[pay["src"], j - self.k]
        return {"code": OK, "scratch_d": d, "scratch_p": p}

    def op_probe_repair(self, op, pay):
        return self._scratch_rebuild(pay, self.prepared, op["form"].startswith("repair"))

    def op_probe_repair_set(self, op, pay):
        return self._scratch_rebuild(pay, self.prepared_set[op["q"]], op["form"] == "repair")

    def op_probe_verify(self, op, pay):
        ok = []
        for d, p in pay["scratch"]:
            ok.append(1 if all(np.array_equal(d[j] if j < self.k else p[j - self.k], self.blk(self.td, self.tp, pay["src"], j))
                               for j in range(self.n) if j not in self.scrub) else 0)
        return {"code": OK, "ok": ok}

    def op_refused(self, op, pay):
        if op["which"] == "bad_read":
            return {"code": E_INVAL, "codes": [E_INVAL, E_INVAL], "rows": canary_rows(2 * (len(op["reads"]) + 1), op["width"]).reshape(-1)}
        if op["which"] in ("bad_degraded_write", "no_set"):
            return {"code": E_INVAL, "codes": [E_INVAL] * len(op["entries"]), "rows": pay["new"].reshape(-1).copy()}
        return {"code": E_INVAL}


class GpuBackend:
    """One fastecc_amd.Encoder for the whole sequence.  `fe` is the package and `torch` is torch (handed in: this module imports neither).
    The pool, the scratch stripe and the new blocks live in device memory; harness work (uploads, pokes, read-back) runs on the null stream,
    library calls on the null stream or a side stream as the sequence says.  Before a call on another stream touches the pool the two streams
    are ordered with an event wait, as a caller must — never with a device-wide synchronise, so the library's own ordering of its buffers
    and of the staged write list stays exposed."""

    def __init__(self, fe, torch, cfg, profile=False):
        import ctypes
        self.ct, self.fe, self.torch, self.cfg = ctypes, fe, torch, cfg
        self.n, self.k, self.m, self.S, self.count = cfg.n, cfg.k, cfg.n - cfg.k, cfg.S, cfg.count
        self.dw, self.pw = self.k * self.S, self.m * self.S
        self.enc = fe.Encoder(cfg.n, cfg.k, 4 * cfg.S, flags=cfg.flags)
        self.side = torch.cuda.Stream(device="cuda:0")
        self.streams = [torch.cuda.default_stream(torch.device("cuda:0")), self.side]
        self.handles = [0, self.side.cuda_stream]
        self.last = self.cur = 0
        self.keep = []
        self.step = 0
        self.scopes = {} if profile else None
        if profile:
            self.enc.profile(True)

    def close(self):
        self.torch.cuda.synchronize()
        self.enc.close()

    # -- plumbing
    def _dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).reshape(-1)).to("cuda:0")

    def _host(self, t):
        return t.cpu().numpy().view(np.uint32).copy()

    def _order(self, to):
        if to != self.last:
            ev = self.torch.cuda.Event()
            ev.record(self.streams[self.last])
            self.streams[to].wait_event(ev)
            self.last = to

    def _lib(self):
        """ready for a library call on the sequence's current stream: its handle"""
        self._order(self.cur)
        return self.handles[self.cur]

    def _code(self, call, *args, **kw):
        try:
            call(*args, **kw)
        except self.fe.FastEccError as e:
            return e.code
        return OK

    def _pool(self, b0=0):
        return self.D[b0 * self.dw:], self.Q[b0 * self.pw:]

    def start(self, d, p, quarantined):
        torch = self.torch
        self.quarantined = set(quarantined)
        self.D = torch.empty(self.count * self.dw, dtype=torch.int32, device="cuda:0")
        self.Q = torch.empty(self.count * self.pw, dtype=torch.int32, device="cuda:0")
        self.D.copy_(self._dev(d))
        self.Q.copy_(self._dev(p))
        self.sd = torch.empty(self.count * self.dw, dtype=torch.int32, device="cuda:0")  # scratch: probes, re-encoded parity
        self.sq = torch.empty(self.count * self.pw, dtype=torch.int32, device="cuda:0")

    def read_pool(self):
        self._order(0)
        return self._host(self.D).reshape(self.count, self.k, self.S), self._host(self.Q).reshape(self.count, self.m, self.S)

    def run(self, op, pay):
        if self.scopes is not None:
            self.enc.profile_reset()
        out = getattr(self, "op_" + op["op"])(op, pay) or {"code": OK}
        if self.scopes is not None:
            self.scopes[self.step] = set(self.enc.profile_read())
        return out

    def _poke(self, pay):
        self._order(0)
        for b, j, row in pay["pokes"]:
            t = self.D[b * self.dw + j * self.S:][:self.S] if j < self.k else self.Q[b * self.pw + (j - self.k) * self.S:][:self.S]
            t.copy_(self._dev(row))

    def op_corrupt(self, op, pay):
        self._poke(pay)

    def op_device_down(self, op, pay):
        self._poke(pay)

    def op_device_replaced(self, op, pay):
        pass

    def _stage(self, op, pay):
        """the new (and old) blocks of a write in device memory, uploaded on the null stream before the call is enqueued"""
        self._order(0)
        staged = (self._dev(pay["new"]), self._dev(pay["old"]) if op["form"] in ("parity", "parity_set") else None)
        self.keep.append(staged)
        return staged

    def op_write(self, op, pay, staged=None):
        k = self.k
        new, old = staged or self._stage(op, pay)
        if op["form"] == "pool":  # the caller stores the run's data blocks itself, on the call's stream; fastecc_encode_pool writes their parity
            D, Q = self._pool(op["b0"])
            cnt, lib = op["b1"] - op["b0"], self._lib()
            with self.torch.cuda.stream(self.streams[self.cur]):
                D[:cnt * self.dw].copy_(new)
            return {"code": self._code(self.enc.encode_pool, D, Q, cnt, stream=lib)}
        writes = op["writes"]
        if op["form"] in SET_FORMS or "width" in op:
            po = None
            if op["form"] in SET_FORMS:
                po = np.array(op["pattern_of"], dtype=np.uint32)
                if op.get("ignored") is not None:
                    po[op["ignored"]] = op["entry"]  # the number of patterns in force, for a stripe that no write names
            return {"code": self._pool_write(op, self.D, self.Q, self.count, po, writes, new, old)}
        if op["form"] == "batch":
            return {"code": self._code(self.enc.update_batch, self.D, self.Q, self.count, writes, new, stream=self._lib())}
        if op["form"] == "single":
            b = writes[0] // k
            D, Q = self._pool(b)
            return {"code": self._code(self.enc.update, D, Q, [w % k for w in writes], new, stream=self._lib())}
        code = self._code(self.enc.update_parity_batch, self.Q, self.count, writes, new, old=old, stream=self._lib())
        with self.torch.cuda.stream(self.streams[self.cur]):  # the data blocks live with the caller: it stores them itself, on the same stream
            for u, w in enumerate(writes):
                self.D[w * self.S:][:self.S].copy_(new[u * self.S:][:self.S])
        return {"code": code}

    def _pool_write(self, op, D, Q, count, po, writes, new, old):
        """one of the four pool forms on the pool (D, Q) of `count` stripes, on the sequence's stream: the _set forms with pattern_of `po`, a
        window where the operation has one (col0 = 0, width = None is the whole-block entry point); rows compact at pitch width.  The parity
        forms store no data: the harness, as the caller, stores the window into the PRESENT data blocks itself, on the same stream."""
        kw = {"col0": op["col0"], "width": op["width"]} if "width" in op and op.get("shape") != "whole_block" else {}
        form, lib = op["form"], self._lib()
        if form == "batch":
            return self._code(self.enc.update_batch, D, Q, count, writes, new, stream=lib, **kw)
        if form == "batch_set":
            code = self._code(self.enc.update_batch_set, D, Q, count, po, writes, new, stream=lib, **kw)
            po[:] = 0xFFFFFFFE  # pattern_of may be reused as soon as the call returns
            return code
        lost = [()] * len(writes)
        if form == "parity":
            code = self._code(self.enc.update_parity_batch, Q, count, writes, new, old=old, stream=lib, **kw)
        else:
            lost = [() if po[w // self.k] == PATTERN_NONE else self.patterns[int(po[w // self.k])] for w in writes]
            code = self._code(self.enc.update_parity_batch_set, Q, count, po, writes, new, old=old, stream=lib, **kw)
            po[:] = 0xFFFFFFFE
        col0, W = op.get("col0", 0), op.get("width", self.S)
        with self.torch.cuda.stream(self.streams[self.cur]):
            for u, w in enumerate(writes):
                if w % self.k not in lost[u]:
                    D[w * self.S + col0:][:W].copy_(new[u * W:][:W])
        return code

    def _set_patterns(self, patterns):
        """fastecc_decode_prepare_set, and the patterns kept for the caller's own stores of the parity form"""
        code = self._code(self.enc.decode_prepare_set, *self._flag_rows(patterns))
        self.patterns = [tuple(q) for q in patterns]
        return code

    def op_probe_write(self, op, pay):
        """a degraded write into the scratch stripe under pattern q; then nothing, a repair under the same pattern on the same stream, or a read of
        the written blocks on the OTHER stream, ordered behind the write by an event only"""
        sd, sq = self._scratch(pay["scratch_d"], pay["scratch_p"])
        new, old = self._dev(pay["new"]), self._dev(pay["old"])
        out = self._read_buffer(len(op["reads"]), op["width"]) if op.get("after") == "read" else None
        self.keep.append((new, old))
        codes = [self._pool_write(op, sd, sq, 1, np.array([op["q"]], dtype=np.uint32), op["writes"], new, old)]
        got = {}
        if op.get("after") == "repair":
            codes.append(self._code(self.enc.repair_batch_set, sd, sq, 1, [op["q"]], stream=self._lib()))
        if op.get("after") == "read":
            cur, self.cur = self.cur, 1 - self.cur
            codes.append(self._read_call(op, sd, sq, 1, op["reads"], [op["q"]], out))
            self.cur = cur
            got = self._read_back(OK, out, len(op["reads"]), op["width"])
        res = dict(self._scratch_out(codes[0]), **{x: got[x] for x in ("rows", "guard") if x in got})
        if len(codes) > 1:
            res["codes"] = codes
        return res

    def op_probe_write_swap(self, op, pay):
        """the two scratch stripes and the rows first; then decode_prepare_set, a degraded write on the side stream, decode_prepare_set again with
        nothing synchronised here (the library waits for the write itself), a degraded write on the sequence's stream; read back at the end"""
        self._order(0)
        rows = []
        for s, (d, p) in enumerate(pay["scratch"]):
            self.sd[s * self.dw:][:self.dw].copy_(self._dev(d))
            self.sq[s * self.pw:][:self.pw].copy_(self._dev(p))
            rows.append((self._dev(pay["new"][s]), self._dev(pay["old"][s])))
        self.keep.append(rows)
        cur, codes = self.cur, []
        for s, (half, (new, old)) in enumerate(zip(op["halves"], rows)):
            codes.append(self._set_patterns(half["patterns"]))
            self.cur = 1 if s == 0 else cur
            codes.append(self._pool_write(half, self.sd[s * self.dw:], self.sq[s * self.pw:], 1, np.array([half["q"]], dtype=np.uint32), half["writes"], new, old))
        self.cur = cur
        self._order(0)
        return {"code": OK, "codes": codes, "scratch_d": self._host(self.sd[:2 * self.dw]).reshape(2, self.k, self.S),
                "scratch_p": self._host(self.sq[:2 * self.pw]).reshape(2, self.m, self.S)}

    def _refused_write(self, op, pay):
        """A degraded write that the library must refuse, through the C entry points (past what the Python methods let through): the codes and the
        caller's rows read back.  The operation is a valid write — its own pattern_of, legal stripes, a window inside the block, rows of S words
        outside the pool — and only the argument that the variant names is spoiled here; one call per entry point it lists."""
        ct, lib, h = self.ct, self.fe.lib(), self.enc._h
        n, variant = len(op["writes"]), op.get("variant")
        rows = self._dev(pay["new"])
        self.keep.append(rows)
        writes = (ct.c_uint64 * n)(*op["writes"])
        po = np.array(op["pattern_of"], dtype=np.uint32)
        if variant == "entry":
            po[op["writes"][0] // self.k] = op["entry"]  # the number of patterns in force, for a touched stripe
        pp = None if variant == "null_pattern_of" else po.ctypes.data_as(ct.POINTER(ct.c_uint32))
        st = self._lib() or None
        D, Q, codes = self.D.data_ptr(), self.Q.data_ptr(), []
        for entry in op["entries"]:
            whole = entry == "whole_block"
            new = rows.data_ptr()
            if variant == "overlap":  # the rows, as n_writes * width words (n_writes blocks for the whole-block call), are the end of the parity pool
                new = self.Q[self.count * self.pw - n * (self.S if whole else op["call_width"]):].data_ptr()
            window = () if whole else (op["call_col0"], op["call_width"])
            if op["form"] == "batch_set":
                call = lib.fastecc_update_batch_set if whole else lib.fastecc_update_batch_set_window
                codes.append(call(h, D, Q, self.count, pp, writes, n, *window, new, st))
            else:
                call = lib.fastecc_update_parity_batch_set if whole else lib.fastecc_update_parity_batch_set_window
                codes.append(call(h, Q, self.count, pp, writes, n, *window, None, new, st))
        self._order(0)
        return {"code": codes[0], "codes": codes, "rows": self._host(rows)}

    def op_burst(self, op, pay):
        """every block uploaded first, then the calls enqueued back to back, each on its stream, with event waits between streams and no
        synchronisation: the next call meets the previous one's list and buffers still in flight"""
        staged = [self._stage(sub, pz) if sub["op"] == "write" else self._read_buffer(len(sub["reads"]), sub["width"]) if sub["op"] == "read" else None
                  for sub, pz in zip(op["ops"], pay["subs"])]
        cur, codes, reads = self.cur, [], []
        for sub, pz, st in zip(op["ops"], pay["subs"], staged):
            self.cur = sub["stream"]
            if sub["op"] == "read":  # enqueued like the rest; its output is read back after the burst
                out = {"code": self._read_call(sub, self.D, self.Q, self.count, sub["reads"], sub.get("pattern_of"), st)}
                reads.append((st, len(sub["reads"]), sub["width"]))
            else:
                out = self.op_write(sub, pz, st) if sub["op"] == "write" else self.run_sub(sub, pz)
            codes.append(out["code"])
        self.cur = cur
        out = {"code": OK, "codes": codes}
        if reads:
            got = [self._read_back(OK, *r) for r in reads]
            out["rows"] = np.concatenate([g["rows"].reshape(-1) for g in got])
            out["guard"] = np.concatenate([g["guard"] for g in got])
        return out

    # -- degraded reads: the output is (n_reads + 1) rows preset to CANARY on the null stream; the call runs on the sequence's stream
    def _read_buffer(self, n, width):
        self._order(0)
        out = self._dev(canary_rows(n + 1, width))
        self.keep.append(out)
        return out

    def _read_call(self, op, D, Q, count, reads, pattern_of, out):
        """fastecc_read_batch_set (pattern_of given) or fastecc_read_batch: the code; nothing is read back here"""
        if pattern_of is not None:
            po = np.array(pattern_of, dtype=np.uint32)
            code = self._code(self.enc.read_batch_set, D, Q, count, po, reads, out, col0=op["col0"], width=op["width"], stream=self._lib())
            po[:] = 0xFFFFFFFE  # pattern_of may be reused as soon as the call returns
            return code
        return self._code(self.enc.read_batch, D, Q, count, reads, out, col0=op["col0"], width=op["width"], stream=self._lib())

    def _read_back(self, code, out, n, width):
        self._order(0)
        host = self._host(out).reshape(n + 1, width)
        return {"code": code, "rows": host[:n], "guard": host[n]}

    def op_read(self, op, pay):
        out = self._read_buffer(len(op["reads"]), op["width"])
        code = self._read_call(op, self.D, self.Q, self.count, op["reads"], op.get("pattern_of") if op["set"] else None, out)
        return self._read_back(code, out, len(op["reads"]), op["width"])

    def op_probe_read(self, op, pay):
        sd, sq = self._scratch(pay["scratch_d"], pay["scratch_p"])
        out = self._read_buffer(len(op["reads"]), op["width"])
        code = self._read_call(op, sd, sq, 1, op["reads"], [op["q"]] if op["set"] else None, out)
        return self._read_back(code, out, len(op["reads"]), op["width"])

    def op_probe_read_swap(self, op, pay):
        """the two scratch stripes and both outputs first; then decode_prepare_set, a read on the side stream, decode_prepare_set again with
        nothing synchronised here (the library waits for the read itself), a read on the sequence's stream; read back at the end"""
        self._order(0)
        for s, (d, p) in enumerate(pay["scratch"]):
            self.sd[s * self.dw:][:self.dw].copy_(self._dev(d))
            self.sq[s * self.pw:][:self.pw].copy_(self._dev(p))
        outs = [self._read_buffer(len(half["reads"]), half["width"]) for half in op["halves"]]
        cur, codes = self.cur, []
        for s, (half, out) in enumerate(zip(op["halves"], outs)):
            codes.append(self._set_patterns(half["patterns"]))
            self.cur = 1 if s == 0 else cur
            codes.append(self._read_call(half, self.sd[s * self.dw:], self.sq[s * self.pw:], 1, half["reads"], [half["q"]], out))
        self.cur = cur
        got = [self._read_back(OK, out, len(half["reads"]), half["width"]) for half, out in zip(op["halves"], outs)]
        return {"code": OK, "codes": codes, "rows": np.concatenate([g["rows"].reshape(-1) for g in got]),
                "guard": np.concatenate([g["guard"] for g in got])}

    def run_sub(self, sub, pz):
        return getattr(self, "op_" + sub["op"])(sub, pz)

    def _flags(self, lost):
        dp, pp = np.ones(self.k, np.uint8), np.ones(self.m, np.uint8)
        for j in lost:
            if j < self.k:
                dp[j] = 0
            else:
                pp[j - self.k] = 0
        return dp, pp

    def _flag_rows(self, patterns):
        rows = [self._flags(q) for q in patterns]
        return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])

    def op_prepare(self, op, pay):
        return {"code": self._code(self.enc.decode_prepare, *self._flags(op["lost"]))}

    def op_prepare_set(self, op, pay):
        return {"code": self._set_patterns(op["patterns"])}

    def op_scrub_pattern(self, op, pay):
        return {"code": self._code(self.enc.scrub_erasures, *self._flags(op["absent"]))}

    def op_scrub_pattern_set(self, op, pay):
        return {"code": self._code(self.enc.scrub_erasures_set, *self._flag_rows(op["patterns"]))}

    def _scrub_call(self, name, op):
        """the C entry point: (code, the count status bytes, *inconsistent); outputs preset to sentinels"""
        ct, cnt = self.ct, op["b1"] - op["b0"]
        D, Q = self._pool(op["b0"])
        out = np.full(cnt, 7, np.uint8)
        bad = ct.c_uint64(0xABCD)
        args = [self.enc._h, D.data_ptr(), Q.data_ptr(), cnt]
        if op["set"]:
            po = np.ascontiguousarray(op["pattern_of"], dtype=np.uint32)
            args.append(po.ctypes.data_as(ct.POINTER(ct.c_uint32)))
        args += [self._lib() or None, op["seed"], out.ctypes.data_as(ct.POINTER(ct.c_uint8)), ct.byref(bad)]
        code = getattr(self.fe.lib(), name + ("_set" if op["set"] else ""))(*args)
        return code, out.tolist(), int(bad.value)

    def op_verify(self, op, pay):
        code, ok, bad = self._scrub_call("fastecc_verify_batch", op)
        out = {"code": code, "consistent": ok, "inconsistent": bad}
        if op.get("single") is not None:
            D, Q = self._pool(op["single"])
            out["single"] = int(self.enc.verify(D, Q, seed=op["seed"], stream=self._lib()))
        return out

    def op_locate(self, op, pay):
        D, Q = self._pool(op["b0"])
        try:
            if op.get("set"):
                po = np.array(op["pattern_of"], dtype=np.uint32)
                status, lists = self.enc.locate_errors_batch_set(D, Q, op["b1"] - op["b0"], po, seed=op["seed"], stream=self._lib())
            else:
                status, lists = self.enc.locate_errors_batch(D, Q, op["b1"] - op["b0"], seed=op["seed"], stream=self._lib())
        except self.fe.FastEccError as e:
            return {"code": e.code, "status": getattr(e, "status", None), "lists": getattr(e, "lists", None)}
        status = status.tolist()
        return {"code": OK, "status": status, "lists": lists, "inconsistent": sum(1 for x in status if x)}

    def op_correct(self, op, pay):
        self.enc.set_option("correct_batch_mode", op["mode"])
        code, status, bad = self._scrub_call("fastecc_correct_batch", op)
        return {"code": code, "status": status, "inconsistent": bad}

    def _rebuild(self, op, name):
        self.enc.set_option("decode_batch_kernel", op["kernel"])
        D, Q = self._pool(op["b0"])
        cnt = op["b1"] - op["b0"]
        if op["set"]:
            po = np.array(op["pattern_of"], dtype=np.uint32)
            code = self._code(getattr(self.enc, name + "_batch_set"), D, Q, cnt, po, stream=self._lib())
            po[:] = 0xFFFFFFFE  # pattern_of may be reused as soon as the call returns
            return {"code": code}
        return {"code": self._code(getattr(self.enc, name + "_batch"), D, Q, cnt, stream=self._lib())}

    def op_repair(self, op, pay):
        return self._rebuild(op, "repair")

    def op_decode(self, op, pay):
        return self._rebuild(op, "decode")

    def op_reencode(self, op, pay):
        D, _ = self._pool(op["b0"])
        cnt = op["b1"] - op["b0"]
        if op["form"] == "pool":
            code = self._code(self.enc.encode_pool, D, self.sq, cnt, stream=self._lib())
        elif op["form"] == "batch":
            code = self._code(self.enc.encode_batch, D, self.sq, cnt, stream=self._lib())
        else:
            code = self._code(self.enc.encode, D, self.sq, stream=self._lib())
        self._order(0)
        return {"code": code, "parity": self._host(self.sq[:cnt * self.pw]).reshape(cnt, self.m, self.S)}

    def op_option(self, op, pay):
        self.enc.set_option(op["name"], op["value"])

    def op_stream(self, op, pay):
        self.cur = op["stream"]

    def _scratch(self, d, p):
        self._order(0)
        self.sd[:self.dw].copy_(self._dev(d))
        self.sq[:self.pw].copy_(self._dev(p))
        return self.sd, self.sq

    def _scratch_out(self, code):
        self._order(0)
        return {"code": code, "scratch_d": self._host(self.sd[:self.dw]).reshape(self.k, self.S),
                "scratch_p": self._host(self.sq[:self.pw]).reshape(self.m, self.S)}

    def op_probe_repair(self, op, pay):
        sd, sq = self._scratch(pay["scratch_d"], pay["scratch_p"])
        call = getattr(self.enc, op["form"])
        code = self._code(call, sd, sq, 1, stream=self._lib()) if op["form"].endswith("_batch") else self._code(call, sd, sq, stream=self._lib())
        return self._scratch_out(code)

    def op_probe_repair_set(self, op, pay):
        sd, sq = self._scratch(pay["scratch_d"], pay["scratch_p"])
        self.enc.set_option("decode_batch_kernel", op["kernel"])
        return self._scratch_out(self._code(getattr(self.enc, op["form"] + "_batch_set"), sd, sq, 1, [op["q"]], stream=self._lib()))

    def op_probe_verify(self, op, pay):
        ok = []
        for d, p in pay["scratch"]:
            sd, sq = self._scratch(d, p)
            ok.append(int(self.enc.verify(sd, sq, seed=op["seed"], stream=self._lib())))
        return {"code": OK, "ok": ok}

    def op_refused(self, op, pay):
        D, Q, lib, h = self.D, self.Q, self.fe.lib(), self.enc._h
        if op["which"] in ("bad_degraded_write", "no_set"):
            return self._refused_write(op, pay)
        if op["which"] == "bad_read":
            n, rotated = len(op["reads"]), self.cfg.placement == "rotated"
            outs = [self._read_buffer(n, op["width"]) for _ in range(2)]
            bad = list(op["reads"])
            bad[op["at"]] = self.count * self.k  # one past the pool's last block, among valid requests
            po = [b % self.n if b not in self.quarantined else PATTERN_NONE for b in range(self.count)]
            codes = [self._read_call(op, D, Q, self.count, bad, po if rotated else None, outs[0])]
            po = [PATTERN_NONE] * self.count
            po[op["reads"][op["at"]] // self.k] = op["entry"]  # the number of patterns in force: one past the last
            codes.append(self._read_call(op, D, Q, self.count, op["reads"], po, outs[1]))
            self._order(0)
            return {"code": codes[0], "codes": codes, "rows": np.concatenate([self._host(o) for o in outs])}
        if op["which"] == "bad_write":
            new = self._dev(np.zeros(2 * self.S, np.uint32))
            self.keep.append(new)
            return {"code": self._code(self.enc.update_batch, D, Q, self.count, [0, self.count * self.k], new, stream=self._lib())}
        if op["which"] == "bad_pattern":
            po = np.zeros(self.count, np.uint32)
            po[self.count // 2] = op["entry"]  # the number of patterns in force: one past the last
            return {"code": self._code(self.enc.repair_batch_set, D, Q, self.count, po, stream=self._lib())}
        return {"code": lib.fastecc_repair_batch(h, D.data_ptr(), Q.data_ptr(), 0, self._lib() or None)}
