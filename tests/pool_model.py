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

Reads ("read", extended sequences): fastecc_read_batch on fixed placement, fastecc_read_batch_set on rotated, over the whole pool: a present
block gives the mirror's words (a corrupted block reads back corrupted, a quarantined stripe's garbage is copied), a block lost under its
stripe's pattern gives the truth; lost blocks are requested only in stripes without a corrupted survivor (which survivors a pass reads is
left open by the header).  The backend presets n_reads + 1 output rows to CANARY and returns the rows and the extra row ("guard").

Bursts: a "burst" operation enqueues 2 to 4 calls (writes of every form, at most one rebuild; in extended sequences reads too, their output
read back only after the burst) back to back on the null and the side stream
with nothing read in between, so a call meets the previous call's staged list and buffers still in flight; its prediction is the calls
applied in order.

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
            new = _below_p(rng, (len(writes), self.S))
            new.reshape(-1)[:3] = [P - 1, 0, 1][: min(3, new.size)]
            pay["new"] = new
            if op["form"] != "pool":
                pay["old"] = np.stack([self.mirror_d[w // self.k, w % self.k] for w in writes])
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


class Generator:
    def __init__(self, model, seed, extended=False):
        self.m, self.rng = model, _rng("gen", model.cfg.name, seed)
        self.queue = collections.deque()
        self.drawn = self.skipped = 0
        self.dseed = 0
        self.verifies = 0
        m = model
        self.extended, self.seed, self.pool_encodes, self.used_form = extended, seed, 0, collections.Counter()
        self.weights, self.probe_list = (EXT_WEIGHTS, EXT_PROBES) if extended else (WEIGHTS, PROBES)
        kinds = [k for k in (EXT_KINDS if extended else KINDS)
                 if not (m.mixed and k == "corrupt") and not (m.rotated and k == "locate" and not extended)]
        self.emitted = self.probes_started = 0
        self.probe_at = 5 * (seed - EXT_SEEDS[0] + (2 if m.rotated else 0)) if extended else 2 * (seed + (4 if model.rotated else 0))
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
        w = np.array([self.weights[k] * (0.25 if idle.get(k) else 3.0 if not self.used[k] else 1.0) for k in self.kinds])
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

    def make_corrupt(self):
        m, rng = self.m, self.rng
        how = self._pick(["word", "word", "block", "big"])
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
        return [{"op": "device_down", "dev": self._pick([d for d in range(m.n) if d not in m.devs]), "dseed": self._ds()}]

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
        if m.ctx.prepared_set is None or (m.rotated and m.ctx.prepared_set != m.needed_set()):
            ops.append(self._state_prepare_set())
            patterns = ops[0]["patterns"]
        else:
            patterns = m.ctx.prepared_set
        if y == "prepare":
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
        else:
            ops.append(self.make_correct()[-1])
        j = self._pick([j for j in range(m.n) if j not in scrub])
        ops.append({"op": "probe_verify", "b": self._pick(m.live()), "j": j, "seed": int(self.rng.integers(1 << 40)), "dseed": self._ds(),
                    "probe": "scrub_after_" + z})
        return ops

    def make_probe_refused(self, which):
        if which == "bad_read":  # among valid requests an index count*k; for a requested stripe a pattern_of entry equal to the number of patterns
            m = self.m
            reads = [int(x) for x in self.rng.integers(m.count * m.k, size=int(self.rng.integers(2, 6)))]
            shape, col0, width = self._window()
            return [{"op": "refused", "which": which, "entry": len(m.ctx.prepared_set or ()), "reads": reads, "at": int(self.rng.integers(len(reads))),
                     "col0": col0, "width": width, "shape": shape, "probe": "refused_" + which}]
        return [{"op": "refused", "which": which, "entry": len(self.m.ctx.prepared_set or ()), "probe": "refused_" + which}]

    def next_op(self):
        self.emitted += 1
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
    def __init__(self, cfg, seed, step, what, log, extended=False):
        self.cfg, self.seed, self.step, self.what, self.log = cfg, seed, step, what, log
        super().__init__("config %s seed %d step %d: %s\nreplay: run_sequence(backend, config_named(%r), %d, steps=%d%s)\noperations:\n%s"
                         % (cfg.name, seed, step, what, cfg.name, seed, step + 1, ", extended=True" if extended else "", "\n".join(log)))


def _same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    return a == b


def run_sequence(backend, cfg, seed, steps=None, oracle=None, on_step=None, extended=False, log=None):
    """Apply the sequence of (cfg, seed) to a fresh model and to `backend`; after every step compare every host output and the whole pool.
    Returns the model's Coverage.  Raises SequenceFailure (config, seed, step, the operation log) at the first difference.  `extended`: the
    generator draws the extended kinds as well (the seeds EXT_SEEDS; off, a sequence is what it always was).  `log`: a list that receives the
    operation log, one JSON line per step."""
    if oracle is None:
        from oracle import Oracle
        oracle = Oracle()
    model = PoolModel(cfg, seed, oracle)
    gen = Generator(model, seed, extended)
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
                raise SequenceFailure(cfg, seed, step, "output %r is %r, the model says %r" % (key, got.get(key), want[key]), log, extended)
        d, p = backend.read_pool()
        if not np.array_equal(d, model.mirror_d) or not np.array_equal(p, model.mirror_p):
            bad = sorted({int(b) for b in np.nonzero((d != model.mirror_d).any(axis=(1, 2)) | (p != model.mirror_p).any(axis=(1, 2)))[0]})
            blocks = [j for j in range(model.n) if not np.array_equal(model.block(d, p, bad[0], j), model.block(model.mirror_d, model.mirror_p, bad[0], j))]
            raise SequenceFailure(cfg, seed, step, "the pool differs from the model in stripes %s (quarantined: %s); stripe %d blocks %s"
                                  % (bad, sorted(model.quarantined), bad[0], blocks), log, extended)
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

    def before(self, op):
        m, kind = self.m, op["op"]
        self.kinds[kind] += 1
        if kind == "burst":
            for sub in op["ops"]:
                self.before(sub)
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
        staged = (self._dev(pay["new"]), self._dev(pay["old"]) if op["form"] == "parity" else None)
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
            codes.append(self._code(self.enc.decode_prepare_set, *self._flag_rows(half["patterns"])))
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
        return {"code": self._code(self.enc.decode_prepare_set, *self._flag_rows(op["patterns"]))}

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
