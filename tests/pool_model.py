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

Bursts: a "burst" operation enqueues 2 to 4 calls (writes of every form, at most one rebuild) back to back on the null and the side stream
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


def config_named(name):
    return next(c for c in CONFIGS if c.name == name)


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
        self.options = {"scrub_batch_chunk": 0, "direct_kernel": 0, "decode_direct_max": 256, "locate_max": 256}
        self.stream = 0

    def snapshot(self):
        return (self.prepared, self.prepared_set, self.scrub, self.scrub_set, tuple(sorted(self.options.items())), self.stream)


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
            new = _below_p(rng, (len(op["writes"]), self.S))
            new.reshape(-1)[:3] = [P - 1, 0, 1][: min(3, new.size)]
            pay["new"] = new
            pay["old"] = np.stack([self.mirror_d[w // self.k, w % self.k] for w in op["writes"]])
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
        writes = op["writes"]
        if len(set(writes)) != len(writes):
            raise ModelError("duplicate write")
        touched = sorted({w // self.k for w in writes})
        if not all(self.whole(b) for b in touched):
            raise ModelError("a write into a stripe that is not whole")
        for u, w in enumerate(writes):
            self.truth_d[w // self.k, w % self.k] = pay["new"][u]
        for b in touched:
            self.truth_p[b] = self.codec.parity(self.truth_d[b])
            self.mirror_d[b], self.mirror_p[b] = self.truth_d[b], self.truth_p[b]

    def _prepare(self, op, pay):
        self.ctx.prepared = tuple(op["lost"])

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
        if self.rotated:
            raise ModelError("locate is a fixed-placement operation")
        self._scrub_ready(False)
        self._check_budget(op["b0"], op["b1"])
        lists = [sorted(self.corrupt[b]) for b in range(op["b0"], op["b1"])]
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
        pay["subs"], codes = [], []
        for sub in op["ops"]:
            if sub["op"] not in ("write", "repair", "decode"):
                raise ModelError("a burst holds enqueued calls only")
            pay["subs"].append(self.payload(sub))
            codes.append(self.apply(sub, pay["subs"][-1])["code"])
        return {"code": OK, "codes": codes}

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


class Generator:
    def __init__(self, model, seed):
        self.m, self.rng = model, _rng("gen", model.cfg.name, seed)
        self.queue = collections.deque()
        self.drawn = self.skipped = 0
        self.dseed = 0
        self.verifies = 0
        m = model
        kinds = [k for k in KINDS if not (m.mixed and k == "corrupt") and not (m.rotated and k == "locate")]
        self.emitted = self.probes_started = 0
        self.probe_at = 2 * (seed + (4 if model.rotated else 0))
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
        for _ in range(len(PROBES)):
            family, variant = PROBES[self.probe_at % len(PROBES)]
            skip = ((m.mixed and (family == "scrub" or variant in ("correct", "locate"))) or (m.rotated and variant == "locate"))
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
        w = np.array([WEIGHTS[k] * (0.25 if idle.get(k) else 3.0 if not self.used[k] else 1.0) for k in self.kinds])
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
    def make_write(self):
        m, rng = self.m, self.rng
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
        return ([pre] if pre else []) + [{"op": "locate", "b0": b0, "b1": b1, "seed": int(self.rng.integers(1 << 40))}]

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
        if m.n == 2 * m.k and not m.mixed and self.rng.random() < 0.5:
            b0, b1 = self._range(clean)
            return [{"op": "reencode", "form": "batch", "b0": b0, "b1": b1}]
        b = self._pick(good)
        return [{"op": "reencode", "form": "one", "b0": b, "b1": b + 1}]

    def make_option(self):
        m = self.m
        name = self._pick(["scrub_batch_chunk", "scrub_batch_chunk", "direct_kernel", "decode_direct_max", "locate_max"])
        if not m.mixed and self.used["option"] == 0:  # a sequence's first flip makes its scrub calls take several chunks
            return [{"op": "option", "name": "scrub_batch_chunk", "value": int(self._pick([3, 4]))}]
        if name == "locate_max":
            t = max([sum(1 for v in m.corrupt[b].values() if v == "small") for b in m.live()] + [1])
            value = self._pick([v for v in (1, 2, 8, 256) if v >= t])
        else:
            value = self._pick({"scrub_batch_chunk": [0, 3, 4, 8], "direct_kernel": [0, 1, 2], "decode_direct_max": [0, 1, 256]}[name])
        return [{"op": "option", "name": name, "value": int(value)}]

    def make_stream(self):
        return [{"op": "stream", "stream": 1 - self.m.ctx.stream}]

    def make_burst(self):
        """2 to 4 enqueued calls back to back (writes of every form, at most one rebuild), each on the null or the side stream"""
        m, rng = self.m, self.rng
        ops = []
        for _ in range(int(rng.integers(2, 5))):
            w = self.make_write()
            if w:
                ops += w
        if self._rebuild_prereq() is None and rng.random() < 0.6:
            r = self._make_rebuild(self._pick(["repair", "decode"]))
            if r:
                ops.insert(int(rng.integers(len(ops) + 1)), r[-1])
        if len(ops) < 2:
            return None
        for sub in ops:
            sub["stream"] = int(rng.integers(2))
        return [{"op": "burst", "ops": ops}]

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
        else:
            ops.append(self.make_correct()[-1])
        j = self._pick([j for j in range(m.n) if j not in scrub])
        ops.append({"op": "probe_verify", "b": self._pick(m.live()), "j": j, "seed": int(self.rng.integers(1 << 40)), "dseed": self._ds(),
                    "probe": "scrub_after_" + z})
        return ops

    def make_probe_refused(self, which):
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
    def __init__(self, cfg, seed, step, what, log):
        self.cfg, self.seed, self.step, self.what, self.log = cfg, seed, step, what, log
        super().__init__("config %s seed %d step %d: %s\nreplay: run_sequence(backend, config_named(%r), %d, steps=%d)\noperations:\n%s"
                         % (cfg.name, seed, step, what, cfg.name, seed, step + 1, "\n".join(log)))


def _same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    return a == b


def run_sequence(backend, cfg, seed, steps=None, oracle=None, on_step=None):
    """Apply the sequence of (cfg, seed) to a fresh model and to `backend`; after every step compare every host output and the whole pool.
    Returns the model's Coverage.  Raises SequenceFailure (config, seed, step, the operation log) at the first difference."""
    if oracle is None:
        from oracle import Oracle
        oracle = Oracle()
    model = PoolModel(cfg, seed, oracle)
    gen = Generator(model, seed)
    cov = Coverage(model)
    backend.start(model.mirror_d, model.mirror_p, sorted(model.quarantined))
    log = []
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
                raise SequenceFailure(cfg, seed, step, "output %r is %r, the model says %r" % (key, got.get(key), want[key]), log)
        d, p = backend.read_pool()
        if not np.array_equal(d, model.mirror_d) or not np.array_equal(p, model.mirror_p):
            bad = sorted({int(b) for b in np.nonzero((d != model.mirror_d).any(axis=(1, 2)) | (p != model.mirror_p).any(axis=(1, 2)))[0]})
            blocks = [j for j in range(model.n) if not np.array_equal(model.block(d, p, bad[0], j), model.block(model.mirror_d, model.mirror_p, bad[0], j))]
            raise SequenceFailure(cfg, seed, step, "the pool differs from the model in stripes %s (quarantined: %s); stripe %d blocks %s"
                                  % (bad, sorted(model.quarantined), bad[0], blocks), log)
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
            return
        v = self.variants
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
            per = collections.Counter(w // m.k for w in op["writes"])
            if op["form"] != "single" and max(per.values()) > 16:
                v["segment_over_16"] += 1
        if kind == "corrupt" and len(op["blocks"]) + len(m.devs) > 16:
            v["over_16_lost"] += 1
        if m.ctx.stream == 1 and kind not in ("stream", "option", "device_replaced", "corrupt", "device_down"):
            v["side_stream"] += 1

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
        for u, w in enumerate(op["writes"]):
            self.d[w // self.k, w % self.k] = pay["new"][u]
        for b in sorted({w // self.k for w in op["writes"]}):
            self.p[b] = self.codec.parity(self.d[b])
            self.td[b], self.tp[b] = self.d[b], self.p[b]

    def op_prepare(self, op, pay):
        self.prepared = tuple(op["lost"])

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
        if not op["set"]:
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
        lists = [self._wrong(b, self.scrub) for b in range(op["b0"], op["b1"])]
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
        return {"code": OK, "codes": [self.run(sub, pz)["code"] for sub, pz in zip(op["ops"], pay["subs"])]}

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
        writes, k = op["writes"], self.k
        new, old = staged or self._stage(op, pay)
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
        staged = [self._stage(sub, pz) if sub["op"] == "write" else None for sub, pz in zip(op["ops"], pay["subs"])]
        cur, codes = self.cur, []
        for sub, pz, st in zip(op["ops"], pay["subs"], staged):
            self.cur = sub["stream"]
            out = self.op_write(sub, pz, st) if sub["op"] == "write" else self.run_sub(sub, pz)
            codes.append(out["code"])
        self.cur = cur
        return {"code": OK, "codes": codes}

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
        if op["form"] == "batch":
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
        if op["which"] == "bad_write":
            new = self._dev(np.zeros(2 * self.S, np.uint32))
            self.keep.append(new)
            return {"code": self._code(self.enc.update_batch, D, Q, self.count, [0, self.count * self.k], new, stream=self._lib())}
        if op["which"] == "bad_pattern":
            po = np.zeros(self.count, np.uint32)
            po[self.count // 2] = op["entry"]  # the number of patterns in force: one past the last
            return {"code": self._code(self.enc.repair_batch_set, D, Q, self.count, po, stream=self._lib())}
        return {"code": lib.fastecc_repair_batch(h, D.data_ptr(), Q.data_ptr(), 0, self._lib() or None)}
