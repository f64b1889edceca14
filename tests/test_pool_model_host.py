"""The pool model and its harness (tests/pool_model.py), checked without a GPU.

  - the model is sound: its parity equals the generator matrix of fastecc_code_coefficient (host-only arithmetic of the library, the one
    thing here that is not the oracle), and decoding its truth under every device-down pattern gives the truth back;
  - every (config, seed) of tests/test_gpu_pool_sequences.py runs green on the exact numpy backend, the extended sequences (EXT_SEEDS) and the
    degraded ones (DEG_SEEDS) included;
  - the 64 sequences of SEEDS are, operation for operation, what they were before the extended kinds existed, and the 32 of EXT_SEEDS what they
    were before the degraded kinds existed (recorded digests);
  - seven injected defects, seven more in the extended operations and ten in the degraded and window writes are each reported at the step where
    they first change a byte or an answer;
  - the committed seeds of every configuration cover what they must (operation kinds, variants, state probes, few illegal draws, the budget)."""
import hashlib
import itertools
import json
import os

import numpy as np
import pytest

import fastecc_amd as fe
import pool_model as pm
from pool_model import P

FIXED = [c for c in pm.CONFIGS if c.placement == "fixed"]
CASES = [(cfg.name, seed) for cfg in pm.CONFIGS for seed in pm.SEEDS]
EXT_CASES = [(cfg.name, seed) for cfg in pm.CONFIGS for seed in pm.EXT_SEEDS]
DEG_CASES = [(cfg.name, seed) for cfg in pm.CONFIGS for seed in pm.DEG_SEEDS]


def group_of(cfg):
    return cfg.name.rsplit("_", 1)[0]


@pytest.fixture(scope="module")
def generator_matrix():
    cache = {}

    def get(cfg):
        key = (cfg.n, cfg.k, cfg.flags)
        if key not in cache:
            cache[key] = np.array([[fe.code_coefficient(cfg.n, cfg.k, i, q, cfg.flags) for i in range(cfg.k)] for q in range(cfg.n - cfg.k)],
                                  dtype=np.uint64)
        return cache[key]
    return get


def matrix_parity(G, x):
    """parity block q = sum_i G[q, i] * data block i mod p, exactly (every product is below 2^64, the sum of reduced terms far below)"""
    out = np.zeros((G.shape[0], x.shape[1]), dtype=np.uint64)
    for i in range(G.shape[1]):
        out += (G[:, i:i + 1] * x[i:i + 1].astype(np.uint64)) % np.uint64(P)
    return (out % np.uint64(P)).astype(np.uint32)


@pytest.mark.parametrize("cfg", FIXED, ids=[c.name for c in FIXED])
def test_model_parity_is_the_generator_matrix(oracle, generator_matrix, cfg):
    assert not cfg.order or fe.mixed_radix_order(cfg.k) == cfg.order
    codec, G = pm.Codec(oracle, cfg.n, cfg.k, cfg.flags, cfg.order), generator_matrix(cfg)
    rng = np.random.default_rng(cfg.n * 1000 + cfg.k)
    x = rng.integers(0, P, size=(cfg.k, 5), dtype=np.uint64).astype(np.uint32)
    x[0, :3] = [0, P - 1, 1]
    assert np.array_equal(codec.parity(x), matrix_parity(G, x))
    units = np.eye(cfg.k, dtype=np.uint32)  # word i of every block: the unit stripe e_i
    assert np.array_equal(codec.parity(units), G.astype(np.uint32))


def solve_lost_data(G, d, p, lost, k):
    """the lost data blocks from the surviving ones: Gaussian elimination over GF(p) on the generator matrix (exact integers)"""
    lost_d = [j for j in lost if j < k]
    rows = [q for q in range(G.shape[0]) if q + k not in lost][:len(lost_d)]
    out = d.copy()
    for w in range(d.shape[1]):
        A = [[int(G[q, i]) for i in lost_d] + [(int(p[q, w]) - sum(int(G[q, i]) * int(d[i, w]) for i in range(k) if i not in lost_d)) % P] for q in rows]
        r = len(lost_d)
        for c in range(r):
            piv = next(i for i in range(c, r) if A[i][c])
            A[c], A[piv] = A[piv], A[c]
            inv = pow(A[c][c], P - 2, P)
            A[c] = [v * inv % P for v in A[c]]
            for i in range(r):
                if i != c and A[i][c]:
                    A[i] = [(v - A[i][c] * u) % P for v, u in zip(A[i], A[c])]
        for c, j in enumerate(lost_d):
            out[j, w] = A[c][r]
    return out


def oracle_decode(oracle, cfg, d, p, lost):
    """Oracle.decode on the (2N,N) code this code is cut from: zero-extended data rows are known, folded parity block j sits at row
    j << fold, the n = 4k code's first coset is the (2k,k) parity (its other cosets are not needed: at most two blocks are lost)."""
    k, m, S = cfg.k, cfg.n - cfg.k, d.shape[1]
    lg = max(1, int(np.ceil(np.log2(k))))
    N = 1 << lg
    coset = cfg.n == 4 * k
    fold = 0 if coset else min(lg - (int(np.ceil(np.log2(m))) if m > 1 else 0), 4)
    D, Q = np.zeros((N, S), np.uint32), np.zeros((N, S), np.uint32)
    dp, pp = np.ones(N, np.uint8), np.zeros(N, np.uint8)
    D[:k] = d
    for j in range(min(m, N) if coset else m):
        Q[j << fold], pp[j << fold] = p[j], 1
    for j in lost:
        if j < k:
            dp[j], D[j] = 0, 0xABABABAB
        elif (j - k) << fold < N and (not coset or j - k < N):
            pp[(j - k) << fold] = 0
    got = oracle.decode(D, Q, dp, pp)
    assert got is not None
    return got[:k]


@pytest.mark.parametrize("cfg", FIXED, ids=[c.name for c in FIXED])
def test_truth_decodes_under_every_device_down_pattern(oracle, generator_matrix, cfg):
    codec = pm.Codec(oracle, cfg.n, cfg.k, cfg.flags, cfg.order)
    rng = np.random.default_rng(cfg.n)
    d = rng.integers(0, P, size=(cfg.k, 3), dtype=np.uint64).astype(np.uint32)
    p = codec.parity(d)
    pairs = [tuple(int(x) for x in rng.choice(cfg.n, size=2, replace=False)) for _ in range(24)] + [(0, cfg.k), (cfg.k - 1, cfg.n - 1), (0, 1)]
    for lost in [(j,) for j in range(cfg.n)] + pairs:
        if cfg.order:
            got = solve_lost_data(generator_matrix(cfg), d, p, lost, cfg.k)
        else:
            got = oracle_decode(oracle, cfg, d, p, lost)
        assert np.array_equal(got, d), lost


_DRY, _LOGS = {}, {}


def dry_run(oracle, name, seed):
    """the sequence of (name, seed) on the exact backend, once per session: its Coverage (the seeds of EXT_SEEDS are the extended sequences, those
    of DEG_SEEDS the degraded ones)"""
    if (name, seed) not in _DRY:
        cfg = pm.config_named(name)
        _LOGS[name, seed] = []
        _DRY[name, seed] = pm.run_sequence(pm.ModelBackend(cfg, oracle), cfg, seed, oracle=oracle, extended=seed in pm.EXT_SEEDS, degraded=seed in pm.DEG_SEEDS,
                                                log=_LOGS[name, seed])
    return _DRY[name, seed]


def test_the_committed_sequences_are_unchanged(oracle):
    """tests/golden/pool_sequence_digests.json: sha256 of the operation log (run_sequence's JSON lines, joined by newlines) of every (config, seed)
    of SEEDS, recorded on the commit before the generator learned the extended kinds, and of EXT_SEEDS, recorded on the commit before it learned
    the degraded kinds.  With `extended` off it draws what it drew then, and with `degraded` off an extended sequence is what it was."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pool_sequence_digests.json")) as f:
        recorded = json.load(f)
    assert sorted(recorded) == sorted("%s:%d" % c for c in CASES + EXT_CASES)
    changed = []
    for name, seed in CASES + EXT_CASES:
        dry_run(oracle, name, seed)
        assert len(_LOGS[name, seed]) == pm.config_named(name).steps
        if hashlib.sha256("\n".join(_LOGS[name, seed]).encode()).hexdigest() != recorded["%s:%d" % (name, seed)]:
            changed.append((name, seed))
    assert not changed


@pytest.mark.parametrize("name,seed", CASES + EXT_CASES + DEG_CASES)
def test_harness_passes_on_the_exact_backend(oracle, name, seed):
    cfg = pm.config_named(name)
    cov = dry_run(oracle, name, seed)
    assert 4 * cov.skipped <= cov.drawn, (cov.skipped, cov.drawn)  # at most a quarter of the draws were illegal
    assert 25 <= cfg.steps <= 40


GROUPS = sorted({group_of(c) for c in pm.CONFIGS})


@pytest.mark.parametrize("group", GROUPS)
def test_coverage_of_the_committed_seeds(oracle, group):
    """Run on the model backend: the sequences are the GPU test's (the generator never reads a backend), and Coverage.before raises if a
    scrub operation meets a stripe outside the budget 2t + b + w <= n - k, t <= locate_max."""
    cfgs = [c for c in pm.CONFIGS if group_of(c) == group]
    total = pm.Coverage(None)
    for cfg in cfgs:
        for seed in pm.SEEDS:
            total.merge(dry_run(oracle, cfg.name, seed))
    mixed, k = bool(cfgs[0].flags), cfgs[0].k
    kinds = [x for x in pm.KINDS if not (mixed and x == "corrupt")] + ["subrange"]
    assert not {x: total.kinds[x] for x in kinds if total.kinds[x] < 5}
    variants = ["set", "single", "correct_mode_0", "correct_mode_1", "correct_mode_2", "kernel_0", "kernel_1", "kernel_2", "write_parity",
                "write_single", "write_batch", "subrange", "side_stream", "burst_two_streams"]
    variants += ["segment_over_16"] if k > 16 else []   # more than 16 writes in one stripe need k > 16
    variants += [] if mixed else ["multi_chunk"]        # a mixed-radix context refuses every scrub call
    variants += ["over_16_lost"] if group == "256_128" else []
    assert not [x for x in variants if not total.variants[x]]
    probes = [f + "_after_" + v if f != "refused" else "refused_" + v for f, v in pm.PROBES]
    if mixed:
        probes = [x for x in probes if not x.startswith("scrub_") and not x.endswith(("_correct", "_locate"))]
    assert not {x: total.probes[x] for x in probes if total.probes[x] < 2}


NEW_PROBES = ["prepared_after_read", "set_after_read", "scrub_after_read", "read_after_prepare", "read_after_prepare_set", "refused_bad_read"]


@pytest.mark.parametrize("group", GROUPS)
def test_coverage_of_the_extended_seeds(oracle, group):
    """What the two extended seeds of a configuration's two placements must meet between them (counted on the model, as above)."""
    cfgs = [c for c in pm.CONFIGS if group_of(c) == group]
    total, fixed = pm.Coverage(None), pm.Coverage(None)
    for cfg in cfgs:
        for seed in pm.EXT_SEEDS:
            total.merge(dry_run(oracle, cfg.name, seed))
            if cfg.placement == "fixed":
                fixed.merge(dry_run(oracle, cfg.name, seed))
    mixed = bool(cfgs[0].flags)
    kinds = ["read", "write_pool", "reencode_pool", "locate"]  # the new kind, the new forms, and locate now on both placements
    assert not {x: total.kinds[x] for x in kinds if total.kinds[x] < 5}
    probes = [x for x in NEW_PROBES if not (mixed and x.startswith("scrub_"))] + ([] if mixed else ["prepared_after_locate"])
    assert not {x: total.probes[x] for x in probes if total.probes[x] < 2}
    variants = ["read_set", "read_single", "read_mixed_list", "read_pattern_none", "read_parity_only", "read_side_stream", "read_in_two_stream_burst",
                "locate_set", "write_pool_subrange", "reencode_pool_kernel_0", "reencode_pool_kernel_1", "reencode_pool_kernel_2",
                "read_after_prepare_plain", "read_after_prepare_transform", "read_after_prepare_parity"]
    variants += ["window_" + x for x in pm.WINDOWS]
    assert not [x for x in variants if not total.variants[x]]
    if group == "256_128":  # the single form serves up to 256 lost blocks, a set at most 16 per pattern
        assert fixed.variants["read_single_over_16_lost"]


DEG_PROBES = ["prepared_after_degraded_write", "set_after_degraded_write", "scrub_after_degraded_write", "write_after_prepare_set",
              "read_after_degraded_write", "repair_after_degraded_write", "untouched_pattern_ignored", "refused_bad_degraded_write", "refused_no_set"]


@pytest.mark.parametrize("group", GROUPS)
def test_coverage_of_the_degraded_seeds(oracle, group):
    """What the two degraded seeds of a configuration's two placements must meet between them (counted on the model, as above)."""
    cfgs = [c for c in pm.CONFIGS if group_of(c) == group]
    total = pm.Coverage(None)
    for cfg in cfgs:
        for seed in pm.DEG_SEEDS:
            total.merge(dry_run(oracle, cfg.name, seed))
    mixed, k = bool(cfgs[0].flags), cfgs[0].k
    probes = [x for x in DEG_PROBES if not (mixed and x.startswith("scrub_"))]
    assert not {x: total.probes[x] for x in probes if total.probes[x] < 2}
    forms = ["write_%s_%s" % (f, w) for f in pm.WINDOW_FORMS for w in ("window", "whole_block")]  # every form, with and without a window
    assert not {x: total.variants[x] for x in forms if total.variants[x] < 5}
    variants = ["write_window_" + x for x in pm.WRITE_WINDOWS]  # (pool writes alone: a probe's scratch write counts as probe_write_*)
    # the scratch writes of the probes, and those in the middle of a state probe, through the whole-block and the window entry points
    variants += ["probe_write_whole_block", "probe_write_window", "state_probe_write_whole_block", "state_probe_write_window"]
    variants += ["write_absent_data", "write_present_of_degraded", "write_mixed_list", "write_parity_only_stripe", "write_pattern_none",
                 "read_of_written_absent_block"]
    variants += [] if mixed else ["window_beside_corruption"]  # the mixed-radix group draws no corruption
    # the bursts: (a) a read beside a rebuilding write on the other stream, in both orders, (b) two rebuilding writes of different widths on
    # different streams, and (c) a plain window write directly after a decode_prepare_set
    variants += ["burst_read_then_rebuilding_write", "burst_rebuilding_write_then_read", "burst_rebuilding_writes_two_widths", "window_after_prepare_set"]
    variants += ["segment_over_16_rebuilt"] if k > 16 else []
    assert not [x for x in variants if not total.variants[x]]


def test_every_refused_degraded_write_is_drawn(oracle):
    """refused_bad_degraded_write draws one variant per probe: the committed sequences meet all six between them, each as a write that the model
    allows but for the variant's own argument (PoolModel._refused raises ModelError otherwise), the variants that are no matter of the window
    through the whole-block and the window entry point"""
    total = pm.Coverage(None)
    for name, seed in DEG_CASES:
        total.merge(dry_run(oracle, name, seed))
    assert not [x for x in pm.BAD_DEGRADED_WRITES if not total.variants["refused_" + x]]
    assert not [(x, e) for x in ("entry", "null_pattern_of", "overlap") for e in ("whole_block", "window") if not total.variants["refused_%s_%s" % (x, e)]]
    assert not [x for x in ("width0", "past_end", "overflow") if not total.variants["refused_%s_window" % x]]


def test_a_refused_degraded_write_has_one_reason(oracle):
    """the model refuses to predict a refusal that has a second reason: a set in force whose number of patterns a touched stripe's entry reaches,
    a quarantined stripe, a window of the call that is not the variant's"""
    cfg = pm.config_named("20_16_s64_rotated")
    model = pm.PoolModel(cfg, 7, oracle)
    b = model.live()[5]
    op = {"op": "refused", "which": "bad_degraded_write", "variant": "past_end", "form": "batch_set", "writes": [b * cfg.k + 1], "entry": model.npat,
          "pattern_of": model.pattern_of(0, cfg.count, lambda x: x not in model.quarantined), "col0": 3, "width": 5, "shape": "narrow",
          "call_col0": cfg.S + 1 - 5, "call_width": 5, "entries": ["window"], "dseed": 1}
    model.apply({"op": "prepare_set", "patterns": [[1], [2], [3]]}, {})  # stripe b's entry b mod n is beyond these three patterns
    with pytest.raises(pm.ModelError):
        model.apply(op, model.payload(op))
    model.apply({"op": "prepare_set", "patterns": [list(q) for q in model.needed_set()]}, {})
    assert model.apply(op, model.payload(op))["codes"] == [pm.E_INVAL]
    for wrong in ({"writes": [sorted(model.quarantined)[0] * cfg.k]}, {"call_col0": 3}, {"entry": 3}, {"writes": [cfg.count * cfg.k]}):
        with pytest.raises(pm.ModelError):
            model.apply(dict(op, **wrong), model.payload(dict(op, **wrong)))


def test_the_model_refuses_illegal_degraded_writes(oracle):
    """include/fastecc.h: a plain form into a stripe with an absent block, a window over a wrong word and a quarantined stripe have no defined
    result: ModelError.  A window beside a single wrong word is legal and the corruption mark stays."""
    cfg = pm.config_named("20_16_s64_rotated")
    model = pm.PoolModel(cfg, 7, oracle)
    b = model.live()[0]

    def write(form, blocks, **kw):
        op = dict({"op": "write", "form": form, "writes": blocks, "dseed": 1}, **kw)
        if form in pm.SET_FORMS:
            op["pattern_of"] = model.pattern_of(0, cfg.count, lambda x: x not in model.quarantined)
        return model.apply(op, model.payload(op))
    corrupt = {"op": "corrupt", "b": b, "blocks": [1], "how": "word", "dseed": 2}
    model.apply(corrupt, model.payload(corrupt))
    col = int(model.wrong_columns(b)[0])
    beside = (col + 1) % cfg.S
    with pytest.raises(pm.ModelError):
        write("batch", [b * cfg.k], col0=col, width=1, shape="word")
    with pytest.raises(pm.ModelError):
        write("batch", [b * cfg.k])
    with pytest.raises(pm.ModelError):
        write("single", [b * cfg.k + 2], col0=beside, width=1, shape="word")  # single and pool keep no window
    write("batch", [b * cfg.k + 1], col0=beside, width=1, shape="word")  # the corrupted block itself, beside its wrong word
    assert model.corrupt[b] == {1: "small"} and model.mirror_d[b, 1, col] != model.truth_d[b, 1, col]
    assert np.array_equal(model.truth_p[b][:, beside], model.mirror_p[b][:, beside])
    with pytest.raises(pm.ModelError):
        write("batch_set", [b * cfg.k + 3])  # no set prepared
    down = {"op": "device_down", "dev": (0 + b) % cfg.n, "dseed": 3}  # stripe b loses data block 0
    model.apply(down, model.payload(down))
    model.apply({"op": "prepare_set", "patterns": [list(q) for q in model.needed_set()]}, {})
    with pytest.raises(pm.ModelError):
        write("parity", [b * cfg.k + 3], col0=beside, width=1, shape="word")  # a plain form, an absent block
    garbage = model.mirror_d[b, 0].copy()
    write("batch_set", [b * cfg.k, b * cfg.k + 3], col0=beside, width=1, shape="word")
    assert np.array_equal(model.mirror_d[b, 0], garbage) and model.truth_d[b, 0, beside] != garbage[beside]  # the absent block stays as it is
    with pytest.raises(pm.ModelError):
        write("batch_set", [sorted(model.quarantined)[0] * cfg.k], col0=beside, width=1, shape="word")


def test_sequences_are_deterministic_and_replayable(oracle):
    cfg = pm.config_named("20_16_s64_rotated")
    logs = []
    for steps in (None, None, 17):
        log = []
        pm.run_sequence(pm.ModelBackend(cfg, oracle), cfg, 3, steps=steps, oracle=oracle, on_step=lambda s, op: log.append(repr(op)))
        logs.append(log)
    assert logs[0] == logs[1] and len(logs[0]) == cfg.steps
    assert logs[2] == logs[0][:17]


def test_the_prepared_pattern_is_unspecified_after_correct(oracle):
    """include/fastecc.h: fastecc_correct* REPLACES the prepared pattern; the model refuses to predict a use of it before a new decode_prepare."""
    cfg = pm.config_named("20_16_s64_fixed")
    model = pm.PoolModel(cfg, 1, oracle)
    model.apply({"op": "prepare", "lost": [2]}, {})
    model.apply({"op": "scrub_pattern", "absent": []}, {})
    model.apply({"op": "correct", "set": False, "b0": 0, "b1": cfg.count, "seed": 1, "mode": 0}, {})
    assert model.ctx.prepared == pm.UNSPECIFIED
    probe = {"op": "probe_repair", "b": 0, "form": "repair", "dseed": 1}
    with pytest.raises(pm.ModelError):
        model.payload(probe)
    with pytest.raises(pm.ModelError):
        model.apply({"op": "repair", "set": False, "b0": 0, "b1": 2, "kernel": 0}, {})
    read = {"op": "read", "set": False, "reads": [0, 17], "col0": 0, "width": cfg.S, "shape": "whole"}
    with pytest.raises(pm.ModelError):
        model.apply(read, {})  # fastecc_read_batch reads the single prepared pattern too
    with pytest.raises(pm.ModelError):
        model.payload({"op": "probe_read", "set": False, "q": 0, "b": 0, "reads": [1], "col0": 0, "width": 1, "shape": "word", "dseed": 2})
    model.apply({"op": "prepare", "lost": []}, {})
    model.apply({"op": "repair", "set": False, "b0": 0, "b1": 2, "kernel": 0}, {})
    assert model.apply(read, {})["code"] == pm.OK


# ---- injected defects: each a ModelBackend that is wrong in one way; `fired` is the step at which the defect first changed a byte of the
# pool or an answer as a caller sees them at the end of a step (None while it has not) ----
class Defective(pm.ModelBackend):
    """Runs an exact ModelBackend beside itself: `fired` is the first step after which its answers or its pool differ from the exact one's."""
    fired = None

    def __init__(self, cfg, oracle):
        super().__init__(cfg, oracle)
        self.exact, self.depth = pm.ModelBackend(cfg, oracle), 0

    def start(self, d, p, quarantined):
        super().start(d, p, quarantined)
        self.exact.start(d, p, quarantined)

    def run(self, op, pay):
        self.depth += 1
        got = super().run(op, pay)
        self.depth -= 1
        if self.depth == 0 and self.fired is None:
            want = self.exact.run(op, pay)
            same = all(pm._same(want[x], got.get(x)) for x in want) and np.array_equal(self.d, self.exact.d) and np.array_equal(self.p, self.exact.p)
            if not same:
                self.fired = self.step
        return got


class SkipsAParityBlock(Defective):
    """update_batch skips one parity block of one touched stripe"""

    def op_write(self, op, pay):
        if op["form"] != "batch":
            return super().op_write(op, pay)
        b = op["writes"][0] // self.k
        old = self.p[b, self.m - 1].copy()
        super().op_write(op, pay)
        self.p[b, self.m - 1] = old


class TouchesAnotherStripe(Defective):
    """update_batch touches a stripe that no write names"""

    def op_write(self, op, pay):
        super().op_write(op, pay)
        touched = {w // self.k for w in pm.writes_of(op, self.k)}
        others = [b for b in range(self.count) if b not in touched]
        if op["form"] == "batch" and others:
            self.p[others[len(others) // 2], 0, 0] ^= np.uint32(1)


class ShiftedPatterns(Defective):
    """repair_batch_set uses stripe b - 1's pattern for stripe b"""

    def op_repair(self, op, pay):
        if op["set"]:
            po = op["pattern_of"]
            shifted = [po[b] if po[b] == pm.PATTERN_NONE or b == 0 or po[b - 1] == pm.PATTERN_NONE else po[b - 1] for b in range(len(po))]
            op = dict(op, pattern_of=shifted)
        return super().op_repair(op, pay)


class RewritesAbsentBlocks(Defective):
    """correct_batch rewrites a consistent stripe's absent block"""

    def op_correct(self, op, pay):
        out = super().op_correct(op, pay)
        if not op["set"] and out["code"] == pm.OK:
            for i, b in enumerate(range(op["b0"], op["b1"])):
                if out["status"][i] == 0:
                    for j in self.scrub:
                        self.blk(self.d, self.p, b, j)[:] = self.blk(self.td, self.tp, b, j)
        return out


class ReadsQuarantined(Defective):
    """verify_batch_set reads a quarantined stripe: reports 0 for it"""

    def op_verify(self, op, pay):
        out = super().op_verify(op, pay)
        if op["set"] and out["code"] == pm.OK:
            for i, q in enumerate(op["pattern_of"]):
                if q == pm.PATTERN_NONE:
                    out["consistent"][i] = 0
            out["inconsistent"] = out["consistent"].count(0)
        return out


class SetClobbersPrepared(Defective):
    """decode_prepare_set clobbers the single prepared pattern"""

    def op_prepare_set(self, op, pay):
        super().op_prepare_set(op, pay)
        self.prepared = self.prepared_set[0]


class StaleChunking(Defective):
    """a call after scrub_batch_chunk changed still walks the old chunks: the wrong stripes are answered"""
    used = 0

    def op_verify(self, op, pay):
        out = super().op_verify(op, pay)
        new = self.options.get("scrub_batch_chunk", 0)
        if out["code"] == pm.OK and new != self.used:
            right, cnt = list(out["consistent"]), op["b1"] - op["b0"]
            old_c, new_c = self.used or 1 << 16, new or 1 << 16
            src = [(i // new_c) * old_c + i % new_c for i in range(cnt)]
            out["consistent"] = [right[s] if s < cnt else 1 for s in src]
            out["inconsistent"] = out["consistent"].count(0)
        self.used = new
        return out


# ---- defects in the extended operations ----
class CopiesLostBlocks(Defective):
    """a read returns what the pool holds for a lost block: a copy instead of a rebuild"""

    def read_rows(self, d, td, reads, lost_of, col0, width):
        return super().read_rows(d, td, reads, lambda b: (), col0, width)


class ReadsUnderTheOldPattern(Defective):
    """fastecc_read_batch keeps using the pattern that was prepared before the last decode_prepare (a stale descriptor)"""
    before = None

    def op_prepare(self, op, pay):
        self.before = self.prepared
        return super().op_prepare(op, pay)

    def single_pattern(self):
        return self.prepared if self.before is None else self.before


class ReadWritesPastItsRows(Defective):
    """a read writes one row past n_reads"""

    def read_rows(self, d, td, reads, lost_of, col0, width):
        out = super().read_rows(d, td, reads, lost_of, col0, width)
        out[len(reads)] = out[0]
        return out


class ReadWritesThePool(Defective):
    """a read writes a word into the pool"""

    def op_read(self, op, pay):
        out = super().op_read(op, pay)
        b, i = divmod(op["reads"][0], self.k)
        self.d[b, i, op["col0"]] ^= np.uint32(1)
        return out


class ShiftedSetLocation(Defective):
    """fastecc_locate_errors_batch_set answers stripe b under pattern pattern_of[b + 1]"""

    def op_locate(self, op, pay):
        if op.get("set"):
            po = op["pattern_of"]
            nxt = [po[i + 1] if i + 1 < len(po) and pm.PATTERN_NONE not in (po[i], po[i + 1]) else po[i] for i in range(len(po))]
            op = dict(op, pattern_of=nxt)
        return super().op_locate(op, pay)


class PoolEncodeSkipsTheLastStripe(Defective):
    """fastecc_encode_pool leaves the last stripe of a sub-range unencoded"""

    def encoded_stripes(self, op, stripes):
        return stripes[:-1] if op["form"] == "pool" else stripes

    def op_reencode(self, op, pay):
        out = super().op_reencode(op, pay)
        if op["form"] == "pool":
            out["parity"][-1] = 0  # (what the scratch parity held)
        return out


class BurstReadSeesTheOldPool(Defective):
    """a read inside a burst sees the pool as it was before the preceding write of the burst"""

    def op_burst(self, op, pay):
        ops = op["ops"]
        real_run = self.run

        def run(sub, pz):
            at = next(i for i, x in enumerate(ops) if x is sub)
            if sub["op"] == "write":
                self.old = self.d.copy()
            if sub["op"] == "read" and at > 0 and ops[at - 1]["op"] == "write":
                now, self.d = self.d, self.old
                try:
                    return real_run(sub, pz)
                finally:
                    self.d = now
            return real_run(sub, pz)
        self.run = run
        try:
            return super().op_burst(op, pay)
        finally:
            del self.run


# ---- defects in the degraded and window writes ----
class StoresIntoAnAbsentBlock(Defective):
    """fastecc_update_batch_set stores the new row into an ABSENT data block"""

    def stores_data(self, form, absent):
        return True if form == "batch_set" else super().stores_data(form, absent)


class UpdatesAnAbsentParityBlock(Defective):
    """a _set form updates an absent parity block"""

    def store_parity(self, p, b, rows, lost, col0, width):
        super().store_parity(p, b, rows, (), col0, width)


class OldRowFromThePool(Defective):
    """an absent written block's old row is taken from the pool (garbage), not from a rebuild"""

    def rebuilt_rows(self, d, td, blocks, col0, width):
        return [d[b, i, col0:col0 + width].copy() for b, i in blocks]


class ParityOneColumnTooWide(Defective):
    """a window call writes width + 1 columns of the parity"""

    def store_parity(self, p, b, rows, lost, col0, width):
        super().store_parity(p, b, rows, lost, col0, width)
        if col0 + width < self.S:
            for q in range(self.m):
                if q not in lost:
                    p[b, q, col0 + width] ^= np.uint32(1)


class DataWindowShiftedRight(Defective):
    """the data store of a window call applies the window one column to the right"""

    def store_data(self, d, b, i, col0, width, row, form):
        if form in ("batch", "batch_set") and width < self.S:
            n = min(width, self.S - col0 - 1)
            d[b, i, col0 + 1:col0 + 1 + n] = row[:n]
        else:
            super().store_data(d, b, i, col0, width, row, form)


class OldRowsAtTheEarlierWidth(Defective):
    """the second of two rebuilding writes reads its old rows from the reconstruction buffer at the first one's pitch"""
    pitch = None

    def rebuilt_rows(self, d, td, blocks, col0, width):
        rows = super().rebuilt_rows(d, td, blocks, col0, width)
        if rows and self.pitch not in (None, width):
            flat = np.concatenate(rows + [np.zeros(len(rows) * self.pitch + width, np.uint32)])
            rows = [flat[r * self.pitch:r * self.pitch + width].copy() for r in range(len(rows))]
        if rows:
            self.pitch = width
        return rows


class WritesUnderTheOldSet(Defective):
    """a degraded write after a second decode_prepare_set still uses the first set (the write_after_prepare_set probe)"""

    def swap_pattern(self, op, half):
        first = op["halves"][0]
        return tuple(first["patterns"][first["q"]])


class BurstReadAnswersTheNextRebuildList(Defective):
    """a read of a burst answers the requests of the following write's rebuild list: the staged list is shared"""

    def op_burst(self, op, pay):
        ops, real_run = op["ops"], self.run

        def run(sub, pz):
            at = next(i for i, x in enumerate(ops) if x is sub)
            nxt = ops[at + 1] if at + 1 < len(ops) else None
            if sub["op"] == "read" and nxt and nxt["op"] == "write" and nxt["form"] == "batch_set":
                rebuilt = [w for w in nxt["writes"] if w % self.k in self.prepared_set[nxt["pattern_of"][w // self.k]]]
                sub = dict(sub, reads=(rebuilt + sub["reads"][len(rebuilt):])[:len(sub["reads"])])
            return real_run(sub, pz)
        self.run = run
        try:
            return super().op_burst(op, pay)
        finally:
            del self.run


class ParityFormStoresData(Defective):
    """a parity form stores data: the window of an absent data block that only its caller may hold"""

    def stores_data(self, form, absent):
        return True if form in ("parity", "parity_set") else super().stores_data(form, absent)


class TouchesAnIgnoredStripe(Defective):
    """a _set form touches a stripe whose pattern_of entry it should have ignored (no write names it)"""

    def op_write(self, op, pay):
        out = super().op_write(op, pay)
        if op.get("ignored") is not None:
            self.p[op["ignored"], 0, 0] ^= np.uint32(1)
        return out


DEG_DEFECTS = [StoresIntoAnAbsentBlock, UpdatesAnAbsentParityBlock, OldRowFromThePool, ParityOneColumnTooWide, DataWindowShiftedRight,
               OldRowsAtTheEarlierWidth, WritesUnderTheOldSet, BurstReadAnswersTheNextRebuildList, ParityFormStoresData, TouchesAnIgnoredStripe]
EXT_DEFECTS = [CopiesLostBlocks, ReadsUnderTheOldPattern, ReadWritesPastItsRows, ReadWritesThePool, ShiftedSetLocation, PoolEncodeSkipsTheLastStripe,
               BurstReadSeesTheOldPool]
DEFECTS = [SkipsAParityBlock, TouchesAnotherStripe, ShiftedPatterns, RewritesAbsentBlocks, ReadsQuarantined, SetClobbersPrepared, StaleChunking]
DEFECT_CONFIGS = ("20_16_s64_fixed", "20_16_s64_rotated", "64_32_rotated", "32_8_fixed")


@pytest.mark.parametrize("defect", DEFECTS + EXT_DEFECTS + DEG_DEFECTS, ids=[d.__name__ for d in DEFECTS + EXT_DEFECTS + DEG_DEFECTS])
def test_injected_defect_is_reported_at_its_step(oracle, defect):
    caught = 0
    extended = defect in EXT_DEFECTS  # a defect of the extended operations is looked for in the extended sequences
    degraded = defect in DEG_DEFECTS  # ... one of the degraded and window writes in the degraded sequences
    for name, seed in itertools.product(DEFECT_CONFIGS, pm.DEG_SEEDS if degraded else pm.EXT_SEEDS if extended else pm.SEEDS):
        cfg = pm.config_named(name)
        backend = defect(cfg, oracle)
        try:
            pm.run_sequence(backend, cfg, seed, oracle=oracle, extended=extended, degraded=degraded)
        except pm.SequenceFailure as e:
            assert backend.fired == e.step, (name, seed, backend.fired, e.step)
            text = str(e)
            assert cfg.name in text and "seed %d" % seed in text and "step %d" % e.step in text
            assert len(e.log) == e.step + 1 and all(line in text for line in e.log)  # the operation log up to that step
            assert "steps=%d" % (e.step + 1) in text                                   # ... and how to replay it
            assert ("degraded=True" in text) == degraded and ("extended=True" in text) == extended  # ... under the flag of its family
            caught += 1
        else:
            assert backend.fired is None, (name, seed, backend.fired)  # the defect changed something and no step noticed
    assert caught >= 2, "no committed seed meets this defect: the generator is too weak"
