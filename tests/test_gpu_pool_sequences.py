"""GPU tests (-m gpu): seeded sequences of pool operations on ONE long-lived context against the CPU model of tests/pool_model.py.

Writes (fastecc_update_batch, _update_parity_batch, fastecc_update), silent corruption, devices going down and coming back, verify, locate,
correct, repair, decode, re-encode, option and stream flips, sub-range calls and the state probes of pool_model's docstring follow one another
as the generator draws them — in the extended sequences (the seeds pool_model.EXT_SEEDS) degraded reads (fastecc_read_batch, _read_batch_set)
alone and inside bursts, location under the pattern set (fastecc_locate_errors_batch_set) and whole-stripe writes and re-encodes
(fastecc_encode_pool under every "encode_pool_kernel") as well; in the degraded sequences (the seeds pool_model.DEG_SEEDS) the writes go on while
devices are down (fastecc_update_batch_set, _update_parity_batch_set: absent blocks written, rebuilt rows, bursts that put a read beside such a
write and two such writes of different widths on different streams) and the four pool forms take column windows (the fastecc_update_*_window
calls); after every step every host output equals the model's prediction and the
whole pool, data and parity, quarantined stripes included, equals the model's mirror bit for bit.  The model's parity is the oracle's; no comparison here uses the library as its own
reference, and none has a tolerance.  A failure names the configuration, the seed, the step and the operations so far;
pool_model.run_sequence(backend, config, seed, steps=N) replays the prefix (with extended=True for an extended sequence, degraded=True for a degraded one: the message says so)."""
import pytest

import pool_model as pm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def fe(hip_lib):
    import fastecc_amd
    return fastecc_amd


CASES = [(cfg.name, seed) for cfg in pm.CONFIGS for seed in pm.SEEDS]
EXT_CASES = [(cfg.name, seed) for cfg in pm.CONFIGS for seed in pm.EXT_SEEDS]
DEG_CASES = [(cfg.name, seed) for cfg in pm.CONFIGS for seed in pm.DEG_SEEDS]


@pytest.mark.parametrize("name,seed", CASES + EXT_CASES + DEG_CASES)
def test_sequence(torch_cuda, fe, oracle, name, seed):
    cfg = pm.config_named(name)
    backend = pm.GpuBackend(fe, torch_cuda, cfg)
    try:
        pm.run_sequence(backend, cfg, seed, oracle=oracle, extended=seed in pm.EXT_SEEDS, degraded=seed in pm.DEG_SEEDS)
    finally:
        backend.close()


BATCHED_SCOPES = ("update_batch", "update_scatter", "fingerprint_batch", "fingerprint_batch_list", "fingerprint_set", "scrub_syndromes_set",
                  "scrub_root_search_batch", "direct_pass_set")
LONG_STEPS = 150


def test_batched_kernels_ran(torch_cuda, fe, oracle):
    """One long sequence per placement with profiling on: the batched kernels ran, not only their per-stripe fallbacks, and direct passes ran
    in steps that did not ask for the stripe-by-stripe mode."""
    seen, free_direct = set(), False
    for name in ("20_16_s64_fixed", "20_16_s64_rotated"):
        cfg = pm.config_named(name)
        backend = pm.GpuBackend(fe, torch_cuda, cfg, profile=True)
        ops = {}
        try:
            pm.run_sequence(backend, cfg, 11, steps=LONG_STEPS, oracle=oracle, on_step=lambda step, op: ops.__setitem__(step, op))
        finally:
            backend.close()
        for step, names in backend.scopes.items():
            seen |= names
            by_stripe = ops[step].get("kernel") == 2 or ops[step].get("mode") == 2
            if any(x.startswith("direct_pass") for x in names) and not by_stripe:
                free_direct = True
    missing = [x for x in BATCHED_SCOPES if x not in seen]
    assert not missing, (missing, sorted(seen))
    assert "direct_pass_batch" in seen or "direct_pass_list" in seen, sorted(seen)
    assert free_direct, "only the steps that asked for mode 2 ran a direct pass"


EXTENDED_SCOPES = ("direct_read", "direct_read_set", "fingerprint_set_list", "encode_pool_valu", "encode_pool_mfma")


def test_extended_kernels_ran(torch_cuda, fe, oracle):
    """One long extended sequence per placement with profiling on: the read kernel ran in both forms, the set location ran its list pass, and the
    pool encode ran as one launch under both kernels (an even block of 64 words: the matrix-core kernel can run)."""
    seen = set()
    for name in ("20_16_s64_fixed", "20_16_s64_rotated"):
        cfg = pm.config_named(name)
        backend = pm.GpuBackend(fe, torch_cuda, cfg, profile=True)
        try:
            pm.run_sequence(backend, cfg, 11, steps=LONG_STEPS, oracle=oracle, extended=True)
        finally:
            backend.close()
        for names in backend.scopes.values():
            seen |= names
    missing = [x for x in EXTENDED_SCOPES if x not in seen]
    assert not missing, (missing, sorted(seen))


DEGRADED_SCOPES = ("update_set", "update_set_recon", "update_window", "update_window_recon", "update_window_scatter")


def test_degraded_kernels_ran(torch_cuda, fe, oracle):
    """One long degraded sequence per placement with profiling on: the set kernel and the window kernel ran, each with a reconstruction pass for
    absent written blocks, and the window scatter stored rows."""
    seen = set()
    for name in ("20_16_s64_fixed", "20_16_s64_rotated"):
        cfg = pm.config_named(name)
        backend = pm.GpuBackend(fe, torch_cuda, cfg, profile=True)
        try:
            pm.run_sequence(backend, cfg, 11, steps=LONG_STEPS, oracle=oracle, degraded=True)
        finally:
            backend.close()
        for names in backend.scopes.values():
            seen |= names
    missing = [x for x in DEGRADED_SCOPES if x not in seen]
    assert not missing, (missing, sorted(seen))
