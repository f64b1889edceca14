"""GPU test (-m gpu): the rotated configuration's long sequence of tests/pool_model.py with profiling on reaches the batched location and the
grouped repair of fastecc_correct_batch_set.

tests/test_gpu_pool_sequences.py compares every step of the same sequences with the CPU model byte for byte, whatever path a step takes; this
test adds that the new path is among the ones taken: "fingerprint_set_list" and "direct_pass_set" appear in a `correct` step whose
"correct_batch_mode" is not 2, and "fingerprint_set_list" in none whose mode is 2.  The sequence is seed 4's: its grouped `correct` steps come
while option "decode_batch_kernel" is not 2 (in seed 11's, the one test_gpu_pool_sequences.py profiles, the only grouped step follows a
repair step that left the option at 2, so the private set's passes run stripe by stripe there, as that option asks)."""
import pytest

import pool_model as pm

pytestmark = pytest.mark.gpu

LONG_STEPS = 150
SEED = 4
GROUPED_SCOPES = ("fingerprint_set_list", "direct_pass_set")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def fe(hip_lib):
    import fastecc_amd
    return fastecc_amd


def test_grouped_set_path_ran(torch_cuda, fe, oracle):
    cfg = pm.config_named("20_16_s64_rotated")
    backend = pm.GpuBackend(fe, torch_cuda, cfg, profile=True)
    ops = {}
    try:
        pm.run_sequence(backend, cfg, SEED, steps=LONG_STEPS, oracle=oracle, on_step=lambda step, op: ops.__setitem__(step, op))
    finally:
        backend.close()
    corrects = {step: op for step, op in ops.items() if op.get("op") == "correct" and op.get("set")}
    assert corrects, "the sequence drew no correct step on the rotated pool"
    grouped = [step for step, op in corrects.items() if op["mode"] != 2 and all(x in backend.scopes.get(step, ()) for x in GROUPED_SCOPES)]
    assert grouped, {step: (op["mode"], sorted(backend.scopes.get(step, ()))) for step, op in corrects.items()}
    for step, op in corrects.items():
        if op["mode"] == 2:
            assert "fingerprint_set_list" not in backend.scopes.get(step, ()), (step, sorted(backend.scopes[step]))
