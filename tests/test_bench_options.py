"""bench.py's command line (a plain run measures the headline only; --full adds the rest) and what --dump-outputs writes, on CPU tensors."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_options_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _parse(bench, argv):
    saved, sys.argv = sys.argv, ["bench.py"] + argv
    try:
        return bench.parse()
    finally:
        sys.argv = saved


def test_full_is_off_by_default():
    bench = _bench()
    a = _parse(bench, ["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = _parse(bench, ["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_dump_whole_parity_is_exact_float64(tmp_path):
    bench = _bench()
    words = np.array([0, 1, 0xFFF00000, 0x80000000, 12345, 0xFFEFFFFF, 7, 9], dtype=np.uint32)
    parity = torch.from_numpy(words.view(np.int32).copy())
    rec = bench.dump_outputs(str(tmp_path), parity, 16, p61=False)
    got = np.load(tmp_path / "parity.npy")
    assert got.dtype == np.float64 and got.shape == (2, 4) and rec["sampled"] is False
    assert np.array_equal(got.reshape(-1).astype(np.uint64), words.astype(np.uint64))
    assert not (tmp_path / "parity_index.npy").exists()


def test_dump_samples_a_large_parity_the_same_way_every_time(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_BYTES", 8 * 1000)
    words = np.random.default_rng(3).integers(0, 0xFFF00001, size=1 << 16, dtype=np.uint64).astype(np.uint32)
    parity = torch.from_numpy(words.view(np.int32).copy())
    runs = []
    for d in ("a", "b"):
        rec = bench.dump_outputs(str(tmp_path / d), parity, 4096, p61=False)
        got, idx = np.load(tmp_path / d / "parity.npy"), np.load(tmp_path / d / "parity_index.npy")
        assert rec["sampled"] is True and got.nbytes <= 8 * 1000 and got.dtype == np.float64
        assert np.array_equal(got, words[idx.astype(np.int64)].astype(np.float64))
        runs.append((got, idx))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


def test_dump_64bit_field_words_as_two_exact_halves(tmp_path):
    bench = _bench()
    words = np.array([(1 << 61) - 2, 0, 1, (1 << 40) + 5], dtype=np.uint64)
    parity = torch.from_numpy(words.view(np.int64).copy())
    bench.dump_outputs(str(tmp_path), parity, 16, p61=True)
    got = np.load(tmp_path / "parity.npy")
    assert got.shape == (2, 2, 2) and got.dtype == np.float64
    flat = got.reshape(-1, 2).astype(np.uint64)
    assert np.array_equal(flat[:, 0] + (flat[:, 1] << np.uint64(32)), words)
