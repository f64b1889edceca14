"""Writes pool_sequence_digests.json: for every (config, seed) of pool_model.CONFIGS x (pool_model.SEEDS + pool_model.EXT_SEEDS) the sha256 of the
sequence's operation log — the JSON lines pool_model.run_sequence builds, "%3d %s" % (step, operation), joined by newlines — on the exact numpy
backend (the seeds of EXT_SEEDS with extended=True).

The committed file was recorded in two steps: the 64 sequences of SEEDS on the commit BEFORE the generator learned the extended kinds (reads, set
location, whole-stripe writes), from the same lines rebuilt in an on_step callback; the 32 sequences of EXT_SEEDS on the commit BEFORE it learned
the degraded kinds (degraded writes, column-window writes: Generator(degraded=True)).
tests/test_pool_model_host.py::test_the_committed_sequences_are_unchanged recomputes all 96, so the file pins them.  Regenerate it only when a
change of those sequences is meant.

    python tests/golden/make_pool_sequence_digests.py"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import pool_model as pm  # noqa: E402
from oracle import Oracle  # noqa: E402


def main():
    oracle, out = Oracle(), {}
    for cfg in pm.CONFIGS:
        for seed in pm.SEEDS + pm.EXT_SEEDS:
            log = []
            pm.run_sequence(pm.ModelBackend(cfg, oracle), cfg, seed, oracle=oracle, extended=seed in pm.EXT_SEEDS, log=log)
            out["%s:%d" % (cfg.name, seed)] = hashlib.sha256("\n".join(log).encode()).hexdigest()
    with open(os.path.join(HERE, "pool_sequence_digests.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
