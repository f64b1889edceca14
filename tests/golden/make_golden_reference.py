"""Record tests/golden/golden_reference.json: what the UNMODIFIED reference (oracle/_ref) returns for the inputs the tests give it.

Run where the reference is built (oracle.build() compiles oracle/_ref when the reference sources are present):
    python tests/golden/make_golden_reference.py
The output is committed; the tests replay it through conftest.RecordedReference and need no reference build.

The CPU tests of tests/test_oracle.py that take the `reference` fixture are run here as they are, with a recorder in place of the
replay: every call goes to the live reference and is recorded (so the oracle is checked against the live reference on the way).  The
GPU tests' calls are made here with the same inputs as in those tests, without a GPU.
"""
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, ROOT)
sys.path.insert(0, TESTS)
from oracle import Oracle, Reference  # noqa: E402


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(TESTS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


conftest = _load("conftest")
RecordedReference = conftest.RecordedReference


class Recorder(RecordedReference):
    """RecordedReference's calls answered by the live reference builds, every answer recorded."""

    def __init__(self, rec, live, avx2=False):
        super().__init__(rec, avx2)
        self.live = live

    def variant(self, avx2):
        return Recorder(self.rec, self.live, avx2)

    def _scalar(self, name, *args):
        v = int(getattr(self.live["scalar"], name)(*args))
        self.rec["scalars"][self.scalar_key(name, *args)] = v
        return v

    def _array(self, name, x, *params):
        ref = self.live[self.build]
        x = np.ascontiguousarray(x, dtype=np.uint32)
        if name == "encode_rows":
            step, count = params
            out = ref.encode(x)[::step][:count]
        elif name == "small_ntt_columns":
            out = np.stack([ref.small_ntt(x[:, c], *params) for c in range(x.shape[1])], axis=1)
        else:
            out = getattr(ref, name)(x, *params)
        key = self.array_key(self.build, name, x, *params)
        if np.isscalar(out) or isinstance(out, int):
            self.rec["arrays"][key] = {"value": int(out)}
            return int(out)
        out = np.ascontiguousarray(out, dtype=np.uint32)
        if out.size <= self.WHOLE_WORDS:
            self.rec["arrays"][key] = {"shape": list(out.shape), "words": out.reshape(-1).tolist()}
        else:
            self.rec["arrays"][key] = {"shape": list(out.shape), "sha256": self.sha256(out)}
        return out


def params(fn):
    """The parameter sets of a test function's single @pytest.mark.parametrize."""
    (mark,) = [m for m in fn.pytestmark if m.name == "parametrize"]
    return mark.args[1]


def main():
    live = {"scalar": Reference(), "avx2": Reference(avx2=True)}
    rec = {"generated_by": "tests/golden/make_golden_reference.py", "scalars": {}, "arrays": {}}
    ref = Recorder(rec, live)
    orc = Oracle()

    # CPU: the tests themselves, the live reference behind the recorder
    t = _load("test_oracle")
    t.test_field_ops_against_reference(orc, ref)
    t.test_oracle_against_reference_encode(orc, ref)
    for n in params(t.test_mixed_radix_is_pinned_to_the_reference):
        t.test_mixed_radix_is_pinned_to_the_reference(orc, ref, n)
    t.test_reference_codelets_of_order_3_and_9(orc, ref)
    t.test_reference_codelets_of_order_2_and_4(orc, ref)

    # GPU tests: the same inputs, the reference's side only
    par = _load("test_gpu_parity")
    for log2n, S, avx2 in params(par.test_encode_equals_unmodified_reference):
        ref.variant(avx2).encode(par.rand_stripe(np.random.default_rng(log2n + S), 1 << log2n, S))
    for log2n, S in params(par.test_ntt_equals_unmodified_reference):
        x = par.rand_stripe(np.random.default_rng(log2n), 1 << log2n, S)
        for inverse in (False, True):
            for which in (Reference.MFA, Reference.REC):
                ref.ntt(x, inverse, which)
    for order in params(par.test_ntt_of_order_2_and_4_equals_the_reference_codelets):
        for S in (1, 33, 1024):
            x = par.rand_stripe(np.random.default_rng(100 * order + S), order, S)
            x[:, 0] = np.array([0, par.P - 1, 1, par.P - 2], dtype=np.uint32)[:order]
            for inverse in (False, True):
                ref.small_ntt_columns(x, inverse)
    fold = _load("test_gpu_fold")
    N = 1 << 11
    ref.encode_rows(fold.stripe(5, N, 513), 4, N // 4)
    k, m, S = 3000, 1000, 64
    x = np.random.default_rng(2).integers(0, par.P, size=(k, S), dtype=np.uint64).astype(np.uint32)
    padded = np.zeros((4096, S), dtype=np.uint32)
    padded[:k] = x
    ref.encode_rows(padded, 4, m)

    with open(os.path.join(HERE, "golden_reference.json"), "w") as f:
        json.dump(rec, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("%d scalars, %d arrays" % (len(rec["scalars"]), len(rec["arrays"])))


if __name__ == "__main__":
    main()
