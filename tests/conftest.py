import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")

# The CPU checkers (oracle/, oracle/_ref) are OpenMP code and most tests call them on tiny stripes.  A team as wide
# as the host (128+ threads on the GPU boxes) makes every such call pay for a full-machine barrier, and when the
# box's CPUs are shared or quota-limited that cost explodes (seconds per call).  A moderate, fixed team keeps the
# suite's run time predictable; it has to be set before libgomp is loaded.
os.environ.setdefault("OMP_NUM_THREADS", "16")
os.environ.setdefault("OMP_WAIT_POLICY", "passive")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def oracle():
    from oracle import Oracle
    return Oracle()


class RecordedReference:
    """What the unmodified reference (oracle/_ref) returned for the inputs the tests give it, recorded by tests/golden/make_golden_reference.py
    into tests/golden/golden_reference.json, so that the tests do not depend on a reference build.  The calls are those of oracle.Reference;
    an array result comes back whole when it was recorded whole (at most WHOLE_WORDS words) and as a Digest (its shape and sha256)
    otherwise: compare results with agrees().  A call the recording does not hold raises KeyError: the inputs have drifted from the
    recording, so regenerate it where the reference is."""
    MFA, REC, SLOW = 0, 1, 2
    WHOLE_WORDS = 1024

    class Digest:
        def __init__(self, shape, sha256):
            self.shape, self.sha256 = tuple(shape), sha256

    def __init__(self, rec, avx2=False):
        self.rec, self.build = rec, "avx2" if avx2 else "scalar"

    def variant(self, avx2):
        """The same recording seen through the AVX2 (or the scalar) build of the reference."""
        return RecordedReference(self.rec, avx2)

    @staticmethod
    def array_key(build, name, x, *params):
        a = np.ascontiguousarray(x, dtype=np.uint32)
        h = hashlib.sha256(("%s %s %r %r " % (build, name, params, a.shape)).encode())
        h.update(a.tobytes())
        return h.hexdigest()[:32]

    @staticmethod
    def scalar_key(name, *args):
        return " ".join([name] + [str(int(v)) for v in args])

    @staticmethod
    def sha256(a):
        return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint32).tobytes()).hexdigest()

    def agrees(self, got, want):
        got = np.asarray(got)
        if isinstance(want, RecordedReference.Digest):
            return got.shape == want.shape and got.dtype == np.uint32 and self.sha256(got) == want.sha256
        return np.array_equal(got, want)

    def _scalar(self, name, *args):
        return self.rec["scalars"][self.scalar_key(name, *args)]

    def _array(self, name, x, *params):
        r = self.rec["arrays"][self.array_key(self.build, name, x, *params)]
        if "value" in r:
            return r["value"]
        if "words" in r:
            return np.array(r["words"], dtype=np.uint32).reshape(r["shape"])
        return RecordedReference.Digest(r["shape"], r["sha256"])

    def gf_add(self, x, y): return self._scalar("gf_add", x, y)
    def gf_sub(self, x, y): return self._scalar("gf_sub", x, y)
    def gf_mul(self, x, y): return self._scalar("gf_mul", x, y)
    def gf_root(self, n): return self._scalar("gf_root", n)
    def gf_inv(self, x): return self._scalar("gf_inv", x)
    def hash(self, data): return self._array("hash", data)
    def ntt(self, data, inverse=False, which=0): return self._array("ntt", data, bool(inverse), which)
    def encode(self, data): return self._array("encode", data)
    def small_ntt(self, f, inverse=False): return self._array("small_ntt", f, bool(inverse))

    def encode_rows(self, data, step, count):
        """Parity blocks [::step][:count] of the reference's encode of `data`."""
        return self._array("encode_rows", data, step, count)

    def small_ntt_columns(self, x, inverse=False):
        """The reference's order-2 / order-4 codelet on every column of x ([order, S])."""
        return self._array("small_ntt_columns", x, bool(inverse))


@pytest.fixture(scope="session")
def reference():
    """The unmodified reference's results, replayed from tests/golden/golden_reference.json (RecordedReference)."""
    with open(os.path.join(GOLDEN, "golden_reference.json")) as f:
        return RecordedReference(json.load(f))


@pytest.fixture(scope="session")
def golden_hashes():
    with open(os.path.join(GOLDEN, "golden_hashes.json")) as f:
        return json.load(f)


@pytest.fixture(scope="session")
def golden_vectors():
    return dict(np.load(os.path.join(GOLDEN, "golden_vectors.npz")))


@pytest.fixture(scope="session")
def hip_lib():
    """Builds (if stale) and loads libfastecc_hip.so."""
    import __graft_entry__ as ge
    ge.build()
    import fastecc_amd
    return fastecc_amd.lib()
