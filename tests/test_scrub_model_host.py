"""The exact model of the scrub fingerprint pass (tests/scrub_model.py) against hand-computed cases, and the argument checks of the probe
fastecc_scrub_fingerprints that happen before any device work.  No GPU."""
import ctypes

import numpy as np
import pytest

import fastecc_amd as fe
import scrub_model as sm

P = sm.P
SEED = 0x5EED


@pytest.fixture(scope="module")
def hip_lib():
    return fe.lib()


def splitmix64_loop(seed, count):
    """The generator as its authors wrote it, one output at a time on Python integers."""
    M = (1 << 64) - 1
    out, s = [], seed
    for _ in range(count):
        s = (s + 0x9E3779B97F4A7C15) & M
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        out.append(z ^ (z >> 31))
    return out


def test_splitmix64_published_vectors():
    """The first outputs for the seeds 0 and 1234567 as published with the generator's reference code."""
    assert splitmix64_loop(0, 1) == [0xE220A8397B1DCDAF]
    assert splitmix64_loop(1234567, 5) == [6457827717110365317, 3203168211198807973, 9817491932198370423, 4593380528125082431, 16408922859458223821]


@pytest.mark.parametrize("seed", [0, 1, SEED, (1 << 64) - 1, 0xDEADBEEFCAFEF00D])
def test_weights_are_the_bit_fields_of_splitmix64(seed):
    S = 1000
    w = sm.weights(seed, S)
    assert w.shape == (S, 3) and w.dtype == np.uint64
    xs = splitmix64_loop(seed, S)
    assert [[int(v) for v in row] for row in w] == [[x & 0xFFFFF, (x >> 20) & 0xFFFFF, (x >> 40) & 0xFFFFF] for x in xs]
    assert np.array_equal(sm.weights(seed, 10), w[:10])  # a prefix: a shorter block has the same first weights


def test_fingerprints_hand_cases():
    S = 9
    w = sm.weights(SEED, S)
    rho = [[int(v) for v in row] for row in w]
    impulse = np.zeros((S, S), np.uint32)
    impulse[np.arange(S), np.arange(S)] = 1
    assert sm.fingerprints(impulse, SEED).tolist() == rho  # block e_i: F_c = rho_c[i]
    ones = np.ones(S, np.uint32)
    assert sm.fingerprints(ones, SEED).tolist() == [sum(r[c] for r in rho) % P for c in range(3)]
    top = np.full(S, P - 1, np.uint32)  # -1 everywhere: F_c = -sum rho_c
    assert sm.fingerprints(top, SEED).tolist() == [(-sum(r[c] for r in rho)) % P for c in range(3)]
    # words >= p enter as stored: p itself counts as 0, 2^32 - 1 as 2^32 - 1 - p
    big = np.array([P, 0xFFFFFFFF, 5] + [0] * (S - 3), np.uint32)
    assert sm.fingerprints(big, SEED).tolist() == [(rho[1][c] * (0xFFFFFFFF - P) + rho[2][c] * 5) % P for c in range(3)]
    # by the definition, on Python integers
    rng = np.random.default_rng(1)
    blk = rng.integers(0, 1 << 32, size=S, dtype=np.uint64).astype(np.uint32)
    assert sm.fingerprints(blk, SEED).tolist() == [sum(rho[i][c] * int(blk[i]) for i in range(S)) % P for c in range(3)]
    assert sm.fingerprints(blk, SEED, w).tolist() == sm.fingerprints(blk, SEED).tolist()


def test_fingerprints_are_linear():
    rng = np.random.default_rng(2)
    S = 777
    a = rng.integers(0, P, size=(3, S), dtype=np.uint64)
    b = rng.integers(0, P, size=(3, S), dtype=np.uint64)
    fa, fb = (sm.fingerprints(x.astype(np.uint32), SEED).astype(np.uint64) for x in (a, b))
    assert np.array_equal(sm.fingerprints(((a + b) % P).astype(np.uint32), SEED), (fa + fb) % P)
    for scalar in (2, P - 1, 0x12345678):
        scaled = np.array([[int(v) * scalar % P for v in row] for row in a], np.uint32)
        assert sm.fingerprints(scaled, SEED).tolist() == [[int(v) * scalar % P for v in row] for row in fa]


def test_lane_maps():
    assert [sm.lane_of(w, sm.VECTOR) for w in (0, 3, 4, 255, 256, 259, 260, 1023, 1024)] == [0, 0, 1, 63, 0, 0, 1, 63, 0]
    assert [sm.lane_of(w, sm.SCALAR) for w in (0, 1, 63, 64, 65, 4099)] == [0, 1, 63, 0, 1, 3]


@pytest.mark.parametrize("form,S", [(sm.VECTOR, 260), (sm.VECTOR, 2052), (sm.SCALAR, 65), (sm.SCALAR, 2051)])
def test_lane_sums_by_definition(form, S):
    rng = np.random.default_rng(S)
    blk = rng.integers(0, 1 << 32, size=S, dtype=np.uint64).astype(np.uint32)
    w = sm.weights(SEED, S)
    want = [[0, 0, 0] for _ in range(64)]
    for i in range(S):
        for c in range(3):
            want[sm.lane_of(i, form)][c] += int(w[i, c]) * int(blk[i])
    got = sm.lane_sums(blk, w, form)
    assert got == want
    assert [sum(lane[c] for lane in got) % P for c in range(3)] == sm.fingerprints(blk, SEED).tolist()


@pytest.mark.parametrize("form,S", [(sm.VECTOR, 786436), (sm.SCALAR, 786437)])
def test_saturated_long_block_needs_the_fold(form, S):
    """The input the GPU tests rely on to exercise the periodic fold: without it a lane's 64-bit sum wraps."""
    sums = sm.lane_sums(np.full(S, P - 1, np.uint32), sm.weights(SEED, S), form)
    assert max(max(lane) for lane in sums) >= 1 << 64
    # and the fold interval is safe: 4096 products on top of a folded sum stay below 2^64
    assert 4096 * ((1 << 32) - 1) * ((1 << 20) - 1) + (1 << 33) < 1 << 64


def test_probe_symbol_exported(hip_lib):
    assert hasattr(hip_lib, "fastecc_scrub_fingerprints")
    assert hasattr(fe.Encoder, "scrub_fingerprints")


def test_probe_argument_validation_without_device(hip_lib):
    """Null context, null out / big, an unknown form, form 0 with count != 1, a list that does not go with the form, count 0 and
    misaligned buffers are refused before any device work."""
    vp = ctypes.c_void_p
    buf = (ctypes.c_uint32 * 64)()
    a = ctypes.addressof(buf)
    out = (ctypes.c_uint32 * 64)(*([7] * 64))
    big = (ctypes.c_uint8 * 4)(*([7] * 4))
    lst = (ctypes.c_uint64 * 2)(0, 1)
    call = hip_lib.fastecc_scrub_fingerprints
    for form, count, l in ((0, 1, None), (1, 2, None), (2, 2, lst)):
        assert call(None, a, a, count, l, form, None, SEED, out, big) == fe.E_INVAL
    fake = vp(a)  # never dereferenced: every check below fails before the context is read
    assert call(fake, a, a, 1, None, 0, None, SEED, None, big) == fe.E_INVAL
    assert call(fake, a, a, 1, None, 0, None, SEED, out, None) == fe.E_INVAL
    for form in (-1, 3, 99):
        assert call(fake, a, a, 1, None, form, None, SEED, out, big) == fe.E_INVAL
    assert call(fake, a, a, 2, None, 0, None, SEED, out, big) == fe.E_INVAL  # form 0 is one stripe
    assert call(fake, a, a, 0, None, 0, None, SEED, out, big) == fe.E_INVAL
    assert call(fake, a, a, 1, lst, 0, None, SEED, out, big) == fe.E_INVAL   # a list without the list form
    assert call(fake, a, a, 2, lst, 1, None, SEED, out, big) == fe.E_INVAL
    assert call(fake, a, a, 2, None, 2, None, SEED, out, big) == fe.E_INVAL  # the list form without a list
    assert call(fake, a, a, 0, None, 1, None, SEED, out, big) == fe.E_INVAL  # an empty batch
    assert call(fake, None, a, 1, None, 0, None, SEED, out, big) == fe.E_INVAL
    assert call(fake, a, None, 2, None, 1, None, SEED, out, big) == fe.E_INVAL
    for form, count, l in ((0, 1, None), (1, 2, None), (2, 2, lst)):
        assert call(fake, a + 2, a, count, l, form, None, SEED, out, big) == fe.E_INVAL  # misaligned data
        assert call(fake, a, a + 1, count, l, form, None, SEED, out, big) == fe.E_INVAL  # misaligned parity
    assert list(out) == [7] * 64 and list(big) == [7] * 4
