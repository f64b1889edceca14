"""Error location (fastecc_verify / _locate_errors / _correct): the host-side pieces, no GPU.

Berlekamp-Massey is checked against locators built in Python integers: power-sum syndromes s_i = sum_u Y_u X_u^i of random
error positions must give back Lambda(x) = prod (1 - X_u x) exactly."""
import ctypes
import random

import pytest

import fastecc_amd as fe

P = fe.P


@pytest.fixture(scope="module")
def hip_lib():
    return fe.lib()


def test_scrub_symbols_exported(hip_lib):
    for name in ("fastecc_verify", "fastecc_locate_errors", "fastecc_correct", "fastecc_gf_berlekamp_massey", "fastecc_scrub_fingerprints"):
        assert hasattr(hip_lib, name), name
    assert fe.E_UNCORRECTABLE == -5
    assert hip_lib.fastecc_version() >= 300


def test_strerror_uncorrectable(hip_lib):
    text = hip_lib.fastecc_strerror(fe.E_UNCORRECTABLE).decode()
    assert text and text != "unknown error"
    assert text != hip_lib.fastecc_strerror(fe.E_UNSUPPORTED).decode()


def test_scrub_argument_validation_without_device(hip_lib):
    """Null context / pointers and misaligned buffers are refused before any device work."""
    vp = ctypes.c_void_p
    ok = ctypes.c_int(7)
    cnt = ctypes.c_uint64(7)
    out = (ctypes.c_uint64 * 4)()
    buf = (ctypes.c_uint32 * 64)()
    a = ctypes.addressof(buf)
    assert hip_lib.fastecc_verify(None, a, a, fe.MEM_DEVICE, None, 0, ctypes.byref(ok)) == fe.E_INVAL
    assert hip_lib.fastecc_locate_errors(None, a, a, fe.MEM_DEVICE, None, 0, out, 4, ctypes.byref(cnt)) == fe.E_INVAL
    assert hip_lib.fastecc_correct(None, a, a, fe.MEM_DEVICE, None, 0, out, 4, ctypes.byref(cnt)) == fe.E_INVAL
    fake = vp(a)  # never dereferenced: every check below fails before the context is read
    assert hip_lib.fastecc_verify(fake, a, a, fe.MEM_DEVICE, None, 0, None) == fe.E_INVAL
    assert hip_lib.fastecc_locate_errors(fake, a, a, fe.MEM_DEVICE, None, 0, out, 4, None) == fe.E_INVAL
    assert hip_lib.fastecc_correct(fake, a, a, fe.MEM_DEVICE, None, 0, None, 4, ctypes.byref(cnt)) == fe.E_INVAL
    assert hip_lib.fastecc_verify(fake, a + 2, a, fe.MEM_DEVICE, None, 0, ctypes.byref(ok)) == fe.E_INVAL  # misaligned data
    assert hip_lib.fastecc_locate_errors(fake, a, a + 1, fe.MEM_DEVICE, None, 0, out, 4, ctypes.byref(cnt)) == fe.E_INVAL
    assert hip_lib.fastecc_correct(fake, None, a, fe.MEM_DEVICE, None, 0, out, 4, ctypes.byref(cnt)) == fe.E_INVAL
    assert ok.value == 7 and cnt.value == 7


def _synd(positions, values, count):
    return [sum(y * pow(x, i, P) for x, y in zip(positions, values)) % P for i in range(count)]


def _locator(xs):
    lam = [1]
    for x in xs:  # times (1 - x z)
        nxt = lam + [0]
        for i, c in enumerate(lam):
            nxt[i + 1] = (nxt[i + 1] - c * x) % P
        lam = nxt
    return lam


@pytest.mark.parametrize("degree", [1, 2, 3, 5, 8, 16, 31, 64])
def test_berlekamp_massey_recovers_locator(degree):
    rng = random.Random(degree)
    w = fe.gf_root(1 << 20)
    for _ in range(3):
        us = rng.sample(range(1 << 20), degree)
        xs = [pow(w, (1 << 20) - u, P) for u in us]  # X_u = w^(-u)
        ys = [rng.randrange(1, P) for _ in us]
        got = fe.gf_berlekamp_massey(_synd(xs, ys, 2 * degree + rng.randrange(0, 3)))
        assert got == _locator(xs)
        # its roots are the positions: Lambda(w^u) = 0
        for u in us:
            x = pow(w, u, P)
            assert sum(c * pow(x, i, P) for i, c in enumerate(got)) % P == 0


def test_berlekamp_massey_zero_and_cap(hip_lib):
    assert fe.gf_berlekamp_massey([0] * 10) == [1]
    assert fe.gf_berlekamp_massey([]) == [1]
    s = _synd([5, 7], [1, 1], 4)
    lam = (ctypes.c_uint32 * 2)()
    arr = (ctypes.c_uint32 * 4)(*s)
    assert hip_lib.fastecc_gf_berlekamp_massey(arr, 4, lam, 2) == fe.E_INVAL  # degree 2 needs 3 words
    assert hip_lib.fastecc_gf_berlekamp_massey(None, 4, lam, 2) == fe.E_INVAL
    assert hip_lib.fastecc_gf_berlekamp_massey(arr, 4, None, 2) == fe.E_INVAL
