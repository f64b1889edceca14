"""Absent blocks per stripe (fastecc_scrub_erasures_set, fastecc_verify_batch_set / _correct_batch_set): argument checks that need no GPU.

Every refusal here happens before any device is touched: a null context, null pointers, a null pattern_of, count == 0 and misaligned
pointers are FASTECC_E_INVAL, and the Python methods reject a bad `count`, `pattern_of` or flag shape before the library is called."""
import ctypes

import numpy as np
import pytest

import fastecc_amd as fe


@pytest.fixture(scope="module")
def hip_lib():
    return fe.lib()


BATCH = ("fastecc_verify_batch_set", "fastecc_correct_batch_set")


def test_symbols_exported(hip_lib):
    for name in BATCH + ("fastecc_scrub_erasures_set",):
        assert hasattr(hip_lib, name), name
    assert hip_lib.fastecc_version() >= 380
    assert fe.PATTERN_NONE == 0xFFFFFFFF


def test_erasures_set_null_arguments_are_inval(hip_lib):
    fn = hip_lib.fastecc_scrub_erasures_set
    flags = (ctypes.c_uint8 * 64)(*([1] * 64))
    assert fn(None, flags, flags, 1) == fe.E_INVAL  # no context
    assert fn(None, None, None, 0) == fe.E_INVAL
    assert fn(None, None, None, 1) == fe.E_INVAL


@pytest.mark.parametrize("name", BATCH)
def test_null_arguments_are_inval(hip_lib, name):
    fn = getattr(hip_lib, name)
    buf = (ctypes.c_uint32 * 64)()
    a = ctypes.addressof(buf)
    po = (ctypes.c_uint32 * 4)(0, 0, 0, 0)
    out = (ctypes.c_uint8 * 4)(7, 7, 7, 7)
    bad = ctypes.c_uint64(99)
    nb = ctypes.byref(bad)
    assert fn(None, a, a, 1, po, None, 0, out, nb) == fe.E_INVAL       # no context
    assert fn(None, None, None, 0, None, None, 0, None, None) == fe.E_INVAL
    assert fn(None, a, a, 1, None, None, 0, out, nb) == fe.E_INVAL     # no pattern_of
    assert fn(None, None, a, 1, po, None, 0, out, nb) == fe.E_INVAL    # no data
    assert fn(None, a, None, 1, po, None, 0, out, nb) == fe.E_INVAL    # no parity
    assert fn(None, a, a, 1, po, None, 0, None, nb) == fe.E_INVAL      # no consistent / status
    assert fn(None, a, a, 1, po, None, 0, out, None) == fe.E_INVAL     # no inconsistent
    assert fn(None, a, a, 0, po, None, 0, out, nb) == fe.E_INVAL       # count 0
    assert fn(None, a + 2, a, 1, po, None, 0, out, nb) == fe.E_INVAL   # misaligned
    assert fn(None, a, a + 1, 1, po, None, 0, out, nb) == fe.E_INVAL
    assert list(out) == [7, 7, 7, 7] and bad.value == 99               # a refused call writes nothing


def _shell(n=6, k=4):
    """an Encoder object without a context (no device is needed to reach the argument checks)"""
    enc = fe.Encoder.__new__(fe.Encoder)
    enc._h = ctypes.c_void_p()
    enc.n, enc.k = n, k
    return enc


@pytest.mark.parametrize("method", ["verify_batch_set", "correct_batch_set"])
def test_python_methods_validate_count_and_pattern_of(hip_lib, method):
    fn = getattr(_shell(), method)
    for bad in (0, -1, 1 << 64):
        with pytest.raises(ValueError):
            fn(0, 0, bad, [0])
    for bad in (1.0, "3", None, True):
        with pytest.raises(TypeError):
            fn(0, 0, bad, [0])
    for bad in ([], [0, 1, 2], np.zeros(1, np.uint32)):  # not one entry per stripe
        with pytest.raises(ValueError):
            fn(0, 0, 2, bad)
    for bad in ([-1, 0], [0, 1 << 32]):  # not a uint32
        with pytest.raises(ValueError):
            fn(0, 0, 2, bad)
    for good in ([0, fe.PATTERN_NONE], np.array([1, 0], np.uint32), np.array([1, 0], np.int64)):
        with pytest.raises(fe.FastEccError) as e:  # valid arguments reach the library, which refuses the null context
            fn(0, 0, 2, good, seed=5)
        assert e.value.code == fe.E_INVAL


def test_python_erasures_set_validates_shapes(hip_lib):
    enc = _shell(6, 4)
    with pytest.raises(ValueError):
        enc.scrub_erasures_set([[1, 1, 1, 1]], [])                      # P differs
    with pytest.raises(ValueError):
        enc.scrub_erasures_set([[1, 1, 1]], [[1, 1]])                   # k - 1 data flags
    with pytest.raises(ValueError):
        enc.scrub_erasures_set(np.ones((2, 4), np.uint8), np.ones((2, 3), np.uint8))  # n - k + 1 parity flags
    for good in (([[1, 0, 1, 1]], [[1, 1]]), (np.ones((3, 4), np.uint8), np.ones((3, 2), np.uint8)), ([], [])):
        with pytest.raises(fe.FastEccError) as e:  # the library refuses the null context
            enc.scrub_erasures_set(*good)
        assert e.value.code == fe.E_INVAL
