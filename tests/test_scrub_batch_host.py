"""Batched scrub (fastecc_verify_batch / _correct_batch): argument checks that need no GPU.

Every refusal here happens before any device is touched: a null context, null pointers (the outputs included), count == 0 and
misaligned stripes are FASTECC_E_INVAL, and a refused call writes nothing."""
import ctypes

import pytest

import fastecc_amd as fe


@pytest.fixture(scope="module")
def hip_lib():
    return fe.lib()


NAMES = ("fastecc_verify_batch", "fastecc_correct_batch")


def test_symbols_exported(hip_lib):
    for name in NAMES:
        assert hasattr(hip_lib, name), name
    assert hip_lib.fastecc_version() >= 330


def _out(count=4):
    res = (ctypes.c_uint8 * count)(*([0xAB] * count))
    n = ctypes.c_uint64(0xDEAD)
    return res, n


@pytest.mark.parametrize("name", NAMES)
def test_invalid_arguments_are_inval(hip_lib, name):
    fn = getattr(hip_lib, name)
    buf = (ctypes.c_uint32 * 64)()
    a = ctypes.addressof(buf)
    res, n = _out()
    u8 = ctypes.cast(res, ctypes.POINTER(ctypes.c_uint8))
    assert fn(None, a, a, 1, None, 0, u8, ctypes.byref(n)) == fe.E_INVAL        # no context
    assert fn(None, None, a, 1, None, 0, u8, ctypes.byref(n)) == fe.E_INVAL     # no data
    assert fn(None, a, None, 1, None, 0, u8, ctypes.byref(n)) == fe.E_INVAL     # no parity
    assert fn(None, a, a, 0, None, 0, u8, ctypes.byref(n)) == fe.E_INVAL        # count 0
    assert fn(None, a + 2, a, 1, None, 0, u8, ctypes.byref(n)) == fe.E_INVAL    # misaligned data
    assert fn(None, a, a + 1, 1, None, 0, u8, ctypes.byref(n)) == fe.E_INVAL    # misaligned parity
    assert fn(None, a, a, (1 << 64) - 1, None, 0, u8, ctypes.byref(n)) == fe.E_INVAL  # (no context to size it: refused all the same)
    assert list(res) == [0xAB] * 4 and n.value == 0xDEAD                       # a refused call writes nothing


@pytest.mark.parametrize("name", NAMES)
def test_null_outputs_are_inval(hip_lib, name):
    fn = getattr(hip_lib, name)
    buf = (ctypes.c_uint32 * 64)()
    a = ctypes.addressof(buf)
    res, n = _out()
    u8 = ctypes.cast(res, ctypes.POINTER(ctypes.c_uint8))
    assert fn(None, a, a, 1, None, 0, None, ctypes.byref(n)) == fe.E_INVAL     # no consistent / status array
    assert fn(None, a, a, 1, None, 0, u8, None) == fe.E_INVAL                  # no inconsistent count
    assert list(res) == [0xAB] * 4 and n.value == 0xDEAD


def _shell():
    """an Encoder object without a context (no device is needed to reach the argument checks)"""
    enc = fe.Encoder.__new__(fe.Encoder)
    enc._h = ctypes.c_void_p()
    return enc


@pytest.mark.parametrize("method", ["verify_batch", "correct_batch"])
def test_python_methods_validate_count(hip_lib, method):
    enc = _shell()
    fn = getattr(enc, method)
    for bad in (0, -1, 1 << 64):
        with pytest.raises(ValueError):
            fn(0, 0, bad)
    for bad in (1.0, "3", None, True):
        with pytest.raises(TypeError):
            fn(0, 0, bad)
    with pytest.raises(fe.FastEccError) as e:  # a valid count reaches the library, which refuses the null context
        fn(0, 0, 1)
    assert e.value.code == fe.E_INVAL


def test_scrub_batch_chunk_option_is_documented():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fastecc.h")).read()
    assert '"scrub_batch_chunk"' in header
    for name in NAMES:
        assert name + "(" in header
