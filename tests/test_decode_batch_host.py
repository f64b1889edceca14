"""Batched decode and repair (fastecc_decode_batch / _repair_batch): argument checks that need no GPU.

Every refusal here happens before any device is touched: a null context, null pointers and count == 0 are FASTECC_E_INVAL."""
import ctypes

import pytest

import fastecc_amd as fe


@pytest.fixture(scope="module")
def hip_lib():
    return fe.lib()


NAMES = ("fastecc_decode_batch", "fastecc_repair_batch")


def test_symbols_exported(hip_lib):
    for name in NAMES:
        assert hasattr(hip_lib, name), name
    assert hip_lib.fastecc_version() >= 320


@pytest.mark.parametrize("name", NAMES)
def test_null_arguments_are_inval(hip_lib, name):
    fn = getattr(hip_lib, name)
    buf = (ctypes.c_uint32 * 64)()
    a = ctypes.addressof(buf)
    assert fn(None, a, a, 1, None) == fe.E_INVAL       # no context
    assert fn(None, None, None, 0, None) == fe.E_INVAL
    assert fn(None, a, a, 0, None) == fe.E_INVAL       # count 0
    assert fn(None, a + 2, a, 1, None) == fe.E_INVAL   # misaligned


def _shell():
    """an Encoder object without a context (no device is needed to reach the argument checks)"""
    enc = fe.Encoder.__new__(fe.Encoder)
    enc._h = ctypes.c_void_p()
    return enc


@pytest.mark.parametrize("method", ["decode_batch", "repair_batch"])
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
