"""fastecc_encode_pool (the parity of a pool of stripes) and its option "encode_pool_kernel": what can be checked without a GPU.

Every refusal here happens before any device is touched: a null context, null pointers, count == 0 and misaligned pointers are
FASTECC_E_INVAL, Encoder.encode_pool rejects a bad `count` before the library is called, and fastecc_set_option refuses a null context or
a null name whatever the value (its range check, 0..3, needs a context and so a device: tests/test_gpu_encode_pool.py)."""
import ctypes

import pytest

import fastecc_amd as fe


@pytest.fixture(scope="module")
def hip_lib():
    return fe.lib()


def test_symbol_exported(hip_lib):
    assert hasattr(hip_lib, "fastecc_encode_pool")
    assert hip_lib.fastecc_version() >= 390
    assert hasattr(fe.Encoder, "encode_pool")


def test_null_arguments_are_inval(hip_lib):
    fn = hip_lib.fastecc_encode_pool
    buf = (ctypes.c_uint32 * 64)()
    a = ctypes.addressof(buf)
    assert fn(None, a, a + 128, 1, None) == fe.E_INVAL    # no context
    assert fn(None, None, None, 0, None) == fe.E_INVAL
    assert fn(None, None, a, 1, None) == fe.E_INVAL       # no data
    assert fn(None, a, None, 1, None) == fe.E_INVAL       # no parity
    assert fn(None, a, a + 128, 0, None) == fe.E_INVAL    # count 0
    assert fn(None, a + 2, a + 128, 1, None) == fe.E_INVAL  # misaligned
    assert fn(None, a, a + 129, 1, None) == fe.E_INVAL


def _shell(n=20, k=16):
    """an Encoder object without a context (no device is needed to reach the argument checks)"""
    enc = fe.Encoder.__new__(fe.Encoder)
    enc._h = ctypes.c_void_p()
    enc.n, enc.k = n, k
    return enc


def test_python_method_validates_count(hip_lib):
    enc = _shell()
    for bad in (0, -1, 1 << 64):
        with pytest.raises(ValueError):
            enc.encode_pool(0, 0, bad)
    for bad in (1.0, "3", None, True):
        with pytest.raises(TypeError):
            enc.encode_pool(0, 0, bad)
    buf = (ctypes.c_uint32 * 64)()
    a = ctypes.addressof(buf)
    for good in (1, 2, (1 << 64) - 1):
        with pytest.raises(fe.FastEccError) as e:  # a valid count reaches the library, which refuses the null context
            enc.encode_pool(a, a + 128, good)
        assert e.value.code == fe.E_INVAL


def test_option_without_context_is_inval(hip_lib):
    for value in (-1, 0, 1, 2, 3, 4):
        assert hip_lib.fastecc_set_option(None, b"encode_pool_kernel", value) == fe.E_INVAL
    with pytest.raises(fe.FastEccError) as e:
        _shell().set_option("encode_pool_kernel", 2)
    assert e.value.code == fe.E_INVAL
