"""Scrub of degraded stripes (fastecc_scrub_erasures): the pieces that need no GPU.

The symbol is exported, the version says so, and a null context is refused before any device is touched."""
import ctypes
import os

import pytest

import fastecc_amd as fe


@pytest.fixture(scope="module")
def hip_lib():
    return fe.lib()


def test_symbol_exported_and_version(hip_lib):
    assert hasattr(hip_lib, "fastecc_scrub_erasures")
    assert hip_lib.fastecc_version() >= 350


def test_null_context_is_inval(hip_lib):
    flags = (ctypes.c_uint8 * 4)(1, 0, 1, 1)
    assert hip_lib.fastecc_scrub_erasures(None, None, None) == fe.E_INVAL
    assert hip_lib.fastecc_scrub_erasures(None, flags, flags) == fe.E_INVAL
    assert list(flags) == [1, 0, 1, 1]


def test_python_method_checks_lengths_and_reaches_the_library(hip_lib):
    enc = fe.Encoder.__new__(fe.Encoder)  # no context: no device is needed to reach the argument checks
    enc._h, enc.n, enc.k = ctypes.c_void_p(), 6, 4
    with pytest.raises(ValueError):
        enc.scrub_erasures([1, 1, 1], None)
    with pytest.raises(ValueError):
        enc.scrub_erasures(None, [1, 1, 1])
    for args in ((), ([1, 0, 1, 1], None), (None, [0, 1]), ([1, 1, 1, 1], [1, 0])):
        with pytest.raises(fe.FastEccError) as e:  # well-formed flags reach the library, which refuses the null context
            enc.scrub_erasures(*args)
        assert e.value.code == fe.E_INVAL


def test_header_documents_the_call():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fastecc.h")).read()
    assert "fastecc_scrub_erasures(" in header
    assert "2t + b + w <= n - k" in header
