"""Batched error location (fastecc_locate_errors_batch) and the "correct_batch_mode" option: what needs no GPU.

Every refusal here happens before any device is touched and writes nothing: a null context, null pointers (the outputs included),
count == 0, misaligned stripes, a count beyond 64 bits of bytes, and a block list asked for (cap > 0) without blocks or counts."""
import ctypes
import os

import pytest

import fastecc_amd as fe


@pytest.fixture(scope="module")
def hip_lib():
    return fe.lib()


def test_symbol_exported(hip_lib):
    assert hasattr(hip_lib, "fastecc_locate_errors_batch")
    assert hip_lib.fastecc_version() >= 360


class Outputs:
    def __init__(self, count=4, cap=2):
        self.status = (ctypes.c_uint8 * count)(*([0xAB] * count))
        self.blocks = (ctypes.c_uint64 * (count * cap))(*([0xB10C] * (count * cap)))
        self.counts = (ctypes.c_uint32 * count)(*([0xC0] * count))
        self.inc = ctypes.c_uint64(0xDEAD)
        self.cap = cap

    def untouched(self):
        return (set(self.status) == {0xAB} and set(self.blocks) == {0xB10C} and set(self.counts) == {0xC0} and self.inc.value == 0xDEAD)


def test_invalid_arguments_are_inval(hip_lib):
    fn = hip_lib.fastecc_locate_errors_batch
    buf = (ctypes.c_uint32 * 64)()
    a = ctypes.addressof(buf)
    o = Outputs()
    u8 = ctypes.cast(o.status, ctypes.POINTER(ctypes.c_uint8))
    rest = (u8, o.blocks, o.cap, o.counts, ctypes.byref(o.inc))
    assert fn(None, a, a, 1, None, 0, *rest) == fe.E_INVAL                # no context
    assert fn(None, None, a, 1, None, 0, *rest) == fe.E_INVAL             # no data
    assert fn(None, a, None, 1, None, 0, *rest) == fe.E_INVAL             # no parity
    assert fn(None, a, a, 0, None, 0, *rest) == fe.E_INVAL                # count 0
    assert fn(None, a + 2, a, 1, None, 0, *rest) == fe.E_INVAL            # misaligned data
    assert fn(None, a, a + 1, 1, None, 0, *rest) == fe.E_INVAL            # misaligned parity
    assert fn(None, a, a, (1 << 64) - 1, None, 0, *rest) == fe.E_INVAL    # (no context to size it: refused all the same)
    assert o.untouched()                                                  # a refused call writes nothing


def test_null_outputs_are_inval(hip_lib):
    fn = hip_lib.fastecc_locate_errors_batch
    buf = (ctypes.c_uint32 * 64)()
    a = ctypes.addressof(buf)
    o = Outputs()
    u8 = ctypes.cast(o.status, ctypes.POINTER(ctypes.c_uint8))
    inc = ctypes.byref(o.inc)
    assert fn(None, a, a, 1, None, 0, None, o.blocks, o.cap, o.counts, inc) == fe.E_INVAL   # no status
    assert fn(None, a, a, 1, None, 0, u8, o.blocks, o.cap, o.counts, None) == fe.E_INVAL    # no inconsistent count
    assert fn(None, a, a, 1, None, 0, u8, None, o.cap, o.counts, inc) == fe.E_INVAL         # cap > 0 without blocks
    assert fn(None, a, a, 1, None, 0, u8, o.blocks, o.cap, None, inc) == fe.E_INVAL         # cap > 0 without counts
    assert o.untouched()


def test_header_documents_the_call_and_the_option():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fastecc.h")).read()
    assert '"correct_batch_mode"' in header
    assert "fastecc_locate_errors_batch(" in header
    for scope in ("fingerprint_batch_list", "scrub_syndromes_gather", "scrub_root_search_batch", "direct_pass_list"):
        assert '"%s"' % scope in header


def test_python_method_validates_count(hip_lib):
    enc = fe.Encoder.__new__(fe.Encoder)  # an Encoder object without a context: no device is needed to reach the argument checks
    enc._h = ctypes.c_void_p()
    enc.n, enc.k = 20, 16
    for bad in (0, -1, 1 << 64):
        with pytest.raises(ValueError):
            enc.locate_errors_batch(0, 0, bad)
    for bad in (1.0, "3", None, True):
        with pytest.raises(TypeError):
            enc.locate_errors_batch(0, 0, bad)
    with pytest.raises(fe.FastEccError) as e:  # a valid count reaches the library, which refuses the null context
        enc.locate_errors_batch(0, 0, 1)
    assert e.value.code == fe.E_INVAL
