"""Batched location with a pattern per stripe (fastecc_locate_errors_batch_set): what needs no GPU.

Every refusal here happens before any device is touched and writes nothing: a null context, null pointers (pattern_of and the outputs
included), count == 0, misaligned stripes, a count beyond 64 bits of bytes, and a block list asked for (cap > 0) without blocks or counts."""
import ctypes
import os

import numpy as np
import pytest

import fastecc_amd as fe


@pytest.fixture(scope="module")
def hip_lib():
    return fe.lib()


def test_symbol_exported(hip_lib):
    assert hasattr(hip_lib, "fastecc_locate_errors_batch_set")
    assert hip_lib.fastecc_version() >= 400


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
    fn = hip_lib.fastecc_locate_errors_batch_set
    buf = (ctypes.c_uint32 * 64)()
    a = ctypes.addressof(buf)
    po = (ctypes.c_uint32 * 4)(0, 0, 0, 0)
    o = Outputs()
    u8 = ctypes.cast(o.status, ctypes.POINTER(ctypes.c_uint8))
    rest = (u8, o.blocks, o.cap, o.counts, ctypes.byref(o.inc))
    assert fn(None, a, a, 1, po, None, 0, *rest) == fe.E_INVAL                # no context
    assert fn(None, None, a, 1, po, None, 0, *rest) == fe.E_INVAL             # no data
    assert fn(None, a, None, 1, po, None, 0, *rest) == fe.E_INVAL             # no parity
    assert fn(None, a, a, 1, None, None, 0, *rest) == fe.E_INVAL              # no pattern_of
    assert fn(None, a, a, 0, po, None, 0, *rest) == fe.E_INVAL                # count 0
    assert fn(None, a + 2, a, 1, po, None, 0, *rest) == fe.E_INVAL            # misaligned data
    assert fn(None, a, a + 1, 1, po, None, 0, *rest) == fe.E_INVAL            # misaligned parity
    assert fn(None, a, a, (1 << 64) - 1, po, None, 0, *rest) == fe.E_INVAL    # (no context to size it: refused all the same)
    assert o.untouched()                                                      # a refused call writes nothing


def test_null_outputs_are_inval(hip_lib):
    fn = hip_lib.fastecc_locate_errors_batch_set
    buf = (ctypes.c_uint32 * 64)()
    a = ctypes.addressof(buf)
    po = (ctypes.c_uint32 * 4)(0, 0, 0, 0)
    o = Outputs()
    u8 = ctypes.cast(o.status, ctypes.POINTER(ctypes.c_uint8))
    inc = ctypes.byref(o.inc)
    assert fn(None, a, a, 1, po, None, 0, None, o.blocks, o.cap, o.counts, inc) == fe.E_INVAL   # no status
    assert fn(None, a, a, 1, po, None, 0, u8, o.blocks, o.cap, o.counts, None) == fe.E_INVAL    # no inconsistent count
    assert fn(None, a, a, 1, po, None, 0, u8, None, o.cap, o.counts, inc) == fe.E_INVAL         # cap > 0 without blocks
    assert fn(None, a, a, 1, po, None, 0, u8, o.blocks, o.cap, None, inc) == fe.E_INVAL         # cap > 0 without counts
    assert o.untouched()


def test_header_documents_the_call_the_modes_and_the_scopes():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fastecc.h")).read()
    assert "fastecc_locate_errors_batch_set(" in header
    for scope in ("fingerprint_set_list", "scrub_syndromes_gather_set", "scrub_root_search_batch", "direct_pass_set"):
        assert '"%s"' % scope in header
    assert '"correct_batch_mode" does not apply' not in header
    section = header[header.index("fastecc_correct_batch_set :"):header.index("int fastecc_scrub_erasures_set(")]
    assert '"correct_batch_mode"' in section and "unspecified" in section


def test_python_method_validates_count_and_pattern_of(hip_lib):
    enc = fe.Encoder.__new__(fe.Encoder)  # an Encoder object without a context: no device is needed to reach the argument checks
    enc._h = ctypes.c_void_p()
    enc.n, enc.k = 20, 16
    fn = enc.locate_errors_batch_set
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
