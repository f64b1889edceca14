"""Degraded writes (fastecc_update_batch_set / fastecc_update_parity_batch_set): argument checks that need no GPU.

Every refusal here happens before any device is touched: a null context, count == 0, null pointers with writes to do (a null pattern_of
among them) and misaligned pointers are FASTECC_E_INVAL, and a refused call writes nothing.  The Python methods check the count, the list
and the length of pattern_of before the library is reached."""
import ctypes
import os

import pytest

import fastecc_amd as fe


@pytest.fixture(scope="module")
def hip_lib():
    return fe.lib()


NAMES = ("fastecc_update_batch_set", "fastecc_update_parity_batch_set")


def test_symbols_exported(hip_lib):
    for name in NAMES:
        assert hasattr(hip_lib, name), name
    assert hip_lib.fastecc_version() >= 420


class Buffers:
    """host words standing in for the pool, the blocks, the write list and the patterns (no call here gets far enough to read them)"""

    def __init__(self):
        self.data = (ctypes.c_uint32 * 64)(*([0xD0D0D0D0] * 64))
        self.parity = (ctypes.c_uint32 * 64)(*([0xE1E1E1E1] * 64))
        self.new = (ctypes.c_uint32 * 64)(*([0xA5A5A5A5] * 64))
        self.writes = (ctypes.c_uint64 * 2)(0, 1)
        self.pattern_of = (ctypes.c_uint32 * 2)(0, fe.PATTERN_NONE)
        self.d, self.p, self.n = (ctypes.addressof(x) for x in (self.data, self.parity, self.new))

    def untouched(self):
        return (list(self.data) == [0xD0D0D0D0] * 64 and list(self.parity) == [0xE1E1E1E1] * 64 and list(self.new) == [0xA5A5A5A5] * 64
                and list(self.writes) == [0, 1] and list(self.pattern_of) == [0, fe.PATTERN_NONE])


def test_update_batch_set_invalid_arguments_are_inval(hip_lib):
    fn = hip_lib.fastecc_update_batch_set
    b = Buffers()
    w, po = b.writes, b.pattern_of
    assert fn(None, b.d, b.p, 1, po, w, 2, b.n, None) == fe.E_INVAL          # no context
    assert fn(None, b.d, b.p, 0, po, w, 2, b.n, None) == fe.E_INVAL          # count 0
    assert fn(None, b.d, b.p, 0, po, w, 0, b.n, None) == fe.E_INVAL          # count 0, nothing to write
    assert fn(None, None, b.p, 1, po, w, 2, b.n, None) == fe.E_INVAL         # no data
    assert fn(None, b.d, None, 1, po, w, 2, b.n, None) == fe.E_INVAL         # no parity
    assert fn(None, b.d, b.p, 1, None, w, 2, b.n, None) == fe.E_INVAL        # no pattern_of
    assert fn(None, b.d, b.p, 1, None, w, 0, b.n, None) == fe.E_INVAL        # ... with nothing to write
    assert fn(None, b.d, b.p, 1, po, None, 2, b.n, None) == fe.E_INVAL       # no list
    assert fn(None, b.d, b.p, 1, po, w, 2, None, None) == fe.E_INVAL         # no new blocks
    assert fn(None, b.d + 2, b.p, 1, po, w, 2, b.n, None) == fe.E_INVAL      # misaligned data
    assert fn(None, b.d, b.p + 1, 1, po, w, 2, b.n, None) == fe.E_INVAL      # misaligned parity
    assert fn(None, b.d, b.p, 1, po, w, 2, b.n + 3, None) == fe.E_INVAL      # misaligned new blocks
    assert fn(None, b.d, b.p, (1 << 64) - 1, po, w, 2, b.n, None) == fe.E_INVAL  # (no context to size it: refused all the same)
    assert b.untouched()                                                     # a refused call writes nothing


def test_update_parity_batch_set_invalid_arguments_are_inval(hip_lib):
    fn = hip_lib.fastecc_update_parity_batch_set
    b = Buffers()
    w, po = b.writes, b.pattern_of
    assert fn(None, b.p, 1, po, w, 2, b.d, b.n, None) == fe.E_INVAL          # no context
    assert fn(None, b.p, 1, po, w, 2, None, b.n, None) == fe.E_INVAL         # ... with old blocks from zero
    assert fn(None, b.p, 0, po, w, 2, b.d, b.n, None) == fe.E_INVAL          # count 0
    assert fn(None, None, 1, po, w, 2, b.d, b.n, None) == fe.E_INVAL         # no parity
    assert fn(None, b.p, 1, None, w, 2, b.d, b.n, None) == fe.E_INVAL        # no pattern_of
    assert fn(None, b.p, 1, po, None, 2, b.d, b.n, None) == fe.E_INVAL       # no list
    assert fn(None, b.p, 1, po, w, 2, b.d, None, None) == fe.E_INVAL         # no new blocks
    assert fn(None, b.p + 2, 1, po, w, 2, b.d, b.n, None) == fe.E_INVAL      # misaligned parity
    assert fn(None, b.p, 1, po, w, 2, b.d + 1, b.n, None) == fe.E_INVAL      # misaligned old blocks
    assert fn(None, b.p, 1, po, w, 2, b.d, b.n + 2, None) == fe.E_INVAL      # misaligned new blocks
    assert fn(None, b.p, (1 << 64) - 1, po, w, 2, b.d, b.n, None) == fe.E_INVAL
    assert b.untouched()


def _shell():
    """an Encoder object without a context (no device is needed to reach the argument checks)"""
    enc = fe.Encoder.__new__(fe.Encoder)
    enc._h = ctypes.c_void_p()
    return enc


def _call(enc, method, count, pattern_of, writes):
    if method == "update_batch_set":
        return enc.update_batch_set(0, 0, count, pattern_of, writes, 0)
    return enc.update_parity_batch_set(0, count, pattern_of, writes, 0)


@pytest.mark.parametrize("method", ["update_batch_set", "update_parity_batch_set"])
def test_python_methods_validate_count_list_and_patterns(hip_lib, method):
    enc = _shell()
    for bad in (0, -1, 1 << 64):
        with pytest.raises(ValueError):
            _call(enc, method, bad, [0], [0])
    for bad in (1.0, "3", None, True):
        with pytest.raises(TypeError):
            _call(enc, method, bad, [0], [0])
    for bad in (None, 5, [None], [[1]]):          # not a list of integers
        with pytest.raises(TypeError):
            _call(enc, method, 1, [0], bad)
    with pytest.raises(ValueError):
        _call(enc, method, 1, [0], ["x"])
    for bad in ([], [0, 0]):                      # pattern_of: one entry per stripe
        with pytest.raises(ValueError):
            _call(enc, method, 1, bad, [0])
    with pytest.raises(ValueError):
        _call(enc, method, 2, [0, 0, 0], [0])
    for bad in ([-1], [1 << 32]):                 # ... each a uint32
        with pytest.raises(ValueError):
            _call(enc, method, 1, bad, [0])
    with pytest.raises(fe.FastEccError) as e:     # valid arguments reach the library, which refuses the null context
        _call(enc, method, 1, [fe.PATTERN_NONE], [0])
    assert e.value.code == fe.E_INVAL


def test_entry_points_are_documented():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fastecc.h")).read()
    for name in NAMES:
        assert name + "(" in header
    assert "No absent block, data or parity, is written" in header   # the promise about absent blocks
