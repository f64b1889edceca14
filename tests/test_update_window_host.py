"""Sub-block pool writes (the four fastecc_update_*_window calls): argument checks that need no GPU.

Every refusal here happens before any device is touched: a null context, count == 0, null or misaligned pointers, width_words == 0 and a window whose
end wraps 2^64 are FASTECC_E_INVAL, and a refused call writes nothing.  The Python methods check col0 and width before the library is reached."""
import ctypes
import os

import pytest

import fastecc_amd as fe


@pytest.fixture(scope="module")
def hip_lib():
    return fe.lib()


NAMES = ("fastecc_update_batch_window", "fastecc_update_parity_batch_window", "fastecc_update_batch_set_window",
         "fastecc_update_parity_batch_set_window")
MAX = (1 << 64) - 1


def test_symbols_exported(hip_lib):
    for name in NAMES:
        assert hasattr(hip_lib, name), name
    assert hip_lib.fastecc_version() >= 430


class Buffers:
    """host words standing in for the pool, the rows, the write list and the patterns (no call here gets far enough to read them)"""

    def __init__(self):
        self.data = (ctypes.c_uint32 * 64)(*([0xD0D0D0D0] * 64))
        self.parity = (ctypes.c_uint32 * 64)(*([0xE1E1E1E1] * 64))
        self.new = (ctypes.c_uint32 * 64)(*([0xA5A5A5A5] * 64))
        self.old = (ctypes.c_uint32 * 64)(*([0xB6B6B6B6] * 64))
        self.writes = (ctypes.c_uint64 * 2)(0, 1)
        self.pattern_of = (ctypes.c_uint32 * 2)(0, fe.PATTERN_NONE)
        self.d, self.p, self.n, self.o = (ctypes.addressof(x) for x in (self.data, self.parity, self.new, self.old))

    def untouched(self):
        return (list(self.data) == [0xD0D0D0D0] * 64 and list(self.parity) == [0xE1E1E1E1] * 64 and list(self.new) == [0xA5A5A5A5] * 64
                and list(self.old) == [0xB6B6B6B6] * 64 and list(self.writes) == [0, 1] and list(self.pattern_of) == [0, fe.PATTERN_NONE])


def _call(lib, name, b, ctx=None, data=True, parity=True, count=1, po=True, writes=True, n=2, col0=0, width=4, old=True, new=True, skew=None):
    """one of the four calls on the host buffers; False for an argument: NULL; skew = (argument name, bytes): that pointer moved"""
    ptr = {"data": b.d if data else None, "parity": b.p if parity else None, "old": b.o if old else None, "new": b.n if new else None}
    if skew:
        ptr[skew[0]] += skew[1]
    w = b.writes if writes else None
    pattern_of = b.pattern_of if po else None
    if name == "fastecc_update_batch_window":
        return lib.fastecc_update_batch_window(ctx, ptr["data"], ptr["parity"], count, w, n, col0, width, ptr["new"], None)
    if name == "fastecc_update_parity_batch_window":
        return lib.fastecc_update_parity_batch_window(ctx, ptr["parity"], count, w, n, col0, width, ptr["old"], ptr["new"], None)
    if name == "fastecc_update_batch_set_window":
        return lib.fastecc_update_batch_set_window(ctx, ptr["data"], ptr["parity"], count, pattern_of, w, n, col0, width, ptr["new"], None)
    return lib.fastecc_update_parity_batch_set_window(ctx, ptr["parity"], count, pattern_of, w, n, col0, width, ptr["old"], ptr["new"], None)


@pytest.mark.parametrize("name", NAMES)
def test_invalid_arguments_are_inval(hip_lib, name):
    b = Buffers()
    has_data, has_old, has_set = "parity_batch" not in name, "parity_batch" in name, "_set_" in name
    cases = [dict(), dict(count=0), dict(count=0, n=0), dict(parity=False), dict(writes=False), dict(new=False), dict(count=MAX),
             dict(skew=("parity", 1)), dict(skew=("new", 3)), dict(skew=("new", 2)),
             dict(width=0), dict(width=0, n=0), dict(col0=1, width=MAX), dict(col0=MAX, width=1), dict(col0=MAX, width=MAX),
             dict(col0=1 << 63, width=1 << 63), dict(col0=MAX - 3, width=4)]
    if has_data:
        cases += [dict(data=False), dict(skew=("data", 2))]
    if has_old:
        cases += [dict(old=False), dict(skew=("old", 1))]
    if has_set:
        cases += [dict(po=False), dict(po=False, n=0)]
    for kw in cases:
        assert _call(hip_lib, name, b, **kw) == fe.E_INVAL, kw
    assert b.untouched()  # a refused call writes nothing


def _shell():
    """an Encoder object without a context (no device is needed to reach the argument checks)"""
    enc = fe.Encoder.__new__(fe.Encoder)
    enc._h = ctypes.c_void_p()
    enc.block_bytes = 4 * 260
    return enc


def _method(enc, method, **kw):
    if method == "update_batch":
        return enc.update_batch(0, 0, 1, [0], 0, **kw)
    if method == "update_parity_batch":
        return enc.update_parity_batch(0, 1, [0], 0, **kw)
    if method == "update_batch_set":
        return enc.update_batch_set(0, 0, 1, [fe.PATTERN_NONE], [0], 0, **kw)
    return enc.update_parity_batch_set(0, 1, [fe.PATTERN_NONE], [0], 0, **kw)


@pytest.mark.parametrize("method", ["update_batch", "update_parity_batch", "update_batch_set", "update_parity_batch_set"])
def test_python_methods_validate_the_window(hip_lib, method):
    enc = _shell()
    for bad in (dict(col0=1.0), dict(col0="1"), dict(col0=None), dict(col0=True), dict(width=2.0), dict(width="8"), dict(width=False),
                dict(col0=4, width=[4])):
        with pytest.raises(TypeError):
            _method(enc, method, **bad)
    for bad in (dict(col0=-1), dict(col0=-1, width=4), dict(col0=1 << 64, width=1), dict(width=0), dict(col0=8, width=0), dict(width=-4),
                dict(width=1 << 64), dict(col0=260), dict(col0=261)):  # (width=None from col0 = S on: no word of the block is left)
        with pytest.raises(ValueError):
            _method(enc, method, **bad)
    # valid windows reach the library, which refuses the null context: the whole block, a window, a window to the end of the block
    for good in (dict(), dict(col0=0, width=260), dict(col0=4, width=128), dict(col0=259)):
        with pytest.raises(fe.FastEccError) as e:
            _method(enc, method, **good)
        assert e.value.code == fe.E_INVAL


def test_entry_points_are_documented():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fastecc.h")).read()
    for name in NAMES:
        assert name + "(" in header
    assert "no word outside the window's columns is read or written, in any block of the pool" in header  # the footprint
