"""Pool writes from a write list in device memory (fastecc_update_batch_device, fastecc_update_parity_batch_device): what needs no GPU.

The return value of the two calls covers what the host can decide without the list, and every such refusal happens before any device is touched:
here a null context, count == 0, null or misaligned pointers, a null status, max_per_stripe 0 and 17 and a window outside the block are
FASTECC_E_INVAL with host memory standing in for the pool, the rows, the list and the status word, and a refused call writes nothing.  The Python
methods check count, n_writes, max_per_stripe, col0 and width before the library is reached."""
import ctypes
import os

import pytest

import fastecc_amd as fe


@pytest.fixture(scope="module")
def hip_lib():
    return fe.lib()


NAMES = ("fastecc_update_batch_device", "fastecc_update_parity_batch_device")
MAX = (1 << 64) - 1


def test_symbols_exported(hip_lib):
    for name in NAMES:
        assert hasattr(hip_lib, name), name
    assert hip_lib.fastecc_version() >= 450
    assert fe.WRITE_NONE == MAX


class Buffers:
    """host words standing in for the pool, the rows, the write list and the status word (no call here gets far enough to read them)"""

    def __init__(self):
        self.data = (ctypes.c_uint32 * 64)(*([0xD0D0D0D0] * 64))
        self.parity = (ctypes.c_uint32 * 64)(*([0xE1E1E1E1] * 64))
        self.new = (ctypes.c_uint32 * 64)(*([0xA5A5A5A5] * 64))
        self.old = (ctypes.c_uint32 * 64)(*([0xB6B6B6B6] * 64))
        self.writes = (ctypes.c_uint64 * 4)(0, 1, MAX, 0x77)  # (two entries are handed in; the others: room for a misaligned pointer)
        self.status = (ctypes.c_uint64 * 2)(0x5151515151515151, 0x5151515151515151)
        self.d, self.p, self.n, self.o, self.w, self.s = (ctypes.addressof(x) for x in (self.data, self.parity, self.new, self.old, self.writes, self.status))

    def untouched(self):
        return (list(self.data) == [0xD0D0D0D0] * 64 and list(self.parity) == [0xE1E1E1E1] * 64 and list(self.new) == [0xA5A5A5A5] * 64
                and list(self.old) == [0xB6B6B6B6] * 64 and list(self.writes) == [0, 1, MAX, 0x77] and list(self.status) == [0x5151515151515151] * 2)


def _call(lib, name, b, ctx=None, data=True, parity=True, count=1, writes=True, n=2, mps=1, col0=0, width=4, old=True, new=True, status=True, skew=None):
    """one of the two calls on the host buffers; False for an argument: NULL; skew = (argument name, bytes): that pointer moved"""
    ptr = {"data": b.d if data else None, "parity": b.p if parity else None, "old": b.o if old else None, "new": b.n if new else None,
           "writes": b.w if writes else None, "status": b.s if status else None}
    if skew:
        ptr[skew[0]] += skew[1]
    if name == "fastecc_update_batch_device":
        return lib.fastecc_update_batch_device(ctx, ptr["data"], ptr["parity"], count, ptr["writes"], n, mps, col0, width, ptr["new"], ptr["status"], None)
    return lib.fastecc_update_parity_batch_device(ctx, ptr["parity"], count, ptr["writes"], n, mps, col0, width, ptr["old"], ptr["new"], ptr["status"], None)


@pytest.mark.parametrize("name", NAMES)
def test_invalid_arguments_are_inval(hip_lib, name):
    b = Buffers()
    cases = [dict(), dict(count=0), dict(count=0, n=0), dict(parity=False), dict(writes=False), dict(new=False), dict(count=MAX),
             dict(skew=("parity", 1)), dict(skew=("new", 3)), dict(skew=("new", 2)), dict(skew=("writes", 4)), dict(skew=("writes", 1)),
             dict(skew=("status", 4)), dict(skew=("status", 2)), dict(status=False), dict(status=False, n=0),
             dict(mps=0), dict(mps=17), dict(mps=0, n=0), dict(mps=17, n=0), dict(mps=0xFFFFFFFF),
             dict(width=0), dict(width=0, n=0), dict(col0=1, width=MAX), dict(col0=MAX, width=1), dict(col0=MAX, width=MAX),
             dict(col0=1 << 63, width=1 << 63), dict(col0=MAX - 3, width=4)]
    if name == "fastecc_update_batch_device":
        cases += [dict(data=False), dict(skew=("data", 2))]
    else:
        cases += [dict(old=False), dict(skew=("old", 1))]
    for kw in cases:
        assert _call(hip_lib, name, b, **kw) == fe.E_INVAL, kw
    assert b.untouched()  # a refused call writes nothing, the status word included


def _shell():
    """an Encoder object without a context (no device is needed to reach the argument checks)"""
    enc = fe.Encoder.__new__(fe.Encoder)
    enc._h = ctypes.c_void_p()
    enc.block_bytes = 4 * 260
    return enc


def _method(enc, method, count=1, n_writes=1, **kw):
    if method == "update_batch_device":
        return enc.update_batch_device(0, 0, count, 0, n_writes, 0, 0, **kw)
    return enc.update_parity_batch_device(0, count, 0, n_writes, 0, 0, **kw)


@pytest.mark.parametrize("method", ["update_batch_device", "update_parity_batch_device"])
def test_python_methods_validate_their_arguments(hip_lib, method):
    enc = _shell()
    for bad in (dict(col0=1.0), dict(col0="1"), dict(col0=None), dict(col0=True), dict(width=2.0), dict(width="8"), dict(width=False),
                dict(col0=4, width=[4]), dict(max_per_stripe=1.0), dict(max_per_stripe=True), dict(max_per_stripe=None), dict(n_writes=2.0),
                dict(n_writes=False), dict(count=1.0), dict(count=True)):
        with pytest.raises(TypeError):
            _method(enc, method, **bad)
    for bad in (dict(col0=-1), dict(col0=-1, width=4), dict(col0=1 << 64, width=1), dict(width=0), dict(col0=8, width=0), dict(width=-4),
                dict(width=1 << 64), dict(col0=260), dict(col0=261), dict(max_per_stripe=0), dict(max_per_stripe=17), dict(max_per_stripe=-1),
                dict(n_writes=-1), dict(n_writes=1 << 64), dict(count=0), dict(count=1 << 64)):
        with pytest.raises(ValueError):
            _method(enc, method, **bad)
    # valid arguments reach the library, which refuses the null context: the whole block, windows, every promise, an empty list
    for good in (dict(), dict(col0=0, width=260), dict(col0=4, width=128), dict(col0=259), dict(max_per_stripe=16), dict(max_per_stripe=3),
                 dict(n_writes=0)):
        with pytest.raises(fe.FastEccError) as e:
            _method(enc, method, **good)
        assert e.value.code == fe.E_INVAL


def test_entry_points_are_documented():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fastecc.h")).read()
    for name in NAMES:
        assert name + "(" in header
    assert "#define FASTECC_WRITE_NONE UINT64_MAX" in header
    assert "All or nothing: when status is non-zero, no word of the pool has been written by the call." in header
    assert "The device form has no rounds" in header  # more than 16 writes to one stripe: the host-list calls or a re-encode
