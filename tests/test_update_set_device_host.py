"""Degraded pool writes from a write list in device memory (fastecc_update_batch_set_device, fastecc_update_parity_batch_set_device): what needs no GPU.

The return value of the two calls covers what the host can decide without the lists.  Every refusal checked here comes BEFORE the context is read:
the context pointer handed in lies in the first page of the address space, which is never mapped, so a call that read it would end the process.
Host memory stands in for the pool, the rows, the write list, pattern_of and the status word, and a refused call writes nothing.  The Python methods
check count, n_writes, max_per_stripe, max_absent, col0 and width before the library is reached."""
import ctypes
import os

import pytest

import fastecc_amd as fe


@pytest.fixture(scope="module")
def hip_lib():
    return fe.lib()


NAMES = ("fastecc_update_batch_set_device", "fastecc_update_parity_batch_set_device")
MAX = (1 << 64) - 1
NEVER_MAPPED = 0x40  # a context pointer that cannot be dereferenced


def test_symbols_exported(hip_lib):
    for name in NAMES:
        assert hasattr(hip_lib, name), name
    assert hip_lib.fastecc_version() >= 470


class Buffers:
    """host words standing in for the pool, the rows, the lists and the status word (no call here gets far enough to read them)"""

    FILL = dict(data=0xD0D0D0D0, parity=0xE1E1E1E1, new=0xA5A5A5A5, old=0xB6B6B6B6, pattern=0xC7C7C7C7)

    def __init__(self):
        self.arr = {name: (ctypes.c_uint32 * 64)(*([v] * 64)) for name, v in self.FILL.items()}
        self.writes = (ctypes.c_uint64 * 4)(0, 1, MAX, 0x77)  # (two entries are handed in; the others: room for a misaligned pointer)
        self.status = (ctypes.c_uint64 * 2)(0x5151515151515151, 0x5151515151515151)
        self.ptr = {name: ctypes.addressof(a) for name, a in self.arr.items()}
        self.ptr["writes"], self.ptr["status"] = ctypes.addressof(self.writes), ctypes.addressof(self.status)

    def untouched(self):
        return (all(list(self.arr[name]) == [v] * 64 for name, v in self.FILL.items()) and list(self.writes) == [0, 1, MAX, 0x77]
                and list(self.status) == [0x5151515151515151] * 2)


def _call(lib, name, b, ctx=NEVER_MAPPED, count=2, n=2, mps=1, max_absent=2, col0=0, width=4, null=(), skew=None, put=None):
    """one of the two calls on the host buffers; null: argument names handed in as NULL; skew = (name, bytes): that pointer moved;
    put = (name, other, bytes): that pointer placed at `other` + bytes"""
    ptr = dict(b.ptr)
    if skew:
        ptr[skew[0]] += skew[1]
    if put:
        ptr[put[0]] = b.ptr[put[1]] + put[2]
    for name_ in null:
        ptr[name_] = None
    if name == "fastecc_update_batch_set_device":
        return lib.fastecc_update_batch_set_device(ctx, ptr["data"], ptr["parity"], count, ptr["pattern"], ptr["writes"], n, mps, max_absent, col0, width,
                                                   ptr["new"], ptr["status"], None)
    return lib.fastecc_update_parity_batch_set_device(ctx, ptr["parity"], count, ptr["pattern"], ptr["writes"], n, mps, col0, width, ptr["old"], ptr["new"],
                                                      ptr["status"], None)


@pytest.mark.parametrize("name", NAMES)
def test_refusals_before_the_context_is_read(hip_lib, name):
    b = Buffers()
    inval = [dict(ctx=None), dict(count=0), dict(count=0, n=0),
             dict(null=("pattern",)), dict(null=("pattern",), n=0), dict(null=("writes",)), dict(null=("status",)), dict(null=("status",), n=0),
             dict(null=("parity",)), dict(null=("new",)),
             dict(skew=("pattern", 1)), dict(skew=("pattern", 2)), dict(skew=("pattern", 3)), dict(skew=("writes", 4)), dict(skew=("writes", 1)),
             dict(skew=("status", 4)), dict(skew=("status", 2)), dict(skew=("parity", 1)), dict(skew=("new", 2)),
             dict(mps=0), dict(mps=17), dict(mps=0, n=0), dict(mps=17, n=0), dict(mps=0xFFFFFFFF), dict(width=0), dict(width=0, n=0),
             # overlaps: pattern_of (count entries of 4 bytes) against the list, the status word and the rows; the list and the status word likewise
             dict(put=("pattern", "writes", 0)), dict(put=("pattern", "writes", 12)), dict(put=("writes", "pattern", 0)),
             dict(put=("pattern", "status", 0)), dict(put=("pattern", "status", 4)), dict(put=("status", "pattern", 0)),
             dict(put=("pattern", "new", 0)), dict(put=("pattern", "new", 28)), dict(put=("new", "pattern", 4)),
             dict(put=("status", "writes", 8)), dict(put=("writes", "new", 8)), dict(put=("status", "new", 24))]
    if name == "fastecc_update_batch_set_device":
        inval += [dict(null=("data",)), dict(skew=("data", 2))]
    else:
        inval += [dict(skew=("old", 1)), dict(put=("pattern", "old", 0)), dict(put=("writes", "old", 16)), dict(put=("status", "old", 8))]
    for kw in inval:
        assert _call(hip_lib, name, b, **kw) == fe.E_INVAL, kw
    for kw in (dict(count=(1 << 24) + 1), dict(n=(1 << 24) + 1), dict(count=1 << 40, n=0), dict(n=MAX)):
        assert _call(hip_lib, name, b, **kw) == fe.E_UNSUPPORTED, kw
    assert b.untouched()  # a refused call writes nothing, the status word included


def _shell():
    """an Encoder object without a context (no device is needed to reach the argument checks)"""
    enc = fe.Encoder.__new__(fe.Encoder)
    enc._h = ctypes.c_void_p()
    enc.block_bytes = 4 * 260
    return enc


def _method(enc, method, count=1, n_writes=1, **kw):
    if method == "update_batch_set_device":
        return enc.update_batch_set_device(0, 0, count, 0, 0, n_writes, 0, 0, **kw)
    return enc.update_parity_batch_set_device(0, count, 0, 0, n_writes, 0, 0, **kw)


@pytest.mark.parametrize("method", ["update_batch_set_device", "update_parity_batch_set_device"])
def test_python_methods_validate_their_arguments(hip_lib, method):
    enc = _shell()
    type_errors = [dict(col0=1.0), dict(col0="1"), dict(col0=None), dict(col0=True), dict(width=2.0), dict(width="8"), dict(width=False),
                   dict(col0=4, width=[4]), dict(max_per_stripe=1.0), dict(max_per_stripe=True), dict(max_per_stripe=None), dict(n_writes=2.0),
                   dict(n_writes=False), dict(count=1.0), dict(count=True)]
    value_errors = [dict(col0=-1), dict(col0=-1, width=4), dict(col0=1 << 64, width=1), dict(width=0), dict(col0=8, width=0), dict(width=-4),
                    dict(width=1 << 64), dict(col0=260), dict(col0=261), dict(max_per_stripe=0), dict(max_per_stripe=17), dict(max_per_stripe=-1),
                    dict(n_writes=-1), dict(n_writes=1 << 64), dict(count=0), dict(count=1 << 64)]
    good = [dict(), dict(col0=0, width=260), dict(col0=4, width=128), dict(col0=259), dict(max_per_stripe=16), dict(max_per_stripe=3), dict(n_writes=0)]
    if method == "update_batch_set_device":
        type_errors += [dict(max_absent=1.0), dict(max_absent=True), dict(max_absent="1")]
        value_errors += [dict(max_absent=-1), dict(max_absent=1 << 64)]
        good += [dict(max_absent=None), dict(max_absent=0), dict(max_absent=1), dict(max_absent=(1 << 64) - 1)]
    for bad in type_errors:
        with pytest.raises(TypeError):
            _method(enc, method, **bad)
    for bad in value_errors:
        with pytest.raises(ValueError):
            _method(enc, method, **bad)
    for kw in good:  # valid arguments reach the library, which refuses the null context
        with pytest.raises(fe.FastEccError) as e:
            _method(enc, method, **kw)
        assert e.value.code == fe.E_INVAL


def test_entry_points_are_documented():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fastecc.h")).read()
    for name in NAMES:
        assert name + "(" in header
    assert "#define FASTECC_VERSION 470" in header
    assert "There are no _set (degraded) forms of these two calls" not in header
    assert "All or nothing: a non-zero status means that no word of the pool has been written by the call." in header
    assert "0 is allowed and means the caller promises that none is absent; n_writes is always safe." in header
    assert "FASTECC_E_NOMEM: more absent written blocks than max_absent; the row is one write" in header
    assert "Entries of pattern_of for stripes that no write" in header
