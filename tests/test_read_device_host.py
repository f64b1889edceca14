"""Degraded reads from a request list in device memory (fastecc_read_batch_set_device, fastecc_read_batch_device): what needs no GPU.

The return value of the two calls covers what the host can decide without the lists.  Every refusal that needs nothing of the context comes
before the context is read: here the context pointer is an address in the never-mapped first page (a check that read it would fault), host
memory stands in for the pool, `out`, the lists and the status word, and a refused call writes none of them.  The refusals that need the
context (the window against the block, overlaps, nothing prepared, the field, sharding, a row pitch) are in tests/test_gpu_read_device.py.  The
Python methods check count, n_reads, col0 and width before the library is reached."""
import ctypes
import os

import pytest

import fastecc_amd as fe


@pytest.fixture(scope="module")
def hip_lib():
    return fe.lib()


NAMES = ("fastecc_read_batch_set_device", "fastecc_read_batch_device")
MAX = (1 << 64) - 1
FAKE = 0x10  # an address in the never-mapped first page


def test_symbols_exported(hip_lib):
    for name in NAMES:
        assert hasattr(hip_lib, name), name
    assert hip_lib.fastecc_version() >= 460
    assert fe.READ_NONE == MAX
    assert hasattr(fe.Encoder, "read_batch_set_device") and hasattr(fe.Encoder, "read_batch_device")


class Buffers:
    """host words standing in for the pool, `out`, the two lists and the status word (no call here gets far enough to read them)"""

    def __init__(self):
        self.data = (ctypes.c_uint32 * 64)(*([0xD0D0D0D0] * 64))
        self.parity = (ctypes.c_uint32 * 64)(*([0xE1E1E1E1] * 64))
        self.out = (ctypes.c_uint32 * 64)(*([0xA5A5A5A5] * 64))
        self.reads = (ctypes.c_uint64 * 4)(0, 1, MAX, 0x77)  # (two entries are handed in; the others: room for a misaligned pointer)
        self.po = (ctypes.c_uint32 * 4)(0, 0, 0, 0)
        self.status = (ctypes.c_uint64 * 2)(0x5151515151515151, 0x5151515151515151)
        self.ptr = {name: ctypes.addressof(x) for name, x in (("data", self.data), ("parity", self.parity), ("out", self.out), ("reads", self.reads),
                                                              ("po", self.po), ("status", self.status))}

    def untouched(self):
        return (list(self.data) == [0xD0D0D0D0] * 64 and list(self.parity) == [0xE1E1E1E1] * 64 and list(self.out) == [0xA5A5A5A5] * 64
                and list(self.reads) == [0, 1, MAX, 0x77] and list(self.po) == [0] * 4 and list(self.status) == [0x5151515151515151] * 2)


def _call(lib, name, b, ctx=FAKE, count=1, n=2, col0=0, width=4, null=(), skew=None):
    """one of the two calls on the host buffers; null: the arguments that are NULL; skew = (argument name, bytes): that pointer moved"""
    ptr = {k: (None if k in null else v) for k, v in b.ptr.items()}
    if skew:
        ptr[skew[0]] += skew[1]
    if name == "fastecc_read_batch_set_device":
        return lib.fastecc_read_batch_set_device(ctx, ptr["data"], ptr["parity"], count, ptr["po"], ptr["reads"], n, col0, width, ptr["out"], ptr["status"], None)
    return lib.fastecc_read_batch_device(ctx, ptr["data"], ptr["parity"], count, ptr["reads"], n, col0, width, ptr["out"], ptr["status"], None)


@pytest.mark.parametrize("name", NAMES)
def test_refusals_before_the_context_is_read(hip_lib, name):
    b = Buffers()
    assert _call(hip_lib, name, b, ctx=None) == fe.E_INVAL  # no context
    assert _call(hip_lib, name, b, ctx=None, n=0, null=("data", "parity", "reads", "out")) == fe.E_INVAL
    assert _call(hip_lib, name, b, ctx=None, n=1 << 30) == fe.E_INVAL
    # what fastecc_read_batch[_set] refuse before they read the context, with the same code
    cases = [dict(null=("data",)), dict(null=("parity",)), dict(null=("reads",)), dict(null=("out",)), dict(count=0), dict(count=0, n=0), dict(width=0),
             dict(width=0, n=0), dict(skew=("data", 2)), dict(skew=("parity", 1)), dict(skew=("out", 2)), dict(skew=("parity", 3), n=0)]
    # the device form's own: a null status, lists and status word that are not aligned
    cases += [dict(null=("status",)), dict(null=("status",), n=0), dict(skew=("status", 4)), dict(skew=("status", 2)), dict(skew=("status", 4), n=0),
              dict(skew=("reads", 4)), dict(skew=("reads", 1)), dict(skew=("reads", 4), n=0)]
    if name == "fastecc_read_batch_set_device":
        cases += [dict(null=("po",)), dict(null=("po",), n=0), dict(skew=("po", 2)), dict(skew=("po", 1)), dict(skew=("po", 3), n=0)]
    for kw in cases:
        for ctx in (None, FAKE):
            assert _call(hip_lib, name, b, ctx=ctx, **kw) == fe.E_INVAL, (kw, ctx)
    # a list above 2^24 entries: the status word's row field and the launch-splitting rule (one above the bound, and far above it)
    for n in ((1 << 24) + 1, 1 << 40, MAX):
        assert _call(hip_lib, name, b, n=n) == fe.E_UNSUPPORTED, n
    assert _call(hip_lib, name, b, n=(1 << 24) + 1, null=("status",)) == fe.E_INVAL  # (a null status first)
    assert b.untouched()  # a refused call writes nothing: `out` and the status word included


def _shell():
    """an Encoder object without a context (no device is needed to reach the argument checks)"""
    enc = fe.Encoder.__new__(fe.Encoder)
    enc._h = ctypes.c_void_p()
    enc.n, enc.k, enc.block_bytes = 6, 4, 4 * 260
    return enc


def _method(enc, method, count=1, n_reads=1, **kw):
    if method == "read_batch_set_device":
        return enc.read_batch_set_device(0, 0, count, 0, 0, n_reads, 0, 0, **kw)
    return enc.read_batch_device(0, 0, count, 0, n_reads, 0, 0, **kw)


@pytest.mark.parametrize("method", ["read_batch_set_device", "read_batch_device"])
def test_python_methods_validate_their_arguments(hip_lib, method):
    enc = _shell()
    for bad in (dict(col0=1.0), dict(col0="1"), dict(col0=None), dict(col0=True), dict(width=2.0), dict(width="8"), dict(width=False),
                dict(col0=4, width=[4]), dict(n_reads=2.0), dict(n_reads=False), dict(n_reads=None), dict(n_reads="3"), dict(count=1.0), dict(count=True),
                dict(count=None)):
        with pytest.raises(TypeError):
            _method(enc, method, **bad)
    for bad in (dict(col0=-1), dict(col0=-1, width=4), dict(col0=1 << 64, width=1), dict(width=0), dict(col0=8, width=0), dict(width=-4),
                dict(width=1 << 64), dict(col0=260), dict(col0=261), dict(n_reads=-1), dict(n_reads=1 << 64), dict(count=0), dict(count=-1),
                dict(count=1 << 64)):
        with pytest.raises(ValueError):
            _method(enc, method, **bad)
    # valid arguments reach the library, which refuses the null context: the whole block, windows, an empty list
    for good in (dict(), dict(col0=0, width=260), dict(col0=4, width=128), dict(col0=259), dict(n_reads=0), dict(n_reads=1 << 24)):
        with pytest.raises(fe.FastEccError) as e:
            _method(enc, method, **good)
        assert e.value.code == fe.E_INVAL


def test_entry_points_are_documented():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fastecc.h")).read()
    for name in NAMES:
        assert name + "(" in header
    assert "#define FASTECC_READ_NONE UINT64_MAX" in header
    assert "All or nothing: when status is non-zero, no word of out has been written by the call." in header
    assert "#define FASTECC_VERSION 460" in header
