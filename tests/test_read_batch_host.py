"""Degraded reads (fastecc_read_batch, fastecc_read_batch_set): argument checks that need no GPU.

Every refusal here happens before the context is dereferenced: a null context, null pointers, count == 0, an empty window and misaligned
pointers are FASTECC_E_INVAL with the output untouched, and the Python methods reject a bad count, list or window before the library is called."""
import ctypes

import numpy as np
import pytest

import fastecc_amd as fe


@pytest.fixture(scope="module")
def hip_lib():
    return fe.lib()


def test_symbols_exported(hip_lib):
    for name in ("fastecc_read_batch", "fastecc_read_batch_set"):
        assert hasattr(hip_lib, name), name
    assert hip_lib.fastecc_version() >= 410
    assert hasattr(fe.Encoder, "read_batch") and hasattr(fe.Encoder, "read_batch_set")


def _buffers():
    pool = np.arange(256, dtype=np.uint32)
    out = np.full(64, 0xA5A5A5A5, np.uint32)
    reads = (ctypes.c_uint64 * 2)(0, 1)
    po = (ctypes.c_uint32 * 4)(0, 0, 0, 0)
    return pool, out, reads, po


# an address in the never-mapped first page: a check that read the context before refusing would fault
FAKE = ctypes.c_void_p(0x10)


def _calls(hip_lib, set_form):
    """call(ctx, data, parity, count, pattern_of, reads, n_reads, col0, width, out) of either entry point"""
    if set_form:
        return lambda c, d, p, count, po, r, n, col0, w, o: hip_lib.fastecc_read_batch_set(c, d, p, count, po, r, n, col0, w, o, None)
    return lambda c, d, p, count, po, r, n, col0, w, o: hip_lib.fastecc_read_batch(c, d, p, count, r, n, col0, w, o, None)


@pytest.mark.parametrize("set_form", [True, False])
def test_null_and_misaligned_arguments_are_inval(hip_lib, set_form):
    call = _calls(hip_lib, set_form)
    pool, out, reads, po = _buffers()
    want = out.copy()
    d, p, o = pool.ctypes.data, pool.ctypes.data + 512, out.ctypes.data
    assert call(None, d, p, 1, po, reads, 2, 0, 4, o) == fe.E_INVAL          # no context
    assert call(None, None, None, 0, None, None, 0, 0, 0, None) == fe.E_INVAL
    for ctx in (None, FAKE):
        assert call(ctx, None, p, 1, po, reads, 2, 0, 4, o) == fe.E_INVAL    # no data
        assert call(ctx, d, None, 1, po, reads, 2, 0, 4, o) == fe.E_INVAL    # no parity
        assert call(ctx, d, p, 1, po, None, 2, 0, 4, o) == fe.E_INVAL        # no reads
        assert call(ctx, d, p, 1, po, reads, 2, 0, 4, None) == fe.E_INVAL    # no out
        assert call(ctx, d, p, 0, po, reads, 2, 0, 4, o) == fe.E_INVAL       # count 0
        assert call(ctx, d, p, 1, po, reads, 2, 0, 0, o) == fe.E_INVAL       # an empty window
        assert call(ctx, d + 2, p, 1, po, reads, 2, 0, 4, o) == fe.E_INVAL   # misaligned data
        assert call(ctx, d, p + 1, 1, po, reads, 2, 0, 4, o) == fe.E_INVAL   # misaligned parity
        assert call(ctx, d, p, 1, po, reads, 2, 0, 4, o + 2) == fe.E_INVAL   # misaligned out
        assert call(ctx, d, p + 3, 1, po, reads, 0, 0, 4, o) == fe.E_INVAL   # ... also with an empty list
        if set_form:
            assert call(ctx, d, p, 1, None, reads, 2, 0, 4, o) == fe.E_INVAL  # no pattern_of
            assert call(ctx, d, p, 1, None, reads, 0, 0, 4, o) == fe.E_INVAL
    assert np.array_equal(out, want)
    assert np.array_equal(pool, np.arange(256, dtype=np.uint32))


def _shell(n=6, k=4, block_bytes=64):
    """an Encoder object without a context (no device is needed to reach the argument checks)"""
    enc = fe.Encoder.__new__(fe.Encoder)
    enc._h = ctypes.c_void_p()
    enc.n, enc.k, enc.block_bytes = n, k, block_bytes
    return enc


@pytest.mark.parametrize("method", ["read_batch_set", "read_batch"])
def test_python_methods_validate_before_the_library(hip_lib, method):
    enc = _shell()
    pool, out, _, _ = _buffers()
    want = out.copy()

    def call(count=2, pattern_of=(0, fe.PATTERN_NONE), reads=(0, 5), **kw):
        fn = getattr(enc, method)
        if method == "read_batch_set":
            return fn(pool, pool[128:], count, pattern_of, reads, out, **kw)
        return fn(pool, pool[128:], count, reads, out, **kw)

    for bad in (0, -1, 1 << 64):
        with pytest.raises(ValueError):
            call(count=bad, pattern_of=[0])
    for bad in (1.0, "3", None, True):
        with pytest.raises(TypeError):
            call(count=bad, pattern_of=[0])
    if method == "read_batch_set":
        for bad in ([], [0, 1, 2], [-1, 0], [0, 1 << 32]):
            with pytest.raises(ValueError):
                call(pattern_of=bad)
    for bad in ([-1], [1 << 64]):
        with pytest.raises(ValueError):
            call(reads=bad)
    for bad in (dict(col0=-1), dict(width=0), dict(width=-4), dict(col0=16), dict(col0=20)):  # (16 words per block: nothing left from col0 on)
        with pytest.raises(ValueError):
            call(**bad)
    for bad in (dict(col0=1.0), dict(width="4"), dict(col0=True)):
        with pytest.raises(TypeError):
            call(**bad)
    for good in (dict(), dict(col0=3, width=5), dict(col0=15), dict(reads=np.array([7, 7, 0], np.uint64)), dict(reads=[])):
        with pytest.raises(fe.FastEccError) as e:  # valid arguments reach the library, which refuses the null context
            call(**good)
        assert e.value.code == fe.E_INVAL
    assert np.array_equal(out, want)
