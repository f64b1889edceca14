"""The guard bands of tests/footprint.py tested on themselves (no GPU): on torch CPU tensors (Banded with device="cpu") and on numpy
(BandedHost).  An untouched buffer passes; a write inside the payload passes check() and fails check_unchanged(); ONE stray word anywhere
in either band — its last and first words, the far end, a row band_rows - 1 rows out — fails check(), and the message names that word's
(row relative to the payload, column); stray zeros, stray field elements and a copy of the row above are caught; a skew of 0..3 words
keeps the payload where .ptr says it is."""
import re

import numpy as np
import pytest

from footprint import Banded, BandedHost

P = 0xFFF00001
P61 = (1 << 61) - 1
ROWS, S, BAND = 5, 7, 4


def payload(dtype, rows=ROWS, width=S, seed=3):
    top = P if dtype == np.uint32 else P61
    return np.random.default_rng(seed).integers(0, top, size=(rows, width), dtype=np.uint64).astype(dtype)


def make(kind, array, band_rows=BAND, row_words=None, seed=11, skew_words=0, col0=0):
    row_words = array.shape[1] if row_words is None else row_words
    if kind == "torch":
        import torch
        return Banded(torch, array, band_rows, row_words, seed, skew_words=skew_words, device="cpu", col0=col0)
    return BandedHost(array, band_rows, row_words, seed, skew_words=skew_words, col0=col0)


def poke(b, word, value):
    """one word of the allocation, by its index"""
    if isinstance(b, BandedHost):
        b.raw[word] = value
    else:
        b.raw[word] = int(np.array([value], dtype=b.dtype).view(np.int64 if b.dtype == np.uint64 else np.int32)[0])


def peek(b, word):
    return int(b._fetch(b.raw)[word])


KINDS = ["torch", "numpy"]
DTYPES = [np.uint32, np.uint64]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_an_untouched_buffer_passes_and_holds_the_array(kind, dtype):
    x = payload(dtype)
    b = make(kind, x).frozen()
    b.check("untouched")
    b.check_unchanged("untouched")
    assert np.array_equal(b.host(), x)
    assert b.view.shape == (ROWS * S,) and b.ptr % 16 == 0
    assert b.start >= BAND * S and b.total - b.end >= BAND * S
    # the bands are no constant, and another seed gives other bands
    front = b._fetch(b.raw)[: b.start]
    assert len(np.unique(front)) > len(front) // 2
    assert not np.array_equal(front, make(kind, x, seed=12)._fetch(make(kind, x, seed=12).raw)[: b.start])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_write_inside_the_payload_passes_check_and_fails_check_unchanged(kind, dtype):
    b = make(kind, payload(dtype)).frozen()
    for row, col in ((0, 0), (ROWS - 1, S - 1), (2, 3)):
        poke(b, b.word_at(row, col), peek(b, b.word_at(row, col)) ^ 1)
    b.check("payload written")
    with pytest.raises(AssertionError, match=r"3 words of a read-only buffer changed; first at \(row 0, column 0\), last at \(row %d, column %d\)" % (ROWS - 1, S - 1)):
        b.check_unchanged("payload written")


# (name, row relative to the payload, column) of the four places of one stray word
PLACES = [("the last word of the front band", -1, S - 1), ("the first word of the back band", ROWS, 0),
          ("the last word of the back band", ROWS + BAND - 1, S - 1), ("the first word of the row band_rows - 1 rows past the end", ROWS + BAND - 1, 0)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("place,row,col", PLACES)
def test_one_stray_word_is_caught_and_its_position_reported(kind, dtype, place, row, col):
    b = make(kind, payload(dtype)).frozen()
    word = b.word_at(row, col)
    assert not b.start <= word < b.end and 0 <= word < b.total, place
    poke(b, word, peek(b, word) ^ (1 << 31))
    with pytest.raises(AssertionError) as ei:
        b.check(place)
    text = str(ei.value)
    assert "1 words outside the buffer changed" in text, text
    assert re.findall(r"\(row (-?\d+), column (\d+)\)", text) == [(str(row), str(col))] * 2, text
    b.check_unchanged(place)   # the payload itself was not touched


@pytest.mark.parametrize("kind", KINDS)
def test_the_first_word_of_the_front_band_is_guarded_too(kind):
    b = make(kind, payload(np.uint32))
    word = b.word_at(-BAND, 0)
    poke(b, word, peek(b, word) + 1 & 0xFFFFFFFF)
    with pytest.raises(AssertionError, match=r"first at \(row -%d, column 0\)" % BAND):
        b.check("front of the front band")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("stray", ["zero", "p - 1", "the payload word one row earlier"])
def test_plausible_stray_values_are_caught(kind, dtype, stray):
    """What a kernel with a bound off by one row would store behind the buffer: zeros (a zero-extended row), a field element, or
    the row above shifted down.  In front of the buffer: the same."""
    x = payload(dtype)
    top = P if dtype == np.uint32 else P61
    for row in (ROWS, -1):
        b = make(kind, x)
        for col in range(S):
            value = {"zero": 0, "p - 1": top - 1}.get(stray, int(x[(row - 1) % ROWS, col]))
            poke(b, b.word_at(row, col), value)
        with pytest.raises(AssertionError, match=r"%d words outside the buffer changed.*first at \(row %d, column 0\).*last at \(row %d, column %d\)" % (S, row, row, S - 1)):
            b.check(stray)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("skew", [0, 1, 2, 3])
def test_a_skew_keeps_the_payload_where_it_says_it_is(kind, dtype, skew):
    x = payload(dtype)
    b = make(kind, x, skew_words=skew)
    item = np.dtype(dtype).itemsize
    assert (b.ptr - skew * item) % 16 == 0 and b.ptr % 16 == (skew * item) % 16
    base = b.raw.ctypes.data if kind == "numpy" else b.raw.data_ptr()
    assert b.ptr == base + b.start * item
    assert (b.view.ctypes.data if kind == "numpy" else b.view.data_ptr()) == b.ptr
    assert np.array_equal(b.host(), x)
    assert np.array_equal(b._fetch(b.raw)[b.start:b.end].reshape(ROWS, S), x)
    assert b.start >= BAND * S and b.total - b.end >= BAND * S
    b.check("skew %d" % skew)
    # a write through .view lands in the payload and nowhere else
    b.view[0] = 5
    b.view[ROWS * S - 1] = 6
    b.check("skew %d, written through the view" % skew)
    assert peek(b, b.start) == 5 and peek(b, b.end - 1) == 6


@pytest.mark.parametrize("kind", KINDS)
def test_pitch_gaps_and_columns_outside_a_window_are_band(kind):
    """A [rows, width] array in rows of row_words words at column col0: the other words of each row hold pattern and are checked."""
    x = payload(np.uint32, width=3)
    for col0 in (0, 2, 4):
        b = make(kind, x, row_words=S, col0=col0).frozen()
        assert np.array_equal(b.host(), x)
        b.check("window")
        for row in range(ROWS):   # the live columns may be written
            poke(b, b.word_at(row, col0 + 1), 0)
        b.check("window, live columns written")
        outside = col0 + 3 if col0 + 3 < S else col0 - 1
        poke(b, b.word_at(ROWS - 1, outside), peek(b, b.word_at(ROWS - 1, outside)) ^ 1)
        with pytest.raises(AssertionError, match=r"1 words outside the buffer changed.*first at \(row %d, column %d\)" % (ROWS - 1, outside)):
            b.check("window, a gap word written")


def test_a_band_has_at_least_two_rows():
    with pytest.raises(AssertionError):
        BandedHost(payload(np.uint32), 1, S, 1)
