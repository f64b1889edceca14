"""Guard bands around a buffer: does a call write only the words it may write?

A result test compares the inside of a buffer with the oracle; a store one row, or one lane vector, past the buffer lands in the allocator's
slack or in a neighbouring allocation and no such test sees it.  Here a buffer is ONE allocation laid out as

    [front band | payload | back band]

with the payload on a 16-byte boundary plus `skew_words` words.  Both bands hold position-dependent pseudo-random words (a seeded numpy
generator; full-range words, so a stray zero, a stray field element and a shifted copy of the data all differ from the band with probability
1 - 2^-32 per word).  A second copy of the whole allocation is kept as the expectation; check() compares the bands with it and, on failure,
names how many words changed and the first and last changed position as (row relative to the payload, column): row -1 is the row in front
of the payload, row `rows` the first one behind it.

The payload is `rows` rows of `row_words` words.  Where the array handed in has fewer columns than `row_words` (a row pitch), or sits at
`col0` of the row (a column window), the other words of every row hold band pattern too and check() covers them.

Banded is over one torch tensor (any device), BandedHost over one numpy array; a word is a uint32, or a uint64 for the 64-bit field.
frozen() / check_unchanged() snapshot the payload for calls that only read it.  Plain helper module (no fixtures, no tests), like
tests/p32_edges.py; nothing of the library is used."""
import numpy as np


class _Bands:
    """The layout and the checks; the two subclasses say how the allocation is made, compared and fetched."""

    def __init__(self, array, band_rows, row_words, seed, skew_words=0, col0=0):
        array = np.asarray(array)
        assert array.dtype in (np.uint32, np.uint64), "words are uint32, or uint64 for the 64-bit field"
        if array.ndim != 2:
            assert array.size % row_words == 0, "the payload is whole rows"
            array = array.reshape(-1, row_words)
        self.dtype = array.dtype
        self.rows, self.width = array.shape
        self.band_rows, self.row_words, self.col0, self.skew_words = int(band_rows), int(row_words), int(col0), int(skew_words)
        assert self.band_rows >= 2, "a band is never fewer than 2 rows"
        assert 0 <= self.col0 and self.col0 + self.width <= self.row_words and self.skew_words >= 0
        self.band_words = self.band_rows * self.row_words
        self.payload_words = self.rows * self.row_words
        item = self.dtype.itemsize
        lead = 16 // item + self.skew_words          # room for the alignment and the skew, in front of the front band
        total = lead + 2 * self.band_words + self.payload_words
        rng = np.random.default_rng(seed)
        image = rng.integers(0, 1 << (8 * item), size=total, dtype=np.uint64 if item == 8 else np.uint32, endpoint=False)
        base = self._allocate(total)                 # the address of word 0
        assert base % item == 0
        align = (-(base + self.band_words * item) % 16) // item
        self.start = align + self.skew_words + self.band_words      # word index of the payload
        self.end = self.start + self.payload_words
        assert self.start - self.band_words >= 0 and self.end + self.band_words <= total
        assert (base + self.start * item - self.skew_words * item) % 16 == 0
        self.total = total
        image[self.start:self.end].reshape(self.rows, self.row_words)[:, self.col0:self.col0 + self.width] = array
        self._fill(image)
        self.ptr = base + self.start * item
        self._snapshot = None

    # ---- positions ----
    def position(self, word):
        """(row relative to the payload, column) of word index `word` of the allocation"""
        off = int(word) - self.start
        return off // self.row_words, off % self.row_words

    def word_at(self, row, col):
        """word index in the allocation (.raw) of (row relative to the payload, column)"""
        return self.start + row * self.row_words + col

    def _guard_slices(self):
        """the guarded parts as (flat slice of the allocation) and, for the gaps in the payload rows, column ranges"""
        return [slice(0, self.start), slice(self.end, self.total)], [c for c in ((0, self.col0), (self.col0 + self.width, self.row_words)) if c[0] < c[1]]

    # ---- checks ----
    def check(self, what=""):
        """Every word outside the payload's live columns still holds its pattern."""
        flats, cols = self._guard_slices()
        ok = all(self._same(self.raw[s], self.expected[s]) for s in flats)
        if ok and cols:
            got, want = self._rows(self.raw), self._rows(self.expected)
            ok = all(self._same(got[:, a:b], want[:, a:b]) for a, b in cols)
        if ok:
            return
        got, want = self._fetch(self.raw), self._fetch(self.expected)
        guarded = np.ones(self.total, dtype=bool)
        guarded[self.start:self.end].reshape(self.rows, self.row_words)[:, self.col0:self.col0 + self.width] = False
        bad = np.flatnonzero((got != want) & guarded)
        first, last = self.position(bad[0]), self.position(bad[-1])
        raise AssertionError("%s: %d words outside the buffer changed (its rows are 0..%d, its columns %d..%d of %d); first at (row %d, column %d) = %#x, "
                             "last at (row %d, column %d) = %#x" % (what, len(bad), self.rows - 1, self.col0, self.col0 + self.width - 1, self.row_words,
                                                                    first[0], first[1], int(got[bad[0]]), last[0], last[1], int(got[bad[-1]])))

    def frozen(self):
        """Snapshot the payload for a call that only reads it: check_unchanged() compares with it.  Returns self."""
        self._snapshot = self._copy(self.view)
        return self

    def check_unchanged(self, what=""):
        assert self._snapshot is not None, "frozen() first"
        if self._same(self.view, self._snapshot):
            return
        got, want = self._fetch(self.view), self._fetch(self._snapshot)
        bad = np.flatnonzero(got != want)
        raise AssertionError("%s: %d words of a read-only buffer changed; first at (row %d, column %d), last at (row %d, column %d)"
                             % ((what, len(bad)) + divmod(int(bad[0]), self.row_words) + divmod(int(bad[-1]), self.row_words)))

    def host(self):
        """The live columns of the payload as a numpy array [rows, width]."""
        return self._fetch(self.view).reshape(self.rows, self.row_words)[:, self.col0:self.col0 + self.width].copy()


class Banded(_Bands):
    """[front band | payload | back band] in one torch tensor.  .view is the payload (flat, rows * row_words words, a view into the
    allocation), .ptr its address, .raw the whole allocation, .expected the second tensor with what .raw held at the start."""

    def __init__(self, torch, array, band_rows, row_words, seed, skew_words=0, device="cuda:0", col0=0):
        self.torch, self.device = torch, device
        super().__init__(array, band_rows, row_words, seed, skew_words, col0)

    def _allocate(self, total):
        self.raw = self.torch.empty(total, dtype=self.torch.int64 if self.dtype == np.uint64 else self.torch.int32, device=self.device)
        return self.raw.data_ptr()

    def _fill(self, image):
        signed = self.torch.from_numpy(image.view(np.int64 if self.dtype == np.uint64 else np.int32))
        self.raw.copy_(signed)
        self.expected = signed.to(self.device).clone()
        self.view = self.raw[self.start:self.end]
        assert self.view.data_ptr() == self.raw.data_ptr() + self.start * self.dtype.itemsize

    def _rows(self, t):
        return t[self.start:self.end].view(self.rows, self.row_words)

    def _same(self, a, b):
        return self.torch.equal(a, b)

    def _copy(self, t):
        return t.clone()

    def _fetch(self, t):
        return t.cpu().numpy().view(self.dtype)


class BandedHost(_Bands):
    """The same over one numpy allocation, for the calls that take host memory.  .view is the payload (flat numpy view), .ptr its address."""

    def __init__(self, array, band_rows, row_words, seed, skew_words=0, col0=0):
        super().__init__(array, band_rows, row_words, seed, skew_words, col0)

    def _allocate(self, total):
        self.raw = np.empty(total, dtype=self.dtype)
        return self.raw.ctypes.data

    def _fill(self, image):
        self.raw[:] = image
        self.expected = image.astype(self.dtype, copy=True)
        self.view = self.raw[self.start:self.end]
        assert self.view.ctypes.data == self.raw.ctypes.data + self.start * self.dtype.itemsize

    def _rows(self, a):
        return a[self.start:self.end].reshape(self.rows, self.row_words)

    def _same(self, a, b):
        return np.array_equal(a, b)

    def _copy(self, a):
        return a.copy()

    def _fetch(self, a):
        return np.asarray(a).view(self.dtype)
