"""GPU tests (-m gpu): every single-stripe entry point writes only the blocks it owns.

The other GPU tests compare the inside of a buffer with the oracle.  Here every buffer handed to a call is a tests/footprint.py Banded
allocation, [front band | payload | back band] with seeded pseudo-random bands, and after the call and a synchronise
  1. the result equals the oracle (the decoders: the original stripe),
  2. check() finds both bands of every buffer as they were, and
  3. check_unchanged() finds every buffer the header calls read-only as it was.
Each case also asserts which path ran (fastecc_plan_string, or the profile's scope names).

THE BAND RULE (band_rows below, asserted for every buffer by Buffers.add): a band has at least as many rows as the transform order the
code runs in — the next power of two >= k, or fastecc_amd.mixed_radix_order(k, pfa) —, at least as many as the parity stripe has (n = 4k /
8k), and never fewer than 2.  A store to ANY row index of the padded transform, from a bound that is off by one row or by the whole zero
extension, then still lands inside the test's own allocation, where check() names its (row, column).  The decoders of the (2k,k) layout run
transforms of 2k points: their bands are twice the order.

Bit-exact throughout.  The pool calls (their buffers end in canaries: tests/test_gpu_launch_seams.py and the batch tests) and the sharded
contexts are not covered here."""
import functools

import numpy as np
import pytest

from footprint import Banded, BandedHost
from test_gpu_cosets import oracle_parity
from test_gpu_general import expected as zero_extended_parity
from test_gpu_p32_edges import ENCODE_LOGN, MIXED_Q, PLANS, SLIM_LOGN, SLIM_PLANS, SLIM_S
from test_gpu_p32_edges import S as EDGE_S, test_the_encode_cases_reach_every_kernel_family as _families
from test_gpu_p61 import p61_oracle_coset_parity
from test_gpu_update import CODES as UPDATE_CODES

pytestmark = pytest.mark.gpu

P = 0xFFF00001
P61 = (1 << 61) - 1
S = 70          # words per block: one full wave and a ragged one
S_MFMA = 64     # vector-4 rows that the matrix-core kernel takes
S_ODD = 33
MARKER = 0xFFFFFFFF   # what a lost block, or an output that is still to be written, holds (no field element)
SEED = 0x5EED


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def fe(hip_lib):
    import fastecc_amd
    return fastecc_amd


@pytest.fixture(scope="module")
def orc61():
    import oracle
    return oracle.OracleP61()


# ------------------------------------------------------------------------------------------------
# the band rule, and the buffers of one case
# ------------------------------------------------------------------------------------------------
def band_rows(order, parity_rows=0):
    """THE BAND RULE: at least the transform order, at least the parity stripe, at least 2 rows."""
    return max(2, int(order), int(parity_rows))


def order_of(fe, k, flags=0):
    """The transform order the code of k data blocks runs in."""
    if flags & fe.CODE_MIXED_RADIX_PFA:
        return fe.mixed_radix_order(k, pfa=True)
    if flags & fe.CODE_MIXED_RADIX:
        return fe.mixed_radix_order(k)
    return max(2, 1 << (k - 1).bit_length())


class Buffers:
    """The banded buffers of one case: add() makes one and asserts the band rule for it, check() runs check() on all of them and
    check_unchanged() on the frozen ones."""

    def __init__(self, torch, what, order, parity_rows=0, factor=1):
        self.torch, self.what, self.order, self.parity_rows = torch, what, order, parity_rows
        self.band = band_rows(factor * order, parity_rows)
        self.all = []

    def add(self, name, array, frozen=False, row_words=None, skew=0, col0=0, host=False):
        array = np.asarray(array)
        row_words = array.shape[1] if row_words is None else row_words
        seed = (len(self.all) + 1) * 7919 + self.order
        b = BandedHost(array, self.band, row_words, seed, skew, col0) if host else Banded(self.torch, array, self.band, row_words, seed, skew, "cuda:0", col0)
        assert b.band_rows >= 2 and b.band_rows >= self.order and b.band_rows >= self.parity_rows, (self.what, name)   # the band rule
        assert b.start >= b.band_rows * row_words and b.total - b.end >= b.band_rows * row_words
        b.name = name
        self.all.append(b.frozen() if frozen else b)
        return b

    def check(self, step=""):
        self.torch.cuda.synchronize()
        for b in self.all:
            b.check("%s %s: %s" % (self.what, step, b.name))
            if b._snapshot is not None:
                b.check_unchanged("%s %s: %s" % (self.what, step, b.name))


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not (got == want).all():
        rows = np.flatnonzero((got != want).any(axis=1))
        raise AssertionError("%s: %d words differ, in rows %s ... %s" % (what, int((got != want).sum()), rows[:6].tolist(), rows[-3:].tolist()))


def through_the_passes(torch, enc, call):
    """Run an encode call and assert that the context's pass plan ran it.  (By default a code with at most 160 parity blocks — a (2k,k)
    code up to k = 2^7 — is encoded straight from the Lagrange basis, whatever its plan: the callers set encode_direct_max = 0.)"""
    prof, _ = profiled(torch, enc, call)
    assert prof and "direct_encode" not in prof, prof
    return prof


def marked(rows, width, dtype=np.uint32):
    return np.full((rows, width), MARKER if dtype == np.uint32 else (1 << 64) - 1, dtype=dtype)


def profiled(torch, enc, call):
    enc.profile(True)
    enc.profile_reset()
    result = call()
    torch.cuda.synchronize()
    prof = enc.profile_read()
    enc.profile(False)
    return prof, result


@functools.lru_cache(maxsize=None)
def orc():
    import oracle
    return oracle.Oracle()


@functools.lru_cache(maxsize=None)
def stripe(k, words=S):
    x = np.random.default_rng(k * 131 + words).integers(0, P, size=(k, words), dtype=np.uint64).astype(np.uint32)
    x.reshape(-1)[:4] = [0, 1, P - 1, P - 2][: min(4, x.size)]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def parity_2k(k, words=S):
    """the oracle's (2k,k) parity of stripe(k, words): computed once, shared, never written to"""
    par = orc().encode_fast(stripe(k, words))
    par.setflags(write=False)
    return par


@functools.lru_cache(maxsize=None)
def code_parity(n, k, flags, words):
    """The oracle's parity of stripe(k, words) under the (n, k) code of fastecc_create / fastecc_create_ex(flags)."""
    import fastecc_amd as fe
    x, m = stripe(k, words), n - k
    order = order_of(fe, k, flags)
    if flags & (fe.CODE_MIXED_RADIX | fe.CODE_MIXED_RADIX_PFA) and order & (order - 1):
        par = orc().encode_mixed_code(x, n, order)
    elif m > order:
        assert k == order and n in (4 * k, 8 * k)
        par = oracle_parity(orc(), x, 2 if n == 4 * k else 3)
    else:
        par = zero_extended_parity(orc(), x, m)
    par = np.ascontiguousarray(par)
    par.setflags(write=False)
    return par


# ------------------------------------------------------------------------------------------------
# encode, (2k,k) powers of two, under every plan
# ------------------------------------------------------------------------------------------------
FORMS = ("contiguous", "skewed by one word", "row pitch S + 32")


def encode_forms(torch, enc, k, words, what):
    """Out of place with the data frozen, and in place: contiguous, with data and parity skewed by one word off their 16-byte boundary, and
    with row_pitch_words = S + 32 (bands in units of the pitch, band pattern in the pitch gaps too)."""
    x, want = stripe(k, words), parity_2k(k, words)
    enc.set_option("encode_direct_max", 0)
    for form in FORMS:
        skew = 1 if form == FORMS[1] else 0
        pitch = words + 32 if form == FORMS[2] else words
        enc.set_option("row_pitch_words", pitch if form == FORMS[2] else 0)
        bufs = Buffers(torch, "%s, %s, %s" % (what, form, enc.plan()), k)
        d = bufs.add("data", x, frozen=True, row_words=pitch, skew=skew)
        out = bufs.add("parity", marked(k, words), row_words=pitch, skew=skew)
        through_the_passes(torch, enc, lambda: enc.encode(d.ptr, out.ptr))
        bufs.check("out of place")
        same(out.host(), want, bufs.what)
        bufs = Buffers(torch, "%s, %s, in place, %s" % (what, form, enc.plan()), k)
        d = bufs.add("stripe", x, row_words=pitch, skew=skew)
        through_the_passes(torch, enc, lambda: enc.encode(d.ptr))
        bufs.check()
        same(d.host(), want, bufs.what)
    enc.set_option("row_pitch_words", 0)


@pytest.mark.parametrize("plan", PLANS)
def test_encode_under_every_plan(torch_cuda, fe, plan):
    """The default plan and every id of test_every_plan_is_bit_exact at k = 2^4, 2^7, 2^11, 2^13, blocks of 70 words (which kernels these
    select: test_the_plans_reach_every_kernel_family)."""
    for logn in ENCODE_LOGN:
        k = 1 << logn
        with fe.Encoder(2 * k, k, 4 * S) as enc:
            enc.set_plan(plan)
            encode_forms(torch_cuda, enc, k, S, "encode k=2^%d plan %d" % (logn, plan))


@pytest.mark.parametrize("plan", SLIM_PLANS)
def test_encode_through_slim_outer_tiles(torch_cuda, fe, plan):
    """k = 2^16, the smallest size that plans the 16-word-per-lane outer tiles, blocks of 40 words."""
    k = 1 << SLIM_LOGN
    with fe.Encoder(2 * k, k, 4 * SLIM_S) as enc:
        enc.set_plan(plan)
        assert "S32:dif8@8" in enc.plan() and "S32:dit8@8" in enc.plan(), enc.plan()
        encode_forms(torch_cuda, enc, k, SLIM_S, "encode k=2^16 plan %d" % plan)


def test_the_plans_reach_every_kernel_family(torch_cuda, fe):
    """The two tests above run the sizes, block widths and plan ids of tests/test_gpu_p32_edges.py, whose own check reads from the contexts
    that these select register passes of 1..5 levels with 1, 2 and 4 words per lane, pair and plain MID tiles and every outer tile."""
    assert S == EDGE_S   # the same block width: the same plans
    _families(torch_cuda, fe)


# ------------------------------------------------------------------------------------------------
# zero extension and fewer parity blocks: in_rows / out_rows / final_out, and the direct encode
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,m", [(41, 12), (100, 30), (1000, 300), (1024, 64), (1024, 160), (2700, 2880), (5000, 3000)])
def test_zero_extension_and_fewer_parity_blocks(torch_cuda, fe, k, m):
    """A transform of order N over a stripe that holds k < N data blocks, or writes n - k < N parity blocks: through the pipeline
    (encode_direct_max = 0), out of place and, where n - k <= k, in place (the first n - k blocks become the parity, the others stay);
    where n - k <= 256 also straight from the Lagrange basis by the VALU and by the matrix-core kernel (64-word blocks)."""
    torch = torch_cuda
    order = order_of(fe, k)
    runs = [(0, 0, S)] + ([(256, 1, S_MFMA), (256, 2, S_MFMA)] if m <= 256 else [])
    for direct_max, kernel, words in runs:
        x, want = stripe(k, words), code_parity(k + m, k, 0, words)
        with fe.Encoder(k + m, k, 4 * words) as enc:
            enc.set_option("encode_direct_max", direct_max)
            enc.set_option("direct_kernel", kernel)
            bufs = Buffers(torch, "(%d, %d) encode_direct_max %d direct_kernel %d %s" % (k + m, k, direct_max, kernel, enc.plan()), order, m)
            d = bufs.add("data", x, frozen=True)
            out = bufs.add("parity", marked(m, words))
            prof, _ = profiled(torch, enc, lambda: enc.encode(d.ptr, out.ptr))
            assert prof and ("direct_encode" in prof) == (direct_max != 0), prof
            if kernel == 2:   # what direct.hip asks of a stripe before the matrix-core kernel takes it (it has no scope name of its own)
                assert words % 2 == 0 and words >= 32 and d.ptr % 8 == 0 and k >= 32
            bufs.check()
            same(out.host(), want, bufs.what)
            if m <= k:
                bufs = Buffers(torch, bufs.what + ", in place", order, m)
                d = bufs.add("stripe", x)
                prof, _ = profiled(torch, enc, lambda: enc.encode(d.ptr))
                assert ("direct_encode" in prof) == (direct_max != 0), prof
                bufs.check()
                same(d.host(), np.concatenate([want, x[m:]]), bufs.what)


@pytest.mark.parametrize("e", [2, 3])
@pytest.mark.parametrize("logn", [5, 6])
def test_more_parity_than_data(torch_cuda, fe, logn, e):
    """n = 4k and n = 8k: the band is as long as the whole parity stripe."""
    k = 1 << logn
    n = k << e
    x, want = stripe(k, S_ODD), code_parity(n, k, 0, S_ODD)
    with fe.Encoder(n, k, 4 * S_ODD) as enc:
        bufs = Buffers(torch_cuda, "n = %dk, k = %d %s" % (1 << e, k, enc.plan()), k, n - k)
        assert bufs.band >= n - k
        d = bufs.add("data", x, frozen=True)
        out = bufs.add("parity", marked(n - k, S_ODD))
        through_the_passes(torch_cuda, enc, lambda: enc.encode(d.ptr, out.ptr))
        bufs.check()
        same(out.host(), want, bufs.what)
        same(out.host()[:k], parity_2k(k, S_ODD), bufs.what + ": the codes nest")


# ------------------------------------------------------------------------------------------------
# mixed radix
# ------------------------------------------------------------------------------------------------
def mixed_flags(fe, q):
    return fe.CODE_MIXED_RADIX if q in fe.MIXED_RADIX_Q else fe.CODE_MIXED_RADIX_PFA


def mixed_encode(torch, fe, q, m, words, fused):
    k = q << m
    flags = mixed_flags(fe, q)
    assert order_of(fe, k, flags) == k
    x = stripe(k, words)
    want = orc().encode_mixed(x)
    with fe.Encoder(2 * k, k, 4 * words, flags=flags) as enc:
        enc.set_option("encode_direct_max", 0)
        for fuse in (1, 0):
            enc.set_option("fuse_radix", fuse)
            # R<q>+ is the odd-radix level inside the outer tile, R<q>: the radix kernel of its own around the power-of-two pipeline
            assert (("R%d+dif" % q) in enc.plan()) == bool(fused and fuse) and (("R%d:" % q) in enc.plan()) == (not (fused and fuse)), enc.plan()
            bufs = Buffers(torch, "order %d * 2^%d fuse_radix %d %s" % (q, m, fuse, enc.plan()), k)
            d = bufs.add("data", x, frozen=True)
            out = bufs.add("parity", marked(k, words))
            prof = through_the_passes(torch, enc, lambda: enc.encode(d.ptr, out.ptr))
            kind = "fused" if fused and fuse else "radix"
            assert {"%s%d_dif" % (kind, q), "%s%d_dit" % (kind, q)} <= {name.rstrip("0123456789") for name in prof}, prof
            bufs.check("out of place")
            same(out.host(), want, bufs.what)
            bufs = Buffers(torch, bufs.what + ", in place", k)
            d = bufs.add("stripe", x)
            through_the_passes(torch, enc, lambda: enc.encode(d.ptr))
            bufs.check()
            same(d.host(), want, bufs.what)


@pytest.mark.parametrize("q", MIXED_Q)
def test_mixed_radix_stand_alone_radix_kernel(torch_cuda, fe, q):
    """Order q 2^3, the smallest the odd-radix kernels of test_gpu_p32_edges.py run at; fuse_radix 0 and 1 (no fused shape this small)."""
    mixed_encode(torch_cuda, fe, q, 3, S, fused=False)


@pytest.mark.parametrize("q", [q for q in MIXED_Q if q <= 63])
def test_mixed_radix_fused_kernel(torch_cuda, fe, q):
    """Order q 2^11, the smallest at which the fused kernel is planned (q = 65, 91, 105, 117 have no fused shape), with fuse_radix 1 and,
    at the same size, 0.  33-word blocks."""
    mixed_encode(torch_cuda, fe, q, 11, S_ODD, fused=True)


@pytest.mark.parametrize("k,m,pfa", [(100, 37, False), (41, 12, True), (131, 40, True)])
def test_mixed_radix_zero_extension_and_fewer_parity_blocks(torch_cuda, fe, k, m, pfa):
    """k < order and n - k < order, for plain q and for prime-factor q, through the odd-radix kernels (encode_direct_max = 0)."""
    flags = fe.CODE_MIXED_RADIX_PFA if pfa else fe.CODE_MIXED_RADIX
    order = order_of(fe, k, flags)
    q = order // (order & -order)
    assert q > 1 and k < order and m < order and (q in fe.MIXED_RADIX_Q) == (not pfa), (order, q)
    x, want = stripe(k, S), code_parity(k + m, k, flags, S)
    with fe.Encoder(k + m, k, 4 * S, flags=flags) as enc:
        enc.set_option("encode_direct_max", 0)   # (so few parity blocks would be encoded straight from the Lagrange basis otherwise)
        for fuse in (1, 0):
            enc.set_option("fuse_radix", fuse)
            bufs = Buffers(torch_cuda, "mixed (%d, %d) order %d fuse_radix %d %s" % (k + m, k, order, fuse, enc.plan()), order, m)
            d = bufs.add("data", x, frozen=True)
            out = bufs.add("parity", marked(m, S))
            prof, _ = profiled(torch_cuda, enc, lambda: enc.encode(d.ptr, out.ptr))
            # the odd-radix kernel reads the k data blocks (in_rows) and its second run stores the n - k parity blocks (out_rows)
            assert "direct_encode" not in prof and {"radix%d_dif" % q, "radix%d_dit" % q} <= set(prof), prof
            bufs.check()
            same(out.host(), want, bufs.what)


# ------------------------------------------------------------------------------------------------
# stand-alone transform, scale_blocks, column windows, encode_batch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", [4, 9])
def test_ntt_and_scale_blocks_in_place(torch_cuda, fe, logn):
    k = 1 << logn
    x = stripe(k, S)
    with fe.Encoder(2 * k, k, 4 * S) as enc:
        for inverse in (False, True):
            bufs = Buffers(torch_cuda, "ntt k=2^%d inverse=%s" % (logn, inverse), k)
            d = bufs.add("stripe", x)
            prof, _ = profiled(torch_cuda, enc, lambda: enc.ntt(d.ptr, inverse))
            assert prof, "no kernel ran"
            bufs.check()
            same(d.host(), orc().ntt_fast(x, inverse), bufs.what)
        scale, base = orc().gf_inv(k), orc().gf_root(2 * k)
        bufs = Buffers(torch_cuda, "scale_blocks k=2^%d" % logn, k)
        d = bufs.add("stripe", x)
        prof, _ = profiled(torch_cuda, enc, lambda: enc.scale_blocks(d.ptr, scale, base))
        assert "scale_rows" in prof, prof
        bufs.check()
        same(d.host(), orc().scale_blocks(x, scale, base), bufs.what)


@pytest.mark.parametrize("col0,width", [(0, 96), (5, 18), (32, 64)])
def test_encode_columns_writes_its_window_only(torch_cuda, fe, col0, width):
    """Words [col0, col0 + width) of every block of S = 96 words at k = 2^7: the columns of the parity outside the window hold band
    pattern beforehand and still hold it afterwards."""
    k, words = 1 << 7, 96
    x, want = stripe(k, words), parity_2k(k, words)
    with fe.Encoder(2 * k, k, 4 * words) as enc:
        enc.set_option("encode_direct_max", 0)
        bufs = Buffers(torch_cuda, "encode_columns(%d, %d) %s" % (col0, width, enc.plan()), k)
        d = bufs.add("data", x, frozen=True)
        out = bufs.add("parity", marked(k, width), row_words=words, col0=col0)
        through_the_passes(torch_cuda, enc, lambda: enc.encode_columns(d.ptr, out.ptr, col0, width))
        bufs.check()
        same(out.host(), want[:, col0:col0 + width], bufs.what)


@pytest.mark.parametrize("logn", [4, 7])
def test_encode_batch_of_three_stripes(torch_cuda, fe, logn):
    k, count = 1 << logn, 3
    x = stripe(count * k, S)
    want = np.concatenate([orc().encode_fast(np.ascontiguousarray(x[b * k:(b + 1) * k])) for b in range(count)])
    with fe.Encoder(2 * k, k, 4 * S) as enc:
        enc.set_option("encode_direct_max", 0)
        bufs = Buffers(torch_cuda, "encode_batch k=2^%d %s" % (logn, enc.plan()), k)
        d = bufs.add("data", x, frozen=True)
        out = bufs.add("parity", marked(count * k, S))
        through_the_passes(torch_cuda, enc, lambda: enc.encode_batch(d.ptr, out.ptr, count))
        bufs.check("out of place")
        same(out.host(), want, bufs.what)
        bufs = Buffers(torch_cuda, bufs.what + ", in place", k)
        d = bufs.add("stripes", x)
        through_the_passes(torch_cuda, enc, lambda: enc.encode_batch(d.ptr, None, count))
        bufs.check()
        same(d.host(), want, bufs.what)


# ------------------------------------------------------------------------------------------------
# decode and repair
# ------------------------------------------------------------------------------------------------
def flags_of(lost, k, m):
    lost = np.asarray(sorted(lost), dtype=np.int64)
    dp, pp = np.ones(k, np.uint8), np.ones(m, np.uint8)
    dp[lost[lost < k]] = 0
    pp[lost[lost >= k] - k] = 0
    return dp, pp


def loss_patterns(k, m, transform, most=1 << 30):
    """One loss only (the LAST data block); then 16, 17 and 33 losses (the sweeps of 16 outputs of the direct path) and, on the transform
    path, as many as the code allows — each with block 0, the LAST data block and the LAST parity block among them."""
    rng = np.random.default_rng(k * 3 + m)
    yield [k - 1]
    for count in [16, 17, 33] + ([m] if transform else []):
        if count > min(m, most):
            continue
        must = [0, k - 1, k + m - 1]
        others = [int(b) for b in rng.permutation(k + m) if b not in must][: count - len(must)]
        lost = must + others
        if sum(b < k for b in lost) > k:
            continue
        yield lost


def decode_and_repair(torch, enc, x, par, lost, order, factor, what, prof_check):
    """The lost blocks hold MARKER.  decode: the data is the original stripe again and the parity, frozen, is as it was; repair: both are."""
    k, m = x.shape[0], par.shape[0]
    dp, pp = flags_of(lost, k, m)
    bad_x, bad_p = x.copy(), par.copy()
    bad_x[dp == 0] = MARKER
    bad_p[pp == 0] = MARKER
    enc.decode_prepare(dp, pp)
    bufs = Buffers(torch, "%s, %d lost, decode" % (what, len(lost)), order, m, factor)
    d = bufs.add("data", bad_x)
    q = bufs.add("parity", bad_p, frozen=True)
    prof, _ = profiled(torch, enc, lambda: enc.decode(d.ptr, q.ptr))
    prof_check(prof, "decode")
    bufs.check()
    same(d.host(), x, bufs.what)
    bufs = Buffers(torch, "%s, %d lost, repair" % (what, len(lost)), order, m, factor)
    d = bufs.add("data", bad_x)
    q = bufs.add("parity", bad_p)
    prof, _ = profiled(torch, enc, lambda: enc.repair(d.ptr, q.ptr))
    prof_check(prof, "repair")
    bufs.check()
    same(d.host(), x, bufs.what + ", data")
    same(q.host(), par, bufs.what + ", parity")


# (n, k, flags): (2k,k) at k = 2^6 and 2^11, zero-extended, fewer parity blocks, n = 4k, mixed radix 3 * 2^5
DECODE_CODES = [(128, 64, 0), (4096, 2048, 0), (130, 100, 0), (1024 + 64, 1024, 0), (4 * 32, 32, 0), (192, 96, 1)]
DECODE_PATHS = {"transform": (0, 0, S), "valu": (256, 1, S_ODD), "mfma": (256, 2, S_MFMA)}


@pytest.mark.parametrize("path", sorted(DECODE_PATHS))
@pytest.mark.parametrize("n,k,flags", DECODE_CODES)
def test_decode_and_repair(torch_cuda, fe, n, k, flags, path):
    """The decoder's scatter stores the lost blocks only: the transform path (decode_direct_max = 0), the direct VALU kernel and the direct
    matrix-core kernel (64-word blocks), on the patterns of loss_patterns."""
    direct_max, kernel, words = DECODE_PATHS[path]
    m = n - k
    x, par = stripe(k, words), code_parity(n, k, flags, words)
    order = order_of(fe, k, flags)

    def prof_check(prof, call):
        # (the transform path of the other layouts runs inside a context of its own, whose scopes this profile does not hold)
        assert ("direct_pass" in prof) == (path != "transform"), (path, call, prof)
        if path == "transform" and call == "decode" and (n, flags) == (2 * k, 0):
            assert "decode_transform_2k" in prof, prof

    with fe.Encoder(n, k, 4 * words, flags=flags) as enc:
        enc.set_option("decode_direct_max", direct_max)
        enc.set_option("direct_kernel", kernel)
        for lost in loss_patterns(k, m, path == "transform"):
            if path == "mfma":   # what direct.hip asks of a stripe before the matrix-core kernel takes it
                assert words % 2 == 0 and words >= 32 and k >= 32
            decode_and_repair(torch_cuda, enc, x, par, lost, order, 2, "(%d, %d) flags %d %s" % (n, k, flags, path), prof_check)


def test_split_decoder_at_its_smallest_size(torch_cuda, fe):
    """k = 2^17 with 5-word blocks, 2 % of the codeword lost (block 0, the last data block and the last parity block among them): the two
    half-size transforms, whose last pass writes the rebuilt blocks straight into the data stripe, and repair's second chain into the parity."""
    k, words = 1 << 17, 5
    x, par = stripe(k, words), parity_2k(k, words)
    lost = [0, k - 1, 2 * k - 1] + [int(b) for b in np.random.default_rng(17).permutation(2 * k)[: 2 * k // 50] if b not in (0, k - 1, 2 * k - 1)]

    def prof_check(prof, call):
        assert ("decode_split_transform" if call == "decode" else "repair_split_transform") in prof and "direct_pass" not in prof, (call, prof)

    with fe.Encoder(2 * k, k, 4 * words) as enc:
        decode_and_repair(torch_cuda, enc, x, par, lost, k, 2, "k = 2^17 split decoder", prof_check)


# ------------------------------------------------------------------------------------------------
# update
# ------------------------------------------------------------------------------------------------
# one (2k,k), one zero-extended, one n = 4k, one mixed radix (3 * 2^5), one prime-factor (21 * 2^3)
UPDATE_CASES = [(128, 64, 0), (37, 20, 0), (4 * 16, 16, 0), (96 + 40, 96, 1), (168 + 50, 168, 4)]
assert set(UPDATE_CASES) <= set(UPDATE_CODES)


@pytest.mark.parametrize("block_bytes", [8, 12, 4100])
@pytest.mark.parametrize("n,k,flags", UPDATE_CASES)
def test_update_and_update_parity(torch_cuda, fe, n, k, flags, block_bytes):
    """Read-modify-write of the parity after t = 1, 17, 40 blocks changed, block k - 1 always among them: the stripe takes the new blocks,
    the parity is the oracle's parity of the new stripe, new_blocks and old_blocks are read only; update_parity is not given the data."""
    torch = torch_cuda
    words, m = block_bytes // 4, n - k
    order = order_of(fe, k, flags)
    x, par = stripe(k, words), code_parity(n, k, flags, words)
    rng = np.random.default_rng(n + k + words)
    with fe.Encoder(n, k, block_bytes, flags=flags) as enc:
        for t in (1, 17, 40):
            if t > k:
                continue
            blocks = [k - 1] + [int(b) for b in rng.permutation(k - 1)[: t - 1]]
            new = rng.integers(0, P, size=(t, words), dtype=np.uint64).astype(np.uint32)
            after = x.copy()
            after[blocks] = new
            padded = np.zeros((order, words), dtype=np.uint32)
            padded[:k] = after
            if flags and order & (order - 1):
                want = orc().encode_mixed(padded)[:m]
            elif m > order:
                want = oracle_parity(orc(), after, 2)
            else:
                want = zero_extended_parity(orc(), after, m)
            bufs = Buffers(torch, "update (%d, %d) flags %d, %d bytes, t = %d" % (n, k, flags, block_bytes, t), order, m)
            d, q = bufs.add("data", x), bufs.add("parity", par)
            nb = bufs.add("new_blocks", new, frozen=True)
            prof, _ = profiled(torch, enc, lambda: enc.update(d.ptr, q.ptr, blocks, nb.ptr))
            assert "update_delta" in prof and "update_parity" in prof, prof
            bufs.check()
            same(d.host(), after, bufs.what + ", data")
            same(q.host(), want, bufs.what + ", parity")
            bufs = Buffers(torch, "update_parity" + bufs.what[6:], order, m)
            q = bufs.add("parity", par)
            nb, ob = bufs.add("new_blocks", new, frozen=True), bufs.add("old_blocks", x[blocks], frozen=True)
            prof, _ = profiled(torch, enc, lambda: enc.update_parity(q.ptr, blocks, nb.ptr, old=ob.ptr))
            assert "update_delta" in prof and "update_parity" in prof, prof
            bufs.check()
            same(q.host(), want, bufs.what)


# ------------------------------------------------------------------------------------------------
# verify, locate_errors, correct
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(20, 16), (256, 128)])
def test_verify_locate_and_correct(torch_cuda, fe, n, k):
    """verify and locate_errors read only (both stripes frozen), on a clean codeword and with one word wrong in the last data block and in
    the last parity block; correct rebuilds exactly those two blocks."""
    torch = torch_cuda
    m = n - k
    x, par = stripe(k, S), code_parity(n, k, 0, S)
    bad_x, bad_p = x.copy(), par.copy()
    bad_x[k - 1, S - 1] ^= 1
    bad_p[m - 1, 0] = (int(bad_p[m - 1, 0]) + 1) % P
    wrong = [k - 1, n - 1]
    with fe.Encoder(n, k, 4 * S) as enc:
        for what, cx, cp, blocks in (("clean", x, par, []), ("two blocks wrong", bad_x, bad_p, wrong)):
            bufs = Buffers(torch, "verify / locate (%d, %d), %s" % (n, k, what), k, m)
            d, q = bufs.add("data", cx, frozen=True), bufs.add("parity", cp, frozen=True)
            prof, ok = profiled(torch, enc, lambda: enc.verify(d.ptr, q.ptr, seed=SEED))
            assert ok == (not blocks) and "fingerprint" in prof, (what, prof)
            bufs.check("verify")
            prof, found = profiled(torch, enc, lambda: enc.locate_errors(d.ptr, q.ptr, seed=SEED))
            assert found == blocks and "fingerprint" in prof, (what, found, prof)
            bufs.check("locate_errors")
        bufs = Buffers(torch, "correct (%d, %d)" % (n, k), k, m, 2)
        d, q = bufs.add("data", bad_x), bufs.add("parity", bad_p)
        assert enc.correct(d.ptr, q.ptr, seed=SEED) == wrong
        bufs.check()
        same(d.host(), x, bufs.what + ", data")
        same(q.host(), par, bufs.what + ", parity")


# ------------------------------------------------------------------------------------------------
# pack / unpack
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,pitch", [(69, 0), (1024, 1056)])
def test_pack_and_unpack_follow_the_row_pitch(torch_cuda, fe, W, pitch):
    """k blocks of W arbitrary words <-> k encodable blocks of W + 1 words, the packed side contiguous and in rows of 1056 words (the gaps
    hold band pattern); the source side of either call is read only."""
    torch = torch_cuda
    k, words = 64, W + 1
    raw = np.random.default_rng(W).integers(0, 1 << 32, size=(k, W), dtype=np.uint64).astype(np.uint32)
    raw[::2, ::5] |= np.uint32(0xFFF00000)
    want = orc().pack_blocks(raw)
    with fe.Encoder(2 * k, k, 4 * words) as enc:
        enc.set_option("row_pitch_words", pitch)
        bufs = Buffers(torch, "pack_blocks W = %d pitch %d" % (W, pitch), k)
        src = bufs.add("raw", raw, frozen=True)
        dst = bufs.add("packed", marked(k, words), row_words=pitch or words)
        prof, _ = profiled(torch, enc, lambda: enc.pack_blocks(src.ptr, dst.ptr))
        assert "pack_blocks" in prof, prof
        bufs.check()
        same(dst.host(), want, bufs.what)
        bufs = Buffers(torch, "unpack_blocks W = %d pitch %d" % (W, pitch), k)
        src = bufs.add("packed", want, frozen=True, row_words=pitch or words)
        dst = bufs.add("raw", marked(k, W))
        prof, bad = profiled(torch, enc, lambda: enc.unpack_blocks(src.ptr, dst.ptr))
        assert bad == 0 and "unpack_blocks" in prof, (bad, prof)
        bufs.check()
        same(dst.host(), raw, bufs.what)


# ------------------------------------------------------------------------------------------------
# GF((2^61 - 1)^2)
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stripe61(k, elems):
    x = np.random.default_rng(k * 17 + elems).integers(0, P61, size=(k, 2 * elems), dtype=np.uint64)
    x.reshape(-1)[:2] = [0, P61 - 1]
    x.setflags(write=False)
    return x


def encoder61(fe, n, k, elems):
    return fe.Encoder(n, k, 16 * elems, field=fe.FIELD_GF_P61_SQUARED)


@pytest.mark.parametrize("elems", [1, 3, 33])
@pytest.mark.parametrize("logn", [3, 11])
def test_p61_encode(torch_cuda, fe, orc61, logn, elems):
    k = 1 << logn
    x = stripe61(k, elems)
    want = orc61.encode(x)
    with encoder61(fe, 2 * k, k, elems) as enc:
        bufs = Buffers(torch_cuda, "p61 encode k=2^%d, %d elements %s" % (logn, elems, enc.plan()), k)
        d = bufs.add("data", x, frozen=True)
        out = bufs.add("parity", marked(k, 2 * elems, np.uint64))
        prof, _ = profiled(torch_cuda, enc, lambda: enc.encode(d.ptr, out.ptr))
        assert prof and all(name.startswith("p61_") for name in prof), prof
        bufs.check("out of place")
        same(out.host(), want, bufs.what)
        bufs = Buffers(torch_cuda, bufs.what + ", in place", k)
        d = bufs.add("stripe", x)
        enc.encode(d.ptr)
        bufs.check()
        same(d.host(), want, bufs.what)


@pytest.mark.parametrize("elems", [1, 3, 33])
def test_p61_other_layouts(torch_cuda, fe, orc61, elems):
    """An any-(n,k) code — (130, 100): the strided copies of encode_device around the padded transform, out of place and in place — and n = 4k."""
    torch = torch_cuda
    k, m = 100, 30
    x = stripe61(k, elems)
    padded = np.zeros((128, 2 * elems), dtype=np.uint64)
    padded[:k] = x
    want = orc61.encode(padded)[:: 1 << min(7 - 5, 4)][:m]
    with encoder61(fe, k + m, k, elems) as enc:
        bufs = Buffers(torch, "p61 (130, 100), %d elements %s" % (elems, enc.plan()), 128, m)
        d = bufs.add("data", x, frozen=True)
        out = bufs.add("parity", marked(m, 2 * elems, np.uint64))
        enc.encode(d.ptr, out.ptr)
        bufs.check("out of place")
        same(out.host(), want, bufs.what)
        bufs = Buffers(torch, bufs.what + ", in place", 128, m)
        d = bufs.add("stripe", x)
        enc.encode(d.ptr)
        bufs.check()
        same(d.host(), np.concatenate([want, x[m:]]), bufs.what)
    k = 32
    x = stripe61(k, elems)
    with encoder61(fe, 4 * k, k, elems) as enc:
        bufs = Buffers(torch, "p61 n = 4k, k = 32, %d elements %s" % (elems, enc.plan()), k, 3 * k)
        d = bufs.add("data", x, frozen=True)
        out = bufs.add("parity", marked(3 * k, 2 * elems, np.uint64))
        enc.encode(d.ptr, out.ptr)
        bufs.check()
        same(out.host(), p61_oracle_coset_parity(orc61, x, 2), bufs.what)


@pytest.mark.parametrize("elems", [1, 3, 33])
@pytest.mark.parametrize("direct_max", [32, 0])
def test_p61_decode_and_repair_with_the_last_blocks_lost(torch_cuda, fe, orc61, elems, direct_max):
    """k = 2^7, the LAST data block and the LAST parity block lost: the direct path and the transform path (its folding MID tile shows in
    the profile)."""
    k = 1 << 7
    x = stripe61(k, elems)
    par = orc61.encode(x)

    def prof_check(prof, call):
        assert call == "repair" or ("p61_tile_mid7_fold" in prof) == (direct_max == 0), (call, prof)

    with encoder61(fe, 2 * k, k, elems) as enc:
        enc.set_option("decode_direct_max", direct_max)
        decode_and_repair(torch_cuda, enc, x, par, [k - 1, 2 * k - 1], k, 2, "p61 k=2^7, %d elements, decode_direct_max %d" % (elems, direct_max), prof_check)


@pytest.mark.parametrize("elems", [1, 3, 33])
@pytest.mark.parametrize("logn", [4, 9])
def test_p61_ntt_in_place(torch_cuda, fe, orc61, logn, elems):
    k = 1 << logn
    x = stripe61(k, elems)
    with encoder61(fe, 2 * k, k, elems) as enc:
        for inverse in (False, True):
            bufs = Buffers(torch_cuda, "p61 ntt k=2^%d, %d elements, inverse=%s" % (logn, elems, inverse), k)
            d = bufs.add("stripe", x)
            enc.ntt(d.ptr, inverse)
            bufs.check()
            same(d.host(), orc61.ntt(x, inverse), bufs.what)


# ------------------------------------------------------------------------------------------------
# host memory: FASTECC_MEM_HOST and fastecc_encode_blocks copy into the caller's heap
# ------------------------------------------------------------------------------------------------
def host_case(fe, field, n, k):
    """(encoder arguments, data, parity, words per row) of a host case in either field"""
    m = n - k
    if field == "p32":
        return dict(block_bytes=4 * S), stripe(k, S), code_parity(n, k, 0, S), S
    import oracle
    o61, elems = oracle.OracleP61(), 3
    order = order_of(fe, k)
    padded = np.zeros((order, 2 * elems), dtype=np.uint64)
    padded[:k] = stripe61(k, elems)
    fold = min((order.bit_length() - 1) - ((m - 1).bit_length() if m > 1 else 0), 4)
    return dict(block_bytes=16 * elems, field=fe.FIELD_GF_P61_SQUARED), stripe61(k, elems), o61.encode(padded)[:: 1 << fold][:m], 2 * elems


@pytest.mark.parametrize("field", ["p32", "p61"])
@pytest.mark.parametrize("n,k", [(256, 128), (130, 100)])
def test_host_stripes(torch_cuda, fe, field, n, k):
    """fastecc_encode, _decode and _repair on pageable host stripes (FASTECC_MEM_HOST: the results come back through the staging ring, two
    helper threads here) write their own rows of the caller's heap only; fastecc_update refuses host memory and writes nothing."""
    torch = torch_cuda
    kw, x, par, row = host_case(fe, field, n, k)
    m, order = n - k, order_of(fe, k)
    dtype = x.dtype
    with fe.Encoder(n, k, **kw) as enc:
        if field == "p32":   # (the 64-bit field's contexts take no such option: their ring runs with its default helpers)
            enc.set_option("stage_threads", 2)
        bufs = Buffers(torch, "host encode %s (%d, %d)" % (field, n, k), order, m)
        d = bufs.add("data", x, frozen=True, host=True)
        out = bufs.add("parity", marked(m, row, dtype), host=True)
        enc.encode(d.ptr, out.ptr, mem=fe.MEM_HOST)
        bufs.check("out of place")
        same(out.host(), par, bufs.what)
        bufs = Buffers(torch, bufs.what + ", in place", order, m)
        d = bufs.add("stripe", x, host=True)
        enc.encode(d.ptr, mem=fe.MEM_HOST)
        bufs.check()
        same(d.host(), np.concatenate([par, x[m:]]), bufs.what)
        lost = [0, k - 1, n - 1]
        dp, pp = flags_of(lost, k, m)
        bad_x, bad_p = x.copy(), par.copy()
        bad_x[dp == 0] = 11
        bad_p[pp == 0] = 13
        enc.decode_prepare(dp, pp)
        # include/fastecc.h: the 64-bit field's any-(n,k) codes decode on device memory only; a refused call writes nothing
        refused = field == "p61" and k & (k - 1) != 0
        for call in ("decode", "repair"):
            bufs = Buffers(torch, "host %s %s (%d, %d)" % (call, field, n, k), order, m, 2)
            d = bufs.add("data", bad_x, frozen=refused, host=True)
            q = bufs.add("parity", bad_p, frozen=(refused or call == "decode"), host=True)
            if refused:
                with pytest.raises(fe.FastEccError) as ei:
                    getattr(enc, call)(d.ptr, q.ptr, mem=fe.MEM_HOST)
                assert ei.value.code == fe.E_UNSUPPORTED
                bufs.check()
                continue
            getattr(enc, call)(d.ptr, q.ptr, mem=fe.MEM_HOST)
            bufs.check()
            same(d.host(), x, bufs.what + ", data")
            same(q.host(), par if call == "repair" else bad_p, bufs.what + ", parity")
        # include/fastecc.h: fastecc_update is FASTECC_MEM_DEVICE only (and GF(0xFFF00001) only); a refused call writes nothing
        bufs = Buffers(torch, "host update %s (%d, %d)" % (field, n, k), order, m)
        d, q = bufs.add("data", x, frozen=True, host=True), bufs.add("parity", par, frozen=True, host=True)
        nb = bufs.add("new_blocks", x[:1], frozen=True, host=True)
        with pytest.raises(fe.FastEccError) as ei:
            enc.update(d.ptr, q.ptr, [k - 1], nb.ptr, mem=fe.MEM_HOST)
        assert ei.value.code == fe.E_UNSUPPORTED
        bufs.check()


@pytest.mark.parametrize("field", ["p32", "p61"])
def test_encode_blocks_with_every_block_in_its_own_allocation(torch_cuda, fe, field):
    """fastecc_encode_blocks takes k block pointers and encodes in place: each block sits in a banded allocation of its own (the band
    rule for a one-row buffer whose neighbours are other allocations: 2 rows either side)."""
    k = 128
    kw, x, par, row = host_case(fe, field, 2 * k, k)
    blocks = [BandedHost(x[i:i + 1], band_rows(1), row, 1000 + i) for i in range(k)]
    assert all(b.band_rows >= 2 for b in blocks)
    with fe.Encoder(2 * k, k, **kw) as enc:
        if field == "p32":
            enc.set_option("stage_threads", 2)
        enc.encode_blocks([b.ptr for b in blocks])
        torch_cuda.cuda.synchronize()
    for i, b in enumerate(blocks):
        b.check("encode_blocks %s, block %d" % (field, i))
    same(np.concatenate([b.host() for b in blocks]), par, "encode_blocks %s" % field)
