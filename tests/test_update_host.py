"""Parity update (fastecc_update / _update_parity): the host-side pieces, no GPU.

fastecc_code_coefficient is the generator-matrix entry L_i(y_q) that the update kernels read from their shift table.  Here it is checked
against brute-force Lagrange interpolation in Python integers, with the evaluation points written down from fastecc_create's
description of each code (not from the library's position formula), and for (2k,k) against the oracle's encode of unit impulses."""
import ctypes

import numpy as np
import pytest

import fastecc_amd as fe

P = fe.P


@pytest.fixture(scope="module")
def hip_lib():
    return fe.lib()


def root(order):
    assert (P - 1) % order == 0
    return pow(19, (P - 1) // order, P)


def lagrange(N, i, y):
    """L_i(y) on the N data points w_N^j (every one a node: zero-extended blocks are known zeros)."""
    w = root(N)
    xs = [pow(w, j, P) for j in range(N)]
    num = den = 1
    for j, x in enumerate(xs):
        if j != i:
            num = num * (y - x) % P
            den = den * (xs[i] - x) % P
    return num * pow(den, P - 2, P) % P


def parity_points(n, k, N, fold=0):
    """y_q of fastecc_create's codes: (2N,N) sub-cosets w_2N^(2 (q << fold) + 1), or the cosets of n = 4k / 8k in nesting order."""
    m = n - k
    if n in (4 * k, 8 * k) and k == N:
        gens = [root(2 * k), root(4 * k), pow(root(4 * k), 3, P)] + [pow(root(8 * k), c, P) for c in (1, 3, 5, 7)]
        wk = root(k)
        return [gens[q // k] * pow(wk, q % k, P) % P for q in range(m)]
    w2 = root(2 * N)
    return [pow(w2, 2 * (q << fold) + 1, P) for q in range(m)]


def coef(n, k, i, q, flags=0):
    return fe.code_coefficient(n, k, i, q, flags)


# (n, k, flags, N, fold): (2k,k) at k = 8 and 64; n = k + N/4; 4k; 8k; zero-extended (37,20) and (1100,1000); mixed radix 3 * 2^5;
# PFA 21 * 2^3
CODES = [(16, 8, 0, 8, 0), (128, 64, 0, 64, 0), (64 + 16, 64, 0, 64, 2), (4 * 16, 16, 0, 16, 0), (8 * 8, 8, 0, 8, 0), (37, 20, 0, 32, 0),
         (1100, 1000, 0, 1024, 3), (96 + 40, 96, fe.CODE_MIXED_RADIX, 96, 0), (168 + 50, 168, fe.CODE_MIXED_RADIX_PFA, 168, 0)]


def test_update_symbols_exported(hip_lib):
    for name in ("fastecc_update", "fastecc_update_parity", "fastecc_code_coefficient"):
        assert hasattr(hip_lib, name), name
    assert hip_lib.fastecc_version() >= 310


@pytest.mark.parametrize("n,k,flags,N,fold", CODES)
def test_code_coefficient_is_the_lagrange_basis(n, k, flags, N, fold):
    assert fe.mixed_radix_order(k, pfa=bool(flags & fe.CODE_MIXED_RADIX_PFA)) == N if flags else True
    ys = parity_points(n, k, N, fold)
    rng = np.random.default_rng(n * 1000 + k)
    pairs = {(0, 0), (k - 1, n - k - 1), (k // 2, (n - k) // 2)}
    pairs |= {(int(rng.integers(k)), int(rng.integers(n - k))) for _ in range(12)}
    for i, q in sorted(pairs):
        assert coef(n, k, i, q, flags) == lagrange(N, i, ys[q]), (i, q)


@pytest.mark.parametrize("k", [8, 64])
def test_code_coefficient_full_matrix_equals_the_oracle_encode_of_impulses(oracle, k):
    """(2k,k): column i of the generator matrix is the encode of a unit impulse at block i (1-word blocks)."""
    for i in range(k):
        x = np.zeros((k, 1), np.uint32)
        x[i, 0] = 1
        want = oracle.encode(x)[:, 0]
        got = [coef(2 * k, k, i, q) for q in range(k)]
        assert got == [int(v) for v in want], i


def test_code_coefficient_shift_structure():
    """The weight depends only on the difference of positions: in (2k,k), moving data and parity block by one keeps it."""
    n, k = 128, 64
    for i, q in [(0, 0), (5, 9), (62, 3)]:
        assert coef(n, k, i, q) == coef(n, k, i + 1, q + 1)


def test_top_radix2_is_the_plain_code():
    k = 1 << 12
    for i, q in [(0, 0), (17, 4000), (4095, 1)]:
        assert coef(2 * k, k, i, q, fe.CODE_TOP_RADIX2) == coef(2 * k, k, i, q)


def test_code_coefficient_refusals(hip_lib):
    out = ctypes.c_uint32(7)
    assert hip_lib.fastecc_code_coefficient(16, 8, 0, 0, 0, None) == fe.E_INVAL
    assert hip_lib.fastecc_code_coefficient(16, 8, 0, 8, 0, ctypes.byref(out)) == fe.E_INVAL  # data block >= k
    assert hip_lib.fastecc_code_coefficient(16, 8, 0, 0, 8, ctypes.byref(out)) == fe.E_INVAL  # parity block >= n - k
    assert hip_lib.fastecc_code_coefficient(8, 8, 0, 0, 0, ctypes.byref(out)) == fe.E_INVAL   # n <= k
    assert hip_lib.fastecc_code_coefficient(16, 8, 64, 0, 0, ctypes.byref(out)) == fe.E_INVAL  # unknown flag
    assert hip_lib.fastecc_code_coefficient(3 << 20, 1 << 20, 0, 0, 0, ctypes.byref(out)) == fe.E_UNSUPPORTED  # k > 2^19
    assert hip_lib.fastecc_code_coefficient(100, 10, 0, 0, 0, ctypes.byref(out)) == fe.E_UNSUPPORTED  # n - k > N
    assert out.value == 7
    with pytest.raises(fe.FastEccError):
        fe.code_coefficient(16, 8, 0, 99)


def test_update_argument_validation_without_device(hip_lib):
    """A null context, null pointers with count > 0 and misaligned pointers are refused before the context is read."""
    buf = (ctypes.c_uint32 * 64)()
    a = ctypes.addressof(buf)
    blocks = (ctypes.c_uint64 * 2)(0, 1)
    D = fe.MEM_DEVICE
    assert hip_lib.fastecc_update(None, a, a, blocks, 2, a, D, None) == fe.E_INVAL
    assert hip_lib.fastecc_update_parity(None, a, blocks, 2, a, a, D, None) == fe.E_INVAL
    fake = ctypes.c_void_p(a)  # never dereferenced: every check below fails before the context is read
    assert hip_lib.fastecc_update(fake, None, a, blocks, 2, a, D, None) == fe.E_INVAL
    assert hip_lib.fastecc_update(fake, a, None, blocks, 2, a, D, None) == fe.E_INVAL
    assert hip_lib.fastecc_update(fake, a, a, None, 2, a, D, None) == fe.E_INVAL
    assert hip_lib.fastecc_update(fake, a, a, blocks, 2, None, D, None) == fe.E_INVAL
    assert hip_lib.fastecc_update(fake, a + 2, a, blocks, 2, a, D, None) == fe.E_INVAL
    assert hip_lib.fastecc_update(fake, a, a, blocks, 2, a, 7, None) == fe.E_INVAL
    assert hip_lib.fastecc_update_parity(fake, None, blocks, 2, a, a, D, None) == fe.E_INVAL
    assert hip_lib.fastecc_update_parity(fake, a, None, 2, a, a, D, None) == fe.E_INVAL
    assert hip_lib.fastecc_update_parity(fake, a, blocks, 2, a, None, D, None) == fe.E_INVAL
    assert hip_lib.fastecc_update_parity(fake, a, blocks, 2, a + 1, a, D, None) == fe.E_INVAL
    assert hip_lib.fastecc_update_parity(fake, a, blocks, 2, None, a + 3, D, None) == fe.E_INVAL
