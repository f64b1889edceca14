"""Small writes over GF((2^61-1)^2): what needs no GPU.

fastecc_gf61_code_coefficient is the generator-matrix entry the update's weight table holds, evaluated on the host.  It is checked against the
oracle's encoder on impulse stripes ((2k,k) and the padded codes) and against a brute-force Lagrange evaluation in Python integers (n = 4k / 8k).
The two device calls refuse a null context before any device is touched."""
import ctypes

import numpy as np
import pytest

import fastecc_amd as fe

P = (1 << 61) - 1


@pytest.fixture(scope="module")
def hip_lib():
    return fe.lib()


@pytest.fixture(scope="module")
def orc61():
    import oracle
    return oracle.OracleP61()


def cmul(x, y):
    return ((x[0] * y[0] - x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


def csub(x, y):
    return ((x[0] - y[0]) % P, (x[1] - y[1]) % P)


def cinv(x):
    ninv = pow((x[0] * x[0] + x[1] * x[1]) % P, P - 2, P)
    return (x[0] * ninv % P, -x[1] * ninv % P)


def cpow(x, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = cmul(r, x)
        x = cmul(x, x)
        e >>= 1
    return r


def test_symbols_exported(hip_lib):
    for name in ("fastecc_gf61_update", "fastecc_gf61_update_parity", "fastecc_gf61_code_coefficient"):
        assert hasattr(hip_lib, name), name
    assert hip_lib.fastecc_version() >= 440


def impulse_parity(orc61, order, i, value):
    """the oracle's (2 order, order) parity, one element per block, of the stripe that is `value` in block i and zero elsewhere"""
    x = np.zeros((order, 2), dtype=np.uint64)
    x[i] = value
    return [(int(r[0]), int(r[1])) for r in orc61.encode(x)]


@pytest.mark.parametrize("k", [2, 4, 8, 32])
def test_2k_k_coefficients_are_the_encoders_impulse_responses(orc61, k):
    for i in range(k):
        one, im = impulse_parity(orc61, k, i, (1, 0)), impulse_parity(orc61, k, i, (0, 1))
        for q in range(k):
            c = fe.gf61_code_coefficient(2 * k, k, i, q)
            assert c[0] < P and c[1] < P
            assert one[q] == c, (k, i, q)
            assert im[q] == cmul(c, (0, 1)), (k, i, q)  # the re / im cross terms


@pytest.mark.parametrize("n,k", [(7, 5), (20, 16), (37, 20)])
def test_padded_code_coefficients(orc61, n, k):
    """zero-extended to N = 2^ceil(log2 k) blocks; parity block j of the code is block j << fold of the (2N,N) parity"""
    m = n - k
    lg = max((k - 1).bit_length(), 1)
    order = 1 << lg
    fold = min(lg - (m - 1).bit_length(), 4)
    for i in range(k):
        one, im = impulse_parity(orc61, order, i, (1, 0)), impulse_parity(orc61, order, i, (0, 1))
        for j in range(m):
            c = fe.gf61_code_coefficient(n, k, i, j)
            assert one[j << fold] == c, (n, k, i, j)
            assert im[j << fold] == cmul(c, (0, 1)), (n, k, i, j)


@pytest.mark.parametrize("e", [2, 3])
@pytest.mark.parametrize("k", [4, 16])
def test_coset_code_coefficients_by_brute_force_lagrange(k, e):
    """n = 4k / 8k: parity block t * k + j is f(g_t w_k^j), the generators in the header's nesting order w_2k; w_4k, w_4k^3; w_8k, w_8k^3, w_8k^5,
    w_8k^7; f the polynomial of degree < k with f(w_k^i) = data block i.  L_i(y) = prod_{m != i} (y - x_m) / (x_i - x_m) in Python integers."""
    wk = fe.gf61_root(k)
    xs = [cpow(wk, i) for i in range(k)]
    gens = []
    for jj in range(1, e + 1):
        w = fe.gf61_root(k << jj)
        gens += [cpow(w, c) for c in range(1, 1 << jj, 2)]
    assert len(gens) == (1 << e) - 1
    denom_inv = []
    for i in range(k):
        d = (1, 0)
        for m in range(k):
            if m != i:
                d = cmul(d, csub(xs[i], xs[m]))
        denom_inv.append(cinv(d))
    for t, g in enumerate(gens):
        for j in range(k):
            y = cmul(g, xs[j])
            for i in range(k):
                num = (1, 0)
                for m in range(k):
                    if m != i:
                        num = cmul(num, csub(y, xs[m]))
                assert fe.gf61_code_coefficient(k << e, k, i, t * k + j) == cmul(num, denom_inv[i]), (k, e, i, t, j)


def test_code_coefficient_refusals(hip_lib):
    out = (ctypes.c_uint64 * 2)(7, 7)

    def code(n, k, i, q, o=out):
        return hip_lib.fastecc_gf61_code_coefficient(n, k, i, q, o)

    assert code(16, 8, 0, 0) == 0
    assert code(8, 8, 0, 0) == fe.E_INVAL        # n <= k
    assert code(7, 8, 0, 0) == fe.E_INVAL
    assert code(16, 8, 8, 0) == fe.E_INVAL       # data_block >= k
    assert code(16, 8, 0, 8) == fe.E_INVAL       # parity_block >= n - k
    assert code(37, 20, 0, 17) == fe.E_INVAL
    assert code(16, 8, 0, 0, None) == fe.E_INVAL  # null out
    assert code((1 << 25) + 2, (1 << 24) + 1, 0, 0) == fe.E_UNSUPPORTED  # k > 2^24
    assert code(1 << 26, 1 << 25, 0, 0) == fe.E_UNSUPPORTED
    assert code(5 + 9, 5, 0, 0) == fe.E_UNSUPPORTED   # n - k = 9 above the order 8, not 4k / 8k
    assert code(3 * 8, 8, 0, 0) == fe.E_UNSUPPORTED   # n - k = 16 above the order 8
    assert code(4 * 6, 6, 0, 0) == fe.E_UNSUPPORTED   # 4k with k no power of two: n - k = 18 above the order 8
    assert code(1 << 25, 1 << 24, (1 << 24) - 1, (1 << 24) - 1) == 0  # the largest (2k,k) code
    assert code(4 * 8, 8, 7, 23) == 0 and code(8 * 8, 8, 7, 55) == 0
    out[0] = out[1] = 7
    assert code(8, 8, 0, 0) == fe.E_INVAL and list(out) == [7, 7]  # a refused call writes nothing


def test_device_calls_refuse_a_null_context_without_a_device(hip_lib):
    words = (ctypes.c_uint64 * 8)(*([0xD0D0D0D0] * 8))
    blocks = (ctypes.c_uint64 * 1)(0)
    a = ctypes.addressof(words)
    assert hip_lib.fastecc_gf61_update(None, a, a, blocks, 1, a, None) == fe.E_INVAL
    assert hip_lib.fastecc_gf61_update_parity(None, a, blocks, 1, a, a, None) == fe.E_INVAL
    assert hip_lib.fastecc_gf61_update(None, None, None, None, 0, None, None) == fe.E_INVAL
    assert hip_lib.fastecc_gf61_update_parity(None, None, None, 0, None, None, None) == fe.E_INVAL
    assert list(words) == [0xD0D0D0D0] * 8
