"""GPU tests (-m gpu) of the pool calls at the sizes where ONE call becomes SEVERAL launches (tests/launch_seams.py has the table of limits and
the periodic pool).  Every later launch of a launcher gets a base — a first lane group, a first entry, a first output row, a first segment, a
first write, a first stripe — that no smaller pool ever uses; a wrong base, a seam inside an entry or a truncated 32-bit wave count gives
words that differ from the oracle's periodic pool.

Every comparison is torch.equal (or launch_seams.equal_periodic on the 8 GiB pools) of the WHOLE pool on the device: blocks named lost hold
0xA5A5A5A5 before the call and the truth after it, FASTECC_PATTERN_NONE stripes hold garbage that must stay, every buffer a call writes ends in
a canary stripe or row, and what a call only reads is compared with a clone taken before.  Each test asserts, next to the call, that its shape
crosses its seam and by how much.

Every test prints its wall time and peak device memory (pytest -s); DESIGN.md section 29 has one run's figures."""
import time

import numpy as np
import pytest

import launch_seams as ls
from launch_seams import CANARY, LOST, T

pytestmark = pytest.mark.gpu

NEED_FREE = 20  # GiB: the 8 GiB + 4 GiB pools of cases e and f
NEED_FREE_B = 24  # GiB: case b holds the 8.7 GB pool as the expectation and as the copy a call works on, and the parity once more


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def fe(hip_lib):
    import fastecc_amd
    return fastecc_amd


@pytest.fixture(autouse=True)
def measured(request, torch_cuda):
    """prints the test's wall time and peak device memory (pytest -s shows it)"""
    torch = torch_cuda
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print("\n[launch seams] %s: %.1f s, peak %.1f GiB" % (request.node.name, time.perf_counter() - t0, torch.cuda.max_memory_allocated() / 2**30))
    torch.cuda.empty_cache()


def need_memory(torch, gib=NEED_FREE):
    free, _ = torch.cuda.mem_get_info()
    if free < gib << 30:
        pytest.skip("needs %d GiB of free HBM, %.1f GiB are free" % (gib, free / 2**30))


def tiles(torch, oracle, n, k, S, seed):
    """device tiles (T, k, S) and (T, n - k, S): T random stripes and the oracle's parity of them (one call)"""
    x = ls.draw_tile(seed, k, S)
    return ls.to_device(torch, ls.tile_to_stripes(x, S)), ls.to_device(torch, ls.tile_to_stripes(ls.tile_parity(oracle, n, k, x), S))


def pool_scopes(enc):
    """{scope: launches} of fastecc_encode_pool's own profile scopes"""
    return {name: v[1] for name, v in enc.profile_read().items() if name.startswith("encode_pool_")}


def garbage(torch, shape, seed):
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    return torch.randint(-(1 << 31), 1 << 31, shape, dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32)


# ---- a, b: the set kernel ----
ONE_LOSS_6_4 = [([j], []) for j in range(4)] + [([], [0]), ([], [1])]                       # pad class 1; the first four lose data
TWO_LOSS_6_4 = [([0], [0]), ([1], [1]), ([2], [0]), ([3], [1]), ([0], [1]), ([2], [1])]  # pad class 2: one data and one parity block each
ONE_LOSS_3_2 = [([0], []), ([1], []), ([], [0])]


def set_case(torch, fe, oracle, shape, patterns, eb, seed):
    """repair_batch_set over every pattern, then decode_batch_set over the patterns that lose data (decode has no work for the others), each on a
    fresh copy of the periodic pool with the lost blocks preset and every 97th stripe garbage under FASTECC_PATTERN_NONE"""
    n, k, S, count = shape["n"], shape["k"], shape["S"], shape["count"]
    m = n - k
    tile_d, tile_p = tiles(torch, oracle, n, k, S, seed)
    want_d, want_p = ls.periodic_pool(torch, tile_d, count), ls.periodic_pool(torch, tile_p, count)
    b = torch.arange(count, device="cuda:0")
    none = (b % ls.NONE_EVERY) == 0
    skipped = none.nonzero().squeeze(1)
    want_d[skipped] = garbage(torch, (len(skipped), k, S), seed + 1)  # not touched by either call: the expectation holds the same garbage
    want_p[skipped] = garbage(torch, (len(skipped), m, S), seed + 2)
    work = count - len(skipped)
    wpe = ls.set_waves_per_entry(eb, S)
    assert work == ls.with_work(count) and work > ls.SET_LAUNCH_WAVES // wpe + 1000, "the class's entries take a second launch"
    with_data = [q for q, (ld, _) in enumerate(patterns) if ld]
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.decode_prepare_set(*ls.flag_rows(k, m, patterns))
        for op, use in (("repair", list(range(len(patterns)))), ("decode", with_data)):
            po = torch.tensor(use, device="cuda:0")[b % len(use)]
            po[none] = -1
            D, Q = want_d.clone(), want_p.clone()
            for q, (ld, lp) in enumerate(patterns):
                rows = (po == q).nonzero().squeeze(1)
                for j in ld:
                    D[rows, j] = LOST
                for j in lp:
                    Q[rows, j] = LOST
            pattern_of = po.cpu().numpy().astype(np.int64)
            pattern_of[pattern_of < 0] = fe.PATTERN_NONE
            pattern_of = pattern_of.astype(np.uint32)
            assert int((pattern_of != fe.PATTERN_NONE).sum()) == work
            before = pattern_of.copy()
            parity_before = Q.clone() if op == "decode" else None
            getattr(enc, op + "_batch_set")(D, Q, count, pattern_of)
            torch.cuda.synchronize()
            assert np.array_equal(pattern_of, before)
            assert torch.equal(D, want_d), "%s_batch_set: the data pool (lost blocks rebuilt, skipped stripes and the canary stripe untouched)" % op
            if op == "repair":
                assert torch.equal(Q, want_p), "repair_batch_set: the parity pool"
            else:
                assert torch.equal(Q, parity_before), "decode_batch_set wrote the parity pool"
            del D, Q, parity_before


@pytest.mark.parametrize("name,patterns,eb", [("one_loss", ONE_LOSS_6_4, 1), ("two_loss", TWO_LOSS_6_4, 2)])
def test_a_set_kernel_one_wave_per_entry(torch_cuda, fe, oracle, name, patterns, eb):
    """(6,4) x 4 B: an entry is one wave, a launch holds 2^24 entries (direct_run_set: a.entries = entries + e0)"""
    assert ls.set_waves_per_entry(eb, ls.SET_A["S"]) == 1
    set_case(torch_cuda, fe, oracle, ls.SET_A, patterns, eb, seed=101 + eb)


def test_b_set_kernel_three_waves_per_entry(torch_cuda, fe, oracle):
    """(3,2) x 516 B: odd S, so one word per lane and three waves per entry — a launch holds floor(2^24 / 3) entries and ends inside wave 2^24 - 1"""
    need_memory(torch_cuda, NEED_FREE_B)
    assert ls.set_waves_per_entry(1, ls.SET_B["S"]) == 3 and ls.SET_LAUNCH_WAVES % 3 != 0
    set_case(torch_cuda, fe, oracle, ls.SET_B, ONE_LOSS_3_2, 1, seed=201)


# ---- c: reads ----
@pytest.mark.parametrize("col0,width,wpe", [(c, w, v) for (c, w), v in zip(ls.READ_WINDOWS, (1, 3))])
def test_c_reads(torch_cuda, fe, oracle, col0, width, wpe):
    """(20,16) x 768 B, 64 stripes, rotated placement with one device down: more requests than a launch holds, walking the pool's blocks with a
    stride coprime to their number (direct_run_read: a.entries and a.row_base = e0 — a second launch that wrote from row 0 is what this catches)"""
    torch = torch_cuda
    n, k, S, count = (ls.READ[x] for x in ("n", "k", "S", "count"))
    m, blocks = n - k, ls.READ["count"] * ls.READ["k"]
    assert ls.read_waves_per_entry(S, col0, width) == wpe
    n_reads = ls.SET_LAUNCH_WAVES // wpe + ls.READ["extra"]
    assert n_reads - ls.SET_LAUNCH_WAVES // wpe == 37, "37 requests belong to the second launch"
    x = ls.draw_tile(301, k, S, period=count)
    truth_d = ls.to_device(torch, ls.tile_to_stripes(x, S))
    truth_p = ls.to_device(torch, ls.tile_to_stripes(ls.tile_parity(oracle, n, k, x), S))
    reads = (np.arange(n_reads, dtype=np.uint64) * np.uint64(ls.READ["stride"])) % np.uint64(blocks)
    reads_before = reads.copy()
    window = truth_d.view(blocks, S)[:, col0:col0 + width].contiguous()
    want = torch.cat([window[torch.from_numpy(reads.astype(np.int64)).to("cuda:0")], torch.full((1, width), CANARY, dtype=torch.int32, device="cuda:0")])
    del window

    def lose(lost_of):
        """the pool with stripe b's blocks lost_of(b) preset"""
        D, Q = truth_d.clone(), truth_p.clone()
        for b in range(count):
            for j in lost_of(b):
                (D[b, j] if j < k else Q[b, j - k])[:] = LOST
        return D, Q

    def check(call, D, Q, what):
        D0, Q0 = D.clone(), Q.clone()
        out = torch.full((n_reads + 1, width), CANARY, dtype=torch.int32, device="cuda:0")
        call(D, Q, out)
        torch.cuda.synchronize()
        assert torch.equal(out, want), what + ": the rows (present blocks copied, lost blocks rebuilt, the canary row untouched)"
        assert torch.equal(D, D0) and torch.equal(Q, Q0) and np.array_equal(reads, reads_before), what + " wrote what it only reads"

    with fe.Encoder(n, k, 4 * S) as enc:
        # stripe b keeps block j on device (j + b) mod n; pattern q = the blocks of a stripe with b mod n == q that the down device held
        down = ls.READ["down"]
        patterns = [([(down - q) % n], []) if (down - q) % n < k else ([], [(down - q) % n - k]) for q in range(n)]
        enc.decode_prepare_set(*ls.flag_rows(k, m, patterns))
        pattern_of = (np.arange(count) % n).astype(np.uint32)
        D, Q = lose(lambda b: [(down - b) % n])
        r = reads.astype(np.int64)
        lost_requests = int(((down - r // k) % n == r % k).sum())  # block i of stripe b is lost iff (down - b) mod n == i
        assert 0 < lost_requests < n_reads and len(np.unique(reads[-37:])) == 37
        check(lambda D, Q, out: enc.read_batch_set(D, Q, count, pattern_of, reads, out, col0=col0, width=width), D, Q, "read_batch_set")
        # one pattern for every stripe: data block 5 and parity block 1 lost
        dp, pp = ls.flag_rows(k, m, [([5], [1])])
        enc.decode_prepare(dp[0], pp[0])
        D, Q = lose(lambda b: [5, k + 1])
        check(lambda D, Q, out: enc.read_batch(D, Q, count, reads, out, col0=col0, width=width), D, Q, "read_batch")


# ---- d: small writes ----
def test_d_small_writes(torch_cuda, fe, oracle):
    """(6,4) x 4 B: burst 1 writes one block of EVERY stripe — more segments than a launch of update_batch_kernel holds (a.segs + s0 * (SEG_HEAD +
    T)) and more writes than a launch of update_scatter_kernel holds (sa.list + w0 * LIST_WORDS); burst 2 writes two blocks of every third stripe
    (length class 2); update_parity_batch repeats burst 1 on the parity alone, with the old blocks given"""
    torch = torch_cuda
    n, k, S, count = (ls.WRITES[x] for x in ("n", "k", "S", "count"))
    assert S == 1 and count > ls.LAUNCH_WAVES + 1000, "one segment of one wave per stripe, one wave per write: both kernels take a second launch"
    x0 = ls.draw_tile(401, k, S)
    rng = np.random.default_rng(402)
    nw, wa, wb = (rng.integers(0, ls.P, size=T, dtype=np.uint64).astype(np.uint32) for _ in range(3))
    x1 = ls.burst1(x0, nw, k)
    x2 = ls.burst2(x1, wa, wb, k)

    def pools(x):
        d = ls.to_device(torch, ls.tile_to_stripes(x, S))
        p = ls.to_device(torch, ls.tile_to_stripes(ls.tile_parity(oracle, n, k, x), S))
        return ls.periodic_pool(torch, d, count), ls.periodic_pool(torch, p, count)

    D, Q = pools(x0)
    D0, Q0 = D.clone(), Q.clone()
    b = torch.arange(count, device="cuda:0")
    w1 = ls.burst1_writes(count, k)
    new1 = ls.to_device(torch, nw)[b % T].view(count, S).contiguous()
    new1_before, w1_before = new1.clone(), w1.copy()
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.update_batch(D, Q, count, w1, new1)
        torch.cuda.synchronize()
        want_d, want_p = pools(x1)
        assert torch.equal(D, want_d), "update_batch, one write per stripe: the data pool"
        assert torch.equal(Q, want_p), "update_batch, one write per stripe: the parity pool"
        assert torch.equal(new1, new1_before) and np.array_equal(w1, w1_before)

        w2, stripe2, which2 = ls.burst2_writes(count, k)
        assert len(w2) == 2 * -(-count // 3)
        at = torch.from_numpy((stripe2 % np.uint64(T)).astype(np.int64)).to("cuda:0")
        second = torch.from_numpy(which2.astype(np.bool_)).to("cuda:0")
        new2 = torch.where(second, ls.to_device(torch, wb)[at], ls.to_device(torch, wa)[at]).view(len(w2), S)
        enc.update_batch(D, Q, count, w2, new2)
        torch.cuda.synchronize()
        want_d, want_p = pools(x2)
        assert torch.equal(D, want_d), "update_batch, two writes in every third stripe: the data pool"
        assert torch.equal(Q, want_p), "update_batch, two writes in every third stripe: the parity pool"
        del D, Q, want_d

        old1 = D0.view(-1, S)[torch.from_numpy(w1.astype(np.int64)).to("cuda:0")].contiguous()
        old1_before = old1.clone()
        enc.update_parity_batch(Q0, count, w1, new1, old=old1)
        torch.cuda.synchronize()
        assert torch.equal(Q0, pools(x1)[1]), "update_parity_batch, one write per stripe"
        assert torch.equal(old1, old1_before) and torch.equal(new1, new1_before) and np.array_equal(w1, w1_before)


# ---- e: lane groups ----
def test_e_lane_groups(torch_cuda, fe, oracle):
    """(3,2) x 4 B, 2^30 + 4102 stripes: one lane group per stripe, so direct_batch_kernel takes a second launch of 4102 groups (a.group_base) —
    under encode_pool's VALU kernel, repair_batch (data block 1 lost) and decode_batch (data block 0 lost)"""
    torch = torch_cuda
    need_memory(torch)
    n, k, S, count = (ls.GROUPS[x] for x in ("n", "k", "S", "count"))
    assert ls.batch_groups(1, S, count) - ls.LAUNCH_GROUPS == T + 3, "4102 lane groups belong to the second launch"
    tile_d, tile_p = tiles(torch, oracle, n, k, S, 501)
    D = ls.periodic_pool(torch, tile_d, count)
    Q = torch.full((count + 1, n - k, S), LOST, dtype=torch.int32, device="cuda:0")
    Q[count:] = CANARY
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.set_option("encode_pool_kernel", 1)
        enc.profile(True)
        enc.encode_pool(D, Q, count)
        torch.cuda.synchronize()
        assert pool_scopes(enc) == {"encode_pool_valu": 1}
        enc.profile(False)
        assert ls.equal_periodic(torch, Q, tile_p, count), "encode_pool (VALU): the parity pool"
        assert ls.equal_periodic(torch, D, tile_d, count), "encode_pool wrote the data pool"
        for op, lost in (("repair", 1), ("decode", 0)):
            dp, pp = ls.flag_rows(k, n - k, [([lost], [])])
            enc.decode_prepare(dp[0], pp[0])
            D[:count, lost] = LOST
            getattr(enc, op + "_batch")(D, Q, count)
            torch.cuda.synchronize()
            assert ls.equal_periodic(torch, D, tile_d, count), "%s_batch: the data pool" % op
            assert ls.equal_periodic(torch, Q, tile_p, count), "%s_batch wrote the parity pool" % op


# ---- f: the matrix-core kernel's limit ----
def test_f_matrix_core_limit(torch_cuda, fe, oracle):
    """(3,2) x 256 B under encode_pool_kernel = 2: 2^24 stripes are the most the matrix-core kernel's one launch holds; one more stripe and the call
    takes the VALU kernel instead.  The same allocation, the expected parity both times"""
    torch = torch_cuda
    need_memory(torch)
    n, k, S, count = (ls.MFMA[x] for x in ("n", "k", "S", "count"))
    assert count * -(-S // 64) == ls.POOL_LAUNCH_WAVES
    tile_d, tile_p = tiles(torch, oracle, n, k, S, 601)
    D = ls.periodic_pool(torch, tile_d, count + 1)
    Q = torch.empty((count + 2, n - k, S), dtype=torch.int32, device="cuda:0")
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.set_option("encode_pool_kernel", 2)
        enc.profile(True)
        for stripes, scope in ((count, "encode_pool_mfma"), (count + 1, "encode_pool_valu")):
            Q[:] = CANARY
            enc.profile_reset()
            enc.encode_pool(D, Q, stripes)
            torch.cuda.synchronize()
            assert pool_scopes(enc) == {scope: 1}, "%d stripes" % stripes
            assert ls.equal_periodic(torch, Q, tile_p, stripes), "%s: the parity pool and everything after it" % scope
            assert ls.equal_periodic(torch, D, tile_d, count + 1), "encode_pool wrote the data pool"


# ---- g: the transform path ----
@pytest.mark.parametrize("call", ["encode_batch", "encode_pool"])
@pytest.mark.parametrize("shape", ls.TRANSFORM, ids=["4_2_register_pass", "128_64_mid_tile"])
def test_g_transform_path(torch_cuda, fe, oracle, shape, call):
    """(2k,k) codes whose one pass takes more than 2^24 waves over the batch: fastecc_encode_batch, and fastecc_encode_pool kept off the direct
    path, run it as several runs of stripes (encode_batch_passes: data + b0 * stride) — the pass's profile scope once per run and no other"""
    torch = torch_cuda
    n, k, S, count = (shape[x] for x in ("n", "k", "S", "count"))
    runs = -(-count // (ls.MAX_LAUNCH_WAVES // shape["stripe_waves"]))
    assert count * shape["stripe_waves"] > ls.MAX_LAUNCH_WAVES + 1000 and runs == (5 if k == 2 else 3), "more than one run of stripes"
    tile_d, tile_p = tiles(torch, oracle, n, k, S, 701 + k)
    D = ls.periodic_pool(torch, tile_d, count)
    want = ls.periodic_pool(torch, tile_p, count)
    Q = torch.full((count + 1, n - k, S), CANARY, dtype=torch.int32, device="cuda:0")
    with fe.Encoder(n, k, 4 * S) as enc:
        assert enc.plan() == shape["plan"]
        enc.set_option("encode_direct_max", 0)
        enc.profile(True)
        getattr(enc, call)(D, Q, count)
        torch.cuda.synchronize()
        launches = {name: v[1] for name, v in enc.profile_read().items()}
        passes = {name: v for name, v in launches.items() if name.startswith(("dif", "dit", "mid", "tile_"))}
        assert passes == {shape["scope"]: runs}, "the plan's one pass, one launch per run of stripes: %r" % launches
        assert not any(name.startswith(("encode_pool_", "direct")) for name in launches), "the direct path ran: %r" % launches
    assert torch.equal(Q, want), call + ": the parity pool"
    assert ls.equal_periodic(torch, D, tile_d, count), call + " wrote the data pool"


# ---- h: one stripe is one launch ----
def test_h_one_stripe_past_the_run_size_is_one_launch(torch_cuda, fe, oracle):
    """64 blocks of 64 MiB + 4 bytes (odd S: one word per lane): fastecc_scale_blocks and the bit reversal of fastecc_ntt are ONE launch of
    2^24 + 64 waves over the stripe — more than the 2^24 waves at which the batched calls split, far fewer than a dispatch holds.  A single stripe
    is neither cut nor refused (launch_limits.hpp: wave_launch_fits).  The oracle on sampled columns, the first and the last wave of a block
    among them; every word through the round trips scale / unscale and transform / inverse / divide by N"""
    torch = torch_cuda
    need_memory(torch, 16)
    N, S = 64, (1 << 24) + 1
    waves = ls.rows_waves(S, 1, N)
    assert waves - ls.MAX_LAUNCH_WAVES == 64 and ls.wave_launch_fits(waves)
    g = torch.Generator(device="cuda:0").manual_seed(801)
    x = torch.empty(N * S, dtype=torch.int32, device="cuda:0")
    for i in range(0, N * S, 1 << 28):
        x[i:i + (1 << 28)] = torch.randint(0, ls.P, (min(1 << 28, N * S - i),), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32)
    cols = [0, 1, 63, 64, S - 2, S - 1]

    def sample(t):
        return np.ascontiguousarray(t.view(N, S)[:, cols].cpu().numpy()).view(np.uint32)

    x_cols = sample(x)
    d = x.clone()
    scale, base = oracle.gf_inv(N), oracle.gf_root(2 * N)
    with fe.Encoder(2 * N, N, 4 * S) as enc:
        enc.scale_blocks(d, scale, base)
        torch.cuda.synchronize()
        assert np.array_equal(sample(d), oracle.scale_blocks(x_cols, scale, base)), "scale_blocks on the sampled columns"
        enc.scale_blocks(d, N, oracle.gf_inv(base))
        torch.cuda.synchronize()
        assert torch.equal(d, x), "scale_blocks and its inverse: the whole stripe"
        enc.ntt(d, False)
        torch.cuda.synchronize()
        assert np.array_equal(sample(d), oracle.ntt_fast(x_cols, False)), "ntt on the sampled columns"
        enc.ntt(d, True)
        enc.scale_blocks(d, oracle.gf_inv(N), 1)
        torch.cuda.synchronize()
        assert torch.equal(d, x), "ntt, its inverse and 1 / N: the whole stripe"
