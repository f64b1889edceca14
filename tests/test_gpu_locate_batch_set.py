"""GPU tests (-m gpu) of batched location and grouped repair with a pattern PER STRIPE: fastecc_locate_errors_batch_set and
the "correct_batch_mode" option of fastecc_correct_batch_set.

What a result is compared with: (a) the per-stripe loop on a clone — fastecc_scrub_erasures(the stripe's pattern) + fastecc_locate_errors /
fastecc_correct with the same seed; (b) the blocks the test itself corrupted, wherever 2t + b + w <= n - k and t <= "locate_max"; (c) for
corrected stripes the original codeword, absent blocks included.  Every comparison is bit-exact.  The shapes are the smallest at which the
kernels can go wrong: S = 16 / 33 / 64 (33: the fingerprint kernel without vector loads), chunks of 8 with 27 - 40 stripes (several chunks, a
ragged last one, several patterns inside a chunk), one pool whose base pointers are 4- but not 16-byte aligned."""
import ctypes

import numpy as np
import pytest

from test_gpu_scrub_set import P, SEED, Pool, _rng, flag_rows, one_word, pick_absent, presence, to_dev

pytestmark = pytest.mark.gpu

GROUPED_SCOPES = ("fingerprint_set_list", "scrub_syndromes_gather_set", "scrub_root_search_batch", "direct_pass_set")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def fe(hip_lib):
    import fastecc_amd
    return fastecc_amd


def locate_loop(fe, pool, patterns, po, seed, D=None, Q=None):
    """(a): fastecc_scrub_erasures(the stripe's pattern) + fastecc_locate_errors, stripe by stripe; a FASTECC_PATTERN_NONE stripe is status 0"""
    enc, status, lists = pool.enc, [], []
    for b, q in enumerate(po):
        found, st = [], 0
        if q != fe.PATTERN_NONE:
            enc.scrub_erasures(*presence(pool.n, pool.k, patterns[q]))
            try:
                found = enc.locate_errors(*pool.stripe(b, D, Q), seed=seed)
                st = 1 if found else 0
            except fe.FastEccError as e:
                assert e.code == fe.E_UNCORRECTABLE
                st = 2
        status.append(st)
        lists.append(found)
    enc.scrub_erasures()
    return status, lists


def correct_loop(fe, pool, patterns, po, seed, D, Q):
    """(a): fastecc_scrub_erasures(the stripe's pattern) + fastecc_correct on the stripes of the clone D, Q"""
    enc, status = pool.enc, []
    for b, q in enumerate(po):
        st = 0
        if q != fe.PATTERN_NONE:
            enc.scrub_erasures(*presence(pool.n, pool.k, patterns[q]))
            try:
                st = 1 if enc.correct(*pool.stripe(b, D, Q), seed=seed) else 0
            except fe.FastEccError as e:
                assert e.code == fe.E_UNCORRECTABLE
                st = 2
        status.append(st)
    enc.scrub_erasures()
    pool.torch.cuda.synchronize()
    return status


def locate_set(fe, enc, D, Q, count, po, seed, stream=0):
    """the Python method: (status list, lists), whether or not a stripe could not be located"""
    try:
        status, lists = enc.locate_errors_batch_set(D, Q, count, po, seed=seed, stream=stream)
    except fe.FastEccError as e:
        assert e.code == fe.E_UNCORRECTABLE
        status, lists = e.status, e.lists
        assert 2 in status.tolist()
    else:
        assert 2 not in status.tolist()
    return status.tolist(), lists


def raw_locate(fe, enc, D, Q, count, po, seed, cap):
    """the C entry point itself, every output preset to a sentinel: (code, status, blocks, counts, *inconsistent)"""
    status = np.full(count, 0xAB, np.uint8)
    blocks = np.full(count * min(max(cap, 1), 4), 0xB10C, np.uint64)  # (a cap beyond that is refused before anything is written)
    counts = np.full(count, 0xC0, np.uint32)
    bad = ctypes.c_uint64(0xDEAD)
    po = np.ascontiguousarray(po, dtype=np.uint32)
    code = fe.lib().fastecc_locate_errors_batch_set(enc._h, D.data_ptr(), Q.data_ptr(), count, po.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), None, seed,
                                                    status.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), blocks.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                                    cap, counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(bad))
    return code, status, blocks, counts, int(bad.value)


def raw_correct(fe, enc, D, Q, count, po, seed):
    out = np.full(count, 7, np.uint8)
    bad = ctypes.c_uint64(0xABCD)
    po = np.ascontiguousarray(po, dtype=np.uint32)
    code = fe.lib().fastecc_correct_batch_set(enc._h, D.data_ptr(), Q.data_ptr(), count, po.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), None, seed,
                                              out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(bad))
    return code, out.tolist(), int(bad.value)


def present_blocks(rng, n, absent, size=1):
    return sorted(int(j) for j in rng.choice([j for j in range(n) if j not in absent], size=size, replace=False))


def unchanged(pool, d, p):
    hd, hq = pool.contents()
    return np.array_equal(hd, d) and np.array_equal(hq, p)


@pytest.mark.parametrize("S,count,offset", [(16, 37, 0), (33, 27, 0), (64, 40, 0), (64, 29, 1)])
def test_rotated_pool_with_a_lying_device(torch_cuda, fe, S, count, offset):
    """(20,16) rotated, device 3 down and device 11 lying: one word of block (11 - b) mod n is wrong in every stripe, which never is the absent
    block (3 - b) mod n.  Every stripe has status 1 and the list [(11 - b) mod n]; the call reads only."""
    torch, rng = torch_cuda, _rng("lying", S, count, offset)
    n, k, down, lying = 20, 16, 3, 11
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.set_option("scrub_batch_chunk", 8)
        pool = Pool(torch, enc, count, S, rng, offset_words=offset)
        patterns = [[q] for q in range(n)]
        po = np.array([(down - b) % n for b in range(count)], dtype=np.uint32)
        enc.scrub_erasures_set(*flag_rows(n, k, patterns))
        d, p = pool.degraded(fe, patterns, po, rng)
        pool.upload(d, p)
        status, lists = locate_set(fe, enc, pool.D, pool.Q, count, po, SEED)
        assert status == [0] * count and lists == [[]] * count  # degraded and clean
        for b in range(count):
            one_word(pool.block(d, p, b, (lying - b) % n), rng)
        pool.upload(d, p)
        enc.profile(True)
        enc.profile_reset()
        code, status, blocks, counts, bad = raw_locate(fe, enc, pool.D, pool.Q, count, po, SEED, cap=2)
        prof = enc.profile_read()
        enc.profile(False)
        assert code == fe.OK and bad == count
        assert status.tolist() == [1] * count and counts.tolist() == [1] * count
        assert blocks.reshape(count, 2)[:, 0].tolist() == [(lying - b) % n for b in range(count)]
        assert set(blocks.reshape(count, 2)[:, 1].tolist()) == {0xB10C}  # entries beyond counts[b] are not written
        chunks = (count + 7) // 8
        for scope in GROUPED_SCOPES[:3]:
            assert prof[scope][1] == chunks, (scope, prof)
        assert prof["fingerprint_set_list"][2] == count * (n - 1) * S * 4  # its bytes: the blocks actually read
        assert unchanged(pool, d, p)
        assert locate_set(fe, enc, pool.D, pool.Q, count, po, SEED) == locate_loop(fe, pool, patterns, po, SEED)
        assert unchanged(pool, d, p)


def test_different_w_in_one_chunk(torch_cuda, fe):
    """(20,16): patterns with w = 0, 1, 3 and n - k = 4 absent blocks and FASTECC_PATTERN_NONE stripes in one chunk.  Errors within each pattern's
    own budget 2t + w <= 4 are listed exactly; three errors at w = 0, two at w = 1 and one at w = 3 are beyond it and answer as the loop does."""
    torch, rng = torch_cuda, _rng("w-locate")
    n, k, S = 20, 16, 16
    m, NONE = n - k, fe.PATTERN_NONE
    with fe.Encoder(n, k, 4 * S) as enc:
        patterns = [[], pick_absent(rng, n, k, 1), pick_absent(rng, n, k, 3), pick_absent(rng, n, k, m)]
        #              0  1  2  3  4     5  6  7  8  9     10 11 12 13 14 15
        po = np.array([0, 1, 2, 3, NONE, 0, 1, 2, 3, NONE, 0, 1, 3, 0, 2, 1], dtype=np.uint32)
        count = len(po)
        pool = Pool(torch, enc, count, S, rng)
        enc.scrub_erasures_set(*flag_rows(n, k, patterns))
        d, p = pool.degraded(fe, patterns, po, rng)
        for b in (3, 12):  # w = n - k: garbage below p in the absent blocks
            for j in patterns[3]:
                pool.block(d, p, b, j)[:] %= np.uint32(P)
        errors = {0: 1, 5: 2, 10: 3, 1: 1, 6: 2, 7: 1, 13: 1}  # stripe -> wrong blocks
        wrong = {b: present_blocks(rng, n, patterns[po[b]], t) for b, t in errors.items()}
        for b, js in wrong.items():
            for j in js:
                one_word(pool.block(d, p, b, j), rng)
        pool.block(d, p, 8, present_blocks(rng, n, patterns[3])[0])[5] = np.uint32(P + 1)  # w = n - k and a word >= p in a present block
        pool.upload(d, p)
        want_status, want_lists = locate_loop(fe, pool, patterns, po, SEED)
        for b, js in wrong.items():  # (b): what the test corrupted, within the pattern's budget
            if 2 * len(js) + len(patterns[po[b]]) <= m:
                assert want_status[b] == 1 and want_lists[b] == js, b
            else:
                assert want_status[b] != 0, b
        assert want_status[10] == 2  # three errors at w = 0: no codeword within two blocks of it
        assert [want_status[b] for b in (3, 12, 4, 9, 2, 14, 11, 15)] == [0] * 8
        assert want_status[8] == 2  # n - k + 1 known erasures
        wants = {SEED: (want_status, want_lists), SEED + 1: locate_loop(fe, pool, patterns, po, SEED + 1)}
        for chunk in (0, 8):
            enc.set_option("scrub_batch_chunk", chunk)
            for seed in (SEED, SEED + 1):
                assert locate_set(fe, enc, pool.D, pool.Q, count, po, seed) == wants[seed], (chunk, seed)
        code, status, blocks, counts, bad = raw_locate(fe, enc, pool.D, pool.Q, count, po, SEED, cap=0)
        assert code == fe.E_UNCORRECTABLE and status.tolist() == want_status and bad == sum(1 for s in want_status if s)
        assert counts.tolist() == [len(x) for x in want_lists] and set(blocks.tolist()) == {0xB10C}  # cap = 0: the full counts, no block written
        assert unchanged(pool, d, p)


FAMILIES = [(8, 4, 32), (72, 64, 33), (64, 16, 16), (64, 8, 32), (130, 100, 16), (1100, 1000, 8)]


@pytest.mark.parametrize("n,k,S", FAMILIES)
def test_code_families(torch_cuda, fe, n, k, S):
    """(2k,k), an odd block length, fixed erasures, n = 4k / 8k, zero-extended codes: the per-stripe loop's answer and the corrupted blocks."""
    torch, m = torch_cuda, n - k
    rng = _rng("families-locate", n, k, S)
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.set_option("scrub_batch_chunk", 4)
        patterns = [pick_absent(rng, n, k, 1), pick_absent(rng, n, k, 2), [], pick_absent(rng, n, k, min(3, m - 2))]
        po = np.array([0, 1, 2, 3, 1, 0, 3], dtype=np.uint32)
        count = len(po)
        pool = Pool(torch, enc, count, S, rng)
        enc.scrub_erasures_set(*flag_rows(n, k, patterns))
        d, p = pool.degraded(fe, patterns, po, rng)
        wrong = {b: present_blocks(rng, n, patterns[po[b]], t) for b, t in ((1, 1), (2, 2 if m >= 4 else 1), (4, 1), (6, 1 if m - len(patterns[3]) >= 2 else 0))}
        for b, js in wrong.items():
            for j in js:
                one_word(pool.block(d, p, b, j), rng)
        pool.upload(d, p)
        status, lists = locate_set(fe, enc, pool.D, pool.Q, count, po, SEED)
        assert (status, lists) == locate_loop(fe, pool, patterns, po, SEED)
        for b in range(count):
            js = wrong.get(b, [])
            assert 2 * len(js) + len(patterns[po[b]]) <= m
            assert lists[b] == js and status[b] == (1 if js else 0), b
        assert unchanged(pool, d, p)


def test_more_syndromes_than_the_batched_pass_gathers(torch_cuda, fe):
    """(1200,600) at S = 8: a pattern with w = 0 (600 syndromes: the single-stripe code) and one with w = 100 (500: batched) in one call."""
    torch, rng = torch_cuda, _rng("1200")
    n, k, S = 1200, 600, 8
    with fe.Encoder(n, k, 4 * S) as enc:
        patterns = [[], pick_absent(rng, n, k, 100)]
        po = np.array([0, 1, 1, 0, 1], dtype=np.uint32)
        count = len(po)
        pool = Pool(torch, enc, count, S, rng)
        enc.scrub_erasures_set(*flag_rows(n, k, patterns))
        d, p = pool.degraded(fe, patterns, po, rng)
        wrong = {0: present_blocks(rng, n, patterns[0], 2), 1: present_blocks(rng, n, patterns[1], 3), 4: present_blocks(rng, n, patterns[1], 1)}
        for b, js in wrong.items():
            for j in js:
                one_word(pool.block(d, p, b, j), rng)
        pool.upload(d, p)
        enc.profile(True)
        enc.profile_reset()
        status, lists = locate_set(fe, enc, pool.D, pool.Q, count, po, SEED)
        prof = enc.profile_read()
        enc.profile(False)
        assert status == [1, 1, 0, 0, 1] and lists == [wrong.get(b, []) for b in range(count)]
        assert prof["fingerprint_set_list"][1] == 1 and prof["fingerprint_set_list"][2] == 2 * (n - 100) * S * 4  # stripes 1 and 4 only
        assert prof["scrub_root_search"][1] == 1  # stripe 0 through the single-stripe code
        assert (status, lists) == locate_loop(fe, pool, patterns, po, SEED)
        assert unchanged(pool, d, p)


def test_correct_batch_set_modes(torch_cuda, fe):
    """(64,16), 33 stripes in chunks of 8: modes 0, 1 and 2 on clones of one corrupted pool give the loop's status, count, return code and bytes;
    the profile scopes prove which path ran; the other states of the context are as before the call."""
    torch, rng = torch_cuda, _rng("modes")
    n, k, S, count = 64, 16, 16, 33
    m, NONE = n - k, fe.PATTERN_NONE
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.set_option("scrub_batch_chunk", 8)
        enc.set_option("locate_max", 2)
        pool = Pool(torch, enc, count, S, rng)
        wide = pick_absent(rng, n, k, 17)
        patterns = [[q] for q in range(8)] + [[], pick_absent(rng, n, k, 3), wide]
        po = np.array([b % 8 for b in range(count)], dtype=np.uint32)
        po[[2, 19]] = 8
        po[[5, 22, 30]] = 9
        po[[12, 27]] = 10
        po[[7, 16]] = NONE
        dp, pp = flag_rows(n, k, patterns)
        enc.decode_prepare_set(*flag_rows(n, k, [a if len(a) <= 16 else [] for a in patterns]))  # before the call: it must compute the same afterwards
        enc.scrub_erasures_set(dp, pp)
        single = [1, k + 2]  # the single scrub pattern: untouched by the set calls
        enc.scrub_erasures(*presence(n, k, single))
        d, p = pool.degraded(fe, patterns, po, rng)
        absent = lambda b: [] if po[b] == NONE else patterns[po[b]]
        fixable = {1: 1, 2: 2, 5: 1, 9: 2, 19: 1, 22: 2, 24: 1, 32: 1, 12: 1}  # stripe -> wrong blocks; stripe 12: w = 17, a lost set of 18 blocks
        wrong = {b: present_blocks(rng, n, absent(b), t) for b, t in fixable.items()}
        big_stripe, hopeless = 14, 26
        wrong[hopeless] = present_blocks(rng, n, absent(hopeless), 3)  # t = 3 > locate_max = 2, and 3 + 2 < n - k - w + 1: no codeword within reach
        for b, js in wrong.items():
            for j in js:
                one_word(pool.block(d, p, b, j), rng)
        pool.block(d, p, big_stripe, present_blocks(rng, n, absent(big_stripe))[0])[3] = np.uint32(P + 7)
        pool.upload(d, p)
        want = [0] * count
        for b in list(fixable) + [big_stripe]:
            want[b] = 1
        want[hopeless] = 2
        before_set = enc.verify_batch_set(pool.D, pool.Q, count, po, seed=SEED + 3).tolist()
        before_single = [enc.verify(*pool.stripe(b), seed=SEED + 3) for b in (0, 3)]
        assert before_set == [w == 0 for w in want]
        # (a) the per-stripe loop on a clone
        DL, QL = pool.D.clone(), pool.Q.clone()
        assert correct_loop(fe, pool, patterns, po, SEED, DL, QL) == want
        enc.scrub_erasures(*presence(n, k, single))
        # the launches mode 1 makes: every flagged stripe is listed (m - w is in [1, 512] for every pattern); the private set takes the lost sets of at
        # most 16 blocks, one launch per size class (the class of a pass: its outputs rounded up to a power of two)
        flagged = sorted(list(fixable) + [big_stripe, hopeless])
        list_chunks = [flagged[i:i + 8] for i in range(0, len(flagged), 8)]
        searched = sum(1 for c in list_chunks if any(b != big_stripe for b in c))
        classes = {1 << (len(wrong[b]) + len(absent(b)) - 1).bit_length() for b in fixable if len(wrong[b]) + len(absent(b)) <= 16}
        # the lost sets of more than 16 blocks go set by set: one prepare and one list-form repair each, whose passes are the single pattern's (DESIGN.md
        # section 13: data AND parity lost, more than 32 blocks in all, is the data pass and then the parity pass; anything else is one pass).  A pass
        # over so few stripes has far fewer than 1024 waves, so the default rule runs it stripe by stripe under "direct_pass", the scope that
        # fastecc_repair of the modes' single-stripe corrections records too: the batched form is asked for, which records "direct_pass_list".
        lost_sets = {tuple(sorted(wrong[b] + absent(b))) for b in fixable}
        wide_passes = sum(2 if len(ls) > 32 and min(ls) < k <= max(ls) else 1 for ls in lost_sets if len(ls) > 16)
        assert wide_passes == 1  # stripe 12 alone: 18 blocks
        enc.set_option("decode_batch_kernel", 1)
        results = {}
        enc.profile(True)
        for mode in (0, 1, 2):
            D, Q = pool.D.clone(), pool.Q.clone()
            enc.set_option("correct_batch_mode", mode)
            enc.profile_reset()
            results[mode] = raw_correct(fe, enc, D, Q, count, po, SEED)
            torch.cuda.synchronize()
            prof = enc.profile_read(cap=128)
            assert results[mode] == (fe.E_UNCORRECTABLE, want, len(flagged)), mode
            assert torch.equal(D, DL) and torch.equal(Q, QL), mode  # the loop's bytes
            if mode == 2:
                assert not [x for x in GROUPED_SCOPES if x in prof], prof
                assert "direct_pass_list" not in prof, prof
            else:
                assert prof["direct_pass_list"][1] == wide_passes, prof
                assert prof["fingerprint_set_list"][1] == len(list_chunks) and prof["scrub_syndromes_gather_set"][1] == len(list_chunks), prof
                assert prof["scrub_root_search_batch"][1] == searched, prof
                assert prof["direct_pass_set"][1] == len(classes), (prof, classes)
        enc.profile(False)
        enc.set_option("decode_batch_kernel", 0)
        # (c) corrected stripes hold the original codeword, absent blocks included; the others are untouched
        hd, hq = pool.contents(D, Q)
        for b in range(count):
            if want[b] == 1:
                assert np.array_equal(hd[b], pool.d[b]) and np.array_equal(hq[b], pool.p[b]), b
            else:
                assert np.array_equal(hd[b], d[b]) and np.array_equal(hq[b], p[b]), b
        # the context's other states answer as before the call: the scrub set, the single scrub pattern, the decode pattern set
        pool.D.copy_(D)
        pool.Q.copy_(Q)
        after = enc.verify_batch_set(pool.D, pool.Q, count, po, seed=SEED + 3).tolist()
        assert after == [w != 2 for w in want]
        pool.upload(d, p)
        assert enc.verify_batch_set(pool.D, pool.Q, count, po, seed=SEED + 3).tolist() == before_set
        assert [enc.verify(*pool.stripe(b), seed=SEED + 3) for b in (0, 3)] == before_single
        pool.D.copy_(D)
        pool.Q.copy_(Q)
        narrow = np.where(po == 10, NONE, po).astype(np.uint32)
        enc.repair_batch_set(pool.D, pool.Q, count, narrow)
        torch.cuda.synchronize()
        hd, hq = pool.contents()
        keep = [b for b in range(count) if b != hopeless and po[b] not in (10, NONE)]
        assert np.array_equal(hd[keep], pool.d[keep]) and np.array_equal(hq[keep], pool.p[keep])


def test_stale_state(torch_cuda, fe):
    """One context through verify_batch, a located call under set A, a disjoint set B, the set cleared and made again.  The absent blocks hold
    garbage below p, so only the syndromes can tell; no answer may depend on what an earlier call or set left in the fingerprint stripes."""
    torch, rng = torch_cuda, _rng("stale-locate")
    n, k, S, count = 32, 16, 64, 11
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.set_option("scrub_batch_chunk", 8)
        pool = Pool(torch, enc, count, S, rng)
        blocks = [int(x) for x in rng.permutation(n)]
        A = [sorted(blocks[0:2]), sorted(blocks[2:4]), sorted(blocks[4:6])]
        B = [sorted(blocks[6:8]), sorted(blocks[8:10]), sorted(blocks[10:13])]
        po = np.arange(count, dtype=np.uint32) % 3

        def corrupted(patterns, stripes):
            d, p = pool.degraded(fe, patterns, po, rng)
            d[:] %= np.uint32(P)
            p[:] %= np.uint32(P)
            wrong = {b: present_blocks(rng, n, patterns[po[b]], t) for b, t in stripes.items()}
            for b, js in wrong.items():
                for j in js:
                    one_word(pool.block(d, p, b, j), rng)
            return d, p, [wrong.get(b, []) for b in range(count)]

        def located(d, p):
            pool.upload(d, p)
            return locate_set(fe, enc, pool.D, pool.Q, count, po, SEED)[1]
        d, p = pool.d.copy(), pool.p.copy()
        one_word(pool.block(d, p, 5, 2), rng)
        pool.upload(d, p)
        assert enc.verify_batch(pool.D, pool.Q, count, seed=SEED).tolist() == [b != 5 for b in range(count)]
        in_a = corrupted(A, {0: 1, 4: 3, 9: 2, 10: 1})
        in_b = corrupted(B, {1: 2, 4: 1, 8: 6, 10: 2})
        enc.scrub_erasures_set(*flag_rows(n, k, A))
        assert located(*in_a[:2]) == in_a[2]
        assert located(*in_a[:2]) == in_a[2]
        enc.scrub_erasures_set(*flag_rows(n, k, B))
        assert located(*in_b[:2]) == in_b[2]
        status, _ = locate_set(fe, enc, *[to_dev(torch, x.reshape(-1)) for x in in_a[:2]], count, po, SEED)
        assert 0 not in status  # set A's garbage is read under set B: every stripe is bad
        assert located(*in_b[:2]) == in_b[2]
        enc.scrub_erasures_set([], [])
        with pytest.raises(fe.FastEccError) as ei:
            enc.locate_errors_batch_set(pool.D, pool.Q, count, po, seed=SEED)
        assert ei.value.code == fe.E_INVAL
        enc.scrub_erasures_set(*flag_rows(n, k, A))
        assert located(*in_a[:2]) == in_a[2]


def test_pattern_of_is_free_on_return(torch_cuda, fe):
    """pattern_of is the caller's again when a call returns: the test overwrites it at once, and the next call gets another array."""
    torch, rng = torch_cuda, _rng("reuse")
    n, k, S, count = 20, 16, 16, 21
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.set_option("scrub_batch_chunk", 8)
        pool = Pool(torch, enc, count, S, rng)
        patterns = [[q] for q in range(n)]
        po = (np.arange(count, dtype=np.uint32) + 5) % n
        enc.scrub_erasures_set(*flag_rows(n, k, patterns))
        d, p = pool.degraded(fe, patterns, po, rng)
        wrong = {b: present_blocks(rng, n, patterns[po[b]]) for b in (0, 7, 8, 20)}
        for b, js in wrong.items():
            one_word(pool.block(d, p, b, js[0]), rng)
        pool.upload(d, p)
        want = [wrong.get(b, []) for b in range(count)]
        arr = po.copy()
        for _ in range(2):
            assert enc.locate_errors_batch_set(pool.D, pool.Q, count, arr, seed=SEED)[1] == want
            arr[:] = (arr + 1) % n  # the wrong patterns: nothing may still read them
            arr = po.copy()
        arr = po.copy()
        enc.set_option("correct_batch_mode", 1)
        assert enc.correct_batch_set(pool.D, pool.Q, count, arr, seed=SEED).tolist() == [int(b in wrong) for b in range(count)]
        arr[:] = fe.PATTERN_NONE - 1
        assert enc.locate_errors_batch_set(pool.D, pool.Q, count, po.copy(), seed=SEED)[1] == [[]] * count


def test_two_streams_one_context(torch_cuda, fe):
    torch, rng = torch_cuda, _rng("streams")
    n, k, S, count = 20, 16, 64, 19
    with fe.Encoder(n, k, 4 * S) as enc:
        enc.set_option("scrub_batch_chunk", 8)
        pool = Pool(torch, enc, count, S, rng)
        patterns = [[q] for q in range(n)]
        po = np.arange(count, dtype=np.uint32) % n
        enc.scrub_erasures_set(*flag_rows(n, k, patterns))
        d, p = pool.degraded(fe, patterns, po, rng)
        wrong = {b: present_blocks(rng, n, patterns[po[b]], t) for b, t in ((2, 1), (9, 1), (10, 2), (18, 1))}
        wrong[10] = wrong[10][:1]  # (one error is all (20,16) with one absent block can locate)
        for b, js in wrong.items():
            one_word(pool.block(d, p, b, js[0]), rng)
        pool.upload(d, p)
        want = ([int(b in wrong) for b in range(count)], [wrong.get(b, []) for b in range(count)])
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        for _ in range(2):
            for s in (s1, s2):
                assert locate_set(fe, enc, pool.D, pool.Q, count, po, SEED, stream=s.cuda_stream) == want
        enc.set_option("correct_batch_mode", 1)
        D2, Q2 = pool.D.clone(), pool.Q.clone()
        torch.cuda.synchronize()
        assert enc.correct_batch_set(pool.D, pool.Q, count, po, seed=SEED, stream=s1.cuda_stream).tolist() == want[0]
        assert enc.correct_batch_set(D2, Q2, count, po, seed=SEED, stream=s2.cuda_stream).tolist() == want[0]
        torch.cuda.synchronize()
        assert torch.equal(pool.D, D2) and torch.equal(pool.Q, Q2)
        hd, hq = pool.contents()
        fixed = sorted(wrong)
        assert np.array_equal(hd[fixed], pool.d[fixed]) and np.array_equal(hq[fixed], pool.p[fixed])


def test_refusals(torch_cuda, fe):
    torch, rng = torch_cuda, _rng("refused-locate")
    n, k, S, count = 8, 4, 32, 5
    with fe.Encoder(n, k, 4 * S) as enc:
        pool = Pool(torch, enc, count, S, rng)
        patterns = [[0], [5], [2, 7]]

        def refused(po, cap=2):
            code, status, blocks, counts, bad = raw_locate(fe, enc, pool.D, pool.Q, count, po, SEED, cap)
            assert set(status.tolist()) == {0xAB} and set(blocks.tolist()) == {0xB10C} and set(counts.tolist()) == {0xC0} and bad == 0xDEAD
            return code
        assert refused([0, 1, 2, 0, 1]) == fe.E_INVAL  # no set prepared
        enc.scrub_erasures_set(*flag_rows(n, k, patterns))
        assert refused([0, 1, 3, 0, 1]) == fe.E_INVAL  # an entry >= P that is not FASTECC_PATTERN_NONE
        assert refused([0, 1, 2, 0, fe.PATTERN_NONE - 1]) == fe.E_INVAL
        assert refused([0, 1, 2, 0, 1], cap=1 << 62) == fe.E_INVAL  # count * cap * 8 beyond 64 bits
    for make in (lambda: fe.Encoder(64, 32, 64, field=fe.FIELD_GF_P61_SQUARED), lambda: fe.ShardedEncoder(64, 32, 256, [0, 0]),
                 lambda: fe.Encoder(2 * 48, 48, 64, flags=fe.CODE_MIXED_RADIX)):
        with make() as enc:
            buf = torch.zeros(2 * enc.n * enc.block_bytes // 4, dtype=torch.int32, device="cuda:0")
            with pytest.raises(fe.FastEccError) as ei:
                enc.locate_errors_batch_set(buf, buf, 2, np.zeros(2, np.uint32))
            assert ei.value.code == fe.E_UNSUPPORTED
