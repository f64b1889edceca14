"""GPU test (-m gpu): the device state behind a context gives back what it took.

Eight identical cycles create contexts, drive every family of state through them (direct and transform decode, host staging and the packed
copy-back, pattern sets and their swap, small writes and their batch form, the scrub family with named erasures and pattern sets, the 64-bit
field's decoder) and close them.  Every result of a cycle equals the first cycle's bit for bit (and the first cycle's equal the stripes the
damage was done to), and the device's free memory after cycle 8 is not below that after cycle 2 (cycle 1 pays for the runtime's one-time
allocations).  A context held open across the cycles is the control: the free-memory reading must see it come and go, or the test is blind."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 0xFFF00001
P61 = (1 << 61) - 1
CYCLES = 8
# Largest drop of free memory from cycle 2 to cycle 8 that the reading itself shows on code that frees everything: measured three times on the
# tree before the owning types, 0 bytes each time.
SLACK = 0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def fe(hip_lib):
    import fastecc_amd
    return fastecc_amd


def dev32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).reshape(-1)).to("cuda:0")


def dev64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).reshape(-1)).to("cuda:0")


def host32(t):
    return t.cpu().numpy().view(np.uint32).copy()


def host64(t):
    return t.cpu().numpy().view(np.uint64).copy()


def flags(count, lost):
    f = np.ones(count, np.uint8)
    f[list(lost)] = 0
    return f


class Stripe:
    """A codeword (data, parity) on the device, a damaged copy of it per erasure pattern, and work buffers the calls write to: all allocated
    once, before the measurement starts."""

    def __init__(self, torch, to_dev, data, parity, patterns):
        self.data, self.parity = data, parity  # host, as encoded
        self.clean = (to_dev(torch, data), to_dev(torch, parity))
        self.work = (torch.empty_like(self.clean[0]), torch.empty_like(self.clean[1]))
        self.present, self.damaged, self.damaged_host = [], [], []
        for lost_d, lost_p in patterns:
            bad_d, bad_p = data.copy(), parity.copy()
            bad_d[list(lost_d)] = 11
            bad_p[list(lost_p)] = 13
            self.present.append((flags(len(data), lost_d), flags(len(parity), lost_p)))
            self.damaged.append((to_dev(torch, bad_d), to_dev(torch, bad_p)))
            self.damaged_host.append((bad_d, bad_p))

    def damage(self, i):
        self.work[0].copy_(self.damaged[i][0])
        self.work[1].copy_(self.damaged[i][1])
        return self.work


def encoded(torch, fe, n, k, block_bytes, data, field=None, stripes=1):
    """parity of `stripes` stripes back to back by fastecc_encode, on a context of its own (closed before the measurement)"""
    p61 = field is not None
    to_dev, to_host = (dev64, host64) if p61 else (dev32, host32)
    per = (n - k) * block_bytes // (8 if p61 else 4)
    out = []
    with fe.Encoder(n, k, block_bytes, **({"field": field} if p61 else {})) as enc:
        for b in range(stripes):
            par = torch.zeros(per, dtype=torch.int64 if p61 else torch.int32, device="cuda:0")
            enc.encode(to_dev(torch, data[b] if stripes > 1 else data), par)
            torch.cuda.synchronize()
            out.append(to_host(par))
    return np.stack(out) if stripes > 1 else out[0]


def test_contexts_give_back_their_device_memory(torch_cuda, fe):
    torch = torch_cuda
    rng = np.random.default_rng(2024)
    free = lambda: torch.cuda.mem_get_info()[0]

    # ---- everything the cycles touch, allocated up front ----
    K, S = 1 << 10, 64  # (2k,k), 256-byte blocks
    data = rng.integers(0, P, size=(K, S), dtype=np.uint64).astype(np.uint32)
    parity = encoded(torch, fe, 2 * K, K, 4 * S, data).reshape(K, S)
    few = ([5, 700], [9])
    many = (sorted(rng.permutation(K)[: K // 8].tolist()), sorted(rng.permutation(K)[: K // 8].tolist()))  # k/4 blocks in all
    big = Stripe(torch, dev32, data, parity, [few, many])
    new3 = dev32(torch, rng.integers(0, P, size=(3, S), dtype=np.uint64))
    junk = dev32(torch, rng.integers(0, P, size=S, dtype=np.uint64))
    absent = (flags(K, [3]), flags(K, [4]))

    PN, PK, PS, B = 20, 16, 4, 8  # the pool: (20,16), 16-byte blocks, 8 stripes
    PM = PN - PK
    pool_data = rng.integers(0, P, size=(B, PK, PS), dtype=np.uint64).astype(np.uint32)
    pool_parity = encoded(torch, fe, PN, PK, 4 * PS, pool_data, stripes=B).reshape(B, PM, PS)
    set4 = [([q, q + 5], [q % PM]) for q in range(4)]
    pattern_of = [b % 4 for b in range(B)]
    bad_d, bad_p = pool_data.copy(), pool_parity.copy()
    for b in range(B):
        bad_d[b, set4[pattern_of[b]][0]] = 11
        bad_p[b, set4[pattern_of[b]][1]] = 13
    pool_clean = (dev32(torch, pool_data), dev32(torch, pool_parity))
    pool_bad = (dev32(torch, bad_d), dev32(torch, bad_p))
    pool_work = (torch.empty_like(pool_clean[0]), torch.empty_like(pool_clean[1]))
    set_flags = lambda pats: (np.stack([flags(PK, d) for d, _ in pats]), np.stack([flags(PM, p) for _, p in pats]))
    writes_short = [0 * PK + 3, 2 * PK + 0, 2 * PK + 15, 5 * PK + 7, 7 * PK + 9]
    writes_long = [int(x) for x in rng.permutation(B * PK)]  # every block of the pool: the longest list it allows
    new_short = dev32(torch, rng.integers(0, P, size=(len(writes_short), PS), dtype=np.uint64))
    new_long = dev32(torch, rng.integers(0, P, size=(len(writes_long), PS), dtype=np.uint64))
    pool_junk = dev32(torch, rng.integers(0, P, size=PS, dtype=np.uint64))

    K61, E61 = 1 << 8, 16  # GF((2^61-1)^2), (2k,k), 256-byte blocks
    data61 = rng.integers(0, P61, size=(K61, 2 * E61), dtype=np.uint64)
    parity61 = encoded(torch, fe, 2 * K61, K61, 16 * E61, data61, field=fe.FIELD_GF_P61_SQUARED).reshape(K61, 2 * E61)
    many61 = (sorted(rng.permutation(K61)[: K61 // 8].tolist()), sorted(rng.permutation(K61)[: K61 // 8].tolist()))
    wide = Stripe(torch, dev64, data61, parity61, [([1, 200], [7]), many61])
    torch.cuda.synchronize()

    def cycle():
        out = []
        with fe.Encoder(2 * K, K, 4 * S) as enc:
            enc.decode_prepare(*big.present[0])  # 3 lost blocks: the direct path
            d, q = big.damage(0)
            enc.repair(d, q)
            out += [host32(d), host32(q)]
            enc.set_option("decode_direct_max", 0)  # k/4 lost blocks through the transform: locator tree, re-encode
            enc.decode_prepare(*big.present[1])
            d, q = big.damage(1)
            enc.repair(d, q)
            out += [host32(d), host32(q)]
            hd, hq = big.damaged_host[1][0].copy(), big.damaged_host[1][1].copy()  # host memory: staging, packed copy-back
            enc.repair(hd, hq, mem=fe.MEM_HOST)
            out += [hd, hq]
            enc.update(d, q, [1, 17, 1000], new3)
            out += [host32(d), host32(q)]
            enc.scrub_erasures(*absent)
            out.append(np.array([enc.verify(d, q, seed=5)]))
            d[77 * S:78 * S].copy_(junk)
            out.append(np.array(enc.correct(d, q, seed=5), dtype=np.uint64))
            out += [host32(d), host32(q)]
        with fe.Encoder(PN, PK, 4 * PS) as enc:
            enc.decode_prepare_set(*set_flags(set4))
            pool_work[0].copy_(pool_bad[0])
            pool_work[1].copy_(pool_bad[1])
            enc.repair_batch_set(pool_work[0], pool_work[1], B, pattern_of)
            out += [host32(pool_work[0]), host32(pool_work[1])]
            enc.decode_prepare_set(*set_flags(set4[:2]))  # the swap
            enc.update_batch(pool_work[0], pool_work[1], B, writes_short, new_short)
            enc.update_batch(pool_work[0], pool_work[1], B, writes_long, new_long)
            out += [host32(pool_work[0]), host32(pool_work[1])]
            enc.scrub_erasures(flags(PK, [2]), None)
            out.append(enc.verify_batch(pool_work[0], pool_work[1], B, seed=9))
            pool_work[0][(3 * PK + 6) * PS:(3 * PK + 7) * PS].copy_(pool_junk)
            out.append(enc.correct_batch(pool_work[0], pool_work[1], B, seed=9))
            out += [host32(pool_work[0]), host32(pool_work[1])]
            enc.scrub_erasures_set(*set_flags(set4))
            out.append(enc.verify_batch_set(pool_work[0], pool_work[1], B, pattern_of, seed=9))
            enc.scrub_erasures_set([], [])
        with fe.Encoder(2 * K61, K61, 16 * E61, field=fe.FIELD_GF_P61_SQUARED) as enc:
            for i in (0, 1):  # few losses (direct), k/4 losses (transform)
                enc.decode_prepare(*wide.present[i])
                d, q = wide.damage(i)
                enc.repair(d, q)
                out += [host64(d), host64(q)]
        torch.cuda.synchronize()
        return out

    # ---- the control: a context that is held must show in the reading ----
    CK, CBYTES = 1 << 10, 4096
    before = free()
    control = fe.Encoder(2 * CK, CK, CBYTES)
    control.set_option("decode_direct_max", 0)
    control.decode_prepare(flags(CK, range(0, CK, 4)), np.ones(CK, np.uint8))
    torch.cuda.synchronize()
    held = free()
    largest = CK * CBYTES  # the k-block stripe the transform leaves x p'(x) in
    assert before - held >= largest, (before, held, largest)

    first, readings = None, []
    for c in range(CYCLES):
        out = cycle()
        readings.append(free())
        print("free memory after cycle %d: %d" % (c + 1, readings[-1]))
        if first is None:
            first = out
            want = [big.data, big.parity, big.data, big.parity, big.data, big.parity]
            for i, w in enumerate(want):
                assert np.array_equal(out[i].reshape(w.shape), w), "cycle 1, result %d differs from the stripe as encoded" % i
            assert out[8][0] and list(out[9]) == [77], (out[8], out[9])
            assert np.array_equal(out[12].reshape(pool_data.shape), pool_data) and np.array_equal(out[13].reshape(pool_parity.shape), pool_parity)
            assert out[16].all() and list(out[17]) == [0, 0, 0, 1, 0, 0, 0, 0] and out[20].all(), (out[16], out[17], out[20])
            for i, w in zip(range(21, 25), [wide.data, wide.parity, wide.data, wide.parity]):
                assert np.array_equal(out[i].reshape(w.shape), w), "cycle 1, result %d differs from the stripe as encoded" % i
        else:
            assert len(out) == len(first)
            for i, (a, b) in enumerate(zip(out, first)):
                assert np.array_equal(a, b), "cycle %d, result %d differs from cycle 1" % (c + 1, i)
    print("drop from cycle 2 to cycle 8:", readings[1] - readings[-1])
    assert readings[1] - readings[-1] <= SLACK, readings

    with_control = free()
    control.close()
    torch.cuda.synchronize()
    assert free() - with_control >= largest, (with_control, free(), largest)


# The same reading for the second test, on the commit before the context's own members became owners: three runs of its cycles, drop from cycle 2
# to cycle 8 of 0, 0 and 0 bytes; the largest is the slack.
CTX_SLACK = 0


def test_context_members_give_back_their_device_memory(torch_cuda, fe, oracle):
    """The same construction for what the context itself and the 64-bit field's path own: work stripes (scratch, parbuf, mixbuf, hostpar, dbuf,
    rawbuf), the twiddle and mixed-radix tables, the slab streams with their events, both staging rings, the profiler's event pairs, the 64-bit
    field's tables.  Eight identical cycles; every result equals cycle 1's bit for bit, cycle 1's equal the oracle's; free memory after cycle 8
    against cycle 2; a held (3k/2,k) context with 4 KiB blocks, whose 4 MiB scratch stripe only the context's members own, is the control.

    Three choices the codes force: (130,100) and the mixed-radix code have few enough parity blocks for the direct encoder, which needs neither
    parbuf nor mixbuf, so both contexts turn it off; no plan at k = 2^10 is all tiles with more than one pass, which is what the option `slabs`
    needs to put its slabs on the internal streams, so a context at k = 2^12 with plan 1060 carries it as well; and a 32 MiB stripe in host
    memory comes down through the download ring only (the pipelined form starts at 256 MiB), so the same context also encodes a table of
    separate blocks, which goes up through the other ring."""
    from oracle import OracleP61
    from pool_model import MIXED_RADIX, Codec
    torch = torch_cuda
    rng = np.random.default_rng(2025)
    free = lambda: torch.cuda.mem_get_info()[0]
    below_p = lambda *shape: rng.integers(0, P, size=shape, dtype=np.uint64).astype(np.uint32)
    empty32 = lambda words: torch.empty(words, dtype=torch.int32, device="cuda:0")

    def padded(x, pitch):
        out = np.zeros((x.shape[0], pitch), dtype=np.uint32)
        out[:, :x.shape[1]] = x
        return out

    # ---- everything the cycles touch, allocated up front; what the oracle says, computed once ----
    K = 1 << 10
    SA, PA = 64, 96  # (3k/2,k), 256-byte blocks; the pitch of its second encode
    xa = below_p(K, SA)
    want_a = oracle.encode_fast(xa)[::2]
    da, da_pitched = dev32(torch, xa), dev32(torch, padded(xa, PA))
    out_a, out_a_pitched = empty32(K // 2 * SA), empty32(K // 2 * PA)

    xb = below_p(100, 8)  # (130,100), 32-byte blocks
    want_b = Codec(oracle, 130, 100).parity(xb)
    db, out_b = dev32(torch, xb), empty32(30 * 8)

    xc = below_p(16, 16)  # (64,16), 64-byte blocks: three cosets
    want_c = Codec(oracle, 64, 16).parity(xc)
    dc, out_c = dev32(torch, xc), empty32(48 * 16)

    xd = below_p(96, 16)  # mixed radix, order 96 = 3 * 2^5; 64 parity blocks: fewer than the 96 the transform computes
    want_d = Codec(oracle, 160, 96, MIXED_RADIX, 96).parity(xd)
    dd, out_d = dev32(torch, xd), empty32(64 * 16)

    SE, PE = 256, 288  # (2k,k), 1 KiB blocks
    xe = below_p(K, SE)
    want_e, want_e_ntt, want_e_scaled = oracle.encode_fast(xe), oracle.ntt_fast(xe, False), oracle.scale_blocks(xe, 3, 5)
    de, de_pitched = dev32(torch, xe), dev32(torch, padded(xe, PE))
    out_e, out_e_pitched, work_e = empty32(K * SE), empty32(K * PE), empty32(K * SE)
    raw_e = rng.integers(0, 1 << 32, size=(K, SE - 1), dtype=np.uint64).astype(np.uint32)
    want_e_packed = oracle.pack_blocks(raw_e)

    KF, SF = 1 << 12, 128  # (2k,k), 512-byte blocks, an all-tile plan of three passes
    xf = below_p(KF, SF)
    want_f = oracle.encode_fast(xf)
    df, out_f = dev32(torch, xf), empty32(KF * SF)

    SG = 8192  # (2k,k), 32 KiB blocks: 32 MiB in host memory
    xg = below_p(K, SG)
    want_g = oracle.encode_fast(xg)
    out_g = np.empty_like(xg)
    rows_g = np.empty((K, SG + 16), dtype=np.uint32)  # a table of blocks that do not follow one another

    K61, E61 = 1 << 8, 16  # GF((2^61-1)^2), 256-byte blocks
    x61 = rng.integers(0, P61, size=(K61, 2 * E61), dtype=np.uint64)
    o61 = OracleP61()
    want_61, want_61_ntt = o61.encode(x61), o61.ntt(x61, False)
    want_61_back = o61.ntt(want_61_ntt, True)  # (unscaled)
    d61 = dev64(torch, x61)
    out_61, out_61_wide, work_61 = torch.empty_like(d61), torch.empty(3 * d61.numel(), dtype=torch.int64, device="cuda:0"), torch.empty_like(d61)

    CS = 1024  # the control: (3k/2,k), 4 KiB blocks
    dctl, out_ctl = dev32(torch, below_p(K, CS)), empty32(K // 2 * CS)
    torch.cuda.synchronize()

    def cycle():
        out = {}
        with fe.Encoder(K + K // 2, K, 4 * SA) as enc:  # scratch, the folded twiddle table
            enc.encode(da, out_a)
            out["fold"] = host32(out_a)
            enc.set_option("row_pitch_words", PA)  # the work stripe goes and comes back at the new pitch
            enc.encode(da_pitched, out_a_pitched)
            out["fold pitched"] = host32(out_a_pitched).reshape(-1, PA)[:, :SA]
        with fe.Encoder(130, 100, 32) as enc:  # parbuf
            enc.set_option("encode_direct_max", 0)
            enc.encode(db, out_b)
            out["zero-extended"] = host32(out_b)
        with fe.Encoder(64, 16, 64) as enc:  # scratch; from host memory: dbuf, hostpar
            enc.encode(dc, out_c)
            out["cosets"] = host32(out_c)
            got = np.empty_like(want_c)
            enc.encode(xc, got, mem=fe.MEM_HOST)
            out["cosets host"] = got
        with fe.Encoder(160, 96, 64, flags=fe.CODE_MIXED_RADIX) as enc:  # the four tables of the odd radix, mixbuf
            enc.set_option("encode_direct_max", 0)
            enc.encode(dd, out_d)
            out["mixed"] = host32(out_d)
        with fe.Encoder(2 * K, K, 4 * SE) as enc:
            enc.encode(de, out_e)
            out["encode"] = host32(out_e)
            enc.set_option("row_pitch_words", PE)
            enc.encode(de_pitched, out_e_pitched)
            out["encode pitched"] = host32(out_e_pitched).reshape(-1, PE)[:, :SE]
            enc.set_option("row_pitch_words", 0)
            for plan in (1060, 0):  # the tables are rebuilt
                enc.set_plan(plan)
                enc.encode(de, out_e)
                out["encode plan %d" % plan] = host32(out_e)
            work_e.copy_(de)
            enc.ntt(work_e)
            out["ntt"] = host32(work_e)
            enc.ntt(work_e, inverse=True)
            enc.scale_blocks(work_e, fe.gf_inv(K), 1)  # the transforms are unscaled: 1 / k closes the round trip
            out["ntt back"] = host32(work_e)
            enc.scale_blocks(work_e, 3, 5)
            out["scaled"] = host32(work_e)
            out["in range"] = np.array([enc.check_range(de), enc.check_range(xe, mem=fe.MEM_HOST)])
            enc.profile(True)
            enc.encode(de, out_e)
            torch.cuda.synchronize()
            out["profiled"] = np.array(sorted((name, launches) for name, (_, launches, _) in enc.profile_read().items()))
            enc.profile(False)
            enc.set_option("slabs", 4)
            enc.encode(de, out_e)
            out["encode slabs"] = host32(out_e)
            packed, raw_back = np.empty((K, SE), dtype=np.uint32), np.empty_like(raw_e)  # rawbuf
            enc.pack_blocks(raw_e, packed, mem=fe.MEM_HOST)
            out["unpack bad"] = np.array([enc.unpack_blocks(packed, raw_back, mem=fe.MEM_HOST)])
            out["packed"], out["unpacked"] = packed, raw_back
        with fe.Encoder(2 * KF, KF, 4 * SF) as enc:  # the slab streams and their events
            enc.set_plan(1060)
            enc.set_option("slabs", 4)
            out["slab plan"] = np.array([enc.plan()])
            enc.encode(df, out_f)
            out["slabs"] = host32(out_f)
        with fe.Encoder(2 * K, K, 4 * SG) as enc:  # both staging rings
            enc.set_option("host_pipeline", 1)
            enc.encode_host(xg, out_g)
            out["host"] = out_g.copy()
            rows_g[:, :SG] = xg
            enc.encode_blocks([rows_g[i].ctypes.data for i in range(K)])
            out["host blocks"] = rows_g[:, :SG].copy()
        with fe.Encoder(2 * K61, K61, 16 * E61, field=fe.FIELD_GF_P61_SQUARED) as enc:
            enc.encode(d61, out_61)
            out["p61"] = host64(out_61)
            for plan in (3, 0):
                enc.set_plan(plan)
                enc.encode(d61, out_61)
                out["p61 plan %d" % plan] = host64(out_61)
            work_61.copy_(d61)
            enc.ntt(work_61)
            out["p61 ntt"] = host64(work_61)
            enc.ntt(work_61, inverse=True)
            out["p61 ntt back"] = host64(work_61)
        with fe.Encoder(4 * K61, K61, 16 * E61, field=fe.FIELD_GF_P61_SQUARED) as enc:  # the cosets' factor table, scratch
            enc.encode(d61, out_61_wide)
            out["p61 cosets"] = host64(out_61_wide)
            work_61.copy_(d61)
            enc.ntt(work_61)
            out["p61 cosets ntt"] = host64(work_61)
        torch.cuda.synchronize()
        return out

    # ---- the control: a context that is held must show in the reading ----
    before = free()
    control = fe.Encoder(K + K // 2, K, 4 * CS)
    control.encode(dctl, out_ctl)
    torch.cuda.synchronize()
    held = free()
    largest = K * CS * 4  # its k-block work stripe
    assert before - held >= largest, (before, held, largest)

    first, readings = None, []
    for c in range(CYCLES):
        out = cycle()
        readings.append(free())
        print("free memory after cycle %d: %d" % (c + 1, readings[-1]))
        if first is None:
            first = out
            want = {"fold": want_a, "fold pitched": want_a, "zero-extended": want_b, "cosets": want_c, "cosets host": want_c, "mixed": want_d,
                    "encode": want_e, "encode pitched": want_e, "encode plan 1060": want_e, "encode plan 0": want_e, "ntt": want_e_ntt,
                    "ntt back": xe, "scaled": want_e_scaled, "encode slabs": want_e, "packed": want_e_packed, "unpacked": raw_e,
                    "slabs": want_f, "host": want_g, "host blocks": want_g, "p61": want_61, "p61 plan 3": want_61, "p61 plan 0": want_61,
                    "p61 ntt": want_61_ntt, "p61 ntt back": want_61_back, "p61 cosets ntt": want_61_ntt}
            for name, w in want.items():
                assert np.array_equal(out[name].reshape(w.shape), w), "cycle 1: %s differs from the oracle" % name
            assert np.array_equal(out["p61 cosets"].reshape(3 * K61, -1)[:K61], want_61), "cycle 1: the first coset is the (2k,k) parity"
            assert list(out["in range"]) == [0, 0] and list(out["unpack bad"]) == [0], (out["in range"], out["unpack bad"])
            assert len(out["profiled"]) and all(int(n) > 0 for _, n in out["profiled"]), out["profiled"]
            assert all(part.startswith("T") for part in str(out["slab plan"][0]).split()[0].split(",")), out["slab plan"]
        else:
            assert out.keys() == first.keys()
            for name in first:
                assert np.array_equal(out[name], first[name]), "cycle %d: %s differs from cycle 1" % (c + 1, name)
    print("drop from cycle 2 to cycle 8:", readings[1] - readings[-1])
    assert readings[1] - readings[-1] <= CTX_SLACK, readings

    with_control = free()
    control.close()
    torch.cuda.synchronize()
    assert free() - with_control >= largest, (with_control, free(), largest)


# The same reading for the third test, on the commit before the sharded context's members became owners: three runs of its cycles, drop from
# cycle 2 to cycle 8 of 0, 0 and 0 bytes; the largest is the slack.
SHARD_SLACK = 0


def test_sharded_contexts_give_back_their_device_memory(torch_cuda, fe, oracle):
    """The same construction for what a sharded context owns on top of its slabs' contexts: three streams, 2 x 8 + 1 events and two slab
    buffers per shard, the peer streams and events of the copy-engine all-to-all (2 G of each per shard), the fork event.  Eight identical
    cycles on four slabs of one device, (2k,k) at k = 2^10 with 1 KiB blocks: a slab is 64 words, the smallest that still runs as two
    sub-slabs.  Every data path in both gather modes, decode and repair, and a call failed by `inject_fault` with a good one after it.
    Every result equals cycle 1's bit for bit, cycle 1's equal the oracle's; free memory after cycle 8 against cycle 2; a held context of two
    slabs with 4 KiB blocks after one full-stripe encode, whose 2 x (2 + 2) MiB of slab buffers only the shards own, is the control."""
    torch = torch_cuda
    rng = np.random.default_rng(2026)
    free = lambda: torch.cuda.mem_get_info()[0]
    below_p = lambda *shape: rng.integers(0, P, size=shape, dtype=np.uint64).astype(np.uint32)
    empty32 = lambda words: torch.empty(words, dtype=torch.int32, device="cuda:0")

    # ---- everything the cycles touch, allocated up front; what the oracle says, computed once ----
    K, S, G = 1 << 10, 256, 4
    w, rows = S // G, K // G
    x = below_p(K, S)
    want = oracle.encode_fast(x)
    slabs = [dev32(torch, x[:, g * w:(g + 1) * w]) for g in range(G)]
    blocks = [dev32(torch, x[g * rows:(g + 1) * rows]) for g in range(G)]
    out_slabs, out_blocks = [empty32(K * w) for _ in range(G)], [empty32(rows * S) for _ in range(G)]
    dx, out_stripe = dev32(torch, x), empty32(K * S)
    pinned_x = torch.from_numpy(x.view(np.int32).reshape(-1)).pin_memory()
    pinned_out = torch.empty_like(pinned_x).pin_memory()
    host_out = np.empty_like(x)
    lost = ([5, 700], [9])
    present = (flags(K, lost[0]), flags(K, lost[1]))
    bad_d, bad_p = x.copy(), want.copy()
    bad_d[lost[0]] = 11
    bad_p[lost[1]] = 13
    damaged = (dev32(torch, bad_d), dev32(torch, bad_p))
    work = (torch.empty_like(damaged[0]), torch.empty_like(damaged[1]))

    CS, CG = 1024, 2  # the control: two slabs, 4 KiB blocks
    dctl, out_ctl = dev32(torch, below_p(K, CS)), empty32(K * CS)
    torch.cuda.synchronize()

    def cycle():
        out = {}
        with fe.ShardedEncoder(2 * K, K, 4 * S, [0] * G) as senc:
            assert "sub_slabs=2" in senc.plan()
            for mode in (1, 2):
                senc.set_option("gather_mode", mode)
                for t in out_slabs + out_blocks + [out_stripe, pinned_out]:
                    t.zero_()
                senc.encode_sharded(slabs, out_slabs, None)
                torch.cuda.synchronize()
                out["slabs to slabs, mode %d" % mode] = np.concatenate([host32(t).reshape(K, w) for t in out_slabs], axis=1)
                senc.encode_sharded(slabs, None, out_stripe)
                torch.cuda.synchronize()
                out["slabs to a stripe, mode %d" % mode] = host32(out_stripe)
                out_stripe.zero_()
                senc.encode(dx, out_stripe)
                torch.cuda.synchronize()
                out["device stripe, mode %d" % mode] = host32(out_stripe)
                senc.encode(pinned_x, pinned_out, mem=fe.MEM_HOST_PINNED)
                torch.cuda.synchronize()
                out["pinned stripe, mode %d" % mode] = pinned_out.numpy().view(np.uint32).copy()
                host_out.fill(0)
                senc.encode(x, host_out, mem=fe.MEM_HOST)
                out["pageable stripe, mode %d" % mode] = host_out.copy()
                for as_blocks in (False, True):  # mode 1 creates the peer streams and events
                    senc.encode_sharded_blocks(blocks if as_blocks else slabs, out_blocks, data_is_blocks=as_blocks)
                    torch.cuda.synchronize()
                    out["%s to blocks, mode %d" % ("blocks" if as_blocks else "slabs", mode)] = np.concatenate([host32(t) for t in out_blocks])
                    for t in out_blocks:
                        t.zero_()
            senc.set_option("gather_mode", 1)
            senc.decode_prepare(*present)
            for call in ("decode", "repair"):
                work[0].copy_(damaged[0])
                work[1].copy_(damaged[1])
                getattr(senc, call)(*work)
                torch.cuda.synchronize()
                out[call + ", data"], out[call + ", parity"] = host32(work[0]), host32(work[1])
            out_stripe.zero_()
            senc.set_option("inject_fault", 3)
            with pytest.raises(fe.FastEccError) as ei:
                senc.encode(dx, out_stripe)
            assert ei.value.code == fe.E_DEVICE
            senc.encode(dx, out_stripe)
            torch.cuda.synchronize()
            out["after a failed call"] = host32(out_stripe)
        torch.cuda.synchronize()
        return out

    # ---- the control: a context that is held must show in the reading ----
    before = free()
    control = fe.ShardedEncoder(2 * K, K, 4 * CS, [0] * CG)
    control.encode(dctl, out_ctl)
    torch.cuda.synchronize()
    held = free()
    largest = CG * (K + K) * (4 * CS // CG)  # every shard's data and parity slab buffers
    assert largest == 2 * (2 + 2) << 20
    assert before - held >= largest, (before, held, largest)

    first, readings = None, []
    for c in range(CYCLES):
        out = cycle()
        readings.append(free())
        print("free memory after cycle %d: %d" % (c + 1, readings[-1]))
        if first is None:
            first = out
            assert len(out) == 2 * 7 + 4 + 1, sorted(out)
            other = {"decode, data": x, "decode, parity": bad_p, "repair, data": x}  # decode leaves the parity as it found it
            for name, got in out.items():
                expect = other.get(name, want)
                assert np.array_equal(got.reshape(expect.shape), expect), "cycle 1: %s differs from the oracle" % name
        else:
            assert out.keys() == first.keys()
            for name in first:
                assert np.array_equal(out[name], first[name]), "cycle %d: %s differs from cycle 1" % (c + 1, name)
    print("drop from cycle 2 to cycle 8:", readings[1] - readings[-1])
    assert readings[1] - readings[-1] <= SHARD_SLACK, readings

    with_control = free()
    control.close()
    torch.cuda.synchronize()
    assert free() - with_control >= largest, (with_control, free(), largest)
