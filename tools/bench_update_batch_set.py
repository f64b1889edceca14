#!/usr/bin/env python3
"""Time fastecc_update_batch_set (small writes into a pool with one device down) against fastecc_update_batch of the SAME write list on the same
pool kept whole.  Cases: rotated (20,16) x 4 KB x 32768 stripes and (256,128) x 4 KB x 4096, placement (i + b) mod n with device 0 down (stripe b
loses codeword block (-b) mod n: n patterns), one uniformly random write per stripe.  Both pools start all zero (pools of codewords); the
degraded one then gets garbage in every absent block.  Calls alternate between two sets of new blocks, so every call changes every block it
names.  Median ms of --repeats calls over HIP events for both (an interval holds the call's host work as well: the stream is idle when a call starts),
their ratio, the share of the writes that hit an absent block, and where the time goes: the host's median time inside the call and the device's
time by profile scope (fastecc_profile_read, mean of 5 calls).  After the timed
calls a few touched stripes of the degraded pool are checked against the oracle: present data blocks, present parity blocks, absent blocks
unchanged.  One JSON line per case, appended to --out (default profiles/update_batch_set/bench_update_batch_set.jsonl).
  python tools/bench_update_batch_set.py [--repeats R] [--out FILE] [--only CASE]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import fastecc_amd  # noqa: E402
from oracle import Oracle  # noqa: E402
from pool_model import Codec  # noqa: E402

P = 0xFFF00001
DEFAULT_OUT = os.path.join(ROOT, "profiles", "update_batch_set", "bench_update_batch_set.jsonl")

# name, (n, k), block bytes, stripes
CASES = [("20_16_rotated_one_down", (20, 16), 4096, 32768),
         ("256_128_rotated_one_down", (256, 128), 4096, 4096)]


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--only", default=None, help="one case name")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "a")
    oracle = Oracle()
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda:0").manual_seed(7)
    rng = np.random.default_rng(3)
    for name, (n, k), block_bytes, count in CASES:
        if args.only and name != args.only:
            continue
        m, S = n - k, block_bytes // 4
        codec = Codec(oracle, n, k)
        with fastecc_amd.Encoder(n, k, block_bytes) as enc:
            dp, pp = np.ones((n, k), np.uint8), np.ones((n, m), np.uint8)
            for u in range(n):  # pattern u loses codeword block u
                (dp if u < k else pp)[u, u if u < k else u - k] = 0
            enc.decode_prepare_set(dp, pp)
            pattern_of = np.array([(-b) % n for b in range(count)], dtype=np.uint32)
            po = pattern_of.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
            pools = {}
            for kind in ("degraded", "whole"):
                pools[kind] = (torch.zeros(count * k * S, dtype=torch.int32, device="cuda:0"), torch.zeros(count * m * S, dtype=torch.int32, device="cuda:0"))
            data, parity = pools["degraded"]
            lost = torch.from_numpy(pattern_of.astype(np.int64)).to("cuda:0")
            stripe = torch.arange(count, device="cuda:0")
            junk = torch.randint(0, 1 << 31, (count, S), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32) | -0x100000  # words >= p
            dsel, psel = lost < k, lost >= k
            data.view(count, k, S)[stripe[dsel], lost[dsel]] = junk[dsel]
            parity.view(count, m, S)[stripe[psel], lost[psel] - k] = junk[psel]
            blocks = rng.integers(0, k, size=count)
            writes = [b * k + int(i) for b, i in enumerate(blocks)]
            writes_arr = (ctypes.c_uint64 * count)(*writes)
            absent = int(np.count_nonzero(blocks == pattern_of))
            news = [torch.randint(0, P, (count * S,), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32) for _ in range(2)]
            turn = [0, 0]
            L = fastecc_amd.lib()

            def degraded():
                turn[0] ^= 1
                code = L.fastecc_update_batch_set(enc._h, data.data_ptr(), parity.data_ptr(), count, po, writes_arr, count, news[turn[0]].data_ptr(), stream or None)
                assert code == 0, code

            def whole():
                turn[1] ^= 1
                d, p = pools["whole"]
                code = L.fastecc_update_batch(enc._h, d.data_ptr(), p.data_ptr(), count, writes_arr, count, news[turn[1]].data_ptr(), stream or None)
                assert code == 0, code

            def check(what):  # the first, a middle and the last stripe, and the first one whose written block is absent
                torch.cuda.synchronize()
                rows = news[turn[0]].view(count, S)
                hit = np.flatnonzero(blocks == pattern_of)
                for b in sorted({0, count // 2, count - 1} | ({int(hit[0])} if len(hit) else set())):
                    x = np.zeros((k, S), np.uint32)
                    x[blocks[b]] = rows[b].cpu().numpy().view(np.uint32)
                    want = np.concatenate([x, codec.parity(x)])
                    got = np.concatenate([data.view(count, k, S)[b].cpu().numpy(), parity.view(count, m, S)[b].cpu().numpy()]).view(np.uint32)
                    u = int(pattern_of[b])
                    present = [j for j in range(n) if j != u]
                    assert np.array_equal(got[present], want[present]), "%s %s: present blocks of stripe %d" % (name, what, b)
                    assert np.array_equal(got[u], junk[b].cpu().numpy().view(np.uint32)), "%s %s: the absent block of stripe %d was written" % (name, what, b)

            degraded()
            check("first call")
            set_ms, set_min = timed(degraded, args.repeats)
            check("timed calls")
            whole_ms, whole_min = timed(whole, args.repeats)

            def split(fn):
                """where a call's time goes: the host's share (the call returns; nothing waits for the device) and the device's by profile scope"""
                host = []
                for _ in range(args.repeats):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    host.append((time.perf_counter() - t0) * 1e3)
                torch.cuda.synchronize()
                enc.profile(True)
                enc.profile_reset()
                for _ in range(5):
                    fn()
                torch.cuda.synchronize()
                scopes = {name: round(ms / 5, 4) for name, (ms, _, _) in enc.profile_read().items()}
                enc.profile(False)
                return round(float(np.median(host)), 4), scopes

            set_host, set_scopes = split(degraded)
            whole_host, whole_scopes = split(whole)
            check("profiled calls")
            rec = dict(case=name, code="(%d,%d)" % (n, k), block_bytes=block_bytes, stripes=count, writes=count, writes_on_absent_blocks=absent,
                       absent_share=round(absent / count, 4), update_batch_set_ms=round(set_ms, 4), update_batch_set_ms_min=round(set_min, 4),
                       update_batch_whole_ms=round(whole_ms, 4), update_batch_whole_ms_min=round(whole_min, 4), ratio=round(set_ms / whole_ms, 3),
                       update_batch_set_host_ms=set_host, update_batch_whole_host_ms=whole_host, update_batch_set_device_ms_by_scope=set_scopes,
                       update_batch_whole_device_ms_by_scope=whole_scopes)
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
            del data, parity, pools, news, junk
            torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
