#!/usr/bin/env python3
"""Time fastecc_read_batch_set (degraded reads) on pools with rotated placement that lost one device, HBM-resident pools.
Pools: (20,16) x 4 KB x 32768 stripes and (256,128) x 4 KB x 4096 stripes; pattern q loses codeword block q, pattern_of[b] = b mod n.
For each pool, in the same process:
  (a) read      : fastecc_read_batch_set of every lost data block at full width into a compact buffer;
  (b) repair    : the only route before the read calls, fastecc_repair_batch_set on the pool itself with pattern_of = FASTECC_PATTERN_NONE for
                  the stripes that lost parity — the same rows read and the same number of blocks written as (a), in one launch as well;
the two alternate over three rounds, each round the median of --repeats HIP-event timings after warm-up.  Acceptance: the median of (a)'s
round medians is no larger than that of (b)'s by more than half the range of (b)'s three round medians.  The two launches alone are also
timed through the library's profile scopes (a call's HIP-event time holds the host's walk over its list as well).
Report only: the same requests with a 512-byte window, a single 4 KB degraded read (latency), and a list in which nine of ten requests are
for present blocks.  Every timed result is checked once against the original data.  One JSON line per pool; --out FILE also appends them.
  python tools/bench_read_set.py [--repeats R] [--out FILE] [--only CASE] [--read-only]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import fastecc_amd  # noqa: E402

P = 0xFFF00001
HBM_TBS = 6.3
ROUNDS = 3

# name, (n, k), block bytes, stripes
CASES = [("20_16_rot", (20, 16), 4096, 32768),
         ("256_128_rot", (256, 128), 4096, 4096)]


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
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="one case name (the kernel-trace run)")
    ap.add_argument("--read-only", action="store_true", help="time the full-width read and the repair alone (the kernel-trace run)")
    args = ap.parse_args()
    out_file = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out_file:
            out_file.write(line + "\n")
            out_file.flush()

    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda:0").manual_seed(7)
    failed = False
    for name, (n, k), block_bytes, count in CASES:
        if args.only and name != args.only:
            continue
        m, S = n - k, block_bytes // 4
        with fastecc_amd.Encoder(n, k, block_bytes) as enc:
            data = torch.randint(0, P, (count * k * S,), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32)
            parity = torch.empty(count * m * S, dtype=torch.int32, device="cuda:0")
            enc.encode_pool(data, parity, count, stream=stream)
            torch.cuda.synchronize()
            want = data.clone().view(count * k, S)
            rows_d, rows_p = data.view(count, k, S), parity.view(count, m, S)

            # rotated placement, one device down: pattern q loses codeword block q, stripe b has pattern b mod n
            dp, pp = np.ones((n, k), np.uint8), np.ones((n, m), np.uint8)
            for q in range(n):
                if q < k:
                    dp[q, q] = 0
                else:
                    pp[q, q - k] = 0
            stripe = np.arange(count, dtype=np.uint64)
            pattern_of = (stripe % n).astype(np.uint32)
            lost_data = pattern_of < k
            pattern_repair = np.where(lost_data, pattern_of, np.uint32(fastecc_amd.PATTERN_NONE)).astype(np.uint32)
            reads = (stripe[lost_data] * k + pattern_of[lost_data]).astype(np.uint64)  # every lost data block
            enc.decode_prepare_set(dp, pp)
            stripes_t = torch.arange(count, device="cuda:0")
            lost_t = stripes_t % n
            in_d, in_p = lost_t < k, lost_t >= k
            rows_d[stripes_t[in_d], lost_t[in_d]] = -1
            rows_p[stripes_t[in_p], lost_t[in_p] - k] = -1
            torch.cuda.synchronize()
            out = torch.empty(len(reads) * S, dtype=torch.int32, device="cuda:0")

            def read(r=reads, col0=0, width=S):
                enc.read_batch_set(data, parity, count, pattern_of, r, out, col0=col0, width=width, stream=stream)

            def check(r, col0, width, what):
                torch.cuda.synchronize()
                idx = torch.from_numpy(r.astype(np.int64)).to("cuda:0")
                assert torch.equal(out[:len(r) * width].view(len(r), width), want[idx, col0:col0 + width]), "%s %s" % (name, what)

            read()
            check(reads, 0, S, "read")
            # (b) works in place: the first call rebuilds the lost data blocks, the timed ones read the same rows (the rebuilt ones at weight 0) and rewrite them
            damaged = data.clone()
            repair = lambda: enc.repair_batch_set(data, parity, count, pattern_repair, stream=stream)  # noqa: E731
            repair()
            torch.cuda.synchronize()
            assert torch.equal(data.view(count * k, S), want), "%s repair" % name
            data.copy_(damaged)  # the reads below see the damaged pool again
            del damaged
            a_ms, b_ms = [], []
            for _ in range(ROUNDS):
                a_ms.append(timed(read, args.repeats))
                b_ms.append(timed(repair, args.repeats))
            # rows a request reads: the k data rows (the lost one at weight 0) and one parity row; one row written
            moved = len(reads) * (k + 2) * block_bytes
            a_med, b_med = float(np.median(a_ms)), float(np.median(b_ms))
            spread = (max(b_ms) - min(b_ms)) / 2
            ok = a_med - b_med <= spread
            failed |= not ok
            rec = dict(case=name, code="(%d,%d)" % (n, k), block_bytes=block_bytes, stripes=count, requests=int(len(reads)),
                       read_ms=round(a_med, 4), read_ms_rounds=[round(x, 4) for x in a_ms],
                       repair_none_ms=round(b_med, 4), repair_none_ms_rounds=[round(x, 4) for x in b_ms], repair_spread_ms=round(spread, 4),
                       ratio_read_over_repair=round(a_med / b_med, 3), accepted=bool(ok),
                       read_gbs=round(moved / (a_med * 1e-3) / 1e9, 1), read_hbm_share=round(moved / (a_med * 1e-3) / 1e9 / (HBM_TBS * 1e3), 3))
            # the two launches alone, from the library's profile scopes (the HIP-event timings above hold the host's work of a call as well:
            # the stream is idle while the host walks the list)
            enc.profile(True)
            for key, scope, fn in (("read_kernel_ms", "direct_read_set", read), ("repair_none_kernel_ms", "direct_pass_set", repair)):
                enc.profile_reset()
                for _ in range(5):
                    fn()
                torch.cuda.synchronize()
                ms, launches, _ = enc.profile_read()[scope]
                rec[key] = round(ms / launches, 4)
            enc.profile(False)
            if not args.read_only:
                # the pool is whole again after (b); damage it once more so that a read that copied a lost block would show
                rows_d[stripes_t[in_d], lost_t[in_d]] = -1
                read(col0=256, width=128)
                check(reads, 256, 128, "512-byte window")
                rec["read_512B_window_ms"] = round(timed(lambda: read(col0=256, width=128), args.repeats), 4)
                one = reads[len(reads) // 2:len(reads) // 2 + 1].copy()
                read(one)
                check(one, 0, S, "single read")
                rec["single_read_ms"] = round(timed(lambda: read(one), args.repeats), 4)
                # nine of ten requests for present blocks: the lost block's right-hand neighbours in the same stripes
                rng = np.random.default_rng(11)
                some = reads[::10]
                near = [(some // k) * k + (some % k + d) % k for d in range(1, 10)]
                mixed = np.concatenate([some] + near).astype(np.uint64)[:len(reads)]
                rng.shuffle(mixed)
                read(mixed)
                check(mixed, 0, S, "mixed list")
                rec["mixed_9_of_10_present_ms"] = round(timed(lambda: read(mixed), args.repeats), 4)
                rec["mixed_requests"] = int(len(mixed))
            emit(rec)
            del data, parity, want, out
            torch.cuda.empty_cache()
    if out_file:
        out_file.close()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
