#!/usr/bin/env python3
"""Time fastecc_repair_batch_set on pools with rotated placement that lost one device, HBM-resident pools (128 MiB and more).
Pools: (20,16) x 4 KB x 32768 stripes and (256,128) x 4 KB x 4096 stripes; pattern q loses codeword block q, pattern_of[b] = b mod n.
For each pool, in the same process:
  (a) set       : fastecc_repair_batch_set of the whole pool (option decode_batch_kernel = 0, what the library chooses);
  (b) loop      : the only public route before the set calls, fastecc_decode_prepare + fastecc_repair stripe by stripe, over the first 256
                  stripes and scaled to the whole count (labelled scaled);
  (c) same      : fastecc_repair_batch of the same pool with ONE pattern, data block 0 lost in every stripe: the same bytes to within one
                  row per stripe (a rotated stripe that lost a parity block reads no parity row) — the yardstick;
and the set-up time of fastecc_decode_prepare_set for the pool's n patterns (host clock around the synchronous call, median of 5).
Median ms over HIP events; every timed result is checked once against the original pool.  One JSON line per pool; --out FILE also appends them.
  python tools/bench_repair_set.py [--repeats R] [--out FILE] [--only CASE] [--set-only]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import fastecc_amd  # noqa: E402

P = 0xFFF00001
HBM_TBS = 6.3
LOOP_STRIPES = 256

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
    return float(np.median(ts)), float(min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="one case name (the kernel-trace run)")
    ap.add_argument("--set-only", action="store_true", help="time the set call and the same-pattern batch alone (the kernel-trace run)")
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda:0").manual_seed(7)
    for name, (n, k), block_bytes, count in CASES:
        if args.only and name != args.only:
            continue
        m, S = n - k, block_bytes // 4
        with fastecc_amd.Encoder(n, k, block_bytes) as enc:
            data = torch.randint(0, P, (count * k * S,), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32)
            parity = torch.empty(count * m * S, dtype=torch.int32, device="cuda:0")
            if n == 2 * k:
                enc.encode_batch(data, parity, count, stream=stream)
            else:
                for b in range(count):
                    enc.encode(data.data_ptr() + b * k * S * 4, parity.data_ptr() + b * m * S * 4, stream=stream)
            torch.cuda.synchronize()
            rows_d, rows_p = data.view(count, k, S), parity.view(count, m, S)
            want_d, want_p = data.clone(), parity.clone()

            # rotated placement, one device down: pattern q loses codeword block q, stripe b has pattern b mod n
            dp, pp = np.ones((n, k), np.uint8), np.ones((n, m), np.uint8)
            for q in range(n):
                if q < k:
                    dp[q, q] = 0
                else:
                    pp[q, q - k] = 0
            pattern_of = (np.arange(count, dtype=np.uint64) % n).astype(np.uint32)
            setup = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                enc.decode_prepare_set(dp, pp)
                setup.append((time.perf_counter() - t0) * 1e3)
            stripes = torch.arange(count, device="cuda:0")
            lost = stripes % n

            def erase_rotated(upto=count):
                in_d, in_p = (lost < k) & (stripes < upto), (lost >= k) & (stripes < upto)
                rows_d[stripes[in_d], lost[in_d]] = -1
                rows_p[stripes[in_p], lost[in_p] - k] = -1

            def verify(what):
                torch.cuda.synchronize()
                assert torch.equal(data, want_d) and torch.equal(parity, want_p), "%s %s" % (name, what)

            enc.set_option("decode_batch_kernel", 0)
            erase_rotated()
            enc.repair_batch_set(data, parity, count, pattern_of, stream=stream)
            verify("set")
            set_ms = timed(lambda: enc.repair_batch_set(data, parity, count, pattern_of, stream=stream), args.repeats)

            # (c) the same pool, one pattern: data block 0 lost in every stripe
            one_d, one_p = np.ones(k, np.uint8), np.ones(m, np.uint8)
            one_d[0] = 0
            enc.decode_prepare(one_d, one_p)
            rows_d[:, 0] = -1
            enc.repair_batch(data, parity, count, stream=stream)
            verify("same pattern")
            same_ms = timed(lambda: enc.repair_batch(data, parity, count, stream=stream), args.repeats)

            # bytes the result depends on: per stripe the k data rows (the lost one included, at weight 0), one parity row when a data block
            # was lost, and the row written
            lost_data_stripes = int((lost < k).sum())
            moved_set = (count * (k + 1) + lost_data_stripes) * block_bytes
            moved_same = count * (k + 2) * block_bytes
            rec = dict(case=name, code="(%d,%d)" % (n, k), block_bytes=block_bytes, stripes=count, patterns=n,
                       set_ms=round(set_ms[0], 4), set_ms_min=round(set_ms[1], 4),
                       same_pattern_batch_ms=round(same_ms[0], 4), same_pattern_batch_ms_min=round(same_ms[1], 4),
                       ratio_set_over_same=round(set_ms[0] / same_ms[0], 3), bytes_set_over_same=round(moved_set / moved_same, 4),
                       set_gbs=round(moved_set / (set_ms[0] * 1e-3) / 1e9, 1), set_hbm_share=round(moved_set / (set_ms[0] * 1e-3) / 1e9 / (HBM_TBS * 1e3), 3),
                       prepare_set_ms=round(float(np.median(setup)), 3), prepare_set_ms_first=round(setup[0], 3))
            if not args.set_only:
                # (b) the per-stripe route over the first LOOP_STRIPES stripes: a prepare and a repair each
                def loop():
                    for b in range(LOOP_STRIPES):
                        q = b % n
                        enc.decode_prepare(dp[q], pp[q])
                        enc.repair(data.data_ptr() + b * k * S * 4, parity.data_ptr() + b * m * S * 4, stream=stream)
                erase_rotated(LOOP_STRIPES)
                loop()
                verify("loop")
                loop_ms, _ = timed(loop, max(5, args.repeats // 4))
                rec.update(loop_ms_scaled=round(loop_ms * count / LOOP_STRIPES, 3), loop_stripes=LOOP_STRIPES,
                           ratio_loop_scaled_over_set=round(loop_ms * count / LOOP_STRIPES / set_ms[0], 1))
            emit(rec)
            del data, parity, want_d, want_p
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
