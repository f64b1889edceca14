#!/usr/bin/env python3
"""Time fastecc_decode_batch / fastecc_repair_batch against the stripe-by-stripe forms, HBM-resident batches (> 256 MiB).
Cases: (256,128) x 4 KB x 4096 stripes with 1, 4, 16, 64 lost data blocks (decode) and 2 data + 2 parity (repair); (14,10) x 64 KB x 4096
with 1 and 4 lost; (20,16) x 4 KB x 32768 with 1 and 4 lost.  For each: the batch (option decode_batch_kernel = 0, what the library chooses),
the same call with decode_batch_kernel = 2 (direct_run stripe by stripe inside the library) and a Python loop of fastecc_decode /
fastecc_repair over the first 256 stripes scaled to the whole count (labelled scaled); for (256,128) also fastecc_encode_batch of the same
stripes.  Median ms over HIP events; GB/s of survivor rows read + lost rows written (from the shapes) and its share of 6.3 TB/s.  Every
timed result is checked once against the original stripes.  One JSON line per case; --out FILE also appends them there.
  python tools/bench_decode_batch.py [--repeats R] [--out FILE] [--only CASE] [--batch-only]"""
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
LOOP_STRIPES = 256

# name, (n, k), block bytes, stripes, lost data, lost parity, op
CASES = [("256_128_d1", (256, 128), 4096, 4096, 1, 0, "decode"),
         ("256_128_d4", (256, 128), 4096, 4096, 4, 0, "decode"),
         ("256_128_d16", (256, 128), 4096, 4096, 16, 0, "decode"),
         ("256_128_d64", (256, 128), 4096, 4096, 64, 0, "decode"),
         ("256_128_r2p2", (256, 128), 4096, 4096, 2, 2, "repair"),
         ("14_10_d1", (14, 10), 65536, 4096, 1, 0, "decode"),
         ("14_10_d4", (14, 10), 65536, 4096, 4, 0, "decode"),
         ("20_16_d1", (20, 16), 4096, 32768, 1, 0, "decode"),
         ("20_16_d4", (20, 16), 4096, 32768, 4, 0, "decode")]


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
    ap.add_argument("--batch-only", action="store_true", help="time the batched call alone (the kernel-trace run)")
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
    rng = np.random.default_rng(3)
    for name, (n, k), block_bytes, count, ld, lp, op in CASES:
        if args.only and name != args.only:
            continue
        m, S = n - k, block_bytes // 4
        with fastecc_amd.Encoder(n, k, block_bytes) as enc:
            data = torch.randint(0, P, (count * k * S,), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32)
            parity = torch.empty(count * m * S, dtype=torch.int32, device="cuda:0")
            enc_ms = None
            if n == 2 * k:
                enc.encode_batch(data, parity, count, stream=stream)
                enc_ms, _ = timed(lambda: enc.encode_batch(data, parity, count, stream=stream), args.repeats)
            else:
                for b in range(count):
                    enc.encode(data.data_ptr() + b * k * S * 4, parity.data_ptr() + b * m * S * 4, stream=stream)
            torch.cuda.synchronize()
            lost_d = sorted(int(x) for x in rng.permutation(k)[:ld])
            lost_p = sorted(int(x) for x in rng.permutation(m)[:lp])
            dp, pp = np.ones(k, np.uint8), np.ones(m, np.uint8)
            dp[lost_d], pp[lost_p] = 0, 0
            enc.decode_prepare(dp, pp)
            rows_d, rows_p = data.view(count, k, S), parity.view(count, m, S)
            want_d, want_p = rows_d[:, lost_d].clone(), rows_p[:, lost_p].clone()

            def erase():
                rows_d[:, lost_d] = -1
                if lost_p:
                    rows_p[:, lost_p] = -1

            def verify(what):
                torch.cuda.synchronize()
                assert torch.equal(rows_d[:, lost_d], want_d), "%s %s: data" % (name, what)
                if op == "repair" and lost_p:
                    assert torch.equal(rows_p[:, lost_p], want_p), "%s %s: parity" % (name, what)

            batch = enc.repair_batch if op == "repair" else enc.decode_batch
            single = enc.repair if op == "repair" else enc.decode
            res = {}
            for mode, label in ((0, "batch"),) + (() if args.batch_only else ((2, "per_stripe"),)):
                enc.set_option("decode_batch_kernel", mode)
                erase()
                batch(data, parity, count, stream=stream)
                verify(label)
                res[label] = timed(lambda: batch(data, parity, count, stream=stream), args.repeats)
            enc.set_option("decode_batch_kernel", 0)
            if args.batch_only:
                emit(dict(case=name, ms=round(res["batch"][0], 4), ms_min=round(res["batch"][1], 4)))
                continue

            def loop():
                for b in range(LOOP_STRIPES):
                    single(data.data_ptr() + b * k * S * 4, parity.data_ptr() + b * m * S * 4, stream=stream)
            erase()
            loop()
            torch.cuda.synchronize()
            assert torch.equal(rows_d[:LOOP_STRIPES, lost_d], want_d[:LOOP_STRIPES]), name
            loop_ms, _ = timed(loop, max(5, args.repeats // 4))
            # survivor rows read: the direct path reads k data rows (lost ones included) + one parity row per lost data row;
            # the bytes counted here are those of the blocks the result depends on: surviving data + those parity rows, plus the rows written
            outputs = ld + (lp if op == "repair" else 0)
            moved = count * ((k - ld) + ld + outputs) * block_bytes
            ms = res["batch"][0]
            gbs = moved / (ms * 1e-3) / 1e9
            rec = dict(case=name, code="(%d,%d)" % (n, k), block_bytes=block_bytes, stripes=count, lost_data=ld, lost_parity=lp, op=op,
                       ms=round(ms, 4), ms_min=round(res["batch"][1], 4), gbs=round(gbs, 1), hbm_share=round(gbs / (HBM_TBS * 1e3), 3),
                       per_stripe_ms=round(res["per_stripe"][0], 4), ratio_per_stripe=round(res["per_stripe"][0] / ms, 1),
                       python_loop_ms_scaled=round(loop_ms * count / LOOP_STRIPES, 3), python_loop_stripes=LOOP_STRIPES,
                       ratio_python_loop_scaled=round(loop_ms * count / LOOP_STRIPES / ms, 1))
            if enc_ms is not None:
                rec["encode_batch_ms"] = round(enc_ms, 4)
            emit(rec)
            del data, parity, want_d, want_p
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
