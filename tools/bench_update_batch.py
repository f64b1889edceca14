#!/usr/bin/env python3
"""Time fastecc_update_batch (small writes into a pool of stripes) against a loop of fastecc_update, one call per touched stripe, on the
same HBM-resident pool.  Cases: (20,16) x 4 KB x 32768 stripes with 4096 one-block writes in distinct stripes and with one write per stripe;
(14,10) x 64 KB x 4096 with 1024 writes; (256,128) x 4 KB x 4096 with 256 writes in distinct stripes and with 64 writes in one stripe.
The pool starts all zero (a pool of codewords); calls alternate between two sets of new blocks, so every call changes every block it
names.  Median ms of --repeats calls over HIP events; the loop runs over at most 256 touched stripes and is scaled to all of them
(labelled scaled).  GB/s over the bytes moved, from the shapes: old and new rows read, the touched stripes' parity read and written once
per segment of 16 writes, the new rows read once more and stored.  A few touched stripes are checked against fastecc_encode after the
timed calls.  One JSON line per case; --out FILE also appends them there.
  python tools/bench_update_batch.py [--repeats R] [--out FILE] [--only CASE] [--batch-only]"""
import argparse
import ctypes
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

# name, (n, k), block bytes, stripes, touched stripes, writes per touched stripe
CASES = [("20_16_w4096", (20, 16), 4096, 32768, 4096, 1),
         ("20_16_w32768", (20, 16), 4096, 32768, 32768, 1),
         ("14_10_w1024", (14, 10), 65536, 4096, 1024, 1),
         ("256_128_w256", (256, 128), 4096, 4096, 256, 1),
         ("256_128_one_stripe_w64", (256, 128), 4096, 4096, 1, 64)]


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
    for name, (n, k), block_bytes, count, touched, per in CASES:
        if args.only and name != args.only:
            continue
        m, S = n - k, block_bytes // 4
        with fastecc_amd.Encoder(n, k, block_bytes) as enc:
            data = torch.zeros(count * k * S, dtype=torch.int32, device="cuda:0")
            parity = torch.zeros(count * m * S, dtype=torch.int32, device="cuda:0")
            stripes = sorted(int(b) for b in rng.permutation(count)[:touched])
            per_stripe = [sorted(int(i) for i in rng.permutation(k)[:per]) for _ in stripes]
            writes = [b * k + i for b, blocks in zip(stripes, per_stripe) for i in blocks]
            writes_arr = (ctypes.c_uint64 * len(writes))(*writes)
            w = len(writes)
            news = [torch.randint(0, P, (w * S,), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32) for _ in range(2)]
            turn = [0]

            def batch():
                turn[0] ^= 1
                code = fastecc_amd.lib().fastecc_update_batch(enc._h, data.data_ptr(), parity.data_ptr(), count, writes_arr, w, news[turn[0]].data_ptr(),
                                                              stream or None)
                assert code == 0, code

            def check(what, upto):  # the first, middle and last of the first `upto` touched stripes
                torch.cuda.synchronize()
                rows = news[turn[0]].view(w, S)
                for t in sorted({0, upto // 2, upto - 1}):
                    b = stripes[t]
                    d = data[b * k * S:(b + 1) * k * S]
                    assert torch.equal(d.view(k, S)[per_stripe[t]], rows[t * per:(t + 1) * per]), "%s %s: data of stripe %d" % (name, what, b)
                    want = torch.empty(m * S, dtype=torch.int32, device="cuda:0")
                    enc.encode(d, want)
                    torch.cuda.synchronize()
                    assert torch.equal(parity[b * m * S:(b + 1) * m * S], want), "%s %s: parity of stripe %d" % (name, what, b)

            batch()
            check("batch", len(stripes))
            batch_ms, batch_min = timed(batch, args.repeats)
            check("batch, timed", len(stripes))
            if args.batch_only:
                emit(dict(case=name, ms=round(batch_ms, 4), ms_min=round(batch_min, 4)))
                continue
            loop_n = min(LOOP_STRIPES, len(stripes))
            lists = [fastecc_amd.Encoder._block_list(blocks)[1] for blocks in per_stripe[:loop_n]]

            def loop():
                turn[0] ^= 1
                base = news[turn[0]].data_ptr()
                for t in range(loop_n):
                    b = stripes[t]
                    code = fastecc_amd.lib().fastecc_update(enc._h, data.data_ptr() + b * k * S * 4, parity.data_ptr() + b * m * S * 4, lists[t], per,
                                                            base + t * per * S * 4, fastecc_amd.MEM_DEVICE, stream or None)
                    assert code == 0, code

            loop()
            check("loop", loop_n)
            loop_ms, _ = timed(loop, args.repeats)
            scaled = loop_ms * len(stripes) / loop_n
            segments = len(stripes) * ((per + 15) // 16)
            moved = (2 * w + 2 * segments * m + 2 * w) * block_bytes
            gbs = moved / (batch_ms * 1e-3) / 1e9
            emit(dict(case=name, code="(%d,%d)" % (n, k), block_bytes=block_bytes, stripes=count, touched_stripes=len(stripes), writes=w,
                      ms=round(batch_ms, 4), ms_min=round(batch_min, 4), bytes_moved=moved, gbs=round(gbs, 1), hbm_share=round(gbs / (HBM_TBS * 1e3), 4),
                      update_loop_ms_scaled=round(scaled, 3), update_loop_stripes=loop_n, update_loop_us_per_call=round(loop_ms * 1e3 / loop_n, 2),
                      ratio_update_loop_scaled=round(scaled / batch_ms, 1)))
            del data, parity, news
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
