#!/usr/bin/env python3
"""Time fastecc_verify_batch / fastecc_correct_batch (scrubbing a pool of stripes) against a loop of the single-stripe calls, HBM-resident.
Cases: (20,16) x 4 KB x 32768 stripes, (14,10) x 64 KB x 4096, (256,128) x 4 KB x 4096, (2^20,2^19) x 4 KB x 2.  For each: the batch
verify (median ms over HIP events around the synchronous call), GB/s over the codeword bytes read and its share of 6.3 TB/s, the
fingerprint_batch kernel's time from the library profile, a Python loop of fastecc_verify over the first 256 stripes scaled to the whole
count (labelled scaled), and fastecc_correct_batch with 1 of 4096 stripes (at least one) corrupted in one block.  Every timed result is
checked: the clean pool verifies consistent, the corrupted stripes are the ones flagged, and correct_batch restores them.  One JSON line
per case; --out FILE also appends them there.
  python tools/bench_scrub_batch.py [--repeats R] [--out FILE] [--only CASE] [--batch-only]"""
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
SEED = 0x5C8B

# name, (n, k), block bytes, stripes
CASES = [("20_16", (20, 16), 4096, 32768),
         ("14_10", (14, 10), 65536, 4096),
         ("256_128", (256, 128), 4096, 4096),
         ("2^20_2^19", (1 << 20, 1 << 19), 4096, 2)]


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
    ap.add_argument("--batch-only", action="store_true", help="time the batched verify alone (the kernel-trace run)")
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda:0").manual_seed(11)
    rng = np.random.default_rng(5)
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
            ok = enc.verify_batch(data, parity, count, seed=SEED, stream=stream)
            assert ok.all(), "%s: clean pool reported inconsistent" % name
            ms, ms_min = timed(lambda: enc.verify_batch(data, parity, count, seed=SEED, stream=stream), args.repeats)
            if args.batch_only:
                emit(dict(case=name, ms=round(ms, 4), ms_min=round(ms_min, 4)))
                continue
            enc.profile(True)
            enc.profile_reset()
            enc.verify_batch(data, parity, count, seed=SEED, stream=stream)
            prof = enc.profile_read()
            enc.profile(False)
            fp_ms = prof.get("fingerprint_batch", (0.0,))[0]
            read = count * n * block_bytes

            loop_n = min(LOOP_STRIPES, count)

            def loop():
                for b in range(loop_n):
                    assert enc.verify(data.data_ptr() + b * k * S * 4, parity.data_ptr() + b * m * S * 4, seed=SEED, stream=stream)
            loop_ms, _ = timed(loop, max(5, args.repeats // 4))
            loop_scaled = loop_ms * count / loop_n

            # correct_batch: 1 of 4096 stripes (at least one) with one changed word in one block
            rows_d, rows_p = data.view(count, k, S), parity.view(count, m, S)
            bad = sorted(int(x) for x in rng.choice(count, size=max(1, count // 4096), replace=False))
            blk = [int(rng.integers(n)) for _ in bad]
            keep = [(rows_d[b, j] if j < k else rows_p[b, j - k]).clone() for b, j in zip(bad, blk)]

            def corrupt():
                for b, j in zip(bad, blk):
                    row = rows_d[b, j] if j < k else rows_p[b, j - k]
                    row[7] ^= 1  # (a word >= p at worst: also a corruption the scrub repairs)
            corrupt()
            torch.cuda.synchronize()
            flags = enc.verify_batch(data, parity, count, seed=SEED, stream=stream)
            assert sorted(np.nonzero(~flags)[0].tolist()) == bad, name
            cts = []
            for rep in range(max(3, args.repeats // 4)):
                if rep:
                    corrupt()
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                status = enc.correct_batch(data, parity, count, seed=SEED, stream=stream)
                e.record()
                e.synchronize()
                cts.append(a.elapsed_time(e))
                assert sorted(np.nonzero(status)[0].tolist()) == bad and (status[bad] == 1).all(), name
                for (b, j), want in zip(zip(bad, blk), keep):
                    assert torch.equal(rows_d[b, j] if j < k else rows_p[b, j - k], want), name
            correct_ms = float(np.median(cts))
            gbs = read / (ms * 1e-3) / 1e9
            emit(dict(case=name, code="(%d,%d)" % (n, k), block_bytes=block_bytes, stripes=count, bytes_read=read,
                      verify_batch_ms=round(ms, 4), verify_batch_ms_min=round(ms_min, 4), gbs=round(gbs, 1), hbm_share=round(gbs / (HBM_TBS * 1e3), 3),
                      fingerprint_batch_ms=round(fp_ms, 4), profile={kk: round(v[0], 4) for kk, v in prof.items()},
                      verify_loop_ms_scaled=round(loop_scaled, 3), verify_loop_stripes=loop_n,
                      ratio_verify_loop_scaled=round(loop_scaled / ms, 1),
                      correct_batch_ms=round(correct_ms, 4), correct_batch_corrupted=len(bad)))
            del data, parity, rows_d, rows_p
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
