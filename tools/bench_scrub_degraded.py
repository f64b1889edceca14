#!/usr/bin/env python3
"""Time the scrub of a degraded pool (fastecc_scrub_erasures + fastecc_verify_batch / fastecc_verify), HBM-resident.
Cases: (20,16) x 4 KB x 32768 stripes and (256,128) x 4 KB x 4096 stripes, verify_batch with 0 and with 1 absent block;
(2^20,2^19) x 4 KB, fastecc_verify with 0 and with 2^17 absent blocks.  For each row: the median and the spread (min, max) of R
HIP-event-timed calls, the bytes the call reads (absent blocks are not read), GB/s over them and the share of 6.3 TB/s, and the
fingerprint kernel's time and byte count from the library profile.  The absent blocks are overwritten with 0xFFFFFFFF words before the
degraded rows are timed, and every timed configuration is checked first: the call must report the pool consistent.
A library without fastecc_scrub_erasures (the commit before it: run this same script in that tree) gives the 0-absent rows only; --label
names the library in every record, so the rows of both land in one file:  the 0-absent rows of the two are the comparison that shows
what the skip costs the present blocks, each with the spread between its repeats (--runs repeats the whole measurement).
  python tools/bench_scrub_degraded.py [--repeats R] [--runs N] [--label NAME] [--out FILE] [--only CASE]"""
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
SEED = 0x5C8B
DEFAULT_OUT = os.path.join(ROOT, "profiles", "scrub_degraded", "bench_scrub_degraded.jsonl")

# name, (n, k), block bytes, stripes (0: the single-stripe call), absent blocks of the degraded row
CASES = [("20_16", (20, 16), 4096, 32768, 1),
         ("256_128", (256, 128), 4096, 4096, 1),
         ("2^20_2^19", (1 << 20, 1 << 19), 4096, 0, 1 << 17)]


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
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--runs", type=int, default=1, help="repeat every measurement this many times (the spread between runs)")
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda:0").manual_seed(11)
    for name, (n, k), block_bytes, count, w_degraded in CASES:
        if args.only and name != args.only:
            continue
        m, S, stripes = n - k, block_bytes // 4, max(count, 1)
        with fastecc_amd.Encoder(n, k, block_bytes) as enc:
            data = torch.randint(0, P, (stripes * k * S,), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32)
            parity = torch.empty(stripes * m * S, dtype=torch.int32, device="cuda:0")
            for b in range(stripes):
                enc.encode(data.data_ptr() + b * k * S * 4, parity.data_ptr() + b * m * S * 4, stream=stream)
            torch.cuda.synchronize()
            if count:
                call, kernel = (lambda: enc.verify_batch(data, parity, count, seed=SEED, stream=stream).all()), "fingerprint_batch"
            else:
                call, kernel = (lambda: enc.verify(data, parity, seed=SEED, stream=stream)), "fingerprint"
            rows = [0] + ([w_degraded] if hasattr(enc, "scrub_erasures") else [])
            for w in rows:
                if w:  # the device that is down held data block 1 (w = 1), or every fourth data block: overwrite them, name them absent
                    dp = np.ones(k, np.uint8)
                    dp[1] = 0
                    if w > 1:
                        dp[:] = 1
                        dp[:4 * w:4] = 0
                    assert int((dp == 0).sum()) == w
                    data.view(stripes, k, S)[:, torch.from_numpy(dp == 0).to("cuda:0"), :] = -1
                    torch.cuda.synchronize()
                    assert not call(), "%s: garbage in the absent blocks went unnoticed without a pattern" % name
                    enc.scrub_erasures(dp, None)
                assert call(), "%s: pool reported inconsistent (absent %d)" % (name, w)
                read = stripes * (n - w) * block_bytes
                for run in range(args.runs):
                    ms, ms_min, ms_max = timed(call, args.repeats)
                    enc.profile(True)
                    enc.profile_reset()
                    call()
                    prof = enc.profile_read()
                    enc.profile(False)
                    fp_ms, _, fp_bytes = prof.get(kernel, (0.0, 0, 0))
                    gbs = read / (ms * 1e-3) / 1e9
                    emit(dict(library=args.label, case=name, code="(%d,%d)" % (n, k), block_bytes=block_bytes, stripes=stripes,
                              call="verify_batch" if count else "verify", absent=w, run=run, repeats=args.repeats, bytes_read=read,
                              ms=round(ms, 4), ms_min=round(ms_min, 4), ms_max=round(ms_max, 4), gbs=round(gbs, 1),
                              hbm_share=round(gbs / (HBM_TBS * 1e3), 3), fingerprint_ms=round(fp_ms, 4), fingerprint_bytes=fp_bytes,
                              profile={kk: round(v[0], 4) for kk, v in prof.items()}))
            del data, parity
            torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
