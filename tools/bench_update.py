#!/usr/bin/env python3
"""Time the parity update for small writes against a fresh encode, 4 KB blocks, HBM-resident stripes.
Codes: (2^20, 2^19) and (2^19 + 16, 2^19).  For t changed blocks in {1, 4, 16, 24, 32, 40, 64, 256}: fastecc_update_parity and fastecc_update
(median ms over HIP events around each call), and the GB/s of parity read + written (8 bytes per parity word, the pass count times
for t > 16) with its share of the 6.3 TB/s achievable HBM rate; fastecc_encode of the same code in the same run.  The results are
checked once against the encode.  One JSON line per case; --out FILE also appends them there.
  python tools/bench_update.py [--repeats R] [--out FILE] [--counts 1,4,16] [--headline-only]"""
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
ROWS_PER_PASS = 16  # update.hip ROWS


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
    ap.add_argument("--counts", default="1,4,16,24,32,40,64,256", help="changed blocks per call, comma-separated")
    ap.add_argument("--headline-only", action="store_true", help="only the (2^20, 2^19) code (counter runs)")
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    S = 1024
    k = 1 << 19
    g = torch.Generator(device="cuda:0").manual_seed(11)
    data = torch.randint(0, P, (k * S,), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(5)
    for n in ((2 * k,) if args.headline_only else (2 * k, k + 16)):
        m = n - k
        base = {"code": "(%d,%d)" % (n, k), "block_bytes": 4 * S}
        parity = torch.empty(m * S, dtype=torch.int32, device="cuda:0")
        with fastecc_amd.Encoder(n, k, 4 * S) as enc:
            ms, best = timed(lambda: enc.encode(data, parity, stream=stream), args.repeats)
            emit(dict(base, case="encode", ms=round(ms, 4), ms_min=round(best, 4)))
            for t in [int(x) for x in args.counts.split(",")]:
                blocks = [int(b) for b in rng.choice(k, size=t, replace=False)]
                idx = torch.tensor(blocks, device="cuda:0", dtype=torch.int64)
                rows = data.view(k, S)
                new = torch.randint(0, P, (t * S,), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32)
                old = rows[idx].reshape(-1).clone()
                enc.encode(data, parity, stream=stream)
                # correctness once: update, then compare with the encode of the new stripe; then back to the old blocks
                enc.update(data, parity, blocks, new, stream=stream)
                want = torch.empty_like(parity)
                enc.encode(data, want, stream=stream)
                torch.cuda.synchronize()
                assert torch.equal(parity, want), "update differs from encode at t=%d" % t
                assert torch.equal(rows[idx].reshape(-1), new)
                del want
                enc.update_parity(parity, blocks, old, old=new, stream=stream)
                rows[idx] = old.view(t, S)
                torch.cuda.synchronize()
                passes = (t + ROWS_PER_PASS - 1) // ROWS_PER_PASS
                moved = passes * m * S * 8
                ms_p, best_p = timed(lambda: enc.update_parity(parity, blocks, new, old=old, stream=stream), args.repeats)
                # fastecc_update alternates the stripe between the two versions of the blocks (same work every call)
                state = {"flip": False}

                def upd():
                    enc.update(data, parity, blocks, old if state["flip"] else new, stream=stream)
                    state["flip"] = not state["flip"]
                ms_u, best_u = timed(upd, args.repeats + (args.repeats % 2))
                for case, v, b in (("update_parity", ms_p, best_p), ("update", ms_u, best_u)):
                    gbs = moved / (v * 1e-3) / 1e9
                    emit(dict(base, case=case, t=t, passes=passes, ms=round(v, 4), ms_min=round(b, 4), parity_gbs=round(gbs, 1),
                              hbm_share=round(gbs / (HBM_TBS * 1e3), 3), encode_ms=round(ms, 4)))
                if state["flip"]:  # leave the stripe as it was
                    upd()
                torch.cuda.synchronize()
        del parity
    if out:
        out.close()


if __name__ == "__main__":
    main()
