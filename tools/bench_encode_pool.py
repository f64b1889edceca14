#!/usr/bin/env python3
"""Time fastecc_encode_pool under option "encode_pool_kernel" = 1 (VALU batch kernel), 2 (matrix-core pool kernel), 3 (stripe by stripe, the only
way before the call existed) and 0 (what the library chooses), on HBM-resident pools of 4 KB blocks: (20,16) x 32768 stripes (the README pool,
2 GiB of data) and (24,16), (48,32), (96,64) at 1 GiB of data.  Modes 1 and 2 are timed alternately in the same window (HIP events around each
call, median and minimum); mode 3 is one launch-bound loop of fastecc_encode's kernels inside the library and is timed a few times only.  Every
mode's parity is compared once with mode 3's.  GB/s = count * n * block_bytes (data read once + parity written once, from the shapes) over the
median, and its share of 6.3 TB/s.  One JSON line per case; --out FILE also appends them there.
  python tools/bench_encode_pool.py [--repeats R] [--out FILE] [--only CASE]"""
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

# name, (n, k), block bytes, stripes
CASES = [("20_16", (20, 16), 4096, 32768),
         ("24_16", (24, 16), 4096, 16384),
         ("48_32", (48, 32), 4096, 8192),
         ("96_64", (96, 64), 4096, 4096)]


def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="one case name")
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda:0").manual_seed(7)
    for name, (n, k), block_bytes, count in CASES:
        if args.only and name != args.only:
            continue
        m, S = n - k, block_bytes // 4
        with fastecc_amd.Encoder(n, k, block_bytes) as enc:
            data = torch.randint(0, P, (count * k * S,), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32)
            parity = torch.empty(count * m * S, dtype=torch.int32, device="cuda:0")
            want = torch.empty_like(parity)

            def call(mode, dst=parity):
                enc.set_option("encode_pool_kernel", mode)
                enc.encode_pool(data, dst, count, stream=stream)

            call(3, want)
            torch.cuda.synchronize()
            chosen = {}
            for mode in (0, 1, 2):
                parity.fill_(-1)
                enc.profile(True)
                enc.profile_reset()
                call(mode)
                torch.cuda.synchronize()
                chosen[mode] = sorted(s for s in enc.profile_read() if s.startswith("encode_pool_")) or ["stripe_by_stripe"]
                enc.profile(False)
                assert torch.equal(parity, want), "%s mode %d differs from stripe by stripe" % (name, mode)
            for mode in (1, 2, 0):  # warm-up of every timed shape
                for _ in range(3):
                    call(mode)
            ts = {0: [], 1: [], 2: [], 3: []}
            for _ in range(args.repeats):
                for mode in (1, 2, 0):
                    ts[mode].append(one(lambda: call(mode)))
            for _ in range(3):
                ts[3].append(one(lambda: call(3)))
            moved = count * n * block_bytes
            rec = dict(case=name, code="(%d,%d)" % (n, k), block_bytes=block_bytes, stripes=count, pool_bytes=moved, repeats=args.repeats)
            for mode, label in ((1, "valu"), (2, "mfma"), (0, "auto"), (3, "stripe_by_stripe")):
                med = float(np.median(ts[mode]))
                rec[label + "_ms"] = round(med, 4)
                rec[label + "_ms_min"] = round(float(min(ts[mode])), 4)
                if mode != 3:
                    rec[label + "_gbs"] = round(moved / (med * 1e-3) / 1e9, 1)
                    rec[label + "_hbm_share"] = round(moved / (med * 1e-3) / 1e9 / (HBM_TBS * 1e3), 3)
                    rec[label + "_scopes"] = chosen[mode]
            rec["valu_over_mfma"] = round(rec["valu_ms"] / rec["mfma_ms"], 3)
            rec["stripe_by_stripe_over_auto"] = round(rec["stripe_by_stripe_ms"] / rec["auto_ms"], 1)
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del data, parity, want
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
