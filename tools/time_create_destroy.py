#!/usr/bin/env python3
"""Wall time of fastecc_create + fastecc_destroy at the headline code, (n,k) = (2^20, 2^19) x 4 KiB: the context's set-up and teardown with no
call in between (the twiddle tables are built at first use, so this is the plans, the per-block factors and the scratch word table going up and
every owner giving its memory back).  `--sharded G`: a sharded context of G column slabs on device 0 instead (G contexts for block_bytes / G, each
shard's streams and events, the fork event).  Median and range of `--runs` pairs after one untimed pair (code objects, runtime set-up).  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import fastecc_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2k", type=int, default=19)
    ap.add_argument("--block-bytes", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--sharded", type=int, default=0, metavar="G")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    k = 1 << args.log2k

    def pair():
        t0 = time.perf_counter()
        if args.sharded:
            fastecc_amd.ShardedEncoder(2 * k, k, args.block_bytes, [0] * args.sharded).close()
        else:
            fastecc_amd.Encoder(2 * k, k, args.block_bytes).close()
        return (time.perf_counter() - t0) * 1e3

    pair()
    torch.cuda.synchronize()
    ms = [pair() for _ in range(args.runs)]
    what = "fastecc_create_sharded (%d slabs on device 0)" % args.sharded if args.sharded else "fastecc_create"
    print(json.dumps({"what": "%s + fastecc_destroy, (2^%d, 2^%d) x %d B" % (what, args.log2k + 1, args.log2k, args.block_bytes), "label": args.label,
                      "runs": args.runs, "median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}))


if __name__ == "__main__":
    main()
