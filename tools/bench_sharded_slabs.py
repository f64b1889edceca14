#!/usr/bin/env python3
"""Encode time of a sharded context whose G column slabs all live on device 0 (the form tests/test_gpu_sharded.py runs): the headline stripe,
(n,k) = (2^20, 2^19) x 4 KiB, from slabs to a gathered parity stripe (fastecc_encode_sharded) and as a full stripe in device memory
(fastecc_encode), in the context's default gather mode with two sub-slabs.  This times the host plumbing of csrc/sharded.hip around unchanged
kernels on one GPU; it says nothing about links.  One JSON line per G."""
import argparse
import json
import os
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
    ap.add_argument("--slabs", type=int, nargs="+", default=[2, 8], metavar="G")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    k, S = 1 << args.log2k, args.block_bytes // 4
    stripe = torch.randint(0, 0xFFF00001, (k * S,), dtype=torch.int64, device="cuda:0").to(torch.int32)
    parity = torch.empty_like(stripe)
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) / args.steps * 1e3, 4)

    for G in args.slabs:
        w = S // G
        slabs = [stripe.view(k, S)[:, g * w:(g + 1) * w].contiguous().reshape(-1) for g in range(G)]
        with fastecc_amd.ShardedEncoder(2 * k, k, args.block_bytes, [0] * G) as enc:
            from_slabs = timed(lambda: enc.encode_sharded(slabs, None, parity, stream=stream))
            full = timed(lambda: enc.encode(stripe, parity, stream=stream))
            print(json.dumps({"what": "sharded encode, %d slabs on device 0, (2^%d, 2^%d) x %d B" % (G, args.log2k + 1, args.log2k, args.block_bytes),
                              "label": args.label, "steps": args.steps, "slabs_to_stripe_ms": from_slabs, "full_stripe_ms": full, "plan": enc.plan()}), flush=True)
        del slabs


if __name__ == "__main__":
    main()
