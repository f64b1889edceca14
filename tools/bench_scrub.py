#!/usr/bin/env python3
"""Time error detection and location at the headline code: (n,k) = (2^20, 2^19), 4 KB blocks, HBM-resident codeword.
Cases: fastecc_verify on a clean codeword (with the fingerprint kernel's own time and GB/s over the 4 GiB it reads, from the
library's per-kernel profile), fastecc_locate_errors and fastecc_correct with 1 / 16 / 64 corrupted blocks, and the alternative
without this feature: re-encode the data and compare the parity (torch.equal).  Wall time per call around a synchronised call
(every scrub call waits for its stream), HIP events for the re-encode; warm-up first, median of the repeats.  One JSON line per case.
  python tools/bench_scrub.py [log2k] [repeats]"""
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


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts))


def main():
    log2k = int(sys.argv[1]) if len(sys.argv) > 1 else 19
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    k, S = 1 << log2k, 1024
    g = torch.Generator(device="cuda:0").manual_seed(7)
    data = torch.randint(0, P, (k * S,), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32)
    parity = torch.empty_like(data)
    stream = torch.cuda.current_stream().cuda_stream
    stripe_bytes = 2 * k * S * 4
    base = {"code": "(2^%d,2^%d)" % (log2k + 1, log2k), "block_bytes": 4 * S}
    with fastecc_amd.Encoder(2 * k, k, 4 * S) as enc:
        enc.encode(data, parity, stream=stream)
        torch.cuda.synchronize()
        assert enc.verify(data, parity, stream=stream)
        ms, best = timed(lambda: enc.verify(data, parity, seed=1, stream=stream), reps)
        enc.profile(True)
        enc.profile_reset()
        enc.verify(data, parity, seed=1, stream=stream)
        prof = enc.profile_read()
        enc.profile(False)
        fp_ms = prof.get("fingerprint", (0.0, 1, 0))[0]
        kernels = {name: round(v[0], 4) for name, v in prof.items()}
        print(json.dumps(dict(base, case="verify_clean", ms=round(ms, 4), ms_min=round(best, 4), fingerprint_ms=round(fp_ms, 4),
                              fingerprint_gbs=round(stripe_bytes / fp_ms / 1e6, 1) if fp_ms else None, kernels_ms=kernels)), flush=True)

        # the alternative today: re-encode the data, compare the parity
        again = torch.empty_like(parity)
        ms, best = timed(lambda: (enc.encode(data, again, stream=stream), torch.equal(again, parity)), reps)
        print(json.dumps(dict(base, case="reencode_compare", ms=round(ms, 4), ms_min=round(best, 4))), flush=True)
        del again

        rng = np.random.default_rng(3)
        for t in (1, 16, 64):
            blocks = sorted(int(b) for b in rng.choice(2 * k, size=t, replace=False))
            saved = []
            for b in blocks:
                buf, row = (data, b) if b < k else (parity, b - k)
                saved.append(buf[row * S:(row + 1) * S].clone())
                buf[row * S + 5] = (int(buf[row * S + 5]) + 1) % (1 << 31)
            torch.cuda.synchronize()
            got = enc.locate_errors(data, parity, seed=2, stream=stream)
            assert got == blocks, (got[:8], blocks[:8])
            ms, best = timed(lambda: enc.locate_errors(data, parity, seed=2, stream=stream), reps)
            print(json.dumps(dict(base, case="locate", corrupted=t, ms=round(ms, 4), ms_min=round(best, 4))), flush=True)

            def corrupt_and_correct():
                for b in blocks:
                    buf, row = (data, b) if b < k else (parity, b - k)
                    buf[row * S + 5] += 1
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                assert enc.correct(data, parity, seed=3, stream=stream) == blocks
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3
            corrupt_and_correct()
            times = [corrupt_and_correct() for _ in range(reps)]
            print(json.dumps(dict(base, case="correct", corrupted=t, ms=round(float(np.median(times)), 4), ms_min=round(min(times), 4))), flush=True)
            for b, want in zip(blocks, saved):
                buf, row = (data, b) if b < k else (parity, b - k)
                assert torch.equal(buf[row * S:(row + 1) * S], want)


if __name__ == "__main__":
    main()
