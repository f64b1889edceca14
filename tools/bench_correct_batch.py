#!/usr/bin/env python3
"""Time fastecc_correct_batch with many corrupted stripes: the grouped path ("correct_batch_mode" 1: one batched location pass, one
repair per lost-block pattern, one closing verify) against fastecc_correct stripe by stripe (mode 2, the code path before the
grouped one existed), in the same run, alternating.  HBM-resident pools:
  (20,16) x 4 KB x 32768 stripes, (14,10) x 64 KB x 4096, (256,128) x 4 KB x 4096
and per pool the cases
  a  the same data block wrong in every stripe            b  the same block wrong in 1 % of the stripes
  c  8 stripes with 8 different blocks    d  1 % of the stripes with a random block each (up to n patterns)
Every corrupted block has one word changed to another value below p.  Per call: ms between HIP events around the synchronous call
and the host's wall time (the host Berlekamp-Massey runs and the per-pattern prepares are part of the cost); per case and mode also
the number of patterns and the launches per profile scope, from a separate profiled call.  Every timed call is checked: exactly the
corrupted stripes get status 1 and the pool equals the clean one afterwards.  A call that takes more than --slow seconds is timed
once, else --repeats times (median).  On a library without the option every call is mode 2 (reported as such).
One JSON line per case and mode; --out FILE also appends them there (profiles/scrub_batch/bench_correct_batch.jsonl).
  python tools/bench_correct_batch.py [--repeats R] [--slow SECONDS] [--out FILE] [--only POOL] [--cases abcd]"""
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
SEED = 0x5C8B
WORD = 7  # the word of a corrupted block that changes

# name, (n, k), block bytes, stripes
POOLS = [("20_16", (20, 16), 4096, 32768),
         ("14_10", (14, 10), 65536, 4096),
         ("256_128", (256, 128), 4096, 4096)]


def corruption(case, n, k, count, rng):
    """(stripes, blocks): block blocks[i] of stripe stripes[i] is corrupted"""
    if case == "a":
        return np.arange(count), np.full(count, 3)
    some = np.sort(rng.choice(count, size=max(2, count // 100), replace=False))
    if case == "b":
        return some, np.full(len(some), 3)
    if case == "c":
        return np.sort(rng.choice(count, size=8, replace=False)), rng.choice(n, size=8, replace=False)
    return some, rng.integers(0, n, size=len(some))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--slow", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="one pool name")
    ap.add_argument("--cases", default="abcd")
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
    for name, (n, k), block_bytes, count in POOLS:
        if args.only and name != args.only:
            continue
        m, S = n - k, block_bytes // 4
        with fastecc_amd.Encoder(n, k, block_bytes) as enc:
            try:
                enc.set_option("correct_batch_mode", 0)
                modes = [1, 2]
            except fastecc_amd.FastEccError:
                modes = [2]  # a library from before the grouped path: its only code path
            data = torch.randint(0, P, (count * k * S,), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32)
            parity = torch.empty(count * m * S, dtype=torch.int32, device="cuda:0")
            for b in range(count):
                enc.encode(data.data_ptr() + b * k * S * 4, parity.data_ptr() + b * m * S * 4, stream=stream)
            torch.cuda.synchronize()
            assert enc.verify_batch(data, parity, count, seed=SEED, stream=stream).all(), "%s: clean pool reported inconsistent" % name
            rows_d, rows_p = data.view(count, k, S), parity.view(count, m, S)
            for case in args.cases:
                stripes, blocks = corruption(case, n, k, count, rng)
                want = np.zeros(count, np.uint8)
                want[stripes] = 1
                sd = torch.from_numpy(stripes[blocks < k]).to("cuda:0")
                jd = torch.from_numpy(blocks[blocks < k]).to("cuda:0")
                sp = torch.from_numpy(stripes[blocks >= k]).to("cuda:0")
                jp = torch.from_numpy(blocks[blocks >= k] - k).to("cuda:0")
                clean_d, clean_p = rows_d[sd, jd, WORD].clone(), rows_p[sp, jp, WORD].clone()

                def corrupt():
                    for rows, s_, j_, clean in ((rows_d, sd, jd, clean_d), (rows_p, sp, jp, clean_p)):
                        v = ((clean.to(torch.int64) & 0xFFFFFFFF) + 1) % P  # another value below p
                        rows[s_, j_, WORD] = torch.where(v >= 1 << 31, v - (1 << 32), v).to(torch.int32)
                    torch.cuda.synchronize()

                def restored():
                    return torch.equal(rows_d[sd, jd, WORD], clean_d) and torch.equal(rows_p[sp, jp, WORD], clean_p)

                def call(mode):
                    """one checked call on the freshly corrupted pool: (event ms, wall ms)"""
                    corrupt()
                    if len(modes) > 1:
                        enc.set_option("correct_batch_mode", mode)
                    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    a.record()
                    status = enc.correct_batch(data, parity, count, seed=SEED, stream=stream)
                    e.record()
                    e.synchronize()
                    wall = (time.perf_counter() - t0) * 1e3
                    assert np.array_equal(status, want) and restored(), (name, case, mode)
                    return a.elapsed_time(e), wall

                times = {mode: [call(mode)] for mode in modes}  # the first call of each: warm-up of its code, and its cost class
                reps = {mode: (1 if times[mode][0][1] > args.slow * 1e3 else args.repeats) for mode in modes}
                for mode in modes:
                    if reps[mode] > 1:
                        times[mode] = []  # (a call that is timed once keeps its first, cold, time: said in the record)
                for r in range(args.repeats):  # alternating
                    for mode in modes:
                        if reps[mode] > 1:
                            times[mode].append(call(mode))
                for mode in modes:
                    prof = {}
                    if reps[mode] > 1:  # (a profiled call of a slow case would record some ten scopes per stripe: left out)
                        corrupt()
                        if len(modes) > 1:
                            enc.set_option("correct_batch_mode", mode)
                        enc.profile(True)
                        enc.profile_reset()
                        enc.correct_batch(data, parity, count, seed=SEED, stream=stream)
                        prof = enc.profile_read(cap=128)
                        enc.profile(False)
                        assert restored()
                    ev, wall = np.array(times[mode]).T
                    emit(dict(pool=name, code="(%d,%d)" % (n, k), block_bytes=block_bytes, stripes=count, case=case, mode=mode,
                              option_known=len(modes) > 1, corrupted=int(len(stripes)), patterns=int(len(set(blocks.tolist()))),
                              calls=int(len(ev)), cold=bool(reps[mode] == 1), ms=round(float(np.median(ev)), 3), ms_min=round(float(ev.min()), 3),
                              wall_ms=round(float(np.median(wall)), 3), ms_per_corrupted=round(float(np.median(ev)) / len(stripes), 5),
                              launches={kk: v[1] for kk, v in sorted(prof.items())}, profile_ms={kk: round(v[0], 3) for kk, v in sorted(prof.items())}))
            del data, parity, rows_d, rows_p
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
