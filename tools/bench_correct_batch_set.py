#!/usr/bin/env python3
"""Time fastecc_correct_batch_set on degraded pools with rotated placement: the grouped path ("correct_batch_mode" 1: one batched location pass
under the stripes' own patterns, one repair launch per size class through a pattern set private to the call, one closing verify; DESIGN.md
section 27) against the stripes one after the other (mode 2, the only code path before), in the same run, alternating.  HBM-resident pools
  (20,16) x 4 KB x 32768 stripes, (256,128) x 4 KB x 4096
with one device down — pattern_of[b] = b mod n, pattern q names block q absent — and per pool the cases
  a  a second device lying: block (b + 7) mod n of every stripe b is wrong, n distinct lost sets
  d  1 % of the stripes with one random wrong block          c  8 stripes with one random wrong block
Every corrupted block has one word changed to another value below p, and the absent block of a corrupted stripe is filled with garbage
first.  Per call: ms between HIP events around the synchronous call and the host's wall time (the host Berlekamp-Massey runs and the table
builds of the private set are part of the cost); per case and mode also the distinct lost sets and the launches and milliseconds per
profile scope, from a separate profiled call.  Every timed call is checked: exactly the corrupted stripes get status 1 and the pool equals
the clean one afterwards.  A call that takes more than --slow seconds is timed once and marked cold, else --repeats times (median).
--label parent: the library of the tree this script runs in has no grouped path; only mode 2 is timed, the records carry the label.
One JSON line per case and mode; --out FILE also appends them there (profiles/scrub_set_grouped/bench_correct_batch_set.jsonl).
With FASTECC_TRACE_PREPARE set in the environment the library prints where each call's wall time goes, host work included ("[fastecc
correct_batch_set]" lines on stderr); use --modes 1 then, mode 2 prints several lines per stripe.
  python tools/bench_correct_batch_set.py [--repeats R] [--slow SECONDS] [--out FILE] [--only POOL] [--cases adc] [--label NAME] [--modes 12]"""
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
         ("256_128", (256, 128), 4096, 4096)]


def corruption(case, n, count, rng):
    """(stripes, blocks): block blocks[i] of stripe stripes[i] is corrupted; never the stripe's absent block stripes[i] mod n"""
    if case == "a":
        stripes = np.arange(count)
        return stripes, (stripes + 7) % n
    stripes = np.sort(rng.choice(count, size=8 if case == "c" else max(2, count // 100), replace=False))
    return stripes, (stripes + 1 + rng.integers(0, n - 1, size=len(stripes))) % n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--slow", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="one pool name")
    ap.add_argument("--cases", default="adc")
    ap.add_argument("--label", default="head")
    ap.add_argument("--modes", default="12", help="the modes to time (--label parent: 2 alone)")
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
    modes = [2] if args.label == "parent" else [int(x) for x in args.modes]
    for name, (n, k), block_bytes, count in POOLS:
        if args.only and name != args.only:
            continue
        m, S = n - k, block_bytes // 4
        with fastecc_amd.Encoder(n, k, block_bytes) as enc:
            data = torch.randint(0, P, (count * k * S,), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32)
            parity = torch.empty(count * m * S, dtype=torch.int32, device="cuda:0")
            enc.encode_pool(data, parity, count, stream=stream)
            torch.cuda.synchronize()
            dp, pp = np.ones((n, k), np.uint8), np.ones((n, m), np.uint8)
            for q in range(n):
                (dp[q] if q < k else pp[q])[q if q < k else q - k] = 0
            enc.scrub_erasures_set(dp, pp)
            po = (np.arange(count) % n).astype(np.uint32)
            assert enc.verify_batch_set(data, parity, count, po, seed=SEED, stream=stream).all(), "%s: clean pool reported inconsistent" % name
            rows_d, rows_p = data.view(count, k, S), parity.view(count, m, S)
            for case in args.cases:
                stripes, blocks = corruption(case, n, count, rng)
                absent = stripes % n
                assert not (blocks == absent).any()
                want = np.zeros(count, np.uint8)
                want[stripes] = 1

                def split(st, bl):
                    """the (stripe, row) index tensors of the blocks in the data pool and in the parity pool"""
                    return ((torch.from_numpy(st[bl < k]).to("cuda:0"), torch.from_numpy(bl[bl < k]).to("cuda:0")),
                            (torch.from_numpy(st[bl >= k]).to("cuda:0"), torch.from_numpy(bl[bl >= k] - k).to("cuda:0")))
                (sd, jd), (sp, jp) = split(stripes, blocks)
                (ad, aj), (ap_, apj) = split(stripes, absent)
                clean_d, clean_p = rows_d[sd, jd, WORD].clone(), rows_p[sp, jp, WORD].clone()
                clean_ad, clean_ap = rows_d[ad, aj].clone(), rows_p[ap_, apj].clone()

                def corrupt():
                    for rows, s_, j_, clean in ((rows_d, sd, jd, clean_d), (rows_p, sp, jp, clean_p)):
                        v = ((clean.to(torch.int64) & 0xFFFFFFFF) + 1) % P  # another value below p
                        rows[s_, j_, WORD] = torch.where(v >= 1 << 31, v - (1 << 32), v).to(torch.int32)
                    rows_d[ad, aj] = -1  # the absent block of a corrupted stripe: words >= p, never read
                    rows_p[ap_, apj] = -1
                    torch.cuda.synchronize()

                def restored():
                    return (torch.equal(rows_d[sd, jd, WORD], clean_d) and torch.equal(rows_p[sp, jp, WORD], clean_p) and
                            torch.equal(rows_d[ad, aj], clean_ad) and torch.equal(rows_p[ap_, apj], clean_ap))

                def call(mode):
                    """one checked call on the freshly corrupted pool: (event ms, wall ms)"""
                    corrupt()
                    enc.set_option("correct_batch_mode", mode)
                    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    a.record()
                    status = enc.correct_batch_set(data, parity, count, po, seed=SEED, stream=stream)
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
                        enc.set_option("correct_batch_mode", mode)
                        enc.profile(True)
                        enc.profile_reset()
                        t0 = time.perf_counter()
                        enc.correct_batch_set(data, parity, count, po, seed=SEED, stream=stream)
                        prof_wall = (time.perf_counter() - t0) * 1e3
                        prof = enc.profile_read(cap=128)
                        enc.profile(False)
                        assert restored()
                    ev, wall = np.array(times[mode]).T
                    lost_sets = len(set(zip(absent.tolist(), blocks.tolist())))
                    emit(dict(label=args.label, pool=name, code="(%d,%d)" % (n, k), block_bytes=block_bytes, stripes=count, case=case, mode=mode,
                              corrupted=int(len(stripes)), lost_sets=int(lost_sets), calls=int(len(ev)), cold=bool(reps[mode] == 1),
                              ms=round(float(np.median(ev)), 3), ms_min=round(float(ev.min()), 3), ms_max=round(float(ev.max()), 3),
                              wall_ms=round(float(np.median(wall)), 3), ms_per_corrupted=round(float(np.median(ev)) / len(stripes), 5),
                              launches={kk: v[1] for kk, v in sorted(prof.items())}, profile_ms={kk: round(v[0], 3) for kk, v in sorted(prof.items())},
                              profiled_call_wall_ms=round(prof_wall, 3) if prof else None))
            del data, parity, rows_d, rows_p
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
