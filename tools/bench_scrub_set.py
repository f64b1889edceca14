#!/usr/bin/env python3
"""Time fastecc_verify_batch_set on degraded pools with rotated placement, HBM-resident pools (128 MiB and more).
Pools: (20,16) x 4 KB x 32768 stripes and (256,128) x 4 KB x 4096 stripes; one device down: pattern q lacks codeword block q, pattern_of[b] = b mod n,
and every absent block holds garbage (0xFFFFFFFF words).  For each pool, in the same process:
  (a) set  : fastecc_verify_batch_set of the whole pool;
  (c) same : fastecc_verify_batch of the same pool under ONE fastecc_scrub_erasures pattern, block 0 absent in every stripe (block 0 of every stripe
             holds garbage for this measurement): the same bytes read — the yardstick, whose code is the parent commit's;
  (b) loop : the only public route before the set calls, fastecc_scrub_erasures + fastecc_verify stripe by stripe, over the first 256 stripes and
             scaled to the whole count (labelled scaled);
and the set-up time of fastecc_scrub_erasures_set for the pool's n patterns (host clock around the synchronous call, median of 5).
Median and minimum ms of --repeats HIP-event-timed calls; the kernel times are the library's own profile scopes, averaged over 5 profiled calls.
Every timed call's answer is checked once.  One JSON line per pool; --out FILE also appends them.
  python tools/bench_scrub_set.py [--repeats R] [--out FILE] [--only CASE] [--set-only]"""
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
HBM_TBS = 6.3
LOOP_STRIPES = 256
SEED = 0x5C2B
PROFILED = 5

# name, (n, k), block bytes, stripes
CASES = [("20_16_rot", (20, 16), 4096, 32768),
         ("256_128_rot", (256, 128), 4096, 4096)]


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


def profiled(enc, fn):
    """{scope: ms per call} of the library's profile over PROFILED calls"""
    enc.profile(True)
    enc.profile_reset()
    for _ in range(PROFILED):
        fn()
    prof = enc.profile_read()
    enc.profile(False)
    return {name: round(v[0] / PROFILED, 4) for name, v in prof.items()}, {name: v[2] // PROFILED for name, v in prof.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="one case name")
    ap.add_argument("--set-only", action="store_true", help="skip the per-stripe loop")
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
            rows_d, rows_p = data.view(count, k, S), parity.view(count, m, S)
            block0 = rows_d[:, 0].clone()

            # rotated placement, one device down: pattern q lacks codeword block q, stripe b has pattern b mod n
            dp, pp = np.ones((n, k), np.uint8), np.ones((n, m), np.uint8)
            for q in range(n):
                if q < k:
                    dp[q, q] = 0
                else:
                    pp[q, q - k] = 0
            pattern_of = (np.arange(count, dtype=np.uint64) % n).astype(np.uint32)
            setup = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                enc.scrub_erasures_set(dp, pp)
                setup.append((time.perf_counter() - t0) * 1e3)
            stripes = torch.arange(count, device="cuda:0")
            lost = stripes % n
            in_d, in_p = lost < k, lost >= k
            rows_d[stripes[in_d], lost[in_d]] = -1
            rows_p[stripes[in_p], lost[in_p] - k] = -1
            torch.cuda.synchronize()

            def set_call():
                return enc.verify_batch_set(data, parity, count, pattern_of, seed=SEED, stream=stream)
            assert set_call().all(), "%s: degraded pool reported inconsistent" % name
            assert not enc.verify_batch(data, parity, count, seed=SEED, stream=stream).any(), "%s: the garbage went unnoticed" % name
            set_ms = timed(set_call, args.repeats)
            set_prof, set_bytes = profiled(enc, set_call)
            rec = dict(case=name, code="(%d,%d)" % (n, k), block_bytes=block_bytes, stripes=count, patterns=n,
                       bytes_read=count * (n - 1) * block_bytes,
                       set_ms=round(set_ms[0], 4), set_ms_min=round(set_ms[1], 4), set_profile_ms=set_prof,
                       fingerprint_set_bytes=set_bytes.get("fingerprint_set"),
                       scrub_erasures_set_ms=round(float(np.median(setup)), 3), scrub_erasures_set_ms_first=round(setup[0], 3))

            if not args.set_only:
                # (b) the per-stripe route over the first LOOP_STRIPES stripes: a pattern and a verify each
                def loop():
                    for b in range(LOOP_STRIPES):
                        q = b % n
                        enc.scrub_erasures(dp[q], pp[q])
                        assert enc.verify(data.data_ptr() + b * k * S * 4, parity.data_ptr() + b * m * S * 4, seed=SEED, stream=stream)
                loop_ms, _ = timed(loop, max(5, args.repeats // 4))
                rec.update(loop_ms_scaled=round(loop_ms * count / LOOP_STRIPES, 3), loop_stripes=LOOP_STRIPES,
                           ratio_loop_scaled_over_set=round(loop_ms * count / LOOP_STRIPES / set_ms[0], 1))

            # (c) the same pool, one pattern: block 0 absent (and garbage) in every stripe, every other block whole
            rows_d[stripes[in_d], lost[in_d]] = 0
            rows_p[stripes[in_p], lost[in_p] - k] = 0
            one_d, one_p = np.ones(k, np.uint8), np.ones(m, np.uint8)
            one_d[0] = 0
            enc.decode_prepare_set(dp, pp)
            enc.repair_batch_set(data, parity, count, pattern_of, stream=stream)
            rows_d[:, 0] = -1
            torch.cuda.synchronize()
            enc.scrub_erasures(one_d, one_p)

            def same_call():
                return enc.verify_batch(data, parity, count, seed=SEED, stream=stream)
            assert same_call().all(), "%s: the one-pattern pool reported inconsistent" % name
            same_ms = timed(same_call, args.repeats)
            same_prof, _ = profiled(enc, same_call)
            enc.scrub_erasures()
            rows_d[:, 0] = block0
            torch.cuda.synchronize()
            assert enc.verify_batch(data, parity, count, seed=SEED, stream=stream).all(), "%s: the pool was not restored" % name

            gbs = rec["bytes_read"] / (set_ms[0] * 1e-3) / 1e9
            rec.update(same_pattern_batch_ms=round(same_ms[0], 4), same_pattern_batch_ms_min=round(same_ms[1], 4), same_profile_ms=same_prof,
                       ratio_call_set_over_same=round(set_ms[0] / same_ms[0], 3),
                       ratio_kernel_set_over_same=round(set_prof["fingerprint_set"] / same_prof["fingerprint_batch"], 3),
                       set_gbs=round(gbs, 1), set_hbm_share=round(gbs / (HBM_TBS * 1e3), 3))
            emit(rec)
            del data, parity, rows_d, rows_p, block0
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
