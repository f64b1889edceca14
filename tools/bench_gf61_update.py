#!/usr/bin/env python3
"""Time the small writes of the 64-bit field against a fresh encode, 64 KB blocks, HBM-resident stripes.
Shapes: (2^20, 2^19) with t changed blocks in {1, 4, 16, 32, 64} and (2^13, 2^12) with t in {1, 16}.  Per t: fastecc_gf61_update_parity and
fastecc_gf61_update (median ms of HIP events around each call; both alternate between two versions of the blocks, the same work every call, and
end on the stripe they started from), the GB/s of parity read + written (32 bytes per parity element, the pass count times for t > 16) with
its share of the 6.3 TB/s achievable HBM rate, and fastecc_encode of the same context in the same run.  After the timed calls a few element
columns of the parity are compared with a fresh encode of those columns of the data.  Each shape runs in a child process under its own time
limit, and a shape that fails ends the run.  One JSON line per case; --out FILE also appends them there.
  python tools/bench_gf61_update.py [--repeats R] [--out FILE] [--shapes big,small]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P = (1 << 61) - 1
HBM_TBS = 6.3
ROWS_PER_PASS = 16  # gf61_update.hip ROWS
ELEMS = 4096        # 64 KB blocks
SHAPES = {"big": (19, [1, 4, 16, 32, 64], 900), "small": (12, [1, 16], 300)}  # log2 k, the counts, the child's time limit in seconds


def timed(torch, fn, reps, warmup=4):
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


def run_shape(name, repeats, emit):
    import torch

    import fastecc_amd as fe
    logk, counts, _ = SHAPES[name]
    k, W = 1 << logk, 2 * ELEMS
    n, m = 2 * k, k
    repeats += repeats % 2  # an even number of alternating calls: the stripe ends where it started
    g = torch.Generator(device="cuda:0").manual_seed(11)
    data = torch.randint(0, P, (k * W,), dtype=torch.int64, device="cuda:0", generator=g)
    parity = torch.empty(m * W, dtype=torch.int64, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(5)
    base = {"code": "(%d,%d)" % (n, k), "block_bytes": 16 * ELEMS, "field": "p61"}
    check_elems = [0, 1, 63, 64, ELEMS - 1]
    cols = torch.tensor([2 * c + h for c in check_elems for h in (0, 1)], device="cuda:0", dtype=torch.int64)
    with fe.Encoder(n, k, 16 * ELEMS, field=fe.FIELD_GF_P61_SQUARED) as enc, \
            fe.Encoder(n, k, 16 * len(check_elems), field=fe.FIELD_GF_P61_SQUARED) as narrow:

        def check(what):
            """the element columns check_elems of the parity against a fresh encode of those columns of the data"""
            want = torch.empty(m * len(cols), dtype=torch.int64, device="cuda:0")
            narrow.encode(data.view(k, W)[:, cols].contiguous().view(-1), want, stream=stream)
            torch.cuda.synchronize()
            assert torch.equal(parity.view(m, W)[:, cols].contiguous().view(-1), want), what

        ms, best = timed(torch, lambda: enc.encode(data, parity, stream=stream), repeats)
        emit(dict(base, case="encode", ms=round(ms, 4), ms_min=round(best, 4)))
        check("encode")
        for t in counts:
            blocks = [int(b) for b in rng.choice(k, size=t, replace=False)]
            idx = torch.tensor(blocks, device="cuda:0", dtype=torch.int64)
            rows = data.view(k, W)
            new = torch.randint(0, P, (t * W,), dtype=torch.int64, device="cuda:0", generator=g)
            old = rows[idx].reshape(-1).clone()
            passes = (t + ROWS_PER_PASS - 1) // ROWS_PER_PASS
            moved = passes * m * ELEMS * 32
            state = {"flip": False}

            def upd_parity():
                a, b = (new, old) if state["flip"] else (old, new)
                enc.gf61_update_parity(parity, blocks, b, old=a, stream=stream)
                state["flip"] = not state["flip"]

            def upd():
                enc.gf61_update(data, parity, blocks, old if state["flip"] else new, stream=stream)
                state["flip"] = not state["flip"]

            ms_p, best_p = timed(torch, upd_parity, repeats)
            assert not state["flip"]
            check("gf61_update_parity t=%d" % t)
            ms_u, best_u = timed(torch, upd, repeats)
            assert not state["flip"]
            check("gf61_update t=%d" % t)
            # ... and once in the other state: the new blocks in the stripe
            upd()
            torch.cuda.synchronize()
            assert torch.equal(rows[idx].reshape(-1), new)
            check("gf61_update t=%d, new blocks" % t)
            upd()
            for case, v, b in (("gf61_update_parity", ms_p, best_p), ("gf61_update", ms_u, best_u)):
                gbs = moved / (v * 1e-3) / 1e9
                emit(dict(base, case=case, t=t, passes=passes, ms=round(v, 4), ms_min=round(b, 4), parity_gbs=round(gbs, 1),
                          hbm_share=round(gbs / (HBM_TBS * 1e3), 3), encode_ms=round(ms, 4), checked_elems=check_elems))
            torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="big,small")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        run_shape(args.child, args.repeats, lambda rec: print(json.dumps(rec), flush=True))
        return 0
    out = open(args.out, "a") if args.out else None
    for name in args.shapes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--repeats", str(args.repeats)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=SHAPES[name][2])
        except subprocess.TimeoutExpired:
            print("shape %s: time limit of %d s" % (name, SHAPES[name][2]), file=sys.stderr)
            return 124
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:  # nothing more is started on the GPU after a failure
            print("shape %s: exit status %d" % (name, r.returncode), file=sys.stderr)
            return r.returncode if r.returncode > 0 else 1
        if out:
            out.write(r.stdout)
            out.flush()
    if out:
        out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
