#!/usr/bin/env python3
"""Time the window forms of the pool writes (fastecc_update_batch_window on a whole pool, fastecc_update_batch_set_window on the same pool rotated with
one device down) against the whole-block call on the SAME write list in the same run.  Case: (20,16) x 4 KB x 32768 stripes, placement (i + b) mod n
with device 0 down for the degraded pool (stripe b loses codeword block (-b) mod n: n patterns), one uniformly random write per stripe.  Windows
(col0, width) in words: (0,128), (0,256), (0,512), (0,1024), (512,128) and (1,127) — the last one runs one word per lane.  Both pools start all zero
(pools of codewords); the degraded one then gets garbage in every absent block.  Calls alternate between two sets of new rows, so every call changes
every word it names.  Per window and pool: median ms of --repeats calls over HIP events (an interval holds the call's host work as well: the stream is
idle when a call starts), the host's median time inside the call, the device's time by profile scope (fastecc_profile_read, mean of 5 calls), and the
achieved bytes/s of the window scopes against the traffic model of DESIGN.md section 36 — per stripe with T writes and M present parity blocks
(2 T + 2 M) * 4 * width bytes in update_window, 8 * width per stored row in update_window_scatter.  After the timed calls of each window a few touched
stripes are checked against the oracle, every column of every present block, and absent blocks against what they held.  One JSON line per window and
pool, appended to --out (default profiles/update_window/bench_update_window.jsonl).
  python tools/bench_update_window.py [--repeats R] [--out FILE] [--stripes N]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import fastecc_amd  # noqa: E402
from oracle import Oracle  # noqa: E402
from pool_model import Codec  # noqa: E402

P = 0xFFF00001
DEFAULT_OUT = os.path.join(ROOT, "profiles", "update_window", "bench_update_window.jsonl")
WINDOWS = [(0, 128), (0, 256), (0, 512), (0, 1024), (512, 128), (1, 127)]


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
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--stripes", type=int, default=32768)
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "a")
    oracle = Oracle()
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda:0").manual_seed(7)
    rng = np.random.default_rng(3)
    (n, k), block_bytes, count = (20, 16), 4096, args.stripes
    m, S = n - k, block_bytes // 4
    codec = Codec(oracle, n, k)
    L = fastecc_amd.lib()
    with fastecc_amd.Encoder(n, k, block_bytes) as enc:
        dp, pp = np.ones((n, k), np.uint8), np.ones((n, m), np.uint8)
        for u in range(n):  # pattern u loses codeword block u
            (dp if u < k else pp)[u, u if u < k else u - k] = 0
        enc.decode_prepare_set(dp, pp)
        pattern_of = np.array([(-b) % n for b in range(count)], dtype=np.uint32)
        po = pattern_of.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        blocks = rng.integers(0, k, size=count)
        writes_arr = (ctypes.c_uint64 * count)(*[b * k + int(i) for b, i in enumerate(blocks)])
        absent = int(np.count_nonzero(blocks == pattern_of))
        present_parity = int(np.count_nonzero(pattern_of < k)) * m + int(np.count_nonzero(pattern_of >= k)) * (m - 1)
        news = [torch.randint(0, P, (count * S,), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32) for _ in range(2)]
        junk = torch.randint(0, 1 << 31, (count, S), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32) | -0x100000  # words >= p
        hit = np.flatnonzero(blocks == pattern_of)
        watched = sorted({0, count // 2, count - 1} | ({int(hit[0])} if len(hit) else set()))
        for kind in ("whole", "degraded"):
            data = torch.zeros(count * k * S, dtype=torch.int32, device="cuda:0")
            parity = torch.zeros(count * m * S, dtype=torch.int32, device="cuda:0")
            if kind == "degraded":
                lost = torch.from_numpy(pattern_of.astype(np.int64)).to("cuda:0")
                stripe = torch.arange(count, device="cuda:0")
                dsel, psel = lost < k, lost >= k
                data.view(count, k, S)[stripe[dsel], lost[dsel]] = junk[dsel]
                parity.view(count, m, S)[stripe[psel], lost[psel] - k] = junk[psel]
            truth = {b: np.zeros((k, S), np.uint32) for b in watched}  # the data of the watched stripes, absent blocks as decode would rebuild them
            turn = [0]

            def call(window):
                """the window call (window = None: the whole-block call) of this pool's form on the list"""
                turn[0] ^= 1
                rows = news[turn[0]].data_ptr()
                if kind == "whole":
                    code = (L.fastecc_update_batch(enc._h, data.data_ptr(), parity.data_ptr(), count, writes_arr, count, rows, stream or None) if window is None else
                            L.fastecc_update_batch_window(enc._h, data.data_ptr(), parity.data_ptr(), count, writes_arr, count, window[0], window[1], rows,
                                                          stream or None))
                else:
                    code = (L.fastecc_update_batch_set(enc._h, data.data_ptr(), parity.data_ptr(), count, po, writes_arr, count, rows, stream or None)
                            if window is None else
                            L.fastecc_update_batch_set_window(enc._h, data.data_ptr(), parity.data_ptr(), count, po, writes_arr, count, window[0], window[1],
                                                              rows, stream or None))
                assert code == 0, code

            def check(window, what):
                """the watched stripes against the oracle after a call with `window`: rows of `width` words, compact, from the last set of new rows"""
                torch.cuda.synchronize()
                c0, w = window or (0, S)
                rows = news[turn[0]][:count * w].view(count, w)
                for b in watched:
                    truth[b][blocks[b], c0:c0 + w] = rows[b].cpu().numpy().view(np.uint32)
                    want = np.concatenate([truth[b], codec.parity(truth[b])])
                    got = np.concatenate([data.view(count, k, S)[b].cpu().numpy(), parity.view(count, m, S)[b].cpu().numpy()]).view(np.uint32)
                    u = int(pattern_of[b]) if kind == "degraded" else -1
                    present = [j for j in range(n) if j != u]
                    assert np.array_equal(got[present], want[present]), "%s %s %r: present blocks of stripe %d" % (kind, what, window, b)
                    if u >= 0:
                        assert np.array_equal(got[u], junk[b].cpu().numpy().view(np.uint32)), "%s %s: the absent block of stripe %d was written" % (kind, what, b)

            def split(fn):
                """where a call's time goes: the host's share (the call returns; nothing waits for the device) and the device's by profile scope"""
                host = []
                for _ in range(args.repeats):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    host.append((time.perf_counter() - t0) * 1e3)
                torch.cuda.synchronize()
                enc.profile(True)
                enc.profile_reset()
                for _ in range(5):
                    fn()
                torch.cuda.synchronize()
                scopes = {name: round(ms / 5, 4) for name, (ms, _, _) in enc.profile_read().items()}
                enc.profile(False)
                return round(float(np.median(host)), 4), scopes

            for window in WINDOWS:
                c0, w = window
                call(window)
                check(window, "first call")
                win_ms, win_min = timed(lambda: call(window), args.repeats)
                check(window, "timed calls")
                blk_ms, blk_min = timed(lambda: call(None), args.repeats)
                check(None, "whole-block calls")
                win_host, win_scopes = split(lambda: call(window))
                check(window, "profiled calls")
                blk_host, blk_scopes = split(lambda: call(None))
                check(None, "profiled whole-block calls")
                parity_blocks = count * m if kind == "whole" else present_parity
                stored = count if kind == "whole" else count - absent
                model = {"update_window": (2 * count + 2 * parity_blocks) * 4 * w, "update_window_scatter": stored * 8 * w}
                gbs = {s: round(model[s] / (win_scopes[s] * 1e-3) / 1e9, 1) for s in model if win_scopes.get(s)}
                whole_scope = "update_batch" if kind == "whole" else "update_set"
                rec = dict(case="20_16_" + kind, code="(%d,%d)" % (n, k), block_bytes=block_bytes, stripes=count, writes=count, col0_words=c0, width_words=w,
                           writes_on_absent_blocks=absent if kind == "degraded" else 0, window_ms=round(win_ms, 4), window_ms_min=round(win_min, 4),
                           whole_block_ms=round(blk_ms, 4), whole_block_ms_min=round(blk_min, 4), ratio=round(win_ms / blk_ms, 3), window_host_ms=win_host,
                           whole_block_host_ms=blk_host, window_device_ms_by_scope=win_scopes, whole_block_device_ms_by_scope=blk_scopes,
                           model_bytes_by_scope=model, achieved_GBps_by_scope=gbs,
                           device_ratio_parity_kernel=round(win_scopes.get("update_window", 0) / blk_scopes[whole_scope], 3) if blk_scopes.get(whole_scope) else None)
                line = json.dumps(rec)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()
            del data, parity
            torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
