#!/usr/bin/env python3
"""Time the degraded pool writes from a write list in device memory (fastecc_update_batch_set_device) against the host-list call on the same pool,
pattern set and list (fastecc_update_batch_set, or fastecc_update_batch_set_window for a window), and against fastecc_update_batch_device on the
same pool kept whole.  Cases (DESIGN.md section 33's two pools): rotated placement with device 0 down, one uniformly random write per stripe,
max_per_stripe = 1, max_absent = n_writes: (20,16) x 4 KB x 32768 stripes and (256,128) x 4 KB x 4096 stripes, each with the whole block and with
the 512-byte window (0, 128).
The pools start as codewords (all zero) with every absent block overwritten by words >= p; calls alternate between two sets of new rows.  The variants
— the device-list call, this library's host-list call, the parent's host-list call (--parent-lib PATH: a libfastecc_hip.so built from the parent
commit, through a context and a pattern set of its own) and the whole pool's device-list call — alternate over --rounds rounds; per variant and
round: the time for the call to return on the host (the stream idle when it starts) and the HIP-event time of the call, medians of --repeats
calls, and the device's time by profile scope (fastecc_profile_read, mean of 5 calls).  The record holds the median over the rounds and each
round's figures, so that the spread of the rounds stands beside every comparison.  Before anything is timed, and after, three stripes of the pool
written through the device list are compared word for word with the pool written through this library's host list.  One JSON line per case,
appended to --out (default profiles/update_set_device/bench_update_set_device.jsonl).
  python tools/bench_update_set_device.py [--repeats R] [--rounds N] [--out FILE] [--parent-lib PATH]"""
import argparse
import ctypes
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
DEFAULT_OUT = os.path.join(ROOT, "profiles", "update_set_device", "bench_update_set_device.jsonl")
# (name, n, k, stripes, window)
CASES = [("20_16_whole_block", 20, 16, 32768, (0, 1024)), ("20_16_window_512B", 20, 16, 32768, (0, 128)),
         ("256_128_whole_block", 256, 128, 4096, (0, 1024)), ("256_128_window_512B", 256, 128, 4096, (0, 128))]
vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
u8p, u32p, u64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(u32), ctypes.POINTER(u64)


def parent_library(path):
    """the parent commit's library with the few entry points this tool calls"""
    L = ctypes.CDLL(path)
    L.fastecc_create.argtypes, L.fastecc_create.restype = [ctypes.POINTER(vp), u64, u64, u64, i32, i32], i32
    L.fastecc_destroy.argtypes, L.fastecc_destroy.restype = [vp], None
    L.fastecc_decode_prepare_set.argtypes, L.fastecc_decode_prepare_set.restype = [vp, u8p, u8p, u64], i32
    L.fastecc_update_batch_set.argtypes, L.fastecc_update_batch_set.restype = [vp, vp, vp, u64, u32p, u64p, u64, vp, vp], i32
    L.fastecc_update_batch_set_window.argtypes, L.fastecc_update_batch_set_window.restype = [vp, vp, vp, u64, u32p, u64p, u64, u64, u64, vp, vp], i32
    L.fastecc_profile_enable.argtypes, L.fastecc_profile_enable.restype = [vp, i32], i32
    L.fastecc_profile_reset.argtypes, L.fastecc_profile_reset.restype = [vp], i32
    L.fastecc_profile_read_bytes.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_double), u64p, u64p, i32]
    L.fastecc_profile_read_bytes.restype = i32
    return L


def scopes_of(L, h, fn, calls=5):
    assert L.fastecc_profile_enable(h, 1) == 0 and L.fastecc_profile_reset(h) == 0
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    cap = 64
    names, ms, cnt, nbytes = (ctypes.c_char_p * cap)(), (ctypes.c_double * cap)(), (u64 * cap)(), (u64 * cap)()
    n = L.fastecc_profile_read_bytes(h, names, ms, cnt, nbytes, cap)
    assert n >= 0 and L.fastecc_profile_enable(h, 0) == 0
    return {names[i].decode(): round(ms[i] / calls, 4) for i in range(n)}


def measure(L, h, fn, reps):
    """(host ms for the call to return, HIP-event ms of the call, device ms by profile scope): medians of reps"""
    for _ in range(3):
        fn()
    host, dev = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        host.append((time.perf_counter() - t0) * 1e3)
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        dev.append(a.elapsed_time(b))
    return round(float(np.median(host)), 4), round(float(np.median(dev)), 4), scopes_of(L, h, fn)


def summary(rounds):
    """the median over the rounds of (returns, event, scopes), beside the rounds themselves"""
    scopes = sorted({s for r in rounds for s in r[2]})
    return dict(returns_ms=round(float(np.median([r[0] for r in rounds])), 4), event_ms=round(float(np.median([r[1] for r in rounds])), 4),
                ms_by_scope={s: round(float(np.median([r[2].get(s, 0.0) for r in rounds])), 4) for s in scopes},
                rounds=[dict(returns_ms=r[0], event_ms=r[1], ms_by_scope=r[2]) for r in rounds])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--cases", default="", help="comma-separated case names (default: all)")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "a")
    L = fastecc_amd.lib()
    parent = parent_library(args.parent_lib) if args.parent_lib else None
    g = torch.Generator(device="cuda:0").manual_seed(7)
    rng = np.random.default_rng(3)
    for name, n, k, count, (col0, width) in CASES:
        if args.cases and name not in args.cases.split(","):
            continue
        block_bytes, m = 4096, n - k
        S = block_bytes // 4
        whole = (col0, width) == (0, S)
        dflags, pflags = np.ones((n, k), np.uint8), np.ones((n, m), np.uint8)  # pattern u loses codeword block u
        for u in range(n):
            (dflags[u] if u < k else pflags[u])[u if u < k else u - k] = 0
        pattern_of = np.array([(0 - b) % n for b in range(count)], dtype=np.uint32)  # placement (i + b) mod n, device 0 down
        with fastecc_amd.Encoder(n, k, block_bytes) as enc, fastecc_amd.Encoder(n, k, block_bytes) as enc_whole:
            enc.decode_prepare_set(dflags, pflags)
            blocks = rng.integers(0, k, size=count)
            indices = [b * k + int(i) for b, i in enumerate(blocks)]
            absent_writes = int(sum(1 for b, i in enumerate(blocks) if pattern_of[b] == i))
            host_list, host_po = (u64 * count)(*indices), (u32 * count)(*[int(q) for q in pattern_of])
            dev_list = torch.tensor(indices, dtype=torch.int64, device="cuda:0")
            dev_po = torch.from_numpy(pattern_of.view(np.int32)).to("cuda:0")
            status = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")

            def degraded_pool():
                data = torch.zeros(count, k, S, dtype=torch.int32, device="cuda:0")
                parity = torch.zeros(count, m, S, dtype=torch.int32, device="cuda:0")
                b = torch.arange(count, device="cuda:0")
                q = torch.from_numpy(pattern_of.astype(np.int64)).to("cuda:0")
                data[b[q < k], q[q < k]] = -1      # 0xFFFFFFFF >= p: an absent block that is read for its content shows
                parity[b[q >= k], q[q >= k] - k] = -1
                return data.view(-1), parity.view(-1)

            pools = {"device": degraded_pool(), "host": degraded_pool()}
            pools["whole"] = (torch.zeros(count * k * S, dtype=torch.int32, device="cuda:0"), torch.zeros(count * m * S, dtype=torch.int32, device="cuda:0"))
            news = [torch.randint(0, P, (count * width,), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32) for _ in range(2)]
            turn = {v: 0 for v in ("device", "host", "parent", "whole")}
            w, s, po = dev_list.data_ptr(), status.data_ptr(), dev_po.data_ptr()

            def rows(variant):
                turn[variant] ^= 1
                return news[turn[variant]].data_ptr()

            def device_call():
                d, p = (t.data_ptr() for t in pools["device"])
                assert L.fastecc_update_batch_set_device(enc._h, d, p, count, po, w, count, 1, count, col0, width, rows("device"), s, None) == 0

            def whole_call():
                d, p = (t.data_ptr() for t in pools["whole"])
                assert L.fastecc_update_batch_device(enc_whole._h, d, p, count, w, count, 1, col0, width, rows("whole"), s, None) == 0

            def host_call(lib, h, variant):
                d, p = (t.data_ptr() for t in pools["host"])
                code = (lib.fastecc_update_batch_set(h, d, p, count, host_po, host_list, count, rows(variant), None) if whole else
                        lib.fastecc_update_batch_set_window(h, d, p, count, host_po, host_list, count, col0, width, rows(variant), None))
                assert code == 0, code

            def check(what):
                """three stripes of the device-list pool against the host-list pool, after one call each with the same rows"""
                turn["device"] = turn["host"] = 0
                device_call()
                host_call(L, enc._h, "host")
                torch.cuda.synchronize()
                assert status.item() == 0, "%s %s: status %#x" % (name, what, status.item() & ((1 << 64) - 1))
                for b in (0, count // 2, count - 1):
                    for got, want, blocks_ in zip(pools["device"], pools["host"], (k, m)):
                        assert torch.equal(got.view(count, blocks_ * S)[b], want.view(count, blocks_ * S)[b]), "%s %s: stripe %d" % (name, what, b)

            check("before the timed calls")
            variants = [("device_list", L, enc._h, device_call), ("host_list", L, enc._h, lambda: host_call(L, enc._h, "host")),
                        ("whole_pool_device_list", L, enc_whole._h, whole_call)]
            ph = vp()
            if parent:
                assert parent.fastecc_create(ctypes.byref(ph), n, k, block_bytes, 0, 0) == 0
                assert parent.fastecc_decode_prepare_set(ph, dflags.ctypes.data_as(u8p), pflags.ctypes.data_as(u8p), n) == 0
                variants.append(("parent_host_list", parent, ph, lambda: host_call(parent, ph, "parent")))
            try:
                got = {v[0]: [] for v in variants}
                for _ in range(args.rounds):
                    for vname, lib, h, fn in variants:
                        got[vname].append(measure(lib, h, fn, args.repeats))
                check("after the timed calls")
            finally:
                torch.cuda.synchronize()
                if parent:
                    parent.fastecc_destroy(ph)
            rec = dict(case=name, code="(%d,%d)" % (n, k), block_bytes=block_bytes, stripes=count, writes=count, absent_writes=absent_writes,
                       max_per_stripe=1, max_absent=count, col0_words=col0, width_words=width, repeats=args.repeats, rounds=args.rounds)
            for vname in got:
                rec[vname] = summary(got[vname])
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
        del pools, news
        torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
