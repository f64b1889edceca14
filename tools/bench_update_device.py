#!/usr/bin/env python3
"""Time the pool writes from a write list in device memory (fastecc_update_batch_device) against the host-list call on the same inputs
(fastecc_update_batch, or fastecc_update_batch_window for a window).  Cases, one uniformly random write per stripe, max_per_stripe = 1:
(20,16) x 4 KB x 32768 stripes with the whole block and with a 512-byte window, and (256,128) x 4 KB x 4096 stripes with the whole block; the window case
once more under max_per_stripe = 16 (the same list: what the promise alone costs).
The pools start all zero (pools of codewords); calls alternate between two sets of new rows, so every call changes every word it names.
Per case and call: the time for the call to return on the host (the stream idle when it starts), the HIP-event time of the call (median of
--repeats, the interval holds the host's work as well) and the device's time by profile scope (fastecc_profile_read, mean of 5 calls) —
update_device_build, update_device and update_device_scatter for the device-list call.  --parent-lib PATH names a libfastecc_hip.so built from the
parent commit: its host-list call is then timed on the same inputs through a context of its own, beside this library's.  Before anything is
timed, and after, a few touched stripes are checked against fastecc_encode of their data.  One JSON line per case, appended to --out (default
profiles/update_device/bench_update_device.jsonl).
  python tools/bench_update_device.py [--repeats R] [--out FILE] [--parent-lib PATH]"""
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
DEFAULT_OUT = os.path.join(ROOT, "profiles", "update_device", "bench_update_device.jsonl")
# (name, n, k, stripes, window, max_per_stripe); the last case: the same one-write-per-stripe list under a promise of 16 — five parity launches
CASES = [("20_16_whole_block", 20, 16, 32768, (0, 1024), 1), ("20_16_window_512B", 20, 16, 32768, (0, 128), 1),
         ("256_128_whole_block", 256, 128, 4096, (0, 1024), 1), ("20_16_window_512B_promise_16", 20, 16, 32768, (0, 128), 16)]
vp, u64, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int


def parent_library(path):
    """the parent commit's library with the few entry points this tool calls"""
    L = ctypes.CDLL(path)
    L.fastecc_create.argtypes, L.fastecc_create.restype = [ctypes.POINTER(vp), u64, u64, u64, i32, i32], i32
    L.fastecc_destroy.argtypes, L.fastecc_destroy.restype = [vp], None
    L.fastecc_update_batch.argtypes, L.fastecc_update_batch.restype = [vp, vp, vp, u64, ctypes.POINTER(u64), u64, vp, vp], i32
    L.fastecc_update_batch_window.argtypes, L.fastecc_update_batch_window.restype = [vp, vp, vp, u64, ctypes.POINTER(u64), u64, u64, u64, vp, vp], i32
    L.fastecc_profile_enable.argtypes, L.fastecc_profile_enable.restype = [vp, i32], i32
    L.fastecc_profile_reset.argtypes, L.fastecc_profile_reset.restype = [vp], i32
    L.fastecc_profile_read_bytes.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(u64), ctypes.POINTER(u64), i32]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--parent-lib", default="")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "a")
    L = fastecc_amd.lib()
    parent = parent_library(args.parent_lib) if args.parent_lib else None
    g = torch.Generator(device="cuda:0").manual_seed(7)
    rng = np.random.default_rng(3)
    for name, n, k, count, (col0, width), mps in CASES:
        block_bytes, m = 4096, n - k
        S = block_bytes // 4
        whole = (col0, width) == (0, S)
        with fastecc_amd.Encoder(n, k, block_bytes) as enc:
            blocks = rng.integers(0, k, size=count)
            indices = [b * k + int(i) for b, i in enumerate(blocks)]
            host_list = (u64 * count)(*indices)
            dev_list = torch.tensor(indices, dtype=torch.int64, device="cuda:0")
            status = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
            data = torch.zeros(count * k * S, dtype=torch.int32, device="cuda:0")
            parity = torch.zeros(count * m * S, dtype=torch.int32, device="cuda:0")
            news = [torch.randint(0, P, (count * width,), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32) for _ in range(2)]
            turn = [0]
            d, p, w, s = data.data_ptr(), parity.data_ptr(), dev_list.data_ptr(), status.data_ptr()

            def rows():
                turn[0] ^= 1
                return news[turn[0]].data_ptr()

            def device_call():
                assert L.fastecc_update_batch_device(enc._h, d, p, count, w, count, mps, col0, width, rows(), s, None) == 0

            def host_call(lib, h):
                code = (lib.fastecc_update_batch(h, d, p, count, host_list, count, rows(), None) if whole else
                        lib.fastecc_update_batch_window(h, d, p, count, host_list, count, col0, width, rows(), None))
                assert code == 0, code

            def check(what):
                """a few touched stripes: the written window holds the last rows, the parity is fastecc_encode of the stripe's data"""
                torch.cuda.synchronize()
                assert status.item() in (0, -1), "%s %s: status %#x" % (name, what, status.item() & ((1 << 64) - 1))
                for b in (0, count // 2, count - 1):
                    stripe = data.view(count, k * S)[b].contiguous()
                    fresh = torch.empty(m * S, dtype=torch.int32, device="cuda:0")
                    enc.encode(stripe, fresh)
                    torch.cuda.synchronize()
                    assert torch.equal(fresh, parity.view(count, m * S)[b]), "%s %s: the parity of stripe %d is not its encode" % (name, what, b)
                    assert torch.equal(stripe.view(k, S)[blocks[b], col0:col0 + width], news[turn[0]].view(count, width)[b]), "%s %s: stripe %d" % (name, what, b)

            device_call()
            check("first device-list call")
            assert status.item() == 0
            rec = dict(case=name, code="(%d,%d)" % (n, k), block_bytes=block_bytes, stripes=count, writes=count, max_per_stripe=mps, col0_words=col0,
                       width_words=width, repeats=args.repeats)
            rec["device_list_host_ms"], rec["device_list_event_ms"], rec["device_list_ms_by_scope"] = measure(L, enc._h, device_call, args.repeats)
            check("device-list calls")
            rec["host_list_host_ms"], rec["host_list_event_ms"], rec["host_list_ms_by_scope"] = measure(L, enc._h, lambda: host_call(L, enc._h), args.repeats)
            check("host-list calls")
            if parent:
                h = vp()
                assert parent.fastecc_create(ctypes.byref(h), n, k, block_bytes, 0, 0) == 0
                try:
                    rec["parent_host_list_host_ms"], rec["parent_host_list_event_ms"], rec["parent_host_list_ms_by_scope"] = measure(
                        parent, h, lambda: host_call(parent, h), args.repeats)
                    check("the parent's host-list calls")
                finally:
                    torch.cuda.synchronize()
                    parent.fastecc_destroy(h)
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
        del data, parity, news
        torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
