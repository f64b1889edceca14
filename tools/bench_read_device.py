#!/usr/bin/env python3
"""Time the degraded reads from a request list in device memory (fastecc_read_batch_set_device) against the host-list call on the same inputs
(fastecc_read_batch_set), in one process on one GPU.  Pools as in tools/bench_read_set.py: rotated (20,16) x 4 KB x 32768 stripes and
(256,128) x 4 KB x 4096 stripes with one device down (pattern q loses codeword block q, pattern_of[b] = b mod n).  Per pool three lists: every
lost data block at full width, the same with a 128-word window, and a list in which nine of ten requests are for present blocks (full width).
For each case:
  (a) the device-list call of this library: the host's time inside the call ("returns", the stream idle when it starts) and the HIP-event
      interval around it;
  (b) the host-list call of this library;
  (c) the host-list call of a library built from the parent commit (--parent-lib PATH), through a context of its own;
alternating over three rounds, each round the median of --repeats calls after warm-up, and per round the device's time by profile scope (mean of
5 calls).  Before anything is timed three requests of each variant are checked against the original data.
Two conditions (reported per case, exit status 1 when one is missed; both need --parent-lib):
  host_list_unchanged : the median of (b)'s round medians is no larger than the largest of (c)'s round medians;
  read_scope_ok       : the read scope of (a) (direct_read_device_set) is no slower than direct_read_set of (c) by more than half the range of
                        (c)'s three round values of that scope.
The event time of (a) against (c) is reported, not gated.  One JSON line per case, appended to --out (default
profiles/read_device/bench_read_device.jsonl).
  python tools/bench_read_device.py [--repeats R] [--out FILE] [--parent-lib PATH]"""
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
ROUNDS = 3
DEFAULT_OUT = os.path.join(ROOT, "profiles", "read_device", "bench_read_device.jsonl")
POOLS = [("20_16_rot", 20, 16, 32768), ("256_128_rot", 256, 128, 4096)]
vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
u8p = ctypes.POINTER(ctypes.c_uint8)


def parent_library(path):
    """the parent commit's library with the few entry points this tool calls"""
    L = ctypes.CDLL(path)
    L.fastecc_create.argtypes, L.fastecc_create.restype = [ctypes.POINTER(vp), u64, u64, u64, i32, i32], i32
    L.fastecc_destroy.argtypes, L.fastecc_destroy.restype = [vp], None
    L.fastecc_decode_prepare_set.argtypes, L.fastecc_decode_prepare_set.restype = [vp, u8p, u8p, u64], i32
    L.fastecc_read_batch_set.argtypes = [vp, vp, vp, u64, ctypes.POINTER(u32), ctypes.POINTER(u64), u64, u64, u64, vp, vp]
    L.fastecc_read_batch_set.restype = i32
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


def one_round(L, h, fn, reps):
    """(host ms for the call to return, HIP-event ms of the call: medians of reps; device ms by profile scope)"""
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
    out_file = open(args.out, "a")
    L = fastecc_amd.lib()
    parent = parent_library(args.parent_lib) if args.parent_lib else None
    g = torch.Generator(device="cuda:0").manual_seed(7)
    failed = False
    for pool_name, n, k, count in POOLS:
        block_bytes, m = 4096, n - k
        S = block_bytes // 4
        with fastecc_amd.Encoder(n, k, block_bytes) as enc:
            data = torch.randint(0, P, (count * k * S,), dtype=torch.int64, device="cuda:0", generator=g).to(torch.int32)
            parity = torch.empty(count * m * S, dtype=torch.int32, device="cuda:0")
            enc.encode_pool(data, parity, count)
            torch.cuda.synchronize()
            want = data.clone().view(count * k, S)
            dp, pp = np.ones((n, k), np.uint8), np.ones((n, m), np.uint8)
            for q in range(n):
                if q < k:
                    dp[q, q] = 0
                else:
                    pp[q, q - k] = 0
            stripe = np.arange(count, dtype=np.uint64)
            pattern_of = (stripe % n).astype(np.uint32)
            lost = pattern_of < k
            every_lost = (stripe[lost] * k + pattern_of[lost]).astype(np.uint64)
            some = every_lost[::10]
            mixed = np.concatenate([some] + [(some // k) * k + (some % k + d) % k for d in range(1, 10)]).astype(np.uint64)[:len(every_lost)]
            np.random.default_rng(11).shuffle(mixed)
            enc.decode_prepare_set(dp, pp)
            ph = vp()
            if parent:
                assert parent.fastecc_create(ctypes.byref(ph), n, k, block_bytes, 0, 0) == 0
                assert parent.fastecc_decode_prepare_set(ph, dp.ctypes.data_as(u8p), pp.ctypes.data_as(u8p), n) == 0
            # the lost blocks hold garbage: a read that copied one would show
            stripes_t = torch.arange(count, device="cuda:0")
            lost_t = stripes_t % n
            in_d, in_p = lost_t < k, lost_t >= k
            data.view(count, k, S)[stripes_t[in_d], lost_t[in_d]] = -1
            parity.view(count, m, S)[stripes_t[in_p], lost_t[in_p] - k] = -1
            d_po = torch.from_numpy(pattern_of.view(np.int32)).to("cuda:0")
            status = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
            out = torch.empty(len(every_lost) * S, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            d, p, o, s, po_d = data.data_ptr(), parity.data_ptr(), out.data_ptr(), status.data_ptr(), d_po.data_ptr()
            po_h = pattern_of.ctypes.data_as(ctypes.POINTER(u32))
            try:
                for list_name, reads, (col0, width) in (("every_lost_full", every_lost, (0, S)), ("every_lost_window_128", every_lost, (256, 128)),
                                                        ("nine_of_ten_present_full", mixed, (0, S))):
                    nr = len(reads)
                    d_reads = torch.from_numpy(reads.view(np.int64)).to("cuda:0")
                    r_h, r_d = reads.ctypes.data_as(ctypes.POINTER(u64)), d_reads.data_ptr()

                    def device_call():
                        assert L.fastecc_read_batch_set_device(enc._h, d, p, count, po_d, r_d, nr, col0, width, o, s, None) == 0

                    def host_call(lib=L, h=None):
                        assert lib.fastecc_read_batch_set(h or enc._h, d, p, count, po_h, r_h, nr, col0, width, o, None) == 0

                    def check(what):
                        """three requests (the first, a middle one, the last) against the original data"""
                        torch.cuda.synchronize()
                        for u in (0, nr // 2, nr - 1):
                            assert torch.equal(out[u * width:(u + 1) * width], want[int(reads[u]), col0:col0 + width]), "%s %s %s: row %d" % (pool_name, list_name, what, u)
                        out.fill_(0)

                    variants = [("device_list", L, enc._h, device_call), ("host_list", L, enc._h, host_call)]
                    if parent:
                        variants.append(("parent_host_list", parent, ph, lambda: host_call(parent, ph)))
                    for vname, _, _, fn in variants:
                        out.fill_(0)
                        fn()
                        check(vname)
                    assert status.item() == 0
                    rounds = {vname: [] for vname, _, _, _ in variants}
                    for _ in range(ROUNDS):
                        for vname, lib, h, fn in variants:
                            rounds[vname].append(one_round(lib, h, fn, args.repeats))
                    device_call()
                    check("device_list after the timed calls")
                    assert status.item() == 0
                    rec = dict(case="%s_%s" % (pool_name, list_name), code="(%d,%d)" % (n, k), block_bytes=block_bytes, stripes=count, requests=int(nr),
                               col0_words=col0, width_words=width, repeats=args.repeats, rounds=ROUNDS)
                    for vname, rs in rounds.items():
                        rec[vname + "_returns_ms"] = round(float(np.median([r[0] for r in rs])), 4)
                        rec[vname + "_event_ms"] = round(float(np.median([r[1] for r in rs])), 4)
                        rec[vname + "_event_ms_rounds"] = [r[1] for r in rs]
                        rec[vname + "_ms_by_scope_rounds"] = [r[2] for r in rs]
                    if parent:
                        c_rounds = rec["parent_host_list_event_ms_rounds"]
                        rec["host_list_unchanged"] = bool(rec["host_list_event_ms"] <= max(c_rounds))
                        c_scope = [r[2]["direct_read_set"] for r in rounds["parent_host_list"]]
                        a_scope = [r[2]["direct_read_device_set"] for r in rounds["device_list"]]
                        rec["read_scope_device_list_ms"] = round(float(np.median(a_scope)), 4)
                        rec["read_scope_parent_ms"] = round(float(np.median(c_scope)), 4)
                        rec["read_scope_parent_half_range_ms"] = round((max(c_scope) - min(c_scope)) / 2, 4)
                        rec["read_scope_ok"] = bool(np.median(a_scope) - np.median(c_scope) <= (max(c_scope) - min(c_scope)) / 2)
                        failed |= not (rec["host_list_unchanged"] and rec["read_scope_ok"])
                    line = json.dumps(rec)
                    print(line, flush=True)
                    out_file.write(line + "\n")
                    out_file.flush()
            finally:
                torch.cuda.synchronize()
                if parent:
                    parent.fastecc_destroy(ph)
        del data, parity, want, out
        torch.cuda.empty_cache()
    out_file.close()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
