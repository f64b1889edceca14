"""CPU tests of tests/launch_seams.py: its limits are the sources' own, its tiles give the pool's stripes and their parity, and its shapes
cross the seams they are meant for (tests/test_gpu_launch_seams.py asserts the same arithmetic again next to each call)."""
import math
import os
import re

import numpy as np

import launch_seams as ls
from pool_model import Codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_limits_are_the_sources_own():
    """every limit launch_seams.LIMITS restates is defined once, by that name, in the file named there, with that value"""
    assert len(ls.LIMITS) == 5
    for name, (path, value) in ls.LIMITS.items():
        text = open(os.path.join(ROOT, "fastecc_amd", "csrc", path)).read()
        found = re.findall(r"constexpr\s+uint64_t\s+%s\s*=\s*1ull\s*<<\s*(\d+)\s*;" % name, text)
        assert len(found) == 1, "%s does not define %s exactly once" % (path, name)
        assert 1 << int(found[0]) == value, "%s changed: the seam tests no longer cross it" % name


def test_transform_cases_are_one_pass_plans(hip_lib):
    """the plans the transform cases assume (host-only fastecc_plan_describe): one register pass of one wave per stripe, one 64-block tile of two"""
    import fastecc_amd as fe
    for shape in ls.TRANSFORM:
        assert fe.plan_describe(shape["k"], 4 * shape["S"]) == shape["plan"]


DISPATCH_PROBE = r"""
#include <stdio.h>
#include "launch_limits.hpp"
using namespace fastecc;
int main()
{
    const uint64_t waves[] = {0, 1, 4, (1ull << 24), (1ull << 24) + 1, 17ull << 20, (1ull << 26) - 4, (1ull << 26) - 3, 1ull << 26, 1ull << 40};
    for (uint64_t w : waves) printf("waves %llu %d\n", (unsigned long long)w, (int)wave_launch_fits(w));
    printf("rows %llu %llu %llu\n", (unsigned long long)rows_waves(1025, 1, 1ull << 20), (unsigned long long)rows_waves(1024, 4, 1ull << 19),
           (unsigned long long)pass_stripe_waves(1, 1, 1, 1));
    printf("stripe %llu %llu %llu\n", (unsigned long long)tile_stripe_waves(6, false, 5, 1, 6), (unsigned long long)tile_stripe_waves(10, true, 5, 1024, 19),
           (unsigned long long)tile_stripe_waves(9, true, 4, 16384, 19));
    // tiles of 16 waves (1024 threads): 2^22 - 1 workgroups fit, 2^22 do not; tiles of 2 waves: 2^25 - 1 and 2^25
    printf("tile %d %d %d %d\n", (int)tile_launch_fits((1ull << 22) - 1, 9, true, 4, true, false, 0, 256), (int)tile_launch_fits(1ull << 22, 9, true, 4, true, false, 0, 256),
           (int)tile_launch_fits((1ull << 25) - 1, 6, false, 5, false, false, 0, 256), (int)tile_launch_fits(1ull << 25, 6, false, 5, false, false, 0, 256));
    // the 128 KiB tiles run persistent (a grid sized to the machine) unless split, windowed or persistence is off; 32-bit tile indices always
    printf("capped %d %d %d %d %d %d %d\n", (int)tile_launch_fits(1ull << 30, 10, true, 5, true, false, 0, 256), (int)tile_launch_fits(1ull << 30, 10, true, 5, true, true, 0, 256),
           (int)tile_launch_fits(1ull << 30, 10, true, 5, true, false, 2, 256), (int)tile_launch_fits(1ull << 30, 10, true, 5, true, false, 0, 0),
           (int)tile_launch_fits(1ull << 30, 9, false, 5, false, true, 0, 256), (int)tile_launch_fits(1ull << 30, 9, false, 5, true, true, 0, 256),
           (int)tile_launch_fits(1ull << 31, 10, true, 5, true, false, 0, 256));
    return 0;
}
"""


def test_one_launch_is_refused_at_the_dispatch_limit_only(tmp_path):
    """launch_limits.hpp compiled on the host: a single launch (a stripe cannot be cut) is refused where it would hold 2^32 work-items or more and
    nowhere below — not at the 2^24 waves the batched split uses as its run size.  k = 2^20 blocks of 4100 bytes (17 * 2^20 waves in the row
    kernels: 1.14e9 work-items) fits."""
    import subprocess
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(DISPATCH_PROBE)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "fastecc_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    got = {int(line.split()[1]): bool(int(line.split()[2])) for line in out if line.startswith("waves")}
    assert len(got) == 10
    for waves, fits in got.items():
        assert fits == ls.wave_launch_fits(waves) == (0 < -(-waves // 4) * 256 < 1 << 32), waves
    assert got[17 << 20] and got[(1 << 26) - 4] and not got[(1 << 26) - 3] and not got[0] and got[(1 << 24) + 1]
    assert out[10].split()[1:] == [str(ls.rows_waves(1025, 1, 1 << 20)), str(ls.rows_waves(1024, 4, 1 << 19)), "1"] and ls.rows_waves(1025, 1, 1 << 20) == 17 << 20
    assert out[11].split()[1:] == [str(shape["stripe_waves"]) for shape in ls.TRANSFORM][1:] + [str(32 * 512 * 16), str(512 * 1024 * 16)]
    assert out[12].split()[1:] == ["1", "0", "1", "0"]
    assert out[13].split()[1:] == ["1", "0", "0", "0", "1", "0", "0"]


def test_tile_is_the_stripes_and_their_parity(oracle):
    """column t * S + c of the tile is word c of stripe t: the rearranged tile and its one-call parity against a per-stripe loop of Codec.parity"""
    for n, k, S in ((3, 2, 129), (6, 4, 1), (20, 16, 192), (4, 2, 1), (128, 64, 1)):
        x = ls.draw_tile(n * 1000 + S, k, S, period=50)
        data, parity = ls.tile_to_stripes(x, S), ls.tile_to_stripes(ls.tile_parity(oracle, n, k, x), S)
        assert data.shape == (50, k, S) and parity.shape == (50, n - k, S) and (data < ls.P).all()
        codec = Codec(oracle, n, k)
        for t in range(50):
            assert np.array_equal(data[t], x[:, t * S:(t + 1) * S])
            assert np.array_equal(parity[t], codec.parity(data[t])), (n, k, S, t)
        assert len({data[t].tobytes() for t in range(50)}) == 50  # neighbours differ: a stripe read one entry off is seen


def test_period_divides_no_launch_size():
    assert all(ls.T % d for d in range(2, 65)) and ls.coprime_to_launch_sizes()
    for size in ls.launch_sizes():
        assert math.gcd(ls.T, size) == 1 and 0 < size % ls.T < ls.T  # every seam falls inside a tile
    k = ls.WRITES["k"]
    for period in (k * ls.T, 3 * k * ls.T):  # the truth after the bursts of the write case has these periods
        assert ls.LAUNCH_WAVES % period != 0


def test_shapes_cross_their_seams():
    for shape, eb in ((ls.SET_A, 1), (ls.SET_A, 2), (ls.SET_B, 1)):
        wpe = ls.set_waves_per_entry(eb, shape["S"])
        assert ls.with_work(shape["count"]) > ls.SET_LAUNCH_WAVES // wpe + 1000
    assert ls.set_waves_per_entry(1, ls.SET_A["S"]) == 1 and ls.set_waves_per_entry(1, ls.SET_B["S"]) == 3
    assert [ls.read_waves_per_entry(ls.READ["S"], c, w) for c, w in ls.READ_WINDOWS] == [1, 3]
    assert math.gcd(ls.READ["stride"], ls.READ["count"] * ls.READ["k"]) == 1
    assert ls.WRITES["count"] > ls.LAUNCH_WAVES + 1000  # one write and one segment of one wave per stripe
    assert ls.batch_groups(1, ls.GROUPS["S"], ls.GROUPS["count"]) == ls.LAUNCH_GROUPS + ls.T + 3
    assert ls.MFMA["count"] * -(-ls.MFMA["S"] // 64) == ls.POOL_LAUNCH_WAVES
    for shape in ls.TRANSFORM:
        assert shape["count"] * shape["stripe_waves"] > ls.MAX_LAUNCH_WAVES + 1000 and shape["count"] * shape["k"] <= 0x7FFFFFFF


def test_write_bursts_rewrite_what_they_name():
    k, count = 4, 50
    x0 = ls.draw_tile(1, k, 1)
    nw, wa, wb = (np.arange(ls.T, dtype=np.uint32) + np.uint32(off) for off in (10, 20000, 40000))
    x1 = ls.burst1(x0, nw, k)
    x2 = ls.burst2(x1, wa, wb, k)
    w1 = ls.burst1_writes(count, k)
    w2, stripe2, which2 = ls.burst2_writes(count, k)
    assert w1.dtype == np.uint64 and w2.dtype == np.uint64 and w2.flags["C_CONTIGUOUS"] and len(set(w2.tolist())) == len(w2)
    pool = np.tile(x0, (1, 12)).T[:count].copy()  # (stripe, block)
    for b, w in enumerate(w1.tolist()):
        assert w // k == b and w % k == b % k
        pool[b, w % k] = nw[b % ls.T]
    assert np.array_equal(pool, x1.T[np.arange(count) % (k * ls.T)])
    for w, b, second in zip(w2.tolist(), stripe2.tolist(), which2.tolist()):
        assert w // k == b and b % 3 == 0 and w % k == (b + 1 + second) % k
        pool[b, w % k] = (wb if second else wa)[b % ls.T]
    assert np.array_equal(pool, x2.T[np.arange(count) % (3 * k * ls.T)])
