"""CPU test of fastecc_amd/csrc/update_list.hpp: the sorted write list and the segment tables that the pool write calls hand their parity kernels.

The header is compiled with the host compiler alone into a small program that reads cases and prints the words sort_writes and build_update_list
give.  They are compared word for word with `expected` below, which restates the formats from their description (the header comment of update.hip,
DESIGN.md sections 15, 33 and 36), and the properties the parity kernels rely on are asserted on the printed words themselves.

A stripe of K = 16 blocks cannot hold 17 or 33 distinct writes, so the K = 16 cases hold stripes of 1, 2, 3, 5, 9 and 16 writes and the cases with
all eight stripe sizes (rounds 0 to 2, every length class, a last segment of one write) run at K = 40."""
import itertools
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF
ROW_ABSENT, OLD_IN_POOL, LOST_PITCH = 0x80000000, 0xFFFFFFFF, 17

PROBE = r"""
#include <iostream>
#include "update_list.hpp"
using namespace fastecc;
int main()
{
    unsigned long long id, K, S, W, col0, M, recon, count, n;
    int e, with_data, long_form, has_set;
    while (std::cin >> id >> K >> e >> S >> W >> col0 >> M >> with_data >> long_form >> has_set >> recon >> count >> n) {
        std::vector<uint64_t> writes(n);
        for (auto& w : writes) std::cin >> w;
        std::vector<uint32_t> arrays[3];
        for (auto& a : arrays) {
            a.resize(has_set ? n : 0);
            for (auto& x : a) std::cin >> x;
        }
        std::vector<SortedWrite> sw;
        const bool ok = sort_writes(K, count, writes.data(), n, sw);
        std::cout << "case " << id << "\nsort " << ok << "\n";
        if (!ok) continue;
        const ListShape shape{K, e, S, W, col0, M, with_data != 0, long_form != 0};
        const ListSet set{arrays[0].data(), arrays[1].data(), arrays[2].data(), %d, recon};
        const bool is_long = long_form || has_set;  // a set always has the long records
        const size_t record = is_long ? SET_LIST_WORDS : LIST_WORDS, head = is_long ? SET_SEG_HEAD : SEG_HEAD;
        std::vector<uint32_t> words(n * (record + head + 1), 0xDEADBEEFu);
        std::vector<BatchLaunch> launches;
        const BuiltList built = build_update_list(sw, shape, has_set ? &set : nullptr, words.data(), launches);
        std::cout << "sorted";
        for (const SortedWrite& w : sw) std::cout << " " << w.index << " " << w.row;
        std::cout << "\nlist";
        for (size_t i = 0; i < n * record; i++) std::cout << " " << words[i];
        std::cout << "\nsegs";
        for (size_t i = 0; i < built.seg_words; i++) std::cout << " " << words[n * record + i];
        std::cout << "\n";
        for (const BatchLaunch& l : launches) std::cout << "launch " << l.T << " " << l.seg0 << " " << l.segs << " " << l.parity_blocks << "\n";
        std::cout << "stored " << built.stored << "\n";
    }
    return 0;
}
""" % LOST_PITCH

ALL_SIZES = (1, 2, 3, 5, 9, 16, 17, 33)
FORMS = {  # name -> (S, W, col0, data pool, long form, pattern set, offset of the reconstruction buffer in words)
    "short": (64, 64, 0, True, False, False, 0),
    "short_parity": (64, 64, 0, False, False, False, 0),
    "long_pool": (64, 64, 0, True, True, False, 0),
    "long_rows": (64, 64, 0, False, True, False, 0),
    "long_set": (64, 64, 0, True, True, True, 5 << 33),
    "long_set_below": (64, 64, 0, True, True, True, (1 << 64) - 4096),  # the buffer lies below the base: a negative offset
    "window_pool": (64, 24, 8, True, True, False, 0),
    "window_rows": (64, 24, 8, False, True, False, 0),
    "window_set": (64, 24, 8, True, True, True, 1 << 20),
    "set_implies_long": (64, 64, 0, True, False, True, 1 << 20),  # a set has the long records whatever the shape says
}


def make_case(K, e, sizes, form, seed):
    S, W, col0, with_data, long_form, has_set, recon = FORMS[form]
    rng = random.Random(seed)
    M = 4
    stripes = sorted(rng.sample(range(1000), len(sizes) - 1)) + [(1 << 32) + 5]  # the last stripe: the high word of b
    rng.shuffle(stripes)
    writes = [b * K + i for b, size in zip(stripes, sizes) for i in rng.sample(range(K), size)]
    rng.shuffle(writes)
    case = dict(K=K, e=e, S=S, W=W, col0=col0, M=M, with_data=with_data, long_form=long_form, recon=recon, count=(1 << 32) + 6, writes=writes, set=None)
    if has_set:  # by SORTED write: two absent blocks (rows 1 and 0 of the reconstruction buffer), a pattern and its present parity per stripe
        order = sorted(writes)
        old_row = [OLD_IN_POOL] * len(order)
        for row, g in enumerate(rng.sample(range(len(order)), 2)):
            old_row[g] = 1 - row
        case["set"] = (old_row, [(w // K) % 7 for w in order], [M - (w // K) % 3 for w in order])
    return case


CASES = [make_case(K, e, sizes, form, 100 * K + 10 * e + j) for K, sizes in ((16, ALL_SIZES[:6]), (40, ALL_SIZES)) for e in (0, 1)
         for j, form in enumerate(FORMS)]
REFUSED = [  # sort_writes alone: count * K = 48
    dict(K=16, count=3, writes=[5, 48, 7], ok=False),  # an index >= count * K
    dict(K=16, count=3, writes=[5, 47, 7], ok=True),
    dict(K=16, count=3, writes=[5, 47, 7, 5], ok=False),  # a duplicate
    dict(K=16, count=3, writes=[9, 9], ok=False),
]


def expected(c):
    """the list, the segment tables and the launches from the description of the formats"""
    K, W, writes, long_form = c["K"], c["W"], c["writes"], c["long_form"] or c["set"] is not None
    order = sorted(range(len(writes)), key=lambda u: writes[u])
    old_row, lost_row, present = c["set"] or (None, None, None)
    records, stored = [], 0
    for g, u in enumerate(order):
        b, i = divmod(writes[u], K)
        rec, absent = [i << c["e"], u, b & M32, b >> 32], bool(old_row) and old_row[g] != OLD_IN_POOL
        if long_form:
            off = c["recon"] + old_row[g] * W if absent else writes[u] * c["S"] + c["col0"] if c["with_data"] else u * W
            rec[1] |= ROW_ABSENT if absent else 0
            rec += [off & M32, (off >> 32) & M32]
        stored += not absent
        records.append(rec)
    tables = {}  # (round, T) -> [(segment words, parity blocks)]
    for _, group in itertools.groupby(range(len(order)), key=lambda g: writes[order[g]] // K):
        group = list(group)
        for rnd, at in enumerate(range(0, len(group), 16)):
            seg = group[at:at + 16]
            T = 1 << (len(seg) - 1).bit_length()
            head = [seg[0], len(seg)] + ([lost_row[seg[0]] * LOST_PITCH if lost_row else 0] if long_form else [])
            positions = [records[g][0] for g in seg] + [records[seg[0]][0]] * (T - len(seg))
            tables.setdefault((rnd, T), []).append((head + positions, present[seg[0]] if present else c["M"]))
    segs, launches = [], []
    for key in sorted(tables):
        launches.append((key[1], len(segs), len(tables[key]), sum(blocks for _, blocks in tables[key])))
        segs += [w for words, _ in tables[key] for w in words]
    return dict(sorted=[x for u in order for x in (writes[u], u)], list=[w for rec in records for w in rec], segs=segs, launches=launches, stored=stored)


def probe_input():
    """what the probe reads: every case, then the lists for sort_writes alone"""
    lines = []
    for i, c in enumerate(CASES + REFUSED):
        full = dict(dict(e=0, S=1, W=1, col0=0, M=1, with_data=1, long_form=0, recon=0, set=None), **c)
        lines.append(" ".join(str(int(x)) for x in [i] + [full[f] for f in ("K", "e", "S", "W", "col0", "M", "with_data", "long_form")]
                              + [full["set"] is not None, full["recon"], full["count"], len(full["writes"])]))
        lines.append(" ".join(str(w) for w in full["writes"]))
        for array in full["set"] or ():
            lines.append(" ".join(str(x) for x in array))
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """every case through the probe, once: case id -> what it printed"""
    tmp = tmp_path_factory.mktemp("update_list")
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text(PROBE)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "fastecc_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], input=probe_input(), capture_output=True, text=True, check=True).stdout
    got, cur = {}, None
    for line in out.splitlines():
        key, *rest = line.split()
        if key == "case":
            cur = got.setdefault(int(rest[0]), dict(launches=[]))
        elif key == "launch":
            cur["launches"].append(tuple(int(x) for x in rest))
        elif key in ("sort", "stored"):
            cur[key] = int(rest[0])
        else:
            cur[key] = [int(x) for x in rest]
    assert sorted(got) == list(range(len(CASES) + len(REFUSED)))
    return got


def test_header_needs_no_hip():
    text = open(os.path.join(ROOT, "fastecc_amd", "csrc", "update_list.hpp")).read()
    includes = sorted(line.split()[1] for line in text.splitlines() if line.startswith("#include"))
    assert includes == ["<algorithm>", "<cstdint>", "<vector>"]


def test_sort_writes_refuses_what_it_must(built):
    for i, c in enumerate(REFUSED, len(CASES)):
        assert built[i]["sort"] == c["ok"], c
    assert all(built[i]["sort"] == 1 for i in range(len(CASES)))


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: "K%d-e%d-case%d" % (CASES[i]["K"], CASES[i]["e"], i))
def test_words_are_the_formats(built, i):
    want, got = expected(CASES[i]), built[i]
    for part in ("sorted", "list", "segs", "launches", "stored"):
        assert got[part] == want[part], part
    if CASES[i]["set"]:
        assert got["stored"] == len(CASES[i]["writes"]) - 2 and sum(w >> 31 for w in got["list"][1::6]) == 2


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: "K%d-e%d-case%d" % (CASES[i]["K"], CASES[i]["e"], i))
def test_what_the_kernels_rely_on(built, i):
    c, got = CASES[i], built[i]
    K, n = c["K"], len(c["writes"])
    record, head = (6, 3) if c["long_form"] or c["set"] else (4, 2)
    assert len(got["list"]) == n * record
    stripe_of = [got["list"][g * record + 2] | got["list"][g * record + 3] << 32 for g in range(n)]
    assert stripe_of == [w // K for w in sorted(c["writes"])] and max(stripe_of) >> 32 == 1
    covered, rounds_of, rnd, at, last_T = [0] * n, {}, 0, 0, 0
    for T, seg0, segs, _ in got["launches"]:
        assert T in (1, 2, 4, 8, 16) and seg0 == at and segs > 0
        rnd += T <= last_T and last_T != 0  # by round, then by class: the classes of a round increase
        assert T > last_T or last_T == 16  # ... and a round that another follows has full segments
        last_T = T
        for s in range(segs):
            seg = got["segs"][at:at + head + T]
            first, length = seg[0], seg[1]
            assert T // 2 < length <= T and first + length <= n  # T: the length padded to a power of two
            assert len(set(stripe_of[first:first + length])) == 1
            for r in range(T):  # the rows' positions; pad slots repeat the first
                assert seg[head + r] == got["list"][(first + (r if r < length else 0)) * record]
            for g in range(first, first + length):
                covered[g] += 1
            rounds_of.setdefault(stripe_of[first], []).append((first, length, rnd))
            at += head + T
    assert at == len(got["segs"]) and covered == [1] * n  # every write in exactly one segment
    for b, segs in rounds_of.items():  # segment r of a stripe: round r, full unless it is the last
        segs.sort()
        assert [rnd for _, _, rnd in segs] == list(range(len(segs)))
        assert all(length == 16 for _, length, _ in segs[:-1])
        assert all(segs[r + 1][0] == segs[r][0] + 16 for r in range(len(segs) - 1))
    sizes = sorted(len(list(g)) for _, g in itertools.groupby(stripe_of))
    assert sizes == list(ALL_SIZES[:6] if K == 16 else ALL_SIZES)
    if K == 40:
        assert rnd == 2 and {T for T, *_ in got["launches"]} == {1, 2, 4, 8, 16}
