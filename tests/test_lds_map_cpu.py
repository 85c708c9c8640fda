"""compairr_amd/csrc/lds_map.h on the CPU: the header compiles with plain g++ -std=c++17, every map's regions
lie back to back in the documented order at the alignment their type needs, `bytes` is the end of the last one,
and the totals -- at the arguments make_plan and the index build pass -- equal what the host formulas gave before
there was a map (tests/golden/lds_budget.json: recorded once, from a program holding the formulas of the commit
the fixture names, over the grid below).

Alignment: 16 bytes for the slices (address 0: read as 32-byte words, copied in 1 KiB LDS-DMA pieces), 8 for the
u64 regions and for everything that holds a u64 (wave queues, ring slots), 4 for the u32 tables.  The tile
references of the rows and pair kernels are LDS-DMA targets too, and they are NOT at 16 bytes: behind a Zobrist
table with an odd number of keys (A + 1 = 21 keys per position, odd zpos) or an odd number of matrix cells they
lie at 8 mod 16, today as before the map -- the order and size of the regions was to stay as it was, so this test
asserts the 8 bytes that hold for them and `test_tile_references_at_16_bytes_where_the_tables_are_even` the 16
where the tables in front are whole 16-byte units.  (Variant 1's tile references are written with plain stores.)
The rows kernel's copies into such a place run in tests/test_lds_decisions_gpu.py (aa_d1_100, aa_d1_282: 21 keys
per position, zpos 103 and 285), matrices held against the oracle; the pair kernel with an odd number of cells is
in no test.
"""

import functools
import hashlib
import json
import os
import subprocess

import pytest

from conftest import ROOT

FIXTURE = os.path.join(ROOT, "tests", "golden", "lds_budget.json")
CSRC = os.path.join(ROOT, "compairr_amd", "csrc")
LDS_BYTES = 160 * 1024

ZPOS = (4, 23, 151, 520, 2600, 5300)
WAVES = (4, 8, 16)
CAPS = (16, 64, 512)
CELLS = (0, 1, 2048)
GENES = (0, 73, 8000)
OFF_CR = 8100            # class-table words in front of the class-residue rows: lengths + V + J


def grid():
    """{formula: [argument tuples]} -- the arguments are the host's (context fields), not the maps'"""
    g = {}
    g["plan_direct"] = [(A, z, w, c) for A in (20, 4) for z in ZPOS for w in WAVES for c in CELLS]
    g["plan_sliced"] = [(A, z, w, wl, c, cap) for A in (20, 4) for z in ZPOS for w in WAVES for wl in (8, 12)
                        for c in CELLS for cap in CAPS]
    # A, d, pair rows, zpos, waves, rw_words, -i, chunk_cap, record tiles, V + J genes (0: -g), off_cr
    g["plan_rows"] = [(A, d, pairs, z, w, rw, ind, cap, rec, genes, OFF_CR)
                      for A in (20, 4) for d, pairs in ((1, 0), (1, 1), (2, 0)) for z in ZPOS for w in WAVES
                      for rw in (1, 640) for ind in ((0, 1) if d == 1 else (0,)) for cap in CAPS
                      for rec, genes in ((0, 0), (0, 73), (1, 0), (1, 73), (2, 8000))]
    g["plan_pairs2"] = [(z, nbuf, rw, c, cap) for z in ZPOS + (24, 150) for nbuf in (1, 2) for rw in (1, 32, 640)
                        for c in CELLS for cap in CAPS]
    g["plan_resolve"] = [(c,) for c in CELLS + (1600,)]
    g["est_sliced"] = [(A, z, swl) for A in (20, 4) for z in ZPOS for swl in (8, 12, 13)]
    g["est_rows"] = [(A, z, w, rw) for A in (20, 4) for z in ZPOS + (24, 150) for w in (4, 16) for rw in (0, 32, 640)]
    g["est_pairs2"] = [(z, nbuf, rw) for z in ZPOS + (24, 150) for nbuf in (0, 1, 2) for rw in (0, 32, 640)]
    return g


# The program evaluates the maps at make_plan's arguments (plan_*: restated here from compairr_hip.hip -- a wrong
# argument THERE is caught only by tests/test_lds_decisions_gpu.py, at its lengths) and the index build's estimates
# (est_*: the functions of lds_map.h that cmpr_build_reference itself calls).  Prints `bytes offset ...` per line.
PROGRAM = r"""
#include "lds_map.h"
#include <iostream>
#include <sstream>
#include <string>
using namespace cmpr;
template <typename... T> static void put(uint64_t bytes, T... offsets)
{
  std::cout << bytes;
  ((std::cout << ' ' << (uint64_t)offsets), ...);
  std::cout << '\n';
}
int main()
{
  put(sizeof(WaveQueue), sizeof(CandQueue), sizeof(RingSlot), sizeof(P2Slot), sizeof(TileRef), LDS_BYTES);
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string f;
    in >> f;
    uint32_t v[16] = {0};
    for (int n = 0; n < 16 && (in >> v[n]); n++) { }
    if (f == "plan_direct") {
      const DirectLds m = direct_lds_map(v[0], v[1], v[2], v[3]);
      put(m.bytes, m.zl, m.mat, m.queues);
    } else if (f == "plan_resolve") {
      const ResolveLds m = resolve_lds_map(4, v[0]);
      put(m.bytes, m.queues, m.mat);
    } else if (f == "plan_sliced") {
      const SlicedLds m = sliced_lds_map(v[0], v[1], v[2], v[3], v[4], v[5]);
      put(m.bytes, m.slice, m.zl, m.ze, m.mat, m.queues, m.cr, m.hv, m.bcast, m.tref);
    } else if (f == "plan_rows") {
      const RowsLds m = rows_lds_map(v[0], zs_of((int)v[0], v[1] == 2 ? 2 : 1, v[2] != 0), v[3], v[4], v[5], v[6] != 0,
                                     v[7], v[8] && v[9] ? v[9] : 0u, v[8] && v[6] ? v[10] : 0u);
      put(m.bytes, m.slices, m.zl, m.queues, m.cr, m.hv, m.ring, m.tref, m.gk, m.cb);
    } else if (f == "plan_pairs2") {
      const Pairs2Lds m = pairs2_lds_map(v[0], 16, v[1], v[2], v[3], v[4]);
      put(m.bytes, m.slices, m.ze, m.pz, m.mat, m.queues, m.cr, m.slots, m.tref);
    } else if (f == "est_sliced") {
      put(sliced_lds_estimate(v[0], v[1], v[2]));
    } else if (f == "est_rows") {
      put(rows_lds_estimate(v[0], v[1], v[2], v[3]));
    } else if (f == "est_pairs2") {
      put(pairs2_lds_estimate(v[0], v[1], v[2]));
    } else {
      return 1;
    }
  }
  return 0;
}
"""


def region_sizes(formula, a, sz):
    """[(name, bytes, alignment)] in the documented order, worked out here from the arguments alone"""
    wq, cq, ring, p2, tref = sz
    if formula == "plan_direct":
        A, z, w, c = a
        return [("zl", A * z * 8, 8), ("mat", c * 8, 8), ("queues", w * wq, 8)]
    if formula == "plan_resolve":
        return [("queues", 4 * cq, 8), ("mat", a[0] * 8, 8)]
    if formula == "plan_sliced":
        A, z, w, wl, c, cap = a
        return [("slice", 8 << wl, 16), ("zl", (4 if A == 4 else 2 * A) * z * 8, 8), ("ze", (16 if A == 4 else 0) * z * 8, 8),
                ("mat", c * 8, 8), ("queues", w * wq, 8), ("cr", 8 * A * 4, 4), ("hv", 2048 * 4, 4), ("bcast", 16, 4),
                ("tref", cap * tref, 4)]
    if formula == "plan_rows":
        A, d, pairs, z, w, rw, ind, cap, rec, genes, off_cr = a
        zs = 2 * A if d == 2 else A + 1 if pairs else A
        gk, cw = (genes if rec else 0), (off_cr if rec and ind else 0)
        return [("slices", 4 * rw * 32, 16), ("zl", zs * z * 8, 8), ("queues", w * wq, 8), ("cr", 8 * A * 4, 4),
                ("hv", 2048 * 4 if ind else 0, 4), ("ring", 4 * ring, 8), ("tref", 4 * cap * tref, 8), ("gk", gk * 8, 8),
                ("cb", cw * 4, 4)]
    z, nbuf, rw, c, cap = a
    return [("slices", nbuf * rw * 32, 16), ("ze", 16 * z * 8, 8), ("pz", 20 * ((z + 1) // 2) * 8, 8), ("mat", c * 8, 8),
            ("queues", 16 * wq, 8), ("cr", 8 * 4 * 4, 4), ("slots", 2 * p2, 4), ("tref", 2 * cap * tref, 8)]


def arguments_digest(tuples):
    """(the fixture holds the totals in the grid's order, and this digest of the arguments they belong to)"""
    return hashlib.sha256(json.dumps([list(a) for a in tuples]).encode()).hexdigest()


@functools.lru_cache(maxsize=None)
def evaluated(tmp):
    """(struct sizes, {formula: [[bytes, offsets ...] per argument tuple]}) from the program built with g++"""
    src, exe = os.path.join(tmp, "lds_map_grid.cc"), os.path.join(tmp, "lds_map_grid")
    with open(src, "w") as fh:
        fh.write(PROGRAM)
    p = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, src, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    g = grid()
    text = "".join("%s %s\n" % (f, " ".join(str(x) for x in a)) for f in g for a in g[f])
    r = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [[int(x) for x in line.split()] for line in r.stdout.decode().splitlines()]
    rows = iter(lines[1:])
    return tuple(lines[0]), {f: [next(rows) for _ in g[f]] for f in g}


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    return evaluated(str(tmp_path_factory.mktemp("lds_map")))


def test_struct_sizes_and_the_constant(maps):
    assert maps[0] == (3072, 3072, 40, 32, 32, LDS_BYTES)


@pytest.mark.parametrize("formula", sorted(f for f in grid() if f.startswith("plan_")))
def test_regions_back_to_back_aligned_and_bytes_is_the_end(maps, formula):
    sizes, out = maps
    for a, row in zip(grid()[formula], out[formula]):
        total, offsets = row[0], row[1:]
        regions = region_sizes(formula, a, sizes[:5])
        assert len(offsets) == len(regions)
        at = 0
        for (name, size, align), off in zip(regions, offsets):
            assert off == at, (formula, a, name)
            assert off % align == 0, (formula, a, name, off)
            at += size
        assert offsets[0] == 0                     # the slices at address 0
        assert total == at, (formula, a)


def test_tile_references_at_16_bytes_where_the_tables_are_even(maps):
    _, out = maps
    for formula, table_even in (("plan_rows", lambda a: (a[3] * (2 * a[0] if a[1] == 2 else a[0] + a[2])) % 2 == 0),
                                ("plan_pairs2", lambda a: a[3] % 2 == 0)):
        seen = 0
        for a, row in zip(grid()[formula], out[formula]):
            if table_even(a):
                tref = row[-3] if formula == "plan_rows" else row[-1]
                assert tref % 16 == 0, (formula, a)
                seen += 1
        assert seen


def test_totals_equal_the_recorded_host_formulas(maps):
    with open(FIXTURE) as fh:
        recorded = json.load(fh)
    g, (_, out) = grid(), maps
    assert recorded["library_commit"]
    assert sorted(recorded["bytes"]) == sorted(g)
    for f in g:
        assert recorded["arguments_sha256"][f] == arguments_digest(g[f]), f
        assert [row[0] for row in out[f]] == recorded["bytes"][f], f


def test_grid_crosses_48k_and_the_lds(maps):
    """every formula with a Zobrist table is evaluated below 48 KiB, between that and LDS_BYTES, and beyond
    (the pair kernel's sixteen wave queues alone are 48 KiB: it starts above)"""
    _, out = maps
    for f in out:
        totals = [row[0] for row in out[f]]
        if f != "plan_resolve":
            assert min(totals) <= 48 * 1024 or "pairs2" in f, f
            assert any(48 * 1024 < t <= LDS_BYTES for t in totals) and max(totals) > LDS_BYTES, f


def test_one_literal_of_the_lds_size_in_csrc():
    hits = [(name, n) for name in sorted(os.listdir(CSRC)) for n, line in enumerate(open(os.path.join(CSRC, name)), 1)
            if "160 * 1024" in line]
    assert len(hits) == 1 and hits[0][0] == "lds_map.h", hits

