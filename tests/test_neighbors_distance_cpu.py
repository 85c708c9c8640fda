"""Edge distances without a GPU: the numpy model of the reference's --distance column (tests/_distance.py) against
the reference's own golden pair lists, the oracle's and the model's figures for the inputs the GPU tests use, and
the header, the binding and the library carrying the two entry points."""

import ctypes
import glob
import os
import re

import numpy as np
import pytest

import _distance
import _neighbors
from compairr_amd import hip

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "compairr_hip.h")
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "expected", "p_*dist*.pairs.tsv")))


def test_model_against_the_reference_distance_column():
    """every line of every golden --pairs --distance output: the model on the line's two sequences gives the
    line's distance"""
    assert len(GOLDEN) == 9
    lines, seen = 0, set()
    for path in GOLDEN:
        with open(path) as fh:
            head = fh.readline().rstrip("\n").lstrip("#").split("\t")
            seq = [k for k, name in enumerate(head) if re.fullmatch(r"(junction|junction_aa|cdr3|cdr3_aa)_[12]", name)]
            assert len(seq) == 2 and head[seq[0]].endswith("_1") and head[seq[1]].endswith("_2"), (path, head)
            at = head.index("distance")
            for line in fh:
                f = line.rstrip("\n").split("\t")
                assert _distance.residues_distance(f[seq[0]], f[seq[1]]) == int(f[at]), (path, line)
                seen.add(int(f[at]))
                lines += 1
    assert lines == 849 and seen == {0, 1, 2}


def test_model_on_a_hand_written_csr():
    s1, s2 = _neighbors.hub_sets()
    # query 0 is the hub, query 2 lies at distance 2 of it: against themselves
    got = _distance.edge_distances(s1, s1, np.array([0, 2, 2, 4] + [4] * 61, dtype=np.uint64),
                                   np.array([0, 2, 0, 1], dtype=np.uint32))
    assert got.dtype == np.uint8 and got.tolist() == [0, 2, 2, 3]
    assert _distance.residues_distance("CASS", "CAS") == 1 and _distance.residues_distance("CASS", "CTSA") == 2


@pytest.mark.parametrize("name", list(_distance.FIGURES))
def test_figures_of_the_small_inputs(name):
    row_start, hits, dist = _distance.small_want(name)
    assert len(dist) == len(hits) == int(row_start[-1])
    assert _distance.histogram(dist) == _distance.FIGURES[name], name
    assert int(dist.max()) <= _distance.small_options(name)["differences"]
    if name == "self_d2":
        assert _distance.mixed_rows(row_start, dist) == (476, 1_282, 1_236)
    if name == "nt_d2g":
        assert _neighbors.shape_of(row_start)[:3] == (57_017, 120, 442)


def test_figures_of_the_long_rows():
    row_start, hits, dist = _distance.hub_want(2)
    rows = [_distance.histogram(dist[int(row_start[i]):int(row_start[i + 1])]) for i in range(3)]
    assert rows == [[1, 304, 43_320], [1, 304, 5_415], [1, 38, 893]]
    row_start, hits, dist = _distance.hub_want(1)
    assert _distance.histogram(dist) == [3, 304 + 304 + 38, 0]       # (the d0 and d1 columns of the rows above)


def test_figures_of_the_rows_at_the_thresholds():
    row_start, hits, dist = _distance.edge_want()
    rs = row_start.astype(np.int64)
    assert np.diff(rs).tolist() == _neighbors.EDGE_ROWS + [0] * 61
    rows = [_distance.histogram(dist[rs[i]:rs[i + 1]]) for i in range(len(_neighbors.EDGE_ROWS))]
    assert rows[7] == [0, 44, 8_148] and rows[8] == [0, 56, 8_137]
    for k in range(7):
        assert rows[k] == [0, 0, _neighbors.EDGE_ROWS[k]]


def test_oracle_equals_brute_force_on_the_long_sequences():
    """40 residues: beyond the 36 a query record and the 32 a table record hold"""
    s1, s2 = _distance.long_sets()
    assert s1.n == 3 and s2.n == 3_001 and s1.longest == s2.longest == _distance.LONG_L
    row_start, hits, dist = _distance.long_want()
    brute = _neighbors.hamming_csr(s1, s2, 2)
    assert np.array_equal(row_start, brute[0]) and np.array_equal(hits, brute[1])
    assert set(dist.tolist()) == {0, 1, 2}
    assert all(row_start[i + 1] > row_start[i] for i in range(3))


def test_header_binding_and_library_carry_the_entry_points():
    with open(HEADER) as fh:
        text = fh.read()
    lib = ctypes.CDLL(hip.library_path())
    for name in ("cmpr_neighbors_distance", "cmpr_neighbors_distance_device"):
        assert re.search(r"^int %s\(cmpr_context \*ctx, uint64_t capacity,$" % name, text, re.M), name
        assert name in hip.EXPORTS
        assert hasattr(lib, name), name
    assert "#define CMPR_ABI_VERSION 5" in text
    assert lib.cmpr_abi_version() == 5
