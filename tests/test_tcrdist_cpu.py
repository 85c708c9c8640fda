"""cmpr_tcrdist_neighbors / cmpr_tcrdist_matrix without a GPU: the brute force of tests/_tcrdist.py against the worked
examples and the gap-range table of the definition, the pinned edge counts of the inputs the GPU tests share, their
non-vacuity, and the entry points in header, binding and library.  No expectation comes from the library."""

import ctypes
import os
import re

import numpy as np
import pytest

import _edit
import _tcrdist
import compairr_amd
from compairr_amd import HipOverlap, TcrdistParams, hip
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "compairr_hip.h")
SOURCE = os.path.join(ROOT, "compairr_amd", "csrc", "allpairs.h")       # (the limit of edit.hip and tcrdist.hip)
NAMES = ["cmpr_tcrdist_neighbors", "cmpr_tcrdist_neighbors_device", "cmpr_tcrdist_matrix", "cmpr_tcrdist_matrix_device"]

# x, y: (trims (3, 2) FIXED, SLIDING, trims (0, 0) FIXED, SLIDING) with W[a][b] = |a - b| in sets.AA order, penalty 12
EXAMPLES = [
    ("CASSLGQYF", "CASSIGQYF", (2, 2, 2, 2)),
    ("CASSLGQYF", "CASSLGGQYF", (12, 12, 12, 12)),
    ("CASSLGGQYF", "CASSLGQYF", (12, 12, 12, 12)),
    ("CAW", "CAWY", (12, 12, 13, 13)),
    ("", "AC", (24, 24, 24, 24)),
    ("CASSYF", "CASRDTGELYF", (66, 66, 66, 66)),
    ("CASSPGTGGYEQYF", "CASSLGTGAYNEQYF", (53, 28, 53, 28)),
]
# Ls: (FIXED, (SLIDING lo, hi))
GAP_RANGES = {0: (0, (0, 0)), 1: (1, (0, 1)), 2: (1, (1, 1)), 3: (2, (1, 2)), 4: (2, (2, 2)), 5: (3, (2, 3)),
              6: (3, (3, 3)), 7: (4, (3, 4)), 8: (4, (4, 4)), 9: (5, (4, 5)), 10: (5, (5, 5)), 11: (6, (5, 6)),
              12: (6, (5, 7)), 13: (6, (5, 8))}


@pytest.mark.parametrize("x,y,want", EXAMPLES)
def test_worked_examples(x, y, want):
    W = np.abs(np.arange(20)[:, None] - np.arange(20)[None, :])
    got = tuple(_tcrdist.distance(x, y, W, ntrim, ctrim, 12, mode)
                for ntrim, ctrim in ((3, 2), (0, 0)) for mode in (_tcrdist.FIXED, _tcrdist.SLIDING))
    assert got == want


def test_operand_order_is_set_1_then_set_2_whichever_is_shorter():
    W = np.zeros((20, 20), dtype=np.int64)
    W[0, 1] = 7                                             # A of set 1 against C of set 2, not the reverse
    for x, y, want in (("A", "C", 7), ("C", "A", 0), ("AA", "C", 7), ("C", "AA", 0), ("A", "CC", 7), ("CC", "A", 0)):
        assert _tcrdist.distance(x, y, W, 0, 0, 0, _tcrdist.SLIDING) == want, (x, y)


def test_gap_ranges():
    for Ls, (fixed, sliding) in GAP_RANGES.items():
        assert _tcrdist.gap_range(Ls, _tcrdist.FIXED) == (fixed, fixed)
        assert _tcrdist.gap_range(Ls, _tcrdist.SLIDING) == sliding
    for Ls in range(0, 300):
        for mode in (_tcrdist.FIXED, _tcrdist.SLIDING):
            lo, hi = _tcrdist.gap_range(Ls, mode)
            assert 0 <= lo <= hi <= Ls


@pytest.mark.parametrize("key", _tcrdist.KEYS, ids=_tcrdist.IDS)
def test_pinned_edges_and_non_vacuity(key):
    """every run has an edge and fewer than all pairs; every case with a cutoff above 0 has an edge across two
    lengths -- asserted on its -g run, which holds the edges of the run with genes and more (mid, case 2 with genes:
    22 edges, all of one length)"""
    name, case, g = key
    s1, s2 = _tcrdist.sets_of(name)
    rows, hits, dist = _tcrdist.want(name, case, g)
    cutoff = _tcrdist.CASES[case][4]
    assert s1.n * s2.n == _tcrdist.PAIRS
    assert len(hits) == _tcrdist.EDGES[key]
    assert 0 < len(hits) < _tcrdist.PAIRS
    assert int(dist.max()) <= cutoff
    if cutoff > 0:
        rows_g, hits_g, _ = _tcrdist.want(name, case, True)
        assert _edit.cross_length(s1, s2, rows_g, hits_g) > 0


def test_the_inputs_reach_every_short_length():
    s1, s2 = _tcrdist.tiny_sets()
    for s in (s1, s2):
        assert set(range(0, 13)) == set(s.lengths.tolist())
    assert len(_tcrdist.edge_sets()[0].lengths) == len(_tcrdist.edge_sets()[1].lengths)
    assert set(_tcrdist.edge_sets()[0].lengths.tolist()) == set(_tcrdist.EDGE_LENGTHS)


def test_the_length_limit_of_the_helper_is_the_kernel_s():
    with open(SOURCE) as fh:
        text = fh.read()
    assert re.search(r"constexpr uint32_t PAIRS_MAX_LEN = (\d+);", text).group(1) == str(_tcrdist.MAX_LEN)


def test_header_binding_and_library_carry_the_entry_points():
    with open(HEADER) as fh:
        text = fh.read()
    lib = ctypes.CDLL(hip.library_path())
    for name in NAMES:
        assert re.search(r"^int %s\(cmpr_context \*ctx, const cmpr_set_view \*(d_)?set1, "
                         r"const cmpr_set_view \*(d_)?set2,$" % name, text, re.M), name
        assert name in hip.EXPORTS
        assert hasattr(lib, name), name
        assert name.replace("_device", "") + "*" in text.split("#define CMPR_ABI_VERSION")[0]
        assert hip._argtypes()[name] == hip._argtypes()[name.replace("_device", "")]
    assert "#define CMPR_ABI_VERSION 5" in text and lib.cmpr_abi_version() == 5
    assert "cmpr_tcrdist: amino acids only" in text and "cmpr_tcrdist: a sequence of more than 256 residues" in text
    assert re.search(r"enum \{ CMPR_GAP_FIXED = 0, CMPR_GAP_SLIDING = 1 \};", text)
    assert (hip.GAP_FIXED, hip.GAP_SLIDING) == (_tcrdist.FIXED, _tcrdist.SLIDING) == (0, 1)
    assert ctypes.sizeof(hip._TcrdistParams) == 48          # two pointers, four words, four reserved words
    for name in ("tcrdist_stage_refs", "tcrdist_segments", "tcrdist_group_us", "tcrdist_compare_us",
                 "tcrdist_order_us", "tcrdist_copy_us"):
        assert '"%s"' % name in text, name
    for name in ("tcrdist_neighbors", "tcrdist_neighbors_device", "tcrdist_matrix", "tcrdist_matrix_device"):
        assert callable(getattr(HipOverlap, name))
    assert callable(compairr_amd.tcrdist_neighbors) and callable(compairr_amd.tcrdist_matrix)


def test_the_params_holder_validates():
    W = _tcrdist.table()
    p = TcrdistParams(W.astype(np.int64), 4, 3, 2, hip.GAP_SLIDING, v_distance=[[0, 9], [7, 0]])
    assert p.substitution.dtype == np.uint8 and p.v_distance.dtype == np.uint16
    t = p.struct(_tcrdist.options())
    assert (t.gap_penalty, t.ntrim, t.ctrim, t.gap_mode) == (4, 3, 2, 1) and list(t.reserved) == [0, 0, 0, 0]
    assert t.substitution == p.substitution.ctypes.data and t.v_distance == p.v_distance.ctypes.data
    assert TcrdistParams(W, 4).struct(_tcrdist.options()).v_distance is None
    for bad in (W[:19], W[:, :19], W.astype(np.float64), W.astype(np.int64) + 300, W.astype(np.int64) - 1, W[:4, :4]):
        with pytest.raises(ValueError):
            TcrdistParams(bad, 4)
    with pytest.raises(ValueError):
        TcrdistParams(W, 4, v_distance=np.full((2, 2), 70000))
    with pytest.raises(ValueError):
        TcrdistParams(W, -1)
    with pytest.raises(ValueError):
        TcrdistParams(W, 4, v_distance=np.zeros((3, 3), dtype=np.uint16)).struct(_tcrdist.options())
