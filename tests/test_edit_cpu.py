"""The edit-distance path without a GPU: the figures of the inputs the GPU tests use, from the numpy brute force
(tests/_edit.py); the brute force against the oracle's pair list at d = 1 with indels and against numpy Hamming
distances; the one place where Levenshtein and the reference's -d 1 -i part; a hand-written case; the hand-built sets
at the word edges; and the header, the binding and the library carrying the four entry points."""

import ctypes
import os
import re

import numpy as np
import pytest

import _edit
import _hamming
import _neighbors
import _oracle
import compairr_amd
from compairr_amd import HipOverlap, hip

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "compairr_hip.h")
SOURCE = os.path.join(HERE, "..", "compairr_amd", "csrc", "allpairs.h")      # (the limit of edit.hip and tcrdist.hip)
NAMES = ("cmpr_edit_neighbors", "cmpr_edit_neighbors_device", "cmpr_edit_matrix", "cmpr_edit_matrix_device")
KEYS = list(_edit.EDGES)
IDS = ["%s-d%d%s" % (k[0], k[1], "-g" if k[2] else "") for k in KEYS]


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_figures_of_the_inputs(key):
    name, d, g = key
    s1, s2 = _edit.sets_of(name)
    row_start, hits, dist = _edit.want(name, d, g)
    assert int(row_start[-1]) == len(hits) == _edit.EDGES[key]
    assert dist.dtype == np.uint16 and int(dist.max()) <= d
    if key in _edit.HISTOGRAMS:
        assert _edit.histogram(dist, d) == _edit.HISTOGRAMS[key]
    if key in _edit.LONGEST_ROW:
        assert _neighbors.shape_of(row_start)[1] == _edit.LONGEST_ROW[key]
    if key in _edit.CROSS_LENGTH:
        assert _edit.cross_length(s1, s2, row_start, hits) == _edit.CROSS_LENGTH[key]
    if d == 1:
        opt = _edit.options_of(name, g, differences=1, indels=True)
        assert _oracle.overlap(s1, s2, opt)[1].matches == _edit.EDGES[key]


def test_shapes_of_the_inputs():
    """the -g rows of `aa` exceed a wave; both `nt` sets and `aa` start above the empty sequence; `min0` has them"""
    assert _neighbors.shape_of(_edit.want("aa", 3, True)[0])[2] > 0
    for name in ("nt", "aa"):
        assert min(int(s.lengths.min()) for s in _edit.sets_of(name)) >= 1
    assert all(int((s.lengths == 0).sum()) > 0 and int((s.lengths == 1).sum()) > 0 for s in _edit.min0_sets())
    s1, s2 = _edit.long_row_sets()
    assert (s1.n, s2.n) == (70, 9001) and s1.n * s2.n == _edit.LONG_ROW_EDGES
    assert sorted(set(s2.lengths.tolist())) == [7, 8, 9]


@pytest.mark.parametrize("name", ["nt", "aa"])
@pytest.mark.parametrize("g", [False, True], ids=["genes", "g"])
def test_brute_force_is_the_oracle_with_indels_at_d1(name, g):
    s1, s2 = _edit.sets_of(name)
    row_start, hits, dist = _edit.want(name, 1, g)
    opt = _edit.options_of(name, g, differences=1, indels=True)
    rows, want_hits = _neighbors.oracle_csr(s1, s2, opt)
    assert np.array_equal(row_start, rows) and np.array_equal(hits, want_hits)
    # on the edges of one length the distance is the number of differing positions; across lengths it is 1
    same = s1.lengths[_edit.queries_of(row_start)] == s2.lengths[hits.astype(np.int64)]
    plain = _hamming.brute_csr(s1, s2, 1, g)
    assert int(same.sum()) == len(plain[1]) and np.array_equal(hits[same], plain[1])
    assert np.array_equal(dist[same], plain[2]) and (dist[~same] == 1).all()
    assert np.array_equal(_hamming.distances(s1, s2, plain[0], plain[1]), plain[2])


@pytest.mark.parametrize("g", [False, True], ids=["genes", "g"])
def test_levenshtein_and_the_reference_part_at_one_residue_against_none(g):
    """variants.cc:301 generates no deletion from a sequence of one residue: the oracle lacks exactly the pairs
    (query of length 1, empty reference), and has every other Levenshtein pair"""
    s1, s2 = _edit.min0_sets()
    row_start, hits, dist = _edit.brute_csr(s1, s2, 1, g)
    opt = _edit.options(ignore_genes=g, differences=1, indels=True)
    oracle = _oracle.pairs(s1, s2, opt)
    assert (len(hits), len(oracle)) == _edit.MIN0[g]
    assert _oracle.overlap(s1, s2, opt)[1].matches == _edit.MIN0[g][1]
    q = _edit.queries_of(row_start)
    odd = (s1.lengths[q] == 1) & (s2.lengths[hits.astype(np.int64)] == 0)
    assert int(odd.sum()) == _edit.MIN0[g][0] - _edit.MIN0[g][1] and (dist[odd] == 1).all()
    kept = np.stack([q[~odd], hits[~odd].astype(np.int64)], axis=1)
    assert np.array_equal(kept, np.asarray(oracle).astype(np.int64))
    # ... while the reverse, an empty query against one residue, is the oracle's too
    assert int(((s1.lengths[q] == 0) & (s2.lengths[hits.astype(np.int64)] == 1)).sum()) > 0


def test_brute_force_on_a_hand_written_case():
    seqs1 = ["CASS", "CAS", "", "WWWW", "ACASS", "C"]
    seqs2 = ["CASS", "CTSA", "", "CAS", "CAWW", "SS"]
    s1, s2 = _edit.hand_set(seqs1, [0] * 6), _edit.hand_set(seqs2, [0, 0, 0, 1, 0, 1])
    want = {  # (i, j): distance, for every pair at distance <= 2
        (0, 0): 0, (0, 1): 2, (0, 3): 1, (0, 4): 2, (0, 5): 2,
        (1, 0): 1, (1, 1): 2, (1, 3): 0, (1, 4): 2, (1, 5): 2,
        (2, 2): 0, (2, 5): 2,
        (3, 4): 2,
        (4, 0): 1, (4, 3): 2,
        (5, 2): 1, (5, 3): 2, (5, 5): 2,
    }
    rows, hits, dist = _edit.brute_csr(s1, s2, 2, ignore_genes=True)
    q = _edit.queries_of(rows)
    assert {(int(a), int(b)): int(c) for a, b, c in zip(q, hits, dist)} == want
    assert rows.tolist() == [0, 5, 10, 12, 13, 15, 18] and dist.dtype == np.uint16
    rows, hits, dist = _edit.brute_csr(s1, s2, 2, ignore_genes=False)
    assert {(int(a), int(b)) for a, b in zip(_edit.queries_of(rows), hits)} == {k for k in want if k[1] not in (3, 5)}
    assert _edit.cross_length(s1, s2, *_edit.brute_csr(s1, s2, 2, True)[:2]) == 18 - 6       # (six pairs of one length)
    m = _edit.matrix_of(s1, s2, rows, hits, _edit.options())
    assert m.shape == (1, 1) and int(m[0, 0]) == len(hits)
    assert _edit.same_genes_pairs(s1, s2, True) == 36 and _edit.same_genes_pairs(s1, s2, False) == 24
    assert _edit.block_distances(np.zeros((1, 0), dtype=np.uint8), np.zeros((1, 3), dtype=np.uint8)).tolist() == [[3]]
    assert _edit.block_distances(np.zeros((1, 3), dtype=np.uint8), np.zeros((1, 0), dtype=np.uint8)).tolist() == [[3]]


@pytest.mark.parametrize("nucleotides", [False, True], ids=["aa", "nt"])
def test_sets_at_the_word_edges(nucleotides):
    """every base length is there with its edits; an edited sequence lies no further from its base than its number
    of operations, the unedited one at 0; no sequence is longer than the limit; at d = 0 .. 3 the Hamming brute force
    gives a subset with distances no smaller"""
    s1, s2, ops, base_of = _edit.edge_sets(nucleotides)
    assert s2.lengths.tolist() == list(_edit.EDGE_LENGTHS) and max(s1.longest, s2.longest) == _edit.MAX_LEN
    assert {0, 1, 2, 3, 4} == set(ops.tolist()) and int(s1.lengths.min()) == 0
    rows, hits, dist = _edit.edge_want(nucleotides)
    rows = rows.astype(np.int64)
    found = 0
    for i, (k, j) in enumerate(zip(ops.tolist(), base_of.tolist())):
        row = hits[rows[i]:rows[i + 1]].tolist()
        if k <= _edit.EDGE_D:
            assert j in row
        if j in row:
            found += 1
            assert int(dist[rows[i] + row.index(j)]) <= k and (k > 0 or int(dist[rows[i] + row.index(j)]) == 0)
    assert found >= int((ops <= _edit.EDGE_D).sum())
    assert set(dist.tolist()) == {0, 1, 2, 3}
    plain = _hamming.brute_csr(s1, s2, _edit.EDGE_D, True)
    pairs = {(int(a), int(b)): int(c) for a, b, c in zip(_edit.queries_of(rows), hits, dist)}
    for a, b, c in zip(_edit.queries_of(plain[0]), plain[1], plain[2]):
        assert pairs[(int(a), int(b))] <= int(c)


def test_the_length_limit_of_the_helper_is_the_kernel_s():
    with open(SOURCE) as fh:
        text = fh.read()
    assert re.search(r"constexpr uint32_t PAIRS_MAX_LEN = (\d+);", text).group(1) == str(_edit.MAX_LEN)


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
    assert hip._argtypes()["cmpr_edit_neighbors"] == hip._argtypes()["cmpr_hamming_neighbors"]
    assert hip._argtypes()["cmpr_edit_matrix"] == hip._argtypes()["cmpr_hamming_matrix"]
    assert "variants.cc:301" in text and "cmpr_edit: a sequence of more than 256 residues" in text
    assert "#define CMPR_ABI_VERSION 5" in text
    assert lib.cmpr_abi_version() == 5
    for name in ("edit_stage_refs", "edit_segments", "edit_words", "edit_group_us", "edit_compare_us",
                 "edit_order_us", "edit_copy_us"):
        assert '"%s"' % name in text, name
    for name in ("edit_neighbors", "edit_neighbors_device", "edit_matrix", "edit_matrix_device"):
        assert callable(getattr(HipOverlap, name))
    assert callable(compairr_amd.edit_neighbors) and callable(compairr_amd.edit_matrix)
