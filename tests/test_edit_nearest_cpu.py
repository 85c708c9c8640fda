"""The nearest neighbour under edit distance without a GPU: the brute force of the definition (tests/_edit_nearest.py)
against the pair list of tests/_edit.py reduced by _nearest.from_pairs, at every cap the pair list reaches; the figures
of the inputs; the hand-written length-gap case, also through a model of the walk by increasing gap with the right and
with the wrong stop; and the header, the binding and the library carrying the two entry points."""

import ctypes
import os
import re

import numpy as np
import pytest

import _edit
import _edit_nearest
import compairr_amd
from compairr_amd import HipOverlap, hip

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "compairr_hip.h")
NAMES = ("cmpr_edit_nearest", "cmpr_edit_nearest_device")
NONE32, NONE16 = _edit_nearest.NONE32, _edit_nearest.NONE16


def assert_same(got, want, why=None):
    for g, w, t in zip(got, want, (np.uint32, np.uint16, np.uint32)):
        assert g.dtype == t and g.shape == w.shape, why
        assert g.tobytes() == w.tobytes(), why


@pytest.mark.parametrize("name", ["nt", "aa", "min0"])
@pytest.mark.parametrize("g", [False, True], ids=["genes", "g"])
@pytest.mark.parametrize("floor", [0, 1])
@pytest.mark.parametrize("cap", [1, 3])
def test_brute_force_against_the_pair_list(name, g, floor, cap):
    """all three arrays, the "none" entries included: `aa` is one set, `min0` has empty sequences"""
    want = _edit_nearest.want(name, g, floor, cap)
    assert_same(_edit_nearest.from_want(name, cap, g, floor), want)
    none = want[2] == 0
    assert (want[0][none] == NONE32).all() and (want[1][none] == NONE16).all() and (want[0][~none] != NONE32).all()
    assert int(want[1][~none].max()) <= cap and (floor == 0 or int(want[1].min()) >= 1)


def test_shapes_of_the_inputs():
    s1, s2 = _edit.aa_sets()
    assert s1 is s2
    assert all(int((s.lengths == 0).sum()) > 0 for s in _edit.min0_sets())
    # one-set mode: nobody is its own neighbour, also at floor 0
    assert (_edit_nearest.want("aa", True, 0, None)[0] != np.arange(s1.n)).all()
    # ... and with the flag every neighbour comes from another repertoire
    other = _edit_nearest.want("aa", True, 0, None, True)
    found = other[2] > 0
    assert (s1.repertoire[other[0][found].astype(np.int64)] != s1.repertoire[found]).all()
    assert not np.array_equal(other[0], _edit_nearest.want("aa", True, 0, None)[0])


@pytest.mark.parametrize("case", _edit_nearest.CASES, ids=_edit_nearest.IDS)
def test_figures_of_the_inputs(case):
    name, g, floor, cap = case
    assert _edit_nearest.figures(_edit_nearest.want(name, g, floor, cap)) == _edit_nearest.FIGURES[case]


def test_the_figures_cover_the_inputs():
    assert set(_edit_nearest.FIGURES) == {(name, g, floor, cap) for name in ("nt", "aa", "min0") for g in (False, True)
                                          for floor in (0, 1) for cap in (1, 3, None)}
    # the edit distance sees what the Hamming distance cannot: uncapped nobody is without a neighbour
    assert all(v[0] == 0 for k, v in _edit_nearest.FIGURES.items() if k[3] is None)


def walk_by_gap(set1, set2, stops):
    """a model of the walk: per query the set-2 sequences of its V by groups of one length in order of the length gap
    (the shorter first), (best, smallest number, ties) kept as the kernel's sink keeps them, the walk left in front of
    the first gap g for which stops(best, g)"""
    dist = _edit_nearest.all_distances(set1, set2)
    out = []
    for i in range(set1.n):
        L = int(set1.lengths[i])
        best, bid, ties = None, NONE32, 0
        lengths = sorted(set(set2.lengths.tolist()), key=lambda n: (abs(n - L), n))
        for n in lengths:
            if best is not None and stops(best, abs(n - L)):
                break
            for j in np.nonzero((set2.lengths == n) & (set2.v_gene == set1.v_gene[i]))[0].tolist():
                dd = int(dist[i, j])
                if best is None or dd < best:
                    best, bid, ties = dd, j, 1
                elif dd == best:
                    bid, ties = min(bid, j), ties + 1
        out.append((bid, NONE16 if best is None else best, ties))
    return out


def test_the_hand_written_length_gap_case():
    s1, s2, want = _edit_nearest.hand()
    assert_same(_edit_nearest.brute(s1, s2, False, 0, None), want)
    assert [a.tolist() for a in want] == [[0, 5, 6], [1, 1, 2], [3, 1, 1]]
    # the candidates of query 0 in number order: one longer, one shorter, one of its own length, and one far away
    assert _edit_nearest.all_distances(s1, s2)[0, :4].tolist() == [1, 1, 1, 8]
    assert s2.lengths[:3].tolist() == [5, 3, 4] and int(s1.lengths[0]) == 4
    # query 1: its own length at 2, a group one residue longer at 1; query 2: the empty sequence alone
    d = _edit_nearest.all_distances(s1, s2)
    assert (int(d[1, 4]), int(d[1, 5])) == (2, 1) and s2.lengths[4:].tolist() == [4, 5, 0] and int(d[2, 6]) == 2
    # the walk by gap that stops when best < g is the definition; one that stops at best <= g is not, on query 0
    right = walk_by_gap(s1, s2, lambda best, g: best < g)
    assert right == [tuple(int(a[i]) for a in want) for i in range(3)]
    wrong = walk_by_gap(s1, s2, lambda best, g: best <= g)
    assert wrong[0] == _edit_nearest.HAND_WRONG_STOP and wrong[0] != right[0]
    # capped at 1 and with a floor of 2: the cap and the floor are part of the candidate rule
    assert [a.tolist() for a in _edit_nearest.brute(s1, s2, False, 0, 1)] == [[0, 5, NONE32], [1, 1, NONE16], [3, 1, 0]]
    assert [a.tolist() for a in _edit_nearest.brute(s1, s2, False, 2, None)] == [[3, 4, 6], [8, 2, 2], [1, 1, 1]]


def test_header_binding_and_library_carry_the_entry_points():
    with open(HEADER) as fh:
        text = fh.read()
    lib = ctypes.CDLL(hip.library_path())
    for name in NAMES:
        assert re.search(r"^int %s\(cmpr_context \*ctx, const cmpr_set_view \*(d_)?set1, "
                         r"const cmpr_set_view \*(d_)?set2,$" % name, text, re.M), name
        assert name in hip.EXPORTS
        assert hasattr(lib, name), name
        assert hip._argtypes()[name] == hip._argtypes()["cmpr_edit_nearest"]
    assert "cmpr_edit_nearest*" in text.split("#define CMPR_ABI_VERSION")[0]
    # cmpr_hamming_nearest's arguments with max_distance behind min_distance
    plain = hip._argtypes()["cmpr_hamming_nearest"]
    assert hip._argtypes()["cmpr_edit_nearest"] == plain[:4] + [ctypes.c_int64] + plain[4:]
    assert "#define CMPR_ABI_VERSION 5" in text and lib.cmpr_abi_version() == 5
    assert "max_distance cannot be negative" in text and '"edit_nearest_prune"' in text
    assert callable(HipOverlap.edit_nearest) and callable(HipOverlap.edit_nearest_device)
    assert callable(compairr_amd.edit_nearest)
