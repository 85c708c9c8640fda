"""cmpr_hamming_nearest without a GPU: the figures of the inputs re-derived from the numpy brute force and, up to d,
from the oracle's pair list; the brute force itself on a hand-written case; the header, the binding and the library
carry both names and the ABI version is unchanged.  No expectation comes from the library."""

import ctypes
import os
import re

import numpy as np
import pytest

import _hamming
import _nearest
import compairr_amd
from compairr_amd import hip
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "compairr_hip.h")
NAMES = ["cmpr_hamming_nearest", "cmpr_hamming_nearest_device"]


@pytest.mark.parametrize("case", _nearest.CASES, ids=_nearest.IDS)
def test_the_figures_from_the_brute_force(case):
    name, g, floor, other = case
    got = _nearest.figures(_nearest.want(name, g, floor, other))
    print(case, got)
    none, histogram, sum_ties, max_ties = _nearest.FIGURES[case]
    assert got[:3] == (none, histogram, sum_ties)
    if max_ties is not None:
        assert got[3] == max_ties
    s1, _ = _hamming.sets_of(name)
    assert none + sum(histogram) == s1.n


@pytest.mark.parametrize("name", ["aa", "nt"])
@pytest.mark.parametrize("d", [3, 6])
@pytest.mark.parametrize("g", [False, True], ids=["genes", "g"])
def test_the_oracle_pair_list_agrees_up_to_d(name, d, g):
    one_set = name == "nt"
    for floor in (0, 1):
        for other in ((False, True) if one_set else (False,)):
            full = _nearest.want(name, g, floor, other)
            partial = _nearest.oracle_nearest(name, d, g, floor, other)
            _nearest.assert_agrees_up_to(full, partial, d)
            # the histogram of the issue up to d, from the oracle alone
            near = partial[2] > 0
            want = _nearest.FIGURES[(name, g, floor, other)][1]
            assert np.bincount(partial[1][near].astype(np.int64), minlength=d + 1).tolist() == (want + [0] * d)[:d + 1]


def test_the_flag_is_exercised_on_nt():
    for g, changed in _nearest.NT_FLAG_CHANGES.items():
        plain, flagged = _nearest.want("nt", g, 0, False), _nearest.want("nt", g, 0, True)
        differs = np.zeros(len(plain[0]), dtype=bool)
        for a, b in zip(plain, flagged):
            differs |= a != b
        assert int(differs.sum()) == changed


@pytest.mark.parametrize("nucleotides", [False, True], ids=["aa", "nt"])
def test_edge_sets_by_construction(nucleotides):
    s1, s2, ks = _hamming.edge_sets(nucleotides)
    nearest, distance, ties = _nearest.brute(s1, s2)
    mutant = ks >= 0
    base_of = {int(L): j for j, L in enumerate(s2.lengths)}
    assert np.array_equal(distance[mutant], ks[mutant])
    assert np.array_equal(nearest[mutant], [base_of[int(L)] for L in s1.lengths[mutant]])
    assert (ties[mutant] == 1).all()
    none = ties == 0
    assert not none[mutant].any() and int(none.sum()) == _nearest.EDGE_NONE[nucleotides]
    assert all(int(L) not in base_of for L in s1.lengths[none])


def test_the_brute_force_on_six_sequences():
    s, table = _nearest.six()
    for (g, floor, other), want in table.items():
        got = _nearest.brute(s, s, g, floor, other)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and np.array_equal(a, b), (g, floor, other)
    # two equal but distinct sets: (i, i) is a candidate, at distance 0
    twin = s.subset(np.arange(s.n))
    nearest, distance, ties = _nearest.brute(s, twin, True)
    assert nearest.tolist() == [0, 0, 2, 3, 4, 5] and distance.tolist() == [0] * 6
    assert ties.tolist() == [2, 2, 1, 1, 1, 1]
    # ... and the pair list at d = 1 gives the same up to 1
    rows, hits, dist = _hamming.brute_csr(s, s, 1, True)
    _nearest.assert_agrees_up_to(_nearest.brute(s, s, True, 0), _nearest.from_pairs(s, s, rows, hits, dist, 0), 1)


def test_header_binding_and_library_carry_both_names():
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(hip.library_path())
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in hip.EXPORTS
        assert hasattr(lib, name), name
    assert re.search(r"enum\s*\{\s*CMPR_NEAREST_OTHER_REPERTOIRE\s*=\s*1\s*\}", code)
    assert hip.NEAREST_OTHER_REPERTOIRE == 1
    assert re.search(r"#define\s+CMPR_ABI_VERSION\s+5\b", code) and lib.cmpr_abi_version() == 5
    assert callable(hip.HipOverlap.hamming_nearest) and callable(hip.HipOverlap.hamming_nearest_device)
    assert callable(compairr_amd.hamming_nearest) and "hamming_nearest" in compairr_amd.__all__
    # the header comment cites the group relation like the rest of the family and names the authoritative test
    comment = text[text.index("The nearest neighbour of every sequence"):text.index("int cmpr_hamming_nearest(")]
    assert "overlap.cc:286-359" in comment and "authoritative" in comment
