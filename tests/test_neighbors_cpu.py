"""Neighbour lists without a GPU: the helper that turns the oracle's pair list into the CSR the GPU tests
compare against (tests/_neighbors.py), the oracle's figures for the inputs those tests use, and the header, the
binding and the library carrying the two entry points."""

import ctypes
import os
import re

import numpy as np
import pytest

import _neighbors
from compairr_amd import Options, hip

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "compairr_hip.h")


def test_csr_of_a_hand_written_list():
    # query 0: hits 1, 4, 7; query 1: none; query 2: hit 0
    row_start, hits = _neighbors.csr_of_pairs(3, [(0, 1), (0, 4), (0, 7), (2, 0)])
    assert row_start.dtype == np.uint64 and row_start.tolist() == [0, 3, 3, 4]
    assert hits.dtype == np.uint32 and hits.tolist() == [1, 4, 7, 0]
    _neighbors.assert_is_csr(row_start, hits, 3)
    assert _neighbors.shape_of(row_start) == (4, 3, 0, 1)
    row_start, hits = _neighbors.csr_of_pairs(2, np.zeros((0, 2), dtype=np.uint32))
    assert row_start.tolist() == [0, 0, 0] and len(hits) == 0
    _neighbors.assert_is_csr(row_start, hits, 2)


def test_the_helper_refuses_repeated_and_unsorted_pairs():
    with pytest.raises(AssertionError, match="repeats"):
        _neighbors.csr_of_pairs(3, [(0, 1), (0, 1), (2, 0)])
    with pytest.raises(AssertionError, match="sorted"):
        _neighbors.csr_of_pairs(3, [(0, 4), (0, 1)])
    with pytest.raises(AssertionError, match="strictly"):
        _neighbors.assert_is_csr(np.array([0, 2, 3], dtype=np.uint64), np.array([5, 5, 1], dtype=np.uint32), 2)
    # a smaller hit at the start of the next row is no disorder
    _neighbors.assert_is_csr(np.array([0, 2, 3], dtype=np.uint64), np.array([4, 5, 1], dtype=np.uint32), 2)


@pytest.mark.parametrize("name", list(_neighbors.SMALL))
def test_oracle_figures_of_the_small_inputs(name):
    """what the GPU tests rely on: no pair repeats (csr_of_pairs asserts it) and the rows have the stated shapes"""
    got = _neighbors.shape_of(_neighbors.small_want(name)[0])
    for have, stated in zip(got, _neighbors.SMALL[name][3]):
        assert stated is None or have == stated, (name, got)


def test_oracle_equals_brute_force_on_the_long_row():
    s1, s2 = _neighbors.hub_sets()
    for d, rows in ((2, [43_625, 5_720, 932]), (1, [305, 305, 39])):
        want = _neighbors.oracle_csr(s1, s2, Options(differences=d, n_v_genes=1, n_j_genes=1))
        brute = _neighbors.hamming_csr(s1, s2, d)
        assert np.array_equal(want[0], brute[0]) and np.array_equal(want[1], brute[1])
        assert np.diff(want[0].astype(np.int64)).tolist() == rows + [0] * 61


def test_rows_at_the_thresholds_have_the_stated_lengths():
    """no stranger lies in a ball and no ball touches another: the rows are exactly EDGE_ROWS, then 61 empty ones"""
    s1, s2 = _neighbors.edge_rows()
    assert s1.n == 70 and s2.n == sum(_neighbors.EDGE_ROWS) + 1_000
    want = _neighbors.edge_want()
    brute = _neighbors.hamming_csr(s1, s2, 2)
    assert np.array_equal(want[0], brute[0]) and np.array_equal(want[1], brute[1])
    assert np.diff(want[0].astype(np.int64)).tolist() == _neighbors.EDGE_ROWS + [0] * 61


def test_header_binding_and_library_carry_the_entry_points():
    with open(HEADER) as fh:
        text = fh.read()
    lib = ctypes.CDLL(hip.library_path())
    for name in ("cmpr_neighbors", "cmpr_neighbors_device"):
        assert re.search(r"^int %s\(cmpr_context \*ctx, uint64_t capacity,$" % name, text, re.M), name
        assert name in hip.EXPORTS
        assert hasattr(lib, name), name
    assert "#define CMPR_ABI_VERSION 5" in text
    assert lib.cmpr_abi_version() == 5
