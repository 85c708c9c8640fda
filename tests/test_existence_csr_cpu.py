"""The -x table as CSR without a GPU: the helper that turns the oracle's dense -x matrix into the CSR the GPU tests
compare against (tests/_existence.py), the oracle's figures for the inputs those tests use, the yardstick a second
way, and the header, the binding and the library carrying the two entry points."""

import ctypes
import os
import re

import numpy as np
import pytest

import _existence
import _neighbors
from compairr_amd import hip

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "compairr_hip.h")


def test_csr_of_a_hand_written_matrix():
    m = np.array([[0, 5, 0, 7],
                  [0, 0, 0, 0],
                  [9, 0, 0, 0],
                  [1, 2, 3, 4]], dtype=np.uint64)
    row_start, rep, val = _existence.csr_of_dense(m)
    assert row_start.dtype == np.uint64 and row_start.tolist() == [0, 2, 2, 3, 7]
    assert rep.dtype == np.uint32 and rep.tolist() == [1, 3, 0, 0, 1, 2, 3]
    assert val.dtype == np.uint64 and val.tolist() == [5, 7, 9, 1, 2, 3, 4]
    _existence.assert_is_cell_csr(row_start, rep, val, 4, 4)
    assert _existence.shape_of(row_start) == (7, 4, 0, 1)
    row_start, rep, val = _existence.csr_of_dense(np.zeros((2, 3), dtype=np.uint64))
    assert row_start.tolist() == [0, 0, 0] and len(rep) == 0 and len(val) == 0
    _existence.assert_is_cell_csr(row_start, rep, val, 2, 3)


def test_the_helper_refuses_disorder_and_zeros():
    u64, u32 = (lambda *x: np.array(x, dtype=np.uint64)), (lambda *x: np.array(x, dtype=np.uint32))
    with pytest.raises(AssertionError, match="strictly"):
        _existence.assert_is_cell_csr(u64(0, 2, 3), u32(5, 5, 1), u64(1, 1, 1), 2, 6)
    with pytest.raises(AssertionError, match="zero"):
        _existence.assert_is_cell_csr(u64(0, 2, 3), u32(4, 5, 1), u64(1, 0, 1), 2, 6)
    # a smaller repertoire at the start of the next row is no disorder
    _existence.assert_is_cell_csr(u64(0, 2, 3), u32(4, 5, 1), u64(1, 1, 1), 2, 6)


@pytest.mark.parametrize("name", list(_existence.SMALL))
def test_oracle_figures_of_the_small_inputs(name):
    """what the GPU tests rely on: the stated edges and cell shapes, every listed cell nonzero, and every edge in
    a listed cell (the sum of the cells under ignore_counts is the number of edges)"""
    s1, s2 = _existence.small_sets(name)
    assert s2.n_repertoires == _existence.SMALL[name][2]
    want = _existence.small_want(name)
    _existence.assert_is_cell_csr(*want, s1.n, s2.n_repertoires)
    assert (_existence.small_edges(name),) + _existence.shape_of(want[0]) == _existence.SMALL[name][4]
    per_pair = _existence.small_want(name, ignore_counts=True)
    assert np.array_equal(per_pair[0], want[0]) and np.array_equal(per_pair[1], want[1])
    assert int(per_pair[2].sum()) == _existence.small_edges(name)


@pytest.mark.parametrize("n_rep,d", list(_existence.HUB_ROWS))
def test_oracle_figures_of_the_long_row(n_rep, d):
    s1, s2 = _existence.hub_sets(n_rep)
    hits, cells = _existence.HUB_ROWS[n_rep, d]
    edges = _neighbors.oracle_csr(s1, s2, _existence.hub_options(d))[0]
    assert np.diff(edges.astype(np.int64)).tolist() == hits + [0] * 61
    want = _existence.hub_want(n_rep, d)
    _existence.assert_is_cell_csr(*want, s1.n, n_rep)
    assert np.diff(want[0].astype(np.int64)).tolist() == cells + [0] * 61
    if n_rep == 3:
        assert int(want[2].sum()) == sum(hits)           # (every count is 1)


@pytest.mark.parametrize("more", [dict()] + _existence.OTHER_SCORES, ids=lambda m: "-".join(map(str, m.values())) or "product")
def test_the_dense_matrix_equals_the_neighbour_lists_reduced_by_repertoire(more):
    name = _existence.SCORES_CASE
    s1, s2 = _existence.small_sets(name)
    opt = _existence.small_options(name, **more)
    assert np.array_equal(_existence.oracle_cells(s1, s2, opt), _existence.cells_of_neighbors(s1, s2, opt))


def test_the_two_yardsticks_agree_on_the_long_row_with_counts():
    s1, s2 = _existence.hub_sets(_existence.HUB_REPS)
    opt = _existence.hub_options(2)
    assert np.array_equal(_existence.oracle_cells(s1, s2, opt), _existence.cells_of_neighbors(s1, s2, opt))


@pytest.mark.parametrize("n_rep", _existence.EDGE_REPS)
def test_oracle_figures_of_the_rows_at_the_thresholds(n_rep):
    s1, s2 = _existence.edge_sets(n_rep)
    opt = _neighbors.edge_options()
    assert s2.n_repertoires == n_rep
    edges = _neighbors.oracle_csr(s1, s2, opt)[0]
    assert np.diff(edges.astype(np.int64)).tolist() == _neighbors.EDGE_ROWS + [0] * 61
    want = _existence.edge_want(n_rep)
    _existence.assert_is_cell_csr(*want, s1.n, n_rep)
    second = _existence.csr_of_dense(_existence.cells_of_neighbors(s1, s2, opt))
    for a, b in zip(want, second):
        assert np.array_equal(a, b)
    if n_rep == 1:
        assert np.diff(want[0].astype(np.int64)).tolist() == [0] + [1] * 8 + [0] * 61


def test_header_binding_and_library_carry_the_entry_points():
    with open(HEADER) as fh:
        text = fh.read()
    lib = ctypes.CDLL(hip.library_path())
    for name in ("cmpr_existence_csr", "cmpr_existence_csr_device"):
        assert re.search(r"^int %s\(cmpr_context \*ctx, uint64_t capacity,$" % name, text, re.M), name
        assert name in hip.EXPORTS
        assert hasattr(lib, name), name
    for name in ("edges", "group", "count", "reduce", "copy"):
        assert '"existence_%s_us"' % name in text
    assert "#define CMPR_ABI_VERSION 5" in text
    assert lib.cmpr_abi_version() == 5
