"""cmpr_existence_csr / cmpr_existence_csr_device on the GPU against the nonzero cells of the oracle's dense -x
matrix (tests/_existence.py), element for element: every row shape and every grouping and reducing path, a row
longer than LDS, the capacity protocol, the device entry point, a repeated step, a reference in parts, what stays
usable afterwards, and the refusals."""

import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import _existence
import _neighbors
import compairr_amd
from _routed import routed_contexts
from compairr_amd import HipError, HipOverlap, Options, RepertoireSet, synth
from test_gpu_parity import LAYOUTS, NT_LAYOUTS

pytestmark = pytest.mark.gpu

CMPR_OK, CMPR_EINVAL, CMPR_EUNSUPPORTED, CMPR_ESTATE = 0, 1, 4, 5
FULL = dict(n_v_genes=synth.N_V, n_j_genes=synth.N_J)
POISON32, POISON64 = 0x25A5A5A5, 0x25A5A5A525A5A5A5


def assert_equal_cells(got, want, n1, n_rep):
    _existence.assert_is_cell_csr(*got, n1, n_rep)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def resident(opt, set1, set2, tunables=None):
    h = HipOverlap(opt)
    for name, value in (tunables or {}).items():
        h.set_tunable(name, value)
    h.set_reference(set2, set1.longest)
    h.set_queries(set1)
    return h


def census(row_start):
    """rows by the number of their HITS, as the paths take them: empty, 1 .. 8 (a lane), 9 .. 64 (a wave),
    65 .. 8192 (a workgroup in LDS), longer (device-wide)"""
    deg = np.diff(row_start.astype(np.int64))
    return [int(((deg > lo) & (deg <= hi)).sum()) for lo, hi in ((-1, 0), (0, 8), (8, 64), (64, 8192), (8192, 1 << 62))]


# ---- 1. small sets, element for element ----

# the layouts tests/test_neighbors_gpu.py uses per alphabet
SMALL_LAYOUTS = [("auto", LAYOUTS["auto"]), ("hbm", LAYOUTS["hbm"]), ("rows_k4_overflow", LAYOUTS["rows_k4_overflow"])]
SMALL_NT_LAYOUTS = [("auto", NT_LAYOUTS["auto"]), ("lds_tiny_k8", NT_LAYOUTS["lds_tiny_k8"]),
                    ("rows_tiny_k5_mixed", NT_LAYOUTS["rows_tiny_k5_mixed"])]
SMALL_CASES = [(name, layout) for name in _existence.SMALL
               for layout in (SMALL_NT_LAYOUTS if _existence.SMALL[name][3].get("nucleotides") else SMALL_LAYOUTS)]


@pytest.mark.parametrize("name,layout", SMALL_CASES, ids=["%s-%s" % (n, l[0]) for n, l in SMALL_CASES])
def test_small_sets_element_for_element(name, layout):
    s1, s2 = _existence.small_sets(name)
    want = _existence.small_want(name)
    assert (_existence.small_edges(name),) + _existence.shape_of(want[0]) == _existence.SMALL[name][4]
    edges = _neighbors.oracle_csr(s1, s2, _existence.small_options(name))[0]
    print("%s %s: rows of 0 | 1-8 | 9-64 | 65-8192 | more hits = %s; cells, most, rows > 64 cells, empty = %s"
          % (name, layout[0], census(edges), _existence.shape_of(want[0])))
    got = compairr_amd.existence_csr(s1, s2, _existence.small_options(name, device=0), layout[1])
    assert_equal_cells(got, want, s1.n, s2.n_repertoires)


@pytest.mark.parametrize("more", _existence.OTHER_SCORES, ids=lambda m: "-".join(map(str, m.values())))
def test_the_other_scores(more):
    name = _existence.SCORES_CASE
    s1, s2 = _existence.small_sets(name)
    want = _existence.small_want(name, **more)
    assert not np.array_equal(want[2], _existence.small_want(name)[2])
    got = compairr_amd.existence_csr(s1, s2, _existence.small_options(name, device=0, **more))
    assert_equal_cells(got, want, s1.n, s2.n_repertoires)


# ---- 2. the long row ----

@pytest.mark.parametrize("n_rep,d", list(_existence.HUB_ROWS))
def test_the_long_row(n_rep, d):
    """Paths are taken by a row's number of hits n (existence.hip: 8, 64, 8192), in both passes.
    d = 2: the row of 43 625 hits is grouped by the device-wide radix sort and reduced by the device-wide
    reduction -- to 3 cells, and to 5 000; the rows of 5 720 and 932 hits are grouped by a workgroup in LDS and
    reduced by it in 23 and 4 rounds of 256 positions, to 3 cells each (runs that cross waves and rounds: all
    sums by atomics) and to 3 404 and 851 (ranks beyond a round).  d = 1: the rows of 305 hits take the LDS path
    (291 / 297 cells: most runs of length one), the row of 39 hits the wave path.  Rows of 1 .. 8 hits (a lane)
    and of 9 .. 64 (a wave), and 429 to 1 164 LDS rows per case, are in test_small_sets_element_for_element,
    whose log lists the census.  Every count is 1 with 3 repertoires, 1 .. 9 with 5 000."""
    s1, s2 = _existence.hub_sets(n_rep)
    hits, cells = _existence.HUB_ROWS[n_rep, d]
    want = _existence.hub_want(n_rep, d)
    assert np.diff(want[0].astype(np.int64)).tolist() == cells + [0] * 61
    with resident(_existence.hub_options(d, device=0), s1, s2) as h:
        got = h.existence_csr()
        assert h.stats().matches == sum(hits)
    assert_equal_cells(got, want, s1.n, n_rep)


@pytest.mark.parametrize("n_rep", _existence.EDGE_REPS)
def test_rows_at_the_thresholds(n_rep):
    """rows of exactly 0, 1, 2, 8, 9, 64, 65, 8192 and 8193 hits (_neighbors.edge_rows), in both passes.  One
    repertoire: one run per row, across every wave and round of the row of 8192 hits; 200: ranks beyond a round."""
    s1, s2 = _existence.edge_sets(n_rep)
    want = _existence.edge_want(n_rep)
    with resident(_neighbors.edge_options(device=0), s1, s2) as h:
        got = h.existence_csr()
        assert h.stats().matches == sum(_neighbors.EDGE_ROWS)
    assert_equal_cells(got, want, s1.n, n_rep)


# ---- 3. the capacity protocol ----

def raw_existence(h, capacity, row_start=None, rep=None, val=None, want_count=True):
    """cmpr_existence_csr as it is declared: (code, n_cells)"""
    n = C.c_uint64(12345)
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = h._lib.cmpr_existence_csr(h._ctx, capacity, ptr(row_start), ptr(rep), ptr(val), C.byref(n) if want_count else None)
    return rc, n.value


def test_capacity_protocol():
    name = "other_d1_r200"
    s1, s2 = _existence.small_sets(name)
    want = _existence.small_want(name)
    cells, n_rep = len(want[1]), s2.n_repertoires
    with resident(_existence.small_options(name, device=0), s1, s2) as h:
        # count only
        assert raw_existence(h, 0) == (CMPR_OK, cells)
        row_start = np.full(s1.n + 1, 7, dtype=np.uint64)
        assert raw_existence(h, 0, row_start) == (CMPR_OK, cells)
        assert np.array_equal(row_start, want[0])
        assert h.stats().matches == _existence.small_edges(name)
        # one short: row_start exact, nothing written to the cells
        row_start[:] = 7
        rep = np.full(cells, POISON32, dtype=np.uint32)
        val = np.full(cells, POISON64, dtype=np.uint64)
        assert raw_existence(h, cells - 1, row_start, rep, val) == (CMPR_OK, cells)
        assert np.array_equal(row_start, want[0])
        assert (rep == POISON32).all() and (val == POISON64).all()
        # exact
        row_start[:] = 7
        assert raw_existence(h, cells, row_start, rep, val) == (CMPR_OK, cells)
        assert_equal_cells((row_start, rep, val), want, s1.n, n_rep)
        # more than enough: what lies behind the cells is not the call's to write
        roomy_rep = np.full(cells + 100, POISON32, dtype=np.uint32)
        roomy_val = np.full(cells + 100, POISON64, dtype=np.uint64)
        assert raw_existence(h, cells + 100, None, roomy_rep, roomy_val) == (CMPR_OK, cells)
        assert np.array_equal(roomy_rep[:cells], want[1]) and (roomy_rep[cells:] == POISON32).all()
        assert np.array_equal(roomy_val[:cells], want[2]) and (roomy_val[cells:] == POISON64).all()
        # refusals of the arguments
        assert raw_existence(h, 5, row_start, None, val)[0] == CMPR_EINVAL
        assert "repertoire_out" in h._lib.cmpr_last_error(h._ctx).decode()
        assert raw_existence(h, 5, row_start, rep, None)[0] == CMPR_EINVAL
        assert "value_out" in h._lib.cmpr_last_error(h._ctx).decode()
        assert raw_existence(h, cells, row_start, rep, val, want_count=False)[0] == CMPR_EINVAL
        assert "n_cells_out" in h._lib.cmpr_last_error(h._ctx).decode()
        assert_equal_cells(h.existence_csr(), want, s1.n, n_rep)


# ---- 4. the device entry point ----

def test_device_entry_point():
    import torch
    name = "self_d1i_r200"
    s1, s2 = _existence.small_sets(name)
    want = _existence.small_want(name)
    cells, n1, n_rep = len(want[1]), s1.n, s2.n_repertoires
    with resident(_existence.small_options(name, device=0), s1, s2) as h:
        host = h.existence_csr()
        d_rows = torch.full((n1 + 1 + 64,), POISON64, dtype=torch.int64, device="cuda")
        d_rep = torch.full((cells + 64,), POISON32, dtype=torch.int32, device="cuda")
        d_val = torch.full((cells + 64,), POISON64, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        # count only; one short; exact
        assert h.existence_csr_device(0, d_rows.data_ptr(), 0, 0) == cells
        assert np.array_equal(d_rows.cpu().numpy().view(np.uint64)[:n1 + 1], want[0])
        assert h.existence_csr_device(cells - 1, d_rows.data_ptr(), d_rep.data_ptr(), d_val.data_ptr()) == cells
        assert (d_rep.cpu().numpy().view(np.uint32) == POISON32).all()
        assert (d_val.cpu().numpy().view(np.uint64) == POISON64).all()
        d_rows.fill_(POISON64)
        torch.cuda.synchronize()
        assert h.existence_csr_device(cells, d_rows.data_ptr(), d_rep.data_ptr(), d_val.data_ptr()) == cells
        rows = d_rows.cpu().numpy().view(np.uint64)
        rep, val = d_rep.cpu().numpy().view(np.uint32), d_val.cpu().numpy().view(np.uint64)
        # the cell arrays alone
        d_rep_only = torch.full((cells + 64,), POISON32, dtype=torch.int32, device="cuda")
        d_val_only = torch.full((cells + 64,), POISON64, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert h.existence_csr_device(cells, 0, d_rep_only.data_ptr(), d_val_only.data_ptr()) == cells
        rep_only, val_only = d_rep_only.cpu().numpy().view(np.uint32), d_val_only.cpu().numpy().view(np.uint64)
    assert_equal_cells(host, want, n1, n_rep)
    assert_equal_cells((rows[:n1 + 1].copy(), rep[:cells].copy(), val[:cells].copy()), host, n1, n_rep)
    assert (rows[n1 + 1:] == POISON64).all() and (rep[cells:] == POISON32).all() and (val[cells:] == POISON64).all()
    assert np.array_equal(rep_only[:cells], host[1]) and (rep_only[cells:] == POISON32).all()
    assert np.array_equal(val_only[:cells], host[2]) and (val_only[cells:] == POISON64).all()


# ---- 5. the repeated step ----

def test_repeated_steps_leave_the_cells_as_they_are():
    """the set-up of test_a_repeated_step_starts_from_clean_degrees_and_cursors (tests/test_neighbors_gpu.py): the
    count step and the fill step of the call overflow without a redo pass and are repeated"""
    a = synth.make_set(40000, 21, prefix="A", pool_size=8000)
    b = synth.make_set(40000, 22, prefix="B", pool_size=8000)
    o = Options(differences=1, **FULL)
    want = _existence.oracle_cell_csr(a, b, o)
    edges = len(_neighbors.oracle_csr(a, b, o)[1])
    with resident(o, a, b, {"variant": 2, "pos_segments": 1, "pos_capacity": 64}) as h:
        n = C.c_uint64()
        h.set_tunable("assume_never_overflows", 1)
        h._check(h._lib.cmpr_existence_csr(h._ctx, 0, None, None, None, C.byref(n)))
        assert n.value == len(want[1])
        assert h.get_tunable("never_overflows") == 0               # withdrawn
        row_start = np.zeros(a.n + 1, dtype=np.uint64)
        rep = np.zeros(n.value, dtype=np.uint32)
        val = np.zeros(n.value, dtype=np.uint64)
        h.set_tunable("assume_never_overflows", 1)
        h._check(h._lib.cmpr_existence_csr(h._ctx, n.value, row_start.ctypes.data, rep.ctypes.data, val.ctypes.data,
                                           C.byref(n)))
        assert h.get_tunable("never_overflows") == 0
        assert h.stats().matches == edges
    assert_equal_cells((row_start, rep, val), want, a.n, b.n_repertoires)


# ---- 6. the reference in parts ----

@functools.lru_cache(maxsize=None)
def big_set():
    return synth.make_set(200_000, 30)


@pytest.mark.parametrize("score", ["product", "max"])
def test_reference_in_parts_gives_the_same_cells(score):
    s = big_set()
    o = Options(differences=1, device=0, score=score, **FULL)
    with resident(dataclasses.replace(o, existence=True), s, s) as dense:
        matrix = dense.overlap_matrix()                          # n x R2 uint64: 25.6 MB
        on_dense = dense.existence_csr()                         # (options.existence plays no part)
    assert matrix.shape == (s.n, s.n_repertoires)
    want = _existence.csr_of_dense(matrix)
    assert len(want[1]) > s.n
    with resident(o, s, s) as h:
        whole = h.existence_csr()
        assert h.get_tunable("reference_parts") == 1
    with resident(o, s, s, {"part_buckets_log2": 17}) as h:
        parts = h.existence_csr()
        assert h.get_tunable("reference_parts") >= 3
    assert_equal_cells(whole, want, s.n, s.n_repertoires)
    assert_equal_cells(parts, whole, s.n, s.n_repertoires)
    assert_equal_cells(on_dense, whole, s.n, s.n_repertoires)


# ---- 7. what stays ----

def test_the_context_is_as_usable_afterwards():
    s = synth.make_set(20_000, 32, pool_size=3000)
    o = Options(differences=1, device=0, **FULL)
    with resident(o, s, s) as fresh:
        matrix, pairs, lists = fresh.overlap_matrix(), fresh.overlap_pairs(), fresh.neighbors()
    want = _existence.oracle_cell_csr(s, s, o)
    with resident(o, s, s) as h:
        one = h.existence_csr()
        assert h.stats().matches == len(pairs)
        assert np.array_equal(h.overlap_matrix(), matrix)
        # pairs and neighbours are listed again: no pointer of the call stays set
        assert np.array_equal(h.overlap_pairs(), pairs)
        again = h.neighbors()
        assert np.array_equal(again[0], lists[0]) and np.array_equal(again[1], lists[1])
        assert np.array_equal(h.overlap_matrix(), matrix)
        two = h.existence_csr()
        assert h.stats().matches == len(pairs)
        for part in ("edges", "group", "count", "reduce", "copy"):
            assert h.get_tunable("existence_%s_us" % part) >= 0
    assert_equal_cells(one, want, s.n, s.n_repertoires)
    for a, b in zip(one, two):
        assert np.array_equal(a, b)


# ---- 8. refusals ----

def test_refusals():
    s1, s2 = _existence.small_sets("other_d1_r200")
    o = _neighbors.tiny_options(differences=1, device=0)
    with HipOverlap(o) as h:
        with pytest.raises(HipError) as want:
            h.overlap_matrix()
        assert want.value.code == CMPR_ESTATE
        for prepare in (lambda: None, lambda: h.set_reference(s2, s1.longest)):
            prepare()
            with pytest.raises(HipError) as e:
                h.existence_csr()
            assert (e.value.code, str(e.value)) == (CMPR_ESTATE, str(want.value))
    with resident(dataclasses.replace(o, score="ratio"), s1, s2) as h:
        with pytest.raises(HipError) as want:
            h.overlap_matrix()
        assert want.value.code == CMPR_EINVAL and "cmpr_overlap_matrix_f64" in str(want.value)
        for call in (h.existence_csr, lambda: h.existence_csr_device(0, 0, 0, 0)):
            with pytest.raises(HipError) as e:
                call()
            assert e.value.code == CMPR_EINVAL and "cmpr_overlap_matrix_f64" in str(e.value)
    with resident(o, s1, s2, {"work_shard_count": 2}) as h:
        for call in (h.existence_csr, lambda: h.existence_csr_device(0, 0, 0, 0)):
            with pytest.raises(HipError) as e:
                call()
            assert e.value.code == CMPR_EUNSUPPORTED and "work_shard_count" in str(e.value)
    (h,) = routed_contexts(s1, s2, o, 1, {})
    with h:
        with pytest.raises(HipError) as e:
            h.existence_csr()
        assert e.value.code == CMPR_EUNSUPPORTED and "cmpr_set_queries_routed" in str(e.value)
        h.overlap_matrix()                      # (the routed set itself is in order)


# ---- 9. nothing to list ----

def test_empty_query_set_and_no_match_at_all():
    z = lambda t: np.zeros(0, dtype=t)
    s2 = _existence.tiny(2500, 6, 200)
    empty = RepertoireSet(z(np.uint8), np.zeros(1, dtype=np.uint64), z(np.uint32), z(np.uint32), z(np.uint32),
                          z(np.uint64), ["T1"])
    with resident(_neighbors.tiny_options(differences=1, device=0), empty, s2) as h:
        row_start = np.full(1, 7, dtype=np.uint64)
        assert raw_existence(h, 0, row_start) == (CMPR_OK, 0)
        assert row_start.tolist() == [0]
        row_start, rep, val = h.existence_csr()
        assert row_start.tolist() == [0] and len(rep) == 0 and len(val) == 0
    # a set 1 whose genes no sequence of set 2 has: no pair at all
    s1 = _existence.tiny(3000, 5, 200)
    strangers = dataclasses.replace(s1, v_gene=np.full(s1.n, 2, dtype=np.uint32))
    o = Options(differences=1, n_v_genes=3, n_j_genes=2, device=0)
    assert len(_neighbors.oracle_csr(strangers, s2, o)[1]) == 0
    with resident(o, strangers, s2) as h:
        import torch
        row_start = np.full(s1.n + 1, 7, dtype=np.uint64)
        assert raw_existence(h, 0, row_start) == (CMPR_OK, 0)
        assert not row_start.any()
        d_rows = torch.full((s1.n + 1,), POISON64, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert h.existence_csr_device(0, d_rows.data_ptr(), 0, 0) == 0
        assert not d_rows.cpu().numpy().any()
        row_start, rep, val = h.existence_csr()
        assert not row_start.any() and len(row_start) == s1.n + 1 and len(rep) == 0 and len(val) == 0
