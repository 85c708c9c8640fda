"""cmpr_neighbors / cmpr_neighbors_device on the GPU against the oracle's pair list as CSR (tests/_neighbors.py),
element for element: every row shape and sorting path, a row longer than LDS, the capacity protocol, the device
entry point, a repeated step, a reference in parts, what stays usable afterwards, and the refusals."""

import ctypes as C
import functools

import numpy as np
import pytest

import _neighbors
import compairr_amd
from _routed import routed_contexts
from compairr_amd import HipError, HipOverlap, Options, RepertoireSet, synth
from test_gpu_parity import LAYOUTS, NT_LAYOUTS

pytestmark = pytest.mark.gpu

CMPR_OK, CMPR_EINVAL, CMPR_EUNSUPPORTED, CMPR_ESTATE = 0, 1, 4, 5
FULL = dict(n_v_genes=synth.N_V, n_j_genes=synth.N_J)
POISON32, POISON64 = 0x25A5A5A5, 0x25A5A5A525A5A5A5


def assert_equal_csr(got, want, n1):
    _neighbors.assert_is_csr(got[0], got[1], n1)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])


def resident(opt, set1, set2, tunables=None):
    h = HipOverlap(opt)
    for name, value in (tunables or {}).items():
        h.set_tunable(name, value)
    h.set_reference(set2, set1.longest)
    h.set_queries(set1)
    return h


# ---- 1. row shapes on small sets ----

# the default layout and two others per case: the table in HBM and the row filter with a positives buffer that
# overflows into the redo pass (amino acids); tiny LDS slices and tiny rows (nucleotides)
SMALL_LAYOUTS = [("auto", LAYOUTS["auto"]), ("hbm", LAYOUTS["hbm"]), ("rows_k4_overflow", LAYOUTS["rows_k4_overflow"])]
SMALL_NT_LAYOUTS = [("auto", NT_LAYOUTS["auto"]), ("lds_tiny_k8", NT_LAYOUTS["lds_tiny_k8"]),
                    ("rows_tiny_k5_mixed", NT_LAYOUTS["rows_tiny_k5_mixed"])]
SMALL_CASES = [(name, layout) for name in _neighbors.SMALL
               for layout in (SMALL_NT_LAYOUTS if _neighbors.SMALL[name][2].get("nucleotides") else SMALL_LAYOUTS)]


@pytest.mark.parametrize("name,layout", SMALL_CASES, ids=["%s-%s" % (n, l[0]) for n, l in SMALL_CASES])
def test_row_shapes_on_small_sets(name, layout):
    s1, s2 = _neighbors.small_sets(name)
    want = _neighbors.small_want(name)
    shape = _neighbors.shape_of(want[0])
    for have, stated in zip(shape, _neighbors.SMALL[name][3]):
        assert stated is None or have == stated
    got = compairr_amd.neighbors(s1, s2, _neighbors.tiny_options(device=0, **_neighbors.SMALL[name][2]), layout[1])
    print("%s %s: edges, longest, rows > 64, empty = %s" % (name, layout[0], shape))
    assert_equal_csr(got, want, s1.n)


# ---- 2. one row longer than LDS ----

@pytest.mark.parametrize("d,rows", [(2, [43_625, 5_720, 932]), (1, [305, 305, 39])])
def test_one_row_longer_than_lds(d, rows):
    """d = 2: the device-wide sort (43 625), the LDS sort (5 720, 932); d = 1: the LDS sort (305) and the wave
    (39).  The oracle equals a numpy Hamming brute force here, and takes 0.1 s."""
    s1, s2 = _neighbors.hub_sets()
    opt = Options(differences=d, n_v_genes=1, n_j_genes=1, device=0)
    want = _neighbors.oracle_csr(s1, s2, opt)
    brute = _neighbors.hamming_csr(s1, s2, d)
    assert np.array_equal(want[0], brute[0]) and np.array_equal(want[1], brute[1])
    assert np.diff(want[0].astype(np.int64)).tolist() == rows + [0] * 61
    assert_equal_csr(compairr_amd.neighbors(s1, s2, opt), want, s1.n)


def test_rows_at_the_thresholds():
    """rows of exactly 0, 1, 2, 8, 9, 64, 65, 8192 and 8193 hits: either side of every length at which the sorting
    path changes (csr_rows.h), the rows of 9 and 64 hits in one wave"""
    s1, s2 = _neighbors.edge_rows()
    want = _neighbors.edge_want()
    assert np.diff(want[0].astype(np.int64)).tolist() == _neighbors.EDGE_ROWS + [0] * 61
    assert_equal_csr(compairr_amd.neighbors(s1, s2, _neighbors.edge_options(device=0)), want, s1.n)


# ---- 3. the capacity protocol ----

def raw_neighbors(h, capacity, row_start=None, hits=None, want_count=True):
    """cmpr_neighbors as it is declared: (code, n_edges)"""
    n = C.c_uint64(12345)
    rc = h._lib.cmpr_neighbors(h._ctx, capacity, None if row_start is None else row_start.ctypes.data,
                               None if hits is None else hits.ctypes.data, C.byref(n) if want_count else None)
    return rc, n.value


def test_capacity_protocol():
    name = "other_d1"
    s1, s2 = _neighbors.small_sets(name)
    want = _neighbors.small_want(name)
    edges = len(want[1])
    with resident(_neighbors.tiny_options(device=0, **_neighbors.SMALL[name][2]), s1, s2) as h:
        # degrees only
        assert raw_neighbors(h, 0) == (CMPR_OK, edges)
        row_start = np.full(s1.n + 1, 7, dtype=np.uint64)
        assert raw_neighbors(h, 0, row_start) == (CMPR_OK, edges)
        assert np.array_equal(row_start, want[0])
        assert h.stats().matches == edges
        # one short: row_start exact, nothing written to the hits
        row_start[:] = 7
        hits = np.full(edges, POISON32, dtype=np.uint32)
        assert raw_neighbors(h, edges - 1, row_start, hits) == (CMPR_OK, edges)
        assert np.array_equal(row_start, want[0])
        assert (hits == POISON32).all()
        # exact
        row_start[:] = 7
        assert raw_neighbors(h, edges, row_start, hits) == (CMPR_OK, edges)
        assert_equal_csr((row_start, hits), want, s1.n)
        # more than enough: what lies behind the edges is not the call's to write
        roomy = np.full(edges + 100, POISON32, dtype=np.uint32)
        assert raw_neighbors(h, edges + 100, None, roomy) == (CMPR_OK, edges)
        assert np.array_equal(roomy[:edges], want[1]) and (roomy[edges:] == POISON32).all()
        # refusals of the arguments
        assert raw_neighbors(h, 5, row_start, None)[0] == CMPR_EINVAL
        assert "hit_out" in h._lib.cmpr_last_error(h._ctx).decode()
        assert raw_neighbors(h, edges, row_start, hits, want_count=False)[0] == CMPR_EINVAL
        assert "n_edges_out" in h._lib.cmpr_last_error(h._ctx).decode()
        assert_equal_csr(h.neighbors(), want, s1.n)


# ---- 4. the device entry point ----

def test_device_entry_point():
    import torch
    name = "self_d1i"
    s1, s2 = _neighbors.small_sets(name)
    want = _neighbors.small_want(name)
    edges, n1 = len(want[1]), s1.n
    with resident(_neighbors.tiny_options(device=0, **_neighbors.SMALL[name][2]), s1, s2) as h:
        host = h.neighbors()
        d_rows = torch.full((n1 + 1 + 64,), POISON64, dtype=torch.int64, device="cuda")
        d_hits = torch.full((edges + 64,), POISON32, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        # degrees only; one short; exact
        assert h.neighbors_device(0, d_rows.data_ptr(), 0) == edges
        assert np.array_equal(d_rows.cpu().numpy().view(np.uint64)[:n1 + 1], want[0])
        assert h.neighbors_device(edges - 1, d_rows.data_ptr(), d_hits.data_ptr()) == edges
        assert (d_hits.cpu().numpy().view(np.uint32) == POISON32).all()
        d_rows.fill_(POISON64)
        torch.cuda.synchronize()
        assert h.neighbors_device(edges, d_rows.data_ptr(), d_hits.data_ptr()) == edges
        rows, hits = d_rows.cpu().numpy().view(np.uint64), d_hits.cpu().numpy().view(np.uint32)
        # the hits alone
        d_only = torch.full((edges + 64,), POISON32, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert h.neighbors_device(edges, 0, d_only.data_ptr()) == edges
        only = d_only.cpu().numpy().view(np.uint32)
    assert_equal_csr(host, want, n1)
    assert_equal_csr((rows[:n1 + 1].copy(), hits[:edges].copy()), host, n1)
    assert (rows[n1 + 1:] == POISON64).all() and (hits[edges:] == POISON32).all()
    assert np.array_equal(only[:edges], host[1]) and (only[edges:] == POISON32).all()


# ---- 5. the repeated step ----

def test_a_repeated_step_starts_from_clean_degrees_and_cursors():
    """the set-up of test_overflow_without_redo_pass_is_never_silent: both steps of the call overflow without a
    redo pass and are repeated; what the first attempt counted or placed must not survive"""
    a = synth.make_set(40000, 21, prefix="A", pool_size=8000)
    b = synth.make_set(40000, 22, prefix="B", pool_size=8000)
    o = Options(differences=1, **FULL)
    want = _neighbors.oracle_csr(a, b, o)
    with resident(o, a, b, {"variant": 2, "pos_segments": 1, "pos_capacity": 64}) as h:
        n = C.c_uint64()
        h.set_tunable("assume_never_overflows", 1)
        h._check(h._lib.cmpr_neighbors(h._ctx, 0, None, None, C.byref(n)))
        assert n.value == len(want[1])
        assert h.get_tunable("never_overflows") == 0               # withdrawn
        row_start = np.zeros(a.n + 1, dtype=np.uint64)
        hits = np.zeros(n.value, dtype=np.uint32)
        # (the pretence holds for every step of the call it precedes: the count step AND the fill step)
        h.set_tunable("assume_never_overflows", 1)
        h._check(h._lib.cmpr_neighbors(h._ctx, n.value, row_start.ctypes.data, hits.ctypes.data, C.byref(n)))
        assert h.get_tunable("never_overflows") == 0
        assert h.stats().matches == len(want[1])
    assert_equal_csr((row_start, hits), want, a.n)


# ---- 6. the reference in parts ----

@functools.lru_cache(maxsize=None)
def big_set():
    return synth.make_set(200_000, 30)


def test_reference_in_parts_gives_the_same_lists():
    s = big_set()
    o = Options(differences=1, device=0, **FULL)
    with resident(o, s, s) as fresh:
        pairs = fresh.overlap_pairs()
    want = _neighbors.csr_of_pairs(s.n, pairs)
    assert len(pairs) > s.n
    with resident(o, s, s) as h:
        whole = h.neighbors()
        assert h.get_tunable("reference_parts") == 1
    with resident(o, s, s, {"part_buckets_log2": 17}) as h:
        parts = h.neighbors()
        assert h.get_tunable("reference_parts") >= 3
    assert_equal_csr(whole, want, s.n)
    assert_equal_csr(parts, whole, s.n)


# ---- 7. what stays ----

def test_the_context_is_as_usable_afterwards():
    s = synth.make_set(20_000, 32, pool_size=3000)
    o = Options(differences=1, device=0, **FULL)
    with resident(o, s, s) as fresh:
        matrix, pairs = fresh.overlap_matrix(), fresh.overlap_pairs()
    want = _neighbors.csr_of_pairs(s.n, pairs)
    with resident(o, s, s) as h:
        one = h.neighbors()
        assert h.stats().matches == len(pairs)
        assert np.array_equal(h.overlap_matrix(), matrix)
        # pairs are listed again: no pointer of the call stays set
        assert np.array_equal(h.overlap_pairs(), pairs)
        assert np.array_equal(h.overlap_matrix(), matrix)
        two = h.neighbors()
        assert h.stats().matches == len(pairs)
    assert_equal_csr(one, want, s.n)
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])


# ---- 8. refusals ----

def test_refusals():
    s1, s2 = _neighbors.small_sets("other_d1")
    o = _neighbors.tiny_options(differences=1, device=0)
    with HipOverlap(o) as h:
        with pytest.raises(HipError) as want:
            h.overlap_matrix()
        assert want.value.code == CMPR_ESTATE
        for prepare in (lambda: None, lambda: h.set_reference(s2, s1.longest)):
            prepare()
            with pytest.raises(HipError) as e:
                h.neighbors()
            assert (e.value.code, str(e.value)) == (CMPR_ESTATE, str(want.value))
    with resident(o, s1, s2, {"work_shard_count": 2}) as h:
        with pytest.raises(HipError) as e:
            h.neighbors()
        assert e.value.code == CMPR_EUNSUPPORTED and "work_shard_count" in str(e.value)
        with pytest.raises(HipError) as e:
            h.neighbors_device(0, 0, 0)
        assert e.value.code == CMPR_EUNSUPPORTED and "work_shard_count" in str(e.value)
    (h,) = routed_contexts(s1, s2, o, 1, {})
    with h:
        with pytest.raises(HipError) as e:
            h.neighbors()
        assert e.value.code == CMPR_EUNSUPPORTED and "cmpr_set_queries_routed" in str(e.value)
        h.overlap_matrix()                      # (the routed set itself is in order)


def test_empty_query_set():
    z = lambda t: np.zeros(0, dtype=t)
    s2 = _neighbors.tiny(2500, 6)
    empty = RepertoireSet(z(np.uint8), np.zeros(1, dtype=np.uint64), z(np.uint32), z(np.uint32), z(np.uint32),
                          z(np.uint64), ["T1"])
    with resident(_neighbors.tiny_options(differences=1, device=0), empty, s2) as h:
        row_start = np.full(1, 7, dtype=np.uint64)
        assert raw_neighbors(h, 0, row_start) == (CMPR_OK, 0)
        assert row_start.tolist() == [0]
        row_start, hits = h.neighbors()
        assert row_start.tolist() == [0] and len(hits) == 0
