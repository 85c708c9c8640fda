"""cmpr_neighbors_distance / cmpr_neighbors_distance_device on the GPU: rows and hits against the oracle's pair list
as CSR (tests/_neighbors.py), the distance of every edge against the numpy model of the reference's --distance
(tests/_distance.py), element for element -- under every kernel family that verifies a pair, with sequences longer
than the records hold, on every sorting path, through the capacity protocol and the device entry point, with a
repeated step, a reference in parts, beside cmpr_neighbors on one context, and the refusals."""

import ctypes as C

import numpy as np
import pytest

import _distance
import _neighbors
import compairr_amd
from _routed import routed_contexts
from compairr_amd import HipError, HipOverlap, Options, RepertoireSet, synth
from test_gpu_parity import LAYOUTS, NT_LAYOUTS

pytestmark = pytest.mark.gpu

CMPR_OK, CMPR_EINVAL, CMPR_EUNSUPPORTED, CMPR_ESTATE = 0, 1, 4, 5
FULL = dict(n_v_genes=synth.N_V, n_j_genes=synth.N_J)
POISON8, POISON32, POISON64 = 0xA5, 0x25A5A5A5, 0x25A5A5A525A5A5A5


def assert_equal_edges(got, want, n1):
    """row_start, hits and distances, element for element: no edge left out, none mislabelled"""
    assert len(got) == 3 and got[2].dtype == np.uint8
    _neighbors.assert_is_csr(got[0], got[1], n1)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    wrong = np.nonzero(got[2] != want[2])[0]
    assert len(wrong) == 0, "%d of %d distances differ; first at edge %d: got %d, want %d" % (
        len(wrong), len(want[2]), wrong[0], got[2][wrong[0]], want[2][wrong[0]])


def resident(opt, set1, set2, tunables=None):
    h = HipOverlap(opt)
    for name, value in (tunables or {}).items():
        h.set_tunable(name, value)
    h.set_reference(set2, set1.longest)
    h.set_queries(set1)
    return h


# ---- 1. every kernel family that reaches score_match ----

AA_LAYOUTS = ["auto", "hbm", "lds", "rows_inline", "rows_k4_overflow", "rows_arrays", "rows_records_hashed_here"]
NT_FAMILY = ["auto", "rows_single_d2", "lds_items_k3", "lds_tiny_k8", "hbm", "pairs2_overflow"]
FAMILY_CASES = ([(name, layout) for name in ("self_d1", "self_d1i", "self_d2") for layout in AA_LAYOUTS] +
                [(name, layout) for name in ("self_d0", "other_d1") for layout in ("auto", "hbm")] +
                [(name, layout) for name in ("nt_d1ig", "nt_d2g") for layout in NT_FAMILY])


@pytest.mark.parametrize("name,layout", FAMILY_CASES, ids=["%s-%s" % c for c in FAMILY_CASES])
def test_kernel_families(name, layout):
    kw = _distance.small_options(name)
    tunables = (NT_LAYOUTS if kw.get("nucleotides") else LAYOUTS)[layout]
    s1, s2 = _distance.small_sets(name)
    want = _distance.small_want(name)
    assert _distance.histogram(want[2]) == _distance.FIGURES[name]
    got = compairr_amd.neighbors_distance(s1, s2, _neighbors.tiny_options(device=0, **kw), tunables)
    print("%s %s: [d0, d1, d2] = %s, got %s" % (name, layout, _distance.FIGURES[name], _distance.histogram(got[2])))
    assert_equal_edges(got, want, s1.n)


# ---- 2. sequences longer than the records hold ----

def test_sequences_longer_than_the_records():
    s1, s2 = _distance.long_sets()
    want = _distance.long_want()
    got = compairr_amd.neighbors_distance(s1, s2, Options(differences=2, n_v_genes=1, n_j_genes=1, device=0))
    assert_equal_edges(got, want, s1.n)


# ---- 3. the sorting paths with a payload ----

@pytest.mark.parametrize("d", [2, 1])
def test_one_row_longer_than_lds(d):
    """d = 2: the device-wide pair sort (43 625), the LDS sort (5 720, 932); d = 1: the LDS sort (305), the wave (39)"""
    s1, s2 = _neighbors.hub_sets()
    want = _distance.hub_want(d)
    got = compairr_amd.neighbors_distance(s1, s2, Options(differences=d, n_v_genes=1, n_j_genes=1, device=0))
    assert_equal_edges(got, want, s1.n)


def test_rows_at_the_thresholds():
    """rows of exactly 0, 1, 2, 8, 9, 64, 65, 8192 and 8193 hits, the two longest with distances 1 and 2 mixed"""
    s1, s2 = _neighbors.edge_rows()
    want = _distance.edge_want()
    assert np.diff(want[0].astype(np.int64)).tolist() == _neighbors.EDGE_ROWS + [0] * 61
    assert_equal_edges(compairr_amd.neighbors_distance(s1, s2, _neighbors.edge_options(device=0)), want, s1.n)


# ---- 4. the capacity protocol ----

def raw(h, capacity, row_start=None, hits=None, dist=None, want_count=True):
    """cmpr_neighbors_distance as it is declared: (code, n_edges)"""
    n = C.c_uint64(12345)
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = h._lib.cmpr_neighbors_distance(h._ctx, capacity, ptr(row_start), ptr(hits), ptr(dist),
                                        C.byref(n) if want_count else None)
    return rc, n.value


def test_capacity_protocol():
    name = "other_d1"
    s1, s2 = _distance.small_sets(name)
    want = _distance.small_want(name)
    edges = len(want[1])
    with resident(_neighbors.tiny_options(device=0, **_distance.small_options(name)), s1, s2) as h:
        # degrees only
        assert raw(h, 0) == (CMPR_OK, edges)
        row_start = np.full(s1.n + 1, 7, dtype=np.uint64)
        assert raw(h, 0, row_start) == (CMPR_OK, edges)
        assert np.array_equal(row_start, want[0])
        assert h.stats().matches == edges
        # one short: row_start exact, nothing written to either array
        row_start[:] = 7
        hits = np.full(edges, POISON32, dtype=np.uint32)
        dist = np.full(edges, POISON8, dtype=np.uint8)
        assert raw(h, edges - 1, row_start, hits, dist) == (CMPR_OK, edges)
        assert np.array_equal(row_start, want[0])
        assert (hits == POISON32).all() and (dist == POISON8).all()
        # exact
        row_start[:] = 7
        assert raw(h, edges, row_start, hits, dist) == (CMPR_OK, edges)
        assert_equal_edges((row_start, hits, dist), want, s1.n)
        assert h.stats().matches == edges
        # more than enough: what lies behind the edges is not the call's to write
        roomy_h = np.full(edges + 100, POISON32, dtype=np.uint32)
        roomy_d = np.full(edges + 100, POISON8, dtype=np.uint8)
        assert raw(h, edges + 100, None, roomy_h, roomy_d) == (CMPR_OK, edges)
        assert np.array_equal(roomy_h[:edges], want[1]) and (roomy_h[edges:] == POISON32).all()
        assert np.array_equal(roomy_d[:edges], want[2]) and (roomy_d[edges:] == POISON8).all()
        # refusals of the arguments
        assert raw(h, 5, row_start, None, dist)[0] == CMPR_EINVAL
        assert "hit_out" in h._lib.cmpr_last_error(h._ctx).decode()
        assert raw(h, 5, row_start, hits, None)[0] == CMPR_EINVAL
        assert "distance_out" in h._lib.cmpr_last_error(h._ctx).decode()
        assert raw(h, edges, row_start, hits, dist, want_count=False)[0] == CMPR_EINVAL
        assert "n_edges_out" in h._lib.cmpr_last_error(h._ctx).decode()
        assert_equal_edges(h.neighbors_distance(), want, s1.n)


# ---- 5. the device entry point ----

def test_device_entry_point():
    import torch
    name = "self_d2"
    s1, s2 = _distance.small_sets(name)
    want = _distance.small_want(name)
    edges, n1 = len(want[1]), s1.n
    with resident(_neighbors.tiny_options(device=0, **_distance.small_options(name)), s1, s2) as h:
        d_rows = torch.full((n1 + 1 + 64,), POISON64, dtype=torch.int64, device="cuda")
        d_hits = torch.full((edges + 64,), POISON32, dtype=torch.int32, device="cuda")
        d_dist = torch.full((edges + 64,), POISON8, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        # degrees only; one short; exact
        assert h.neighbors_distance_device(0, d_rows.data_ptr(), 0, 0) == edges
        assert np.array_equal(d_rows.cpu().numpy().view(np.uint64)[:n1 + 1], want[0])
        assert h.neighbors_distance_device(edges - 1, d_rows.data_ptr(), d_hits.data_ptr(), d_dist.data_ptr()) == edges
        assert (d_hits.cpu().numpy().view(np.uint32) == POISON32).all()
        assert (d_dist.cpu().numpy() == POISON8).all()
        d_rows.fill_(POISON64)
        torch.cuda.synchronize()
        assert h.neighbors_distance_device(edges, d_rows.data_ptr(), d_hits.data_ptr(), d_dist.data_ptr()) == edges
        rows, hits = d_rows.cpu().numpy().view(np.uint64), d_hits.cpu().numpy().view(np.uint32)
        dist = d_dist.cpu().numpy()
        # the two edge arrays alone
        o_hits = torch.full((edges + 64,), POISON32, dtype=torch.int32, device="cuda")
        o_dist = torch.full((edges + 64,), POISON8, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert h.neighbors_distance_device(edges, 0, o_hits.data_ptr(), o_dist.data_ptr()) == edges
        only_h, only_d = o_hits.cpu().numpy().view(np.uint32), o_dist.cpu().numpy()
    assert_equal_edges((rows[:n1 + 1].copy(), hits[:edges].copy(), dist[:edges].copy()), want, n1)
    assert (rows[n1 + 1:] == POISON64).all() and (hits[edges:] == POISON32).all() and (dist[edges:] == POISON8).all()
    assert np.array_equal(only_h[:edges], want[1]) and (only_h[edges:] == POISON32).all()
    assert np.array_equal(only_d[:edges], want[2]) and (only_d[edges:] == POISON8).all()


# ---- 6. the repeated step ----

def test_a_repeated_step_places_every_distance_once():
    """as test_a_repeated_step_starts_from_clean_degrees_and_cursors (tests/test_neighbors_gpu.py): both steps
    overflow without a redo pass and are repeated"""
    a = synth.make_set(40000, 21, prefix="A", pool_size=8000)
    b = synth.make_set(40000, 22, prefix="B", pool_size=8000)
    o = Options(differences=1, **FULL)
    rows, hits = _neighbors.oracle_csr(a, b, o)
    want = (rows, hits, _distance.edge_distances(a, b, rows, hits))
    with resident(o, a, b, {"variant": 2, "pos_segments": 1, "pos_capacity": 64}) as h:
        n = C.c_uint64()
        h.set_tunable("assume_never_overflows", 1)
        h._check(h._lib.cmpr_neighbors_distance(h._ctx, 0, None, None, None, C.byref(n)))
        assert n.value == len(want[1])
        assert h.get_tunable("never_overflows") == 0               # withdrawn
        row_start = np.zeros(a.n + 1, dtype=np.uint64)
        hits = np.zeros(n.value, dtype=np.uint32)
        dist = np.full(n.value, POISON8, dtype=np.uint8)
        h.set_tunable("assume_never_overflows", 1)
        h._check(h._lib.cmpr_neighbors_distance(h._ctx, n.value, row_start.ctypes.data, hits.ctypes.data,
                                                dist.ctypes.data, C.byref(n)))
        assert h.get_tunable("never_overflows") == 0
        assert h.stats().matches == len(want[1])
    assert_equal_edges((row_start, hits, dist), want, a.n)


# ---- 7. the reference in parts ----

def test_reference_in_parts_gives_the_same_arrays():
    s = synth.make_set(200_000, 30)        # (the set and the parts of tests/test_neighbors_gpu.py)
    o = Options(differences=1, device=0, **FULL)
    with resident(o, s, s) as h:
        whole = h.neighbors_distance()
        assert h.get_tunable("reference_parts") == 1
    with resident(o, s, s, {"part_buckets_log2": 17}) as h:
        parts = h.neighbors_distance()
        assert h.get_tunable("reference_parts") >= 3
    assert len(whole[1]) > s.n and set(whole[2].tolist()) == {0, 1}
    assert np.array_equal(whole[2], _distance.edge_distances(s, s, whole[0], whole[1]))
    assert_equal_edges(parts, whole, s.n)


# ---- 8. beside cmpr_neighbors on one context ----

def test_agreement_with_neighbors_on_one_context():
    s = synth.make_set(20_000, 32, pool_size=3000)
    o = Options(differences=1, device=0, **FULL)
    with resident(o, s, s) as fresh:
        matrix, pairs = fresh.overlap_matrix(), fresh.overlap_pairs()
    want = _neighbors.csr_of_pairs(s.n, pairs)
    with resident(o, s, s) as h:
        plain = h.neighbors()
        one = h.neighbors_distance()
        assert h.stats().matches == len(pairs)
        assert np.array_equal(h.overlap_matrix(), matrix)
        assert np.array_equal(h.overlap_pairs(), pairs)             # no pointer of the call stays set
        assert np.array_equal(h.overlap_matrix(), matrix)
        two = h.neighbors_distance()
        again = h.neighbors()
    for got in (plain, again, one[:2], two[:2]):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert_equal_edges(one, (want[0], want[1], _distance.edge_distances(s, s, want[0], want[1])), s.n)
    assert np.array_equal(one[2], two[2])


# ---- 9. refusals and the empty set ----

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
                h.neighbors_distance()
            assert (e.value.code, str(e.value)) == (CMPR_ESTATE, str(want.value))
    with resident(o, s1, s2, {"work_shard_count": 2}) as h:
        for call in (h.neighbors_distance, lambda: h.neighbors_distance_device(0, 0, 0, 0)):
            with pytest.raises(HipError) as e:
                call()
            assert e.value.code == CMPR_EUNSUPPORTED and "work_shard_count" in str(e.value)
            assert "cmpr_neighbors_distance:" in str(e.value)
    (h,) = routed_contexts(s1, s2, o, 1, {})
    with h:
        with pytest.raises(HipError) as e:
            h.neighbors_distance()
        assert e.value.code == CMPR_EUNSUPPORTED and "cmpr_set_queries_routed" in str(e.value)
        assert "cmpr_neighbors_distance:" in str(e.value)
        h.overlap_matrix()                      # (the routed set itself is in order)


def test_empty_query_set():
    z = lambda t: np.zeros(0, dtype=t)
    s2 = _neighbors.tiny(2500, 6)
    empty = RepertoireSet(z(np.uint8), np.zeros(1, dtype=np.uint64), z(np.uint32), z(np.uint32), z(np.uint32),
                          z(np.uint64), ["T1"])
    with resident(_neighbors.tiny_options(differences=1, device=0), empty, s2) as h:
        row_start = np.full(1, 7, dtype=np.uint64)
        assert raw(h, 0, row_start) == (CMPR_OK, 0)
        assert row_start.tolist() == [0]
        row_start, hits, dist = h.neighbors_distance()
        assert row_start.tolist() == [0] and len(hits) == 0 and len(dist) == 0
