"""The edit-distance kernel on the GPU at CDR3 lengths, in every register form of the query and at every distance, on
the inputs of tests/_edit_forms.py: the CSR and the matrix of the family sets against the numpy Levenshtein brute force
(tests/_edit.py), agreement with the hashed path at d = 1 and the Hamming path at d = 0, the same bytes under every
tunable, every distance up to 256 on the distance sets under every forced word count and staging, the nearest
neighbour against its brute force (tests/_edit_nearest.py), the clusters of the two family sets joined against the
connected components of the brute force's pairs, and the device entry points once.  A failing comparison names the
form of the query, the column words of the hit and both lengths.  No expectation comes from the library."""

import itertools

import numpy as np
import pytest

import _edit
import _edit_forms as ef
import _edit_nearest
import _neighbors
import compairr_amd
from _cluster_table import table_of
from compairr_amd import HipOverlap
from test_edit_gpu import SCORES

pytestmark = pytest.mark.gpu

POISON16, POISON32, POISON64 = 0xA5A5, 0x25A5A5A5, 0x25A5A5A525A5A5A5
NONE32, NONE16 = _edit_nearest.NONE32, _edit_nearest.NONE16
ALPHABETS = pytest.mark.parametrize("nucleotides", [False, True], ids=["aa", "nt"])
NAME = {False: "aa", True: "nt"}


def assert_edges(got, want, s1, s2, nucleotides, why=None):
    """the three arrays, byte for byte"""
    assert len(got) == 3 and got[2].dtype == np.uint16, why
    same = all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(got, want))
    assert same, "%s %s: %s" % (NAME[nucleotides], why, ef.differences_of(got, want, s1, s2, nucleotides))
    _neighbors.assert_is_csr(got[0], got[1], s1.n)


def assert_nearest(got, want, s1, nucleotides, why=None):
    """the three arrays: dtypes and bytes; the three sentinels exactly where ties are 0"""
    assert len(got) == 3
    for g, w, t in zip(got, want, (np.uint32, np.uint16, np.uint32)):
        assert g.dtype == t and g.shape == w.shape, why
    bad = np.nonzero((got[0] != want[0]) | (got[1] != want[1]) | (got[2] != want[2]))[0]
    lines = ["query %d (%d residues, NW = %d): got %s, want %s"
             % (i, s1.lengths[i], ef.form_of(int(s1.lengths[i]), nucleotides), [int(a[i]) for a in got],
                [int(a[i]) for a in want]) for i in bad[:8].tolist()]
    assert not len(bad), "%s %s: %d queries differ\n%s" % (NAME[nucleotides], why, len(bad), "\n".join(lines))
    none = got[2] == 0
    assert (got[0][none] == NONE32).all() and (got[1][none] == NONE16).all() and (got[0][~none] != NONE32).all(), why


# ---- 1. CSR and matrix on the family sets, and with the two sets swapped ----

@pytest.mark.parametrize("key", ef.FAMILY_KEYS, ids=ef.FAMILY_IDS)
def test_family_neighbors_and_matrix_against_the_brute_force(key):
    nucleotides, d, g = key
    s1, s2 = ef.family_sets(nucleotides)
    want = ef.family_want(nucleotides, d, g)
    back = ef.swapped(s1, s2, want)
    with HipOverlap(ef.family_options(nucleotides, g, device=0)) as h:
        got = h.edit_neighbors(s1, s2, d)
        print(key, len(got[1]), "edges, want", ef.FAMILY_FIGURES[key][0])
        assert_edges(got, want, s1, s2, nucleotides, "d = %d" % d)
        assert len(got[1]) == ef.FAMILY_FIGURES[key][0]
        assert_edges(h.edit_neighbors(s2, s1, d), back, s2, s1, nucleotides, "swapped, d = %d" % d)
    for kw in SCORES:
        opt = ef.family_options(nucleotides, g, device=0, **kw)
        with HipOverlap(opt) as h:
            for a, b, pairs in ((s1, s2, want), (s2, s1, back)):
                m = h.edit_matrix(a, b, d)
                m_want = _edit.matrix_of(a, b, pairs[0], pairs[1], opt)
                assert m.dtype == np.uint64 and m.shape == m_want.shape
                assert np.array_equal(m, m_want), (kw, a is s2)


# ---- 2. two independent kernels at d = 1; the Hamming path at d = 0 ----

@ALPHABETS
@pytest.mark.parametrize("g", [False, True], ids=["genes", "g"])
def test_agreement_with_the_hashed_path_at_d1_and_the_hamming_path_at_d0(nucleotides, g):
    s1, s2 = ef.family_sets(nucleotides)
    opt = ef.family_options(nucleotides, g, differences=1, indels=True, device=0)
    rows, hits, dist = compairr_amd.neighbors_distance(s1, s2, opt)
    want = ef.family_want(nucleotides, 1, g)
    with HipOverlap(opt) as h:
        got = h.edit_neighbors(s1, s2, 1)
        assert_edges(got, want, s1, s2, nucleotides, "d = 1")
        assert np.array_equal(got[0], rows) and np.array_equal(got[1], hits)
        assert np.array_equal(got[2].astype(np.int64), dist.astype(np.int64))
    with HipOverlap(ef.family_options(nucleotides, g, device=0)) as h:        # (the Hamming path takes no indels)
        zero = h.edit_neighbors(s1, s2, 0)
        assert_edges(zero, _edit.brute_csr(s1, s2, 0, g), s1, s2, nucleotides, "d = 0")
        for a, b in zip(zero, h.hamming_neighbors(s1, s2, 0)):
            assert a.tobytes() == b.tobytes()


# ---- 3. every tunable, the same bytes: every form of the query against columns of two and four words ----

@pytest.mark.parametrize("d", [3, 6])
def test_every_tunable_gives_the_same_bytes(d):
    s1, s2 = ef.family_sets(False)
    want = ef.family_want(False, d, True)
    opt = ef.family_options(False, True, device=0)
    m_want = _edit.matrix_of(s1, s2, want[0], want[1], opt)
    with HipOverlap(opt) as h:
        for seg, stage, words in itertools.product((1, 3, 64), (0, 1, 5), (0, 2, 4)):
            for name, value in (("edit_segments", seg), ("edit_stage_refs", stage), ("edit_words", words)):
                h.set_tunable(name, value)
            why = "d = %d, segments %d, stage %d, words %d" % (d, seg, stage, words)
            assert_edges(h.edit_neighbors(s1, s2, d), want, s1, s2, False, why)
            assert h.edit_matrix(s1, s2, d).tobytes() == m_want.tobytes(), why


# ---- 4. every distance ----

@ALPHABETS
def test_every_distance_at_every_word_count(nucleotides):
    s1, s2 = ef.distance_sets(nucleotides)
    want = ef.distance_want(nucleotides)
    back = ef.swapped(s1, s2, want)
    assert len(want[1]) == s1.n * s2.n == 5184
    opt = ef.distance_options(nucleotides, device=0)
    at_100 = ef.distance_want(nucleotides, 100)
    back_100 = ef.swapped(s1, s2, at_100)
    with HipOverlap(opt) as h:
        for words, stage in itertools.product((0, 2, 4), (0, 1)):
            h.set_tunable("edit_words", words)
            h.set_tunable("edit_stage_refs", stage)
            for d in (ef.DISTANCE_D, 2 ** 40):
                why = "d = %d, words %d, stage %d" % (d, words, stage)
                assert_edges(h.edit_neighbors(s1, s2, d), want, s1, s2, nucleotides, why)
                assert_edges(h.edit_neighbors(s2, s1, d), back, s2, s1, nucleotides, "swapped, " + why)
            for a, b, pairs, all_pairs in ((s1, s2, at_100, want), (s2, s1, back_100, back)):
                assert np.array_equal(h.edit_matrix(a, b, 100), _edit.matrix_of(a, b, pairs[0], pairs[1], opt)), \
                    (words, stage, a is s2)
                assert np.array_equal(h.edit_matrix(a, b, 2 ** 40),
                                      _edit.matrix_of(a, b, all_pairs[0], all_pairs[1], opt)), (words, stage, a is s2)
            assert_edges(h.edit_neighbors(s1, s2, 100), at_100, s1, s2, nucleotides, "d = 100, words %d" % words)


# ---- 5. the nearest neighbour ----

@ALPHABETS
@pytest.mark.parametrize("g", [False, True], ids=["genes", "g"])
def test_family_nearest_against_the_brute_force(nucleotides, g):
    s1, s2 = ef.family_sets(nucleotides)
    dist = ef.family_distances(nucleotides)
    lonely = ef.carries(s1, ef.PARTNERLESS_VJ)
    with HipOverlap(ef.family_options(nucleotides, g, device=0)) as h:
        for prune, floor, cap in itertools.product((0, 1), (0, 1), (3, 6, None)):
            h.set_tunable("edit_nearest_prune", prune)
            got = h.edit_nearest(s1, s2, floor, cap)
            want = _edit_nearest.brute(s1, s2, g, floor, cap, False, dist)
            assert_nearest(got, want, s1, nucleotides, "prune %d, floor %d, cap %s" % (prune, floor, cap))
            if not g and cap is not None:
                # the family without a partner: the three sentinels
                assert (got[0][lonely] == NONE32).all() and (got[1][lonely] == NONE16).all()
                assert not got[2][lonely].any() and got[2][~lonely].any()


@ALPHABETS
@pytest.mark.parametrize("g", [False, True], ids=["genes", "g"])
def test_family_nearest_in_one_set_mode(nucleotides, g):
    s1, _ = ef.family_sets(nucleotides)
    dist = ef.family_distances(nucleotides, True)
    with HipOverlap(ef.family_options(nucleotides, g, device=0)) as h:
        for other, floor, cap in itertools.product((False, True), (0, 1), (3, None)):
            got = h.edit_nearest(s1, s1, floor, cap, other)
            want = _edit_nearest.brute(s1, s1, g, floor, cap, other, dist)
            assert_nearest(got, want, s1, nucleotides, "other %d, floor %d, cap %s" % (other, floor, cap))


@ALPHABETS
def test_nearest_at_every_word_count(nucleotides):
    """uncapped on the distance sets: the nearest of a long random sequence is far away"""
    s1, s2 = ef.distance_sets(nucleotides)
    dist = _edit_nearest.all_distances(s1, s2)
    far = 0
    with HipOverlap(ef.distance_options(nucleotides, device=0)) as h:
        for prune, floor in itertools.product((0, 1), (0, 1)):
            h.set_tunable("edit_nearest_prune", prune)
            want = _edit_nearest.brute(s1, s2, True, floor, None, False, dist)
            assert_nearest(h.edit_nearest(s1, s2, floor, None), want, s1, nucleotides,
                           "prune %d, floor %d" % (prune, floor))
            far = max(far, int(want[1].max()))
            assert (want[2] > 0).all()
    assert far > 64


# ---- 6. clusters of the two family sets joined ----

@ALPHABETS
@pytest.mark.parametrize("d,g", [(1, False), (1, True), (3, False), (3, True), (6, False), (6, True)],
                         ids=["d1", "d1-g", "d3", "d3-g", "d6", "d6-g"])
def test_clusters_of_the_joined_family_sets(nucleotides, d, g):
    s = ef.family_union(nucleotides)
    label, size, clusters = ef.union_want(nucleotides, d, g)
    assert 1 < clusters < s.n
    want_table = table_of(label, s.count)
    with HipOverlap(compairr_amd.Options(device=0, **ef.family_kw(nucleotides, g))) as h:
        for seg in (1, 7):
            h.set_tunable("edit_segments", seg)
            got = h.edit_cluster(s, d)
            bad = np.nonzero(got[0] != label)[0]
            assert not len(bad), "%s segments %d: %s" % (
                NAME[nucleotides], seg, [(i, int(s.lengths[i]), ef.form_of(int(s.lengths[i]), nucleotides),
                                          int(got[0][i]), int(label[i])) for i in bad[:8].tolist()])
            assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32
            assert np.array_equal(got[1], size) and got[2] == clusters
            table = h.edit_cluster_table(s, d)
            for a, b in zip(table, want_table):
                assert a.dtype == b.dtype and np.array_equal(a, b), seg


# ---- 7. the device entry points, once ----

def test_device_entry_points():
    import torch
    d = 3
    s1, s2 = ef.family_sets(False)
    u = ef.family_union(False)
    want = ef.family_want(False, d, False)
    edges, n1, pad = len(want[1]), s1.n, 64
    opt = ef.family_options(False, False, device=0)
    m_want = _edit.matrix_of(s1, s2, want[0], want[1], opt)
    near = _edit_nearest.brute(s1, s2, False, 1, d, False, ef.family_distances(False))
    label, size, clusters = ef.union_want(False, d, False)
    t_want = table_of(label, u.count)
    full = lambda n, value, t: torch.full((n,), value, dtype=t, device="cuda")
    with HipOverlap(opt) as h:
        v1, keep1 = HipOverlap.device_view(s1)
        v2, keep2 = HipOverlap.device_view(s2)
        vu, keep3 = HipOverlap.device_view(u)
        d_rows = full(n1 + 1 + pad, POISON64, torch.int64)
        d_hits = full(edges + pad, POISON32, torch.int32)
        d_dist = full(edges + pad, POISON16 - 65536, torch.int16)
        d_mat = full(m_want.size + pad, POISON64, torch.int64)
        d_near = [full(n1 + pad, POISON32, torch.int32), full(n1 + pad, POISON16 - 65536, torch.int16),
                  full(n1 + pad, POISON32, torch.int32)]
        d_table = [full(u.n + pad, POISON32, torch.int32), full(u.n + 1 + pad, POISON64, torch.int64),
                   full(u.n + pad, POISON32, torch.int32), full(u.n + pad, POISON64, torch.int64)]
        torch.cuda.synchronize()
        assert h.edit_neighbors_device(v1, v2, d, edges + pad, d_rows.data_ptr(), d_hits.data_ptr(),
                                       d_dist.data_ptr()) == edges
        h.edit_matrix_device(v1, v2, d, d_mat.data_ptr())
        found = h.edit_nearest_device(v1, v2, 1, d, 0, *[t.data_ptr() for t in d_near])
        assert h.edit_cluster_table_device(vu, d, *[t.data_ptr() for t in d_table]) == clusters
        rows, hits = d_rows.cpu().numpy().view(np.uint64), d_hits.cpu().numpy().view(np.uint32)
        dist, mat = d_dist.cpu().numpy().view(np.uint16), d_mat.cpu().numpy().view(np.uint64)
        got_near = [t.cpu().numpy().view(k) for t, k in zip(d_near, (np.uint32, np.uint16, np.uint32))]
        got_table = [t.cpu().numpy().view(k) for t, k in zip(d_table, (np.uint32, np.uint64, np.uint32, np.uint64))]
        del keep1, keep2, keep3
    # neighbours: the edges, and nothing behind them
    assert_edges((rows[:n1 + 1].copy(), hits[:edges].copy(), dist[:edges].copy()), want, s1, s2, False, "device")
    assert (rows[n1 + 1:] == POISON64).all() and (hits[edges:] == POISON32).all() and (dist[edges:] == POISON16).all()
    # matrix
    assert np.array_equal(mat[:m_want.size].reshape(m_want.shape), m_want) and (mat[m_want.size:] == POISON64).all()
    # nearest
    assert found == int((near[2] > 0).sum()) and 0 < found < n1
    assert_nearest([a[:n1].copy() for a in got_near], near, s1, False, "device")
    for a, p in zip(got_near, (POISON32, POISON16, POISON32)):
        assert (a[n1:] == p).all()
    # cluster table: n of cluster_of and members, K + 1 of cluster_start, K of count, no more
    for a, w, m in zip(got_table, t_want, (u.n, clusters + 1, u.n, clusters)):
        assert np.array_equal(a[:m], w) and (a[m:] == (POISON64 if a.dtype == np.uint64 else POISON32)).all()
