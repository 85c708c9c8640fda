"""cmpr_edit_neighbors / cmpr_edit_matrix and their _device variants on the GPU: the CSR and the matrix against the
numpy Levenshtein brute force (tests/_edit.py) on every input of the issue, the oracle's -d 1 -i cells, agreement with
the hashed path at d = 1 and with cmpr_hamming_neighbors at d = 0 and d = 3, the column words at their edges under
every forced word count and staging, the length limit, the same bytes under every tunable, a row beyond LDS, wrapping
sums, the capacity protocol, the device entry points, huge d, the resident state left alone, the refusals,
determinism and empty sets.  No expectation comes from the library."""

import ctypes as C
import itertools

import numpy as np
import pytest

import _edit
import _hamming
import _neighbors
import _oracle
import compairr_amd
from compairr_amd import HipError, HipOverlap, Options, RepertoireSet
from compairr_amd.hip import _view
from compairr_amd.sets import AA

pytestmark = pytest.mark.gpu

CMPR_OK, CMPR_EINVAL, CMPR_EUNSUPPORTED = 0, 1, 4
POISON16, POISON32, POISON64 = 0xA5A5, 0x25A5A5A5, 0x25A5A5A525A5A5A5
KEYS = list(_edit.EDGES)
IDS = ["%s-d%d%s" % (k[0], k[1], "-g" if k[2] else "") for k in KEYS]


def assert_equal_edges(got, want, n1):
    assert len(got) == 3 and got[2].dtype == np.uint16
    _neighbors.assert_is_csr(got[0], got[1], n1)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


# ---- 1. CSR and matrix parity ----

@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_neighbors_against_the_brute_force(key):
    name, d, g = key
    s1, s2 = _edit.sets_of(name)
    want = _edit.want(name, d, g)
    got = compairr_amd.edit_neighbors(s1, s2, _edit.options_of(name, g, device=0), d)
    print("%s d=%d g=%d: %d edges, want %d" % (name, d, g, len(got[1]), _edit.EDGES[key]))
    assert int(got[0][-1]) == len(got[1]) == _edit.EDGES[key]
    assert_equal_edges(got, want, s1.n)


SCORES = [dict(score="product"), dict(score="min"), dict(score="max"), dict(score="mean"),
          dict(ignore_counts=True), dict(existence=True), dict(existence=True, score="mean")]


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_matrix_against_the_brute_force(key):
    name, d, g = key
    s1, s2 = _edit.sets_of(name)
    rows, hits, _ = _edit.want(name, d, g)
    for kw in SCORES:
        opt = _edit.options_of(name, g, device=0, **kw)
        got = compairr_amd.edit_matrix(s1, s2, opt, d)
        want = _edit.matrix_of(s1, s2, rows, hits, opt)
        assert got.dtype == np.uint64 and got.shape == want.shape
        assert np.array_equal(got, want), kw
        if d == 1:
            cells, st = _oracle.overlap(s1, s2, _edit.options_of(name, g, differences=1, indels=True, **kw))
            assert st.matches == _edit.EDGES[key]
            assert np.array_equal(got, _oracle.integer_cells(cells, opt)), kw


def test_matrix_beyond_the_lds_copy():
    """33 x 33 repertoires: more cells than the workgroup's copy of the matrix holds -- global atomics"""
    a, b = _edit.nt_sets()
    rng = np.random.default_rng(7)
    many = lambda s, p: RepertoireSet(s.residues, s.offsets, s.v_gene, s.j_gene,
                                      np.concatenate([np.arange(33), rng.integers(0, 33, size=s.n - 33)]).astype(np.uint32),
                                      s.count, ["%s%d" % (p, k) for k in range(33)], s.v_names, s.j_names, s.alphabet)
    a, b = many(a, "A"), many(b, "B")
    rows, hits, _ = _edit.brute_csr(a, b, 3, True)
    opt = _edit.options_of("nt", True, device=0)
    assert np.array_equal(compairr_amd.edit_matrix(a, b, opt, 3), _edit.matrix_of(a, b, rows, hits, opt))


@pytest.mark.parametrize("g", [False, True], ids=["genes", "g"])
def test_one_residue_against_none_is_a_pair(g):
    """where Levenshtein and the reference's -d 1 -i part (variants.cc:301): the brute force has the pairs"""
    s1, s2 = _edit.min0_sets()
    want = _edit.brute_csr(s1, s2, 1, g)
    got = compairr_amd.edit_neighbors(s1, s2, _edit.options(ignore_genes=g, device=0), 1)
    assert len(got[1]) == _edit.MIN0[g][0]
    assert_equal_edges(got, want, s1.n)


# ---- 2. agreement of the kernels ----

@pytest.mark.parametrize("name", ["nt", "aa"])
@pytest.mark.parametrize("g", [False, True], ids=["genes", "g"])
def test_agreement_with_the_hashed_path_at_d1(name, g):
    s1, s2 = _edit.sets_of(name)
    opt = _edit.options_of(name, g, differences=1, indels=True, device=0)
    rows, hits, dist = compairr_amd.neighbors_distance(s1, s2, opt)
    got = compairr_amd.edit_neighbors(s1, s2, opt, 1)
    assert np.array_equal(got[0], rows) and np.array_equal(got[1], hits)
    assert np.array_equal(got[2].astype(np.int64), dist.astype(np.int64))


@pytest.mark.parametrize("name", ["nt", "aa"])
@pytest.mark.parametrize("g", [False, True], ids=["genes", "g"])
def test_agreement_with_the_hamming_path(name, g):
    s1, s2 = _edit.sets_of(name)
    with HipOverlap(_edit.options_of(name, g, device=0)) as h:
        for a, b in zip(h.edit_neighbors(s1, s2, 0), h.hamming_neighbors(s1, s2, 0)):
            assert a.tobytes() == b.tobytes()
        assert np.array_equal(h.edit_matrix(s1, s2, 0), h.hamming_matrix(s1, s2, 0))
        rows, hits, dist = h.edit_neighbors(s1, s2, 3)
        p_rows, p_hits, p_dist = h.hamming_neighbors(s1, s2, 3)
    edges = {(int(q), int(j)): int(dd) for q, j, dd in zip(_edit.queries_of(rows), hits, dist)}
    assert 0 < len(p_hits) < len(hits)
    for q, j, dd in zip(_edit.queries_of(p_rows), p_hits, p_dist):
        assert edges[(int(q), int(j))] <= int(dd)


# ---- 3. the column words at their edges ----

@pytest.mark.parametrize("nucleotides", [False, True], ids=["aa", "nt"])
def test_lengths_at_the_word_edges(nucleotides):
    s1, s2, _, _ = _edit.edge_sets(nucleotides)
    want = _edit.edge_want(nucleotides)
    opt = _edit.edge_options(nucleotides, device=0)
    rows, hits, _ = want
    with HipOverlap(opt) as h:
        for words, stage in itertools.product((0, 2, 4), (0, 1, 3)):
            h.set_tunable("edit_words", words)
            h.set_tunable("edit_stage_refs", stage)
            assert_equal_edges(h.edit_neighbors(s1, s2, _edit.EDGE_D), want, s1.n)
            assert np.array_equal(h.edit_matrix(s1, s2, _edit.EDGE_D), _edit.matrix_of(s1, s2, rows, hits, opt))
        # the two sets swapped: the long sequences as queries of every form, the edited ones as references
        h.set_tunable("edit_words", 0)
        assert_equal_edges(h.edit_neighbors(s2, s1, _edit.EDGE_D), _edit.brute_csr(s2, s1, _edit.EDGE_D), s2.n)


def test_the_length_limit():
    """one sequence of 257 residues: refused with code and text, whichever set holds it; the resident state unharmed"""
    rng = np.random.default_rng(257)
    ok = _neighbors._set_of_rows(rng.integers(0, 20, size=(5, 256), dtype=np.uint8), 1, 2)
    long = _neighbors._set_of_rows(rng.integers(0, 20, size=(1, 257), dtype=np.uint8), 2, 1)
    s1, s2 = _edit.aa_sets()
    with HipOverlap(Options(differences=1, n_v_genes=2, n_j_genes=2, device=0)) as h:
        h.set_reference(s2, s1.longest)
        h.set_queries(s1)
        before, matches = h.overlap_matrix(), h.stats().matches
        for call in (lambda: h.edit_neighbors(ok, long, 2), lambda: h.edit_neighbors(long, ok, 2),
                     lambda: h.edit_matrix(long, long, 2), lambda: h.edit_matrix(ok, long, 2)):
            with pytest.raises(HipError) as e:
                call()
            assert e.value.code == CMPR_EUNSUPPORTED
            assert str(e.value).endswith("cmpr_edit: a sequence of more than 256 residues")
        assert np.array_equal(h.overlap_matrix(), before) and h.stats().matches == matches
        want = _edit.brute_csr(ok, ok, 2, True)
        assert_equal_edges(h.edit_neighbors(ok, ok, 2), want, ok.n)


# ---- 4. the same bytes under every tunable ----

@pytest.mark.parametrize("d", [3, 5])
def test_every_tunable_gives_the_same_bytes(d):
    s1, s2 = _edit.aa_sets()
    want = _edit.want("aa", d, True)
    opt = _edit.options_of("aa", True, device=0)
    m_want = _edit.matrix_of(s1, s2, want[0], want[1], opt)
    with HipOverlap(opt) as h:
        for seg, stage, words in itertools.product((1, 2, 7, 64), (0, 1, 5), (0, 2, 4)):
            for name, value in (("edit_segments", seg), ("edit_stage_refs", stage), ("edit_words", words)):
                h.set_tunable(name, value)
            got = h.edit_neighbors(s1, s2, d)
            for g, w in zip(got, want):
                assert g.tobytes() == w.tobytes(), (seg, stage, words)
            assert h.edit_matrix(s1, s2, d).tobytes() == m_want.tobytes(), (seg, stage, words)
        h.edit_neighbors(s1, s2, d)
        assert h.get_tunable("edit_compare_us") > 0 and h.get_tunable("edit_group_us") > 0
        assert h.get_tunable("edit_order_us") > 0 and h.get_tunable("edit_copy_us") > 0
        for name, bad in (("edit_words", 3), ("edit_words", 8), ("edit_segments", 65), ("edit_stage_refs", -1)):
            with pytest.raises(HipError) as e:
                h.set_tunable(name, bad)
            assert e.value.code == CMPR_EINVAL
    assert len(want[1]) == _edit.EDGES[("aa", d, True)]


# ---- 5. a row beyond LDS ----

def test_rows_beyond_lds():
    """every pair is an edge: rows of 9 001 hits, put in order by the device-wide sort; with and without distances"""
    s1, s2 = _edit.long_row_sets()
    want = _edit.want("long", 9, True)
    assert len(want[1]) == _edit.LONG_ROW_EDGES and int(want[2].max()) <= 9
    assert np.array_equal(want[1], np.tile(np.arange(9001, dtype=np.uint32), 70))
    with HipOverlap(_edit.options_of("long", True, device=0)) as h:
        assert_equal_edges(h.edit_neighbors(s1, s2, 9), want, s1.n)
        rows, hits, none = h.edit_neighbors(s1, s2, 9, distances=False)
        assert none is None and np.array_equal(rows, want[0]) and np.array_equal(hits, want[1])
        h.set_tunable("edit_segments", 7)
        assert_equal_edges(h.edit_neighbors(s1, s2, 9), want, s1.n)


# ---- 6. sums wrap ----

def test_wrapping_sums():
    seqs1 = [[1, 2, 3, 4, 5], [1, 2, 3, 4], [2, 3, 4, 5, 6, 7]]
    seqs2 = [[1, 2, 3, 4, 5], [2, 3, 4, 5], [1, 2, 9, 9, 6, 7]]
    c1 = [2 ** 33 + 1, 2 ** 33 + 5, 2 ** 40 + 7]
    c2 = [2 ** 33 + 3, 2 ** 35 + 11, 2 ** 63 + 9]

    def make(seqs, counts):
        off = np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)
        n = len(seqs)
        return RepertoireSet(np.concatenate(seqs).astype(np.uint8), off, np.zeros(n, dtype=np.uint32),
                             np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32),
                             np.array(counts, dtype=np.uint64), ["R1"], ["V0"], ["J0"], AA)
    a, b = make(seqs1, c1), make(seqs2, c2)
    opt = Options(n_v_genes=1, n_j_genes=1, device=0)
    for d in (0, 1, 2, 6):
        rows, hits, _ = _edit.brute_csr(a, b, d)
        want = sum(c1[i] * c2[int(j)] for i, j in zip(_edit.queries_of(rows), hits))
        assert want >= 2 ** 64 or d == 0
        assert int(compairr_amd.edit_matrix(a, b, opt, d)[0, 0]) == want % 2 ** 64
    assert len(_edit.brute_csr(a, b, 6)[1]) == 9
    want = sum(c1[i] + c2[j] for i in range(3) for j in range(3))
    assert int(compairr_amd.edit_matrix(a, b, Options(n_v_genes=1, n_j_genes=1, score="mean", device=0), 6)[0, 0]) \
        == want % 2 ** 64


# ---- 7. the capacity protocol ----

def raw(h, v1, v2, d, capacity, row_start=None, hits=None, dist=None, want_count=True):
    """cmpr_edit_neighbors as it is declared: (code, n_edges)"""
    n = C.c_uint64(12345)
    ptr = lambda a: None if a is None else a.ctypes.data
    ref = lambda v: None if v is None else C.byref(v)
    rc = h._lib.cmpr_edit_neighbors(h._ctx, ref(v1), ref(v2), d, capacity, ptr(row_start), ptr(hits), ptr(dist),
                                    C.byref(n) if want_count else None)
    return rc, n.value


def test_capacity_protocol():
    s1, s2 = _edit.nt_sets()
    want = _edit.want("nt", 3, True)
    edges = len(want[1])
    v1, v2 = _view(s1), _view(s2)
    with HipOverlap(_edit.options_of("nt", True, device=0)) as h:
        # count only
        assert raw(h, v1, v2, 3, 0) == (CMPR_OK, edges)
        row_start = np.full(s1.n + 1, 7, dtype=np.uint64)
        assert raw(h, v1, v2, 3, 0, row_start) == (CMPR_OK, edges)
        assert np.array_equal(row_start, want[0])
        # one short: row_start exact, nothing written to either array
        row_start[:] = 7
        hits = np.full(edges, POISON32, dtype=np.uint32)
        dist = np.full(edges, POISON16, dtype=np.uint16)
        assert raw(h, v1, v2, 3, edges - 1, row_start, hits, dist) == (CMPR_OK, edges)
        assert np.array_equal(row_start, want[0])
        assert (hits == POISON32).all() and (dist == POISON16).all()
        # exact
        row_start[:] = 7
        assert raw(h, v1, v2, 3, edges, row_start, hits, dist) == (CMPR_OK, edges)
        assert_equal_edges((row_start, hits, dist), want, s1.n)
        # generous: what lies behind the edges is not the call's to write
        roomy_h = np.full(edges + 100, POISON32, dtype=np.uint32)
        roomy_d = np.full(edges + 100, POISON16, dtype=np.uint16)
        assert raw(h, v1, v2, 3, edges + 100, None, roomy_h, roomy_d) == (CMPR_OK, edges)
        assert np.array_equal(roomy_h[:edges], want[1]) and (roomy_h[edges:] == POISON32).all()
        assert np.array_equal(roomy_d[:edges], want[2]) and (roomy_d[edges:] == POISON16).all()
        # hits only
        only = np.full(edges, POISON32, dtype=np.uint32)
        assert raw(h, v1, v2, 3, edges, None, only, None) == (CMPR_OK, edges)
        assert np.array_equal(only, want[1])
        assert h.edit_neighbors(s1, s2, 3, distances=False)[2] is None
        # refusals of the arguments
        assert raw(h, v1, v2, 3, 5, row_start, None, dist)[0] == CMPR_EINVAL
        assert "hit_out" in h._lib.cmpr_last_error(h._ctx).decode()
        assert raw(h, v1, v2, 3, edges, row_start, hits, dist, want_count=False)[0] == CMPR_EINVAL
        assert "n_edges_out" in h._lib.cmpr_last_error(h._ctx).decode()


# ---- 8. the device entry points ----

def test_device_entry_points():
    import torch
    s1, s2 = _edit.nt_sets()
    want = _edit.want("nt", 4, False)
    edges, n1 = len(want[1]), s1.n
    opt = _edit.options_of("nt", False, device=0)
    m_want = _edit.matrix_of(s1, s2, want[0], want[1], opt)
    with HipOverlap(opt) as h:
        v1, keep1 = HipOverlap.device_view(s1)
        v2, keep2 = HipOverlap.device_view(s2)
        d_rows = torch.full((n1 + 1 + 64,), POISON64, dtype=torch.int64, device="cuda")
        d_hits = torch.full((edges + 64,), POISON32, dtype=torch.int32, device="cuda")
        d_dist = torch.full((edges + 64,), POISON16 - 65536, dtype=torch.int16, device="cuda")
        d_mat = torch.full((s1.n_repertoires * s2.n_repertoires + 8,), POISON64, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        # count only; one short; exact
        assert h.edit_neighbors_device(v1, v2, 4, 0, d_rows.data_ptr()) == edges
        assert np.array_equal(d_rows.cpu().numpy().view(np.uint64)[:n1 + 1], want[0])
        assert h.edit_neighbors_device(v1, v2, 4, edges - 1, d_rows.data_ptr(), d_hits.data_ptr(),
                                       d_dist.data_ptr()) == edges
        assert (d_hits.cpu().numpy().view(np.uint32) == POISON32).all()
        assert (d_dist.cpu().numpy().view(np.uint16) == POISON16).all()
        d_rows.fill_(POISON64)
        torch.cuda.synchronize()
        assert h.edit_neighbors_device(v1, v2, 4, edges + 10, d_rows.data_ptr(), d_hits.data_ptr(),
                                       d_dist.data_ptr()) == edges
        h.edit_matrix_device(v1, v2, 4, d_mat.data_ptr())
        rows, hits = d_rows.cpu().numpy().view(np.uint64), d_hits.cpu().numpy().view(np.uint32)
        dist, mat = d_dist.cpu().numpy().view(np.uint16), d_mat.cpu().numpy().view(np.uint64)
        # hits only, no row_start: the rows are put in order all the same
        d_only = torch.full((edges,), POISON32, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert h.edit_neighbors_device(v1, v2, 4, edges, 0, d_only.data_ptr()) == edges
        only = d_only.cpu().numpy().view(np.uint32)
        # one-file mode: the same view twice
        self_edges = h.edit_neighbors_device(v1, v1, 4)
        host = h.edit_neighbors(s1, s2, 4)
        del keep1, keep2
    assert_equal_edges((rows[:n1 + 1].copy(), hits[:edges].copy(), dist[:edges].copy()), want, n1)
    assert_equal_edges(host, want, n1)
    assert np.array_equal(only, want[1])
    assert (rows[n1 + 1:] == POISON64).all() and (hits[edges:] == POISON32).all() and (dist[edges:] == POISON16).all()
    assert np.array_equal(mat[:-8].reshape(m_want.shape), m_want) and (mat[-8:] == POISON64).all()
    assert self_edges == len(_edit.brute_csr(s1, s1, 4)[1])


# ---- 9. d above the longest sequence ----

@pytest.mark.parametrize("name,g", [("nt", False), ("nt", True), ("aa", False), ("min0", False)])
def test_huge_d(name, g):
    s1, s2 = _edit.sets_of(name)
    longest = max(s1.longest, s2.longest)
    with HipOverlap(_edit.options_of(name, g, device=0)) as h:
        at_longest = h.edit_neighbors(s1, s2, longest)
        for d in (2 ** 40, 2 ** 62):
            got = h.edit_neighbors(s1, s2, d)
            for a, b in zip(got, at_longest):
                assert np.array_equal(a, b)
    assert len(at_longest[1]) == _edit.same_genes_pairs(s1, s2, g)
    assert_equal_edges(at_longest, _edit.brute_csr(s1, s2, longest, g), s1.n)


# ---- 10. the resident state is left alone; the context's own d and indels play no part ----

def test_resident_state_is_left_alone():
    s1, s2 = _edit.nt_sets()
    want = _edit.want("nt", 3, False)
    with HipOverlap(_edit.options_of("nt", False, differences=1, device=0)) as h:
        h.set_reference(s2, s1.longest)
        h.set_queries(s1)
        before, matches = h.overlap_matrix(), h.stats().matches
        assert_equal_edges(h.edit_neighbors(s1, s2, 3), want, s1.n)
        h.edit_matrix(s1, s2, 3)
        assert h.stats().matches == matches
        assert np.array_equal(h.overlap_matrix(), before) and h.stats().matches == matches
        assert np.array_equal(h.neighbors()[0],
                              _neighbors.oracle_csr(s1, s2, _edit.options_of("nt", False, differences=1))[0])


@pytest.mark.parametrize("kw", [dict(differences=1, indels=True), dict(differences=2), dict(differences=0)],
                         ids=["indels", "d2", "d0"])
def test_the_options_distance_and_indels_are_ignored(kw):
    s1, s2 = _edit.nt_sets()
    want = _edit.want("nt", 3, False)
    opt = _edit.options_of("nt", False, device=0, **kw)
    with HipOverlap(opt) as h:
        assert_equal_edges(h.edit_neighbors(s1, s2, 3), want, s1.n)
        assert np.array_equal(h.edit_matrix(s1, s2, 3), _edit.matrix_of(s1, s2, want[0], want[1], opt))


# ---- 11. refusals ----

def test_refusals():
    s1, s2 = _edit.nt_sets()
    v1, v2 = _view(s1), _view(s2)
    m = np.zeros((3, 3), dtype=np.uint64)
    nt = lambda **kw: _edit.options_of("nt", False, device=0, **kw)

    def both(h, d=3, a=v1, b=v2):
        ref = lambda v: None if v is None else C.byref(v)
        out = []
        for call in (lambda: raw(h, a, b, d, 0)[0],
                     lambda: h._lib.cmpr_edit_matrix(h._ctx, ref(a), ref(b), d, m.ctypes.data)):
            out.append((call(), h._lib.cmpr_last_error(h._ctx).decode()))
        return out

    with HipOverlap(nt()) as h:
        for rc, text in both(h, d=-1):
            assert rc == CMPR_EINVAL and text == "Differences specified with -d or -differences cannot be negative."
        for a, b in ((None, v2), (v1, None)):
            for rc, text in both(h, a=a, b=b):
                assert rc == CMPR_EINVAL and text == "set view is NULL"
        h.set_tunable("work_shard_count", 2)
        for rc, text in both(h):
            assert rc == CMPR_EUNSUPPORTED and "work_shard_count" in text
    with HipOverlap(nt(score="ratio")) as h:
        (rc_n, _), (rc_m, text) = both(h)
        assert rc_n == CMPR_OK and rc_m == CMPR_EINVAL and "ratio score needs cmpr_overlap_matrix_f64" in text
    with HipOverlap(nt(score="ratio", ignore_counts=True)) as h:
        assert [rc for rc, _ in both(h)] == [CMPR_OK, CMPR_OK]
    for score in ("mh", "jaccard"):
        with HipOverlap(nt(score=score)) as h:
            for rc, text in both(h, d=1):
                assert rc == CMPR_EINVAL and text == "The Morisita-Horn / Jaccard index is not defined when d>0"
            assert [rc for rc, _ in both(h, d=0)] == [CMPR_OK, CMPR_OK]
    with HipOverlap(Options(nucleotides=True, n_v_genes=2 ** 24, n_j_genes=2 ** 23, device=0)) as h:
        for rc, text in both(h):
            assert rc == CMPR_EUNSUPPORTED and "n_v_genes x n_j_genes > 2^46" in text
    # a set the validation refuses: the same code and text as cmpr_set_reference
    bad = RepertoireSet(s2.residues, s2.offsets, s2.v_gene, s2.j_gene, s2.repertoire, s2.count.copy(),
                        s2.repertoire_ids, s2.v_names, s2.j_names, s2.alphabet)
    bad.count[17] = 0
    with HipOverlap(nt()) as h:
        with pytest.raises(HipError) as want:
            h.set_reference(bad)
        for call in (lambda: h.edit_neighbors(s1, bad, 3), lambda: h.edit_matrix(bad, s2, 3)):
            with pytest.raises(HipError) as e:
                call()
            assert (e.value.code, str(e.value)) == (want.value.code, str(want.value))
        assert_equal_edges(h.edit_neighbors(s1, s2, 3), _edit.want("nt", 3, False), s1.n)


# ---- 12. determinism; empty sets ----

def test_two_runs_give_the_same_bytes():
    s1, s2 = _edit.aa_sets()
    opt = _edit.options_of("aa", True, device=0)
    one = compairr_amd.edit_neighbors(s1, s2, opt, 5)
    two = compairr_amd.edit_neighbors(s1, s2, opt, 5)
    assert [a.tobytes() for a in one] == [b.tobytes() for b in two]
    assert compairr_amd.edit_matrix(s1, s2, opt, 5).tobytes() == compairr_amd.edit_matrix(s1, s2, opt, 5).tobytes()


def test_empty_sets():
    z = lambda t: np.zeros(0, dtype=t)
    s = _edit.aa_sets()[0]
    empty = RepertoireSet(z(np.uint8), np.zeros(1, dtype=np.uint64), z(np.uint32), z(np.uint32), z(np.uint32),
                          z(np.uint64), ["T1", "T2"], ["V0", "V1"], ["J0", "J1"], AA)
    with HipOverlap(_edit.options(device=0)) as h:
        rows, hits, dist = h.edit_neighbors(empty, s, 3)
        assert rows.tolist() == [0] and len(hits) == 0 and len(dist) == 0
        rows, hits, dist = h.edit_neighbors(s, empty, 3)
        assert rows.tolist() == [0] * (s.n + 1) and len(hits) == 0
        m = np.full((2, 3), 7, dtype=np.uint64)
        v_e, v_s = _view(empty), _view(s)
        assert h._lib.cmpr_edit_matrix(h._ctx, C.byref(v_e), C.byref(v_s), 3, m.ctypes.data) == CMPR_OK
        assert not m.any()
        m = np.full((3, 2), 7, dtype=np.uint64)
        assert h._lib.cmpr_edit_matrix(h._ctx, C.byref(v_s), C.byref(v_e), 3, m.ctypes.data) == CMPR_OK
        assert not m.any()
        assert h.edit_neighbors(empty, empty, 3)[0].tolist() == [0]


# ---- 13. the drivers shared with cmpr_hamming_*: each family's timers are its own; the order of the refusals ----

HAMMING_TIMERS = ("hamming_group_us", "hamming_compare_us", "hamming_copy_us")
EDIT_TIMERS = ("edit_group_us", "edit_compare_us", "edit_order_us", "edit_copy_us")


def test_timers_stay_apart():
    """a cmpr_edit_* call leaves the three hamming_*_us as they were, a cmpr_hamming_* call the four edit_*_us; the
    copy-out of either lands in its own family's slot, and a matrix call has no row order"""
    s1, s2 = _edit.aa_sets()
    read = lambda h, names: [h.get_tunable(name) for name in names]
    with HipOverlap(_edit.options_of("aa", True, device=0)) as h:
        h.hamming_neighbors(s1, s2, 3)
        hamming = read(h, HAMMING_TIMERS)
        assert h.get_tunable("hamming_copy_us") > 0
        h.edit_neighbors(s1, s2, 3)
        assert read(h, HAMMING_TIMERS) == hamming
        edit = read(h, EDIT_TIMERS)
        h.hamming_neighbors(s1, s2, 3)
        assert read(h, EDIT_TIMERS) == edit
        assert h.get_tunable("hamming_copy_us") > 0
        h.edit_matrix(s1, s2, 3)
        assert h.get_tunable("edit_copy_us") > 0 and h.get_tunable("edit_order_us") == 0


def test_a_bad_view_of_set_2_is_refused_before_the_length_of_set_1():
    """both views are looked at before either set is staged: a NULL view of set 2 is what the call answers, not the
    257 residues of set 1 that staging would refuse"""
    rng = np.random.default_rng(257)
    long = _neighbors._set_of_rows(rng.integers(0, 20, size=(1, 257), dtype=np.uint8), 2, 1)
    with HipOverlap(Options(differences=1, n_v_genes=2, n_j_genes=2, device=0)) as h:
        assert raw(h, _view(long), None, 2, 0)[0] == CMPR_EINVAL
        assert h._lib.cmpr_last_error(h._ctx).decode() == "set view is NULL"
        with pytest.raises(HipError) as e:
            h.edit_neighbors(long, long, 2)
        assert e.value.code == CMPR_EUNSUPPORTED
