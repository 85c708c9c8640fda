"""cmpr_hamming_matrix / cmpr_hamming_neighbors and their _device variants on the GPU: the CSR against the oracle's
pair list at d >= 3 and numpy distances, the matrix against the oracle's cells, the reference's own -d 3 outputs,
agreement with the hashed path at d <= 2, both forms of the compare kernel at the word and form edges and under
every staging, segment count and form, wrapping sums, the capacity protocol, the device entry points, huge d, the
resident state left alone, the refusals, determinism and empty sets.  No expectation comes from the library."""

import ctypes as C
import itertools

import numpy as np
import pytest

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
KEYS = list(_hamming.EDGES)
IDS = ["%s-d%d%s" % (k[0], k[1], "-g" if k[2] else "") for k in KEYS]


def assert_equal_edges(got, want, n1):
    assert len(got) == 3 and got[2].dtype == np.uint16
    _neighbors.assert_is_csr(got[0], got[1], n1)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


# ---- 1. CSR and matrix parity ----

@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_neighbors_against_the_oracle(key):
    name, d, g = key
    s1, s2 = _hamming.sets_of(name)
    want = _hamming.want(name, d, g)
    got = compairr_amd.hamming_neighbors(s1, s2, _hamming.options_of(name, g, device=0), d)
    print("%s d=%d g=%d: %d edges, want %d" % (name, d, g, len(got[1]), _hamming.EDGES[key]))
    assert int(got[0][-1]) == len(got[1]) == _hamming.EDGES[key]
    assert_equal_edges(got, want, s1.n)


SCORES = [dict(score="product"), dict(score="min"), dict(score="max"), dict(score="mean"),
          dict(ignore_counts=True), dict(existence=True), dict(existence=True, score="mean")]


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_matrix_against_the_oracle(key):
    name, d, g = key
    s1, s2 = _hamming.sets_of(name)
    for kw in SCORES:
        want, st = _oracle.overlap(s1, s2, _hamming.options_of(name, g, differences=d, **kw))
        assert st.matches == _hamming.EDGES[key]
        opt = _hamming.options_of(name, g, device=0, **kw)
        got = compairr_amd.hamming_matrix(s1, s2, opt, d)
        assert got.dtype == np.uint64 and got.shape == want.shape
        assert np.array_equal(got, _oracle.integer_cells(want, opt)), kw
    if name == "empty":
        assert got.shape == (200, 3)
        assert int(compairr_amd.hamming_matrix(s1, s2, _hamming.options_of(name, g, device=0, existence=True,
                                                                           ignore_counts=True), d).sum()) \
            == _hamming.EDGES[key]


def test_matrix_beyond_the_lds_copy():
    """33 x 33 repertoires: more cells than the workgroup's copy of the matrix holds -- global atomics"""
    a, b = _hamming.aa_sets()
    rng = np.random.default_rng(7)
    many = lambda s, p: RepertoireSet(s.residues, s.offsets, s.v_gene, s.j_gene,
                                      np.concatenate([np.arange(33), rng.integers(0, 33, size=s.n - 33)]).astype(np.uint32),
                                      s.count, ["%s%d" % (p, k) for k in range(33)], s.v_names, s.j_names, AA)
    a, b = many(a, "A"), many(b, "B")
    want, _ = _oracle.overlap(a, b, _hamming.options(differences=4, ignore_genes=True))
    opt = _hamming.options(ignore_genes=True, device=0)
    assert np.array_equal(compairr_amd.hamming_matrix(a, b, opt, 4), _oracle.integer_cells(want, opt))


# ---- 1b. lengths at the word and form edges; both forms ----

@pytest.mark.parametrize("nucleotides", [False, True], ids=["aa", "nt"])
@pytest.mark.parametrize("generic", [0, 1])
def test_lengths_at_the_word_and_form_edges(nucleotides, generic):
    s1, s2, _ = _hamming.edge_sets(nucleotides)
    d = _hamming.EDGE_D
    want = _hamming.oracle_want(s1, s2, _hamming.edge_options(nucleotides, differences=d))
    brute = _hamming.brute_csr(s1, s2, d)
    opt = _hamming.edge_options(nucleotides, device=0)
    got = compairr_amd.hamming_neighbors(s1, s2, opt, d, {"hamming_generic": generic})
    assert_equal_edges(got, want, s1.n)
    assert_equal_edges(got, brute, s1.n)
    cells, _ = _oracle.overlap(s1, s2, _hamming.edge_options(nucleotides, differences=d))
    assert np.array_equal(compairr_amd.hamming_matrix(s1, s2, opt, d, {"hamming_generic": generic}),
                          _oracle.integer_cells(cells, opt))


def test_a_reference_longer_than_the_staging_buffer():
    """20 000 amino acids are 5 000 packed words: the generic form stages such a reference in runs of words"""
    rng = np.random.default_rng(20)
    L = 20_000
    base = rng.integers(0, 20, size=L, dtype=np.uint8)
    rows = [base.copy() for _ in range(6)]
    for k, row in enumerate(rows):             # k substitutions, the first and the last position among them
        for p in ([0, L - 1] + [4_095 * 4 + 3, 4_096 * 4, 9_999])[:k]:
            row[p] = (row[p] + 1) % 20
    far = rng.integers(0, 20, size=L, dtype=np.uint8)
    s = _neighbors._set_of_rows(np.stack(rows + [far]), 201, 2)
    want = _hamming.brute_csr(s, s, 3)
    assert want[2].max() == 3 and 0 < len(want[1]) < s.n * s.n
    got = compairr_amd.hamming_neighbors(s, s, Options(n_v_genes=1, n_j_genes=1, device=0), 3)
    assert_equal_edges(got, want, s.n)


@pytest.mark.parametrize("d", [8, 4])
def test_every_staging_segment_count_and_form_gives_the_same_bytes(d):
    s1, s2 = _hamming.dense_sets()
    want = _hamming.want("dense", d, True)
    opt = _hamming.options_of("dense", True, device=0)
    with HipOverlap(opt) as h:
        for stage, seg, generic in itertools.product((0, 1, 63, 64, 65), (0, 1, 2, 7), (0, 1)):
            for name, value in (("hamming_stage_refs", stage), ("hamming_segments", seg), ("hamming_generic", generic)):
                h.set_tunable(name, value)
            got = h.hamming_neighbors(s1, s2, d)
            for g, w in zip(got, want):
                assert g.tobytes() == w.tobytes(), (stage, seg, generic)
        assert h.get_tunable("hamming_compare_us") > 0 and h.get_tunable("hamming_group_us") > 0
    assert len(want[1]) == _hamming.EDGES[("dense", d, True)]


# ---- 2. the reference's own d = 3 matrices ----

@pytest.mark.parametrize("name", list(_hamming.GOLDEN))
def test_reference_goldens(name):
    a, b = _hamming.golden_sets(name)
    opt = Options(n_v_genes=len(a.v_names), n_j_genes=len(a.j_names), device=0)
    got = compairr_amd.hamming_matrix(a, b, opt, 3)
    cells = _hamming.golden_cells(name)
    assert len(cells) == got.size
    for (r, c), text in cells.items():
        cell = int(got[a.repertoire_ids.index(r), b.repertoire_ids.index(c)])
        assert "%.10g" % float(cell) == text and str(cell) == text, (r, c)


# ---- 3. agreement with the hashed path ----

@pytest.mark.parametrize("name", ["aa", "nt"])
@pytest.mark.parametrize("d", [0, 1, 2])
@pytest.mark.parametrize("g", [False, True], ids=["genes", "g"])
def test_agreement_with_the_hashed_path(name, d, g):
    s1, s2 = _hamming.sets_of(name)
    with HipOverlap(_hamming.options_of(name, g, differences=d, device=0)) as h:
        h.set_reference(s2, s1.longest)
        h.set_queries(s1)
        matrix = h.overlap_matrix()
        rows, hits, dist = h.neighbors_distance()
        got_m = h.hamming_matrix(s1, s2, d)
        got = h.hamming_neighbors(s1, s2, d)
    assert np.array_equal(got_m, matrix)
    assert np.array_equal(got[0], rows) and np.array_equal(got[1], hits)
    assert np.array_equal(got[2].astype(np.int64), dist.astype(np.int64))


# ---- 4. sums wrap ----

def test_wrapping_sums():
    seqs = np.array([[1, 2, 3, 4, 5], [1, 2, 3, 4, 6], [1, 2, 9, 9, 6]], dtype=np.uint8)
    c1 = [2 ** 33 + 1, 2 ** 33 + 5, 2 ** 40 + 7]
    c2 = [2 ** 33 + 3, 2 ** 35 + 11, 2 ** 63 + 9]

    def make(counts):
        s = _neighbors._set_of_rows(seqs, 1, 1)
        s.count = np.array(counts, dtype=np.uint64)
        s.repertoire[:] = 0
        return s
    a, b = make(c1), make(c2)
    dist = (seqs[:, None, :] != seqs[None, :, :]).sum(axis=2)
    opt = Options(n_v_genes=1, n_j_genes=1, device=0)
    for d in (0, 1, 3):
        want = sum(c1[i] * c2[j] for i in range(3) for j in range(3) if dist[i, j] <= d)
        assert want >= 2 ** 64
        assert int(compairr_amd.hamming_matrix(a, b, opt, d)[0, 0]) == want % 2 ** 64
    want = sum(c1[i] + c2[j] for i in range(3) for j in range(3))
    assert int(compairr_amd.hamming_matrix(a, b, Options(n_v_genes=1, n_j_genes=1, score="mean", device=0), 5)[0, 0]) \
        == want % 2 ** 64


# ---- 5. the capacity protocol ----

def raw(h, v1, v2, d, capacity, row_start=None, hits=None, dist=None, want_count=True):
    """cmpr_hamming_neighbors as it is declared: (code, n_edges)"""
    n = C.c_uint64(12345)
    ptr = lambda a: None if a is None else a.ctypes.data
    ref = lambda v: None if v is None else C.byref(v)
    rc = h._lib.cmpr_hamming_neighbors(h._ctx, ref(v1), ref(v2), d, capacity, ptr(row_start), ptr(hits), ptr(dist),
                                       C.byref(n) if want_count else None)
    return rc, n.value


def test_capacity_protocol():
    s1, s2 = _hamming.aa_sets()
    want = _hamming.want("aa", 3, True)
    edges = len(want[1])
    v1, v2 = _view(s1), _view(s2)
    with HipOverlap(_hamming.options(ignore_genes=True, device=0)) as h:
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
        assert h.hamming_neighbors(s1, s2, 3, distances=False)[2] is None
        # refusals of the arguments
        assert raw(h, v1, v2, 3, 5, row_start, None, dist)[0] == CMPR_EINVAL
        assert "hit_out" in h._lib.cmpr_last_error(h._ctx).decode()
        assert raw(h, v1, v2, 3, edges, row_start, hits, dist, want_count=False)[0] == CMPR_EINVAL
        assert "n_edges_out" in h._lib.cmpr_last_error(h._ctx).decode()


# ---- 6. the device entry points ----

def test_device_entry_points():
    import torch
    s1, s2 = _hamming.aa_sets()
    want = _hamming.want("aa", 4, False)
    edges, n1 = len(want[1]), s1.n
    opt = _hamming.options(device=0)
    cells, _ = _oracle.overlap(s1, s2, _hamming.options(differences=4))
    with HipOverlap(opt) as h:
        v1, keep1 = HipOverlap.device_view(s1)
        v2, keep2 = HipOverlap.device_view(s2)
        d_rows = torch.full((n1 + 1 + 64,), POISON64, dtype=torch.int64, device="cuda")
        d_hits = torch.full((edges + 64,), POISON32, dtype=torch.int32, device="cuda")
        d_dist = torch.full((edges + 64,), POISON16 - 65536, dtype=torch.int16, device="cuda")
        d_mat = torch.full((s1.n_repertoires * s2.n_repertoires + 8,), POISON64, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        # count only; one short; exact
        assert h.hamming_neighbors_device(v1, v2, 4, 0, d_rows.data_ptr()) == edges
        assert np.array_equal(d_rows.cpu().numpy().view(np.uint64)[:n1 + 1], want[0])
        assert h.hamming_neighbors_device(v1, v2, 4, edges - 1, d_rows.data_ptr(), d_hits.data_ptr(),
                                          d_dist.data_ptr()) == edges
        assert (d_hits.cpu().numpy().view(np.uint32) == POISON32).all()
        assert (d_dist.cpu().numpy().view(np.uint16) == POISON16).all()
        d_rows.fill_(POISON64)
        torch.cuda.synchronize()
        assert h.hamming_neighbors_device(v1, v2, 4, edges + 10, d_rows.data_ptr(), d_hits.data_ptr(),
                                          d_dist.data_ptr()) == edges
        h.hamming_matrix_device(v1, v2, 4, d_mat.data_ptr())
        rows, hits = d_rows.cpu().numpy().view(np.uint64), d_hits.cpu().numpy().view(np.uint32)
        dist, mat = d_dist.cpu().numpy().view(np.uint16), d_mat.cpu().numpy().view(np.uint64)
        # one-file mode: the same view twice
        self_edges = h.hamming_neighbors_device(v1, v1, 4)
        host = h.hamming_neighbors(s1, s2, 4)
        del keep1, keep2
    assert_equal_edges((rows[:n1 + 1].copy(), hits[:edges].copy(), dist[:edges].copy()), want, n1)
    assert_equal_edges(host, want, n1)
    assert (rows[n1 + 1:] == POISON64).all() and (hits[edges:] == POISON32).all() and (dist[edges:] == POISON16).all()
    assert np.array_equal(mat[:-8].reshape(cells.shape), _oracle.integer_cells(cells, opt)) and (mat[-8:] == POISON64).all()
    assert self_edges == len(_neighbors.oracle_csr(s1, s1, _hamming.options(differences=4))[1])


# ---- 7. d above the longest sequence ----

@pytest.mark.parametrize("name,g", [("aa", False), ("aa", True), ("nt", True), ("dense", True), ("empty", False)])
def test_huge_d(name, g):
    s1, s2 = _hamming.sets_of(name)
    longest = max(s1.longest, s2.longest)
    groups = _hamming.same_group_pairs(s1, s2, g)
    with HipOverlap(_hamming.options_of(name, g, device=0)) as h:
        at_longest = h.hamming_neighbors(s1, s2, longest)
        for d in (70_000, 2 ** 31 - 1, 2 ** 62):
            got = h.hamming_neighbors(s1, s2, d)
            for a, b in zip(got, at_longest):
                assert np.array_equal(a, b)
    assert len(at_longest[1]) == groups
    assert np.array_equal(at_longest[2], _hamming.distances(s1, s2, at_longest[0], at_longest[1]))
    if name == "dense":
        assert groups == 630_070


# ---- 8. the resident state is left alone ----

def test_resident_state_is_left_alone():
    s1, s2 = _hamming.aa_sets()
    want = _hamming.want("aa", 3, False)
    with HipOverlap(_hamming.options(differences=1, device=0)) as h:
        h.set_reference(s2, s1.longest)
        h.set_queries(s1)
        before, matches = h.overlap_matrix(), h.stats().matches
        assert_equal_edges(h.hamming_neighbors(s1, s2, 3), want, s1.n)
        h.hamming_matrix(s1, s2, 3)
        assert h.stats().matches == matches
        assert np.array_equal(h.overlap_matrix(), before) and h.stats().matches == matches
        assert np.array_equal(h.neighbors()[0], _neighbors.oracle_csr(s1, s2, _hamming.options(differences=1))[0])
    for d in (0, 1, 2):
        with HipOverlap(_hamming.options(differences=d, device=0)) as h:
            assert_equal_edges(h.hamming_neighbors(s1, s2, 3), want, s1.n)


# ---- 9. refusals ----

def test_refusals():
    s1, s2 = _hamming.aa_sets()
    v1, v2 = _view(s1), _view(s2)
    m = np.zeros((3, 3), dtype=np.uint64)

    def both(h, d=3, a=v1, b=v2):
        ref = lambda v: None if v is None else C.byref(v)
        out = []
        for call in (lambda: raw(h, a, b, d, 0)[0],
                     lambda: h._lib.cmpr_hamming_matrix(h._ctx, ref(a), ref(b), d, m.ctypes.data)):
            out.append((call(), h._lib.cmpr_last_error(h._ctx).decode()))
        return out

    with HipOverlap(_hamming.options(device=0)) as h:
        for rc, text in both(h, d=-1):
            assert rc == CMPR_EINVAL and text == "Differences specified with -d or -differences cannot be negative."
        for a, b in ((None, v2), (v1, None)):
            for rc, text in both(h, a=a, b=b):
                assert rc == CMPR_EINVAL and text == "set view is NULL"
        h.set_tunable("work_shard_count", 2)
        for rc, text in both(h):
            assert rc == CMPR_EUNSUPPORTED and "work_shard_count" in text
    with HipOverlap(_hamming.options(differences=1, indels=True, device=0)) as h:
        for rc, text in both(h):
            assert rc == CMPR_EINVAL and "the all-against-all path has no indels" in text
    with HipOverlap(_hamming.options(score="ratio", device=0)) as h:
        (rc_n, _), (rc_m, text) = both(h)
        assert rc_n == CMPR_OK and rc_m == CMPR_EINVAL and "ratio score needs cmpr_overlap_matrix_f64" in text
    with HipOverlap(_hamming.options(score="ratio", ignore_counts=True, device=0)) as h:
        assert [rc for rc, _ in both(h)] == [CMPR_OK, CMPR_OK]
    for score in ("mh", "jaccard"):
        with HipOverlap(_hamming.options(score=score, device=0)) as h:
            for rc, text in both(h, d=1):
                assert rc == CMPR_EINVAL and text == "The Morisita-Horn / Jaccard index is not defined when d>0"
            assert [rc for rc, _ in both(h, d=0)] == [CMPR_OK, CMPR_OK]
    # a set the validation refuses: the same code and text as cmpr_set_reference
    bad = RepertoireSet(s2.residues, s2.offsets, s2.v_gene, s2.j_gene, s2.repertoire, s2.count.copy(),
                        s2.repertoire_ids, s2.v_names, s2.j_names, AA)
    bad.count[17] = 0
    with HipOverlap(_hamming.options(device=0)) as h:
        with pytest.raises(HipError) as want:
            h.set_reference(bad)
        for call in (lambda: h.hamming_neighbors(s1, bad, 3), lambda: h.hamming_matrix(bad, s2, 3)):
            with pytest.raises(HipError) as e:
                call()
            assert (e.value.code, str(e.value)) == (want.value.code, str(want.value))
        assert_equal_edges(h.hamming_neighbors(s1, s2, 3), _hamming.want("aa", 3, False), s1.n)


# ---- 10. determinism; empty sets ----

def test_two_runs_give_the_same_bytes():
    s1, s2 = _hamming.dense_sets()
    opt = _hamming.options_of("dense", False, device=0)
    one = compairr_amd.hamming_neighbors(s1, s2, opt, 4)
    two = compairr_amd.hamming_neighbors(s1, s2, opt, 4)
    assert [a.tobytes() for a in one] == [b.tobytes() for b in two]
    assert compairr_amd.hamming_matrix(s1, s2, opt, 4).tobytes() == compairr_amd.hamming_matrix(s1, s2, opt, 4).tobytes()


def test_empty_sets():
    z = lambda t: np.zeros(0, dtype=t)
    s = _hamming.aa_sets()[0]
    empty = RepertoireSet(z(np.uint8), np.zeros(1, dtype=np.uint64), z(np.uint32), z(np.uint32), z(np.uint32),
                          z(np.uint64), ["T1", "T2"], ["V0", "V1"], ["J0", "J1"], AA)
    with HipOverlap(_hamming.options(device=0)) as h:
        rows, hits, dist = h.hamming_neighbors(empty, s, 3)
        assert rows.tolist() == [0] and len(hits) == 0 and len(dist) == 0
        rows, hits, dist = h.hamming_neighbors(s, empty, 3)
        assert rows.tolist() == [0] * (s.n + 1) and len(hits) == 0
        m = np.full((2, 3), 7, dtype=np.uint64)
        v_e, v_s = _view(empty), _view(s)
        assert h._lib.cmpr_hamming_matrix(h._ctx, C.byref(v_e), C.byref(v_s), 3, m.ctypes.data) == CMPR_OK
        assert not m.any()
        m = np.full((3, 2), 7, dtype=np.uint64)
        assert h._lib.cmpr_hamming_matrix(h._ctx, C.byref(v_s), C.byref(v_e), 3, m.ctypes.data) == CMPR_OK
        assert not m.any()
        assert h.hamming_neighbors(empty, empty, 3)[0].tolist() == [0]
