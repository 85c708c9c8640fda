"""cmpr_tcrdist_neighbors / cmpr_tcrdist_matrix and their _device variants on the GPU: the CSR and the matrix against
the numpy brute force of the definition (tests/_tcrdist.py) on every input and case of the issue, an asymmetric table
and its transpose law, agreement with cmpr_hamming_neighbors under unit weights, the V table, the lengths at which
the query forms change, workgroups, staged pieces and long rows, the job table with a skipped group, the same bytes
under every tunable, wrapping sums, the capacity protocol, the device entry points, empty sets, determinism, the
resident state left alone and every refusal.  No expectation comes from the library."""

import ctypes as C

import numpy as np
import pytest

import _edit
import _neighbors
import _tcrdist
import compairr_amd
from _tcrdist import FIXED, SLIDING
from compairr_amd import HipError, HipOverlap, Options, RepertoireSet, TcrdistParams, synth
from compairr_amd.hip import _view
from compairr_amd.sets import AA

pytestmark = pytest.mark.gpu

CMPR_OK, CMPR_EINVAL, CMPR_EUNSUPPORTED = 0, 1, 4
POISON16, POISON32, POISON64 = 0xA5A5, 0x25A5A5A5, 0x25A5A5A525A5A5A5
# (the list of tests/test_edit_gpu.py)
SCORES = [dict(score="product"), dict(score="min"), dict(score="max"), dict(score="mean"),
          dict(ignore_counts=True), dict(existence=True), dict(existence=True, score="mean")]


def params_of(case, W=None, V=None):
    ntrim, ctrim, gap, mode, _ = _tcrdist.CASES[case]
    return TcrdistParams(_tcrdist.table() if W is None else W, gap, ntrim, ctrim, mode, v_distance=V)


def assert_equal_edges(got, want, n1):
    assert len(got) == 3 and got[2].dtype == np.uint16
    _neighbors.assert_is_csr(got[0], got[1], n1)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


# ---- 1. CSR and matrix parity ----

@pytest.mark.parametrize("key", _tcrdist.KEYS, ids=_tcrdist.IDS)
def test_neighbors_against_the_brute_force(key):
    name, case, g = key
    s1, s2 = _tcrdist.sets_of(name)
    want = _tcrdist.want(name, case, g)
    got = compairr_amd.tcrdist_neighbors(s1, s2, _tcrdist.options(ignore_genes=g, device=0), params_of(case),
                                         _tcrdist.CASES[case][4])
    print("%s case %d g=%d: %d edges, want %d" % (name, case, g, len(got[1]), _tcrdist.EDGES[key]))
    assert int(got[0][-1]) == len(got[1]) == _tcrdist.EDGES[key]
    assert_equal_edges(got, want, s1.n)


@pytest.mark.parametrize("key", _tcrdist.KEYS, ids=_tcrdist.IDS)
def test_matrix_against_the_brute_force(key):
    name, case, g = key
    s1, s2 = _tcrdist.sets_of(name)
    rows, hits, _ = _tcrdist.want(name, case, g)
    for kw in SCORES:
        opt = _tcrdist.options(ignore_genes=g, device=0, **kw)
        got = compairr_amd.tcrdist_matrix(s1, s2, opt, params_of(case), _tcrdist.CASES[case][4])
        want = _edit.matrix_of(s1, s2, rows, hits, opt)
        assert got.dtype == np.uint64 and got.shape == want.shape
        assert np.array_equal(got, want), kw


def test_matrix_beyond_the_lds_copy():
    """33 x 33 repertoires: more cells than the workgroup's copy of the matrix holds -- global atomics"""
    a, b = _tcrdist.tiny_sets()
    rng = np.random.default_rng(7)
    many = lambda s, p: RepertoireSet(s.residues, s.offsets, s.v_gene, s.j_gene,
                                      np.concatenate([np.arange(33), rng.integers(0, 33, size=s.n - 33)]).astype(np.uint32),
                                      s.count, ["%s%d" % (p, k) for k in range(33)], s.v_names, s.j_names, s.alphabet)
    a, b = many(a, "A"), many(b, "B")
    rows, hits, _ = _tcrdist.want("tiny", 1, True)
    opt = _tcrdist.options(ignore_genes=True, device=0)
    assert np.array_equal(compairr_amd.tcrdist_matrix(a, b, opt, params_of(1), 6), _edit.matrix_of(a, b, rows, hits, opt))


def test_wrapping_sums():
    seqs = [[1, 2, 3, 4, 5], [1, 2, 3, 4], [2, 3, 4, 5, 6, 7]]
    c1 = [2 ** 33 + 1, 2 ** 33 + 5, 2 ** 40 + 7]
    c2 = [2 ** 33 + 3, 2 ** 35 + 11, 2 ** 63 + 9]

    def make(counts):
        off = np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)
        n = len(seqs)
        return RepertoireSet(np.concatenate(seqs).astype(np.uint8), off, np.zeros(n, dtype=np.uint32),
                             np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32),
                             np.array(counts, dtype=np.uint64), ["R1"], ["V0"], ["J0"], AA)
    a, b = make(c1), make(c2)
    p = TcrdistParams(_tcrdist.table(), 0, 0, 0, SLIDING)
    rows, hits, _ = _tcrdist.brute_csr(a, b, _tcrdist.table(), 0, 0, 0, SLIDING, 1000)
    assert len(hits) == 9                                   # every pair, at no gap penalty and a cutoff above all
    want = sum(c1[i] * c2[int(j)] for i, j in zip(_edit.queries_of(rows), hits))
    assert want >= 2 ** 64
    assert int(compairr_amd.tcrdist_matrix(a, b, Options(device=0), p, 1000)[0, 0]) == want % 2 ** 64
    want = sum(c1[i] + c2[j] for i in range(3) for j in range(3))
    assert int(compairr_amd.tcrdist_matrix(a, b, Options(score="mean", device=0), p, 1000)[0, 0]) == want % 2 ** 64


# ---- 2. an asymmetric table ----

def asymmetric_table():
    i, j = np.indices((20, 20))
    return ((3 * i + 7 * j) % 5 + (i != j)).astype(np.uint8)


@pytest.mark.parametrize("name", ["tiny", "mid"])
@pytest.mark.parametrize("mode", [FIXED, SLIDING], ids=["fixed", "sliding"])
def test_asymmetric_table_and_the_transpose_law(name, mode):
    s1, s2 = _tcrdist.sets_of(name)
    W2 = asymmetric_table()
    assert not np.array_equal(W2, W2.T)
    cutoff = 9
    want = _tcrdist.brute_csr(s1, s2, W2, 3, 2, 4, mode, cutoff, True)
    assert 0 < len(want[1]) < s1.n * s2.n and _edit.cross_length(s1, s2, want[0], want[1]) > 0
    with HipOverlap(_tcrdist.options(ignore_genes=True, device=0)) as h:
        got = h.tcrdist_neighbors(s1, s2, TcrdistParams(W2, 4, 3, 2, mode), cutoff)
        back = h.tcrdist_neighbors(s2, s1, TcrdistParams(W2.T, 4, 3, 2, mode), cutoff)
    assert_equal_edges(got, want, s1.n)
    # (set2, set1, W2 transposed): the same edges with their ends swapped, at the same distances
    there = sorted(zip(_edit.queries_of(got[0]).tolist(), got[1].tolist(), got[2].tolist()))
    here = sorted(zip(back[1].tolist(), _edit.queries_of(back[0]).tolist(), back[2].tolist()))
    assert there == here
    # and the table does matter: its transpose on the same sets gives other edges
    other = _tcrdist.brute_csr(s1, s2, W2.T, 3, 2, 4, mode, cutoff, True)
    assert there != sorted(zip(_edit.queries_of(other[0]).tolist(), other[1].tolist(), other[2].tolist()))


# ---- 3. agreement with the Hamming kernel under unit weights ----

@pytest.mark.parametrize("name", ["tiny", "aa"])
@pytest.mark.parametrize("g", [False, True], ids=["genes", "g"])
@pytest.mark.parametrize("cutoff", [0, 3])
def test_agreement_with_the_hamming_path(name, g, cutoff):
    """(the mid input has no two sequences of one length within three substitutions: the sets of the edit tests
    stand in, 300 sequences of 1 .. 9 residues against themselves)"""
    s1, s2 = _tcrdist.tiny_sets() if name == "tiny" else _edit.aa_sets()
    unit = (np.arange(20)[:, None] != np.arange(20)[None, :]).astype(np.uint8)
    with HipOverlap(_tcrdist.options(ignore_genes=g, device=0)) as h:
        want = h.hamming_neighbors(s1, s2, cutoff)
        for mode in (FIXED, SLIDING):
            got = h.tcrdist_neighbors(s1, s2, TcrdistParams(unit, cutoff + 1, 0, 0, mode), cutoff)
            assert len(got[1]) > 0
            for a, b in zip(got, want):
                assert a.tobytes() == b.tobytes()


# ---- 4. the V table ----

def v_sets():
    kw = dict(letters=3, min_len=4, max_len=9, n_v=3, n_j=2)
    return synth.tiny_set(150, 43, **kw), synth.tiny_set(140, 44, **kw)


V_TABLE = np.array([[0, 2, 50], [3, 0, 1], [50, 4, 1]], dtype=np.uint16)   # asymmetric; 50 is above the cutoff


@pytest.mark.parametrize("mode", [FIXED, SLIDING], ids=["fixed", "sliding"])
def test_v_table(mode):
    s1, s2 = v_sets()
    cutoff = 7
    opt = Options(n_v_genes=3, n_j_genes=2, device=0)
    want = _tcrdist.brute_csr(s1, s2, _tcrdist.table(), 3, 2, 4, mode, cutoff, V=V_TABLE)
    q, hits = _edit.queries_of(want[0]), want[1].astype(np.int64)
    v1, v2 = s1.v_gene[q].astype(np.int64), s2.v_gene[hits].astype(np.int64)
    # pairs across V at both asymmetric prices, a (V, V) pair at a price on the diagonal, pairs across J, and no
    # pair of the two V genes the table puts above the cutoff, though both sets hold them
    for a, b in ((0, 1), (1, 0), (1, 2), (2, 1), (2, 2)):
        assert ((v1 == a) & (v2 == b)).any(), (a, b)
    assert not ((v1 == 0) & (v2 == 2)).any() and not ((v1 == 2) & (v2 == 0)).any()
    assert (s1.v_gene == 0).any() and (s2.v_gene == 2).any()
    assert (s1.j_gene[q] != s2.j_gene[hits]).any()
    assert (want[2].astype(np.int64) >= V_TABLE[v1, v2]).all()
    p = TcrdistParams(_tcrdist.table(), 4, 3, 2, mode, v_distance=V_TABLE)
    with HipOverlap(opt) as h:
        assert_equal_edges(h.tcrdist_neighbors(s1, s2, p, cutoff), want, s1.n)
        assert np.array_equal(h.tcrdist_matrix(s1, s2, p, cutoff), _edit.matrix_of(s1, s2, want[0], want[1], opt))
        # one-file mode: the (i, i) pairs at the diagonal's price -- V2 against itself costs 1
        self_want = _tcrdist.brute_csr(s1, s1, _tcrdist.table(), 3, 2, 4, mode, cutoff, V=V_TABLE)
        assert_equal_edges(h.tcrdist_neighbors(s1, s1, p, cutoff), self_want, s1.n)
    with HipOverlap(Options(n_v_genes=3, n_j_genes=2, ignore_genes=True, device=0)) as h:
        with pytest.raises(HipError) as e:
            h.tcrdist_neighbors(s1, s2, p, cutoff)
        assert e.value.code == CMPR_EINVAL and "v_distance with options.ignore_genes" in str(e.value)
        with pytest.raises(HipError) as e:
            h.tcrdist_matrix(s1, s2, p, cutoff)
        assert e.value.code == CMPR_EINVAL and "v_distance with options.ignore_genes" in str(e.value)


# ---- 5. the lengths at which the query forms change ----

@pytest.mark.parametrize("mode", [FIXED, SLIDING], ids=["fixed", "sliding"])
@pytest.mark.parametrize("trims", [(3, 2), (0, 0)], ids=["trim32", "trim00"])
def test_lengths_at_the_form_edges(mode, trims):
    """every length of 0..6, 15..17, 31..33, 63..65, 127..129, 255, 256 as query and as reference: the register forms
    of 2, 4, 8 and 16 words and the generic form, each against shorter, equal and longer references"""
    s1, s2 = _tcrdist.edge_sets()
    gap, cutoff = _tcrdist.EDGE_GAP, _tcrdist.EDGE_CUTOFF
    opt = Options(device=0)
    p = TcrdistParams(_tcrdist.table(), gap, trims[0], trims[1], mode)
    with HipOverlap(opt) as h:
        for a, b in ((s1, s2), (s2, s1)):
            want = _tcrdist.brute_csr(a, b, _tcrdist.table(), trims[0], trims[1], gap, mode, cutoff)
            q, hits = _edit.queries_of(want[0]), want[1].astype(np.int64)
            la, lb = a.lengths[q].astype(np.int64), b.lengths[hits].astype(np.int64)
            assert 0 < len(hits) < a.n * b.n
            # an edge from every length, and across lengths on either side of 64 residues in both directions
            assert set(la.tolist()) == set(_tcrdist.EDGE_LENGTHS)
            for lo, hi in ((0, 64), (65, 256)):
                assert ((la < lb) & (la >= lo) & (lb <= hi)).any() and ((la > lb) & (lb >= lo) & (la <= hi)).any()
            assert ((la <= 64) & (lb > 64)).any() and ((la > 64) & (lb <= 64)).any()
            assert_equal_edges(h.tcrdist_neighbors(a, b, p, cutoff), want, a.n)
            assert np.array_equal(h.tcrdist_matrix(a, b, p, cutoff), _edit.matrix_of(a, b, want[0], want[1], opt))


def test_the_length_limit():
    """one sequence of 257 residues: refused with code and text, whichever set holds it; the resident state unharmed"""
    rng = np.random.default_rng(257)
    ok = _neighbors._set_of_rows(rng.integers(0, 20, size=(5, 256), dtype=np.uint8), 1, 2)
    long = _neighbors._set_of_rows(rng.integers(0, 20, size=(1, 257), dtype=np.uint8), 2, 1)
    s1, s2 = _edit.aa_sets()
    p = params_of(1)
    with HipOverlap(Options(differences=1, n_v_genes=2, n_j_genes=2, device=0)) as h:
        h.set_reference(s2, s1.longest)
        h.set_queries(s1)
        before, matches = h.overlap_matrix(), h.stats().matches
        for call in (lambda: h.tcrdist_neighbors(ok, long, p, 6), lambda: h.tcrdist_neighbors(long, ok, p, 6),
                     lambda: h.tcrdist_matrix(long, long, p, 6), lambda: h.tcrdist_matrix(ok, long, p, 6)):
            with pytest.raises(HipError) as e:
                call()
            assert e.value.code == CMPR_EUNSUPPORTED
            assert str(e.value).endswith("cmpr_tcrdist: a sequence of more than 256 residues")
        assert np.array_equal(h.overlap_matrix(), before) and h.stats().matches == matches
        want = _tcrdist.brute_csr(ok, ok, _tcrdist.table(), 3, 2, 4, SLIDING, 6, True)
        assert_equal_edges(h.tcrdist_neighbors(ok, ok, p, 6), want, ok.n)


# ---- 6. shapes ----

def near_stem(n, L, seed, changes):
    """n sequences of L residues: one stem with up to `changes` residues replaced"""
    rng = np.random.default_rng(seed)
    stem = rng.integers(0, 20, size=L, dtype=np.uint8)
    rows = np.tile(stem, (n, 1))
    for _ in range(changes):
        rows[np.arange(n), rng.integers(0, L, size=n)] = rng.integers(0, 20, size=n, dtype=np.uint8)
    return rows


def test_one_large_group():
    """one group of 700 sequences against itself: three workgroups per job, two staged pieces per partner, rows of
    more than 64 hits; the same bytes from every staging and segment count"""
    s = _neighbors._set_of_rows(near_stem(700, 14, 61, 4), 61, 3)
    p, cutoff = TcrdistParams(_tcrdist.table(), 4, 3, 2, SLIDING), 7
    want = _tcrdist.brute_csr(s, s, _tcrdist.table(), 3, 2, 4, SLIDING, cutoff)
    assert int(np.diff(want[0].astype(np.int64)).max()) > 64 and len(want[1]) < 700 * 700
    opt = Options(device=0)
    m_want = _edit.matrix_of(s, s, want[0], want[1], opt)
    with HipOverlap(opt) as h:
        assert_equal_edges(h.tcrdist_neighbors(s, s, p, cutoff), want, s.n)
        assert np.array_equal(h.tcrdist_matrix(s, s, p, cutoff), m_want)
        for stage, seg in [(k, 0) for k in (1, 2, 63, 64, 65)] + [(0, k) for k in (1, 2, 3, 64)] + [(65, 3)]:
            h.set_tunable("tcrdist_stage_refs", stage)
            h.set_tunable("tcrdist_segments", seg)
            for g, w in zip(h.tcrdist_neighbors(s, s, p, cutoff), want):
                assert g.tobytes() == w.tobytes(), (stage, seg)
            assert h.tcrdist_matrix(s, s, p, cutoff).tobytes() == m_want.tobytes(), (stage, seg)
        for name, bad in (("tcrdist_segments", 65), ("tcrdist_stage_refs", -1)):
            with pytest.raises(HipError) as e:
                h.set_tunable(name, bad)
            assert e.value.code == CMPR_EINVAL


def job_table_sets():
    """one stem of 70 residues over two letters that cost 1 against each other under table(); every sequence a prefix
    of it with two residues replaced at random, the rows shuffled.  (length, count) per set: at gap penalty 4 and cutoff
    7 a length pairs with itself and its neighbours only, so set 1's length 11 has no partner in set 2"""
    W = _tcrdist.table()
    rng = np.random.default_rng(2600)
    stem = np.array([0, int(np.nonzero(W[0] == 1)[0][0])], dtype=np.uint8)[rng.integers(0, 2, size=70)]

    def rows(shape):
        out = []
        for n, count in shape:
            for _ in range(count):
                r = stem[:n].copy()
                r[rng.integers(0, n, size=2)] = rng.integers(0, 20, size=2, dtype=np.uint8)
                out.append(r)
        return [out[k] for k in rng.permutation(len(out))]
    return (_tcrdist.hand_set(rows(((8, 40), (11, 30), (14, 600), (20, 50), (70, 20))), 261),
            _tcrdist.hand_set(rows(((8, 30), (9, 30), (14, 300), (15, 40), (20, 40), (70, 20))), 262))


@pytest.mark.parametrize("mode", [FIXED, SLIDING], ids=["fixed", "sliding"])
def test_the_job_table(mode):
    """in one call: a set-1 group without partners (length 11) between two jobs, a job of three workgroups (length 14)
    that is not the first, and runs of the forms 2, 4, 8 and generic (lengths 8, 14, 20, 70) -- what the job table, its
    runs and the search of a workgroup's job must get right together"""
    s1, s2 = job_table_sets()
    cutoff = 7
    want = _tcrdist.brute_csr(s1, s2, _tcrdist.table(), 3, 2, 4, mode, cutoff)
    q, hits = _edit.queries_of(want[0]), want[1].astype(np.int64)
    la, lb = s1.lengths[q].astype(np.int64), s2.lengths[hits].astype(np.int64)
    print("job table, mode %d: %d edges of %d pairs, per set-1 length %s, %d across lengths" % (
        mode, len(hits), s1.n * s2.n, {n: int((la == n).sum()) for n in (8, 11, 14, 20, 70)}, int((la != lb).sum())))
    for n in (8, 14, 20, 70):
        assert (la == n).any(), n
    assert not (la == 11).any() and (s1.lengths == 11).any()
    assert (la != lb).any() and len(hits) < s1.n * s2.n
    opt = Options(device=0)
    p = TcrdistParams(_tcrdist.table(), 4, 3, 2, mode)
    m_want = _edit.matrix_of(s1, s2, want[0], want[1], opt)
    with HipOverlap(opt) as h:
        assert_equal_edges(h.tcrdist_neighbors(s1, s2, p, cutoff), want, s1.n)
        assert np.array_equal(h.tcrdist_matrix(s1, s2, p, cutoff), m_want)
        h.set_tunable("tcrdist_segments", 3)
        h.set_tunable("tcrdist_stage_refs", 65)
        for g, w in zip(h.tcrdist_neighbors(s1, s2, p, cutoff), want):
            assert g.tobytes() == w.tobytes()
        assert h.tcrdist_matrix(s1, s2, p, cutoff).tobytes() == m_want.tobytes()


@pytest.mark.parametrize("key", [("tiny", 1, True), ("mid", 2, False), ("tiny", 3, True)], ids=["tiny", "mid", "gap0"])
def test_every_tunable_gives_the_same_bytes(key):
    name, case, g = key
    s1, s2 = _tcrdist.sets_of(name)
    want = _tcrdist.want(name, case, g)
    opt = _tcrdist.options(ignore_genes=g, device=0)
    m_want = _edit.matrix_of(s1, s2, want[0], want[1], opt)
    p, cutoff = params_of(case), _tcrdist.CASES[case][4]
    with HipOverlap(opt) as h:
        for stage in (0, 1, 2, 63, 64, 65):
            for seg in (0, 1, 2, 3, 64):
                h.set_tunable("tcrdist_stage_refs", stage)
                h.set_tunable("tcrdist_segments", seg)
                for a, b in zip(h.tcrdist_neighbors(s1, s2, p, cutoff), want):
                    assert a.tobytes() == b.tobytes(), (stage, seg)
                assert h.tcrdist_matrix(s1, s2, p, cutoff).tobytes() == m_want.tobytes(), (stage, seg)


def test_rows_beyond_lds():
    """a few queries against 9 000 references, all but 300 of them near one stem: rows of more than 8 192 hits, put
    in order by the device-wide sort; with and without distances"""
    rows = near_stem(9000, 12, 71, 2)
    rows[100:400] = np.random.default_rng(73).integers(0, 20, size=(300, 12), dtype=np.uint8)
    ref = _neighbors._set_of_rows(rows, 71, 3)
    qry = _neighbors._set_of_rows(near_stem(5, 12, 71, 1), 72, 2)
    p, cutoff = TcrdistParams(_tcrdist.table(), 4, 0, 0, FIXED), 13
    want = _tcrdist.brute_csr(qry, ref, _tcrdist.table(), 0, 0, 4, FIXED, cutoff)
    assert int(np.diff(want[0].astype(np.int64)).max()) > 8192 and len(want[1]) < 5 * 9000
    with HipOverlap(Options(device=0)) as h:
        assert_equal_edges(h.tcrdist_neighbors(qry, ref, p, cutoff), want, qry.n)
        rows, hits, none = h.tcrdist_neighbors(qry, ref, p, cutoff, distances=False)
        assert none is None and np.array_equal(rows, want[0]) and np.array_equal(hits, want[1])
        h.set_tunable("tcrdist_segments", 7)
        assert_equal_edges(h.tcrdist_neighbors(qry, ref, p, cutoff), want, qry.n)


# ---- 7. the protocol ----

def raw(h, v1, v2, t, cutoff, capacity, row_start=None, hits=None, dist=None, want_count=True):
    """cmpr_tcrdist_neighbors as it is declared: (code, n_edges)"""
    n = C.c_uint64(12345)
    ptr = lambda a: None if a is None else a.ctypes.data
    ref = lambda v: None if v is None else C.byref(v)
    rc = h._lib.cmpr_tcrdist_neighbors(h._ctx, ref(v1), ref(v2), ref(t), cutoff, capacity, ptr(row_start), ptr(hits),
                                       ptr(dist), C.byref(n) if want_count else None)
    return rc, n.value


def test_capacity_protocol():
    s1, s2 = _tcrdist.tiny_sets()
    want = _tcrdist.want("tiny", 1, True)
    edges = len(want[1])
    v1, v2 = _view(s1), _view(s2)
    p = params_of(1)
    with HipOverlap(_tcrdist.options(ignore_genes=True, device=0)) as h:
        t = p.struct(h.opt)
        # count only
        assert raw(h, v1, v2, t, 6, 0) == (CMPR_OK, edges)
        row_start = np.full(s1.n + 1, 7, dtype=np.uint64)
        assert raw(h, v1, v2, t, 6, 0, row_start) == (CMPR_OK, edges)
        assert np.array_equal(row_start, want[0])
        # one short: row_start exact, nothing written to either array
        row_start[:] = 7
        hits = np.full(edges, POISON32, dtype=np.uint32)
        dist = np.full(edges, POISON16, dtype=np.uint16)
        assert raw(h, v1, v2, t, 6, edges - 1, row_start, hits, dist) == (CMPR_OK, edges)
        assert np.array_equal(row_start, want[0])
        assert (hits == POISON32).all() and (dist == POISON16).all()
        # exact
        row_start[:] = 7
        assert raw(h, v1, v2, t, 6, edges, row_start, hits, dist) == (CMPR_OK, edges)
        assert_equal_edges((row_start, hits, dist), want, s1.n)
        # generous: what lies behind the edges is not the call's to write
        roomy_h = np.full(edges + 100, POISON32, dtype=np.uint32)
        roomy_d = np.full(edges + 100, POISON16, dtype=np.uint16)
        assert raw(h, v1, v2, t, 6, edges + 100, None, roomy_h, roomy_d) == (CMPR_OK, edges)
        assert np.array_equal(roomy_h[:edges], want[1]) and (roomy_h[edges:] == POISON32).all()
        assert np.array_equal(roomy_d[:edges], want[2]) and (roomy_d[edges:] == POISON16).all()
        # hits only: distance_out NULL
        only = np.full(edges, POISON32, dtype=np.uint32)
        assert raw(h, v1, v2, t, 6, edges, None, only, None) == (CMPR_OK, edges)
        assert np.array_equal(only, want[1])
        assert h.tcrdist_neighbors(s1, s2, p, 6, distances=False)[2] is None
        # refusals of the arguments
        assert raw(h, v1, v2, t, 6, 5, row_start, None, dist)[0] == CMPR_EINVAL
        assert "hit_out" in h._lib.cmpr_last_error(h._ctx).decode()
        assert raw(h, v1, v2, t, 6, edges, row_start, hits, dist, want_count=False)[0] == CMPR_EINVAL
        assert "n_edges_out" in h._lib.cmpr_last_error(h._ctx).decode()
        # the four timers are the call's own
        h.tcrdist_neighbors(s1, s2, p, 6)
        assert all(h.get_tunable("tcrdist_%s_us" % k) > 0 for k in ("group", "compare", "order", "copy"))
        h.tcrdist_matrix(s1, s2, p, 6)
        assert h.get_tunable("tcrdist_copy_us") > 0 and h.get_tunable("tcrdist_order_us") == 0


def test_device_entry_points():
    import torch
    s1, s2 = _tcrdist.mid_sets()
    want = _tcrdist.want("mid", 1, False)
    edges, n1 = len(want[1]), s1.n
    opt = _tcrdist.options(device=0)
    m_want = _edit.matrix_of(s1, s2, want[0], want[1], opt)
    p = params_of(1)
    with HipOverlap(opt) as h:
        v1, keep1 = HipOverlap.device_view(s1)
        v2, keep2 = HipOverlap.device_view(s2)
        d_rows = torch.full((n1 + 1 + 64,), POISON64, dtype=torch.int64, device="cuda")
        d_hits = torch.full((edges + 64,), POISON32, dtype=torch.int32, device="cuda")
        d_dist = torch.full((edges + 64,), POISON16 - 65536, dtype=torch.int16, device="cuda")
        d_mat = torch.full((s1.n_repertoires * s2.n_repertoires + 8,), POISON64, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        # count only; one short; exact
        assert h.tcrdist_neighbors_device(v1, v2, p, 6, 0, d_rows.data_ptr()) == edges
        assert np.array_equal(d_rows.cpu().numpy().view(np.uint64)[:n1 + 1], want[0])
        assert h.tcrdist_neighbors_device(v1, v2, p, 6, edges - 1, d_rows.data_ptr(), d_hits.data_ptr(),
                                          d_dist.data_ptr()) == edges
        assert (d_hits.cpu().numpy().view(np.uint32) == POISON32).all()
        assert (d_dist.cpu().numpy().view(np.uint16) == POISON16).all()
        d_rows.fill_(POISON64)
        torch.cuda.synchronize()
        assert h.tcrdist_neighbors_device(v1, v2, p, 6, edges + 10, d_rows.data_ptr(), d_hits.data_ptr(),
                                          d_dist.data_ptr()) == edges
        h.tcrdist_matrix_device(v1, v2, p, 6, d_mat.data_ptr())
        rows, hits = d_rows.cpu().numpy().view(np.uint64), d_hits.cpu().numpy().view(np.uint32)
        dist, mat = d_dist.cpu().numpy().view(np.uint16), d_mat.cpu().numpy().view(np.uint64)
        # hits only, no row_start: the rows are put in order all the same
        d_only = torch.full((edges,), POISON32, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert h.tcrdist_neighbors_device(v1, v2, p, 6, edges, 0, d_only.data_ptr()) == edges
        only = d_only.cpu().numpy().view(np.uint32)
        # one-file mode: the same view twice
        self_edges = h.tcrdist_neighbors_device(v1, v1, p, 6)
        del keep1, keep2
    assert_equal_edges((rows[:n1 + 1].copy(), hits[:edges].copy(), dist[:edges].copy()), want, n1)
    assert np.array_equal(only, want[1])
    assert (rows[n1 + 1:] == POISON64).all() and (hits[edges:] == POISON32).all() and (dist[edges:] == POISON16).all()
    assert np.array_equal(mat[:-8].reshape(m_want.shape), m_want) and (mat[-8:] == POISON64).all()
    assert self_edges == len(_tcrdist.brute_csr(s1, s1, _tcrdist.table(), 3, 2, 4, SLIDING, 6)[1])


def test_empty_sets():
    z = lambda t: np.zeros(0, dtype=t)
    s = _tcrdist.tiny_sets()[0]
    empty = RepertoireSet(z(np.uint8), np.zeros(1, dtype=np.uint64), z(np.uint32), z(np.uint32), z(np.uint32),
                          z(np.uint64), ["T1", "T2"], ["V0", "V1"], ["J0", "J1"], AA)
    p = params_of(1)
    with HipOverlap(_tcrdist.options(device=0)) as h:
        rows, hits, dist = h.tcrdist_neighbors(empty, s, p, 6)
        assert rows.tolist() == [0] and len(hits) == 0 and len(dist) == 0
        rows, hits, dist = h.tcrdist_neighbors(s, empty, p, 6)
        assert rows.tolist() == [0] * (s.n + 1) and len(hits) == 0
        assert not h.tcrdist_matrix(empty, s, p, 6).any() and h.tcrdist_matrix(empty, s, p, 6).shape == (2, 3)
        assert not h.tcrdist_matrix(s, empty, p, 6).any()
        assert h.tcrdist_neighbors(empty, empty, p, 6)[0].tolist() == [0]


def test_two_runs_give_the_same_bytes():
    s1, s2 = _tcrdist.tiny_sets()
    opt = _tcrdist.options(ignore_genes=True, device=0)
    p = params_of(3)
    one = compairr_amd.tcrdist_neighbors(s1, s2, opt, p, 4)
    two = compairr_amd.tcrdist_neighbors(s1, s2, opt, p, 4)
    assert [a.tobytes() for a in one] == [b.tobytes() for b in two]
    assert compairr_amd.tcrdist_matrix(s1, s2, opt, p, 4).tobytes() == compairr_amd.tcrdist_matrix(s1, s2, opt, p, 4).tobytes()


def test_resident_state_is_left_alone():
    """resident sets, statistics and the timers of the other families are as before a call in between; the context's
    own differences play no part"""
    s1, s2 = _tcrdist.mid_sets()
    want = _tcrdist.want("mid", 1, False)
    p = params_of(1)
    with HipOverlap(_tcrdist.options(differences=1, device=0)) as h:
        h.set_reference(s2, s1.longest)
        h.set_queries(s1)
        before, matches = h.overlap_matrix(), h.stats().matches
        h.edit_neighbors(s1, s2, 2)
        h.hamming_neighbors(s1, s2, 2)
        timers = [h.get_tunable(n) for n in ("edit_group_us", "edit_compare_us", "edit_order_us", "edit_copy_us",
                                             "hamming_group_us", "hamming_compare_us", "hamming_copy_us")]
        assert_equal_edges(h.tcrdist_neighbors(s1, s2, p, 6), want, s1.n)
        h.tcrdist_matrix(s1, s2, p, 6)
        assert timers == [h.get_tunable(n) for n in ("edit_group_us", "edit_compare_us", "edit_order_us", "edit_copy_us",
                                                     "hamming_group_us", "hamming_compare_us", "hamming_copy_us")]
        assert h.stats().matches == matches
        assert np.array_equal(h.overlap_matrix(), before) and h.stats().matches == matches


def test_refusals():
    s1, s2 = _tcrdist.tiny_sets()
    v1, v2 = _view(s1), _view(s2)
    m = np.zeros((3, 3), dtype=np.uint64)
    p = params_of(1)
    aa = lambda **kw: _tcrdist.options(device=0, **kw)

    def both(h, cutoff=6, a=v1, b=v2, t=-1):
        ref = lambda v: None if v is None else C.byref(v)
        t = p.struct(h.opt) if t == -1 else t
        out = []
        for call in (lambda: raw(h, a, b, t, cutoff, 0)[0],
                     lambda: h._lib.cmpr_tcrdist_matrix(h._ctx, ref(a), ref(b), ref(t), cutoff, m.ctypes.data)):
            out.append((call(), h._lib.cmpr_last_error(h._ctx).decode()))
        return out

    with HipOverlap(aa()) as h:
        for rc, text in both(h, cutoff=-1):
            assert rc == CMPR_EINVAL and text == "Differences specified with -d or -differences cannot be negative."
        for a, b in ((None, v2), (v1, None)):
            for rc, text in both(h, a=a, b=b):
                assert rc == CMPR_EINVAL and text == "set view is NULL"
        for rc, text in both(h, t=None):
            assert rc == CMPR_EINVAL and text.endswith("params is NULL")
        t = p.struct(h.opt)
        t.substitution = None
        for rc, text in both(h, t=t):
            assert rc == CMPR_EINVAL and text.endswith("params->substitution is NULL")
        for rc, text in both(h, cutoff=65536):
            assert rc == CMPR_EINVAL and "cutoff above 65535" in text
        assert [rc for rc, _ in both(h, cutoff=65535)] == [CMPR_OK, CMPR_OK]
        for word in range(4):
            t = p.struct(h.opt)
            t.reserved[word] = 1
            for rc, text in both(h, t=t):
                assert rc == CMPR_EINVAL and text.endswith("params->reserved must be zero")
        t = p.struct(h.opt)
        t.gap_mode = 2
        for rc, text in both(h, t=t):
            assert rc == CMPR_EINVAL and "gap_mode" in text
        h.set_tunable("work_shard_count", 2)
        for rc, text in both(h):
            assert rc == CMPR_EUNSUPPORTED and "work_shard_count" in text
    with HipOverlap(aa(score="ratio")) as h:
        (rc_n, _), (rc_m, text) = both(h)
        assert rc_n == CMPR_OK and rc_m == CMPR_EINVAL and "ratio score needs cmpr_overlap_matrix_f64" in text
    for score in ("mh", "jaccard"):
        with HipOverlap(aa(score=score)) as h:
            for rc, text in both(h, cutoff=1):
                assert rc == CMPR_EINVAL and text == "The Morisita-Horn / Jaccard index is not defined when d>0"
            assert [rc for rc, _ in both(h, cutoff=0)] == [CMPR_OK, CMPR_OK]
    with HipOverlap(Options(n_v_genes=2 ** 24, n_j_genes=2 ** 23, device=0)) as h:
        for rc, text in both(h):
            assert rc == CMPR_EUNSUPPORTED and "n_v_genes x n_j_genes > 2^46" in text
    with HipOverlap(aa(nucleotides=True)) as h:
        for rc, text in both(h):
            assert rc == CMPR_EUNSUPPORTED and text == "cmpr_tcrdist: amino acids only"
    with HipOverlap(aa(ignore_genes=True)) as h:
        t = TcrdistParams(_tcrdist.table(), 4, v_distance=np.zeros((2, 2), dtype=np.uint16)).struct(h.opt)
        for rc, text in both(h, t=t):
            assert rc == CMPR_EINVAL and "v_distance with options.ignore_genes" in text
    # the options' own distance and indels are not refused; a set the validation refuses: as cmpr_set_reference
    bad = RepertoireSet(s2.residues, s2.offsets, s2.v_gene, s2.j_gene, s2.repertoire, s2.count.copy(),
                        s2.repertoire_ids, s2.v_names, s2.j_names, s2.alphabet)
    bad.count[17] = 0
    with HipOverlap(aa(differences=1, indels=True)) as h:
        assert [rc for rc, _ in both(h)] == [CMPR_OK, CMPR_OK]
        with pytest.raises(HipError) as want:
            h.set_reference(bad)
        for call in (lambda: h.tcrdist_neighbors(s1, bad, p, 6), lambda: h.tcrdist_matrix(bad, s2, p, 6)):
            with pytest.raises(HipError) as e:
                call()
            assert (e.value.code, str(e.value)) == (want.value.code, str(want.value))
        assert_equal_edges(h.tcrdist_neighbors(s1, s2, p, 6), _tcrdist.want("tiny", 1, False), s1.n)
