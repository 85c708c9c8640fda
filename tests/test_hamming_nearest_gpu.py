"""cmpr_hamming_nearest and its _device variant on the GPU: parity with the numpy brute force on every input, with and
without genes, floor and flag, and with the oracle's pair list up to d; a group larger than a workgroup and a staged
piece, against itself and swapped; the same bytes under every staging, segment count and form; the word and form
edges; the device variant's optional outputs, bounds and two modes; small and empty cases; the refusals; the resident
state left alone; determinism.  No expectation comes from the library."""

import ctypes as C
import itertools

import numpy as np
import pytest

import _hamming
import _nearest
import compairr_amd
from compairr_amd import HipError, HipOverlap, Options, RepertoireSet
from compairr_amd.hip import NEAREST_OTHER_REPERTOIRE, _view
from compairr_amd.sets import AA

pytestmark = pytest.mark.gpu

CMPR_OK, CMPR_EINVAL, CMPR_EUNSUPPORTED = 0, 1, 4
POISON16, POISON32 = 0xA5A5, 0x25A5A5A5
NONE32, NONE16 = _nearest.NONE32, _nearest.NONE16
DTYPES = (np.uint32, np.uint16, np.uint32)


def assert_same(got, want, why=None):
    """the three arrays: dtypes, lengths and bytes; the three sentinels exactly where ties are 0"""
    assert len(got) == 3
    for g, w, t in zip(got, want, DTYPES):
        assert g.dtype == t and g.shape == w.shape, why
        assert g.tobytes() == w.tobytes(), why
    none = got[2] == 0
    assert (got[0][none] == NONE32).all() and (got[1][none] == NONE16).all() and (got[0][~none] != NONE32).all(), why


def dense_options(g, **more):
    return _hamming.options(nucleotides=True, ignore_genes=g, **more)


# ---- 1. parity with the brute force and, up to d, with the oracle ----

@pytest.mark.parametrize("case", _nearest.CASES, ids=_nearest.IDS)
def test_against_the_brute_force(case):
    name, g, floor, other = case
    s1, s2 = _hamming.sets_of(name)
    want = _nearest.want(name, g, floor, other)
    got = compairr_amd.hamming_nearest(s1, s2, _hamming.options_of(name, g, device=0), floor, other)
    print(case, _nearest.figures(got))
    assert_same(got, want)
    assert _nearest.figures(got)[:3] == _nearest.FIGURES[case][:3]


@pytest.mark.parametrize("name", ["aa", "nt"])
@pytest.mark.parametrize("d", [3, 6])
@pytest.mark.parametrize("g", [False, True], ids=["genes", "g"])
def test_against_the_oracle_pair_list_up_to_d(name, d, g):
    s1, s2 = _hamming.sets_of(name)
    with HipOverlap(_hamming.options_of(name, g, device=0)) as h:
        for floor in (0, 1):
            for other in ((False, True) if s2 is s1 else (False,)):
                got = h.hamming_nearest(s1, s2, floor, other)
                _nearest.assert_agrees_up_to(got, _nearest.oracle_nearest(name, d, g, floor, other), d)


# ---- 2. one group larger than a workgroup and a staged piece ----

@pytest.mark.parametrize("floor", [0, 1])
@pytest.mark.parametrize("other", [False, True], ids=["plain", "other"])
def test_a_large_group_against_itself(floor, other):
    s, _ = _nearest.sets_of("self")
    want = _nearest.want_of("self", True, floor, other)
    assert (want[0] != np.arange(s.n)).all()                           # (nobody is its own neighbour)
    got = compairr_amd.hamming_nearest(s, s, dense_options(True, device=0), floor, other)
    assert_same(got, want)


@pytest.mark.parametrize("floor", [0, 1])
@pytest.mark.parametrize("g", [False, True], ids=["genes", "g"])
def test_a_large_set_of_queries_against_a_small_group(g, floor):
    s1, s2 = _nearest.sets_of("swapped")
    assert (s1.n, s2.n) == (9001, 70)
    got = compairr_amd.hamming_nearest(s1, s2, dense_options(g, device=0), floor)
    assert_same(got, _nearest.want_of("swapped", g, floor, False))


# ---- 3. the same bytes under every staging, segment count and form ----

@pytest.mark.parametrize("kind,g,floor,other", [("dense", True, 0, False), ("swapped", False, 1, False),
                                                ("self", True, 1, True), ("self", False, 0, False)],
                         ids=["dense-g", "swapped-genes-floor1", "self-g-floor1-other", "self-genes"])
def test_every_staging_segment_count_and_form_gives_the_same_bytes(kind, g, floor, other):
    s1, s2 = _nearest.sets_of(kind)
    want = _nearest.want_of(kind, g, floor, other)
    with HipOverlap(dense_options(g, device=0)) as h:
        for stage, seg, generic in itertools.product((0, 1, 63, 64, 65), (0, 1, 2, 7, 64), (0, 1)):
            for name, value in (("hamming_stage_refs", stage), ("hamming_segments", seg), ("hamming_generic", generic)):
                h.set_tunable(name, value)
            assert_same(h.hamming_nearest(s1, s2, floor, other), want, (stage, seg, generic))
        assert h.get_tunable("hamming_compare_us") > 0 and h.get_tunable("hamming_group_us") > 0
        assert h.get_tunable("hamming_copy_us") > 0


# ---- 4. word and form edges ----

@pytest.mark.parametrize("nucleotides", [False, True], ids=["aa", "nt"])
@pytest.mark.parametrize("generic", [0, 1])
def test_lengths_at_the_word_and_form_edges(nucleotides, generic):
    s1, s2, ks = _hamming.edge_sets(nucleotides)
    opt = _hamming.edge_options(nucleotides, device=0)
    for floor in (1, 0):
        got = compairr_amd.hamming_nearest(s1, s2, opt, floor, False, {"hamming_generic": generic})
        assert_same(got, _nearest.brute(s1, s2, False, floor))
    # (floor 0) by construction: a mutant with k substitutions lies k from its base and has nobody else
    mutant = ks >= 0
    base_of = {int(L): j for j, L in enumerate(s2.lengths)}
    assert np.array_equal(got[1][mutant], ks[mutant]) and (got[2][mutant] == 1).all()
    assert np.array_equal(got[0][mutant], [base_of[int(L)] for L in s1.lengths[mutant]])
    assert int((got[2] == 0).sum()) == _nearest.EDGE_NONE[nucleotides]


def test_a_reference_longer_than_the_staging_buffer():
    s = _nearest.long_set()
    opt = Options(n_v_genes=1, n_j_genes=1, device=0)
    for floor, other in ((0, False), (2, False), (0, True)):
        want = _nearest.brute(s, s, False, floor, other)
        assert (want[2] > 0).all() and want[1].max() > 3
        assert_same(compairr_amd.hamming_nearest(s, s, opt, floor, other), want, (floor, other))


# ---- 5. the device variant ----

def test_device_variant():
    import torch
    s1, s2 = _hamming.aa_sets()
    n1, pad = s1.n, 8
    want = _nearest.want("aa", False, 1, False)
    found = int((want[2] > 0).sum())
    # (torch dtype, the fill as torch takes it, numpy dtype, the fill as numpy reads it)
    kinds = ((torch.int32, POISON32, np.uint32, POISON32), (torch.int16, POISON16 - 65536, np.uint16, POISON16),
             (torch.int32, POISON32, np.uint32, POISON32))
    with HipOverlap(_hamming.options(device=0)) as h:
        v1, keep1 = HipOverlap.device_view(s1)
        v2, keep2 = HipOverlap.device_view(s2)
        d_out = [torch.full((n1 + pad,), f, dtype=t, device="cuda") for t, f, _, _ in kinds]
        torch.cuda.synchronize()
        # all three; what lies behind n1 is not the call's to write
        assert h.hamming_nearest_device(v1, v2, 1, 0, *[d.data_ptr() for d in d_out]) == found
        host = [d.cpu().numpy().view(u) for d, (_, _, u, _) in zip(d_out, kinds)]
        assert_same([a[:n1].copy() for a in host], want)
        for a, (_, _, _, p) in zip(host, kinds):
            assert (a[n1:] == p).all()
        # each output in turn is NULL: the other two as before, the absent one untouched
        for absent in range(3):
            for d, (_, f, _, _) in zip(d_out, kinds):
                d.fill_(f)
            torch.cuda.synchronize()
            ptrs = [0 if k == absent else d.data_ptr() for k, d in enumerate(d_out)]
            assert h.hamming_nearest_device(v1, v2, 1, 0, *ptrs) == found
            host = [d.cpu().numpy().view(u) for d, (_, _, u, _) in zip(d_out, kinds)]
            for k, (a, (_, _, _, p)) in enumerate(zip(host, kinds)):
                if k == absent:
                    assert (a == p).all()
                else:
                    assert a[:n1].tobytes() == want[k].tobytes() and (a[n1:] == p).all()
        # no array at all: the count alone; and n_found_out NULL
        assert h.hamming_nearest_device(v1, v2, 1, 0) == found
        for d, (_, f, _, _) in zip(d_out, kinds):
            d.fill_(f)
        torch.cuda.synchronize()
        rc = h._lib.cmpr_hamming_nearest_device(h._ctx, C.byref(v1), C.byref(v2), 1, 0,
                                                *[C.c_void_p(d.data_ptr()) for d in d_out], None)
        assert rc == CMPR_OK
        assert_same([d.cpu().numpy().view(u)[:n1].copy() for d, (_, _, u, _) in zip(d_out, kinds)], want)
        # the same view twice is one-set mode; two equal but distinct views are two sets: (i, i) at distance 0
        twin, keep3 = HipOverlap.device_view(s1)
        for second, s_second in ((v1, s1), (twin, s1.subset(np.arange(n1)))):
            assert h.hamming_nearest_device(v1, second, 0, 0, *[d.data_ptr() for d in d_out]) == n1
            got = [d.cpu().numpy().view(u)[:n1].copy() for d, (_, _, u, _) in zip(d_out, kinds)]
            assert_same(got, _nearest.brute(s1, s_second, False, 0))
        assert (got[1] == 0).all() and (got[0] <= np.arange(n1)).all()
        assert not (_nearest.brute(s1, s1, False, 0)[1] == 0).all()
        del keep1, keep2, keep3


# ---- 6. small and empty cases ----

def test_small_and_empty_cases():
    z = lambda t: np.zeros(0, dtype=t)
    s = _hamming.aa_sets()[0]
    empty = RepertoireSet(z(np.uint8), np.zeros(1, dtype=np.uint64), z(np.uint32), z(np.uint32), z(np.uint32),
                          z(np.uint64), ["T1", "T2"], ["V0", "V1"], ["J0", "J1"], AA)
    six, _ = _nearest.six()
    with HipOverlap(_hamming.options(device=0)) as h:
        # n1 = 0; n2 = 0
        assert [len(a) for a in h.hamming_nearest(empty, s)] == [0, 0, 0]
        assert [len(a) for a in h.hamming_nearest(empty, empty)] == [0, 0, 0]
        n = C.c_uint64(99)
        v_e, v_s = _view(empty), _view(s)
        out = [np.full(s.n + 1, 7, dtype=t) for t in DTYPES]
        assert h._lib.cmpr_hamming_nearest(h._ctx, C.byref(v_s), C.byref(v_e), 0, 0, *[a.ctypes.data for a in out],
                                           C.byref(n)) == CMPR_OK
        assert n.value == 0 and all(a[-1] == 7 for a in out)
        assert (out[0][:-1] == NONE32).all() and (out[1][:-1] == NONE16).all() and (out[2][:-1] == 0).all()
        assert h._lib.cmpr_hamming_nearest(h._ctx, C.byref(v_e), C.byref(v_s), 0, 0, *[a.ctypes.data for a in out],
                                           C.byref(n)) == CMPR_OK and n.value == 0
        # one sequence against itself
        one = six.subset(np.array([2]))
        assert [a.tolist() for a in h.hamming_nearest(one, one)] == [[NONE32], [NONE16], [0]]
        # two identical sequences of one repertoire
        two = six.subset(np.array([0, 1]))
        assert [a.tolist() for a in h.hamming_nearest(two, two, 0, True)] == [[NONE32] * 2, [NONE16] * 2, [0, 0]]
        assert [a.tolist() for a in h.hamming_nearest(two, two)] == [[1, 0], [0, 0], [1, 1]]
        assert [a.tolist() for a in h.hamming_nearest(two, two, 1)] == [[NONE32] * 2, [NONE16] * 2, [0, 0]]
        # a floor nobody reaches
        for floor in (10, 65536, 10 ** 9, 2 ** 62):
            got = h.hamming_nearest(s, _hamming.aa_sets()[1], floor)
            assert (got[0] == NONE32).all() and (got[1] == NONE16).all() and not got[2].any()
    # the hand-written case
    _, table = _nearest.six()
    for (g, floor, other), want in table.items():
        assert_same(compairr_amd.hamming_nearest(six, six, _hamming.options(ignore_genes=g, device=0), floor, other),
                    want, (g, floor, other))


# ---- 7. refusals ----

def raw(h, v1, v2, floor=0, flags=0):
    """cmpr_hamming_nearest as it is declared, no output wanted: (code, text)"""
    ref = lambda v: None if v is None else C.byref(v)
    rc = h._lib.cmpr_hamming_nearest(h._ctx, ref(v1), ref(v2), floor, flags, None, None, None, None)
    return rc, h._lib.cmpr_last_error(h._ctx).decode()


def test_refusals():
    s1, s2 = _hamming.aa_sets()
    v1, v2 = _view(s1), _view(s2)
    with HipOverlap(_hamming.options(device=0)) as h:
        rc, text = raw(h, v1, v2, -1)
        assert rc == CMPR_EINVAL and "min_distance" in text and "negative" in text
        for a, b in ((None, v2), (v1, None)):
            assert raw(h, a, b) == (CMPR_EINVAL, "set view is NULL")
        rc, text = raw(h, v1, v2, 0, NEAREST_OTHER_REPERTOIRE)
        assert rc == CMPR_EINVAL and "CMPR_NEAREST_OTHER_REPERTOIRE" in text
        assert raw(h, v1, v1, 0, NEAREST_OTHER_REPERTOIRE)[0] == CMPR_OK
        for flags in (2, 3, 1 << 31):
            rc, text = raw(h, v1, v1, 0, flags)
            assert rc == CMPR_EINVAL and "flags" in text
        h.set_tunable("work_shard_count", 2)
        rc, text = raw(h, v1, v2)
        assert rc == CMPR_EUNSUPPORTED and "work_shard_count" in text
    with HipOverlap(_hamming.options(differences=1, indels=True, device=0)) as h:
        rc, text = raw(h, v1, v2)
        assert rc == CMPR_EINVAL and "the all-against-all path has no indels" in text
    with HipOverlap(Options(n_v_genes=2 ** 24, n_j_genes=2 ** 23, device=0)) as h:
        rc, text = raw(h, v1, v2)
        assert rc == CMPR_EUNSUPPORTED and "n_v_genes x n_j_genes > 2^46" in text
    # no score plays a part
    want = _nearest.want("aa", False, 1, False)
    for kw in (dict(score="mh"), dict(score="jaccard"), dict(score="ratio"), dict(existence=True)):
        assert_same(compairr_amd.hamming_nearest(s1, s2, _hamming.options(device=0, **kw), 1), want, kw)
    # a set the validation refuses: the same code and text as cmpr_set_reference
    bad = RepertoireSet(s2.residues, s2.offsets, s2.v_gene, s2.j_gene, s2.repertoire, s2.count.copy(),
                        s2.repertoire_ids, s2.v_names, s2.j_names, AA)
    bad.count[17] = 0
    with HipOverlap(_hamming.options(device=0)) as h:
        with pytest.raises(HipError) as refused:
            h.set_reference(bad)
        for call in (lambda: h.hamming_nearest(s1, bad), lambda: h.hamming_nearest(bad, s2)):
            with pytest.raises(HipError) as e:
                call()
            assert (e.value.code, str(e.value)) == (refused.value.code, str(refused.value))
        assert_same(h.hamming_nearest(s1, s2, 1), want)


# ---- 8. the resident state is left alone ----

def test_resident_state_is_left_alone():
    s1, s2 = _hamming.aa_sets()
    with HipOverlap(_hamming.options(differences=1, device=0)) as h:
        h.set_reference(s2, s1.longest)
        h.set_queries(s1)
        before, stats = h.overlap_matrix(), h.stats()
        assert_same(h.hamming_nearest(s1, s2, 1), _nearest.want("aa", False, 1, False))
        assert h.stats() == stats
        assert np.array_equal(h.overlap_matrix(), before) and h.stats().matches == stats.matches


# ---- 9. determinism ----

def test_two_runs_give_the_same_bytes():
    s, _ = _nearest.sets_of("self")
    opt = dense_options(False, device=0)
    one = compairr_amd.hamming_nearest(s, s, opt, 1, True)
    two = compairr_amd.hamming_nearest(s, s, opt, 1, True)
    assert [a.tobytes() for a in one] == [b.tobytes() for b in two]
    assert_same(one, _nearest.want_of("self", False, 1, True))
