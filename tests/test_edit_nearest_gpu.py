"""cmpr_edit_nearest and its _device variant on the GPU: parity with the numpy brute force (tests/_edit_nearest.py) on
every input, with and without genes, floor, cap and flag; with cmpr_edit_neighbors at the cap and cmpr_hamming_neighbors
at 0, reduced on the host; the hand-written length-gap case with and without the stop; the relation to
cmpr_hamming_nearest; the same bytes under every segment count, staging, word count and with the stop on and off, on
groups of several workgroups and staged pieces; swapped sizes; the column words at their edges; the device variant's
optional outputs and bounds; small and empty cases; the refusals; the resident state left alone; determinism; the
timers.  No expectation comes from the library."""

import ctypes as C
import itertools

import numpy as np
import pytest

import _edit
import _edit_nearest
import _hamming
import _nearest
import _neighbors
import compairr_amd
from compairr_amd import HipError, HipOverlap, Options, RepertoireSet
from compairr_amd.hip import NEAREST_OTHER_REPERTOIRE, _view
from compairr_amd.sets import AA

pytestmark = pytest.mark.gpu

CMPR_OK, CMPR_EINVAL, CMPR_EUNSUPPORTED = 0, 1, 4
POISON16, POISON32 = 0xA5A5, 0x25A5A5A5
NONE32, NONE16 = _edit_nearest.NONE32, _edit_nearest.NONE16
DTYPES = (np.uint32, np.uint16, np.uint32)
# (input, ignore_genes, other repertoire): `aa` is one set, with and without the flag
INPUTS = [("nt", False, False), ("nt", True, False), ("aa", False, False), ("aa", True, False), ("aa", False, True),
          ("aa", True, True), ("min0", False, False), ("min0", True, False)]
INPUT_IDS = ["%s%s%s" % (n, "-g" if g else "", "-other" if o else "") for n, g, o in INPUTS]
FLOORS, CAPS = (0, 1), (0, 1, 3, None)


def assert_same(got, want, why=None):
    """the three arrays: dtypes, lengths and bytes; the three sentinels exactly where ties are 0"""
    assert len(got) == 3
    for g, w, t in zip(got, want, DTYPES):
        assert g.dtype == t and g.shape == w.shape, why
        assert g.tobytes() == w.tobytes(), why
    none = got[2] == 0
    assert (got[0][none] == NONE32).all() and (got[1][none] == NONE16).all() and (got[0][~none] != NONE32).all(), why


# ---- 1. parity with the brute force ----

@pytest.mark.parametrize("name,g,other", INPUTS, ids=INPUT_IDS)
def test_against_the_brute_force(name, g, other):
    s1, s2 = _edit.sets_of(name)
    with HipOverlap(_edit.options_of(name, g, device=0)) as h:
        for floor, cap in itertools.product(FLOORS, CAPS):
            got = h.edit_nearest(s1, s2, floor, cap, other)
            print(name, g, other, floor, cap, _edit_nearest.figures(got))
            assert_same(got, _edit_nearest.want(name, g, floor, cap, other), (floor, cap))
            if not other and (name, g, floor, cap) in _edit_nearest.FIGURES:
                assert _edit_nearest.figures(got) == _edit_nearest.FIGURES[(name, g, floor, cap)]


# ---- 2. agreement with the thresholded calls, reduced on the host ----

@pytest.mark.parametrize("name,g,other", INPUTS, ids=INPUT_IDS)
def test_against_the_neighbours_at_the_cap(name, g, other):
    s1, s2 = _edit.sets_of(name)
    longest = max(s1.longest, s2.longest)
    with HipOverlap(_edit.options_of(name, g, device=0)) as h:
        for cap in CAPS:
            edges = h.edit_neighbors(s1, s2, longest if cap is None else cap)
            for floor in FLOORS:
                assert_same(h.edit_nearest(s1, s2, floor, cap, other),
                            _edit_nearest.from_edges(s1, s2, edges, floor, other), (floor, cap))


@pytest.mark.parametrize("name,g,other", INPUTS, ids=INPUT_IDS)
def test_cap_0_is_the_hamming_neighbours_at_0(name, g, other):
    s1, s2 = _edit.sets_of(name)
    with HipOverlap(_edit.options_of(name, g, device=0)) as h:
        want = _edit_nearest.from_edges(s1, s2, h.hamming_neighbors(s1, s2, 0), 0, other)
        assert_same(h.edit_nearest(s1, s2, 0, 0, other), want)
    assert (want[1][want[2] > 0] == 0).all()


# ---- 3. the hand-written length-gap case ----

@pytest.mark.parametrize("prune", [0, 1])
def test_the_hand_written_length_gap_case(prune):
    s1, s2, want = _edit_nearest.hand()
    with HipOverlap(_edit_nearest.options_of("hand", False, device=0)) as h:
        h.set_tunable("edit_nearest_prune", prune)
        got = h.edit_nearest(s1, s2, 0, None)
        print(prune, [a.tolist() for a in got])
        assert tuple(int(a[0]) for a in got) != _edit_nearest.HAND_WRONG_STOP
        assert_same(got, want)
        assert_same(got, _edit_nearest.brute(s1, s2, False, 0, None))
        for floor, cap in ((0, 1), (2, None), (1, 2), (0, 0)):
            assert_same(h.edit_nearest(s1, s2, floor, cap), _edit_nearest.brute(s1, s2, False, floor, cap), (floor, cap))
    with HipOverlap(_edit_nearest.options_of("hand", True, device=0)) as h:
        h.set_tunable("edit_nearest_prune", prune)
        assert_same(h.edit_nearest(s1, s2, 0, None), _edit_nearest.brute(s1, s2, True, 0, None))


# ---- 4. the relation to cmpr_hamming_nearest ----

@pytest.mark.parametrize("name,g,other", INPUTS, ids=INPUT_IDS)
def test_whoever_hamming_finds_is_found_here_no_further(name, g, other):
    s1, s2 = _edit.sets_of(name)
    with HipOverlap(_edit.options_of(name, g, device=0)) as h:
        for floor in FLOORS:
            plain = h.hamming_nearest(s1, s2, floor, other)
            got = h.edit_nearest(s1, s2, floor, None, other)
            found = plain[2] > 0
            assert found.any() and (got[2][found] > 0).all()
            assert (got[1][found] <= plain[1][found]).all()


# ---- 5. the same bytes under every tunable ----

def test_every_segment_count_staging_word_count_and_stop_gives_the_same_bytes():
    """groups of some 830 sequences: four workgroups per group, with edit_stage_refs 7 and with 64 segments many staged
    pieces per partner, three partners per job"""
    s, _ = _edit_nearest.tuned_sets()
    assert np.bincount(s.lengths)[7:].min() > 3 * 256 and set(s.lengths.tolist()) == {7, 8, 9}
    want = _edit_nearest.want("tuned", True, 1, None)
    assert (want[2] > 0).all() and len(set(want[1].tolist())) > 1
    with HipOverlap(_edit_nearest.options_of("tuned", True, device=0)) as h:
        for seg, stage, words, prune in itertools.product((1, 2, 3, 64), (0, 1, 7), (0, 2, 4), (0, 1)):
            for name, value in (("edit_segments", seg), ("edit_stage_refs", stage), ("edit_words", words),
                                ("edit_nearest_prune", prune)):
                h.set_tunable(name, value)
            assert_same(h.edit_nearest(s, s, 1, None), want, (seg, stage, words, prune))
        # capped, at floor 0 and with the flag: the automatic segments, the stop on and off
        for name in ("edit_segments", "edit_stage_refs", "edit_words"):
            h.set_tunable(name, 0)
        for prune in (0, 1):
            h.set_tunable("edit_nearest_prune", prune)
            assert_same(h.edit_nearest(s, s, 0, 1, True), _edit_nearest.want("tuned", True, 0, 1, True), prune)


# ---- 6. swapped sizes ----

@pytest.mark.parametrize("name", ["long", "swapped"])
@pytest.mark.parametrize("g", [False, True], ids=["genes", "g"])
def test_few_queries_against_many_references_and_the_reverse(name, g):
    s1, s2 = _edit_nearest.sets_of(name)
    assert (s1.n, s2.n) == ((70, 9001) if name == "long" else (9001, 70))
    with HipOverlap(_edit_nearest.options_of(name, g, device=0)) as h:
        for floor in FLOORS:
            assert_same(h.edit_nearest(s1, s2, floor, 2), _edit_nearest.want(name, g, floor, 2), floor)


# ---- 7. the column words at their edges ----

@pytest.mark.parametrize("nucleotides", [False, True], ids=["aa", "nt"])
@pytest.mark.parametrize("words", [0, 2, 4])
def test_lengths_at_the_word_edges(nucleotides, words):
    """lengths 63 / 64 / 65, 127 / 128 / 129 and 255 / 256: every column word count, the queries of more than 64
    residues read from global memory"""
    s1, s2, ops, base_of = _edit.edge_sets(nucleotides)
    want = _edit_nearest.from_edges(s1, s2, _edit.edge_want(nucleotides))
    got = compairr_amd.edit_nearest(s1, s2, _edit.edge_options(nucleotides, device=0), 0, _edit.EDGE_D, False,
                                    {"edit_words": words})
    assert_same(got, want)
    assert_same(got, _edit_nearest.want("edge-nt" if nucleotides else "edge-aa", False, 0, _edit.EDGE_D))
    # every edited sequence finds its base, or somebody nearer, at no more than its number of operations
    near = ops <= _edit.EDGE_D
    assert (got[2][near] > 0).all() and (got[1][near] <= ops[near]).all()
    exact = ops == 0
    assert (got[1][exact] == 0).all() and np.array_equal(got[0][exact], base_of[exact])


# ---- 8. the device variant ----

def test_device_variant():
    import torch
    s1, s2 = _edit.nt_sets()
    n1, pad = s1.n, 8
    want = _edit_nearest.want("nt", False, 1, 3)
    found = int((want[2] > 0).sum())
    assert 0 < found < n1
    # (torch dtype, the fill as torch takes it, numpy dtype, the fill as numpy reads it)
    kinds = ((torch.int32, POISON32, np.uint32, POISON32), (torch.int16, POISON16 - 65536, np.uint16, POISON16),
             (torch.int32, POISON32, np.uint32, POISON32))
    with HipOverlap(_edit.options_of("nt", False, device=0)) as h:
        v1, keep1 = HipOverlap.device_view(s1)
        v2, keep2 = HipOverlap.device_view(s2)
        d_out = [torch.full((n1 + pad,), f, dtype=t, device="cuda") for t, f, _, _ in kinds]
        torch.cuda.synchronize()
        for seg in (0, 3):
            h.set_tunable("edit_segments", seg)
            for d, (_, f, _, _) in zip(d_out, kinds):
                d.fill_(f)
            torch.cuda.synchronize()
            # all three; what lies behind n1 is not the call's to write
            assert h.edit_nearest_device(v1, v2, 1, 3, 0, *[d.data_ptr() for d in d_out]) == found
            host = [d.cpu().numpy().view(u) for d, (_, _, u, _) in zip(d_out, kinds)]
            assert_same([a[:n1].copy() for a in host], want, seg)
            for a, (_, _, _, p) in zip(host, kinds):
                assert (a[n1:] == p).all()
            # each output in turn is NULL: the other two as before, the absent one untouched
            for absent in range(3):
                for d, (_, f, _, _) in zip(d_out, kinds):
                    d.fill_(f)
                torch.cuda.synchronize()
                ptrs = [0 if k == absent else d.data_ptr() for k, d in enumerate(d_out)]
                assert h.edit_nearest_device(v1, v2, 1, 3, 0, *ptrs) == found
                host = [d.cpu().numpy().view(u) for d, (_, _, u, _) in zip(d_out, kinds)]
                for k, (a, (_, _, _, p)) in enumerate(zip(host, kinds)):
                    if k == absent:
                        assert (a == p).all()
                    else:
                        assert a[:n1].tobytes() == want[k].tobytes() and (a[n1:] == p).all()
            # no array at all: the count alone; uncapped everybody is found
            assert h.edit_nearest_device(v1, v2, 1, 3, 0) == found
            assert h.edit_nearest_device(v1, v2, 1, None, 0) == n1
        # n_found_out NULL
        for d, (_, f, _, _) in zip(d_out, kinds):
            d.fill_(f)
        torch.cuda.synchronize()
        rc = h._lib.cmpr_edit_nearest_device(h._ctx, C.byref(v1), C.byref(v2), 1, 3, 0,
                                             *[C.c_void_p(d.data_ptr()) for d in d_out], None)
        assert rc == CMPR_OK
        assert_same([d.cpu().numpy().view(u)[:n1].copy() for d, (_, _, u, _) in zip(d_out, kinds)], want)
        # the same view twice is one-set mode; two equal but distinct views are two sets: (i, i) at distance 0
        twin, keep3 = HipOverlap.device_view(s1)
        for second, s_second in ((v1, s1), (twin, s1.subset(np.arange(n1)))):
            assert h.edit_nearest_device(v1, second, 0, None, 0, *[d.data_ptr() for d in d_out]) == n1
            got = [d.cpu().numpy().view(u)[:n1].copy() for d, (_, _, u, _) in zip(d_out, kinds)]
            assert_same(got, _edit_nearest.brute(s1, s_second, False, 0, None))
        assert (got[1] == 0).all() and (got[0] <= np.arange(n1)).all()
        assert not (_edit_nearest.brute(s1, s1, False, 0, None)[1] == 0).all()
        # the flag, in one-set mode
        assert h.edit_nearest_device(v1, v1, 1, 3, NEAREST_OTHER_REPERTOIRE, *[d.data_ptr() for d in d_out]) > 0
        got = [d.cpu().numpy().view(u)[:n1].copy() for d, (_, _, u, _) in zip(d_out, kinds)]
        assert_same(got, _edit_nearest.brute(s1, s1, False, 1, 3, True))
        del keep1, keep2, keep3


# ---- 9. small and empty cases ----

def test_small_and_empty_cases():
    z = lambda t: np.zeros(0, dtype=t)
    s = _edit.aa_sets()[0]
    empty = RepertoireSet(z(np.uint8), np.zeros(1, dtype=np.uint64), z(np.uint32), z(np.uint32), z(np.uint32),
                          z(np.uint64), ["T1", "T2"], ["V0", "V1"], ["J0", "J1"], AA)
    six, _ = _nearest.six()
    with HipOverlap(_edit.options(device=0)) as h:
        for seg in (0, 2):
            h.set_tunable("edit_segments", seg)
            # n1 = 0; n2 = 0
            assert [len(a) for a in h.edit_nearest(empty, s)] == [0, 0, 0]
            assert [len(a) for a in h.edit_nearest(empty, empty)] == [0, 0, 0]
            n = C.c_uint64(99)
            v_e, v_s = _view(empty), _view(s)
            out = [np.full(s.n + 1, 7, dtype=t) for t in DTYPES]
            assert h._lib.cmpr_edit_nearest(h._ctx, C.byref(v_s), C.byref(v_e), 0, 5, 0, *[a.ctypes.data for a in out],
                                            C.byref(n)) == CMPR_OK
            assert n.value == 0 and all(a[-1] == 7 for a in out)
            assert (out[0][:-1] == NONE32).all() and (out[1][:-1] == NONE16).all() and (out[2][:-1] == 0).all()
            assert h._lib.cmpr_edit_nearest(h._ctx, C.byref(v_e), C.byref(v_s), 0, 5, 0, *[a.ctypes.data for a in out],
                                            C.byref(n)) == CMPR_OK and n.value == 0
            # one sequence against itself
            one = six.subset(np.array([2]))
            assert [a.tolist() for a in h.edit_nearest(one, one, 0)] == [[NONE32], [NONE16], [0]]
            # two identical sequences: each other's neighbour at 0, nobody's at floor 1 or from another repertoire
            two = six.subset(np.array([0, 1]))
            assert [a.tolist() for a in h.edit_nearest(two, two, 0)] == [[1, 0], [0, 0], [1, 1]]
            assert [a.tolist() for a in h.edit_nearest(two, two, 1)] == [[NONE32] * 2, [NONE16] * 2, [0, 0]]
            assert [a.tolist() for a in h.edit_nearest(two, two, 0, None, True)] == [[NONE32] * 2, [NONE16] * 2, [0, 0]]
            # min_distance above max_distance, a floor nobody reaches, caps above every sequence
            for floor, cap in ((2, 1), (10, None), (65536, None), (2 ** 62, 2 ** 62)):
                got = h.edit_nearest(s, s, floor, cap)
                assert (got[0] == NONE32).all() and (got[1] == NONE16).all() and not got[2].any()
            uncapped = _edit_nearest.want("aa", False, 1, None)
            for cap in (s.longest, 2 ** 40, 2 ** 63 - 1):
                assert_same(h.edit_nearest(s, s, 1, cap), uncapped, cap)
    # the six of the Hamming call, where the lengths now mix: against the brute force
    for g, floor, other in itertools.product((False, True), (0, 1, 2), (False, True)):
        assert_same(compairr_amd.edit_nearest(six, six, _hamming.options(ignore_genes=g, device=0), floor, None, other),
                    _edit_nearest.brute(six, six, g, floor, None, other), (g, floor, other))


# ---- 10. refusals ----

def raw(h, v1, v2, floor=0, cap=3, flags=0):
    """cmpr_edit_nearest as it is declared, no output wanted: (code, text)"""
    ref = lambda v: None if v is None else C.byref(v)
    rc = h._lib.cmpr_edit_nearest(h._ctx, ref(v1), ref(v2), floor, cap, flags, None, None, None, None)
    return rc, h._lib.cmpr_last_error(h._ctx).decode()


def test_refusals():
    s1, s2 = _edit.nt_sets()
    v1, v2 = _view(s1), _view(s2)
    nt = lambda **kw: _edit.options_of("nt", False, device=0, **kw)
    with HipOverlap(nt()) as h:
        assert raw(h, v1, v2, -1) == (CMPR_EINVAL, "cmpr_edit_nearest: min_distance cannot be negative")
        assert raw(h, v1, v2, 0, -1) == (CMPR_EINVAL, "cmpr_edit_nearest: max_distance cannot be negative")
        for a, b in ((None, v2), (v1, None)):
            assert raw(h, a, b) == (CMPR_EINVAL, "set view is NULL")
        rc, text = raw(h, v1, v2, 0, 3, NEAREST_OTHER_REPERTOIRE)
        assert rc == CMPR_EINVAL and "CMPR_NEAREST_OTHER_REPERTOIRE" in text
        assert raw(h, v1, v1, 0, 3, NEAREST_OTHER_REPERTOIRE)[0] == CMPR_OK
        for flags in (2, 3, 1 << 31):
            rc, text = raw(h, v1, v1, 0, 3, flags)
            assert rc == CMPR_EINVAL and "flags" in text
        assert raw(h, v1, v2, 2, 1)[0] == CMPR_OK
        h.set_tunable("work_shard_count", 2)
        rc, text = raw(h, v1, v2)
        assert rc == CMPR_EUNSUPPORTED and "work_shard_count" in text
    with HipOverlap(Options(nucleotides=True, n_v_genes=2 ** 24, n_j_genes=2 ** 23, device=0)) as h:
        rc, text = raw(h, v1, v2)
        assert rc == CMPR_EUNSUPPORTED and "n_v_genes x n_j_genes > 2^46" in text
    # a sequence of 257 residues, in either set
    rng = np.random.default_rng(257)
    long = _neighbors._set_of_rows(rng.integers(0, 20, size=(1, 257), dtype=np.uint8), 2, 1)
    short = _neighbors._set_of_rows(rng.integers(0, 20, size=(1, 256), dtype=np.uint8), 2, 1)
    with HipOverlap(Options(n_v_genes=2, n_j_genes=2, device=0)) as h:
        for a, b in ((long, short), (short, long), (long, long)):
            assert raw(h, _view(a), _view(b)) == (CMPR_EUNSUPPORTED, "cmpr_edit: a sequence of more than 256 residues")
        assert raw(h, _view(short), _view(short))[0] == CMPR_OK
    # options.indels and options.differences play no part; nor does any score or `existence`
    want = _edit_nearest.want("nt", False, 1, 3)
    for kw in (dict(differences=1, indels=True), dict(differences=2), dict(score="mh"), dict(score="jaccard"),
               dict(score="ratio"), dict(existence=True)):
        assert_same(compairr_amd.edit_nearest(s1, s2, nt(**kw), 1, 3), want, kw)
    # a set the validation refuses: the same code and text as cmpr_set_reference
    bad = RepertoireSet(s2.residues, s2.offsets, s2.v_gene, s2.j_gene, s2.repertoire, s2.count.copy(),
                        s2.repertoire_ids, s2.v_names, s2.j_names, s2.alphabet)
    bad.count[17] = 0
    with HipOverlap(nt()) as h:
        with pytest.raises(HipError) as refused:
            h.set_reference(bad)
        for call in (lambda: h.edit_nearest(s1, bad), lambda: h.edit_nearest(bad, s2)):
            with pytest.raises(HipError) as e:
                call()
            assert (e.value.code, str(e.value)) == (refused.value.code, str(refused.value))
        assert_same(h.edit_nearest(s1, s2, 1, 3), want)


# ---- 11. the resident state is left alone; determinism; the timers ----

def test_resident_state_is_left_alone():
    s1, s2 = _edit.nt_sets()
    with HipOverlap(_edit.options_of("nt", False, differences=1, device=0)) as h:
        h.set_reference(s2, s1.longest)
        h.set_queries(s1)
        before, stats = h.overlap_matrix(), h.stats()
        assert_same(h.edit_nearest(s1, s2, 1, 3), _edit_nearest.want("nt", False, 1, 3))
        assert h.stats() == stats
        assert np.array_equal(h.overlap_matrix(), before) and h.stats().matches == stats.matches


def test_two_runs_give_the_same_bytes():
    s1, s2 = _edit.aa_sets()
    opt = _edit.options_of("aa", True, device=0)
    one = compairr_amd.edit_nearest(s1, s2, opt, 1, None, True)
    two = compairr_amd.edit_nearest(s1, s2, opt, 1, None, True)
    assert [a.tobytes() for a in one] == [b.tobytes() for b in two]
    assert_same(one, _edit_nearest.want("aa", True, 1, None, True))


HAMMING_TIMERS = ("hamming_group_us", "hamming_compare_us", "hamming_copy_us")


def test_timers():
    """the call sets edit_group_us, edit_compare_us and edit_copy_us, zeroes edit_order_us and leaves hamming_*_us"""
    s1, s2 = _edit.aa_sets()
    with HipOverlap(_edit.options_of("aa", True, device=0)) as h:
        h.hamming_nearest(s1, s2, 1)
        hamming = [h.get_tunable(name) for name in HAMMING_TIMERS]
        assert all(v > 0 for v in hamming)
        h.edit_neighbors(s1, s2, 3)
        assert h.get_tunable("edit_order_us") > 0
        for seg in (0, 2):
            h.set_tunable("edit_segments", seg)
            h.edit_nearest(s1, s2, 1, 3)
            assert h.get_tunable("edit_group_us") > 0 and h.get_tunable("edit_compare_us") > 0
            assert h.get_tunable("edit_copy_us") > 0 and h.get_tunable("edit_order_us") == 0
        assert [h.get_tunable(name) for name in HAMMING_TIMERS] == hamming
        assert h.get_tunable("edit_nearest_prune") == 1
        with pytest.raises(HipError):
            h.set_tunable("edit_nearest_prune", 2)
