"""cmpr_cluster / cmpr_cluster_device on the GPU: the partitions the reference's --cluster recorded, one giant
component under contention, large sets against a union-find over the existing pair path, a reference indexed
in parts, both entry points, what stays resident afterwards, and the contract of the entry points."""

import ctypes as C
import functools

import numpy as np
import pytest

import _cluster
import compairr_amd
from compairr_amd import HipError, HipOverlap, Options, RepertoireSet, synth
from compairr_amd.sets import AA

pytestmark = pytest.mark.gpu

CASES = _cluster.cases()
CMPR_EINVAL, CMPR_EUNSUPPORTED = 1, 4
FULL = dict(n_v_genes=synth.N_V, n_j_genes=synth.N_J)


def assert_consistent(label, size, clusters):
    """what holds for every result: a label is a root and no larger than its members, the sizes follow from the
    labels, the count is the number of roots"""
    n = len(label)
    assert label.dtype == np.uint32 and size.dtype == np.uint32
    assert (label <= np.arange(n)).all() and (label[label] == label).all()
    assert np.array_equal(size, _cluster.sizes_of_labels(label))
    assert clusters == int((label == np.arange(n)).sum())


# ---- 1. the recorded cases ----

@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_recorded_cases(case):
    s, keys = _cluster.read_input(case)
    want = _cluster.recorded_partition(case, keys)
    label, size, clusters = compairr_amd.cluster(s, _cluster.options_of(s, case, device=0))
    assert clusters == want[2]
    assert np.array_equal(label, want[0]) and np.array_equal(size, want[1])
    assert label.dtype == np.uint32 and size.dtype == np.uint32


# ---- 2. one giant, contended component ----

@functools.lru_cache(maxsize=None)
def hypercube(two_genes):
    """the 4096 sequences of length 12 over two amino acids in a seeded random order: the vertices of a
    hypercube, 12 neighbours each at d = 1.  two_genes: V gene = parity of the sequence number."""
    L, n = 12, 4096
    bits = (np.arange(n)[:, None] >> np.arange(L)[None, :]) & 1
    rows = np.where(bits == 1, AA.index("W"), AA.index("C")).astype(np.uint8)
    rows = rows[np.random.default_rng(4096).permutation(n)]
    v = (np.arange(n) & 1).astype(np.uint32) if two_genes else np.zeros(n, dtype=np.uint32)
    return RepertoireSet(rows.reshape(-1), np.arange(n + 1, dtype=np.uint64) * L, v, np.zeros(n, dtype=np.uint32),
                         np.zeros(n, dtype=np.uint32), np.ones(n, dtype=np.uint64), ["H1"],
                         ["V0", "V1"][:2 if two_genes else 1], ["J0"], AA)


def test_hypercube_is_one_cluster():
    s = hypercube(False)
    label, size, clusters = compairr_amd.cluster(s, Options(differences=1, n_v_genes=1, n_j_genes=1, device=0))
    assert clusters == 1
    assert not label.any() and (size == 4096).all()


def test_hypercube_with_two_genes_equals_the_model():
    s = hypercube(True)
    opt = Options(differences=1, n_v_genes=2, n_j_genes=1, device=0)
    want = _cluster.model(s, opt)
    assert 1 < want[2] < 4096
    label, size, clusters = compairr_amd.cluster(s, opt)
    assert clusters == want[2]
    assert np.array_equal(label, want[0]) and np.array_equal(size, want[1])


# ---- 3. against the existing pair path; 4. a reference in parts ----

BIG = {
    "aa_d1": (dict(differences=1), False),
    "aa_d1i": (dict(differences=1, indels=True), False),
    "nt_d2_g": (dict(differences=2, nucleotides=True, ignore_genes=True), True),
}


@functools.lru_cache(maxsize=None)
def big_set(nucleotides):
    return synth.make_set(50_000, 31, nucleotides=True) if nucleotides else synth.make_set(200_000, 30)


def big_options(name):
    return Options(device=0, **FULL, **BIG[name][0])


@functools.lru_cache(maxsize=None)
def labels_by_pairs(name):
    """the labels of big_set under BIG[name] from overlap_pairs() of a context given the set twice, united on
    the host: computed once, read-only"""
    s = big_set(BIG[name][1])
    with HipOverlap(big_options(name)) as h:
        h.set_reference(s, s.longest)
        h.set_queries(s)
        pairs = h.overlap_pairs()
    assert len(pairs) > s.n                        # (beyond the identity pairs)
    label = _cluster.labels_of_pairs(s.n, pairs[:, 0], pairs[:, 1])
    label.setflags(write=False)
    return label


@pytest.mark.parametrize("name", list(BIG))
def test_large_sets_equal_a_union_find_over_the_pair_list(name):
    s = big_set(BIG[name][1])
    want = labels_by_pairs(name)
    label, size, clusters = compairr_amd.cluster(s, big_options(name))
    print("%s: %d sequences, %d clusters, largest %d" % (name, s.n, clusters, int(size.max())))
    assert np.array_equal(label, want)
    assert_consistent(label, size, clusters)
    assert 1 < clusters < s.n


def test_reference_in_parts_gives_the_same_clusters():
    s = big_set(False)
    want = labels_by_pairs("aa_d1")
    with HipOverlap(big_options("aa_d1")) as h:
        h.set_tunable("part_buckets_log2", 17)
        label, size, clusters = h.cluster(s)
        assert h.get_tunable("reference_parts") >= 3
    assert np.array_equal(label, want)
    assert_consistent(label, size, clusters)


# ---- 5. both entry points, repeatability ----

@functools.lru_cache(maxsize=None)
def medium_set():
    return synth.make_set(20_000, 32, pool_size=3000)


def device_cluster(h, s, want_label=True, want_size=True):
    import torch
    view, keep = HipOverlap.device_view(s)
    d_label = torch.full((s.n + 64,), 0x25A5A5A5, dtype=torch.int32, device="cuda")
    d_size = torch.full((s.n + 64,), 0x25A5A5A5, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    clusters = h.cluster_device(view, d_label.data_ptr() if want_label else 0, d_size.data_ptr() if want_size else 0)
    del keep
    return d_label.cpu().numpy().view(np.uint32), d_size.cpu().numpy().view(np.uint32), clusters


def test_device_entry_point_and_repeated_calls():
    s, other = medium_set(), synth.tiny_set(3000, 5, letters=3, max_len=7, n_v=synth.N_V, n_j=synth.N_J)
    opt = Options(differences=1, indels=True, device=0, **FULL)
    with HipOverlap(opt) as h:
        one = h.cluster(s)
        assert_consistent(*one)
        assert 1 < one[2] < s.n
        two = h.cluster(s)
        d_label, d_size, d_clusters = device_cluster(h, s)
        between = h.cluster(other)
        assert_consistent(*between)
        three = h.cluster(s)
        # one array only: the other is left alone, the count is the same
        l_only = device_cluster(h, s, want_size=False)
        s_only = device_cluster(h, s, want_label=False)
    for again in (two, three):
        assert np.array_equal(one[0], again[0]) and np.array_equal(one[1], again[1]) and one[2] == again[2]
    assert d_clusters == one[2] and l_only[2] == one[2] and s_only[2] == one[2]
    assert np.array_equal(d_label[:s.n], one[0]) and np.array_equal(d_size[:s.n], one[1])
    # (the device arrays have n elements: what lies behind them is not the call's to write)
    assert (d_label[s.n:] == 0x25A5A5A5).all() and (d_size[s.n:] == 0x25A5A5A5).all()
    assert np.array_equal(l_only[0][:s.n], one[0]) and (l_only[1] == 0x25A5A5A5).all()
    assert np.array_equal(s_only[1][:s.n], one[1]) and (s_only[0] == 0x25A5A5A5).all()
    want = _cluster.model(other, opt)
    assert np.array_equal(between[0], want[0]) and between[2] == want[2]


# ---- 6. what stays resident ----

def test_the_set_stays_resident_as_both_sets():
    s = medium_set()
    opt = Options(differences=1, device=0, **FULL)
    with HipOverlap(opt) as fresh:
        fresh.set_reference(s, s.longest)
        fresh.set_queries(s)
        matrix, pairs = fresh.overlap_matrix(), fresh.overlap_pairs()
    assert len(pairs) > s.n
    with HipOverlap(opt) as h:
        label, size, clusters = h.cluster(s)
        assert h.shape == matrix.shape
        assert np.array_equal(h.overlap_matrix(), matrix)
        # pairs are listed again: the link pointer does not stay set
        assert np.array_equal(h.overlap_pairs(), pairs)
        assert np.array_equal(h.overlap_matrix(), matrix)
        again = h.cluster(s)
    assert np.array_equal(label, _cluster.labels_of_pairs(s.n, pairs[:, 0], pairs[:, 1]))
    assert np.array_equal(again[0], label) and np.array_equal(again[1], size) and again[2] == clusters


# ---- 7. the contract ----

def raw_cluster(h, s, label=None, size=None, device=False):
    """cmpr_cluster as it is declared: (code, n_clusters)"""
    v = compairr_amd.hip._view(s) if s is not None else None
    clusters = C.c_uint64(12345)
    fn = h._lib.cmpr_cluster_device if device else h._lib.cmpr_cluster
    rc = fn(h._ctx, C.byref(v) if v is not None else None, None if label is None else label.ctypes.data,
            None if size is None else size.ctypes.data, C.byref(clusters))
    return rc, clusters.value


def test_empty_set_is_ok_with_zero_clusters():
    z = lambda t: np.zeros(0, dtype=t)
    s = RepertoireSet(z(np.uint8), np.zeros(1, dtype=np.uint64), z(np.uint32), z(np.uint32), z(np.uint32),
                      z(np.uint64), ["T1"])
    with HipOverlap(Options(differences=1, device=0, **FULL)) as h:
        label, size, clusters = h.cluster(s)
        assert (len(label), len(size), clusters) == (0, 0, 0)
        assert raw_cluster(h, s) == (0, 0)


def test_null_set_existence_and_work_shards_are_refused():
    s = medium_set()
    with HipOverlap(Options(differences=1, device=0, **FULL)) as h:
        for device in (False, True):
            assert raw_cluster(h, None, device=device)[0] == CMPR_EINVAL
            assert h._lib.cmpr_last_error(h._ctx).decode() == "set view is NULL"
        h.set_tunable("work_shard_count", 2)
        with pytest.raises(HipError) as e:
            h.cluster(s)
        assert e.value.code == CMPR_EUNSUPPORTED and "work_shard_count" in str(e.value)
    with HipOverlap(Options(differences=1, existence=True, device=0, **FULL)) as h:
        with pytest.raises(HipError) as e:
            h.cluster(s)
        assert e.value.code == CMPR_EINVAL and "existence" in str(e.value)


def test_either_array_may_be_left_out():
    s = medium_set()
    with HipOverlap(Options(differences=1, device=0, **FULL)) as h:
        label, size, clusters = h.cluster(s)
        assert raw_cluster(h, s) == (0, clusters)
        only_label, only_size = np.zeros(s.n, dtype=np.uint32), np.zeros(s.n, dtype=np.uint32)
        assert raw_cluster(h, s, label=only_label) == (0, clusters)
        assert raw_cluster(h, s, size=only_size) == (0, clusters)
        # the count may be left out too
        v = compairr_amd.hip._view(s)
        assert h._lib.cmpr_cluster(h._ctx, C.byref(v), None, None, None) == 0
    assert np.array_equal(only_label, label) and np.array_equal(only_size, size)


def test_three_differences_fail_as_they_do_today():
    """cmpr_create refuses d = 3.  (The library keeps the message of a failed cmpr_create per thread, and
    tests/test_tunables_gpu.py records that of this one as empty: the call is made on a thread of its own.)"""
    import threading
    caught = []

    def call():
        try:
            compairr_amd.cluster(medium_set(), Options(differences=3, device=0, **FULL))
        except HipError as e:
            caught.append(e)

    t = threading.Thread(target=call)
    t.start()
    t.join()
    assert len(caught) == 1
    assert caught[0].code == CMPR_EUNSUPPORTED and "d > 2" in str(caught[0])


def test_a_refusal_of_the_set_passes_through_unchanged():
    """a zero duplicate_count: the code and text cmpr_set_reference gives"""
    s = synth.tiny_set(300, 4)
    s.count[123] = 0
    opt = Options(differences=1, n_v_genes=2, n_j_genes=2, device=0)
    with HipOverlap(opt) as h:
        with pytest.raises(HipError) as want:
            h.set_reference(s, 0)
    with HipOverlap(opt) as h:
        with pytest.raises(HipError) as got:
            h.cluster(s)
    assert (got.value.code, str(got.value)) == (want.value.code, str(want.value))
