"""cmpr_edit_cluster / cmpr_edit_cluster_table and their _device variants on the GPU: the partitions of the yardstick
(tests/_edit_cluster.py) for its figures, agreement with the hashed indel path at d = 1 and the Hamming clusters at
d = 0 and d = 3, every staging, segment count, column width and the snapshot switch, the device entry points, the
resident state and the timers, the refusals, and the small and extreme cases.  Everything is compared for exact
equality, and no expectation comes from the library."""

import ctypes as C
import itertools

import numpy as np
import pytest

import _cluster
import _edit
import _edit_cluster as ec
import _neighbors
import compairr_amd
from _cluster_table import TABLE_DTYPES, TABLE_NAMES, assert_partition, assert_table, table_of
from compairr_amd import HipError, HipOverlap, Options, RepertoireSet
from compairr_amd.hip import _view
from compairr_amd.sets import AA

pytestmark = pytest.mark.gpu

CMPR_OK, CMPR_EINVAL, CMPR_EUNSUPPORTED = 0, 1, 4
POISON32, POISON64 = 0x25A5A5A5, 0x25A5A5A525A5A5A5
HAMMING_TIMERS = ("hamming_group_us", "hamming_compare_us", "hamming_copy_us")


def assert_everything(s, opt_kw, d, label, tunables=None):
    """label, size, K and the table, with counts and with ignore_counts, against the partition `label`"""
    with HipOverlap(Options(device=0, **opt_kw)) as h:
        for name, value in (tunables or {}).items():
            h.set_tunable(name, value)
        assert_partition(h.edit_cluster(s, d), label)
        assert_table(h.edit_cluster_table(s, d), table_of(label, s.count))
    with HipOverlap(Options(device=0, ignore_counts=True, **opt_kw)) as h:
        for name, value in (tunables or {}).items():
            h.set_tunable(name, value)
        assert_table(h.edit_cluster_table(s, d), table_of(label, np.ones(s.n, dtype=np.uint64)))


# ---- 1. the figures ----

@pytest.mark.parametrize("key", ec.KEYS, ids=ec.ids_of(ec.KEYS))
def test_figures_against_the_yardstick(key):
    name, d, g = key
    label, size, clusters = ec.want(name, d, g)
    assert ec.figures_of(label, size) == ec.FIGURES[key]
    assert_everything(ec.set_of(name), ec.kw_of(name, g), d, label)


@pytest.mark.parametrize("key", ec.MORE_KEYS, ids=ec.ids_of(ec.MORE_KEYS))
def test_edge_sets_and_the_chain_against_the_yardstick(key):
    name, d, g = key
    label = ec.want(name, d, g)[0]
    if name == "chain":
        assert label.tolist() == (ec.CHAIN_LABEL if d == 1 else list(range(11)))
    assert_everything(ec.set_of(name), ec.kw_of(name, g), d, label)


# ---- 2. agreement between the calls ----

@pytest.mark.parametrize("key", ec.D1_KEYS, ids=ec.ids_of(ec.D1_KEYS))
def test_agreement_with_the_hashed_indel_path_at_d1(key):
    name, _, g = key
    s = ec.set_of(name)
    hashed = Options(differences=1, indels=True, device=0, **ec.kw_of(name, g))
    want = compairr_amd.cluster(s, hashed)
    want_table = compairr_amd.cluster_table(s, hashed)
    with HipOverlap(Options(device=0, **ec.kw_of(name, g))) as h:
        got = h.edit_cluster(s, 1)
        table = h.edit_cluster_table(s, 1)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert_table(table, want_table)
    assert_partition(got, ec.want(name, 1, g)[0])


@pytest.mark.parametrize("name", ["nt", "aa", "min0"])
@pytest.mark.parametrize("g", [False, True], ids=["genes", "g"])
def test_agreement_with_the_hamming_clusters(name, g):
    """d = 0: byte for byte; d = 3: every Hamming cluster inside one cluster here"""
    s = ec.set_of(name)
    with HipOverlap(Options(device=0, **ec.kw_of(name, g))) as h:
        got, table = h.edit_cluster(s, 0), h.edit_cluster_table(s, 0)
        plain, plain_table = h.hamming_cluster(s, 0), h.hamming_cluster_table(s, 0)
        assert [np.asarray(a).tobytes() for a in got + table] == [np.asarray(a).tobytes() for a in plain + plain_table]
        assert_partition(got, ec.want(name, 0, g)[0])
        wide, narrow = h.edit_cluster(s, 3)[0], h.hamming_cluster(s, 3)[0]
        assert ec.refines(narrow, wide)
        if (name, 3, g) in ec.FIGURES:
            assert_partition(h.edit_cluster(s, 3), ec.want(name, 3, g)[0])


# ---- 3. every staging, segment count and column width ----

def test_every_staging_segment_count_and_width_gives_the_yardstick_s_partition():
    """three groups of three query workgroups each, staged in pieces of 1, 3 or 512 references, in 1 to 64 segments:
    the giant component of d = 2 -g is reached only through chains across workgroups, segments and lengths"""
    s = ec.dense_set()
    label, size, clusters = ec.want("dense", 2, True)
    want_table = table_of(label, s.count)
    with HipOverlap(Options(device=0, **ec.kw_of("dense", True))) as h:
        combos = list(itertools.product((0, 1, 3, 512), (1, 2, 7, 64), (0, 2, 4), (1,)))
        combos += [(0, 0, 0, 0), (0, 0, 4, 0), (3, 7, 0, 0), (1, 64, 2, 0)]
        for stage, seg, words, snapshot in combos:
            for name, value in (("edit_stage_refs", stage), ("edit_segments", seg), ("edit_words", words),
                                ("edit_link_snapshot", snapshot)):
                h.set_tunable(name, value)
            got = h.edit_cluster(s, 2)
            assert got[0].tobytes() == label.tobytes() and got[1].tobytes() == size.tobytes(), (stage, seg, words)
            assert got[2] == clusters == 27
        assert_table(h.edit_cluster_table(s, 2), want_table)


@pytest.mark.parametrize("nucleotides", [False, True], ids=["aa", "nt"])
def test_edge_sets_under_every_width_and_staging(nucleotides):
    name = "edge_nt" if nucleotides else "edge_aa"
    s = ec.set_of(name)
    label, size, clusters = ec.want(name, _edit.EDGE_D, False)
    with HipOverlap(Options(device=0, **ec.kw_of(name, False))) as h:
        for words, stage in itertools.product((0, 2, 4), (0, 1, 3)):
            h.set_tunable("edit_words", words)
            h.set_tunable("edit_stage_refs", stage)
            got = h.edit_cluster(s, _edit.EDGE_D)
            assert got[0].tobytes() == label.tobytes() and got[1].tobytes() == size.tobytes(), (words, stage)
            assert got[2] == clusters
        assert_table(h.edit_cluster_table(s, _edit.EDGE_D), table_of(label, s.count))


# ---- 4. the device entry points ----

def subsets(names):
    return [tuple(n for n, keep in zip(names, mask) if not keep)
            for mask in itertools.product((True, False), repeat=len(names))]


def test_device_entry_points_write_what_is_documented():
    import torch
    s = ec.set_of("aa")
    n, d = s.n, 2
    label, size, clusters = ec.want("aa", d, False)
    want = table_of(label, s.count)
    with HipOverlap(Options(device=0, **ec.kw_of("aa", False))) as h:
        view, keep = HipOverlap.device_view(s)
        for left_out in subsets(("label", "size")):
            bufs = {name: torch.full((n + 64,), POISON32, dtype=torch.int32, device="cuda") for name in ("label", "size")}
            torch.cuda.synchronize()
            k = h.edit_cluster_device(view, d, *[0 if name in left_out else bufs[name].data_ptr()
                                                 for name in ("label", "size")])
            assert k == clusters
            for name, w in (("label", label), ("size", size)):
                a = bufs[name].cpu().numpy().view(np.uint32)
                if name in left_out:
                    assert (a == POISON32).all(), (name, left_out)
                else:
                    assert np.array_equal(a[:n], w) and (a[n:] == POISON32).all(), (name, left_out)
        lengths = (n, clusters + 1, n, clusters)
        for left_out in subsets(TABLE_NAMES):
            bufs = [torch.full((n + 64,), POISON32, dtype=torch.int32, device="cuda"),
                    torch.full((n + 1 + 64,), POISON64, dtype=torch.int64, device="cuda"),
                    torch.full((n + 64,), POISON32, dtype=torch.int32, device="cuda"),
                    torch.full((n + 64,), POISON64, dtype=torch.int64, device="cuda")]
            torch.cuda.synchronize()
            k = h.edit_cluster_table_device(view, d, *[0 if name in left_out else b.data_ptr()
                                                       for name, b in zip(TABLE_NAMES, bufs)])
            assert k == clusters
            for name, b, t, m, w in zip(TABLE_NAMES, bufs, TABLE_DTYPES, lengths, want):
                a = b.cpu().numpy().view(t)
                poison = POISON64 if t == np.uint64 else POISON32
                if name in left_out:
                    assert (a == poison).all(), (name, left_out)
                else:                                       # (K + 1 of cluster_start and K of count, no more)
                    assert np.array_equal(a[:m], w) and (a[m:] == poison).all(), (name, left_out)
        del keep


def test_host_entry_points_take_null_outputs():
    s = ec.set_of("aa")
    label, size, clusters = ec.want("aa", 2, True)
    want = table_of(label, s.count)
    v = _view(s)
    with HipOverlap(Options(device=0, **ec.kw_of("aa", True))) as h:
        for left_out in subsets(("label", "size")):
            out = {"label": np.full(s.n, POISON32, dtype=np.uint32), "size": np.full(s.n, POISON32, dtype=np.uint32)}
            k = C.c_uint64(12345)
            rc = h._lib.cmpr_edit_cluster(h._ctx, C.byref(v), 2, *[None if name in left_out else out[name].ctypes.data
                                                                   for name in ("label", "size")], C.byref(k))
            assert (rc, k.value) == (CMPR_OK, clusters)
            for name, w in (("label", label), ("size", size)):
                assert (out[name] == POISON32).all() if name in left_out else np.array_equal(out[name], w)
        for left_out in subsets(TABLE_NAMES):
            out = [np.full(s.n + 1 if name == "cluster_start" else s.n, POISON64 if t == np.uint64 else POISON32, dtype=t)
                   for name, t in zip(TABLE_NAMES, TABLE_DTYPES)]
            k = C.c_uint64(12345)
            rc = h._lib.cmpr_edit_cluster_table(h._ctx, C.byref(v), 2,
                                                *[None if name in left_out else a.ctypes.data
                                                  for name, a in zip(TABLE_NAMES, out)], C.byref(k))
            assert (rc, k.value) == (CMPR_OK, clusters)
            for name, a, m, w in zip(TABLE_NAMES, out, (s.n, clusters + 1, s.n, clusters), want):
                poison = POISON64 if a.dtype == np.uint64 else POISON32
                if name in left_out:
                    assert (a == poison).all(), (name, left_out)
                else:
                    assert np.array_equal(a[:m], w) and (a[m:] == poison).all(), (name, left_out)
        # the count may be left out too
        assert h._lib.cmpr_edit_cluster(h._ctx, C.byref(v), 2, None, None, None) == CMPR_OK
        assert h._lib.cmpr_edit_cluster_table(h._ctx, C.byref(v), 2, None, None, None, None, None) == CMPR_OK


# ---- 5. the resident state and the timers ----

def test_resident_state_and_timers_are_left_alone():
    s1, s2 = _edit.aa_sets()[0], _edit.min0_sets()[1]
    label = ec.want("aa", 2, False)[0]
    read = lambda h, names: [h.get_tunable(name) for name in names]
    with HipOverlap(_edit.options(differences=1, device=0)) as h:
        h.set_reference(s2, s1.longest)
        h.set_queries(s1)
        before, stats = h.overlap_matrix(), h.stats()
        h.hamming_neighbors(s1, s2, 3)
        hamming = read(h, HAMMING_TIMERS)
        assert_partition(h.edit_cluster(s1, 2), label)
        assert h.get_tunable("edit_group_us") > 0 and h.get_tunable("edit_compare_us") > 0
        assert h.get_tunable("edit_order_us") == 0 and h.get_tunable("edit_copy_us") > 0
        assert_table(h.edit_cluster_table(s1, 2), table_of(label, s1.count))
        assert h.get_tunable("edit_group_us") > 0 and h.get_tunable("edit_compare_us") > 0
        assert h.get_tunable("edit_order_us") == 0 and h.get_tunable("edit_copy_us") == 0
        assert h.get_tunable("cluster_table_us") > 0 and h.get_tunable("cluster_links_us") == 0
        assert read(h, HAMMING_TIMERS) == hamming
        assert h.shape == before.shape
        after = h.stats()
        assert (after.queries, after.matches, after.variants) == (stats.queries, stats.matches, stats.variants)
        assert np.array_equal(h.overlap_matrix(), before) and h.stats().matches == stats.matches
        # cmpr_cluster afterwards still works, at the context's own d
        want = _cluster.model(s1, _edit.options(differences=1))
        for a, b in zip(h.cluster(s1), want):
            assert np.array_equal(a, b)


# ---- 6. refusals ----

def raw(h, name, v, d):
    """an entry point as it is declared, all arrays NULL: (code, n_clusters, message)"""
    clusters = C.c_uint64(12345)
    outs = (None,) * (4 if "table" in name else 2)
    rc = getattr(h._lib, name)(h._ctx, C.byref(v) if v is not None else None, d, *outs, C.byref(clusters))
    return rc, clusters.value, h._lib.cmpr_last_error(h._ctx).decode() if rc else ""


ENTRY_POINTS = ("cmpr_edit_cluster", "cmpr_edit_cluster_table")


def test_refusals():
    s = ec.set_of("aa")
    v = _view(s)
    label = ec.want("aa", 2, False)[0]
    with HipOverlap(_edit.options(device=0)) as h:
        for name in ENTRY_POINTS:
            assert raw(h, name, v, -1) == (CMPR_EINVAL, 0, "Differences specified with -d or -differences cannot be negative.")
            assert raw(h, name, None, 2) == (CMPR_EINVAL, 0, "set view is NULL")
        h.set_tunable("work_shard_count", 2)
        for name in ENTRY_POINTS:
            rc, k, text = raw(h, name, v, 2)
            assert rc == CMPR_EUNSUPPORTED and k == 0 and text.startswith(name + ": ") and "work_shard_count > 1" in text
    with HipOverlap(Options(device=0, n_v_genes=1 << 24, n_j_genes=1 << 23)) as h:
        for name in ENTRY_POINTS:
            rc, k, text = raw(h, name, v, 2)
            assert rc == CMPR_EUNSUPPORTED and k == 0 and text.startswith(name + ": ") and "n_v_genes x n_j_genes > 2^46" in text
    with HipOverlap(_edit.options(existence=True, device=0)) as h:
        for name in ENTRY_POINTS:
            assert raw(h, name, v, 2) == (CMPR_EINVAL, 0, "cmpr_cluster: clusters are not defined with options.existence")
    # indels and a d of the context's own play no part and are not refused
    for more in (dict(differences=1, indels=True), dict(differences=2)):
        with HipOverlap(_edit.options(device=0, **more)) as h:
            assert_partition(h.edit_cluster(s, 2), label)
            assert_table(h.edit_cluster_table(s, 2), table_of(label, s.count))
    # no score plays a part
    for score in ("mh", "jaccard", "ratio"):
        with HipOverlap(_edit.options(score=score, device=0)) as h:
            assert_partition(h.edit_cluster(s, 2), label)
            assert_table(h.edit_cluster_table(s, 2), table_of(label, s.count))
    # a sequence of 257 residues
    rng = np.random.default_rng(257)
    long = _neighbors._set_of_rows(rng.integers(0, 20, size=(2, 257), dtype=np.uint8), 2, 1)
    with HipOverlap(_edit.options(device=0)) as h:
        for name in ENTRY_POINTS:
            assert raw(h, name, _view(long), 2) == (CMPR_EUNSUPPORTED, 0, "cmpr_edit: a sequence of more than 256 residues")
    # a set the validation refuses: the same code and text as cmpr_set_reference
    bad = RepertoireSet(s.residues, s.offsets, s.v_gene, s.j_gene, s.repertoire, s.count.copy(),
                        s.repertoire_ids, s.v_names, s.j_names, AA)
    bad.count[17] = 0
    with HipOverlap(_edit.options(device=0)) as h:
        with pytest.raises(HipError) as want:
            h.set_reference(bad)
    with HipOverlap(_edit.options(device=0)) as h:
        for call in (lambda: h.edit_cluster(bad, 2), lambda: h.edit_cluster_table(bad, 2)):
            with pytest.raises(HipError) as e:
                call()
            assert (e.value.code, str(e.value)) == (want.value.code, str(want.value))
        assert_partition(h.edit_cluster(s, 2), label)


# ---- 7. small and extreme cases ----

def empty_set():
    z = lambda t: np.zeros(0, dtype=t)
    return RepertoireSet(z(np.uint8), np.zeros(1, dtype=np.uint64), z(np.uint32), z(np.uint32), z(np.uint32),
                         z(np.uint64), ["T1", "T2"], ["V0", "V1"], ["J0", "J1"], AA)


def test_empty_set_is_ok_with_zero_clusters():
    import torch
    s = empty_set()
    v = _view(s)
    with HipOverlap(_edit.options(device=0)) as h:
        label, size, clusters = h.edit_cluster(s, 2)
        assert len(label) == 0 and len(size) == 0 and clusters == 0
        got = h.edit_cluster_table(s, 2)
        assert [len(a) for a in got] == [0, 1, 0, 0] and got[1][0] == 0
        start = np.full(4, POISON64, dtype=np.uint64)
        count = np.full(4, POISON64, dtype=np.uint64)
        k = C.c_uint64(12345)
        assert h._lib.cmpr_edit_cluster_table(h._ctx, C.byref(v), 2, None, start.ctypes.data, None,
                                              count.ctypes.data, C.byref(k)) == CMPR_OK
        assert k.value == 0 and start.tolist() == [0] + [POISON64] * 3 and (count == POISON64).all()
        d_start = torch.full((4,), POISON64, dtype=torch.int64, device="cuda")
        d_count = torch.full((4,), POISON64, dtype=torch.int64, device="cuda")
        d_label = torch.full((4,), POISON32, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        view, keep = HipOverlap.device_view(s)
        assert h.edit_cluster_table_device(view, 2, 0, d_start.data_ptr(), 0, d_count.data_ptr()) == 0
        assert h.edit_cluster_device(view, 2, d_label.data_ptr(), d_label.data_ptr()) == 0
        assert d_start.cpu().tolist() == [0] + [POISON64] * 3 and (d_count.cpu() == POISON64).all()
        assert (d_label.cpu() == POISON32).all()
        del keep


def test_one_sequence():
    s = ec.set_of("aa").subset(slice(0, 1))
    with HipOverlap(_edit.options(device=0)) as h:
        for d in (0, 3):
            label, size, clusters = h.edit_cluster(s, d)
            assert (label.tolist(), size.tolist(), clusters) == ([0], [1], 1)
            got = h.edit_cluster_table(s, d)
            assert [a.tolist() for a in got] == [[0], [0, 1], [0], [int(s.count[0])]]


@pytest.mark.parametrize("name,g", [("aa", False), ("nt", True), ("min0", False), ("dense", True)])
def test_huge_d(name, g):
    """above the longest sequence: as that length -- every (V, J) class, or the whole set with -g, one cluster"""
    s = ec.set_of(name)
    key = np.zeros(s.n, dtype=np.int64) if g else s.v_gene.astype(np.int64) * 1000 + s.j_gene
    first = {}
    label = np.array([first.setdefault(k, i) for i, k in enumerate(key.tolist())], dtype=np.uint32)
    with HipOverlap(Options(device=0, **ec.kw_of(name, g))) as h:
        at_longest = h.edit_cluster(s, int(s.longest)) + h.edit_cluster_table(s, int(s.longest))
        assert_partition(at_longest[:3], label)
        assert_table(at_longest[3:], table_of(label, s.count))
        for d in (10 ** 9, 2 ** 62):
            got = h.edit_cluster(s, d) + h.edit_cluster_table(s, d)
            assert [np.asarray(a).tobytes() for a in got] == [np.asarray(a).tobytes() for a in at_longest]


def test_two_runs_give_the_same_bytes():
    s = ec.dense_set()
    opt = Options(device=0, **ec.kw_of("dense", False))
    one = compairr_amd.edit_cluster(s, opt, 2) + compairr_amd.edit_cluster_table(s, opt, 2)
    two = compairr_amd.edit_cluster(s, opt, 2) + compairr_amd.edit_cluster_table(s, opt, 2)
    assert [np.asarray(a).tobytes() for a in one] == [np.asarray(b).tobytes() for b in two]
    assert_partition(one[:3], ec.want("dense", 2, False)[0])
