"""cmpr_hamming_cluster / cmpr_hamming_cluster_table and their _device variants on the GPU: the partitions of the
model (tests/_cluster.py) for the figures of tests/_hamming_cluster.py, the reference's own `-c` partitions at d <= 2
and d >= 3, agreement with the hashed path, both forms of the compare kernel under every staging, segment count and
form, the device entry points, the resident state left alone, the refusals, and the small cases.  Everything is
compared for exact equality, and no expectation comes from the library."""

import ctypes as C
import itertools

import numpy as np
import pytest

import _cluster
import _cluster_table
import _hamming
import _hamming_cluster as hc
import _neighbors
import compairr_amd
from _cluster_table import TABLE_DTYPES, TABLE_NAMES, assert_partition, assert_table, table_of
from compairr_amd import HipError, HipOverlap, Options, RepertoireSet
from compairr_amd.hip import _view
from compairr_amd.sets import AA

pytestmark = pytest.mark.gpu

CMPR_OK, CMPR_EINVAL, CMPR_EUNSUPPORTED = 0, 1, 4
POISON32, POISON64 = 0x25A5A5A5, 0x25A5A5A525A5A5A5


def assert_everything(s, opt_kw, d, label, tunables=None):
    """label, size, K and the table, with counts and with ignore_counts, against the partition `label`"""
    with HipOverlap(Options(device=0, **opt_kw)) as h:
        for name, value in (tunables or {}).items():
            h.set_tunable(name, value)
        assert_partition(h.hamming_cluster(s, d), label)
        assert_table(h.hamming_cluster_table(s, d), table_of(label, s.count))
    with HipOverlap(Options(device=0, ignore_counts=True, **opt_kw)) as h:
        for name, value in (tunables or {}).items():
            h.set_tunable(name, value)
        assert_table(h.hamming_cluster_table(s, d), table_of(label, np.ones(s.n, dtype=np.uint64)))


def kw_of(name, g):
    return dict(n_v_genes=2, n_j_genes=2, nucleotides=_hamming.SETS[name][1], ignore_genes=g)


# ---- 1. the figures ----

@pytest.mark.parametrize("key", hc.KEYS, ids=hc.IDS)
def test_figures_against_the_model(key):
    name, d, g = key
    s = hc.set_of(name)
    label, size, clusters = hc.model(name, d, g)
    assert hc.figures_of(label, size) == hc.FIGURES[key]
    assert_everything(s, kw_of(name, g), d, label)


# ---- 2. the reference's own partitions ----

RECORDED = [c for c in _cluster.cases() if not _cluster.flags_of(c)["indels"]]
GOLDEN = hc.golden_cases()


def kw_of_case(s, case):
    f = _cluster.flags_of(case)
    return dict(nucleotides=f["nucleotides"], ignore_genes=f["ignore_genes"], n_v_genes=max(1, len(s.v_names)),
                n_j_genes=max(1, len(s.j_names)))


@pytest.mark.parametrize("case", RECORDED + GOLDEN, ids=[c["name"] for c in RECORDED + GOLDEN])
def test_reference_partitions(case):
    assert len(RECORDED) == 29 and len(GOLDEN) == 5
    d = _cluster.flags_of(case)["differences"]
    assert d <= 2 if case in RECORDED else d >= 3
    s, keys = _cluster.read_input(case)
    label, size, clusters = _cluster.recorded_partition(case, keys)
    no = _cluster_table.printed(case, keys)[0]
    with HipOverlap(Options(device=0, **kw_of_case(s, case))) as h:
        got = h.hamming_cluster(s, d)
        table = h.hamming_cluster_table(s, d)
    assert_partition(got, label)
    assert np.array_equal(got[1], size) and got[2] == clusters
    assert np.array_equal(table[0].astype(np.int64) + 1, no)
    assert_table(table, table_of(label, s.count))


# ---- 3. agreement with the hashed path ----

@pytest.mark.parametrize("name,g", [("aa", False), ("aa", True), ("dense", False), ("dense", True)])
@pytest.mark.parametrize("d", [0, 1, 2])
def test_agreement_with_the_hashed_path(name, g, d):
    s = hc.set_of(name)
    hashed = Options(differences=d, device=0, **kw_of(name, g))
    want = compairr_amd.cluster(s, hashed)
    want_table = compairr_amd.cluster_table(s, hashed)
    with HipOverlap(Options(device=0, **kw_of(name, g))) as h:
        got = h.hamming_cluster(s, d)
        table = h.hamming_cluster_table(s, d)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert_table(table, want_table)
    if (name, d, g) in hc.FIGURES:
        assert_partition(got, hc.model(name, d, g)[0])


# ---- 4. both kernel forms and every staging ----

@pytest.mark.parametrize("nucleotides", [False, True], ids=["aa", "nt"])
@pytest.mark.parametrize("generic", [0, 1])
def test_lengths_at_the_word_and_form_edges(nucleotides, generic):
    s = _hamming.edge_sets(nucleotides)[0]
    bound = _hamming.REG_BOUND[nucleotides]
    assert {1, 1000, bound, bound + 1} <= set(s.lengths.tolist())
    d = _hamming.EDGE_D
    label = _cluster.model(s, _hamming.edge_options(nucleotides, differences=d))[0]
    assert 1 < int((label == np.arange(s.n)).sum()) < s.n
    assert_everything(s, dict(n_v_genes=1, n_j_genes=1, nucleotides=nucleotides), d, label,
                      {"hamming_generic": generic})


def test_a_reference_longer_than_the_staging_buffer():
    """20 000 amino acids are 5 000 packed words: the generic form stages such a reference in runs of words.  Row k
    has k substitutions, so rows k and m differ at |k - m| positions: one chain; the seventh row is far from all."""
    rng = np.random.default_rng(20)
    L = 20_000
    base = rng.integers(0, 20, size=L, dtype=np.uint8)
    rows = [base.copy() for _ in range(6)]
    for k, row in enumerate(rows):
        for p in ([0, L - 1] + [4_095 * 4 + 3, 4_096 * 4, 9_999])[:k]:
            row[p] = (row[p] + 1) % 20
    far = rng.integers(0, 20, size=L, dtype=np.uint8)
    s = _neighbors._set_of_rows(np.stack(rows[::-1] + [far]), 201, 2)
    kw = dict(n_v_genes=1, n_j_genes=1)
    for d, want in ((3, [0, 0, 0, 0, 0, 0, 6]), (1, [0, 0, 0, 0, 0, 0, 6]), (0, list(range(7)))):
        label = _cluster.model(s, Options(differences=d, **kw))[0]
        assert label.tolist() == want
        assert_everything(s, kw, d, label)


def test_every_staging_segment_count_and_form_gives_the_model_s_partition():
    """one group over 36 query workgroups, staged in pieces of 1, 3 or 512 references, in 1 to 64 segments: the
    giant component of d = 1 -g is reached only through chains across all of them"""
    s = hc.set_of("dense")
    label, size, clusters = hc.model("dense", 1, True)
    want_table = table_of(label, s.count)
    with HipOverlap(Options(device=0, **kw_of("dense", True))) as h:
        combos = list(itertools.product((1, 3, 512), (1, 2, 7, 64), (0, 1), (1,)))
        combos += [(0, 0, 0, 0), (0, 0, 1, 0), (3, 7, 0, 0)]
        for stage, seg, generic, snapshot in combos:
            for name, value in (("hamming_stage_refs", stage), ("hamming_segments", seg), ("hamming_generic", generic),
                                ("hamming_link_snapshot", snapshot)):
                h.set_tunable(name, value)
            got = h.hamming_cluster(s, 1)
            assert got[0].tobytes() == label.tobytes() and got[1].tobytes() == size.tobytes(), (stage, seg, generic)
            assert got[2] == clusters == 342
        assert_table(h.hamming_cluster_table(s, 1), want_table)
        assert h.get_tunable("hamming_group_us") > 0 and h.get_tunable("hamming_compare_us") > 0
        assert h.get_tunable("cluster_table_us") > 0 and h.get_tunable("cluster_links_us") == 0


# ---- 5. the device entry points ----

def subsets(names):
    return [tuple(n for n, keep in zip(names, mask) if not keep)
            for mask in itertools.product((True, False), repeat=len(names))]


def test_device_entry_points_write_what_is_documented():
    import torch
    s = hc.set_of("aa")
    n, d = s.n, 3
    label, size, clusters = hc.model("aa", d, False)
    want = table_of(label, s.count)
    with HipOverlap(Options(device=0, **kw_of("aa", False))) as h:
        view, keep = HipOverlap.device_view(s)
        for left_out in subsets(("label", "size")):
            bufs = {name: torch.full((n + 64,), POISON32, dtype=torch.int32, device="cuda") for name in ("label", "size")}
            torch.cuda.synchronize()
            k = h.hamming_cluster_device(view, d, *[0 if name in left_out else bufs[name].data_ptr()
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
            k = h.hamming_cluster_table_device(view, d, *[0 if name in left_out else b.data_ptr()
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
    s = hc.set_of("aa")
    label, size, clusters = hc.model("aa", 3, True)
    want = table_of(label, s.count)
    v = _view(s)
    with HipOverlap(Options(device=0, **kw_of("aa", True))) as h:
        for left_out in subsets(("label", "size")):
            out = {"label": np.full(s.n, POISON32, dtype=np.uint32), "size": np.full(s.n, POISON32, dtype=np.uint32)}
            k = C.c_uint64(12345)
            rc = h._lib.cmpr_hamming_cluster(h._ctx, C.byref(v), 3, *[None if name in left_out else out[name].ctypes.data
                                                                      for name in ("label", "size")], C.byref(k))
            assert (rc, k.value) == (CMPR_OK, clusters)
            for name, w in (("label", label), ("size", size)):
                assert (out[name] == POISON32).all() if name in left_out else np.array_equal(out[name], w)
        for left_out in subsets(TABLE_NAMES):
            out = [np.full(s.n + 1 if name == "cluster_start" else s.n, POISON64 if t == np.uint64 else POISON32, dtype=t)
                   for name, t in zip(TABLE_NAMES, TABLE_DTYPES)]
            k = C.c_uint64(12345)
            rc = h._lib.cmpr_hamming_cluster_table(h._ctx, C.byref(v), 3,
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
        assert h._lib.cmpr_hamming_cluster(h._ctx, C.byref(v), 3, None, None, None) == CMPR_OK
        assert h._lib.cmpr_hamming_cluster_table(h._ctx, C.byref(v), 3, None, None, None, None, None) == CMPR_OK


# ---- 6. the resident state is left alone ----

def test_resident_state_is_left_alone():
    s1, s2 = _hamming.aa_sets()
    other = hc.set_of("nt")
    aa_label = hc.model("aa", 3, False)[0]
    with HipOverlap(_hamming.options(differences=1, device=0)) as h:
        h.set_reference(s2, s1.longest)
        h.set_queries(s1)
        before, stats = h.overlap_matrix(), h.stats()
        assert_partition(h.hamming_cluster(s1, 3), aa_label)
        assert_table(h.hamming_cluster_table(s1, 3), table_of(aa_label, s1.count))
        assert h.shape == before.shape
        after = h.stats()
        assert (after.queries, after.matches, after.variants) == (stats.queries, stats.matches, stats.variants)
        assert np.array_equal(h.overlap_matrix(), before) and h.stats().matches == stats.matches
        # cmpr_cluster afterwards still works, at the context's own d
        want = _cluster.model(s1, _hamming.options(differences=1))
        for a, b in zip(h.cluster(s1), want):
            assert np.array_equal(a, b)
    # on a nucleotide context, another set than the resident one
    with HipOverlap(_hamming.options(differences=2, nucleotides=True, device=0)) as h:
        h.set_reference(other, other.longest)
        h.set_queries(other)
        before = h.overlap_matrix()
        assert_partition(h.hamming_cluster(hc.set_of("dense"), 2), hc.model("dense", 2, False)[0])
        assert np.array_equal(h.overlap_matrix(), before)


# ---- 7. refusals ----

def raw(h, name, v, d):
    """an entry point as it is declared, all arrays NULL: (code, n_clusters, message)"""
    clusters = C.c_uint64(12345)
    outs = (None,) * (4 if "table" in name else 2)
    rc = getattr(h._lib, name)(h._ctx, C.byref(v) if v is not None else None, d, *outs, C.byref(clusters))
    return rc, clusters.value, h._lib.cmpr_last_error(h._ctx).decode() if rc else ""


ENTRY_POINTS = ("cmpr_hamming_cluster", "cmpr_hamming_cluster_table")


def test_refusals():
    s = hc.set_of("aa")
    v = _view(s)
    with HipOverlap(_hamming.options(device=0)) as h:
        for name in ENTRY_POINTS:
            assert raw(h, name, v, -1) == (CMPR_EINVAL, 0, "Differences specified with -d or -differences cannot be negative.")
            assert raw(h, name, None, 3) == (CMPR_EINVAL, 0, "set view is NULL")
        h.set_tunable("work_shard_count", 2)
        for name in ENTRY_POINTS:
            rc, k, text = raw(h, name, v, 3)
            assert rc == CMPR_EUNSUPPORTED and k == 0 and text.startswith(name + ": ") and "work_shard_count > 1" in text
    with HipOverlap(_hamming.options(differences=1, indels=True, device=0)) as h:
        for name in ENTRY_POINTS:
            assert raw(h, name, v, 3) == (CMPR_EINVAL, 0, name + ": the all-against-all path has no indels")
    with HipOverlap(_hamming.options(existence=True, device=0)) as h:
        clusters = C.c_uint64(12345)                     # (the text cmpr_cluster gives)
        rc = h._lib.cmpr_cluster(h._ctx, C.byref(v), None, None, C.byref(clusters))
        text = h._lib.cmpr_last_error(h._ctx).decode()
        assert rc == CMPR_EINVAL and "clusters are not defined with options.existence" in text
        for name in ENTRY_POINTS:
            assert raw(h, name, v, 3) == (CMPR_EINVAL, 0, text)
    # no score plays a part: what the pair calls refuse of MH, Jaccard and ratio is accepted
    label = hc.model("aa", 3, False)[0]
    for score in ("mh", "jaccard", "ratio"):
        with HipOverlap(_hamming.options(score=score, device=0)) as h:
            assert_partition(h.hamming_cluster(s, 3), label)
            assert_table(h.hamming_cluster_table(s, 3), table_of(label, s.count))
    # a set the validation refuses: the same code and text as cmpr_set_reference
    bad = RepertoireSet(s.residues, s.offsets, s.v_gene, s.j_gene, s.repertoire, s.count.copy(),
                        s.repertoire_ids, s.v_names, s.j_names, AA)
    bad.count[17] = 0
    with HipOverlap(_hamming.options(device=0)) as h:
        with pytest.raises(HipError) as want:
            h.set_reference(bad)
    with HipOverlap(_hamming.options(device=0)) as h:
        for call in (lambda: h.hamming_cluster(bad, 3), lambda: h.hamming_cluster_table(bad, 3)):
            with pytest.raises(HipError) as e:
                call()
            assert (e.value.code, str(e.value)) == (want.value.code, str(want.value))
        assert_partition(h.hamming_cluster(s, 3), label)


# ---- 8. other cases ----

def empty_set():
    z = lambda t: np.zeros(0, dtype=t)
    return RepertoireSet(z(np.uint8), np.zeros(1, dtype=np.uint64), z(np.uint32), z(np.uint32), z(np.uint32),
                         z(np.uint64), ["T1", "T2"], ["V0", "V1"], ["J0", "J1"], AA)


def test_empty_set_is_ok_with_zero_clusters():
    import torch
    s = empty_set()
    v = _view(s)
    with HipOverlap(_hamming.options(device=0)) as h:
        label, size, clusters = h.hamming_cluster(s, 3)
        assert len(label) == 0 and len(size) == 0 and clusters == 0
        got = h.hamming_cluster_table(s, 3)
        assert [len(a) for a in got] == [0, 1, 0, 0] and got[1][0] == 0
        start = np.full(4, POISON64, dtype=np.uint64)
        count = np.full(4, POISON64, dtype=np.uint64)
        k = C.c_uint64(12345)
        assert h._lib.cmpr_hamming_cluster_table(h._ctx, C.byref(v), 3, None, start.ctypes.data, None,
                                                 count.ctypes.data, C.byref(k)) == CMPR_OK
        assert k.value == 0 and start.tolist() == [0] + [POISON64] * 3 and (count == POISON64).all()
        d_start = torch.full((4,), POISON64, dtype=torch.int64, device="cuda")
        d_count = torch.full((4,), POISON64, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        view, keep = HipOverlap.device_view(s)
        assert h.hamming_cluster_table_device(view, 3, 0, d_start.data_ptr(), 0, d_count.data_ptr()) == 0
        assert h.hamming_cluster_device(view, 3) == 0
        assert d_start.cpu().tolist() == [0] + [POISON64] * 3 and (d_count.cpu() == POISON64).all()
        del keep


def test_one_sequence():
    s = hc.set_of("aa").subset(slice(0, 1))
    with HipOverlap(_hamming.options(device=0)) as h:
        for d in (0, 3):
            label, size, clusters = h.hamming_cluster(s, d)
            assert (label.tolist(), size.tolist(), clusters) == ([0], [1], 1)
            got = h.hamming_cluster_table(s, d)
            assert [a.tolist() for a in got] == [[0], [0, 1], [0], [int(s.count[0])]]


def test_every_sequence_a_cluster_of_its_own():
    case = {"name": None, "args": "-d 4 -n -g", "files": ["rand_nt_a.tsv"]}
    s, _ = _cluster.read_input(case)
    label = _cluster.model(s, Options(differences=4, nucleotides=True, ignore_genes=True))[0]
    assert s.n == 300 and label.tolist() == list(range(300))
    assert_everything(s, kw_of_case(s, case), 4, label)


@pytest.mark.parametrize("name,g", [("aa", False), ("nt", True), ("empty", False), ("dense", True)])
def test_huge_d(name, g):
    """above the longest sequence: as that length -- every group one cluster"""
    s = hc.set_of(name)
    key = s.lengths.astype(np.int64) if g else (s.lengths.astype(np.int64) * 1000 + s.v_gene) * 1000 + s.j_gene
    first = {}
    label = np.array([first.setdefault(k, i) for i, k in enumerate(key.tolist())], dtype=np.uint32)
    with HipOverlap(Options(device=0, **kw_of(name, g))) as h:
        for d in (int(s.longest), 10 ** 9, 2 ** 62):
            assert_partition(h.hamming_cluster(s, d), label)
        assert_table(h.hamming_cluster_table(s, 10 ** 9), table_of(label, s.count))


def test_two_runs_give_the_same_bytes():
    s = hc.set_of("dense")
    opt = Options(device=0, **kw_of("dense", False))
    one = compairr_amd.hamming_cluster(s, opt, 2) + compairr_amd.hamming_cluster_table(s, opt, 2)
    two = compairr_amd.hamming_cluster(s, opt, 2) + compairr_amd.hamming_cluster_table(s, opt, 2)
    assert [np.asarray(a).tobytes() for a in one] == [np.asarray(b).tobytes() for b in two]
    assert_partition(one[:3], hc.model("dense", 2, False)[0])
