"""cmpr_cluster_table / cmpr_cluster_table_device on the GPU: the reference's own cluster numbers for the recorded
`-c` cases, a crafted partition (clusters far beyond a wave, thousands of small ones, ties in size) against the
numpy yardstick over cmpr_cluster's labels, both entry points, what stays resident, independence from tunables
and options, and the contract of the entry points."""

import ctypes as C
import functools

import numpy as np
import pytest

import _cluster
import _cluster_table
import compairr_amd
from _cluster_table import table_of
from compairr_amd import HipError, HipOverlap, Options, RepertoireSet, synth

pytestmark = pytest.mark.gpu

CASES = _cluster.cases()
CMPR_EINVAL, CMPR_EUNSUPPORTED = 1, 4
FULL = dict(n_v_genes=synth.N_V, n_j_genes=synth.N_J)
# (score: the validation every set goes through bounds a repertoire's summed counts so that an INTEGER score's cell
# stays below 2^63 -- with the crafted sets' counts of up to 2^40 the library says "duplicate counts too large for
# exact 64-bit accumulation", as cmpr_cluster does --; the ratio score has no such bound, and no score plays a
# part in the clusters or their summed counts)
ONE_GENE = dict(differences=1, n_v_genes=1, n_j_genes=1, score="ratio", device=0)
NAMES = ("cluster_of", "cluster_start", "members", "count")
DTYPES = (np.uint32, np.uint64, np.uint32, np.uint64)
SENTINEL32, SENTINEL64 = 0x25A5A5A5, 0x25A5A5A5A5A5A5A5


def assert_table(got, want):
    for name, dtype, g, w in zip(NAMES, DTYPES, got, want):
        assert g.dtype == dtype, name
        assert g.shape == w.shape and np.array_equal(g, w), name


# ---- 1. the recorded cases ----

@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_recorded_cases(case):
    s, keys = _cluster.read_input(case)
    label = _cluster.recorded_partition(case, keys)[0]
    no = _cluster_table.printed(case, keys)[0]
    got = compairr_amd.cluster_table(s, _cluster.options_of(s, case, device=0))
    assert np.array_equal(got[0].astype(np.int64) + 1, no)
    assert_table(got, table_of(label, s.count))


# ---- 2. a crafted partition ----

CUBES = (17, 14, 13, 7, 6)
GROUPS = [(2, 1000), (3, 1000), (1, 5000), (63, 1), (64, 1), (65, 1), (324, 1)]


@functools.lru_cache(maxsize=None)
def crafted(contiguous):
    s, label = _cluster_table.crafted(CUBES, GROUPS, seed=2024, contiguous=contiguous)
    label.setflags(write=False)
    return s, label


@pytest.mark.parametrize("contiguous", [False, True], ids=["shuffled", "contiguous"])
def test_crafted_partition(contiguous):
    s, built = crafted(contiguous)
    assert s.n == 166356 and s.n % 256
    label, size, clusters = compairr_amd.cluster(s, Options(**ONE_GENE))
    assert np.array_equal(label, built) and clusters == 5 + 7004
    want = table_of(label, s.count)
    got = compairr_amd.cluster_table(s, Options(**ONE_GENE))
    assert_table(got, want)
    # what the construction promises: the sizes in order, the tie of the two clusters of 64, sums beyond 32 bits
    sizes = np.diff(got[1].astype(np.int64))
    assert sizes[:9].tolist() == [131072, 16384, 8192, 324, 128, 65, 64, 64, 63]
    assert got[2][int(got[1][6])] < got[2][int(got[1][7])]
    assert int(got[3].max()) > 1 << 50


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
def test_small_sets(n):
    whole = _cluster_table.crafted((5, 6), [(2, 10), (3, 10), (1, 20), (19, 1), (20, 1), (37, 1), (64, 1)], seed=11,
                                   contiguous=False)[0]
    s = whole.subset(slice(0, n))
    label, size, clusters = compairr_amd.cluster(s, Options(**ONE_GENE))
    got = compairr_amd.cluster_table(s, Options(**ONE_GENE))
    assert len(got[1]) == clusters + 1
    assert_table(got, table_of(label, s.count))


# ---- 3. both entry points ----

@functools.lru_cache(maxsize=None)
def medium_set():
    return synth.make_set(20_000, 32, pool_size=3000)


def device_table(h, s, leave_out=()):
    """cluster_table_device into sentinel-filled torch buffers with 64 elements to spare: (the four arrays as numpy,
    whole, K)"""
    import torch
    view, keep = HipOverlap.device_view(s)
    bufs = [torch.full((s.n + 64,), SENTINEL32, dtype=torch.int32, device="cuda"),
            torch.full((s.n + 1 + 64,), SENTINEL64, dtype=torch.int64, device="cuda"),
            torch.full((s.n + 64,), SENTINEL32, dtype=torch.int32, device="cuda"),
            torch.full((s.n + 64,), SENTINEL64, dtype=torch.int64, device="cuda")]
    torch.cuda.synchronize()
    k = h.cluster_table_device(view, *[0 if name in leave_out else b.data_ptr() for name, b in zip(NAMES, bufs)])
    del keep
    return [b.cpu().numpy().view(t) for b, t in zip(bufs, DTYPES)], k


def assert_device_table(arrays, k, n, want, leave_out=()):
    lengths = (n, k + 1, n, k)
    for name, a, m, w in zip(NAMES, arrays, lengths, want):
        sentinel = SENTINEL64 if a.dtype == np.uint64 else SENTINEL32
        if name in leave_out:
            assert (a == sentinel).all(), name
        else:
            assert np.array_equal(a[:m], w), name
            assert (a[m:] == sentinel).all(), name     # (behind K + 1 and K: not the call's to write)


def test_device_entry_point_sentinels_and_repeated_calls():
    s = medium_set()
    opt = Options(differences=1, indels=True, device=0, **FULL)
    with HipOverlap(opt) as h:
        one = h.cluster_table(s)
        two = h.cluster_table(s)
        arrays, k = device_table(h, s)
        assert h.get_tunable("cluster_links_us") > 0 and h.get_tunable("cluster_table_us") > 0
        again, k2 = device_table(h, s)
        label = h.cluster(s)[0]
    assert 1 < k < s.n and k == k2 == len(one[3])
    assert_table(one, table_of(label, s.count))
    assert_table(two, one)
    assert_device_table(arrays, k, s.n, one)
    for a, b in zip(arrays, again):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("left_out", NAMES + (NAMES,), ids=list(NAMES) + ["all"])
def test_outputs_may_be_left_out(left_out):
    left_out = (left_out,) if isinstance(left_out, str) else left_out
    s = medium_set()
    with HipOverlap(Options(differences=1, device=0, **FULL)) as h:
        want = h.cluster_table(s)
        arrays, k = device_table(h, s, leave_out=left_out)
        assert k == len(want[3])
        assert_device_table(arrays, k, s.n, want, leave_out=left_out)
        # the host variant, as declared
        host = [np.full(s.n + 1 if name == "cluster_start" else s.n, SENTINEL64 if t == np.uint64 else SENTINEL32, dtype=t)
                for name, t in zip(NAMES, DTYPES)]
        v = compairr_amd.hip._view(s)
        clusters = C.c_uint64(12345)
        rc = h._lib.cmpr_cluster_table(h._ctx, C.byref(v), *[None if name in left_out else a.ctypes.data
                                                              for name, a in zip(NAMES, host)], C.byref(clusters))
        assert (rc, clusters.value) == (0, k)
        assert_device_table(host, k, s.n, want, leave_out=left_out)
        # the count may be left out too
        assert h._lib.cmpr_cluster_table(h._ctx, C.byref(v), None, None, None, None, None) == 0


# ---- 4. what stays resident ----

def test_the_set_stays_resident_as_both_sets():
    s = medium_set()
    opt = Options(differences=1, device=0, **FULL)
    with HipOverlap(opt) as fresh:
        fresh.set_reference(s, s.longest)
        fresh.set_queries(s)
        matrix = fresh.overlap_matrix()
    with HipOverlap(opt) as fresh:
        clusters_fresh = fresh.cluster(s)
    with HipOverlap(opt) as h:
        got = h.cluster_table(s)
        assert h.shape == matrix.shape
        assert np.array_equal(h.overlap_matrix(), matrix)
        after = h.cluster(s)
        assert np.array_equal(h.overlap_matrix(), matrix)
    for a, b in zip(after, clusters_fresh):
        assert np.array_equal(a, b)
    assert_table(got, table_of(clusters_fresh[0], s.count))


# ---- 5. independence from tunables, parts and options ----

@functools.lru_cache(maxsize=None)
def big_set():
    return synth.make_set(200_000, 30)


@functools.lru_cache(maxsize=None)
def big_labels():
    label = compairr_amd.cluster(big_set(), Options(differences=1, device=0, **FULL))[0]
    label.setflags(write=False)
    return label


@pytest.mark.parametrize("how", ["default", "parts", "ignore_counts"])
def test_big_set_under_tunables_parts_and_ignore_counts(how):
    s, label = big_set(), big_labels()
    opt = Options(differences=1, device=0, ignore_counts=how == "ignore_counts", **FULL)
    with HipOverlap(opt) as h:
        if how == "parts":
            h.set_tunable("part_buckets_log2", 17)
        got = h.cluster_table(s)
        if how == "parts":
            assert h.get_tunable("reference_parts") >= 3
    print("%s: %d sequences, %d clusters, largest %d" % (how, s.n, len(got[3]), int(got[1][1])))
    assert 1 < len(got[3]) < s.n
    assert_table(got, table_of(label, np.ones(s.n, dtype=np.uint64) if how == "ignore_counts" else s.count))


# ---- 6. the contract ----

def raw(h, name, s):
    """an entry point as it is declared, all arrays NULL: (code, n_clusters, message)"""
    v = compairr_amd.hip._view(s) if s is not None else None
    clusters = C.c_uint64(12345)
    args = (None,) * (4 if "table" in name else 2)
    rc = getattr(h._lib, name)(h._ctx, C.byref(v) if v is not None else None, *args, C.byref(clusters))
    return rc, clusters.value, h._lib.cmpr_last_error(h._ctx).decode() if rc else ""


def test_refusals_are_those_of_cmpr_cluster():
    s = medium_set()
    plain = Options(differences=1, device=0, **FULL)
    for opt, tunable, code in ((plain, None, CMPR_EINVAL), (plain, "work_shard_count", CMPR_EUNSUPPORTED),
                               (Options(differences=1, existence=True, device=0, **FULL), None, CMPR_EINVAL)):
        with HipOverlap(opt) as h:
            if tunable:
                h.set_tunable(tunable, 2)
            which = None if opt is plain and not tunable else s        # (the NULL set on the plain context)
            want = raw(h, "cmpr_cluster", which)
            assert want[0] == code and want[2]
            for name in ("cmpr_cluster_table", "cmpr_cluster_table_device"):
                assert raw(h, name, which) == want, name


def empty_set():
    z = lambda t: np.zeros(0, dtype=t)
    return RepertoireSet(z(np.uint8), np.zeros(1, dtype=np.uint64), z(np.uint32), z(np.uint32), z(np.uint32),
                         z(np.uint64), ["T1"])


def test_empty_set_is_ok_with_zero_clusters():
    import torch
    s = empty_set()
    with HipOverlap(Options(differences=1, device=0, **FULL)) as h:
        got = h.cluster_table(s)
        assert [len(a) for a in got] == [0, 1, 0, 0] and got[1][0] == 0
        # nothing written but cluster_start[0]
        start = np.full(4, SENTINEL64, dtype=np.uint64)
        count = np.full(4, SENTINEL64, dtype=np.uint64)
        v = compairr_amd.hip._view(s)
        clusters = C.c_uint64(12345)
        assert h._lib.cmpr_cluster_table(h._ctx, C.byref(v), None, start.ctypes.data, None, count.ctypes.data,
                                         C.byref(clusters)) == 0
        assert clusters.value == 0 and start.tolist() == [0] + [SENTINEL64] * 3 and (count == SENTINEL64).all()
        d_start = torch.full((4,), SENTINEL64, dtype=torch.int64, device="cuda")
        d_count = torch.full((4,), SENTINEL64, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        view, keep = HipOverlap.device_view(s)
        assert h.cluster_table_device(view, 0, d_start.data_ptr(), 0, d_count.data_ptr()) == 0
        assert d_start.cpu().tolist() == [0] + [SENTINEL64] * 3 and (d_count.cpu() == SENTINEL64).all()
        del keep


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
            h.cluster_table(s)
    assert (got.value.code, str(got.value)) == (want.value.code, str(want.value))
