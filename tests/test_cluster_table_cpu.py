"""The cluster table without a GPU: the numpy yardstick of the GPU tests (tests/_cluster_table.py table_of)
reproduces, for every recorded `-c` run of the reference, the print-out itself -- the cluster_no of every row,
its cluster_size, the member set of every cluster and the row each cluster starts with --; the library, the
header and the binding carry the two entry points; and the crafted set of the GPU tests has, at reduced size,
the partition its constructor says it has (tests/_cluster.py model, brute force)."""

import ctypes
import os
import re

import numpy as np
import pytest

import _cluster
import _cluster_table
from compairr_amd import HipOverlap, Options, hip

CASES = _cluster.cases()
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "compairr_hip.h")
ENTRY_POINTS = ("cmpr_cluster_table", "cmpr_cluster_table_device")
CMPR_EINVAL = 1


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_table_of_reproduces_the_print_out(case):
    s, keys = _cluster.read_input(case)
    label, size, clusters = _cluster.recorded_partition(case, keys)
    no, printed_size, rows = _cluster_table.printed(case, keys)
    cluster_of, cluster_start, members, count = _cluster_table.table_of(label, s.count)
    assert len(cluster_start) == clusters + 1 and len(count) == clusters
    assert np.array_equal(cluster_of.astype(np.int64) + 1, no)
    assert np.array_equal(np.diff(cluster_start.astype(np.int64))[cluster_of], printed_size)
    # the rows of a cluster are printed together; its members are those rows, its first member the first of them
    printed_members = {}
    for i in rows:
        printed_members.setdefault(int(no[i]), []).append(i)
    assert [int(no[i]) for i in rows] == sorted(int(no[i]) for i in rows)
    for k in range(clusters):
        mine = members[int(cluster_start[k]):int(cluster_start[k + 1])].tolist()
        assert mine == sorted(printed_members[k + 1])
        assert mine[0] == printed_members[k + 1][0] == label[mine[0]]
        assert int(count[k]) == int(s.count[mine].sum())


def test_table_of_orders_ties_by_the_smallest_member():
    label = np.array([0, 1, 1, 3, 0, 5, 3, 7, 7, 7])
    cluster_of, cluster_start, members, count = _cluster_table.table_of(label, np.arange(10) + 1)
    assert cluster_of.tolist() == [1, 2, 2, 3, 1, 4, 3, 0, 0, 0]
    assert cluster_start.tolist() == [0, 3, 5, 7, 9, 10]
    assert members.tolist() == [7, 8, 9, 0, 4, 1, 2, 3, 6, 5]
    assert count.tolist() == [27, 6, 5, 11, 6]
    assert (cluster_of.dtype, cluster_start.dtype, members.dtype, count.dtype) == \
        (np.uint32, np.uint64, np.uint32, np.uint64)


def test_header_binding_and_library_carry_the_entry_points():
    with open(HEADER) as fh:
        text = fh.read()
    lib = ctypes.CDLL(hip.library_path())
    for name in ENTRY_POINTS:
        assert re.search(r"^int %s\(cmpr_context \*ctx, const cmpr_set_view \*" % name, text, re.M), name
        assert name in hip.EXPORTS
        assert hasattr(lib, name), name
    for name in ("cluster_links_us", "cluster_table_us"):
        assert '"%s"' % name in text
    assert "#define CMPR_ABI_VERSION 5" in text and lib.cmpr_abi_version() == 5


def test_hip_overlap_has_both_methods():
    assert callable(HipOverlap.cluster_table) and callable(HipOverlap.cluster_table_device)
    import compairr_amd
    assert callable(compairr_amd.cluster_table)


def test_a_null_context_is_refused_before_any_device_work():
    lib = hip.load_library()
    view = hip._SetView()
    clusters = ctypes.c_uint64(12345)
    for name in ENTRY_POINTS:
        assert getattr(lib, name)(None, ctypes.byref(view), None, None, None, None, ctypes.byref(clusters)) == CMPR_EINVAL
        assert clusters.value == 12345


# ---- the crafted set of tests/test_cluster_table_gpu.py, small enough for brute force ----

@pytest.mark.parametrize("contiguous", [False, True], ids=["shuffled", "contiguous"])
def test_the_crafted_set_has_the_partition_it_is_built_for(contiguous):
    groups = [(2, 10), (3, 10), (1, 20), (19, 1), (20, 1), (37, 1), (64, 1)]
    s, label = _cluster_table.crafted((5, 6), groups, seed=11, contiguous=contiguous)
    assert s.n == 32 + 64 + 20 + 30 + 20 + 19 + 20 + 37 + 64
    got = _cluster.model(s, Options(differences=1, n_v_genes=1, n_j_genes=1))
    assert got[2] == 2 + 44
    assert np.array_equal(got[0], label)
    assert sorted(np.bincount(label)[np.unique(label)].tolist(), reverse=True)[:6] == [64, 64, 37, 32, 20, 19]
    if contiguous:
        assert (np.diff(label.astype(np.int64)) >= 0).all()
    assert int(s.count.max()) >= 1 << 32
