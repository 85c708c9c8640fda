"""Clusters at any d without a GPU: the header, the binding and the library carry the four entry points; the figures
of the inputs the GPU tests use, from the model (tests/_cluster.py) and from a union-find over the brute-force pair
list (tests/_hamming.py), which must agree, a sample also with the oracle's pair list; and the reference's own `-c`
runs at d >= 3 against the model."""

import ctypes
import os
import re

import numpy as np
import pytest

import _cluster
import _cluster_table
import _hamming
import _hamming_cluster as hc
import _neighbors
import compairr_amd
from compairr_amd import HipOverlap, hip

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "compairr_hip.h")
NAMES = ("cmpr_hamming_cluster", "cmpr_hamming_cluster_device", "cmpr_hamming_cluster_table",
         "cmpr_hamming_cluster_table_device")
CMPR_EINVAL = 1


def test_header_binding_and_library_carry_the_entry_points():
    with open(HEADER) as fh:
        text = fh.read()
    lib = ctypes.CDLL(hip.library_path())
    for name in NAMES:
        assert re.search(r"^int %s\(cmpr_context \*ctx, const cmpr_set_view \*(d_)?set, int64_t differences,$" % name,
                         text, re.M), name
        assert name in hip.EXPORTS
        assert hasattr(lib, name), name
        assert name.replace("_device", "") + "*" in text.split("#define CMPR_ABI_VERSION")[0]
    assert text.count("cluster.cc:165-211") >= 4
    assert "#define CMPR_ABI_VERSION 5" in text
    assert lib.cmpr_abi_version() == 5
    for method in ("hamming_cluster", "hamming_cluster_device", "hamming_cluster_table", "hamming_cluster_table_device"):
        assert callable(getattr(HipOverlap, method))
    assert callable(compairr_amd.hamming_cluster) and callable(compairr_amd.hamming_cluster_table)


def test_a_null_context_is_refused_before_any_device_work():
    lib = hip.load_library()
    view = hip._SetView()
    clusters = ctypes.c_uint64(12345)
    for name in NAMES:
        outs = (None,) * (4 if "table" in name else 2)
        assert getattr(lib, name)(None, ctypes.byref(view), 3, *outs, ctypes.byref(clusters)) == CMPR_EINVAL
        assert clusters.value == 12345


@pytest.mark.parametrize("key", hc.KEYS, ids=hc.IDS)
def test_figures_of_the_inputs(key):
    name, d, g = key
    s = hc.set_of(name)
    label, size, clusters = hc.model(name, d, g)
    assert hc.figures_of(label, size) == hc.FIGURES[key] and clusters == hc.FIGURES[key][0]
    row_start, hits, _ = _hamming.brute_csr(s, s, d, g)
    q = np.repeat(np.arange(s.n), np.diff(row_start.astype(np.int64)))
    by_pairs = _cluster.labels_of_pairs(s.n, q, hits)
    assert np.array_equal(by_pairs, label)
    assert np.array_equal(_cluster.sizes_of_labels(by_pairs), size)
    if key in (("aa", 3, False), ("nt", 3, True), ("empty", 3, False), ("dense", 3, True)):
        o_rows, o_hits = _neighbors.oracle_csr(s, s, _hamming.options_of(name, g, differences=d))
        assert np.array_equal(o_rows, row_start) and np.array_equal(o_hits, hits)


def test_shapes_of_the_inputs():
    assert hc.set_of("dense").n == 9001 and (hc.set_of("dense").lengths == 8).all()
    assert [hc.set_of(name).n for name in ("aa", "nt", "empty")] == [300, 300, 200]
    assert int((hc.set_of("empty").lengths == 0).sum()) == 39
    # the pairs the link sink skips at d = 3: 2.2 million, one component
    row_start = _hamming.brute_csr(hc.set_of("dense"), hc.set_of("dense"), 3, True)[0]
    assert 2_200_000 < int(row_start[-1]) < 2_300_000


GOLDEN = hc.golden_cases()


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_reference_goldens_against_the_model(case):
    f = _cluster.flags_of(case)
    assert f["differences"] >= 3 and not f["indels"] and case["cmd"] == "-c" and case["exit"] == 0
    s, keys = _cluster.read_input(case)
    assert len(set(keys)) == len(keys)
    label, size, clusters = _cluster.recorded_partition(case, keys)
    assert (clusters, int(size.max())) == hc.GOLDEN_FIGURES[case["name"]]
    want = _cluster.model(s, _cluster.options_of(s, case))
    assert np.array_equal(label, want[0]) and np.array_equal(size, want[1]) and clusters == want[2]
    no, printed_size, rows = _cluster_table.printed(case, keys)
    cluster_of, cluster_start, members, count = _cluster_table.table_of(label, s.count)
    assert np.array_equal(cluster_of.astype(np.int64) + 1, no)
    assert np.array_equal(np.diff(cluster_start.astype(np.int64))[cluster_of], printed_size)
    assert [int(no[i]) for i in rows] == sorted(int(no[i]) for i in rows)


def test_the_golden_manifest_lists_what_is_recorded():
    assert sorted(c["name"] for c in GOLDEN) == sorted(hc.GOLDEN_FIGURES)
    for c in GOLDEN:
        assert os.path.exists(os.path.join(_cluster.EXPECTED, c["name"] + ".tsv"))
        assert os.path.exists(os.path.join(_cluster.INPUTS, c["files"][0]))
