"""Clustering without a GPU: the Python statement of what cmpr_cluster computes (tests/_cluster.py model)
gives, for every recorded `-c` run of the reference (tests/golden/manifest.json, expected/c_*.tsv), the
partition the reference printed -- label = the cluster's first printed row = its smallest input number, size
= its cluster_size column, count = its number of clusters -- which ties the model the GPU tests compare
against to the real reference; and the header, the binding and the library carry the two entry points."""

import ctypes
import os
import re

import numpy as np
import pytest

import _cluster
from compairr_amd import hip

CASES = _cluster.cases()
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "compairr_hip.h")


def test_there_are_43_recorded_cases():
    assert len(CASES) == 43
    assert {(_cluster.flags_of(c)["differences"], _cluster.flags_of(c)["indels"]) for c in CASES} == \
        {(0, False), (1, False), (1, True), (2, False)}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_reproduces_the_reference(case):
    s, keys = _cluster.read_input(case)
    want = _cluster.recorded_partition(case, keys)
    got = _cluster.model(s, _cluster.options_of(s, case))
    assert got[2] == want[2]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert want[2] == int((want[0] == np.arange(s.n)).sum())


def test_labels_of_pairs_is_a_union_find():
    rng = np.random.default_rng(7)
    n = 3000
    q, h = rng.integers(0, n, 2000), rng.integers(0, n, 2000)
    parent = list(range(n))

    def root(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for a, b in zip(q.tolist(), h.tolist()):
        ra, rb = root(a), root(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    assert _cluster.labels_of_pairs(n, q, h).tolist() == [root(i) for i in range(n)]
    # a path of 1000 edges, listed from the far end
    assert not _cluster.labels_of_pairs(1001, np.arange(1000, 0, -1), np.arange(999, -1, -1)).any()


def test_header_binding_and_library_carry_the_entry_points():
    with open(HEADER) as fh:
        text = fh.read()
    lib = ctypes.CDLL(hip.library_path())
    for name in ("cmpr_cluster", "cmpr_cluster_device"):
        assert re.search(r"^int %s\(cmpr_context \*ctx, const cmpr_set_view \*" % name, text, re.M), name
        assert name in hip.EXPORTS
        assert hasattr(lib, name), name
    assert "#define CMPR_ABI_VERSION 5" in text
    assert lib.cmpr_abi_version() == 5
