"""cmpr_edit_cluster / cmpr_edit_cluster_table without a GPU: the figures of the inputs the GPU tests use, from the
yardstick (tests/_edit_cluster.py: the components of the Levenshtein brute force's pairs); the equality with the indel
model at d = 1; the chain built by hand; the conditions on the sets at the word edges; and the header, the binding and
the library carrying the four entry points."""

import ctypes
import os
import re

import numpy as np
import pytest

import _cluster
import _cluster_table
import _edit
import _edit_cluster as ec
import compairr_amd
from compairr_amd import HipOverlap, hip

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "compairr_hip.h")
NAMES = ("cmpr_edit_cluster", "cmpr_edit_cluster_device", "cmpr_edit_cluster_table", "cmpr_edit_cluster_table_device")


@pytest.mark.parametrize("key", ec.KEYS, ids=ec.ids_of(ec.KEYS))
def test_figures_of_the_inputs(key):
    name, d, g = key
    s = ec.set_of(name)
    label, size, clusters = ec.want(name, d, g)
    assert ec.figures_of(label, size) == ec.FIGURES[key] and clusters == ec.FIGURES[key][0]
    assert label.dtype == np.uint32 and (label <= np.arange(s.n)).all() and np.array_equal(label[label], label)
    table = _cluster_table.table_of(label, s.count)
    assert len(table[1]) == clusters + 1 and int(table[1][1]) == ec.FIGURES[key][1]


def test_shapes_of_the_inputs():
    for name in ("nt", "aa", "min0"):
        assert ec.set_of(name).n == 300
    s = ec.dense_set()
    assert s.n == 1800 and dict(zip(*[a.tolist() for a in np.unique(s.lengths, return_counts=True)])) == ec.DENSE_GROUPS
    # the giant component of d = 2 -g has members of all three lengths
    label, size, _ = ec.want("dense", 2, True)
    giant = np.flatnonzero(size == 1773)
    assert len(np.unique(label[giant])) == 1 and set(s.lengths[giant].tolist()) == {7, 8, 9}


@pytest.mark.parametrize("key", ec.D1_KEYS, ids=ec.ids_of(ec.D1_KEYS))
def test_at_d1_the_partition_is_the_indel_model_s(key):
    """also on min0, where the pair lists differ (variants.cc:301): a link has no direction"""
    name, _, g = key
    label, size, clusters = ec.want(name, 1, g)
    want = ec.indel_model(name, g)
    assert np.array_equal(label, want[0]) and np.array_equal(size, want[1]) and clusters == want[2]


@pytest.mark.parametrize("name", ["nt", "aa", "min0"])
def test_at_d0_the_partition_is_the_hamming_model_s(name):
    for g in (False, True):
        want = _cluster.model(ec.set_of(name), compairr_amd.Options(differences=0, **ec.kw_of(name, g)))
        assert np.array_equal(ec.want(name, 0, g)[0], want[0])


def test_hamming_clusters_lie_inside_edit_clusters():
    for name in ("nt", "aa"):
        for g in (False, True):
            plain = _cluster.model(ec.set_of(name), compairr_amd.Options(differences=3, **ec.kw_of(name, g)))[0]
            assert ec.refines(plain, ec.want(name, 3, g)[0])
    assert not ec.refines(ec.want("aa", 3, False)[0], ec.want("aa", 2, False)[0])


def test_the_chain_built_by_hand():
    s = ec.chain_set()
    assert s.n == 11 and sorted(s.lengths[:10].tolist()) == list(range(21, 31)) and int(s.lengths[0]) != 21
    assert ec.want("chain", 1, False)[0].tolist() == ec.CHAIN_LABEL
    assert ec.want("chain", 0, False)[0].tolist() == list(range(11)) and ec.want("chain", 0, False)[2] == 11


@pytest.mark.parametrize("nucleotides", [False, True], ids=["aa", "nt"])
def test_sets_at_the_word_edges(nucleotides):
    s = ec.edge_set(nucleotides)
    s1, s2, _, _ = _edit.edge_sets(nucleotides)
    assert s.n == s1.n + s2.n and s.longest == _edit.MAX_LEN
    assert s.sequence(s1.n) == s2.sequence(0) and s.sequence(s.n - 1) == s2.sequence(s2.n - 1)
    label, size, clusters = ec.want("edge_nt" if nucleotides else "edge_aa", _edit.EDGE_D, False)
    assert 1 < clusters < s.n
    lengths = s.lengths
    for bound in (64, 128):
        spans = [lab for lab in np.unique(label).tolist()
                 if lengths[label == lab].min() <= bound < lengths[label == lab].max()]
        assert spans, bound


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
        assert hip._argtypes()[name] == hip._argtypes()[name.replace("cmpr_edit_", "cmpr_hamming_")]
    assert text.index("int cmpr_edit_matrix_device(") < text.index("int cmpr_edit_cluster(")
    assert "#define CMPR_ABI_VERSION 5" in text
    assert lib.cmpr_abi_version() == 5
    assert '"edit_link_snapshot"' in text
    for name in ("edit_cluster", "edit_cluster_device", "edit_cluster_table", "edit_cluster_table_device"):
        assert callable(getattr(HipOverlap, name))
    assert callable(compairr_amd.edit_cluster) and callable(compairr_amd.edit_cluster_table)
