"""The all-against-all path without a GPU: the figures of the inputs the GPU tests use, from the oracle and from
the numpy brute force (tests/_hamming.py), which must agree; the helper's CSR on a hand-written case; the
reference's own d = 3 matrices against the brute force; and the header, the binding and the library carrying the
four entry points."""

import ctypes
import os
import re

import numpy as np
import pytest

import _hamming
import _neighbors
import _oracle
from compairr_amd import RepertoireSet, hip
from compairr_amd.sets import AA

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "compairr_hip.h")
SOURCE = os.path.join(HERE, "..", "compairr_amd", "csrc", "allpairs.h")
NAMES = ("cmpr_hamming_matrix", "cmpr_hamming_matrix_device", "cmpr_hamming_neighbors", "cmpr_hamming_neighbors_device")


@pytest.mark.parametrize("key", list(_hamming.EDGES), ids=["%s-d%d%s" % (k[0], k[1], "-g" if k[2] else "")
                                                           for k in _hamming.EDGES])
def test_figures_of_the_inputs(key):
    name, d, g = key
    s1, s2 = _hamming.sets_of(name)
    row_start, hits, dist = _hamming.want(name, d, g)
    opt = _hamming.options_of(name, g, differences=d)
    assert int(row_start[-1]) == len(hits) == _hamming.EDGES[key] == _oracle.overlap(s1, s2, opt)[1].matches
    if key in _hamming.HISTOGRAMS:
        assert _hamming.histogram(dist, d) == _hamming.HISTOGRAMS[key]
    if key in _hamming.LONGEST_ROW:
        assert _neighbors.shape_of(row_start)[1] == _hamming.LONGEST_ROW[key]
    if name != "dense" or d == 3:          # (the brute force of the largest cases adds nothing the others lack)
        brute = _hamming.brute_csr(s1, s2, d, g)
        assert np.array_equal(brute[0], row_start) and np.array_equal(brute[1], hits)
        assert np.array_equal(brute[2], dist)


def test_shapes_of_the_inputs():
    a, b = _hamming.aa_sets()
    keys = lambda s: set(zip(s.lengths.tolist(), s.v_gene.tolist(), s.j_gene.tolist()))
    assert len(keys(a) | keys(b)) == 28        # (groups of one set only: the hand-built sets below have them)
    row_start = _hamming.want("dense", 8, True)[0]
    assert np.array_equal(np.diff(row_start.astype(np.int64)), np.full(70, 9001))
    assert np.array_equal(_hamming.want("dense", 8, True)[1], np.tile(np.arange(9001, dtype=np.uint32), 70))
    deg = np.diff(_hamming.want("dense", 4, True)[0].astype(np.int64))
    assert (int(deg.min()), int(deg.max())) == (961, 1105)
    e, _ = _hamming.empty_sets()
    assert int((e.lengths == 0).sum()) == 39
    assert _hamming.same_group_pairs(*_hamming.dense_sets(), True) == 630_070


def test_csr_builder_on_a_hand_written_case():
    seqs1, seqs2 = ["CASS", "CAS", "", "WWWW"], ["CASS", "CTSA", "", "CAS", "CAWW", ""]

    def make(seqs, genes):
        res = np.array([AA.index(c) for s in seqs for c in s], dtype=np.uint8)
        off = np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)
        n = len(seqs)
        return RepertoireSet(res, off, np.array(genes, dtype=np.uint32), np.zeros(n, dtype=np.uint32),
                             np.zeros(n, dtype=np.uint32), np.ones(n, dtype=np.uint64), ["R1"], ["V0", "V1"], ["J0"], AA)
    s1, s2 = make(seqs1, [0, 0, 0, 0]), make(seqs2, [0, 0, 0, 1, 0, 1])
    rows, hits, dist = _hamming.brute_csr(s1, s2, 2, ignore_genes=True)
    assert rows.tolist() == [0, 3, 4, 6, 7] and hits.tolist() == [0, 1, 4, 3, 2, 5, 4]
    assert dist.dtype == np.uint16 and dist.tolist() == [0, 2, 2, 0, 0, 0, 2]
    rows, hits, dist = _hamming.brute_csr(s1, s2, 2, ignore_genes=False)
    assert rows.tolist() == [0, 3, 3, 4, 5] and hits.tolist() == [0, 1, 4, 2, 4]
    assert np.array_equal(_hamming.distances(s1, s2, rows, hits), dist)
    assert _hamming.same_group_pairs(s1, s2, True) == 2 * 3 + 1 + 2 and _hamming.same_group_pairs(s1, s2, False) == 7


@pytest.mark.parametrize("nucleotides", [False, True], ids=["aa", "nt"])
def test_lengths_at_the_word_and_form_edges(nucleotides):
    """the oracle and the brute force agree on the hand-built set; a mutant with k substitutions lies at distance
    k of its base; the sequence one residue longer never matches the base it was made of"""
    s1, s2, ks = _hamming.edge_sets(nucleotides)
    bound = _hamming.REG_BOUND[nucleotides]
    assert bound in s2.lengths and bound + 1 in s2.lengths and 1000 in s2.lengths
    opt = _hamming.edge_options(nucleotides, differences=_hamming.EDGE_D)
    want = _hamming.oracle_want(s1, s2, opt)
    brute = _hamming.brute_csr(s1, s2, _hamming.EDGE_D)
    for a, b in zip(want, brute):
        assert np.array_equal(a, b)
    rows = want[0].astype(np.int64)
    base_of = {int(L): j for j, L in enumerate(s2.lengths)}
    for i, k in enumerate(ks):
        hits = want[1][rows[i]:rows[i + 1]].tolist()
        dist = want[2][rows[i]:rows[i + 1]].tolist()
        if k < 0:
            assert base_of[int(s1.lengths[i]) - 1] not in hits
        elif k <= _hamming.EDGE_D:
            assert dist[hits.index(base_of[int(s1.lengths[i])])] == k
        else:
            assert base_of[int(s1.lengths[i])] not in hits


@pytest.mark.parametrize("name", list(_hamming.GOLDEN))
def test_brute_force_gives_the_reference_matrices(name):
    """the reference's own -d 3 output: product of the counts summed over the brute force's pairs"""
    a, b = _hamming.golden_sets(name)
    rows, hits, _ = _hamming.brute_csr(a, b, 3)
    q = np.repeat(np.arange(a.n), np.diff(rows.astype(np.int64)))
    m = np.zeros((a.n_repertoires, b.n_repertoires), dtype=np.uint64)
    np.add.at(m, (a.repertoire[q], b.repertoire[hits]), a.count[q] * b.count[hits])
    cells = _hamming.golden_cells(name)
    assert len(cells) == m.size
    for (r, c), text in cells.items():
        assert "%.10g" % float(m[a.repertoire_ids.index(r), b.repertoire_ids.index(c)]) == text


def test_the_form_bound_of_the_helper_is_the_kernel_s():
    with open(SOURCE) as fh:
        text = fh.read()
    assert re.search(r"constexpr uint32_t HAMMING_REG_WORDS = (\d+);", text).group(1) == str(_hamming.REG_WORDS)
    assert "AA_PER_WORD = 4, NT_PER_WORD = 16" in text


def test_header_binding_and_library_carry_the_entry_points():
    with open(HEADER) as fh:
        text = fh.read()
    lib = ctypes.CDLL(hip.library_path())
    for name in NAMES:
        assert re.search(r"^int %s\(cmpr_context \*ctx, const cmpr_set_view \*(d_)?set1, "
                         r"const cmpr_set_view \*(d_)?set2,$" % name, text, re.M), name
        assert name in hip.EXPORTS
        assert hasattr(lib, name), name
        assert name.replace("_device", "") + "*" in text.split("#define CMPR_ABI_VERSION")[0]
    assert text.count("overlap.cc:286-359") >= 4
    assert "#define CMPR_ABI_VERSION 5" in text
    assert lib.cmpr_abi_version() == 5
    for name in ("hamming_stage_refs", "hamming_segments", "hamming_generic", "hamming_group_us",
                 "hamming_compare_us", "hamming_copy_us"):
        assert '"%s"' % name in text, name
