"""Helpers of the tests of cmpr_edit_cluster / cmpr_edit_cluster_table (not a test module): the inputs and figures the
CPU and GPU tests share, and the yardstick's partition of each, computed once -- the connected components
(tests/_cluster.py labels_of_pairs) of the Levenshtein brute force's pair list (tests/_edit.py brute_csr).  Nothing
here calls the library under test."""

import functools

import numpy as np

import _cluster
import _edit
from compairr_amd import Options, RepertoireSet, synth
from compairr_amd.sets import AA, NT


@functools.lru_cache(maxsize=None)
def dense_set():
    """1 800 nucleotide sequences of 7 .. 9 residues: with ignore_genes three groups of 613 / 577 / 610, three query
    workgroups each -- the smallest shape at which the triangle across workgroups, segments and lengths can go wrong"""
    return synth.tiny_set(1800, 41, alphabet_size=4, letters=4, min_len=7, max_len=9)


DENSE_GROUPS = {7: 613, 8: 577, 9: 610}


def joined(s1, s2):
    """the sequences of s1, then those of s2, as one set: the two share their gene and repertoire numbering"""
    assert s1.alphabet == s2.alphabet and s1.n_repertoires == s2.n_repertoires
    off = np.concatenate([s1.offsets, s2.offsets[1:] + s1.offsets[-1]])
    cat = lambda name: np.concatenate([getattr(s1, name), getattr(s2, name)])
    return RepertoireSet(cat("residues"), off, cat("v_gene"), cat("j_gene"), cat("repertoire"), cat("count"),
                         list(s1.repertoire_ids), s1.v_names, s1.j_names, s1.alphabet)


@functools.lru_cache(maxsize=None)
def edge_set(nucleotides):
    """both hand-built sets at the edges of the column words (tests/_edit.py edge_sets) as one"""
    s1, s2, _, _ = _edit.edge_sets(nucleotides)
    return joined(s1, s2)


CHAIN_LABEL = [0] * 10 + [10]


@functools.lru_cache(maxsize=None)
def chain_set():
    """a random 30-mer and its prefixes of 29 .. 21 residues -- ten groups of one sequence each, a chain at d = 1 --
    in shuffled order, so that the smallest number is not in the shortest group, and behind them one unrelated 25-mer"""
    rng = np.random.default_rng(2300)
    base = rng.integers(0, 20, size=30, dtype=np.uint8)
    lens = rng.permutation(np.arange(21, 31)).tolist()
    assert lens[0] != 21
    rows = [base[:n] for n in lens] + [(base[:25] + 1 + rng.integers(0, 19, size=25, dtype=np.uint8)) % 20]
    off = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    n = len(rows)
    return RepertoireSet(np.concatenate(rows).astype(np.uint8), off, np.zeros(n, dtype=np.uint32),
                         np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32),
                         np.arange(1, n + 1, dtype=np.uint64), ["R1"], ["V0"], ["J0"], AA)


# name: (the set, nucleotides, n_v_genes, n_j_genes)
SETS = {
    "nt": (lambda: _edit.nt_sets()[0], True, 2, 2),
    "aa": (lambda: _edit.aa_sets()[0], False, 2, 2),
    "min0": (lambda: _edit.min0_sets()[0], False, 2, 2),
    "dense": (dense_set, True, 2, 2),
    "edge_aa": (lambda: edge_set(False), False, 1, 1),
    "edge_nt": (lambda: edge_set(True), True, 1, 1),
    "chain": (chain_set, False, 1, 1),
}

# (input, d, ignore_genes): (clusters, the largest cluster), computed on the CPU
FIGURES = {
    ("nt", 0, False): (276, 4), ("nt", 1, False): (147, 40), ("nt", 2, False): (33, 75), ("nt", 3, False): (4, 86),
    ("nt", 0, True): (239, 8), ("nt", 1, True): (79, 195), ("nt", 2, True): (2, 299), ("nt", 3, True): (1, 300),
    ("aa", 0, False): (262, 5), ("aa", 1, False): (168, 36), ("aa", 2, False): (53, 75), ("aa", 3, False): (11, 83),
    ("aa", 0, True): (231, 15), ("aa", 1, True): (113, 165), ("aa", 2, True): (16, 283), ("aa", 3, True): (1, 300),
    ("min0", 0, False): (98, 16), ("min0", 1, False): (4, 85), ("min0", 2, False): (4, 85),
    ("min0", 0, True): (31, 57), ("min0", 1, True): (1, 300),
    ("dense", 1, True): (1303, 42), ("dense", 2, True): (27, 1773), ("dense", 2, False): (418, 340),
}
KEYS = list(FIGURES)
# the six partitions at d = 1 that are the indel model's (tests/_cluster.py model with indels)
D1_KEYS = [(name, 1, g) for name in ("nt", "aa", "min0") for g in (False, True)]
# the edge sets and the chain: no figures pinned, conditions asserted by the CPU test
MORE_KEYS = [("edge_aa", _edit.EDGE_D, False), ("edge_nt", _edit.EDGE_D, False), ("chain", 1, False), ("chain", 0, False)]


def ids_of(keys):
    return ["%s-d%d%s" % (k[0], k[1], "-g" if k[2] else "") for k in keys]


def set_of(name):
    return SETS[name][0]()


def kw_of(name, ignore_genes):
    """the fields of Options that describe the input"""
    _, nucleotides, n_v, n_j = SETS[name]
    return dict(n_v_genes=n_v, n_j_genes=n_j, nucleotides=nucleotides, ignore_genes=ignore_genes)


@functools.lru_cache(maxsize=None)
def want(name, d, ignore_genes):
    """(label, size, clusters) of the input by the yardstick, read-only"""
    s = set_of(name)
    rows, hits, _ = _edit.brute_csr(s, s, d, ignore_genes)
    label = _cluster.labels_of_pairs(s.n, _edit.queries_of(rows), hits)
    size = _cluster.sizes_of_labels(label)
    label.setflags(write=False)
    size.setflags(write=False)
    return label, size, int((label == np.arange(s.n)).sum())


def figures_of(label, size):
    """(clusters, largest) of a partition"""
    return int((label == np.arange(len(label))).sum()), int(size.max())


def indel_model(name, ignore_genes):
    """the partition of the hashed path's model at d = 1 with indels"""
    return _cluster.model(set_of(name), Options(differences=1, indels=True, **kw_of(name, ignore_genes)))


def refines(fine, coarse):
    """every label class of `fine` lies inside one label class of `coarse`"""
    fine, coarse = np.asarray(fine).astype(np.int64), np.asarray(coarse).astype(np.int64)
    return bool(np.array_equal(coarse, coarse[fine]))
