"""Helpers of the tests of cmpr_hamming_cluster / cmpr_hamming_cluster_table (not a test module): the inputs and
figures the CPU and GPU tests share, the model's partition of each (tests/_cluster.py model, computed once), and the
reference's own `-c` runs at d >= 3 recorded in tests/golden/hamming_cluster.json.  Nothing here calls the library
under test."""

import functools
import json
import os

import numpy as np

import _cluster
import _hamming

HERE = os.path.dirname(os.path.abspath(__file__))

# which set of the pair tests/_hamming.py builds is clustered
WHICH = {"aa": 0, "nt": 0, "empty": 0, "dense": 1}

# (input, d, ignore_genes): (clusters, the largest cluster, clusters of one sequence)
FIGURES = {
    ("aa", 0, False): (291, 2, 282), ("aa", 0, True): (265, 5, 239),
    ("aa", 3, False): (91, 16, 57), ("aa", 3, True): (20, 47, 6),
    ("aa", 4, False): (47, 16, 12), ("aa", 4, True): (7, 47, 0),
    ("aa", 6, False): (28, 16, 0), ("aa", 6, True): (7, 47, 0),
    ("nt", 3, False): (226, 13, 200), ("nt", 3, True): (159, 41, 141),
    ("nt", 4, False): (157, 13, 128), ("nt", 4, True): (98, 44, 85),
    ("empty", 3, False): (16, 18, 0), ("empty", 3, True): (4, 63, 0),
    ("dense", 0, True): (8405, 4, 7837),
    ("dense", 1, False): (5350, 28, 3850), ("dense", 1, True): (342, 8578, 280),
    ("dense", 2, False): (6, 2284, 2), ("dense", 2, True): (1, 9001, 0),
    ("dense", 3, True): (1, 9001, 0),
}
KEYS = list(FIGURES)
IDS = ["%s-d%d%s" % (k[0], k[1], "-g" if k[2] else "") for k in KEYS]


def set_of(name):
    return _hamming.sets_of(name)[WHICH[name]]


@functools.lru_cache(maxsize=None)
def model(name, d, ignore_genes):
    """(label, size, clusters) of the input by tests/_cluster.py model, read-only"""
    label, size, clusters = _cluster.model(set_of(name), _hamming.options_of(name, ignore_genes, differences=d))
    label.setflags(write=False)
    size.setflags(write=False)
    return label, size, clusters


def figures_of(label, size):
    """(clusters, largest, singletons) of a partition"""
    roots = np.flatnonzero(label == np.arange(len(label)))
    return len(roots), int(size.max()), int((size[roots] == 1).sum())


def golden_cases():
    """the reference's `-c` runs at d >= 3, in the shape of the manifest's entries"""
    with open(os.path.join(HERE, "golden", "hamming_cluster.json")) as fh:
        return json.load(fh)


# name of the golden case: (clusters, the largest cluster)
GOLDEN_FIGURES = {"hc_clus_aa_d3": (24, 74), "hc_clus_aa_d4_g": (6, 269), "hc_clus_nt_d3": (356, 40),
                  "hc_clus_nt_d5_g": (6, 219), "hc_tiny_aa_a_d3": (23, 14)}
