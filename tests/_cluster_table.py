"""Helpers of the cluster-table tests (not a test module): the yardstick in plain numpy, what the reference's
--cluster printed for the recorded `-c` cases row by row, and the crafted set of hypercubes and rook's-graph
groups whose partition is known by construction."""

import os

import numpy as np

import _cluster
from compairr_amd import RepertoireSet
from compairr_amd.sets import AA


def table_of(label, count):
    """(cluster_of uint32[n], cluster_start uint64[K + 1], members uint32[n], cluster_count uint64[K]) of the
    partition `label` (label[i] = the smallest member of i's cluster): the clusters numbered by (size descending,
    root ascending), the members of each in increasing order, the counts summed per cluster (uint64, wrapping)."""
    label = np.asarray(label).astype(np.int64)
    n = len(label)
    size = np.bincount(label, minlength=n)
    roots = np.flatnonzero(label == np.arange(n))
    order = roots[np.lexsort((roots, -size[roots]))]
    number = np.full(n, -1, dtype=np.int64)
    number[order] = np.arange(len(order))
    cluster_of = number[label]
    members = np.argsort(cluster_of, kind="stable")
    cluster_start = np.zeros(len(order) + 1, dtype=np.uint64)
    np.cumsum(size[order], out=cluster_start[1:])
    cluster_count = np.zeros(len(order), dtype=np.uint64)
    np.add.at(cluster_count, cluster_of, np.asarray(count).astype(np.uint64))
    return cluster_of.astype(np.uint32), cluster_start, members.astype(np.uint32), cluster_count


TABLE_NAMES = ("cluster_of", "cluster_start", "members", "count")
TABLE_DTYPES = (np.uint32, np.uint64, np.uint32, np.uint64)


def assert_partition(got, label):
    """(label, size, n_clusters) as a cluster call gives them against the partition `label`"""
    assert len(got) == 3 and got[0].dtype == np.uint32 and got[1].dtype == np.uint32
    assert np.array_equal(got[0], label)
    assert np.array_equal(got[1], _cluster.sizes_of_labels(label))
    assert got[2] == int((label == np.arange(len(label))).sum())


def assert_table(got, want):
    """the four arrays of a cluster-table call against table_of()"""
    for name, dtype, g, w in zip(TABLE_NAMES, TABLE_DTYPES, got, want):
        assert g.dtype == dtype, name
        assert g.shape == w.shape and np.array_equal(g, w), name


def printed(case, keys):
    """(cluster_no int64[n], cluster_size int64[n], rows): the reference's print-out of `case` per INPUT row, and
    the input numbers of its output rows in the order printed"""
    f = _cluster.flags_of(case)
    where = {k: i for i, k in enumerate(keys)}
    header, rows = _cluster._rows(os.path.join(_cluster.EXPECTED, case["name"] + ".tsv"))
    col = {name: k for k, name in enumerate(header)}
    seq_col = col[_cluster._sequence_column(f["nucleotides"], f["cdr3"])]
    no = np.zeros(len(keys), dtype=np.int64)
    size = np.zeros(len(keys), dtype=np.int64)
    order = []
    for r in rows:
        i = where[(r[col["repertoire_id"]], r[col["sequence_id"]], _cluster._text(r[seq_col], f["nucleotides"]))]
        no[i] = int(r[col["cluster_no"]])
        size[i] = int(r[col["cluster_size"]])
        order.append(i)
    assert sorted(order) == list(range(len(keys)))
    return no, size, order


# ---- the crafted set: d = 1, one V and one J gene, no indels ----

CUBE_LETTERS = (AA.index("W"), AA.index("C"))
GROUP_LETTERS = np.array([k for k in range(len(AA)) if k not in CUBE_LETTERS], dtype=np.uint8)   # the other 18
GROUP_LENGTH = 12


def crafted(cube_lengths, groups, seed, contiguous):
    """(set, label): hypercubes over two amino acids, one per length of `cube_lengths` (2^L sequences, each a single
    cluster; different lengths never link without indels), and groups at length 12 over the other 18 letters,
    `groups` = [(members, how many groups)]: positions 0-8 are the group number in base 18, position 9 their sum
    mod 18 -- two groups differ in at least two positions and never link --, positions 10 and 11 enumerate the
    members row-major: a rook's graph, connected for every size up to 324.  contiguous: each cluster's members
    lie side by side; otherwise the set is in a random order seeded with `seed`.  The counts are drawn up to 2^40.
    label[i] = the smallest number of the constructed cluster of i."""
    assert GROUP_LENGTH not in cube_lengths and len(set(cube_lengths)) == len(cube_lengths)
    rows, cluster = [], []
    for L in cube_lengths:
        bits = (np.arange(1 << L)[:, None] >> np.arange(L)[None, :]) & 1
        rows.append(np.where(bits == 1, CUBE_LETTERS[0], CUBE_LETTERS[1]).astype(np.uint8))
        cluster.append(np.full(1 << L, len(cluster)))
    sizes = np.array([m for m, how_many in groups for _ in range(how_many)], dtype=np.int64)
    assert len(sizes) < 18 ** 9 and sizes.max(initial=1) <= 324 and sizes.min(initial=1) >= 1
    group = np.repeat(np.arange(len(sizes)), sizes)
    member = np.arange(len(group)) - np.repeat(np.cumsum(sizes) - sizes, sizes)
    digits = (group[:, None] // 18 ** np.arange(9)[None, :]) % 18
    code = np.concatenate([digits, digits.sum(axis=1, keepdims=True) % 18, (member // 18)[:, None],
                           (member % 18)[:, None]], axis=1)
    rows.append(GROUP_LETTERS[code])
    cluster.append(len(cluster) + group)
    cluster = np.concatenate(cluster)
    lengths = np.concatenate([np.full(len(r), r.shape[1]) for r in rows])
    n = len(cluster)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lengths, out=offsets[1:])
    rng = np.random.default_rng(seed)
    zeros = np.zeros(n, dtype=np.uint32)
    s = RepertoireSet(np.concatenate([r.reshape(-1) for r in rows]), offsets, zeros, zeros, zeros,
                      rng.integers(1, 1 << 40, n).astype(np.uint64), ["T1"], ["V0"], ["J0"], AA)
    if not contiguous:
        perm = rng.permutation(n)
        s, cluster = s.subset(perm), cluster[perm]
    first = np.full(int(cluster.max()) + 1, n, dtype=np.int64)
    np.minimum.at(first, cluster, np.arange(n))
    return s, first[cluster].astype(np.uint32)
