"""The -x table as CSR (cmpr_existence_csr): the yardstick -- the nonzero cells of the oracle's dense -x matrix as
(row_start, repertoire, value) -- and the inputs the CPU and GPU tests share (test infrastructure).  Every input
here has counts of at most 9, so no cell sums to zero or wraps: "nonzero" and "has a match" coincide."""

import dataclasses
import functools

import numpy as np

import _neighbors
import _oracle
from compairr_amd import Options, synth


def csr_of_dense(m):
    """(row_start uint64[rows + 1], repertoire uint32[C], value uint64[C]) of the nonzero cells of a matrix"""
    m = np.asarray(m)
    rows, cols = np.nonzero(m)                        # (row-major: rows ascending, columns ascending inside a row)
    row_start = np.zeros(m.shape[0] + 1, dtype=np.uint64)
    np.cumsum(np.bincount(rows, minlength=m.shape[0]), out=row_start[1:])
    return row_start, cols.astype(np.uint32), m[rows, cols].astype(np.uint64)


def assert_is_cell_csr(row_start, repertoire, value, n1, n_rep):
    assert row_start.dtype == np.uint64 and repertoire.dtype == np.uint32 and value.dtype == np.uint64
    assert len(row_start) == n1 + 1 and row_start[0] == 0
    assert row_start[-1] == len(repertoire) == len(value)
    assert (np.diff(row_start.astype(np.int64)) >= 0).all()
    assert len(repertoire) == 0 or int(repertoire.max()) < n_rep
    inner = np.ones(len(repertoire), dtype=bool)
    inner[row_start[:-1][np.diff(row_start.astype(np.int64)) > 0].astype(np.int64)] = False   # a row's first cell
    assert (np.diff(repertoire.astype(np.int64))[inner[1:]] > 0).all(), "a row is not strictly increasing"
    assert (value != 0).all(), "a listed cell is zero"


def shape_of(row_start):
    """(cells, most cells in a row, rows with more than 64 cells, empty rows)"""
    deg = np.diff(row_start.astype(np.int64))
    return int(row_start[-1]), int(deg.max()) if len(deg) else 0, int((deg > 64).sum()), int((deg == 0).sum())


def oracle_cells(set1, set2, opt):
    """the yardstick: the oracle's dense -x matrix under `opt`, as the integers the C ABI holds"""
    o = dataclasses.replace(opt, existence=True)
    return _oracle.integer_cells(_oracle.overlap(set1, set2, o)[0], o)


def oracle_cell_csr(set1, set2, opt):
    got = csr_of_dense(oracle_cells(set1, set2, opt))
    for a in got:
        a.setflags(write=False)
    return got


# ---- 1. small sets: the sequences of _neighbors.SMALL (edge counts carry over), other repertoire numbers ----

@functools.lru_cache(maxsize=None)
def tiny(n, seed, n_rep, nucleotides=False):
    return synth.tiny_set(n, seed, alphabet_size=4 if nucleotides else 20, n_repertoires=n_rep, **_neighbors.TINY)


# name: (set 1, set 2, R2, options, (edges, cells, most cells in a row, rows with > 64 cells, empty rows))
NT_KW = dict(differences=1, indels=True, ignore_genes=True, nucleotides=True)
SMALL = {
    "self_d1_r1": ((3000, 5), (3000, 5), 1, dict(differences=1), (94_306, 3_000, 1, 0, 0)),
    "self_d1_r3": ((3000, 5), (3000, 5), 3, dict(differences=1), (94_524, 7_694, 3, 0, 0)),
    "self_d0_r200": ((3000, 5), (3000, 5), 200, dict(differences=0), (25_932, 24_285, 46, 0, 0)),
    "self_d1_r200": ((3000, 5), (3000, 5), 200, dict(differences=1), (94_524, 78_773, 90, 429, 0)),
    "self_d1i_r200": ((3000, 5), (3000, 5), 200, dict(differences=1, indels=True), (184_640, 135_960, 121, 929, 0)),
    "self_d2_r200": ((3000, 5), (3000, 5), 200, dict(differences=2), (160_148, 130_576, 90, 1_032, 0)),
    "other_d1_r200": ((3000, 5), (2500, 6), 200, dict(differences=1), (36_819, 30_014, 72, 429, 2_571)),
    "nt_d1ig_r200": ((3000, 5), (2500, 6), 200, NT_KW, (411_759, 185_300, 193, 1_164, 1_210)),
}
SCORES_CASE = "self_d1_r200"
OTHER_SCORES = [dict(score="min"), dict(score="max"), dict(score="mean"), dict(ignore_counts=True)]


def small_sets(name):
    a, b, n_rep, kw, _ = SMALL[name]
    nt = bool(kw.get("nucleotides"))
    s1 = tiny(*a, n_rep, nucleotides=nt)
    return s1, (s1 if a == b else tiny(*b, n_rep, nucleotides=nt))


def small_options(name, **more):
    return _neighbors.tiny_options(**dict(SMALL[name][3], **more))


@functools.lru_cache(maxsize=None)
def _small_want(name, more):
    s1, s2 = small_sets(name)
    return oracle_cell_csr(s1, s2, small_options(name, **dict(more)))


def small_want(name, **more):
    return _small_want(name, tuple(sorted(more.items())))


@functools.lru_cache(maxsize=None)
def small_edges(name):
    s1, s2 = small_sets(name)
    return len(_oracle.pairs(s1, s2, small_options(name)))


# ---- 2. the long row ----

HUB_REPS = 5000
# per (repertoires of set 2, d): the hits of the three non-empty rows and the cells they collapse to
HUB_ROWS = {
    (3, 2): ([43_625, 5_720, 932], [3, 3, 3]),
    (3, 1): ([305, 305, 39], [3, 3, 3]),
    (HUB_REPS, 2): ([43_625, 5_720, 932], [5_000, 3_404, 851]),
    (HUB_REPS, 1): ([305, 305, 39], [291, 297, 39]),
}


@functools.lru_cache(maxsize=None)
def hub_sets(n_rep=3):
    """_neighbors.hub_sets() as it is (3 repertoires, every count 1), or with its set 2 renumbered into HUB_REPS
    repertoires and both sets given counts of 1 .. 9"""
    s1, s2 = _neighbors.hub_sets()
    if n_rep == 3:
        return s1, s2
    assert n_rep == HUB_REPS
    rng = np.random.default_rng(163)
    rep = rng.integers(0, HUB_REPS, size=s2.n, dtype=np.uint32)
    rep[:HUB_REPS] = np.arange(HUB_REPS)
    cnt2 = rng.integers(1, 10, size=s2.n).astype(np.uint64)
    cnt1 = rng.integers(1, 10, size=s1.n).astype(np.uint64)
    return (dataclasses.replace(s1, count=cnt1),
            dataclasses.replace(s2, repertoire=rep, count=cnt2,
                                repertoire_ids=["H%d" % (k + 1) for k in range(HUB_REPS)]))


def hub_options(d, **more):
    return Options(differences=d, n_v_genes=1, n_j_genes=1, **more)


@functools.lru_cache(maxsize=None)
def hub_want(n_rep, d):
    s1, s2 = hub_sets(n_rep)
    return oracle_cell_csr(s1, s2, hub_options(d))


# ---- 3. rows of exactly the lengths at which the path changes ----

EDGE_REPS = [1, 200]


@functools.lru_cache(maxsize=None)
def edge_sets(n_rep):
    """_neighbors.edge_rows() with its set 2 renumbered into n_rep repertoires (1: one run per row, across every
    wave and round of the row of 8192 hits) and both sets given counts of 1 .. 9"""
    s1, s2 = _neighbors.edge_rows()
    rng = np.random.default_rng(173)
    rep = rng.integers(0, n_rep, size=s2.n, dtype=np.uint32)
    rep[:n_rep] = np.arange(n_rep)
    cnt2 = rng.integers(1, 10, size=s2.n).astype(np.uint64)
    cnt1 = rng.integers(1, 10, size=s1.n).astype(np.uint64)
    return (dataclasses.replace(s1, count=cnt1),
            dataclasses.replace(s2, repertoire=rep, count=cnt2,
                                repertoire_ids=["H%d" % (k + 1) for k in range(n_rep)]))


@functools.lru_cache(maxsize=None)
def edge_want(n_rep):
    return oracle_cell_csr(*edge_sets(n_rep), _neighbors.edge_options())


# ---- the yardstick a second way: the neighbour lists reduced by repertoire in numpy ----

def cells_of_neighbors(set1, set2, opt):
    """dense uint64 (n1, R2): every pair of _neighbors.oracle_csr scored as score_match does and added to the cell
    (its query, the repertoire of its hit)"""
    row_start, hits = _neighbors.oracle_csr(set1, set2, opt)
    q = np.repeat(np.arange(set1.n), np.diff(row_start.astype(np.int64)))
    f, g = set1.count[q], set2.count[hits]
    if opt.ignore_counts:
        sc = np.ones(len(hits), dtype=np.uint64)
    else:
        sc = {"product": f * g, "mh": f * g, "min": np.minimum(f, g), "jaccard": np.minimum(f, g),
              "max": np.maximum(f, g), "mean": f + g}[opt.score.lower()]
    m = np.zeros((set1.n, set2.n_repertoires), dtype=np.uint64)
    np.add.at(m, (q, set2.repertoire[hits].astype(np.int64)), sc)
    return m
