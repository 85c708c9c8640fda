"""Edge distances of the neighbour CSR (cmpr_neighbors_distance): a numpy model of the reference's --distance column
(overlap.cc:491-502) -- the Hamming distance of two sequences of one length, 1 otherwise -- and the inputs the CPU
and GPU tests of the call add to those of tests/_neighbors.py (test infrastructure)."""

import functools

import numpy as np

import _neighbors
from compairr_amd.sets import AA


def residues_distance(a, b):
    """the model for one pair: two arrays (or strings) of residues"""
    if len(a) != len(b):
        return 1
    return int(sum(1 for x, y in zip(a, b) if x != y))


def edge_distances(set1, set2, row_start, hits):
    """uint8[E]: for edge k of the CSR -- query i with row_start[i] <= k < row_start[i + 1], hit hits[k] -- the
    number of positions at which the two sequences differ when they have one length, 1 otherwise"""
    row_start = np.asarray(row_start).astype(np.int64)
    hits = np.asarray(hits).astype(np.int64)
    query = np.repeat(np.arange(set1.n, dtype=np.int64), np.diff(row_start))
    assert len(query) == len(hits)
    len1, len2 = set1.lengths[query], set2.lengths[hits]
    off1, off2 = set1.offsets.astype(np.int64)[query], set2.offsets.astype(np.int64)[hits]
    out = np.ones(len(hits), dtype=np.uint8)
    same = len1 == len2
    for L in np.unique(len1[same]):
        sel = np.nonzero(same & (len1 == L))[0]
        span = np.arange(int(L), dtype=np.int64)
        a = set1.residues[off1[sel, None] + span]
        b = set2.residues[off2[sel, None] + span]
        out[sel] = (a != b).sum(axis=1).astype(np.uint8)
    out.setflags(write=False)
    return out


def histogram(dist):
    """[d0, d1, d2] edge counts"""
    return np.bincount(dist, minlength=3).tolist()


def mixed_rows(row_start, dist):
    """rows holding more than one distance value, as (of at most 8 hits, of 9..64, above 64)"""
    row_start = row_start.astype(np.int64)
    deg = np.diff(row_start)
    rows = np.nonzero(deg > 0)[0]
    lo = np.minimum.reduceat(dist, row_start[rows])
    hi = np.maximum.reduceat(dist, row_start[rows])
    d = deg[rows][lo != hi]
    return int((d <= 8).sum()), int(((d > 8) & (d <= 64)).sum()), int((d > 64).sum())


# ---- the small inputs: those of _neighbors.SMALL and one of nucleotides at d = 2 ----

# name: ((set 1), (set 2), options) as in _neighbors.SMALL
EXTRA = {
    "nt_d2g": ((1000, 5), (800, 6), dict(differences=2, ignore_genes=True, nucleotides=True)),
}
# [d0, d1, d2] edge counts, measured with the oracle and the model (tests/test_neighbors_distance_cpu.py pins them)
FIGURES = {
    "self_d0": [25_932, 0, 0],
    "self_d1": [25_932, 68_592, 0],
    "self_d1i": [25_932, 158_708, 0],
    "self_d2": [25_932, 68_592, 65_624],
    "other_d1": [0, 36_819, 0],
    "nt_d1ig": [45_081, 366_678, 0],
    "nt_d2g": [8_050, 24_440, 24_527],
}


def small_options(name):
    return dict(_neighbors.SMALL[name][2] if name in _neighbors.SMALL else EXTRA[name][2])


def small_sets(name):
    if name in _neighbors.SMALL:
        return _neighbors.small_sets(name)
    a, b, kw = EXTRA[name]
    nt = bool(kw.get("nucleotides"))
    return _neighbors.tiny(*a, nucleotides=nt), _neighbors.tiny(*b, nucleotides=nt)


@functools.lru_cache(maxsize=None)
def small_want(name):
    """(row_start, hits, distance) the GPU has to give: the oracle's CSR and the model's distances"""
    s1, s2 = small_sets(name)
    if name in _neighbors.SMALL:
        row_start, hits = _neighbors.small_want(name)
    else:
        row_start, hits = _neighbors.oracle_csr(s1, s2, _neighbors.tiny_options(**small_options(name)))
    return row_start, hits, edge_distances(s1, s2, row_start, hits)


@functools.lru_cache(maxsize=None)
def want_of(sets, opt_items):
    """the same for any pair of sets: sets = a function without arguments, opt_items = sorted option items"""
    from compairr_amd import Options
    s1, s2 = sets()
    row_start, hits = _neighbors.oracle_csr(s1, s2, Options(**dict(opt_items)))
    return row_start, hits, edge_distances(s1, s2, row_start, hits)


def hub_want(d):
    return want_of(_neighbors.hub_sets, (("differences", d), ("n_j_genes", 1), ("n_v_genes", 1)))


def edge_want():
    return want_of(_neighbors.edge_rows, (("differences", 2), ("n_j_genes", 1), ("n_v_genes", 1)))


# ---- sequences longer than a query record (36 residues) and a table record (32) hold ----

LONG_L = 40


@functools.lru_cache(maxsize=None)
def long_sets():
    """set 2: a seeded 3 000 members of the radius-2 ball of a 40-mer hub, and the hub; set 1: the hub, a sequence
    at distance 1 and one at distance 2 of it, the changes behind position 36.  One V gene, one J gene."""
    rng = np.random.default_rng(40)
    hub = rng.integers(0, 20, size=LONG_L, dtype=np.uint8)
    ball = _neighbors.ball_of(hub)
    rows2 = np.concatenate([ball[1:][rng.permutation(len(ball) - 1)[:3_000]], hub[None, :]])
    rows2 = rows2[rng.permutation(len(rows2))]
    one, two = hub.copy(), hub.copy()
    one[37] = (hub[37] + 1) % 20
    two[5], two[38] = (hub[5] + 3) % 20, (hub[38] + 7) % 20
    return _neighbors._set_of_rows(np.stack([hub, one, two]), 401, 3), _neighbors._set_of_rows(rows2, 402, 3)


def long_want():
    return want_of(long_sets, (("differences", 2), ("n_j_genes", 1), ("n_v_genes", 1)))


assert len(AA) == 20
