"""The nearest neighbour per sequence at any distance (cmpr_hamming_nearest): a numpy brute force of the definition --
per length all distances, the eligibility mask, row minimum, argmin and the count of the minimum --, the same three
arrays from a pair list (the oracle's, at some d), and the inputs and figures the CPU and GPU tests share (test
infrastructure).  Nothing here calls the library under test."""

import functools

import numpy as np

import _hamming
import _neighbors

NONE32, NONE16 = 0xFFFFFFFF, 0xFFFF


# ---- (a) the brute force ----

def eligible(set1, set2, i1, i2, dist, ignore_genes, floor, one_set, other_rep):
    """bool[len(i1), len(i2)]: which of the sequences i2 of set2 are candidates of the sequences i1 of set1, all of
    one length, `dist` apart"""
    ok = dist >= floor
    if not ignore_genes:
        ok &= set1.v_gene[i1, None] == set2.v_gene[None, i2]
        ok &= set1.j_gene[i1, None] == set2.j_gene[None, i2]
    if one_set:
        ok &= i1[:, None] != i2[None, :]
    if other_rep:
        ok &= set1.repertoire[i1, None] != set2.repertoire[None, i2]
    return ok


def brute(set1, set2, ignore_genes=False, floor=0, other_rep=False):
    """(nearest uint32[n1], distance uint16[n1], ties uint32[n1]); `set2 is set1` is one-set mode"""
    one_set = set2 is set1
    assert one_set or not other_rep
    n1 = set1.n
    nearest = np.full(n1, NONE32, dtype=np.uint32)
    distance = np.full(n1, NONE16, dtype=np.uint16)
    ties = np.zeros(n1, dtype=np.uint32)
    len1, len2 = set1.lengths, set2.lengths
    off1, off2 = set1.offsets.astype(np.int64), set2.offsets.astype(np.int64)
    far = np.iinfo(np.int64).max
    for L in np.intersect1d(np.unique(len1), np.unique(len2)):
        L = int(L)
        i1, i2 = np.nonzero(len1 == L)[0], np.nonzero(len2 == L)[0]
        span = np.arange(L, dtype=np.int64)
        a = set1.residues[off1[i1, None] + span].reshape(len(i1), L)
        b = set2.residues[off2[i2, None] + span].reshape(len(i2), L)
        step = max(1, (1 << 24) // max(1, len(i2) * max(L, 1)))
        for lo in range(0, len(i1), step):
            rows = i1[lo:lo + step]
            dist = np.count_nonzero(a[lo:lo + step, None, :] != b[None, :, :], axis=2).astype(np.int64)
            dist[~eligible(set1, set2, rows, i2, dist, ignore_genes, floor, one_set, other_rep)] = far
            best = dist.min(axis=1)
            found = best != far
            nearest[rows[found]] = i2[dist.argmin(axis=1)[found]]      # (i2 increases: the first is the smallest)
            distance[rows[found]] = best[found]
            ties[rows[found]] = (dist == best[:, None]).sum(axis=1)[found]
    return nearest, distance, ties


# ---- (b) from a pair list at d ----

def from_pairs(set1, set2, row_start, hits, dist, floor=0, other_rep=False):
    """the three arrays from a CSR pair list with distances (rows increasing in the hit, as the oracle's): a row is
    filtered by the floor, the self pair (one-set mode) and the repertoire, then minimum, first hit at it, count.  A
    sequence whose filtered row is empty is "none" HERE: its neighbour, if any, lies above the list's d"""
    one_set = set2 is set1
    n1 = set1.n
    row_start = np.asarray(row_start).astype(np.int64)
    hits = np.asarray(hits).astype(np.int64)
    dist = np.asarray(dist).astype(np.int64)
    query = np.repeat(np.arange(n1, dtype=np.int64), np.diff(row_start))
    ok = dist >= floor
    if one_set:
        ok &= hits != query
    if other_rep:
        ok &= set1.repertoire[query] != set2.repertoire[hits]
    query, hits, dist = query[ok], hits[ok], dist[ok]
    nearest = np.full(n1, NONE32, dtype=np.uint32)
    distance = np.full(n1, NONE16, dtype=np.uint16)
    ties = np.zeros(n1, dtype=np.uint32)
    order = np.lexsort((hits, dist, query))                          # per query: by distance, then by number
    query, hits, dist = query[order], hits[order], dist[order]
    first = np.nonzero(np.r_[True, query[1:] != query[:-1]])[0] if len(query) else np.zeros(0, dtype=np.int64)
    nearest[query[first]] = hits[first]
    distance[query[first]] = dist[first]
    best = np.full(n1, -1, dtype=np.int64)
    best[query[first]] = dist[first]
    ties[:] = np.bincount(query[dist == best[query]], minlength=n1)
    return nearest, distance, ties


def oracle_nearest(name, d, ignore_genes, floor=0, other_rep=False):
    """(b) on an input of _hamming: the oracle's pair list at d (_hamming.oracle_want), filtered and reduced"""
    s1, s2 = _hamming.sets_of(name)
    row_start, hits, dist = _hamming.want(name, d, ignore_genes)
    return from_pairs(s1, s2, row_start, hits, dist, floor, other_rep)


def assert_agrees_up_to(full, partial, d):
    """`partial` (from a pair list at d) against `full` (the brute force): the same three figures for every sequence
    whose nearest distance is at most d, and an empty row exactly where the distance is above d or "none" """
    near = (full[2] > 0) & (full[1].astype(np.int64) <= d)
    for f, p in zip(full, partial):
        assert np.array_equal(f[near], p[near])
    assert np.array_equal(partial[2] == 0, ~near)
    assert (partial[0][~near] == NONE32).all() and (partial[1][~near] == NONE16).all()


# ---- the figures of the issue ----

def figures(got):
    """(none, histogram of the nearest distances of those who have one, sum of ties, largest ties)"""
    nearest, distance, ties = got
    none = ties == 0
    assert np.array_equal(none, nearest == NONE32) and (distance[none] == NONE16).all()
    return (int(none.sum()), np.bincount(distance[~none].astype(np.int64)).tolist(), int(ties.sum()),
            int(ties.max()) if len(ties) else 0)


# (input, ignore_genes, floor, other_rep): (none, histogram, sum of ties, largest ties or None where not recorded)
FIGURES = {
    ("aa", False, 0, False): (0, [0, 4, 40, 60, 50, 52, 55, 29, 8, 2], 1050, 14),
    ("aa", False, 1, False): (0, [0, 4, 40, 60, 50, 52, 55, 29, 8, 2], 1050, 14),
    ("aa", True, 0, False): (0, [0, 13, 36, 68, 53, 57, 42, 24, 5, 2], 3182, 42),
    ("aa", True, 1, False): (0, [0, 13, 36, 68, 53, 57, 42, 24, 5, 2], 3182, 42),
    ("nt", False, 0, False): (0, [0, 4, 30, 66, 72, 45, 43, 29, 10, 1], 540, 7),
    ("nt", False, 1, False): (0, [0, 4, 30, 66, 72, 45, 43, 29, 10, 1], 540, 7),
    ("nt", True, 0, False): (0, [2, 25, 70, 62, 56, 38, 40, 7], 642, 12),
    ("nt", True, 1, False): (0, [0, 25, 72, 62, 56, 38, 40, 7], 642, 12),
    ("dense", False, 0, False): (0, [5, 32, 33], 338, 15),
    ("dense", False, 1, False): (0, [0, 35, 35], 356, 15),
    ("dense", True, 0, False): (0, [14, 53, 3], 299, 41),
    ("dense", True, 1, False): (0, [0, 67, 3], 339, 41),
    ("empty", False, 0, False): (0, [181, 19], 1156, 15),
    ("empty", False, 1, False): (39, [0, 161], 1008, 10),
    ("empty", True, 0, False): (0, [200], 4272, 38),
    ("empty", True, 1, False): (39, [0, 161], 3992, 34),
    ("nt", False, 0, True): (0, [0, 4, 26, 49, 71, 57, 43, 28, 16, 4, 2], 487, None),
    ("nt", False, 1, True): (0, [0, 4, 26, 49, 71, 57, 43, 28, 16, 4, 2], 487, None),
    ("nt", True, 0, True): (0, [2, 15, 60, 57, 65, 40, 46, 14, 1], 636, None),
    ("nt", True, 1, True): (0, [0, 15, 62, 57, 65, 40, 46, 14, 1], 636, None),
    ("empty", False, 0, True): (0, [176, 24], 754, None),
    ("empty", False, 1, True): (39, [0, 159, 2], 715, None),
    ("empty", True, 0, True): (0, [200], 2782, None),
    ("empty", True, 1, True): (39, [0, 161], 2762, None),
}
CASES = list(FIGURES)
IDS = ["%s%s-floor%d%s" % (k[0], "-g" if k[1] else "", k[2], "-other" if k[3] else "") for k in CASES]
# sequences of `nt` for which the flag changes at least one of the three outputs, by ignore_genes (floor 0)
NT_FLAG_CHANGES = {False: 133, True: 176}
# sequences of edge_sets(nucleotides) set 1 that have no neighbour: the appended ones whose length no base has
EDGE_NONE = {False: 9, True: 10}


@functools.lru_cache(maxsize=None)
def want(name, ignore_genes, floor, other_rep):
    """(a) on an input of _hamming, computed once and read-only"""
    s1, s2 = _hamming.sets_of(name)
    out = brute(s1, s2, ignore_genes, floor, other_rep)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def dense_self():
    """the 9001 sequences of `dense` as ONE set: the self case"""
    s = _hamming.dense_sets()[1]
    return s, s


@functools.lru_cache(maxsize=None)
def want_of(kind, ignore_genes, floor, other_rep):
    """(a) on dense in both directions and on the self case: kind is 'dense', 'swapped' or 'self'"""
    s1, s2 = sets_of(kind)
    out = brute(s1, s2, ignore_genes, floor, other_rep)
    for a in out:
        a.setflags(write=False)
    return out


def sets_of(kind):
    if kind == "swapped":
        return _hamming.dense_sets()[::-1]
    if kind == "self":
        return dense_self()
    return _hamming.sets_of(kind)


def long_set():
    """the 20 000-residue case of test_hamming_gpu.test_a_reference_longer_than_the_staging_buffer: six sequences with
    0 .. 5 substitutions of one base, and one far away"""
    rng = np.random.default_rng(20)
    L = 20_000
    base = rng.integers(0, 20, size=L, dtype=np.uint8)
    rows = [base.copy() for _ in range(6)]
    for k, row in enumerate(rows):
        for p in ([0, L - 1] + [4_095 * 4 + 3, 4_096 * 4, 9_999])[:k]:
            row[p] = (row[p] + 1) % 20
    far = rng.integers(0, 20, size=L, dtype=np.uint8)
    return _neighbors._set_of_rows(np.stack(rows + [far]), 201, 2)


def six():
    """a hand-written case: (set, {(ignore_genes, floor, other_rep): (nearest, distance, ties)}).
         0 AAAA v0 rep0    1 AAAA v0 rep0    2 AAAC v0 rep1    3 AACC v1 rep1    4 CC v0 rep0    5 (empty) v0 rep1"""
    from compairr_amd import RepertoireSet
    from compairr_amd.sets import AA
    rows = [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 1], [1, 1], []]
    off = np.zeros(7, dtype=np.uint64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    s = RepertoireSet(np.array(sum(rows, []), dtype=np.uint8), off, np.array([0, 0, 0, 1, 0, 0], dtype=np.uint32),
                      np.zeros(6, dtype=np.uint32), np.array([0, 0, 1, 1, 0, 1], dtype=np.uint32),
                      np.ones(6, dtype=np.uint64), ["R0", "R1"], ["V0", "V1"], ["J0"], AA)
    N, F = NONE32, NONE16
    table = {
        # genes: {0, 1, 2} are a group, 3 is alone (V1), 4 and 5 are alone by length
        (False, 0, False): ([1, 0, 0, N, N, N], [0, 0, 1, F, F, F], [1, 1, 2, 0, 0, 0]),
        (False, 1, False): ([2, 2, 0, N, N, N], [1, 1, 1, F, F, F], [1, 1, 2, 0, 0, 0]),
        (False, 0, True): ([2, 2, 0, N, N, N], [1, 1, 1, F, F, F], [1, 1, 2, 0, 0, 0]),
        (False, 2, False): ([N, N, N, N, N, N], [F, F, F, F, F, F], [0, 0, 0, 0, 0, 0]),
        # -g: {0, 1, 2, 3} are a group
        (True, 0, False): ([1, 0, 0, 2, N, N], [0, 0, 1, 1, F, F], [1, 1, 3, 1, 0, 0]),
        (True, 1, False): ([2, 2, 0, 2, N, N], [1, 1, 1, 1, F, F], [1, 1, 3, 1, 0, 0]),
        (True, 0, True): ([2, 2, 0, 0, N, N], [1, 1, 1, 2, F, F], [1, 1, 2, 2, 0, 0]),
        (True, 2, False): ([3, 3, N, 0, N, N], [2, 2, F, 2, F, F], [1, 1, 0, 2, 0, 0]),
    }
    return s, {k: (np.array(v[0], dtype=np.uint32), np.array(v[1], dtype=np.uint16), np.array(v[2], dtype=np.uint32))
               for k, v in table.items()}
