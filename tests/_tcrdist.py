"""The all-against-all path under the weighted CDR3 distance (cmpr_tcrdist_neighbors, cmpr_tcrdist_matrix): a numpy
brute force that restates the definition of include/compairr_hip.h and nothing else -- vectorised across all pairs of
one (length 1, length 2) block --, the CSR (_neighbors.csr_of_pairs) and the matrix cells (_edit.matrix_of) of its pair
list, and the inputs and figures the CPU and GPU tests share (test infrastructure).  Nothing here calls the library
under test."""

import functools

import numpy as np

import _neighbors
from compairr_amd import Options, RepertoireSet, synth
from compairr_amd.sets import AA

FIXED, SLIDING = 0, 1
MAX_LEN = 256                  # PAIRS_MAX_LEN of compairr_amd/csrc/allpairs.h


def options(**kw):
    return Options(n_v_genes=2, n_j_genes=2, **kw)


# ---- the yardstick ----

def gap_range(Ls, mode):
    """(lo, hi): the gap positions tried for a shorter sequence of Ls residues"""
    if mode == FIXED:
        g = min(6, 3 + (Ls - 5) // 2)          # (Python's // floors)
        return g, g
    lo, hi = 5, Ls - 5
    while lo > hi:
        lo, hi = lo - 1, hi + 1
    return lo, hi


def block_distances(a, b, W, ntrim, ctrim, gap_penalty, mode):
    """int64[m1, m2]: the distance of every row of a (m1 x L1, set 1) to every row of b (m2 x L2, set 2), no V term.
    W is indexed [set-1 residue][set-2 residue] whichever side is shorter."""
    (m1, L1), (m2, L2) = a.shape, b.shape
    W = np.asarray(W).astype(np.int64)
    a, b = a.astype(np.int64), b.astype(np.int64)
    Ls, delta = min(L1, L2), abs(L1 - L2)
    k = np.arange(Ls)

    def w(p1, p2):
        """int64[Ls, m1, m2]: positions p1 of the set-1 sequences against positions p2 of the set-2 sequences"""
        return W[a[:, p1].T[:, :, None], b[:, p2].T[:, None, :]]

    same = w(k, k)                                          # w(s_k, l_k)
    if L1 == L2:
        return same[ntrim:max(ntrim, L1 - ctrim)].sum(axis=0)
    moved = w(k, k + delta) if L1 < L2 else w(k + delta, k)  # w(s_k, l_{k + delta})
    same[:ntrim] = 0                                        # the first sum runs over k = ntrim .. g - 1
    moved[max(0, Ls - ctrim):] = 0                          # the second over k = g .. Ls - 1 - ctrim
    zero = np.zeros((1, m1, m2), dtype=np.int64)
    first = np.concatenate([zero, np.cumsum(same, axis=0)])                    # [g]: sum over k < g
    second = np.concatenate([np.cumsum(moved[::-1], axis=0)[::-1], zero])      # [g]: sum over k >= g
    lo, hi = gap_range(Ls, mode)
    assert 0 <= lo <= hi <= Ls
    return (first[lo:hi + 1] + second[lo:hi + 1]).min(axis=0) + delta * gap_penalty


def brute_csr(set1, set2, W, ntrim, ctrim, gap_penalty, mode, cutoff, ignore_genes=False, V=None):
    """(row_start uint64[n1 + 1], hits uint32[E], distance uint16[E]): every sequence of set1 against every sequence
    of set2, block by block of lengths.  Without V the pairs share both genes unless ignore_genes; with V any two V
    genes pair at V[v1][v2] and the J gene plays no part."""
    len1, len2 = set1.lengths.astype(np.int64), set2.lengths.astype(np.int64)
    off1, off2 = set1.offsets.astype(np.int64), set2.offsets.astype(np.int64)
    q_all, h_all, d_all = [], [], []
    for L1 in np.unique(len1).tolist():
        i1 = np.nonzero(len1 == L1)[0]
        a = set1.residues[off1[i1, None] + np.arange(L1, dtype=np.int64)].reshape(len(i1), L1)
        for L2 in np.unique(len2).tolist():
            if abs(L1 - L2) * gap_penalty > cutoff:
                continue                                    # (no pair of the block can be within the cutoff)
            i2 = np.nonzero(len2 == L2)[0]
            b = set2.residues[off2[i2, None] + np.arange(L2, dtype=np.int64)].reshape(len(i2), L2)
            dist = block_distances(a, b, W, ntrim, ctrim, gap_penalty, mode)
            if V is not None:
                dist = dist + np.asarray(V).astype(np.int64)[set1.v_gene[i1].astype(np.int64)[:, None],
                                                             set2.v_gene[i2].astype(np.int64)[None, :]]
            ok = dist <= cutoff
            if V is None and not ignore_genes:
                ok &= set1.v_gene[i1, None] == set2.v_gene[None, i2]
                ok &= set1.j_gene[i1, None] == set2.j_gene[None, i2]
            q, h = np.nonzero(ok)
            q_all.append(i1[q])
            h_all.append(i2[h])
            d_all.append(dist[q, h])
    if q_all:
        q, h, dd = np.concatenate(q_all), np.concatenate(h_all), np.concatenate(d_all)
    else:
        q = h = dd = np.zeros(0, dtype=np.int64)
    order = np.lexsort((h, q))
    row_start, hits = _neighbors.csr_of_pairs(set1.n, np.stack([q[order], h[order]], axis=1))
    out = (row_start, hits, dd[order].astype(np.uint16))
    for x in out:
        x.setflags(write=False)
    return out


def distance(x, y, W, ntrim, ctrim, gap_penalty, mode):
    """the distance of two strings over sets.AA"""
    a = np.array([[AA.index(ch) for ch in x]], dtype=np.uint8).reshape(1, len(x))
    b = np.array([[AA.index(ch) for ch in y]], dtype=np.uint8).reshape(1, len(y))
    return int(block_distances(a, b, W, ntrim, ctrim, gap_penalty, mode)[0, 0])


# ---- the inputs of the issue and their figures (the CPU test asserts them with the brute force) ----

@functools.lru_cache(maxsize=None)
def table():
    rng = np.random.default_rng(5)
    W = rng.integers(1, 5, (20, 20))
    np.fill_diagonal(W, 0)
    W = np.minimum(W, W.T).astype(np.uint8)
    W.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def tiny_sets():
    kw = dict(letters=3, min_len=0, max_len=12)
    return synth.tiny_set(120, 41, **kw), synth.tiny_set(110, 42, **kw)


@functools.lru_cache(maxsize=None)
def mid_sets():
    kw = dict(letters=4, min_len=6, max_len=16)
    return synth.tiny_set(120, 41, **kw), synth.tiny_set(110, 42, **kw)


SETS = {"tiny": tiny_sets, "mid": mid_sets}

# (ntrim, ctrim, gap_penalty, gap_mode, cutoff)
CASES = [(3, 2, 4, FIXED, 6), (3, 2, 4, SLIDING, 6), (0, 0, 4, SLIDING, 8), (3, 2, 0, SLIDING, 4), (3, 2, 4, SLIDING, 0)]

# (input, case, ignore_genes): edges
EDGES = {
    ("tiny", 0, True): 2_034, ("tiny", 1, True): 2_038, ("tiny", 2, True): 1_237, ("tiny", 3, True): 12_015,
    ("tiny", 4, True): 520,
    ("mid", 0, True): 694, ("mid", 1, True): 717, ("mid", 2, True): 61, ("mid", 3, True): 5_471, ("mid", 4, True): 9,
    ("tiny", 0, False): 506, ("tiny", 1, False): 509, ("tiny", 2, False): 333, ("tiny", 3, False): 2_957,
    ("tiny", 4, False): 154,
    ("mid", 0, False): 203, ("mid", 1, False): 211, ("mid", 2, False): 22, ("mid", 3, False): 1_505,
    ("mid", 4, False): 4,
}
KEYS = list(EDGES)
IDS = ["%s-case%d%s" % (k[0], k[1], "-g" if k[2] else "") for k in KEYS]
PAIRS = 13_200


def sets_of(name):
    return SETS[name]()


@functools.lru_cache(maxsize=None)
def want(name, case, ignore_genes):
    s1, s2 = sets_of(name)
    ntrim, ctrim, gap, mode, cutoff = CASES[case]
    return brute_csr(s1, s2, table(), ntrim, ctrim, gap, mode, cutoff, ignore_genes)


def hand_set(rows, seed, n_rep=2, v_gene=None, j_gene=None, n_v=1, n_j=1):
    """a set of the given residue rows (arrays of codes, any lengths): repertoires dealt in turn, counts 1 .. 5"""
    n = len(rows)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    res = np.concatenate([np.asarray(r, dtype=np.uint8) for r in rows]) if off[-1] else np.zeros(0, dtype=np.uint8)
    rng = np.random.default_rng(seed)
    zeros = np.zeros(n, dtype=np.uint32)
    return RepertoireSet(res.astype(np.uint8), off, zeros if v_gene is None else np.asarray(v_gene, dtype=np.uint32),
                         zeros if j_gene is None else np.asarray(j_gene, dtype=np.uint32),
                         (np.arange(n) % n_rep).astype(np.uint32), rng.integers(1, 6, size=n, dtype=np.uint64),
                         ["H%d" % (k + 1) for k in range(n_rep)], ["V%d" % k for k in range(n_v)],
                         ["J%d" % k for k in range(n_j)], AA)


# ---- lengths at the edges of the query forms, built by hand ----

EDGE_LENGTHS = (0, 1, 2, 3, 4, 5, 6, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256)


@functools.lru_cache(maxsize=None)
def edge_sets():
    """one stem of 256 residues over two letters that cost 1 against each other under table(); per length of
    EDGE_LENGTHS the stem's first residues, then that sequence with one residue replaced by a third letter at the
    front, in the middle and at the end: distances stay small, also across neighbouring lengths (a shifted stretch of
    n residues costs some n / 2).  Set 2 holds the same stems with other letters put in.  One V gene, one J gene."""
    W = table()
    x = 0
    y = int(np.nonzero(W[x] == 1)[0][0])
    others = [int(j) for j in np.nonzero(W[x] >= 2)[0][:2]]
    rng = np.random.default_rng(2500)
    stem = np.array([x, y], dtype=np.uint8)[rng.integers(0, 2, size=MAX_LEN)]

    def rows(letter):
        out = []
        for n in EDGE_LENGTHS:
            base = stem[:n].copy()
            out.append(base)
            for pos in sorted({0, n // 2, n - 1} & set(range(n))):
                m = base.copy()
                m[pos] = letter
                out.append(m)
        return out
    return hand_set(rows(others[0]), 251), hand_set(rows(others[1]), 252)


EDGE_GAP, EDGE_CUTOFF = 2, 70
