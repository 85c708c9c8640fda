"""The all-against-all path under edit distance (cmpr_edit_neighbors, cmpr_edit_matrix): a numpy brute force of the
Levenshtein distance -- the DP over the rows of one sequence, vectorised across all pairs of one (length 1, length 2)
block --, the CSR and the matrix cells of its pair list, and the inputs and figures the CPU and GPU tests share (test
infrastructure).  Nothing here calls the library under test."""

import functools

import numpy as np

import _neighbors
from compairr_amd import Options, RepertoireSet, synth
from compairr_amd.sets import AA, NT

MAX_LEN = 256                  # PAIRS_MAX_LEN of compairr_amd/csrc/allpairs.h: four 64-bit words of the column


def options(**kw):
    return Options(n_v_genes=2, n_j_genes=2, **kw)


# ---- the yardstick ----

def block_distances(a, b):
    """int32[m1, m2]: the Levenshtein distance of every row of a (m1 x L1) to every row of b (m2 x L2).  Row i + 1 of
    the DP from row i: t[j] = min(prev[j] + 1, prev[j - 1] + (a[i] != b[j - 1])), then the insertions along the row,
    new[j] = min over k <= j of t[k] + (j - k), as a running minimum of t[k] - k."""
    (m1, L1), (m2, L2) = a.shape, b.shape
    j = np.arange(L2 + 1, dtype=np.int32)
    prev = np.broadcast_to(j, (m1, m2, L2 + 1)).copy()
    for i in range(L1):
        t = np.empty_like(prev)
        t[..., 0] = i + 1
        t[..., 1:] = np.minimum(prev[..., 1:] + 1, prev[..., :-1] + (a[:, None, i, None] != b[None, :, :]))
        prev = np.minimum.accumulate(t - j, axis=2) + j
    return prev[..., L2]


def brute_csr(set1, set2, d, ignore_genes=False):
    """(row_start uint64[n1 + 1], hits uint32[E], distance uint16[E]): per pair of lengths no more than d apart, every
    sequence of set1 of the one against every sequence of set2 of the other"""
    len1, len2 = set1.lengths.astype(np.int64), set2.lengths.astype(np.int64)
    off1, off2 = set1.offsets.astype(np.int64), set2.offsets.astype(np.int64)
    q_all, h_all, d_all = [], [], []
    for L1 in np.unique(len1).tolist():
        i1 = np.nonzero(len1 == L1)[0]
        a = set1.residues[off1[i1, None] + np.arange(L1, dtype=np.int64)].reshape(len(i1), L1)
        for L2 in np.unique(len2).tolist():
            if abs(L1 - L2) > d:
                continue
            i2 = np.nonzero(len2 == L2)[0]
            b = set2.residues[off2[i2, None] + np.arange(L2, dtype=np.int64)].reshape(len(i2), L2)
            step = max(1, (1 << 23) // max(1, len(i2) * (L2 + 1)))
            for lo in range(0, len(i1), step):
                dist = block_distances(a[lo:lo + step], b)
                ok = dist <= d
                if not ignore_genes:
                    ok &= set1.v_gene[i1[lo:lo + step], None] == set2.v_gene[None, i2]
                    ok &= set1.j_gene[i1[lo:lo + step], None] == set2.j_gene[None, i2]
                q, h = np.nonzero(ok)
                q_all.append(i1[lo + q])
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


def queries_of(row_start):
    return np.repeat(np.arange(len(row_start) - 1, dtype=np.int64), np.diff(np.asarray(row_start).astype(np.int64)))


def cross_length(set1, set2, row_start, hits):
    """the number of edges that join two lengths"""
    return int((set1.lengths[queries_of(row_start)] != set2.lengths[np.asarray(hits).astype(np.int64)]).sum())


def histogram(dist, d):
    return np.bincount(dist, minlength=d + 1).tolist()


def matrix_of(set1, set2, row_start, hits, opt):
    """uint64 cells summed from a pair list as cmpr_hamming_matrix documents them: product, min, max, count1 + count2
    for the mean, the product sum for MH and the min sum for Jaccard (cmpr_overlap_matrix's integer sums, as
    tests/_existence.py has them), 1 per pair with ignore_counts; n1 rows with `existence`.  uint64 arithmetic,
    wrapping."""
    q, h = queries_of(row_start), np.asarray(hits).astype(np.int64)
    f, g = set1.count[q].astype(np.uint64), set2.count[h].astype(np.uint64)
    if opt.ignore_counts:
        v = np.ones(len(q), dtype=np.uint64)
    else:
        with np.errstate(over="ignore"):
            v = {"product": lambda: f * g, "min": lambda: np.minimum(f, g), "max": lambda: np.maximum(f, g),
                 "mean": lambda: f + g, "mh": lambda: f * g, "jaccard": lambda: np.minimum(f, g)}[opt.score.lower()]()
    rows = q if opt.existence else set1.repertoire[q].astype(np.int64)
    m = np.zeros((set1.n if opt.existence else set1.n_repertoires, set2.n_repertoires), dtype=np.uint64)
    with np.errstate(over="ignore"):
        np.add.at(m, (rows, set2.repertoire[h].astype(np.int64)), v)
    return m


def same_genes_pairs(set1, set2, ignore_genes):
    """the number of pairs with one V and one J: what a d >= the longest sequence finds"""
    if ignore_genes:
        return set1.n * set2.n
    k1 = set1.v_gene.astype(np.int64) * 1000 + set1.j_gene
    k2 = set2.v_gene.astype(np.int64) * 1000 + set2.j_gene
    return int((np.bincount(k1, minlength=4000).astype(np.int64) * np.bincount(k2, minlength=4000)).sum())


# ---- the inputs of the issue and their figures (the CPU test asserts them with the brute force and the oracle) ----

@functools.lru_cache(maxsize=None)
def nt_sets():
    kw = dict(alphabet_size=4, letters=3, min_len=2, max_len=8)
    return synth.tiny_set(300, 31, **kw), synth.tiny_set(257, 32, **kw)


@functools.lru_cache(maxsize=None)
def aa_sets():
    s = synth.tiny_set(300, 33, letters=3, min_len=1, max_len=9)
    return s, s


@functools.lru_cache(maxsize=None)
def min0_sets():
    kw = dict(letters=2, min_len=0, max_len=4)
    return synth.tiny_set(300, 31, **kw), synth.tiny_set(257, 32, **kw)


@functools.lru_cache(maxsize=None)
def long_row_sets():
    """70 queries against 9 001 nucleotide sequences of 7 .. 9 residues: at d = 9 every pair is an edge, rows of 9 001"""
    kw = dict(alphabet_size=4, letters=4, min_len=7, max_len=9)
    return synth.tiny_set(70, 11, **kw), synth.tiny_set(9001, 12, **kw)


SETS = {"nt": (nt_sets, True), "aa": (aa_sets, False), "min0": (min0_sets, False), "long": (long_row_sets, True)}

# (input, d, ignore_genes): edges
EDGES = {
    ("nt", 1, False): 372, ("nt", 1, True): 1_478, ("nt", 2, False): 1_706, ("nt", 2, True): 6_784,
    ("nt", 3, False): 4_420, ("nt", 3, True): 17_458, ("nt", 4, False): 8_221, ("nt", 4, True): 32_981,
    ("aa", 1, False): 1_272, ("aa", 1, True): 4_182, ("aa", 2, False): 3_162, ("aa", 2, True): 11_652,
    ("aa", 3, False): 6_652, ("aa", 3, True): 25_450, ("aa", 5, False): 16_618, ("aa", 5, True): 65_348,
}
HISTOGRAMS = {
    ("nt", 2, False): [23, 349, 1_334], ("nt", 2, True): [112, 1_366, 5_306],
    ("aa", 2, False): [416, 856, 1_890], ("aa", 2, True): [830, 3_352, 7_470],
}
LONGEST_ROW = {
    ("nt", 2, False): 30, ("nt", 2, True): 92, ("nt", 3, False): 41, ("nt", 3, True): 155,
    ("nt", 4, False): 58, ("nt", 4, True): 216,
    ("aa", 2, False): 31, ("aa", 2, True): 111, ("aa", 3, False): 45, ("aa", 3, True): 181,
    ("aa", 5, False): 83, ("aa", 5, True): 288,
}
CROSS_LENGTH = {("nt", 2, False): 974, ("nt", 2, True): 3_875, ("aa", 2, False): 2_004, ("aa", 2, True): 7_834}
# min0 at d = 1, by ignore_genes: (Levenshtein edges, the oracle's with indels)
MIN0 = {False: (2_913, 2_213), True: (11_655, 8_847)}
LONG_ROW_EDGES = 630_070


def sets_of(name):
    return SETS[name][0]()


def options_of(name, ignore_genes, **more):
    return options(nucleotides=SETS[name][1], ignore_genes=ignore_genes, **more)


@functools.lru_cache(maxsize=None)
def want(name, d, ignore_genes):
    s1, s2 = sets_of(name)
    return brute_csr(s1, s2, d, ignore_genes)


# ---- lengths at the edges of the column words, built by hand ----

EDGE_D = 3
EDGE_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256)

# the edits of a base of n residues, by name: ("ins", position, ) / ("del", position) / ("sub", position); a position
# is taken modulo the sequence as it stands, negative from the end.  "sub63" .. "sub128": bit 63 / 64 and 127 / 128
# of the column.
RECIPES = [
    [],
    [("ins", 0)], [("ins", None)], [("del", 0)], [("del", -1)],
    [("sub", 63)], [("sub", 64)], [("sub", 127)], [("sub", 128)], [("sub", 0)], [("sub", -1)],
    [("del", -1), ("ins", 0)], [("del", 0), ("ins", None)], [("sub", 63), ("sub", 64)], [("sub", 127), ("sub", 128)],
    [("del", 0), ("del", -1)], [("del", 0), ("sub", 63), ("ins", None)], [("del", -1), ("sub", 64), ("ins", 0)],
    [("sub", 0), ("sub", 63), ("sub", -1)], [("del", 0), ("del", 0), ("del", -1)],
    [("sub", 0), ("sub", 62), ("sub", 65), ("sub", -1)], [("del", 0), ("del", -1), ("ins", 0), ("ins", None)],
    [("del", 0), ("del", 0), ("del", -1), ("del", -1)],
]


def apply_recipe(base, recipe, A, rng):
    """the base edited; None when the recipe does not fit it (a position beyond it, a length above MAX_LEN)"""
    s = base.tolist()
    for op in recipe:
        kind, pos = op[0], op[1]
        if kind == "ins":
            if len(s) >= MAX_LEN:
                return None
            s.insert(len(s) if pos is None else pos, int(rng.integers(0, A)))
            continue
        if not s or pos >= len(s) or -pos > len(s):
            return None
        if kind == "del":
            del s[pos]
        else:
            s[pos] = (s[pos] + 1 + int(rng.integers(0, A - 1))) % A
    return np.array(s, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def edge_sets(nucleotides):
    """set 2: per length of EDGE_LENGTHS a seeded base; set 1: per base every recipe that fits it.  Also the number
    of operations of every set-1 sequence and the set-2 number of its base.  One V gene, one J gene, two
    repertoires, counts 1 .. 5."""
    A = 4 if nucleotides else 20
    rng = np.random.default_rng(2100 + A)
    rows1, rows2, ops, base_of = [], [], [], []
    for k, n in enumerate(EDGE_LENGTHS):
        base = rng.integers(0, A, size=n, dtype=np.uint8)
        rows2.append(base)
        for recipe in RECIPES:
            m = apply_recipe(base, recipe, A, rng)
            if m is not None:
                rows1.append(m)
                ops.append(len(recipe))
                base_of.append(k)

    def build(rows, seed, prefix):
        n = len(rows)
        off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum([len(r) for r in rows], out=off[1:])
        r = np.random.default_rng(seed)
        rep = (np.arange(n) % 2).astype(np.uint32)
        res = np.concatenate(rows).astype(np.uint8)
        return RepertoireSet(res, off, np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), rep,
                             r.integers(1, 6, size=n, dtype=np.uint64), [prefix + "1", prefix + "2"], ["V0"], ["J0"],
                             NT if nucleotides else AA)
    return build(rows1, 211, "E"), build(rows2, 212, "F"), np.array(ops), np.array(base_of)


def edge_options(nucleotides, **more):
    return Options(n_v_genes=1, n_j_genes=1, nucleotides=nucleotides, **more)


@functools.lru_cache(maxsize=None)
def edge_want(nucleotides):
    s1, s2, _, _ = edge_sets(nucleotides)
    return brute_csr(s1, s2, EDGE_D)


def hand_set(seqs, v_genes):
    res = np.array([AA.index(c) for s in seqs for c in s], dtype=np.uint8)
    off = np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)
    n = len(seqs)
    return RepertoireSet(res, off, np.array(v_genes, dtype=np.uint32), np.zeros(n, dtype=np.uint32),
                         np.zeros(n, dtype=np.uint32), np.ones(n, dtype=np.uint64), ["R1"], ["V0", "V1"], ["J0"], AA)
