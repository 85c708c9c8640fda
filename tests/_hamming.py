"""The all-against-all path for any d (cmpr_hamming_matrix, cmpr_hamming_neighbors): a numpy brute force of the
reference's process_trad (overlap.cc:286-359) -- same length, same V and J unless -g, at most d differing positions --,
the oracle's pair list as CSR, and the inputs and figures the CPU and GPU tests share (test infrastructure).
Nothing here calls the library under test."""

import functools
import os

import numpy as np

import _dedup
import _neighbors
import _oracle
from compairr_amd import Options, RepertoireSet, synth
from compairr_amd.sets import AA, NT

HERE = os.path.dirname(os.path.abspath(__file__))
INPUTS = os.path.join(HERE, "golden", "inputs")
EXPECTED = os.path.join(HERE, "golden", "expected")

# HAMMING_REG_WORDS of compairr_amd/csrc/allpairs.h (tests/test_hamming_cpu.py reads the constant there): a sequence
# of more 32-bit words -- four amino acids or sixteen nucleotides each -- takes the generic form
REG_WORDS = 16
REG_BOUND = {False: REG_WORDS * 4, True: REG_WORDS * 16}        # residues, by `nucleotides`


def options(**kw):
    return Options(n_v_genes=2, n_j_genes=2, **kw)


# ---- the yardsticks ----

def brute_csr(set1, set2, d, ignore_genes=False):
    """(row_start uint64[n1 + 1], hits uint32[E], distance uint16[E]) by numpy: per length, every sequence of set1
    against every sequence of set2 of that length"""
    len1, len2 = set1.lengths, set2.lengths
    off1, off2 = set1.offsets.astype(np.int64), set2.offsets.astype(np.int64)
    q_all, h_all, d_all = [], [], []
    for L in np.intersect1d(np.unique(len1), np.unique(len2)):
        L = int(L)
        i1, i2 = np.nonzero(len1 == L)[0], np.nonzero(len2 == L)[0]
        span = np.arange(L, dtype=np.int64)
        a = set1.residues[off1[i1, None] + span].reshape(len(i1), L)
        b = set2.residues[off2[i2, None] + span].reshape(len(i2), L)
        step = max(1, (1 << 24) // max(1, len(i2) * max(L, 1)))
        for lo in range(0, len(i1), step):
            part = a[lo:lo + step]
            dist = (part[:, None, :] != b[None, :, :]).sum(axis=2)
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
    return row_start, hits, dd[order].astype(np.uint16)


def distances(set1, set2, row_start, hits):
    """uint16[E]: the numpy Hamming distance of every edge of a CSR whose pairs have one length each"""
    row_start = np.asarray(row_start).astype(np.int64)
    hits = np.asarray(hits).astype(np.int64)
    query = np.repeat(np.arange(set1.n, dtype=np.int64), np.diff(row_start))
    len1 = set1.lengths[query]
    assert np.array_equal(len1, set2.lengths[hits]), "an edge joins two lengths"
    off1, off2 = set1.offsets.astype(np.int64)[query], set2.offsets.astype(np.int64)[hits]
    out = np.zeros(len(hits), dtype=np.uint16)
    for L in np.unique(len1):
        sel = np.nonzero(len1 == L)[0]
        span = np.arange(int(L), dtype=np.int64)
        out[sel] = (set1.residues[off1[sel, None] + span] != set2.residues[off2[sel, None] + span]).sum(axis=1)
    return out


def oracle_want(set1, set2, opt):
    """(row_start, hits, distance): the oracle's pair list at opt.differences as CSR, numpy distances beside it"""
    row_start, hits = _neighbors.oracle_csr(set1, set2, opt)
    dist = distances(set1, set2, row_start, hits)
    dist.setflags(write=False)
    return row_start, hits, dist


def histogram(dist, d):
    return np.bincount(dist, minlength=d + 1).tolist()


def same_group_pairs(set1, set2, ignore_genes):
    """the number of pairs with one length (and one V and J): what any d >= the longest sequence finds"""
    def keys(s):
        k = s.lengths.astype(np.int64)
        return k if ignore_genes else (k * 1000 + s.v_gene) * 1000 + s.j_gene
    k1, c1 = np.unique(keys(set1), return_counts=True)
    k2, c2 = np.unique(keys(set2), return_counts=True)
    _, i1, i2 = np.intersect1d(k1, k2, return_indices=True)
    return int((c1[i1].astype(np.int64) * c2[i2]).sum())


# ---- the inputs of the issue and their figures (the CPU test asserts them with the oracle and the brute force) ----

@functools.lru_cache(maxsize=None)
def aa_sets():
    return (synth.tiny_set(300, 4, letters=3, min_len=3, max_len=9),
            synth.tiny_set(257, 5, letters=3, min_len=3, max_len=9))


@functools.lru_cache(maxsize=None)
def nt_sets():
    s = synth.tiny_set(300, 6, alphabet_size=4, letters=4, min_len=5, max_len=12)
    return s, s


@functools.lru_cache(maxsize=None)
def dense_sets():
    return (synth.tiny_set(70, 11, alphabet_size=4, letters=4, min_len=8, max_len=8),
            synth.tiny_set(9001, 12, alphabet_size=4, letters=4, min_len=8, max_len=8))


@functools.lru_cache(maxsize=None)
def empty_sets():
    s = synth.tiny_set(200, 13, letters=2, min_len=0, max_len=3)
    return s, s


SETS = {"aa": (aa_sets, False), "nt": (nt_sets, True), "dense": (dense_sets, True), "empty": (empty_sets, False)}

# (input, d, ignore_genes): edges
EDGES = {
    ("aa", 3, False): 563, ("aa", 3, True): 2_211, ("aa", 4, False): 1_038, ("aa", 4, True): 4_090,
    ("aa", 6, False): 1_924, ("aa", 6, True): 7_590,
    ("nt", 3, False): 526, ("nt", 3, True): 1_254, ("nt", 4, False): 922, ("nt", 4, True): 2_774,
    ("nt", 6, False): 1_854, ("nt", 6, True): 6_652,
    ("dense", 8, True): 630_070, ("dense", 4, True): 71_755, ("dense", 4, False): 18_141, ("dense", 3, True): 17_250,
    ("empty", 3, False): 2_732, ("empty", 3, True): 10_294,
}
HISTOGRAMS = {
    ("aa", 3, False): [0, 8, 110, 445], ("aa", 3, True): [0, 49, 383, 1_779],
    ("nt", 3, False): [300, 4, 50, 172], ("nt", 3, True): [302, 36, 222, 694],
    ("dense", 8, True): [14, 234, 2_478, 14_524, 54_505, 131_374, 196_318, 167_566, 63_057],
}
LONGEST_ROW = {("aa", 3, False): 10, ("aa", 3, True): 32}


def sets_of(name):
    return SETS[name][0]()


def options_of(name, ignore_genes, **more):
    return options(nucleotides=SETS[name][1], ignore_genes=ignore_genes, **more)


@functools.lru_cache(maxsize=None)
def want(name, d, ignore_genes):
    s1, s2 = sets_of(name)
    return oracle_want(s1, s2, options_of(name, ignore_genes, differences=d))


# ---- lengths at the word and form edges, built by hand ----

EDGE_D = 3


def edge_lengths(nucleotides):
    bound = REG_BOUND[nucleotides]
    return sorted({1, 3, 4, 5, 16, 17, 31, 32, 33, 36, 37, 63, 64, 65, 96, 97, 200, 1000, bound, bound + 1})


@functools.lru_cache(maxsize=None)
def edge_sets(nucleotides):
    """set 2: per length L a seeded base sequence; set 1: per L the mutants of the base with k = 0 .. EDGE_D + 1
    substitutions (k <= L; the changed positions include 0 and L - 1 when k >= 2) and one sequence of length L + 1 --
    the base with a residue appended -- that no base of its own length matches unless it is that length's mutant.
    One V gene, one J gene, two repertoires, counts 1 .. 5.  Also the expected k of every set-1 sequence
    (-1: the appended one)."""
    A = 4 if nucleotides else 20
    rng = np.random.default_rng(1600 + A)
    rows1, rows2, ks = [], [], []
    for L in edge_lengths(nucleotides):
        base = rng.integers(0, A, size=L, dtype=np.uint8)
        rows2.append(base)
        for k in range(min(EDGE_D + 1, L) + 1):
            m = base.copy()
            where = []
            if k >= 2:
                where = [0, L - 1]
            if k >= 1:
                inner = [p for p in rng.permutation(L).tolist() if p not in where]
                where = where + inner[:k - len(where)]
            for p in where:
                m[p] = (m[p] + 1 + rng.integers(0, A - 1)) % A
            rows1.append(m)
            ks.append(k)
        rows1.append(np.concatenate([base, base[:1]]))
        ks.append(-1)

    def build(rows, seed, prefix):
        n = len(rows)
        off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum([len(r) for r in rows], out=off[1:])
        r = np.random.default_rng(seed)
        rep = (np.arange(n) % 2).astype(np.uint32)
        return RepertoireSet(np.concatenate(rows), off, np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32),
                             rep, r.integers(1, 6, size=n, dtype=np.uint64), [prefix + "1", prefix + "2"], ["V0"], ["J0"],
                             NT if nucleotides else AA)
    return build(rows1, 161, "E"), build(rows2, 162, "F"), np.array(ks)


def edge_options(nucleotides, **more):
    return Options(n_v_genes=1, n_j_genes=1, nucleotides=nucleotides, **more)


# ---- the reference's own d = 3 matrices ----

GOLDEN = {"ref_kat_09": ("seta.tsv", "setb.tsv"), "tiny_aa_d3": ("tiny_aa_a.tsv", "tiny_aa_b.tsv")}


def golden_sets(name):
    """the two input files of a golden case, their genes renumbered by name into one numbering"""
    a, b = (_dedup.read_tsv(os.path.join(INPUTS, f)) for f in GOLDEN[name])
    for names, field in (("v_names", "v_gene"), ("j_names", "j_gene")):
        joint = {}
        for s in (a, b):
            own = getattr(s, names)
            renum = np.array([joint.setdefault(x, len(joint)) for x in own], dtype=np.uint32)
            setattr(s, field, renum[getattr(s, field)] if len(own) else getattr(s, field))
        for s in (a, b):
            setattr(s, names, list(joint))
    return a, b


def golden_cells(name):
    """{(row repertoire, column repertoire): the cell as the reference printed it}"""
    with open(os.path.join(EXPECTED, name + ".tsv")) as fh:
        lines = fh.read().splitlines()
    cols = lines[0].split("\t")[1:]
    cells = {}
    for line in lines[1:]:
        f = line.split("\t")
        for c, text in zip(cols, f[1:]):
            cells[(f[0], c)] = text
    return cells
