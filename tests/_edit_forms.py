"""The edit-distance kernel (compairr_amd/csrc/edit.hip, ed_compare_kernel) at CDR3 lengths, in every register form of
the query and at every distance: two hand-built inputs, their figures from the numpy brute force (tests/_edit.py) and
the helpers the CPU and GPU tests share (test infrastructure).  Nothing here calls the library under test.

What each input reaches (NW: packed words of the query held in registers, 0 a query read from global memory; W: 64-bit
words of a reference's column, 1 up to 64 residues, 2 up to 128, 4 up to 256, or what edit_words forces):

  family_sets(False)  clonal families around 26 ancestor lengths from 5 to 66, full alphabet of 20, 5 x 3 genes, every
                      distance 0 .. 6 and beyond: NW = 2 (up to 8 residues), 4 (9 .. 16), 8 (17 .. 32), 16 (33 .. 64)
                      and 0 (65 and more), each with hundreds of edges of its own queries and edges into the next
                      form across 8 / 9, 16 / 17, 32 / 33 and 64 / 65; W = 1 and, for the references of 65 and more
                      residues, W = 2; W = 2 and 4 for every form under edit_words.  Sinks: CSR (edit_neighbors),
                      matrix, nearest, and link on the two sets joined (family_union).  One set-1 family has no
                      partner group in set 2 within 6 residues (a job that is never built), one meets a key miss
                      between two key hits in the partner search of ed_setup.
  family_sets(True)   the same around 16 ancestor lengths from 12 to 90 over 4 letters: NW = 2 (up to 32), 4 (33 .. 64)
                      and 0; W = 1 and 2; the crossings 32 / 33 and 64 / 65.  The same sinks and gene cases.
  distance_sets(nt)   72 sequences a set at the lengths 1 .. 256 where the query form and the column's word count
                      change, random, homopolymer, period 3 and rotated: with ignore_genes and d = 256 all 5 184 pairs
                      are edges, some 200 distinct distances up to 256 -- every NW against W = 1, 2 and 4, the score
                      read at every bit of the last word, unrelated and low-complexity columns.  Sinks: CSR, matrix,
                      nearest."""

import functools

import numpy as np

import _cluster
import _edit
import _edit_cluster
import _edit_nearest
from compairr_amd import Options, RepertoireSet
from compairr_amd.sets import AA, NT

# ---- the register form of a query ----

REG_RESIDUES = 64              # PAIRS_REG_RESIDUES of compairr_amd/csrc/allpairs.h: a longer query is read from global memory
FORMS = (2, 4, 8, 16)          # the forms pairs_form_of of compairr_amd/csrc/allpairs.hip walks through
STRIDES = (1, 2, 3, 4, 5, 6, 8, 12, 16)    # the word counts of stride_of, compairr_amd/csrc/allpairs.hip
PER_WORD = {False: 4, True: 16}            # residues per packed word: amino acids, nucleotides
ALL_FORMS = {False: (2, 4, 8, 16, 0), True: (2, 4, 0)}
CROSSINGS = {False: (8, 16, 32, 64), True: (32, 64)}     # an edge crosses c: one end has at most c residues, one more


def form_of(length, nucleotides):
    """pairs_form_of(len, stride_of(len, per_word)): 2, 4, 8, 16, or 0"""
    if length > REG_RESIDUES:
        return 0
    words = max(1, -(-length // PER_WORD[nucleotides]))
    stride = next((f for f in STRIDES if words <= f), words)
    return next((f for f in FORMS if stride <= f), 0)


def forms_of(lengths, nucleotides):
    return np.array([form_of(int(n), nucleotides) for n in lengths], dtype=np.int64)


# ---- input A: clonal families at CDR3 lengths ----

ANCESTORS = {
    False: (5, 7, 8, 9, 10, 12, 13, 14, 15, 16, 17, 18, 20, 22, 24, 27, 30, 31, 32, 33, 34, 40, 48, 62, 64, 66),
    True: (12, 20, 30, 31, 32, 33, 34, 36, 45, 48, 60, 63, 64, 65, 66, 90),
}
DESCENDANTS = 10               # per ancestor and set; descendant m after m % 7 operations
N_V, N_J = 5, 3
FAMILY_D = (1, 2, 3, 6)
SEED = {False: 5203, True: 5200}
# two (V, J) no ordinary sequence draws
PARTNERLESS_VJ, KEYMISS_VJ = (4, 2), (4, 1)
# the family whose set-1 members carry PARTNERLESS_VJ, and the far family three of whose set-2 members carry it
PARTNERLESS, FAR = {False: 20, True: 20}, {False: 66, True: 90}
# the family whose set-1 members carry KEYMISS_VJ; in set 2 its members do, except those of the ancestor's own length
KEYMISS = {False: 14, True: 45}
ORDINARY_VJ = [(v, j) for v in range(N_V) for j in range(N_J) if (v, j) not in (PARTNERLESS_VJ, KEYMISS_VJ)]


def mutated(seq, ops, A, rng):
    """`seq` after `ops` random operations: a substitution to a different letter, an insertion of a random letter or a
    deletion, at a random position (an empty sequence takes an insertion)"""
    s = list(seq)
    for _ in range(ops):
        kind = int(rng.integers(0, 3)) if s else 1
        if kind == 0:
            p = int(rng.integers(0, len(s)))
            s[p] = (s[p] + 1 + int(rng.integers(0, A - 1))) % A
        elif kind == 1:
            s.insert(int(rng.integers(0, len(s) + 1)), int(rng.integers(0, A)))
        else:
            del s[int(rng.integers(0, len(s)))]
    return np.array(s, dtype=np.uint8)


def _set_of(rows, v, j, rng, prefix, nucleotides):
    n = len(rows)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    rep = rng.integers(0, 3, size=n, dtype=np.uint32)
    rep[:3] = np.arange(3)                                     # (numbered in order of first appearance)
    return RepertoireSet(np.concatenate(rows).astype(np.uint8), off, np.array(v, dtype=np.uint32),
                         np.array(j, dtype=np.uint32), rep, rng.integers(1, 6, size=n, dtype=np.uint64),
                         [prefix + str(k + 1) for k in range(3)], ["V%d" % k for k in range(N_V)],
                         ["J%d" % k for k in range(N_J)], NT if nucleotides else AA)


@functools.lru_cache(maxsize=None)
def families(nucleotides):
    """(set 1, set 2, family 1, family 2): per sequence the ancestor length of its family.  5 V x 3 J genes, three
    repertoires, counts 1 .. 5, each set shuffled."""
    A = 4 if nucleotides else 20
    rng = np.random.default_rng(SEED[nucleotides])
    sets = []
    ancestors = [(n, rng.integers(0, A, size=n, dtype=np.uint8), ORDINARY_VJ[int(rng.integers(0, len(ORDINARY_VJ)))])
                 for n in ANCESTORS[nucleotides]]
    for which in (1, 2):
        rows, genes, fam = [], [], []
        for n, base, vj in ancestors:
            for m in range(DESCENDANTS):
                row = mutated(base, m % 7, A, rng)
                own = vj if rng.random() >= 0.15 else ORDINARY_VJ[int(rng.integers(0, len(ORDINARY_VJ)))]
                if n == PARTNERLESS[nucleotides] and which == 1:
                    own = PARTNERLESS_VJ
                if n == FAR[nucleotides] and which == 2 and m % 3 == 0:
                    own = PARTNERLESS_VJ
                if n == KEYMISS[nucleotides] and (which == 1 or len(row) != n):
                    own = KEYMISS_VJ
                rows.append(row)
                genes.append(own)
                fam.append(n)
        order = rng.permutation(len(rows))
        s = _set_of([rows[k] for k in order], [genes[k][0] for k in order], [genes[k][1] for k in order], rng,
                    "AB"[which - 1], nucleotides)
        sets.append((s, np.array(fam)[order]))
    return sets[0][0], sets[1][0], sets[0][1], sets[1][1]


def family_sets(nucleotides):
    return families(nucleotides)[:2]


def family_options(nucleotides, ignore_genes, **more):
    return Options(n_v_genes=N_V, n_j_genes=N_J, nucleotides=nucleotides, ignore_genes=ignore_genes, **more)


def family_kw(nucleotides, ignore_genes):
    return dict(n_v_genes=N_V, n_j_genes=N_J, nucleotides=nucleotides, ignore_genes=ignore_genes)


@functools.lru_cache(maxsize=None)
def family_want(nucleotides, d, ignore_genes):
    s1, s2 = family_sets(nucleotides)
    return _edit.brute_csr(s1, s2, d, ignore_genes)


@functools.lru_cache(maxsize=None)
def family_union(nucleotides):
    """both family sets as one: set 1's sequences, then set 2's"""
    s1, s2 = family_sets(nucleotides)
    return _edit_cluster.joined(s1, s2)


@functools.lru_cache(maxsize=None)
def family_distances(nucleotides, one_set=False):
    """every distance of set 1 to set 2 (one_set: to itself), for the nearest-neighbour brute force; read-only"""
    s1, s2 = family_sets(nucleotides)
    return _edit_nearest.all_distances(s1, s1 if one_set else s2)


@functools.lru_cache(maxsize=None)
def union_want(nucleotides, d, ignore_genes):
    """(label, size, clusters) of family_union by the yardstick, numbered as _edit_cluster.want numbers them: the
    connected components of the brute force's pair list, each labelled with its smallest number"""
    s = family_union(nucleotides)
    rows, hits, _ = _edit.brute_csr(s, s, d, ignore_genes)
    label = _cluster.labels_of_pairs(s.n, _edit.queries_of(rows), hits)
    size = _cluster.sizes_of_labels(label)
    label.setflags(write=False)
    size.setflags(write=False)
    return label, size, int((label == np.arange(s.n)).sum())


def carries(s, vj):
    """bool[n]: which sequences of s have that (V, J)"""
    return (s.v_gene == vj[0]) & (s.j_gene == vj[1])


# ---- input B: every distance at every word count ----

DISTANCE_LENGTHS = (1, 2, 8, 9, 16, 17, 32, 33, 63, 64, 65, 100, 127, 128, 129, 200, 255, 256)
DISTANCE_SEEDS = (5301, 5302)
DISTANCE_D = 256


@functools.lru_cache(maxsize=None)
def distance_sets(nucleotides):
    """per length of DISTANCE_LENGTHS a random sequence, a homopolymer, a period-3 repeat and the random one rotated
    by one residue; one V, one J, two repertoires, counts 1 .. 5"""
    A = 4 if nucleotides else 20
    out = []
    for seed, prefix in zip(DISTANCE_SEEDS, "CD"):
        rng = np.random.default_rng(seed + A)
        rows = []
        for n in DISTANCE_LENGTHS:
            random = rng.integers(0, A, size=n, dtype=np.uint8)
            rows += [random, np.full(n, rng.integers(0, A), dtype=np.uint8),
                     np.resize(rng.integers(0, A, size=3, dtype=np.uint8), n), np.roll(random, 1)]
        n = len(rows)
        off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum([len(r) for r in rows], out=off[1:])
        out.append(RepertoireSet(np.concatenate(rows).astype(np.uint8), off, np.zeros(n, dtype=np.uint32),
                                 np.zeros(n, dtype=np.uint32), (np.arange(n) % 2).astype(np.uint32),
                                 rng.integers(1, 6, size=n, dtype=np.uint64), [prefix + "1", prefix + "2"], ["V0"],
                                 ["J0"], NT if nucleotides else AA))
    return tuple(out)


def distance_options(nucleotides, **more):
    return Options(n_v_genes=1, n_j_genes=1, nucleotides=nucleotides, ignore_genes=True, **more)


@functools.lru_cache(maxsize=None)
def distance_want(nucleotides, d=DISTANCE_D):
    s1, s2 = distance_sets(nucleotides)
    return _edit.brute_csr(s1, s2, d, True)


# ---- helpers ----

def swapped(set1, set2, want):
    """the pair list of (set2, set1) from that of (set1, set2): the distance is symmetric, so every edge (i, j, dd) is
    the edge (j, i, dd) of the swapped call; rows by the hit again"""
    rows, hits, dist = want
    q, h = _edit.queries_of(rows), np.asarray(hits).astype(np.int64)
    order = np.lexsort((q, h))
    new_rows = np.zeros(set2.n + 1, dtype=np.uint64)
    np.cumsum(np.bincount(h, minlength=set2.n), out=new_rows[1:])
    return new_rows, q[order].astype(np.uint32), np.asarray(dist)[order]


def differences_of(got, want, set1, set2, nucleotides, limit=8):
    """a failing comparison in words: the first edges that one pair list has and the other lacks or has at another
    distance, each with the query's length and form and the hit's length and column words"""
    def edges(csr):
        q, h = _edit.queries_of(csr[0]), np.asarray(csr[1]).astype(np.int64)
        return {(int(a), int(b)): int(c) for a, b, c in zip(q, h, csr[2])}
    try:
        g, w = edges(got), edges(want)
    except Exception as e:                                             # (not even a CSR)
        return "malformed result: %r" % e
    lines = []
    for q, h in sorted(set(g) | set(w)):
        if g.get((q, h)) != w.get((q, h)):
            n1, n2 = int(set1.lengths[q]), int(set2.lengths[h])
            lines.append("query %d (%d residues, NW = %d) hit %d (%d residues, W = %d): got %s, want %s"
                         % (q, n1, form_of(n1, nucleotides), h, n2, 1 if n2 <= 64 else 2 if n2 <= 128 else 4,
                            g.get((q, h)), w.get((q, h))))
    return "%d edges differ (got %d, want %d)\n" % (len(lines), len(g), len(w)) + "\n".join(lines[:limit])


def wagner_fischer(a, b):
    """the Levenshtein distance of two sequences by the scalar textbook DP, in plain Python integers"""
    a, b = [int(x) for x in a], [int(x) for x in b]
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        row = [i]
        for j, y in enumerate(b, 1):
            row.append(min(prev[j] + 1, row[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = row
    return prev[len(b)]


def sequence_of(s, i):
    return s.residues[int(s.offsets[i]):int(s.offsets[i + 1])]


def edges_by_form(set1, set2, want, nucleotides):
    """({form: edges of its queries}, edges whose query and hit have different forms, {crossing: edges across it})"""
    rows, hits, _ = want
    len1 = set1.lengths[_edit.queries_of(rows)]
    len2 = set2.lengths[np.asarray(hits).astype(np.int64)]
    f1, f2 = forms_of(len1, nucleotides), forms_of(len2, nucleotides)
    lo, hi = np.minimum(len1, len2), np.maximum(len1, len2)
    return ({f: int((f1 == f).sum()) for f in ALL_FORMS[nucleotides]}, int((f1 != f2).sum()),
            {c: int(((lo <= c) & (hi > c)).sum()) for c in CROSSINGS[nucleotides]})


def figures_of(set1, set2, want, d):
    """(edges, histogram of the distances, edges across two lengths, longest row)"""
    rows, hits, dist = want
    deg = np.diff(rows.astype(np.int64))
    return len(hits), _edit.histogram(dist, d), _edit.cross_length(set1, set2, rows, hits), int(deg.max())


# (nucleotides, d, ignore_genes): (edges, histogram, edges across two lengths, longest row), from the brute force
FAMILY_FIGURES = {
    (False, 1, False): (230, [70, 160], 99, 5),
    (False, 1, True): (338, [106, 232], 148, 6),
    (False, 2, False): (475, [70, 160, 245], 268, 8),
    (False, 2, True): (695, [106, 232, 357], 392, 8),
    (False, 3, False): (740, [70, 160, 245, 265], 462, 8),
    (False, 3, True): (1_092, [106, 232, 357, 397], 687, 9),
    (False, 6, False): (1_549, [70, 160, 245, 265, 276, 281, 252], 1_096, 14),
    (False, 6, True): (2_404, [106, 232, 357, 397, 400, 434, 478], 1_723, 28),
    (True, 1, False): (141, [45, 96], 50, 4),
    (True, 1, True): (204, [65, 139], 80, 4),
    (True, 2, False): (285, [45, 96, 144], 146, 6),
    (True, 2, True): (411, [65, 139, 207], 224, 7),
    (True, 3, False): (436, [45, 96, 144, 151], 254, 9),
    (True, 3, True): (638, [65, 139, 207, 227], 389, 9),
    (True, 6, False): (914, [45, 96, 144, 151, 171, 168, 139], 640, 10),
    (True, 6, True): (1_315, [65, 139, 207, 227, 247, 232, 198], 937, 10),
}
FAMILY_KEYS = list(FAMILY_FIGURES)
FAMILY_IDS = ["%s-d%d%s" % ("nt" if k[0] else "aa", k[1], "-g" if k[2] else "") for k in FAMILY_KEYS]
# at d = 6 with ignore_genes: ({form: edges of its queries}, edges between two forms, {crossing: edges across it})
FORM_FIGURES = {
    False: ({2: 519, 4: 610, 8: 729, 16: 453, 0: 93}, 328, {8: 117, 16: 95, 32: 75, 64: 41}),
    True: ({2: 433, 4: 655, 0: 227}, 159, {32: 63, 64: 96}),
}
# input B at d = 256: (edges, largest distance, distances above 128, above 64, distinct distances)
DISTANCE_FIGURES = {False: (5_184, 256, 1_700, 3_334, 202), True: (5_184, 256, 1_561, 3_205, 238)}
