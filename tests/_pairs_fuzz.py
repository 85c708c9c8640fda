"""The randomised parity sweep of the all-against-all calls (cmpr_hamming_*, cmpr_edit_*, cmpr_tcrdist_*): the
generator of its cases, their expectations from the yardsticks of tests/_hamming.py, _edit.py, _tcrdist.py, _nearest.py,
_edit_nearest.py and _cluster.py, and the coverage tags that prove a sweep is not vacuous (test infrastructure).
Nothing here calls the library under test: tests/_pairs_fuzz_call.py makes the calls and compares.

case(seed, index) is deterministic in (seed, index) alone -- every case has its own np.random.default_rng([seed, index])
-- so any case is replayed alone: `python tests/fuzz_pairs_gpu.py --seed S --case K`.

The caps that keep a yardstick cheap (cost(): the elementary steps of the case's brute force):
  Hamming   sum over the shared lengths L of n1(L) x n2(L) x (L + 1)                        <= CAPS["hamming"]
  edit      sum over the pairs of lengths the brute force walks -- |L1 - L2| <= d for neighbors, matrix and clusters,
            every pair for nearest, capped or not -- of n1(L1) x n2(L2) x (L1 + 1) x (L2 + 1)  <= CAPS["edit"]
            (uncapped nearest at 200 x 183 sequences of up to 256 residues took 27 s; the cap allows some two dozen
            sequences of 256 residues a set, or a few hundred of a dozen residues)
  TCRdist   sum over the pairs of lengths with |L1 - L2| x gap_penalty <= cutoff of
            n1(L1) x n2(L2) x (min(L1, L2) + 1)                                             <= CAPS["tcrdist"]
and a set has at most MAX_N sequences.  A case above its cap loses sequences of the most expensive length until it
fits."""

import hashlib
import types

import numpy as np

import _cluster
import _cluster_table
import _edit
import _edit_forms
import _edit_nearest
import _hamming
import _nearest
import _tcrdist
from compairr_amd import Options, RepertoireSet
from compairr_amd.sets import AA, NT

SLICE_SEEDS = (20261021, 27)               # the committed slice: tests/test_pairs_fuzz_gpu.py, proven in _cpu.py
SLICE_CASES = 96                           # per seed
CHUNK = 16                                 # cases per pytest item of the slice

# (metric, result kind): five each under Hamming and edit distance, two under TCRdist -- twelve, dealt in turn
COMBOS = ([(m, k) for m in ("hamming", "edit") for k in ("neighbors", "matrix", "cluster", "cluster_table", "nearest")]
          + [("tcrdist", "neighbors"), ("tcrdist", "matrix")])
CAPS = {"hamming": 60_000_000, "edit": 30_000_000, "tcrdist": 20_000_000}
MAX_N = 1200

EDGE_LENGTHS = (0, 1, 2, 3, 4, 5, 6, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256)
HAMMING_LENGTHS = (96, 97, 200, 1000)
GENES = ((1, 1), (2, 2), (3, 2), (60, 13))
REPERTOIRES = (1, 2, 3, 32, 33)
GROWN = (1, 63, 64, 65, 255, 256, 257)     # a tile, a workgroup; beyond: more than one staged piece
STAGE_REFS = (0, 1, 2, 63, 64, 65, 511, 512, 513)
SEGMENTS = (0, 1, 2, 3, 7, 64)
SCORES = ("product", "min", "max", "mean")
FIXED, SLIDING = _tcrdist.FIXED, _tcrdist.SLIDING

# what the kernels divide by (compairr_amd/csrc/allpairs.h, hamming.hip, edit.hip, tcrdist.hip), for the tags only
PAIRS_WG, PAIRS_STAGE_MAX, PAIRS_MAT_CELLS, LONG_ROW = 256, 512, 1024, 64
HM_LDS_WORDS, ED_PEQ_WORDS, TD_STAGE_WORDS = 4096, 2048, 4096

TAGS = ("multi-workgroup job", "several pieces", "row > 64", "matrix > 1024 cells", "one-file mode", "empty set 1",
        "empty set 2", "empty sequences", "partnerless group")


def combo_of(seed, index):
    return COMBOS[(seed + index) % len(COMBOS)]


# ---- the generator ----

def _mutated(row, ops, letters, indels, max_len, rng):
    """`row` after `ops` operations: substitutions to another of `letters`, and with `indels` insertions and
    deletions too (an empty sequence takes an insertion; none grows beyond max_len)"""
    s = row.tolist()
    for _ in range(ops):
        kind = int(rng.integers(0, 3)) if indels else 0
        if not s:
            kind = 1 if indels else -1
        if kind == 1 and len(s) >= max_len:
            kind = 2
        if kind == 0:
            p = int(rng.integers(0, len(s)))
            other = [x for x in letters if x != s[p]]
            s[p] = other[int(rng.integers(0, len(other)))]
        elif kind == 1:
            s.insert(int(rng.integers(0, len(s) + 1)), letters[int(rng.integers(0, len(letters)))])
        elif kind == 2:
            del s[int(rng.integers(0, len(s)))]
    return np.array(s, dtype=np.uint8)


def _unit(metric, L1, L2):
    if metric == "hamming":
        return L1 + 1
    if metric == "edit":
        return (L1 + 1) * (L2 + 1)
    return min(L1, L2) + 1


def _walked(c, L1, L2):
    """whether the case's brute force compares sequences of these two lengths"""
    gap = abs(L1 - L2)
    if c.metric == "hamming":
        return gap == 0
    if c.metric == "edit":
        return c.kind == "nearest" or gap <= c.differences
    return gap * c.gap_penalty <= c.cutoff


def _cost_of(c, len1, len2):
    u1, n1 = np.unique(np.asarray(len1, dtype=np.int64), return_counts=True)
    u2, n2 = np.unique(np.asarray(len2, dtype=np.int64), return_counts=True)
    total, per_length = 0, {}
    for L1, a in zip(u1.tolist(), n1.tolist()):
        for L2, b in zip(u2.tolist(), n2.tolist()):
            if _walked(c, L1, L2):
                x = a * b * _unit(c.metric, L1, L2)
                total += x
                per_length[L1] = per_length.get(L1, 0) + x
                per_length[L2] = per_length.get(L2, 0) + x
    return total, per_length


def cost(c):
    """the elementary steps of the case's brute force (see the module docstring)"""
    return _cost_of(c, c.set1.lengths, c.set2.lengths)[0]


def _set_of(rows, genes, n_rep, n_v, n_j, prefix, nucleotides, big_counts, rng):
    n = len(rows)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    res = np.concatenate(rows).astype(np.uint8) if n and off[-1] else np.zeros(0, dtype=np.uint8)
    count = rng.integers(1, 10, size=n, dtype=np.uint64)
    if big_counts and n:                                               # near 2^63: the sums wrap
        where = rng.random(n) < 0.3
        where[int(rng.integers(0, n))] = True
        count[where] = (np.uint64(1) << np.uint64(63)) - np.uint64(4) + rng.integers(0, 9, size=int(where.sum()),
                                                                                    dtype=np.uint64)
    v = np.array([g[0] for g in genes], dtype=np.uint32)
    j = np.array([g[1] for g in genes], dtype=np.uint32)
    return RepertoireSet(res, off, v, j, rng.integers(0, n_rep, size=n, dtype=np.uint32), count,
                         ["%s%d" % (prefix, k + 1) for k in range(n_rep)], ["V%d" % k for k in range(n_v)],
                         ["J%d" % k for k in range(n_j)], NT if nucleotides else AA)


def _pick(rng, values, weights=None):
    if weights is None:
        return values[int(rng.integers(0, len(values)))]
    w = np.asarray(weights, dtype=np.float64)
    return values[int(rng.choice(len(values), p=w / w.sum()))]


def _tunables(c, rng, often):
    """a setting of the family's tunables: each with probability `often`"""
    prefix, t = c.metric, {}
    if rng.random() < often:
        t[prefix + "_stage_refs"] = int(_pick(rng, STAGE_REFS))
    if rng.random() < often:
        t[prefix + "_segments"] = int(_pick(rng, SEGMENTS))
    if c.metric == "hamming" and rng.random() < often:
        t["hamming_generic"] = int(rng.integers(0, 2))
    if c.metric != "tcrdist" and c.kind in ("cluster", "cluster_table") and rng.random() < often:
        t[prefix + "_link_snapshot"] = int(rng.integers(0, 2))
    if c.metric == "edit" and rng.random() < often:
        t["edit_words"] = int(_pick(rng, (0, 2, 4)))
    if c.metric == "edit" and c.kind == "nearest" and rng.random() < max(often, 0.5):
        t["edit_nearest_prune"] = int(rng.integers(0, 2))
    return t


def _tables(c, rng):
    """the substitution table and, in a share of the cases with genes, the V table"""
    which = _pick(rng, ("table", "asymmetric", "unit", "cells255"))
    if which == "table":
        W = _tcrdist.table().copy()
    elif which == "asymmetric":
        W = rng.integers(0, 7, (20, 20)).astype(np.uint8)
        diag = np.where(rng.random(20) < 0.8, 0, rng.integers(1, 4, 20)).astype(np.uint8)
        W[np.arange(20), np.arange(20)] = diag
    elif which == "unit":
        W = (1 - np.eye(20, dtype=np.uint8)).astype(np.uint8)
    else:
        W = _tcrdist.table().copy()
        for _ in range(6):
            a, b = int(rng.integers(0, 20)), int(rng.integers(0, 20))
            if a != b:
                W[a, b] = 255
    c.table_kind, c.W = which, np.ascontiguousarray(W, dtype=np.uint8)
    c.V = None
    if not c.ignore_genes and rng.random() < 0.5:
        n = c.n_v
        V = rng.integers(0, 1 + max(1, min(c.cutoff, 24) // 2), (n, n)).astype(np.int64)
        V[np.arange(n), np.arange(n)] = np.where(rng.random(n) < 0.8, 0, V[np.arange(n), np.arange(n)])
        if n > 1:
            above = (rng.random((n, n)) < 0.2) & ~np.eye(n, dtype=bool)
            V[above] = np.minimum(65535, c.cutoff + 1 + rng.integers(0, 50, (n, n)))[above]
            a = int(rng.integers(0, n))
            V[a, (a + 1 + int(rng.integers(0, n - 1))) % n] = 65535
        c.V = np.ascontiguousarray(V, dtype=np.uint16)


def case(seed, index):
    """one fully described case (a namespace): metric and kind, the two sets, the call's arguments, the options, two
    settings of the tunables (the second for the cases that repeat the call under another one) and how it is called"""
    rng = np.random.default_rng([seed, index])
    c = types.SimpleNamespace(seed=seed, index=index)
    c.metric, c.kind = combo_of(seed, index)
    c.nucleotides = c.metric != "tcrdist" and rng.random() < 0.4
    A = 4 if c.nucleotides else 20
    max_len = 65535 if c.metric == "hamming" else _edit.MAX_LEN
    indels = c.metric != "hamming"
    n_letters = A if rng.random() < 0.5 else int(rng.integers(2, 5))
    letters = rng.permutation(A)[:n_letters].tolist()
    c.letters = n_letters
    c.n_v, c.n_j = _pick(rng, GENES)
    c.ignore_genes = bool(rng.random() < 0.3)
    c.one_set = c.kind in ("cluster", "cluster_table") or bool(rng.random() < (0.45 if c.kind == "nearest" else 0.2))
    c.n_rep1 = int(_pick(rng, REPERTOIRES))
    c.n_rep2 = c.n_rep1 if c.one_set or rng.random() < 0.6 else int(_pick(rng, REPERTOIRES))
    special = rng.random()
    c.special = ("empty set 1" if special < 0.02 else "empty set 2" if special < 0.04 and not c.one_set else
                 "only empty sequences" if special < 0.07 else "")
    c.big_counts = bool(rng.random() < 0.12)

    # ---- the families ----
    lengths = list(EDGE_LENGTHS)
    if c.metric == "hamming":
        bound = _hamming.REG_BOUND[c.nucleotides]
        lengths += list(HAMMING_LENGTHS) + [bound, bound + 1]
    short = [n for n in lengths if n <= (6 if indels else 33)]
    n_anc = int(rng.integers(3, 8))
    anc_lengths = [int(_pick(rng, lengths)) for _ in range(n_anc)]
    # (a length that carries edges of its own form; the lengths of the list's middle come up too seldom otherwise)
    anc_lengths[0] = int(_pick(rng, (4, 8, 12, 16, 24, 32, 40, 64, 65, 100)))
    rows = ([], [])                        # per set: (residues, (V, J))
    only_set1 = int(rng.integers(0, n_anc)) if rng.random() < 0.35 else -1     # a family without partners
    k_max = int(_pick(rng, (1, 2, 3, 6)))
    per_family = int(_pick(rng, (4, 8, 12, 20)))
    for a, L in enumerate(anc_lengths):
        base = np.array([letters[int(x)] for x in rng.integers(0, n_letters, size=L)], dtype=np.uint8)
        vj = (int(rng.integers(0, c.n_v)), int(rng.integers(0, c.n_j)))
        m = per_family if L <= 70 else max(2, per_family // (2 if L <= 130 else 4))
        for which in ((0,) if c.one_set or a == only_set1 else (0, 1)):
            rows[which].append((base, vj))                             # (the ancestor itself: a pair at distance 0)
        for k in range(m):
            row = _mutated(base, int(rng.integers(0, k_max + 1)), letters, indels, max_len, rng)
            own = vj if rng.random() >= 0.15 else (int(rng.integers(0, c.n_v)), int(rng.integers(0, c.n_j)))
            which = 0 if c.one_set or a == only_set1 else int(rng.integers(0, 2))
            rows[which].append((row, own))
        # one residue lost at the front, lost near the end and gained near the end: pairs of two lengths whose best
        # alignment has its gap at an end (TCRdist: at or beyond the last gap position tried)
        for kind in (("front", "back", "gain") if indels and L >= 2 else ()):
            s = base.tolist()
            p = int(rng.integers(max(0, L - 6), L))
            if kind == "front":
                del s[int(rng.integers(0, min(3, L)))]
            elif kind == "back":
                del s[p]
            elif L < max_len:
                s.insert(p + 1, letters[int(rng.integers(0, n_letters))])
            which = 0 if c.one_set or a == only_set1 else int(rng.integers(0, 2))
            rows[which].append((np.array(s, dtype=np.uint8), vj))
    # one family grown to the sizes the kernels divide by: substitutions only, genes inherited -- one group a set
    grown = [int(_pick(rng, GROWN + (int(rng.integers(300, 420)),), (2, 1, 1, 1, 1, 1, 1, 2))) for _ in range(2)]
    L = int(_pick(rng, short[1:] if len(short) > 1 else short))
    if max(grown) > 257:
        L = min(L, 6 if indels else 17)
    base = np.array([letters[int(x)] for x in rng.integers(0, n_letters, size=L)], dtype=np.uint8)
    vj = (int(rng.integers(0, c.n_v)), int(rng.integers(0, c.n_j)))
    for which in ((0,) if c.one_set else (0, 1)):
        for k in range(grown[which]):
            rows[which].append((_mutated(base, int(rng.integers(0, min(k_max, 3) + 1)), letters, False, max_len, rng), vj))
    c.grown, c.grown_length = tuple(grown[:1 if c.one_set else 2]), L
    # unrelated filler, empty sequences now and then, and exact duplicates
    for which in ((0,) if c.one_set else (0, 1)):
        for _ in range(int(rng.integers(0, 12))):
            n = int(rng.integers(0, 21))
            row = np.array([letters[int(x)] for x in rng.integers(0, n_letters, size=n)], dtype=np.uint8)
            rows[which].append((row, (int(rng.integers(0, c.n_v)), int(rng.integers(0, c.n_j)))))
        for _ in range(int(rng.integers(0, 6))):
            src = rows[int(rng.integers(0, 2))] if not c.one_set else rows[0]
            if src:
                rows[which].append(src[int(rng.integers(0, len(src)))])
    if c.special == "only empty sequences":
        which = 0 if c.one_set else int(rng.integers(0, 2))
        rows[which][:] = [(np.zeros(0, dtype=np.uint8), g) for _, g in rows[which][:int(rng.integers(1, 70))]]
    if c.special == "empty set 1":
        rows[0].clear()
    if c.special == "empty set 2":
        rows[1].clear()

    # ---- the call's arguments ----
    longest = max([len(r) for r, _ in rows[0] + rows[1]] + [0])
    c.differences = c.floor = c.cap = None
    c.other_repertoire = False
    if c.kind == "nearest":
        c.floor = int(_pick(rng, (0, 1, 2), (3, 4, 2)))
        if c.metric == "edit":
            c.cap = _pick(rng, (None, 0, 1, 3), (3, 3, 2, 3))
            if c.cap is not None and c.cap < c.floor and rng.random() < 0.6:
                c.floor = 0                                            # (floor > cap finds nobody: valid, kept rare)
        c.other_repertoire = bool(c.one_set and c.n_rep1 > 1 and rng.random() < 0.5)
    elif c.metric != "tcrdist":
        c.differences = int(_pick(rng, (0, 1, 2, 3, 6, longest, longest + 5), (2, 3, 3, 3, 3, 1, 1)))
    if c.metric == "tcrdist":
        c.ntrim, c.ctrim = int(rng.integers(0, 5)), int(rng.integers(0, 5))
        c.gap_penalty = int(_pick(rng, (0, 1, 4, 12)))
        c.gap_mode = int(_pick(rng, (FIXED, SLIDING)))
        c.cutoff = int(_pick(rng, (0, int(rng.integers(3, 13)), int(rng.integers(30, 121)), 65535), (2, 4, 3, 1)))
        _tables(c, rng)

    # ---- the caps: sequences of the most expensive length leave until the brute force is cheap ----
    def lens(which):
        return [len(r) for r, _ in rows[which]]
    for which in (0, 1):
        del rows[which][MAX_N:]
    while True:
        total, per_length = _cost_of(c, lens(0), lens(0 if c.one_set else 1))
        if total <= CAPS[c.metric]:
            break
        worst = max(per_length, key=lambda n: (per_length[n], n))
        which = max((0,) if c.one_set else (0, 1), key=lambda w: sum(1 for n in lens(w) if n == worst))
        members = [k for k, n in enumerate(lens(which)) if n == worst]
        for k in reversed(members[len(members) - max(1, len(members) // 4):]):
            del rows[which][k]

    # ---- the sets ----
    sets = []
    for which in ((0,) if c.one_set else (0, 1)):
        order = rng.permutation(len(rows[which])).tolist()
        sets.append(_set_of([rows[which][k][0] for k in order], [rows[which][k][1] for k in order],
                            (c.n_rep1, c.n_rep2)[which], c.n_v, c.n_j, "AB"[which], c.nucleotides, c.big_counts, rng))
    c.set1 = sets[0]
    c.set2 = sets[0] if c.one_set else sets[1]

    # ---- options, tunables, how it is called ----
    zero = c.differences == 0 or (c.metric == "tcrdist" and c.cutoff == 0)
    c.ignore_counts = bool(rng.random() < 0.25)
    c.existence = bool(c.kind in ("matrix", "neighbors", "nearest") and rng.random() < (0.3 if c.kind == "matrix" else 0.1))
    index_score = zero and not c.existence and c.kind != "nearest" and rng.random() < 0.5
    c.score = str(_pick(rng, ("mh", "jaccard") if index_score else SCORES))
    c.tunables = _tunables(c, rng, 0.35)
    c.tunables2 = _tunables(c, rng, 0.6)
    c.entry = "device" if rng.random() < 0.5 else "host"
    c.capacity = str(_pick(rng, ("exact", "short", "generous"))) if c.kind == "neighbors" else ""
    return c


DRAWN = ("seed", "index", "metric", "kind", "nucleotides", "letters", "n_v", "n_j", "ignore_genes", "one_set", "n_rep1",
         "n_rep2", "special", "big_counts", "grown", "grown_length", "differences", "floor", "cap", "other_repertoire",
         "ntrim", "ctrim", "gap_penalty", "gap_mode", "cutoff", "table_kind", "ignore_counts", "existence", "score",
         "tunables", "tunables2", "entry", "capacity")


def describe(c):
    """the case in full: every drawn value and the sizes of the sets"""
    drawn = ", ".join("%s=%r" % (k, getattr(c, k)) for k in DRAWN if hasattr(c, k))
    sizes = "n1=%d n2=%d longest=%d/%d lengths1=%s" % (c.set1.n, c.set2.n, c.set1.longest, c.set2.longest,
                                                      sorted(set(c.set1.lengths.tolist())))
    v = "" if getattr(c, "V", None) is None else " V table %dx%d" % c.V.shape
    return "%s\n  %s%s\n  replay: %s" % (drawn, sizes, v, replay(c))


def replay(c):
    return "python tests/fuzz_pairs_gpu.py --seed %d --case %d" % (c.seed, c.index)


def fingerprint(c):
    """a digest of everything the case holds: two builds of one case agree in it byte for byte"""
    h = hashlib.sha256(", ".join("%s=%r" % (k, getattr(c, k)) for k in DRAWN if hasattr(c, k)).encode())
    for s in (c.set1, c.set2):
        for a in (s.residues, s.offsets, s.v_gene, s.j_gene, s.repertoire, s.count):
            h.update(a.tobytes())
        h.update(repr((s.repertoire_ids, s.v_names, s.j_names, s.alphabet)).encode())
    for name in ("W", "V"):
        a = getattr(c, name, None)
        h.update(b"-" if a is None else a.tobytes())
    return h.hexdigest()


def options_of(c, **more):
    return Options(n_v_genes=c.n_v, n_j_genes=c.n_j, nucleotides=c.nucleotides, ignore_genes=c.ignore_genes,
                   ignore_counts=c.ignore_counts, existence=c.existence, score=c.score, **more)


# ---- the expectation ----

def pair_list(c):
    """(row_start, hits, distance) of the case's pair relation by the metric's brute force; None for nearest"""
    s1, s2 = c.set1, c.set2
    if c.kind == "nearest":
        return None
    if c.metric == "hamming":
        return _hamming.brute_csr(s1, s2, c.differences, c.ignore_genes)
    if c.metric == "edit":
        return _edit.brute_csr(s1, s2, c.differences, c.ignore_genes)
    return _tcrdist.brute_csr(s1, s2, c.W, c.ntrim, c.ctrim, c.gap_penalty, c.gap_mode, c.cutoff, c.ignore_genes, c.V)


def expect(c):
    """a namespace: `pairs` -- the brute force's pair list, None for nearest -- and what the call must give:
    neighbors `pairs` itself; matrix `matrix`; cluster and cluster_table `label` and `table`; nearest `nearest`, the
    three arrays, and `n_found`"""
    want = types.SimpleNamespace(pairs=pair_list(c))
    s1, s2 = c.set1, c.set2
    if c.kind == "matrix":
        want.matrix = _edit.matrix_of(s1, s2, want.pairs[0], want.pairs[1], options_of(c))
    elif c.kind in ("cluster", "cluster_table"):
        want.label = _cluster.labels_of_pairs(s1.n, _edit.queries_of(want.pairs[0]), want.pairs[1])
        want.table = _cluster_table.table_of(want.label, np.ones(s1.n, dtype=np.uint64) if c.ignore_counts else s1.count)
    elif c.kind == "nearest":
        if c.metric == "hamming":
            want.nearest = _nearest.brute(s1, s2, c.ignore_genes, c.floor, c.other_repertoire)
        else:
            want.nearest = _edit_nearest.brute(s1, s2, c.ignore_genes, c.floor, c.cap, c.other_repertoire)
        want.n_found = int((want.nearest[2] > 0).sum())
    return want


# ---- the coverage tags ----

def _groups(c, s, with_j):
    """{(length, V, J): sequences} of a set as the call groups it"""
    length = s.lengths.astype(np.int64)
    zero = np.zeros(s.n, dtype=np.int64)
    v = zero if c.ignore_genes else s.v_gene.astype(np.int64)
    j = zero if c.ignore_genes or not with_j else s.j_gene.astype(np.int64)
    keys, counts = np.unique(np.stack([length, v, j], axis=1), axis=0, return_counts=True) if s.n else ((), ())
    return {tuple(int(x) for x in k): int(n) for k, n in zip(keys, counts)}


def _piece(c, tunables, length):
    """references of a staged piece of a set-2 group of `length` residues: pairs_piece of allpairs.h"""
    per_word = _edit_forms.PER_WORD[c.nucleotides]
    words = max(1, -(-length // per_word))
    stride = next((f for f in _edit_forms.STRIDES if words <= f), words)
    if c.metric == "hamming":
        fit = HM_LDS_WORDS // stride
    elif c.metric == "edit":
        w = max(1 if length <= 64 else 2 if length <= 128 else 4, tunables.get("edit_words", 0))
        fit = ED_PEQ_WORDS // ((4 if c.nucleotides else 20) * w)
    else:
        fit = TD_STAGE_WORDS // stride
    R = max(1, min(fit, PAIRS_STAGE_MAX))
    staged = tunables.get(c.metric + "_stage_refs", 0)
    return staged if 1 <= staged < R else R


def _partners(c):
    """per set-1 group: (its size, [(length, size) of its partner groups in set 2])"""
    v_table = c.metric == "tcrdist" and c.V is not None
    g1, g2 = _groups(c, c.set1, not v_table), _groups(c, c.set2, not v_table)
    out = []
    for (L1, v1, j1), n1 in g1.items():
        mine = []
        for (L2, v2, j2), n2 in g2.items():
            gap = abs(L1 - L2)
            if c.metric == "tcrdist":
                base = gap * c.gap_penalty + (int(c.V[v1, v2]) if v_table else 0)
                ok = base <= c.cutoff and (v_table or (v1, j1) == (v2, j2))
            else:
                limit = 0 if c.metric == "hamming" else c.differences if c.kind != "nearest" else \
                    (1 << 30) if c.cap is None else c.cap
                ok = gap <= limit and (v1, j1) == (v2, j2)
            if ok:
                mine.append((L2, n2))
        out.append((n1, mine))
    return out


def classify(c, want):
    """the case's coverage tags, a set of strings: "vacuous", "cross-length", "form N" (the register form of a query
    that carries an edge; edit and TCRdist), "hamming register" / "hamming generic" (the side of REG_BOUND of a length
    that carries an edge) and those of TAGS"""
    tags = set()
    s1, s2 = c.set1, c.set2
    if want.pairs is not None:
        q, h = _edit.queries_of(want.pairs[0]), np.asarray(want.pairs[1]).astype(np.int64)
        off = q != h
        q, h = q[off], h[off]                                          # (the edges outside (i, i))
        len_q, len_h = s1.lengths[q], s2.lengths[h]
        if c.kind == "matrix":
            vacuous = not want.matrix.any()
        elif c.kind in ("cluster", "cluster_table"):
            vacuous = bool((want.label == np.arange(s1.n)).all())
        else:
            vacuous = len(q) == 0
        if len(np.asarray(want.pairs[1])) and np.diff(want.pairs[0].astype(np.int64)).max() > LONG_ROW:
            tags.add("row > 64")
    else:
        found = want.nearest[2] > 0
        q, h = np.nonzero(found)[0], want.nearest[0][found].astype(np.int64)
        len_q, len_h = s1.lengths[q], s2.lengths[h]
        vacuous = not found.any()
    if vacuous:
        tags.add("vacuous")
    if c.metric != "hamming":
        if (len_q != len_h).any():
            tags.add("cross-length")
        for f in set(_edit_forms.forms_of(np.unique(len_q), c.nucleotides).tolist()):
            tags.add("form %d" % f)
    elif len(len_q):
        bound = _hamming.REG_BOUND[c.nucleotides]
        if (len_q <= bound).any():
            tags.add("hamming register")
        if (len_q > bound).any():
            tags.add("hamming generic")
    partners = _partners(c)
    if s1.n and s2.n and any(not mine for _, mine in partners):
        tags.add("partnerless group")
    if any(n1 > PAIRS_WG and mine for n1, mine in partners):
        tags.add("multi-workgroup job")
    largest = max([n for _, mine in partners for _, n in mine] + [0])
    segments = c.tunables.get(c.metric + "_segments", 0) or min(64, max(1, largest // 64))     # (0: at most this many)
    if any(n > segments * _piece(c, c.tunables, L) for _, mine in partners for L, n in mine):
        tags.add("several pieces")
    if c.kind == "matrix" and want.matrix.size > PAIRS_MAT_CELLS:
        tags.add("matrix > 1024 cells")
    if c.one_set:
        tags.add("one-file mode")
    if s1.n == 0:
        tags.add("empty set 1")
    if s2.n == 0:
        tags.add("empty set 2")
    if (s1.n and (s1.lengths == 0).any()) or (s2.n and (s2.lengths == 0).any()):
        tags.add("empty sequences")
    return tags


def features(c):
    """what the case draws of the options, arguments, tunables and entries: the names the coverage conditions count"""
    f = {"score " + c.score, "entry " + c.entry}
    f |= {name for name in ("existence", "ignore_counts", "ignore_genes", "other_repertoire") if getattr(c, name)}
    if c.metric == "tcrdist":
        f |= {"V table"} if c.V is not None else set()
        f |= {"gap penalty 0"} if c.gap_penalty == 0 else set()
        f |= {"cutoff 0"} if c.cutoff == 0 else set()
    if c.differences is not None:
        longest = max(c.set1.longest, c.set2.longest)
        f |= {"differences 0"} if c.differences == 0 else set()
        f |= {"differences >= longest"} if c.differences >= longest else set()
    if c.kind == "nearest":
        f.add("floor %d" % c.floor)
        if c.metric == "edit":
            f.add("cap %s" % c.cap)
    used = dict(c.tunables)
    if c.index % 4 == 0:
        used.update(c.tunables2)
    f |= {"tunable " + name for name in used}
    if c.capacity:
        f.add("capacity " + c.capacity)
    return f


TUNABLE_NAMES = ("hamming_stage_refs", "hamming_segments", "hamming_generic", "hamming_link_snapshot",
                 "edit_stage_refs", "edit_segments", "edit_words", "edit_link_snapshot", "edit_nearest_prune",
                 "tcrdist_stage_refs", "tcrdist_segments")
