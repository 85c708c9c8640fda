"""Sets at a chosen longest length L for the lengths at which the hashed path changes form (test infrastructure:
tests/test_length_edges_cpu.py, tests/test_length_edges_gpu.py, tests/fuzz_gpu.py, tests/golden/make_golden.py).

ladder_sets(L, nucleotides, seed) gives two sets from one pool of parents.  Every child is one mutation of one
parent (one substitution, two substitutions, one deletion, one insertion) and the two sets mutate independently,
so that set 1 against set 2 holds parent-child, child-parent and child-child pairs at d = 0, 1, 2 and with -i.
The mutated positions are dealt by construction (children()):
  * every position 0 .. L-1 of a parent of length L is substituted once with the genes kept and once more, at the
    mirrored position, every third time with another V gene;
  * every position 0 .. L-1 of a parent of length L is deleted once, and at every position 0 .. L-1 of a parent of
    length L-1 a residue is inserted once (the child has length L): with -i both sets then hold a pair of lengths
    (L, L-1) and one of (L-1, L) for every deleted position;
  * two substitutions on either side of every threshold of THRESHOLDS below L, then pairs of positions that cycle.
preconditions() works the properties out from the oracle's pair lists and the sets alone and asserts them; the
generator was chosen so that they hold at every value of the ladder.  Nothing here imports the library."""

import functools

import numpy as np

import _oracle
from compairr_amd import Options
from compairr_amd.sets import AA, NT, RepertoireSet

# both sides of every length at which a decision flips (derived in tests/test_length_edges_gpu.py)
AA_LADDER = (24, 28, 29, 31, 32, 33, 34, 36, 37, 40, 49, 50, 52, 53, 65, 66, 73, 74, 81, 82, 97, 98, 112, 113)
NT_LADDER = (33, 34, 36, 37, 72, 96, 97, 112, 113, 128, 129, 150)
AA_D2_MAX = 40                                  # the oracle's time at d = 2: 0.9 s at 40 amino acids, 9 s at 113

N_V, N_J, N_REP = 3, 2, 3
PARENTS = 40
# 28: the hash in a query's record from byte 28 on; 32, 128: the residues of a reference record (layout.h REC_RES,
# REC_RES_NT); 36: the residues of a query's record (layout.h QueryRec)
THRESHOLDS = (28, 32, 36, 128)

# name: (differences, indels)
OPTION_SETS = {"d0": (0, False), "d1": (1, False), "d1i": (1, True), "d2": (2, False)}


def ladder_cases(with_d2_beyond=False):
    """[(nucleotides, L, option set, seed)]: genes on for even seeds, ignore_genes for odd ones"""
    out = []
    for nt, ladder in ((False, AA_LADDER), (True, NT_LADDER)):
        for L in ladder:
            for k, name in enumerate(OPTION_SETS):
                if name == "d2" and not nt and L > AA_D2_MAX and not with_d2_beyond:
                    continue
                out.append((nt, L, name, L + k))
    return out


def case_id(case):
    nt, L, name, seed = case
    return "%s%d_%s_%s" % ("nt" if nt else "aa", L, name, "g" if seed % 2 else "genes")


def options_of(case, **more):
    nt, _, name, seed = case
    d, indels = OPTION_SETS[name]
    return Options(differences=d, indels=indels, nucleotides=nt, ignore_genes=bool(seed % 2), n_v_genes=N_V,
                   n_j_genes=N_J, **more)


def parents(L, A, seed):
    """[(residues, v, j)]: half of length L - 1, a quarter of length L, a quarter spread over L - 17 .. L - 1"""
    rng = np.random.default_rng([seed, L, A, 0x1ADD])
    lens = np.full(PARENTS, L - 1)
    lens[PARENTS // 2:3 * PARENTS // 4] = L
    spread = np.arange(3 * PARENTS // 4, PARENTS)
    lens[spread] = L - 1 - (spread * 7 + seed) % 17
    return [(rng.integers(0, A, size=int(n), dtype=np.uint8), int(rng.integers(0, N_V)), int(rng.integers(0, N_J)))
            for n in lens]


def children(pool, L, A, rng):
    """[(residues, v, j)] of one set: see the module docstring"""
    out = []
    at_L = [p for p in pool if len(p[0]) == L]
    below = [p for p in pool if len(p[0]) == L - 1]
    others = [p for p in pool if len(p[0]) != L]
    many = max(L // 2, 40)

    def other(x, r):
        return (x + 1 + int(rng.integers(0, A - 1))) % A if r is None else r

    def substituted(parent, positions, new_v=False):
        s, v, j = parent
        s = s.copy()
        for p in positions:
            s[p] = other(int(s[p]), None)
        out.append((s, (v + 1) % N_V if new_v else v, j))

    for i in range(L):                           # one substitution at every position of a sequence of length L
        substituted(at_L[i % len(at_L)], [i])
        substituted(at_L[(i + 3) % len(at_L)], [L - 1 - i], new_v=i % 3 == 0)
    for i in range(many):                        # ... and on the other lengths
        parent = others[i % len(others)]
        substituted(parent, [(7 * i + 3) % len(parent[0])], new_v=i % 4 == 0)
    k = 0
    for T in THRESHOLDS:                         # two substitutions on either side of a threshold
        for lo, hi in ((T - 1, T), (0, T), (T - 1, L - 1), (T - 3, T + 2)):
            if 0 <= lo < T <= hi < L:
                substituted(at_L[k % len(at_L)], [lo, hi])
                k += 1
    for i in range(many):                        # ... and anywhere
        parent = pool[i % len(pool)]
        n = len(parent[0])
        p = (5 * i) % n
        substituted(parent, [p, (p + 1 + (3 * i) % (n - 1)) % n], new_v=i % 8 == 0)
    for i in range(L):                           # every position deleted, a residue inserted at every position
        s, v, j = at_L[(i + 1) % len(at_L)]
        out.append((np.delete(s, i), v, j))
        s, v, j = below[i % len(below)]
        out.append((np.insert(s, i, rng.integers(0, A)).astype(np.uint8), v, j))
    for i in range(4):                           # a parent again under another V gene: fails on genes alone at d = 0
        substituted(pool[(9 * i + 1) % len(pool)], [], new_v=True)
    for i in range(20):                          # deletions on the other lengths
        s, v, j = others[(i + 5) % len(others)]
        out.append((np.delete(s, (11 * i) % len(s)), (v + 1) % N_V if i % 5 == 0 else v, j))
    return out


def set_of(rows, rng, prefix, A):
    order = rng.permutation(len(rows))           # the sequence order is shuffled
    rows = [rows[k] for k in order]
    n = len(rows)
    lens = np.array([len(r[0]) for r in rows], dtype=np.int64)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=offsets[1:])
    rep = rng.integers(0, N_REP, size=n).astype(np.uint32)
    rep[:N_REP] = np.arange(N_REP)               # (numbered by first appearance)
    return RepertoireSet(np.concatenate([r[0] for r in rows]).astype(np.uint8), offsets,
                         np.array([r[1] for r in rows], dtype=np.uint32), np.array([r[2] for r in rows], dtype=np.uint32),
                         rep, rng.integers(1, 10, size=n, dtype=np.uint64),
                         ["%s%d" % (prefix, k + 1) for k in range(N_REP)], ["V%d" % k for k in range(N_V)],
                         ["J%d" % k for k in range(N_J)], NT if A == 4 else AA)


@functools.lru_cache(maxsize=8)
def ladder_sets(L, nucleotides, seed):
    """(a, b): two sets with `longest` == L, 3 V x 2 J genes, 3 repertoires, counts 1 .. 9 (do not change them)"""
    assert L >= 19
    A = 4 if nucleotides else 20
    pool = parents(L, A, seed)
    sets = []
    for which, prefix in ((1, "A"), (2, "B")):
        rng = np.random.default_rng([seed, L, A, which])
        sets.append(set_of(pool + children(pool, L, A, rng), rng, prefix, A))
    for s in sets:
        assert s.longest == L
        for x in (s.residues, s.offsets, s.v_gene, s.j_gene, s.repertoire, s.count):
            x.setflags(write=False)
    return tuple(sets)


# ---- the properties of a case, worked out from the oracle's pairs ----

def sequence(s, i):
    return s.residues[int(s.offsets[i]):int(s.offsets[i + 1])]


@functools.lru_cache(maxsize=4)
def oracle_pairs(L, nucleotides, seed, d, indels, ignore_genes):
    a, b = ladder_sets(L, nucleotides, seed)
    out = _oracle.pairs(a, b, Options(differences=d, indels=indels, nucleotides=nucleotides, ignore_genes=ignore_genes,
                                      n_v_genes=N_V, n_j_genes=N_J))
    out.setflags(write=False)
    return out


def phases(s):
    return s.offsets[:-1].astype(np.int64) & 15


def preconditions(case):
    """assert what the issue asks of the inputs of `case`; returns the figures (for a reader of -s output)"""
    nt, L, name, seed = case
    d, indels = OPTION_SETS[name]
    a, b = ladder_sets(L, nt, seed)
    g = bool(seed % 2)
    pairs = oracle_pairs(L, nt, seed, d, indels, g)
    la, lb = a.lengths[pairs[:, 0]], b.lengths[pairs[:, 1]]
    seen = {"pairs": len(pairs), "n": (a.n, b.n)}

    # the sets themselves
    assert a.longest == L and b.longest == L
    for s in (a, b):
        assert len(set(phases(s).tolist())) == 16
        assert s.n_repertoires == N_REP and set(s.repertoire.tolist()) == set(range(N_REP))
        assert 1 <= s.count.min() and s.count.max() <= 9
        assert set(s.v_gene.tolist()) == set(range(N_V)) and set(s.j_gene.tolist()) == set(range(N_J))
        reach = s.lengths + phases(s)
        if not nt and 34 <= L <= 36:             # three 16-byte pieces: some sequences fit them, some do not
            assert (reach > 48).any() and (reach <= 48).any()
        if 98 <= L <= 112:                       # ... and seven
            assert (reach > 112).any() and (reach <= 112).any()

    # pairs at distance 0
    same = [(q, h) for q, h in pairs[la == lb] if np.array_equal(sequence(a, q), sequence(b, h))]
    assert same
    seen["d0"] = len(same)

    # a pair that fails on genes alone (at d = 2 read from the lists of d = 1: such a pair is within d = 2 as well)
    dg, ig = (1, False) if d == 2 else (d, indels)
    with_genes = oracle_pairs(L, nt, seed, dg, ig, False)
    without = oracle_pairs(L, nt, seed, dg, ig, True)
    assert len(without) > len(with_genes)
    assert set(map(tuple, with_genes.tolist())) < set(map(tuple, without.tolist()))
    seen["genes_alone"] = len(without) - len(with_genes)

    if d >= 1:
        # every position is the only difference of two sequences of length L
        single, double = set(), []
        for q, h in pairs[(la == L) & (lb == L)]:
            w = np.flatnonzero(sequence(a, q) != sequence(b, h))
            if len(w) == 1:
                single.add(int(w[0]))
            elif len(w) == 2:
                double.append((int(w[0]), int(w[1])))
        assert single == set(range(L)), sorted(set(range(L)) - single)
        if d == 2:
            for T in THRESHOLDS:
                if T < L:
                    assert any(lo < T <= hi for lo, hi in double), T
                    assert any((lo, hi) == (T - 1, T) for lo, hi in double), T
            seen["two"] = len(double)
    if indels:
        # every position is the deleted one of a pair of lengths (L, L - 1) and of one of (L - 1, L)
        for longer_first in (True, False):
            deleted = set()
            sel = (la == L) & (lb == L - 1) if longer_first else (la == L - 1) & (lb == L)
            for q, h in pairs[sel]:
                x, y = (sequence(a, q), sequence(b, h)) if longer_first else (sequence(b, h), sequence(a, q))
                diff = np.flatnonzero(x[:-1] != y)
                first = int(diff[0]) if len(diff) else L - 1
                # (deleting any residue of the run that ends at `first` gives y)
                p = first
                while p >= 0 and x[p] == x[first] and np.array_equal(np.delete(x, p), y):
                    deleted.add(p)
                    p -= 1
            assert deleted == set(range(L)), (longer_first, sorted(set(range(L)) - deleted))
        seen["unequal"] = int((la != lb).sum())
    return seen
