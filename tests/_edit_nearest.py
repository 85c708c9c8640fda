"""The nearest neighbour per sequence under edit distance (cmpr_edit_nearest): a numpy brute force of the definition --
the Levenshtein distance of every pair of every two lengths (_edit.block_distances), the eligibility mask, row minimum,
smallest number at it and the count of the minimum --, the same three arrays from the pair list of _edit at some d
(_nearest.from_pairs), and the inputs and figures the CPU and GPU tests share (test infrastructure).  Nothing here
calls the library under test."""

import functools

import numpy as np

import _edit
import _nearest
from compairr_amd import Options, RepertoireSet, synth
from compairr_amd.sets import AA

NONE32, NONE16 = _nearest.NONE32, _nearest.NONE16
FAR = np.iinfo(np.int64).max


# ---- (a) the brute force ----

def all_distances(set1, set2):
    """int64[n1, n2]: the Levenshtein distance of every sequence of set1 to every sequence of set2, by pairs of lengths"""
    len1, len2 = set1.lengths.astype(np.int64), set2.lengths.astype(np.int64)
    off1, off2 = set1.offsets.astype(np.int64), set2.offsets.astype(np.int64)
    out = np.zeros((set1.n, set2.n), dtype=np.int64)
    for L1 in np.unique(len1).tolist():
        i1 = np.nonzero(len1 == L1)[0]
        a = set1.residues[off1[i1, None] + np.arange(L1, dtype=np.int64)].reshape(len(i1), L1)
        for L2 in np.unique(len2).tolist():
            i2 = np.nonzero(len2 == L2)[0]
            b = set2.residues[off2[i2, None] + np.arange(L2, dtype=np.int64)].reshape(len(i2), L2)
            step = max(1, (1 << 23) // max(1, len(i2) * (L2 + 1)))
            for lo in range(0, len(i1), step):
                out[np.ix_(i1[lo:lo + step], i2)] = _edit.block_distances(a[lo:lo + step], b)
    out.setflags(write=False)
    return out


def brute(set1, set2, ignore_genes=False, floor=0, cap=None, other_rep=False, dist=None):
    """(nearest uint32[n1], distance uint16[n1], ties uint32[n1]); `set2 is set1` is one-set mode, cap None is uncapped;
    `dist`: all_distances(set1, set2) where the caller has it already"""
    one_set = set2 is set1
    assert one_set or not other_rep
    n1 = set1.n
    nearest = np.full(n1, NONE32, dtype=np.uint32)
    distance = np.full(n1, NONE16, dtype=np.uint16)
    ties = np.zeros(n1, dtype=np.uint32)
    if n1 == 0 or set2.n == 0:
        return nearest, distance, ties
    dist = (all_distances(set1, set2) if dist is None else dist).copy()
    rows, cols = np.arange(n1), np.arange(set2.n)
    ok = _nearest.eligible(set1, set2, rows, cols, dist, ignore_genes, floor, one_set, other_rep)
    if cap is not None:
        ok &= dist <= cap
    dist[~ok] = FAR
    best = dist.min(axis=1)
    found = best != FAR
    nearest[found] = dist.argmin(axis=1)[found]                        # (the first is the smallest number)
    distance[found] = best[found]
    ties[found] = (dist == best[:, None]).sum(axis=1)[found]
    return nearest, distance, ties


# ---- (b) from the pair list of _edit at d ----

def from_edges(set1, set2, edges, floor=0, other_rep=False):
    """the three arrays from a CSR pair list with distances, complete up to its d: _nearest.from_pairs"""
    return _nearest.from_pairs(set1, set2, edges[0], edges[1], edges[2], floor, other_rep)


def from_want(name, cap, ignore_genes, floor=0, other_rep=False):
    s1, s2 = _edit.sets_of(name)
    return from_edges(s1, s2, _edit.want(name, cap, ignore_genes), floor, other_rep)


# ---- the inputs ----

@functools.lru_cache(maxsize=None)
def distances_of(name):
    return all_distances(*sets_of(name))


@functools.lru_cache(maxsize=None)
def want(name, ignore_genes, floor, cap, other_rep=False):
    """(a) on an input by name, computed once and read-only"""
    s1, s2 = sets_of(name)
    out = brute(s1, s2, ignore_genes, floor, cap, other_rep, distances_of(name))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tuned_sets():
    """2 500 nucleotide sequences of 7 .. 9 residues against themselves: with ignore_genes about 830 per length, four
    workgroups per group, two staged pieces per partner"""
    s = synth.tiny_set(2500, 12, alphabet_size=4, letters=4, min_len=7, max_len=9)
    return s, s


def swapped_sets():
    return _edit.long_row_sets()[::-1]


def edge_sets_of(nucleotides):
    return _edit.edge_sets(nucleotides)[:2]


SETS = {"tuned": tuned_sets, "long": _edit.long_row_sets, "swapped": swapped_sets, "hand": lambda: hand()[:2],
        "edge-aa": lambda: edge_sets_of(False), "edge-nt": lambda: edge_sets_of(True)}


def sets_of(name):
    return SETS[name]() if name in SETS else _edit.sets_of(name)


def options_of(name, ignore_genes, **more):
    if name in ("tuned", "long", "swapped"):
        return _edit.options(nucleotides=True, ignore_genes=ignore_genes, **more)
    if name == "hand":
        return Options(n_v_genes=3, n_j_genes=1, ignore_genes=ignore_genes, **more)
    if name.startswith("edge-"):
        return _edit.edge_options(name == "edge-nt", **more)
    return _edit.options_of(name, ignore_genes, **more)


@functools.lru_cache(maxsize=None)
def hand():
    """(set 1, set 2, the three arrays at floor 0, uncapped, with genes): the length-gap case, written by hand.
         set 1   0 AAAA v0          1 CCCC v1          2 DD v2
         set 2   0 AAAAC v0   1 AAA v0   2 AAAC v0   3 WWWWWWWW v0   4 CCDD v1   5 CCCCD v1   6 (empty) v2
    Query 0 has three candidates at distance 1, two of them one residue longer or shorter and one of its own length,
    and the smallest number among them is NOT in the group of its own length: a walk that stops at the gap g when
    `best > g` fails in place of `best >= g` answers ties 1 and number 2.  Query 1 has its own length at 2 and a group
    one residue longer at 1.  Query 2 has the empty sequence alone, at 2."""
    def build(seqs, v, prefix):
        res = np.array([AA.index(ch) for s in seqs for ch in s], dtype=np.uint8)
        off = np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)
        n = len(seqs)
        return RepertoireSet(res, off, np.array(v, dtype=np.uint32), np.zeros(n, dtype=np.uint32),
                             np.zeros(n, dtype=np.uint32), np.ones(n, dtype=np.uint64), [prefix], ["V0", "V1", "V2"],
                             ["J0"], AA)
    s1 = build(["AAAA", "CCCC", "DD"], [0, 1, 2], "Q")
    s2 = build(["AAAAC", "AAA", "AAAC", "WWWWWWWW", "CCDD", "CCCCD", ""], [0, 0, 0, 0, 1, 1, 2], "R")
    result = (np.array([0, 5, 6], dtype=np.uint32), np.array([1, 1, 2], dtype=np.uint16),
              np.array([3, 1, 1], dtype=np.uint32))
    return s1, s2, result


# what the stop with `best > g` would answer for query 0 of hand(): (nearest, distance, ties)
HAND_WRONG_STOP = (2, 1, 1)


# ---- the figures ----

def figures(got):
    """(none, histogram of the nearest distances of those who have one, sum of ties)"""
    return _nearest.figures(got)[:3]


# (input, ignore_genes, floor, cap): (none, histogram, sum of ties); from the brute force
FIGURES = {
    ("nt", False, 0, 1): (206, [17, 77], 230),
    ("nt", False, 0, 3): (56, [17, 77, 84, 66], 807),
    ("nt", False, 0, None): (0, [17, 77, 84, 66, 38, 15, 3], 1_227),
    ("nt", False, 1, 1): (206, [0, 94], 349),
    ("nt", False, 1, 3): (56, [0, 94, 84, 66], 926),
    ("nt", False, 1, None): (0, [0, 94, 84, 66, 38, 15, 3], 1_346),
    ("nt", True, 0, 1): (181, [33, 86], 692),
    ("nt", True, 0, 3): (36, [33, 86, 84, 61], 1_995),
    ("nt", True, 0, None): (0, [33, 86, 84, 61, 25, 8, 3], 2_852),
    ("nt", True, 1, 1): (182, [0, 118], 1_366),
    ("nt", True, 1, 3): (36, [0, 118, 85, 61], 2_676),
    ("nt", True, 1, None): (0, [0, 118, 85, 61, 25, 8, 3], 3_533),
    ("aa", False, 0, 1): (148, [62, 90], 468),
    ("aa", False, 0, 3): (7, [62, 90, 106, 35], 1_010),
    ("aa", False, 0, None): (0, [62, 90, 106, 35, 7], 1_068),
    ("aa", False, 1, 1): (156, [0, 144], 856),
    ("aa", False, 1, 3): (7, [0, 144, 114, 35], 1_434),
    ("aa", False, 1, None): (0, [0, 144, 114, 35, 7], 1_492),
    ("aa", True, 0, 1): (94, [94, 112], 987),
    ("aa", True, 0, 3): (0, [94, 112, 80, 14], 1_624),
    ("aa", True, 0, None): (0, [94, 112, 80, 14], 1_624),
    ("aa", True, 1, 1): (96, [0, 204], 3_352),
    ("aa", True, 1, 3): (0, [0, 204, 82, 14], 4_033),
    ("aa", True, 1, None): (0, [0, 204, 82, 14], 4_033),
    ("min0", False, 0, 1): (189, [57, 54], 2_172),
    ("min0", False, 0, 3): (65, [57, 54, 55, 69], 7_662),
    ("min0", False, 0, None): (0, [57, 54, 55, 69, 65], 11_622),
    ("min0", False, 1, 1): (189, [0, 111], 2_171),
    ("min0", False, 1, 3): (65, [0, 111, 55, 69], 7_661),
    ("min0", False, 1, None): (0, [0, 111, 55, 69, 65], 11_621),
    ("min0", True, 0, 1): (189, [57, 54], 8_634),
    ("min0", True, 0, 3): (65, [57, 54, 55, 69], 30_712),
    ("min0", True, 0, None): (0, [57, 54, 55, 69, 65], 47_417),
    ("min0", True, 1, 1): (189, [0, 111], 8_691),
    ("min0", True, 1, 3): (65, [0, 111, 55, 69], 30_769),
    ("min0", True, 1, None): (0, [0, 111, 55, 69, 65], 47_474),
}
CASES = list(FIGURES)
IDS = ["%s%s-floor%d-cap%s" % (k[0], "-g" if k[1] else "", k[2], "none" if k[3] is None else k[3]) for k in CASES]
