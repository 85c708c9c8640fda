"""Neighbour lists in CSR (cmpr_neighbors): the yardstick -- the oracle's sorted pair list turned into
(row_start, hits) -- and the inputs the CPU and GPU tests share (test infrastructure)."""

import functools
import itertools

import numpy as np

import _oracle
from compairr_amd import Options, RepertoireSet, synth
from compairr_amd.sets import AA

TINY = dict(letters=3, max_len=7, n_v=2, n_j=2)
HUB = "CASSLGQGAYNEQYFG"


def csr_of_pairs(n1, pairs):
    """(row_start uint64[n1 + 1], hits uint32[E]) of a pair list sorted by (query, hit).  No pair may repeat:
    the uint32 degrees of cmpr_neighbors and its strictly increasing rows rest on that."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    q, h = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    step_q, step_h = np.diff(q), np.diff(h)
    assert (step_q >= 0).all() and (step_h[step_q == 0] >= 0).all(), "pair list is not sorted"
    assert not ((step_q == 0) & (step_h == 0)).any(), "a pair repeats"
    assert len(q) == 0 or (q[0] >= 0 and q[-1] < n1)
    row_start = np.zeros(n1 + 1, dtype=np.uint64)
    np.cumsum(np.bincount(q, minlength=n1), out=row_start[1:])
    return row_start, h.astype(np.uint32)


def oracle_csr(set1, set2, opt):
    row_start, hits = csr_of_pairs(set1.n, _oracle.pairs(set1, set2, opt))
    row_start.setflags(write=False)
    hits.setflags(write=False)
    return row_start, hits


def shape_of(row_start):
    """(edges, longest row, rows above 64, empty rows)"""
    deg = np.diff(row_start.astype(np.int64))
    return int(row_start[-1]), int(deg.max()) if len(deg) else 0, int((deg > 64).sum()), int((deg == 0).sum())


def assert_is_csr(row_start, hits, n1):
    assert row_start.dtype == np.uint64 and hits.dtype == np.uint32
    assert len(row_start) == n1 + 1 and row_start[0] == 0 and row_start[-1] == len(hits)
    inner = np.ones(len(hits), dtype=bool)
    inner[row_start[:-1][np.diff(row_start.astype(np.int64)) > 0].astype(np.int64)] = False   # a row's first hit
    assert (np.diff(hits.astype(np.int64))[inner[1:]] > 0).all(), "a row is not strictly increasing"


# ---- 1. row shapes on small sets ----

@functools.lru_cache(maxsize=None)
def tiny(n, seed, nucleotides=False):
    return synth.tiny_set(n, seed, alphabet_size=4 if nucleotides else 20, **TINY)


def tiny_options(**kw):
    return Options(n_v_genes=2, n_j_genes=2, **kw)


# name: (set 1, set 2, options, (edges, longest row, rows above 64, empty rows); None = not stated)
SMALL = {
    "self_d0": ((3000, 5), (3000, 5), dict(differences=0), (25_932, 51, None, None)),
    "self_d1": ((3000, 5), (3000, 5), dict(differences=1), (94_524, 130, 524, None)),
    "self_d1i": ((3000, 5), (3000, 5), dict(differences=1, indels=True), (184_640, 196, 1_110, None)),
    "self_d2": ((3000, 5), (3000, 5), dict(differences=2), (160_148, None, None, None)),
    "other_d1": ((3000, 5), (2500, 6), dict(differences=1), (36_819, None, None, 2_571)),
    "nt_d1ig": ((3000, 5), (2500, 6), dict(differences=1, indels=True, ignore_genes=True, nucleotides=True),
                (411_759, 554, None, None)),
}


def small_sets(name):
    a, b, kw, _ = SMALL[name]
    nt = bool(kw.get("nucleotides"))
    s1 = tiny(*a, nucleotides=nt)
    return s1, (s1 if a == b else tiny(*b, nucleotides=nt))


@functools.lru_cache(maxsize=None)
def small_want(name):
    s1, s2 = small_sets(name)
    return oracle_csr(s1, s2, tiny_options(**SMALL[name][2]))


# ---- 2. one row longer than LDS ----

def _set_of_rows(rows, seed, n_rep):
    rows = np.asarray(rows, dtype=np.uint8)
    n, L = rows.shape
    rep = np.random.default_rng(seed).integers(0, n_rep, size=n, dtype=np.uint32)
    rep[:n_rep] = np.arange(n_rep)             # (numbered in order of first appearance)
    return RepertoireSet(rows.reshape(-1), np.arange(n + 1, dtype=np.uint64) * L, np.zeros(n, dtype=np.uint32),
                         np.zeros(n, dtype=np.uint32), rep, np.ones(n, dtype=np.uint64),
                         ["H%d" % (k + 1) for k in range(n_rep)], ["V0"], ["J0"], AA)


def ball_of(hub):
    """every sequence within Hamming distance 2 of `hub`, the hub first"""
    L = len(hub)
    ball = [hub.copy()]
    for p in range(L):
        for r in range(20):
            if r != hub[p]:
                s = hub.copy()
                s[p] = r
                ball.append(s)
    others = [[r for r in range(20) if r != hub[p]] for p in range(L)]
    for p, q in itertools.combinations(range(L), 2):
        block = np.tile(hub, (361, 1))
        rs = np.array(list(itertools.product(others[p], others[q])), dtype=np.uint8)
        block[:, p], block[:, q] = rs[:, 0], rs[:, 1]
        ball.extend(block)
    ball = np.array(ball, dtype=np.uint8)
    assert len(ball) == 1 + L * 19 + L * (L - 1) // 2 * 361
    return ball


@functools.lru_cache(maxsize=None)
def hub_sets():
    """set 2: every sequence within Hamming distance 2 of HUB (1 + 16 x 19 + 120 x 361 = 43 625) and 1 375
    uniform random strangers, shuffled; set 1: the hub, a sequence at distance 1, one at distance 2, and 61
    random strangers.  One V gene, one J gene, three repertoires."""
    hub = np.array([AA.index(ch) for ch in HUB], dtype=np.uint8)
    L = len(hub)
    ball = ball_of(hub)
    rng = np.random.default_rng(16)
    rows2 = np.concatenate([ball, rng.integers(0, 20, size=(1_375, L), dtype=np.uint8)])
    rows2 = rows2[rng.permutation(len(rows2))]
    one, two = hub.copy(), hub.copy()
    one[4] = AA.index("W")
    two[2], two[11] = AA.index("W"), AA.index("H")
    rows1 = np.concatenate([np.stack([hub, one, two]), rng.integers(0, 20, size=(61, L), dtype=np.uint8)])
    return _set_of_rows(rows1, 161, 3), _set_of_rows(rows2, 162, 3)


def hamming_csr(set1, set2, d):
    """numpy brute force for sets of one length, one V and one J gene"""
    L = int(set1.lengths[0])
    a = set1.residues.reshape(-1, L)
    b = set2.residues.reshape(-1, L)
    q, h = np.nonzero((a[:, None, :] != b[None, :, :]).sum(axis=2) <= d)
    return csr_of_pairs(set1.n, np.stack([q, h], axis=1))


# ---- 3. rows of exactly the lengths at which the sorting path changes ----

EDGE_ROWS = [0, 1, 2, 8, 9, 64, 65, 8192, 8193]      # either side of 1, LANE_MAX = 8, WAVE = 64, LDS_MAX = 8192


def edge_options(**more):
    return Options(differences=2, n_v_genes=1, n_j_genes=1, **more)


@functools.lru_cache(maxsize=None)
def edge_rows():
    """set 1: nine hubs (random 16-mers, pairwise at Hamming distance >= 5: their radius-2 balls are disjoint, so
    at d = 2 a query matches only members of its own ball), then 61 random strangers -- two waves, the rows of 9
    and of 64 in one; set 2: of the ball of hub k its first EDGE_ROWS[k] members in a seeded order, and 1 000
    random strangers, shuffled.  One V gene, one J gene, three repertoires, every count 1."""
    rng = np.random.default_rng(17)
    L = len(HUB)
    hubs = rng.integers(0, 20, size=(len(EDGE_ROWS), L), dtype=np.uint8)
    apart = (hubs[:, None, :] != hubs[None, :, :]).sum(axis=2)
    assert (apart[~np.eye(len(hubs), dtype=bool)] >= 5).all()
    members = []
    for hub, n in zip(hubs, EDGE_ROWS):
        ball = ball_of(hub)
        members.append(ball[rng.permutation(len(ball))[:n]])
    rows2 = np.concatenate(members + [rng.integers(0, 20, size=(1_000, L), dtype=np.uint8)])
    rows2 = rows2[rng.permutation(len(rows2))]
    rows1 = np.concatenate([hubs, rng.integers(0, 20, size=(61, L), dtype=np.uint8)])
    return _set_of_rows(rows1, 171, 3), _set_of_rows(rows2, 172, 3)


@functools.lru_cache(maxsize=None)
def edge_want():
    return oracle_csr(*edge_rows(), edge_options())
