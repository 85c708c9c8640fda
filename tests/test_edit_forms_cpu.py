"""The inputs of tests/_edit_forms.py without a GPU: the figures of the family sets from the numpy brute force, the
register forms, form changes and symbols they reach, the family without a partner and the one with a key miss, the
brute force against the oracle at d = 1 with indels and against a scalar Wagner-Fischer DP on long unrelated sequences,
and the figures of the distance sets."""

import os
import re

import numpy as np
import pytest

import _edit
import _edit_forms as ef
import _neighbors

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "compairr_amd", "csrc")
ALPHABETS = pytest.mark.parametrize("nucleotides", [False, True], ids=["aa", "nt"])


# ---- the family sets ----

@pytest.mark.parametrize("key", ef.FAMILY_KEYS, ids=ef.FAMILY_IDS)
def test_figures_of_the_family_sets(key):
    nucleotides, d, g = key
    s1, s2 = ef.family_sets(nucleotides)
    want = ef.family_want(nucleotides, d, g)
    got = ef.figures_of(s1, s2, want, d)
    print(key, got)
    assert got == ef.FAMILY_FIGURES[key]
    assert len(got[1]) == d + 1 and min(got[1]) > 0                    # every distance 0 .. d has its edges
    assert want[2].dtype == np.uint16 and int(want[0][-1]) == len(want[1])


@ALPHABETS
def test_shape_of_the_family_sets(nucleotides):
    s1, s2, fam1, fam2 = ef.families(nucleotides)
    n = len(ef.ANCESTORS[nucleotides]) * ef.DESCENDANTS
    assert (s1.n, s2.n) == (n, n) == ((160, 160) if nucleotides else (260, 260))
    for s, fam in ((s1, fam1), (s2, fam2)):
        assert s.n_repertoires == 3 and set(s.repertoire.tolist()) == {0, 1, 2}
        assert int(s.count.min()) == 1 and int(s.count.max()) == 5
        assert int(s.v_gene.max()) == ef.N_V - 1 and int(s.j_gene.max()) == ef.N_J - 1
        assert (np.abs(s.lengths - fam) <= 6).all() and int(s.lengths.max()) <= _edit.MAX_LEN
        assert (np.diff(fam) != 0).sum() > n // 2                       # (shuffled: the input order is not the group order)
        # every symbol of the alphabet
        assert set(s.residues.tolist()) == set(range(4 if nucleotides else 20))


def test_the_forms_of_the_helper_are_the_kernel_s():
    with open(os.path.join(CSRC, "allpairs.h")) as fh:
        header = fh.read()
    with open(os.path.join(CSRC, "allpairs.hip")) as fh:
        text = fh.read()
    assert re.search(r"constexpr uint32_t PAIRS_REG_RESIDUES = (\d+);", header).group(1) == str(ef.REG_RESIDUES)
    forms = re.search(r"uint32_t cmpr::pairs_form_of\(uint32_t len, uint32_t stride\)\n\{\n"
                      r"  if \(len > PAIRS_REG_RESIDUES\)\n    return 0;\n  for \(uint32_t f : \{([0-9u, ]+)\}\)\n"
                      r"    if \(stride <= f\)\n      return f;\n  return 0;\n\}", text)
    assert tuple(int(f.strip(" u")) for f in forms.group(1).split(",")) == ef.FORMS
    strides = re.search(r"static const uint32_t forms\[\] = \{([0-9, ]+), HAMMING_REG_WORDS\};", text).group(1)
    reg_words = int(re.search(r"constexpr uint32_t HAMMING_REG_WORDS = (\d+);", header).group(1))
    assert tuple(int(f) for f in strides.split(",")) + (reg_words,) == ef.STRIDES
    # the lengths at which the form changes
    for nucleotides, edges in ((False, {8: 2, 9: 4, 16: 4, 17: 8, 32: 8, 33: 16, 64: 16, 65: 0, 256: 0, 0: 2, 1: 2}),
                               (True, {32: 2, 33: 4, 64: 4, 65: 0, 256: 0, 0: 2, 1: 2})):
        for length, form in edges.items():
            assert ef.form_of(length, nucleotides) == form, (nucleotides, length)


@ALPHABETS
def test_form_coverage_of_the_family_sets(nucleotides):
    s1, s2 = ef.family_sets(nucleotides)
    assert set(ef.forms_of(s1.lengths, nucleotides).tolist()) == set(ef.ALL_FORMS[nucleotides])
    assert set(ef.forms_of(s2.lengths, nucleotides).tolist()) == set(ef.ALL_FORMS[nucleotides])
    got = ef.edges_by_form(s1, s2, ef.family_want(nucleotides, 6, True), nucleotides)
    print(got)
    assert got == ef.FORM_FIGURES[nucleotides]
    per_form, between, across = got
    assert set(per_form) == set(ef.ALL_FORMS[nucleotides]) and min(per_form.values()) >= 50
    assert between >= 50
    assert set(across) == set(ef.CROSSINGS[nucleotides]) and min(across.values()) >= 1
    # references of more than 64 residues: two column words without forcing them
    assert int((s2.lengths > 64).sum()) >= 10 and int((s1.lengths > 64).sum()) >= 10


@ALPHABETS
def test_the_family_without_a_partner(nucleotides):
    """its ten set-1 members carry a (V, J) that set 2 has, but nowhere within 6 residues of them: with genes their
    rows are empty at every d, while without genes they do have neighbours"""
    s1, s2, fam1, fam2 = ef.families(nucleotides)
    mine = ef.carries(s1, ef.PARTNERLESS_VJ)
    assert np.array_equal(mine, fam1 == ef.PARTNERLESS[nucleotides]) and int(mine.sum()) == ef.DESCENDANTS
    theirs = ef.carries(s2, ef.PARTNERLESS_VJ)
    assert int(theirs.sum()) >= 3 and (fam2[theirs] == ef.FAR[nucleotides]).all()
    gap = np.abs(s1.lengths[mine][:, None] - s2.lengths[theirs][None, :])
    assert int(gap.min()) > max(ef.FAMILY_D)
    for d in ef.FAMILY_D:
        deg = np.diff(ef.family_want(nucleotides, d, False)[0].astype(np.int64))
        assert not deg[mine].any() and deg[~mine].any()
    assert np.diff(ef.family_want(nucleotides, 6, True)[0].astype(np.int64))[mine].all()


@ALPHABETS
def test_the_family_with_a_key_miss(nucleotides):
    """its set-1 members carry a (V, J) that set 2 has at the lengths on either side of the ancestor's, not at the
    ancestor's own, which set 2 has under other genes: the partner search misses a key between two hits"""
    s1, s2, fam1, fam2 = ef.families(nucleotides)
    K = ef.KEYMISS[nucleotides]
    mine, theirs = ef.carries(s1, ef.KEYMISS_VJ), ef.carries(s2, ef.KEYMISS_VJ)
    assert np.array_equal(mine, fam1 == K) and (fam2[theirs] == K).all()
    lengths = set(s2.lengths[theirs].tolist())
    assert K - 1 in lengths and K + 1 in lengths and K not in lengths
    assert K in s2.lengths[~theirs].tolist() and K in s1.lengths[mine].tolist()
    for d in ef.FAMILY_D:
        rows, hits, _ = ef.family_want(nucleotides, d, False)
        of_mine = mine[_edit.queries_of(rows)]
        h = hits[of_mine].astype(np.int64)
        # (d = 1 may find nobody: what set 2 has at one operation or none is mostly of the ancestor's length)
        assert (len(h) or d == 1) and theirs[h].all() and K not in s2.lengths[h].tolist()
    assert int(s2.lengths[h].min()) < K < int(s2.lengths[h].max())      # (d = 6: lengths on both sides)
    # it is the key that is missing, not the distance: without genes the family has edges to the ancestor's length
    rows, hits, _ = ef.family_want(nucleotides, 6, True)
    assert K in s2.lengths[hits[mine[_edit.queries_of(rows)]].astype(np.int64)].tolist()


# ---- the yardstick ----

@ALPHABETS
@pytest.mark.parametrize("g", [False, True], ids=["genes", "g"])
def test_brute_force_is_the_oracle_with_indels_at_d1(nucleotides, g):
    s1, s2 = ef.family_sets(nucleotides)
    # (no sequence of one residue, so the pair (one residue, none) that the reference's -d 1 -i lacks does not arise)
    assert min(int(s1.lengths.min()), int(s2.lengths.min())) >= 3
    rows, hits, _ = ef.family_want(nucleotides, 1, g)
    want = _neighbors.oracle_csr(s1, s2, ef.family_options(nucleotides, g, differences=1, indels=True))
    assert np.array_equal(rows, want[0]) and np.array_equal(hits, want[1])


@ALPHABETS
def test_block_distances_against_wagner_fischer_on_long_sequences(nucleotides):
    """200 seeded pairs of the distance sets, 40 of them with both sequences above 128 residues: the vectorised DP of
    tests/_edit.py against the scalar one, and the pair list at d = 256 carrying the same number"""
    s1, s2 = ef.distance_sets(nucleotides)
    rows, hits, dist = ef.distance_want(nucleotides)
    rng = np.random.default_rng(5400)
    long1, long2 = np.nonzero(s1.lengths > 128)[0], np.nonzero(s2.lengths > 128)[0]
    pairs = [(int(rng.choice(long1)), int(rng.choice(long2))) for _ in range(40)]
    pairs += [(int(rng.integers(0, s1.n)), int(rng.integers(0, s2.n))) for _ in range(160)]
    seen = set()
    for i, j in pairs:
        a, b = ef.sequence_of(s1, i), ef.sequence_of(s2, j)
        want = ef.wagner_fischer(a, b)
        assert int(_edit.block_distances(a[None, :], b[None, :])[0, 0]) == want, (i, j)
        assert int(hits[int(rows[i]) + j]) == j and int(dist[int(rows[i]) + j]) == want, (i, j)
        seen.add(want)
    assert len(seen) >= 40 and max(seen) > 128


# ---- the distance sets ----

@ALPHABETS
def test_figures_of_the_distance_sets(nucleotides):
    s1, s2 = ef.distance_sets(nucleotides)
    assert s1.n == s2.n == 4 * len(ef.DISTANCE_LENGTHS) == 72
    assert sorted(set(s1.lengths.tolist())) == sorted(set(s2.lengths.tolist())) == list(ef.DISTANCE_LENGTHS)
    assert s1.residues.tobytes() != s2.residues.tobytes()
    rows, hits, dist = ef.distance_want(nucleotides)
    # every pair is an edge
    assert np.array_equal(rows, np.arange(s1.n + 1, dtype=np.uint64) * s2.n)
    assert np.array_equal(hits, np.tile(np.arange(s2.n, dtype=np.uint32), s1.n))
    got = (len(hits), int(dist.max()), int((dist > 128).sum()), int((dist > 64).sum()), len(set(dist.tolist())))
    print(got)
    assert got == ef.DISTANCE_FIGURES[nucleotides]
    assert got[0] == 5184 and got[1] >= 200 and got[2] >= 1000
    # (a homopolymer of 256 against a sequence without its letter: the length of the longer one)
    assert int(dist.max()) == _edit.MAX_LEN
    # the forms of the queries and the word counts of the columns
    assert set(ef.forms_of(s1.lengths, nucleotides).tolist()) == set(ef.ALL_FORMS[nucleotides])
    assert {1 if n <= 64 else 2 if n <= 128 else 4 for n in s2.lengths.tolist()} == {1, 2, 4}


def test_swapping_a_pair_list():
    s1, s2 = ef.family_sets(False)
    for d, g in ((2, False), (6, True)):
        got = ef.swapped(s1, s2, ef.family_want(False, d, g))
        want = _edit.brute_csr(s2, s1, d, g)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and np.array_equal(a, b)
