"""The inputs of tests/test_length_edges_gpu.py, checked without a GPU: at every value of the ladder and every option
set the properties the GPU tests rely on (tests/_ladder.py preconditions: every position mutated, deleted and
inserted in a pair the reference finds, pairs on either side of the record thresholds, all byte phases), and the
oracle's hashed path against its own brute force, which had not been held against anything at these lengths."""

import numpy as np
import pytest

import _ladder
import _oracle

CASES = _ladder.ladder_cases()


def test_the_ladder_is_the_one_the_issue_names():
    assert _ladder.AA_LADDER == (24, 28, 29, 31, 32, 33, 34, 36, 37, 40, 49, 50, 52, 53, 65, 66, 73, 74, 81, 82, 97, 98,
                                 112, 113)
    assert _ladder.NT_LADDER == (33, 34, 36, 37, 72, 96, 97, 112, 113, 128, 129, 150)
    aa_d2 = [c[1] for c in CASES if not c[0] and c[2] == "d2"]
    assert aa_d2 == [L for L in _ladder.AA_LADDER if L <= 40]
    assert len(CASES) == 3 * 24 + 10 + 4 * 12
    for name in _ladder.OPTION_SETS:             # genes on and ignore_genes both occur under every option set
        assert {c[3] % 2 for c in CASES if c[2] == name} == {0, 1}


@pytest.mark.parametrize("case", CASES, ids=_ladder.case_id)
def test_preconditions_and_oracle_against_bruteforce(case):
    nt, L, name, seed = case
    seen = _ladder.preconditions(case)
    print(_ladder.case_id(case), seen)
    a, b = _ladder.ladder_sets(L, nt, seed)
    o = _ladder.options_of(case)
    want, st = _oracle.overlap(a, b, o, threads=4)
    assert st.matches == seen["pairs"] > 0
    assert np.array_equal(want, _oracle.bruteforce(a, b, o))
    if name == "d1":                             # one-file mode, as the GPU test runs it once per case
        assert np.array_equal(_oracle.overlap(a, a, o, threads=4)[0], _oracle.bruteforce(a, a, o))


def test_sets_are_sized_from_the_length():
    for nt, ladder in ((False, _ladder.AA_LADDER), (True, _ladder.NT_LADDER)):
        for L in ladder:
            a, b = _ladder.ladder_sets(L, nt, L)
            at_L = int((a.lengths == L).sum())
            assert 200 <= a.n <= 1000 and 200 <= b.n <= 1000, (L, a.n, b.n)
            assert at_L >= 2 * L                 # (the substitution children of the parents of length L alone)
