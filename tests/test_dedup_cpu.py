"""Deduplication without a GPU: the Python statement of what cmpr_deduplicate computes (tests/_dedup.py
model), printed through RepertoireSet.dedup_tsv, reproduces byte for byte what the reference's --deduplicate
wrote for the recorded cases (tests/golden/dedup/, tests/golden/make_dedup.py) -- which ties the model the GPU
tests compare against to the real reference -- and the library and its binding carry the two entry points."""

import ctypes

import pytest

import _dedup
from compairr_amd import hip

CASES = _dedup.cases()

# "Duplicates merged:" of the reference per (file, args): the table the cases were chosen by
MERGED = {
    ("dups.tsv", ""): 1, ("dups.tsv", "-f"): 1, ("dups.tsv", "-g"): 1, ("dups.tsv", "-n"): 2,
    ("lower.tsv", ""): 1, ("lower.tsv", "-n"): 1, ("lower.tsv", "-n -g"): 1, ("setb.tsv", ""): 0,
    ("tiny_aa_a.tsv", ""): 12, ("tiny_aa_a.tsv", "-g -f"): 34, ("tiny_nt_a.tsv", "-n"): 14,
    ("tiny_nt_b.tsv", "-n -g"): 19, ("rand_aa_a.tsv", ""): 1, ("clus_aa.tsv", ""): 124,
    ("clus_nt.tsv", "-n"): 4, ("clus_nt.tsv", "-n -g"): 26, ("norep.tsv", ""): 0, ("nogenes.tsv", "-g"): 0,
    ("nocount.tsv", "-f"): 0, ("cdr3.tsv", "--cdr3"): 0,
}


def test_recorded_cases_are_the_chosen_ones():
    assert {(c["file"], c["args"]): c["merged"] for c in CASES} == MERGED
    assert len(CASES) == len(MERGED)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_reproduces_the_reference(case):
    flags = _dedup.flags_of(case)
    s = _dedup.read_case(case)
    assert s.n == case["sequences"]
    first, count, merged = _dedup.model(s, _dedup.options_of(s, **flags))
    assert merged == case["merged"]
    assert len(first) == s.n - merged and list(first) == sorted(set(first.tolist()))
    got = _dedup.merged_set(s, first, count).dedup_tsv(ignore_genes=flags["ignore_genes"], cdr3=flags["cdr3"])
    assert got == _dedup.expected_of(case)


def test_dups_n_sums_the_counts():
    """dups.tsv as nucleotides: three of X1 are one entry of 3000000 + 5 + 7"""
    case = next(c for c in CASES if c["name"] == "dups_n")
    s = _dedup.read_case(case)
    first, count, merged = _dedup.model(s, _dedup.options_of(s, nucleotides=True))
    assert (first.tolist(), count.tolist(), merged) == ([0, 3], [3000012, 4000000], 2)


def test_writer_drops_the_gene_columns_and_prints_nucleotides_in_lower_case():
    case = next(c for c in CASES if c["name"] == "lower_n")
    s = _dedup.read_case(case)
    lines = s.dedup_tsv().split(b"\n")
    assert lines[0] == b"repertoire_id\tduplicate_count\tv_call\tj_call\tjunction"
    assert lines[1] == b"X1\t2\tV1\tJ1\ttgtgct"
    lines = s.dedup_tsv(ignore_genes=True, cdr3=True).split(b"\n")
    assert lines[0] == b"repertoire_id\tduplicate_count\tcdr3" and lines[1] == b"X1\t2\ttgtgct"


def test_binding_and_library_carry_the_entry_points():
    lib = ctypes.CDLL(hip.library_path())
    for name in ("cmpr_deduplicate", "cmpr_deduplicate_device"):
        assert name in hip.EXPORTS
        assert hasattr(lib, name), name
    assert lib.cmpr_abi_version() == 5
