"""Helpers of the deduplication tests (not a test module): the recorded cases of tests/golden/dedup/, a
minimal reader of their input files, and a dict-based statement of what cmpr_deduplicate computes."""

import json
import os

import numpy as np

from compairr_amd import Options, RepertoireSet
from compairr_amd.sets import AA, NT

HERE = os.path.dirname(os.path.abspath(__file__))
INPUTS = os.path.join(HERE, "golden", "inputs")
DEDUP = os.path.join(HERE, "golden", "dedup")


def cases():
    with open(os.path.join(DEDUP, "manifest.json")) as fh:
        return json.load(fh)


def expected_of(case) -> bytes:
    with open(os.path.join(DEDUP, case["name"] + ".tsv"), "rb") as fh:
        return fh.read()


def flags_of(case) -> dict:
    """the reference's command-line flags of a case as keywords of read_tsv"""
    a = case["args"].split()
    return {"nucleotides": "-n" in a, "ignore_genes": "-g" in a, "ignore_counts": "-f" in a, "cdr3": "--cdr3" in a}


def options_of(s: RepertoireSet, nucleotides=False, ignore_genes=False, ignore_counts=False, cdr3=False,
               **more) -> Options:
    return Options(nucleotides=nucleotides, ignore_genes=ignore_genes, ignore_counts=ignore_counts,
                   n_v_genes=max(1, len(s.v_names)), n_j_genes=max(1, len(s.j_names)), **more)


def read_tsv(path, nucleotides=False, ignore_genes=False, ignore_counts=False, cdr3=False) -> RepertoireSet:
    """What the recorded cases need of an AIRR TSV, and no more: columns found by their header name; a file
    without repertoire_id is repertoire "1"; the gene columns may be missing under -g and the count empty
    under -f; residues are upper-cased, U is T; --cdr3 takes the cdr3 / cdr3_aa column.  Repertoires and
    genes are numbered by first appearance."""
    with open(path, newline="") as fh:
        lines = [l.rstrip("\r") for l in fh.read().split("\n") if l.rstrip("\r")]
    col = {name: k for k, name in enumerate(lines[0].split("\t"))}
    seq_col = col[("cdr3" if cdr3 else "junction") + ("" if nucleotides else "_aa")]
    alphabet = NT if nucleotides else AA
    code = {c: k for k, c in enumerate(alphabet)}
    numbers = {"rep": {}, "v": {}, "j": {}}

    def number(kind, name):
        return numbers[kind].setdefault(name, len(numbers[kind]))

    res, off, v, j, rep, cnt = [], [0], [], [], [], []
    for line in lines[1:]:
        f = line.split("\t")
        rep.append(number("rep", f[col["repertoire_id"]] if "repertoire_id" in col else "1"))
        if ignore_genes and ("v_call" not in col or "j_call" not in col):
            v.append(number("v", ""))
            j.append(number("j", ""))
        else:
            v.append(number("v", f[col["v_call"]]))
            j.append(number("j", f[col["j_call"]]))
        text = f[col["duplicate_count"]] if "duplicate_count" in col else ""
        cnt.append(1 if ignore_counts and not text else int(text))
        seq = f[seq_col].upper()
        if nucleotides:
            seq = seq.replace("U", "T")
        res.extend(code[c] for c in seq)
        off.append(len(res))
    return RepertoireSet(np.array(res, dtype=np.uint8), np.array(off, dtype=np.uint64),
                         np.array(v, dtype=np.uint32), np.array(j, dtype=np.uint32),
                         np.array(rep, dtype=np.uint32), np.array(cnt, dtype=np.uint64),
                         list(numbers["rep"]), list(numbers["v"]), list(numbers["j"]), alphabet)


def read_case(case) -> RepertoireSet:
    return read_tsv(os.path.join(INPUTS, case["file"]), **flags_of(case))


def model(s: RepertoireSet, opt: Options):
    """(first, count, merged): sequences with the same repertoire, the same V and J unless ignore_genes, and
    the same residues (hence the same length) are one class; per class in increasing `first` its smallest
    sequence number and the sum of its counts modulo 2^64 -- with ignore_counts the number of its members;
    merged = n - classes."""
    text = s.residues.tobytes()
    off = s.offsets.astype(np.int64).tolist()
    rep, v, j, cnt = s.repertoire.tolist(), s.v_gene.tolist(), s.j_gene.tolist(), s.count.tolist()
    where, first, count = {}, [], []
    for i in range(s.n):
        key = (rep[i], text[off[i]:off[i + 1]]) if opt.ignore_genes else (rep[i], v[i], j[i], text[off[i]:off[i + 1]])
        k = where.setdefault(key, len(first))
        if k == len(first):
            first.append(i)
            count.append(0)
        count[k] = (count[k] + (1 if opt.ignore_counts else cnt[i])) & (2 ** 64 - 1)
    return np.array(first, dtype=np.uint32), np.array(count, dtype=np.uint64), s.n - len(first)


def merged_set(s: RepertoireSet, first, count) -> RepertoireSet:
    out = s.subset(first)
    out.count = np.ascontiguousarray(count, dtype=np.uint64)
    return out
