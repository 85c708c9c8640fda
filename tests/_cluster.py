"""Helpers of the clustering tests (not a test module): the partition the reference's --cluster recorded for
the `-c` cases of tests/golden/manifest.json, a plain statement of what cmpr_cluster computes, and a numpy
union-find over a pair list."""

import json
import os

import numpy as np

from compairr_amd import Options, RepertoireSet
from compairr_amd.sets import AA, NT

HERE = os.path.dirname(os.path.abspath(__file__))
INPUTS = os.path.join(HERE, "golden", "inputs")
EXPECTED = os.path.join(HERE, "golden", "expected")


def cases():
    """the recorded runs of the reference with -c that exit 0"""
    with open(os.path.join(HERE, "golden", "manifest.json")) as fh:
        return [c for c in json.load(fh) if c["cmd"] == "-c" and c["exit"] == 0]


def flags_of(case) -> dict:
    a = case["args"].split()
    d = int(a[a.index("-d") + 1]) if "-d" in a else 0
    return {"differences": d, "indels": "-i" in a, "nucleotides": "-n" in a, "ignore_genes": "-g" in a,
            "cdr3": "--cdr3" in a}


def _rows(path):
    with open(path, newline="") as fh:
        lines = [l.rstrip("\r") for l in fh.read().split("\n") if l.rstrip("\r")]
    return lines[0].lstrip("#").split("\t"), [l.split("\t") for l in lines[1:]]


def _sequence_column(nucleotides, cdr3):
    return ("cdr3" if cdr3 else "junction") + ("" if nucleotides else "_aa")


def _text(seq, nucleotides):
    seq = seq.upper()
    return seq.replace("U", "T") if nucleotides else seq


def read_input(case):
    """(set, keys): the case's input file as a RepertoireSet -- columns found by their header name; the gene
    columns may be missing under -g, the sequence_id column altogether; residues upper-cased, U is T under -n;
    repertoires and genes numbered by first appearance -- and per input row its (repertoire_id, sequence_id,
    sequence) key."""
    f = flags_of(case)
    header, rows = _rows(os.path.join(INPUTS, case["files"][0]))
    col = {name: k for k, name in enumerate(header)}
    seq_col = col[_sequence_column(f["nucleotides"], f["cdr3"])]
    alphabet = NT if f["nucleotides"] else AA
    code = {c: k for k, c in enumerate(alphabet)}
    numbers = {"rep": {}, "v": {}, "j": {}}

    def number(kind, name):
        return numbers[kind].setdefault(name, len(numbers[kind]))

    genes = "v_call" in col and "j_call" in col
    assert genes or f["ignore_genes"]
    res, off, v, j, rep, cnt, keys = [], [0], [], [], [], [], []
    for r in rows:
        rid = r[col["repertoire_id"]] if "repertoire_id" in col else "1"
        sid = r[col["sequence_id"]] if "sequence_id" in col else ""
        seq = _text(r[seq_col], f["nucleotides"])
        rep.append(number("rep", rid))
        v.append(number("v", r[col["v_call"]] if genes else ""))
        j.append(number("j", r[col["j_call"]] if genes else ""))
        cnt.append(int(r[col["duplicate_count"]]) if "duplicate_count" in col and r[col["duplicate_count"]] else 1)
        res.extend(code[c] for c in seq)
        off.append(len(res))
        keys.append((rid, sid, seq))
    s = RepertoireSet(np.array(res, dtype=np.uint8), np.array(off, dtype=np.uint64), np.array(v, dtype=np.uint32),
                      np.array(j, dtype=np.uint32), np.array(rep, dtype=np.uint32), np.array(cnt, dtype=np.uint64),
                      list(numbers["rep"]), list(numbers["v"]), list(numbers["j"]), alphabet)
    return s, keys


def options_of(s: RepertoireSet, case, **more) -> Options:
    f = flags_of(case)
    return Options(differences=f["differences"], indels=f["indels"], nucleotides=f["nucleotides"],
                   ignore_genes=f["ignore_genes"], n_v_genes=max(1, len(s.v_names)),
                   n_j_genes=max(1, len(s.j_names)), **more)


def recorded_partition(case, keys=None):
    """(label, size, clusters) as the reference printed them for `case`: every output row mapped back to its
    input row by (repertoire_id, sequence_id, sequence); label[i] = the input number of the FIRST printed row
    of i's cluster, size[i] = the cluster_size column.  Asserts what makes that the yardstick: every row maps,
    no key names two input rows, and each cluster's first row is its member with the smallest input number."""
    f = flags_of(case)
    if keys is None:
        keys = read_input(case)[1]
    where = {}
    for i, k in enumerate(keys):
        assert k not in where, "key %r names input rows %d and %d" % (k, where[k], i)
        where[k] = i
    header, rows = _rows(os.path.join(EXPECTED, case["name"] + ".tsv"))
    col = {name: k for k, name in enumerate(header)}
    seq_col = col[_sequence_column(f["nucleotides"], f["cdr3"])]
    n = len(keys)
    assert len(rows) == n
    label = np.full(n, -1, dtype=np.int64)
    size = np.zeros(n, dtype=np.int64)
    first, members = {}, {}
    for r in rows:
        k = (r[col["repertoire_id"]], r[col["sequence_id"]], _text(r[seq_col], f["nucleotides"]))
        assert k in where, "output row %r maps to no input row" % (k,)
        i = where[k]
        assert label[i] < 0, "output rows map twice to input row %d" % i
        no = int(r[col["cluster_no"]])
        label[i] = first.setdefault(no, i)
        size[i] = int(r[col["cluster_size"]])
        members.setdefault(no, []).append(i)
    assert (label >= 0).all()                                  # zero unmapped rows, either way
    for no, m in members.items():
        assert first[no] == min(m), "cluster %d starts at row %d, its minimum is %d" % (no, first[no], min(m))
        assert all(size[i] == len(m) for i in m)
    return label.astype(np.uint32), size.astype(np.uint32), len(first)


# ---- what cmpr_cluster computes, stated plainly ----

def labels_of_pairs(n, q, h):
    """label[i] = the smallest number of i's connected component under the edges (q[k], h[k]): numpy
    min-label propagation with pointer jumping (each round at least halves the longest chain)"""
    q, h = np.asarray(q, dtype=np.int64), np.asarray(h, dtype=np.int64)
    label = np.arange(n, dtype=np.int64)
    while True:
        new = label.copy()
        np.minimum.at(new, q, label[h])
        np.minimum.at(new, h, label[q])
        while True:
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, label):
            return label.astype(np.uint32)
        label = new


def sizes_of_labels(label):
    return np.bincount(label, minlength=len(label))[label].astype(np.uint32)


def model(s: RepertoireSet, opt: Options):
    """(label, size, clusters): a union-find over the pairs found by brute force.  Two sequences are a pair when
    they have the same length and differ in at most `differences` positions, or -- with indels -- one is the
    other with one residue deleted; and, unless ignore_genes, the same V and the same J.  Every sequence is
    compared with every other one of its genes and length (numpy, a row against the rows behind it) and, for
    indels, each of its one-residue deletions is looked up among the sequences one shorter.  For sets of a few
    thousand sequences."""
    text = s.residues.tobytes()
    off = s.offsets.astype(np.int64).tolist()
    seqs = [text[off[i]:off[i + 1]] for i in range(s.n)]
    gene = [(0, 0)] * s.n if opt.ignore_genes else list(zip(s.v_gene.tolist(), s.j_gene.tolist()))
    parent = list(range(s.n))

    def root(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def unite(a, b):
        ra, rb = root(a), root(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)

    # equal sequences with equal genes are a pair at any d: each is linked to the first copy, and the first
    # copies -- the distinct entries -- are compared with each other
    distinct, groups = {}, {}
    for i in range(s.n):
        k = (gene[i], seqs[i])
        if k in distinct:
            parent[i] = distinct[k]
        else:
            distinct[k] = i
            groups.setdefault((gene[i], len(seqs[i])), []).append(i)
    for (g, L), members in groups.items():
        if opt.differences and L and len(members) > 1:
            rows = np.frombuffer(b"".join(seqs[i] for i in members), dtype=np.uint8).reshape(len(members), L)
            for x in range(len(members) - 1):
                near = np.flatnonzero((rows[x + 1:] != rows[x]).sum(axis=1) <= opt.differences)
                for y in near.tolist():
                    unite(members[x], members[x + 1 + y])
        if opt.indels:
            for i in members:
                q = seqs[i]
                for p in range(L):
                    other = distinct.get((g, q[:p] + q[p + 1:]))
                    if other is not None:
                        unite(i, other)
    label = np.array([root(i) for i in range(s.n)], dtype=np.uint32)
    return label, sizes_of_labels(label), int((label == np.arange(s.n)).sum())
