"""Set 2 in parts: a reference set that one record table cannot hold is indexed as contiguous
sequence ranges that share one geometry, and every launch walks them.  The tunable
part_buckets_log2 caps a part's table, so that small sets reach the splitting code; results
must equal the oracle's and those of one index."""

import os

import numpy as np
import pytest

import _dedup
import _oracle
from compairr_amd import HipOverlap, Options, synth
from compairr_amd import hip as hipmod
from compairr_amd.sets import RepertoireSet
from conftest import (expected_of, expected_pairs_of, load_manifest, run_cli, sorted_pairs,
                      warnings_of)

pytestmark = pytest.mark.gpu

FULL = dict(n_v_genes=synth.N_V, n_j_genes=synth.N_J)


def part_capacity(log2, delta=1):
    """Sequences one part holds when its table may have 2^log2 buckets (70 % rule x 2^delta)."""
    return 70 * (1 << (log2 - delta)) // 100


def run(a, b, opt, log2=None, device=False, tun=None):
    """matrix (or f64 matrix), stats, sorted pairs and the number of parts of one context"""
    with HipOverlap(opt) as h:
        for k, v in (tun or {}).items():
            h.set_tunable(k, v)
        if log2 is not None:
            h.set_tunable("part_buckets_log2", log2)
        if device:
            vb, keep = h.device_view(b)
            h.set_reference_device(vb, a.longest)
            del keep
        else:
            h.set_reference(b, a.longest)
        h.set_queries(a)
        if opt.score == "ratio" and not opt.ignore_counts:
            m = h.overlap_matrix_f64()
        else:
            m = h.overlap_matrix()
        st = h.stats()
        pairs = h.overlap_pairs()
        return m, st, pairs, h.get_tunable("reference_parts")


def slice_set(s, lo, hi):
    """Sequences lo .. hi - 1 of s, same repertoire and gene numbering (same n_repertoires)."""
    o = s.offsets
    return RepertoireSet(residues=s.residues[int(o[lo]):int(o[hi])], offsets=o[lo:hi + 1] - o[lo],
                         v_gene=s.v_gene[lo:hi], j_gene=s.j_gene[lo:hi],
                         repertoire=s.repertoire[lo:hi], count=s.count[lo:hi],
                         repertoire_ids=list(s.repertoire_ids), v_names=s.v_names, j_names=s.j_names,
                         alphabet=s.alphabet)


def check_against_oracle(a, b, opt, log2, device=False, tun=None):
    m, st, pairs, parts = run(a, b, opt, log2, device, tun)
    assert parts > 1, (log2, b.n)
    want, ost = _oracle.overlap(a, b, opt, threads=4)
    if opt.score == "ratio" and not opt.ignore_counts:
        assert np.allclose(m, want, rtol=1e-12, atol=0)
    else:
        assert np.array_equal(m, _oracle.integer_cells(want, opt))
    assert st.matches == ost.matches
    assert np.array_equal(pairs, _oracle.pairs(a, b, opt))
    return m, st


CONFIGS = [
    ("aa_d0", dict(differences=0), False),
    ("aa_d1", dict(differences=1), False),
    ("aa_d1_i", dict(differences=1, indels=True), False),
    ("aa_d2", dict(differences=2), False),
    ("nt_d1", dict(differences=1), True),
    ("nt_d2", dict(differences=2, ignore_genes=True), True),
    ("aa_d1_g", dict(differences=1, ignore_genes=True), False),
    ("aa_d1_f", dict(differences=1, ignore_counts=True), False),
    ("aa_d1_x", dict(differences=1, existence=True), False),
]


@pytest.mark.parametrize("log2", [6, 8, 10])
@pytest.mark.parametrize("name,opt,nt", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_parts_match_the_oracle(name, opt, nt, log2):
    d2 = opt["differences"] == 2
    n = 600 if d2 else 3000
    nrep = 1 if opt.get("existence") else 6
    a = synth.make_set(n // 2 if opt.get("existence") else n, 61, prefix="A", nucleotides=nt,
                       pool_size=n // 3, n_repertoires=nrep)
    b = synth.make_set(n + 37, 62, prefix="B", nucleotides=nt, pool_size=n // 3, n_repertoires=5)
    o = Options(nucleotides=nt, **opt, **FULL)
    check_against_oracle(a, b, o, log2)
    check_against_oracle(b, b, o, log2)           # one-file mode: duplicates straddle the parts


@pytest.mark.parametrize("score", ["product", "ratio", "min", "max", "mean", "MH", "jaccard"])
def test_parts_every_score(score):
    a = synth.make_set(2500, 71, prefix="A", pool_size=800)
    b = synth.make_set(2600, 72, prefix="B", pool_size=800)
    d = 0 if score in ("MH", "jaccard") else 1        # (defined at d = 0 only)
    check_against_oracle(a, b, Options(differences=d, score=score, **FULL), 8)


def test_parts_tiny_adversarial_and_device_resident():
    """homopolymer runs and many exact duplicates, two sequences per part; and a reference
    handed over from device memory"""
    for seed in range(3):
        x = synth.tiny_set(200, seed, letters=2, max_len=6)
        y = synth.tiny_set(180, seed + 50, letters=2, max_len=6)
        for d, indels in ((0, False), (1, False), (1, True), (2, False)):
            o = Options(differences=d, indels=indels, n_v_genes=2, n_j_genes=2)
            check_against_oracle(x, y, o, 3)
    a = synth.make_set(3000, 81, prefix="A", pool_size=1000)
    b = synth.make_set(3100, 82, prefix="B", pool_size=1000)
    for opt in (dict(differences=1, indels=True), dict(differences=0)):
        check_against_oracle(a, b, Options(**opt, **FULL), 7, device=True)


def test_one_part_by_default_and_tunable_rules():
    a = synth.make_set(2000, 91, prefix="A", pool_size=500)
    b = synth.make_set(2000, 92, prefix="B", pool_size=500)
    o = Options(differences=1, **FULL)
    with HipOverlap(o) as h:
        assert h.get_tunable("part_buckets_log2") == 30
        assert h.get_tunable("reference_parts") == 0
        for bad in (1, 31):
            with pytest.raises(hipmod.HipError) as e:
                h.set_tunable("part_buckets_log2", bad)
            assert e.value.code == 1                      # CMPR_EINVAL
        h.set_reference(b, a.longest)
        assert h.get_tunable("reference_parts") == 1
        with pytest.raises(hipmod.HipError) as e:
            h.set_tunable("part_buckets_log2", 8)
        assert e.value.code == 5                          # CMPR_ESTATE
    with HipOverlap(o) as h:                               # a part below one table's bucket multiple
        h.set_tunable("table_log2_delta", 3)
        h.set_tunable("part_buckets_log2", 2)
        with pytest.raises(hipmod.HipError):
            h.set_reference(b, a.longest)
    # the part count follows the cap: at most part_capacity sequences per part
    for log2 in (6, 8, 10):
        with HipOverlap(o) as h:
            h.set_tunable("part_buckets_log2", log2)
            h.set_reference(b, a.longest)
            P = h.get_tunable("reference_parts")
            assert -(-b.n // P) <= part_capacity(log2) and P >= -(-b.n // part_capacity(log2))


def test_count_duplicates_across_parts():
    """duplicates whose earlier copy lies in another part: the resident set and a passed-in set"""
    for genes in (True, False):
        a = synth.make_set(4000, 101, prefix="A", pool_size=300, n_repertoires=3)
        b = synth.make_set(5000, 102, prefix="B", pool_size=300, n_repertoires=2)
        o = Options(differences=1, ignore_genes=not genes, **FULL)
        _, ost = _oracle.overlap(a, b, o)
        assert ost.dup_set1 > 20 and ost.dup_set2 > 20
        for log2 in (4, 6, 8, 10):
            with HipOverlap(o) as h:
                h.set_tunable("part_buckets_log2", log2)
                assert h.count_duplicates(a) == ost.dup_set1        # no reference resident
                h.set_reference(b, a.longest)
                assert h.get_tunable("reference_parts") > 1
                assert h.count_duplicates() == ost.dup_set2
                assert h.count_duplicates(a) == ost.dup_set1
    # buckets with long runs of equal records; the resident path (in one part and in many) and the passed-in
    # path (a table of its own, in parts too) agree with each other, with the oracle and with the dedup model
    t = synth.tiny_set(500, 3, letters=2, max_len=4)
    for genes in (True, False):
        o = Options(differences=0, ignore_genes=not genes, n_v_genes=2, n_j_genes=2)
        _, ost = _oracle.overlap(t, t, o)
        want = _dedup.model(t, o)[2]
        assert want == ost.dup_set2 > 100
        for log2 in (None, 4):
            with HipOverlap(o) as h:
                if log2:
                    h.set_tunable("part_buckets_log2", log2)
                h.set_reference(t, 0)
                assert (h.get_tunable("reference_parts") > 1) == bool(log2)
                assert h.count_duplicates() == want
                assert h.count_duplicates(t) == want


@pytest.mark.parametrize("name,opt,nt", [("aa_d1", dict(differences=1), False),
                                         ("aa_d0", dict(differences=0), False),
                                         ("nt_d2", dict(differences=2), True)])
def test_parts_add_up_to_separate_contexts(name, opt, nt):
    """the matrix over parts = the sum of the matrices of contexts given one slice of set 2 each"""
    n = 800 if opt["differences"] == 2 else 4000
    a = synth.make_set(n, 111, prefix="A", nucleotides=nt, pool_size=n // 3)
    b = synth.make_set(n + 5, 112, prefix="B", nucleotides=nt, pool_size=n // 3)
    o = Options(nucleotides=nt, **opt, **FULL)
    whole, st, _, parts = run(a, b, o, 8)
    assert parts > 1
    cuts = np.linspace(0, b.n, 4).astype(int)
    total = sum(run(a, slice_set(b, lo, hi), o)[0] for lo, hi in zip(cuts[:-1], cuts[1:]))
    assert np.array_equal(total, whole)
    one, st1, _, p1 = run(a, b, o)
    assert p1 == 1 and np.array_equal(one, whole)
    # (every part's pass tests every variant: the counters are summed over the passes)
    assert (st.matches, st.variants, st.queries) == (st1.matches, parts * st1.variants, st1.queries)


@pytest.mark.parametrize("opt", [dict(differences=1), dict(differences=1, indels=True)])
def test_work_shards_compose_with_parts(opt):
    """each work shard does its share of the slices for every part: the shards add up"""
    a = synth.make_set(6000, 121, prefix="A", pool_size=2000)
    b = synth.make_set(6000, 122, prefix="B", pool_size=2000)
    o = Options(**opt, **FULL)
    whole, st, _, parts = run(a, b, o, 9)
    assert parts > 1
    want, _ = _oracle.overlap(a, b, o, threads=4)
    assert np.array_equal(whole, _oracle.integer_cells(want, o))
    shards = [run(a, b, o, 9, tun={"work_shard_count": 3, "work_shard_index": i}) for i in range(3)]
    assert np.array_equal(sum(s[0] for s in shards), whole)
    assert sum(s[1].matches for s in shards) == st.matches


def test_repeated_and_device_launches_over_parts():
    """launches back to back (the no-redo shortcut, device output) give the same matrix"""
    import torch
    a = synth.make_set(5000, 131, prefix="A", pool_size=1500)
    b = synth.make_set(5000, 132, prefix="B", pool_size=1500)
    o = Options(differences=1, **FULL)
    with HipOverlap(o) as h:
        h.set_tunable("part_buckets_log2", 8)
        h.set_reference(b, a.longest)
        h.set_queries(a)
        first = h.overlap_matrix()
        for _ in range(4):
            assert np.array_equal(h.overlap_matrix(), first)
        d = torch.zeros(first.size, dtype=torch.int64, device="cuda")
        s = torch.cuda.Stream()
        for _ in range(3):
            h.overlap_matrix_device(d.data_ptr(), s.cuda_stream)
        s.synchronize()
        h.stats()
        assert np.array_equal(d.cpu().numpy().view(np.uint64).reshape(first.shape), first)
        assert len(h.kernel_times(8)[0]) >= 3


@pytest.mark.parametrize("opt,nt,tun", [(dict(differences=1), False, {}),
                                        (dict(differences=1, indels=True), False, {}),
                                        (dict(differences=1), True, {"variant": 1})],
                         ids=["rows", "rows_indels", "sliced_nt"])
def test_positives_overflow_in_every_part(opt, nt, tun):
    """a positives buffer of 64 entries: every part's pass overflows it, its redo pass (or inline
    resolve) does the part, and the counters of the passes still add up"""
    a = synth.make_set(4000, 141, prefix="A", nucleotides=nt, pool_size=1000)
    b = synth.make_set(4000, 142, prefix="B", nucleotides=nt, pool_size=1000)
    o = Options(nucleotides=nt, **opt, **FULL)
    tun = dict(tun, pos_capacity=64, pos_grow=0)
    m, st = check_against_oracle(a, b, o, 8, tun=tun)
    one, st1, _, _ = run(a, b, o, tun=tun)
    assert np.array_equal(m, one) and st.matches == st1.matches
    with HipOverlap(o) as h:                       # launches back to back on an overflowing buffer
        for k, v in tun.items():
            h.set_tunable(k, v)
        h.set_tunable("part_buckets_log2", 8)
        h.set_reference(b, a.longest)
        h.set_queries(a)
        for _ in range(3):
            assert np.array_equal(h.overlap_matrix(), m)
            assert h.stats().matches == st.matches


def test_empty_launch_reports_zero_counters():
    """a step that launches nothing (an empty query set) reports zero counters, not a previous step's"""
    a = synth.make_set(3000, 151, prefix="A", pool_size=1000)
    b = synth.make_set(3000, 152, prefix="B", pool_size=1000)
    with HipOverlap(Options(differences=1, **FULL)) as h:
        h.set_tunable("part_buckets_log2", 8)
        h.set_reference(b, a.longest)
        h.set_queries(a)
        assert h.overlap_matrix().sum() > 0 and h.stats().matches > 0
        h.set_queries(slice_set(a, 0, 0))
        h.overlap_matrix()
        st = h.stats()
        assert (st.matches, st.variants, st.bloom_positive) == (0, 0, 0)


# ---- the golden vectors through bin/compairr, set 2 in 2 .. 16 parts, set 1 in 2 .. 4 batches ----

def _d_of(case):
    a = case["args"].split()
    return int(a[a.index("-d") + 1]) if "-d" in a else 0


CASES = [c for c in load_manifest() if c["exit"] == 0 and _d_of(c) <= 2]
# (--devices: the cases of tests/test_gpu_parity.py's sharded run)
DEVICE_CASES = [c for c in CASES if "ratio" not in c["args"] and c["name"].startswith(
    ("rand_aa_d1", "tiny_nt_d2", "x_aa_d1", "x_nt_d2", "x_readme", "p_x_", "p_rand_nt", "p_tiny_aa",
     "c_clus_aa_d1", "c_clus_nt_d2", "edge_dups", "ref_test_sh"))]


def _lines(case, k):
    """sequences in input file k of a case (data lines)"""
    path = os.path.join(os.path.dirname(__file__), "golden", "inputs", case["files"][k])
    with open(path, errors="replace") as fh:
        lines = [l for l in fh]
    while lines and lines[0][:1] in ("#", "@"):       # (comment lines in front of the header)
        lines.pop(0)
    return max(0, sum(1 for l in lines if l.strip()) - 1)


def _table_buckets(n, delta=1):
    s = 1
    while 70 * s < 100 * n:
        s <<= 1
    return max(s << delta, 4)


def _parts(n, log2, delta=1):
    """ref_index.hip choose_parts"""
    m0 = part_capacity(log2, delta)
    if n <= m0:
        return 1
    best = None
    for k in range(4):
        if log2 - k < 2:
            break
        m = part_capacity(log2 - k, delta)
        if m == 0:
            break
        P = -(-n // m)
        total = P * _table_buckets(-(-n // P), delta)
        if best is None or total < best[1]:
            best = (P, total)
    return best[0]


def _log2_for(n2):
    """the smallest cap that leaves set 2 in 2 .. 16 parts (one where it holds fewer than two sequences)"""
    for log2 in range(2, 31):
        if 2 <= _parts(n2, log2) <= 16:
            return log2
    return 30


def _logged_parts(log):
    """(parts, batches) of the log's "Index parts:" line, (1, 1) without one"""
    with open(log, errors="replace") as fh:
        for l in fh:
            if l.startswith("Index parts:"):
                w = l.split()
                return int(w[5]), int(w[10])
    return 1, 1


@pytest.mark.parametrize("case,devices", [(c, None) for c in CASES] + [(c, "0,0") for c in DEVICE_CASES],
                         ids=[c["name"] for c in CASES] + [c["name"] + "-devices" for c in DEVICE_CASES])
def test_cli_golden_with_reference_in_parts(case, devices, tmp_path, monkeypatch):
    n1, n2 = _lines(case, 0), _lines(case, -1)
    monkeypatch.setenv("COMPAIRR_HIP_PART_BUCKETS_LOG2", str(_log2_for(n2)))
    if n1 >= 2:
        monkeypatch.setenv("COMPAIRR_QUERY_BATCH", str(-(-n1 // 3)))
    log = str(tmp_path / "log.txt")
    pairs = str(tmp_path / "pairs.tsv")
    p = run_cli("bin/compairr", case, log=log, pairs=pairs,
                extra=["--devices", devices] if devices else [])
    assert p.returncode == 0, p.stderr.decode()
    assert warnings_of(log) == case["warnings"]
    parts, batches = _logged_parts(log)
    if n2 >= 3:
        assert 2 <= parts <= 16, (n2, parts)
    if n1 >= 3:
        assert 2 <= batches <= (4 if devices is None else 8), (n1, batches)
    if case.get("pairs"):
        assert sorted_pairs(pairs) == expected_pairs_of(case)
    if "ratio" in case["args"]:
        got = [l.split(b"\t") for l in p.stdout.splitlines()]
        exp = [l.split(b"\t") for l in expected_of(case).splitlines()]
        assert got[0] == exp[0]
        for g, e in zip(got[1:], exp[1:]):
            assert g[0] == e[0]
            assert np.allclose([float(x) for x in g[1:]], [float(x) for x in e[1:]], rtol=1e-9, atol=0)
        return
    assert p.stdout == expected_of(case)
