"""Parity at the lengths where the query layout and the probe kernels of the hashed path change form.

Everything below is decided from Lcap = zpos - 3 (cmpr_layout_queries: `Lcap`; ref_index.hip sets zpos from the
longest sequence of set 2 and the `longest_query` given to cmpr_set_reference, and no query may be longer), so a
ladder of set pairs whose longest sequence IS a chosen L (tests/_ladder.py) walks every decision on both sides.

Amino acids (A = 20), from the code:
  * 24            the top of compairr_amd.synth's sets: the control.
  * 28 | 29       `rec_hash` = rows_rec && recompute_on && Lcap <= 28: the query's hash rides in bytes 28 .. 35 of
                  its record (scatter_kernel; kernels_rows.h reads 7 words of residues), beyond it the probe
                  kernel hashes the record itself.  record_tiles reads back 1 | 2.
  * 32 | 33       `rows_rec` needs Lcap <= 32 (31 with -i: 31 | 32): record tiles give way to per-slot arrays,
                  record_tiles reads back 0.  REC_RES = 32 is also what a RefRec holds: from 33 on verify_candidate
                  reads the hit's residues past the 32nd where set 2 lies (`M > REC_RES`).
  * 33 | 34       `own_np_want` = max(3, (Lcap + 30) / 16) goes 3 -> 4.  The modes of d = 1 on rows (`lmode` 1, 2:
                  while recompute_on) keep own_np = 3, so from 34 to 36 a sequence with length + (offset & 15) > 48
                  does not fit its pieces (own_load `fits`) and is read where it lies; `lmode` 3 (three pieces,
                  any option set) ends at 33.
  * 36 | 37       QueryRec holds 36 residues: `recompute_on` = Lcap <= 36 goes off, `lmode` 1 / 2 -> 0, QAux is
                  scattered, and route_record_bytes = sizeof(QueryRec) + 16 * ceil((L - 36) / 16) goes 64 -> 80.
  * 39 | 40       make_plan shrinks the slice of variant 2 (pinned as a decision by test_lds_decisions_gpu.py).
  * 49 | 50, 65 | 66, 81 | 82     own_np_want 4 -> 5 -> 6 -> 7 (OWN_NP_MAX).
  * 52 | 53, 68 | 69              route_record_bytes 80 -> 96 -> 112 (the ladder holds 52 | 53).
  * 73 | 74       `zob_lds`: (20 * (Lcap + 3) + genes) * 8 <= 12288 with the 5 genes of these sets, and with -g.
  * 97 | 98 .. 112 | 113          seven pieces hold length + (offset & 15) <= 112: up to 97 every sequence fits,
                  from 98 some do not, from 113 none of length L does.
Nucleotides (A = 4): 33 | 34 and 36 | 37 as above; 72 the top of synth; 96 | 97 RESPACK_MAX (pair rows of d = 2 ->
single rows, an item holds 96 residues); 97 .. 113 the own pieces; 128 | 129 REC_RES_NT (a record's packed
residues end); 150 as a top.  Not covered: the `zob_lds` edge of nucleotides (near 380) and amino acids at d = 2
beyond 40 (the oracle takes 9 s at 113).

The declared length is moved apart from the data (test_declared_length_moves_the_data_does_not), the record
edges are crossed routed and sharded, and the residues of a device view are handed over at byte phases 1, 3, 8, 15
of a 16-byte line: own_load and validate_res_kernel then read them where they lie.  On the ladder a wrong candidate
of the record table never gets as far as the residues behind REC_RES (it fails inside the record), so one test
builds sets that agree inside the record and differ only behind it.  No listed layout refuses any case up to these
lengths.  Every comparison is exact."""

import functools

import numpy as np
import pytest

import _distance
import _ladder
import _oracle
from _routed import routed_contexts
from compairr_amd import HipOverlap, Options, synth
from compairr_amd import hip as hipmod
from test_gpu_parity import LAYOUTS, NT_LAYOUTS

pytestmark = pytest.mark.gpu

FULL = dict(n_v_genes=synth.N_V, n_j_genes=synth.N_J)
CASES = _ladder.ladder_cases()
LADDER_LAYOUTS = ([("auto", {}), ("variant0", {"variant": 0}), ("variant1", {"variant": 1}), ("variant2", {"variant": 2})] +
                  [(name, LAYOUTS[name]) for name in ("rows_arrays", "rows_records_hashed_here", "rows_layout_r5",
                                                      "rows_tiny_k3")] +
                  [("zob_in_memory", {"layout_zob_lds": 0}), ("narrow_upload", {"narrow_upload": 1})])
NT_D2_LAYOUTS = [(name, NT_LAYOUTS[name]) for name in ("rows_single_d2", "lds_items_k3")]


def csr_of(n1, pairs):
    """(row_start, hits) of a pair list sorted by (query, hit)"""
    row_start = np.zeros(n1 + 1, dtype=np.uint64)
    np.cumsum(np.bincount(pairs[:, 0], minlength=n1), out=row_start[1:])
    return row_start, pairs[:, 1].astype(np.uint32)


def wanted(a, b, o, with_pairs=True):
    cells, ost = _oracle.overlap(a, b, o, threads=8)
    out = {"cells": _oracle.integer_cells(cells, o), "matches": ost.matches, "variants": ost.variants}
    if with_pairs:
        out["pairs"] = _oracle.pairs(a, b, o)
        assert len(out["pairs"]) == ost.matches
        out["row_start"], out["hits"] = csr_of(a.n, out["pairs"])
        out["distance"] = _distance.edge_distances(a, b, out["row_start"], out["hits"])
    return out


def compare(a, b, o, tun, want, tag):
    with HipOverlap(o) as h:
        for k, v in tun.items():
            h.set_tunable(k, v)
        h.set_reference(b, a.longest)
        h.set_queries(a)
        assert np.array_equal(h.overlap_matrix(), want["cells"]), tag
        st = h.stats()
        assert (st.matches, st.variants) == (want["matches"], want["variants"]), tag
        if "pairs" in want:
            assert np.array_equal(h.overlap_pairs(), want["pairs"]), tag
            row_start, hits, distance = h.neighbors_distance()
            assert np.array_equal(row_start, want["row_start"]), tag
            assert np.array_equal(hits, want["hits"]), tag
            assert np.array_equal(distance, want["distance"]), tag


# ---- a. the ladder ----

@pytest.mark.parametrize("case", CASES, ids=_ladder.case_id)
def test_ladder(case):
    nt, L, name, seed = case
    a, b = _ladder.ladder_sets(L, nt, seed)
    o = _ladder.options_of(case)
    want = wanted(a, b, o)
    assert want["matches"] > 0
    layouts = LADDER_LAYOUTS + (NT_D2_LAYOUTS if nt and name == "d2" else [])
    for layout, tun in layouts:                  # (every layout runs: none is left out, none may refuse)
        compare(a, b, o, tun, want, (_ladder.case_id(case), layout))
    compare(a, a, o, {}, wanted(a, a, o, with_pairs=False), (_ladder.case_id(case), "one file"))


# ---- b. both sides are really taken ----

def record_tiles_of(L, indels):
    case = (False, L, "d1i" if indels else "d1", L + (2 if indels else 1))
    a, b = _ladder.ladder_sets(L, False, case[3])
    with HipOverlap(_ladder.options_of(case)) as h:
        h.set_reference(b, a.longest)
        h.set_queries(a)
        return h.get_tunable("record_tiles")


def routed_record_bytes(L):
    import torch
    case = (False, L, "d1", L + 1)
    a, b = _ladder.ladder_sets(L, False, case[3])
    with HipOverlap(_ladder.options_of(case)) as h:
        h.set_tunable("work_shard_count", 3)
        h.set_tunable("work_shard_index", 0)
        h.set_reference(b, a.longest)
        counts, rb, _ = h.route_queries(a, 0, 3)
        buf = torch.empty(max(int(counts.sum()), 1) * rb, dtype=torch.uint8, device="cuda")
        h.route_pack(buf.data_ptr(), int(counts.sum()) * rb)
        torch.cuda.synchronize()
        return rb


def test_both_sides_of_the_record_edges_are_taken():
    assert (record_tiles_of(28, False), record_tiles_of(29, False)) == (1, 2)
    assert record_tiles_of(32, False) != 0 and record_tiles_of(33, False) == 0
    assert record_tiles_of(31, True) != 0 and record_tiles_of(32, True) == 0
    assert [routed_record_bytes(L) for L in (36, 37, 52, 53)] == [64, 80, 80, 96]


# ---- c. the declared length moves, the data does not ----

@functools.lru_cache(maxsize=None)
def synth_sets(nt):
    n = 1500 if nt else 3000
    return (synth.make_set(n, 1, prefix="A", nucleotides=nt, pool_size=1000),
            synth.make_set(n, 2, prefix="B", nucleotides=nt, pool_size=1000))


@pytest.mark.parametrize("name", list(_ladder.OPTION_SETS))
@pytest.mark.parametrize("nt", [False, True], ids=["aa", "nt"])
def test_declared_length_moves_the_data_does_not(nt, name):
    """(a declared length below the longest query is no declaration: those values of the ladder fall together at
    the longest query)"""
    a, b = synth_sets(nt)
    d, indels = _ladder.OPTION_SETS[name]
    o = Options(differences=d, indels=indels, nucleotides=nt, **FULL)
    cells, ost = _oracle.overlap(a, b, o, threads=8)
    cells, pairs = _oracle.integer_cells(cells, o), _oracle.pairs(a, b, o)
    assert ost.matches == len(pairs) > 0
    ladder = _ladder.NT_LADDER if nt else _ladder.AA_LADDER
    for declared in sorted({max(L, a.longest) for L in ladder}):
        with HipOverlap(o) as h:
            h.set_reference(b, declared)
            h.set_queries(a)
            assert np.array_equal(h.overlap_matrix(), cells), declared
            assert h.stats().matches == ost.matches, declared
            assert np.array_equal(h.overlap_pairs(), pairs), declared


# ---- d. routed and sharded at the record edges ----

@pytest.mark.parametrize("indels", [False, True], ids=["d1", "d1i"])
@pytest.mark.parametrize("L", [36, 37, 52, 53])
def test_routed_and_sharded_at_the_record_edges(L, indels):
    case = (False, L, "d1i" if indels else "d1", L + (2 if indels else 1))
    a, b = _ladder.ladder_sets(L, False, case[3])
    o = _ladder.options_of(case)
    want = wanted(a, b, o)

    def add_up(hs):
        parts = [(h.overlap_matrix(), h.stats().matches, h.overlap_pairs()) for h in hs]
        pairs = np.concatenate([p[2] for p in parts])
        assert np.array_equal(sum(p[0] for p in parts), want["cells"])
        assert sum(p[1] for p in parts) == want["matches"]
        assert np.array_equal(pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))], want["pairs"])

    hs = routed_contexts(a, b, o, 3, {})
    try:
        add_up(hs)
    finally:
        for h in hs:
            h.close()
    hs = []
    try:
        for index in range(3):
            h = HipOverlap(o)
            hs.append(h)
            h.set_tunable("work_shard_count", 3)
            h.set_tunable("work_shard_index", index)
            h.set_reference(b, a.longest)
            h.set_queries(a)
        add_up(hs)
    finally:
        for h in hs:
            h.close()


# ---- the tail behind a reference record decides ----
#
# A candidate reaches verify_candidate when its bucket and the 15 tag bits of its key agree with the variant's hash
# (REC_TAG_SHIFT): on the ladder sets a wrong candidate then always fails on the residues inside the record.  Here
# every sequence of both sets has one length, one V and one J gene and the SAME residues inside a record (REC_RES /
# REC_RES_NT of them), so a wrong candidate can fail only on the tail that is read where set 2 lies -- and with a
# filter eight times as dense as the default and d = 2 (282 000 variants per query of 40 amino acids) there are such
# candidates: Stats.hash_equal counts them, and the test asks that verification has said no at least once.

def shared_prefix_sets(nt, prefix, tail, n):
    from compairr_amd.sets import AA, NT, RepertoireSet
    A = 4 if nt else 20
    rng = np.random.default_rng([prefix, tail, A])
    head = rng.integers(0, A, size=prefix, dtype=np.uint8)
    bases = rng.integers(0, A, size=(n // 8, tail), dtype=np.uint8)
    out = []
    for which in (1, 2):
        r = np.random.default_rng([prefix, tail, A, which])
        t = bases[r.integers(0, len(bases), size=n)].copy()
        for _ in range(3):                       # up to three substitutions in the tail
            sel = np.flatnonzero(r.random(n) < 0.6)
            pos = r.integers(0, tail, size=len(sel))
            t[sel, pos] = (t[sel, pos] + r.integers(1, A, size=len(sel))) % A
        rows = np.concatenate([np.tile(head, (n, 1)), t], axis=1)
        out.append(RepertoireSet(rows.reshape(-1), np.arange(n + 1, dtype=np.uint64) * (prefix + tail),
                                 np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32),
                                 (np.arange(n) % 3).astype(np.uint32), r.integers(1, 10, size=n, dtype=np.uint64),
                                 ["%s%d" % ("AB"[which - 1], k + 1) for k in range(3)], ["V0"], ["J0"], NT if nt else AA))
    return out


@pytest.mark.parametrize("nt,prefix,tail,delta", [(False, 32, 8, -3), (False, 32, 16, -4), (True, 128, 8, -3)],
                         ids=["aa_tail8", "aa_tail16", "nt_tail8"])
def test_the_tail_behind_a_reference_record_decides(nt, prefix, tail, delta):
    """Measured on the library of this commit: 1 362 (aa_tail8), 2 987 (aa_tail16) and 435 (nt_tail8) candidates
    turned down under variant 1.  Nearly all of them fail inside the record all the same (a variant that changes a
    residue of the shared part): a library that takes amino-acid residues from REC_RES on as equal gives 1 (aa_tail8)
    and 2 (aa_tail16) matches too many under variant 1, none under the other two."""
    n = 1500
    DENSE = [("variant%d_dense" % v, {"variant": v, "bloom_bits_log2_delta": delta}) for v in (0, 1, 2)]
    a, b = shared_prefix_sets(nt, prefix, tail, n)
    o = Options(differences=2, nucleotides=nt, n_v_genes=1, n_j_genes=1)
    want = _oracle.integer_cells(_oracle.bruteforce(a, b, o), o)
    ta = a.residues.reshape(n, -1)[:, prefix:]
    tb = b.residues.reshape(n, -1)[:, prefix:]
    matches = int(((ta[:, None, :] != tb[None, :, :]).sum(axis=2) <= 2).sum())
    assert 0 < matches < n * n // 4
    rejected = {}
    for layout, tun in DENSE:
        with HipOverlap(o) as h:
            for k, v in tun.items():
                h.set_tunable(k, v)
            h.set_reference(b, a.longest)
            h.set_queries(a)
            got, st = h.overlap_matrix(), h.stats()
        rejected[layout] = st.hash_equal - st.matches
        print(layout, "candidates", st.hash_equal, "matches", st.matches, "bloom positives", st.bloom_positive)
        assert np.array_equal(got, want), layout
        assert st.matches == matches, layout
    assert max(rejected.values()) > 0, rejected


# ---- e. residues that are not 16-byte aligned ----

JUNK = 0xEE                                      # around the residues: no residue code of either alphabet


def unaligned_view(s, k):
    """HipOverlap.device_view with the residues k bytes behind a 16-byte line, inside a larger tensor"""
    import torch
    view, keep = HipOverlap.device_view(s)
    n = len(s.residues)
    big = torch.full((k + n + 64,), JUNK, dtype=torch.uint8, device="cuda")
    big[k:k + n] = keep[0]
    assert big.data_ptr() % 16 == 0 and 0 < k < 16
    view.residues = big.data_ptr() + k
    keep[0] = big
    torch.cuda.synchronize()
    return view, keep


def ladder_pair(L, name):
    case = (False, L, name, L + list(_ladder.OPTION_SETS).index(name))
    return _ladder.ladder_sets(L, False, case[3]) + (_ladder.options_of(case),)


UNALIGNED = {
    "aa5000_d1": lambda: (synth.make_set(5000, 1, prefix="A", pool_size=1000),
                          synth.make_set(5000, 2, prefix="B", pool_size=1000), Options(differences=1, **FULL)),
    "aa5000_d1i": lambda: (synth.make_set(5000, 1, prefix="A", pool_size=1000),
                           synth.make_set(5000, 2, prefix="B", pool_size=1000),
                           Options(differences=1, indels=True, **FULL)),
    "ladder37_d1": lambda: ladder_pair(37, "d1"),
    "ladder37_d1i": lambda: ladder_pair(37, "d1i"),
    "ladder98_d1": lambda: ladder_pair(98, "d1"),
    "ladder98_d1i": lambda: ladder_pair(98, "d1i"),
    "nt3000_d1": lambda: (synth.make_set(3000, 3, prefix="A", nucleotides=True, pool_size=800),
                          synth.make_set(3000, 4, prefix="B", nucleotides=True, pool_size=800),
                          Options(differences=1, nucleotides=True, **FULL)),
}


@functools.lru_cache(maxsize=None)
def host_path(name):
    """(a, b, options, matrix, pairs) of the host path -- itself held against the oracle's matrix"""
    a, b, o = UNALIGNED[name]()
    with HipOverlap(o) as h:
        h.set_reference(b, a.longest)
        h.set_queries(a)
        m, pairs = h.overlap_matrix(), h.overlap_pairs()
    want, ost = _oracle.overlap(a, b, o, threads=8)
    assert ost.matches == len(pairs) > 0 and np.array_equal(m, _oracle.integer_cells(want, o))
    return a, b, o, m, pairs


@pytest.mark.parametrize("k", [1, 3, 8, 15])
@pytest.mark.parametrize("name", sorted(UNALIGNED))
def test_queries_in_place_at_any_byte_phase(name, k):
    a, b, o, m, pairs = host_path(name)
    view, keep = unaligned_view(a, k)
    with HipOverlap(o) as h:
        h.set_reference(b, a.longest)
        h.set_queries_device(view)
        assert np.array_equal(h.overlap_matrix(), m)
        assert np.array_equal(h.overlap_pairs(), pairs)
    del keep


def test_calls_that_copy_the_set_at_byte_phase_3():
    import torch
    a, b, o, m, pairs = host_path("aa5000_d1")
    view_a, keep_a = unaligned_view(a, 3)
    view_b, keep_b = unaligned_view(b, 3)
    with HipOverlap(o) as h:
        h.set_reference_device(view_b, a.longest)
        h.set_queries(a)
        assert np.array_equal(h.overlap_matrix(), m) and np.array_equal(h.overlap_pairs(), pairs)
    with HipOverlap(o) as h:
        first, count, merged = h.deduplicate(a)
        d_first = torch.zeros(a.n, dtype=torch.int32, device="cuda")
        d_count = torch.zeros(a.n, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert h.deduplicate_device(view_a, a.n, d_first.data_ptr(), d_count.data_ptr()) == (len(first), merged)
        assert np.array_equal(d_first.cpu().numpy().view(np.uint32)[:len(first)], first)
        assert np.array_equal(d_count.cpu().numpy().view(np.uint64)[:len(first)], count)
    with HipOverlap(o) as h:
        row_start, hits, distance = h.hamming_neighbors(a, b, 3)
        assert len(hits) > 0
        d_rows = torch.zeros(a.n + 1, dtype=torch.int64, device="cuda")
        d_hits = torch.zeros(len(hits), dtype=torch.int32, device="cuda")
        d_dist = torch.zeros(len(hits), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        assert h.hamming_neighbors_device(view_a, view_b, 3, len(hits), d_rows.data_ptr(), d_hits.data_ptr(),
                                          d_dist.data_ptr()) == len(hits)
        assert np.array_equal(d_rows.cpu().numpy().view(np.uint64), row_start)
        assert np.array_equal(d_hits.cpu().numpy().view(np.uint32), hits)
        assert np.array_equal(d_dist.cpu().numpy().view(np.uint16), distance)
    del keep_a, keep_b


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_a_residue_out_of_range_is_refused_at_byte_phase_5(where):
    a, b, o, _, _ = host_path("aa5000_d1")
    bad = a.subset(slice(0, a.n))
    bad.residues = bad.residues.copy()
    bad.residues[{"first": 0, "middle": len(bad.residues) // 2 + 1, "last": len(bad.residues) - 1}[where]] = 20
    view, keep = unaligned_view(bad, 5)
    with HipOverlap(o) as h:
        h.set_reference(b, a.longest)
        with pytest.raises(hipmod.HipError) as host:
            h.set_queries(bad)
        with pytest.raises(hipmod.HipError) as device:
            h.set_queries_device(view)
        assert (device.value.code, str(device.value)) == (host.value.code, str(host.value))
        assert host.value.code == 1 and "residue code out of range" in str(host.value)
    del keep
