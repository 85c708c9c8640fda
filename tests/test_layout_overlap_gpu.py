"""The layout of the next query set beside the launch on the previous one.

cmpr_set_queries* no longer waits for the previous set's launches at its start: the first half of the
layout (keys, sizes) runs while such a launch is still in flight on the caller's stream, and the wait
sits where the layout first writes what a launch reads.  These tests order the calls the way a
streaming caller does -- launch on a caller's stream, the next set handed over at once, nothing
synchronised in between -- and compare every matrix with the oracle's."""

import numpy as np
import pytest
import torch

import _oracle
from compairr_amd import HipOverlap, Options, synth
from compairr_amd import hip as hipmod

pytestmark = pytest.mark.gpu

FULL = dict(n_v_genes=synth.N_V, n_j_genes=synth.N_J)
POISON = -7                                    # what a matrix holds until a launch has written it


def oracle_cells(a, b, o):
    want, ost = _oracle.overlap(a, b, o, threads=8)
    return _oracle.integer_cells(want, o), ost


def rows_of(s, o):
    return s.n if o.existence else s.n_repertoires


def poisoned(rows, cols):
    return torch.full((rows * cols,), POISON, dtype=torch.int64, device="cuda")


def cells_of(t, shape):
    return t.cpu().numpy().astype(np.uint64).reshape(shape)


def stream_through(h, sets, b, o, rounds, from_host=False):
    """`rounds` times over `sets`: set the queries, launch on a caller's stream into a matrix of its own,
    go on at once.  Returns [(index of the set, matrix)] once the stream is through."""
    views = None if from_host else [HipOverlap.device_view(s) for s in sets]
    mats = [poisoned(rows_of(sets[k % len(sets)], o), b.n_repertoires) for k in range(rounds * len(sets))]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for k, m in enumerate(mats):
        i = k % len(sets)
        if from_host:
            h.set_queries(sets[i])
        else:
            h.set_queries_device(views[i][0])
        assert h.shape == (rows_of(sets[i], o), b.n_repertoires)
        h.overlap_matrix_device(m.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    return [(k % len(sets), cells_of(m, (rows_of(sets[k % len(sets)], o), b.n_repertoires)))
            for k, m in enumerate(mats)]


def amino_sets(n_a, n_b, n_ref, reps=16):
    """two query sets of different sizes and length mixes (the second: the longer half of another draw) and
    the reference"""
    a = synth.make_set(n_a, 41, prefix="A", pool_size=4000, n_repertoires=reps)
    b0 = synth.make_set(2 * n_b, 42, prefix="A", pool_size=4000, n_repertoires=reps)
    b = b0.subset(np.argsort(-b0.lengths, kind="stable")[:n_b])
    ref = synth.make_set(n_ref, 43, prefix="B", pool_size=4000)
    return a, b, ref


def nucleotide_sets(n_a, n_b, n_ref):
    a = synth.make_set(n_a, 44, prefix="A", nucleotides=True, pool_size=2000)
    b0 = synth.make_set(2 * n_b, 45, prefix="A", nucleotides=True, pool_size=2000)
    b = b0.subset(np.argsort(b0.lengths, kind="stable")[:n_b])         # (the shorter half)
    ref = synth.make_set(n_ref, 46, prefix="B", nucleotides=True, pool_size=2000)
    return a, b, ref


def long_sets():
    """amino acids beyond the 36 residues of a query's record: nothing is recomputed from records"""
    whole = synth.tiny_set(2000, 51, letters=3, min_len=30, max_len=44, n_repertoires=3)

    def every_third_changed(s):                # (random sequences of this length have no neighbours of their own)
        s.residues = s.residues.copy()
        last = s.offsets[1:][::3].astype(np.int64) - 1
        s.residues[last] = (s.residues[last] + 1) % 20
        return s

    return (every_third_changed(whole.subset(slice(300, 1200))), every_third_changed(whole.subset(slice(1000, 1400))),
            whole.subset(slice(0, 1200)))


# the layouts that differ in what a launch reads
CASES = {
    "aa_d1": (lambda: amino_sets(20000, 7000, 30000), dict(differences=1, **FULL), {}),
    "aa_d1_i": (lambda: amino_sets(20000, 7000, 30000), dict(differences=1, indels=True, **FULL), {}),
    "aa_d0": (lambda: amino_sets(20000, 7000, 30000), dict(differences=0, **FULL), {}),
    "aa_d2": (lambda: amino_sets(3000, 1200, 3000), dict(differences=2, **FULL), {}),
    "nt_d1": (lambda: nucleotide_sets(8000, 3000, 10000), dict(differences=1, nucleotides=True, **FULL), {}),
    "nt_d2": (lambda: nucleotide_sets(1500, 700, 1500),
              dict(differences=2, nucleotides=True, ignore_genes=True, **FULL), {}),
    "aa_long": (long_sets, dict(differences=1, n_v_genes=2, n_j_genes=2), {}),
    "aa_d1_no_record_tiles": (lambda: amino_sets(20000, 7000, 30000), dict(differences=1, **FULL),
                              {"record_tiles": 0}),
    "aa_d1_x": (lambda: amino_sets(6000, 2500, 30000, reps=1), dict(differences=1, existence=True, **FULL), {}),
}


@pytest.mark.parametrize("from_host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_alternating_sets_with_launches_in_flight(name, from_host):
    make, opt, tun = CASES[name]
    a, b, ref = make()
    o = Options(**opt)
    wants = [oracle_cells(s, ref, o) for s in (a, b)]
    assert all(w[1].matches > 0 for w in wants)
    with HipOverlap(o) as h:
        for k, v in tun.items():
            h.set_tunable(k, v)
        h.set_reference(ref, max(a.longest, b.longest))
        got = stream_through(h, [a, b], ref, o, 6, from_host)
        assert len(got) == 12
        for step, (i, m) in enumerate(got):
            assert np.array_equal(m, wants[i][0]), (name, step, i)
        assert h.stats().matches == wants[1][1].matches          # (the last launch: set B)


@pytest.mark.parametrize("name", ["aa_d1", "aa_d1_i", "aa_d0"])
def test_alternating_sets_on_two_work_shards(name):
    make, opt, tun = CASES[name]
    a, b, ref = make()
    o = Options(**opt)
    wants = [oracle_cells(s, ref, o)[0] for s in (a, b)]
    parts = []
    for index in range(2):
        with HipOverlap(o) as h:
            h.set_tunable("work_shard_count", 2)
            h.set_tunable("work_shard_index", index)
            h.set_reference(ref, max(a.longest, b.longest))
            parts.append(stream_through(h, [a, b], ref, o, 6))
    for step in range(12):
        i = parts[0][step][0]
        assert np.array_equal(parts[0][step][1] + parts[1][step][1], wants[i]), (name, step)
        assert parts[0][step][1].sum() > 0 and parts[1][step][1].sum() > 0


@pytest.mark.parametrize("indels", [False, True])
def test_growth_behind_a_launch_in_flight(indels):
    """A small set and its launch, then at once a set large enough to reallocate both arenas and the
    resident buffers."""
    small = synth.make_set(600, 61, prefix="A", pool_size=4000)
    large = synth.make_set(150000, 62, prefix="A", pool_size=4000)
    ref = synth.make_set(30000, 43, prefix="B", pool_size=4000)
    o = Options(differences=1, indels=indels, **FULL)
    wants = [oracle_cells(s, ref, o)[0] for s in (small, large)]
    with HipOverlap(o) as h:
        h.set_reference(ref, max(small.longest, large.longest))
        got = stream_through(h, [small, large], ref, o, 1)
        for i, m in got:
            assert np.array_equal(m, wants[i]), i


def bad_residue(s):
    bad = s.subset(slice(0, s.n))
    bad.residues = bad.residues.copy()
    bad.residues[len(bad.residues) // 2] = 200
    return bad


def too_long(s, longest):
    """`s` with one sequence of longest + 3 residues in front"""
    from compairr_amd.sets import RepertoireSet
    extra = np.zeros(longest + 3, dtype=np.uint8)
    offs = np.concatenate([[0], s.offsets.astype(np.uint64) + np.uint64(len(extra))]).astype(np.uint64)
    one = lambda x: np.concatenate([x[:1], x])
    return RepertoireSet(np.concatenate([extra, s.residues]), offs, one(s.v_gene), one(s.j_gene),
                         one(s.repertoire), one(s.count), list(s.repertoire_ids), s.v_names, s.j_names,
                         s.alphabet)


@pytest.mark.parametrize("from_host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("what", ["residue", "too_long"])
def test_a_bad_set_while_a_launch_is_in_flight(what, from_host):
    a, b, ref = amino_sets(20000, 7000, 30000)
    o = Options(differences=1, **FULL)
    wants = [oracle_cells(s, ref, o)[0] for s in (a, b)]
    longest = max(a.longest, b.longest)
    bad = bad_residue(b) if what == "residue" else too_long(b, longest)
    # today's answers (compairr_hip.h; query_layout.hip verr_message)
    code, text = ((1, "residue code out of range") if what == "residue" else
                  (1, "query longer than the longest_query given to cmpr_set_reference"))

    def hand_over(h, s, keep):
        if from_host:
            h.set_queries(s)
        else:
            v, k = HipOverlap.device_view(s)
            keep.append(k)
            h.set_queries_device(v)

    for close_at_once in (False, True):
        keep = []
        h = HipOverlap(o)
        try:
            h.set_reference(ref, longest)
            stream = torch.cuda.Stream()
            m_a, m_b = poisoned(a.n_repertoires, ref.n_repertoires), poisoned(b.n_repertoires, ref.n_repertoires)
            bad_view = None if from_host else HipOverlap.device_view(bad)
            hand_over(h, a, keep)
            torch.cuda.synchronize()
            h.overlap_matrix_device(m_a.data_ptr(), stream.cuda_stream)
            with pytest.raises(hipmod.HipError) as e:
                if from_host:
                    h.set_queries(bad)
                else:
                    h.set_queries_device(bad_view[0])
            assert e.value.code == code and text in str(e.value)
            if close_at_once:
                h.close()                                          # (neither hangs nor faults)
                stream.synchronize()
                assert np.array_equal(cells_of(m_a, wants[0].shape), wants[0])
                continue
            with pytest.raises(hipmod.HipError) as e:              # no queries set
                h.overlap_matrix_device(m_b.data_ptr(), stream.cuda_stream)
            assert e.value.code == 5
            hand_over(h, b, keep)                                  # a good set is accepted
            h.overlap_matrix_device(m_b.data_ptr(), stream.cuda_stream)
            stream.synchronize()
            assert np.array_equal(cells_of(m_a, wants[0].shape), wants[0])      # the launch that was in flight
            assert np.array_equal(cells_of(m_b, wants[1].shape), wants[1])
        finally:
            h.close()


def test_sticky_overflow_is_reported_by_the_call_that_sets_the_next_queries():
    """An asynchronous launch without redo pass that overflowed, nobody asks cmpr_get_stats: the next
    cmpr_set_queries_device still fails with CMPR_ESTATE (now from the middle of the layout, where it waits for
    that launch), and the same call repeated succeeds."""
    a = synth.make_set(40000, 21, prefix="A", pool_size=8000)
    b = synth.make_set(40000, 22, prefix="B", pool_size=8000)
    nxt = synth.make_set(9000, 23, prefix="A", pool_size=8000)
    o = Options(differences=1, **FULL)
    want = oracle_cells(nxt, b, o)[0]
    with HipOverlap(o) as h:
        h.set_tunable("variant", 2)
        h.set_tunable("pos_segments", 1)
        h.set_tunable("pos_capacity", 64)
        h.set_reference(b, max(a.longest, nxt.longest))
        h.set_queries(a)
        t = poisoned(a.n_repertoires, b.n_repertoires)
        view, keep = HipOverlap.device_view(nxt)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        h.set_tunable("assume_never_overflows", 1)
        h.overlap_matrix_device(t.data_ptr(), s.cuda_stream)
        with pytest.raises(hipmod.HipError) as e:
            h.set_queries_device(view)
        assert e.value.code == 5                                   # CMPR_ESTATE
        assert "positives buffer overflowed in a launch without redo pass on the previous query set" in str(e.value)
        assert "repeat the call to set the new queries" in str(e.value)
        h.set_queries_device(view)                                 # the same call repeated
        m = poisoned(nxt.n_repertoires, b.n_repertoires)
        torch.cuda.synchronize()
        h.overlap_matrix_device(m.data_ptr(), s.cuda_stream)
        s.synchronize()
        assert np.array_equal(cells_of(m, want.shape), want)
        assert h.stats().matches == oracle_cells(nxt, b, o)[1].matches
        del keep
