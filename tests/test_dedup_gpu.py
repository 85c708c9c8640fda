"""cmpr_deduplicate / cmpr_deduplicate_device on the GPU: the recorded cases of the reference's --deduplicate
byte for byte, large sets of mostly duplicates against the Python model (tests/_dedup.py, tied to the
reference by tests/test_dedup_cpu.py), a skewed set whose heaviest class puts 8 192 adds on one sum, and the
contract of the entry points (capacity, counting only, empty set, errors, nothing resident disturbed)."""

import ctypes as C
import functools

import numpy as np
import pytest

import _dedup
import compairr_amd
from compairr_amd import HipError, HipOverlap, Options, RepertoireSet, synth
from compairr_amd.sets import AA

pytestmark = pytest.mark.gpu

CASES = _dedup.cases()
CMPR_EINVAL = 1


@pytest.mark.parametrize("tag_bits", (32, 2, 0))
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_recorded_cases_byte_for_byte(case, tag_bits):
    flags = _dedup.flags_of(case)
    s = _dedup.read_case(case)
    opt = _dedup.options_of(s, device=0, **flags)
    out, merged = compairr_amd.deduplicate(s, opt, tunables={"dedup_tag_bits": tag_bits})
    assert merged == case["merged"]
    assert out.dedup_tsv(ignore_genes=flags["ignore_genes"], cdr3=flags["cdr3"]) == _dedup.expected_of(case)
    if tag_bits == 32:
        with HipOverlap(opt) as h:
            assert h.count_duplicates(s) == merged


# ---- large sets of few distinct sequences ----

@functools.lru_cache(maxsize=None)
def big_set(nucleotides):
    return synth.tiny_set(200_000, 11 if nucleotides else 12, alphabet_size=4 if nucleotides else 20,
                          letters=3, max_len=8)


def tiny_options(nucleotides, genes=True, counts=True, **more):
    return Options(nucleotides=nucleotides, ignore_genes=not genes, ignore_counts=not counts, n_v_genes=2,
                   n_j_genes=2, device=0, **more)


def device_deduplicate(h, s, capacity=None):
    """cmpr_deduplicate_device on a copy of `s` in device memory: (first, count, merged)"""
    import torch
    view, keep = HipOverlap.device_view(s)
    cap = s.n if capacity is None else capacity
    d_first = torch.zeros(max(cap, 1), dtype=torch.int32, device="cuda")
    d_count = torch.zeros(max(cap, 1), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    unique, merged = h.deduplicate_device(view, cap, d_first.data_ptr(), d_count.data_ptr())
    k = min(cap, unique)
    assert unique + merged == s.n
    del keep
    return d_first.cpu().numpy().view(np.uint32)[:k], d_count.cpu().numpy().view(np.uint64)[:k], merged


@pytest.mark.parametrize("counts", (True, False), ids=("counts", "nocounts"))
@pytest.mark.parametrize("genes", (True, False), ids=("genes", "nogenes"))
@pytest.mark.parametrize("nucleotides", (False, True), ids=("aa", "nt"))
def test_mostly_duplicates_equal_the_model(nucleotides, genes, counts):
    s = big_set(nucleotides)
    opt = tiny_options(nucleotides, genes, counts)
    first, count, merged = _dedup.model(s, opt)
    assert merged > s.n // 3                    # (most sequences repeat another)
    with HipOverlap(opt) as h:
        for tag_bits in (32, 0):
            h.set_tunable("dedup_tag_bits", tag_bits)
            got = h.deduplicate(s)
            assert got[2] == merged, tag_bits
            assert np.array_equal(got[0], first) and np.array_equal(got[1], count), tag_bits
            dev = device_deduplicate(h, s)
            assert dev[2] == merged
            assert np.array_equal(dev[0], got[0]) and np.array_equal(dev[1], got[1]), tag_bits
        assert got[0].dtype == np.uint32 and got[1].dtype == np.uint64


# ---- one heavy class ----

HEAVY = 8192
BASE_COUNT = 1 << 40


@functools.lru_cache(maxsize=None)
def skewed_set():
    """20 000 sequences in a seeded random order: 8 192 copies of one sequence S in repertoire 0 (V 1, J 1)
    with counts 2^40 + k; S three times in repertoire 1; S with another V twice and with another J twice; S
    plus one residue twice; S with another last residue twice; the rest is a synthetic set of its own."""
    S = [AA.index(c) for c in "CASSLGQAYEQYF"]
    special = [(S, 1, 1, 0, BASE_COUNT + k) for k in range(HEAVY)]
    special += [(S, 1, 1, 1, 5 + k) for k in range(3)]
    special += [(S, 2, 1, 0, 100 + k) for k in range(2)] + [(S, 1, 2, 0, 200 + k) for k in range(2)]
    special += [(S + [AA.index("F")], 1, 1, 0, 300 + k) for k in range(2)]
    special += [(S[:-1] + [AA.index("W")], 1, 1, 0, 400 + k) for k in range(2)]
    bg = synth.make_set(20_000 - len(special), 5)
    off = bg.offsets.astype(np.int64)
    rows = special + [(bg.residues[off[i]:off[i + 1]].tolist(), int(bg.v_gene[i]), int(bg.j_gene[i]),
                       int(bg.repertoire[i]), int(bg.count[i])) for i in range(bg.n)]
    order = np.random.default_rng(20240).permutation(len(rows))
    rows = [rows[k] for k in order]
    res = np.array([c for r in rows for c in r[0]], dtype=np.uint8)
    offsets = np.zeros(len(rows) + 1, dtype=np.uint64)
    np.cumsum([len(r[0]) for r in rows], out=offsets[1:])
    return RepertoireSet(res, offsets, [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows],
                         np.array([r[4] for r in rows], dtype=np.uint64), list(bg.repertoire_ids), bg.v_names,
                         bg.j_names, AA), len(S)


@pytest.mark.parametrize("genes", (True, False), ids=("genes", "nogenes"))
def test_heavy_class_sums_exactly(genes):
    s, L = skewed_set()
    assert s.n == 20_000
    opt = Options(ignore_genes=not genes, n_v_genes=synth.N_V, n_j_genes=synth.N_J, device=0)
    with HipOverlap(opt) as h:
        first, count, merged = h.deduplicate(s)
    want = _dedup.model(s, opt)
    assert merged == want[2] and np.array_equal(first, want[0]) and np.array_equal(count, want[1])
    # the classes of S and of its neighbours, named one by one
    seq = [s.sequence(int(i)) for i in first]
    key = {(seq[k], int(s.repertoire[i]), int(s.v_gene[i]), int(s.j_gene[i])): int(count[k])
           for k, i in enumerate(first)}
    S = "CASSLGQAYEQYF"
    assert len(S) == L
    heavy = HEAVY * BASE_COUNT + HEAVY * (HEAVY - 1) // 2
    if genes:
        assert key[(S, 0, 1, 1)] == heavy
        assert key[(S, 0, 2, 1)] == 100 + 101 and key[(S, 0, 1, 2)] == 200 + 201
    else:
        # (one class: the entry carries the genes of whichever member comes first)
        got = [c for (q, r, _, _), c in key.items() if q == S and r == 0]
        assert got == [heavy + 100 + 101 + 200 + 201]
    assert [c for (q, r, _, _), c in key.items() if q == S and r == 1] == [5 + 6 + 7]       # never across repertoires
    assert [c for (q, r, _, _), c in key.items() if q == S + "F" and r == 0] == [300 + 301]
    assert [c for (q, r, _, _), c in key.items() if q == S[:-1] + "W" and r == 0] == [400 + 401]


# ---- the contract of the entry points ----

def raw_deduplicate(h, s, capacity, first, count):
    """cmpr_deduplicate as it is declared: (code, n_unique, merged)"""
    v = compairr_amd.hip._view(s)
    unique, merged = C.c_uint64(12345), C.c_uint64(12345)
    rc = h._lib.cmpr_deduplicate(h._ctx, C.byref(v), capacity, None if first is None else first.ctypes.data,
                                 None if count is None else count.ctypes.data, C.byref(unique), C.byref(merged))
    return rc, unique.value, merged.value


@functools.lru_cache(maxsize=None)
def small_set():
    return synth.tiny_set(5000, 3, letters=3, max_len=7)


def test_capacity_below_the_classes_writes_the_first_ones_and_nothing_behind():
    s, opt = small_set(), tiny_options(False)
    want = _dedup.model(s, opt)
    cap = 1000
    assert cap + 64 < len(want[0])
    first = np.full(cap + 64, 0xA5A5A5A5, dtype=np.uint32)
    count = np.full(cap + 64, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    with HipOverlap(opt) as h:
        assert raw_deduplicate(h, s, cap, first, count) == (0, len(want[0]), want[2])
        dev = device_deduplicate(h, s, cap)
        # (the device arrays have `cap` elements: what lies behind them is not the call's to write)
    assert np.array_equal(first[:cap], want[0][:cap]) and np.array_equal(count[:cap], want[1][:cap])
    assert (first[cap:] == 0xA5A5A5A5).all() and (count[cap:] == 0x5A5A5A5A5A5A5A5A).all()
    assert np.array_equal(dev[0], want[0][:cap]) and np.array_equal(dev[1], want[1][:cap]) and dev[2] == want[2]


def test_device_capacity_leaves_the_rest_of_the_arrays_alone():
    import torch
    s, opt = small_set(), tiny_options(False)
    want = _dedup.model(s, opt)
    cap = 777
    view, keep = HipOverlap.device_view(s)
    d_first = torch.full((cap + 64,), 0x25A5A5A5, dtype=torch.int32, device="cuda")
    d_count = torch.full((cap + 64,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with HipOverlap(opt) as h:
        assert h.deduplicate_device(view, cap, d_first.data_ptr(), d_count.data_ptr()) == (len(want[0]), want[2])
    first, count = d_first.cpu().numpy().view(np.uint32), d_count.cpu().numpy().view(np.uint64)
    assert np.array_equal(first[:cap], want[0][:cap]) and np.array_equal(count[:cap], want[1][:cap])
    assert (first[cap:] == 0x25A5A5A5).all() and (count[cap:] == 0x5A5A5A5A5A5A5A5A).all()


def test_counting_only():
    s, opt = small_set(), tiny_options(False)
    want = _dedup.model(s, opt)
    with HipOverlap(opt) as h:
        assert raw_deduplicate(h, s, 0, None, None) == (0, len(want[0]), want[2])
        view, keep = HipOverlap.device_view(s)
        assert h.deduplicate_device(view) == (len(want[0]), want[2])
        # either figure may be left out
        v = compairr_amd.hip._view(s)
        assert h._lib.cmpr_deduplicate(h._ctx, C.byref(v), 0, None, None, None, None) == 0
        # a capacity needs arrays
        assert raw_deduplicate(h, s, 10, None, None)[0] == CMPR_EINVAL


def test_empty_set_is_ok_with_zero_classes():
    z = lambda t: np.zeros(0, dtype=t)
    s = RepertoireSet(z(np.uint8), np.zeros(1, dtype=np.uint64), z(np.uint32), z(np.uint32), z(np.uint32),
                      z(np.uint64), ["T1"])
    with HipOverlap(tiny_options(False)) as h:
        first, count, merged = h.deduplicate(s)
        assert (len(first), len(count), merged) == (0, 0, 0)
        assert raw_deduplicate(h, s, 0, None, None) == (0, 0, 0)
        # the count alone: with nothing resident, and beside a resident reference
        assert h.count_duplicates(s) == 0
        h.set_reference(small_set(), small_set().longest)
        assert h.count_duplicates(s) == 0


def test_zero_count_fails_with_the_existing_message():
    s = synth.tiny_set(300, 4)
    s.count[123] = 0
    with HipOverlap(tiny_options(False)) as h:
        with pytest.raises(HipError) as e:
            h.deduplicate(s)
        assert e.value.code == CMPR_EINVAL and "duplicate_count must be >= 1" in str(e.value)
        with pytest.raises(HipError) as e:
            h.count_duplicates(s)
        assert "duplicate_count must be >= 1" in str(e.value)
    # (with ignore_counts the column is not looked at)
    with HipOverlap(tiny_options(False, counts=False)) as h:
        assert h.deduplicate(s)[2] == _dedup.model(s, tiny_options(False, counts=False))[2]


def test_null_set_is_einval():
    with HipOverlap(tiny_options(False)) as h:
        unique = C.c_uint64()
        for fn in (h._lib.cmpr_deduplicate, h._lib.cmpr_deduplicate_device):
            assert fn(h._ctx, None, 0, None, None, C.byref(unique), None) == CMPR_EINVAL
            assert h._lib.cmpr_last_error(h._ctx).decode() == "set view is NULL"


def test_resident_sets_are_not_disturbed():
    """between two overlap_matrix() calls: a third set with the resident Zobrist keys, and one too long for them"""
    a, b = synth.make_set(3000, 1, pool_size=500), synth.make_set(3000, 2, pool_size=500)
    opt = Options(differences=1, n_v_genes=synth.N_V, n_j_genes=synth.N_J, device=0)
    short = synth.tiny_set(4000, 8, letters=2, max_len=6)
    long = synth.tiny_set(4000, 9, letters=2, min_len=30, max_len=40)
    assert long.longest > max(a.longest, b.longest) + 3
    with HipOverlap(opt) as h:
        h.set_reference(b, a.longest)
        h.set_queries(a)
        before, stats = h.overlap_matrix(), h.stats()
        assert before.sum() > 0
        for third in (short, long):
            got, want = h.deduplicate(third), _dedup.model(third, opt)
            assert got[2] == want[2] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            assert h.count_duplicates(third) == want[2]
        assert np.array_equal(h.overlap_matrix(), before)
        after = h.stats()
        assert (after.queries, after.variants, after.matches) == (stats.queries, stats.variants, stats.matches)
        assert h.shape == before.shape


def test_two_calls_give_identical_arrays():
    s, opt = big_set(False), tiny_options(False)
    with HipOverlap(opt) as h:
        one, two = h.deduplicate(s), h.deduplicate(s)
    with HipOverlap(opt) as h:
        three = h.deduplicate(s)
    for other in (two, three):
        assert np.array_equal(one[0], other[0]) and np.array_equal(one[1], other[1]) and one[2] == other[2]
