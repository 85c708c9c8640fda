"""What the LDS budget decides, pinned case by case: kernel variant, waves per workgroup, slice size and count,
pair rows of d = 2 and their buffers, record tiles, and the code and text of every refusal.

Only the longest sequence and the option set matter to the budget, so the sets are a few hundred sequences.  The
lengths are taken from the formulas (tests/test_lds_map_cpu.py) so that each decision is seen on both sides:
  * variant 2 shrinking its slice next to a longer Zobrist table (amino acids: beyond 39 residues; seen with a
    filter of 7.25 bytes per entry, just over two full slices of these sets: two slices of 20 KiB, or four smaller)
  * variant 2 / variant 1 giving way to variant 0 (amino acids: beyond 282 residues; nucleotides, d = 1: beyond 572)
  * pair rows of d = 2: up to 96 nucleotides (beyond, single rows: the residues no longer pack; the budget's own
    exit there is out of reach below 444 nucleotides)
  * make_plan halving the waves of a workgroup (512 tile references per chunk; 16 waves asked for)
  * both CMPR_EUNSUPPORTED texts of make_plan
  * record tiles with thousands of V and J genes, with and without -i
The expectations are in tests/golden/lds_decisions.json, recorded by tests/golden/make_lds_decisions.py from the
library of the commit named in that file -- never from the library under test.  Where a case launches, its matrix
is held against the oracle's as well.
"""

import dataclasses
import functools
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(HERE, "golden", "lds_decisions.json")
ASKED = ("variant", "waves_per_block", "slice_bytes", "slices", "d2_pairs", "d2_buffers", "record_tiles")

# name -> (nucleotides, d, -i, longest sequence, V genes, J genes, tunables)
CASES = {
    "aa_d1": (False, 1, False, 24, 60, 13, {}),
    "aa_d1_39": (False, 1, False, 39, 60, 13, {"row_filter_x16": 116}),
    "aa_d1_40": (False, 1, False, 40, 60, 13, {"row_filter_x16": 116}),
    "aa_d1_100": (False, 1, False, 100, 60, 13, {"row_filter_x16": 116}),
    "aa_d1i_100": (False, 1, True, 100, 60, 13, {}),
    "aa_d1_282": (False, 1, False, 282, 60, 13, {}),
    "aa_d1_283": (False, 1, False, 283, 60, 13, {}),
    "aa_d1_280_tiles512": (False, 1, False, 280, 60, 13, {"chunk_tiles": 512}),
    "aa_d1_1000": (False, 1, False, 1000, 60, 13, {}),
    "aa_d2": (False, 2, False, 24, 60, 13, {}),
    "aa_d2_39": (False, 2, False, 39, 60, 13, {"row_filter_x16": 116}),
    "aa_d2_40": (False, 2, False, 40, 60, 13, {"row_filter_x16": 116}),
    "aa_d2_100": (False, 2, False, 100, 60, 13, {}),
    "nt_d1": (True, 1, False, 72, 60, 13, {}),
    "nt_d1_572": (True, 1, False, 572, 60, 13, {}),
    "nt_d1_573": (True, 1, False, 573, 60, 13, {}),
    "nt_d1_500_waves16": (True, 1, False, 500, 60, 13, {"waves_per_block": 16}),
    "nt_d1_572_waves16_tiles512": (True, 1, False, 572, 60, 13, {"waves_per_block": 16, "chunk_tiles": 512}),
    "nt_d1_500_tiles512": (True, 1, False, 500, 60, 13, {"chunk_tiles": 512}),
    "nt_d2_96": (True, 2, False, 96, 60, 13, {}),
    "nt_d2_97": (True, 2, False, 97, 60, 13, {}),
    "nt_d2_96_two_buffers": (True, 2, False, 96, 60, 13, {"d2_buffers": 2}),
    "nt_d2_96_tiles512": (True, 2, False, 96, 60, 13, {"chunk_tiles": 512, "row_filter_x16": 128}),
    "aa_d1_genes5000": (False, 1, False, 24, 3000, 2000, {}),
    "aa_d1i_genes5000": (False, 1, True, 24, 3000, 2000, {}),
    "aa_d1_genes9000": (False, 1, False, 24, 6000, 3000, {}),
    "aa_d1i_genes9000": (False, 1, True, 24, 6000, 3000, {}),
    "aa_d1_genes5000_no_record_tiles": (False, 1, False, 24, 3000, 2000, {"record_tiles": 0}),
}


def make_set(seed, shared, nucleotides, longest, n_v, n_j, n=340, n_rep=4):
    """n sequences of ordinary length, the first two of `longest` residues; a third of them taken from `shared`
    (residues, length, V, J per row), half of those with one residue replaced"""
    from compairr_amd.sets import AA, NT, RepertoireSet
    rng = np.random.default_rng([seed, 0x1D5])
    A, lo, hi = (4, 24, 72) if nucleotides else (20, 8, 24)
    sres, slen, sv, sj = shared
    lens = rng.integers(lo, min(hi, longest) + 1, size=n)
    pad = rng.integers(0, A, size=(n, longest), dtype=np.uint8)
    v = rng.integers(0, n_v, size=n, dtype=np.uint32)
    j = rng.integers(0, n_j, size=n, dtype=np.uint32)
    take = np.flatnonzero(rng.random(n) < 0.33)
    take = np.union1d(take, [0, 1])
    pick = take % len(slen)                       # (rows 0 and 1 of `shared` are the long ones)
    pad[take], lens[take], v[take], j[take] = sres[pick], slen[pick], sv[pick], sj[pick]
    mut = take[rng.random(len(take)) < 0.5]
    pos = rng.integers(0, 1 << 30, size=len(mut)) % lens[mut]
    pad[mut, pos] = (pad[mut, pos] + rng.integers(1, A, size=len(mut)).astype(np.uint8)) % A
    residues = pad[np.arange(longest)[None, :] < lens[:, None]]
    offsets = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=offsets[1:])
    rep = np.arange(n, dtype=np.uint32) % n_rep   # (numbered by first appearance)
    return RepertoireSet(residues, offsets, v, j, rep, rng.integers(1, 10, size=n, dtype=np.uint64),
                         ["R%d" % (k + 1) for k in range(n_rep)], ["V%d" % k for k in range(n_v)],
                         ["J%d" % k for k in range(n_j)], NT if nucleotides else AA)


@functools.lru_cache(maxsize=None)
def sets_of(name):
    nucleotides, _, _, longest, n_v, n_j, _ = CASES[name]
    rng = np.random.default_rng([len(name), longest, 0x5A])
    A, lo, hi = (4, 24, 72) if nucleotides else (20, 8, 24)
    m = 100
    slen = rng.integers(lo, min(hi, longest) + 1, size=m)
    slen[:2] = longest
    shared = (rng.integers(0, A, size=(m, longest), dtype=np.uint8), slen,
              rng.integers(0, n_v, size=m, dtype=np.uint32), rng.integers(0, n_j, size=m, dtype=np.uint32))
    return (make_set(1, shared, nucleotides, longest, n_v, n_j), make_set(2, shared, nucleotides, longest, n_v, n_j))


def options_of(name):
    from compairr_amd import Options
    nucleotides, d, indels, _, n_v, n_j, _ = CASES[name]
    return Options(differences=d, indels=indels, nucleotides=nucleotides, n_v_genes=n_v, n_j_genes=n_j, device=0)


def observe(name):
    """({"calls": [[call, code, text], ...], "tunables": {...}}, the matrix or None) of the loaded library"""
    import ctypes as C
    from compairr_amd import HipOverlap
    from compairr_amd import hip as hipmod
    a, b = sets_of(name)
    h = HipOverlap(options_of(name))
    lib, ctx = h._lib, h._ctx
    for k, v in CASES[name][6].items():
        h.set_tunable(k, v)
    va, vb = hipmod._view(a), hipmod._view(b)
    cells = np.zeros((a.n_repertoires, b.n_repertoires), dtype=np.uint64)
    calls, matrix = [], None
    for call, run in (("cmpr_set_reference", lambda: lib.cmpr_set_reference(ctx, C.byref(vb), a.longest)),
                      ("cmpr_set_queries", lambda: lib.cmpr_set_queries(ctx, C.byref(va))),
                      ("cmpr_overlap_matrix", lambda: lib.cmpr_overlap_matrix(ctx, cells.ctypes.data))):
        rc = run()
        calls.append([call, rc, lib.cmpr_last_error(ctx).decode() if rc else ""])
        if rc:
            break
    else:
        matrix = cells
    tunables = {k: h.get_tunable(k) for k in ASKED}
    h.close()
    return {"calls": calls, "tunables": tunables}, matrix


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as fh:
        return json.load(fh)


def test_cases_are_the_recorded_ones(recorded):
    assert recorded["library_commit"]
    assert recorded["cases"] == {name: [int(x) if not isinstance(x, dict) else x for x in CASES[name]] for name in CASES}
    assert sorted(recorded["observed"]) == sorted(CASES)


def test_every_decision_is_taken_on_both_sides(recorded):
    """(of the recorded library: the cases were chosen from the formulas, this is the proof that they land)"""
    seen = recorded["observed"]
    t = lambda name, key: seen[name]["tunables"][key]
    for d in ("d1", "d2"):      # (a filter of just over two full slices: four smaller ones once the slice shrinks)
        assert t("aa_%s_39" % d, "slice_bytes") == 640 * 32 > t("aa_%s_40" % d, "slice_bytes") > 0
        assert t("aa_%s_39" % d, "slices") < t("aa_%s_40" % d, "slices")
    assert (t("aa_d1_282", "variant"), t("aa_d1_283", "variant")) == (2, 0)
    assert (t("nt_d1_572", "variant"), t("nt_d1_573", "variant")) == (1, 0)
    assert (t("nt_d2_96", "d2_pairs"), t("nt_d2_97", "d2_pairs")) == (1, 0)
    assert (t("nt_d2_96", "d2_buffers"), t("nt_d2_96_two_buffers", "d2_buffers")) == (1, 2)
    assert t("nt_d1_572_waves16_tiles512", "waves_per_block") == 8 and t("nt_d1_500_waves16", "waves_per_block") == 16
    assert t("aa_d1_280_tiles512", "waves_per_block") == 8 and t("aa_d1_282", "waves_per_block") == 16
    texts = {c[2] for name in seen for c in seen[name]["calls"] if c[1]}
    assert any("pair-row kernel of d = 2 does not fit" in x for x in texts)
    assert any("Zobrist table does not fit" in x for x in texts)
    assert t("aa_d1_genes5000", "record_tiles") != 0 and t("aa_d1i_genes5000", "record_tiles") != 0
    assert t("aa_d1_genes5000_no_record_tiles", "record_tiles") == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_decisions_as_recorded_and_matrix_as_the_oracle(recorded, name):
    import _oracle
    got, matrix = observe(name)
    print(name, json.dumps(got))
    assert got == recorded["observed"][name]
    if matrix is not None:
        a, b = sets_of(name)
        opt = options_of(name)
        want, _ = _oracle.overlap(a, b, opt, threads=2)
        assert matrix.sum() > 0
        assert np.array_equal(matrix, _oracle.integer_cells(want, opt))


def test_lds_limit_of_a_kernel_never_drops():
    """One context, variant 1 (its LDS holds the matrix cells): 1600 cells, then one cell, then the 1600 again --
    the limit raised for the first launch must still stand for the third (raise_lds_limit keeps, per kernel, the
    largest value set and never sets a smaller one)."""
    import _oracle
    from compairr_amd import HipOverlap, Options, synth
    opt = Options(differences=1, nucleotides=True, n_v_genes=synth.N_V, n_j_genes=synth.N_J, device=0)
    ref = synth.make_set(2000, 2, nucleotides=True, n_repertoires=1, pool_size=1500)
    wide = synth.make_set(3200, 1, nucleotides=True, n_repertoires=1, pool_size=1500)
    wide = dataclasses.replace(wide, repertoire=np.arange(wide.n, dtype=np.uint32) % 1600,
                               repertoire_ids=["W%d" % k for k in range(1600)])
    one = synth.make_set(2000, 3, nucleotides=True, n_repertoires=1, pool_size=1500)
    assert (wide.n_repertoires * ref.n_repertoires, one.n_repertoires * ref.n_repertoires) == (1600, 1)
    want = {id(s): _oracle.integer_cells(_oracle.overlap(s, ref, opt, threads=2)[0], opt) for s in (wide, one)}
    with HipOverlap(opt) as h:
        h.set_tunable("waves_per_block", 16)        # (sixteen wave queues: every launch asks for more than 48 KiB)
        h.set_reference(ref, max(wide.longest, one.longest))
        for s in (wide, one, wide):
            h.set_queries(s)
            assert h.get_tunable("variant") == 1
            got = h.overlap_matrix()
            assert got.sum() > 0 and np.array_equal(got, want[id(s)])
