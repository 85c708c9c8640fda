"""The generator of the all-against-all sweep (tests/_pairs_fuzz.py), proven on the CPU for the committed slice of
tests/test_pairs_fuzz_gpu.py -- SLICE_SEEDS x SLICE_CASES cases --: determinism, the size caps, and the coverage
conditions under which the slice is not vacuous.  The shares below are conditions on the generator, met by the brute
force alone; nothing here calls the library under test."""

import functools
import time

import _edit_forms
import _pairs_fuzz as pf

MIN_PER_COMBO = 8
MIN_SEEN = 2


@functools.lru_cache(maxsize=None)
def slice_cases():
    """[(case, tags, features, seconds of its yardstick)] of the whole slice, computed once"""
    out = []
    for seed in pf.SLICE_SEEDS:
        for index in range(pf.SLICE_CASES):
            c = pf.case(seed, index)
            t0 = time.perf_counter()
            want = pf.expect(c)
            seconds = time.perf_counter() - t0
            out.append((c, frozenset(pf.classify(c, want)), frozenset(pf.features(c)), seconds))
    return out


def seen(name, where=None, live_only=True):
    """the cases of the slice (of one metric, of one alphabet) that carry a tag or a feature"""
    return [c for c, tags, feats, _ in slice_cases()
            if (name in tags or name in feats) and not (live_only and "vacuous" in tags) and (where is None or where(c))]


def test_a_case_is_deterministic_and_self_contained():
    in_order = [pf.fingerprint(c) for c, _, _, _ in slice_cases()]
    seed = pf.SLICE_SEEDS[0]
    for index in (pf.SLICE_CASES - 1, 40, 13, 0):                      # alone, in another order, after the others
        assert pf.fingerprint(pf.case(seed, index)) == in_order[index]
        assert pf.fingerprint(pf.case(seed, index)) == in_order[index]
    assert len(set(in_order)) == len(in_order)
    assert pf.fingerprint(pf.case(pf.SLICE_SEEDS[1], 7)) == in_order[pf.SLICE_CASES + 7]


def test_every_case_respects_the_caps():
    for c, _, _, _ in slice_cases():
        assert pf.cost(c) <= pf.CAPS[c.metric], pf.describe(c)
        assert c.set1.n <= pf.MAX_N and c.set2.n <= pf.MAX_N, pf.describe(c)
        longest = max(c.set1.longest, c.set2.longest)
        assert longest <= (65535 if c.metric == "hamming" else 256), pf.describe(c)


def test_every_case_is_a_valid_call():
    """what the calls refuse is not drawn: MH / Jaccard above d = 0 or with existence, existence with clusters, a V
    table with ignore_genes, nucleotides under TCRdist, other_repertoire with two sets"""
    for c, _, _, _ in slice_cases():
        zero = c.differences == 0 or (c.metric == "tcrdist" and c.cutoff == 0)
        assert c.score in pf.SCORES or (zero and not c.existence), pf.describe(c)
        assert not (c.existence and c.kind in ("cluster", "cluster_table")), pf.describe(c)
        assert not (c.other_repertoire and not c.one_set), pf.describe(c)
        if c.metric == "tcrdist":
            assert not c.nucleotides and not (c.V is not None and c.ignore_genes) and 0 <= c.cutoff <= 65535
            assert c.V is None or c.V.shape == (c.n_v, c.n_v)
        for s, n_rep in ((c.set1, c.n_rep1), (c.set2, c.n_rep2)):
            assert s.n_repertoires == n_rep and (s.count >= 1).all()
            assert (s.repertoire < n_rep).all() and (s.v_gene < c.n_v).all() and (s.j_gene < c.n_j).all()
            assert (s.residues < (4 if c.nucleotides else 20)).all()


def test_the_slice_is_not_vacuous(capsys):
    cases = slice_cases()
    vacuous = [c for c, tags, _, _ in cases if "vacuous" in tags]
    lines = ["%d cases, %d vacuous" % (len(cases), len(vacuous)),
             "%-24s %5s %8s %12s" % ("combination", "cases", "vacuous", "cross-length")]
    for metric, kind in pf.COMBOS:
        mine = [(c, tags) for c, tags, _, _ in cases if (c.metric, c.kind) == (metric, kind)]
        empty = sum(1 for _, tags in mine if "vacuous" in tags)
        live = [tags for _, tags in mine if "vacuous" not in tags]
        cross = sum(1 for tags in live if "cross-length" in tags)
        lines.append("%-24s %5d %8d %12d" % (metric + " " + kind, len(mine), empty, cross))
        assert len(mine) >= MIN_PER_COMBO, (metric, kind)
        assert 4 * empty <= len(mine), (metric, kind, empty, len(mine))
    assert 10 * len(vacuous) <= len(cases)
    for metric in ("edit", "tcrdist"):
        live = [tags for c, tags, _, _ in cases if c.metric == metric and "vacuous" not in tags]
        cross = sum(1 for tags in live if "cross-length" in tags)
        lines.append("%s: %d of %d live cases have a cross-length edge" % (metric, cross, len(live)))
        assert 2 * cross >= len(live), metric
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_every_form_and_every_tag_is_seen(capsys):
    lines, missing = [], []

    def need(name, where=None, live_only=True, label=""):
        n = len(seen(name, where, live_only))
        lines.append("%-34s %3d" % ((label + " " + name).strip(), n))
        if n < MIN_SEEN:
            missing.append((label, name, n))

    for metric, nucleotides in (("edit", False), ("edit", True), ("tcrdist", False)):
        for form in _edit_forms.ALL_FORMS[nucleotides]:
            need("form %d" % form, lambda c: (c.metric, c.nucleotides) == (metric, nucleotides),
                 label="%s %s" % (metric, "nt" if nucleotides else "aa"))
    for side in ("hamming register", "hamming generic"):
        need(side)
    for tag in pf.TAGS:
        need(tag, live_only=tag not in ("empty set 1", "empty set 2"))
    for feature in (["score " + s for s in pf.SCORES + ("mh", "jaccard")]
                    + ["existence", "ignore_counts", "V table", "gap penalty 0", "cutoff 0", "differences 0",
                       "differences >= longest", "other_repertoire", "floor 0", "floor 1", "floor 2", "cap None", "cap 0",
                       "cap 1", "cap 3", "entry host", "entry device", "capacity exact", "capacity short",
                       "capacity generous"] + ["tunable " + t for t in pf.TUNABLE_NAMES]):
        need(feature, live_only=False)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not missing, missing


def test_matrix_of_under_every_score_against_plain_integers():
    """_edit.matrix_of -- MH and Jaccard included: the product and the min sums -- against a loop over the pairs in
    Python integers modulo 2^64, on a case whose counts lie near 2^63"""
    c = next(c for c, tags, _, _ in slice_cases() if c.big_counts and "vacuous" not in tags and not c.one_set
             and c.n_rep1 > 1 and c.n_rep2 > 1)
    rows, hits, _ = pf.pair_list(c)
    q = pf._edit.queries_of(rows).tolist()
    score = {"product": lambda f, g: f * g, "mh": lambda f, g: f * g, "min": min, "jaccard": min, "max": max,
             "mean": lambda f, g: f + g}
    for name, fn in score.items():
        for ignore_counts in (False, True):
            cells = {}
            for i, j in zip(q, hits.tolist()):
                key = (int(c.set1.repertoire[i]), int(c.set2.repertoire[j]))
                v = 1 if ignore_counts else fn(int(c.set1.count[i]), int(c.set2.count[j]))
                cells[key] = (cells.get(key, 0) + v) % 2 ** 64
            opt = pf.Options(score=name, ignore_counts=ignore_counts)
            got = pf._edit.matrix_of(c.set1, c.set2, rows, hits, opt)
            assert got.shape == (c.n_rep1, c.n_rep2)
            assert {k: int(got[k]) for k in zip(*got.nonzero())} == {k: v for k, v in cells.items() if v}, name


def test_the_yardstick_time_of_every_item_is_printed(capsys):
    """no time is asserted: the figures go to profiles/r27/pairs_fuzz.txt"""
    cases = slice_cases()
    lines = ["yardstick seconds per item of tests/test_pairs_fuzz_gpu.py (seed, first case: seconds, slowest case)"]
    for k in range(0, len(cases), pf.CHUNK):
        chunk = cases[k:k + pf.CHUNK]
        slow = max(chunk, key=lambda x: x[3])
        lines.append("%10d %3d: %6.2f  (case %d: %.2f)" % (chunk[0][0].seed, chunk[0][0].index, sum(x[3] for x in chunk),
                                                          slow[0].index, slow[3]))
    lines.append("all: %.2f" % sum(x[3] for x in cases))
    with capsys.disabled():
        print("\n" + "\n".join(lines))
