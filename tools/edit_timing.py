#!/usr/bin/env python3
"""usage (GPU box): timeout 1100 python3 tools/edit_timing.py [--against OTHER/libcompairr_hip.so]
                                             [--n 1000000] [--out build/edit_timing]

What cmpr_edit_neighbors_device costs, written to <out>/edit.txt (the committed copy: profiles/rNN/edit.txt).  The one
condition is that of (a); the rest is a report, and nothing is re-routed on its strength.

  shapes  --n synth.make_set CDR3aa sequences against as many of another seed at d = 1, 2, 3, V/J matched and with
          ignore_genes, and --nt-n nucleotide sequences with ignore_genes at d = 2, the sets already in HBM:
          cmpr_edit_neighbors_device count-only and with the exact capacity (hits and distances), host clock around the
          synchronous calls, --reps calls each after one count-only call that also warms up; the parts as the library
          clocks them (tunables edit_{group,compare,order,copy}_us); the edges, their distances, the longest row, and
          the pairs compared (the sum over the jobs of queries x references of every partner group);
  (a) bench.py's default `value` (query sequences/s) with this tree's library ("branch") and with --against LIB
      ("parent", the parent commit's build), alternately, --rounds runs each: all values, the medians, the parent's
      own max - min, and whether the branch's median falls below the parent's median by more than that (exit status
      2 when it does: no hot-path file changed, so that would be a finding);
  (b) at d = 3, the compare part of the count-only call beside that of cmpr_hamming_neighbors_device's count-only call
      on the same sets in the same process: time per pair compared of either, and their ratio -- the cost of an
      edit comparison in units of a Hamming comparison;
  (c) d = 1 on the --n set against itself: the edit call (count, then fill) beside cmpr_set_reference_device +
      cmpr_set_queries_device + cmpr_neighbors_distance_device on a context with indels, the hashed route to the
      same edges; whether the two CSRs are equal.

Every step that uses the GPU is a child process under its own time limit; a step that fails ends the run."""

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

PARTS = ("group", "compare", "order", "copy")


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else (xs[len(xs) // 2 - 1] + xs[len(xs) // 2]) / 2


def spread(xs):
    return "%s  median %.2f  min %.2f  max %.2f" % (" ".join("%.2f" % x for x in xs), median(xs), min(xs), max(xs))


def pairs_of(s1, s2, ignore_genes, d):
    """pairs compared at distance d (lengths no more than d apart, one V and J) and at d = 0 (one length: what
    cmpr_hamming_* compares), from the group sizes"""
    def table(s):
        genes = np.zeros(s.n, dtype=np.int64) if ignore_genes else s.v_gene.astype(np.int64) * 4096 + s.j_gene
        keys, counts = np.unique(genes * 1024 + s.lengths.astype(np.int64), return_counts=True)   # (lengths <= 256)
        t = {}
        for k, c in zip(keys.tolist(), counts.tolist()):
            t.setdefault(k // 1024, {})[k % 1024] = c
        return t
    t1, t2 = table(s1), table(s2)
    within = same = 0
    for g, lens1 in t1.items():
        lens2 = t2.get(g, {})
        for L1, c1 in lens1.items():
            same += c1 * lens2.get(L1, 0)
            within += c1 * sum(c2 for L2, c2 in lens2.items() if abs(L1 - L2) <= d)
    return within, same


def timed(h, call, reps):
    ms, parts = [], {p: [] for p in PARTS}
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
        for p in PARTS:
            parts[p].append(h.get_tunable("edit_%s_us" % p) / 1e3)
    return ms, parts


def sets_of(n, nucleotides, same):
    from compairr_amd import synth
    a = synth.make_set(n, 1, prefix="A", pool_size=n // 4, nucleotides=nucleotides)
    return a, (a if same else synth.make_set(n, 2, prefix="B", pool_size=n // 4, nucleotides=nucleotides))


def measure(n, d, ignore_genes, nucleotides, reps, with_hamming):
    """(child) one JSON line: the device call on one pair of sets; with_hamming: cmpr_hamming_neighbors_device's
    count-only call beside it"""
    import torch
    from compairr_amd import HipOverlap, Options, synth
    a, b = sets_of(n, nucleotides, False)
    within, same = pairs_of(a, b, ignore_genes, d)
    out = {"n": n, "d": d, "g": ignore_genes, "nt": nucleotides, "pairs": within, "pairs_one_length": same}
    opt = Options(n_v_genes=synth.N_V, n_j_genes=synth.N_J, ignore_genes=ignore_genes, nucleotides=nucleotides, device=0)
    with HipOverlap(opt) as h:
        v1, keep1 = HipOverlap.device_view(a)
        v2, keep2 = HipOverlap.device_view(b)
        d_rows = torch.zeros(a.n + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        edges = h.edit_neighbors_device(v1, v2, d, 0, d_rows.data_ptr())
        ms, parts = timed(h, lambda: h.edit_neighbors_device(v1, v2, d, 0, d_rows.data_ptr()), reps)
        out.update(edges=edges, count_only_ms=ms, count_only_compare_ms=parts["compare"], count_only_group_ms=parts["group"])
        d_hits = torch.zeros(max(edges, 1), dtype=torch.int32, device="cuda")
        d_dist = torch.zeros(max(edges, 1), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        ms, parts = timed(h, lambda: h.edit_neighbors_device(v1, v2, d, edges, d_rows.data_ptr(), d_hits.data_ptr(),
                                                              d_dist.data_ptr()), reps)
        hist = torch.bincount(d_dist[:edges].to(torch.int64), minlength=d + 1).cpu().tolist() if edges else []
        out.update(neighbors_ms=ms, histogram=hist, longest_row=int(torch.diff(d_rows).max().item()),
                   **{"neighbors_%s_ms" % p: v for p, v in parts.items()})
        if with_hamming:
            h_edges = h.hamming_neighbors_device(v1, v2, d, 0, d_rows.data_ptr())
            ham = []
            for _ in range(reps):
                h.hamming_neighbors_device(v1, v2, d, 0, d_rows.data_ptr())
                ham.append(h.get_tunable("hamming_compare_us") / 1e3)
            out.update(hamming_edges=h_edges, hamming_compare_ms=ham)
    print(json.dumps(out))


def measure_hashed(n, reps):
    """(child) one JSON line: the edit call beside the hashed path with indels on one set against itself at d = 1"""
    import torch
    from compairr_amd import HipOverlap, Options, synth
    a, _ = sets_of(n, False, True)
    out = {"n": n}
    opt = Options(differences=1, indels=True, n_v_genes=synth.N_V, n_j_genes=synth.N_J, device=0)
    d_rows = torch.zeros(a.n + 1, dtype=torch.int64, device="cuda")
    hashed, edit = [], []
    for k in range(reps + 1):                      # (the first round is the warm-up one)
        with HipOverlap(opt) as h:
            v, keep = HipOverlap.device_view(a)
            t0 = time.perf_counter()
            h.set_reference_device(v, a.longest)
            h.set_queries_device(v)
            edges = h.neighbors_distance_device(0, d_rows.data_ptr(), 0, 0)
            d_hits = torch.zeros(max(edges, 1), dtype=torch.int32, device="cuda")
            d_dist = torch.zeros(max(edges, 1), dtype=torch.uint8, device="cuda")
            h.neighbors_distance_device(edges, d_rows.data_ptr(), d_hits.data_ptr(), d_dist.data_ptr())
            torch.cuda.synchronize()
            hashed.append((time.perf_counter() - t0) * 1e3)
            want_rows = d_rows.clone()
            t0 = time.perf_counter()
            e2 = h.edit_neighbors_device(v, v, 1, 0, d_rows.data_ptr())
            d_hits2 = torch.zeros(max(e2, 1), dtype=torch.int32, device="cuda")
            d_dist2 = torch.zeros(max(e2, 1), dtype=torch.int16, device="cuda")
            h.edit_neighbors_device(v, v, 1, e2, d_rows.data_ptr(), d_hits2.data_ptr(), d_dist2.data_ptr())
            torch.cuda.synchronize()
            edit.append((time.perf_counter() - t0) * 1e3)
            out.update(edges=edges, edit_edges=e2, shortest=int(a.lengths.min()),
                       equal=bool(e2 == edges and torch.equal(want_rows, d_rows) and torch.equal(d_hits, d_hits2)
                                  and torch.equal(d_dist.to(torch.int16), d_dist2)))
    out.update(hashed_ms=hashed[1:], edit_ms=edit[1:])
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nt-n", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3, help="(a): bench.py runs of each library")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "edit_timing"))
    ap.add_argument("--against", metavar="LIB", help="the parent commit's library")
    ap.add_argument("--child", choices=("measure", "hashed"))
    ap.add_argument("--d", type=int, default=3)
    ap.add_argument("--g", type=int, default=0)
    ap.add_argument("--nt", type=int, default=0)
    ap.add_argument("--hamming", type=int, default=0)
    args = ap.parse_args()
    if args.child == "measure":
        return measure(args.n, args.d, bool(args.g), bool(args.nt), args.reps, bool(args.hamming))
    if args.child == "hashed":
        return measure_hashed(args.n, args.reps)

    os.makedirs(args.out, exist_ok=True)
    lines = ["cmpr_edit_*: the existing workload beside the parent commit, and the new calls (tools/edit_timing.py)"]
    status = 0

    def flush():
        with open(os.path.join(args.out, "edit.txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")

    def failed(what, p):
        lines.append("%s failed with %d: %s" % (what, p.returncode, p.stderr.decode(errors="replace")[-500:]))
        flush()
        print(lines[-1], flush=True)
        return p.returncode or 1

    branch_env = {k: v for k, v in os.environ.items() if k != "COMPAIRR_HIP_LIB"}

    def child(limit, *extra):
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--reps",
                            str(args.reps)] + [str(x) for x in extra], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=branch_env)
        return p, (json.loads(p.stdout.decode().strip().splitlines()[-1]) if p.returncode == 0 else None)

    # (a) bench.py, parent and branch in turn
    if args.against:
        sides = [("parent", dict(os.environ, COMPAIRR_HIP_LIB=os.path.abspath(args.against))), ("branch", branch_env)]
        values = {"parent": [], "branch": []}
        for rnd in range(args.rounds):
            for side, env in sides:
                p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                                    "--steps", str(args.steps), "--warmup", str(args.warmup)],
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=ROOT)
                if p.returncode != 0:
                    return failed("bench.py (%s, round %d)" % (side, rnd), p)
                values[side].append(float(json.loads(p.stdout.decode().strip().splitlines()[-1])["value"]))
                print("%s round %d: %.4g" % (side, rnd, values[side][-1]), flush=True)
        pa, br = values["parent"], values["branch"]
        slower = median(br) < median(pa) - (max(pa) - min(pa))
        lines.append("(a) bench.py --gpus 1 --steps %d --warmup %d, `value` in query sequences/s, %d runs each in turn"
                     % (args.steps, args.warmup, args.rounds))
        lines.append("    parent: %s  median %.4g  min %.4g  max %.4g" % (" ".join("%.4g" % x for x in pa), median(pa), min(pa), max(pa)))
        lines.append("    branch: %s  median %.4g  min %.4g  max %.4g" % (" ".join("%.4g" % x for x in br), median(br), min(br), max(br)))
        lines.append("    branch median / parent median = %.4f; parent median - branch median = %.4g, parent max - min = %.4g: %s"
                     % (median(br) / median(pa), median(pa) - median(br), max(pa) - min(pa),
                        "SLOWER by more than the parent's own spread" if slower else "within the condition"))
        if slower:
            status = 2
    else:
        lines.append("(a) not measured: no --against library")
    flush()

    # the shapes; (b) beside the d = 3 ones
    cases = [(args.n, d, g, 0) for d in (1, 2, 3) for g in (0, 1)] + [(args.nt_n, 2, 1, 1)]
    for n, d, g, nt in cases:
        p, r = child(900, "--child", "measure", "--n", n, "--d", d, "--g", g, "--nt", nt, "--hamming", int(d == 3))
        if r is None:
            return failed("timing child (n = %d, d = %d, g = %d, nt = %d)" % (n, d, g, nt), p)
        first = len(lines)
        lines.append("%d x %d %s, d = %d%s: %d pairs compared, %d edges, longest row %d, distances %s"
                     % (n, n, "nucleotide sequences" if nt else "CDR3aa", d, ", ignore_genes" if g else "", r["pairs"],
                        r["edges"], r["longest_row"], r["histogram"]))
        lines.append("    cmpr_edit_neighbors_device, sets in HBM, count-only, host ms per call (%d calls after a warm-up): %s"
                     % (len(r["count_only_ms"]), spread(r["count_only_ms"])))
        lines.append("      group    %s" % spread(r["count_only_group_ms"]))
        lines.append("      compare  %s" % spread(r["count_only_compare_ms"]))
        one_pass = median(r["count_only_compare_ms"]) / 1e3
        lines.append("      compare kernel, one pass: %.3g pairs/s" % (r["pairs"] / one_pass))
        lines.append("    cmpr_edit_neighbors_device, exact capacity, hits and distances: %s" % spread(r["neighbors_ms"]))
        for part in PARTS[:3]:
            lines.append("      %-8s %s" % (part, spread(r["neighbors_%s_ms" % part])))
        if "hamming_compare_ms" in r:
            ham = median(r["hamming_compare_ms"]) / 1e3
            per_edit, per_ham = one_pass / max(1, r["pairs"]), ham / max(1, r["pairs_one_length"])
            lines.append("(b) cmpr_hamming_neighbors_device count-only on the same sets, d = %d: %d pairs of one length compared, "
                         "%d edges, compare %s" % (d, r["pairs_one_length"], r["hamming_edges"], spread(r["hamming_compare_ms"])))
            lines.append("    per pair compared: edit %.3g s, Hamming %.3g s: an edit comparison costs %.1f Hamming comparisons"
                         % (per_edit, per_ham, per_edit / per_ham))
        flush()
        print("\n".join(lines[first:]), flush=True)

    # (c) the hashed route with indels at d = 1
    p, r = child(500, "--child", "hashed", "--n", args.n)
    if r is None:
        return failed("hashed child", p)
    first = len(lines)
    lines.append("(c) %d CDR3aa against themselves, d = 1 with indels: %d edges (hashed), %d (edit); shortest sequence %d; "
                 "the two CSRs equal: %s" % (r["n"], r["edges"], r["edit_edges"], r["shortest"], r["equal"]))
    lines.append("    cmpr_set_reference_device + cmpr_set_queries_device + cmpr_neighbors_distance_device (count, then fill), ms: %s"
                 % spread(r["hashed_ms"]))
    lines.append("    cmpr_edit_neighbors_device (count, then fill), ms: %s" % spread(r["edit_ms"]))
    flush()
    print("\n".join(lines[first:]), flush=True)
    return status


if __name__ == "__main__":
    sys.exit(main())
