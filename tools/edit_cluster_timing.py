#!/usr/bin/env python3
"""usage (GPU box): timeout 1100 python3 tools/edit_cluster_timing.py [--against OTHER/libcompairr_hip.so]
                                                [--n 1000000] [--parts abc] [--out build/edit_cluster_timing]

What cmpr_edit_cluster_table_device costs, written to <out>/edit_cluster.txt (the committed copy:
profiles/r23/edit_cluster.txt).  The one condition is that of (a); the rest is a report.

  (a) bench.py's default `value` (query sequences/s) with this tree's library ("branch") and with --against LIB
      ("parent", the parent commit's build), alternately, --rounds runs each: all values, the medians, the parent's
      own max - min, and whether the branch's median falls below the parent's median by more than that (exit status
      2 when it does: nothing on the hashed path changed, so that would be a finding);
  (b) --n synth.make_set CDR3aa sequences, the set already in HBM, at d = 1, 2, 3 V/J matched and d = 1 with
      ignore_genes:
        * cmpr_edit_cluster_table_device, host clock around the synchronous call, --reps calls after a warm-up one
          (--g-reps with ignore_genes), and its parts as the library clocks them (edit_group_us: grouping and jobs;
          edit_compare_us: link kernel, flatten, sizes; cluster_table_us: the table);
        * the route to the same table without it: cmpr_edit_neighbors_device of the set against itself (count, then
          fill, no distances), the edges to the host, a numpy union-find (min-label propagation with pointer jumping,
          as tools/cluster_timing.py), np.lexsort for the cluster order and the members -- clocked in its parts; the
          two tables must be equal (exit status 3 when they are not);
        * the link kernel against the count-only walk: edit_compare_us of the new call beside that of the count-only
          cmpr_edit_neighbors_device call, which walks every ordered pair, and their ratio;
  (c) the segments of the link walk: edit_compare_us of cmpr_edit_cluster_device under the tunable edit_segments =
      0 (automatic: no segment longer than ED_LINK_SEGMENT references of the largest group) and every value of
      --segments, at d = 1 with ignore_genes and at d = 3 V/J matched; one call each after a warm-up one.

Every step that uses the GPU is a child process under its own time limit; a step that fails ends the run."""

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from cluster_timing import labels_of_pairs, median  # noqa: E402
from hamming_cluster_timing import spread, table_of  # noqa: E402

CASES = ((1, 0), (2, 0), (3, 0), (1, 1))       # (d, ignore_genes)


def the_set(n):
    from compairr_amd import synth
    return synth.make_set(n, 1, prefix="A", pool_size=n // 4)


def options(ignore_genes):
    from compairr_amd import Options, synth
    return Options(n_v_genes=synth.N_V, n_j_genes=synth.N_J, ignore_genes=ignore_genes, device=0)


def measure(n, d, ignore_genes, reps):
    """(child) one JSON line: the new call, the count-only walk and the route without the call on one set"""
    import torch
    from compairr_amd import HipOverlap
    s = the_set(n)
    out = {"n": s.n, "d": d, "g": ignore_genes}
    with HipOverlap(options(ignore_genes)) as h:
        v, keep = HipOverlap.device_view(s)
        d_of = torch.zeros(s.n, dtype=torch.int32, device="cuda")
        d_start = torch.zeros(s.n + 1, dtype=torch.int64, device="cuda")
        d_member = torch.zeros(s.n, dtype=torch.int32, device="cuda")
        d_count = torch.zeros(s.n, dtype=torch.int64, device="cuda")
        d_rows = torch.zeros(s.n + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ms, parts = [], {"group": [], "compare": [], "table": []}
        for k in range(reps + 1):                  # (the first call is the warm-up one)
            t0 = time.perf_counter()
            K = h.edit_cluster_table_device(v, d, d_of.data_ptr(), d_start.data_ptr(), d_member.data_ptr(),
                                            d_count.data_ptr())
            ms.append((time.perf_counter() - t0) * 1e3)
            parts["group"].append(h.get_tunable("edit_group_us") / 1e3)
            parts["compare"].append(h.get_tunable("edit_compare_us") / 1e3)
            parts["table"].append(h.get_tunable("cluster_table_us") / 1e3)
        got = (d_of.cpu().numpy().view(np.uint32), d_start.cpu().numpy().view(np.uint64)[:K + 1],
               d_member.cpu().numpy().view(np.uint32))
        out.update(clusters=K, largest=int(got[1][1]) if K else 0, call_ms=ms[1:],
                   **{"call_%s_ms" % p: x[1:] for p, x in parts.items()})
        # the count-only walk over every ordered pair
        walk = []
        for k in range(reps + 1):
            edges = h.edit_neighbors_device(v, v, d, 0, d_rows.data_ptr())
            walk.append(h.get_tunable("edit_compare_us") / 1e3)
        out.update(edges=edges, count_only_compare_ms=walk[1:])
        # the route without the call
        t0 = time.perf_counter()
        edges = h.edit_neighbors_device(v, v, d, 0, d_rows.data_ptr())
        d_hits = torch.zeros(max(edges, 1), dtype=torch.int32, device="cuda")
        h.edit_neighbors_device(v, v, d, edges, d_rows.data_ptr(), d_hits.data_ptr(), 0)
        t1 = time.perf_counter()
        rows = d_rows.cpu().numpy().view(np.uint64).astype(np.int64)
        hits = d_hits.cpu().numpy().view(np.uint32)[:edges]
        t2 = time.perf_counter()
        label = labels_of_pairs(s.n, np.repeat(np.arange(s.n, dtype=np.uint32), np.diff(rows)), hits)
        t3 = time.perf_counter()
        want = table_of(label)
        t4 = time.perf_counter()
        del keep
    out.update(route_edges_ms=(t1 - t0) * 1e3, route_copy_ms=(t2 - t1) * 1e3, route_union_ms=(t3 - t2) * 1e3,
               route_table_ms=(t4 - t3) * 1e3, route_ms=(t4 - t0) * 1e3, edge_list_bytes=int(4 * edges + 8 * (s.n + 1)),
               tables_equal=bool(all(np.array_equal(a, b) for a, b in zip(got, want))))
    print(json.dumps(out))


def measure_segments(n, d, ignore_genes, segments):
    """(child) one JSON line: the link walk under every forced segment count"""
    import torch
    from compairr_amd import HipOverlap
    s = the_set(n)
    lengths = s.lengths
    key = lengths if ignore_genes else (lengths.astype(np.int64) * 100_000 + s.v_gene) * 100_000 + s.j_gene
    out = {"n": s.n, "d": d, "g": ignore_genes, "largest_group": int(np.unique(key, return_counts=True)[1].max()),
           "compare_ms": {}}
    with HipOverlap(options(ignore_genes)) as h:
        v, keep = HipOverlap.device_view(s)
        d_label = torch.zeros(s.n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        first = None
        for seg in [0, 0] + list(segments):        # (the first call is the warm-up one)
            h.set_tunable("edit_segments", seg)
            K = h.edit_cluster_device(v, d, d_label.data_ptr(), 0)
            label = d_label.cpu().numpy()
            first = label if first is None else first
            out["compare_ms"][str(seg)] = h.get_tunable("edit_compare_us") / 1e3
            out["same_labels"] = out.get("same_labels", True) and bool(np.array_equal(label, first))
        out["clusters"] = K
        del keep
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=3)
    ap.add_argument("--g", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--g-reps", type=int, default=1, help="calls after the warm-up one with ignore_genes")
    ap.add_argument("--segments", default="1,2,4,8,16,32,64")
    ap.add_argument("--rounds", type=int, default=5, help="(a): bench.py runs of each library")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "edit_cluster_timing"))
    ap.add_argument("--against", metavar="LIB", help="the parent commit's library")
    ap.add_argument("--parts", default="abc", help="which of (a), (b), (c) to run")
    ap.add_argument("--child", choices=("measure", "segments"))
    args = ap.parse_args()
    if args.child == "measure":
        return measure(args.n, args.d, bool(args.g), args.reps)
    if args.child == "segments":
        return measure_segments(args.n, args.d, bool(args.g), [int(x) for x in args.segments.split(",") if x])

    os.makedirs(args.out, exist_ok=True)
    lines = ["cmpr_edit_cluster*: the existing workload beside the parent commit, and the new calls "
             "(tools/edit_cluster_timing.py)"]
    status = 0

    def flush():
        with open(os.path.join(args.out, "edit_cluster.txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")

    def failed(what, p):
        lines.append("%s failed with %d: %s" % (what, p.returncode, p.stderr.decode(errors="replace")[-500:]))
        flush()
        print(lines[-1], flush=True)
        return p.returncode or 1

    branch_env = {k: v for k, v in os.environ.items() if k != "COMPAIRR_HIP_LIB"}

    def child(limit, *extra):
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)]
                           + [str(x) for x in extra], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=branch_env)
        return p, (json.loads(p.stdout.decode().strip().splitlines()[-1]) if p.returncode == 0 else None)

    # (a) bench.py, parent and branch in turn
    if "a" not in args.parts:
        lines.append("(a) not asked for")
    elif args.against:
        sides = [("parent", dict(os.environ, COMPAIRR_HIP_LIB=os.path.abspath(args.against))), ("branch", branch_env)]
        values = {"parent": [], "branch": []}
        for rnd in range(args.rounds):
            for side, env in sides:
                p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "bench.py"), "--gpus",
                                    "1", "--steps", str(args.steps), "--warmup", str(args.warmup)],
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=ROOT)
                if p.returncode != 0:
                    return failed("bench.py (%s, round %d)" % (side, rnd), p)
                values[side].append(float(json.loads(p.stdout.decode().strip().splitlines()[-1])["value"]))
                print("%s round %d: %.4g" % (side, rnd, values[side][-1]), flush=True)
        pa, br = values["parent"], values["branch"]
        slower = median(br) < median(pa) - (max(pa) - min(pa))
        lines.append("(a) bench.py --gpus 1 --steps %d --warmup %d, `value` in query sequences/s, %d runs each in turn"
                     % (args.steps, args.warmup, args.rounds))
        for side, xs in (("parent", pa), ("branch", br)):
            lines.append("    %s: %s  median %.4g  min %.4g  max %.4g"
                         % (side, " ".join("%.4g" % x for x in xs), median(xs), min(xs), max(xs)))
        lines.append("    branch median / parent median = %.4f; parent median - branch median = %.4g, parent max - min = "
                     "%.4g: %s" % (median(br) / median(pa), median(pa) - median(br), max(pa) - min(pa),
                                   "SLOWER by more than the parent's own spread" if slower else "within the condition"))
        if slower:
            status = 2
    else:
        lines.append("(a) not measured: no --against library")
    flush()

    # (b) the new call, the count-only walk, the route without the call
    for d, g in CASES if "b" in args.parts else ():
        p, r = child(900, "--child", "measure", "--n", args.n, "--d", d, "--g", g, "--reps",
                     args.g_reps if g else args.reps)
        if r is None:
            return failed("timing child (n = %d, d = %d, g = %d)" % (args.n, d, g), p)
        first = len(lines)
        lines.append("(b) %d CDR3aa, d = %d%s: %d clusters, the largest of %d; %d edges in the pair list"
                     % (r["n"], r["d"], ", ignore_genes" if g else "", r["clusters"], r["largest"], r["edges"]))
        lines.append("    cmpr_edit_cluster_table_device, set in HBM, host ms per call (%d calls after a warm-up): %s"
                     % (len(r["call_ms"]), spread(r["call_ms"])))
        for part, what in (("group", "grouping + jobs"), ("compare", "link kernel + flatten + sizes"), ("table", "table")):
            lines.append("      %-8s %s   (%s)" % (part, spread(r["call_%s_ms" % part]), what))
        lines.append("    without it: cmpr_edit_neighbors_device (count, then fill) %.2f ms + edges to the host (%d bytes) "
                     "%.2f + numpy union-find %.2f + np.lexsort table %.2f = %.2f ms; the two tables equal: %s; the call "
                     "is %.1f times as fast"
                     % (r["route_edges_ms"], r["edge_list_bytes"], r["route_copy_ms"], r["route_union_ms"],
                        r["route_table_ms"], r["route_ms"], r["tables_equal"], r["route_ms"] / median(r["call_ms"])))
        lines.append("    link kernel + flatten + sizes (edit_compare_us) %.2f ms; the count-only walk over every ordered "
                     "pair %.2f ms; ratio %.3f" % (median(r["call_compare_ms"]), median(r["count_only_compare_ms"]),
                                                   median(r["call_compare_ms"]) / median(r["count_only_compare_ms"])))
        flush()
        print("\n".join(lines[first:]), flush=True)
        if not r["tables_equal"]:
            status = status or 3

    # (c) the segments of the link walk
    for d, g in ((1, 1), (3, 0)) if "c" in args.parts else ():
        p, r = child(900, "--child", "segments", "--n", args.n, "--d", d, "--g", g, "--segments", args.segments)
        if r is None:
            return failed("segments child (n = %d, d = %d, g = %d)" % (args.n, d, g), p)
        first = len(lines)
        lines.append("(c) %d CDR3aa, d = %d%s, the largest group of %d sequences: cmpr_edit_cluster_device, "
                     "edit_compare_us in ms by edit_segments (0: automatic); %d clusters, the same labels every time: %s"
                     % (r["n"], r["d"], ", ignore_genes" if g else "", r["largest_group"], r["clusters"],
                        r["same_labels"]))
        lines.append("    " + "   ".join("%s: %.2f" % kv for kv in r["compare_ms"].items()))
        flush()
        print("\n".join(lines[first:]), flush=True)
    return status


if __name__ == "__main__":
    sys.exit(main())
