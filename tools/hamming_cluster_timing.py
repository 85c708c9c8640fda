#!/usr/bin/env python3
"""usage (GPU box): timeout 1100 python3 tools/hamming_cluster_timing.py [--against OTHER/libcompairr_hip.so]
                                                [--n 1000000] [--dense-n 250000] [--parts abc]
                                                [--out build/hamming_cluster_timing]

What cmpr_hamming_cluster_table_device costs, written to <out>/hamming_cluster.txt (the committed copy:
profiles/r17/hamming_cluster.txt).  The one condition is that of (a); the rest is a report.

  (a) bench.py's default `value` (query sequences/s) with this tree's library ("branch") and with --against LIB
      ("parent", the parent commit's build), alternately, --rounds runs each: all values, the medians, the parent's
      own max - min, and whether the branch's median falls below the parent's median by more than that (exit status
      2 when it does: nothing on the hashed path changed, so that would be a finding);
  (b) --n synth.make_set CDR3aa sequences at d = 3, V/J matched and with ignore_genes, the set already in HBM:
        * cmpr_hamming_cluster_table_device, host clock around the synchronous call, --reps calls after a warm-up
          one, and its parts as the library clocks them (hamming_group_us, hamming_compare_us, cluster_table_us);
        * the route to the same table without it: cmpr_hamming_neighbors_device of the set against itself (count,
          then fill, no distances), the edges to the host, a numpy union-find (min-label propagation with pointer
          jumping, as tools/cluster_timing.py), np.lexsort for the cluster order and the members -- clocked in its
          parts; the two tables must be equal;
        * the link kernel against the count-only walk: hamming_compare_us of the new call beside that of the
          count-only cmpr_hamming_neighbors_device call, which walks every ordered pair, and their ratio;
  (c) a dense input: 9001 nucleotide sequences of length 8 over four letters (the `dense` set of the tests) repeated
      to --dense-n sequences, ignore_genes -- ONE group, one cluster, a 37th of all pairs within d = 3 --,
      cmpr_hamming_cluster_device with the root-snapshot shortcut (tunable hamming_link_snapshot = 1) and without.

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


def spread(xs):
    return "%s  median %.2f  min %.2f  max %.2f" % (" ".join("%.2f" % x for x in xs), median(xs), min(xs), max(xs))


def table_of(label):
    """(cluster_of, cluster_start, members) of the partition `label` by np.lexsort"""
    n = len(label)
    label = label.astype(np.int64)
    size = np.bincount(label, minlength=n)
    roots = np.flatnonzero(label == np.arange(n))
    order = roots[np.lexsort((roots, -size[roots]))]
    number = np.zeros(n, dtype=np.int64)
    number[order] = np.arange(len(order))
    cluster_of = number[label]
    members = np.lexsort((np.arange(n), cluster_of))
    start = np.zeros(len(order) + 1, dtype=np.uint64)
    np.cumsum(size[order], out=start[1:])
    return cluster_of.astype(np.uint32), start, members.astype(np.uint32)


def measure(n, d, ignore_genes, reps):
    """(child) one JSON line: the new call, the count-only walk and the route without the call on one set"""
    import torch
    from compairr_amd import HipOverlap, Options, synth
    s = synth.make_set(n, 1, prefix="A", pool_size=n // 4)
    out = {"n": s.n, "d": d, "g": ignore_genes}
    opt = Options(n_v_genes=synth.N_V, n_j_genes=synth.N_J, ignore_genes=ignore_genes, device=0)
    with HipOverlap(opt) as h:
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
            K = h.hamming_cluster_table_device(v, d, d_of.data_ptr(), d_start.data_ptr(), d_member.data_ptr(),
                                               d_count.data_ptr())
            ms.append((time.perf_counter() - t0) * 1e3)
            parts["group"].append(h.get_tunable("hamming_group_us") / 1e3)
            parts["compare"].append(h.get_tunable("hamming_compare_us") / 1e3)
            parts["table"].append(h.get_tunable("cluster_table_us") / 1e3)
        got = (d_of.cpu().numpy().view(np.uint32), d_start.cpu().numpy().view(np.uint64)[:K + 1],
               d_member.cpu().numpy().view(np.uint32))
        out.update(clusters=K, largest=int(got[1][1]) if K else 0, call_ms=ms[1:],
                   **{"call_%s_ms" % p: x[1:] for p, x in parts.items()})
        # the count-only walk over every ordered pair
        walk = []
        for k in range(reps + 1):
            edges = h.hamming_neighbors_device(v, v, d, 0, d_rows.data_ptr())
            walk.append(h.get_tunable("hamming_compare_us") / 1e3)
        out.update(edges=edges, count_only_compare_ms=walk[1:])
        # the route without the call
        t0 = time.perf_counter()
        edges = h.hamming_neighbors_device(v, v, d, 0, d_rows.data_ptr())
        d_hits = torch.zeros(max(edges, 1), dtype=torch.int32, device="cuda")
        h.hamming_neighbors_device(v, v, d, edges, d_rows.data_ptr(), d_hits.data_ptr(), 0)
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


def measure_dense(n, reps):
    """(child) one JSON line: one dense group with and without the root-snapshot shortcut"""
    import torch
    from compairr_amd import HipOverlap, Options, synth
    base = synth.tiny_set(9001, 12, alphabet_size=4, letters=4, min_len=8, max_len=8)
    s = base.subset(np.arange(n) % base.n)
    out = {"n": s.n}
    with HipOverlap(Options(n_v_genes=2, n_j_genes=2, nucleotides=True, ignore_genes=True, device=0)) as h:
        v, keep = HipOverlap.device_view(s)
        d_label = torch.zeros(s.n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for snapshot in (1, 0):
            h.set_tunable("hamming_link_snapshot", snapshot)
            ms, compare = [], []
            for k in range(reps + 1):
                t0 = time.perf_counter()
                K = h.hamming_cluster_device(v, 3, d_label.data_ptr(), 0)
                ms.append((time.perf_counter() - t0) * 1e3)
                compare.append(h.get_tunable("hamming_compare_us") / 1e3)
            out["snapshot%d" % snapshot] = {"ms": ms[1:], "compare_ms": compare[1:], "clusters": K,
                                            "labels_zero": bool((d_label == 0).all().item())}
        del keep
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dense-n", type=int, default=250_000)
    ap.add_argument("--d", type=int, default=3)
    ap.add_argument("--g", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="(a): bench.py runs of each library")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "hamming_cluster_timing"))
    ap.add_argument("--against", metavar="LIB", help="the parent commit's library")
    ap.add_argument("--parts", default="abc", help="which of (a), (b), (c) to run")
    ap.add_argument("--child", choices=("measure", "dense"))
    args = ap.parse_args()
    if args.child == "measure":
        return measure(args.n, args.d, bool(args.g), args.reps)
    if args.child == "dense":
        return measure_dense(args.n, args.reps)

    os.makedirs(args.out, exist_ok=True)
    lines = ["cmpr_hamming_cluster*: the existing workload beside the parent commit, and the new calls "
             "(tools/hamming_cluster_timing.py)"]
    status = 0

    def flush():
        with open(os.path.join(args.out, "hamming_cluster.txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")

    def failed(what, p):
        lines.append("%s failed with %d: %s" % (what, p.returncode, p.stderr.decode(errors="replace")[-500:]))
        flush()
        print(lines[-1], flush=True)
        return p.returncode or 1

    branch_env = {k: v for k, v in os.environ.items() if k != "COMPAIRR_HIP_LIB"}

    def child(limit, *extra):
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--reps",
                            str(args.reps)] + [str(x) for x in extra], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           env=branch_env)
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
    for g in (0, 1) if "b" in args.parts else ():
        p, r = child(500, "--child", "measure", "--n", args.n, "--d", args.d, "--g", g)
        if r is None:
            return failed("timing child (n = %d, d = %d, g = %d)" % (args.n, args.d, g), p)
        first = len(lines)
        lines.append("(b) %d CDR3aa, d = %d%s: %d clusters, the largest of %d; %d edges in the pair list"
                     % (r["n"], r["d"], ", ignore_genes" if g else "", r["clusters"], r["largest"], r["edges"]))
        lines.append("    cmpr_hamming_cluster_table_device, set in HBM, host ms per call (%d calls after a warm-up): %s"
                     % (len(r["call_ms"]), spread(r["call_ms"])))
        for part in ("group", "compare", "table"):
            lines.append("      %-8s %s" % (part, spread(r["call_%s_ms" % part])))
        lines.append("    without it: cmpr_hamming_neighbors_device (count, then fill) %.2f ms + edges to the host (%d bytes) "
                     "%.2f + numpy union-find %.2f + np.lexsort table %.2f = %.2f ms; the two tables equal: %s"
                     % (r["route_edges_ms"], r["edge_list_bytes"], r["route_copy_ms"], r["route_union_ms"],
                        r["route_table_ms"], r["route_ms"], r["tables_equal"]))
        lines.append("    link kernel + flatten + sizes (hamming_compare_us) %.2f ms; the count-only walk over every ordered "
                     "pair %.2f ms; ratio %.3f" % (median(r["call_compare_ms"]), median(r["count_only_compare_ms"]),
                                                   median(r["call_compare_ms"]) / median(r["count_only_compare_ms"])))
        flush()
        print("\n".join(lines[first:]), flush=True)
        if not r["tables_equal"]:
            status = status or 3

    # (c) one dense group, with and without the root snapshots
    if "c" not in args.parts:
        return status
    p, r = child(500, "--child", "dense", "--n", args.dense_n)
    if r is None:
        return failed("dense child", p)
    first = len(lines)
    lines.append("(c) %d nucleotide sequences of length 8 in ONE group (9001 distinct rows repeated), d = 3, ignore_genes: "
                 "cmpr_hamming_cluster_device" % r["n"])
    for snapshot in (1, 0):
        x = r["snapshot%d" % snapshot]
        lines.append("    hamming_link_snapshot = %d: %d cluster(s), every label 0: %s; host ms per call: %s"
                     % (snapshot, x["clusters"], x["labels_zero"], spread(x["ms"])))
        lines.append("      compare  %s" % spread(x["compare_ms"]))
    lines.append("    compare without / with the snapshots = %.2f"
                 % (median(r["snapshot0"]["compare_ms"]) / median(r["snapshot1"]["compare_ms"])))
    flush()
    print("\n".join(lines[first:]), flush=True)
    return status


if __name__ == "__main__":
    sys.exit(main())
