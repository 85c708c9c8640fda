#!/usr/bin/env python3
"""usage (GPU box): timeout 1100 python3 tools/edit_nearest_timing.py [--against OTHER/libcompairr_hip.so]
                                                [--n 1000000] [--out build/edit_nearest_timing]

What cmpr_edit_nearest_device costs, written to <out>/edit_nearest.txt (the committed copy:
profiles/r24/edit_nearest.txt).  The one condition is that of (a); the rest is a report.

  (a) bench.py's default `value` (query sequences/s) with this tree's library ("branch") and with --against LIB
      ("parent", the parent commit's build), alternately, --rounds runs each: all values, the medians, the parent's
      own max - min, and whether the branch's median falls below the parent's median by more than that (exit status
      2 when it does: no existing kernel changed, so that would be a finding);
  (b) --n synth.make_set CDR3aa sequences against as many of another seed, V/J matched and with ignore_genes, and
      --nt-n nucleotide sequences with ignore_genes, the sets already in HBM, at max_distance 3 and uncapped:
      cmpr_edit_nearest_device (min_distance 1, all three outputs) with the length-gap stop (the tunable
      edit_nearest_prune 1) and without it (0), host clock around the synchronous call, --reps calls after a warm-up
      one, and the parts as the library clocks them (tunables edit_{group,compare}_us); beside it the count-only call
      of cmpr_edit_neighbors_device at d = the cap on the same sets -- the same walk without the sink --; the ratios
      of the compare parts (sink: stop off / count-only; stop: on / off); the histogram of the nearest distances, and
      whether the two settings of the stop gave the same three arrays;
  (c) the route without this call on a SAMPLE of --sample-n V/J-matched CDR3aa sequences per set, where it still
      fits: cmpr_edit_neighbors_device with `differences` = the longest length (every same-gene pair as an edge),
      filled, and a segmented minimum in torch, checked to give the same three arrays.

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

PARTS = ("group", "compare")


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else (xs[len(xs) // 2 - 1] + xs[len(xs) // 2]) / 2


def spread(xs):
    return "%s  median %.2f  min %.2f  max %.2f" % (" ".join("%.2f" % x for x in xs), median(xs), min(xs), max(xs))


def timed(h, call, reps):
    ms, parts = [], {p: [] for p in PARTS}
    for k in range(reps + 1):                      # (the first call is the warm-up one)
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
        for p in PARTS:
            parts[p].append(h.get_tunable("edit_%s_us" % p) / 1e3)
    return ms[1:], {p: v[1:] for p, v in parts.items()}


def sets_of(n, nucleotides):
    from compairr_amd import synth
    return (synth.make_set(n, 1, prefix="A", pool_size=n // 4, nucleotides=nucleotides),
            synth.make_set(n, 2, prefix="B", pool_size=n // 4, nucleotides=nucleotides))


def pairs_of(s1, s2, ignore_genes, cap):
    """the pairs a walk without the stop compares: same V and J unless ignore_genes, lengths no more than cap apart"""
    longest = int(max(s1.longest, s2.longest))

    def table(s):
        genes = np.zeros(s.n, dtype=np.int64) if ignore_genes else s.v_gene.astype(np.int64) * 4096 + s.j_gene
        return genes, s.lengths.astype(np.int64)
    g1, l1 = table(s1)
    g2, l2 = table(s2)
    names, inverse = np.unique(np.concatenate([g1, g2]), return_inverse=True)
    c1 = np.zeros((len(names), longest + 1), dtype=np.int64)
    c2 = np.zeros_like(c1)
    np.add.at(c1, (inverse[:s1.n], l1), 1)
    np.add.at(c2, (inverse[s1.n:], l2), 1)
    total = int((c1 * c2).sum())
    for gap in range(1, min(cap, longest) + 1):
        total += int((c1[:, gap:] * c2[:, :-gap]).sum()) + int((c1[:, :-gap] * c2[:, gap:]).sum())
    return total


def outputs(torch, n):
    return (torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int16, device="cuda"),
            torch.zeros(n, dtype=torch.int32, device="cuda"))


def measure(n, ignore_genes, nucleotides, cap, reps):
    """(child) one JSON line: the nearest call with and without the stop and the count-only neighbour call at the
    cap (cap < 0: uncapped) on one pair of sets"""
    import torch
    from compairr_amd import HipOverlap, Options, synth
    a, b = sets_of(n, nucleotides)
    longest = int(max(a.longest, b.longest))
    out = {"n": n, "g": ignore_genes, "nt": nucleotides, "cap": cap,
           "pairs": pairs_of(a, b, ignore_genes, longest if cap < 0 else cap)}
    opt = Options(n_v_genes=synth.N_V, n_j_genes=synth.N_J, ignore_genes=ignore_genes, nucleotides=nucleotides, device=0)
    with HipOverlap(opt) as h:
        v1, keep1 = HipOverlap.device_view(a)
        v2, keep2 = HipOverlap.device_view(b)
        arrays = {prune: outputs(torch, a.n) for prune in (1, 0)}
        torch.cuda.synchronize()
        for prune in (1, 0):
            d_near, d_dist, d_ties = arrays[prune]
            found = [0]
            h.set_tunable("edit_nearest_prune", prune)

            def nearest():
                found[0] = h.edit_nearest_device(v1, v2, 1, None if cap < 0 else cap, 0, d_near.data_ptr(),
                                                 d_dist.data_ptr(), d_ties.data_ptr())
            ms, parts = timed(h, nearest, reps)
            out.update({"prune%d_ms" % prune: ms, "found": found[0]},
                       **{"prune%d_%s_ms" % (prune, p): v for p, v in parts.items()})
        d_near, d_dist, d_ties = arrays[1]
        has = d_ties != 0
        out.update(sum_ties=int(d_ties.to(torch.int64).sum().item()),
                   histogram=torch.bincount(d_dist[has].to(torch.int64) & 0xFFFF).cpu().tolist(),
                   equal=all(bool(torch.equal(x, y)) for x, y in zip(arrays[1], arrays[0])))
        edges = [0]

        def count():
            edges[0] = h.edit_neighbors_device(v1, v2, longest if cap < 0 else cap, 0)
        ms, parts = timed(h, count, reps)
        out.update(count_ms=ms, edges=edges[0], **{"count_%s_ms" % p: v for p, v in parts.items()})
    print(json.dumps(out))


def measure_route(n, reps):
    """(child) one JSON line: every same-gene pair as an edge and a segmented minimum in torch, beside the call"""
    import torch
    from compairr_amd import HipOverlap, Options, synth
    a, b = sets_of(n, False)
    out = {"n": n}
    with HipOverlap(Options(n_v_genes=synth.N_V, n_j_genes=synth.N_J, device=0)) as h:
        v1, keep1 = HipOverlap.device_view(a)
        v2, keep2 = HipOverlap.device_view(b)
        d_near, d_dist, d_ties = outputs(torch, a.n)
        d_rows = torch.zeros(a.n + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ms, _ = timed(h, lambda: h.edit_nearest_device(v1, v2, 1, None, 0, d_near.data_ptr(), d_dist.data_ptr(),
                                                       d_ties.data_ptr()), reps)
        out["nearest_ms"] = ms
        longest = int(max(a.longest, b.longest))
        route, equal = [], True
        for k in range(reps + 1):
            t0 = time.perf_counter()
            edges = h.edit_neighbors_device(v1, v2, longest, 0, d_rows.data_ptr())
            d_hits = torch.empty(max(edges, 1), dtype=torch.int32, device="cuda")
            d_edge = torch.empty(max(edges, 1), dtype=torch.int16, device="cuda")
            h.edit_neighbors_device(v1, v2, longest, edges, d_rows.data_ptr(), d_hits.data_ptr(), d_edge.data_ptr())
            query = torch.repeat_interleave(torch.arange(a.n, device="cuda"), torch.diff(d_rows))
            key = ((d_edge[:edges].to(torch.int64) & 0xFFFF) << 32) | (d_hits[:edges].to(torch.int64) & 0xFFFFFFFF)
            keep = (key >> 32) >= 1                                      # (min_distance 1)
            query, key = query[keep], key[keep]
            best = torch.full((a.n,), 2 ** 62, dtype=torch.int64, device="cuda").scatter_reduce(0, query, key, "amin")
            ties = torch.zeros(a.n, dtype=torch.int64, device="cuda").index_add_(
                0, query, ((key >> 32) == (best[query] >> 32)).to(torch.int64))
            torch.cuda.synchronize()
            route.append((time.perf_counter() - t0) * 1e3)
            has = ties != 0
            equal &= bool(torch.equal(has, d_ties != 0)
                          and torch.equal(best[has] & 0xFFFFFFFF, d_near[has].to(torch.int64) & 0xFFFFFFFF)
                          and torch.equal(best[has] >> 32, d_dist[has].to(torch.int64) & 0xFFFF)
                          and torch.equal(ties, d_ties.to(torch.int64)))
            del d_hits, d_edge, query, key, keep, best, ties
        out.update(route_ms=route[1:], edges=edges, equal=equal)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nt-n", type=int, default=100_000)
    ap.add_argument("--sample-n", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3, help="(a): bench.py runs of each library")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds a timing child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "edit_nearest_timing"))
    ap.add_argument("--against", metavar="LIB", help="the parent commit's library")
    ap.add_argument("--child", choices=("measure", "route"))
    ap.add_argument("--g", type=int, default=0)
    ap.add_argument("--nt", type=int, default=0)
    ap.add_argument("--cap", type=int, default=-1)
    args = ap.parse_args()
    if args.child == "measure":
        return measure(args.n, bool(args.g), bool(args.nt), args.cap, args.reps)
    if args.child == "route":
        return measure_route(args.n, args.reps)

    os.makedirs(args.out, exist_ok=True)
    lines = ["cmpr_edit_nearest_device: the existing workload beside the parent commit, and the new call "
             "(tools/edit_nearest_timing.py)"]
    status = 0
    branch_env = {k: v for k, v in os.environ.items() if k != "COMPAIRR_HIP_LIB"}

    def flush():
        with open(os.path.join(args.out, "edit_nearest.txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")

    def failed(what, p):
        lines.append("%s failed with %d: %s" % (what, p.returncode, p.stderr.decode(errors="replace")[-500:]))
        flush()
        print(lines[-1], flush=True)
        return p.returncode or 1

    def child(limit, reps, *extra):
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--reps",
                            str(reps)] + [str(x) for x in extra], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           env=branch_env)
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

    # (b) the new call with and without the stop, beside the count-only walk at the cap
    for n, g, nt in ((args.n, 0, 0), (args.n, 1, 0), (args.nt_n, 1, 1)):
        for cap in (3, -1):
            # (a walk of some 10^12 pairs takes ten seconds and more: one call after the warm-up one)
            reps = 1 if g and not nt else args.reps
            p, r = child(args.limit, reps, "--child", "measure", "--n", n, "--g", g, "--nt", nt, "--cap", cap)
            if r is None:
                return failed("timing child (n = %d, g = %d, nt = %d, cap = %d)" % (n, g, nt, cap), p)
            first = len(lines)
            lines.append("(b) %d x %d %s%s, min_distance 1, max_distance %s: %d pairs within the cap; %d sequences have a "
                         "neighbour, ties in all %d, nearest distances %s"
                         % (n, n, "nucleotide sequences" if nt else "CDR3aa", ", ignore_genes" if g else ", V/J matched",
                            "none" if cap < 0 else cap, r["pairs"], r["found"], r["sum_ties"], r["histogram"]))
            for prune in (1, 0):
                lines.append("    cmpr_edit_nearest_device, edit_nearest_prune %d, sets in HBM, host ms per call (%d calls after a "
                             "warm-up): %s" % (prune, len(r["prune%d_ms" % prune]), spread(r["prune%d_ms" % prune])))
                for part in PARTS:
                    lines.append("      %-8s %s" % (part, spread(r["prune%d_%s_ms" % (prune, part)])))
            lines.append("      the same three arrays with and without the stop: %s" % r["equal"])
            lines.append("    cmpr_edit_neighbors_device, count-only, d = %s (%d edges): %s"
                         % ("the longest length" if cap < 0 else cap, r["edges"], spread(r["count_ms"])))
            for part in PARTS:
                lines.append("      %-8s %s" % (part, spread(r["count_%s_ms" % part])))
            lines.append("      compare kernel, count-only: %.3g pairs/s" % (r["pairs"] / (median(r["count_compare_ms"]) / 1e3)))
            lines.append("    compare part: the sink, stop off / count-only = %.3f; the stop, on / off = %.3f"
                         % (median(r["prune0_compare_ms"]) / median(r["count_compare_ms"]),
                            median(r["prune1_compare_ms"]) / median(r["prune0_compare_ms"])))
            if not r["equal"]:
                status = status or 3
            flush()
            print("\n".join(lines[first:]), flush=True)

    # (c) the route without the call, on a sample
    p, r = child(args.limit, args.reps, "--child", "route", "--n", args.sample_n)
    if r is None:
        return failed("route child", p)
    first = len(lines)
    lines.append("(c) SAMPLE of %d x %d CDR3aa, V/J matched: cmpr_edit_neighbors_device with differences = the longest "
                 "length (count, then %d edges filled) and a segmented minimum in torch, ms: %s"
                 % (r["n"], r["n"], r["edges"], spread(r["route_ms"])))
    lines.append("    cmpr_edit_nearest_device on the same sample, min_distance 1, uncapped, ms: %s" % spread(r["nearest_ms"]))
    lines.append("    the three arrays equal: %s" % r["equal"])
    if not r["equal"]:
        status = status or 3
    flush()
    print("\n".join(lines[first:]), flush=True)
    return status


if __name__ == "__main__":
    sys.exit(main())
