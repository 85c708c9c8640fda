#!/usr/bin/env python3
"""usage (GPU box): timeout 1100 python3 tools/neighbors_timing.py [--against OTHER/libcompairr_hip.so]
                                                  [--sizes 1000000,10000000] [--out build/neighbors_timing]

What the neighbour branch in score_match costs the existing workload and what cmpr_neighbors_device costs and
gains, written to <out>/neighbors.txt (the committed copy: profiles/r11/neighbors.txt).  The one condition is
that of (a); the rest is a report.

  (a) bench.py's default `value` (query sequences/s) with this tree's library ("branch") and with --against LIB
      (COMPAIRR_HIP_LIB; "parent", the parent commit's build), alternately, --rounds runs each: all values, the
      medians, the parent's own max - min, and whether the branch's median falls below the parent's median by
      more than that (exit status 2 when it does: the cause is then in how the mode was wired into score_match);
  (b) per size of --sizes, synth.make_set CDR3aa sequences (uniform law, as bench.py builds its sets) against
      themselves at d = 1, V/J matched, the sets resident:
        * cmpr_neighbors_device with both arrays already in HBM and the exact capacity, host clock around the
          synchronous call, --reps calls after a warm-up one;
        * its parts as the library clocks them (tunables neighbors_{count,scan,fill,order}_us: host clock,
          each part ends in a wait): the count step, the sum, the fill step, the ordering of the rows;
        * the route to the same CSR that exists without it: cmpr_overlap_pairs to the host (count, then list),
          np.lexsort, np.bincount + np.cumsum -- clocked in its parts; the two results must be equal.

  (c) per size of --sizes and for d = 1 and d = 2 (--distance-d), the same sets against themselves:
        * cmpr_neighbors_distance_device with the three arrays in HBM and the exact capacity, and its parts, beside
          cmpr_neighbors_device on the same context (the hits of the two must be equal, and the distances lie in
          0 .. d with every value present);
        * at d = 2 the route to the graphs at d <= 0, <= 1, <= 2 that exists without it: one cmpr_neighbors_device
          call on each of three resident contexts of d = 0, 1, 2 (the calls alone; the contexts are set up before).
      Skipped when the timed library lacks the entry point (the parent commit's).

Without --against, (a) is skipped and (b) times the library the environment names (COMPAIRR_HIP_LIB, e.g. the parent
commit's build, for the same report of the parent), or this tree's when it names none.

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

PARTS = ("count", "scan", "fill", "order")


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else (xs[len(xs) // 2 - 1] + xs[len(xs) // 2]) / 2


def spread(xs):
    return "%s  median %.2f  min %.2f  max %.2f" % (" ".join("%.2f" % x for x in xs), median(xs), min(xs), max(xs))


def measure(n, reps):
    """(child) one JSON line for one set size"""
    import ctypes as C
    import torch
    from compairr_amd import HipOverlap, Options, synth
    opt = Options(differences=1, n_v_genes=synth.N_V, n_j_genes=synth.N_J, device=0)
    s = synth.make_set(n, 2, prefix="B", pool_size=n // 4)
    out = {"n": s.n}
    with HipOverlap(opt) as h:
        h.set_reference(s, s.longest)
        h.set_queries(s)
        edges = h.neighbors_device(0, 0, 0)
        d_rows = torch.zeros(s.n + 1, dtype=torch.int64, device="cuda")
        d_hits = torch.zeros(max(edges, 1), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ms, parts = [], {p: [] for p in PARTS}
        for k in range(reps + 1):              # (the first call is the warm-up one)
            t0 = time.perf_counter()
            got = h.neighbors_device(edges, d_rows.data_ptr(), d_hits.data_ptr())
            ms.append((time.perf_counter() - t0) * 1e3)
            assert got == edges
            for p in PARTS:
                parts[p].append(h.get_tunable("neighbors_%s_us" % p) / 1e3)
        degree_ms = []
        for k in range(reps + 1):
            t0 = time.perf_counter()
            h.neighbors_device(0, d_rows.data_ptr(), 0)
            degree_ms.append((time.perf_counter() - t0) * 1e3)
        row_start = d_rows.cpu().numpy().view(np.uint64)
        hits = d_hits.cpu().numpy().view(np.uint32)[:edges]
        deg = np.diff(row_start.astype(np.int64))
        out.update(edges=edges, longest=int(deg.max()), rows_above_8=int((deg > 8).sum()),
                   rows_above_64=int((deg > 64).sum()), neighbors_ms=ms[1:], degree_only_ms=degree_ms[1:],
                   **{"%s_ms" % p: parts[p][1:] for p in PARTS})
        # the route that exists without the call, on the same resident sets
        route = {"pairs": [], "lexsort": [], "bincount": [], "all": []}
        for k in range(reps):
            t0 = time.perf_counter()
            npairs = C.c_uint64()
            h._check(h._lib.cmpr_overlap_pairs(h._ctx, 0, None, None, C.byref(npairs)))
            q = np.zeros(npairs.value, dtype=np.uint32)
            hit = np.zeros(npairs.value, dtype=np.uint32)
            h._check(h._lib.cmpr_overlap_pairs(h._ctx, npairs.value, q.ctypes.data, hit.ctypes.data, C.byref(npairs)))
            t1 = time.perf_counter()
            order = np.lexsort((hit, q))
            want_hits = hit[order]
            t2 = time.perf_counter()
            want_rows = np.zeros(s.n + 1, dtype=np.uint64)
            np.cumsum(np.bincount(q, minlength=s.n), out=want_rows[1:])
            t3 = time.perf_counter()
            for name, dt in zip(("pairs", "lexsort", "bincount", "all"), (t1 - t0, t2 - t1, t3 - t2, t3 - t0)):
                route[name].append(dt * 1e3)
        out.update(equal=bool(np.array_equal(row_start, want_rows) and np.array_equal(hits, want_hits)),
                   **{"route_%s_ms" % k: v for k, v in route.items()})
    print(json.dumps(out))


def timed_calls(h, call, reps):
    """host ms per call and the library's parts, `reps` calls after a warm-up one"""
    ms, parts = [], {p: [] for p in PARTS}
    for k in range(reps + 1):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
        for p in PARTS:
            parts[p].append(h.get_tunable("neighbors_%s_us" % p) / 1e3)
    return ms[1:], {p: v[1:] for p, v in parts.items()}


def measure_distance(n, d, reps):
    """(child) one JSON line for one set size and one d: the distance call beside cmpr_neighbors_device"""
    import torch
    from compairr_amd import HipOverlap, Options, synth
    s = synth.make_set(n, 2, prefix="B", pool_size=n // 4)
    out = {"n": s.n, "d": d}

    def context(dd):
        h = HipOverlap(Options(differences=dd, n_v_genes=synth.N_V, n_j_genes=synth.N_J, device=0))
        h.set_reference(s, s.longest)
        h.set_queries(s)
        return h

    with context(d) as h:
        if not hasattr(h._lib, "cmpr_neighbors_distance_device"):
            print(json.dumps(dict(out, missing=True)))
            return
        edges = h.neighbors_device(0, 0, 0)
        d_rows = torch.zeros(s.n + 1, dtype=torch.int64, device="cuda")
        d_hits = torch.zeros(max(edges, 1), dtype=torch.int32, device="cuda")
        d_hits2 = torch.zeros(max(edges, 1), dtype=torch.int32, device="cuda")
        d_dist = torch.full((max(edges, 1),), 255, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ms, parts = timed_calls(h, lambda: h.neighbors_device(edges, d_rows.data_ptr(), d_hits.data_ptr()), reps)
        out.update(edges=edges, neighbors_ms=ms, **{"neighbors_%s_ms" % p: v for p, v in parts.items()})
        ms, parts = timed_calls(h, lambda: h.neighbors_distance_device(edges, d_rows.data_ptr(), d_hits2.data_ptr(),
                                                                       d_dist.data_ptr()), reps)
        out.update(distance_ms=ms, **{"distance_%s_ms" % p: v for p, v in parts.items()})
        hist = torch.bincount(d_dist[:edges].to(torch.int64), minlength=3).cpu().tolist()
        out.update(histogram=hist, equal=bool(torch.equal(d_hits[:edges], d_hits2[:edges]) and sum(hist[:d + 1]) == edges
                                              and all(x > 0 for x in hist[:d + 1])))
        del d_hits2, d_dist
    if d == 2:
        # the route without the call: a context per d, one cmpr_neighbors_device call on each
        per_d = []
        for dd in (0, 1, 2):
            with context(dd) as h:
                e = h.neighbors_device(0, 0, 0)
                hits = torch.zeros(max(e, 1), dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                ms, _ = timed_calls(h, lambda: h.neighbors_device(e, d_rows.data_ptr(), hits.data_ptr()), reps)
                per_d.append(ms)
                del hits
        out.update(three_contexts_ms=[sum(x) for x in zip(*per_d)], per_context_ms=[median(x) for x in per_d])
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="(a): bench.py runs of each library")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "neighbors_timing"))
    ap.add_argument("--against", metavar="LIB", help="the parent commit's library")
    ap.add_argument("--measure", type=int, default=0, metavar="N", help="(child) time one set size, print one JSON line")
    ap.add_argument("--distance-d", default="1,2", help="(c): the d of the cmpr_neighbors_distance_device timings; empty: none")
    ap.add_argument("--measure-distance", type=int, default=0, metavar="N", help="(child) (c) for one set size and --d")
    ap.add_argument("--d", type=int, default=1, help="(child) the d of --measure-distance")
    args = ap.parse_args()
    if args.measure:
        return measure(args.measure, args.reps)
    if args.measure_distance:
        return measure_distance(args.measure_distance, args.d, args.reps)

    os.makedirs(args.out, exist_ok=True)
    lines = ["cmpr_neighbors: cost to the existing workload and the new call (tools/neighbors_timing.py)"]
    status = 0

    def flush():
        with open(os.path.join(args.out, "neighbors.txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")

    def failed(what, p):
        lines.append("%s failed with %d: %s" % (what, p.returncode, p.stderr.decode(errors="replace")[-500:]))
        flush()
        print(lines[-1], flush=True)
        return p.returncode or 1

    branch_env = {k: v for k, v in os.environ.items() if k != "COMPAIRR_HIP_LIB"}
    # (b) times this tree's library beside a comparison; without --against, whichever library the caller's
    # environment names (COMPAIRR_HIP_LIB: the parent commit's build, for the same report of the parent)
    timed_env = branch_env if args.against else dict(os.environ)
    if not args.against and os.environ.get("COMPAIRR_HIP_LIB"):
        lines.append("(b) is of the library COMPAIRR_HIP_LIB names, not of this tree's")

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

    # (b) the new call
    me = [sys.executable, os.path.abspath(__file__)]
    for n in [int(x) for x in args.sizes.split(",") if x]:
        p = subprocess.run(["timeout", "-k", "10", "500"] + me + ["--measure", str(n), "--reps", str(args.reps)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=timed_env)
        if p.returncode != 0:
            return failed("timing child (n = %d)" % n, p)
        r = json.loads(p.stdout.decode().strip().splitlines()[-1])
        first = len(lines)
        lines.append("(b) n = %d CDR3aa against themselves, d = 1: %d edges, longest row %d, rows above 8: %d, above 64: %d; "
                     "both routes equal: %s" % (r["n"], r["edges"], r["longest"], r["rows_above_8"], r["rows_above_64"], r["equal"]))
        lines.append("    cmpr_neighbors_device, arrays in HBM, host ms per call (%d calls after a warm-up): %s"
                     % (len(r["neighbors_ms"]), spread(r["neighbors_ms"])))
        for part, what in zip(PARTS, ("count step", "sum + census", "fill step", "rows ordered")):
            lines.append("      %-13s %s" % (what, spread(r["%s_ms" % part])))
        lines.append("    degree-only call (row_start in HBM): %s" % spread(r["degree_only_ms"]))
        lines.append("    without it, same resident sets: cmpr_overlap_pairs (count, then list to the host) %s"
                     % spread(r["route_pairs_ms"]))
        lines.append("      np.lexsort    %s" % spread(r["route_lexsort_ms"]))
        lines.append("      bincount+sum  %s" % spread(r["route_bincount_ms"]))
        lines.append("      in all        %s" % spread(r["route_all_ms"]))
        flush()
        print("\n".join(lines[first:]), flush=True)
        if not r["equal"]:
            lines.append("n = %d: the two routes differ" % n)
            flush()
            return 1

    # (c) the distance of every edge
    for n in [int(x) for x in args.sizes.split(",") if x]:
        for d in [int(x) for x in args.distance_d.split(",") if x]:
            p = subprocess.run(["timeout", "-k", "10", "500"] + me + ["--measure-distance", str(n), "--d", str(d), "--reps",
                                                                     str(args.reps)],
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=timed_env)
            if p.returncode != 0:
                return failed("distance timing child (n = %d, d = %d)" % (n, d), p)
            r = json.loads(p.stdout.decode().strip().splitlines()[-1])
            if r.get("missing"):
                lines.append("(c) not measured: the timed library has no cmpr_neighbors_distance_device")
                break
            first = len(lines)
            lines.append("(c) n = %d CDR3aa against themselves, d = %d: %d edges, [d0, d1, d2] = %s; hits equal to "
                         "cmpr_neighbors_device's and every distance in 0 .. d: %s" % (r["n"], d, r["edges"], r["histogram"], r["equal"]))
            for call, what in (("neighbors", "cmpr_neighbors_device"), ("distance", "cmpr_neighbors_distance_device")):
                lines.append("    %s, arrays in HBM, host ms per call (%d calls after a warm-up): %s"
                             % (what, len(r["%s_ms" % call]), spread(r["%s_ms" % call])))
                for part, name in zip(PARTS, ("count step", "sum + census", "fill step", "rows ordered")):
                    lines.append("      %-13s %s" % (name, spread(r["%s_%s_ms" % (call, part)])))
            if "three_contexts_ms" in r:
                lines.append("    without it: cmpr_neighbors_device on three resident contexts of d = 0, 1, 2, the three calls in all: %s"
                             % spread(r["three_contexts_ms"]))
                lines.append("      medians per context d = 0, 1, 2: %s" % " ".join("%.2f" % x for x in r["per_context_ms"]))
            flush()
            print("\n".join(lines[first:]), flush=True)
            if not r["equal"]:
                lines.append("n = %d, d = %d: the two calls differ" % (n, d))
                flush()
                return 1
    flush()
    print("\n".join(lines), flush=True)
    return status


if __name__ == "__main__":
    sys.exit(main())
