#!/usr/bin/env python3
"""usage (GPU box): timeout 1100 python3 tools/existence_timing.py [--against OTHER/libcompairr_hip.so]
                                                  [--sizes 1000000,10000000] [--reps-of-set 16,80]
                                                  [--out build/existence_timing]

What cmpr_existence_csr costs the existing workload (nothing of a step changed: the condition of (a) guards the
build) and what the call costs and gains, written to <out>/existence.txt (the committed copy:
profiles/r12/existence.txt).  The one condition is that of (a); the rest is a report.

  (a) bench.py's default `value` (query sequences/s) with this tree's library ("branch") and with --against LIB
      (COMPAIRR_HIP_LIB; "parent", the parent commit's build), alternately, --rounds runs each: all values, the
      medians, the parent's own max - min, and whether the branch's median falls below the parent's median by
      more than that (exit status 2 when it does);
  (b) per size of --sizes and per repertoire count of --reps-of-set, synth.make_set CDR3aa sequences against
      themselves at d = 1, V/J matched, the sets resident:
        * cmpr_existence_csr_device with its three arrays already in HBM and the exact capacity, host clock around
          the synchronous call, --reps calls after a warm-up one, and its parts as the library clocks them
          (tunables existence_{edges,group,count,reduce}_us; the grouping kernels are only enqueued unless a row
          beyond LDS makes the host wait, so their device time shows in the next part);
        * cmpr_neighbors_device on the same resident sets: the part of the call that existed before;
        * the route that exists without the call: a context with options.existence, cmpr_overlap_matrix_device
          into an n x R2 torch buffer, torch.nonzero and a gather; the two results must be equal.

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

PARTS = ("edges", "group", "count", "reduce")


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else (xs[len(xs) // 2 - 1] + xs[len(xs) // 2]) / 2


def spread(xs):
    return "%s  median %.2f  min %.2f  max %.2f" % (" ".join("%.2f" % x for x in xs), median(xs), min(xs), max(xs))


def measure(n, n_rep, reps):
    """(child) one JSON line for one set size and repertoire count"""
    import dataclasses
    import torch
    from compairr_amd import HipOverlap, Options, synth
    opt = Options(differences=1, n_v_genes=synth.N_V, n_j_genes=synth.N_J, device=0)
    s = synth.make_set(n, 2, prefix="B", pool_size=n // 4, n_repertoires=n_rep)
    out = {"n": s.n, "repertoires": s.n_repertoires}
    with HipOverlap(opt) as h:
        h.set_reference(s, s.longest)
        h.set_queries(s)
        cells = h.existence_csr_device(0, 0, 0, 0)
        edges = h.stats().matches
        d_rows = torch.zeros(s.n + 1, dtype=torch.int64, device="cuda")
        d_rep = torch.zeros(max(cells, 1), dtype=torch.int32, device="cuda")
        d_val = torch.zeros(max(cells, 1), dtype=torch.int64, device="cuda")
        d_hits = torch.zeros(max(edges, 1), dtype=torch.int32, device="cuda")
        d_erows = torch.zeros(s.n + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ms, parts, count_ms, nb_ms = [], {p: [] for p in PARTS}, [], []
        for k in range(reps + 1):              # (the first call is the warm-up one)
            t0 = time.perf_counter()
            got = h.existence_csr_device(cells, d_rows.data_ptr(), d_rep.data_ptr(), d_val.data_ptr())
            ms.append((time.perf_counter() - t0) * 1e3)
            assert got == cells
            for p in PARTS:
                parts[p].append(h.get_tunable("existence_%s_us" % p) / 1e3)
        for k in range(reps + 1):
            t0 = time.perf_counter()
            h.existence_csr_device(0, d_rows.data_ptr(), 0, 0)
            count_ms.append((time.perf_counter() - t0) * 1e3)
        for k in range(reps + 1):
            t0 = time.perf_counter()
            assert h.neighbors_device(edges, d_erows.data_ptr(), d_hits.data_ptr()) == edges
            nb_ms.append((time.perf_counter() - t0) * 1e3)
        deg = np.diff(d_erows.cpu().numpy().view(np.uint64).astype(np.int64))
        per_row = np.diff(d_rows.cpu().numpy().view(np.uint64).astype(np.int64))
        out.update(edges=edges, cells=cells, longest=int(deg.max()), most_cells=int(per_row.max()),
                   rows_above_8=int((deg > 8).sum()), rows_above_64=int((deg > 64).sum()),
                   existence_ms=ms[1:], count_only_ms=count_ms[1:], neighbors_ms=nb_ms[1:],
                   **{"%s_ms" % p: parts[p][1:] for p in PARTS})
        del d_hits, d_erows
    # the route that exists without the call: the dense table on the device, its nonzero cells picked out
    route = {"matrix": [], "nonzero": [], "all": []}
    with HipOverlap(dataclasses.replace(opt, existence=True)) as h:
        h.set_reference(s, s.longest)
        h.set_queries(s)
        d_m = torch.zeros((s.n, s.n_repertoires), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        for k in range(reps + 1):
            t0 = time.perf_counter()
            h.overlap_matrix_device(d_m.data_ptr())
            t1 = time.perf_counter()
            where = torch.nonzero(d_m)
            want_val = d_m[where[:, 0], where[:, 1]]
            want_rows = torch.zeros(s.n + 1, dtype=torch.int64, device="cuda")
            want_rows[1:] = torch.cumsum(torch.bincount(where[:, 0], minlength=s.n), 0)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if k:
                for name, dt in zip(("matrix", "nonzero", "all"), (t1 - t0, t2 - t1, t2 - t0)):
                    route[name].append(dt * 1e3)
        equal = (bool(torch.equal(want_rows, d_rows)) and len(where) == cells
                 and bool(torch.equal(where[:, 1].to(torch.int32), d_rep[:cells]))
                 and bool(torch.equal(want_val, d_val[:cells])))
    out.update(equal=equal, dense_bytes=s.n * s.n_repertoires * 8, **{"route_%s_ms" % k: v for k, v in route.items()})
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--reps-of-set", default="16,80", help="(b): repertoires of the set, one run each")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="(a): bench.py runs of each library")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "existence_timing"))
    ap.add_argument("--against", metavar="LIB", help="the parent commit's library")
    ap.add_argument("--measure", default="", metavar="N,R", help="(child) time one set size, print one JSON line")
    args = ap.parse_args()
    if args.measure:
        n, n_rep = (int(x) for x in args.measure.split(","))
        return measure(n, n_rep, args.reps)

    os.makedirs(args.out, exist_ok=True)
    lines = ["cmpr_existence_csr: the existing workload beside the parent commit, and the new call (tools/existence_timing.py)"]
    status = 0

    def flush():
        with open(os.path.join(args.out, "existence.txt"), "w") as fh:
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
        for n_rep in [int(x) for x in args.reps_of_set.split(",") if x]:
            p = subprocess.run(["timeout", "-k", "10", "400"] + me + ["--measure", "%d,%d" % (n, n_rep), "--reps", str(args.reps)],
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=timed_env)
            if p.returncode != 0:
                return failed("timing child (n = %d, %d repertoires)" % (n, n_rep), p)
            r = json.loads(p.stdout.decode().strip().splitlines()[-1])
            first = len(lines)
            lines.append("(b) n = %d CDR3aa in %d repertoires against themselves, d = 1: %d edges, longest row %d (rows above 8: "
                         "%d, above 64: %d), %d cells, most in a row %d; both routes equal: %s"
                         % (r["n"], r["repertoires"], r["edges"], r["longest"], r["rows_above_8"], r["rows_above_64"],
                            r["cells"], r["most_cells"], r["equal"]))
            lines.append("    cmpr_existence_csr_device, arrays in HBM, host ms per call (%d calls after a warm-up): %s"
                         % (len(r["existence_ms"]), spread(r["existence_ms"])))
            for part, what in zip(PARTS, ("edges (count, sum, fill)", "rows grouped", "cells summed", "cells reduced")):
                lines.append("      %-25s %s" % (what, spread(r["%s_ms" % part])))
            lines.append("    count-only call (row_start in HBM): %s" % spread(r["count_only_ms"]))
            lines.append("    cmpr_neighbors_device, same resident sets (the part that existed): %s" % spread(r["neighbors_ms"]))
            lines.append("    without it: a context with options.existence (%d bytes of matrix), cmpr_overlap_matrix_device %s"
                         % (r["dense_bytes"], spread(r["route_matrix_ms"])))
            lines.append("      torch.nonzero + gather + row sums %s" % spread(r["route_nonzero_ms"]))
            lines.append("      in all                            %s" % spread(r["route_all_ms"]))
            flush()
            print("\n".join(lines[first:]), flush=True)
            if not r["equal"]:
                lines.append("n = %d, %d repertoires: the two routes differ" % (n, n_rep))
                flush()
                return 1
    flush()
    print("\n".join(lines), flush=True)
    return status


if __name__ == "__main__":
    sys.exit(main())
