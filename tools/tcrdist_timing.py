#!/usr/bin/env python3
"""usage (GPU box): timeout 1100 python3 tools/tcrdist_timing.py [--against OTHER/libcompairr_hip.so]
                                                [--n 1000000] [--out build/tcrdist_timing]

What cmpr_tcrdist_neighbors_device costs, written to <out>/tcrdist.txt (the committed copy: profiles/rNN/tcrdist.txt).

  shapes  --n synth.make_set CDR3aa sequences against as many of another seed, V/J matched and with ignore_genes, the
          sets already in HBM, trims (3, 2), gap_penalty 12, a seeded symmetric table of costs 0, 3, 6, 9, 12 with a
          zero diagonal: cutoff 12 (partners |L - L'| <= 1) and cutoff 36 (|L - L'| <= 3), FIXED and SLIDING each;
          cmpr_tcrdist_neighbors_device count-only and with the exact capacity (hits and distances), --reps calls each
          after a warm-up call; the parts as the library clocks them (tunables tcrdist_{group,compare,order,copy}_us);
          the edges, the longest row, the pairs compared and pairs per second of one pass of the compare kernel;
  yardstick  the count-only cmpr_edit_neighbors_device call of the same build on the same sets in the same process at
          d = 1, respectively d = 3: it walks the same partner groups.  Per case: both medians, both spreads, and
          whether the tcrdist call's median lies above the edit call's by more than the two spreads (exit status 2);
  (a) bench.py's default `value` with this tree's library ("branch") and with --against LIB ("parent", the parent
      commit's build), alternately, --rounds runs each, as tools/edit_timing.py (a): exit status 2 when the branch's
      median falls below the parent's by more than the parent's own max - min.

Every step that uses the GPU is a child process under its own time limit; a step that fails ends the run."""

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
from edit_timing import median, pairs_of, sets_of, spread  # noqa: E402

PARTS = ("group", "compare", "order", "copy")
GAP = 12
CASES = [(12, 1, 0), (12, 1, 1), (36, 3, 0), (36, 3, 1)]      # (cutoff, the edit call's d, gap mode)


def table():
    rng = np.random.default_rng(5)
    W = rng.integers(1, 5, (20, 20))
    np.fill_diagonal(W, 0)
    return (3 * np.minimum(W, W.T)).astype(np.uint8)


def timed(h, family, call, reps):
    ms, parts = [], {p: [] for p in PARTS}
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
        for p in PARTS:
            parts[p].append(h.get_tunable("%s_%s_us" % (family, p)) / 1e3)
    return ms, parts


def measure(n, ignore_genes, reps):
    """(child) one JSON line: every case on one pair of sets, the edit yardstick beside each"""
    import torch
    from compairr_amd import HipOverlap, Options, TcrdistParams, synth
    a, b = sets_of(n, False, False)
    out = {"n": n, "g": ignore_genes, "cases": []}
    opt = Options(n_v_genes=synth.N_V, n_j_genes=synth.N_J, ignore_genes=ignore_genes, device=0)
    with HipOverlap(opt) as h:
        v1, keep1 = HipOverlap.device_view(a)
        v2, keep2 = HipOverlap.device_view(b)
        d_rows = torch.zeros(a.n + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        for cutoff, d, mode in CASES:
            p = TcrdistParams(table(), GAP, 3, 2, mode)
            r = {"cutoff": cutoff, "d": d, "mode": mode, "pairs": pairs_of(a, b, ignore_genes, d)[0]}
            count = lambda: h.tcrdist_neighbors_device(v1, v2, p, cutoff, 0, d_rows.data_ptr())
            edges = count()
            ms, parts = timed(h, "tcrdist", count, reps)
            r.update(edges=edges, count_only_ms=ms, count_only_compare_ms=parts["compare"],
                     count_only_group_ms=parts["group"])
            d_hits = torch.zeros(max(edges, 1), dtype=torch.int32, device="cuda")
            d_dist = torch.zeros(max(edges, 1), dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            ms, parts = timed(h, "tcrdist", lambda: h.tcrdist_neighbors_device(
                v1, v2, p, cutoff, edges, d_rows.data_ptr(), d_hits.data_ptr(), d_dist.data_ptr()), reps)
            r.update(neighbors_ms=ms, longest_row=int(torch.diff(d_rows).max().item()),
                     **{"neighbors_%s_ms" % k: v for k, v in parts.items()})
            del d_hits, d_dist
            edit = lambda: h.edit_neighbors_device(v1, v2, d, 0, d_rows.data_ptr())
            r["edit_edges"] = edit()
            ms, parts = timed(h, "edit", edit, reps)
            r.update(edit_count_only_ms=ms, edit_compare_ms=parts["compare"], edit_group_ms=parts["group"])
            out["cases"].append(r)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="(a): bench.py runs of each library")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "tcrdist_timing"))
    ap.add_argument("--against", metavar="LIB", help="the parent commit's library")
    ap.add_argument("--child", choices=("measure",))
    ap.add_argument("--g", type=int, default=0)
    args = ap.parse_args()
    if args.child == "measure":
        return measure(args.n, bool(args.g), args.reps)

    os.makedirs(args.out, exist_ok=True)
    lines = ["cmpr_tcrdist_*: the new calls beside cmpr_edit_neighbors_device, and the existing workload beside the "
             "parent commit (tools/tcrdist_timing.py)"]
    status = 0

    def flush():
        with open(os.path.join(args.out, "tcrdist.txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")

    def failed(what, p):
        lines.append("%s failed with %d: %s" % (what, p.returncode, p.stderr.decode(errors="replace")[-500:]))
        flush()
        print(lines[-1], flush=True)
        return p.returncode or 1

    branch_env = {k: v for k, v in os.environ.items() if k != "COMPAIRR_HIP_LIB"}

    for g in (0, 1):
        p = subprocess.run(["timeout", "-k", "10", "500", sys.executable, os.path.abspath(__file__), "--child", "measure",
                            "--n", str(args.n), "--g", str(g), "--reps", str(args.reps)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=branch_env)
        if p.returncode != 0:
            return failed("timing child (g = %d)" % g, p)
        first = len(lines)
        for r in json.loads(p.stdout.decode().strip().splitlines()[-1])["cases"]:
            lines.append("%d x %d CDR3aa%s, trims (3, 2), gap_penalty %d, cutoff %d, %s: %d pairs compared, %d edges, longest row %d"
                         % (args.n, args.n, ", ignore_genes" if g else "", GAP, r["cutoff"],
                            "SLIDING" if r["mode"] else "FIXED", r["pairs"], r["edges"], r["longest_row"]))
            lines.append("    cmpr_tcrdist_neighbors_device, sets in HBM, count-only, host ms per call (%d calls after a warm-up): %s"
                         % (len(r["count_only_ms"]), spread(r["count_only_ms"])))
            lines.append("      group    %s" % spread(r["count_only_group_ms"]))
            lines.append("      compare  %s" % spread(r["count_only_compare_ms"]))
            lines.append("      compare kernel, one pass: %.3g pairs/s"
                         % (r["pairs"] / (median(r["count_only_compare_ms"]) / 1e3)))
            lines.append("    cmpr_tcrdist_neighbors_device, exact capacity, hits and distances: %s" % spread(r["neighbors_ms"]))
            for part in PARTS[:3]:
                lines.append("      %-8s %s" % (part, spread(r["neighbors_%s_ms" % part])))
            lines.append("    yardstick: cmpr_edit_neighbors_device, count-only, d = %d, %d edges: %s"
                         % (r["d"], r["edit_edges"], spread(r["edit_count_only_ms"])))
            lines.append("      group    %s" % spread(r["edit_group_ms"]))
            lines.append("      compare  %s" % spread(r["edit_compare_ms"]))
            td, ed = r["count_only_ms"], r["edit_count_only_ms"]
            slower = median(td) > median(ed) + (max(td) - min(td)) + (max(ed) - min(ed))
            lines.append("    tcrdist median / edit median = %.3f: %s" % (median(td) / median(ed),
                         "SLOWER beyond the spread of the runs" if slower else "not slower"))
            if slower:
                status = 2
        flush()
        print("\n".join(lines[first:]), flush=True)

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
    print("\n".join(lines[-5:]), flush=True)
    return status


if __name__ == "__main__":
    sys.exit(main())
