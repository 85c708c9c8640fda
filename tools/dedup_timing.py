#!/usr/bin/env python3
"""usage (GPU box): timeout 1100 python3 tools/dedup_timing.py [--n 10000000] [--out build/dedup_timing]

What cmpr_deduplicate_device costs, written to <out>/dedup.txt (the committed copy: profiles/r08/dedup.txt):

  * two sets of --n sequences: synth.make_set as bench.py builds its reference set ("uniform"), and a copy in
    which 1 % of the sequences are one repeated clone ("skewed": every add of that class lands on one sum);
  * per set, after a warm-up call, the host-clocked time of five cmpr_deduplicate_device calls (the call ends
    in a synchronise) -- a child process of its own;
  * the per-kernel split of the same calls from a `rocprofv3 --kernel-trace --stats` run of its own;
  * the "Deduplicating:" phase of oracle/_ref/compairr -z on the same sets written as TSV (the reference is
    single-threaded there) -- the only yardstick there is.

Every step that uses the GPU is a child process under its own time limit; a step that fails ends the run."""

import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def build_sets(n):
    """[("uniform", set), ("skewed", set)]"""
    from compairr_amd import synth
    s = synth.make_set(n, 2, prefix="B", pool_size=n // 4)
    src = np.arange(n)
    clone = np.random.default_rng(8).choice(n, size=n // 100, replace=False)
    src[clone] = clone[0]
    skewed = s.subset(src)
    skewed.count = s.count.copy()
    return [("uniform", s), ("skewed", skewed)]


def measure(n, reps):
    """(child) one JSON line: per set the times of `reps` calls after a warm-up one"""
    import torch
    from compairr_amd import HipOverlap, Options, synth
    out = {}
    with HipOverlap(Options(n_v_genes=synth.N_V, n_j_genes=synth.N_J, device=0)) as h:
        for name, s in build_sets(n):
            view, keep = HipOverlap.device_view(s)
            d_first = torch.zeros(s.n, dtype=torch.int32, device="cuda")
            d_count = torch.zeros(s.n, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            unique, merged = h.deduplicate_device(view, s.n, d_first.data_ptr(), d_count.data_ptr())
            ms = []
            for _ in range(reps):
                t0 = time.perf_counter()
                h.deduplicate_device(view, s.n, d_first.data_ptr(), d_count.data_ptr())
                ms.append((time.perf_counter() - t0) * 1e3)
            heaviest = int(d_count.cpu().numpy().view(np.uint64).max())
            out[name] = {"n": s.n, "unique": unique, "merged": merged, "largest_count": heaviest, "ms": ms}
            del keep, d_first, d_count
    print(json.dumps(out))


def reference_phase(n, lines):
    """the reference's own clock around its loop over the sequences (dedup.cc:183-190)"""
    exe = os.path.join(ROOT, "oracle", "_ref", "compairr")
    if not os.path.exists(exe):
        lines.append("reference: oracle/_ref/compairr is missing -- not measured")
        return
    with tempfile.TemporaryDirectory() as tmp:
        for name, s in build_sets(n):
            tsv, log = os.path.join(tmp, name + ".tsv"), os.path.join(tmp, name + ".log")
            s.write_tsv_fast(tsv)
            t0 = time.perf_counter()
            p = subprocess.run([exe, "-z", tsv, "-o", os.devnull, "-l", log], stdout=subprocess.DEVNULL,
                               stderr=subprocess.DEVNULL, timeout=600)
            wall = time.perf_counter() - t0
            text = open(log, errors="replace").read() if os.path.exists(log) else ""
            m = re.search(r"Deduplicating:\s+100% \(([0-9.]+)s\)", text)
            d = re.search(r"Duplicates merged:\s+(\d+)", text)
            lines.append("reference %-8s rc %d  Deduplicating: %s s  merged %s  whole run %.1f s (1 thread)"
                         % (name, p.returncode, m.group(1) if m else "?", d.group(1) if d else "?", wall))
            print(lines[-1], flush=True)
            os.remove(tsv)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "dedup_timing"))
    ap.add_argument("--measure", action="store_true", help="(child) time the calls, print one JSON line")
    ap.add_argument("--no-reference", action="store_true")
    args = ap.parse_args()
    if args.measure:
        return measure(args.n, args.reps)

    os.makedirs(args.out, exist_ok=True)
    lines = ["cmpr_deduplicate_device, n = %d sequences per set (tools/dedup_timing.py)" % args.n]
    me = [sys.executable, os.path.abspath(__file__), "--measure", "--n", str(args.n)]

    def flush():
        with open(os.path.join(args.out, "dedup.txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")

    # 1. the host-clocked calls
    p = subprocess.run(["timeout", "-k", "10", "300"] + me + ["--reps", str(args.reps)], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    if p.returncode != 0:
        lines.append("timing child failed with %d: %s" % (p.returncode, p.stderr.decode(errors="replace")[-500:]))
        flush()
        return p.returncode
    got = json.loads(p.stdout.decode().strip().splitlines()[-1])
    for name, r in got.items():
        ms = sorted(r["ms"])
        lines.append("%-8s unique %d  merged %d  largest count %d" % (name, r["unique"], r["merged"], r["largest_count"]))
        lines.append("%-8s host-clocked ms per call, %d calls after a warm-up: %s  median %.2f"
                     % (name, len(ms), " ".join("%.2f" % x for x in r["ms"]), ms[len(ms) // 2]))
    flush()
    print("\n".join(lines), flush=True)

    # 2. the per-kernel split: a run of its own (2 sets x (1 warm-up + 2) calls)
    prof = os.path.join(args.out, "prof")
    p = subprocess.run(["timeout", "-k", "10", "400", "rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "p",
                        "--output-format", "csv", "--"] + me + ["--reps", "2"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=tempfile.gettempdir())
    if p.returncode != 0:
        lines.append("rocprofv3 run failed with %d: %s" % (p.returncode, p.stderr.decode(errors="replace")[-500:]))
        flush()
        return p.returncode
    lines.append("per kernel (rocprofv3 --kernel-trace --stats; both sets, 3 calls each):")
    for f in glob.glob(prof + "/**/*kernel_stats.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if "dedup_" in r["Name"] or "validate_" in r["Name"]:
                lines.append("  %-46s calls %3s  total %10.1f us  avg %9.1f us  min %9.1f  max %9.1f"
                             % (re.sub(r"\(.*", "", r["Name"])[-46:], r["Calls"], float(r["TotalDurationNs"]) / 1e3,
                                float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))
    # (the same run call by call: the first three calls are the uniform set's, the last three the skewed one's)
    for f in glob.glob(prof + "/**/*kernel_trace.csv", recursive=True):
        rows = list(csv.DictReader(open(f)))
        try:
            rows = sorted((r for r in rows if "dedup_" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
            calls = {}
            for r in rows:
                name = re.search(r"dedup_[a-z]+", r["Kernel_Name"]).group(0)
                calls.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
            for name, us in calls.items():
                lines.append("  %-22s us per call in order: %s" % (name, " ".join("%.1f" % x for x in us)))
        except (KeyError, AttributeError, ValueError):
            lines.append("  (kernel trace columns not as expected: %s)" % ",".join(rows[0].keys() if rows else []))
    flush()
    print("\n".join(lines[-12:]), flush=True)

    # 3. the reference on the CPU
    if not args.no_reference:
        reference_phase(args.n, lines)
    flush()
    print("\n".join(lines), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
