#!/usr/bin/env python3
"""usage (GPU box): timeout 1100 python3 tools/dedup_timing.py [--n 10000000] [--out build/dedup_timing]
                                                                 [--against OTHER/libcompairr_hip.so]

What cmpr_deduplicate_device and cmpr_count_duplicates cost, written to <out>/dedup.txt (the committed copy:
profiles/r09/dedup.txt):

  * two sets of --n sequences: synth.make_set as bench.py builds its reference set ("uniform"), and a copy in
    which 1 % of the sequences are one repeated clone ("skewed": every add of that class lands on one sum);
  * per set, after a warm-up call each, the host-clocked time of five calls (every call ends in a synchronise)
    of cmpr_deduplicate_device, of count_duplicates(set) on a context with no reference ("passed": the set is
    uploaded and indexed for the call) and of count_duplicates() after set_reference(set) ("resident":
    the lookups in the record table) -- a child process of its own;
  * the per-kernel split of the same calls from a `rocprofv3 --kernel-trace --stats` run of its own, and from
    its trace the kernel time of every call;
  * the "Deduplicating:" phase of oracle/_ref/compairr -z on the same sets written as TSV (the reference is
    single-threaded there) -- the only yardstick there is.

--against LIB runs every GPU step with that library too (COMPAIRR_HIP_LIB; "parent"), alternately with this
tree's ("branch"), --rounds times each, and writes <out>/duplicates.txt: all calls, medians, spreads and, per
row, whether the branch's median is at most the parent's median plus the parent's own spread (max - min over
its calls of all rounds) -- on shared machines that spread is the resolution there is.

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


def timed(reps, call):
    """ms of `reps` calls after a warm-up one, and the last result"""
    got = call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        got = call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms, got


def measure(n, reps):
    """(child) one JSON line: per set the times of `reps` calls of each kind after a warm-up one"""
    import torch
    from compairr_amd import HipOverlap, Options, synth
    opt = Options(n_v_genes=synth.N_V, n_j_genes=synth.N_J, device=0)
    out = {}
    for name, s in build_sets(n):
        with HipOverlap(opt) as h:
            view, keep = HipOverlap.device_view(s)
            d_first = torch.zeros(s.n, dtype=torch.int32, device="cuda")
            d_count = torch.zeros(s.n, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            ms, (unique, merged) = timed(reps, lambda: h.deduplicate_device(view, s.n, d_first.data_ptr(),
                                                                            d_count.data_ptr()))
            heaviest = int(d_count.cpu().numpy().view(np.uint64).max())
            del keep, d_first, d_count
            passed_ms, passed = timed(reps, lambda: h.count_duplicates(s))
        with HipOverlap(opt) as h:
            h.set_reference(s, s.longest)
            resident_ms, resident = timed(reps, lambda: h.count_duplicates())
        out[name] = {"n": s.n, "unique": unique, "merged": merged, "largest_count": heaviest, "ms": ms,
                     "passed": passed, "passed_ms": passed_ms, "resident": resident, "resident_ms": resident_ms}
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


KERNELS = ("dedup_", "count_duplicates", "build_index")
KINDS = (("dedup", "ms"), ("passed", "passed_ms"), ("resident", "resident_ms"))


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else (xs[len(xs) // 2 - 1] + xs[len(xs) // 2]) / 2


def kernel_calls(trace_csv, reps):
    """{(kind, set): [kernel us of each call after the warm-up one]} from a trace of measure(): the kernels
    of KERNELS in start order, cut into calls at the kernel each kind of call ends with"""
    rows = [r for r in csv.DictReader(open(trace_csv)) if any(k in r["Kernel_Name"] for k in KERNELS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [re.search(r"dedup_[a-z_]+|count_duplicates[a-z_]*|build_index[a-z_]*", r["Kernel_Name"]).group(0)
             for r in rows]
    calls = {"dedup": [], "passed": [], "resident": []}
    cur, us = [], 0.0
    for k, (r, name) in enumerate(zip(rows, names)):
        cur.append(name)
        us += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        last = name == "dedup_scatter_kernel" or name.startswith("count_duplicates") or \
            (name == "dedup_scan_kernel" and (k + 1 == len(names) or names[k + 1] != "dedup_scatter_kernel"))
        if last:
            kind = "dedup" if "dedup_scatter_kernel" in cur else \
                "resident" if all(x.startswith("count_duplicates") for x in cur) else "passed"
            calls[kind].append(us)
            cur, us = [], 0.0
    out = {}
    for kind, v in calls.items():
        if len(v) != 2 * (1 + reps):
            raise ValueError("%s: %d calls in the trace, expected %d" % (kind, len(v), 2 * (1 + reps)))
        out[(kind, "uniform")] = v[1:1 + reps]
        out[(kind, "skewed")] = v[2 + reps:]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "dedup_timing"))
    ap.add_argument("--measure", action="store_true", help="(child) time the calls, print one JSON line")
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--against", metavar="LIB", help="the library to compare with (the parent commit's)")
    ap.add_argument("--rounds", type=int, default=2, help="with --against: runs of each library")
    args = ap.parse_args()
    if args.measure:
        return measure(args.n, args.reps)

    os.makedirs(args.out, exist_ok=True)
    lines = ["cmpr_deduplicate_device and cmpr_count_duplicates, n = %d sequences per set (tools/dedup_timing.py)"
             % args.n]
    cmp_lines = ["cmpr_count_duplicates (and cmpr_deduplicate_device), parent against branch, n = %d sequences per "
                 "set, %d rounds in turn (tools/dedup_timing.py --against)" % (args.n, args.rounds)]
    me = [sys.executable, os.path.abspath(__file__), "--measure", "--n", str(args.n)]
    trace_reps = 2
    sides = [("parent", dict(os.environ, COMPAIRR_HIP_LIB=os.path.abspath(args.against)))] if args.against else []
    sides.append(("branch", {k: v for k, v in os.environ.items() if k != "COMPAIRR_HIP_LIB"}))
    runs = [(side, env, rnd) for rnd in range(args.rounds if args.against else 1) for side, env in sides]

    def flush():
        with open(os.path.join(args.out, "dedup.txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")
        if args.against:
            with open(os.path.join(args.out, "duplicates.txt"), "w") as fh:
                fh.write("\n".join(cmp_lines) + "\n")

    def failed(what, p):
        for out in (lines, cmp_lines):
            out.append("%s failed with %d: %s" % (what, p.returncode, p.stderr.decode(errors="replace")[-500:]))
        flush()
        print(lines[-1], flush=True)
        return p.returncode or 1

    # 1. the host-clocked calls
    host = {}                              # (side, kind, set) -> ms of all rounds
    for side, env, rnd in runs:
        p = subprocess.run(["timeout", "-k", "10", "400"] + me + ["--reps", str(args.reps)], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, env=env)
        if p.returncode != 0:
            return failed("timing child (%s, round %d)" % (side, rnd), p)
        got = json.loads(p.stdout.decode().strip().splitlines()[-1])
        for name, r in got.items():
            if r["passed"] != r["merged"] or r["resident"] != r["merged"]:
                return failed("%s: merged %d, count_duplicates(set) %d, count_duplicates() %d -- they differ; run"
                              % (name, r["merged"], r["passed"], r["resident"]), p)
            for kind, key in KINDS:
                host.setdefault((side, kind, name), []).extend(r[key])
                cmp_lines.append("%-6s round %d  %-8s %-8s host ms: %s"
                                 % (side, rnd, kind, name, " ".join("%.2f" % x for x in r[key])))
            if side == "branch" and rnd == 0:
                lines.append("%-8s unique %d  merged %d  largest count %d  count_duplicates: passed-in %d, resident %d"
                             % (name, r["unique"], r["merged"], r["largest_count"], r["passed"], r["resident"]))
                for kind, key in KINDS:
                    lines.append("%-8s %-8s host-clocked ms per call, %d calls after a warm-up: %s  median %.2f"
                                 % (name, kind, len(r[key]), " ".join("%.2f" % x for x in r[key]), median(r[key])))
        flush()
        print("%s round %d timed" % (side, rnd), flush=True)

    # 2. the per-kernel split: runs of their own (2 sets x 3 kinds x (1 warm-up + 2) calls)
    kern = {}                              # (side, kind, set) -> kernel us per call, all rounds
    for side, env, rnd in runs:
        prof = os.path.join(args.out, "prof_%s_%d" % (side, rnd))
        p = subprocess.run(["timeout", "-k", "10", "500", "rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "p",
                            "--output-format", "csv", "--"] + me + ["--reps", str(trace_reps)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=tempfile.gettempdir(), env=env)
        if p.returncode != 0:
            return failed("rocprofv3 run (%s, round %d)" % (side, rnd), p)
        stats = ["per kernel (rocprofv3 --kernel-trace --stats; %s, round %d; both sets, 3 calls of each kind):" % (side, rnd)]
        for f in glob.glob(prof + "/**/*kernel_stats.csv", recursive=True):
            for r in csv.DictReader(open(f)):
                if any(k in r["Name"] for k in KERNELS + ("validate_",)):
                    stats.append("  %-46s calls %3s  total %10.1f us  avg %9.1f us  min %9.1f  max %9.1f"
                                 % (re.sub(r"\(.*", "", r["Name"])[-46:], r["Calls"], float(r["TotalDurationNs"]) / 1e3,
                                    float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))
        for f in glob.glob(prof + "/**/*kernel_trace.csv", recursive=True):
            try:
                for (kind, name), us in kernel_calls(f, trace_reps).items():
                    kern.setdefault((side, kind, name), []).extend(us)
                    stats.append("  %-8s %-8s kernel us per call: %s" % (kind, name, " ".join("%.1f" % x for x in us)))
            except (KeyError, AttributeError, ValueError) as e:
                stats.append("  (kernel trace not as expected: %s)" % e)
        cmp_lines.extend(stats)
        if side == "branch" and rnd == 0:
            lines.extend(stats)
        flush()
        print("%s round %d traced" % (side, rnd), flush=True)

    # 3. the gate
    if args.against:
        cmp_lines.append("gate: branch median <= parent median + parent spread (max - min of its calls, all rounds)")
        for what, data, unit in (("host", host, "ms"), ("kernels", kern, "us")):
            for kind, _ in KINDS:
                for name in ("uniform", "skewed"):
                    pa, br = data.get(("parent", kind, name)), data.get(("branch", kind, name))
                    if not pa or not br:
                        cmp_lines.append("%-8s %-8s %-8s not measured" % (what, kind, name))
                        continue
                    spread = max(pa) - min(pa)
                    cmp_lines.append("%-8s %-8s %-8s parent median %.2f spread %.2f (%d calls) | branch median %.2f "
                                     "spread %.2f (%d calls) %s: %s"
                                     % (what, kind, name, median(pa), spread, len(pa), median(br), max(br) - min(br),
                                        len(br), unit, "PASS" if median(br) <= median(pa) + spread else "FAIL"))
        flush()
        print("\n".join(cmp_lines), flush=True)

    # 4. the reference on the CPU
    if not args.no_reference:
        reference_phase(args.n, lines)
    flush()
    print("\n".join(lines), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
