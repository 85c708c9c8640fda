#!/usr/bin/env python3
"""usage (GPU box): timeout 1100 python3 tools/hamming_timing.py [--against OTHER/libcompairr_hip.so]
                                                [--n 1000000] [--out build/hamming_timing]

What cmpr_hamming_neighbors_device and cmpr_hamming_matrix_device cost, written to <out>/hamming.txt (the committed
copy: profiles/r16/hamming.txt).  The one condition is that of (a); the rest is a report.

  (a) bench.py's default `value` (query sequences/s) with this tree's library ("branch") and with --against LIB
      ("parent", the parent commit's build), alternately, --rounds runs each: all values, the medians, the parent's
      own max - min, and whether the branch's median falls below the parent's median by more than that (exit status
      2 when it does: no hot-path file changed, so that would be a finding);
  (b) --n synth.make_set CDR3aa sequences against as many of another seed at d = 3 and d = 5, with and without
      ignore_genes, and --nt-n nucleotide sequences at d = 4 with ignore_genes, the sets already in HBM:
        * cmpr_hamming_matrix_device and cmpr_hamming_neighbors_device (count-only call, then the exact capacity),
          host clock around the synchronous calls, --reps calls after a warm-up one, and the parts as the library
          clocks them (tunables hamming_{group,compare,copy}_us);
        * the pairs compared (the sum over the matched groups of queries x references), pairs per second of the
          compare kernel -- the matrix call's compare part, one pass --, and that rate as a fraction of the
          vector-issue peak as bench.py defines it (SIMDs x clock / 2 wave-instructions per second), with the
          instruction count per (wave, reference) read from the disassembly: 4 per packed word (xor, add or shift,
          and, popcount-accumulate) + 2 (the LDS address, the comparison with d), for amino acids and nucleotides;
  (c) the reference, `compairr -m -d 3` on --ref-n sequences of the same generator per set (a bounded sample: its
      all-against-all path takes hours at --n), wall clock, --threads threads, beside the library on the same sample;
  (d) d = 1 and d = 2 on the --n set against itself: the Hamming call beside cmpr_neighbors_distance_device,
      the index build and the query layout the hashed path needs included.  Recorded; nothing is re-routed.

Every step that uses the GPU is a child process under its own time limit; a step that fails ends the run."""

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

PARTS = ("group", "compare", "copy")
SIMDS, CLOCK_HZ = 1024, 2.4e9                       # 256 CUs x 4 SIMDs; the nominal clock (bench.py's calibration)
VALU_PEAK = SIMDS * CLOCK_HZ / 2.0                  # wave-instructions per second
REG_FORMS = (1, 2, 3, 4, 5, 6, 8, 12, 16)           # words per sequence the register form is compiled for


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else (xs[len(xs) // 2 - 1] + xs[len(xs) // 2]) / 2


def spread(xs):
    return "%s  median %.2f  min %.2f  max %.2f" % (" ".join("%.2f" % x for x in xs), median(xs), min(xs), max(xs))


def work_of(s1, s2, ignore_genes, per_word):
    """(pairs compared, wave-instructions of the compare kernel's inner loop) from the group sizes"""
    def keys(s):
        k = s.lengths.astype(np.int64)
        return k if ignore_genes else (k * 4096 + s.v_gene) * 4096 + s.j_gene
    k1, c1 = np.unique(keys(s1), return_counts=True)
    k2, c2 = np.unique(keys(s2), return_counts=True)
    common, i1, i2 = np.intersect1d(k1, k2, return_indices=True)
    lens = common if ignore_genes else common // (4096 * 4096)
    words = np.maximum(1, (lens + per_word - 1) // per_word)
    forms = np.array([next((f for f in REG_FORMS if w <= f), w) for w in words.tolist()], dtype=np.int64)
    pairs = c1[i1].astype(np.int64) * c2[i2]
    waves = ((c1[i1] + 63) // 64).astype(np.int64) * c2[i2]
    return int(pairs.sum()), int((waves * (4 * forms + 2)).sum())


def timed(h, call, reps):
    ms, parts = [], {p: [] for p in PARTS}
    for k in range(reps + 1):                      # (the first call is the warm-up one)
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
        for p in PARTS:
            parts[p].append(h.get_tunable("hamming_%s_us" % p) / 1e3)
    return ms[1:], {p: v[1:] for p, v in parts.items()}


def sets_of(n, nucleotides, same):
    from compairr_amd import synth
    a = synth.make_set(n, 1, prefix="A", pool_size=n // 4, nucleotides=nucleotides)
    return a, (a if same else synth.make_set(n, 2, prefix="B", pool_size=n // 4, nucleotides=nucleotides))


def measure(n, d, ignore_genes, nucleotides, reps):
    """(child) one JSON line: both device calls on one pair of sets"""
    import torch
    from compairr_amd import HipOverlap, Options, synth
    a, b = sets_of(n, nucleotides, False)
    pairs, insts = work_of(a, b, ignore_genes, 16 if nucleotides else 4)
    out = {"n": n, "d": d, "g": ignore_genes, "nt": nucleotides, "pairs": pairs, "insts": insts}
    opt = Options(n_v_genes=synth.N_V, n_j_genes=synth.N_J, ignore_genes=ignore_genes, nucleotides=nucleotides, device=0)
    with HipOverlap(opt) as h:
        v1, keep1 = HipOverlap.device_view(a)
        v2, keep2 = HipOverlap.device_view(b)
        d_mat = torch.zeros(a.n_repertoires * b.n_repertoires, dtype=torch.int64, device="cuda")
        d_rows = torch.zeros(a.n + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ms, parts = timed(h, lambda: h.hamming_matrix_device(v1, v2, d, d_mat.data_ptr()), reps)
        out.update(matrix_ms=ms, matrix_sum=int(d_mat.cpu().numpy().view(np.uint64).sum(dtype=np.uint64)),
                   **{"matrix_%s_ms" % p: v for p, v in parts.items()})
        edges = h.hamming_neighbors_device(v1, v2, d, 0, d_rows.data_ptr())
        ms, parts = timed(h, lambda: h.hamming_neighbors_device(v1, v2, d, 0, d_rows.data_ptr()), reps)
        out.update(edges=edges, count_only_ms=ms)
        d_hits = torch.zeros(max(edges, 1), dtype=torch.int32, device="cuda")
        d_dist = torch.zeros(max(edges, 1), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        ms, parts = timed(h, lambda: h.hamming_neighbors_device(v1, v2, d, edges, d_rows.data_ptr(), d_hits.data_ptr(),
                                                                 d_dist.data_ptr()), reps)
        hist = torch.bincount(d_dist[:edges].to(torch.int64), minlength=d + 1).cpu().tolist() if edges else []
        out.update(neighbors_ms=ms, histogram=hist, longest_row=int(torch.diff(d_rows).max().item()),
                   **{"neighbors_%s_ms" % p: v for p, v in parts.items()})
    print(json.dumps(out))


def measure_reference(n, threads, reps):
    """(child) one JSON line: the reference binary on a bounded sample, the library on the same sample"""
    from compairr_amd import HipOverlap, Options, synth
    exe = os.path.join(ROOT, "oracle", "_ref", "compairr")
    a, b = sets_of(n, False, False)
    out = {"n": n, "threads": threads}
    with HipOverlap(Options(n_v_genes=synth.N_V, n_j_genes=synth.N_J, device=0)) as h:
        ms, parts = timed(h, lambda: h.hamming_matrix(a, b, 3), reps)
        got = h.hamming_matrix(a, b, 3)
    out.update(library_ms=ms, library_compare_ms=parts["compare"], library_group_ms=parts["group"])
    if not os.path.exists(exe):
        print(json.dumps(dict(out, missing=True)))
        return
    with tempfile.TemporaryDirectory() as tmp:
        fa, fb, fo = (os.path.join(tmp, x) for x in ("a.tsv", "b.tsv", "out.tsv"))
        a.write_tsv_fast(fa)
        b.write_tsv_fast(fb)
        t0 = time.perf_counter()
        p = subprocess.run([exe, "-m", fa, fb, "-d", "3", "-t", str(threads), "-o", fo, "-l", os.devnull],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        out["reference_s"] = time.perf_counter() - t0
        if p.returncode != 0:
            print(json.dumps(dict(out, failed=p.stderr.decode(errors="replace")[-300:])))
            return
        with open(fo) as fh:
            lines = fh.read().splitlines()
    cols = lines[0].split("\t")[1:]
    equal = True
    for line in lines[1:]:
        f = line.split("\t")
        for c, text in zip(cols, f[1:]):
            equal &= "%.10g" % float(got[a.repertoire_ids.index(f[0]), b.repertoire_ids.index(c)]) == text
    print(json.dumps(dict(out, equal=bool(equal))))


def measure_crossover(n, d, reps):
    """(child) one JSON line: the Hamming call beside the hashed path on one set against itself at d = 1 or 2"""
    import torch
    from compairr_amd import HipOverlap, Options, synth
    a, _ = sets_of(n, False, True)
    out = {"n": n, "d": d}
    opt = Options(differences=d, n_v_genes=synth.N_V, n_j_genes=synth.N_J, device=0)
    d_rows = torch.zeros(a.n + 1, dtype=torch.int64, device="cuda")
    hashed, hamming = [], []
    for k in range(reps + 1):
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
            want = d_hits.clone()
            t0 = time.perf_counter()
            e2 = h.hamming_neighbors_device(v, v, d, 0, d_rows.data_ptr())
            d_hits2 = torch.zeros(max(e2, 1), dtype=torch.int32, device="cuda")
            d_dist2 = torch.zeros(max(e2, 1), dtype=torch.int16, device="cuda")
            h.hamming_neighbors_device(v, v, d, e2, d_rows.data_ptr(), d_hits2.data_ptr(), d_dist2.data_ptr())
            torch.cuda.synchronize()
            hamming.append((time.perf_counter() - t0) * 1e3)
            out.update(edges=edges, equal=bool(e2 == edges and torch.equal(want, d_hits2)
                                               and torch.equal(d_dist.to(torch.int16), d_dist2)))
    out.update(hashed_ms=hashed[1:], hamming_ms=hamming[1:])
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nt-n", type=int, default=100_000)
    ap.add_argument("--ref-n", type=int, default=50_000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="(a): bench.py runs of each library")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "hamming_timing"))
    ap.add_argument("--against", metavar="LIB", help="the parent commit's library")
    ap.add_argument("--child", choices=("measure", "reference", "crossover"))
    ap.add_argument("--d", type=int, default=3)
    ap.add_argument("--g", type=int, default=0)
    ap.add_argument("--nt", type=int, default=0)
    args = ap.parse_args()
    if args.child == "measure":
        return measure(args.n, args.d, bool(args.g), bool(args.nt), args.reps)
    if args.child == "reference":
        return measure_reference(args.n, args.threads, args.reps)
    if args.child == "crossover":
        return measure_crossover(args.n, args.d, args.reps)

    os.makedirs(args.out, exist_ok=True)
    lines = ["cmpr_hamming_*: the existing workload beside the parent commit, and the new calls (tools/hamming_timing.py)"]
    status = 0

    def flush():
        with open(os.path.join(args.out, "hamming.txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")

    def failed(what, p):
        lines.append("%s failed with %d: %s" % (what, p.returncode, p.stderr.decode(errors="replace")[-500:]))
        flush()
        print(lines[-1], flush=True)
        return p.returncode or 1

    def child(limit, *extra):
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--reps",
                            str(args.reps)] + [str(x) for x in extra], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=branch_env)
        return p, (json.loads(p.stdout.decode().strip().splitlines()[-1]) if p.returncode == 0 else None)

    branch_env = {k: v for k, v in os.environ.items() if k != "COMPAIRR_HIP_LIB"}

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

    # (b) the new calls
    cases = [(args.n, d, g, 0) for d in (3, 5) for g in (0, 1)] + [(args.nt_n, 4, 1, 1)]
    for n, d, g, nt in cases:
        p, r = child(500, "--child", "measure", "--n", n, "--d", d, "--g", g, "--nt", nt)
        if r is None:
            return failed("timing child (n = %d, d = %d, g = %d, nt = %d)" % (n, d, g, nt), p)
        first = len(lines)
        kernel_s = median(r["matrix_compare_ms"]) / 1e3
        lines.append("(b) %d x %d %s, d = %d%s: %d pairs compared, %d edges, longest row %d, distances %s"
                     % (n, n, "nucleotide sequences" if nt else "CDR3aa", d, ", ignore_genes" if g else "", r["pairs"],
                        r["edges"], r["longest_row"], r["histogram"]))
        lines.append("    cmpr_hamming_matrix_device, sets in HBM, host ms per call (%d calls after a warm-up): %s"
                     % (len(r["matrix_ms"]), spread(r["matrix_ms"])))
        for part in PARTS[:2]:
            lines.append("      %-8s %s" % (part, spread(r["matrix_%s_ms" % part])))
        lines.append("      compare kernel, one pass: %.3g pairs/s; %d wave-instructions of the inner loop = %.3g /s = %.3f "
                     "of the vector-issue peak (%.4g /s)" % (r["pairs"] / kernel_s, r["insts"], r["insts"] / kernel_s,
                                                              r["insts"] / kernel_s / VALU_PEAK, VALU_PEAK))
        lines.append("    cmpr_hamming_neighbors_device, count-only: %s" % spread(r["count_only_ms"]))
        lines.append("    cmpr_hamming_neighbors_device, exact capacity, hits and distances: %s" % spread(r["neighbors_ms"]))
        for part in PARTS[:2]:
            lines.append("      %-8s %s" % (part, spread(r["neighbors_%s_ms" % part])))
        flush()
        print("\n".join(lines[first:]), flush=True)

    # (c) the reference on a bounded sample
    p, r = child(900, "--child", "reference", "--n", args.ref_n, "--threads", args.threads)
    if r is None:
        return failed("reference child", p)
    first = len(lines)
    if r.get("missing"):
        lines.append("(c) not measured: oracle/_ref/compairr is not built")
    elif r.get("failed"):
        lines.append("(c) the reference failed: %s" % r["failed"])
    else:
        lines.append("(c) SAMPLE of %d x %d CDR3aa, d = 3: reference `compairr -m -d 3 -t %d`, wall clock with parsing: %.1f s; "
                     "cells equal to the library's: %s" % (r["n"], r["n"], r["threads"], r["reference_s"], r["equal"]))
        lines.append("    cmpr_hamming_matrix (host variant, upload included) on the same sample, ms: %s" % spread(r["library_ms"]))
        lines.append("      group %s" % spread(r["library_group_ms"]))
        lines.append("      compare %s" % spread(r["library_compare_ms"]))
    flush()
    print("\n".join(lines[first:]), flush=True)

    # (d) the crossover with the hashed path
    for d in (1, 2):
        p, r = child(500, "--child", "crossover", "--n", args.n, "--d", d)
        if r is None:
            return failed("crossover child (d = %d)" % d, p)
        first = len(lines)
        lines.append("(d) %d CDR3aa against themselves, d = %d, %d edges; the two CSRs equal: %s" % (r["n"], d, r["edges"], r["equal"]))
        lines.append("    cmpr_set_reference_device + cmpr_set_queries_device + cmpr_neighbors_distance_device (count, then fill), ms: %s"
                     % spread(r["hashed_ms"]))
        lines.append("    cmpr_hamming_neighbors_device (count, then fill), ms: %s" % spread(r["hamming_ms"]))
        flush()
        print("\n".join(lines[first:]), flush=True)
    flush()
    return status


if __name__ == "__main__":
    sys.exit(main())
