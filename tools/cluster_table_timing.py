#!/usr/bin/env python3
"""usage (GPU box): timeout 1100 python3 tools/cluster_table_timing.py [--against OTHER/libcompairr_hip.so]
                        [--variant NAME=OTHER/libcompairr_hip.so] [--sizes 1000000,10000000] [--out build/cluster_table_timing]

What cmpr_cluster_table_device costs and gains, written to <out>/cluster_table.txt (the committed copy:
profiles/r13/cluster_table.txt).  Report only: nothing here is a threshold.

  (a) bench.py's default `value` (query sequences/s) with this tree's library ("branch") and with --against LIB
      (COMPAIRR_HIP_LIB; "parent", the parent commit's build), alternately, --rounds runs each: all values, the
      medians and the parent's own min-max spread (--rounds 0: skipped);
  (b) per size of --sizes, synth.make_set CDR3aa sequences (uniform law, as bench.py builds its sets; the sets of
      tools/cluster_timing.py) at d = 1, V/J matched, the set in device memory before the clock starts:
        * cmpr_cluster_table_device into arrays in HBM, host-clocked, and its two parts as the library clocks
          them (tunables cluster_links_us, cluster_table_us: host clock, each part ending in a wait);
        * the same table reached without it, on the --against library when one is given (this tree's otherwise):
          cmpr_cluster_device, then either labels and sizes to the host + numpy lexsort / stable argsort, or two
          stable torch.sort calls on the device -- each clocked from the end of cmpr_cluster_device;
        * --variant NAME=LIB (any number): the same call on another build of this tree's library -- how the
          one-sort variant of the pass, a build that is no longer in the tree, was measured once.
      Every route's four arrays are summarised by CRC-32 and must agree.

Every step that uses the GPU is a child process under its own time limit; a step that fails ends the run."""

import argparse
import json
import os
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else (xs[len(xs) // 2 - 1] + xs[len(xs) // 2]) / 2


def crc(arrays, k, n):
    """one word per array of a table: cluster_of[n], cluster_start[k + 1], members[n], count[k]"""
    return [zlib.crc32(np.ascontiguousarray(a[:m]).astype(t).tobytes())
            for a, m, t in zip(arrays, (n, k + 1, n, k), (np.uint32, np.uint64, np.uint32, np.uint64))]


def table_numpy(label, size, count):
    label = label.astype(np.int64)
    roots = np.flatnonzero(label == np.arange(len(label)))
    order = roots[np.lexsort((roots, -size[roots].astype(np.int64)))]
    number = np.empty(len(label), dtype=np.int64)
    number[order] = np.arange(len(order))
    cluster_of = number[label]
    members = np.argsort(cluster_of, kind="stable")
    cluster_start = np.concatenate([[0], np.cumsum(size[order].astype(np.int64))])
    return cluster_of, cluster_start, members, np.add.reduceat(count[members], cluster_start[:-1])


def table_torch(torch, d_label, d_size, d_count):
    label, size = d_label.long(), d_size.long()
    roots = torch.nonzero(label == torch.arange(len(label), device=label.device)).flatten()
    order = roots[torch.sort(-size[roots], stable=True).indices]
    number = torch.empty_like(label)
    number[order] = torch.arange(len(order), device=label.device)
    cluster_of = number[label]
    members = torch.sort(cluster_of, stable=True).indices
    cluster_start = torch.cat([torch.zeros(1, dtype=torch.long, device=label.device), torch.cumsum(size[order], 0)])
    sums = torch.zeros(len(order), dtype=torch.long, device=label.device).index_add_(0, cluster_of, d_count)
    torch.cuda.synchronize()
    return cluster_of, cluster_start, members, sums


def measure(n, reps, routes):
    """(child) one JSON line for one set size, on the library COMPAIRR_HIP_LIB names.  routes: the call itself
    ("call"), the compositions without it ("compose"), or both"""
    import torch
    from compairr_amd import HipOverlap, Options, synth
    opt = Options(differences=1, n_v_genes=synth.N_V, n_j_genes=synth.N_J, device=0)
    s = synth.make_set(n, 2, prefix="B", pool_size=n // 4)
    out = {"n": s.n}
    with HipOverlap(opt) as h:
        view, keep = HipOverlap.device_view(s)
        i32 = lambda m: torch.zeros(m, dtype=torch.int32, device="cuda")
        i64 = lambda m: torch.zeros(m, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        if "call" in routes:
            bufs = [i32(s.n), i64(s.n + 1), i32(s.n), i64(s.n)]
            ms, links, table = [], [], []
            for _ in range(reps + 1):              # (the first call is the warm-up one)
                t0 = time.perf_counter()
                k = h.cluster_table_device(view, *[b.data_ptr() for b in bufs])
                ms.append((time.perf_counter() - t0) * 1e3)
                links.append(h.get_tunable("cluster_links_us") / 1e3)
                table.append(h.get_tunable("cluster_table_us") / 1e3)
            arrays = [b.cpu().numpy() for b in bufs]
            out.update(clusters=k, largest=int(arrays[1][1]), call_ms=ms[1:], links_ms=links[1:], table_ms=table[1:],
                       call_crc=crc(arrays, k, s.n))
        if "compose" in routes:
            d_label, d_size = i32(s.n), i32(s.n)
            d_count = torch.from_numpy(s.count.astype(np.int64)).cuda()
            torch.cuda.synchronize()
            cluster_ms, numpy_ms, torch_ms = [], [], []
            for _ in range(reps + 1):
                t0 = time.perf_counter()
                k = h.cluster_device(view, d_label.data_ptr(), d_size.data_ptr())
                t1 = time.perf_counter()
                by_numpy = table_numpy(d_label.cpu().numpy().view(np.uint32), d_size.cpu().numpy().view(np.uint32), s.count)
                t2 = time.perf_counter()
                by_torch = table_torch(torch, d_label, d_size, d_count)
                t3 = time.perf_counter()
                cluster_ms.append((t1 - t0) * 1e3)
                numpy_ms.append((t2 - t1) * 1e3)
                torch_ms.append((t3 - t2) * 1e3)
            out.update(compose_clusters=k, cluster_ms=cluster_ms[1:], numpy_ms=numpy_ms[1:], torch_ms=torch_ms[1:],
                       numpy_crc=crc(by_numpy, k, s.n), torch_crc=crc([a.cpu().numpy() for a in by_torch], k, s.n))
        del keep
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="(a): bench.py runs of each library")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "cluster_table_timing"))
    ap.add_argument("--against", metavar="LIB", help="the parent commit's library")
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=LIB",
                    help="another build of this tree's library to time the call on (the one-sort variant of profiles/r13 was "
                         "such a build; its source is not in the repository, so that figure cannot be retaken from it)")
    ap.add_argument("--measure", type=int, default=0, metavar="N", help="(child) time one set size, print one JSON line")
    ap.add_argument("--routes", default="call,compose", help="(child) what to time")
    args = ap.parse_args()
    if args.measure:
        return measure(args.measure, args.reps, args.routes.split(","))

    os.makedirs(args.out, exist_ok=True)
    lines = ["cmpr_cluster_table: the existing workload beside the parent commit, and the new call (tools/cluster_table_timing.py)"]

    def flush():
        with open(os.path.join(args.out, "cluster_table.txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")

    def failed(what, p):
        lines.append("%s failed with %d: %s" % (what, p.returncode, p.stderr.decode(errors="replace")[-500:]))
        flush()
        print(lines[-1], flush=True)
        return p.returncode or 1

    def row(name, xs, digits=2):
        f = "%%.%df" % digits
        return "%s %s  median %s  min %s  max %s" % (name, " ".join(f % x for x in xs), f % median(xs), f % min(xs), f % max(xs))

    branch_env = {k: v for k, v in os.environ.items() if k != "COMPAIRR_HIP_LIB"}
    parent_env = dict(os.environ, COMPAIRR_HIP_LIB=os.path.abspath(args.against)) if args.against else None

    # (a) bench.py, parent and branch in turn
    if args.against and args.rounds:
        values = {"parent": [], "branch": []}
        for rnd in range(args.rounds):
            for side, env in (("parent", parent_env), ("branch", branch_env)):
                p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                                    "--steps", str(args.steps), "--warmup", str(args.warmup)],
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=ROOT)
                if p.returncode != 0:
                    return failed("bench.py (%s, round %d)" % (side, rnd), p)
                values[side].append(float(json.loads(p.stdout.decode().strip().splitlines()[-1])["value"]))
                print("%s round %d: %.4g" % (side, rnd, values[side][-1]), flush=True)
        pa, br = values["parent"], values["branch"]
        lines.append("(a) bench.py --gpus 1 --steps %d --warmup %d, `value` in query sequences/s, %d runs each in turn"
                     % (args.steps, args.warmup, args.rounds))
        for side, xs in (("parent", pa), ("branch", br)):
            lines.append("    %s: %s  median %.4g  min %.4g  max %.4g" % (side, " ".join("%.4g" % x for x in xs), median(xs), min(xs), max(xs)))
        lines.append("    branch median / parent median = %.4f; parent median - branch median = %.4g, parent max - min = %.4g"
                     % (median(br) / median(pa), median(pa) - median(br), max(pa) - min(pa)))
    else:
        lines.append("(a) not measured: no --against library, or --rounds 0")
    flush()

    # (b) the new call, the table without it, the variants
    me = [sys.executable, os.path.abspath(__file__)]

    def child(n, routes, env, what):
        p = subprocess.run(["timeout", "-k", "10", "500"] + me + ["--measure", str(n), "--reps", str(args.reps), "--routes", routes],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        if p.returncode != 0:
            failed("%s (n = %d)" % (what, n), p)
            return None
        return json.loads(p.stdout.decode().strip().splitlines()[-1])

    for n in [int(x) for x in args.sizes.split(",") if x]:
        r = child(n, "call", branch_env, "timing child")
        if r is None:
            return 1
        lines.append("(b) n = %d CDR3aa, d = 1: %d clusters, largest %d" % (r["n"], r["clusters"], r["largest"]))
        lines.append(row("    cmpr_cluster_table_device, arrays in HBM, host ms per call (%d calls after a warm-up):" % len(r["call_ms"]), r["call_ms"]))
        lines.append(row("      labels and sizes (set, layout, step, flatten, sizes) ", r["links_ms"]))
        lines.append(row("      the table (numbering, members, counts)               ", r["table_ms"]))
        o = child(n, "compose", parent_env or branch_env, "composition child")
        if o is None:
            return 1
        lines.append(row("    without it, on %s library: cmpr_cluster_device" % ("the parent's" if args.against else "this tree's"), o["cluster_ms"]))
        lines.append(row("      then labels, sizes to the host + numpy lexsort, stable argsort", o["numpy_ms"]))
        lines.append(row("      or two stable torch.sort on the device (+ nonzero, gathers)  ", o["torch_ms"]))
        equal = o["numpy_crc"] == r["call_crc"] and o["torch_crc"] == r["call_crc"] and o["compose_clusters"] == r["clusters"]
        lines.append("      the three tables are equal: %s" % equal)
        for spec in args.variant:
            name, lib = spec.split("=", 1)
            v = child(n, "call", dict(os.environ, COMPAIRR_HIP_LIB=os.path.abspath(lib)), "variant %s" % name)
            if v is None:
                return 1
            lines.append(row("    variant %s: the call" % name, v["call_ms"]))
            lines.append(row("      the table", v["table_ms"]))
            equal = equal and v["call_crc"] == r["call_crc"]
            lines.append("      equal to this tree's table: %s" % (v["call_crc"] == r["call_crc"]))
        flush()
        print("\n".join(lines), flush=True)
        if not equal:
            lines.append("n = %d: the routes differ" % n)
            flush()
            return 1
    flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
