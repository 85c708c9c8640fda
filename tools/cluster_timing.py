#!/usr/bin/env python3
"""usage (GPU box): timeout 1100 python3 tools/cluster_timing.py [--against OTHER/libcompairr_hip.so]
                                                  [--sizes 1000000,10000000] [--out build/cluster_timing]

What the link branch in score_match costs the existing workload and what cmpr_cluster_device gains, written to
<out>/cluster.txt (the committed copy: profiles/r10/cluster.txt).  Report only: nothing here is a threshold
but the comparison of (a).

  (a) bench.py's default `value` (query sequences/s) with this tree's library ("branch") and with --against LIB
      (COMPAIRR_HIP_LIB; "parent", the parent commit's build), alternately, --rounds runs each: all values,
      the medians, the parent's own min-max spread, and whether the branch's median lies below the parent's
      minimum -- outside the spread on the slow side;
  (b) per size of --sizes, synth.make_set CDR3aa sequences (uniform law, as bench.py builds its sets) at
      d = 1, V/J matched:
        * cmpr_cluster_device end to end, host-clocked (index + layout + link-mode step + labels; the set is
          in device memory before the clock starts), against the only route to the same labels without it:
          set_reference + set_queries + cmpr_overlap_pairs into host arrays + a numpy union-find
          (min-label propagation with pointer jumping) -- also clocked in its parts; the labels must be equal;
        * the link-mode step against the pairs-mode step of the same resident sets, HIP events
          (cmpr_get_kernel_times: kernel_ms of the last call).

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


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else (xs[len(xs) // 2 - 1] + xs[len(xs) // 2]) / 2


def labels_of_pairs(n, q, h):
    """label[i] = the smallest number of i's component under the edges (q[k], h[k])"""
    q, h = q.astype(np.int64), h.astype(np.int64)
    keep = q > h                               # (every pair is listed from both sides; identity pairs say nothing)
    q, h = q[keep], h[keep]
    label = np.arange(n, dtype=np.int64)
    while True:
        new = label.copy()
        np.minimum.at(new, q, label[h])
        np.minimum.at(new, h, label[q])
        while True:
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, label):
            return label.astype(np.uint32)
        label = new


def measure(n, reps):
    """(child) one JSON line for one set size"""
    import ctypes as C
    import torch
    from compairr_amd import HipOverlap, Options, synth
    opt = Options(differences=1, n_v_genes=synth.N_V, n_j_genes=synth.N_J, device=0)
    s = synth.make_set(n, 2, prefix="B", pool_size=n // 4)
    out = {"n": s.n}
    with HipOverlap(opt) as h:
        view, keep = HipOverlap.device_view(s)
        d_label = torch.zeros(s.n, dtype=torch.int32, device="cuda")
        d_size = torch.zeros(s.n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ms, link_ms = [], []
        for k in range(reps + 1):              # (the first call is the warm-up one)
            t0 = time.perf_counter()
            clusters = h.cluster_device(view, d_label.data_ptr(), d_size.data_ptr())
            ms.append((time.perf_counter() - t0) * 1e3)
            link_ms.append(h.kernel_times(1)[0][-1])
        label = d_label.cpu().numpy().view(np.uint32)
        out.update(clusters=clusters, largest=int(d_size.max().item()), cluster_ms=ms[1:], link_step_ms=link_ms[1:])
        # the pairs-mode step of the same resident sets (counting only: the list's size)
        count = C.c_uint64()
        pair_ms = []
        for k in range(reps + 1):
            h._check(h._lib.cmpr_overlap_pairs(h._ctx, 0, None, None, C.byref(count)))
            pair_ms.append(h.kernel_times(1)[0][-1])
        out.update(pairs=count.value, pairs_step_ms=pair_ms[1:])
        del keep
    # the route without cmpr_cluster, on a context of its own
    with HipOverlap(opt) as h:
        t0 = time.perf_counter()
        h.set_reference(s, s.longest)
        h.set_queries(s)
        t1 = time.perf_counter()
        npairs = C.c_uint64()
        h._check(h._lib.cmpr_overlap_pairs(h._ctx, 0, None, None, C.byref(npairs)))
        q = np.zeros(npairs.value, dtype=np.uint32)
        hit = np.zeros(npairs.value, dtype=np.uint32)
        h._check(h._lib.cmpr_overlap_pairs(h._ctx, npairs.value, q.ctypes.data, hit.ctypes.data, C.byref(npairs)))
        t2 = time.perf_counter()
        want = labels_of_pairs(s.n, q, hit)
        t3 = time.perf_counter()
    out.update(route_sets_ms=(t1 - t0) * 1e3, route_pairs_ms=(t2 - t1) * 1e3, route_union_ms=(t3 - t2) * 1e3,
               route_ms=(t3 - t0) * 1e3, pair_list_bytes=int(8 * npairs.value), labels_equal=bool(np.array_equal(label, want)))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="(a): bench.py runs of each library")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "cluster_timing"))
    ap.add_argument("--against", metavar="LIB", help="the parent commit's library")
    ap.add_argument("--measure", type=int, default=0, metavar="N", help="(child) time one set size, print one JSON line")
    args = ap.parse_args()
    if args.measure:
        return measure(args.measure, args.reps)

    os.makedirs(args.out, exist_ok=True)
    lines = ["cmpr_cluster: cost to the existing workload and the new call (tools/cluster_timing.py)"]

    def flush():
        with open(os.path.join(args.out, "cluster.txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")

    def failed(what, p):
        lines.append("%s failed with %d: %s" % (what, p.returncode, p.stderr.decode(errors="replace")[-500:]))
        flush()
        print(lines[-1], flush=True)
        return p.returncode or 1

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
        lines.append("(a) bench.py --gpus 1 --steps %d --warmup %d, `value` in query sequences/s, %d runs each in turn"
                     % (args.steps, args.warmup, args.rounds))
        lines.append("    parent: %s  median %.4g  min %.4g  max %.4g" % (" ".join("%.4g" % x for x in pa), median(pa), min(pa), max(pa)))
        lines.append("    branch: %s  median %.4g  min %.4g  max %.4g" % (" ".join("%.4g" % x for x in br), median(br), min(br), max(br)))
        lines.append("    branch median / parent median = %.4f; branch median %s the parent's min-max spread%s"
                     % (median(br) / median(pa), "below" if median(br) < min(pa) else "inside or above",
                        " -- SLOWER: move the link branch out of the matrix instantiations" if median(br) < min(pa) else ""))
    else:
        lines.append("(a) not measured: no --against library")
    flush()

    # (b) the new call
    me = [sys.executable, os.path.abspath(__file__)]
    for n in [int(x) for x in args.sizes.split(",") if x]:
        p = subprocess.run(["timeout", "-k", "10", "500"] + me + ["--measure", str(n), "--reps", str(args.reps)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=branch_env)
        if p.returncode != 0:
            return failed("timing child (n = %d)" % n, p)
        r = json.loads(p.stdout.decode().strip().splitlines()[-1])
        lines.append("(b) n = %d CDR3aa, d = 1: %d clusters, largest %d, %d pairs (a list of %.1f MB on the device and again "
                     "on the host); labels equal: %s"
                     % (r["n"], r["clusters"], r["largest"], r["pairs"], r["pair_list_bytes"] / 1e6, r["labels_equal"]))
        lines.append("    cmpr_cluster_device end to end, host ms per call (%d calls after a warm-up): %s  median %.1f"
                     % (len(r["cluster_ms"]), " ".join("%.1f" % x for x in r["cluster_ms"]), median(r["cluster_ms"])))
        lines.append("    without it: set_reference + set_queries %.1f ms, cmpr_overlap_pairs (count, then list to the host) "
                     "%.1f ms, numpy union-find %.1f ms: %.1f ms in all (one cold call)"
                     % (r["route_sets_ms"], r["route_pairs_ms"], r["route_union_ms"], r["route_ms"]))
        lines.append("    step, HIP events (kernel_ms): link mode %s  median %.3f | pairs mode (counting) %s  median %.3f"
                     % (" ".join("%.3f" % x for x in r["link_step_ms"]), median(r["link_step_ms"]),
                        " ".join("%.3f" % x for x in r["pairs_step_ms"]), median(r["pairs_step_ms"])))
        flush()
        print("\n".join(lines[-4:]), flush=True)
        if not r["labels_equal"]:
            lines.append("n = %d: the labels of the two routes differ" % n)
            flush()
            return 1
    flush()
    print("\n".join(lines), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
